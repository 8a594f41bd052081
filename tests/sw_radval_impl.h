/* tests/sw_radval_impl.h -- TEST INFRASTRUCTURE ONLY.  Plain-C restatement of what the reference's rrtmg_sw computes for its
 * SOLAR_RADVAL dummy arguments, statement by statement (SW = GEOSsolar_GridComp/RRTMG/rrtmg_sw/gcm_model/src):
 *   SW/rrtmg_sw_cldprmc.F90:131-411   cldprmc_sw with the phase-split arrays of its #ifdef SOLAR_RADVAL sections (:321-351, :394-410)
 *   SW/rrtmg_sw_spcvmc.F90:676-746    zeroing, :749-1109 the accumulation over the PAR sub-columns
 *   SW/rrtmg_sw_rad.F90:893-1127      solar variability scalars (isolvar -1, 0, 2, 3 with the optional arguments absent),
 *                                     :1540-1590 zeros for cloud-free columns, :1658-1720 the sums of the cloudy ones
 * It reuses the oracle's pinned helpers for everything up to the cloud optics (sub-column generator, clearCounts, setcoef_sw,
 * taumol_sw's solar source) and restates the rest here; nothing in it comes from the GPU kernels.  Included twice by sw_radval_ref.c.
 * rrtmg_sw_spcvmc.F90 and rrtmg_sw_rad.F90 need ESMF / MAPL, so - as for the oracle's own spcvmc - the reference cannot be run for this.
 */
#define RVNG 112
#define RVLIN(tab, n1, i, ig, f) (F2(tab, n1, i, ig) + (f) * (F2(tab, n1, (i) + 1, ig) - F2(tab, n1, i, ig)))
#define RV_NCELL 14      /* ltaor lomor lasor ltauc lomgc lasyc forwliq | itaor iomor iasor itauc iomgc iasyc forwice */

/* cldprmc_sw for ONE column with the SOLAR_RADVAL arrays.  comb[4] = taormc taucmc ssacmc asmcmc, ph[14] as RV_NCELL, all
 * F2(x,nlay,lay,ig); reicmc / relqmc 1-based per layer. */
static int SFX(rv_cldprmc_col)(int nlay, int iceflag, const int *cldymc, const REAL *ciwpmc, const REAL *clwpmc, const REAL *reicmc,
                               const REAL *relqmc, REAL **comb, REAL **ph)
{
    const SFX(sw_tables_t) *t = &SFX(S);
    const REAL epsg = (REAL)1.e-06, cldmin = (REAL)1.e-20;
    if (iceflag < 1 || iceflag > 4) return 10;
    for (int ig = 1; ig <= RVNG; ig++) {
        const int ibf = t->ngb[ig - 1], ib = ibf - 15;
        for (int lay = 1; lay <= nlay; lay++) {
            if (!F2(cldymc, nlay, lay, ig)) {
                /* not cldymc (:385-411): 0 / 1 / 0 for every family */
                F2(comb[0], nlay, lay, ig) = 0; F2(comb[1], nlay, lay, ig) = 0; F2(comb[2], nlay, lay, ig) = 1; F2(comb[3], nlay, lay, ig) = 0;
                for (int p = 0; p < 2; p++) {
                    F2(ph[7 * p + 0], nlay, lay, ig) = 0; F2(ph[7 * p + 1], nlay, lay, ig) = 1; F2(ph[7 * p + 2], nlay, lay, ig) = 0;
                    F2(ph[7 * p + 3], nlay, lay, ig) = 0; F2(ph[7 * p + 4], nlay, lay, ig) = 1; F2(ph[7 * p + 5], nlay, lay, ig) = 0;
                    F2(ph[7 * p + 6], nlay, lay, ig) = 0;      /* forw? is zeroed at entry (:131-133) and multiplies a zero tau */
                }
                continue;
            }
            /* coefficients are zero at entry (:131-133) and stay so for a phase without condensate */
            REAL extcoice = 0, ssacoice = 0, gice = 0, forwice = 0, extcoliq = 0, ssacoliq = 0, gliq = 0, forwliq = 0;
            const REAL ciwp = F2(ciwpmc, nlay, lay, ig), clwp = F2(clwpmc, nlay, lay, ig);
            if (ciwp != 0) {      /* ice (:140-254) */
                REAL radice = reicmc[lay];
                if (iceflag == 1) {
                    int ic = t->icxa[ibf - 16];
                    extcoice = t->abari[ic - 1] + t->bbari[ic - 1] / radice;
                    ssacoice = (REAL)1. - t->cbari[ic - 1] - t->dbari[ic - 1] * radice;
                    gice = t->ebari[ic - 1] + t->fbari[ic - 1] * radice;
                    if (gice > (REAL)1. - epsg) gice = (REAL)1. - epsg;
                    forwice = gice * gice;
                } else if (iceflag == 2) {
                    REAL factor = (radice - (REAL)2.) / (REAL)3.; int index = (int)factor; if (index == 43) index = 42;
                    REAL fint = factor - (REAL)index;
                    extcoice = RVLIN(t->extice2, 43, index, ib, fint); ssacoice = RVLIN(t->ssaice2, 43, index, ib, fint);
                    gice = RVLIN(t->asyice2, 43, index, ib, fint); forwice = gice * gice;
                } else if (iceflag == 3) {
                    REAL factor = (radice - (REAL)2.) / (REAL)3.; int index = (int)factor; if (index == 46) index = 45;
                    REAL fint = factor - (REAL)index;
                    extcoice = RVLIN(t->extice3, 46, index, ib, fint); ssacoice = RVLIN(t->ssaice3, 46, index, ib, fint);
                    gice = RVLIN(t->asyice3, 46, index, ib, fint);
                    REAL fdelta = RVLIN(t->fdlice3, 46, index, ib, fint);
                    forwice = fdelta + (REAL)0.5 / ssacoice;
                    if (forwice > gice) forwice = gice;
                } else {
                    REAL factor = radice; int index = (int)factor; REAL fint = factor - (REAL)index;
                    extcoice = RVLIN(t->extice4, 200, index, ib, fint); ssacoice = RVLIN(t->ssaice4, 200, index, ib, fint);
                    gice = RVLIN(t->asyice4, 200, index, ib, fint); forwice = gice * gice;
                }
            }
            if (clwp != 0) {      /* liquid, liqflag 1 (:262-300) */
                REAL radliq = relqmc[lay];
                int index = (int)(radliq - (REAL)1.5);
                if (index == 0) index = 1;
                if (index == 58) index = 57;
                REAL fint = radliq - (REAL)1.5 - (REAL)index;
                extcoliq = RVLIN(t->extliq1, 58, index, ib, fint);
                ssacoliq = RVLIN(t->ssaliq1, 58, index, ib, fint);
                if (fint < 0 && ssacoliq > (REAL)1.) ssacoliq = F2(t->ssaliq1, 58, index, ib);
                gliq = RVLIN(t->asyliq1, 58, index, ib, fint);
                forwliq = gliq * gliq;
            }
            /* (:316-351) */
            REAL tauliqorig = clwp * extcoliq, tauiceorig = ciwp * extcoice;
            F2(comb[0], nlay, lay, ig) = tauliqorig + tauiceorig;
            F2(ph[0], nlay, lay, ig) = tauliqorig; F2(ph[7], nlay, lay, ig) = tauiceorig;      /* ltaormc, itaormc */
            F2(ph[1], nlay, lay, ig) = ssacoliq; F2(ph[8], nlay, lay, ig) = ssacoice;          /* lomormc, iomormc */
            F2(ph[2], nlay, lay, ig) = gliq; F2(ph[9], nlay, lay, ig) = gice;                  /* lasormc, iasormc */
            REAL ssaliq = ssacoliq * ((REAL)1. - forwliq) / ((REAL)1. - forwliq * ssacoliq);
            REAL ssaice = ssacoice * ((REAL)1. - forwice) / ((REAL)1. - forwice * ssacoice);
            REAL tauliq = ((REAL)1. - forwliq * ssacoliq) * tauliqorig;
            REAL tauice = ((REAL)1. - forwice * ssacoice) * tauiceorig;
            REAL scatliq = ssaliq * tauliq, scatice = ssaice * tauice;
            REAL tc = tauliq + tauice;
            F2(ph[3], nlay, lay, ig) = tauliq; F2(ph[10], nlay, lay, ig) = tauice;             /* ltaucmc, itaucmc */
            F2(ph[4], nlay, lay, ig) = ssaliq; F2(ph[11], nlay, lay, ig) = ssaice;             /* lomgcmc, iomgcmc */
            F2(ph[5], nlay, lay, ig) = (gliq - forwliq) / ((REAL)1. - forwliq);                /* lasycmc */
            F2(ph[12], nlay, lay, ig) = (gice - forwice) / ((REAL)1. - forwice);               /* iasycmc */
            F2(ph[6], nlay, lay, ig) = forwliq; F2(ph[13], nlay, lay, ig) = forwice;
            /* (:353-383) */
            if (tc == 0) tc = cldmin;
            if (scatice == 0) scatice = cldmin;
            F2(comb[1], nlay, lay, ig) = tc;
            F2(comb[2], nlay, lay, ig) = (scatliq + scatice) / tc;
            if (iceflag == 3)
                F2(comb[3], nlay, lay, ig) = ((REAL)1. / (scatliq + scatice)) *
                    (scatliq * (gliq - forwliq) / ((REAL)1. - forwliq) + scatice * ((gice - forwice) / ((REAL)1. - forwice)));
            else
                F2(comb[3], nlay, lay, ig) = (scatliq * (gliq - forwliq) / ((REAL)1. - forwliq) +
                                              scatice * (gice - forwice) / ((REAL)1. - forwice)) / (scatliq + scatice);
        }
    }
    return 0;
}

/* Fortran sum(a(l0:l1)), sum(a * b), sum(a * b * c): accumulated in index order from zero */
static REAL SFX(rv_sum1)(const REAL *a, int nlay, int ig, int l0, int l1)
{ REAL s = 0; for (int l = l0; l <= l1; l++) s = s + F2(a, nlay, l, ig); return s; }
static REAL SFX(rv_sum2)(const REAL *a, const REAL *b, int nlay, int ig, int l0, int l1)
{ REAL s = 0; for (int l = l0; l <= l1; l++) s = s + F2(a, nlay, l, ig) * F2(b, nlay, l, ig); return s; }
static REAL SFX(rv_sum3)(const REAL *a, const REAL *b, const REAL *c, int nlay, int ig, int l0, int l1)
{ REAL s = 0; for (int l = l0; l <= l1; l++) s = s + F2(a, nlay, l, ig) * F2(b, nlay, l, ig) * F2(c, nlay, l, ig); return s; }

/* slot of family f (reference order: cds | cotl cdsl coti cdsi | ssal sdsl ssai sdsi | asml adsl asmi adsi | forl fori), d (0) or
 * n (1), super-layer k (0 tp, 1 hp, 2 mp, 3 lp): the order of the dummy arguments (SW/rrtmg_sw_rad.F90:86-119) */
#define RVSLOT(f, dn, k) ((f) * 8 + (dn) * 4 + (k))
#ifndef RV_FAMILIES_DEFINED
#define RV_FAMILIES_DEFINED
enum { RV_CDS, RV_COTL, RV_CDSL, RV_COTI, RV_CDSI, RV_SSAL, RV_SDSL, RV_SSAI, RV_SDSI, RV_ASML, RV_ADSL, RV_ASMI, RV_ADSI, RV_FORL, RV_FORI, RV_NFAM };
#endif

/* one phase, one super-layer set k, one sub-column: the guarded accumulation of e.g. :812-870 (low), :1054-1104 (whole column).
 * s[7] = sum(tau), sum(tau om), sum(tau om as) un-scaled; sum(tau), sum(tau om), sum(tau om asy), sum(tau om forw) scaled */
static void SFX(rv_acc_phase)(REAL *z, int k, REAL wgt, const REAL *s, int fcot, int fcds, int fssa, int fsds, int fasm, int fads, int ffor)
{
    if (s[0] > 0) {
        z[RVSLOT(fcot, 0, k)] = z[RVSLOT(fcot, 0, k)] + wgt;        z[RVSLOT(fcot, 1, k)] = z[RVSLOT(fcot, 1, k)] + wgt * s[0];
        z[RVSLOT(fssa, 0, k)] = z[RVSLOT(fssa, 0, k)] + wgt * s[0]; z[RVSLOT(fssa, 1, k)] = z[RVSLOT(fssa, 1, k)] + wgt * s[1];
        z[RVSLOT(fasm, 0, k)] = z[RVSLOT(fasm, 0, k)] + wgt * s[1]; z[RVSLOT(fasm, 1, k)] = z[RVSLOT(fasm, 1, k)] + wgt * s[2];
    }
    if (s[3] > 0) {
        z[RVSLOT(fcds, 0, k)] = z[RVSLOT(fcds, 0, k)] + wgt;        z[RVSLOT(fcds, 1, k)] = z[RVSLOT(fcds, 1, k)] + wgt * s[3];
        z[RVSLOT(fsds, 0, k)] = z[RVSLOT(fsds, 0, k)] + wgt * s[3]; z[RVSLOT(fsds, 1, k)] = z[RVSLOT(fsds, 1, k)] + wgt * s[4];
        z[RVSLOT(fads, 0, k)] = z[RVSLOT(fads, 0, k)] + wgt * s[4]; z[RVSLOT(fads, 1, k)] = z[RVSLOT(fads, 1, k)] + wgt * s[5];
        z[RVSLOT(ffor, 0, k)] = z[RVSLOT(ffor, 0, k)] + wgt * s[4]; z[RVSLOT(ffor, 1, k)] = z[RVSLOT(ffor, 1, k)] + wgt * s[6];
    }
}

/* API layouts as oracle_rrtmg_sw; cot (8,ncol) as there; radval (120,ncol); cell: NULL or (ncol,14,112,nlay) per-cell phase values;
 * comb: NULL or (ncol,4,112,nlay) taormc taucmc ssacmc asmcmc.  Returns 0, 10 invalid iceflag, 20 unsupported solar option. */
int SFX(rv_rrtmg_sw_radval)(int ncol, int nlay, REAL scon, REAL adjes, int isolvar, const REAL *play, const REAL *plev, const REAL *tlay,
                            const REAL *h2ovmr, const REAL *o3vmr, const REAL *co2vmr, const REAL *ch4vmr, const REAL *o2vmr, int iceflgsw,
                            const REAL *cld, const REAL *ciwp, const REAL *clwp, const REAL *rei, const REAL *rel, int dyofyr,
                            const REAL *zm, const REAL *alat, int cloudLM, int cloudMH, int *clearCounts, REAL *cot, REAL *radval,
                            REAL *cell, REAL *comb)
{
    const SFX(sw_tables_t) *t = &SFX(S);
    /* solar variability, optional arguments absent, scon > 0 (SW/rrtmg_sw_rad.F90:893-1127) */
    REAL solvar[30], adjflux[30], svar[3] = {1, 1, 1}, svar_bnd[29 * 3];
    for (int b = 0; b < 30; b++) { solvar[b] = 1; adjflux[b] = 1; }
    for (int i = 0; i < 29 * 3; i++) svar_bnd[i] = 1;
    const REAL Iint = *t->Iint, Fint = *t->Fint, Sint = *t->Sint;
    if (!(scon > 0)) return 20;
    if (isolvar == -1) { for (int b = 16; b <= 29; b++) solvar[b] = scon / *t->rrsw_scon; }
    else if (isolvar == 0) { REAL scon_int = Fint + Sint + Iint, r = scon / scon_int; svar[0] = r; svar[1] = r; svar[2] = r; }
    else if (isolvar == 2) {
        svar[0] = (*t->Mg_avg - *t->Mg_0) / (*t->Mg_avg - *t->Mg_0); svar[1] = (*t->SB_avg - *t->SB_0) / (*t->SB_avg - *t->SB_0);
        svar[2] = (scon - (svar[0] * Fint + svar[1] * Sint)) / Iint;
    } else if (isolvar == 3) {
        REAL scon_int = Fint + Sint + Iint;
        for (int b = 16; b <= 29; b++) { solvar[b] = scon / scon_int; F2(svar_bnd, 29, b, 1) = solvar[b]; F2(svar_bnd, 29, b, 2) = solvar[b]; F2(svar_bnd, 29, b, 3) = solvar[b]; }
    } else return 20;
    for (int b = 16; b <= 29; b++) adjflux[b] = adjes;
    if (isolvar < 0) for (int b = 16; b <= 29; b++) adjflux[b] = adjflux[b] * solvar[b];

    const size_t n1 = (size_t)nlay + 3, ng = (size_t)RVNG * nlay;
    SFX(swcol_t) s;
    SFX(swcol_alloc)(&s, nlay);
    REAL *w[14];
    for (int k = 0; k < 14; k++) w[k] = (REAL *)calloc(n1, sizeof(REAL));
    REAL *pav = w[0], *tav = w[1], *plv = w[2], *vh = w[3], *vc = w[4], *vo = w[5], *vm = w[6], *vx = w[7], *vcld = w[8], *vci = w[9],
         *vcl = w[10], *vrei = w[11], *vrel = w[12], *vzm = w[13];
    REAL *taug = calloc(ng, sizeof(REAL)), *taur = calloc(ng, sizeof(REAL)), *ciwpm = calloc(ng, sizeof(REAL)), *clwpm = calloc(ng, sizeof(REAL));
    REAL *cb[4], *ph[RV_NCELL];
    for (int k = 0; k < 4; k++) cb[k] = calloc(ng, sizeof(REAL));
    for (int k = 0; k < RV_NCELL; k++) ph[k] = calloc(ng, sizeof(REAL));
    int *cldym = calloc(ng, sizeof(int));
    static const int so[4] = {4, 3, 2, 1};       /* seed_order of the SW call (SW/rrtmg_sw_rad.F90:1401) */
    const int surface_at_one = play[0] > play[(size_t)(nlay - 1) * ncol];
    int rc = 0;
    for (int c = 0; c < ncol && !rc; c++) {
        for (int l = 1; l <= nlay; l++) {
            size_t i = (size_t)(l - 1) * ncol + c;
            pav[l] = play[i]; tav[l] = tlay[i]; vh[l] = h2ovmr[i]; vc[l] = co2vmr[i]; vo[l] = o3vmr[i]; vm[l] = ch4vmr[i]; vx[l] = o2vmr[i];
            vcld[l] = cld[i]; vci[l] = ciwp[i]; vcl[l] = clwp[i]; vrei[l] = rei[i]; vrel[l] = rel[i]; vzm[l] = zm[i];
        }
        for (int l = 1; l <= nlay + 1; l++) plv[l] = plev[(size_t)(l - 1) * ncol + c];
        int cloudy_col = 0;
        for (int l = 1; l <= nlay; l++) if (vcld[l] > 0) cloudy_col = 1;
        int cnt[4] = {RVNG, RVNG, RVNG, RVNG};
        REAL z[8 * RV_NFAM], zc[8];
        for (int k = 0; k < 8 * RV_NFAM; k++) z[k] = 0;      /* spcvmc :676-746; rrtmg_sw_rad :1540-1590 for cloud-free columns */
        for (int k = 0; k < 8; k++) zc[k] = 0;
        if (cloudy_col) {      /* cc == 2 (spcvmc :749) */
            SFX(mcica_col)(RVNG, nlay, surface_at_one, vzm, alat[c], dyofyr, pav, vcld, vci, vcl, (REAL)1.e-20, so, cldym, ciwpm, clwpm);
            SFX(clearcounts_col)(RVNG, nlay, cloudLM, cloudMH, cldym, cnt);
            rc = SFX(rv_cldprmc_col)(nlay, iceflgsw, cldym, ciwpm, clwpm, vrei, vrel, cb, ph);
            if (rc) break;
            SFX(sw_setcoef_col)(&s, pav, tav, plv, vh, vc, vo, vm, vx);
            REAL ssi[RVNG], sfz[RVNG];
            for (int g = 0; g < RVNG; g++) { ssi[g] = 0; sfz[g] = 0; }
            SFX(sw_taumol_col)(&s, isolvar, svar, svar_bnd, taug, taur, ssi, sfz);
            for (int iw = 1; iw <= RVNG; iw++) {
                const int jb = t->ngb[iw - 1], ibm = jb - 15;
                REAL wgt;      /* band weights (:756-771) */
                if (ibm >= 10 && ibm <= 11) wgt = (REAL)1.0; else if (ibm == 9) wgt = (REAL)0.5; else continue;
                REAL zincflx = isolvar < 0 ? adjflux[jb] * sfz[iw - 1] : adjflux[jb] * ssi[iw - 1];      /* (:775-779) */
                wgt = wgt * zincflx;
                /* the layer sums of the three super-layers: low 1:cloudLM (:782-870), mid cloudLM+1:cloudMH, high cloudMH+1:nlay */
                const int l0[3] = {1, cloudLM + 1, cloudMH + 1}, l1[3] = {cloudLM, cloudMH, nlay};
                REAL stao[3], stau[3], sp[2][3][7];
                for (int k = 0; k < 3; k++) {
                    stao[k] = SFX(rv_sum1)(cb[0], nlay, iw, l0[k], l1[k]);
                    stau[k] = SFX(rv_sum1)(cb[1], nlay, iw, l0[k], l1[k]);
                    for (int p = 0; p < 2; p++) {
                        REAL **q = ph + 7 * p, *o = sp[p][k];
                        for (int j = 0; j < 7; j++) o[j] = 0;
                        o[0] = SFX(rv_sum1)(q[0], nlay, iw, l0[k], l1[k]);
                        if (o[0] > 0) {      /* the product sums are formed under the guard, else they stay 0 (:809-812) */
                            o[1] = SFX(rv_sum2)(q[0], q[1], nlay, iw, l0[k], l1[k]);
                            o[2] = SFX(rv_sum3)(q[0], q[1], q[2], nlay, iw, l0[k], l1[k]);
                        }
                        o[3] = SFX(rv_sum1)(q[3], nlay, iw, l0[k], l1[k]);
                        if (o[3] > 0) {
                            o[4] = SFX(rv_sum2)(q[3], q[4], nlay, iw, l0[k], l1[k]);
                            o[5] = SFX(rv_sum3)(q[3], q[4], q[5], nlay, iw, l0[k], l1[k]);
                            o[6] = SFX(rv_sum3)(q[3], q[4], q[6], nlay, iw, l0[k], l1[k]);
                        }
                    }
                }
                /* super-layer k of the outputs: 3 lp = low (0), 2 mp = mid (1), 1 hp = high (2); then the whole column (:1043-1104):
                 * the sum of the three super-layer sums in the order low + mid + high */
                for (int kk = 0; kk < 4; kk++) {
                    const int k = kk < 3 ? 3 - kk : 0;
                    REAL a, u, sv[2][7];
                    if (kk < 3) { a = stao[kk]; u = stau[kk]; for (int p = 0; p < 2; p++) for (int j = 0; j < 7; j++) sv[p][j] = sp[p][kk][j]; }
                    else {
                        a = stao[0] + stao[1] + stao[2]; u = stau[0] + stau[1] + stau[2];
                        for (int p = 0; p < 2; p++) for (int j = 0; j < 7; j++) sv[p][j] = sp[p][0][j] + sp[p][1][j] + sp[p][2][j];
                    }
                    if (a > 0) { zc[k] = zc[k] + wgt; zc[4 + k] = zc[4 + k] + wgt * a; }
                    if (u > 0) { z[RVSLOT(RV_CDS, 0, k)] = z[RVSLOT(RV_CDS, 0, k)] + wgt; z[RVSLOT(RV_CDS, 1, k)] = z[RVSLOT(RV_CDS, 1, k)] + wgt * u; }
                    SFX(rv_acc_phase)(z, k, wgt, sv[0], RV_COTL, RV_CDSL, RV_SSAL, RV_SDSL, RV_ASML, RV_ADSL, RV_FORL);
                    SFX(rv_acc_phase)(z, k, wgt, sv[1], RV_COTI, RV_CDSI, RV_SSAI, RV_SDSI, RV_ASMI, RV_ADSI, RV_FORI);
                }
            }
            if (cell) for (int k = 0; k < RV_NCELL; k++) memcpy(cell + ((size_t)c * RV_NCELL + k) * ng, ph[k], ng * sizeof(REAL));
            if (comb) for (int k = 0; k < 4; k++) memcpy(comb + ((size_t)c * 4 + k) * ng, cb[k], ng * sizeof(REAL));
        } else {
            if (cell) for (int k = 0; k < RV_NCELL; k++) for (size_t i = 0; i < ng; i++) cell[((size_t)c * RV_NCELL + k) * ng + i] = (k % 7 == 1 || k % 7 == 4) ? 1 : 0;
            if (comb) for (int k = 0; k < 4; k++) for (size_t i = 0; i < ng; i++) comb[((size_t)c * 4 + k) * ng + i] = k == 2 ? 1 : 0;
        }
        for (int k = 0; k < 4; k++) clearCounts[(size_t)k * ncol + c] = cnt[k];
        for (int k = 0; k < 8; k++) cot[(size_t)k * ncol + c] = zc[k];
        for (int k = 0; k < 8 * RV_NFAM; k++) radval[(size_t)k * ncol + c] = z[k];
    }
    for (int k = 0; k < 14; k++) free(w[k]);
    for (int k = 0; k < 4; k++) free(cb[k]);
    for (int k = 0; k < RV_NCELL; k++) free(ph[k]);
    free(taug); free(taur); free(ciwpm); free(clwpm); free(cldym);
    SFX(swcol_free)(&s);
    return rc;
}
#undef RVLIN
#undef RVNG
#undef RVSLOT
#undef RV_NCELL
