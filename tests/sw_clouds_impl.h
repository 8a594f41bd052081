/* sw_clouds_impl.h -- TEST INFRASTRUCTURE: plain-C restatement of the cloud diagnostics of the Solar GridComp's UPDATE_EXPORT
 * (GEOSsolar_GridComp/GEOS_SolarGridComp.F90:7006-7058, :7223-7392) and of the routine it calls per column, getvistau
 * (GEOS_RadiationShared/gettau.F90:33-96, getvistau.code), keeping taudiff PER SPECIES (the oracle's cs_gettau returns only the
 * species sums).  Statement by statement, whole-array statements as loops over the columns.  Included once per precision by
 * sw_clouds_ref.c (REAL / SFX / LOG10 defined there); the tables are the oracle's (oracle_chou_sw_set_table_*). */

/* getvistau (getvistau.code): nlevs layers, arrays 1-based over k as the oracle's cs_gettau (dp[k], fcld[k], reff[(l-1)*(nlevs+1)+k]);
 * taubeam / taudiff [(l-1)*(nlevs+1)+k].  grav = MAPL_GRAV. */
static void SFX(swk_getvistau)(int nlevs, REAL cosz, const REAL *dp, const REAL *fcld, const REAL *reff, const REAL *hydromets,
                               int ict, int icb, REAL grav, REAL *taubeam, REAL *taudiff)
{
    const SFX(chsw_tables_t) *t = &SFX(CS);
    const int nm = 11, nt = 9, na = 11, n1 = nlevs + 1;
    const REAL dm = (REAL)0.1, dt = (REAL)0.30103, da = (REAL)0.1, t1 = (REAL)-0.9031;
#define RE(k, l) reff[((l) - 1) * n1 + (k)]
#define HY(k, l) hydromets[((l) - 1) * n1 + (k)]
#define TB(k, l) taubeam[((l) - 1) * n1 + (k)]
#define TD(k, l) taudiff[((l) - 1) * n1 + (k)]
#define CAIB(a, b, c) t->caib[(((c) - 1) * 9 + ((b) - 1)) * 11 + ((a) - 1)]
#define CAIF(a, b) t->caif[((b) - 1) * 9 + ((a) - 1)]
    for (int k = 1; k <= nlevs; k++)
        for (int l = 1; l <= 4; l++) TB(k, l) = TD(k, l) = 0;
    REAL cc[4] = {0, 0, 0, 0};
    if (ict != 0) {
        for (int k = 1; k <= ict - 1; k++) cc[1] = fcld[k] > cc[1] ? fcld[k] : cc[1];
        for (int k = ict; k <= icb - 1; k++) cc[2] = fcld[k] > cc[2] ? fcld[k] : cc[2];
        for (int k = icb; k <= nlevs; k++) cc[3] = fcld[k] > cc[3] ? fcld[k] : cc[3];
    }
    for (int k = 1; k <= nlevs; k++) {
        REAL taucld1, taucld2, taucld3, taucld4;
        if (RE(k, 1) <= (REAL)0.) taucld1 = 0;
        else taucld1 = (((dp[k] * (REAL)1.0e3) / grav) * HY(k, 1)) * *t->aib_uv / RE(k, 1);
        if (RE(k, 2) <= (REAL)0.) taucld2 = 0;
        else taucld2 = (((dp[k] * (REAL)1.0e3) / grav) * HY(k, 2)) * (t->awb_uv[0] + t->awb_uv[1] / RE(k, 2));
        taucld3 = (((dp[k] * (REAL)1.0e3) / grav) * HY(k, 3)) * t->arb_uv[0];
        const REAL reff_snow = RE(k, 4) < (REAL)112.0 ? RE(k, 4) : (REAL)112.0;
        if (reff_snow <= (REAL)0.) taucld4 = 0;
        else taucld4 = (((dp[k] * (REAL)1.0e3) / grav) * HY(k, 4)) * *t->aib_uv / reff_snow;
        if (ict != 0) {
            int kk;
            if (k < ict) kk = 1;
            else if (k >= ict && k < icb) kk = 2;
            else kk = 3;
            REAL tauc = taucld1 + taucld2 + taucld3 + taucld4;
            if (tauc > (REAL)0.02 && fcld[k] > (REAL)0.01) {
                REAL fa = fcld[k] / cc[kk];
                tauc = tauc < (REAL)32. ? tauc : (REAL)32.;
                REAL fm = cosz / dm;
                REAL ft = (LOG10(tauc) - t1) / dt;
                fa = fa / da;
                int im = (int)(fm + (REAL)1.5), it = (int)(ft + (REAL)1.5), ia = (int)(fa + (REAL)1.5);
                im = im > 2 ? im : 2; it = it > 2 ? it : 2; ia = ia > 2 ? ia : 2;
                im = im < nm - 1 ? im : nm - 1; it = it < nt - 1 ? it : nt - 1; ia = ia < na - 1 ? ia : na - 1;
                fm = fm - (REAL)(im - 1); ft = ft - (REAL)(it - 1); fa = fa - (REAL)(ia - 1);
                REAL xai = (-CAIB(im - 1, it, ia) * ((REAL)1. - fm) + CAIB(im + 1, it, ia) * ((REAL)1. + fm)) * fm * (REAL).5 +
                           CAIB(im, it, ia) * ((REAL)1. - fm * fm);
                xai = xai + (-CAIB(im, it - 1, ia) * ((REAL)1. - ft) + CAIB(im, it + 1, ia) * ((REAL)1. + ft)) * ft * (REAL).5 +
                      CAIB(im, it, ia) * ((REAL)1. - ft * ft);
                xai = xai + (-CAIB(im, it, ia - 1) * ((REAL)1. - fa) + CAIB(im, it, ia + 1) * ((REAL)1. + fa)) * fa * (REAL).5 +
                      CAIB(im, it, ia) * ((REAL)1. - fa * fa);
                xai = xai - (REAL)2. * CAIB(im, it, ia);
                xai = xai > (REAL)0.0 ? xai : (REAL)0.0;
                xai = xai < (REAL)1.0 ? xai : (REAL)1.0;
                TB(k, 1) = taucld1 * xai; TB(k, 2) = taucld2 * xai; TB(k, 3) = taucld3 * xai; TB(k, 4) = taucld4 * xai;
                xai = (-CAIF(it - 1, ia) * ((REAL)1. - ft) + CAIF(it + 1, ia) * ((REAL)1. + ft)) * ft * (REAL).5 +
                      CAIF(it, ia) * ((REAL)1. - ft * ft);
                xai = xai + (-CAIF(it, ia - 1) * ((REAL)1. - fa) + CAIF(it, ia + 1) * ((REAL)1. + fa)) * fa * (REAL).5 +
                      CAIF(it, ia) * ((REAL)1. - fa * fa);
                xai = xai - CAIF(it, ia);
                xai = xai > (REAL)0.0 ? xai : (REAL)0.0;
                xai = xai < (REAL)1.0 ? xai : (REAL)1.0;
                TD(k, 1) = taucld1 * xai; TD(k, 2) = taucld2 * xai; TD(k, 3) = taucld3 * xai; TD(k, 4) = taucld4 * xai;
            }
        } else {
            TB(k, 1) = TD(k, 1) = taucld1; TB(k, 2) = TD(k, 2) = taucld2; TB(k, 3) = TD(k, 3) = taucld3; TB(k, 4) = TD(k, 4) = taucld4;
        }
        /* asycl (getvistau.code, end) is a dummy argument of the UPDATE_EXPORT call: not restated */
    }
#undef RE
#undef HY
#undef TB
#undef TD
#undef CAIB
#undef CAIF
}

/* per-species taudiff of one column, summed in the order TAUCLD(:,:,:,1) uses (SOL:7280) */
int SFX(swk_getvistau_sum)(int np, REAL cosz, const REAL *dp, const REAL *fcld, const REAL *reff, const REAL *hyd, int ict, int icb,
                           REAL grav, REAL *tausum)
{
    REAL *tb = (REAL *)calloc((size_t)8 * (np + 1), sizeof(REAL));
    if (!tb) return 1;
    REAL *td = tb + (size_t)4 * (np + 1);
    SFX(swk_getvistau)(np, cosz, dp, fcld, reff, hyd, ict, icb, grav, tb, td);
    for (int k = 1; k <= np; k++) tausum[k] = td[k] + td[(np + 1) + k] + td[2 * (np + 1) + k] + td[3 * (np + 1) + k];
    free(tb);
    return 0;
}

/* the oracle's getvistau (cs_gettau, ib = 0): its diffuse species sum tauclf */
int SFX(swk_cs_tauclf)(int np, REAL cosz, const REAL *dp, const REAL *fcld, const REAL *reff, const REAL *hyd, int ict, int icb,
                       REAL *tauclf)
{
    REAL *w = (REAL *)calloc((size_t)4 * (np + 1), sizeof(REAL));
    if (!w) return 1;
    SFX(cs_gettau)(0, np, cosz, dp, fcld, reff, hyd, ict, icb, w, tauclf, w + (np + 1), w + 2 * (np + 1));
    free(w);
    return 0;
}

/* UPDATE_EXPORT's cloud block over ncol columns, every export associated.  in / out: the GEOSRAD_SWK_* orders of include/geosrad.h
 * (fields (ncol,LM) column fastest, PLE (ncol,0:LM), ZTH and the 2-D exports (ncol)). */
#ifndef SWK_ORDERS
#define SWK_ORDERS
enum { K_FCLD, K_PLE, K_T, K_QI, K_QL, K_QR, K_QS, K_RI, K_RL, K_RR, K_RS, K_ZTH };
enum { X_FCLD, X_TAUI, X_TAUW, X_TAUR, X_TAUS, X_CLDL, X_CLDM, X_CLDH, X_CLDT, X_COTDL, X_COTDM, X_COTDH, X_COTDT, X_TAUL, X_TAUM, X_TAUH,
       X_TAUT, X_TAUX, X_COTL, X_COTM, X_COTH, X_COTT, X_COTNL, X_COTNM, X_COTNH, X_COTNT, X_CLDTMP, X_CLDPRS };
#endif
int SFX(swk_update_clouds)(int ncol, int lm, int lcldmh, int lcldlm, REAL taucrit, REAL grav, REAL undef, const REAL *const *in,
                           REAL *const *out)
{
    const int n1 = lm + 1;
#define F3D(p, i, l) (p)[(size_t)((l) - 1) * ncol + (i)]          /* Fortran X(i, l), l = 1..LM */
#define PLL(i, l) in[K_PLE][(size_t)(l) * ncol + (i)]              /* PLE(i, l), l = 0..LM */
    REAL *taucld = (REAL *)calloc((size_t)ncol * lm * 4, sizeof(REAL));   /* TAUCLD(i, l, s) */
    REAL *col = (REAL *)calloc((size_t)12 * n1, sizeof(REAL));
    if (!taucld || !col) { free(taucld); free(col); return 1; }
#define TC(i, l, s) taucld[(((size_t)(s) - 1) * lm + ((l) - 1)) * ncol + (i)]
    REAL *dp = col, *fc = col + n1, *reff = col + 2 * n1, *hyd = col + 6 * n1;
    REAL *tbeam = (REAL *)calloc((size_t)4 * n1, sizeof(REAL)), *tdiff = (REAL *)calloc((size_t)4 * n1, sizeof(REAL));
    for (int i = 0; i < ncol; i++) {
        /* FCLD = CLIN (:7006) */
        for (int l = 1; l <= lm; l++) F3D(out[X_FCLD], i, l) = F3D(in[K_FCLD], i, l);
        REAL aCLDH = 0, aCLDM = 0, aCLDL = 0;
        for (int l = 1; l <= lcldmh - 1; l++) aCLDH = F3D(in[K_FCLD], i, l) > aCLDH ? F3D(in[K_FCLD], i, l) : aCLDH;
        for (int l = lcldmh; l <= lcldlm - 1; l++) aCLDM = F3D(in[K_FCLD], i, l) > aCLDM ? F3D(in[K_FCLD], i, l) : aCLDM;
        for (int l = lcldlm; l <= lm; l++) aCLDL = F3D(in[K_FCLD], i, l) > aCLDL ? F3D(in[K_FCLD], i, l) : aCLDL;
        const REAL aCLDT = (REAL)1. - ((REAL)1 - aCLDH) * ((REAL)1 - aCLDM) * ((REAL)1 - aCLDL);
        out[X_CLDH][i] = out[X_COTDH][i] = aCLDH;
        out[X_CLDM][i] = out[X_COTDM][i] = aCLDM;
        out[X_CLDL][i] = out[X_COTDL][i] = aCLDL;
        out[X_CLDT][i] = out[X_COTDT][i] = aCLDT;
        /* DP, REFF, HYDROMETS, GETVISTAU (:7238-7272) */
        REAL zth = in[K_ZTH][i];
        zth = zth > (REAL)0.0 ? zth : (REAL)0.0;
        for (int l = 1; l <= lm; l++) {
            dp[l] = PLL(i, l) - PLL(i, l - 1);
            fc[l] = F3D(in[K_FCLD], i, l);
            for (int s = 1; s <= 4; s++) {
                reff[(s - 1) * n1 + l] = F3D(in[K_RI + s - 1], i, l) * (REAL)1.e6;
                hyd[(s - 1) * n1 + l] = F3D(in[K_QI + s - 1], i, l);
            }
        }
        SFX(swk_getvistau)(lm, zth, dp, fc, reff, hyd, lcldmh, lcldlm, grav, tbeam, tdiff);
        for (int l = 1; l <= lm; l++)
            for (int s = 1; s <= 4; s++) TC(i, l, s) = tdiff[(s - 1) * n1 + l];
    }
    for (int i = 0; i < ncol; i++)
        for (int l = 1; l <= lm; l++) {
            F3D(out[X_TAUI], i, l) = TC(i, l, 1); F3D(out[X_TAUW], i, l) = TC(i, l, 2);
            F3D(out[X_TAUR], i, l) = TC(i, l, 3); F3D(out[X_TAUS], i, l) = TC(i, l, 4);
            TC(i, l, 1) = TC(i, l, 1) + TC(i, l, 2) + TC(i, l, 3) + TC(i, l, 4);
        }
    for (int i = 0; i < ncol; i++) {
        const REAL aCLDH = out[X_CLDH][i], aCLDM = out[X_CLDM][i], aCLDL = out[X_CLDL][i], aCLDT = out[X_CLDT][i];
        REAL aTAUH = 0, aTAUM = 0, aTAUL = 0;
        for (int l = 1; l <= lcldmh - 1; l++) aTAUH = aTAUH + TC(i, l, 1);
        for (int l = lcldmh; l <= lcldlm - 1; l++) aTAUM = aTAUM + TC(i, l, 1);
        for (int l = lcldlm; l <= lm; l++) aTAUL = aTAUL + TC(i, l, 1);
        out[X_TAUH][i] = aTAUH; out[X_COTH][i] = aCLDH > (REAL)0. ? aTAUH : undef; out[X_COTNH][i] = aCLDH * aTAUH;
        out[X_TAUM][i] = aTAUM; out[X_COTM][i] = aCLDM > (REAL)0. ? aTAUM : undef; out[X_COTNM][i] = aCLDM * aTAUM;
        out[X_TAUL][i] = aTAUL; out[X_COTL][i] = aCLDL > (REAL)0. ? aTAUL : undef; out[X_COTNL][i] = aCLDL * aTAUL;
        out[X_TAUT][i] = aTAUH + aTAUM + aTAUL;
        REAL aTAUT = 0;
        if (aCLDT > (REAL)0.) aTAUT = (aTAUL * aCLDL + aTAUM * aCLDM + aTAUH * aCLDH) / aCLDT;
        out[X_TAUX][i] = aTAUT;
        out[X_COTT][i] = aCLDT > (REAL)0. ? aTAUT : undef;
        out[X_COTNT][i] = aCLDT * aTAUT;
        /* cloud top (:7375-7389): L = LM..1, the last hit (the topmost layer) stays */
        out[X_CLDTMP][i] = undef; out[X_CLDPRS][i] = undef;
        for (int l = lm; l >= 1; l--)
            if (TC(i, l, 1) > taucrit) { out[X_CLDTMP][i] = F3D(in[K_T], i, l); out[X_CLDPRS][i] = PLL(i, l - 1); }
    }
#undef TC
#undef F3D
#undef PLL
    free(taucld); free(col); free(tbeam); free(tdiff);
    return 0;
}
