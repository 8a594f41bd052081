/* gettau_impl.h -- TEST INFRASTRUCTURE: plain-C restatement of GEOS_RadiationShared/gettau.F90 (getvistau.code, getnirtau.code,
 * getirtau.code) with every output PER SPECIES, over a batch of columns in the layout of include/geosrad_gettau.h (column index fastest:
 * dp, fcld (ncol,nlevs); reff, hydromets, taubeam, taudiff, taudiag (ncol,nlevs,4); tcldlyr, enn (ncol,0:nlevs)), statement by statement;
 * the same routines through the oracle's cs_gettau / ch_getirtau (species sums; an independent statement of each); and the infrared cloud
 * exports of LW_Driver (GEOS_IrradGridComp.F90:1898-1912, :3626-3650).  Included once per precision by gettau_ref.c (REAL / SFX / LOG10 /
 * POW / EXP defined there); the tables are the oracle's (oracle_chou_sw_set_table_*, oracle_chou_set_table_*). */

#define GT2(a, i, k) (a)[(size_t)((k) - 1) * ncol + (i)]                              /* X(i, k), k = 1..nlevs */
#define GT3(a, i, k, l) (a)[((size_t)((l) - 1) * nlevs + ((k) - 1)) * ncol + (i)]     /* X(i, k, l), l = 1..4 */
#define GT0(a, i, k) (a)[(size_t)(k) * ncol + (i)]                                    /* X(i, k), k = 0..nlevs */

/* getvistau.code (ib = 0) / getnirtau.code (ib = 1..3) for every column */
int SFX(gtr_swtau)(int ib, int ncol, int nlevs, const REAL *coszs, const REAL *dp, const REAL *fcld, const REAL *reff, const REAL *hydromets,
                   int ict, int icb, REAL grav, REAL *taubeam, REAL *taudiff, REAL *asycl, REAL *ssacl)
{
    const SFX(chsw_tables_t) *t = &SFX(CS);
    const int nm = 11, nt = 9, na = 11;
    const REAL dm = (REAL)0.1, dt = (REAL)0.30103, da = (REAL)0.1, t1 = (REAL)-0.9031;
#define CAIB(a, b, c) t->caib[(((c) - 1) * 9 + ((b) - 1)) * 11 + ((a) - 1)]
#define CAIF(a, b) t->caif[((b) - 1) * 9 + ((a) - 1)]
#define NIR(tab, j) t->tab[((j) - 1) * 3 + (ib - 1)]                                  /* tab(ib, j) */
    for (int i = 0; i < ncol; i++) {
        const REAL cosz = coszs[i];
        for (int k = 1; k <= nlevs; k++)
            for (int l = 1; l <= 4; l++) GT3(taubeam, i, k, l) = GT3(taudiff, i, k, l) = 0;
        REAL cc[4] = {0, 0, 0, 0};
        if (ict != 0) {
            for (int k = 1; k <= ict - 1; k++) cc[1] = GT2(fcld, i, k) > cc[1] ? GT2(fcld, i, k) : cc[1];
            for (int k = ict; k <= icb - 1; k++) cc[2] = GT2(fcld, i, k) > cc[2] ? GT2(fcld, i, k) : cc[2];
            for (int k = icb; k <= nlevs; k++) cc[3] = GT2(fcld, i, k) > cc[3] ? GT2(fcld, i, k) : cc[3];
        }
        for (int k = 1; k <= nlevs; k++) {
            const REAL re1 = GT3(reff, i, k, 1), re2 = GT3(reff, i, k, 2), re4 = GT3(reff, i, k, 4);
            const REAL aib = ib == 0 ? *t->aib_uv : *t->aib_nir;
            const REAL awb1 = ib == 0 ? t->awb_uv[0] : NIR(awb_nir, 1), awb2 = ib == 0 ? t->awb_uv[1] : NIR(awb_nir, 2);
            const REAL arb1 = ib == 0 ? t->arb_uv[0] : NIR(arb_nir, 1);
            REAL taucld1, taucld2, taucld3, taucld4;
            if (re1 <= (REAL)0.) taucld1 = 0;
            else taucld1 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 1)) * aib / re1;
            if (re2 <= (REAL)0.) taucld2 = 0;
            else taucld2 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 2)) * (awb1 + awb2 / re2);
            taucld3 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 3)) * arb1;
            const REAL reff_snow = re4 < (REAL)112.0 ? re4 : (REAL)112.0;
            if (reff_snow <= (REAL)0.) taucld4 = 0;
            else taucld4 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 4)) * aib / reff_snow;
            if (ict != 0) {
                int kk;
                if (k < ict) kk = 1;
                else if (k >= ict && k < icb) kk = 2;
                else kk = 3;
                REAL tauc = taucld1 + taucld2 + taucld3 + taucld4;
                if (tauc > (REAL)0.02 && GT2(fcld, i, k) > (REAL)0.01) {
                    REAL fa;
                    if (ib == 0) fa = GT2(fcld, i, k) / cc[kk];                      /* getvistau.code divides */
                    else if (cc[kk] != (REAL)0.0) fa = GT2(fcld, i, k) / cc[kk];     /* getnirtau.code:97-101 guards */
                    else fa = 0;
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
                    GT3(taubeam, i, k, 1) = taucld1 * xai; GT3(taubeam, i, k, 2) = taucld2 * xai;
                    GT3(taubeam, i, k, 3) = taucld3 * xai; GT3(taubeam, i, k, 4) = taucld4 * xai;
                    xai = (-CAIF(it - 1, ia) * ((REAL)1. - ft) + CAIF(it + 1, ia) * ((REAL)1. + ft)) * ft * (REAL).5 +
                          CAIF(it, ia) * ((REAL)1. - ft * ft);
                    xai = xai + (-CAIF(it, ia - 1) * ((REAL)1. - fa) + CAIF(it, ia + 1) * ((REAL)1. + fa)) * fa * (REAL).5 +
                          CAIF(it, ia) * ((REAL)1. - fa * fa);
                    xai = xai - CAIF(it, ia);
                    xai = xai > (REAL)0.0 ? xai : (REAL)0.0;
                    xai = xai < (REAL)1.0 ? xai : (REAL)1.0;
                    GT3(taudiff, i, k, 1) = taucld1 * xai; GT3(taudiff, i, k, 2) = taucld2 * xai;
                    GT3(taudiff, i, k, 3) = taucld3 * xai; GT3(taudiff, i, k, 4) = taucld4 * xai;
                }
            } else {
                GT3(taubeam, i, k, 1) = GT3(taudiff, i, k, 1) = taucld1; GT3(taubeam, i, k, 2) = GT3(taudiff, i, k, 2) = taucld2;
                GT3(taubeam, i, k, 3) = GT3(taudiff, i, k, 3) = taucld3; GT3(taubeam, i, k, 4) = GT3(taudiff, i, k, 4) = taucld4;
            }
            REAL ssaclt = (REAL)0.99999, asyclt = (REAL)1.0;
            const REAL tauc = taucld1 + taucld2 + taucld3 + taucld4;
            if (tauc > (REAL)0.02 && GT2(fcld, i, k) > (REAL)0.01) {
                if (ib == 0) {
                    const REAL g1 = (t->aig_uv[0] + (t->aig_uv[1] + t->aig_uv[2] * re1) * re1) * taucld1;
                    const REAL g2 = (t->awg_uv[0] + (t->awg_uv[1] + t->awg_uv[2] * re2) * re2) * taucld2;
                    const REAL g3 = t->arg_uv[0] * taucld3;
                    const REAL g4 = (t->aig_uv[0] + (t->aig_uv[1] + t->aig_uv[2] * reff_snow) * reff_snow) * taucld4;
                    asyclt = (g1 + g2 + g3 + g4) / tauc;
                } else {
                    const REAL w1 = ((REAL)1. - (NIR(aia_nir, 1) + (NIR(aia_nir, 2) + NIR(aia_nir, 3) * re1) * re1)) * taucld1;
                    const REAL w2 = ((REAL)1. - (NIR(awa_nir, 1) + (NIR(awa_nir, 2) + NIR(awa_nir, 3) * re2) * re2)) * taucld2;
                    const REAL w3 = ((REAL)1. - NIR(ara_nir, 1)) * taucld3;
                    const REAL w4 = ((REAL)1. - (NIR(aia_nir, 1) + (NIR(aia_nir, 2) + NIR(aia_nir, 3) * reff_snow) * reff_snow)) * taucld4;
                    ssaclt = (w1 + w2 + w3 + w4) / tauc;
                    const REAL g1 = (NIR(aig_nir, 1) + (NIR(aig_nir, 2) + NIR(aig_nir, 3) * re1) * re1) * w1;
                    const REAL g2 = (NIR(awg_nir, 1) + (NIR(awg_nir, 2) + NIR(awg_nir, 3) * re2) * re2) * w2;
                    const REAL g3 = NIR(arg_nir, 1) * w3;
                    const REAL g4 = (NIR(aig_nir, 1) + (NIR(aig_nir, 2) + NIR(aig_nir, 3) * re4) * re4) * w4;   /* reff(k,4): getnirtau.code:205 */
                    if ((w1 + w2 + w3 + w4) != (REAL)0.0) asyclt = (g1 + g2 + g3 + g4) / (w1 + w2 + w3 + w4);
                }
            }
            if (ssacl) GT2(ssacl, i, k) = ssaclt;
            GT2(asycl, i, k) = asyclt;
        }
    }
#undef CAIB
#undef CAIF
#undef NIR
    return 0;
}

/* getirtau.code for every column */
int SFX(gtr_irtau)(int ib, int ncol, int nlevs, const REAL *dp, const REAL *fcld, const REAL *reff, const REAL *hydromets, REAL grav,
                   REAL *taudiag, REAL *tcldlyr, REAL *enn)
{
    const SFX(chou_tables_t) *t = &SFX(CH);
#define IR3(tab, j) t->tab[(ib - 1) * 3 + ((j) - 1)]      /* tab(j, ib), j = 1..3 */
#define IR(tab, j) t->tab[(ib - 1) * 4 + ((j) - 1)]       /* tab(j, ib), j = 1..4 */
    for (int i = 0; i < ncol; i++) {
        GT0(tcldlyr, i, 0) = (REAL)1.0;
        GT0(enn, i, 0) = (REAL)0.0;
        for (int k = 1; k <= nlevs; k++) {
            const REAL re1 = GT3(reff, i, k, 1), re2 = GT3(reff, i, k, 2), re4 = GT3(reff, i, k, 4);
            REAL taucld1, taucld2, taucld3, taucld4;
            if (re1 <= (REAL)0.0) taucld1 = 0;
            else taucld1 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 1)) * (IR3(aib_ir, 1) + IR3(aib_ir, 2) / POW(re1, IR3(aib_ir, 3)));
            taucld2 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 2)) *
                      (IR(awb_ir, 1) + (IR(awb_ir, 2) + (IR(awb_ir, 3) + IR(awb_ir, 4) * re2) * re2) * re2);
            taucld3 = (REAL)0.00307 * (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 3));
            const REAL reff_snow = re4 < (REAL)112.0 ? re4 : (REAL)112.0;
            if (reff_snow <= (REAL)0.0) taucld4 = 0;
            else taucld4 = (((GT2(dp, i, k) * (REAL)1.0e3) / grav) * GT3(hydromets, i, k, 4)) * (IR3(aib_ir, 1) + IR3(aib_ir, 2) / POW(reff_snow, IR3(aib_ir, 3)));
            GT3(taudiag, i, k, 1) = taucld1; GT3(taudiag, i, k, 2) = taucld2; GT3(taudiag, i, k, 3) = taucld3; GT3(taudiag, i, k, 4) = taucld4;
            REAL tauc = taucld1 + taucld2 + taucld3 + taucld4;
            if (tauc > (REAL)0.02 && GT2(fcld, i, k) > (REAL)0.01) {
                const REAL w1 = taucld1 * (IR(aiw_ir, 1) + (IR(aiw_ir, 2) + (IR(aiw_ir, 3) + IR(aiw_ir, 4) * re1) * re1) * re1);
                const REAL w2 = taucld2 * (IR(aww_ir, 1) + (IR(aww_ir, 2) + (IR(aww_ir, 3) + IR(aww_ir, 4) * re2) * re2) * re2);
                const REAL w3 = taucld3 * (REAL)0.54;
                const REAL w4 = taucld4 * (IR(aiw_ir, 1) + (IR(aiw_ir, 2) + (IR(aiw_ir, 3) + IR(aiw_ir, 4) * reff_snow) * reff_snow) * reff_snow);
                const REAL ww = (w1 + w2 + w3 + w4) / tauc;
                const REAL g1 = w1 * (IR(aig_ir, 1) + (IR(aig_ir, 2) + (IR(aig_ir, 3) + IR(aig_ir, 4) * re1) * re1) * re1);
                const REAL g2 = w2 * (IR(awg_ir, 1) + (IR(awg_ir, 2) + (IR(awg_ir, 3) + IR(awg_ir, 4) * re2) * re2) * re2);
                const REAL g3 = w3 * (REAL)0.95;
                const REAL g4 = w4 * (IR(aig_ir, 1) + (IR(aig_ir, 2) + (IR(aig_ir, 3) + IR(aig_ir, 4) * reff_snow) * reff_snow) * reff_snow);
                REAL gg;
                if (w1 + w2 + w3 + w4 != (REAL)0.0) gg = (g1 + g2 + g3 + g4) / (w1 + w2 + w3 + w4);
                else gg = (REAL)0.5;
                const REAL ff = (REAL)0.5 + ((REAL)0.3739 + ((REAL)0.0076 + (REAL)0.1185 * gg) * gg) * gg;
                const REAL sc = ((REAL)1. - ww * ff) > (REAL)0.0 ? ((REAL)1. - ww * ff) : (REAL)0.0;
                tauc = sc * tauc;
                GT0(tcldlyr, i, k) = EXP((REAL)-1.66 * tauc);
                GT0(enn, i, k) = GT2(fcld, i, k) * ((REAL)1.0 - GT0(tcldlyr, i, k));
            } else {
                GT0(tcldlyr, i, k) = (REAL)1.0;
                GT0(enn, i, k) = (REAL)0.0;
            }
        }
    }
#undef IR
#undef IR3
    return 0;
}

/* the oracle's statement of the same routines, column by column (its arrays: 1-based over k, species-major [(l-1)*(np+1)+k]; its gravity
 * is the constant 9.80665): cs_gettau gives the species SUMS of taubeam / taudiff, ch_getirtau the species */
int SFX(gtr_oracle_swtau)(int ib, int ncol, int nlevs, const REAL *coszs, const REAL *dp, const REAL *fcld, const REAL *reff,
                          const REAL *hydromets, int ict, int icb, REAL *tauclb, REAL *tauclf, REAL *asycl, REAL *ssacl)
{
    const int n1 = nlevs + 1;
    REAL *w = (REAL *)calloc((size_t)14 * n1, sizeof(REAL));
    if (!w) return 1;
    REAL *d = w, *f = w + n1, *re = w + 2 * n1, *hy = w + 6 * n1, *o = w + 10 * n1;
    for (int i = 0; i < ncol; i++) {
        for (int k = 1; k <= nlevs; k++) {
            d[k] = GT2(dp, i, k); f[k] = GT2(fcld, i, k);
            for (int l = 1; l <= 4; l++) { re[(l - 1) * n1 + k] = GT3(reff, i, k, l); hy[(l - 1) * n1 + k] = GT3(hydromets, i, k, l); }
        }
        SFX(cs_gettau)(ib, nlevs, coszs[i], d, f, re, hy, ict, icb, o, o + n1, o + 2 * n1, o + 3 * n1);
        for (int k = 1; k <= nlevs; k++) {
            GT2(tauclb, i, k) = o[k]; GT2(tauclf, i, k) = o[n1 + k]; GT2(asycl, i, k) = o[2 * n1 + k]; GT2(ssacl, i, k) = o[3 * n1 + k];
        }
    }
    free(w);
    return 0;
}

int SFX(gtr_oracle_irtau)(int ib, int ncol, int nlevs, const REAL *dp, const REAL *fcld, const REAL *reff, const REAL *hydromets,
                          REAL *taudiag, REAL *tcldlyr, REAL *enn)
{
    const int n1 = nlevs + 1;
    REAL *w = (REAL *)calloc((size_t)16 * n1, sizeof(REAL));
    if (!w) return 1;
    REAL *d = w, *f = w + n1, *re = w + 2 * n1, *hy = w + 6 * n1, *td = w + 10 * n1, *tc = w + 14 * n1, *en = w + 15 * n1;
    for (int i = 0; i < ncol; i++) {
        for (int k = 1; k <= nlevs; k++) {
            d[k] = GT2(dp, i, k); f[k] = GT2(fcld, i, k);
            for (int l = 1; l <= 4; l++) { re[(l - 1) * n1 + k] = GT3(reff, i, k, l); hy[(l - 1) * n1 + k] = GT3(hydromets, i, k, l); }
        }
        SFX(ch_getirtau)(ib, nlevs, d, f, re, hy, td, tc, en);
        for (int k = 0; k <= nlevs; k++) { GT0(tcldlyr, i, k) = tc[k]; GT0(enn, i, k) = en[k]; }
        for (int k = 1; k <= nlevs; k++)
            for (int l = 1; l <= 4; l++) GT3(taudiag, i, k, l) = td[(l - 1) * n1 + k];
    }
    free(w);
    return 0;
}

/* TAUIR, CLDTMP, CLDPRS of LW_Driver (GEOS_IrradGridComp.F90:1898-1912 cloud preparation, :3626-3650 exports) from the GEOS fields in
 * model ordering: ple (ncol,0:lm), t, q[4], r[4] (ncol,lm), radii in metres.  taucrit: the resource value. */
int SFX(gtr_lw_cloud_diag)(int ncol, int lm, REAL grav, REAL undef, REAL taucrit, const REAL *ple, const REAL *tt, const REAL *const *q,
                           const REAL *const *r, REAL *tauir, REAL *cldtmp, REAL *cldprs)
{
    const int nlevs = lm;
    const size_t cells = (size_t)ncol * lm;
    REAL *w = (REAL *)calloc(cells * 18 + (size_t)ncol * (lm + 1) * 2, sizeof(REAL));
    if (!w) return 1;
    REAL *dp = w, *fc = w + cells, *reff = w + 2 * cells, *cwc = w + 6 * cells, *td3 = w + 10 * cells, *td4 = w + 14 * cells,
         *tc = w + 18 * cells, *en = tc + (size_t)ncol * (lm + 1);
    const REAL dflt[4] = {(REAL)36.e-6, (REAL)14.e-6, (REAL)50.e-6, (REAL)50.e-6};
    for (int i = 0; i < ncol; i++)
        for (int k = 1; k <= lm; k++) {
            GT2(dp, i, k) = GT0(ple, i, k) - GT0(ple, i, k - 1);
            GT2(fc, i, k) = 0;
            for (int l = 1; l <= 4; l++) {
                REAL rad = GT2(r[l - 1], i, k);
                if (rad == undef) rad = dflt[l - 1];                 /* WHERE (RI == MAPL_UNDEF) RI = 36.e-6 ... */
                GT3(reff, i, k, l) = rad * (REAL)1.0e6;
                GT3(cwc, i, k, l) = GT2(q[l - 1], i, k);
            }
        }
    SFX(gtr_irtau)(3, ncol, lm, dp, fc, reff, cwc, grav, td3, tc, en);
    SFX(gtr_irtau)(4, ncol, lm, dp, fc, reff, cwc, grav, td4, tc, en);
    const REAL crit = taucrit / (REAL)2.13;
    for (int i = 0; i < ncol; i++) {
        cldtmp[i] = undef; cldprs[i] = undef;
        for (int k = 1; k <= lm; k++) {
            const REAL b3 = GT3(td3, i, k, 1) + GT3(td3, i, k, 2) + GT3(td3, i, k, 3) + GT3(td3, i, k, 4);
            const REAL b4 = GT3(td4, i, k, 1) + GT3(td4, i, k, 2) + GT3(td4, i, k, 3) + GT3(td4, i, k, 4);
            GT2(tauir, i, k) = (REAL)0.5 * (b3 + b4);
        }
        for (int k = lm; k >= 1; k--)                                 /* the topmost hit stays */
            if (GT2(tauir, i, k) > crit) { cldtmp[i] = GT2(tt, i, k); cldprs[i] = GT0(ple, i, k - 1); }
    }
    free(w);
    return 0;
}

#undef GT2
#undef GT3
#undef GT0
