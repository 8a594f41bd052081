/* chou_overcast_impl.h -- TEST INFRASTRUCTURE: plain-C restatement of the reference's -DOVERCAST build of the Chou-Suarez drivers
 * irrad (GEOSirrad_GridComp/irrad.F90) and sorad (GEOSsolar_GridComp/sorad.F90).  Only the driver bodies are restated, from
 * oracle/chou_oracle_impl.h / chou_sw_oracle_impl.h (their helpers - tables, getirtau, cs_gettau, cs_deledd, ... - are reused as they are),
 * with the OVERCAST branches of the reference:
 *   irrad: no mkicx (:658-665), fclr = fclr_above * tcldlyr(k2-1) in the level-pair loop (:1187-1195; fclr_above :1046, :1275);
 *          the layer emission still uses enn = fcld (1 - tcldlyr) (:908, getirtau.code:93);
 *   sorad: getvistau / getnirtau with ict = icb = 0 (:421, :955: unscaled cloud optical thickness), CLDFLXY (:556-690, :1086-1210)
 *          instead of CLDFLX.
 * Included once per precision by chou_overcast_ref.c (REAL / SFX / EXP ... defined there, as in oracle/lw_oracle.c). */

/* the oracle headers' own constants (they #undef them at their end) */
#define CH_NX 26
#define CH_NO 21
#define CH_NC 30
#define CH_NH 31
#define CH_GRAV ((REAL)9.80665)
#define CS_GRAV ((REAL)9.80665)
#define CS_DSM ((REAL)0.602)

int SFX(oc_irrad)(int m, int np, const REAL *ple, const REAL *ta, const REAL *wa, const REAL *oa, const REAL *tb, REAL co2,
                      int trace, const REAL *n2o, const REAL *ch4, const REAL *cfc11, const REAL *cfc12, const REAL *cfc22,
                      const REAL *cwc, const REAL *fcld, int ict, int icb, const REAL *reff, int ns, const REAL *fs, const REAL *tg,
                      const REAL *eg, const REAL *tv, const REAL *ev, const REAL *rv, int na, int nb, REAL *taua, REAL *ssaa,
                      REAL *asya, REAL *flxu, REAL *flcu, REAL *flau, REAL *flxau, REAL *flxd, REAL *flcd, REAL *flad, REAL *flxad,
                      REAL *dfdts, REAL *sfcem, REAL *taudiag)
{
    const SFX(chou_tables_t) *t = &SFX(CH);
    if (ns > 15) return 2;
    const int n1 = np + 1, n2 = np + 2;
    const size_t cl = (size_t)m * np;
    /* work arrays, 0-based index = the reference's index */
    REAL *W = (REAL *)calloc((size_t)64 * n2 + (size_t)17 * n1 + 16 * n1, sizeof(REAL));
    REAL *p = W;
#define TAKE(n) (p += (n), p - (n))
    REAL *pa = TAKE(n2), *dt = TAKE(n2), *dp = TAKE(n2), *dp_pa = TAKE(n2), *dh2o = TAKE(n2), *dcont = TAKE(n2), *dco2 = TAKE(n2),
         *do3 = TAKE(n2), *dn2o = TAKE(n2), *dch4 = TAKE(n2), *df11 = TAKE(n2), *df12 = TAKE(n2), *df22 = TAKE(n2);
    REAL *blayer = TAKE(n2), *blevel = TAKE(n2), *dd = TAKE(n2), *du = TAKE(n2), *cd = TAKE(n2), *cu = TAKE(n2), *bd = TAKE(n2),
         *bu = TAKE(n2), *ad = TAKE(n2), *au = TAKE(n2);
    REAL *transfc = TAKE(n2), *transfca = TAKE(n2), *trantcr = TAKE(n2), *trantca = TAKE(n2);
    REAL *flau_c = TAKE(n2), *flad_c = TAKE(n2), *flcu_c = TAKE(n2), *flcd_c = TAKE(n2), *flxu_c = TAKE(n2), *flxd_c = TAKE(n2),
         *flxau_c = TAKE(n2), *flxad_c = TAKE(n2);
    REAL *taerlyr = TAKE(n2), *enn = TAKE(n2), *tcldlyr = TAKE(n2), *fcld_c = TAKE(n2);
    REAL *exptbl = TAKE((size_t)17 * n1);              /* exptbl[(j-1)*n1 + k], k = 0..np, j = 1..17 */
    REAL *reff_c = TAKE((size_t)4 * n1), *cwc_c = TAKE((size_t)4 * n1), *taud = TAKE((size_t)4 * n1);
#undef TAKE
#define EX(k, j) exptbl[(size_t)((j) - 1) * n1 + (k)]
#define A2(a, k) a[(size_t)((k) - 1) * m + i]               /* Fortran a(i,k) */

    for (int i = 0; i < m; i++) {
        for (int k = 1; k <= np; k++) {
            pa[k] = (REAL)0.5 * (A2(ple, k + 1) + A2(ple, k)) * (REAL)0.01;
            dp[k] = (A2(ple, k + 1) - A2(ple, k)) * (REAL)0.01;
            dp_pa[k] = A2(ple, k + 1) - A2(ple, k);
            dt[k] = A2(ta, k) - (REAL)250.0;
            dh2o[k] = (REAL)1.02 * A2(wa, k) * dp[k];
            do3[k] = (REAL)476. * A2(oa, k) * dp[k];
            dco2[k] = (REAL)789. * co2 * dp[k];
            dch4[k] = (REAL)789. * A2(ch4, k) * dp[k];
            dn2o[k] = (REAL)789. * A2(n2o, k) * dp[k];
            df11[k] = (REAL)789. * A2(cfc11, k) * dp[k];
            df12[k] = (REAL)789. * A2(cfc12, k) * dp[k];
            df22[k] = (REAL)789. * A2(cfc22, k) * dp[k];
            if (dh2o[k] < (REAL)1.e-10) dh2o[k] = (REAL)1.e-10;
            if (do3[k] < (REAL)1.e-6) do3[k] = (REAL)1.e-6;
            if (dco2[k] < (REAL)1.e-4) dco2[k] = (REAL)1.e-4;
            const REAL xx = pa[k] * (REAL)0.001618 * A2(wa, k) * A2(wa, k) * dp[k];
            dcont[k] = xx * EXP((REAL)1800. / A2(ta, k) - (REAL)6.081);
            fcld_c[k] = A2(fcld, k);
            for (int l = 0; l < 4; l++) {
                reff_c[l * n1 + k] = reff[((size_t)l * np + (k - 1)) * m + i];
                cwc_c[l * n1 + k] = cwc[((size_t)l * np + (k - 1)) * m + i];
            }
        }
        /* layer 0 above the model top (:432-453) */
        dp[0] = A2(ple, 1) * (REAL)0.01 > (REAL)0.005 ? A2(ple, 1) * (REAL)0.01 : (REAL)0.005;
        pa[0] = (REAL)0.5 * dp[0];
        dt[0] = A2(ta, 1) - (REAL)250.0;
        dh2o[0] = (REAL)1.02 * A2(wa, 1) * dp[0];
        do3[0] = (REAL)476. * A2(oa, 1) * dp[0];
        dco2[0] = (REAL)789. * co2 * dp[0];
        dch4[0] = (REAL)789. * A2(ch4, 1) * dp[0];
        dn2o[0] = (REAL)789. * A2(n2o, 1) * dp[0];
        df11[0] = (REAL)789. * A2(cfc11, 1) * dp[0];
        df12[0] = (REAL)789. * A2(cfc12, 1) * dp[0];
        df22[0] = (REAL)789. * A2(cfc22, 1) * dp[0];
        if (dh2o[0] < (REAL)1.e-10) dh2o[0] = (REAL)1.e-10;
        if (do3[0] < (REAL)1.e-6) do3[0] = (REAL)1.e-6;
        if (dco2[0] < (REAL)1.e-4) dco2[0] = (REAL)1.e-4;
        {
            const REAL xx = pa[0] * (REAL)0.001618 * A2(wa, 1) * A2(wa, 1) * dp[0];
            dcont[0] = xx * EXP((REAL)1800. / A2(ta, 1) - (REAL)6.081);
        }
        sfcem[i] = 0;
        transfc[np + 1] = 1; transfca[np + 1] = 1; trantcr[np + 1] = 1; trantca[np + 1] = 1;
        for (int k = 1; k <= np + 1; k++) {
            A2(flxu, k) = 0; A2(flxau, k) = 0; A2(flcu, k) = 0; A2(flau, k) = 0; A2(flxd, k) = 0; A2(flxad, k) = 0; A2(flcd, k) = 0;
            A2(flad, k) = 0; A2(dfdts, k) = 0;
        }
        for (int l = 0; l < 10; l++) for (int k = 1; k <= np; k++) taudiag[((size_t)l * np + (k - 1)) * m + i] = 0;

        for (int ibn = 1; ibn <= 10; ibn++) {
            /* the reference `return`s here (irrad.F90:478), i.e. stops after the first column when trace is false; GEOS always
             * passes trace = .true. (GEOS_IrradGridComp.F90:1487) -- band 10 is simply skipped here */
            if (ibn == 10 && !trace) break;
            {   /* test hook: ORACLE_CHOU_BAND=n keeps band n only (per-band comparison with the tables of the technical memoranda) */
                const char *only = getenv("ORACLE_CHOU_BAND");
                if (only && atoi(only) != ibn) continue;
            }
            const int h2otable = ibn == 1 || ibn == 2 || ibn == 8, conbnd = ibn >= 2 && ibn <= 7, co2bnd = ibn == 3, oznbnd = ibn == 5,
                      n2obnd = ibn == 6 || ibn == 7, ch4bnd = n2obnd, combnd = ibn == 4 || ibn == 5, f11bnd = combnd,
                      f12bnd = ibn == 4 || ibn == 6, f22bnd = f12bnd, b10bnd = ibn == 10, do_aerosol = na > 0;
            memset(exptbl, 0, (size_t)17 * n1 * sizeof(REAL));
            /* packing of the exponential tables by band (:501-566) */
            int h2o_s = 0, con_s = 0, co2_s = 0, n2o_s = 0, ch4_s = 0, com_s = 0, f11_s = 0, f12_s = 0, f22_s = 0;
            switch (ibn) {
                case 2: con_s = 1; break;
                case 3: h2o_s = 1; con_s = 7; break;
                case 4: h2o_s = 1; con_s = 7; com_s = 8; f11_s = 14; f12_s = 15; f22_s = 16; break;
                case 5: h2o_s = 1; con_s = 7; com_s = 8; f11_s = 14; break;
                case 6: h2o_s = 1; con_s = 7; n2o_s = 8; ch4_s = 12; f12_s = 16; f22_s = 17; break;
                case 7: h2o_s = 1; con_s = 7; n2o_s = 8; ch4_s = 12; break;
                case 9: h2o_s = 1; break;
                case 10: h2o_s = 1; con_s = 6; co2_s = 7; n2o_s = 13; break;
                default: break;
            }
            for (int k = 1; k <= np; k++) blayer[k] = SFX(ch_planck)(ibn, A2(ta, k));
            blayer[0] = blayer[1]; blevel[0] = blayer[1];
            REAL bs, dbs, rflxs;
            SFX(ch_sfcflux)(ibn, m, i, ns, fs, tg, eg, tv, ev, rv, &bs, &dbs, &rflxs);
            blayer[np + 1] = bs;
            for (int k = 2; k <= np; k++) blevel[k] = (blayer[k - 1] * dp[k] + blayer[k] * dp[k - 1]) / (dp[k - 1] + dp[k]);
            blevel[1] = blayer[1] + (blayer[1] - blayer[2]) * dp[1] / (dp[1] + dp[2]);
            blevel[0] = blevel[1];
            blevel[np + 1] = SFX(ch_planck)(ibn, tb[i]);
            SFX(ch_getirtau)(ibn, np, dp_pa, fcld_c, reff_c, cwc_c, taud, tcldlyr, enn);
            for (int k = 1; k <= np; k++)
                taudiag[((size_t)(ibn - 1) * np + (k - 1)) * m + i] += taud[0 * n1 + k] + taud[1 * n1 + k] + taud[2 * n1 + k] + taud[3 * n1 + k];
            /* OVERCAST: no icx / mkicx (irrad.F90:658-665) */
            /* aerosol scaling, in place as in the reference (:655-678) */
            if (do_aerosol) {
                taerlyr[0] = 1;
                for (int k = 1; k <= np; k++) {
                    const size_t j = ((size_t)(ibn - 1) * np + (k - 1)) * m + i;
                    taerlyr[k] = 1;
                    if (taua[j] > (REAL)0.001) {
                        if (ssaa[j] > (REAL)0.001) {
                            asya[j] = asya[j] / ssaa[j];
                            ssaa[j] = ssaa[j] / taua[j];
                            const REAL ff = (REAL).5 + ((REAL).3739 + ((REAL)0.0076 + (REAL)0.1185 * asya[j]) * asya[j]) * asya[j];
                            taua[j] = taua[j] * ((REAL)1. - ssaa[j] * ff);
                        }
                        taerlyr[k] = EXP((REAL)-1.66 * taua[j]);
                    }
                }
            }
            /* exponentials of the k-distribution terms per layer (:684-780; helpers :1379-1884) */
            if (!h2otable && !b10bnd) {
                for (int k = 0; k <= np; k++) {
                    REAL xh = dh2o[k] * POW(pa[k] / (REAL)500., t->pm[ibn - 1]) * ((REAL)1. + (t->aw[ibn - 1] + t->bw[ibn - 1] * dt[k]) * dt[k]);
                    EX(k, h2o_s) = EXP(-xh * t->xkw[ibn - 1]);
                    for (int ik = 2; ik <= 6; ik++) {
                        const REAL e = EX(k, h2o_s + ik - 2);
                        const int mwv = t->mw[ibn - 1];
                        if (mwv == 6) { xh = e * e; EX(k, h2o_s + ik - 1) = xh * xh * xh; }
                        else if (mwv == 8) { xh = e * e; xh = xh * xh; EX(k, h2o_s + ik - 1) = xh * xh; }
                        else if (mwv == 9) { xh = e * e * e; EX(k, h2o_s + ik - 1) = xh * xh * xh; }
                        else { xh = e * e; xh = xh * xh; xh = xh * xh; EX(k, h2o_s + ik - 1) = xh * xh; }
                    }
                }
            }
            int ne = 0;
            if (conbnd) {
                ne = 1; if (ibn == 3) ne = 3;
                for (int k = 0; k <= np; k++) {
                    EX(k, con_s) = EXP(-dcont[k] * t->xke[ibn - 1]);
                    if (ibn == 3) { EX(k, con_s + 1) = EX(k, con_s) * EX(k, con_s); EX(k, con_s + 2) = EX(k, con_s + 1) * EX(k, con_s + 1); }
                }
            }
            if (trace) {
                if (n2obnd)
                    for (int k = 0; k <= np; k++) {
                        if (ibn == 6) {
                            REAL xc = dn2o[k] * ((REAL)1. + ((REAL)1.9297e-3 + (REAL)4.3750e-6 * dt[k]) * dt[k]);
                            EX(k, n2o_s) = EXP(-xc * (REAL)6.31582e-2);
                            xc = EX(k, n2o_s) * EX(k, n2o_s) * EX(k, n2o_s);
                            const REAL xc1 = xc * xc, xc2 = xc1 * xc1;
                            EX(k, n2o_s + 1) = xc * xc1 * xc2;
                        } else {
                            REAL xc = dn2o[k] * POW(pa[k] / (REAL)500.0, (REAL)0.48) * ((REAL)1. + ((REAL)1.3804e-3 + (REAL)7.4838e-6 * dt[k]) * dt[k]);
                            EX(k, n2o_s) = EXP(-xc * (REAL)5.35779e-2);
                            for (int q = 1; q <= 3; q++) { xc = EX(k, n2o_s + q - 1) * EX(k, n2o_s + q - 1); xc = xc * xc; EX(k, n2o_s + q) = xc * xc; }
                        }
                    }
                if (ch4bnd)
                    for (int k = 0; k <= np; k++) {
                        if (ibn == 6) {
                            const REAL xc = dch4[k] * ((REAL)1. + ((REAL)1.7007e-2 + (REAL)1.5826e-4 * dt[k]) * dt[k]);
                            EX(k, ch4_s) = EXP(-xc * (REAL)5.80708e-3);
                        } else {
                            REAL xc = dch4[k] * POW(pa[k] / (REAL)500.0, (REAL)0.65) * ((REAL)1. + ((REAL)5.9590e-4 - (REAL)2.2931e-6 * dt[k]) * dt[k]);
                            EX(k, ch4_s) = EXP(-xc * (REAL)6.29247e-2);
                            for (int q = 1; q <= 3; q++) {
                                xc = EX(k, ch4_s + q - 1) * EX(k, ch4_s + q - 1) * EX(k, ch4_s + q - 1); xc = xc * xc; EX(k, ch4_s + q) = xc * xc;
                            }
                        }
                    }
                if (combnd)
                    for (int k = 0; k <= np; k++) {
                        REAL xc;
                        if (ibn == 4) xc = dco2[k] * ((REAL)1. + ((REAL)3.5775e-2 + (REAL)4.0447e-4 * dt[k]) * dt[k]);
                        else xc = dco2[k] * ((REAL)1. + ((REAL)3.4268e-2 + (REAL)3.7401e-4 * dt[k]) * dt[k]);
                        EX(k, com_s) = EXP(-xc * (REAL)1.922e-7);
                        for (int ik = 2; ik <= 6; ik++) { xc = EX(k, com_s + ik - 2) * EX(k, com_s + ik - 2); xc = xc * xc; EX(k, com_s + ik - 1) = xc * EX(k, com_s + ik - 2); }
                    }
                /* CFCs, Table 7 (:723-766): band 4 uses (a1,b1,fk1), the other band (a2,b2,fk2) */
                static const double cf11[6] = {1.26610e-3, 3.55940e-6, 1.89736e+1, 8.19370e-4, 4.67810e-6, 1.01487e+1};
                static const double cf12[6] = {8.77370e-4, -5.88440e-6, 1.58104e+1, 8.62000e-4, -4.22500e-6, 3.70107e+1};
                static const double cf22[6] = {9.65130e-4, 1.31280e-5, 6.18536e+0, -3.00010e-5, 5.25010e-7, 3.27912e+1};
                for (int q = 0; q < 3; q++) {
                    const int on = q == 0 ? f11bnd : (q == 1 ? f12bnd : f22bnd), s = q == 0 ? f11_s : (q == 1 ? f12_s : f22_s);
                    const double *c = q == 0 ? cf11 : (q == 1 ? cf12 : cf22);
                    const REAL *dcfc = q == 0 ? df11 : (q == 1 ? df12 : df22);
                    if (!on) continue;
                    const int o = ibn == 4 ? 0 : 3;
                    for (int k = 0; k <= np; k++) {
                        const REAL xf = dcfc[k] * ((REAL)1. + ((REAL)c[o] + (REAL)c[o + 1] * dt[k]) * dt[k]);
                        EX(k, s) = EXP(-xf * (REAL)c[o + 2]);
                    }
                }
                if (b10bnd)
                    for (int k = 0; k <= np; k++) {
                        REAL xx = dh2o[k] * (pa[k] / (REAL)500.0) * ((REAL)1. + ((REAL)0.0149 + (REAL)6.20e-5 * dt[k]) * dt[k]);
                        EX(k, h2o_s) = EXP(-xx * (REAL)0.10624);
                        for (int q = 1; q <= 4; q++) { xx = EX(k, h2o_s + q - 1) * EX(k, h2o_s + q - 1); xx = xx * xx; EX(k, h2o_s + q) = xx * xx; }
                        EX(k, con_s) = EXP(-dcont[k] * (REAL)109.0);
                        xx = dco2[k] * POW(pa[k] / (REAL)300.0, (REAL)0.5) * ((REAL)1. + ((REAL)0.0179 + (REAL)1.02e-4 * dt[k]) * dt[k]);
                        EX(k, co2_s) = EXP(-xx * (REAL)2.656e-5);
                        for (int q = 1; q <= 5; q++) { xx = EX(k, co2_s + q - 1) * EX(k, co2_s + q - 1); xx = xx * xx; EX(k, co2_s + q) = xx * xx; }
                        xx = dn2o[k] * ((REAL)1. + ((REAL)1.4476e-3 + (REAL)3.6656e-6 * dt[k]) * dt[k]);
                        EX(k, n2o_s) = EXP(-xx * (REAL)0.25238);
                        xx = EX(k, n2o_s) * EX(k, n2o_s);
                        REAL xx1 = xx * xx; xx1 = xx1 * xx1;
                        const REAL xx2 = xx1 * xx1, xx3 = xx2 * xx2;
                        EX(k, n2o_s + 1) = xx * xx1 * xx2 * xx3;
                    }
            }
            bu[0] = 0; bd[0] = blayer[1]; bu[np + 1] = blayer[np + 1];
            au[0] = 0; ad[0] = blayer[1]; au[np + 1] = blayer[np + 1];
            cu[0] = 0; cd[0] = blayer[1]; cu[np + 1] = blayer[np + 1];
            du[0] = 0; dd[0] = blayer[1]; du[np + 1] = blayer[np + 1];

            /* transmittance of one layer km added to the running state (the shared body of loops 1500 and 3000) */
            REAL th2o[6], tcon[3], tco2[6], tn2o[4], tch4[4], tcom[6], tf11 = 1, tf12 = 1, tf22 = 1, x1, x2, x3;
#define LAYER_TRAN(km, full, trant)                                                                                          \
    do {                                                                                                                      \
        if (h2otable) {                                                                                                       \
            const REAL *ha = ibn == 1 ? t->h11 : (ibn == 2 ? t->h21 : t->h81), *hb = ibn == 1 ? t->h12 : (ibn == 2 ? t->h22 : t->h82),   \
                       *hc = ibn == 1 ? t->h13 : (ibn == 2 ? t->h23 : t->h83);                                                \
            SFX(ch_tablup)(CH_NX, CH_NH, dh2o[km], pa[km], dt[km], &x1, &x2, &x3, *t->w11, *t->p11, *t->dwe, *t->dpe, ha, hb, hc, &trant); \
            if (conbnd) { tcon[0] = tcon[0] * EX(km, con_s); trant = trant * tcon[0]; }                                     \
        } else if (!b10bnd) {                                                                                                 \
            for (int q = 0; q < 6; q++) th2o[q] = th2o[q] * EX(km, h2o_s + q);                                               \
            REAL trn;                                                                                                         \
            if (ne == 0) {                                                                                                    \
                trn = 0; for (int q = 0; q < 6; q++) trn = trn + F2(t->fkw, 6, q + 1, ibn) * th2o[q];                       \
            } else if (ne == 1) {                                                                                             \
                tcon[0] = tcon[0] * EX(km, con_s);                                                                          \
                trn = 0; for (int q = 0; q < 6; q++) trn = trn + F2(t->fkw, 6, q + 1, ibn) * th2o[q];                       \
                trn = trn * tcon[0];                                                                                          \
            } else {                                                                                                          \
                for (int q = 0; q < 3; q++) tcon[q] = tcon[q] * EX(km, con_s + q);                                          \
                trn = 0;                                                                                                      \
                for (int sb = 1; sb <= 3; sb++) {                                                                             \
                    REAL s = 0; for (int q = 0; q < 6; q++) s = s + F2(t->gkw, 6, q + 1, sb) * th2o[q];                     \
                    trn = trn + s * tcon[sb - 1];                                                                             \
                }                                                                                                             \
            }                                                                                                                 \
            trant = trant * trn;                                                                                              \
        }                                                                                                                     \
        if (co2bnd) SFX(ch_tablup)(CH_NX, CH_NC, dco2[km], pa[km], dt[km], &x1, &x2, &x3, *t->w12, *t->p12, *t->dwe, *t->dpe, t->c1, t->c2, t->c3, &trant); \
        if (oznbnd) SFX(ch_tablup)(CH_NX, CH_NO, do3[km], pa[km], dt[km], &x1, &x2, &x3, *t->w13, *t->p13, *t->dwe, *t->dpe, t->oo1, t->oo2, t->oo3, &trant); \
        if ((full) && trace) {                                                                                                \
            if (n2obnd) {                                                                                                     \
                REAL xc;                                                                                                      \
                if (ibn == 6) { tn2o[0] *= EX(km, n2o_s); xc = (REAL)0.940414 * tn2o[0]; tn2o[1] *= EX(km, n2o_s + 1); xc = xc + (REAL)0.059586 * tn2o[1]; } \
                else { static const double w[4] = {0.561961, 0.138707, 0.240670, 0.058662}; xc = 0;                          \
                       for (int q = 0; q < 4; q++) { tn2o[q] *= EX(km, n2o_s + q); xc = xc + (REAL)w[q] * tn2o[q]; } }       \
                trant = trant * xc;                                                                                           \
            }                                                                                                                 \
            if (ch4bnd) {                                                                                                     \
                REAL xc;                                                                                                      \
                if (ibn == 6) { tch4[0] *= EX(km, ch4_s); xc = tch4[0]; }                                                    \
                else { static const double w[4] = {0.610650, 0.280212, 0.107349, 0.001789}; xc = 0;                          \
                       for (int q = 0; q < 4; q++) { tch4[q] *= EX(km, ch4_s + q); xc = xc + (REAL)w[q] * tch4[q]; } }       \
                trant = trant * xc;                                                                                           \
            }                                                                                                                 \
            if (combnd) {                                                                                                     \
                static const double w4[6] = {0.12159, 0.24359, 0.24981, 0.26427, 0.07807, 0.04267};                           \
                static const double w5[6] = {0.06869, 0.14795, 0.19512, 0.33446, 0.17199, 0.08179};                           \
                const double *w = ibn == 4 ? w4 : w5; REAL xc = 0;                                                            \
                for (int q = 0; q < 6; q++) { tcom[q] *= EX(km, com_s + q); xc = xc + (REAL)w[q] * tcom[q]; }                \
                trant = trant * xc;                                                                                           \
            }                                                                                                                 \
            if (f11bnd) { tf11 = tf11 * EX(km, f11_s); trant = trant * tf11; }                                              \
            if (f12bnd) { tf12 = tf12 * EX(km, f12_s); trant = trant * tf12; }                                              \
            if (f22bnd) { tf22 = tf22 * EX(km, f22_s); trant = trant * tf22; }                                              \
            if (b10bnd) {                                                                                                     \
                static const double wh[5] = {0.3153, 0.4604, 0.1326, 0.0798, 0.0119};                                         \
                static const double wc[6] = {0.2673, 0.2201, 0.2106, 0.2409, 0.0196, 0.0415};                                 \
                REAL xx = 0; for (int q = 0; q < 5; q++) { th2o[q] *= EX(km, h2o_s + q); xx = xx + (REAL)wh[q] * th2o[q]; }  \
                trant = xx;                                                                                                   \
                tcon[0] = tcon[0] * EX(km, con_s); trant = trant * tcon[0];                                                 \
                xx = 0; for (int q = 0; q < 6; q++) { tco2[q] *= EX(km, co2_s + q); xx = xx + (REAL)wc[q] * tco2[q]; }       \
                trant = trant * xx;                                                                                           \
                tn2o[0] *= EX(km, n2o_s); xx = (REAL)0.970831 * tn2o[0]; tn2o[1] *= EX(km, n2o_s + 1); xx = xx + (REAL)0.029169 * tn2o[1]; \
                trant = trant * (xx - (REAL)1.0);                                                                             \
            }                                                                                                                 \
        }                                                                                                                     \
    } while (0)

            /* loop 1500 (:802-935): emission of the single layer k2-1 */
            for (int k2 = 1; k2 <= np + 1; k2++) {
                if (!h2otable) for (int q = 0; q < 6; q++) th2o[q] = 1;
                tcon[0] = tcon[1] = tcon[2] = 1;
                x1 = 0; x2 = 0; x3 = 0;
                REAL trant = 1;
                const int km = k2 - 1;
                LAYER_TRAN(km, 0, trant);
                const REAL taant = trant;
                if (do_aerosol) trant = trant * taerlyr[km];
                SFX(ch_emis)(((REAL)1. - enn[km]) * trant, blevel[km], blevel[k2], &bd[km], &bu[km]);
                if (do_aerosol) SFX(ch_emis)(((REAL)1. - enn[km]) * taant, blevel[km], blevel[k2], &dd[km], &du[km]);
                else { dd[km] = bd[km]; du[km] = bu[km]; }
                SFX(ch_emis)(trant, blevel[km], blevel[k2], &cd[km], &cu[km]);
                if (do_aerosol) SFX(ch_emis)(taant, blevel[km], blevel[k2], &ad[km], &au[km]);
                else { ad[km] = cd[km]; au[km] = cu[km]; }
            }
            for (int k = 0; k <= np + 1; k++) { flxu_c[k] = 0; flxd_c[k] = 0; flxau_c[k] = 0; flxad_c[k] = 0; flcu_c[k] = 0; flcd_c[k] = 0; flau_c[k] = 0; flad_c[k] = 0; }

            /* loop 2000 (:948-1290): transmittance between levels k1 and k2, fluxes */
            for (int k1 = 0; k1 <= np; k1++) {
                REAL tranal = 1;
                if (!h2otable) for (int q = 0; q < 6; q++) th2o[q] = 1;
                tcon[0] = tcon[1] = tcon[2] = 1;
                if (trace) {
                    if (n2obnd) for (int q = 0; q < 4; q++) tn2o[q] = 1;
                    if (ch4bnd) for (int q = 0; q < 4; q++) tch4[q] = 1;
                    if (combnd) for (int q = 0; q < 6; q++) tcom[q] = 1;
                    if (f11bnd) tf11 = 1;
                    if (f12bnd) tf12 = 1;
                    if (f22bnd) tf22 = 1;
                    if (b10bnd) { for (int q = 0; q < 6; q++) { th2o[q] = 1; tco2[q] = 1; } tcon[0] = 1; for (int q = 0; q < 4; q++) tn2o[q] = 1; }
                }
                x1 = 0; x2 = 0; x3 = 0;
                REAL taant = 1, trant = 1, fclr = 1, fclr_above = 1;     /* fclr_above = 1.0 (:1046) */
                for (int k2 = k1 + 1; k2 <= np + 1; k2++) {
                    taant = 1; trant = 1; fclr = 1;
                    const int km = k2 - 1;
                    LAYER_TRAN(km, 1, trant);
                    taant = trant;
                    if (do_aerosol) { tranal = tranal * taerlyr[km]; trant = trant * tranal; }
                    fclr = fclr_above * tcldlyr[km];                        /* OVERCAST (:1193-1195) */
                    if (k2 == k1 + 1 && ibn != 10) {
                        flau_c[k1] -= au[k1]; flad_c[k2] += ad[k1]; flcu_c[k1] -= cu[k1]; flcd_c[k2] += cd[k1];
                        flxu_c[k1] -= bu[k1]; flxd_c[k2] += bd[k1]; flxau_c[k1] -= du[k1]; flxad_c[k2] += dd[k1];
                    }
                    REAL xx = trant * (bu[k2 - 1] - bu[k2]);
                    flxu_c[k1] = flxu_c[k1] + xx * fclr;
                    if (do_aerosol) xx = taant * (du[k2 - 1] - du[k2]);
                    flxau_c[k1] = flxau_c[k1] + xx * fclr;
                    xx = trant * (cu[k2 - 1] - cu[k2]);
                    flcu_c[k1] = flcu_c[k1] + xx;
                    if (do_aerosol) xx = taant * (au[k2 - 1] - au[k2]);
                    flau_c[k1] = flau_c[k1] + xx;
                    if (k1 == 0) xx = -trant * bd[k1]; else xx = trant * (bd[k1 - 1] - bd[k1]);
                    flxd_c[k2] = flxd_c[k2] + xx * fclr;
                    if (do_aerosol) { if (k1 == 0) xx = -taant * dd[k1]; else xx = taant * (dd[k1 - 1] - dd[k1]); }
                    flxad_c[k2] = flxad_c[k2] + xx * fclr;
                    if (k1 == 0) xx = -trant * cd[k1]; else xx = trant * (cd[k1 - 1] - cd[k1]);
                    flcd_c[k2] = flcd_c[k2] + xx;
                    if (do_aerosol) { if (k1 == 0) xx = -taant * ad[k1]; else xx = taant * (ad[k1 - 1] - ad[k1]); }
                    flad_c[k2] = flad_c[k2] + xx;
                    fclr_above = fclr;                                      /* (:1275) */
                }
                trantca[k1] = taant; trantcr[k1] = trant; transfc[k1] = trant * fclr; transfca[k1] = taant * fclr;
                if (k1 > 0) A2(dfdts, k1) = A2(dfdts, k1) - dbs * transfc[k1];
            }
#undef LAYER_TRAN
            if (!b10bnd) {
                flau_c[np + 1] = -blayer[np + 1]; flcu_c[np + 1] = -blayer[np + 1]; flxu_c[np + 1] = -blayer[np + 1]; flxau_c[np + 1] = -blayer[np + 1];
                sfcem[i] = sfcem[i] - blayer[np + 1];
                A2(dfdts, np + 1) = A2(dfdts, np + 1) - dbs;
                for (int k = 1; k <= np + 1; k++) {
                    flau_c[k] = flau_c[k] - flad_c[np + 1] * trantca[k] * rflxs;
                    flcu_c[k] = flcu_c[k] - flcd_c[np + 1] * trantcr[k] * rflxs;
                    flxu_c[k] = flxu_c[k] - flxd_c[np + 1] * transfc[k] * rflxs;
                    flxau_c[k] = flxau_c[k] - flxad_c[np + 1] * transfca[k] * rflxs;
                }
            }
            for (int k = 1; k <= np + 1; k++) {
                A2(flau, k) += flau_c[k]; A2(flcu, k) += flcu_c[k]; A2(flxu, k) += flxu_c[k]; A2(flxau, k) += flxau_c[k];
                A2(flad, k) += flad_c[k]; A2(flcd, k) += flcd_c[k]; A2(flxd, k) += flxd_c[k]; A2(flxad, k) += flxad_c[k];
            }
        }
    }
    (void)cl; (void)nb;
    free(W);
    return 0;
#undef EX
#undef A2
}

/* "Inline CLDFLXY" (sorad.F90:556-690 = :1086-1210): the clear (ih = 1: fclr, fupc) and the cloudy (ih = 2: fall, fupa, fsdir, fsdif)
 * portion of every layer, one adding chain each.  rr, tt, td, rs, ts as in cs_cldflx: [k * 2 + ih - 1]. */
static void SFX(cs_cldflxy)(int np, const REAL *rr, const REAL *tt, const REAL *td, const REAL *rs, const REAL *ts, REAL *W, REAL *fclr,
                            REAL *fall, REAL *fupc, REAL *fupa, REAL *fsdir, REAL *fsdif)
{
    REAL *rra = W, *rxa = W + (np + 2);
#define L2(a, k, i) a[(k) * 2 + (i) - 1]
    REAL fdndir = 0, fdndif = 0;
    for (int ih = 1; ih <= 2; ih++) {
        rra[np + 1] = L2(rr, np + 1, ih);
        rxa[np + 1] = L2(rs, np + 1, ih);
        for (int k = np; k >= 0; k--) {
            const REAL denm = L2(ts, k, ih) / ((REAL)1. - L2(rs, k, ih) * rxa[k + 1]);
            rra[k] = L2(rr, k, ih) + (L2(td, k, ih) * rra[k + 1] + (L2(tt, k, ih) - L2(td, k, ih)) * rxa[k + 1]) * denm;
            rxa[k] = L2(rs, k, ih) + L2(ts, k, ih) * rxa[k + 1] * denm;
        }
        REAL tdaold = L2(td, 0, ih), ttaold = L2(tt, 0, ih), rsaold = L2(rs, 0, ih);
        for (int k = 1; k <= np + 1; k++) {
            REAL tdanew = 0, ttanew = 0, rsanew = 0;
            if (k <= np) {
                const REAL denm = L2(ts, k, ih) / ((REAL)1. - rsaold * L2(rs, k, ih));
                tdanew = tdaold * L2(td, k, ih);
                ttanew = tdaold * L2(tt, k, ih) + (tdaold * rsaold * L2(rr, k, ih) + ttaold - tdaold) * denm;
                rsanew = L2(rs, k, ih) + L2(ts, k, ih) * rsaold * denm;
            }
            const REAL denm = (REAL)1. / ((REAL)1. - rsaold * rxa[k]);
            fdndir = tdaold;
            const REAL xx4 = tdaold * rra[k], yy = ttaold - tdaold;
            fdndif = (xx4 * rsaold + yy) * denm;
            const REAL fupdif = (xx4 + yy * rxa[k]) * denm;
            const REAL flxdn = fdndir + fdndif - fupdif;
            if (ih == 1) { fupc[k] = fupdif; fclr[k] = flxdn; }
            else { fupa[k] = fupdif; fall[k] = flxdn; }
            tdaold = tdanew; ttaold = ttanew; rsaold = rsanew;
        }
    }
    *fsdir = fdndir;              /* the ih = 2 chain's surface values (:689-690) */
    *fsdif = fdndif;
#undef L2
}

int SFX(oc_sorad)(int m, int np, int nb, const REAL *cosz, const REAL *pl, const REAL *ta, const REAL *wa, const REAL *oa, REAL co2,
                      const REAL *cwc, const REAL *fcld, int ict, int icb, const REAL *reff, const REAL *hk_uv, const REAL *hk_ir,
                      const REAL *taua, const REAL *ssaa, const REAL *asya, const REAL *rsuvbm, const REAL *rsuvdf, const REAL *rsirbm,
                      const REAL *rsirdf, REAL *flx, REAL *flc, REAL *fdiruv, REAL *fdifuv, REAL *fdirpar, REAL *fdifpar, REAL *fdirir,
                      REAL *fdifir, REAL *flxu, REAL *flcu, REAL *flx_sfc_band, int do_drfband, REAL *drband, REAL *dfband)
{
    const SFX(chsw_tables_t) *t = &SFX(CS);
    const int n1 = np + 1, n2 = np + 2;
    REAL *W = (REAL *)calloc((size_t)60 * n2, sizeof(REAL));
    REAL *p = W;
#define TAKE(n) (p += (n), p - (n))
    REAL *dp = TAKE(n2), *dp_pa = TAKE(n2), *wh = TAKE(n2), *oh = TAKE(n2), *scal = TAKE(n2), *swh = TAKE(n2), *so2 = TAKE(n2), *df = TAKE(n2);
    REAL *tauclb = TAKE(n2), *tauclf = TAKE(n2), *asycl = TAKE(n2), *ssacl = TAKE(n2), *fcld_c = TAKE(n2);
    REAL *reff_c = TAKE(4 * n1), *cwc_c = TAKE(4 * n1);
    REAL *rr = TAKE(2 * n2), *tt = TAKE(2 * n2), *td = TAKE(2 * n2), *rs = TAKE(2 * n2), *ts = TAKE(2 * n2);
    REAL *fall = TAKE(n2), *fclr = TAKE(n2), *fupa = TAKE(n2), *fupc = TAKE(n2);
    REAL *CW = TAKE(20 * n2);
#undef TAKE
#define A2(a, k) a[(size_t)((k) - 1) * m + i]
#define A3B(a, k, ib) a[((size_t)((ib) - 1) * np + ((k) - 1)) * m + i]
    (void)nb;
    for (int i = 0; i < m; i++) {
        int ntop = 0;
        const REAL cz = cosz[i];
        const REAL snt = (REAL)1.0 / cz;
        const REAL xtoa = A2(pl, 1) > (REAL)1.e-3 ? A2(pl, 1) : (REAL)1.e-3;
        const REAL scal0 = xtoa * POW((REAL)0.5 * xtoa / (REAL)300., (REAL).8);
        const REAL o3toa = (REAL)1.02 * A2(oa, 1) * xtoa * (REAL)466.7 + (REAL)1.0e-8;
        const REAL wvtoa = (REAL)1.02 * A2(wa, 1) * scal0 * ((REAL)1.0 + (REAL)0.00135 * (A2(ta, 1) - (REAL)240.)) + (REAL)1.0e-9;
        swh[1] = wvtoa;
        for (int k = 1; k <= np; k++) {
            dp[k] = A2(pl, k + 1) - A2(pl, k);
            dp_pa[k] = dp[k] * (REAL)100.;
            const REAL pa = (REAL)0.5 * (A2(pl, k) + A2(pl, k + 1));
            scal[k] = dp[k] * POW(pa / (REAL)300., (REAL).8);
            wh[k] = (REAL)1.02 * A2(wa, k) * scal[k] * ((REAL)1. + (REAL)0.00135 * (A2(ta, k) - (REAL)240.)) + (REAL)1.e-9;
            swh[k + 1] = swh[k] + wh[k];
            oh[k] = (REAL)1.02 * A2(oa, k) * dp[k] * (REAL)466.7 + (REAL)1.e-8;
            fcld_c[k] = A2(fcld, k);
            for (int l = 0; l < 4; l++) {
                reff_c[l * n1 + k] = reff[((size_t)l * np + (k - 1)) * m + i];
                cwc_c[l * n1 + k] = cwc[((size_t)l * np + (k - 1)) * m + i];
            }
        }
        memset(rr, 0, 2 * n2 * sizeof(REAL)); memset(tt, 0, 2 * n2 * sizeof(REAL)); memset(td, 0, 2 * n2 * sizeof(REAL));
        memset(rs, 0, 2 * n2 * sizeof(REAL)); memset(ts, 0, 2 * n2 * sizeof(REAL)); memset(CW, 0, 20 * n2 * sizeof(REAL));
        for (int k = 1; k <= np + 1; k++) { A2(flx, k) = 0; A2(flc, k) = 0; A2(flxu, k) = 0; A2(flcu, k) = 0; }
        for (int ib = 1; ib <= 8; ib++) {
            flx_sfc_band[(size_t)(ib - 1) * m + i] = 0;
            if (do_drfband) { drband[(size_t)(ib - 1) * m + i] = 0; dfband[(size_t)(ib - 1) * m + i] = 0; }
        }
        REAL cc1 = 0, cc2 = 0, cc3 = 0;
        for (int k = 1; k <= np; k++) {
            if (k < ict) { if (fcld_c[k] > cc1) cc1 = fcld_c[k]; }
            else if (k < icb) { if (fcld_c[k] > cc2) cc2 = fcld_c[k]; }
            else if (fcld_c[k] > cc3) cc3 = fcld_c[k];
        }
        /* ---- UV + PAR (SOLUV inline, :359-905) ---- */
        fdiruv[i] = 0; fdifuv[i] = 0;
#define L2(a, k, j) a[(k) * 2 + (j) - 1]
        for (int j = 1; j <= 2; j++) {
            L2(rr, np + 1, j) = rsuvbm[i]; L2(rs, np + 1, j) = rsuvdf[i]; L2(td, np + 1, j) = 0; L2(tt, np + 1, j) = 0; L2(ts, np + 1, j) = 0;
            L2(rr, 0, j) = 0; L2(rs, 0, j) = 0; L2(tt, 0, j) = 1; L2(ts, 0, j) = 1;
        }
        SFX(cs_gettau)(0, np, cz, dp_pa, fcld_c, reff_c, cwc_c, 0, 0, tauclb, tauclf, asycl, ssacl);      /* OVERCAST (:421) */
        for (int ib = 1; ib <= 5; ib++) {
            L2(td, 0, 1) = EXP(-(wvtoa * t->wk_uv[ib - 1] + o3toa * t->zk_uv[ib - 1]) / cz);
            L2(td, 0, 2) = L2(td, 0, 1);
            for (int k = 1; k <= np; k++) {
                const REAL taurs = t->ry_uv[ib - 1] * dp[k], tauoz = t->zk_uv[ib - 1] * oh[k], tauwv = t->wk_uv[ib - 1] * wh[k];
                const REAL tausto = taurs + tauoz + tauwv + A3B(taua, k, ib) + (REAL)1.0e-7;
                const REAL ssatau = A3B(ssaa, k, ib) + taurs;
                const REAL asysto = A3B(asya, k, ib);
                REAL tautob = tausto, asytob = asysto / ssatau, ssatob = ssatau / tautob + (REAL)1.0e-8;
                if (ssatob > (REAL)0.999999) ssatob = (REAL)0.999999;
                REAL rrt, ttt, tdt, rst, tst, dum;
                SFX(cs_deledd)(tautob, ssatob, asytob, cz, &rrt, &ttt, &tdt);
                SFX(cs_deledd)(tautob, ssatob, asytob, CS_DSM, &rst, &tst, &dum);
                L2(rr, k, 1) = rrt; L2(tt, k, 1) = ttt; L2(td, k, 1) = tdt; L2(rs, k, 1) = rst; L2(ts, k, 1) = tst;
                tautob = tausto + tauclb[k];
                ssatob = (ssatau + tauclb[k]) / tautob + (REAL)1.0e-8;
                if (ssatob > (REAL)0.999999) ssatob = (REAL)0.999999;
                asytob = (asysto + asycl[k] * tauclb[k]) / (ssatob * tautob);
                const REAL tautof = tausto + tauclf[k];
                REAL ssatof = (ssatau + tauclf[k]) / tautof + (REAL)1.0e-8;
                if (ssatof > (REAL)0.999999) ssatof = (REAL)0.999999;
                const REAL asytof = (asysto + asycl[k] * tauclf[k]) / (ssatof * tautof);
                SFX(cs_deledd)(tautob, ssatob, asytob, cz, &rrt, &ttt, &tdt);
                SFX(cs_deledd)(tautof, ssatof, asytof, CS_DSM, &rst, &tst, &dum);
                L2(rr, k, 2) = rrt; L2(tt, k, 2) = ttt; L2(td, k, 2) = tdt; L2(rs, k, 2) = rst; L2(ts, k, 2) = tst;
            }
            for (int k = 1; k <= np + 1; k++) { fclr[k] = 0; fall[k] = 0; fupa[k] = 0; fupc[k] = 0; }
            REAL fsdir = 0, fsdif = 0;
            SFX(cs_cldflxy)(np, rr, tt, td, rs, ts, CW, fclr, fall, fupc, fupa, &fsdir, &fsdif);
            const REAL hk = hk_uv[ib - 1];
            for (int k = 1; k <= np + 1; k++) {
                A2(flx, k) += fall[k] * hk; A2(flc, k) += fclr[k] * hk; A2(flxu, k) += fupa[k] * hk; A2(flcu, k) += fupc[k] * hk;
            }
            flx_sfc_band[(size_t)(ib - 1) * m + i] += fall[np + 1] * hk;
            if (do_drfband) { drband[(size_t)(ib - 1) * m + i] += fsdir * hk; dfband[(size_t)(ib - 1) * m + i] += fsdif * hk; }
            if (ib < 5) { fdiruv[i] += fsdir * hk; fdifuv[i] += fsdif * hk; }
            else { fdirpar[i] = fsdir * hk; fdifpar[i] = fsdif * hk; }
        }
        /* ---- near IR (SOLIR inline, :907-1423) ---- */
        fdirir[i] = 0; fdifir[i] = 0;
        for (int j = 1; j <= 2; j++) {
            L2(rr, np + 1, j) = rsirbm[i]; L2(rs, np + 1, j) = rsirdf[i]; L2(td, np + 1, j) = 0; L2(tt, np + 1, j) = 0; L2(ts, np + 1, j) = 0;
            L2(rr, 0, j) = 0; L2(rs, 0, j) = 0; L2(tt, 0, j) = 1; L2(ts, 0, j) = 1;
        }
        for (int ib = 1; ib <= 3; ib++) {
            const int iv = ib + 5;
            SFX(cs_gettau)(ib, np, cz, dp_pa, fcld_c, reff_c, cwc_c, 0, 0, tauclb, tauclf, asycl, ssacl);     /* OVERCAST (:955) */
            for (int ik = 1; ik <= 10; ik++) {
                L2(td, 0, 1) = EXP(-wvtoa * t->xk_ir[ik - 1] / cz);
                L2(td, 0, 2) = L2(td, 0, 1);
                for (int k = 1; k <= np; k++) {
                    const REAL taurs = t->ry_ir[ib - 1] * dp[k], tauwv = t->xk_ir[ik - 1] * wh[k];
                    const REAL tausto = taurs + tauwv + A3B(taua, k, iv) + (REAL)1.0e-7;
                    const REAL ssatau = A3B(ssaa, k, iv) + taurs + (REAL)1.0e-8;
                    const REAL asysto = A3B(asya, k, iv);
                    REAL tautob = tausto, asytob = asysto / ssatau, ssatob = ssatau / tautob + (REAL)1.0e-8;
                    if (ssatob > (REAL)0.999999) ssatob = (REAL)0.999999;
                    REAL rrt, ttt, tdt, rst, tst, dum;
                    SFX(cs_deledd)(tautob, ssatob, asytob, cz, &rrt, &ttt, &tdt);
                    SFX(cs_deledd)(tautob, ssatob, asytob, CS_DSM, &rst, &tst, &dum);
                    L2(rr, k, 1) = rrt; L2(tt, k, 1) = ttt; L2(td, k, 1) = tdt; L2(rs, k, 1) = rst; L2(ts, k, 1) = tst;
                    tautob = tausto + tauclb[k];
                    ssatob = (ssatau + ssacl[k] * tauclb[k]) / tautob + (REAL)1.0e-8;
                    if (ssatob > (REAL)0.999999) ssatob = (REAL)0.999999;
                    asytob = (asysto + asycl[k] * ssacl[k] * tauclb[k]) / (ssatob * tautob);
                    const REAL tautof = tausto + tauclf[k];
                    REAL ssatof = (ssatau + ssacl[k] * tauclf[k]) / tautof + (REAL)1.0e-8;
                    if (ssatof > (REAL)0.999999) ssatof = (REAL)0.999999;
                    const REAL asytof = (asysto + asycl[k] * ssacl[k] * tauclf[k]) / (ssatof * tautof);
                    SFX(cs_deledd)(tautob, ssatob, asytob, cz, &rrt, &ttt, &tdt);
                    SFX(cs_deledd)(tautof, ssatof, asytof, CS_DSM, &rst, &tst, &dum);
                    L2(rr, k, 2) = rrt; L2(tt, k, 2) = ttt; L2(td, k, 2) = tdt; L2(rs, k, 2) = rst; L2(ts, k, 2) = tst;
                }
                for (int k = 1; k <= np + 1; k++) { fclr[k] = 0; fall[k] = 0; fupa[k] = 0; fupc[k] = 0; }
                REAL fsdir = 0, fsdif = 0;
                SFX(cs_cldflxy)(np, rr, tt, td, rs, ts, CW, fclr, fall, fupc, fupa, &fsdir, &fsdif);
                const REAL hk = F2(hk_ir, 3, ib, ik);
                for (int k = 1; k <= np + 1; k++) {
                    A2(flx, k) += fall[k] * hk; A2(flc, k) += fclr[k] * hk; A2(flxu, k) += fupa[k] * hk; A2(flcu, k) += fupc[k] * hk;
                }
                fdirir[i] += fsdir * hk; fdifir[i] += fsdif * hk;
                flx_sfc_band[(size_t)(iv - 1) * m + i] += fall[np + 1] * hk;
                if (do_drfband) { drband[(size_t)(iv - 1) * m + i] += fsdir * hk; dfband[(size_t)(iv - 1) * m + i] += fsdif * hk; }
            }
        }
#undef L2
        /* ---- O2 and CO2 flux reductions (:1425-1552) ---- */
        df[0] = 0;
        const REAL cnt = (REAL)165.22 * snt;
        so2[1] = scal0 * cnt;
        df[1] = (REAL)0.0633 * ((REAL)1. - EXP((REAL)-0.000155 * SQRT(so2[1])));
        for (int k = 1; k <= np; k++) {
            so2[k + 1] = so2[k] + scal[k] * cnt;
            df[k + 1] = (REAL)0.0633 * ((REAL)1.0 - EXP((REAL)-0.000155 * SQRT(so2[k + 1])));
        }
        so2[1] = ((REAL)789. * co2) * scal0;
        for (int k = 1; k <= np; k++) so2[k + 1] = so2[k] + ((REAL)789. * co2) * scal[k];
        {   /* band 7: table cah(43,37) in (log10 co2 amount, log10 h2o amount) */
            const REAL u1 = (REAL)-3.0, du = (REAL)0.15, w1 = (REAL)-4.0, dw = (REAL)0.15;
            const int nu = 43, nw = 37;
            const REAL x0 = u1 + (REAL)nu * du, y0 = w1 + (REAL)nw * dw, x1 = u1 - (REAL)0.5 * du, y1 = w1 - (REAL)0.5 * dw;
            for (int k = 1; k <= np + 1; k++) {
                REAL ulog = LOG10(so2[k] * snt); if (ulog > x0) ulog = x0;
                REAL wlog = LOG10(swh[k] * snt); if (wlog > y0) wlog = y0;
                int ic = (int)((ulog - x1) / du + (REAL)1.), iw = (int)((wlog - y1) / dw + (REAL)1.);
                if (ic < 2) ic = 2; if (iw < 2) iw = 2; if (ic > nu) ic = nu; if (iw > nw) iw = nw;
                const REAL dc = ulog - (REAL)(ic - 2) * du - u1, dd = wlog - (REAL)(iw - 2) * dw - w1;
                const REAL x2 = F2(t->cah, 43, ic - 1, iw - 1) + (F2(t->cah, 43, ic - 1, iw) - F2(t->cah, 43, ic - 1, iw - 1)) / dw * dd;
                REAL y2 = x2 + (F2(t->cah, 43, ic, iw - 1) - F2(t->cah, 43, ic - 1, iw - 1)) / du * dc;
                if (y2 < 0) y2 = 0;
                df[k] = df[k] + (REAL)1.5 * y2;
            }
        }
        {   /* band 8: table coa(62,101) in (co2 * sec, log10 p) */
            const REAL u1 = (REAL)0.000250, du = (REAL)0.000050, w1 = (REAL)-2.0, dw = (REAL)0.05;
            const int nx = 62, ny = 101;
            const REAL x0 = u1 + (REAL)nx * du, y0 = w1 + (REAL)ny * dw, x1 = u1 - (REAL)0.5 * du, y1 = w1 - (REAL)0.5 * dw;
            for (int k = 1; k <= np + 1; k++) {
                REAL ulog = co2 * snt; if (ulog > x0) ulog = x0;
                REAL wlog = LOG10(A2(pl, k)); if (wlog > y0) wlog = y0;
                int ic = (int)((ulog - x1) / du + (REAL)1.), iw = (int)((wlog - y1) / dw + (REAL)1.);
                if (ic < 2) ic = 2; if (iw < 2) iw = 2; if (ic > nx) ic = nx; if (iw > ny) iw = ny;
                const REAL dc = ulog - (REAL)(ic - 2) * du - u1, dd = wlog - (REAL)(iw - 2) * dw - w1;
                const REAL x2 = F2(t->coa, 62, ic - 1, iw - 1) + (F2(t->coa, 62, ic - 1, iw) - F2(t->coa, 62, ic - 1, iw - 1)) / dw * dd;
                REAL y2 = x2 + (F2(t->coa, 62, ic, iw - 1) - F2(t->coa, 62, ic - 1, iw - 1)) / du * dc;
                if (y2 < 0) y2 = 0;
                df[k] = df[k] + (REAL)1.5 * y2;
            }
        }
        int foundtop = 0;
        for (int k = 1; k <= np; k++) if (fcld_c[k] > (REAL)0.02 && !foundtop) { foundtop = 1; ntop = k; }
        if (!foundtop) ntop = np + 1;
        const REAL dftop = df[ntop];
        for (int k = 1; k <= np + 1; k++)
            if (k > ntop) { const REAL xx4 = A2(flx, k) / A2(flx, ntop); df[k] = dftop + xx4 * (df[k] - dftop); }
        for (int k = 1; k <= np + 1; k++) {
            if (df[k] > A2(flx, k) - (REAL)1.0e-8) df[k] = A2(flx, k) - (REAL)1.0e-8;
            A2(flx, k) = A2(flx, k) - df[k];
            A2(flc, k) = A2(flc, k) - df[k];
        }
        REAL xx4 = A2(flx, np + 1) + df[np + 1];
        const REAL eps = sizeof(REAL) == 4 ? (REAL)1.1920929e-07 : (REAL)2.220446049250313e-16;
        if (FABS(xx4) > eps) {
            xx4 = (REAL)1.0 - df[np + 1] / xx4;
            if (xx4 > 1) xx4 = 1;
            if (xx4 < 0) xx4 = 0;
        } else xx4 = 0;
        fdirir[i] *= xx4; fdifir[i] *= xx4; fdiruv[i] *= xx4; fdifuv[i] *= xx4; fdirpar[i] *= xx4; fdifpar[i] *= xx4;
        for (int ib = 1; ib <= 8; ib++) {
            flx_sfc_band[(size_t)(ib - 1) * m + i] *= xx4;
            if (do_drfband) { drband[(size_t)(ib - 1) * m + i] *= xx4; dfband[(size_t)(ib - 1) * m + i] *= xx4; }
        }
    }
    free(W);
    return 0;
#undef A2
#undef A3B
}

#undef CH_NX
#undef CH_NO
#undef CH_NC
#undef CH_NH
#undef CH_GRAV
#undef CS_GRAV
#undef CS_DSM
