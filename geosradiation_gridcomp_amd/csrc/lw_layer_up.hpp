// lw_layer_up.hpp -- one layer of band_body's upward sweep, included once per instantiation of the layer body with LW_ABOVE = 0 (general)
// or 1 (the layers above the highest gas-only pair of the wave); see lw_layer_down.hpp.  Not a header of its own.
        constexpr bool ABOVE = LW_ABOVE;
        R u0 = 0, uc0 = 0, du0 = 0, duc0 = 0;       // level 0 (surface) sums, formed in the first trip
        usum = 0; ucsum = 0; dusum = 0; ducsum = 0;
        PK sv[NG], sg[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) sv[g] = ldg_nt(s1_b, SCELL(lay, g) * (uint32_t)sizeof(PK));
        if (CLD && !ABOVE) {
            // (lanes that have no pair of their own here read what happens to be there and do not use it)
#pragma unroll
            for (int g = 0; g < NG; g++) sg[g] = ldg_nt(s2_b, SCELL(lay, g) * (uint32_t)sizeof(PK));
        } else {
#pragma unroll
            for (int g = 0; g < NG; g++) sg[g] = sv[g];
        }
        const bool own = CLD && !ABOVE && ccol && diverge && lay <= ltop;      // above ltop the layer is clear for every g-point: gas == total
        // (absorptivity, upward source) of the cell from its parked index: the transmittance table, the layer's Planck terms and
        // the Planck fraction, which the band body evaluates again (its optical-depth terms are dead code here)
        Layer<R> L;
        load_layer<R>(A, lay, col, pc, L);
        const R blay = planck_at<R>(T.totplnk, IB, ldg(A.tlay, L.ab));
        const R dplankup = planck_at<R>(T.totplnk, IB, ldg(A.tlev + (size_t)ld, L.ab)) - blay;
        Prep<R> P;
        BAND::template prep<R>(T, A, L, P);
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            R tau[W], pf[W];
            BAND::template eval<R, W>(T, L, P, q * W, tau, pf);
#pragma unroll
            for (int j = 0; j < W; j++) {
                const int g = q * W + j;
                if (g >= NG) continue;
                if (lay == 0) {
                    // surface: emission + reflection turn the downward radiance into the upward one (:319-333)
                    const R rad0 = pf[j] * plankbnd;
                    rad[g] = rad0 + reflect * rad[g];
                    dlu[g] = pf[j] * dplankbnd;
                    u0 = u0 + sumfac * rad[g];
                    du0 = du0 + sumfac * dlu[g];
                    if (CLD) {
                        radc[g] = rad0 + reflect * radc[g];
                        dclu[g] = dlu[g];
                        uc0 = uc0 + sumfac * radc[g];
                        duc0 = duc0 + sumfac * dclu[g];
                    }
                }
                const R2 e1 = lut_at((int)sv[g]);
                const R a1 = (R)1. - e1.x, b1 = pf[j] * (blay + e1.y * dplankup);
                rad[g] = rad[g] + (b1 - rad[g]) * a1;
                dlu[g] = dlu[g] - dlu[g] * a1;
                usum = usum + sumfac * rad[g];
                dusum = dusum + sumfac * dlu[g];
                if (CLD) {
                    // (ABOVE: the first look-up's pair, through an opaque copy - merged with the total stream's terms the source term would
                    // not be contracted as in the general body and round differently)
                    R2 e2 = e1;
                    if constexpr (ABOVE) asm volatile("" : "+v"(e2.x), "+v"(e2.y));
                    else e2 = lut_at(own ? (int)sg[g] : (int)sv[g]);
                    const R gx = (R)1. - e2.x, gy = pf[j] * (blay + e2.y * dplankup);
                    const R rc = radc[g] + (gy - radc[g]) * gx, dc = dclu[g] - dclu[g] * gx;
                    radc[g] = diverge ? rc : rad[g];
                    dclu[g] = diverge ? dc : dlu[g];
                    ucsum = ucsum + sumfac * radc[g];
                    ducsum = ducsum + sumfac * dclu[g];
                }
            }
        }
        if (lay == 0) {
            PART(2, 0, u0);
            if (CLD && ccol) PART(3, 0, uc0);
            if (dudTs) { PART(4, 0, du0); if (CLD && ccol) PART(5, 0, duc0); }
        }
        PART(2, lay + 1, usum);
        if (CLD && ccol) PART(3, lay + 1, ucsum);
        if (dudTs) { PART(4, lay + 1, dusum); if (CLD && ccol) PART(5, lay + 1, ducsum); }
