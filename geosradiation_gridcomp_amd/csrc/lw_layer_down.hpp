// lw_layer_down.hpp -- one layer of band_body's downward sweep, included once per instantiation of the layer body with LW_ABOVE = 0
// (general) or 1 (the layers above the wave's highest cloud top): the text of a loop body in band_body's scope.  Not a header of its own.
        constexpr bool ABOVE = LW_ABOVE;
        constexpr bool CL = CLD && !ABOVE;                  // the layer may hold cloud
        const int lc_cur = lc_next;
        if (CL && lay > 0) lc_next = (int)ldg(A.laycloudy, (uint32_t)(lay - 1) * (uint32_t)n + ucol);
        const bool laycld0 = CL && ccol && lc_cur != 0;
        const bool wlc0 = CL && __ballot(laycld0) != 0;
        // McICA optical depths of ALL the layer's g-points, requested with the layer record: one HBM round trip per cloudy layer instead
        // of one per g-group
        R tcall[CLD ? NG : 1];
        if (CL) {
#pragma unroll
            for (int g = 0; g < NG; g++) tcall[g] = 0;
            if (wlc0) {
#pragma unroll
                for (int g = 0; g < NG; g++)
                    tcall[g] = ldg(taucmc_b, (((uint32_t)lay * (uint32_t)NG + (uint32_t)g) * (uint32_t)n + ucol) * (uint32_t)sizeof(R));
            }
        }
        Layer<R> L;
        load_layer<R>(A, lay, col, pc, L);
        // the layer's aerosol and temperatures are requested, and the Planck look-ups they lead to made, BEFORE the band's prep: behind
        // it they were a memory round trip of their own in every layer (5.12 -> 4.85 ms per 100 000 clear-sky columns)
        const R ta = A.tauaer ? ldg(A.tauaer + (size_t)(IB - 1) * nlay * ld, L.ab) : (R)0;
        const R blay = planck_at<R>(T.totplnk, IB, ldg(A.tlay, L.ab));
        const R plk_dn = planck_at<R>(T.totplnk, IB, ldg(A.tlev, L.ab));
        Prep<R> P;
        BAND::template prep<R>(T, A, L, P);
        const R dplankup = plk_up - blay, dplankdn = plk_dn - blay;
        plk_up = plk_dn;
        bool laycld = false;
        if (CL) {
            laycld = laycld0;
            if (laycld && !diverge) { diverge = true; ltop = lay; }   // (:297-299) before this layer's clear-sky update
        }
        const uint32_t cell0 = ((uint32_t)lay * (uint32_t)NG) * (uint32_t)n + ucol;   // g = 0 cell of this layer; + g*n
        R dsum = 0, dcsum = 0;
        if constexpr (!CLD) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            R tau[W], pf[W];
            BAND::template eval<R, W>(T, L, P, q * W, tau, pf);
            // phase 1: Pade index of the gas optical depth + LUT gathers of the whole group
            int itg[W];
            R2 eg[W];
#pragma unroll
            for (int j = 0; j < W; j++) {
                const int g = q * W + j;
                if (g >= NG) { itg[j] = 0; eg[j].x = 0; eg[j].y = 0; continue; }   // padding of the last group
                if (DBG) {
                    const size_t o = ((size_t)pc * NG_LW + (G0 + g)) * nlay + lay;   // Fortran (nlay,140,ncol)
                    A.dbg_taug[o] = tau[j] + ta;
                    A.dbg_pfracs[o] = pf[j];
                }
                R odepth = secdiff * (tau[j] + ta);
                if (odepth < 0) odepth = 0;
                const R tblind = lw_pade<R>(odepth, bpade);
                itg[j] = (int)(tblint * tblind + (R)0.5);
                eg[j] = lut_at(itg[j]);
            }
            __builtin_amdgcn_sched_barrier(0);
            // phase 2: only now write the PREVIOUS group's parked cells.  Loads and stores share one in-order counter
            // (vmcnt) on gfx9: a load issued after a store cannot be consumed before that store is acknowledged, so the
            // stores go behind this group's loads and get a whole group of arithmetic to drain.
            if (npend) {
#pragma unroll
                for (int j = 0; j < W; j++)
                    if (j < npend) {
                        stg_nt(s1_b, poff[j] * (uint32_t)sizeof(PK), pend1[j]);
                        if (CLD && (pmask2 >> j) & 1u) stg_nt(s2_b, poff[j] * (uint32_t)sizeof(PK), pend2[j]);
                    }
            }
            npend = 0; pmask2 = 0;
            __builtin_amdgcn_sched_barrier(0);
            // phase 3: radiance recurrences of the group
#pragma unroll
            for (int j = 0; j < W; j++) {
                const int g = q * W + j;
                if (g >= NG) continue;
                const int itgas = itg[j];
                const R2 e = eg[j];
                const R agas = (R)1. - e.x, tfacgas = e.y;
                const R bbdgas = pf[j] * (blay + tfacgas * dplankdn);
                const R bbugas = pf[j] * (blay + tfacgas * dplankup);
                const uint32_t cell = cell0 + (uint32_t)g * (uint32_t)n;
                const uint32_t scell = SCELL(lay, g);
                R atot = agas, bbutot = bbugas;
                int itp = itgas;                 // index parked for the total-sky stream
                const R radprev = rad[g];
                bool cldcell = false;
                if (CLD && laycld) {
                    const R tc = ldg(taucmc_b, cell * (uint32_t)sizeof(R));
                    if (tc > 0) {
                        cldcell = true;
                        // cloud added to the DISCRETISED gas tau (:264-268)
                        const R odtot = ldg(T.tau_tbl, (uint32_t)itgas * (uint32_t)sizeof(R)) + secdiff * tc;
                        const R tb2 = lw_pade<R>(odtot, bpade);
                        const int ittot = (int)(tblint * tb2 + (R)0.5);
                        itp = ittot;
                        const R2 e2 = lut_at(ittot);
                        atot = (R)1. - e2.x;
                        const R bbdtot = pf[j] * (blay + e2.y * dplankdn);
                        bbutot = pf[j] * (blay + e2.y * dplankup);
                        rad[g] = radprev + (bbdtot - radprev) * atot;
                    }
                }
                if (!cldcell) rad[g] = radprev + (bbdgas - radprev) * agas;
                if (DEFER) { pend1[j] = (PK)(itp); poff[j] = scell; npend = j + 1; }
                else stg_nt(s1_b, scell * (uint32_t)sizeof(PK), (PK)(itp));
                dsum = dsum + sumfac * rad[g];
                if (CLD && ccol) {
                    if (diverge) {
                        radc[g] = radc[g] + (bbdgas - radc[g]) * agas;
                        if (DEFER) { pend2[j] = (PK)(itgas); pmask2 |= 1u << j; }
                        else stg_nt(s2_b, scell * (uint32_t)sizeof(PK), (PK)(itgas));
                    } else {
                        radc[g] = rad[g];
                    }
                    dcsum = dcsum + sumfac * radc[g];
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // keep one g-group's table rows in flight at a time
        }
        } else {
        // general (cloudy-column) body.  Control flow around memory operations is wave-uniform only (ballots): a per-lane branch
        // with a load inside makes the loads of a group wait for one another.  Lanes the test does not concern load / store
        // along and select afterwards (their values are never used: unwritten cloud cells, gas-only pairs above their own cloud top).
        const bool wlc = CL && __ballot(laycld) != 0;        // some column of the wave has cloud in this layer
        const bool wdv = CL && __ballot(diverge) != 0;       // some column of the wave keeps gas-only pairs from here down
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            R tcv[W];
#pragma unroll
            for (int j = 0; j < W; j++) tcv[j] = 0;
            if (wlc) {
#pragma unroll
                for (int j = 0; j < W; j++)
                    if (q * W + j < NG) tcv[j] = tcall[q * W + j];
#pragma unroll
                for (int j = 0; j < W; j++) tcv[j] = laycld ? tcv[j] : (R)0;
            }
            R tau[W], pf[W];
            BAND::template eval<R, W>(T, L, P, q * W, tau, pf);
            int itg[W];
            R2 eg[W];
            R ttb[W];
            bool anyc = false;
#pragma unroll
            for (int j = 0; j < W; j++) {
                const int g = q * W + j;
                ttb[j] = 0;
                if (g >= NG) { itg[j] = 0; eg[j].x = 0; eg[j].y = 0; continue; }   // padding of the last group
                if (DBG) {
                    const size_t o = ((size_t)pc * NG_LW + (G0 + g)) * nlay + lay;   // Fortran (nlay,140,ncol)
                    A.dbg_taug[o] = tau[j] + ta;
                    A.dbg_pfracs[o] = pf[j];
                }
                R odepth = secdiff * (tau[j] + ta);
                if (odepth < 0) odepth = 0;
                const R tblind = lw_pade<R>(odepth, bpade);
                itg[j] = (int)(tblint * tblind + (R)0.5);
                eg[j] = lut_at(itg[j]);
                anyc = anyc || tcv[j] > 0;
            }
            const bool wcl = wlc && __ballot(anyc) != 0;         // some cell of the group is cloudy in some column of the wave
            if (wcl) {
#pragma unroll
                for (int j = 0; j < W; j++) ttb[j] = ldg(T.tau_tbl, (uint32_t)itg[j] * (uint32_t)sizeof(R));
            }
            // the PREVIOUS group's parked cells are written only now, behind this group's loads (see the cloud-free body)
            __builtin_amdgcn_sched_barrier(0);
            if (npend) {
#pragma unroll
                for (int j = 0; j < W; j++)
                    if (j < npend) {
                        stg_nt(s1_b, poff[j] * (uint32_t)sizeof(PK), pend1[j]);
                        if ((pmask2 >> j) & 1u) stg_nt(s2_b, poff[j] * (uint32_t)sizeof(PK), pend2[j]);
                    }
            }
            npend = 0; pmask2 = 0;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < W; j++) {
                const int g = q * W + j;
                if (g >= NG) continue;
                const R agas = (R)1. - eg[j].x, tfacgas = eg[j].y;
                const R bbdgas = pf[j] * (blay + tfacgas * dplankdn);
                const R bbugas = pf[j] * (blay + tfacgas * dplankup);
                const uint32_t scell = SCELL(lay, g);
                R atot = agas, bbutot = bbugas, bbd = bbdgas;
                // (ABOVE: the general body takes bbd out of a select; as a plain product it would be contracted into the subtraction below
                // and round differently - a column's bits must not depend on the loop a layer runs in)
                if constexpr (ABOVE) asm volatile("" : "+v"(bbd));
                int itp = itg[j];
                if (wcl) {
                    // cloud added to the DISCRETISED gas tau (:264-268); evaluated for the whole wave, kept for the cloudy cells
                    const bool cld = tcv[j] > 0;
                    const R odtot = ttb[j] + secdiff * tcv[j];
                    const R tb2 = lw_pade<R>(odtot, bpade);
                    const int ittot = (int)(tblint * tb2 + (R)0.5);
                    itp = cld ? ittot : itg[j];
                    const R2 e2 = lut_at(itp);
                    const R ac = (R)1. - e2.x;
                    const R bbdtot = pf[j] * (blay + e2.y * dplankdn), bbut = pf[j] * (blay + e2.y * dplankup);
                    atot = cld ? ac : agas; bbutot = cld ? bbut : bbugas; bbd = cld ? bbdtot : bbdgas;
                }
                rad[g] = rad[g] + (bbd - rad[g]) * atot;
                pend1[j] = (PK)(itp); poff[j] = scell; npend = j + 1;
                dsum = dsum + sumfac * rad[g];
                if constexpr (CL) {
                    const R rc = radc[g] + (bbdgas - radc[g]) * agas;
                    radc[g] = diverge ? rc : rad[g];
                    if (wdv) { pend2[j] = (PK)(itg[j]); pmask2 |= 1u << j; }
                    dcsum = dcsum + sumfac * radc[g];
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // keep one g-group's table rows in flight at a time
        }
        }
        err_wave(ta < 0, A.err, 20);      // LW/rrtmg_lw_rad.F90:209-318 on tauaer: every band visits every layer of its columns
        PART(0, lay, dsum);
        if (CLD && ccol) PART(1, lay, ABOVE ? dsum : dcsum);
