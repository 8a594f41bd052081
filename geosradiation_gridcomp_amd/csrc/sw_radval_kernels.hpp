// sw_radval_kernels.hpp -- the reference's SOLAR_RADVAL cloud-optics diagnostics of rrtmg_sw (gfx950).
//
// Reference behaviour: SW/rrtmg_sw_spcvmc.F90:676-746 (zeroing), :749-1109 (accumulation over the PAR sub-columns),
// SW/rrtmg_sw_rad.F90:1540-1590 (zeros for cloud-free columns), :1658-1720 (scatter of the cloudy ones).
//
// k_mcica<R, 2, true> leaves, per cloudy column, the 15 phase-split layer sums (mcica_kernels.hpp rv_add_phase) of every
// (super-layer, PAR sub-column): rvsum [3][15][20][ncol].  k_sw_radval folds them, weighted by the TOA flux of the sub-column's
// g-point, into the 15 families x {d, n} x {tp, hp, mp, lp} = 120 values per column of include/geosrad.h GEOSRAD_RV_*.
#pragma once
#include "sw_kernels.hpp"
#include "mcica_kernels.hpp"

namespace geosrad {

// adjflux * ssi (zsflxzen when isolvar < 0) of the g-points of band B, without the cosine: the solar source section of sw_band_body /
// swr_body (sw_kernels.hpp "solar source of the band's g-points"), statement for statement, so that the weights are the ones the band
// sweeps use for the cotd?? / cotn?? family.  It is the third copy (sw_band_body, swr_body): factoring the band kernels' section into a shared
// device function was not done because their instruction stream must stay the parent's; an edit to one copy goes to all three, and
// tests/test_gpu_sw_radval.py (cotl?? == cot?? bit for bit) fails if they drift apart
template <typename R, typename B>
GR_DEV void sw_solar_weights(const SwArgs<R> &A, const SwDev<R> &T, const SwSolar<R> &SV, int col, R *zinc)
{
    constexpr int NG = B::NG, IBM = B::JB - 15;
    constexpr int W = NG >= 4 ? 4 : 2;
    constexpr int NQ = (NG + W - 1) / W;
    constexpr int S = pad4(NG);
    const int n = A.ncol, nlay = A.nlay;
    const uint32_t ucol = (uint32_t)col;
    const SwBandTab<R> &Bt = T.b[IBM];
    int js = 1; R fs = 0;
    if constexpr (B::SRC != 0) {
        int laytrop = 0;
        for (int lay = 0; lay < nlay; lay++) laytrop += (int)((ldg(A.scidx, ((uint32_t)lay * (uint32_t)n + ucol) * 4u) >> 23) & 1u);
        int lsol;
        if constexpr (B::SRC == 1) {
            lsol = laytrop - 1;
            for (int lay = 0; lay < laytrop; lay++) {
                const int jp0 = (int)(ldg(A.scidx, ((uint32_t)lay * (uint32_t)n + ucol) * 4u) & 63u);
                const int jp1 = lay + 1 < nlay ? (int)(ldg(A.scidx, ((uint32_t)(lay + 1) * (uint32_t)n + ucol) * 4u) & 63u) : 99;
                if (jp0 < B::LREF && jp1 >= B::LREF) { lsol = (lay + 1 < laytrop - 1) ? lay + 1 : laytrop - 1; break; }
            }
            if (lsol < 0) lsol = 0;
        } else {
            lsol = nlay - 1;
            for (int lay = laytrop; lay < nlay; lay++) {
                const int jpm = lay > 0 ? (int)(ldg(A.scidx, ((uint32_t)(lay - 1) * (uint32_t)n + ucol) * 4u) & 63u) : 0;
                const int jp0 = (int)(ldg(A.scidx, ((uint32_t)lay * (uint32_t)n + ucol) * 4u) & 63u);
                if (jpm < B::LREF && jp0 >= B::LREF) { lsol = lay; break; }
            }
        }
        SwLayer<R> Ls;
        sw_load_layer<R>(A, lsol, col, Ls);
        const SwSpec<R> sp = (B::SRC == 1) ? sw_spec<R>(Ls.col[B::LOA], (R)B::STR, Ls.col[B::LOB], 8, T.oneminus)
                                           : sw_spec<R>(Ls.col[B::UPA], (R)B::STR, Ls.col[B::UPB], 4, T.oneminus);
        js = sp.js; fs = sp.fs;
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        R sf[W], fb[W], sd[W], ir[W];
        const int go = q * W;
        if constexpr (B::NSRC == 1) {
            ldw<R, W>(Bt.sflux, (uint32_t)go * (uint32_t)sizeof(R), sf); ldw<R, W>(Bt.facb, (uint32_t)go * (uint32_t)sizeof(R), fb);
            ldw<R, W>(Bt.snsp, (uint32_t)go * (uint32_t)sizeof(R), sd); ldw<R, W>(Bt.irrad, (uint32_t)go * (uint32_t)sizeof(R), ir);
        } else {
            linw<R, W, S>(sf, fs, Bt.sflux, js - 1, go); linw<R, W, S>(fb, fs, Bt.facb, js - 1, go);
            linw<R, W, S>(sd, fs, Bt.snsp, js - 1, go); linw<R, W, S>(ir, fs, Bt.irrad, js - 1, go);
        }
#pragma unroll
        for (int j = 0; j < W; j++) {
            const int g = go + j;
            if (g >= NG) continue;
            R src;
            if (SV.isolvar < 0) src = sf[j];
            else if (SV.isolvar <= 2) src = SV.svar_f * fb[j] + SV.svar_s * sd[j] + SV.svar_i * ir[j];
            else src = SV.svar_bnd[IBM] * fb[j] + SV.svar_bnd[IBM] * sd[j] + SV.svar_bnd[IBM] * ir[j];
            zinc[g] = SV.adjflux[IBM] * src;
        }
    }
}

// The 20 PAR sub-columns are summed in groups: each group's partial sum starts at zero and the partials are added in order.  The
// groups are those of the band sweeps' own cotd?? / cotn?? family (k_sw_reform: its units of g-points; k_sw_bands: the three
// bands), so that a family whose terms and guard coincide with that family's (cotl?? of a liquid-only column) has the same bits.
struct SwRvGroups { int n, end[RV_NPAR]; };      // group k = sub-columns [end[k - 1], end[k]), end[n - 1] = RV_NPAR

constexpr int RV_NFAM = 15;                      // families, each x {d, n} x {tp, hp, mp, lp}: GEOSRAD_RV_COUNT = 120

// one phase's families of one sub-column (spcvmc :812-870, and the totals :1054-1104); s: its 7 layer sums, a: {d, n} pairs of
// cot?, cds?, ssa?, sds?, asm?, ads?, for? in this order
template <typename R> GR_DEV void rv_fold_phase(R wgt, const R *s, R *a)
{
    if (s[0] > 0) {      // un-scaled tau of the phase
        a[0] += wgt; a[1] += wgt * s[0];
        a[4] += wgt * s[0]; a[5] += wgt * s[1];
        a[8] += wgt * s[1]; a[9] += wgt * s[2];
    }
    if (s[3] > 0) {      // delta-scaled tau of the phase
        a[2] += wgt; a[3] += wgt * s[3];
        a[6] += wgt * s[3]; a[7] += wgt * s[4];
        a[10] += wgt * s[4]; a[11] += wgt * s[5];
        a[12] += wgt * s[4]; a[13] += wgt * s[6];
    }
}

// lane = column (workspace order), blockIdx.y = 0 tp | 1 hp | 2 mp | 3 lp.  radval: (GEOSRAD_RV_COUNT, ld), column fastest, original
// column order; cloud-free columns get zeros (rrtmg_sw_rad.F90:1540).
template <typename R>
__global__ void __launch_bounds__(256) k_sw_radval(SwArgs<R> A, SwDev<R> T, SwSolar<R> SV, SwRvGroups G, const R *__restrict__ rvsum,
                                                   R *__restrict__ radval)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= A.ncol) return;
    const int n = A.ncol, kp = blockIdx.y;
    const int pc = A.perm[col];
    // {d, n} of: 0 cds | liquid 1 .. 7: cotl cdsl ssal sdsl asml adsl forl | ice 8 .. 14: coti cdsi ssai sdsi asmi adsi fori
    R tot[2 * RV_NFAM];
#pragma unroll
    for (int k = 0; k < 2 * RV_NFAM; k++) tot[k] = 0;
    if (col >= *A.nclear) {
        R zinc[RV_NPAR];
        sw_solar_weights<R, SwB24>(A, T, SV, col, zinc);
        sw_solar_weights<R, SwB25>(A, T, SV, col, zinc + 8);
        sw_solar_weights<R, SwB26>(A, T, SV, col, zinc + 14);
        R part[2 * RV_NFAM];
#pragma unroll
        for (int k = 0; k < 2 * RV_NFAM; k++) part[k] = 0;
        int grp = 0;
#pragma unroll
        for (int g = 0; g < RV_NPAR; g++) {
            const R w0 = g < 8 ? (R)0.5 : (R)1.0;      // band 24: half PAR, half NIR (:762-771)
            const R wgt = w0 * zinc[g];
            R s[RV_NSUM];
#pragma unroll
            for (int q = 0; q < RV_NSUM; q++) {
                const size_t o = ((size_t)q * RV_NPAR + g) * n + col, ss = (size_t)RV_NSUM * RV_NPAR * n;
                if (kp == 0) { const R sl = rvsum[o], sm = rvsum[ss + o], sh = rvsum[2 * ss + o]; s[q] = sl + sm + sh; }      // (:1043-1104)
                else s[q] = rvsum[(size_t)(3 - kp) * ss + o];
            }
            if (s[0] > 0) { part[0] += wgt; part[1] += wgt * s[0]; }
            rv_fold_phase<R>(wgt, s + 1, part + 2);
            rv_fold_phase<R>(wgt, s + 8, part + 16);
            if (g + 1 == G.end[grp]) {
#pragma unroll
                for (int k = 0; k < 2 * RV_NFAM; k++) { tot[k] += part[k]; part[k] = 0; }
                grp++;
            }
        }
    }
    // slot order of the reference's argument list (rrtmg_sw_rad.F90:86-119): cds | cotl cdsl coti cdsi | ssal sdsl ssai sdsi |
    // asml adsl asmi adsi | forl fori, each d(tp hp mp lp) then n(tp hp mp lp)
    constexpr int src[RV_NFAM] = {0, 1, 2, 8, 9, 3, 4, 10, 11, 5, 6, 12, 13, 7, 14};
#pragma unroll
    for (int f = 0; f < RV_NFAM; f++) {
        radval[(size_t)(f * 8 + kp) * A.ld + pc] = tot[2 * src[f]];
        radval[(size_t)(f * 8 + 4 + kp) * A.ld + pc] = tot[2 * src[f] + 1];
    }
}

}  // namespace geosrad
