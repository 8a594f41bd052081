// gettau_kernels.hpp -- GEOS_RadiationShared/gettau.F90 (getvistau :33, getnirtau :102, getirtau :173; bodies getvistau.code,
// getnirtau.code, getirtau.code) over a batch of columns, per species, and the infrared cloud exports of LW_Driver for any LW scheme
// (GEOS_IrradGridComp.F90:1898-1912, :3626-3650).  getvistau / getnirtau are stated beside their tables, as so_cld_tau, so_cld_index,
// so_caib_scale, so_caif_scale and so_cld_asy (sorad_kernels.hpp): gt_swtau uses all five, k_sw_update_clouds the first, second and fourth
// for its taudiff, bit for bit getvistau's.  k_sorad_cloud (species summed; contraction on) and k_chou_bands (getirtau inside its hand-tuned
// band body) keep their own statements: sharing changes the one's rounding, the other's stream (profiles/r16_chou_physics_once.md).
//
// Arrays in the solver-API layout, the column index fastest: dp, fcld (ncol,nlevs); reff, hydromets and the per-species outputs
// (ncol,nlevs,4); tcldlyr, enn (ncol,0:nlevs).  A null output is neither computed nor written.
//
// Mapping: lane = column (every access coalesced), blockIdx.y = a run of GT_LC layers that the thread walks, two layers' loads issued
// before the first is used.  A (column block x layer run) grid rather than one thread per column: at 70 columns x 72 layers a
// thread-per-column kernel is two wavefronts on one CU, this one nine blocks; at 97 200 x 72 it is 3 420 blocks of streaming loads.
// The super-layer maxima cc(1:3) of the overlap mode need every layer of the column before the first is scaled: a pre-kernel
// (k_gettau_cc, lane = column, one read of fcld = 1 real of the ~19 a cell moves) leaves them in a (3,ncol) workspace, because a first
// walk of fcld in every thread of the layer grid would read the plane nlevs / GT_LC times.  ict = 0 needs neither.
// caib (11,9,11) and caif (9,11) are gathered per lane (seven and five entries per cloudy cell): a block copies them to LDS once for
// its 256 x GT_LC cells (1 188 reals = 0.6 per cell), only in the overlap mode and only the one whose output is wanted.
#pragma once
#include "sorad_kernels.hpp"     // SoradDev: the Chou-Suarez SW tables
#include "chou_kernels.hpp"      // ChouDev: aib_ir ...; ch_pow, ch_exp

namespace geosrad {

constexpr int GT_LC = 8;      // layers per thread of the layer grid
constexpr int GT_NB = 2;      // layers whose loads are in flight together

template <typename R> struct GtArgs {
    int ncol, nlevs, ib, ict, icb;      // ib: NIR band 1..3 / IR band 1..10; ict = 0: in-cloud mode (icb not read)
    R grav;
    const R *cosz, *dp, *fcld, *reff, *hyd;
    const R *cc;                        // (ncol,3) super-layer maxima of fcld (k_gettau_cc); overlap mode only
    R *taubeam, *taudiff, *asycl, *ssacl;      // getvistau / getnirtau
    R *taudiag, *tcldlyr, *enn;                // getirtau
};

// cc(1:3) of getvistau.code / getnirtau.code: the largest fcld above ict, from ict to icb - 1, from icb down (an empty range: 0)
template <typename R>
__global__ void __launch_bounds__(256) k_gettau_cc(int ncol, int nlevs, int ict, int icb, const R *__restrict__ fcld, R *__restrict__ cc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncol) return;
    R c1 = 0, c2 = 0, c3 = 0;
    for (int k0 = 0; k0 < nlevs; k0 += 4) {
        R f[4];
#pragma unroll
        for (int j = 0; j < 4; j++) f[j] = k0 + j < nlevs ? fcld[(size_t)(k0 + j) * ncol + i] : (R)0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = k0 + j + 1;
            if (k < ict) c1 = f[j] > c1 ? f[j] : c1;
            else if (k < icb) c2 = f[j] > c2 ? f[j] : c2;
            else c3 = f[j] > c3 ? f[j] : c3;
        }
    }
    cc[i] = c1; cc[(size_t)ncol + i] = c2; cc[2 * (size_t)ncol + i] = c3;
}

// getvistau.code (NIR = false) / getnirtau.code (NIR = true, band A.ib) for the thread's column and run of layers
template <typename R, bool NIR> GR_DEV void gt_swtau(const GtArgs<R> &A, const SoradDev<R> *__restrict__ Tp)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    __shared__ R s_caib[11 * 9 * 11];
    __shared__ R s_caif[9 * 11];
    const SoradDev<R> &T = *Tp;
    const bool scaled = A.ict != 0;
    if (scaled) {      // uniform over the grid
        if (A.taubeam) for (int t = threadIdx.x; t < 11 * 9 * 11; t += blockDim.x) s_caib[t] = T.caib[t];
        if (A.taudiff) for (int t = threadIdx.x; t < 9 * 11; t += blockDim.x) s_caif[t] = T.caif[t];
        __syncthreads();
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.ncol) return;
    const int n = A.ncol, np = A.nlevs, ib = A.ib, ict = A.ict, icb = A.icb;
    const size_t sp = (size_t)np * n;      // one species' plane
    const R grav = A.grav;
    const bool want_tau = A.taubeam || A.taudiff, want_g = A.asycl || (NIR && A.ssacl);
    const R cosz = scaled && A.taubeam ? A.cosz[i] : (R)0;
    R cc[4] = {0, 0, 0, 0};
    if (scaled && want_tau) { cc[1] = A.cc[i]; cc[2] = A.cc[(size_t)n + i]; cc[3] = A.cc[2 * (size_t)n + i]; }
    const int kb = (int)blockIdx.y * GT_LC, ke = kb + GT_LC < np ? kb + GT_LC : np;      // 0-based layers [kb, ke)
    for (int k0 = kb; k0 < ke; k0 += GT_NB) {
        R dpv[GT_NB], f[GT_NB], re[4][GT_NB], h[4][GT_NB];
#pragma unroll
        for (int j = 0; j < GT_NB; j++) {
            const bool live = k0 + j < ke;
            const size_t o = (size_t)(k0 + j) * n + i;
            dpv[j] = live ? A.dp[o] : (R)0;
            f[j] = live ? A.fcld[o] : (R)0;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                h[s][j] = live ? A.hyd[s * sp + o] : (R)0;
                re[s][j] = live && s != 2 ? A.reff[s * sp + o] : (R)0;      // the rain radius enters nothing
            }
        }
#pragma unroll
        for (int j = 0; j < GT_NB; j++) {
            const int k = k0 + j + 1;      // the reference's layer index
            if (k > ke) break;
            const size_t o = (size_t)(k - 1) * n + i;
            const R wp = (dpv[j] * (R)1.0e3) / grav;
            const R r1 = re[0][j], r2 = re[1][j], r4 = re[3][j], fc = f[j];
            R tc1, tc2, tc3, tc4, rs;      // rs: reff_snow = min(reff(k,4),112.0)
            so_cld_tau<R, NIR>(T, ib, wp, r1, r2, r4, h[0][j], h[1][j], h[2][j], h[3][j], tc1, tc2, tc3, tc4, rs);
            const R tauc = tc1 + tc2 + tc3 + tc4;
            const bool cloudy = tauc > (R)0.02 && fc > (R)0.01;
            if (want_tau) {
                R xb = 1, xf = 1;      // in-cloud mode: the species' thicknesses as they are, whatever fcld
                if (scaled) {
                    xb = 0; xf = 0;    // overlap mode: a thin or nearly uncovered layer gets none
                    if (cloudy) {
                        const int kk = k < ict ? 1 : (k < icb ? 2 : 3);
                        R fa = NIR ? (cc[kk] != 0 ? fc / cc[kk] : (R)0) : fc / cc[kk];      // getnirtau guards, getvistau divides
                        int it, ia; R ft;
                        so_cld_index<R>(tauc, fa, it, ia, ft);
                        if (A.taubeam) xb = so_caib_scale<R>(s_caib, cosz, it, ia, ft, fa);
                        if (A.taudiff) xf = so_caif_scale<R>(s_caif, it, ia, ft, fa);
                    }
                }
                const bool zero = scaled && !cloudy;      // written as the reference's 0., not as 0 * tc (an infinite tc stays a zero)
                if (A.taubeam) {
                    A.taubeam[o] = zero ? (R)0 : (scaled ? tc1 * xb : tc1); A.taubeam[sp + o] = zero ? (R)0 : (scaled ? tc2 * xb : tc2);
                    A.taubeam[2 * sp + o] = zero ? (R)0 : (scaled ? tc3 * xb : tc3); A.taubeam[3 * sp + o] = zero ? (R)0 : (scaled ? tc4 * xb : tc4);
                }
                if (A.taudiff) {
                    A.taudiff[o] = zero ? (R)0 : (scaled ? tc1 * xf : tc1); A.taudiff[sp + o] = zero ? (R)0 : (scaled ? tc2 * xf : tc2);
                    A.taudiff[2 * sp + o] = zero ? (R)0 : (scaled ? tc3 * xf : tc3); A.taudiff[3 * sp + o] = zero ? (R)0 : (scaled ? tc4 * xf : tc4);
                }
            }
            if (want_g) {
                R asy = 1, ssa = (R)0.99999;
                if (cloudy) so_cld_asy<R, NIR>(T, ib, r1, r2, r4, rs, tc1, tc2, tc3, tc4, tauc, asy, ssa);
                if (A.asycl) A.asycl[o] = asy;
                if (NIR && A.ssacl) A.ssacl[o] = ssa;
            }
        }
    }
}

template <typename R> __global__ void __launch_bounds__(256) k_getvistau(GtArgs<R> A, const SoradDev<R> *__restrict__ Tp) { gt_swtau<R, false>(A, Tp); }
template <typename R> __global__ void __launch_bounds__(256) k_getnirtau(GtArgs<R> A, const SoradDev<R> *__restrict__ Tp) { gt_swtau<R, true>(A, Tp); }

// the four species' optical thicknesses of getirtau.code for band ib, written as k_chou_bands writes them (same expressions, same power
// function, same contraction mode), so that their sum is irrad's TAUDIAG; rs = the capped snow radius
template <typename R>
GR_DEV void gt_irtau(const ChouDev<R> &T, int ib, R wp, R r1, R r2, R r4, R h1, R h2, R h3, R h4, R &tau1, R &tau2, R &tau3, R &tau4, R &rs)
{
    const R *aib = T.aib + 3 * (ib - 1), *awb = T.awb + 4 * (ib - 1);
    rs = r4 < (R)112.0 ? r4 : (R)112.0;
    tau1 = r1 <= 0 ? (R)0 : (wp * h1) * (aib[0] + aib[1] / ch_pow<R>(r1, aib[2]));
    tau2 = (wp * h2) * (awb[0] + (awb[1] + (awb[2] + awb[3] * r2) * r2) * r2);
    tau3 = (R)0.00307 * (wp * h3);
    tau4 = rs <= 0 ? (R)0 : (wp * h4) * (aib[0] + aib[1] / ch_pow<R>(rs, aib[2]));
}

// getirtau.code for band A.ib; level 0 of tcldlyr / enn (1 / 0) is written by the thread of layer 1
template <typename R>
__global__ void __launch_bounds__(256) k_getirtau(GtArgs<R> A, const ChouDev<R> *__restrict__ Tp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.ncol) return;
    const ChouDev<R> &T = *Tp;
    const int n = A.ncol, np = A.nlevs, ib = A.ib;
    const size_t sp = (size_t)np * n;
    const R grav = A.grav;
    const R *aiw = T.aiw + 4 * (ib - 1), *aww = T.aww + 4 * (ib - 1), *aig = T.aig + 4 * (ib - 1), *awg = T.awg + 4 * (ib - 1);
    const bool want_t = A.tcldlyr || A.enn;
    const int kb = (int)blockIdx.y * GT_LC, ke = kb + GT_LC < np ? kb + GT_LC : np;
    if (kb == 0) {
        if (A.tcldlyr) A.tcldlyr[i] = 1;
        if (A.enn) A.enn[i] = 0;
    }
    for (int k0 = kb; k0 < ke; k0 += GT_NB) {
        R dpv[GT_NB], f[GT_NB], re[4][GT_NB], h[4][GT_NB];
#pragma unroll
        for (int j = 0; j < GT_NB; j++) {
            const bool live = k0 + j < ke;
            const size_t o = (size_t)(k0 + j) * n + i;
            dpv[j] = live ? A.dp[o] : (R)0;
            f[j] = live && want_t ? A.fcld[o] : (R)0;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                h[s][j] = live ? A.hyd[s * sp + o] : (R)0;
                re[s][j] = live && s != 2 ? A.reff[s * sp + o] : (R)0;
            }
        }
#pragma unroll
        for (int j = 0; j < GT_NB; j++) {
            const int k = k0 + j + 1;
            if (k > ke) break;
            const size_t o = (size_t)(k - 1) * n + i;
            const R wp = (dpv[j] * (R)1.0e3) / grav;
            const R r1 = re[0][j], r2 = re[1][j];
            R tau1, tau2, tau3, tau4, rs;
            gt_irtau<R>(T, ib, wp, r1, r2, re[3][j], h[0][j], h[1][j], h[2][j], h[3][j], tau1, tau2, tau3, tau4, rs);
            if (A.taudiag) { A.taudiag[o] = tau1; A.taudiag[sp + o] = tau2; A.taudiag[2 * sp + o] = tau3; A.taudiag[3 * sp + o] = tau4; }
            if (!want_t) continue;
            R tauc = tau1 + tau2 + tau3 + tau4;
            const R fc = f[j];
            R tcl = 1, en = 0;
            if (tauc > (R)0.02 && fc > (R)0.01) {
                const R w1 = tau1 * (aiw[0] + (aiw[1] + (aiw[2] + aiw[3] * r1) * r1) * r1);
                const R w2 = tau2 * (aww[0] + (aww[1] + (aww[2] + aww[3] * r2) * r2) * r2);
                const R w3 = tau3 * (R)0.54;
                const R w4 = tau4 * (aiw[0] + (aiw[1] + (aiw[2] + aiw[3] * rs) * rs) * rs);
                const R ww = (w1 + w2 + w3 + w4) / tauc;
                const R g1 = w1 * (aig[0] + (aig[1] + (aig[2] + aig[3] * r1) * r1) * r1);
                const R g2 = w2 * (awg[0] + (awg[1] + (awg[2] + awg[3] * r2) * r2) * r2);
                const R g3 = w3 * (R)0.95;
                const R g4 = w4 * (aig[0] + (aig[1] + (aig[2] + aig[3] * rs) * rs) * rs);
                const R gg = (w1 + w2 + w3 + w4 != 0) ? (g1 + g2 + g3 + g4) / (w1 + w2 + w3 + w4) : (R)0.5;
                const R ff = (R)0.5 + ((R)0.3739 + ((R)0.0076 + (R)0.1185 * gg) * gg) * gg;
                R sc = (R)1. - ww * ff; sc = sc > 0 ? sc : (R)0;
                tauc = sc * tauc;
                tcl = ch_exp<R>((R)-1.66 * tauc);
                en = fc * ((R)1.0 - tcl);
            }
            if (A.tcldlyr) A.tcldlyr[(size_t)k * n + i] = tcl;
            if (A.enn) A.enn[(size_t)k * n + i] = en;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_lw_cloud_diag: TAUIR, CLDTMP, CLDPRS of LW_Driver (GEOS_IrradGridComp.F90:3626-3650) from the GEOS fields in model ordering, for
// any LW scheme: the cloud preparation of :1898-1912 (CWC = QI QL QR QS, REFF = the radius, 36 / 14 / 50 / 50 microns where it is
// MAPL_UNDEF, * 1.0e6), getirtau's species thicknesses of bands 3 and 4, TAUIR = 0.5 (band 3 + band 4), and the first layer from the
// top whose TAUIR exceeds TAUCRIT / 2.13.  Neither thickness depends on the cloud fraction.  One thread per column walking down
// (the cloud top is a serial search); no taudiag plane in HBM.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct LwCldDiag {
    int ncol, lm;
    R grav, undef, taucrit;            // taucrit: TAUCRIT / 2.13 in the real kind (:3628)
    const R *ple, *t, *q[4], *r[4];
    R *tauir, *cldtmp, *cldprs;
};
template <typename R>
__global__ void __launch_bounds__(256) k_lw_cloud_diag(LwCldDiag<R> D, const ChouDev<R> *__restrict__ Tp)
{
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= D.ncol) return;
    const ChouDev<R> &T = *Tp;
    const int n = D.ncol, lm = D.lm;
    const R dflt[4] = {(R)36.e-6, (R)14.e-6, (R)50.e-6, (R)50.e-6};      // IRR:1905-1908
    int top = -1;
    R pup = D.ple[ij];
    for (int l0 = 0; l0 < lm; l0 += GT_NB) {
        R pl[GT_NB], h[4][GT_NB], re[4][GT_NB];
#pragma unroll
        for (int j = 0; j < GT_NB; j++) {
            const bool live = l0 + j < lm;
            const size_t o = (size_t)(l0 + j) * n + ij;
            pl[j] = live ? D.ple[o + n] : (R)0;
#pragma unroll
            for (int s = 0; s < 4; s++) { h[s][j] = live ? D.q[s][o] : (R)0; re[s][j] = live && s != 2 ? D.r[s][o] : (R)0; }
        }
#pragma unroll
        for (int j = 0; j < GT_NB; j++) {
            const int l = l0 + j;
            if (l >= lm) break;
            const R dp = pl[j] - pup;
            pup = pl[j];
            const R wp = (dp * (R)1.0e3) / D.grav;
            R rr[4];
#pragma unroll
            for (int s = 0; s < 4; s++) { R r = re[s][j]; if (r == D.undef) r = dflt[s]; rr[s] = r * (R)1.0e6; }      // IRR:1909-1912
            R a1, a2, a3, a4, b1, b2, b3, b4, rs;
            gt_irtau<R>(T, 3, wp, rr[0], rr[1], rr[3], h[0][j], h[1][j], h[2][j], h[3][j], a1, a2, a3, a4, rs);
            gt_irtau<R>(T, 4, wp, rr[0], rr[1], rr[3], h[0][j], h[1][j], h[2][j], h[3][j], b1, b2, b3, b4, rs);
            const R t3 = a1 + a2 + a3 + a4, t4 = b1 + b2 + b3 + b4;      // TAUDIAG(:,:,:,3), (:,:,:,4)
            const R tau = (R)0.5 * (t3 + t4);
            if (D.tauir) D.tauir[(size_t)l * n + ij] = tau;
            if (top < 0 && tau > D.taucrit) top = l;
        }
        if (!D.tauir && top >= 0) break;
    }
    // layer L = top + 1: T(L) and PLE(L-1), the layer's upper edge, are both row `top` of their arrays
    if (D.cldtmp) D.cldtmp[ij] = top >= 0 ? D.t[(size_t)top * n + ij] : D.undef;
    if (D.cldprs) D.cldprs[ij] = top >= 0 ? D.ple[(size_t)top * n + ij] : D.undef;
}

}  // namespace geosrad
