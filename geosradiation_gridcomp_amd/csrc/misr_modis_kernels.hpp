// misr_modis_kernels.hpp -- the two passive simulators of GEOSsatsim_GridComp's COSP beside ISCCP on the device, on the SCOPS byte mask
// that satsim_kernels.hpp makes: MISR (MISR_simulator.f) in the first half of this file, MODIS (modis_simulator.F90 with the rules of
// cosp.F90 and cosp_modis_simulator.F90 around it) in the second.  The statements are the reference's, operation by operation, in the real
// kind R (contraction off); exp, sqrt, log, log10 and the divisions are the precise device functions.
//
// Arrays: the reference's Fortran layouts, the point index fastest: zfull, at, dtau_s, dtau_c (npoints,nlev), frac_out (npoints,ncol,nlev)
// as one byte per cell, fq_MISR_TAU_v_CTH (npoints,7 tau,16 heights), dist_model_layertops (npoints,16).  Level 1 is the top of the atmosphere.
//
// Mapping, as satsim_kernels.hpp.  k_misr_box: lane = (point, sub-column), the point fastest, so that a wave's load of a level of dtau_s ...
// is one coalesced row that a point's sub-columns re-read from L2; a lane walks the levels once with its tau, its cloud-layer tau and the
// thres_crossed_MISR state in registers and leaves tau and box_MISR_ztop in two (npoints,ncol) planes.  k_misr_stats: lane = point; the sums
// over the sub-columns run in ibox order, the histogram is counted and then added as the reference adds it.
//
// Two oddities of the reference are reproduced (include/geosrad_misr_modis.h): the pattern matcher of :314-335 works on box_MISR_ztop(1,ibox),
// the first point of the call, only; and a dark point sets MISR_mean_ztop(npoints), not (j).  `first` / `last` say whether this launch's
// point 0 / point npoints-1 are the call's: a chunk of the host pipeline or a shard of a multi-device context is a launch of its own.
#pragma once
#include <cstdint>

#include "satsim_kernels.hpp"      // ss_log, ss_opt

namespace geosrad {

constexpr int MISR_NCTH = 16;      // n_MISR_CTH

template <typename R> struct MisrArgs {
    int npoints, nlev, ncol;
    int first, last;
    R missing_value;
    const int32_t *sunlit;
    const R *zfull, *at, *dtau_s, *dtau_c;      // dtau_c null (geosrad_cosp_dev only): zero
    const uint8_t *frac;
    R *tau, *ztop;      // workspace, (npoints,ncol): the column's optical depth, box_MISR_ztop before the pattern matcher
    R *fq, *dist, *mean_ztop, *cldarea;
};

// :139-149, :412-422: the MISR height bin (2..16; 1 is the "no height" bin) of a height in metres.  1000 * MISR_CTH_boundaries(3:17) is
// exact in either kind
template <typename R> GR_DEV int misr_bin(R z)
{
    const R b[MISR_NCTH - 1] = {(R)500, (R)1000, (R)1500, (R)2000, (R)2500, (R)3000, (R)4000, (R)5000, (R)7000, (R)9000, (R)11000, (R)13000,
                                (R)15000, (R)17000, (R)99000};
    int i = 2;
#pragma unroll
    for (int loop = 2; loop <= MISR_NCTH; loop++)
        if (z > b[loop - 2]) i = loop + 1;
    return i;
}

// MISR_simulator.f:159-278 for one sub-column
template <typename R>
__global__ void __launch_bounds__(256) k_misr_box(const MisrArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = A.npoints, nlev = A.nlev, ncol = A.ncol;
    if (idx >= (size_t)n * ncol) return;
    const int j = (int)(idx % n), b = (int)(idx / n);
    const R zero = (R)0, one = (R)1, half = (R)0.5;
    R tau = 0, ztop = 0, cloud_dtau = 0;
    int thres = 0;      // thres_crossed_MISR
    for (int k = 0; k < nlev; k++) {
        const size_t o = (size_t)k * n + j;
        const uint8_t f = A.frac[((size_t)k * ncol + b) * n + j];
        R dtau = 0;
        if (f == 1) dtau = A.dtau_s[o];
        if (f == 2) dtau = ss_opt(A.dtau_c, o);
        tau = tau + dtau;
        if (thres == 0 && dtau > zero) { thres = 1; cloud_dtau = 0; }
        if (thres < 99 && thres > 0) {
            if (dtau == zero) cloud_dtau = 0;
            else cloud_dtau = cloud_dtau + dtau;
            if (dtau > zero && (cloud_dtau - dtau) < one) {
                if (dtau < one || k == 0 || k == nlev - 1) ztop = A.zfull[o];
                else ztop = half * (A.zfull[o] + A.zfull[o - n]) - half * (A.zfull[o - n] - A.zfull[o + n]) / dtau;
            }
            if (dtau > one && A.at[o] > (R)273) thres = 99;
            if (tau > (R)5) thres = 99;
        }
    }
    if (thres == 1) {      // :254-276
        if (tau > (R)0.5) { }
        else if (tau > (R)0.2) ztop = (R)-1;
        else ztop = 0;
    }
    A.tau[idx] = tau; A.ztop[idx] = ztop;
}

// MISR_simulator.f:128-153, :314-335, :342-470 for one point
constexpr int MISR_STATS_T = 128;
template <typename R>
__global__ void __launch_bounds__(MISR_STATS_T) k_misr_stats(const MisrArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    __shared__ uint16_t s_cnt[7 * MISR_NCTH][MISR_STATS_T];      // sub-columns per (tau, height) class; a lane touches its own column only
    __shared__ uint32_t s_top[MISR_NCTH][MISR_STATS_T];          // layer tops per height bin
    const int j = blockIdx.x * blockDim.x + threadIdx.x, t = threadIdx.x;
    const int n = A.npoints, nlev = A.nlev, ncol = A.ncol;
    if (j >= n) return;
    const R zero = (R)0, miss = A.missing_value;
    const R tauchk = (R)-1. * ss_log((R)0.9999999), isccp_taumin = (R)0.3;
    const bool lit = A.sunlit[j] == 1;
    for (int c = 0; c < 7 * MISR_NCTH; c++) s_cnt[c][t] = 0;
    for (int c = 0; c < MISR_NCTH; c++) s_top[c][t] = 0;
    if (A.dist) {      // :128-153
        R zup = 0;
        for (int k = 0; k < nlev; k++) {
            const R z = A.zfull[(size_t)k * n + j];
            const R ztest = (k == 0 || k == nlev - 1) ? z : (R)0.5 * (z + zup);
            s_top[misr_bin(ztest) - 1][t]++;
            zup = z;
        }
        // a sum of at most nlev ones is exact in either kind: the count itself
        for (int c = 0; c < MISR_NCTH; c++) A.dist[(size_t)c * n + j] = lit ? (R)s_top[c][t] : miss;
    }
    const bool matcher = A.first && j == 0;      // :314-335 reads and writes box_MISR_ztop(1,ibox)
    const R boxarea = (R)1. / (R)ncol;
    R mean_ztop = 0, cldarea = 0, zprev = 0;
    for (int b = 0; b < ncol; b++) {
        const size_t o = (size_t)b * n + j;
        R z = A.ztop[o];
        if (matcher && b >= 1 && b <= ncol - 2) {      // sequential in ibox: zprev is ibox-1 as the matcher left it, ibox+1 is untouched yet
            const R znext = A.ztop[o + n];
            if (zprev > zero && znext > zero) {
                const R d = zprev - znext, ad = d < zero ? -d : d;
                if (ad < (R)500 && z < znext) z = znext;
            }
        }
        zprev = z;
        if (!lit) continue;
        const R tau = A.tau[o];
        const bool cloudy = tau > tauchk;
        int itau = 0;
        if (cloudy) {      // :366-385
            if (tau < isccp_taumin) itau = 1;
            else if (tau >= isccp_taumin && tau < (R)1.3) itau = 2;
            else if (tau >= (R)1.3 && tau < (R)3.6) itau = 3;
            else if (tau >= (R)3.6 && tau < (R)9.4) itau = 4;
            else if (tau >= (R)9.4 && tau < (R)23.) itau = 5;
            else if (tau >= (R)23. && tau < (R)60.) itau = 6;
            else if (tau >= (R)60.) itau = 7;
        }
        if (z == zero) continue;      // no cloud detected
        if (z == (R)-1) {             // detected, too thin for a height: the "no height" bin
            // k_misr_box sets -1 under tau > 0.2 only, and tauchk (1.2e-7 in fp32, 1.0e-7 in fp64) is below 0.2 in both kinds, so such a
            // sub-column is cloudy and itau >= 1; the test keeps the index inside s_cnt where the reference would write fq(j,0,1)
            if (itau >= 1) s_cnt[itau - 1][t]++;
            continue;
        }
        const int iz = misr_bin(z);
        if (cloudy) s_cnt[(iz - 1) * 7 + itau - 1][t]++;      // :424-442: a height the matcher gave a clear sub-column is not in the histogram
        mean_ztop = mean_ztop + z * boxarea;
        cldarea = cldarea + boxarea;
    }
    if (!lit) {      // :451-462: MISR_mean_ztop(npoints) is set, not (j), and the call's last point is reset at its own turn
        cldarea = miss;
        if (A.last && j == n - 1) mean_ztop = miss;
    }
    if (A.fq)
        for (int c = 0; c < 7 * MISR_NCTH; c++) {
            R v = lit ? zero : miss;
            if (lit) for (int k = s_cnt[c][t]; k > 0; k--) v = v + boxarea;      // fq = fq + boxarea, once per sub-column of the class
            A.fq[(size_t)c * n + j] = v;
        }
    if (cldarea > zero) mean_ztop = mean_ztop / cldarea;      // :466-468
    if (A.cldarea) A.cldarea[j] = cldarea;
    if (A.mean_ztop) A.mean_ztop[j] = mean_ztop;
}


// =====================================================================================================================================
// MODIS: modis_simulator.F90 (mod_modis_sim) as COSP_Modis_Simulator drives it (cosp_modis_simulator.F90:69-296)
//
// Arrays: t, p, dtau_s, dtau_c, the four water contents and the four radii (npoints,nlev); ph (npoints,nlev+1); boxptop (npoints,ncol) in
// hPa; modis_mean (npoints,17), modis_hist (npoints,7 tau,7 pressure).
//
// Mapping.  k_cosp_fracs: lane = (point, level): the stratiform / convective fractions of a cell as counts over the sub-columns
// (cosp.F90:414-431) and the range check of modis_simulator.F90:202-206 on what the wrapper would hand it.  k_modis_box: lane = (point,
// sub-column), the point fastest.  A sub-column's cell contents (cosp.F90:453-494, cosp_modis_simulator.F90:146-170) are formed by index
// from the gridbox rows and the mask byte - the reference's five (npoints,ncol,nlev) arrays never exist.  The lane walks the levels ONCE:
// the total optical thickness, cloud_top_pressure and weight_by_extinction (both stop at an optical depth of 1 from the top) and the
// adding of the near-infrared layer reflectances from the top depend on the cell alone, not on each other, so the three walks of the
// reference are one loop with their states in registers; the retrieval, which needs the column's total and its phase, follows the loop.
// k_modis_stats: lane = point, modis_L3_simulator with its sums in sub-column order and the wrapper's output rules.
// =====================================================================================================================================
#define GR_HD __host__ __device__ inline
constexpr int MD_NTRIAL = 15, MD_NMEAN = 17;      // num_trial_res; the means of modis_L3_simulator's argument list
enum { MDERR_T, MDERR_P, MDERR_DTAU_S, MDERR_DTAU_C, MDERR_REFF_LSLIQ, MDERR_REFF_LSICE, MDERR_REFF_CVLIQ, MDERR_REFF_CVICE, MDERR_N };

GR_HD float md_exp(float x) { return expf(x); }
GR_HD double md_exp(double x) { return exp(x); }
GR_HD float md_sqrt(float x) { return sqrtf(x); }
GR_HD double md_sqrt(double x) { return sqrt(x); }
GR_HD float md_log10(float x) { return log10f(x); }
GR_HD double md_log10(double x) { return log10(x); }

// fit_to_quadratic, fit_to_cubic, :785-801
template <typename R> GR_HD R md_quad(R x, R c1, R c2, R c3)
{
#pragma clang fp contract(off)
    return c1 + x * (c2 + x * (c3));
}
template <typename R> GR_HD R md_cubic(R x, R c1, R c2, R c3, R c4)
{
#pragma clang fp contract(off)
    return c1 + x * (c2 + x * (c3 + x * c4));
}
// get_g_nir, :726-756; re in microns
template <typename R> GR_HD R md_g_nir(bool liquid, R re)
{
    if (liquid) {
        if (re < (R)8.) return md_quad(re < (R)4. ? (R)4. : re, (R)0.8027, (R)-1.0496e-2, (R)1.7071e-3);
        return md_quad(re > (R)30. ? (R)30. : re, (R)0.7931, (R)5.3087e-3, (R)-7.4995e-5);
    }
    return md_quad(re < (R)5. ? (R)5. : re > (R)90. ? (R)90. : re, (R)0.7432, (R)4.5563e-3, (R)-2.8697e-5);
}
// get_ssa_nir, :759-783
template <typename R> GR_HD R md_ssa_nir(bool liquid, R re)
{
    if (liquid) return md_quad(re < (R)4. ? (R)4. : re > (R)30. ? (R)30. : re, (R)1.0008, (R)-2.5626e-3, (R)1.6024e-5);
    return md_cubic(re < (R)5. ? (R)5. : re > (R)90. ? (R)90. : re, (R)0.9994, (R)-4.5199e-3, (R)3.9370e-5, (R)-1.5235e-7);
}

// trial_re_w, trial_re_i (:85-87) and g_w, w0_w, g_i, w0_i (:235-238): constants of the real kind, evaluated with the reference's own
// expressions in that kind on the host, once a context
template <typename R> struct ModisTab { R re_w[MD_NTRIAL], g_w[MD_NTRIAL], w0_w[MD_NTRIAL], re_i[MD_NTRIAL], g_i[MD_NTRIAL], w0_i[MD_NTRIAL]; };
template <typename R> inline ModisTab<R> md_tables()
{
#pragma clang fp contract(off)
    ModisTab<R> T;
    for (int i = 0; i < MD_NTRIAL; i++) {
        T.re_w[i] = (R)4. + ((R)30. - (R)4.) / (R)(MD_NTRIAL - 1) * (R)i;
        T.re_i[i] = (R)5. + ((R)90. - (R)5.) / (R)(MD_NTRIAL - 1) * (R)i;
        T.g_w[i] = md_g_nir<R>(true, T.re_w[i]); T.w0_w[i] = md_ssa_nir<R>(true, T.re_w[i]);
        T.g_i[i] = md_g_nir<R>(false, T.re_i[i]); T.w0_i[i] = md_ssa_nir<R>(false, T.re_i[i]);
    }
    return T;
}

// two_stream with beam = 2 (:830-907); two_stream_reflectance (:909-982) is its `ref`, expression for expression
template <typename R> GR_DEV void md_two_stream(R tauint, R gint, R w0int, R &ref, R &tra)
{
#pragma clang fp contract(off)
    const R one = (R)1;
    const R f = gint * gint;
    const R tau = (one - w0int * f) * tauint;
    const R w0 = (one - f) * w0int / (one - w0int * f);
    const R g = (gint - f) / (one - f);
    const R gamma1 = ((R)7 - w0 * ((R)4 + (R)3 * g)) / (R)4.0;
    const R gamma2 = -(one - w0 * ((R)4 - (R)3 * g)) / (R)4.0;
    if (w0int > (R)0.9999999) {      // conservative scattering
        ref = gamma1 * tau / (one + gamma1 * tau);
        tra = one - ref;
        return;
    }
    const R xmu = (R)0.866;
    const R rk = md_sqrt(gamma1 * gamma1 - gamma2 * gamma2);
    const R r4 = (one - (rk * xmu) * (rk * xmu)) * (rk + gamma1);
    const R r5 = (one - (rk * xmu) * (rk * xmu)) * (rk - gamma1);
    const R beta = -r5 / r4;
    const R rt = rk * tau, e1 = rt < (R)500. ? rt : (R)500.;
    const R ef1 = md_exp(-e1);
    const R ef2 = md_exp((R)-2 * e1);
    ref = (gamma2 * (one - ef2)) / ((rk + gamma1) * (one - beta * ef2));
    tra = ((R)2 * rk * ef1) / ((rk + gamma1) * (one - beta * ef2));
}

template <typename R> struct ModisArgs {
    int npoints, nlev, ncol;
    int ple_shift;      // `ph` is PLE (npoints,0:nlev): ph(1) = 0, ph(k) = PLE(k-2), as ICARUS's phalf (cosp_modis_simulator.F90:138-141 on gbx%ph)
    int clamp_mr;       // the water contents are GEOS's QLTOT / QITOT: negative ones are zero (GEOS_SatsimGridComp.F90:3700)
    const int32_t *sunlit;
    const R *t, *p, *ph, *dtau_s, *dtau_c;      // dtau_c null: zero
    const uint8_t *frac;
    const R *mr[4], *reff[4];                   // ls liquid, ls ice, cv liquid, cv ice; the cv ones null: zero
    const R *boxptop;
    R *frac_ls, *frac_cv;                       // workspace, (npoints,nlev)
    int32_t *phase; R *ctp, *tau, *size;        // workspace, (npoints,ncol): the L2 results
    uint32_t *err;
    R *mean, *hist;
    int32_t *o_phase; R *o_ctp, *o_tau, *o_size;
    ModisTab<R> tab;
};
template <typename R> GR_DEV R md_ph(const ModisArgs<R> &A, int k, int j)      // k = 0..nlev: pressureLevels(k + 1)
{
    if (!A.ple_shift) return A.ph[(size_t)k * A.npoints + j];
    return k == 0 ? (R)0 : A.ph[(size_t)(k - 1) * A.npoints + j];
}

// cosp.F90:414-431: frac_ls, frac_cv of a cell; modis_simulator.F90:202-206 on a sunlit point's cells (a stratiform / convective array
// is looked at where a sub-column of the cell is stratiform / convective: elsewhere the wrapper hands the simulator zeros).  grid (points, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_cosp_fracs(const ModisArgs<R> A)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    const int n = A.npoints, ncol = A.ncol;
    if (j >= n) return;
    int ls = 0, cv = 0;
    for (int b = 0; b < ncol; b++) {
        const uint8_t f = A.frac[((size_t)k * ncol + b) * n + j];
        ls += f == 1; cv += f == 2;
    }
    const size_t o = (size_t)k * n + j;
    A.frac_ls[o] = (R)ls / (R)ncol; A.frac_cv[o] = (R)cv / (R)ncol;      // a count of ones is exact: the reference's sum of 1.
    if (A.sunlit[j] <= 0) return;
    const R zero = (R)0;
    uint32_t bad = 0;
    if (A.t[o] <= zero) bad |= 1u << MDERR_T;
    if (A.p[o] <= zero) bad |= 1u << MDERR_P;
    if (ls) {
        if (A.dtau_s[o] < zero) bad |= 1u << MDERR_DTAU_S;
        if (A.reff[0][o] < zero) bad |= 1u << MDERR_REFF_LSLIQ;
        if (A.reff[1][o] < zero) bad |= 1u << MDERR_REFF_LSICE;
    }
    if (cv) {
        if (ss_opt(A.dtau_c, o) < zero) bad |= 1u << MDERR_DTAU_C;
        if (ss_opt(A.reff[2], o) < zero) bad |= 1u << MDERR_REFF_CVLIQ;
        if (ss_opt(A.reff[3], o) < zero) bad |= 1u << MDERR_REFF_CVICE;
    }
    if (bad) atomicOr(A.err, bad);
}

// modis_L2_simulator_oneTau (:361-375) and _twoTaus (:212-314) for one sub-column
template <typename R>
__global__ void __launch_bounds__(256) k_modis_box(const ModisArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = A.npoints, nlev = A.nlev, ncol = A.ncol;
    if (idx >= (size_t)n * ncol) return;
    const int j = (int)(idx % n), b = (int)(idx / n);
    const R one = (R)1, zero = (R)0, undef = (R)-1.0E30;
    int phase = 0;
    R ctp = undef, rtau = undef, size = undef;
    if (A.sunlit[j] > 0) {
        R total = 0, ctau = 0, cprod = 0, wtau = 0, wprod = 0, rc = 0, tc = 0;
        bool cdone = false, wdone = false, first = true;
        R p0 = md_ph(A, 0, j);
        for (int k = 0; k < nlev; k++) {
            const size_t o = (size_t)k * n + j;
            const uint8_t f = A.frac[((size_t)k * ncol + b) * n + j];
            const R p1 = md_ph(A, k + 1, j);
            R tau = 0, water = 0, ice = 0, rw = 0, ri = 0;
            if (f == 1 || f == 2) {
                const int c = f == 1 ? 0 : 2;
                const R fr = f == 1 ? A.frac_ls[o] : A.frac_cv[o];
                tau = f == 1 ? A.dtau_s[o] : ss_opt(A.dtau_c, o);
                R mw = ss_opt(A.mr[c], o), mi = ss_opt(A.mr[c + 1], o);
                if (A.clamp_mr) { if (mw < zero) mw = zero; if (mi < zero) mi = zero; }
                water = mw / fr; ice = mi / fr;
                rw = ss_opt(A.reff[c], o); ri = ss_opt(A.reff[c + 1], o);
            }
            // :361-375
            R share;
            if (ice <= zero) share = one;
            else if (water <= zero) share = zero;
            else share = (water / rw) / (water / rw + ice / ((R)0.93 * ri));
            const R tl = share * tau;
            const R ti = tau - tl;
            // :212-217
            const R tt = tl + ti;
            const R lf = tt > zero ? tl / tt : zero;
            total = total + tt;
            if (!cdone) {      // cloud_top_pressure, :531-562, tauLimit 1
                if (ctau + tt > one) {
                    const R dx = one - ctau;
                    ctau = ctau + dx;
                    cprod = cprod + p0 * dx + (p1 - p0) * (dx * dx) / ((R)2. * tt);
                } else {
                    ctau = ctau + tt;
                    cprod = cprod + tt * (p1 + p0) / (R)2.;
                }
                cdone = ctau >= one;
            }
            if (!wdone) {      // weight_by_extinction of the liquid share, :564-588, tauLimit 1
                if (wtau + tt > one) {
                    const R dx = one - wtau;
                    wtau = wtau + dx;
                    wprod = wprod + dx * lf;
                } else {
                    wtau = wtau + tt;
                    wprod = wprod + tt * lf;
                }
                wdone = wtau >= one;
            }
            const R tn = ti + tl;
            if (tn > zero) {      // compute_nir_reflectance, :590-614; compute_toa_reflectace + adding_doubling, :805-828, :984-1005
                const R rwu = rw * (R)1.0e6, riu = ri * (R)1.0e6;
                const R wg = md_g_nir<R>(true, rwu), ww0 = md_ssa_nir<R>(true, rwu), ig = md_g_nir<R>(false, riu), iw0 = md_ssa_nir<R>(false, riu);
                const R g = (tl * wg + ti * ig) / tn;
                const R w0 = (tl * wg * ww0 + ti * ig * iw0) / (g * tn);
                R ref, tra;
                md_two_stream(tn, g, w0, ref, tra);
                if (first) { rc = ref; tc = tra; first = false; }
                else {
                    const R nr = rc + ref * (tc * tc) / (one - rc * ref);
                    tc = (tc * tra) / (one - rc * ref);
                    rc = nr;
                }
            }
            p0 = p1;
        }
        if (total >= (R)0.3) {      // min_OpticalThickness
            rtau = total;
            ctp = cprod / ctau;
            const R ilf = wprod / wtau;
            phase = ilf >= (R)0.7 ? 1 : ilf <= one - (R)0.7 ? 2 : 3;
            // retrieve_re (:618-678) with interpolate_to_min (:680-722): the first minimum of |predicted - observed| over the 15 trial
            // radii with its two neighbours, kept in a sliding window
            const bool liq = phase != 2;
            int m = 0;
            R best = 0, dl = 0, dm = 0, dn = 0, xl = 0, xm = 0, xn = 0, dlast = 0, xlast = 0;
#pragma unroll
            for (int i = 0; i < MD_NTRIAL; i++) {
                const R x = liq ? A.tab.re_w[i] : A.tab.re_i[i];
                R pred, tr;
                md_two_stream(total, liq ? A.tab.g_w[i] : A.tab.g_i[i], liq ? A.tab.w0_w[i] : A.tab.w0_i[i], pred, tr);
                const R d = pred - rc;
                const R ad = d < zero ? -d : d;
                if (i == m + 1) { dn = d; xn = x; }
                if (i == 0 || ad < best) { best = ad; m = i; dl = dlast; xl = xlast; dm = d; xm = x; }
                dlast = d; xlast = x;
            }
            R dlo, dup, xlo, xup;
            if (m == 0) { dlo = dm; xlo = xm; dup = dn; xup = xn; }
            else if (m == MD_NTRIAL - 1 || dl * dm < zero) { dlo = dl; xlo = xl; dup = dm; xup = xm; }
            else { dlo = dm; xlo = xm; dup = dn; xup = xn; }
            const R re = dlo * dup < zero ? xup - dup * (xup - xlo) / (dup - dlo) : (R)-999.;
            size = (R)1.0e-06 * re;
            if (size < zero && size != undef) size = (R)1.0e-06 * (R)-999.;
            if (ctp > (R)700. * (R)100.) ctp = A.boxptop[idx] * (R)100.;      // :313-314
        }
    }
    A.phase[idx] = phase; A.ctp[idx] = ctp; A.tau[idx] = rtau; A.size[idx] = size;
    if (A.o_phase) A.o_phase[idx] = phase;
    if (A.o_ctp) A.o_ctp[idx] = ctp;
    if (A.o_tau) A.o_tau[idx] = rtau;
    if (A.o_size) A.o_size[idx] = size;
}

// modis_L3_simulator (:445-527) for one point and what the wrapper does with it (cosp_modis_simulator.F90:205-263, :338-339)
constexpr int MD_STATS_T = 128;
template <typename R>
__global__ void __launch_bounds__(MD_STATS_T) k_modis_stats(const ModisArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    __shared__ uint16_t s_cnt[42][MD_STATS_T];      // sub-columns per (pressure, tau) bin; a lane touches its own column only
    const int j = blockIdx.x * blockDim.x + threadIdx.x, t = threadIdx.x;
    const int n = A.npoints, ncol = A.ncol;
    if (j >= n) return;
    const R zero = (R)0, undef = (R)-1.0E30;
    if (A.sunlit[j] <= 0) {
        if (A.mean) for (int c = 0; c < MD_NMEAN; c++) A.mean[(size_t)c * n + j] = undef;
        if (A.hist) for (int c = 0; c < 49; c++) A.hist[(size_t)c * n + j] = undef;
        return;
    }
    for (int c = 0; c < 42; c++) s_cnt[c][t] = 0;
    int cT = 0, cW = 0, cI = 0, hi = 0, lo = 0;
    R sT = 0, sW = 0, sI = 0, lT = 0, lW = 0, lI = 0, zW = 0, zI = 0, pT = 0, wW = 0, wI = 0;
    for (int b = 0; b < ncol; b++) {
        const size_t o = (size_t)b * n + j;
        const int ph = A.phase[o];
        const R size = A.size[o], tau = A.tau[o], ctp = A.ctp[o];
        if (!(size > zero) || ph == 0) continue;      // validRetrievalMask, cloudMask
        const R lt = md_log10(tau < zero ? -tau : tau);
        cT++; sT = sT + tau; lT = lT + lt; pT = pT + ctp;
        if (ctp <= (R)440. * (R)100.) hi++;
        if (ctp > (R)680. * (R)100.) lo++;
        if (ph == 1) { cW++; sW = sW + tau; lW = lW + lt; zW = zW + size; wW = wW + size * tau; }
        if (ph == 2) { cI++; sI = sI + tau; lI = lI + lt; zI = zI + size; wI = wI + size * tau; }
        int it = -1, ip = -1;
        if (tau >= (R)0.3) it = 0;
        if (tau >= (R)1.3) it = 1;
        if (tau >= (R)3.6) it = 2;
        if (tau >= (R)9.4) it = 3;
        if (tau >= (R)23.) it = 4;
        if (tau >= (R)60.) it = 5;
        if (ctp >= (R)0.) ip = 0;
        if (ctp >= (R)18000.) ip = 1;
        if (ctp >= (R)31000.) ip = 2;
        if (ctp >= (R)44000.) ip = 3;
        if (ctp >= (R)56000.) ip = 4;
        if (ctp >= (R)68000.) ip = 5;
        if (ctp >= (R)80000.) ip = 6;
        if (it >= 0 && ip >= 0) s_cnt[ip * 6 + it][t]++;
    }
    if (A.mean) {
        const R nc = (R)ncol;
        const R mid = (R)cT - (R)hi - (R)lo;
        const R nT = cT == 0 ? (R)-1. : (R)cT, nW = cW == 0 ? (R)-1. : (R)cW, nI = cI == 0 ? (R)-1. : (R)cI;
        const R conv = (R)2. / (R)3. * (R)1000.;      // LWP_conversion
        R m[MD_NMEAN];
        m[0] = nT / nc; m[1] = nW / nc; m[2] = nI / nc;
        for (int c = 0; c < 3; c++) m[c] = m[c] > zero ? m[c] : zero;
        m[3] = (R)hi / nc; m[4] = mid / nc; m[5] = (R)lo / nc;
        m[6] = sT / nT; m[7] = sW / nW; m[8] = sI / nI;
        m[9] = lT / nT; m[10] = lW / nW; m[11] = lI / nI;
        m[12] = zW / nW; m[13] = zI / nI;
        m[14] = pT / (R)(cT > 1 ? cT : 1);
        m[15] = conv * wW / nW;
        m[16] = conv * (R)0.93 * wI / nI;
#pragma unroll
        for (int c = 0; c < MD_NMEAN; c++) A.mean[(size_t)c * n + j] = m[c];
    }
    if (A.hist)      // tau index 1 stays R_UNDEF, 2-7 hold the six bins, the pressure index is reversed
        for (int ip = 0; ip < 7; ip++) {
            A.hist[(size_t)((6 - ip) * 7) * n + j] = undef;
            for (int it = 0; it < 6; it++) A.hist[(size_t)((6 - ip) * 7 + it + 1) * n + j] = (R)s_cnt[ip * 6 + it][t] / (R)ncol;
        }
}

// GEOS_SatsimGridComp.F90:3574-3580, :3696: the height of the layer centres above the surface from the edge heights ZLE (npoints,0:lm);
// grid (points, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_cosp_zfull(int n, int lm, const R *__restrict__ zle, R *__restrict__ zfull)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (j >= n) return;
    const R zs = zle[(size_t)lm * n + j];
    zfull[(size_t)k * n + j] = (R)0.5 * ((zle[(size_t)k * n + j] - zs) + (zle[(size_t)(k + 1) * n + j] - zs));
}

}  // namespace geosrad
