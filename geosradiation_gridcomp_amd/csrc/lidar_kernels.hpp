// lidar_kernels.hpp -- the lidar path of GEOSsatsim_GridComp's COSP on the device, on the SCOPS byte mask that satsim_kernels.hpp makes:
// COSP_LIDAR (cosp_lidar.F90:44-82) with lidar_simulator and parasol (actsim/lidar_simulator.F90:25-415, :419-553) and diag_lidar with
// COSP_CLDFRAC and COSP_CFAD_SR (actsim/lmd_ipsl_stats.F90:34-179, :186-264, :270-437) as cosp_stats.F90:126-140 calls and leaves it.
// The statements are the reference's, operation by operation, in the real kind R (contraction off); exp and the divisions are the precise
// device functions.
//
// Arrays: the reference's Fortran layouts, the point index fastest: p, t, pplay, the four contents and the four radii (npoints,nlev), presf
// (npoints,nlev+1), frac_out (npoints,ncol,nlev) as one byte per cell, cfad_sr (npoints,15,nlev).  Level 1 is the top of the atmosphere;
// the reference counts from the surface, so its level k is level nlev+1-k here and its presf(:,k) is presf(:,nlev+2-k).
//
// The reference's arithmetic decides the split.  The layer thickness is a difference of a height sum built from the surface up (:262-266,
// :320-321); the optical depths are running sums from the top, one for the molecules and one for each of the four particle kinds, each
// added on its own and only then summed (:323-338, :362-367); a layer's own depth is again a difference of two running sums (:346, :374).
// None of these is the plain increment in fp32, so the kernels carry the same sums in the same order.
//
// Mapping.  k_lidar_point: what does not depend on the sub-column, as (npoints,nlev) planes.  Lane = (point, level) for the four kp
// polynomials and the stratiform / convective fractions of a cell (cosp.F90:414-431); the lanes of level 1 also take their point's two
// walks: up for the heights and 3/4 Qscat rhoair (the factor of alpha that multiplies the content), with the range check, and down for
// tau_mol, beta_mol and pmol.  k_lidar_box: lane = (point, sub-column), the point fastest; one walk down with the four particle sums in
// registers; a cell's contents are formed by index from the gridbox rows and the mask byte (cosp.F90:453-494).  It leaves one byte per cell, the CFAD bin of the scattering ratio, one byte per sub-column with COSP_CLDFRAC's
// eight flags, and the two surface-level optical depths PARASOL needs.  k_lidar_stats: lane = (point, level) for lidarcld and cfad_sr; the
// lanes of level 1 also form cldlayer and the PARASOL reflectances of their point, summed in sub-column order.
//
// "Cloudy" (ratio > 5) and "usable" (ratio > 0.01) follow from the bin byte: S_cld and S_att are bin edges (:223-236).  A pnorm at or above
// undef - 1 cannot occur for finite inputs (it is bounded by kp / (2 x 0.7) < 0.1), so a sub-column is undefined only where pmol
// disqualifies its whole level, and the order-dependent sum of lmd_ipsl_stats.F90:249-254 over a single undefined sub-column is not
// reproduced: a non-finite pnorm raises the input flag.
#pragma once
#include <cmath>
#include <cstdint>

#include "satsim_kernels.hpp"      // ss_exp, ss_opt

namespace geosrad {

constexpr int LD_NBIN = 15, LD_NREFL = 5, LD_NCAT = 4, LD_NTAU = 7;      // SR_BINS, PARASOL_NREFL, LIDAR_NCAT; parasol's nbtau
constexpr int LD_ABOVE = 15, LD_NOBIN = 16, LD_UNDEF = 255;              // bin bytes beside 0..14: above the last edge, in no bin, undefined
enum { LDERR_P, LDERR_T, LDERR_PNORM, LDERR_N };

// what lidar_simulator and parasol evaluate once a call in the real kind: on the host, with the reference's own expressions, once a context
template <typename R> struct LidarTab {
    R amol;                                       // 8.0*pi/3.0, pi = dacos(-1.D0) rounded to the kind (:191, :277)
    R pol[2][2][5];                               // polpart: [ice_type][liquid, ice][5] (:200-241)
    R aA[LD_NREFL][LD_NTAU - 1], bA[LD_NREFL][LD_NTAU - 1], aB[LD_NREFL][LD_NTAU - 1], bB[LD_NREFL][LD_NTAU - 1];      // :527-534
    R r_norm[LD_NREFL];                           // :508-509
};
template <typename R> inline LidarTab<R> ld_tables()
{
#pragma clang fp contract(off)
    LidarTab<R> T;
    const R pi = (R)std::acos(-1.0);
    T.amol = (R)8.0 * pi / (R)3.0;
    const R liq[5] = {(R)2.6980e-8, (R)-3.7701e-6, (R)1.6594e-4, (R)-0.0024, (R)0.0626};
    const R ice[2][5] = {{(R)-1.0176e-8, (R)1.7615e-6, (R)-1.0480e-4, (R)0.0019, (R)0.0460},
                         {(R)1.3615e-8, (R)-2.04206e-6, (R)7.51799e-5, (R)0.00078213, (R)0.0182131}};
    for (int s = 0; s < 2; s++)
        for (int c = 0; c < 5; c++) { T.pol[s][0][c] = liq[c]; T.pol[s][1][c] = ice[s][c]; }
    const R tau[LD_NTAU] = {(R)0., (R)1., (R)5., (R)10., (R)20., (R)50., (R)100.};
    const R tetas[LD_NREFL] = {(R)0., (R)20., (R)40., (R)60., (R)80.};
    const R rlumA[LD_NREFL][LD_NTAU] = {{(R)0.03, (R)0.090886, (R)0.283965, (R)0.480587, (R)0.695235, (R)0.908229, (R)1.0},
                                        {(R)0.03, (R)0.072185, (R)0.252596, (R)0.436401, (R)0.631352, (R)0.823924, (R)0.909013},
                                        {(R)0.03, (R)0.058410, (R)0.224707, (R)0.367451, (R)0.509180, (R)0.648152, (R)0.709554},
                                        {(R)0.03, (R)0.052498, (R)0.175844, (R)0.252916, (R)0.326551, (R)0.398581, (R)0.430405},
                                        {(R)0.03, (R)0.034730, (R)0.064488, (R)0.081667, (R)0.098215, (R)0.114411, (R)0.121567}};
    const R rlumB[LD_NREFL][LD_NTAU] = {{(R)0.03, (R)0.092170, (R)0.311941, (R)0.511298, (R)0.712079, (R)0.898243, (R)0.976646},
                                        {(R)0.03, (R)0.087082, (R)0.304293, (R)0.490879, (R)0.673565, (R)0.842026, (R)0.912966},
                                        {(R)0.03, (R)0.083325, (R)0.285193, (R)0.430266, (R)0.563747, (R)0.685773, (R)0.737154},
                                        {(R)0.03, (R)0.084935, (R)0.233450, (R)0.312280, (R)0.382376, (R)0.446371, (R)0.473317},
                                        {(R)0.03, (R)0.054157, (R)0.089911, (R)0.107854, (R)0.124127, (R)0.139004, (R)0.145269}};
    const R pi2 = std::acos((R)-1.0);
    for (int it = 0; it < LD_NREFL; it++) {
        T.r_norm[it] = (R)1. / std::cos(pi2 / (R)180. * tetas[it]);
        for (int ny = 0; ny < LD_NTAU - 1; ny++) {
            T.aA[it][ny] = (rlumA[it][ny + 1] - rlumA[it][ny]) / (tau[ny + 1] - tau[ny]);
            T.bA[it][ny] = rlumA[it][ny] - T.aA[it][ny] * tau[ny];
            T.aB[it][ny] = (rlumB[it][ny + 1] - rlumB[it][ny]) / (tau[ny + 1] - tau[ny]);
            T.bB[it][ny] = rlumB[it][ny] - T.aB[it][ny] * tau[ny];
        }
    }
    return T;
}

template <typename R> struct LidarArgs {
    int npoints, nlev, ncol, ice_type;
    int ple_shift;      // `presf` is PLE (npoints,0:nlev): presf(1) = 0, presf(k) = PLE(k-2) (GEOS_SatsimGridComp.F90:3672, cosp_lidar.F90:60-61)
    int clamp_mr;       // the water contents are GEOS's QLTOT / QITOT: negative ones are zero (GEOS_SatsimGridComp.F90:3700)
    int ocean;          // `land` is FROCEAN: land = 1 where it is < 0.5, else 0 (GEOS_SatsimGridComp.F90:3548, :3584)
    const R *p, *t, *presf, *pplay;
    const uint8_t *frac;
    const R *mr[4], *reff[4];                   // ls liquid, ls ice, cv liquid, cv ice; the cv ones null: zero
    const R *land;
    R *dz, *taumol, *betamol, *pmol, *rho, *kp[4], *frac_ls, *frac_cv;      // workspace, (npoints,nlev)
    uint8_t *bin;                               // workspace, (npoints,ncol,nlev): the CFAD bin of the cell's scattering ratio
    uint8_t *cat;                               // workspace, (npoints,ncol): bit c cloudy, bit 4 + c usable in category c (low, mid, high, total)
    R *tau_liq, *tau_ice;                       // workspace, (npoints,ncol): tautot_S_liq, tautot_S_ice
    uint32_t *err;
    R *lidarcld, *cldlayer, *cfad, *parasol, *o_pmol, *o_beta, *o_tau, *o_refl;
    LidarTab<R> tab;
};
template <typename R> GR_DEV R ld_presf(const LidarArgs<R> &A, int k, int j)      // k = 0..nlev: presf(k + 1)
{
    if (!A.ple_shift) return A.presf[(size_t)k * A.npoints + j];
    return k == 0 ? (R)0 : A.presf[(size_t)(k - 1) * A.npoints + j];
}
template <typename R> GR_DEV R ld_rad(const R *reff, size_t o)      // :254-259
{
    R r = ss_opt(reff, o);
    r = r > (R)0. ? r : (R)0.;
    return r < (R)70.0e-6 ? r : (R)70.0e-6;
}

// lidar_simulator.F90:245-295, :320-325, :342-354 and cosp.F90:414-431; grid (points, levels).  Every lane does what belongs to its own
// (point, level) alone: the four kp polynomials and the two fractions, 30 mask bytes a lane.  The lanes of level 1 then take the two
// walks of their point, which are serial in the level.  (With the fractions inside the walk, 72 x 30 dependent byte loads a lane on 97 200
// lanes, this kernel took as long as k_lidar_box: profiles/satsim_lidar.md.)
template <typename R>
__global__ void __launch_bounds__(256) k_lidar_point(const LidarArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int j = blockIdx.x * blockDim.x + threadIdx.x, lev = blockIdx.y;
    const int n = A.npoints, nlev = A.nlev, ncol = A.ncol;
    if (j >= n) return;
    const R zero = (R)0, one = (R)1;
    {
        const size_t o = (size_t)lev * n + j;
        // :284-295
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const R rad = ld_rad(A.reff[i], o);
            R kp = 0;
            if (rad > zero) {
                const R *c = A.tab.pol[A.ice_type][i & 1];
                const R x = rad * (R)1e6, x2 = x * x;
                kp = c[0] * (x2 * x2) + c[1] * (x2 * x) + c[2] * x2 + c[3] * x + c[4];
            }
            A.kp[i][o] = kp;
        }
        int ls = 0, cv = 0;
        for (int b = 0; b < ncol; b++) {
            const uint8_t f = A.frac[((size_t)lev * ncol + b) * n + j];
            ls += f == 1; cv += f == 2;
        }
        A.frac_ls[o] = (R)ls / (R)ncol; A.frac_cv[o] = (R)cv / (R)ncol;      // a count of ones is exact: the reference's sum of 1.
    }
    if (lev != 0) return;
    uint32_t bad = 0;
    // :245, :262-266, :276: the heights from the surface up; the thickness of a layer is the difference of its two edge heights
    R zlow = 0, pflow = ld_presf(A, nlev, j);
    for (int k = nlev - 1; k >= 0; k--) {
        const size_t o = (size_t)k * n + j;
        const R p = A.p[o], t = A.t[o];
        if (p <= zero) bad |= 1u << LDERR_P;
        if (t <= zero) bad |= 1u << LDERR_T;
        const R rhoair = p / ((R)287.04 * t);
        const R pf = ld_presf(A, k, j);
        const R zup = zlow - (pf - pflow) / (rhoair * (R)9.81);
        A.dz[o] = zup - zlow;
        A.rho[o] = (R)3.0 / (R)4.0 * (R)2.0 * rhoair;      // 3.0/4.0 * Qscat * rhoair, :306-307
        A.betamol[o] = p / (R)1.38e-23 / t * (R)6.2446e-32;
        zlow = zup; pflow = pf;
    }
    if (bad) atomicOr(A.err, bad);
    // :277, :320-325, :342-354: the molecular optical depth from the top and the molecular signal
    R tabove = 0;
    for (int k = 0; k < nlev; k++) {
        const size_t o = (size_t)k * n + j;
        const R beta = A.betamol[o];
        const R lay0 = A.tab.amol * beta * A.dz[o];
        const R tau = k == 0 ? lay0 : lay0 + tabove;
        R pmol;
        if (k == 0) pmol = beta / ((R)2. * tau) * (one - ss_exp((R)-2.0 * tau));
        else {
            const R lay = tau - tabove;
            if (lay > zero) pmol = beta * ss_exp((R)-2.0 * tabove) / ((R)2. * lay) * (one - ss_exp((R)-2.0 * lay));
            else pmol = beta * ss_exp((R)-2.0 * tabove);
        }
        A.taumol[o] = tau; A.pmol[o] = pmol;
        if (A.o_pmol) A.o_pmol[o] = pmol;
        tabove = tau;
    }
}

// the CFAD bin of a scattering ratio (lmd_ipsl_stats.F90:223-240, :250): bin i holds srbval_ext(i-1) < x <= srbval_ext(i)
template <typename R> GR_DEV int ld_bin(R x, R xmax)
{
    const R e[LD_NBIN - 1] = {(R)0.01, (R)1.2, (R)3.0, (R)5.0, (R)7.0, (R)10.0, (R)15.0, (R)20.0, (R)25.0, (R)30.0, (R)40.0, (R)50.0, (R)60.0, (R)80.0};
    if (!(x > (R)-1.0)) return LD_NOBIN;
    int c = 0;
#pragma unroll
    for (int i = 0; i < LD_NBIN - 1; i++) c += x > e[i];
    return c + (x > xmax);
}

// lidar_simulator.F90:298-338, :362-407 for one sub-column; lmd_ipsl_stats.F90:119-133, :318-334, :384-406
template <typename R>
__global__ void __launch_bounds__(256) k_lidar_box(const LidarArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = A.npoints, nlev = A.nlev, ncol = A.ncol;
    if (idx >= (size_t)n * ncol) return;
    const int j = (int)(idx % n), b = (int)(idx / n);
    const R zero = (R)0, one = (R)1;
    const R xmax = (R)999.999 - (R)1.0;      // undef - 1.0, :113
    const R rhopart[2] = {(R)1.0e+03, (R)0.5e+03};
    R tp[4] = {0, 0, 0, 0};      // tau_part(:,k,i), the four running sums from the top
    R tabove = 0;
    unsigned cat = 0;
    bool odd = false;
    for (int k = 0; k < nlev; k++) {
        const size_t o = (size_t)k * n + j, oc = ((size_t)k * ncol + b) * n + j;
        const uint8_t f = A.frac[oc];
        const R dz = A.dz[o];
        R betatot = A.betamol[o];
        if (f == 1 || f == 2) {
            const int c = f == 1 ? 0 : 2;
            const R fr = f == 1 ? A.frac_ls[o] : A.frac_cv[o], rho = A.rho[o];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int i = c + s;
                R q = ss_opt(A.mr[i], o);
                if (A.clamp_mr && q < zero) q = zero;
                q = q / fr;
                const R rad = ld_rad(A.reff[i], o);
                const R alpha = rad > zero ? rho * q / (rhopart[s] * rad) : zero;
                const R lay = (R)0.7 * alpha * dz;
                // the other kinds add a zero to their sums and to betatot, which changes neither
                if (f == 1) tp[s] = k == 0 ? lay : lay + tp[s];
                else tp[2 + s] = k == 0 ? lay : lay + tp[2 + s];
                betatot = betatot + (f == 1 ? A.kp[s][o] : A.kp[2 + s][o]) * alpha;
            }
        }
        R tautot = A.taumol[o];
#pragma unroll
        for (int i = 0; i < 4; i++) tautot = tautot + tp[i];
        R pnorm;
        if (k == 0) pnorm = betatot / ((R)2. * tautot) * (one - ss_exp((R)-2.0 * tautot));
        else {
            const R lay = tautot - tabove;
            if (lay > zero) pnorm = betatot * ss_exp((R)-2.0 * tabove) / ((R)2. * lay) * (one - ss_exp((R)-2.0 * lay));
            else pnorm = betatot * ss_exp((R)-2.0 * tabove);
        }
        tabove = tautot;
        if (A.o_beta) A.o_beta[oc] = pnorm;
        if (A.o_tau) A.o_tau[oc] = tautot;
        odd |= !(pnorm - pnorm == zero);      // not finite
        const R pmol = A.pmol[o];
        int code = LD_UNDEF;
        if (pnorm < xmax && pmol < xmax && pmol > zero) code = ld_bin(pnorm / pmol, xmax);
        A.bin[oc] = (uint8_t)code;
        // COSP_CLDFRAC, :384-406: S_cld = 5 and S_att = 0.01 are the upper edges of bins 4 and 1
        const unsigned cloudy = code >= 4 && code <= LD_ABOVE, usable = code >= 1 && code <= LD_ABOVE;
        const R p1 = A.pplay[o];
        int iz = 0;
        if (p1 > zero && p1 < (R)440. * (R)100.) iz = 2;
        else if (p1 >= (R)440. * (R)100. && p1 < (R)680. * (R)100.) iz = 1;
        cat |= (cloudy << iz) | (cloudy << 3) | (usable << (4 + iz)) | (usable << 7);
    }
    if (odd) atomicOr(A.err, 1u << LDERR_PNORM);
    A.cat[idx] = (uint8_t)cat;
    // :402-407
    R sl = 0, si = 0;
    sl = sl + tp[0] + tp[2];
    si = si + tp[1] + tp[3];
    A.tau_liq[idx] = sl; A.tau_ice[idx] = si;
}

// parasol (lidar_simulator.F90:505-550) for one sub-column
template <typename R> GR_DEV void ld_parasol(const LidarTab<R> &T, R sl, R si, R (&refl)[LD_NREFL])
{
#pragma clang fp contract(off)
    const R zero = (R)0;
    const R tau[LD_NTAU] = {(R)0., (R)1., (R)5., (R)10., (R)20., (R)50., (R)100.};
    sl = sl > tau[0] ? sl : tau[0];
    si = si > tau[0] ? si : tau[0];
    R ts = si + sl;
    R fl = (R)1., fi = (R)0.;
    if (ts > zero) { fl = sl / ts; fi = si / ts; }
    ts = ts < tau[LD_NTAU - 1] ? ts : tau[LD_NTAU - 1];
    int ny = -1;      // the last interval that holds ts, as the WHERE of :536-543 leaves it
#pragma unroll
    for (int i = 0; i < LD_NTAU - 1; i++)
        if (ts >= tau[i] && ts <= tau[i + 1]) ny = i;
    // one row of the four tables by the lane's own index: a load, not 120 scalars held at once
    const int i = ny < 0 ? 0 : ny;
#pragma unroll
    for (int it = 0; it < LD_NREFL; it++) {
        R ra = 0, rb = 0;
        if (ny >= 0) { ra = T.aA[it][i] * ts + T.bA[it][i]; rb = T.aB[it][i] * ts + T.bB[it][i]; }
        refl[it] = (fl * ra + fi * rb) * T.r_norm[it];
    }
}

// diag_lidar (lmd_ipsl_stats.F90:140-176) and what cosp_stats.F90:137-140 does to its results; grid (points, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_lidar_stats(const LidarArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    __shared__ uint16_t s_cnt[LD_NBIN][256];      // sub-columns per bin; a lane touches its own column only
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y, t = threadIdx.x;
    const int n = A.npoints, ncol = A.ncol;
    if (j >= n) return;
    const R zero = (R)0, undef = (R)-1.0E30, lundef = (R)999.999, xmax = lundef - (R)1.0;
    const size_t o = (size_t)k * n + j;
    const R nc = (R)ncol;
    if (A.lidarcld || A.cfad) {
        for (int c = 0; c < LD_NBIN; c++) s_cnt[c][t] = 0;
        int cloudy = 0, usable = 0;
        for (int b = 0; b < ncol; b++) {
            const int code = A.bin[((size_t)k * ncol + b) * n + j];
            if (code < LD_NBIN) s_cnt[code][t]++;
            cloudy += code >= 4 && code <= LD_ABOVE; usable += code >= 1 && code <= LD_ABOVE;
        }
        // :411-415; a sum of ones is the count itself
        if (A.lidarcld) A.lidarcld[o] = usable > 0 ? (R)cloudy / (R)usable : undef;
        if (A.cfad) {      // :245-260: a level that pmol disqualifies is undefined in every sub-column
            const R pmol = A.pmol[o];
            const bool off = !(pmol < xmax && pmol > zero);
            for (int c = 0; c < LD_NBIN; c++) A.cfad[((size_t)k * LD_NBIN + c) * n + j] = off ? undef : (R)s_cnt[c][t] / nc;
        }
    }
    if (k != 0) return;
    if (A.cldlayer) {      // :419-434
        int cl[LD_NCAT] = {0, 0, 0, 0}, us[LD_NCAT] = {0, 0, 0, 0};
        for (int b = 0; b < ncol; b++) {
            const unsigned c = A.cat[(size_t)b * n + j];
#pragma unroll
            for (int z = 0; z < LD_NCAT; z++) { cl[z] += (c >> z) & 1u; us[z] += (c >> (4 + z)) & 1u; }
        }
#pragma unroll
        for (int z = 0; z < LD_NCAT; z++) A.cldlayer[(size_t)z * n + j] = us[z] > 0 ? (R)cl[z] / (R)us[z] : undef;
    }
    if (A.parasol || A.o_refl) {      // :162-176
        R sum[LD_NREFL] = {0, 0, 0, 0, 0};
        for (int b = 0; b < ncol; b++) {
            R refl[LD_NREFL];
            ld_parasol(A.tab, A.tau_liq[(size_t)b * n + j], A.tau_ice[(size_t)b * n + j], refl);
#pragma unroll
            for (int it = 0; it < LD_NREFL; it++) {
                sum[it] = sum[it] + refl[it];
                if (A.o_refl) A.o_refl[((size_t)it * ncol + b) * n + j] = refl[it];
            }
        }
        if (A.parasol) {
            R land = A.land[j];
            if (A.ocean) land = land < (R)0.5 ? (R)1.0 : (R)0.0;
            const R m0 = (R)1.0 - land, m = m0 > (R)0.0 ? m0 : (R)0.0;
#pragma unroll
            for (int it = 0; it < LD_NREFL; it++) {
                R v = sum[it] / nc;
                v = v * m + ((R)1.0 - m) * lundef;
                A.parasol[(size_t)it * n + j] = v == lundef ? undef : v;
            }
        }
    }
}

}  // namespace geosrad
