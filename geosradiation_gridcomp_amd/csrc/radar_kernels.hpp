// radar_kernels.hpp -- the front end of the radar simulator of GEOSsatsim_GridComp's COSP on the device, on the SCOPS byte mask that
// satsim_kernels.hpp makes: prec_scops (llnl/prec_scops.f:25-267), the sub-grid hydrometeor contents of cosp_iter (cosp.F90:399-519 with
// use_precipitation_fluxes = .false.), and the gaseous attenuation of quickbeam: gases (quickbeam/gases.f90) for every volume and
// path_integral / avint (quickbeam/math_lib.f90:96-155, :160-393) for every gate, as radar_simulator.f90:470-484 calls them on the matrices of
// cosp_radar.F90:136-144.  What comes after them - dsd, zeff, the Mie sum with its hp%Ze_scaled cache - depends on the order of the points
// and is not here.
//
// Arrays: the reference's Fortran layouts, the point index fastest: gridbox fields (npoints,nlev), masks (npoints,ncol,nlev) as one byte per
// cell, mr_sub (npoints,nlev,9), mr_hydro_sg (npoints,ncol,nlev,9).  Level 1 is the top of the atmosphere, which is how prec_scops takes
// its arguments (cosp.F90:404-411); COSP's own gridbox arrays count from the surface.
//
// Mapping.  k_prec_columns: lane = (point, sub-column), one walk down the mask for the two column-wide flags frac_out_ls / frac_out_cv
// (prec_scops.f:65-86), one byte.  k_prec_scops: lane = point, because the levels are a serial recurrence a point and each level needs two
// any-over-sub-columns decisions a kind before it can choose its possibility; with the point index fastest every byte row a wave reads or
// writes is 64 consecutive bytes.  A level is two walks over the sub-columns - decide, then write - and the row of prec_frac above is the
// only carried state: it is read back from the output.  A level without precipitation of either kind is one walk of zero stores.
// k_sghydro: lane = (point, level), the counts and the nine divisions.  k_sghydro_expand: lane = (point, sub-column) on a (.., levels) grid,
// only when the expanded array is asked for.  k_radar_gases: lane = (point, level), the 78 lines of Liebe's model from constant memory, every
// lane of a wave on the same line.  k_radar_gas_parab: lane = (point, gate), the parabola through a gate and its two neighbours.
// k_radar_gas_path: lane = (point, gate), AVINT summed directly in the reference's order from those coefficients: (nlev - 3) / 2 steps a
// lane on average, 4 loads and 23 flops a step.
#pragma once
#include <cmath>
#include <cstdint>

#include "satsim_kernels.hpp"

namespace geosrad {

constexpr int RD_NHYDRO = 9;
enum { RDERR_P, RDERR_T, RDERR_ZLEV, RDERR_N };

// ---- prec_scops ----------------------------------------------------------------------------------------------------------------------
template <typename R> struct PrecArgs {
    int npoints, nlev, ncol, cv_col;
    const R *ls[3], *cv[2];            // the rates are ls[0] + ls[1] + ls[2] and cv[0] + cv[1] in this order, a null term left out (cosp.F90:404-408)
    const uint8_t *frac;               // (npoints,ncol,nlev)
    uint8_t *colflag;                  // workspace, (npoints,ncol): bit 0 stratiform, bit 1 convective cloud somewhere in the sub-column
    uint8_t *prec;                     // (npoints,ncol,nlev)
};

// prec_scops.f:65-86; lane = (point, sub-column), the point fastest
template <typename R>
__global__ void __launch_bounds__(256) k_prec_columns(const PrecArgs<R> A)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)A.npoints * A.ncol;
    if (i >= n) return;
    unsigned f = 0;
    for (int l = 0; l < A.nlev; l++) {
        const unsigned v = A.frac[(size_t)l * n + i];
        f |= (v == 1u ? 1u : 0u) | (v == 2u ? 2u : 0u);
    }
    A.colflag[i] = (uint8_t)f;
}

template <typename R> GR_DEV R rd_rate(const R *const *term, int nterm, size_t o)
{
#pragma clang fp contract(off)
    R s = term[0] ? term[0][o] : (R)0;
    for (int k = 1; k < nterm; k++)
        if (term[k]) s = s + term[k][o];
    return s;
}

// prec_scops.f:89-265; lane = point.  The first level is the general one with nothing above it.  bit 0 of a byte below is the large-scale
// kind, bit 1 the convective one, which is also prec_frac's own coding (1, 2, 3 = both).
template <typename R>
__global__ void __launch_bounds__(256) k_prec_scops(const PrecArgs<R> A)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.npoints) return;
    const size_t np = (size_t)A.npoints, row = np * A.ncol;
    unsigned any4 = 0;                                                       // possibility Four's any: cloud of the kind anywhere in the column
    for (int b = 0; b < A.ncol; b++) any4 |= A.colflag[(size_t)b * np + j];
    for (int l = 0; l < A.nlev; l++) {
        const size_t o = (size_t)l * np + j;
        const unsigned active = (rd_rate(A.ls, 3, o) > (R)0 ? 1u : 0u) | (rd_rate(A.cv, 2, o) > (R)0 ? 2u : 0u);
        const uint8_t *f0 = A.frac + (size_t)l * row + j, *f1 = f0 + row;
        uint8_t *out = A.prec + (size_t)l * row + j;
        const uint8_t *up = l ? out - row : out;                               // the row above, not read at the first level
        const bool below = l + 1 < A.nlev;
        if (!active) {
            for (int b = 0; b < A.ncol; b++) out[(size_t)b * np] = 0;
            continue;
        }
        auto cloud = [](unsigned v) { return (v == 1u ? 1u : 0u) | (v == 2u ? 2u : 0u); };
        unsigned any1 = 0, any3 = 0;                                         // ONE&TWO and THREE, per kind
        for (int b = 0; b < A.ncol; b++) {
            any1 |= cloud(f0[(size_t)b * np]) | (l ? up[(size_t)b * np] : 0u);
            if (below) any3 |= cloud(f1[(size_t)b * np]);
        }
        // the possibility of each kind: 1 ONE&TWO, 3 THREE, 4 Four, 5 Five
        unsigned poss[2];
        for (int k = 0; k < 2; k++) poss[k] = (any1 >> k & 1u) ? 1u : (any3 >> k & 1u) ? 3u : (any4 >> k & 1u) ? 4u : 5u;
        for (int b = 0; b < A.ncol; b++) {
            const unsigned one = cloud(f0[(size_t)b * np]) | (l ? up[(size_t)b * np] : 0u);
            const unsigned three = below ? cloud(f1[(size_t)b * np]) : 0u;
            const unsigned four = A.colflag[(size_t)b * np + j];
            const unsigned five = 1u | (b < A.cv_col ? 2u : 0u);             // :208-213 all sub-columns, :253-260 the first cv_col
            unsigned v = 0;
            for (int k = 0; k < 2; k++) {
                const unsigned s = poss[k] == 1u ? one : poss[k] == 3u ? three : poss[k] == 4u ? four : five;
                v |= s & (1u << k);
            }
            out[(size_t)b * np] = (uint8_t)(v & active);
        }
    }
}

// ---- the sub-grid hydrometeor contents -----------------------------------------------------------------------------------------------
template <typename R> struct SgHydroArgs {
    int npoints, nlev, ncol;
    const uint8_t *frac, *prec;        // (npoints,ncol,nlev)
    const R *mr[RD_NHYDRO];            // (npoints,nlev), cosp_constants' I_* order; null: zero
    R *frac_ls, *frac_cv, *prec_ls, *prec_cv;      // (npoints,nlev), any may be null
    R *mr_sub;                         // (npoints,nlev,9) or null (workspace when the caller does not want it and the expansion does)
    R *mr_sg;                          // (npoints,ncol,nlev,9) or null
};
// which fraction divides a class (cosp.F90:484-516): 0 frac_ls, 1 frac_cv, 2 prec_ls, 3 prec_cv
GR_DEV int rd_divisor(int c) { return c < 2 ? 0 : c < 4 ? 2 : c < 6 ? 1 : c < 8 ? 3 : 2; }

// cosp.F90:414-431 and :484-516; grid (points, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_sghydro(const SgHydroArgs<R> A)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
    if (j >= A.npoints) return;
    const size_t np = (size_t)A.npoints, base = (size_t)l * np * A.ncol + j;
    int n[4] = {0, 0, 0, 0};
    for (int b = 0; b < A.ncol; b++) {
        const unsigned f = A.frac[base + (size_t)b * np], p = A.prec[base + (size_t)b * np];
        n[0] += f == 1u; n[1] += f == 2u; n[2] += p & 1u; n[3] += p >> 1 & 1u;
    }
    // the reference adds 1. a sub-column and divides by Ncolumns: a count below 2^24 is exact in either kind
    R fr[4];
    for (int k = 0; k < 4; k++) fr[k] = (R)n[k] / (R)A.ncol;
    const size_t o = (size_t)l * np + j, plane = np * A.nlev;
    if (A.frac_ls) A.frac_ls[o] = fr[0];
    if (A.frac_cv) A.frac_cv[o] = fr[1];
    if (A.prec_ls) A.prec_ls[o] = fr[2];
    if (A.prec_cv) A.prec_cv[o] = fr[3];
    for (int c = 0; c < RD_NHYDRO; c++) {
        const R m = A.mr[c] ? A.mr[c][o] : (R)0, d = fr[rd_divisor(c)];
        if (A.mr_sub) A.mr_sub[(size_t)c * plane + o] = d != (R)0 ? m / d : m;
    }
}

// cosp.F90:453-480: the index rule; grid (points x sub-columns, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_sghydro_expand(const SgHydroArgs<R> A)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, np = (size_t)A.npoints, row = np * A.ncol;
    const int l = blockIdx.y;
    if (i >= row) return;
    const size_t j = i % np, cell = (size_t)l * row + i, cells = row * A.nlev, o = (size_t)l * np + j, plane = np * A.nlev;
    const unsigned f = A.frac[cell];
    for (int c = 0; c < RD_NHYDRO; c++) {
        const unsigned kind = (c >= 4 && c < 8) ? 2u : 1u;
        A.mr_sg[(size_t)c * cells + cell] = f == kind ? A.mr_sub[(size_t)c * plane + o] : (R)0;
    }
}

// ---- gases ---------------------------------------------------------------------------------------------------------------------------
// Liebe (1985), the oxygen lines (v0, a1 .. a6) and the water-vapour lines (v1, b1, b2, b3) of gases.f90:35-109.  The reference holds them
// in real*8 arrays initialised from default-real constants: each is the single-precision number, widened where it is used.
constexpr int RD_NO2 = 48, RD_NH2O = 30;
static __constant__ float RD_O2[RD_NO2][7] = {
    {49.4523790f, 0.0000001f, 11.83f, 0.0083f, 0.0f, 0.0056f, 1.7f},    {49.9622570f, 0.0000003f, 10.72f, 0.0085f, 0.0f, 0.0056f, 1.7f},
    {50.4742380f, 0.0000009f, 9.69f, 0.0086f, 0.0f, 0.0056f, 1.7f},     {50.9877480f, 0.0000025f, 8.89f, 0.0087f, 0.0f, 0.0055f, 1.7f},
    {51.5033500f, 0.0000061f, 7.74f, 0.0089f, 0.0f, 0.0056f, 1.8f},     {52.0214090f, 0.0000141f, 6.84f, 0.0092f, 0.0f, 0.0055f, 1.8f},
    {52.5423930f, 0.0000310f, 6.00f, 0.0094f, 0.0f, 0.0057f, 1.8f},     {53.0669060f, 0.0000641f, 5.22f, 0.0097f, 0.0f, 0.0053f, 1.9f},
    {53.5957480f, 0.0001247f, 4.48f, 0.0100f, 0.0f, 0.0054f, 1.8f},     {54.1299999f, 0.0002280f, 3.81f, 0.0102f, 0.0f, 0.0048f, 2.0f},
    {54.6711570f, 0.0003918f, 3.19f, 0.0105f, 0.0f, 0.0048f, 1.9f},     {55.2213650f, 0.0006316f, 2.62f, 0.01079f, 0.0f, 0.00417f, 2.1f},
    {55.7838000f, 0.0009535f, 2.115f, 0.0111f, 0.0f, 0.00375f, 2.1f},   {56.2647770f, 0.0005489f, 0.01f, 0.01646f, 0.0f, 0.00774f, 0.9f},
    {56.3378700f, 0.0013440f, 1.655f, 0.01144f, 0.0f, 0.00297f, 2.3f},  {56.9681000f, 0.0017630f, 1.255f, 0.01181f, 0.0f, 0.00212f, 2.5f},
    {57.6124810f, 0.0000213f, 0.91f, 0.01221f, 0.0f, 0.00094f, 3.7f},   {58.3238740f, 0.0000239f, 0.621f, 0.01266f, 0.0f, -0.00055f, -3.1f},
    {58.4465890f, 0.0000146f, 0.079f, 0.01449f, 0.0f, 0.00597f, 0.8f},  {59.1642040f, 0.0000240f, 0.386f, 0.01319f, 0.0f, -0.00244f, 0.1f},
    {59.5909820f, 0.0000211f, 0.207f, 0.0136f, 0.0f, 0.00344f, 0.5f},   {60.3060570f, 0.0000212f, 0.207f, 0.01382f, 0.0f, -0.00413f, 0.7f},
    {60.4347750f, 0.0000246f, 0.386f, 0.01297f, 0.0f, 0.00132f, -1.0f}, {61.1505580f, 0.0000250f, 0.621f, 0.01248f, 0.0f, -0.00036f, 5.8f},
    {61.8001520f, 0.0000230f, 0.91f, 0.01207f, 0.0f, -0.00159f, 2.9f},  {62.4112120f, 0.0000193f, 1.255f, 0.01171f, 0.0f, -0.00266f, 2.3f},
    {62.4862530f, 0.0000152f, 0.078f, 0.01468f, 0.0f, -0.00477f, 0.9f}, {62.9979740f, 0.0000150f, 1.66f, 0.01139f, 0.0f, -0.00334f, 2.2f},
    {63.5685150f, 0.0000109f, 2.11f, 0.01108f, 0.0f, -0.00417f, 2.0f},  {64.1277640f, 0.0007335f, 2.62f, 0.01078f, 0.0f, -0.00448f, 2.0f},
    {64.6789000f, 0.0004635f, 3.19f, 0.0105f, 0.0f, -0.0051f, 1.8f},    {65.2240670f, 0.0002748f, 3.81f, 0.0102f, 0.0f, -0.0051f, 1.9f},
    {65.7647690f, 0.0001530f, 4.48f, 0.0100f, 0.0f, -0.0057f, 1.8f},    {66.3020880f, 0.0000801f, 5.22f, 0.0097f, 0.0f, -0.0055f, 1.8f},
    {66.8368270f, 0.0000395f, 6.00f, 0.0094f, 0.0f, -0.0059f, 1.7f},    {67.3695950f, 0.0000183f, 6.84f, 0.0092f, 0.0f, -0.0056f, 1.8f},
    {67.9008620f, 0.0000080f, 7.74f, 0.0089f, 0.0f, -0.0058f, 1.7f},    {68.4310010f, 0.0000033f, 8.69f, 0.0087f, 0.0f, -0.0057f, 1.7f},
    {68.9603060f, 0.0000013f, 9.69f, 0.0086f, 0.0f, -0.0056f, 1.7f},    {69.4890210f, 0.0000005f, 10.72f, 0.0085f, 0.0f, -0.0056f, 1.7f},
    {70.0173420f, 0.0000002f, 11.83f, 0.0084f, 0.0f, -0.0056f, 1.7f},   {118.7503410f, 0.0000094f, 0.0f, 0.01592f, 0.0f, -0.00044f, 0.9f},
    {368.4983500f, 0.0000679f, 0.02f, 0.0192f, 0.6f, 0.0f, 1.0f},       {424.7631200f, 0.0006380f, 0.011f, 0.01916f, 0.6f, 0.0f, 1.0f},
    {487.2493700f, 0.0002350f, 0.011f, 0.0192f, 0.6f, 0.0f, 1.0f},      {715.3931500f, 0.0000996f, 0.089f, 0.0181f, 0.6f, 0.0f, 1.0f},
    {773.8387300f, 0.0006710f, 0.079f, 0.0181f, 0.6f, 0.0f, 1.0f},      {834.1453300f, 0.0001800f, 0.079f, 0.0181f, 0.6f, 0.0f, 1.0f}};
static __constant__ float RD_H2O[RD_NH2O][4] = {
    {22.2350800f, 0.109f, 2.143f, 0.02784f},   {67.8139600f, 0.0011f, 8.73f, 0.0276f},    {119.9959400f, 0.0007f, 8.347f, 0.027f},
    {183.3101170f, 2.3f, 0.653f, 0.02835f},    {321.2256440f, 0.0464f, 6.156f, 0.0214f},  {325.1529190f, 1.54f, 1.515f, 0.027f},
    {336.1870000f, 0.001f, 9.802f, 0.0265f},   {380.1973720f, 11.9f, 1.018f, 0.0276f},    {390.1345080f, 0.0044f, 7.318f, 0.019f},
    {437.3466670f, 0.0637f, 5.015f, 0.0137f},  {439.1508120f, 0.921f, 3.561f, 0.0164f},   {443.0182950f, 0.194f, 5.015f, 0.0144f},
    {448.0010750f, 10.6f, 1.37f, 0.0238f},     {470.8889740f, 0.33f, 3.561f, 0.0182f},    {474.6891270f, 1.28f, 2.342f, 0.0198f},
    {488.4911330f, 0.253f, 2.814f, 0.0249f},   {503.5685320f, 0.0374f, 6.693f, 0.0115f},  {504.4826920f, 0.0125f, 6.693f, 0.0119f},
    {556.9360020f, 510.0f, 0.114f, 0.03f},     {620.7008070f, 5.09f, 2.15f, 0.0223f},     {658.0065000f, 0.274f, 7.767f, 0.03f},
    {752.0332270f, 250.0f, 0.336f, 0.0286f},   {841.0735950f, 0.013f, 8.113f, 0.0141f},   {859.8650000f, 0.133f, 7.989f, 0.0286f},
    {899.4070000f, 0.055f, 7.845f, 0.0286f},   {902.5550000f, 0.038f, 8.36f, 0.0264f},    {906.2055240f, 0.183f, 5.039f, 0.0234f},
    {916.1715820f, 8.56f, 1.369f, 0.0253f},    {970.3150220f, 9.16f, 1.842f, 0.024f},     {987.9267640f, 138.0f, 0.178f, 0.0286f}};

// the Van Vleck-Weisskopf shape both line sums share (fpp_o2, fpp_h2o: gases.f90:152-170); delt = 0 for water vapour
GR_DEV double rd_fpp(double gm, double delt, double f, double v0)
{
    const double x = (v0 - f) * (v0 - f) + gm * gm, y = (v0 + f) * (v0 + f) + gm * gm;
    return ((1. / x) + (1. / y)) * (gm * f / v0) - (delt * f / v0) * (((v0 - f) / x) - ((v0 + f) / x));
}

// gases.f90:112-146: PRES_mb hPa, T K, RH %, f GHz -> dB/km two-way.  Every literal is the reference's default-real constant, widened.
GR_DEV double rd_gases(double pres_mb, double t, double rh, double f)
{
    const double th = (double)300.f / t, th2 = th * th, th3 = th2 * th, th5 = (th2 * th2) * th;
    const double e = (rh * th5) / ((double)41.45f * pow(10.0, (double)9.834f * th - 10.0));
    const double p = pres_mb / (double)10.f - e;
    const double one_th = 1.0 - th, th08 = pow(th, (double)0.8f), th25 = pow(th, (double)2.5f);
    double sumo = 0.;
    for (int i = 0; i < RD_NO2; i++) {
        const double v0 = RD_O2[i][0], a1 = RD_O2[i][1], a2 = RD_O2[i][2], a3 = RD_O2[i][3], a4 = RD_O2[i][4], a5 = RD_O2[i][5], a6 = RD_O2[i][6];
        // a4 is 0 but for the last six lines, and those have a5 = 0: every lane of the wave takes the same side
        const double gm = a3 * (p * (a4 == 0. ? th08 : pow(th, (double)0.8f - a4)) + (double)1.1f * e * th);
        const double delt = a5 == 0. ? a5 * p : a5 * p * pow(th, a6);
        sumo = sumo + rd_fpp(gm, delt, f, v0) * (a1 * p * th3 * exp(a2 * one_th));
    }
    const double term1 = sumo;
    const double gm0 = (double)5.6E-3f * (p + (double)1.1f * e) * th08;
    const double a0 = (double)3.07E-4f;
    const double ap = (double)1.4f * (1 - (double)1.2f * pow(f, (double)1.5f) * (double)1E-5f) * (double)1E-10f;
    const double term2 = (2 * a0 * (1.0 / (gm0 * (1 + (f / gm0) * (f / gm0)) * (1 + (f / (double)60.f) * (f / (double)60.f)))) + ap * p * th25) * f * p * th2;
    sumo = 0.;
    const double th35 = pow(th, (double)3.5f);
    for (int i = 0; i < RD_NH2O; i++) {
        const double v1 = RD_H2O[i][0], b1 = RD_H2O[i][1], b2 = RD_H2O[i][2], b3 = RD_H2O[i][3];
        const double gm = b3 * (p * th08 + (double)4.8f * e * th);
        sumo = sumo + rd_fpp(gm, 0., f, v1) * (b1 * e * th35 * exp(b2 * one_th));
    }
    const double term3 = sumo;
    const double term4 = ((double)1.4E-6f * p + (double)5.41E-5f * e * th3) * f * e * th25;
    const double npp = term1 + term2 + term3 + term4;
    return (double)0.182f * f * npp;
}

template <typename R> struct GasArgs {
    int npoints, nlev, surface_radar;
    double freq;
    const R *p, *t, *rh, *zlev;        // (npoints,nlev), level 1 the top
    double *g, *x, *ca, *cb, *cc;      // workspace, (npoints,ngate), the radar's first gate first: g_vol, the height in km, the parabola of a gate
    double *g_vol, *g_to_vol;          // (npoints,nlev) in level order, either may be null
    uint32_t *err;
};
// gate k (from 0, the radar's first) of level l and back: order_data, format_input.f90:66-130
template <typename R> GR_DEV int rd_gate(const GasArgs<R> &A, int l) { return A.surface_radar ? A.nlev - 1 - l : l; }

// cosp_radar.F90:136-139 and radar_simulator.f90:478-479; grid (points, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_radar_gases(const GasArgs<R> A)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
    if (j >= A.npoints) return;
    const size_t np = (size_t)A.npoints, o = (size_t)l * np + j;
    double p_mb, t_c, hgt;
    unsigned bad = 0;
    {
#pragma clang fp contract(off)
        const R p = A.p[o], t = A.t[o];
        bad = (p > (R)0 ? 0u : 1u << RDERR_P) | (t > (R)0 ? 0u : 1u << RDERR_T);
        p_mb = (double)(p / (R)100.0);          // From Pa to hPa, in the real kind
        t_c = (double)(t - (R)273.15);          // From K to C
        const R h = A.zlev[o] / (R)1000.0;      // From m to km
        hgt = (double)h;
        // strictly decreasing with the level, still so in km: the abscissas AVINT needs
        if (l + 1 < A.nlev && !(h > A.zlev[o + np] / (R)1000.0)) bad |= 1u << RDERR_ZLEV;
    }
    if (bad) atomicOr(A.err, bad);
    const double g = rd_gases(p_mb, t_c + (double)273.15f, (double)A.rh[o], A.freq);
    const size_t og = (size_t)rd_gate(A, l) * np + j;
    A.g[og] = g;
    A.x[og] = hgt;
    if (A.g_vol) A.g_vol[o] = g;
}

// avint's overlapping parabola through a gate and its two neighbours (math_lib.f90:337-351), the abscissas ascending; grid (points, gates),
// the first and the last gate have none
template <typename R>
__global__ void __launch_bounds__(256) k_radar_gas_parab(const GasArgs<R> A)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y + 1;
    if (j >= A.npoints || k + 1 >= A.nlev) return;
    const size_t np = (size_t)A.npoints, o = (size_t)k * np + j;
    const size_t lo = A.surface_radar ? o - np : o + np, hi = A.surface_radar ? o + np : o - np;      // a spaceborne radar's gates descend
    const double x1 = A.x[lo], x2 = A.x[o], x3 = A.x[hi];
    const double term1 = A.g[lo] / ((x1 - x2) * (x1 - x3));
    const double term2 = A.g[o] / ((x2 - x1) * (x2 - x3));
    const double term3 = A.g[hi] / ((x3 - x1) * (x3 - x2));
    A.ca[o] = term1 + term2 + term3;
    A.cb[o] = -(x2 + x3) * term1 - (x1 + x3) * term2 - (x1 + x2) * term3;
    A.cc[o] = x2 * x3 * term1 + x1 * x3 * term2 + x1 * x2 * term3;
}

// g_to_vol(k) = path_integral(g_vol, hgt, 1, k-1), radar_simulator.f90:480; grid (points, gates).  n = k - 1 points lie before the gate.
// n <= 3: math_lib.f90:145-150.  n > 3: avint from the lowest to the highest of them (:285-379): with a = xtab(1) and b = xtab(ntab) its
// brackets are ilo = 2 and ihi = ntab - 2, so ascending index i runs 2 .. n - 2 and the last parabola also covers [x(n-2), x(n)].
// Ascending index i is gate i of a surface radar and gate n + 1 - i of a spaceborne one (both from 1).
template <typename R>
__global__ void __launch_bounds__(256) k_radar_gas_path(const GasArgs<R> A)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (j >= A.npoints || !A.g_to_vol) return;
    const size_t np = (size_t)A.npoints;
    const int l = A.surface_radar ? A.nlev - 1 - n : n;
    double res = 0.;
    if (n > 0 && n <= 3) {
        const double deltah = fabs(A.x[np + j] - A.x[j]);
        for (int k = 0; k < n; k++) res = res + A.g[(size_t)k * np + j] * deltah;
    } else if (n > 3) {
        auto at = [&](int i) { return (size_t)(A.surface_radar ? i - 1 : n - i) * np + j; };      // ascending index from 1 -> gate from 0
        double syl = A.x[at(1)], sum1 = 0., ca = 0., cb = 0., cc = 0.;
        for (int i = 2; i <= n - 2; i++) {
            const size_t o = at(i);
            const double x2 = A.x[o], atemp = A.ca[o], btemp = A.cb[o], ctemp = A.cc[o];
            if (i <= 2) { ca = atemp; cb = btemp; cc = ctemp; }
            else { ca = 0.5 * (atemp + ca); cb = 0.5 * (btemp + cb); cc = 0.5 * (ctemp + cc); }
            sum1 = sum1 + ca * (x2 * x2 * x2 - syl * syl * syl) / 3.0 + cb * 0.5 * (x2 * x2 - syl * syl) + cc * (x2 - syl);
            ca = atemp; cb = btemp; cc = ctemp;
            syl = x2;
        }
        const double b = A.x[at(n)];
        res = sum1 + ca * (b * b * b - syl * syl * syl) / 3.0 + cb * 0.5 * (b * b - syl * syl) + cc * (b - syl);
    }
    A.g_to_vol[(size_t)l * np + j] = res;
}

}  // namespace geosrad
