// gridcomp_kernels.hpp -- the data path of the GridComp drivers either side of the RRTMG solvers,
// as HBM-streaming kernels (gfx950):
//   k_lwd_prep / k_lwd_zm / k_lwd_post   the RRTMG branch of LW_Driver (GEOSirrad_GridComp/GEOS_IrradGridComp.F90:3188-3372 and
//                                        :3487-3533, :3601-3615): unit conversions, level temperatures, effective-radius limits,
//                                        absorption aerosol optical depth, vertical flip; after the solver: flip back, sign
//                                        conventions, SFCEM, net fluxes, super-layer cloud fractions
//   k_swd_prep / k_swd_zm / k_swd_post   the same for SORADCORE's RRTMG branch (GEOSsolar_GridComp/GEOS_SolarGridComp.F90:6113-6219,
//                                        :6395-6454)
//   k_swd_prep<R, true> / k_swc_prep<R, true> / k_swd_post_lit / k_lit_scatter
//                                        the same on the un-packed tile: PackIt (SOL:3839-3894) inside the prep kernels, UnPackIt with
//                                        its DEFAULT (SOL:6520-6580) inside the post kernel and one scatter over the remaining results
//   k_lw_update_flx                      Update_Flx (IRR:3861-3999): the heartbeat linearisation of the LW fluxes in the surface
//                                        temperature, every model step between two full calculations
//   k_sw_update_export                   the 3-D / TOA / surface flux part of UPDATE_EXPORT (SOL:7540-7579): normalised fluxes x SLR
//   k_sw_update_obio                     the SOLAR TO OBIO band conversion of UPDATE_EXPORT (SOL:7584-7737): DRBANDN / DFBANDN -> DROBIO / DFOBIO
//   k_rad_tendencies                     the parent's heating rates (GEOS_RadiationGridComp.F90:798-819)
// GEOS fields are (IM,JM,levels): column index fastest, which is the [level][column] layout of every kernel here (lane = column,
// blockIdx.y = level): all accesses are coalesced, nothing is transposed, the vertical flip is an index calculation.
// A null output pointer = Fortran "not associated" (export not requested).
#pragma once
#include <iterator>
#include <type_traits>
#include "../../include/geosrad.h"
#include "lw_device.hpp"
#include "chou_kernels.hpp"
#include "sorad_kernels.hpp"     // SoradDev: the Chou-Suarez SW tables; so_cld_tau, so_cld_index, so_caif_scale; gr_log10 (lw_kernels.hpp)
#include "obio_bands.hpp"        // NB_OBIO, OBIO_MAXBANDS, OBIO_MAXPAIRS

namespace geosrad {

// ---------------------------------------------------------------------------------------------------------------------------
// Host only: where slot k of an entry point's public `in[]` / `out[]` pointer table (the GEOSRAD_*_* enums of geosrad.h) goes in the argument
// struct S of a kernel.  Next to each such struct stands Fields<S> (or a named variant) with one table per direction in the enum's order: a
// pointer to member, elem<&S::array, k> for an element of an array member, {} where S has no member for the slot.  bind() fills a struct from
// the caller's tables; a new field is one member, one enum value and one entry here.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename S, typename R> struct Slot {
    const R *S::*rd = nullptr;
    R *S::*wr = nullptr;
    void (*el)(S &, R *) = nullptr;
    constexpr Slot() {}
    constexpr Slot(const R *S::*m) : rd(m) {}
    constexpr Slot(R *S::*m) : wr(m) {}
    constexpr Slot(void (*f)(S &, R *)) : el(f) {}
    // a member that is written (an export, or an in-out import such as SwdArgs::taua from `in[]`) takes the pointer with its const cast away
    void set(S &s, const void *p) const { if (rd) s.*rd = (const R *)p; else if (wr) s.*wr = (R *)p; else if (el) el(s, (R *)p); }
};
template <auto A, int K, typename S, typename R> void elem(S &s, R *p) { (s.*A)[K] = p; }
template <typename S> struct Fields;
#define GR_TABLE(dir, N, ...) static constexpr Slot<S, R> dir[] = {__VA_ARGS__}; static_assert(std::size(dir) == N, "one entry for each of the " #N " slots")
template <typename F, typename S> void bind_in(S &s, const void *const *in) { int k = 0; for (const auto &f : F::in) f.set(s, in[k++]); }
template <typename F, typename S> void bind_out(S &s, void *const *out) { int k = 0; for (const auto &f : F::out) f.set(s, out[k++]); }
template <typename S> void bind(S &s, const void *const *in, void *const *out) { bind_in<Fields<S>>(s, in); bind_out<Fields<S>>(s, out); }

// the un-packed tile of the lit-aware SW drivers (geosrad_sw_driver_*_lit_dev): its columns, geosrad_lit_index_dev's two index arrays
// (device), UnPackIt's DEFAULT of every output (host) and the outputs whose dark columns keep their values
struct LitTile { int tile; const int32_t *idx, *pos; const double *dark; uint64_t keep; };
inline const char *lit_check(const LitTile &t, int nlit, void *const *out, int nout)      // what is wrong with the tile's description, or null
{
    if (nlit < 0 || nlit > t.tile) return "nlit must lie in 0 .. ncol";
    if (nlit > 0 && (!t.idx || !t.pos)) return "lit_index / lit_pos null";
    bool fill = false;
    for (int k = 0; k < nout; k++) fill = fill || (out[k] && !(t.keep >> k & 1));
    return fill && (!t.pos || !t.dark) ? "an output whose keep bit is clear needs lit_pos and dark" : nullptr;
}
// One output of an SW driver on a tile, in its out[] enum's order: its rows (0: lm + 1) and where its packed result is: slot `at` of the post kernel
// of the aerosol (POST) or no-aerosol pass (POST_NA), which un-packs it itself, or plane `at` of the driver's workspace, which k_lit_scatter un-packs.
enum TileSrc { POST, POST_NA, PLANE };
struct TileOut { int rows; TileSrc src; int at; int nrows(int lm) const { return rows ? rows : lm + 1; } };

// ---------------------------------------------------------------------------------------------------------------------------
// LW_Driver, RRTMG branch
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct LwdArgs {
    int ncol, lm, nb;                 // columns (IM*JM), layers, aerosol bands of TAUA/SSAA (16)
    int iceflg, liqflg;
    // GEOS side, model ordering (k = 1 top .. LM bottom); ple has LM+1 levels (0..LM)
    const R *ple, *pl, *t, *q, *o3, *ch4, *n2o, *co2_3d, *cfc11, *cfc12, *hcfc22, *fcld;
    const R *cwc_liq, *cwc_ice, *reff_liq, *reff_ice;      // CWC(:,:,:,KLIQUID|KICE), REFF(...)
    const R *taua, *ssaa;                                  // (IM,JM,LM,nb) or null
    const R *ts, *emis, *lats, *t2m;
    R co2_fixed, o2, ccl4, airmw_over_h2omw, airmw_over_o3mw, rgas, grav;
    // RRTMG side, 1 = bottom layer; [K][ncol]
    R *play, *plev, *tlay, *tlev, *tsfc, *emis_r, *h2o, *o3_r, *co2_r, *ch4_r, *n2o_r, *o2_r, *cfc11_r, *cfc12_r, *cfc22_r, *ccl4_r,
        *cldf, *ciwp, *clwp, *rei, *rel, *tauaer, *zm, *alat;
};

template <typename R> struct Fields<LwdArgs<R>> { using S = LwdArgs<R>;
    GR_TABLE(in, GEOSRAD_LWD_NIN, &S::ple, &S::pl, &S::t, &S::q, &S::o3, &S::ch4, &S::n2o, &S::co2_3d, &S::cfc11, &S::cfc12, &S::hcfc22, &S::fcld, &S::cwc_liq,
             &S::cwc_ice, &S::reff_liq, &S::reff_ice, &S::taua, &S::ssaa, &S::ts, &S::emis, &S::lats, &S::t2m);
};
// geosrad_lw_driver_rrtmg*_dev, as geosrad.h has it (nrats == 0 without the RATS diagnostics, na_out null without the aerosol-free INTERNALs)
struct LwdCall {
    int ncol, lm, nb; const void *const *in; const double *consts; int iceflg, liqflg, doy, lcldlm, lcldmh; const int32_t *band_output; void *const *out;
    int nrats; const int32_t *rat_gas; void *const *rat_out;
    void *const *na_out;
};
// interface temperature of model level k (1..LM+1), IRR:3248-3256
template <typename R> GR_DEV R lwd_tlev(const LwdArgs<R> &A, int k, int ij)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int n = A.ncol, lm = A.lm;
    if (k == lm + 1) return A.t2m[ij];
    if (k == 1) k = 2;
    auto PLE = [&](int l) { return A.ple[(size_t)l * n + ij]; };
    auto T = [&](int l) { return A.t[(size_t)(l - 1) * n + ij]; };
    const R dpk = PLE(k) - PLE(k - 1), dpm = PLE(k - 1) - PLE(k - 2);
    return (T(k - 1) * dpk + T(k) * dpm) / (dpm + dpk);
}

template <typename R> GR_DEV R clampr(R x, R lo, R hi) { x = x > lo ? x : lo; return x < hi ? x : hi; }      // min(max(x,lo),hi)

// effective-radius limits RRTMG assumes (IRR:3272-3291, SOL:6144-6170)
template <typename R> GR_DEV void rrtmg_reff_limits(int iceflg, int liqflg, R &reice, R &reliq)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    if (liqflg == 0) reliq = clampr<R>(reliq, (R)5.0, (R)10.0);
    else if (liqflg == 1) reliq = clampr<R>(reliq, (R)2.5, (R)60.0);
    if (iceflg == 0) reice = clampr<R>(reice, (R)10.0, (R)30.0);
    else if (iceflg == 1) reice = clampr<R>(reice, (R)13.0, (R)130.0);
    else if (iceflg == 2) reice = clampr<R>(reice, (R)5.0, (R)131.0);
    else if (iceflg == 3) reice = clampr<R>(reice, (R)5.0, (R)140.0);
    else if (iceflg == 4) reice = clampr<R>(reice * (R)2., (R)1.0, (R)200.0);
}

// one thread per (column, RRTMG layer K = 1..LM); blockIdx.y = K - 1, and K = LM additionally writes the top level
template <typename R> __global__ void __launch_bounds__(256) k_lwd_prep(LwdArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= A.ncol) return;
    const int n = A.ncol, lm = A.lm, K = blockIdx.y + 1, LV = lm - K + 1;
    const size_t o = (size_t)(K - 1) * n + ij;          // RRTMG layer K
    const size_t g = (size_t)(LV - 1) * n + ij;         // GEOS layer LV
    const R pleb = A.ple[(size_t)LV * n + ij], plet = A.ple[(size_t)(LV - 1) * n + ij];
    const R dp = pleb - plet;
    // content [kg/kg] -> path [g/m2]: 1000*dp/g ~ 1.02*100*dp (IRR:3262-3267)
    const R xx = (R)1.02 * (R)100 * dp;
    A.clwp[o] = xx * A.cwc_liq[g];
    A.ciwp[o] = xx * A.cwc_ice[g];
    R reliq = A.reff_liq[g], reice = A.reff_ice[g];
    rrtmg_reff_limits<R>(A.iceflg, A.liqflg, reice, reliq);
    A.rel[o] = reliq; A.rei[o] = reice;
    // levels: PLE_R(0:LM) = PLE(LM:0)/100, TLEV_R(0:LM) = TLEV(LM+1:1) (IRR:3293-3299, :3340-3342)
    A.plev[o] = pleb / (R)100.;
    A.tlev[o] = lwd_tlev<R>(A, LV + 1, ij);
    if (K == lm) {
        A.plev[(size_t)lm * n + ij] = A.ple[ij] / (R)100.;
        A.tlev[(size_t)lm * n + ij] = lwd_tlev<R>(A, 1, ij);
    }
    // layers (IRR:3301-3322) with the clean-up of negatives (IRR:3361-3371)
    auto pos = [](R x) { return x < 0 ? (R)0 : x; };
    A.play[o] = A.pl[g] / (R)100.;
    A.tlay[o] = A.t[g];
    const R q = A.q[g];
    A.h2o[o] = pos(q / ((R)1. - q) * A.airmw_over_h2omw);
    A.o3_r[o] = pos(A.o3[g] * A.airmw_over_o3mw);
    A.ch4_r[o] = pos(A.ch4[g]);
    A.n2o_r[o] = pos(A.n2o[g]);
    A.co2_r[o] = pos(A.co2_3d ? A.co2_3d[g] : A.co2_fixed);
    A.o2_r[o] = pos(A.o2);
    A.ccl4_r[o] = pos(A.ccl4);
    A.cfc11_r[o] = pos(A.cfc11[g]);
    A.cfc12_r[o] = pos(A.cfc12[g]);
    A.cfc22_r[o] = pos(A.hcfc22[g]);
    A.cldf[o] = pos(A.fcld[g]);
    // absorption aerosol optical thickness (IRR:3324-3335); tauaer is (ncol,nlay,16)
    for (int b = 0; b < 16; b++) {
        R v = 0;
        if (A.taua && b < A.nb) {
            const size_t ga = ((size_t)b * lm + (LV - 1)) * n + ij;
            v = A.taua[ga] - A.ssaa[ga];
            v = v > 0 ? v : (R)0;
        }
        A.tauaer[((size_t)b * lm + (K - 1)) * n + ij] = v;
    }
    if (K == 1) {
        A.tsfc[ij] = A.ts[ij];
        A.alat[ij] = A.lats[ij];
        const R e = A.emis[ij];
        for (int b = 0; b < 16; b++) A.emis_r[(size_t)b * n + ij] = e;      // all bands get the same emissivity (IRR:3244)
    }
}

// layer mid-point heights, a running sum up the column (IRR:3344-3356): one thread per column
template <typename R> __global__ void __launch_bounds__(256) k_lwd_zm(LwdArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= A.ncol) return;
    const int n = A.ncol, lm = A.lm;
    R z = 0;
    A.zm[ij] = 0;
    R plm = A.play[ij];
    for (int K = 2; K <= lm; K++) {
        const R plk = A.play[(size_t)(K - 1) * n + ij];
        // dz ~ RT/g x dp/p; the jump from LAYER K-1 to K is centred on LEVEL K-1 (0-based levels)
        z = z + A.rgas * A.tlev[(size_t)(K - 1) * n + ij] / A.grav * (plm - plk) / A.plev[(size_t)(K - 1) * n + ij];
        A.zm[(size_t)(K - 1) * n + ij] = z;
        plm = plk;
    }
}

template <typename R> struct LwdPost {
    int ncol, lm, ngpt;
    const R *uflx, *dflx, *uflxc, *dflxc, *duflx, *duflxc;      // RRTMG (ncol, LM+1), 1 = surface
    const int32_t *clearCounts;                                 // (ncol,4)
    const R *emis, *ts;
    // GEOS internal state (IM,JM,0:LM); any may be null
    R *flxu_int, *flxd_int, *flcu_int, *flcd_int, *dfdts, *dfdtsc, *dfdtsna, *dfdtscna, *flx_int, *flc_int;
    R *sfcem_int, *ts_int, *cldttlw, *cldhilw, *cldmdlw, *cldlolw;
};

template <typename R> struct Fields<LwdPost<R>> { using S = LwdPost<R>;      // OLRB, DOLRB are the solver's own
    GR_TABLE(out, GEOSRAD_LWD_NOUT, &S::flxu_int, &S::flxd_int, &S::flcu_int, &S::flcd_int, &S::dfdts, &S::dfdtsc, &S::dfdtsna, &S::dfdtscna, &S::flx_int,
             &S::flc_int, &S::sfcem_int, &S::ts_int, &S::cldttlw, &S::cldhilw, &S::cldmdlw, &S::cldlolw, {}, {});
};
// one thread per (column, GEOS level K = 0..LM) (IRR:3487-3533, :3601-3615, :3560-3565)
template <typename R> __global__ void __launch_bounds__(256) k_lwd_post(LwdPost<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    const int n = P.ncol, lm = P.lm, K = blockIdx.y, LV = lm - K + 1;
    const size_t s = (size_t)(LV - 1) * n + ij, o = (size_t)K * n + ij;
    // upward negative in the GEOS convention
    const R fu = -P.uflx[s], fd = P.dflx[s], cu = -P.uflxc[s], cd = P.dflxc[s], du = -P.duflx[s], dc = -P.duflxc[s];
    if (P.flxu_int) P.flxu_int[o] = fu;
    if (P.flxd_int) P.flxd_int[o] = fd;
    if (P.flcu_int) P.flcu_int[o] = cu;
    if (P.flcd_int) P.flcd_int[o] = cd;
    if (P.dfdts) P.dfdts[o] = du;
    if (P.dfdtsc) P.dfdtsc[o] = dc;
    if (P.dfdtsna) P.dfdtsna[o] = du;        // RRTMG has no no-aerosol derivatives (IRR:3560-3565)
    if (P.dfdtscna) P.dfdtscna[o] = dc;
    if (P.flx_int) P.flx_int[o] = fd + fu;   // net downward (IRR:3601-3604)
    if (P.flc_int) P.flc_int[o] = cd + cu;
    if (K == lm) {
        // surface emitted: reflected LW is not counted; first negative (Chou-Suarez convention), then reverted (IRR:3512, :3608)
        R sf = -(P.uflx[ij] - P.dflx[ij] * ((R)1. - P.emis[ij]));
        sf = -sf;
        if (P.sfcem_int) P.sfcem_int[ij] = sf;
        if (P.ts_int) P.ts_int[ij] = P.ts[ij];
        const R ng = (R)P.ngpt;
        if (P.cldttlw) P.cldttlw[ij] = (R)1.0 - (R)P.clearCounts[(size_t)0 * n + ij] / ng;
        if (P.cldhilw) P.cldhilw[ij] = (R)1.0 - (R)P.clearCounts[(size_t)1 * n + ij] / ng;
        if (P.cldmdlw) P.cldmdlw[ij] = (R)1.0 - (R)P.clearCounts[(size_t)2 * n + ij] / ng;
        if (P.cldlolw) P.cldlolw[ij] = (R)1.0 - (R)P.clearCounts[(size_t)3 * n + ij] / ng;
    }
}

// Aerosol-free share of the un-flip, with the conventions the reference's other two branches have for these INTERNALs (IRR:3506-3515 signs,
// :3604-3607 net fluxes): one thread per (column, GEOS level K = 0..LM).  DFDTSNA / DFDTSCNA are the aerosol-free pass's own derivatives.
template <typename R> struct LwdPostNa {
    int ncol, lm;
    const R *uflx, *dflx, *uflxc, *dflxc, *duflx, *duflxc;      // RRTMG without aerosols (ncol, LM+1), 1 = surface
    R *flxau_int, *flxad_int, *flau_int, *flad_int, *flxa_int, *fla_int, *dfdtsna, *dfdtscna;      // (IM,JM,0:LM); any may be null
};
template <typename R> struct Fields<LwdPostNa<R>> { using S = LwdPostNa<R>;
    GR_TABLE(out, GEOSRAD_LWNA_NOUT, &S::flxau_int, &S::flxad_int, &S::flau_int, &S::flad_int, &S::flxa_int, &S::fla_int, &S::dfdtsna, &S::dfdtscna);
};
template <typename R> __global__ void __launch_bounds__(256) k_lwd_post_na(LwdPostNa<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    const int n = P.ncol, lm = P.lm, K = blockIdx.y, LV = lm - K + 1;
    const size_t s = (size_t)(LV - 1) * n + ij, o = (size_t)K * n + ij;
    const R fu = -P.uflx[s], fd = P.dflx[s], cu = -P.uflxc[s], cd = P.dflxc[s];
    if (P.flxau_int) P.flxau_int[o] = fu;
    if (P.flxad_int) P.flxad_int[o] = fd;
    if (P.flau_int) P.flau_int[o] = cu;
    if (P.flad_int) P.flad_int[o] = cd;
    if (P.flxa_int) P.flxa_int[o] = fd + fu;
    if (P.fla_int) P.fla_int[o] = cd + cu;
    if (P.dfdtsna) P.dfdtsna[o] = -P.duflx[s];
    if (P.dfdtscna) P.dfdtscna[o] = -P.duflxc[s];
}

// RATS share of the un-flip (IRR:3522-3530) and of the net fluxes (IRR:3614): one thread per (column, GEOS level K, gas)
template <typename R> struct LwdRatPost {
    int ncol, lm, nrats;
    const R *uflx, *dflx, *duflx;               // RRTMG (ncol, LM+1, nrats), 1 = surface
    const R *emis;                              // EMIS(I,J) = EMISS(IJ,1): all bands share it (IRR:3249)
    R *flxu_rat, *flxd_rat, *flx_rat, *dfdts_rat, *sfcem_rat;     // (ncol,0:LM,nrats), SFCEM_RAT (ncol,nrats); any may be null
};
template <typename R> struct Fields<LwdRatPost<R>> { using S = LwdRatPost<R>;
    GR_TABLE(out, GEOSRAD_LWD_NRATOUT, &S::flxu_rat, &S::flxd_rat, &S::flx_rat, &S::dfdts_rat, &S::sfcem_rat);
};
template <typename R> __global__ void __launch_bounds__(256) k_lwd_rat_post(LwdRatPost<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    const int n = P.ncol, lm = P.lm, K = blockIdx.y, r = blockIdx.z, LV = lm - K + 1;
    const size_t plane = (size_t)(lm + 1) * n * r;
    const size_t s = plane + (size_t)(LV - 1) * n + ij, o = plane + (size_t)K * n + ij;
    const R fu = -P.uflx[s], fd = P.dflx[s];
    if (P.flxu_rat) P.flxu_rat[o] = fu;
    if (P.flxd_rat) P.flxd_rat[o] = fd;
    if (P.dfdts_rat) P.dfdts_rat[o] = -P.duflx[s];
    if (P.flx_rat) P.flx_rat[o] = fd + fu;
    if (K == lm && P.sfcem_rat) P.sfcem_rat[(size_t)r * n + ij] = P.uflx[plane + ij] - P.dflx[plane + ij] * ((R)1.0 - P.emis[ij]);
}

// RATS exports of Update_Flx (IRR:4036-4120): one thread per (column, level K = 0..LM, gas)
template <typename R> struct LwRatUpd {
    int ncol, lm, nrats;
    const R *flx_int, *sfcem_int, *dfdts;                 // (ncol,0:LM), (ncol), (ncol,0:LM)
    const R *flx_rat, *sfcem_rat, *dfdts_rat;             // (ncol,0:LM,nrats), (ncol,nrats), (ncol,0:LM,nrats)
    R *dolr, *dlws, *dflns, *dsfcem, *nettrap;            // (ncol,nrats)
    R *coltrap;                                           // (ncol,LM,nrats)
    R *flx, *dfdts_out;                                   // (ncol,0:LM,nrats)
};
template <typename R> struct Fields<LwRatUpd<R>> { using S = LwRatUpd<R>;
    GR_TABLE(in, GEOSRAD_LWR_NIN, &S::flx_int, &S::sfcem_int, &S::dfdts, &S::flx_rat, &S::sfcem_rat, &S::dfdts_rat);
    GR_TABLE(out, GEOSRAD_LWR_NOUT, &S::dolr, &S::dlws, &S::dflns, &S::dsfcem, &S::nettrap, &S::coltrap, &S::flx, &S::dfdts_out);
};
template <typename R> __global__ void __launch_bounds__(256) k_lw_update_rats(LwRatUpd<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    const int n = P.ncol, lm = P.lm, K = blockIdx.y, r = blockIdx.z;
    const size_t pl = (size_t)(lm + 1) * n * r, o = (size_t)K * n + ij;
    const R f = P.flx_int[o], fr = P.flx_rat[pl + o];
    if (P.flx) P.flx[pl + o] = f - fr;
    if (P.dfdts_out) P.dfdts_out[pl + o] = P.dfdts[o] - P.dfdts_rat[pl + o];
    if (K >= 1 && P.coltrap) {
        R t = f - P.flx_int[o - n];
        t = t - (fr - P.flx_rat[pl + o - n]);
        P.coltrap[(size_t)lm * n * r + (size_t)(K - 1) * n + ij] = t;
    }
    if (K == lm) {
        const size_t q = (size_t)r * n + ij;
        const R f0 = P.flx_int[ij], fr0 = P.flx_rat[pl + ij], se = P.sfcem_int[ij], ser = P.sfcem_rat[q];
        if (P.dolr) { const R a = -(fr0); P.dolr[q] = (-(f0)) - a; }
        if (P.dlws) P.dlws[q] = (f + se) - (fr + ser);
        if (P.dflns) P.dflns[q] = f - fr;
        if (P.dsfcem) P.dsfcem[q] = se - ser;
        if (P.nettrap) { R t = f - f0; t = t - (fr - fr0); P.nettrap[q] = t; }
    }
}

// band OLR and brightness temperature of Update_Flx (IRR:3993-4021, Tbr_from_band_flux :4132-4186, invert_Planck_for_T :4188-4208):
// one thread per (column, band).  PASS 0 writes the updated band flux and records whether any column of the band is non-zero
// (the reference tests `all(Fband_ == 0.0)` on the whole field); PASS 1 inverts the Planck function.
template <typename R> struct LwBandUpd {
    int ncol;
    int band_output[16];
    R wn1[16], wn2[16];                 // [m-1], in the caller's real kind like wavenum1(ibnd)*100.
    R undef;
    const R *tsinst, *ts_int, *olrb_int, *dolrb_int;      // (ncol), (ncol), (16,ncol), (16,ncol)
    R *olrb_exp, *tbrb_exp;             // (ncol,16); either may be null
    int *nonzero;                       // [16]
};
template <typename R, int PASS> __global__ void __launch_bounds__(256) k_lw_update_bands(LwBandUpd<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x, ib = blockIdx.y;
    if (ij >= P.ncol || !P.band_output[ib]) return;
    const R delt = P.tsinst[ij] - P.ts_int[ij];
    const R f = P.olrb_int[(size_t)ij * 16 + ib] + P.dolrb_int[(size_t)ij * 16 + ib] * delt;
    const size_t o = (size_t)ib * P.ncol + ij;
    if (PASS == 0) {
        if (P.olrb_exp) P.olrb_exp[o] = f;
        if (f != (R)0) P.nonzero[ib] = 1;           // every writer writes 1
    } else {
        if (!P.nonzero[ib]) { P.tbrb_exp[o] = P.undef; return; }
        const double h = 6.626070040e-34, c = 2.99792458e8, kB = 1.38064852e-23, pi = 3.14159265358979323846;
        const double alT = h * c / kB, bigC = 2.0 * h * (c * c);
        const double Fband = (double)f;
        const double Bmean = Fband / (pi * (double)(P.wn2[ib] - P.wn1[ib]));
        const R wnMid = (R)((double)(P.wn1[ib] + P.wn2[ib]) / 2.0);
        const R wn3 = (wnMid * wnMid) * wnMid;       // wn**3 in the real kind of wn
        const double T = alT * (double)wnMid / log(bigC * (double)wn3 / Bmean + 1.0);
        P.tbrb_exp[o] = (R)T;
    }
}

// Chou-Suarez branch of LW_Driver: `irrad` takes the GEOS fields as they are (no flip, no unit conversion) and fills the INTERNAL
// fluxes itself; what the driver adds (IRR:2101-2108, :3601-3616): the derivatives irrad does not provide, the net fluxes of the four
// flavours, the sign of SFCEM, TS_INT.
template <typename R> struct LwcPost {
    int ncol, lm;
    const R *flxu, *flcu, *flau, *flxau, *flxd, *flcd, *flad, *flxad, *dfdts, *ts;
    R *sfcem_int;                                                         // in: as irrad leaves it (negative); out: positive
    R *flx_int, *flxa_int, *flc_int, *fla_int, *dfdtsc, *dfdtsna, *dfdtscna, *ts_int;
};
template <typename R> struct Fields<LwcPost<R>> { using S = LwcPost<R>;
    GR_TABLE(in, GEOSRAD_LWC_NIN, &S::flxu, &S::flcu, &S::flau, &S::flxau, &S::flxd, &S::flcd, &S::flad, &S::flxad, &S::dfdts, &S::ts);
    GR_TABLE(out, GEOSRAD_LWC_NOUT, &S::sfcem_int, &S::flx_int, &S::flxa_int, &S::flc_int, &S::fla_int, &S::dfdtsc, &S::dfdtsna, &S::dfdtscna, &S::ts_int);
};
template <typename R> __global__ void __launch_bounds__(256) k_lwd_chou_post(LwcPost<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    const size_t o = (size_t)blockIdx.y * P.ncol + ij;
    if (P.flx_int) P.flx_int[o] = P.flxd[o] + P.flxu[o];
    if (P.flxa_int) P.flxa_int[o] = P.flxad[o] + P.flxau[o];
    if (P.flc_int) P.flc_int[o] = P.flcd[o] + P.flcu[o];
    if (P.fla_int) P.fla_int[o] = P.flad[o] + P.flau[o];
    if (P.dfdtsc) P.dfdtsc[o] = 0;                       // Chou-Suarez has no clear-sky derivative (IRR:2104-2108)
    if (P.dfdtsna) P.dfdtsna[o] = P.dfdts[o];
    if (P.dfdtscna) P.dfdtscna[o] = 0;
    if (blockIdx.y == 0) {
        if (P.sfcem_int) P.sfcem_int[ij] = -P.sfcem_int[ij];
        if (P.ts_int) P.ts_int[ij] = P.ts[ij];
    }
}

// Chou-Suarez branch of SORADCORE (SOL:4484-4528): `sorad` takes the packed GEOS fields in their own layout and ordering; what the
// driver prepares for it: interface pressures in hPa, ozone as a non-negative MASS fraction from the odd-oxygen prognostic (above 1 hPa
// scaled by exp(-1.5 (log10 p - 2)^2), p the mid-layer pressure in Pa), the four condensate species and their effective radii in
// microns as (ncol, LM, 4) arrays with MAPL_UNDEF radii replaced by 36 / 14 / 50 / 50 microns.  (The reference overwrites the undefined
// radii in its packed import buffer, which it discards afterwards; here the imports stay untouched.)  The relative humidity it also
// forms (:4489) is not an argument of SHRTWAVE.
template <typename R> struct SwcPrep {
    int ncol, lm;
    const R *ple, *ox, *q[4], *r[4];      // q / r: ice, liquid, rain, snow
    R o3fac, undef;                       // MAPL_O3MW / MAPL_AIRMW
    R *plhpa, *o3, *qq3, *rr3;            // (ncol, LM+1), (ncol, LM), (ncol, LM, 4) x 2
};
// LIT: the imports are the un-packed tile's (leading dimension `tile`), read at column lit[m] of packed position m = the lane (PackIt,
// SOL:3839-3894); every store goes to the packed workspace as before.  What `sorad` reads as it is travels along: T, Q, CL (row k < LM),
// the aerosol arrays (rows (band, k)), cos zenith and the four albedos (row LM).
template <typename R> struct SwcLit : SwcPrep<R> {
    int tile;
    const int32_t *lit;
    const R *lay_in[3], *aer_in[3], *col_in[5];      // T Q CL; TAUA SSAA ASYA (all three or none); ZT ALBVR ALBVF ALBNR ALBNF
    R *lay_out[3], *aer_out[3], *col_out[5];
};
template <typename R> struct Fields<SwcLit<R>> { using S = SwcLit<R>;
    GR_TABLE(in, GEOSRAD_SWC_NIN, &S::ple, elem<&S::lay_in, 0>, elem<&S::lay_in, 1>, &S::ox, elem<&S::lay_in, 2>, elem<&S::q, 0>, elem<&S::q, 1>,
             elem<&S::q, 2>, elem<&S::q, 3>, elem<&S::r, 0>, elem<&S::r, 1>, elem<&S::r, 2>, elem<&S::r, 3>, elem<&S::aer_in, 0>, elem<&S::aer_in, 1>,
             elem<&S::aer_in, 2>, elem<&S::col_in, 0>, elem<&S::col_in, 1>, elem<&S::col_in, 2>, elem<&S::col_in, 3>, elem<&S::col_in, 4>);
};
// geosrad_sw_driver_chou*_dev, as geosrad.h has it; with `lit`, in / out are the un-packed tile's and ncol is NumLit
// na_out (GEOSRAD_SWCNA_*): the aerosol-free internals of geosrad_sw_driver_chou_na[_lit]_dev, with their dark values and keep bits on a
// tile; empty from the entry points without them
struct SwcCall {
    int ncol, lm; const void *const *in; const double *consts; int lcldmh, lcldlm; const void *hk_uv, *hk_ir; int do_drfband; void *const *out; const LitTile *lit;
    void *const *na_out; const double *dark_na; int keep_na;
};
// sorad's results on a tile: each in a plane of its own; the GEOSRAD_SWC_* outputs, then the GEOSRAD_SWCNA_* ones
constexpr TileOut swc_tile[] = {{0, PLANE, 0}, {0, PLANE, 1}, {0, PLANE, 2}, {0, PLANE, 3}, {1, PLANE, 4}, {1, PLANE, 5}, {1, PLANE, 6}, {1, PLANE, 7},
                                {1, PLANE, 8}, {1, PLANE, 9}, {8, PLANE, 10}, {8, PLANE, 11}, {8, PLANE, 12},
                                {0, PLANE, 13}, {0, PLANE, 14}, {0, PLANE, 15}, {0, PLANE, 16}, {8, PLANE, 17}};
constexpr int SWC_NTILE = GEOSRAD_SWC_NOUT + GEOSRAD_SWCNA_NOUT;
// the `out` row of which na_out[k] is the aerosol-free twin
constexpr int SWCNA_TWIN[GEOSRAD_SWCNA_NOUT] = {GEOSRAD_SWC_FSW, GEOSRAD_SWC_FSC, GEOSRAD_SWC_FSWU, GEOSRAD_SWC_FSCU, GEOSRAD_SWC_FSWBAND};
static_assert(std::size(swc_tile) == SWC_NTILE && GEOSRAD_SWC_FSCU == 3 && GEOSRAD_SWC_FSWBAND == 10 && GEOSRAD_SWCNA_FSWBANDNA == 4,
              "one row for each GEOSRAD_SWC_* and GEOSRAD_SWCNA_* output");
template <typename R, bool LIT> using SwcPrepOf = std::conditional_t<LIT, SwcLit<R>, SwcPrep<R>>;
template <typename R, bool LIT = false> __global__ void __launch_bounds__(256) k_swc_prep(SwcPrepOf<R, LIT> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    const int k = blockIdx.y;                                      // 0 .. LM
    const size_t o = (size_t)k * P.ncol + ij;
    size_t g = o, gn = P.ncol;                                     // the same cell of the imports
    if constexpr (LIT) { gn = P.tile; g = (size_t)k * gn + P.lit[ij]; }
    const R pe = P.ple[g];
    P.plhpa[o] = pe * (R)0.01;                                     // SOL:4490
    if constexpr (LIT) {
        if (k == P.lm) {
            const size_t c = g - (size_t)k * gn;
#pragma unroll
            for (int s = 0; s < 5; s++) P.col_out[s][ij] = P.col_in[s][c];
        } else {
#pragma unroll
            for (int s = 0; s < 3; s++) P.lay_out[s][o] = P.lay_in[s][g];
            if (P.aer_in[0])
                for (int b = 0; b < 8; b++) {
                    const size_t bo = (size_t)b * P.lm * P.ncol + o, bg = (size_t)b * P.lm * gn + g;
#pragma unroll
                    for (int s = 0; s < 3; s++) P.aer_out[s][bo] = P.aer_in[s][bg];
                }
        }
    }
    if (k == P.lm) return;
    const R pl = (R)0.5 * (pe + P.ple[g + gn]);                    // SOL:4488
    R o3 = P.ox[g];                                                // SOL:4523-4533
    if (pl < (R)100.) {
        const R x = gr_log10<R>(pl) - (R)2.;
        o3 = o3 * gr_exp<R>((R)-1.5 * (x * x));
    }
    o3 = o3 * P.o3fac;
    P.o3[o] = o3 > (R)0. ? o3 : (R)0.;
    const R dflt[4] = {(R)36.e-6, (R)14.e-6, (R)50.e-6, (R)50.e-6};   // SOL:4508-4511
    const size_t sp = (size_t)P.lm * P.ncol;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        P.qq3[s * sp + o] = P.q[s][g];                             // SOL:4502-4505
        R r = P.r[s][g];
        if (r == P.undef) r = dflt[s];
        P.rr3[s * sp + o] = r * (R)1.e6;                           // SOL:4512-4515
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Update_Flx (IRR:3796-3999)
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct LwUpd {
    int ncol, lm, rrtmg;                 // rrtmg != 0: the no-aerosol flavours are MAPL_UNDEF (IRR:3927-3990)
    int lev_mid_high, lev_low_mid;       // 1-based model levels separating the cloud super-layers (IRR:3811-3829)
    R undef;
    // internal state
    const R *tsinst, *ts_int, *sfcem_int, *fcld;
    const R *flx_int, *flxa_int, *flc_int, *fla_int, *flxu_int, *flxau_int, *flcu_int, *flau_int, *flxd_int, *flxad_int, *flcd_int,
        *flad_int, *dfdts, *dfdtsna, *dfdtsc, *dfdtscna;
    // exports, (IM,JM,0:LM)
    R *flx, *flxa, *flc, *fla, *flxu, *flxau, *flcu, *flau, *flxd, *flxad, *flcd, *flad;
    // exports, (IM,JM)
    R *olr, *olra, *olc, *ola, *olcc5, *dsfdts, *sfcem, *lws, *lwsa, *lcs, *las, *lcsc5, *flns, *flnsna, *flnsc, *flnsa, *dsfdts0,
        *sfcem0, *tsreff, *cldtt;
};

template <typename R> struct Fields<LwUpd<R>> { using S = LwUpd<R>;
    GR_TABLE(in, GEOSRAD_LWU_NIN, &S::tsinst, &S::ts_int, &S::sfcem_int, &S::fcld, &S::flx_int, &S::flxa_int, &S::flc_int, &S::fla_int, &S::flxu_int,
             &S::flxau_int, &S::flcu_int, &S::flau_int, &S::flxd_int, &S::flxad_int, &S::flcd_int, &S::flad_int, &S::dfdts, &S::dfdtsna, &S::dfdtsc,
             &S::dfdtscna);
    GR_TABLE(out, GEOSRAD_LWU_NOUT, &S::flx, &S::flxa, &S::flc, &S::fla, &S::flxu, &S::flxau, &S::flcu, &S::flau, &S::flxd, &S::flxad, &S::flcd, &S::flad,
             &S::olr, &S::olra, &S::olc, &S::ola, &S::olcc5, &S::dsfdts, &S::sfcem, &S::lws, &S::lwsa, &S::lcs, &S::las, &S::lcsc5, &S::flns, &S::flnsna,
             &S::flnsc, &S::flnsa, &S::dsfdts0, &S::sfcem0, &S::tsreff, &S::cldtt);
};
// V consecutive columns per thread (V = 4 floats / 2 doubles = one 16-byte access when the column count and the field
// addresses allow, else V = 1): these kernels do nothing but stream, and wide accesses are what keeps enough bytes in flight
template <typename R, int V> GR_DEV void ldv(const R *__restrict__ p, size_t o, R (&x)[V])
{
    if constexpr (V == 1) x[0] = p[o];
    else if constexpr (sizeof(R) == 4) { const float4 t = *reinterpret_cast<const float4 *>(p + o); x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w; }
    else { const double2 t = *reinterpret_cast<const double2 *>(p + o); x[0] = t.x; x[1] = t.y; }
}
template <typename R, int V> GR_DEV void stv(R *__restrict__ p, size_t o, const R (&x)[V])
{
    if constexpr (V == 1) p[o] = x[0];
    else if constexpr (sizeof(R) == 4) { float4 t; t.x = x[0]; t.y = x[1]; t.z = x[2]; t.w = x[3]; *reinterpret_cast<float4 *>(p + o) = t; }
    else { double2 t; t.x = x[0]; t.y = x[1]; *reinterpret_cast<double2 *>(p + o) = t; }
}
#define VFOR for (int v = 0; v < V; v++)
// out = expr, V columns at a time; `expr` may use the per-column arrays declared before it, indexed [v]
#define VSET(out, off, expr) do { if (out) { R r_[V]; VFOR r_[v] = (expr); stv<R, V>(out, off, r_); } } while (0)

// one thread per (V columns, level K = 0..LM); the 2-D exports are written by the K = 0 / K = LM threads
template <typename R, int V> __global__ void __launch_bounds__(256) k_lw_update_flx(LwUpd<R> U)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (ij >= U.ncol) return;
    const int n = U.ncol, lm = U.lm, K = blockIdx.y;
    const size_t o = (size_t)K * n + ij;
    const bool rr = U.rrtmg != 0;
    const R undef = U.undef;
    R delt[V], tsi[V], d[V], dc[V], dna[V], dcna[V], a[V], b[V];
    ldv<R, V>(U.tsinst, ij, tsi); ldv<R, V>(U.ts_int, ij, a);
    VFOR delt[v] = tsi[v] - a[v];                    // surface temperature change since the last full calculation
    ldv<R, V>(U.dfdts, o, d); ldv<R, V>(U.dfdtsc, o, dc);
    VFOR { dna[v] = 0; dcna[v] = 0; }
    if (!rr) { ldv<R, V>(U.dfdtsna, o, dna); ldv<R, V>(U.dfdtscna, o, dcna); }
    const bool edge = K == 0 || K == lm;
    R fx[V], fc[V], fxa[V], fca[V];
    VFOR { fx[v] = 0; fc[v] = 0; fxa[v] = 0; fca[v] = 0; }
    if (U.flx || edge) ldv<R, V>(U.flx_int, o, fx);
    if (U.flc || edge) ldv<R, V>(U.flc_int, o, fc);
    if (!rr && (U.flxa || edge)) ldv<R, V>(U.flxa_int, o, fxa);
    if (!rr && (U.fla || edge)) ldv<R, V>(U.fla_int, o, fca);
    // net downward, negated upward (linearised), downward (not linearised)
    VSET(U.flx, o, fx[v] + d[v] * delt[v]);
    VSET(U.flc, o, fc[v] + dc[v] * delt[v]);
    if (U.flxu) { ldv<R, V>(U.flxu_int, o, a); VSET(U.flxu, o, a[v] + d[v] * delt[v]); }
    if (U.flcu) { ldv<R, V>(U.flcu_int, o, a); VSET(U.flcu, o, a[v] + dc[v] * delt[v]); }
    if (U.flxd) { ldv<R, V>(U.flxd_int, o, a); VSET(U.flxd, o, a[v]); }
    if (U.flcd) { ldv<R, V>(U.flcd_int, o, a); VSET(U.flcd, o, a[v]); }
    VSET(U.flxa, o, rr ? undef : fxa[v] + dna[v] * delt[v]);
    VSET(U.fla, o, rr ? undef : fca[v] + dcna[v] * delt[v]);
    if (U.flxau) { if (!rr) ldv<R, V>(U.flxau_int, o, a); VSET(U.flxau, o, rr ? undef : a[v] + dna[v] * delt[v]); }
    if (U.flau) { if (!rr) ldv<R, V>(U.flau_int, o, a); VSET(U.flau, o, rr ? undef : a[v] + dcna[v] * delt[v]); }
    if (U.flxad) { if (!rr) ldv<R, V>(U.flxad_int, o, a); VSET(U.flxad, o, rr ? undef : a[v]); }
    if (U.flad) { if (!rr) ldv<R, V>(U.flad_int, o, a); VSET(U.flad, o, rr ? undef : a[v]); }
    if (!edge) return;
    // 2-D total cloud fraction, max overlap within / random between the super-layers (IRR:3831-3846)
    R cldtt[V];
    VFOR cldtt[v] = 0;
    if (U.cldtt || U.olcc5 || U.lcsc5) {
        R m1[V], m2[V], m3[V];
        VFOR { m1[v] = 0; m2[v] = 0; m3[v] = 0; }
        for (int k = 1; k <= U.lev_mid_high - 1; k++) { ldv<R, V>(U.fcld, (size_t)(k - 1) * n + ij, b); VFOR m1[v] = m1[v] > b[v] ? m1[v] : b[v]; }
        for (int k = U.lev_mid_high; k <= U.lev_low_mid - 1; k++) { ldv<R, V>(U.fcld, (size_t)(k - 1) * n + ij, b); VFOR m2[v] = m2[v] > b[v] ? m2[v] : b[v]; }
        for (int k = U.lev_low_mid; k <= lm; k++) { ldv<R, V>(U.fcld, (size_t)(k - 1) * n + ij, b); VFOR m3[v] = m3[v] > b[v] ? m3[v] : b[v]; }
        VFOR {
            R x = ((R)1 - m1[v]);
            x = x * ((R)1 - m2[v]);
            cldtt[v] = (R)1.0 - x * ((R)1 - m3[v]);
        }
    }
    if (K == 0) {
        // TOA: outgoing longwave radiation (IRR:3879-3893)
        VSET(U.olr, ij, -(fx[v] + d[v] * delt[v]));
        VSET(U.olc, ij, -(fc[v] + dc[v] * delt[v]));
        VSET(U.olra, ij, rr ? undef : -(fxa[v] + dna[v] * delt[v]));
        VSET(U.ola, ij, rr ? undef : -(fca[v] + dcna[v] * delt[v]));
        VSET(U.olcc5, ij, cldtt[v] <= (R)0.05 ? -(fc[v] + dc[v] * delt[v]) : undef);
        VSET(U.cldtt, ij, cldtt[v]);
    }
    if (K == lm) {
        // surface (IRR:3895-3925, :3991-3999)
        R se[V];
        ldv<R, V>(U.sfcem_int, ij, se);
        VSET(U.dsfdts, ij, -d[v]);
        VSET(U.sfcem, ij, se[v] - d[v] * delt[v]);
        VSET(U.lws, ij, fx[v] + se[v]);
        VSET(U.lcs, ij, fc[v] + se[v]);
        VSET(U.lwsa, ij, rr ? undef : fxa[v] + se[v]);
        VSET(U.las, ij, rr ? undef : fca[v] + se[v]);
        VSET(U.lcsc5, ij, cldtt[v] <= (R)0.05 ? fc[v] + se[v] : undef);
        VSET(U.flns, ij, fx[v] + d[v] * delt[v]);
        VSET(U.flnsc, ij, fc[v] + dc[v] * delt[v]);
        VSET(U.flnsna, ij, rr ? undef : fxa[v] + dna[v] * delt[v]);
        VSET(U.flnsa, ij, rr ? undef : fca[v] + dcna[v] * delt[v]);
        VSET(U.dsfdts0, ij, -d[v]);
        VSET(U.sfcem0, ij, se[v] - d[v] * delt[v]);
        VSET(U.tsreff, ij, tsi[v]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// LW_Driver, Chou-Suarez branch (geosrad_lw_driver_chou_dev): the arguments of `irrad` that are per-column (IRR:1876-1892) and the
// exports formed after it (IRR:3626-3663).  The per-layer arguments are prepared inside k_chou_prep<R, true> (chou_kernels.hpp).
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct LwkSurf {
    int ncol, lm;
    R mkappa;                                  // -MAPL_KAPPA
    const R *ple, *t, *ts, *emis;
    R *t2m, *fs, *tg, *tv, *eg, *ev, *rv;      // NS = 1: (ncol) x 4, (ncol,10) x 3
};
template <typename R> struct Fields<LwkSurf<R>> { using S = LwkSurf<R>;      // the per-layer fields go to irrad as they are
    GR_TABLE(in, GEOSRAD_LWK_NIN, &S::ple, &S::t, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, &S::ts, &S::emis, {}, {}, {});
};
// one thread per (V columns, row): row 0 = T2M, FS, TG, TV; rows 1..10 = band row - 1 of EG, EV, RV
template <typename R, int V> __global__ void __launch_bounds__(256) k_lwk_surface(LwkSurf<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (ij >= P.ncol) return;
    const int n = P.ncol, lm = P.lm;
    R a[V], b[V], c[V];
    if (blockIdx.y == 0) {
        ldv<R, V>(P.t, (size_t)(lm - 1) * n + ij, a); ldv<R, V>(P.ple, (size_t)(lm - 1) * n + ij, b); ldv<R, V>(P.ple, (size_t)lm * n + ij, c);
        VSET(P.t2m, ij, a[v] * gr_pow<R>((R)0.5 * ((R)1.0 + b[v] / c[v]), P.mkappa));      // IRR:1876
        ldv<R, V>(P.ts, ij, a);
        VSET(P.fs, ij, (R)1.0); VSET(P.tg, ij, a[v]); VSET(P.tv, ij, a[v]);                    // IRR:1888-1890
    } else {
        const size_t o = (size_t)(blockIdx.y - 1) * n + ij;
        ldv<R, V>(P.emis, ij, a);
        VSET(P.eg, o, a[v]); VSET(P.ev, o, (R)0.0); VSET(P.rv, o, (R)0.0);                     // IRR:1881-1883, :1891-1892
    }
}

template <typename R> struct LwkDiag {
    int ncol, lm;
    R taucrit, undef;                          // TAUCRIT / 2.13 (IRR:3628), MAPL_UNDEF
    const R *taudiag, *t, *ple, *ts, *dfdts, *sfcem_int, *flx_int;      // sfcem_int already positive (IRR:3611)
    R *tauir, *cldtmp, *cldprs, *tsreff, *dsfdts0, *sfcem0, *lws0;
};
template <typename R> struct Fields<LwkDiag<R>> { using S = LwkDiag<R>;      // the INTERNAL fluxes are irrad's and k_lwd_chou_post's
    GR_TABLE(in, GEOSRAD_LWK_NIN, &S::ple, &S::t, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, &S::ts, {}, {}, {}, {});
    GR_TABLE(out, GEOSRAD_LWK_NOUT, {}, {}, {}, {}, {}, {}, {}, {}, &S::dfdts, &S::sfcem_int, &S::flx_int, {}, {}, {}, {}, {}, {}, {}, &S::tauir, &S::cldtmp,
             &S::cldprs, &S::tsreff, &S::dsfdts0, &S::sfcem0, &S::lws0, {}, {});
};
// one thread per V columns, walking the layers from the top: TAUIR and the first layer whose infrared cloud optical thickness passes
// the threshold (IRR:3634-3650); the refresh-time exports ride along (IRR:3659-3663)
template <typename R, int V> __global__ void __launch_bounds__(256) k_lwk_diag(LwkDiag<R> D)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (ij >= D.ncol) return;
    const int n = D.ncol, lm = D.lm;
    const size_t sp = (size_t)lm * n;
    R a[V], b[V];
    if (D.tauir || D.cldtmp || D.cldprs) {
        int top[V], nfound = 0;
        VFOR top[v] = -1;
#pragma unroll 4
        for (int l = 0; l < lm; l++) {
            const size_t o = (size_t)l * n + ij;
            R tau[V];
            ldv<R, V>(D.taudiag, 2 * sp + o, a); ldv<R, V>(D.taudiag, 3 * sp + o, b);
            VFOR tau[v] = (R)0.5 * (a[v] + b[v]);
            if (D.tauir) stv<R, V>(D.tauir, o, tau);
            VFOR if (top[v] < 0 && tau[v] > D.taucrit) { top[v] = l; nfound++; }
            if (!D.tauir && nfound == V) break;
        }
        // layer L = top + 1: T(L) and PLE(L-1), the layer's upper edge, are both row `top` of their arrays
        VFOR {
            a[v] = D.undef; b[v] = D.undef;
            if (top[v] >= 0) {
                if (D.cldtmp) a[v] = D.t[(size_t)top[v] * n + ij + v];
                if (D.cldprs) b[v] = D.ple[(size_t)top[v] * n + ij + v];
            }
        }
        VSET(D.cldtmp, ij, a[v]); VSET(D.cldprs, ij, b[v]);
    }
    if (D.tsreff) { ldv<R, V>(D.ts, ij, a); VSET(D.tsreff, ij, a[v]); }
    if (D.dsfdts0) { ldv<R, V>(D.dfdts, sp + ij, a); VSET(D.dsfdts0, ij, -a[v]); }
    if (D.sfcem0 || D.lws0) {
        ldv<R, V>(D.sfcem_int, ij, b);
        VSET(D.sfcem0, ij, b[v]);
        if (D.lws0) { ldv<R, V>(D.flx_int, sp + ij, a); VSET(D.lws0, ij, a[v] + b[v]); }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// SORADCORE, RRTMG branch (works on the packed daytime columns; ple has LM+1 levels 1..LM+1)
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct SwdArgs {
    int ncol, lm, nb;                 // nb = 14 aerosol bands
    int iceflg, liqflg;
    const R *ple, *pl, *t, *q, *o3, *ch4, *cl, *ts;
    const R *qq_ice, *qq_liq, *rr_ice, *rr_liq;      // QQ3(:,:,1|2), RR3(:,:,1|2)
    R *taua, *ssaa, *asya;                           // (ncol,LM,nb) GEOS side: normalised IN PLACE like the reference (SOL:6116-6125)
    R co2, o2, airmw_over_h2omw, airmw_over_o3mw, rgas, grav;
    R *play, *plev, *tlay, *tlev, *h2o, *o3_r, *co2_r, *ch4_r, *o2_r, *cldf, *ciwp, *clwp, *rei, *rel, *zl, *tauaer, *ssaaer, *asmaer;
};

// LIT: the imports are the un-packed tile's (leading dimension `tile`), read at column lit[m] of packed position m = the lane (PackIt,
// SOL:3839-3894); every store goes to the packed workspace as before, and the aerosol imports are only read (the reference normalises its
// packed buffer, SOL:6116-6125 on BufInp, never the import).  The per-column imports the solver reads as they are travel along (row K = 1).
template <typename R> struct SwdLit : SwdArgs<R> {
    int tile;
    const int32_t *lit;
    const R *col_in[6];      // ZT ALAT ALBVR ALBVF ALBNR ALBNF
    R *col_out[6];
};
template <typename R> struct Fields<SwdLit<R>> { using S = SwdLit<R>;
    GR_TABLE(in, GEOSRAD_SWD_NIN, &S::ple, &S::pl, &S::t, &S::q, &S::o3, &S::ch4, &S::cl, &S::ts, &S::qq_ice, &S::qq_liq, &S::rr_ice, &S::rr_liq, &S::taua,
             &S::ssaa, &S::asya, elem<&S::col_in, 0>, elem<&S::col_in, 1>, elem<&S::col_in, 2>, elem<&S::col_in, 3>, elem<&S::col_in, 4>, elem<&S::col_in, 5>);
};
// The driver's outputs on a tile: GEOSRAD_SWD_*, then DRBAND and DFBAND of the ocean-biology coupling.  The driver's workspace planes: 0 - 5 the
// solver's surface scalars, then the band fluxes of the aerosol and the no-aerosol pass, DRBAND and DFBAND.
enum { SWD_DRBAND = GEOSRAD_SWD_NOUT, SWD_DFBAND, SWD_NROW, SWD_P_BAND = 6, SWD_P_NBAND, SWD_P_DRBAND, SWD_P_DFBAND, SWD_NPLANE };
constexpr TileOut swd_tile[] = {{0, POST, 0}, {0, POST, 1}, {0, POST, 2}, {0, POST, 3}, {1, PLANE, 0}, {1, PLANE, 1}, {1, PLANE, 2}, {1, PLANE, 3}, {1, PLANE, 4},
                                {1, PLANE, 5}, {14, PLANE, SWD_P_BAND}, {1, POST, 4}, {1, POST, 5}, {1, POST, 6}, {1, POST, 7}, {1, POST, 8}, {1, POST, 9},
                                {1, POST, 10}, {1, POST, 11}, {0, POST_NA, 0}, {0, POST_NA, 1}, {0, POST_NA, 2}, {0, POST_NA, 3}, {14, PLANE, SWD_P_NBAND},
                                {14, PLANE, SWD_P_DRBAND}, {14, PLANE, SWD_P_DFBAND}};
static_assert(std::size(swd_tile) == SWD_NROW && GEOSRAD_SWD_NIRR == 4 && GEOSRAD_SWD_FSWBAND == 10 && GEOSRAD_SWD_CLDTS == 11 && GEOSRAD_SWD_COTTP == 15 &&
              GEOSRAD_SWD_FSWNA == 19 && GEOSRAD_SWD_FSWBANDNA == 23, "one row for each GEOSRAD_SWD_* output, then DRBAND and DFBAND");
// geosrad_sw_driver_rrtmg*_dev, as geosrad.h has it; with `lit`, in / out are the un-packed tile's and ncol is NumLit; drband / dfband: the _obio
// entry points'.  rows / dark / keep: a tile's SWD_NROW outputs; the driver reads them, so a tile's record goes through swd_merge first (swd_call).
struct SwdCall {
    int ncol, lm, nb; const void *const *in; const double *consts; int iceflg, liqflg; double sc, dist; int isolvar, dyofyr, include_aerosols, lcldlm, lcldmh;
    int normflx; const void *bndsolvar, *indsolvar; void *const *out; const LitTile *lit; void *drband, *dfband; const double *dark_obio; int keep_obio;
    void *rows[SWD_NROW]; double dark[SWD_NROW]; uint64_t keep;
    bool drf() const { return drband && include_aerosols != 0; }      // do_drfband = SOLAR_TO_OBIO .and. include_aerosols (SOL:6385), else untouched
};
inline void swd_merge(SwdCall &C)
{
    for (int k = 0; k < GEOSRAD_SWD_NOUT; k++) { C.rows[k] = C.out[k]; C.dark[k] = C.lit->dark ? C.lit->dark[k] : 0.0; }
    C.rows[SWD_DRBAND] = C.drf() ? C.drband : nullptr; C.rows[SWD_DFBAND] = C.drf() ? C.dfband : nullptr;
    for (int k = 0; k < 2; k++) C.dark[SWD_DRBAND + k] = C.drf() && C.dark_obio ? C.dark_obio[k] : 0.0;
    C.keep = (C.lit->keep & ((1ull << GEOSRAD_SWD_NOUT) - 1)) | (C.drf() ? (uint64_t)(C.keep_obio & 3) << GEOSRAD_SWD_NOUT : 0);
}
template <typename R, bool LIT> using SwdArgsOf = std::conditional_t<LIT, SwdLit<R>, SwdArgs<R>>;

// ij, n: the column of the imports and their leading dimension
template <typename R> GR_DEV R swd_tlev(const SwdArgs<R> &A, int k, int ij, int n)      // TLEV(1..LM+1), SOL:6172-6176
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int lm = A.lm;
    if (k == lm + 1) return A.ts[ij];
    if (k == 1) k = 2;
    auto PLE = [&](int l) { return A.ple[(size_t)(l - 1) * n + ij]; };
    auto T = [&](int l) { return A.t[(size_t)(l - 1) * n + ij]; };
    const R dpk = PLE(k + 1) - PLE(k), dpm = PLE(k) - PLE(k - 1);        // DPR(k), DPR(k-1)
    return (T(k - 1) * dpk + T(k) * dpm) / (dpm + dpk);
}

template <typename R, bool LIT = false> __global__ void __launch_bounds__(256) k_swd_prep(SwdArgsOf<R, LIT> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int m = blockIdx.x * blockDim.x + threadIdx.x;                               // packed position
    if (m >= A.ncol) return;
    const int n = A.ncol, lm = A.lm, K = blockIdx.y + 1, LV = lm - K + 1;
    int ij = m, gn = n;                                                                // column and leading dimension of the imports
    if constexpr (LIT) { ij = A.lit[m]; gn = A.tile; }
    const size_t o = (size_t)(K - 1) * n + m, g = (size_t)(LV - 1) * gn + ij;
    const R dpr = A.ple[(size_t)LV * gn + ij] - A.ple[(size_t)(LV - 1) * gn + ij];    // DPR(LV) = PLE(LV+1) - PLE(LV)
    const R xx = (R)1.02 * (R)100 * dpr;
    A.ciwp[o] = xx * A.qq_ice[g];
    A.clwp[o] = xx * A.qq_liq[g];
    R reice = A.rr_ice[g], reliq = A.rr_liq[g];
    // SW limits (SOL:6144-6170): liqflg 0 is 10..30 here
    if (A.liqflg == 0) reliq = clampr<R>(reliq, (R)10., (R)30.);
    else if (A.liqflg == 1) reliq = clampr<R>(reliq, (R)2.5, (R)60.);
    if (A.iceflg == 0) reice = clampr<R>(reice, (R)10., (R)30.);
    else if (A.iceflg == 1) reice = clampr<R>(reice, (R)13., (R)130.);
    else if (A.iceflg == 2) reice = clampr<R>(reice, (R)5., (R)131.);
    else if (A.iceflg == 3) reice = clampr<R>(reice, (R)5., (R)140.);
    else if (A.iceflg == 4) reice = clampr<R>(reice * (R)2., (R)1., (R)200.);
    A.rei[o] = reice; A.rel[o] = reliq;
    // PLE_R(1:LM+1) = PLE(LM+1:1)/100, TLEV_R likewise (SOL:6180-6181)
    A.plev[o] = A.ple[(size_t)LV * gn + ij] / (R)100.;     // PLE(LV+1)
    A.tlev[o] = swd_tlev<R>(A, LV + 1, ij, gn);
    if (K == lm) {
        A.plev[(size_t)lm * n + m] = A.ple[ij] / (R)100.;
        A.tlev[(size_t)lm * n + m] = swd_tlev<R>(A, 1, ij, gn);
    }
    auto pos = [](R x) { return x < 0 ? (R)0 : x; };
    A.play[o] = A.pl[g] / (R)100.;
    A.tlay[o] = A.t[g];
    const R q = A.q[g];
    A.h2o[o] = pos(q / ((R)1. - q) * A.airmw_over_h2omw);
    A.o3_r[o] = pos(A.o3[g] * A.airmw_over_o3mw);
    A.ch4_r[o] = pos(A.ch4[g]);
    A.co2_r[o] = pos(A.co2);
    A.o2_r[o] = pos(A.o2);
    A.cldf[o] = pos(A.cl[g]);
    // aerosols: normalise (SOL:6116-6125) and flip (SOL:6210-6212)
    for (int b = 0; b < A.nb; b++) {
        R ta = 0, ss = 0, as = 0;
        if (A.taua) {
            const size_t ga = ((size_t)b * lm + (LV - 1)) * gn + ij;
            ta = A.taua[ga]; ss = A.ssaa[ga]; as = A.asya[ga];
            if (ta > 0 && ss > 0) { as = as / ss; ss = ss / ta; }
            else { ta = 0; ss = 0; as = 0; }
            if constexpr (!LIT) { A.taua[ga] = ta; A.ssaa[ga] = ss; A.asya[ga] = as; }
        }
        const size_t oa = ((size_t)b * lm + (K - 1)) * n + m;
        A.tauaer[oa] = ta; A.ssaaer[oa] = ss; A.asmaer[oa] = as;
    }
    if constexpr (LIT) {
        if (K == 1)
#pragma unroll
            for (int s = 0; s < 6; s++) A.col_out[s][m] = A.col_in[s][ij];
    }
}

// ZL_R (SOL:6200-6207): note the level index differs from LW (levels are 1-based here).  Reads the workspace only: packed either way.
template <typename R> __global__ void __launch_bounds__(256) k_swd_zm(SwdArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= A.ncol) return;
    const int n = A.ncol, lm = A.lm;
    R z = 0;
    A.zl[ij] = 0;
    R plm = A.play[ij];
    for (int k = 2; k <= lm; k++) {
        const R plk = A.play[(size_t)(k - 1) * n + ij];
        z = z + A.rgas * A.tlev[(size_t)(k - 1) * n + ij] / A.grav * (plm - plk) / A.plev[(size_t)(k - 1) * n + ij];
        A.zl[(size_t)(k - 1) * n + ij] = z;
        plm = plk;
    }
}

template <typename R> struct SwdPost {
    int ncol, lm, ngpt, aerosols;
    R undef;
    const R *swuflx, *swdflx, *swuflxc, *swdflxc;          // RRTMG (ncol, LM+1), 1 = surface
    const int32_t *clearCounts;
    const R *cotn[4], *cotd[4];                            // COTN?P / COTD?P: T, H, M, L
    R *fsw, *fsc, *fswu, *fscu;                            // (ncol, LM+1) model ordering
    R *cldts, *cldhs, *cldms, *cldls, *cot[4];
};

// the aerosol pass, and the no-aerosol pass whose un-flipped fluxes are the FS*NA outputs; the scalars and band fluxes are the solver's own
template <typename R> struct Fields<SwdPost<R>> { using S = SwdPost<R>;
    GR_TABLE(out, GEOSRAD_SWD_NOUT, &S::fsw, &S::fsc, &S::fswu, &S::fscu, {}, {}, {}, {}, {}, {}, {}, &S::cldts, &S::cldhs, &S::cldms, &S::cldls,
             elem<&S::cot, 0>, elem<&S::cot, 1>, elem<&S::cot, 2>, elem<&S::cot, 3>, {}, {}, {}, {}, {});
};
template <typename R> struct SwdPostNa { using S = SwdPost<R>;
    GR_TABLE(out, GEOSRAD_SWD_NOUT, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, &S::fsw, &S::fsc, &S::fswu, &S::fscu, {});
};
// the statements of the post step for one (column, level L = model level 0..LM of the un-flipped arrays): the solver's results are read
// at column ij of n, the outputs written at column c of ld
template <typename R> GR_DEV void swd_post_cell(const SwdPost<R> &P, int L, int ij, int n, int c, int ld)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int lm = P.lm;
    const size_t s = (size_t)(lm - L) * n + ij, o = (size_t)L * ld + c;
    const R u = P.swuflx[s], d = P.swdflx[s], uc = P.swuflxc[s], dcl = P.swdflxc[s];
    if (P.fsw) P.fsw[o] = d - u;                          // SOL:6447-6450
    if (P.fsc) P.fsc[o] = dcl - uc;
    if (P.fswu) P.fswu[o] = u;
    if (P.fscu) P.fscu[o] = uc;
    if (L == 0) {
        const R ng = (R)P.ngpt;
        if (P.aerosols) {                                  // SOL:6405-6410
            if (P.cldts) P.cldts[c] = (R)1. - (R)P.clearCounts[(size_t)0 * n + ij] / ng;
            if (P.cldhs) P.cldhs[c] = (R)1. - (R)P.clearCounts[(size_t)1 * n + ij] / ng;
            if (P.cldms) P.cldms[c] = (R)1. - (R)P.clearCounts[(size_t)2 * n + ij] / ng;
            if (P.cldls) P.cldls[c] = (R)1. - (R)P.clearCounts[(size_t)3 * n + ij] / ng;
        }
        for (int k = 0; k < 4; k++)                        // SOL:6416-6438
            if (P.cot[k]) {
                const R a = P.cotn[k][ij], b = P.cotd[k][ij];
                P.cot[k][c] = (a > 0 && b > 0) ? a / b : P.undef;
            }
    }
}

template <typename R> __global__ void __launch_bounds__(256) k_swd_post(SwdPost<R> P)
{
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= P.ncol) return;
    swd_post_cell<R>(P, blockIdx.y, ij, P.ncol, ij, P.ncol);
}

// k_swd_post on the un-packed tile: one thread per (TILE column, model level).  A lit column (pos >= 0) reads the solver's packed result
// at its position; a dark one receives UnPackIt's DEFAULT (SOL:6534) unless the output's keep bit is set (an InOut internal,
// SOL:6523-6524).  dark[] / keep bits in the order fsw fsc fswu fscu cldts cldhs cldms cldls cot[0..3].
template <typename R> struct SwdPostLit : SwdPost<R> {
    int tile;
    const int32_t *pos;
    R dark[12];
    uint32_t keep;
};
template <typename R> __global__ void __launch_bounds__(256) k_swd_post_lit(SwdPostLit<R> P)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= P.tile) return;
    const int n = P.ncol, L = blockIdx.y;                 // n = NumLit, the leading dimension of the solver's arrays
    const int ij = P.pos[c];
    if (ij >= 0 && ij < n) swd_post_cell<R>(P, L, ij, n, c, P.tile);
    else {
        const size_t o = (size_t)L * P.tile + c;
        auto fill = [&](R *q, int k, size_t at) { if (q && !(P.keep >> k & 1u)) q[at] = P.dark[k]; };
        fill(P.fsw, 0, o); fill(P.fsc, 1, o); fill(P.fswu, 2, o); fill(P.fscu, 3, o);
        if (L == 0) {
            fill(P.cldts, 4, c); fill(P.cldhs, 5, c); fill(P.cldms, 6, c); fill(P.cldls, 7, c);
            for (int k = 0; k < 4; k++) fill(P.cot[k], 8 + k, c);
        }
    }
}

// UnPackIt (SOL:7776-7799) of every result a solver leaves as it is, in one launch: field k holds the rows f[k].row0 .. f[k + 1].row0 - 1 of
// blockIdx.y; UnPacked(c, l) = Packed(pos[c], l) on a lit column, `dark` on a dark one unless `keep`.  One thread per (tile column, row).
constexpr int LIT_NFIELD = 26;      // the 24 GEOSRAD_SWD_* outputs + DRBAND, DFBAND
template <typename R> struct LitScatter {
    int tile, nlit, nf;
    const int32_t *pos;
    struct { const R *src; R *dst; int row0, keep; R dark; } f[LIT_NFIELD];
    int rows;                                             // row0 of the field after the last
};
// Host: k_lit_scatter's argument over the first n rows of a driver's tile table, for the outputs the caller requested.  With daytime columns
// the PLANE rows, from plane[at]; with none (nlit == 0) the dark fill of every row whose keep bit is clear.
template <typename R, size_t N>
LitScatter<R> lit_scatter_pack(const TileOut (&rows)[N], int n, int lm, const LitTile &t, int nlit, void *const *out, const R *const *plane)
{
    static_assert(N <= LIT_NFIELD, "a field of LitScatter for every row");
    LitScatter<R> S{};
    S.tile = t.tile; S.nlit = nlit; S.pos = t.pos;
    for (int k = 0; k < n; k++) {
        const int keep = (int)(t.keep >> k & 1);
        if (!out[k] || (nlit == 0 ? keep != 0 : rows[k].src != PLANE)) continue;
        S.f[S.nf].src = nlit ? plane[rows[k].at] : nullptr; S.f[S.nf].dst = (R *)out[k]; S.f[S.nf].row0 = S.rows; S.f[S.nf].keep = keep;
        S.f[S.nf].dark = t.dark ? (R)t.dark[k] : (R)0;
        S.nf++; S.rows += rows[k].nrows(lm);
    }
    return S;
}
// Host: k_swd_post_lit's tile, dark values and keep bits for one pass, from the rows of swd_tile that pass un-packs
template <typename R> void post_lit_pack(SwdPostLit<R> &P, TileSrc pass, const LitTile &t)
{
    P.tile = t.tile; P.pos = t.pos; P.keep = 0;
    for (R &d : P.dark) d = (R)0;
    for (int k = 0; k < GEOSRAD_SWD_NOUT; k++) {
        if (swd_tile[k].src != pass) continue;
        if (t.keep >> k & 1) P.keep |= 1u << swd_tile[k].at;
        P.dark[swd_tile[k].at] = t.dark ? (R)t.dark[k] : (R)0;
    }
}
template <typename R> __global__ void __launch_bounds__(256) k_lit_scatter(LitScatter<R> S)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (c >= S.tile) return;
    int k = 0;
    while (k + 1 < S.nf && S.f[k + 1].row0 <= row) k++;
    const size_t l = (size_t)(row - S.f[k].row0);
    const int m = S.pos[c];
    if (m >= 0 && m < S.nlit) S.f[k].dst[l * S.tile + c] = S.f[k].src[l * S.nlit + m];
    else if (!S.f[k].keep) S.f[k].dst[l * S.tile + c] = S.f[k].dark;
}

// ---------------------------------------------------------------------------------------------------------------------------
// UPDATE_EXPORT, 2-D block (SOL:7403-7533): albedo exports, total surface albedo, incident / surface fluxes.  One thread per column.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct SwSfc {
    int ncol, lm;
    R undef;
    const R *slr, *zth, *alb_imp[4], *dn[6];          // ALBVF ALBVR ALBNF ALBNR; DRUVRN DFUVRN DRPARN DFPARN DRNIRN DFNIRN
    const R *fswn, *fscn, *fswnan, *fscnan;           // (ncol,0:LM)
    R *alb_exp[4], *albedo, *slrtp, *dx[6], *drn[3], *slrsf, *slrsfc, *slrsfna, *slrsfcna, *slrsuf, *slrsufc, *slrsufna, *slrsufcna;
};
template <typename R> struct Fields<SwSfc<R>> { using S = SwSfc<R>;
    GR_TABLE(in, GEOSRAD_SWS_NIN, &S::slr, &S::zth, elem<&S::alb_imp, 0>, elem<&S::alb_imp, 1>, elem<&S::alb_imp, 2>, elem<&S::alb_imp, 3>, elem<&S::dn, 0>,
             elem<&S::dn, 1>, elem<&S::dn, 2>, elem<&S::dn, 3>, elem<&S::dn, 4>, elem<&S::dn, 5>, &S::fswn, &S::fscn, &S::fswnan, &S::fscnan);
    GR_TABLE(out, GEOSRAD_SWS_NOUT, elem<&S::alb_exp, 0>, elem<&S::alb_exp, 1>, elem<&S::alb_exp, 2>, elem<&S::alb_exp, 3>, &S::albedo, &S::slrtp,
             elem<&S::dx, 0>, elem<&S::dx, 1>, elem<&S::dx, 2>, elem<&S::dx, 3>, elem<&S::dx, 4>, elem<&S::dx, 5>, elem<&S::drn, 0>, elem<&S::drn, 1>,
             elem<&S::drn, 2>, &S::slrsf, &S::slrsfc, &S::slrsfna, &S::slrsfcna, &S::slrsuf, &S::slrsufc, &S::slrsufna, &S::slrsufcna);
};
template <typename R> __global__ void __launch_bounds__(256) k_sw_update_surface(SwSfc<R> U)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= U.ncol) return;
    const size_t sfc = (size_t)U.lm * U.ncol + ij;
    const R slr = U.slr[ij], undef = U.undef;
    for (int k = 0; k < 4; k++)
        if (U.alb_exp[k]) U.alb_exp[k][ij] = slr > 0 ? U.alb_imp[k][ij] * (R)1. : undef;      // FAC = 1. (SOL:7406)
    R d[6];
    for (int k = 0; k < 6; k++) d[k] = U.dn[k][ij];
    const R sum6 = d[0] + d[1] + d[2] + d[3] + d[4] + d[5];      // DRUVRN+DFUVRN+DRPARN+DFPARN+DRNIRN+DFNIRN, left to right
    R alb = sum6;
    if (slr > (R)0.0 && alb > (R)0.0) {
        R x = (R)1.0 - U.fswn[sfc] / alb;
        x = x > (R).01 ? x : (R).01;                 // max(x, .01)
        alb = x < (R)0.9 ? x : (R)0.9;               // min(.., 0.9)
    } else alb = undef;
    if (U.albedo) U.albedo[ij] = alb;
    if (U.slrtp) U.slrtp[ij] = slr;
    for (int k = 0; k < 6; k++)
        if (U.dx[k]) U.dx[k][ij] = d[k] * slr;
    if (U.drn[0] || U.drn[1] || U.drn[2]) {
        const R zth = U.zth[ij] > (R)0.0 ? U.zth[ij] : (R)0.0;          // ZTH = max(ZTH,0.0)
        const R sln = zth > (R)0.0 ? slr / zth : (R)0.0;
        if (U.drn[0]) U.drn[0][ij] = d[0] * sln;
        if (U.drn[1]) U.drn[1][ij] = d[2] * sln;
        if (U.drn[2]) U.drn[2][ij] = d[4] * sln;
    }
    if (U.slrsf) U.slrsf[ij] = sum6 * slr;
    const bool def = alb != undef;
    if (U.slrsfc) U.slrsfc[ij] = def ? (U.fscn[sfc] * slr) / ((R)1. - alb) : (R)0.0;
    if (U.slrsfna) U.slrsfna[ij] = def ? (U.fswnan[sfc] * slr) / ((R)1. - alb) : (R)0.0;
    if (U.slrsfcna) U.slrsfcna[ij] = def ? (U.fscnan[sfc] * slr) / ((R)1. - alb) : (R)0.0;
    if (U.slrsuf) U.slrsuf[ij] = alb * sum6 * slr;
    if (U.slrsufc) U.slrsufc[ij] = def ? alb * (U.fscn[sfc] / ((R)1. - alb)) * slr : (R)0.0;
    if (U.slrsufna) U.slrsufna[ij] = def ? alb * (U.fswnan[sfc] / ((R)1. - alb)) * slr : (R)0.0;
    if (U.slrsufcna) U.slrsufcna[ij] = def ? alb * (U.fscnan[sfc] / ((R)1. - alb)) * slr : (R)0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// UPDATE_EXPORT, cloud diagnostics (SOL:7006-7058, :7223-7392): super-layer cloud fractions, GETVISTAU's diffuse optical thickness
// per species (getvistau.code with ict = LCLDMH, icb = LCLDLM; its beam output and asymmetry factor are dummies here, :7270, so caib is
// not read), super-layer sums, TAUTX, COT / COTNUM, cloud top.  One thread per column, two walks down the column: the maxima (which
// GETVISTAU's cover normalisation needs for every layer), then the optics.  Each walk issues the loads of NB layers before it uses the
// first of them.  NB = 2 (94 VGPRs in fp32, 136 in fp64) measured fastest; NB = 8 needs 256 VGPRs plus AGPRs, drops to one wavefront per
// SIMD and is the slowest; a second wavefront per SIMD forced by WPS = 2 only spills it (profiles/r05_sw_clouds.md).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SWK_NB = 2, SWK_WPS = 1;
template <typename R> struct SwCld {
    int ncol, lm, ict, icb;          // ict = LCLDMH, icb = LCLDLM (model ordering, 1 = top)
    int optics;                      // some requested export needs GETVISTAU
    R grav, undef, taucrit;
    const R *in[GEOSRAD_SWK_NIN];    // GEOSRAD_SWK_* order
    R *out[GEOSRAD_SWK_NOUT];
};
template <typename R, int NB = SWK_NB, int WPS = SWK_WPS>
__global__ void __launch_bounds__(256, WPS) k_sw_update_clouds(SwCld<R> U, const SoradDev<R> *__restrict__ Tp)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= U.ncol) return;
    const int n = U.ncol, lm = U.lm, ict = U.ict, icb = U.icb;
    const R *__restrict__ fcld = U.in[GEOSRAD_SWK_FCLD];
    R *const *O = U.out;
    // aCLDH / aCLDM / aCLDL (SOL:7008-7050); also getvistau.code's cc(1:3), the same maxima
    R ch = 0, cm = 0, cl = 0;
    for (int k0 = 0; k0 < lm; k0 += NB) {
        R f[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) f[j] = k0 + j < lm ? fcld[(size_t)(k0 + j) * n + ij] : (R)0;
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int k = k0 + j + 1;
            if (k > lm) break;
            if (O[GEOSRAD_SWK_FCLD_X]) O[GEOSRAD_SWK_FCLD_X][(size_t)(k - 1) * n + ij] = f[j];      // FCLD = CLIN (:7006)
            if (k < ict) ch = ch > f[j] ? ch : f[j];
            else if (k < icb) cm = cm > f[j] ? cm : f[j];
            else cl = cl > f[j] ? cl : f[j];
        }
    }
    const R ct = (R)1. - ((R)1 - ch) * ((R)1 - cm) * ((R)1 - cl);      // aCLDT (:7054)
    const R c4[4] = {cl, cm, ch, ct};                                   // LO MD HI TT, the order of the exports
    for (int s = 0; s < 4; s++) {
        if (O[GEOSRAD_SWK_CLDLO + s]) O[GEOSRAD_SWK_CLDLO + s][ij] = c4[s];
        if (O[GEOSRAD_SWK_COTDENLO + s]) O[GEOSRAD_SWK_COTDENLO + s][ij] = c4[s];
    }
    if (!U.optics) return;

    const SoradDev<R> &T = *Tp;
    const R grav = U.grav, taucrit = U.taucrit;
    const R *__restrict__ ple = U.in[GEOSRAD_SWK_PLE];
    const R *__restrict__ q[4] = {U.in[GEOSRAD_SWK_QI], U.in[GEOSRAD_SWK_QL], U.in[GEOSRAD_SWK_QR], U.in[GEOSRAD_SWK_QS]};
    const R *__restrict__ r[4] = {U.in[GEOSRAD_SWK_RI], U.in[GEOSRAD_SWK_RL], U.in[GEOSRAD_SWK_RR], U.in[GEOSRAD_SWK_RS]};
    // GETVISTAU's cosz (ZTH = max(ZTH,0.0), :6874) enters only its beam scaling (fm, caib), which no export reads: ZTH is not read.
    R th = 0, tm = 0, tl = 0;                 // aTAUH / aTAUM / aTAUL (:7293-7345), summed top down
    int ktop = 0;                             // topmost layer with TAUCLD(:,:,L,1) > TAUCRIT (:7380-7388), 0 = none
    R pup = ple[ij];                          // PLE(k-1)
    for (int k0 = 0; k0 < lm; k0 += NB) {
        R pl[NB], f[NB], h[4][NB], re[4][NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const bool live = k0 + j < lm;
            const size_t o = (size_t)(k0 + j) * n + ij;
            pl[j] = live ? ple[o + n] : (R)0;
            f[j] = live ? fcld[o] : (R)0;
#pragma unroll
            for (int s = 0; s < 4; s++) { h[s][j] = live ? q[s][o] : (R)0; re[s][j] = live ? r[s][o] : (R)0; }
        }
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int k = k0 + j + 1;
            if (k > lm) break;
            const size_t o = (size_t)(k - 1) * n + ij;
            const R dp = pl[j] - pup;                                       // DP = PLL(:,:,1:LM)-PLL(:,:,0:LM-1) (:7238)
            const R wp = (dp * (R)1.0e3) / grav;
            const R r1 = re[0][j] * (R)1.e6, r2 = re[1][j] * (R)1.e6, r4 = re[3][j] * (R)1.e6;      // REFF = R? * 1.e6 (:7246-7249)
            R tc1, tc2, tc3, tc4, rs;
            so_cld_tau<R, false>(T, 0, wp, r1, r2, r4, h[0][j], h[1][j], h[2][j], h[3][j], tc1, tc2, tc3, tc4, rs);
            R d1 = 0, d2 = 0, d3 = 0, d4 = 0;                                // taudiff(k,1:4)
            const R tauc = tc1 + tc2 + tc3 + tc4;
            if (tauc > (R)0.02 && f[j] > (R)0.01) {
                const R cc = k < ict ? ch : (k < icb ? cm : cl);
                R fa = f[j] / cc;
                int it, ia; R ft;
                so_cld_index<R>(tauc, fa, it, ia, ft);
                const R xai = so_caif_scale<R>(T.caif, it, ia, ft, fa);
                d1 = tc1 * xai; d2 = tc2 * xai; d3 = tc3 * xai; d4 = tc4 * xai;
            }
            if (O[GEOSRAD_SWK_TAUCLI]) O[GEOSRAD_SWK_TAUCLI][o] = d1;
            if (O[GEOSRAD_SWK_TAUCLW]) O[GEOSRAD_SWK_TAUCLW][o] = d2;
            if (O[GEOSRAD_SWK_TAUCLR]) O[GEOSRAD_SWK_TAUCLR][o] = d3;
            if (O[GEOSRAD_SWK_TAUCLS]) O[GEOSRAD_SWK_TAUCLS][o] = d4;
            const R tot = d1 + d2 + d3 + d4;                                  // TAUCLD(:,:,:,1) = 1 + 2 + 3 + 4 (:7280)
            if (k < ict) th = th + tot; else if (k < icb) tm = tm + tot; else tl = tl + tot;
            if (ktop == 0 && tot > taucrit) ktop = k;
            pup = pl[j];
        }
    }
    const R undef = U.undef;
    const R tx = ct > (R)0. ? (tl * cl + tm * cm + th * ch) / ct : (R)0;       // aTAUT (:7361)
    const R t4[4] = {tl, tm, th, th + tm + tl}, x4[4] = {tl, tm, th, tx};      // TAUT = aTAUH + aTAUM + aTAUL (:7352)
    for (int s = 0; s < 4; s++) {
        if (O[GEOSRAD_SWK_TAULO + s]) O[GEOSRAD_SWK_TAULO + s][ij] = t4[s];
        if (O[GEOSRAD_SWK_COTLO + s]) O[GEOSRAD_SWK_COTLO + s][ij] = c4[s] > (R)0. ? x4[s] : undef;
        if (O[GEOSRAD_SWK_COTNUMLO + s]) O[GEOSRAD_SWK_COTNUMLO + s][ij] = c4[s] * x4[s];
    }
    if (O[GEOSRAD_SWK_TAUTX]) O[GEOSRAD_SWK_TAUTX][ij] = tx;
    if (O[GEOSRAD_SWK_CLDTMP]) O[GEOSRAD_SWK_CLDTMP][ij] = ktop ? U.in[GEOSRAD_SWK_T][(size_t)(ktop - 1) * n + ij] : undef;
    if (O[GEOSRAD_SWK_CLDPRS]) O[GEOSRAD_SWK_CLDPRS][ij] = ktop ? ple[(size_t)(ktop - 1) * n + ij] : undef;
}

// ---------------------------------------------------------------------------------------------------------------------------
// UPDATE_EXPORT, flux part (SOL:7540-7579): exports = normalised internals x SLR
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct SwUpd {
    int ncol, lm, nbands;
    const R *slr;
    const R *fswn, *fscn, *fswnan, *fscnan, *fswun, *fscun, *fswunan, *fscunan;      // (IM,JM,0:LM)
    const R *fswbandn, *fswbandnan;                                                  // (IM,JM,nbands)
    R *fsw, *fsc, *fswna, *fscna, *fswu, *fscu, *fswuna, *fscuna, *fswd, *fscd, *fswdna, *fscdna;
    R *fswband, *fswbandna;
    R *rsr, *rsc, *rsrna, *rscna, *rsrs, *rscs, *rsrsna, *rscsna, *osr, *osrclr, *osrna, *osrcna;
};

template <typename R> struct Fields<SwUpd<R>> { using S = SwUpd<R>;
    GR_TABLE(in, GEOSRAD_SWU_NIN, &S::slr, &S::fswn, &S::fscn, &S::fswnan, &S::fscnan, &S::fswun, &S::fscun, &S::fswunan, &S::fscunan, &S::fswbandn,
             &S::fswbandnan);
    GR_TABLE(out, GEOSRAD_SWU_NOUT, &S::fsw, &S::fsc, &S::fswna, &S::fscna, &S::fswu, &S::fscu, &S::fswuna, &S::fscuna, &S::fswd, &S::fscd, &S::fswdna,
             &S::fscdna, &S::fswband, &S::fswbandna, &S::rsr, &S::rsc, &S::rsrna, &S::rscna, &S::rsrs, &S::rscs, &S::rsrsna, &S::rscsna, &S::osr, &S::osrclr,
             &S::osrna, &S::osrcna);
};
// blockIdx.y = level 0..LM, then the bands; V columns per thread
template <typename R, int V> __global__ void __launch_bounds__(256) k_sw_update_export(SwUpd<R> U)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (ij >= U.ncol) return;
    const int n = U.ncol, lm = U.lm;
    R slr[V], a[V];
    ldv<R, V>(U.slr, ij, slr);
    if ((int)blockIdx.y > lm) {
        const size_t o = (size_t)(blockIdx.y - lm - 1) * n + ij;
        if (U.fswband) { ldv<R, V>(U.fswbandn, o, a); VSET(U.fswband, o, a[v] * slr[v]); }
        if (U.fswbandna) { ldv<R, V>(U.fswbandnan, o, a); VSET(U.fswbandna, o, a[v] * slr[v]); }
        return;
    }
    const int L = blockIdx.y;
    const size_t o = (size_t)L * n + ij;
    const bool edge = L == 0 || L == lm;
    R w[V], c[V], wna[V], cna[V], wu[V], cu[V], wuna[V], cuna[V];
    VFOR { w[v] = 0; c[v] = 0; wna[v] = 0; cna[v] = 0; wu[v] = 0; cu[v] = 0; wuna[v] = 0; cuna[v] = 0; }
    if (U.fsw || U.fswd || (edge && (U.rsr || U.rsrs || U.osr))) ldv<R, V>(U.fswn, o, w);
    if (U.fsc || U.fscd || (edge && (U.rsc || U.rscs || U.osrclr))) ldv<R, V>(U.fscn, o, c);
    if (U.fswna || U.fswdna || (edge && (U.rsrna || U.rsrsna || U.osrna))) ldv<R, V>(U.fswnan, o, wna);
    if (U.fscna || U.fscdna || (edge && (U.rscna || U.rscsna || U.osrcna))) ldv<R, V>(U.fscnan, o, cna);
    if (U.fswu || U.fswd) ldv<R, V>(U.fswun, o, wu);
    if (U.fscu || U.fscd) ldv<R, V>(U.fscun, o, cu);
    if (U.fswuna || U.fswdna) ldv<R, V>(U.fswunan, o, wuna);
    if (U.fscuna || U.fscdna) ldv<R, V>(U.fscunan, o, cuna);
    VSET(U.fsw, o, w[v] * slr[v]);
    VSET(U.fsc, o, c[v] * slr[v]);
    VSET(U.fswna, o, wna[v] * slr[v]);
    VSET(U.fscna, o, cna[v] * slr[v]);
    VSET(U.fswu, o, wu[v] * slr[v]);
    VSET(U.fscu, o, cu[v] * slr[v]);
    VSET(U.fswuna, o, wuna[v] * slr[v]);
    VSET(U.fscuna, o, cuna[v] * slr[v]);
    VSET(U.fswd, o, (w[v] + wu[v]) * slr[v]);
    VSET(U.fscd, o, (c[v] + cu[v]) * slr[v]);
    VSET(U.fswdna, o, (wna[v] + wuna[v]) * slr[v]);
    VSET(U.fscdna, o, (cna[v] + cuna[v]) * slr[v]);
    if (L == 0) {
        VSET(U.rsr, ij, w[v] * slr[v]);
        VSET(U.rsc, ij, c[v] * slr[v]);
        VSET(U.rsrna, ij, wna[v] * slr[v]);
        VSET(U.rscna, ij, cna[v] * slr[v]);
        VSET(U.osr, ij, ((R)1. - w[v]) * slr[v]);
        VSET(U.osrclr, ij, ((R)1. - c[v]) * slr[v]);
        VSET(U.osrna, ij, ((R)1. - wna[v]) * slr[v]);
        VSET(U.osrcna, ij, ((R)1. - cna[v]) * slr[v]);
    }
    if (L == lm) {
        VSET(U.rsrs, ij, w[v] * slr[v]);
        VSET(U.rscs, ij, c[v] * slr[v]);
        VSET(U.rsrsna, ij, wna[v] * slr[v]);
        VSET(U.rscsna, ij, cna[v] * slr[v]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// UPDATE_EXPORT, SOLAR TO OBIO conversion (SOL:7584-7737): the surface beam / diffuse fluxes of the solver's bands spread over the 33
// ocean-biology bands in proportion to the wavenumber overlap, then x SLR.  The overlaps are a fixed list (obio_bands.hpp: the walk of
// :7665-7728) that travels by value: `w`, `kb` in the walk's own order = solar bands in increasing wavenumber (position jb) and, within
// one, OBIO bands in increasing wavenumber; both partitions are gapless, so the pairs of one OBIO band are consecutive and already in
// the order the reference adds them.  Bit 7 of kb[p] marks the last pair of its OBIO band.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct ObioUpd {
    int ncol, nbands, nzero;
    const R *slr;                     // (IM,JM)
    const R *x[2];                    // the requested of DRBANDN, DFBANDN (IM,JM,nbands) ...
    R *y[2];                          // ... and their DROBIO, DFOBIO (IM,JM,33): blockIdx.y
    R w[OBIO_MAXPAIRS];               // sfrac of pair p
    int kb[OBIO_MAXPAIRS];            // its OBIO band, 0-based | 128 on the band's last pair
    int ib[OBIO_MAXBANDS];            // SOLAR_band_number_in_wvn_order - 1 at position jb
    int np[OBIO_MAXBANDS];            // pairs of that solar band
    int zkb[NB_OBIO];                 // the nzero OBIO bands no solar band reaches: 0 * SLR
};

// One thread = V columns of one family.  Its nbands inputs are loaded once, all loads in flight together, into registers indexed by the
// unrolled position jb; the pairs are then walked in a wave-uniform loop whose weights and indices are scalar loads from the arguments.
// Per OBIO band: accumulator from zero, + x(ib) * sfrac in the reference's order, * SLR, one store (:7666-7734 without the read-modify-
// write passes over DROBIO).
template <typename R, int V> __global__ void __launch_bounds__(256) k_sw_update_obio(ObioUpd<R> U)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (ij >= U.ncol) return;
    const int n = U.ncol, nb = U.nbands;
    const R *__restrict__ xin = U.x[blockIdx.y];
    R *__restrict__ out = U.y[blockIdx.y];
    R slr[V], acc[V], x[OBIO_MAXBANDS][V];
    ldv<R, V>(U.slr, ij, slr);
#pragma unroll
    for (int jb = 0; jb < OBIO_MAXBANDS; jb++)
        if (jb < nb) ldv<R, V>(xin, (size_t)U.ib[jb] * n + ij, x[jb]);
    VFOR acc[v] = 0;
    int p = 0;
#pragma unroll
    for (int jb = 0; jb < OBIO_MAXBANDS; jb++) {
        const int e = jb < nb ? p + U.np[jb] : p;
        for (; p < e; p++) {
            const R w = U.w[p];
            const int k = U.kb[p];
            VFOR acc[v] = acc[v] + x[jb][v] * w;
            if (k & 128) {
                VSET(out, (size_t)(k & 127) * n + ij, acc[v] * slr[v]);
                VFOR acc[v] = 0;
            }
        }
    }
    for (int z = 0; z < U.nzero; z++) VSET(out, (size_t)U.zkb[z] * n + ij, (R)0 * slr[v]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// parent RUN: heating rates from the net fluxes (GEOS_RadiationGridComp.F90:798-819)
// ---------------------------------------------------------------------------------------------------------------------------
template <typename R> struct RadTend {
    int ncol, lm;
    R grav, cp;
    const R *ple, *flw, *fsw, *flwclr, *fswclr, *fswna, *fla, *fscna;      // (IM,JM,0:LM); any flux may be null with its export
    const R *dsfdts, *sfcem, *trd;
    R *dtdt, *radlw, *radsw, *radlwc, *radswc, *radswna, *radlwcna, *radswcna;      // (IM,JM,LM)
    R *blw, *alw, *radsrf;
};

template <typename R> struct Fields<RadTend<R>> { using S = RadTend<R>;
    GR_TABLE(in, GEOSRAD_RT_NIN, &S::ple, &S::flw, &S::fsw, &S::flwclr, &S::fswclr, &S::fswna, &S::fla, &S::fscna, &S::dsfdts, &S::sfcem, &S::trd);
    GR_TABLE(out, GEOSRAD_RT_NOUT, &S::dtdt, &S::radlw, &S::radsw, &S::radlwc, &S::radswc, &S::radswna, &S::radlwcna, &S::radswcna, &S::blw, &S::alw,
             &S::radsrf);
};
template <typename R, int V> __global__ void __launch_bounds__(256) k_rad_tendencies(RadTend<R> P)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int ij = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (ij >= P.ncol) return;
    const int n = P.ncol, lm = P.lm, k = blockIdx.y;      // layer k+1 lies between levels k and k+1
    const size_t t = (size_t)k * n + ij, b = (size_t)(k + 1) * n + ij;
    const R gcp = P.grav / P.cp;
    R lt[V], lb[V], st[V], sb[V], x[V], y[V], dmi[V];
    VFOR { lt[v] = 0; lb[v] = 0; st[v] = 0; sb[v] = 0; dmi[v] = 0; }
    const bool last = k == lm - 1;
    if (P.dtdt || P.radlw || (last && P.radsrf)) { ldv<R, V>(P.flw, t, lt); ldv<R, V>(P.flw, b, lb); }
    if (P.dtdt || P.radsw || (last && P.radsrf)) { ldv<R, V>(P.fsw, t, st); ldv<R, V>(P.fsw, b, sb); }
    VSET(P.dtdt, t, ((lt[v] - lb[v]) + (st[v] - sb[v])) * gcp);
    if (P.radlw || P.radsw || P.radlwc || P.radswc || P.radswna || P.radlwcna || P.radswcna) {
        ldv<R, V>(P.ple, t, x); ldv<R, V>(P.ple, b, y);
        VFOR dmi[v] = P.grav / (P.cp * (y[v] - x[v]));
    }
    VSET(P.radlw, t, (lt[v] - lb[v]) * dmi[v]);
    VSET(P.radsw, t, (st[v] - sb[v]) * dmi[v]);
    if (P.radlwc) { ldv<R, V>(P.flwclr, t, x); ldv<R, V>(P.flwclr, b, y); VSET(P.radlwc, t, (x[v] - y[v]) * dmi[v]); }
    if (P.radswc) { ldv<R, V>(P.fswclr, t, x); ldv<R, V>(P.fswclr, b, y); VSET(P.radswc, t, (x[v] - y[v]) * dmi[v]); }
    if (P.radswna) { ldv<R, V>(P.fswna, t, x); ldv<R, V>(P.fswna, b, y); VSET(P.radswna, t, (x[v] - y[v]) * dmi[v]); }
    if (P.radlwcna) { ldv<R, V>(P.fla, t, x); ldv<R, V>(P.fla, b, y); VSET(P.radlwcna, t, (x[v] - y[v]) * dmi[v]); }
    if (P.radswcna) { ldv<R, V>(P.fscna, t, x); ldv<R, V>(P.fscna, b, y); VSET(P.radswcna, t, (x[v] - y[v]) * dmi[v]); }
    if (last) {
        if (P.blw) { ldv<R, V>(P.dsfdts, ij, x); VSET(P.blw, ij, x[v]); }
        if (P.alw) { R se[V], tr[V]; ldv<R, V>(P.dsfdts, ij, x); ldv<R, V>(P.sfcem, ij, se); ldv<R, V>(P.trd, ij, tr); VSET(P.alw, ij, se[v] - x[v] * tr[v]); }
        VSET(P.radsrf, ij, sb[v] + lb[v]);
    }
}

#undef VFOR
#undef VSET
#undef GR_TABLE

// ---------------------------------------------------------------------------------------------------
// Lit-column compaction of the solar component (GEOS_SolarGridComp.F90:3686 `daytime = ZTH > 0.`, PackIt / UnPackIt :7753-7799):
// SORADCORE only sees the NumLit daytime columns, packed to the front of every field in (i, j) order.
//   k_lit_index: stable list of the lit columns (one 1024-thread block, like k_partition8 of sorad): idx[m] = column of packed position m,
//                pos[column] = packed position or -1, *nlit = NumLit
//   k_lit_pack  : Packed(m, l) = UnPacked(idx[m], l)
//   k_lit_unpack: UnPacked(idx[m], l) = Packed(m, l); dark columns get DEFAULT when one is given (PRESENT(DEFAULT)), else keep their value
// ---------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(1024) k_lit_index(int ncol, const R *__restrict__ zth, int32_t *__restrict__ idx, int32_t *__restrict__ pos,
                                                    int32_t *__restrict__ nlit)
{
    __shared__ int cnt[1024];
    const int t = threadIdx.x;
    const int chunk = (ncol + 1023) / 1024;
    const int b = t * chunk, e = (b + chunk < ncol) ? b + chunk : ncol;
    int c = 0;
    for (int i = b; i < e; i++) c += zth[i] > (R)0;
    cnt[t] = c;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {          // inclusive Hillis-Steele scan
        const int v = t >= d ? cnt[t - d] : 0;
        __syncthreads();
        cnt[t] += v;
        __syncthreads();
    }
    int m = cnt[t] - c;                              // lit columns before this thread's chunk
    for (int i = b; i < e; i++) {
        if (zth[i] > (R)0) { idx[m] = i; pos[i] = m; m++; }
        else pos[i] = -1;
    }
    if (t == 0) *nlit = cnt[1023];
}
template <typename R>
__global__ void __launch_bounds__(256) k_lit_pack(int pdim, int udim, const int32_t *__restrict__ idx, const int32_t *__restrict__ nlit,
                                                  const R *__restrict__ unpacked, R *__restrict__ packed)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
    if (m >= *nlit || m >= pdim) return;             // a packed buffer shorter than NumLit holds the first pdim lit columns
    packed[(size_t)l * pdim + m] = unpacked[(size_t)l * udim + idx[m]];
}
template <typename R>
__global__ void __launch_bounds__(256) k_lit_unpack(int pdim, int udim, const int32_t *__restrict__ pos, const R *__restrict__ packed,
                                                    R *__restrict__ unpacked, int use_default, R dflt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
    if (i >= udim) return;
    const int m = pos[i];
    if (m >= 0 && m < pdim) unpacked[(size_t)l * udim + i] = packed[(size_t)l * pdim + m];
    else if (m < 0 && use_default) unpacked[(size_t)l * udim + i] = dflt;
}

}  // namespace geosrad
