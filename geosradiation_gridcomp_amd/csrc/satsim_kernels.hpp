// satsim_kernels.hpp -- the ISCCP path of GEOSsatsim_GridComp on the device: the SCOPS sub-column generator (scops.f + congvec.f), the
// ICARUS ISCCP simulator (icarus.f) and what COSP does around them (cosp.F90:167-174, cosp_isccp_simulator.F90:58-90,
// GEOS_SatsimGridComp.F90:3727-3732).  The statements are the reference's, operation by operation, in the real kind R (contraction off);
// exp, log and the powers are the precise device functions.
//
// Arrays: the reference's Fortran layouts, the point index fastest: cc (npoints,nlev), frac_out (npoints,ncol,nlev) as one byte per cell,
// boxtau (npoints,ncol), fq_isccp (npoints,7 tau,7 pressure).  Level 1 is the top of the atmosphere.
//
// Mapping.  k_scops and k_icarus_box: lane = (point, sub-column), the point fastest, so that a wave's load of a level of cc, dtau_s,
// dem_wv ... is one coalesced row and its 30 sub-columns re-read it from L2; every lane walks the levels once and carries its own
// threshold / tau / fluxtop / transmission in registers.  k_icarus_point and k_icarus_stats: lane = point.
//
// The stream of a point (congvec.f) is seed <- mod(69069 seed + 1234567 [wrapping 32 bits], 2^30) with Fortran's mod, which keeps the
// dividend's sign: |seed| < 2^30 after the first draw, and the sign matters in fp32, where real(seed) rounds.  The low 30 bits u of the
// state obey the plain LCG u <- 69069 u + 1234567 mod 2^30 whatever the signs were, so a lane reaches its draw of the next level, ncol
// draws on, with one multiply-add (constants from the host).  The sign of state n is that of t = 69069 s(n-1) + 1234567 (32 bits): with
// v = bits 30-31 of 69069 u(n-1) + 1234567, t's bits 30-31 are v for s(n-1) >= 0 and v - 1 for s(n-1) < 0 (69069 2^30 = 2^30 mod 2^32), so
// an odd v settles it (v = 3: negative) and an even one needs the predecessor's sign: ss_negative steps back with the inverse multiplier
// until an odd v, a zero state or the caller's own seed - two steps on average, never more than the draw's index.
#pragma once
#include <cstdint>

#include "lw_kernels.hpp"      // GR_DEV

namespace geosrad {

constexpr uint32_t SS_A = 69069u, SS_C = 1234567u, SS_M = (1u << 30) - 1u;
constexpr int SS_NPT = 7;     // per-point plane of k_icarus_point: ptrop, attrop, atmax, fluxtop_clrsky, meantbclr, bb(skt), btcmin
enum { SSP_PTROP, SSP_ATTROP, SSP_ATMAX, SSP_CLR, SSP_TBCLR, SSP_BBSFC, SSP_BTCMIN };

GR_DEV float ss_exp(float x) { return expf(x); }
GR_DEV double ss_exp(double x) { return exp(x); }
GR_DEV float ss_log(float x) { return logf(x); }
GR_DEV double ss_log(double x) { return log(x); }
GR_DEV float ss_pow(float x, float y) { return powf(x, y); }
GR_DEV double ss_pow(double x, double y) { return pow(x, y); }

// congvec.f:39-41
GR_DEV int32_t ss_step(int32_t s)
{
    const int32_t t = (int32_t)(SS_A * (uint32_t)s + SS_C);
    return t % (1 << 30);      // truncating remainder: the dividend's sign, as Fortran's mod
}
// congvec.f:42, :49-50
template <typename R> GR_DEV R ss_ran(int32_t s)
{
#pragma clang fp contract(off)
    R ran = (R)s * (R)0.931322574615479E-09;
    ran = ran + (R)1;
    return ran - (R)(int)ran;
}
// is state n of the stream that started at s0 negative?  u: its low 30 bits; n >= 1
GR_DEV bool ss_negative(uint32_t u, int n, int32_t s0, uint32_t ainv)
{
    bool flip = false;
    for (int m = n;; m--) {
        if (u == 0u) return flip;                                                       // -0 is 0
        if (m == 1) return flip != ((int32_t)(SS_A * (uint32_t)s0 + SS_C) < 0);         // the caller's seed may be any 32-bit integer
        const uint32_t up = (ainv * (u - SS_C)) & SS_M;
        const uint32_t v = ((SS_A * up + SS_C) >> 30) & 3u;
        if (v & 1u) return flip != (v == 3u);
        flip = flip != (v == 2u);
        u = up;
    }
}

template <typename R> struct ScopsArgs {
    int npoints, nlev, ncol, overlap;
    uint32_t jA, jC, ainv;      // u -> jA u + jC: ncol draws on; ainv = 69069^-1, all mod 2^30
    const int32_t *seed_in;     // a copy of the caller's seeds: the last sub-column's lane writes `seed` while others still read
    int32_t *seed;
    const R *cc, *conv;         // conv null: zero
    uint8_t *frac_out;
};

template <typename R>
__global__ void __launch_bounds__(256) k_scops(const ScopsArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = A.npoints, ncol = A.ncol;
    if (idx >= (size_t)n * ncol) return;
    const int j = (int)(idx % n), b = (int)(idx / n);
    const R one = (R)1;
    const int32_t s0 = A.seed_in[j];
    // the lane's first draw, b + 1 <= ncol steps in: the states themselves
    int32_t s = s0;
    for (int k = 0; k <= b; k++) s = ss_step(s);
    int draw = b + 1;
    uint32_t u = (uint32_t)s & SS_M;
    auto next_level = [&]() {
        draw += ncol;
        u = (A.jA * u + A.jC) & SS_M;
        s = ss_negative(u, draw, s0, A.ainv) ? (int32_t)u - (1 << 30) : (int32_t)u;
    };
    auto load = [&](const R *p, int ilev) { return p ? p[(size_t)ilev * n + j] : (R)0; };
    const R boxpos = ((R)(b + 1) - (R).5) / (R)ncol;
    R threshold;
    R cv = load(A.conv, 0);
    if (A.overlap == 1) threshold = boxpos;
    else {
        threshold = cv + (one - cv) * ss_ran<R>(s);
        next_level();
    }
    R tprev = 0;
    for (int ilev = 0; ilev < A.nlev; ilev++) {
        if (ilev > 0) cv = load(A.conv, ilev);
        const R tca = load(A.cc, ilev);
        const R maxocc = boxpos <= cv ? one : (R)0;
        R threshold_min = cv, maxosc = A.overlap == 1 ? one : (R)0;
        if (A.overlap == 3) {
            const R mn = tprev < tca ? tprev : tca;
            threshold_min = cv > mn ? cv : mn;
            maxosc = (threshold < mn && threshold > cv) ? one : (R)0;
        }
        const R ran = ss_ran<R>(s);
        threshold = maxocc * boxpos + (one - maxocc) * (maxosc * threshold + (one - maxosc) * (threshold_min + (one - threshold_min) * ran));
        uint8_t f = tca > threshold ? 1 : 0;
        if (threshold <= cv) f = 2;
        A.frac_out[((size_t)ilev * ncol + b) * n + j] = f;
        tprev = tca;
        if (ilev + 1 < A.nlev) next_level();
    }
    if (b == ncol - 1) A.seed[j] = s;      // the stream's last draw is this lane's
}

// the mask between its byte form and the real array a Fortran caller holds (0, 1, 2; any other value: 3 - cloud for the physical top of
// top_height = 2 only, as icarus.f:482-489, :993 treat it)
template <typename R> __global__ void __launch_bounds__(256) k_mask_to_real(size_t n, const uint8_t *__restrict__ m, R *__restrict__ f)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) f[i] = (R)m[i];
}
template <typename R> __global__ void __launch_bounds__(256) k_real_to_mask(size_t n, const R *__restrict__ f, uint8_t *__restrict__ m)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const R v = f[i]; m[i] = v == (R)0 ? 0 : v == (R)1 ? 1 : v == (R)2 ? 2 : 3; }
}

template <typename R> struct IcArgs {
    int npoints, nlev, ncol, top_height, top_height_direction;
    int ple_shift;      // `phalf` is PLE (npoints,0:nlev): phalf(1) = 0, phalf(k) = PLE(k-2) (cosp_isccp_simulator.F90:62-63 on gbx%ph = PLECOSP(:,1:LM))
    int scaled;         // cc, conv are FCLD, CCA: multiplied by 0.999999 where icarus reads them, its range check (cosp_isccp_simulator.F90:65-66;
                        // SCOPS takes them as they are, cosp.F90:392-397)
    int cosp_out;       // the fq_isccp pressure flip and the totalcldarea snap of cosp_isccp_simulator.F90:84-90
    R emsfc_lw;
    const int32_t *sunlit;
    const R *pfull, *phalf, *qv, *cc, *conv, *dtau_s, *dtau_c, *skt, *at, *dem_s, *dem_c;      // conv, dtau_c, dem_c null: zero
    const uint8_t *frac;
    // workspace: two (npoints,nlev) planes, the per-point plane, four per-sub-column planes
    R *dem_wv, *bb, *pt;
    int32_t *itrop;
    R *tbb, *ptop, *alb;      // (npoints,ncol): brightness temperature before the adjustment, cloud-top pressure in hPa, albedo
    uint8_t *bin;             // itau | ipres << 4; 0: not a cloudy sub-column of a point that is looked at
    uint32_t *err;
    R *fq, *totalcldarea, *meanptop, *meantaucld, *meanalbedocld, *meantb, *meantbclr, *boxtau, *boxptop;
};

template <typename R> GR_DEV R ss_phalf(const IcArgs<R> &A, int k, int j)      // k = 0..nlev: phalf(k + 1)
{
    if (!A.ple_shift) return A.phalf[(size_t)k * A.npoints + j];
    return k == 0 ? (R)0 : A.phalf[(size_t)(k - 1) * A.npoints + j];
}
template <typename R> GR_DEV R ss_opt(const R *p, size_t o) { return p ? p[o] : (R)0; }
template <typename R> GR_DEV R ss_tb(R flux) { return (R)1307.27 / (ss_log((R)1 + ((R)1 / flux))); }

// icarus.f:354-455, :522-626: the tropopause, the range check, dem_wv and the Planck term per level, the clear-sky radiance
template <typename R>
__global__ void __launch_bounds__(256) k_icarus_point(const IcArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = A.npoints, nlev = A.nlev;
    if (j >= n) return;
    const R one = (R)1, sc = (R)0.999999;
    uint32_t bad = 0;
    for (int k = 0; k < nlev; k++) {      // :403-455
        const size_t o = (size_t)k * n + j;
        R cc = A.cc[o], conv = ss_opt(A.conv, o);
        if (A.scaled) { cc = sc * cc; conv = sc * conv; }
        const R ts = A.dtau_s[o], tc = ss_opt(A.dtau_c, o), es = A.dem_s[o], ec = ss_opt(A.dem_c, o);
        if (cc < (R)0 || cc > one) bad |= 1u;
        if (conv < (R)0 || conv > one) bad |= 2u;
        if (ts < (R)0) bad |= 4u;
        if (tc < (R)0) bad |= 8u;
        if (es < (R)0 || es > one) bad |= 16u;
        if (ec < (R)0 || ec > one) bad |= 32u;
    }
    if (bad) atomicOr(A.err, bad);
    if (A.top_height == 2) {
        if (A.meantbclr) A.meantbclr[j] = (R)-1.E+30;
        return;
    }
    R ptrop = (R)5000., attropmin = (R)400., atmax = (R)0., attrop = (R)120.;
    int itrop = 1;
    const R wtmair = (R)28.9644, wtmh20 = (R)18.01534, Navo = (R)6.023E+23, grav = (R)9.806650E+02, pstd = (R)1.013250E+06, t0 = (R)296.;
    R fluxtop_clrsky = 0, trans = one;
    R ph = ss_phalf(A, 0, j);
    for (int k = 0; k < nlev; k++) {
        const size_t o = (size_t)k * n + j;
        const R pf = A.pfull[o], at = A.at[o], qv = A.qv[o], ph1 = ss_phalf(A, k + 1, j);
        if (pf < (R)40000. && pf > (R)5000. && at < attropmin) { ptrop = pf; attropmin = at; attrop = attropmin; itrop = k + 1; }
        const R press = pf * (R)10.;
        const R dpress = (ph1 - ph) * (R)10;
        const R atmden = dpress / grav;
        const R rvh20 = qv * wtmair / wtmh20;
        const R wk = rvh20 * Navo * atmden / wtmair;
        const R rhoave = (press / pstd) * (t0 / at);
        const R rh20s = rvh20 * rhoave;
        const R rfrgn = rhoave - rh20s;
        const R tmpexp = ss_exp((R)-0.02 * (at - t0));
        const R tauwv = wk * (R)1.e-20 * (((R)0.0224697 * rh20s * tmpexp) + ((R)3.41817e-7 * rfrgn)) * (R)0.98;
        const R dem_wv = one - ss_exp((R)-1. * tauwv);
        const R bb = one / (ss_exp((R)1307.27 / at) - one);
        A.dem_wv[o] = dem_wv; A.bb[o] = bb;
        fluxtop_clrsky = fluxtop_clrsky + dem_wv * bb * trans;
        trans = trans * (one - dem_wv);
        ph = ph1;
    }
    for (int k = itrop - 1; k < nlev; k++) {      // :377-382
        const R at = A.at[(size_t)k * n + j];
        if (at > atmax) atmax = at;
    }
    const R bbs = one / (ss_exp((R)1307.27 / A.skt[j]) - one);
    fluxtop_clrsky = fluxtop_clrsky + A.emsfc_lw * bbs * trans;
    const R tbclr = ss_tb(fluxtop_clrsky);
    R *pt = A.pt + j;
    pt[(size_t)SSP_PTROP * n] = ptrop; pt[(size_t)SSP_ATTROP * n] = attrop; pt[(size_t)SSP_ATMAX * n] = atmax; pt[(size_t)SSP_CLR * n] = fluxtop_clrsky;
    pt[(size_t)SSP_TBCLR * n] = tbclr; pt[(size_t)SSP_BBSFC * n] = bbs;
    pt[(size_t)SSP_BTCMIN * n] = one / (ss_exp((R)1307.27 / (attrop - (R)5.)) - one);      // :806
    A.itrop[j] = itrop;
    if (A.meantbclr) A.meantbclr[j] = tbclr;
}

// icarus.f:467-492, :665-753, :804-869, :930-1008 and the per-sub-column part of :1065-1166
template <typename R>
__global__ void __launch_bounds__(256) k_icarus_box(const IcArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = A.npoints, nlev = A.nlev, ncol = A.ncol, th = A.top_height;
    if (idx >= (size_t)n * ncol) return;
    const int j = (int)(idx % n), b = (int)(idx / n);
    const R one = (R)1, zero = (R)0;
    const R tauchk = (R)-1. * ss_log((R)0.9999999), rec2p13 = one / (R)2.13;
    const bool adj = th != 2;
    R tau = 0, fluxtop = 0, trans = one, ptop = 0;
    for (int k = 0; k < nlev; k++) {
        const size_t o = (size_t)k * n + j;
        const uint8_t f = A.frac[((size_t)k * ncol + b) * n + j];
        const R ds = A.dtau_s[o], dc = ss_opt(A.dtau_c, o);
        if (f == 1) tau = tau + ds;
        if (f == 2) tau = tau + dc;
        if (adj) {
            const R wv = A.dem_wv[o], bb = A.bb[o], es = A.dem_s[o], ec = ss_opt(A.dem_c, o);
            R dem = wv;
            if (f == 1) dem = one - ((one - wv) * (one - es));
            else if (f == 2) dem = one - ((one - wv) * (one - ec));
            fluxtop = fluxtop + dem * bb * trans;
            trans = trans * (one - dem);
        } else if (ptop == zero && f != 0) ptop = ss_phalf(A, k, j);      // :990-998
    }
    R tbb = (R)-1.E+30;
    if (adj) {
        const R *pt = A.pt + j;
        const R ptrop = pt[(size_t)SSP_PTROP * n], attrop = pt[(size_t)SSP_ATTROP * n], atmax = pt[(size_t)SSP_ATMAX * n];
        const R clr = pt[(size_t)SSP_CLR * n], tbclr = pt[(size_t)SSP_TBCLR * n], bbs = pt[(size_t)SSP_BBSFC * n], btcmin = pt[(size_t)SSP_BTCMIN * n];
        const int itrop = A.itrop[j];
        fluxtop = fluxtop + A.emsfc_lw * bbs * trans;
        tbb = ss_tb(fluxtop);      // :758
        R transmax = one;
        if (clr - btcmin != zero) transmax = (fluxtop - btcmin) / (clr - btcmin);
        R tauir = tau * rec2p13;
        const R tm = transmax < (R)0.9999999 ? transmax : (R)0.9999999;
        const R taumin = (R)-1. * ss_log(tm > (R)0.001 ? tm : (R)0.001);
        const bool cloudy = tau > tauchk;
        if (th == 1 && cloudy && transmax > (R)0.001 && transmax <= (R)0.9999999) {
            const R fluxtopinit = fluxtop;
            for (int icycle = 0; icycle < 2; icycle++) {
                const R emcld = one - ss_exp((R)-1. * tauir);
                fluxtop = fluxtopinit - ((one - emcld) * clr);
                const R q = fluxtop / emcld;
                fluxtop = (R)1.E-06 > q ? (R)1.E-06 : q;
                if (ss_tb(fluxtop) > (R)260.) tauir = tau / (R)2.56;
            }
        }
        R tb;
        if (cloudy) {
            tb = ss_tb(fluxtop);
            if (th == 1 && tauir < taumin) { tb = attrop - (R)5.; tau = (R)2.13 * taumin; }
        } else tb = tbclr;
        // :935-982: the last match in the direction asked for = walking down, the first one (direction 2) or the last one (direction 1)
        int k1 = 0;
        R a1 = A.at[(size_t)(itrop - 1) * n + j];
        for (int ilev = itrop; ilev < nlev; ilev++) {
            const R a2 = A.at[(size_t)ilev * n + j];
            if (((a1 >= tb && a2 <= tb) || (a1 <= tb && a2 >= tb)) && (k1 == 0 || A.top_height_direction != 2)) k1 = ilev;
            a1 = a2;
        }
        if (k1 >= 1) {
            const size_t o1 = (size_t)(k1 - 1) * n + j, o2 = o1 + n;
            const R p1 = A.pfull[o1], p2 = A.pfull[o2], t1 = A.at[o1], t2 = A.at[o2];
            const R logp1 = ss_log(p1), logp2 = ss_log(p2);
            const R d = t2 - t1, ad = d < zero ? -d : d;
            const R atd = tauchk > ad ? tauchk : ad;
            const R e = tb - t1, ae = e < zero ? -e : e;
            const R logp = logp1 + (logp2 - logp1) * ae / atd;
            ptop = ss_exp(logp);
        } else {      // a brightness temperature between attrop and atmax always matches; the reference leaves ptop unset otherwise
            if (tb <= attrop) ptop = ptrop;
            if (tb >= atmax) ptop = A.pfull[(size_t)(nlev - 1) * n + j];
        }
    }
    const bool cloudy = tau > tauchk;
    if (!cloudy) ptop = zero;
    // :1065-1166 for this sub-column; the sums over sub-columns are k_icarus_stats'
    const bool lit = A.sunlit[j] == 1 || th == 3;
    const bool on = cloudy && ptop > zero && lit;
    R alb = 0, pmb = 0;
    uint8_t bin = 0;
    if (on) {
        pmb = ptop / (R)100.;
        int itau = 1, ipres = 1;
        if (tau >= (R)0.3) { itau = 2; const R tp = ss_pow(tau, (R)0.895); alb = tp / (tp + (R)6.82); }
        if (tau >= (R)1.3) itau = 3;
        if (tau >= (R)3.6) itau = 4;
        if (tau >= (R)9.4) itau = 5;
        if (tau >= (R)23.) itau = 6;
        if (tau >= (R)60.) itau = 7;
        if (pmb >= (R)180.) ipres = 2;
        if (pmb >= (R)310.) ipres = 3;
        if (pmb >= (R)440.) ipres = 4;
        if (pmb >= (R)560.) ipres = 5;
        if (pmb >= (R)680.) ipres = 6;
        if (pmb >= (R)800.) ipres = 7;
        bin = (uint8_t)(itau | (ipres << 4));
    }
    A.tbb[idx] = tbb; A.ptop[idx] = pmb; A.alb[idx] = alb; A.bin[idx] = bin;
    if (A.boxtau) A.boxtau[idx] = on ? tau : (R)-1.E+30;
    if (A.boxptop) A.boxptop[idx] = on ? pmb : (R)-1.E+30;
}

// icarus.f:756-763, :1037-1191: the sums over the sub-columns in ibox order, the histogram, the in-cloud means
constexpr int SS_STATS_T = 128;
template <typename R>
__global__ void __launch_bounds__(SS_STATS_T) k_icarus_stats(const IcArgs<R> A)
{
#pragma clang fp contract(off)      // the statements below are the reference's, operation by operation
    __shared__ uint16_t s_cnt[49][SS_STATS_T];      // sub-columns per cloud type; a lane touches its own column only
    const int j = blockIdx.x * blockDim.x + threadIdx.x, t = threadIdx.x;
    const int n = A.npoints, ncol = A.ncol;
    if (j >= n) return;
    const R one = (R)1, zero = (R)0, miss = (R)-1.E+30;
    const bool lit = A.sunlit[j] == 1 || A.top_height == 3;
    for (int c = 0; c < 49; c++) s_cnt[c][t] = 0;
    const R boxarea = one / (R)ncol;
    R totalcldarea = 0, meanalbedocld = 0, meanptop = 0, meantb = 0;
    for (int b = 0; b < ncol; b++) {
        const size_t o = (size_t)b * n + j;
        const uint8_t bin = A.bin[o];
        if (A.top_height != 2) meantb = meantb + A.tbb[o];
        if (bin) {
            const int itau = bin & 15, ipres = bin >> 4;
            if (itau >= 2) {      // tau >= isccp_taumin
                totalcldarea = totalcldarea + boxarea;
                meanalbedocld = meanalbedocld + A.alb[o] * boxarea;
                meanptop = meanptop + A.ptop[o] * boxarea;
            }
            s_cnt[(ipres - 1) * 7 + (itau - 1)][t]++;
        }
    }
    if (A.meantb) A.meantb[j] = A.top_height != 2 ? meantb / (R)ncol : miss;
    if (A.fq)
        for (int c = 0; c < 49; c++) {
            R v = lit ? zero : miss;
            for (int k = s_cnt[c][t]; k > 0; k--) v = v + boxarea;      // fq = fq + boxarea, once per sub-column of the type
            const int ipres = c / 7, itau = c % 7;
            A.fq[(size_t)((A.cosp_out ? 6 - ipres : ipres) * 7 + itau) * n + j] = v;
        }
    R meantaucld = miss;
    if (totalcldarea > zero) {
        meanptop = meanptop / totalcldarea;
        meanalbedocld = meanalbedocld / totalcldarea;
        meantaucld = ss_pow((R)6.82 / ((one / meanalbedocld) - one), one / (R)0.895);
    } else meanptop = meanalbedocld = miss;
    if (!lit) totalcldarea = miss;
    else if (A.cosp_out && totalcldarea > (R)1.0 - (R)1.e-5 && totalcldarea < (R)1.0 + (R)1.e-5) totalcldarea = (R)1.0;
    if (A.totalcldarea) A.totalcldarea[j] = totalcldarea;
    if (A.meanptop) A.meanptop[j] = meanptop;
    if (A.meantaucld) A.meantaucld[j] = meantaucld;
    if (A.meanalbedocld) A.meanalbedocld[j] = meanalbedocld;
}

// cosp.F90:169-174: seed = int((psfc - minp) / (maxp - minp) * 100000) + 1, for one point int(psfc).  k_cosp_minmax: one block
template <typename R>
__global__ void __launch_bounds__(1024) k_cosp_minmax(int n, const R *__restrict__ psfc, R *__restrict__ mm)
{
    __shared__ R s_lo[1024], s_hi[1024];
    R lo = psfc[0], hi = lo;
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const R p = psfc[i]; lo = p < lo ? p : lo; hi = p > hi ? p : hi; }
    s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_lo[threadIdx.x] = s_lo[threadIdx.x + w] < s_lo[threadIdx.x] ? s_lo[threadIdx.x + w] : s_lo[threadIdx.x];
            s_hi[threadIdx.x] = s_hi[threadIdx.x + w] > s_hi[threadIdx.x] ? s_hi[threadIdx.x + w] : s_hi[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { mm[0] = s_lo[0]; mm[1] = s_hi[0]; }
}
template <typename R>
__global__ void __launch_bounds__(256) k_cosp_seeds(int n, const R *__restrict__ psfc, const R *__restrict__ mm, int32_t *__restrict__ seed)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (n == 1) { seed[i] = (int32_t)psfc[i]; return; }
    const R minp = mm[0], maxp = mm[1];
    seed[i] = (int32_t)((psfc[i] - minp) / (maxp - minp) * (R)100000) + 1;
}

// GEOS_SatsimGridComp.F90:3727-3732: SGFCLD = sum(frac_out, 2) / (1. * Ncolumns), a convective cell counting 2; grid (points, levels)
template <typename R>
__global__ void __launch_bounds__(256) k_sgfcld(int n, int ncol, const uint8_t *__restrict__ frac, R *__restrict__ sgfcld)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (j >= n) return;
    int s = 0;
    for (int b = 0; b < ncol; b++) s += frac[((size_t)k * ncol + b) * n + j];
    sgfcld[(size_t)k * n + j] = (R)s / ((R)1. * (R)ncol);
}

}  // namespace geosrad
