// Host program of tests/test_gridcomp_rules.py.  It carries, as the drivers stated them before the call records and tile tables of
// csrc/gridcomp_kernels.hpp existed, the test of a tile's description (ref_lit_check) and the packing of LitScatter / SwdPostLit (ref_scatter,
// ref_post_lit with the drivers' lists), and requires the same from lit_check, swd_merge, lit_scatter_pack and post_lit_pack.  lit_check: all slots
// present; every single slot null; every pair null; each scalar at each side of each of its limits, alone and with every single slot null; a
// fixed-seed sweep of random null masks, scalars and keep masks.  Every message must come up and one case must be accepted.  No pointer is
// dereferenced, so the slots hold dummy addresses.  Prints the number of cases per sweep; a mismatch ends it with status 1.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "../geosradiation_gridcomp_amd/csrc/gridcomp_kernels.hpp"
using namespace geosrad;
using R = float;
using In = const void *const *;
using Out = void *const *;
struct V { int code; const char *msg; };
static const V ACCEPT{GEOSRAD_OK, nullptr};
static V of(const char *msg) { return {msg ? GEOSRAD_EINVAL : GEOSRAD_OK, msg}; }
#define REJECT(m) return V{GEOSRAD_EINVAL, m}
static void *slot(int k) { return (void *)(uintptr_t)(0x1000 + 8 * k); }
static const double *dbl(long long on) { return on ? (const double *)slot(200) : nullptr; }
static const int32_t *i32(long long on, int k) { return on ? (const int32_t *)slot(k) : nullptr; }

// ---- the parent's statements ----------------------------------------------------------------------------------------------
static V ref_lit_check(const LitTile &t, int nlit, Out out, int nout)
{
    if (nlit < 0 || nlit > t.tile) REJECT("nlit must lie in 0 .. ncol");
    if (nlit > 0 && (!t.idx || !t.pos)) REJECT("lit_index / lit_pos null");
    bool fill = false;
    for (int k = 0; k < nout; k++) fill = fill || (out[k] && !(t.keep >> k & 1));
    if (fill && (!t.pos || !t.dark)) REJECT("an output whose keep bit is clear needs lit_pos and dark");
    return ACCEPT;
}
struct RefObio { void *drband, *dfband; const double *dark; int keep; };      // the parent's record of DRBAND / DFBAND

// ---- the sweep ------------------------------------------------------------------------------------------------------------
struct Case { const void *in[64]; void *out[64]; long long s[16]; };
struct Entry {
    const char *name;
    int nin, nout;
    std::vector<std::vector<long long>> cand;      // per scalar: its values, the first of each accepted together
    int mask;                                        // the scalar that is a keep mask (random 64-bit values in the random sweep), or -1
    std::function<V(const Case &)> ref, now;
    std::vector<const char *> msgs;                  // every message of the parent's text
};
static long total = 0;
static void run(const Entry &E)
{
    std::set<std::string> seen;
    long n = 0, accepted = 0;
    auto one = [&](const Case &c) {
        const V a = E.ref(c), b = E.now(c);
        n++;
        if (a.code != b.code || std::string(a.msg ? a.msg : "") != std::string(b.msg ? b.msg : "")) {
            fprintf(stderr, "%s case %ld: parent (%d, %s), now (%d, %s)\n", E.name, n, a.code, a.msg ? a.msg : "-", b.code, b.msg ? b.msg : "-");
            exit(1);
        }
        if (a.code == GEOSRAD_OK) accepted++; else seen.insert(a.msg);
    };
    Case base{};
    for (int k = 0; k < 64; k++) { base.in[k] = slot(k); base.out[k] = slot(64 + k); }
    for (size_t i = 0; i < E.cand.size(); i++) base.s[i] = E.cand[i][0];
    const int ns = E.nin + E.nout;
    auto null = [&](Case &c, int k) { if (k < E.nin) c.in[k] = nullptr; else c.out[k - E.nin] = nullptr; };
    one(base);
    for (int i = 0; i < ns; i++) {
        Case c = base; null(c, i); one(c);
        for (int j = i + 1; j < ns; j++) { Case d = c; null(d, j); one(d); }
    }
    for (size_t i = 0; i < E.cand.size(); i++)
        for (const long long v : E.cand[i]) {
            Case c = base; c.s[i] = v; one(c);
            for (int k = 0; k < ns; k++) { Case d = c; null(d, k); one(d); }
        }
    std::mt19937_64 rng(20261018);
    for (int it = 0; it < 20000; it++) {
        Case c = base;
        const int shift = 1 + 2 * (it % 3);      // a slot is null with probability 1/2, 1/8, 1/32
        for (int k = 0; k < ns; k++) if ((rng() & ((1u << shift) - 1)) == 0) null(c, k);
        for (size_t i = 0; i < E.cand.size(); i++) if (rng() & 1) c.s[i] = E.cand[i][rng() % E.cand[i].size()];
        if (E.mask >= 0 && (rng() & 1)) c.s[E.mask] = (long long)rng();
        one(c);
    }
    for (const char *m : E.msgs) if (!seen.count(m)) { fprintf(stderr, "%s: the sweep never produced \"%s\"\n", E.name, m); exit(1); }
    if (seen.size() != E.msgs.size()) { fprintf(stderr, "%s: %zu messages seen, %zu listed\n", E.name, seen.size(), E.msgs.size()); exit(1); }
    if (!accepted) { fprintf(stderr, "%s: no case accepted\n", E.name); exit(1); }
    printf("%s %ld\n", E.name, n);
    total += n;
}

// ---- the packing of LitScatter / SwdPostLit, the parent's statements ---------------------------------------------------------------
struct LitField { int k; const R *src; int rows; };
using LitFields = std::vector<LitField>;
static LitScatter<R> ref_scatter(const LitTile &t, int nlit, Out out, const LitFields &fields)
{
    LitScatter<R> S{};
    S.tile = t.tile; S.nlit = nlit; S.pos = t.pos;
    for (const LitField &f : fields) {
        const int keep = (int)(t.keep >> f.k & 1);
        if (!out[f.k] || (nlit == 0 && keep)) continue;
        if (S.nf == LIT_NFIELD) { fprintf(stderr, "lit_scatter: too many fields\n"); exit(1); }
        S.f[S.nf].src = f.src; S.f[S.nf].dst = (R *)out[f.k]; S.f[S.nf].row0 = S.rows; S.f[S.nf].keep = keep;
        S.f[S.nf].dark = t.dark ? (R)t.dark[f.k] : (R)0;
        S.nf++; S.rows += f.rows;
    }
    return S;
}
static void ref_post_lit(SwdPostLit<R> &P, const LitTile *lit, std::initializer_list<int> ix)
{
    P.tile = lit->tile; P.pos = lit->pos; P.keep = 0;
    int s = 0;
    for (const int k : ix) {
        if (k >= 0 && (lit->keep >> k & 1)) P.keep |= 1u << s;
        P.dark[s++] = k >= 0 && lit->dark ? (R)lit->dark[k] : (R)0;
    }
}
static void same(const char *what, long n, const LitScatter<R> &a, const LitScatter<R> &b)
{
    bool ok = a.tile == b.tile && a.nlit == b.nlit && a.nf == b.nf && a.pos == b.pos && a.rows == b.rows;
    for (int k = 0; k < LIT_NFIELD; k++)
        ok = ok && a.f[k].src == b.f[k].src && a.f[k].dst == b.f[k].dst && a.f[k].row0 == b.f[k].row0 && a.f[k].keep == b.f[k].keep && a.f[k].dark == b.f[k].dark;
    if (!ok) { fprintf(stderr, "%s case %ld: LitScatter differs (nf %d / %d, rows %d / %d)\n", what, n, a.nf, b.nf, a.rows, b.rows); exit(1); }
}
static void same(const char *what, long n, const SwdPostLit<R> &a, const SwdPostLit<R> &b)
{
    bool ok = a.tile == b.tile && a.pos == b.pos && a.keep == b.keep;
    for (int k = 0; k < 12; k++) ok = ok && a.dark[k] == b.dark[k];
    if (!ok) { fprintf(stderr, "%s case %ld: SwdPostLit differs (keep %x / %x)\n", what, n, a.keep, b.keep); exit(1); }
}
static void pack_sweeps()
{
    std::mt19937_64 rng(20261018);
    double dark[SWD_NROW], dark_obio[2];
    for (int k = 0; k < SWD_NROW; k++) dark[k] = 1.5 + k;
    dark_obio[0] = -7.25; dark_obio[1] = -9.5;
    R *plane[13];
    for (int k = 0; k < 13; k++) plane[k] = (R *)slot(300 + k);
    const int lm = 72;
    long n = 0;
    for (int it = 0; it < 6000; it++, n++) {      // the RRTMG driver
        void *out[GEOSRAD_SWD_NOUT];
        const int shift = it % 3;                   // an output is requested with probability 1/2, 1/4 (mostly without the no-aerosol family), 7/8
        for (int k = 0; k < GEOSRAD_SWD_NOUT; k++) out[k] = (shift == 2 ? (rng() & 7) != 0 : (rng() & ((2u << shift) - 1)) == 0) ? slot(64 + k) : nullptr;
        if (it % 5 == 0) for (int k = GEOSRAD_SWD_FSWNA; k <= GEOSRAD_SWD_FSWBANDNA; k++) out[k] = nullptr;
        const bool has_dark = rng() & 3, with_obio = rng() & 1, has_dark_obio = rng() & 3;
        const LitTile lit{100, (const int32_t *)slot(401), (const int32_t *)slot(402), has_dark ? dark : nullptr, (it % 7 == 0) ? ~0ull : (it % 11 == 0) ? 0ull : rng()};
        const RefObio ob{with_obio ? slot(90) : nullptr, with_obio ? slot(91) : nullptr, has_dark_obio ? dark_obio : nullptr, (int)(rng() & 3)};
        const RefObio *obio = (it & 1) ? &ob : nullptr;
        const int include_aerosols = (rng() & 3) != 0, nlit = (it & 2) ? 37 : 0;
        // parent
        const bool drf = obio && obio->drband && include_aerosols != 0;
        enum { X_DRBAND = GEOSRAD_SWD_NOUT, X_DFBAND, X_NOUT };
        void *xout[X_NOUT];
        double xdark[X_NOUT];
        LitTile xl = lit;
        for (int k = 0; k < GEOSRAD_SWD_NOUT; k++) { xout[k] = out[k]; xdark[k] = lit.dark ? lit.dark[k] : 0.0; }
        xout[X_DRBAND] = drf ? obio->drband : nullptr; xout[X_DFBAND] = drf ? obio->dfband : nullptr;
        for (int k = 0; k < 2; k++) xdark[X_DRBAND + k] = drf && obio->dark ? obio->dark[k] : 0.0;
        xl.dark = xdark;
        xl.keep = (lit.keep & ((1ull << GEOSRAD_SWD_NOUT) - 1)) | (drf ? (uint64_t)(obio->keep & 3) << GEOSRAD_SWD_NOUT : 0);
        auto rows = [lm](int k) {
            return k <= GEOSRAD_SWD_FSCU || (k >= GEOSRAD_SWD_FSWNA && k <= GEOSRAD_SWD_FSCUNA) ? lm + 1 : (k == GEOSRAD_SWD_FSWBAND || k == GEOSRAD_SWD_FSWBANDNA ? 14 : 1);
        };
        const bool want_na = out[GEOSRAD_SWD_FSWNA] || out[GEOSRAD_SWD_FSCNA] || out[GEOSRAD_SWD_FSWUNA] || out[GEOSRAD_SWD_FSCUNA] || out[GEOSRAD_SWD_FSWBANDNA];
        R **scal = plane, *band = plane[6], *nband = plane[7], **drfb = plane + 8;
        const int sc_ix[6] = {GEOSRAD_SWD_NIRR, GEOSRAD_SWD_NIRF, GEOSRAD_SWD_PARR, GEOSRAD_SWD_PARF, GEOSRAD_SWD_UVRR, GEOSRAD_SWD_UVRF};
        LitFields F;
        if (nlit == 0) {
            for (int k = 0; k < GEOSRAD_SWD_NOUT; k++) F.push_back({k, nullptr, rows(k)});
            if (drf) for (int k = X_DRBAND; k < X_NOUT; k++) F.push_back({k, nullptr, 14});
        } else {
            for (int k = 0; k < 6; k++) F.push_back({sc_ix[k], scal[k], 1});
            F.push_back({GEOSRAD_SWD_FSWBAND, band, 14});
            if (want_na) F.push_back({GEOSRAD_SWD_FSWBANDNA, nband, 14});
            if (drf) for (int k = 0; k < 2; k++) F.push_back({X_DRBAND + k, drfb[k], 14});
        }
        const LitScatter<R> S0 = ref_scatter(xl, nlit, xout, F);
        SwdPostLit<R> Q0{}, N0{};
        ref_post_lit(Q0, &lit, {GEOSRAD_SWD_FSW, GEOSRAD_SWD_FSC, GEOSRAD_SWD_FSWU, GEOSRAD_SWD_FSCU, GEOSRAD_SWD_CLDTS, GEOSRAD_SWD_CLDHS,
                                GEOSRAD_SWD_CLDMS, GEOSRAD_SWD_CLDLS, GEOSRAD_SWD_COTTP, GEOSRAD_SWD_COTHP, GEOSRAD_SWD_COTMP, GEOSRAD_SWD_COTLP});
        ref_post_lit(N0, &lit, {GEOSRAD_SWD_FSWNA, GEOSRAD_SWD_FSCNA, GEOSRAD_SWD_FSWUNA, GEOSRAD_SWD_FSCUNA, -1, -1, -1, -1, -1, -1, -1, -1});
        // tables
        SwdCall C{};
        C.ncol = nlit; C.lm = lm; C.out = out; C.lit = &lit; C.include_aerosols = include_aerosols;
        if (obio) { C.drband = ob.drband; C.dfband = ob.dfband; C.dark_obio = ob.dark; C.keep_obio = ob.keep; }
        swd_merge(C);
        const LitTile t{lit.tile, lit.idx, lit.pos, C.dark, C.keep};
        same("pack_swd", n, S0, lit_scatter_pack<R>(swd_tile, SWD_NROW, lm, t, nlit, C.rows, plane));
        SwdPostLit<R> Q1{}, N1{};
        post_lit_pack(Q1, POST, t); post_lit_pack(N1, POST_NA, t);
        same("pack_swd", n, Q0, Q1); same("pack_swd", n, N0, N1);
    }
    printf("pack_swd %ld\n", n);
    total += n;
    for (n = 0; n < 3000; n++) {      // the Chou-Suarez driver
        void *out[GEOSRAD_SWC_NOUT];
        for (int k = 0; k < GEOSRAD_SWC_NOUT; k++) out[k] = (n % 3 == 0 || (rng() & 3)) ? slot(64 + k) : nullptr;
        const LitTile lit{100, (const int32_t *)slot(401), (const int32_t *)slot(402), (rng() & 3) ? dark : nullptr, (n % 7 == 0) ? ~0ull : rng()};
        const int do_drfband = rng() & 1, nlit = (n & 1) ? 37 : 0, nres = do_drfband ? GEOSRAD_SWC_NOUT : GEOSRAD_SWC_DRBAND;
        auto rows = [lm](int k) { return k <= GEOSRAD_SWC_FSCU ? lm + 1 : (k >= GEOSRAD_SWC_FSWBAND ? 8 : 1); };
        LitFields F;
        for (int k = 0; k < nres; k++) F.push_back({k, nlit ? plane[k] : nullptr, rows(k)});
        same("pack_swc", n, ref_scatter(lit, nlit, out, F), lit_scatter_pack<R>(swc_tile, nres, lm, lit, nlit, out, plane));
    }
    printf("pack_swc %ld\n", n);
    total += n;
}

int main()
{
    // s: tile, nlit, lit_index, lit_pos, dark, keep; the slots are the tile's outputs (the RRTMG driver's, then the Chou-Suarez driver's with DRBAND / DFBAND)
    for (const int nout : {(int)GEOSRAD_SWD_NOUT, (int)GEOSRAD_SWC_NOUT}) {
        auto tile = [](const Case &c) { return LitTile{(int)c.s[0], i32(c.s[2], 210), i32(c.s[3], 211), dbl(c.s[4]), (uint64_t)c.s[5]}; };
        run({nout == GEOSRAD_SWD_NOUT ? "lit_check_swd" : "lit_check_swc", 0, nout, {{100, 0, 1}, {10, -1, 0, 100, 101}, {1, 0}, {1, 0}, {1, 0}, {0, -1, 0x555555}}, 5,
             [=](const Case &c) { return ref_lit_check(tile(c), c.s[1], c.out, nout); }, [=](const Case &c) { return of(lit_check(tile(c), c.s[1], c.out, nout)); },
             {"nlit must lie in 0 .. ncol", "lit_index / lit_pos null", "an output whose keep bit is clear needs lit_pos and dark"}});
    }
    pack_sweeps();
    printf("total %ld\n", total);
    return 0;
}
