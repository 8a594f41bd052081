// geosrad.hip -- C-ABI (include/geosrad.h) of the MI355X-native radiation hot path: context, coefficient
// table upload (GRTB blobs -> GPU-friendly layouts), HBM workspace, kernel launches.
// There is deliberately NO CPU fallback: without a HIP device geosrad_create() fails with GEOSRAD_ENODEV.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <memory>
#include <atomic>
#include <functional>
#include <chrono>

#include <dlfcn.h>
#include <sched.h>
#include <cstddef>
#include <cstdint>
#include "../../include/geosrad.h"
#include "../../include/geosrad_gettau.h"
#include "../../include/geosrad_satsim.h"
#include "../../include/geosrad_misr_modis.h"
#include "../../include/geosrad_lidar.h"
#include "../../include/geosrad_radar.h"
#include "dev_buf.hpp"
#include "lw_device.hpp"
#include "lw_kernels.hpp"
#include "sw_kernels.hpp"
#include "mcica_kernels.hpp"
#include "sw_radval_kernels.hpp"
#include "chou_kernels.hpp"
#include "sorad_kernels.hpp"
#include "gridcomp_kernels.hpp"
#include "gettau_kernels.hpp"
#include "satsim_kernels.hpp"
#include "misr_modis_kernels.hpp"
#include "lidar_kernels.hpp"
#include "radar_kernels.hpp"
#include "lw_cols.hpp"
#include "lw_split.hpp"
#include "sw_reform.hpp"

using namespace geosrad;

namespace {

struct BlobEntry { int kind, ndim, dims[4]; const char *data; size_t count; };
struct Blob {
    int realbytes = 0;
    std::map<std::string, BlobEntry> e;
    std::string err;
    bool parse(const void *blob, size_t nbytes)
    {
        const char *b = (const char *)blob;
        if (nbytes < 12 || memcmp(b, "GRTB", 4) != 0) { err = "not a GRTB blob"; return false; }
        int32_t ver, rb;
        memcpy(&ver, b + 4, 4); memcpy(&rb, b + 8, 4);
        if (ver != 1 || (rb != 4 && rb != 8)) { err = "unsupported GRTB version / real size"; return false; }
        realbytes = rb;
        size_t off = 12;
        while (true) {
            if (off + 56 > nbytes) { err = "truncated GRTB blob"; return false; }
            char name[33]; memcpy(name, b + off, 32); name[32] = 0;
            int32_t h[6]; memcpy(h, b + off + 32, 24);
            off += 56;
            if (!strcmp(name, "END")) break;
            BlobEntry en; en.kind = h[0]; en.ndim = h[1];
            size_t cnt = 1;
            for (int k = 0; k < 4; k++) { en.dims[k] = h[2 + k]; if (k < en.ndim) cnt *= (size_t)h[2 + k]; }
            en.count = cnt; en.data = b + off;
            size_t nb = cnt * (size_t)(en.kind < 0 ? -en.kind : en.kind);
            if (off + nb > nbytes) { err = "truncated GRTB blob"; return false; }
            off += nb + ((8 - nb % 8) % 8);
            e[name] = en;
        }
        return true;
    }
};

// inside a context's member functions: a failed HIP call becomes GEOSRAD_EHIP with the call's text in last_error (geosrad_ctx::hip_rc)
#define HIPCHK(call) do { if (const int rc_ = hip_rc(#call, (call))) return rc_; } while (0)

// ---- KISS jump-ahead constants (see mcica_kernels.hpp: KissJump) --------------------------------------------
static uint32_t xs_step(uint32_t x) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; }
static uint32_t mat_apply(const uint32_t *cols, uint32_t v)
{
    uint32_t y = 0;
    for (int i = 0; i < 32; i++) if ((v >> i) & 1u) y ^= cols[i];
    return y;
}
static uint32_t powmod(uint64_t a, uint64_t n, uint64_t m)
{
    uint64_t r = 1 % m; a %= m;
    while (n) { if (n & 1) r = r * a % m; a = a * a % m; n >>= 1; }
    return (uint32_t)r;
}
static KissJump make_kiss_jump(uint64_t n)
{
    KissJump J;
    // LCG: compose (A,C) by binary exponentiation of x -> a x + c
    uint32_t A = 1, C = 0, a = 69069u, c = 1327217885u;
    for (uint64_t k = n; k; k >>= 1) {
        if (k & 1) { A = A * a; C = C * a + c; }
        c = c * a + c; a = a * a;          // (a,c) o (a,c)
    }
    J.A1 = A; J.C1 = C;
    // xorshift matrix power
    uint32_t R[32], P[32], t[32];
    for (int i = 0; i < 32; i++) { R[i] = 1u << i; P[i] = xs_step(1u << i); }
    for (uint64_t k = n; k; k >>= 1) {
        if (k & 1) { for (int i = 0; i < 32; i++) t[i] = mat_apply(P, R[i]); memcpy(R, t, sizeof t); }
        for (int i = 0; i < 32; i++) t[i] = mat_apply(P, P[i]);
        memcpy(P, t, sizeof t);
    }
    memcpy(J.M2, R, sizeof R);
    J.K3 = powmod(18000u, n, 18000ull * 65536ull - 1ull);
    J.K4 = powmod(30903u, n, 30903ull * 65536ull - 1ull);
    return J;
}
// staging of one coefficient blob into GPU-friendly layouts: k-table rows [index][NGP = pad4(ng)] so that a lane
// fetches 4 consecutive g-points of its own row with one 16-byte load
template <typename R> struct TableStage {
    const Blob &B;
    std::vector<char> stage;
    std::vector<std::pair<const R **, size_t>> fix;   // (pointer slot, byte offset)
    std::string missing;
    explicit TableStage(const Blob &b) : B(b) {}
    const R *get(const std::string &nm, size_t expect)
    {
        auto it = B.e.find(nm);
        if (it == B.e.end() || it->second.kind != (int)sizeof(R) || (expect && it->second.count != expect)) {
            missing += nm + " ";
            return nullptr;
        }
        return (const R *)it->second.data;
    }
    size_t reserve(size_t nreal)
    {
        size_t off = (stage.size() + 15) & ~(size_t)15;
        stage.resize(off + nreal * sizeof(R), 0);
        return off;
    }
    R *at(size_t off) { return (R *)(stage.data() + off); }
    // Fortran (n1, ng) -> [n1][NGP]
    void tr2(const R **slot, const std::string &nm, int n1, int ng)
    {
        const R *s = get(nm, (size_t)n1 * ng);
        if (!s) return;
        const int ngp = pad4(ng);
        size_t off = reserve((size_t)n1 * ngp);
        for (int g = 0; g < ng; g++)
            for (int i = 0; i < n1; i++) at(off)[(size_t)i * ngp + g] = s[(size_t)g * n1 + i];
        fix.push_back({slot, off});
    }
    // Fortran (nsp, 19, ng) -> [19][nsp][NGP]
    void tr3(const R **slot, const std::string &nm, int nsp, int ng)
    {
        const R *s = get(nm, (size_t)nsp * 19 * ng);
        if (!s) return;
        const int ngp = pad4(ng);
        size_t off = reserve((size_t)19 * nsp * ngp);
        for (int g = 0; g < ng; g++)
            for (int im = 0; im < 19; im++)
                for (int j = 0; j < nsp; j++) at(off)[((size_t)im * nsp + j) * ngp + g] = s[((size_t)g * 19 + im) * nsp + j];
        fix.push_back({slot, off});
    }
    // Fortran (ng, m) -> [m][NGP]   (m = 1 for plain per-g vectors)
    void rows(const R **slot, const std::string &nm, int ng, int m)
    {
        const R *s = get(nm, (size_t)ng * m);
        if (!s) return;
        const int ngp = pad4(ng);
        size_t off = reserve((size_t)m * ngp);
        for (int j = 0; j < m; j++)
            for (int g = 0; g < ng; g++) at(off)[(size_t)j * ngp + g] = s[(size_t)j * ng + g];
        fix.push_back({slot, off});
    }
    // one scalar replicated over a [NGP] row
    void splat(const R **slot, const std::string &nm, int ng)
    {
        const R *s = get(nm, 1);
        if (!s) return;
        const int ngp = pad4(ng);
        size_t off = reserve((size_t)ngp);
        for (int g = 0; g < ngp; g++) at(off)[g] = *s;
        fix.push_back({slot, off});
    }
    void raw(const R **slot, const std::string &nm, size_t cnt)
    {
        const R *s = get(nm, cnt);
        if (!s) return;
        size_t off = reserve(cnt);
        memcpy(at(off), s, cnt * sizeof(R));
        fix.push_back({slot, off});
    }
    R scalar(const std::string &nm) { const R *s = get(nm, 1); return s ? *s : (R)0; }
    bool ints(const std::string &nm, size_t cnt, int32_t *dst)
    {
        auto it = B.e.find(nm);
        if (it == B.e.end() || it->second.kind != -4 || it->second.count != cnt) { missing += nm + " "; return false; }
        memcpy(dst, it->second.data, cnt * sizeof(int32_t));
        return true;
    }
};

// roctx ranges with the reference's MAPL timer names around the kernel groups (the names of GEOS_IrradGridComp.F90:1138-1155 and
// rrtmg_sw_rad.F90:1181-1200 / rrtmg_sw_spcvmc.F90:382-567 survive on the GPU timeline: `rocprofv3 --marker-trace`).  Off unless
// GEOSRAD_ROCTX=1; the marker library is looked up at run time (no link dependency).  A fused kernel group carries the names of all the
// reference stages it covers, nested.
struct RoctxApi {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi()
    {
        const char *e = getenv("GEOSRAD_ROCTX");
        if (!e || atoi(e) == 0) return;
        for (const char *lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            void *h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
static RoctxApi &roctx_api() { static RoctxApi a; return a; }
// kernel-group id (geosrad_kernel_name) -> the reference timers it stands for (up to three, outermost first)
static const char *const ROCTX_NAMES[14][3] = {
    {"---RRTMG_RUN", "k_validate_pwv", nullptr}, {"---RRTMG_RUN", "setcoef", nullptr}, {"---RRTMG_CLDSGEN", "overlap", nullptr},
    {"---RRTMG_CLDSGEN", "---RRTMG_CLDPRMC", nullptr}, {"---RRTMG_RUN", "taumol+rtrnmc", nullptr}, {"---RRTMG_RUN", "reduce", nullptr},
    {"---RRTMG_PART", nullptr, nullptr}, {"---RRTMG_SETCOEF", nullptr, nullptr}, {"---RRTMG_TAUMOL", "---RRTMG_REFTRA", "---RRTMG_VRTQDR"},
    {"---RRTMG_PART", "reduce", nullptr}, {"---IRRAD_RUN", "prep", nullptr}, {"---IRRAD_RUN", "bands", nullptr}, {"---SORAD_RUN", "prep", nullptr},
    {"---SORAD_RUN", "passes", nullptr}};

static const char *LW_NEG_NAMES[21] = {"play", "tlay", "h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr",
                                       "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr", "cldf", "ciwp", "clwp", "rei", "rel",
                                       "plev", "tsfc", "emis", "tauaer"};

}  // namespace

// The copy threads of the host-pointer entry points: created once per context (first chunk that is worth splitting) and parked on a
// condition variable between chunks - a chunk's gather / scatter is a few milliseconds, a std::thread spawn + join per chunk and
// direction was a measurable part of it
class CopyPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    const std::function<void(size_t, size_t)> *job = nullptr;
    size_t nitems = 0, per = 0;
    int pending = 0;
    unsigned long gen = 0;
    bool quit = false;
    void loop(int t)
    {
        unsigned long seen = 0;
        for (;;) {
            const std::function<void(size_t, size_t)> *f; size_t lo, hi;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return quit || gen != seen; });
                if (quit) return;
                seen = gen; f = job;
                lo = (size_t)t * per; hi = lo + per < nitems ? lo + per : nitems;
            }
            if (lo < hi) (*f)(lo, hi);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--pending == 0) cv_done.notify_one();
            }
        }
    }
public:
    explicit CopyPool(int n) { for (int t = 0; t < n; t++) th.emplace_back([this, t] { loop(t); }); }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv_go.notify_all();
        for (auto &t : th) t.join();
    }
    int size() const { return (int)th.size(); }
    // fn(lo, hi) over [0, n) cut into size() contiguous pieces; returns when all pieces are done
    void run(size_t n, const std::function<void(size_t, size_t)> &fn)
    {
        std::unique_lock<std::mutex> lk(mu);
        job = &fn; nitems = n; per = (n + th.size() - 1) / th.size(); pending = (int)th.size(); gen++;
        cv_go.notify_all();
        cv_done.wait(lk, [&] { return pending == 0; });
    }
};

// copy threads per context when GEOSRAD_HOST_THREADS is not set: the host's hardware threads shared out among the ranks of the node (the
// launchers' node-local size; 96 ranks x 8 copy threads would oversubscribe a host), at most 8, at least 1
// CPUs this process may use at once: the hardware threads it is allowed on, capped by the cgroup's CPU quota (a container that sees 256
// hardware threads may own 16 of them)
static int usable_cpus()
{
    long n = (long)std::thread::hardware_concurrency();
    cpu_set_t m;
    if (sched_getaffinity(0, sizeof m, &m) == 0 && CPU_COUNT(&m) > 0) n = CPU_COUNT(&m);
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {          // cgroup v2: "<quota> <period>" or "max <period>"
        long q = 0, per = 0;
        if (fscanf(f, "%ld %ld", &q, &per) == 2 && q > 0 && per > 0) { const long c = (q + per - 1) / per; if (c < n) n = c; }
        fclose(f);
    }
    return (int)(n < 1 ? 1 : n);
}

static int default_host_threads()
{
    unsigned hw = (unsigned)usable_cpus();
    if (hw == 0) hw = 8;
    long ranks = 1;
    static const char *vars[] = {"OMPI_COMM_WORLD_LOCAL_SIZE", "MV2_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS", "PMI_LOCAL_SIZE", "SLURM_NTASKS_PER_NODE"};
    for (const char *v : vars) {
        const char *e = getenv(v);
        if (!e || !*e) continue;
        char *end = nullptr;
        const long r = strtol(e, &end, 10);
        if (end != e && r >= 1) { ranks = r; break; }
    }
    long n = (long)hw / ranks;
    return (int)(n < 1 ? 1 : (n > 8 ? 8 : n));
}

// ---------------------------------------------------------------------------------------------------
struct geosrad_ctx {
    int device = 0, real_kind = 4, chunk = 131072;
    bool sorad_col_path = false;    // Chou-Suarez sorad passes: HBM scratch planes, lane = column (default) | GEOSRAD_SORAD_PATH=col: on chip
    bool lw_cols_path = false;      // RRTMG_LW band sweeps: parked cells in HBM (default) | GEOSRAD_LW_PATH=cols: on-chip intermediates
    bool lw_split_path = false;     //                       | GEOSRAD_LW_PATH=split: k-distribution layer-parallel (k_lw_cells) + recurrences (k_lw_sweep)
    int sw_path = 2;                // RRTMG_SW band sweeps: k_sw_reform (2, default) | GEOSRAD_SW_PATH=bands: k_sw_bands, the first mapping (0)
    int overcast = 0;               // GEOSRAD_OVERCAST_IRRAD | GEOSRAD_OVERCAST_SORAD: the Chou-Suarez schemes as built with -DOVERCAST
    std::string last_error;
    hipStream_t stream = nullptr;   // internal stream of the host-pointer entry points
    // optional per-kernel timing with HIP events recorded on the launch stream (geosrad_profile*)
    bool profiling = false;
    struct Span { int kid; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> evpool;
    double prof_ms[16] = {0};
    long prof_n[16] = {0};
    hipEvent_t getev()
    {
        hipEvent_t e = nullptr;
        if (!evpool.empty()) { e = evpool.back(); evpool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    }
    int roctx_depth = 0;
    void span_begin(int kid, hipStream_t st)
    {
        if (roctx_api().push && kid >= 0 && kid < 14) {
            for (int k = 0; k < 3; k++) if (ROCTX_NAMES[kid][k]) { roctx_api().push(ROCTX_NAMES[kid][k]); roctx_depth++; }
        }
        if (!profiling) return;
        Span s{kid, getev(), getev()};
        (void)hipEventRecord(s.a, st);
        spans.push_back(s);
    }
    void span_end(hipStream_t st)
    {
        if (profiling && !spans.empty()) (void)hipEventRecord(spans.back().b, st);
        for (; roctx_depth > 0; roctx_depth--) roctx_api().pop();
    }
    void prof_collect()
    {
        for (auto &s : spans) {
            float ms = 0;
            if (hipEventSynchronize(s.b) == hipSuccess && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { prof_ms[s.kid] += ms; prof_n[s.kid]++; }
            evpool.push_back(s.a); evpool.push_back(s.b);
        }
        spans.clear();
    }
    int fail(int code, const std::string &msg) { last_error = msg; return code; }
    int hip_rc(const char *what, hipError_t e) { return e == hipSuccess ? GEOSRAD_OK : fail(GEOSRAD_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }

    // ---- host-pointer entry points: chunk pipeline --------------------------------------------------------------------------
    // The reference interface hands over host arrays, Fortran (ncol, rows): column index fastest.  A batch goes through the GPU in
    // chunks of `host_chunk` columns: copy threads gather a chunk's rows into a pinned staging slot, one DMA moves the slot to HBM,
    // the solver runs on it, one DMA brings the outputs back and the threads scatter them - on three streams and two slots, so that
    // the gathering of chunk k+1, the transfers and the kernels of chunk k and the scattering of chunk k-1 overlap.
    struct PipeArr { const void *src; void *dst; size_t rows, ebytes; size_t off; };      // src: copied in; dst: copied back (either may be null)
    int host_chunk = 16384, host_chunk_default = 16384, host_threads = default_host_threads();
    std::unique_ptr<CopyPool> copy_pool;
    size_t host_ld = 0;             // leading dimension (columns) of the caller's arrays when the call covers a shard of them (multi-device context); 0: ncol
    bool host_nt = true;            // non-temporal stores into the staging slots (GEOSRAD_HOST_NT=0: plain memcpy)
    // three staging slots, results copied back to the caller two chunks behind the one being gathered: the host thread then never waits
    // for the GPU in steady state and the H2D engine always has the next chunk queued (two slots in lock-step left it idle while the
    // host gathered: 4.25 instead of 3.4 ms per 16 384-column chunk)
    static constexpr int PIPE_SLOTS = 3, PIPE_LAG = 2;
    static constexpr int PIPE_FLAGGED = -77;      // host_pipeline: a chunk came back with the device error word set (the caller's check() names it)
    char *pipe_pin[PIPE_SLOTS][2] = {};      // [slot][0 = to the device, 1 = from the device]
    DevBuf<> pipe_dev[PIPE_SLOTS];           // all of one size
    size_t pipe_pin_bytes[2] = {0, 0};       // [0] holds a chunk's inputs, [1] its outputs only
    uint32_t *pipe_err = nullptr;            // pinned: the solver's device error word as of each slot's copy-back
    hipStream_t pipe_h2d = nullptr, pipe_d2h = nullptr;
    hipEvent_t pipe_ev[PIPE_SLOTS][3] = {};      // per slot: h2d, compute, d2h done
    void pipe_release()
    {
        for (int s = 0; s < PIPE_SLOTS; s++) {
            for (int d = 0; d < 2; d++) if (pipe_pin[s][d]) { (void)hipHostFree(pipe_pin[s][d]); pipe_pin[s][d] = nullptr; }
            pipe_dev[s].release();
            for (int e = 0; e < 3; e++) if (pipe_ev[s][e]) { (void)hipEventDestroy(pipe_ev[s][e]); pipe_ev[s][e] = nullptr; }
        }
        if (pipe_h2d) { (void)hipStreamDestroy(pipe_h2d); pipe_h2d = nullptr; }
        if (pipe_d2h) { (void)hipStreamDestroy(pipe_d2h); pipe_d2h = nullptr; }
        if (pipe_err) { (void)hipHostFree(pipe_err); pipe_err = nullptr; }
        pipe_pin_bytes[0] = pipe_pin_bytes[1] = 0;
    }
    // a row into the write-once staging memory with non-temporal stores: no read-for-ownership of the destination lines (the rows,
    // 64 KB each, are below the size from which memcpy streams by itself)
    static void copy_stream(char *dst, const char *src, size_t n)
    {
        typedef long long v2a __attribute__((vector_size(16), aligned(16)));
        typedef long long v2u __attribute__((vector_size(16), aligned(1)));
        size_t head = (16 - ((uintptr_t)dst & 15)) & 15;
        if (head > n) head = n;
        memcpy(dst, src, head); dst += head; src += head; n -= head;
        const size_t nv = n / 16;
        for (size_t i = 0; i < nv; i++) __builtin_nontemporal_store(*(const v2u *)(src + 16 * i), (v2a *)(dst + 16 * i));
        memcpy(dst + 16 * nv, src + 16 * nv, n - 16 * nv);
    }
    // rows of `arrs` (a chunk's nc columns starting at c0 of ncol) between the caller's arrays and a staging slot, on copy threads
    void pipe_copy(std::vector<PipeArr> &arrs, char *slot, size_t slot_base, int ncol, int c0, int nc, bool to_slot)
    {
        struct Item { const PipeArr *a; size_t row; };
        std::vector<Item> items;
        for (auto &a : arrs) {
            if (to_slot ? !a.src : !a.dst) continue;
            for (size_t r = 0; r < a.rows; r++) items.push_back({&a, r});
        }
        auto work = [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                const PipeArr &a = *items[i].a;
                const size_t r = items[i].row;
                char *sl = slot + (a.off - slot_base) + r * (size_t)nc * a.ebytes;      // a chunk's arrays are dense: leading dimension nc
                if (to_slot) {
                    if (host_nt) copy_stream(sl, (const char *)a.src + (r * (size_t)ncol + (size_t)c0) * a.ebytes, (size_t)nc * a.ebytes);
                    else memcpy(sl, (const char *)a.src + (r * (size_t)ncol + (size_t)c0) * a.ebytes, (size_t)nc * a.ebytes);
                } else memcpy((char *)a.dst + (r * (size_t)ncol + (size_t)c0) * a.ebytes, sl, (size_t)nc * a.ebytes);
            }
            if (to_slot && host_nt) std::atomic_thread_fence(std::memory_order_seq_cst);      // the streamed rows are visible before the DMA reads them
        };
        size_t bytes = 0;
        for (auto &it : items) bytes += (size_t)nc * it.a->ebytes;
        const int nt = bytes < ((size_t)4 << 20) ? 1 : host_threads;
        if (nt <= 1) { work(0, items.size()); return; }
        if (!copy_pool || copy_pool->size() != nt) copy_pool.reset(new CopyPool(nt));
        const std::function<void(size_t, size_t)> fn = work;
        copy_pool->run(items.size(), fn);
    }
    // arrs must be ordered: copied in only, copied both ways, copied back only.  run(stream, nc, c0, device base of the slot) enqueues
    // the solver for one chunk whose arrays lie at dev + a.off, dense with leading dimension nc (slots are sized for
    // cn = min(ncol, host_chunk) columns).  err_dev: the solver's device-side input-assertion word (null: the scheme has none); it
    // comes back with every chunk's outputs, and a chunk whose word is set is NOT scattered into the caller's arrays - the pipeline
    // drains and returns PIPE_FLAGGED for the caller's check() to turn into the reference's message (the reference stops before it
    // computes anything; here the chunks before the offending one have been delivered).
    int host_pipeline(int ncol, std::vector<PipeArr> &arrs, const std::function<int(hipStream_t, int, int, char *, int)> &run,
                      const uint32_t *err_dev = nullptr)
    {
        const int cn = ncol < host_chunk ? ncol : host_chunk;
        const int ld_host = host_ld ? (int)host_ld : ncol;
        // a chunk's arrays lie dense in its slot (leading dimension = the chunk's columns): the offsets are those of the chunk's own size, so
        // that a small chunk moves only its own bytes
        size_t in_end = 0, out_begin = 0, total = 0;
        auto layout = [&](int nc_) {
            size_t off = 0; in_end = 0; out_begin = (size_t)-1;
            for (auto &a : arrs) {
                a.off = off;
                if (a.dst && out_begin == (size_t)-1) out_begin = off;
                off += (a.rows * (size_t)nc_ * a.ebytes + 255) & ~(size_t)255;
                if (a.src) in_end = off;
            }
            if (out_begin == (size_t)-1) out_begin = off;
            total = off;
        };
        layout(cn);
        const size_t total_max = total, in_bytes_max = in_end, out_bytes_max = total - out_begin;
        if (!pipe_h2d) {
            HIPCHK(hipStreamCreateWithFlags(&pipe_h2d, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&pipe_d2h, hipStreamNonBlocking));
            for (int s = 0; s < PIPE_SLOTS; s++) for (int e = 0; e < 3; e++) HIPCHK(hipEventCreateWithFlags(&pipe_ev[s][e], hipEventDisableTiming));
            HIPCHK(hipHostMalloc((void **)&pipe_err, PIPE_SLOTS * sizeof(uint32_t), hipHostMallocDefault));
        }
        const size_t pipe_dev_bytes = pipe_dev[0].bytes;
        if (total_max > pipe_dev_bytes || in_bytes_max > pipe_pin_bytes[0] || out_bytes_max > pipe_pin_bytes[1]) {
            HIPCHK(hipDeviceSynchronize());
            const size_t want_dev = total_max > pipe_dev_bytes ? total_max : pipe_dev_bytes;
            const size_t want_pin[2] = {in_bytes_max > pipe_pin_bytes[0] ? in_bytes_max : pipe_pin_bytes[0],
                                        out_bytes_max > pipe_pin_bytes[1] ? out_bytes_max : pipe_pin_bytes[1]};
            pipe_pin_bytes[0] = pipe_pin_bytes[1] = 0;      // a failure below leaves "nothing allocated", not stale sizes
            for (int s = 0; s < PIPE_SLOTS; s++) {
                pipe_dev[s].release();
                for (int d = 0; d < 2; d++) if (pipe_pin[s][d]) { (void)hipHostFree(pipe_pin[s][d]); pipe_pin[s][d] = nullptr; }
            }
            for (int s = 0; s < PIPE_SLOTS; s++) {
                if (pipe_dev[s].resize(want_dev) != hipSuccess) { pipe_release(); return fail(GEOSRAD_ENOMEM, "hipMalloc of the host-API staging slot failed"); }
                for (int d = 0; d < 2; d++)
                    if (hipHostMalloc((void **)&pipe_pin[s][d], want_pin[d] ? want_pin[d] : 256, hipHostMallocDefault) != hipSuccess) {
                        pipe_release();
                        return fail(GEOSRAD_ENOMEM, "hipHostMalloc of the pinned host-API staging slot failed");
                    }
            }
            pipe_pin_bytes[0] = want_pin[0]; pipe_pin_bytes[1] = want_pin[1];
        }
        for (int s = 0; s < PIPE_SLOTS; s++) pipe_err[s] = 0;
        bool input_error = false;
        // chunk boundaries.  (Small first chunks that double up to cn - so that the first transfer starts before 171 / 265 MB have been
        // gathered - were measured: 58.3 against 56.7 ms per RRTMG_LW + RRTMG_SW call pair of 97 200 columns; the call is bound by the
        // H2D transfer itself, 2.59 GB at the box's 57.5 GB/s = 45 ms, profiles/r04_host_api.md.)
        std::vector<int> cstart;
        for (int c = 0; c < ncol; c += cn) cstart.push_back(c);
        cstart.push_back(ncol);
        const int nchunks = (int)cstart.size() - 1;
        const bool trace = getenv("GEOSRAD_HOST_TRACE") != nullptr;
        auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        double t_g = 0, t_s = 0, t_w = 0, t_e = 0;
        const double t_begin = now();
        for (int k = 0; k < nchunks + PIPE_LAG; k++) {
            if (k < nchunks) {
                const int s = k % PIPE_SLOTS, c0 = cstart[k], nc = cstart[k + 1] - c0;
                double t0 = now();
                if (k >= PIPE_SLOTS) HIPCHK(hipEventSynchronize(pipe_ev[s][0]));   // the slot's previous transfer has left the staging memory
                double t1 = now(); t_w += t1 - t0;
                layout(nc);
                const size_t in_bytes = in_end, out_bytes = total - out_begin;
                pipe_copy(arrs, pipe_pin[s][0], 0, ld_host, c0, nc, true);
                t0 = now(); t_g += t0 - t1;
                if (k >= PIPE_SLOTS) HIPCHK(hipStreamWaitEvent(pipe_h2d, pipe_ev[s][2], 0));   // ... and its previous chunk has been copied out of the device slot
                if (in_bytes) HIPCHK(hipMemcpyAsync(pipe_dev[s], pipe_pin[s][0], in_bytes, hipMemcpyHostToDevice, pipe_h2d));
                HIPCHK(hipEventRecord(pipe_ev[s][0], pipe_h2d));
                HIPCHK(hipStreamWaitEvent(stream, pipe_ev[s][0], 0));
                const int rc = run(stream, nc, c0, pipe_dev[s], cn);
                if (rc) { (void)hipDeviceSynchronize(); return rc; }
                HIPCHK(hipEventRecord(pipe_ev[s][1], stream));
                HIPCHK(hipStreamWaitEvent(pipe_d2h, pipe_ev[s][1], 0));
                if (out_bytes) HIPCHK(hipMemcpyAsync(pipe_pin[s][1], pipe_dev[s] + out_begin, out_bytes, hipMemcpyDeviceToHost, pipe_d2h));
                if (err_dev) HIPCHK(hipMemcpyAsync(&pipe_err[s], err_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, pipe_d2h));
                HIPCHK(hipEventRecord(pipe_ev[s][2], pipe_d2h));
                t_e += now() - t0;
            }
            if (k >= PIPE_LAG && k - PIPE_LAG < nchunks) {
                const int j = k - PIPE_LAG, s = j % PIPE_SLOTS, c0 = cstart[j], nc = cstart[j + 1] - c0;
                double t0 = now();
                HIPCHK(hipEventSynchronize(pipe_ev[s][2]));
                double t1 = now(); t_w += t1 - t0;
                if (err_dev && pipe_err[s]) { input_error = true; break; }      // this chunk (or one enqueued behind it) tripped an input assertion
                layout(nc);
                pipe_copy(arrs, pipe_pin[s][1], out_begin, ld_host, c0, nc, false);
                t_s += now() - t1;
            }
        }
        if (input_error) { HIPCHK(hipDeviceSynchronize()); return PIPE_FLAGGED; }
        if (trace)
            fprintf(stderr, "geosrad host pipeline: %d columns, %d chunks of %d, %.1f MB in / %.1f MB out per chunk: total %.1f ms = gather %.1f + "
                            "scatter %.1f + enqueue %.1f + waiting for the GPU %.1f\n", ncol, nchunks, cn, in_bytes_max / 1e6, out_bytes_max / 1e6,
                    now() - t_begin, t_g, t_s, t_e, t_w);
        return GEOSRAD_OK;
    }
    virtual ~geosrad_ctx() { pipe_release(); }
    virtual int init() = 0;
    virtual int set_tables_lw(const void *blob, size_t n) = 0;
    virtual int set_inhomogeneity(int ih, const void *blob, size_t n) = 0;
    virtual int set_corr(const double *adl, const double *rdl) = 0;
    virtual size_t workspace_bytes() const = 0;
    // RATS diagnostics of LW_Driver (GEOS_IrradGridComp.F90:3405-3468): total-sky profiles with one gas removed, per gas
    struct LwRats { int n; int gas[GEOSRAD_RAT_NGAS]; void *uflx, *dflx, *duflx_dTs; };      // outputs [n][nlay+1][ncol]
    // The `_dev` entry points: device pointers belong to ONE device, so a context that is not a single device's refuses them.  Arguments as
    // in include/geosrad.h after the stream (solvers: as their *_host twin; lw_dev ends dbg_taug, dbg_pfracs, rats).
    int nodev(const char *what) { return fail(GEOSRAD_EINVAL, std::string(what) + ": device-pointer entry points need a single-device context (geosrad_create)"); }
    using In = const void *const *; using Out = void *const *;
    virtual int lw_dev(hipStream_t, int, int, int, In, int, int, int, int, int, int32_t *, Out, const int32_t *, void *, void *, const LwRats *)
    { return nodev("geosrad_rrtmg_lw_dev"); }
    virtual int lw_host(int ncol, int nlay, int dudTs, const void *const *in, int iceflg, int liqflg, int dyofyr, int cloudLM,
                        int cloudMH, int32_t *clearCounts, void *const *out, const int32_t *band_output, void *taug,
                        void *pfracs) = 0;
    virtual int mcica_host(int ncol, int nsubcol, int nlay, const void *zmid, const void *alat, int doy, const void *play,
                           const void *cldfrac, const void *ciwp, const void *clwp, double cwp_tiny, const int32_t *so,
                           int32_t *cldy, void *ciwp_s, void *clwp_s) = 0;
    virtual int mcica_dev(hipStream_t, int, int, int, const void *, const void *, int, const void *, const void *, const void *, const void *, double,
                          const int32_t *, int32_t *, void *, void *) { return nodev("geosrad_mcica_dev"); }
    virtual int check(hipStream_t st, int which = -1) = 0;      // which: -1 either solver's assertions, 0 RRTMG_LW (+ McICA), 1 RRTMG_SW
    virtual int set_tables_sw(const void *blob, size_t n) = 0;
    virtual int set_tables_chou_lw(const void *blob, size_t n) = 0;
    virtual int set_tables_chou_sw(const void *blob, size_t n) = 0;
    // na_out: the aerosol-free fluxes of the same call (GEOSRAD_SONA_*), null from the entry points without them
    virtual int sorad_dev(hipStream_t, int, int, int, In, double, int, int, const void *, const void *, Out, int, Out /*na_out*/)
    { return nodev("geosrad_sorad_dev"); }
    virtual int sorad_host(int m, int np, int nb, const void *const *in, double co2, int ict, int icb, const void *hk_uv, const void *hk_ir,
                           void *const *out, int do_drfband, void *const *na_out) = 0;
    virtual int irrad_dev(hipStream_t, int, int, In, double, int, int, int, int, int, int, Out, Out) { return nodev("geosrad_irrad_dev"); }
    virtual int irrad_host(int m, int np, const void *const *in, double co2, int trace, int ict, int icb, int ns, int na, int nb,
                           void *const *aer, void *const *out) = 0;
    virtual int sw_dev(hipStream_t, int, int, double, double, int, In, int, int, int, int, int, int, int, int32_t *, Out, int, const void *, const void *,
                       const void *, Out, void *) { return nodev("geosrad_rrtmg_sw_dev"); }
    virtual int lw_driver_dev(hipStream_t, const LwdCall &) { return nodev("geosrad_lw_driver_rrtmg_dev"); }
    virtual int sw_driver_dev(hipStream_t, const SwdCall &C) { return nodev(C.lit ? "geosrad_sw_driver_rrtmg_lit_dev" : "geosrad_sw_driver_rrtmg_dev"); }
    virtual int sw_driver_chou_dev(hipStream_t, const SwcCall &C) { return nodev(C.lit ? "geosrad_sw_driver_chou_lit_dev" : "geosrad_sw_driver_chou_dev"); }
    virtual int lw_chou_post_dev(hipStream_t, int, int, In, Out) { return nodev("geosrad_lw_chou_post_dev"); }
    virtual int lw_driver_chou_dev(hipStream_t, int, int, In, const double *, int, int, int, int, Out) { return nodev("geosrad_lw_driver_chou_dev"); }
    virtual int lw_update_flx_dev(hipStream_t, int, int, int, int, int, double, In, Out) { return nodev("geosrad_lw_update_flx_dev"); }
    virtual int lw_update_rats_dev(hipStream_t, int, int, int, In, Out) { return nodev("geosrad_lw_update_rats_dev"); }
    virtual int lw_update_bands_dev(hipStream_t, int, const int32_t *, const double *, const double *, double, const void *, const void *, const void *,
                                    const void *, void *, void *) { return nodev("geosrad_lw_update_bands_dev"); }
    virtual int sw_update_export_dev(hipStream_t, int, int, int, In, Out) { return nodev("geosrad_sw_update_export_dev"); }
    virtual int sw_update_obio_dev(hipStream_t, int, int, int, const double *, const double *, const int32_t *, const void *, const void *, const void *,
                                   void *, void *) { return nodev("geosrad_sw_update_obio_dev"); }
    virtual int sw_update_surface_dev(hipStream_t, int, int, double, In, Out) { return nodev("geosrad_sw_update_surface_dev"); }
    virtual int sw_update_clouds_dev(hipStream_t, int, int, int, int, double, const double *, In, Out) { return nodev("geosrad_sw_update_clouds_dev"); }
    virtual int sw_update_cldhb_dev(hipStream_t, int, int, int, int, int, const double *, In, Out) { return nodev("geosrad_sw_update_cldhb_dev"); }
    virtual int rad_tendencies_dev(hipStream_t, int, int, double, double, In, Out) { return nodev("geosrad_rad_tendencies_dev"); }
    virtual int sw_host(int ncol, int nlay, double scon, double adjes, int isolvar, const void *const *in, int iceflg, int liqflg,
                        int dyofyr, int iaer, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *const *out,
                        int do_drfband, const void *bndscl, const void *indsolvar, const void *solcycfrac,
                       void *const *dbg, void *radval) = 0;
    virtual int lit_index_dev(hipStream_t, int, const void *, int32_t *, int32_t *, int32_t *, int *) { return nodev("geosrad_lit_index_dev"); }
    virtual int lit_pack_dev(hipStream_t, int, int, int, const int32_t *, const int32_t *, const void *, void *) { return nodev("geosrad_lit_pack_dev"); }
    virtual int lit_unpack_dev(hipStream_t, int, int, int, const int32_t *, const void *, void *, int, double) { return nodev("geosrad_lit_unpack_dev"); }
    // gettau (include/geosrad_gettau.h): one record for the three routines, shared by the `_dev` and the host-pointer variant
    struct GtCall {
        int kind;                       // 0 getvistau, 1 getnirtau, 2 getirtau
        int ib, ncol, nlevs, ict, icb;
        double grav;
        const void *cosz, *dp, *fcld, *reff, *hyd;
        void *out[4];                   // taubeam, taudiff, asycl, ssacl | taudiag, tcldlyr, enn, -
        const char *name() const { return kind == 0 ? "geosrad_getvistau" : kind == 1 ? "geosrad_getnirtau" : "geosrad_getirtau"; }
    };
    // the argument rules of include/geosrad_gettau.h, the same for every kind of context
    int gettau_check(const GtCall &C)
    {
        const std::string who = C.name();
        if (C.ncol <= 0 || C.nlevs < 1) return fail(GEOSRAD_EINVAL, who + ": ncol must be positive and nlevs at least 1");
        if (C.kind == 1 && (C.ib < 1 || C.ib > 3)) return fail(GEOSRAD_EINVAL, who + ": ib must be in 1..3");
        if (C.kind == 2 && (C.ib < 1 || C.ib > 10)) return fail(GEOSRAD_EINVAL, who + ": ib must be in 1..10");
        if (C.kind != 2 && C.ict != 0 && !(1 <= C.ict && C.ict <= C.icb && C.icb <= C.nlevs + 1))
            return fail(GEOSRAD_EINVAL, who + ": ict / icb must satisfy 1 <= ict <= icb <= nlevs + 1 (or ict = 0: the in-cloud mode)");
        if (!C.out[0] && !C.out[1] && !C.out[2] && !C.out[3]) return fail(GEOSRAD_EINVAL, who + ": every output is NULL");
        if (!C.dp || !C.fcld || !C.reff || !C.hyd) return fail(GEOSRAD_EINVAL, who + ": null input array");
        if (C.kind != 2 && C.ict != 0 && C.out[0] && !C.cosz) return fail(GEOSRAD_EINVAL, who + ": taubeam of the overlap mode needs cosz");
        return GEOSRAD_OK;
    }
    virtual int gettau_dev(hipStream_t, const GtCall &C) { return nodev(C.name()); }
    virtual int gettau_host(const GtCall &C) = 0;
    virtual int lw_cloud_diag_dev(hipStream_t, int, int, double, double, double, In, Out) { return nodev("geosrad_lw_cloud_diag_dev"); }
    // the satellite simulator's ISCCP path (include/geosrad_satsim.h): one record per routine, shared by the `_dev` and the host variant
    struct ScopsCall {
        int npoints, nlev, ncol, overlap;
        int32_t *seed;
        const void *cc, *conv;
        void *frac_out;                 // bytes (`_dev`) or reals (host)
    };
    enum IcIn { IC_PFULL, IC_PHALF, IC_QV, IC_CC, IC_CONV, IC_DTAU_S, IC_DTAU_C, IC_SKT, IC_AT, IC_DEM_S, IC_DEM_C, IC_NIN };
    enum IcOut { ICO_FQ, ICO_TCA, ICO_PTOP, ICO_TAU, ICO_ALB, ICO_TB, ICO_TBCLR, ICO_BOXTAU, ICO_BOXPTOP, ICO_NOUT };
    struct IcarusCall {
        int npoints, nlev, ncol, top_height, top_height_direction, overlap;
        double emsfc_lw;
        const int32_t *sunlit;
        const void *in[IC_NIN];
        const void *frac_out;           // bytes (`_dev`) or reals (host)
        void *out[ICO_NOUT];
        // geosrad_isccp_dev only: the fields are GEOS's (FCLD / CCA unscaled, in[IC_PHALF] = PLE(0:LM), CCA / DTAU_C / DEM_C may be null),
        // SCOPS runs first on the unscaled fractions into the context's mask with `seed`, the outputs are COSP's, SGFCLD on request
        bool cosp = false;
        int32_t *seed = nullptr;
        void *sgfcld = nullptr;
        bool scops_only = false;        // geosrad_cosp_dev with neither an ISCCP output nor MODIS wanted: SCOPS, the seeds and SGFCLD only
    };
    // the argument rules of include/geosrad_satsim.h, the same for every kind of context
    int satsim_check(const char *who, int npoints, int nlev, int ncol, int overlap, int top_height, int top_height_direction)
    {
        const std::string w = who;
        if (npoints < 1) return fail(GEOSRAD_EINVAL, w + ": npoints must be positive");
        if (nlev < 2) return fail(GEOSRAD_EINVAL, w + ": nlev must be at least 2");
        // k_icarus_stats counts a point's sub-columns per cloud type in 16 bits (GEOS: Ncolumns <= 30, GEOS_SatsimGridComp.F90:3057)
        if (ncol < 1 || ncol > 65535) return fail(GEOSRAD_EINVAL, w + ": ncol must be in 1..65535");
        if (overlap < 1 || overlap > 3) return fail(GEOSRAD_EINVAL, w + ": overlap must be 1, 2 or 3");
        if (top_height < 1 || top_height > 3) return fail(GEOSRAD_EINVAL, w + ": top_height must be 1, 2 or 3");
        if (top_height_direction < 1 || top_height_direction > 2) return fail(GEOSRAD_EINVAL, w + ": top_height_direction must be 1 or 2");
        return GEOSRAD_OK;
    }
    int scops_check(const ScopsCall &C)
    {
        if (const int rc = satsim_check("geosrad_scops", C.npoints, C.nlev, C.ncol, C.overlap, 1, 1)) return rc;
        if (!C.seed || !C.cc || !C.conv || !C.frac_out) return fail(GEOSRAD_EINVAL, "geosrad_scops: null array");
        return GEOSRAD_OK;
    }
    int icarus_check(const IcarusCall &C)
    {
        const char *who = C.cosp ? "geosrad_isccp_dev" : "geosrad_icarus";
        if (const int rc = satsim_check(who, C.npoints, C.nlev, C.ncol, C.overlap, C.top_height, C.top_height_direction)) return rc;
        for (int k = 0; k < IC_NIN; k++)
            if (!C.in[k] && !(C.cosp && (k == IC_CONV || k == IC_DTAU_C || k == IC_DEM_C))) return fail(GEOSRAD_EINVAL, std::string(who) + ": null input array");
        if (!C.sunlit || (C.cosp ? !C.seed : !C.frac_out)) return fail(GEOSRAD_EINVAL, std::string(who) + ": null input array");
        return GEOSRAD_OK;
    }
    virtual int scops_dev(hipStream_t, const ScopsCall &) { return nodev("geosrad_scops_dev"); }
    virtual int scops_host(const ScopsCall &) = 0;
    virtual int icarus_dev(hipStream_t, const IcarusCall &C) { return nodev(C.cosp ? "geosrad_isccp_dev" : "geosrad_icarus_dev"); }
    virtual int icarus_host(const IcarusCall &) = 0;
    virtual int cosp_seeds_dev(hipStream_t, int, const void *, int32_t *) { return nodev("geosrad_cosp_seeds_dev"); }
    // the MISR simulator (include/geosrad_misr_modis.h): one record, shared by the `_dev` and the host variant
    enum MisrIn { MI_ZFULL, MI_AT, MI_DTAU_S, MI_DTAU_C, MI_NIN };
    enum MisrOut { MIO_FQ, MIO_DIST, MIO_ZTOP, MIO_AREA, MIO_NOUT };
    struct MisrCall {
        int npoints, nlev, ncol;
        double missing_value;
        const int32_t *sunlit;
        const void *in[MI_NIN];
        const void *frac_out;           // bytes (`_dev`) or reals (host)
        void *out[MIO_NOUT];
        // whether the points of this record begin / end the caller's: the pattern matcher works on the call's first point and a dark
        // last point of the call gets missing_value in MISR_mean_ztop; a chunk or a shard in the middle has neither
        bool first = true, last = true;
    };
    int misr_check(const MisrCall &C)
    {
        if (const int rc = satsim_check("geosrad_misr", C.npoints, C.nlev, C.ncol, 1, 1, 1)) return rc;
        // MISR_simulator.f:294-313: with one sub-column the pattern matcher couples neighbouring points in one serial scan over the grid
        if (C.ncol == 1) return fail(GEOSRAD_EINVAL, "geosrad_misr: ncol must be at least 2 (ncol = 1 is the reference's serial scan over the points)");
        for (int k = 0; k < MI_NIN; k++)
            if (!C.in[k]) return fail(GEOSRAD_EINVAL, "geosrad_misr: null input array");
        if (!C.sunlit || !C.frac_out) return fail(GEOSRAD_EINVAL, "geosrad_misr: null input array");
        return GEOSRAD_OK;
    }
    virtual int misr_dev(hipStream_t, const MisrCall &) { return nodev("geosrad_misr_dev"); }
    virtual int misr_host(const MisrCall &) = 0;
    // the MODIS simulator: one record, shared by the `_dev` and the host variant
    enum ModisIn { MDI_T, MDI_P, MDI_PH, MDI_DTAU_S, MDI_DTAU_C, MDI_MR, MDI_REFF = MDI_MR + 4, MDI_BOXTAU = MDI_REFF + 4, MDI_BOXPTOP, MDI_NIN };
    enum ModisOut { MDO_MEAN, MDO_HIST, MDO_PHASE, MDO_CTP, MDO_TAU, MDO_SIZE, MDO_NOUT };
    struct ModisCall {
        int npoints, nlev, ncol;
        const int32_t *sunlit;
        const void *in[MDI_NIN];        // dtau_c and the convective contents and radii may be null (zero); boxtau is not read
        const void *frac_out;           // bytes (`_dev`) or reals (host)
        void *out[MDO_NOUT];
        bool geos = false;              // geosrad_cosp_dev: in[MDI_PH] is PLE (npoints,0:lm), the water contents are clamped at 0
    };
    static bool modis_optional(int k) { return k == MDI_DTAU_C || k == MDI_MR + 2 || k == MDI_MR + 3 || k == MDI_REFF + 2 || k == MDI_REFF + 3 || k == MDI_BOXTAU; }
    int modis_check(const ModisCall &C)
    {
        if (const int rc = satsim_check("geosrad_modis", C.npoints, C.nlev, C.ncol, 1, 1, 1)) return rc;
        for (int k = 0; k < MDI_NIN; k++)
            if (!C.in[k] && !modis_optional(k)) return fail(GEOSRAD_EINVAL, "geosrad_modis: null input array");
        if (!C.sunlit || !C.frac_out) return fail(GEOSRAD_EINVAL, "geosrad_modis: null input array");
        return GEOSRAD_OK;
    }
    virtual int modis_dev(hipStream_t, const ModisCall &) { return nodev("geosrad_modis_dev"); }
    virtual int modis_host(const ModisCall &) = 0;
    // geosrad_cosp_dev: the record of geosrad_isccp_dev and what MISR and MODIS need beside it
    struct CospCall {
        IcarusCall ic;
        const void *zle, *qltot, *qitot, *rdfl, *rdfi;
        void *misr[MIO_NOUT], *modis[2];
    };
    virtual int cosp_dev(hipStream_t, const CospCall &) { return nodev("geosrad_cosp_dev"); }
    // the lidar simulator (include/geosrad_lidar.h): one record, shared by the `_dev` and the host variant
    enum LidarIn { LDI_P, LDI_T, LDI_PRESF, LDI_PPLAY, LDI_MR, LDI_REFF = LDI_MR + 4, LDI_LAND = LDI_REFF + 4, LDI_NIN };
    enum LidarOut { LDO_CLD, LDO_LAYER, LDO_CFAD, LDO_PARASOL, LDO_PMOL, LDO_BETA, LDO_TAU, LDO_REFL, LDO_NOUT };
    struct LidarCall {
        int npoints, nlev, ncol, ice_type;
        const void *in[LDI_NIN];        // the convective contents and radii may be null (zero)
        const void *frac_out;           // bytes (`_dev`) or reals (host)
        void *out[LDO_NOUT];
        bool geos = false;              // geosrad_cosp_lidar_dev: in[LDI_PRESF] and in[LDI_PPLAY] are PLE (npoints,0:lm), in[LDI_LAND] is FROCEAN, the contents are clamped at 0
    };
    static bool lidar_optional(int k) { return k == LDI_MR + 2 || k == LDI_MR + 3 || k == LDI_REFF + 2 || k == LDI_REFF + 3; }
    int lidar_check(const LidarCall &C)
    {
        if (const int rc = satsim_check("geosrad_lidar", C.npoints, C.nlev, C.ncol, 1, 1, 1)) return rc;
        // lidar_simulator.F90:206-241 sets the ice coefficients under ice_type = 0 and = 1 only
        if (C.ice_type != 0 && C.ice_type != 1) return fail(GEOSRAD_EINVAL, "geosrad_lidar: ice_type must be 0 or 1");
        for (int k = 0; k < LDI_NIN; k++)
            if (!C.in[k] && !lidar_optional(k)) return fail(GEOSRAD_EINVAL, "geosrad_lidar: null input array");
        if (!C.frac_out) return fail(GEOSRAD_EINVAL, "geosrad_lidar: null input array");
        return GEOSRAD_OK;
    }
    virtual int lidar_dev(hipStream_t, const LidarCall &) { return nodev("geosrad_lidar_dev"); }
    virtual int lidar_host(const LidarCall &) = 0;
    // geosrad_cosp_lidar_dev: the record of geosrad_cosp_dev and what the lidar needs beside it
    struct CospLidarCall {
        CospCall cosp;
        const void *frocean;
        int ice_type;
        void *lidar[5];                 // clcalipso, cldlayer, cfad_sr, parasolrefl, lidarpmol
    };
    virtual int cosp_lidar_dev(hipStream_t, const CospLidarCall &) { return nodev("geosrad_cosp_lidar_dev"); }
    // the radar simulator's front end (include/geosrad_radar.h): one record an entry point, shared by the `_dev` and the host variant
    struct PrecScopsCall {
        int npoints, nlev, ncol;
        const void *ls, *cv;
        const void *frac_out;           // bytes (`_dev`) or reals (host)
        void *prec_frac;                // the same
    };
    int prec_scops_check(const PrecScopsCall &C)
    {
        if (const int rc = satsim_check("geosrad_prec_scops", C.npoints, C.nlev, C.ncol, 1, 1, 1)) return rc;
        if (!C.ls || !C.cv || !C.frac_out || !C.prec_frac) return fail(GEOSRAD_EINVAL, "geosrad_prec_scops: null array");
        return GEOSRAD_OK;
    }
    virtual int prec_scops_dev(hipStream_t, const PrecScopsCall &) { return nodev("geosrad_prec_scops_dev"); }
    virtual int prec_scops_host(const PrecScopsCall &) = 0;
    enum SgOut { SGO_FRAC_LS, SGO_FRAC_CV, SGO_PREC_LS, SGO_PREC_CV, SGO_MR_SUB, SGO_MR_SG, SGO_NOUT };
    struct SgHydroCall {
        int npoints, nlev, ncol;
        const void *frac_out;           // bytes (`_dev`) or reals (host)
        const void *mr[GEOSRAD_NHYDRO]; // the convective ones and the graupel may be null (zero)
        void *prec_frac;                // bytes (`_dev`) or reals (host), may be null
        void *out[SGO_NOUT];
    };
    int sghydro_check(const SgHydroCall &C)
    {
        if (const int rc = satsim_check("geosrad_cosp_sghydro", C.npoints, C.nlev, C.ncol, 1, 1, 1)) return rc;
        bool ok = C.frac_out != nullptr;
        for (int k = GEOSRAD_HYDRO_LSLIQ; k <= GEOSRAD_HYDRO_LSSNOW; k++) ok = ok && C.mr[k];
        if (!ok) return fail(GEOSRAD_EINVAL, "geosrad_cosp_sghydro: null input array");
        return GEOSRAD_OK;
    }
    virtual int sghydro_dev(hipStream_t, const SgHydroCall &) { return nodev("geosrad_cosp_sghydro_dev"); }
    virtual int sghydro_host(const SgHydroCall &) = 0;
    enum GasIn { GI_P, GI_T, GI_RH, GI_ZLEV, GI_NIN };
    struct GasCall {
        int npoints, nlev, surface_radar;
        double freq;
        const void *in[GI_NIN];
        void *out[2];                   // g_vol, g_to_vol: doubles in either kind
    };
    int radar_gases_check(const GasCall &C)
    {
        if (const int rc = satsim_check("geosrad_radar_gases", C.npoints, C.nlev, 1, 1, 1, 1)) return rc;
        // order_data knows a radar at the surface and a spaceborne one (format_input.f90:111-116)
        if (C.surface_radar != 0 && C.surface_radar != 1) return fail(GEOSRAD_EINVAL, "geosrad_radar_gases: surface_radar must be 0 or 1");
        if (!(C.freq > 0)) return fail(GEOSRAD_EINVAL, "geosrad_radar_gases: freq must be positive");
        for (int k = 0; k < GI_NIN; k++)
            if (!C.in[k]) return fail(GEOSRAD_EINVAL, "geosrad_radar_gases: null input array");
        return GEOSRAD_OK;
    }
    virtual int radar_gases_dev(hipStream_t, const GasCall &) { return nodev("geosrad_radar_gases_dev"); }
    virtual int radar_gases_host(const GasCall &) = 0;
};

// order of the `in` / `out` pointer arrays of sw_dev / sw_host
enum SwIn { S_PLAY, S_PLEV, S_TLAY, S_H2O, S_O3, S_CO2, S_CH4, S_O2, S_CLD, S_CIWP, S_CLWP, S_REI, S_REL, S_ZM, S_ALAT, S_TAUAER,
            S_SSAAER, S_ASMAER, S_COSZEN, S_ASDIR, S_ASDIF, S_ALDIR, S_ALDIF, S_NIN };
enum SwOutIx { SO_UFLX, SO_DFLX, SO_UFLXC, SO_DFLXC, SO_NIRR, SO_NIRF, SO_PARR, SO_PARF, SO_UVRR, SO_UVRF, SO_FSWBAND, SO_COT0,
               SO_DRBAND = SO_COT0 + 8, SO_DFBAND, SO_NOUT };

// sorad: order of the `in` (15) / `out` (13) pointer arrays
enum SoIn { SI_COSZ, SI_PL, SI_TA, SI_WA, SI_OA, SI_CWC, SI_FCLD, SI_REFF, SI_TAUA, SI_SSAA, SI_ASYA, SI_RSUVBM, SI_RSUVDF, SI_RSIRBM,
            SI_RSIRDF, SI_NIN };
enum SoOutIx { SOO_FLX, SOO_FLC, SOO_FDIRUV, SOO_FDIFUV, SOO_FDIRPAR, SOO_FDIFPAR, SOO_FDIRIR, SOO_FDIFIR, SOO_FLXU, SOO_FLCU,
               SOO_SFCBAND, SOO_DRBAND, SOO_DFBAND, SOO_NOUT };
// the `out` row of which na_out[k] (GEOSRAD_SONA_*) is the aerosol-free twin
constexpr int SONA_TWIN[GEOSRAD_SONA_NOUT] = {SOO_FLX, SOO_FLC, SOO_FLXU, SOO_FLCU, SOO_SFCBAND};
static inline bool sona_any(void *const *na_out)
{
    for (int k = 0; na_out && k < GEOSRAD_SONA_NOUT; k++) if (na_out[k]) return true;
    return false;
}

// irrad: order of the `in` (19) / `aer` (3, in-out) / `out` (11) pointer arrays
enum ChIn { C_PLE, C_TA, C_WA, C_OA, C_TB, C_N2O, C_CH4, C_CFC11, C_CFC12, C_CFC22, C_CWC, C_FCLD, C_REFF, C_FS, C_TG, C_EG, C_TV, C_EV,
            C_RV, C_NIN };
enum ChOutIx { CO_FLXU, CO_FLCU, CO_FLAU, CO_FLXAU, CO_FLXD, CO_FLCD, CO_FLAD, CO_FLXAD, CO_DFDTS, CO_SFCEM, CO_TAUDIAG, CO_NOUT };

// order of the `in` pointer array of lw_dev / lw_host
enum LwIn { I_PLAY, I_PLEV, I_TLAY, I_TLEV, I_TSFC, I_EMIS, I_H2O, I_O3, I_CO2, I_CH4, I_N2O, I_O2, I_CFC11, I_CFC12, I_CFC22,
            I_CCL4, I_CLDF, I_CIWP, I_CLWP, I_REI, I_REL, I_TAUAER, I_ZM, I_ALAT, I_NIN };
// O_UFLX_NA ..: the aerosol-free twins of the first six (geosrad_rrtmg_lw_na[_dev]); null from every other entry point
enum LwOutIx { O_UFLX, O_DFLX, O_UFLXC, O_DFLXC, O_DUFLX, O_DUFLXC, O_OLRB, O_DOLRB, O_UFLX_NA, O_DFLX_NA, O_UFLXC_NA, O_DFLXC_NA,
               O_DUFLX_NA, O_DUFLXC_NA, O_NOUT };

// Shape of every host array of the pointer lists above, stated here once: Fortran (ncol, rows) of records of `rec` reals, the column
// index the fastest but for the one inside a record (olrb is (16, ncol): one row of 16-real records; so are the stage dumps).  The
// `*_host` functions stage `rows` rows per column from it, MultiCtx finds a shard's first column at `c0 * rec` reals.  L = layers.
struct ArrShape { size_t rows, rec; };
static inline ArrShape lw_in_shape(int k, size_t L)
{
    return {(k == I_PLEV || k == I_TLEV) ? L + 1 : (k == I_TSFC || k == I_ALAT) ? 1 : k == I_EMIS ? 16 : k == I_TAUAER ? 16 * L : L, 1};
}
static inline ArrShape lw_out_shape(int k, size_t L) { return (k == O_OLRB || k == O_DOLRB) ? ArrShape{1, 16} : ArrShape{L + 1, 1}; }
static inline ArrShape lw_dump_shape(size_t L) { return {1, L * NG_LW}; }      // taug, pfracs: (nlay, 140, ncol)
static inline ArrShape sw_in_shape(int k, size_t L)
{
    return {k == S_PLEV ? L + 1 : (k == S_TAUAER || k == S_SSAAER || k == S_ASMAER) ? (size_t)NB_SW * L : (k == S_ALAT || k >= S_COSZEN) ? 1 : L, 1};
}
static inline ArrShape sw_out_shape(int k, size_t L)
{
    return {k <= SO_DFLXC ? L + 1 : (k == SO_FSWBAND || k == SO_DRBAND || k == SO_DFBAND) ? (size_t)NB_SW : 1, 1};
}
static inline ArrShape sw_dump_shape(int k, size_t L) { return {1, (k == 2 ? 1 : L) * NG_SW}; }      // taug, taur, ssi (112, ncol), the three cldprmc planes
static inline ArrShape ch_in_shape(int k, size_t L, size_t ns)
{
    return {k == C_PLE ? L + 1 : k == C_TB ? 1 : (k == C_CWC || k == C_REFF) ? 4 * L : (k == C_FS || k == C_TG || k == C_TV) ? ns
            : (k == C_EG || k == C_EV || k == C_RV) ? ns * 10 : L, 1};
}
static inline ArrShape ch_aer_shape(size_t L, size_t nb) { return {L * nb, 1}; }
static inline ArrShape ch_out_shape(int k, size_t L) { return {k == CO_SFCEM ? 1 : k == CO_TAUDIAG ? 10 * L : L + 1, 1}; }
static inline ArrShape so_in_shape(int k, size_t L, size_t nb)
{
    return {(k == SI_COSZ || k >= SI_RSUVBM) ? 1 : k == SI_PL ? L + 1 : (k == SI_CWC || k == SI_REFF) ? 4 * L
            : (k == SI_TAUA || k == SI_SSAA || k == SI_ASYA) ? L * nb : L, 1};
}
static inline ArrShape so_out_shape(int k, size_t L)
{
    return {(k == SOO_FLX || k == SOO_FLC || k == SOO_FLXU || k == SOO_FLCU) ? L + 1 : (k == SOO_SFCBAND || k == SOO_DRBAND || k == SOO_DFBAND) ? 8 : 1, 1};
}

// gettau: inputs cosz, dp, fcld, reff, hydromets; outputs of GtCall::out by kind
static inline ArrShape gt_in_shape(int k, size_t L) { return {k == 0 ? 1 : k <= 2 ? L : 4 * L, 1}; }
static inline ArrShape gt_out_shape(int kind, int k, size_t L) { return {kind == 2 ? (k == 0 ? 4 * L : L + 1) : (k <= 1 ? 4 * L : L), 1}; }
// icarus: the inputs of IcIn, the outputs of IcOut (L levels, S sub-columns); frac_out is (S * L) rows
static inline ArrShape ic_in_shape(int k, size_t L) { return {k == geosrad_ctx::IC_PHALF ? L + 1 : k == geosrad_ctx::IC_SKT ? 1 : L, 1}; }
static inline ArrShape ic_out_shape(int k, size_t S) { return {k == geosrad_ctx::ICO_FQ ? 49 : k >= geosrad_ctx::ICO_BOXTAU ? S : 1, 1}; }
// misr: every input of MisrIn is (npoints,L); the outputs of MisrOut
// modis: the inputs of ModisIn and the outputs of ModisOut (L levels, S sub-columns)
static inline ArrShape modis_in_shape(int k, size_t L, size_t S) { return {k == geosrad_ctx::MDI_PH ? L + 1 : k >= geosrad_ctx::MDI_BOXTAU ? S : L, 1}; }
static inline ArrShape modis_out_shape(int k, size_t S) { return {k == geosrad_ctx::MDO_MEAN ? (size_t)17 : k == geosrad_ctx::MDO_HIST ? (size_t)49 : S, 1}; }
// lidar: the inputs of LidarIn and the outputs of LidarOut (L levels, S sub-columns)
static inline ArrShape lidar_in_shape(int k, size_t L) { return {k == geosrad_ctx::LDI_PRESF ? L + 1 : k == geosrad_ctx::LDI_LAND ? 1 : L, 1}; }
static inline ArrShape lidar_out_shape(int k, size_t L, size_t S)
{
    const size_t rows[geosrad_ctx::LDO_NOUT] = {L, 4, 15 * L, 5, L, S * L, S * L, S * 5};
    return {rows[k], 1};
}
static inline ArrShape misr_out_shape(int k) { return {k == geosrad_ctx::MIO_FQ ? (size_t)(7 * 16) : k == geosrad_ctx::MIO_DIST ? (size_t)16 : (size_t)1, 1}; }

// The arrays of one host-pointer call, added in host_pipeline's order (copied in only, both ways, back only).  src: copied in, dst:
// copied back (null: the array only has its place on the device).  *at receives the array's device address before the solver is
// enqueued for a chunk; the slot of an array that is not added keeps what the caller put there (null).
struct HostArrs {
    size_t E;      // bytes per real
    std::vector<geosrad_ctx::PipeArr> arrs;
    std::vector<const void **> at;
    explicit HostArrs(size_t real_bytes) : E(real_bytes) {}
    void add(const void *src, void *dst, ArrShape s, const void **at_, size_t ebytes = 0)      // ebytes 0: reals
    {
        arrs.push_back({src, dst, s.rows, s.rec * (ebytes ? ebytes : E), 0});
        at.push_back(at_);
    }
    void add(const void *src, void *dst, ArrShape s, void **at_, size_t ebytes = 0) { add(src, dst, s, (const void **)at_, ebytes); }
    void add_clear_counts(int32_t *dst, void **at_) { add(nullptr, dst, {4, 1}, at_, sizeof(int32_t)); }      // (ncol, 4); a null dst stays on the device
};

// The library is built from this one source as three objects compiled in parallel (GEOSRAD_PART = 4: the fp32
// instantiation of Ctx and of every kernel, 8: the fp64 one, 0: the extern "C" layer); without GEOSRAD_PART it is
// a single translation unit.
geosrad_ctx *geosrad_new_ctx_f32();
geosrad_ctx *geosrad_new_ctx_f64();

#if !defined(GEOSRAD_PART) || GEOSRAD_PART != 0
namespace {

// inside Ctx<R> (its R, VW, grid256): kernel<R, VW> over a VW-th of the threads when `wide`, else kernel<R, 1>; `rows` = gridDim.y
#define LAUNCH_WIDE(kernel, wide, ncol, rows, st, arg) do {                                                            \
        if (wide) hipLaunchKernelGGL((kernel<R, VW>), dim3(grid256((ncol) / VW), rows), dim3(256), 0, st, arg);       \
        else hipLaunchKernelGGL((kernel<R, 1>), dim3(grid256(ncol), rows), dim3(256), 0, st, arg); } while (0)
template <typename R> struct Ctx : geosrad_ctx {
    using R2 = typename Vec2<R>::T;
    // tables
    DevBuf<> d_tab, d_xcw;
    size_t so_lds_set = 0;       // dynamic-LDS limit granted to k_sorad_col so far
    LwDev<R> h_T{};            // host copy (device pointers inside)
    DevBuf<LwDev<R>> d_T;
    bool have_lw = false;
    // RRTMG_SW tables
    DevBuf<> d_tab_sw;
    SwDev<R> h_S{};
    std::vector<R> avgcyc_mg, avgcyc_sb;          // NRLSSI2 mgavgcyc / sbavgcyc (134 each), host only: isolvar == 1
    DevBuf<SwDev<R>> d_S;
    bool have_sw = false;
    DevBuf<> d_ws_sw; int ws_sw_ncol = 0, ws_sw_nlay = 0, ws_sw_planes = 0; bool ws_sw_radval = false;
    // Chou-Suarez SW tables + workspace
    DevBuf<> d_tab_so;
    SoradDev<R> h_O{};
    DevBuf<SoradDev<R>> d_O;
    bool have_sorad = false;
    DevBuf<> d_ws_so;
    DevBuf<> d_ws_swc;      // sw_driver_chou_dev: the arrays SORADCORE prepares for sorad
    // Chou-Suarez LW tables + workspace
    DevBuf<> d_tab_ch;
    ChouDev<R> h_C{};
    DevBuf<ChouDev<R>> d_C;
    bool have_chou = false;
    DevBuf<> d_ws_ch;
    DevBuf<> d_ws_lwk;      // lw_driver_chou_dev: irrad's per-column surface arguments (+ TAUDIAG when not exported)
    DevBuf<> d_ws_drvs[2];      // RRTMG-side arrays of the LW / SW GridComp drivers (separate: the two may run on two streams)
    DevBuf<> d_ws_hb;           // sw_update_cldhb_dev: overlap correlation planes, cloud-layer range, partition and counts of one chunk
    // McICA segment plans (jump-ahead constants), cached per (mode, nsubcol, nlay, inhomogeneous?)
    struct PlanEntry { DevBuf<McSegDev> d_seg; int nseg; KissJump jsub, jhalf; };
    std::map<std::tuple<int, int, int, int>, PlanEntry> plans;
    // workspace
    DevBuf<> d_ws; int ws_ncol = 0, ws_nlay = 0;
    DevBuf<> d_zero;      // all-zero (nlay, ncol) plane of the RATS passes, and the second set of band partials they share with the aerosol-free pass
    DevBuf<int> d_bandflags;      // Update_Flx band exports: "band has a non-zero flux somewhere"
    DevBuf<uint32_t> d_err;
    // plain staging of mcica_host, the one host-pointer entry point that does not go through host_pipeline
    DevBuf<> d_io;

    Ctx() { for (int i = 0; i < 4; i++) { h_T.aam[i] = 0; h_T.ram[i] = 0; } }
    ~Ctx() override { if (stream) (void)hipStreamDestroy(stream); }      // the buffers free themselves

    int init() override
    {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIPCHK(d_err.resize(256));
        HIPCHK(hipMemset(d_err, 0, 256));
        HIPCHK(d_T.resize(sizeof(LwDev<R>)));
        HIPCHK(d_S.resize(sizeof(SwDev<R>)));
        HIPCHK(d_C.resize(sizeof(ChouDev<R>)));
        HIPCHK(d_O.resize(sizeof(SoradDev<R>)));
        if (lw_bands_lds_bytes<R>() > 64 * 1024) {      // the LDS copy of the LW transmittance table (fp32 build)
            const int lds = (int)lw_bands_lds_bytes<R>();
            HIPCHK(hipFuncSetAttribute((const void *)k_lw_bands<R, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            if constexpr (sizeof(R) == 4)
                HIPCHK(hipFuncSetAttribute((const void *)k_lw_bands<R, false, false, LW_WIDE_BLOCK>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            HIPCHK(hipFuncSetAttribute((const void *)k_lw_bands<R, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            HIPCHK(hipFuncSetAttribute((const void *)k_lw_bands<R, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        }
        // Oreopoulos et al. (2012) defaults (cloud_subcol_gen.F90:51-59)
        const double adl[4] = {1.4315, 2.1219, 7., -25.584}, rdl[4] = {0.72192, 0.78996, 8.5, 40.404};
        for (int i = 0; i < 4; i++) { h_T.aam[i] = (R)(sizeof(R) == 4 ? (float)adl[i] : adl[i]); h_T.ram[i] = (R)(sizeof(R) == 4 ? (float)rdl[i] : rdl[i]); }
        // the McICA kernels of the SW solver and of the stand-alone generator read aam / ram / xcw from d_T: it must hold the
        // defaults (and a null xcw) even when neither the LW tables, an inhomogeneity table nor correlation lengths are ever set
        return sync_T();
    }

    int sync_T()
    {
        HIPCHK(hipMemcpy(d_T, &h_T, sizeof(LwDev<R>), hipMemcpyHostToDevice));
        return GEOSRAD_OK;
    }

    // ---- table upload ----------------------------------------------------------------------------------
    int set_tables_lw(const void *blob, size_t nbytes) override
    {
        HIPCHK(hipSetDevice(device));
        Blob B;
        if (!B.parse(blob, nbytes)) return fail(GEOSRAD_ETABLE, B.err);
        if (B.realbytes != (int)sizeof(R))
            return fail(GEOSRAD_ETABLE, "table blob real size does not match the context's real_kind (use the _r4 blob for "
                                        "real_kind 4 and the _r8 blob for real_kind 8)");
        TableStage<R> S(B);
        std::string &missing = S.missing;
        auto &fix = S.fix;
        auto get = [&](const std::string &nm, size_t expect) { return S.get(nm, expect); };
        auto reserve = [&](size_t nreal) { return S.reserve(nreal); };
        auto at = [&](size_t off) { return S.at(off); };
        auto tr2 = [&](const R **slot, const std::string &nm, int n1, int ng) { S.tr2(slot, nm, n1, ng); };
        auto tr3 = [&](const R **slot, const std::string &nm, int nsp, int ng) { S.tr3(slot, nm, nsp, ng); };
        auto rows = [&](const R **slot, const std::string &nm, int ng, int m) { S.rows(slot, nm, ng, m); };
        auto raw = [&](const R **slot, const std::string &nm, size_t cnt) { S.raw(slot, nm, cnt); };
        auto scalar = [&](const std::string &nm) { return S.scalar(nm); };

        static const int ng[17] = {0, 10, 12, 16, 14, 16, 8, 12, 8, 12, 6, 8, 8, 4, 2, 2, 2};
        static const int nspa[17] = {0, 1, 1, 9, 9, 9, 1, 9, 1, 9, 1, 1, 9, 9, 1, 9, 9};
        static const int nspb[17] = {0, 1, 1, 5, 5, 5, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0};
        LwDev<R> &T = h_T;
        const R *xcw_keep = T.xcw;
        R aam[4], ram[4];
        for (int i = 0; i < 4; i++) { aam[i] = T.aam[i]; ram[i] = T.ram[i]; }
        memset(&T, 0, sizeof(T));
        T.xcw = xcw_keep;
        for (int i = 0; i < 4; i++) { T.aam[i] = aam[i]; T.ram[i] = ram[i]; }
        char nm[64];
        for (int b = 1; b <= 16; b++) {
            BandTab<R> &bt = T.b[b];
            auto N = [&](const char *s) { snprintf(nm, sizeof nm, "b%02d_%s", b, s); return std::string(nm); };
            tr2(&bt.absa, N("absa"), 65 * nspa[b], ng[b]);
            // band 16 declares absb(235,ng) although nspb(16) = 0 (rrlw_kg16.F90); bands 6,12,13,15 have no absb
            if (nspb[b] > 0 || b == 16) tr2(&bt.absb, N("absb"), 235 * (b == 16 ? 1 : nspb[b]), ng[b]);
            rows(&bt.fracrefa, N("fracrefa"), ng[b], nspa[b] == 9 ? 9 : 1);
            if (b != 6 && b != 12 && b != 15) rows(&bt.fracrefb, N("fracrefb"), ng[b], nspb[b] == 5 ? 5 : 1);
            tr2(&bt.selfref, N("selfref"), 10, ng[b]);
            tr2(&bt.forref, N("forref"), 4, ng[b]);
        }
        tr2(&T.b[1].m[0], "b01_ka_mn2", 19, ng[1]);   tr2(&T.b[1].m[1], "b01_kb_mn2", 19, ng[1]);
        tr3(&T.b[3].m[0], "b03_ka_mn2o", 9, ng[3]);   tr3(&T.b[3].m[1], "b03_kb_mn2o", 5, ng[3]);
        tr3(&T.b[5].m[0], "b05_ka_mo3", 9, ng[5]);    rows(&T.b[5].m[1], "b05_ccl4", ng[5], 1);
        tr2(&T.b[6].m[0], "b06_ka_mco2", 19, ng[6]);  rows(&T.b[6].m[1], "b06_cfc11adj", ng[6], 1);
        rows(&T.b[6].m[2], "b06_cfc12", ng[6], 1);
        tr3(&T.b[7].m[0], "b07_ka_mco2", 9, ng[7]);   tr2(&T.b[7].m[1], "b07_kb_mco2", 19, ng[7]);
        tr2(&T.b[8].m[0], "b08_ka_mco2", 19, ng[8]);  tr2(&T.b[8].m[1], "b08_kb_mco2", 19, ng[8]);
        tr2(&T.b[8].m[2], "b08_ka_mo3", 19, ng[8]);   tr2(&T.b[8].m[3], "b08_ka_mn2o", 19, ng[8]);
        tr2(&T.b[8].m[4], "b08_kb_mn2o", 19, ng[8]);  rows(&T.b[8].m[5], "b08_cfc12", ng[8], 1);
        rows(&T.b[8].m[6], "b08_cfc22adj", ng[8], 1);
        tr3(&T.b[9].m[0], "b09_ka_mn2o", 9, ng[9]);   tr2(&T.b[9].m[1], "b09_kb_mn2o", 19, ng[9]);
        tr2(&T.b[11].m[0], "b11_ka_mo2", 19, ng[11]); tr2(&T.b[11].m[1], "b11_kb_mo2", 19, ng[11]);
        tr3(&T.b[13].m[0], "b13_ka_mco2", 9, ng[13]); tr3(&T.b[13].m[1], "b13_ka_mco", 9, ng[13]);
        tr2(&T.b[13].m[2], "b13_kb_mo3", 19, ng[13]);
        tr3(&T.b[15].m[0], "b15_ka_mn2", 9, ng[15]);

        raw(&T.totplnk, "totplnk", 181 * 16); raw(&T.totplnkderiv, "totplnkderiv", 181 * 16);
        raw(&T.preflog, "preflog", 59); raw(&T.tref, "tref", 59); raw(&T.chi_mls, "chi_mls", 7 * 59);
        raw(&T.tau_tbl, "tau_tbl", NTBL + 1);
        raw(&T.absice0, "absice0", 2); raw(&T.absice1, "absice1", 10); raw(&T.absice2, "absice2", 43 * 16);
        raw(&T.absice3, "absice3", 46 * 16); raw(&T.absice4, "absice4", 200 * 16); raw(&T.absliq1, "absliq1", 58 * 16);
        {   // interleaved (exp_tbl, tfn_tbl)
            const R *ex = get("exp_tbl", NTBL + 1), *tf = get("tfn_tbl", NTBL + 1);
            if (ex && tf) {
                size_t off = reserve(2 * (size_t)(NTBL + 1));
                for (int i = 0; i <= NTBL; i++) { at(off)[2 * i] = ex[i]; at(off)[2 * i + 1] = tf[i]; }
                fix.push_back({(const R **)&T.lut, off});
            }
        }
        {   // chi_mls ratio tables: the same IEEE divisions setcoef performs per layer
            const R *chi = get("chi_mls", 7 * 59);
            if (chi) {
                static const int pa[RAT_NPAIR] = {1, 1, 1, 1, 4, 3}, pb[RAT_NPAIR] = {2, 3, 4, 6, 2, 2};
                size_t off = reserve((size_t)RAT_NPAIR * 60);
                for (int p = 0; p < RAT_NPAIR; p++)
                    for (int j = 1; j <= 59; j++) at(off)[p * 60 + j] = chi[(j - 1) * 7 + pa[p] - 1] / chi[(j - 1) * 7 + pb[p] - 1];
                fix.push_back({&T.rat, off});
            }
        }
        T.bpade = scalar("bpade"); T.fluxfac = scalar("fluxfac"); T.oneminus = scalar("oneminus");
        T.grav = scalar("grav"); T.avogad = scalar("avogad");
        {
            const R *dw = get("delwave", 16);
            if (dw) for (int b = 1; b <= 16; b++) T.delwave[b] = dw[b - 1];
            auto it = B.e.find("ice1b");
            if (it == B.e.end() || it->second.kind != -4 || it->second.count != 16) missing += "ice1b ";
            else memcpy(T.ice1b, it->second.data, 16 * sizeof(int32_t));
            // the band <-> g-point map is compiled into the kernels; refuse tables that disagree
            auto ig = B.e.find("ngb");
            if (ig == B.e.end() || ig->second.count != 140) missing += "ngb ";
            else {
                const int32_t *ngb = (const int32_t *)ig->second.data;
                int g = 0;
                for (int b = 1; b <= 16; b++) for (int k = 0; k < ng[b]; k++, g++) if (ngb[g] != b) missing += "ngb(mismatch) ";
            }
        }
        if (!missing.empty()) return fail(GEOSRAD_ETABLE, "missing/ill-shaped table entries: " + missing);

        HIPCHK(d_tab.resize(S.stage.size()));
        HIPCHK(hipMemcpy(d_tab, S.stage.data(), d_tab.bytes, hipMemcpyHostToDevice));
        for (auto &f : fix) *f.first = (const R *)(d_tab + f.second);
        have_lw = true;
        return sync_T();
    }

    int set_inhomogeneity(int ih, const void *blob, size_t nbytes) override
    {
        HIPCHK(hipSetDevice(device));
        if (ih == 0) {
            h_T.xcw = nullptr;
            return sync_T();
        }
        if (ih != 1 && ih != 2) return fail(GEOSRAD_EINPUT, "unknown inhomogeneity type");
        Blob B;
        if (!blob || !B.parse(blob, nbytes)) return fail(GEOSRAD_ETABLE, blob ? B.err : "xcw blob required for ih > 0");
        auto it = B.e.find("xcw");
        if (B.realbytes != (int)sizeof(R) || it == B.e.end() || it->second.count != 140000 || it->second.kind != (int)sizeof(R))
            return fail(GEOSRAD_ETABLE, "xcw blob missing / wrong precision");
        auto ii = B.e.find("ih");
        if (ii != B.e.end() && *(const int32_t *)ii->second.data != ih) return fail(GEOSRAD_ETABLE, "xcw blob is for a different ih");
        HIPCHK(d_xcw.reserve(140000 * sizeof(R)));
        HIPCHK(hipMemcpy(d_xcw, it->second.data, 140000 * sizeof(R), hipMemcpyHostToDevice));
        h_T.xcw = (const R *)d_xcw.p;
        return sync_T();
    }

    int set_corr(const double *adl, const double *rdl) override
    {
        // parameters are default-real in the reference: round through float for real_kind 4
        for (int i = 0; i < 4; i++) {
            if (adl) h_T.aam[i] = (R)adl[i];
            if (rdl) h_T.ram[i] = (R)rdl[i];
        }
        return sync_T();
    }

    // not counted: d_ws_swc, d_mc, d_xcw, d_tab_so, the fixed-size structs and McICA plans, the pipeline slots
    // (d_ws_hb is counted: like the solvers' workspaces it is sized by the chunk, two real planes of nlay x chunk columns)
    size_t workspace_bytes() const override
    {
        size_t t = 0;
        for (const DevBuf<> *b : {&d_ws, &d_ws_sw, &d_ws_ch, &d_ws_lwk, &d_ws_so, &d_ws_drvs[0], &d_ws_drvs[1], &d_ws_hb, &d_ws_ss, &d_ws_misr, &d_ws_modis, &d_ws_lidar, &d_ws_radar, &d_zero, &d_io, &d_tab, &d_tab_sw, &d_tab_ch})
            t += b->bytes;
        return t;
    }

    // ---- workspace -------------------------------------------------------------------------------------
    // the LW workspace of nc columns, straight into the kernels' arguments: on Carve() the bytes it takes, on Carve(d_ws) its planes
    size_t ws_layout(int nc, int nlay, LwArgs<R> &w, Carve c) const
    {
        const size_t cl = (size_t)nlay * nc;
        w.sc = c.take<R>(SC_NFIELD * cl);
        w.scidx = c.take<uint32_t>(cl);
        w.pwvcm = c.take<R>(nc);
        w.colcloudy = c.take<uint8_t>(nc);
        w.perm = c.take<int32_t>(nc);
        w.nclear = c.take<int32_t>(1 + part_blocks(nc));      // + the tile counts of the partition (launch_partition)
        w.laycloudy = c.take<uint8_t>(cl);
        w.alpha = c.take<R>(cl);
        w.rcorr = c.take<R>(cl);
        w.taucmc = c.take<R>(NG_LW * cl);
        const size_t clp = (size_t)nlay * (((size_t)nc + 255) & ~(size_t)255);      // tiled by 256-column block
        // parked cells of the band sweeps: a 2-byte Pade index per (layer, g-point) and stream (lw_kernels.hpp band_body)
        w.s1 = c.take<uint16_t>(NG_LW * clp);
        w.s2 = c.take<uint16_t>(NG_LW * clp);
        w.part = c.take<R>((size_t)6 * NB_LW * (nlay + 1) * nc);
        // split path: the Planck-fraction selector of every (band, layer, column) (lw_split_kernels.hpp)
        w.pfcode = c.take<uint32_t>(lw_split_path ? NB_LW * cl : 0);
        w.pffs = c.take<R>(lw_split_path ? NB_LW * cl : 0);
        return c.off;
    }
    int ensure_ws(int nc, int nlay)
    {
        if (d_ws && nc <= ws_ncol && nlay == ws_nlay) return GEOSRAD_OK;
        // grow-only in columns for a given nlay
        const int want = (d_ws && nlay == ws_nlay && nc < ws_ncol) ? ws_ncol : nc;
        LwArgs<R> w;
        const size_t need = ws_layout(want, nlay, w, Carve());
        if (d_ws.resize(need) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the LW workspace failed (" + std::to_string(need >> 20) +
                                                         " MiB); lower it with geosrad_set_chunk()");
        ws_ncol = want; ws_nlay = nlay;
        return GEOSRAD_OK;
    }

    // ---- what every `_dev` entry point is made of ------------------------------------------------------------------------
    static unsigned grid256(size_t n) { return (unsigned)((n + 255) / 256); }      // 256-thread blocks over n items
    // a caller's array from column c0 on; an array that is not there stays null
    static const R *colp(const void *p, size_t c0) { return p ? (const R *)p + c0 : nullptr; }
    static R *colp(void *p, size_t c0) { return p ? (R *)p + c0 : nullptr; }
    // columns a solver takes at once: the context's chunk, below `cap` where 32-bit byte offsets into one workspace plane set one
    int chunk_cols(int n, long cap = 0x7FFFFFFFL) const { const long nc = n < chunk ? n : chunk; return (int)(nc > cap ? cap : nc); }
    // body(c0, nc) for every chunk of [0, n), then the launches' status; a body that returns non-zero ends the walk with that code
    template <typename F> int chunk_walk(int n, int nc_max, F &&body)
    {
        for (int c0 = 0; c0 < n; c0 += nc_max)
            if (const int rc = body(c0, (n - c0) < nc_max ? (n - c0) : nc_max)) return rc;
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    // 16-byte accesses (VW reals per thread) when the column count and every address of the listed pointer arrays allow
    static constexpr int VW = 16 / (int)sizeof(R);
    struct PtrList { const void *const *p; int n; };
    static bool wide16(int ncol, std::initializer_list<PtrList> lists)
    {
        bool wide = ncol % VW == 0;
        for (const PtrList &l : lists) for (int k = 0; k < l.n; k++) wide = wide && ((uintptr_t)l.p[k] & 15) == 0;
        return wide;
    }

    // quads of sub-columns that never straddle a band; jump distances in units of draws
    int mc_plan(int mode, int nsubcol, int nlay, McPlan &out, int &nseg_out)
    {
        const bool inhomo = h_T.xcw != nullptr;
        const auto key = std::make_tuple(mode, nsubcol, nlay, inhomo ? 1 : 0);
        auto it = plans.find(key);
        if (it == plans.end()) {
            std::vector<McSegDev> segs;
            const uint64_t per = (uint64_t)(inhomo ? 4 : 2) * (uint64_t)nlay;
            auto add_range = [&](int g0, int ng, int band) {
                for (int q = 0; q < ng; q += MC_S) {
                    McSegDev sd;
                    memset(&sd, 0, sizeof sd);
                    sd.start = g0 + q; sd.count = (ng - q) < MC_S ? (ng - q) : MC_S; sd.band = band;
                    sd.j = make_kiss_jump((uint64_t)sd.start * per);
                    segs.push_back(sd);
                }
            };
            if (mode == 0) for (int b = 1; b <= NB_LW; b++) add_range(lw_band_g0(b), lw_band_ng(b), b);
            else if (mode == 2) for (int b = 16; b <= 29; b++) add_range(sw_band_g0(b), sw_band_ng(b), b);
            else add_range(0, nsubcol, 0);
            PlanEntry pe;
            pe.nseg = (int)segs.size();
            pe.jsub = make_kiss_jump(per);
            pe.jhalf = make_kiss_jump(2ull * (uint64_t)nlay);
            HIPCHK(pe.d_seg.resize(segs.size() * sizeof(McSegDev)));
            HIPCHK(hipMemcpy(pe.d_seg, segs.data(), pe.d_seg.bytes, hipMemcpyHostToDevice));
            it = plans.emplace(key, std::move(pe)).first;
        }
        out.seg = it->second.d_seg; out.nseg = it->second.nseg; out.jsub = it->second.jsub; out.jhalf = it->second.jhalf;
        nseg_out = it->second.nseg;
        return GEOSRAD_OK;
    }

    // The front end of both RRTMG solvers for one chunk, MODE 0: RRTMG_LW (A: LwArgs), 2: RRTMG_SW (A: SwArgs) - the column pass and the
    // clear | cloudy partition in one profile slot, setcoef with the per-layer input assertions (the aerosol ones are made by the band
    // sweeps), the overlap correlations, the McICA sub-columns with their cloud optics
    // (threads of clear columns exit at once).  radval: the RADVAL instantiation of the generator, which also fills rvsum.
    template <int MODE, typename Args> int rrtmg_front(hipStream_t st, const Args &A, bool radval = false, R *rvsum = nullptr)
    {
        constexpr bool SW = MODE == 2;
        const dim3 blk(256);
        const unsigned gx = grid256(A.ncol);
        const LwDev<R> *dT = d_T;
        const SwDev<R> *dS = SW ? (const SwDev<R> *)d_S : nullptr;
        span_begin(SW ? 6 : 0, st);
        if constexpr (SW) {
            hipLaunchKernelGGL(k_sw_validate<R>, dim3(gx), blk, 0, st, A);
        } else hipLaunchKernelGGL(k_validate_pwv<R>, dim3(gx), blk, 0, st, A, d_T);
        launch_partition(st, A.ncol, A.colcloudy, A.perm, A.nclear);
        span_end(st);
        span_begin(SW ? 7 : 1, st);
        if constexpr (SW) hipLaunchKernelGGL(k_sw_setcoef<R>, dim3(gx, A.nlay), blk, 0, st, A, dS);
        else hipLaunchKernelGGL((k_setcoef<R, true>), dim3(gx, A.nlay), blk, 0, st, A, d_T);
        span_end(st);
        span_begin(2, st);
        hipLaunchKernelGGL(k_overlap<R>, dim3(gx, A.nlay), blk, 0, st, A.ncol, A.ld, A.nlay, A.doy, A.zm, A.alat, (const int32_t *)A.perm,
                           (const int32_t *)A.nclear, dT, A.alpha, A.rcorr, A.laycloudy);
        span_end(st);
        McArgs<R> M{};
        M.ncol = A.ncol; M.ld = A.ld; M.nlay = A.nlay; M.nsubcol = SW ? NG_SW : NG_LW; M.doy = A.doy; M.cloudLM = A.cloudLM; M.cloudMH = A.cloudMH;
        M.iceflg = A.iceflg; M.liqflg = A.liqflg;
        // seed_order = [1,2,3,4] (rrtmg_lw_rad.F90:546) | [4,3,2,1] (SW/rrtmg_sw_rad.F90:1401)
        for (int k = 0; k < 4; k++) M.so[k] = SW ? 4 - k : 1 + k;
        M.cwp_tiny = (R)1.e-20;                                       // rrtmg_lw_rad.F90:544
        M.play = A.play; M.ciwp = A.ciwp; M.clwp = A.clwp; M.rei = A.rei; M.rel = A.rel;
        M.alpha = A.alpha; M.rcorr = A.rcorr; M.perm = A.perm; M.nclear = A.nclear; M.cftop = A.colcloudy;
        M.taucmc = A.taucmc; M.laycloudy = A.laycloudy; M.clearCounts = A.clearCounts; M.err = A.err;
        if constexpr (SW) { M.cldf = A.cld; M.ssacmc = A.ssacmc; M.asmcmc = A.asmcmc; M.cotsum = A.cotsum; M.rvsum = rvsum; }
        else M.cldf = A.cldf;
        McPlan MP; int nseg = 0;
        if (const int rc = mc_plan(MODE, M.nsubcol, A.nlay, MP, nseg)) return rc;
        const dim3 grid(xcd_grid(A.ncol, 64, nseg));
        span_begin(3, st);
        if constexpr (SW) {
            if (radval) hipLaunchKernelGGL((k_mcica<R, 2, true>), grid, dim3(64), 0, st, M, MP, dT, dS);
            else hipLaunchKernelGGL((k_mcica<R, 2>), grid, dim3(64), 0, st, M, MP, dT, dS);
        } else hipLaunchKernelGGL((k_mcica<R, 0>), grid, dim3(64), 0, st, M, MP, dT, dS);
        span_end(st);
        return GEOSRAD_OK;
    }

    // RRTMG_LW band sweeps of one chunk and the band reduction behind them.  lw_cols: (layer, g-point) intermediates in LDS, fluxes written
    // directly (lw_cols_kernels.hpp), no reduction; with A.dbg_taug the stage-dump instantiation; lw_split; else lw_bands: lane = column
    // with the parked cells (2-byte Pade indices) in HBM.  allow_cols: false for a call with RATS diagnostics or the aerosol-free fluxes, whose
    // passes need the per-band partials of the reduction - such a call takes that path throughout.  O.part_alt: the pass's own partials.
    int lw_sweeps(hipStream_t st, const LwArgs<R> &A, const LwOut<R> &O, bool allow_cols)
    {
        const dim3 blk(256);
        const unsigned gx = grid256(A.ncol);
        const size_t lds = lw_bands_lds_bytes<R>();
        const bool cols = lw_cols_path && allow_cols;
        LwArgs<R> S = A;      // a RATS pass sweeps into the partials its reduction takes the gas's bands from, and reduces with A's
        if (O.part_alt) S.part = const_cast<R *>(O.part_alt);
        span_begin(4, st);
        if (cols) {
            if (const int rc = hip_rc("lw_cols_launch", lw_cols_launch<R>(st, S, O, h_T, A.dbg_taug != nullptr))) return rc;
        } else if (A.dbg_taug) {
            hipLaunchKernelGGL((k_lw_bands<R, true, true>), dim3(gx, NB_LW), blk, lds, st, S, h_T);
        } else if (lw_split_path) {
            if (const int rc = hip_rc("lw_split_launch", lw_split_launch<R>(st, S, h_T))) return rc;
        } else {
            // (both instantiations band-major, heaviest band first: see band_block in lw_kernels.hpp)
            hipLaunchKernelGGL((k_lw_bands<R, false, false>), dim3(gx, NB_LW), blk, lds, st, S, h_T);
            if constexpr (sizeof(R) == 4)      // the 768-thread cloud-free blocks: run instead of the 256-thread ones when the batch has many cloud-free columns
                hipLaunchKernelGGL((k_lw_bands<R, false, false, LW_WIDE_BLOCK>), dim3((unsigned)((A.ncol + LW_WIDE_BLOCK - 1) / LW_WIDE_BLOCK), NB_LW),
                                   dim3(LW_WIDE_BLOCK), lds, st, S, h_T);
            hipLaunchKernelGGL((k_lw_bands<R, true, false>), dim3(gx, NB_LW), blk, lds, st, S, h_T);
        }
        span_end(st);
        if (!cols) { span_begin(5, st); hipLaunchKernelGGL(k_lw_reduce<R>, dim3(gx, A.nlay + 1), blk, 0, st, A, O); span_end(st); }
        return GEOSRAD_OK;
    }

    // the array checks lw_host makes before it stages anything and lw_dev makes in its own order
    int lw_check_arrays(const void *const *in, void *const *out)
    {
        for (int k = 0; k < I_NIN; k++) if (!in[k] && k != I_TAUAER) return fail(GEOSRAD_EINVAL, "null input array");
        for (int k = 0; k < 4; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null output array");
        return GEOSRAD_OK;
    }

    // ---- RRTMG_LW, device pointers ---------------------------------------------------------------------------
    int lw_dev(hipStream_t st, int ncol, int nlay, int dudTs, const void *const *in, int iceflg, int liqflg, int dyofyr,
               int cloudLM, int cloudMH, int32_t *clearCounts, void *const *out, const int32_t *band_output, void *dbg_taug,
               void *dbg_pfracs, const LwRats *rats) override
    {
        HIPCHK(hipSetDevice(device));
        if (!have_lw) return fail(GEOSRAD_EINVAL, "RRTMG_LW tables not set: call geosrad_set_tables_lw first (rrtmg_lw_ini)");
        if (ncol <= 0 || nlay < 4 || nlay > 203) return fail(GEOSRAD_EINVAL, "bad ncol/nlay (4 <= nlay <= mxlay = 203)");
        // checks the reference performs on scalars
        if (iceflg < 0 || iceflg > 4) return fail(GEOSRAD_EINPUT, "cldprmc: invalid iceflag");
        if (liqflg != 1) return fail(GEOSRAD_EINPUT, "cldprmc: invalid liqflag");
        if (cloudLM == cloudMH) return fail(GEOSRAD_EINPUT, "invalid pressure super-layers!");
        if (const int rc = lw_check_arrays(in, out)) return rc;
        if (dudTs && (!out[O_DUFLX] || !out[O_DUFLXC])) return fail(GEOSRAD_EINVAL, "dudTs set but duflx_dTs/duflxc_dTs null");
        bool any_bo = false;
        LwOut<R> O{};
        for (int b = 0; b < NB_LW; b++) { O.band_output[b] = band_output ? (band_output[b] != 0) : 0; any_bo |= O.band_output[b] != 0; }
        if (any_bo && (!out[O_OLRB] || (dudTs && !out[O_DOLRB]))) return fail(GEOSRAD_EINVAL, "band_output set but olrb/dolrb_dTs null");

        // one band's [layer][g<=16][column] plane of (a,bbu) pairs must stay below 4 GiB (32-bit byte offsets)
        const int nc_max = chunk_cols(ncol, (long)(0xFFFFFFFFull / ((unsigned long long)nlay * 16ull * sizeof(R2))) & ~255L);
        if (const int rc = ensure_ws(nc_max, nlay)) return rc;
        const int nrats = rats ? rats->n : 0;
        // the aerosol-free fluxes: requested by their first array (geosrad_rrtmg_lw_na[_dev] have checked the set, the driver passes its own)
        const bool na = out[O_UFLX_NA] != nullptr;
        R *zero = nullptr, *rat_part = nullptr;
        if (nrats > 0) {
            if (nrats > GEOSRAD_RAT_NGAS || !rats->uflx || !rats->dflx || (dudTs && !rats->duflx_dTs))
                return fail(GEOSRAD_EINVAL, "RATS: at most 8 gases; uflx_rat / dflx_rat (and duflx_dTs_rat with dudTs) must not be null");
            for (int r = 0; r < nrats; r++)
                if (rats->gas[r] < 0 || rats->gas[r] >= GEOSRAD_RAT_NGAS) return fail(GEOSRAD_EINVAL, "RATS: unknown gas code");
        }
        if (nrats > 0 || na) {
            // an all-zero (nlay, ncol) plane stands for the removed gas's mixing ratio (and for pwvcm of a dry column); behind it
            // a second set of band partials, so that the main call's stay available to the bands a gas does not touch.  The
            // aerosol-free pass needs the partials alone.
            auto carve = [&](Carve c) {
                if (nrats > 0) zero = c.take<R>((size_t)nlay * ncol);
                rat_part = c.take<R>((size_t)6 * NB_LW * (nlay + 1) * nc_max);
                return c.off;
            };
            if (d_zero.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the RATS workspace failed");
            carve(Carve(d_zero));
            if (zero) HIPCHK(hipMemsetAsync(zero, 0, (char *)rat_part - (char *)zero, st));
        }

        return chunk_walk(ncol, nc_max, [&](int c0, int nc) -> int {
            LwArgs<R> A{};
            ws_layout(nc, nlay, A, Carve(d_ws));
            A.ncol = nc; A.ld = ncol; A.nlay = nlay; A.dudTs = dudTs; A.iceflg = iceflg; A.liqflg = liqflg; A.doy = dyofyr;
            A.cloudLM = cloudLM; A.cloudMH = cloudMH;
            auto P = [&](int k) { return colp(in[k], c0); };
            A.play = P(I_PLAY); A.plev = P(I_PLEV); A.tlay = P(I_TLAY); A.tlev = P(I_TLEV); A.tsfc = P(I_TSFC); A.emis = P(I_EMIS);
            A.h2o = P(I_H2O); A.o3 = P(I_O3); A.co2 = P(I_CO2); A.ch4 = P(I_CH4); A.n2o = P(I_N2O); A.o2 = P(I_O2);
            A.cfc11 = P(I_CFC11); A.cfc12 = P(I_CFC12); A.cfc22 = P(I_CFC22); A.ccl4 = P(I_CCL4);
            A.cldf = P(I_CLDF); A.ciwp = P(I_CIWP); A.clwp = P(I_CLWP); A.rei = P(I_REI); A.rel = P(I_REL);
            A.tauaer = P(I_TAUAER); A.zm = P(I_ZM); A.alat = P(I_ALAT);
            A.err = d_err;
            A.dbg_taug = colp(dbg_taug, (size_t)c0 * NG_LW * nlay);
            A.dbg_pfracs = colp(dbg_pfracs, (size_t)c0 * NG_LW * nlay);
            A.clearCounts = clearCounts + c0;
            A.band_mask = LW_ALL_BANDS;
            if (const int e = rrtmg_front<0>(st, A)) return e;
            auto Q = [&](int k) { return colp(out[k], c0); };
            O.uflx = Q(O_UFLX); O.dflx = Q(O_DFLX); O.uflxc = Q(O_UFLXC); O.dflxc = Q(O_DFLXC);
            O.duflx_dTs = Q(O_DUFLX); O.duflxc_dTs = Q(O_DUFLXC);
            O.olrb = (R *)out[O_OLRB]; O.dolrb_dTs = (R *)out[O_DOLRB]; O.col0 = c0;
            if (const int e = lw_sweeps(st, A, O, nrats <= 0 && !na)) return e;

            // Aerosol-free fluxes: the reference's RRTMG branch leaves FLXA / FLA undefined (GEOS_IrradGridComp.F90:3552-3556, :3927-3990);
            // its other two branches compute them.  Nothing the clouds decide depends on the aerosols, and neither does setcoef, whose
            // output of the main pass is still in the workspace: the fluxes cost the band sweeps with a null aerosol pointer and one
            // more reduction.  The sweep writes all 16 bands into the second set of partials, which the RATS passes below use after
            // it: one stream runs the passes in order, so each pass's reduction has read the buffer before the next sweep writes it.
            // Without aerosols there is nothing to remove: the main pass's partials are reduced once more.
            if (na) {
                LwOut<R> ON{};      // band_output all zero: olrb / dolrb_dTs are the main pass's
                ON.uflx = Q(O_UFLX_NA); ON.dflx = Q(O_DFLX_NA); ON.uflxc = Q(O_UFLXC_NA); ON.dflxc = Q(O_DFLXC_NA);
                ON.duflx_dTs = Q(O_DUFLX_NA); ON.duflxc_dTs = Q(O_DUFLXC_NA); ON.col0 = c0;
                if (A.tauaer) {
                    LwArgs<R> B = A;
                    B.tauaer = nullptr; B.dbg_taug = nullptr; B.dbg_pfracs = nullptr; B.band_mask = LW_ALL_BANDS;
                    ON.part_alt = rat_part; ON.alt_mask = LW_ALL_BANDS;
                    if (const int e = lw_sweeps(st, B, ON, false)) return e;
                } else {
                    span_begin(5, st);
                    hipLaunchKernelGGL(k_lw_reduce<R>, dim3(grid256(nc), nlay + 1), dim3(256), 0, st, A, ON);
                    span_end(st);
                }
            }

            // RATS diagnostics (GEOS_IrradGridComp.F90:3405-3468): the reference calls the whole of rrtmg_lw once more per listed
            // gas with that gas's mixing ratio set to zero and keeps the total-sky uflx, dflx, duflx_dTs of each call.  Nothing
            // the clouds decide depends on the gases: the input checks (zero passes them), the clear | cloudy partition, the
            // overlap correlations, the sub-columns with their cloud optical depths (`taucmc`, `laycloudy`) and clearCounts of
            // the batch are still in the workspace, so a gas costs setcoef + band sweeps + the reduction only - and only the bands
            // the gas appears in are swept again (LW_RAT_BANDS, lw_device.hpp): their partials go to a second buffer and the
            // reduction takes every other band's from the main call.  Without water vapour the precipitable water
            // (rrtmg_lw_setcoef.F90:206-272) is 0 / amttl = exactly zero.
            for (int r = 0; r < nrats; r++) {
                static const R *LwArgs<R>::*const GAS[GEOSRAD_RAT_NGAS] = {&LwArgs<R>::h2o, &LwArgs<R>::o3, &LwArgs<R>::co2, &LwArgs<R>::ch4, &LwArgs<R>::n2o,
                                                                           &LwArgs<R>::cfc11, &LwArgs<R>::cfc12, &LwArgs<R>::cfc22};      // GEOSRAD_RAT_* order
                static_assert(GEOSRAD_RAT_H2O == 0 && GEOSRAD_RAT_N2O == 4 && GEOSRAD_RAT_HCFC22 == 7 && GEOSRAD_RAT_NGAS == 8, "GAS follows GEOSRAD_RAT_*");
                LwArgs<R> B = A;
                B.*GAS[rats->gas[r]] = zero;
                if (rats->gas[r] == GEOSRAD_RAT_H2O) B.pwvcm = zero;      // pwvcm is only read from here on
                B.dbg_taug = nullptr; B.dbg_pfracs = nullptr;
                B.band_mask = LW_RAT_BANDS[rats->gas[r]];
                span_begin(1, st); hipLaunchKernelGGL((k_setcoef<R, false>), dim3(grid256(nc), nlay), dim3(256), 0, st, B, d_T); span_end(st);
                LwOut<R> OR{};
                const size_t ro = (size_t)r * (nlay + 1) * ncol + c0;
                OR.uflx = (R *)rats->uflx + ro; OR.dflx = (R *)rats->dflx + ro;
                OR.duflx_dTs = rats->duflx_dTs ? (R *)rats->duflx_dTs + ro : nullptr;
                OR.col0 = c0; OR.part_alt = rat_part; OR.alt_mask = B.band_mask;
                if (const int e = lw_sweeps(st, B, OR, false)) return e;
            }
            return GEOSRAD_OK;
        });
    }

    // ---- GridComp drivers (gridcomp_kernels.hpp) ---------------------------------------------------------------------------
    int drv_reserve(int which, size_t need)
    {
        if (d_ws_drvs[which].reserve(need) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the driver workspace failed");
        return GEOSRAD_OK;
    }

    // one k_lit_scatter over a tile's outputs (lit_scatter_pack)
    int lit_scatter(hipStream_t st, const LitScatter<R> &S)
    {
        if (S.nf) hipLaunchKernelGGL((k_lit_scatter<R>), dim3(grid256(S.tile), S.rows), dim3(256), 0, st, S);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int lw_driver_dev(hipStream_t st, const LwdCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        const int ncol = C.ncol, lm = C.lm, nrats = C.nrats, iceflg = C.iceflg, liqflg = C.liqflg;
        const void *const *in = C.in;
        void *const *out = C.out;
        if (ncol <= 0 || lm < 4 || C.nb < 0 || C.nb > 16) return fail(GEOSRAD_EINVAL, "bad ncol/lm/nb_aer");
        if (nrats < 0 || nrats > GEOSRAD_RAT_NGAS || (nrats > 0 && (!C.rat_gas || !C.rat_out))) return fail(GEOSRAD_EINVAL, "bad RATS arguments");
        for (int k = 0; k < GEOSRAD_LWD_NIN; k++)
            if (!in[k] && k != GEOSRAD_LWD_CO2_3D && k != GEOSRAD_LWD_TAUA && k != GEOSRAD_LWD_SSAA) return fail(GEOSRAD_EINVAL, "null input array");
        if ((in[GEOSRAD_LWD_TAUA] == nullptr) != (in[GEOSRAD_LWD_SSAA] == nullptr)) return fail(GEOSRAD_EINVAL, "TAUA and SSAA go together");
        const size_t n = (size_t)ncol, cl = n * lm, cv = n * (lm + 1);
        R *lay[18], *lev[2], *tsfc, *alat, *emis, *aerp, *flux[6], *olrb, *dolrb, *rat[3], *flux_na[6];
        int32_t *cc;
        // the aerosol-free INTERNALs (geosrad_lw_driver_rrtmg_na_dev): without one of them the call is the RATS driver's
        bool na = false;
        for (int k = 0; C.na_out && k < GEOSRAD_LWNA_NOUT; k++) na = na || C.na_out[k];
        auto carve = [&](Carve c) {
            for (auto &q : lay) q = c.take<R>(cl);
            for (auto &q : lev) q = c.take<R>(cv);
            tsfc = c.take<R>(n); alat = c.take<R>(n); emis = c.take<R>(n * 16); aerp = c.take<R>(cl * 16);
            for (auto &q : flux) q = c.take<R>(cv);
            olrb = c.take<R>(n * 16); dolrb = c.take<R>(n * 16);
            cc = (int32_t *)c.take<R>(n * 4);      // clearCounts (ncol, 4) int32 in 4 n reals: twice the bytes in fp64, kept so that the layout stays as it was
            for (auto &q : rat) q = c.take<R>(cv * (size_t)nrats);
            for (auto &q : flux_na) q = c.take<R>(na ? cv : 0);      // the solver's six aerosol-free planes
            return c.off;
        };
        if (const int rc = drv_reserve(0, carve(Carve()))) return rc;
        carve(Carve(d_ws_drvs[0]));
        LwdArgs<R> A{};
        A.ncol = ncol; A.lm = lm; A.nb = in[GEOSRAD_LWD_TAUA] ? C.nb : 0; A.iceflg = iceflg; A.liqflg = liqflg;
        bind_in<Fields<LwdArgs<R>>>(A, in);
        A.co2_fixed = (R)C.consts[GEOSRAD_LWD_C_CO2_FIXED]; A.o2 = (R)C.consts[GEOSRAD_LWD_C_O2]; A.ccl4 = (R)C.consts[GEOSRAD_LWD_C_CCL4];
        // (MAPL_AIRMW/MAPL_H2OMW), (MAPL_AIRMW/MAPL_O3MW): constant expressions of the caller's real kind
        A.airmw_over_h2omw = (R)C.consts[GEOSRAD_C_AIRMW] / (R)C.consts[GEOSRAD_C_H2OMW];
        A.airmw_over_o3mw = (R)C.consts[GEOSRAD_C_AIRMW] / (R)C.consts[GEOSRAD_C_O3MW];
        A.rgas = (R)C.consts[GEOSRAD_C_RGAS]; A.grav = (R)C.consts[GEOSRAD_C_GRAV];
        A.play = lay[0]; A.tlay = lay[1]; A.h2o = lay[2]; A.o3_r = lay[3]; A.co2_r = lay[4]; A.ch4_r = lay[5];
        A.n2o_r = lay[6]; A.o2_r = lay[7]; A.cfc11_r = lay[8]; A.cfc12_r = lay[9]; A.cfc22_r = lay[10];
        A.ccl4_r = lay[11]; A.cldf = lay[12]; A.ciwp = lay[13]; A.clwp = lay[14]; A.rei = lay[15];
        A.rel = lay[16]; A.zm = lay[17]; A.plev = lev[0]; A.tlev = lev[1]; A.tsfc = tsfc; A.alat = alat;
        A.emis_r = emis; A.tauaer = aerp;
        const dim3 blk(256);
        const unsigned gx = grid256(ncol);
        hipLaunchKernelGGL((k_lwd_prep<R>), dim3(gx, lm), blk, 0, st, A);
        hipLaunchKernelGGL((k_lwd_zm<R>), dim3(gx), blk, 0, st, A);
        // reverse the super-layer interface indices (IRR:3237-3239) and call the solver with Ts_derivs = .true.
        const int cloudMH = lm - C.lcldmh + 1, cloudLM = lm - C.lcldlm + 1;
        const void *lin[I_NIN];
        lin[I_PLAY] = A.play; lin[I_PLEV] = A.plev; lin[I_TLAY] = A.tlay; lin[I_TLEV] = A.tlev; lin[I_TSFC] = A.tsfc; lin[I_EMIS] = A.emis_r;
        lin[I_H2O] = A.h2o; lin[I_O3] = A.o3_r; lin[I_CO2] = A.co2_r; lin[I_CH4] = A.ch4_r; lin[I_N2O] = A.n2o_r; lin[I_O2] = A.o2_r;
        lin[I_CFC11] = A.cfc11_r; lin[I_CFC12] = A.cfc12_r; lin[I_CFC22] = A.cfc22_r; lin[I_CCL4] = A.ccl4_r; lin[I_CLDF] = A.cldf;
        lin[I_CIWP] = A.ciwp; lin[I_CLWP] = A.clwp; lin[I_REI] = A.rei; lin[I_REL] = A.rel; lin[I_TAUAER] = A.tauaer; lin[I_ZM] = A.zm;
        lin[I_ALAT] = A.alat;
        void *lout[O_NOUT] = {flux[0], flux[1], flux[2], flux[3], flux[4], flux[5],
                              out[GEOSRAD_LWD_OLRB] ? out[GEOSRAD_LWD_OLRB] : (void *)olrb,
                              out[GEOSRAD_LWD_DOLRB] ? out[GEOSRAD_LWD_DOLRB] : (void *)dolrb};
        if (na) for (int k = 0; k < 6; k++) lout[O_UFLX_NA + k] = flux_na[k];
        static const int32_t no_bands[16] = {0};
        LwRats RT{};
        RT.n = nrats; RT.uflx = rat[0]; RT.dflx = rat[1]; RT.duflx_dTs = rat[2];
        for (int r = 0; r < nrats; r++) RT.gas[r] = C.rat_gas[r];
        if (const int rc = lw_dev(st, ncol, lm, 1, lin, iceflg, liqflg, C.doy, cloudLM, cloudMH, cc, lout, C.band_output ? C.band_output : no_bands,
                                  nullptr, nullptr, nrats > 0 ? &RT : nullptr)) return rc;
        if (nrats > 0) {
            LwdRatPost<R> RP{};
            RP.ncol = ncol; RP.lm = lm; RP.nrats = nrats; RP.uflx = rat[0]; RP.dflx = rat[1]; RP.duflx = rat[2]; RP.emis = A.emis;
            bind_out<Fields<LwdRatPost<R>>>(RP, C.rat_out);
            hipLaunchKernelGGL((k_lwd_rat_post<R>), dim3(gx, lm + 1, nrats), blk, 0, st, RP);
        }
        LwdPost<R> Q{};
        Q.ncol = ncol; Q.lm = lm; Q.ngpt = NG_LW;
        Q.uflx = flux[0]; Q.dflx = flux[1]; Q.uflxc = flux[2]; Q.dflxc = flux[3]; Q.duflx = flux[4];
        Q.duflxc = flux[5]; Q.clearCounts = cc; Q.emis = A.emis; Q.ts = A.ts;
        bind_out<Fields<LwdPost<R>>>(Q, out);
        hipLaunchKernelGGL((k_lwd_post<R>), dim3(gx, lm + 1), blk, 0, st, Q);
        if (na) {
            LwdPostNa<R> N{};
            N.ncol = ncol; N.lm = lm;
            N.uflx = flux_na[0]; N.dflx = flux_na[1]; N.uflxc = flux_na[2]; N.dflxc = flux_na[3]; N.duflx = flux_na[4]; N.duflxc = flux_na[5];
            bind_out<Fields<LwdPostNa<R>>>(N, C.na_out);
            hipLaunchKernelGGL((k_lwd_post_na<R>), dim3(gx, lm + 1), blk, 0, st, N);
        }
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    // lit != nullptr (both SW drivers): `in` / `out` are the un-packed tile's and ncol is NumLit (geosrad_sw_driver_*_lit_dev)
    int sw_driver_dev(hipStream_t st, const SwdCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        const int ncol = C.ncol, lm = C.lm, nb = C.nb, iceflg = C.iceflg, liqflg = C.liqflg;
        const void *const *in = C.in;
        void *const *out = C.out;
        const LitTile *lit = C.lit;
        const bool drf = C.drf();
        if ((lit ? lit->tile : ncol) <= 0 || lm < 4 || nb < 0 || nb > 14) return fail(GEOSRAD_EINVAL, "bad ncol/lm/nb_aer");
        if (lit) if (const char *msg = lit_check(*lit, ncol, out, GEOSRAD_SWD_NOUT)) return fail(GEOSRAD_EINVAL, msg);
        if (!C.drband != !C.dfband) return fail(GEOSRAD_EINVAL, "DRBAND and DFBAND go together");
        if (drf && lit && (C.keep_obio & 3) != 3 && (!lit->pos || !C.dark_obio))
            return fail(GEOSRAD_EINVAL, "DRBAND / DFBAND with a clear keep bit need lit_pos and dark_obio");
        // SORADCORE asserts the solar-variability options it supports before the call (GEOS_SolarGridComp.F90:6286-6292): no isolvar 1
        if (C.isolvar == 1) return fail(GEOSRAD_EINPUT, "SORADCORE: ISOLVAR == 1 is not supported by the GridComp (the solver entry point rrtmg_sw accepts it)");
        for (int k = 0; k < GEOSRAD_SWD_NIN; k++)
            if (!in[k] && k != GEOSRAD_SWD_TAUA && k != GEOSRAD_SWD_SSAA && k != GEOSRAD_SWD_ASYA) return fail(GEOSRAD_EINVAL, "null input array");
        const bool aer = in[GEOSRAD_SWD_TAUA] != nullptr;
        if (aer && (!in[GEOSRAD_SWD_SSAA] || !in[GEOSRAD_SWD_ASYA])) return fail(GEOSRAD_EINVAL, "TAUA, SSAA and ASYA go together");
        if (aer && nb != 14) return fail(GEOSRAD_EINVAL, "RRTMG_SW aerosol arrays have 14 bands");
        const LitTile xl{lit ? lit->tile : 0, lit ? lit->idx : nullptr, lit ? lit->pos : nullptr, C.dark, C.keep};      // the tile with DRBAND, DFBAND as rows
        if (lit) {      // what rrtmg_sw would reject, before anything is launched
            if (const int rc = sw_check_options(1, lm, iceflg, liqflg, lm - C.lcldlm + 1, lm - C.lcldmh + 1, 10)) return rc;
            SwSolar<R> SV;
            if (const int rc = sw_solar(C.sc, C.dist, C.isolvar, (const R *)C.bndsolvar, (const R *)C.indsolvar, nullptr, SV)) return rc;
        }
        if (lit && ncol == 0) return lit_scatter(st, lit_scatter_pack<R>(swd_tile, SWD_NROW, lm, xl, 0, C.rows, nullptr));      // no daytime column: the dark fill
        const size_t n = (size_t)ncol, cl = n * lm, cv = n * (lm + 1);
        const bool want_na = out[GEOSRAD_SWD_FSWNA] || out[GEOSRAD_SWD_FSCNA] || out[GEOSRAD_SWD_FSWUNA] || out[GEOSRAD_SWD_FSCUNA] ||
                             out[GEOSRAD_SWD_FSWBANDNA];
        R *lay[13], *lev[2], *aerp[3], *flux[4], *cot[8], *nflux[4] = {}, *nsc[14] = {}, *col[6] = {}, *plane[SWD_NPLANE] = {};
        R **scal = plane, *&band = plane[SWD_P_BAND], *&nband = plane[SWD_P_NBAND], **drfb = plane + SWD_P_DRBAND;      // the planes of swd_tile
        int32_t *cc;
        auto carve = [&](Carve c) {
            for (auto &q : lay) q = c.take<R>(cl);
            for (auto &q : lev) q = c.take<R>(cv);
            for (auto &q : aerp) q = c.take<R>(cl * 14);
            for (auto &q : flux) q = c.take<R>(cv);
            for (int k = 0; k < 6; k++) scal[k] = c.take<R>(n);
            for (auto &q : cot) q = c.take<R>(n);
            band = c.take<R>(n * 14);
            cc = (int32_t *)c.take<R>(n * 4);      // clearCounts (ncol, 4) int32 in 4 n reals, as in lw_driver_dev
            if (want_na) {      // the no-aerosol pass's own fluxes, surface scalars + optical thicknesses, band fluxes
                for (auto &q : nflux) q = c.take<R>(cv);
                for (auto &q : nsc) q = c.take<R>(n);
                nband = c.take<R>(n * 14);
            }
            if (lit) for (auto &q : col) q = c.take<R>(n);      // the packed per-column imports the solver reads as they are
            if (lit && drf) for (int k = 0; k < 2; k++) drfb[k] = c.take<R>(n * 14);      // DRBAND, DFBAND of the packed columns
            return c.off;
        };
        if (const int rc = drv_reserve(1, carve(Carve()))) return rc;
        carve(Carve(d_ws_drvs[1]));
        SwdLit<R> AL{};
        SwdArgs<R> &A = AL;
        A.ncol = ncol; A.lm = lm; A.nb = 14; A.iceflg = iceflg; A.liqflg = liqflg;
        bind_in<Fields<SwdLit<R>>>(AL, in);
        A.co2 = (R)C.consts[GEOSRAD_SWD_C_CO2]; A.o2 = (R)C.consts[GEOSRAD_SWD_C_O2];
        A.airmw_over_h2omw = (R)C.consts[GEOSRAD_SWD_C_AIRMW] / (R)C.consts[GEOSRAD_SWD_C_H2OMW];
        A.airmw_over_o3mw = (R)C.consts[GEOSRAD_SWD_C_AIRMW] / (R)C.consts[GEOSRAD_SWD_C_O3MW];
        A.rgas = (R)C.consts[GEOSRAD_SWD_C_RGAS]; A.grav = (R)C.consts[GEOSRAD_SWD_C_GRAV];
        A.play = lay[0]; A.tlay = lay[1]; A.h2o = lay[2]; A.o3_r = lay[3]; A.co2_r = lay[4]; A.ch4_r = lay[5];
        A.o2_r = lay[6]; A.cldf = lay[7]; A.ciwp = lay[8]; A.clwp = lay[9]; A.rei = lay[10]; A.rel = lay[11];
        A.zl = lay[12]; A.plev = lev[0]; A.tlev = lev[1]; A.tauaer = aerp[0]; A.ssaaer = aerp[1]; A.asmaer = aerp[2];
        const dim3 blk(256);
        const unsigned gx = grid256(ncol);
        // ZT ALAT ALBVR ALBVF ALBNR ALBNF: the caller's packed arrays, or the tile's gathered by the prep kernel
        const void *cin[6];
        for (int k = 0; k < 6; k++) { AL.col_out[k] = col[k]; cin[k] = lit ? col[k] : AL.col_in[k]; }
        if (lit) {
            AL.tile = lit->tile; AL.lit = lit->idx;
            hipLaunchKernelGGL((k_swd_prep<R, true>), dim3(gx, lm), blk, 0, st, AL);
        } else hipLaunchKernelGGL((k_swd_prep<R>), dim3(gx, lm), blk, 0, st, A);
        hipLaunchKernelGGL((k_swd_zm<R>), dim3(gx), blk, 0, st, A);
        const void *sin[S_NIN];
        sin[S_PLAY] = A.play; sin[S_PLEV] = A.plev; sin[S_TLAY] = A.tlay; sin[S_H2O] = A.h2o; sin[S_O3] = A.o3_r; sin[S_CO2] = A.co2_r;
        sin[S_CH4] = A.ch4_r; sin[S_O2] = A.o2_r; sin[S_CLD] = A.cldf; sin[S_CIWP] = A.ciwp; sin[S_CLWP] = A.clwp; sin[S_REI] = A.rei;
        sin[S_REL] = A.rel; sin[S_ZM] = A.zl; sin[S_ALAT] = cin[1]; sin[S_TAUAER] = A.tauaer; sin[S_SSAAER] = A.ssaaer;
        sin[S_ASMAER] = A.asmaer; sin[S_COSZEN] = cin[0]; sin[S_ASDIR] = cin[2]; sin[S_ASDIF] = cin[3];
        sin[S_ALDIR] = cin[4]; sin[S_ALDIF] = cin[5];
        void *sout[SO_NOUT] = {};
        for (int k = 0; k < 4; k++) sout[SO_UFLX + k] = flux[k];
        // what the solver writes as the driver returns it goes straight to the caller's packed arrays; a tile's takes the workspace planes
        auto direct = [&](int k, R *plane) { return out[k] && !lit ? out[k] : (void *)plane; };
        for (int k = 0; k < 6; k++) sout[SO_NIRR + k] = direct(GEOSRAD_SWD_NIRR + k, scal[k]);
        sout[SO_FSWBAND] = direct(GEOSRAD_SWD_FSWBAND, band);
        for (int k = 0; k < 8; k++) sout[SO_COT0 + k] = cot[k];      // cotd t/h/m/l then cotn t/h/m/l
        if (drf) { sout[SO_DRBAND] = lit ? (void *)drfb[0] : C.drband; sout[SO_DFBAND] = lit ? (void *)drfb[1] : C.dfband; }
        // IAER = 10 always (SOL:6235; without aerosols the arrays are zero); super-layer indices flipped in the call (SOL:6341)
        void *nout[SO_NOUT] = {};
        if (want_na) {
            for (int k = 0; k < 4; k++) nout[SO_UFLX + k] = nflux[k];
            for (int k = 0; k < 6; k++) nout[SO_NIRR + k] = nsc[k];
            for (int k = 0; k < 8; k++) nout[SO_COT0 + k] = nsc[6 + k];
            nout[SO_FSWBAND] = direct(GEOSRAD_SWD_FSWBANDNA, nband);
        }
        if (const int rc = sw_run(st, ncol, lm, C.sc, C.dist, C.isolvar, sin, iceflg, liqflg, C.dyofyr, 10, lm - C.lcldlm + 1, lm - C.lcldmh + 1,
                                  C.normflx, cc, sout, drf ? 1 : 0, C.bndsolvar, C.indsolvar, nullptr, nullptr, want_na ? nout : nullptr)) return rc;
        SwdPostLit<R> QL{};
        SwdPost<R> &Q = QL;
        Q.ncol = ncol; Q.lm = lm; Q.ngpt = NG_SW; Q.aerosols = C.include_aerosols; Q.undef = (R)C.consts[GEOSRAD_SWD_C_UNDEF];
        Q.swuflx = flux[0]; Q.swdflx = flux[1]; Q.swuflxc = flux[2]; Q.swdflxc = flux[3]; Q.clearCounts = cc;
        for (int k = 0; k < 4; k++) { Q.cotd[k] = cot[k]; Q.cotn[k] = cot[4 + k]; }
        bind_out<Fields<SwdPost<R>>>(Q, out);
        auto post_lit = [&](SwdPostLit<R> &P, TileSrc pass) {
            post_lit_pack(P, pass, xl);
            hipLaunchKernelGGL((k_swd_post_lit<R>), dim3(grid256(lit->tile), lm + 1), blk, 0, st, P);
        };
        if (lit) post_lit(QL, POST);
        else hipLaunchKernelGGL((k_swd_post<R>), dim3(gx, lm + 1), blk, 0, st, Q);
        if (want_na) {      // un-flip of the no-aerosol fluxes (the FS*NAN internals, SOL:4152-4159)
            SwdPostLit<R> NL{};
            SwdPost<R> &N = NL;
            N.ncol = ncol; N.lm = lm; N.ngpt = NG_SW; N.aerosols = 0; N.undef = Q.undef;
            N.swuflx = nflux[0]; N.swdflx = nflux[1]; N.swuflxc = nflux[2]; N.swdflxc = nflux[3]; N.clearCounts = cc;
            bind_out<SwdPostNa<R>>(N, out);
            if (lit) post_lit(NL, POST_NA);
            else hipLaunchKernelGGL((k_swd_post<R>), dim3(gx, lm + 1), blk, 0, st, N);
        }
        if (lit) return lit_scatter(st, lit_scatter_pack<R>(swd_tile, SWD_NROW, lm, xl, ncol, C.rows, plane));      // the results the solver wrote as returned
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int lw_chou_post_dev(hipStream_t st, int ncol, int lm, const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        LwcPost<R> P{};
        P.ncol = ncol; P.lm = lm;
        bind(P, in, out);
        auto need = [&](const R *o, const R *a, const R *b = (const R *)1) { return !o || (a && b); };
        if (!(need(P.flx_int, P.flxd, P.flxu) && need(P.flxa_int, P.flxad, P.flxau) && need(P.flc_int, P.flcd, P.flcu) &&
              need(P.fla_int, P.flad, P.flau) && need(P.dfdtsna, P.dfdts) && need(P.ts_int, P.ts)))
            return fail(GEOSRAD_EINVAL, "an output was requested without the field it is computed from");
        hipLaunchKernelGGL((k_lwd_chou_post<R>), dim3(grid256(ncol), lm + 1), dim3(256), 0, st, P);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    // Chou-Suarez branch of LW_Driver: k_lwk_surface (T2M and the surface arguments) + irrad with the cloud records prepared from the GEOS
    // fields (k_chou_prep<R, true>) + k_lwd_chou_post + k_lwk_diag.  Beyond irrad's own workspace: 34 values a column, and TAUDIAG when it
    // is not exported.
    int lw_driver_chou_dev(hipStream_t st, int ncol, int lm, const void *const *in, const double *consts, int trace, int lcldmh, int lcldlm,
                           int binary_clouds, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (!have_chou) return fail(GEOSRAD_EINVAL, "Chou-Suarez LW tables not set: call geosrad_load_tables_chou_lw first");
        if (ncol <= 0 || lm < 4 || lm > 400) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        if (!consts) return fail(GEOSRAD_EINVAL, "consts null");
        if (!(1 < lcldmh && lcldmh < lcldlm && lcldlm <= lm)) return fail(GEOSRAD_EINVAL, "super-layer levels must satisfy 1 < lcldmh < lcldlm <= lm");
        const bool aer = in[GEOSRAD_LWK_TAUA] != nullptr;
        if (aer != (in[GEOSRAD_LWK_SSAA] != nullptr) || aer != (in[GEOSRAD_LWK_ASYA] != nullptr))
            return fail(GEOSRAD_EINVAL, "TAUA / SSAA / ASYA: all three or none");
        for (int k = 0; k < GEOSRAD_LWK_TAUA; k++) if (!in[k]) return fail(GEOSRAD_EINVAL, "null input field");
        for (int k = 0; k <= GEOSRAD_LWK_SFCEM_INT; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null INTERNAL flux array");
        if (out[GEOSRAD_LWK_LWS0] && !out[GEOSRAD_LWK_FLX_INT]) return fail(GEOSRAD_EINVAL, "LWS0 was requested without FLX_INT, which it is computed from");
        auto I = [&](int k) { return (const R *)in[k]; };
        auto O = [&](int k) { return (R *)out[k]; };
        R *ws, *taudiag = O(GEOSRAD_LWK_TAUDIAG);      // ws: T2M, FS, TG, TV (ncol); EG, EV, RV (ncol,10); 256-byte aligned base, ncol % VW == 0 keeps 16
        auto carve = [&](Carve c) {
            ws = c.take<R>((size_t)34 * ncol);
            if (!out[GEOSRAD_LWK_TAUDIAG]) taudiag = c.take<R>((size_t)10 * lm * ncol);
            return c.off;
        };
        if (d_ws_lwk.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "LW_Driver (Chou-Suarez) workspace");
        carve(Carve(d_ws_lwk));
        // the addresses the two kernels touch
        const bool wide = wide16(ncol, {{in + GEOSRAD_LWK_PLE, 1}, {in + GEOSRAD_LWK_T, 1}, {in + GEOSRAD_LWK_TS, 1}, {in + GEOSRAD_LWK_EMIS, 1},
                                        {out + GEOSRAD_LWK_DFDTS, GEOSRAD_LWK_NOUT - GEOSRAD_LWK_DFDTS}});
        LwkSurf<R> S{};
        S.ncol = ncol; S.lm = lm; S.mkappa = -(R)consts[GEOSRAD_LWK_C_KAPPA];
        bind_in<Fields<LwkSurf<R>>>(S, in);
        S.t2m = O(GEOSRAD_LWK_T2M) ? O(GEOSRAD_LWK_T2M) : ws;
        S.fs = ws + (size_t)ncol; S.tg = ws + (size_t)2 * ncol; S.tv = ws + (size_t)3 * ncol;
        S.eg = ws + (size_t)4 * ncol; S.ev = ws + (size_t)14 * ncol; S.rv = ws + (size_t)24 * ncol;
        LAUNCH_WIDE(k_lwk_surface, wide, ncol, 11, st, S);
        HIPCHK(hipGetLastError());
        const void *ci[C_NIN] = {};
        ci[C_PLE] = in[GEOSRAD_LWK_PLE]; ci[C_TA] = in[GEOSRAD_LWK_T]; ci[C_WA] = in[GEOSRAD_LWK_Q]; ci[C_OA] = in[GEOSRAD_LWK_O3]; ci[C_TB] = S.t2m;
        ci[C_N2O] = in[GEOSRAD_LWK_N2O]; ci[C_CH4] = in[GEOSRAD_LWK_CH4]; ci[C_CFC11] = in[GEOSRAD_LWK_CFC11]; ci[C_CFC12] = in[GEOSRAD_LWK_CFC12];
        ci[C_CFC22] = in[GEOSRAD_LWK_HCFC22]; ci[C_FCLD] = in[GEOSRAD_LWK_FCLD];
        ci[C_FS] = S.fs; ci[C_TG] = S.tg; ci[C_EG] = S.eg; ci[C_TV] = S.tv; ci[C_EV] = S.ev; ci[C_RV] = S.rv;
        ChouGeos<R> G{};
        for (int s = 0; s < 4; s++) { G.q[s] = I(GEOSRAD_LWK_QI + s); G.r[s] = I(GEOSRAD_LWK_RI + s); }
        G.undef = (R)consts[GEOSRAD_LWK_C_UNDEF]; G.binary = binary_clouds != 0;
        void *ca[3] = {(void *)in[GEOSRAD_LWK_TAUA], (void *)in[GEOSRAD_LWK_SSAA], (void *)in[GEOSRAD_LWK_ASYA]};      // in-out, like irrad's
        void *co[CO_NOUT];
        static_assert(GEOSRAD_LWK_FLXU_INT == CO_FLXU && GEOSRAD_LWK_SFCEM_INT == CO_SFCEM, "the INTERNAL fluxes lead GEOSRAD_LWK_* in irrad's order");
        for (int k = 0; k <= CO_SFCEM; k++) co[k] = out[k];
        co[CO_TAUDIAG] = taudiag;
        // NA = 0 without an aerosol provider (IRR:1966-1970): irrad then never reads the three arrays
        const int rc = irrad_run(st, ncol, lm, ci, consts[GEOSRAD_LWK_C_CO2_FIXED], trace, lcldmh, lcldlm, 1, aer ? 1 : 0, 10, ca, co, &G);
        if (rc) return rc;
        const void *pi[GEOSRAD_LWC_NIN];
        for (int k = 0; k <= GEOSRAD_LWC_DFDTS; k++) pi[k] = out[k];
        pi[GEOSRAD_LWC_TS] = in[GEOSRAD_LWK_TS];
        void *po[GEOSRAD_LWC_NOUT];
        static_assert(GEOSRAD_LWK_TS_INT - GEOSRAD_LWK_SFCEM_INT == GEOSRAD_LWC_TS_INT - GEOSRAD_LWC_SFCEM_INT, "GEOSRAD_LWK_SFCEM_INT .. TS_INT follow GEOSRAD_LWC_*");
        for (int k = 0; k < GEOSRAD_LWC_NOUT; k++) po[k] = out[GEOSRAD_LWK_SFCEM_INT + k];
        if (const int rc2 = lw_chou_post_dev(st, ncol, lm, pi, po)) return rc2;
        LwkDiag<R> D{};
        D.ncol = ncol; D.lm = lm; D.taucrit = (R)consts[GEOSRAD_LWK_C_TAUCRIT] / (R)2.13; D.undef = G.undef;
        D.taudiag = taudiag;
        bind(D, in, out);
        if (D.tauir || D.cldtmp || D.cldprs || D.tsreff || D.dsfdts0 || D.sfcem0 || D.lws0) LAUNCH_WIDE(k_lwk_diag, wide, ncol, 1, st, D);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    // Chou-Suarez branch of SORADCORE: k_swc_prep + sorad_dev.  The prepared arrays live in a buffer of their own (sorad_dev's scratch is
    // sized per chunk, these per call).  On a tile (lit) that buffer also holds, NumLit wide, the imports sorad reads as they are and all its
    // results, which one k_lit_scatter takes to the tile.  With C.na_out the same prep and the same solver call also give the aerosol-free
    // internals (sorad_dev's na_out); their planes are further rows of the same scatter.  Without aerosol inputs the one pass is the
    // aerosol-free one: na_out are copies of their twins.
    int sw_driver_chou_dev(hipStream_t st, const SwcCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        const int ncol = C.ncol, lm = C.lm, nres = C.do_drfband ? GEOSRAD_SWC_NOUT : GEOSRAD_SWC_DRBAND;      // results sorad writes
        const void *const *in = C.in;
        void *const *out = C.out;
        const LitTile *lit = C.lit;
        if ((lit ? lit->tile : ncol) <= 0 || lm < 4) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        if (!C.consts) return fail(GEOSRAD_EINVAL, "consts null");
        const bool aer = in[GEOSRAD_SWC_TAUA] != nullptr;
        if (aer != (in[GEOSRAD_SWC_SSAA] != nullptr) || aer != (in[GEOSRAD_SWC_ASYA] != nullptr))
            return fail(GEOSRAD_EINVAL, "TAUA / SSAA / ASYA: all three or none");
        for (int k = 0; k < GEOSRAD_SWC_NIN; k++)
            if (!in[k] && !(k >= GEOSRAD_SWC_TAUA && k <= GEOSRAD_SWC_ASYA)) return fail(GEOSRAD_EINVAL, "null input field");
        if (lit) if (const char *msg = lit_check(*lit, ncol, out, nres)) return fail(GEOSRAD_EINVAL, msg);
        void *nao[GEOSRAD_SWCNA_NOUT] = {};      // the aerosol-free outputs requested
        bool na = false;
        for (int k = 0; C.na_out && k < GEOSRAD_SWCNA_NOUT; k++) { nao[k] = C.na_out[k]; na = na || nao[k]; }
        // the tile with the aerosol-free outputs as further rows: outputs, dark values and keep bits of out, then those of na_out
        void *tout[SWC_NTILE] = {};
        double tdark[SWC_NTILE] = {};
        LitTile xl{};
        if (lit) {
            const LitTile nl{lit->tile, lit->idx, lit->pos, C.dark_na, (uint64_t)(unsigned)C.keep_na};
            if (const char *msg = lit_check(nl, ncol, nao, GEOSRAD_SWCNA_NOUT)) return fail(GEOSRAD_EINVAL, msg);
            for (int k = 0; k < nres; k++) { tout[k] = out[k]; if (lit->dark) tdark[k] = lit->dark[k]; }
            for (int k = 0; k < GEOSRAD_SWCNA_NOUT; k++) { tout[GEOSRAD_SWC_NOUT + k] = nao[k]; if (C.dark_na) tdark[GEOSRAD_SWC_NOUT + k] = C.dark_na[k]; }
            const uint64_t low = ((uint64_t)1 << GEOSRAD_SWC_NOUT) - 1;
            xl = LitTile{lit->tile, lit->idx, lit->pos, tdark, (lit->keep & low) | ((uint64_t)(unsigned)C.keep_na << GEOSRAD_SWC_NOUT)};
        }
        if (lit) {      // what sorad_dev would reject, before anything is launched
            if (const int rc = sorad_check_options(1, lm, 8, C.lcldmh, C.lcldlm, C.hk_uv, C.hk_ir)) return rc;
            for (int k = 0; k < nres; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null output array");
            if (ncol == 0) return lit_scatter(st, lit_scatter_pack<R>(swc_tile, SWC_NTILE, lm, xl, 0, tout, nullptr));
        }
        const size_t n = (size_t)ncol, cl = (size_t)lm * ncol;
        SwcLit<R> PL{};
        SwcPrep<R> &P = PL;
        R *zero = nullptr;          // TAUA = SSAA = ASYA = 0 (SOL:4543-4546): one block serves the three
        R *res[SWC_NTILE] = {};
        auto carve = [&](Carve c) {
            P.plhpa = c.take<R>(cl + ncol); P.o3 = c.take<R>(cl); P.qq3 = c.take<R>(4 * cl); P.rr3 = c.take<R>(4 * cl);
            if (!aer) zero = c.take<R>(8 * cl);
            if (lit) {
                for (auto &q : PL.lay_out) q = c.take<R>(cl);
                if (aer) for (auto &q : PL.aer_out) q = c.take<R>(8 * cl);
                for (auto &q : PL.col_out) q = c.take<R>(n);
                for (int k = 0; k < nres; k++) res[k] = c.take<R>(n * swc_tile[k].nrows(lm));
                for (int k = 0; k < GEOSRAD_SWCNA_NOUT; k++)      // without aerosols: the twin's plane
                    if (nao[k]) res[GEOSRAD_SWC_NOUT + k] = aer ? c.take<R>(n * swc_tile[GEOSRAD_SWC_NOUT + k].nrows(lm)) : res[SWCNA_TWIN[k]];
            }
            return c.off;
        };
        if (d_ws_swc.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "SORADCORE (Chou-Suarez) workspace");
        carve(Carve(d_ws_swc));
        P.ncol = ncol; P.lm = lm;
        bind_in<Fields<SwcLit<R>>>(PL, in);
        P.o3fac = (R)C.consts[GEOSRAD_SWC_C_O3MW] / (R)C.consts[GEOSRAD_SWC_C_AIRMW]; P.undef = (R)C.consts[GEOSRAD_SWC_C_UNDEF];
        // T Q CL, TAUA SSAA ASYA, ZT ALBVR ALBVF ALBNR ALBNF: the caller's packed arrays, or the tile's gathered by the prep kernel
        const void *lay[3], *aerp[3], *col[5];
        for (int k = 0; k < 3; k++) { lay[k] = lit ? PL.lay_out[k] : PL.lay_in[k]; aerp[k] = !aer ? zero : (lit ? PL.aer_out[k] : PL.aer_in[k]); }
        for (int k = 0; k < 5; k++) col[k] = lit ? PL.col_out[k] : PL.col_in[k];
        if (lit) {
            PL.tile = lit->tile; PL.lit = lit->idx;
            hipLaunchKernelGGL((k_swc_prep<R, true>), dim3(grid256(ncol), lm + 1), dim3(256), 0, st, PL);
        } else hipLaunchKernelGGL((k_swc_prep<R>), dim3(grid256(ncol), lm + 1), dim3(256), 0, st, P);
        HIPCHK(hipGetLastError());
        if (!aer) HIPCHK(hipMemsetAsync(zero, 0, 8 * cl * sizeof(R), st));
        const void *si[SI_NIN];
        si[SI_COSZ] = col[0]; si[SI_PL] = P.plhpa; si[SI_TA] = lay[0]; si[SI_WA] = lay[1]; si[SI_OA] = P.o3;
        si[SI_CWC] = P.qq3; si[SI_FCLD] = lay[2]; si[SI_REFF] = P.rr3;
        si[SI_TAUA] = aerp[0]; si[SI_SSAA] = aerp[1]; si[SI_ASYA] = aerp[2];
        si[SI_RSUVBM] = col[1]; si[SI_RSUVDF] = col[2]; si[SI_RSIRBM] = col[3]; si[SI_RSIRDF] = col[4];
        auto O = [&](int k) { return lit ? (void *)res[k] : out[k]; };
        void *so[SOO_NOUT];
        so[SOO_FLX] = O(GEOSRAD_SWC_FSW); so[SOO_FLC] = O(GEOSRAD_SWC_FSC); so[SOO_FLXU] = O(GEOSRAD_SWC_FSWU); so[SOO_FLCU] = O(GEOSRAD_SWC_FSCU);
        so[SOO_FDIRIR] = O(GEOSRAD_SWC_NIRR); so[SOO_FDIFIR] = O(GEOSRAD_SWC_NIRF); so[SOO_FDIRPAR] = O(GEOSRAD_SWC_PARR);
        so[SOO_FDIFPAR] = O(GEOSRAD_SWC_PARF); so[SOO_FDIRUV] = O(GEOSRAD_SWC_UVRR); so[SOO_FDIFUV] = O(GEOSRAD_SWC_UVRF);
        so[SOO_SFCBAND] = O(GEOSRAD_SWC_FSWBAND); so[SOO_DRBAND] = O(GEOSRAD_SWC_DRBAND); so[SOO_DFBAND] = O(GEOSRAD_SWC_DFBAND);
        // GEOSRAD_SWCNA_* is GEOSRAD_SONA_*'s order: the second pass only with aerosols to take away
        void *sna[GEOSRAD_SONA_NOUT] = {};
        static_assert(GEOSRAD_SONA_NOUT == GEOSRAD_SWCNA_NOUT && (int)GEOSRAD_SONA_SFCBAND == (int)GEOSRAD_SWCNA_FSWBANDNA, "the driver's na_out is the solver's");
        for (int k = 0; na && aer && k < GEOSRAD_SWCNA_NOUT; k++) sna[k] = lit ? (void *)res[GEOSRAD_SWC_NOUT + k] : nao[k];
        if (const int rc = sorad_dev(st, ncol, lm, 8, si, C.consts[GEOSRAD_SWC_C_CO2], C.lcldmh, C.lcldlm, C.hk_uv, C.hk_ir, so, C.do_drfband, sna)) return rc;
        if (!lit) {
            for (int k = 0; na && !aer && k < GEOSRAD_SWCNA_NOUT; k++)
                if (nao[k]) HIPCHK(hipMemcpyAsync(nao[k], out[SWCNA_TWIN[k]], n * swc_tile[SWCNA_TWIN[k]].nrows(lm) * sizeof(R), hipMemcpyDeviceToDevice, st));
            return GEOSRAD_OK;
        }
        return lit_scatter(st, lit_scatter_pack<R>(swc_tile, SWC_NTILE, lm, xl, ncol, tout, res));
    }

    int lw_update_flx_dev(hipStream_t st, int ncol, int lm, int rrtmg, int lev_mid_high, int lev_low_mid, double undef,
                          const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        if (lev_mid_high < 1 || lev_mid_high > lm || lev_low_mid < 1 || lev_low_mid > lm) return fail(GEOSRAD_EINVAL, "bad super-layer levels");
        auto na = [](int k) {
            return k == GEOSRAD_LWU_FLXA_INT || k == GEOSRAD_LWU_FLA_INT || k == GEOSRAD_LWU_FLXAU_INT || k == GEOSRAD_LWU_FLAU_INT ||
                   k == GEOSRAD_LWU_FLXAD_INT || k == GEOSRAD_LWU_FLAD_INT || k == GEOSRAD_LWU_DFDTSNA || k == GEOSRAD_LWU_DFDTSCNA;
        };
        for (int k = 0; k < GEOSRAD_LWU_NIN; k++)
            if (!in[k] && !(rrtmg && na(k))) return fail(GEOSRAD_EINVAL, "null internal-state array");
        LwUpd<R> U{};
        U.ncol = ncol; U.lm = lm; U.rrtmg = rrtmg; U.lev_mid_high = lev_mid_high; U.lev_low_mid = lev_low_mid; U.undef = (R)undef;
        bind(U, in, out);
        const bool wide = wide16(ncol, {{in, GEOSRAD_LWU_NIN}, {out, GEOSRAD_LWU_NOUT}});
        LAUNCH_WIDE(k_lw_update_flx, wide, ncol, lm + 1, st, U);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int lw_update_rats_dev(hipStream_t st, int ncol, int lm, int nrats, const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0 || nrats < 0 || nrats > GEOSRAD_RAT_NGAS) return fail(GEOSRAD_EINVAL, "bad ncol/lm/nrats");
        if (nrats == 0) return GEOSRAD_OK;
        for (int k = 0; k < GEOSRAD_LWR_NIN; k++)
            if (!in[k] && !(k == GEOSRAD_LWR_DFDTS || k == GEOSRAD_LWR_DFDTS_RAT)) return fail(GEOSRAD_EINVAL, "null internal-state array");
        if (out[GEOSRAD_LWR_DFDTS_OUT] && (!in[GEOSRAD_LWR_DFDTS] || !in[GEOSRAD_LWR_DFDTS_RAT]))
            return fail(GEOSRAD_EINVAL, "DFDTS_<gas> requested without DFDTS / DFDTS_RAT");
        LwRatUpd<R> U{};
        U.ncol = ncol; U.lm = lm; U.nrats = nrats;
        bind(U, in, out);
        hipLaunchKernelGGL((k_lw_update_rats<R>), dim3(grid256(ncol), lm + 1, nrats), dim3(256), 0, st, U);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int lw_update_bands_dev(hipStream_t st, int ncol, const int32_t *band_output, const double *wn1, const double *wn2, double undef,
                            const void *tsinst, const void *ts_int, const void *olrb_int, const void *dolrb_int, void *olrb_exp,
                            void *tbrb_exp) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || !band_output || !wn1 || !wn2 || !tsinst || !ts_int || !olrb_int || !dolrb_int) return fail(GEOSRAD_EINVAL, "bad arguments");
        if (!olrb_exp && !tbrb_exp) return GEOSRAD_OK;
        HIPCHK(d_bandflags.reserve(16 * sizeof(int)));
        HIPCHK(hipMemsetAsync(d_bandflags, 0, 16 * sizeof(int), st));
        LwBandUpd<R> U{};
        U.ncol = ncol; U.undef = (R)undef;
        for (int b = 0; b < 16; b++) {
            U.band_output[b] = band_output[b] != 0;
            U.wn1[b] = (R)wn1[b] * (R)100.; U.wn2[b] = (R)wn2[b] * (R)100.;      // wavenum1(ibnd)*100. [m-1] (IRR:4016)
            if (U.band_output[b] && !(wn2[b] > wn1[b] && wn1[b] + wn2[b] > 0)) return fail(GEOSRAD_EINVAL, "band limits must satisfy 0 <= wavenum1 < wavenum2");
        }
        U.tsinst = (const R *)tsinst; U.ts_int = (const R *)ts_int; U.olrb_int = (const R *)olrb_int; U.dolrb_int = (const R *)dolrb_int;
        U.olrb_exp = (R *)olrb_exp; U.tbrb_exp = (R *)tbrb_exp; U.nonzero = d_bandflags;
        const dim3 grid(grid256(ncol), 16);
        hipLaunchKernelGGL((k_lw_update_bands<R, 0>), grid, dim3(256), 0, st, U);
        if (tbrb_exp) hipLaunchKernelGGL((k_lw_update_bands<R, 1>), grid, dim3(256), 0, st, U);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int sw_update_export_dev(hipStream_t st, int ncol, int lm, int nbands, const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0 || nbands < 0) return fail(GEOSRAD_EINVAL, "bad ncol/lm/nbands");
        SwUpd<R> U{};
        U.ncol = ncol; U.lm = lm; U.nbands = nbands;
        bind(U, in, out);
        if (!U.slr) return fail(GEOSRAD_EINVAL, "SLR is required");
        // an export needs the internals it is computed from
        auto need = [&](const R *o, const R *a, const R *b = (const R *)1) { return !o || (a && b); };
        const bool ok = need(U.fsw, U.fswn) && need(U.fsc, U.fscn) && need(U.fswna, U.fswnan) && need(U.fscna, U.fscnan) &&
                        need(U.fswu, U.fswun) && need(U.fscu, U.fscun) && need(U.fswuna, U.fswunan) && need(U.fscuna, U.fscunan) &&
                        need(U.fswd, U.fswn, U.fswun) && need(U.fscd, U.fscn, U.fscun) && need(U.fswdna, U.fswnan, U.fswunan) &&
                        need(U.fscdna, U.fscnan, U.fscunan) && need(U.fswband, U.fswbandn) && need(U.fswbandna, U.fswbandnan) &&
                        need(U.rsr, U.fswn) && need(U.rsrs, U.fswn) && need(U.osr, U.fswn) && need(U.rsc, U.fscn) && need(U.rscs, U.fscn) &&
                        need(U.osrclr, U.fscn) && need(U.rsrna, U.fswnan) && need(U.rsrsna, U.fswnan) && need(U.osrna, U.fswnan) &&
                        need(U.rscna, U.fscnan) && need(U.rscsna, U.fscnan) && need(U.osrcna, U.fscnan);
        if (!ok) return fail(GEOSRAD_EINVAL, "an export was requested without the internal field it is computed from");
        const bool wide = wide16(ncol, {{in, GEOSRAD_SWU_NIN}, {out, GEOSRAD_SWU_NOUT}});
        LAUNCH_WIDE(k_sw_update_export, wide, ncol, lm + 1 + nbands, st, U);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    // the walk of SOL:7665-7728 in R, as the list k_sw_update_obio takes
    int obio_table(int scheme, int nbands, const double *wvn1, const double *wvn2, const int32_t *order, ObioUpd<R> &U)
    {
        R s1[OBIO_MAXBANDS], s2[OBIO_MAXBANDS];
        int ord[OBIO_MAXBANDS], npairs = 0;
        if (const char *e = obio_solar_bands<R>(scheme, nbands, wvn1, wvn2, order, s1, s2, ord)) return fail(GEOSRAD_EINVAL, e);
        U.nbands = nbands;
        for (int jb = 0; jb < nbands; jb++) { U.ib[jb] = ord[jb] - 1; U.np[jb] = 0; }
        bool fed[NB_OBIO] = {};
        const char *e = obio_walk<R>(nbands, s1, s2, ord, [&](int jb, int, int kb, R sfrac) {
            if (npairs < OBIO_MAXPAIRS) { U.w[npairs] = sfrac; U.kb[npairs] = kb - 1; U.np[jb]++; fed[kb - 1] = true; }
            npairs++;
        });
        if (e) return fail(GEOSRAD_EINVAL, e);
        if (npairs > OBIO_MAXPAIRS) return fail(GEOSRAD_EINVAL, "SOLAR TO OBIO: more overlaps than two gapless band sets can have");
        for (int p = 0; p < npairs; p++) if (p + 1 == npairs || U.kb[p + 1] != U.kb[p]) U.kb[p] |= 128;
        for (int k = 0; k < NB_OBIO; k++) if (!fed[k]) U.zkb[U.nzero++] = k;
        return GEOSRAD_OK;
    }

    int sw_update_obio_dev(hipStream_t st, int ncol, int scheme, int nbands, const double *wvn1, const double *wvn2, const int32_t *order,
                           const void *slr, const void *drbandn, const void *dfbandn, void *drobio, void *dfobio) override
    {
        if (ncol < 1) return fail(GEOSRAD_EINVAL, "bad ncol");
        ObioUpd<R> U{};
        if (const int rc = obio_table(scheme, nbands, wvn1, wvn2, order, U)) return rc;
        if (!drobio && !dfobio) return GEOSRAD_OK;
        if (!slr || (drobio && !drbandn) || (dfobio && !dfbandn))
            return fail(GEOSRAD_EINVAL, "an export was requested without the internal field it is computed from");
        HIPCHK(hipSetDevice(device));
        U.ncol = ncol; U.slr = (const R *)slr;
        int nfam = 0;
        if (drobio) { U.x[nfam] = (const R *)drbandn; U.y[nfam++] = (R *)drobio; }
        if (dfobio) { U.x[nfam] = (const R *)dfbandn; U.y[nfam++] = (R *)dfobio; }
        const void *ptrs[5] = {slr, U.x[0], U.y[0], U.x[nfam - 1], U.y[nfam - 1]};
        const bool wide = wide16(ncol, {{ptrs, 5}});
        LAUNCH_WIDE(k_sw_update_obio, wide, ncol, nfam, st, U);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int sw_update_surface_dev(hipStream_t st, int ncol, int lm, double undef, const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        for (int k = 0; k <= GEOSRAD_SWS_FSWN; k++) {
            const bool alb_imp = k >= GEOSRAD_SWS_ALBVF && k <= GEOSRAD_SWS_ALBNR;
            if (!in[k] && !(alb_imp && !out[GEOSRAD_SWS_ALBVF_X + (k - GEOSRAD_SWS_ALBVF)]) &&
                !(k == GEOSRAD_SWS_ZTH && !out[GEOSRAD_SWS_DRNUVR] && !out[GEOSRAD_SWS_DRNPAR] && !out[GEOSRAD_SWS_DRNNIR]))
                return fail(GEOSRAD_EINVAL, "null input field");
        }
        if ((!in[GEOSRAD_SWS_FSCN] && (out[GEOSRAD_SWS_SLRSFC] || out[GEOSRAD_SWS_SLRSUFC])) ||
            (!in[GEOSRAD_SWS_FSWNAN] && (out[GEOSRAD_SWS_SLRSFNA] || out[GEOSRAD_SWS_SLRSUFNA])) ||
            (!in[GEOSRAD_SWS_FSCNAN] && (out[GEOSRAD_SWS_SLRSFCNA] || out[GEOSRAD_SWS_SLRSUFCNA])))
            return fail(GEOSRAD_EINVAL, "a requested surface export needs an internal flux that is null");
        SwSfc<R> U{};
        U.ncol = ncol; U.lm = lm; U.undef = (R)undef;
        bind(U, in, out);
        hipLaunchKernelGGL((k_sw_update_surface<R>), dim3(grid256(ncol)), dim3(256), 0, st, U);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int sw_update_clouds_dev(hipStream_t st, int ncol, int lm, int lcldmh, int lcldlm, double taucrit, const double *consts,
                             const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        if (!(1 < lcldmh && lcldmh < lcldlm && lcldlm <= lm)) return fail(GEOSRAD_EINVAL, "super-layer levels must satisfy 1 < lcldmh < lcldlm <= lm");
        if (!consts) return fail(GEOSRAD_EINVAL, "consts null");
        if (!have_sorad) return fail(GEOSRAD_EINVAL, "Chou-Suarez SW tables not set: call geosrad_load_tables_chou_sw first");
        bool any = false, optics = false;          // optics: an export GETVISTAU's optical thickness feeds
        for (int k = 0; k < GEOSRAD_SWK_NOUT; k++) {
            any = any || out[k];
            optics = optics || (out[k] && ((k >= GEOSRAD_SWK_TAUCLI && k <= GEOSRAD_SWK_TAUCLS) || k >= GEOSRAD_SWK_TAULO));
        }
        if (any && !in[GEOSRAD_SWK_FCLD]) return fail(GEOSRAD_EINVAL, "FCLD is required");
        for (int k = GEOSRAD_SWK_QI; k <= GEOSRAD_SWK_RS; k++)
            if (optics && !in[k]) return fail(GEOSRAD_EINVAL, "an optical-thickness export was requested without QI..QS / RI..RS");
        if (optics && !in[GEOSRAD_SWK_PLE]) return fail(GEOSRAD_EINVAL, "an optical-thickness export was requested without PLE");
        if (out[GEOSRAD_SWK_CLDTMP] && !in[GEOSRAD_SWK_T]) return fail(GEOSRAD_EINVAL, "CLDTMP requested without T");
        if (!any) return GEOSRAD_OK;
        SwCld<R> U{};
        U.ncol = ncol; U.lm = lm; U.ict = lcldmh; U.icb = lcldlm; U.optics = optics;
        U.grav = (R)consts[GEOSRAD_SWK_C_GRAV]; U.undef = (R)consts[GEOSRAD_SWK_C_UNDEF]; U.taucrit = (R)taucrit;
        for (int k = 0; k < GEOSRAD_SWK_NIN; k++) U.in[k] = (const R *)in[k];
        for (int k = 0; k < GEOSRAD_SWK_NOUT; k++) U.out[k] = (R *)out[k];
        hipLaunchKernelGGL((k_sw_update_clouds<R>), dim3(grid256(ncol)), dim3(256), 0, st, U, (const SoradDev<R> *)d_O);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    // CLD??SWHB of UPDATE_EXPORT (mcica_kernels.hpp: k_swhb_prep, k_swhb_count, k_swhb_export), chunk by chunk
    int sw_update_cldhb_dev(hipStream_t st, int ncol, int lm, int lcldmh, int lcldlm, int doy, const double *consts,
                            const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol < 1) return fail(GEOSRAD_EINVAL, "bad ncol");
        if (lm < 4 || lm > 0xFFFE) return fail(GEOSRAD_EINVAL, "the generator's seeds need four layers (and lm < 65535)");
        if (!(1 < lcldmh && lcldmh < lcldlm && lcldlm <= lm)) return fail(GEOSRAD_EINVAL, "super-layer levels must satisfy 1 < lcldmh < lcldlm <= lm");
        bool any = false;
        for (int k = 0; k < GEOSRAD_SWHB_NOUT; k++) any = any || out[k];
        if (!any) return GEOSRAD_OK;
        for (int k = 0; k < GEOSRAD_SWHB_NIN; k++)
            if (!in[k]) return fail(GEOSRAD_EINVAL, "null input field");
        HbArgs<R> H{};
        H.lm = lm; H.ld = ncol; H.doy = doy; H.lcldmh = lcldmh; H.lcldlm = lcldlm;
        // MAPL_GRAV, MAPL_RGAS = MAPL_RUNIV / MAPL_AIRMW (MAPL_Constants)
        H.grav = (R)(consts ? consts[GEOSRAD_SWHB_C_GRAV] : 9.80665); H.rgas = (R)(consts ? consts[GEOSRAD_SWHB_C_RGAS] : 8314.47 / 28.965);
        H.cwp_tiny = (R)1.e-20;                                       // (:7177)
        const int nc_max = chunk_cols(ncol);
        const char *ab = getenv("GEOSRAD_SWHB_COMPACT");              // A/B of the compaction only (profiles/r08_sw_cldhb.md)
        const bool compact = ab ? atoi(ab) != 0 : SWHB_COMPACT;
        int32_t *perm, *nclear;
        auto carve = [&](Carve c) {
            const size_t cl = (size_t)lm * nc_max;
            H.alpha = c.take<R>(cl); H.rcorr = c.take<R>(cl);
            H.cf0 = c.take<uint16_t>(nc_max); H.cf1 = c.take<uint16_t>(nc_max); H.cloudy = c.take<uint8_t>(nc_max);
            perm = c.take<int32_t>(compact ? nc_max : 0); nclear = c.take<int32_t>(compact ? 1 + part_blocks(nc_max) : 0);
            H.cnt = c.take<int32_t>((size_t)4 * nc_max);
            return c.off;
        };
        const size_t need = carve(Carve());
        if (d_ws_hb.reserve(need) != hipSuccess)
            return fail(GEOSRAD_ENOMEM, "hipMalloc of the CLD??SWHB workspace failed (" + std::to_string(need >> 20) + " MiB); lower it with geosrad_set_chunk()");
        carve(Carve(d_ws_hb));
        if (compact) { H.perm = perm; H.nclear = nclear; }
        McPlan MP; int nseg = 0;
        if (const int rc = mc_plan(1, HB_NSUB, lm, MP, nseg)) return rc;
        const LwDev<R> *dT = d_T;
        return chunk_walk(ncol, nc_max, [&](int c0, int nc) {
            H.ncol = nc;
            H.fcld = colp(in[GEOSRAD_SWHB_FCLD], c0); H.ple = colp(in[GEOSRAD_SWHB_PLE], c0); H.t = colp(in[GEOSRAD_SWHB_T], c0);
            H.qi = colp(in[GEOSRAD_SWHB_QI], c0); H.ql = colp(in[GEOSRAD_SWHB_QL], c0); H.lats = colp(in[GEOSRAD_SWHB_LATS], c0);
            for (int k = 0; k < GEOSRAD_SWHB_NOUT; k++) H.out[k] = colp(out[k], c0);
            hipLaunchKernelGGL((k_swhb_prep<R>), dim3(grid256(nc)), dim3(256), 0, st, H, dT);
            if (compact) launch_partition(st, nc, H.cloudy, perm, nclear);
            hipLaunchKernelGGL((k_swhb_count<R>), dim3(xcd_grid(nc, 64, nseg)), dim3(64), 0, st, H, MP, dT);
            hipLaunchKernelGGL((k_swhb_export<R>), dim3(grid256(nc)), dim3(256), 0, st, H);
            return GEOSRAD_OK;
        });
    }

    // ---- lit-column compaction (GEOS_SolarGridComp.F90:3686, PackIt / UnPackIt :7753-7799) --------------------------------------
    int lit_index_dev(hipStream_t st, int ncol, const void *zth, int32_t *idx, int32_t *pos, int32_t *nlit_dev, int *nlit_host) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || !zth || !idx || !pos || !nlit_dev) return fail(GEOSRAD_EINVAL, "lit_index: bad arguments");
        hipLaunchKernelGGL(k_lit_index<R>, dim3(1), dim3(1024), 0, st, ncol, (const R *)zth, idx, pos, nlit_dev);
        HIPCHK(hipGetLastError());
        if (nlit_host) {      // the caller sizes the packed call with it (NumLit = count(daytime) in the GridComp)
            int32_t v = 0;
            HIPCHK(hipMemcpyAsync(&v, nlit_dev, sizeof v, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            *nlit_host = v;
        }
        return GEOSRAD_OK;
    }
    int lit_pack_dev(hipStream_t st, int pdim, int udim, int nlev, const int32_t *idx, const int32_t *nlit_dev, const void *unpacked,
                     void *packed) override
    {
        HIPCHK(hipSetDevice(device));
        if (pdim <= 0 || udim <= 0 || nlev <= 0 || !idx || !nlit_dev || !unpacked || !packed) return fail(GEOSRAD_EINVAL, "lit_pack: bad arguments");
        const int nmax = pdim < udim ? pdim : udim;
        hipLaunchKernelGGL(k_lit_pack<R>, dim3(grid256(nmax), nlev), dim3(256), 0, st, pdim, udim, idx, nlit_dev,
                           (const R *)unpacked, (R *)packed);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int lit_unpack_dev(hipStream_t st, int pdim, int udim, int nlev, const int32_t *pos, const void *packed, void *unpacked, int use_default,
                       double dflt) override
    {
        HIPCHK(hipSetDevice(device));
        if (pdim <= 0 || udim <= 0 || nlev <= 0 || !pos || !unpacked || !packed) return fail(GEOSRAD_EINVAL, "lit_unpack: bad arguments");
        hipLaunchKernelGGL(k_lit_unpack<R>, dim3(grid256(udim), nlev), dim3(256), 0, st, pdim, udim, pos, (const R *)packed,
                           (R *)unpacked, use_default, (R)dflt);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int rad_tendencies_dev(hipStream_t st, int ncol, int lm, double grav, double cp, const void *const *in, void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/lm");
        RadTend<R> P{};
        P.ncol = ncol; P.lm = lm; P.grav = (R)grav; P.cp = (R)cp;
        bind(P, in, out);
        auto need = [&](const R *o, const R *a, const R *b = (const R *)1, const R *c = (const R *)1) { return !o || (a && b && c); };
        const bool any3 = P.radlw || P.radsw || P.radlwc || P.radswc || P.radswna || P.radlwcna || P.radswcna;
        const bool ok = need(P.dtdt, P.flw, P.fsw) && (!any3 || P.ple) && need(P.radlw, P.flw) && need(P.radsw, P.fsw) &&
                        need(P.radlwc, P.flwclr) && need(P.radswc, P.fswclr) && need(P.radswna, P.fswna) && need(P.radlwcna, P.fla) &&
                        need(P.radswcna, P.fscna) && need(P.blw, P.dsfdts) && need(P.alw, P.sfcem, P.dsfdts, P.trd) &&
                        need(P.radsrf, P.fsw, P.flw);
        if (!ok) return fail(GEOSRAD_EINVAL, "an export was requested without the field it is computed from");
        const bool wide = wide16(ncol, {{in, GEOSRAD_RT_NIN}, {out, GEOSRAD_RT_NOUT}});
        LAUNCH_WIDE(k_rad_tendencies, wide, ncol, lm, st, P);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int check(hipStream_t st, int which = -1) override
    {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamSynchronize(st));
        uint32_t e2[7] = {0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpy(e2, d_err, 28, hipMemcpyDeviceToHost));
        // slot 0 = RRTMG_LW (+ McICA), slot 1 = RRTMG_SW; the Chou schemes have no input assertions (neither has the reference).
        // The host-pointer entry points look at their own solver's slot only (a flag left by an unchecked `_dev` call of the other
        // solver is that call's to report); geosrad_check reports either.  Only the slot that is reported is cleared - with the two
        // solvers on two streams the other one's flag stays up for the check of its own stream - and it is cleared in stream order
        // on `st`, so a kernel of the other solver running on another stream cannot lose a bit to it.
        // slot 3 = the range check of ICARUS (icarus.f:403-455), slot 4 = that of MODIS (modis_simulator.F90:202-206), reported last
        // (slot 2 is k_chou_prep's and is not looked at here); slot 5 = the range check of the lidar simulator, reported after MODIS's;
        // slot 6 = that of the radar's gaseous attenuation (geosrad_radar_gases), reported after the lidar's
        for (int k : {0, 1, 3, 4, 5, 6})
            if (which >= 0 && which != k) e2[k] = 0;
        if (!e2[0] && !e2[1] && !e2[3] && !e2[4] && !e2[5] && !e2[6]) return GEOSRAD_OK;
        HIPCHK(hipMemsetAsync(d_err + (e2[1] ? 1 : e2[0] ? 0 : e2[3] ? 3 : e2[4] ? 4 : e2[5] ? 5 : 6), 0, 4, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!e2[0] && !e2[1] && !e2[3] && !e2[4] && !e2[5]) {
            static const char *RD_NAMES[RDERR_N] = {"p", "t", "zlev (heights must decrease strictly with the level)"};
            for (int k = 0; k < RDERR_N; k++)
                if (e2[6] & (1u << k)) return fail(GEOSRAD_EINPUT, std::string("Input values out of bounds (radar_gases): ") + RD_NAMES[k]);
            return fail(GEOSRAD_EINPUT, "device-side input check failed (radar_gases)");
        }
        if (!e2[0] && !e2[1] && !e2[3] && !e2[4]) {
            if (e2[5] & (1u << LDERR_P)) return fail(GEOSRAD_EINPUT, "Input values out of bounds (lidar): p");
            if (e2[5] & (1u << LDERR_T)) return fail(GEOSRAD_EINPUT, "Input values out of bounds (lidar): t");
            return fail(GEOSRAD_EINPUT, "Input values out of bounds (lidar): a non-finite pnorm");
        }
        if (!e2[0] && !e2[1] && !e2[3]) {
            static const char *MD_NAMES[MDERR_N] = {"t", "p", "dtau_s", "dtau_c", "reff_lsliq", "reff_lsice", "reff_cvliq", "reff_cvice"};
            for (int k = 0; k < MDERR_N; k++)
                if (e2[4] & (1u << k)) return fail(GEOSRAD_EINPUT, std::string("Input values out of bounds: ") + MD_NAMES[k]);
            return fail(GEOSRAD_EINPUT, "device-side input check failed (modis)");
        }
        if (!e2[0] && !e2[1]) {
            static const char *IC_NAMES[6] = {"cc", "conv", "dtau_s", "dtau_c", "dem_s", "dem_c"};
            for (int k = 0; k < 6; k++)
                if (e2[3] & (1u << k)) return fail(GEOSRAD_EINPUT, std::string("Input variable out of range: ") + IC_NAMES[k]);
            return fail(GEOSRAD_EINPUT, "device-side input check failed (icarus)");
        }
        if (e2[1]) {   // RRTMG_SW input assertions (SW/rrtmg_sw_rad.F90:365-383)
            static const char *SW_NEG_NAMES[12] = {"play", "tlay", "h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "o2vmr", "cld", "ciwp", "clwp", "rei", "rel"};
            for (int k = 0; k < 12; k++)
                if (e2[1] & (1u << k)) return fail(GEOSRAD_EINPUT, std::string("negative values in input: ") + SW_NEG_NAMES[k]);
            if (e2[1] & (1u << SWERR_PLEV)) return fail(GEOSRAD_EINPUT, "negative values in input: plev");
            if (e2[1] & (1u << SWERR_ALB)) return fail(GEOSRAD_EINPUT, "negative values in input: surface albedo");
            if (e2[1] & (1u << SWERR_AER)) return fail(GEOSRAD_EINPUT, "negative values in input: aerosol optical properties");
            return fail(GEOSRAD_EINPUT, "device-side input check failed (rrtmg_sw)");
        }
        const uint32_t e = e2[0];
        for (int k = 0; k < 21; k++)
            if (e & (1u << k)) return fail(GEOSRAD_EINPUT, std::string("negative values in input: ") + LW_NEG_NAMES[k]);
        if (e & (1u << ERR_PRESSURE_ORDER)) return fail(GEOSRAD_EINPUT, "RRTMG LW pressure misordering");
        if (e & (1u << ERR_ICE_RADIUS_HI)) return fail(GEOSRAD_EINPUT, "cldprmc: iceflag: excessive high-radius extrapolation forbidden!");
        if (e & (1u << ERR_ICE_RADIUS_LO)) return fail(GEOSRAD_EINPUT, "cldprmc: iceflag: excessive low-radius extrapolation forbidden!");
        if (e & (1u << ERR_LIQ_RADIUS_HI)) return fail(GEOSRAD_EINPUT, "cldprmc: liqflag 1: excessive high-radius extrapolation forbidden!");
        if (e & (1u << ERR_LIQ_RADIUS_LO)) return fail(GEOSRAD_EINPUT, "cldprmc: liqflag 1: excessive low-radius extrapolation forbidden!");
        return fail(GEOSRAD_EINPUT, "device-side input check failed");
    }

    // host-pointer entry points start from a clean slot of their own solver (stream-ordered on the internal stream)
    int clear_slot(int which) { HIPCHK(hipMemsetAsync(d_err + which, 0, 4, stream)); return GEOSRAD_OK; }

    // One host-pointer call through the chunk pipeline (pinned staging + host_pipeline): run(stream, columns) enqueues the solver for one
    // chunk, whose device arrays are where H.add() said.  which: the solver's slot of input assertions (0 RRTMG_LW, 1 RRTMG_SW) - the
    // call starts from a clean slot and ends with its check(), which turns a flagged chunk into the reference's message; -1: a scheme
    // without assertions, the caller synchronises.
    int host_call(int ncol, HostArrs &H, int which, const std::function<int(hipStream_t, int)> &run)
    {
        return host_call_at(ncol, H, which, [&](hipStream_t st, int nc, int) { return run(st, nc); });
    }
    // the same for a solver that has to know where in the call its chunk lies: run(stream, columns, first column)
    int host_call_at(int ncol, HostArrs &H, int which, const std::function<int(hipStream_t, int, int)> &run)
    {
        auto chunk = [&](hipStream_t st, int nc, int c0, char *dev, int) -> int {
            for (size_t i = 0; i < H.arrs.size(); i++) *H.at[i] = dev + H.arrs[i].off;
            return run(st, nc, c0);
        };
        if (which < 0) return host_pipeline(ncol, H.arrs, chunk);
        int rc = clear_slot(which);
        if (rc) return rc;
        rc = host_pipeline(ncol, H.arrs, chunk, d_err + which);
        if (rc && rc != PIPE_FLAGGED) return rc;
        return check(stream, which);
    }

    // ---- RRTMG_LW, host pointers --------------------------------------------------------------------------------
    // taug / pfracs (the geosrad_rrtmg_lw_taumol stage dump): per-column records behind the regular outputs.  A test hook for small
    // batches: each record is nlay x 140 reals (40 KB a column in fp32), and the three device and pinned slots are sized for
    // min(ncol, 16 384) columns of them - 1.3 GB a slot for the two arrays at a full chunk.
    int lw_host(int ncol, int nlay, int dudTs, const void *const *in, int iceflg, int liqflg, int dyofyr, int cloudLM, int cloudMH,
                int32_t *clearCounts, void *const *out, const int32_t *band_output, void *taug, void *pfracs) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || nlay <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/nlay");
        if (const int rc = lw_check_arrays(in, out)) return rc;
        bool any_bo = false;
        if (band_output) for (int b = 0; b < 16; b++) any_bo |= band_output[b] != 0;
        const size_t L = (size_t)nlay;
        HostArrs H(sizeof(R));
        const void *din[I_NIN] = {};
        void *dout[O_NOUT] = {}, *dcc = nullptr, *ddump[2] = {};
        for (int k = 0; k < I_NIN; k++) if (in[k]) H.add(in[k], nullptr, lw_in_shape(k, L), &din[k]);
        // olrb / dolrb_dTs: the reference leaves un-requested bands untouched, so the caller's content makes the round trip
        for (int k : {O_OLRB, O_DOLRB})
            if (any_bo && out[k] && (k == O_OLRB || dudTs)) H.add(out[k], out[k], lw_out_shape(k, L), &dout[k]);
        for (int k = 0; k < O_OLRB; k++)
            if (out[k] && (dudTs || (k != O_DUFLX && k != O_DUFLXC))) H.add(nullptr, out[k], lw_out_shape(k, L), &dout[k]);
        for (int k = O_UFLX_NA; k < O_NOUT; k++)
            if (out[k] && (dudTs || k < O_DUFLX_NA)) H.add(nullptr, out[k], lw_out_shape(k, L), &dout[k]);
        H.add_clear_counts(clearCounts, &dcc);
        if (taug) { H.add(nullptr, taug, lw_dump_shape(L), &ddump[0]); H.add(nullptr, pfracs, lw_dump_shape(L), &ddump[1]); }
        return host_call(ncol, H, 0, [&](hipStream_t st, int nc) {
            return lw_dev(st, nc, nlay, dudTs, din, iceflg, liqflg, dyofyr, cloudLM, cloudMH, (int32_t *)dcc, dout, band_output, ddump[0],
                          ddump[1], nullptr);
        });
    }

    // =====================================================================================================
    // RRTMG_SW
    // =====================================================================================================
    int set_tables_sw(const void *blob, size_t nbytes) override
    {
        HIPCHK(hipSetDevice(device));
        Blob B;
        if (!B.parse(blob, nbytes)) return fail(GEOSRAD_ETABLE, B.err);
        if (B.realbytes != (int)sizeof(R))
            return fail(GEOSRAD_ETABLE, "table blob real size does not match the context's real_kind");
        TableStage<R> S(B);
        SwDev<R> &T = h_S;
        memset(&T, 0, sizeof(T));
        static const int ng[15] = {0, 6, 12, 8, 8, 10, 10, 2, 10, 8, 6, 6, 8, 6, 12};
        static const int rowsa[15] = {0, 585, 585, 585, 585, 65, 585, 585, 65, 585, 65, 0, 65, 585, 65};
        static const int rowsb[15] = {0, 235, 1175, 235, 235, 235, 1175, 235, 0, 235, 0, 0, 235, 1175, 235};
        static const int nfor[15] = {0, 3, 4, 3, 3, 4, 4, 3, 3, 3, 0, 0, 0, 0, 4};
        static const int nsrc[15] = {0, 1, 5, 9, 9, 1, 9, 9, 1, 9, 1, 1, 1, 5, 1};
        char nm[64];
        for (int b = 1; b <= NB_SW; b++) {
            SwBandTab<R> &bt = T.b[b];
            auto N = [&](const char *s) { snprintf(nm, sizeof nm, "b%02d_%s", b + 15, s); return std::string(nm); };
            if (rowsa[b]) S.tr2(&bt.absa, N("absa"), rowsa[b], ng[b]);
            if (rowsb[b]) S.tr2(&bt.absb, N("absb"), rowsb[b], ng[b]);
            if (nfor[b]) { S.tr2(&bt.selfref, N("selfref"), 10, ng[b]); S.tr2(&bt.forref, N("forref"), nfor[b], ng[b]); }
            S.rows(&bt.sflux, N("sfluxref"), ng[b], nsrc[b]); S.rows(&bt.irrad, N("irradnce"), ng[b], nsrc[b]);
            S.rows(&bt.facb, N("facbrght"), ng[b], nsrc[b]); S.rows(&bt.snsp, N("snsptdrk"), ng[b], nsrc[b]);
            const int jb = b + 15;
            if (jb == 24) { S.rows(&bt.rayl, N("rayla"), ng[b], 9); S.rows(&bt.raylb, N("raylb"), ng[b], 1); }
            else if (jb == 23 || jb == 25 || jb == 26 || jb == 27) S.rows(&bt.rayl, N("rayl"), ng[b], 1);
            else S.splat(&bt.rayl, N("rayl"), ng[b]);
            if (jb == 20) S.rows(&bt.x0, N("absch4"), ng[b], 1);
            if (jb == 24 || jb == 25) { S.rows(&bt.x0, N("abso3a"), ng[b], 1); S.rows(&bt.x1, N("abso3b"), ng[b], 1); }
            if (jb == 29) { S.rows(&bt.x0, N("absco2"), ng[b], 1); S.rows(&bt.x1, N("absh2o"), ng[b], 1); }
        }
        S.raw(&T.preflog, "preflog", 59); S.raw(&T.tref, "tref", 59);
        S.raw(&T.extliq1, "extliq1", 58 * 14); S.raw(&T.ssaliq1, "ssaliq1", 58 * 14); S.raw(&T.asyliq1, "asyliq1", 58 * 14);
        S.raw(&T.extice2, "extice2", 43 * 14); S.raw(&T.ssaice2, "ssaice2", 43 * 14); S.raw(&T.asyice2, "asyice2", 43 * 14);
        S.raw(&T.extice3, "extice3", 46 * 14); S.raw(&T.ssaice3, "ssaice3", 46 * 14); S.raw(&T.asyice3, "asyice3", 46 * 14);
        S.raw(&T.fdlice3, "fdlice3", 46 * 14);
        S.raw(&T.extice4, "extice4", 200 * 14); S.raw(&T.ssaice4, "ssaice4", 200 * 14); S.raw(&T.asyice4, "asyice4", 200 * 14);
        {
            const char *bn[6] = {"abari", "bbari", "cbari", "dbari", "ebari", "fbari"};
            R *dst[6] = {T.abari, T.bbari, T.cbari, T.dbari, T.ebari, T.fbari};
            for (int k = 0; k < 6; k++) { const R *s = S.get(bn[k], 5); if (s) memcpy(dst[k], s, 5 * sizeof(R)); }
        }
        T.oneminus = S.scalar("oneminus"); T.grav = S.scalar("grav"); T.avogad = S.scalar("avogad"); T.rrsw_scon = S.scalar("rrsw_scon");
        T.Iint = S.scalar("Iint"); T.Fint = S.scalar("Fint"); T.Sint = S.scalar("Sint");
        T.Mg_avg = S.scalar("Mg_avg"); T.Mg_0 = S.scalar("Mg_0"); T.SB_avg = S.scalar("SB_avg"); T.SB_0 = S.scalar("SB_0");
        {   // AvgCyc11 of the two indices (isolvar == 1 only; blobs written before round 4 lack them: that option is then refused)
            avgcyc_mg.clear(); avgcyc_sb.clear();
            if (B.e.count("mgavgcyc") && B.e.count("sbavgcyc")) {
                const R *m = S.get("mgavgcyc", 134), *q = S.get("sbavgcyc", 134);
                if (m && q) { avgcyc_mg.assign(m, m + 134); avgcyc_sb.assign(q, q + 134); }
            }
        }
        {
            int32_t icxa[14], ngb[112];
            if (S.ints("icxa", 14, icxa)) for (int b = 1; b <= NB_SW; b++) T.icxa[b] = icxa[b - 1];
            // the band <-> g-point map is compiled into the kernels; refuse tables that disagree
            if (S.ints("ngb", 112, ngb)) {
                int g = 0;
                for (int b = 1; b <= NB_SW; b++) for (int k = 0; k < ng[b]; k++, g++) if (ngb[g] != b + 15) S.missing += "ngb(mismatch) ";
            }
        }
        if (!S.missing.empty()) return fail(GEOSRAD_ETABLE, "missing/ill-shaped table entries: " + S.missing);
        HIPCHK(d_tab_sw.resize(S.stage.size()));
        HIPCHK(hipMemcpy(d_tab_sw, S.stage.data(), d_tab_sw.bytes, hipMemcpyHostToDevice));
        for (auto &f : S.fix) *f.first = (const R *)(d_tab_sw + f.second);
        // sw_eval reaches a band's upper-atmosphere tables as the lower ones' base + a 32-bit byte offset (one allocation, staged in this order)
        for (int b = 1; b <= NB_SW; b++)
            if ((T.b[b].absb && T.b[b].absb < T.b[b].absa) || (T.b[b].x1 && T.b[b].x1 < T.b[b].x0) || d_tab_sw.bytes >= ((size_t)1 << 32))
                return fail(GEOSRAD_ETABLE, "internal: RRTMG_SW table staging order");
        HIPCHK(hipMemcpy(d_S, &h_S, sizeof(SwDev<R>), hipMemcpyHostToDevice));
        have_sw = true;
        return GEOSRAD_OK;
    }

    // the SW workspace of nc columns, straight into the kernels' arguments (+ rvsum, which is none of them): on Carve() the bytes it takes,
    // on Carve(d_ws_sw) its planes
    size_t ws_layout_sw(int nc, int nlay, SwArgs<R> &w, R *&rvsum, Carve c, int planes, bool radval) const
    {
        const size_t cl = (size_t)nlay * nc;
        w.sc = c.take<R>(SW_NFIELD * cl);
        w.scidx = c.take<uint32_t>(cl);
        w.colcloudy = c.take<uint8_t>(nc);
        w.perm = c.take<int32_t>(nc);
        w.nclear = c.take<int32_t>(1 + part_blocks(nc));      // + the tile counts of the partition (launch_partition)
        w.laycloudy = c.take<uint8_t>(cl);
        w.alpha = c.take<R>(cl);
        w.rcorr = c.take<R>(cl);
        w.taucmc = c.take<R>(NG_SW * cl);
        w.ssacmc = c.take<R>(NG_SW * cl);
        w.asmcmc = c.take<R>(NG_SW * cl);
        w.cotsum = c.take<R>((size_t)3 * NG_SW * nc);
        // parked planes of the band sweeps: k_sw_reform fp32 5 (gas optical depth + 2 x 2 upward reflectances), fp64 15 (no gas optical
        // depth, 2 x 5 layer properties instead); k_sw_bands 14
        // (the stage-dump instantiation is always k_sw_bands: sw_planes(true))
        w.cell = c.take<R>((size_t)planes * NG_SW * nlay * (((size_t)nc + 255) & ~(size_t)255));
        // partial fluxes per slot: the units of k_sw_reform's mapping (23 fp32 / 32 fp64), which also cover the 14 bands of k_sw_bands (the
        // stage-dump hook always runs that kernel); 14 when GEOSRAD_SW_PATH=bands
        const size_t slots = sw_path == 2 ? (size_t)(sw_reform_nslot<R>() > NB_SW ? sw_reform_nslot<R>() : NB_SW) : (size_t)NB_SW;
        w.part = c.take<R>((size_t)4 * slots * (nlay + 1) * nc);
        w.bsfc = c.take<R>((size_t)3 * slots * nc);
        w.cot = c.take<R>((size_t)8 * 6 * nc);
        // SOLAR_RADVAL layer sums of k_mcica<R, 2, true>, [3][15][20][nc]: only once a geosrad_rrtmg_sw_radval* call asked for them
        rvsum = radval ? c.take<R>((size_t)3 * RV_NSUM * RV_NPAR * nc) : nullptr;
        return c.off;
    }
    int sw_planes(bool dbg) const { return (sw_path == 2 && !dbg) ? (sizeof(R) == 4 ? 5 : 15) : 14; }
    int ensure_ws_sw(int nc, int nlay, int planes, bool radval)
    {
        if (d_ws_sw && nc <= ws_sw_ncol && nlay == ws_sw_nlay && planes <= ws_sw_planes && (ws_sw_radval || !radval)) return GEOSRAD_OK;
        if (planes < ws_sw_planes) planes = ws_sw_planes;
        radval = radval || ws_sw_radval;
        const int want = (d_ws_sw && nlay == ws_sw_nlay && nc < ws_sw_ncol) ? ws_sw_ncol : nc;
        SwArgs<R> w; R *rvsum;
        const size_t need = ws_layout_sw(want, nlay, w, rvsum, Carve(), planes, radval);
        if (d_ws_sw.resize(need) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the SW workspace failed (" + std::to_string(need >> 20) +
                                                         " MiB); lower it with geosrad_set_chunk()");
        ws_sw_ncol = want; ws_sw_nlay = nlay; ws_sw_planes = planes; ws_sw_radval = radval;
        return GEOSRAD_OK;
    }

    // solar variability block of the driver (SW/rrtmg_sw_rad.F90:893-1127), scalars only
    // NRLSSI2's host routines for isolvar == 1 (SW/NRLSSI2.F90; nsolfrac = 134, intrvl_len = 1 / 132) - false where the reference error-stops
    static bool nrl_adjust(R solcycfr, const R *indsolvar, R *scl)          // adjust_solcyc_amplitudes (:236-271)
    {
        const R fmin = (R)0.0189, fmax = (R)0.3750, dmin2max = fmax - fmin, dmax2min = (R)1. - dmin2max;
        if (solcycfr >= 0 && solcycfr < fmin) {
            const R wgt = (solcycfr + (R)1. - fmax) / dmax2min;
            scl[0] = indsolvar[0] + wgt * ((R)1. - indsolvar[0]); scl[1] = indsolvar[1] + wgt * ((R)1. - indsolvar[1]);
        } else if (solcycfr >= fmin && solcycfr <= fmax) {
            const R wgt = (solcycfr - fmin) / dmin2max;
            scl[0] = (R)1. + wgt * (indsolvar[0] - (R)1.); scl[1] = (R)1. + wgt * (indsolvar[1] - (R)1.);
        } else if (solcycfr > fmax && solcycfr <= 1) {
            const R wgt = (solcycfr - fmax) / dmax2min;
            scl[0] = indsolvar[0] + wgt * ((R)1. - indsolvar[0]); scl[1] = indsolvar[1] + wgt * ((R)1. - indsolvar[1]);
        } else return false;
        return true;
    }
    bool nrl_interp(R solcycfr, R &Mg, R &SB) const                         // interpolate_indices (:277-332)
    {
        const R il = (R)1.0 / (R)132, ilh = (R)0.5 * il;
        const R *mg = avgcyc_mg.data() - 1, *sb = avgcyc_sb.data() - 1;     // 1-based like the reference
        if (solcycfr > 0 && solcycfr < 1) {
            int sfid; R lo, hi;
            if (solcycfr <= ilh) { sfid = 1; lo = 0; hi = ilh; }
            else if (solcycfr > ilh && solcycfr < (R)1. - ilh) { sfid = (int)std::floor((solcycfr - ilh) * (R)132) + 2; lo = (R)(sfid - 2) * il + ilh; hi = lo + il; }
            else { sfid = 133; lo = (R)1. - ilh; hi = 1; }
            const R f = (solcycfr - lo) / (hi - lo);
            Mg = mg[sfid] + f * (mg[sfid + 1] - mg[sfid]); SB = sb[sfid] + f * (sb[sfid + 1] - sb[sfid]);
        } else if (solcycfr == 0) { Mg = mg[1]; SB = sb[1]; }
        else if (solcycfr == 1) { Mg = mg[134]; SB = sb[134]; }
        else return false;
        return true;
    }
    void nrl_means(const R *ind_opt, R &mean_f, R &mean_s) const             // initialize_NRLSSI2, isolvar == 1 (:160-232)
    {
        const SwDev<R> &T = h_S;
        const R il = (R)1.0 / (R)132, ilh = (R)0.5 * il;
        const R *mg = avgcyc_mg.data() - 1, *sb = avgcyc_sb.data() - 1;
        const R ind[2] = {ind_opt ? ind_opt[0] : (R)1, ind_opt ? ind_opt[1] : (R)1};
        mean_f = 1; mean_s = 1;
        const bool s1 = ind[0] != 1, s2 = ind[1] != 1;
        if (!s1 && !s2) return;
        const R m1 = ((R)1. + ind[0]) / (R)2., m2 = ((R)1. + ind[1]) / (R)2.;
        R a1 = 0, a2 = 0, scl[2], fr = ilh;
        for (int n = 2; n <= 133; n++) {
            nrl_adjust(fr, ind, scl);
            if (s1) a1 = a1 + scl[0] * mg[n];
            if (s2) a2 = a2 + scl[1] * sb[n];
            fr = fr + il;
        }
        if (s1) { a1 = a1 / (R)132; mean_f = (a1 - m1 * T.Mg_0) / (T.Mg_avg - T.Mg_0); }
        if (s2) { a2 = a2 / (R)132; mean_s = (a2 - m2 * T.SB_0) / (T.SB_avg - T.SB_0); }
    }

    int sw_solar(double scon_d, double adjes_d, int isolvar, const R *bndscl, const R *indsolvar, const R *solcycfrac, SwSolar<R> &SV)
    {
        const SwDev<R> &T = h_S;
        const R scon = (R)scon_d, adjes = (R)adjes_d;
        R solvar[NB_SW + 1];
        for (int b = 0; b <= NB_SW; b++) { solvar[b] = 1; SV.svar_bnd[b] = 1; SV.adjflux[b] = 1; }
        SV.isolvar = isolvar; SV.svar_f = 1; SV.svar_s = 1; SV.svar_i = 1;
        if (isolvar != -1 && isolvar != 0 && isolvar != 1 && isolvar != 2 && isolvar != 3) return fail(GEOSRAD_EINPUT, "invalid isolvar");
        if (isolvar == 1) {
            // position in AvgCyc11 from solcycfrac, amplitude scaling from indsolvar (rrtmg_sw_rad.F90:906-930, :994-1008, :1060-1079)
            if (!solcycfrac) return fail(GEOSRAD_EINPUT, "isolvar == 1 requires solcycfrac present!");
            if (avgcyc_mg.size() != 134 || avgcyc_sb.size() != 134)
                return fail(GEOSRAD_ETABLE, "isolvar == 1 needs the mgavgcyc / sbavgcyc entries of the RRTMG_SW table blob");
            if (scon < 0) return fail(GEOSRAD_EINPUT, "scon must be >= 0");
            const R fr = *solcycfrac;
            R scl[2] = {1, 1}, Mg_now, SB_now, mean_f, mean_s;
            if (indsolvar && (indsolvar[0] != 1 || indsolvar[1] != 1))
                if (!nrl_adjust(fr, indsolvar, scl)) return fail(GEOSRAD_EINPUT, "RRTMG_SW: solcycfr must be in [0,1]");
            nrl_means(indsolvar, mean_f, mean_s);
            if (!nrl_interp(fr, Mg_now, SB_now)) return fail(GEOSRAD_EINPUT, "RRTMG_SW: solcycfr must be in [0,1]");
            SV.svar_f = scl[0] * (Mg_now - T.Mg_0) / (T.Mg_avg - T.Mg_0);
            SV.svar_s = scl[1] * (SB_now - T.SB_0) / (T.SB_avg - T.SB_0);
            SV.svar_i = scon == 0 ? (R)1 : (scon - (mean_f * T.Fint + mean_s * T.Sint)) / T.Iint;
        }
        R ndx0 = T.Mg_avg, ndx1 = T.SB_avg;
        if (isolvar == 2 && indsolvar) { ndx0 = indsolvar[0]; ndx1 = indsolvar[1]; }
        if (scon == 0) {
            if (isolvar == -1) { if (bndscl) for (int b = 1; b <= NB_SW; b++) solvar[b] = bndscl[b - 1]; }
            else if (isolvar == 2) { SV.svar_f = (ndx0 - T.Mg_0) / (T.Mg_avg - T.Mg_0); SV.svar_s = (ndx1 - T.SB_0) / (T.SB_avg - T.SB_0); SV.svar_i = 1; }
            else if (isolvar == 3) { if (bndscl) for (int b = 1; b <= NB_SW; b++) solvar[b] = bndscl[b - 1];
                for (int b = 1; b <= NB_SW; b++) SV.svar_bnd[b] = solvar[b]; }
        } else if (scon > 0) {
            const R scon_int = T.Fint + T.Sint + T.Iint;
            if (isolvar == -1) { for (int b = 1; b <= NB_SW; b++) solvar[b] = scon / T.rrsw_scon;
                if (bndscl) for (int b = 1; b <= NB_SW; b++) solvar[b] = solvar[b] * bndscl[b - 1]; }
            else if (isolvar == 0) { const R r = scon / scon_int; SV.svar_f = r; SV.svar_s = r; SV.svar_i = r; }
            else if (isolvar == 2) { SV.svar_f = (ndx0 - T.Mg_0) / (T.Mg_avg - T.Mg_0); SV.svar_s = (ndx1 - T.SB_0) / (T.SB_avg - T.SB_0);
                SV.svar_i = (scon - (SV.svar_f * T.Fint + SV.svar_s * T.Sint)) / T.Iint; }
            else { for (int b = 1; b <= NB_SW; b++) solvar[b] = scon / scon_int;
                if (bndscl) for (int b = 1; b <= NB_SW; b++) solvar[b] = solvar[b] * bndscl[b - 1];
                for (int b = 1; b <= NB_SW; b++) SV.svar_bnd[b] = solvar[b]; }
        } else return fail(GEOSRAD_EINPUT, "scon must be >= 0");
        for (int b = 1; b <= NB_SW; b++) SV.adjflux[b] = adjes;
        if (isolvar < 0) for (int b = 1; b <= NB_SW; b++) SV.adjflux[b] = SV.adjflux[b] * solvar[b];
        return GEOSRAD_OK;
    }

    // ---- RRTMG_SW, device pointers -------------------------------------------------------------------------
    int sw_dev(hipStream_t st, int ncol, int nlay, double scon, double adjes, int isolvar, const void *const *in, int iceflg, int liqflg,
               int dyofyr, int iaer, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *const *out, int do_drfband,
               const void *bndscl, const void *indsolvar, const void *solcycfrac, void *const *dbg, void *radval) override
    {
        return sw_run(st, ncol, nlay, scon, adjes, isolvar, in, iceflg, liqflg, dyofyr, iaer, cloudLM, cloudMH, normFlx, clearCounts, out,
                      do_drfband, bndscl, indsolvar, solcycfrac, dbg, nullptr, radval);
    }

    // RRTMG_SW band sweeps of one chunk and the reduction into out (SwOutIx order, SO_NOUT entries; one that is null is not written):
    // k_sw_reform (lane = (column, unit of g-points); fp32 re-forms the cell optics in its second sweep and parks 12 bytes per cell; in
    // fp64 the second two-stream - IEEE divisions, double-precision exp / sqrt - costs more than the parked bytes it would save, 32.5
    // against 29.4 ms per 97 200 columns, so that instantiation parks the layer properties too); GEOSRAD_SW_PATH=bands selects the first
    // mapping, k_sw_bands, and the stage dumps (dbg) always run its dumping instantiation
    bool sw_reform_on() const { return sw_path == 2; }
    int sw_sweeps(hipStream_t st, const SwArgs<R> &A, const SwSolar<R> &SV, void *const *out, int c0, bool dbg)
    {
        const dim3 blk(256), grid(band_grid(A.ncol, NB_SW));
        const bool reform = sw_reform_on() && !dbg;
        span_begin(8, st);
        if (dbg) {
            hipLaunchKernelGGL((k_sw_bands<R, true, true>), grid, blk, 0, st, A, h_S, SV);
        } else if (reform) {
            if (const int rc = hip_rc("sw_reform_launch", sw_reform_launch<R>(st, A, h_S, SV))) return rc;
        } else {
            hipLaunchKernelGGL((k_sw_bands<R, false, false>), grid, blk, 0, st, A, h_S, SV);
            hipLaunchKernelGGL((k_sw_bands<R, true, false>), grid, blk, 0, st, A, h_S, SV);
        }
        span_end(st);
        SwOut<R> O{};
        auto Q = [&](int k) { return colp(out[k], c0); };
        O.swuflx = Q(SO_UFLX); O.swdflx = Q(SO_DFLX); O.swuflxc = Q(SO_UFLXC); O.swdflxc = Q(SO_DFLXC);
        O.nirr = Q(SO_NIRR); O.nirf = Q(SO_NIRF); O.parr = Q(SO_PARR); O.parf = Q(SO_PARF); O.uvrr = Q(SO_UVRR); O.uvrf = Q(SO_UVRF);
        O.fswband = Q(SO_FSWBAND);
        for (int k = 0; k < 8; k++) O.cot[k] = Q(SO_COT0 + k);
        O.drband = Q(SO_DRBAND); O.dfband = Q(SO_DFBAND);
        span_begin(9, st);
        if (reform) { if (const int rc = hip_rc("sw_reform_reduce", sw_reform_reduce<R>(st, A, O))) return rc; }
        else hipLaunchKernelGGL(k_sw_reduce<R>, dim3(grid256(A.ncol), A.nlay + 2), blk, 0, st, A, O);
        span_end(st);
        return GEOSRAD_OK;
    }

    // the array checks sw_host makes before it stages anything and sw_run makes in its own order
    int sw_check_options(int ncol, int nlay, int iceflg, int liqflg, int cloudLM, int cloudMH, int iaer)
    {
        if (!have_sw) return fail(GEOSRAD_EINVAL, "RRTMG_SW tables not set: call geosrad_set_tables_sw first (rrtmg_sw_ini)");
        if (ncol <= 0 || nlay < 4 || nlay > 203) return fail(GEOSRAD_EINVAL, "bad ncol/nlay (4 <= nlay <= mxlay = 203)");
        if (iceflg < 1 || iceflg > 4) return fail(GEOSRAD_EINPUT, "cldprmc_sw: invalid iceflag");
        if (liqflg != 1) return fail(GEOSRAD_EINPUT, "cldprmc_sw: invalid liqflag");
        if (cloudLM == cloudMH) return fail(GEOSRAD_EINPUT, "invalid pressure super-layers!");
        if (iaer != 0 && iaer != 10) return fail(GEOSRAD_EINPUT, "iaer must be 0 or 10");
        return GEOSRAD_OK;
    }
    int sw_check_arrays(const void *const *in, void *const *out, int iaer, int do_drfband)
    {
        for (int k = 0; k < S_NIN; k++)
            if (!in[k] && !((k == S_TAUAER || k == S_SSAAER || k == S_ASMAER) && iaer != 10)) return fail(GEOSRAD_EINVAL, "null input array");
        for (int k = 0; k < SO_DRBAND; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null output array");
        if (do_drfband && (!out[SO_DRBAND] || !out[SO_DFBAND])) return fail(GEOSRAD_EINVAL, "do_drfband set but drband/dfband null");
        return GEOSRAD_OK;
    }

    // sw_na_out (SwOutIx order, SO_NOUT entries, all of SO_UFLX .. SO_COT0 + 7 non-null) requests an additional pass without the aerosol
    // terms; radval ((GEOSRAD_RV_COUNT, ncol) device array) requests the SOLAR_RADVAL diagnostics: the RADVAL instantiation of k_mcica,
    // then k_sw_radval - once per call, they do not depend on the aerosols
    int sw_run(hipStream_t st, int ncol, int nlay, double scon, double adjes, int isolvar, const void *const *in, int iceflg, int liqflg,
               int dyofyr, int iaer, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *const *out, int do_drfband,
               const void *bndscl, const void *indsolvar, const void *solcycfrac, void *const *dbg, void *const *sw_na_out,
               void *radval = nullptr)
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = sw_check_options(ncol, nlay, iceflg, liqflg, cloudLM, cloudMH, iaer)) return rc;
        if (const int rc = sw_check_arrays(in, out, iaer, do_drfband)) return rc;
        if (radval && dbg) return fail(GEOSRAD_EINVAL, "the stage dumps do not produce the SOLAR_RADVAL diagnostics");
        SwSolar<R> SV;
        if (const int rc = sw_solar(scon, adjes, isolvar, (const R *)bndscl, (const R *)indsolvar, (const R *)solcycfrac, SV)) return rc;

        // one band's [layer][g<=12][column] plane must stay below 4 GiB (32-bit byte offsets)
        const int nc_max = chunk_cols(ncol, (long)(0xFFFFFFFFull / ((unsigned long long)nlay * 12ull * sizeof(R))) & ~255L);
        if (const int rc = ensure_ws_sw(nc_max, nlay, sw_planes(dbg != nullptr), radval != nullptr)) return rc;

        return chunk_walk(ncol, nc_max, [&](int c0, int nc) -> int {
            SwArgs<R> A{};
            R *rvsum;
            ws_layout_sw(nc, nlay, A, rvsum, Carve(d_ws_sw), ws_sw_planes, ws_sw_radval);
            A.ncol = nc; A.ld = ncol; A.nlay = nlay; A.iceflg = iceflg; A.liqflg = liqflg; A.doy = dyofyr; A.cloudLM = cloudLM;
            A.cloudMH = cloudMH; A.iaer = iaer; A.normFlx = normFlx; A.do_drfband = do_drfband;
            auto P = [&](int k) { return colp(in[k], c0); };
            A.play = P(S_PLAY); A.plev = P(S_PLEV); A.tlay = P(S_TLAY); A.h2o = P(S_H2O); A.o3 = P(S_O3); A.co2 = P(S_CO2);
            A.ch4 = P(S_CH4); A.o2 = P(S_O2); A.cld = P(S_CLD); A.ciwp = P(S_CIWP); A.clwp = P(S_CLWP); A.rei = P(S_REI);
            A.rel = P(S_REL); A.zm = P(S_ZM); A.alat = P(S_ALAT);
            A.tauaer = iaer == 10 ? P(S_TAUAER) : nullptr; A.ssaaer = iaer == 10 ? P(S_SSAAER) : nullptr;
            A.asmaer = iaer == 10 ? P(S_ASMAER) : nullptr;
            A.coszen = P(S_COSZEN); A.asdir = P(S_ASDIR); A.asdif = P(S_ASDIF); A.aldir = P(S_ALDIR); A.aldif = P(S_ALDIF);
            A.err = d_err + 1;
            A.clearCounts = clearCounts + c0;
            const size_t d0 = (size_t)c0 * NG_SW * nlay;      // a chunk's first record of the per-cell stage dumps
            if (dbg) { A.dbg_taug = (R *)dbg[0] + d0; A.dbg_taur = (R *)dbg[1] + d0; A.dbg_ssi = (R *)dbg[2] + (size_t)c0 * NG_SW; }
            if (const int e = rrtmg_front<2>(st, A, radval != nullptr, rvsum)) return e;
            const dim3 blk(256);
            const unsigned gx = grid256(nc);
            if (radval) {
                // the sub-columns are summed in the groups of the band sweeps' own cotd?? / cotn?? family (sw_radval_kernels.hpp)
                SwRvGroups G{};
                if (sw_reform_on()) {
                    int sz[RV_NPAR];
                    G.n = sw_reform_par_units<R>(sz);
                    for (int k = 0, e = 0; k < G.n; k++) { e += sz[k]; G.end[k] = e; }
                } else { G.n = 3; G.end[0] = 8; G.end[1] = 14; G.end[2] = 20; }
                hipLaunchKernelGGL(k_sw_radval<R>, dim3(gx, 4), blk, 0, st, A, h_S, SV, G, (const R *)rvsum, (R *)radval + c0);
            }
            if (dbg && dbg[3])       // cldprmc_sw stage dump (6-entry dbg of geosrad_rrtmg_sw_cldprmc)
                hipLaunchKernelGGL(k_sw_dump_cldprmc<R>, dim3(gx, nlay), blk, 0, st, A, (R *)dbg[3] + d0, (R *)dbg[4] + d0, (R *)dbg[5] + d0);
            if (const int e = sw_sweeps(st, A, SV, out, c0, dbg != nullptr)) return e;
            if (sw_na_out && !dbg) {
                // the GridComp's "no-aerosol" diagnostics (GEOS_SolarGridComp.F90:3249-3259 calls the whole of SORADCORE a second
                // time): same columns, same clouds (McICA is seeded by the pressures), same gas optical depths - only the band
                // sweeps and the reduction are repeated, without the aerosol terms; validation, setcoef and McICA are shared
                A.iaer = 0; A.do_drfband = 0;
                return sw_sweeps(st, A, SV, sw_na_out, c0, false);
            }
            return GEOSRAD_OK;
        });
    }

    // ---- RRTMG_SW, host pointers ---------------------------------------------------------------------------
    int sw_host(int ncol, int nlay, double scon, double adjes, int isolvar, const void *const *in, int iceflg, int liqflg, int dyofyr,
                int iaer, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *const *out, int do_drfband, const void *bndscl,
                const void *indsolvar, const void *solcycfrac, void *const *dbg, void *radval) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || nlay <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/nlay");
        if (radval && dbg) return fail(GEOSRAD_EINVAL, "the stage dumps do not produce the SOLAR_RADVAL diagnostics");
        if (const int rc = sw_check_arrays(in, out, iaer, do_drfband)) return rc;
        auto aer = [](int k) { return k == S_TAUAER || k == S_SSAAER || k == S_ASMAER; };
        const size_t L = (size_t)nlay;
        HostArrs H(sizeof(R));
        const void *din[S_NIN] = {};
        void *dout[SO_NOUT] = {}, *dcc = nullptr, *drv = nullptr, *ddump[6] = {};
        for (int k = 0; k < S_NIN; k++) if (in[k] && !(aer(k) && iaer != 10)) H.add(in[k], nullptr, sw_in_shape(k, L), &din[k]);
        for (int k = 0; k < SO_NOUT; k++) if (k < SO_DRBAND || do_drfband) H.add(nullptr, out[k], sw_out_shape(k, L), &dout[k]);
        H.add_clear_counts(clearCounts, &dcc);
        if (radval) H.add(nullptr, radval, {(size_t)GEOSRAD_RV_COUNT, 1}, &drv);
        // the stage dumps of geosrad_rrtmg_sw_taumol (taug, taur, ssi) and geosrad_rrtmg_sw_cldprmc (+ the three cloud planes): test
        // hooks for small batches, like lw_host's (up to five records of nlay x 112 reals a column in every staging slot)
        for (int k = 0; dbg && k < 6; k++) if (dbg[k]) H.add(nullptr, dbg[k], sw_dump_shape(k, L), &ddump[k]);
        return host_call(ncol, H, 1, [&](hipStream_t st, int nc) {
            return sw_dev(st, nc, nlay, scon, adjes, isolvar, din, iceflg, liqflg, dyofyr, iaer, cloudLM, cloudMH, normFlx, (int32_t *)dcc,
                          dout, do_drfband, bndscl, indsolvar, solcycfrac, dbg ? ddump : nullptr, drv);
        });
    }

    // =====================================================================================================
    // Chou-Suarez longwave (irrad)
    // =====================================================================================================
    int set_tables_chou_lw(const void *blob, size_t nbytes) override
    {
        HIPCHK(hipSetDevice(device));
        Blob B;
        if (!B.parse(blob, nbytes)) return fail(GEOSRAD_ETABLE, B.err);
        if (B.realbytes != (int)sizeof(R)) return fail(GEOSRAD_ETABLE, "table blob real size does not match the context's real_kind");
        TableStage<R> S(B);
        ChouDev<R> &T = h_C;
        memset(&T, 0, sizeof(T));
        auto cp = [&](R *dst, const char *nm, size_t n) { const R *s = S.get(nm, n); if (s) memcpy(dst, s, n * sizeof(R)); };
        cp(T.xkw, "xkw", 9); cp(T.xke, "xke", 9); cp(T.aw, "aw", 9); cp(T.bw, "bw", 9); cp(T.pm, "pm", 9);
        cp(T.fkw, "fkw", 54); cp(T.gkw, "gkw", 18); cp(T.cb, "cb", 60); cp(T.dcb, "dcb", 50);
        cp(T.aib, "aib_ir", 30); cp(T.awb, "awb_ir", 40); cp(T.aiw, "aiw_ir", 40); cp(T.aww, "aww_ir", 40); cp(T.aig, "aig_ir", 40);
        cp(T.awg, "awg_ir", 40);
        { int32_t mw[9]; if (S.ints("mw", 9, mw)) for (int k = 0; k < 9; k++) T.mw[k] = mw[k]; }
        T.w11 = S.scalar("w11"); T.w12 = S.scalar("w12"); T.w13 = S.scalar("w13"); T.p11 = S.scalar("p11"); T.p12 = S.scalar("p12");
        T.p13 = S.scalar("p13"); T.dwe = S.scalar("dwe"); T.dpe = S.scalar("dpe");
        S.raw(&T.c1, "c1", 26 * 30); S.raw(&T.c2, "c2", 26 * 30); S.raw(&T.c3, "c3", 26 * 30);
        S.raw(&T.oo1, "oo1", 26 * 21); S.raw(&T.oo2, "oo2", 26 * 21); S.raw(&T.oo3, "oo3", 26 * 21);
        S.raw(&T.h11, "h11", 26 * 31); S.raw(&T.h12, "h12", 26 * 31); S.raw(&T.h13, "h13", 26 * 31);
        S.raw(&T.h21, "h21", 26 * 31); S.raw(&T.h22, "h22", 26 * 31); S.raw(&T.h23, "h23", 26 * 31);
        S.raw(&T.h81, "h81", 26 * 31); S.raw(&T.h82, "h82", 26 * 31); S.raw(&T.h83, "h83", 26 * 31);
        if (!S.missing.empty()) return fail(GEOSRAD_ETABLE, "missing/ill-shaped table entries: " + S.missing);
        HIPCHK(d_tab_ch.resize(S.stage.size()));
        HIPCHK(hipMemcpy(d_tab_ch, S.stage.data(), d_tab_ch.bytes, hipMemcpyHostToDevice));
        for (auto &f : S.fix) *f.first = (const R *)(d_tab_ch + f.second);
        HIPCHK(hipMemcpy(d_C, &h_C, sizeof(ChouDev<R>), hipMemcpyHostToDevice));
        have_chou = true;
        return GEOSRAD_OK;
    }

    int irrad_dev(hipStream_t st, int m, int np, const void *const *in, double co2, int trace, int ict, int icb, int ns, int na, int nb,
                  void *const *aer, void *const *out) override
    {
        return irrad_run(st, m, np, in, co2, trace, ict, icb, ns, na, nb, aer, out, nullptr);
    }

    // geos != nullptr (lw_driver_chou_dev): in[C_FCLD] is the FCLD import and the cloud records come from the GEOS fields of *geos
    // (k_chou_prep<R, true>); in[C_CWC] / in[C_REFF] are not read
    int irrad_run(hipStream_t st, int m, int np, const void *const *in, double co2, int trace, int ict, int icb, int ns, int na, int nb,
                  void *const *aer, void *const *out, const ChouGeos<R> *geos)
    {
        HIPCHK(hipSetDevice(device));
        if (!have_chou) return fail(GEOSRAD_EINVAL, "Chou-Suarez LW tables not set: call geosrad_load_tables_chou_lw first");
        if (m <= 0 || np < 4 || np > 400) return fail(GEOSRAD_EINVAL, "bad m/np");
        if (ns < 1 || ns > 15) return fail(GEOSRAD_EINVAL, "ns must be in 1..15");
        const bool oc = (overcast & GEOSRAD_OVERCAST_IRRAD) != 0;      // -DOVERCAST reads neither ict nor icb
        if (!oc && !(ict >= 1 && ict < icb && icb <= np)) return fail(GEOSRAD_EINPUT, "ict / icb must satisfy 1 <= ict < icb <= np");
        if (nb < 10) return fail(GEOSRAD_EINVAL, "nb (bands of the aerosol arrays) must be 10");
        for (int k = 0; k < C_NIN; k++) if (!in[k] && !(geos && (k == C_CWC || k == C_REFF))) return fail(GEOSRAD_EINVAL, "null input array");
        for (int k = 0; k < CO_NOUT; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null output array");
        if (na > 0 && (!aer[0] || !aer[1] || !aer[2])) return fail(GEOSRAD_EINVAL, "na > 0 but taua/ssaa/asya null");
        const int K1 = np + 1, K2 = np + 2;
        const int nc_max = chunk_cols(m);
        R *rec, *part;
        auto carve = [&](Carve c) {
            rec = c.take<R>((size_t)nc_max * CF_NFIELD * K1);
            part = c.take<R>((size_t)nc_max * CH_NB * CH_NKIND * K2);
            return c.off;
        };
        if (d_ws_ch.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the irrad workspace failed");
        carve(Carve(d_ws_ch));
        const int nband = trace ? 10 : 9;      // irrad.F90:478 (band 10 only with trace gases)
#ifndef GEOSRAD_EXP_LDS_PAD
#define GEOSRAD_EXP_LDS_PAD 0
#endif
        const size_t lds = chou_bands_lds_bytes<R>(np) + GEOSRAD_EXP_LDS_PAD;
        const void *kb = oc ? (const void *)k_chou_bands<R, true> : (const void *)k_chou_bands<R>;
        if (lds > 64 * 1024) {
            if (hipFuncSetAttribute(kb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return fail(GEOSRAD_EINVAL, "np too large for the LDS-resident band state");
        }
        return chunk_walk(m, nc_max, [&](int c0, int nc) -> int {
            ChouArgs<R> A{};
            A.m = nc; A.ld = m; A.np = np; A.trace = trace; A.ict = ict; A.icb = icb; A.ns = ns; A.na = na; A.nb = nb; A.co2 = (R)co2;
            auto P = [&](int k) { return colp(in[k], c0); };
            A.ple = P(C_PLE); A.ta = P(C_TA); A.wa = P(C_WA); A.oa = P(C_OA); A.tb = P(C_TB); A.n2o = P(C_N2O); A.ch4 = P(C_CH4);
            A.cfc11 = P(C_CFC11); A.cfc12 = P(C_CFC12); A.cfc22 = P(C_CFC22); A.fcld = P(C_FCLD);
            ChouGeos<R> G{};
            if (geos) { G = *geos; for (int l = 0; l < 4; l++) { G.q[l] += c0; G.r[l] += c0; } }
            else { A.cwc = P(C_CWC); A.reff = P(C_REFF); }
            A.fs = P(C_FS); A.tg = P(C_TG); A.eg = P(C_EG); A.tv = P(C_TV); A.ev = P(C_EV); A.rv = P(C_RV);
            A.taua = colp(aer[0], c0); A.ssaa = colp(aer[1], c0); A.asya = colp(aer[2], c0);
            A.taudiag = (R *)out[CO_TAUDIAG] + c0;
            A.rec = rec; A.part = part;
            A.err = d_err + 2;
            span_begin(10, st);
            const dim3 gp((unsigned)((nc + 63) / 64), (unsigned)chou_prep_tiles<R>(np));
            if (geos) hipLaunchKernelGGL((k_chou_prep<R, true>), gp, dim3(256), 0, st, A, G);
            else hipLaunchKernelGGL((k_chou_prep<R, false>), gp, dim3(256), 0, st, A, G);
            span_end(st);
            span_begin(11, st);
            if (oc) hipLaunchKernelGGL((k_chou_bands<R, true>), dim3((unsigned)((nc + CH_CPW - 1) / CH_CPW), nband), dim3(64), lds, st, A, (const ChouDev<R> *)d_C);
            else hipLaunchKernelGGL(k_chou_bands<R>, dim3((unsigned)((nc + CH_CPW - 1) / CH_CPW), nband), dim3(64), lds, st, A, (const ChouDev<R> *)d_C);
            span_end(st);
            ChouOut<R> O{};
            auto Q = [&](int k) { return colp(out[k], c0); };
            O.flxu = Q(CO_FLXU); O.flcu = Q(CO_FLCU); O.flau = Q(CO_FLAU); O.flxau = Q(CO_FLXAU); O.flxd = Q(CO_FLXD); O.flcd = Q(CO_FLCD);
            O.flad = Q(CO_FLAD); O.flxad = Q(CO_FLXAD); O.dfdts = Q(CO_DFDTS); O.sfcem = Q(CO_SFCEM);
            hipLaunchKernelGGL(k_chou_reduce<R>, dim3((unsigned)((nc + 63) / 64), 9), dim3(256), 0, st, A, O, nband);
            if (!trace)      // band 10 of taudiag stays zero (the reference zeroes the array and never reaches band 10)
                for (int k = 0; k < np; k++)
                    HIPCHK(hipMemsetAsync((R *)out[CO_TAUDIAG] + ((size_t)9 * np + k) * m + c0, 0, (size_t)nc * sizeof(R), st));
            return GEOSRAD_OK;
        });
    }

    int irrad_host(int m, int np, const void *const *in, double co2, int trace, int ict, int icb, int ns, int na, int nb, void *const *aer,
                   void *const *out) override
    {
        // host arrays through the chunk pipeline like rrtmg_lw / rrtmg_sw - transfers of a chunk overlap the kernels of its neighbours
        // (irrad is 0.33 ms of kernels per 1 000 columns against 0.08 ms of transfers)
        HIPCHK(hipSetDevice(device));
        if (m <= 0 || np <= 0 || ns < 1 || nb < 1) return fail(GEOSRAD_EINVAL, "bad m/np/ns/nb");
        for (int k = 0; k < C_NIN; k++) if (!in[k]) return fail(GEOSRAD_EINVAL, "null input array");
        for (int k = 0; k < CO_NOUT; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null output array");
        HostArrs H(sizeof(R));
        const void *din[C_NIN] = {};
        void *dout[CO_NOUT] = {}, *daer[3] = {};
        for (int k = 0; k < C_NIN; k++) H.add(in[k], nullptr, ch_in_shape(k, np, ns), &din[k]);
        for (int k = 0; k < 3; k++) if (na > 0 && aer[k]) H.add(aer[k], aer[k], ch_aer_shape(np, nb), &daer[k]);      // rescaled in place
        for (int k = 0; k < CO_NOUT; k++) H.add(nullptr, out[k], ch_out_shape(k, np), &dout[k]);
        const int rc = host_call(m, H, -1, [&](hipStream_t st, int nc) { return irrad_dev(st, nc, np, din, co2, trace, ict, icb, ns, na, nb, daer, dout); });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));      // the Chou schemes have no input assertions (neither has the reference)
        return GEOSRAD_OK;
    }

    // =====================================================================================================
    // Chou-Suarez shortwave (sorad)
    // =====================================================================================================
    int set_tables_chou_sw(const void *blob, size_t nbytes) override
    {
        HIPCHK(hipSetDevice(device));
        Blob B;
        if (!B.parse(blob, nbytes)) return fail(GEOSRAD_ETABLE, B.err);
        if (B.realbytes != (int)sizeof(R)) return fail(GEOSRAD_ETABLE, "table blob real size does not match the context's real_kind");
        TableStage<R> S(B);
        SoradDev<R> &T = h_O;
        memset(&T, 0, sizeof(T));
        auto cp = [&](R *dst, const char *nm, size_t n) { const R *s = S.get(nm, n); if (s) memcpy(dst, s, n * sizeof(R)); };
        cp(T.zk_uv, "zk_uv", 5); cp(T.wk_uv, "wk_uv", 5); cp(T.ry_uv, "ry_uv", 5); cp(T.xk_ir, "xk_ir", 10); cp(T.ry_ir, "ry_ir", 3);
        cp(T.aig_uv, "aig_uv", 3); cp(T.awg_uv, "awg_uv", 3); cp(T.arg_uv, "arg_uv", 3); cp(T.awb_uv, "awb_uv", 2); cp(T.arb_uv, "arb_uv", 2);
        cp(T.awb_nir, "awb_nir", 6); cp(T.arb_nir, "arb_nir", 6); cp(T.aia_nir, "aia_nir", 9); cp(T.awa_nir, "awa_nir", 9);
        cp(T.ara_nir, "ara_nir", 9); cp(T.aig_nir, "aig_nir", 9); cp(T.awg_nir, "awg_nir", 9); cp(T.arg_nir, "arg_nir", 9);
        T.aib_uv = S.scalar("aib_uv"); T.aib_nir = S.scalar("aib_nir");
        S.raw(&T.coa, "coa", 62 * 101); S.raw(&T.cah, "cah", 43 * 37); S.raw(&T.caib, "caib", 11 * 9 * 11); S.raw(&T.caif, "caif", 9 * 11);
        if (!S.missing.empty()) return fail(GEOSRAD_ETABLE, "missing/ill-shaped table entries: " + S.missing);
        HIPCHK(d_tab_so.resize(S.stage.size()));
        HIPCHK(hipMemcpy(d_tab_so, S.stage.data(), d_tab_so.bytes, hipMemcpyHostToDevice));
        for (auto &f : S.fix) *f.first = (const R *)(d_tab_so + f.second);
        HIPCHK(hipMemcpy(d_O, &h_O, sizeof(SoradDev<R>), hipMemcpyHostToDevice));
        have_sorad = true;
        return GEOSRAD_OK;
    }

    int sorad_check_options(int m, int np, int nb, int ict, int icb, const void *hk_uv, const void *hk_ir)
    {
        if (!have_sorad) return fail(GEOSRAD_EINVAL, "Chou-Suarez SW tables not set: call geosrad_load_tables_chou_sw first");
        if (m <= 0 || np < 4 || np > 400) return fail(GEOSRAD_EINVAL, "bad m/np");
        if (nb < 8) return fail(GEOSRAD_EINVAL, "nb (bands of the aerosol arrays) must be 8");
        const bool oc = (overcast & GEOSRAD_OVERCAST_SORAD) != 0;      // -DOVERCAST reads neither ict nor icb
        if (!oc && !(ict >= 1 && ict < icb && icb <= np)) return fail(GEOSRAD_EINPUT, "ict / icb must satisfy 1 <= ict < icb < np + 1");
        if (!hk_uv || !hk_ir) return fail(GEOSRAD_EINVAL, "hk_uv / hk_ir null");
        return GEOSRAD_OK;
    }
    // One body for geosrad_sorad_dev (na_out null, or all its members: no second pass) and geosrad_sorad_na_dev.  Per chunk: the
    // preparation once; `sweep` - the spectral passes over the selectable paths, their sum and the reduction - with the aerosols into `out`
    // and then, aerosol-free (NA flavour of the same kernels), into na_out.  The second sweep reuses scr, psum and the dynamic LDS: one stream
    // runs the two in order, and the first reduction has read psum before the second pass rewrites it.  k_sorad_sum / k_sorad_reduce need
    // all of flx, flc, flxu, flcu: a member of na_out the caller does not take has its place in the workspace.
    int sorad_dev(hipStream_t st, int m, int np, int nb, const void *const *in, double co2, int ict, int icb, const void *hk_uv,
                  const void *hk_ir, void *const *out, int do_drfband, void *const *na_out) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = sorad_check_options(m, np, nb, ict, icb, hk_uv, hk_ir)) return rc;
        const bool oc = (overcast & GEOSRAD_OVERCAST_SORAD) != 0;      // -DOVERCAST reads neither ict nor icb
        for (int k = 0; k < SI_NIN; k++) if (!in[k]) return fail(GEOSRAD_EINVAL, "null input array");
        for (int k = 0; k < SOO_DRBAND; k++) if (!out[k]) return fail(GEOSRAD_EINVAL, "null output array");
        if (do_drfband && (!out[SOO_DRBAND] || !out[SOO_DFBAND])) return fail(GEOSRAD_EINVAL, "do_drfband set but drband/dfband null");
        const int K2 = np + 2;
        const int nc_max = chunk_cols(m);
        const size_t per = (size_t)nc_max;
        // passes: k_sorad_pass (lane = column, the per-level arrays of every pass in HBM scratch planes, 30 x K2 reals per (column, pass))
        // or k_sorad_col (one block per column, everything on chip, no scratch; GEOSRAD_SORAD_PATH=col)
        // (a layer count whose on-chip arrays exceed the LDS takes the scratch-plane path; so does OVERCAST: k_sorad_col has no OVERCAST
        // variant, the OVERCAST passes are k_sorad_pass_oc whatever GEOSRAD_SORAD_PATH says)
        const bool col_path = !oc && sorad_col_path && K2 <= 256 && sorad_col_lds_reals<R>(np) * sizeof(R) <= (size_t)160 * 1024;
        const bool na = sona_any(na_out);
        void *na_arr[GEOSRAD_SONA_NOUT] = {};      // na_out, or the workspace's place for a member not taken (whole call wide, like the caller's)
        SoradArgs<R> W{};      // the workspace planes, the same for every chunk; the gathered aerosol planes and the scratch planes only on the paths that use them
        auto carve = [&](Carve c) {
            W.lay = c.take<R>(4 * K2 * per); W.swh = c.take<R>(K2 * per); W.colv = c.take<R>(8 * per); W.cld = c.take<R>((size_t)SO_NGRP * 4 * K2 * per);
            W.psum = c.take<R>((size_t)SO_NPASS * 3 * per);
            W.aer = col_path || oc ? nullptr : c.take<R>((size_t)3 * SO_NGATHER * np * per);
            W.perm = c.take<int32_t>(per); W.cls = c.take<uint8_t>(per); W.cls_off = c.take<int32_t>(16);
            W.scr = col_path ? nullptr : c.take<R>((size_t)SO_NPASS * SO_NPLANE * K2 * per);
            for (int k = 0; na && k < GEOSRAD_SONA_NOUT; k++)
                na_arr[k] = na_out[k] ? na_out[k] : (void *)c.take<R>(so_out_shape(SONA_TWIN[k], np).rows * (size_t)m);
            return c.off;
        };
        const size_t need = carve(Carve());
        const size_t so_lds = sorad_col_lds_reals<R>(np) * sizeof(R);
        if (col_path) {
            if (so_lds > so_lds_set) {
                HIPCHK(hipFuncSetAttribute((const void *)k_sorad_col<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)so_lds));
                HIPCHK(hipFuncSetAttribute((const void *)k_sorad_col<R, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)so_lds));
                so_lds_set = so_lds;
            }
        }
        if (d_ws_so.reserve(need) != hipSuccess)
            return fail(GEOSRAD_ENOMEM, "hipMalloc of the sorad workspace failed (" + std::to_string(need >> 20) + " MiB); lower it with geosrad_set_chunk()");
        carve(Carve(d_ws_so));
        return chunk_walk(m, nc_max, [&](int c0, int nc) -> int {
            SoradArgs<R> A = W;
            A.m = nc; A.ld = m; A.np = np; A.ict = ict; A.icb = icb; A.do_drfband = do_drfband; A.co2 = (R)co2;
            for (int p = 0; p < 5; p++) A.hk[p] = ((const R *)hk_uv)[p];
            for (int ib = 0; ib < 3; ib++) for (int ik = 0; ik < 10; ik++) A.hk[5 + ib * 10 + ik] = ((const R *)hk_ir)[ik * 3 + ib];   // hk_ir(3,10)
            auto P = [&](int k) { return colp(in[k], c0); };
            A.cosz = P(SI_COSZ); A.pl = P(SI_PL); A.ta = P(SI_TA); A.wa = P(SI_WA); A.oa = P(SI_OA); A.cwc = P(SI_CWC); A.fcld = P(SI_FCLD);
            A.reff = P(SI_REFF); A.taua = P(SI_TAUA); A.ssaa = P(SI_SSAA); A.asya = P(SI_ASYA); A.rsuvbm = P(SI_RSUVBM);
            A.rsuvdf = P(SI_RSUVDF); A.rsirbm = P(SI_RSIRBM); A.rsirdf = P(SI_RSIRDF);
            const dim3 blk(256);
            const unsigned gx = grid256(nc);
            span_begin(12, st);
            if (oc) {          // OVERCAST: one class, positions are columns
                hipLaunchKernelGGL(k_sorad_ident<R>, dim3(gx), blk, 0, st, A);
                hipLaunchKernelGGL(k_sorad_prep<R>, dim3(gx), blk, 0, st, A);
                hipLaunchKernelGGL((k_sorad_cloud<R, true>), dim3(gx, (unsigned)np), blk, 0, st, A, (const SoradDev<R> *)d_O);
            } else {
                // the columns sorted by which cloud groups hold cloud (8 classes): workspace by position from here on (the on-chip path keeps the
                // caller's order: one class)
                hipLaunchKernelGGL(k_sorad_class<R>, dim3(gx), blk, 0, st, A, col_path ? 1 : 0);
                hipLaunchKernelGGL(k_partition8, dim3(1), dim3(1024), 0, st, nc, (const uint8_t *)A.cls, A.perm, A.cls_off);
                if (!col_path) hipLaunchKernelGGL(k_sorad_gather<R>, dim3(gx, (unsigned)(3 * SO_NGATHER * np)), blk, 0, st, A);
                hipLaunchKernelGGL(k_sorad_prep<R>, dim3(gx), blk, 0, st, A);
                hipLaunchKernelGGL(k_sorad_cloud<R>, dim3(gx, (unsigned)np), blk, 0, st, A, (const SoradDev<R> *)d_O);
            }
            span_end(st);
            SoradOut<R> O{};
            auto Q = [&](int k) { return colp(out[k], c0); };
            O.flx = Q(SOO_FLX); O.flc = Q(SOO_FLC); O.fdiruv = Q(SOO_FDIRUV); O.fdifuv = Q(SOO_FDIFUV); O.fdirpar = Q(SOO_FDIRPAR);
            O.fdifpar = Q(SOO_FDIFPAR); O.fdirir = Q(SOO_FDIRIR); O.fdifir = Q(SOO_FDIFIR); O.flxu = Q(SOO_FLXU); O.flcu = Q(SOO_FLCU);
            O.flx_sfc_band = Q(SOO_SFCBAND); O.drband = Q(SOO_DRBAND); O.dfband = Q(SOO_DFBAND);
            // the spectral passes (slot 13), their sum over the passes and the reduction, into O; NA: the aerosol-free flavour
            auto sweep = [&](auto na_c, const SoradOut<R> &O) {
                constexpr bool NA = decltype(na_c)::value;
                const SoradDev<R> *dO = (const SoradDev<R> *)d_O;
                span_begin(13, st);
                if (oc) {
                    hipLaunchKernelGGL((k_sorad_pass_oc<R, NA>), dim3(band_grid(nc, SO_NPASS)), blk, 0, st, A, dO);
                } else if (col_path) {   // one block per column, lanes = (pass slot, level) (whole wavefronts), all 35 passes on chip
                    const unsigned nthr = (unsigned)sorad_col_threads(np);
                    const unsigned grid = 8u * (unsigned)((nc + 7) / 8);
                    hipLaunchKernelGGL((k_sorad_col<R, NA>), dim3(grid), dim3(nthr), so_lds, st, A, dO, O);
                } else {
                    // one instantiation per class, the classes with the most sky situations first; a block without a position of the class
                    // returns at once
                    // one-dimensional XCD-aware grid (band_block): the 35 passes of a position block run together on one XCD and share its layer
                    // inputs from that L2 (8.7 -> 8.1 ms per 100 000 columns against a (block, pass) grid)
                    const dim3 g(band_grid(nc, SO_NPASS));
                    hipLaunchKernelGGL((k_sorad_pass<R, 7, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 6, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 5, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 3, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 4, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 2, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 1, NA>), g, blk, 0, st, A, dO);
                    hipLaunchKernelGGL((k_sorad_pass<R, 0, NA>), g, blk, 0, st, A, dO);
                }
                span_end(st);               // the slot times k_sorad_pass alone (= its average duration in a rocprofv3 kernel trace)
                if (!col_path) hipLaunchKernelGGL(k_sorad_sum<R>, dim3(gx, np + 1), blk, 0, st, A, O);
                hipLaunchKernelGGL((k_sorad_reduce<R, NA>), dim3(gx), blk, 0, st, A, dO, O);
            };
            sweep(std::false_type{}, O);
            if (na) {
                SoradOut<R> N{};      // the members the aerosol-free reduction never writes stay null
                auto QN = [&](int k) { return colp(na_arr[k], c0); };
                N.flx = QN(GEOSRAD_SONA_FLX); N.flc = QN(GEOSRAD_SONA_FLC); N.flxu = QN(GEOSRAD_SONA_FLXU); N.flcu = QN(GEOSRAD_SONA_FLCU);
                N.flx_sfc_band = QN(GEOSRAD_SONA_SFCBAND);
                sweep(std::true_type{}, N);
            }
            return GEOSRAD_OK;
        });
    }

    int sorad_host(int m, int np, int nb, const void *const *in, double co2, int ict, int icb, const void *hk_uv, const void *hk_ir,
                   void *const *out, int do_drfband, void *const *na_out) override
    {
        // host arrays through the chunk pipeline
        HIPCHK(hipSetDevice(device));
        if (m <= 0 || np <= 0 || nb < 1) return fail(GEOSRAD_EINVAL, "bad m/np/nb");
        for (int k = 0; k < SI_NIN; k++) if (!in[k]) return fail(GEOSRAD_EINVAL, "null input array");
        HostArrs H(sizeof(R));
        const void *din[SI_NIN] = {};
        void *dout[SOO_NOUT] = {};
        for (int k = 0; k < SI_NIN; k++) H.add(in[k], nullptr, so_in_shape(k, np, nb), &din[k]);
        // an output the caller does not take (or drband / dfband without do_drfband) still has its place on the device
        for (int k = 0; k < SOO_NOUT; k++)
            H.add(nullptr, ((k == SOO_DRBAND || k == SOO_DFBAND) && !do_drfband) ? nullptr : out[k], so_out_shape(k, np), &dout[k]);
        // the aerosol-free arrays the caller takes: further per-column records (the others keep their place in sorad_dev's workspace)
        void *dna[GEOSRAD_SONA_NOUT] = {};
        for (int k = 0; na_out && k < GEOSRAD_SONA_NOUT; k++) if (na_out[k]) H.add(nullptr, na_out[k], so_out_shape(SONA_TWIN[k], np), &dna[k]);
        const int rc = host_call(m, H, -1, [&](hipStream_t st, int nc) { return sorad_dev(st, nc, np, nb, din, co2, ict, icb, hk_uv, hk_ir, dout, do_drfband, dna); });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));      // the Chou schemes have no input assertions (neither has the reference)
        return GEOSRAD_OK;
    }

    // =====================================================================================================
    // gettau (include/geosrad_gettau.h; gettau_kernels.hpp)
    // =====================================================================================================
    DevBuf<> d_ws_gt;      // (ncol,3) super-layer cloud maxima of the overlap mode
    int gettau_dev(hipStream_t st, const GtCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = gettau_check(C)) return rc;
        if (C.kind == 2 ? !have_chou : !have_sorad)
            return fail(GEOSRAD_EINVAL, C.kind == 2 ? "Chou-Suarez LW tables not set: call geosrad_load_tables_chou_lw first"
                                                    : "Chou-Suarez SW tables not set: call geosrad_load_tables_chou_sw first");
        GtArgs<R> A{};
        A.ncol = C.ncol; A.nlevs = C.nlevs; A.ib = C.ib; A.ict = C.kind == 2 ? 0 : C.ict; A.icb = C.icb; A.grav = (R)C.grav;
        A.cosz = (const R *)C.cosz; A.dp = (const R *)C.dp; A.fcld = (const R *)C.fcld; A.reff = (const R *)C.reff; A.hyd = (const R *)C.hyd;
        const dim3 grid(grid256(C.ncol), (unsigned)((C.nlevs + GT_LC - 1) / GT_LC));
        if (C.kind == 2) {
            A.taudiag = (R *)C.out[0]; A.tcldlyr = (R *)C.out[1]; A.enn = (R *)C.out[2];
            hipLaunchKernelGGL((k_getirtau<R>), grid, dim3(256), 0, st, A, (const ChouDev<R> *)d_C);
        } else {
            A.taubeam = (R *)C.out[0]; A.taudiff = (R *)C.out[1]; A.asycl = (R *)C.out[2]; A.ssacl = C.kind == 1 ? (R *)C.out[3] : nullptr;
            if (A.ict != 0 && (A.taubeam || A.taudiff)) {
                if (d_ws_gt.reserve((size_t)3 * C.ncol * sizeof(R)) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the gettau workspace failed");
                A.cc = (const R *)d_ws_gt.p;
                hipLaunchKernelGGL((k_gettau_cc<R>), dim3(grid256(C.ncol)), dim3(256), 0, st, C.ncol, C.nlevs, A.ict, A.icb, A.fcld, (R *)d_ws_gt.p);
            }
            if (C.kind == 0) hipLaunchKernelGGL((k_getvistau<R>), grid, dim3(256), 0, st, A, (const SoradDev<R> *)d_O);
            else hipLaunchKernelGGL((k_getnirtau<R>), grid, dim3(256), 0, st, A, (const SoradDev<R> *)d_O);
        }
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int gettau_host(const GtCall &C) override
    {
        // host arrays through the chunk pipeline; an output the caller does not take has no place on the device either
        HIPCHK(hipSetDevice(device));
        if (const int rc = gettau_check(C)) return rc;
        HostArrs H(sizeof(R));
        GtCall D = C;
        const void *in[5] = {C.cosz, C.dp, C.fcld, C.reff, C.hyd};
        const void **din[5] = {&D.cosz, &D.dp, &D.fcld, &D.reff, &D.hyd};
        for (int k = 0; k < 5; k++) { *din[k] = nullptr; if (in[k] && !(k == 0 && C.kind == 2)) H.add(in[k], nullptr, gt_in_shape(k, C.nlevs), din[k]); }
        for (int k = 0; k < 4; k++) { D.out[k] = nullptr; if (C.out[k]) H.add(nullptr, C.out[k], gt_out_shape(C.kind, k, C.nlevs), &D.out[k]); }
        const int rc = host_call(C.ncol, H, -1, [&](hipStream_t st, int nc) { D.ncol = nc; return gettau_dev(st, D); });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        return GEOSRAD_OK;
    }

    // =====================================================================================================
    // the satellite simulator's ISCCP path (include/geosrad_satsim.h; satsim_kernels.hpp)
    // =====================================================================================================
    DevBuf<> d_ws_ss;
    struct SsWs { int32_t *seed0, *itrop; uint8_t *mask, *bin; R *dem_wv, *bb, *pt, *tbb, *ptop, *alb, *mm; };
    // the workspace of one call: on Carve() the bytes it takes, on Carve(d_ws_ss) its planes.  mask: the byte mask is the context's too
    size_t ss_layout(int np, int nlev, int ncol, bool mask, SsWs &w, Carve c) const
    {
        const size_t pl = (size_t)np * nlev, ps = (size_t)np * ncol;
        w.seed0 = c.take<int32_t>(np); w.itrop = c.take<int32_t>(np); w.mm = c.take<R>(2);
        w.dem_wv = c.take<R>(pl); w.bb = c.take<R>(pl); w.pt = c.take<R>((size_t)SS_NPT * np);
        w.tbb = c.take<R>(ps); w.ptop = c.take<R>(ps); w.alb = c.take<R>(ps); w.bin = c.take<uint8_t>(ps);
        w.mask = c.take<uint8_t>(mask ? ps * nlev : 0);
        return c.off;
    }
    // the planes of a call; a larger request than any before re-allocates (as every workspace here: not inside a graph capture)
    int ss_workspace(int np, int nlev, int ncol, bool mask, SsWs &w)
    {
        // the mask, once taken, stays part of the layout, so that calls with and without it do not move the other planes about
        ss_mask |= mask;
        if (d_ws_ss.reserve(ss_layout(np, nlev, ncol, ss_mask, w, Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the satellite simulator's workspace failed");
        ss_layout(np, nlev, ncol, ss_mask, w, Carve(d_ws_ss.p));
        return GEOSRAD_OK;
    }
    bool ss_mask = false;

    int scops_launch(hipStream_t st, const ScopsCall &C, int32_t *seed0)
    {
        ScopsArgs<R> A{};
        A.npoints = C.npoints; A.nlev = C.nlev; A.ncol = C.ncol; A.overlap = C.overlap;
        // ncol draws on: x -> a x + c composed ncol times; the inverse multiplier by Newton's iteration (exact mod 2^32, so mod 2^30)
        uint32_t jA = 1, jC = 0;
        for (int k = 0; k < C.ncol; k++) { jC = jC * SS_A + SS_C; jA = jA * SS_A; }
        uint32_t inv = SS_A;
        for (int k = 0; k < 5; k++) inv *= 2u - SS_A * inv;
        A.jA = jA; A.jC = jC; A.ainv = inv;
        A.seed_in = seed0; A.seed = C.seed; A.cc = (const R *)C.cc; A.conv = (const R *)C.conv; A.frac_out = (uint8_t *)C.frac_out;
        HIPCHK(hipMemcpyAsync(seed0, C.seed, (size_t)C.npoints * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL((k_scops<R>), dim3(grid256((size_t)C.npoints * C.ncol)), dim3(256), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int scops_dev(hipStream_t st, const ScopsCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = scops_check(C)) return rc;
        SsWs w;
        if (const int rc = ss_workspace(C.npoints, C.nlev, C.ncol, false, w)) return rc;
        return scops_launch(st, C, w.seed0);
    }
    int icarus_dev(hipStream_t st, const IcarusCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = icarus_check(C)) return rc;
        SsWs w;
        if (const int rc = ss_workspace(C.npoints, C.nlev, C.ncol, C.cosp, w)) return rc;
        const int np = C.npoints;
        if (C.cosp) {
            const ScopsCall S{np, C.nlev, C.ncol, C.overlap, C.seed, C.in[IC_CC], C.in[IC_CONV], w.mask};
            // SCOPS takes FCLD / CCA as they are (cosp.F90:392-397); the 0.999999 of cosp_isccp_simulator.F90:65-66 is on icarus' arguments only
            if (const int rc = scops_launch(st, S, w.seed0)) return rc;
            if (C.sgfcld) hipLaunchKernelGGL((k_sgfcld<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, np, C.ncol, (const uint8_t *)w.mask, (R *)C.sgfcld);
            if (C.scops_only) { HIPCHK(hipGetLastError()); return GEOSRAD_OK; }
        }
        IcArgs<R> A{};
        A.npoints = np; A.nlev = C.nlev; A.ncol = C.ncol; A.top_height = C.top_height; A.top_height_direction = C.top_height_direction;
        A.ple_shift = C.cosp; A.scaled = C.cosp; A.cosp_out = C.cosp; A.emsfc_lw = (R)C.emsfc_lw;
        A.sunlit = C.sunlit;
        auto I = [&](int k) { return (const R *)C.in[k]; };
        A.pfull = I(IC_PFULL); A.phalf = I(IC_PHALF); A.qv = I(IC_QV); A.cc = I(IC_CC); A.conv = I(IC_CONV); A.dtau_s = I(IC_DTAU_S);
        A.dtau_c = I(IC_DTAU_C); A.skt = I(IC_SKT); A.at = I(IC_AT); A.dem_s = I(IC_DEM_S); A.dem_c = I(IC_DEM_C);
        A.frac = C.cosp ? w.mask : (const uint8_t *)C.frac_out;
        A.dem_wv = w.dem_wv; A.bb = w.bb; A.pt = w.pt; A.itrop = w.itrop; A.tbb = w.tbb; A.ptop = w.ptop; A.alb = w.alb; A.bin = w.bin;
        A.err = d_err + 3;
        auto O = [&](int k) { return (R *)C.out[k]; };
        A.fq = O(ICO_FQ); A.totalcldarea = O(ICO_TCA); A.meanptop = O(ICO_PTOP); A.meantaucld = O(ICO_TAU); A.meanalbedocld = O(ICO_ALB);
        A.meantb = O(ICO_TB); A.meantbclr = O(ICO_TBCLR); A.boxtau = O(ICO_BOXTAU); A.boxptop = O(ICO_BOXPTOP);
        hipLaunchKernelGGL((k_icarus_point<R>), dim3(grid256(np)), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_icarus_box<R>), dim3(grid256((size_t)np * C.ncol)), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_icarus_stats<R>), dim3((unsigned)((np + SS_STATS_T - 1) / SS_STATS_T)), dim3(SS_STATS_T), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int cosp_seeds_dev(hipStream_t st, int npoints, const void *psfc, int32_t *seed) override
    {
        HIPCHK(hipSetDevice(device));
        if (npoints < 1 || !psfc || !seed) return fail(GEOSRAD_EINVAL, "geosrad_cosp_seeds_dev: npoints must be positive, psfc and seed given");
        SsWs w;
        if (const int rc = ss_workspace(npoints, 2, 1, false, w)) return rc;
        if (npoints > 1) hipLaunchKernelGGL((k_cosp_minmax<R>), dim3(1), dim3(1024), 0, st, npoints, (const R *)psfc, w.mm);
        hipLaunchKernelGGL((k_cosp_seeds<R>), dim3(grid256(npoints)), dim3(256), 0, st, npoints, (const R *)psfc, (const R *)w.mm, seed);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    // host arrays through the chunk pipeline: chunks split the points, a point's stream stays in one chunk.  The real mask of the caller
    // and the byte mask of the kernels are two arrays of the slot, converted on the device
    int scops_host(const ScopsCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = scops_check(C)) return rc;
        HostArrs H(sizeof(R));
        ScopsCall D = C;
        // the seeds go in as one array and come back as another, so that the byte mask between them is transferred in neither direction
        const void *seed_in = nullptr, *seed_at = nullptr, *frac_at = nullptr, *u8_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev;
        H.add(C.cc, nullptr, {(size_t)C.nlev, 1}, &D.cc);
        H.add(C.conv, nullptr, {(size_t)C.nlev, 1}, &D.conv);
        H.add(C.seed, nullptr, {1, 1}, &seed_in, sizeof(int32_t));
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        H.add(nullptr, C.seed, {1, 1}, &seed_at, sizeof(int32_t));
        H.add(nullptr, C.frac_out, {cells, 1}, &frac_at);
        const int rc = host_call(C.npoints, H, -1, [&](hipStream_t st, int nc) {
            D.npoints = nc; D.seed = (int32_t *)seed_at; D.frac_out = (void *)u8_at;
            if (const int r = hip_rc("hipMemcpyAsync", hipMemcpyAsync((void *)seed_at, seed_in, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToDevice, st))) return r;
            if (const int r = scops_dev(st, D)) return r;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_mask_to_real<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const uint8_t *)u8_at, (R *)frac_at);
            return hip_rc("k_mask_to_real", hipGetLastError());
        });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        return GEOSRAD_OK;
    }
    int icarus_host(const IcarusCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (C.cosp) return fail(GEOSRAD_EINVAL, "geosrad_isccp_dev has no host variant");
        if (const int rc = icarus_check(C)) return rc;
        HostArrs H(sizeof(R));
        IcarusCall D = C;
        const void *sun_at = nullptr, *frac_at = nullptr, *u8_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev;
        for (int k = 0; k < IC_NIN; k++) H.add(C.in[k], nullptr, ic_in_shape(k, C.nlev), &D.in[k]);
        H.add(C.sunlit, nullptr, {1, 1}, &sun_at, sizeof(int32_t));
        H.add(C.frac_out, nullptr, {cells, 1}, &frac_at);
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        for (int k = 0; k < ICO_NOUT; k++) { D.out[k] = nullptr; if (C.out[k]) H.add(nullptr, C.out[k], ic_out_shape(k, C.ncol), &D.out[k]); }
        return host_call(C.npoints, H, 3, [&](hipStream_t st, int nc) {
            D.npoints = nc; D.sunlit = (const int32_t *)sun_at; D.frac_out = u8_at;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_real_to_mask<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const R *)frac_at, (uint8_t *)u8_at);
            return icarus_dev(st, D);
        });
    }

    // =====================================================================================================
    // the MISR simulator (include/geosrad_misr_modis.h; misr_modis_kernels.hpp)
    // =====================================================================================================
    DevBuf<> d_ws_misr;      // two (npoints,ncol) planes: a sub-column's optical depth and its MISR cloud-top height
    int misr_dev(hipStream_t st, const MisrCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = misr_check(C)) return rc;
        return misr_launch(st, C);
    }
    // the two kernels on a record that misr_check has passed (a chunk of misr_host's: checked once for the call)
    int misr_launch(hipStream_t st, const MisrCall &C)
    {
        const size_t ps = (size_t)C.npoints * C.ncol;
        if (d_ws_misr.reserve(2 * ps * sizeof(R)) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the MISR simulator's workspace failed");
        MisrArgs<R> A{};
        A.npoints = C.npoints; A.nlev = C.nlev; A.ncol = C.ncol; A.first = C.first; A.last = C.last; A.missing_value = (R)C.missing_value;
        A.sunlit = C.sunlit;
        A.zfull = (const R *)C.in[MI_ZFULL]; A.at = (const R *)C.in[MI_AT]; A.dtau_s = (const R *)C.in[MI_DTAU_S]; A.dtau_c = (const R *)C.in[MI_DTAU_C];
        A.frac = (const uint8_t *)C.frac_out;
        A.tau = (R *)d_ws_misr.p; A.ztop = A.tau + ps;
        A.fq = (R *)C.out[MIO_FQ]; A.dist = (R *)C.out[MIO_DIST]; A.mean_ztop = (R *)C.out[MIO_ZTOP]; A.cldarea = (R *)C.out[MIO_AREA];
        hipLaunchKernelGGL((k_misr_box<R>), dim3(grid256(ps)), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_misr_stats<R>), dim3((unsigned)((C.npoints + MISR_STATS_T - 1) / MISR_STATS_T)), dim3(MISR_STATS_T), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    // host arrays through the chunk pipeline: chunks split the points; only the chunk that holds the call's first / last point gets the
    // record's `first` / `last`
    int misr_host(const MisrCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = misr_check(C)) return rc;
        HostArrs H(sizeof(R));
        MisrCall D = C;
        const void *sun_at = nullptr, *frac_at = nullptr, *u8_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev;
        for (int k = 0; k < MI_NIN; k++) H.add(C.in[k], nullptr, {(size_t)C.nlev, 1}, &D.in[k]);
        H.add(C.sunlit, nullptr, {1, 1}, &sun_at, sizeof(int32_t));
        H.add(C.frac_out, nullptr, {cells, 1}, &frac_at);
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        for (int k = 0; k < MIO_NOUT; k++) { D.out[k] = nullptr; if (C.out[k]) H.add(nullptr, C.out[k], misr_out_shape(k), &D.out[k]); }
        const int rc = host_call_at(C.npoints, H, -1, [&](hipStream_t st, int nc, int c0) {
            D.npoints = nc; D.sunlit = (const int32_t *)sun_at; D.frac_out = u8_at;
            D.first = C.first && c0 == 0; D.last = C.last && c0 + nc == C.npoints;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_real_to_mask<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const R *)frac_at, (uint8_t *)u8_at);
            return misr_launch(st, D);
        });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        return GEOSRAD_OK;
    }

    // =====================================================================================================
    // the MODIS simulator and the whole COSP path (include/geosrad_misr_modis.h; misr_modis_kernels.hpp)
    // =====================================================================================================
    DevBuf<> d_ws_modis;      // two (npoints,nlev) planes, four (npoints,ncol) planes; for geosrad_cosp_dev zfull and boxptop too
    const ModisTab<R> md_tab = md_tables<R>();
    struct MdWs { R *frac_ls, *frac_cv, *ctp, *tau, *size, *zfull, *boxptop; int32_t *phase; };
    size_t md_layout(int np, int nlev, int ncol, bool cosp, MdWs &w, Carve c) const
    {
        const size_t pl = (size_t)np * nlev, ps = (size_t)np * ncol;
        w.frac_ls = c.take<R>(pl); w.frac_cv = c.take<R>(pl); w.ctp = c.take<R>(ps); w.tau = c.take<R>(ps); w.size = c.take<R>(ps);
        w.phase = c.take<int32_t>(ps);
        w.zfull = c.take<R>(cosp ? pl : 0); w.boxptop = c.take<R>(cosp ? ps : 0);
        return c.off;
    }
    bool md_cosp = false;      // once taken, the two planes of geosrad_cosp_dev stay part of the layout
    int md_workspace(int np, int nlev, int ncol, bool cosp, MdWs &w)
    {
        md_cosp |= cosp;
        if (d_ws_modis.reserve(md_layout(np, nlev, ncol, md_cosp, w, Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the MODIS simulator's workspace failed");
        md_layout(np, nlev, ncol, md_cosp, w, Carve(d_ws_modis.p));
        return GEOSRAD_OK;
    }
    int modis_dev(hipStream_t st, const ModisCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = modis_check(C)) return rc;
        return modis_launch(st, C);
    }
    // the three kernels on a record that modis_check has passed
    int modis_launch(hipStream_t st, const ModisCall &C)
    {
        MdWs w;
        if (const int rc = md_workspace(C.npoints, C.nlev, C.ncol, false, w)) return rc;
        const int np = C.npoints;
        ModisArgs<R> A{};
        A.npoints = np; A.nlev = C.nlev; A.ncol = C.ncol; A.ple_shift = C.geos; A.clamp_mr = C.geos;
        A.sunlit = C.sunlit;
        auto I = [&](int k) { return (const R *)C.in[k]; };
        A.t = I(MDI_T); A.p = I(MDI_P); A.ph = I(MDI_PH); A.dtau_s = I(MDI_DTAU_S); A.dtau_c = I(MDI_DTAU_C);
        for (int k = 0; k < 4; k++) { A.mr[k] = I(MDI_MR + k); A.reff[k] = I(MDI_REFF + k); }
        A.boxptop = I(MDI_BOXPTOP);
        A.frac = (const uint8_t *)C.frac_out;
        A.frac_ls = w.frac_ls; A.frac_cv = w.frac_cv; A.phase = w.phase; A.ctp = w.ctp; A.tau = w.tau; A.size = w.size;
        A.err = d_err + 4;
        A.mean = (R *)C.out[MDO_MEAN]; A.hist = (R *)C.out[MDO_HIST];
        A.o_phase = (int32_t *)C.out[MDO_PHASE]; A.o_ctp = (R *)C.out[MDO_CTP]; A.o_tau = (R *)C.out[MDO_TAU]; A.o_size = (R *)C.out[MDO_SIZE];
        A.tab = md_tab;
        hipLaunchKernelGGL((k_cosp_fracs<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_modis_box<R>), dim3(grid256((size_t)np * C.ncol)), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_modis_stats<R>), dim3((unsigned)((np + MD_STATS_T - 1) / MD_STATS_T)), dim3(MD_STATS_T), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int modis_host(const ModisCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = modis_check(C)) return rc;
        HostArrs H(sizeof(R));
        ModisCall D = C;
        const void *sun_at = nullptr, *frac_at = nullptr, *u8_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev;
        for (int k = 0; k < MDI_NIN; k++) { D.in[k] = nullptr; if (C.in[k] && k != MDI_BOXTAU) H.add(C.in[k], nullptr, modis_in_shape(k, C.nlev, C.ncol), &D.in[k]); }
        H.add(C.sunlit, nullptr, {1, 1}, &sun_at, sizeof(int32_t));
        H.add(C.frac_out, nullptr, {cells, 1}, &frac_at);
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        for (int k = 0; k < MDO_NOUT; k++) {
            D.out[k] = nullptr;
            if (C.out[k]) H.add(nullptr, C.out[k], modis_out_shape(k, C.ncol), &D.out[k], k == MDO_PHASE ? sizeof(int32_t) : 0);
        }
        return host_call(C.npoints, H, 4, [&](hipStream_t st, int nc) {
            D.npoints = nc; D.sunlit = (const int32_t *)sun_at; D.frac_out = u8_at;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_real_to_mask<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const R *)frac_at, (uint8_t *)u8_at);
            return modis_launch(st, D);
        });
    }
    // call COSP with the ISCCP, MISR and MODIS simulators on: one SCOPS mask in the workspace serves the three
    int cosp_dev(hipStream_t st, const CospCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        IcarusCall I = C.ic;
        if (const int rc = icarus_check(I)) return rc;
        if (!C.zle || !C.qltot || !C.qitot || !C.rdfl || !C.rdfi) return fail(GEOSRAD_EINVAL, "geosrad_cosp_dev: null input array");
        bool want_isccp = false, want_misr = false;
        for (int k = 0; k < ICO_NOUT; k++) want_isccp |= I.out[k] != nullptr;
        for (int k = 0; k < MIO_NOUT; k++) want_misr |= C.misr[k] != nullptr;
        const bool want_modis = C.modis[0] || C.modis[1];
        const int np = I.npoints, lm = I.nlev, ncol = I.ncol;
        // MISR_simulator.f:294-313: one sub-column is the reference's serial scan over the points
        if (want_misr && ncol == 1) return fail(GEOSRAD_EINVAL, "geosrad_cosp_dev: the MISR simulator needs ncol of at least 2");
        MdWs m;
        if (const int rc = md_workspace(np, lm, ncol, true, m)) return rc;
        if (want_modis && !I.out[ICO_BOXPTOP]) I.out[ICO_BOXPTOP] = m.boxptop;      // ISCCP runs into the workspace for MODIS
        I.scops_only = !want_isccp && !want_modis;
        if (const int rc = icarus_dev(st, I)) return rc;
        SsWs w;
        if (const int rc = ss_workspace(np, lm, ncol, true, w)) return rc;      // no larger than icarus_dev's: the same planes, the mask among them
        if (want_misr) {
            hipLaunchKernelGGL((k_cosp_zfull<R>), dim3(grid256(np), lm), dim3(256), 0, st, np, lm, (const R *)C.zle, m.zfull);
            MisrCall M{np, lm, ncol, -1.0E30, I.sunlit, {m.zfull, I.in[IC_AT], I.in[IC_DTAU_S], I.in[IC_DTAU_C]}, w.mask,
                       {C.misr[MIO_FQ], C.misr[MIO_DIST], C.misr[MIO_ZTOP], C.misr[MIO_AREA]}};
            if (const int rc = misr_launch(st, M)) return rc;
        }
        if (want_modis) {
            ModisCall D{};
            D.npoints = np; D.nlev = lm; D.ncol = ncol; D.sunlit = I.sunlit; D.frac_out = w.mask; D.geos = true;
            D.in[MDI_T] = I.in[IC_AT]; D.in[MDI_P] = I.in[IC_PFULL]; D.in[MDI_PH] = I.in[IC_PHALF]; D.in[MDI_DTAU_S] = I.in[IC_DTAU_S];
            D.in[MDI_DTAU_C] = I.in[IC_DTAU_C];
            D.in[MDI_MR] = C.qltot; D.in[MDI_MR + 1] = C.qitot; D.in[MDI_REFF] = C.rdfl; D.in[MDI_REFF + 1] = C.rdfi;
            D.in[MDI_BOXPTOP] = I.out[ICO_BOXPTOP];
            D.out[MDO_MEAN] = C.modis[0]; D.out[MDO_HIST] = C.modis[1];
            if (const int rc = modis_launch(st, D)) return rc;
        }
        return GEOSRAD_OK;
    }

    // =====================================================================================================
    // the lidar simulator and the COSP path with it (include/geosrad_lidar.h; lidar_kernels.hpp)
    // =====================================================================================================
    DevBuf<> d_ws_lidar;      // eleven (npoints,nlev) planes, two (npoints,ncol) planes, one byte per cell and one per sub-column
    const LidarTab<R> ld_tab = ld_tables<R>();
    struct LdWs { R *pl[11], *tau_liq, *tau_ice; uint8_t *bin, *cat; };
    size_t ld_layout(int np, int nlev, int ncol, LdWs &w, Carve c) const
    {
        const size_t pl = (size_t)np * nlev, ps = (size_t)np * ncol;
        for (int k = 0; k < 11; k++) w.pl[k] = c.take<R>(pl);
        w.tau_liq = c.take<R>(ps); w.tau_ice = c.take<R>(ps);
        w.bin = c.take<uint8_t>(ps * nlev); w.cat = c.take<uint8_t>(ps);
        return c.off;
    }
    int lidar_dev(hipStream_t st, const LidarCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = lidar_check(C)) return rc;
        return lidar_launch(st, C);
    }
    // the three kernels on a record that lidar_check has passed
    int lidar_launch(hipStream_t st, const LidarCall &C)
    {
        LdWs w;
        const int np = C.npoints;
        if (d_ws_lidar.reserve(ld_layout(np, C.nlev, C.ncol, w, Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the lidar simulator's workspace failed");
        ld_layout(np, C.nlev, C.ncol, w, Carve(d_ws_lidar.p));
        LidarArgs<R> A{};
        A.npoints = np; A.nlev = C.nlev; A.ncol = C.ncol; A.ice_type = C.ice_type;
        A.ple_shift = C.geos; A.clamp_mr = C.geos; A.ocean = C.geos;
        auto I = [&](int k) { return (const R *)C.in[k]; };
        A.p = I(LDI_P); A.t = I(LDI_T); A.presf = I(LDI_PRESF); A.pplay = I(LDI_PPLAY); A.land = I(LDI_LAND);
        for (int k = 0; k < 4; k++) { A.mr[k] = I(LDI_MR + k); A.reff[k] = I(LDI_REFF + k); A.kp[k] = w.pl[5 + k]; }
        A.frac = (const uint8_t *)C.frac_out;
        A.dz = w.pl[0]; A.taumol = w.pl[1]; A.betamol = w.pl[2]; A.pmol = w.pl[3]; A.rho = w.pl[4]; A.frac_ls = w.pl[9]; A.frac_cv = w.pl[10];
        A.tau_liq = w.tau_liq; A.tau_ice = w.tau_ice; A.bin = w.bin; A.cat = w.cat;
        A.err = d_err + 5;
        auto O = [&](int k) { return (R *)C.out[k]; };
        A.lidarcld = O(LDO_CLD); A.cldlayer = O(LDO_LAYER); A.cfad = O(LDO_CFAD); A.parasol = O(LDO_PARASOL); A.o_pmol = O(LDO_PMOL);
        A.o_beta = O(LDO_BETA); A.o_tau = O(LDO_TAU); A.o_refl = O(LDO_REFL);
        A.tab = ld_tab;
        hipLaunchKernelGGL((k_lidar_point<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_lidar_box<R>), dim3(grid256((size_t)np * C.ncol)), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_lidar_stats<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int lidar_host(const LidarCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = lidar_check(C)) return rc;
        HostArrs H(sizeof(R));
        LidarCall D = C;
        const void *frac_at = nullptr, *u8_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev;
        for (int k = 0; k < LDI_NIN; k++) { D.in[k] = nullptr; if (C.in[k]) H.add(C.in[k], nullptr, lidar_in_shape(k, C.nlev), &D.in[k]); }
        H.add(C.frac_out, nullptr, {cells, 1}, &frac_at);
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        for (int k = 0; k < LDO_NOUT; k++) {
            D.out[k] = nullptr;
            if (C.out[k]) H.add(nullptr, C.out[k], lidar_out_shape(k, C.nlev, C.ncol), (const void **)&D.out[k]);
        }
        return host_call(C.npoints, H, 5, [&](hipStream_t st, int nc) {
            D.npoints = nc; D.frac_out = u8_at;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_real_to_mask<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const R *)frac_at, (uint8_t *)u8_at);
            return lidar_launch(st, D);
        });
    }
    // call COSP with all four simulators on: geosrad_cosp_dev's own path, then the lidar on the same SCOPS mask
    int cosp_lidar_dev(hipStream_t st, const CospLidarCall &C) override
    {
        bool want = false;
        for (int k = 0; k < 5; k++) want |= C.lidar[k] != nullptr;
        if (want && !C.frocean) return fail(GEOSRAD_EINVAL, "geosrad_cosp_lidar_dev: null input array");
        if (want && C.ice_type != 0 && C.ice_type != 1) return fail(GEOSRAD_EINVAL, "geosrad_cosp_lidar_dev: ice_type must be 0 or 1");
        if (const int rc = cosp_dev(st, C.cosp)) return rc;
        if (!want) return GEOSRAD_OK;
        const IcarusCall &I = C.cosp.ic;
        SsWs w;
        if (const int rc = ss_workspace(I.npoints, I.nlev, I.ncol, true, w)) return rc;      // no larger than cosp_dev's: the same planes, the mask among them
        LidarCall D{};
        D.npoints = I.npoints; D.nlev = I.nlev; D.ncol = I.ncol; D.ice_type = C.ice_type; D.frac_out = w.mask; D.geos = true;
        D.in[LDI_P] = I.in[IC_PFULL]; D.in[LDI_T] = I.in[IC_AT]; D.in[LDI_PRESF] = I.in[IC_PHALF]; D.in[LDI_PPLAY] = I.in[IC_PHALF];
        D.in[LDI_MR] = C.cosp.qltot; D.in[LDI_MR + 1] = C.cosp.qitot; D.in[LDI_REFF] = C.cosp.rdfl; D.in[LDI_REFF + 1] = C.cosp.rdfi;
        D.in[LDI_LAND] = C.frocean;
        for (int k = 0; k < 5; k++) D.out[k] = C.lidar[k];
        return lidar_launch(st, D);
    }

    // =====================================================================================================
    // the radar simulator's front end (include/geosrad_radar.h; radar_kernels.hpp)
    // =====================================================================================================
    DevBuf<> d_ws_radar;      // what the call at hand needs of: one byte per (point, sub-column) and per cell, nine and five (npoints,nlev) planes
    // prec_scops on a record that prec_scops_check has passed; the rates are sums of up to three / two device planes (cosp.F90:404-408)
    int prec_launch(hipStream_t st, int np, int nlev, int ncol, const R *const *ls, const R *const *cv, const uint8_t *frac, uint8_t *prec, uint8_t *colflag)
    {
        PrecArgs<R> A{};
        A.npoints = np; A.nlev = nlev; A.ncol = ncol;
        {
#pragma clang fp contract(off)
            A.cv_col = (int)((R)0.05 * (R)ncol);      // prec_scops.f:54-55, formed in the real kind
        }
        if (A.cv_col == 0) A.cv_col = 1;
        for (int k = 0; k < 3; k++) A.ls[k] = ls[k];
        for (int k = 0; k < 2; k++) A.cv[k] = cv[k];
        A.frac = frac; A.prec = prec; A.colflag = colflag;
        hipLaunchKernelGGL((k_prec_columns<R>), dim3(grid256((size_t)np * ncol)), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_prec_scops<R>), dim3(grid256(np)), dim3(256), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int prec_scops_dev(hipStream_t st, const PrecScopsCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = prec_scops_check(C)) return rc;
        if (d_ws_radar.reserve((size_t)C.npoints * C.ncol) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the radar front end's workspace failed");
        const R *ls[3] = {(const R *)C.ls, nullptr, nullptr}, *cv[2] = {(const R *)C.cv, nullptr};
        return prec_launch(st, C.npoints, C.nlev, C.ncol, ls, cv, (const uint8_t *)C.frac_out, (uint8_t *)C.prec_frac, (uint8_t *)d_ws_radar.p);
    }
    int prec_scops_host(const PrecScopsCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = prec_scops_check(C)) return rc;
        HostArrs H(sizeof(R));
        PrecScopsCall D = C;
        const void *frac_at = nullptr, *u8_at = nullptr, *p8_at = nullptr, *prec_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev;
        H.add(C.ls, nullptr, {(size_t)C.nlev, 1}, &D.ls);
        H.add(C.cv, nullptr, {(size_t)C.nlev, 1}, &D.cv);
        H.add(C.frac_out, nullptr, {cells, 1}, &frac_at);
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        H.add(nullptr, nullptr, {cells, 1}, &p8_at, 1);
        H.add(nullptr, C.prec_frac, {cells, 1}, &prec_at);
        const int rc = host_call(C.npoints, H, -1, [&](hipStream_t st, int nc) {
            D.npoints = nc; D.frac_out = u8_at; D.prec_frac = (void *)p8_at;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_real_to_mask<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const R *)frac_at, (uint8_t *)u8_at);
            if (const int r = prec_scops_dev(st, D)) return r;
            hipLaunchKernelGGL((k_mask_to_real<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const uint8_t *)p8_at, (R *)prec_at);
            return hip_rc("k_mask_to_real", hipGetLastError());
        });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        return GEOSRAD_OK;
    }
    // the sub-grid hydrometeor contents on a byte mask in HBM (a caller's, or the one SCOPS left in the workspace)
    struct SgWs { uint8_t *colflag, *prec; R *mr_sub; };
    size_t sg_layout(const SgHydroCall &C, SgWs &w, Carve c) const
    {
        const size_t np = (size_t)C.npoints;
        w.colflag = c.take<uint8_t>(np * C.ncol);
        w.prec = C.prec_frac ? nullptr : c.take<uint8_t>(np * C.ncol * C.nlev);
        w.mr_sub = (C.out[SGO_MR_SUB] || !C.out[SGO_MR_SG]) ? nullptr : c.take<R>(np * C.nlev * GEOSRAD_NHYDRO);
        return c.off;
    }
    int sghydro_launch(hipStream_t st, const SgHydroCall &C)
    {
        SgWs w;
        const int np = C.npoints;
        if (d_ws_radar.reserve(sg_layout(C, w, Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the radar front end's workspace failed");
        sg_layout(C, w, Carve(d_ws_radar.p));
        SgHydroArgs<R> A{};
        A.npoints = np; A.nlev = C.nlev; A.ncol = C.ncol;
        A.frac = (const uint8_t *)C.frac_out;
        uint8_t *prec = C.prec_frac ? (uint8_t *)C.prec_frac : w.prec;
        A.prec = prec;
        for (int k = 0; k < GEOSRAD_NHYDRO; k++) A.mr[k] = (const R *)C.mr[k];
        auto O = [&](int k) { return (R *)C.out[k]; };
        A.frac_ls = O(SGO_FRAC_LS); A.frac_cv = O(SGO_FRAC_CV); A.prec_ls = O(SGO_PREC_LS); A.prec_cv = O(SGO_PREC_CV);
        A.mr_sub = C.out[SGO_MR_SUB] ? O(SGO_MR_SUB) : w.mr_sub; A.mr_sg = O(SGO_MR_SG);
        // cosp.F90:404-408: rain + snow + graupel, convective rain + snow
        const R *ls[3] = {A.mr[GEOSRAD_HYDRO_LSRAIN], A.mr[GEOSRAD_HYDRO_LSSNOW], A.mr[GEOSRAD_HYDRO_LSGRPL]};
        const R *cv[2] = {A.mr[GEOSRAD_HYDRO_CVRAIN], A.mr[GEOSRAD_HYDRO_CVSNOW]};
        if (const int rc = prec_launch(st, np, C.nlev, C.ncol, ls, cv, A.frac, prec, w.colflag)) return rc;
        hipLaunchKernelGGL((k_sghydro<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, A);
        if (A.mr_sg) hipLaunchKernelGGL((k_sghydro_expand<R>), dim3(grid256((size_t)np * C.ncol), C.nlev), dim3(256), 0, st, A);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int sghydro_dev(hipStream_t st, const SgHydroCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = sghydro_check(C)) return rc;
        return sghydro_launch(st, C);
    }
    int sghydro_host(const SgHydroCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = sghydro_check(C)) return rc;
        HostArrs H(sizeof(R));
        SgHydroCall D = C;
        const void *frac_at = nullptr, *u8_at = nullptr, *p8_at = nullptr, *prec_at = nullptr;
        const size_t cells = (size_t)C.ncol * C.nlev, L = (size_t)C.nlev;
        const size_t rows[SGO_NOUT] = {L, L, L, L, L * GEOSRAD_NHYDRO, cells * GEOSRAD_NHYDRO};
        for (int k = 0; k < GEOSRAD_NHYDRO; k++) { D.mr[k] = nullptr; if (C.mr[k]) H.add(C.mr[k], nullptr, {L, 1}, &D.mr[k]); }
        H.add(C.frac_out, nullptr, {cells, 1}, &frac_at);
        H.add(nullptr, nullptr, {cells, 1}, &u8_at, 1);
        if (C.prec_frac) { H.add(nullptr, nullptr, {cells, 1}, &p8_at, 1); H.add(nullptr, C.prec_frac, {cells, 1}, &prec_at); }
        for (int k = 0; k < SGO_NOUT; k++) { D.out[k] = nullptr; if (C.out[k]) H.add(nullptr, C.out[k], {rows[k], 1}, (const void **)&D.out[k]); }
        const int rc = host_call(C.npoints, H, -1, [&](hipStream_t st, int nc) {
            D.npoints = nc; D.frac_out = u8_at; D.prec_frac = (void *)p8_at;
            const size_t nn = cells * nc;
            hipLaunchKernelGGL((k_real_to_mask<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const R *)frac_at, (uint8_t *)u8_at);
            if (const int r = sghydro_launch(st, D)) return r;
            if (p8_at) hipLaunchKernelGGL((k_mask_to_real<R>), dim3(grid256(nn)), dim3(256), 0, st, nn, (const uint8_t *)p8_at, (R *)prec_at);
            return hip_rc("k_mask_to_real", hipGetLastError());
        });
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        return GEOSRAD_OK;
    }
    // the gaseous attenuation: every volume's, then the path to every gate
    int radar_gases_launch(hipStream_t st, const GasCall &C)
    {
        const int np = C.npoints;
        const size_t pl = (size_t)np * C.nlev;
        GasArgs<R> A{};
        auto carve = [&](Carve c) {
            A.g = c.take<double>(pl); A.x = c.take<double>(pl); A.ca = c.take<double>(pl); A.cb = c.take<double>(pl); A.cc = c.take<double>(pl);
            return c.off;
        };
        if (d_ws_radar.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the radar front end's workspace failed");
        carve(Carve(d_ws_radar.p));
        A.npoints = np; A.nlev = C.nlev; A.surface_radar = C.surface_radar; A.freq = C.freq;
        A.p = (const R *)C.in[GI_P]; A.t = (const R *)C.in[GI_T]; A.rh = (const R *)C.in[GI_RH]; A.zlev = (const R *)C.in[GI_ZLEV];
        A.g_vol = (double *)C.out[0]; A.g_to_vol = (double *)C.out[1];
        A.err = d_err + 6;
        hipLaunchKernelGGL((k_radar_gases<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, A);
        if (A.g_to_vol) {
            if (C.nlev > 2) hipLaunchKernelGGL((k_radar_gas_parab<R>), dim3(grid256(np), C.nlev - 2), dim3(256), 0, st, A);
            hipLaunchKernelGGL((k_radar_gas_path<R>), dim3(grid256(np), C.nlev), dim3(256), 0, st, A);
        }
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }
    int radar_gases_dev(hipStream_t st, const GasCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = radar_gases_check(C)) return rc;
        return radar_gases_launch(st, C);
    }
    int radar_gases_host(const GasCall &C) override
    {
        HIPCHK(hipSetDevice(device));
        if (const int rc = radar_gases_check(C)) return rc;
        HostArrs H(sizeof(R));
        GasCall D = C;
        for (int k = 0; k < GI_NIN; k++) H.add(C.in[k], nullptr, {(size_t)C.nlev, 1}, &D.in[k]);
        for (int k = 0; k < 2; k++) { D.out[k] = nullptr; if (C.out[k]) H.add(nullptr, C.out[k], {(size_t)C.nlev, 1}, (const void **)&D.out[k], sizeof(double)); }
        return host_call(C.npoints, H, 6, [&](hipStream_t st, int nc) {
            D.npoints = nc;
            return radar_gases_launch(st, D);
        });
    }

    // in: ple, t, fcld, qi, ql, qr, qs, ri, rl, rr, rs; out: tauir, cldtmp, cldprs
    int lw_cloud_diag_dev(hipStream_t st, int ncol, int lm, double grav, double undef, double taucrit, const void *const *in,
                          void *const *out) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || lm < 1) return fail(GEOSRAD_EINVAL, "geosrad_lw_cloud_diag_dev: ncol must be positive and lm at least 1");
        if (!have_chou) return fail(GEOSRAD_EINVAL, "Chou-Suarez LW tables not set: call geosrad_load_tables_chou_lw first");
        if (!out[0] && !out[1] && !out[2]) return fail(GEOSRAD_EINVAL, "geosrad_lw_cloud_diag_dev: every output is NULL");
        for (int k = 0; k < 11; k++)
            if (!in[k] && k != 2 && k != 9 && !(k == 1 && !out[1])) return fail(GEOSRAD_EINVAL, "geosrad_lw_cloud_diag_dev: null input field");
        LwCldDiag<R> D{};
        D.ncol = ncol; D.lm = lm; D.grav = (R)grav; D.undef = (R)undef; D.taucrit = (R)taucrit / (R)2.13;
        D.ple = (const R *)in[0]; D.t = (const R *)in[1];
        for (int s = 0; s < 4; s++) { D.q[s] = (const R *)in[3 + s]; D.r[s] = (const R *)in[7 + s]; }
        D.tauir = (R *)out[0]; D.cldtmp = (R *)out[1]; D.cldprs = (R *)out[2];
        hipLaunchKernelGGL((k_lw_cloud_diag<R>), dim3(grid256(ncol)), dim3(256), 0, st, D, (const ChouDev<R> *)d_C);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    // ---- stand-alone McICA generator ---------------------------------------------------------------------------------
    DevBuf<> d_mc;      // alpha / rcorr scratch of the stand-alone generator
    std::map<std::tuple<int, int, int>, DevBuf<KissJump>> sa_jumps;      // (nsubcol, nlay, inhomogeneous?) -> jump to every sub-column
    int mcica_dev(hipStream_t st, int ncol, int nsubcol, int nlay, const void *zmid, const void *alat, int doy, const void *play,
                  const void *cldfrac, const void *ciwp, const void *clwp, double cwp_tiny, const int32_t *so, int32_t *cldy,
                  void *ciwp_s, void *clwp_s) override
    {
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || nlay < 4 || nsubcol <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/nlay/nsubcol");
        // seed_order validation as in the reference (cloud_subcol_gen.F90:273-295)
        int sov[4] = {1, 2, 3, 4};
        if (so) {
            for (int k = 0; k < 4; k++) {
                if (so[k] < 1) return fail(GEOSRAD_EINPUT, "seed_order element < 1");
                if (so[k] > 4) return fail(GEOSRAD_EINPUT, "seed_order element > 4");
                sov[k] = so[k];
            }
        }
        const size_t cl = (size_t)ncol * nlay;
        R *d_alpha, *d_rcorr;
        auto carve = [&](Carve c) { d_alpha = c.take<R>(cl); d_rcorr = c.take<R>(cl); return c.off; };
        if (d_mc.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the McICA scratch failed");
        carve(Carve(d_mc));
        const unsigned gx = grid256(ncol);
        span_begin(2, st);
        hipLaunchKernelGGL(k_overlap<R>, dim3(gx, nlay), dim3(256), 0, st, ncol, ncol, nlay, doy, (const R *)zmid, (const R *)alat,
                           (const int32_t *)nullptr, (const int32_t *)nullptr, (const LwDev<R> *)d_T, d_alpha, d_rcorr, (uint8_t *)nullptr);
        span_end(st);
        McArgs<R> M{};
        M.ncol = ncol; M.ld = ncol; M.nlay = nlay; M.nsubcol = nsubcol; M.doy = doy; M.cloudLM = 1; M.cloudMH = 2;
        for (int k = 0; k < 4; k++) M.so[k] = sov[k];
        M.cwp_tiny = (R)cwp_tiny;
        M.play = (const R *)play; M.cldf = (const R *)cldfrac; M.ciwp = (const R *)ciwp; M.clwp = (const R *)clwp;
        M.alpha = d_alpha; M.rcorr = d_rcorr;
        M.cldy = cldy; M.ciwp_s = (R *)ciwp_s; M.clwp_s = (R *)clwp_s;
        McPlan MP; int nseg = 0;
        if (const int rc = mc_plan(1, nsubcol, nlay, MP, nseg)) return rc;
        const size_t lds = mc_sa_lds_reals(nlay, nsubcol) * sizeof(R);
        const long nblk = ((long)ncol * nsubcol + 64 * MC_SA_K - 1) / (64 * MC_SA_K);
        span_begin(3, st);
        if (lds <= 160 * 1024 && nblk <= 0x7FFFFFFFL && !getenv("GEOSRAD_MCICA_LANE_COLUMN")) {
            // lane = (column, sub-column) pair, outputs written row-major through an LDS tile (k_mcica_sa)
            const bool inhomo = h_T.xcw != nullptr;
            const auto key = std::make_tuple(nsubcol, nlay, inhomo ? 1 : 0);
            auto it = sa_jumps.find(key);
            if (it == sa_jumps.end()) {
                const uint64_t per = (uint64_t)(inhomo ? 4 : 2) * (uint64_t)nlay;
                std::vector<KissJump> js((size_t)nsubcol);
                for (int q = 0; q < nsubcol; q++) js[q] = make_kiss_jump((uint64_t)q * per);
                DevBuf<KissJump> dj;
                HIPCHK(dj.resize(js.size() * sizeof(KissJump)));
                HIPCHK(hipMemcpy(dj, js.data(), dj.bytes, hipMemcpyHostToDevice));
                it = sa_jumps.emplace(key, std::move(dj)).first;
            }
            if (lds > 65536) HIPCHK(hipFuncSetAttribute((const void *)k_mcica_sa<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((k_mcica_sa<R>), dim3((unsigned)nblk), dim3(64), lds, st, M, (const KissJump *)it->second.p, MP.jhalf,
                               (const LwDev<R> *)d_T);
        } else {
            // lane = column (tiles beyond 64 KB of LDS: fp64 with more than 127 layers)
            hipLaunchKernelGGL((k_mcica<R, 1>), dim3(xcd_grid(ncol, 64, nseg)), dim3(64), 0, st, M, MP, (const LwDev<R> *)d_T, (const SwDev<R> *)nullptr);
        }
        span_end(st);
        HIPCHK(hipGetLastError());
        return GEOSRAD_OK;
    }

    int mcica_host(int ncol, int nsubcol, int nlay, const void *zmid, const void *alat, int doy, const void *play, const void *cldfrac,
                   const void *ciwp, const void *clwp, double cwp_tiny, const int32_t *so, int32_t *cldy, void *ciwp_s,
                   void *clwp_s) override
    {
        // not through host_pipeline: the outputs are 12 B x nlay x nsubcol per column (173 KB at 72 x 200), so a 16 384-column chunk would
        // make each of the three pinned and device slots 2.8 GB.  The one user of d_io.
        HIPCHK(hipSetDevice(device));
        if (ncol <= 0 || nlay < 4 || nsubcol <= 0) return fail(GEOSRAD_EINVAL, "bad ncol/nlay/nsubcol");
        const size_t cl = (size_t)ncol * nlay, co = cl * nsubcol;
        R *d[6], *d_ci, *d_cl;      // zmid, play, cldfrac, ciwp, clwp (nlay, ncol), alat (ncol); the generator's three outputs behind them
        int32_t *d_cy;
        auto carve = [&](Carve c) {
            for (int k = 0; k < 6; k++) d[k] = c.take<R>(k == 5 ? (size_t)ncol : cl);
            d_cy = c.take<int32_t>(co); d_ci = c.take<R>(co); d_cl = c.take<R>(co);
            return c.off;
        };
        if (d_io.reserve(carve(Carve())) != hipSuccess) return fail(GEOSRAD_ENOMEM, "hipMalloc of the host-API staging buffer failed");
        carve(Carve(d_io));
        const void *src[6] = {zmid, play, cldfrac, ciwp, clwp, alat};
        for (int k = 0; k < 6; k++)
            HIPCHK(hipMemcpyAsync(d[k], src[k], (k == 5 ? (size_t)ncol : cl) * sizeof(R), hipMemcpyHostToDevice, stream));
        if (const int rc = mcica_dev(stream, ncol, nsubcol, nlay, d[0], d[5], doy, d[1], d[2], d[3], d[4], cwp_tiny, so, d_cy, d_ci, d_cl)) return rc;
        HIPCHK(hipMemcpyAsync(cldy, d_cy, co * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(ciwp_s, d_ci, co * sizeof(R), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(clwp_s, d_cl, co * sizeof(R), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return GEOSRAD_OK;
    }
};
#undef LAUNCH_WIDE
}  // namespace

#if !defined(GEOSRAD_PART) || GEOSRAD_PART == 4
geosrad_ctx *geosrad_new_ctx_f32() { return new Ctx<float>(); }
#endif
#if !defined(GEOSRAD_PART) || GEOSRAD_PART == 8
geosrad_ctx *geosrad_new_ctx_f64() { return new Ctx<double>(); }
#endif
#endif   // GEOSRAD_PART != 0

#if !defined(GEOSRAD_PART) || GEOSRAD_PART == 0
// ---------------------------------------------------------------------------------------------------
// extern "C"
// ---------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------
// A context over several devices (`geosrad_create(ctx**, device_ids, ndev, kind)`; 2a: "splitting that batch ... ways").
// It owns one single-device context per entry of device_ids; the host-pointer solver entry points cut [0, ncol) into ndev contiguous
// shards and run one child's pipeline per shard concurrently (one host thread each; a child reads / writes its shard of the
// caller's arrays in place: base pointer + shard start, leading dimension = the full ncol).  Columns are independent, so the
// result is bitwise the single-device one (tested with device_ids = {0, 0}).  Table / parameter setters go to every child;
// the `_dev` entry points keep geosrad_ctx's refusal.
// ---------------------------------------------------------------------------------------------------
namespace {
struct MultiCtx final : geosrad_ctx {
    std::vector<geosrad_ctx *> kid;
    ~MultiCtx() override { for (auto *k : kid) { (void)hipSetDevice(k->device); delete k; } }
    int init() override { return GEOSRAD_OK; }
    int all(const std::function<int(geosrad_ctx *)> &f)
    {
        for (auto *k : kid) { const int rc = f(k); if (rc) { last_error = k->last_error; return rc; } }
        return GEOSRAD_OK;
    }
    // shard s of n columns: [start, start + count)
    static void shard(int n, int nk, int s, int &start, int &count) { const int per = (n + nk - 1) / nk; start = s * per; count = start >= n ? 0 : (n - start < per ? n - start : per); }
    // fn(child, first column, columns) per shard, concurrently; the first failing shard's status and message
    int run_shards(int ncol, const std::function<int(geosrad_ctx *, int, int)> &fn)
    {
        const int nk = (int)kid.size();
        std::vector<int> rc(nk, GEOSRAD_OK);
        std::vector<std::thread> th;
        for (int s = 0; s < nk; s++) {
            int c0, nc; shard(ncol, nk, s, c0, nc);
            if (nc <= 0) continue;
            th.emplace_back([&, s, c0, nc] { kid[s]->host_ld = (size_t)ncol; rc[s] = fn(kid[s], c0, nc); kid[s]->host_ld = 0; });
        }
        for (auto &t : th) t.join();
        for (int s = 0; s < nk; s++) if (rc[s]) { last_error = kid[s]->last_error; return rc[s]; }
        return GEOSRAD_OK;
    }
    // a shard's part of a caller's array: its first column lies c0 records in (ArrShape::rec reals each)
    const void *off(const void *p, int c0, ArrShape s = {1, 1}) const { return p ? (const char *)p + (size_t)c0 * s.rec * (size_t)real_kind : nullptr; }
    void *off(void *p, int c0, ArrShape s = {1, 1}) const { return p ? (char *)p + (size_t)c0 * s.rec * (size_t)real_kind : nullptr; }

    int set_tables_lw(const void *b, size_t n) override { return all([&](geosrad_ctx *k) { return k->set_tables_lw(b, n); }); }
    int set_tables_sw(const void *b, size_t n) override { return all([&](geosrad_ctx *k) { return k->set_tables_sw(b, n); }); }
    int set_tables_chou_lw(const void *b, size_t n) override { return all([&](geosrad_ctx *k) { return k->set_tables_chou_lw(b, n); }); }
    int set_tables_chou_sw(const void *b, size_t n) override { return all([&](geosrad_ctx *k) { return k->set_tables_chou_sw(b, n); }); }
    int set_inhomogeneity(int ih, const void *b, size_t n) override { return all([&](geosrad_ctx *k) { return k->set_inhomogeneity(ih, b, n); }); }
    int set_corr(const double *a, const double *r) override { return all([&](geosrad_ctx *k) { return k->set_corr(a, r); }); }
    size_t workspace_bytes() const override { size_t t = 0; for (auto *k : kid) t += k->workspace_bytes(); return t; }
    int check(hipStream_t, int which) override { return all([&](geosrad_ctx *k) { (void)hipSetDevice(k->device); return k->check(k->stream, which); }); }

    int lw_host(int ncol, int nlay, int dudTs, const void *const *in, int iceflg, int liqflg, int dyofyr, int cloudLM, int cloudMH,
                int32_t *clearCounts, void *const *out, const int32_t *band_output, void *taug, void *pfracs) override
    {
        if (taug || pfracs) return fail(GEOSRAD_EINVAL, "stage dumps need a single-device context");
        return run_shards(ncol, [&](geosrad_ctx *k, int c0, int nc) {
            const void *i2[I_NIN]; void *o2[O_NOUT];
            for (int j = 0; j < I_NIN; j++) i2[j] = off(in[j], c0, lw_in_shape(j, nlay));
            for (int j = 0; j < O_NOUT; j++) o2[j] = off(out[j], c0, lw_out_shape(j, nlay));
            return k->lw_host(nc, nlay, dudTs, i2, iceflg, liqflg, dyofyr, cloudLM, cloudMH, clearCounts ? clearCounts + c0 : nullptr, o2,
                              band_output, nullptr, nullptr);
        });
    }
    int sw_host(int ncol, int nlay, double scon, double adjes, int isolvar, const void *const *in, int iceflg, int liqflg, int dyofyr,
                int iaer, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *const *out, int do_drfband, const void *bndscl,
                const void *indsolvar, const void *solcycfrac, void *const *dbg, void *radval) override
    {
        if (dbg) return fail(GEOSRAD_EINVAL, "stage dumps need a single-device context");
        return run_shards(ncol, [&](geosrad_ctx *k, int c0, int nc) {
            const void *i2[S_NIN]; void *o2[SO_NOUT];
            for (int j = 0; j < S_NIN; j++) i2[j] = off(in[j], c0, sw_in_shape(j, nlay));
            for (int j = 0; j < SO_NOUT; j++) o2[j] = off(out[j], c0, sw_out_shape(j, nlay));
            return k->sw_host(nc, nlay, scon, adjes, isolvar, i2, iceflg, liqflg, dyofyr, iaer, cloudLM, cloudMH, normFlx,
                              clearCounts ? clearCounts + c0 : nullptr, o2, do_drfband, bndscl, indsolvar, solcycfrac, nullptr,
                              off(radval, c0));
        });
    }
    int irrad_host(int m, int np, const void *const *in, double co2, int trace, int ict, int icb, int ns, int na, int nb, void *const *aer,
                   void *const *out) override
    {
        return run_shards(m, [&](geosrad_ctx *k, int c0, int nc) {
            const void *i2[C_NIN]; void *a2[3], *o2[CO_NOUT];
            for (int j = 0; j < C_NIN; j++) i2[j] = off(in[j], c0, ch_in_shape(j, np, ns));
            for (int j = 0; j < 3; j++) a2[j] = off(aer[j], c0, ch_aer_shape(np, nb));
            for (int j = 0; j < CO_NOUT; j++) o2[j] = off(out[j], c0, ch_out_shape(j, np));
            return k->irrad_host(nc, np, i2, co2, trace, ict, icb, ns, na, nb, a2, o2);
        });
    }
    int sorad_host(int m, int np, int nb, const void *const *in, double co2, int ict, int icb, const void *hk_uv, const void *hk_ir,
                   void *const *out, int do_drfband, void *const *na_out) override
    {
        return run_shards(m, [&](geosrad_ctx *k, int c0, int nc) {
            const void *i2[SI_NIN]; void *o2[SOO_NOUT], *n2[GEOSRAD_SONA_NOUT];
            for (int j = 0; j < SI_NIN; j++) i2[j] = off(in[j], c0, so_in_shape(j, np, nb));
            for (int j = 0; j < SOO_NOUT; j++) o2[j] = off(out[j], c0, so_out_shape(j, np));
            for (int j = 0; j < GEOSRAD_SONA_NOUT; j++) n2[j] = na_out ? off(na_out[j], c0, so_out_shape(SONA_TWIN[j], np)) : nullptr;
            return k->sorad_host(nc, np, nb, i2, co2, ict, icb, hk_uv, hk_ir, o2, do_drfband, n2);
        });
    }
    int gettau_host(const GtCall &C) override
    {
        if (const int rc = gettau_check(C)) return rc;
        return run_shards(C.ncol, [&](geosrad_ctx *k, int c0, int nc) {
            GtCall S = C;
            S.ncol = nc;
            S.cosz = off(C.cosz, c0); S.dp = off(C.dp, c0); S.fcld = off(C.fcld, c0); S.reff = off(C.reff, c0); S.hyd = off(C.hyd, c0);
            for (int j = 0; j < 4; j++) S.out[j] = off(C.out[j], c0);
            return k->gettau_host(S);
        });
    }
    int scops_host(const ScopsCall &C) override
    {
        if (const int rc = scops_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            ScopsCall S = C;
            S.npoints = nc; S.seed = C.seed + c0; S.cc = off(C.cc, c0); S.conv = off(C.conv, c0); S.frac_out = off(C.frac_out, c0);
            return k->scops_host(S);
        });
    }
    int icarus_host(const IcarusCall &C) override
    {
        if (const int rc = icarus_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            IcarusCall S = C;
            S.npoints = nc; S.sunlit = C.sunlit + c0; S.frac_out = off(C.frac_out, c0);
            for (int j = 0; j < IC_NIN; j++) S.in[j] = off(C.in[j], c0);
            for (int j = 0; j < ICO_NOUT; j++) S.out[j] = off(C.out[j], c0);
            return k->icarus_host(S);
        });
    }
    int misr_host(const MisrCall &C) override
    {
        if (const int rc = misr_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            MisrCall S = C;
            S.npoints = nc; S.sunlit = C.sunlit + c0; S.frac_out = off(C.frac_out, c0);
            S.first = C.first && c0 == 0; S.last = C.last && c0 + nc == C.npoints;
            for (int j = 0; j < MI_NIN; j++) S.in[j] = off(C.in[j], c0);
            for (int j = 0; j < MIO_NOUT; j++) S.out[j] = off(C.out[j], c0);
            return k->misr_host(S);
        });
    }
    int modis_host(const ModisCall &C) override
    {
        if (const int rc = modis_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            ModisCall S = C;
            S.npoints = nc; S.sunlit = C.sunlit + c0; S.frac_out = off(C.frac_out, c0);
            for (int j = 0; j < MDI_NIN; j++) S.in[j] = off(C.in[j], c0);
            for (int j = 0; j < MDO_NOUT; j++) S.out[j] = j == MDO_PHASE && C.out[j] ? (void *)((int32_t *)C.out[j] + c0) : off(C.out[j], c0);
            return k->modis_host(S);
        });
    }
    int lidar_host(const LidarCall &C) override
    {
        if (const int rc = lidar_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            LidarCall S = C;
            S.npoints = nc; S.frac_out = off(C.frac_out, c0);
            for (int j = 0; j < LDI_NIN; j++) S.in[j] = off(C.in[j], c0);
            for (int j = 0; j < LDO_NOUT; j++) S.out[j] = off(C.out[j], c0);
            return k->lidar_host(S);
        });
    }
    int prec_scops_host(const PrecScopsCall &C) override
    {
        if (const int rc = prec_scops_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            PrecScopsCall S = C;
            S.npoints = nc; S.ls = off(C.ls, c0); S.cv = off(C.cv, c0); S.frac_out = off(C.frac_out, c0); S.prec_frac = off(C.prec_frac, c0);
            return k->prec_scops_host(S);
        });
    }
    int sghydro_host(const SgHydroCall &C) override
    {
        if (const int rc = sghydro_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            SgHydroCall S = C;
            S.npoints = nc; S.frac_out = off(C.frac_out, c0); S.prec_frac = off(C.prec_frac, c0);
            for (int j = 0; j < GEOSRAD_NHYDRO; j++) S.mr[j] = off(C.mr[j], c0);
            for (int j = 0; j < SGO_NOUT; j++) S.out[j] = off(C.out[j], c0);
            return k->sghydro_host(S);
        });
    }
    int radar_gases_host(const GasCall &C) override
    {
        if (const int rc = radar_gases_check(C)) return rc;
        return run_shards(C.npoints, [&](geosrad_ctx *k, int c0, int nc) {
            GasCall S = C;
            S.npoints = nc;
            for (int j = 0; j < GI_NIN; j++) S.in[j] = off(C.in[j], c0);
            for (int j = 0; j < 2; j++) S.out[j] = C.out[j] ? (char *)C.out[j] + (size_t)c0 * sizeof(double) : nullptr;      // doubles in either kind
            return k->radar_gases_host(S);
        });
    }
    int mcica_host(int, int, int, const void *, const void *, int, const void *, const void *, const void *, const void *, double,
                   const int32_t *, int32_t *, void *, void *) override { return fail(GEOSRAD_EINVAL, "geosrad_mcica needs a single-device context"); }
};
}  // namespace

extern "C" {

// Which device a process should use when nothing says so explicitly: GEOSRAD_DEVICE if set, else the node-local MPI rank the launcher
// exports (Open MPI, Slurm, MVAPICH2, Intel MPI / MPICH Hydra) modulo the number of visible devices - 96 ranks of a GEOS job on an
// 8-GPU node then share the GPUs 12 to one without any configuration (the reference balances its ranks' work, not its devices:
// GEOS_SolarGridComp.F90:3701-3709).  Pure function of the environment and ndev (no HIP call): 0 when nothing is set.
int geosrad_pick_device(int ndev)
{
    if (ndev <= 0) return 0;
    // an explicit device id is taken as it is: out of range (a stale or mistyped GEOSRAD_DEVICE) is an error (-1 -> GEOSRAD_ENODEV from
    // geosrad_create), not another GPU; only the launchers' node-local ranks wrap around the device count
    if (const char *e = getenv("GEOSRAD_DEVICE")) {
        if (*e) {
            char *end = nullptr;
            const long r = strtol(e, &end, 10);
            return (end == e || *end || r < 0 || r >= ndev) ? -1 : (int)r;
        }
    }
    static const char *vars[] = {"OMPI_COMM_WORLD_LOCAL_RANK", "SLURM_LOCALID", "MV2_COMM_WORLD_LOCAL_RANK", "MPI_LOCALRANKID", "PMI_LOCAL_RANK"};
    for (const char *v : vars) {
        const char *e = getenv(v);
        if (!e || !*e) continue;
        char *end = nullptr;
        const long r = strtol(e, &end, 10);
        if (end == e || r < 0) continue;
        return (int)(r % ndev);
    }
    return 0;
}

int geosrad_create_multi(geosrad_ctx **out, const int *device_ids, int ndev, int real_kind)
{
    if (!out || !device_ids || ndev < 1 || (real_kind != 4 && real_kind != 8)) return GEOSRAD_EINVAL;
    *out = nullptr;
    MultiCtx *m = new MultiCtx();
    m->real_kind = real_kind; m->device = device_ids[0];
    for (int k = 0; k < ndev; k++) {
        geosrad_ctx *c = nullptr;
        const int rc = geosrad_create(&c, device_ids[k], real_kind);
        if (rc) { delete m; return rc; }
        m->kid.push_back(c);
    }
    *out = m;
    return GEOSRAD_OK;
}

int geosrad_create(geosrad_ctx **out, int device_id, int real_kind)
{
    if (!out || (real_kind != 4 && real_kind != 8)) return GEOSRAD_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GEOSRAD_ENODEV;
    if (device_id == GEOSRAD_DEVICE_AUTO) device_id = geosrad_pick_device(ndev);
    if (device_id < 0 || device_id >= ndev) return GEOSRAD_ENODEV;
    geosrad_ctx *c = real_kind == 4 ? geosrad_new_ctx_f32() : geosrad_new_ctx_f64();
    c->device = device_id; c->real_kind = real_kind;
    {   // A/B switch for the measurements in profiles/: GEOSRAD_LW_PATH=cols | bands
        const char *e = getenv("GEOSRAD_LW_PATH");
        if (e) { c->lw_cols_path = !strcmp(e, "cols"); c->lw_split_path = !strcmp(e, "split"); }
        e = getenv("GEOSRAD_SW_PATH");
        if (e) c->sw_path = !strcmp(e, "bands") ? 0 : 2;
        if ((e = getenv("GEOSRAD_SORAD_PATH"))) c->sorad_col_path = !strcmp(e, "col");
        // tuning of the host-pointer pipeline: columns per staged chunk, copy threads
        if ((e = getenv("GEOSRAD_HOST_CHUNK")) && atoi(e) >= 64) c->host_chunk = c->host_chunk_default = atoi(e);
        if ((e = getenv("GEOSRAD_HOST_THREADS")) && atoi(e) >= 1) c->host_threads = atoi(e) > 64 ? 64 : atoi(e);
        if ((e = getenv("GEOSRAD_HOST_NT"))) c->host_nt = atoi(e) != 0;
    }
    int rc = c->init();
    if (rc) { delete c; return rc; }
    *out = c;
    return GEOSRAD_OK;
}

int geosrad_destroy(geosrad_ctx *c) { if (!c) return GEOSRAD_EINVAL; (void)hipSetDevice(c->device); delete c; return GEOSRAD_OK; }
// ctx-less entry points (geosrad_obio_weights) leave their complaint here, per thread
static thread_local std::string g_ctxless_error;
const char *geosrad_last_error(const geosrad_ctx *c) { return c ? c->last_error.c_str() : g_ctxless_error.empty() ? "null context" : g_ctxless_error.c_str(); }
int geosrad_real_kind(const geosrad_ctx *c) { return c ? c->real_kind : 0; }
int geosrad_set_chunk(geosrad_ctx *c, int n)
{
    if (!c || n < 64) return GEOSRAD_EINVAL;
    if (auto *m = dynamic_cast<MultiCtx *>(c)) { for (auto *k : m->kid) (void)geosrad_set_chunk(k, n); return GEOSRAD_OK; }
    c->chunk = n;
    c->host_chunk = n < c->host_chunk_default ? n : c->host_chunk_default;      // the host-pointer pipeline never stages more than a batch
    return GEOSRAD_OK;
}
size_t geosrad_workspace_bytes(const geosrad_ctx *c) { return c ? c->workspace_bytes() : 0; }
int geosrad_set_overcast(geosrad_ctx *c, int flags)
{
    if (!c) return GEOSRAD_EINVAL;
    if (flags & ~(GEOSRAD_OVERCAST_IRRAD | GEOSRAD_OVERCAST_SORAD)) return c->fail(GEOSRAD_EINVAL, "unknown geosrad_set_overcast flag bits");
    if (auto *m = dynamic_cast<MultiCtx *>(c)) for (auto *k : m->kid) k->overcast = flags;
    c->overcast = flags;
    return GEOSRAD_OK;
}
int geosrad_get_overcast(const geosrad_ctx *c) { return c ? c->overcast : 0; }

int geosrad_set_tables_lw(geosrad_ctx *c, const void *blob, size_t n) { return c ? c->set_tables_lw(blob, n) : GEOSRAD_EINVAL; }

// a whole coefficient file; false with the reason in err
static bool read_file(const char *path, std::vector<char> &buf, std::string &err)
{
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) { err = std::string("cannot open table file: ") + (path ? path : "(null)"); return false; }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    buf.resize(n > 0 ? (size_t)n : 0);
    size_t got = n > 0 ? fread(buf.data(), 1, (size_t)n, f) : 0;
    fclose(f);
    if (got != buf.size()) { err = std::string("short read: ") + path; return false; }
    return true;
}
// geosrad_load_*: read the file, hand it to the setter
static int load_file(geosrad_ctx *c, const char *path, const std::function<int(const void *, size_t)> &set)
{
    if (!c) return GEOSRAD_EINVAL;
    std::vector<char> buf;
    std::string err;
    if (!read_file(path, buf, err)) return c->fail(GEOSRAD_ETABLE, err);
    return set(buf.data(), buf.size());
}
int geosrad_load_tables_lw(geosrad_ctx *c, const char *path) { return load_file(c, path, [&](const void *b, size_t n) { return c->set_tables_lw(b, n); }); }
int geosrad_set_inhomogeneity(geosrad_ctx *c, int ih, const void *blob, size_t n) { return c ? c->set_inhomogeneity(ih, blob, n) : GEOSRAD_EINVAL; }
int geosrad_load_inhomogeneity(geosrad_ctx *c, int ih, const char *path)
{
    if (c && ih == 0) return c->set_inhomogeneity(0, nullptr, 0);
    return load_file(c, path, [&](const void *b, size_t n) { return c->set_inhomogeneity(ih, b, n); });
}
int geosrad_set_corr_lengths(geosrad_ctx *c, const double *adl, const double *rdl) { return c ? c->set_corr(adl, rdl) : GEOSRAD_EINVAL; }

// Host-side copy of one named real array of a GRTB coefficient file (no context, no device): the Fortran shim keeps the xcw table
// on the host as well, because the reference's public zcw_lookup (cloud_condensate_inhomogeneity.F90:86-124) is a host function
// that the GridComps import for their RRTMGP branch.
int geosrad_read_table(const char *path, const char *name, int real_kind, void *dst, size_t count)
{
    if (!path || !name || !dst || (real_kind != 4 && real_kind != 8)) return GEOSRAD_EINVAL;
    std::vector<char> buf;
    std::string err;
    Blob B;
    if (!read_file(path, buf, err) || !B.parse(buf.data(), buf.size())) return GEOSRAD_ETABLE;
    auto it = B.e.find(name);
    if (it == B.e.end() || it->second.kind != real_kind || it->second.count != count) return GEOSRAD_ETABLE;
    memcpy(dst, it->second.data, count * (size_t)real_kind);
    return GEOSRAD_OK;
}


int geosrad_set_tables_sw(geosrad_ctx *c, const void *blob, size_t n) { return c ? c->set_tables_sw(blob, n) : GEOSRAD_EINVAL; }
int geosrad_load_tables_sw(geosrad_ctx *c, const char *path) { return load_file(c, path, [&](const void *b, size_t n) { return c->set_tables_sw(b, n); }); }

#define SW_PACK()                                                                                                              \
    const void *in[S_NIN] = {play, plev, tlay, h2ovmr, o3vmr, co2vmr, ch4vmr, o2vmr, cld, ciwp, clwp, rei, rel, zm, alat, tauaer,     \
                             ssaaer, asmaer, coszen, asdir, asdif, aldir, aldif};                                              \
    void *out[SO_NOUT] = {swuflx, swdflx, swuflxc, swdflxc, nirr, nirf, parr, parf, uvrr, uvrf, fswband, cotdtp, cotdhp, cotdmp,     \
                          cotdlp, cotntp, cotnhp, cotnmp, cotnlp, drband, dfband}

int geosrad_rrtmg_sw(geosrad_ctx *c, int rpart, int ncol, int nlay, double scon, double adjes, const void *coszen, int isolvar,
                     const void *play, const void *plev, const void *tlay, const void *h2ovmr, const void *o3vmr, const void *co2vmr,
                     const void *ch4vmr, const void *o2vmr, int iceflgsw, int liqflgsw, const void *cld, const void *ciwp,
                     const void *clwp, const void *rei, const void *rel, int dyofyr, const void *zm, const void *alat, int iaer,
                     const void *tauaer, const void *ssaaer, const void *asmaer, const void *asdir, const void *asdif,
                     const void *aldir, const void *aldif, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *swuflx,
                     void *swdflx, void *swuflxc, void *swdflxc, void *nirr, void *nirf, void *parr, void *parf, void *uvrr,
                     void *uvrf, void *fswband, void *cotdtp, void *cotdhp, void *cotdmp, void *cotdlp, void *cotntp, void *cotnhp,
                     void *cotnmp, void *cotnlp, int do_drfband, void *drband, void *dfband, const void *bndscl, const void *indsolvar,
                     const void *solcycfrac)
{
    if (!c) return GEOSRAD_EINVAL;
    (void)rpart;
    SW_PACK();
    return c->sw_host(ncol, nlay, scon, adjes, isolvar, in, iceflgsw, liqflgsw, dyofyr, iaer, cloudLM, cloudMH, normFlx, clearCounts, out,
                      do_drfband, bndscl, indsolvar, solcycfrac, nullptr, nullptr);
}

int geosrad_rrtmg_sw_dev(geosrad_ctx *c, void *stream, int rpart, int ncol, int nlay, double scon, double adjes, const void *coszen,
                         int isolvar, const void *play, const void *plev, const void *tlay, const void *h2ovmr, const void *o3vmr,
                         const void *co2vmr, const void *ch4vmr, const void *o2vmr, int iceflgsw, int liqflgsw, const void *cld,
                         const void *ciwp, const void *clwp, const void *rei, const void *rel, int dyofyr, const void *zm,
                         const void *alat, int iaer, const void *tauaer, const void *ssaaer, const void *asmaer, const void *asdir,
                         const void *asdif, const void *aldir, const void *aldif, int cloudLM, int cloudMH, int normFlx,
                         int32_t *clearCounts, void *swuflx, void *swdflx, void *swuflxc, void *swdflxc, void *nirr, void *nirf,
                         void *parr, void *parf, void *uvrr, void *uvrf, void *fswband, void *cotdtp, void *cotdhp, void *cotdmp,
                         void *cotdlp, void *cotntp, void *cotnhp, void *cotnmp, void *cotnlp, int do_drfband, void *drband,
                         void *dfband, const void *bndscl, const void *indsolvar,
                     const void *solcycfrac)
{
    if (!c || !clearCounts) return GEOSRAD_EINVAL;
    (void)rpart;
    SW_PACK();
    return c->sw_dev((hipStream_t)stream, ncol, nlay, scon, adjes, isolvar, in, iceflgsw, liqflgsw, dyofyr, iaer, cloudLM, cloudMH, normFlx,
                     clearCounts, out, do_drfband, bndscl, indsolvar, solcycfrac, nullptr, nullptr);
}

int geosrad_rrtmg_sw_radval(geosrad_ctx *c, int rpart, int ncol, int nlay, double scon, double adjes, const void *coszen, int isolvar,
                            const void *play, const void *plev, const void *tlay, const void *h2ovmr, const void *o3vmr,
                            const void *co2vmr, const void *ch4vmr, const void *o2vmr, int iceflgsw, int liqflgsw, const void *cld,
                            const void *ciwp, const void *clwp, const void *rei, const void *rel, int dyofyr, const void *zm,
                            const void *alat, int iaer, const void *tauaer, const void *ssaaer, const void *asmaer, const void *asdir,
                            const void *asdif, const void *aldir, const void *aldif, int cloudLM, int cloudMH, int normFlx,
                            int32_t *clearCounts, void *swuflx, void *swdflx, void *swuflxc, void *swdflxc, void *nirr, void *nirf,
                            void *parr, void *parf, void *uvrr, void *uvrf, void *fswband, void *cotdtp, void *cotdhp, void *cotdmp,
                            void *cotdlp, void *cotntp, void *cotnhp, void *cotnmp, void *cotnlp, int do_drfband, void *drband,
                            void *dfband, const void *bndscl, const void *indsolvar, const void *solcycfrac, void *radval)
{
    if (!c) return GEOSRAD_EINVAL;
    if (!radval) return c->fail(GEOSRAD_EINVAL, "geosrad_rrtmg_sw_radval: null radval array");
    (void)rpart;
    SW_PACK();
    return c->sw_host(ncol, nlay, scon, adjes, isolvar, in, iceflgsw, liqflgsw, dyofyr, iaer, cloudLM, cloudMH, normFlx, clearCounts, out,
                      do_drfband, bndscl, indsolvar, solcycfrac, nullptr, radval);
}

int geosrad_rrtmg_sw_radval_dev(geosrad_ctx *c, void *stream, int rpart, int ncol, int nlay, double scon, double adjes,
                                const void *coszen, int isolvar, const void *play, const void *plev, const void *tlay,
                                const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                                int iceflgsw, int liqflgsw, const void *cld, const void *ciwp, const void *clwp, const void *rei,
                                const void *rel, int dyofyr, const void *zm, const void *alat, int iaer, const void *tauaer,
                                const void *ssaaer, const void *asmaer, const void *asdir, const void *asdif, const void *aldir,
                                const void *aldif, int cloudLM, int cloudMH, int normFlx, int32_t *clearCounts, void *swuflx,
                                void *swdflx, void *swuflxc, void *swdflxc, void *nirr, void *nirf, void *parr, void *parf, void *uvrr,
                                void *uvrf, void *fswband, void *cotdtp, void *cotdhp, void *cotdmp, void *cotdlp, void *cotntp,
                                void *cotnhp, void *cotnmp, void *cotnlp, int do_drfband, void *drband, void *dfband,
                                const void *bndscl, const void *indsolvar, const void *solcycfrac, void *radval)
{
    if (!c || !clearCounts) return GEOSRAD_EINVAL;
    if (!radval) return c->fail(GEOSRAD_EINVAL, "geosrad_rrtmg_sw_radval_dev: null radval array");
    (void)rpart;
    SW_PACK();
    return c->sw_dev((hipStream_t)stream, ncol, nlay, scon, adjes, isolvar, in, iceflgsw, liqflgsw, dyofyr, iaer, cloudLM, cloudMH, normFlx,
                     clearCounts, out, do_drfband, bndscl, indsolvar, solcycfrac, nullptr, radval);
}

int geosrad_rrtmg_sw_taumol(geosrad_ctx *c, int ncol, int nlay, double scon, int isolvar, const void *play, const void *plev,
                            const void *tlay, const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr,
                            const void *o2vmr, const void *bndscl, const void *indsolvar, const void *solcycfrac, void *taug, void *taur,
                            void *ssi)
{
    if (!c || !taug || !taur || !ssi || ncol <= 0 || nlay <= 0) return GEOSRAD_EINVAL;
    // clear-sky run (zero cloud field, overhead sun, black surface); fluxes are discarded
    const size_t esz = (size_t)c->real_kind;
    const size_t cv = (size_t)ncol * (nlay + 1) * esz;
    std::vector<char> zero(cv, 0), tens((size_t)ncol * nlay * esz, 0), one((size_t)ncol * esz, 0), scratch(4 * cv + (size_t)ncol * esz * (6 + 14 + 8));
    for (size_t i = 0; i < (size_t)ncol * nlay; i++) { if (esz == 4) ((float *)tens.data())[i] = 10.f; else ((double *)tens.data())[i] = 10.; }
    for (size_t i = 0; i < (size_t)ncol; i++) { if (esz == 4) ((float *)one.data())[i] = 1.f; else ((double *)one.data())[i] = 1.; }
    std::vector<int32_t> cc((size_t)ncol * 4);
    const void *cld = zero.data(), *ciwp = zero.data(), *clwp = zero.data(), *rei = tens.data(), *rel = tens.data(), *zm = zero.data(),
               *alat = zero.data(), *tauaer = nullptr, *ssaaer = nullptr, *asmaer = nullptr, *coszen = one.data(), *asdir = zero.data(),
               *asdif = zero.data(), *aldir = zero.data(), *aldif = zero.data();
    char *s = scratch.data();
    const size_t cn = (size_t)ncol * esz;
    void *swuflx = s, *swdflx = s + cv, *swuflxc = s + 2 * cv, *swdflxc = s + 3 * cv;
    char *q = s + 4 * cv;
    void *nirr = q, *nirf = q + cn, *parr = q + 2 * cn, *parf = q + 3 * cn, *uvrr = q + 4 * cn, *uvrf = q + 5 * cn, *fswband = q + 6 * cn;
    q += 20 * cn;
    void *cotdtp = q, *cotdhp = q + cn, *cotdmp = q + 2 * cn, *cotdlp = q + 3 * cn, *cotntp = q + 4 * cn, *cotnhp = q + 5 * cn,
         *cotnmp = q + 6 * cn, *cotnlp = q + 7 * cn, *drband = nullptr, *dfband = nullptr;
    SW_PACK();
    void *dbg[6] = {taug, taur, ssi, nullptr, nullptr, nullptr};
    return c->sw_host(ncol, nlay, scon, 1.0, isolvar, in, 3, 1, 1, 0, 1, 2, 0, cc.data(), out, 0, bndscl, indsolvar, solcycfrac, dbg, nullptr);
}

int geosrad_rrtmg_sw_cldprmc(geosrad_ctx *c, int ncol, int nlay, const void *play, const void *plev, const void *tlay, const void *h2ovmr,
                             const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr, int iceflgsw, int liqflgsw,
                             const void *cld, const void *ciwp, const void *clwp, const void *rei, const void *rel, int dyofyr,
                             const void *zm, const void *alat, int cloudLM, int cloudMH, void *taucmc, void *ssacmc, void *asmcmc)
{
    if (!c || !taucmc || !ssacmc || !asmcmc || ncol <= 0 || nlay <= 0) return GEOSRAD_EINVAL;
    // the solver's own McICA + cldprmc_sw on these columns (overhead sun, black surface, no aerosol); fluxes are discarded
    const size_t esz = (size_t)c->real_kind;
    const size_t cv = (size_t)ncol * (nlay + 1) * esz, cn = (size_t)ncol * esz, cg = (size_t)ncol * nlay * NG_SW * esz;
    std::vector<char> zero(cn, 0), one(cn, 0), scratch(4 * cv + cn * (6 + 14 + 8) + 2 * cg + cn * NG_SW);
    for (size_t i = 0; i < (size_t)ncol; i++) { if (esz == 4) ((float *)one.data())[i] = 1.f; else ((double *)one.data())[i] = 1.; }
    std::vector<int32_t> cc((size_t)ncol * 4);
    const void *tauaer = nullptr, *ssaaer = nullptr, *asmaer = nullptr, *coszen = one.data(), *asdir = zero.data(), *asdif = zero.data(),
               *aldir = zero.data(), *aldif = zero.data();
    char *s = scratch.data();
    void *swuflx = s, *swdflx = s + cv, *swuflxc = s + 2 * cv, *swdflxc = s + 3 * cv;
    char *q = s + 4 * cv;
    void *nirr = q, *nirf = q + cn, *parr = q + 2 * cn, *parf = q + 3 * cn, *uvrr = q + 4 * cn, *uvrf = q + 5 * cn, *fswband = q + 6 * cn;
    q += 20 * cn;
    void *cotdtp = q, *cotdhp = q + cn, *cotdmp = q + 2 * cn, *cotdlp = q + 3 * cn, *cotntp = q + 4 * cn, *cotnhp = q + 5 * cn,
         *cotnmp = q + 6 * cn, *cotnlp = q + 7 * cn, *drband = nullptr, *dfband = nullptr;
    q += 8 * cn;
    SW_PACK();
    void *dbg[6] = {q, q + cg, q + 2 * cg, taucmc, ssacmc, asmcmc};
    return c->sw_host(ncol, nlay, 1361.0, 1.0, 0, in, iceflgsw, liqflgsw, dyofyr, 0, cloudLM, cloudMH, 0, cc.data(), out, 0, nullptr, nullptr, nullptr, dbg, nullptr);
}

int geosrad_set_tables_chou_lw(geosrad_ctx *c, const void *blob, size_t n) { return c ? c->set_tables_chou_lw(blob, n) : GEOSRAD_EINVAL; }
int geosrad_load_tables_chou_lw(geosrad_ctx *c, const char *path) { return load_file(c, path, [&](const void *b, size_t n) { return c->set_tables_chou_lw(b, n); }); }

#define CH_PACK()                                                                                                                   \
    const void *in[C_NIN] = {ple, ta, wa, oa, tb, n2o, ch4, cfc11, cfc12, cfc22, cwc, fcld, reff, fs, tg, eg, tv, ev, rv};             \
    void *aer[3] = {taua, ssaa, asya};                                                                                              \
    void *out[CO_NOUT] = {flxu, flcu, flau, flxau, flxd, flcd, flad, flxad, dfdts, sfcem, taudiag}

int geosrad_irrad(geosrad_ctx *c, int m, int np, const void *ple, const void *ta, const void *wa, const void *oa, const void *tb, double co2,
                  int trace, const void *n2o, const void *ch4, const void *cfc11, const void *cfc12, const void *cfc22, const void *cwc,
                  const void *fcld, int ict, int icb, const void *reff, int ns, const void *fs, const void *tg, const void *eg,
                  const void *tv, const void *ev, const void *rv, int na, int nb, void *taua, void *ssaa, void *asya, void *flxu,
                  void *flcu, void *flau, void *flxau, void *flxd, void *flcd, void *flad, void *flxad, void *dfdts, void *sfcem,
                  void *taudiag)
{
    if (!c) return GEOSRAD_EINVAL;
    CH_PACK();
    return c->irrad_host(m, np, in, co2, trace, ict, icb, ns, na, nb, aer, out);
}

int geosrad_irrad_dev(geosrad_ctx *c, void *stream, int m, int np, const void *ple, const void *ta, const void *wa, const void *oa,
                      const void *tb, double co2, int trace, const void *n2o, const void *ch4, const void *cfc11, const void *cfc12,
                      const void *cfc22, const void *cwc, const void *fcld, int ict, int icb, const void *reff, int ns, const void *fs,
                      const void *tg, const void *eg, const void *tv, const void *ev, const void *rv, int na, int nb, void *taua,
                      void *ssaa, void *asya, void *flxu, void *flcu, void *flau, void *flxau, void *flxd, void *flcd, void *flad,
                      void *flxad, void *dfdts, void *sfcem, void *taudiag)
{
    if (!c) return GEOSRAD_EINVAL;
    CH_PACK();
    return c->irrad_dev((hipStream_t)stream, m, np, in, co2, trace, ict, icb, ns, na, nb, aer, out);
}

int geosrad_set_tables_chou_sw(geosrad_ctx *c, const void *blob, size_t n) { return c ? c->set_tables_chou_sw(blob, n) : GEOSRAD_EINVAL; }
int geosrad_load_tables_chou_sw(geosrad_ctx *c, const char *path) { return load_file(c, path, [&](const void *b, size_t n) { return c->set_tables_chou_sw(b, n); }); }

#define SO_PACK()                                                                                                                    \
    const void *in[SI_NIN] = {cosz, pl, ta, wa, oa, cwc, fcld, reff, taua, ssaa, asya, rsuvbm, rsuvdf, rsirbm, rsirdf};                 \
    void *out[SOO_NOUT] = {flx, flc, fdiruv, fdifuv, fdirpar, fdifpar, fdirir, fdifir, flxu, flcu, flx_sfc_band, drband, dfband}

int geosrad_sorad(geosrad_ctx *c, int m, int np, int nb, const void *cosz, const void *pl, const void *ta, const void *wa, const void *oa,
                  double co2, const void *cwc, const void *fcld, int ict, int icb, const void *reff, const void *hk_uv, const void *hk_ir,
                  const void *taua, const void *ssaa, const void *asya, const void *rsuvbm, const void *rsuvdf, const void *rsirbm,
                  const void *rsirdf, void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar, void *fdifpar, void *fdirir,
                  void *fdifir, void *flxu, void *flcu, void *flx_sfc_band, int do_drfband, void *drband, void *dfband)
{
    if (!c) return GEOSRAD_EINVAL;
    SO_PACK();
    return c->sorad_host(m, np, nb, in, co2, ict, icb, hk_uv, hk_ir, out, do_drfband, nullptr);
}

int geosrad_sorad_na(geosrad_ctx *c, int m, int np, int nb, const void *cosz, const void *pl, const void *ta, const void *wa, const void *oa,
                     double co2, const void *cwc, const void *fcld, int ict, int icb, const void *reff, const void *hk_uv, const void *hk_ir,
                     const void *taua, const void *ssaa, const void *asya, const void *rsuvbm, const void *rsuvdf, const void *rsirbm,
                     const void *rsirdf, void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar, void *fdifpar, void *fdirir,
                     void *fdifir, void *flxu, void *flcu, void *flx_sfc_band, int do_drfband, void *drband, void *dfband,
                     void *const *na_out)
{
    if (!c) return GEOSRAD_EINVAL;
    SO_PACK();
    return c->sorad_host(m, np, nb, in, co2, ict, icb, hk_uv, hk_ir, out, do_drfband, na_out);
}

int geosrad_sorad_dev(geosrad_ctx *c, void *stream, int m, int np, int nb, const void *cosz, const void *pl, const void *ta, const void *wa,
                      const void *oa, double co2, const void *cwc, const void *fcld, int ict, int icb, const void *reff, const void *hk_uv,
                      const void *hk_ir, const void *taua, const void *ssaa, const void *asya, const void *rsuvbm, const void *rsuvdf,
                      const void *rsirbm, const void *rsirdf, void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar,
                      void *fdifpar, void *fdirir, void *fdifir, void *flxu, void *flcu, void *flx_sfc_band, int do_drfband,
                      void *drband, void *dfband)
{
    if (!c) return GEOSRAD_EINVAL;
    SO_PACK();
    return c->sorad_dev((hipStream_t)stream, m, np, nb, in, co2, ict, icb, hk_uv, hk_ir, out, do_drfband, nullptr);
}

int geosrad_sorad_na_dev(geosrad_ctx *c, void *stream, int m, int np, int nb, const void *cosz, const void *pl, const void *ta, const void *wa,
                         const void *oa, double co2, const void *cwc, const void *fcld, int ict, int icb, const void *reff, const void *hk_uv,
                         const void *hk_ir, const void *taua, const void *ssaa, const void *asya, const void *rsuvbm, const void *rsuvdf,
                         const void *rsirbm, const void *rsirdf, void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar,
                         void *fdifpar, void *fdirir, void *fdifir, void *flxu, void *flcu, void *flx_sfc_band, int do_drfband,
                         void *drband, void *dfband, void *const *na_out)
{
    if (!c) return GEOSRAD_EINVAL;
    SO_PACK();
    return c->sorad_dev((hipStream_t)stream, m, np, nb, in, co2, ict, icb, hk_uv, hk_ir, out, do_drfband, na_out);
}

#define LW_PACK_IN()                                                                                                     \
    const void *in[I_NIN] = {play, plev, tlay, tlev, tsfc, emis, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, \
                             cfc12vmr, cfc22vmr, ccl4vmr, cldf, ciwp, clwp, rei, rel, tauaer, zm, alat}

int geosrad_rrtmg_lw(geosrad_ctx *c, int ncol, int nlay, int psize, int dudTs, const void *play, const void *plev, const void *tlay,
                     const void *tlev, const void *tsfc, const void *emis, const void *h2ovmr, const void *o3vmr, const void *co2vmr,
                     const void *ch4vmr, const void *n2ovmr, const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr,
                     const void *cfc22vmr, const void *ccl4vmr, const void *cldf, const void *ciwp, const void *clwp, const void *rei,
                     const void *rel, int iceflglw, int liqflglw, const void *tauaer, const void *zm, const void *alat, int dyofyr,
                     int cloudLM, int cloudMH, int32_t *clearCounts, void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs,
                     void *duflxc_dTs, const int32_t *band_output, void *olrb, void *dolrb_dTs)
{
    if (!c) return GEOSRAD_EINVAL;
    (void)psize;
    LW_PACK_IN();
    void *out[O_NOUT] = {uflx, dflx, uflxc, dflxc, duflx_dTs, duflxc_dTs, olrb, dolrb_dTs};
    return c->lw_host(ncol, nlay, dudTs, in, iceflglw, liqflglw, dyofyr, cloudLM, cloudMH, clearCounts, out, band_output, nullptr, nullptr);
}

int geosrad_rrtmg_lw_dev(geosrad_ctx *c, void *stream, int ncol, int nlay, int psize, int dudTs, const void *play, const void *plev,
                         const void *tlay, const void *tlev, const void *tsfc, const void *emis, const void *h2ovmr, const void *o3vmr,
                         const void *co2vmr, const void *ch4vmr, const void *n2ovmr, const void *o2vmr, const void *cfc11vmr,
                         const void *cfc12vmr, const void *cfc22vmr, const void *ccl4vmr, const void *cldf, const void *ciwp,
                         const void *clwp, const void *rei, const void *rel, int iceflglw, int liqflglw, const void *tauaer, const void *zm,
                         const void *alat, int dyofyr, int cloudLM, int cloudMH, int32_t *clearCounts, void *uflx, void *dflx, void *uflxc,
                         void *dflxc, void *duflx_dTs, void *duflxc_dTs, const int32_t *band_output, void *olrb, void *dolrb_dTs)
{
    if (!c || !clearCounts) return GEOSRAD_EINVAL;
    (void)psize;
    LW_PACK_IN();
    void *out[O_NOUT] = {uflx, dflx, uflxc, dflxc, duflx_dTs, duflxc_dTs, olrb, dolrb_dTs};
    return c->lw_dev((hipStream_t)stream, ncol, nlay, dudTs, in, iceflglw, liqflglw, dyofyr, cloudLM, cloudMH, clearCounts, out,
                     band_output, nullptr, nullptr, nullptr);
}

int geosrad_rrtmg_lw_rats_dev(geosrad_ctx *c, void *stream, int ncol, int nlay, int psize, int dudTs, const void *play, const void *plev,
                              const void *tlay, const void *tlev, const void *tsfc, const void *emis, const void *h2ovmr, const void *o3vmr,
                              const void *co2vmr, const void *ch4vmr, const void *n2ovmr, const void *o2vmr, const void *cfc11vmr,
                              const void *cfc12vmr, const void *cfc22vmr, const void *ccl4vmr, const void *cldf, const void *ciwp,
                              const void *clwp, const void *rei, const void *rel, int iceflglw, int liqflglw, const void *tauaer,
                              const void *zm, const void *alat, int dyofyr, int cloudLM, int cloudMH, int32_t *clearCounts, void *uflx,
                              void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs, const int32_t *band_output,
                              void *olrb, void *dolrb_dTs, int nrats, const int32_t *rat_gas, void *uflx_rat, void *dflx_rat,
                              void *duflx_dTs_rat)
{
    if (!c || !clearCounts) return GEOSRAD_EINVAL;
    if (nrats < 0 || nrats > GEOSRAD_RAT_NGAS || (nrats > 0 && !rat_gas)) return c->fail(GEOSRAD_EINVAL, "bad RATS arguments");
    (void)psize;
    LW_PACK_IN();
    void *out[O_NOUT] = {uflx, dflx, uflxc, dflxc, duflx_dTs, duflxc_dTs, olrb, dolrb_dTs};
    geosrad_ctx::LwRats RT{};
    RT.n = nrats; RT.uflx = uflx_rat; RT.dflx = dflx_rat; RT.duflx_dTs = duflx_dTs_rat;
    for (int r = 0; r < nrats; r++) RT.gas[r] = rat_gas[r];
    return c->lw_dev((hipStream_t)stream, ncol, nlay, dudTs, in, iceflglw, liqflglw, dyofyr, cloudLM, cloudMH, clearCounts, out,
                     band_output, nullptr, nullptr, nrats > 0 ? &RT : nullptr);
}

// the `out` table of the aerosol-free entry points: all four flux arrays, and with dudTs both derivatives (ignored without)
#define LW_PACK_OUT_NA()                                                                                                             \
    if (!uflx_na || !dflx_na || !uflxc_na || !dflxc_na || (dudTs && (!duflx_dTs_na || !duflxc_dTs_na)))                              \
        return c->fail(GEOSRAD_EINVAL, "aerosol-free fluxes: uflx_na .. dflxc_na (and the two derivatives with dudTs) must not be null"); \
    void *out[O_NOUT] = {uflx, dflx, uflxc, dflxc, duflx_dTs, duflxc_dTs, olrb, dolrb_dTs, uflx_na, dflx_na, uflxc_na, dflxc_na,    \
                         dudTs ? duflx_dTs_na : nullptr, dudTs ? duflxc_dTs_na : nullptr}

int geosrad_rrtmg_lw_na(geosrad_ctx *c, int ncol, int nlay, int psize, int dudTs, const void *play, const void *plev, const void *tlay,
                        const void *tlev, const void *tsfc, const void *emis, const void *h2ovmr, const void *o3vmr, const void *co2vmr,
                        const void *ch4vmr, const void *n2ovmr, const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr,
                        const void *cfc22vmr, const void *ccl4vmr, const void *cldf, const void *ciwp, const void *clwp, const void *rei,
                        const void *rel, int iceflglw, int liqflglw, const void *tauaer, const void *zm, const void *alat, int dyofyr,
                        int cloudLM, int cloudMH, int32_t *clearCounts, void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs,
                        void *duflxc_dTs, const int32_t *band_output, void *olrb, void *dolrb_dTs, void *uflx_na, void *dflx_na,
                        void *uflxc_na, void *dflxc_na, void *duflx_dTs_na, void *duflxc_dTs_na)
{
    if (!c) return GEOSRAD_EINVAL;
    (void)psize;
    LW_PACK_IN();
    LW_PACK_OUT_NA();
    return c->lw_host(ncol, nlay, dudTs, in, iceflglw, liqflglw, dyofyr, cloudLM, cloudMH, clearCounts, out, band_output, nullptr, nullptr);
}

int geosrad_rrtmg_lw_na_dev(geosrad_ctx *c, void *stream, int ncol, int nlay, int psize, int dudTs, const void *play, const void *plev,
                            const void *tlay, const void *tlev, const void *tsfc, const void *emis, const void *h2ovmr, const void *o3vmr,
                            const void *co2vmr, const void *ch4vmr, const void *n2ovmr, const void *o2vmr, const void *cfc11vmr,
                            const void *cfc12vmr, const void *cfc22vmr, const void *ccl4vmr, const void *cldf, const void *ciwp,
                            const void *clwp, const void *rei, const void *rel, int iceflglw, int liqflglw, const void *tauaer,
                            const void *zm, const void *alat, int dyofyr, int cloudLM, int cloudMH, int32_t *clearCounts, void *uflx,
                            void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs, const int32_t *band_output,
                            void *olrb, void *dolrb_dTs, int nrats, const int32_t *rat_gas, void *uflx_rat, void *dflx_rat,
                            void *duflx_dTs_rat, void *uflx_na, void *dflx_na, void *uflxc_na, void *dflxc_na, void *duflx_dTs_na,
                            void *duflxc_dTs_na)
{
    if (!c || !clearCounts) return GEOSRAD_EINVAL;
    if (nrats < 0 || nrats > GEOSRAD_RAT_NGAS || (nrats > 0 && !rat_gas)) return c->fail(GEOSRAD_EINVAL, "bad RATS arguments");
    (void)psize;
    LW_PACK_IN();
    LW_PACK_OUT_NA();
    geosrad_ctx::LwRats RT{};
    RT.n = nrats; RT.uflx = uflx_rat; RT.dflx = dflx_rat; RT.duflx_dTs = duflx_dTs_rat;
    for (int r = 0; r < nrats; r++) RT.gas[r] = rat_gas[r];
    return c->lw_dev((hipStream_t)stream, ncol, nlay, dudTs, in, iceflglw, liqflglw, dyofyr, cloudLM, cloudMH, clearCounts, out,
                     band_output, nullptr, nullptr, nrats > 0 ? &RT : nullptr);
}
#undef LW_PACK_OUT_NA

// The drivers with a call record (gridcomp_kernels.hpp): an entry point fills it, its family's one statement passes it on (a tile's through swd_merge).
static int lwd_call(geosrad_ctx *c, void *st, const LwdCall &C) { return !c || !C.in || !C.consts || !C.out ? GEOSRAD_EINVAL : c->lw_driver_dev((hipStream_t)st, C); }
#define LWD_COMMON ncol, lm, nb_aer, in, consts, iceflglw, liqflglw, doy, lcldlm, lcldmh, band_output, out
int geosrad_lw_driver_rrtmg_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nb_aer, const void *const *in, const double *consts,
                                int iceflglw, int liqflglw, int doy, int lcldlm, int lcldmh, const int32_t *band_output, void *const *out)
{
    return lwd_call(c, stream, {LWD_COMMON, 0, nullptr, nullptr});
}

int geosrad_lw_driver_rrtmg_rats_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nb_aer, const void *const *in, const double *consts,
                                     int iceflglw, int liqflglw, int doy, int lcldlm, int lcldmh, const int32_t *band_output,
                                     void *const *out, int nrats, const int32_t *rat_gas, void *const *rat_out)
{
    return lwd_call(c, stream, {LWD_COMMON, nrats, rat_gas, rat_out});
}

int geosrad_lw_driver_rrtmg_na_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nb_aer, const void *const *in, const double *consts,
                                   int iceflglw, int liqflglw, int doy, int lcldlm, int lcldmh, const int32_t *band_output,
                                   void *const *out, int nrats, const int32_t *rat_gas, void *const *rat_out, void *const *na_out)
{
    return lwd_call(c, stream, {LWD_COMMON, nrats, rat_gas, rat_out, na_out});
}
#undef LWD_COMMON
static int swd_call(geosrad_ctx *c, void *stream, SwdCall C)
{
    if (!c || !C.in || !C.consts || !C.out) return GEOSRAD_EINVAL;
    if (C.lit) swd_merge(C);
    return c->sw_driver_dev((hipStream_t)stream, C);
}
#define SWD_COMMON lm, nb_aer, in, consts, iceflgsw, liqflgsw, sc, dist, isolvar, dyofyr, include_aerosols, lcldlm, lcldmh, normflx, bndsolvar, indsolvar, out
int geosrad_sw_driver_rrtmg_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nb_aer, const void *const *in, const double *consts,
                                int iceflgsw, int liqflgsw, double sc, double dist, int isolvar, int dyofyr, int include_aerosols,
                                int lcldlm, int lcldmh, int normflx, const void *bndsolvar, const void *indsolvar, void *const *out)
{
    return swd_call(c, stream, {ncol, SWD_COMMON});
}

int geosrad_sw_driver_rrtmg_lit_dev(geosrad_ctx *c, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos, int lm,
                                    int nb_aer, const void *const *in, const double *consts, int iceflgsw, int liqflgsw, double sc, double dist,
                                    int isolvar, int dyofyr, int include_aerosols, int lcldlm, int lcldmh, int normflx, const void *bndsolvar,
                                    const void *indsolvar, const double *dark, uint64_t keep_mask, void *const *out)
{
    const LitTile lit{ncol, lit_index, lit_pos, dark, keep_mask};
    return swd_call(c, stream, {nlit, SWD_COMMON, &lit});
}

int geosrad_sw_driver_rrtmg_obio_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nb_aer, const void *const *in, const double *consts,
                                     int iceflgsw, int liqflgsw, double sc, double dist, int isolvar, int dyofyr, int include_aerosols,
                                     int lcldlm, int lcldmh, int normflx, const void *bndsolvar, const void *indsolvar, void *const *out,
                                     void *drband, void *dfband)
{
    return swd_call(c, stream, {ncol, SWD_COMMON, nullptr, drband, dfband});
}

int geosrad_sw_driver_rrtmg_obio_lit_dev(geosrad_ctx *c, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos,
                                         int lm, int nb_aer, const void *const *in, const double *consts, int iceflgsw, int liqflgsw,
                                         double sc, double dist, int isolvar, int dyofyr, int include_aerosols, int lcldlm, int lcldmh,
                                         int normflx, const void *bndsolvar, const void *indsolvar, const double *dark, uint64_t keep_mask,
                                         void *const *out, const double *dark_obio, int keep_obio, void *drband, void *dfband)
{
    const LitTile lit{ncol, lit_index, lit_pos, dark, keep_mask};
    return swd_call(c, stream, {nlit, SWD_COMMON, &lit, drband, dfband, dark_obio, keep_obio});
}
#undef SWD_COMMON
static int swc_call(geosrad_ctx *c, void *st, const SwcCall &C) { return !c || !C.in || !C.out ? GEOSRAD_EINVAL : c->sw_driver_chou_dev((hipStream_t)st, C); }

int geosrad_sw_driver_chou_dev(geosrad_ctx *c, void *stream, int ncol, int lm, const void *const *in, const double *consts, int lcldmh,
                               int lcldlm, const void *hk_uv, const void *hk_ir, int do_drfband, void *const *out)
{
    return swc_call(c, stream, {ncol, lm, in, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband, out, nullptr});
}

int geosrad_sw_driver_chou_lit_dev(geosrad_ctx *c, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos, int lm,
                                   const void *const *in, const double *consts, int lcldmh, int lcldlm, const void *hk_uv, const void *hk_ir,
                                   int do_drfband, const double *dark, uint64_t keep_mask, void *const *out)
{
    const LitTile lit{ncol, lit_index, lit_pos, dark, keep_mask};
    return swc_call(c, stream, {nlit, lm, in, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband, out, &lit});
}

int geosrad_sw_driver_chou_na_dev(geosrad_ctx *c, void *stream, int ncol, int lm, const void *const *in, const double *consts, int lcldmh,
                                  int lcldlm, const void *hk_uv, const void *hk_ir, int do_drfband, void *const *out, void *const *na_out)
{
    return swc_call(c, stream, {ncol, lm, in, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband, out, nullptr, na_out});
}

int geosrad_sw_driver_chou_na_lit_dev(geosrad_ctx *c, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos, int lm,
                                      const void *const *in, const double *consts, int lcldmh, int lcldlm, const void *hk_uv,
                                      const void *hk_ir, int do_drfband, const double *dark, uint64_t keep_mask, void *const *out,
                                      const double *dark_na, int keep_na, void *const *na_out)
{
    const LitTile lit{ncol, lit_index, lit_pos, dark, keep_mask};
    return swc_call(c, stream, {nlit, lm, in, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband, out, &lit, na_out, dark_na, keep_na});
}

int geosrad_lw_driver_chou_dev(geosrad_ctx *c, void *stream, int ncol, int lm, const void *const *in, const double *consts, int trace,
                               int lcldmh, int lcldlm, int binary_clouds, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->lw_driver_chou_dev((hipStream_t)stream, ncol, lm, in, consts, trace, lcldmh, lcldlm, binary_clouds, out);
}

int geosrad_lw_chou_post_dev(geosrad_ctx *c, void *stream, int ncol, int lm, const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->lw_chou_post_dev((hipStream_t)stream, ncol, lm, in, out);
}

int geosrad_lw_update_flx_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int rrtmg, int lev_mid_high, int lev_low_mid, double undef,
                              const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->lw_update_flx_dev((hipStream_t)stream, ncol, lm, rrtmg, lev_mid_high, lev_low_mid, undef, in, out);
}

int geosrad_lw_update_rats_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nrats, const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->lw_update_rats_dev((hipStream_t)stream, ncol, lm, nrats, in, out);
}

int geosrad_lw_update_bands_dev(geosrad_ctx *c, void *stream, int ncol, const int32_t *band_output, const double *wavenum1,
                                const double *wavenum2, double undef, const void *tsinst, const void *ts_int, const void *olrb_int,
                                const void *dolrb_int, void *olrb_exp, void *tbrb_exp)
{
    if (!c) return GEOSRAD_EINVAL;
    return c->lw_update_bands_dev((hipStream_t)stream, ncol, band_output, wavenum1, wavenum2, undef, tsinst, ts_int, olrb_int, dolrb_int,
                                  olrb_exp, tbrb_exp);
}

int geosrad_sw_update_export_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int nbands, const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->sw_update_export_dev((hipStream_t)stream, ncol, lm, nbands, in, out);
}

int geosrad_obio_weights(int scheme, int real_kind, int nbands, const double *wvn1, const double *wvn2, const int32_t *order,
                         double *weights, int32_t *npairs)
{
    auto run = [&](auto zero) -> const char * {
        using T = decltype(zero);
        T s1[OBIO_MAXBANDS], s2[OBIO_MAXBANDS];
        int ord[OBIO_MAXBANDS], np = 0;
        if (const char *e = obio_solar_bands<T>(scheme, nbands, wvn1, wvn2, order, s1, s2, ord)) return e;
        if (weights) for (int k = 0; k < NB_OBIO * nbands; k++) weights[k] = 0.0;
        const char *e = obio_walk<T>(nbands, s1, s2, ord, [&](int, int ib, int kb, T sfrac) {
            if (weights) weights[(size_t)(ib - 1) * NB_OBIO + (kb - 1)] = (double)sfrac;
            np++;
        });
        if (!e && npairs) *npairs = np;
        return e;
    };
    const char *e = real_kind == 4 ? run(0.0f) : real_kind == 8 ? run(0.0) : "real_kind must be 4 or 8";
    if (!e) return GEOSRAD_OK;
    g_ctxless_error = e;
    return GEOSRAD_EINVAL;
}

int geosrad_sw_update_obio_dev(geosrad_ctx *c, void *stream, int ncol, int scheme, int nbands, const double *wvn1, const double *wvn2,
                               const int32_t *order, const void *slr, const void *drbandn, const void *dfbandn, void *drobio, void *dfobio)
{
    if (!c) return GEOSRAD_EINVAL;
    return c->sw_update_obio_dev((hipStream_t)stream, ncol, scheme, nbands, wvn1, wvn2, order, slr, drbandn, dfbandn, drobio, dfobio);
}

int geosrad_sw_update_surface_dev(geosrad_ctx *c, void *stream, int ncol, int lm, double undef, const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->sw_update_surface_dev((hipStream_t)stream, ncol, lm, undef, in, out);
}

int geosrad_sw_update_clouds_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int lcldmh, int lcldlm, double taucrit,
                                 const double *consts, const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->sw_update_clouds_dev((hipStream_t)stream, ncol, lm, lcldmh, lcldlm, taucrit, consts, in, out);
}

int geosrad_sw_update_cldhb_dev(geosrad_ctx *c, void *stream, int ncol, int lm, int lcldmh, int lcldlm, int doy, const double *consts,
                                const void *const *in, void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->sw_update_cldhb_dev((hipStream_t)stream, ncol, lm, lcldmh, lcldlm, doy, consts, in, out);
}

int geosrad_rad_tendencies_dev(geosrad_ctx *c, void *stream, int ncol, int lm, double grav, double cp, const void *const *in,
                               void *const *out)
{
    if (!c || !in || !out) return GEOSRAD_EINVAL;
    return c->rad_tendencies_dev((hipStream_t)stream, ncol, lm, grav, cp, in, out);
}

int geosrad_lit_index_dev(geosrad_ctx *c, void *stream, int ncol, const void *zth, int32_t *lit_index, int32_t *lit_pos, int32_t *nlit_dev,
                          int *nlit_host)
{
    return c ? c->lit_index_dev((hipStream_t)stream, ncol, zth, lit_index, lit_pos, nlit_dev, nlit_host) : GEOSRAD_EINVAL;
}
int geosrad_lit_pack_dev(geosrad_ctx *c, void *stream, int pdim, int udim, int nlev, const int32_t *lit_index, const int32_t *nlit_dev,
                         const void *unpacked, void *packed)
{
    return c ? c->lit_pack_dev((hipStream_t)stream, pdim, udim, nlev, lit_index, nlit_dev, unpacked, packed) : GEOSRAD_EINVAL;
}
int geosrad_lit_unpack_dev(geosrad_ctx *c, void *stream, int pdim, int udim, int nlev, const int32_t *lit_pos, const void *packed,
                           void *unpacked, int use_default, double dflt)
{
    return c ? c->lit_unpack_dev((hipStream_t)stream, pdim, udim, nlev, lit_pos, packed, unpacked, use_default, dflt) : GEOSRAD_EINVAL;
}

// ---- include/geosrad_gettau.h ------------------------------------------------------------------------------------------------
static int gt_call(geosrad_ctx *c, void *stream, bool dev, const geosrad_ctx::GtCall &C)
{
    if (!c) return GEOSRAD_EINVAL;
    return dev ? c->gettau_dev((hipStream_t)stream, C) : c->gettau_host(C);
}
int geosrad_getvistau(geosrad_ctx *c, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld, const void *reff,
                      const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff, void *asycl)
{
    return gt_call(c, nullptr, false, {0, 0, ncol, nlevs, ict, icb, grav, cosz, dp, fcld, reff, hydromets, {taubeam, taudiff, asycl, nullptr}});
}
int geosrad_getvistau_dev(geosrad_ctx *c, void *stream, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld,
                          const void *reff, const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff, void *asycl)
{
    return gt_call(c, stream, true, {0, 0, ncol, nlevs, ict, icb, grav, cosz, dp, fcld, reff, hydromets, {taubeam, taudiff, asycl, nullptr}});
}
int geosrad_getnirtau(geosrad_ctx *c, int ib, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld, const void *reff,
                      const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff, void *asycl, void *ssacl)
{
    return gt_call(c, nullptr, false, {1, ib, ncol, nlevs, ict, icb, grav, cosz, dp, fcld, reff, hydromets, {taubeam, taudiff, asycl, ssacl}});
}
int geosrad_getnirtau_dev(geosrad_ctx *c, void *stream, int ib, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld,
                          const void *reff, const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff, void *asycl,
                          void *ssacl)
{
    return gt_call(c, stream, true, {1, ib, ncol, nlevs, ict, icb, grav, cosz, dp, fcld, reff, hydromets, {taubeam, taudiff, asycl, ssacl}});
}
int geosrad_getirtau(geosrad_ctx *c, int ib, int ncol, int nlevs, const void *dp, const void *fcld, const void *reff, const void *hydromets,
                     double grav, void *taudiag, void *tcldlyr, void *enn)
{
    return gt_call(c, nullptr, false, {2, ib, ncol, nlevs, 0, 0, grav, nullptr, dp, fcld, reff, hydromets, {taudiag, tcldlyr, enn, nullptr}});
}
int geosrad_getirtau_dev(geosrad_ctx *c, void *stream, int ib, int ncol, int nlevs, const void *dp, const void *fcld, const void *reff,
                         const void *hydromets, double grav, void *taudiag, void *tcldlyr, void *enn)
{
    return gt_call(c, stream, true, {2, ib, ncol, nlevs, 0, 0, grav, nullptr, dp, fcld, reff, hydromets, {taudiag, tcldlyr, enn, nullptr}});
}
int geosrad_lw_cloud_diag_dev(geosrad_ctx *c, void *stream, int ncol, int lm, double grav, double undef, double taucrit, const void *ple,
                              const void *t, const void *fcld, const void *qi, const void *ql, const void *qr, const void *qs, const void *ri,
                              const void *rl, const void *rr, const void *rs, void *tauir, void *cldtmp, void *cldprs)
{
    if (!c) return GEOSRAD_EINVAL;
    const void *in[11] = {ple, t, fcld, qi, ql, qr, qs, ri, rl, rr, rs};
    void *out[3] = {tauir, cldtmp, cldprs};
    return c->lw_cloud_diag_dev((hipStream_t)stream, ncol, lm, grav, undef, taucrit, in, out);
}

// ---- include/geosrad_satsim.h ------------------------------------------------------------------------------------------------
int geosrad_scops(geosrad_ctx *c, int npoints, int nlev, int ncol, int32_t *seed, const void *cc, const void *conv, int overlap, void *frac_out)
{
    return c ? c->scops_host({npoints, nlev, ncol, overlap, seed, cc, conv, frac_out}) : GEOSRAD_EINVAL;
}
int geosrad_scops_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, int ncol, int32_t *seed, const void *cc, const void *conv, int overlap,
                      void *frac_out_u8)
{
    return c ? c->scops_dev((hipStream_t)stream, {npoints, nlev, ncol, overlap, seed, cc, conv, frac_out_u8}) : GEOSRAD_EINVAL;
}
#define IC_CALL(frac) geosrad_ctx::IcarusCall C{npoints, nlev, ncol, top_height, top_height_direction, overlap, emsfc_lw, sunlit,          \
        {pfull, phalf, qv, cc, conv, dtau_s, dtau_c, skt, at, dem_s, dem_c}, frac,                                                       \
        {fq_isccp, totalcldarea, meanptop, meantaucld, meanalbedocld, meantb, meantbclr, boxtau, boxptop}}
int geosrad_icarus(geosrad_ctx *c, int npoints, const int32_t *sunlit, int nlev, int ncol, const void *pfull, const void *phalf, const void *qv,
                   const void *cc, const void *conv, const void *dtau_s, const void *dtau_c, int top_height, int top_height_direction, int overlap,
                   const void *frac_out, const void *skt, double emsfc_lw, const void *at, const void *dem_s, const void *dem_c, void *fq_isccp,
                   void *totalcldarea, void *meanptop, void *meantaucld, void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau,
                   void *boxptop)
{
    if (!c) return GEOSRAD_EINVAL;
    IC_CALL(frac_out);
    return c->icarus_host(C);
}
int geosrad_icarus_dev(geosrad_ctx *c, void *stream, int npoints, const int32_t *sunlit, int nlev, int ncol, const void *pfull, const void *phalf,
                       const void *qv, const void *cc, const void *conv, const void *dtau_s, const void *dtau_c, int top_height,
                       int top_height_direction, int overlap, const void *frac_out_u8, const void *skt, double emsfc_lw, const void *at,
                       const void *dem_s, const void *dem_c, void *fq_isccp, void *totalcldarea, void *meanptop, void *meantaucld,
                       void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop)
{
    if (!c) return GEOSRAD_EINVAL;
    IC_CALL(frac_out_u8);
    return c->icarus_dev((hipStream_t)stream, C);
}
int geosrad_cosp_seeds_dev(geosrad_ctx *c, void *stream, int npoints, const void *psfc, int32_t *seed)
{
    return c ? c->cosp_seeds_dev((hipStream_t)stream, npoints, psfc, seed) : GEOSRAD_EINVAL;
}
int geosrad_isccp_dev(geosrad_ctx *c, void *stream, int npoints, int lm, int ncol, const void *t, const void *qv, const void *fcld, const void *cca,
                      const void *ple, const void *plo, const void *dtau_s, const void *emiss, const void *dtau_c, const void *dem_c, const void *ts,
                      const int32_t *sunlit, int32_t *seed, int overlap, int top_height, int top_height_direction, double emsfc_lw, void *fq_isccp,
                      void *totalcldarea, void *meanptop, void *meantaucld, void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau,
                      void *boxptop, void *sgfcld)
{
    if (!c) return GEOSRAD_EINVAL;
    const int nlev = lm;
    const void *pfull = plo, *phalf = ple, *cc = fcld, *conv = cca, *skt = ts, *at = t, *dem_s = emiss;
    IC_CALL(nullptr);
    C.cosp = true; C.seed = seed; C.sgfcld = sgfcld;
    return c->icarus_dev((hipStream_t)stream, C);
}
#undef IC_CALL

// ---- include/geosrad_misr_modis.h --------------------------------------------------------------------------------------------
int geosrad_misr(geosrad_ctx *c, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *zfull, const void *at, const void *dtau_s,
                 const void *dtau_c, const void *frac_out, double missing_value, void *fq_MISR_TAU_v_CTH, void *dist_model_layertops,
                 void *MISR_mean_ztop, void *MISR_cldarea)
{
    if (!c) return GEOSRAD_EINVAL;
    return c->misr_host({npoints, nlev, ncol, missing_value, sunlit, {zfull, at, dtau_s, dtau_c}, frac_out,
                         {fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea}});
}
#define MD_CALL(frac) geosrad_ctx::ModisCall C{npoints, nlev, ncol, sunlit,                                                              \
        {t, p, ph, dtau_s, dtau_c, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, isccp_boxtau,     \
         isccp_boxptop}, frac, {modis_mean, modis_hist, phase, ctp, tau, size}}
int geosrad_modis(geosrad_ctx *c, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *t, const void *p, const void *ph,
                  const void *dtau_s, const void *dtau_c, const void *frac_out, const void *mr_lsliq, const void *mr_lsice, const void *mr_cvliq,
                  const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq, const void *reff_cvice,
                  const void *isccp_boxtau, const void *isccp_boxptop, void *modis_mean, void *modis_hist, int32_t *phase, void *ctp, void *tau,
                  void *size)
{
    if (!c) return GEOSRAD_EINVAL;
    MD_CALL(frac_out);
    return c->modis_host(C);
}
int geosrad_modis_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *t, const void *p,
                      const void *ph, const void *dtau_s, const void *dtau_c, const void *frac_out_u8, const void *mr_lsliq, const void *mr_lsice,
                      const void *mr_cvliq, const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq,
                      const void *reff_cvice, const void *isccp_boxtau, const void *isccp_boxptop, void *modis_mean, void *modis_hist,
                      int32_t *phase, void *ctp, void *tau, void *size)
{
    if (!c) return GEOSRAD_EINVAL;
    MD_CALL(frac_out_u8);
    return c->modis_dev((hipStream_t)stream, C);
}
#undef MD_CALL
int geosrad_cosp_dev(geosrad_ctx *c, void *stream, int npoints, int lm, int ncol, const void *t, const void *qv, const void *fcld, const void *cca,
                     const void *ple, const void *plo, const void *dtau_s, const void *emiss, const void *dtau_c, const void *dem_c, const void *ts,
                     const int32_t *sunlit, int32_t *seed, int overlap, int top_height, int top_height_direction, double emsfc_lw, void *fq_isccp,
                     void *totalcldarea, void *meanptop, void *meantaucld, void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau,
                     void *boxptop, void *sgfcld, const void *zle, const void *qltot, const void *qitot, const void *rdfl, const void *rdfi,
                     void *fq_MISR_TAU_v_CTH, void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea, void *modis_mean,
                     void *modis_hist)
{
    if (!c) return GEOSRAD_EINVAL;
    geosrad_ctx::CospCall C{{npoints, lm, ncol, top_height, top_height_direction, overlap, emsfc_lw, sunlit,
                             {plo, ple, qv, fcld, cca, dtau_s, dtau_c, ts, t, emiss, dem_c}, nullptr,
                             {fq_isccp, totalcldarea, meanptop, meantaucld, meanalbedocld, meantb, meantbclr, boxtau, boxptop}},
                            zle, qltot, qitot, rdfl, rdfi, {fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea},
                            {modis_mean, modis_hist}};
    C.ic.cosp = true; C.ic.seed = seed; C.ic.sgfcld = sgfcld;
    return c->cosp_dev((hipStream_t)stream, C);
}
// ---- include/geosrad_lidar.h -------------------------------------------------------------------------------------------------
#define LD_CALL(frac) geosrad_ctx::LidarCall C{npoints, nlev, ncol, ice_type,                                                             \
        {p, t, presf, pplay, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, land}, frac,            \
        {lidarcld, cldlayer, cfad_sr, parasolrefl, pmol, beta_tot, tau_tot, refl}}
int geosrad_lidar(geosrad_ctx *c, int npoints, int nlev, int ncol, int ice_type, const void *p, const void *t, const void *presf,
                  const void *pplay, const void *frac_out, const void *mr_lsliq, const void *mr_lsice, const void *mr_cvliq, const void *mr_cvice,
                  const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq, const void *reff_cvice, const void *land,
                  void *lidarcld, void *cldlayer, void *cfad_sr, void *parasolrefl, void *pmol, void *beta_tot, void *tau_tot, void *refl)
{
    if (!c) return GEOSRAD_EINVAL;
    LD_CALL(frac_out);
    return c->lidar_host(C);
}
int geosrad_lidar_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, int ncol, int ice_type, const void *p, const void *t,
                      const void *presf, const void *pplay, const void *frac_out_u8, const void *mr_lsliq, const void *mr_lsice,
                      const void *mr_cvliq, const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq,
                      const void *reff_cvice, const void *land, void *lidarcld, void *cldlayer, void *cfad_sr, void *parasolrefl, void *pmol,
                      void *beta_tot, void *tau_tot, void *refl)
{
    if (!c) return GEOSRAD_EINVAL;
    LD_CALL(frac_out_u8);
    return c->lidar_dev((hipStream_t)stream, C);
}
#undef LD_CALL
int geosrad_cosp_lidar_dev(geosrad_ctx *c, void *stream, int npoints, int lm, int ncol, const void *t, const void *qv, const void *fcld,
                           const void *cca, const void *ple, const void *plo, const void *dtau_s, const void *emiss, const void *dtau_c,
                           const void *dem_c, const void *ts, const int32_t *sunlit, int32_t *seed, int overlap, int top_height,
                           int top_height_direction, double emsfc_lw, void *fq_isccp, void *totalcldarea, void *meanptop, void *meantaucld,
                           void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop, void *sgfcld, const void *zle,
                           const void *qltot, const void *qitot, const void *rdfl, const void *rdfi, void *fq_MISR_TAU_v_CTH,
                           void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea, void *modis_mean, void *modis_hist,
                           const void *frocean, int ice_type, void *clcalipso, void *cldlayer, void *cfad_sr, void *parasolrefl,
                           void *lidarpmol)
{
    if (!c) return GEOSRAD_EINVAL;
    geosrad_ctx::CospLidarCall C{{{npoints, lm, ncol, top_height, top_height_direction, overlap, emsfc_lw, sunlit,
                                  {plo, ple, qv, fcld, cca, dtau_s, dtau_c, ts, t, emiss, dem_c}, nullptr,
                                  {fq_isccp, totalcldarea, meanptop, meantaucld, meanalbedocld, meantb, meantbclr, boxtau, boxptop}},
                                 zle, qltot, qitot, rdfl, rdfi, {fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea},
                                 {modis_mean, modis_hist}},
                                frocean, ice_type, {clcalipso, cldlayer, cfad_sr, parasolrefl, lidarpmol}};
    C.cosp.ic.cosp = true; C.cosp.ic.seed = seed; C.cosp.ic.sgfcld = sgfcld;
    return c->cosp_lidar_dev((hipStream_t)stream, C);
}

// ---- include/geosrad_radar.h -------------------------------------------------------------------------------------------------
int geosrad_prec_scops(geosrad_ctx *c, int npoints, int nlev, int ncol, const void *ls_p_rate, const void *cv_p_rate, const void *frac_out,
                       void *prec_frac)
{
    return c ? c->prec_scops_host({npoints, nlev, ncol, ls_p_rate, cv_p_rate, frac_out, prec_frac}) : GEOSRAD_EINVAL;
}
int geosrad_prec_scops_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, int ncol, const void *ls_p_rate, const void *cv_p_rate,
                           const void *frac_out_u8, void *prec_frac_u8)
{
    return c ? c->prec_scops_dev((hipStream_t)stream, {npoints, nlev, ncol, ls_p_rate, cv_p_rate, frac_out_u8, prec_frac_u8}) : GEOSRAD_EINVAL;
}
#define SGHYDRO_CALL(frac, prec)                                                                                                         \
    {npoints, nlev, ncol, frac, {mr_lsliq, mr_lsice, mr_lsrain, mr_lssnow, mr_cvliq, mr_cvice, mr_cvrain, mr_cvsnow, mr_lsgrpl}, prec,   \
        {frac_ls, frac_cv, prec_ls, prec_cv, mr_sub, mr_hydro_sg}}
int geosrad_cosp_sghydro(geosrad_ctx *c, int npoints, int nlev, int ncol, const void *frac_out, const void *mr_lsliq, const void *mr_lsice,
                         const void *mr_lsrain, const void *mr_lssnow, const void *mr_cvliq, const void *mr_cvice, const void *mr_cvrain,
                         const void *mr_cvsnow, const void *mr_lsgrpl, void *prec_frac, void *frac_ls, void *frac_cv, void *prec_ls,
                         void *prec_cv, void *mr_sub, void *mr_hydro_sg)
{
    if (!c) return GEOSRAD_EINVAL;
    const geosrad_ctx::SgHydroCall C = SGHYDRO_CALL(frac_out, prec_frac);
    return c->sghydro_host(C);
}
int geosrad_cosp_sghydro_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, int ncol, const void *frac_out_u8, const void *mr_lsliq,
                             const void *mr_lsice, const void *mr_lsrain, const void *mr_lssnow, const void *mr_cvliq, const void *mr_cvice,
                             const void *mr_cvrain, const void *mr_cvsnow, const void *mr_lsgrpl, void *prec_frac_u8, void *frac_ls,
                             void *frac_cv, void *prec_ls, void *prec_cv, void *mr_sub, void *mr_hydro_sg)
{
    if (!c) return GEOSRAD_EINVAL;
    const geosrad_ctx::SgHydroCall C = SGHYDRO_CALL(frac_out_u8, prec_frac_u8);
    return c->sghydro_dev((hipStream_t)stream, C);
}
int geosrad_radar_gases(geosrad_ctx *c, int npoints, int nlev, const void *p, const void *t, const void *rh, const void *zlev, double freq,
                        int surface_radar, void *g_vol, void *g_to_vol)
{
    return c ? c->radar_gases_host({npoints, nlev, surface_radar, freq, {p, t, rh, zlev}, {g_vol, g_to_vol}}) : GEOSRAD_EINVAL;
}
int geosrad_radar_gases_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, const void *p, const void *t, const void *rh,
                            const void *zlev, double freq, int surface_radar, void *g_vol, void *g_to_vol)
{
    return c ? c->radar_gases_dev((hipStream_t)stream, {npoints, nlev, surface_radar, freq, {p, t, rh, zlev}, {g_vol, g_to_vol}}) : GEOSRAD_EINVAL;
}
int geosrad_misr_dev(geosrad_ctx *c, void *stream, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *zfull, const void *at,
                     const void *dtau_s, const void *dtau_c, const void *frac_out_u8, double missing_value, void *fq_MISR_TAU_v_CTH,
                     void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea)
{
    if (!c) return GEOSRAD_EINVAL;
    return c->misr_dev((hipStream_t)stream, {npoints, nlev, ncol, missing_value, sunlit, {zfull, at, dtau_s, dtau_c}, frac_out_u8,
                                             {fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea}});
}

int geosrad_profile(geosrad_ctx *c, int enable)
{
    if (!c) return GEOSRAD_EINVAL;
    c->prof_collect();
    c->profiling = enable != 0;
    for (int k = 0; k < 16; k++) { c->prof_ms[k] = 0; c->prof_n[k] = 0; }
    return GEOSRAD_OK;
}
int geosrad_profile_read(geosrad_ctx *c, int kernel_id, double *total_ms, long *launches)
{
    if (!c || kernel_id < 0 || kernel_id >= 16) return GEOSRAD_EINVAL;
    (void)hipSetDevice(c->device);
    c->prof_collect();
    if (total_ms) *total_ms = c->prof_ms[kernel_id];
    if (launches) *launches = c->prof_n[kernel_id];
    return GEOSRAD_OK;
}
const char *geosrad_kernel_name(int kernel_id)
{
    static const char *nm[14] = {"k_validate_pwv", "k_setcoef", "k_overlap", "k_mcica", "k_lw_bands", "k_lw_reduce",
                                 "k_sw_validate", "k_sw_setcoef", "k_sw_bands", "k_sw_reduce", "k_chou_prep", "k_chou_bands",
                                 "k_sorad_prep", "k_sorad_pass"};
    return kernel_id >= 0 && kernel_id < 14 ? nm[kernel_id] : "";
}

// the name of the kernel that runs in a profile slot under THIS context's kernel paths (GEOSRAD_SW_PATH / _LW_PATH / _SORAD_PATH), as it
// appears in rocprofv3's kernel trace
const char *geosrad_kernel_label(geosrad_ctx *c, int kernel_id)
{
    if (!c) return geosrad_kernel_name(kernel_id);
    switch (kernel_id) {
    case 4: return c->lw_cols_path ? "k_lw_cols" : (c->lw_split_path ? "k_lw_cells+k_lw_sweep" : "k_lw_bands");
    case 8: return c->sw_path == 2 ? "k_sw_reform" : "k_sw_bands";
    case 9: return c->sw_path == 2 ? "k_swr_reduce" : "k_sw_reduce";
    case 13: return (c->overcast & GEOSRAD_OVERCAST_SORAD) ? "k_sorad_pass_oc" : (c->sorad_col_path ? "k_sorad_col" : "k_sorad_pass");
    default: return geosrad_kernel_name(kernel_id);
    }
}

int geosrad_check(geosrad_ctx *c, void *stream) { return c ? c->check((hipStream_t)stream) : GEOSRAD_EINVAL; }

// test hook: gr_div64 / gr_rcp64 / gr_sqrt64 (lw_kernels.hpp), the division / reciprocal / square root of the fp64 RRTMG_SW instantiation
static __global__ void k_dbg_fast64(int n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ q,
                                    double *__restrict__ r, double *__restrict__ s)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { q[i] = geosrad::gr_div64(a[i], b[i]); r[i] = geosrad::gr_rcp64(b[i]); s[i] = geosrad::gr_sqrt64(b[i]); }
}
int geosrad_dbg_fast64(int n, const double *a, const double *b, double *quot, double *rcp, double *root)
{
    if (n <= 0 || !a || !b || !quot || !rcp || !root) return GEOSRAD_EINVAL;
    DevBuf<double> d;
    const size_t nb = (size_t)n * sizeof(double);
    if (d.resize(5 * nb) != hipSuccess) return GEOSRAD_EHIP;
    int rc = GEOSRAD_OK;
    if (hipMemcpy(d, a, nb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + n, b, nb, hipMemcpyHostToDevice) != hipSuccess) rc = GEOSRAD_EHIP;
    if (rc == GEOSRAD_OK) {
        k_dbg_fast64<<<(n + 255) / 256, 256>>>(n, d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, d + 4 * (size_t)n);
        if (hipMemcpy(quot, d + 2 * (size_t)n, nb, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rcp, d + 3 * (size_t)n, nb, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(root, d + 4 * (size_t)n, nb, hipMemcpyDeviceToHost) != hipSuccess) rc = GEOSRAD_EHIP;
    }
    return rc;
}

int geosrad_rrtmg_lw_taumol(geosrad_ctx *c, int ncol, int nlay, const void *play, const void *plev, const void *tlay, const void *tlev,
                            const void *tsfc, const void *emis, const void *h2ovmr, const void *o3vmr, const void *co2vmr,
                            const void *ch4vmr, const void *n2ovmr, const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr,
                            const void *cfc22vmr, const void *ccl4vmr, const void *tauaer, void *taug, void *pfracs)
{
    if (!c || !taug || !pfracs) return GEOSRAD_EINVAL;
    // clear-sky run with a zero cloud field; fluxes are discarded
    const size_t esz = (size_t)c->real_kind;
    std::vector<char> zero((size_t)ncol * (nlay + 1) * esz, 0), ones((size_t)ncol * nlay * esz, 0), scratch((size_t)ncol * (nlay + 1) * esz * 4);
    for (size_t i = 0; i < (size_t)ncol * nlay; i++) { if (esz == 4) ((float *)ones.data())[i] = 10.f; else ((double *)ones.data())[i] = 10.; }
    std::vector<int32_t> cc((size_t)ncol * 4);
    const void *cldf = zero.data(), *ciwp = zero.data(), *clwp = zero.data(), *rei = ones.data(), *rel = ones.data(), *zm = zero.data(),
               *alat = zero.data();
    LW_PACK_IN();
    char *s = scratch.data();
    const size_t cv = (size_t)ncol * (nlay + 1) * esz;
    void *out[O_NOUT] = {s, s + cv, s + 2 * cv, s + 3 * cv, nullptr, nullptr, nullptr, nullptr};
    return c->lw_host(ncol, nlay, 0, in, 3, 1, 1, 1, 2, cc.data(), out, nullptr, taug, pfracs);
}

int geosrad_mcica(geosrad_ctx *c, int ncol, int nsubcol, int nlay, const void *zmid, const void *alat, int doy, const void *play,
                  const void *cldfrac, const void *ciwp, const void *clwp, double cwp_tiny, const int32_t seed_order[4],
                  int32_t *cldy_stoch, void *ciwp_stoch, void *clwp_stoch)
{
    if (!c || !zmid || !alat || !play || !cldfrac || !ciwp || !clwp || !cldy_stoch || !ciwp_stoch || !clwp_stoch) return GEOSRAD_EINVAL;
    return c->mcica_host(ncol, nsubcol, nlay, zmid, alat, doy, play, cldfrac, ciwp, clwp, cwp_tiny, seed_order, cldy_stoch, ciwp_stoch,
                         clwp_stoch);
}

int geosrad_mcica_dev(geosrad_ctx *c, void *stream, int ncol, int nsubcol, int nlay, const void *zmid, const void *alat, int doy,
                      const void *play, const void *cldfrac, const void *ciwp, const void *clwp, double cwp_tiny,
                      const int32_t seed_order[4], int32_t *cldy_stoch, void *ciwp_stoch, void *clwp_stoch)
{
    if (!c || !zmid || !alat || !play || !cldfrac || !ciwp || !clwp || !cldy_stoch || !ciwp_stoch || !clwp_stoch) return GEOSRAD_EINVAL;
    return c->mcica_dev((hipStream_t)stream, ncol, nsubcol, nlay, zmid, alat, doy, play, cldfrac, ciwp, clwp, cwp_tiny, seed_order,
                        cldy_stoch, ciwp_stoch, clwp_stoch);
}

int geosrad_clearcounts(geosrad_ctx *c, int ncol, int nsubcol, int nlay, int cloudLM, int cloudMH, const int32_t *cldy, int32_t *cnt)
{
    if (!c || !cldy || !cnt || ncol <= 0) return GEOSRAD_EINVAL;
    if (cloudLM == cloudMH) return c->fail(GEOSRAD_EINPUT, "invalid pressure super-layers!");
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(GEOSRAD_EHIP, "hipSetDevice");
    DevBuf<int32_t> d_in, d_out;
    const size_t nin = (size_t)ncol * nsubcol * nlay * 4;
    if (d_in.resize(nin) != hipSuccess || d_out.resize((size_t)ncol * 16) != hipSuccess) return c->fail(GEOSRAD_ENOMEM, "hipMalloc failed in geosrad_clearcounts");
    int rc = GEOSRAD_OK;
    if (hipMemcpy(d_in, cldy, nin, hipMemcpyHostToDevice) != hipSuccess) rc = c->fail(GEOSRAD_EHIP, "hipMemcpy H2D");
    if (!rc) {
        hipLaunchKernelGGL(k_clearcounts, dim3((unsigned)((ncol + 63) / 64)), dim3(64), 0, c->stream, ncol, nsubcol, nlay, cloudLM, cloudMH,
                           (const int32_t *)d_in, d_out.p);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(cnt, d_out, (size_t)ncol * 16, hipMemcpyDeviceToHost) != hipSuccess)
            rc = c->fail(GEOSRAD_EHIP, "k_clearcounts failed");
    }
    return rc;
}

}  // extern "C"
#endif   // GEOSRAD_PART == 0
