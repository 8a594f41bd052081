// A/B of k_sw_update_clouds<R, NB, WPS> (profiles/r05_sw_clouds.md): layers per load batch NB in {1, 2, 4, 8} x minimum waves per SIMD
// WPS in {1, 2} (__launch_bounds__), 97 200 columns x 72 layers of synthetic cloudy columns, every export and the 2-D ones.  Build and run:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize profiles/tools/sw_clouds_ab.hip -o sw_clouds_ab
//   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ab -- ./sw_clouds_ab
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
#include "../../include/geosrad.h"
#include "../../geosradiation_gridcomp_amd/csrc/gridcomp_kernels.hpp"
using namespace geosrad;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

template <typename R> struct Bench {
    int n = 97200, lm = 72;
    SwCld<R> U{};
    SoradDev<R> *dT = nullptr;
    std::vector<void *> bufs;
    R *dev(const std::vector<R> &h) { R *p; CK(hipMalloc((void **)&p, h.size() * sizeof(R))); CK(hipMemcpy(p, h.data(), h.size() * sizeof(R), hipMemcpyHostToDevice)); bufs.push_back(p); return p; }
    Bench() {
        std::mt19937 g(7); std::uniform_real_distribution<double> u(0, 1);
        size_t c = (size_t)n * lm;
        std::vector<R> fc(c), ple((size_t)n * (lm + 1)), t(c), q(c), r(c), z(n);
        for (size_t i = 0; i < c; i++) { fc[i] = u(g) < 0.5 ? (R)u(g) : 0; t[i] = 200 + 90 * u(g); }
        for (int k = 0; k <= lm; k++) for (int i = 0; i < n; i++) ple[(size_t)k * n + i] = (R)(100.0 + k * 1400.0);
        for (int i = 0; i < n; i++) z[i] = (R)(u(g) - 0.4);
        U.ncol = n; U.lm = lm; U.ict = 30; U.icb = 50; U.optics = 1; U.grav = (R)9.80665; U.undef = (R)1e15; U.taucrit = (R)0.1;
        U.in[GEOSRAD_SWK_FCLD] = dev(fc); U.in[GEOSRAD_SWK_PLE] = dev(ple); U.in[GEOSRAD_SWK_T] = dev(t); U.in[GEOSRAD_SWK_ZTH] = dev(z);
        for (int s = 0; s < 4; s++) {
            for (size_t i = 0; i < c; i++) { q[i] = (R)(1e-5 * u(g)); r[i] = (R)((10 + 60 * u(g)) * 1e-6); }
            U.in[GEOSRAD_SWK_QI + s] = dev(q); U.in[GEOSRAD_SWK_RI + s] = dev(r);
        }
        std::vector<R> caif(99); for (auto &x : caif) x = (R)(0.5 + 0.4 * u(g));
        SoradDev<R> T{}; T.caif = dev(caif); T.aib_uv = (R)1.64; T.awb_uv[0] = (R)-6.59e-3; T.awb_uv[1] = (R)1.65; T.arb_uv[0] = (R)3.07e-3;
        CK(hipMalloc((void **)&dT, sizeof(T))); CK(hipMemcpy(dT, &T, sizeof(T), hipMemcpyHostToDevice));
        for (int k = 0; k < GEOSRAD_SWK_NOUT; k++) { R *p; size_t m = k <= GEOSRAD_SWK_TAUCLS ? c : (size_t)n; CK(hipMalloc((void **)&p, m * sizeof(R))); bufs.push_back(p); U.out[k] = p; }
    }
    template <int NB, int WPS> void run(bool all) {
        SwCld<R> V = U;
        if (!all) for (int k = 0; k <= GEOSRAD_SWK_TAUCLS; k++) V.out[k] = nullptr;
        hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
        float best = 1e9;
        for (int it = 0; it < 6; it++) {
            CK(hipEventRecord(a));
            hipLaunchKernelGGL((k_sw_update_clouds<R, NB, WPS>), dim3((n + 255) / 256), dim3(256), 0, 0, V, (const SoradDev<R> *)dT);
            CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
            float ms; CK(hipEventElapsedTime(&ms, a, b)); if (it) best = ms < best ? ms : best;
        }
        CK(hipGetLastError());
        printf("%-6s %-4s NB=%d WPS=%d: %.3f ms\n", sizeof(R) == 4 ? "fp32" : "fp64", all ? "all" : "2d", NB, WPS, best);
    }
    template <int WPS> void sweep(bool all) { run<1, WPS>(all); run<2, WPS>(all); run<4, WPS>(all); run<8, WPS>(all); }
};
int main() {
    { Bench<float> B; for (bool all : {true, false}) { B.sweep<1>(all); B.sweep<2>(all); } }
    { Bench<double> B; for (bool all : {true, false}) { B.sweep<1>(all); B.sweep<2>(all); } }
    return 0;
}
