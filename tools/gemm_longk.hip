// Micro-benchmark (development tool): the fp64 MFMA GEMM kernels at long K -- how far the main loop alone is from the
// 78.6 TFLOP/s peak, beside the short-K shapes of the trailing update (prologue / epilogue share).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -Wall -Wno-unused-function -Wno-unused-value tools/gemm_longk.hip -o tools/gemm_bench_longk
#include "../conicip.jl_amd/csrc/gemm_f64.hip"
#include <cstdio>
#include <vector>
#include <cstdlib>
void cip_set_error(const char *fmt, ...) {}
int cip_env_int(const char *, int dflt) { return dflt; }      // (stand-alone build: every switch at its default)
thread_local CipGraphBuilder *cip_tl_builder = nullptr;
thread_local CipBatchCtx cip_tl_bz = {1, 0, 1ull, nullptr, nullptr};
int main() {
    const int Nmax = 8192, Kmax = 8192;
    double *W, *L, *C;
    hipMalloc(&W, (size_t)Nmax * Kmax * 8); hipMalloc(&L, (size_t)Nmax * Kmax * 8); hipMalloc(&C, (size_t)Nmax * Nmax * 8);
    std::vector<double> h((size_t)Nmax * Kmax);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (double)rand() / RAND_MAX - 0.5;
    hipMemcpy(W, h.data(), h.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(L, h.data(), h.size() * 8, hipMemcpyHostToDevice);
    hipMemset(C, 0, (size_t)Nmax * Nmax * 8);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int shapes[][3] = {{8192, 768, 1}, {8192, 2048, 1}, {8192, 8192, 1}, {4096, 768, 0}, {4096, 8192, 0}, {8192, 8192, 0}};
    for (auto &sh : shapes) {
        const int r = sh[0], K = sh[1], lower = sh[2];
        auto launch = [&] {
            return lower ? cip_gemm_lower(0, r, K, -1.0, W, Nmax, L, Nmax, C, Nmax) : cip_gemm_rect(0, r, r, K, -1.0, W, Nmax, L, Nmax, C, Nmax);
        };
        for (int w = 0; w < 2; ++w) launch();
        hipDeviceSynchronize();
        const int reps = 5;
        hipEventRecord(e0, 0);
        for (int i = 0; i < reps; ++i) launch();
        hipEventRecord(e1, 0); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        const double alg = lower ? (double)r * (r + 1) * K : 2.0 * r * r * K;
        printf("r=%5d K=%4d lower=%d : %9.1f us  %.1f TF\n", r, K, lower, ms * 1e3 / reps, alg / (ms / reps) / 1e9);
    }
    return 0;
}
