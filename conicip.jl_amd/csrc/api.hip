// C ABI of libcipkkt (see include/cipkkt.h for the contract and the reference lines
// each entry point replaces).
#include "cip_handle.h"
#include <thread>
#include <stdlib.h>
#include "../../include/cipkkt.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <new>

static thread_local char g_err[512] = "";
void cip_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *cip_last_error(void) { return g_err; }

// ------------------------------------------------------------------ environment switches (cip_internal.h)
int cip_env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
long cip_env_long(const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; }
double cip_env_double(const char *name, double dflt) { const char *e = getenv(name); return e ? atof(e) : dflt; }
bool cip_env_set(const char *name) { return getenv(name) != nullptr; }

// ------------------------------------------------------------------ profiler ranges (roctx)
// "cip:scaling", "cip:assemble", "cip:ldlt", "cip:solve3x3", "cip:iteration" ranges for rocprofv3 --marker-trace.  The
// marker library is looked up at run time (no link-time dependency: the library links libamdhip64 only); absent or
// CIP_ROCTX=0 -> no-ops.
#include <dlfcn.h>
#include <mutex>
static int (*g_roctx_push)(const char *) = nullptr;
static int (*g_roctx_pop)(void) = nullptr;
static std::once_flag g_roctx_once;
static void roctx_init(void) {
    if (cip_env_int("CIP_ROCTX", 1) == 0) return;
    for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
        if (void *lib = dlopen(name, RTLD_LAZY | RTLD_LOCAL)) {
            g_roctx_push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
            g_roctx_pop = (int (*)(void))dlsym(lib, "roctxRangePop");
            if (g_roctx_push && g_roctx_pop) return;
            g_roctx_push = nullptr; g_roctx_pop = nullptr;
        }
    }
}
void cip_range_push(const char *name) {
    std::call_once(g_roctx_once, roctx_init);
    if (g_roctx_push) (void)g_roctx_push(name);
}
void cip_range_pop(void) { if (g_roctx_pop) (void)g_roctx_pop(); }

static int rup(int x, int q) { return ((x + q - 1) / q) * q; }

// TEST SWITCH (CIP_DEBUG_POISON=<byte 1..255>): every buffer of a handle starts out filled with that byte (255: NaNs and -1s; 63: doubles of
// 4.8e-4 and huge ints) instead of whatever the allocator hands out -- fresh memory of a fresh process is zero, recycled memory of a long
// one is not, and nothing may depend on either.  tests/test_gpu_poison.py runs trajectories under it and compares the bits.
static int debug_poison(void *p, size_t bytes) {
    static const int v = cip_env_int("CIP_DEBUG_POISON", 0) & 255;
    if (!v) return 0;
    CIP_HIP_CHECK(hipDeviceSynchronize());
    CIP_HIP_CHECK(hipMemset(p, v, bytes));
    CIP_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}
// A device allocation of the handle's own: its block (create_impl), or a buffer of first use
int cip_handle_alloc(cip_handle *h, void **out, size_t bytes) {
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipErrorOutOfMemory) {
        // the lock-step arena of an earlier batch (several GB, kept for the next one) may be what is in the way: give it back, once
        (void)hipGetLastError();
        (void)cip_release_cached_memory();
        e = hipMalloc(out, bytes);
    }
    CIP_HIP_CHECK(e);
    h->owned.push_back(*out);
    return debug_poison(*out, bytes);
}

static void free_all(cip_handle *h) {
    if (h->gx_factor) { (void)hipGraphExecDestroy(h->gx_factor); h->gx_factor = nullptr; }
    if (h->ldlt_side) { cip_ldlt_side_destroy(h->ldlt_side); h->ldlt_side = nullptr; }
    if (h->gx_solve) { (void)hipGraphExecDestroy(h->gx_solve); h->gx_solve = nullptr; }
    if (h->cs.lg) { cip_sdp_large_destroy(h->cs.lg); h->cs.lg = nullptr; }
    for (auto it = h->owned.rbegin(); it != h->owned.rend(); ++it) (void)hipFree(*it);
    h->owned.clear();
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev2) (void)hipEventDestroy(h->ev2);
    if (h->info_host) (void)hipHostFree(h->info_host);
    if (h->ws.prof) { cip_ldlt_profile_destroy(h->ws.prof); h->ws.prof = nullptr; }
}

// copy a (rows x cols, ld) column-major matrix from src (host or device) into a tight device buffer
static int upload_matrix(double *dst, long ld_dst, const double *src, long ld_src, int rows, int cols, bool src_dev,
                         hipStream_t s) {
    if (rows == 0 || cols == 0) return 0;
    CIP_HIP_CHECK(hipMemcpy2DAsync(dst, ld_dst * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), cols,
                                   src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    return 0;
}

// dst (cols x rows, ld ld_dst) = src' ; tiled through LDS
__global__ __launch_bounds__(256) void k_transpose(const double *src, long ld_src, int rows, int cols, double *dst, long ld_dst) {
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    for (int q = 0; q < 32; q += 8) {
        const int r = r0 + tx, c = c0 + ty + q;
        if (r < rows && c < cols) t[ty + q][tx] = src[r + (long)c * ld_src];
    }
    __syncthreads();
    for (int q = 0; q < 32; q += 8) {
        const int c = c0 + tx, r = r0 + ty + q;
        if (r < rows && c < cols) dst[c + (long)r * ld_dst] = t[tx][ty + q];
    }
}
static int transpose_dev(hipStream_t s, const double *src, long ld_src, int rows, int cols, double *dst, long ld_dst) {
    if (rows == 0 || cols == 0) return 0;
    hipLaunchKernelGGL(k_transpose, dim3((rows + 31) / 32, (cols + 31) / 32), dim3(256), 0, s, src, ld_src, rows, cols, dst, ld_dst);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- CSR Q (CIP_FLAG_Q_CSR): the level-1 check, on the host, O(nnz).  Device-resident arrays are copied back first (as A's are).
// Two counting-sort transposes: T = Q' lists, for every i, the stored (j, i) with j ascending; its transpose S is Q again with the
// columns of every row ascending.  A duplicate is a repeated column in a row of S; Q is symmetric when S and T agree entry for entry,
// values bit for bit.  On success the handle's staging vectors hold S (what is uploaded: the mat-vec's summation order does not
// depend on the caller's column order) and *maxrow the longest row.  No device allocation, nothing enqueued.
// expect_nnz >= 0 (cip_update_problem): the count the handle was created with.
static void csr_transpose(int n, const std::vector<int> &rp, const std::vector<int> &ci, const std::vector<double> &v,
                          std::vector<int> &trp, std::vector<int> &tci, std::vector<double> &tv) {
    const int nnz = rp[n];
    trp.assign(n + 1, 0); tci.assign(nnz > 0 ? nnz : 1, 0); tv.assign(nnz > 0 ? nnz : 1, 0.0);
    for (int q = 0; q < nnz; ++q) trp[ci[q] + 1]++;
    for (int i = 0; i < n; ++i) trp[i + 1] += trp[i];
    std::vector<int> fill(trp.begin(), trp.end() - 1);
    for (int r = 0; r < n; ++r)
        for (int q = rp[r]; q < rp[r + 1]; ++q) { const int d = fill[ci[q]]++; tci[d] = r; tv[d] = v[q]; }
}
static int stage_Q_csr(cip_handle *h, const cip_problem *pr, int expect_nnz, int *maxrow) {
    const int n = pr->n;
    if (pr->Q) { cip_set_error("CIP_FLAG_Q_CSR is set but Q is not NULL"); return CIP_E_INVALID; }
    if (!pr->Q_rowptr) { cip_set_error("CSR Q: Q_rowptr is NULL"); return CIP_E_INVALID; }
    const bool csr_dev = (pr->flags & CIP_FLAG_DEVICE_PTRS) && !(pr->flags & CIP_FLAG_CSR_HOST);
    std::vector<int> rp(n + 1), ci, trp, tci;
    std::vector<double> v, tv;
    if (csr_dev) CIP_HIP_CHECK(hipMemcpy(rp.data(), pr->Q_rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
    else memcpy(rp.data(), pr->Q_rowptr, sizeof(int) * (n + 1));
    if (rp[0] != 0) { cip_set_error("CSR Q: rowptr[0] is %d, not 0", rp[0]); return CIP_E_INVALID; }
    for (int i = 0; i < n; ++i)
        if (rp[i + 1] < rp[i]) { cip_set_error("CSR Q: the row pointer decreases at row %d (%d after %d)", i, rp[i + 1], rp[i]); return CIP_E_INVALID; }
    const int nnz = rp[n];
    if (expect_nnz >= 0 && nnz != expect_nnz) {
        cip_set_error("cip_update_problem: CSR Q has %d non-zeros, the handle holds %d", nnz, expect_nnz);
        return CIP_E_INVALID;
    }
    if (nnz > 0 && !pr->Q_colind) { cip_set_error("CSR Q: Q_colind is NULL"); return CIP_E_INVALID; }
    if (nnz > 0 && !pr->Q_val) { cip_set_error("CSR Q: Q_val is NULL"); return CIP_E_INVALID; }
    ci.assign(nnz > 0 ? nnz : 1, 0); v.assign(nnz > 0 ? nnz : 1, 0.0);
    if (nnz > 0) {
        if (csr_dev) {
            CIP_HIP_CHECK(hipMemcpy(ci.data(), pr->Q_colind, sizeof(int) * nnz, hipMemcpyDeviceToHost));
            CIP_HIP_CHECK(hipMemcpy(v.data(), pr->Q_val, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        } else {
            memcpy(ci.data(), pr->Q_colind, sizeof(int) * nnz);
            memcpy(v.data(), pr->Q_val, sizeof(double) * nnz);
        }
    }
    int mx = 0;
    for (int i = 0; i < n; ++i) {
        if (rp[i + 1] - rp[i] > mx) mx = rp[i + 1] - rp[i];
        for (int q = rp[i]; q < rp[i + 1]; ++q)
            if (ci[q] < 0 || ci[q] >= n) {
                cip_set_error("CSR Q: entry %d of row %d has column index %d outside [0, %d)", q - rp[i], i, ci[q], n);
                return CIP_E_INVALID;
            }
    }
    csr_transpose(n, rp, ci, v, trp, tci, tv);                 // T = Q'
    std::vector<int> &srp = h->st_qrp, &sci = h->st_qci;
    std::vector<double> &sv = h->st_qv;
    csr_transpose(n, trp, tci, tv, srp, sci, sv);              // S = Q, columns ascending
    for (int i = 0; i < n; ++i)
        for (int q = srp[i] + 1; q < srp[i + 1]; ++q)
            if (sci[q] == sci[q - 1]) { cip_set_error("CSR Q: entry (%d, %d) is stored twice", i, sci[q]); return CIP_E_INVALID; }
    for (int i = 0; i < n; ++i) {
        int a = srp[i], b = trp[i];
        const int a1 = srp[i + 1], b1 = trp[i + 1];
        while (a < a1 || b < b1) {
            if (b == b1 || (a < a1 && sci[a] < tci[b])) {
                cip_set_error("CSR Q: entry (%d, %d) has no stored mirror entry (%d, %d)", i, sci[a], sci[a], i);
                return CIP_E_INVALID;
            }
            if (a == a1 || tci[b] < sci[a]) {
                cip_set_error("CSR Q: entry (%d, %d) has no stored mirror entry (%d, %d)", tci[b], i, i, tci[b]);
                return CIP_E_INVALID;
            }
            if (memcmp(&sv[a], &tv[b], sizeof(double)) != 0) {
                cip_set_error("CSR Q: entry (%d, %d) = %.17g and its mirror entry (%d, %d) = %.17g differ", i, sci[a], sv[a], sci[a], i, tv[b]);
                return CIP_E_INVALID;
            }
            ++a; ++b;
        }
    }
    if (maxrow) *maxrow = mx;
    return 0;
}
// the mat-vec form of a CSR Q, from its longest row: one thread per row, or one wave per row (vecops.hip) above the threshold
static int q_wave_form(int maxrow) {
    static const int wave_min = cip_env_int("CIP_QSPMV_WAVE_MIN", CIP_SPMV_WAVE_MIN);
    return maxrow > wave_min ? 1 : 0;
}

// y = alpha Q x + beta y with the handle's Q, dense or CSR (cip_gemv_dev(CIP_MAT_Q), the refinement's residual).  symv: a dense Q
// may go through the symmetric mat-vec (the refinement's residual never did: it keeps its bits)
int cip_mul_Q(cip_handle *h, double alpha, const double *x, double beta, double *y, bool symv) {
    hipStream_t s = h->stream;
    if (h->Q_sparse && cip_in_batch()) {
        // a lock-step group: h is problem 0's handle, the form is each live problem's own (a ragged group may hold both)
        const unsigned long long live = cip_tl_bz.mask, wave = cip_tl_bz.q_wave & live;
        if (wave == 0) return cip_spmv_csr(s, h->n, h->Q_rp, h->Q_ci, h->Q_v, alpha, x, beta, y);
        if (wave == live) return cip_spmv_csr_wave(s, h->n, h->Q_rp, h->Q_ci, h->Q_v, alpha, x, beta, y);
        return cip_spmv_csr_forms(s, h->n, h->Q_rp, h->Q_ci, h->Q_v, alpha, x, beta, y, wave);
    }
    if (h->Q_sparse)
        return h->Q_wave ? cip_spmv_csr_wave(s, h->n, h->Q_rp, h->Q_ci, h->Q_v, alpha, x, beta, y)
                         : cip_spmv_csr(s, h->n, h->Q_rp, h->Q_ci, h->Q_v, alpha, x, beta, y);
    if (symv && h->symv_ws && !(((uintptr_t)x) & 15)) return cip_symv_lower(s, h->n, alpha, h->Q, h->n, x, beta, y, h->symv_ws);
    return cip_gemv_t(s, h->n, h->n, alpha, h->Q, h->n, x, beta, y);
}

// Contents of Q, G (+G'), A (+A', or the CSR of A and of A') into the handle's buffers, on its stream.  A CSR Q has been checked and
// staged by stage_Q_csr (the caller waited for an earlier upload from the staging vectors first).
static int upload_problem(cip_handle *h, const cip_problem *pr) {
    const int n = h->n, m = h->m, p = h->p;
    const bool dev = (pr->flags & CIP_FLAG_DEVICE_PTRS) != 0;
    hipStream_t s = h->stream;
    const bool was_live = h->staging_live;                  // an earlier upload may still be reading A's staging vectors
    cip_sdp_large_invalidate(h->cs.lg);                     // (the mat(a_i) images of the large S cones follow A)
    if (h->Q_sparse) {
        CIP_HIP_CHECK(hipMemcpyAsync(h->Q_rp, h->st_qrp.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, s));
        if (h->Q_nnz > 0) {
            CIP_HIP_CHECK(hipMemcpyAsync(h->Q_ci, h->st_qci.data(), sizeof(int) * h->Q_nnz, hipMemcpyHostToDevice, s));
            CIP_HIP_CHECK(hipMemcpyAsync(h->Q_v, h->st_qv.data(), sizeof(double) * h->Q_nnz, hipMemcpyHostToDevice, s));
        }
        h->staging_live = true;
    } else CIP_TRY(upload_matrix(h->Q, n, pr->Q, pr->ldq > 0 ? pr->ldq : n, n, n, dev, s));
    if (p > 0) {
        CIP_TRY(upload_matrix(h->G, p, pr->G, pr->ldg > 0 ? pr->ldg : p, p, n, dev, s));
        CIP_TRY(transpose_dev(s, h->G, p, p, n, h->Gt, n));
    }
    if (!h->A_sparse) {
        if (m > 0) {
            CIP_TRY(upload_matrix(h->A, m, pr->A, pr->lda > 0 ? pr->lda : m, m, n, dev, s));
            CIP_TRY(transpose_dev(s, h->A, m, m, n, h->At, h->npad));
        }
        return 0;
    }
    // CSR of A (given) and of A' (built here on the host).  The host arrays live in the handle: the uploads below are
    // asynchronous and nothing here waits for them (a previous upload from the same vectors is waited for first).
    if (was_live) CIP_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int> &rp = h->st_rp, &ci = h->st_ci, &trp = h->st_trp, &tci = h->st_tci;
    std::vector<double> &av = h->st_av, &tv = h->st_tv;
    rp.assign(m + 1, 0);
    const bool csr_dev = dev && !(pr->flags & CIP_FLAG_CSR_HOST);
    if (csr_dev) CIP_HIP_CHECK(hipMemcpy(rp.data(), pr->A_rowptr, sizeof(int) * (m + 1), hipMemcpyDeviceToHost));
    else memcpy(rp.data(), pr->A_rowptr, sizeof(int) * (m + 1));
    const int nnz = rp[m];
    if (rp[0] != 0 || nnz != h->A_nnz) { cip_set_error("bad CSR row pointer (nnz %d, handle holds %d)", nnz, h->A_nnz); return CIP_E_INVALID; }
    ci.assign(nnz > 0 ? nnz : 1, 0);
    av.assign(nnz > 0 ? nnz : 1, 0.0);
    if (nnz > 0) {
        if (csr_dev) {
            CIP_HIP_CHECK(hipMemcpy(ci.data(), pr->A_colind, sizeof(int) * nnz, hipMemcpyDeviceToHost));
            CIP_HIP_CHECK(hipMemcpy(av.data(), pr->A_val, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        } else {
            memcpy(ci.data(), pr->A_colind, sizeof(int) * nnz);
            memcpy(av.data(), pr->A_val, sizeof(double) * nnz);
        }
    }
    for (int q = 0; q < nnz; ++q)
        if (ci[q] < 0 || ci[q] >= n) { cip_set_error("CSR column index out of range"); return CIP_E_INVALID; }
    h->A_one_per_row = true;
    for (int r = 0; r < m; ++r) if (rp[r + 1] - rp[r] > 1) { h->A_one_per_row = false; break; }
    trp.assign(n + 1, 0); tci.assign(nnz > 0 ? nnz : 1, 0);
    tv.assign(nnz > 0 ? nnz : 1, 0.0);
    for (int q = 0; q < nnz; ++q) trp[ci[q] + 1]++;
    for (int i = 0; i < n; ++i) trp[i + 1] += trp[i];
    {
        std::vector<int> fill(trp.begin(), trp.end() - 1);
        for (int r = 0; r < m; ++r)
            for (int q = rp[r]; q < rp[r + 1]; ++q) { const int d = fill[ci[q]]++; tci[d] = r; tv[d] = av[q]; }
    }
    CIP_HIP_CHECK(hipMemcpyAsync(h->A_rp, rp.data(), sizeof(int) * (m + 1), hipMemcpyHostToDevice, s));
    CIP_HIP_CHECK(hipMemcpyAsync(h->T_rp, trp.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        CIP_HIP_CHECK(hipMemcpyAsync(h->A_ci, ci.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, s));
        CIP_HIP_CHECK(hipMemcpyAsync(h->A_v, av.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, s));
        CIP_HIP_CHECK(hipMemcpyAsync(h->T_ci, tci.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, s));
        CIP_HIP_CHECK(hipMemcpyAsync(h->T_v, tv.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, s));
    }
    h->staging_live = true;
    if (h->AtS) return cip_scatter_AtS(h);                  // assemble.hip: the S cones' rows of A' as a dense block
    return 0;
}

// ---- level 1 in three parts: the plan (host), the layout of the device block (one walk sizes it, one carves it), the fill
// Plan: argument checks, the cone and work-item tables and their index lists, padded sizes, what the problem's form selects (route,
// dense / CSR Q and A, split-K images) and the counts the layout needs.  Nothing is allocated on the device; the one thing read from
// it is the nnz of a CSR A whose row pointers live there.
static int handle_plan(const cip_problem *pr, cip_handle *h) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        cip_set_error("no HIP device available (libcipkkt has no CPU fallback)");
        return CIP_E_NODEVICE;
    }
    CIP_HIP_CHECK(hipGetDevice(&h->device));
    if (cip_kernels_init()) return CIP_E_HIP;
    const int n = pr->n, m = pr->m, p = pr->p;
    if (n <= 0 || m < 0 || p < 0 || pr->ncones < 0) { cip_set_error("bad dimensions n=%d m=%d p=%d", n, m, p); return CIP_E_INVALID; }
    const bool q_csr = (pr->flags & CIP_FLAG_Q_CSR) != 0;
    if (!q_csr && !pr->Q) { cip_set_error("Q is NULL"); return CIP_E_INVALID; }
    if (m > 0 && !pr->A && !(pr->A_rowptr && pr->A_colind && pr->A_val)) { cip_set_error("A is NULL"); return CIP_E_INVALID; }
    if (p > 0 && !pr->G) { cip_set_error("G is NULL"); return CIP_E_INVALID; }
    if (pr->route != CIP_ROUTE_SCHUR && pr->route != CIP_ROUTE_FULL3X3) { cip_set_error("bad route"); return CIP_E_INVALID; }
    if (q_csr) {                                          // checked on the host before anything is allocated on the device
        int maxrow = 0;
        CIP_TRY(stage_Q_csr(h, pr, -1, &maxrow));
        h->Q_sparse = true; h->Q_nnz = h->st_qrp[n]; h->Q_wave = q_wave_form(maxrow);
    }
    h->n = n; h->m = m; h->p = p; h->ncones = pr->ncones; h->route = pr->route;
    const bool dev = (pr->flags & CIP_FLAG_DEVICE_PTRS) != 0;

    // ---- cones
    int off = 0, nq = 0;
    size_t soff = 0;
    bool has_S = false;
    std::vector<int> &sidx = h->st_sidx;
    int rmax = 0, kmax = 0;
    for (int c = 0; c < pr->ncones; ++c) {
        ConeDesc cd = {};
        cd.type = pr->cone_type[c]; cd.dim = pr->cone_dim[c]; cd.off = off; cd.soff = (int)soff; cd.r = 0; cd.qidx = -1; cd.aoff = off;
        if (cd.dim <= 0) { cip_set_error("cone %d has dimension %d", c, cd.dim); return CIP_E_INVALID; }
        if (cd.type == CIP_CONE_R) { soff += cd.dim; }
        else if (cd.type == CIP_CONE_Q) { soff += 1 + cd.dim; cd.qidx = nq++; }
        else if (cd.type == CIP_CONE_S) {
            const int r = (int)llround((sqrt(1.0 + 8.0 * cd.dim) - 1.0) / 2.0);     // ord() src/ConicIP.jl:85
            if (r * (r + 1) / 2 != cd.dim) { cip_set_error("S cone %d: %d is not a triangular number", c, cd.dim); return CIP_E_INVALID; }
            if (r > 2048) { cip_set_error("S cone %d: matrix order %d > 2048 is not supported", c, r); return CIP_E_UNSUPPORTED; }
            cd.r = r; soff += 2 * (size_t)r * r; has_S = true;
            sidx.push_back(c);
            if (r > rmax) rmax = r;
            if (cd.dim > kmax) kmax = cd.dim;
        } else { cip_set_error("cone %d: unknown type %d", c, cd.type); return CIP_E_INVALID; }
        if (soff > 0x7fffffffULL) { cip_set_error("scaling storage too large"); return CIP_E_INVALID; }
        h->h_cones.push_back(cd);
        off += cd.dim;
    }
    // work items (one workgroup each) and partial-result slots.  Consecutive Q cones of dimension <= 64 are packed:
    // lane segments of width W = next power of two of the run's largest cone, 256 / W cones per workgroup.
    int nslots = 0;
    for (int c = 0; c < pr->ncones;) {
        ConeDesc &cd = h->h_cones[c];
        if (cd.type == CIP_CONE_R) {
            cd.item = nslots;
            for (int st = 0; st < cd.dim; st += 2048) h->h_items.push_back(WorkItem{c, st, (cd.dim - st < 2048) ? cd.dim - st : 2048, nslots++, 0});
            ++c;
        } else if (cd.type == CIP_CONE_Q && cd.dim <= 64) {
            int e = c, dmax = 0;
            while (e < pr->ncones && h->h_cones[e].type == CIP_CONE_Q && h->h_cones[e].dim <= 64) { if (h->h_cones[e].dim > dmax) dmax = h->h_cones[e].dim; ++e; }
            int W = 1;
            while (W < dmax) W *= 2;
            const int per = 256 / W;
            for (int q = c; q < e; q += per) {
                const int cnt = (e - q < per) ? (e - q) : per;
                for (int u = 0; u < cnt; ++u) h->h_cones[q + u].item = nslots + u;
                h->h_items.push_back(WorkItem{q, 0, cnt, nslots, W});
                nslots += cnt;
            }
            c = e;
        } else {
            cd.item = nslots;
            h->h_items.push_back(WorkItem{c, 0, cd.dim, nslots++, 0});      // a large Q cone or an S cone: one workgroup
            ++c;
        }
    }
    if (off != m) { cip_set_error("cone_dims cover %d rows but A has %d", off, m); return CIP_E_INVALID; }
    if (has_S && pr->A == NULL && m > 0) {
        // CSR A with S cones (round 4; the reference builds its Schur system from a sparse A whatever the cones,
        // src/kktsolvers.jl:289-293): the S cones' rows are expanded, once, into a dense transposed block of their own
        // (upload_problem) for the congruences of the Schur scaling; everything else stays CSR
        int ao = 0;
        for (ConeDesc &cd : h->h_cones) if (cd.type == CIP_CONE_S) { cd.aoff = ao; ao += cd.dim; }
        h->mS = ao; h->mSpad = rup(ao, CIP_KT);
    }
    h->nq = nq; h->nqpad = rup(nq > 0 ? nq : 1, CIP_KT);
    for (size_t it = 0; it < h->h_items.size(); ++it) {       // index lists: R items, large Q cones (one item each), packs of small Q cones
        const int type = h->h_cones[h->h_items[it].cone].type;
        if (type == CIP_CONE_R) h->st_ritems.push_back((int)it);
        else if (type == CIP_CONE_Q) (h->h_items[it].width == 0 ? h->st_bigq : h->st_packq).push_back((int)it);
    }
    h->cs.nbigq = (int)h->st_bigq.size(); h->cs.nritems = (int)h->st_ritems.size(); h->cs.npackq = (int)h->st_packq.size();
    h->cs.ncones = pr->ncones; h->cs.nitems = (int)h->h_items.size(); h->cs.nslots = nslots; h->cs.m = m; h->cs.scal_len = soff; h->cs.has_S = has_S;
    h->cs.ns = (int)sidx.size(); h->cs.rmax = rmax; h->cs.kmax = kmax;
    h->cs.ns_small = 0; h->cs.rmax_small = 0; h->cs.nlarge = 0;
    h->cs.h_cones = h->h_cones.data();
    if (has_S) {
        std::vector<int> &small = h->st_small;
        for (int c : sidx) {
            if (h->h_cones[c].r >= CIP_LARGE_S_MIN) {
                if (h->cs.nlarge == CIP_MAX_LARGE_S) { cip_set_error("more than %d S cones of order >= %d", CIP_MAX_LARGE_S, CIP_LARGE_S_MIN); return CIP_E_UNSUPPORTED; }
                h->cs.large_cone[h->cs.nlarge++] = c;
            } else {
                small.push_back(c);
                if (h->h_cones[c].r > h->cs.rmax_small) h->cs.rmax_small = h->h_cones[c].r;
            }
        }
        h->cs.ns_small = (int)small.size();
        const int per = n < 64 ? n : 64;
        h->cs.sdp_slots = h->cs.ns * (per > 0 ? per : 1);
    }

    // ---- sizes
    h->npad = rup(n, CIP_NB);
    h->mpad = rup(m > 0 ? m : 1, CIP_KT);
    h->N = (h->route == CIP_ROUTE_SCHUR) ? n + p : n + p + m;
    h->Npad = rup(h->N, CIP_NB);
    h->ldk = h->Npad;

    // ---- the forms of A
    h->A_sparse = (pr->A == NULL && m > 0);
    if (!h->A_sparse) {
        if (h->route == CIP_ROUTE_SCHUR) h->syrk_n = cip_syrk_split(h->npad, h->mpad, &h->syrk_len);
    } else {
        int nnz = 0;
        if (dev && !(pr->flags & CIP_FLAG_CSR_HOST)) CIP_HIP_CHECK(hipMemcpy(&nnz, pr->A_rowptr + m, sizeof(int), hipMemcpyDeviceToHost));
        else nnz = pr->A_rowptr[m];
        if (nnz < 0) { cip_set_error("bad CSR row pointer"); return CIP_E_INVALID; }
        h->A_nnz = nnz;
        std::vector<int> &rc_ = h->st_rowcone;
        rc_.assign(m > 0 ? m : 1, 0);
        for (size_t c = 0; c < h->h_cones.size(); ++c)
            for (int e = 0; e < h->h_cones[c].dim; ++e) rc_[h->h_cones[c].off + e] = (int)c;
    }
    h->ldlt_fused = cip_ldlt_fused_for(h->Npad);          // read ONCE: sizing and carve must agree
    return 0;
}

// [0]: an iterate left the cone; [4 + li]: gate of large cone li's general division (li < nlarge <= CIP_MAX_LARGE_S)
static size_t sdp_flag_words(const ConeSet &cs) { return (size_t)rup(4 + (cs.nlarge > 12 ? cs.nlarge : 12), 16); }

// Layout: every creation-time buffer of a planned handle, in order, each rounded up to 256 bytes; a member of length zero still takes
// a granule (distinct non-null pointers).  Over a null base the walk sizes the handle's device block, over the block it carves: an
// ordinary handle's own allocation, or its slab of a lock-step group's arena -- problem z's walk is problem 0's, so its buffers sit
// at problem 0's addresses + z * stride.  `extras`: what an ordinary handle allocates on first use and a lock-step handle must hold
// at a fixed offset.  The workspace of chip-wide S cones is not part of it (cip_sdp_large_create: an allocation of its own).
template <typename T> static void take(CipLayout &L, T *&ptr, size_t count) { ptr = L.take<T>(count ? count : 1); }
size_t cip_handle_layout(CipLayout L, cip_handle *h, unsigned extras, const CipCsrCap *cap) {
    ConeSet &cs = h->cs;
    const size_t n = h->n, m = h->m, p = h->p, npad = h->npad;
    // (a capacity never below the handle's own count: the uploads fit whatever the caller passed)
    const size_t nnz = cap && cap->A_nnz > (size_t)h->A_nnz ? cap->A_nnz : (size_t)h->A_nnz;
    const size_t qnnz = cap && cap->Q_nnz > (size_t)h->Q_nnz ? cap->Q_nnz : (size_t)h->Q_nnz;
    if (cs.npackq > 0) take(L, cs.d_packq, cs.npackq);
    if (cs.nritems > 0) take(L, cs.d_ritems, cs.nritems);
    if (cs.nbigq > 0) take(L, cs.d_bigq, cs.nbigq);
    take(L, cs.d_cones, cs.ncones); take(L, cs.d_items, cs.nitems); take(L, cs.d_scal, cs.scal_len);
    take(L, cs.d_partial, 2 * ((size_t)cs.nslots + 1));            // two sets: the pair of max-steps (cip_cones_maxstep2)
    take(L, cs.d_scalar, 8);
    if (cs.has_S) {
        take(L, cs.d_sidx_small, (size_t)cs.ns_small + 1); take(L, cs.d_sidx, cs.ns);
        take(L, cs.d_sdpws, (size_t)cs.sdp_slots * CIP_SDP_WS_MATS * cs.rmax * cs.rmax); take(L, cs.d_sdpvec, (size_t)cs.sdp_slots * 2 * cs.kmax);
        take(L, cs.d_sdpflag, sdp_flag_words(cs));
    }
    // Q, G, A: contents by upload_problem (also used by cip_update_problem)
    if (h->Q_sparse) {                                    // O(nnz): neither the dense image nor the symv tables
        take(L, h->Q_rp, n + 1); take(L, h->Q_ci, qnnz); take(L, h->Q_v, qnnz);
    } else {
        take(L, h->Q, n * n);
        if (n >= 2048 && n % 128 == 0) take(L, h->symv_ws, 2 * (n / 128) * n);
    }
    take(L, h->G, p * n); take(L, h->Gt, p * n);
    if (!h->A_sparse) {
        take(L, h->A, m * n); take(L, h->At, npad * h->mpad);
        if (h->route == CIP_ROUTE_SCHUR) {
            take(L, h->Wt, npad * h->mpad);
            if (h->syrk_n > 1) take(L, h->syrk_ws, h->syrk_n * npad * npad);
        }
    } else {
        take(L, h->A_rp, m + 1); take(L, h->A_ci, nnz); take(L, h->A_v, nnz);
        take(L, h->T_rp, n + 1); take(L, h->T_ci, nnz); take(L, h->T_v, nnz);
        take(L, h->kdiag, n); take(L, h->row_cone, m);
        if (h->mS > 0 && h->route == CIP_ROUTE_SCHUR) { take(L, h->AtS, npad * h->mSpad); take(L, h->WtS, npad * h->mSpad); }
        if (h->route == CIP_ROUTE_SCHUR) take(L, h->Gm, npad * h->nqpad);
    }
    // KKT matrix, LDL' workspace, scratch
    take(L, h->K, (size_t)h->ldk * h->Npad);
    h->ws_base = L.take<char>(cip_ldlt_ws_bytes(h->Npad, h->ldlt_fused));
    cip_ldlt_ws_carve(h->ws_base, h->Npad, &h->ws, h->ldlt_fused);
    take(L, h->rhs, h->Npad);
    take(L, h->mt1, m); take(L, h->mt2, m); take(L, h->mt3, m); take(L, h->nt1, n); take(L, h->pt1, p);
    take(L, h->dot_scratch, 32 * 32 + 32);
    { StageView v; h->stage = (double *)L.take<char>(stage_layout(nullptr, h, 1, &v)); }
    if (extras & CIP_EXTRA_DRIVER) h->drv = (double *)L.take<char>(cip_driver_bytes(h));
    if (extras & CIP_EXTRA_REFINE) {
        RefView v;
        h->ref = (double *)L.take<char>(ref_layout(nullptr, h, &v));
        if (m > 0 && h->route == CIP_ROUTE_SCHUR) take(L, h->c2x2, m);
    }
    return L.bytes();
}

// Fill: the small tables, the zero padding, the problem's matrices and the identity scaling into a carved handle, on its stream
static int handle_fill(const cip_problem *pr, cip_handle *h, bool final_sync) {
    ConeSet &cs = h->cs;
    const int n = h->n, m = h->m, p = h->p;
    hipStream_t s = h->stream;   // default (null) stream until cip_set_stream
    auto upload = [s](auto *dst, const auto &src, size_t count) {
        return count ? hipMemcpyAsync(dst, src.data(), sizeof(*dst) * count, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    if (cs.npackq > 0) CIP_HIP_CHECK(upload(cs.d_packq, h->st_packq, cs.npackq));
    if (cs.nritems > 0) CIP_HIP_CHECK(upload(cs.d_ritems, h->st_ritems, cs.nritems));
    if (cs.nbigq > 0) CIP_HIP_CHECK(upload(cs.d_bigq, h->st_bigq, cs.nbigq));
    if (cs.has_S) {
        CIP_HIP_CHECK(upload(cs.d_sidx_small, h->st_small, cs.ns_small));
        if (cs.nlarge > 0) {
            int rmax_large = 0;
            for (int li = 0; li < cs.nlarge; ++li) if (h->h_cones[cs.large_cone[li]].r > rmax_large) rmax_large = h->h_cones[cs.large_cone[li]].r;
            CIP_TRY(cip_sdp_large_create(rmax_large, cs.nlarge, n, &cs.lg));
        }
        CIP_HIP_CHECK(upload(cs.d_sidx, h->st_sidx, cs.ns));
        CIP_HIP_CHECK(hipMemsetAsync(cs.d_sdpflag, 0, sizeof(int) * sdp_flag_words(cs), s));
    }
    CIP_HIP_CHECK(upload(cs.d_cones, h->h_cones, cs.ncones));
    CIP_HIP_CHECK(upload(cs.d_items, h->h_items, cs.nitems));
    if (!h->A_sparse) {
        CIP_HIP_CHECK(hipMemsetAsync(h->At, 0, sizeof(double) * (size_t)h->npad * h->mpad, s));
        if (h->Wt) CIP_HIP_CHECK(hipMemsetAsync(h->Wt, 0, sizeof(double) * (size_t)h->npad * h->mpad, s));
    } else {
        CIP_HIP_CHECK(upload(h->row_cone, h->st_rowcone, m));
        if (h->AtS) {
            CIP_HIP_CHECK(hipMemsetAsync(h->AtS, 0, sizeof(double) * (size_t)h->npad * h->mSpad, s));
            CIP_HIP_CHECK(hipMemsetAsync(h->WtS, 0, sizeof(double) * (size_t)h->npad * h->mSpad, s));
        }
    }
    CIP_TRY(upload_problem(h, pr));
    h->ws.x_zeroed = &h->x_zeroed;
    h->ws.side = h->in_slab ? nullptr : &h->ldlt_side;    // (handles of a lock-step arena factor inside batched launches)
    // pivot signs of the quasi-definite order: Schur route [S G'; G 0] = n positive, p negative; literal 3x3 in the
    // order (3,1,2) = m negative (-F'F), n positive, p negative
    h->ws.signs = (h->route == CIP_ROUTE_SCHUR) ? PivotSigns{0, n, n + p} : PivotSigns{m, m + n, m + n + p};
    CIP_HIP_CHECK(hipEventCreate(&h->ev0)); CIP_HIP_CHECK(hipEventCreate(&h->ev1)); CIP_HIP_CHECK(hipEventCreate(&h->ev2));
    // (the pinned pivot-flag words are allocated by the first factorisation: pinned allocations cost ~0.1 ms each, and the
    //  64 handles of a lock-step group never use theirs)
    CIP_TRY(cip_cones_identity_scaling(s, cs));
    CIP_TRY(cip_sdp_scaling_changed(s, cs));
    // the caller's Q / A / G may go away as soon as a public create returns: wait for the uploads.  A lock-step group
    // keeps its problems alive for the whole call and creates its 64 handles without a single host wait.
    if (final_sync) CIP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int cip_create_ex(const cip_problem *prob, cip_handle **out) {
    if (!prob || !out) { cip_set_error("NULL argument"); return CIP_E_INVALID; }
    *out = NULL;
    cip_handle *h = nullptr;
    int rc = cip_plan(prob, nullptr, &h);
    void *block = nullptr;
    if (!rc) rc = cip_handle_alloc(h, &block, cip_handle_layout(nullptr, h, 0));      // ONE device allocation (poisoned under CIP_DEBUG_POISON)
    if (!rc) { cip_handle_layout(block, h, 0); rc = handle_fill(prob, h, true); }
    if (rc) { if (h) { free_all(h); delete h; } return rc; }
    *out = h;
    return 0;
}

// A planned handle: the host half of level 1 on `stream`, nothing on the device yet (cip_destroy takes it back as it is)
int cip_plan(const cip_problem *pr, hipStream_t stream, cip_handle **out) {
    *out = nullptr;
    cip_handle *h = new (std::nothrow) cip_handle();
    if (!h) { cip_set_error("out of host memory"); return CIP_E_INVALID; }
    h->stream = stream;
    const int rc = handle_plan(pr, h);
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}

// The device half for a handle of a lock-step group: carved out of `slab` (cap bytes; it belongs to the caller and outlives the
// handle) and filled without a host wait.
int cip_create_in_slab(cip_handle *h, const cip_problem *pr, char *slab, size_t cap, unsigned extras, const CipCsrCap *csr_cap) {
    const size_t bytes = cip_handle_layout(nullptr, h, extras, csr_cap);
    if (bytes > cap) { cip_set_error("lock-step batch: a handle of %zu bytes in a slab of %zu", bytes, cap); return CIP_E_UNSUPPORTED; }
    h->in_slab = true;
    cip_handle_layout(slab, h, extras, csr_cap);
    CIP_TRY(debug_poison(slab, bytes));
    return handle_fill(pr, h, false);
}

extern "C" int cip_create(int n, int m, int p, int ncones, const int *cone_type, const int *cone_dim, const double *Q,
                          const double *A, const double *G, int route, cip_handle **out) {
    cip_problem pr;
    memset(&pr, 0, sizeof(pr));
    pr.n = n; pr.m = m; pr.p = p; pr.ncones = ncones; pr.cone_type = cone_type; pr.cone_dim = cone_dim;
    pr.Q = Q; pr.ldq = n; pr.A = A; pr.lda = m; pr.G = G; pr.ldg = p; pr.route = route; pr.flags = 0;
    if (m > 0 && !A) { cip_set_error("A is NULL"); return CIP_E_INVALID; }
    return cip_create_ex(&pr, out);
}

// Level 1 again on an existing handle: new Q / A / G of the SAME shape (n, m, p, cones, route, dense-or-CSR A with the same
// number of non-zeros).  Keeps every allocation -- hipMalloc / hipFree synchronise the whole device, which is what a
// batch of small problems on several streams must avoid (csrc/batch.hip reuses one handle per worker this way).
extern "C" int cip_update_problem(cip_handle *h, const cip_problem *pr) {
    if (!h || !pr) { cip_set_error("NULL argument"); return CIP_E_INVALID; }
    if (pr->n != h->n || pr->m != h->m || pr->p != h->p || pr->ncones != h->ncones || pr->route != h->route ||
        (pr->A == NULL && pr->m > 0) != h->A_sparse) { cip_set_error("cip_update_problem: shape differs from the handle's"); return CIP_E_INVALID; }
    for (int c = 0; c < pr->ncones; ++c)
        if (pr->cone_type[c] != h->h_cones[c].type || pr->cone_dim[c] != h->h_cones[c].dim) { cip_set_error("cip_update_problem: cone %d differs", c); return CIP_E_INVALID; }
    if (((pr->flags & CIP_FLAG_Q_CSR) != 0) != h->Q_sparse) {
        cip_set_error("cip_update_problem: Q is %s, the handle was created with a %s Q", h->Q_sparse ? "dense" : "CSR", h->Q_sparse ? "CSR" : "dense");
        return CIP_E_INVALID;
    }
    if ((!h->Q_sparse && !pr->Q) || (h->p > 0 && !pr->G)) { cip_set_error("NULL matrix"); return CIP_E_INVALID; }
    if (h->Q_sparse) {
        // refused (other nnz, or the level-1 check fails) before anything of the handle's device state is touched: it stays usable
        if (h->staging_live) { CIP_HIP_CHECK(hipStreamSynchronize(h->stream)); h->staging_live = false; }
        int maxrow = 0;
        CIP_TRY(stage_Q_csr(h, pr, h->Q_nnz, &maxrow));
        h->Q_wave = q_wave_form(maxrow);
    }
    CIP_TRY(upload_problem(h, pr));
    h->assembled = h->factored = false;
    h->info_pending = false;
    h->reg_rel = 0.0; h->n_regularized = 0;          // a fresh problem starts unregularised, as a fresh handle does
    CIP_TRY(cip_cones_identity_scaling(h->stream, h->cs));
    return cip_sdp_scaling_changed(h->stream, h->cs);
}

extern "C" int cip_destroy(cip_handle *h) {
    if (!h) return 0;
    (void)hipStreamSynchronize(h->stream);
    free_all(h);
    delete h;
    return 0;
}

extern "C" int cip_set_stream(cip_handle *h, void *stream) {
    if (!h) return CIP_E_INVALID;
    CIP_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->stream = (hipStream_t)stream;
    h->graph_state = 0;              // graphs are decided per stream (no capture on the null stream); existing ones stay valid
    return 0;
}

// ------------------------------------------------------------------ level 2
extern "C" size_t cip_scaling_packed_len(const cip_handle *h) { return h ? h->cs.scal_len : 0; }

extern "C" int cip_set_scaling_packed(cip_handle *h, const double *packedF) {
    if (!h || !packedF) { cip_set_error("NULL argument"); return CIP_E_INVALID; }
    CIP_HIP_CHECK(hipMemcpyAsync(h->cs.d_scal, packedF, sizeof(double) * h->cs.scal_len, hipMemcpyHostToDevice, h->stream));
    CIP_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->assembled = h->factored = false;
    return cip_sdp_scaling_changed(h->stream, h->cs);
}
extern "C" int cip_get_scaling_packed(cip_handle *h, double *packedF) {
    if (!h || !packedF) { cip_set_error("NULL argument"); return CIP_E_INVALID; }
    CIP_HIP_CHECK(hipMemcpyAsync(packedF, h->cs.d_scal, sizeof(double) * h->cs.scal_len, hipMemcpyDeviceToHost, h->stream));
    CIP_HIP_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int cip_set_scaling_identity(cip_handle *h) {
    if (!h) return CIP_E_INVALID;
    h->assembled = h->factored = false;
    CIP_TRY(cip_cones_identity_scaling(h->stream, h->cs));
    return cip_sdp_scaling_changed(h->stream, h->cs);
}
extern "C" int cip_set_scaling_from_iterate_dev(cip_handle *h, const double *v, const double *s, double *lambda_out) {
    if (!h || (h->m > 0 && (!v || !s))) { cip_set_error("NULL argument"); return CIP_E_INVALID; }
    h->assembled = h->factored = false;
    CipRange rg("cip:scaling");
    return cip_cones_nt_scaling(h->stream, h->cs, v, s, lambda_out);
}

extern "C" int cip_assemble_only(cip_handle *h) {
    if (!h) return CIP_E_INVALID;
    return cip_assemble(h);
}

// ---- hipGraph replay of the LDL' factorisation / the triangular solves of SMALL systems (opt-in: CIP_GRAPH=1).  The
// launch sequence of a handle never changes (same pointers, same sizes), so it is recorded once as an explicit graph
// (cip_launch, cip_internal.h) and replayed: ~60 launches per factorisation and ~10-33 per solve become one graph launch.
// Built for config 5 (64 x n = 2048, 8 problems in flight) on the hypothesis that the batch is bound by the host's launch
// rate (95 k launches per pass).  It is not: 1936 KKT solves/s with graphs, 1995 without.  A kernel trace of a pass
// (profiles/r2/c5_*) shows 16.8 ms of serial kernel time per problem and an average of 3.4 kernels executing at once with
// 8 problems in flight (more hardware queues make it worse): the ceiling is the number of concurrently progressing
// launch-latency-bound streams, which only a lock-step batch (one launch for many problems) would lift.  Off by default
// (rocprofv3 also crashed on the graph path with several host threads).  graph_run (cip_handle.h) records and replays.
bool cip_graph_wanted(cip_handle *h) {
    if (h->graph_state == 0) {
        const int npmax = cip_env_int("CIP_GRAPH_NMAX", 4096);
        h->graph_state = (h->Npad <= npmax && cip_env_int("CIP_GRAPH", 0) == 1 && !h->timing && !h->ws.prof) ? 1 : -1;
    }
    return h->graph_state == 1;
}
thread_local CipGraphBuilder *cip_tl_builder = nullptr;

// the factorisation's four flag words -> host-mapped pinned memory, by a store from the device.  (Until round 5 a 16-byte
// hipMemcpyAsync: a blit kernel between two barriers -- in the kernel trace the main queue stood idle for 24 us between the last
// panel launch and the first solve's first kernel, of which the copy itself was 5.)
// No event behind it either (an event record is a barrier packet with a system-scope release: 11 us in the same trace): the fifth
// word is the factorisation's sequence number, stored with system-scope release behind the four flags; the host polls it.
__global__ void k_publish_info(const int *info, int *host, int seq) {
    if (threadIdx.x == 0) {
        host[0] = info[0]; host[1] = info[1]; host[2] = info[2]; host[3] = info[3];
        __hip_atomic_store(host + 4, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// The host's side of such a word (this kernel's, and k_lg_pubflag's of sdp_large_nt.hip): spin until it equals `seq`, yielding every
// 4096 polls and looking at the stream once then -- a failed launch must not hang the host.
int cip_await_seq(hipStream_t s, const volatile int *word, int seq, const char *what) {
    for (long spin = 0; __atomic_load_n(word, __ATOMIC_ACQUIRE) != seq; ++spin) {
        if ((spin & 0xfff) != 0xfff) continue;
        std::this_thread::yield();
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) {                                       // everything enqueued has run: the word must be there
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return 0;
            cip_set_error("%s never arrived", what);
            return CIP_E_HIP;
        }
        if (q != hipErrorNotReady) { cip_set_error("hipStreamQuery failed: %s", hipGetErrorString(q)); return CIP_E_HIP; }
    }
    return 0;
}
// has the flag read-back of factorisation `info_seq` landed?  wait: until it has
static int info_landed(cip_handle *h, bool wait, bool *landed) {
    *landed = __atomic_load_n((volatile int *)h->info_host + 4, __ATOMIC_ACQUIRE) == h->info_seq;
    if (*landed || !wait) return 0;
    char what[64];
    snprintf(what, sizeof(what), "LDL': the pivot flags of factorisation %d", h->info_seq);
    CIP_TRY(cip_await_seq(h->stream, h->info_host + 4, h->info_seq, what));
    *landed = true;
    return 0;
}
// assembly + LDL' + an asynchronous read-back of the pivot flag into pinned host memory; nothing here waits for the GPU
static int factor_enqueue(cip_handle *h) {
    { CipRange rg("cip:assemble"); CIP_TRY(cip_assemble(h, true)); }
    if (h->timing) CIP_HIP_CHECK(hipEventRecord(h->ev1, h->stream));
    {
        CipRange rg("cip:ldlt");
        // recorded under another lazy-copy state or chain form (a replay after a give-up must not run the fused chain again): record again
        if (h->gx_factor && (h->gx_factor_lazyC != h->ws.lazyC || h->gx_factor_unfused != h->ws.unfused)) {
            (void)hipGraphExecDestroy(h->gx_factor); h->gx_factor = nullptr;
        }
        h->gx_factor_lazyC = h->ws.lazyC;
        h->gx_factor_unfused = h->ws.unfused;
        bool replayed = false;
        CIP_TRY(graph_run(h, &h->gx_factor, [&]() {
            const int r = cip_ldlt_factor(h->stream, h->K, h->Npad, h->ldk, h->ws);
            if (cip_tl_builder) h->gx_factor_fused = cip_ldlt_last_factor_fused();
            return r;
        }, &replayed));
        // the give-up test hook of a replay decides from the chain the graph holds (a direct launch: cip_ldlt_factor has seen to it)
        if (replayed) CIP_TRY(cip_ldlt_debug_giveup(h->stream, h->K, h->Npad, h->ldk, h->ws, h->gx_factor_fused));
    }
    h->n_factor += 1;
    if (!h->info_host) {
        CIP_HIP_CHECK(hipHostMalloc((void **)&h->info_host, 8 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        memset(h->info_host, 0, 8 * sizeof(int));
    }
    {
        int *info_dev = nullptr;
        CIP_HIP_CHECK(hipHostGetDevicePointer((void **)&info_dev, h->info_host, 0));
        h->info_seq = (h->info_seq == 0x7fffffff) ? 1 : h->info_seq + 1;
        hipLaunchKernelGGL(k_publish_info, dim3(1), dim3(64), 0, h->stream, (const int *)h->ws.info, info_dev, h->info_seq);
        CIP_HIP_CHECK(hipGetLastError());
    }
    h->info_pending = true;
    h->spec_solves = 0;
    h->factored = true;
    return 0;
}

// enqueue the factorisation again and wait for its flags (after a give-up, or with the regularisation switched on).  A give-up of
// the fused chain in THIS factorisation is answered at once: the handle switches to the three-launch chain and redoes it.
static int refactor_and_wait(cip_handle *h) {
    for (;;) {
        CIP_TRY(factor_enqueue(h));
        { bool landed = false; CIP_TRY(info_landed(h, true, &landed)); }
        h->info_pending = false;
        if (h->info_host[3] == 0 || h->info_host[1] != 0 || h->ws.unfused) return 0;
        h->ws.unfused = 1;
        h->n_chain_fallbacks += 1;
    }
}
// the two verdicts on a factorisation that was (re)done.  The chain gave up for good (flag words [3] or [1], below): there is no factor
static int chain_gave_up(cip_handle *h) {
    if (h->info_host[3] == 0 && h->info_host[1] == 0) return 0;
    cip_set_error("LDL': in-launch wait of the panel chain gave up (%d)", h->info_host[3]);
    h->factored = false;
    return CIP_E_HIP;
}
// ... and the redone factor is good, but `spec` solves were enqueued on the one it replaces (`why` it was replaced)
static int solves_to_repeat(int spec, const char *why) {
    if (spec <= 0) return 0;
    cip_set_error("LDL': %d solve(s) were enqueued on a factorisation %s -- repeat them", spec, why);
    return CIP_E_RETRY;
}
// Resolve the pivot flag of the last factorisation.  wait = false: only if the read-back has already landed (no host
// wait; the caller goes ahead speculatively otherwise).  A zero / non-finite / wrong-sign pivot means [S G'; G 0] is not
// quasi-definite in the static order (typically an LP or a QP with singular Q and free variables: S is singular although
// the KKT matrix is not).  The reference's pivoting LU / QR does not care; the static-order LDL' switches to a
// regularised factorisation, once, for good -- and if that one fails too the error is reported (CIP_E_SINGULAR).
int cip_factor_resolve(cip_handle *h, bool wait) {
    if (!h->info_pending) return 0;
    bool landed = false;
    CIP_TRY(info_landed(h, wait, &landed));
    if (!landed) return 0;
    h->info_pending = false;
    // solves enqueued on the factorisation being resolved: if it is redone below, they ran on another factor -- repeat them
    const int spec = h->spec_solves;
    bool redone = false;
    // info_host: [0] first bad pivot of any kind (1-based column), [1] bail-out flag of the sweep kernels,
    //            [2] first zero / non-finite pivot, [3] an in-launch wait of the fused chain gave up
    if (h->info_host[3] != 0 && h->info_host[1] == 0 && !h->ws.unfused) {
        // An in-launch wait of the fused panel chain gave up.  Its waits are for workgroups of the same launch and end within
        // microseconds when the launch has the GPU's attention; on a GPU SHARED WITH OTHER PROCESSES the hardware scheduler can take
        // a launch's workgroups off the chip for longer than the bound (seen with eight processes on one MI355X: round 6).  The
        // three-launch chain has no in-launch wait and produces the same bits: this handle keeps it from now on, and the
        // factorisation is redone (assembly included: K holds a partial factor).  The redo's own pivot flags go through the
        // checks below like any factorisation's.
        h->ws.unfused = 1;
        h->n_chain_fallbacks += 1;
        CIP_TRY(refactor_and_wait(h));
        redone = true;
    }
    CIP_TRY(chain_gave_up(h));
    int info = h->info_host[0];
    if (info == 0 || (h->reg_rel > 0.0 && h->info_host[2] == 0)) {
        // (regularised factor: a wrong-sign pivot -- |d| ~ delta, rounding decides its sign -- is harmless, the refinement in
        //  solve3x3 works against the true operator; a zero / non-finite one is not)
        h->pivots_verified = true;
        return redone ? solves_to_repeat(spec, "whose panel chain gave up an in-launch wait; the handle has switched to the three-launch chain") : 0;
    }
    if (h->reg_rel > 0.0) {
        info = h->info_host[2];
    } else if (h->auto_reg) {
        h->reg_rel = cip_env_double("CIP_AUTO_REG", CIP_AUTO_REG);
        h->n_regularized += 1;
        CIP_TRY(refactor_and_wait(h));
        CIP_TRY(chain_gave_up(h));
        if (h->info_host[2] == 0) {
            h->pivots_verified = true;
            return solves_to_repeat(spec, "that met a bad pivot; the handle has switched to the regularised factorisation");
        }
        info = h->info_host[2];
    }
    h->factored = false;
    h->pivots_verified = false;      // keep waiting for the flag after a factorisation that failed
    cip_set_error("LDL': zero, non-finite or wrong-sign pivot at column %d%s", info,
                  h->reg_rel > 0.0 ? " (regularised factorisation)" : "");
    return CIP_E_SINGULAR;
}

extern "C" int cip_factor(cip_handle *h) {
    if (!h) return CIP_E_INVALID;
    if (h->timing) CIP_HIP_CHECK(hipEventRecord(h->ev0, h->stream));
    CIP_TRY(factor_enqueue(h));
    h->flops_ldlt = (double)h->N * h->N * h->N / 3.0;
    h->factored = true;
    if (h->timing) {
        // (timed factorisations include the solve preparation that otherwise runs beside the first solve)
        CIP_TRY(cip_ldlt_side_join(h->stream, h->ws, -1));
        CIP_HIP_CHECK(hipEventRecord(h->ev2, h->stream));
        CIP_HIP_CHECK(hipEventSynchronize(h->ev2));
        float a = 0, b = 0;
        CIP_HIP_CHECK(hipEventElapsedTime(&a, h->ev0, h->ev1));
        CIP_HIP_CHECK(hipEventElapsedTime(&b, h->ev1, h->ev2));
        h->ms_assemble = a; h->ms_ldlt = b;
        return cip_factor_resolve(h, true);
    }
    return 0;
}
extern "C" int cip_set_regularization(cip_handle *h, double rel, int automatic) {
    if (!h || !(rel >= 0.0)) { cip_set_error("cip_set_regularization: bad argument"); return CIP_E_INVALID; }
    h->reg_rel = rel;
    h->auto_reg = automatic != 0;
    h->pivots_verified = false;      // a different matrix is factored from now on: the next *_dev solve waits for its flag again
    return 0;
}
extern "C" int cip_get_regularization(cip_handle *h, double *rel, int *times_switched_on) {
    if (!h) return CIP_E_INVALID;
    if (rel) *rel = h->reg_rel;
    if (times_switched_on) *times_switched_on = h->n_regularized;
    return 0;
}

extern "C" int cip_check_factor(cip_handle *h) {
    if (!h) return CIP_E_INVALID;
    if (!h->factored) { cip_set_error("no factorisation"); return CIP_E_NOTFACTORED; }
    CIP_TRY(cip_factor_resolve(h, true));
    CIP_HIP_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ------------------------------------------------------------------ cone algebra / vector helpers
extern "C" int cip_apply_F_dev(cip_handle *h, int mode, const double *x, double *out) {
    if (!h || mode < 0 || mode > 3) { cip_set_error("bad argument"); return CIP_E_INVALID; }
    return cip_cones_apply(h->stream, h->cs, mode, x, out);
}
extern "C" int cip_cone_prod_dev(cip_handle *h, const double *x, const double *y, double *out) {
    if (!h) return CIP_E_INVALID;
    return cip_cones_prod(h->stream, h->cs, x, y, out);
}
extern "C" int cip_cone_div_dev(cip_handle *h, const double *x, const double *y, double *out) {
    if (!h) return CIP_E_INVALID;
    return cip_cones_div(h->stream, h->cs, x, y, out);
}
extern "C" int cip_maxstep_dev(cip_handle *h, const double *x, const double *d, double scale, double *alpha_host) {
    if (!h || !alpha_host) return CIP_E_INVALID;
    return cip_cones_maxstep(h->stream, h->cs, x, d, scale, alpha_host);
}
extern "C" int cip_maxstep_pair_dev(cip_handle *h, const double *x1, const double *d1, const double *x2, const double *d2, double scale,
                                    double *alpha_host2) {
    if (!h || !alpha_host2) return CIP_E_INVALID;
    return cip_cones_maxstep2(h->stream, h->cs, x1, d1, x2, d2, scale, alpha_host2);
}
extern "C" int cip_cone_identity_dev(cip_handle *h, double *e) {
    if (!h) return CIP_E_INVALID;
    return cip_cones_identity(h->stream, h->cs, e);
}

extern "C" int cip_gemv_dev(cip_handle *h, int which, int trans, double alpha, const double *x, double beta, double *y) {
    if (!h) return CIP_E_INVALID;
    hipStream_t s = h->stream;
    switch (which) {
        case CIP_MAT_Q: return cip_mul_Q(h, alpha, x, beta, y);                             // Q symmetric
        case CIP_MAT_A: return trans ? cip_mul_At(h, alpha, x, beta, y) : cip_mul_A(h, alpha, x, beta, y);
        case CIP_MAT_G:
            if (h->p == 0) {
                if (trans && beta == 0.0) return cip_zero(s, h->n, y);
                if (trans && beta != 1.0) return cip_axpby(s, h->n, 0.0, y, beta, y);
                return 0;
            }
            return trans ? cip_gemv_t(s, h->p, h->n, alpha, h->G, h->p, x, beta, y)
                         : cip_gemv_t(s, h->n, h->p, alpha, h->Gt, h->n, x, beta, y);
        default: cip_set_error("bad matrix id"); return CIP_E_INVALID;
    }
}
extern "C" int cip_dots_dev(cip_handle *h, int count, const double *const *x, const double *const *y, const int *len,
                            double *out_host) {
    if (!h) return CIP_E_INVALID;
    return cip_dots(h->stream, count, x, y, len, h->dot_scratch, out_host);
}
extern "C" int cip_axpby_dev(cip_handle *h, int len, double alpha, const double *x, double beta, double *y) {
    if (!h) return CIP_E_INVALID;
    return cip_axpby(h->stream, len, alpha, x, beta, y);
}

// ------------------------------------------------------------------ stand-alone LDL' / GEMM
extern "C" int cip_ldlt_workspace_bytes(int N, size_t *bytes) {
    if (N <= 0 || N % CIP_NB || !bytes) { cip_set_error("N must be a positive multiple of 128"); return CIP_E_INVALID; }
    *bytes = cip_ldlt_ws_bytes(N, -1);                  // room for the one-launch block steps whatever the mode is now or later
    return 0;
}
// N and ld multiples of 128 (cipkkt.h), checked here before anything is enqueued
static bool ldlt_dims_ok(const double *K, int N, int ld, const void *workspace) {
    return K && workspace && N > 0 && N % CIP_NB == 0 && ld >= N && ld % CIP_NB == 0;
}
extern "C" int cip_ldlt_factor_dev(void *stream, double *K, int N, int ld, void *workspace, int *info_host) {
    if (!ldlt_dims_ok(K, N, ld, workspace)) {
        cip_set_error("cip_ldlt_factor_dev: bad argument (K, workspace non-NULL; N > 0 and ld >= N multiples of 128)");
        return CIP_E_INVALID;
    }
    LdltWorkspace ws{};
    cip_ldlt_ws_carve(workspace, N, &ws, cip_ldlt_fused_for(N));      // (the workspace has room for either mode: cip_ldlt_workspace_bytes)
    CIP_TRY(cip_ldlt_factor((hipStream_t)stream, K, N, ld, ws));
    // all four flag words: [3] != 0 -- an in-launch wait of the fused chain gave up and K holds a partial factor
    int flags[4] = {0, 0, 0, 0};
    CIP_HIP_CHECK(hipMemcpyAsync(flags, ws.info, sizeof(flags), hipMemcpyDeviceToHost, (hipStream_t)stream));
    CIP_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (info_host) *info_host = flags[0];
    if (flags[3] != 0) {
        cip_set_error("cip_ldlt_factor_dev: an in-launch wait of the panel chain gave up (%d): K holds a partial factor -- supply K "
                      "again and repeat the call", flags[3]);
        return CIP_E_RETRY;
    }
    return 0;
}
extern "C" int cip_ldlt_solve_dev(void *stream, const double *K, int N, int ld, const void *workspace, double *rhs) {
    if (!ldlt_dims_ok(K, N, ld, workspace) || !rhs) {
        cip_set_error("cip_ldlt_solve_dev: bad argument (K, workspace, rhs non-NULL; N > 0 and ld >= N multiples of 128)");
        return CIP_E_INVALID;
    }
    LdltWorkspace ws{};
    cip_ldlt_ws_carve((void *)workspace, N, &ws, cip_ldlt_fused_for(N));   // same mode as at the factorisation: cip_set_solve_fused must not change between a factor and its solves
    return cip_ldlt_solve((hipStream_t)stream, K, N, ld, ws, rhs);
}
// scratch of cip_ldlt_solve_many_dev: the widest solve block any setting of the solve-block limit gives this order x min(nrhs, 64)
extern "C" int cip_ldlt_solve_many_scratch_bytes(int N, int nrhs, size_t *bytes) {
    if (N <= 0 || N % CIP_NB || nrhs < 0 || !bytes) { cip_set_error("N must be a positive multiple of 128, nrhs >= 0"); return CIP_E_INVALID; }
    *bytes = sizeof(double) * (size_t)cip_ldlt_solve_many_scratch_block(N) * (size_t)(nrhs < 64 ? nrhs : 64);
    return 0;
}
extern "C" int cip_ldlt_solve_many_dev(void *stream, const double *K, int N, int ld, const void *workspace, void *scratch, double *B,
                                       int ldb, int nrhs) {
    if (!ldlt_dims_ok(K, N, ld, workspace) || nrhs < 0 || ldb < N) {
        cip_set_error("cip_ldlt_solve_many_dev: bad argument (K, workspace non-NULL; N > 0 and ld >= N multiples of 128; nrhs >= 0; "
                      "ldb >= N)");
        return CIP_E_INVALID;
    }
    if (nrhs == 0) return 0;
    if (!B || !scratch) { cip_set_error("cip_ldlt_solve_many_dev: B and scratch must be non-NULL"); return CIP_E_INVALID; }
    LdltWorkspace ws{};
    cip_ldlt_ws_carve((void *)workspace, N, &ws, cip_ldlt_fused_for(N));
    return cip_ldlt_solve_many((hipStream_t)stream, K, N, ld, ws, (double *)scratch, B, ldb, nrhs, true);
}
extern "C" int cip_gemm_nt_dev(void *stream, int M, int N, int K, double alpha, const double *A, int lda, const double *B,
                               int ldb, double *C, int ldc, int lower_only) {
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || M % CIP_NB || N % CIP_NB || K % 16 || lda < M || ldb < N || ldc < M ||
        (lower_only && M != N)) {
        cip_set_error("cip_gemm_nt_dev: bad argument (A, B, C non-NULL; M, N > 0 multiples of 128, K > 0 a multiple of 16, "
                      "lda >= M, ldb >= N, ldc >= M; M == N with lower_only)");
        return CIP_E_INVALID;
    }
    if (lower_only) return cip_gemm_lower((hipStream_t)stream, M, K, alpha, A, lda, B, ldb, C, ldc);
    return cip_gemm_rect((hipStream_t)stream, M, N, K, alpha, A, lda, B, ldb, C, ldc);
}

// ------------------------------------------------------------------ introspection
extern "C" int cip_kkt_order(const cip_handle *h, int *N, int *N_padded) {
    if (!h) return CIP_E_INVALID;
    if (N) *N = h->N;
    if (N_padded) *N_padded = h->Npad;
    return 0;
}
extern "C" int cip_get_kkt_matrix(cip_handle *h, double *K_host) {
    if (!h || !K_host) return CIP_E_INVALID;
    CIP_TRY(cip_ldlt_side_join(h->stream, h->ws, -1));
    CIP_HIP_CHECK(hipStreamSynchronize(h->stream));
    CIP_HIP_CHECK(hipMemcpy(K_host, h->K, sizeof(double) * (size_t)h->ldk * h->Npad, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int cip_stats(cip_handle *h, double *out8) {
    if (!h || !out8) return CIP_E_INVALID;
    out8[0] = h->n_factor; out8[1] = h->n_solve; out8[2] = h->ms_assemble; out8[3] = h->ms_ldlt; out8[4] = h->flops_ldlt;
    out8[5] = cip_ldlt_outer_block_for(h->Npad); out8[6] = h->N; out8[7] = h->Npad;
    return 0;
}
extern "C" int cip_set_timing(cip_handle *h, int enabled) {
    if (!h) return CIP_E_INVALID;
    h->timing = enabled != 0;
    return 0;
}
// per-launch timing of the LDL' trailing-update kernel (HIP events on the handle's stream)
extern "C" int cip_profile_trailing(cip_handle *h, int enabled) {
    if (!h) return CIP_E_INVALID;
    if (enabled && !h->ws.prof) h->ws.prof = cip_ldlt_profile_create();
    if (enabled) cip_ldlt_profile_stride(h->ws.prof, enabled);      // enabled = k > 1: every k-th factorisation (the first one included)
    if (!enabled && h->ws.prof) { cip_ldlt_profile_destroy(h->ws.prof); h->ws.prof = nullptr; }
    return 0;
}
// out3 = [launches, total ms, total algorithmic flops] accumulated since profiling was enabled
extern "C" int cip_profile_get(cip_handle *h, double *out3) {
    if (!h || !out3 || !h->ws.prof) { cip_set_error("profiling not enabled"); return CIP_E_INVALID; }
    return cip_ldlt_profile_collect(h->ws.prof, &out3[0], &out3[1], &out3[2]);
}
// HIP-event timing of further dominant kernels on the calling thread (cip_conicip runs on the caller's thread):
// slot 0 = LDL' trailing update (== cip_profile_trailing_thread), 1 = Schur formation with a dense A, 2 = one-sided Jacobi of
// a large S cone's NT scaling.  out3 = [launches, total ms, total algorithmic flops (0 for the latency-bound Jacobi)]
extern "C" int cip_profile_kernel_thread(int slot, int enabled) {
    if (cip_prof_slot_enable(slot, enabled)) { cip_set_error("cip_profile_kernel_thread: no slot %d", slot); return CIP_E_INVALID; }
    return 0;
}
extern "C" int cip_profile_kernel_thread_get(int slot, double *out3) {
    if (!out3) return CIP_E_INVALID;
    if (cip_prof_slot_collect(slot, &out3[0], &out3[1], &out3[2])) { cip_set_error("slot %d: profiling not enabled", slot); return CIP_E_INVALID; }
    return 0;
}
// the calling thread's own trailing-update profile: covers factorisations of handles it does not hold (lock-step batches)
extern "C" int cip_profile_trailing_thread(int enabled) { return cip_ldlt_profile_thread(enabled); }
extern "C" int cip_profile_thread_get(double *out3) {
    if (!out3) return CIP_E_INVALID;
    if (cip_ldlt_profile_thread_collect(&out3[0], &out3[1], &out3[2])) { cip_set_error("thread profiling not enabled"); return CIP_E_INVALID; }
    return 0;
}
extern "C" int cip_set_lazy_copy(int on) { return cip_lazy_copy_set(on); }
extern "C" int cip_set_sdp_lanczos(int on) { return cip_sdp_large_lanczos(on); }
extern "C" int cip_debug_chain_giveup(int n) { return cip_debug_chain_giveup_set(n); }
extern "C" int cip_get_chain_fallbacks(cip_handle *h) { return h ? h->n_chain_fallbacks : -1; }
extern "C" int cip_sdp_lanczos_fallbacks(cip_handle *h, int *count) {
    if (!h || !count) { cip_set_error("bad argument"); return CIP_E_INVALID; }
    int out2[2] = {0, 0};
    const int rc = cip_sdp_large_cert_stats(h->stream, h->cs.lg, out2);
    *count = out2[0];
    return rc;
}
extern "C" int cip_set_ldlt_fused_chain(int on) { return cip_ldlt_set_fused_chain(on); }
extern "C" int cip_set_ldlt_side_prep(int on) { return cip_ldlt_set_side_prep(on); }
extern "C" int cip_set_solve_block_max(int b) { return cip_solve_block_max_set(b); }
extern "C" int cip_set_solve_fused(int mode) { return cip_solve_fused_set(mode); }
extern "C" int cip_set_ldlt_outer_block(int nbo) { cip_ldlt_set_outer_block(nbo); return cip_ldlt_outer_block(); }
