// The pre-solve's full-row-rank certificate on the device (gfx950): cip_rowrank_cert.
//
// M = [B_1 B_2 ...] has n rows; it certainly has n independent rows by the reference's criterion (every |R_ii| of the pivoted QR of
// (M / ||M||_F)' above eps, src/preprocessor.jl:19-23) when sigma_min(M) / ||M||_F >= thr = max(100 eps, 1e-6), i.e. when
// lambda_min(G) >= thr^2 ||M||_F^2 for the n x n Gram matrix G = sum B_i B_i'.  By Sylvester's law of inertia that holds exactly
// when the unpivoted LDL' of G - tau I has only positive pivots: no eigenvalue solver, only pieces the library has --
//
//   fro2     ||M||_F^2 as column sums of squares (k_rr_colsq) added up in order by one workgroup (k_rr_accum)
//   Gram     dense blocks through the fp64 MFMA lower-triangle GEMM (cip_gemm_lower), read in place when they meet its multiples,
//            otherwise staged in zero-padded column panels of RR_PANEL columns; CSR blocks by k_rr_gram_csr, one wave per row of G
//            walking CSR(B) and CSR(B'), stored entries only (the pattern of assemble.hip: k_schur_rows) -- no atomics, fixed order
//   shift    k_rr_shift: G_ii -= tau, identity on the padding.  tau = (thr^2 + 2 (L + n) 2^-53) fro2, L = all columns: the second
//            term bounds what rounding can add (DESIGN_LOG.md, "The full-row-rank certificate on the device"), so that a rounding
//            error can only turn "certified" into "not certified", never the other way round
//   factor   cip_ldlt_factor on the three-launch chain (no in-launch wait, hence no give-up to handle), the factor only
//   verdict  k_rr_verdict: the smallest pivot and a non-finite flag; certified = every pivot finite and > 0
//
// The call owns its device memory, works on the null stream and waits for its result, as cip_create_ex does.
#include "cip_internal.h"
#include "../../include/cipkkt.h"
#include <math.h>
#include <string.h>
#include <vector>

#define RR_PANEL 1024           // columns of a staging panel (a multiple of CIP_KT)
#define RR_CHUNK 4096           // CSR values enter fro2 as columns of this many entries
#define RR_MAXW 16

// sum over the workgroup, the same bits in every thread: wave sums, then the waves in order
__device__ __forceinline__ double rr_block_sum(double x, double *red) {
    x = cip_wave_sum(x);
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = red[0];
    for (int i = 1; i < nw; ++i) s += red[i];
    return s;
}

// part[c] = sum of squares of column c = blockIdx.x (rows entries, leading dimension ld)
__global__ __launch_bounds__(256) void k_rr_colsq(const double *P, int rows, long ld, double *part) {
    __shared__ double red[RR_MAXW];
    const double *a = P + (long)blockIdx.x * ld;
    double s = 0.0;
    for (int i = threadIdx.x; i < rows; i += 256) s = fma(a[i], a[i], s);
    s = rr_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// scal[0] += part[0] + ... + part[cnt - 1], one workgroup
__global__ __launch_bounds__(1024) void k_rr_accum(const double *part, int cnt, double *scal) {
    __shared__ double red[RR_MAXW];
    double s = 0.0;
    for (int c = threadIdx.x; c < cnt; c += 1024) s += part[c];
    s = rr_block_sum(s, red);
    if (threadIdx.x == 0) scal[0] += s;
}

// G[i, j] += sum_k B[i, k] B[j, k] for j <= i, B in CSR (rp, ci, v) with its transpose (trp, tci, tv; rows ascending).  One wave
// OWNS row i of the lower triangle: it takes the stored (i, k) one after the other and hands column k of B -- row k of B', distinct
// rows j -- to its lanes.  Entry (i, j) receives its additions in the order of row i's stored columns: the same bits on every run.  Two
// columns may hit the same (i, j) from different lanes: the accesses go to L2 and one column's stores are waited for before the next
// column's loads.
__global__ __launch_bounds__(256) void k_rr_gram_csr(int n, const int *rp, const int *ci, const double *v, const int *trp, const int *tci,
                                                      const double *tv, double *G, long ld) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double *Gi = G + i;
    const int q1 = rp[i + 1];
    for (int q = rp[i]; q < q1; ++q) {
        const int k = ci[q];
        const double a = v[q];
        const int b1 = trp[k + 1];
        for (int b = trp[k] + lane; b < b1; b += 64) {
            const int j = tci[b];
            if (j <= i) {
                double *gp = Gi + (long)j * ld;
                double x = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x = fma(a, tv[b], x);
                __hip_atomic_store(gp, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// G_ii -= tau (i < n); the padding's diagonal = 1 (its off-diagonal entries are the zeros the padded panels left)
__global__ __launch_bounds__(256) void k_rr_shift(double *G, long ld, int n, int N, double tau) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double *d = G + i + (long)i * ld;
    *d = i < n ? *d - tau : 1.0;
}

// out[0] = the smallest pivot d_i, i < n; out[1] = 1 when a pivot is not finite or the factorisation raised a flag of its own
__global__ __launch_bounds__(1024) void k_rr_verdict(const double *K, long ld, int n, const int *info, double *out) {
    __shared__ double mn[1024];
    __shared__ int bad[1024];
    double m = INFINITY;
    int b = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double d = K[i + (long)i * ld];
        if (!(fabs(d) < INFINITY)) b = 1;
        else if (d < m) m = d;
    }
    mn[threadIdx.x] = m; bad[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 1024; ++t) { if (mn[t] < m) m = mn[t]; b |= bad[t]; }
        if (info[0] != 0 || info[2] != 0 || info[3] != 0) b = 1;
        out[0] = m;
        out[1] = b ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
namespace {
struct RrCsr {                  // a CSR block on the host: B as handed over, and B' (rows ascending)
    std::vector<int> rp, ci, trp, tci;
    std::vector<double> v, tv;
};
struct RrDev {                  // every device allocation of the call: freed when the call returns, whichever way
    std::vector<void *> ptrs;
    ~RrDev() { for (void *p : ptrs) (void)hipFree(p); }
    template <typename T> int alloc(T **out, size_t count) {
        void *p = nullptr;
        CIP_HIP_CHECK(hipMalloc(&p, sizeof(T) * (count ? count : 1)));
        ptrs.push_back(p);
        *out = (T *)p;
        return 0;
    }
    template <typename T> int upload(T **out, const std::vector<T> &src, size_t count) {
        CIP_TRY(alloc(out, count));
        if (count) CIP_HIP_CHECK(hipMemcpyAsync(*out, src.data(), sizeof(T) * count, hipMemcpyHostToDevice, 0));
        return 0;
    }
};
}  // namespace

// A CSR block's level-1 check on the host, O(nnz): rowptr[0] == 0, a monotone row pointer, indices in [0, cols), no entry stored
// twice.  Device-resident arrays are copied back first, as A's and Q's are.  On success `c` holds B and B'.
static int rr_stage_csr(int bi, int n, const cip_cert_block &B, bool csr_dev, RrCsr &c) {
    c.rp.assign((size_t)n + 1, 0);
    if (csr_dev) CIP_HIP_CHECK(hipMemcpy(c.rp.data(), B.rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    else memcpy(c.rp.data(), B.rowptr, sizeof(int) * ((size_t)n + 1));
    if (c.rp[0] != 0) { cip_set_error("cip_rowrank_cert: block %d: rowptr[0] is %d, not 0", bi, c.rp[0]); return CIP_E_INVALID; }
    for (int i = 0; i < n; ++i)
        if (c.rp[i + 1] < c.rp[i]) {
            cip_set_error("cip_rowrank_cert: block %d: the row pointer decreases at row %d (%d after %d)", bi, i, c.rp[i + 1], c.rp[i]);
            return CIP_E_INVALID;
        }
    const size_t nnz = (size_t)c.rp[n];
    if (nnz > 0 && (!B.colind || !B.val)) { cip_set_error("cip_rowrank_cert: block %d: colind or val is NULL", bi); return CIP_E_INVALID; }
    c.ci.assign(nnz ? nnz : 1, 0); c.v.assign(nnz ? nnz : 1, 0.0);
    if (nnz > 0) {
        if (csr_dev) {
            CIP_HIP_CHECK(hipMemcpy(c.ci.data(), B.colind, sizeof(int) * nnz, hipMemcpyDeviceToHost));
            CIP_HIP_CHECK(hipMemcpy(c.v.data(), B.val, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        } else {
            memcpy(c.ci.data(), B.colind, sizeof(int) * nnz);
            memcpy(c.v.data(), B.val, sizeof(double) * nnz);
        }
    }
    std::vector<int> seen((size_t)B.cols, -1);                 // the last row that stored this column
    for (int i = 0; i < n; ++i)
        for (int q = c.rp[i]; q < c.rp[i + 1]; ++q) {
            const int k = c.ci[q];
            if (k < 0 || k >= B.cols) {
                cip_set_error("cip_rowrank_cert: block %d: entry %d of row %d has column index %d outside [0, %d)", bi, q - c.rp[i], i, k, B.cols);
                return CIP_E_INVALID;
            }
            if (seen[k] == i) { cip_set_error("cip_rowrank_cert: block %d: entry (%d, %d) is stored twice", bi, i, k); return CIP_E_INVALID; }
            seen[k] = i;
        }
    // B' by a counting sort: row k of B' lists the stored (j, k) with j ascending
    c.trp.assign((size_t)B.cols + 1, 0); c.tci.assign(nnz ? nnz : 1, 0); c.tv.assign(nnz ? nnz : 1, 0.0);
    for (size_t q = 0; q < nnz; ++q) c.trp[c.ci[q] + 1]++;
    for (int k = 0; k < B.cols; ++k) c.trp[k + 1] += c.trp[k];
    std::vector<int> fill(c.trp.begin(), c.trp.end() - 1);
    for (int i = 0; i < n; ++i)
        for (int q = c.rp[i]; q < c.rp[i + 1]; ++q) { const int d = fill[c.ci[q]]++; c.tci[d] = i; c.tv[d] = c.v[q]; }
    return 0;
}

// scal[0] += the squares of a rows x cols block, column by column, RR_PANEL columns per launch pair
static int rr_sumsq(const double *P, int rows, long cols, long ld, double *part, double *scal) {
    for (long c0 = 0; c0 < cols; c0 += RR_PANEL) {
        const int w = (int)(cols - c0 < RR_PANEL ? cols - c0 : RR_PANEL);
        hipLaunchKernelGGL(k_rr_colsq, dim3((unsigned)w), dim3(256), 0, 0, P + c0 * ld, rows, ld, part);
        hipLaunchKernelGGL(k_rr_accum, dim3(1), dim3(1024), 0, 0, (const double *)part, w, scal);
    }
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// can cip_gemm_lower read this device block where it lies? (128 rows, 16 in k, 16-byte accesses along a column)
static bool rr_in_place(int n, const cip_cert_block &B) {
    return n % CIP_NB == 0 && B.cols % CIP_KT == 0 && B.ld % 2 == 0 && B.ld < (1 << 26) && ((uintptr_t)B.dense & 15) == 0;
}

static int rr_run(int n, int nblocks, const cip_cert_block *blocks, const std::vector<RrCsr> &csr, bool dense_dev, long Ltot, double eps,
                  int *certified, double *fro2_out, double *shift_out) {
    RrDev dev;
    const int N = (n + CIP_NB - 1) / CIP_NB * CIP_NB;
    int stage_cols = 0;                                          // the widest padded panel any block needs
    for (int b = 0; b < nblocks; ++b) {
        const cip_cert_block &B = blocks[b];
        if (B.cols <= 0 || !B.dense || (dense_dev && rr_in_place(n, B))) continue;
        const int w = B.cols < RR_PANEL ? (B.cols + CIP_KT - 1) / CIP_KT * CIP_KT : RR_PANEL;
        if (w > stage_cols) stage_cols = w;
    }
    double *G = nullptr, *scal = nullptr, *part = nullptr, *stage = nullptr;
    char *wsbase = nullptr;
    CIP_TRY(dev.alloc(&G, (size_t)N * N));
    CIP_TRY(dev.alloc(&scal, 8));
    CIP_TRY(dev.alloc(&part, RR_PANEL));
    if (stage_cols) CIP_TRY(dev.alloc(&stage, (size_t)N * stage_cols));
    CIP_TRY(dev.alloc(&wsbase, cip_ldlt_ws_bytes(N, 0)));
    CIP_HIP_CHECK(hipMemsetAsync(G, 0, sizeof(double) * (size_t)N * N, 0));
    CIP_HIP_CHECK(hipMemsetAsync(scal, 0, sizeof(double) * 8, 0));
    if (stage_cols) CIP_HIP_CHECK(hipMemsetAsync(stage, 0, sizeof(double) * (size_t)N * stage_cols, 0));   // rows n.. stay zero throughout

    for (int b = 0; b < nblocks; ++b) {
        const cip_cert_block &B = blocks[b];
        if (B.cols <= 0) continue;
        if (B.dense && dense_dev && rr_in_place(n, B)) {
            CIP_TRY(rr_sumsq(B.dense, n, B.cols, B.ld, part, scal));
            CIP_TRY(cip_gemm_lower(0, N, B.cols, 1.0, B.dense, B.ld, B.dense, B.ld, G, N));
        } else if (B.dense) {
            for (long c0 = 0; c0 < B.cols; c0 += RR_PANEL) {
                const int w = (int)(B.cols - c0 < RR_PANEL ? B.cols - c0 : RR_PANEL), wp = (w + CIP_KT - 1) / CIP_KT * CIP_KT;
                if (wp > w) CIP_HIP_CHECK(hipMemsetAsync(stage + (size_t)w * N, 0, sizeof(double) * (size_t)(wp - w) * N, 0));
                CIP_HIP_CHECK(hipMemcpy2DAsync(stage, sizeof(double) * (size_t)N, B.dense + c0 * (long)B.ld, sizeof(double) * (size_t)B.ld,
                                               sizeof(double) * (size_t)n, (size_t)w, dense_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, 0));
                CIP_TRY(rr_sumsq(stage, n, w, N, part, scal));
                CIP_TRY(cip_gemm_lower(0, N, wp, 1.0, stage, N, stage, N, G, N));
            }
        } else {
            const RrCsr &c = csr[b];
            const size_t nnz = (size_t)c.rp[n];
            if (nnz == 0) continue;
            int *rp, *ci, *trp, *tci;
            double *v, *tv;
            CIP_TRY(dev.upload(&rp, c.rp, (size_t)n + 1)); CIP_TRY(dev.upload(&ci, c.ci, nnz)); CIP_TRY(dev.upload(&v, c.v, nnz));
            CIP_TRY(dev.upload(&trp, c.trp, (size_t)B.cols + 1)); CIP_TRY(dev.upload(&tci, c.tci, nnz)); CIP_TRY(dev.upload(&tv, c.tv, nnz));
            const long full = (long)(nnz / RR_CHUNK), rest = (long)(nnz % RR_CHUNK);
            CIP_TRY(rr_sumsq(v, RR_CHUNK, full, RR_CHUNK, part, scal));
            if (rest) CIP_TRY(rr_sumsq(v + full * RR_CHUNK, (int)rest, 1, rest, part, scal));
            hipLaunchKernelGGL(k_rr_gram_csr, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, n, (const int *)rp, (const int *)ci, (const double *)v,
                               (const int *)trp, (const int *)tci, (const double *)tv, G, (long)N);
            CIP_HIP_CHECK(hipGetLastError());
        }
    }
    double fro2 = 0.0;
    CIP_HIP_CHECK(hipMemcpyAsync(&fro2, scal, sizeof(double), hipMemcpyDeviceToHost, 0));
    CIP_HIP_CHECK(hipStreamSynchronize(0));
    if (!(fro2 < INFINITY)) { cip_set_error("cip_rowrank_cert: non-finite entry"); return CIP_E_INVALID; }
    if (fro2_out) *fro2_out = fro2;
    if (fro2 == 0.0) return 0;                                   // an all-zero M: not certified

    const double thr = 100.0 * eps > 1e-6 ? 100.0 * eps : 1e-6;
    const double thr2 = thr * thr, slack = 2.0 * (double)(Ltot + n) * 0x1p-53;       // (statements of their own: nothing contracts into an fma)
    const double tau = (thr2 + slack) * fro2;
    if (shift_out) *shift_out = tau;
    hipLaunchKernelGGL(k_rr_shift, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, G, (long)N, n, N, tau);
    CIP_HIP_CHECK(hipGetLastError());
    LdltWorkspace ws{};
    cip_ldlt_ws_carve(wsbase, N, &ws, 0);
    ws.no_prep = 1;                                              // the factor only: nobody solves with it
    ws.unfused = 1;                                              // three launches per panel: no in-launch wait, no give-up
    CIP_TRY(cip_ldlt_factor(0, G, N, N, ws));
    hipLaunchKernelGGL(k_rr_verdict, dim3(1), dim3(1024), 0, 0, (const double *)G, (long)N, n, (const int *)ws.info, scal + 2);
    CIP_HIP_CHECK(hipGetLastError());
    double out[2] = {0.0, 1.0};
    CIP_HIP_CHECK(hipMemcpyAsync(out, scal + 2, sizeof(out), hipMemcpyDeviceToHost, 0));
    CIP_HIP_CHECK(hipStreamSynchronize(0));
    *certified = (out[1] == 0.0 && out[0] > 0.0) ? 1 : 0;
    return 0;
}

extern "C" int cip_rowrank_cert(int n, int nblocks, const cip_cert_block *blocks, double eps, int flags, int *certified, double *fro2,
                                double *shift) {
    // ---- argument rules: nothing is allocated on the device before they all hold
    if (n < 0 || nblocks < 0) { cip_set_error("cip_rowrank_cert: n = %d, nblocks = %d must be >= 0", n, nblocks); return CIP_E_INVALID; }
    if (!(eps >= 0.0) || !(eps < INFINITY)) { cip_set_error("cip_rowrank_cert: eps must be finite and >= 0"); return CIP_E_INVALID; }
    if (!certified) { cip_set_error("cip_rowrank_cert: certified is NULL"); return CIP_E_INVALID; }
    if (nblocks > 0 && !blocks) { cip_set_error("cip_rowrank_cert: blocks is NULL"); return CIP_E_INVALID; }
    long Ltot = 0;
    for (int b = 0; b < nblocks; ++b) {
        const cip_cert_block &B = blocks[b];
        if (B.cols < 0) { cip_set_error("cip_rowrank_cert: block %d: cols = %d must be >= 0", b, B.cols); return CIP_E_INVALID; }
        Ltot += B.cols;
        if (B.cols == 0 || n == 0) continue;
        const bool csr_any = B.rowptr || B.colind || B.val;
        if (B.dense && csr_any) { cip_set_error("cip_rowrank_cert: block %d: both a dense pointer and CSR arrays are given", b); return CIP_E_INVALID; }
        if (!B.dense && !B.rowptr) { cip_set_error("cip_rowrank_cert: block %d: neither a dense pointer nor a CSR row pointer is given", b); return CIP_E_INVALID; }
        if (B.dense && B.ld < n) { cip_set_error("cip_rowrank_cert: block %d: ld = %d is below n = %d", b, B.ld, n); return CIP_E_INVALID; }
    }
    const auto nothing_certified = [&] { *certified = 0; if (fro2) *fro2 = 0.0; if (shift) *shift = 0.0; };
    if (n == 0 || Ltot == 0) { nothing_certified(); return 0; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        cip_set_error("no HIP device available (libcipkkt has no CPU fallback)");
        return CIP_E_NODEVICE;
    }
    if (cip_kernels_init()) return CIP_E_HIP;
    const bool dense_dev = (flags & CIP_FLAG_DEVICE_PTRS) != 0;
    const bool csr_dev = dense_dev && !(flags & CIP_FLAG_CSR_HOST);
    std::vector<RrCsr> csr((size_t)nblocks);
    for (int b = 0; b < nblocks; ++b)
        if (blocks[b].cols > 0 && !blocks[b].dense) CIP_TRY(rr_stage_csr(b, n, blocks[b], csr_dev, csr[b]));
    nothing_certified();                                         // (a refused call has written nothing)
    return rr_run(n, nblocks, blocks, csr, dense_dev, Ltot, eps, certified, fro2, shift);
}
