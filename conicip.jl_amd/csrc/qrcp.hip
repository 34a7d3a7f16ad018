// Rank-revealing (column-pivoted) Householder QR on the device, and the reference's `imcols` (src/preprocessor.jl:10-28) on top
// of it (gfx950).
//
// M is len x cnt, column-major, leading dimension ld; the result has LAPACK geqp3's layout (columns physically permuted, R on and
// above the diagonal, the reflector tails -- leading 1 implicit -- below it in the first k columns, tau, 0-based pivots).  The form is
// the unblocked one: per step, two passes over the trailing matrix.  That is HBM-bound work, it is needed once per problem, and it
// is two launches per step:
//
//   k_qr_pivot   ONE workgroup: picks the column with the largest remaining norm (lowest index on ties), recomputes that column's
//                norm from the column itself, stops when it is <= stop, otherwise swaps it into place and forms the reflector
//                (beta = -sign(x0) ||x||, tau = (beta - x0) / beta, tail scaled by 1 / (x0 - beta); a zero tail gives tau = 0).
//   k_qr_update  one workgroup per trailing column: reads the column ONCE into registers (up to 24 doubles per lane at 1024 lanes:
//                24576 rows), w = v'a, a -= tau w v, writes it back and sums, in the same pass, the squares of what is left below the
//                new row.  Every step's pivot norms are therefore freshly computed: no down-dating, no cancellation safeguard.
//                Longer columns take a looped two-read form.  v is read by every workgroup (L2 / Infinity Cache).
//
// No workgroup waits for another inside a launch, nothing is accumulated with atomics, every sum is a wave sum (DPP / permlane,
// cip_wave_sum) followed by the waves in order: the same input gives the same bits.  The squares are summed unscaled: entries whose
// squares overflow count as non-finite, and a column below 1e-154 counts as zero (imcols normalises by ||A||_F first).
//
// Early stop: the steps are enqueued in chunks; a step that finds the largest norm <= stop sets a device flag that turns every later
// launch into a no-op, and the host reads {done, k, status} back after each chunk (a copy and a stream synchronisation, never a
// spin on device memory).
#include "cip_internal.h"
#include "../../include/cipkkt.h"
#include <math.h>
#include <algorithm>

#define QR_MAXW 16              // waves of the largest workgroup
#define QR_FLAGS 16             // ints at the head of the workspace: [0] done, [1] k (steps finished), [2] status (1: non-finite)

// sum over the workgroup, the same bits in every thread: wave sums, then the waves in order.  Two calls in a row need two different
// `red` arrays (the barrier sits between the store and the loads).
__device__ __forceinline__ double qr_block_sum(double x, double *red) {
    x = cip_wave_sum(x);
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = red[0];
    for (int i = 1; i < nw; ++i) s += red[i];
    return s;
}

// norms[c] = sum of squares of column c, piv[c] = c (piv == NULL: norms only)
__global__ __launch_bounds__(256) void k_qr_init(const double *M, int len, long ld, double *norms, int *piv) {
    __shared__ double red[QR_MAXW];
    const int c = blockIdx.x;
    const double *a = M + (long)c * ld;
    double s = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) s += a[i] * a[i];
    s = qr_block_sum(s, red);
    if (threadIdx.x == 0) {
        norms[c] = s;
        if (piv) piv[c] = c;
    }
}

__global__ __launch_bounds__(1024) void k_qr_pivot(double *M, int len, int cnt, long ld, int j, double stop, double *norms, int *piv,
                                                   double *tau, double *rdiag, int *flags) {
    __shared__ double red[QR_MAXW], bval[QR_MAXW];
    __shared__ int bidx[QR_MAXW];
    if (flags[0]) return;                                   // (read by every thread before the first barrier; written after it)
    const int tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    // the largest remaining norm, lowest index on ties; a NaN counts as +inf
    double bv = -1.0;
    int bi = cnt;
    for (int c = j + tid; c < cnt; c += nt) {
        double v = norms[c];
        if (!(v == v)) v = INFINITY;
        if (v > bv) { bv = v; bi = c; }
    }
    for (int off = 32; off; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { bval[tid >> 6] = bv; bidx[tid >> 6] = bi; }
    __syncthreads();
    bv = bval[0]; bi = bidx[0];
    for (int w = 1; w < nw; ++w)
        if (bval[w] > bv || (bval[w] == bv && bidx[w] < bi)) { bv = bval[w]; bi = bidx[w]; }
    if (!(bv < INFINITY)) {                                 // non-finite entry
        if (tid == 0) { flags[2] = 1; flags[0] = 1; }
        return;
    }
    // the pivot column's norm, from the column itself
    double *cj = M + (long)j * ld, *cp = M + (long)bi * ld;
    const double x0 = cp[j];
    double ss = 0.0;
    for (int i = j + 1 + tid; i < len; i += nt) ss += cp[i] * cp[i];
    ss = qr_block_sum(ss, red);
    const double nrm = ss == 0.0 ? fabs(x0) : sqrt(x0 * x0 + ss);
    if (nrm <= stop) {                                      // every later |R_jj| would be <= stop: finished with k = j
        if (tid == 0) flags[0] = 1;
        return;
    }
    double beta = x0, t = 0.0, scale = 0.0;
    if (ss != 0.0) {
        beta = -copysign(nrm, x0);
        t = (beta - x0) / beta;
        scale = 1.0 / (x0 - beta);
    }
    // swap the two columns (all rows: R's rows above are permuted with them) and scale the reflector's tail
    for (int i = tid; i < len; i += nt) {
        const double b = cp[i];
        if (bi != j) cp[i] = cj[i];
        cj[i] = i > j ? b * scale : (i == j ? beta : b);
    }
    if (tid == 0) {
        if (bi != j) {
            norms[bi] = norms[j];
            const int pj = piv[j];
            piv[j] = piv[bi];
            piv[bi] = pj;
        }
        tau[j] = t;
        rdiag[j] = beta;
        flags[1] = j + 1;
    }
}

// One trailing column c = j + 1 + blockIdx.x per workgroup, NV pairs of rows per lane in registers: lane t holds the rows
// r0 + 2 (t + q * lanes) and the one after it, q < NV, r0 = the even row at or just above j.  VEC: the pairs move as 16-byte
// accesses (ld even, M 16-byte aligned); otherwise as two 8-byte ones -- the same rows in the same lanes, so the same bits.  The
// element in front of row j, if any, is written back unchanged.
template <int NV, bool VEC>
__global__ __launch_bounds__(1024) void k_qr_update(double *M, int len, long ld, int j, const double *tau, double *norms,
                                                    const int *flags) {
    __shared__ double red0[QR_MAXW], red1[QR_MAXW];
    if (flags[0]) return;
    const int tid = threadIdx.x, nt = blockDim.x, c = j + 1 + blockIdx.x;
    const double *v = M + (long)j * ld;
    double *a = M + (long)c * ld;
    const double t = tau[j];
    const int r0 = j & ~1;
    double A0[NV], A1[NV];
    double w = 0.0, ns = 0.0;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int r = r0 + 2 * (tid + q * nt);
        double v0 = 0.0, v1 = 0.0;
        A0[q] = 0.0; A1[q] = 0.0;
        if (VEC && r + 1 < len) {
            const v2d x = *(const v2d *)(a + r), u = *(const v2d *)(v + r);
            A0[q] = x[0]; A1[q] = x[1]; v0 = u[0]; v1 = u[1];
        } else {
            if (r < len) { A0[q] = a[r]; v0 = v[r]; }
            if (r + 1 < len) { A1[q] = a[r + 1]; v1 = v[r + 1]; }
        }
        if (r <= j) v0 = r == j ? 1.0 : 0.0;
        if (r + 1 <= j) v1 = r + 1 == j ? 1.0 : 0.0;
        w = fma(A1[q], v1, fma(A0[q], v0, w));               // (explicit: both access widths must contract alike)
    }
    w = qr_block_sum(w, red0);
    const double tw = t * w;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int r = r0 + 2 * (tid + q * nt);
        double v0 = 0.0, v1 = 0.0;
        if (VEC && r + 1 < len) {
            const v2d u = *(const v2d *)(v + r);
            v0 = u[0]; v1 = u[1];
        } else {
            if (r < len) v0 = v[r];
            if (r + 1 < len) v1 = v[r + 1];
        }
        if (r == j) v0 = 1.0;
        if (r + 1 == j) v1 = 1.0;
        if (r >= j) A0[q] = fma(-tw, v0, A0[q]);
        if (r + 1 >= j) A1[q] = fma(-tw, v1, A1[q]);
        if (r > j) ns = fma(A0[q], A0[q], ns);
        if (r + 1 > j) ns = fma(A1[q], A1[q], ns);           // (rows >= len hold zeros)
        if (VEC && r + 1 < len) {
            *(v2d *)(a + r) = v2d{A0[q], A1[q]};
        } else {
            if (r < len) a[r] = A0[q];
            if (r + 1 < len) a[r + 1] = A1[q];
        }
    }
    ns = qr_block_sum(ns, red1);
    if (tid == 0) norms[c] = ns;
}

// the same for columns longer than the register tile holds: the column is read twice
__global__ __launch_bounds__(1024) void k_qr_update_loop(double *M, int len, long ld, int j, const double *tau, double *norms,
                                                         const int *flags) {
    __shared__ double red0[QR_MAXW], red1[QR_MAXW];
    if (flags[0]) return;
    const int tid = threadIdx.x, nt = blockDim.x, c = j + 1 + blockIdx.x;
    const double *v = M + (long)j * ld;
    double *a = M + (long)c * ld;
    const double t = tau[j];
    double w = tid == 0 ? a[j] : 0.0, ns = 0.0;
    for (int r = j + 1 + tid; r < len; r += nt) w += a[r] * v[r];
    w = qr_block_sum(w, red0);
    const double tw = t * w;
    if (tid == 0) a[j] -= tw;
    for (int r = j + 1 + tid; r < len; r += nt) {
        const double x = a[r] - tw * v[r];
        ns += x * x;
        a[r] = x;
    }
    ns = qr_block_sum(ns, red1);
    if (tid == 0) norms[c] = ns;
}

#define QR_TILE_ROWS 24576      // rows the largest register tile holds (1024 lanes x 24 doubles); beyond: the looped form

template <int NV>
static void qr_update_tile(hipStream_t s, int threads, bool vec, unsigned grid, double *M, int len, long ld, int j, const double *tau,
                           double *norms, const int *flags) {
    if (vec) hipLaunchKernelGGL((k_qr_update<NV, true>), dim3(grid), dim3(threads), 0, s, M, len, ld, j, tau, norms, flags);
    else hipLaunchKernelGGL((k_qr_update<NV, false>), dim3(grid), dim3(threads), 0, s, M, len, ld, j, tau, norms, flags);
}
static void qr_launch_update(hipStream_t s, bool vec, double *M, int len, int cnt, long ld, int j, const double *tau, double *norms,
                             const int *flags) {
    const unsigned grid = (unsigned)(cnt - j - 1);
    const int rows = len - (j & ~1);                        // rows a workgroup holds, from the even row (either access width)
    if (rows <= 512) qr_update_tile<1>(s, 256, vec, grid, M, len, ld, j, tau, norms, flags);
    else if (rows <= 2048) qr_update_tile<4>(s, 256, vec, grid, M, len, ld, j, tau, norms, flags);
    else if (rows <= 4096) qr_update_tile<2>(s, 1024, vec, grid, M, len, ld, j, tau, norms, flags);
    else if (rows <= 8192) qr_update_tile<4>(s, 1024, vec, grid, M, len, ld, j, tau, norms, flags);
    else if (rows <= QR_TILE_ROWS) qr_update_tile<12>(s, 1024, vec, grid, M, len, ld, j, tau, norms, flags);
    else hipLaunchKernelGGL(k_qr_update_loop, dim3(grid), dim3(1024), 0, s, M, len, ld, j, tau, norms, flags);
}

// ------------------------------------------------------------------------------------------------------------ workspace
struct QrWs {
    int *flags;                 // QR_FLAGS ints
    double *norms;              // cnt
    double *tau, *rdiag;        // min(len, cnt) each
    int *piv;                   // cnt
};
static size_t qr_ws_layout(CipLayout L, int len, int cnt, QrWs *w) {
    const size_t k = (size_t)(len < cnt ? len : cnt);
    w->flags = L.take<int>(QR_FLAGS);
    w->norms = L.take<double>(cnt);
    w->tau = L.take<double>(k); w->rdiag = L.take<double>(k);
    w->piv = L.take<int>(cnt);
    return L.bytes();
}

// The factorisation (len, cnt > 0).  tau: device, min(len, cnt) entries.  *k = steps done; *status != 0: non-finite entry.
static int qr_run(hipStream_t s, double *M, int len, int cnt, long ld, double stop, const QrWs &w, double *tau, int *k, int *status) {
    const int kmax = len < cnt ? len : cnt;
    const bool vec = ld % 2 == 0 && ((uintptr_t)M & 15) == 0;
    const int pthreads = (len > 4096 || cnt > 4096) ? 1024 : 256;
    int fl[4] = {0, 0, 0, 0};
    CIP_HIP_CHECK(hipMemsetAsync(w.flags, 0, sizeof(int) * QR_FLAGS, s));
    hipLaunchKernelGGL(k_qr_init, dim3((unsigned)cnt), dim3(256), 0, s, (const double *)M, len, ld, w.norms, w.piv);
    // chunks of steps, doubling from 32 to 512: a small rank costs few idle launches, a large one few round trips
    for (int j0 = 0, chunk = 32; j0 < kmax && !fl[0]; j0 += chunk, chunk = chunk < 512 ? 2 * chunk : 512) {
        const int j1 = j0 + chunk < kmax ? j0 + chunk : kmax;
        for (int j = j0; j < j1; ++j) {
            hipLaunchKernelGGL(k_qr_pivot, dim3(1), dim3(pthreads), 0, s, M, len, cnt, ld, j, stop, w.norms, w.piv, tau, w.rdiag, w.flags);
            if (j + 1 < cnt) qr_launch_update(s, vec, M, len, cnt, ld, j, tau, w.norms, w.flags);
        }
        CIP_HIP_CHECK(hipGetLastError());
        CIP_HIP_CHECK(hipMemcpyAsync(fl, w.flags, sizeof(fl), hipMemcpyDeviceToHost, s));
        CIP_HIP_CHECK(hipStreamSynchronize(s));
    }
    *k = fl[1];
    *status = fl[2];
    return 0;
}

static bool qr_dims_ok(int len, int cnt, int ld) { return len >= 0 && cnt >= 0 && ld >= (len > 1 ? len : 1); }

extern "C" int cip_qrcp_workspace_bytes(int len, int cnt, size_t *bytes) {
    if (len < 0 || cnt < 0 || !bytes) { cip_set_error("cip_qrcp_workspace_bytes: len, cnt >= 0 and bytes non-NULL"); return CIP_E_INVALID; }
    QrWs w;
    *bytes = qr_ws_layout(nullptr, len, cnt, &w);
    return 0;
}

extern "C" int cip_qrcp_dev(void *stream, double *M, int len, int cnt, int ld, double stop, void *workspace, double *tau_dev,
                            int *piv_host, double *rdiag_host, int *k_host) {
    const bool empty = len == 0 || cnt == 0;
    if (!qr_dims_ok(len, cnt, ld) || !(stop >= 0.0) || !(stop < INFINITY) || !k_host || (!empty && (!M || !workspace))) {
        cip_set_error("cip_qrcp_dev: bad argument (len, cnt >= 0; ld >= max(len, 1); stop >= 0 and finite; k_host non-NULL; M, workspace "
                      "non-NULL when len * cnt > 0)");
        return CIP_E_INVALID;
    }
    *k_host = 0;
    if (empty) {
        if (piv_host) for (int c = 0; c < cnt; ++c) piv_host[c] = c;
        return 0;
    }
    hipStream_t s = (hipStream_t)stream;
    QrWs w;
    qr_ws_layout(workspace, len, cnt, &w);
    int k = 0, status = 0;
    const int rc = qr_run(s, M, len, cnt, ld, stop, w, tau_dev ? tau_dev : w.tau, &k, &status);
    if (rc) return rc;
    if (status) { cip_set_error("cip_qrcp_dev: non-finite entry"); return CIP_E_INVALID; }
    if (piv_host) CIP_HIP_CHECK(hipMemcpyAsync(piv_host, w.piv, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, s));
    if (rdiag_host && k > 0) CIP_HIP_CHECK(hipMemcpyAsync(rdiag_host, w.rdiag, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
    CIP_HIP_CHECK(hipStreamSynchronize(s));
    *k_host = k;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ imcols
// scal[0] = sqrt(sum of the column sums of squares), in order
__global__ __launch_bounds__(1024) void k_im_fro(const double *norms, int cnt, double *scal) {
    __shared__ double red[QR_MAXW];
    double s = 0.0;
    for (int c = threadIdx.x; c < cnt; c += 1024) s += norms[c];
    s = qr_block_sum(s, red);
    if (threadIdx.x == 0) scal[0] = sqrt(s);
}
// W = M / fro (column blockIdx.x), bs = b / fro
__global__ __launch_bounds__(256) void k_im_scale(const double *M, int len, long ld, double *W, long ldw, const double *b, double *bs,
                                                  double fro) {
    const int c = blockIdx.x;
    const double *a = M + (long)c * ld;
    double *o = W + (long)c * ldw;
    for (int i = threadIdx.x; i < len; i += 256) o[i] = a[i] / fro;
    if (threadIdx.x == 0) bs[c] = b[c] / fro;
}
__global__ __launch_bounds__(256) void k_im_gather(const double *src, const int *piv, int r, double *dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < r) dst[i] = src[piv[i]];
}
// R1' y = y in place, R1 = the leading r x r triangle of W: y_i = (y_i - sum_{l < i} R[l, i] y_l) / R[i, i], the sums along the
// (contiguous) columns of R1.  One workgroup; thread t owns the entries l = t (mod 1024) of y and is the only one to touch them.
__global__ __launch_bounds__(1024) void k_im_fwd(const double *W, long ldw, int r, double *y) {
    __shared__ double red[2][QR_MAXW];
    const int tid = threadIdx.x;
    for (int i = 0; i < r; ++i) {
        const double *col = W + (long)i * ldw;
        double s = 0.0;
        for (int l = tid; l < i; l += 1024) s += col[l] * y[l];
        s = qr_block_sum(s, red[i & 1]);
        if (tid == (i & 1023)) y[i] = (y[i] - s) / col[i];
    }
}
// z = H_0 H_1 ... H_{r-1} [y; 0] (the reflectors in reverse order), x = z or x += z.  One workgroup; thread t owns z_i, i = t (mod 1024).
__global__ __launch_bounds__(1024) void k_im_applyq(const double *W, long ldw, int len, int r, const double *tau, const double *y, double *z,
                                                    double *x, int accumulate) {
    __shared__ double red[2][QR_MAXW];
    const int tid = threadIdx.x;
    for (int i = tid; i < len; i += 1024) z[i] = i < r ? y[i] : 0.0;
    for (int j = r - 1; j >= 0; --j) {
        const double *v = W + (long)j * ldw;
        const int i0 = (j & ~1023) + tid;                   // this thread's first row >= j - 1023
        double s = 0.0;
        for (int i = i0; i < len; i += 1024)
            if (i >= j) s += (i == j ? 1.0 : v[i]) * z[i];
        s = qr_block_sum(s, red[j & 1]);
        const double tw = tau[j] * s;
        for (int i = i0; i < len; i += 1024)
            if (i >= j) z[i] -= tw * (i == j ? 1.0 : v[i]);
    }
    for (int i = tid; i < len; i += 1024) x[i] = accumulate ? x[i] + z[i] : z[i];
}
// res[c] = (b[c] - M[:, c]' x) / fro: the residual of the scaled system, from the untouched M
__global__ __launch_bounds__(256) void k_im_resid(const double *M, int len, long ld, const double *x, const double *b, double fro,
                                                  double *res) {
    __shared__ double red[QR_MAXW];
    const int c = blockIdx.x;
    const double *a = M + (long)c * ld;
    double s = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) s += a[i] * x[i];
    s = qr_block_sum(s, red);
    if (threadIdx.x == 0) res[c] = b[c] / fro - s / fro;
}
// out[0] = max |res| (NaN when any entry is)
__global__ __launch_bounds__(1024) void k_im_absmax(const double *res, int cnt, double *out) {
    __shared__ double mx[1024];
    __shared__ int bad[1024];
    double m = 0.0;
    int nan = 0;
    for (int c = threadIdx.x; c < cnt; c += 1024) {
        const double a = fabs(res[c]);
        if (a != a) nan = 1;
        else if (a > m) m = a;
    }
    mx[threadIdx.x] = m; bad[threadIdx.x] = nan;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 1024; ++t) { if (mx[t] > m) m = mx[t]; nan |= bad[t]; }
        out[0] = nan ? NAN : m;
    }
}

struct ImWs { QrWs qr; double *W; long ldw; double *bs, *y, *x, *z, *res, *scal; };
static long im_ldw(int len) { return ((long)len + 1) & ~1L; }     // even: the working copy always takes the 16-byte accesses
static size_t im_ws_layout(CipLayout L, int len, int cnt, ImWs *w) {
    const size_t k = (size_t)(len < cnt ? len : cnt);
    L.take<char>(qr_ws_layout(L.base, len, cnt, &w->qr));          // the factorisation's workspace comes first
    w->ldw = im_ldw(len);
    w->W = L.take<double>((size_t)w->ldw * (size_t)cnt);
    w->bs = L.take<double>(cnt); w->res = L.take<double>(cnt);
    w->y = L.take<double>(k);
    w->x = L.take<double>(len); w->z = L.take<double>(len);
    w->scal = L.take<double>(8);
    return L.bytes();
}

extern "C" int cip_imcols_workspace_bytes(int len, int cnt, size_t *bytes) {
    if (len < 0 || cnt < 0 || !bytes) { cip_set_error("cip_imcols_workspace_bytes: len, cnt >= 0 and bytes non-NULL"); return CIP_E_INVALID; }
    ImWs w;
    *bytes = im_ws_layout(nullptr, len, cnt, &w);
    return 0;
}

extern "C" int cip_imcols_dev(void *stream, const double *M, int len, int cnt, int ld, const double *b, double eps, void *workspace,
                              int *rows_host, int *nrows_host, int *consistent_host, double *resid_host) {
    const bool empty = len == 0 || cnt == 0;
    if (!qr_dims_ok(len, cnt, ld) || !(eps >= 0.0) || !(eps < INFINITY) || !nrows_host || !consistent_host ||
        (!empty && (!M || !b || !workspace || !rows_host))) {
        cip_set_error("cip_imcols_dev: bad argument (len, cnt >= 0; ld >= max(len, 1); eps >= 0 and finite; nrows_host, consistent_host "
                      "non-NULL; M, b, workspace, rows_host non-NULL when len * cnt > 0)");
        return CIP_E_INVALID;
    }
    *nrows_host = 0;
    *consistent_host = 1;
    if (resid_host) *resid_host = 0.0;
    if (empty) return 0;
    hipStream_t s = (hipStream_t)stream;
    ImWs w;
    im_ws_layout(workspace, len, cnt, &w);
    // scale = ||A||_F (src/preprocessor.jl:14)
    double fro = 0.0;
    hipLaunchKernelGGL(k_qr_init, dim3((unsigned)cnt), dim3(256), 0, s, M, len, (long)ld, w.qr.norms, (int *)nullptr);
    hipLaunchKernelGGL(k_im_fro, dim3(1), dim3(1024), 0, s, (const double *)w.qr.norms, cnt, w.scal);
    CIP_HIP_CHECK(hipGetLastError());
    CIP_HIP_CHECK(hipMemcpyAsync(&fro, w.scal, sizeof(double), hipMemcpyDeviceToHost, s));
    CIP_HIP_CHECK(hipStreamSynchronize(s));
    if (!(fro < INFINITY)) { cip_set_error("cip_imcols_dev: non-finite entry"); return CIP_E_INVALID; }
    if (fro == 0.0) return 0;                               // all-zero A: the reference's empty-R branch
    hipLaunchKernelGGL(k_im_scale, dim3((unsigned)cnt), dim3(256), 0, s, M, len, (long)ld, w.W, w.ldw, b, w.bs, fro);
    int k = 0, status = 0;
    int rc = qr_run(s, w.W, len, cnt, w.ldw, eps, w.qr, w.qr.tau, &k, &status);
    if (rc) return rc;
    if (status) { cip_set_error("cip_imcols_dev: non-finite entry"); return CIP_E_INVALID; }
    if (k == 0) return 0;
    // every |R_jj|, j < k, is above eps (k_qr_pivot tests the pivot column's own norm): the kept rows are the first k pivots
    CIP_HIP_CHECK(hipMemcpyAsync(rows_host, w.qr.piv, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, s));
    // x = A[R, :] \ b[R], minimum norm (src/preprocessor.jl:26): x = Q1 R1^-T b_R, then one refinement step x += minnorm(b - A x)
    const unsigned gk = (unsigned)((k + 255) / 256);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(k_im_gather, dim3(gk), dim3(256), 0, s, (const double *)(pass ? w.res : w.bs), (const int *)w.qr.piv, k, w.y);
        hipLaunchKernelGGL(k_im_fwd, dim3(1), dim3(1024), 0, s, (const double *)w.W, w.ldw, k, w.y);
        hipLaunchKernelGGL(k_im_applyq, dim3(1), dim3(1024), 0, s, (const double *)w.W, w.ldw, len, k, (const double *)w.qr.tau,
                           (const double *)w.y, w.z, w.x, pass);
        hipLaunchKernelGGL(k_im_resid, dim3((unsigned)cnt), dim3(256), 0, s, M, len, (long)ld, (const double *)w.x, b, fro, w.res);
    }
    hipLaunchKernelGGL(k_im_absmax, dim3(1), dim3(1024), 0, s, (const double *)w.res, cnt, w.scal + 1);
    CIP_HIP_CHECK(hipGetLastError());
    double resid = 0.0;
    CIP_HIP_CHECK(hipMemcpyAsync(&resid, w.scal + 1, sizeof(double), hipMemcpyDeviceToHost, s));
    CIP_HIP_CHECK(hipStreamSynchronize(s));
    std::sort(rows_host, rows_host + k);
    *nrows_host = k;
    *consistent_host = resid < eps ? 1 : 0;
    if (resid_host) *resid_host = resid;
    return 0;
}
