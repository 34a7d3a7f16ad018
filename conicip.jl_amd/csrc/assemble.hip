// KKT assembly on the device (level 2 of the plugin, before the factorisation).
//
//  CIP_ROUTE_SCHUR    K = [ Q + A'(F'F)^-1 A   G' ]   -- the elimination order of `pivot`
//                         [ G                  0  ]      (src/kktsolvers.jl:289-293, :316-338)
//  CIP_ROUTE_FULL3X3  K = [ -F'F  -A   0  ]            -- the literal 3x3 block assembly
//                         [ -A'    Q   G' ]               [Q G' -A'; G 0 0; A 0 F'F]
//                         [  0     G   0  ]               (src/kktsolvers.jl:254-256), symmetrised and
//                                                         permuted to the static pivot order (3,1,2)
// Only the lower triangle is written / referenced; K is padded to a multiple of 128 with an
// identity block.
#include "cip_handle.h"
#include "../../include/cipkkt.h"

// rows >= n of the Schur-route matrix: G block, zero block, identity padding (lower part)
__global__ __launch_bounds__(256) void k_fill_rest(double *K, long ldk, int n, int p, int Npad, const double *G, long ldg, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, K, G);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Npad) return;
    for (int i = n + blockIdx.y; i < Npad; i += gridDim.y) {
        if (j > i) continue;
        double v;
        if (i < n + p) v = (j < n) ? G[(i - n) + (long)j * ldg] : 0.0;
        else v = (i == j) ? 1.0 : 0.0;
        K[i + (long)j * ldk] = v;
    }
}

// K[r0 + i, c0 + j] = sign * M[i + j*ldm]   (i < rows, j < cols); coalesced along i
__global__ __launch_bounds__(256) void k_copy_block(double *K, long ldk, int r0, int c0, const double *M, long ldm,
                                                     int rows, int cols, double sign, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, K, M);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    for (int j = blockIdx.y; j < cols; j += gridDim.y)
        K[(r0 + i) + (long)(c0 + j) * ldk] = sign * M[i + (long)j * ldm];
}

// The same for a square block on the diagonal (r0 == c0), restricted to the 128x128 tiles of K on or below the
// diagonal: the factorisation never references a tile above it, and Q is half of the assembly's HBM traffic
// (n = 8192: 1.07 GB -> 0.56 GB per factorisation).
__global__ __launch_bounds__(256) void k_copy_block_lower(double *K, long ldk, int r0, const double *M, long ldm, int n, double sign, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, K, M);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int jend = min(n, (((r0 + i) >> 7) + 1) * 128 - r0);      // columns up to the end of this row's diagonal tile
    for (int j = blockIdx.y; j < jend; j += gridDim.y)
        K[(r0 + i) + (long)(r0 + j) * ldk] = sign * M[i + (long)j * ldm];
}
// The 16-byte form for even n, r0 and leading dimensions and 16-byte-aligned bases: a workgroup moves 512 rows x 8 columns
// per step, a thread's eight loads in flight before its first store (one column of 512 rows per workgroup -- the first
// 16-byte version, 262144 workgroups at n = 8192 -- ran at 2.8 TB/s: 0.19 ms of a 6.1-ms step).
#define COPY_COLS 8
__global__ __launch_bounds__(256) void k_copy_block_lower_v(double *K, long ldk, int r0, const double *M, long ldm, int n, double sign, int jmax, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, K, M);
    const int i = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int jend = min(min(n, jmax), (((r0 + i) >> 7) + 1) * 128 - r0);      // columns up to the end of this row pair's diagonal tile (and < jmax)
    for (int j0 = blockIdx.y * COPY_COLS; j0 < jend; j0 += gridDim.y * COPY_COLS) {
        v2d v[COPY_COLS];
#pragma unroll
        for (int u = 0; u < COPY_COLS; ++u)
            if (j0 + u < jend) v[u] = *(const v2d *)(M + i + (long)(j0 + u) * ldm);
#pragma unroll
        for (int u = 0; u < COPY_COLS; ++u)
            if (j0 + u < jend) *(v2d *)(K + (r0 + i) + (long)(r0 + j0 + u) * ldk) = sign * v[u];
    }
}
static bool copy_lower_vectorisable(const double *K, long ldk, int r0, const double *M, long ldm, int n) {
    return !(n & 1) && !(r0 & 1) && !(ldk & 1) && !(ldm & 1) && !(((uintptr_t)K | (uintptr_t)M) & 15);
}
// jmax < n: only the columns [0, jmax) (the lazy copy of the Schur route)
static void launch_copy_block_lower(hipStream_t s, double *K, long ldk, int r0, const double *M, long ldm, int n, double sign, int jmax = 1 << 30) {
    if (copy_lower_vectorisable(K, ldk, r0, M, ldm, n)) {
        const int nc = n < jmax ? n : jmax;
        const int gy = (nc + COPY_COLS - 1) / COPY_COLS;
        cip_launch_b(k_copy_block_lower_v, dim3((n + 511) / 512, gy < 32768 ? gy : 32768), dim3(256), 0, s, K, ldk, r0, M, ldm, n, sign, jmax);
    } else {
        cip_launch_b(k_copy_block_lower, dim3((n + 255) / 256, n < 32768 ? n : 32768), dim3(256), 0, s, K, ldk, r0, M, ldm, n, sign);
    }
}

// ---------------------------------------------------------------- Q block from a CSR Q (CIP_FLAG_Q_CSR)
// Q is symmetric and stored whole (level 1 checks it), so whoever owns COLUMN j of the column-major K reads CSR ROW j: entry
// (j, i) of the row is Q[i, j], and all of a column's writes land in that one column.  No duplicates: every entry of K is touched
// at most once per launch -- no atomics, nothing to order between workgroups.
// An entry is taken when the dense copy / the Schur formation would have written it: ((r0 + i) >> shift) >= ((r0 + j) >> shift),
// shift 7 = the 128-tiles on or below the diagonal (k_copy_block_lower), 6 = the 64-quarter-tiles (cip_syrk_schur).
//
// Schur route with a CSR A (r0 = 0): ONE pass per column instead of the copy of n^2 / 2 doubles out of a dense Q -- the
// workgroup zeroes column j from the top of its diagonal tile down to row n (16-byte stores when `vec`: K 16-byte aligned, ldk
// even; the tile top is a multiple of 128), then scatters the column's entries.
__global__ __launch_bounds__(256) void k_qcsr_fill_cols(double *K, long ldk, int n, const int *rp, const int *ci, const double *v, int vec,
                                                         CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO4(cb, K, rp, ci, v);
    const int j = blockIdx.x, tid = threadIdx.x;
    if (j >= n) return;
    double *col = K + (long)j * ldk;
    const int z0 = j & ~127;
    if (vec) {
        const int nv = (n - z0) >> 1;
        for (int t = tid; t < nv; t += 256) *(v2d *)(col + z0 + 2 * t) = (v2d){0.0, 0.0};
        if (((n - z0) & 1) && tid == 0) col[n - 1] = 0.0;
    } else {
        for (int i = z0 + tid; i < n; i += 256) col[i] = 0.0;
    }
    __syncthreads();                                            // the zeroes of the whole workgroup land before its entries
    const int q1 = rp[j + 1];
    for (int q = rp[j] + tid; q < q1; q += 256) {
        const int i = ci[q];
        if ((i >> 7) >= (j >> 7)) col[i] = v[q];
    }
}
// The scatter alone, one WAVE per column (four columns per workgroup), at row / column offset r0: K[r0 + i, r0 + j] = Q[i, j]
// (full 3x3 route: K was zeroed) or += Q[i, j] (Schur route with a dense A, behind the Qin-less Schur formation)
template <bool ADD>
__global__ __launch_bounds__(256) void k_qcsr_scatter(double *K, long ldk, int r0, int n, const int *rp, const int *ci, const double *v,
                                                       int shift, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO4(cb, K, rp, ci, v);
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    double *col = K + r0 + (long)(r0 + j) * ldk;
    const int q1 = rp[j + 1];
    for (int q = rp[j] + lane; q < q1; q += 64) {
        const int i = ci[q];
        if (((r0 + i) >> shift) < ((r0 + j) >> shift)) continue;
        if (ADD) col[i] += v[q];
        else col[i] = v[q];
    }
}

// ---------------------------------------------------------------- sparse-A Schur terms (R and Q cones)
// K[i, j] += sum_r w_r a_ri a_rj  (i >= j), w_r = 1/d_r^2 (R), -J_rr/beta^2 (Q).  One thread per variable i OWNS row i
// of the lower triangle: it walks column i of A (= row i of the CSR of A', rows r ascending) and, for every r, row r
// of A.  No atomics, fixed summation order: bit-reproducible (the first version scattered with unsafeAtomicAdd per
// row of A).
__device__ __forceinline__ double schur_row_weight(const ConeDesc &cd, const double *scal, int r) {
    if (cd.type == CIP_CONE_R) { const double d = scal[cd.soff + (r - cd.off)]; return 1.0 / (d * d); }
    if (cd.type == CIP_CONE_S) return 0.0;                  // (never used: the callers skip S rows, whose (F'F)^-1 is not diagonal)
    const double beta = scal[cd.soff];
    return ((r == cd.off) ? -1.0 : 1.0) / (beta * beta);
}
__global__ __launch_bounds__(256) void k_schur_rows(int n, const int *trp, const int *tci, const double *tv, const int *rp,
                                                     const int *ci, const double *av, const int *row_cone,
                                                     const ConeDesc *cones, const double *scal, double *K, long ldk, int base, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO8(cb, trp, tci, tv, rp, ci, av, scal, K);
    // Round 4: one WAVE per variable i (it was one thread: n = 500 with a 10 %-dense A -- the reference's "many small SOCs"
    // benchmark, benchmark/profile.jl:54-69 -- put 3750 dependent read-modify-writes on each of 500 threads, 2.3 ms beside a
    // 0.19-ms factorisation).  The rows r of column i are still taken one after the other, ascending; the entries of row r
    // (distinct columns j) go to the lanes.  Entry (i, j) therefore receives the same additions in the same order as
    // before: bit-identical, no atomics.  Two rows may hit the same (i, j) from different lanes: the wave's accesses to K go
    // to L2 (agent scope) and one row's stores are waited for before the next row's loads.
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double *Ki = K + (base + i) + (long)base * ldk;
    for (int q = trp[i]; q < trp[i + 1]; ++q) {
        const int r = tci[q];
        const ConeDesc rc = cones[row_cone[r]];
        if (rc.type == CIP_CONE_S) continue;                // S rows: dense congruences + a GEMM (assemble_schur)
        const double wa = schur_row_weight(rc, scal, r) * tv[q];
        const int b1 = rp[r + 1];
        bool wrote = false;
        for (int b = rp[r] + lane; b < b1; b += 64) {
            const int j = ci[b];
            if (j <= i) {
                double *kp = Ki + (long)j * ldk;
                double x = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x += wa * av[b];
                __hip_atomic_store(kp, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                wrote = true;
            }
        }
        (void)wrote;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}
// The same for an A with at most one entry per row and R cones only -- the Schur terms are then on the diagonal -- when the
// copy of Q is lazy: rows below `nb0` deliver K_ii = Q_ii + sum_r w_r a_ri^2 (the same fused multiply-adds in the same order
// on the same start value as k_schur_rows on the copied Q_ii) into kdiag[i] instead of K
__global__ __launch_bounds__(256) void k_schur_diag_lazy(int n, int nb0, const int *trp, const int *tci, const double *tv, const int *rp,
                                                          const int *ci, const double *av, const int *row_cone, const ConeDesc *cones,
                                                          const double *scal, const double *Q, long ldq, double *K, long ldk, double *kdiag,
                                                          CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO8(cb, trp, tci, tv, rp, ci, av, scal, Q);
    CIP_BO2(cb, K, kdiag);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d = i < nb0 ? K[i + (long)i * ldk] : Q[i + (long)i * ldq];
    for (int q = trp[i]; q < trp[i + 1]; ++q) {
        const int r = tci[q];
        const double wa = schur_row_weight(cones[row_cone[r]], scal, r) * tv[q];
        for (int b = rp[r]; b < rp[r + 1]; ++b)
            if (ci[b] == i) d += wa * av[b];
    }
    if (i < nb0) K[i + (long)i * ldk] = d;
    else kdiag[i] = d;
}
// Gm[i, qidx] = sum over the rows r of Q cone qidx of (sqrt2/beta) (J wbar)_r A[r, i]: same ownership (thread i, column i of
// A in ascending r; the rows of one cone are consecutive)
__global__ __launch_bounds__(256) void k_schur_qcols(int n, const int *trp, const int *tci, const double *tv,
                                                      const int *row_cone, const ConeDesc *cones, const double *scal,
                                                      double *Gm, long ldgm, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO5(cb, trp, tci, tv, scal, Gm);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int cur = -1;
    double acc = 0.0;
    for (int q = trp[i]; q < trp[i + 1]; ++q) {
        const int r = tci[q];
        const ConeDesc cd = cones[row_cone[r]];
        if (cd.type != CIP_CONE_Q) continue;
        if (cd.qidx != cur) {
            if (cur >= 0) Gm[i + (long)cur * ldgm] = acc;
            cur = cd.qidx; acc = 0.0;
        }
        const double beta = scal[cd.soff];
        const double *w = scal + cd.soff + 1;
        const int e = r - cd.off;
        // wbar_1 = w1^2/beta - 1 ; wbar_t = w1 w_t / beta ; (J wbar)_t = -wbar_t
        const double jw = (e == 0) ? (w[0] * w[0] / beta - 1.0) : -(w[0] * w[e] / beta);
        acc += (jw * 1.4142135623730951 / beta) * tv[q];
    }
    if (cur >= 0) Gm[i + (long)cur * ldgm] = acc;
}

// CSR A with S cones: AtS[i, aoff_c + (r - off_c)] = A[r, i] for the rows r of every S cone c (thread i walks column i of A)
__global__ __launch_bounds__(256) void k_scatter_AtS(int n, const int *trp, const int *tci, const double *tv, const int *row_cone,
                                                      const ConeDesc *cones, double *AtS, long ld, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO4(cb, trp, tci, tv, AtS);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int q = trp[i]; q < trp[i + 1]; ++q) {
        const int r = tci[q];
        const ConeDesc cd = cones[row_cone[r]];
        if (cd.type == CIP_CONE_S) AtS[i + (long)(cd.aoff + (r - cd.off)) * ld] = tv[q];
    }
}
int cip_scatter_AtS(cip_handle *h) {
    if (!h->AtS || h->n == 0) return 0;
    CIP_HIP_CHECK(hipMemsetAsync(h->AtS, 0, sizeof(double) * (size_t)h->npad * h->mSpad, h->stream));      // (cip_update_problem: new values)
    hipLaunchKernelGGL(k_scatter_AtS, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->n, h->T_rp, h->T_ci, h->T_v, h->row_cone,
                       h->cs.d_cones, h->AtS, (long)h->npad, CipBatch{0, 1ull});
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- full 3x3 route: -F'F block
__global__ __launch_bounds__(256) void k_fill_ftf(const ConeDesc *cones, const WorkItem *items, const double *scal,
                                                   double *K, long ldk, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, scal, K);
    const WorkItem it = items[blockIdx.x];
    const ConeDesc cd = cones[it.cone];
    const int tid = threadIdx.x;
    if (cd.type == CIP_CONE_R) {
        for (int e = it.start + tid; e < it.start + it.len; e += 256) {
            const double d = scal[cd.soff + e];
            const long g = cd.off + e;
            K[g + g * ldk] = -d * d;
        }
    } else if (cd.type == CIP_CONE_Q) {
        // F'F = F^2 = beta^2 (2 wbar wbar' - J); a pack of small cones: the workgroup walks through its cones
        if (!it.width) return;                            // a large cone: k_fill_ftf_qbig
        const int ncone = it.len;
        for (int q = 0; q < ncone; ++q) {
            const ConeDesc qc = cones[it.cone + q];
            const int k = qc.dim;
            const double beta = scal[qc.soff];
            const double *w = scal + qc.soff + 1;
            const double b2 = beta * beta, w0 = w[0];
            for (long e = tid; e < (long)k * k; e += 256) {
                const int i = (int)(e % k), j = (int)(e / k);
                if (i < j) continue;
                const double wi = (i == 0) ? (w0 * w0 / beta - 1.0) : (w0 * w[i] / beta);
                const double wj = (j == 0) ? (w0 * w0 / beta - 1.0) : (w0 * w[j] / beta);
                double v = 2.0 * wi * wj;
                if (i == j) v -= (i == 0) ? 1.0 : -1.0;
                K[(qc.off + i) + (long)(qc.off + j) * ldk] = -b2 * v;
            }
        }
    }
}
// -F'F of a Q cone of dimension > 64: the k (k + 1) / 2 entries of its lower triangle by column, many workgroups (round 4: one
// workgroup walked all k^2 of them, 19 ms at k = 4097)
__global__ __launch_bounds__(256) void k_fill_ftf_qbig(const ConeDesc *cones, const WorkItem *items, const int *bigq, const double *scal,
                                                        double *K, long ldk, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, scal, K);
    const WorkItem it = items[bigq[blockIdx.x]];
    const ConeDesc qc = cones[it.cone];
    const int k = qc.dim;
    const double beta = scal[qc.soff];
    const double *w = scal + qc.soff + 1;
    const double b2 = beta * beta, w0 = w[0];
    for (int j = blockIdx.y; j < k; j += gridDim.y) {
        const double wj = (j == 0) ? (w0 * w0 / beta - 1.0) : (w0 * w[j] / beta);
        for (int i = j + threadIdx.x; i < k; i += 256) {
            const double wi = (i == 0) ? (w0 * w0 / beta - 1.0) : (w0 * w[i] / beta);
            double v = 2.0 * wi * wj;
            if (i == j) v -= (i == 0) ? 1.0 : -1.0;
            K[(qc.off + i) + (long)(qc.off + j) * ldk] = -b2 * v;
        }
    }
}
__global__ __launch_bounds__(256) void k_scatter_negA(int nrowsT, const int *trp, const int *tci, const double *tv,
                                                       double *K, long ldk, int r0, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO4(cb, trp, tci, tv, K);
    // CSR of A' (row i = variable, column = constraint r):  K[r0 + i, r] = -A[r, i]
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nrowsT) return;
    for (int q = trp[i]; q < trp[i + 1]; ++q) K[(r0 + i) + (long)tci[q] * ldk] = -tv[q];
}
__global__ __launch_bounds__(256) void k_pad_identity(double *K, long ldk, int N, int Npad, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO1(cb, K);
    const int i = N + blockIdx.x * 256 + threadIdx.x;
    if (i < Npad) K[i + (long)i * ldk] = 1.0;
}

// lazy_ok (the caller runs cip_ldlt_factor on the result right away): with a CSR A that has one entry per row, R cones only,
// no equality block and no padding, K = Q + diag(..) -- and 3/4 (order 2048) to 9/10 (order 8192) of the copy of Q into K
// is overwritten by the FIRST trailing update without anybody else having looked at it.  Then only the first outer block's
// columns are copied; the first trailing update takes its C operand from Q itself with the Schur diagonal from h->kdiag
// (EPI_LAZYC) and writes K.  Every entry of K goes through the same operations as with the full copy (bit-identical
// factor): 115 -> 25 us per factorisation at n = 8192, 7 of the 86 ms of a config-5 pass.
static CipKnob g_lazy_copy{[] { return (int)(cip_env_int("CIP_LAZY_COPY", 1) != 0); }};    // cip_set_lazy_copy: 1 (default) on, 0 off; read by worker threads
int cip_lazy_copy_set(int on) { return g_lazy_copy.set(on, [](int v) { return v == 0 || v == 1; }); }
static int assemble_schur(cip_handle *h, bool lazy_ok) {
    hipStream_t s = h->stream;
    int rc;
    const int n = h->n, p = h->p;
    h->ws.lazyC = nullptr;
    if (!h->A_sparse) {
        if ((rc = cip_cones_scale_At(s, h->cs, n, h->At, h->npad, h->Wt, h->npad))) return rc;
        // (algorithmic work of the Schur formation: m n^2 flop on the lower half)
        if ((rc = cip_prof_slot_begin(CIP_PROF_SYRK, s, (double)h->m * (double)n * (double)n * (cip_in_batch() ? (double)__builtin_popcountll(cip_tl_bz.mask) : 1.0)))) return rc;
        // (CSR Q: the Schur formation stores W W' alone -- h->Q is NULL -- and the stored entries of Q are added, each touched once)
        if ((rc = cip_syrk_schur(s, h->npad, h->mpad, n, 1.0, h->Wt, h->npad, h->Q, n, h->K, h->ldk, h->syrk_ws, h->syrk_n, h->syrk_len))) return rc;
        if ((rc = cip_prof_slot_end(CIP_PROF_SYRK, s))) return rc;
        if (h->Q_sparse && cip_grp_Q_nonempty(h))
            cip_launch_b(k_qcsr_scatter<true>, dim3((n + 3) / 4), dim3(256), 0, s, h->K, h->ldk, 0, n, h->Q_rp, h->Q_ci, h->Q_v, 6);
    } else {
        const int lazy_on = g_lazy_copy.get();
        bool all_r = cip_all_r(h);
        // nb0 must be the width of the FIRST outer block of the factorisation that follows: only its columns are copied, and that
        // factorisation's first trailing update is what fills the rest of K.  The two agree because both ask the same rule
        // (cip_ldlt_plan.h: ldlt_outer_block) with the settings as they stand -- the lazy form needs n > nb0, where the first block
        // is the regular width whatever the tail rule -- and the caller factors right behind this assembly (lazy_ok)
        const int nb0 = cip_ldlt_outer_block_for(h->Npad);
        if (!h->Q_sparse && lazy_on && lazy_ok && all_r && cip_grp_A_one_per_row(h) && p == 0 && h->Npad == n && n > nb0 && h->reg_rel <= 0.0 && h->kdiag &&
            copy_lower_vectorisable(h->K, h->ldk, 0, h->Q, (long)n, n)) {
            launch_copy_block_lower(s, h->K, h->ldk, 0, h->Q, (long)n, n, 1.0, nb0);
            cip_launch_b(k_schur_diag_lazy, dim3((n + 255) / 256), dim3(256), 0, s, n, nb0, h->T_rp, h->T_ci, h->T_v, h->A_rp, h->A_ci, h->A_v,
                         h->row_cone, h->cs.d_cones, h->cs.d_scal, h->Q, (long)n, h->K, h->ldk, h->kdiag);
            CIP_HIP_CHECK(hipGetLastError());
            h->ws.lazyC = h->Q; h->ws.lazy_ld = n; h->ws.lazy_diag = h->kdiag;
            return 0;
        }
        if (h->Q_sparse) {
            const int vec = !(h->ldk & 1) && !(((uintptr_t)h->K) & 15);
            cip_launch_b(k_qcsr_fill_cols, dim3(n), dim3(256), 0, s, h->K, h->ldk, n, h->Q_rp, h->Q_ci, h->Q_v, vec);
        } else if (n > 0) {
            launch_copy_block_lower(s, h->K, h->ldk, 0, h->Q, (long)n, n, 1.0);
        }
        if (h->m > 0) {
            cip_launch_b(k_schur_rows, dim3((n + 3) / 4), dim3(256), 0, s, n, h->T_rp, h->T_ci, h->T_v, h->A_rp, h->A_ci,
                               h->A_v, h->row_cone, h->cs.d_cones, h->cs.d_scal, h->K, h->ldk, 0);
            if (h->nq > 0) {
                if ((rc = cip_zero(s, (long)h->npad * h->nqpad, h->Gm))) return rc;
                cip_launch_b(k_schur_qcols, dim3((n + 255) / 256), dim3(256), 0, s, n, h->T_rp, h->T_ci, h->T_v,
                                   h->row_cone, h->cs.d_cones, h->cs.d_scal, h->Gm, (long)h->npad);
            }
        }
    }
    if (h->Npad > n) {
        cip_launch_b(k_fill_rest, dim3((h->Npad + 255) / 256, (h->Npad - n) < 32768 ? (h->Npad - n) : 32768), dim3(256), 0, s, h->K, h->ldk, n, p,
                           h->Npad, h->G, (long)p);
    }
    if (h->A_sparse && h->AtS) {
        // the S cones' part of A'(F'F)^-1 A: W = A_S' F^-1 by congruences on the dense block of their rows, then K += W W'
        if ((rc = cip_sdp_scale_At(s, h->cs, n, h->AtS, (long)h->npad, h->WtS, (long)h->npad))) return rc;
        if ((rc = cip_gemm_lower(s, h->npad, h->mSpad, 1.0, h->WtS, h->npad, h->WtS, h->npad, h->K, h->ldk))) return rc;
    }
    if (h->A_sparse && h->nq > 0 && h->m > 0) {
        // after k_fill_rest: the rank-nq update touches whole 128-tiles (adds exact zeros outside [0,n)^2)
        if ((rc = cip_gemm_lower(s, h->npad, h->nqpad, 1.0, h->Gm, h->npad, h->Gm, h->npad, h->K, h->ldk))) return rc;
    }
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cip_sdp_fill_ftf(hipStream_t s, const ConeSet &cs, double *K, long ldk);     // sdp.hip

static int assemble_full(cip_handle *h) {
    hipStream_t s = h->stream;
    const int n = h->n, m = h->m, p = h->p;
    { int rcz = cip_zero(s, (long)h->ldk * h->Npad, h->K); if (rcz) return rcz; }
    if (h->cs.nitems > 0)
        cip_launch_b(k_fill_ftf, dim3(h->cs.nitems), dim3(256), 0, s, h->cs.d_cones, h->cs.d_items, h->cs.d_scal,
                           h->K, h->ldk);
    if (h->cs.nbigq > 0)
        cip_launch_b(k_fill_ftf_qbig, dim3(h->cs.nbigq, 128), dim3(256), 0, s, h->cs.d_cones, h->cs.d_items, (const int *)h->cs.d_bigq, h->cs.d_scal, h->K, h->ldk);
    if (h->cs.has_S) { int rc = cip_sdp_fill_ftf(s, h->cs, h->K, h->ldk); if (rc) return rc; }
    if (m > 0 && n > 0) {
        if (!h->A_sparse)
            cip_launch_b(k_copy_block, dim3((n + 255) / 256, m < 32768 ? m : 32768), dim3(256), 0, s, h->K, h->ldk, m, 0, h->At,
                               (long)h->npad, n, m, -1.0);
        else
            cip_launch_b(k_scatter_negA, dim3((n + 255) / 256), dim3(256), 0, s, n, h->T_rp, h->T_ci, h->T_v,
                               h->K, h->ldk, m);
    }
    if (h->Q_sparse) {
        if (cip_grp_Q_nonempty(h))
            cip_launch_b(k_qcsr_scatter<false>, dim3((n + 3) / 4), dim3(256), 0, s, h->K, h->ldk, m, n, h->Q_rp, h->Q_ci, h->Q_v, 7);
    } else if (n > 0)
        launch_copy_block_lower(s, h->K, h->ldk, m, h->Q, (long)n, n, 1.0);
    if (p > 0)
        cip_launch_b(k_copy_block, dim3((p + 255) / 256, n < 32768 ? n : 32768), dim3(256), 0, s, h->K, h->ldk, m + n, m, h->G,
                           (long)p, p, n, 1.0);
    if (h->Npad > h->N)
        cip_launch_b(k_pad_identity, dim3((h->Npad - h->N + 255) / 256), dim3(256), 0, s, h->K, h->ldk, h->N, h->Npad);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// Static regularisation, scaled per row: K_ii += s_i * rel * max_j |K_ij| (the symmetric matrix' full row i: its stored
// row part j <= i and its column part below the diagonal), s_i = +1 on the positive-pivot block [p0, p1), -1 elsewhere.
// Late interior-point iterates spread the diagonal of S over 20 orders of magnitude; one global delta either drowns
// the small rows or does nothing for the large ones.
//
// One pass over the lower triangle: a workgroup per 128 x 128 tile reads its tile once, 16 columns at a time with the threads
// along the rows (coalesced), and reduces |K_ij| into the maxima of its 128 rows (in registers) and of its 128 columns (through
// LDS: 16 lanes per column, then four shuffle steps).  The partial maxima of all tiles meet in mx[0 .. N) by atomicMax on the bit
// pattern -- non-negative doubles order like unsigned integers, and a maximum does not depend on the order it is taken in, so
// mx[i] has the bits of fmax over the whole row whatever the tiles' schedule.  fmax(0, |x|) drops a NaN entry, as fmax always did
// here.  A diagonal tile takes j <= i for the row part and r > i for the column part (what lies above the diagonal is not K).
// Before: one thread per row over the row parts (N / 256 workgroups), then one workgroup per column over the column parts -- two
// reads of the triangle, the first on a fraction of the chip (DESIGN_LOG.md, "Problems that need the regularised LDL' stay in
// their group", has both forms' timings).
#define REG_TILE 128
#define REG_COLS 16                       // columns per pass: 256 threads = 128 rows x 2 halves of 8 columns
__global__ __launch_bounds__(256) void k_regmax_tiles(const double *K, long ldk, int N, double *mx_d, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, K, mx_d);
    unsigned long long *mx = (unsigned long long *)mx_d;
    __shared__ double sh[2][REG_COLS][REG_TILE + 1];      // |K| of one pass, by column (two buffers: one barrier per pass)
    __shared__ double shrow[REG_TILE];
    // tile (ti, tj), tj <= ti, from the linear index ti (ti + 1) / 2 + tj
    const int t = blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
    while ((long)ti * (ti + 1) / 2 > t) --ti;
    const int tj = t - (int)((long)ti * (ti + 1) / 2);
    const int r = threadIdx.x & (REG_TILE - 1), hh = threadIdx.x >> 7;
    const int cc = threadIdx.x >> 4, sg = threadIdx.x & 15;
    const int gi = ti * REG_TILE + r;
    double rmx = 0.0;
    for (int q = 0; q < REG_TILE / REG_COLS; ++q) {
        double (*buf)[REG_TILE + 1] = sh[q & 1];
        double a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int gj = tj * REG_TILE + q * REG_COLS + hh * 8 + k;
            a[k] = (gi < N && gj <= gi) ? fmax(0.0, fabs(K[gi + (long)gj * ldk])) : 0.0;     // (gj <= gi < N)
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int gj = tj * REG_TILE + q * REG_COLS + hh * 8 + k;
            rmx = fmax(rmx, a[k]);
            buf[hh * 8 + k][r] = gj < gi ? a[k] : 0.0;          // the diagonal belongs to the row part only
        }
        __syncthreads();
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) v = fmax(v, buf[cc][sg + 16 * e]);
        for (int o = 8; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
        const int gc = tj * REG_TILE + q * REG_COLS + cc;
        if (sg == 0 && gc < N && v > 0.0) atomicMax(&mx[gc], (unsigned long long)__double_as_longlong(v));
    }
    if (hh == 1) shrow[r] = rmx;
    __syncthreads();
    if (hh == 0) {
        rmx = fmax(rmx, shrow[r]);
        if (gi < N && rmx > 0.0) atomicMax(&mx[gi], (unsigned long long)__double_as_longlong(rmx));
    }
}
__global__ __launch_bounds__(256) void k_regularize_diag(double *K, long ldk, int N, int p0, int p1, double rel, const double *mx, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO2(cb, K, mx);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double delta = rel * mx[i];
    K[i + (long)i * ldk] += (i >= p0 && i < p1) ? delta : -delta;
}
// three launches (zero, tile pass, diagonal update) for every problem of the thread's mask; the maxima live in h->rhs (free between
// an assembly and the next solve).  The diagonal is modified only after every maximum has been taken: its launch is behind the tiles'
int cip_regularize(cip_handle *h, double rel) {
    if (h->N <= 0) return 0;
    const int T = (h->N + REG_TILE - 1) / REG_TILE;
    { const int rc = cip_zero(h->stream, h->N, h->rhs); if (rc) return rc; }
    cip_launch_b(k_regmax_tiles, dim3((unsigned)((long)T * (T + 1) / 2)), dim3(256), 0, h->stream, (const double *)h->K, h->ldk, h->N, h->rhs);
    cip_launch_b(k_regularize_diag, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, h->K, h->ldk, h->N, h->ws.signs.p0, h->ws.signs.p1, rel,
                 (const double *)h->rhs);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cip_assemble(cip_handle *h, bool lazy_ok) {
    h->ws.lazyC = nullptr;
    // K is about to be overwritten: the side stream may still be reading the previous factor (a factorisation without solves)
    { const int rj = cip_ldlt_side_join(h->stream, h->ws, -1); if (rj) return rj; }
    int rc = (h->route == CIP_ROUTE_SCHUR) ? assemble_schur(h, lazy_ok) : assemble_full(h);
    if (rc == 0 && h->reg_rel > 0.0) rc = cip_regularize(h, h->reg_rel);
    if (rc == 0) { h->assembled = true; h->factored = false; }
    return rc;
}
