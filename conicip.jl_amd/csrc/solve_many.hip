// Many right-hand sides for one LDL' factor (gfx950).
//
// The single-column solves (ldlt.hip: cip_ldlt_solve) stream the whole factor twice per right-hand side with column-dot
// launches.  With k columns every block step becomes a narrow level-3 product,
//   C[M x k] = alpha A' B + beta C,   A: Kr x M col-major (lda),  B: Kr x k (ldb),  C: M x k (ldc),
// the reduction along A's contiguous columns -- the layout the sweeps already read (XT_J / X_J, the L' blocks right of the
// diagonal block and the L blocks left of it) and the one of the handle's A (m x n, ld m) and At (n x m, ld npad).
// L is then read once per sweep for up to 64 columns, on v_mfma_f64_16x16x4_f64.
//
// Determinism: no atomics, no hand-off between workgroups.  An output element is reduced by the W waves of one workgroup, wave w
// over the 16-row chunks w, w + W, ... of Kr, each chunk as four MFMAs (rows r + 4g + q, g = 0..3, for q = 0, 1, 2, 3: the MFMA is
// a chain of individually rounded FMAs over its four k, tools/mfma_order.hip), and the W partial sums are added in wave order.  W
// depends on M and Kr only: every column's bits are independent of k and of the other columns of the call.
#include "cip_internal.h"

struct TnArgs {
    const double *A; long lda;
    const double *B; long ldb;
    double *C; long ldc;
    int M, Kr, k;
    double alpha, beta;
};

// four consecutive rows r, r+1, r+2, r+3 of one column (zeros for rows >= Kr or a column that does not exist)
template <bool VEC>
__device__ __forceinline__ v4d load_rows4(const double *col, bool ok, int r, int Kr) {
    v4d v = {0.0, 0.0, 0.0, 0.0};
    if (!ok) return v;
    if (VEC) return *(const v4d *)(col + r);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (r + q < Kr) v[q] = col[r + q];
    return v;
}

// One workgroup = 16 rows of C (its A columns) x all k (<= 16 KC) columns; W waves split Kr.  VEC: Kr % 16 == 0 and the
// A / B columns 32-byte aligned (v4d loads); the other form guards every row and does the same arithmetic.
template <int W, int KC, bool VEC>
__global__ __launch_bounds__(W * 64) void k_gemm_tn(TnArgs a) {
    __shared__ v4d red[W > 1 ? W : 1][KC][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int m = blockIdx.x * 16 + l15;
    const bool mok = m < a.M;
    const double *Ap = a.A + (long)(mok ? m : 0) * a.lda;
    const double *Bp[KC];
    bool bok[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) {
        const int j = t * 16 + l15;
        bok[t] = j < a.k;
        Bp[t] = a.B + (long)(bok[t] ? j : 0) * a.ldb;
    }
    v4d acc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    const int nch = (a.Kr + 15) >> 4;
    int c = w;
    // two chunks in flight per wave
    for (; c + W < nch; c += 2 * W) {
        const int r0 = c * 16 + 4 * g, r1 = r0 + 16 * W;
        const v4d a0 = load_rows4<VEC>(Ap, mok, r0, a.Kr), a1 = load_rows4<VEC>(Ap, mok, r1, a.Kr);
        v4d b0[KC], b1[KC];
#pragma unroll
        for (int t = 0; t < KC; ++t) { b0[t] = load_rows4<VEC>(Bp[t], bok[t], r0, a.Kr); b1[t] = load_rows4<VEC>(Bp[t], bok[t], r1, a.Kr); }
#pragma unroll
        for (int t = 0; t < KC; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0[t][q], a0[q], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < KC; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1[t][q], a1[q], acc[t], 0, 0, 0);
    }
    if (c < nch) {
        const int r0 = c * 16 + 4 * g;
        const v4d a0 = load_rows4<VEC>(Ap, mok, r0, a.Kr);
#pragma unroll
        for (int t = 0; t < KC; ++t) {
            const v4d b0 = load_rows4<VEC>(Bp[t], bok[t], r0, a.Kr);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0[q], a0[q], acc[t], 0, 0, 0);
        }
    }
    // acc[t][q] @ lane (l15, g) = partial C[m, 16 t + g + 4 q]; the W partials are added in wave order, wave t finishes column tile t
    int t0 = 0;
    v4d sum = acc[0];
    if (W > 1) {
#pragma unroll
        for (int t = 0; t < KC; ++t) red[w][t][lane] = acc[t];
        __syncthreads();
        if (w >= KC) return;
        t0 = w;
        sum = red[0][t0][lane];
#pragma unroll
        for (int ww = 1; ww < W; ++ww) sum += red[ww][t0][lane];
    }
    for (int t = t0; t < (W > 1 ? t0 + 1 : KC); ++t) {
        if (W == 1) sum = acc[t];
        if (!mok) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = t * 16 + g + 4 * q;
            if (j >= a.k) continue;
            double *cp = a.C + m + (long)j * a.ldc;
            *cp = a.beta == 0.0 ? a.alpha * sum[q] : a.alpha * sum[q] + a.beta * *cp;
        }
    }
}

// waves per workgroup: from M and Kr only (never from k) -- more waves on Kr when the rows alone would not fill the chip
static int tn_waves(int M, int Kr) { return (Kr >= 512 && M <= 4096) ? 8 : 4; }

template <int W, int KC>
static void tn_launch(hipStream_t s, const TnArgs &a, bool vec) {
    const dim3 grid((unsigned)((a.M + 15) / 16)), block(W * 64);
    if (vec) hipLaunchKernelGGL((k_gemm_tn<W, KC, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_gemm_tn<W, KC, false>), grid, block, 0, s, a);
}
template <int W>
static void tn_launch_w(hipStream_t s, const TnArgs &a, bool vec) {
    switch ((a.k + 15) / 16) {
    case 1: tn_launch<W, 1>(s, a, vec); break;
    case 2: tn_launch<W, 2>(s, a, vec); break;
    case 3: tn_launch<W, 3>(s, a, vec); break;
    default: tn_launch<W, 4>(s, a, vec); break;
    }
}

int cip_gemm_tn(hipStream_t s, int M, int k, int Kr, double alpha, const double *A, long lda, const double *B, long ldb,
                double beta, double *C, long ldc) {
    if (M <= 0 || k <= 0) return 0;
    const int W = tn_waves(M, Kr);
    for (int c0 = 0; c0 < k; c0 += 64) {
        TnArgs a{A, lda, B + (long)c0 * ldb, ldb, C + (long)c0 * ldc, ldc, M, Kr, k - c0 < 64 ? k - c0 : 64, alpha, beta};
        const bool vec = Kr % 16 == 0 && lda % 4 == 0 && ldb % 4 == 0 && !((((uintptr_t)a.A) | ((uintptr_t)a.B)) & 31);
        if (W == 8) tn_launch_w<8>(s, a, vec);
        else tn_launch_w<4>(s, a, vec);
    }
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// dst[i + j ldd] = alpha src[i + j lds] d[i]   (d == NULL: 1; src == NULL: 0) for i < rows, j < cols
__global__ __launch_bounds__(256) void k_block_copy(int rows, double alpha, const double *src, long lds, const double *d, double *dst,
                                                    long ldd) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= rows) return;
    double v = 0.0;
    if (src) {
        v = alpha * src[i + (long)j * lds];
        if (d) v *= d[i];
    }
    dst[i + (long)j * ldd] = v;
}
int cip_block_copy(hipStream_t s, int rows, int cols, double alpha, const double *src, long lds, const double *d, double *dst, long ldd) {
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(k_block_copy, dim3((unsigned)((rows + 255) / 256), (unsigned)cols), dim3(256), 0, s, rows, alpha, src, lds, d,
                       dst, ldd);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The sweeps of cip_ldlt_solve for k columns at once, 64 at a time, with a Bs x 64 scratch block S:
//   forward   S = XT_J' R_J ;  R_below -= L'_{J,below}' S ;  R_J = D^-1_J S
//   backward  S = X_J' Z_J  ;  Z_J = S ;  Z_above -= L_{J,above}' S
// Three launches per block step and sweep.  k == 1 goes through cip_ldlt_solve (same bits as the single solve) unless the caller
// solves one column of a larger set (one_is_single false: every column the same arithmetic whatever k is).
int cip_ldlt_solve_many_scratch_block(int Npad) {
    for (int b = 1024; b > CIP_NB; b >>= 1)
        if (Npad % b == 0) return b;
    return CIP_NB;
}
int cip_ldlt_solve_many(hipStream_t s, const double *K, int Npad, long ld, const LdltWorkspace &ws, double *scratch, double *B, long ldb,
                        int k, bool one_is_single) {
    if (k <= 0) return 0;
    if (k == 1 && one_is_single) return cip_ldlt_solve(s, K, Npad, ld, ws, B);
    const int Bs = ws.Bs, nbk = Npad / Bs;
    if (Bs > cip_ldlt_solve_many_scratch_block(Npad)) { cip_set_error("cip_ldlt_solve_many: solve block %d is wider than the scratch", Bs); return -3; }
    const double *X = (Bs == CIP_NB) ? ws.Linv : ws.X, *XT = (Bs == CIP_NB) ? ws.LinvT : ws.XT;
    const size_t bs2 = (size_t)Bs * Bs;
    double *S = scratch;
    int rc;
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int kc = k - c0 < 64 ? k - c0 : 64;
        double *Bc = B + (long)c0 * ldb;
        for (int J = 0; J < nbk; ++J) {
            const long C0 = (long)J * Bs;
            if ((rc = cip_ldlt_side_join(s, ws, J))) return rc;
            if ((rc = cip_gemm_tn(s, Bs, kc, Bs, 1.0, XT + J * bs2, Bs, Bc + C0, ldb, 0.0, S, Bs))) return rc;
            const int below = Npad - (int)C0 - Bs;
            if (below > 0 && (rc = cip_gemm_tn(s, below, kc, Bs, -1.0, K + C0 + (C0 + Bs) * ld, ld, S, Bs, 1.0, Bc + C0 + Bs, ldb))) return rc;
            if ((rc = cip_block_copy(s, Bs, kc, 1.0, S, Bs, ws.dinv + C0, Bc + C0, ldb))) return rc;
        }
        for (int J = nbk - 1; J >= 0; --J) {
            const long C0 = (long)J * Bs;
            if ((rc = cip_gemm_tn(s, Bs, kc, Bs, 1.0, X + J * bs2, Bs, Bc + C0, ldb, 0.0, S, Bs))) return rc;
            if ((rc = cip_block_copy(s, Bs, kc, 1.0, S, Bs, nullptr, Bc + C0, ldb))) return rc;
            if (C0 > 0 && (rc = cip_gemm_tn(s, (int)C0, kc, Bs, -1.0, K + C0, ld, S, Bs, 1.0, Bc, ldb))) return rc;
        }
    }
    return 0;
}
