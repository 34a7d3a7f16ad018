// S cones of matrix order 133 .. 2048: the stages that do not fit one workgroup's LDS.
//
// The workgroup-per-cone kernels of sdp.hip keep ONE r x r matrix LDS-resident up to r = 132; above that they ran the
// same serial chains from global memory (BASELINE config 4 at its literal size, r = 256: 67 ms per NT scaling, 10.9 ms
// per max-step, 10 ms per Schur scaling).  Here the three expensive entry points are rebuilt from chip-wide pieces, one file per row
// of the map below; which form a stage runs at which order is decided in cip_sdp_large_forms.h alone, the workspace and the
// launchers that cross files are in cip_sdp_large.h:
//
//   nestod_sdc  (src/ConicIP.jl:196-210)                                                                   sdp_large_nt.hip
//       chol(mat(z)), chol(mat(s))        the library's own blocked LDL' (ldlt.hip: MFMA trailing updates) on the matrix
//                                         padded to 256 / 512 / 1024 / 2048 with an identity block; L_chol = L D^1/2
//       G = Lz' Ls                        one fp64-MFMA GEMM (64x64 tiles over the chip; 16x16 split-k tiles at order 256)
//       svd(G): U, Lambda                 BLOCK one-sided Jacobi (k_lg_jacobi): column blocks of 8 / 16 / 8 / 4 at the four
//                                         padded orders, disjoint block pairs on different workgroups (a pair = 128 KB of
//                                         LDS), a full inner sweep per pair, ONE LAUNCH PER PHASE: the launch boundary
//                                         orders the rounds of the tournament over blocks
//       R = Lz^-T U Lambda^1/2, R^-1      GEMMs with the explicit inverse of the unit-lower factor (the block inverses the
//                                         LDL' builds for its solves: one block = the whole matrix here)
//   maxstep_sdc (src/ConicIP.jl:272-303)                                                                   sdp_large_eig.hip
//       lambda_max(L^-1 D L^-T)           LDL' + two GEMMs with inv(L), then the extreme eigenvalue by
//                                         order <= 256   Lanczos with the matrix in one workgroup's registers (k_lg_lanczos1)
//                                                        + an inertia certificate; its fallback, and CIP_LG_LANCZOS=0, is a
//                                                        Householder tridiagonalisation in registers (k_lg_tridiag1)
//                                         <= 1024        a COOPERATIVE Householder tridiagonalisation (k_lg_tridiag): each
//                                                        workgroup keeps a slab of 32 or 16 columns in LDS for the whole
//                                                        reduction; per column one grid barrier and two r-vectors through
//                                                        global memory (coherent 8-byte accesses)
//                                         above          the matrix in global memory, two launches per column (k_tg_*)
//                                         and, behind every tridiagonalisation, Sturm multisection (k_lg_sturm)
//   A' F^-1 for the Schur complement (Block * matrix, src/blockmatrices.jl:176-177; src/kktsolvers.jl:289-290)       this file
//       vecm(Rinv mat(a_i) Rinv') for all columns i: two BATCHED MFMA GEMMs per chunk of columns
//
// apply and product are two and one chip-wide GEMMs, the division by a diagonal element is element-wise; the general
// division stays on the workgroup-per-cone kernel of sdp.hip.  They are in this file too, with the workspace's creation, mat / vecm
// and the single products (k_gemm_nt_small, lg_gemm) that the other two files launch through cip_sdp_large.h.
#include "cip_sdp_large.h"
#include "cip_gemm_tile.h"
#include "cip_sdp_numerics.h"
#include "../../include/cipkkt.h"
#include <string.h>

// ------------------------------------------------------------------------------------------ element-wise pieces
// X[b] (rp x rp) = mat(x_b) in the leading r x r block, pad: `padval` on the diagonal, 0 elsewhere.
// x_b = x + b * xb, element e at stride xs (a column block of A' is strided by its leading dimension).
__global__ __launch_bounds__(256) void k_lg_mat(const double *x, long xs, long xb, double *X, int r, int rp, double padval) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)rp * rp) return;
    const int i = (int)(e % rp), j = (int)(e / rp);
    double v;
    if (i < r && j < r) {
        const int a = i < j ? i : j, b = i < j ? j : i;
        v = x[(long)blockIdx.y * xb + (long)vidx(a, b, r) * xs];
        if (a != b) v *= SQRT1_2;
    } else {
        v = (i == j) ? padval : 0.0;
    }
    X[(size_t)blockIdx.y * rp * rp + e] = v;
}
void lg_mat(hipStream_t s, const double *x, long xs, long xb, double *X, int r, int rp, double padval, int batch) {
    hipLaunchKernelGGL(k_lg_mat, dim3((unsigned)(((long)rp * rp + 255) / 256), batch), dim3(256), 0, s, x, xs, xb, X, r, rp, padval);
}
// out_b = vecm(Y_b leading r x r), strided like the input of k_lg_mat
__global__ __launch_bounds__(256) void k_lg_vecm(const double *Y, double *out, long os, long ob, int r, int rp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)r * r) return;
    const int i = (int)(e % r), j = (int)(e / r);
    if (i > j) return;
    const double y = Y[(size_t)blockIdx.y * rp * rp + i + (long)j * rp];
    out[(long)blockIdx.y * ob + (long)vidx(i, j, r) * os] = (i == j) ? y : y * SQRT2;
}
// The same for a batch of nb matrices whose vecm images are the COLUMNS i0.. of a matrix with leading dimension `os` (W' = A'F^-1:
// element e of matrix i goes to out[i + e os]): 64 entries x 64 matrices per workgroup through LDS, so that both sides move whole
// cache lines -- entry (a, b) is read from the LOWER triangle, Y[b + a rp] (consecutive entries of a vecm row are consecutive
// there; the batched GEMM in front computes the lower tiles), and 64 consecutive i are written per entry.  (One thread per entry
// and matrix wrote 8 bytes every `os` doubles: 0.35 ms per factorisation at order 256, n = 1024.)
__global__ __launch_bounds__(256) void k_lg_vecm_cols(const double *Y, int nb, double *out, long os, int r, int rp) {
    __shared__ double tile[64][65];
    const long dim = (long)r * (r + 1) / 2;
    const long e0 = (long)blockIdx.x * 64;
    const int i0 = blockIdx.y * 64;
    {
        const int el = threadIdx.x & 63, cq = threadIdx.x >> 6;
        const long e = e0 + el;
        if (e < dim) {
            int a = (int)(((double)(2 * r + 1) - sqrt((double)(2 * r + 1) * (2 * r + 1) - 8.0 * (double)e)) * 0.5);
            while (a > 0 && vrowoff(a, r) > e) --a;
            while (vrowoff(a + 1, r) <= e) ++a;
            const int b = a + (int)(e - vrowoff(a, r));
            const double sc = (a == b) ? 1.0 : SQRT2;
            for (int k = 0; k < 16; ++k) {
                const int il = cq + 4 * k;
                if (i0 + il < nb) tile[el][il] = Y[(size_t)(i0 + il) * rp * rp + b + (long)a * rp] * sc;
            }
        }
    }
    __syncthreads();
    {
        const int il = threadIdx.x & 63, eg = threadIdx.x >> 6;
        if (i0 + il < nb)
            for (int k = 0; k < 16; ++k) {
                const int el = eg + 4 * k;
                if (e0 + el < dim) out[(i0 + il) + (e0 + el) * os] = tile[el][il];
            }
    }
}
// out = vecm(Y + Y') of the leading r x r block (Jordan product X o Y = XY + YX from the one product XY)
__global__ __launch_bounds__(256) void k_lg_vecm_sym(const double *Y, double *out, int r, int rp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)r * r) return;
    const int i = (int)(e % r), j = (int)(e / r);
    if (i > j) return;
    const double y = Y[i + (long)j * rp] + Y[j + (long)i * rp];
    out[vidx(i, j, r)] = (i == j) ? y : y * SQRT2;
}
// the four padded matrices from a packed scaling handed over by the host (cip_set_scaling_packed / identity)
__global__ __launch_bounds__(256) void k_lg_pad(const double *R, const double *Ri, double *pad, int r, int rp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)rp * rp) return;
    const int i = (int)(e % rp), j = (int)(e / rp);
    const bool in = i < r && j < r;
    const double rv = in ? R[i + (long)j * r] : 0.0, iv = in ? Ri[i + (long)j * r] : 0.0;
    const long n2 = (long)rp * rp, et = j + (long)i * rp;
    pad[e] = iv; pad[n2 + et] = iv; pad[2 * n2 + e] = rv; pad[3 * n2 + et] = rv;
}
// ONE product C = A B' of padded order 256 (lg_small_product; the congruences of apply / max-step / NT scaling: ~60 per iteration of
// config 4).  The 64x64-tile kernel has 16 workgroups for it and walks K = 256 in each: 14 us on 16 of 256 CUs.  Here a workgroup owns one 16x16
// tile of C (256 workgroups at order 256) and its four waves split the k range (cip_gemm_tile.h: gemm_tile_16_splitk; operands
// from L2, 0.5 MB per matrix).
// BVEC: B is mat(xv) of a vecm vector (symmetric; zero outside the leading r x r block), read straight from the vector -- no k_lg_mat
// pass; CVEC: the result goes out as vecm (entries i <= j < r, off-diagonal ones times sqrt 2; tiles below the diagonal are not
// computed) -- no k_lg_vecm pass.  Same MFMAs on the same operands in the same order as the plain form: same bits.
template <bool BVEC, bool CVEC>
__global__ __launch_bounds__(256) void k_gemm_nt_small(const double *A, long lda, const double *B, long ldb, double *C, long ldc, int K, int r) {
    if (CVEC && blockIdx.x > blockIdx.y) return;               // (16 i0 > 16 j0 + 15 for every entry of the tile)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int kq = K >> 2;
    const double *a = A + (long)blockIdx.x * 16 + l15 + (long)(wave * kq + l4) * lda;
    const double *b = B + (long)blockIdx.y * 16 + l15 + (long)(wave * kq + l4) * ldb;
    const int jb = blockIdx.y * 16 + l15, kb0 = wave * kq + l4;      // BVEC: this lane's row of mat(xv) and its first k
    gemm_tile_16_splitk(a, lda, K,
        [&](int dk) {
            if (!BVEC) return b[(long)dk * ldb];
            const int kk = kb0 + dk;
            double v = 0.0;
            if (jb < r && kk < r) {
                const int lo = jb < kk ? jb : kk, hi = jb < kk ? kk : jb;
                v = B[vidx(lo, hi, r)];
                if (lo != hi) v *= SQRT1_2;
            }
            return v;
        },
        [&](int q, double c) {
            const int i = blockIdx.x * 16 + l15, j = blockIdx.y * 16 + l4 + 4 * q;
            if (CVEC) { if (i <= j && j < r) C[vidx(i, j, r)] = (i == j) ? c : c * SQRT2; }
            else C[i + (long)j * ldc] = c;
        });
}
void lg_gemm_from_vec(hipStream_t s, double *C, const double *A, const double *xv, int rp, int r) {
    hipLaunchKernelGGL((k_gemm_nt_small<true, false>), dim3(rp / 16, rp / 16), dim3(256), 0, s, A, (long)rp, xv, 0L, C, (long)rp, rp, r);
}
void lg_gemm_to_vec(hipStream_t s, double *outv, const double *A, const double *B, int rp, int r) {
    hipLaunchKernelGGL((k_gemm_nt_small<false, true>), dim3(rp / 16, rp / 16), dim3(256), 0, s, A, (long)rp, B, (long)rp, outv, 0L, rp, r);
}
int lg_gemm(hipStream_t s, double *C, long sC, const double *A, long sA, const double *B, long sB, int rp, int batch, int tiles) {
    if (batch == 1 && tiles == GEMM_TILES_ALL && lg_small_product(rp)) {
        hipLaunchKernelGGL((k_gemm_nt_small<false, false>), dim3(rp / 16, rp / 16), dim3(256), 0, s, A, (long)rp, B, (long)rp, C, (long)rp, rp, rp);
        CIP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    return cip_gemm_batched_64(s, rp, rp, rp, 1.0, GemmBatchIn{A, rp, sA, 0}, GemmBatchIn{B, rp, sB, 0}, GemmBatchOut{C, rp, sC, 0}, GemmBatchOut{}, batch, 1, tiles);
}
// ------------------------------------------------------------------------------------------ the workspace
int cip_sdp_large_padded(int r) { return lg_padded_order(r); }

// The one device allocation, in order; sizing is the same walk over a null base.  The two LDL' workspaces come last.
static size_t lg_ws_layout(CipLayout L, LargeWs *w, int nlarge, bool cache_mat) {
    const size_t n2 = (size_t)w->rp * w->rp;
    for (double **m : {&w->Kz, &w->Ks, &w->Tz, &w->Ts, &w->G, &w->M1, &w->M2, &w->M3, &w->G0, &w->W1, &w->W2}) *m = L.take<double>(n2);
    w->Vw = L.take<double>(nlarge * n2);
    w->Rip = L.take<double>(LG_NPAD * nlarge * n2);
    w->vec = L.take<double>(LG_V_SLOTS * (size_t)w->rp);
    w->batchX = L.take<double>(w->chunk * n2); w->batchT = L.take<double>(w->chunk * n2);
    w->amat = cache_mat ? L.take<double>((size_t)nlarge * w->ncols * n2) : nullptr;
    w->ctr = L.take<unsigned>(LG_C_WORDS);
    w->vstate = L.take<unsigned long long>(2 * (size_t)nlarge);
    for (LdltWorkspace *x : {&w->wz, &w->ws}) cip_ldlt_ws_carve(L.take<char>(cip_ldlt_ws_bytes(w->rp, 0)), w->rp, x, 0);
    return L.bytes();
}

int cip_sdp_large_create(int rmax_large, int nlarge, int ncols, LargeWs **out) {
    LargeWs *w = new LargeWs();
    const int rp = cip_sdp_large_padded(rmax_large);
    w->rp = rp;
    const size_t m2 = (size_t)rp * rp * 8;
    // columns of A per batched congruence: all n of them when the two images fit 2 GB each (round 4: at order 256, n = 1024 the
    // 16 chunks of 64 columns were 64 launches of 512 tiles -- two workgroups per CU, 40 TFLOP/s -- now two launches), at least 16
    {
        const size_t cap = ((size_t)2 << 30) / m2;
        int c = ncols > 0 ? ncols : 64;
        if ((size_t)c > cap) c = (int)cap;
        if (c < 16) c = 16;
        if (const int e = cip_env_int("CIP_LG_CHUNK", 0); e >= 1) c = e;
        w->chunk = c;
    }
    w->ncols = ncols;
    const bool cache_mat = ncols > 0 && w->chunk >= ncols && (size_t)nlarge * ncols * m2 <= ((size_t)4 << 30);
    // the two LDL' workspaces: solve block = the whole padded matrix (X = inv(L_unit) in one piece: the "triangular solves" here are
    // GEMMs with it), also at order 2048 (the calling thread's solve-block limit for the sizing and the carve)
    struct SolveBlockOverride {          // restores the thread's limit on every way out
        int saved;
        explicit SolveBlockOverride(int b) : saved(cip_tl_solve_block_max) { cip_tl_solve_block_max = b; }
        ~SolveBlockOverride() { cip_tl_solve_block_max = saved; }
    } whole_matrix_block(rp);
    const size_t bytes = lg_ws_layout(nullptr, w, nlarge, cache_mat);
    if (hipMalloc((void **)&w->base, bytes) != hipSuccess) { cip_set_error("large S cone workspace: hipMalloc of %zu bytes failed", bytes); delete w; return -3; }
    lg_ws_layout(w->base, w, nlarge, cache_mat);
    CIP_HIP_CHECK(hipMemset(w->ctr, 0, LG_C_WORDS * sizeof(unsigned)));
    CIP_HIP_CHECK(hipMemset(w->vstate, 0, 16 * (size_t)nlarge));
    if (hipHostMalloc((void **)&w->hflag, 8 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&w->hflag_dev, w->hflag, 0) != hipSuccess) {
        cip_set_error("large S cone workspace: host-mapped flag words"); if (w->hflag) (void)hipHostFree(w->hflag); (void)hipFree(w->base); delete w; return -3;
    }
    memset(w->hflag, 0, 8 * sizeof(int));
    CIP_HIP_CHECK(hipMemset(w->vec, 0, LG_V_SLOTS * (size_t)rp * sizeof(double)));
    w->wz.signs = w->ws.signs = PivotSigns{0, rp, rp};       // a Cholesky in disguise: every pivot must be positive
    w->wz.x_zeroed = &w->xz_z; w->ws.x_zeroed = &w->xz_s;
    // the three-launch panel chain: no in-launch wait that could give up (the consumers of these factors -- NT scaling, inertia
    // certificate, max-step -- read the pivot flags only, not info[3]); same bits as the fused chain
    w->wz.unfused = w->ws.unfused = 1;
    *out = w;
    return 0;
}
void cip_sdp_large_destroy(LargeWs *w) {
    if (!w) return;
    if (w->hflag) (void)hipHostFree(w->hflag);
    if (w->s2) (void)hipStreamDestroy(w->s2);
    if (w->efork) (void)hipEventDestroy(w->efork);
    if (w->ejoin) (void)hipEventDestroy(w->ejoin);
    if (cip_env_int("CIP_LG_LANCZOS_STATS", 0)) lg_lanczos_stats_print();
    if (w->base) (void)hipFree(w->base);
    delete w;
}
// padded Rinv after the host replaced the packed scaling
int cip_sdp_large_refresh(hipStream_t s, LargeWs *w, const ConeDesc &cd, int li, const double *scal) {
    const int r = cd.r, rp = w->rp;
    w->have_v[li] = 0;                                     // the next NT scaling of this cone starts its Jacobi cold
    hipLaunchKernelGGL(k_lg_pad, lg_grid((long)rp * rp), dim3(256), 0, s, scal + cd.soff, scal + cd.soff + (size_t)r * r,
                       w->Rip + LG_NPAD * (size_t)li * rp * rp, r, rp);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}
// Wt[i, off + e] = (F^-T a_i)_e = vecm(Rinv mat(a_i) Rinv')_e for every row i of At (= column of A): two batched GEMMs over all
// columns (chunks when they do not fit), the second on the lower tiles only, then the tiled vecm pass; mat(a_i) comes from the
// per-upload cache when the workspace has one
void cip_sdp_large_invalidate(LargeWs *w) {
    if (w) for (auto &p : w->amat_src) p = nullptr;
}
int cip_sdp_large_scale_At(hipStream_t s, LargeWs *w, const ConeDesc &cd, int li, int n, const double *At, long ldat, double *Wt,
                           long ldwt) {
    const int r = cd.r, rp = w->rp;
    const long n2 = (long)rp * rp;
    const double *Rip = w->Rip + LG_NPAD * (size_t)li * n2;
    const long dim = (long)r * (r + 1) / 2;
    int rc;
    const bool cached = w->amat && n == w->ncols && n <= w->chunk;
    double *amat = cached ? w->amat + (size_t)li * n * n2 : nullptr;
    if (cached && w->amat_src[li] != At) {
        dim3 gm((unsigned)((n2 + 255) / 256), n);
        hipLaunchKernelGGL(k_lg_mat, gm, dim3(256), 0, s, At + (long)cd.aoff * ldat, ldat, 1L, amat, r, rp, 0.0);
        w->amat_src[li] = At;
    }
    for (int i0 = 0; i0 < n; i0 += w->chunk) {
        const int nb = (n - i0 < w->chunk) ? (n - i0) : w->chunk;
        const double *X = amat;
        if (!cached) {
            dim3 gm((unsigned)((n2 + 255) / 256), nb);
            hipLaunchKernelGGL(k_lg_mat, gm, dim3(256), 0, s, At + i0 + (long)cd.aoff * ldat, ldat, 1L, w->batchX, r, rp, 0.0);
            X = w->batchX;
        }
        if ((rc = lg_gemm(s, w->batchT, n2, Rip, 0, X, n2, rp, nb))) return rc;                  // Rinv X      (X symmetric)
        if ((rc = lg_gemm(s, w->batchX, n2, w->batchT, n2, Rip, 0, rp, nb, GEMM_TILES_TOUCH_LOWER))) return rc;     // (Rinv X) Rinv': lower tiles, all k_lg_vecm_cols reads
        dim3 gv((unsigned)((dim + 63) / 64), (unsigned)((nb + 63) / 64));
        hipLaunchKernelGGL(k_lg_vecm_cols, gv, dim3(256), 0, s, w->batchX, nb, Wt + i0 + (long)cd.aoff * ldwt, ldwt, r, rp);
    }
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// out = vecm(P' mat(x) P), P = R (F), R' (F'), Rinv (F^-1), Rinv' (F^-T)  (VecCongurance, src/ConicIP.jl:35-40, :69):
// two chip-wide GEMMs  Y = Q X Q'  with Q = P' taken from the padded copies
int cip_sdp_large_apply(hipStream_t s, LargeWs *w, const ConeDesc &cd, int li, int mode, const double *x, double *out) {
    const int r = cd.r, rp = w->rp;
    const long n2 = (long)rp * rp;
    // pad[]: 0 Rinv, 1 Rinv', 2 R, 3 R'
    const int which = (mode == CIP_OP_F) ? 3 : (mode == CIP_OP_FT) ? 2 : (mode == CIP_OP_FINV) ? 1 : 0;
    const double *Q = w->Rip + (LG_NPAD * (size_t)li + which) * n2;
    int rc;
    if (lg_small_product(rp)) {
        // two launches: mat(x) is read from the vector by the first product, the second writes vecm (k_gemm_nt_small<BVEC / CVEC>)
        lg_gemm_from_vec(s, w->M2, Q, x + cd.off, rp, r);
        lg_gemm_to_vec(s, out + cd.off, w->M2, Q, rp, r);
        CIP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(k_lg_mat, lg_grid(n2), dim3(256), 0, s, x + cd.off, 1L, 0L, w->M1, r, rp, 0.0);
    if ((rc = lg_gemm(s, w->M2, 0, Q, 0, w->M1, 0, rp, 1))) return rc;              // Q X      (X symmetric)
    if ((rc = lg_gemm(s, w->M3, 0, w->M2, 0, Q, 0, rp, 1))) return rc;              // (Q X) Q'
    hipLaunchKernelGGL(k_lg_vecm, lg_grid((long)r * r), dim3(256), 0, s, w->M3, out + cd.off, 1L, 0L, r, rp);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// Jordan division by a DIAGONAL element (dsdc!, src/ConicIP.jl:347-353, with Y = diag(y): every division of the interior-point loop
// is by lambda = vecm(diag(Lambda)), :686): O_ij = X_ij / (y_i + y_j), element-wise on the vecm layout (the sqrt(2) of the off-diagonal
// entries cancels) -- chip-wide, one workgroup per matrix row, instead of one workgroup walking mat / divide / vecm over r^2
// entries (225 us at order 256).  k_lg_div_check raises flag[0] when y has a non-zero off-diagonal entry; k_lg_div_diag writes the
// quotient when it has none; the general kernel (sdp.hip: k_sdp_div) runs behind them and returns at once unless the flag is up.
__global__ __launch_bounds__(256) void k_lg_div_check(const double *y, int r, int *flag) {
    const int i = blockIdx.x;
    const double *row = y + vrowoff(i, r);
    int bad = 0;
    for (int j = 1 + threadIdx.x; j < r - i; j += 256) bad |= (row[j] != 0.0);
    if (threadIdx.x == 0 && !(row[0] == row[0])) bad = 1;                  // NaN on the diagonal: let the general path propagate it
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}
__global__ __launch_bounds__(256) void k_lg_div_diag(const double *x, const double *y, double *out, int r, const int *flag) {
    if (*flag) return;
    const int i = blockIdx.x;
    const long o = vrowoff(i, r);
    const double yi = y[o];
    for (int j = threadIdx.x; j < r - i; j += 256) out[o + j] = x[o + j] / (yi + y[vrowoff(i + j, r)]);
}
// returns with flag[0] = 1 when the general path must run for this cone (the caller launches it; it resets the flag)
int cip_sdp_large_div(hipStream_t s, LargeWs *w, const ConeDesc &cd, const double *x, const double *y, double *out, int *flag) {
    (void)w;
    hipLaunchKernelGGL(k_lg_div_check, dim3(cd.r), dim3(256), 0, s, y + cd.off, cd.r, flag);
    hipLaunchKernelGGL(k_lg_div_diag, dim3(cd.r), dim3(256), 0, s, x + cd.off, y + cd.off, out + cd.off, cd.r, (const int *)flag);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// out = x o y = vecm(XY + YX)  (xsdc!, src/ConicIP.jl:355-360): one chip-wide GEMM
int cip_sdp_large_prod(hipStream_t s, LargeWs *w, const ConeDesc &cd, const double *x, const double *y, double *out) {
    const int r = cd.r, rp = w->rp;
    const long n2 = (long)rp * rp;
    int rc;
    hipLaunchKernelGGL(k_lg_mat, lg_grid(n2), dim3(256), 0, s, x + cd.off, 1L, 0L, w->M1, r, rp, 0.0);
    hipLaunchKernelGGL(k_lg_mat, lg_grid(n2), dim3(256), 0, s, y + cd.off, 1L, 0L, w->M2, r, rp, 0.0);
    if ((rc = lg_gemm(s, w->M3, 0, w->M1, 0, w->M2, 0, rp, 1))) return rc;          // X Y'  = X Y  (Y symmetric)
    hipLaunchKernelGGL(k_lg_vecm_sym, lg_grid((long)r * r), dim3(256), 0, s, w->M3, out + cd.off, r, rp);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}
