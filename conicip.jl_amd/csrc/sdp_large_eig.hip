// maxstep_sdc (src/ConicIP.jl:272-303) for an S cone of order 133 .. 2048: the extreme eigenvalue of the max-step's matrix by the
// form cip_sdp_large_forms.h names for its order (lg_eig_form) -- Lanczos with its inertia certificate, or one of three Householder
// tridiagonalisations followed by Sturm multisection -- and the verdict.  sdp_large.hip has the map of the whole large path.
#include "cip_sdp_large.h"
#include "cip_sdp_numerics.h"
#include "../../include/cipkkt.h"
#include <stdio.h>

#define LG_T 1024

__device__ int g_lz_hist[40];           // k_lg_lanczos1: histogram of step counts (bins of 8)
void lg_lanczos_stats_print(void) {
    int st[40];
    if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_lz_hist), sizeof(st)) != hipSuccess) return;
    fprintf(stderr, "lanczos max-step, steps per call (bins of 8):");
    for (int q = 0; q <= 32; ++q) if (st[q]) fprintf(stderr, " [%d-%d]: %d", 8 * q, 8 * q + 7, st[q]);
    fprintf(stderr, "\n");
}
// grid barrier for the workgroups of a cooperative launch (all resident: at most 64 of them, order 1024 in slabs of 16): monotonic counter,
// every thread drains its stores, one lane arrives and polls (`sc1` loads).  Bounded spin (cip_bounded_wait) -> *err.
__device__ __forceinline__ void lg_grid_barrier(unsigned *ctr, unsigned nwg, unsigned &phase, int *err) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ++phase;
    if (threadIdx.x == 0) {
        atomicAdd(ctr, 1u);
        cip_bounded_wait<1>([&] { return __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= nwg * phase; }, err,
                            CIP_GIVEUP_XWG);
    }
    __syncthreads();
}
// ------------------------------------------------------------------------------------------ cooperative tridiagonalisation
// A = the symmetric r x r matrix  0.5 (M + M') .* (rs rs')  (rs == NULL: no scaling), column slab [slab w, slab w + slab) in the
// LDS of workgroup w for the whole reduction.  Output: dg[0..r), of[0..r-1) (sub-diagonal).  Householder by columns
// exactly as sd_extreme_eig (sdp.hip) does it in one workgroup.
// ONE grid barrier per column: beside its entries of p = beta A v every step also publishes the NOT YET UPDATED next
// column (by its owner), so that after the barrier every workgroup can form the updated next column -- the Householder
// vector of the following step -- by itself:  a[:, k+1] - v w_0 - w v_0.
__global__ __launch_bounds__(LG_T) void k_lg_tridiag(const double *M, int ldm, const double *dscale, int r, double *dg, double *of,
                                                      double *xbuf /* 2 x ldm */, double *pbuf /* 2 x ldm */, unsigned *ctr, int *err, int slab) {
    extern __shared__ double sh[];
    const int tid = threadIdx.x;
    const int nwg = gridDim.x, w = blockIdx.x;
    const int c0 = w * slab, ncol = (r - c0 < slab) ? (r - c0) : slab;
    const int ld = r | 1;
    double *a = sh;                                  // slab: a[i + c * ld]
    double *v = sh + (size_t)slab * ld, *wv = v + r, *vn = wv + r, *red = vn + r;
    unsigned phase = 0;
    for (int e = tid; e < ncol * r; e += LG_T) {
        const int i = e % r, c = e / r, j = c0 + c;
        a[i + c * ld] = sd_scaled_sym_entry(M, ldm, dscale, i, j);
    }
    __syncthreads();
    // column `col` below its diagonal, as it stands in the owner's slab -> xb
    auto publish = [&](int col, double *xb) {
        if (col / slab == w) {
            const int cc = col - c0, mm = r - col - 1;
            for (int i = tid; i < mm; i += LG_T) lg_st(xb + i, a[(col + 1 + i) + cc * ld]);
        }
    };
    publish(0, xbuf);
    lg_grid_barrier(ctr, nwg, phase, err);
    for (int i = tid; i < r - 1; i += LG_T) v[i] = lg_ld(xbuf + i);
    __syncthreads();
    for (int k = 0; k + 1 < r; ++k) {
        const int m = r - k - 1;
        const int owner = k / slab, kc = k - owner * slab;
        double *xb = xbuf + (size_t)((k + 1) & 1) * ldm, *pb = pbuf + (size_t)(k & 1) * ldm;
        if (w == owner && tid == 0) dg[k] = a[k + kc * ld];
        double part = 0.0;
        for (int i = tid; i < m; i += LG_T) part += v[i] * v[i];
        const double sigma = sd_block_sum(part, red, LG_T / 64, SdSyncAll());
        const double x0 = v[0];
        if (m == 1) { if (w == owner && tid == 0) of[k] = x0; break; }
        const SdReflector h = sd_reflector(sigma, x0);       // flat: already tridiagonal in this column (uniform over the grid)
        const bool flat = h.flat;
        const double alpha = h.alpha, beta = h.beta;
        __syncthreads();
        if (tid == 0) { if (!flat) v[0] = x0 - alpha; if (w == owner) of[k] = alpha; }
        __syncthreads();
        if (!flat) {
            // p_j = beta sum_i A[i, j] v_i for the slab's columns j > k: 32 lanes per column
            const int c = tid >> 5, l32 = tid & 31, j = c0 + c;
            if (c < ncol && j > k) {
                double acc = 0.0;
                const double *col = a + (k + 1) + c * ld;
                for (int i = l32; i < m; i += 32) acc += col[i] * v[i];
                for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                if (l32 == 0) lg_st(pb + (j - k - 1), beta * acc);
            }
        }
        publish(k + 1, xb);                                  // the next column BEFORE this step's update
        lg_grid_barrier(ctr, nwg, phase, err);
        if (flat) {
            for (int i = tid; i < m - 1; i += LG_T) v[i] = lg_ld(xb + i);
            __syncthreads();
            continue;
        }
        part = 0.0;
        for (int i = tid; i < m; i += LG_T) { const double p = lg_ld(pb + i); wv[i] = p; part += p * v[i]; }
        const double kk = 0.5 * beta * sd_block_sum(part, red, LG_T / 64, SdSyncAll());
        for (int i = tid; i < m; i += LG_T) wv[i] -= kk * v[i];
        __syncthreads();
        // A22 -= v w' + w v' on the slab's columns j > k
        for (int e = tid; e < ncol * m; e += LG_T) {
            const int i = e % m, c = e / m, j = c0 + c;
            if (j > k) a[(k + 1 + i) + c * ld] -= v[i] * wv[j - k - 1] + wv[i] * v[j - k - 1];
        }
        // the updated column k+1 below its diagonal = next step's x, formed by everybody
        for (int i = tid; i < m - 1; i += LG_T) vn[i] = lg_ld(xb + i) - (v[i + 1] * wv[0] + wv[i + 1] * v[0]);
        __syncthreads();
        double *t = v; v = vn; vn = t;
    }
    if ((r - 1) / slab == w && tid == 0) { dg[r - 1] = a[(r - 1) + ((r - 1) - c0) * ld]; of[r - 1] = 0.0; }
}
// ---- Householder tridiagonalisation of a symmetric matrix of order r <= 256 by ONE workgroup, the matrix in REGISTERS.
// The cooperative kernel above pays a grid barrier and two coherent global round trips per column (5.7 us x 255 columns
// at r = 256: 76 % of a max-step).  A CU's register file holds what its LDS cannot: 512 threads (two waves per SIMD: 256
// registers each) as a 32 x 16 grid, thread (tr, tc) owning the entries (i, j) with i = tr (mod 32), j = tc (mod 16) of the
// blocks on or below the block diagonal -- 72 of the 128 blocks of 32 x 16, the 32 x 32 diagonal blocks whole -- in 72
// doubles.  A Householder step is then
//   column k -> LDS, norm, v (zero outside the active rows), p = A v as 8 row + 16 column partial sums per thread reduced
//   through two LDS images (row parts over tc, column parts over tr), w = p - (beta v'p / 2) v, rank-2 update from LDS
//   copies of v and w (zero-padded: finished rows and columns take no part, no index tests in the inner loops)
// with workgroup barriers only.  Same reflectors as k_lg_tridiag; d and e go to the same Sturm kernel.
// Measured at r = 256: 1.17 ms against 1.45 ms for the cooperative kernel (max-step 1.45 against 1.75 ms).  Phases switched off
// one at a time: barriers + norm + scalars 1.3 us per column, rank-2 update 1.4, A v 1.0, the reduction of its partial sums 0.7,
// column extraction 0.15 -- the arithmetic of a column (2.6e5 flop) is now one CU's (0.85 + 0.43 us at its fp64 rate), which
// is the floor of this form.  (A 1024-thread version with 36 doubles per thread was built first: at four waves per SIMD the
// budget is 128 registers, 23 of the 36 spilled, 22 us per column; and `break` / `continue` inside the column loop made the
// compiler spill the register matrix around the exits even at 256 registers: 16 us per column.)
#define T1_LDS_DOUBLES (256 * 17 + 32 * 256 + 4 * 256 + 64)     // row parts, column parts, 2 column buffers, v, p, reduction scratch
template <int KB>
__device__ __forceinline__ void t1_extract(const double (&a)[8][16], double *xs, int tr) {      // column block KB (16 wide)
#pragma unroll
    for (int ai = KB / 2; ai < 8; ++ai) xs[32 * ai + tr] = a[ai][KB];
}__global__ __launch_bounds__(512) void k_lg_tridiag1(const double *M, int ldm, const double *dscale, int r, double *dg, double *of, const int *gate) {
    extern __shared__ double sh[];
    if (gate && !gate[0]) return;                              // (the fallback behind a passed inertia certificate)
    double *rowp = sh, *colp = sh + 256 * 17;                 // partial sums: [i][tc] (pitch 17) and [tr][j]
    double *xs0 = colp + 32 * 256, *vs = xs0 + 512, *red = vs + 512;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    // (the same load stands in k_lg_lanczos1: behind a shared inline function both kernels keep their register counts, but their code comes out different)
    double a[8][16];                                           // blocks bj <= 2 ai + 1 only
#pragma unroll
    for (int ai = 0; ai < 8; ++ai)
#pragma unroll
        for (int bj = 0; bj < 16; ++bj) {
            if (bj <= 2 * ai + 1) {
                a[ai][bj] = 0.0;
                const int i = 32 * ai + tr, j = 16 * bj + tc;
                if (i < r && j < r) a[ai][bj] = sd_scaled_sym_entry(M, ldm, dscale, j, i);       // (tc runs along j: the coalesced load of the pair)
            }
        }
    double *ps = vs + 256;                                    // p, read back by everybody
    // columns 0 .. r-2 (the last one only hands out d and e: its "reflector" is 1 x 1).  Five barriers per column; the column
    // buffer alternates, so the next column's extraction may start while slower waves still read this one's
    for (int k = 0; k + 1 < r; ++k) {
        const int kb = k >> 4, kc = k & 15;
        double *xs = xs0 + (k & 1) * 256;
        // ---- column k -> xs (rows of the stored blocks: everything below the diagonal, and d_k); readers mask by index
        if (tc == kc) {
            switch (kb) {
                case 0: t1_extract<0>(a, xs, tr); break;
                case 1: t1_extract<1>(a, xs, tr); break;
                case 2: t1_extract<2>(a, xs, tr); break;
                case 3: t1_extract<3>(a, xs, tr); break;
                case 4: t1_extract<4>(a, xs, tr); break;
                case 5: t1_extract<5>(a, xs, tr); break;
                case 6: t1_extract<6>(a, xs, tr); break;
                case 7: t1_extract<7>(a, xs, tr); break;
                case 8: t1_extract<8>(a, xs, tr); break;
                case 9: t1_extract<9>(a, xs, tr); break;
                case 10: t1_extract<10>(a, xs, tr); break;
                case 11: t1_extract<11>(a, xs, tr); break;
                case 12: t1_extract<12>(a, xs, tr); break;
                case 13: t1_extract<13>(a, xs, tr); break;
                case 14: t1_extract<14>(a, xs, tr); break;
                default: t1_extract<15>(a, xs, tr); break;
            }
        }
        __syncthreads();                                                                        // (1)
        if (tid == 0) dg[k] = xs[k];
        // ---- sigma = |x(k+1:)|^2
        double part = 0.0;
        if (tid < 256 && tid > k && tid < r) part = xs[tid] * xs[tid];
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (tid < 256 && (tid & 63) == 0) red[(k & 1) * 4 + (tid >> 6)] = part;
        __syncthreads();                                                                        // (2)
        const double *rs = red + (k & 1) * 4;
        const double sigma = (rs[0] + rs[1]) + (rs[2] + rs[3]);
        const double x0 = xs[k + 1];
        // flat: already tridiagonal in this column (always so for the last one); the reflector is then the identity:
        // beta = 0 makes p, w and the update vanish -- one code path, no divergent loop exits around the register matrix
        const SdReflector h = sd_reflector(sigma, x0);
        const bool flat = h.flat;
        const double alpha = h.alpha, beta = h.beta;
        if (tid == 0) of[k] = alpha;
        if (tid < 256) vs[tid] = (tid > k && tid < r && !flat) ? (tid == k + 1 ? x0 - alpha : xs[tid]) : 0.0;
        __syncthreads();                                                                        // (3)
        // ---- p = A v: row parts (all stored blocks) and column parts (blocks strictly below the 32 x 32 diagonal blocks)
        {
            double t16[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) t16[q] = vs[16 * q + tc];
#pragma unroll
            for (int ai = 0; ai < 8; ++ai) {
                double pr = 0.0;
#pragma unroll
                for (int bj = 0; bj <= 2 * ai + 1; ++bj) pr = fma(a[ai][bj], t16[bj], pr);
                rowp[(32 * ai + tr) * 17 + tc] = pr;
            }
            double t8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t8[q] = vs[32 * q + tr];
#pragma unroll
            for (int bj = 0; bj < 16; ++bj) {
                double pc = 0.0;
#pragma unroll
                for (int ai = bj / 2 + 1; ai < 8; ++ai) pc = fma(a[ai][bj], t8[ai], pc);
                colp[tr * 256 + 16 * bj + tc] = pc;
            }
        }
        __syncthreads();                                                                        // (4)
        {
            double pj = 0.0;
            if (tid < 256) {
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int q = 0; q < 16; ++q) s0 += rowp[tid * 17 + q];
#pragma unroll 8
                for (int q = 0; q < 32; ++q) s1 += colp[q * 256 + tid];
                pj = (tid > k && tid < r) ? beta * (s0 + s1) : 0.0;
                ps[tid] = pj;
            }
            part = (tid < 256) ? pj * vs[tid] : 0.0;
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
            if (tid < 256 && (tid & 63) == 0) red[8 + (k & 1) * 4 + (tid >> 6)] = part;
        }
        __syncthreads();                                                                        // (5)
        const double *rk = red + 8 + (k & 1) * 4;
        const double kk = 0.5 * beta * ((rk[0] + rk[1]) + (rk[2] + rk[3]));
        // ---- A -= v w' + w v',  w = p - kk v
        {
            double t16[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) { const int j = 16 * q + tc; t16[q] = ps[j] - kk * vs[j]; }
#pragma unroll
            for (int ai = 0; ai < 8; ++ai) {                    // - v w'
                const double vi = vs[32 * ai + tr];
#pragma unroll
                for (int bj = 0; bj <= 2 * ai + 1; ++bj) a[ai][bj] = fma(-vi, t16[bj], a[ai][bj]);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) t16[q] = vs[16 * q + tc];
#pragma unroll
            for (int ai = 0; ai < 8; ++ai) {                    // - w v'
                const int i = 32 * ai + tr;
                const double wi = ps[i] - kk * vs[i];
#pragma unroll
                for (int bj = 0; bj <= 2 * ai + 1; ++bj) a[ai][bj] = fma(-wi, t16[bj], a[ai][bj]);
            }
        }
        // (no barrier here: the next column's extraction writes the OTHER column buffer; vs, ps and red are next written
        //  behind barriers (2), (4) and (1) of the next column, which every reader of this column's values has passed by then)
    }
    __syncthreads();
    // the last diagonal entry
    if (tr == ((r - 1) & 31) && tc == ((r - 1) & 15)) {
        double dlast = 0.0;
#pragma unroll
        for (int ai = 0; ai < 8; ++ai)
#pragma unroll
            for (int bj = 2 * ai; bj <= 2 * ai + 1; ++bj)
                if (ai == ((r - 1) >> 5) && bj == ((r - 1) >> 4)) dlast = a[ai][bj];
        dg[r - 1] = dlast; of[r - 1] = 0.0;
    }
}
// ---- Orders above 1024: the slabs of the cooperative kernel no longer fit the LDS of 256 resident workgroups.  The matrix lives in
// global memory (A, full symmetric storage, both triangles kept up to date) and a Householder step is TWO launches, the launch
// boundary in place of the grid barrier:
//   k_tg_symv   every workgroup forms the reflector of column k for itself (x = A[k+1:, k], at most 2047 entries: sigma, alpha, beta, v --
//               exactly k_lg_tridiag's), workgroup 0 stores v, beta and d_k, e_k; then p_j = beta A22[:, j] . v, one wave per column j
//   k_tg_rank2  every workgroup forms kk = beta v'p / 2 for itself; A22 -= v w' + w v' with w = p - kk v, one 64 x 64 tile each
// 2 (r - 1) launches, 8 r^3 bytes in all: ~35 ms at order 2048.  Same reflectors as the other two forms; d and e go to k_lg_sturm.
__global__ __launch_bounds__(256) void k_tg_init(const double *M, int ldm, const double *dscale, int r, double *A, int lda) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)r * r) return;
    const int i = (int)(e % r), j = (int)(e / r);
    A[i + (long)j * lda] = sd_scaled_sym_entry(M, ldm, dscale, i, j);
}
__device__ __forceinline__ double tg_block_sum(double x, double *red) {          // 256 threads; every thread gets the sum
    x = cip_wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// scal: [0] beta, [1] flat (1.0: nothing to do in this column)
__global__ __launch_bounds__(256) void k_tg_symv(const double *A, int lda, int r, int k, double *vbuf, double *pbuf, double *dg, double *of, double *scal) {
    __shared__ double red[4];
    __shared__ double vs[2048];
    const int tid = threadIdx.x, m = r - k - 1;
    const double *x = A + (k + 1) + (long)k * lda;
    double part = 0.0;
    for (int i = tid; i < m; i += 256) { const double xi = x[i]; vs[i] = xi; part += xi * xi; }
    const double sigma = tg_block_sum(part, red);
    const double x0 = vs[0];
    const SdReflector h = sd_reflector(sigma, x0, m == 1);
    const bool flat = h.flat;
    const double alpha = h.alpha, beta = h.beta;
    if (blockIdx.x == 0 && tid == 0) {
        dg[k] = A[k + (long)k * lda];
        of[k] = alpha;
        if (m == 1) { dg[r - 1] = A[(r - 1) + (long)(r - 1) * lda]; of[r - 1] = 0.0; }
        scal[0] = beta; scal[1] = flat ? 1.0 : 0.0;
    }
    if (flat) return;
    if (tid == 0) vs[0] = x0 - alpha;
    __syncthreads();
    if (blockIdx.x == 0) for (int i = tid; i < m; i += 256) vbuf[i] = vs[i];
    const int lane = tid & 63, j = blockIdx.x * 4 + (tid >> 6);
    if (j >= m) return;
    const double *col = A + (k + 1) + (long)(k + 1 + j) * lda;
    double acc = 0.0;
    for (int i = lane; i < m; i += 64) acc = fma(col[i], vs[i], acc);
    acc = cip_wave_sum(acc);
    if (lane == 0) pbuf[j] = beta * acc;
}
__global__ __launch_bounds__(256) void k_tg_rank2(double *A, int lda, int r, int k, const double *vbuf, const double *pbuf, const double *scal) {
    __shared__ double red[4];
    __shared__ double vi[64], wi[64], vj[64], wj[64];
    if (scal[1] != 0.0) return;
    const int tid = threadIdx.x, m = r - k - 1;
    const double beta = scal[0];
    double part = 0.0;
    for (int i = tid; i < m; i += 256) part += pbuf[i] * vbuf[i];
    const double kk = 0.5 * beta * tg_block_sum(part, red);
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    if (tid < 64) {
        const int i = i0 + tid;
        const double v = i < m ? vbuf[i] : 0.0, p = i < m ? pbuf[i] : 0.0;
        vi[tid] = v; wi[tid] = p - kk * v;
    } else if (tid < 128) {
        const int j = j0 + tid - 64;
        const double v = j < m ? vbuf[j] : 0.0, p = j < m ? pbuf[j] : 0.0;
        vj[tid - 64] = v; wj[tid - 64] = p - kk * v;
    }
    __syncthreads();
    const int ti = tid & 63, tq = tid >> 6;
    if (i0 + ti >= m) return;
    double *a = A + (k + 1 + i0 + ti) + (long)(k + 1 + j0) * lda;
    const double v_i = vi[ti], w_i = wi[ti];
#pragma unroll 4
    for (int c = tq; c < 64; c += 4)
        if (j0 + c < m) a[(long)c * lda] -= v_i * wj[c] + w_i * vj[c];
}
static int lg_tridiag_stepped(hipStream_t s, LargeWs *w, const double *M, const double *dscale, int r, double *work) {
    const int rp = w->rp;
    double *dg = w->dg(), *of = w->of(), *vbuf = w->slot(LG_V_XBUF), *pbuf = w->slot(LG_V_PBUF), *scal = w->slot(LG_V_SCAL);
    hipLaunchKernelGGL(k_tg_init, lg_grid((long)r * r), dim3(256), 0, s, M, rp, dscale, r, work, rp);
    for (int k = 0; k + 1 < r; ++k) {
        const int m = r - k - 1;
        hipLaunchKernelGGL(k_tg_symv, dim3((m + 3) / 4), dim3(256), 0, s, (const double *)work, rp, r, k, vbuf, pbuf, dg, of, scal);
        if (m > 1) hipLaunchKernelGGL(k_tg_rank2, dim3((m + 63) / 64, (m + 63) / 64), dim3(256), 0, s, work, rp, r, k, (const double *)vbuf, (const double *)pbuf, (const double *)scal);
    }
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}
// extreme eigenvalue of the tridiagonal (dg, of) by multisection on the Sturm count (one workgroup), then the max-step
// verdict of maxstep_sdc (src/ConicIP.jl:272-303): partial[item] <- Inf / 1/(scale lambda_max) / the `nothing` variant
__global__ __launch_bounds__(LG_T) void k_lg_sturm(const double *dgg, const double *ofg, int r, int want_max, double scale,
                                                    const int *info, double *partial, int item, const int *gate = nullptr) {
    if (gate && !gate[0]) return;
    __shared__ double dg[2048], of[2048], red[64];
    __shared__ int first;
    const int tid = threadIdx.x;
    if (info && info[0]) {                                   // X not positive definite -> Inf (:277-280)
        if (tid == 0) partial[item] = __builtin_inf();
        return;
    }
    for (int i = tid; i < r; i += LG_T) { dg[i] = dgg[i]; of[i] = ofg[i]; }
    __syncthreads();
    const double ev = sd_tridiag_extreme(dg, of, r, want_max != 0, LG_T, red, &first, SdSyncAll());
    if (tid == 0) partial[item] = sd_maxstep_verdict(want_max != 0, ev, scale);
}
// ---- The max-step needs ONE eigenvalue -- the largest (or smallest) -- of its symmetric r x r matrix, not the tridiagonal
// form: Lanczos (round 6: the plain three-term recurrence by default, the Gram-Schmidt sweeps below behind CIP_LG_LANCZOS_REORTH=1:
// lz_reorth), the matrix in registers as in k_lg_tridiag1 (same load, same p = A v), and the
// verdict of maxstep_sdc (src/ConicIP.jl:272-303) in the same launch (round 3; replaces k_lg_tridiag1 + k_lg_sturm for
// r <= 256: 1.15 + 0.28 ms per max-step, six max-steps per iteration, half of config 4's time).
//   v_1 fixed (every component non-zero inside the r x r block, zero in the padding: the padded rows never enter);
//   step j:  w = A v_j, alpha_j = w'v_j, w orthogonalised against v_1..v_j twice (classical Gram-Schmidt, "twice is
//   enough": it also removes alpha_j v_j and beta_{j-1} v_{j-1}), beta_j = |w|, v_{j+1} = w / beta_j;
//   at j = 8, 12, .., 32, 40, .., 64, 80, ..: theta = the wanted extreme eigenvalue of T_j by multisection on the Sturm
//   count (512 shifts per round, down to the last bit), s = its eigenvector by one inverse iteration with the shift at the
//   OUTER end of the final bracket (T - sigma I is then definite: the LDL' sweep needs no pivoting), and the classical
//   bound: A has an eigenvalue within beta_j |s_j| of theta.  Stop at beta_j |s_j| <= 1e-11 |T|; at j = r the recurrence is
//   a complete tridiagonalisation and theta is exact -- the fallback is the loop's own end.
// theta <= lambda_max always (Ritz values lie inside the spectrum); that the largest Ritz value converges to lambda_max
// and not to a smaller eigenvalue rests on v_1 not being orthogonal to the extreme eigenvector, as in every Krylov eigensolver.
// On the max-step matrices of config 4's family the stop comes after 9-90 steps, 30 on average; the eigenvalue then agrees
// with LAPACK's to 1e-15 (the bound is quadratic in the residual when the eigenvalue is isolated).  Deterministic: fixed
// start, fixed order of every sum.
#define LZ_LDSV 64                      // Lanczos vectors kept in LDS; the later ones in a global scratch (L2)
#define LZ_LDS_DOUBLES (256 + 8 * 256 + 256 * 6 + 64 + LZ_LDSV * 256)
// 1/x to ~1 ulp (hardware estimate + one Newton step): the Sturm counts only look at signs, the inverse iteration only
// feeds a convergence test
__device__ __forceinline__ double lz_rcp(double x) {
    const double r0 = __builtin_amdgcn_rcp(x);
    return fma(fma(-x, r0, 1.0), r0, r0);
}
__device__ __forceinline__ double lz_sum256(double x, double *red, int slot) {      // sum over threads 0..255 (4 waves), all 512 threads call
    const int tid = threadIdx.x;
    x = lz_sum_rows(lz_sum16(x));
    if (tid < 256 && (tid & 63) == 0) red[slot * 4 + (tid >> 6)] = x;
    __syncthreads();
    return (red[slot * 4] + red[slot * 4 + 1]) + (red[slot * 4 + 2] + red[slot * 4 + 3]);
}
__global__ __launch_bounds__(512) void k_lg_lanczos1(const double *M, int ldm, const double *dscale, int r, int want_max, double scale,
                                                      const int *info, double *partial, int item, double *Vg, int *stat, double *cert, double cert_tol, int reorth) {
    extern __shared__ double sh[];
    double *rowp = sh, *colp = sh + 256;                      // p = A v: row sums [i], column sums per wave [wave][j]
    double *vs = colp + 8 * 256, *wsv = vs + 256, *al = wsv + 256, *be = al + 256, *hb = be + 256, *zz = hb + 256;
    double *red = zz + 256, *Vl = red + 64;
    __shared__ int s_first;
    __shared__ double s_res[4];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const double INF = __builtin_inf();
    if (info && info[0]) {                                     // X not positive definite -> Inf (:277-280)
        if (tid == 0) { partial[item] = INF; if (stat) stat[0] = 0; if (cert) { cert[0] = 0.0; cert[1] = 1.0; } }
        return;
    }
    // (k_lg_tridiag1's load, repeated: behind a shared inline function both kernels keep their register counts, but their code comes out different)
    double a[8][16];                                           // blocks bj <= 2 ai + 1 only (k_lg_tridiag1's layout)
#pragma unroll
    for (int ai = 0; ai < 8; ++ai)
#pragma unroll
        for (int bj = 0; bj < 16; ++bj) {
            if (bj <= 2 * ai + 1) {
                a[ai][bj] = 0.0;
                const int i = 32 * ai + tr, j = 16 * bj + tc;
                if (i < r && j < r) a[ai][bj] = sd_scaled_sym_entry(M, ldm, dscale, j, i);       // (tc runs along j: the coalesced load of the pair)
            }
        }
    // LDS copy of v_k: element i at k 256 + (i ^ 8 (k & 7)) -- the eight vectors a wave reads together in the dot products
    // (eight lanes each, eight consecutive elements) then sit in different banks; a whole vector read by 256 threads is a permutation
    auto vput = [&](int k, int i, double x) { if (k < LZ_LDSV) Vl[k * 256 + (i ^ ((k & 7) << 3))] = x; else __builtin_nontemporal_store(x, Vg + (size_t)(k - LZ_LDSV) * 256 + i); };
    // v_1
    double vi = 0.0;
    if (tid < r) vi = cos(0.7 * tid + 0.3) + 1.0 / (1.0 + tid);
    {
        const double n2 = lz_sum256(tid < 256 ? vi * vi : 0.0, red, 0);
        vi *= 1.0 / sqrt(n2);
    }
    if (tid < 256) { vs[tid] = vi; vput(0, tid, vi); }
    __syncthreads();
    int m = 0;
    double th_lo = 0.0, th_hi = 0.0, ascale = 0.0, prev_lo = 0.0;
    bool done = false, have_prev = false;
    for (int j = 0; j < r && !done; ++j) {
        // ---- w = A v_j: row parts (all stored blocks) summed over the 16 lanes of a row of the thread grid, column parts (blocks
        // strictly below the 32 x 32 diagonal blocks) over the wave's four grid rows, then over the eight waves through LDS
        {
            double t16[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) t16[q] = vs[16 * q + tc];
#pragma unroll
            for (int ai = 0; ai < 8; ++ai) {
                double pr = 0.0;
#pragma unroll
                for (int bj = 0; bj <= 2 * ai + 1; ++bj) pr = fma(a[ai][bj], t16[bj], pr);
                pr = lz_sum16(pr);
                if (tc == 0) rowp[32 * ai + tr] = pr;
            }
            double t8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t8[q] = vs[32 * q + tr];
#pragma unroll
            for (int bj = 0; bj < 16; ++bj) {
                double pc = 0.0;
#pragma unroll
                for (int ai = bj / 2 + 1; ai < 8; ++ai) pc = fma(a[ai][bj], t8[ai], pc);
                pc = lz_sum_rows(pc);
                if ((tid & 63) < 16) colp[(tid >> 6) * 256 + 16 * bj + tc] = pc;
            }
        }
        __syncthreads();
        double wi = 0.0;
        if (tid < 256) {
            double s1 = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s1 += colp[q * 256 + tid];
            wi = rowp[tid] + s1;
        }
        // ---- the recurrence's own terms first: w -= beta_{j-1} v_{j-1}, alpha_j = v_j'w, w -= alpha_j v_j.  (Taking them out
        // in the Gram-Schmidt sweep with everything else needs its second pass at EVERY step: they are the large components,
        // and with a basis orthogonal to delta the sweep then puts delta |alpha| / beta of them back along the old vectors.)
        if (tid < 256 && j > 0) {
            const int k = j - 1;
            const double vp = k < LZ_LDSV ? Vl[k * 256 + (tid ^ ((k & 7) << 3))] : __builtin_nontemporal_load(Vg + (size_t)(k - LZ_LDSV) * 256 + tid);
            wi = fma(-be[k], vp, wi);
        }
        double alpha = lz_sum256(tid < 256 ? wi * vs[tid] : 0.0, red, 2);
        if (tid < 256) { wi = fma(-alpha, vs[tid], wi); wsv[tid] = wi; }
        __syncthreads();
        // ---- then w orthogonal to v_0 .. v_j by classical Gram-Schmidt: what it finds is rounding noise while the basis is
        // orthogonal; a second sweep when the first one took out a sizeable part of w ("twice is enough")
        double nrm2 = 0.0;
        if (!reorth) nrm2 = lz_sum256(tid < 256 ? wi * wi : 0.0, red, 0);       // plain three-term Lanczos (the default since round 6: see lz_reorth)
        for (int pass = 0; pass < (reorth ? 2 : 0); ++pass) {
            {                                                  // h_k = v_k'w: eight threads per vector
                const int k = tid >> 3, l8 = tid & 7;
                double h = 0.0;
                if (k <= j) {
                    const double *vk = Vl + k * 256;
                    const int sw = (k & 7) << 3;
#pragma unroll 8
                    for (int q = 0; q < 32; ++q) { const int i = 8 * q + l8; h = fma(vk[i ^ sw], wsv[i], h); }
                }
                h += __shfl_xor(h, 1); h += __shfl_xor(h, 2); h += __shfl_xor(h, 4);
                if (k <= j && l8 == 0) hb[k] = h;
            }
            for (int k0 = LZ_LDSV; k0 <= j; k0 += 64) {         // the vectors beyond the LDS copy
                const int k = k0 + (tid >> 3), l8 = tid & 7;
                double h = 0.0;
                if (k <= j) {
                    const double *vk = Vg + (size_t)(k - LZ_LDSV) * 256;
#pragma unroll 8
                    for (int q = 0; q < 32; ++q) { const int i = 8 * q + l8; h = fma(__builtin_nontemporal_load(vk + i), wsv[i], h); }
                }
                h += __shfl_xor(h, 1); h += __shfl_xor(h, 2); h += __shfl_xor(h, 4);
                if (k <= j && l8 == 0) hb[k] = h;
            }
            __syncthreads();
            alpha += hb[j];
            double h2 = 0.0;                                   // |h|^2: what this sweep takes out of w
            {
                // w -= V h on all 512 threads (round 5, second session): the even-k chain (acc0) on threads 0..255, the odd-k chain and
                // the vectors beyond the LDS copy (acc1) on threads 256..511 for the same element i, handed over through `zz` (free
                // outside the convergence test); same two chains, same final acc0 + acc1: same bits as the 256-thread form
                const int i = tid & 255;
                const int jl = j < LZ_LDSV ? j : LZ_LDSV - 1;
                if (tid >= 256) {
                    double acc1 = 0.0;
                    int k = 0;
                    for (; k + 1 <= jl; k += 2) acc1 = fma(hb[k + 1], Vl[(k + 1) * 256 + (i ^ (((k + 1) & 7) << 3))], acc1);
#pragma unroll 8
                    for (int kk = LZ_LDSV; kk <= j; ++kk) acc1 = fma(hb[kk], __builtin_nontemporal_load(Vg + (size_t)(kk - LZ_LDSV) * 256 + i), acc1);
                    zz[i] = acc1;
                }
                double acc0 = 0.0;
                if (tid < 256) {
                    int k = 0;
                    for (; k + 1 <= jl; k += 2) {
                        const double h0 = hb[k], h1 = hb[k + 1];
                        acc0 = fma(h0, Vl[k * 256 + (i ^ ((k & 7) << 3))], acc0);
                        h2 = fma(h0, h0, fma(h1, h1, h2));
                    }
                    if (k <= jl) { const double h0 = hb[k]; acc0 = fma(h0, Vl[k * 256 + (i ^ ((k & 7) << 3))], acc0); h2 = fma(h0, h0, h2); }
                    for (int kk = LZ_LDSV; kk <= j; ++kk) { const double h0 = hb[kk]; h2 = fma(h0, h0, h2); }
                }
                __syncthreads();
                if (tid < 256) {
                    wi -= acc0 + zz[i];
                    wsv[tid] = wi;
                }
            }
            nrm2 = lz_sum256(tid < 256 ? wi * wi : 0.0, red, pass);        // (its barrier also publishes wsv)
            // (Daniel, Gragg, Kaufman, Stewart.)  h2 is the same in every thread below 256; thread 0 decides
            if (pass == 0) {
                if (tid == 0) s_first = (nrm2 >= 0.5 * (nrm2 + h2)) ? 1 : 0;
                __syncthreads();
                const int skip = s_first;
                __syncthreads();
                if (skip) break;
            }
        }
        const double beta = sqrt(nrm2);
        if (tid == 0) { al[j] = alpha; be[j] = beta; }
        m = j + 1;
        // ---- convergence test
        ascale = fmax(ascale, fabs(alpha) + beta);
        const bool check = m == r || !(beta > 1e-13 * ascale) || (m >= 24 && ((m <= 64 && (m & 7) == 0) || (m & 15) == 0));
        if (check) {
            __syncthreads();                                   // al / be of this step
            double lo = INF, hi = -INF;
            for (int i = tid; i < m; i += 512) {
                const double rad = (i > 0 ? fabs(be[i - 1]) : 0.0) + (i + 1 < m ? fabs(be[i]) : 0.0);
                lo = fmin(lo, al[i] - rad);
                hi = fmax(hi, al[i] + rad);
            }
            for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o)); hi = fmax(hi, __shfl_xor(hi, o)); }
            if ((tid & 63) == 0) { red[16 + (tid >> 6)] = lo; red[24 + (tid >> 6)] = hi; }
            __syncthreads();
            lo = red[16]; hi = red[24];
            for (int q = 1; q < 8; ++q) { lo = fmin(lo, red[16 + q]); hi = fmax(hi, red[24 + q]); }
            const double span = fmax(fabs(lo), fabs(hi));
            const double isp = 1.0 / fmax(span, 1e-300);
            hi += 1e-15 * span + 1e-300;
            lo -= 1e-15 * span + 1e-300;
            // the extreme Ritz value only moves outwards as T grows (interlacing): the last test's inner bracket end still bounds it
            // on the inside, and it usually moves very little -- the first round's shifts crowd towards that end (geometrically,
            // eight per octave), the others are uniform
            // scaled copies for the Sturm counts: a_i / |T| in zz, (b_i / |T|)^2 in wsv (both free here)
            for (int i = tid; i < m; i += 512) { zz[i] = al[i] * isp; const double bsc = be[i] * isp; wsv[i] = bsc * bsc; }
            __syncthreads();
            bool geo = false;
            if (have_prev) { if (want_max) { if (prev_lo > lo) { lo = prev_lo; geo = true; } } else if (prev_lo < hi) { hi = prev_lo; geo = true; } }
            for (int round = 0; round < 9; ++round) {
                if (!(hi - lo > 1e-15 * fmax(fabs(lo), fabs(hi)))) break;      // a few ulps: the midpoint is good to 5e-16
                // shift number t (1 .. 512) at distance u_t (hi - lo) from the inner end: u_t = t / 513, or 2^((t - 513) / 8) in a
                // warm-started first round (eight per octave, crowding towards the inner end)
                const bool g0 = geo && round == 0;
                const double wdt = hi - lo;
                auto u_of = [&](int t) -> double {
                    if (!g0) return (double)t * (1.0 / 513.0);
                    const double c8[8] = {1.0, 1.0905077326652577, 1.189207115002721, 1.2968395546510096, 1.4142135623730951,
                                          1.5422108254079407, 1.681792830507429, 1.8340080864093424};       // 2^(q / 8)
                    const int e = t - 513;
                    return ldexp(c8[e & 7], e >> 3);
                };
                auto shift_at = [&](int t) -> double {         // t = 0 .. 513: inner end .. outer end
                    if (t <= 0) return want_max ? lo : hi;
                    if (t >= 513) return want_max ? hi : lo;
                    return want_max ? lo + u_of(t) * wdt : hi - u_of(t) * wdt;
                };
                const double xs = want_max ? lo + u_of(tid + 1) * wdt : hi - u_of(tid + 1) * wdt;
                // Sturm count without divisions: p_i = (a_i - x) p_{i-1} - b_{i-1}^2 p_{i-2} on entries scaled by 1 / |T| (factors
                // of modulus <= 2; the pair is rescaled every eight steps); an eigenvalue below x for every i where p_i and
                // p_{i-1} differ in sign -- the q_i = p_i / p_{i-1} < 0 of the quotient form (a zero takes its predecessor's sign)
                int cnt = 0;
                const double xsc = xs * isp;
                double p0 = 1.0, p1 = zz[0] - xsc;
                if (p1 < 0.0) ++cnt;
#pragma unroll 4
                for (int i = 1; i < m; ++i) {
                    const double p2 = fma(zz[i] - xsc, p1, -wsv[i - 1] * p0);
                    // q_i = p2 / p1 < 0  <=>  signs differ (a zero p1 counts as positive, as the 1e-300 of the quotient form)
                    if ((p2 < 0.0) != (p1 < 0.0 || (p1 == 0.0 && p0 < 0.0))) ++cnt;
                    p0 = p1; p1 = p2;
                    if ((i & 7) == 7) {
                        const double mg = fmax(fabs(p0), fabs(p1));
                        const double sc = mg > 1e100 ? 1e-100 : (mg < 1e-100 ? 1e100 : 1.0);
                        p0 *= sc; p1 *= sc;
                    }
                }
                // outside the spectrum of T (on the wanted side)?  the first such shift, counted from the inner end
                const bool hit = want_max ? (cnt >= m) : (cnt == 0);
                if (tid == 0) s_first = 512;
                __syncthreads();
                if (hit) atomicMin(&s_first, tid);
                __syncthreads();
                const int f = s_first;
                __syncthreads();
                const double inner = shift_at(f), outer = shift_at(f + 1);      // theta lies between shifts f and f + 1
                if (want_max) { lo = inner; hi = outer; } else { hi = inner; lo = outer; }
            }
            th_lo = lo; th_hi = hi;
            prev_lo = want_max ? lo : hi; have_prev = true;
            if (tid == 0) {
                // the Ritz vector's last component: (T - theta I) s = 0 solved from the BOTTOM with s_m = 1 --
                //   s_{i-1} = ((theta - a_i) s_i - b_i s_{i+1}) / b_{i-1}
                // -- the growing direction of the recurrence when the Ritz pair has converged (its weight sits in the early
                // Lanczos vectors), hence the stable one; before convergence the estimate is rough and the answer is "go on" anyway
                const double th = 0.5 * (lo + hi);
                double s1 = 1.0, s2 = 0.0, n2 = 1.0;               // s_i, s_{i+1}
                int rescaled = 0;
                for (int i = m - 1; i >= 1; --i) {
                    double bb = be[i - 1];
                    if (fabs(bb) < 1e-300) bb = 1e-300;
                    const double s0 = ((th - al[i]) * s1 - (i + 1 < m ? be[i] : 0.0) * s2) * lz_rcp(bb);
                    s2 = s1; s1 = s0;
                    n2 += s0 * s0;
                    if (n2 > 1e200) { s1 *= 1e-100; s2 *= 1e-100; n2 *= 1e-200; rescaled += 1; }
                }
                // |s_m| / |s| = 10^(-100 rescaled) / sqrt(n2)
                s_res[0] = rescaled ? 0.0 : beta / sqrt(n2);
                s_res[1] = span;
            }
            __syncthreads();
            done = (s_res[0] <= 1e-11 * s_res[1]) || !(beta > 1e-14 * s_res[1]) || m == r;
        }
        if (!done) {
            const double vn = wi / beta;
            if (tid < 256) { vs[tid] = vn; vput(j + 1, tid, vn); }
            __syncthreads();
        }
    }
    if (tid == 0) {
        const double ev = 0.5 * (th_lo + th_hi);
        partial[item] = sd_maxstep_verdict(want_max != 0, ev, scale);
        if (stat) stat[0] = m;
        // the bound the inertia certificate checks: no eigenvalue beyond theta by more than 1e-9 |T| (the stop was at 1e-11 |T|)
        if (cert) { const double tol = cert_tol * s_res[1] + 1e-300; cert[0] = want_max ? ev + tol : ev - tol; cert[1] = 0.0; }
        atomicAdd(g_lz_hist + (m >> 3 < 32 ? m >> 3 : 32), 1);       // histogram of step counts (CIP_LG_LANCZOS_STATS=1 prints it at destroy)
    }
}
// ---- inertia certificate of the Lanczos max-step (mode 2; ADVICE r3: a Ritz value can settle on an interior eigenvalue when the
// fixed start vector has no component along the extreme eigenvector).  With theta' = theta +- 1e-9 |T| from the kernel:
//   B = theta' I - A (largest eigenvalue wanted)  or  A - theta' I (smallest)  must be positive definite
// -- checked by the library's own LDL' with all-positive prescribed pivot signs (a wrong-sign or dead pivot raises info).  If it is
// not, `gate` goes up and the tridiagonalisation + Sturm path behind it recomputes the verdict from the same scaled matrix
// (both kernels return at once on a lowered gate).  cert[1] != 0: the Lanczos kernel answered Inf for an X outside the cone --
// nothing to certify (B = I).  Asym: the matrix the Lanczos kernel saw (scaled, symmetrised), for the fallback.
__global__ __launch_bounds__(256) void k_lg_cert_build(const double *M, int ldm, const double *dscale, int r, int rp, int want_max,
                                                        const double *cert, double *B, double *Asym) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)rp * rp) return;
    const int i = (int)(e % rp), j = (int)(e / rp);
    double a = 0.0, b = (i == j) ? 1.0 : 0.0;
    if (i < r && j < r) {
        a = sd_scaled_sym_entry(M, ldm, dscale, j, i);
        if (cert[1] == 0.0) {
            const double th = (i == j) ? cert[0] : 0.0;
            b = want_max ? th - a : a - th;
        }
    }
    B[e] = b;
    Asym[e] = a;
}
__global__ void k_lg_cert_check(const int *info, int *gate, unsigned *count) {
    if (threadIdx.x == 0) {
        const int up = (info[0] != 0 || info[2] != 0) ? 1 : 0;
        gate[0] = up;
        if (up) atomicAdd(count, 1u);
    }
}

// ------------------------------------------------------------------------------------------ host side
static int lg_certify(hipStream_t s, LargeWs *w, const LargeSide &sd, const double *dscale, int r, int want_max, double scale,
                      double *partial, int item) {
    const int rp = w->rp;
    const long n2 = (long)rp * rp;
    hipLaunchKernelGGL(k_lg_cert_build, lg_grid(n2), dim3(256), 0, s, (const double *)sd.M3, rp, dscale, r, rp, want_max, (const double *)sd.cert, sd.M2, sd.M1);
    LdltWorkspace wc = *sd.wx;
    wc.no_prep = 1; wc.lazyC = nullptr; wc.prof = nullptr;
    CIP_TRY(cip_ldlt_factor(s, sd.M2, rp, rp, wc));
    hipLaunchKernelGGL(k_lg_cert_check, dim3(1), dim3(64), 0, s, (const int *)wc.info, sd.gate, w->fallbacks());      // (w->ctr is cleared by every NT scaling)
    // the fallback (one workgroup each, at once back unless the gate is up): side 1 of a pair has its own d / e vectors
    const size_t shm1 = T1_LDS_DOUBLES * sizeof(double);
    CIP_TRY(lg_set_attr((const void *)k_lg_tridiag1, shm1));
    hipLaunchKernelGGL(k_lg_tridiag1, dim3(1), dim3(512), shm1, s, (const double *)sd.M1, rp, (const double *)nullptr, r, sd.dg, sd.of, (const int *)sd.gate);
    hipLaunchKernelGGL(k_lg_sturm, dim3(1), dim3(LG_T), 0, s, sd.dg, sd.of, r, want_max, scale, (const int *)nullptr, partial, item, (const int *)sd.gate);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}
// dg, of of side 0 <- the tridiagonal form of M, by the form of its order; work: a matrix for the stepped form
static int lg_tridiag(hipStream_t s, LargeWs *w, const LgEigForm &f, const double *M, const double *dscale, int r, double *work) {
    if (f.kind == LG_EIG_STEPPED) return lg_tridiag_stepped(s, w, M, dscale, r, work);
    if (f.kind == LG_EIG_REGISTERS) {
        const size_t shm1 = T1_LDS_DOUBLES * sizeof(double);
        CIP_TRY(lg_set_attr((const void *)k_lg_tridiag1, shm1));
        hipLaunchKernelGGL(k_lg_tridiag1, dim3(1), dim3(512), shm1, s, M, w->rp, dscale, r, w->dg(), w->of(), (const int *)nullptr);
        CIP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    CIP_TRY(lg_set_attr((const void *)k_lg_tridiag, f.lds));
    CIP_HIP_CHECK(hipMemsetAsync(w->ctr, 0, LG_C_WORDS * sizeof(unsigned), s));
    double *xbuf = w->slot(LG_V_XBUF), *pbuf = w->slot(LG_V_PBUF);   // 2 x rp each
    hipLaunchKernelGGL(k_lg_tridiag, dim3(f.nwg), dim3(LG_T), f.lds, s, M, w->rp, dscale, r, w->dg(), w->of(), xbuf, pbuf, w->ctr + LG_C_BARRIER,
                       (int *)(w->ctr + LG_C_GIVEUP), f.slab);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// Round 6: the max-step's Lanczos WITHOUT the Gram-Schmidt sweeps by default (CIP_LG_LANCZOS_REORTH=1 restores them).  The recurrence
// stops at the FIRST convergence of the extreme Ritz value, and a Lanczos basis loses its orthogonality only when a Ritz value
// converges (Paige): up to the stop the plain three-term recurrence is the reorthogonalised one to working precision, unless the
// other end of the spectrum converges first -- then the wanted end takes more steps (config 4's max-steps: the longest runs 144-151 ->
// 176-183 steps, the typical 40-47 unchanged).  What the returned value claims is checked by the inertia certificate either way.
// Measured: config 4 8.17-8.22 -> 7.88-8.00 ms per iteration; tests/test_gpu_sdp.py (LAPACK on hard spectra, the certificate's
// self-test, five trajectories) green in both modes.
static int lz_reorth(void) {
    static const int on = cip_env_int("CIP_LG_LANCZOS_REORTH", 0);
    return on;
}
// 2 (default; CIP_LG_LANCZOS changes it): the max-step's extreme eigenvalue by k_lg_lanczos1 at orders <= 256 + the inertia certificate
// (lg_certify); 1: Lanczos alone; 3: certificate self-test; 0: full
// tridiagonalisation + Sturm multisection at every order (A/B runs, tests).  on < 0 only reads; returns the previous setting
static CipKnob g_lg_lanczos{[] { const int v = cip_env_int("CIP_LG_LANCZOS", 2); return (v >= 0 && v <= 3) ? v : 2; }};
int cip_sdp_large_lanczos(int on) { return g_lg_lanczos.set(on, [](int v) { return v >= 0 && v <= 3; }); }
// The two max-steps of a pair (v side, s side: src/ConicIP.jl:708-709, :881-882, :927-928) are independent: side 1 works in the
// NT scaling's s-side buffers (LargeWs::side) on a second stream.  With the Lanczos form only (lg_pairable): there each side has its
// own stat / gate words, certificate pair and fallback dg / of.  The tridiagonalisations that serve every other case have ONE set of
// vec slots 1-7 (dg, of, xbuf / vbuf, pbuf, scal), and the cooperative one clears all of ctr and counts its barrier in word 0: two of
// them side by side would overwrite each other.
bool cip_sdp_large_pairable(const LargeWs *w) { return w && lg_pairable(w->rp, cip_sdp_large_lanczos(-1)); }
int cip_sdp_large_fork(hipStream_t s, LargeWs *w, hipStream_t *s2) {
    if (!w->s2) {
        CIP_HIP_CHECK(hipStreamCreateWithFlags(&w->s2, hipStreamNonBlocking));
        CIP_HIP_CHECK(hipEventCreateWithFlags(&w->efork, hipEventDisableTiming));
        CIP_HIP_CHECK(hipEventCreateWithFlags(&w->ejoin, hipEventDisableTiming));
    }
    CIP_HIP_CHECK(hipEventRecord(w->efork, s));
    CIP_HIP_CHECK(hipStreamWaitEvent(w->s2, w->efork, 0));
    *s2 = w->s2;
    return 0;
}
int cip_sdp_large_join(hipStream_t s, LargeWs *w) {
    CIP_HIP_CHECK(hipEventRecord(w->ejoin, w->s2));
    CIP_HIP_CHECK(hipStreamWaitEvent(s, w->ejoin, 0));
    return 0;
}
int cip_sdp_large_cert_stats(hipStream_t s, LargeWs *w, int *out2) {
    unsigned c = 0;
    if (w) { CIP_HIP_CHECK(hipMemcpyAsync(&c, w->fallbacks(), sizeof(c), hipMemcpyDeviceToHost, s)); CIP_HIP_CHECK(hipStreamSynchronize(s)); }
    out2[0] = (int)c; out2[1] = 0;
    return 0;
}

// partial[item] <- the max-step verdict from the extreme eigenvalue (want_max: the largest) of sd.M3 scaled by dscale on both sides
// (null: as it is); info: the pivot flags of the factorisation behind M3 (null: none).  Lanczos and, in modes 2 / 3, its certificate;
// or a tridiagonalisation -- into side 0's dg / of: no pair without the Lanczos form -- and Sturm.
static int lg_extreme_eig(hipStream_t s, LargeWs *w, const LargeSide &sd, int r, const double *dscale, const int *info, int want_max,
                          double scale, double *partial, int item) {
    const int lzmode = cip_sdp_large_lanczos(-1);
    const LgEigForm f = lg_eig_form(r, lzmode);
    if (f.kind != LG_EIG_LANCZOS) {
        CIP_TRY(lg_tridiag(s, w, f, sd.M3, dscale, r, sd.M2));
        hipLaunchKernelGGL(k_lg_sturm, dim3(1), dim3(LG_T), 0, s, w->dg(), w->of(), r, want_max, scale, info, partial, item);
        CIP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    double *const cert = f.certificate ? sd.cert : nullptr;
    const double cert_tol = lzmode == 3 ? -1e-3 : 1e-9;      // mode 3 (self-test): the bound on the WRONG side of theta -- every certificate fails, every verdict comes from the fallback
    CIP_TRY(lg_set_attr((const void *)k_lg_lanczos1, LZ_LDS_DOUBLES * sizeof(double)));
    hipLaunchKernelGGL(k_lg_lanczos1, dim3(1), dim3(512), LZ_LDS_DOUBLES * sizeof(double), s, (const double *)sd.M3, w->rp, dscale, r, want_max,
                       scale, info, partial, item, sd.M1, sd.stat, cert, cert_tol, lz_reorth());
    CIP_HIP_CHECK(hipGetLastError());
    return cert ? lg_certify(s, w, sd, dscale, r, want_max, scale, partial, item) : 0;
}
// maxstep_sdc for one large cone: partial[cd.item]
int cip_sdp_large_maxstep(hipStream_t s, LargeWs *w, const ConeDesc &cd, const double *x, const double *d, double scale,
                          double *partial, int side) {
    const int r = cd.r, rp = w->rp;
    const LargeSide sd = w->side(side);
    if (!d) {                                                                       // maxstep_sdc(x, nothing) :295-303
        lg_mat(s, x + cd.off, 1L, 0L, sd.M3, r, rp, 0.0);
        return lg_extreme_eig(s, w, sd, r, nullptr, nullptr, 0, 1.0, partial, cd.item);
    }
    lg_mat(s, x + cd.off, 1L, 0L, sd.Kx, r, rp, 1.0);
    CIP_TRY(cip_ldlt_factor(s, sd.Kx, rp, rp, *sd.wx));                             // X = L D L'
    const double *Xi = (sd.wx->Bs == CIP_NB) ? sd.wx->Linv : sd.wx->X;              // inv(L_unit)
    if (lg_small_product(rp)) {                                                     // inv(L) D, D = mat(d) read from the vector
        lg_gemm_from_vec(s, sd.M2, Xi, d + cd.off, rp, r);
    } else {
        lg_mat(s, d + cd.off, 1L, 0L, sd.M1, r, rp, 0.0);
        CIP_TRY(lg_gemm(s, sd.M2, 0, Xi, 0, sd.M1, 0, rp, 1));                      // inv(L) D        (D symmetric)
    }
    CIP_TRY(lg_gemm(s, sd.M3, 0, sd.M2, 0, Xi, 0, rp, 1));                          // inv(L) D inv(L)'
    return lg_extreme_eig(s, w, sd, r, sd.wx->dvec, sd.wx->info, 1, scale, partial, cd.item);      // ... scaled by d^-1/2 on both sides
}
