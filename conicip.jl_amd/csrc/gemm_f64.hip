// fp64 MFMA "NT" GEMM for gfx950:  C (+)= alpha * A * B'   (all column-major): every O(N^3) term of the KKT path, i.e. the work
// the reference does in src/kktsolvers.jl:32-35 (dense GEMMs + QR) and :289-295 (Schur + LU), re-designed for CDNA4.
// One launcher per form (declared in cip_internal.h, defined at the end of this file); DESIGN.md section 5 has the kernel
// table, the tile design and the measurements behind each choice.
//   cip_gemm_lower        k_ldlt_trailing_64<EPI_ACCUM>: the LDL' trailing update C -= (L21 D) L21' (K = outer block) and the rank
//                         updates of the assembly, on 64x64 quarter tiles of the lower triangle, operands global -> LDS directly
//   cip_gemm_lower_lazyc  k_ldlt_trailing_64<EPI_LAZYC>: the same with C read from Q (assemble.hip: lazy copy)
//   cip_gemm_rect         k_gemm_nt_64 (64x64, register staging, raised priority) below 256 128-tiles: the wide and short in-block
//                         update of the three-launch panel chain (K = 128); k_gemm_nt_128 (128x128) from there on
//   cip_syrk_schur        S = Q + (A'F^-1)(A'F^-1)', K = m: k_syrkq_64<GLDS> on quarter tiles; with few tiles and K >= 4096 the k range
//                         in slices, k_syrk_splitk_64 (or, <= 64 tiles and K >= 16384, k_syrk_splitk_128) + k_syrk_reduce; without a
//                         Qin (CSR Q) the same launches with epilogues that store alpha W W' alone (EPI_SYRK0, k_syrk_reduce<false>)
//   cip_gemm_batched_64   k_gemm_nt_64_batched (64x64, optional transposed copy / tile selection): block-inverse doubling
//                         (ldlt.hip), congruences of the large S cones (sdp_large.hip)
//   cip_gemm_batched_16   k_gemm_nt_16_batched (16x16, k split over the four waves, no LDS staging): the doubling of the last
//                         1024-wide solve block, the one preparation nothing hides
// The 64x64 tile (cip_gemm_tile.h: gemm_tile_64) is the workhorse: 4 wave64s in a 2x2 grid, each a 32x32 sub-tile = 2x2
// v_mfma_f64_16x16x4_f64 accumulators, 32 KB of LDS, five workgroups per CU.  It beats the 128x128 tile at two workgroups per CU
// on the trailing update (55.0 vs 52.4 TFLOP/s at r = 8192, K = 512) and has a quarter of its per-tile latency on the skinny
// updates.  The 128x128 tile (gemm_tile_128, below: each wave a 64x64 sub-tile = 4x4 accumulators, 64 KB of LDS) moves half the LDS
// and operand traffic per flop and is kept where that decides: big rectangles and the long-K split Schur formation.  Both tiles:
//   * Both operands are "row-contiguous, k-strided" in memory (a panel column is a contiguous run of rows), so a k-tile of
//     16 columns is staged as lds[k][row], double-buffered, one barrier per k-tile.
//   * Fragments are read with ds_read_b128: lane c takes rows (2c, 2c+1) of a 32-row group, feeding two MFMA tiles per read;
//     the row pitch is a multiple of 256 B, which is conflict-free for the b128 lane groups.
//   * The MFMA is issued "transposed" (A-operand = B rows, B-operand = A rows) so that an accumulator's lane index runs
//     along C's rows: the epilogue then moves 16-byte double2 per lane, 256 B contiguous per 16 lanes.
//   * blockIdx of the rectangular kernels is remapped so that each XCD (own L2) walks a contiguous run of tiles (bijective
//     variant of the xcd swizzle).
#include "cip_internal.h"
#include "cip_gemm_tile.h"
#include <stdlib.h>
#include <mutex>

#define LDS_TILE (CIP_KT * CIP_NB)        // doubles per operand per buffer (2048)

__device__ __forceinline__ int xcd_remap(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// linear tile index -> (block row, block column), row-major over the lower triangle
__device__ __forceinline__ void lower_tile_coords(int t, int &bi, int &bj) {
    bi = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)bi * (bi + 1) / 2 > t) --bi;
    while ((long)(bi + 1) * (bi + 2) / 2 <= t) ++bi;
    bj = t - (int)((long)bi * (bi + 1) / 2);
}

// 128x128 tile of C: STORE ? C = alpha acc : C += alpha acc
template <bool STORE>
__device__ __forceinline__ void gemm_tile_128(const GemmArgs &g, double *lds, int bi, int bj) {

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;

    const long i0 = (long)bi * CIP_NB, j0 = (long)bj * CIP_NB;
    const double *Ap = g.A + i0 + 2 * lane;
    const double *Bp = g.B + j0 + 2 * lane;

    v2d ra[4], rb[4];
    auto gload = [&](int kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long k = (long)kt * CIP_KT + q * 4 + wave;
            ra[q] = *(const v2d *)(Ap + k * g.lda);
            rb[q] = *(const v2d *)(Bp + k * g.ldb);
        }
    };
    auto lstore = [&](int buf) {
        double *la = lds + buf * (2 * LDS_TILE);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *(v2d *)(la + (q * 4 + wave) * CIP_NB + 2 * lane) = ra[q];
            *(v2d *)(la + LDS_TILE + (q * 4 + wave) * CIP_NB + 2 * lane) = rb[q];
        }
    };

    v4d acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};

    const int KT = g.K / CIP_KT;
    gload(0);
    lstore(0);
    __syncthreads();

    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) gload(kt + 1);
        const double *la = lds + buf * (2 * LDS_TILE) + wm * 64 + 2 * l15;
        const double *lb = lds + buf * (2 * LDS_TILE) + LDS_TILE + wn * 64 + 2 * l15;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int kk = ks * 4 + l4;
            const v2d fi0 = *(const v2d *)(la + kk * CIP_NB);
            const v2d fi1 = *(const v2d *)(la + kk * CIP_NB + 32);
            const v2d fj0 = *(const v2d *)(lb + kk * CIP_NB);
            const v2d fj1 = *(const v2d *)(lb + kk * CIP_NB + 32);
            const double fi[4] = {fi0.x, fi0.y, fi1.x, fi1.y};
            const double fj[4] = {fj0.x, fj0.y, fj1.x, fj1.y};
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti)
                    acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fj[tj], fi[ti], acc[ti][tj], 0, 0, 0);
        }
        if (kt + 1 < KT) lstore(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue.  lane holds, for tile (ti,tj), reg q:  C[row, col] with
    //   row = i0 + wm*64 + (ti>>1)*32 + 2*l15 + (ti&1)
    //   col = j0 + wn*64 + (tj>>1)*32 + 2*(l4 + 4q) + (tj&1)
    // The C operand is fetched one tj (eight loads) at a time, the batch of tj + 1 issued before the stores of tj: a load
    // placed behind a store to C cannot be hoisted over it (gemm_tile_64: cfetch).
    v2d cbuf[2][4][2];
    auto cfetch = [&](int tj) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long col = j0 + wn * 64 + (tj >> 1) * 32 + 2 * (l4 + 4 * q) + (tj & 1);
#pragma unroll
            for (int gi = 0; gi < 2; ++gi)
                cbuf[tj & 1][q][gi] = STORE ? (v2d){0.0, 0.0} : *(const v2d *)(g.C + i0 + wm * 64 + gi * 32 + 2 * l15 + col * g.ldc);
        }
    };
    cfetch(0);
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        if (tj + 1 < 4) cfetch(tj + 1);
        const auto &cin = cbuf[tj & 1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long col = j0 + wn * 64 + (tj >> 1) * 32 + 2 * (l4 + 4 * q) + (tj & 1);
#pragma unroll
            for (int gi = 0; gi < 2; ++gi) {
                const long row = i0 + wm * 64 + gi * 32 + 2 * l15;
                v2d val = (v2d){acc[2 * gi][tj][q], acc[2 * gi + 1][tj][q]};
                double *cp = g.C + row + col * g.ldc;
                v2d c = cin[q][gi];
                c += g.alpha * val;
                *(v2d *)cp = c;
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void k_gemm_nt_128(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * LDS_TILE];   // 64 KB
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    const int tm = g.M / CIP_NB;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    gemm_tile_128<false>(g, lds, t % tm, t / tm);
}

__global__ __launch_bounds__(256, 4) void k_gemm_nt_64(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * CIP_KT * SB];   // 32 KB
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    __builtin_amdgcn_s_setprio(3);       // skinny critical-path updates: priority over co-resident waves
    const int tm = g.M / SB;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    gemm_tile_64(g, lds, (long)(t % tm) * SB, (long)(t / tm) * SB);
}

// The LDL' trailing update C -= (L21 D) L21' on the lower triangle, in 64x64 quarter tiles (its own symbol so that
// profiles separate it from the skinny in-block updates): block b -> 128-tile b/4, quadrant b%4.
// 5 workgroups (20 waves) per CU; measured against the 128x128-tile kernel at 2 workgroups per CU:
// 55.0 vs 52.4 TFLOP/s at r = 8192, K = 512 and 53.1 vs 44.0 at K = 256 (tools/gemm_bench.hip, same session).
template <int EPI>
__global__ __launch_bounds__(256, 4) void k_ldlt_trailing_64(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * CIP_KT * SB];   // 32 KB
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    __builtin_amdgcn_s_setprio(3);                     // measured: 58.0 vs 56.6 TFLOP/s without
    int bi, bj;
    lower_tile_coords((int)(blockIdx.x >> 2), bi, bj);
    const int sub = blockIdx.x & 3;
    if (bi == bj && sub == 2) return;            // strictly-upper quadrant of a diagonal tile: never referenced
    gemm_tile_64<EPI, true>(g, lds, (long)bi * CIP_NB + (sub & 1) * SB, (long)bj * CIP_NB + (sub >> 1) * SB);
}

// Batched small products (block-inverse doubling): grid.y x grid.z independent problems, C = alpha A B' (overwrite)
__global__ __launch_bounds__(256, 4) void k_gemm_nt_64_batched(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * CIP_KT * SB];   // 32 KB
    bool live;
    const unsigned oz = gemm_batch_prologue(g, cb, live);
    if (!live) return;
    gemm_own_batch(g, oz);
    const int tm = g.M / SB;
    if (g.tiles == GEMM_TILES_TOUCH_UPPER && (blockIdx.x % tm) > (blockIdx.x / tm)) return;     // tiles strictly below the diagonal are not wanted
    if (g.tiles == GEMM_TILES_TOUCH_LOWER && (blockIdx.x % tm) < (blockIdx.x / tm)) return;     // tiles strictly above
    gemm_tile_64<EPI_STORE>(g, lds, (long)(blockIdx.x % tm) * SB, (long)(blockIdx.x / tm) * SB);
}

// The same batched overwrite form with ONE 16x16 tile of C per workgroup, the k range split over its four waves: the tile of
// cip_gemm_tile.h's gemm_tile_16_splitk (same MFMAs, same reduction order), written out here with alpha and the transposed copy in
// its epilogue.  For the block-inverse doubling (ldlt.hip): a level is a handful of h x h x h products, and a 64x64 tile walks its
// whole K = h on one CU -- 512 dependent MFMAs per wave at h = 512, 14 us of one CU's MFMA pipe behind a latency-bound k-loop, 19 us
// per launch on an idle chip -- while here the same product is (h / 16)^2 workgroups with 8 h / 128 MFMAs per wave.  K a multiple
// of 128, M and N of 16.  Register q of lane l holds C[i0 + l % 16, j0 + l / 16 + 4 q].
__global__ __launch_bounds__(256) void k_gemm_nt_16_batched(GemmArgs g, CipBatch cb) {
    __shared__ double red[3][4][64];
    bool live;
    const unsigned oz = gemm_batch_prologue(g, cb, live);
    if (!live) return;
    gemm_own_batch(g, oz);
    const int tm = g.M / 16;
    const long i0 = (long)(blockIdx.x % tm) * 16, j0 = (long)(blockIdx.x / tm) * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int kq = g.K >> 2;
    const double *a = g.A + i0 + l15 + (long)(wave * kq + l4) * g.lda;
    const double *b = g.B + j0 + l15 + (long)(wave * kq + l4) * g.ldb;
    v4d acc0 = (v4d){0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
    for (int k = 0; k < kq; k += 32) {
        double av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            av[u] = a[(long)(k + 4 * u) * g.lda];
            bv[u] = b[(long)(k + 4 * u) * g.ldb];
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[u], av[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[u + 1], av[u + 1], acc1, 0, 0, 0);
        }
    }
    acc0 += acc1;
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][lane] = acc0[q];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double c = g.alpha * (((acc0[q] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane]);
            const long i = i0 + l15, j = j0 + l4 + 4 * q;
            g.C[i + j * g.ldc] = c;
            if (g.Ct) g.Ct[j + i * g.ldct] = c;
        }
    }
}

// Schur formation S = Q + Wt Wt' (lower tiles) in quarter tiles: the long-K (K = m) counterpart of the trailing update
template <bool GLDS, int EPI = EPI_SYRKQ>
__global__ __launch_bounds__(256, 4) void k_syrkq_64(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * CIP_KT * SB];   // 32 KB
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    if (GLDS) __builtin_amdgcn_s_setprio(3);
    int bi, bj;
    lower_tile_coords((int)(blockIdx.x >> 2), bi, bj);
    const int sub = blockIdx.x & 3;
    if (bi == bj && sub == 2) return;
    gemm_tile_64<EPI, GLDS>(g, lds, (long)bi * CIP_NB + (sub & 1) * SB, (long)bj * CIP_NB + (sub >> 1) * SB);
}

// The same with few output tiles and a long K -- config 4: S = 1024 x 1024 from K = m = 32896, 136 quarter tiles on a chip with
// room for 1280 workgroups, 23 TFLOP/s.  Split-K: grid.y slices of the k range, each slice's product stored to its own image
// (EPI_STORE), then k_syrk_reduce adds the images in slice order to Qin: deterministic, no atomics.
__global__ __launch_bounds__(256, 4) void k_syrk_splitk_64(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * CIP_KT * SB];   // 32 KB
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    int bi, bj;
    lower_tile_coords((int)(blockIdx.x >> 2), bi, bj);
    const int sub = blockIdx.x & 3;
    if (bi == bj && sub == 2) return;
    const long k0 = (long)blockIdx.y * g.ksplit_len;
    g.A += k0 * g.lda; g.B += k0 * g.ldb;
    g.K = (g.K - k0 < g.ksplit_len) ? (int)(g.K - k0) : g.ksplit_len;
    g.C = (double *)((char *)g.ksplit_ws + (long)(blockIdx.z / (g.bz > 0 ? g.bz : 1)) * cb.stride) + (long)blockIdx.y * g.M * g.M;
    g.ldc = g.M; g.Ct = nullptr;
    gemm_tile_64<EPI_STORE>(g, lds, (long)bi * CIP_NB + (sub & 1) * SB, (long)bj * CIP_NB + (sub >> 1) * SB);
}
// The same on 128x128 tiles (two workgroups per CU): half the operand traffic per flop.  With K = m in the tens of thousands a
// slice's operand panel (M x len doubles) is far larger than an XCD's L2 and every tile streams it again: the 64-tile form ran
// at 36 TFLOP/s at M = 1024, K = 32896 (config 4).  CIP_SYRK_TILE = 64 / 128 forces a form.
__global__ __launch_bounds__(256, 2) void k_syrk_splitk_128(GemmArgs g, CipBatch cb) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * LDS_TILE];   // 64 KB
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    int bi, bj;
    lower_tile_coords((int)blockIdx.x, bi, bj);
    const long k0 = (long)blockIdx.y * g.ksplit_len;
    g.A += k0 * g.lda; g.B += k0 * g.ldb;
    g.K = (g.K - k0 < g.ksplit_len) ? (int)(g.K - k0) : g.ksplit_len;
    g.C = (double *)((char *)g.ksplit_ws + (long)(blockIdx.z / (g.bz > 0 ? g.bz : 1)) * cb.stride) + (long)blockIdx.y * g.M * g.M;
    g.ldc = g.M;
    gemm_tile_128<true>(g, lds, bi, bj);
}
// C[i, j] = Qin[i, j] + sum_b image_b[i, j] for i >= j (by 64-tiles), i, j < nvalid; one thread per row pair of a 64 x 64 tile column.
// HAVEQ = false: no Qin (a CSR Q is added afterwards)
template <bool HAVEQ>
__global__ __launch_bounds__(256) void k_syrk_reduce(GemmArgs g, CipBatch cb) {
    bool live;
    (void)gemm_batch_prologue(g, cb, live);
    if (!live) return;
    const double *ws = (const double *)((const char *)g.ksplit_ws + (long)(blockIdx.z / (g.bz > 0 ? g.bz : 1)) * cb.stride);
    int bi, bj;
    lower_tile_coords((int)blockIdx.x, bi, bj);                 // 64-tiles of the lower triangle
    const int r2 = threadIdx.x & 31, c0 = threadIdx.x >> 5;             // row pair, first column (8 columns per pass)
    const long row = (long)bi * SB + 2 * r2;
    const long img = (long)g.M * g.M;
    for (int c = c0; c < SB; c += 8) {
        const long col = (long)bj * SB + c;
        if (col >= g.nvalid || row >= g.nvalid) continue;
        v2d acc = (v2d){0.0, 0.0};
        for (int b = 0; b < g.ksplit_n; ++b) acc += *(const v2d *)(ws + b * img + row + col * g.M);
        double *cp = g.C + row + col * g.ldc;
        if (!HAVEQ) {
            if (row + 1 < g.nvalid) *(v2d *)cp = g.alpha * acc;
            else *cp = g.alpha * acc.x;
            continue;
        }
        const double *qp = g.Qin + row + col * g.ldq;
        if (row + 1 < g.nvalid) *(v2d *)cp = (v2d){qp[0], qp[1]} + g.alpha * acc;
        else *cp = qp[0] + g.alpha * acc.x;
    }
}
// 128-tile form of the split: few tiles and a K so long that the 64-tile form is bound by re-streaming its operands
static bool syrk_split_128(int M, int K) {
    static const int force = cip_env_int("CIP_SYRK_TILE", 0);
    if (force == 64) return false;
    const long tm = M / CIP_NB, t128 = tm * (tm + 1) / 2;
    if (force == 128) return t128 <= 256;
    return t128 <= 64 && K >= 16384;
}
int cip_syrk_split(int M, int K, int *len) {
    static const int on = cip_env_int("CIP_SYRK_SPLITK", 1);
    const long tm = M / CIP_NB, wgs = 4 * (tm * (tm + 1) / 2);
    int n = 1;
    if (on && wgs < 640 && K >= 4096) {
        if (syrk_split_128(M, K)) { n = (int)(512 / (wgs / 4)); if (n > 16) n = 16; if (n < 1) n = 1; }     // 512 slots of 64 KB of LDS
        else { n = (int)((1280 + wgs - 1) / wgs); if (n > 16) n = 16; }
    }
    int l = ((K + n - 1) / n + CIP_KT - 1) / CIP_KT * CIP_KT;
    n = (K + l - 1) / l;
    if (len) *len = l;
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- launchers
// false: nothing to launch, *rc is what the launcher returns (0 for an empty product, -1 with the error set)
static bool gemm_dims_ok(int M, int N, int K, int *rc) {
    *rc = 0;
    if (M <= 0 || N <= 0) return false;
    if (M % CIP_NB || N % CIP_NB || K % CIP_KT || K <= 0) {
        cip_set_error("gemm: bad dims M=%d N=%d K=%d", M, N, K);
        *rc = -1;
        return false;
    }
    return true;
}
// the accumulate epilogues of gemm_tile_64 address C (and Qin) with a 32-bit byte offset per lane, below 48 ld + 256
static bool gemm_pitch_ok(long ld) {
    if (ld < (1L << 26)) return true;
    cip_set_error("gemm: leading dimension %ld too large", ld);
    return false;
}
static long lower_tiles_128(int M) { const long tm = M / CIP_NB; return tm * (tm + 1) / 2; }
static GemmArgs gemm_args(int M, int N, int K, double alpha, const double *A, long lda, const double *B, long ldb, double *C, long ldc) {
    GemmArgs g = {};
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.alpha = alpha;
    return g;
}

int cip_gemm_lower(hipStream_t s, int M, int K, double alpha, const double *A, long lda, const double *B, long ldb, double *C, long ldc) {
    int rc; if (!gemm_dims_ok(M, M, K, &rc)) return rc;
    if (!gemm_pitch_ok(ldc)) return -1;
    GemmArgs g = gemm_args(M, M, K, alpha, A, lda, B, ldb, C, ldc);
    // every 128-tile of the lower triangle as four 64x64 quarter tiles (in plain tile order: an XCD-aware patch order fetched
    // less and ran slower, DESIGN_LOG.md "Experiments removed from the library")
    cip_launch_b(k_ldlt_trailing_64<EPI_ACCUM>, dim3((unsigned)(4 * lower_tiles_128(M))), dim3(256), 0, s, g);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cip_gemm_lower_lazyc(hipStream_t s, int M, int K, double alpha, const double *A, long lda, const double *B, long ldb, double *C, long ldc,
                         const double *Qin, long ldq, const double *Cdiag) {
    int rc; if (!gemm_dims_ok(M, M, K, &rc)) return rc;
    if (!Qin || !Cdiag || (ldq & 1) || (((uintptr_t)Qin) & 15)) { cip_set_error("gemm: bad lazy-C arguments"); return -1; }
    if (!gemm_pitch_ok(ldc) || !gemm_pitch_ok(ldq)) return -1;
    GemmArgs g = gemm_args(M, M, K, alpha, A, lda, B, ldb, C, ldc);
    g.Qin = Qin; g.ldq = ldq; g.Cdiag = Cdiag;
    cip_launch_b(k_ldlt_trailing_64<EPI_LAZYC>, dim3((unsigned)(4 * lower_tiles_128(M))), dim3(256), 0, s, g);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// skinny, latency-critical: quarter-size tiles
static bool rect_on_quarter_tiles(long tiles128) { return tiles128 < 256; }

int cip_gemm_rect(hipStream_t s, int M, int N, int K, double alpha, const double *A, long lda, const double *B, long ldb, double *C, long ldc) {
    int rc; if (!gemm_dims_ok(M, N, K, &rc)) return rc;
    if (!gemm_pitch_ok(ldc)) return -1;
    const GemmArgs g = gemm_args(M, N, K, alpha, A, lda, B, ldb, C, ldc);
    const long tiles = (long)(M / CIP_NB) * (N / CIP_NB);
    if (rect_on_quarter_tiles(tiles)) cip_launch_b(k_gemm_nt_64, dim3((unsigned)(4 * tiles)), dim3(256), 0, s, g);
    else cip_launch_b(k_gemm_nt_128, dim3((unsigned)tiles), dim3(256), 0, s, g);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// operands global -> LDS directly + raised wave priority, as the trailing update (round 4, config 3: 1.35 -> 1.28 ms per
// Schur formation, same-session A/B 4.17 -> 4.10 ms per iteration, same bits); register staging for odd leading
// dimensions and misaligned operands
static bool syrkq_glds(const double *W, long ldw) { return !(ldw & 1) && !(((uintptr_t)W) & 15); }

int cip_syrk_schur(hipStream_t s, int M, int K, int nvalid, double alpha, const double *W, long ldw, const double *Qin, long ldq, double *C, long ldc,
                   double *split_ws, int split_n, int split_len) {
    int rc; if (!gemm_dims_ok(M, M, K, &rc)) return rc;
    GemmArgs g = gemm_args(M, M, K, alpha, W, ldw, W, ldw, C, ldc);
    g.Qin = Qin; g.ldq = ldq; g.nvalid = nvalid;
    const long tiles = lower_tiles_128(M);
    if (split_ws && split_n > 1) {
        g.ksplit_ws = split_ws; g.ksplit_n = split_n; g.ksplit_len = split_len;
        GemmArgs gs = g;
        gs.alpha = 1.0;                                          // (the images hold the plain products; alpha is applied by the reduction)
        if (syrk_split_128(M, K)) cip_launch_b(k_syrk_splitk_128, dim3((unsigned)tiles, (unsigned)split_n), dim3(256), 0, s, gs);
        else cip_launch_b(k_syrk_splitk_64, dim3((unsigned)(4 * tiles), (unsigned)split_n), dim3(256), 0, s, gs);
        const long t64 = (long)(M / SB) * (M / SB + 1) / 2;
        if (Qin) cip_launch_b(k_syrk_reduce<true>, dim3((unsigned)t64), dim3(256), 0, s, g);
        else cip_launch_b(k_syrk_reduce<false>, dim3((unsigned)t64), dim3(256), 0, s, g);
    } else if (syrkq_glds(W, ldw)) {
        if (Qin) cip_launch_b(k_syrkq_64<true>, dim3((unsigned)(4 * tiles)), dim3(256), 0, s, g);
        else cip_launch_b(k_syrkq_64<true, EPI_SYRK0>, dim3((unsigned)(4 * tiles)), dim3(256), 0, s, g);
    } else {
        if (Qin) cip_launch_b(k_syrkq_64<false>, dim3((unsigned)(4 * tiles)), dim3(256), 0, s, g);
        else cip_launch_b(k_syrkq_64<false, EPI_SYRK0>, dim3((unsigned)(4 * tiles)), dim3(256), 0, s, g);
    }
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

static GemmArgs gemm_batched_args(int M, int N, int K, double alpha, const GemmBatchIn &A, const GemmBatchIn &B, const GemmBatchOut &C,
                                  const GemmBatchOut &Ct, int bz) {
    GemmArgs g = gemm_args(M, N, K, alpha, A.p, A.ld, B.p, B.ld, C.p, C.ld);
    g.bz = bz;
    g.sAy = A.sy; g.sAz = A.sz; g.sBy = B.sy; g.sBz = B.sz; g.sCy = C.sy; g.sCz = C.sz;
    g.Ct = Ct.p; g.ldct = Ct.ld; g.sCty = Ct.sy; g.sCtz = Ct.sz;
    return g;
}

int cip_gemm_batched_64(hipStream_t s, int M, int N, int K, double alpha, const GemmBatchIn &A, const GemmBatchIn &B, const GemmBatchOut &C,
                        const GemmBatchOut &Ct, int by, int bz, int tiles) {
    int rc; if (!gemm_dims_ok(M, N, K, &rc)) return rc;
    GemmArgs g = gemm_batched_args(M, N, K, alpha, A, B, C, Ct, bz);
    g.tiles = tiles;
    cip_launch_b(k_gemm_nt_64_batched, dim3((unsigned)((M / SB) * (N / SB)), by, bz), dim3(256), 0, s, g);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cip_gemm_batched_16(hipStream_t s, int M, int N, int K, double alpha, const GemmBatchIn &A, const GemmBatchIn &B, const GemmBatchOut &C,
                        const GemmBatchOut &Ct, int by, int bz) {
    int rc; if (!gemm_dims_ok(M, N, K, &rc)) return rc;
    if (K % 128) return cip_gemm_batched_64(s, M, N, K, alpha, A, B, C, Ct, by, bz, GEMM_TILES_ALL);     // (the waves split k in 32-column steps)
    const GemmArgs g = gemm_batched_args(M, N, K, alpha, A, B, C, Ct, bz);
    cip_launch_b(k_gemm_nt_16_batched, dim3((unsigned)((M / 16) * (N / 16)), by, bz), dim3(256), 0, s, g);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}
