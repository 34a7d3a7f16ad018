// nestod_sdc (src/ConicIP.jl:196-210) for an S cone of order 133 .. 2048: two Choleskys, G = Lz' Ls, its singular values and left
// singular vectors by a block one-sided Jacobi, R and R^-1.  sdp_large.hip has the map of the whole large path.
#include "cip_sdp_large.h"
#include "cip_sdp_numerics.h"
#include "../../include/cipkkt.h"
#include <stdio.h>

// ------------------------------------------------------------------------------------------ element-wise pieces
// T = (L D^1/2)' as a dense matrix, from the factored K (unit L strictly below the diagonal, d separately):
//   T[i, k] = L[k, i] sqrt(d_i)  (k > i),  sqrt(d_i) on the diagonal, 0 below
// L is read from the LOWER triangle (round 5: the factorisation no longer mirrors the 128 x 128 diagonal blocks into the upper
// triangle -- the solves never read them there -- and this kernel was the one reader; a strided read of a <= 8 MB matrix)
__global__ __launch_bounds__(256) void k_lg_tfac(const double *K, const double *d, double *T, int rp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)rp * rp) return;
    const int i = (int)(e % rp), k = (int)(e / rp);
    const double sd = sqrt(d[i]);
    T[e] = (i < k) ? K[k + (long)i * rp] * sd : (i == k ? sd : 0.0);
}
// lam[j] = || G[:, j] ||   (one wave per column)
__global__ __launch_bounds__(256) void k_lg_colnorm(const double *G, double *lam, int rp) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= rp) return;
    double s = 0.0;
    for (int i = lane; i < rp; i += 64) { const double g = G[i + (long)j * rp]; s += g * g; }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) lam[j] = sqrt(s);
}
// operands of the two closing GEMMs of nestod_sdc, from G = U diag(lam) (columns), d_z and the factored K_z:
//   U2t[j, k] = U[k, j] sqrt(lam_j) / sqrt(dz_k)        R    = inv(Lz_unit)' (U2t)'
//   U3t[i, k] = U[k, i] sqrt(dz_k) / sqrt(lam_i)        Rinv = U3t Lz_unit'
//   Lu        = Lz_unit as a dense lower-triangular matrix
__global__ __launch_bounds__(256) void k_lg_build(const double *G, const double *lam, const double *dz, const double *Kz,
                                                   double *U2t, double *U3t, double *Lu, int rp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)rp * rp) return;
    const int k = (int)(e % rp), j = (int)(e / rp);          // element (k, j) of G
    const double u = G[e] / lam[j];
    const double sl = sqrt(lam[j]), sd = sqrt(dz[k]);
    U2t[j + (long)k * rp] = u * sl / sd;
    U3t[j + (long)k * rp] = u * sd / sl;
    Lu[e] = (k > j) ? Kz[e] : (k == j ? 1.0 : 0.0);
}
// compact copies into the packed scaling (R, Rinv: r x r, pitch r) + zero-padded Rinv, Rinv', R, R' (pad[0..3]) for the
// chip-wide congruences; lambda = vecm(diag(lam)) (src/ConicIP.jl:735: lambda = F v = vecm(R' Z R))
__global__ __launch_bounds__(256) void k_lg_store(const double *Rp, const double *Rip_full, double *R, double *Ri, double *pad,
                                                   const double *lam, double *lambda, int r, int rp, int kdim) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < (long)rp * rp) {
        const int i = (int)(e % rp), j = (int)(e / rp);
        const bool in = i < r && j < r;
        const double rv = in ? Rp[e] : 0.0, iv = in ? Rip_full[e] : 0.0;
        if (in) { R[i + (long)j * r] = rv; Ri[i + (long)j * r] = iv; }
        const long n2 = (long)rp * rp, et = j + (long)i * rp;
        pad[e] = iv; pad[n2 + et] = iv; pad[2 * n2 + e] = rv; pad[3 * n2 + et] = rv;
    }
    if (lambda && e < kdim) {
        // diagonal positions of the row-major upper triangle: i r - i (i - 1) / 2
        lambda[e] = 0.0;
    }
}
__global__ __launch_bounds__(256) void k_lg_lambda_diag(const double *lam, double *lambda, int r) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < r) lambda[vidx(i, i, r)] = lam[i];
}
// a non-positive pivot of either Cholesky = the iterate has left the cone: same flag the small-cone kernels raise
__global__ void k_lg_flag(const int *info_a, const int *info_b, int *flag) {
    if (threadIdx.x == 0) {
        if (info_a[0]) *flag = info_a[0];
        else if (info_b && info_b[0]) *flag = info_b[0];
    }
}

// sum over a group of tpp = 32 or 64 consecutive lanes (aligned), in every lane: DPP + lane swaps, no LDS permutes
__device__ __forceinline__ double lg_sum_group(double x, int tpp) {
    x = lz_sum16(x);
    if (tpp == 16) return x;
    return tpp == 64 ? lz_sum_rows(x) : lz_sum_row_pair(x);
}
// ------------------------------------------------------------------------------------------ block one-sided Jacobi
__host__ __device__ inline int lg_pitch(int rows) { return rows + ((4 - rows % 32) + 32) % 32; }   // == 4 (mod 32) doubles
// nbk / 2 workgroups, every column pair rotated exactly once per sweep (cyclic Jacobi), ONE PHASE PER LAUNCH:
//   step 0              workgroup k holds blocks 2k, 2k+1 in LDS: b - 1 rounds of the round-robin tournament inside
//                       each block (b / 2 + b / 2 disjoint pairs per round)
//   step t + 1          round t of the tournament over blocks (nbk - 1 rounds): the workgroup holds its block pair (I, J) and
//                       rotates the b x b cross pairs in b rounds of b disjoint pairs (p in I with p + it in J)
// The launch boundary orders the phases: 255 rotation rounds per sweep at r = 256 -- the depth of the plain parallel ordering.
// (Rounds 3-5 also had ONE persistent launch per NT scaling with a grid barrier per phase and the blocks handed from workgroup to
//  workgroup through `sc1` stores + a counter: about one scaling in 800 / 4000 / 40000 at order 1024 / 512 / 256 came out with other
//  bits and the cause was never found -- DESIGN_LOG.md, round 5.  Round 6 removed that form and its switch: a library must not offer
//  a mode whose documented effect is other bits once in a while.)
// rp / 8 lanes per pair, both columns in registers between the dot products and the rotation.  A sweep behind one that found no
// rotation with cos^2 >= 1e-16 returns at once (the next sweep would find nothing above the 1e-30 threshold: quadratic convergence).
// G_in V = U diag(sigma): column i ends as sigma_i u_i, all of svd(Lz' Ls) that nestod_sdc uses (src/ConicIP.jl:204-208).
// EPL: elements of a column per lane (rp == EPL * tpp): 8 up to order 512; 16 at order 1024 (round 4), where 64 lanes hold a column
template <int NT, int EPL = 8>
__global__ __launch_bounds__(NT) void k_lg_jacobi(double *G, int rp, int bflags, unsigned *ctr) {
    // (8-byte aligned, behind the 264 bytes of s_rot and s_nrm: where the kernel was measured and pinned.  An aligned(16) here had no
    //  effect while the file's other kernels declared their own `sh` without it; alone in its file it would move the base to 272)
    extern __shared__ double sh[];
    const int b = bflags & 0xff;
    const int step_sweep = (bflags >> 16) & 0x3f, step = (bflags >> 22) & 0x1ff;
    __shared__ int s_rot;
    __shared__ double s_nrm[32];
    const int tid = threadIdx.x;
    const int nbk = rp / b, m = nbk;
    const int ld = lg_pitch(rp);
    const int tpp = NT / b;                              // lanes per column pair (32 or 64); rp == EPL * tpp
    const int part = tid % tpp, pair = tid / tpp;
    unsigned *sweepflag = ctr + LG_C_SWEEP;
    // the host enqueues sweeps ahead of reading their flags; a sweep behind one that found nothing to rotate is a no-op
    if (step_sweep > 0 && __hip_atomic_load(sweepflag + step_sweep - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
    // rotation of LDS columns p, q; returns 0 / 1 (rotated, small) / 2 (rotated, cos^2 >= 1e-16)
    auto rotate = [&](int p, int q) -> int {
        double *gp = sh + p * ld, *gq = sh + q * ld;
        double xv[EPL], yv[EPL], a = 0.0, bb = 0.0, c = 0.0;
#pragma unroll
        for (int u = 0; u < EPL; ++u) { xv[u] = gp[part + u * tpp]; yv[u] = gq[part + u * tpp]; }
#pragma unroll
        for (int u = 0; u < EPL; ++u) { a += xv[u] * xv[u]; bb += yv[u] * yv[u]; c += xv[u] * yv[u]; }
        a = lg_sum_group(a, tpp); bb = lg_sum_group(bb, tpp); c = lg_sum_group(c, tpp);
        if (!(c * c > 1e-30 * (a * bb) && c != 0.0)) return 0;
        const double zeta = (bb - a) * 0.5 * sd_rcp(c);
        const double h2 = 1.0 + zeta * zeta;
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) * sd_rcp(fabs(zeta) + h2 * sd_rsqrt(h2));
        const double cs = sd_rsqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
            gp[part + u * tpp] = cs * xv[u] - sn * yv[u];
            gq[part + u * tpp] = sn * xv[u] + cs * yv[u];
        }
        return (c * c > 1e-16 * (a * bb)) ? 2 : 1;
    };
    // a block pair is 2 b rp = 16384 doubles whatever (b, rp): 16 per thread.  All loads of a thread are issued before the first
    // LDS store (one at a time, store after load, each global round trip was exposed: 16 x ~1.5 us per outer round -- half of a
    // sweep's time).  16-byte buffer accesses with the `sc1` policy bit: a relic of the in-launch block exchange (the blocks now
    // change hands across a launch boundary, where plain accesses would do); kept because the one-launch-per-phase form was
    // measured, repeated 11 500 times and pinned bit for bit with exactly these instructions.
    typedef int v4i_t __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void *)G, 0, 0x7fffffff, 0x00020000);
    auto load = [&](int bp, int bq) {                      // coherent loads: other workgroups wrote these blocks
        v4i_t t[EPL];
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
            const int e = 2 * (tid + u * NT), i = e % rp, c = e / rp;
            t[u] = __builtin_amdgcn_raw_buffer_load_b128(grs, (int)((i + (long)(c < b ? bp * b + c : bq * b + (c - b)) * rp) * 8), 0, 16);
        }
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
            const int e = 2 * (tid + u * NT);
            *(v2d *)(sh + e % rp + (e / rp) * ld) = __builtin_bit_cast(v2d, t[u]);
        }
        if (tid == 0) s_rot = 0;
        __syncthreads();
    };
    auto store = [&](int bp, int bq) {
        v2d t[EPL];
#pragma unroll
        for (int u = 0; u < EPL; ++u) { const int e = 2 * (tid + u * NT); t[u] = *(const v2d *)(sh + e % rp + (e / rp) * ld); }
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
            const int e = 2 * (tid + u * NT), i = e % rp, c = e / rp;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i_t, t[u]), grs, (int)((i + (long)(c < b ? bp * b + c : bq * b + (c - b)) * rp) * 8), 0, 16);
        }
    };
    int rotated = 0;
    if (step == 0) {
        // ---- pairs inside the blocks
        const int bp = 2 * (int)blockIdx.x, bq = bp + 1;
        load(bp, bq);
        const int hb = b / 2, blk = pair / hb, kk = pair % hb;
        for (int it = 0; it < b - 1; ++it) {
            int p, q;
            if (kk == 0) { p = b - 1; q = it; }
            else { p = (it + kk) % (b - 1); q = (it - kk + (b - 1)) % (b - 1); }
            const int rr = rotate(blk * b + p, blk * b + q);
            if (rr && part == 0) atomicMax(&s_rot, rr);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        rotated = s_rot > rotated ? s_rot : rotated;
        store(bp, bq);
    } else {
        // ---- pairs across blocks: round t = step - 1 of the tournament
        const int t = step - 1;
        int bp, bq;
        const int k = blockIdx.x;
        if (k == 0) { bp = m - 1; bq = t; }
        else { bp = (t + k) % (m - 1); bq = (t - k + (m - 1)) % (m - 1); }
        load(bp, bq);
        {
            // column p = `pair` of block I stays with this lane group for all b rounds: it lives in registers, its
            // squared norm `a` and the partners' (s_nrm, in LDS) follow the rotations (a' = a - t c, b' = b + t c)
            // instead of being re-summed -- a round is then one dot product, 8 LDS loads and 8 stores per lane
            double *gp = sh + pair * ld;
            double xv[EPL], a = 0.0;
#pragma unroll
            for (int u = 0; u < EPL; ++u) { xv[u] = gp[part + u * tpp]; a += xv[u] * xv[u]; }
            {
                double *gq0 = sh + (b + pair) * ld;
                double bq2 = 0.0;
#pragma unroll
                for (int u = 0; u < EPL; ++u) { const double y = gq0[part + u * tpp]; bq2 += y * y; }
                a = lg_sum_group(a, tpp); bq2 = lg_sum_group(bq2, tpp);
                if (part == 0) s_nrm[pair] = bq2;
            }
            __syncthreads();
            for (int it = 0; it < b; ++it) {
                const int qi = (pair + it) % b;
                double *gq = sh + (b + qi) * ld;
                double yv[EPL], c = 0.0;
#pragma unroll
                for (int u = 0; u < EPL; ++u) { yv[u] = gq[part + u * tpp]; c += xv[u] * yv[u]; }
                c = lg_sum_group(c, tpp);
                const double bb = s_nrm[qi];
                if (c * c > 1e-30 * (a * bb) && c != 0.0) {
                    const double zeta = (bb - a) * 0.5 * sd_rcp(c);
                    const double h2 = 1.0 + zeta * zeta;
                    const double tt = (zeta >= 0.0 ? 1.0 : -1.0) * sd_rcp(fabs(zeta) + h2 * sd_rsqrt(h2));
                    const double cs = sd_rsqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
                    for (int u = 0; u < EPL; ++u) {
                        const double x = xv[u];
                        xv[u] = cs * x - sn * yv[u];
                        gq[part + u * tpp] = sn * x + cs * yv[u];
                    }
                    if (part == 0) { s_nrm[qi] = bb + tt * c; atomicMax(&s_rot, (c * c > 1e-16 * (a * bb)) ? 2 : 1); }
                    a -= tt * c;
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
#pragma unroll
            for (int u = 0; u < EPL; ++u) gp[part + u * tpp] = xv[u];
            __syncthreads();
        }
        rotated = s_rot > rotated ? s_rot : rotated;
        store(bp, bq);
    }
    if (tid == 0 && rotated == 2) atomicAdd(sweepflag + step_sweep, 1u);
}
// dst = src' (optionally row j of dst scaled by 1 / sc[j]^2), rp x rp through a 32 x 33 LDS tile
__global__ __launch_bounds__(256) void k_lg_transpose(const double *src, double *dst, int rp, const double *sc) {
    __shared__ double t[32][33];
    const int bi = blockIdx.x * 32, bj = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int q = 0; q < 32; q += 8) t[ty + q][tx] = src[(bi + tx) + (long)(bj + ty + q) * rp];        // t[j][i] = src[i, j]
    __syncthreads();
    for (int q = 0; q < 32; q += 8) {
        const int j = bj + tx, i = bi + ty + q;                                                      // dst[j, i] = src[i, j]
        double v = t[tx][ty + q];
        if (sc) { const double s1 = sc[j]; v = v / (s1 * s1); }
        dst[j + (long)i * rp] = v;
    }
}
// M <- 1.5 I - 0.5 M   (the Newton-Schulz factor of V <- V (3 I - V'V) / 2)
// M = V'V  ->  1.5 I - 0.5 M (the Newton-Schulz factor); vst[1] = max |V'V - I| as the bit pattern of a non-negative double
// (monotone for finite values; NaN / inf compare as larger than every finite tolerance): what the gate below looks at
__global__ __launch_bounds__(256) void k_lg_ns(double *M, int rp, unsigned long long *vst) {
    __shared__ unsigned long long smax;
    if (threadIdx.x == 0) smax = 0ull;
    __syncthreads();
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < (long)rp * rp) {
        const double d = ((e % rp) == (e / rp)) ? 1.0 : 0.0, mv = M[e];
        M[e] = 1.5 * d - 0.5 * mv;
        atomicMax(&smax, (unsigned long long)__double_as_longlong(fabs(mv - d)));
    }
    __syncthreads();
    if (threadIdx.x == 0 && smax) atomicMax(vst + 1, smax);
}
// Round 6 (advisor): the warm start must not be taken from a V that is not a (near-)orthogonal matrix -- the previous scaling of
// this cone came from an iterate outside the cone (sqrt of a negative pivot: G, lam, V all NaN), or from a G so ill-conditioned
// that V = G'A_f Sigma^-2 is orthogonal to less than what ONE Newton-Schulz step repairs to rounding (e <= 1e-6 -> 4e-13).  Decided
// on the device, no read-back: vst[0] = 1 when the previous call ended with clean Cholesky flags and finite positive singular
// values (k_lg_vok), vst[1] from k_lg_ns; otherwise G <- G0, i.e. exactly the cold start.
#define LG_WARM_TOL 1e-6
__global__ __launch_bounds__(256) void k_lg_warm_gate(double *G, const double *G0, long n2, const unsigned long long *vst) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n2) return;
    if (vst[0] != 1ull || vst[1] > (unsigned long long)__double_as_longlong(LG_WARM_TOL)) G[e] = G0[e];
}
__global__ __launch_bounds__(256) void k_lg_vok(const double *lam, int rp, const int *info_a, const int *info_b, unsigned long long *vst) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = (info_a[0] != 0 || info_b[0] != 0) ? 1 : 0;
    __syncthreads();
    for (int j = threadIdx.x; j < rp; j += 256) { const double l = lam[j]; if (!(l > 0.0 && l < 1.7e308)) bad = 1; }
    __syncthreads();
    if (threadIdx.x == 0) { vst[0] = bad ? 0ull : 1ull; vst[1] = 0ull; }
}
// a sweep's flag and the two Cholesky flags -> host-mapped memory, the sequence word behind them with system-scope release (the
// pattern of api.hip: k_publish_info): the host polls the word instead of a 4-byte copy + stream synchronisation per checked sweep
__global__ void k_lg_pubflag(const unsigned *sweepflag, const int *info_a, const int *info_b, int *host, int seq) {
    if (threadIdx.x == 0) {
        host[0] = (int)(*sweepflag != 0u);
        host[1] = (info_a[0] != 0 || info_b[0] != 0) ? 1 : 0;
        __hip_atomic_store(host + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------------------------------ host side: the steps of one NT scaling
// chol(mat(z)), chol(mat(s)), the cone flag and G = Lz' Ls
static int nt_factor(hipStream_t s, LargeWs *w, const ConeDesc &cd, const double *v, const double *sv, int *flag) {
    const int r = cd.r, rp = w->rp;
    const long n2 = (long)rp * rp;
    lg_mat(s, v + cd.off, 1L, 0L, w->Kz, r, rp, 1.0);
    lg_mat(s, sv + cd.off, 1L, 0L, w->Ks, r, rp, 1.0);
    CIP_TRY(cip_ldlt_factor(s, w->Kz, rp, rp, w->wz));                              // Lz (unit) and d_z  (:202-203)
    CIP_TRY(cip_ldlt_factor(s, w->Ks, rp, rp, w->ws));
    hipLaunchKernelGGL(k_lg_flag, dim3(1), dim3(64), 0, s, w->wz.info, w->ws.info, flag);
    hipLaunchKernelGGL(k_lg_tfac, lg_grid(n2), dim3(256), 0, s, w->Kz, w->wz.dvec, w->Tz, rp);
    hipLaunchKernelGGL(k_lg_tfac, lg_grid(n2), dim3(256), 0, s, w->Ks, w->ws.dvec, w->Ts, rp);
    return lg_gemm(s, w->G, 0, w->Tz, 0, w->Ts, 0, rp, 1);                          // G = Lz' Ls          (:204)
}
// Round 5: WARM START of the one-sided Jacobi.  svd(G) = U Sigma V' is needed for U and Sigma only (:204-208), and the
// Jacobi may start from G W for ANY orthogonal W: the left singular vectors and the singular values are those of G.
// Between two interior-point iterations the NT scaling moves little, so with W = the right singular vectors V of the previous
// scaling of this cone the columns of G W are already nearly orthogonal and the sweeps drop from 8 to 2-4 (each sweep of order
// 256 is 255 latency-bound rotation rounds, 0.38 ms: the NT scaling was 30 % of config 4's iteration).  V is not tracked
// through the rotations: afterwards, with the columns A_f = U Sigma in hand, V = G' A_f Sigma^-2 is one GEMM (nt_keep_v); before it
// is used again one Newton-Schulz step V <- V (3 I - V'V) / 2 restores its orthogonality to rounding (G' U Sigma^-1 is orthogonal
// only to cond(G) eps, and a W that is not orthogonal would change the answer by that much).  Four extra 256^3 products per
// scaling (~5 us each).  The first scaling after the packed scaling was replaced from outside (cip_set_scaling_identity at the
// start of every interior-point solve, cip_set_scaling_packed) starts cold: a solve's results do not depend on what the handle
// did before.  G0 keeps the cold start either way: the gate falls back to it, nt_keep_v builds V from it.
static int nt_warm_start(hipStream_t s, LargeWs *w, int li, bool warm) {
    const int rp = w->rp;
    const long n2 = (long)rp * rp;
    const dim3 tg(rp / 32, rp / 32);
    const double *Vw = w->Vw + (size_t)li * n2;
    unsigned long long *vst = w->vstate + 2 * (size_t)li;
    CIP_HIP_CHECK(hipMemcpyAsync(w->G0, w->G, sizeof(double) * n2, hipMemcpyDeviceToDevice, s));
    if (!warm) return 0;
    hipLaunchKernelGGL(k_lg_transpose, tg, dim3(256), 0, s, Vw, w->W1, rp, (const double *)nullptr);                        // V'
    CIP_TRY(lg_gemm(s, w->W2, 0, w->W1, 0, w->W1, 0, rp, 1));                                                               // V'V
    hipLaunchKernelGGL(k_lg_ns, lg_grid(n2), dim3(256), 0, s, w->W2, rp, vst);                                              // 1.5 I - 0.5 V'V (symmetric); max |V'V - I|
    CIP_TRY(lg_gemm(s, w->W1, 0, Vw, 0, w->W2, 0, rp, 1));                                                                  // Vn = V (1.5 I - 0.5 V'V)
    hipLaunchKernelGGL(k_lg_transpose, tg, dim3(256), 0, s, (const double *)w->W1, w->W2, rp, (const double *)nullptr);      // Vn'
    CIP_TRY(lg_gemm(s, w->G, 0, w->G0, 0, w->W2, 0, rp, 1));                                                                // G <- G Vn
    hipLaunchKernelGGL(k_lg_warm_gate, lg_grid(n2), dim3(256), 0, s, w->G, (const double *)w->G0, n2, (const unsigned long long *)vst);   // ... unless V is not fit for it: G <- G0 (cold)
    return 0;
}
// ONE LAUNCH PER PHASE (round 5, second session; the only form since round 6): the pairs inside the blocks, then each round of
// the tournament over blocks, the launch boundary in place of a grid barrier.  0 differing results in 11 500 repeated scalings
// at orders 256 ... 1024 and in 40 000 at order 256 (profiles/r5/jacobi_repeatability.txt).  The host enqueues whole sweeps; a
// sweep behind a converged one is a no-op (the kernel's gate), so the sweep flags are read only from the sweep on that is
// usually the last but one (warm start: 6-8 sweeps, cold: 9-11) -- through host-mapped memory (k_lg_pubflag: a one-wave kernel
// and a polled word; until round 6 a 4-byte copy + stream synchronisation per checked sweep).
// The column blocks (cip_sdp_large_forms.h: lg_jacobi_form) are 8 wide at order 256 (16 workgroups of 256 threads; round 4, with
// the DPP sums: 4 / 8 / 16 / 32 wide -> 3.95 / 3.11 / 3.25 / 4.48 ms per NT scaling -- a rotation round is bound by the hand-over
// between the wave's lane groups (LDS + workgroup barrier: fewer waves per workgroup, shorter rounds), an outer round costs ~3 us
// (block exchange through L2 + launch boundary) and their number doubles as the blocks halve), 16 at order 512 (16 workgroups), 8
// at order 1024, 4 at order 2048.  *left_cone: either Cholesky met a non-positive pivot (read back with the sweep flags).
static int nt_sweeps(hipStream_t s, LargeWs *w, bool warm, bool *converged, bool *left_cone) {
    const int rp = w->rp;
    const LgJacobiForm jf = lg_jacobi_form(rp);
    void (*kern)(double *, int, int, unsigned *) = nullptr;      // (a template argument needs a constant: the one switch on the form)
    switch (jf.kernel) {
        case LG_JACOBI_256_8: kern = k_lg_jacobi<256>; break;
        case LG_JACOBI_1024_8: kern = k_lg_jacobi<1024>; break;
        case LG_JACOBI_512_16: kern = k_lg_jacobi<512, 16>; break;
        case LG_JACOBI_256_32: kern = k_lg_jacobi<256, 32>; break;
    }
    const size_t lds = (size_t)2 * jf.block * lg_pitch(rp) * sizeof(double);
    CIP_TRY(lg_set_attr((const void *)kern, lds));
    const int m = rp / jf.block;
    const int first_check = warm ? 4 : 7;
    for (int sweep = 0; sweep < 40; ++sweep) {
        for (int step = 0; step < m; ++step)
            hipLaunchKernelGGL(kern, dim3(m / 2), dim3(jf.threads), lds, s, w->G, rp, jf.block | (sweep << 16) | (step << 22), w->ctr);
        if (sweep < first_check) continue;
        w->hseq = (w->hseq == 0x7fffffff) ? 1 : w->hseq + 1;
        hipLaunchKernelGGL(k_lg_pubflag, dim3(1), dim3(64), 0, s, (const unsigned *)(w->ctr + LG_C_SWEEP + sweep), (const int *)w->wz.info, (const int *)w->ws.info, w->hflag_dev, w->hseq);
        CIP_HIP_CHECK(hipGetLastError());
        CIP_TRY(cip_await_seq(s, w->hflag + 2, w->hseq, "NT scaling of an S cone: the Jacobi's sweep flag"));
        *left_cone = w->hflag[1] != 0;
        if (!w->hflag[0]) { *converged = true; break; }
    }
    return 0;
}
// V = G0' (A_f Sigma^-2) for the next call, and whether it is fit for that call's warm start.  The host knows the Cholesky flags
// from the sweep read-back (an iterate outside the cone leaves NaN in G, lam and V: round 5 kept such a V, and the next scaling of a
// perfectly interior iterate came out NaN with a clean flag); the device-side word also covers non-finite / non-positive singular
// values (k_lg_warm_gate reads it)
static int nt_keep_v(hipStream_t s, LargeWs *w, int li, const double *lam, bool left_cone) {
    const int rp = w->rp;
    const dim3 tg(rp / 32, rp / 32);
    hipLaunchKernelGGL(k_lg_transpose, tg, dim3(256), 0, s, (const double *)w->G, w->W1, rp, lam);                           // (A_f Sigma^-2)'
    hipLaunchKernelGGL(k_lg_transpose, tg, dim3(256), 0, s, (const double *)w->G0, w->W2, rp, (const double *)nullptr);      // G0'
    CIP_TRY(lg_gemm(s, w->Vw + (size_t)li * rp * rp, 0, w->W2, 0, w->W1, 0, rp, 1));
    hipLaunchKernelGGL(k_lg_vok, dim3(1), dim3(256), 0, s, lam, rp, (const int *)w->wz.info, (const int *)w->ws.info, w->vstate + 2 * (size_t)li);
    w->have_v[li] = left_cone ? 0 : 1;
    return 0;
}
// R = Lz^-T U Lambda^1/2 and R^-1 = Lambda^-1/2 U' Lz'  (:206-208) into the packed scaling and the padded copies; lambda
static int nt_scaling(hipStream_t s, LargeWs *w, const ConeDesc &cd, int li, const double *lam, double *scal, double *lambda) {
    const int r = cd.r, rp = w->rp;
    const long n2 = (long)rp * rp;
    hipLaunchKernelGGL(k_lg_build, lg_grid(n2), dim3(256), 0, s, w->G, lam, w->wz.dvec, w->Kz, w->M1, w->M2, w->M3, rp);
    const double *XTz = (w->wz.Bs == CIP_NB) ? w->wz.LinvT : w->wz.XT;             // inv(Lz_unit)' (one block = the matrix)
    CIP_TRY(lg_gemm(s, w->Tz, 0, XTz, 0, w->M1, 0, rp, 1));                         // R    = Lz^-T U Lambda^1/2
    CIP_TRY(lg_gemm(s, w->Ts, 0, w->M2, 0, w->M3, 0, rp, 1));                       // Rinv = Lambda^-1/2 U' Lz'
    double *R = scal + cd.soff, *Ri = R + (size_t)r * r;
    hipLaunchKernelGGL(k_lg_store, lg_grid(n2 > cd.dim ? n2 : cd.dim), dim3(256), 0, s, w->Tz, w->Ts, R, Ri, w->Rip + LG_NPAD * (size_t)li * n2,
                       lam, lambda ? lambda + cd.off : nullptr, r, rp, cd.dim);
    if (lambda) hipLaunchKernelGGL(k_lg_lambda_diag, lg_grid(r), dim3(256), 0, s, lam, lambda + cd.off, r);
    CIP_HIP_CHECK(hipGetLastError());
    return 0;
}

// nestod_sdc for one large cone (index li among the large cones)
int cip_sdp_large_nt(hipStream_t s, LargeWs *w, const ConeDesc &cd, int li, const double *v, const double *sv, double *scal,
                     double *lambda, int *flag) {
    const bool warm = w->have_v[li] != 0;
    CIP_TRY(nt_factor(s, w, cd, v, sv, flag));
    CIP_TRY(nt_warm_start(s, w, li, warm));
    bool converged = false, left_cone = false;
    CIP_HIP_CHECK(hipMemsetAsync(w->ctr, 0, LG_C_WORDS * sizeof(unsigned), s));
    CIP_TRY(cip_prof_slot_begin(CIP_PROF_JACOBI, s, 0.0));
    const int rc = nt_sweeps(s, w, warm, &converged, &left_cone);
    const int rce = cip_prof_slot_end(CIP_PROF_JACOBI, s);      // (also on the error paths: an unpaired event would mis-pair every later collect)
    if (rc) return rc;
    if (rce) return rce;
    if (!converged) {
        // (never seen: the cyclic one-sided Jacobi converges quadratically; a scaling built on unconverged columns would be silently wrong)
        w->have_v[li] = 0;
        cip_set_error("NT scaling of an S cone of order %d: the one-sided Jacobi still rotated after 40 sweeps", cd.r);
        return CIP_E_SINGULAR;
    }
    if (cip_env_set("CIP_LG_DEBUG")) {
        unsigned hc[64];
        CIP_HIP_CHECK(hipMemcpyAsync(hc, w->ctr, sizeof(hc), hipMemcpyDeviceToHost, s));
        CIP_HIP_CHECK(hipStreamSynchronize(s));
        int sweeps = 0;
        for (int q = LG_C_SWEEP; q < LG_C_SWEEP + 40; ++q) if (hc[q]) ++sweeps;
        fprintf(stderr, "[lg] jacobi: %d sweeps with a rotation above cos^2 = 1e-16%s\n", sweeps, left_cone ? " (iterate outside the cone)" : "");
    }
    double *lam = w->slot(LG_V_LAM);
    hipLaunchKernelGGL(k_lg_colnorm, dim3((w->rp + 3) / 4), dim3(256), 0, s, w->G, lam, w->rp);
    CIP_TRY(nt_keep_v(s, w, li, lam, left_cone));
    return nt_scaling(s, w, cd, li, lam, scal, lambda);
}
