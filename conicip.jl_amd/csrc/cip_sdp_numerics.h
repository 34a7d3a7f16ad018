// What the S-cone kernels of sdp.hip (one workgroup per cone) and sdp_large.hip (chip-wide pieces) compute the same way: the vecm
// index arithmetic, the Newton-refined reciprocals, the Householder reflector of the tridiagonalisations, the scaled symmetrised
// matrix the max-step takes its eigenvalue of, the extreme eigenvalue of a tridiagonal matrix and the verdict of maxstep_sdc
// (src/ConicIP.jl:272-303).  One copy each: a change to the numerics is a change to every form.  Three forms sum or count in an
// order of their own and stay where they are: tg_block_sum, lz_sum256 and the division-free Sturm count inside k_lg_lanczos1.
#pragma once
#include <math.h>

#define SQRT2 1.4142135623730951
#define SQRT1_2 0.7071067811865476

#ifdef __HIPCC__
// vecm layout (upper triangle by rows, src/ConicIP.jl:85-151): position of entry (i, j), i <= j, and of the diagonal entry (i, i)
__device__ __forceinline__ int vidx(int i, int j, int r) { return i * r - i * (i - 1) / 2 + (j - i); }
__device__ __forceinline__ long vrowoff(int i, int r) { return (long)i * r - (long)i * (i - 1) / 2; }

// Newton-refined hardware reciprocal / reciprocal square root (v_rcp_f64, v_rsq_f64 give ~2^-26; two steps reach
// the last bits): a handful of instructions where the IEEE division / sqrt expansions cost 30-40 each.  Used where the
// value feeds a rotation or a multiplier of a serial chain that every lane recomputes (the chains are issue-bound).
__device__ __forceinline__ double sd_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    r = fma(r, fma(-d, r, 1.0), r);
    return r;
}
__device__ __forceinline__ double sd_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    return r;
}

// Workgroup barriers, as functors for the two routines below.  SdSyncLds: the data exchanged lives in LDS, so only lgkmcnt has to
// drain -- __syncthreads() also waits for every outstanding global access (vmcnt(0)), which would expose the latency of prefetched
// global loads at every step of a serial chain.
struct SdSyncLds { __device__ __forceinline__ void operator()() const { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); } };
struct SdSyncAll { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

// sum over the workgroup (nwaves waves), in every thread: xor-shuffles inside a wave, then the waves' sums in wave order.
// red: nwaves doubles of LDS, free again after the next barrier
template <class Sync>
__device__ __forceinline__ double sd_block_sum(double x, double *red, int nwaves, Sync sync) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    sync();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    sync();
    double sum = 0.0;
    for (int q = 0; q < nwaves; ++q) sum += red[q];
    return sum;
}

// Householder reflector H = I - beta v v' that maps x (first entry x0, squared norm sigma) onto alpha e1: v = x - alpha e1,
// beta = 2 / |v|^2.  flat: x is a multiple of e1 already (or the caller says so: a column of length 1) -- H = I, alpha = x0, beta = 0
struct SdReflector { bool flat; double alpha, beta; };
__device__ __forceinline__ SdReflector sd_reflector(double sigma, double x0, bool is_flat = false) {
    SdReflector h;
    h.flat = is_flat || !(sigma - x0 * x0 > 0.0);
    h.alpha = h.flat ? x0 : -copysign(sqrt(sigma), x0);
    h.beta = h.flat ? 0.0 : 1.0 / (sigma - x0 * h.alpha);
    return h;
}

// Entry (i, j) of the matrix the max-step takes its extreme eigenvalue of: 0.5 (M + M') .* (rs rs') with rs = dscale^-1/2, or M
// itself when there is no dscale -- M is then mat(x) or an image of this very function, symmetric to the bit, and the one load
// M[i + j ldm] gives the same value as the mean of the pair.  The caller picks (i, j) so that this load is its coalesced one.
__device__ __forceinline__ double sd_scaled_sym_entry(const double *M, int ldm, const double *dscale, int i, int j) {
    double x = M[i + (long)j * ldm];
    if (dscale) x = 0.5 * (M[j + (long)i * ldm] + x) * (rsqrt(dscale[j]) * rsqrt(dscale[i]));
    return x;
}

// Extreme eigenvalue (want_max: the largest, else the smallest) of the symmetric tridiagonal matrix with diagonal dg[0..r) and
// sub-diagonal of[0..r-1), both in LDS and published: Gershgorin interval, then multisection on the Sturm count, one shift per
// thread and round, down to the last bits.  Called by all nthreads threads of the workgroup; red: 32 doubles, first: one int of
// LDS.  The result is the same in every thread.
template <class Sync>
__device__ __forceinline__ double sd_tridiag_extreme(const double *dg, const double *of, int r, bool want_max, int nthreads,
                                                     double *red, int *first, Sync sync) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int i = tid; i < r; i += nthreads) {
        const double rad = (i > 0 ? fabs(of[i - 1]) : 0.0) + (i + 1 < r ? fabs(of[i]) : 0.0);
        lo = fmin(lo, dg[i] - rad);
        hi = fmax(hi, dg[i] + rad);
    }
    for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o)); hi = fmax(hi, __shfl_xor(hi, o)); }
    sync();
    if (lane == 0) { red[wave] = lo; red[16 + wave] = hi; }
    sync();
    lo = red[0]; hi = red[16];
    for (int q = 1; q < nthreads / 64; ++q) { lo = fmin(lo, red[q]); hi = fmax(hi, red[16 + q]); }
    const double span = fmax(fabs(lo), fabs(hi));
    hi += 1e-15 * span + 1e-300;                               // the count at hi must be r, at lo 0
    lo -= 1e-15 * span + 1e-300;
    for (int round = 0; round < 12; ++round) {
        if (!(hi - lo > 4.4e-16 * fmax(fabs(lo), fabs(hi)))) break;
        const double step = (hi - lo) / (nthreads + 1);
        const double xs = lo + step * (tid + 1);
        // Sturm count: number of eigenvalues below xs
        int cnt = 0;
        double q = dg[0] - xs;
        if (q < 0.0) ++cnt;
        for (int i = 1; i < r; ++i) {
            if (q == 0.0) q = 1e-300;
            q = (dg[i] - xs) - of[i - 1] * of[i - 1] / q;
            if (q < 0.0) ++cnt;
        }
        const bool hit = want_max ? (cnt >= r) : (cnt >= 1);   // monotone in tid
        if (tid == 0) *first = nthreads;
        sync();
        if (hit) atomicMin(first, tid);
        sync();
        const int f = *first;
        sync();
        const double nlo = (f == 0) ? lo : lo + step * f;       // x_{f-1}
        const double nhi = (f == nthreads) ? hi : lo + step * (f + 1);
        lo = nlo; hi = nhi;
    }
    return 0.5 * (lo + hi);
}

// The verdict of maxstep_sdc.  With a direction: the largest step that keeps x - step scale d in the cone, from lambda_max of
// X^-1/2 D X^-1/2 -- Inf when nothing limits it (:290-293).  Without (`nothing`): how far x is outside the cone, 0 inside, from
// the smallest eigenvalue (:295-303; the R cone's form of it, :227-240, is the same expression on the smallest entry)
__device__ __forceinline__ double cip_maxstep_nothing(double mn) { return (mn > 0.0) ? 0.0 : -1.0 + mn; }
__device__ __forceinline__ double sd_maxstep_verdict(bool want_max, double ev, double scale) {
    if (!want_max) return cip_maxstep_nothing(ev);
    const double mx = ev * scale;
    return (mx < 0.0) ? __builtin_inf() : 1.0 / mx;
}
#endif
