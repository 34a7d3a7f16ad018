// Batches of SMALL conic programs, one workgroup per problem (include/cipkkt.h: cip_conicip_small).
//
// Every other path of the library pays a launch chain per interior-point iteration whatever the problem size.
// Here a problem of order n + p <= 128 with m <= 1024 cone rows is ONE 256-thread workgroup: its KKT matrix [S G'; G 0],
// S = Q + A'(F'F)^-1 A, lives in the CU's LDS for the whole step, and nothing outside the workgroup is waited for.  Per iteration the
// call issues two launches and one read-back, whatever the number of problems:
//
//   k_small_residuals   one workgroup per live problem: NT scaling and lambda (src/ConicIP.jl:732-735), the residuals (:746-753)
//                       and the 16 dot products of IterDots (cip_driver_scalars.h), written to row z of a count x 16 buffer
//   (host)              the verdict of src/ConicIP.jl:756-873 per problem -- evaluate_iteration, the one copy every loop calls --
//                       and the list of live problem indices (a device array: no 64-bit mask, no group limit)
//   k_small_step        one workgroup per live problem, everything else of the iteration: Schur matrix into LDS on
//                       v_mfma_f64_16x16x4_f64, unpivoted right-looking LDL' in LDS, predictor (:879-887), corrector (:893-901),
//                       Newton step with iterative refinement against the 4x4 operator (:907-921), step lengths and update (:927-932)
//
// The algorithm is Loop::run of driver.hip.  The factorisation of an iteration sits behind the verdict instead of in front of it (the
// terminating iteration's is skipped; n_factor counts it all the same, as cip_conicip does), so a bad pivot is seen one read-back
// later: the problem has taken one meaningless step by then, leaves the live list and is solved from the start by cip_conicip_mixed.
//
// Determinism: every sum has a fixed order that depends on the problem's dimensions alone -- lane-strided partial sums, xor
// butterflies, wave partials added in wave order, k-panels in ascending order -- so a problem's bits do not depend on count, on its
// index or on the run.  No workgroup reads, waits for or signals another; every loop is bounded by a dimension, maxRefinementSteps or
// (on the host) maxIters; __syncthreads() and LDS are the only coordination.
//
// The cone bodies are written after the kernels of cones.hip (k_nt_scaling :72-123, k_apply :151-192, k_scale_At :199-221,
// k_cone_prod :282-308, k_cone_div :311-340, k_maxstep :345-408) and the element-wise chains of vecops.hip (k_loop_resid, k_loop_corr,
// k_loop_refine); they are copies for one workgroup per problem, not shared device functions: a shared tile body has changed another
// kernel's code generation before (k_gemm_nt_16_batched).
#include "cip_batch_front.h"
#include "cip_driver_scalars.h"
#include <math.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

namespace {

struct SmallCone { int type, off, dim, soff; };    // one per cone, shared by every problem of the call

// problem 0's pointers; problem z's are the same + z * stride
struct SmallSlab {
    double *c, *b, *d, *Q, *A, *G;                 // uploaded (Q n x n, A m x n, G p x n, column-major, compact)
    double *At, *Gt, *W;                           // A' (n x m), G' (n x p), A' F^-1 (n x m): k_small_prepare / k_small_step
    double *z, *r0, *r, *daff, *dz, *dzr, *rIr;    // 4-block vectors (y[n], w[p], v[m], s[m])
    double *lam, *scal, *e, *Qy, *pinf, *Ays, *Gy; // lambda, packed scaling (R: k, Q: 1 + k), cone identity, certificate vectors
    double *q, *t, *t1, *u, *tmp, *mb1, *mb2, *x3; // scratch (m each; x3: n + p)
};
size_t small_layout(const void *base, int n, int m, int p, size_t scal_len, SmallSlab *S, size_t *host_prefix, size_t *dev_prefix) {
    CipLayout L(base);
    const size_t NT = (size_t)n + p + 2 * (size_t)m;
    S->c = L.take<double>(n); S->b = L.take<double>(m); S->d = L.take<double>(p);
    if (dev_prefix) *dev_prefix = L.bytes();       // device-pointer problems: c, b, d come from the host, the matrices from the device
    S->Q = L.take<double>((size_t)n * n); S->A = L.take<double>((size_t)m * n); S->G = L.take<double>((size_t)p * n);
    if (host_prefix) *host_prefix = L.bytes();
    S->At = L.take<double>((size_t)m * n); S->Gt = L.take<double>((size_t)p * n); S->W = L.take<double>((size_t)m * n);
    S->z = L.take<double>(NT); S->r0 = L.take<double>(NT); S->r = L.take<double>(NT); S->daff = L.take<double>(NT);
    S->dz = L.take<double>(NT); S->dzr = L.take<double>(NT); S->rIr = L.take<double>(NT);
    S->lam = L.take<double>(m); S->scal = L.take<double>(scal_len); S->e = L.take<double>(m);
    S->Qy = L.take<double>(n); S->pinf = L.take<double>(n); S->Ays = L.take<double>(m); S->Gy = L.take<double>(p);
    S->q = L.take<double>(m); S->t = L.take<double>(m); S->t1 = L.take<double>(m); S->u = L.take<double>(m);
    S->tmp = L.take<double>(m); S->mb1 = L.take<double>(m); S->mb2 = L.take<double>(m); S->x3 = L.take<double>((size_t)n + p);
    return L.bytes();
}

struct SmallSrc { const double *Q, *A, *G; int ldq, lda, ldg; };    // a device-pointer problem's matrices

struct SmallArgs {
    SmallSlab S;
    long stride8;                  // slab stride in doubles
    int n, m, p, ncones;
    int ldk, kcols, pld;           // LDS: K is ldk x kcols (ldk odd: rows and columns both conflict-free), a k-panel pld x 16
    const SmallCone *cones;
    const int *live;               // live problem indices (NULL: blockIdx.x itself)
    double *dots;                  // count x 16
    int *flags, *nref;             // per problem: 1-based column of a bad pivot (0: none); refinement solves of its last step
    double conedim, DTB, refThr;
    int maxRef, init;
};

// LDS of k_small_step in doubles: K, the k-panel, then rhs[128] cw[128] red[16] part[256]
#define SMALL_TAIL 528
size_t small_lds_bytes(int ldk, int kcols, int pld) { return sizeof(double) * ((size_t)ldk * kcols + (size_t)pld * 16 + SMALL_TAIL); }

#define SMALL_T 256

// ---------------------------------------------------------------- reductions (fixed order, every thread gets the result)
__device__ __forceinline__ double sm_wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double sm_wmin(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ void sm_bsum4(double &a, double &b, double &c, double &d, double *red /* 16 */) {
    a = sm_wsum(a); b = sm_wsum(b); c = sm_wsum(c); d = sm_wsum(d);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[4 + w] = b; red[8 + w] = c; red[12 + w] = d; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
    c = (red[8] + red[9]) + (red[10] + red[11]);
    d = (red[12] + red[13]) + (red[14] + red[15]);
}
// NaN-propagating minimum over the workgroup (Julia's min propagates NaN, src/ConicIP.jl:582; cones.hip: k_min_reduce)
__device__ __forceinline__ double sm_bmin(double mn, int nan_seen, double *red) {
    mn = sm_wmin(mn);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = mn;
    __syncthreads();
    const double r = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    return __syncthreads_or(nan_seen) ? __builtin_nan("") : r;
}
__device__ __forceinline__ double sm_dot1(int len, const double *x, const double *y, double *red) {
    double a = 0, b = 0, c = 0, d = 0;
    for (int e = threadIdx.x; e < len; e += SMALL_T) a += x[e] * y[e];
    sm_bsum4(a, b, c, d, red);
    return a;
}

// out[r] = alpha * sum_c M[r + c ld] x[c] + beta * out[r] (beta == 0: out is not read), r < rows.  Up to 128 rows: the columns are cut
// into 256 / rows slices, the slices' partial sums added in slice order.  Ends with a barrier.
__device__ __forceinline__ void sm_gemv(int rows, int cols, const double *M, long ld, const double *x, double alpha, double beta, double *out,
                                        double *part /* 256 */) {
    if (rows <= 0) return;
    const int tid = threadIdx.x;
    if (rows > 128) {
        for (int r = tid; r < rows; r += SMALL_T) {
            double acc = 0.0;
            for (int c = 0; c < cols; ++c) acc += M[r + (long)c * ld] * x[c];
            out[r] = beta != 0.0 ? alpha * acc + beta * out[r] : alpha * acc;
        }
        __syncthreads();
        return;
    }
    const int P = SMALL_T / rows, pi = tid / rows, r = tid - pi * rows;
    if (pi < P) {
        const int chunk = (cols + P - 1) / P, c0 = pi * chunk, c1 = min(cols, c0 + chunk);
        double acc = 0.0;
        for (int c = c0; c < c1; ++c) acc += M[r + (long)c * ld] * x[c];
        part[pi * rows + r] = acc;
    }
    __syncthreads();
    if (tid < rows) {
        double s = 0.0;
        for (int q = 0; q < P; ++q) s += part[q * rows + tid];
        out[tid] = beta != 0.0 ? alpha * s + beta * out[tid] : alpha * s;
    }
    __syncthreads();
}

// ---------------------------------------------------------------- cone bodies: R elements over all threads, a Q cone per wave
// (Q cones are dealt to the four waves in turn; a wave's reductions are lane-strided sums + an xor butterfly: no barrier inside)
#define SM_CONES_BEGIN(a)                                             \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;       \
    int qi = 0;                                                       \
    for (int cidx = 0; cidx < (a).ncones; ++cidx) {                   \
        const SmallCone cd = (a).cones[cidx];
#define SM_CONES_END }

// nt_scaling + lambda = F v (src/ConicIP.jl:589-605, :165-194, :735; cones.hip: k_nt_scaling)
__device__ __forceinline__ void sm_nt_scaling(const SmallArgs &a, const double *v, const double *s, double *scal, double *lambda) {
    SM_CONES_BEGIN(a)
        if (cd.type == CIP_CONE_R) {
            for (int e = threadIdx.x; e < cd.dim; e += SMALL_T) {
                const double vi = v[cd.off + e], si = s[cd.off + e];
                const double d = sqrt(si / vi);                        // :598
                scal[cd.soff + e] = d;
                lambda[cd.off + e] = d * vi;
            }
        } else if ((qi++ & 3) == wave) {
            const double *z = v + cd.off, *sv = s + cd.off;
            const int k = cd.dim;
            double zz = 0, ss = 0, zs = 0;
            for (int e = 1 + lane; e < k; e += 64) { zz += z[e] * z[e]; ss += sv[e] * sv[e]; zs += z[e] * sv[e]; }
            zz = sm_wsum(zz); ss = sm_wsum(ss); zs = sm_wsum(zs);
            const double z0 = z[0], s0 = sv[0];
            const double qfz = z0 * z0 - zz, qfs = s0 * s0 - ss;
            const double beta = sqrt(sqrt(qfs / qfz));
            const double rz = 1.0 / sqrt(qfz), rs = 1.0 / sqrt(qfs);
            const double zdots = (z0 * s0 + zs) * rz * rs;
            const double gamma = sqrt((1.0 + zdots) * 0.5);
            const double h = 1.0 / (2.0 * gamma);
            const double wb0 = h * (s0 * rs + z0 * rz);
            const double c = sqrt(beta / (wb0 + 1.0));
            const double wdotz = c * (h * ((z0 * s0 + zs) * rs + qfz * rz) + z0);
            if (lane == 0) {
                scal[cd.soff] = beta;
                const double w0 = c * (wb0 + 1.0);
                scal[cd.soff + 1] = w0;
                lambda[cd.off] = -beta * z0 + w0 * wdotz;
            }
            for (int e = 1 + lane; e < k; e += 64) {
                const double we = c * h * (sv[e] * rs - z[e] * rz);
                scal[cd.soff + 1 + e] = we;
                lambda[cd.off + e] = beta * z[e] + we * wdotz;
            }
        }
    SM_CONES_END
    __syncthreads();
}
// F = I and the cone identity e (src/ConicIP.jl:704, :559-565; cones.hip: k_identity_scaling, k_cone_identity)
__device__ __forceinline__ void sm_identity(const SmallArgs &a, double *scal, double *ev) {
    SM_CONES_BEGIN(a)
        if (cd.type == CIP_CONE_R) {
            for (int e = threadIdx.x; e < cd.dim; e += SMALL_T) { scal[cd.soff + e] = 1.0; ev[cd.off + e] = 1.0; }
        } else if ((qi++ & 3) == wave) {
            if (lane == 0) { scal[cd.soff] = 1.0; scal[cd.soff + 1] = sqrt(2.0); ev[cd.off] = 1.0; }
            for (int e = 1 + lane; e < cd.dim; e += 64) { scal[cd.soff + 1 + e] = 0.0; ev[cd.off + e] = 0.0; }
        }
    SM_CONES_END
    __syncthreads();
}
// out = F x or F^-1 x (F is symmetric for R and Q cones: F' and F^-T are the same calls; cones.hip: k_apply).  out may be x.
__device__ __forceinline__ void sm_apply(const SmallArgs &a, const double *scal, bool inv, const double *x, double *out) {
    SM_CONES_BEGIN(a)
        if (cd.type == CIP_CONE_R) {
            for (int e = threadIdx.x; e < cd.dim; e += SMALL_T) {
                const double d = scal[cd.soff + e];
                out[cd.off + e] = inv ? x[cd.off + e] / d : x[cd.off + e] * d;
            }
        } else if ((qi++ & 3) == wave) {
            const int k = cd.dim;
            const double beta = scal[cd.soff];
            const double *w = scal + cd.soff + 1, *xb = x + cd.off;
            double *ob = out + cd.off;
            double wx = 0;
            for (int e = 1 + lane; e < k; e += 64) wx += w[e] * xb[e];
            const double w0 = w[0], x0 = xb[0];
            wx = sm_wsum(wx);
            if (!inv) {
                const double t = w0 * x0 + wx;                         // F x = -beta J x + w (w.x)
                if (lane == 0) ob[0] = -beta * x0 + w0 * t;
                for (int e = 1 + lane; e < k; e += 64) ob[e] = beta * xb[e] + w[e] * t;
            } else {
                const double t = (w0 * x0 - wx) / beta, ib = 1.0 / beta;   // F^-1 x = ((Jw)(Jw.x) / beta - J x) / beta
                if (lane == 0) ob[0] = (w0 * t - x0) * ib;
                for (int e = 1 + lane; e < k; e += 64) ob[e] = (xb[e] - w[e] * t) * ib;
            }
        }
    SM_CONES_END
    __syncthreads();
}
// out = alpha * (x o y) + (add ? add : 0)   (xrp!, xsoc!: src/ConicIP.jl:311-315, :340-345; cones.hip: k_cone_prod).  out differs from x, y.
__device__ __forceinline__ void sm_prod(const SmallArgs &a, const double *x, const double *y, const double *add, double *out) {
    SM_CONES_BEGIN(a)
        if (cd.type == CIP_CONE_R) {
            for (int e = threadIdx.x; e < cd.dim; e += SMALL_T) {
                const double v = x[cd.off + e] * y[cd.off + e];
                out[cd.off + e] = add ? add[cd.off + e] + v : v;
            }
        } else if ((qi++ & 3) == wave) {
            const int k = cd.dim;
            const double *xb = x + cd.off, *yb = y + cd.off;
            double *ob = out + cd.off;
            double xy = 0;
            for (int e = 1 + lane; e < k; e += 64) xy += xb[e] * yb[e];
            xy = sm_wsum(xy);
            const double x0 = xb[0], y0 = yb[0];
            if (lane == 0) { const double v = x0 * y0 + xy; ob[0] = add ? add[cd.off] + v : v; }
            for (int e = 1 + lane; e < k; e += 64) { const double v = x0 * yb[e] + y0 * xb[e]; ob[e] = add ? add[cd.off + e] + v : v; }
        }
    SM_CONES_END
    __syncthreads();
}
// out = x (./) y: solves y o out = x   (drp!, dsoc!: src/ConicIP.jl:305-309, :317-338; cones.hip: k_cone_div).  out differs from x, y.
__device__ __forceinline__ void sm_div(const SmallArgs &a, const double *x, const double *y, double *out) {
    SM_CONES_BEGIN(a)
        if (cd.type == CIP_CONE_R) {
            for (int e = threadIdx.x; e < cd.dim; e += SMALL_T) out[cd.off + e] = x[cd.off + e] / y[cd.off + e];
        } else if ((qi++ & 3) == wave) {
            const int k = cd.dim;
            const double *xb = x + cd.off, *yb = y + cd.off;
            double *ob = out + cd.off;
            double yy = 0, yx = 0;
            for (int e = 1 + lane; e < k; e += 64) { yy += yb[e] * yb[e]; yx += yb[e] * xb[e]; }
            yy = sm_wsum(yy); yx = sm_wsum(yx);
            const double y1 = yb[0], x1 = xb[0];
            const double alpha = y1 * y1 - yy;
            const double b1 = (-x1 / alpha) + yx / (y1 * alpha), b2 = 1.0 / y1;
            if (lane == 0) ob[0] = (y1 * x1 - yx) / alpha;
            for (int e = 1 + lane; e < k; e += 64) ob[e] = yb[e] * b1 + xb[e] * b2;
        }
    SM_CONES_END
    __syncthreads();
}
// maxstep(x, scale * d), or with d == NULL the `nothing` variant (src/ConicIP.jl:571-587, :212-270; cones.hip: k_maxstep).  The R
// cones share one minimum: x / d is a minimum over elements either way, and t -> (t > 0 ? 0 : t - 1) of the `nothing` variant is
// monotone, so the minimum over the cones of the cones' values is the value of the minimum.
__device__ __forceinline__ double sm_maxstep(const SmallArgs &a, const double *x, const double *d, double scale, double *red) {
    const double INF = __builtin_inf();
    double mn = INF, qmn = INF;
    int nan_seen = 0, any_r = 0;
    SM_CONES_BEGIN(a)
        if (cd.type == CIP_CONE_R) {
            any_r = 1;
            for (int e = threadIdx.x; e < cd.dim; e += SMALL_T) {
                if (d) {
                    const double de = d[cd.off + e] * scale;
                    if (de > 0) { const double q = x[cd.off + e] / de; if (q != q) nan_seen = 1; else mn = fmin(mn, q); }
                } else {
                    const double xe = x[cd.off + e];
                    if (xe != xe) nan_seen = 1; else mn = fmin(mn, xe);
                }
            }
        } else if ((qi++ & 3) == wave) {
            const int k = cd.dim;
            const double *xb = x + cd.off;
            double val;
            if (!d) {                                                  // maxstep_soc(x, nothing) :264-270
                double xx = 0;
                for (int e = 1 + lane; e < k; e += 64) xx += xb[e] * xb[e];
                xx = sm_wsum(xx);
                const double al = sqrt(xx) - xb[0];
                val = (al < 0) ? 0.0 : -1.0 - al;
            } else {                                                   // maxstep_soc(x, d) :242-262
                const double *db = d + cd.off;
                double xx = 0, xd = 0;
                for (int e = 1 + lane; e < k; e += 64) { xx += xb[e] * xb[e]; xd += xb[e] * (-scale * db[e]); }
                xx = sm_wsum(xx); xd = sm_wsum(xd);
                const double x0 = xb[0], d0 = -scale * db[0];
                const double gam = x0 * x0 - xx, rg = 1.0 / sqrt(gam);
                const double bet = (x0 * d0 - xd) * rg, rho1 = bet * rg;
                const double mu = (bet + d0) / (x0 * rg + 1.0);
                double r2 = 0;
                for (int e = 1 + lane; e < k; e += 64) { const double t = (-scale * db[e]) - mu * xb[e] * rg; r2 += t * t; }
                r2 = sm_wsum(r2);
                const double al = sqrt(r2) * rg - rho1;
                val = (al < 0) ? INF : 1.0 / al;
            }
            if (val != val) nan_seen = 1; else qmn = fmin(qmn, val);
        }
    SM_CONES_END
    mn = sm_bmin(mn, nan_seen, red);
    if (!d && any_r && mn == mn) mn = (mn > 0.0) ? 0.0 : -1.0 + mn;
    if (!d && !any_r) mn = INF;
    const double q = sm_bmin(qmn, 0, red);
    return mn != mn ? mn : fmin(mn, q);
}
// W[i, off + e] = (F^-T a_i)_e for every row i of A' (cones.hip: k_scale_At, k_scale_At_r): R entries over all threads; a Q cone's rows
// one thread each, the cones dealt to the 256 / n thread segments in turn
__device__ __forceinline__ void sm_scale_At(const SmallArgs &a, const double *scal, const double *At, double *W) {
    const int n = a.n, nseg = SMALL_T / n, seg = threadIdx.x / n, row = threadIdx.x - seg * n;
    SM_CONES_BEGIN(a)
        (void)lane; (void)wave;
        if (cd.type == CIP_CONE_R) {
            for (int e = threadIdx.x; e < cd.dim * n; e += SMALL_T) {
                const int col = cd.off + e / n;
                W[(long)cd.off * n + e] = At[(long)cd.off * n + e] / scal[cd.soff + (col - cd.off)];
            }
        } else if ((qi++ % nseg) == seg) {
            const int k = cd.dim;
            const double beta = scal[cd.soff], ib = 1.0 / beta;
            const double *w = scal + cd.soff + 1;
            const double *ap = At + row + (long)cd.off * n;
            double *wp = W + row + (long)cd.off * n;
            double t = w[0] * ap[0];
            for (int e = 1; e < k; ++e) t -= w[e] * ap[(long)e * n];
            t /= beta;
            wp[0] = (w[0] * t - ap[0]) * ib;
            for (int e = 1; e < k; ++e) wp[(long)e * n] = (ap[(long)e * n] - w[e] * t) * ib;
        }
    SM_CONES_END
    __syncthreads();
}

// ---------------------------------------------------------------- the KKT matrix in LDS
// K = [Q + W W'  .; G  0] (lower triangle; W = A' F^-1, n x m).  The product runs on v_mfma_f64_16x16x4_f64 over the 16 x 16 tiles of
// the lower triangle, dealt to the four waves in turn, 16 columns of W at a time through a zero-padded LDS panel (edge tiles are
// padded here, not in HBM); a tile's sum runs over the panels in ascending order.  Rows / columns n .. of an edge tile only ever
// receive + 0.
__device__ __forceinline__ void sm_form_K(const SmallArgs &a, const double *Q, const double *G, const double *W, double *K, double *pan) {
    const int n = a.n, m = a.m, p = a.p, ldk = a.ldk, pld = a.pld, tid = threadIdx.x;
    for (int e = tid; e < ldk * a.kcols; e += SMALL_T) K[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < n * n; e += SMALL_T) { const int j = e / n, i = e - j * n; if (i >= j) K[i + j * ldk] = Q[e]; }
    for (int e = tid; e < p * n; e += SMALL_T) { const int j = e / p, r = e - j * p; K[n + r + j * ldk] = G[e]; }
    __syncthreads();
    if (m == 0) return;
    const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int nt = (n + 15) / 16, ntiles = nt * (nt + 1) / 2, np16 = nt * 16;
    for (int k0 = 0; k0 < m; k0 += 16) {
        for (int e = tid; e < 16 * np16; e += SMALL_T) {
            const int kk = e / np16, r = e - kk * np16;
            pan[r + kk * pld] = (r < n && k0 + kk < m) ? W[r + (long)(k0 + kk) * n] : 0.0;
        }
        __syncthreads();
        for (int t = wave; t < ntiles; t += 4) {
            int bj = 0, tt = t;
            while (tt >= nt - bj) { tt -= nt - bj; ++bj; }
            const int i0 = 16 * (bj + tt), j0 = 16 * bj;
            // lane (l15, g), register q: C[i0 + l15][j0 + g + 4 q] (sdp.hip: sd_gemm)
            double *cp = K + (i0 + l15) + (j0 + g) * ldk;
            v4d acc = {cp[0], cp[4 * ldk], cp[8 * ldk], cp[12 * ldk]};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double fj = pan[j0 + l15 + (4 * s + g) * pld], fi = pan[i0 + l15 + (4 * s + g) * pld];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fj, fi, acc, 0, 0, 0);
            }
            cp[0] = acc[0]; cp[4 * ldk] = acc[1]; cp[8 * ldk] = acc[2]; cp[12 * ldk] = acc[3];
        }
        __syncthreads();
    }
}
// Unpivoted right-looking LDL' of the order-N lower triangle in LDS: L below the diagonal, D on it.  Returns the 1-based column of the
// first bad pivot -- zero, non-finite, or of the wrong sign: positive on the first n, negative on the last p (diag.hip:247-253) --
// or 0; the same value in every thread.
__device__ __forceinline__ int sm_ldlt(double *K, int ldk, int N, int n, double *cw) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    for (int j = 0; j < N; ++j) {
        const double d = K[j + j * ldk];
        const bool dead = !(fabs(d) > 0.0 && fabs(d) < 1.7e308);
        if (dead || ((d > 0.0) != (j < n))) return j + 1;
        const int i = j + 1 + tid;
        if (i < N) { const double w = K[i + j * ldk]; cw[i] = w; K[i + j * ldk] = w / d; }
        __syncthreads();
        for (int k = j + 1 + ty; k < N; k += 16) {
            const double ck = cw[k];
            for (int r = k + tx; r < N; r += 16) K[r + k * ldk] -= K[r + j * ldk] * ck;
        }
        __syncthreads();
    }
    return 0;
}
// the two triangular sweeps in LDS: x <- (L D L')^-1 x, every entry's sum in column order
__device__ __forceinline__ void sm_ldlt_solve(const double *K, int ldk, int N, double *x) {
    const int tid = threadIdx.x;
    for (int j = 0; j < N - 1; ++j) {
        const double xj = x[j];
        const int i = j + 1 + tid;
        if (i < N) x[i] -= K[i + j * ldk] * xj;
        __syncthreads();
    }
    if (tid < N) x[tid] /= K[tid + tid * ldk];
    __syncthreads();
    for (int j = N - 1; j > 0; --j) {
        const double xj = x[j];
        if (tid < j) x[tid] -= K[j + tid * ldk] * xj;
        __syncthreads();
    }
}

struct SmallLds { double *K, *pan, *rhs, *cw, *red, *part; };

// solve4x4 (src/ConicIP.jl:684-692) on the factor in LDS, with solve3x3 in the algebra of pivotgen (src/kktsolvers.jl:324-330;
// solve.hip: solve3x3_once, cip_solve4x4_dev):
//   q = r.s (./) lambda ; t1 = F'q ; z3 = r.v + t1 ; t = (F'F)^-1 z3 ; [S G'; G 0][dy; dw] = [r.y + A't; r.w] ;
//   dv = t - (F'F)^-1 A dy ; ds = t1 - F'(F dv)
__device__ __forceinline__ void sm_solve4x4(const SmallArgs &a, const SmallSlab &S, const SmallLds &L, const double *lam, const double *r,
                                            double *dz) {
    const int n = a.n, m = a.m, p = a.p, N = n + p, tid = threadIdx.x;
    const double *ry = r, *rw = r + n, *rv = r + n + p, *rs = r + n + p + m;
    double *dy = dz, *dw = dz + n, *dv = dz + n + p, *ds = dz + n + p + m;
    if (m > 0) {
        sm_div(a, rs, lam, S.q);
        sm_apply(a, S.scal, false, S.q, S.t1);
        for (int e = tid; e < m; e += SMALL_T) S.tmp[e] = rv[e] + S.t1[e];
        __syncthreads();
        sm_apply(a, S.scal, true, S.tmp, S.tmp);
        sm_apply(a, S.scal, true, S.tmp, S.t);
        sm_gemv(n, m, S.At, n, S.t, 1.0, 0.0, S.x3, L.part);
    }
    if (tid < N) L.rhs[tid] = tid < n ? (m > 0 ? ry[tid] + S.x3[tid] : ry[tid]) : rw[tid - n];
    __syncthreads();
    sm_ldlt_solve(L.K, a.ldk, N, L.rhs);
    if (tid < N) { if (tid < n) dy[tid] = L.rhs[tid]; else dw[tid - n] = L.rhs[tid]; }
    __syncthreads();
    if (m > 0) {
        sm_gemv(m, n, S.A, m, dy, 1.0, 0.0, S.u, L.part);
        sm_apply(a, S.scal, true, S.u, S.u);
        sm_apply(a, S.scal, true, S.u, S.u);
        for (int e = tid; e < m; e += SMALL_T) dv[e] = S.t[e] - S.u[e];
        __syncthreads();
        sm_apply(a, S.scal, false, dv, S.u);
        sm_apply(a, S.scal, false, S.u, S.u);
        for (int e = tid; e < m; e += SMALL_T) ds[e] = S.t1[e] - S.u[e];
        __syncthreads();
    }
}

__device__ __forceinline__ SmallSlab sm_shift(const SmallSlab &S, long o) {
    SmallSlab T;
    T.c = S.c + o; T.b = S.b + o; T.d = S.d + o; T.Q = S.Q + o; T.A = S.A + o; T.G = S.G + o; T.At = S.At + o; T.Gt = S.Gt + o; T.W = S.W + o;
    T.z = S.z + o; T.r0 = S.r0 + o; T.r = S.r + o; T.daff = S.daff + o; T.dz = S.dz + o; T.dzr = S.dzr + o; T.rIr = S.rIr + o;
    T.lam = S.lam + o; T.scal = S.scal + o; T.e = S.e + o; T.Qy = S.Qy + o; T.pinf = S.pinf + o; T.Ays = S.Ays + o; T.Gy = S.Gy + o;
    T.q = S.q + o; T.t = S.t + o; T.t1 = S.t1 + o; T.u = S.u + o; T.tmp = S.tmp + o; T.mb1 = S.mb1 + o; T.mb2 = S.mb2 + o; T.x3 = S.x3 + o;
    return T;
}

// ---------------------------------------------------------------- the kernels
// Copies a device-pointer problem's matrices into its slab (src != NULL), then forms A' and G'.  One workgroup per problem.
__global__ __launch_bounds__(SMALL_T) void k_small_prepare(SmallArgs a, const SmallSrc *src) {
    const int z = blockIdx.x, n = a.n, m = a.m, p = a.p, tid = threadIdx.x;
    const SmallSlab S = sm_shift(a.S, (long)z * a.stride8);
    if (src) {
        const SmallSrc sc = src[z];
        for (int e = tid; e < n * n; e += SMALL_T) { const int j = e / n, i = e - j * n; S.Q[e] = sc.Q[i + (long)j * sc.ldq]; }
        for (int e = tid; e < m * n; e += SMALL_T) { const int j = e / m, i = e - j * m; S.A[e] = sc.A[i + (long)j * sc.lda]; }
        for (int e = tid; e < p * n; e += SMALL_T) { const int j = e / p, i = e - j * p; S.G[e] = sc.G[i + (long)j * sc.ldg]; }
        __syncthreads();
    }
    for (int e = tid; e < m * n; e += SMALL_T) { const int j = e / n, i = e - j * n; S.At[e] = S.A[j + (long)i * m]; }     // At[i + j n] = A[j, i]
    for (int e = tid; e < p * n; e += SMALL_T) { const int j = e / n, i = e - j * n; S.Gt[e] = S.G[j + (long)i * p]; }
}

// src/ConicIP.jl:732-735, :746-753 and the 16 dot products of IterDots, in that order (driver.hip: Loop::run)
__global__ __launch_bounds__(SMALL_T) void k_small_residuals(SmallArgs a) {
    __shared__ double red[16], part[256];
    const int z = a.live ? a.live[blockIdx.x] : (int)blockIdx.x, n = a.n, m = a.m, p = a.p, tid = threadIdx.x;
    const SmallSlab S = sm_shift(a.S, (long)z * a.stride8);
    double *y = S.z, *w = S.z + n, *v = S.z + n + p, *s = S.z + n + p + m;
    double *r0y = S.r0, *r0w = S.r0 + n, *r0v = S.r0 + n + p, *r0s = S.r0 + n + p + m;
    if (m > 0) {
        sm_nt_scaling(a, v, s, S.scal, S.lam);                         // :732-735
        sm_prod(a, S.lam, S.lam, nullptr, r0s);                        // :746
    }
    sm_gemv(n, n, S.Q, n, y, 1.0, 0.0, S.Qy, part);
    for (int e = tid; e < n; e += SMALL_T) S.pinf[e] = 0.0;            // pinf = G'w - A'v (:810)
    __syncthreads();
    if (p > 0) {
        sm_gemv(n, p, S.Gt, n, w, 1.0, 0.0, S.pinf, part);
        sm_gemv(p, n, S.G, p, y, 1.0, 0.0, S.Gy, part);
    }
    if (m > 0) {
        sm_gemv(n, m, S.At, n, v, -1.0, 1.0, S.pinf, part);
        sm_gemv(m, n, S.A, m, y, 1.0, 0.0, S.Ays, part);
    }
    for (int e = tid; e < n; e += SMALL_T) r0y[e] = (S.Qy[e] + S.pinf[e]) - S.c[e];     // :747, :753
    for (int e = tid; e < p; e += SMALL_T) r0w[e] = S.Gy[e] - S.d[e];
    for (int e = tid; e < m; e += SMALL_T) { const double t = S.Ays[e] - s[e]; S.Ays[e] = t; r0v[e] = t - S.b[e]; }
    __syncthreads();
    double d0, d1, d2, d3, o[16];
#define DOT(x, y, len, acc) for (int e = tid; e < (len); e += SMALL_T) acc += (x)[e] * (y)[e]
    d0 = d1 = d2 = d3 = 0; DOT(v, s, m, d0); DOT(S.c, y, n, d1); DOT(r0y, r0y, n, d2); DOT(r0v, r0v, m, d3);
    sm_bsum4(d0, d1, d2, d3, red); o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3;
    d0 = d1 = d2 = d3 = 0; DOT(r0s, r0s, m, d0); DOT(y, S.Qy, n, d1); DOT(w, r0w, p, d2); DOT(v, r0v, m, d3);
    sm_bsum4(d0, d1, d2, d3, red); o[4] = d0; o[5] = d1; o[6] = d2; o[7] = d3;
    d0 = d1 = d2 = d3 = 0; DOT(S.d, w, p, d0); DOT(S.b, v, m, d1); DOT(S.pinf, S.pinf, n, d2); DOT(y, y, n, d3);
    sm_bsum4(d0, d1, d2, d3, red); o[8] = d0; o[9] = d1; o[10] = d2; o[11] = d3;
    d0 = d1 = d2 = d3 = 0; DOT(v, v, m, d0); DOT(S.Ays, S.Ays, m, d1); DOT(S.Gy, S.Gy, p, d2); DOT(S.Qy, S.Qy, n, d3);
    sm_bsum4(d0, d1, d2, d3, red); o[12] = d0; o[13] = d1; o[14] = d2; o[15] = d3;
#undef DOT
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) a.dots[(long)z * 16 + i] = o[i];
    }
}

// init != 0: the initial point (src/ConicIP.jl:704-713).  Otherwise one iteration behind its verdict: factorisation (:737), predictor
// (:879-887), corrector (:893-901), Newton step + refinement (:907-921), step (:927-932).  The scalar formulas are Loop::run's.
__global__ __launch_bounds__(SMALL_T) void k_small_step(SmallArgs a) {
    extern __shared__ double lds[];
    SmallLds L;
    L.K = lds; L.pan = L.K + (long)a.ldk * a.kcols; L.rhs = L.pan + a.pld * 16; L.cw = L.rhs + 128; L.red = L.cw + 128; L.part = L.red + 16;
    const int z = a.live ? a.live[blockIdx.x] : (int)blockIdx.x, n = a.n, m = a.m, p = a.p, N = n + p, NT = n + p + 2 * m, tid = threadIdx.x;
    const SmallSlab S = sm_shift(a.S, (long)z * a.stride8);
    double *v = S.z + n + p, *s = S.z + n + p + m;
    if (a.init) {
        if (m > 0) sm_identity(a, S.scal, S.e);
    } else if (m > 0) sm_scale_At(a, S.scal, S.At, S.W);               // (scaling and lambda: k_small_residuals left them in the slab)
    sm_form_K(a, S.Q, S.G, a.init ? S.At : S.W, L.K, L.pan);
    const int bad = sm_ldlt(L.K, a.ldk, N, n, L.cw);
    if (bad) { if (tid == 0) a.flags[z] = bad; return; }
    if (a.init) {
        for (int e = tid; e < NT; e += SMALL_T) S.r0[e] = e < n ? S.c[e] : (e < N ? S.d[e - n] : (e < N + m ? S.b[e - N] : 0.0));
        __syncthreads();
        sm_solve4x4(a, S, L, S.e, S.r0, S.z);
        if (m > 0) {
            const double av = sm_maxstep(a, v, nullptr, 1.0, L.red), as = sm_maxstep(a, s, nullptr, 1.0, L.red);
            for (int e = tid; e < m; e += SMALL_T) { v[e] = -av * S.e[e] + v[e]; s[e] = -as * S.e[e] + s[e]; }
        }
        return;
    }
    const double mubar = a.dots[(long)z * 16], mu = mubar / a.conedim;
    // ---- predictor
    sm_solve4x4(a, S, L, S.lam, S.r0, S.daff);
    double sigma = 0.0;
    double *dfv = S.daff + n + p, *dfs = S.daff + n + p + m;
    if (m > 0) {
        const double a1 = sm_maxstep(a, v, dfv, 1.0, L.red), a2 = sm_maxstep(a, s, dfs, 1.0, L.red);
        const double a_aff = fmin(fmin(a1, 1.0), a2);
        double q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        for (int e = tid; e < m; e += SMALL_T) { q0 += v[e] * s[e]; q1 += v[e] * dfs[e]; q2 += dfv[e] * s[e]; q3 += dfv[e] * dfs[e]; }
        sm_bsum4(q0, q1, q2, q3, L.red);
        const double rho = (q0 - a_aff * q1 - a_aff * q2 + a_aff * a_aff * q3) / mubar;       // fts :162-163, :886
        const double cl = fmax(0.0, fmin(1.0, rho));
        sigma = cl * cl * cl;
        // ---- corrector: r = r0 ; r.s += (F^-T d_aff.s) o (F d_aff.v) - sigma mu e
        sm_apply(a, S.scal, true, dfs, S.mb1);
        sm_apply(a, S.scal, false, dfv, S.mb2);
        sm_prod(a, S.mb1, S.mb2, S.r0 + N + m, S.r + N + m);
        const double sm = sigma * mu;
        for (int e = tid; e < N + m; e += SMALL_T) S.r[e] = S.r0[e];
        for (int e = tid; e < m; e += SMALL_T) S.r[N + m + e] -= sm * S.e[e];
    } else {
        for (int e = tid; e < NT; e += SMALL_T) S.r[e] = S.r0[e];
    }
    __syncthreads();
    // ---- Newton step + refinement
    sm_solve4x4(a, S, L, S.lam, S.r, S.dz);
    double *dy = S.dz, *dw = S.dz + n, *dv = S.dz + N, *ds = S.dz + N + m;
    double *ky = S.rIr, *kw = S.rIr + n, *kv = S.rIr + N, *ks = S.rIr + N + m;
    int nref = 0;
    for (int it = 0; it < a.maxRef; ++it) {
        // rIr = r - K4 dz:  K4 dz = (Q dy + G'dw - A'dv, G dy, A dy - ds, lam o (F dv) + lam o (F^-T ds))
        sm_gemv(n, n, S.Q, n, dy, 1.0, 0.0, ky, L.part);
        if (p > 0) { sm_gemv(n, p, S.Gt, n, dw, 1.0, 1.0, ky, L.part); sm_gemv(p, n, S.G, p, dy, 1.0, 0.0, kw, L.part); }
        if (m > 0) {
            sm_gemv(n, m, S.At, n, dv, -1.0, 1.0, ky, L.part);
            sm_gemv(m, n, S.A, m, dy, 1.0, 0.0, kv, L.part);
            sm_apply(a, S.scal, false, dv, S.mb1);
            sm_prod(a, S.lam, S.mb1, nullptr, S.mb2);
            sm_apply(a, S.scal, true, ds, S.mb1);
            sm_prod(a, S.lam, S.mb1, S.mb2, ks);
        }
        for (int e = tid; e < N; e += SMALL_T) S.rIr[e] = S.r[e] - S.rIr[e];
        for (int e = tid; e < m; e += SMALL_T) { kv[e] = S.r[N + e] - (kv[e] - ds[e]); ks[e] = S.r[N + m + e] - ks[e]; }
        __syncthreads();
        double n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        for (int e = tid; e < n; e += SMALL_T) n0 += ky[e] * ky[e];
        for (int e = tid; e < p; e += SMALL_T) n1 += kw[e] * kw[e];
        for (int e = tid; e < m; e += SMALL_T) { n2 += kv[e] * kv[e]; n3 += ks[e] * ks[e]; }
        sm_bsum4(n0, n1, n2, n3, L.red);
        const double rnorm = (sqrt(n0) + (p > 0 ? sqrt(n1) : 0.0) + (m > 0 ? sqrt(n2) + sqrt(n3) : 0.0)) / (n + 2 * m);   // :917 (norm(v4x1) :61)
        if (rnorm < a.refThr) break;
        sm_solve4x4(a, S, L, S.lam, S.rIr, S.dzr);
        ++nref;
        for (int e = tid; e < NT; e += SMALL_T) S.dz[e] += S.dzr[e];                     // :920
        __syncthreads();
    }
    // ---- step
    double alpha = 1.0;
    if (m > 0) {
        const double sc = 1.0 / (1.0 - a.DTB);
        const double a1 = sm_maxstep(a, v, dv, sc, L.red), a2 = sm_maxstep(a, s, ds, sc, L.red);
        alpha = fmin(fmin(a1, 1.0), fmin(a2, 1.0));
    }
    for (int e = tid; e < NT; e += SMALL_T) S.z[e] = -alpha * S.dz[e] + S.z[e];
    if (tid == 0) a.nref[z] = nref;
}

// ---------------------------------------------------------------- host
thread_local int g_small_stats[4] = {0, 0, 0, 0};
thread_local int g_small_timing = 0;
thread_local double g_small_time[2] = {0.0, 0.0};

// what cip_conicip_small takes (include/cipkkt.h); the message names the rule
int small_check(const cip_problem *q, const char *who) {
    if (!q) { cip_set_error("%s: null problem", who); return CIP_E_INVALID; }
    if (q->n < 1 || q->m < 0 || q->p < 0 || q->ncones < 0 || (q->ncones > 0 && (!q->cone_type || !q->cone_dim))) {
        cip_set_error("%s: bad dimensions or cone list", who); return CIP_E_INVALID;
    }
    long sum = 0;
    bool has_s = false;
    for (int c = 0; c < q->ncones; ++c) {
        if (q->cone_dim[c] < 1 || q->cone_type[c] < CIP_CONE_R || q->cone_type[c] > CIP_CONE_S) { cip_set_error("%s: bad cone %d", who, c); return CIP_E_INVALID; }
        has_s |= q->cone_type[c] == CIP_CONE_S;
        sum += q->cone_dim[c];
    }
    if (sum != q->m) { cip_set_error("%s: the cones cover %ld rows, A has %d", who, sum, q->m); return CIP_E_INVALID; }
    if (q->route != CIP_ROUTE_SCHUR) { cip_set_error("%s: the Schur route only", who); return CIP_E_UNSUPPORTED; }
    if (q->flags & CIP_FLAG_Q_CSR) { cip_set_error("%s: a CSR Q (CIP_FLAG_Q_CSR) is not taken", who); return CIP_E_UNSUPPORTED; }
    if (q->m > 0 && !q->A && q->A_rowptr) { cip_set_error("%s: a CSR A is not taken", who); return CIP_E_UNSUPPORTED; }
    if (has_s) { cip_set_error("%s: S cones are not taken", who); return CIP_E_UNSUPPORTED; }
    if (q->n + q->p > CIP_SMALL_MAX_N) { cip_set_error("%s: n + p = %d exceeds CIP_SMALL_MAX_N = %d", who, q->n + q->p, CIP_SMALL_MAX_N); return CIP_E_UNSUPPORTED; }
    if (q->m > CIP_SMALL_MAX_M) { cip_set_error("%s: m = %d exceeds CIP_SMALL_MAX_M = %d", who, q->m, CIP_SMALL_MAX_M); return CIP_E_UNSUPPORTED; }
    if (!q->Q) { cip_set_error("%s: Q is NULL", who); return CIP_E_INVALID; }
    if (q->m > 0 && !q->A) { cip_set_error("%s: A is NULL", who); return CIP_E_INVALID; }
    if (q->p > 0 && !q->G) { cip_set_error("%s: G is NULL", who); return CIP_E_INVALID; }
    if ((q->ldq > 0 && q->ldq < q->n) || (q->lda > 0 && q->lda < q->m) || (q->ldg > 0 && q->ldg < q->p)) {
        cip_set_error("%s: a leading dimension is smaller than its row count", who); return CIP_E_INVALID;
    }
    return CIP_OK;
}

// everything the call owns, freed on every path
struct SmallCall {
    hipStream_t stream = nullptr;
    char *arena = nullptr;
    void *back_host = nullptr, *live_host = nullptr, *stage = nullptr, *iter_host = nullptr;
    std::vector<hipEvent_t> ev;
    ~SmallCall() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (back_host) (void)hipHostFree(back_host);
        if (live_host) (void)hipHostFree(live_host);
        if (iter_host) (void)hipHostFree(iter_host);
        free(stage);
        if (arena) (void)hipFree(arena);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int small_run(int count, const cip_problem *probs, const double *const *c, const double *const *b, const double *const *d, const cip_options &o,
              double *const *y, double *const *w, double *const *v, cip_result *res, std::vector<int> &fallback) {
    using namespace cipdrv;
    const cip_problem &q0 = probs[0];
    const int n = q0.n, m = q0.m, p = q0.p, N = n + p, ncones = q0.ncones;
    const bool dev = (q0.flags & CIP_FLAG_DEVICE_PTRS) != 0;
    int *stats = g_small_stats;
    // ---- the cone table and the packed-scaling offsets
    std::vector<SmallCone> cones(ncones);
    size_t scal_len = 0;
    double conedim = 0;
    for (int k = 0, off = 0; k < ncones; ++k) {
        cones[k] = SmallCone{q0.cone_type[k], off, q0.cone_dim[k], (int)scal_len};
        scal_len += q0.cone_type[k] == CIP_CONE_R ? q0.cone_dim[k] : 1 + q0.cone_dim[k];
        conedim += q0.cone_type[k] == CIP_CONE_R ? q0.cone_dim[k] : 1;               // (:547-552)
        off += q0.cone_dim[k];
    }
    // ---- one arena: a slab per problem, then what the host reads back, the live list, the cone table, the source table
    SmallArgs a = {};
    size_t host_prefix = 0, dev_prefix = 0;
    const size_t slab = small_layout(nullptr, n, m, p, scal_len, &a.S, &host_prefix, &dev_prefix);
    const size_t stride = slab_stride(slab), prefix = dev ? dev_prefix : host_prefix;
    struct Arena { char *slabs; double *dots; int *flags, *nref, *live; SmallCone *cones; SmallSrc *src; };
    auto arena_layout = [&](const void *base, Arena *A) {
        CipLayout L(base);
        A->slabs = L.take<char>(stride * (size_t)count);
        A->dots = L.take<double>((size_t)count * 16); A->flags = L.take<int>(count, 8); A->nref = L.take<int>(count, 8);     // one read-back
        A->live = L.take<int>(count); A->cones = L.take<SmallCone>(ncones); A->src = L.take<SmallSrc>(dev ? count : 0);
        return L.bytes();
    };
    Arena A;
    const size_t arena_bytes = arena_layout(nullptr, &A);
    const size_t ints = ((size_t)count * sizeof(int) + 7) / 8 * 8;
    SmallCall C;
    CIP_HIP_CHECK(hipStreamCreateWithFlags(&C.stream, hipStreamNonBlocking));
    hipStream_t s = C.stream;
    CIP_HIP_CHECK(hipMalloc((void **)&C.arena, arena_bytes));
    arena_layout(C.arena, &A);
    small_layout(A.slabs, n, m, p, scal_len, &a.S, nullptr, nullptr);
    const size_t back_span = (size_t)((char *)A.nref - (char *)A.dots) + ints;       // dots, flags, nref: contiguous in the arena
    CIP_HIP_CHECK(hipHostMalloc(&C.back_host, back_span, hipHostMallocDefault));
    CIP_HIP_CHECK(hipHostMalloc(&C.live_host, sizeof(int) * (size_t)count, hipHostMallocDefault));
    const size_t iter_row = sizeof(double) * ((size_t)N + m);
    CIP_HIP_CHECK(hipHostMalloc(&C.iter_host, iter_row * (size_t)count, hipHostMallocDefault));
    double *dots_h = (double *)C.back_host;
    int *flags_h = (int *)((char *)C.back_host + ((char *)A.flags - (char *)A.dots)), *nref_h = (int *)((char *)C.back_host + ((char *)A.nref - (char *)A.dots));
    int *live_h = (int *)C.live_host;
    CIP_HIP_CHECK(hipMemsetAsync(A.dots, 0, back_span, s));
    CIP_HIP_CHECK(hipMemcpyAsync(A.cones, cones.data(), sizeof(SmallCone) * ncones, hipMemcpyHostToDevice, s));
    // ---- the upload: every problem's slab prefix (c, b, d and, for host-pointer problems, Q, A, G made compact) through a bounded
    // staging buffer, then one launch that gathers device-pointer matrices and forms A', G'
    std::vector<Norms> nm(count);
    {
        const size_t per = std::max<size_t>(1, std::min<size_t>((size_t)count, ((size_t)64 << 20) / std::max<size_t>(prefix, 1)));
        C.stage = calloc(per, prefix ? prefix : 1);
        if (!C.stage) { cip_set_error("cip_conicip_small: host staging allocation failed"); return CIP_E_HIP; }
        SmallSlab H;
        std::vector<SmallSrc> src(dev ? count : 0);
        for (int z0 = 0; z0 < count; z0 += (int)per) {
            const int cnt = std::min<int>((int)per, count - z0);
            for (int k = 0; k < cnt; ++k) {
                const int z = z0 + k;
                const cip_problem &q = probs[z];
                small_layout((char *)C.stage + (size_t)k * prefix, n, m, p, scal_len, &H, nullptr, nullptr);
                memcpy(H.c, c[z], sizeof(double) * n);
                if (m > 0) memcpy(H.b, b[z], sizeof(double) * m);
                if (p > 0) memcpy(H.d, d[z], sizeof(double) * p);
                nm[z] = host_norms(n, m, p, c[z], m > 0 ? b[z] : nullptr, p > 0 ? d[z] : nullptr);
                const int ldq = q.ldq > 0 ? q.ldq : n, lda = q.lda > 0 ? q.lda : m, ldg = q.ldg > 0 ? q.ldg : p;
                if (dev) { src[z] = SmallSrc{q.Q, q.A, q.G, ldq, lda, ldg}; continue; }
                for (int j = 0; j < n; ++j) {
                    memcpy(H.Q + (size_t)j * n, q.Q + (size_t)j * ldq, sizeof(double) * n);
                    if (m > 0) memcpy(H.A + (size_t)j * m, q.A + (size_t)j * lda, sizeof(double) * m);
                    if (p > 0) memcpy(H.G + (size_t)j * p, q.G + (size_t)j * ldg, sizeof(double) * p);
                }
            }
            CIP_HIP_CHECK(hipMemcpy2DAsync(A.slabs + stride * (size_t)z0, stride, C.stage, prefix, prefix, cnt, hipMemcpyHostToDevice, s));
            CIP_HIP_CHECK(hipStreamSynchronize(s));
        }
        if (dev) CIP_HIP_CHECK(hipMemcpyAsync(A.src, src.data(), sizeof(SmallSrc) * count, hipMemcpyHostToDevice, s));
        CIP_HIP_CHECK(hipStreamSynchronize(s));          // (src is a local)
    }
    a.stride8 = (long)(stride / sizeof(double));
    a.n = n; a.m = m; a.p = p; a.ncones = ncones;
    const int N16 = (N + 15) / 16 * 16, n16 = (n + 15) / 16 * 16;
    a.ldk = N16 + 1; a.kcols = N16; a.pld = n16 + 2;
    a.cones = A.cones; a.live = nullptr; a.dots = A.dots; a.flags = A.flags; a.nref = A.nref;
    a.conedim = conedim; a.DTB = o.DTB; a.refThr = o.refinementThreshold; a.maxRef = o.maxRefinementSteps; a.init = 1;
    const size_t lds = small_lds_bytes(a.ldk, a.kcols, a.pld);
    CIP_HIP_CHECK(hipFuncSetAttribute((const void *)k_small_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_small_prepare, dim3(count), dim3(SMALL_T), 0, s, a, dev ? (const SmallSrc *)A.src : (const SmallSrc *)nullptr);
    hipLaunchKernelGGL(k_small_step, dim3(count), dim3(SMALL_T), lds, s, a);        // initial point (:704-713)
    CIP_HIP_CHECK(hipGetLastError());
    stats[2] += 2;
    a.init = 0; a.live = A.live;

    std::vector<int> live(count), n_factor(count, 1), n_solve(count, 1);
    std::vector<IterOutcome> outcome(count);
    std::vector<double> optBest(count, INFINITY);
    std::vector<char> gone(count, 0);
    for (int z = 0; z < count; ++z) {
        live[z] = z; live_h[z] = z;
        res[z] = fresh_result();
    }
    CIP_HIP_CHECK(hipMemcpyAsync(A.live, live_h, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, s));
    auto read_back = [&]() -> int {
        CIP_HIP_CHECK(hipMemcpyAsync(C.back_host, A.dots, back_span, hipMemcpyDeviceToHost, s));
        CIP_HIP_CHECK(hipStreamSynchronize(s));
        stats[3] += 1;
        return 0;
    };
    const bool timing = g_small_timing != 0;
    int nlive = count, steps = 0;
    cip_options quiet = o;
    quiet.verbose = 0;                                         // (nothing is printed per problem)
    for (int Iter = 1; Iter <= o.maxIters && nlive > 0; ++Iter) {                      // :730
        hipLaunchKernelGGL(k_small_residuals, dim3(nlive), dim3(SMALL_T), 0, s, a);
        CIP_HIP_CHECK(hipGetLastError());
        stats[2] += 1;
        CIP_TRY(read_back());
        int k = 0;
        for (int j = 0; j < nlive; ++j) {
            const int z = live[j];
            if (flags_h[z]) { gone[z] = 1; fallback.push_back(z); continue; }       // bad pivot in the factorisation behind the last verdict
            if (Iter > 1) n_solve[z] += nref_h[z];
            n_factor[z] += 1;                                                        // :737 precedes :786
            IterDots dd;
            for (int i = 0; i < 16; ++i) dd.v[i] = dots_h[(size_t)z * 16 + i];
            outcome[z] = evaluate_iteration(dd, nm[z], conedim, m, p, quiet, Iter, &res[z], optBest[z], nullptr);
            if (outcome[z].status != CIP_STATUS_NONE) { gone[z] = 2; continue; }
            live[k++] = z;
        }
        nlive = k;
        if (nlive == 0) break;
        for (int j = 0; j < nlive; ++j) { live_h[j] = live[j]; n_solve[live[j]] += 2; }
        CIP_HIP_CHECK(hipMemcpyAsync(A.live, live_h, sizeof(int) * (size_t)nlive, hipMemcpyHostToDevice, s));
        if (timing) {
            hipEvent_t e0, e1;
            CIP_HIP_CHECK(hipEventCreate(&e0)); C.ev.push_back(e0);
            CIP_HIP_CHECK(hipEventCreate(&e1)); C.ev.push_back(e1);
            CIP_HIP_CHECK(hipEventRecord(e0, s));
        }
        hipLaunchKernelGGL(k_small_step, dim3(nlive), dim3(SMALL_T), lds, s, a);
        CIP_HIP_CHECK(hipGetLastError());
        if (timing) CIP_HIP_CHECK(hipEventRecord(C.ev.back(), s));
        stats[2] += 1;
        ++steps;
    }
    // ---- the last iterates, and what the last step left for the problems still live (:936)
    CIP_HIP_CHECK(hipMemcpy2DAsync(C.iter_host, iter_row, (char *)a.S.z, stride, iter_row, count, hipMemcpyDeviceToHost, s));
    CIP_TRY(read_back());
    for (int j = 0; j < nlive; ++j) {
        const int z = live[j];
        if (flags_h[z]) { gone[z] = 1; fallback.push_back(z); continue; }
        if (steps > 0) n_solve[z] += nref_h[z];
        outcome[z].status = CIP_STATUS_ABANDONED;
    }
    if (timing) {
        double ms = 0;
        for (size_t k = 0; k + 1 < C.ev.size(); k += 2) { float t = 0; CIP_HIP_CHECK(hipEventElapsedTime(&t, C.ev[k], C.ev[k + 1])); ms += t; }
        g_small_time[0] = (double)(C.ev.size() / 2); g_small_time[1] = ms;
    }
    for (int z = 0; z < count; ++z) {
        if (gone[z] == 1) continue;
        const double *it = (const double *)((char *)C.iter_host + iter_row * (size_t)z);
        memcpy(y[z], it, sizeof(double) * n);
        if (p > 0) memcpy(w[z], it + n, sizeof(double) * p);
        if (m > 0) memcpy(v[z], it + N, sizeof(double) * m);
        res[z].status = outcome[z].status; res[z].n_factor = n_factor[z]; res[z].n_solve = n_solve[z];
        apply_certificate(outcome[z], n, m, p, y[z], p > 0 ? w[z] : nullptr, m > 0 ? v[z] : nullptr);
        stats[0] += 1;
    }
    return 0;
}

}   // namespace

extern "C" int cip_conicip_small_fits(const cip_problem *prob) { return small_check(prob, "cip_conicip_small_fits"); }

extern "C" int cip_conicip_small(int count, const cip_problem *probs, const double *const *c, const double *const *bvec,
                                 const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                                 double *const *v, cip_result *res) {
    for (int &q : g_small_stats) q = 0;
    g_small_time[0] = g_small_time[1] = 0.0;
    using namespace cipdrv;
    const char *who = "cip_conicip_small";
    const BatchCall call = {count, probs, nullptr, c, bvec, d, opt, y, w, v, res};
    CIP_TRY(check_batch_call(who, call, CHECK_ARRAYS));
    if (count == 0) return 0;
    const auto t_start = std::chrono::steady_clock::now();
    for (int i = 0; i < count; ++i) CIP_TRY(small_check(&probs[i], who));
    // (same_dims, not lock-step's same_shape: small_check has pinned the route and the matrix forms; whether an m = 0 problem's A is null does not count)
    for (int i = 1; i < count; ++i)
        if (!same_dims(probs[0], probs[i])) { cip_set_error("%s: problem %d differs in shape from problem 0", who, i); return CIP_E_UNSUPPORTED; }
    CIP_TRY(check_batch_call(who, call, CHECK_PROBLEM0));
    CIP_TRY(check_batch_call(who, call, CHECK_EVERY));
    const cip_options o = resolve_options(opt);
    std::vector<int> fallback;
    CIP_TRY(small_run(count, probs, c, bvec, d, o, y, w, v, res, fallback));
    // ---- the problems the kernels could not finish (a bad pivot: LPs, singular Q with free variables): from the start through
    // cip_conicip_mixed, whose results they get bit for bit
    if (!fallback.empty()) {
        SubBatch sub(call, fallback);
        const BatchCall g = sub.view();
        cip_options quiet;
        if (opt) { quiet = *opt; quiet.verbose = 0; }
        CIP_TRY(cip_conicip_mixed(g.count, g.probs, g.c, g.b, g.d, opt ? &quiet : nullptr, g.y, g.w, g.v, g.res, 4));
        sub.scatter();
        g_small_stats[1] = g.count;
    }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    for (int i = 0; i < count; ++i) res[i].wall_s = wall;
    return 0;
}

extern "C" int cip_small_stats(int *out4) {
    if (!out4) { cip_set_error("cip_small_stats: null argument"); return CIP_E_INVALID; }
    for (int i = 0; i < 4; ++i) out4[i] = g_small_stats[i];
    return 0;
}

extern "C" int cip_small_step_time(int enable, double *out2) {
    const int prev = g_small_timing;
    if (enable == 0 || enable == 1) g_small_timing = enable;
    if (out2) { out2[0] = g_small_time[0]; out2[1] = g_small_time[1]; }
    return prev;
}
