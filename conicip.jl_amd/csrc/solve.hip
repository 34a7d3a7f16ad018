// The Newton-step solves of the C ABI (include/cipkkt.h, level 3): solve3x3, solve2x2, their many-column forms and solve4x4, on the
// factor api.hip keeps.  Every entry point goes through ONE prologue (solve_begin), counts through ONE counter (solves_counted) and
// asks ONE function which problems of the call sit on a regularised factor (regularised).
#include "cip_handle.h"
#include "../../include/cipkkt.h"
#include <math.h>

// ------------------------------------------------------------------ products with A, A'
int cip_mul_A(cip_handle *h, double alpha, const double *x, double beta, double *y) {      // y = alpha A x + beta y  (m)
    if (h->m == 0) return 0;
    if (h->A_sparse) return cip_spmv_csr(h->stream, h->m, h->A_rp, h->A_ci, h->A_v, alpha, x, beta, y);
    return cip_gemv_t(h->stream, h->n, h->m, alpha, h->At, h->npad, x, beta, y);
}
int cip_mul_At(cip_handle *h, double alpha, const double *x, double beta, double *y) {     // y = alpha A' x + beta y (n)
    if (h->m == 0) {                                                                       // y = beta y, as the G branch of cip_gemv_dev
        if (beta == 0.0) return cip_zero(h->stream, h->n, y);
        if (beta != 1.0) return cip_axpby(h->stream, h->n, 0.0, y, beta, y);
        return 0;
    }
    if (h->A_sparse) return cip_spmv_csr(h->stream, h->n, h->T_rp, h->T_ci, h->T_v, alpha, x, beta, y);
    return cip_gemv_t(h->stream, h->m, h->n, alpha, h->A, h->m, x, beta, y);
}

// (F'F)^-1 z = F^-1 F^-T z
static int apply_FtF_inv(cip_handle *h, const double *z, double *tmp, double *out) {
    CIP_TRY(cip_cones_apply(h->stream, h->cs, CIP_OP_FINVT, z, tmp));
    return cip_cones_apply(h->stream, h->cs, CIP_OP_FINV, tmp, out);
}

// ------------------------------------------------------------------ what every solve starts with
// The factor must exist (`who`: the entry point, for the message) and its pivot flag is resolved: speculatively (no host wait, only if
// the read-back has landed) once a factorisation of this handle has been verified; before that the solve waits for the flag.
static int solve_begin(cip_handle *h, const char *who) {
    if (!h->factored) { cip_set_error("%s: no factorisation (call cip_factor first)", who); return CIP_E_NOTFACTORED; }
    return cip_factor_resolve(h, !h->pivots_verified);
}
// k solves are about to be enqueued (include/cipkkt.h: one per single solve, nrhs per many call); those on a factor whose flag is
// still in flight are the ones cip_factor_resolve asks the caller to repeat (CIP_E_RETRY) if it has to redo the factor
static void solves_counted(cip_handle *h, int k) {
    if (h->info_pending) h->spec_solves += k;
    h->n_solve += k;
}
// which problems of the call sit on a regularised factor: the group's mask in a batch, the handle's own state for one problem
static unsigned long long regularised(const cip_handle *h) {
    return cip_in_batch() ? (cip_tl_bz.mask & cip_tl_bz.reg_mask) : (h->reg_rel > 0.0 ? 1ull : 0ull);
}
// the entry points whose host code knows one problem only (h->reg_rel, launches without the batch argument)
static int refuse_batch(const char *who) {
    if (!cip_in_batch()) return 0;
    cip_set_error("%s: not available inside a lock-step group", who);
    return CIP_E_INVALID;
}
// what the refined solves of a regularised factor allocate on first use; a lock-step group that may regularise has them in its
// handles' slabs instead (cip_handle_layout: CIP_EXTRA_REFINE)
static int alloc_refine_buffers(cip_handle *h) {
    RefView v;
    if (!h->ref) CIP_TRY(cip_handle_alloc(h, (void **)&h->ref, ref_layout(nullptr, h, &v)));
    if (!h->c2x2 && h->m > 0 && h->route == CIP_ROUTE_SCHUR) CIP_TRY(cip_handle_alloc(h, (void **)&h->c2x2, sizeof(double) * h->m));
    return 0;
}
static int ldlt_sweeps(cip_handle *h) {      // the triangular sweeps on h->rhs, replayed from the handle's graph where it has one
    return graph_run(h, &h->gx_solve, [h]() { return cip_ldlt_solve(h->stream, h->K, h->Npad, h->ldk, h->ws, h->rhs); });
}

// ------------------------------------------------------------------ one solve on the factor as it is, two ways (level 3)
// solve3x3_once: one column -- batch-aware copies and mat-vecs, the recorded sweeps.  solve3x3_chunk: kc <= 64 columns (X n x kc,
// Y p x kc, Z m x kc, col-major, ld = rows) -- the cone operations and the CSR products per column, the dense A / A' products and the
// LDL' sweeps over all columns (solve_many.hip).  The same steps in the same order; each keeps its own bits.
// z == NULL (Schur route only): the 2x2 form [S G'; G 0][a; b] = [x; y] (src/kktsolvers.jl:297-302), c is not written; c may alias z
static int solve3x3_once(cip_handle *h, const double *x, const double *y, const double *z, double *a, double *b, double *c) {
    hipStream_t s = h->stream;
    const int n = h->n, p = h->p, N = h->N, Npad = h->Npad;
    const int m = z ? h->m : 0;
    double *R = h->rhs, *t = h->mt1, *tmp = h->mt2, *u = h->mt3;
    if (h->route == CIP_ROUTE_SCHUR) {
        // algebra of pivotgen, src/kktsolvers.jl:324-330, with the exact (F'F)^-1 = F^-1 F^-T:
        //   t = (F'F)^-1 z ; [S G'; G 0][a; b] = [x + A't; y] ; c = t - (F'F)^-1 A a
        if (m > 0) CIP_TRY(apply_FtF_inv(h, z, tmp, t));
        CIP_TRY(cip_copy(s, n, x, R));
        if (m > 0) CIP_TRY(cip_mul_At(h, 1.0, t, 1.0, R));
        if (p > 0) CIP_TRY(cip_copy(s, p, y, R + n));
        if (Npad > N) CIP_TRY(cip_zero(s, Npad - N, R + N));
        CIP_TRY(ldlt_sweeps(h));
        CIP_TRY(cip_copy(s, n, R, a));
        if (p > 0) CIP_TRY(cip_copy(s, p, R + n, b));
        if (m > 0) {
            CIP_TRY(cip_mul_A(h, 1.0, R, 0.0, u));
            CIP_TRY(apply_FtF_inv(h, u, tmp, u));
            CIP_TRY(cip_axpby(s, m, 1.0, t, 0.0, c));
            CIP_TRY(cip_axpby(s, m, -1.0, u, 1.0, c));
        }
    } else {
        // [-F'F -A 0; -A' Q G'; 0 G 0] [c; a; b] = [-z; x; y]
        if (m > 0) CIP_TRY(cip_axpby(s, m, -1.0, z, 0.0, R));
        CIP_TRY(cip_copy(s, n, x, R + m));
        if (p > 0) CIP_TRY(cip_copy(s, p, y, R + m + n));
        if (Npad > N) CIP_TRY(cip_zero(s, Npad - N, R + N));
        CIP_TRY(ldlt_sweeps(h));
        if (m > 0) CIP_TRY(cip_copy(s, m, R, c));
        CIP_TRY(cip_copy(s, n, R + m, a));
        if (p > 0) CIP_TRY(cip_copy(s, p, R + m + n, b));
    }
    return 0;
}
static int solve3x3_chunk(cip_handle *h, int kc, const double *x, const double *y, const double *z, double *a, double *b, double *c) {
    hipStream_t s = h->stream;
    const int n = h->n, p = h->p, N = h->N, Npad = h->Npad;
    const int m = z ? h->m : 0;
    const long ldr = Npad;
    ManyView v;
    many_layout(h->many, h, &v);
    double *R = v.R, *T = v.T, *U = v.U, *S = v.S, *tmp = h->mt2;
    if (h->route == CIP_ROUTE_SCHUR) {
        // t = (F'F)^-1 z ; [S G'; G 0][a; b] = [x + A't; y] ; c = t - (F'F)^-1 A a
        for (int j = 0; j < kc && m > 0; ++j) CIP_TRY(apply_FtF_inv(h, z + (long)j * m, tmp, T + (long)j * m));
        CIP_TRY(cip_block_copy(s, n, kc, 1.0, x, n, nullptr, R, ldr));
        if (m > 0 && !h->A_sparse) CIP_TRY(cip_gemm_tn(s, n, kc, m, 1.0, h->A, m, T, m, 1.0, R, ldr));
        if (m > 0 && h->A_sparse)
            for (int j = 0; j < kc; ++j) CIP_TRY(cip_spmv_csr(s, n, h->T_rp, h->T_ci, h->T_v, 1.0, T + (long)j * m, 1.0, R + j * ldr));
        if (p > 0) CIP_TRY(cip_block_copy(s, p, kc, 1.0, y, p, nullptr, R + n, ldr));
        if (Npad > N) CIP_TRY(cip_block_copy(s, Npad - N, kc, 0.0, nullptr, 0, nullptr, R + N, ldr));
        CIP_TRY(cip_ldlt_solve_many(s, h->K, Npad, h->ldk, h->ws, S, R, ldr, kc, false));
        CIP_TRY(cip_block_copy(s, n, kc, 1.0, R, ldr, nullptr, a, n));
        if (p > 0) CIP_TRY(cip_block_copy(s, p, kc, 1.0, R + n, ldr, nullptr, b, p));
        if (m > 0) {
            if (!h->A_sparse) CIP_TRY(cip_gemm_tn(s, m, kc, n, 1.0, h->At, h->npad, R, ldr, 0.0, U, m));
            if (h->A_sparse)
                for (int j = 0; j < kc; ++j) CIP_TRY(cip_spmv_csr(s, m, h->A_rp, h->A_ci, h->A_v, 1.0, R + j * ldr, 0.0, U + (long)j * m));
            for (int j = 0; j < kc; ++j) CIP_TRY(apply_FtF_inv(h, U + (long)j * m, tmp, U + (long)j * m));
            CIP_TRY(cip_axpby(s, m * kc, 1.0, T, 0.0, c));
            CIP_TRY(cip_axpby(s, m * kc, -1.0, U, 1.0, c));
        }
    } else {
        // [-F'F -A 0; -A' Q G'; 0 G 0] [c; a; b] = [-z; x; y]
        if (m > 0) CIP_TRY(cip_block_copy(s, m, kc, -1.0, z, m, nullptr, R, ldr));
        CIP_TRY(cip_block_copy(s, n, kc, 1.0, x, n, nullptr, R + m, ldr));
        if (p > 0) CIP_TRY(cip_block_copy(s, p, kc, 1.0, y, p, nullptr, R + m + n, ldr));
        if (Npad > N) CIP_TRY(cip_block_copy(s, Npad - N, kc, 0.0, nullptr, 0, nullptr, R + N, ldr));
        CIP_TRY(cip_ldlt_solve_many(s, h->K, Npad, h->ldk, h->ws, S, R, ldr, kc, false));
        if (m > 0) CIP_TRY(cip_block_copy(s, m, kc, 1.0, R, ldr, nullptr, c, m));
        CIP_TRY(cip_block_copy(s, n, kc, 1.0, R + m, ldr, nullptr, a, n));
        if (p > 0) CIP_TRY(cip_block_copy(s, p, kc, 1.0, R + m + n, ldr, nullptr, b, p));
    }
    return 0;
}

// r = (x, y, z) - K3 (a, b, c) with the TRUE (unregularised) operator:
//   rx = x - (Q a + G' b - A' c) ;  ry = y - G a ;  rz = z - (A a + F'F c)
static int kkt3_residual(cip_handle *h, const double *x, const double *y, const double *z, const double *a, const double *b,
                         const double *c, double *rx, double *ry, double *rz) {
    hipStream_t s = h->stream;
    const int n = h->n, m = h->m, p = h->p;
    CIP_TRY(cip_axpby(s, n, 1.0, x, 0.0, rx));
    CIP_TRY(cip_mul_Q(h, -1.0, a, 1.0, rx, false));
    if (p > 0) {
        CIP_TRY(cip_gemv_t(s, p, n, -1.0, h->G, p, b, 1.0, rx));
        CIP_TRY(cip_axpby(s, p, 1.0, y, 0.0, ry));
        CIP_TRY(cip_gemv_t(s, n, p, -1.0, h->Gt, n, a, 1.0, ry));
    }
    if (m > 0) {
        CIP_TRY(cip_mul_At(h, 1.0, c, 1.0, rx));
        CIP_TRY(cip_axpby(s, m, 1.0, z, 0.0, rz));
        CIP_TRY(cip_mul_A(h, -1.0, a, 1.0, rz));
        CIP_TRY(cip_cones_apply(s, h->cs, CIP_OP_F, c, h->mt2));
        CIP_TRY(cip_cones_apply(s, h->cs, CIP_OP_FT, h->mt2, h->mt2));
        CIP_TRY(cip_axpby(s, m, -1.0, h->mt2, 1.0, rz));
    }
    return 0;
}

// ------------------------------------------------------------------ solve3x3, solve2x2 on device pointers
extern "C" int cip_solve3x3_dev(cip_handle *h, const double *x, const double *y, const double *z, double *a, double *b,
                                double *c) {
    if (!h) return CIP_E_INVALID;
    const int n = h->n, m = h->m, p = h->p;
    CipRange rg("cip:solve3x3");
    CIP_TRY(solve_begin(h, "cip_solve3x3"));
    solves_counted(h, 1);
    const bool batch = cip_in_batch();
    unsigned long long live = regularised(h);
    if (!live) return solve3x3_once(h, x, y, z, a, b, c);
    // Regularised factor: iterative refinement against the true operator (the factor is of K + E, |E_ii| = reg_rel
    // times the row's largest entry): a few steps bring the residual to rounding level while ||K^-1 E|| < 1.
    // In a batch the first solve runs for every problem of the mask, from the private copy of the right-hand side (copies are
    // exact: the others get the bits of solve3x3_once on the original); the refinement then runs under the mask of the regularised
    // problems, each leaving it when ITS residual has converged, stagnates or is not finite -- every problem sees the launches it
    // sees alone.
    hipStream_t s = h->stream;
    if (!h->ref) {
        if (batch) { cip_set_error("cip_solve3x3: regularised problems in a batch whose handles have no refinement buffers"); return CIP_E_INVALID; }
        CIP_TRY(alloc_refine_buffers(h));
    }
    RefView v;
    ref_layout(h->ref, h, &v);
    double *xs = v.rhs.x, *ys = v.rhs.y, *zs = v.rhs.z;           // private copy of the right-hand side (z may alias c)
    double *rx = v.res.x, *ry = v.res.y, *rz = v.res.z, *da = v.cor.x, *db = v.cor.y, *dc = v.cor.z;
    CIP_TRY(cip_copy(s, n, x, xs));
    if (p > 0) CIP_TRY(cip_copy(s, p, y, ys));
    if (m > 0) CIP_TRY(cip_copy(s, m, z, zs));
    CIP_TRY(solve3x3_once(h, xs, ys, zs, a, b, c));
    CipMaskScope mask;
    const int B = batch ? cip_tl_bz.B : 1;
    double prev[CIP_BATCH_MAX], d6[6 * CIP_BATCH_MAX];
    for (int q = 0; q < B; ++q) prev[q] = __builtin_inf();
    for (int it = 0; it < 6 && live; ++it) {
        if (batch) mask.set(live);
        CIP_TRY(kkt3_residual(h, xs, ys, zs, a, b, c, rx, ry, rz));
        const double *px[6] = {rx, ry, rz, xs, ys, zs};
        const int ln[6] = {n, p, m, n, p, m};
        CIP_TRY(cip_dots(s, 6, px, px, ln, h->dot_scratch, d6));       // (a batch: B x 6, problem-major)
        for (int q = 0; q < B; ++q) {
            if (!((live >> q) & 1ull)) continue;
            const double *dq = d6 + 6 * q;
            const double rn = sqrt(dq[0] + dq[1] + dq[2]), bn = sqrt(dq[3] + dq[4] + dq[5]);
            if (!(rn > 1e-14 * bn) || !(rn < prev[q])) live &= ~(1ull << q);         // converged, stagnating, or not finite
            prev[q] = rn;
        }
        if (!live) break;
        if (batch) mask.set(live);
        CIP_TRY(solve3x3_once(h, rx, ry, rz, da, db, dc));
        CIP_TRY(cip_axpby(s, n, 1.0, da, 1.0, a));
        if (p > 0) CIP_TRY(cip_axpby(s, p, 1.0, db, 1.0, b));
        if (m > 0) CIP_TRY(cip_axpby(s, m, 1.0, dc, 1.0, c));
    }
    return 0;
}

// The 2x2 form of the plugin (src/ConicIP.jl:450-466; what `pivot` wraps, src/kktsolvers.jl:297-302, :316-349):
//   [Q + A'(F'F)^-1 A   G'] [dy]   [y]
//   [G                  0 ] [dw] = [w]      on the factor of the Schur route.
// One problem only: the loops, which run under a lock-step group's batch context, solve through cip_solve4x4_dev.
extern "C" int cip_solve2x2_dev(cip_handle *h, const double *y, const double *w, double *dy, double *dw) {
    if (!h) return CIP_E_INVALID;
    if (h->route != CIP_ROUTE_SCHUR) { cip_set_error("cip_solve2x2: needs the Schur route"); return CIP_E_UNSUPPORTED; }
    CIP_TRY(refuse_batch("cip_solve2x2"));
    CIP_TRY(solve_begin(h, "cip_solve2x2"));
    if (h->reg_rel > 0.0 && h->m > 0) {
        // regularised factor: the refined 3x3 solve with z = 0 (its first two components are the 2x2 solution), which counts itself
        CIP_TRY(cip_zero(h->stream, h->m, h->mt1));
        if (!h->c2x2) CIP_TRY(alloc_refine_buffers(h));
        return cip_solve3x3_dev(h, y, w, h->mt1, dy, dw, h->c2x2);
    }
    solves_counted(h, 1);
    return solve3x3_once(h, y, w, nullptr, dy, dw, nullptr);
}

// ------------------------------------------------------------------ many right-hand sides (level 3)
// X n x nrhs, Y p x nrhs, Z m x nrhs (col-major, ld = rows); the same as nrhs calls of the single entry point, 64 columns at a time
// through solve3x3_chunk.  Regularised factor: nrhs refined single solves.  One problem only, as cip_solve2x2_dev.
// two2: the 2x2 form (y, w -> dy, dw; z, c unused).  one_is_single: nrhs == 1 is the single entry point (its bits)
static int solve_many_impl(cip_handle *h, bool two2, int nrhs, const double *X, const double *Y, const double *Z, double *A, double *Bo,
                           double *C, bool one_is_single) {
    const int n = h->n, m = h->m, p = h->p;
    if (nrhs == 1 && one_is_single) return two2 ? cip_solve2x2_dev(h, X, Y, A, Bo) : cip_solve3x3_dev(h, X, Y, Z, A, Bo, C);
    const char *who = two2 ? "cip_solve2x2_many" : "cip_solve3x3_many";
    CIP_TRY(refuse_batch(who));
    CIP_TRY(solve_begin(h, who));
    if (h->reg_rel > 0.0 && (!two2 || m > 0)) {
        // regularised factor: the refinement against the true operator runs per column, through the single path (which counts)
        for (int j = 0; j < nrhs; ++j)
            CIP_TRY(two2 ? cip_solve2x2_dev(h, X + (long)j * n, Y + (long)j * p, A + (long)j * n, Bo + (long)j * p)
                         : cip_solve3x3_dev(h, X + (long)j * n, Y + (long)j * p, Z + (long)j * m, A + (long)j * n, Bo + (long)j * p,
                                            C + (long)j * m));
        return 0;
    }
    solves_counted(h, nrhs);
    ManyView v;
    if (!h->many) CIP_TRY(cip_handle_alloc(h, (void **)&h->many, many_layout(nullptr, h, &v)));
    CipRange rg(two2 ? "cip:solve2x2_many" : "cip:solve3x3_many");
    for (int c0 = 0; c0 < nrhs; c0 += CIP_MANY_CHUNK) {
        const int kc = nrhs - c0 < CIP_MANY_CHUNK ? nrhs - c0 : CIP_MANY_CHUNK;
        CIP_TRY(solve3x3_chunk(h, kc, X + (long)c0 * n, Y + (long)c0 * p, two2 ? nullptr : Z + (long)c0 * m, A + (long)c0 * n,
                               Bo + (long)c0 * p, two2 ? nullptr : C + (long)c0 * m));
    }
    return 0;
}

// ------------------------------------------------------------------ host pointers
// The host-pointer entry points, `cap` columns at a time through a StageView of `stage` (h->stage, one column: the single entry
// points; h->many_stage, CIP_MANY_CHUNK columns: the many-column ones).  Per chunk: the copies in, the pivot flag (these calls are
// synchronous anyway), the device entry point, the copies back, a wait.
static int solve_host(cip_handle *h, bool two2, int nrhs, double *stage, int cap, const double *X, const double *Y, const double *Z,
                      double *A, double *Bo, double *C) {
    hipStream_t s = h->stream;
    const size_t n = h->n, p = h->p, m = two2 ? 0 : h->m;
    StageView v;
    stage_layout(stage, h, cap, &v);                 // (a chunk of fewer than `cap` columns: the front of every block)
    for (int c0 = 0; c0 < nrhs; c0 += cap) {
        const size_t kc = nrhs - c0 < cap ? nrhs - c0 : cap;
        CIP_HIP_CHECK(hipMemcpyAsync(v.in.x, X + c0 * n, sizeof(double) * n * kc, hipMemcpyHostToDevice, s));
        if (p > 0) CIP_HIP_CHECK(hipMemcpyAsync(v.in.y, Y + c0 * p, sizeof(double) * p * kc, hipMemcpyHostToDevice, s));
        if (m > 0) CIP_HIP_CHECK(hipMemcpyAsync(v.in.z, Z + c0 * m, sizeof(double) * m * kc, hipMemcpyHostToDevice, s));
        if (h->factored) CIP_TRY(cip_factor_resolve(h, true));
        CIP_TRY(solve_many_impl(h, two2, (int)kc, v.in.x, v.in.y, v.in.z, v.out.x, v.out.y, v.out.z, nrhs == 1));
        CIP_HIP_CHECK(hipMemcpyAsync(A + c0 * n, v.out.x, sizeof(double) * n * kc, hipMemcpyDeviceToHost, s));
        if (p > 0) CIP_HIP_CHECK(hipMemcpyAsync(Bo + c0 * p, v.out.y, sizeof(double) * p * kc, hipMemcpyDeviceToHost, s));
        if (m > 0) CIP_HIP_CHECK(hipMemcpyAsync(C + c0 * m, v.out.z, sizeof(double) * m * kc, hipMemcpyDeviceToHost, s));
        CIP_HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
}
extern "C" int cip_solve3x3(cip_handle *h, const double *x, const double *y, const double *z, double *a, double *b,
                            double *c) {
    if (!h) return CIP_E_INVALID;
    return solve_host(h, false, 1, h->stage, 1, x, y, z, a, b, c);
}
extern "C" int cip_solve2x2(cip_handle *h, const double *y, const double *w, double *dy, double *dw) {
    if (!h) return CIP_E_INVALID;
    return solve_host(h, true, 1, h->stage, 1, y, w, nullptr, dy, dw, nullptr);
}

// the four many-column entry points: argument checks, then the device form or its host staging (h->many_stage, on first use)
static int solve_many_entry(cip_handle *h, const char *who, bool two2, bool host, int nrhs, const double *X, const double *Y,
                            const double *Z, double *A, double *Bo, double *C) {
    const bool ok = h && nrhs >= 0 && (nrhs == 0 || (X && A && (h->p == 0 || (Y && Bo)) && (two2 || h->m == 0 || (Z && C))));
    if (!ok) { cip_set_error("%s: bad argument", who); return CIP_E_INVALID; }
    if (nrhs == 0) return 0;
    if (two2 && h->route != CIP_ROUTE_SCHUR) { cip_set_error("cip_solve2x2_many: needs the Schur route"); return CIP_E_UNSUPPORTED; }
    if (!host) return solve_many_impl(h, two2, nrhs, X, Y, Z, A, Bo, C, true);
    StageView v;
    if (!h->many_stage) CIP_TRY(cip_handle_alloc(h, (void **)&h->many_stage, stage_layout(nullptr, h, CIP_MANY_CHUNK, &v)));
    return solve_host(h, two2, nrhs, h->many_stage, CIP_MANY_CHUNK, X, Y, Z, A, Bo, C);
}
extern "C" int cip_solve3x3_many_dev(cip_handle *h, int nrhs, const double *X, const double *Y, const double *Z, double *A, double *Bo,
                                     double *C) {
    return solve_many_entry(h, "cip_solve3x3_many_dev", false, false, nrhs, X, Y, Z, A, Bo, C);
}
extern "C" int cip_solve3x3_many(cip_handle *h, int nrhs, const double *X, const double *Y, const double *Z, double *A, double *Bo,
                                 double *C) {
    return solve_many_entry(h, "cip_solve3x3_many", false, true, nrhs, X, Y, Z, A, Bo, C);
}
extern "C" int cip_solve2x2_many_dev(cip_handle *h, int nrhs, const double *Y, const double *W, double *DY, double *DW) {
    return solve_many_entry(h, "cip_solve2x2_many_dev", true, false, nrhs, Y, W, nullptr, DY, DW, nullptr);
}
extern "C" int cip_solve2x2_many(cip_handle *h, int nrhs, const double *Y, const double *W, double *DY, double *DW) {
    return solve_many_entry(h, "cip_solve2x2_many", true, true, nrhs, Y, W, nullptr, DY, DW, nullptr);
}

// ------------------------------------------------------------------ solve4x4
// diag F (the packed scaling) when the cone set is R cones only -- the native loops then fuse the cone operations of their
// element-wise chains into the vector kernels (vecops.hip: k_loop_*), solve4x4 those around its sweeps; NULL otherwise
const double *cip_loop_all_r(cip_handle *h) { return cip_all_r(h) ? h->cs.d_scal : nullptr; }
// solve4x4 (src/ConicIP.jl:684-692):  q = r.s (./) lambda ; t1 = F'q ; (dy,dw,dv) = solve3x3(r.y, r.w, r.v + t1) ;
// ds = t1 - F'(F dv).   r, dz are contiguous (y[n], w[p], v[m], s[m]).
extern "C" int cip_solve4x4_dev(cip_handle *h, const double *lambda, const double *r, double *dz) {
    if (!h) return CIP_E_INVALID;
    hipStream_t s = h->stream;
    const int n = h->n, m = h->m, p = h->p;
    const double *ry = r, *rw = r + n, *rv = r + n + p, *rs = r + n + p + m;
    double *dy = dz, *dw = dz + n, *dv = dz + n + p, *ds = dz + n + p + m;
    if (h->s4_fused < 0) h->s4_fused = cip_all_r(h) && cip_env_int("CIP_S4_FUSED", 1) != 0;
    // the fused kernels read r across threads (CSR gathers) while writing dz: an in-place call (dz overlapping r) takes the
    // element-wise generic path, which tolerates it
    const size_t len4 = (size_t)n + p + 2 * (size_t)m;
    const bool aliased = dz < r + len4 && r < dz + len4;
    // the regularised problems of the call (a lock-step group may hold both kinds, lockstep.hip) take the generic path below with its
    // refined solve; the others take the fused path first, under their own mask
    const unsigned long long regd = regularised(h), plain = cip_tl_bz.mask & ~regd;
    CipMaskScope mask;
    if (h->s4_fused && !aliased && h->route == CIP_ROUTE_SCHUR && plain) {
        mask.set(plain);
        // all cones R (F = diag(f), f = the packed scaling): the element-wise launches around the sweeps fused into one kernel
        // in front and one behind them (vecops.hip: k_s4_pre_r / k_s4_post_r), the same operations on every element
        CipRange rg("cip:solve3x3");
        CIP_TRY(solve_begin(h, "cip_solve4x4"));
        if (!regularised(h)) {                         // (the resolve may have switched the handle to the regularised factorisation)
            solves_counted(h, 1);
            const double *f = h->cs.d_scal;
            double *t = h->mt1, *u = h->mt3;
            CIP_TRY(cip_s4_pre_r(s, m, n, p, h->Npad, f, rs, lambda, rv, ry, rw, ds, t, h->rhs, h->A_sparse ? h->T_rp : nullptr, h->T_ci, h->T_v));
            if (!h->A_sparse) CIP_TRY(cip_mul_At(h, 1.0, t, 1.0, h->rhs));
            CIP_TRY(ldlt_sweeps(h));
            if (!h->A_sparse) CIP_TRY(cip_mul_A(h, 1.0, h->rhs, 0.0, u));
            CIP_TRY(cip_s4_post_r(s, m, n, p, f, t, h->rhs, h->A_sparse ? nullptr : u, h->A_sparse ? h->A_rp : nullptr, h->A_ci, h->A_v, dy, dw, dv, ds));
            if (!regd) return 0;
            mask.set(regd);
        }
    }
    // ds is used as t1; dv temporarily holds r.v + t1 (input z of the 3x3 solve; solve3x3 copies it before writing c)
    if (m > 0) {
        CIP_TRY(cip_cones_div(s, h->cs, rs, lambda, ds));          // q
        CIP_TRY(cip_cones_apply(s, h->cs, CIP_OP_FT, ds, ds));     // t1 = F'q (in place)
        CIP_TRY(cip_axpby(s, m, 1.0, rv, 0.0, dv));
        CIP_TRY(cip_axpby(s, m, 1.0, ds, 1.0, dv));                // dv <- r.v + t1
    }
    CIP_TRY(cip_solve3x3_dev(h, ry, rw, dv, dy, dw, dv));
    if (m > 0) {
        double *u = h->mt3;
        CIP_TRY(cip_cones_apply(s, h->cs, CIP_OP_F, dv, u));
        CIP_TRY(cip_cones_apply(s, h->cs, CIP_OP_FT, u, u));
        CIP_TRY(cip_axpby(s, m, -1.0, u, 1.0, ds));                // ds = t1 - F'(F dv)
    }
    return 0;
}
