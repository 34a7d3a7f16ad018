// Native interior-point loop: the Mehrotra predictor-corrector iteration of the reference's `conicIP`
// (src/ConicIP.jl:468-939) driven from C++ through the library's own device entry points, every vector
// resident in HBM.  The host sees only scalars (residual norms, mu, step lengths), exactly as the Python
// driver (cipkkt/driver.py) does -- this is the same loop without the interpreter between the launches
// (measured, warm library: dense QP n = 8192 0.111 -> 0.087 s to converge, n = 2048 20.2 -> 18.4 ms; the loop is
// GPU-bound either way).  The Python and the native loop issue the same kernels in the same order and agree to the
// last bit (tests/test_gpu_driver.py).
//
// The iteration is written once (Loop::run), for the B problems of the calling thread's batch context: cip_conicip below
// is B = 1 under the default context, a lock-step group (lockstep.hip) B problems under its own.
//
// Quirks of the reference are kept: a factorisation also happens in the terminating
// iteration (:737 precedes :786), rPr ignores the equality residual (:765), norm(v4x1) is the sum of the
// block 2-norms (:61), the returned (y, w, v) is the last iterate.
#include "cip_driver.h"
#include "cip_batch_front.h"
#include <chrono>
#include <vector>

using namespace cipdrv;

size_t cip_driver_bytes(const cip_handle *h) { return Vectors().carve(nullptr, h->n, h->m, h->p); }

int cipdrv::Loop::run(const double *const *c, const double *const *b, const double *const *d, const cip_options &o, cip_result *res,
                      double *trace, int trace_cap) {
    const int n = h->n, m = h->m, p = h->p, NT = n + p + 2 * m;
    hipStream_t s = h->stream;
    V.carve(h->drv, n, m, p);
    double *c_d = V.c_d, *b_d = V.b_d, *d_d = V.d_d;
    Vec4 &zv = V.z, &r0 = V.r0, &rleft = V.rleft, &r = V.r, &daff = V.daff, &dz = V.dz, &dzr = V.dzr, &rIr = V.rIr, &rkkt = V.rkkt;
    double *e = V.e, *lam = V.lam, *mb1 = V.mb1, *mb2 = V.mb2, *mb3 = V.mb3;
    double *Qy = V.Qy, *pinf = V.pinf, *Ays = V.Ays, *Gy = V.Gy;
    CipHostScratch hs;
    if (cip_host_scratch(&hs)) { cip_set_error("interior-point loop: host scratch"); return CIP_E_HIP; }
    int rc;
#define CK(x) do { if ((rc = (x)) != 0) return rc; } while (0)
    CK(cip_zero(s, (long)(cip_driver_bytes(h) / sizeof(double)), h->drv));
    std::vector<Norms> nm(B);
    for (int z = 0; z < B; ++z) {                   // problem z's vectors are problem 0's addresses + z * stride
        const size_t off = (size_t)cip_tl_bz.stride * z;
        CIP_HIP_CHECK(hipMemcpyAsync((char *)c_d + off, c[z], sizeof(double) * n, hipMemcpyHostToDevice, s));
        if (m > 0) CIP_HIP_CHECK(hipMemcpyAsync((char *)b_d + off, b[z], sizeof(double) * m, hipMemcpyHostToDevice, s));
        if (p > 0) CIP_HIP_CHECK(hipMemcpyAsync((char *)d_d + off, d[z], sizeof(double) * p, hipMemcpyHostToDevice, s));
        nm[z] = host_norms(n, m, p, c[z], m > 0 ? b[z] : nullptr, p > 0 ? d[z] : nullptr);
        res[z] = fresh_result();
    }
    const double conedim = cone_degree(h);          // (:547-552); e (:559-565) below
    const double *f = cip_loop_all_r(h);            // diag F when every cone is an R cone (the loop's cone operations are then fused into its vector kernels), else NULL
    if (m > 0) CK(cip_cone_identity_dev(h, e));

    std::vector<double> optBest(B, INFINITY), dt((size_t)B * 16), q4((size_t)B * 4), n2((size_t)B * 4), sigma(B), mu(B), mubar(B),
        alpha(B), av(B), as(B), tmp(B);
    // (the loop narrows the thread's batch mask as problems stop; it leaves the mask as it found it)
    CipMaskScope mask;
    auto count = [&](std::vector<int> &cnt, unsigned long long mk) { for (int z = 0; z < B; ++z) cnt[z] += (int)((mk >> z) & 1ull); };
    // The max-step pair (x1, d1), (x2, d2) of every problem of the mask (:708-709, :881-882, :927-928).  The minima ride on the next
    // read-back (wait: read back now); pair(z) reads problem z's behind it.  One problem: slots MS_SLOT, MS_SLOT + 1 of the host-mapped
    // scratch (the dot products use 0 .. 31); a batch: slots STEP_SLOT, STEP_SLOT + 1 of every problem's row of the gather buffer
    // (0 .. 31: the dot products, 32 .. 35: pivot flags)
    constexpr int MS_SLOT = 64, STEP_SLOT = 40;
    auto maxstep_pair = [&](const double *x1, const double *d1, const double *x2, const double *d2, double scale, bool wait) -> int {
        int e2;
        if (!cip_in_batch()) {
            if ((e2 = cip_cones_maxstep2(s, h->cs, x1, d1, x2, d2, scale, nullptr, MS_SLOT))) return e2;
            return wait ? cip_wait(s) : 0;
        }
        if ((e2 = cip_cones_maxstep(s, h->cs, x1, d1, scale, nullptr, STEP_SLOT))) return e2;
        if ((e2 = cip_cones_maxstep(s, h->cs, x2, d2, scale, nullptr, STEP_SLOT + 1))) return e2;
        if (!wait) return 0;
        CIP_HIP_CHECK(hipMemcpyAsync(cip_tl_bz.gather_host, cip_tl_bz.gather_dev, sizeof(double) * B * CIP_GATHER, hipMemcpyDeviceToHost, s));
        return cip_wait(s);
    };
    auto pair = [&](int z) -> const double * {
        return cip_in_batch() ? cip_tl_bz.gather_host + (size_t)z * CIP_GATHER + STEP_SLOT : hs.host + MS_SLOT;
    };

    // ---------------------------------------------------------------- initial point (:704-713)
    mask.set(active);
    CK(cip_set_scaling_identity(h));
    CK(factor()); count(n_factor, active);
    CK(cip_axpby(s, n, 1.0, c_d, 0.0, r0.y)); CK(cip_axpby(s, p, 1.0, d_d, 0.0, r0.w)); CK(cip_axpby(s, m, 1.0, b_d, 0.0, r0.v));
    CK(cip_zero(s, m, r0.s));
    // initial point: one wait (LPs meet their first bad pivot here)
    CK(ride_pivots());
    CK(take_pivots(false));
    mask.set(active);
    if (active) {
        CK(cip_solve4x4_dev(h, e, r0.base, zv.base)); count(n_solve, active);
        if (m > 0) {
            CK(maxstep_pair(zv.v, nullptr, zv.s, nullptr, 1.0, true));
            for (int z = 0; z < B; ++z) { av[z] = -pair(z)[0]; as[z] = -pair(z)[1]; }
            CK(cip_axpby_ps(s, m, av.data(), e, 1.0, zv.v));
            CK(cip_axpby_ps(s, m, as.data(), e, 1.0, zv.s));
        }
    }

    for (iters = 1; iters <= o.maxIters && active; ++iters) {                          // :730
        const int Iter = iters;
        CipRange iter_range("cip:iteration");
        mask.set(active);
        if (m > 0) CK(cip_set_scaling_from_iterate_dev(h, zv.v, zv.s, lam));           // :732-735 (F, lambda = F v)
        CK(factor()); count(n_factor, active);                                        // :737 -> :682
        // (round 5) the element-wise part of :746-753 is one kernel (vecops.hip: k_loop_resid) behind the mat-vecs; with R cones
        // only (f != NULL) lam o lam is formed there too
        if (m > 0 && !f) CK(cip_cone_prod_dev(h, lam, lam, rleft.s));                  // :746
        CK(cip_gemv_dev(h, CIP_MAT_Q, 0, 1.0, zv.y, 0.0, Qy));                         // needed by the certificates
        CK(cip_axpby(s, n, 1.0, Qy, 0.0, rleft.y));                                    // :747-750: Q y + G'w - A'v, G y, A y (- s: in the kernel)
        if (p > 0) {
            CK(cip_gemv_dev(h, CIP_MAT_G, 1, 1.0, zv.w, 1.0, rleft.y));
            CK(cip_gemv_dev(h, CIP_MAT_G, 0, 1.0, zv.y, 0.0, rleft.w));
            CK(cip_gemv_dev(h, CIP_MAT_G, 1, 1.0, zv.w, 0.0, pinf));
        }
        if (m > 0) {
            CK(cip_gemv_dev(h, CIP_MAT_A, 1, -1.0, zv.v, 1.0, rleft.y));
            CK(cip_gemv_dev(h, CIP_MAT_A, 0, 1.0, zv.y, 0.0, rleft.v));
            CK(cip_gemv_dev(h, CIP_MAT_A, 1, -1.0, zv.v, p > 0 ? 1.0 : 0.0, pinf));    // pinf = G'w - A'v (a zero start when p == 0: the same bits)
        } else if (p == 0) CK(cip_zero(s, n, pinf));
        // rleft.v -= s, [rleft.s = lam o lam], Gy = rleft.w, Ays = rleft.v, r0 = rleft - (c, d, b, 0)   (:753)
        CK(cip_loop_resid(s, n, m, p, rleft.base, zv.s, c_d, d_d, b_d, lam, f, r0.base, Gy, Ays));

        const double *px[16] = {zv.v, c_d, r0.y, r0.v, r0.s, zv.y, zv.w, zv.v, d_d, b_d, pinf, zv.y, zv.v, Ays, Gy, Qy};
        const double *py[16] = {zv.s, zv.y, r0.y, r0.v, r0.s, Qy, r0.w, r0.v, zv.w, zv.v, pinf, zv.y, zv.v, Ays, Gy, Qy};
        const int ln[16] = {m, n, n, m, m, n, p, m, p, m, n, n, m, m, p, n};
        CK(ride_pivots());
        CK(cip_dots_dev(h, 16, px, py, ln, dt.data()));
        CK(take_pivots(true));             // the stream has just been drained: the pivot flags of this iteration's factorisation are in
        double *tr = (trace && Iter <= trace_cap) ? trace + (size_t)(Iter - 1) * CIP_TRACE_COLS : nullptr;   // (one problem only)
        for (int z = 0; z < B; ++z) {
            if (!((active >> z) & 1ull)) continue;
            IterDots dd;
            for (int i = 0; i < 16; ++i) dd.v[i] = dt[(size_t)z * 16 + i];
            outcome[z] = evaluate_iteration(dd, nm[z], conedim, m, p, o, Iter, &res[z], optBest[z], tr);
            mu[z] = outcome[z].mu; mubar[z] = outcome[z].mubar;
            if (outcome[z].status != CIP_STATUS_NONE) active &= ~(1ull << z);
        }
        if (!active) break;
        mask.set(active);

        // ------------------------------------------------------------ predictor (:879-887)
        CK(cip_solve4x4_dev(h, lam, r0.base, daff.base)); count(n_solve, active);
        for (int z = 0; z < B; ++z) sigma[z] = 0.0;
        if (m > 0) {
            // one host round trip for the pair of max-steps and the four dot products: the minima ride on the dots' read-back
            CK(maxstep_pair(zv.v, daff.v, zv.s, daff.s, 1.0, false));
            const double *qx[4] = {zv.v, zv.v, daff.v, daff.v};
            const double *qy[4] = {zv.s, daff.s, zv.s, daff.s};
            const int ql[4] = {m, m, m, m};
            CK(cip_dots_dev(h, 4, qx, qy, ql, q4.data()));
            for (int z = 0; z < B; ++z) {
                if (!((active >> z) & 1ull)) continue;
                const double a_aff = std::fmin(std::fmin(pair(z)[0], 1.0), pair(z)[1]);
                const double *q = &q4[(size_t)z * 4];
                const double rho = (q[0] - a_aff * q[1] - a_aff * q[2] + a_aff * a_aff * q[3]) / mubar[z];   // fts :162-163, :886
                const double cl = std::fmax(0.0, std::fmin(1.0, rho));
                sigma[z] = std::pow(cl, 3.0);      // as the Python driver's `** 3` (the two drivers agree to the last bit)
            }
        }

        // ------------------------------------------------------------ corrector (:893-901)
        // r = r0 ; r.s += (F^-T d_aff.s) o (F d_aff.v) - sigma mu e     -- one kernel (vecops.hip: k_loop_corr); the cone operations in
        // front of it unless every cone is an R cone
        if (m > 0 && !f) {
            CK(cip_apply_F_dev(h, CIP_OP_FINVT, daff.s, mb1));                         // F^-T d_aff.s
            CK(cip_apply_F_dev(h, CIP_OP_F, daff.v, mb2));                             // F d_aff.v
            CK(cip_cone_prod_dev(h, mb1, mb2, mb3));
        }
        if (m > 0) {
            for (int z = 0; z < B; ++z) tmp[z] = sigma[z] * mu[z];
            CK(cip_loop_corr(s, n, m, p, r0.base, daff.base, mb3, e, f, tmp.data(), r.base));
        } else CK(cip_axpby(s, NT, 1.0, r0.base, 0.0, r.base));

        // ------------------------------------------------------------ Newton step + refinement (:907-921)
        CK(cip_solve4x4_dev(h, lam, r.base, dz.base)); count(n_solve, active);
        unsigned long long refine = active;
        bool step_known = false;
        for (int it = 0; it < o.maxRefinementSteps && refine; ++it) {
            mask.set(refine);
            // rkkt = K dz (mat-vecs), then rkkt.v -= dz.s, rkkt.s = lam o (F dz.v) + lam o (F^-T dz.s), rIr = r - rkkt: one kernel
            // (vecops.hip: k_loop_refine)
            CK(cip_gemv_dev(h, CIP_MAT_Q, 0, 1.0, dz.y, 0.0, rkkt.y));
            if (p > 0) {
                CK(cip_gemv_dev(h, CIP_MAT_G, 1, 1.0, dz.w, 1.0, rkkt.y));
                CK(cip_gemv_dev(h, CIP_MAT_G, 0, 1.0, dz.y, 0.0, rkkt.w));
            }
            if (m > 0) {
                CK(cip_gemv_dev(h, CIP_MAT_A, 1, -1.0, dz.v, 1.0, rkkt.y));
                CK(cip_gemv_dev(h, CIP_MAT_A, 0, 1.0, dz.y, 0.0, rkkt.v));
                if (!f) {
                    CK(cip_apply_F_dev(h, CIP_OP_F, dz.v, mb1));
                    CK(cip_cone_prod_dev(h, lam, mb1, mb2));
                    CK(cip_apply_F_dev(h, CIP_OP_FINVT, dz.s, mb1));
                    CK(cip_cone_prod_dev(h, lam, mb1, mb3));
                }
            }
            CK(cip_loop_refine(s, n, m, p, rkkt.base, dz.base, r.base, lam, mb2, mb3, f, rIr.base));
            const double *nx[4] = {rIr.y, rIr.w, rIr.v, rIr.s};
            const int nl[4] = {n, p, m, m};
            // the step's two max-steps ride on the first refinement test's read-back: when no problem asks for refinement -- the usual
            // case -- dz is final and the iteration has saved a host round trip; otherwise they are taken again behind the loop
            const bool spec = it == 0 && m > 0;
            if (spec) CK(maxstep_pair(zv.v, dz.v, zv.s, dz.s, 1.0 / (1.0 - o.DTB), false));
            CK(cip_dots_dev(h, 4, nx, nx, nl, n2.data()));
            for (int z = 0; z < B; ++z) {
                if (!((refine >> z) & 1ull)) continue;
                const double *q = &n2[(size_t)z * 4];
                const double rnorm = (nrm(q[0]) + (p > 0 ? nrm(q[1]) : 0.0) + (m > 0 ? nrm(q[2]) + nrm(q[3]) : 0.0)) / (n + 2 * m);   // :917 (norm(v4x1) :61)
                if (rnorm < o.refinementThreshold) refine &= ~(1ull << z);
            }
            if (!refine) { step_known = spec; break; }
            mask.set(refine);
            CK(cip_solve4x4_dev(h, lam, rIr.base, dzr.base)); count(n_solve, refine);
            CK(cip_axpby(s, NT, 1.0, dzr.base, 1.0, dz.base));                        // :920
        }
        mask.set(active);

        // ------------------------------------------------------------ step (:927-932)
        for (int z = 0; z < B; ++z) alpha[z] = 1.0;
        if (m > 0) {
            if (!step_known) CK(maxstep_pair(zv.v, dz.v, zv.s, dz.s, 1.0 / (1.0 - o.DTB), true));
            for (int z = 0; z < B; ++z) alpha[z] = std::fmin(std::fmin(pair(z)[0], 1.0), std::fmin(pair(z)[1], 1.0));
        }
        for (int z = 0; z < B; ++z) tmp[z] = -alpha[z];
        CK(cip_axpby_ps(s, NT, tmp.data(), dz.base, 1.0, zv.base));
        if (tr) { tr[7] = alpha[0]; tr[8] = sigma[0]; }
    }
#undef CK
    for (int z = 0; z < B; ++z) {
        if ((active >> z) & 1ull) outcome[z].status = CIP_STATUS_ABANDONED;           // :936
        res[z].status = outcome[z].status; res[z].n_factor = n_factor[z]; res[z].n_solve = n_solve[z];
    }
    return 0;
}

namespace {

// One problem: the handle's own policy -- a bad pivot switches it to the regularised factorisation for good (api.hip:
// cip_factor_resolve); a dead (zero / non-finite) pivot even then is where the reference's LU hands back NaNs and the loop ends
// with :Error at its next residual check (src/ConicIP.jl:870-873)
struct OneProblem final : Loop {
    explicit OneProblem(cip_handle *h_) : Loop(h_, 1) {}
    int factor() override { return cip_factor(h); }
    int ride_pivots() override { return 0; }           // (cip_factor has enqueued their read-back)
    int take_pivots(bool) override {
        const int rc = cip_factor_resolve(h, true);
        if (rc != CIP_E_SINGULAR) return rc;
        outcome[0].status = CIP_STATUS_ERROR;
        active = 0;
        return 0;
    }
};

}   // namespace

extern "C" int cip_conicip(cip_handle *h, const double *c_host, const double *b_host, const double *d_host,
                           const cip_options *opt_in, double *y_out, double *w_out, double *v_out, cip_result *res,
                           double *trace, int trace_cap) {
    if (!h || !res || !c_host || (h->m > 0 && !b_host) || (h->p > 0 && !d_host) || !y_out || (h->p > 0 && !w_out) ||
        (h->m > 0 && !v_out)) { cip_set_error("cip_conicip: null argument"); return CIP_E_INVALID; }
    const auto t_start = std::chrono::steady_clock::now();
    const cip_options o = resolve_options(opt_in);
    CIP_HIP_CHECK(hipSetDevice(h->device));
    if (!h->drv) {
        void *ptr = nullptr;
        if (cip_handle_alloc(h, &ptr, cip_driver_bytes(h)) != 0) { cip_set_error("cip_conicip: device allocation failed"); return CIP_E_HIP; }
        h->drv = (double *)ptr;
    }
    OneProblem L(h);
    int rc;
    if ((rc = L.run(&c_host, &b_host, &d_host, o, res, trace, trace_cap))) return rc;
    const int n = h->n, m = h->m, p = h->p;
    CIP_HIP_CHECK(hipMemcpyAsync(y_out, L.V.z.y, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (p > 0) CIP_HIP_CHECK(hipMemcpyAsync(w_out, L.V.z.w, sizeof(double) * p, hipMemcpyDeviceToHost, h->stream));
    if (m > 0) CIP_HIP_CHECK(hipMemcpyAsync(v_out, L.V.z.v, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
    CIP_HIP_CHECK(hipStreamSynchronize(h->stream));
    res->wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    apply_certificate(L.outcome[0], n, m, p, y_out, w_out, v_out);
    return 0;
}
