// The native interior-point loop (driver.hip), written once for B problems under a batch mask: cip_conicip runs it for one
// problem, a lock-step group (lockstep.hip) for B.  Here: the vector layout of the loop inside one device allocation and
// the loop itself (Loop).  The per-iteration scalar logic of src/ConicIP.jl:756-873 (residuals, best-iterate bookkeeping, objective
// values, stopping tests, certificates) is host-only and lives in cip_driver_scalars.h.
#pragma once
#include "cip_handle.h"
#include "cip_driver_scalars.h"
#include <vector>

namespace cipdrv {

struct Vec4 {          // (y[n], w[p], v[m], s[m]) stored contiguously
    double *base = nullptr, *y = nullptr, *w = nullptr, *v = nullptr, *s = nullptr;
};

// every vector of the loop, carved out of h->drv in a fixed order, each 256-byte aligned
struct Vectors {
    double *c_d, *b_d, *d_d;
    Vec4 z, r0, rleft, r, daff, dz, dzr, rIr, rkkt;
    double *e, *lam, *mb1, *mb2, *mb3, *Qy, *pinf, *Ays, *Gy;
    size_t carve(double *base, int n, int m, int p) {          // returns the bytes of the layout (base == NULL: sizing only)
        CipLayout L(base);
        const size_t NT = (size_t)n + p + 2 * (size_t)m;
        auto vec4 = [&]() { Vec4 v; if ((v.base = v.y = L.take<double>(NT))) { v.w = v.y + n; v.v = v.w + p; v.s = v.v + m; } return v; };
        c_d = L.take<double>(n); b_d = L.take<double>(m); d_d = L.take<double>(p);
        z = vec4(); r0 = vec4(); rleft = vec4(); r = vec4(); daff = vec4(); dz = vec4(); dzr = vec4(); rIr = vec4(); rkkt = vec4();
        e = L.take<double>(m); lam = L.take<double>(m); mb1 = L.take<double>(m); mb2 = L.take<double>(m); mb3 = L.take<double>(m);
        Qy = L.take<double>(n); pinf = L.take<double>(n); Ays = L.take<double>(m); Gy = L.take<double>(p);
        L.take<double>(32);               // tail: part of h->drv's size, which the lock-step arena's stride is built from
        return L.bytes();
    }
};

inline double cone_degree(const cip_handle *h) {      // conedim (:547-552)
    double conedim = 0;
    for (const ConeDesc &cd : h->h_cones) conedim += cd.type == CIP_CONE_R ? cd.dim : (cd.type == CIP_CONE_Q ? 1 : cd.r);
    return conedim;
}

inline unsigned long long full_mask(int B) { return B >= 64 ? ~0ull : ((1ull << B) - 1ull); }

// The iteration of src/ConicIP.jl:704-936 -- initial point, predictor, corrector, refinement, step, final status -- for the B problems
// of the calling thread's batch context, every step one launch for all of them (driver.hip: Loop::run).  Per-problem host state is
// problem-major, as cip_dots returns it; problem z takes part in a launch while bit z of `active` is set.  What a factorisation's
// pivot flags lead to is the caller's policy: in-loop regularisation and :Error for one problem (driver.hip: cip_conicip), leaving
// the group for a lock-step group (lockstep.hip).
struct Loop {
    cip_handle *h;                          // problem 0's handle (a group's other problems: the same pointers + z * stride)
    int B;
    unsigned long long active;              // problems still iterating
    std::vector<IterOutcome> outcome;       // final status of every problem, and what its certificate does to the iterate
    std::vector<int> n_factor, n_solve;
    int iters = 0;
    Vectors V;                              // carved out of h->drv; V.z holds every problem's last iterate when run() returns
    Loop(cip_handle *h_, int B_) : h(h_), B(B_), active(full_mask(B_)), outcome(B_), n_factor(B_, 0), n_solve(B_, 0) {}
    virtual ~Loop() = default;
    // c, b, d: problem z's data (host).  Fills res[z] but for wall_s; the caller downloads V.z and applies the certificates.
    int run(const double *const *c, const double *const *b, const double *const *d, const cip_options &o, cip_result *res,
            double *trace, int trace_cap);

  protected:
    virtual int factor() = 0;                  // enqueue assembly + LDL' of the active problems (:737 -> :682)
    virtual int ride_pivots() = 0;             // enqueue what brings their pivot flags back with the next read-back
    virtual int take_pivots(bool fresh) = 0;   // act on the flags (fresh: a read-back has just returned); problems that stop leave `active`
};

}   // namespace cipdrv
