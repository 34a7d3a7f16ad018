// TEST INFRASTRUCTURE (tests/test_ldlt_plan.py), one source, two stand-alone programs:
//
// plan_table (the default): includes conicip.jl_amd/csrc/cip_ldlt_plan.h and nothing else of the library.  Reads rows of fourteen integers
//     Npad  nbo nbo_auto tail chain side_prep side_from ls_panel_max ls_panel_cus  Bs B recording has_side unfused
// from standard input and prints for each what the plan makes of them, walking it the way ldlt.hip's block loop does:
//     widths=896,896,2816 fused=1 forks=1 groups=3072:0:6,4096:6:8,4608:8:9          (group: fork column : J0 : J1)
//
// plan_trace (-DPLAN_TRACE, linked against the host-only library and the fake HIP runtime of tests/hostsan): drives factorisations
// through the public C ABI alone -- so that it also builds against an older libcipkkt -- with the fake runtime's launch trace switched
// on, and leaves the trace in the file named on its command line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef PLAN_TRACE
#include "cip_ldlt_plan.h"

int main() {
    int v[14];
    for (;;) {
        for (int i = 0; i < 14; ++i)
            if (scanf("%d", &v[i]) != 1) return i == 0 ? 0 : 2;
        const LdltKnobs k{v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
        const LdltCtx x{v[0], v[9], v[10], v[11] != 0, v[12] != 0, v[13] != 0};
        const LdltPlan p = ldlt_plan(k, x);
        printf("widths=");
        for (int C0 = 0, w = 0; C0 < x.Npad; C0 += w) {
            w = p.width_at(C0);
            if (w <= 0 || w % 128) return 3;
            printf(C0 ? ",%d" : "%d", w);
        }
        printf(" fused=%d forks=%d groups=", (int)p.fused, (int)(p.fork_C0 >= 0));
        int Jdone = 0, n = 0;
        auto group = [&](int c) {
            const int J1 = p.next_fork(c, Jdone);
            if (!J1) return;
            printf(n++ ? ",%d:%d:%d" : "%d:%d:%d", c, Jdone, J1);
            Jdone = J1;
        };
        if (p.fork_C0 >= 0) {
            for (int c = p.fork_C0; c < x.Npad; c = (c / x.Bs + 1) * x.Bs) group(c);
            group(x.Npad);
        }
        printf("\n");
    }
}

#else
#include "cipkkt.h"

extern "C" int fake_hip_trace(const char *path);
extern "C" void fake_hip_trace_note(const char *text);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "plan_trace: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static void note(const char *fmt, int a = 0, int b = 0, int c = 0) {
    char buf[128];
    snprintf(buf, sizeof(buf), fmt, a, b, c);
    fake_hip_trace_note(buf);
}

static void standalone(int N, int chain, int nbo) {
    const int pc = cip_set_ldlt_fused_chain(chain);
    cip_set_ldlt_outer_block(nbo);
    size_t bytes = 0;
    REQUIRE(cip_ldlt_workspace_bytes(N, &bytes) == CIP_OK && bytes > 0);
    std::vector<double> K((size_t)N * N, 0.0), rhs(N, 1.0);
    for (int i = 0; i < N; ++i) K[i + (size_t)i * N] = 1.0;
    std::vector<char> ws(bytes);
    int info = -1;
    note("ldlt factor N %d chain %d nbo %d", N, chain, nbo);
    REQUIRE(cip_ldlt_factor_dev(nullptr, K.data(), N, N, ws.data(), &info) == CIP_OK);
    note("ldlt solve N %d chain %d nbo %d", N, chain, nbo);
    REQUIRE(cip_ldlt_solve_dev(nullptr, K.data(), N, N, ws.data(), rhs.data()) == CIP_OK);
    note("end");
    cip_set_ldlt_outer_block(0);
    cip_set_ldlt_fused_chain(pc);
}

struct Qp {                   // min x'Qx/2 + c'x  s.t.  A x >= b on one R cone; Q diagonal, A dense
    int n, m;
    int ctype[1], cdim[1];
    std::vector<double> Q, A, c, b;
    Qp(int n_, int m_) : n(n_), m(m_), Q((size_t)n_ * n_, 0.0), A((size_t)m_ * n_, 0.0), c(n_, 1.0), b(m_, -1.0) {
        ctype[0] = CIP_CONE_R; cdim[0] = m;
        for (int i = 0; i < n; ++i) Q[i + (size_t)i * n] = 2.0;
        for (int i = 0; i < m; ++i) A[i + (size_t)i * m] = 1.0;
    }
    cip_problem desc() const {
        cip_problem pr;
        memset(&pr, 0, sizeof(pr));
        pr.n = n; pr.m = m; pr.p = 0; pr.ncones = 1; pr.cone_type = ctype; pr.cone_dim = cdim;
        pr.Q = Q.data(); pr.ldq = n; pr.A = A.data(); pr.lda = m; pr.ldg = 1; pr.route = CIP_ROUTE_SCHUR;
        return pr;
    }
};

static void handle(int n, int side) {
    const int ps = cip_set_ldlt_side_prep(side);
    Qp P(n, 8);
    cip_problem pr = P.desc();
    cip_handle *h = nullptr;
    REQUIRE(cip_create_ex(&pr, &h) == CIP_OK && h);
    REQUIRE(cip_set_scaling_identity(h) == CIP_OK);
    note("handle factor N %d side %d", n, side);
    REQUIRE(cip_factor(h) == CIP_OK);
    note("handle solve N %d side %d", n, side);
    std::vector<double> x(n, 1.0), y(1, 0.5), z(P.m, 0.25), dx(n), dy(1), dz(P.m);
    REQUIRE(cip_solve3x3(h, x.data(), y.data(), z.data(), dx.data(), dy.data(), dz.data()) == CIP_OK);
    note("end");
    REQUIRE(cip_destroy(h) == CIP_OK);
    cip_set_ldlt_side_prep(ps);
}

static void lockstep_pair(int n) {
    Qp P(n, 16);
    const cip_problem pr[2] = {P.desc(), P.desc()};
    const double *c[2] = {P.c.data(), P.c.data()}, *b[2] = {P.b.data(), P.b.data()}, *d[2] = {nullptr, nullptr};
    std::vector<double> y0(n), y1(n), v0(P.m), v1(P.m), w0(1), w1(1);
    double *y[2] = {y0.data(), y1.data()}, *v[2] = {v0.data(), v1.data()}, *w[2] = {w0.data(), w1.data()};
    cip_result res[2];
    cip_options o;
    o.optTol = 1e-6; o.DTB = 0.01; o.infeasTol = -1.0; o.refinementThreshold = -1.0;
    o.maxRefinementSteps = 3; o.maxIters = 1; o.verbose = 0;
    const int ps = cip_set_lockstep_split(1);
    note("lockstep N %d", n);
    REQUIRE(cip_conicip_lockstep(2, pr, c, b, d, &o, y, w, v, res) == CIP_OK);
    note("end");
    cip_set_lockstep_split(ps);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: plan_trace OUTPUT\n"); return 2; }
    remove(argv[1]);
    REQUIRE(fake_hip_trace(argv[1]) == 0);
    for (int N : {384, 1152, 2048, 4096, 4608})
        for (int chain : {0, 3})
            for (int nbo : {0, 512}) standalone(N, chain, nbo);
    handle(4608, 1);
    handle(4608, 0);
    lockstep_pair(2048);
    fake_hip_trace(nullptr);
    REQUIRE(cip_release_cached_memory() == CIP_OK);
    printf("plan_trace: ok\n");
    return 0;
}
#endif
