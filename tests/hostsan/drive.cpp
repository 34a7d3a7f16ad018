// TEST INFRASTRUCTURE: drives the product's host control plane (libcipkkt built host-only under ASan + UBSan or TSan, linked against
// tests/hostsan/fake_hip.cpp) through the C ABI of include/cipkkt.h:
//   1. the plugin levels on one handle (create, identity scaling, factor, check, host-pointer solves, every many-column entry point at 1
//      and 65 right-hand sides, solve4x4, the refined solves of a regularised factor -- with n_solve counted as include/cipkkt.h says --,
//      packed scaling, destroy), dense and CSR A, p = 0 and p > 0, both routes;
//   2. the native loop (cip_conicip) on a handle, with a trace buffer;
//   3. cip_conicip_mixed on a batch built to hit every branch of the binning: 65 problems of one shape (a lock-step group of 64 and a
//      group of ONE -- round 4's NULL write lived there), CSR problems of equal shape but different nnz, problems with p > 0, a
//      problem with a chip-wide S cone (lock-step refuses it: thread pool), and a batch holding an S cone beyond the envelope
//      (refused at level 1: the call must fail cleanly and free everything);
//      and the worker pool alone (cip_batch_conicip, cip_conicip_many, cip_conicip_problems), a failing problem among sound ones included;
//   4. the same entry points from several caller threads at once (thread-local batch contexts, the cached arena, the pool);
//   5. the stand-alone LDL' entry points with a caller-owned workspace in both solve modes, and their refusals of bad arguments;
//   6. the handle's device block: one "device" allocation per handle (two with a chip-wide S cone), lock-step calls of one shape
//      under changing solve modes, and -- `drive slab K`, a fresh process per case -- the slab sizes of every branch of the layout.
// At the end every "device" allocation must have been returned (the fake runtime counts them).
#include "cipkkt.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
extern "C" long fake_hip_device_allocs(void);

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

struct Prob {
    int n, m, p;
    std::vector<int> ctype, cdim;
    std::vector<double> Q, A, G, c, b, d, Av;
    std::vector<int> rp, ci, qrp, qci;
    std::vector<double> qv;
    bool csr = false, qcsr = false;
    int route = CIP_ROUTE_SCHUR;
    cip_problem desc() const {
        cip_problem pr;
        memset(&pr, 0, sizeof(pr));
        pr.n = n; pr.m = m; pr.p = p; pr.ncones = (int)ctype.size();
        pr.cone_type = ctype.data(); pr.cone_dim = cdim.data();
        pr.Q = Q.data(); pr.ldq = n;
        if (csr) { pr.A = nullptr; pr.A_rowptr = rp.data(); pr.A_colind = ci.data(); pr.A_val = Av.data(); }
        else { pr.A = A.data(); pr.lda = m; }
        pr.G = p > 0 ? G.data() : nullptr; pr.ldg = p > 0 ? p : 1;
        pr.route = route; pr.flags = 0;
        if (qcsr) { pr.Q = nullptr; pr.Q_rowptr = qrp.data(); pr.Q_colind = qci.data(); pr.Q_val = qv.data(); pr.flags |= CIP_FLAG_Q_CSR; }
        return pr;
    }
};
static thread_local unsigned long long g_rng = 88172645463325252ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng % 20001) / 10000.0 - 1.0; }

// n variables, cones given as (type, dim) pairs; density < 1 -> CSR with roughly that share of entries (at least the diagonal)
static Prob make(int n, int p, std::vector<std::pair<int, int>> cones, double density, int route = CIP_ROUTE_SCHUR) {
    Prob P;
    P.n = n; P.p = p; P.route = route;
    P.m = 0;
    for (auto &c : cones) { P.ctype.push_back(c.first); P.cdim.push_back(c.second); P.m += c.second; }
    P.Q.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) P.Q[i + (size_t)i * n] = 2.0 + 0.1 * i;
    P.c.resize(n); for (auto &x : P.c) x = rnd();
    P.b.assign(P.m, -1.0);
    P.d.assign(p, 0.0);
    P.G.resize((size_t)p * n); for (auto &x : P.G) x = rnd();
    if (density >= 1.0) {
        P.A.resize((size_t)P.m * n); for (auto &x : P.A) x = 0.3 * rnd();
    } else {
        P.csr = true;
        P.rp.push_back(0);
        for (int i = 0; i < P.m; ++i) {
            for (int j = 0; j < n; ++j)
                if (j == i % n || (rnd() + 1.0) * 0.5 < density) { P.ci.push_back(j); P.Av.push_back(0.3 * rnd() + (j == i % n ? 1.0 : 0.0)); }
            P.rp.push_back((int)P.ci.size());
        }
    }
    return P;
}

static cip_options opts() {
    cip_options o;
    o.optTol = 1e-6; o.DTB = 0.01; o.infeasTol = -1.0; o.refinementThreshold = -1.0;
    o.maxRefinementSteps = 3; o.maxIters = 100; o.verbose = 0;
    return o;
}

static void plugin_levels(const Prob &P) {
    cip_problem pr = P.desc();
    cip_handle *h = nullptr;
    REQUIRE(cip_create_ex(&pr, &h) == CIP_OK && h);
    int N = 0, Np = 0;
    REQUIRE(cip_kkt_order(h, &N, &Np) == CIP_OK && N > 0 && Np >= N && Np % 128 == 0);
    REQUIRE(cip_set_scaling_identity(h) == CIP_OK);
    REQUIRE(cip_factor(h) == CIP_OK);
    REQUIRE(cip_check_factor(h) == CIP_OK);
    std::vector<double> x(P.n, 1.0), y(P.p > 0 ? P.p : 1, 0.5), z(P.m, 0.25), dx(P.n), dy(P.p > 0 ? P.p : 1), dz(P.m);
    const bool schur = P.route == CIP_ROUTE_SCHUR;
    REQUIRE(cip_solve3x3(h, x.data(), y.data(), z.data(), dx.data(), dy.data(), dz.data()) == CIP_OK);
    REQUIRE(cip_solve2x2(h, x.data(), y.data(), dx.data(), dy.data()) == (schur ? CIP_OK : CIP_E_UNSUPPORTED));
    {   // 65 right-hand sides: a full chunk and a chunk of one through the handle's many-column buffers and their host staging
        const int k = 65;
        std::vector<double> X((size_t)P.n * k, 1.0), Y(y.size() * k, 0.5), Z((size_t)P.m * k, 0.25), DX(X.size()), DY(Y.size()), DZ(Z.size());
        REQUIRE(cip_solve3x3_many(h, k, X.data(), Y.data(), Z.data(), DX.data(), DY.data(), DZ.data()) == CIP_OK);
        // 63: a chunk one column short of the staging buffer's 64 (on the tiny problem of main(): the blocks of the staging view must
        // stay inside the allocation that was sized for 64 columns)
        REQUIRE(cip_solve3x3_many(h, 63, X.data(), Y.data(), Z.data(), DX.data(), DY.data(), DZ.data()) == CIP_OK);
        // the other many-column entry points, a single column (the single entry point) and 65 (the "device" pointers are host memory here)
        for (int nr : {1, k}) {
            REQUIRE(cip_solve2x2_many(h, nr, X.data(), Y.data(), DX.data(), DY.data()) == (schur ? CIP_OK : CIP_E_UNSUPPORTED));
            REQUIRE(cip_solve3x3_many_dev(h, nr, X.data(), Y.data(), Z.data(), DX.data(), DY.data(), DZ.data()) == CIP_OK);
            REQUIRE(cip_solve2x2_many_dev(h, nr, X.data(), Y.data(), DX.data(), DY.data()) == (schur ? CIP_OK : CIP_E_UNSUPPORTED));
        }
    }
    std::vector<double> lam(P.m, 1.0), r4((size_t)P.n + P.p + 2 * P.m, 1.0), dz4(r4.size());
    REQUIRE(cip_solve4x4_dev(h, lam.data(), r4.data(), dz4.data()) == CIP_OK);
    // a regularised factor: the refined solves carve the handle's refinement buffers on first use
    REQUIRE(cip_set_regularization(h, 1e-13, 0) == CIP_OK);
    REQUIRE(cip_factor(h) == CIP_OK);
    REQUIRE(cip_solve3x3(h, x.data(), y.data(), z.data(), dx.data(), dy.data(), dz.data()) == CIP_OK);
    if (schur) REQUIRE(cip_solve2x2(h, x.data(), y.data(), dx.data(), dy.data()) == CIP_OK);
    REQUIRE(cip_solve4x4_dev(h, lam.data(), r4.data(), dz4.data()) == CIP_OK);
    {   // n_solve by the rule of include/cipkkt.h -- one per single solve, nrhs per many-column call, none for a refused call -- from
        // the calls above: on the plain factor solve3x3, [solve2x2], solve3x3_many(65), solve3x3_many(63), then for nrhs = 1 and 65
        // [solve2x2_many], solve3x3_many_dev, [solve2x2_many_dev], and solve4x4; on the regularised one solve3x3, [solve2x2], solve4x4.
        // [Schur route only]
        const int two2 = schur ? 1 : 0;
        const int expect = (1 + two2 + 65 + 63 + (1 + 65) * (two2 + 1 + two2) + 1) + (1 + two2 + 1);
        double st[8];
        REQUIRE(cip_stats(h, st) == CIP_OK);
        if ((int)st[1] != expect) fprintf(stderr, "drive: n_solve is %d, the call list gives %d\n", (int)st[1], expect);
        REQUIRE((int)st[1] == expect);
    }
    REQUIRE(cip_set_regularization(h, 0.0, 1) == CIP_OK);
    REQUIRE(cip_factor(h) == CIP_OK);
    const size_t len = cip_scaling_packed_len(h);
    std::vector<double> F(len ? len : 1);
    REQUIRE(cip_get_scaling_packed(h, F.data()) == CIP_OK);
    REQUIRE(cip_set_scaling_packed(h, F.data()) == CIP_OK);
    REQUIRE(cip_set_timing(h, 1) == CIP_OK);
    REQUIRE(cip_factor(h) == CIP_OK);
    double st[8];
    REQUIRE(cip_stats(h, st) == CIP_OK);
    REQUIRE(cip_set_timing(h, 0) == CIP_OK);
    std::vector<double> K((size_t)Np * Np);
    REQUIRE(cip_get_kkt_matrix(h, K.data()) == CIP_OK);
    REQUIRE(cip_update_problem(h, &pr) == CIP_OK);
    // the native loop on the same handle, with a trace
    cip_options o = opts();
    cip_result res;
    std::vector<double> yy(P.n), ww(P.p > 0 ? P.p : 1), vv(P.m), trace(CIP_TRACE_COLS * 8);
    REQUIRE(cip_conicip(h, P.c.data(), P.b.data(), P.p > 0 ? P.d.data() : nullptr, &o, yy.data(), ww.data(), vv.data(), &res, trace.data(), 8) == CIP_OK);
    REQUIRE(res.status >= CIP_STATUS_OPTIMAL && res.status <= CIP_STATUS_ERROR && res.n_factor >= 1);
    REQUIRE(cip_destroy(h) == CIP_OK);
}

struct Batch {
    std::vector<Prob> P;
    std::vector<cip_problem> desc;
    std::vector<const double *> c, b, d;
    std::vector<std::vector<double>> y, w, v;
    std::vector<double *> yp, wp, vp;
    std::vector<cip_result> res;
    void finish() {
        const size_t k = P.size();
        desc.resize(k); c.resize(k); b.resize(k); d.resize(k); y.resize(k); w.resize(k); v.resize(k); yp.resize(k); wp.resize(k); vp.resize(k); res.resize(k);
        for (size_t i = 0; i < k; ++i) {
            desc[i] = P[i].desc(); c[i] = P[i].c.data(); b[i] = P[i].b.data(); d[i] = P[i].p > 0 ? P[i].d.data() : nullptr;
            y[i].assign(P[i].n, 777.0); w[i].assign(P[i].p > 0 ? P[i].p : 1, 777.0); v[i].assign(P[i].m, 777.0);
            yp[i] = y[i].data(); wp[i] = w[i].data(); vp[i] = v[i].data();
            memset(&res[i], 0, sizeof(cip_result));
        }
    }
};

static Batch mixed_batch(int same_shape, bool with_large_s) {
    Batch B;
    for (int i = 0; i < same_shape; ++i) B.P.push_back(make(8, 0, {{CIP_CONE_R, 8}}, 1.0));                 // 65 -> groups of 64 and 1
    for (int i = 0; i < 3; ++i) B.P.push_back(make(10, 0, {{CIP_CONE_R, 6}, {CIP_CONE_Q, 4}}, 0.2 + 0.25 * i));   // equal shapes, different nnz
    for (int i = 0; i < 2; ++i) B.P.push_back(make(12, 3, {{CIP_CONE_R, 5}, {CIP_CONE_Q, 5}, {CIP_CONE_S, 6}}, 1.0));   // p > 0, a small S cone
    B.P.push_back(make(9, 0, {{CIP_CONE_R, 9}}, 1.0, CIP_ROUTE_FULL3X3));                                    // a bin of one: thread pool
    if (with_large_s) B.P.push_back(make(4, 0, {{CIP_CONE_S, 133 * 134 / 2}}, 1.0));                          // chip-wide S cone: lock-step refuses it
    B.finish();
    return B;
}

static void run_mixed(int same_shape, bool with_large_s, int in_flight) {
    Batch B = mixed_batch(same_shape, with_large_s);
    cip_options o = opts();
    const int k = (int)B.P.size();
    REQUIRE(cip_conicip_mixed(k, B.desc.data(), B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data(), in_flight) == CIP_OK);
    for (int i = 0; i < k; ++i) {
        REQUIRE(B.res[i].status >= CIP_STATUS_OPTIMAL && B.res[i].status <= CIP_STATUS_ERROR);
        REQUIRE(B.y[i][0] != 777.0);                               // every problem's solution was written
    }
    int st[3];
    REQUIRE(cip_lockstep_stats(st) == CIP_OK && st[1] >= same_shape);
    // the same problems through the two other batch entry points
    REQUIRE(cip_conicip_problems(k, B.desc.data(), B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data(), in_flight) == CIP_OK);
    cip_batch *bt = nullptr;
    REQUIRE(cip_batch_create(k, B.desc.data(), &bt) == CIP_OK && cip_batch_size(bt) == k);
    REQUIRE(cip_batch_conicip(bt, B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data(), in_flight) == CIP_OK);
    REQUIRE(cip_batch_destroy(bt) == CIP_OK);
}

static void refused_batch(void) {
    // an S cone of matrix order 2049 (vectorised length 2049 * 2050 / 2): refused at level 1 from the cone table alone -- A is never read
    Batch B;
    B.P.push_back(make(8, 0, {{CIP_CONE_R, 8}}, 1.0));
    B.P.push_back(make(8, 0, {{CIP_CONE_R, 8}}, 1.0));
    B.finish();
    Prob big;
    big.n = 2; big.p = 0; big.m = 2049 * 2050 / 2;
    big.ctype = {CIP_CONE_S}; big.cdim = {big.m};
    big.Q = {1.0, 0.0, 0.0, 1.0}; big.A.assign(4, 0.0); big.c = {1.0, 1.0}; big.b.assign(4, 0.0);
    cip_problem pd = big.desc();
    cip_handle *h = nullptr;
    REQUIRE(cip_create_ex(&pd, &h) == CIP_E_UNSUPPORTED && h == nullptr);
    std::vector<cip_problem> desc = B.desc;
    desc.push_back(pd);
    std::vector<const double *> c = B.c, b = B.b, d = B.d;
    c.push_back(big.c.data()); b.push_back(big.b.data()); d.push_back(nullptr);
    std::vector<double> y3(2, 777.0), w3(1, 777.0), v3(4, 777.0);
    std::vector<double *> yp = B.yp, wp = B.wp, vp = B.vp;
    yp.push_back(y3.data()); wp.push_back(w3.data()); vp.push_back(v3.data());
    std::vector<cip_result> res(3);
    cip_options o = opts();
    const int rc = cip_conicip_mixed(3, desc.data(), c.data(), b.data(), d.data(), &o, yp.data(), wp.data(), vp.data(), res.data(), 2);
    REQUIRE(rc != CIP_OK);                                         // the refusal surfaces; nothing leaks (checked at the end)
    REQUIRE(y3[0] == 777.0);
}

// ---- the worker pool of batch.hip on three problems of the smallest shape: handles built once (cip_batch_create, cip_batch_conicip,
// cip_conicip_many) and problems in (cip_conicip_problems), with every problem sound and with the middle one failing -- once with one
// worker (the failure is the calling thread's) and once with more (it may be another thread's)
static Batch three_small(int middle_cone_dim = 5) {
    Batch B;
    for (int i = 0; i < 3; ++i) B.P.push_back(make(6, 1, {{CIP_CONE_R, 5}, {CIP_CONE_Q, 3}}, 1.0));
    B.P[1].cdim[0] = middle_cone_dim;                              // (another value: the cone list no longer covers m = 8)
    B.finish();
    return B;
}
static void poison(Batch &B) { for (auto &r : B.res) memset(&r, 0x5a, sizeof(cip_result)); }
static bool final_status(const cip_result &r) { return r.status >= CIP_STATUS_OPTIMAL && r.status <= CIP_STATUS_ERROR; }
static void middle_failed(int rc, const Batch &B) {
    REQUIRE(rc != CIP_OK);
    REQUIRE(!strncmp(cip_last_error(), "problem failed:", 15));
    REQUIRE(B.res[1].status == CIP_STATUS_ERROR);
    REQUIRE(final_status(B.res[0]) && final_status(B.res[2]));     // reached: no longer the poison
}
static void pool_cases(void) {
    cip_options o = opts();
    {
        Batch B = three_small();
        cip_batch *bt = nullptr;
        REQUIRE(cip_batch_create(3, B.desc.data(), &bt) == CIP_OK && cip_batch_size(bt) == 3);
        for (int in_flight : {1, 3}) {
            poison(B);
            REQUIRE(cip_batch_conicip(bt, B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data(), in_flight) == CIP_OK);
            for (const auto &r : B.res) REQUIRE(final_status(r));
        }
        // a NULL c: refused by cip_conicip, hence a failed problem of cip_conicip_many
        cip_handle *hs[3] = {cip_batch_handle(bt, 0), cip_batch_handle(bt, 1), cip_batch_handle(bt, 2)};
        REQUIRE(cip_conicip(hs[1], nullptr, B.b[1], B.d[1], &o, B.yp[1], B.wp[1], B.vp[1], &B.res[1], nullptr, 0) == CIP_E_INVALID);
        B.c[1] = nullptr;
        for (int in_flight : {1, 2}) {
            poison(B);
            middle_failed(cip_conicip_many(hs, 3, B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data(), in_flight), B);
        }
        REQUIRE(cip_batch_destroy(bt) == CIP_OK);
    }
    Batch B = three_small(4);                                      // level 1 refuses the middle problem
    for (int in_flight : {1, 2}) {
        poison(B);
        middle_failed(cip_conicip_problems(3, B.desc.data(), B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data(), in_flight), B);
    }
}

static void standalone_ldlt(void) {
    const int N = 384;
    size_t bytes = 0;
    for (int mode = 0; mode <= 2; mode += 2) {
        const int prev = cip_set_solve_fused(mode);
        const int pb = cip_set_solve_block_max(128);
        REQUIRE(cip_ldlt_workspace_bytes(N, &bytes) == CIP_OK && bytes > 0);
        std::vector<double> K((size_t)N * N, 0.0), rhs(N, 1.0);
        for (int i = 0; i < N; ++i) K[i + (size_t)i * N] = 1.0;
        std::vector<char> ws(bytes);                               // caller-owned workspace of EXACTLY the advertised size
        int info = -1;
        REQUIRE(cip_ldlt_factor_dev(nullptr, K.data(), N, N, ws.data(), &info) == CIP_OK);
        REQUIRE(cip_ldlt_solve_dev(nullptr, K.data(), N, N, ws.data(), rhs.data()) == CIP_OK);
        cip_set_solve_block_max(pb);
        cip_set_solve_fused(prev);
    }
    // refusals (include/cipkkt.h): a leading dimension below the order or not a multiple of 128, NULL pointers -- CIP_E_INVALID from
    // the host-side check, with nothing enqueued (the buffers are large enough for every stride tried, should one get through)
    long l0, l1, e, b, a;
    std::vector<double> K((size_t)(N + 128) * (N + 128), 0.0), rhs(N + 128, 1.0);
    std::vector<char> ws(bytes);
    int info = -1;
    fake_hip_stats(&l0, &e, &b, &a);
    for (int ld : {N - 128, N + 64, N + 2, N - 1, 0, -N}) {
        REQUIRE(cip_ldlt_factor_dev(nullptr, K.data(), N, ld, ws.data(), &info) == CIP_E_INVALID);
        REQUIRE(cip_ldlt_solve_dev(nullptr, K.data(), N, ld, ws.data(), rhs.data()) == CIP_E_INVALID);
    }
    REQUIRE(cip_ldlt_factor_dev(nullptr, nullptr, N, N, ws.data(), &info) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_factor_dev(nullptr, K.data(), N, N, nullptr, &info) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_dev(nullptr, nullptr, N, N, ws.data(), rhs.data()) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_dev(nullptr, K.data(), N, N, nullptr, rhs.data()) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_dev(nullptr, K.data(), N, N, ws.data(), nullptr) == CIP_E_INVALID);
    const int M = 256, Nn = 128, Kk = 16;                            // A: M x Kk, B: Nn x Kk, C: M x Nn
    double *A = K.data(), *B = K.data(), *C = K.data();
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M - 1, B, Nn, C, M, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M, B, Nn - 16, C, M, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M, B, Nn, C, M - 128, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, nullptr, M, B, Nn, C, M, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M, nullptr, Nn, C, M, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M, B, Nn, nullptr, M, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, 0, 1.0, A, M, B, Nn, C, M, 0) == CIP_E_INVALID);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M, B, Nn, C, M, 1) == CIP_E_INVALID);      // lower_only needs M == N
    fake_hip_stats(&l1, &e, &b, &a);
    REQUIRE(l1 == l0);
    // the valid strides of the same calls go through
    REQUIRE(cip_ldlt_factor_dev(nullptr, K.data(), N, N + 128, ws.data(), &info) == CIP_OK);
    REQUIRE(cip_gemm_nt_dev(nullptr, M, Nn, Kk, 1.0, A, M + 16, B, Nn + 2, C, M + 128, 0) == CIP_OK);
}

// ---- the handle's device block and the lock-step slab (api.hip: handle_layout; lockstep.hip: lockstep_group)
static int lockstep(Batch &B, int max_iters) {
    cip_options o = opts();
    o.maxIters = max_iters;
    return cip_conicip_lockstep((int)B.P.size(), B.desc.data(), B.c.data(), B.b.data(), B.d.data(), &o, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data());
}
static Batch pair_of(const Prob &a, const Prob &b) { Batch B; B.P = {a, b}; B.finish(); return B; }

// A cip_set_solve_fused between two lock-step calls of one shape changes what the handles' LDL' workspace holds (two solve blocks: the
// pre-multiplied neighbour blocks), hence the slab: every call must size its slabs for the mode it runs under.
static void knob_sequence(void) {
    const int pb = cip_set_solve_block_max(128), ps = cip_set_lockstep_split(1), pf = cip_set_solve_fused(-1), pc = cip_set_ldlt_fused_chain(-1);
    for (int mode : {0, 2, 0}) {
        cip_set_solve_fused(mode);
        cip_set_ldlt_outer_block(mode ? 128 : 0); cip_set_ldlt_fused_chain(mode ? 0 : 3);      // the factorisation's plan: a new one per call
        Batch B = pair_of(make(200, 0, {{CIP_CONE_R, 200}}, 1.0), make(200, 0, {{CIP_CONE_R, 200}}, 1.0));
        REQUIRE(lockstep(B, 1) == CIP_OK);
        for (auto &y : B.y) REQUIRE(y[0] != 777.0);
    }
    cip_set_solve_fused(pf); cip_set_lockstep_split(ps); cip_set_solve_block_max(pb); cip_set_ldlt_fused_chain(pc);
}

// One device allocation per handle (two with a chip-wide S cone, whose workspace keeps its own), none after destruction.
static void allocation_count(const Prob &P, long expect) {
    cip_problem pr = P.desc();
    cip_handle *h = nullptr;
    const long before = fake_hip_device_allocs();
    REQUIRE(cip_create_ex(&pr, &h) == CIP_OK && h);
    const long held = fake_hip_device_allocs() - before;
    if (held != expect) fprintf(stderr, "drive: the handle holds %ld device allocations, expected %ld\n", held, expect);
    REQUIRE(held == expect);
    REQUIRE(cip_destroy(h) == CIP_OK);
    REQUIRE(fake_hip_device_allocs() == before);
}

// `drive slab K`, a fresh process per case: what is live right after the first two-problem lock-step call (split 1) -- the arena of two
// slabs and the gather rows, the group's pinned gather rows and the thread's 4-KB pinned scratch.  The expected figures were recorded
// with this program from the library as it stood when every handle was created twice, once to be measured and once in its slab: a
// slab is sized by the walk that carves it now, and must come out at the same number of bytes.
struct SlabCase { const char *what; long expect; };
static const SlabCase slab_cases[] = {
    {"dense A, R cone, n = m = 200, solve block 128", 10722816},
    {"dense A, R cone, n = m = 1024", 124857856},
    {"dense A, R cone, n = m = 1152: nine solve blocks", 136332800},
    {"p > 0, R + Q + S cones, Schur route", 3651072},
    {"p > 0, R + Q + S cones, literal 3x3 route", 3618304},
    {"CSR A, R + Q cones", 3597824},
    {"CSR A, R + S cones, Schur route", 3682816},
    {"CSR Q", 3626496},
    {"p > 0, R + Q cones, regularised problems stay in their group", 3630592},
    {"dense A, n = 2048: symv tables", 217748992},
    {"dense A, n = 128, m = 4096: split-K images of the Schur formation", 35229184},
    {"dense A, R cone, n = m = 1152, one-launch block steps", 141051392},
};
static Batch slab_batch(int k) {
    auto two = [](int n, int p, std::vector<std::pair<int, int>> cones, double density, int route = CIP_ROUTE_SCHUR) {
        Prob a = make(n, p, cones, density, route);
        return pair_of(a, a);                                    // (one CSR pattern: equal nnz)
    };
    switch (k) {
    case 0: cip_set_solve_block_max(128); return two(200, 0, {{CIP_CONE_R, 200}}, 1.0);
    case 1: return two(1024, 0, {{CIP_CONE_R, 1024}}, 1.0);
    case 2: return two(1152, 0, {{CIP_CONE_R, 1152}}, 1.0);
    case 3: return two(12, 3, {{CIP_CONE_R, 5}, {CIP_CONE_Q, 5}, {CIP_CONE_S, 6}}, 1.0);
    case 4: return two(12, 3, {{CIP_CONE_R, 5}, {CIP_CONE_Q, 5}, {CIP_CONE_S, 6}}, 1.0, CIP_ROUTE_FULL3X3);
    case 5: return two(10, 0, {{CIP_CONE_R, 6}, {CIP_CONE_Q, 4}}, 0.4);
    case 6: return two(12, 0, {{CIP_CONE_R, 5}, {CIP_CONE_S, 6}}, 0.4);
    case 7: {
        Prob a = make(9, 0, {{CIP_CONE_R, 9}}, 1.0);
        a.qcsr = true;
        for (int i = 0; i < a.n; ++i) { a.qrp.push_back(i); a.qci.push_back(i); a.qv.push_back(a.Q[i + (size_t)i * a.n]); }
        a.qrp.push_back(a.n);
        return pair_of(a, a);
    }
    case 8: cip_set_lockstep_regularize(1); return two(10, 2, {{CIP_CONE_R, 4}, {CIP_CONE_Q, 6}}, 1.0);
    case 9: return two(2048, 0, {{CIP_CONE_R, 16}}, 1.0);
    case 10: return two(128, 0, {{CIP_CONE_R, 4096}}, 1.0);
    default: cip_set_solve_fused(2); return two(1152, 0, {{CIP_CONE_R, 1152}}, 1.0);
    }
}
static int slab_main(int k) {
    cip_set_lockstep_split(1);
    Batch B = slab_batch(k);
    REQUIRE(lockstep(B, 1) == CIP_OK);
    long launches, emulated, live_bytes, live_allocs;
    fake_hip_stats(&launches, &emulated, &live_bytes, &live_allocs);
    printf("drive: slab case %d (%s): %ld bytes live, expected %ld\n", k, slab_cases[k].what, live_bytes, slab_cases[k].expect);
    return live_bytes == slab_cases[k].expect ? 0 : 3;
}

int main(int argc, char **argv) {
    const int ncases = (int)(sizeof(slab_cases) / sizeof(slab_cases[0]));
    if (argc > 1 && !strcmp(argv[1], "slab")) {
        if (argc < 3) { printf("%d\n", ncases); return 0; }
        const int k = atoi(argv[2]);
        return k >= 0 && k < ncases ? slab_main(k) : 2;
    }
    const int nthreads = argc > 1 ? atoi(argv[1]) : 3;
    allocation_count(make(200, 0, {{CIP_CONE_R, 200}}, 1.0), 1);
    allocation_count(make(10, 2, {{CIP_CONE_R, 4}, {CIP_CONE_Q, 6}}, 0.4), 1);
    allocation_count(make(4, 0, {{CIP_CONE_S, 133 * 134 / 2}}, 1.0), 2);
    knob_sequence();
    plugin_levels(make(8, 0, {{CIP_CONE_R, 8}}, 1.0));
    plugin_levels(make(10, 2, {{CIP_CONE_R, 4}, {CIP_CONE_Q, 6}}, 0.4));
    plugin_levels(make(12, 3, {{CIP_CONE_R, 5}, {CIP_CONE_Q, 5}, {CIP_CONE_S, 6}}, 1.0, CIP_ROUTE_FULL3X3));
    plugin_levels(make(4, 0, {{CIP_CONE_S, 133 * 134 / 2}}, 1.0));
    plugin_levels(make(1, 0, {{CIP_CONE_R, 1}}, 1.0));               // n + p + m = 2: every staged block is a few doubles
    plugin_levels(make(3, 1, {{CIP_CONE_R, 1}}, 1.0));               // odd block lengths 3, 1, 1
    standalone_ldlt();
    run_mixed(65, true, 3);
    run_mixed(1, false, 1);
    pool_cases();
    refused_batch();
    // concurrent callers: every thread its own batches, all through the same process-wide state
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([t] {
            run_mixed(3 + 31 * t, t == 0, 2 + t);
            plugin_levels(make(8 + t, t % 2, {{CIP_CONE_R, 4}, {CIP_CONE_Q, 4 + t}}, t == 1 ? 0.5 : 1.0));
            REQUIRE(cip_release_cached_memory() == CIP_OK);
        });
    for (auto &x : th) x.join();
    REQUIRE(cip_release_cached_memory() == CIP_OK);
    long launches, emulated, live_bytes, live_allocs;
    fake_hip_stats(&launches, &emulated, &live_bytes, &live_allocs);
    printf("drive: %ld launches (%ld emulated), %ld device allocations / %ld bytes still live\n", launches, emulated, live_allocs, live_bytes);
    return 0;
}
