// The host side of cip_conicip_small (include/cipkkt.h, csrc/small.hip), driven through the host-only build of the library linked
// against the fake HIP runtime of tests/hostsan/fake_hip.cpp, under AddressSanitizer / UBSan: every refusal comes before any "device"
// allocation and leaves the outputs alone; count 0, 1 and 200 run to the end with host and with "device" pointers; on the fake
// runtime's all-zero memory the loop ends by the verdict (zero residuals: Optimal at the first test) or by maxIters (Abandoned); the
// launch and read-back counts are those of the header; no allocation is left behind.
#include "cipkkt.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
extern "C" int hipMalloc(void **p, size_t bytes);
extern "C" int hipFree(void *p);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive_small: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static long live_allocs() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return a; }
static long launches() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return l; }

static const double SENTINEL = -7.25;

// `count` problems of one shape: an R cone and a Q cone beside it, equalities when p > 0
struct Batch {
    int count, n, m, p;
    std::vector<int> ctype, cdim;
    std::vector<double> Q, A, G, c, b, d, y, w, v;
    std::vector<cip_problem> pr;
    std::vector<const double *> cp, bp, dp;
    std::vector<double *> yp, wp, vp;
    std::vector<cip_result> res;
    std::vector<void *> dev;
    Batch(int count_, int n_, int m_, int p_, bool device = false) : count(count_), n(n_), m(m_), p(p_) {
        if (m >= 4) { ctype = {CIP_CONE_R, CIP_CONE_Q}; cdim = {m - 3, 3}; }
        else if (m > 0) { ctype = {CIP_CONE_R}; cdim = {m}; }
        Q.assign((size_t)n * n, 0.0); A.assign((size_t)m * n + 1, 0.5); G.assign((size_t)p * n + 1, 0.25);
        for (int i = 0; i < n; ++i) Q[i + (size_t)i * n] = 1.0;
        c.assign(n, 1.0); b.assign(m + 1, 1.0); d.assign(p + 1, 1.0);
        y.assign((size_t)count * n, SENTINEL); w.assign((size_t)count * p + 1, SENTINEL); v.assign((size_t)count * m + 1, SENTINEL);
        pr.resize(count); res.resize(count);
        void *dQ = nullptr, *dA = nullptr, *dG = nullptr;
        if (device) {
            REQUIRE(hipMalloc(&dQ, sizeof(double) * Q.size()) == 0); REQUIRE(hipMalloc(&dA, sizeof(double) * A.size()) == 0);
            REQUIRE(hipMalloc(&dG, sizeof(double) * G.size()) == 0);
            dev = {dQ, dA, dG};
        }
        for (int i = 0; i < count; ++i) {
            memset(&pr[i], 0, sizeof(cip_problem));
            pr[i].n = n; pr[i].m = m; pr[i].p = p; pr[i].ncones = (int)ctype.size(); pr[i].cone_type = ctype.data(); pr[i].cone_dim = cdim.data();
            pr[i].Q = device ? (double *)dQ : Q.data(); pr[i].ldq = n;
            pr[i].A = m > 0 ? (device ? (double *)dA : A.data()) : nullptr; pr[i].lda = m;
            pr[i].G = p > 0 ? (device ? (double *)dG : G.data()) : nullptr; pr[i].ldg = p;
            pr[i].route = CIP_ROUTE_SCHUR; pr[i].flags = device ? CIP_FLAG_DEVICE_PTRS : 0;
            cp.push_back(c.data()); bp.push_back(b.data()); dp.push_back(d.data());
            yp.push_back(y.data() + (size_t)i * n); wp.push_back(w.data() + (size_t)i * p); vp.push_back(v.data() + (size_t)i * m);
            memset(&res[i], 0x5a, sizeof(cip_result));
        }
    }
    ~Batch() { for (void *q : dev) hipFree(q); }
    int run(const cip_options *opt = nullptr) {
        return cip_conicip_small(count, pr.data(), cp.data(), m > 0 ? bp.data() : nullptr, p > 0 ? dp.data() : nullptr, opt, yp.data(),
                                 p > 0 ? wp.data() : nullptr, m > 0 ? vp.data() : nullptr, res.data());
    }
    bool untouched() const {
        for (size_t i = 0; i < (size_t)count * n; ++i) if (y[i] != SENTINEL) return false;
        for (size_t i = 0; i < (size_t)count * p; ++i) if (w[i] != SENTINEL) return false;
        for (size_t i = 0; i < (size_t)count * m; ++i) if (v[i] != SENTINEL) return false;
        const unsigned char *r = (const unsigned char *)res.data();
        for (size_t i = 0; i < sizeof(cip_result) * count; ++i) if (r[i] != 0x5a) return false;
        return true;
    }
};

// refused with `code` before any launch or allocation, the outputs untouched, the message holding `word`
static void refused(Batch &B, int code, const char *word, bool fits_too = false) {
    const long a0 = live_allocs(), l0 = launches();
    REQUIRE(B.run() == code);
    if (!strstr(cip_last_error(), word)) { fprintf(stderr, "drive_small: \"%s\" not in \"%s\"\n", word, cip_last_error()); exit(2); }
    REQUIRE(live_allocs() == a0 && launches() == l0);
    REQUIRE(B.untouched());
    if (fits_too) {          // the same answer for the single description
        REQUIRE(cip_conicip_small_fits(&B.pr[B.count - 1]) == code);
        REQUIRE(strstr(cip_last_error(), word) != nullptr);
    }
}

static void refusals() {
    { Batch B(3, 100, 8, 29); refused(B, CIP_E_UNSUPPORTED, "CIP_SMALL_MAX_N", true); }                       // n + p = 129
    { Batch B(2, 129, 8, 0); refused(B, CIP_E_UNSUPPORTED, "CIP_SMALL_MAX_N", true); }
    { Batch B(2, 4, 1025, 0); refused(B, CIP_E_UNSUPPORTED, "CIP_SMALL_MAX_M", true); }
    { Batch B(2, 6, 8, 1); B.ctype[1] = CIP_CONE_S; refused(B, CIP_E_UNSUPPORTED, "S cones", true); }
    { Batch B(2, 6, 8, 1); B.pr[1].route = CIP_ROUTE_FULL3X3; refused(B, CIP_E_UNSUPPORTED, "Schur route", true); }
    { Batch B(2, 6, 8, 1); B.pr[1].flags |= CIP_FLAG_Q_CSR; B.pr[1].Q = nullptr; refused(B, CIP_E_UNSUPPORTED, "CIP_FLAG_Q_CSR", true); }
    {
        Batch B(2, 6, 8, 1);
        std::vector<int> rp(9, 0), ci(1, 0); std::vector<double> av(1, 0.0);
        B.pr[1].A = nullptr; B.pr[1].A_rowptr = rp.data(); B.pr[1].A_colind = ci.data(); B.pr[1].A_val = av.data();
        refused(B, CIP_E_UNSUPPORTED, "CSR A", true);
    }
    { Batch B(2, 6, 8, 1); B.pr[1].n = 5; refused(B, CIP_E_UNSUPPORTED, "differs in shape"); }
    { Batch B(2, 6, 8, 1); std::vector<int> other = {6, 2}; B.pr[1].cone_dim = other.data(); refused(B, CIP_E_UNSUPPORTED, "differs in shape"); }
    // argument errors
    { Batch B(2, 6, 8, 1); B.cdim[0] = 4; refused(B, CIP_E_INVALID, "cones cover", true); }
    { Batch B(2, 6, 8, 1); B.pr[1].Q = nullptr; refused(B, CIP_E_INVALID, "Q is NULL", true); }
    { Batch B(2, 6, 8, 1); B.pr[1].G = nullptr; refused(B, CIP_E_INVALID, "G is NULL", true); }
    { Batch B(2, 6, 8, 1); B.pr[1].lda = 7; refused(B, CIP_E_INVALID, "leading dimension", true); }
    { Batch B(2, 6, 8, 1); B.bp[1] = nullptr; refused(B, CIP_E_INVALID, "null vector"); }
    { Batch B(2, 6, 8, 1); B.yp[0] = nullptr; REQUIRE(B.run() == CIP_E_INVALID); }
    { Batch B(2, 6, 8, 1); REQUIRE(cip_conicip_small(-1, B.pr.data(), B.cp.data(), B.bp.data(), B.dp.data(), nullptr, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data()) == CIP_E_INVALID); }
    { Batch B(2, 6, 8, 1); REQUIRE(cip_conicip_small(2, B.pr.data(), B.cp.data(), nullptr, B.dp.data(), nullptr, B.yp.data(), B.wp.data(), B.vp.data(), B.res.data()) == CIP_E_INVALID); REQUIRE(B.untouched()); }
    REQUIRE(cip_conicip_small_fits(nullptr) == CIP_E_INVALID);
    REQUIRE(cip_small_stats(nullptr) == CIP_E_INVALID);
    // the edges that are taken
    { Batch B(1, 100, 1024, 28); REQUIRE(cip_conicip_small_fits(&B.pr[0]) == CIP_OK); }
    { Batch B(1, 128, 0, 0); REQUIRE(cip_conicip_small_fits(&B.pr[0]) == CIP_OK); }
    // without rows A is never read: whether its pointer is NULL is no part of the shape (lock-step's rule, which refuses such a pair, is another)
    {
        Batch B(2, 3, 0, 1);
        B.pr[1].A = B.A.data();
        REQUIRE(B.pr[0].A == nullptr && B.run() == CIP_OK);
        for (int i = 0; i < 2; ++i) REQUIRE(B.res[i].status == CIP_STATUS_OPTIMAL && B.res[i].iter == 1);
    }
}

static void runs(int count, int n, int m, int p, bool device) {
    const long a0 = live_allocs();
    int st[4];
    {
        Batch B(count, n, m, p, device);
        const long a1 = live_allocs(), l0 = launches();
        REQUIRE(B.run() == CIP_OK);
        REQUIRE(live_allocs() == a1);
        REQUIRE(cip_small_stats(st) == CIP_OK);
        if (count == 0) { REQUIRE(launches() == l0 && st[0] == 0 && st[2] == 0 && B.untouched()); }
        else {
            // zero residuals on the fake runtime: the verdict ends every problem at its first test -- upload gather + initial point + one residual launch, the
            // verdict's read-back + the iterates'
            REQUIRE(st[0] == count && st[1] == 0 && st[2] == 3 && st[3] == 2 && launches() - l0 == 3);
            for (int i = 0; i < count; ++i) {
                REQUIRE(B.res[i].status == CIP_STATUS_OPTIMAL && B.res[i].iter == 1 && B.res[i].n_factor == 2 && B.res[i].n_solve == 1);
                REQUIRE(B.res[i].wall_s > 0 && B.res[i].trace_rows == 0);
                for (int k = 0; k < n; ++k) REQUIRE(B.yp[i][k] == 0.0);
            }
        }
        // ... and by maxIters: two iterations' steps are taken, then Abandoned needs more than the verdict allows -- with maxIters = 0 nothing iterates
        cip_options o = {1e-6, 0.01, -1.0, -1.0, 3, 0, 1};
        REQUIRE(B.run(&o) == CIP_OK);
        REQUIRE(cip_small_stats(st) == CIP_OK);
        for (int i = 0; i < count; ++i) REQUIRE(B.res[i].status == CIP_STATUS_ABANDONED && B.res[i].iter == 0 && B.res[i].n_factor == 1 && B.res[i].n_solve == 1);
        if (count > 0) REQUIRE(st[2] == 2 && st[3] == 1);
        // a negative tolerance nothing can meet: the loop runs to maxIters = 3, two launches and one read-back per iteration
        o.maxIters = 3; o.optTol = -1.0; o.infeasTol = 0.0; o.refinementThreshold = 0.0;
        REQUIRE(B.run(&o) == CIP_OK);
        REQUIRE(cip_small_stats(st) == CIP_OK);
        // (without cones mu = 0 / 0 is not finite: the reference's :Error at its first unconverged test, src/ConicIP.jl:870-873)
        const int iters = m > 0 ? 3 : 1;
        for (int i = 0; i < count; ++i)
            REQUIRE(B.res[i].status == (m > 0 ? CIP_STATUS_ABANDONED : CIP_STATUS_ERROR) && B.res[i].n_factor == 1 + iters && B.res[i].n_solve == 1 + 2 * (iters - (m > 0 ? 0 : 1)));
        if (count > 0) REQUIRE(st[0] == count && st[2] == 2 + 2 * iters - (m > 0 ? 0 : 1) && st[3] == iters + 1);
        double t2[2];
        REQUIRE(cip_small_step_time(1, nullptr) == 0);
        REQUIRE(B.run(&o) == CIP_OK);
        REQUIRE(cip_small_step_time(0, t2) == 1);
        if (count > 0) REQUIRE(t2[0] == (m > 0 ? 3.0 : 0.0) && (m == 0 || t2[1] > 0.0));
    }
    REQUIRE(live_allocs() == a0);
}

int main() {
    refusals();
    for (int device = 0; device < 2; ++device) {
        runs(0, 5, 7, 1, device);
        runs(1, 5, 7, 1, device);
        runs(200, 5, 7, 1, device);
        runs(3, 1, 1, 0, device);
        runs(3, 3, 0, 1, device);
        runs(2, 100, 1024, 28, device);
    }
    printf("drive_small: ok\n");
    return 0;
}
