// Ragged lock-step groups (cip_set_lockstep_ragged, include/cipkkt.h) on the host-only build of the library linked against the fake HIP
// runtime of tests/hostsan/fake_hip.cpp, under AddressSanitizer / UBSan: three problems of one shape whose CSR matrices hold three
// different numbers of non-zeros, (a) CSR A on the Schur route, (b) CSR A and CSR Q, (c) both on the literal 3x3 route -- with the CSR
// arrays in host memory and again in "device" memory (CIP_FLAG_DEVICE_PTRS without CIP_FLAG_CSR_HOST: the fake runtime's device
// memory is host memory).  Switch off: cip_conicip_lockstep refuses with CIP_E_UNSUPPORTED and writes nothing, cip_conicip_mixed forms
// no group.  Switch on: one group of three from either entry point, slabs laid out for the group's largest arrays, every handle
// uploading its own nnz.  (The kernels are no-ops here: what they compute is tests/test_gpu_lockstep_ragged.py's business.)
#include "cipkkt.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive_ragged: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

struct Csr { std::vector<int> rp, ci; std::vector<double> v; };

// m x n, `extra` entries per row beside the (r, r mod n) one; columns ascending
static Csr rows_with(int m, int n, int extra) {
    Csr a;
    a.rp.push_back(0);
    for (int r = 0; r < m; ++r) {
        std::vector<char> on(n, 0);
        on[r % n] = 1;
        for (int e = 1; e <= extra; ++e) on[(r + 3 * e) % n] = 1;
        for (int j = 0; j < n; ++j)
            if (on[j]) { a.ci.push_back(j); a.v.push_back(j == r % n ? 1.0 : 0.25); }
        a.rp.push_back((int)a.ci.size());
    }
    return a;
}
// symmetric n x n: the diagonal and `band` off-diagonals on either side (band 0: thread per row; band 5: rows of up to 11 entries, wave per row)
static Csr banded(int n, int band) {
    Csr q;
    q.rp.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            if (abs(i - j) <= band) { q.ci.push_back(j); q.v.push_back(i == j ? 4.0 + band : -0.125); }
        q.rp.push_back((int)q.ci.size());
    }
    return q;
}

struct Prob {
    int n = 12, m = 12;
    int cone_type[2] = {CIP_CONE_R, CIP_CONE_Q}, cone_dim[2] = {8, 4};
    Csr A, Q;
    std::vector<double> Qd, c, b, y, v, w;
    cip_problem pr;
    Prob(int a_extra, int q_band, bool q_csr, int route, bool dev) {
        A = rows_with(m, n, a_extra);
        Q = banded(n, q_band);
        Qd.assign((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i) Qd[i + (size_t)i * n] = 2.0;
        c.assign(n, 1.0); b.assign(m, 0.0);
        for (int i = 0; i <= 8; ++i) b[i] = -1.0;              // b = -e: the R cone's ones and the Q cone's first entry
        y.assign(n, 777.0); v.assign(m, 777.0); w.assign(1, 777.0);
        memset(&pr, 0, sizeof(pr));
        pr.n = n; pr.m = m; pr.p = 0; pr.ncones = 2; pr.cone_type = cone_type; pr.cone_dim = cone_dim;
        pr.ldq = n; pr.route = route;
        pr.flags = dev ? CIP_FLAG_DEVICE_PTRS : 0;
        if (q_csr) pr.flags |= CIP_FLAG_Q_CSR;
    }
    // (the struct points into this object: taken once the object sits where it stays)
    const cip_problem &desc() {
        pr.A_rowptr = A.rp.data(); pr.A_colind = A.ci.data(); pr.A_val = A.v.data();
        pr.cone_type = cone_type; pr.cone_dim = cone_dim;
        if (pr.flags & CIP_FLAG_Q_CSR) { pr.Q = nullptr; pr.Q_rowptr = Q.rp.data(); pr.Q_colind = Q.ci.data(); pr.Q_val = Q.v.data(); }
        else pr.Q = Qd.data();
        return pr;
    }
    bool untouched() const {
        for (double x : y) if (x != 777.0) return false;
        for (double x : v) if (x != 777.0) return false;
        return true;
    }
    void reset() { y.assign(n, 777.0); v.assign(m, 777.0); }
};

struct Batch {
    std::vector<Prob> P;
    std::vector<cip_problem> desc;
    std::vector<const double *> c, b, d;
    std::vector<double *> y, w, v;
    std::vector<cip_result> res;
    void finish() {
        for (Prob &p : P) {
            desc.push_back(p.desc()); c.push_back(p.c.data()); b.push_back(p.b.data()); d.push_back(nullptr);
            y.push_back(p.y.data()); w.push_back(p.w.data()); v.push_back(p.v.data());
        }
        res.resize(P.size());
    }
    int lockstep(const cip_options &o) {
        return cip_conicip_lockstep((int)P.size(), desc.data(), c.data(), b.data(), d.data(), &o, y.data(), w.data(), v.data(), res.data());
    }
    int mixed(const cip_options &o) {
        return cip_conicip_mixed((int)P.size(), desc.data(), c.data(), b.data(), d.data(), &o, y.data(), w.data(), v.data(), res.data(), 2);
    }
    bool untouched() const { for (const Prob &p : P) if (!p.untouched()) return false; return true; }
    void reset() { for (Prob &p : P) p.reset(); }
};

static void groups(int want_groups, int want_problems) {
    int st[3] = {-1, -1, -1};
    REQUIRE(cip_lockstep_stats(st) == CIP_OK);
    if (st[0] != want_groups || st[1] != want_problems)
        fprintf(stderr, "drive_ragged: %d group(s) of %d problem(s), expected %d of %d\n", st[0], st[1], want_groups, want_problems);
    REQUIRE(st[0] == want_groups && st[1] == want_problems && st[2] == 0);
}

static void run_case(const char *what, bool q_csr, int route, bool dev) {
    Batch B;
    B.P.reserve(3);
    // three numbers of non-zeros in A (12, 24, 36 + ..) and, for a CSR Q, in Q -- the middle one in the wave-per-row form
    const int a_extra[3] = {0, 1, 3}, q_band[3] = {0, 5, 1};
    for (int k = 0; k < 3; ++k) B.P.emplace_back(a_extra[k], q_band[k], q_csr, route, dev);
    B.finish();
    REQUIRE(B.P[0].A.ci.size() != B.P[1].A.ci.size() && B.P[1].A.ci.size() != B.P[2].A.ci.size() && B.P[0].A.ci.size() != B.P[2].A.ci.size());
    cip_options o;
    o.optTol = 1e-6; o.DTB = 0.01; o.infeasTol = -1.0; o.refinementThreshold = -1.0;
    o.maxRefinementSteps = 3; o.maxIters = 2; o.verbose = 0;
    const int ps = cip_set_lockstep_split(1);
    // ---- off (the default)
    REQUIRE(cip_set_lockstep_ragged(-1) == 0);
    REQUIRE(B.lockstep(o) == CIP_E_UNSUPPORTED);
    REQUIRE(B.untouched());
    REQUIRE(B.mixed(o) == CIP_OK);
    groups(0, 0);
    REQUIRE(!B.untouched());                                   // (the thread pool solved them)
    // ---- on
    REQUIRE(cip_set_lockstep_ragged(1) == 0);
    B.reset();
    REQUIRE(B.lockstep(o) == CIP_OK);
    groups(1, 3);
    for (const Prob &p : B.P) REQUIRE(p.y[0] != 777.0 && p.v[0] != 777.0);
    B.reset();
    REQUIRE(B.mixed(o) == CIP_OK);
    groups(1, 3);
    for (const Prob &p : B.P) REQUIRE(p.y[0] != 777.0 && p.v[0] != 777.0);
    // the regularised problems of a ragged group stay in it as well (the slab then holds the refinement buffers)
    const int pr = cip_set_lockstep_regularize(1);
    B.reset();
    REQUIRE(B.lockstep(o) == CIP_OK);
    groups(1, 3);
    cip_set_lockstep_regularize(pr);
    REQUIRE(cip_set_lockstep_ragged(0) == 1);
    // ---- off again: refused as before
    B.reset();
    REQUIRE(B.lockstep(o) == CIP_E_UNSUPPORTED);
    REQUIRE(B.untouched());
    cip_set_lockstep_split(ps);
    printf("drive_ragged: %s, %s CSR arrays: ok\n", what, dev ? "\"device\"" : "host");
}

int main() {
    for (int dev = 0; dev < 2; ++dev) {
        run_case("(a) CSR A, Schur route", false, CIP_ROUTE_SCHUR, dev != 0);
        run_case("(b) CSR A and CSR Q, Schur route", true, CIP_ROUTE_SCHUR, dev != 0);
        run_case("(c) CSR A and CSR Q, literal 3x3 route", true, CIP_ROUTE_FULL3X3, dev != 0);
    }
    {   // two groups side by side, each with capacities of its own
        Batch B;
        B.P.reserve(16);
        for (int k = 0; k < 16; ++k) B.P.emplace_back(k % 4, (k % 3) * 2, true, CIP_ROUTE_SCHUR, false);
        B.finish();
        cip_options o;
        o.optTol = 1e-6; o.DTB = 0.01; o.infeasTol = -1.0; o.refinementThreshold = -1.0;
        o.maxRefinementSteps = 3; o.maxIters = 2; o.verbose = 0;
        const int ps = cip_set_lockstep_split(2);
        REQUIRE(cip_set_lockstep_ragged(1) == 0);
        REQUIRE(B.lockstep(o) == CIP_OK);
        groups(2, 16);
        REQUIRE(cip_set_lockstep_ragged(0) == 1);
        cip_set_lockstep_split(ps);
    }
    REQUIRE(cip_release_cached_memory() == CIP_OK);
    long launches, emulated, live_bytes, live_allocs;
    fake_hip_stats(&launches, &emulated, &live_bytes, &live_allocs);
    printf("drive_ragged: ok, %ld launches, %ld device allocations still live\n", launches, live_allocs);
    return 0;
}
