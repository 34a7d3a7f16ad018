// Level-1 rules of a CSR objective matrix Q (CIP_FLAG_Q_CSR, include/cipkkt.h), driven through the host-only build of the library
// linked against the fake HIP runtime of tests/hostsan/fake_hip.cpp: every violation is refused with CIP_E_INVALID and a message
// that names the first offending entry, before any device allocation; valid matrices (a diagonal, the empty one, one with unsorted
// columns) go through cip_create_ex / cip_update_problem / cip_destroy to the end, under the sanitizers.
#include "cipkkt.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive_args: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static long live_allocs() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return a; }

struct Csr { std::vector<int> rp, ci; std::vector<double> v; };

// n variables, the bound constraints y >= 0 as a CSR identity, one R cone
struct Problem {
    int n;
    std::vector<int> a_rp, a_ci; std::vector<double> a_v;
    int cone_type[1], cone_dim[1];
    cip_problem pr;
    explicit Problem(int n_, int route = CIP_ROUTE_SCHUR) : n(n_) {
        for (int i = 0; i <= n; ++i) a_rp.push_back(i);
        for (int i = 0; i < n; ++i) { a_ci.push_back(i); a_v.push_back(1.0); }
        cone_type[0] = CIP_CONE_R; cone_dim[0] = n;
        memset(&pr, 0, sizeof(pr));
        pr.n = n; pr.m = n; pr.p = 0; pr.ncones = 1; pr.cone_type = cone_type; pr.cone_dim = cone_dim;
        pr.ldq = n; pr.A_rowptr = a_rp.data(); pr.A_colind = a_ci.data(); pr.A_val = a_v.data();
        pr.route = route; pr.flags = CIP_FLAG_Q_CSR;
    }
    void set_q(const Csr &q) { pr.Q = nullptr; pr.Q_rowptr = q.rp.data(); pr.Q_colind = q.ci.data(); pr.Q_val = q.v.data(); }
};

// refused with CIP_E_INVALID, the message holds every one of `words`, nothing allocated on the device, no handle returned
static void refused(const cip_problem &pr, std::initializer_list<const char *> words) {
    const long a0 = live_allocs();
    cip_handle *h = (cip_handle *)0x1;
    REQUIRE(cip_create_ex(&pr, &h) == CIP_E_INVALID);
    REQUIRE(h == nullptr);
    for (const char *w : words)
        if (!strstr(cip_last_error(), w)) { fprintf(stderr, "drive_args: \"%s\" not in \"%s\"\n", w, cip_last_error()); exit(2); }
    REQUIRE(live_allocs() == a0);
}

// the 4 x 4 symmetric matrix [2 1 0 0; 1 3 0 5; 0 0 0 0; 0 5 0 4] (row 2 empty)
static Csr good4() { return Csr{{0, 2, 5, 5, 7}, {0, 1, 0, 1, 3, 1, 3}, {2.0, 1.0, 1.0, 3.0, 5.0, 5.0, 4.0}}; }

static void violations() {
    Problem P(4);
    Csr q = good4();
    P.set_q(q);
    {   // the flag with a dense Q as well
        std::vector<double> dense(16, 0.0);
        cip_problem pr = P.pr; pr.Q = dense.data();
        refused(pr, {"CIP_FLAG_Q_CSR", "Q is not NULL"});
    }
    {   // Q == NULL without the flag keeps its old answer
        cip_problem pr = P.pr; pr.flags = 0;
        refused(pr, {"Q is NULL"});
    }
    { cip_problem pr = P.pr; pr.Q_rowptr = nullptr; refused(pr, {"Q_rowptr is NULL"}); }
    { cip_problem pr = P.pr; pr.Q_colind = nullptr; refused(pr, {"Q_colind is NULL"}); }
    { cip_problem pr = P.pr; pr.Q_val = nullptr; refused(pr, {"Q_val is NULL"}); }
    { Csr b = q; b.rp[0] = 1; P.set_q(b); refused(P.pr, {"rowptr[0] is 1"}); }
    { Csr b = q; b.rp[2] = 1; P.set_q(b); refused(P.pr, {"decreases at row 1", "(1 after 2)"}); }
    { Csr b = q; b.ci[4] = 4; P.set_q(b); refused(P.pr, {"entry 2 of row 1", "column index 4"}); }
    { Csr b = q; b.ci[1] = -1; P.set_q(b); refused(P.pr, {"entry 1 of row 0", "column index -1"}); }
    {   // (1, 3) twice, in an unsorted row: [0, 3, 1, 3]
        Csr b{{0, 2, 6, 6, 8}, {0, 1, 0, 3, 1, 3, 1, 3}, {2.0, 1.0, 1.0, 2.5, 3.0, 2.5, 5.0, 4.0}};
        P.set_q(b); refused(P.pr, {"entry (1, 3) is stored twice"});
    }
    {   // (1, 3) without (3, 1)
        Csr b{{0, 2, 5, 5, 6}, {0, 1, 0, 1, 3, 3}, {2.0, 1.0, 1.0, 3.0, 5.0, 4.0}};
        P.set_q(b); refused(P.pr, {"entry (1, 3) has no stored mirror entry (3, 1)"});
    }
    {   // (3, 1) without (1, 3): found at row 1, where the mirror is missing
        Csr b{{0, 2, 4, 4, 6}, {0, 1, 0, 1, 1, 3}, {2.0, 1.0, 1.0, 3.0, 5.0, 4.0}};
        P.set_q(b); refused(P.pr, {"entry (3, 1) has no stored mirror entry (1, 3)"});
    }
    {   // the mirror entry differs in its last bit
        Csr b = q;
        unsigned long long bits; memcpy(&bits, &b.v[5], 8); bits += 1; memcpy(&b.v[5], &bits, 8);
        P.set_q(b); refused(P.pr, {"entry (1, 3)", "mirror entry (3, 1)", "differ"});
    }
    {   // +0.0 against -0.0 is a difference too
        Csr b = q; b.v[1] = 0.0; b.v[2] = -0.0;
        P.set_q(b); refused(P.pr, {"entry (0, 1)", "differ"});
    }
}

// create -> update (same nnz: accepted; other nnz, the other form, a broken matrix: refused, the handle goes on) -> destroy
static void valid(const Csr &q, const Csr &q_same_nnz, int route) {
    const int n = (int)q.rp.size() - 1;
    Problem P(n, route);
    P.set_q(q);
    cip_handle *h = nullptr;
    REQUIRE(cip_create_ex(&P.pr, &h) == CIP_OK && h);
    int N = 0, Np = 0;
    REQUIRE(cip_kkt_order(h, &N, &Np) == CIP_OK && N == (route == CIP_ROUTE_SCHUR ? n : 2 * n));
    REQUIRE(cip_assemble_only(h) == CIP_OK);
    REQUIRE(cip_factor(h) == CIP_OK && cip_check_factor(h) == CIP_OK);
    P.set_q(q_same_nnz);
    REQUIRE(cip_update_problem(h, &P.pr) == CIP_OK);
    {   // one entry more
        Csr b = q;
        b.ci.push_back(n - 1); b.v.push_back(1.0); b.rp[n] += 1;
        P.set_q(b);
        REQUIRE(cip_update_problem(h, &P.pr) == CIP_E_INVALID);
        REQUIRE(strstr(cip_last_error(), "non-zeros") != nullptr);
    }
    {   // the dense form
        std::vector<double> dense((size_t)n * n, 0.0);
        cip_problem pr = P.pr; pr.flags = 0; pr.Q = dense.data(); pr.Q_rowptr = nullptr; pr.Q_colind = nullptr; pr.Q_val = nullptr;
        REQUIRE(cip_update_problem(h, &pr) == CIP_E_INVALID);
        REQUIRE(strstr(cip_last_error(), "created with a CSR Q") != nullptr);
    }
    if (q.rp[n] > 0) {   // same nnz, an index out of range
        Csr b = q; b.ci[0] = n;
        P.set_q(b);
        REQUIRE(cip_update_problem(h, &P.pr) == CIP_E_INVALID);
    }
    P.set_q(q);
    REQUIRE(cip_update_problem(h, &P.pr) == CIP_OK);
    REQUIRE(cip_assemble_only(h) == CIP_OK);
    REQUIRE(cip_destroy(h) == CIP_OK);
    // a dense handle refuses the CSR form
    std::vector<double> dense((size_t)n * n, 0.0);
    cip_problem pd = P.pr; pd.flags = 0; pd.Q = dense.data(); pd.Q_rowptr = nullptr; pd.Q_colind = nullptr; pd.Q_val = nullptr;
    REQUIRE(cip_create_ex(&pd, &h) == CIP_OK && h);
    P.set_q(q);
    REQUIRE(cip_update_problem(h, &P.pr) == CIP_E_INVALID);
    REQUIRE(strstr(cip_last_error(), "created with a dense Q") != nullptr);
    REQUIRE(cip_update_problem(h, &pd) == CIP_OK);
    REQUIRE(cip_destroy(h) == CIP_OK);
}

int main() {
    {   // the process' one-time allocations first, so that the refusals below can count
        Csr d{{0, 1}, {0}, {1.0}};
        Problem P(1);
        P.set_q(d);
        cip_handle *h = nullptr;
        REQUIRE(cip_create_ex(&P.pr, &h) == CIP_OK && cip_destroy(h) == CIP_OK);
    }
    violations();
    for (int route : {CIP_ROUTE_SCHUR, CIP_ROUTE_FULL3X3}) {
        {   // a diagonal of order 130 (more than one 128-tile)
            Csr d, d2;
            for (int i = 0; i <= 130; ++i) d.rp.push_back(i);
            for (int i = 0; i < 130; ++i) { d.ci.push_back(i); d.v.push_back(1.0 + i); }
            d2 = d;
            for (double &x : d2.v) x *= 0.5;
            valid(d, d2, route);
        }
        {   // the zero objective: nnz = 0, no index or value array at all
            Csr z;
            z.rp.assign(6, 0);
            Problem P(5, route);
            P.pr.Q_rowptr = z.rp.data(); P.pr.Q_colind = nullptr; P.pr.Q_val = nullptr;
            cip_handle *h = nullptr;
            REQUIRE(cip_create_ex(&P.pr, &h) == CIP_OK && h);
            REQUIRE(cip_assemble_only(h) == CIP_OK);
            REQUIRE(cip_update_problem(h, &P.pr) == CIP_OK);
            REQUIRE(cip_destroy(h) == CIP_OK);
            valid(z, z, route);
        }
        {   // columns in any order: good4 with rows 1 and 3 reversed
            Csr u{{0, 2, 5, 5, 7}, {1, 0, 3, 1, 0, 3, 1}, {1.0, 2.0, 5.0, 3.0, 1.0, 4.0, 5.0}};
            Csr u2 = u;
            for (double &x : u2.v) x = -x;
            valid(u, u2, route);
        }
    }
    long l, e, b, a;
    fake_hip_stats(&l, &e, &b, &a);
    printf("drive_args: ok, %ld launches, %ld device allocations still live\n", l, a);
    return 0;
}
