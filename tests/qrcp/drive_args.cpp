// Argument rules and control flow of the rank-revealing QR entry points (include/cipkkt.h), driven through the host-only build of
// the library linked against the fake HIP runtime of tests/hostsan/fake_hip.cpp: every refusal returns CIP_E_INVALID with nothing
// launched, len * cnt == 0 is a no-op, and valid calls run their host code (workspace carving, the chunked step loop and its
// read-backs, the solve sequence of imcols) under the sanitizers with a workspace of exactly the advertised size.  Device memory
// reads zero there: the step loop must end on its own after min(len, cnt) steps and report k = 0, nrows = 0.
#include "cipkkt.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive_args: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static long launches() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return l; }

static void refusals() {
    const int len = 12, cnt = 7;
    size_t qb = 0, ib = 0;
    REQUIRE(cip_qrcp_workspace_bytes(-1, cnt, &qb) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_workspace_bytes(len, -1, &qb) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_workspace_bytes(len, cnt, nullptr) == CIP_E_INVALID);
    REQUIRE(cip_imcols_workspace_bytes(-1, cnt, &ib) == CIP_E_INVALID);
    REQUIRE(cip_imcols_workspace_bytes(len, -1, &ib) == CIP_E_INVALID);
    REQUIRE(cip_imcols_workspace_bytes(len, cnt, nullptr) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_workspace_bytes(len, cnt, &qb) == CIP_OK && qb > 0);
    REQUIRE(cip_imcols_workspace_bytes(len, cnt, &ib) == CIP_OK && ib >= qb + sizeof(double) * len * cnt);
    std::vector<double> M((size_t)(len + 3) * cnt, 0.0), b(cnt, 0.0), tau(cnt), rdiag(cnt);
    std::vector<char> ws(ib);
    std::vector<int> piv(cnt), rows(cnt);
    int k = -1, nrows = -1, ok = -1;
    double resid = -1.0;
    const long l0 = launches();
    REQUIRE(cip_qrcp_dev(nullptr, nullptr, len, cnt, len, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, cnt, len, 0.0, nullptr, tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, cnt, len, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), nullptr) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_dev(nullptr, M.data(), -1, cnt, len, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, -1, len, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    for (int ld : {len - 1, 0, -len})
        REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, cnt, ld, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    REQUIRE(cip_qrcp_dev(nullptr, M.data(), 0, cnt, 0, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    for (double stop : {-1.0, -0.0 - 1e-300, (double)NAN, (double)INFINITY})
        REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, cnt, len, stop, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, nullptr, len, cnt, len, b.data(), 1e-8, ws.data(), rows.data(), &nrows, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len, nullptr, 1e-8, ws.data(), rows.data(), &nrows, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len, b.data(), 1e-8, nullptr, rows.data(), &nrows, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len, b.data(), 1e-8, ws.data(), nullptr, &nrows, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len, b.data(), 1e-8, ws.data(), rows.data(), nullptr, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len, b.data(), 1e-8, ws.data(), rows.data(), &nrows, nullptr, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len - 1, b.data(), 1e-8, ws.data(), rows.data(), &nrows, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(cip_imcols_dev(nullptr, M.data(), -2, cnt, len, b.data(), 1e-8, ws.data(), rows.data(), &nrows, &ok, &resid) == CIP_E_INVALID);
    for (double eps : {-1e-8, (double)NAN, (double)INFINITY})
        REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, len, b.data(), eps, ws.data(), rows.data(), &nrows, &ok, &resid) == CIP_E_INVALID);
    REQUIRE(launches() == l0);
    REQUIRE(k == -1 && nrows == -1 && ok == -1);                 // a refusal writes nothing
    // len * cnt == 0: no-op with k = 0 (NULL M / workspace are fine then), no rows, consistent
    REQUIRE(cip_qrcp_dev(nullptr, nullptr, 0, cnt, 1, 0.0, nullptr, nullptr, piv.data(), nullptr, &k) == CIP_OK && k == 0);
    for (int c = 0; c < cnt; ++c) REQUIRE(piv[c] == c);
    k = -1;
    REQUIRE(cip_qrcp_dev(nullptr, nullptr, len, 0, len, 0.0, nullptr, nullptr, nullptr, nullptr, &k) == CIP_OK && k == 0);
    REQUIRE(cip_qrcp_dev(nullptr, nullptr, 0, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, &k) == CIP_OK && k == 0);
    REQUIRE(cip_imcols_dev(nullptr, nullptr, 0, cnt, 1, nullptr, 1e-8, nullptr, nullptr, &nrows, &ok, &resid) == CIP_OK && nrows == 0 && ok == 1 && resid == 0.0);
    nrows = ok = -1;
    REQUIRE(cip_imcols_dev(nullptr, nullptr, len, 0, len, nullptr, 1e-8, nullptr, nullptr, &nrows, &ok, nullptr) == CIP_OK && nrows == 0 && ok == 1);
    REQUIRE(launches() == l0);
}

// valid calls with a workspace of exactly the advertised size; every optional output given, then none
static void valid(int len, int cnt, int ld) {
    size_t qb = 0, ib = 0;
    REQUIRE(cip_qrcp_workspace_bytes(len, cnt, &qb) == CIP_OK && cip_imcols_workspace_bytes(len, cnt, &ib) == CIP_OK);
    const int kmax = len < cnt ? len : cnt;
    std::vector<double> M((size_t)ld * cnt, 1.0), b(cnt, 1.0), tau(kmax), rdiag(kmax);
    std::vector<int> piv(cnt, -1), rows(cnt, -1);
    int k = -1, nrows = -1, ok = -1;
    double resid = -1.0;
    const long l0 = launches();
    {
        std::vector<char> ws(qb);
        REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, cnt, ld, 0.0, ws.data(), tau.data(), piv.data(), rdiag.data(), &k) == CIP_OK);
        REQUIRE(k == 0);                                         // device memory reads zero: no step is ever reported done
        REQUIRE(launches() - l0 >= 2L * kmax - 1);               // ... and the loop still enqueued every step and ended
        k = -1;
        REQUIRE(cip_qrcp_dev(nullptr, M.data(), len, cnt, ld, 1e-8, ws.data(), nullptr, nullptr, nullptr, &k) == CIP_OK && k == 0);
    }
    {
        std::vector<char> ws(ib);
        REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, ld, b.data(), 1e-8, ws.data(), rows.data(), &nrows, &ok, &resid) == CIP_OK);
        REQUIRE(nrows == 0 && ok == 1);
        nrows = ok = -1;
        REQUIRE(cip_imcols_dev(nullptr, M.data(), len, cnt, ld, b.data(), 0.0, ws.data(), rows.data(), &nrows, &ok, nullptr) == CIP_OK);
        REQUIRE(nrows == 0 && ok == 1);
    }
}

int main() {
    refusals();
    const int shapes[][3] = {{1, 1, 1}, {3, 1, 3}, {1, 5, 4}, {12, 7, 12}, {12, 7, 17}, {65, 300, 66}, {700, 40, 700}, {5000, 3, 5001}, {30, 1100, 30}};
    for (const auto &s : shapes) valid(s[0], s[1], s[2]);
    long l, e, b, a;
    fake_hip_stats(&l, &e, &b, &a);
    printf("drive_args: ok, %ld launches, %ld device allocations still live\n", l, a);
    return 0;
}
