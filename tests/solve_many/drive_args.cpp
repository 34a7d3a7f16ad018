// Argument rules of the many-right-hand-side entry points (include/cipkkt.h), driven through the host-only build of the library
// linked against the fake HIP runtime of tests/hostsan/fake_hip.cpp: every refusal returns CIP_E_INVALID with nothing launched,
// nrhs == 0 is a no-op, and valid calls run their host code (launch sequences, chunking, lazy scratch) under the sanitizers.
#include "cipkkt.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive_args: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static long launches() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return l; }

static void standalone() {
    const int N = 512;
    size_t bytes = 0, sb = 0, prev = 0;
    REQUIRE(cip_ldlt_workspace_bytes(N, &bytes) == CIP_OK);
    // the scratch query: refusals, monotone in nrhs, bounded by the 64-column chunk
    REQUIRE(cip_ldlt_solve_many_scratch_bytes(N, -1, &sb) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_scratch_bytes(N + 1, 4, &sb) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_scratch_bytes(0, 4, &sb) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_scratch_bytes(N, 4, nullptr) == CIP_E_INVALID);
    for (int k = 0; k <= 300; ++k) {
        REQUIRE(cip_ldlt_solve_many_scratch_bytes(N, k, &sb) == CIP_OK);
        REQUIRE(sb >= prev);
        REQUIRE(sb <= sizeof(double) * 1024 * 64);
        if (k > 0) REQUIRE(sb > 0);
        prev = sb;
    }
    size_t s64 = 0, s1000 = 0;
    REQUIRE(cip_ldlt_solve_many_scratch_bytes(8192, 64, &s64) == CIP_OK && cip_ldlt_solve_many_scratch_bytes(8192, 1000, &s1000) == CIP_OK);
    REQUIRE(s64 == s1000 && s64 == sizeof(double) * 1024 * 64);

    const int nrhs = 5, ldb = N + 3;
    std::vector<double> K((size_t)(N + 128) * (N + 128), 0.0), B((size_t)ldb * 70, 1.0);
    for (int i = 0; i < N; ++i) K[i + (size_t)i * N] = 1.0;
    std::vector<char> ws(bytes);
    REQUIRE(cip_ldlt_solve_many_scratch_bytes(N, 70, &sb) == CIP_OK);
    std::vector<char> scratch(sb);
    int info = -1;
    REQUIRE(cip_ldlt_factor_dev(nullptr, K.data(), N, N, ws.data(), &info) == CIP_OK);
    const long l0 = launches();
    for (int ld : {N - 128, N + 64, N + 2, N - 1, 0, -N})
        REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, ld, ws.data(), scratch.data(), B.data(), ldb, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N + 1, N + 128, ws.data(), scratch.data(), B.data(), ldb, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, nullptr, N, N, ws.data(), scratch.data(), B.data(), ldb, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, nullptr, scratch.data(), B.data(), ldb, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, ws.data(), nullptr, B.data(), ldb, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, ws.data(), scratch.data(), nullptr, ldb, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, ws.data(), scratch.data(), B.data(), N - 1, nrhs) == CIP_E_INVALID);
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, ws.data(), scratch.data(), B.data(), ldb, -1) == CIP_E_INVALID);
    REQUIRE(launches() == l0);
    // nrhs == 0: no-op (NULL B / scratch are fine then)
    REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, ws.data(), nullptr, nullptr, ldb, 0) == CIP_OK);
    REQUIRE(launches() == l0);
    // valid calls go through: one column (the single solve), several, more than one chunk
    for (int k : {1, nrhs, 70}) REQUIRE(cip_ldlt_solve_many_dev(nullptr, K.data(), N, N, ws.data(), scratch.data(), B.data(), ldb, k) == CIP_OK);
    REQUIRE(launches() > l0);
}

static void handle(int route, bool with_p) {
    const int n = 24, m = 24, p = with_p ? 3 : 0;
    std::vector<double> Q((size_t)n * n, 0.0), A((size_t)m * n, 0.0), G((size_t)(p > 0 ? p : 1) * n, 0.0);
    for (int i = 0; i < n; ++i) { Q[i + (size_t)i * n] = 2.0; A[i + (size_t)i * m] = 1.0; }
    for (int i = 0; i < p; ++i) G[i + (size_t)i * p] = 1.0;
    const int ct[1] = {CIP_CONE_R}, cdim[1] = {m};
    cip_handle *h = nullptr;
    REQUIRE(cip_create(n, m, p, 1, ct, cdim, Q.data(), A.data(), p > 0 ? G.data() : nullptr, route, &h) == CIP_OK);
    REQUIRE(cip_set_scaling_identity(h) == CIP_OK);
    const int k = 70;
    std::vector<double> X((size_t)n * k, 1.0), Y((size_t)(p + 1) * k, 1.0), Z((size_t)m * k, 1.0), Ao((size_t)n * k), Bo((size_t)(p + 1) * k),
        Co((size_t)m * k);
    const double *y = p > 0 ? Y.data() : nullptr;
    double *bo = p > 0 ? Bo.data() : nullptr;
    // before a factorisation: the argument checks come first
    const long l0 = launches();
    REQUIRE(cip_solve3x3_many(nullptr, 2, X.data(), y, Z.data(), Ao.data(), bo, Co.data()) == CIP_E_INVALID);
    REQUIRE(cip_solve3x3_many_dev(nullptr, 2, X.data(), y, Z.data(), Ao.data(), bo, Co.data()) == CIP_E_INVALID);
    for (int dev = 0; dev < 2; ++dev) {
        auto s3 = dev ? cip_solve3x3_many_dev : cip_solve3x3_many;
        auto s2 = dev ? cip_solve2x2_many_dev : cip_solve2x2_many;
        REQUIRE(s3(h, -1, X.data(), y, Z.data(), Ao.data(), bo, Co.data()) == CIP_E_INVALID);
        REQUIRE(s3(h, 2, nullptr, y, Z.data(), Ao.data(), bo, Co.data()) == CIP_E_INVALID);
        REQUIRE(s3(h, 2, X.data(), y, Z.data(), nullptr, bo, Co.data()) == CIP_E_INVALID);
        REQUIRE(s3(h, 2, X.data(), y, nullptr, Ao.data(), bo, Co.data()) == CIP_E_INVALID);
        REQUIRE(s3(h, 2, X.data(), y, Z.data(), Ao.data(), bo, nullptr) == CIP_E_INVALID);
        if (p > 0) {
            REQUIRE(s3(h, 2, X.data(), nullptr, Z.data(), Ao.data(), bo, Co.data()) == CIP_E_INVALID);
            REQUIRE(s3(h, 2, X.data(), y, Z.data(), Ao.data(), nullptr, Co.data()) == CIP_E_INVALID);
            REQUIRE(s2(h, 2, X.data(), nullptr, Ao.data(), bo) == CIP_E_INVALID);
            REQUIRE(s2(h, 2, X.data(), y, Ao.data(), nullptr) == CIP_E_INVALID);
        }
        REQUIRE(s2(nullptr, 2, X.data(), y, Ao.data(), bo) == CIP_E_INVALID);
        REQUIRE(s2(h, -3, X.data(), y, Ao.data(), bo) == CIP_E_INVALID);
        REQUIRE(s2(h, 2, nullptr, y, Ao.data(), bo) == CIP_E_INVALID);
        REQUIRE(s2(h, 2, X.data(), y, nullptr, bo) == CIP_E_INVALID);
        // nrhs == 0: no-op, also before any factorisation
        REQUIRE(s3(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == CIP_OK);
        REQUIRE(s2(h, 0, nullptr, nullptr, nullptr, nullptr) == CIP_OK);
        REQUIRE(s3(h, 2, X.data(), y, Z.data(), Ao.data(), bo, Co.data()) == CIP_E_NOTFACTORED);
    }
    REQUIRE(launches() == l0);
    REQUIRE(cip_factor(h) == CIP_OK);
    REQUIRE(cip_check_factor(h) == CIP_OK);
    for (int kk : {1, 5, 64, k}) {
        REQUIRE(cip_solve3x3_many(h, kk, X.data(), y, Z.data(), Ao.data(), bo, Co.data()) == CIP_OK);
        REQUIRE(cip_solve3x3_many(h, kk, X.data(), y, Z.data(), Ao.data(), bo, Z.data()) == CIP_OK);      // C aliases Z
        const int rc2 = cip_solve2x2_many(h, kk, X.data(), y, Ao.data(), bo);
        REQUIRE(rc2 == (route == CIP_ROUTE_SCHUR ? CIP_OK : CIP_E_UNSUPPORTED));
    }
    double st[8];
    REQUIRE(cip_stats(h, st) == CIP_OK);
    REQUIRE(cip_destroy(h) == CIP_OK);
}

int main() {
    standalone();
    for (int route : {CIP_ROUTE_SCHUR, CIP_ROUTE_FULL3X3})
        for (bool wp : {false, true}) handle(route, wp);
    long l, e, b, a;
    fake_hip_stats(&l, &e, &b, &a);
    printf("drive_args: ok, %ld launches, %ld device allocations still live\n", l, a);
    return 0;
}
