// Argument rules of cip_rowrank_cert (include/cipkkt.h), driven through the host-only build of the library linked against the fake
// HIP runtime of tests/hostsan/fake_hip.cpp: every violation is refused with CIP_E_INVALID and a message naming the block and the
// entry before the runtime sees an allocation; the empty cases answer CIP_OK "not certified"; valid mixed dense / CSR inputs --
// host and "device" pointers, panel staging, an in-place block, an empty block -- run to the end and leave no allocation behind,
// under the sanitizers.  (The fake runtime's device memory reads zero, so every valid call ends at fro2 == 0: what runs here is the
// control plane -- checks, staging, uploads, clean-up -- not the arithmetic; that is tests/test_gpu_rowrank_cert.py.)
#include "cipkkt.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

extern "C" void fake_hip_stats(long *launches, long *emulated, long *live_bytes, long *live_allocs);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "drive_args: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static long live_allocs() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return a; }
static long launches() { long l, e, b, a; fake_hip_stats(&l, &e, &b, &a); return l; }

struct Csr { std::vector<int> rp, ci; std::vector<double> v; };
static cip_cert_block dense_block(const std::vector<double> &a, int cols, int ld) {
    cip_cert_block b; memset(&b, 0, sizeof(b));
    b.cols = cols; b.dense = a.data(); b.ld = ld;
    return b;
}
static cip_cert_block csr_block(const Csr &c, int cols) {
    cip_cert_block b; memset(&b, 0, sizeof(b));
    b.cols = cols; b.rowptr = c.rp.data(); b.colind = c.ci.data(); b.val = c.v.data();
    return b;
}

// refused with CIP_E_INVALID, the message holds every one of `words`, no allocation and no launch
static void refused(int n, int nblocks, const cip_cert_block *blocks, double eps, int flags, int *certified, std::initializer_list<const char *> words) {
    const long a0 = live_allocs(), l0 = launches();
    double fro2 = -1.0, shift = -1.0;
    REQUIRE(cip_rowrank_cert(n, nblocks, blocks, eps, flags, certified, &fro2, &shift) == CIP_E_INVALID);
    for (const char *w : words)
        if (!strstr(cip_last_error(), w)) { fprintf(stderr, "drive_args: \"%s\" not in \"%s\"\n", w, cip_last_error()); exit(2); }
    REQUIRE(live_allocs() == a0 && launches() == l0);
}

// 4 x 5: rows {0: cols 0, 3}, {1: col 1}, {2: none}, {3: cols 4, 2, 0} (unsorted)
static Csr good() { return Csr{{0, 2, 3, 3, 6}, {0, 3, 1, 4, 2, 0}, {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}}; }

static void violations() {
    const int n = 4;
    std::vector<double> d((size_t)n * 3, 1.0);
    const Csr c = good();
    int cert = 7;
    cip_cert_block two[2] = {dense_block(d, 3, n), csr_block(c, 5)};
    refused(-1, 2, two, 1e-8, 0, &cert, {"n = -1"});
    refused(n, -1, two, 1e-8, 0, &cert, {"nblocks = -1"});
    refused(n, 2, two, -1e-8, 0, &cert, {"eps"});
    refused(n, 2, two, NAN, 0, &cert, {"eps"});
    refused(n, 2, two, INFINITY, 0, &cert, {"eps"});
    refused(n, 2, two, 1e-8, 0, nullptr, {"certified is NULL"});
    refused(n, 2, nullptr, 1e-8, 0, &cert, {"blocks is NULL"});
    { cip_cert_block b[2] = {two[0], two[1]}; b[1].cols = -2; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "cols = -2"}); }
    { cip_cert_block b[2] = {two[0], two[1]}; b[1].dense = d.data(); refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "both"}); }
    { cip_cert_block b[2] = {two[0], two[1]}; b[0].dense = nullptr; refused(n, 2, b, 1e-8, 0, &cert, {"block 0", "neither"}); }
    { cip_cert_block b[2] = {two[0], two[1]}; b[0].ld = 3; refused(n, 2, b, 1e-8, 0, &cert, {"block 0", "ld = 3"}); }
    { cip_cert_block b[2] = {two[0], two[1]}; b[1].colind = nullptr; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "colind or val is NULL"}); }
    { cip_cert_block b[2] = {two[0], two[1]}; b[1].val = nullptr; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "colind or val is NULL"}); }
    { Csr x = c; x.rp[0] = 1; cip_cert_block b[2] = {two[0], csr_block(x, 5)}; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "rowptr[0] is 1"}); }
    { Csr x = c; x.rp[2] = 1; cip_cert_block b[2] = {two[0], csr_block(x, 5)}; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "decreases at row 1", "(1 after 2)"}); }
    { Csr x = c; x.ci[4] = 5; cip_cert_block b[2] = {two[0], csr_block(x, 5)}; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "entry 1 of row 3", "column index 5"}); }
    { Csr x = c; x.ci[1] = -1; cip_cert_block b[2] = {two[0], csr_block(x, 5)}; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "entry 1 of row 0", "column index -1"}); }
    { Csr x = c; x.ci[5] = 4; cip_cert_block b[2] = {two[0], csr_block(x, 5)}; refused(n, 2, b, 1e-8, 0, &cert, {"block 1", "entry (3, 4) is stored twice"}); }
    // the same rules for CSR arrays that live on the "device" (copied back first) ...
    { Csr x = c; x.ci[5] = 4; cip_cert_block b[1] = {csr_block(x, 5)}; refused(n, 1, b, 1e-8, CIP_FLAG_DEVICE_PTRS, &cert, {"block 0", "stored twice"}); }
    // ... and a rule of a later block still comes before any allocation for an earlier one
    { Csr x = c; x.rp[4] = 5; x.rp[3] = 6; cip_cert_block b[3] = {two[0], two[1], csr_block(x, 5)}; refused(n, 3, b, 1e-8, 0, &cert, {"block 2", "decreases"}); }
    REQUIRE(cert == 7);                                         // a refused call writes no verdict
}

static void empties() {
    const long a0 = live_allocs();
    int cert = 7; double fro2 = -1.0, shift = -1.0;
    REQUIRE(cip_rowrank_cert(0, 0, nullptr, 1e-8, 0, &cert, &fro2, &shift) == CIP_OK && cert == 0 && fro2 == 0.0 && shift == 0.0);
    cip_cert_block none[2]; memset(none, 0, sizeof(none));      // two blocks without a column: their pointers are never looked at
    cert = 7; fro2 = -1.0;
    REQUIRE(cip_rowrank_cert(5, 2, none, 1e-8, 0, &cert, &fro2, nullptr) == CIP_OK && cert == 0 && fro2 == 0.0);
    none[0].cols = 3;                                           // n == 0: columns without rows
    cert = 7;
    REQUIRE(cip_rowrank_cert(0, 2, none, 0.0, 0, &cert, nullptr, nullptr) == CIP_OK && cert == 0);
    cert = 7;
    REQUIRE(cip_rowrank_cert(5, 0, nullptr, 1e-8, 0, &cert, nullptr, nullptr) == CIP_OK && cert == 0);
    REQUIRE(live_allocs() == a0);
}

// dense + CSR + empty blocks, with n and the widths chosen so that panels are staged (n % 128 != 0; a block wider than a panel;
// cols % 16 != 0; ld > n) or, with "device" pointers and n = 128, read in place
static void valid(int n, int flags) {
    const long a0 = live_allocs();
    const int ld = n + 3, wide = 1024 + 37;
    const int ld3 = 3 * n + 20;                                 // a leading dimension far above n: the strided copy, no contiguous span
    std::vector<double> d1((size_t)ld * wide, 0.5), d2((size_t)n * 16, 0.25), d3((size_t)ld3 * 5, 1.0);
    Csr eye;
    for (int i = 0; i <= n; ++i) eye.rp.push_back(i);
    for (int i = 0; i < n; ++i) { eye.ci.push_back(i); eye.v.push_back(1.0); }
    Csr zero; zero.rp.assign((size_t)n + 1, 0);                 // nnz == 0: no index or value array
    cip_cert_block z = csr_block(zero, 9); z.colind = nullptr; z.val = nullptr;
    cip_cert_block skip; memset(&skip, 0, sizeof(skip));        // cols == 0
    cip_cert_block b[6] = {dense_block(d1, wide, ld), csr_block(eye, n), skip, dense_block(d2, 16, n), z, dense_block(d3, 5, ld3)};
    const long l0 = launches();
    int cert = 7; double fro2 = -1.0, shift = -1.0;
    REQUIRE(cip_rowrank_cert(n, 6, b, 1e-8, flags, &cert, &fro2, &shift) == CIP_OK);
    REQUIRE(cert == 0 && fro2 == 0.0 && shift == 0.0);          // (the fake device reads zero: an all-zero M)
    REQUIRE(launches() > l0);                                   // sums of squares, GEMMs and the CSR kernel were enqueued
    REQUIRE(live_allocs() == a0);
    cert = 7;
    REQUIRE(cip_rowrank_cert(n, 6, b, 1e-8, flags, &cert, nullptr, nullptr) == CIP_OK && cert == 0);   // outputs may be NULL
    REQUIRE(live_allocs() == a0);
}

int main() {
    {   // the process' one-time allocations first, so that the calls below can count
        std::vector<double> one(1, 1.0);
        cip_cert_block b = dense_block(one, 1, 1);
        int cert = 0;
        REQUIRE(cip_rowrank_cert(1, 1, &b, 1e-8, 0, &cert, nullptr, nullptr) == CIP_OK);
    }
    violations();
    empties();
    for (int flags : {0, CIP_FLAG_DEVICE_PTRS | CIP_FLAG_CSR_HOST, CIP_FLAG_DEVICE_PTRS})
        for (int n : {1, 40, 128, 129}) valid(n, flags);
    violations();                                               // ... and again behind the valid calls
    long l, e, b, a;
    fake_hip_stats(&l, &e, &b, &a);
    printf("drive_args: ok, %ld launches, %ld allocations still live\n", l, a);
    return 0;
}
