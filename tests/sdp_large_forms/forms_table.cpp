// TEST INFRASTRUCTURE (tests/test_sdp_large_forms.py), one source, two stand-alone programs:
//
// forms_table (the default): includes conicip.jl_amd/csrc/cip_sdp_large_forms.h and nothing else of the library.  Reads rows of three
// integers
//     r_max  r  mode          (order of the handle's largest large S cone, order of this cone, Lanczos mode 0 .. 3)
// from standard input and prints for each the forms the header names:
//     rp=1024 jacobi=512,16,8 small=0 pairable=0 eig=cooperative cert=0 slab=16 nwg=37 lds=89408 launches=0
//
// forms_trace (-DFORMS_TRACE, linked against the host-only library and the fake HIP runtime of tests/hostsan): one NT scaling and one
// max-step of a handle with one large S cone, through the public C ABI alone -- so that it also builds against an older libcipkkt --
// with the fake runtime's launch trace switched on; the trace goes to the file named on its command line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef FORMS_TRACE
#include "cip_sdp_large_forms.h"

int main() {
    static const char *const kinds[] = {"lanczos", "registers", "cooperative", "stepped"};
    int r_max, r, mode;
    for (;;) {
        const int got = scanf("%d %d %d", &r_max, &r, &mode);
        if (got != 3) return got == EOF ? 0 : 2;
        if (r < 133 || r > r_max || r_max > 2048 || mode < 0 || mode > 3) return 3;
        const int rp = lg_padded_order(r_max);
        const LgJacobiForm j = lg_jacobi_form(rp);
        const LgEigForm e = lg_eig_form(r, mode);
        // what the kernel's template arguments must satisfy: a column pair's lanes times their elements are a column
        if (j.threads % j.block || j.epl * (j.threads / j.block) != rp || (int)j.kernel < 0 || (int)j.kernel > 3) return 4;
        printf("rp=%d jacobi=%d,%d,%d small=%d pairable=%d eig=%s cert=%d slab=%d nwg=%d lds=%zu launches=%d\n", rp, j.threads, j.epl, j.block,
               (int)lg_small_product(rp), (int)lg_pairable(rp, mode), kinds[e.kind], (int)e.certificate, e.slab, e.nwg, e.lds, e.launches);
    }
}

#else
#include "cipkkt.h"

extern "C" int fake_hip_trace(const char *path);
extern "C" void fake_hip_trace_note(const char *text);
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "forms_trace: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, cip_last_error()); exit(2); } } while (0)

static void note(const char *fmt, int a = 0, int b = 0) {
    char buf[128];
    snprintf(buf, sizeof(buf), fmt, a, b);
    fake_hip_trace_note(buf);
}

// min c'x s.t. A x >= b on one S cone of order r (n = 4 variables); under the fake runtime "device" pointers are host memory
static void one_cone(int r, int mode) {
    const int n = 4, m = r * (r + 1) / 2;
    int ctype[1] = {CIP_CONE_S}, cdim[1] = {m};
    std::vector<double> Q((size_t)n * n, 0.0), A((size_t)m * n, 0.0);
    for (int i = 0; i < n; ++i) { Q[i + (size_t)i * n] = 2.0; A[i + (size_t)i * m] = 1.0; }
    cip_problem pr;
    memset(&pr, 0, sizeof(pr));
    pr.n = n; pr.m = m; pr.p = 0; pr.ncones = 1; pr.cone_type = ctype; pr.cone_dim = cdim;
    pr.Q = Q.data(); pr.ldq = n; pr.A = A.data(); pr.lda = m; pr.ldg = 1; pr.route = CIP_ROUTE_SCHUR;
    const int pm = cip_set_sdp_lanczos(mode);
    cip_handle *h = nullptr;
    REQUIRE(cip_create_ex(&pr, &h) == CIP_OK && h);
    std::vector<double> v(m, 0.0), s(m, 0.0), lam(m, 0.0), d(m, 0.0);
    double alpha = 0.0;
    note("nt r %d mode %d", r, mode);
    REQUIRE(cip_set_scaling_from_iterate_dev(h, v.data(), s.data(), lam.data()) == CIP_OK);
    note("maxstep r %d mode %d", r, mode);
    REQUIRE(cip_maxstep_dev(h, v.data(), d.data(), 1.0, &alpha) == CIP_OK);
    note("end");
    REQUIRE(cip_destroy(h) == CIP_OK);
    cip_set_sdp_lanczos(pm);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: forms_trace OUTPUT\n"); return 2; }
    remove(argv[1]);
    REQUIRE(fake_hip_trace(argv[1]) == 0);
    one_cone(133, 2);
    one_cone(133, 0);
    one_cone(257, 2);
    fake_hip_trace(nullptr);
    REQUIRE(cip_release_cached_memory() == CIP_OK);
    printf("forms_trace: ok\n");
    return 0;
}
#endif
