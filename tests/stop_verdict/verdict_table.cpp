// TEST INFRASTRUCTURE (tests/test_stop_verdict.py): a stand-alone program that includes conicip.jl_amd/csrc/cip_driver_scalars.h and
// nothing else of the library.  Reads rows of whitespace-separated numbers (strtod: decimal, hex floats, nan, inf) from standard input
//     reset optBest0 has_trace | 16 dots (the order of IterDots) | normc normb normd | conedim m p |
//     has_opt optTol DTB infeasTol refinementThreshold maxRefinementSteps maxIters | Iter | ny nw nv | y.. w.. v..
// and prints one line per row.  reset = 1 starts a fresh cip_result (the values of a Solution before the first iteration) and
// takes optBest0 as the running best; reset = 0 carries both over from the row before, which is how a sequence is replayed.
// has_opt = 0 passes NULL to resolve_options.  The line: the verdict (status, scale, mu), the cip_result fields the verdict may
// update, the running best, the trace row, host_norms of (c, b, d) = (y, v, w), the three vectors after apply_certificate with
// (n, m, p) = (ny, nv, nw), and the resolved options.  Doubles are printed with %a.
#include "cip_driver_scalars.h"

#include <cstdlib>
#include <cstring>
#include <vector>

static bool next(double *x) {
    char tok[128];
    if (scanf("%127s", tok) != 1) return false;
    char *end = nullptr;
    *x = strtod(tok, &end);
    if (end == tok || *end) { fprintf(stderr, "verdict_table: bad token '%s'\n", tok); exit(2); }
    return true;
}

static double need() {
    double x;
    if (!next(&x)) { fprintf(stderr, "verdict_table: row ends early\n"); exit(2); }
    return x;
}

static void vec(const char *name, const std::vector<double> &x) {
    printf(" %s=", name);
    for (size_t i = 0; i < x.size(); ++i) printf(i ? ",%a" : "%a", x[i]);
}

int main() {
    cip_result res;
    double optBest = INFINITY;
    memset(&res, 0, sizeof(res));
    for (double first; next(&first);) {
        const bool reset = first != 0;
        const double optBest0 = need();
        const bool has_trace = need() != 0;
        cipdrv::IterDots dd;
        for (int i = 0; i < 16; ++i) dd.v[i] = need();
        cipdrv::Norms nm;
        nm.normc = need(); nm.normb = need(); nm.normd = need();
        const double conedim = need();
        const int m = (int)need(), p = (int)need();
        const bool has_opt = need() != 0;
        cip_options in;
        in.optTol = need(); in.DTB = need(); in.infeasTol = need(); in.refinementThreshold = need();
        in.maxRefinementSteps = (int)need(); in.maxIters = (int)need(); in.verbose = 0;
        const int Iter = (int)need();
        const int ny = (int)need(), nw = (int)need(), nv = (int)need();
        if (ny < 0 || nw < 0 || nv < 0 || ny > 64 || nw > 64 || nv > 64) return 3;
        std::vector<double> y(ny), w(nw), v(nv);
        for (double &x : y) x = need();
        for (double &x : w) x = need();
        for (double &x : v) x = need();
        if (reset) {
            memset(&res, 0, sizeof(res));
            res.prFeas = res.duFeas = res.muFeas = res.pobj = INFINITY; res.dobj = -INFINITY;
            optBest = optBest0;
        }
        const cip_options o = cipdrv::resolve_options(has_opt ? &in : nullptr);
        double tr[9];
        for (double &x : tr) x = -1.0;
        const cipdrv::IterOutcome oc = cipdrv::evaluate_iteration(dd, nm, conedim, m, p, o, Iter, &res, optBest, has_trace ? tr : nullptr);
        printf("status=%d scale=%a mu=%a mubar=%a iter=%d resmu=%a prFeas=%a duFeas=%a muFeas=%a pobj=%a dobj=%a trace_rows=%d optBest=%a",
               oc.status, oc.scale, oc.mu, oc.mubar, res.iter, res.mu, res.prFeas, res.duFeas, res.muFeas, res.pobj, res.dobj,
               res.trace_rows, optBest);
        vec("tr", std::vector<double>(tr, tr + 9));
        const cipdrv::Norms hn = cipdrv::host_norms(ny, nv, nw, y.data(), v.data(), w.data());
        printf(" hn=%a,%a,%a", hn.normc, hn.normb, hn.normd);
        cipdrv::apply_certificate(oc, ny, nv, nw, y.data(), w.data(), v.data());
        vec("y", y); vec("w", w); vec("v", v);
        printf(" opt=%.17g,%.17g,%.17g,%.17g,%d,%d,%d\n", o.optTol, o.DTB, o.infeasTol, o.refinementThreshold, o.maxRefinementSteps,
               o.maxIters, o.verbose);
    }
    return 0;
}
