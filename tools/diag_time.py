"""The diagonal kernel alone: time of an order-128 factorisation (one k_ldlt_panel<false> launch without strips, then the block
inverse) on two or more builds of the library, alternating, each build in a fresh child process.

    python tools/diag_time.py PARENT.so BRANCH.so [MORE.so ...] [--pairs 3] [--reps 3000] [--order 128]

A child factors the KKT matrix of a dense box QP of the given order `reps` times through a handle with cip_set_timing on: the
library then records HIP events around the LDL' launches on its own stream (csrc/api.hip: cip_factor; ms_ldlt of cip_stats).
Every factorisation is enqueued behind a spin kernel that keeps the stream busy while the host enqueues, so that the events
bracket GPU time and not the host's launch gaps.  The figure of a run is the median over the repetitions; the child also prints a
hash of the factor it produced (the builds must agree bit for bit).  The parent prints every run, the spread of the first build's
own runs and the verdict: every other build below the first in every round by more than that spread, or not.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(order, reps):
    for p in (ROOT, os.path.join(ROOT, "conicip.jl_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import scipy.sparse as sp
    import torch
    import cipkkt

    rng = np.random.default_rng(order)
    M = rng.standard_normal((order, order))
    ks = cipkkt.KKTSystem(M.T @ M / order, sp.identity(order, format="csr"), None, [("R", order)], route="schur")
    f64 = dict(dtype=torch.float64, device="cuda:0")
    ks.set_scaling_from_iterate(torch.as_tensor(rng.random(order) + 0.1, **f64), torch.as_tensor(rng.random(order) + 1e-3, **f64))
    stream = torch.cuda.Stream()
    ks.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        # spin length: ~300 us of the stream per factorisation, calibrated once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        stream.synchronize()
        e0.record(); torch.cuda._sleep(1000000); e1.record(); stream.synchronize()
        spin = int(1000000 * 0.3 / max(e0.elapsed_time(e1), 1e-3))
        ks.set_timing(True)
        for _ in range(50):
            torch.cuda._sleep(spin)
            ks.factor(check=False)
        t = np.empty(reps)
        for i in range(reps):
            torch.cuda._sleep(spin)
            ks.factor(check=False)                      # (timed: returns when the LDL' events have landed)
            t[i] = ks.stats()["ms_ldlt"] * 1e3
        ks.set_timing(False)
        ks.factor(check=True)
        digest = hashlib.sha1(np.ascontiguousarray(np.tril(ks.kkt_matrix())).tobytes()).hexdigest()[:16]
    ks.close()
    print("DIAG_TIME " + json.dumps(dict(median_us=float(np.median(t)), p10_us=float(np.quantile(t, 0.1)),
                                         p90_us=float(np.quantile(t, 0.9)), reps=reps, order=order, factor=digest)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3000)
    ap.add_argument("--order", type=int, default=128)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.order, a.reps)
    if len(a.libs) < 2:
        ap.error("two or more builds of libcipkkt.so: the parent's first")
    runs = {lib: [] for lib in a.libs}
    for rnd in range(a.pairs):
        for lib in a.libs:
            env = dict(os.environ, CIPKKT_LIB=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--order", str(a.order)],
                                 env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("DIAG_TIME ")]
            if out.returncode != 0 or not line:
                sys.exit("child failed on %s (exit %d):\n%s\n%s" % (lib, out.returncode, out.stdout[-2000:], out.stderr[-2000:]))
            r = json.loads(line[0][len("DIAG_TIME "):])
            runs[lib].append(r)
            print("round %d  %-40s median %.2f us  (p10 %.2f, p90 %.2f)  factor %s"
                  % (rnd, lib, r["median_us"], r["p10_us"], r["p90_us"], r["factor"]), flush=True)
    base = a.libs[0]
    bm = [r["median_us"] for r in runs[base]]
    spread = max(bm) - min(bm)
    print("first build's own spread over %d runs: %.2f us" % (len(bm), spread))
    ok = True
    for lib in a.libs[1:]:
        m = [r["median_us"] for r in runs[lib]]
        same = all(r["factor"] == runs[base][0]["factor"] for r in runs[lib] + runs[base])
        lower = all(b - x > spread for b, x in zip(bm, m))
        ok = ok and same and lower
        print("%-40s mean %.2f us against %.2f (%+.1f %%); lower in every round by more than the spread: %s; same bits: %s"
              % (lib, sum(m) / len(m), sum(bm) / len(bm), 100.0 * (sum(m) / sum(bm) - 1.0), lower, same))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
