"""How the `measured` figures of tests/_stop_cases.py were obtained:  python tests/_stop_spread.py

Runs the oracle on every case with both of its solvers under each of five OpenBLAS kernel sets, each set in a process of its own
(OPENBLAS_CORETYPE is read when the library loads; numpy has to be linked against a DYNAMIC_ARCH OpenBLAS), and prints per
case the largest deviation between any two of the ten runs, per group of quantities, in the form the table holds it.  The ten
runs must agree on status, Iter, trace rows, n_factor and n_solve."""
import itertools
import os
import pickle
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
KERNELS = ("Prescott", "Nehalem", "Sandybridge", "Haswell", "SkylakeX")


def dump(path):
    import _stop_cases as SC
    out = {}
    for name in list(SC.CASES) + list(SC.GROUP_EXTRA):
        for solver in ("qr", SC.case(name).get("second", "2x2")):
            r = SC.oracle_run(name, solver)
            out[name, solver] = dict(y=r.y, w=r.w, v=r.v, counts=SC.counts(r), **{f: getattr(r, f) for f in SC.FIELDS})
    with open(path, "wb") as f:
        pickle.dump(out, f)


def main():
    import _stop_cases as SC
    runs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in KERNELS:
            path = os.path.join(tmp, k)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], check=True, env=dict(os.environ, OPENBLAS_CORETYPE=k))
            with open(path, "rb") as f:
                for (name, solver), rec in pickle.load(f).items():
                    runs.setdefault(name, []).append(types.SimpleNamespace(**rec))
    for name, rs in runs.items():
        assert len({r.counts for r in rs}) == 1, (name, {r.counts for r in rs})
        worst = dict.fromkeys(SC.GROUPS, 0.0)
        for a, b in itertools.permutations(rs, 2):
            for g, v in SC.by_group(SC.deviation(a, b)).items():
                worst[g] = max(worst[g], v)
        print("%-26s measured=(%s)" % (name, ", ".join("%.2g" % worst[g] for g in SC.GROUPS)))


if __name__ == "__main__":
    dump(sys.argv[2]) if sys.argv[1:2] == ["--dump"] else main()
