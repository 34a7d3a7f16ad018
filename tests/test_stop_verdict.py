"""The interior-point loop's stopping verdict (conicip.jl_amd/csrc/cip_driver_scalars.h: evaluate_iteration, apply_certificate,
resolve_options, host_norms) on the CPU, against the oracle's statement of the same block (oracle/conicip.py: evaluate_iteration,
apply_certificate -- the functions the oracle's own loop calls, so tests/test_oracle_kats.py pins them).

tests/stop_verdict/verdict_table.cpp, a stand-alone program under AddressSanitizer / UBSan that includes the header alone, is fed
rows of scalars; the same rows go through the oracle.  Statuses must be equal, every number within 2 ulp (the compiler may
contract `0.5 * yQy - cTy` into an fma), NaN must meet NaN and an infinity its own sign.  The rows: seeded random tuples far from
every threshold, the edges of the block one at a time, exact ties, rows where two or three verdicts hold at once, the options'
derived defaults, and a replayed sequence for the best-iterate bookkeeping.  This is the only place where :Error is reached: no
GPU test feeds the loop non-finite data.  No device call."""
import functools
import inspect
import math
import os
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

from oracle import conicip as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conicip.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "stop_verdict", "verdict_table.cpp")
CLANGXX = os.environ.get("CIP_CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
SAN = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# (a sanitizer runtime that a whole-suite run preloads into python does not go into the child, which links its own; anything
# else LD_PRELOAD names stays.  The child never opens the GPU.)
_PRELOADED_SANITIZER = any(t in os.environ.get("LD_PRELOAD", "") for t in ("clang_rt", "asan", "tsan", "ubsan"))
ENV = dict({k: v for k, v in os.environ.items() if not (k == "LD_PRELOAD" and _PRELOADED_SANITIZER)},
           ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
STATUS = {"None": 0, "Optimal": 1, "Infeasible": 2, "Unbounded": 3, "Error": 5}          # include/cipkkt.h: CIP_STATUS_*
DOTS = ("mubar", "cTy", "r0y2", "r0v2", "r0s2", "yQy", "wr0w", "vr0v", "dTw", "bTv", "pinf2", "yy", "vv", "ays2", "gy2", "qy2")
NORMS = ("normc", "normb", "normd")
SQUARES = ("r0y2", "r0v2", "r0s2", "pinf2", "yy", "vv", "ays2", "gy2", "qy2")
ULPS = 2
MARGIN = 1e-9


def _have_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists(CLANGXX) and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


pytestmark = pytest.mark.skipif(not _have_toolchain(), reason="clang sanitizer runtimes not available")


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "hostsan", "_build", "stop_verdict")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "verdict_table")
    subprocess.run([CLANGXX, "-I", CSRC] + SAN + [SRC, "-o", exe], check=True, capture_output=True, text=True)
    return exe


# ---------------------------------------------------------------------------------------------------------------- rows
OPT = dict(optTol=1e-6, DTB=0.01, infeasTol=1e-6, refinementThreshold=1e-13, maxRefinementSteps=3, maxIters=100)
VEC = dict(y=[1.0, -2.0, 4.0], w=[0.5, -0.25], v=[3.0, 1.0, 2.0])
# four rows that end None / Optimal / Infeasible / Unbounded with every quantity finite and far from its threshold
_NONE = dict(mubar=3.0, cTy=2.0, r0y2=4.0, r0v2=9.0, r0s2=1.0, yQy=5.0, wr0w=0.5, vr0v=-0.25, dTw=1.0, bTv=0.5, pinf2=2.0, yy=16.0,
             vv=4.0, ays2=9.0, gy2=1.0, qy2=25.0, normc=3.0, normb=4.0, normd=2.0)
BASES = {
    "none": _NONE,
    "optimal": dict(_NONE, r0y2=1e-20, r0v2=4e-20, r0s2=9e-22, cTy=-2.0),
    "infeasible": dict(_NONE, dTw=-2.0, bTv=1.0, pinf2=1e-20),
    "unbounded": dict(_NONE, ays2=1e-20, gy2=4e-20, qy2=9e-22),
}


def row(name, base, m=3, p=2, conedim=None, opt=OPT, Iter=1, reset=1, optBest0=math.inf, has_trace=1, expect=None, **over):
    vals = dict(BASES[base] if isinstance(base, str) else base, **over)
    assert set(vals) == set(DOTS) | set(NORMS), set(vals) ^ (set(DOTS) | set(NORMS))
    if p == 0 and "normd" not in over:
        vals["normd"] = -math.inf                      # the loop's value without equalities (src/ConicIP.jl:532)
    return dict(name=name, dots=[float(vals[k]) for k in DOTS], norms=[float(vals[k]) for k in NORMS],
                conedim=float((m if m > 0 else 0) if conedim is None else conedim), m=m, p=p, opt=opt, Iter=Iter, reset=reset,
                optBest0=optBest0, has_trace=has_trace, expect=expect, y=VEC["y"], w=VEC["w"][:min(p, 2)], v=VEC["v"][:min(m, 3)])


def edge_rows():
    rows = [row("base %s" % b, b, expect=b.capitalize()) for b in BASES]
    for b in BASES:
        rows.append(row("m == 0 / %s" % b, b, m=0))
        rows.append(row("p == 0 / %s" % b, b, p=0))
        rows.append(row("m == 0 and p == 0 / %s" % b, b, m=0, p=0))                 # the :790 skip
        rows.append(row("conedim == 0 / %s" % b, b, conedim=0))                     # mu NaN
        rows.append(row("normd = -inf with p == 0 / %s" % b, b, p=0, normd=-math.inf))
        rows.append(row("no trace / %s" % b, b, has_trace=0, Iter=7))
    tiny = 5e-324
    for pinf2 in (0.0, 1e-20):
        rows.append(row("dTw - bTv == 0, pinf2 %g" % pinf2, "infeasible", dTw=1.0, bTv=1.0, pinf2=pinf2))
        rows.append(row("dTw - bTv == +tiny, pinf2 %g" % pinf2, "infeasible", dTw=tiny, bTv=0.0, pinf2=pinf2))
        rows.append(row("dTw - bTv == -tiny, pinf2 %g" % pinf2, "infeasible", dTw=0.0, bTv=tiny, pinf2=pinf2))
        rows.append(row("|y| + |v| == 0, pinf2 %g" % pinf2, "infeasible", yy=0.0, vv=0.0, pinf2=pinf2))
        rows.append(row("|y| == 0 (primal), pinf2 %g" % pinf2, "infeasible", yy=0.0, pinf2=pinf2))
    rows.append(row("dTw - bTv == -0.0", "infeasible", dTw=-0.0, bTv=0.0))
    for cTy in (0.0, -0.0, -2.0, tiny, -tiny):
        rows.append(row("cTy == %r" % cTy, "unbounded", cTy=cTy))
    rows.append(row("|y| == 0 (dual)", "unbounded", yy=0.0))
    rows.append(row("|y| == 0 (dual), zero residuals", "unbounded", yy=0.0, ays2=0.0, gy2=0.0, qy2=0.0))
    rows.append(row("|y| + |v| == 0 (dual)", "unbounded", yy=0.0, vv=0.0))
    for b in BASES:                                    # NaN and +-inf, one slot at a time: where :Error is reached
        for slot in DOTS + NORMS:
            for bad in (math.nan, math.inf, -math.inf):
                rows.append(row("%s = %r / %s" % (slot, bad, b), b, **{slot: bad}))
        for slot in SQUARES:                           # nrm of a negative square is NaN
            rows.append(row("%s = -1 / %s" % (slot, b), b, **{slot: -1.0}))
    return rows


def tie_rows():
    """exactly representable: optTol = infeasTol = 2^-10, every norm of the data 1, so rDu = |r0.y| / 2, p_ecos = |pinf| / |dTy_bTv|
    and d_cvx = d1 / cTy; the neighbour one ulp below the tie takes the verdict, the tie itself does not (strict <)"""
    t = 2.0 ** -10
    opt = dict(OPT, optTol=t, infeasTol=t)
    below = lambda x: math.nextafter(x, 0.0)
    base = dict(_NONE, normc=1.0, normb=1.0, normd=1.0, r0y2=4.0, r0v2=1.0, r0s2=1.0, yy=4.0, vv=4.0)
    o = dict(base, r0y2=4 * t * t, r0v2=t * t, r0s2=t * t, cTy=-1.0)           # rDu = 2t / 2 = t, rPr = t / 2, rCp = t / 2
    i = dict(base, dTw=-1.0, bTv=0.0, pinf2=t * t)                             # p_ecos = t, p_cvx = t / 4
    u = dict(base, cTy=1.0, ays2=t * t, gy2=t * t / 4, qy2=t * t / 16)         # d_cvx = t, d_ecos = t / 2
    return [row("tie worst == optTol", o, opt=opt, expect="None"),
            row("below worst == optTol", dict(o, r0y2=below(4 * t * t)), opt=opt, expect="Optimal"),
            row("tie p_infeas == infeasTol", i, opt=opt, expect="None"),
            row("below p_infeas == infeasTol", dict(i, pinf2=below(t * t)), opt=opt, expect="Infeasible"),
            row("tie d_infeas == infeasTol", u, opt=opt, expect="None"),
            row("below d_infeas == infeasTol", dict(u, ays2=below(t * t)), opt=opt, expect="Unbounded")]


_ALL3 = dict(BASES["optimal"], cTy=2.0, dTw=-2.0, bTv=1.0, pinf2=1e-20, ays2=1e-20, gy2=4e-20, qy2=9e-22)
PRECEDENCE = {
    # name: (the row, its verdict, {what is switched off: the verdict that is left})
    "Optimal with Infeasible": (dict(BASES["optimal"], dTw=-2.0, bTv=1.0, pinf2=1e-20), "Infeasible",
                                {("dTw",): "Optimal", ("r0y2",): "Infeasible"}),
    "Optimal with Unbounded": (dict(BASES["optimal"], cTy=2.0, ays2=1e-20, gy2=4e-20, qy2=9e-22), "Unbounded",
                               {("ays2",): "Optimal", ("r0y2",): "Unbounded"}),
    "Optimal with Infeasible with Unbounded": (_ALL3, "Infeasible", {("dTw",): "Unbounded", ("dTw", "ays2"): "Optimal",
                                                                      ("dTw", "r0y2"): "Unbounded", ("r0y2", "ays2"): "Infeasible"}),
    "Infeasible with Unbounded": (dict(_ALL3, r0y2=4.0), "Infeasible", {("dTw",): "Unbounded", ("ays2",): "Infeasible"}),
}
_OFF = dict(dTw=1.0, r0y2=4.0, ays2=9.0)               # no primal certificate / not optimal / no dual certificate


def precedence_rows():
    rows = []
    for name, (vals, verdict, off) in PRECEDENCE.items():
        rows.append(row(name, vals, expect=verdict))
        for slots, left in off.items():
            rows.append(row("%s without %s" % (name, "+".join(slots)), dict(vals, **{s: _OFF[s] for s in slots}), expect=left))
    return rows


def option_rows():
    certifiable = dict(BASES["infeasible"], pinf2=0.0)
    return [row("infeasTol < 0 and refinementThreshold < 0", "infeasible", opt=dict(OPT, optTol=1e-4, infeasTol=-1.0, refinementThreshold=-1.0),
                pinf2=1e-9, expect="Infeasible"),       # p_infeas 3.5e-6: below the derived 1e-4, above the 1e-6 of a lost default
            row("infeasTol < 0 only", "none", opt=dict(OPT, optTol=1e-8, infeasTol=-3.0)),
            row("refinementThreshold < 0 only", "none", opt=dict(OPT, optTol=1e-3, refinementThreshold=-1e-300)),
            row("infeasTol == 0.0 never certifies (primal)", certifiable, opt=dict(OPT, infeasTol=0.0), expect="None"),
            row("infeasTol == 0.0 never certifies (dual)", "unbounded", opt=dict(OPT, infeasTol=0.0), ays2=0.0, gy2=0.0, qy2=0.0, expect="None"),
            row("infeasTol == -0.0", certifiable, opt=dict(OPT, infeasTol=-0.0), expect="None"),
            row("infeasTol > 0 certifies the same row", certifiable, expect="Infeasible"),
            row("opt == NULL", "optimal", opt=None, expect="Optimal"),
            row("opt == NULL, between the default and a wider optTol", "none", opt=None, r0y2=1e-8, r0v2=1e-8, r0s2=1e-8, expect="None"),
            row("options go through unchanged", "none", opt=dict(optTol=1e-3, DTB=0.5, infeasTol=1e-2, refinementThreshold=0.0,
                                                                 maxRefinementSteps=0, maxIters=7))]


def sequence_rows():
    """worst falls, rises, ties, falls: the best iterate is the one of row 2 until row 5 -- a tie does not replace it.  Every row
    has its own mubar, so a wrong row would show in Mu as well"""
    worst = [1e-1, 1e-2, 1e-1, 1e-2, 1e-3, 1e-3]
    rows = []
    for i, w in enumerate(worst):
        r0y2 = (w * 4.0) ** 2                          # rDu = sqrt(r0y2) / (1 + 3); rPr and rCp stay below it
        rows.append(row("sequence row %d" % (i + 1), "none", reset=int(i == 0), Iter=i + 1, mubar=3.0 / (i + 1),
                        r0y2=r0y2, r0v2=r0y2 / 100, r0s2=r0y2 / 100, yQy=5.0 + i, expect="None"))
    return rows, [1, 2, 2, 2, 5, 5]


def _spread(rng, lo=-20.0, hi=20.0):
    return 10.0 ** rng.uniform(lo, hi)


def _draw(rng, want):
    """one tuple with the dots log-spread over 1e-20 .. 1e20, the squares and mubar positive; `want` only biases the draw towards
    a verdict -- what the row is counted as is what the oracle says"""
    # (:Error out of finite data: without cones conedim is 0 and mu = 0 / 0)
    m, p = [(3, 2), (3, 0), (0, 2), (5, 1)][rng.integers(0, 4)] if want != "Error" else (0, int(rng.integers(1, 3)))
    vals = {k: _spread(rng) for k in DOTS + NORMS}
    for k in ("cTy", "wr0w", "vr0v", "dTw", "bTv"):
        vals[k] *= rng.choice([-1.0, 1.0])
    small = lambda: _spread(rng, -20.0, -13.0)
    if want == "Optimal":
        vals.update(r0y2=small(), r0v2=small(), r0s2=small(), dTw=abs(vals["dTw"]), bTv=-abs(vals["bTv"]), cTy=-abs(vals["cTy"]))
    elif want == "Infeasible":
        vals.update(dTw=-_spread(rng, 0, 20), bTv=_spread(rng, -20, 20), pinf2=small(), yy=_spread(rng, 0, 20))
    elif want == "Unbounded":
        vals.update(dTw=abs(vals["dTw"]), bTv=-abs(vals["bTv"]), cTy=_spread(rng, 0, 20), ays2=small(), gy2=small(), qy2=small(),
                    yy=_spread(rng, 0, 20))
    opt = dict(OPT, optTol=[1e-6, 1e-9, 1e-3][rng.integers(0, 3)], infeasTol=[1e-6, 1e-3, 1e-9, -1.0][rng.integers(0, 4)])
    r = row("random", vals, m=m, p=p, conedim=int(rng.integers(1, m + 1)) if m else 0, opt=opt, Iter=int(rng.integers(1, 100)),
            optBest0=[math.inf, _spread(rng, -12, 3)][rng.integers(0, 2)])
    r["y"], r["w"], r["v"] = (list(rng.standard_normal(k) * _spread(rng, -3, 3)) for k in (3, len(r["w"]), len(r["v"])))
    return r


def _margin_ok(r):
    """no verdict of the row within 1e-9 relative of its threshold (the oracle alone decides)"""
    o = _resolve(r["opt"])
    vd = O.evaluate_iteration(r["dots"], *r["norms"], r["conedim"], r["m"], r["p"], o["optTol"], o["infeasTol"], r["Iter"], r["optBest0"])
    worst = O._jlmax(O._jlmax(vd.rDu, vd.rPr), vd.rCp)
    far = lambda x, t: not (math.isfinite(x) and math.isfinite(t)) or abs(x - t) > MARGIN * max(abs(x), abs(t))
    dTy = r["dots"][8] - r["dots"][9]
    return (far(worst, o["optTol"]) and far(worst, r["optBest0"]) and far(vd.p_infeas, o["infeasTol"]) and far(vd.d_infeas, o["infeasTol"])
            and dTy != 0.0 and r["dots"][1] != 0.0)


@functools.lru_cache(maxsize=None)
def random_rows():
    rng = np.random.default_rng(20240611)
    rows, redrawn = [], 0
    for want in ("None", "Optimal", "Infeasible", "Unbounded", "Error"):
        got = 0
        while got < 60:
            r = _draw(rng, want)
            if not _margin_ok(r):
                redrawn += 1
                continue
            r["name"] = "random %d (drawn for %s)" % (len(rows), want)
            rows.append(r)
            got += 1
    return rows, redrawn


# ---------------------------------------------------------------------------------------------------------------- the two sides
def _resolve(opt):
    """the options as the reference's signature resolves them (src/ConicIP.jl:498-509; the oracle's conicIP carries the defaults)"""
    dflt = {k: v.default for k, v in inspect.signature(O.conicIP).parameters.items() if v.default is not inspect.Parameter.empty}
    o = dict(optTol=dflt["optTol"], DTB=dflt["DTB"], infeasTol=-1.0, refinementThreshold=-1.0,
             maxRefinementSteps=dflt["maxRefinementSteps"], maxIters=dflt["maxIters"]) if opt is None else dict(opt)
    assert dflt["infeasTol"] is None and dflt["refinementThreshold"] is None
    if o["infeasTol"] < 0:
        o["infeasTol"] = o["optTol"]                   # :506
    if o["refinementThreshold"] < 0:
        o["refinementThreshold"] = o["optTol"] / 1e7   # :509
    return o


def _seq_norm(x):
    s = 0.0
    for t in x:
        s += t * t
    return math.sqrt(s)


def oracle_side(rows):
    out, st, best = [], None, math.inf
    for r in rows:
        if r["reset"]:
            st = dict(iter=0, resmu=0.0, prFeas=math.inf, duFeas=math.inf, muFeas=math.inf, pobj=math.inf, dobj=-math.inf, trace_rows=0)
            best = r["optBest0"]
        o = _resolve(r["opt"])
        vd = O.evaluate_iteration(r["dots"], *r["norms"], r["conedim"], r["m"], r["p"], o["optTol"], o["infeasTol"], r["Iter"], best)
        best = vd.optBest
        if vd.improved:
            st.update(iter=r["Iter"], resmu=vd.mu, prFeas=vd.rPr, duFeas=vd.rDu, muFeas=vd.rCp)
        st.update(pobj=vd.pobj, dobj=vd.dobj)
        if r["has_trace"]:
            st["trace_rows"] = r["Iter"]
        y, w, v = O.apply_certificate(vd.status, vd.scale, np.array(r["y"]), np.array(r["w"]), np.array(r["v"]))
        out.append(dict(st, status=STATUS[vd.status], scale=vd.scale, mu=vd.mu, mubar=r["dots"][0], optBest=best,
                        tr=[float(r["Iter"]), vd.mu, vd.rDu, vd.rPr, vd.rCp, vd.pobj, vd.dobj, math.nan, math.nan] if r["has_trace"] else [-1.0] * 9,
                        hn=[_seq_norm(r["y"]), _seq_norm(r["v"]), _seq_norm(r["w"]) if r["w"] else -math.inf],
                        y=list(y), w=list(w), v=list(v), verdict=vd,
                        opt=[o["optTol"], o["DTB"], o["infeasTol"], o["refinementThreshold"], o["maxRefinementSteps"], o["maxIters"], 0]))
    return out


def _num(x):
    return float(x).hex() if math.isfinite(x) else repr(float(x))


def program_side(rows):
    lines = []
    for r in rows:
        o = r["opt"] if r["opt"] is not None else dict(optTol=-7.0, DTB=-7.0, infeasTol=-7.0, refinementThreshold=-7.0, maxRefinementSteps=-7, maxIters=-7)
        f = ([r["reset"], r["optBest0"], r["has_trace"]] + r["dots"] + r["norms"] + [r["conedim"], r["m"], r["p"], int(r["opt"] is not None)]
             + [o[k] for k in ("optTol", "DTB", "infeasTol", "refinementThreshold", "maxRefinementSteps", "maxIters")]
             + [r["Iter"], len(r["y"]), len(r["w"]), len(r["v"])] + r["y"] + r["w"] + r["v"])
        lines.append(" ".join(_num(x) for x in f))
    run = subprocess.run([_exe()], input="\n".join(lines) + "\n", env=ENV, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
    out = []
    for line in run.stdout.splitlines():
        d = dict(kv.split("=", 1) for kv in line.split(" "))
        rec = {}
        for k, s in d.items():
            if k in ("status", "iter", "trace_rows"):
                rec[k] = int(s)
            elif k in ("tr", "hn", "y", "w", "v"):
                rec[k] = [float.fromhex(t) for t in s.split(",") if t]
            elif k == "opt":
                rec[k] = [float(t) for t in s.split(",")]
            else:
                rec[k] = float.fromhex(s)
        out.append(rec)
    assert len(out) == len(rows), (len(out), len(rows))
    return out


def _ordered(x):
    i = struct.unpack("<q", struct.pack("<d", x))[0]
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


def close(a, b, ulps=ULPS):
    if a != a or b != b:
        return a != a and b != b                       # NaN meets NaN
    if math.isinf(a) or math.isinf(b):
        return a == b                                  # and an infinity its own sign
    return abs(_ordered(a) - _ordered(b)) <= ulps


def compare(rows):
    """every field of every row; returns the oracle's records"""
    want, got = oracle_side(rows), program_side(rows)
    for r, w, g in zip(rows, want, got):
        for k in ("status", "iter", "trace_rows"):
            assert g[k] == w[k], (r["name"], k, g[k], w[k])
        for k in ("scale", "mu", "mubar", "resmu", "prFeas", "duFeas", "muFeas", "pobj", "dobj", "optBest"):
            assert close(g[k], w[k]), (r["name"], k, g[k], w[k])
        for k in ("tr", "hn", "y", "w", "v", "opt"):
            assert len(g[k]) == len(w[k]), (r["name"], k, g[k], w[k])
            for a, b in zip(g[k], w[k]):
                assert close(a, b, 0 if k == "opt" else ULPS), (r["name"], k, g[k], w[k])
        if r["expect"] is not None:
            assert w["verdict"].status == r["expect"], (r["name"], w["verdict"].status, r["expect"])
    return want


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_the_comparison_itself():
    assert close(math.nan, math.nan) and not close(math.nan, 1.0) and not close(math.inf, -math.inf) and close(-math.inf, -math.inf)
    assert close(1.0, 1.0 + 2 ** -51) and not close(1.0, 1.0 + 2 ** -50) and close(0.0, -0.0) and close(5e-324, -5e-324)
    assert not close(math.inf, 1.7976931348623157e308)
    assert float.fromhex("-nan") != float.fromhex("-nan") and float.fromhex("-inf") == -math.inf


def test_random_rows():
    rows, redrawn = random_rows()
    want = compare(rows)
    seen = Counter(w["verdict"].status for w in want)
    print("random rows: %d, redrawn for the margin: %d, statuses %s" % (len(rows), redrawn, dict(seen)))
    assert len(rows) >= 300 and all(seen[s] >= 20 for s in STATUS), seen
    assert all(_margin_ok(r) for r in rows)
    # both certificates, both signs of the objective terms, with and without either block
    assert {(r["m"] > 0, r["p"] > 0) for r in rows} >= {(True, True), (True, False), (False, True)}
    assert sum(1 for w in want if w["verdict"].improved) >= 20 and sum(1 for w in want if not w["verdict"].improved) >= 20


def test_edge_rows():
    rows = edge_rows()
    want = compare(rows)
    seen = Counter(w["verdict"].status for w in want)
    print("edge rows: %d, statuses %s" % (len(rows), dict(seen)))
    by = {r["name"]: w["verdict"] for r, w in zip(rows, want)}
    assert len(by) == len(rows)                        # every edge has its own name
    assert all(seen[s] > 0 for s in STATUS), seen
    # what the edges are there for, on the oracle's side
    for b in BASES:
        assert math.isnan(by["conedim == 0 / %s" % b].mu) and math.isnan(by["m == 0 / %s" % b].mu)
        skipped = by["m == 0 and p == 0 / %s" % b]
        assert skipped.status == ("Optimal" if b == "optimal" else "Error") and math.isnan(skipped.p_infeas) and math.isnan(skipped.d_infeas)
    assert by["conedim == 0 / none"].status == "Error" and by["conedim == 0 / infeasible"].status == "Infeasible"
    assert by["m == 0 / unbounded"].status == "Unbounded" and by["p == 0 / unbounded"].status == "Unbounded"     # d1 / d2 = -inf drop out
    assert by["dTw - bTv == 0, pinf2 0"].status == by["dTw - bTv == +tiny, pinf2 0"].status == by["dTw - bTv == -0.0"].status == "None"
    tiny = by["dTw - bTv == -tiny, pinf2 0"]
    assert tiny.status == "Infeasible" and tiny.scale == 5e-324 and by["dTw - bTv == -tiny, pinf2 1e-20"].status == "None"
    assert all(by["cTy == %r" % c].status == "None" for c in (0.0, -0.0, -2.0, -5e-324)) and by["cTy == 5e-324"].status == "None"
    assert by["|y| + |v| == 0, pinf2 0"].status == "None" and by["|y| + |v| == 0, pinf2 1e-20"].status == "None"           # 0 / 0 and x / 0
    assert by["|y| == 0 (primal), pinf2 1e-20"].status == "Infeasible"
    assert by["|y| == 0 (dual)"].status == "None" and by["|y| == 0 (dual), zero residuals"].status == "None"
    for slot in ("r0y2", "r0v2", "r0s2"):              # NaN propagates through the max; a negative square has no norm
        for bad in ("nan", "inf"):
            assert by["%s = %s / none" % (slot, bad)].status == "Error", (slot, bad)
        assert by["%s = -1 / none" % slot].status == "Error" and by["%s = -1 / optimal" % slot].status == "Error"
    assert by["mubar = nan / none"].status == "Error" and by["mubar = nan / optimal"].status == "Optimal"
    assert by["normc = nan / infeasible"].status == "Error" and by["normc = nan / unbounded"].status == "Error"
    assert by["pinf2 = -1 / infeasible"].status == "None" and by["ays2 = -1 / unbounded"].status == "None"
    assert by["r0y2 = nan / infeasible"].status == "Infeasible"                     # a certificate does not look at the residuals
    print("every edge row exercised: %d" % len(rows))


def test_ties_are_not_verdicts():
    rows = tie_rows()
    want = compare(rows)
    t = 2.0 ** -10
    v = {r["name"]: w["verdict"] for r, w in zip(rows, want)}
    assert max(v["tie worst == optTol"].rDu, v["tie worst == optTol"].rPr, v["tie worst == optTol"].rCp) == t
    assert v["tie p_infeas == infeasTol"].p_infeas == t and v["tie d_infeas == infeasTol"].d_infeas == t
    assert v["below p_infeas == infeasTol"].p_infeas < t and v["below d_infeas == infeasTol"].d_infeas < t


def test_precedence_of_the_verdicts():
    rows = precedence_rows()
    compare(rows)                                      # `expect` of every row: the verdict, and what is left when one is switched off
    names = [r["name"] for r in rows]
    assert all(n in names for n in PRECEDENCE)
    print("precedence rows exercised: %s" % ", ".join(PRECEDENCE))


def test_options():
    rows = option_rows()
    want = compare(rows)
    by = {r["name"]: w for r, w in zip(rows, want)}
    assert by["opt == NULL"]["opt"] == [1e-6, 0.01, 1e-6, 1e-6 / 1e7, 3, 100, 0]
    assert by["infeasTol < 0 and refinementThreshold < 0"]["opt"][2:4] == [1e-4, 1e-4 / 1e7]
    assert by["infeasTol < 0 only"]["opt"][2:4] == [1e-8, 1e-13] and by["refinementThreshold < 0 only"]["opt"][2:4] == [1e-6, 1e-3 / 1e7]
    assert by["infeasTol == 0.0 never certifies (primal)"]["verdict"].p_infeas == 0.0
    assert by["infeasTol == 0.0 never certifies (dual)"]["verdict"].d_infeas == 0.0
    assert by["options go through unchanged"]["opt"] == [1e-3, 0.5, 1e-2, 0.0, 0, 7, 0]


def test_best_iterate_bookkeeping():
    rows, best_iter = sequence_rows()
    want = compare(rows)
    assert [w["iter"] for w in want] == best_iter
    assert [w["verdict"].improved for w in want] == [True, True, False, False, True, False]
    assert want[3]["verdict"].optBest == want[1]["verdict"].optBest and want[3]["resmu"] == want[1]["mu"] != want[3]["mu"]
    assert [w["trace_rows"] for w in want] == [1, 2, 3, 4, 5, 6]
