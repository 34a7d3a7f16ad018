"""The small-problem batch path (cip_conicip_small, include/cipkkt.h), CPU only: the entry points are declared, exported and
bound; the Python keyword exists and defaults to off; `small_fits` answers every rule at its edge without a GPU; the argument
rules that need no device hold; and the host side of the call -- compiled host-only and linked against the fake HIP runtime of
tests/hostsan -- runs under AddressSanitizer / UBSan (tests/small/drive_small.cpp, a stand-alone program)."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("cip_conicip_small_fits", "cip_conicip_small", "cip_small_stats")


def test_entry_points_are_declared_exported_and_bound():
    from cipkkt import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cipkkt.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, header), f
        assert hasattr(lib, f), f
        assert f in _lib.SIGNATURES, f
    assert re.search(r"#define\s+CIP_SMALL_MAX_N\s+128\b", header) and re.search(r"#define\s+CIP_SMALL_MAX_M\s+1024\b", header)
    # the same parameter list as cip_conicip_lockstep; neither a handle nor a stream (tests/test_stream_table.py)
    assert _lib.SIGNATURES["cip_conicip_small"] == _lib.SIGNATURES["cip_conicip_lockstep"]
    decl = re.search(r"int\s+cip_conicip_small\s*\(([^)]*)\)", header).group(1)
    assert "cip_handle" not in decl and "hip_stream" not in decl
    assert "small.hip" in open(os.path.join(ROOT, "conicip.jl_amd", "build.py")).read()


def test_python_keyword_exists_and_defaults_to_off():
    import cipkkt
    from cipkkt import batch, kkt
    par = inspect.signature(batch.solve_batch).parameters
    assert "small" in par and par["small"].default is False
    assert cipkkt.small_fits is batch.small_fits and callable(batch.solve_small)
    assert list(inspect.signature(cipkkt.small_fits).parameters)[:4] == ["Q", "A", "G", "cone_dims"]
    # make_problem keeps its signature and its three return values
    assert list(inspect.signature(kkt.make_problem).parameters) == ["Q", "A", "G", "cone_dims", "route", "device", "sparse_q"]
    pr, keep, a_sparse = kkt.make_problem(sp.identity(3, format="csr"), sp.identity(3, format="csr"), None, [("R", 3)], "schur", "cpu",
                                          sparse_q=True)
    assert a_sparse is True


def _dense(n, m, p, cones=None):
    """(Q, A, G, cone_dims) of the given dimensions"""
    return np.eye(n), np.ones((m, n)), (np.ones((p, n)) if p else None), (cones if cones is not None else ([("R", m)] if m else []))


# (label, description) of everything the path refuses with CIP_E_UNSUPPORTED: (Q, A, G, cone_dims, route) and struct edits
REFUSED = [
    ("n + p = 129", lambda: (_dense(100, 8, 29), "schur", None)),
    ("n = 129", lambda: (_dense(129, 8, 0), "schur", None)),
    ("m = 1025", lambda: (_dense(4, 1025, 0), "schur", None)),
    ("an S cone", lambda: (_dense(6, 8, 1, [("R", 5), ("S", 3)]), "schur", None)),
    ("a CSR A", lambda: ((np.eye(6), sp.random(8, 6, density=0.5, format="csr", random_state=0), None, [("R", 8)]), "schur", None)),
    ("CIP_FLAG_Q_CSR", lambda: (_dense(6, 8, 1), "schur", "q_csr")),
    ("the full 3x3 route", lambda: (_dense(6, 8, 1), "full3x3", None)),
]
TAKEN = [
    ("n + p = 128", lambda: (_dense(100, 8, 28), "schur", None)),
    ("n = 128", lambda: (_dense(128, 0, 0), "schur", None)),
    ("m = 1024", lambda: (_dense(4, 1024, 0), "schur", None)),
    ("Q cones of any dimension", lambda: (_dense(6, 204, 1, [("Q", 1), ("Q", 200), ("R", 3)]), "schur", None)),
    ("m = 0 and p = 0", lambda: (_dense(5, 0, 0), "schur", None)),
]


def description(make):
    """the cip_problem (host pointers) of a table entry, with its keep-alive list"""
    from cipkkt import _lib as L, batch
    (Q, A, G, cones), route, edit = make()
    st, keep = batch._host_problem(Q, A, G, cones, route)
    if edit == "q_csr":
        rp, ci, va = np.arange(st.n + 1, dtype=np.int32), np.arange(st.n, dtype=np.int32), np.ones(st.n)
        keep += [rp, ci, va]
        st.Q, st.flags = None, st.flags | L.FLAG_Q_CSR
        st.Q_rowptr, st.Q_colind, st.Q_val = (C.c_void_p(x.ctypes.data) for x in (rp, ci, va))
    return st, keep


def test_small_fits_rule_table():
    import cipkkt
    from cipkkt import _lib as L
    lib = L.load()
    for label, make in REFUSED:
        st, keep = description(make)
        assert lib.cip_conicip_small_fits(C.byref(st)) == L.E_UNSUPPORTED, label
        assert lib.cip_last_error(), label
        (Q, A, G, cones), route, edit = make()
        if edit is None:
            assert cipkkt.small_fits(Q, A, G, cones, route) is False and cipkkt.small_fits.reason, label
    for label, make in TAKEN:
        st, keep = description(make)
        assert lib.cip_conicip_small_fits(C.byref(st)) == 0, (label, lib.cip_last_error())
        (Q, A, G, cones), route, _ = make()
        assert cipkkt.small_fits(Q, A, G, cones, route) is True, label
    # the messages name the rule
    st, keep = description(REFUSED[0][1])
    lib.cip_conicip_small_fits(C.byref(st))
    assert b"CIP_SMALL_MAX_N" in lib.cip_last_error()
    st, keep = description(REFUSED[2][1])
    lib.cip_conicip_small_fits(C.byref(st))
    assert b"CIP_SMALL_MAX_M" in lib.cip_last_error()


def test_argument_rules_that_need_no_device():
    """CIP_E_INVALID (-1) before any allocation; a refused batch returns CIP_E_UNSUPPORTED before it, too: no GPU is needed here"""
    from cipkkt import _lib as L
    lib = L.load()
    st, keep = description(TAKEN[0][1])
    k = 2
    arr = (L.CipProblem * k)(st, st)
    vp = C.c_void_p * k
    vec = np.ones(1024)
    ptrs = vp(vec.ctypes.data, vec.ctypes.data)
    res = (L.CipResult * k)()
    assert lib.cip_conicip_small(-1, arr, ptrs, ptrs, ptrs, None, ptrs, ptrs, ptrs, res) == -1
    assert lib.cip_conicip_small(k, None, ptrs, ptrs, ptrs, None, ptrs, ptrs, ptrs, res) == -1
    assert lib.cip_conicip_small(k, arr, None, ptrs, ptrs, None, ptrs, ptrs, ptrs, res) == -1
    assert lib.cip_conicip_small(k, arr, ptrs, None, ptrs, None, ptrs, ptrs, ptrs, res) == -1            # m > 0 and no b
    assert lib.cip_conicip_small(k, arr, ptrs, ptrs, ptrs, None, ptrs, None, ptrs, res) == -1            # p > 0 and no w
    assert lib.cip_conicip_small(k, arr, ptrs, ptrs, ptrs, None, ptrs, ptrs, ptrs, None) == -1
    assert lib.cip_conicip_small(k, arr, vp(vec.ctypes.data, None), ptrs, ptrs, None, ptrs, ptrs, ptrs, res) == -1
    assert lib.cip_conicip_small(0, None, None, None, None, None, None, None, None, None) == 0            # count 0: a no-op
    out = (C.c_int * 4)(9, 9, 9, 9)
    assert lib.cip_small_stats(out) == 0 and list(out) == [0, 0, 0, 0]
    assert lib.cip_small_stats(None) == -1 and lib.cip_conicip_small_fits(None) == -1
    # cones that do not cover m, a leading dimension below its row count
    bad, keep2 = description(TAKEN[0][1])
    bad.m = 9
    assert lib.cip_conicip_small_fits(C.byref(bad)) == -1
    bad, keep3 = description(TAKEN[0][1])
    bad.lda = 7
    assert lib.cip_conicip_small_fits(C.byref(bad)) == -1
    # a refused description and one of another shape in the batch: CIP_E_UNSUPPORTED
    big, keep4 = description(REFUSED[0][1])
    assert lib.cip_conicip_small(k, (L.CipProblem * k)(st, big), ptrs, ptrs, ptrs, None, ptrs, ptrs, ptrs, res) == L.E_UNSUPPORTED
    other, keep5 = description(TAKEN[2][1])
    assert lib.cip_conicip_small(k, (L.CipProblem * k)(st, other), ptrs, ptrs, ptrs, None, ptrs, ptrs, ptrs, res) == L.E_UNSUPPORTED
    assert b"differs in shape" in lib.cip_last_error()


def test_solve_batch_bins_without_a_gpu():
    """the binning of solve_batch(small=True) is host work: shapes that fit, shapes that do not, and problems of one shape together"""
    from cipkkt import batch
    mk = lambda n, m, sparse=False: dict(Q=np.eye(n), c=np.ones(n), A=(sp.identity(m, format="csr") if sparse else np.ones((m, n))), b=np.zeros(m),
                                         cone_dims=[("R", m)])
    probs = [mk(4, 4), mk(200, 8), mk(4, 4), mk(4, 4, sparse=True), mk(5, 4)]
    bins = batch._small_bins(probs, range(len(probs)))
    assert sorted((fits, idx) for fits, idx in bins) == [(False, [1]), (False, [3]), (True, [0, 2]), (True, [4])]


def _have_hostsan_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists("/opt/rocm/bin/hipcc") and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


@pytest.mark.skipif(not _have_hostsan_toolchain(), reason="hipcc / clang sanitizer runtimes not available")
def test_host_side_on_the_fake_runtime():
    spec = importlib.util.spec_from_file_location("cip_build_hostsan", os.path.join(ROOT, "tests", "hostsan", "build_hostsan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe, env = mod.build("asan")
    out = os.path.dirname(exe)
    so = os.path.join(out, "libcipkkt_host_asan.so")
    drv = os.path.join(out, "drive_small")
    subprocess.run([mod.CLANGXX, "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "small", "drive_small.cpp"), so,
                    "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "drive_small: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
