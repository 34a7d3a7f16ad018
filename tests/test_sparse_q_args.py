"""The CSR objective matrix (CIP_FLAG_Q_CSR, include/cipkkt.h), CPU only: the flag and the three fields exist in the bindings,
the Python layers take `sparse_q`, and the level-1 check -- compiled host-only and linked against the fake HIP runtime of
tests/hostsan -- refuses every violation with CIP_E_INVALID and a message naming the first offending entry before any device
allocation, then runs valid matrices through create / cip_update_problem / destroy (tests/sparseq/drive_args.cpp, a stand-alone
program under AddressSanitizer / UBSan)."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_and_fields_are_bound():
    from cipkkt import _lib
    assert _lib.FLAG_Q_CSR == 4
    names = [f[0] for f in _lib.CipProblem._fields_]
    assert names[-3:] == ["Q_rowptr", "Q_colind", "Q_val"]                 # at the END: the old struct is a prefix of the new one
    assert names.index("flags") == len(names) - 4
    assert all(f[1] is ctypes.c_void_p for f in _lib.CipProblem._fields_[-3:])
    header = open(os.path.join(ROOT, "include", "cipkkt.h")).read()
    assert re.search(r"#define\s+CIP_FLAG_Q_CSR\s+4\b", header)
    flags = {int(v) for v in re.findall(r"#define\s+CIP_FLAG_\w+\s+(\d+)", header)}
    assert flags == {1, 2, 4}


def test_python_layers_take_the_keyword_and_default_to_dense():
    import cipkkt
    from cipkkt import batch, driver, kkt
    for fn in (kkt.make_problem, kkt.KKTSystem.__init__, kkt.kktsolver_hip, kkt.kktsolver_2x2_hip, kkt.kktsolver_hip_full3x3,
               driver.conicIP, batch.solve_batch, batch._solve_many_native, batch._solve_problems_native):
        par = inspect.signature(fn).parameters
        assert "sparse_q" in par and par["sparse_q"].default is False, fn
    assert cipkkt.conicIP is driver.conicIP


def test_make_problem_hands_over_host_csr_arrays():
    """no GPU needed for a CSR Q with a CSR A and no G: nothing is staged on the device"""
    import numpy as np
    import scipy.sparse as sp
    from cipkkt import _lib, kkt
    Q = sp.csr_matrix(np.array([[2.0, 0, 1.0], [0, 0, 0], [1.0, 0, 3.0]]))
    Q = Q[:, ::-1][:, ::-1]                                     # (whatever order scipy left the indices in)
    pr, keep, a_sparse = kkt.make_problem(Q, sp.identity(3, format="csr"), None, [("R", 3)], "schur", "cpu", sparse_q=True)
    assert a_sparse and pr.Q is None and pr.flags & _lib.FLAG_Q_CSR and pr.flags & _lib.FLAG_CSR_HOST
    rp = np.ctypeslib.as_array(ctypes.cast(pr.Q_rowptr, ctypes.POINTER(ctypes.c_int32)), (4,))
    ci = np.ctypeslib.as_array(ctypes.cast(pr.Q_colind, ctypes.POINTER(ctypes.c_int32)), (4,))
    va = np.ctypeslib.as_array(ctypes.cast(pr.Q_val, ctypes.POINTER(ctypes.c_double)), (4,))
    assert rp.tolist() == [0, 2, 2, 4] and ci.tolist() == [0, 2, 0, 2] and va.tolist() == [2.0, 1.0, 1.0, 3.0]
    del keep


def _have_hostsan_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists("/opt/rocm/bin/hipcc") and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


@pytest.mark.skipif(not _have_hostsan_toolchain(), reason="hipcc / clang sanitizer runtimes not available")
def test_level_one_check_on_the_fake_runtime():
    spec = importlib.util.spec_from_file_location("cip_build_hostsan", os.path.join(ROOT, "tests", "hostsan", "build_hostsan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe, env = mod.build("asan")
    out = os.path.dirname(exe)
    so = os.path.join(out, "libcipkkt_host_asan.so")
    drv = os.path.join(out, "drive_sparseq_args")
    subprocess.run([mod.CLANGXX, "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "sparseq", "drive_args.cpp"), so,
                    "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "drive_args: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
