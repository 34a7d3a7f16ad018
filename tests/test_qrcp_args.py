"""Argument rules of the rank-revealing QR entry points (include/cipkkt.h), CPU only: the bindings and exports exist, bad arguments
are refused with CIP_E_INVALID before anything touches a GPU, and the host code -- compiled host-only and linked against the fake
HIP runtime of tests/hostsan -- runs its chunked step loop to the end with a workspace of exactly the advertised size
(tests/qrcp/drive_args.cpp, a stand-alone program under AddressSanitizer / UBSan)."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cip_qrcp_workspace_bytes", "cip_imcols_workspace_bytes", "cip_qrcp_dev", "cip_imcols_dev")


def test_entry_points_are_exported_and_bound():
    import cipkkt
    from cipkkt import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for f in NEW:
        assert hasattr(lib, f), f
        assert f in _lib.SIGNATURES, f
    assert callable(cipkkt.qrcp_hip) and callable(cipkkt.imcols_hip)


def test_refusals_need_no_gpu():
    from cipkkt import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.cip_qrcp_workspace_bytes(-1, 4, ctypes.byref(nb)) == -1
    assert lib.cip_imcols_workspace_bytes(4, -1, ctypes.byref(nb)) == -1
    assert lib.cip_qrcp_workspace_bytes(12, 7, None) == -1
    assert lib.cip_qrcp_workspace_bytes(12, 7, ctypes.byref(nb)) == 0 and nb.value > 0
    small = nb.value
    assert lib.cip_imcols_workspace_bytes(12, 7, ctypes.byref(nb)) == 0 and nb.value >= small + 8 * 12 * 7
    assert lib.cip_imcols_workspace_bytes(24576, 8192, ctypes.byref(nb)) == 0 and nb.value > 8 * 24576 * 8192   # no 32-bit overflow
    M = np.ones((7, 12))
    ws = np.zeros(nb.value // 8 if nb.value < 1 << 20 else 1 << 16)
    k, n, ok = ctypes.c_int(-5), ctypes.c_int(-5), ctypes.c_int(-5)
    piv = np.zeros(7, dtype=np.int32)
    pp = piv.ctypes.data_as(_lib.c_int_p)
    m, w = M.ctypes.data, ws.ctypes.data
    bad_qr = [(None, 12, 7, 12, 0.0, w, k), (m, 12, 7, 12, 0.0, None, k), (m, 12, 7, 12, 0.0, w, None), (m, -1, 7, 12, 0.0, w, k),
              (m, 12, -7, 12, 0.0, w, k), (m, 12, 7, 11, 0.0, w, k), (m, 12, 7, 12, -1e-9, w, k), (m, 12, 7, 12, float("nan"), w, k),
              (m, 12, 7, 12, float("inf"), w, k), (m, 0, 7, 0, 0.0, w, k)]
    for (mm, ln, cnt, ld, stop, wsp, kk) in bad_qr:
        assert lib.cip_qrcp_dev(None, mm, ln, cnt, ld, stop, wsp, None, pp, None, ctypes.byref(kk) if kk is not None else None) == -1
    assert k.value == -5
    b = np.ones(7).ctypes.data
    bad_im = [(None, 12, 7, 12, b, 1e-8, w, pp), (m, 12, 7, 12, None, 1e-8, w, pp), (m, 12, 7, 12, b, 1e-8, None, pp),
              (m, 12, 7, 12, b, 1e-8, w, None), (m, 12, 7, 11, b, 1e-8, w, pp), (m, -12, 7, 12, b, 1e-8, w, pp),
              (m, 12, 7, 12, b, -1.0, w, pp), (m, 12, 7, 12, b, float("nan"), w, pp)]
    for (mm, ln, cnt, ld, bb, eps, wsp, rr) in bad_im:
        assert lib.cip_imcols_dev(None, mm, ln, cnt, ld, bb, eps, wsp, rr, ctypes.byref(n), ctypes.byref(ok), None) == -1
    assert lib.cip_imcols_dev(None, m, 12, 7, 12, b, 1e-8, w, pp, None, ctypes.byref(ok), None) == -1
    assert n.value == -5 and ok.value == -5
    assert b"cip_imcols_dev" in lib.cip_last_error()
    # len * cnt == 0: a no-op that needs no device
    assert lib.cip_qrcp_dev(None, None, 0, 7, 1, 0.0, None, None, pp, None, ctypes.byref(k)) == 0 and k.value == 0
    assert list(piv) == list(range(7))
    assert lib.cip_imcols_dev(None, None, 12, 0, 12, None, 1e-8, None, None, ctypes.byref(n), ctypes.byref(ok), None) == 0
    assert (n.value, ok.value) == (0, 1)


def test_rank_solver_must_be_host_or_device():
    import scipy.sparse as sp
    import cipkkt
    n = 4
    with pytest.raises(ValueError, match="rank_solver"):
        cipkkt.preprocess_conicIP(np.eye(n), np.ones(n), sp.identity(n, format="csr"), np.zeros(n), [("R", n)], rank_solver="bogus")


def test_no_host_fallback_without_a_gpu():
    import torch
    import cipkkt
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        cipkkt.imcols_hip(np.eye(3), np.ones(3))
    with pytest.raises(RuntimeError):
        cipkkt.qrcp_hip(np.eye(3))
    # ... and the device path of the pre-solve raises instead of running the host QR (rank-deficient G: the certificate fails)
    G = np.array([[1.0, 0, 0], [1.0, 0, 0]])
    with pytest.raises(RuntimeError):
        cipkkt.preprocess_conicIP(np.eye(3), np.ones(3), np.eye(3), np.zeros(3), [("R", 3)], G, np.zeros(2), rank_solver="device")


def _have_hostsan_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists("/opt/rocm/bin/hipcc") and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


@pytest.mark.skipif(not _have_hostsan_toolchain(), reason="hipcc / clang sanitizer runtimes not available")
def test_argument_rules_and_step_loop_on_the_fake_runtime():
    spec = importlib.util.spec_from_file_location("cip_build_hostsan", os.path.join(ROOT, "tests", "hostsan", "build_hostsan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe, env = mod.build("asan")
    out = os.path.dirname(exe)
    so = os.path.join(out, "libcipkkt_host_asan.so")
    drv = os.path.join(out, "drive_qrcp_args")
    subprocess.run([mod.CLANGXX, "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "qrcp", "drive_args.cpp"), so,
                    "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "drive_args: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
