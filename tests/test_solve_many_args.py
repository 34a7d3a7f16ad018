"""Argument rules of the many-right-hand-side entry points (include/cipkkt.h), CPU only: the bindings and exports exist, and the
host code -- compiled host-only and linked against the fake HIP runtime of tests/hostsan -- refuses every bad argument with
CIP_E_INVALID before anything is launched, treats nrhs == 0 as a no-op, and sizes the stand-alone scratch monotonically in nrhs
within one 64-column chunk (tests/solve_many/drive_args.cpp, under AddressSanitizer / UBSan)."""
import ctypes
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cip_ldlt_solve_many_scratch_bytes", "cip_ldlt_solve_many_dev", "cip_solve3x3_many", "cip_solve3x3_many_dev",
       "cip_solve2x2_many", "cip_solve2x2_many_dev")


def test_entry_points_are_exported_and_bound():
    from cipkkt import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for f in NEW:
        assert hasattr(lib, f), f
        assert f in _lib.SIGNATURES, f


def test_refusals_without_a_handle_need_no_gpu():
    from cipkkt import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.cip_ldlt_solve_many_scratch_bytes(1024, -1, ctypes.byref(nb)) == -1
    assert lib.cip_ldlt_solve_many_scratch_bytes(1000, 4, ctypes.byref(nb)) == -1
    sizes = []
    for k in (0, 1, 2, 63, 64, 65, 1000):
        assert lib.cip_ldlt_solve_many_scratch_bytes(1024, k, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[-1] == sizes[4] == 8 * 1024 * 64
    assert lib.cip_ldlt_solve_many_dev(None, None, 1024, 1024, None, None, None, 1024, 2) == -1
    assert lib.cip_solve3x3_many_dev(None, 2, None, None, None, None, None, None) == -1
    assert lib.cip_solve3x3_many(None, 2, None, None, None, None, None, None) == -1
    assert lib.cip_solve2x2_many_dev(None, 2, None, None, None, None) == -1
    assert lib.cip_solve2x2_many(None, 2, None, None, None, None) == -1


def _have_hostsan_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists("/opt/rocm/bin/hipcc") and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


@pytest.mark.skipif(not _have_hostsan_toolchain(), reason="hipcc / clang sanitizer runtimes not available")
def test_argument_rules_on_the_fake_runtime():
    spec = importlib.util.spec_from_file_location("cip_build_hostsan", os.path.join(ROOT, "tests", "hostsan", "build_hostsan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe, env = mod.build("asan")
    out = os.path.dirname(exe)
    so = os.path.join(out, "libcipkkt_host_asan.so")
    drv = os.path.join(out, "drive_many_args")
    subprocess.run([mod.CLANGXX, "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "solve_many", "drive_args.cpp"), so,
                    "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "drive_args: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
