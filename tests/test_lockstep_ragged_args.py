"""The switch of the ragged lock-step groups (include/cipkkt.h: cip_set_lockstep_ragged) and its Python face through ctypes on the
built library, and the groups' host side -- shape rule, slab capacities, per-handle uploads, both entry points, host and "device"
CSR arrays -- compiled host-only and linked against the fake HIP runtime of tests/hostsan (tests/ragged/drive_ragged.cpp, a
stand-alone program under AddressSanitizer / UBSan).  No device call."""
import importlib.util
import inspect
import os
import subprocess

import pytest

from cipkkt import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setter_returns_the_previous_value_and_other_values_only_query():
    lib = L.load()
    first = lib.cip_set_lockstep_ragged(-1)
    try:
        assert first == 0                                # the default: the nnz of a CSR matrix is part of the shape
        assert lib.cip_set_lockstep_ragged(1) == 0
        assert lib.cip_set_lockstep_ragged(1) == 1
        for query in (-1, 2, 7, -100):
            assert lib.cip_set_lockstep_ragged(query) == 1
        assert lib.cip_set_lockstep_ragged(0) == 1
        assert lib.cip_set_lockstep_ragged(-1) == 0
    finally:
        lib.cip_set_lockstep_ragged(first)


def test_the_switch_is_an_int_in_an_int_out():
    import ctypes as C
    assert L.SIGNATURES["cip_set_lockstep_ragged"] == (C.c_int, [C.c_int])
    assert L.SIGNATURES["cip_set_lockstep_ragged"] == L.SIGNATURES["cip_set_lockstep_regularize"]


def test_python_switch_and_keywords():
    from cipkkt import batch
    prev = batch.lockstep_ragged()
    try:
        assert batch.lockstep_ragged(True) == prev
        assert batch.lockstep_ragged() == 1
        assert batch.lockstep_ragged(False) == 1
        assert batch.lockstep_ragged(None) == 0
    finally:
        batch.lockstep_ragged(prev)
    for fn in (batch._solve_problems_native, batch.solve_batch):
        par = inspect.signature(fn).parameters
        assert par["ragged"].default is False
        assert list(par)[-1] == "ragged"                 # appended last: positional callers keep their meaning


def test_julia_wrapper_takes_the_keyword():
    src = open(os.path.join(ROOT, "integration", "ConicIPHIP", "src", "ConicIPHIP.jl")).read()
    assert "ragged = false" in src and src.count(":cip_set_lockstep_ragged") == 2      # set, and restored


def _have_hostsan_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists("/opt/rocm/bin/hipcc") and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


@pytest.mark.skipif(not _have_hostsan_toolchain(), reason="hipcc / clang sanitizer runtimes not available")
def test_ragged_groups_on_the_fake_runtime():
    spec = importlib.util.spec_from_file_location("cip_build_hostsan", os.path.join(ROOT, "tests", "hostsan", "build_hostsan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe, env = mod.build("asan")
    out = os.path.dirname(exe)
    so = os.path.join(out, "libcipkkt_host_asan.so")
    drv = os.path.join(out, "drive_ragged")
    subprocess.run([mod.CLANGXX, "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "ragged", "drive_ragged.cpp"), so,
                    "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "drive_ragged: ok" in r.stdout
    assert r.stdout.count("CSR arrays: ok") == 6         # (a), (b), (c) with host and with "device" arrays
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
