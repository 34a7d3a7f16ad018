"""The device full-row-rank certificate (cip_rowrank_cert, include/cipkkt.h), CPU only: the function is declared, exported and
bound, `cip_cert_block` and its ctypes mirror agree, the Python layers carry `full_row_rank_hip` and the `certificate` keyword with
their defaults, nothing falls back to the host without a GPU, and the argument rules -- compiled host-only and linked against the
fake HIP runtime of tests/hostsan -- are refused with CIP_E_INVALID before any device allocation, while valid inputs leave none
behind (tests/rowrank/drive_args.cpp, a stand-alone program under AddressSanitizer / UBSan)."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cipkkt.h")).read(), flags=re.S)


def test_the_call_is_declared_exported_and_bound():
    from cipkkt import _lib
    m = re.search(r"\bint\s+cip_rowrank_cert\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8
    assert not any("cip_handle" in p or "hip_stream" in p for p in params)          # it owns its streams
    res, args = _lib.SIGNATURES["cip_rowrank_cert"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[2] == ctypes.POINTER(_lib.CipCertBlock) and args[3] is ctypes.c_double
    lib = _lib.load()
    assert hasattr(lib, "cip_rowrank_cert")
    flags = {int(v) for v in re.findall(r"#define\s+CIP_FLAG_\w+\s+(\d+)", _header())}
    assert flags == {1, 2, 4}                                                       # no new flag


def test_cert_block_and_its_ctypes_mirror_agree_field_for_field():
    from cipkkt import _lib
    body = re.search(r"typedef struct cip_cert_block \{(.*?)\} cip_cert_block;", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            name = re.findall(r"([A-Za-z_]\w*)\s*$", decl)[0]
            fields.append((name, ctypes.c_void_p if "*" in decl else {"int": ctypes.c_int, "double": ctypes.c_double}[decl.split()[0]]))
    assert [(n, t) for n, t in _lib.CipCertBlock._fields_] == fields
    assert [f[0] for f in fields] == ["cols", "dense", "ld", "rowptr", "colind", "val"]


def test_the_julia_shim_mirrors_the_block_and_binds_the_call():
    src = open(os.path.join(ROOT, "integration", "ConicIPHIP", "src", "ConicIPHIP.jl"), encoding="utf-8").read()
    body = re.sub(r"#.*", "", re.search(r"^struct CipCertBlock\b[^\n]*\n(.*?)\n^end", src, flags=re.S | re.M).group(1))
    got = re.findall(r"([A-Za-z_]\w*)::(Ptr\{\w+\}|Cint|Cdouble)", body)
    assert got == [("cols", "Cint"), ("dense", "Ptr{Float64}"), ("ld", "Cint"), ("rowptr", "Ptr{Cint}"), ("colind", "Ptr{Cint}"),
                   ("val", "Ptr{Float64}")]
    assert "ccall(_sym(:cip_rowrank_cert)" in src and re.search(r"^export .*\bfull_row_rank_hip\b", src, flags=re.M)
    assert "certificate = :host" in src and "certificate == :device" in src
    tests = open(os.path.join(ROOT, "integration", "ConicIPHIP", "test", "runtests.jl"), encoding="utf-8").read()
    assert "full_row_rank_hip(" in tests and "certificate = :device" in tests


def test_python_layers_carry_the_function_and_the_keyword():
    import cipkkt
    from cipkkt import preprocess, qrcp
    assert cipkkt.full_row_rank_hip is qrcp.full_row_rank_hip and "full_row_rank_hip" in cipkkt.__all__
    par = inspect.signature(qrcp.full_row_rank_hip).parameters
    assert list(par)[:2] == ["blocks", "eps"] and par["eps"].default == 1e-8
    par = inspect.signature(preprocess.preprocess_conicIP).parameters
    assert par["certificate"].default == "host" and par["rank_solver"].default == "host"


def _box(n=6):
    return np.eye(n), -np.ones(n), sp.identity(n, format="csr"), np.zeros(n), [("R", n)]


def test_an_unknown_certificate_is_refused():
    from cipkkt import preprocess_conicIP
    with pytest.raises(ValueError, match="certificate"):
        preprocess_conicIP(*_box(), certificate="bogus")
    with pytest.raises(ValueError, match="certificate"):
        preprocess_conicIP(*_box(), certificate=None)


def test_no_fall_back_to_the_host_without_a_gpu(monkeypatch):
    """certificate="device" without a HIP device raises, with and without equality rows; so does the function itself"""
    import torch
    import cipkkt
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device"):
        cipkkt.preprocess_conicIP(*_box(), certificate="device")
    with pytest.raises(RuntimeError, match="no HIP device"):
        cipkkt.preprocess_conicIP(*_box(), G=np.ones((1, 6)), d=np.zeros(1), certificate="device", rank_solver="device")
    with pytest.raises(RuntimeError, match="no HIP device"):
        cipkkt.full_row_rank_hip([np.eye(3)])


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
    drv = os.path.join(out, "drive_rowrank_args")
    subprocess.run([mod.CLANGXX, "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "rowrank", "drive_args.cpp"), so,
                    "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "drive_args: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
