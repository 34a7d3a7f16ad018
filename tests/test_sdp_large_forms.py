"""The form rules of the large S cones (conicip.jl_amd/csrc/cip_sdp_large_forms.h) on the CPU.

tests/sdp_large_forms/forms_table.cpp, a stand-alone program under AddressSanitizer / UBSan that includes the header alone, prints
the forms of (largest order, order, Lanczos mode) rows; here that is compared with the independent restatement of the rules in
tests/_sdp_large_forms.py at every order from 133 to 2048 and every mode, and with edges worked out by hand.  The same source
built as forms_trace drives the host-only library through the fake HIP runtime of tests/hostsan with its launch trace on: the
launches of an NT scaling and a max-step at orders 133 and 257 must be the ones the header names.  (Orders above 512 are left to
tests/test_gpu_sdp_large_edges.py: under the fake runtime their workspaces are gigabytes of host memory.)  No device call."""
import functools
import importlib.util
import os
import re
import subprocess

import pytest

from _sdp_large_forms import LARGE_S_MIN, _reach

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conicip.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sdp_large_forms", "forms_table.cpp")
CLANGXX = os.environ.get("CIP_CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
SAN = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict({k: v for k, v in os.environ.items() if k != "LD_PRELOAD"},
           ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _have_toolchain():
    rt = "/opt/rocm/lib/llvm/lib/clang"
    return os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(CLANGXX) and os.path.isdir(rt) and any(
        os.path.exists(os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.a")) for v in os.listdir(rt))


pytestmark = pytest.mark.skipif(not _have_toolchain(), reason="hipcc / clang sanitizer runtimes not available")


def _s(r):
    return ("S", r * (r + 1) // 2)


@functools.lru_cache(maxsize=None)
def _table_exe():
    out = os.path.join(ROOT, "tests", "hostsan", "_build", "forms")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "forms_table")
    subprocess.run([CLANGXX, "-I", CSRC] + SAN + [SRC, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def forms(rows):
    """rows: (r_max, r, mode) -> dicts in the vocabulary of _reach, plus cert / lds / raw slab, nwg, launches"""
    text = "".join("%d %d %d\n" % row for row in rows)
    r = subprocess.run([_table_exe()], input=text, env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = []
    for line in r.stdout.splitlines():
        m = re.fullmatch(r"rp=(\d+) jacobi=(\d+),(\d+),(\d+) small=([01]) pairable=([01]) eig=(\w+) cert=([01]) slab=(\d+) nwg=(\d+) "
                         r"lds=(\d+) launches=(\d+)", line)
        assert m, line
        g = m.groups()
        kind, slab, nwg, launches = g[6], int(g[8]), int(g[9]), int(g[11])
        count = {"lanczos": 1, "registers": 1, "cooperative": nwg, "stepped": launches}[kind]
        out.append(dict(rp=int(g[0]), jacobi=(int(g[1]), int(g[2]), int(g[3])), gemm="small" if g[4] == "1" else "batched-64",
                        pairable=g[5] == "1", maxstep=(kind, slab, count), cert=g[7] == "1", lds=int(g[10]), nwg=nwg, launches=launches))
    assert len(out) == len(rows)
    return out


def form(r_max, r=None, mode=2):
    return forms([(r_max, r_max if r is None else r, mode)])[0]


def test_the_header_is_the_restatement_at_every_order_and_mode():
    rows = [(r, r, mode) for r in range(LARGE_S_MIN, 2048 + 1) for mode in range(4)]
    assert len(rows) == 1916 * 4
    kinds = set()
    for (r, _, mode), f in zip(rows, forms(rows)):
        want = _reach([_s(r)], mode)
        assert {k: f[k] for k in ("rp", "jacobi", "gemm", "pairable")} == {k: want[k] for k in ("rp", "jacobi", "gemm", "pairable")}, (r, mode)
        assert [f["maxstep"]] == want["maxstep"], (r, mode)
        # the certificate follows the Lanczos form in modes 2 and 3 and nothing else; only the cooperative form has a slab and LDS
        assert f["cert"] == (f["maxstep"][0] == "lanczos" and mode >= 2), (r, mode)
        if f["maxstep"][0] == "cooperative":
            slab = f["maxstep"][1]
            assert f["lds"] == (slab * (r | 1) + 3 * r + 64) * 8 <= 160 * 1024 and (f["nwg"] - 1) * slab < r <= f["nwg"] * slab, (r, mode)
            assert f["nwg"] <= 64                                  # all resident: the grid barrier's premise
        else:
            assert (f["lds"], f["nwg"], f["maxstep"][1]) == (0, 0, 0), (r, mode)
        assert f["launches"] == (2 * (r - 1) if f["maxstep"][0] == "stepped" else 0), (r, mode)
        kinds.add(f["maxstep"][0])
    assert kinds == {"lanczos", "registers", "cooperative", "stepped"}


def test_edges_by_hand():
    J = {256: (256, 8, 8), 512: (1024, 8, 16), 1024: (512, 16, 8), 2048: (256, 32, 4)}
    # 256 / 257: the last order of the small product, the pair and the one-workgroup eigenvalue forms
    f = form(256)
    assert (f["rp"], f["jacobi"], f["gemm"], f["pairable"], f["maxstep"], f["cert"]) == (256, J[256], "small", True, ("lanczos", 0, 1), True)
    assert form(256, mode=1)["cert"] is False and form(256, mode=3)["cert"] is True and form(256, mode=1)["pairable"]
    f = form(256, mode=0)
    assert (f["pairable"], f["maxstep"], f["cert"], f["gemm"]) == (False, ("registers", 0, 1), False, "small")
    for mode in range(4):
        f = form(257, mode=mode)
        assert (f["rp"], f["jacobi"], f["gemm"], f["pairable"], f["maxstep"], f["cert"]) == (512, J[512], "batched-64", False, ("cooperative", 32, 9), False)
        assert f["lds"] == (32 * 257 + 3 * 257 + 64) * 8 == 72472
    # 512 / 513: the padded order moves, the slab does not (r | 1 = 513 for both)
    f, g = form(512), form(513)
    assert (f["rp"], f["jacobi"], f["maxstep"], f["lds"]) == (512, J[512], ("cooperative", 32, 16), 144128)
    assert (g["rp"], g["jacobi"], g["maxstep"], g["lds"]) == (1024, J[1024], ("cooperative", 32, 17), 144152)
    # 583 / 584: 32 x 583 + 1749 + 64 = 20469 doubles = 163752 bytes fit 163840; 32 x 585 + 1752 + 64 = 20536 doubles = 164288 do not
    f, g = form(583), form(584)
    assert (f["maxstep"], f["lds"]) == (("cooperative", 32, 19), 163752)
    assert (g["maxstep"], g["lds"]) == (("cooperative", 16, 37), (16 * 585 + 1752 + 64) * 8) and g["lds"] == 89408
    # 1024 / 1025: the last cooperative order (64 workgroups) and the first stepped one
    f, g = form(1024), form(1025)
    assert (f["rp"], f["jacobi"], f["maxstep"], f["lds"]) == (1024, J[1024], ("cooperative", 16, 64), (16 * 1025 + 3072 + 64) * 8)
    assert (g["rp"], g["jacobi"], g["maxstep"], g["lds"], g["gemm"]) == (2048, J[2048], ("stepped", 0, 2048), 0, "batched-64")
    f = form(2048)
    assert (f["rp"], f["jacobi"], f["maxstep"], f["pairable"]) == (2048, J[2048], ("stepped", 0, 4094), False)
    # two cones [140, 300]: the padded order, and with it the Jacobi, the GEMM and the pair, come from the larger cone; the
    # eigenvalue form from each cone's own order
    a, b = forms([(300, 140, 2), (300, 300, 2)])
    for f in (a, b):
        assert (f["rp"], f["jacobi"], f["gemm"], f["pairable"]) == (512, J[512], "batched-64", False)
    assert (a["maxstep"], a["cert"]) == (("lanczos", 0, 1), True) and b["maxstep"] == ("cooperative", 32, 10)
    want = _reach([_s(140), ("R", 5), _s(300)])
    assert want["maxstep"] == [a["maxstep"], b["maxstep"]] and want["padding"] == [372, 212]
    assert forms([(300, 140, 0)])[0]["maxstep"] == ("registers", 0, 1)


# ---------------------------------------------------------------- the launches of the host-only library are the header's
@functools.lru_cache(maxsize=None)
def _trace():
    """{section title: [lines]} of the trace that forms_trace leaves"""
    spec = importlib.util.spec_from_file_location("cip_build_hostsan", os.path.join(ROOT, "tests", "hostsan", "build_hostsan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe, env = mod.build("asan")
    out = os.path.dirname(exe)
    drv, path = os.path.join(out, "forms_trace"), os.path.join(out, "forms_trace.txt")
    subprocess.run([mod.CLANGXX, "-DFORMS_TRACE", "-I", os.path.join(ROOT, "include")] + SAN +
                   [SRC, os.path.join(out, "libcipkkt_host_asan.so"), "-Wl,-rpath," + out, "-o", drv], check=True, capture_output=True, text=True)
    r = subprocess.run([drv, path], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "forms_trace: ok" in r.stdout, (r.stdout[-1000:], r.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    sections, cur = {}, None
    for line in open(path).read().splitlines():
        assert "0x" not in line
        if line.startswith("# "):
            cur = None if line == "# end" else sections.setdefault(line[2:], [])
            assert cur is None or not cur, "section twice: " + line
        elif cur is not None:
            cur.append(line)
    return sections


def _launches(lines, kernel):
    """[(mangled name, grid x, block x, lds)] of the launches of `kernel` (its plain name, as the mangled one spells it)"""
    out = []
    for line in lines:
        m = re.fullmatch(r"launch (\S+) grid (\d+) (\d+) (\d+) block (\d+) 1 1 lds (\d+) stream \d+", line)
        if m and re.match(r"_Z%d%s(?![a-z0-9_])" % (len(kernel), kernel), m.group(1)):
            assert m.group(3) == "1" or kernel.startswith("k_gemm")
            out.append((m.group(1), int(m.group(2)), int(m.group(5)), int(m.group(6))))
    return out


def _pitch(rows):                    # the Jacobi's LDS column pitch (sdp_large_nt.hip: lg_pitch): == 4 (mod 32) doubles
    return rows + ((4 - rows % 32) + 32) % 32


@pytest.mark.parametrize("r, mode", [(133, 2), (133, 0), (257, 2)])
def test_a_scaling_and_a_max_step_launch_what_the_header_names(r, mode):
    T = _trace()
    f = form(r, mode=mode)
    nt, ms = T["nt r %d mode %d" % (r, mode)], T["maxstep r %d mode %d" % (r, mode)]
    threads, epl, block = f["jacobi"]
    # one launch per phase, rp / block phases per sweep, half as many workgroups; a cold start reads its first flag behind sweep 8,
    # and the fake runtime's flags say "nothing rotated"
    jac = _launches(nt, "k_lg_jacobi")
    assert len(jac) == 8 * (f["rp"] // block) and len(_launches(nt, "k_lg_pubflag")) == 1
    assert set(jac) == {(jac[0][0], f["rp"] // block // 2, threads, 2 * block * _pitch(f["rp"]) * 8)}
    assert jac[0][0].startswith("_Z11k_lg_jacobiILi%dELi%dEE" % (threads, epl))
    assert not _launches(ms, "k_lg_jacobi")
    # single products: the 16 x 16 split-k tile at padded order 256 only
    small = _launches(nt + ms, "k_gemm_nt_small")
    assert bool(small) == (f["gemm"] == "small") and all(x[1:] == (f["rp"] // 16, 256, 0) for x in small)
    # the max-step's eigenvalue
    kind = f["maxstep"][0]
    n = {k: _launches(ms, k) for k in ("k_lg_lanczos1", "k_lg_tridiag1", "k_lg_tridiag", "k_lg_sturm", "k_lg_cert_build", "k_tg_symv")}
    assert not n["k_tg_symv"]
    if kind == "lanczos":
        # ... with its certificate and the gated fallback behind it
        assert f["cert"] and [x[1:3] for x in n["k_lg_lanczos1"]] == [(1, 512)]
        assert (len(n["k_lg_cert_build"]), len(n["k_lg_tridiag1"]), len(n["k_lg_sturm"]), len(n["k_lg_tridiag"])) == (1, 1, 1, 0)
    elif kind == "registers":
        assert [x[1:3] for x in n["k_lg_tridiag1"]] == [(1, 512)] and len(n["k_lg_sturm"]) == 1
        assert not n["k_lg_lanczos1"] and not n["k_lg_cert_build"] and not n["k_lg_tridiag"]
    else:
        assert kind == "cooperative" and [x[1:] for x in n["k_lg_tridiag"]] == [(f["nwg"], 1024, f["lds"])] and len(n["k_lg_sturm"]) == 1
        assert not n["k_lg_lanczos1"] and not n["k_lg_cert_build"] and not n["k_lg_tridiag1"]
