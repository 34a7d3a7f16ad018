"""The reference-side binding (integration/ConicIPHIP: a Julia package) cannot be executed in this image --
no Julia -- so it is checked mechanically against the C ABI it binds: every `ccall` names a function declared in
include/cipkkt.h with the same number of arguments, the Julia `CipProblem` / `CipOptions` / `CipResult` structs mirror `cip_problem` / `cip_options` / `cip_result` field for field (order, names, C types),
the package files are complete, and integration/moi_kktsolver.patch applies to the reference's src/MOI_wrapper.jl (whose lines
are pinned by their digests in tests/golden/reference_api.json)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "integration", "ConicIPHIP")
JL = os.path.join(PKG, "src", "ConicIPHIP.jl")
HEADER = os.path.join(ROOT, "include", "cipkkt.h")


def _header():
    src = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _c_prototypes():
    """name -> number of parameters, for every function declared in the header."""
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char \*)\s*(cip_[A-Za-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return out


def _split_top_level(s):
    parts, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur)
    return [p.strip() for p in parts]


def _julia_ccalls():
    """(symbol, number of argument TYPES in the ccall's type tuple) for every ccall of the package."""
    src = open(JL).read()
    out = []
    for m in re.finditer(r"ccall\(_sym\(:(cip_[A-Za-z0-9_]+)\),\s*(\w+),\s*\(", src):
        i = m.end()
        depth, j = 1, i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        types = src[i:j - 1]
        out.append((m.group(1), len([t for t in _split_top_level(types) if t])))
    return out


def test_package_files_are_complete():
    toml = open(os.path.join(PKG, "Project.toml")).read()
    for key in ('name = "ConicIPHIP"', "uuid =", "ConicIP =", "Libdl =", "SparseArrays =", "LinearAlgebra ="):
        assert key in toml, key
    src = open(JL).read()
    assert re.search(r"^module ConicIPHIP", src, flags=re.M) and src.rstrip().endswith("end # module")
    for name in ("kktsolver_hip", "kktsolver_hip_full3x3", "kktsolver_2x2_hip", "__init__", "Libdl.find_library", "Libdl.dlopen"):
        assert name in src, name
    assert os.path.exists(os.path.join(PKG, "test", "runtests.jl"))
    # balanced block structure (a cheap parse check: every `function` / `struct` / `if` / `for` / `begin` / `module` closes)
    code = re.sub(r'"""(.|\n)*?"""', "", src)
    code = re.sub(r"#.*", "", code)
    code = re.sub(r'"(\\.|[^"\\])*"', '""', code)
    # block openers at the start of a statement (comprehension `for`s and ternaries do not open blocks), `x = if ...`, and
    # the `GC.@preserve ... begin` form
    opens = len(re.findall(r"^\s*(?:mutable\s+)?(function|struct|if|for|begin|module|while|let)\b", code, flags=re.M))
    opens += len(re.findall(r"=\s*if\b", code)) + len(re.findall(r"\S[^\n]*\bbegin\s*$", code, flags=re.M))
    closes = len(re.findall(r"^\s*end\b", code, flags=re.M))
    assert opens == closes, (opens, closes)


def _c_param_classes():
    """name -> ['int' | 'double' | 'ptr', ...] for every function declared in the header"""
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char \*)\s*(cip_[A-Za-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S):
        args = m.group(2).strip()
        cls = []
        for a in ([] if args in ("", "void") else args.split(",")):
            a = a.strip()
            cls.append("ptr" if "*" in a else "double" if re.match(r"(const\s+)?double\b", a) else "int")
        out[m.group(1)] = cls
    return out


def test_every_ccall_argument_has_the_headers_type_class():
    """beyond the count: an `int` parameter is bound as Cint, a `double` as Cdouble, every pointer as Ptr{..} / Ref{..}"""
    src = open(JL).read()
    classes = _c_param_classes()
    n = 0
    for m in re.finditer(r"ccall\(_sym\(:(cip_[A-Za-z0-9_]+)\),\s*(\w+),\s*\(", src):
        i = m.end()
        depth, j = 1, i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        types = [t for t in _split_top_level(src[i:j - 1]) if t]
        got = ["int" if t == "Cint" else "double" if t in ("Cdouble", "Float64") else "ptr" if re.match(r"(Ptr|Ref)\{", t) else t
               for t in types]
        assert got == classes[m.group(1)], (m.group(1), got, classes[m.group(1)])
        n += 1
    assert n >= 10


def test_every_ccall_matches_the_header():
    protos = _c_prototypes()
    calls = _julia_ccalls()
    assert {c[0] for c in calls} >= {"cip_create", "cip_create_ex", "cip_set_scaling_packed", "cip_factor", "cip_solve3x3",
                                     "cip_solve2x2", "cip_destroy", "cip_last_error", "cip_conicip", "cip_conicip_mixed"}
    for name, nargs in calls:
        assert name in protos, "%s is not declared in include/cipkkt.h" % name
        assert protos[name] == nargs, "%s: %d argument types in the ccall, %d parameters in the header" % (name, nargs, protos[name])


def _c_struct_fields(name):
    """[(field, julia type class)] of `typedef struct <name> {...}`: 'Cint', 'Cdouble' or 'Ptr{Cint}' / 'Ptr{Float64}'."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const\s+)?(int|double)\b", decl)
        assert base, decl
        scalar = {"int": "Cint", "double": "Cdouble"}[base.group(2)]
        elem = {"int": "Cint", "double": "Float64"}[base.group(2)]
        rest = decl[base.end():]
        for piece in rest.split(","):
            piece = piece.strip()
            fname = re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", piece)[0]
            out.append((fname, "Ptr{%s}" % elem if "*" in piece else scalar))
    return out


def _julia_struct_fields(name):
    src = open(JL).read()
    jbody = re.search(r"^struct %s\b[^\n]*\n(.*?)\n^end" % name, src, flags=re.S | re.M).group(1)
    jbody = re.sub(r"#.*", "", jbody)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)::(Ptr\{\w+\}|Cint|Cdouble|Float64)", jbody)


@pytest.mark.parametrize("cname, jname", [("cip_problem", "CipProblem"), ("cip_options", "CipOptions"), ("cip_result", "CipResult")])
def test_julia_structs_mirror_the_c_structs(cname, jname):
    """field ORDER, NAMES and C TYPES (int <-> Cint, double <-> Cdouble, T* <-> Ptr{T}): Julia lays an immutable struct of
    such fields out as the C compiler does, so these three facts are the whole ABI of the struct"""
    c = _c_struct_fields(cname)
    j = [(n, "Cdouble" if t == "Float64" else t) for n, t in _julia_struct_fields(jname)]
    assert [f[0] for f in j] == [f[0] for f in c], (j, c)
    for (jn, jt), (cn, ct) in zip(j, c):
        assert jt == ct, "%s.%s: Julia %s, C %s" % (jname, jn, jt, ct)


def test_struct_sizes_match_the_python_binding():
    """the ctypes mirrors the GPU tests drive (cipkkt/_lib.py) have the same fields in the same order as the header: the Julia
    mirrors are then checked against the same source of truth"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "conicip.jl_amd"))
    from cipkkt import _lib as L
    for cname, ct in (("cip_problem", L.CipProblem), ("cip_options", L.CipOptions), ("cip_result", L.CipResult)):
        assert [f[0] for f in ct._fields_] == [f[0] for f in _c_struct_fields(cname)], cname


def test_native_loop_and_batch_are_bound():
    """SURVEY 8 f1 from the reference side: `conicIP_hip` binds cip_conicip, `conicIP_hip_batch` binds cip_conicip_mixed; both
    return ConicIP.Solution with the reference's keyword names and defaults (src/ConicIP.jl:498-509)"""
    src = open(JL).read()
    calls = {c[0] for c in _julia_ccalls()}
    assert {"cip_conicip", "cip_conicip_mixed"} <= calls
    sig = re.search(r"function conicIP_hip\((.*?)\)\n", src, flags=re.S).group(1)
    for kw in ("optTol = 1e-6", "DTB = 0.01", "verbose = true", "maxRefinementSteps = 3", "maxIters = 100", "cache_nestodd = false",
               "infeasTol = optTol", "refinementThreshold = optTol / 1e7", "G = spzeros(0, length(c))", "d = zeros(0)"):
        assert kw in sig, kw
    assert "ConicIP.Solution(y, w, v, _STATUS[r.status + 1]" in src
    # status codes of the header in the order of the Julia tuple
    h = _header()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define CIP_STATUS_(\w+)\s+(\d+)", h)}
    tup = re.search(r"const _STATUS = \((.*?)\)", src).group(1)
    names = [t.strip().lstrip(":").upper() for t in tup.split(",")]
    assert [codes[nm] for nm in names] == list(range(len(names))), (names, codes)
    # Diagonal / Id(n) goes over as CSR, not as a dense identity (src/ConicIP.jl:18)
    assert "_as_csr_source(A::Diagonal) = sparse(A)" in src
    for name in ("conicIP_hip", "conicIP_hip_batch", "preprocess_conicIP_hip", "CipOptions", "CipResult"):
        assert re.search(r"^export .*\b%s\b" % name, src, flags=re.M), name
    tests = open(os.path.join(PKG, "test", "runtests.jl")).read()
    for name in ("conicIP_hip(", "conicIP_hip_batch(", "preprocess_conicIP_hip(", "Id(n)"):
        assert name in tests, name


REF_API = os.path.join(ROOT, "tests", "golden", "reference_api.json")      # pinned by tests/golden/make_reference_api.py


def _reference_api():
    import json
    with open(REF_API) as f:
        return json.load(f)


def _patch_hunks(text):
    """The hunks of a unified diff of one file: [(old_start, old_lines, new_lines)], lines without their one-character tag."""
    hunks, cur = [], None
    for line in text.split("\n"):
        m = re.match(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
        if m:
            cur = (int(m.group(1)), [], [], int(m.group(2) or 1), int(m.group(4) or 1))
            hunks.append(cur)
        elif cur is not None and (line[:1] in (" ", "-", "+") or line == ""):
            tag, body = (line[:1] or " "), line[1:]
            if tag in (" ", "-"):
                cur[1].append(body)
            if tag in (" ", "+"):
                cur[2].append(body)
    for start, old, new, n_old, n_new in hunks:       # (a trailing empty string of the file is not a context line)
        while len(old) > n_old and old[-1] == "" and new and new[-1] == "":
            old.pop(); new.pop()
        assert (len(old), len(new)) == (n_old, n_new), ("hunk at line %d: %d / %d lines, header says %d / %d"
                                                        % (start, len(old), len(new), n_old, n_new))
    return [(start, old, new) for start, old, new, _, _ in hunks]


def test_moi_patch_applies_to_the_reference():
    """integration/moi_kktsolver.patch applies to the reference's src/MOI_wrapper.jl exactly (no offset, no fuzz): every context
    and removed line of every hunk is, by its sha256, the reference's line at that place (tests/golden/reference_api.json), the
    hunks are in order and do not overlap -- and the patched file has the `kktsolver` / `solve` options the shim documents."""
    import hashlib
    ref = _reference_api()["moi_wrapper_line_sha256"]
    digest = lambda line: hashlib.sha256(line.encode("utf-8")).hexdigest()
    patch = open(os.path.join(ROOT, "integration", "moi_kktsolver.patch"), encoding="utf-8").read()
    assert patch.startswith("--- a/src/MOI_wrapper.jl\n+++ b/src/MOI_wrapper.jl\n")
    hunks = _patch_hunks(patch)
    assert hunks
    out, pos = [], 0                                  # the patched file: the reference's lines stand in by their digests
    for start, old, new in hunks:
        at = start - 1
        assert at >= pos, "hunks overlap or are out of order at line %d" % start
        assert at + len(old) <= len(ref), "hunk at line %d runs past the end of the reference's file" % start
        for k, line in enumerate(old):
            assert digest(line) == ref[at + k], "line %d of src/MOI_wrapper.jl is not %r" % (at + k + 1, line)
        out += ref[pos:at] + new
        pos = at + len(old)
    out = "\n".join(out + ref[pos:])
    assert "kktsolver = dest.kktsolver" in out and 'attr.name == "kktsolver"' in out and "kktsolver::Any" in out
    assert "dest.sol = dest.solve(Q, c_int, A, b, cone_dims, G, d;" in out and "solve::Any" in out


def test_every_conicip_identifier_the_julia_shim_uses_exists_in_the_reference():
    """integration/ConicIPHIP cannot be executed here (no julia in the image): a second static check beside the ccall / struct
    ones -- every name the shim takes from ConicIP is defined in the reference where the shim's comments say: `Block` with a
    `Blocks` vector (src/blockmatrices.jl:35-41), `VecCongurance` with its `R` (src/ConicIP.jl:35), `ord` (:85), `Solution` with
    the eleven fields the shim fills positionally (:384-398), `imcols` / `preprocess_conicIP` (src/preprocessor.jl), `pivot` and
    `kktsolver_2x2` (src/kktsolvers.jl), the keyword names and defaults of `conicIP` (src/ConicIP.jl:498-509).  The reference's
    side is pinned as data in tests/golden/reference_api.json (tests/golden/make_reference_api.py)."""
    api = _reference_api()
    shim = open(os.path.join(ROOT, "integration", "ConicIPHIP", "src", "ConicIPHIP.jl"), encoding="utf-8").read()
    for what in ("Block: mutable struct with Blocks::Vector{BlockElem}", "VecCongurance: mutable struct with R::Matrix", "ord",
                 "imcols", "preprocess_conicIP", "pivot", "kktsolver_2x2"):
        assert api["definitions"][what] is True, what
    assert api["solution_fields"] == ["y", "w", "v", "status", "Iter", "Mu", "prFeas", "duFeas", "muFeas", "pobj", "dobj"]
    # the shim builds Solution positionally with exactly these eleven values, in this order
    call = re.search(r"ConicIP\.Solution\(y, w, v, _STATUS\[r\.status \+ 1\], Int\(r\.iter\), r\.mu, r\.prFeas, r\.duFeas, r\.muFeas, r\.pobj, r\.dobj\)", shim)
    assert call, "the shim's Solution constructor call changed: re-check it against src/ConicIP.jl:384-398"
    # every `ConicIP.<name>` of the shim is a name the reference defines somewhere in src/
    for name in sorted(set(re.findall(r"ConicIP\.(\w+)", shim))):
        if name in ("jl",):                                   # "ConicIP.jl:123" in comments
            continue
        assert name in api["names_defined"], "ConicIP.%s is new in the shim: re-pin with tests/golden/make_reference_api.py" % name
        assert api["names_defined"][name] is True, "ConicIP.%s is not a name of the reference" % name
    # keyword names and defaults of conicIP the shim repeats (src/ConicIP.jl:498-509)
    for kw, default in (("optTol", "1e-6"), ("DTB", "0.01"), ("maxRefinementSteps", "3"), ("maxIters", "100")):
        assert api["conicIP_keyword_defaults"][kw] == default, kw
        assert re.search(r"%s\s*=\s*%s" % (kw, re.escape(default)), shim), kw
