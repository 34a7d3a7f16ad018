#!/usr/bin/env python3
"""Pins the facts of the reference's source that tests/test_integration_files.py checks the Julia shim and the MOI patch
against, as DATA in tests/golden/reference_api.json: sha256 digests of the files read and of every line of src/MOI_wrapper.jl
(the patch's context and removed lines are matched against them), the fields of `Solution` in order, the keyword defaults of
`conicIP`, whether the definitions the shim relies on exist, and which of the `ConicIP.<name>`s the shim takes the reference
defines.  No source text is stored.  usage: python tests/golden/make_reference_api.py <root of the reference checkout>"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_api.json")
FILES = ("ConicIP.jl", "blockmatrices.jl", "preprocessor.jl", "kktsolvers.jl", "MOI_wrapper.jl")
KEYWORDS = ("optTol", "DTB", "maxRefinementSteps", "maxIters")


def sha(text):
    return hashlib.sha256(text.encode("utf-8")).hexdigest()


def shim_names(shim):
    return sorted(set(re.findall(r"ConicIP\.(\w+)", shim)) - {"jl"})          # ("ConicIP.jl:123" in comments)


def main(ref):
    src = {f: open(os.path.join(ref, "src", f), encoding="utf-8").read() for f in FILES}
    core, blocks, pre, kkt = src["ConicIP.jl"], src["blockmatrices.jl"], src["preprocessor.jl"], src["kktsolvers.jl"]
    m = re.search(r"mutable struct Solution\n(.*?)\nend", core, re.S)
    sig = core[core.index("function conicIP("):core.index("function conicIP(") + 1500]
    defaults = {}
    for kw in KEYWORDS:
        d = re.search(r"\b%s\s*=\s*([^,;\s)]+)" % kw, sig)
        defaults[kw] = d.group(1) if d else None
    everything = "".join(src[f] for f in FILES)
    shim = open(os.path.join(ROOT, "integration", "ConicIPHIP", "src", "ConicIPHIP.jl"), encoding="utf-8").read()
    out = {
        "files_sha256": {"src/" + f: sha(src[f]) for f in FILES},
        "moi_wrapper_line_sha256": [sha(line) for line in src["MOI_wrapper.jl"].split("\n")],
        "definitions": {
            "Block: mutable struct with Blocks::Vector{BlockElem}": bool(re.search(r"mutable struct Block\b", blocks)
                                                                       and re.search(r"Blocks::Vector\{BlockElem\}", blocks)),
            "VecCongurance: mutable struct with R::Matrix": bool(re.search(r"mutable struct VecCongurance; R :: Matrix; end", core)),
            "ord": bool(re.search(r"^ord\(x\) = ", core, re.M)),
            "imcols": bool(re.search(r"^function imcols\(A, b", pre, re.M)),
            "preprocess_conicIP": bool(re.search(r"^function preprocess_conicIP\(Q, c", pre, re.M)),
            "pivot": bool(re.search(r"^function pivot", kkt, re.M) or re.search(r"^pivot\(", kkt, re.M) or "pivotgen" in kkt),
            "kktsolver_2x2": bool(re.search(r"function kktsolver_2x2", kkt)),
        },
        "solution_fields": re.findall(r"^\s*(\w+)\s*::", m.group(1), re.M) if m else None,
        "conicIP_keyword_defaults": defaults,
        "names_defined": {name: bool(re.search(r"\b%s\b" % re.escape(name), everything)) for name in shim_names(shim)},
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
