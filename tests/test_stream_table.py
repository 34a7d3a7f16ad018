"""The stream table of tests/test_gpu_streams.py stays complete (no GPU needed): every function of include/cipkkt.h that takes a
cip_handle * together with data pointers, or a hip_stream argument, is either run there on a late stream or exempted below with a
reason.  An entry point added later without a stream test fails here."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cipkkt.h")
STREAMS = os.path.join(ROOT, "tests", "test_gpu_streams.py")

# functions that enqueue nothing on a caller's stream, or own their streams
EXEMPT = {
    "creation and destruction (cip_create_ex uploads on the null stream and waits; cip_destroy waits for the handle's stream)":
        ["cip_create", "cip_create_ex", "cip_destroy"],
    "knobs and counters: host state only, nothing is enqueued":
        ["cip_set_regularization", "cip_get_regularization", "cip_stats", "cip_set_timing", "cip_kkt_order",
         "cip_get_chain_fallbacks", "cip_sdp_lanczos_fallbacks"],
    "lock-step, mixed and batch calls: they create the streams they run on":
        ["cip_batch_create", "cip_batch_conicip", "cip_conicip_problems", "cip_conicip_lockstep", "cip_conicip_mixed",
         "cip_conicip_many"],
    "profiling: event pairs on launches the table's tests already cover":
        ["cip_profile_trailing", "cip_profile_get"],
}


def declarations():
    """name -> parameter text of every function the header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cip_[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def needs_a_stream_test(params):
    """a hip_stream argument, or a handle (or an array of handles) together with at least one more pointer argument"""
    args = [a.strip() for a in params.split(",")]
    if any(re.search(r"\bhip_stream\b", a) for a in args):
        return True
    handle = [a for a in args if re.search(r"\bcip_handle\b", a) or re.search(r"\bcip_batch\s*\*", a)]
    others = [a for a in args if a not in handle and "*" in a]
    return bool(handle) and bool(others)


def stream_table():
    tree = ast.parse(open(STREAMS).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "STREAM_TABLE" for t in node.targets):
            table = ast.literal_eval(node.value)
            tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
            return table, tests
    raise AssertionError("tests/test_gpu_streams.py has no STREAM_TABLE")


def test_the_parser_sees_the_header():
    decl = declarations()
    from cipkkt import _lib
    assert sorted(decl) == sorted(_lib.SIGNATURES)
    assert needs_a_stream_test(decl["cip_gemm_nt_dev"]) and needs_a_stream_test(decl["cip_axpby_dev"])
    assert needs_a_stream_test(decl["cip_set_stream"]) and needs_a_stream_test(decl["cip_conicip_many"])
    assert not needs_a_stream_test(decl["cip_factor"])              # a handle alone: listed in the table all the same
    assert not needs_a_stream_test(decl["cip_ldlt_workspace_bytes"]) and not needs_a_stream_test(decl["cip_set_solve_fused"])


def test_every_streamed_entry_point_is_in_the_table_or_exempt():
    decl = declarations()
    table, tests = stream_table()
    exempt = {f: why for why, fns in EXEMPT.items() for f in fns}
    assert all(why.strip() for why in EXEMPT)
    unknown = sorted((set(table) | set(exempt)) - set(decl))
    assert not unknown, "not declared in include/cipkkt.h: %s" % unknown
    both = sorted(set(table) & set(exempt))
    assert not both, "in the table and exempt: %s" % both
    missing = sorted(f for f, params in decl.items() if needs_a_stream_test(params) and f not in table and f not in exempt)
    assert not missing, "no late-stream test and no exemption: %s" % missing
    # the calls that take a handle alone but enqueue on its stream are in the table too
    for f in ("cip_factor", "cip_check_factor", "cip_set_scaling_identity", "cip_assemble_only"):
        assert f in table, f


def test_the_table_names_tests_that_exist_and_call_the_entry_point():
    table, tests = stream_table()
    src = open(STREAMS).read()
    for f, names in table.items():
        assert names, f
        for t in names:
            assert t in tests, "%s: no test %s in tests/test_gpu_streams.py" % (f, t)
    # every stand-alone entry point is called there with the stream argument of the run, never with a literal None
    for f, params in declarations().items():
        if re.search(r"\bhip_stream\b", params) and f != "cip_set_stream":
            calls = re.findall(r"lib\.%s\(([^,]+)," % f, src)
            assert calls and all(c.strip() == "r.ptr" for c in calls), (f, calls)
