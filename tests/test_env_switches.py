"""The library's environment switches and their documentation cannot drift apart: every `CIP_*` variable the C++ sources
read goes through one of the `cip_env_*` helpers (csrc/cip_internal.h, defined in api.hip), and the set of names handed to
them is exactly the set INTEGRATION.md section 6 lists -- apart from the names that section documents as read by Python or
Julia."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conicip.jl_amd", "csrc")
DOC = os.path.join(ROOT, "INTEGRATION.md")
NOT_READ_BY_THE_LIBRARY = {"CIP_BATCH", "CIP_LIBCIPKKT", "CIPKKT_LIB"}
HELPER_DEF = re.compile(r"^\w+ cip_env_\w+\(const char \*name[^)]*\) \{")


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            yield f, open(os.path.join(CSRC, f)).read()


def _code_lines(text):
    """(line number, line without its // comment) of every line"""
    for k, line in enumerate(text.splitlines(), 1):
        yield k, line.split("//", 1)[0]


def _documented():
    text = open(DOC).read()
    sec = text[text.index("## 6. Environment switches"):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    names = set()
    for line in sec.splitlines():
        if not line.startswith("|"):
            continue
        first = line.split("|")[1]
        names.update(re.findall(r"`(CIP[A-Z0-9_]*)`", first))
    return names


def test_documented_switches_are_the_ones_read():
    read = set()
    for _, text in _sources():
        read.update(re.findall(r"\bcip_env_\w+\(\s*\"(CIP_[A-Z0-9_]+)\"", text))
    documented = _documented()
    assert read, "no cip_env_* call found"
    assert NOT_READ_BY_THE_LIBRARY <= documented
    assert read == documented - NOT_READ_BY_THE_LIBRARY, (
        "read but not in INTEGRATION.md section 6: %s; documented but not read: %s"
        % (sorted(read - documented), sorted(documented - NOT_READ_BY_THE_LIBRARY - read)))


def test_getenv_only_inside_the_helpers():
    stray, helpers = [], 0
    for f, text in _sources():
        for k, code in _code_lines(text):
            if not re.search(r"\bgetenv\s*\(", code):
                continue
            if f == "api.hip" and HELPER_DEF.match(code):
                helpers += 1
            else:
                stray.append("%s:%d" % (f, k))
    assert not stray, "getenv outside the cip_env_* helpers: %s" % stray
    assert helpers == 4
