"""The advertised sizes of the caller-owned device workspaces (include/cipkkt.h), CPU only: the library loads and answers size
queries without a GPU.

Every workspace is sized and carved by one walk of its layout (csrc/cip_internal.h: CipLayout); a change of a layout moves these
numbers.  The expected values were NOT produced by the code under test: they are what a build of the commit before the layouts
were unified answered (when sizing and carve were two hand-kept copies), recorded once.  A deliberate change of a layout
replaces them with the values of the build before that change, or with values worked out by hand -- never with the new build's.
"""
import ctypes

import pytest

LDLT_BYTES = {        # one solve block; several blocks of 128 (MT / PT reserved); both sides of the Wbuf width change at 4096
    128: 1626624, 256: 3842560, 384: 5665280, 512: 10043904, 1152: 16994816, 2048: 92602880, 3968: 58536704,
    4096: 252314368, 4224: 131519232, 8192: 504628480,
}
LDLT_2048_BYTES_AT_LIMIT = {128: 30212608, 256: 39125504, 512: 56951296, 1024: 92602880}     # cip_set_solve_block_max
SHAPES = ((1, 1), (3, 5), (5, 3), (128, 128), (1000, 37))       # (len, cnt)
QRCP_BYTES = (1280, 1280, 1280, 3840, 2048)
IMCOLS_BYTES = (3072, 3072, 3072, 140288, 316416)


@pytest.fixture(scope="module")
def lib():
    from cipkkt import _lib
    return _lib.load()


def _ldlt_bytes(lib, N):
    nb = ctypes.c_size_t()
    assert lib.cip_ldlt_workspace_bytes(N, ctypes.byref(nb)) == 0
    return nb.value


def test_ldlt_workspace_bytes(lib):
    prev = lib.cip_set_solve_block_max(1024)
    try:
        assert {N: _ldlt_bytes(lib, N) for N in LDLT_BYTES} == LDLT_BYTES
    finally:
        lib.cip_set_solve_block_max(prev)


def test_ldlt_workspace_bytes_under_the_process_wide_solve_block_limit(lib):
    prev = lib.cip_set_solve_block_max(0)
    try:
        got = {}
        for b in LDLT_2048_BYTES_AT_LIMIT:
            lib.cip_set_solve_block_max(b)
            got[b] = _ldlt_bytes(lib, 2048)
        assert got == LDLT_2048_BYTES_AT_LIMIT
    finally:
        lib.cip_set_solve_block_max(prev)
    assert lib.cip_set_solve_block_max(0) == prev


@pytest.mark.parametrize("fn, want", [("cip_qrcp_workspace_bytes", QRCP_BYTES), ("cip_imcols_workspace_bytes", IMCOLS_BYTES)])
def test_qr_workspace_bytes(lib, fn, want):
    nb = ctypes.c_size_t()
    got = []
    for length, cnt in SHAPES:
        assert getattr(lib, fn)(length, cnt, ctypes.byref(nb)) == 0
        got.append(nb.value)
    assert tuple(got) == want


def test_solve_many_scratch_bytes_is_untouched(lib):
    nb = ctypes.c_size_t()
    assert lib.cip_ldlt_solve_many_scratch_bytes(1024, 64, ctypes.byref(nb)) == 0
    assert nb.value == 524288
