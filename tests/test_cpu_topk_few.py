"""Host side of the few-query search on a prepared gallery (include/coot_hip.h: coot_retrieval_row_norms,
coot_retrieval_topk_few; retrieval.GalleryIndex): the three new functions are declared, bound and exported by both builds under
the unchanged ABI version, the workspace is pure host arithmetic that stops growing with the gallery, and the Python entry
refuses what it cannot serve.  The device results are compared with coot_retrieval_topk byte for byte in
tests/test_gpu_topk_few.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_row_norms": 5, "coot_retrieval_topk_few_workspace_bytes": 4, "coot_retrieval_topk_few": 13}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_few_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert lib.coot_retrieval_topk_few_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_workspace_stops_growing_with_the_gallery(cva):
    """Pure host arithmetic: the partial lists are bounded by the capped split count, so 16 queries against a million rows and
    against ten million need the same workspace, far below the M x N fp32 matrix; the split option does not change it."""
    lib = cva.lib.load()
    m, k, d = 16, 10, 768
    small, large = (lib.coot_retrieval_topk_few_workspace_bytes(m, n, d, k) for n in (10 ** 6, 10 ** 7))
    assert small == large and 0 < small < m * 10 ** 6 * 4 // 16, (small, large)
    assert small >= 32 * 16 * 4 * (d // 32) + m * 1024 * k * 8  # the query copy and 1 024 lists per query are in it
    # it does not grow with d beyond the query copy
    assert lib.coot_retrieval_topk_few_workspace_bytes(m, 10 ** 6, 2 * d, k) - small == d * 16 * 4
    for args in ((0, 100, 8, 1), (1, 0, 8, 1), (1, 100, 0, 1), (1, 100, 8, 0), (-3, -3, -3, -3)):
        assert lib.coot_retrieval_topk_few_workspace_bytes(*args) == 256, args
    try:
        assert lib.coot_set_option(b"rt_few_splits", 3) == 0
        got = ctypes.c_int(-1)
        assert lib.coot_get_option(b"rt_few_splits", ctypes.byref(got)) == 0 and got.value == 3
        assert lib.coot_retrieval_topk_few_workspace_bytes(m, 10 ** 6, d, k) == small
    finally:
        assert lib.coot_set_option(b"rt_few_splits", 0) == 0


def test_gallery_index_refuses_on_the_host(cva):
    import torch
    from coot_videotext_amd import GalleryIndex, RETRIEVAL_FEW_MAX
    m = re.search(r"#define\s+COOT_RETRIEVAL_FEW_MAX\s+(\d+)", _header())
    assert m and int(m.group(1)) == RETRIEVAL_FEW_MAX == cva.retrieval.RETRIEVAL_FEW_MAX
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GalleryIndex(torch.zeros(5, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GalleryIndex(torch.zeros(5, 8), normalize=False)
