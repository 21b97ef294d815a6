"""Host side of the tile route of the range search (include/coot_hip.h: coot_retrieval_range_tile_workspace_bytes,
coot_retrieval_range_tile_count, _fill; retrieval.RANGE_TILE_MIN_M, RANGE_TILE_MIN_M_16BIT): the new functions declared, bound, listed
and exported by both builds under the unchanged ABI version; the workspace size; the routing constants; and the wrappers refusing on the
host what they cannot serve, whichever route a call would take.  The device results are compared in tests/test_gpu_range_tile.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_range_tile_workspace_bytes": 3, "coot_retrieval_range_tile_count": 13, "coot_retrieval_range_tile_fill": 17}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def _params(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return " ".join(m.group(1).split())


def test_range_tile_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        assert _params(hdr, name).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    # the two passes take the arguments of their siblings on the sweep, one for one
    assert _params(hdr, "coot_retrieval_range_tile_count") == _params(hdr, "coot_retrieval_range_count")
    assert _params(hdr, "coot_retrieval_range_tile_fill") == _params(hdr, "coot_retrieval_range_fill")
    assert list(lib.coot_retrieval_range_tile_count.argtypes) == list(lib.coot_retrieval_range_count.argtypes)
    assert list(lib.coot_retrieval_range_tile_fill.argtypes) == list(lib.coot_retrieval_range_fill.argtypes)
    assert lib.coot_retrieval_range_tile_fill.argtypes[11] is ctypes.c_int64  # capacity
    assert lib.coot_retrieval_range_tile_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_range_tile" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_range_tile.hip"))
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in stub, name
    declared = set(re.findall(r"\b(coot_[a-z0-9_]+)\s*\(", hdr)) - {"coot_stream_t"}
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert exported == declared, (so, sorted(exported ^ declared)[:5])  # exactly the header's names
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_workspace_size(cva):
    """No device needed.  The query norms only: it grows with M and depends on neither N nor d; each argument out of range gives 256."""
    f = cva.lib.load().coot_retrieval_range_tile_workspace_bytes
    assert f(1, 1, 1) > 256
    assert f(4917, 200000, 768) - 256 >= 4917 * 4
    assert f(100000, 1000, 64) - f(1000, 1000, 64) >= 99000 * 4
    assert f(130, 1000, 64) == f(130, 5, 768) == f(130, 200000, 1)
    top = 65535 * 64
    assert f(top, 1000, 64) - 256 >= top * 4
    for args in ((0, 1000, 64), (-1, 1000, 64), (top + 1, 1000, 64), (4, 0, 64), (4, -5, 64), (4, 1000, 0), (4, 1000, -1)):
        assert f(*args) == 256, args


def test_routing_constants(cva):
    r = cva.retrieval
    for name in ("RANGE_TILE_MIN_M", "RANGE_TILE_MIN_M_16BIT"):
        v = getattr(r, name)
        assert type(v) is int and v > r.RETRIEVAL_FEW_MAX, (name, v)  # up to 16 queries the sweep always serves


@pytest.mark.parametrize("threshold_m", [1, 10 ** 9])
def test_wrappers_refuse_on_the_host_on_either_route(cva, monkeypatch, threshold_m):
    """CPU tensors and 40 queries, more than any slice: the checks and their order are those of tests/test_cpu_range.py whether the
    call would have gone to the tile route (constants at 1) or to the slices (at 10^9)."""
    import numpy as np
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_range_device
    monkeypatch.setattr(cva.retrieval, "RANGE_TILE_MIN_M", threshold_m)
    monkeypatch.setattr(cva.retrieval, "RANGE_TILE_MIN_M_16BIT", threshold_m)
    m = 40
    q, g = torch.zeros(m, 8), torch.zeros(5, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    calls = {"retrieval_range_device": lambda thr=0.5, **kw: retrieval_range_device(q, g, None, thr, **kw),
             "GalleryIndex.search_range": lambda thr=0.5, **kw: index.search_range(q, thr, **kw),
             "GalleryIndex.count_range": lambda thr=0.5, **kw: index.count_range(q, thr, **kw)}
    for fn, call in calls.items():
        if fn != "GalleryIndex.count_range":
            with pytest.raises(ValueError, match=fn + r': order="score" needs max_results=None'):
                call(order="score", max_results=10)
            with pytest.raises(ValueError, match=fn + ": max_results = 0"):
                call(torch.zeros(4), max_results=0)  # (before the threshold is looked at)
            for kw in (dict(), dict(max_results=7), dict(order="score")):
                with pytest.raises(RuntimeError, match=fn + r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_range\)"):
                    call(**kw)
        with pytest.raises(ValueError, match=fn + r": threshold of shape .*, 40 queries \(one number, or one per query: \[40\]\)"):
            call(np.zeros(4, np.float32))
        with pytest.raises(ValueError, match=fn + ": threshold has to be a number or hold one number per query, not dtype"):
            call("0.5")
        for thr in (0.5, np.zeros(m, np.float32), torch.zeros(m)):
            with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_range"):
                call(thr)
            with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_range"):
                call(thr, keep=torch.ones(5, dtype=torch.bool))
        with pytest.raises(ValueError, match=fn + ": keep has to be"):
            call(torch.zeros(4), keep=torch.ones(5))  # keep before the threshold
