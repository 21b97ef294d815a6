"""Host side of the tile route of the adjusted search (include/coot_hip.h: coot_retrieval_topk_adjusted_tile,
coot_retrieval_topk_adjusted_tile_workspace_bytes; retrieval.ADJUSTED_TILE_MIN_M, ADJUSTED_TILE_MIN_M_16BIT): the new functions declared,
bound and exported by both builds; the workspace size, exact; the split option round-trips; and the wrappers refusing on the host what
they refused before, whichever route the constants select.  The device results are compared in tests/test_gpu_adjusted_tile.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_adjusted_tile": 16, "coot_retrieval_topk_adjusted_tile_workspace_bytes": 4}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS

    def args(name):
        return " ".join(re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1).split())
    assert args("coot_retrieval_topk_adjusted_tile") == args("coot_retrieval_topk_adjusted")  # the same arguments in the same order
    assert list(lib.coot_retrieval_topk_adjusted_tile.argtypes) == list(lib.coot_retrieval_topk_adjusted.argtypes)
    assert lib.coot_retrieval_topk_adjusted_tile_workspace_bytes.restype is ctypes.c_size_t
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_adjusted_tile" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_adjusted_tile.hip"))
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\b", vs), name
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, so


def _up(b):
    return (b + 255) // 256 * 256


def _auto_shares(m, n):
    """The plan of the header: about 2 048 workgroups, no share under 8 blocks, at most 32, every share at least one block."""
    mt, nb = (m + 63) // 64, (n + 127) // 128
    s = max(1, min((2048 + mt - 1) // mt, nb // 8, 32, nb))
    blocks = (nb + s - 1) // s
    return (nb + blocks - 1) // blocks


def test_workspace_size_and_the_split_option(cva):
    """No device needed.  Exact: M floats and, for S > 1 shares, M x S x K 64-bit words, each rounded up to 256 bytes; 0 for arguments
    out of range.  The option round-trips and sets S."""
    lib = cva.lib.load()
    f = lib.coot_retrieval_topk_adjusted_tile_workspace_bytes
    val = ctypes.c_int(-1)
    assert lib.coot_get_option(b"rt_adjusted_tile_splits", ctypes.byref(val)) == 0 and val.value == 0
    for m, n, k in ((1, 1000, 10), (130, 1000, 128), (17, 5, 5), (1024, 200000, 10), (17500, 18000, 10), (64, 130, 1)):
        s = _auto_shares(m, n)
        assert f(m, n, 64, k) == _up(4 * m) + (_up(8 * m * s * k) if s > 1 else 0), (m, n, k, s)
    assert _auto_shares(130, 1000) == 1 and _auto_shares(1024, 200000) == 32 and _auto_shares(17500, 18000) == 8
    for args in ((0, 1000, 64, 10), (-1, 1000, 64, 10), (4, 0, 64, 10), (4, 1000, 64, 0), (4, 1000, 64, 129), (4, 5, 64, 6), (4, 1000, 64, -2)):
        assert f(*args) == 0, args
    try:
        for s, shares in ((1, 1), (2, 2), (3, 3), (1000, 8), (5, 4)):  # 8 blocks: five shares of two blocks are four
            assert lib.coot_set_option(b"rt_adjusted_tile_splits", s) == 0
            assert lib.coot_get_option(b"rt_adjusted_tile_splits", ctypes.byref(val)) == 0 and val.value == s
            assert f(130, 1000, 64, 10) == _up(4 * 130) + (_up(8 * 130 * shares * 10) if shares > 1 else 0), s
    finally:
        assert lib.coot_set_option(b"rt_adjusted_tile_splits", 0) == 0
    assert lib.coot_get_option(b"rt_adjusted_tile_splits", ctypes.byref(val)) == 0 and val.value == 0


def test_routing_constants(cva):
    r = cva.retrieval
    for name in ("ADJUSTED_TILE_MIN_M", "ADJUSTED_TILE_MIN_M_16BIT"):
        v = getattr(r, name)
        assert isinstance(v, int) and (v == r.ADJUSTED_TILE_NEVER or v in (17, 32, 64, 128, 256, 320, 512, 1024)), (name, v)  # a measured rung, or never


@pytest.mark.parametrize("route", ["slices", "tile"])
def test_wrappers_refuse_on_the_host_on_either_route(cva, route, monkeypatch):
    """Signatures and the order of the host checks are what they were: keep first, then the offset (ValueError), then the devices."""
    import numpy as np
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_topk_adjusted_device
    v = 1 if route == "tile" else cva.retrieval.ADJUSTED_TILE_NEVER
    monkeypatch.setattr(cva.retrieval, "ADJUSTED_TILE_MIN_M", v)
    monkeypatch.setattr(cva.retrieval, "ADJUSTED_TILE_MIN_M_16BIT", v)
    q, g = torch.zeros(3, 8), torch.zeros(5, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    good = [0.0] * 5
    calls = {"retrieval_topk_adjusted_device": lambda offset=good, k=2, **kw: retrieval_topk_adjusted_device(q, g, None, offset, k, **kw),
             "GalleryIndex.search_adjusted": lambda offset=good, k=2, **kw: index.search_adjusted(q, k, offset, **kw)}
    for fn, call in calls.items():
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8"):
            call("abc", keep=torch.ones(5))  # (before the offset is looked at)
        with pytest.raises(ValueError, match=fn + r": offset of shape .*, a gallery of 5 rows \(one number per row: \[5\]\)"):
            call(np.zeros(6, np.float32))
        with pytest.raises(ValueError, match=fn + ": offset has to hold one number per gallery row, not dtype"):
            call(["a"] * 5)
        for kw in (dict(), dict(keep=torch.ones(5, dtype=torch.bool)), dict(k=0), dict(want_sim=True)):
            with pytest.raises(RuntimeError, match=fn + " needs CUDA tensors .*no CPU fallback; use compute_retrieval_topk_adjusted"):
                call(good, **kw)
