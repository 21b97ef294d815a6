"""Host side of the filtered top-K search (include/coot_hip.h: coot_retrieval_topk_masked, coot_retrieval_topk_few_masked;
retrieval.compute_retrieval_topk_masked, keep= of retrieval_topk_device and GalleryIndex.search): the numpy mirror against a
brute-force sort and at its edges, the two new functions declared, bound and exported by both builds under the unchanged ABI
version, and the wrappers refusing on the host what they cannot serve.  Every comparison of results is for byte equality.  The
device results are compared with the unfiltered search on the compacted gallery in tests/test_gpu_topk_masked.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_masked": 14, "coot_retrieval_topk_few_masked": 15}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _brute(sim, k, keep):
    """Per row: the kept columns sorted by (score, index), descending, in plain Python; -1 / -inf where they run out."""
    m, n = sim.shape
    idx = np.full((m, k), -1, np.int32)
    sc = np.full((m, k), -np.inf, sim.dtype)
    for i in range(m):
        best = sorted(((float(sim[i, j]), j) for j in range(n) if keep[j]), reverse=True)[:k]
        for r, (_, j) in enumerate(best):
            idx[i, r], sc[i, r] = j, sim[i, j]
    return idx, sc


@pytest.mark.parametrize("m,n,k,frac", [(1, 1, 1, 0.5), (4, 37, 5, 0.5), (7, 130, 128, 0.5), (3, 300, 9, 0.02), (5, 64, 64, 0.9)])
def test_mirror_against_brute_force(cva, m, n, k, frac):
    from coot_videotext_amd import compute_retrieval_topk_masked
    rs = np.random.RandomState(m * 1000 + n + k)
    for trial in range(3):
        sim = rs.randn(m, n).astype(np.float32)
        keep = rs.rand(n) < frac
        for mask in (keep, keep.astype(np.uint8) * 3):  # booleans, or bytes of which any nonzero value keeps
            idx, sc = compute_retrieval_topk_masked(sim, k, mask)
            want_idx, want_sc = _brute(sim, k, keep)
            assert idx.dtype == np.int32 and sc.dtype == np.float32
            assert _bytes_equal(idx, want_idx) and _bytes_equal(sc, want_sc), (trial, keep.sum())


def test_mirror_edges(cva):
    from coot_videotext_amd import compute_retrieval_topk, compute_retrieval_topk_masked
    rs = np.random.RandomState(3)
    m, n = 6, 50
    sim = rs.randn(m, n).astype(np.float32)
    # all kept: the unfiltered mirror
    for k in (1, 5, n):
        got, want = compute_retrieval_topk_masked(sim, k, np.ones(n, bool)), compute_retrieval_topk(sim, k)
        assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1])
    # none kept: nothing to return
    idx, sc = compute_retrieval_topk_masked(sim, 5, np.zeros(n, bool))
    assert _bytes_equal(idx, np.full((m, 5), -1, np.int32)) and _bytes_equal(sc, np.full((m, 5), -np.inf, np.float32))
    # 3 kept at k = 5: the three in order, then the padding
    keep = np.zeros(n, bool)
    keep[[4, 17, 49]] = True
    idx, sc = compute_retrieval_topk_masked(sim, 5, keep)
    assert _bytes_equal(idx, _brute(sim, 5, keep)[0]) and _bytes_equal(sc, _brute(sim, 5, keep)[1])
    assert (np.sort(idx[:, :3], axis=1) == [4, 17, 49]).all() and (idx[:, 3:] == -1).all() and np.isneginf(sc[:, 3:]).all()
    assert _bytes_equal(sc[:, :3], np.take_along_axis(sim, idx[:, :3].astype(np.int64), axis=1))
    # exact ties: of equal scores the later index is ahead, among the kept columns as among all
    ties = rs.randint(-1, 2, size=(m, n)).astype(np.float32)
    keep = rs.rand(n) < 0.6
    idx, sc = compute_retrieval_topk_masked(ties, 20, keep)
    want = _brute(ties, 20, keep)
    assert _bytes_equal(idx, want[0]) and _bytes_equal(sc, want[1])
    for i in range(m):
        for r in range(19):
            assert sc[i, r] > sc[i, r + 1] or (sc[i, r] == sc[i, r + 1] and idx[i, r] > idx[i, r + 1])
    assert keep[idx].all()
    # k is checked against N, not against the mask
    with pytest.raises(AssertionError):
        compute_retrieval_topk_masked(sim, n + 1, np.ones(n, bool))
    with pytest.raises(AssertionError):
        compute_retrieval_topk_masked(sim, 5, np.ones(n - 1, bool))


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_masked_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert "const uint8_t* keep" in m.group(1), name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    assert re.search(r"#define\s+COOT_GALLERY_F32\s+0\b", hdr)  # the code GalleryIndex passes for an fp32 gallery
    # the version script exports by pattern: the new names fall under it and are named in its comment
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert name in vs, name
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  keep's dtype and shape are checked first (ValueError), then the
    devices ("no CPU fallback", naming the mirror of the filtered search)."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_topk_device
    from coot_videotext_amd.retrieval import _check_keep
    q, g = torch.zeros(2, 8), torch.zeros(5, 8)
    for keep in (torch.ones(5, dtype=torch.bool), torch.ones(5, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_masked"):
            retrieval_topk_device(q, g, 2, keep=keep)
        with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_masked"):
            _check_keep("GalleryIndex.search", keep, 5)
    with pytest.raises(RuntimeError, match=r"no CPU fallback; use compute_retrieval_topk\)"):
        retrieval_topk_device(q, g, 2)  # unfiltered: the message it always had
    bad = {"bool or torch.uint8": (torch.ones(5), torch.ones(5, dtype=torch.int32), [1, 1, 1, 1, 1], np.ones(5, bool)),
           "one flag per row": (torch.ones(4, dtype=torch.bool), torch.ones(6, dtype=torch.uint8), torch.ones(5, 1, dtype=torch.bool),
                                torch.ones(1, 5, dtype=torch.bool))}
    for msg, keeps in bad.items():
        for keep in keeps:
            with pytest.raises(ValueError, match=msg):
                retrieval_topk_device(q, g, 2, keep=keep)
            with pytest.raises(ValueError, match=msg):
                _check_keep("GalleryIndex.search", keep, 5)
    # an index cannot be built without a device, so its search is reached through an instance made by hand: keep is looked at first
    index = object.__new__(GalleryIndex)
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    with pytest.raises(ValueError, match="one flag per row"):
        index.search(q, 2, keep=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or torch.uint8"):
        index.search(q, 2, keep=torch.ones(5))
    with pytest.raises(RuntimeError, match="compute_retrieval_topk_masked"):
        index.search(q, 2, keep=torch.ones(5, dtype=torch.bool))
    with pytest.raises(IndexError, match=r"row 5 is outside \[0, 5\)"):
        index.remove([1, 5])
    with pytest.raises(IndexError, match=r"row -1 is outside"):
        index.remove(torch.tensor([-1]))
    with pytest.raises(IndexError, match="row 7"):
        index.restore((0, 7))
    with pytest.raises(TypeError, match="integers"):
        index.remove([0.5])
    assert index.keep is None
    # remove and restore on a host-resident stand-in: the flags themselves are plain tensor operations
    index.remove([1, 3, 3])
    assert index.keep.dtype is torch.bool and index.keep.tolist() == [True, False, True, False, True]
    index.remove(torch.tensor([4]))
    index.restore([3])
    assert index.keep.tolist() == [True, False, True, True, False]
    index.restore()
    assert index.keep is None
