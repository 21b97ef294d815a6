"""Host side of the grouped top-K search (include/coot_hip.h: coot_retrieval_topk_grouped, coot_retrieval_topk_grouped_workspace_bytes;
retrieval.compute_retrieval_topk_grouped, retrieval_topk_grouped_device, GalleryIndex.search_grouped): the numpy mirror (argsort,
then a walk) against an independent brute force (per-group argmax under the tie rule, then a sort) and at its two identities, the two
new functions declared, bound and exported by both builds under the unchanged ABI version, and the wrappers refusing on the host what
they cannot serve.  Every comparison of results is for byte equality.  The device results are compared with the mirror in
tests/test_gpu_topk_grouped.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_grouped": 18, "coot_retrieval_topk_grouped_workspace_bytes": 5}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _brute(sim, k, groups, g_total, keep=None):
    """Per row and group: the best kept column, (score, column) maximal; the groups sorted by that pair, descending; -1 / -inf where
    they run out.  Plain Python, nothing shared with the mirror."""
    m, n = sim.shape
    grp = np.full((m, k), -1, np.int32)
    idx = np.full((m, k), -1, np.int32)
    sc = np.full((m, k), -np.inf, sim.dtype)
    for i in range(m):
        best = {}
        for j in range(n):
            g = int(groups[j])
            if 0 <= g < g_total and (keep is None or keep[j]):
                key = (float(sim[i, j]), j)
                if g not in best or key > best[g]:
                    best[g] = key
        ranked = sorted(((key, g) for g, key in best.items()), reverse=True)[:k]
        for r, ((_, j), g) in enumerate(ranked):
            grp[i, r], idx[i, r], sc[i, r] = g, j, sim[i, j]
    return grp, idx, sc


def _layouts(rs, n):
    """Group ids of n columns: contiguous runs of 1 - 9 columns, and the same ids scattered."""
    runs = []
    while sum(runs) < n:
        runs.append(int(rs.randint(1, 10)))
    contiguous = np.repeat(np.arange(len(runs)), runs)[:n]
    return {"contiguous": contiguous, "scattered": contiguous[rs.permutation(n)]}


@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (4, 37, 5), (3, 130, 128), (5, 300, 9), (2, 64, 64)])
def test_mirror_against_brute_force(cva, m, n, k):
    from coot_videotext_amd import compute_retrieval_topk_grouped
    rs = np.random.RandomState(m * 1000 + n + k)
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n)).astype(np.float32)
        for name, groups in _layouts(rs, n).items():
            g_total = int(groups.max()) + 1
            keep = rs.rand(n) < 0.6
            wild = groups.copy()  # ids outside [0, G): never returned
            wild[rs.rand(n) < 0.2] = rs.choice([-1, g_total, 2 ** 31 - 1, -7])
            for gr, gt, kp in ((groups, None, None), (groups, g_total, keep), (groups.astype(np.int32), g_total, keep.astype(np.uint8) * 3),
                               (wild, g_total, None), (wild, g_total, keep), (groups, max(g_total // 2, 1), None)):
                got = compute_retrieval_topk_grouped(sim, k, gr, num_groups=gt, keep=kp)
                want = _brute(sim, k, gr, g_total if gt is None else gt, None if kp is None else kp != 0)
                assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32
                for a, b in zip(got, want):
                    assert _bytes_equal(a, b), (name, exact_ties, gt)


def test_mirror_identities_and_edges(cva):
    from coot_videotext_amd import compute_retrieval_topk, compute_retrieval_topk_grouped, compute_retrieval_topk_masked
    rs = np.random.RandomState(5)
    m, n = 6, 50
    for sim in (rs.randn(m, n).astype(np.float32), rs.randint(-1, 2, size=(m, n)).astype(np.float32)):
        keep = rs.rand(n) < 0.5
        # every column its own group: the row search, filtered or not, and group == idx
        for k in (1, 7, n):
            grp, idx, sc = compute_retrieval_topk_grouped(sim, k, np.arange(n))
            want = compute_retrieval_topk(sim, k)
            assert _bytes_equal(idx, want[0]) and _bytes_equal(sc, want[1]) and _bytes_equal(grp, idx)
            grp, idx, sc = compute_retrieval_topk_grouped(sim, k, np.arange(n), num_groups=n, keep=keep)
            want = compute_retrieval_topk_masked(sim, k, keep)
            assert _bytes_equal(idx, want[0]) and _bytes_equal(sc, want[1]) and _bytes_equal(grp, idx)
        # one group: slot 0 is the top-1 row, the rest is unfilled
        grp, idx, sc = compute_retrieval_topk_grouped(sim, 4, np.zeros(n, np.int64), num_groups=1)
        top = compute_retrieval_topk(sim, 1)
        assert _bytes_equal(idx[:, :1], top[0]) and _bytes_equal(sc[:, :1], top[1]) and (grp[:, 0] == 0).all()
        assert (grp[:, 1:] == -1).all() and (idx[:, 1:] == -1).all() and np.isneginf(sc[:, 1:]).all()
    # fewer than k groups left: three groups, one of them masked out entirely
    sim = rs.randn(m, n).astype(np.float32)
    groups = np.arange(n) % 3
    keep = groups != 1
    grp, idx, sc = compute_retrieval_topk_grouped(sim, 5, groups, keep=keep)
    assert (np.sort(grp[:, :2], axis=1) == [0, 2]).all() and (grp[:, 2:] == -1).all() and (idx[:, 2:] == -1).all() and np.isneginf(sc[:, 2:]).all()
    assert _bytes_equal(sc[:, :2], np.take_along_axis(sim, idx[:, :2].astype(np.int64), axis=1))
    assert (groups[idx[:, :2]] == grp[:, :2]).all()
    # ties: of two equal rows of one group the later represents it; of two groups with equal best scores the later row is ahead
    ties = np.zeros((1, 6), np.float32)
    grp, idx, sc = compute_retrieval_topk_grouped(ties, 3, np.array([0, 0, 1, 1, 2, 0]))
    assert grp.tolist() == [[0, 2, 1]] and idx.tolist() == [[5, 4, 3]]
    # nothing in range: all unfilled; k is checked against N, not against the groups
    grp, idx, sc = compute_retrieval_topk_grouped(sim, 2, np.full(n, -1))
    assert (grp == -1).all() and (idx == -1).all() and np.isneginf(sc).all()
    with pytest.raises(AssertionError):
        compute_retrieval_topk_grouped(sim, n + 1, np.arange(n))
    with pytest.raises(AssertionError):
        compute_retrieval_topk_grouped(sim, 5, np.arange(n - 1))
    with pytest.raises(AssertionError):
        compute_retrieval_topk_grouped(sim, 5, np.arange(n), keep=np.ones(n - 1, bool))


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_grouped_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    args = re.search(r"\bcoot_retrieval_topk_grouped\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    assert "const int32_t* groups" in args and "const uint8_t* keep" in args and "int32_t* group_out" in args
    assert lib.coot_retrieval_topk_grouped_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_grouped" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7
    # the workspace size needs no device: it grows with the table, 8 bytes per (query, group), and does not depend on the split options
    f = lib.coot_retrieval_topk_grouped_workspace_bytes
    assert f(16, 1000, 64, 10, 5000) - f(16, 1000, 64, 10, 1000) >= 16 * 4000 * 8
    assert f(0, 1000, 64, 10, 100) == 256 and f(1, 1000, 64, 10, 0) == 256
    got = ctypes.c_int(-1)
    try:
        base = f(3, 1000, 64, 10, 700)
        assert lib.coot_set_option(b"rt_grouped_splits", 5) == 0 and lib.coot_set_option(b"rt_few_splits", 3) == 0
        assert lib.coot_get_option(b"rt_grouped_splits", ctypes.byref(got)) == 0 and got.value == 5
        assert f(3, 1000, 64, 10, 700) == base
    finally:
        assert lib.coot_set_option(b"rt_grouped_splits", 0) == 0 and lib.coot_set_option(b"rt_few_splits", 0) == 0


def test_package_exports(cva):
    for name in ("compute_retrieval_topk_grouped", "retrieval_topk_grouped_device"):
        assert callable(getattr(cva, name)), name
    assert callable(cva.GalleryIndex.search_grouped)


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  groups' dtype and shape are checked first (ValueError), then its
    device ("no CPU fallback", naming the mirror of the grouped search)."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_topk_grouped_device
    q, g = torch.zeros(2, 8), torch.zeros(5, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    calls = (lambda groups, **kw: retrieval_topk_grouped_device(q, g, None, groups, 2, **kw),
             lambda groups, **kw: index.search_grouped(q, 2, groups, **kw))
    for call in calls:
        for groups in (torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)):
            with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_grouped"):
                call(groups, num_groups=1)
        for groups in (torch.zeros(5), torch.zeros(5, dtype=torch.int16), torch.zeros(5, dtype=torch.bool), [0, 0, 0, 0, 0], np.zeros(5, np.int32)):
            with pytest.raises(ValueError, match="torch.int32 or torch.int64"):
                call(groups, num_groups=1)
        for groups in (torch.zeros(4, dtype=torch.int32), torch.zeros(6, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int32)):
            with pytest.raises(ValueError, match="one group id per row"):
                call(groups, num_groups=1)
    with pytest.raises(ValueError, match=r"GalleryIndex.search_grouped: groups of shape"):
        index.search_grouped(q, 2, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"retrieval_topk_grouped_device: groups has to be"):
        retrieval_topk_grouped_device(q, g, None, torch.zeros(5), 2)
    # (width and k are checked after the devices, as in search: tests/test_gpu_topk_grouped.py::test_width_and_k_are_refused_on_the_host)
