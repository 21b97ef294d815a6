"""Host side of the K best partners of every row (include/coot_hip.h: coot_retrieval_knn_join; GalleryIndex.knn_join, knn_graph,
retrieval_knn_join_device, compute_retrieval_knn_join): the function declared, bound, listed and exported by both builds under the
unchanged ABI version; the mirror against a brute-force loop over the definition and against the masked and scoped mirrors where the
definition says they coincide; and the wrappers refusing on the host what they cannot serve.  The device results are compared in
tests/test_gpu_knn_join.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_knn_join_workspace_bytes": 3, "coot_retrieval_knn_join": 20}


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


def test_knn_join_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        assert _params(hdr, name).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert _params(hdr, "coot_retrieval_knn_join") == (
        "const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype, const float* right_norms, "
        "const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups, const int32_t* right_groups, "
        "int exclude_same_row, int N_left, int N_right, int d, int K, int32_t* idx_out, float* score_out, void* workspace, "
        "size_t workspace_bytes, coot_stream_t stream")
    # the operands and filters come in the order of the join of two indexes
    cross = _params(hdr, "coot_retrieval_cross_join_count")
    assert _params(hdr, "coot_retrieval_knn_join").startswith(cross[:cross.index("const float* thresholds")])
    assert lib.coot_retrieval_knn_join_workspace_bytes.restype is ctypes.c_size_t
    assert lib.coot_retrieval_knn_join.argtypes[18] is ctypes.c_size_t  # workspace_bytes
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_knn" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_knn.hip"))
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in stub, name
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, so


def test_workspace_size_and_split_option_need_no_device(cva):
    lib = cva.lib.load()
    ws = lib.coot_retrieval_knn_join_workspace_bytes
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 6), (5, 300, 129)):
        assert ws(*bad) == 256, bad
    got = ctypes.c_int(-1)
    try:
        assert lib.coot_set_option(b"rt_knn_splits", 1) == 0
        assert lib.coot_get_option(b"rt_knn_splits", ctypes.byref(got)) == 0 and got.value == 1
        assert ws(130, 1000, 10) == 256  # one share writes the result itself: no lists
        assert lib.coot_set_option(b"rt_knn_splits", 3) == 0
        assert ws(130, 1000, 10) == 130 * 3 * 10 * 8 + 256  # 8 blocks in shares of 3: three lists of 10 entries per row
        assert ws(130, 100, 10) == 256  # one block: one share whatever the option says
        assert lib.coot_set_option(b"rt_knn_splits", 1000) == 0
        assert ws(130, 1000, 10) == 130 * 8 * 10 * 8 + 256  # no more shares than blocks
        assert ws(130, 128 * 64, 10) == 130 * 32 * 10 * 8 + 256  # and no more than 32: one merge round
        assert ws(130, 128 * 100, 10) == 130 * 25 * 10 * 8 + 256  # 100 blocks in shares of 4: every share has a block
    finally:
        assert lib.coot_set_option(b"rt_knn_splits", 0) == 0
    assert ws(200000, 200000, 10) == 256  # automatic: 3 125 row tiles fill the device without a split
    assert ws(64, 128 * 256, 10) == 64 * 32 * 10 * 8 + 256  # one row tile: the cap
    assert ws(64, 128 * 64, 10) == 64 * 8 * 10 * 8 + 256  # no share shorter than 8 blocks
    assert ws(18000, 18000, 10) == 18000 * 8 * 10 * 8 + 256  # 282 row tiles: 8 shares make 2 256 workgroups
    assert ws(64, 128 * 7, 10) == 256  # fewer than 8 blocks: one share


def test_the_names_are_exported_by_the_package(cva):
    for name in ("retrieval_knn_join_device", "compute_retrieval_knn_join"):
        assert getattr(cva, name) is getattr(cva.retrieval, name), name
    assert cva.retrieval.compute_retrieval_knn_join is cva.retrieval_mirror.compute_retrieval_knn_join
    assert callable(cva.GalleryIndex.knn_join) and callable(cva.GalleryIndex.knn_graph)
    assert cva.retrieval.KNN_JOIN_ROWS_MAX == 65535 * 64


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def _brute(sim, k, keep=None, other_keep=None, groups=None, other_groups=None, exclude_same_row=False):
    """The definition, pair by pair: the eligible columns of a row sorted by (score, column), both descending."""
    m, n = sim.shape
    idx = np.full((m, k), -1, np.int32)
    sc = np.full((m, k), -np.inf, sim.dtype)
    for i in range(m):
        if keep is not None and not keep[i]:
            continue
        el = []
        for j in range(n):
            if other_keep is not None and not other_keep[j]:
                continue
            if groups is not None and int(groups[i]) == int(other_groups[j]):
                continue
            if exclude_same_row and j == i:
                continue
            el.append((float(sim[i, j]), j))
        el.sort(reverse=True)
        for r, (_, j) in enumerate(el[:k]):
            idx[i, r], sc[i, r] = j, sim[i, j]
    return idx, sc


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def sims():
    rs = np.random.RandomState(4)
    out = [rs.randn(m, n).astype(np.float32) for m, n in ((7, 11), (1, 5), (40, 3), (33, 130), (12, 12))]
    out.append(rs.randint(-2, 3, (20, 20)).astype(np.float32))  # ties everywhere: the larger column is ahead
    return out


def test_mirror_is_the_definition(cva, sims):
    rs = np.random.RandomState(5)
    f = cva.compute_retrieval_knn_join
    for sim in sims:
        m, n = sim.shape
        keep, ok = rs.rand(m) < 0.7, rs.rand(n) < 0.6
        ga = (rs.randint(-2, 3, m).astype(np.int64)) * (2 ** 33 + 5)  # int64 ids, negative ones among them
        gb = (rs.randint(-2, 3, n).astype(np.int64)) * (2 ** 33 + 5)
        for k in sorted({1, min(3, n), n}):
            for kw in (dict(), dict(keep=keep), dict(other_keep=ok), dict(groups=ga, other_groups=gb), dict(exclude_same_row=True),
                       dict(keep=keep, other_keep=ok, groups=ga, other_groups=gb, exclude_same_row=True)):
                got = f(sim, k, **kw)
                assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == got[1].shape == (m, k)
                assert _same(got, _brute(sim, k, **kw)), (sim.shape, k, sorted(kw))


def test_mirror_ties_tail_and_masked_rows(cva):
    f = cva.compute_retrieval_knn_join
    sim = np.array([[1, 2, 2, 0], [3, 3, 3, 3], [0, -0.0, 5, 5]], np.float32)
    idx, sc = f(sim, 3)
    assert idx.tolist() == [[2, 1, 0], [3, 2, 1], [3, 2, 1]]  # equal scores: the larger row first; -0 == +0
    assert np.signbit(sc[2, 2])  # the score's bytes
    idx, sc = f(sim, 4, other_keep=[1, 0, 1, 0])
    assert idx.tolist() == [[2, 0, -1, -1], [2, 0, -1, -1], [2, 0, -1, -1]] and np.isneginf(sc[:, 2:]).all()  # a short tail
    idx, sc = f(sim, 2, keep=[0, 3, 0])
    assert idx.tolist() == [[-1, -1], [3, 2], [-1, -1]] and np.isneginf(sc[[0, 2]]).all()  # a masked row does not ask
    idx, _ = f(sim, 2, exclude_same_row=True)
    assert idx.tolist() == [[2, 1], [3, 2], [3, 1]]  # (2, 2) is the row itself
    idx, _ = f(sim, 2, groups=np.array([7, -1, 7]), other_groups=np.array([7, 7, -1, -1], np.int32))
    assert idx.tolist() == [[2, 3], [1, 0], [3, 2]]
    assert f(sim, 1, groups=np.zeros(3, np.int64), other_groups=np.zeros(4, np.int64))[0].tolist() == [[-1]] * 3
    for kw in (dict(groups=np.zeros(3, np.int64)), dict(other_groups=np.zeros(4, np.int64))):
        with pytest.raises(ValueError, match="groups and other_groups"):
            f(sim, 1, **kw)
    for bad in (dict(k=0), dict(k=5), dict(k=1, keep=np.ones(4)), dict(k=1, other_keep=np.ones(3)),
                dict(k=1, groups=np.zeros(3), other_groups=np.zeros(4, np.int64)), dict(k=1, groups=np.zeros(4, np.int64), other_groups=np.zeros(3, np.int64))):
        with pytest.raises(AssertionError):
            f(sim, **bad)


def test_mirror_coincides_with_the_masked_and_scoped_mirrors(cva, sims):
    rs = np.random.RandomState(6)
    f = cva.compute_retrieval_knn_join
    for sim in sims:
        m, n = sim.shape
        ok = rs.rand(n) < 0.6
        ga, gb = rs.randint(-3, 4, m), rs.randint(-3, 4, n)
        for k in sorted({1, min(4, n), n}):
            assert _same(f(sim, k), cva.compute_retrieval_topk(sim, k))
            assert _same(f(sim, k, other_keep=ok), cva.compute_retrieval_topk_masked(sim, k, ok))
            assert _same(f(sim, k, groups=ga, other_groups=gb), cva.compute_retrieval_topk_scoped(sim, k, gb, exclude=ga))
            assert _same(f(sim, k, other_keep=ok, groups=ga, other_groups=gb), cva.compute_retrieval_topk_scoped(sim, k, gb, exclude=ga, keep=ok))
            if m == n:  # the self case without groups: every row is its own id, as in GalleryIndex.neighbors
                assert _same(f(sim, k, exclude_same_row=True), cva.compute_retrieval_topk_scoped(sim, k, None, exclude=np.arange(n)))
                keep = rs.rand(n) < 0.7
                got = f(sim, k, keep=keep, other_keep=keep, exclude_same_row=True)
                want = cva.compute_retrieval_topk_scoped(sim, k, None, exclude=np.arange(n), keep=keep)
                want[0][~keep], want[1][~keep] = -1, -np.inf
                assert _same(got, want)


# ---- refusals on the host ------------------------------------------------------------------------------------------------------------

def _index(cva, g, normalize=False):
    """An index cannot be built without a device: an instance made by hand."""
    import torch
    index = object.__new__(cva.GalleryIndex)
    index.gallery, index.keep, index.normalize, index._code, index.storage = g, None, normalize, 0, torch.float32
    index.norms = torch.ones(g.shape[0]) if normalize else None
    return index


def test_wrappers_refuse_on_the_host(cva):
    """CPU tensors: every check comes before a launch, under the calling function's name."""
    import torch
    nl, nr = 5, 7
    a, b = torch.zeros(nl, 8), torch.zeros(nr, 8)
    left, right = _index(cva, a), _index(cva, b)
    calls = {"retrieval_knn_join_device": lambda k=3, **kw: cva.retrieval_knn_join_device(a, None, b, None, k, **kw),
             "GalleryIndex.knn_join": lambda k=3, **kw: left.knn_join(right, k, **kw)}
    cpu = r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_knn_join\)"
    for fn, call in calls.items():
        for k in (0, -1, 8, 129):
            with pytest.raises(ValueError, match=fn + f": k = {k} is outside 1 .. min\\(N_right = 7, 128\\)"):
                call(k)
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"):
            call(0, keep=torch.ones(nl))  # keep before k
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"):
            call(other_keep=torch.ones(nr))
        with pytest.raises(ValueError, match=fn + r": keep of shape \(7,\), a gallery of 5 rows"):
            call(keep=torch.ones(nr, dtype=torch.bool))
        with pytest.raises(ValueError, match=fn + r": keep of shape \(5,\), a gallery of 7 rows"):
            call(other_keep=torch.ones(nl, dtype=torch.bool))
        for kw in (dict(groups=torch.zeros(nl, dtype=torch.int32)), dict(other_groups=torch.zeros(nr, dtype=torch.int64))):
            with pytest.raises(ValueError, match=fn + ": groups and other_groups are given together or not at all"):
                call(**kw)
        with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"):
            call(keep=torch.ones(nl), groups=torch.zeros(nl), other_groups=torch.zeros(nr, dtype=torch.int32))  # groups before keep
        with pytest.raises(ValueError, match=fn + r": groups of shape \(7,\), a gallery of 5 rows"):
            call(groups=torch.zeros(nr, dtype=torch.int64), other_groups=torch.zeros(nr, dtype=torch.int64))
        with pytest.raises(ValueError, match=fn + r": groups of shape \(5,\), a gallery of 7 rows"):
            call(groups=torch.zeros(nl, dtype=torch.int64), other_groups=torch.zeros(nl, dtype=torch.int64))
        for kw in (dict(), dict(keep=torch.ones(nl, dtype=torch.bool)), dict(other_keep=torch.ones(nr, dtype=torch.uint8)),
                   dict(groups=torch.zeros(nl, dtype=torch.int32), other_groups=torch.arange(nr))):
            with pytest.raises(RuntimeError, match=fn + cpu):
                call(**kw)
    with pytest.raises(TypeError):
        left.knn_join(right, 3, exclude_same_row=True)  # the flag belongs to the function on bare tensors
    with pytest.raises(RuntimeError, match="retrieval_knn_join_device" + cpu):
        cva.retrieval_knn_join_device(a, None, a, None, 3, exclude_same_row=True)
    # what two indexes have to share
    fn = "GalleryIndex.knn_join"
    for other in (b, None, "right", (b, None)):
        with pytest.raises(TypeError, match=fn + ": the right side has to be a GalleryIndex, not "):
            left.knn_join(other, 3)
    with pytest.raises(ValueError, match=fn + ": this index holds rows of width 8, the right one of width 9"):
        left.knn_join(_index(cva, torch.zeros(nr, 9)), 3)
    with pytest.raises(ValueError, match=fn + r": this index has normalize=False, the right one normalize=True \(one similarity needs both norms or none\)"):
        left.knn_join(_index(cva, b, normalize=True), 3)
    with pytest.raises(ValueError, match=fn + ": this index lives on cpu, the right one on meta"):
        left.knn_join(_index(cva, torch.zeros(nr, 8, device="meta")), 3)
    with pytest.raises(RuntimeError, match=fn + cpu):
        left.knn_join(left, 3)  # the index itself is allowed as the right side
    # the graph: the index against itself
    fn = "GalleryIndex.knn_graph"
    for k in (0, 6):
        with pytest.raises(ValueError, match=fn + f": k = {k} is outside 1 .. min\\(N_right = 5, 128\\)"):
            left.knn_graph(k)
    with pytest.raises(ValueError, match=fn + r": keep of shape \(7,\), a gallery of 5 rows"):
        left.knn_graph(3, keep=torch.ones(nr, dtype=torch.bool))
    with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"):
        left.knn_graph(3, groups=torch.zeros(nl))
    for kw in (dict(), dict(keep=torch.ones(nl, dtype=torch.bool)), dict(groups=torch.arange(nl))):
        with pytest.raises(RuntimeError, match=fn + cpu):
            left.knn_graph(3, **kw)
    # too many left rows for one grid (a tensor without storage: only its shape is looked at)
    big = torch.zeros(65535 * 64 + 1, 8, device="meta")
    with pytest.raises(ValueError, match=r"retrieval_knn_join_device: 4194241 left rows; one call takes 1 .. 4194240"):
        cva.retrieval_knn_join_device(big, None, torch.zeros(nr, 8, device="meta"), None, 3)
    with pytest.raises(ValueError, match="retrieval_knn_join_device: left rows of width 8, right rows of width 9"):
        cva.retrieval_knn_join_device(a, None, torch.zeros(nr, 9), None, 3)
    for norms in ((torch.ones(nl), None), (None, torch.ones(nr))):
        with pytest.raises(ValueError, match="retrieval_knn_join_device: one side brings row norms and the other does not"):
            cva.retrieval_knn_join_device(a, norms[0], b, norms[1], 3)
    with pytest.raises(ValueError, match="retrieval_knn_join_device: the right rows live on meta, the left rows on cpu"):
        cva.retrieval_knn_join_device(a, None, torch.zeros(nr, 8, device="meta"), None, 3)
