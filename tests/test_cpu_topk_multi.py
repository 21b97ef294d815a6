"""Host side of the multi-vector top-K search (include/coot_hip.h: coot_retrieval_topk_multi, coot_retrieval_topk_multi_workspace_bytes;
retrieval.compute_retrieval_topk_multi, retrieval_topk_multi_device, GalleryIndex.search_multi): the numpy mirror on a case worked out
by hand, against an independent brute force, at its identity with the grouped mirror and at a sum whose fp32 value depends on the
order; the two new functions declared, bound and exported by both builds under the unchanged ABI version; how a search is cut into
library calls; and the wrappers refusing on the host what they cannot serve.  Every comparison of results is for byte equality.  The
device results are compared with the mirror in tests/test_gpu_topk_multi.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_multi": 21, "coot_retrieval_topk_multi_workspace_bytes": 6}
NINF = -np.inf


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_mirror_on_a_case_worked_out_by_hand(cva):
    """Three groups over eight columns, two of them with ids outside [0, 3); three sentences in the paragraphs [0, 2), [2, 2) and [2, 3).
    Paragraph 0: group 0 scores 3 + 2, group 1 2 + 1, group 2 5 + 0: the groups 0 and 2 tie at 5 and the larger id is ahead.  Inside a
    group equal columns tie to the later one.  k = 4 is more than the three candidates."""
    from coot_videotext_amd import compute_retrieval_topk_multi
    groups = np.array([0, 0, 1, 1, 2, 2, 7, -1])
    sim = np.array([[1, 3, 2, 2, 0, 5, 9, 9],
                    [2, 0, 1, 0, 0, 0, 9, 9],
                    [4, 4, -1, 1, 7, 7, 0, 0]], np.float32)
    offsets = [0, 2, 2, 3]
    grp, sc, rows, rsc = compute_retrieval_topk_multi(sim, offsets, 4, groups, num_groups=3)
    assert grp.dtype == np.int32 and rows.dtype == np.int32 and sc.dtype == np.float32 and rsc.dtype == np.float32
    assert grp.tolist() == [[2, 0, 1, -1], [-1, -1, -1, -1], [2, 0, 1, -1]]
    assert sc.tolist() == [[5, 5, 3, NINF], [NINF] * 4, [7, 4, 1, NINF]]
    assert rows.tolist() == [[5, 1, 3, -1], [5, 0, 2, -1], [5, 1, 3, -1]]
    assert rsc.tolist() == [[5, 3, 2, NINF], [0, 2, 1, NINF], [7, 4, 1, NINF]]
    # keep removes group 1 entirely and the best column of group 2: two candidates, group 2 through column 4
    keep = np.array([1, 1, 0, 0, 1, 0, 1, 1], bool)
    for kp in (keep, keep.astype(np.uint8) * 5):
        grp, sc, rows, rsc = compute_retrieval_topk_multi(sim, np.array(offsets), 4, groups, num_groups=3, keep=kp)
        assert grp.tolist() == [[0, 2, -1, -1], [-1] * 4, [2, 0, -1, -1]]
        assert sc.tolist() == [[5, 0, NINF, NINF], [NINF] * 4, [7, 4, NINF, NINF]]
        assert rows.tolist() == [[1, 4, -1, -1], [0, 4, -1, -1], [4, 1, -1, -1]]
        assert rsc.tolist() == [[3, 0, NINF, NINF], [2, 0, NINF, NINF], [7, 4, NINF, NINF]]
    # num_groups=None: max(groups) + 1 = 8, so column 6 is a group of its own (9 + 9 leads paragraph 0); the id -1 stays outside
    grp, sc, rows, rsc = compute_retrieval_topk_multi(sim, offsets, 2, groups)
    assert grp.tolist() == [[7, 2], [-1, -1], [2, 0]] and sc.tolist() == [[18, 5], [NINF, NINF], [7, 4]]
    assert rows.tolist() == [[6, 5], [6, 5], [5, 1]]
    # a score of -0 is +0, as the device's entries hold it
    grp, sc, rows, rsc = compute_retrieval_topk_multi(np.array([[-0.0, -1.0]], np.float32), [0, 1], 1, [0, 0])
    assert rows.tolist() == [[0]] and not np.signbit(rsc[0, 0]) and not np.signbit(sc[0, 0])
    # nothing in range: every slot unfilled; shapes are asserted like the grouped mirror's
    grp, sc, rows, rsc = compute_retrieval_topk_multi(sim, offsets, 2, np.full(8, -1))
    assert (grp == -1).all() and np.isneginf(sc).all() and (rows == -1).all() and np.isneginf(rsc).all()
    for bad in (dict(k=9), dict(groups=groups[:7]), dict(keep=np.ones(7, bool)), dict(offsets=[0, 2]), dict(offsets=[1, 3]), dict(offsets=[0, 2, 1, 3]),
                dict(offsets=[3]), dict(offsets=[0.0, 3.0]), dict(offsets=[[0, 3]])):
        kw = dict(k=2, groups=groups, keep=None, offsets=offsets)
        kw.update(bad)
        with pytest.raises(AssertionError):
            compute_retrieval_topk_multi(sim, kw["offsets"], kw["k"], kw["groups"], num_groups=3, keep=kw["keep"])


def _brute(sim, offsets, k, groups, g_total, keep=None):
    """Per sentence and group the best kept column, (score, column) maximal; per paragraph the groups that every sentence reaches,
    their scores added one np.float32 at a time, sorted by (sum, group id) descending.  Plain Python, nothing shared with the mirror."""
    m, n = sim.shape
    p_total = len(offsets) - 1
    grp, sc = np.full((p_total, k), -1, np.int32), np.full((p_total, k), -np.inf, np.float32)
    rows, rsc = np.full((m, k), -1, np.int32), np.full((m, k), -np.inf, np.float32)
    best = []
    for i in range(m):
        b = {}
        for j in range(n):
            g = int(groups[j])
            if 0 <= g < g_total and (keep is None or keep[j]):
                key = (float(sim[i, j]), j)
                if g not in b or key > b[g]:
                    b[g] = key
        best.append(b)
    for p in range(p_total):
        sents = range(offsets[p], offsets[p + 1])
        if not len(sents):
            continue
        ranked = []
        for g in set.intersection(*(set(best[i]) for i in sents)):
            s = np.float32(0)
            for i in sents:
                s = np.float32(s + np.float32(best[i][g][0]))
            ranked.append((float(s), g))
        for r, (s, g) in enumerate(sorted(ranked, reverse=True)[:k]):
            grp[p, r], sc[p, r] = g, s
            for i in sents:
                rows[i, r], rsc[i, r] = best[i][g][1], best[i][g][0]
    return grp, sc, rows, rsc


@pytest.mark.parametrize("n,k", [(37, 5), (130, 128), (64, 9)])
def test_mirror_against_brute_force(cva, n, k):
    """Random similarities, and small integers so that sums and columns tie; a paragraph of 40 sentences adds in an order that a
    pairwise sum does not reproduce."""
    from coot_videotext_amd import compute_retrieval_topk_multi
    rs = np.random.RandomState(n + k)
    offsets = [0, 1, 1, 6, 17, 19, 59]
    m = offsets[-1]
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n) * 100).astype(np.float32)
        contiguous = np.repeat(np.arange(n), 3)[:n]
        g_total = int(contiguous.max()) + 1
        keep = rs.rand(n) < 0.6
        wild = contiguous.copy()
        wild[rs.rand(n) < 0.2] = rs.choice([-1, g_total, 2 ** 31 - 1, -7])
        for gr, gt, kp in ((contiguous, None, None), (contiguous[rs.permutation(n)], g_total, keep), (wild, g_total, None), (wild.astype(np.int32), g_total, keep),
                           (contiguous, max(g_total // 2, 1), None)):
            got = compute_retrieval_topk_multi(sim, offsets, k, gr, num_groups=gt, keep=kp)
            want = _brute(sim, offsets, k, gr, g_total if gt is None else gt, kp)
            for a, b in zip(got, want):
                assert _bytes_equal(a, b), (exact_ties, gt)


def test_single_sentence_paragraphs_are_the_grouped_search(cva):
    from coot_videotext_amd import compute_retrieval_topk_grouped, compute_retrieval_topk_multi
    rs = np.random.RandomState(3)
    m, n = 7, 60
    sim = rs.randn(m, n).astype(np.float32)  # no ties: the two searches order tied groups differently
    groups = rs.randint(0, 14, size=n)
    keep = rs.rand(n) < 0.7
    for k in (1, 6, 20):
        for kp in (None, keep):
            grp, sc, rows, rsc = compute_retrieval_topk_multi(sim, np.arange(m + 1), k, groups, num_groups=14, keep=kp)
            want = compute_retrieval_topk_grouped(sim, k, groups, num_groups=14, keep=kp)
            assert _bytes_equal(grp, want[0]) and _bytes_equal(rows, want[1]) and _bytes_equal(sc, want[2]) and _bytes_equal(rsc, want[2])


def test_the_sum_runs_over_the_sentences_in_order(cva):
    """fp32: (1 + 1e8) - 1e8 = 0 and (1e8 - 1e8) + 1 = 1.  One column, one group: the paragraph's score is the sum of its column."""
    from coot_videotext_amd import compute_retrieval_topk_multi
    sim = np.array([[1], [1e8], [-1e8], [1e8], [-1e8], [1]], np.float32)
    grp, sc, rows, rsc = compute_retrieval_topk_multi(sim, [0, 3, 6], 1, [0])
    assert grp.tolist() == [[0], [0]] and sc.tolist() == [[0.0], [1.0]] and (rows == 0).all() and _bytes_equal(rsc, sim)
    # 50 sentences of mixed magnitude: one float32 add after the other, not numpy's pairwise sum
    rs = np.random.RandomState(1)
    col = (rs.randn(50, 1) * 10.0 ** rs.randint(-3, 6, size=(50, 1))).astype(np.float32)
    s = np.float32(0)
    for x in col[:, 0]:
        s = np.float32(s + x)
    grp, sc, rows, rsc = compute_retrieval_topk_multi(col, [0, 50], 1, [0])
    assert sc[0, 0].tobytes() == s.tobytes()


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_multi_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    args = re.search(r"\bcoot_retrieval_topk_multi\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    for part in ("const int32_t* groups", "const int32_t* offsets", "const uint8_t* keep", "int32_t* group_out", "int32_t* row_out", "float* row_score_out"):
        assert part in args, part
    assert lib.coot_retrieval_topk_multi_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    srcs = re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert "retrieval_multi" in srcs and "retrieval_grouped" in srcs
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_multi.hip"))
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
    """No device needed.  The table is 8 bytes per (sentence, group); the size does not depend on the split options; arguments out of
    range give 256."""
    lib = cva.lib.load()
    f = lib.coot_retrieval_topk_multi_workspace_bytes
    assert f(4, 48, 1000, 64, 10, 1000) - f(4, 16, 1000, 64, 10, 1000) >= 8 * 32 * 1000
    assert f(4, 19, 1000, 64, 10, 5000) - f(4, 19, 1000, 64, 10, 1000) >= 8 * 19 * 4000
    assert f(40, 19, 1000, 64, 10, 700) > f(4, 19, 1000, 64, 10, 700)  # lists per paragraph and range
    assert f(1, 1, 1, 1, 1, 1) > 256
    for args in ((0, 19, 1000, 64, 10, 100), (65536, 19, 1000, 64, 10, 100), (4, 0, 1000, 64, 10, 100), (4, 19, 0, 64, 10, 100), (4, 19, 1000, 0, 10, 100),
                 (4, 19, 1000, 64, 0, 100), (4, 19, 1000, 64, 10, 0), (4, 19, 1000, 64, 10, 2 ** 26 + 1), (4, 2 ** 14 + 1, 1000, 64, 10, 2 ** 14)):
        assert f(*args) == 256, args
    assert f(4, 2 ** 14, 1000, 64, 10, 2 ** 14) >= 8 * 2 ** 28
    got = ctypes.c_int(-1)
    try:
        base = f(5, 19, 1000, 64, 10, 700)
        assert lib.coot_set_option(b"rt_grouped_splits", 5) == 0 and lib.coot_set_option(b"rt_few_splits", 3) == 0
        assert lib.coot_get_option(b"rt_grouped_splits", ctypes.byref(got)) == 0 and got.value == 5
        assert f(5, 19, 1000, 64, 10, 700) == base
    finally:
        assert lib.coot_set_option(b"rt_grouped_splits", 0) == 0 and lib.coot_set_option(b"rt_few_splits", 0) == 0


def test_package_exports(cva):
    for name in ("compute_retrieval_topk_multi", "retrieval_topk_multi_device"):
        assert callable(getattr(cva, name)), name
    assert callable(cva.GalleryIndex.search_multi)


def test_a_search_is_cut_where_a_paragraph_ends(cva, monkeypatch):
    """retrieval._multi_calls: paragraphs [p0, p1) per library call, at most MULTI_TABLE_ENTRIES table entries unless one paragraph
    alone has more, every paragraph in exactly one call."""
    from coot_videotext_amd import retrieval
    off = np.array([0, 1, 1, 6, 17, 19, 19])
    assert retrieval._multi_calls(off, 37) == [(0, 6)]
    monkeypatch.setattr(retrieval, "MULTI_TABLE_ENTRIES", 6 * 37)
    assert retrieval._multi_calls(off, 37) == [(0, 3), (3, 4), (4, 6)]  # 1 + 0 + 5 sentences, 11 (alone above the budget), 2 + 0
    monkeypatch.setattr(retrieval, "MULTI_TABLE_ENTRIES", 1)
    assert retrieval._multi_calls(off, 37) == [(p, p + 1) for p in range(6)]
    monkeypatch.setattr(retrieval, "MULTI_PARAGRAPHS_MAX", 4)
    monkeypatch.setattr(retrieval, "MULTI_TABLE_ENTRIES", 1 << 25)
    assert retrieval._multi_calls(off, 37) == [(0, 4), (4, 6)]


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  The types and shapes of groups, keep and offsets are checked first
    (ValueError), then the devices ("no CPU fallback", naming the mirror of this search)."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_topk_multi_device
    q, g = torch.zeros(3, 8), torch.zeros(5, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    good = torch.zeros(5, dtype=torch.int32)
    calls = {"retrieval_topk_multi_device": lambda offsets, groups=good, **kw: retrieval_topk_multi_device(q, offsets, g, None, groups, 2, **kw),
             "GalleryIndex.search_multi": lambda offsets, groups=good, **kw: index.search_multi(q, offsets, 2, groups, **kw)}
    for fn, call in calls.items():
        for offsets in ([0, 1, 3], (0, 3), np.array([0, 0, 3, 3]), np.array([0, 2, 3], np.int32), torch.tensor([0, 2, 3]), torch.tensor([0, 3], dtype=torch.int32)):
            for groups in (good, torch.zeros(5, dtype=torch.int64)):
                with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_multi"):
                    call(offsets, groups, num_groups=1)
            with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_multi"):
                call(offsets, num_groups=1, keep=torch.ones(5, dtype=torch.bool))
        for offsets in ([0], [], 3, None, "03", [0.0, 3.0], np.array([0.0, 3.0]), torch.tensor([0.0, 3.0]), torch.tensor([True, True]), [[0, 3]], np.zeros((2, 2), np.int64)):
            with pytest.raises(ValueError, match=fn + ": offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers"):
                call(offsets, num_groups=1)
        for offsets in ([1, 3], [0, 2], [0, 1, 4], [-1, 3], torch.tensor([0, 5])):
            with pytest.raises(ValueError, match=fn + ": offsets runs from .* start at 0 and end at M = 3"):
                call(offsets, num_groups=1)
        for offsets in ([0, 2, 1, 3], np.array([0, 3, 0, 3])):
            with pytest.raises(ValueError, match=fn + ": offsets decreases at entry 2"):
                call(offsets, num_groups=1)
        for groups in (torch.zeros(5), torch.zeros(5, dtype=torch.int16), [0, 0, 0, 0, 0], np.zeros(5, np.int32)):
            with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64"):
                call([0, 3], groups, num_groups=1)
        for groups in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.int32)):
            with pytest.raises(ValueError, match="one group id per row"):
                call([0, 3], groups, num_groups=1)
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8"):
            call([0, 3], num_groups=1, keep=torch.ones(5))
        with pytest.raises(ValueError, match="one flag per row"):
            call([0, 3], num_groups=1, keep=torch.ones(4, dtype=torch.bool))
    # (offsets on the device, width and k: tests/test_gpu_topk_multi.py::test_width_k_and_offsets_are_refused_on_the_host)
