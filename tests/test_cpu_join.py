"""Host side of the join of two indexes (include/coot_hip.h: coot_retrieval_cross_join_count, coot_retrieval_cross_join_fill;
GalleryIndex.join, count_join, retrieval_join_device, compute_retrieval_join, retrieval._cross_join_chunks): the two functions
declared, bound, listed and exported by both builds under the unchanged ABI version; the mirror against the range mirror and the
self-join mirror; the chunk planner as a pure function; and the wrappers refusing on the host what they cannot serve.  The device
results are compared in tests/test_gpu_join.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_cross_join_count": 18, "coot_retrieval_cross_join_fill": 22}


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


def test_cross_join_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        assert _params(hdr, name).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    count, fill = _params(hdr, "coot_retrieval_cross_join_count"), _params(hdr, "coot_retrieval_cross_join_fill")
    # fill takes the count call's arguments again, then the scanned table's companions, and the stream last
    head = count[:count.index("int32_t* block_counts")]
    assert head == ("const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype, const float* right_norms, "
                    "const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups, const int32_t* right_groups, "
                    "const float* thresholds, int row0, int rows, int N_left, int N_right, int d, ")
    assert count[len(head):] == "int32_t* block_counts, coot_stream_t stream"
    assert fill.startswith(head)
    assert fill[len(head):] == "const int32_t* block_base, const int64_t* offsets, int64_t capacity, int32_t* rows_out, float* scores_out, coot_stream_t stream"
    assert "workspace" not in count and "workspace" not in fill and "queries" not in count
    assert list(lib.coot_retrieval_cross_join_fill.argtypes[:16]) == list(lib.coot_retrieval_cross_join_count.argtypes[:16])
    assert lib.coot_retrieval_cross_join_fill.argtypes[18] is ctypes.c_int64  # capacity
    # the self-join pair is as it was
    assert _params(hdr, "coot_retrieval_join_count").count(",") + 1 == 12 and _params(hdr, "coot_retrieval_join_fill").count(",") + 1 == 16
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_cross_join" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_cross_join.hip"))
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


def test_the_names_are_exported_by_the_package(cva):
    for name in ("retrieval_join_device", "compute_retrieval_join"):
        assert getattr(cva, name) is getattr(cva.retrieval, name), name
    assert cva.retrieval.compute_retrieval_join is cva.retrieval_mirror.compute_retrieval_join
    assert callable(cva.GalleryIndex.join) and callable(cva.GalleryIndex.count_join)
    assert "repeat_interleave" in cva.GalleryIndex.join.__doc__ and "output_size=T" in cva.GalleryIndex.join.__doc__
    assert cva.retrieval.JOIN_TABLE_BYTES == 1 << 28  # the existing budget, not a second one


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _pairs(res):
    off, rows, sc = res
    return [(i, int(rows[p]), sc[p].tobytes()) for i in range(len(off) - 1) for p in range(off[i], off[i + 1])]


@pytest.fixture(scope="module")
def sims():
    rs = np.random.RandomState(4)
    return [rs.randn(m, n).astype(np.float32) for m, n in ((7, 11), (1, 5), (40, 3), (33, 130))]


def test_mirror_without_filters_is_the_range_mirror(cva, sims):
    rs = np.random.RandomState(5)
    for sim in sims:
        m = sim.shape[0]
        for thr in (0.3, -np.inf, rs.randn(m).astype(np.float32), rs.randn(m).tolist()):
            got = cva.compute_retrieval_join(sim, thr)
            assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
            assert _same(got, cva.compute_retrieval_range(sim, thr))


def test_mirror_keep_empties_the_masked_left_rows_and_nothing_else(cva, sims):
    rs = np.random.RandomState(6)
    for sim in sims:
        m = sim.shape[0]
        thr = (rs.randn(m) * 0.5).astype(np.float32)
        keep = rs.rand(m) < 0.6
        full = cva.compute_retrieval_range(sim, thr)
        for kp in (keep, keep.astype(np.uint8) * 3):
            off, rows, sc = cva.compute_retrieval_join(sim, thr, keep=kp)
            for i in range(m):
                lo, hi = full[0][i], full[0][i + 1]
                if keep[i]:
                    assert rows[off[i]:off[i + 1]].tobytes() == full[1][lo:hi].tobytes() and sc[off[i]:off[i + 1]].tobytes() == full[2][lo:hi].tobytes()
                else:
                    assert off[i] == off[i + 1]
        assert cva.compute_retrieval_join(sim, -np.inf, keep=np.zeros(m, bool))[0].tolist() == [0] * (m + 1)


def test_mirror_other_keep_is_the_range_mirrors_keep(cva, sims):
    rs = np.random.RandomState(7)
    for sim in sims:
        m, n = sim.shape
        thr = (rs.randn(m) * 0.5).astype(np.float32)
        ok = rs.rand(n) < 0.5
        assert _same(cva.compute_retrieval_join(sim, thr, other_keep=ok), cva.compute_retrieval_range(sim, thr, keep=ok))
        assert _same(cva.compute_retrieval_join(sim, thr, other_keep=ok.astype(np.uint8) * 7), cva.compute_retrieval_range(sim, thr, keep=ok))


def test_mirror_groups_act_by_inequality(cva):
    sim = np.arange(12, dtype=np.float32).reshape(3, 4)
    ga, gb = np.array([4, -2, 9]), np.array([4, -2, -2, 5])
    got = cva.compute_retrieval_join(sim, -np.inf, groups=ga, other_groups=gb)
    assert [(i, j) for i, j, _ in _pairs(got)] == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3)]
    assert got[2].tolist() == [sim[i, j] for i, j, _ in _pairs(got)]
    assert _same(got, cva.compute_retrieval_join(sim, -np.inf, groups=ga.astype(np.int32), other_groups=gb.astype(np.int64)))
    assert cva.compute_retrieval_join(sim, -np.inf, groups=np.zeros(3, np.int64), other_groups=np.zeros(4, np.int32))[0].tolist() == [0] * 4
    both = cva.compute_retrieval_join(sim, 5.0, keep=[1, 1, 0], other_keep=[0, 1, 1, 1], groups=ga, other_groups=gb)
    assert [(i, j) for i, j, _ in _pairs(both)] == [(1, 3)]  # (1, 1) and (1, 2): one group; row 0 stays below 5; row 2 does not ask
    for kw in (dict(groups=ga), dict(other_groups=gb)):
        with pytest.raises(ValueError, match="groups and other_groups"):
            cva.compute_retrieval_join(sim, 0.0, **kw)
    with pytest.raises(AssertionError):
        cva.compute_retrieval_join(sim, 0.0, groups=np.zeros(3), other_groups=gb)  # floats are no ids
    with pytest.raises(AssertionError):
        cva.compute_retrieval_join(sim, 0.0, groups=gb, other_groups=ga)  # the sides swapped: wrong lengths
    with pytest.raises(AssertionError):
        cva.compute_retrieval_join(sim, 0.0, keep=np.ones(4))
    with pytest.raises(AssertionError):
        cva.compute_retrieval_join(sim, 0.0, other_keep=np.ones(3))
    with pytest.raises(AssertionError):
        cva.compute_retrieval_join(sim, np.zeros(4))


def test_mirror_per_row_thresholds_and_special_values(cva):
    s = np.zeros((4, 4), np.float32)
    s[0] = [np.nan, -0.0, np.inf, -np.inf]
    s[1] = [0.5, np.nan, -1.0, np.inf]
    s[2] = [np.inf, np.inf, np.nan, 1.0]
    s[3] = [-0.0, 0.0, -np.inf, np.nan]
    f = cva.compute_retrieval_join
    assert [(i, j) for i, j, _ in _pairs(f(s, 0.0))] == [(0, 1), (0, 2), (1, 0), (1, 3), (2, 0), (2, 1), (2, 3), (3, 0), (3, 1)]  # -0 >= +0
    assert np.signbit(f(s, 0.0)[2][0])  # the score's bytes, not a rounded copy
    assert [(i, j) for i, j, _ in _pairs(f(s, -0.0))] == [(i, j) for i, j, _ in _pairs(f(s, 0.0))]
    assert [(i, j) for i, j, _ in _pairs(f(s, np.inf))] == [(0, 2), (1, 3), (2, 0), (2, 1)]  # +inf: only scores that are +inf
    assert f(s, -np.inf)[0].tolist() == [0, 3, 6, 9, 12]  # -inf: everything but the NaNs
    assert f(s, np.nan)[0].tolist() == [0] * 5  # a NaN threshold: nothing
    thr = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
    assert [(i, j) for i, j, _ in _pairs(f(s, thr))] == [(1, 3), (2, 0), (2, 1), (2, 3), (3, 0), (3, 1)]  # the LEFT row's threshold decides
    assert _same(f(s, thr), f(s, thr.tolist())) and _same(f(s, thr), cva.compute_retrieval_range(s, thr))
    assert _same(f(s, np.float64(0.1)), f(s, np.float32(0.1)))  # rounded to float32 once


def test_mirror_on_a_square_symmetric_matrix_holds_the_self_join(cva):
    rs = np.random.RandomState(2)
    n = 37
    a = rs.randn(n, n).astype(np.float32)
    sim = a + a.T  # symmetric on bytes
    assert sim.tobytes() == sim.T.copy().tobytes()
    thr = rs.randn(n).astype(np.float32)
    groups = rs.randint(-2, 3, n)
    for keep in (None, rs.rand(n) < 0.7):
        for gr in (None, groups):
            off, rows, sc = cva.compute_retrieval_join(sim, thr, keep=keep, other_keep=keep, groups=gr, other_groups=gr)
            seg = np.repeat(np.arange(n), np.diff(off))
            sel = rows > seg  # j <= i dropped
            out = np.zeros(n + 1, np.int64)
            out[1:] = np.cumsum(np.bincount(seg[sel], minlength=n))
            assert _same((out, rows[sel], sc[sel]), cva.compute_retrieval_self_join(sim, thr, keep=keep, groups=gr))


# ---- the chunk planner ---------------------------------------------------------------------------------------------------------------

def _table_bytes(n_right, rows):
    return 4 * rows * ((n_right + 127) // 128 + 1)


@pytest.mark.parametrize("n_left", [1, 5, 63, 64, 65, 1000, 18000, 200000, 5000000])
@pytest.mark.parametrize("n_right", [1, 128, 129, 1000, 200000, 1000000])
@pytest.mark.parametrize("budget", [1, 4096, 13824, 1 << 20, 1 << 28, 1 << 62])
def test_chunk_planner(cva, n_left, n_right, budget):
    chunks = cva.retrieval._cross_join_chunks(n_left, n_right, budget)
    assert chunks[0][0] == 0 and sum(r for _, r in chunks) == n_left
    for (row0, rows), nxt in zip(chunks, chunks[1:] + [(n_left, 0)]):
        assert row0 % 64 == 0 and rows >= 1 and row0 + rows == nxt[0]  # in order, [0, n_left) once
        assert rows >= 64 or row0 + rows == n_left  # at least 64 rows, but for what is left at the end
        assert _table_bytes(n_right, rows) <= budget or rows == min(64, n_left - row0)  # within the budget, or the smallest chunk there is
        assert rows <= 65535 * 64
        if row0 + rows < n_left:  # as many rows as fit: 64 more would not have
            assert rows % 64 == 0 and (_table_bytes(n_right, rows + 64) > budget or rows + 64 > 65535 * 64)
    if budget == 1 << 62:
        assert len(chunks) == (n_left + 65535 * 64 - 1) // (65535 * 64)


def test_chunk_planner_counts(cva):
    # 1000 right rows: a table row has ceil(1000 / 128) + 1 = 9 slots, 36 bytes, so 13 824 bytes hold 384 rows
    f = cva.retrieval._cross_join_chunks
    assert f(1000, 1000, 1 << 28) == [(0, 1000)]
    assert f(1000, 1000, 13824) == [(0, 384), (384, 384), (768, 232)]
    assert len(f(1000, 1000, 1)) == 16 and f(1000, 1000, 1)[-1] == (960, 40)
    assert f(200000, 200000, 1 << 28)[0][1] * 4 * (200000 // 128 + 2) <= 1 << 28  # the table the issue's 1.25 GB shrinks to


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
    calls = {"retrieval_join_device": lambda thr=0.5, **kw: cva.retrieval_join_device(a, None, b, None, thr, **kw),
             "GalleryIndex.join": lambda thr=0.5, **kw: left.join(right, thr, **kw),
             "GalleryIndex.count_join": lambda thr=0.5, **kw: left.count_join(right, thr, **kw)}
    cpu = r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_join\)"
    for fn, call in calls.items():
        if fn != "GalleryIndex.count_join":
            for bad in (0, -3, 2.5, True):
                with pytest.raises(ValueError, match=fn + ": max_results = "):
                    call(torch.zeros(4), max_results=bad)  # (before the threshold is looked at)
            with pytest.raises(TypeError):
                call(order="score")  # there is no order= here
            with pytest.raises(RuntimeError, match=fn + cpu):
                call(max_results=7)
        with pytest.raises(ValueError, match=fn + r": threshold of shape \(7,\), 5 queries \(one number, or one per query: \[5\]\)"):
            call(np.zeros(nr, np.float32))  # one threshold per LEFT row
        with pytest.raises(ValueError, match=fn + ": threshold has to be a number or hold one number per query, not dtype"):
            call("0.5")
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"):
            call(torch.zeros(4), keep=torch.ones(nl))  # keep before the threshold
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"):
            call(other_keep=torch.ones(nr))
        with pytest.raises(ValueError, match=fn + r": keep of shape \(7,\), a gallery of 5 rows"):
            call(keep=torch.ones(nr, dtype=torch.bool))  # the right side's length on the left
        with pytest.raises(ValueError, match=fn + r": keep of shape \(5,\), a gallery of 7 rows"):
            call(other_keep=torch.ones(nl, dtype=torch.bool))
        for kw in (dict(groups=torch.zeros(nl, dtype=torch.int32)), dict(other_groups=torch.zeros(nr, dtype=torch.int64))):
            with pytest.raises(ValueError, match=fn + ": groups and other_groups are given together or not at all"):
                call(**kw)
        with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"):
            call(torch.zeros(4), keep=torch.ones(nl), groups=torch.zeros(nl), other_groups=torch.zeros(nr, dtype=torch.int32))  # groups before keep
        with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64 tensor, not list"):
            call(groups=torch.zeros(nl, dtype=torch.int32), other_groups=[0] * nr)
        with pytest.raises(ValueError, match=fn + r": groups of shape \(7,\), a gallery of 5 rows"):
            call(groups=torch.zeros(nr, dtype=torch.int64), other_groups=torch.zeros(nr, dtype=torch.int64))
        with pytest.raises(ValueError, match=fn + r": groups of shape \(5,\), a gallery of 7 rows"):
            call(groups=torch.zeros(nl, dtype=torch.int64), other_groups=torch.zeros(nl, dtype=torch.int64))
        for thr in (0.5, np.zeros(nl, np.float32), torch.zeros(nl), [0.0] * nl):
            for kw in (dict(), dict(keep=torch.ones(nl, dtype=torch.bool)), dict(other_keep=torch.ones(nr, dtype=torch.uint8)),
                       dict(groups=torch.zeros(nl, dtype=torch.int32), other_groups=torch.arange(nr))):
                with pytest.raises(RuntimeError, match=fn + cpu):
                    call(thr, **kw)
    # what two indexes have to share
    for fn, call in (("GalleryIndex.join", lambda l, r: l.join(r, 0.5)), ("GalleryIndex.count_join", lambda l, r: l.count_join(r, 0.5))):
        for other in (b, None, "right", (b, None)):
            with pytest.raises(TypeError, match=fn + ": the right side has to be a GalleryIndex, not "):
                call(left, other)
        with pytest.raises(ValueError, match=fn + ": this index holds rows of width 8, the right one of width 9"):
            call(left, _index(cva, torch.zeros(nr, 9)))
        with pytest.raises(ValueError, match=fn + r": this index has normalize=False, the right one normalize=True \(one similarity needs both norms or none\)"):
            call(left, _index(cva, b, normalize=True))
        with pytest.raises(ValueError, match=fn + r": this index has normalize=True, the right one normalize=False"):
            call(_index(cva, a, normalize=True), right)
        with pytest.raises(ValueError, match=fn + ": this index lives on cpu, the right one on meta"):
            call(left, _index(cva, torch.zeros(nr, 8, device="meta")))
        with pytest.raises(RuntimeError, match=fn + cpu):
            call(left, left)  # the index itself is allowed as the right side
    with pytest.raises(ValueError, match="retrieval_join_device: left rows of width 8, right rows of width 9"):
        cva.retrieval_join_device(a, None, torch.zeros(nr, 9), None, 0.5)
    for norms in ((torch.ones(nl), None), (None, torch.ones(nr))):
        with pytest.raises(ValueError, match="retrieval_join_device: one side brings row norms and the other does not"):
            cva.retrieval_join_device(a, norms[0], b, norms[1], 0.5)
    with pytest.raises(ValueError, match="retrieval_join_device: the right rows live on meta, the left rows on cpu"):
        cva.retrieval_join_device(a, None, torch.zeros(nr, 8, device="meta"), None, 0.5)
