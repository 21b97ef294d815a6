"""Host side of the self-join (include/coot_hip.h: coot_retrieval_join_count, coot_retrieval_join_fill; GalleryIndex.self_join,
count_self_join, retrieval_self_join_device, compute_retrieval_self_join, retrieval.JOIN_TABLE_BYTES): the two functions declared,
bound, listed and exported by both builds under the unchanged ABI version; the mirror on hand-made similarity matrices; the chunk
planner as a pure function; and the wrappers refusing on the host what they cannot serve.  The device results are compared in
tests/test_gpu_self_join.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_join_count": 12, "coot_retrieval_join_fill": 16}


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


def test_join_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        assert _params(hdr, name).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    count, fill = _params(hdr, "coot_retrieval_join_count"), _params(hdr, "coot_retrieval_join_fill")
    # fill takes the count call's arguments again, then the scanned table's companions, and the stream last
    head = count[:count.index("int32_t* block_counts")]
    assert fill.startswith(head) and head.endswith("int row0, int rows, int N, int d, ")
    assert fill[len(head):] == "const int32_t* block_base, const int64_t* offsets, int64_t capacity, int32_t* rows_out, float* scores_out, coot_stream_t stream"
    assert "const int32_t* groups" in head and "const int32_t* groups" in _params(hdr, "coot_retrieval_topk_scoped")
    assert "workspace" not in count and "workspace" not in fill and "queries" not in count
    assert list(lib.coot_retrieval_join_fill.argtypes[:10]) == list(lib.coot_retrieval_join_count.argtypes[:10])
    assert lib.coot_retrieval_join_fill.argtypes[12] is ctypes.c_int64  # capacity
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_join" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_join.hip"))
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
    for name in ("retrieval_self_join_device", "compute_retrieval_self_join"):
        assert getattr(cva, name) is getattr(cva.retrieval, name), name
    assert cva.retrieval.compute_retrieval_self_join is cva.retrieval_mirror.compute_retrieval_self_join
    assert callable(cva.GalleryIndex.self_join) and callable(cva.GalleryIndex.count_self_join)
    assert "repeat_interleave" in cva.GalleryIndex.self_join.__doc__ and "one\n        synchronisation when the table fits in one chunk" in cva.GalleryIndex.self_join.__doc__
    assert cva.retrieval.JOIN_TABLE_BYTES == 1 << 28


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def _pairs(res):
    off, rows, sc = res
    return [(i, int(rows[p]), sc[p]) for i in range(len(off) - 1) for p in range(off[i], off[i + 1])]


SIM = np.array([[1.0, 0.9, 0.2, 0.9, 0.5],
                [0.9, 1.0, 0.7, 0.1, 0.9],
                [0.2, 0.7, 1.0, 0.7, 0.3],
                [0.9, 0.1, 0.7, 1.0, 0.6],
                [0.5, 0.9, 0.3, 0.6, 1.0]], np.float32)


def test_mirror_returns_each_pair_once_under_its_smaller_row(cva):
    f = cva.compute_retrieval_self_join
    off, rows, sc = f(SIM, 0.7)
    assert off.dtype == np.int64 and rows.dtype == np.int32 and sc.dtype == np.float32
    assert off.tolist() == [0, 2, 4, 5, 5, 5]
    assert rows.tolist() == [1, 3, 2, 4, 3]  # j > i only (no diagonal, although it is 1.0), ascending inside a segment
    assert sc.tolist() == [np.float32(0.9), np.float32(0.9), np.float32(0.7), np.float32(0.9), np.float32(0.7)]  # on the threshold: a hit
    assert all(i < j for i, j, _ in _pairs((off, rows, sc)))
    # -inf: every pair once, in row order
    off, rows, _ = f(SIM, -np.inf)
    assert off.tolist() == [0, 4, 7, 9, 10, 10] and rows.tolist() == [1, 2, 3, 4, 2, 3, 4, 3, 4, 4]
    # the lower triangle is never read: garbage there changes nothing
    low = SIM.copy()
    low[np.tril_indices(5)] = 7.0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(f(low, 0.7), f(SIM, 0.7)))


def test_mirror_keep_applies_to_both_sides_and_groups_by_inequality(cva):
    f = cva.compute_retrieval_self_join
    keep = np.array([1, 0, 1, 1, 1], np.uint8)
    off, rows, _ = f(SIM, 0.6, keep=keep)
    assert off.tolist() == [0, 1, 1, 2, 3, 3]  # row 1 neither asks (its segment is empty) nor is returned
    assert rows.tolist() == [3, 3, 4]
    assert f(SIM, 0.6, keep=keep.astype(bool))[1].tolist() == [3, 3, 4] and f(SIM, 0.6, keep=keep * 5)[1].tolist() == [3, 3, 4]
    groups = np.array([4, 4, -2, 4, -2])
    assert [(i, j) for i, j, _ in _pairs(f(SIM, 0.6, groups=groups))] == [(1, 2), (1, 4), (2, 3), (3, 4)]  # (0, 1), (0, 3): one group
    assert [(i, j) for i, j, _ in _pairs(f(SIM, 0.6, keep=keep, groups=groups.astype(np.int32)))] == [(2, 3), (3, 4)]
    assert f(SIM, -np.inf, groups=np.zeros(5, np.int64))[0].tolist() == [0] * 6  # one group: no pair at all
    assert f(SIM, -np.inf, groups=np.arange(5))[0][-1] == 10  # every row its own group: every pair


def test_mirror_per_row_thresholds_and_special_values(cva):
    f = cva.compute_retrieval_self_join
    thr = np.array([0.9, 0.95, -np.inf, np.inf, 0.0], np.float32)
    off, rows, _ = f(SIM, thr)
    assert off.tolist() == [0, 2, 2, 4, 4, 4] and rows.tolist() == [1, 3, 3, 4]  # the threshold of the SMALLER row decides
    assert f(SIM, thr.tolist())[1].tolist() == [1, 3, 3, 4] and f(SIM, np.float64(0.7))[0].tolist() == f(SIM, 0.7)[0].tolist()
    s = np.zeros((4, 4), np.float32)
    s[0, 1], s[0, 2], s[0, 3] = np.nan, -0.0, np.inf
    s[1, 2], s[1, 3] = np.nan, -np.inf
    s[2, 3] = np.inf
    assert [(i, j) for i, j, _ in _pairs(f(s, 0.0))] == [(0, 2), (0, 3), (2, 3)]  # -0 >= +0 holds; a NaN score is no hit
    assert np.signbit(f(s, 0.0)[2][0])  # the score's bytes, not a rounded copy
    assert [(i, j) for i, j, _ in _pairs(f(s, np.inf))] == [(0, 3), (2, 3)]  # +inf: only scores that are +inf
    assert [(i, j) for i, j, _ in _pairs(f(s, -np.inf))] == [(0, 2), (0, 3), (1, 3), (2, 3)]  # -inf: everything but the NaNs
    assert f(s, np.nan)[0].tolist() == [0] * 5  # a NaN threshold: nothing
    assert f(s, [np.nan, -np.inf, 0.0, 0.0])[0].tolist() == [0, 0, 1, 2, 2]
    with pytest.raises(AssertionError):
        f(np.zeros((3, 4), np.float32), 0.0)
    with pytest.raises(AssertionError):
        f(SIM, np.zeros(4))
    with pytest.raises(AssertionError):
        f(SIM, 0.0, keep=np.ones(4))
    with pytest.raises(AssertionError):
        f(SIM, 0.0, groups=np.zeros(5))  # floats are no ids


def test_mirror_is_the_range_mirror_with_the_left_half_dropped(cva):
    rs = np.random.RandomState(2)
    n = 37
    a = rs.randn(n, n).astype(np.float32)
    sim = a + a.T  # symmetric on bytes
    assert sim.tobytes() == sim.T.copy().tobytes()
    thr = rs.randn(n).astype(np.float32)
    for keep in (None, rs.rand(n) < 0.7):
        off, rows, sc = cva.compute_retrieval_self_join(sim, thr, keep=keep)
        for i in range(n):
            _, r, s = cva.compute_retrieval_range(sim[i:i + 1], thr[i], keep=keep)
            sel = r > i
            if keep is not None and not keep[i]:
                sel[:] = False
            assert rows[off[i]:off[i + 1]].tobytes() == r[sel].tobytes() and sc[off[i]:off[i + 1]].tobytes() == s[sel].tobytes(), i
        # and the pairs a full range search holds twice are held once
        full = cva.compute_retrieval_range(sim, -np.inf, keep=keep)[0][-1]
        kept = n if keep is None else int(keep.sum())
        assert cva.compute_retrieval_self_join(sim, -np.inf, keep=keep)[0][-1] == kept * (kept - 1) // 2 and full == n * kept


# ---- the chunk planner ---------------------------------------------------------------------------------------------------------------

def _table_bytes(n, row0, rows):
    return 4 * rows * ((n - row0 + 127) // 128 + 1)


@pytest.mark.parametrize("n", [1, 5, 127, 128, 129, 1000, 18000, 200000, 1000000])
@pytest.mark.parametrize("budget", [1, 4096, 20000, 1 << 20, 1 << 28, 1 << 62])
def test_chunk_planner(cva, n, budget):
    chunks = cva.retrieval._join_chunks(n, budget)
    assert chunks[0][0] == 0 and sum(r for _, r in chunks) == n
    for (row0, rows), nxt in zip(chunks, chunks[1:] + [(n, 0)]):
        assert row0 % 128 == 0 and rows >= 1 and row0 + rows == nxt[0]  # in order, [0, n) once
        assert rows >= 128 or row0 + rows == n  # at least 128 rows, but for what is left at the end
        assert _table_bytes(n, row0, rows) <= budget or rows == min(128, n - row0)  # within the budget, or the smallest chunk there is
        assert rows <= 65535 * 64
        if row0 + rows < n:  # as many rows as fit: 128 more would not have
            assert rows % 128 == 0 and (_table_bytes(n, row0, rows + 128) > budget or rows + 128 > 65535 * 64)
    if budget == 1 << 62 and n <= 65535 * 64:
        assert chunks == [(0, n)]
    if n == 1000:
        assert len(cva.retrieval._join_chunks(n, 1)) == 8 and len(cva.retrieval._join_chunks(n, 1 << 28)) == 1
    if n == 200000 and budget == 1 << 28:
        assert 3 <= len(chunks) <= 8 and chunks[1][1] > chunks[0][1]  # later chunks are narrower, so longer


# ---- refusals on the host ------------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_on_the_host(cva):
    """CPU tensors: the checks and their order are those of the range search, under the calling function's name."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_self_join_device
    n = 5
    g = torch.zeros(n, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    calls = {"retrieval_self_join_device": lambda thr=0.5, **kw: retrieval_self_join_device(g, None, thr, **kw),
             "GalleryIndex.self_join": lambda thr=0.5, **kw: index.self_join(thr, **kw),
             "GalleryIndex.count_self_join": lambda thr=0.5, **kw: index.count_self_join(thr, **kw)}
    for fn, call in calls.items():
        if fn != "GalleryIndex.count_self_join":
            for bad in (0, -3, 2.5, True):
                with pytest.raises(ValueError, match=fn + ": max_results = "):
                    call(torch.zeros(4), max_results=bad)  # (before the threshold is looked at)
            with pytest.raises(TypeError):
                call(order="score")  # there is no order= here
            with pytest.raises(RuntimeError, match=fn + r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_self_join\)"):
                call(max_results=7)
        with pytest.raises(ValueError, match=fn + r": threshold of shape \(4,\), 5 queries \(one number, or one per query: \[5\]\)"):
            call(np.zeros(4, np.float32))
        with pytest.raises(ValueError, match=fn + ": threshold has to be a number or hold one number per query, not dtype"):
            call("0.5")
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"):
            call(torch.zeros(4), keep=torch.ones(n))  # keep before the threshold
        with pytest.raises(ValueError, match=fn + r": keep of shape \(4,\), a gallery of 5 rows"):
            call(keep=torch.ones(4, dtype=torch.bool))
        with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"):
            call(torch.zeros(4), keep=torch.ones(n), groups=torch.zeros(n))  # groups before keep
        with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64 tensor, not list"):
            call(groups=[0] * n)
        with pytest.raises(ValueError, match=fn + r": groups of shape \(6,\), a gallery of 5 rows"):
            call(groups=torch.zeros(6, dtype=torch.int64))
        for thr in (0.5, np.zeros(n, np.float32), torch.zeros(n), [0.0] * n):
            for kw in (dict(), dict(keep=torch.ones(n, dtype=torch.bool)), dict(groups=torch.zeros(n, dtype=torch.int32)),
                       dict(keep=torch.ones(n, dtype=torch.uint8), groups=torch.arange(n))):
                with pytest.raises(RuntimeError, match=fn + r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_self_join\)"):
                    call(thr, **kw)
