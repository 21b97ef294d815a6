"""Host side of the range search (include/coot_hip.h: coot_retrieval_range_workspace_bytes, coot_retrieval_range_count, _scan, _fill;
retrieval.compute_retrieval_range, retrieval_range_device, GalleryIndex.search_range, GalleryIndex.count_range): the numpy mirror
against an independent brute force; the new functions declared, bound and exported by both builds under the unchanged ABI version;
the workspace size; and the wrappers refusing on the host what they cannot serve.  Every comparison of results is for byte equality.
The device results are compared with the mirror in tests/test_gpu_range.py."""
import ctypes
import fnmatch
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_range_workspace_bytes": 3, "coot_retrieval_range_count": 13, "coot_retrieval_range_scan": 6, "coot_retrieval_range_fill": 17}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _f32(x):
    """A Python number rounded to float32, as a Python float: struct, not numpy."""
    try:
        return struct.unpack("f", struct.pack("f", float(x)))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _brute(sim, thr, keep=None, order="row"):
    """Python floats and Python compares (a float32 widens to a double exactly), nothing shared with the mirror."""
    m, n = sim.shape
    thr = [_f32(thr)] * m if np.ndim(thr) == 0 else [_f32(t) for t in thr]
    offsets, rows, scores = [0], [], []
    for i in range(m):
        hits = [j for j in range(n) if (keep is None or keep[j]) and float(sim[i, j]) >= thr[i]]
        if order == "score":
            hits.sort(key=lambda j: (float(sim[i, j]) + 0.0, j), reverse=True)
        rows += hits
        scores += [sim[i, j] for j in hits]
        offsets.append(len(rows))
    return np.array(offsets, np.int64), np.array(rows, np.int32), np.array(scores, np.float32)


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert all(_bytes_equal(a, b) for a, b in zip(got, want)), (got, want)


@pytest.mark.parametrize("n", [37, 130])
def test_mirror_against_brute_force(cva, n):
    """Random similarities, and small integers (with -0 among them) so that scores tie and sit exactly on the threshold; thresholds
    -inf, +inf, NaN, an exact score, a scalar and one per query; keep as bool and as bytes with values other than 1; both orders."""
    from coot_videotext_amd import compute_retrieval_range
    rs = np.random.RandomState(n)
    m = 9
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n) * 100).astype(np.float32)
        if exact_ties:
            sim[sim == 0] *= rs.choice([-1.0, 1.0], size=int((sim == 0).sum())).astype(np.float32)  # -0 and +0 tie, and -0 >= +0
            assert np.signbit(sim[sim == 0]).any() and not np.signbit(sim[sim == 0]).all()
        sim[2, 5], sim[3, 7] = np.nan, np.inf
        keep = rs.rand(n) < 0.6
        per_query = np.array([-np.inf, np.inf, np.nan, sim[3].max(), np.median(sim[4]), 0.0, -0.0, sim[7, 1], 1e39], np.float64)
        with np.errstate(over="ignore"):
            per_query32 = per_query.astype(np.float32)  # (1e39 becomes +inf)
        for thr in (per_query, per_query32, per_query.tolist(), 0, -0.0, 1.0, 0.1, float("-inf"), float("inf"), float("nan"),
                    np.float32(sim[0, 0]), float(sim[1, 3]), 1e39):
            for kp in (None, keep, keep.astype(np.uint8) * 5):
                for order in ("row", "score"):
                    got = compute_retrieval_range(sim, thr, keep=kp, order=order)
                    _same(got, _brute(sim, thr, kp, order))
        off, rows, sc = compute_retrieval_range(sim, per_query)
        assert off[1] - off[0] == n - int(np.isnan(sim[0]).sum()) and off[2] == off[1] and off[3] == off[2]  # -inf: all; +inf, NaN: none
        assert off[4] - off[3] >= 1 and np.isinf(sc[off[3]:off[4]]).all()  # row 3 holds +inf: its maximum, exactly on the threshold
        assert 5 not in rows[off[2]:off[3]].tolist()
        if exact_ties:  # 0.0 and -0.0 as thresholds take the same rows, zeros of either sign among them
            assert np.signbit(sc[off[5]:off[6]][sc[off[5]:off[6]] == 0]).any()
            a, b = compute_retrieval_range(sim[5:6], 0.0), compute_retrieval_range(sim[5:6], -0.0)
            _same(a, b)
    _same(compute_retrieval_range(np.zeros((0, 4), np.float32), 0.0), (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))


def test_a_host_threshold_is_rounded_to_float32_once(cva):
    from coot_videotext_amd import compute_retrieval_range
    s = np.float32(0.1)
    sim = np.array([[s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))]], np.float32)
    assert float(s) > 0.1  # float32(0.1) lies above the double 0.1: compared as doubles, 0.1 would also take the smaller neighbour
    assert compute_retrieval_range(sim, 0.1)[1].tolist() == [0, 2]
    assert compute_retrieval_range(sim, np.float64(0.1))[1].tolist() == [0, 2]
    assert compute_retrieval_range(sim, [0.1])[1].tolist() == [0, 2]


def test_score_order_is_the_order_of_the_masked_search(cva):
    """For k <= the hit count the first k entries of a segment under order="score" are compute_retrieval_topk_masked's row."""
    from coot_videotext_amd import compute_retrieval_range, compute_retrieval_topk_masked
    rs = np.random.RandomState(5)
    m, n = 7, 90
    sim = rs.randint(-3, 4, size=(m, n)).astype(np.float32)
    sim[sim == 0] *= rs.choice([-1.0, 1.0], size=int((sim == 0).sum())).astype(np.float32)
    keep = rs.rand(n) < 0.7
    thr = np.array([-3, -1, 0, 1, 2, 3, -np.inf], np.float32)
    for kp in (None, keep):
        off, rows, sc = compute_retrieval_range(sim, thr, keep=kp, order="score")
        mask = np.ones(n, bool) if kp is None else kp
        for i in range(m):
            c = int(off[i + 1] - off[i])
            assert c >= 1
            for k in {1, c // 2 + 1, c}:
                idx, top = compute_retrieval_topk_masked(sim[i:i + 1], k, mask)
                assert _bytes_equal(rows[off[i]:off[i] + k], idx[0]) and _bytes_equal(sc[off[i]:off[i] + k], top[0]), (i, k)
            if c < int(mask.sum()):  # the next entry of the search scores below the threshold
                assert compute_retrieval_topk_masked(sim[i:i + 1], c + 1, mask)[1][0, c] < thr[i]


def test_mirror_refuses_bad_arguments(cva):
    from coot_videotext_amd import compute_retrieval_range
    sim = np.zeros((3, 8), np.float32)
    for kw in (dict(threshold=[0, 1]), dict(threshold=[[0, 1, 2]]), dict(keep=np.ones(7, bool)), dict(order="best")):
        with pytest.raises(AssertionError):
            compute_retrieval_range(sim, **dict(dict(threshold=0.0), **kw))
    with pytest.raises(AssertionError):
        compute_retrieval_range(np.zeros(8, np.float32), 0.0)


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_range_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    fill = re.search(r"\bcoot_retrieval_range_fill\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    for part in ("const void* gallery", "int gallery_dtype", "const uint8_t* keep", "const float* thresholds", "const int32_t* block_base",
                 "const int64_t* offsets", "int64_t capacity", "int32_t* rows_out", "float* scores_out"):
        assert part in fill, part
    assert lib.coot_retrieval_range_fill.argtypes[11] is ctypes.c_int64  # capacity
    assert lib.coot_retrieval_range_workspace_bytes.restype is ctypes.c_size_t
    assert re.search(r"#define\s+COOT_RETRIEVAL_RANGE_BLOCK\s+128\b", hdr) and cva.retrieval.RETRIEVAL_RANGE_BLOCK == 128
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_range" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_range.hip"))
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
    """No device needed.  The operand table grows with d; neither M nor N changes the layout; each argument out of range gives 256."""
    f = cva.lib.load().coot_retrieval_range_workspace_bytes
    assert f(4, 1000, 640) - f(4, 1000, 64) >= 4 * 16 * 576  # the operand table [d rounded up to 32][16]
    assert f(1, 1, 1) > 256
    assert f(16, 1000, 64) == f(1, 1000, 64) == f(16, 200000, 64)
    for args in ((0, 1000, 64), (17, 1000, 64), (-1, 1000, 64), (4, 0, 64), (4, -5, 64), (4, 1000, 0), (4, 1000, -1)):
        assert f(*args) == 256, args


def test_package_exports(cva):
    for name in ("compute_retrieval_range", "retrieval_range_device"):
        assert callable(getattr(cva, name)), name
    assert callable(cva.GalleryIndex.search_range) and callable(cva.GalleryIndex.count_range)
    assert cva.retrieval.compute_retrieval_range is cva.retrieval_mirror.compute_retrieval_range


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  max_results and order first, then the types and shapes of keep and the
    threshold (ValueError), then the devices ("no CPU fallback", naming the mirror of this search)."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_range_device
    q, g = torch.zeros(3, 8), torch.zeros(5, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    calls = {"retrieval_range_device": lambda thr=0.5, **kw: retrieval_range_device(q, g, None, thr, **kw),
             "GalleryIndex.search_range": lambda thr=0.5, **kw: index.search_range(q, thr, **kw),
             "GalleryIndex.count_range": lambda thr=0.5, **kw: index.count_range(q, thr, **kw)}
    for fn, call in calls.items():
        if fn != "GalleryIndex.count_range":
            with pytest.raises(ValueError, match=fn + r': order="score" needs max_results=None'):
                call(order="score", max_results=10)
            for c in (0, -1, 2.5, "3", True):
                with pytest.raises(ValueError, match=fn + ": max_results = .* it has to be None .* or an integer >= 1"):
                    call(max_results=c)
            with pytest.raises(ValueError, match=fn + ": order = 'best'"):
                call(order="best")
            with pytest.raises(ValueError, match=fn + ": max_results = 0"):
                call(torch.zeros(4), max_results=0)  # (before the threshold is looked at)
            for kw in (dict(), dict(max_results=7), dict(order="score"), dict(max_results=np.int64(2))):
                with pytest.raises(RuntimeError, match=fn + r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_range\)"):
                    call(**kw)
        for thr in ([0.0, 1.0], [[0.0, 1.0, 2.0]], np.zeros(4, np.float32), torch.zeros(2), torch.zeros(3, 1), []):
            with pytest.raises(ValueError, match=fn + r": threshold of shape .*, 3 queries \(one number, or one per query: \[3\]\)"):
                call(thr)
        for thr in ("0.5", ["a", "b", "c"], None, [None] * 3, np.zeros(3, bool), torch.zeros(3, dtype=torch.bool), 1j, object()):
            with pytest.raises(ValueError, match=fn + ": threshold has to be a number or hold one number per query, not dtype"):
                call(thr)
        for thr in (0.5, 1, np.float32(0.5), float("nan"), [0.0, 1.0, 2.0], (0, 1, 2), np.zeros(3), np.zeros(3, np.float32), np.zeros(3, np.int64),
                    torch.zeros(3), torch.zeros(3, dtype=torch.float64), torch.tensor(0.5)):
            with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_range"):
                call(thr)
            with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_range"):
                call(thr, keep=torch.ones(5, dtype=torch.bool))
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8"):
            call(keep=torch.ones(5))
        with pytest.raises(ValueError, match="one flag per row"):
            call(keep=torch.ones(4, dtype=torch.bool))
        with pytest.raises(ValueError, match=fn + ": keep has to be"):
            call(torch.zeros(4), keep=torch.ones(5))  # keep before the threshold
    # (the width, and a device threshold of the wrong type or shape: tests/test_gpu_range.py::test_refusals_that_need_a_device)
