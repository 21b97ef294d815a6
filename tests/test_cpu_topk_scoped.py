"""Host side of the scoped top-K search (include/coot_hip.h: coot_retrieval_topk_scoped, coot_retrieval_topk_scoped_workspace_bytes;
retrieval.compute_retrieval_topk_scoped, retrieval_topk_scoped_device, GalleryIndex.search_scoped, GalleryIndex.neighbors): the numpy
mirror against an independent brute force; the two new functions declared, bound and exported by both builds under the unchanged ABI
version; the workspace size; and the wrappers refusing on the host what they cannot serve.  Every comparison of results is for byte
equality.  The device results are compared with the mirror in tests/test_gpu_topk_scoped.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_scoped": 18, "coot_retrieval_topk_scoped_workspace_bytes": 4}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _brute(sim, k, groups, scope, exclude, keep=None):
    """Per row: the eligible columns sorted by (score with -0 as +0, column), both descending.  Plain Python, nothing shared with the
    mirror."""
    m, n = sim.shape
    idx, sc = np.full((m, k), -1, np.int32), np.full((m, k), -np.inf, np.float32)
    for i in range(m):
        ranked = []
        for j in range(n):
            g = j if groups is None else int(groups[j])
            if (keep is None or keep[j]) and ((g == int(scope[i])) != exclude):
                ranked.append((float(sim[i, j]) + 0.0, j))
        for r, (_, j) in enumerate(sorted(ranked, reverse=True)[:k]):
            idx[i, r], sc[i, r] = j, sim[i, j]
    return idx, sc


@pytest.mark.parametrize("n,k", [(37, 5), (130, 128), (64, 9)])
def test_mirror_against_brute_force(cva, n, k):
    """Random similarities, and small integers (with -0 among them) so that columns tie; ids that no column has (under only: a whole row
    unfilled), groups smaller than k (the tail -1 / -inf), groups=None, both modes, with and without keep."""
    from coot_videotext_amd import compute_retrieval_topk_scoped
    rs = np.random.RandomState(n + k)
    m = 11
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n) * 100).astype(np.float32)
        if exact_ties:
            sim[sim == 0] *= rs.choice([-1.0, 1.0], size=int((sim == 0).sum())).astype(np.float32)  # -0 and +0 tie
        runs = np.repeat(np.arange(n), 7)[:n] * 3 - 5  # ids -5, -2, 1, ...: any int32 value, seven adjacent columns each
        keep = rs.rand(n) < 0.6
        for groups in (runs, runs[rs.permutation(n)].astype(np.int32), np.zeros(n, np.int64), None):
            ids = np.arange(n) if groups is None else np.unique(groups)
            scope = rs.choice(ids, size=m)
            scope[0], scope[1], scope[2] = 2 ** 31 - 1, -2 ** 31, int(ids.max()) + 1  # ids that no column carries
            for kp in (None, keep, keep.astype(np.uint8) * 5):
                for exclude in (False, True):
                    kw = dict(exclude=scope) if exclude else dict(only=scope.tolist())
                    got = compute_retrieval_topk_scoped(sim, k, groups, keep=kp, **kw)
                    want = _brute(sim, k, groups, scope, exclude, kp)
                    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
                    assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1]), (exact_ties, exclude)
                    if not exclude:
                        assert (got[0][:3] == -1).all() and np.isneginf(got[1][:3]).all()
                        if groups is not None and k > 7 and groups.max() > 0:
                            assert (got[0][3:, 7:] == -1).all()  # a group has seven columns at the most
                    elif kp is None and groups is not None:  # an absent id excludes nothing
                        from coot_videotext_amd import compute_retrieval_topk
                        plain = compute_retrieval_topk(sim[:3] + np.float32(0), k)
                        assert np.array_equal(got[0][:3], plain[0])


def test_mirror_refuses_bad_arguments(cva):
    from coot_videotext_amd import compute_retrieval_topk_scoped
    sim = np.zeros((3, 8), np.float32)
    g = np.arange(8)
    for kw in (dict(), dict(only=[0, 1, 2], exclude=[0, 1, 2]), dict(only=[0, 1]), dict(exclude=[0, 1, 2, 3]), dict(only=[0, 1, 2], keep=np.ones(7, bool)),
               dict(only=[0, 1, 2], k=9), dict(only=[0, 1, 2], k=0), dict(only=[0, 1, 2], groups=g[:7])):
        kw = dict(dict(k=2, groups=g), **kw)
        with pytest.raises(AssertionError):
            compute_retrieval_topk_scoped(sim, kw.pop("k"), kw.pop("groups"), **kw)


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_scoped_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    args = re.search(r"\bcoot_retrieval_topk_scoped\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    for part in ("const void* gallery", "int gallery_dtype", "const uint8_t* keep", "const int32_t* groups", "const int32_t* scope", "int exclude",
                 "int32_t* idx_out", "float* score_out", "float* sim_out"):
        assert part in args, part
    assert lib.coot_retrieval_topk_scoped_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    srcs = re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert "retrieval_scoped" in srcs and "retrieval_few" in srcs
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_scoped.hip"))
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
    """No device needed.  Lists of K entries per query and split; the size does not depend on the split option; each argument out of
    range gives 256."""
    lib = cva.lib.load()
    f = lib.coot_retrieval_topk_scoped_workspace_bytes
    assert f(16, 1000, 64, 128) - f(16, 1000, 64, 10) >= 8 * 16 * 8 * 118  # 8 blocks of 128 rows: 8 lists per query at the most
    assert f(16, 1000, 64, 10) > f(1, 1000, 64, 10)
    assert f(4, 1000, 640, 10) - f(4, 1000, 64, 10) >= 4 * 16 * 576  # the operand table
    assert f(1, 1, 1, 1) > 256
    assert f(5, 1000, 64, 10) == lib.coot_retrieval_topk_few_workspace_bytes(5, 1000, 64, 10)  # the few-query search's layout
    for args in ((0, 1000, 64, 10), (17, 1000, 64, 10), (-1, 1000, 64, 10), (4, 0, 64, 10), (4, 1000, 0, 10), (4, 1000, 64, 0), (4, 1000, 64, 129),
                 (4, 5, 64, 6), (4, 1000, 64, -2)):
        assert f(*args) == 256, args
    try:
        base = f(5, 1000, 64, 10)
        for s in (1, 3, 1000):
            assert lib.coot_set_option(b"rt_few_splits", s) == 0
            assert f(5, 1000, 64, 10) == base, s
    finally:
        assert lib.coot_set_option(b"rt_few_splits", 0) == 0


def test_package_exports(cva):
    for name in ("compute_retrieval_topk_scoped", "retrieval_topk_scoped_device"):
        assert callable(getattr(cva, name)), name
    assert callable(cva.GalleryIndex.search_scoped) and callable(cva.GalleryIndex.neighbors)


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  only / exclude first, then the types and shapes of groups, keep and the
    scope (ValueError), then the devices ("no CPU fallback", naming the mirror of this search)."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_topk_scoped_device
    q, g = torch.zeros(3, 8), torch.zeros(5, 8)
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, False, None, 0, torch.float32
    good = torch.zeros(5, dtype=torch.int32)
    calls = {"retrieval_topk_scoped_device": lambda groups=good, k=2, **kw: retrieval_topk_scoped_device(q, g, None, groups, k, **kw),
             "GalleryIndex.search_scoped": lambda groups=good, k=2, **kw: index.search_scoped(q, k, groups, **kw)}
    for fn, call in calls.items():
        with pytest.raises(ValueError, match=fn + ": exactly one of only= and exclude= has to be given, not neither"):
            call()
        with pytest.raises(ValueError, match=fn + ": exactly one of only= and exclude= has to be given, not both"):
            call(only=[0, 1, 2], exclude=[0, 1, 2])
        with pytest.raises(ValueError, match=fn + ": exactly one of only= and exclude= has to be given, not neither"):
            call(groups=torch.zeros(4))  # (before groups is looked at)
        for name in ("only", "exclude"):
            for scope in ([0, 1], [[0, 1, 2]], np.zeros(4, np.int64), torch.zeros(2, dtype=torch.int32), 3):
                with pytest.raises(ValueError, match=fn + ": " + name + r" of shape .*, 3 queries \(one id per query: \[3\]\)"):
                    call(**{name: scope})
            for scope in ([0.0, 1.0, 2.0], np.zeros(3, np.float32), torch.zeros(3), torch.zeros(3, dtype=torch.bool), ["a", "b", "c"], "abc", []):
                with pytest.raises(ValueError, match=fn + ": " + name + " has to hold integers"):
                    call(**{name: scope})
            with pytest.raises(ValueError, match=fn + ": " + name + " holds an id outside int32"):
                call(**{name: [0, 2 ** 31, 1]})
            for scope in ([0, 1, 2], (0, -1, 2 ** 31 - 1), np.array([0, 1, 2], np.int32), np.array([0, 1, 2], np.uint8), torch.tensor([0, 1, 2]),
                          torch.tensor([0, 1, 2], dtype=torch.int32)):
                for groups in (good, torch.zeros(5, dtype=torch.int64), None):
                    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_scoped"):
                        call(groups, **{name: scope})
                with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_scoped"):
                    call(keep=torch.ones(5, dtype=torch.bool), **{name: scope})
        for groups in (torch.zeros(5), torch.zeros(5, dtype=torch.int16), [0, 0, 0, 0, 0], np.zeros(5, np.int32)):
            with pytest.raises(ValueError, match=fn + ": groups has to be a torch.int32 or torch.int64"):
                call(groups, only=[0, 1, 2])
        for groups in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.int32)):
            with pytest.raises(ValueError, match="one group id per row"):
                call(groups, exclude=[0, 1, 2])
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8"):
            call(only=[0, 1, 2], keep=torch.ones(5))
        with pytest.raises(ValueError, match="one flag per row"):
            call(only=[0, 1, 2], keep=torch.ones(4, dtype=torch.bool))
    # neighbors: the row numbers are checked like remove()'s, groups like search_scoped's, then the device
    for rows, exc, text in (([5], IndexError, r"GalleryIndex.neighbors: row 5 is outside \[0, 5\)"), ([-1], IndexError, "row -1 is outside"),
                            ([0.5], TypeError, "GalleryIndex.neighbors: rows of dtype float64; row numbers are integers"),
                            (torch.tensor([0, 7]), IndexError, "row 7 is outside")):
        with pytest.raises(exc, match=text):
            index.neighbors(rows, 2)
    with pytest.raises(ValueError, match="GalleryIndex.neighbors: groups has to be a torch.int32 or torch.int64"):
        index.neighbors([0, 1], 2, groups=[0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="one group id per row"):
        index.neighbors([0, 1], 2, groups=torch.zeros(4, dtype=torch.int32))
    for groups in (None, good):
        with pytest.raises(RuntimeError, match="GalleryIndex.neighbors needs CUDA tensors .*use compute_retrieval_topk_scoped"):
            index.neighbors([0, 1], 2, groups=groups)
    # (k and the width are checked after the device: tests/test_gpu_topk_scoped.py::test_k_and_width_are_refused_on_the_host)
