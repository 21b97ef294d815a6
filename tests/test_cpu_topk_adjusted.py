"""Host side of the adjusted top-K search and the hubness offsets (include/coot_hip.h: coot_retrieval_topk_adjusted,
coot_retrieval_topk_adjusted_workspace_bytes, coot_retrieval_hub_offsets; retrieval.compute_retrieval_topk_adjusted,
compute_retrieval_hub_offsets, retrieval_topk_adjusted_device, GalleryIndex.search_adjusted, GalleryIndex.hubness_offsets): the numpy
mirrors against an independent brute force; the planted hub on the mirrors alone; the new functions declared, bound and exported by
both builds under the unchanged ABI version; the workspace size; and the wrappers refusing on the host what they cannot serve.  Every
comparison of results is for byte equality.  The device results are compared with the mirrors in tests/test_gpu_topk_adjusted.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_adjusted": 16, "coot_retrieval_topk_adjusted_workspace_bytes": 4, "coot_retrieval_hub_offsets": 6}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _brute(sim, offset, k, keep=None):
    """Per row: the kept columns ranked with the tie rule of the device ranks (_ahead: a higher score, or an equal one at a later
    column), on a = sim - offset in float32.  Plain Python loops, nothing shared with the mirror."""
    from coot_videotext_amd.retrieval_mirror import _ahead
    m, n = sim.shape
    idx, sc = np.full((m, k), -1, np.int32), np.full((m, k), -np.inf, np.float32)
    for i in range(m):
        a = [np.float32(np.float32(sim[i, j]) - np.float32(offset[j])) for j in range(n)]
        cols = [j for j in range(n) if keep is None or keep[j]]
        for j in cols:
            r = sum(1 for t in cols if t != j and bool(_ahead(a[t], t, a[j], j)))
            if r < k:
                idx[i, r], sc[i, r] = j, a[j]
    return idx, sc


def test_ahead_is_the_tie_rule():
    from coot_videotext_amd.retrieval_mirror import _ahead
    assert bool(_ahead(np.float32(1), 0, np.float32(0), 5)) and not bool(_ahead(np.float32(0), 5, np.float32(1), 0))
    assert bool(_ahead(np.float32(0), 5, np.float32(-0.0), 2)) and not bool(_ahead(np.float32(0), 2, np.float32(0), 5))


@pytest.mark.parametrize("n,k", [(37, 5), (130, 128), (64, 9)])
def test_adjusted_mirror_against_brute_force(cva, n, k):
    """Random similarities and offsets; small integers (with -0 among them) so that adjusted scores tie; +inf and -inf offsets; with
    and without keep, as booleans and as bytes."""
    from coot_videotext_amd import compute_retrieval_topk, compute_retrieval_topk_adjusted, compute_retrieval_topk_masked
    rs = np.random.RandomState(n + k)
    m = 7
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n)).astype(np.float32)
        off = (rs.randint(-1, 2, size=n) if exact_ties else 0.1 * rs.randn(n)).astype(np.float32)
        if exact_ties:
            sim[sim == 0] *= rs.choice([-1.0, 1.0], size=int((sim == 0).sum())).astype(np.float32)  # -0 and +0 tie
        special = off.copy()
        special[[0, n // 2, n - 1]] = np.inf
        special[3] = -np.inf
        keep = rs.rand(n) < 0.6
        for o in (off, special, np.zeros(n, np.float32), off.astype(np.float64).tolist()):
            o32 = np.asarray(o).astype(np.float32)
            for kp in (None, keep, keep.astype(np.uint8) * 5, np.zeros(n, bool)):
                got = compute_retrieval_topk_adjusted(sim, o, k, keep=kp)
                want = _brute(sim, o32, k, kp)
                assert got[0].dtype == np.int32 and got[1].dtype == np.float32
                assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1]), exact_ties
        for kp in (None, keep):
            plain = compute_retrieval_topk(sim, k) if kp is None else compute_retrieval_topk_masked(sim, k, kp)
            got = compute_retrieval_topk_adjusted(sim, np.zeros(n), k, keep=kp)  # offset 0: the search itself
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        got = compute_retrieval_topk_adjusted(sim, special, n)  # +inf: still a column, last, the later column first; -inf: first
        assert (got[0][:, 0] == 3).all() and (got[0][:, -3:] == [n - 1, n // 2, 0]).all() and np.isneginf(got[1][:, -3:]).all()


def test_hub_offsets_mirror_against_brute_force(cva):
    """The sequential float32 sum of the filled slots, which differs from the pairwise np.sum on long lists; unfilled tails; a row
    without a filled slot is 0."""
    from coot_videotext_amd import compute_retrieval_hub_offsets
    rs = np.random.RandomState(0)
    n, k = 50, 128
    sc = np.sort(rs.randn(n, k).astype(np.float32) * 3, axis=1)[:, ::-1].copy()
    idx = rs.randint(0, 1000, size=(n, k)).astype(np.int32)
    filled = rs.randint(0, k + 1, size=n)
    filled[0], filled[1], filled[2] = 0, k, 1
    for j in range(n):
        idx[j, filled[j]:], sc[j, filled[j]:] = -1, -np.inf
    got = compute_retrieval_hub_offsets(sc, idx)
    want = np.zeros(n, np.float32)
    for j in range(n):
        acc, c = np.float32(0), 0
        for t in range(k):
            if idx[j, t] >= 0:
                acc, c = np.float32(acc + sc[j, t]), c + 1
        if c:
            want[j] = np.float32(np.float32(0.5) * np.float32(acc / np.float32(c)))
    assert got.dtype == np.float32 and _bytes_equal(got, want)
    assert got[0] == 0 and got[2] == np.float32(0.5) * sc[2, 0]
    pairwise = np.float32(0.5) * (sc[1].sum(dtype=np.float32) / np.float32(k))
    assert np.isclose(got[1], pairwise, rtol=1e-4, atol=1e-6)
    with pytest.raises(AssertionError):
        compute_retrieval_hub_offsets(sc.astype(np.float64), idx)
    with pytest.raises(AssertionError):
        compute_retrieval_hub_offsets(sc, idx[:, :5])


def _planted_hub(seed, n, d, m):
    def unit(x):
        return x / np.sqrt((x * x).sum(-1, keepdims=True))
    rs = np.random.RandomState(seed)
    x, c = rs.randn(n, d), rs.randn(1, d)
    g = unit(x)
    g[n - 1] = unit(c)
    lab = rs.permutation(n - 1)[:m]
    q = unit(g[lab] + 0.9 * unit(rs.randn(m, d)) + 0.9 * unit(c))
    bank = unit(g[rs.permutation(n - 1)[:m]] + 0.9 * unit(rs.randn(m, d)) + 0.9 * unit(c))
    return g.astype(np.float32), q.astype(np.float32), bank.astype(np.float32), lab


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_hub_on_the_mirrors(cva, seed):
    """Row n - 1 is the direction every query leans towards: raw top-1 returns it for a quarter of the queries.  The offsets of
    compute_retrieval_knn_join -> compute_retrieval_hub_offsets against a bank of like queries take it out."""
    from coot_videotext_amd import (compute_retrieval_hub_offsets, compute_retrieval_knn_join, compute_retrieval_topk,
                                    compute_retrieval_topk_adjusted)
    n, d, m, k = 300, 32, 200, 10
    g, q, bank, lab = _planted_hub(seed, n, d, m)
    sim = (q @ g.T).astype(np.float32)
    idx, sc = compute_retrieval_knn_join((g @ bank.T).astype(np.float32), k)
    off = compute_retrieval_hub_offsets(sc, idx)
    raw = compute_retrieval_topk(sim, 1)[0][:, 0]
    cor = compute_retrieval_topk_adjusted(sim, off, 1)[0][:, 0]
    hub_raw, hub_cor = int((raw == n - 1).sum()), int((cor == n - 1).sum())
    assert hub_raw > 0 and 5 * hub_cor <= hub_raw, (hub_raw, hub_cor)
    assert (cor == lab).mean() >= (raw == lab).mean() + 0.1


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_adjusted_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    args = re.search(r"\bcoot_retrieval_topk_adjusted\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    for part in ("const void* gallery", "int gallery_dtype", "const uint8_t* keep", "const float* offset", "int32_t* idx_out", "float* score_out",
                 "float* sim_out"):
        assert part in args, part
    assert lib.coot_retrieval_topk_adjusted_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    srcs = re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert "retrieval_adjusted" in srcs and "retrieval_few" in srcs and "retrieval_knn" in srcs
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_adjusted.hip"))
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
    """No device needed.  The few-query search's layout; the size does not depend on the split option; each argument out of range
    gives 256."""
    lib = cva.lib.load()
    f = lib.coot_retrieval_topk_adjusted_workspace_bytes
    assert f(16, 1000, 64, 128) - f(16, 1000, 64, 10) >= 8 * 16 * 8 * 118  # 8 blocks of 128 rows: 8 lists per query at the most
    assert f(16, 1000, 64, 10) > f(1, 1000, 64, 10)
    assert f(1, 1, 1, 1) > 256
    for args in ((5, 1000, 64, 10), (16, 200000, 768, 128), (1, 5, 37, 5)):
        assert f(*args) == lib.coot_retrieval_topk_few_workspace_bytes(*args), args
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
    for name in ("compute_retrieval_topk_adjusted", "compute_retrieval_hub_offsets", "retrieval_topk_adjusted_device"):
        assert callable(getattr(cva, name)), name
        assert getattr(cva.retrieval, name) is getattr(cva, name)
    assert cva.compute_retrieval_topk_adjusted is cva.retrieval_mirror.compute_retrieval_topk_adjusted
    assert callable(cva.GalleryIndex.search_adjusted) and callable(cva.GalleryIndex.hubness_offsets)


def _hand_made_index(torch, GalleryIndex, g, normalize=False):
    index = object.__new__(GalleryIndex)  # an index cannot be built without a device: an instance made by hand
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = g, None, normalize, None, 0, torch.float32
    return index


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  keep first, then the offset's type and shape (ValueError), then the
    devices ("no CPU fallback", naming the mirror of this search).  k and the width come after the device:
    tests/test_gpu_topk_adjusted.py::test_arguments_are_refused_on_the_host."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_topk_adjusted_device
    q, g = torch.zeros(3, 8), torch.zeros(5, 8)
    index = _hand_made_index(torch, GalleryIndex, g)
    good = [0.0] * 5
    calls = {"retrieval_topk_adjusted_device": lambda offset=good, k=2, **kw: retrieval_topk_adjusted_device(q, g, None, offset, k, **kw),
             "GalleryIndex.search_adjusted": lambda offset=good, k=2, **kw: index.search_adjusted(q, k, offset, **kw)}
    for fn, call in calls.items():
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8"):
            call(keep=torch.ones(5))
        with pytest.raises(ValueError, match=fn + ": keep has to be a torch.bool or torch.uint8"):
            call("abc", keep=torch.ones(5))  # (before the offset is looked at)
        with pytest.raises(ValueError, match="one flag per row"):
            call(keep=torch.ones(4, dtype=torch.bool))
        for offset in ([0.0] * 4, [[0.0] * 5], np.zeros(6, np.float32), torch.zeros(5, 1), 0.5, np.float32(1), []):
            with pytest.raises(ValueError, match=fn + r": offset of shape .*, a gallery of 5 rows \(one number per row: \[5\]\)"):
                call(offset)
        for offset in (["a"] * 5, "abcde", None, np.zeros(5, bool), torch.zeros(5, dtype=torch.bool), np.zeros(5, np.complex64), [None] * 5,
                       torch.zeros(5, dtype=torch.bfloat16)):
            with pytest.raises(ValueError, match=fn + ": offset has to hold one number per gallery row, not dtype"):
                call(offset)
        for offset in (good, tuple(good), np.zeros(5), np.arange(5), np.zeros(5, np.float16), torch.zeros(5), torch.zeros(5, dtype=torch.float64),
                       torch.arange(5), [0, np.inf, -np.inf, 1e300, 1]):
            for kw in (dict(), dict(keep=torch.ones(5, dtype=torch.bool)), dict(k=0), dict(want_sim=True)):
                with pytest.raises(RuntimeError, match=fn + " needs CUDA tensors .*no CPU fallback; use compute_retrieval_topk_adjusted"):
                    call(offset, **kw)


def test_hubness_offsets_refuses_on_the_host(cva):
    """knn_join's checks under the new method's name, without a device."""
    import torch
    from coot_videotext_amd import GalleryIndex
    who = "GalleryIndex.hubness_offsets"
    index = _hand_made_index(torch, GalleryIndex, torch.zeros(5, 8))
    bank = _hand_made_index(torch, GalleryIndex, torch.zeros(12, 8))
    with pytest.raises(TypeError, match=who + ": the right side has to be a GalleryIndex, not Tensor"):
        index.hubness_offsets(torch.zeros(12, 8))
    with pytest.raises(ValueError, match=who + ": this index holds rows of width 8, the right one of width 7"):
        index.hubness_offsets(_hand_made_index(torch, GalleryIndex, torch.zeros(12, 7)))
    with pytest.raises(ValueError, match=who + ": this index has normalize=False, the right one normalize=True"):
        index.hubness_offsets(_hand_made_index(torch, GalleryIndex, torch.zeros(12, 8), normalize=True))
    with pytest.raises(ValueError, match=who + ": keep has to be a torch.bool or torch.uint8"):
        index.hubness_offsets(bank, keep=torch.ones(5))
    with pytest.raises(ValueError, match="one flag per row"):
        index.hubness_offsets(bank, other_keep=torch.ones(5, dtype=torch.bool))  # (the bank has 12 rows)
    for k in (0, 13, 129):
        with pytest.raises(ValueError, match=who + rf": k = {k} is outside 1 .. min\(N_right = 12, 128\)"):
            index.hubness_offsets(bank, k)
    with pytest.raises(ValueError, match=who + r": k = 10 is outside 1 .. min\(N_right = 9, 128\)"):
        index.hubness_offsets(_hand_made_index(torch, GalleryIndex, torch.zeros(9, 8)))  # the default k = 10
    for kw in (dict(), dict(k=1), dict(keep=torch.ones(5, dtype=torch.bool), other_keep=torch.ones(12, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match=who + " needs CUDA tensors .*no CPU fallback; use compute_retrieval_knn_join"):
            index.hubness_offsets(bank, **kw)
