"""Host side of the duplicate clusters (include/coot_hip.h: coot_retrieval_components; GalleryIndex.components, deduplicate,
retrieval_components_device, compute_retrieval_components): the function declared, bound, listed and exported by both builds under the
unchanged ABI version; the mirror on hand-made similarity matrices; and the wrappers refusing on the host what they cannot serve.  The
device results are compared in tests/test_gpu_components.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_components": 11}


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


def test_components_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        assert _params(hdr, name).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    comp, count = _params(hdr, "coot_retrieval_components"), _params(hdr, "coot_retrieval_join_count")
    # the count call's operands and filters, then the whole gallery (no row0 / rows, no table), the workspace, the result, the stream
    head = count[:count.index("int row0")]
    assert comp.startswith(head) and head.endswith("const int32_t* groups, const float* thresholds, ")
    assert comp[len(head):] == "int N, int d, int32_t* parent, int32_t* labels, coot_stream_t stream"
    assert list(lib.coot_retrieval_components.argtypes[:6]) == list(lib.coot_retrieval_join_count.argtypes[:6])
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # a new function only: the ABI version stays
    csrc = os.path.join(ROOT, "coot-videotext_amd", "csrc")
    vs = open(os.path.join(csrc, "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert re.search(r"\b" + name + r"\b", vs), name
    build = open(os.path.join(csrc, "build.sh")).read()
    assert "retrieval_components" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(csrc, "retrieval_components.hip"))
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in stub, name
    assert "rt_comp_blocks_per_wg" in stub
    declared = set(re.findall(r"\b(coot_[a-z0-9_]+)\s*\(", hdr)) - {"coot_stream_t"}
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert exported == declared, (so, sorted(exported ^ declared)[:5])  # exactly the header's names
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_the_schedule_option_is_set_and_read_back(cva):
    lib = cva.lib.load()
    got = ctypes.c_int(-1)
    assert lib.coot_get_option(b"rt_comp_blocks_per_wg", ctypes.byref(got)) == 0 and got.value == 0  # automatic
    try:
        assert lib.coot_set_option(b"rt_comp_blocks_per_wg", 3) == 0
        assert lib.coot_get_option(b"rt_comp_blocks_per_wg", ctypes.byref(got)) == 0 and got.value == 3
    finally:
        assert lib.coot_set_option(b"rt_comp_blocks_per_wg", 0) == 0
    assert cva.lib.get_option("rt_comp_blocks_per_wg") == 0


def test_the_names_are_exported_by_the_package(cva):
    for name in ("retrieval_components_device", "compute_retrieval_components"):
        assert getattr(cva, name) is getattr(cva.retrieval, name), name
    assert cva.retrieval.compute_retrieval_components is cva.retrieval_mirror.compute_retrieval_components
    assert callable(cva.GalleryIndex.components) and callable(cva.GalleryIndex.deduplicate)
    assert "through a row of another group" in cva.GalleryIndex.components.__doc__
    assert cva.retrieval.COMPONENTS_ROWS_MAX == 65535 * 64


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

def _chain(n, score=0.9):
    """Row i scores `score` with rows i - 1 and i + 1, 1 with itself and 0 with every other row."""
    s = np.eye(n, dtype=np.float32)
    for i in range(n - 1):
        s[i, i + 1] = s[i + 1, i] = score
    return s


def test_mirror_labels_a_chain_with_its_smallest_row(cva):
    f = cva.compute_retrieval_components
    lab = f(_chain(6), 0.5)
    assert lab.dtype == np.int32 and lab.shape == (6,) and lab.tolist() == [0] * 6
    assert f(_chain(6), 0.95).tolist() == [0, 1, 2, 3, 4, 5]  # a row without an edge labels itself (the diagonal is no edge)
    assert f(_chain(6), 0.9).tolist() == [0] * 6  # on the threshold: an edge
    s = _chain(6)
    s[2, 3] = s[3, 2] = 0.0
    assert f(s, 0.5).tolist() == [0, 0, 0, 3, 3, 3]
    # the label does not depend on the order in which the edges arrive: the chain under a permutation of its rows
    perm = np.array([4, 0, 5, 2, 1, 3])
    assert f(_chain(6)[np.ix_(perm, perm)], 0.5).tolist() == [0] * 6
    s = s[np.ix_(perm, perm)]  # chain position perm[r] sits in row r: {0, 1, 2} are rows 1, 4, 3 and {3, 4, 5} rows 5, 0, 2
    assert f(s, 0.5).tolist() == [0, 1, 0, 1, 1, 0]
    # the lower triangle is never read
    low = _chain(6)
    low[np.tril_indices(6)] = 7.0
    assert f(low, 0.5).tolist() == [0] * 6
    assert f(np.ones((1, 1), np.float32), 0.0).tolist() == [0]


def test_mirror_a_masked_row_is_no_vertex(cva):
    f = cva.compute_retrieval_components
    keep = np.array([1, 1, 0, 1, 1], np.uint8)
    assert f(_chain(5), 0.5, keep=keep).tolist() == [0, 0, -1, 3, 3]  # the chain is cut: the masked row does not connect its neighbours
    assert f(_chain(5), 0.5, keep=keep.astype(bool)).tolist() == [0, 0, -1, 3, 3] and f(_chain(5), 0.5, keep=keep * 5).tolist() == [0, 0, -1, 3, 3]
    assert f(_chain(5), 0.5, keep=np.zeros(5, bool)).tolist() == [-1] * 5
    assert f(_chain(5), 0.95, keep=keep).tolist() == [0, 1, -1, 3, 4]


def test_mirror_rows_of_one_group_meet_through_a_third_row(cva):
    f = cva.compute_retrieval_components
    s = np.ones((3, 3), np.float32)
    assert f(s, 0.5, groups=np.array([7, 7, 7])).tolist() == [0, 1, 2]  # one group: no edge at all
    assert f(s, 0.5, groups=np.array([7, 7, -2])).tolist() == [0, 0, 0]  # (0, 1) is no edge; (0, 2) and (1, 2) are
    s[0, 2] = s[2, 0] = 0.0
    assert f(s, 0.5, groups=np.array([7, 7, -2], np.int32)).tolist() == [0, 1, 1]
    assert f(s, 0.5).tolist() == [0, 0, 0]
    with pytest.raises(AssertionError):
        f(s, 0.5, groups=np.zeros(3))  # floats are no ids


def test_mirror_thresholds_per_row_and_special_values(cva):
    f = cva.compute_retrieval_components
    # the threshold of the SMALLER row decides: a NaN there is no edge, whatever the larger row's threshold is
    assert f(_chain(4), [np.nan, 0.5, 0.5, 0.5]).tolist() == [0, 1, 1, 1]
    assert f(_chain(4), [0.5, 0.5, 0.5, np.nan]).tolist() == [0, 0, 0, 0]  # the last row never asks
    assert f(_chain(4), np.nan).tolist() == [0, 1, 2, 3]
    assert f(_chain(4), [0.5, np.inf, 0.5, 0.5]).tolist() == [0, 0, 2, 2]
    # -inf: one component of all kept rows
    rs = np.random.RandomState(4)
    sim = rs.randn(9, 9).astype(np.float32)
    assert f(sim, -np.inf).tolist() == [0] * 9
    keep = np.array([0, 1, 1, 0, 1, 1, 1, 0, 1], bool)
    assert f(sim, -np.inf, keep=keep).tolist() == [-1, 1, 1, -1, 1, 1, 1, -1, 1]
    assert f(sim, np.float64(-np.inf), keep=keep).tolist() == f(sim, [-np.inf] * 9, keep=keep).tolist()
    s = np.zeros((3, 3), np.float32)
    s[0, 1], s[0, 2], s[1, 2] = np.nan, -0.0, np.nan
    assert f(s, 0.0).tolist() == [0, 1, 0] and f(s, -np.inf).tolist() == [0, 1, 0]  # -0 >= +0 holds; a NaN score is no edge
    with pytest.raises(AssertionError):
        f(np.zeros((3, 4), np.float32), 0.0)
    with pytest.raises(AssertionError):
        f(_chain(4), np.zeros(3))
    with pytest.raises(AssertionError):
        f(_chain(4), 0.0, keep=np.ones(3))


def test_mirror_is_a_union_find_over_the_self_join_mirror(cva):
    rs = np.random.RandomState(2)
    n = 41
    a = rs.randn(n, n).astype(np.float32)
    sim = a + a.T
    thr = (1.5 + rs.rand(n)).astype(np.float32)
    groups = rs.randint(0, 5, n)
    for keep in (None, rs.rand(n) < 0.7):
        for gr in (None, groups):
            off, rows, _ = cva.compute_retrieval_self_join(sim, thr, keep=keep, groups=gr)
            lab = np.arange(n)
            for _ in range(n):  # label propagation to the fixed point: the definition, without a forest
                for i in range(n):
                    for j in rows[off[i]:off[i + 1]]:
                        lab[i] = lab[j] = min(lab[i], lab[j])
            if keep is not None:
                lab[~keep] = -1
            got = cva.compute_retrieval_components(sim, thr, keep=keep, groups=gr)
            assert got.tolist() == lab.tolist()
            assert 1 < len(set(got.tolist())) < n  # neither trivial


# ---- refusals on the host ------------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_on_the_host(cva):
    """CPU tensors: the checks and their order are those of the self-join, under the calling function's name."""
    import torch
    from coot_videotext_amd import GalleryIndex, retrieval_components_device
    n = 5
    g = torch.zeros(n, 8)

    def made(gallery):  # an index cannot be built without a device: an instance made by hand
        index = object.__new__(GalleryIndex)
        index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = gallery, None, False, None, 0, torch.float32
        return index

    index = made(g)
    calls = {"retrieval_components_device": lambda thr=0.5, **kw: retrieval_components_device(g, None, thr, **kw),
             "GalleryIndex.components": lambda thr=0.5, **kw: index.components(thr, **kw),
             "GalleryIndex.deduplicate": lambda thr=0.5, **kw: index.deduplicate(thr, **kw)}
    for fn, call in calls.items():
        with pytest.raises(TypeError):
            call(max_results=7)  # there is no pair list to size
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
                with pytest.raises(RuntimeError, match=fn + r" needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_components\)"):
                    call(thr, **kw)
    assert index.keep is None  # a refused deduplicate leaves the filter alone
    # too many rows for the one launch (a view of one row: no memory behind it)
    big = torch.zeros(1, 8).expand(65535 * 64 + 1, 8)
    wide = made(big)
    for fn, call in (("retrieval_components_device", lambda: retrieval_components_device(big, None, 0.5)),
                     ("GalleryIndex.components", lambda: wide.components(0.5)), ("GalleryIndex.deduplicate", lambda: wide.deduplicate(0.5))):
        with pytest.raises(ValueError, match=fn + r": a gallery of 4194241 rows; one launch covers all rows, at most 4194240 \(ceil\(N / 64\) <= 65535\)"):
            call()
    most = made(torch.zeros(1, 8).expand(65535 * 64, 8))
    with pytest.raises(RuntimeError, match=r"GalleryIndex.components needs CUDA tensors"):
        most.components(0.5)  # the largest gallery passes this check
