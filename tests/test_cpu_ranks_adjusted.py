"""Host side of the labelled ranking under offsets (include/coot_hip.h: coot_retrieval_ranks_adjusted,
coot_retrieval_ranks_adjusted_workspace_bytes; retrieval.compute_retrieval_labeled_adjusted, retrieval_ranks_adjusted_device,
compute_retrieval_adjusted_device, compute_retrieval_csls_device): the numpy mirror against an independent brute force; without
offsets and with zeros the bytes of compute_retrieval_labeled; with a column offset alone the position of the label in
compute_retrieval_topk_adjusted; the planted hub on the mirrors alone; the new functions declared, bound and exported by both builds;
the workspace size; and the wrappers refusing on the host what they cannot serve.  Every comparison of results is for byte equality.
The device results are compared with the mirror in tests/test_gpu_ranks_adjusted.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_ranks_adjusted": 17, "coot_retrieval_ranks_adjusted_workspace_bytes": 3}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _brute(sim, labels, col, row):
    """Ranks in plain loops on explicitly rounded float32, with the tie rule _ahead and nothing else shared with the mirror."""
    from coot_videotext_amd.retrieval_mirror import _ahead
    m, n = sim.shape
    a = [[np.float32(sim[i, j]) for j in range(n)] for i in range(m)]
    with np.errstate(invalid="ignore", over="ignore"):
        if col is not None:
            a = [[np.float32(a[i][j] - np.float32(col[j])) for j in range(n)] for i in range(m)]
        if row is not None:
            a = [[np.float32(a[i][j] - np.float32(row[i])) for j in range(n)] for i in range(m)]
    rq, rg = np.full(m, -1, np.int32), np.full(n, -1, np.int32)
    for i in range(m):
        g = int(labels[i])
        if 0 <= g < n:
            rq[i] = sum(1 for j in range(n) if j != g and bool(_ahead(a[i][j], j, a[i][g], g)))
    for j in range(n):
        pos = [i for i in range(m) if int(labels[i]) == j]
        if pos:  # the best-ranked ground truth: the smallest position among the column's positives
            rg[j] = min(sum(1 for t in range(m) if t != i and bool(_ahead(a[t][j], t, a[i][j], i))) for i in pos)
    return rq, rg


def _labels(rs, m, n):
    lab = rs.randint(0, n, size=m)
    lab[rs.rand(m) < 0.3] = rs.randint(0, max(1, n // 3))  # several queries per column, columns without one
    if m > 2:
        lab[1], lab[2] = -1, n
    return lab.astype(np.int32)


@pytest.mark.parametrize("m,n", [(9, 13), (20, 7), (1, 5), (6, 6)])
def test_mirror_against_brute_force(cva, m, n):
    """Random similarities and offsets; integers (with -0 among them) so that adjusted scores tie; +inf and -inf offsets, a labelled
    column at +inf among them."""
    from coot_videotext_amd import compute_retrieval_labeled_adjusted
    from coot_videotext_amd.retrieval_mirror import _labeled_metrics
    rs = np.random.RandomState(10 * m + n)
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n)).astype(np.float32)
        col = (rs.randint(-1, 2, size=n) if exact_ties else 0.1 * rs.randn(n)).astype(np.float32)
        row = (rs.randint(-1, 2, size=m) if exact_ties else 0.1 * rs.randn(m)).astype(np.float32)
        if exact_ties:
            sim[sim == 0] *= rs.choice([-1.0, 1.0], size=int((sim == 0).sum())).astype(np.float32)  # -0 and +0 tie
        lab = _labels(rs, m, n)
        special = col.copy()
        special[[0, n - 1]] = np.inf
        special[n // 2] = -np.inf
        lab[0] = n - 1  # a labelled column at +inf
        for c, r in ((None, None), (col, None), (None, row), (col, row), (special, None), (special, row), (col.astype(np.float64).tolist(), row.tolist())):
            res_q, res_g, rq, rg = compute_retrieval_labeled_adjusted(sim, lab, c, r)
            wq, wg = _brute(sim, lab, c, r)
            assert rq.dtype == np.int32 and rg.dtype == np.int32
            assert _bytes_equal(rq, wq) and _bytes_equal(rg, wg), (exact_ties, c is not None, r is not None)
            assert res_q == _labeled_metrics(wq)[0] and res_g == _labeled_metrics(wg)[0]
        rq = compute_retrieval_labeled_adjusted(sim, lab, special)[2]
        assert rq[0] >= 0  # the label at +inf scores -inf and is still ranked: behind every finite column


def test_no_offsets_and_zero_offsets_are_the_labelled_ranking(cva):
    from coot_videotext_amd import compute_retrieval_labeled, compute_retrieval_labeled_adjusted
    rs = np.random.RandomState(3)
    m, n = 30, 17
    sim = rs.randint(-2, 3, size=(m, n)).astype(np.float32)
    sim[sim == 0] *= rs.choice([-1.0, 1.0], size=int((sim == 0).sum())).astype(np.float32)
    lab = _labels(rs, m, n)
    want = compute_retrieval_labeled(sim, lab)
    for c, r in ((None, None), (np.zeros(n), None), (None, np.zeros(m, np.float32)), ([0] * n, [0.0] * m)):
        got = compute_retrieval_labeled_adjusted(sim, lab, c, r)
        assert got[0] == want[0] and got[1] == want[1] and _bytes_equal(got[2], want[2]) and _bytes_equal(got[3], want[3])
    with pytest.raises(AssertionError):
        compute_retrieval_labeled_adjusted(sim, lab, np.zeros(n + 1))
    with pytest.raises(AssertionError):
        compute_retrieval_labeled_adjusted(sim, lab, None, np.zeros(m - 1))
    with pytest.raises(AssertionError):
        compute_retrieval_labeled_adjusted(sim.astype(np.float64), lab)


def test_column_offset_alone_is_the_position_in_the_adjusted_search(cva):
    from coot_videotext_amd import compute_retrieval_labeled_adjusted, compute_retrieval_topk_adjusted
    rs = np.random.RandomState(5)
    m, n = 25, 40
    for exact_ties in (False, True):
        sim = (rs.randint(-2, 3, size=(m, n)) if exact_ties else rs.randn(m, n)).astype(np.float32)
        col = (rs.randint(-1, 2, size=n) if exact_ties else 0.1 * rs.randn(n)).astype(np.float32)
        col[[0, n - 1]] = np.inf
        lab = _labels(rs, m, n)
        lab[0] = n - 1
        rq = compute_retrieval_labeled_adjusted(sim, lab, col)[2]
        idx = compute_retrieval_topk_adjusted(sim, col, n)[0]
        for i in range(m):
            if 0 <= lab[i] < n:
                assert idx[i, rq[i]] == lab[i], (i, exact_ties)
            else:
                assert rq[i] == -1


def _planted_hub(seed, n=300, d=32, m=200):
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


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_hub_on_the_mirrors(cva, seed):
    """query -> gallery R@1 under col = compute_retrieval_hub_offsets(...) is at least 0.1 above raw (seed 0: 0.670 -> 0.955), gallery ->
    query R@1 does not fall by more than 0.02."""
    from coot_videotext_amd import (compute_retrieval_hub_offsets, compute_retrieval_knn_join, compute_retrieval_labeled,
                                    compute_retrieval_labeled_adjusted)
    g, q, bank, lab = _planted_hub(seed)
    sim = (q @ g.T).astype(np.float32)
    idx, sc = compute_retrieval_knn_join((g @ bank.T).astype(np.float32), 10)
    col = compute_retrieval_hub_offsets(sc, idx)
    raw_q, raw_g, _, _ = compute_retrieval_labeled(sim, lab)
    cor_q, cor_g, _, _ = compute_retrieval_labeled_adjusted(sim, lab, col)
    assert cor_q["r1"] >= raw_q["r1"] + 0.1, (raw_q["r1"], cor_q["r1"])
    assert cor_g["r1"] >= raw_g["r1"] - 0.02, (raw_g["r1"], cor_g["r1"])
    if seed == 0:
        assert abs(raw_q["r1"] - 0.670) < 1e-6 and abs(cor_q["r1"] - 0.955) < 1e-6, (raw_q["r1"], cor_q["r1"])


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    args = re.search(r"\bcoot_retrieval_ranks_adjusted\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    order = ["const float* queries", "const float* gallery", "const int32_t* labels", "const float* row_offset", "const float* col_offset", "int M",
             "int N", "int d", "int normalize", "int32_t* ranks_q", "int32_t* ranks_g", "int32_t* n_valid", "float* metrics", "float* sim_out",
             "void* workspace", "size_t workspace_bytes", "coot_stream_t stream"]
    assert [a.strip() for a in " ".join(args.split()).split(",")] == order
    assert lib.coot_retrieval_ranks_adjusted_workspace_bytes.restype is ctypes.c_size_t
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    build = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "build.sh")).read()
    assert "retrieval_ranks_adjusted" in re.search(r'SRCS="([^"]*)"', build).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "coot-videotext_amd", "csrc", "retrieval_ranks_adjusted.hip"))
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\b", vs), name
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, so


def test_workspace_size(cva):
    """No device needed.  Exact: the layout of coot_retrieval_ranks_labeled, (2 M + N) floats, N 64-bit words and (M + N) int32, each
    piece rounded up to 256 bytes; 0 for arguments out of range."""
    lib = cva.lib.load()
    f = lib.coot_retrieval_ranks_adjusted_workspace_bytes

    def up(b):
        return (b + 255) // 256 * 256
    for m, n, d in ((130, 200, 64), (1, 300, 16), (5, 5, 37), (4917, 4917, 384), (18000, 18000, 384)):
        assert f(m, n, d) == 2 * up(4 * m) + up(4 * n) + up(8 * n) + up(4 * (m + n)), (m, n, d)
        assert f(m, n, d) == lib.coot_retrieval_ranks_labeled_workspace_bytes(m, n, d)
    for args in ((0, 5, 8), (5, 0, 8), (-1, 5, 8)):
        assert f(*args) == 0, args


def test_package_exports(cva):
    for name in ("compute_retrieval_labeled_adjusted", "retrieval_ranks_adjusted_device", "compute_retrieval_adjusted_device",
                 "compute_retrieval_csls_device"):
        assert callable(getattr(cva, name)), name
        assert getattr(cva.retrieval, name) is getattr(cva, name)
    assert cva.compute_retrieval_labeled_adjusted is cva.retrieval_mirror.compute_retrieval_labeled_adjusted


def test_wrappers_refuse_on_the_host(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  The shapes and types first (ValueError under the function's name), the
    offsets among them, then the devices ("no CPU fallback", naming the mirror)."""
    import torch
    fn = "retrieval_ranks_adjusted_device"
    q, g, lab = torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(3, dtype=torch.int32)
    for f in (cva.retrieval_ranks_adjusted_device, cva.compute_retrieval_adjusted_device):
        with pytest.raises(ValueError, match=fn + ": queries of width 7, gallery of width 8"):
            f(torch.zeros(3, 7), g, lab)
        with pytest.raises(ValueError, match=fn + ": queries has to be a torch.float32 tensor of two dimensions"):
            f(q.double(), g, lab)
        with pytest.raises(ValueError, match=fn + ": gallery has to be a torch.float32 tensor of two dimensions"):
            f(q, g[0], lab)
        for bad in (lab.long(), lab[:2], torch.zeros(5, dtype=torch.int32), [0, 1, 2]):  # M / N mismatches among them
            with pytest.raises(ValueError, match=fn + r": labels has to be a torch.int32 tensor \[3\]"):
                f(q, g, bad)
        for col in ([0.0] * 3, np.zeros(6, np.float32), torch.zeros(5, 1), 0.5):  # (3 = M: the column offset has N entries)
            with pytest.raises(ValueError, match=fn + r" \(col_offset\): offset of shape .* 5 rows"):
                f(q, g, lab, col)
        for row in ([0.0] * 5, np.zeros(4, np.float32), torch.zeros(3, 1)):  # (5 = N: the row offset has M entries)
            with pytest.raises(ValueError, match=fn + r" \(row_offset\): offset of shape .* 3 rows"):
                f(q, g, lab, None, row)
        for bad in (["a"] * 5, np.zeros(5, bool), torch.zeros(5, dtype=torch.bfloat16)):
            with pytest.raises(ValueError, match=fn + r" \(col_offset\): offset has to hold one number per gallery row, not dtype"):
                f(q, g, lab, bad)
        for col, row in ((None, None), ([0.0] * 5, None), (None, np.zeros(3)), (torch.zeros(5), torch.zeros(3, dtype=torch.float64))):
            with pytest.raises(RuntimeError, match=fn + " needs CUDA tensors .*no CPU fallback; use compute_retrieval_labeled_adjusted"):
                f(q, g, lab, col, row)


def test_csls_refuses_on_the_host(cva):
    import torch
    fn = "compute_retrieval_csls_device"
    f = cva.compute_retrieval_csls_device
    a, b = torch.zeros(12, 8), torch.zeros(12, 8)
    with pytest.raises(ValueError, match=fn + ": emb1 has to be a torch.float32 tensor of two dimensions"):
        f(a.half(), b)
    with pytest.raises(ValueError, match=fn + ": emb2 has to be a torch.float32 tensor of two dimensions"):
        f(a, b[0])
    with pytest.raises(ValueError, match=fn + ": emb1 of width 8, emb2 of width 7"):
        f(a, torch.zeros(12, 7))
    for k in (0, 13, 129, 2.0, True):
        with pytest.raises(ValueError, match=fn + r": k = .* is outside 1 .. min\(M = 12, N = 12, 128\)"):
            f(a, b, k)
    with pytest.raises(ValueError, match=fn + r": k = 10 is outside 1 .. min\(M = 12, N = 9, 128\)"):
        f(a, torch.zeros(9, 8), labels=torch.zeros(12, dtype=torch.int32))  # the default k = 10
    with pytest.raises(ValueError, match=fn + ": labels=None puts the ground truth on the diagonal"):
        f(a, torch.zeros(15, 8))
    for bad in (torch.zeros(12, dtype=torch.int64), torch.zeros(11, dtype=torch.int32), list(range(12))):
        with pytest.raises(ValueError, match=fn + r": labels has to be None or a torch.int32 tensor \[12\]"):
            f(a, b, 10, bad)
    for kw in (dict(), dict(k=1), dict(labels=torch.zeros(12, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match=fn + " needs CUDA tensors .*no CPU fallback; use compute_retrieval_labeled_adjusted"):
            f(a, b, **kw)
