"""Host side of the labelled retrieval ranking (include/coot_hip.h: coot_retrieval_ranks_labeled; retrieval.compute_retrieval_labeled):
the numpy mirror — what the device results are compared with bit for bit in tests/test_gpu_labeled.py — against brute-force stable
argsorts on tie-heavy matrices, against the square functions on the reference-generated golden matrices
(tests/golden/retrieval_metrics.npz), its metric arithmetic, and the two new functions declared, bound and exported by both
builds under the unchanged ABI version."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_ranks_labeled_workspace_bytes": 3, "coot_retrieval_ranks_labeled": 15}
SHAPES = [(7, 7), (130, 65), (65, 130), (300, 40), (1, 1)]


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _brute(sim, labels):
    """Positions in stable ascending argsorts reversed: per row the label's column, per column the minimum over its positives."""
    m, n = sim.shape
    rq, rg = np.full(m, -1, np.int32), np.full(n, -1, np.int32)
    valid = (labels >= 0) & (labels < n)
    for i in range(m):
        if valid[i]:
            rq[i] = np.where(np.argsort(sim[i], kind="stable")[::-1] == labels[i])[0][0]
    for j in range(n):
        pos = np.nonzero(valid & (labels == j))[0]
        if len(pos):
            order = np.argsort(sim[:, j], kind="stable")[::-1]
            rg[j] = min(np.where(order == i)[0][0] for i in pos)
    return rq, rg


def _tie_matrix(m, n, seed):
    rs = np.random.RandomState(seed)
    sim = rs.randint(-3, 4, size=(m, n)).astype(np.float32)  # seven values: ties in every row and column
    sim[sim == 0] = np.where(rs.rand(int((sim == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))  # -0 ties with +0
    return rs, sim


@pytest.mark.parametrize("invalid", [False, True])
@pytest.mark.parametrize("m,n", SHAPES)
def test_mirror_against_brute_force(cva, m, n, invalid):
    from coot_videotext_amd.retrieval import compute_retrieval_labeled
    rs, sim = _tie_matrix(m, n, 100 * m + n)
    labels = rs.randint(0, n, size=m).astype(np.int32)
    if invalid:
        labels[rs.rand(m) < 0.2] = -1
        labels[rs.rand(m) < 0.2] = n
        labels[0] = -1 if m > 1 else n
    res_q, res_g, rq, rg = compute_retrieval_labeled(sim, labels)
    want_q, want_g = _brute(sim, labels)
    assert rq.dtype == np.int32 and rg.dtype == np.int32
    assert np.array_equal(rq, want_q) and np.array_equal(rg, want_g)
    valid = (labels >= 0) & (labels < n)
    assert np.array_equal(rq >= 0, valid) and np.array_equal(rg >= 0, np.isin(np.arange(n), labels[valid]))
    for res, r in ((res_q, want_q), (res_g, want_g)):
        r = r[r >= 0]
        assert list(res) == cva.retrieval.VALKEYS
        if len(r):
            assert res["r1"] == float(np.float32((r < 1).sum()) / np.float32(len(r)))
            assert res["medr"] == float(np.floor(np.median(r)) + 1) and res["meanr"] == float(np.float32(r.mean() + 1))
        else:
            assert all(v == 0.0 for v in res.values())


def test_square_arange_is_the_square_functions(cva, golden_dir):
    from coot_videotext_amd.retrieval import compute_retrieval_cosine, compute_retrieval_counts_part, compute_retrieval_labeled
    g = np.load(os.path.join(golden_dir, "retrieval_metrics.npz"))
    untied = 0
    for c in range(3):
        d = g[f"d{c}"].astype(np.float32)
        n = len(d)
        res_q, res_g, rq, rg = compute_retrieval_labeled(d, np.arange(n, dtype=np.int32))
        c12, c21 = compute_retrieval_counts_part(d, 0, n)
        assert np.array_equal(rq, c12) and np.array_equal(rg, c21)
        for sim, ranks, res in ((d, rq, res_q), (d.T, rg, res_g)):
            ref, _, ref_ranks = compute_retrieval_cosine(sim)
            free = np.array([(sim[i] == sim[i, i]).sum() == 1 for i in range(n)])
            untied += int(free.sum())
            assert np.array_equal(ranks[free], ref_ranks[free].astype(np.int32))
            if free.all():
                assert all(abs(res[k] - ref[k]) < 1e-6 * max(1.0, abs(ref[k])) for k in ref), (res, ref)
    assert untied > 0


def test_metric_formulas(cva):
    from coot_videotext_amd.retrieval import compute_retrieval_labeled
    # 4 queries, 3 gallery rows; query 3 has no ground truth, gallery row 2 has no query; queries 0 and 1 share row 0
    sim = np.array([[5, 1, 9], [7, 8, 9], [2, 3, 1], [9, 9, 9]], dtype=np.float32)
    labels = np.array([0, 0, 1, -1], dtype=np.int32)
    res_q, res_g, rq, rg = compute_retrieval_labeled(sim, labels)
    assert rq.tolist() == [1, 2, 0, -1]
    # column 0 = (5, 7, 2, 9): the best positive is query 1 (7), only the unlabelled query 3 is ahead; column 1 = (1, 8, 3, 9): 3 -> 2 ahead
    assert rg.tolist() == [1, 2, -1]
    assert res_q == {"r1": float(np.float32(1) / np.float32(3)), "r5": 1.0, "r10": 1.0, "r50": 1.0, "medr": 2.0, "meanr": 2.0,
                     "sum": float(np.float32(1) / np.float32(3) + np.float32(1) + np.float32(1))}
    # two entries (1, 2): the median 1.5 lies between two integers, medr = floor(1.5) + 1
    assert res_g == {"r1": 0.0, "r5": 1.0, "r10": 1.0, "r50": 1.0, "medr": 2.0, "meanr": 2.5, "sum": 2.0}
    # a direction with n == 0 (both, here): seven zeros, ranks all -1
    res_q, res_g, rq, rg = compute_retrieval_labeled(sim, np.array([-1, 3, 7, -5], dtype=np.int32))
    assert (rq == -1).all() and (rg == -1).all()
    assert res_q == res_g == {k: 0.0 for k in cva.retrieval.VALKEYS}
    # an equal best positive: the later query is the best one, the earlier is not counted ahead of it
    sim = np.array([[4.0], [4.0], [4.0]], dtype=np.float32)
    _, _, rq, rg = compute_retrieval_labeled(sim, np.array([0, 0, -1], dtype=np.int32))
    assert rq.tolist() == [0, 0, -1] and rg.tolist() == [1]  # the unlabelled query 2 ties and is later: ahead


def test_labeled_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert lib.coot_retrieval_ranks_labeled_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7 and lib.coot_version() == 7  # new functions only
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_workspace_is_far_below_the_similarity_matrix(cva):
    """Pure host arithmetic: 20 000 queries against 4 917 items need the norms, one score per query, one word per item and the
    histograms — not the 393 MB matrix; bad sizes need nothing."""
    lib = cva.lib.load()
    m, n = 20000, 4917
    ws = lib.coot_retrieval_ranks_labeled_workspace_bytes(m, n, 768)
    assert (2 * m + n) * 4 + n * 8 + (m + n) * 4 <= ws < 1 << 20, ws
    assert lib.coot_retrieval_ranks_labeled_workspace_bytes(0, n, 768) == 0


def test_device_entry_refuses_cpu_tensors(cva):
    import torch
    from coot_videotext_amd.retrieval import compute_retrieval_labeled_device, retrieval_ranks_labeled_device
    assert cva.retrieval_ranks_labeled_device is retrieval_ranks_labeled_device and cva.compute_retrieval_labeled is cva.retrieval.compute_retrieval_labeled
    lab = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_labeled"):
        retrieval_ranks_labeled_device(torch.zeros(3, 8), torch.zeros(5, 8), lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_retrieval_labeled_device(torch.zeros(3, 8), torch.zeros(5, 8), lab)
