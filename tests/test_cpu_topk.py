"""Host side of the top-K retrieval search (include/coot_hip.h: coot_retrieval_topk; retrieval.compute_retrieval_topk): the two
new functions are declared, bound and exported by both builds under the unchanged ABI version, and the numpy mirror — what the
device results are compared with bit for bit in tests/test_gpu_topk.py — follows the reference's definitions on the
reference-generated golden matrices (tests/golden/retrieval_metrics.npz, written by nntrainer/retrieval.py itself)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_workspace_bytes": 4, "coot_retrieval_topk": 13}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_topk_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert lib.coot_retrieval_topk_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_workspace_is_far_below_the_similarity_matrix(cva):
    """Pure host arithmetic: 1 024 queries against 200 000 clips need less than a quarter of the M x N fp32 matrix
    (in fact the row norms and the partial lists only)."""
    lib = cva.lib.load()
    m, n = 1024, 200000
    ws = lib.coot_retrieval_topk_workspace_bytes(m, n, 768, 10)
    assert 0 < ws < m * n * 4 // 4, ws


def test_host_mirror_on_the_golden_matrices(cva, golden_dir):
    from coot_videotext_amd.retrieval import compute_retrieval_topk
    g = np.load(os.path.join(golden_dir, "retrieval_metrics.npz"))
    tie_cases = 0
    for c in range(3):
        d = g[f"d{c}"].astype(np.float32)
        n = len(d)
        gold = g[f"ranks{c}"].astype(np.int64)
        for k in sorted({1, 5, min(n, 50), n}):
            idx, sc = compute_retrieval_topk(d, k)
            assert idx.shape == (n, k) and idx.dtype == np.int32 and sc.shape == (n, k) and sc.dtype == d.dtype
            assert np.array_equal(sc, d[np.arange(n)[:, None], idx])
            for i in range(n):
                row = d[i]
                # column 0 = the reference's top1 = argsort(row)[::-1][0] wherever the maximum is unique
                if (row == row.max()).sum() == 1:
                    assert idx[i, 0] == np.argsort(row)[::-1][0]
                # the position of i in row i = the golden rank, where it is inside k and the row has no tie with its diagonal
                where = np.where(idx[i] == i)[0]
                if (row == row[i]).sum() == 1:
                    assert (where[0] == gold[i]) if gold[i] < k else (len(where) == 0), (c, k, i)
                else:
                    tie_cases += 1
                # the rule itself, ties included: a stable ascending sort reversed (score descending, then index descending)
                want = np.argsort(row, kind="stable")[::-1][:k]
                assert np.array_equal(idx[i], want)
                assert all((sc[i, r] > sc[i, r + 1]) or (sc[i, r] == sc[i, r + 1] and idx[i, r] > idx[i, r + 1]) for r in range(k - 1))
    assert tie_cases > 0  # the fixture's forced-tie case was exercised


def test_host_mirror_rectangular_and_forced_ties(cva):
    from coot_videotext_amd.retrieval import compute_retrieval_topk
    sim = np.array([[0.5, 0.5, 0.1, 0.5], [0.0, -0.0, 1.0, -1.0]], dtype=np.float32)
    idx, sc = compute_retrieval_topk(sim, 3)
    assert idx.tolist() == [[3, 1, 0], [2, 1, 0]] and sc.tolist() == [[0.5, 0.5, 0.5], [1.0, 0.0, 0.0]]
    with pytest.raises(AssertionError):
        compute_retrieval_topk(sim, 5)


def test_device_entry_refuses_cpu_tensors(cva):
    import torch
    from coot_videotext_amd.retrieval import retrieval_topk_device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval_topk_device(torch.zeros(3, 8), torch.zeros(5, 8), 2)
