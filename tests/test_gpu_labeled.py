"""Labelled retrieval ranking on the MI355X (coot_retrieval_ranks_labeled; retrieval.retrieval_ranks_labeled_device) against the host
mirror (retrieval.compute_retrieval_labeled) ON THE MATRIX THE KERNEL COUNTED ON — the call can hand its fp32 similarities out, so
both rank vectors, n_valid and the 14 metric floats are compared bit for bit — against coot_retrieval_ranks on square input with
labels = arange, and against coot_retrieval_topk's matrix (the same FMA chain).  The matrix itself is held to the float64 product of
the unit rows within 2e-6 absolute, the bound tests/test_retrieval_device.py and tests/test_gpu_topk.py use for the same chain
(fp32 FMA chains of <= 768 terms on unit-norm rows)."""
import os

import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal as _bytes_equal, planted as _planted, unit as _unit

pytestmark = pytest.mark.gpu

# (M, N, d): one tile; partial tiles on either side with M > N and M < N; ~8 positives per column over several row tiles of one
# column tile; most gallery rows without a query at the video-level width
SHAPES = [(1, 1, 8), (130, 65, 32), (65, 130, 32), (300, 40, 96), (333, 1000, 768)]


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _labels(m, n, seed):
    """i mod N, a random tenth redirected to random rows, a few without ground truth."""
    rs = np.random.RandomState(seed)
    lab = (np.arange(m) % n).astype(np.int32)
    move = rs.rand(m) < 0.1
    lab[move] = rs.randint(0, n, size=int(move.sum()))
    if m > 1:
        lab[rs.choice(m, size=max(1, m // 40), replace=False)] = -1
    return lab


def _run(torch, q, g, lab, normalize, want_sim=False):
    from coot_videotext_amd.retrieval import retrieval_ranks_labeled_device
    out = retrieval_ranks_labeled_device(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(lab).cuda(),
                                         normalize=normalize, want_sim=want_sim)
    torch.cuda.synchronize()
    return [None if x is None else x.cpu().numpy() for x in out]


def _check_against_mirror(rq, rg, nv, met, sim, lab):
    from coot_videotext_amd.retrieval import VALKEYS, compute_retrieval_labeled
    res_q, res_g, want_q, want_g = compute_retrieval_labeled(sim, lab)
    m, n = sim.shape
    assert rq.dtype == np.int32 and rg.dtype == np.int32 and nv.dtype == np.int32 and met.dtype == np.float32
    assert rq.shape == (m,) and rg.shape == (n,) and nv.shape == (2,) and met.shape == (2, 7)
    assert np.array_equal(rq, want_q), np.argwhere(rq != want_q)[:5]
    assert np.array_equal(rg, want_g), np.argwhere(rg != want_g)[:5]
    assert np.array_equal(nv, [(want_q >= 0).sum(), (want_g >= 0).sum()])
    want_met = np.array([[r[k] for k in VALKEYS] for r in (res_q, res_g)], dtype=np.float32)
    assert _bytes_equal(met, want_met), (met, want_met)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("m,n,dim", SHAPES)
def test_labeled_is_exact(env, m, n, dim, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import retrieval_topk_device
    q, g = _planted(m, n, dim, m + n + dim)
    if not normalize:
        q, g = _unit(q), _unit(g)
    lab = _labels(m, n, m + 3 * n)
    rq, rg, nv, met, sim = _run(torch, q, g, lab, normalize, want_sim=True)
    a, b = (_unit(q), _unit(g)) if normalize else (q, g)  # fp32 rows x / sqrt(sum x^2), as validate_epoch normalises
    err = np.abs(sim - a.astype(np.float64) @ b.astype(np.float64).T).max()
    print(f"[{m} x {n} x {dim}, normalize = {normalize}] max |sim - float64 product| = {err:.3e}")
    assert err < 2e-6
    _check_against_mirror(rq, rg, nv, met, sim, lab)
    # the matrix the top-K search selects from, byte for byte
    sim_topk = retrieval_topk_device(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), 1, normalize=normalize, want_sim=True)[2]
    torch.cuda.synchronize()
    assert _bytes_equal(sim_topk.cpu().numpy(), sim)


@pytest.mark.parametrize("m,n,dim", [(300, 40, 96), (333, 1000, 768)])
def test_same_bytes_without_the_matrix_and_on_a_second_call(env, m, n, dim):
    torch, cva = env
    q, g = _planted(m, n, dim, 5 * m + n)
    lab = _labels(m, n, m + n)
    first = _run(torch, q, g, lab, True, want_sim=True)
    for want_sim in (False, False, True):
        again = _run(torch, q, g, lab, True, want_sim=want_sim)
        assert (again[4] is None) == (not want_sim)
        for x, y in zip(first[:4], again[:4]):
            assert _bytes_equal(x, y)
        if want_sim:
            assert _bytes_equal(first[4], again[4])


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n,dim", [(700, 96), (301, 384)])
def test_square_arange_is_the_rank_kernel(env, n, dim, normalize):
    """labels = arange on square input: both rank vectors and all 14 metric floats of coot_retrieval_ranks, byte for byte."""
    torch, cva = env
    from coot_videotext_amd.retrieval import retrieval_ranks_device, retrieval_ranks_labeled_device
    rs = np.random.RandomState(n + dim)
    e1 = rs.randn(n, dim).astype(np.float32)
    e2 = (0.35 * e1 + rs.randn(n, dim)).astype(np.float32)
    if not normalize:
        e1, e2 = _unit(e1), _unit(e2)
    t1, t2 = torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda()
    r12, r21, met_r, sim_r = retrieval_ranks_device(t1, t2, normalize=normalize, want_sim=True)
    rq, rg, nv, met, sim = retrieval_ranks_labeled_device(t1, t2, torch.arange(n, dtype=torch.int32, device="cuda"), normalize=normalize, want_sim=True)
    torch.cuda.synchronize()
    assert _bytes_equal(sim.cpu().numpy(), sim_r.cpu().numpy())
    assert _bytes_equal(rq.cpu().numpy(), r12.cpu().numpy()) and _bytes_equal(rg.cpu().numpy(), r21.cpu().numpy())
    assert _bytes_equal(met.cpu().numpy(), met_r.cpu().numpy())
    assert nv.cpu().numpy().tolist() == [n, n]


def test_forced_ties_through_identity(env, golden_dir):
    """gallery = identity makes the similarity matrix exactly the queries (products with 0 and 1 are exact): a golden matrix rounded
    to 84 distinct integer values, so ties run through every row and column; labels with duplicates, gaps and invalid entries."""
    torch, cva = env
    from coot_videotext_amd.retrieval import compute_retrieval_labeled, compute_retrieval_labeled_device
    d = np.load(os.path.join(golden_dir, "retrieval_metrics.npz"))["d2"].astype(np.float32)
    q = (np.round(d, 1) * 10).astype(np.float32)
    assert np.array_equal(q, np.round(q)) and len(np.unique(q)) < 100
    q[q == 0] = np.where(np.arange(int((q == 0).sum())) % 2 == 0, np.float32(-0.0), np.float32(0.0))  # -0 ties with +0
    n = len(q)
    eye = np.eye(n, dtype=np.float32)
    rs = np.random.RandomState(11)
    for lab in ((np.arange(n) // 3).astype(np.int32), rs.randint(-2, n + 2, size=n).astype(np.int32)):
        rq, rg, nv, met, sim = _run(torch, q, eye, lab, False, want_sim=True)
        assert np.array_equal(sim, q)
        _check_against_mirror(rq, rg, nv, met, q, lab)
        assert 0 < nv[1] < nv[0] <= n
        res_q, res_g, _, _ = compute_retrieval_labeled(q, lab)
        dev_q, dev_g, sum1 = compute_retrieval_labeled_device(torch.from_numpy(q).cuda(), torch.from_numpy(eye).cuda(), torch.from_numpy(lab).cuda())
        assert dev_q == res_q and dev_g == res_g and sum1 == (res_q["r1"] + res_g["r1"]) / 2


@pytest.mark.parametrize("which", ["minus_one", "n"])
def test_invalid_labels_only(env, which):
    torch, cva = env
    m, n, dim = 130, 65, 32
    q, g = _planted(m, n, dim, 3)
    lab = np.full(m, -1 if which == "minus_one" else n, dtype=np.int32)
    rq, rg, nv, met, _ = _run(torch, q, g, lab, True)
    assert (rq == -1).all() and (rg == -1).all() and nv.tolist() == [0, 0]
    assert _bytes_equal(met, np.zeros((2, 7), np.float32))


def test_refusals_launch_nothing(env):
    torch, cva = env
    lib = cva.lib.load()
    m, n, dim = 130, 65, 32
    q, g = torch.randn(m, dim, device="cuda"), torch.randn(n, dim, device="cuda")
    lab = torch.arange(m, dtype=torch.int32, device="cuda") % n
    rq = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    rg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    nv = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    met = torch.full((2, 7), -7.0, device="cuda")
    need = lib.coot_retrieval_ranks_labeled_workspace_bytes(m, n, dim)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(mm, nn, dd, ws_bytes):
        return lib.coot_retrieval_ranks_labeled(q.data_ptr(), g.data_ptr(), lab.data_ptr(), mm, nn, dd, 1, rq.data_ptr(), rg.data_ptr(), nv.data_ptr(),
                                                met.data_ptr(), None, ws.data_ptr(), ws_bytes, st)
    for what, args in {"workspace": (m, n, dim, need - 1), "M = 0": (0, n, dim, need), "N = 0": (m, 0, dim, need), "d = 0": (m, n, 0, need)}.items():
        assert call(*args) != 0, what
        msg = lib.coot_last_error().decode()
        assert "retrieval_labeled" in msg and ("workspace too small" in msg if what == "workspace" else "M = " in msg), (what, msg)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in (rq, rg, nv, met)) and not bool(ws.any()), what
    assert call(m, n, dim, need) == 0  # the same buffers, accepted
    torch.cuda.synchronize()
    assert bool((rq >= 0).all()) and bool((rg >= 0).all()) and nv.tolist() == [m, n]
