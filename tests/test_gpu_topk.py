"""Top-K retrieval search on the MI355X (coot_retrieval_topk; retrieval.retrieval_topk_device) against the host mirror
(retrieval.compute_retrieval_topk: a stable ascending argsort reversed) ON THE MATRIX THE KERNEL SELECTED FROM — the call can hand
its fp32 similarities out, so indices and scores are compared bit for bit — and against coot_retrieval_ranks on square input (the
same FMA chain and the same tie rule: item i sits at position ranks_12[i] of row i).  The matrix itself is held to the float64
product of the unit rows within 2e-6 absolute, the bound tests/test_retrieval_device.py uses for the same chain (fp32 FMA chains
of <= 768 terms on unit-norm rows)."""
import os

import numpy as np
import pytest

from oracle import coot_oracle as O

from tests.retrieval_cases import bytes_equal as _bytes_equal, check_against_mirror as _check_against_mirror, planted as _planted, unit as _unit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def splits(env):
    """Sets rt_topk_splits and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(n):
        assert lib.coot_set_option(b"rt_topk_splits", n) == 0
    yield set_
    set_(0)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("m,n,dim,k", [(700, 700, 96, 10), (333, 1000, 768, 50), (5, 4099, 384, 128), (1, 1, 8, 1), (130, 65, 32, 65)])
def test_topk_is_exact(env, m, n, dim, k, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import retrieval_topk_device
    q, g = _planted(m, n, dim, m + n + dim)
    if not normalize:
        q, g = _unit(q), _unit(g)
    idx, sc, sim = retrieval_topk_device(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), k, normalize=normalize, want_sim=True)
    torch.cuda.synchronize()
    idx, sc, sim = idx.cpu().numpy(), sc.cpu().numpy(), sim.cpu().numpy()
    a, b = (_unit(q), _unit(g)) if normalize else (q, g)  # fp32 rows x / sqrt(sum x^2), as validate_epoch normalises
    err = np.abs(sim - a.astype(np.float64) @ b.astype(np.float64).T).max()
    print(f"[{m} x {n} x {dim}, K = {k}, normalize = {normalize}] max |sim - float64 product| = {err:.3e}")
    assert err < 2e-6
    _check_against_mirror(idx, sc, sim, k)
    # without the testing aid: the same bytes
    idx2, sc2, none = retrieval_topk_device(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), k, normalize=normalize)
    torch.cuda.synchronize()
    assert none is None and _bytes_equal(idx2.cpu().numpy(), idx) and _bytes_equal(sc2.cpu().numpy(), sc)


def test_golden_matrices_through_identity(env, golden_dir):
    """gallery = identity makes the similarity matrix exactly the golden matrix d (products with 0 and 1 are exact), forced exact
    ties of case 1 included: the top-K must be the host mirror's, column 0 the reference's top1 where the maximum is unique, and the
    diagonal item must sit at the golden rank where the row has no tie with it."""
    torch, cva = env
    from coot_videotext_amd.retrieval import retrieval_topk_device
    g = np.load(os.path.join(golden_dir, "retrieval_metrics.npz"))
    ties = 0
    for c in range(3):
        d = g[f"d{c}"].astype(np.float32)
        n = len(d)
        gold = g[f"ranks{c}"].astype(np.int64)
        for k in sorted({1, min(n, 10), min(n, 128)}):
            idx, sc, sim = retrieval_topk_device(torch.from_numpy(d).cuda(), torch.eye(n, device="cuda"), k, normalize=False, want_sim=True)
            torch.cuda.synchronize()
            idx, sc, sim = idx.cpu().numpy(), sc.cpu().numpy(), sim.cpu().numpy()
            assert np.array_equal(sim, d)
            _check_against_mirror(idx, sc, d, k)
            for i in range(n):
                if (d[i] == d[i].max()).sum() == 1:
                    assert idx[i, 0] == np.argsort(d[i])[::-1][0]
                if (d[i] == d[i, i]).sum() == 1:
                    where = np.where(idx[i] == i)[0]
                    assert (where[0] == gold[i]) if gold[i] < k else (len(where) == 0)
                else:
                    ties += 1
    assert ties > 0


@pytest.mark.parametrize("n,dim,k,normalize", [(700, 96, 10, True), (333, 768, 50, False), (64, 32, 64, True), (2, 384, 1, False)])
def test_agrees_with_the_rank_kernel_on_square_input(env, n, dim, k, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import retrieval_ranks_device, retrieval_topk_device
    rs = np.random.RandomState(n + dim)
    e1 = rs.randn(n, dim).astype(np.float32)
    e2 = (0.35 * e1 + rs.randn(n, dim)).astype(np.float32)
    if not normalize:
        e1, e2 = _unit(e1), _unit(e2)
    t1, t2 = torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda()
    r12, r21, _, sim_r = retrieval_ranks_device(t1, t2, normalize=normalize, want_sim=True)
    idx12, _, sim_12 = retrieval_topk_device(t1, t2, k, normalize=normalize, want_sim=True)
    idx21, _, sim_21 = retrieval_topk_device(t2, t1, k, normalize=normalize, want_sim=True)
    torch.cuda.synchronize()
    sim_r = sim_r.cpu().numpy()
    assert _bytes_equal(sim_12.cpu().numpy(), sim_r)
    assert _bytes_equal(sim_21.cpu().numpy(), np.ascontiguousarray(sim_r.T))  # (a product of two floats does not depend on their order)
    for idx, ranks in ((idx12.cpu().numpy(), r12.cpu().numpy()), (idx21.cpu().numpy(), r21.cpu().numpy())):
        hit = idx == np.arange(n, dtype=np.int32)[:, None]
        inside = ranks < k
        assert inside.any() and np.array_equal(hit.any(1), inside)
        assert np.array_equal(hit.argmax(1)[inside], ranks[inside]) and (hit.sum(1) <= 1).all()


@pytest.mark.parametrize("m,n,dim,k,signs", [(333, 1000, 768, 50, False), (5, 4099, 384, 128, False), (700, 700, 96, 10, False), (64, 640, 40, 7, True)])
def test_result_does_not_depend_on_splits_or_schedule(env, splits, m, n, dim, k, signs):
    """The column range is split over workgroups and the partial lists are merged: 1 split (no merge launch), 3 splits, the
    automatic choice, a forced maximum and a second run of the same call give identical bytes.  The last shape (signs: +-1 entries) has rows of a few
    repeated values: whole runs of exact ties cross the split boundaries."""
    torch, cva = env
    from coot_videotext_amd.retrieval import retrieval_topk_device
    q, g = _planted(m, n, dim, 7 * m + n)
    if signs:
        q, g = np.sign(q).astype(np.float32), np.sign(g).astype(np.float32)  # similarities are small integers: ties everywhere
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    got = []
    for s in (1, 3, 0, 0, 64):
        splits(s)
        idx, sc, sim = retrieval_topk_device(tq, tg, k, normalize=False, want_sim=(s == 1))
        torch.cuda.synchronize()
        got.append((idx.cpu().numpy(), sc.cpu().numpy()))
        if s == 1:
            _check_against_mirror(got[0][0], got[0][1], sim.cpu().numpy(), k)
    for idx, sc in got[1:]:
        assert _bytes_equal(idx, got[0][0]) and _bytes_equal(sc, got[0][1])


def test_refusals_write_nothing(env):
    torch, cva = env
    lib = cva.lib.load()
    m, n, dim = 40, 300, 16
    q, g = torch.randn(m, dim, device="cuda"), torch.randn(n, dim, device="cuda")
    idx = torch.full((m, 128), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((m, 128), -7.0, device="cuda")
    ws = torch.zeros(lib.coot_retrieval_topk_workspace_bytes(m, n, dim, 128) + (1 << 20), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(nn, k, ws_bytes):
        return lib.coot_retrieval_topk(q.data_ptr(), g.data_ptr(), m, nn, dim, k, 1, idx.data_ptr(), sc.data_ptr(), None, ws.data_ptr(), ws_bytes, st)
    for what, (nn, k, ws_bytes) in {"K = 0": (n, 0, ws.numel()), "K > N": (100, 101, ws.numel()), "K > 128": (n, 129, ws.numel()),
                                    "workspace": (n, 10, 64)}.items():
        assert call(nn, k, ws_bytes) != 0, what
        msg = lib.coot_last_error().decode()
        assert "retrieval_topk" in msg and ("workspace too small" in msg if what == "workspace" else "K = " in msg), (what, msg)
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool((sc == -7.0).all()) and not bool(ws.any()), what
    assert call(n, 128, ws.numel()) == 0  # the same buffers, accepted
    torch.cuda.synchronize()
    assert bool(((idx >= 0) & (idx < n)).all())
    from coot_videotext_amd.retrieval import retrieval_topk_device
    with pytest.raises(RuntimeError, match="K = 301"):
        retrieval_topk_device(q, g, 301)


def test_large_gallery_without_the_matrix(env):
    """1 024 queries against 200 000 clips of width 768: the workspace is below a quarter of the M x N fp32 matrix (819 MB) and
    the call completes with nothing allocated but the inputs (0.8 GB), the outputs and that workspace — measured on the
    allocator's peak, which an M x N tensor would more than double.  Spot rows are checked against a float64 product."""
    torch, cva = env
    lib = cva.lib.load()
    m, n, dim, k = 1024, 200000, 768, 10
    ws_bytes = lib.coot_retrieval_topk_workspace_bytes(m, n, dim, k)
    assert ws_bytes < m * n * 4 // 4, ws_bytes
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randn(n, dim, device="cuda", generator=gen)
    q = torch.randn(m, dim, device="cuda", generator=gen) + 0.5 * g[torch.arange(m, device="cuda") * 190]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    idx = torch.empty(m, k, dtype=torch.int32, device="cuda")
    sc = torch.empty(m, k, dtype=torch.float32, device="cuda")
    rc = lib.coot_retrieval_topk(q.data_ptr(), g.data_ptr(), m, n, dim, k, 1, idx.data_ptr(), sc.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.coot_last_error()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"workspace {ws_bytes} bytes; allocated during the call {grown} bytes; M x N x 4 = {m * n * 4}")
    assert grown <= ws_bytes + 2 * m * k * 4 + (1 << 16) and grown < m * n * 4 // 4
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert (idx[:, 0] == np.arange(m) * 190).mean() > 0.99  # the planted clip wins
    gu = g / (g * g).sum(-1, keepdim=True).sqrt()
    for i in (0, 511, 1023):
        qi = q[i] / (q[i] * q[i]).sum().sqrt()
        s64 = (gu.double() @ qi.double()).cpu().numpy()
        order = np.argsort(s64, kind="stable")[::-1][:k]
        assert np.abs(sc[i] - s64[idx[i]]).max() < 2e-6
        # the float64 order can differ from the fp32 one only between scores closer than the chain's error
        assert all(idx[i, r] == order[r] or abs(s64[idx[i, r]] - s64[order[r]]) < 4e-6 for r in range(k))
        assert (np.diff(sc[i]) <= 0).all()


def test_validate_epoch_topk(env):
    """validate_epoch(topk=5) on the three synthetic batches of tests/test_retrieval_device.py: every key of the plain result is
    unchanged, and out["topk"] is the host mirror on the fp32 device similarities of the collected, normalised embeddings."""
    torch, cva = env
    from tests import helpers as H
    from coot_videotext_amd.retrieval import compute_retrieval_topk, retrieval_topk_device
    dims = (64, 48, 64, 4, 64, 128)
    cfgs = H.full_cfgs(*dims)
    Ps = [O.make_params(cfgs[i], 1 + i, scale=0.05) for i in range(4)]
    cfg, mgr = H.make_manager(cfgs, Ps, dropout=0.0)
    tr = cva.RetrievalTrainer(cfg, mgr, is_test=True)
    batches = [cva.synthetic.make_batch(10 + i, 6, [1, 2, 3, 4, 2, 1], 12, 10, 9, 6, dims[0], dims[1], ragged=True) for i in range(3)]
    # (the cycle-consistency part of "loss" draws one random position per video, as the reference's validation does: both calls get
    # the same seeded generator, so that the loss too can be compared for equality)
    tr.cc_generator = torch.Generator(device="cuda").manual_seed(3)
    plain = tr.validate_epoch(batches)
    tr.cc_generator = torch.Generator(device="cuda").manual_seed(3)
    out = tr.validate_epoch(batches, topk=5)
    assert "topk" not in plain and set(out) == set(plain) | {"topk"}
    for key in plain:
        assert out[key] == plain[key], key
    assert set(out["topk"]) == {"v2p", "p2v", "c2s", "s2c"}
    assert set(tr.validate_epoch(batches, val_clips=False, topk=5)["topk"]) == {"v2p", "p2v"}
    mgr.set_all_models_eval()
    with torch.no_grad():
        vis = [mgr.encode_visual(b) for b in batches]
        txt = [mgr.encode_text(b) for b in batches]
    emb = {"vid": torch.cat([x.vid_emb for x in vis]).float(), "par": torch.cat([x.par_emb for x in txt]).float(),
           "clip": torch.cat([x.clip_emb for x in vis]).float(), "sent": torch.cat([x.sent_emb for x in txt]).float()}
    for name, a, b in (("v2p", "vid", "par"), ("p2v", "par", "vid"), ("c2s", "clip", "sent"), ("s2c", "sent", "clip")):
        _, _, sim = retrieval_topk_device(emb[a], emb[b], 5, normalize=True, want_sim=True)
        torch.cuda.synchronize()
        want_idx, want_sc = compute_retrieval_topk(sim.cpu().numpy(), 5)
        idx, sc = out["topk"][name]
        assert isinstance(idx, np.ndarray) and isinstance(sc, np.ndarray)
        assert _bytes_equal(idx, want_idx) and _bytes_equal(sc, want_sc), name
    # R@1 of the metric dictionaries is the share of queries whose first retrieved item is their own
    n = len(emb["vid"])
    assert abs((out["topk"]["v2p"][0][:, 0] == np.arange(n)).mean() - out["v2p"]["r1"]) < 1e-6
