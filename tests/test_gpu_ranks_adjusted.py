"""The labelled ranking under offsets (coot_retrieval_ranks_adjusted; retrieval_ranks_adjusted_device, compute_retrieval_adjusted_device,
compute_retrieval_csls_device) against its definition.  The similarities come back with want_sim=True and have to be the bytes of
retrieval_ranks_labeled_device's; ranks, n_valid and metrics have to be, byte for byte, the host mirror
compute_retrieval_labeled_adjusted of those bytes (tests/test_cpu_ranks_adjusted.py checks the mirror against a brute force) — whatever
the offsets; without offsets and with zeros they are the bytes of retrieval_ranks_labeled_device.  With a column offset alone a query's
rank is the position of its label in GalleryIndex.search_adjusted.  Last, the planted hub through compute_retrieval_csls_device.
Shapes (M, N, d): (130, 200, 64) three by four tiles with short last ones; (70, 130, 37) a width that is no multiple of the chunk;
(200, 63, 16) one column tile, not full; (1, 300, 16) one query; (5, 5, 37) fewer rows than a tile on both sides."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted, unit

pytestmark = pytest.mark.gpu

SHAPES = [(130, 200, 64), (70, 130, 37), (200, 63, 16), (1, 300, 16), (5, 5, 37)]


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _labels(m, n, seed=2):
    """Several queries per row, rows without a query, and -1 and N among the labels."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, n, size=m)
    lab[rs.rand(m) < 0.3] = rs.randint(0, max(1, n // 3))
    if m > 4:
        lab[1], lab[3] = -1, n
    return lab.astype(np.int32)


def _assert_mirror(got, labels, col, row):
    """ranks, n_valid and metrics are the mirror of the returned similarities."""
    from coot_videotext_amd import compute_retrieval_labeled_adjusted
    from coot_videotext_amd.retrieval_mirror import _labeled_metrics
    rq, rg, nv, met, sim = got
    _, _, wq, wg = compute_retrieval_labeled_adjusted(sim, labels, col, row)
    assert rq.dtype == np.int32 and rg.dtype == np.int32 and nv.dtype == np.int32 and met.dtype == np.float32 and met.shape == (2, 7)
    assert bytes_equal(rq, wq), np.argwhere(rq != wq)[:5]
    assert bytes_equal(rg, wg), np.argwhere(rg != wg)[:5]
    assert nv.tolist() == [int((wq >= 0).sum()), int((wg >= 0).sum())]
    assert bytes_equal(met, np.stack([_labeled_metrics(wq)[1], _labeled_metrics(wg)[1]]))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_ranks_are_the_mirror_of_their_similarities(env, shape, normalize):
    torch, cva = env
    m, n, dim = shape
    q, g = _planted(m, n, dim, 17)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    lab = _labels(m, n)
    tl = _dev(torch, lab)
    plain = _host(torch, *cva.retrieval_ranks_labeled_device(tq, tg, tl, normalize=normalize, want_sim=True))
    rs = np.random.RandomState(5)
    scale = 0.1 if normalize else 0.1 * dim ** 0.5  # about a tenth of the similarities' spread
    col, row = (scale * rs.randn(n)).astype(np.float32), (scale * rs.randn(m)).astype(np.float32)
    inf_col = col.copy()
    inf_col[sorted({c for c in (0, 63, 64, n - 1) if c < n})] = np.inf
    lab_inf = lab.copy()
    lab_inf[0] = n - 1  # a labelled column at +inf
    cases = [("none", None, None, lab), ("col", col, None, lab), ("row", None, row, lab), ("both", col, row, lab),
             ("zeros", np.zeros(n, np.float32), np.zeros(m, np.float32), lab), ("zero col", np.zeros(n, np.float32), None, lab),
             ("inf", inf_col, row, lab_inf), ("inf col", inf_col, None, lab_inf)]
    for t, (name, c, r, lb) in enumerate(cases):
        # a host list, a host array, the device
        tc, tr = [None if o is None else o.tolist() if (t + s) % 3 == 0 else o if (t + s) % 3 == 1 else _dev(torch, o) for s, o in enumerate((c, r))]
        tlb = tl if lb is lab else _dev(torch, lb)
        got = _host(torch, *cva.retrieval_ranks_adjusted_device(tq, tg, tlb, tc, tr, normalize=normalize, want_sim=True))
        _assert_mirror(got, lb, c, r)
        assert bytes_equal(got[4], plain[4]), name  # the raw similarities of the labelled ranking
        if name in ("none", "zeros", "zero col"):  # against code that exists without this call
            for a, b in zip(got[:4], plain[:4]):
                assert bytes_equal(a, b), name
        again = _host(torch, *cva.retrieval_ranks_adjusted_device(tq, tg, tlb, tc, tr, normalize=normalize)[:4])  # a second run, without sim
        for a, b in zip(again, got[:4]):
            assert bytes_equal(a, b), name
        if name == "inf col":
            assert got[0][0] >= 0 and got[1][n - 1] >= 0  # still a column, still a valid label


@pytest.mark.parametrize("shape", [(130, 200, 64), (200, 63, 16), (5, 5, 37)])
def test_integer_scores_tie_across_tile_edges(env, shape):
    """Integer embeddings and integer offsets without normalisation: whole runs of a are equal, and only the tie rule orders them."""
    torch, cva = env
    m, n, dim = shape
    rs = np.random.RandomState(m + n)
    q, g = rs.randint(-1, 2, size=(m, dim)).astype(np.float32), rs.randint(-1, 2, size=(n, dim)).astype(np.float32)
    g[n // 2:] = g[:n - n // 2]  # repeated rows: equal columns on both sides of a tile edge
    col, row = rs.randint(-1, 2, size=n).astype(np.float32), rs.randint(-1, 2, size=m).astype(np.float32)
    lab = _labels(m, n, seed=9)
    tq, tg, tl = _dev(torch, q), _dev(torch, g), _dev(torch, lab)
    for c, r in ((col, None), (None, row), (col, row)):
        got = _host(torch, *cva.retrieval_ranks_adjusted_device(tq, tg, tl, _dev(torch, c), _dev(torch, r), want_sim=True))
        assert np.array_equal(got[4], (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.float32))  # small integers: exact in any order
        _assert_mirror(got, lab, c, r)
        a = got[4] - (0 if c is None else c[None, :]) - (0 if r is None else r[:, None])
        assert min(len(np.unique(a[i])) for i in range(m)) < n  # there are ties


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_a_rank_below_k_is_the_position_in_search_adjusted(env, storage):
    torch, cva = env
    for m, n, dim in ((130, 200, 64), (70, 130, 37), (5, 5, 37)):
        q, g = _planted(m, n, dim, 17)
        g = _host(torch, torch.tensor(g).to(getattr(torch, storage)).float().cuda())[0]  # rows that the storage holds exactly
        tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        lab = _labels(m, n)
        col = (0.1 * np.random.RandomState(6).randn(n)).astype(np.float32)
        col[[0, n - 1]] = np.inf
        tc = _dev(torch, col)
        rq = _host(torch, cva.retrieval_ranks_adjusted_device(tq, tg, _dev(torch, lab), tc, normalize=True)[0])[0]
        k = min(n, 128)
        idx = _host(torch, cva.GalleryIndex(tg, normalize=True, storage=getattr(torch, storage)).search_adjusted(tq, k, tc)[0])[0]
        for i in range(m):
            if 0 <= lab[i] < n:
                hit = np.nonzero(idx[i] == lab[i])[0]
                assert (rq[i] < k) == (len(hit) == 1) and (rq[i] >= k or hit[0] == rq[i]), i
            else:
                assert rq[i] == -1


def planted_hub(seed=0, n=300, d=32, m=200):
    """tests/test_gpu_topk_adjusted.py::planted_hub: row n - 1 is the common direction that every query and every bank row leans towards."""
    rs = np.random.RandomState(seed)
    x, c = rs.randn(n, d), rs.randn(1, d)
    g = unit(x)
    g[n - 1] = unit(c)
    lab = rs.permutation(n - 1)[:m]
    q = unit(g[lab] + 0.9 * unit(rs.randn(m, d)) + 0.9 * unit(c))
    lab_b = rs.permutation(n - 1)[:m]
    bank = unit(g[lab_b] + 0.9 * unit(rs.randn(m, d)) + 0.9 * unit(c))
    return g.astype(np.float32), q.astype(np.float32), bank.astype(np.float32), lab


def test_planted_hub_end_to_end(env):
    """The explicit calls with a bank (query -> gallery R@1 at least 0.1 above raw, gallery -> query within 0.02), the device metrics
    the mirror's; then compute_retrieval_csls_device, the queries themselves as the bank, against the same calls made by hand."""
    torch, cva = env
    from coot_videotext_amd import compute_retrieval_labeled_adjusted
    g, q, bank, lab = planted_hub(0)
    tq, tg, tl = _dev(torch, q), _dev(torch, g), _dev(torch, lab.astype(np.int32))
    index, bank_index = cva.GalleryIndex(tg, normalize=True), cva.GalleryIndex(_dev(torch, bank), normalize=True)
    col = index.hubness_offsets(bank_index, 10)
    raw_q, raw_g, _ = cva.compute_retrieval_labeled_device(tq, tg, tl, normalize=True)
    got = _host(torch, *cva.retrieval_ranks_adjusted_device(tq, tg, tl, col, normalize=True, want_sim=True))
    _assert_mirror(got, lab, _host(torch, col)[0], None)
    cor_q, cor_g, s1 = cva.compute_retrieval_adjusted_device(tq, tg, tl, col, normalize=True)
    want_q, want_g, _, _ = compute_retrieval_labeled_adjusted(got[4], lab, _host(torch, col)[0])
    assert cor_q == want_q and cor_g == want_g and s1 == (cor_q["r1"] + cor_g["r1"]) / 2
    print(f"q->g R@1: {raw_q['r1']:.3f} -> {cor_q['r1']:.3f}; g->q R@1: {raw_g['r1']:.3f} -> {cor_g['r1']:.3f}")
    assert cor_q["r1"] >= raw_q["r1"] + 0.1, (raw_q["r1"], cor_q["r1"])
    assert cor_g["r1"] >= raw_g["r1"] - 0.02, (raw_g["r1"], cor_g["r1"])
    # CSLS of the pair itself: both offsets, each side the other's bank
    idx_q = cva.GalleryIndex(tq, normalize=True)
    row, col2 = idx_q.hubness_offsets(index, 10), index.hubness_offsets(idx_q, 10)
    by_hand = _host(torch, *cva.retrieval_ranks_adjusted_device(tq, tg, tl, col2, row, normalize=True, want_sim=True))
    _assert_mirror(by_hand, lab, *_host(torch, col2, row))
    res = cva.compute_retrieval_csls_device(tq, tg, 10, tl)
    assert res == cva.retrieval._metric_dicts(torch.from_numpy(by_hand[3]))
    assert res[0]["r1"] >= raw_q["r1"] + 0.1, (raw_q["r1"], res[0]["r1"])
    sq = cva.compute_retrieval_csls_device(tg[:200], tg[:200] + 0.0, 5)  # labels=None: the diagonal
    assert sq[0]["r1"] == 1.0 and sq[1]["r1"] == 1.0


class _CCall:
    """coot_retrieval_ranks_adjusted through ctypes on buffers with a known fill."""

    def __init__(self, torch, cva, m, n, dim):
        self.lib, self.m, self.n, self.dim = cva.lib.load(), m, n, dim
        q, g = _planted(m, n, dim, 11)
        self.q, self.g = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        self.lab = torch.zeros(m, dtype=torch.int32, device="cuda")
        self.size = self.lib.coot_retrieval_ranks_adjusted_workspace_bytes(m, n, dim)
        self.ws = torch.zeros(self.size + 16, dtype=torch.uint8, device="cuda")
        self.rq = torch.full((m,), -7, dtype=torch.int32, device="cuda")
        self.rg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.nv = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        self.met = torch.full((14,), -7.0, device="cuda")
        self.col, self.row = torch.zeros(n, device="cuda"), torch.zeros(m, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def __call__(self, m=None, n=None, d=None, q=-1, rq=-1, ws=-1, ws_bytes=None, ws_off=0, col=-1, row=-1):
        p = lambda v, t: t.data_ptr() if v == -1 else v  # noqa: E731
        return self.lib.coot_retrieval_ranks_adjusted(p(q, self.q), self.g.data_ptr(), self.lab.data_ptr(), p(row, self.row), p(col, self.col),
                                                      self.m if m is None else m, self.n if n is None else n, self.dim if d is None else d, 1,
                                                      p(rq, self.rq), self.rg.data_ptr(), self.nv.data_ptr(), self.met.data_ptr(), None,
                                                      None if ws is None else self.ws.data_ptr() + ws_off,
                                                      self.size if ws_bytes is None else ws_bytes, self.st)

    def untouched(self, torch):
        torch.cuda.synchronize()
        return (bool((self.rq == -7).all()) and bool((self.rg == -7).all()) and bool((self.nv == -7).all()) and bool((self.met == -7.0).all())
                and not bool(self.ws.any()))


def test_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message under the new name, and every buffer as it was."""
    torch, cva = env
    c = _CCall(torch, cva, 70, 130, 16)
    cases = {"M = 0": (dict(m=0), "M = 0"), "N = 0": (dict(n=0), "N = 0"), "d = 0": (dict(d=0), "d = 0"),
             "row tiles": (dict(m=65535 * 64 + 1), "M = 4194241"), "null queries": (dict(q=None), "null pointer"),
             "null output": (dict(rq=None), "null pointer"), "null workspace": (dict(ws=None), "null pointer"),
             "one byte short": (dict(ws_bytes=c.size - 1), "workspace too small"), "misaligned": (dict(ws_off=4), "8-byte aligned")}
    for what, (kw, part) in cases.items():
        assert c(**kw) != 0, what
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_ranks_adjusted:" in msg and part in msg, (what, msg)
        assert c.untouched(torch), what
    for kw in (dict(), dict(col=None), dict(row=None), dict(col=None, row=None)):  # either offset may be null; exactly the layout's size
        assert c(**kw) == 0, c.lib.coot_last_error()
        torch.cuda.synchronize()
        assert bool((c.rq >= 0).all()) and c.nv.tolist() == [70, 1] and int(c.rg[0]) >= 0 and bool((c.rg[1:] == -1).all())


def test_arguments_are_refused_on_the_host(env):
    """What needs a device to get as far as the check: an offset on the device of the wrong type or shape, and tensors that are not."""
    torch, cva = env
    fn = "retrieval_ranks_adjusted_device"
    q, g, lab = torch.zeros(3, 8, device="cuda"), torch.zeros(5, 8, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=fn + r" \(col_offset\): offset of shape \(3,\), a gallery of 5 rows"):
        cva.retrieval_ranks_adjusted_device(q, g, lab, torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError, match=fn + r" \(row_offset\): offset of shape \(5,\), a gallery of 3 rows"):
        cva.retrieval_ranks_adjusted_device(q, g, lab, None, torch.zeros(5, device="cuda"))
    with pytest.raises(ValueError, match=fn + r" \(col_offset\): offset on the device has to be torch.float32, not torch.float64"):
        cva.retrieval_ranks_adjusted_device(q, g, lab, torch.zeros(5, device="cuda").double())
    with pytest.raises(ValueError, match=fn + r" \(col_offset\): offset lives on cuda:0, the gallery on cpu"):
        cva.retrieval_ranks_adjusted_device(q, g.cpu(), lab, torch.zeros(5, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_labeled_adjusted"):
        cva.retrieval_ranks_adjusted_device(q, g, lab.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_labeled_adjusted"):
        cva.compute_retrieval_csls_device(torch.zeros(12, 8, device="cuda"), torch.zeros(12, 8))
    rq, rg, nv, met, _ = cva.retrieval_ranks_adjusted_device(q + 1, g + 1, lab, [0, 0, 1, 0, -1], [0, 0, 0])  # host numbers
    assert _host(torch, rq)[0].tolist() == [3, 3, 3] and _host(torch, rg)[0].tolist() == [0, -1, -1, -1, -1]
