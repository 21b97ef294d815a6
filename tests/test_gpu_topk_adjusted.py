"""The adjusted top-K search (coot_retrieval_topk_adjusted; retrieval_topk_adjusted_device, GalleryIndex.search_adjusted) and the
hubness offsets (coot_retrieval_hub_offsets; GalleryIndex.hubness_offsets) against their definitions.  The similarities come back with
want_sim=True and have to be the bytes of GalleryIndex.search's; idx and scores have to be, byte for byte, the host mirror
compute_retrieval_topk_adjusted of those bytes (tests/test_cpu_topk_adjusted.py checks the mirrors against a brute force) — whatever
the storage, the mask, the offsets and the sweep's row splits; with offset = 0 they are the bytes of GalleryIndex.search.  The offsets
are compute_retrieval_hub_offsets of GalleryIndex.knn_join's own output and of the mirror chain on the similarities.  Last, the
composition on a planted hub: the corrected search stops returning it.
Shapes (N, d): (1000, 64) is eight 128-row blocks with a short last one and 16-byte loads; (130, 37) one block and two rows, no
16-byte loads; (5, 37) fewer rows than lanes.  (M, K): one query; 3 (4 accumulators); 16 at K = 128; 17 and 33 cross the slices of
16.  K is clipped to N."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted, unit

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
SHAPES = [(1000, 64), (130, 37), (5, 37)]
MK = [(1, 1), (3, 10), (16, 128), (17, 10), (33, 128)]
PAIRS = [("float32", "float32"), ("bfloat16", "float32"), ("float16", "bfloat16")]
NINF = np.float32(-np.inf)
MINUS_ROW = 2  # the row with offset -inf: none of 0, 63, 64, 127, 128, N - 1 at any N used here


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def splits(env):
    """Sets rt_few_splits (the sweep) and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(few):
        assert lib.coot_set_option(b"rt_few_splits", few) == 0
    try:
        yield set_
    finally:
        set_(0)


def _index(torch, cva, storage, normalize, n, dim, seed=11):
    q, g = _planted(33, n, dim, seed)
    return torch.tensor(q, device="cuda"), cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=normalize, storage=getattr(torch, storage))


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _offsets(n, seed=5):
    """The three vectors: 0.1 randn; zeros; +inf at rows 0, 63, 64, 127, 128 and N - 1 (those that exist) and -inf at MINUS_ROW."""
    small = (0.1 * np.random.RandomState(seed).randn(n)).astype(np.float32)
    special = small.copy()
    plus = sorted({r for r in (0, 63, 64, 127, 128, n - 1) if r < n})
    special[plus] = np.inf
    assert MINUS_ROW not in plus
    special[MINUS_ROW] = -np.inf
    return {"small": small, "zero": np.zeros(n, np.float32), "special": special}


def _assert_mirror(got, offset, k, keep=None):
    """idx and scores are the mirror of the returned similarities; the scores are sim - offset, one float32 subtraction, at idx."""
    from coot_videotext_amd import compute_retrieval_topk_adjusted
    idx, sc, sim = got
    want = compute_retrieval_topk_adjusted(sim, offset, k, keep=keep)
    assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (sim.shape[0], k)
    assert np.array_equal(idx, want[0]), np.argwhere(idx != want[0])[:5]
    assert bytes_equal(sc, want[1])
    filled = idx >= 0
    rows = np.nonzero(filled)[0]
    assert bytes_equal(sc[filled], (sim[rows, idx[filled]] - offset[idx[filled]]).astype(np.float32))
    assert (sc[~filled] == NINF).all()
    if keep is not None:
        assert keep[idx[filled]].all()  # a masked row never appears
        assert (filled.sum(1) == min(k, int(keep.sum()))).all()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_adjusted_search_is_the_mirror_of_its_similarities(env, storage, normalize):
    torch, cva = env
    case = 0
    for n, dim in SHAPES:
        tq, index = _index(torch, cva, storage, normalize, n, dim)
        keep = np.random.RandomState(3).rand(n) < 0.6
        offsets = _offsets(n)
        plain = {}
        for m, k in MK:
            k = min(k, n)
            if m not in plain:  # the similarities of the plain search, once per M
                plain[m] = _host(torch, index.search(tq[:m], 1, want_sim=True)[2])[0]
            for kp in (None, keep):
                tk = _dev(torch, kp)
                for name, off in offsets.items():
                    case += 1
                    to = off.tolist() if case % 5 == 0 else off if case % 7 == 0 else _dev(torch, off)  # a host list, a host array, the device
                    got = _host(torch, *index.search_adjusted(tq[:m], k, to, keep=tk, want_sim=True))
                    _assert_mirror(got, off, k, kp)
                    assert bytes_equal(got[2], plain[m]), (n, m, k, name)
                    if name == "zero":  # against code that exists without this search
                        want = _host(torch, *index.search(tq[:m], k, keep=tk)[:2])
                        assert bytes_equal(got[0], want[0]) and bytes_equal(got[1], want[1]), (n, m, k)
                    if name == "special":
                        ok = np.ones(n, bool) if kp is None else kp
                        if ok[MINUS_ROW]:  # offset -inf: the row comes first, with score +inf
                            assert (got[0][:, 0] == MINUS_ROW).all() and (got[1][:, 0] == np.float32(np.inf)).all()
                        plus = np.nonzero(np.isposinf(off) & ok)[0]
                        finite = int(ok.sum()) - len(plus)
                        if k > finite:  # the +inf rows are rows still: score -inf under their own index, the larger row first
                            c = min(k - finite, len(plus))
                            assert (got[0][:, finite:finite + c] == plus[::-1][:c]).all() and (got[1][:, finite:finite + c] == NINF).all()
                            assert (got[0][:, finite + c:] == -1).all()


def test_the_result_does_not_depend_on_the_row_splits(env, splits):
    torch, cva = env
    n, dim = 1000, 64
    for storage in ("bfloat16", "float32"):
        tq, index = _index(torch, cva, storage, True, n, dim)
        keep = _dev(torch, np.random.RandomState(4).rand(n) < 0.7)
        for name, off in _offsets(n).items():
            to = _dev(torch, off)
            for m, k in ((16, 128), (3, 10), (33, 10)):
                for kp in (None, keep):
                    runs = []
                    for s in (1, 3, 0):
                        splits(s)
                        runs.append(_host(torch, *index.search_adjusted(tq[:m], k, to, keep=kp)[:2]))
                        runs.append(_host(torch, *index.search_adjusted(tq[:m], k, to, keep=kp, want_sim=True)[:2]))
                    for r in runs[1:]:
                        assert bytes_equal(r[0], runs[0][0]) and bytes_equal(r[1], runs[0][1]), (storage, name, m)


def test_a_query_does_not_depend_on_its_batch_mates(env):
    """Query 20 alone, in a batch of 16 and in the second slice of 33: the same bytes."""
    torch, cva = env
    n, dim, k = 1000, 64, 10
    tq, index = _index(torch, cva, "float16", True, n, dim)
    off = _dev(torch, _offsets(n)["small"])
    alone = _host(torch, *index.search_adjusted(tq[20], k, off)[:2])
    batch = _host(torch, *index.search_adjusted(tq[12:28], k, off)[:2])
    whole = _host(torch, *index.search_adjusted(tq, k, off)[:2])
    for a, b, w in zip(alone, batch, whole):
        assert bytes_equal(a, b[8:9]) and bytes_equal(a, w[20:21])


def test_blocks_without_a_kept_row_are_skipped_with_the_same_result(env, splits):
    """keep leaves rows of the first and of the last of eight blocks only: the sweep without sim leaves the six between them before
    their first load, with sim every block is computed.  The same idx and scores, on one workgroup and on the automatic splits."""
    torch, cva = env
    n, dim, k, m = 1000, 64, 10, 16
    tq, index = _index(torch, cva, "float16", True, n, dim)
    keep = np.zeros(n, bool)
    keep[3:40] = keep[990:] = True
    off = _offsets(n)["small"]
    for s in (1, 0):
        splits(s)
        skipping = _host(torch, *index.search_adjusted(tq[:m], k, _dev(torch, off), keep=_dev(torch, keep))[:2])
        full = _host(torch, *index.search_adjusted(tq[:m], k, _dev(torch, off), keep=_dev(torch, keep), want_sim=True))
        _assert_mirror(full, off, k, keep)
        assert bytes_equal(skipping[0], full[0]) and bytes_equal(skipping[1], full[1])
        idx, sc = _host(torch, *index.search_adjusted(tq, k, _dev(torch, off), keep=_dev(torch, np.zeros(n, bool)))[:2])  # nothing kept
        assert idx.shape == (33, k) and (idx == -1).all() and (sc == NINF).all()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_adjusted_search_on_a_mutated_index(env, storage):
    """Removed rows are never returned and combine with keep by AND; the function on the index's tensors gives the method's bytes;
    after compact the caller's offset[old rows] gives the bytes of a fresh index."""
    torch, cva = env
    n, dim, k, m = 600, 64, 10, 17
    q, g = _planted(33, n, dim, 51)
    tq, tg = torch.tensor(q[:m], device="cuda"), torch.tensor(g, device="cuda")
    index = cva.GalleryIndex(tg, normalize=True, storage=getattr(torch, storage))
    off = _offsets(n)["small"]
    to = _dev(torch, off)
    a = _host(torch, *index.search_adjusted(tq, k, to)[:2])
    b = _host(torch, *cva.retrieval_topk_adjusted_device(tq, index.gallery, index.norms, to, k)[:2])
    assert bytes_equal(a[0], b[0]) and bytes_equal(a[1], b[1])
    gone = np.arange(0, n, 4)
    index.remove(gone.tolist())
    kept = np.ones(n, bool)
    kept[gone] = False
    user = np.random.RandomState(6).rand(n) < 0.8
    _assert_mirror(_host(torch, *index.search_adjusted(tq, k, to, want_sim=True)), off, k, kept)
    _assert_mirror(_host(torch, *index.search_adjusted(tq, k, to, keep=_dev(torch, user), want_sim=True)), off, k, kept & user)
    removed = index.search_adjusted(tq, k, to)
    old = index.compact().to(torch.int64)
    fresh = cva.GalleryIndex(tg[old].contiguous(), normalize=True, storage=getattr(torch, storage))
    got = index.search_adjusted(tq, k, to[old])
    want = fresh.search_adjusted(tq, k, to[old])
    back = old[got[0].to(torch.int64)].to(torch.int32)  # in the old numbering: the search that skipped the removed rows
    for x, y in zip(_host(torch, got[0], got[1], back, got[1]), _host(torch, want[0], want[1], removed[0], removed[1])):
        assert bytes_equal(x, y)


def _hub_case(torch, cva, n, dim, b, left, right, seed):
    _, g = _planted(33, n, dim, 11)
    rs = np.random.RandomState(seed)
    bank = (0.5 * g[rs.randint(0, n, size=b)] + rs.randn(b, dim)).astype(np.float32)
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=True, storage=getattr(torch, left))
    bank_index = cva.GalleryIndex(torch.tensor(bank, device="cuda"), normalize=True, storage=getattr(torch, right))
    return index, bank_index


@pytest.mark.parametrize("left,right", PAIRS)
def test_hubness_offsets_are_the_mirror_of_the_knn_join(env, left, right):
    torch, cva = env
    from coot_videotext_amd import compute_retrieval_hub_offsets, compute_retrieval_knn_join
    for n, dim in ((130, 37), (1000, 64)):
        for b in (33, 200):
            index, bank = _hub_case(torch, cva, n, dim, b, left, right, seed=n + b)
            sim = _host(torch, bank.search(index.gallery.float(), 1, want_sim=True)[2])[0]  # [N, B]
            rs = np.random.RandomState(b)
            keep, other = rs.rand(n) < 0.7, rs.rand(b) < 0.5
            for k in (1, 10, min(b, 128)):
                for kp, okp in ((None, None), (keep, other), (None, np.zeros(b, bool))):
                    kw = dict(keep=_dev(torch, kp), other_keep=_dev(torch, okp))
                    got = _host(torch, index.hubness_offsets(bank, k, **kw))[0]
                    assert got.dtype == np.float32 and got.shape == (n,)
                    jidx, jsc = _host(torch, *index.knn_join(bank, k, **kw))
                    assert bytes_equal(got, compute_retrieval_hub_offsets(jsc, jidx)), (n, b, k)
                    midx, msc = compute_retrieval_knn_join(sim, k, keep=kp, other_keep=okp)
                    assert bytes_equal(got, compute_retrieval_hub_offsets(msc, midx)), (n, b, k)
                    if kp is not None:
                        assert (got[~kp] == 0).all() and got[kp].any()
                    if okp is not None and not okp.any():
                        assert (got == 0).all()
            index.remove([1, 5])  # the index's own filter masks a row as keep does
            got = _host(torch, index.hubness_offsets(bank))[0]
            assert got[1] == 0 and got[5] == 0 and got[0] != 0
            assert bytes_equal(got, compute_retrieval_hub_offsets(*_host(torch, *index.knn_join(bank, 10))[::-1]))


def planted_hub(seed=0, n=300, d=32, m=200):
    """The recipe of the planted hub: row n - 1 is the common direction c that every query and every bank row leans towards."""
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
    """search_adjusted(q, 1, index.hubness_offsets(bank, 10)) against search(q, 1): the hub is top-1 for at most a fifth as many
    queries, and R@1 rises by at least 0.1.  (A numpy restatement gives 53 - 63 -> 1 - 4 and 0.635 - 0.67 -> 0.955 - 0.97.)"""
    torch, cva = env
    g, q, bank, lab = planted_hub(0)
    n = len(g)
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=True)
    bank_index = cva.GalleryIndex(torch.tensor(bank, device="cuda"), normalize=True)
    tq = torch.tensor(q, device="cuda")
    raw = _host(torch, index.search(tq, 1)[0])[0][:, 0]
    off = index.hubness_offsets(bank_index, 10)
    assert off.is_cuda and off.dtype == torch.float32 and tuple(off.shape) == (n,)
    cor = _host(torch, index.search_adjusted(tq, 1, off)[0])[0][:, 0]
    hub_raw, hub_cor = int((raw == n - 1).sum()), int((cor == n - 1).sum())
    r1_raw, r1_cor = float((raw == lab).mean()), float((cor == lab).mean())
    print(f"hub top-1: {hub_raw} -> {hub_cor}; R@1: {r1_raw:.3f} -> {r1_cor:.3f}")
    assert hub_raw > 0 and 5 * hub_cor <= hub_raw, (hub_raw, hub_cor)
    assert r1_cor >= r1_raw + 0.1, (r1_raw, r1_cor)


class _CCall:
    """coot_retrieval_topk_adjusted through ctypes on buffers with a known fill."""

    def __init__(self, torch, cva, n, dim):
        self.lib, self.n, self.dim = cva.lib.load(), n, dim
        q, g = _planted(33, n, dim, 11)
        self.q, self.g = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        self.size = self.lib.coot_retrieval_topk_adjusted_workspace_bytes(16, n, dim, 128)
        self.ws = torch.zeros(self.size, dtype=torch.uint8, device="cuda")
        self.idx = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((17, 129), -7.0, device="cuda")
        self.off = torch.zeros(n, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def __call__(self, m=16, k=128, dt=0, off=-1, ws_bytes=None, ws_off=0, idx=-1):
        return self.lib.coot_retrieval_topk_adjusted(self.q.data_ptr(), self.g.data_ptr(), dt, None, None, self.off.data_ptr() if off == -1 else off, m,
                                                     self.n, self.dim, k, self.idx.data_ptr() if idx == -1 else idx, self.sc.data_ptr(), None,
                                                     self.ws.data_ptr() + ws_off, (self.size if ws_bytes is None else ws_bytes) - ws_off, self.st)


def test_adjusted_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message, and every buffer as it was."""
    torch, cva = env
    n, dim = 300, 16
    c = _CCall(torch, cva, n, dim)
    exact = c.size - 256  # the layout itself: the reported size has one piece of slack
    cases = {"M = 17": (dict(m=17), "M = 17"), "M = 0": (dict(m=0), "M = 0"), "K = 0": (dict(k=0), "K = 0 is outside"),
             "K > N": (None, "K = 101 is outside 1 .. min(N = 100"), "K = 129": (dict(k=129), "K = 129 is outside"),
             "null offset": (dict(off=None), "null pointer"), "null output": (dict(idx=None), "null pointer"), "dtype": (dict(dt=7), "dtype = 7"),
             "one byte short": (dict(ws_bytes=exact - 1), "workspace too small"), "misaligned": (dict(ws_off=8), "16-byte aligned")}
    for what, (kw, part) in cases.items():
        if what == "K > N":
            small = _CCall(torch, cva, 100, dim)
            assert small(k=101, m=1) != 0, what
        else:
            assert c(**kw) != 0, what
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_topk_adjusted:" in msg and part in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((c.idx == -7).all()) and bool((c.sc == -7.0).all()) and not bool(c.ws.any()), what
    assert c(ws_bytes=exact) == 0, c.lib.coot_last_error()  # the same buffers, accepted at exactly the layout's size
    torch.cuda.synchronize()
    assert bool((c.idx.view(-1)[:16 * 128] >= 0).all()) and bool((c.idx.view(-1)[16 * 128:] == -7).all())
    out = torch.full((4,), -7.0, device="cuda")
    for args, part in (((None, c.idx.data_ptr(), 4, 2, out.data_ptr()), "null pointer"), ((c.sc.data_ptr(), c.idx.data_ptr(), 0, 2, out.data_ptr()), "N = 0"),
                       ((c.sc.data_ptr(), c.idx.data_ptr(), 4, 129, out.data_ptr()), "K = 129")):
        assert c.lib.coot_retrieval_hub_offsets(*args, c.st) != 0
        assert "retrieval_hub_offsets:" in c.lib.coot_last_error().decode() and part in c.lib.coot_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_arguments_are_refused_on_the_host(env):
    """What needs a device to get as far as the check: k and the width under the new names, an offset on the device of the wrong type
    or shape, a keep that is not on the device, and the bank's checks under hubness_offsets' name."""
    torch, cva = env
    g = torch.zeros(5, 8, device="cuda")
    index = cva.GalleryIndex(g, normalize=False)
    zero = torch.zeros(5, device="cuda")
    q = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError, match=r"GalleryIndex.search_adjusted: queries of width 7, gallery of width 8"):
        index.search_adjusted(torch.zeros(2, 7, device="cuda"), 2, zero)
    with pytest.raises(ValueError, match=r"retrieval_topk_adjusted_device: queries of width 7, gallery of width 8"):
        cva.retrieval_topk_adjusted_device(torch.zeros(2, 7, device="cuda"), g, None, zero, 2)
    for k in (0, 6, 129):
        with pytest.raises(ValueError, match=rf"GalleryIndex.search_adjusted: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            index.search_adjusted(q, k, zero)
        with pytest.raises(ValueError, match=rf"retrieval_topk_adjusted_device: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            cva.retrieval_topk_adjusted_device(q, g, None, zero, k)
    with pytest.raises(ValueError, match=r"GalleryIndex.search_adjusted: offset of shape \(4,\), a gallery of 5 rows"):
        index.search_adjusted(q, 2, zero[:4])
    with pytest.raises(ValueError, match="GalleryIndex.search_adjusted: offset on the device has to be torch.float32, not torch.float64"):
        index.search_adjusted(q, 2, zero.double())
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_adjusted"):
        index.search_adjusted(q, 2, zero, keep=torch.ones(5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_adjusted"):
        index.search_adjusted(q.cpu(), 2, zero)
    bank = cva.GalleryIndex(torch.zeros(3, 8, device="cuda") + 1, normalize=False)
    for k in (0, 4, 129):
        with pytest.raises(ValueError, match=rf"GalleryIndex.hubness_offsets: k = {k} is outside 1 .. min\(N_right = 3, 128\)"):
            index.hubness_offsets(bank, k)
    with pytest.raises(ValueError, match="GalleryIndex.hubness_offsets: this index has normalize=False, the right one normalize=True"):
        index.hubness_offsets(cva.GalleryIndex(torch.ones(3, 8, device="cuda")))
    # one query as [d]; host numbers; the default k = 10 needs a bank of ten rows
    idx, sc, _ = index.search_adjusted(q[0], 2, [0, 0, 1, 0, -1])
    assert _host(torch, idx, sc)[0].tolist() == [[4, 3]] and _host(torch, sc)[0].tolist() == [[1.0, 0.0]]
    assert _host(torch, index.hubness_offsets(bank, 3))[0].tolist() == [0.0] * 5  # (zero rows: every similarity is 0)
