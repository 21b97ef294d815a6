"""The tile route of the adjusted search (coot_retrieval_topk_adjusted_tile) against the slices (coot_retrieval_topk_adjusted) and against
the definition: both routes are forced through retrieval.ADJUSTED_TILE_MIN_M / ADJUSTED_TILE_MIN_M_16BIT, the similarities come back
with want_sim=True, and idx and scores of either route have to be, byte for byte, the host mirror compute_retrieval_topk_adjusted of
those bytes and each other's — whatever the storage, the mask, the offsets and the shares of the gallery; with offset = 0 they are
the bytes of GalleryIndex.search.
Shapes (N, d): (1000, 64) is eight 128-row blocks with a short last one; (130, 37) one block and two rows, a width that is no multiple
of the chunk; (5, 37) fewer rows than a block.  M = 1, 17, 63, 64, 65, 130: one query, a quarter of a row tile, one tile but one row,
a full tile, one row more, and three tiles with a short last one.  K = 1, 10 and 128 where N allows."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
SHAPES = [(1000, 64), (130, 37), (5, 37)]
MS = [1, 17, 63, 64, 65, 130]
NINF = np.float32(-np.inf)
MINUS_ROW = 2  # the row with offset -inf: none of 63, 64, 127, 128, N - 1 at any N used here


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def route(env, monkeypatch):
    """Forces the tile call ("tile") or the slices ("slices") through the two constants."""
    _, cva = env

    def set_(which):
        v = 1 if which == "tile" else cva.retrieval.ADJUSTED_TILE_NEVER
        monkeypatch.setattr(cva.retrieval, "ADJUSTED_TILE_MIN_M", v)
        monkeypatch.setattr(cva.retrieval, "ADJUSTED_TILE_MIN_M_16BIT", v)
    return set_


@pytest.fixture
def splits(env):
    """Sets rt_adjusted_tile_splits and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(s):
        assert lib.coot_set_option(b"rt_adjusted_tile_splits", s) == 0
    try:
        yield set_
    finally:
        set_(0)


def _index(torch, cva, storage, normalize, n, dim, seed=11):
    q, g = _planted(130, n, dim, seed)
    return torch.tensor(q, device="cuda"), cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=normalize, storage=getattr(torch, storage))


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _offsets(n, seed=5):
    """The three vectors: 0.1 randn; zeros; +inf at rows 63, 64, 127, 128 and N - 1 (those that exist) and -inf at MINUS_ROW."""
    small = (0.1 * np.random.RandomState(seed).randn(n)).astype(np.float32)
    special = small.copy()
    plus = sorted({r for r in (63, 64, 127, 128, n - 1) if r < n})
    special[plus] = np.inf
    assert MINUS_ROW not in plus
    special[MINUS_ROW] = -np.inf
    return {"small": small, "zero": np.zeros(n, np.float32), "special": special}


def _keeps(n, k):
    """None; random; one whole 128-row block masked (the first, or all but the last row where there is one block only); everything
    masked; fewer than K kept."""
    rs = np.random.RandomState(3)
    block = np.ones(n, bool)
    block[:min(128, n - 1)] = False
    few = np.zeros(n, bool)
    few[rs.permutation(n)[:max(1, k // 2)]] = True
    return {"none": None, "random": rs.rand(n) < 0.6, "block": block, "nothing": np.zeros(n, bool), "few": few}


def _assert_mirror(got, offset, k, keep=None):
    """idx and scores are the mirror of the returned similarities; the tail of a row with fewer than k kept rows is -1 / -inf."""
    from coot_videotext_amd import compute_retrieval_topk_adjusted
    idx, sc, sim = got
    want = compute_retrieval_topk_adjusted(sim, offset, k, keep=keep)
    assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (sim.shape[0], k)
    assert np.array_equal(idx, want[0]), np.argwhere(idx != want[0])[:5]
    assert bytes_equal(sc, want[1])
    filled = idx >= 0
    assert (sc[~filled] == NINF).all()
    if keep is not None:
        assert keep[idx[filled]].all()  # a masked row never appears
        assert (filled.sum(1) == min(k, int(keep.sum()))).all()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_both_routes_are_the_mirror_and_each_other(env, route, storage, normalize):
    torch, cva = env
    for n, dim in SHAPES:
        tq, index = _index(torch, cva, storage, normalize, n, dim)
        offsets = _offsets(n)
        plain = _host(torch, index.search(tq, 1, want_sim=True)[2])[0]
        for k in sorted({min(k, n) for k in (1, 10, 128)}):
            keeps = _keeps(n, k)
            for t, m in enumerate(MS):
                # every M with the random mask and the small offsets; the other masks and offsets rotate over the Ms
                combos = [("random", "small"), (list(keeps)[t % 5], "special"), (list(keeps)[(t + 2) % 5], "zero"), (list(keeps)[(t + 3) % 5], "small")]
                for kname, oname in combos:
                    kp, off = keeps[kname], offsets[oname]
                    tk, to = _dev(torch, kp), _dev(torch, off)
                    route("tile")
                    tile = _host(torch, *index.search_adjusted(tq[:m], k, to, keep=tk, want_sim=True))
                    bare = _host(torch, *index.search_adjusted(tq[:m], k, to, keep=tk)[:2])  # want_sim off: blocks may be skipped
                    route("slices")
                    slices = _host(torch, *index.search_adjusted(tq[:m], k, to, keep=tk, want_sim=True))
                    what = (n, k, m, kname, oname)
                    _assert_mirror(tile, off, k, kp)
                    assert bytes_equal(tile[2], plain[:m]), what
                    for a, b, c in zip(tile, slices, bare):
                        assert bytes_equal(a, b) and bytes_equal(a, c), what
                    assert bytes_equal(tile[2], slices[2]), what
                    if oname == "zero":  # against code that exists without this search
                        want = _host(torch, *index.search(tq[:m], k, keep=tk)[:2])
                        assert bytes_equal(tile[0], want[0]) and bytes_equal(tile[1], want[1]), what
                    if kname == "nothing":
                        assert (tile[0] == -1).all() and (tile[1] == NINF).all()
                    if oname == "special" and (kp is None or kp[MINUS_ROW]):  # offset -inf: the row comes first, with score +inf
                        assert (tile[0][:, 0] == MINUS_ROW).all() and (tile[1][:, 0] == np.float32(np.inf)).all()


def test_the_result_does_not_depend_on_the_shares(env, route, splits):
    """rt_adjusted_tile_splits = 1, 2, 3, the cap and automatic at N = 1 000 (8 blocks) and at 3 blocks: the same bytes."""
    torch, cva = env
    route("tile")
    for n, dim in ((1000, 64), (300, 37)):
        for storage in ("bfloat16", "float32"):
            tq, index = _index(torch, cva, storage, True, n, dim)
            keep = _dev(torch, np.random.RandomState(4).rand(n) < 0.7)
            for name, off in _offsets(n).items():
                to = _dev(torch, off)
                for m, k in ((130, 128), (17, 10), (65, 1)):
                    for kp in (None, keep):
                        runs = []
                        for s in (1, 2, 3, 32, 0):
                            splits(s)
                            runs.append(_host(torch, *index.search_adjusted(tq[:m], k, to, keep=kp, want_sim=(s == 2))[:2]))
                        for r in runs[1:]:
                            assert bytes_equal(r[0], runs[0][0]) and bytes_equal(r[1], runs[0][1]), (n, storage, name, m)
                        if name == "small" and kp is None and m == 130:  # and they are the definition, not only each other
                            splits(3)
                            _assert_mirror(_host(torch, *index.search_adjusted(tq[:m], k, to, want_sim=True)), off, k)


def test_a_query_does_not_depend_on_its_batch_mates(env, route):
    """Query 70 alone (a row tile with one row) and as row 70 of 130 (the second tile): the same bytes, on the slices too."""
    torch, cva = env
    n, dim, k = 1000, 64, 10
    tq, index = _index(torch, cva, "float16", True, n, dim)
    off = _dev(torch, _offsets(n)["small"])
    route("tile")
    alone = _host(torch, *index.search_adjusted(tq[70], k, off)[:2])
    whole = _host(torch, *index.search_adjusted(tq, k, off)[:2])
    route("slices")
    ref = _host(torch, *index.search_adjusted(tq[70], k, off)[:2])
    for a, w, r in zip(alone, whole, ref):
        assert bytes_equal(a, w[70:71]) and bytes_equal(a, r)


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_tile_route_on_a_mutated_index(env, route, storage):
    """After add, remove and compact: removed rows are never returned and combine with keep by AND; the function on the index's
    tensors gives the method's bytes; after compact the caller's offset[old rows] gives the bytes of a fresh index."""
    torch, cva = env
    route("tile")
    n, dim, k, m = 600, 64, 10, 65
    q, g = _planted(130, n, dim, 51)
    tq, tg = torch.tensor(q[:m], device="cuda"), torch.tensor(g, device="cuda")
    index = cva.GalleryIndex(tg[:500].contiguous(), normalize=True, storage=getattr(torch, storage))
    index.add(tg[500:])
    off = _offsets(n)["small"]
    to = _dev(torch, off)
    a = _host(torch, *index.search_adjusted(tq, k, to)[:2])
    b = _host(torch, *cva.retrieval_topk_adjusted_device(tq, index.gallery, index.norms, to, k)[:2])
    c = _host(torch, *cva.GalleryIndex(tg, normalize=True, storage=getattr(torch, storage)).search_adjusted(tq, k, to)[:2])
    assert bytes_equal(a[0], b[0]) and bytes_equal(a[1], b[1]) and bytes_equal(a[0], c[0]) and bytes_equal(a[1], c[1])
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


class _CCall:
    """coot_retrieval_topk_adjusted_tile through ctypes on buffers with a known fill."""

    def __init__(self, torch, cva, n, dim, m=70, k=128):
        self.lib, self.n, self.dim, self.m, self.k = cva.lib.load(), n, dim, m, k
        q, g = _planted(130, n, dim, 11)
        self.q, self.g = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        self.size = self.lib.coot_retrieval_topk_adjusted_tile_workspace_bytes(m, n, dim, k)
        self.ws = torch.zeros(self.size + 32, dtype=torch.uint8, device="cuda")
        self.idx = torch.full((m + 1, k + 1), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((m + 1, k + 1), -7.0, device="cuda")
        self.off = torch.zeros(n, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def __call__(self, m=None, k=None, dt=0, off=-1, ws_bytes=None, ws_off=0, idx=-1, d=None):
        return self.lib.coot_retrieval_topk_adjusted_tile(self.q.data_ptr(), self.g.data_ptr(), dt, None, None, self.off.data_ptr() if off == -1 else off,
                                                          self.m if m is None else m, self.n, self.dim if d is None else d, self.k if k is None else k,
                                                          self.idx.data_ptr() if idx == -1 else idx, self.sc.data_ptr(), None, self.ws.data_ptr() + ws_off,
                                                          self.size if ws_bytes is None else ws_bytes, self.st)


def test_refusals_write_nothing(env, splits):
    """Refused before any launch: the return code, the message, and every buffer as it was."""
    torch, cva = env
    splits(2)  # two shares: the workspace holds the lists too
    c = _CCall(torch, cva, 300, 16)
    cases = {"M = 0": (dict(m=0), "M = 0"), "row tiles": (dict(m=65535 * 64 + 1), "M = 4194241"), "d = 0": (dict(d=0), "d = 0"),
             "K = 0": (dict(k=0), "K = 0 is outside"), "K = 129": (dict(k=129), "K = 129 is outside"),
             "null offset": (dict(off=None), "null pointer"), "null output": (dict(idx=None), "null pointer"), "dtype": (dict(dt=7), "dtype = 7"),
             "one byte short": (dict(ws_bytes=c.size - 1), "workspace too small"), "misaligned": (dict(ws_off=8), "16-byte aligned")}
    for what, (kw, part) in cases.items():
        assert c(**kw) != 0, what
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_topk_adjusted_tile:" in msg and part in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((c.idx == -7).all()) and bool((c.sc == -7.0).all()) and not bool(c.ws.any()), what
    small = _CCall(torch, cva, 100, 16)
    assert small(k=101) != 0 and "K = 101 is outside 1 .. min(N = 100" in c.lib.coot_last_error().decode()
    assert c() == 0, c.lib.coot_last_error()  # the same buffers, accepted at exactly the layout's size
    torch.cuda.synchronize()
    flat = c.idx.view(-1)
    assert bool((flat[:70 * 128] >= 0).all()) and bool((flat[70 * 128:] == -7).all())
