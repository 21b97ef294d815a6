"""The tile route of the range search (coot_retrieval_range_tile_count, _fill; retrieval.RANGE_TILE_MIN_M, RANGE_TILE_MIN_M_16BIT)
against the definition and against the sweep's slices of 16: the reference similarities are those that index.search(q, 1,
want_sim=True) returns, and (offsets, rows, scores) have to be, byte for byte, the host mirror compute_retrieval_range of those bytes on
BOTH routes, which a test selects by setting the two constants to 1 (tile) or to 10^9 (slices).
Shapes (N, d): (1000, 64) is eight 128-row blocks, the last one 104 rows, so its second tile is short; (192, 64): the second block is
exactly one tile; (130, 37): block 1 has two rows, no 16-byte loads, d no multiple of 32; (5, 37): fewer rows than a tile.
M: 1, 17, 63, 64, 65, 130: inside, at and across the edges of the 64-query row tiles.
The thresholds are taken from the reference bytes, so that scores sit exactly on them."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
SHAPES = [(1000, 64), (192, 64), (130, 37), (5, 37)]
MS = [1, 17, 63, 64, 65, 130]
MQ = 130
KINDS = ["-inf", "+inf", "nan", "max", "median", "between"]
TILE, SLICES = 1, 10 ** 9
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def route(env, monkeypatch):
    """Sets both routing constants: route(TILE) sends every search to the tile calls, route(SLICES) to the sweep's slices."""
    _, cva = env

    def set_(v):
        monkeypatch.setattr(cva.retrieval, "RANGE_TILE_MIN_M", v)
        monkeypatch.setattr(cva.retrieval, "RANGE_TILE_MIN_M_16BIT", v)
    return set_


_CASES = {}


def _case(torch, cva, storage, normalize, n, dim, seed=11):
    """(queries [130, d] on the device, the index, the reference similarities [130, N] on the host): made once and shared, read only."""
    key = (storage, normalize, n, dim, seed)
    if key not in _CASES:
        q, g = _planted(MQ, n, dim, seed)
        tq = torch.tensor(q, device="cuda")
        index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=normalize, storage=getattr(torch, storage))
        sim = _host(torch, index.search(tq, 1, want_sim=True)[2])[0]
        assert sim.shape == (MQ, n) and not np.isnan(sim).any()
        sim.setflags(write=False)
        _CASES[key] = (tq, index, sim)
    return _CASES[key]


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _threshold(row, kind):
    """One threshold from a query's reference similarities (float32 [N], no NaN among them)."""
    s = np.sort(row)
    if kind == "-inf":
        return np.float32(-np.inf)
    if kind == "+inf":
        return np.float32(np.inf)
    if kind == "nan":
        return np.float32(np.nan)
    if kind == "max":
        return s[-1]  # the >= boundary on the query's best row
    if kind == "median":
        return s[len(s) // 2]  # an exact score: that row and every row above it
    t = np.float32((np.float64(s[-1]) + np.float64(s[-2])) / 2)
    return t if s[-2] < t < s[-1] else s[-1]


def _thresholds(sim, shift=0):
    return np.array([_threshold(sim[i], KINDS[(i + shift) % len(KINDS)]) for i in range(sim.shape[0])], np.float32)


def _assert_mirror(got, sim, thr, keep=None, order="row"):
    from coot_videotext_amd import compute_retrieval_range
    want = compute_retrieval_range(sim, thr, keep=keep, order=order)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert bytes_equal(got[0], want[0]), (got[0], want[0])
    assert bytes_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert bytes_equal(got[2], want[2])
    return want


def _same(a, b):
    return all(bytes_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_both_routes_are_the_mirror_of_the_reference_similarities(env, route, storage, normalize):
    torch, cva = env
    case = 0
    for n, dim in SHAPES:
        tq, index, ref = _case(torch, cva, storage, normalize, n, dim)
        keep = np.random.RandomState(3).rand(n) < 0.6
        for m in MS:
            sim = ref[:m]
            thr = _thresholds(sim, shift=m)
            case += 1
            kp = (None, keep)[case % 2]
            tt = [thr.tolist(), thr, _dev(torch, thr)][case % 3]  # a host list (doubles that round back), a host array, a device tensor
            got = {}
            for r in (TILE, SLICES):
                route(r)
                got[r] = _host(torch, *index.search_range(tq[:m], tt, keep=_dev(torch, kp)))
                want = _assert_mirror(got[r], sim, thr, kp)
                by_score = _host(torch, *index.search_range(tq[:m], _dev(torch, thr), keep=_dev(torch, kp), order="score"))
                _assert_mirror(by_score, sim, thr, kp, order="score")
                counts = _host(torch, index.count_range(tq[:m], tt, keep=_dev(torch, kp)))[0]
                assert counts.dtype == np.int32 and np.array_equal(counts, np.diff(want[0]))
            assert _same(got[TILE], got[SLICES]), (n, dim, m)
            cnt = np.diff(got[TILE][0])
            kept_n = n if kp is None else int(kp.sum())
            for i in range(m):  # what the thresholds are there for
                kind = KINDS[(i + m) % len(KINDS)]
                if kind == "-inf":
                    assert cnt[i] == kept_n
                elif kind in ("+inf", "nan"):
                    assert cnt[i] == 0
                elif kp is None and kind == "median":
                    assert cnt[i] >= n - n // 2
                elif kp is None:
                    assert cnt[i] >= 1
            route(TILE)
            scalar = float(np.sort(sim[0])[n // 2])  # one number for every query: exactly a score of query 0
            _assert_mirror(_host(torch, *cva.retrieval_range_device(tq[:m], index.gallery, index.norms, scalar, keep=_dev(torch, keep))), sim, scalar, keep)


class _Tile:
    """The library calls through ctypes on buffers with a known fill: m queries, a gallery as the index holds it."""

    def __init__(self, torch, cva, tq, index, m, room, keep=None):
        self.torch, self.lib, self.m = torch, cva.lib.load(), m
        self.q, self.g, self.norms, self.keep = tq[:m].contiguous(), index.gallery, index.norms if index.normalize else None, keep
        self.code = {torch.float32: 0, torch.bfloat16: cva.retrieval.GALLERY_BF16, torch.float16: cva.retrieval.GALLERY_F16}[index.gallery.dtype]
        self.n, self.dim = index.gallery.shape
        self.size = self.lib.coot_retrieval_range_tile_workspace_bytes(m, self.n, self.dim)
        self.ws = torch.zeros(self.size, dtype=torch.uint8, device="cuda")
        self.nb = (self.n + 127) // 128
        self.table = torch.full((m, self.nb + 1), -7, dtype=torch.int32, device="cuda")
        self.off = torch.full((m + 1,), -7, dtype=torch.int64, device="cuda")
        self.rows = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((room,), -7.0, device="cuda")
        self.thr = torch.zeros(m, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def _p(self, t):
        return None if t is None else t.data_ptr()

    def count(self, m=None, dt=None, q=-1, table=-1, thr=-1, ws=-1, ws_bytes=None, ws_off=0, n=None, d=None):
        return self.lib.coot_retrieval_range_tile_count(self.q.data_ptr() if q == -1 else q, self.g.data_ptr(), self.code if dt is None else dt,
                                                        self._p(self.norms), self._p(self.keep), self.thr.data_ptr() if thr == -1 else thr,
                                                        self.m if m is None else m, self.n if n is None else n, self.dim if d is None else d,
                                                        self.table.data_ptr() if table == -1 else table, (self.ws.data_ptr() + ws_off) if ws == -1 else ws,
                                                        (self.size if ws_bytes is None else ws_bytes) - ws_off, self.st)

    def sweep_count(self, table):
        """coot_retrieval_range_count in slices of 16 on the rows of `table`."""
        ws = self.torch.empty(self.lib.coot_retrieval_range_workspace_bytes(16, self.n, self.dim), dtype=self.torch.uint8, device="cuda")
        for i in range(0, self.m, 16):
            assert self.lib.coot_retrieval_range_count(self.q[i:].data_ptr(), self.g.data_ptr(), self.code, self._p(self.norms), self._p(self.keep),
                                                       self.thr[i:].data_ptr(), min(16, self.m - i), self.n, self.dim, table[i:].data_ptr(), ws.data_ptr(),
                                                       ws.numel(), self.st) == 0, self.lib.coot_last_error()

    def scan(self):
        return self.lib.coot_retrieval_range_scan(self.table.data_ptr(), self.m, self.n, self.off.data_ptr(), None, self.st)

    def fill(self, capacity, m=None, dt=None, rows=-1, sc=-1, off=-1, table=-1, ws_bytes=None, ws_off=0, n=None, d=None):
        return self.lib.coot_retrieval_range_tile_fill(self.q.data_ptr(), self.g.data_ptr(), self.code if dt is None else dt, self._p(self.norms),
                                                       self._p(self.keep), self.thr.data_ptr(), self.m if m is None else m, self.n if n is None else n,
                                                       self.dim if d is None else d, self.table.data_ptr() if table == -1 else table,
                                                       self.off.data_ptr() if off == -1 else off, capacity, self.rows.data_ptr() if rows == -1 else rows,
                                                       self.sc.data_ptr() if sc == -1 else sc, self.ws.data_ptr() + ws_off,
                                                       (self.size if ws_bytes is None else ws_bytes) - ws_off, self.st)

    def untouched(self):
        self.torch.cuda.synchronize()
        return (bool((self.table == -7).all()) and bool((self.off == -7).all()) and bool((self.rows == -7).all()) and bool((self.sc == -7.0).all())
                and not bool(self.ws.any()))


@pytest.mark.parametrize("storage,normalize", [("float32", False), ("float32", True), ("bfloat16", True), ("float16", False)])
def test_the_count_call_writes_the_table_of_the_sweep(env, storage, normalize):
    """Slot for slot: after coot_retrieval_range_tile_count the slots [i][0 .. nb) of a sentinel-filled table are the bytes that
    coot_retrieval_range_count writes for the same queries in slices of 16, and slot nb, the scan's, still holds the sentinel."""
    torch, cva = env
    for n, dim in SHAPES:
        tq, index, ref = _case(torch, cva, storage, normalize, n, dim)
        masks = [None, _dev(torch, (np.random.RandomState(5).rand(n) < 0.5).astype(np.uint8))]
        if n == 1000:
            hollow = np.zeros(n, np.uint8)
            hollow[5:120:3] = 1
            hollow[900:] = 1
            masks.append(_dev(torch, hollow))
        for m in (65, 130):
            for keep in masks:
                c = _Tile(torch, cva, tq, index, m, room=1, keep=keep)
                c.thr.copy_(torch.from_numpy(_thresholds(ref[:m], shift=1)))
                assert c.count() == 0, c.lib.coot_last_error()
                want = torch.full_like(c.table, -7)
                c.sweep_count(want)
                got, want = _host(torch, c.table, want)
                assert (want[:, :c.nb] >= 0).all() and (keep is not None or want[:, :c.nb].sum() > 0)
                assert bytes_equal(got, want), (n, m, np.argwhere(got != want)[:5])
                assert (got[:, c.nb] == -7).all()


def test_keep_the_own_filter_and_blocks_that_are_left_out(env, route):
    """A random mask; a mask that empties six of the eight blocks (the count pass leaves them before their first load); index.remove
    combined with keep; a threshold with hits in one block only per query (the fill pass leaves the others): the mirror's bytes."""
    torch, cva = env
    n, dim = 1000, 64
    for storage, m in (("float16", 130), ("float32", 65)):
        tq, index, ref = _case(torch, cva, storage, True, n, dim)
        sim = ref[:m]
        thr = _thresholds(sim, shift=0)
        rnd = np.random.RandomState(4).rand(n) < 0.7
        hollow = np.zeros(n, bool)
        hollow[5:120:3] = True
        hollow[900:] = True
        gone = np.arange(1, n, 3)
        kept = np.ones(n, bool)
        kept[gone] = False
        top = sim.max(axis=1)
        for r in (TILE, SLICES):
            route(r)
            for kp in (rnd, hollow, rnd.astype(np.uint8) * 3):
                _assert_mirror(_host(torch, *index.search_range(tq[:m], thr, keep=_dev(torch, kp))), sim, thr, kp.astype(bool))
            got = _host(torch, *index.search_range(tq[:m], top))
            _assert_mirror(got, sim, top)
            assert (np.diff(got[0]) >= 1).all() and all(int(sim[i].argmax()) in got[1][got[0][i]:got[0][i + 1]] for i in range(m))
            try:
                index.remove(gone.tolist())
                _assert_mirror(_host(torch, *index.search_range(tq[:m], thr)), sim, thr, kept)
                _assert_mirror(_host(torch, *index.search_range(tq[:m], thr, keep=_dev(torch, rnd), order="score")), sim, thr, kept & rnd, order="score")
                assert np.array_equal(_host(torch, index.count_range(tq[:m], thr, keep=_dev(torch, hollow)))[0],
                                      np.diff(cva.compute_retrieval_range(sim, thr, keep=kept & hollow)[0]))
            finally:
                index.restore()


def test_the_fill_call_writes_nothing_at_or_beyond_the_capacity(env, route):
    """The library call itself, on buffers larger than the capacity that hold a sentinel: the entries below min(T, capacity) are the
    result's, everything else still holds the sentinel.  And max_results cuts the wrapper's result and leaves the offsets exact."""
    torch, cva = env
    n, dim, m = 1000, 64, 130
    tq, index, ref = _case(torch, cva, "bfloat16", True, n, dim)
    thr = _thresholds(ref, shift=4)
    want = cva.compute_retrieval_range(ref, thr)
    off, rows, sc = want
    t = int(off[m])
    assert t > 1000
    for cap in (0, 1, t // 2, t, t + 5):
        c = _Tile(torch, cva, tq, index, m, room=t + 64)
        c.thr.copy_(torch.from_numpy(thr))
        assert c.count() == 0 and c.scan() == 0 and c.fill(cap) == 0, c.lib.coot_last_error()
        got_off, got_rows, got_sc = _host(torch, c.off, c.rows, c.sc)
        assert bytes_equal(got_off, off)
        u = min(t, cap)
        assert bytes_equal(got_rows[:u], rows[:u]) and bytes_equal(got_sc[:u], sc[:u]), cap
        assert (got_rows[u:] == -7).all() and (got_sc[u:] == -7.0).all(), cap
    route(TILE)
    i = next(i for i in range(m // 2, m) if off[i + 1] - off[i] >= 3)
    inside = int(off[i] + (off[i + 1] - off[i]) // 2)  # cuts inside a segment
    assert off[i] < inside < off[i + 1] - 1
    for c in (1, t // 2, inside, t, t + 5):
        got = _host(torch, *index.search_range(tq, _dev(torch, thr), max_results=c))
        assert got[1].shape == got[2].shape == (c,) and bytes_equal(got[0], off)
        u = min(t, c)
        assert bytes_equal(got[1][:u], rows[:u]) and bytes_equal(got[2][:u], sc[:u])
        assert (got[1][u:] == -1).all() and (got[2][u:] == NINF).all()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_a_query_does_not_depend_on_its_batch_mates_or_its_row_tile(env, route, storage):
    """Query i alone (M = 1 through the tile calls, row 0 of tile 0) against its segment in M = 130 (row i mod 64 of tile i / 64); and
    two runs of the same search are the same bytes."""
    torch, cva = env
    n, dim = 1000, 64
    tq, index, ref = _case(torch, cva, storage, True, n, dim)
    tt = _dev(torch, _thresholds(ref, shift=3))
    keep = _dev(torch, np.random.RandomState(4).rand(n) < 0.7)
    route(TILE)
    for kp in (None, keep):
        whole = _host(torch, *index.search_range(tq, tt, keep=kp))
        again = _host(torch, *index.search_range(tq, tt, keep=kp))
        assert _same(whole, again)
        off = whole[0]
        for i in list(range(0, MQ, 7)) + [63, 64, 65, 127, 128, 129]:
            one = _host(torch, *index.search_range(tq[i:i + 1], tt[i:i + 1], keep=kp))
            assert one[0].tolist() == [0, off[i + 1] - off[i]]
            assert bytes_equal(one[1], whole[1][off[i]:off[i + 1]]) and bytes_equal(one[2], whole[2][off[i]:off[i + 1]]), i


def test_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message naming the entry, and every buffer as it was."""
    torch, cva = env
    n, dim, m = 300, 16, 70
    q, g = _planted(m, n, dim, 11)
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=True)
    c = _Tile(torch, cva, torch.tensor(q, device="cuda"), index, m, room=64)
    exact = c.size - 256  # the layout itself: the reported size has one piece of slack
    big = 65535 * 64 + 1
    cases = [("count", dict(m=0), "M = 0"), ("count", dict(m=big), "M = %d" % big), ("count", dict(n=0), "N = 0"), ("count", dict(d=0), "d = 0"),
             ("count", dict(q=None), "null pointer"), ("count", dict(table=None), "null pointer"), ("count", dict(thr=None), "null pointer"),
             ("count", dict(ws=None), "null pointer"), ("count", dict(dt=7), "dtype = 7"), ("count", dict(ws_bytes=exact - 1), "workspace too small"),
             ("count", dict(ws_off=8), "16-byte aligned"),
             ("fill", dict(capacity=-1), "capacity = -1"), ("fill", dict(capacity=8, m=0), "M = 0"), ("fill", dict(capacity=8, m=big), "M = %d" % big),
             ("fill", dict(capacity=8, n=0), "N = 0"), ("fill", dict(capacity=8, d=0), "d = 0"), ("fill", dict(capacity=8, rows=None), "null pointer"),
             ("fill", dict(capacity=8, sc=None), "null pointer"), ("fill", dict(capacity=8, off=None), "null pointer"),
             ("fill", dict(capacity=8, table=None), "null pointer"), ("fill", dict(capacity=8, dt=-1), "dtype = -1"),
             ("fill", dict(capacity=8, ws_bytes=exact - 1), "workspace too small"), ("fill", dict(capacity=8, ws_off=8), "16-byte aligned")]
    for which, kw, part in cases:
        assert getattr(c, which)(**kw) != 0, (which, kw)
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_range_tile_" + which + ":" in msg and part in msg, (which, kw, msg)
        assert c.untouched(), (which, kw)
    assert c.count(ws_bytes=exact) == 0, c.lib.coot_last_error()  # the same buffers, accepted at exactly the layout's size
    torch.cuda.synchronize()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_the_shipped_threshold_changes_the_route_and_not_the_bytes(env, storage):
    """With the constants as shipped: a search of M queries, M the storage's threshold, and a search of the first M - 1 of them return
    the same bytes for those M - 1.  (Which route served which is not observable, and nothing else is claimed about routing.)"""
    torch, cva = env
    n, dim = 1000, 64
    m = cva.retrieval.RANGE_TILE_MIN_M if storage == "float32" else cva.retrieval.RANGE_TILE_MIN_M_16BIT
    q, g = _planted(m, n, dim, 23)
    tq = torch.tensor(q, device="cuda")
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=True, storage=getattr(torch, storage))
    thr = torch.full((m,), 0.25, device="cuda")
    thr[::3] = 0.1
    at = _host(torch, *index.search_range(tq, thr))
    below = _host(torch, *index.search_range(tq[:m - 1], thr[:m - 1]))
    t = int(below[0][-1])
    assert t > m and bytes_equal(at[0][:m], below[0]) and bytes_equal(at[1][:t], below[1]) and bytes_equal(at[2][:t], below[2])
    assert np.array_equal(_host(torch, index.count_range(tq, thr))[0], np.diff(at[0]))
