"""The self-join (GalleryIndex.self_join, count_self_join, retrieval_self_join_device; coot_retrieval_join_count, _fill) against its
definition: the reference similarities are those that index.search(index.gallery.float(), 1, want_sim=True) returns, and (offsets,
rows, scores) have to be, byte for byte, the host mirror compute_retrieval_self_join of those bytes, and the range search on the widened
gallery with j <= i dropped.
Shapes (N, d): (1000, 64) is eight 128-row blocks and sixteen row tiles, the last block short; (192, 64): the second block is exactly
one row tile; (129, 37): one row beyond the first block, no 16-byte loads, d no multiple of 32; (130, 37): block 1 has two rows;
(64, 64): one tile that is all diagonal; (5, 37): fewer rows than a tile.
Exact duplicate rows are planted on top of the random gallery: at (63, 64) and (127, 128), across a row tile's and a block's edge, inside
one block, in different blocks, and one triple.  The thresholds are taken from the reference bytes, so that scores sit exactly on them."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
SHAPES = [(1000, 64), (192, 64), (129, 37), (130, 37), (64, 64), (5, 37)]
KINDS = ["-inf", "+inf", "nan", "max", "median", "between"]
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _dups(n):
    """(source, copy) rows: the copy becomes the bytes of the source."""
    if n >= 1000:
        return [(63, 64), (127, 128), (10, 40), (7, 700), (20, 333), (20, 901), (998, 999)]
    if n >= 129:
        return [(63, 64), (127, 128), (10, 40), (5, 90), (20, 21), (20, 100)] + ([(11, 150)] if n > 150 else [])
    if n >= 64:
        return [(10, 40), (2, 50), (2, 51), (62, 63)]
    return [(1, 3)]


def _gallery(n, dim, seed=11):
    g = _planted(1, n, dim, seed)[1].copy()
    for a, b in _dups(n):
        g[b] = g[a]
    return g


_CASES = {}


def _case(torch, cva, storage, normalize, n, dim):
    """(the index, the reference similarities [N, N] on the host, the thresholds [N]): made once and shared, read only."""
    key = (storage, normalize, n, dim)
    if key not in _CASES:
        index = cva.GalleryIndex(torch.tensor(_gallery(n, dim), device="cuda"), normalize=normalize, storage=getattr(torch, storage))
        sim = _host(torch, index.search(index.gallery.float(), 1, want_sim=True)[2])[0]
        assert sim.shape == (n, n) and not np.isnan(sim).any()
        thr = _thresholds(sim)
        sim.setflags(write=False)
        thr.setflags(write=False)
        _CASES[key] = (index, sim, thr)
    return _CASES[key]


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared arrays are read only)


def _threshold(right, kind):
    """One threshold from a row's reference similarities right of the diagonal (float32, no NaN among them)."""
    s = np.sort(right)
    if kind == "-inf" or len(s) == 0:
        return np.float32(-np.inf)
    if kind == "+inf":
        return np.float32(np.inf)
    if kind == "nan":
        return np.float32(np.nan)
    if kind == "max" or len(s) == 1:
        return s[-1]  # the >= boundary on the row's best partner
    if kind == "median":
        return s[len(s) // 2]  # an exact score: that row and every row above it
    t = np.float32((np.float64(s[-1]) + np.float64(s[-2])) / 2)
    return t if s[-2] < t < s[-1] else s[-1]


def _thresholds(sim, shift=0):
    return np.array([_threshold(sim[i, i + 1:], KINDS[(i + shift) % len(KINDS)]) for i in range(sim.shape[0])], np.float32)


def _groups(n, kind):
    if kind is None:
        return None
    if kind == "runs":  # clips of one video are adjacent: ids in runs of 10
        return (np.arange(n) // 10).astype(np.int32)
    return (np.random.RandomState(8).randint(-3, 4, n) * 1000003).astype(np.int64)  # scattered, negative ids among them


def _assert_same(got, want, what=None):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert bytes_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert bytes_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:5])
    assert bytes_equal(got[2], want[2]), what


def _range_as_pairs(res, ok):
    """A range search of the gallery against itself, (offsets, rows, scores), with j <= i dropped and the rows i with ok[i] false emptied."""
    off, rows, sc = res
    n = len(off) - 1
    seg = np.repeat(np.arange(n), np.diff(off))
    sel = (rows > seg) & ok[seg]
    out = np.zeros(n + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(seg[sel], minlength=n))
    return out, rows[sel], sc[sel]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_self_join_is_the_mirror_and_the_range_search_right_of_the_diagonal(env, storage, normalize):
    torch, cva = env
    case = 0
    for n, dim in SHAPES:
        index, sim, thr = _case(torch, cva, storage, normalize, n, dim)
        assert bytes_equal(sim, np.ascontiguousarray(sim.T)), (n, dim)  # s(i, j) == s(j, i) on bytes: what makes one half enough
        keep = np.random.RandomState(3).rand(n) < 0.6
        gone = np.arange(1, n, 3)
        case += 1  # (seven per shape: what alternates does so from shape to shape too)
        for kp in (None, keep):
            for gk in (None, "runs", "scattered"):
                case += 1
                groups = _groups(n, gk)
                own = np.ones(n, bool)
                tt = [thr.tolist(), thr, _dev(torch, thr)][case % 3]  # a host list (doubles that round back), a host array, a device tensor
                try:
                    if case % 2:
                        index.remove(gone.tolist())
                        own[gone] = False
                    ok = own if kp is None else own & kp
                    got = _host(torch, *index.self_join(tt, keep=_dev(torch, kp), groups=_dev(torch, groups)))
                    want = cva.compute_retrieval_self_join(sim, thr, keep=ok, groups=groups)
                    _assert_same(got, want, (n, dim, case))
                    counts = _host(torch, index.count_self_join(tt, keep=_dev(torch, kp), groups=_dev(torch, groups)))[0]
                    assert counts.dtype == np.int32 and np.array_equal(counts, np.diff(want[0]))
                    if gk is None:
                        rr = _host(torch, *index.search_range(index.gallery.float(), _dev(torch, thr), keep=_dev(torch, kp)))
                        _assert_same(got, _range_as_pairs(rr, ok), ("range", n, dim, case))
                        if n >= 64 and kp is None and not case % 2:  # what the planted rows and the thresholds are there for
                            pairs = set(zip(np.repeat(np.arange(n), np.diff(got[0])).tolist(), got[1].tolist()))
                            for a, b in _dups(n):
                                assert ((a, b) in pairs) == (KINDS[a % len(KINDS)] not in ("+inf", "nan")), (a, b)  # a copy is the row's best partner
                            assert all(np.diff(got[0])[i] == n - 1 - i for i in range(0, n, len(KINDS)))  # -inf: every row right of i
                finally:
                    index.restore()
        whole = _host(torch, *cva.retrieval_self_join_device(index.gallery, index.norms if normalize else None, float(thr[3]), keep=_dev(torch, keep)))
        _assert_same(whole, cva.compute_retrieval_self_join(sim, thr[3], keep=keep), ("scalar", n, dim))


def test_the_bytes_do_not_depend_on_the_chunks(env, monkeypatch):
    """N = 1000 in one, three and eight chunks (retrieval.JOIN_TABLE_BYTES at its value, 13 824 and 1), in both max_results modes, with
    keep and groups: the same bytes; and two calls give the same bytes."""
    torch, cva = env
    n, dim = 1000, 64
    for storage, normalize in (("bfloat16", True), ("float32", False)):
        index, sim, thr = _case(torch, cva, storage, normalize, n, dim)
        keep, groups = np.random.RandomState(5).rand(n) < 0.8, _groups(n, "runs")
        for kp, gr in ((None, None), (keep, groups)):
            want = cva.compute_retrieval_self_join(sim, thr, keep=kp, groups=gr)
            t = int(want[0][-1])
            assert t > 1000
            for budget, chunks in ((1 << 28, 1), (13824, 3), (1, 8)):
                monkeypatch.setattr(cva.retrieval, "JOIN_TABLE_BYTES", budget)
                assert len(cva.retrieval._join_chunks(n, cva.retrieval.JOIN_TABLE_BYTES)) == chunks
                args = dict(keep=_dev(torch, kp), groups=_dev(torch, gr))
                _assert_same(_host(torch, *index.self_join(_dev(torch, thr), **args)), want, (budget, "exact"))
                _assert_same(_host(torch, *index.self_join(_dev(torch, thr), **args)), want, (budget, "again"))
                got = _host(torch, *index.self_join(thr, max_results=t + 9, **args))
                _assert_same((got[0], got[1][:t], got[2][:t]), want, (budget, "room"))
                assert (got[1][t:] == -1).all() and (got[2][t:] == NINF).all()
                assert np.array_equal(_host(torch, index.count_self_join(thr, **args))[0], np.diff(want[0]))


def test_max_results_cuts_the_result_and_leaves_the_offsets_exact(env, monkeypatch):
    torch, cva = env
    n, dim = 1000, 64
    index, sim, thr = _case(torch, cva, "float16", True, n, dim)
    want = cva.compute_retrieval_self_join(sim, thr)
    off, rows, sc = want
    t = int(off[n])
    i = next(i for i in range(n // 2, n) if off[i + 1] - off[i] >= 3)
    inside = int(off[i] + (off[i + 1] - off[i]) // 2)  # cuts inside a segment
    for budget in (1 << 28, 13824):
        monkeypatch.setattr(cva.retrieval, "JOIN_TABLE_BYTES", budget)
        for c in (1, t // 2, inside, t - 1, t, t + 5):
            got = _host(torch, *index.self_join(_dev(torch, thr), max_results=c))
            assert got[1].shape == got[2].shape == (c,) and bytes_equal(got[0], off)
            u = min(t, c)
            assert bytes_equal(got[1][:u], rows[:u]) and bytes_equal(got[2][:u], sc[:u]), c
            assert (got[1][u:] == -1).all() and (got[2][u:] == NINF).all(), c
        got = _host(torch, *index.self_join(float("-inf"), max_results=7))  # every pair, and room for seven
        assert got[0].tolist() == np.concatenate([[0], np.cumsum(np.arange(n - 1, -1, -1))]).tolist() and got[0][n] == n * (n - 1) // 2
        assert got[1].tolist() == [1, 2, 3, 4, 5, 6, 7] and bytes_equal(got[2], sim[0, 1:8])


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_an_index_that_changed_joins_as_a_fresh_one(env, storage):
    torch, cva = env
    n, dim = 192, 64
    fresh, sim, thr = _case(torch, cva, storage, True, n, dim)
    g = torch.tensor(_gallery(n, dim), device="cuda")
    junk = torch.tensor(_planted(1, 3, dim, 99)[1], device="cuda")
    h = torch.cat([g[:50], junk[:1], g[50:150]])
    h[3], h[121] = junk[1], junk[2]  # (row 121 is row 120 once the junk row is gone)
    index = cva.GalleryIndex(h, normalize=True, storage=getattr(torch, storage))
    index.remove([50])
    index.compact()
    index.update([3, 120], g[[3, 120]])
    index.add(g[150:])
    assert index.n == n
    want = _host(torch, *fresh.self_join(_dev(torch, thr)))
    _assert_same(want, cva.compute_retrieval_self_join(sim, thr))
    _assert_same(_host(torch, *index.self_join(_dev(torch, thr))), want)
    _assert_same(_host(torch, *index.self_join(thr, max_results=len(want[1]))), want)


class _Join:
    """The library calls through ctypes on buffers with a known fill: the rows [row0, row0 + rows) of an index."""

    def __init__(self, torch, cva, index, thr, row0, rows, room, keep=None, groups=None):
        self.torch, self.lib = torch, cva.lib.load()
        self.g, self.norms, self.keep, self.groups = index.gallery, index.norms if index.normalize else None, keep, groups
        self.code = {torch.float32: 0, torch.bfloat16: cva.retrieval.GALLERY_BF16, torch.float16: cva.retrieval.GALLERY_F16}[index.gallery.dtype]
        self.n, self.dim = index.gallery.shape
        self.row0, self.rows = row0, rows
        self.nbc = (self.n - row0 + 127) // 128
        self.table = torch.full((rows, self.nbc + 1), -7, dtype=torch.int32, device="cuda")
        self.off = torch.full((rows + 1,), -7, dtype=torch.int64, device="cuda")
        self.out = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((room,), -7.0, device="cuda")
        self.thr = torch.from_numpy(np.asarray(thr)).cuda()
        self.st = torch.cuda.current_stream().cuda_stream

    def _p(self, t):
        return None if t is None else t.data_ptr()

    def count(self, dt=None, g=-1, table=-1, thr=-1, row0=None, rows=None, n=None, d=None):
        return self.lib.coot_retrieval_join_count(self.g.data_ptr() if g == -1 else g, self.code if dt is None else dt, self._p(self.norms),
                                                  self._p(self.keep), self._p(self.groups), self.thr.data_ptr() if thr == -1 else thr,
                                                  self.row0 if row0 is None else row0, self.rows if rows is None else rows,
                                                  self.n if n is None else n, self.dim if d is None else d,
                                                  self.table.data_ptr() if table == -1 else table, self.st)

    def scan(self):
        return self.lib.coot_retrieval_range_scan(self.table.data_ptr(), self.rows, self.n - self.row0, self.off.data_ptr(), None, self.st)

    def fill(self, capacity, dt=None, off=-1, out=-1, sc=-1, row0=None, rows=None, n=None, d=None):
        return self.lib.coot_retrieval_join_fill(self.g.data_ptr(), self.code if dt is None else dt, self._p(self.norms), self._p(self.keep),
                                                 self._p(self.groups), self.thr.data_ptr(), self.row0 if row0 is None else row0,
                                                 self.rows if rows is None else rows, self.n if n is None else n, self.dim if d is None else d,
                                                 self.table.data_ptr(), self.off.data_ptr() if off == -1 else off, capacity,
                                                 self.out.data_ptr() if out == -1 else out, self.sc.data_ptr() if sc == -1 else sc, self.st)

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.table == -7).all()) and bool((self.off == -7).all()) and bool((self.out == -7).all()) and bool((self.sc == -7.0).all())


def test_the_calls_write_every_slot_of_their_table_and_nothing_beyond_the_capacity(env):
    """The library calls on a chunk that starts inside the gallery (rows 256 .. 655 of 1000), on buffers that hold a sentinel: after the
    count call every slot [r][0 .. nbc) holds the row's hits in that block, zeros left of the diagonal included, and slot nbc, the
    scan's, still the sentinel; the fill writes the chunk's segment of the result below the capacity and nothing else."""
    torch, cva = env
    n, dim, row0, rows = 1000, 64, 256, 400
    for storage, normalize, with_filters in (("bfloat16", True, False), ("float32", True, True)):
        index, sim, thr = _case(torch, cva, storage, normalize, n, dim)
        keep = (np.random.RandomState(6).rand(n) < 0.7) if with_filters else None
        groups = _groups(n, "runs") if with_filters else None
        off, hits, sc = cva.compute_retrieval_self_join(sim, thr, keep=keep, groups=groups)
        lo, hi = int(off[row0]), int(off[row0 + rows])
        t = hi - lo
        assert t > 1000
        seg = np.repeat(np.arange(n), np.diff(off))[lo:hi]
        per_block = np.zeros((rows, (n - row0 + 127) // 128), np.int32)
        np.add.at(per_block, (seg - row0, hits[lo:hi] // 128 - row0 // 128), 1)
        assert (per_block[200:, 0] == 0).all() and (per_block[384:, :3] == 0).all() and per_block[:, 0].sum() > 0  # (left of the diagonal)
        for cap in (0, 1, t // 2, t, t + 5):
            c = _Join(torch, cva, index, thr, row0, rows, room=t + 64, keep=None if keep is None else _dev(torch, keep.astype(np.uint8)),
                      groups=_dev(torch, groups))
            assert c.count() == 0, c.lib.coot_last_error()
            table = _host(torch, c.table)[0]
            assert bytes_equal(np.ascontiguousarray(table[:, :c.nbc]), per_block) and (table[:, c.nbc] == -7).all()
            assert c.scan() == 0 and c.fill(cap) == 0, c.lib.coot_last_error()
            got_off, got_rows, got_sc = _host(torch, c.off, c.out, c.sc)
            assert bytes_equal(got_off, off[row0:row0 + rows + 1] - lo)
            u = min(t, cap)
            assert bytes_equal(got_rows[:u], hits[lo:lo + u]) and bytes_equal(got_sc[:u], sc[lo:lo + u]), cap
            assert (got_rows[u:] == -7).all() and (got_sc[u:] == -7.0).all(), cap


def test_garbage_in_the_wrappers_buffers_does_not_show(env, monkeypatch):
    """The wrapper allocates its table, counts, offsets and result with torch.empty: blocks of exactly those sizes are filled with a
    pattern and freed first, so that the caching allocator hands them out again."""
    torch, cva = env
    n, dim = 1000, 64
    index, sim, thr = _case(torch, cva, "bfloat16", True, n, dim)
    want = cva.compute_retrieval_self_join(sim, thr)
    t = int(want[0][-1])
    for budget in (1 << 28, 13824):
        monkeypatch.setattr(cva.retrieval, "JOIN_TABLE_BYTES", budget)
        chunks = cva.retrieval._join_chunks(n, budget)
        sizes = [4 * max(r * ((n - r0 + 127) // 128 + 1) for r0, r in chunks), 4 * n, 8 * (n + 1), 4 * t, 4 * t] + [8 * (r + 1) for _, r in chunks]
        for mode in (None, t):
            junk = [torch.full((s,), 0x5A, dtype=torch.uint8, device="cuda") for s in sizes for _ in range(2)]
            torch.cuda.synchronize()
            del junk
            _assert_same(_host(torch, *index.self_join(_dev(torch, thr), max_results=mode)), want, (budget, mode))
            assert np.array_equal(_host(torch, index.count_self_join(_dev(torch, thr)))[0], np.diff(want[0]))


def test_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message naming the entry, and every buffer as it was."""
    torch, cva = env
    n, dim = 300, 16
    index = cva.GalleryIndex(torch.tensor(_gallery(n, dim), device="cuda"), normalize=True)
    c = _Join(torch, cva, index, np.zeros(n, np.float32), 128, 100, room=64)
    big = 65535 * 64 + 1
    cases = [("count", dict(row0=64), "row0 = 64"), ("count", dict(row0=-128), "row0 = -128"), ("count", dict(rows=0), "rows = 0"),
             ("count", dict(rows=173), "rows = 173"), ("count", dict(row0=384), "row0 = 384"), ("count", dict(n=0), "N = 0"), ("count", dict(d=0), "d = 0"),
             ("count", dict(rows=big, n=2 ** 31 - 1), "rows = %d" % big), ("count", dict(g=None), "null pointer"), ("count", dict(table=None), "null pointer"),
             ("count", dict(thr=None), "null pointer"), ("count", dict(dt=7), "dtype = 7"),
             ("fill", dict(capacity=-1), "capacity = -1"), ("fill", dict(capacity=8, row0=64), "row0 = 64"), ("fill", dict(capacity=8, rows=0), "rows = 0"),
             ("fill", dict(capacity=8, rows=173), "rows = 173"), ("fill", dict(capacity=8, n=0), "N = 0"), ("fill", dict(capacity=8, d=0), "d = 0"),
             ("fill", dict(capacity=8, out=None), "null pointer"), ("fill", dict(capacity=8, sc=None), "null pointer"),
             ("fill", dict(capacity=8, off=None), "null pointer"), ("fill", dict(capacity=8, dt=-1), "dtype = -1")]
    for which, kw, part in cases:
        assert getattr(c, which)(**kw) != 0, (which, kw)
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_join_" + which + ":" in msg and part in msg, (which, kw, msg)
        assert c.untouched(), (which, kw)
    assert c.count() == 0, c.lib.coot_last_error()  # the same buffers, accepted as they were made
    torch.cuda.synchronize()
