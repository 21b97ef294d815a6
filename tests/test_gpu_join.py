"""The join of two indexes (GalleryIndex.join, count_join, retrieval_join_device; coot_retrieval_cross_join_count, _fill) against its
definition: the reference similarities are those that right.search(left.gallery.float(), 1, want_sim=True) returns, and (offsets,
rows, scores) have to be, byte for byte, the host mirror compute_retrieval_join of those bytes, and the range search of the right
index with the widened left rows as queries, the segments of masked left rows emptied.
Shapes (N_left, N_right, d): (130, 1000, 64) is three row tiles, the last with two rows, and eight blocks, the last short; (64, 128,
64): exactly one tile and one block; (65, 129, 37): one row beyond each, d no multiple of 32 and no 16-byte rows; (1000, 5, 64): many
left rows, fewer right rows than a block; (5, 5, 37); (1, 300, 16).
Right rows 63, 64, 127, 128 and the last one are byte copies of left rows from both sides of the 63 / 64 tile edge.  The thresholds are
taken from the reference bytes, so that scores sit exactly on them."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
PAIRS = [(a, b) for a in STORAGES for b in STORAGES]
FEW_PAIRS = [(s, s) for s in STORAGES] + [("float32", "bfloat16"), ("bfloat16", "float32")]
MAIN = (130, 1000, 64)
SHAPES = [MAIN, (64, 128, 64), (65, 129, 37), (1000, 5, 64), (5, 5, 37), (1, 300, 16)]
KINDS = ["-inf", "+inf", "nan", "max", "median", "between"]
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _plants(nl, nr):
    """(left row, right row): the right row becomes the bytes of the left row.  Every left row is planted once."""
    lefts = [r for r in (63, 64, 62, 65, 3) if r < nl] or [0]
    rights = sorted({r for r in (63, 64, 127, 128, nr - 1) if r < nr})
    return [(lefts[q % len(lefts)], r) for q, r in enumerate(rights)][:len(lefts)]


def _rows(nl, nr, dim):
    """The float32 rows of both sides (read only), the right ones with the planted copies."""
    left = _planted(1, nl, dim, 21)[1]
    right = _planted(1, nr, dim, 22)[1].copy()
    for a, b in _plants(nl, nr):
        right[b] = left[a]
    right.setflags(write=False)
    return left, right


def _threshold(row, kind):
    """One threshold from a left row's reference similarities (float32, no NaN among them)."""
    s = np.sort(row)
    if kind == "-inf":
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


def _thresholds(sim):
    return np.array([_threshold(sim[i], KINDS[i % len(KINDS)]) for i in range(sim.shape[0])], np.float32)


_INDEXES, _CASES = {}, {}


def _index(torch, cva, side, storage, normalize, shape):
    key = (side, storage, normalize, shape)
    if key not in _INDEXES:
        rows = _rows(*shape)[side == "right"]
        _INDEXES[key] = cva.GalleryIndex(torch.tensor(rows, device="cuda"), normalize=normalize, storage=getattr(torch, storage))
    return _INDEXES[key]


def _case(torch, cva, sl, sr, normalize, shape):
    """(left index, right index, the reference similarities [N_left, N_right] on the host, the thresholds [N_left]): made once and
    shared, read only.  The reference is computed by the top-K search, code that does not know of joins."""
    key = (sl, sr, normalize, shape)
    if key not in _CASES:
        left, right = _index(torch, cva, "left", sl, normalize, shape), _index(torch, cva, "right", sr, normalize, shape)
        sim = _host(torch, right.search(left.gallery.float(), 1, want_sim=True)[2])[0]
        assert sim.shape == shape[:2] and sim.dtype == np.float32 and not np.isnan(sim).any()
        thr = _thresholds(sim)
        sim.setflags(write=False)
        thr.setflags(write=False)
        _CASES[key] = (left, right, sim, thr)
    return _CASES[key]


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared arrays are read only)


def _groups(nl, nr, kind):
    """(groups, other_groups) in one id space."""
    if kind is None:
        return None, None
    if kind == "runs":  # clips of one video are adjacent: ids in runs of 10 on either side
        return (np.arange(nl) // 10).astype(np.int32), (np.arange(nr) // 10 % 7).astype(np.int32)
    rs = np.random.RandomState(8)  # scattered, negative ids among them, as int64
    return (rs.randint(-3, 4, nl) * 1000003).astype(np.int64), (rs.randint(-3, 4, nr) * 1000003).astype(np.int64)


def _assert_same(got, want, what=None):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert bytes_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert bytes_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:5])
    assert bytes_equal(got[2], want[2]), what


def _emptied(res, ask):
    """A range search (offsets, rows, scores) with the segments of the queries i with ask[i] false emptied."""
    off, rows, sc = res
    m = len(off) - 1
    seg = np.repeat(np.arange(m), np.diff(off))
    sel = ask[seg]
    out = np.zeros(m + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(seg[sel], minlength=m))
    return out, rows[sel], sc[sel]


def _pairs(res):
    off, rows, sc = res
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return seg, rows, sc


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("sl,sr", PAIRS)
def test_join_is_the_mirror_and_the_range_search_of_the_right_index(env, sl, sr, normalize):
    torch, cva = env
    _check_plants()
    case = 0
    for shape in SHAPES:
        if shape != MAIN and (sl, sr) not in FEW_PAIRS:
            continue  # (the four other mixed pairs run at the main shape: same code, other template arguments)
        nl, nr, dim = shape
        left, right, sim, thr = _case(torch, cva, sl, sr, normalize, shape)
        rs = np.random.RandomState(3)
        keep_l, keep_r = rs.rand(nl) < 0.6, rs.rand(nr) < 0.6
        gone_l, gone_r = np.arange(1, nl, 3) if nl > 1 else np.array([0]), np.arange(0, nr, 4)
        case += 1  # (what alternates does so from shape to shape too)
        # nothing filtered, nothing removed: what the planted rows and the thresholds are there for
        seg, rows, _ = _pairs(_host(torch, *left.join(right, thr)))
        pairs = set(zip(seg.tolist(), rows.tolist()))
        for a, b in _plants(nl, nr):
            assert sim[a, b] == sim[a].max(), (a, b)  # a copy is the row's best partner
            assert ((a, b) in pairs) == (KINDS[a % len(KINDS)] not in ("+inf", "nan")), (a, b)
        for kp, okp in ((None, None), (keep_l, None), (None, keep_r), (keep_l, keep_r)):
            for gk in (None, "runs", "scattered"):
                case += 1
                groups, other_groups = _groups(nl, nr, gk)
                ask, ok = np.ones(nl, bool), np.ones(nr, bool)
                tt = [thr.tolist(), thr, _dev(torch, thr)][case % 3]  # a host list (doubles that round back), a host array, a device tensor
                try:
                    if case % 2:
                        left.remove(gone_l.tolist())
                        ask[gone_l] = False
                    if case // 2 % 2:
                        right.remove(gone_r.tolist())
                        ok[gone_r] = False
                    ask = ask if kp is None else ask & kp
                    ok = ok if okp is None else ok & okp
                    args = dict(keep=_dev(torch, kp), other_keep=_dev(torch, okp), groups=_dev(torch, groups), other_groups=_dev(torch, other_groups))
                    got = _host(torch, *left.join(right, tt, **args))
                    want = cva.compute_retrieval_join(sim, thr, keep=ask, other_keep=ok, groups=groups, other_groups=other_groups)
                    _assert_same(got, want, (shape, case))
                    counts = _host(torch, left.count_join(right, tt, **args))[0]
                    assert counts.dtype == np.int32 and np.array_equal(counts, np.diff(want[0]))
                    if gk is None:
                        rr = _host(torch, *right.search_range(left.gallery.float(), _dev(torch, thr), keep=_dev(torch, okp)))
                        _assert_same(got, _emptied(rr, ask), ("range", shape, case))
                        for i in range(0, nl, len(KINDS)):  # -inf: every eligible right row
                            assert counts[i] == (int(ok.sum()) if ask[i] else 0), i
                finally:
                    left.restore()
                    right.restore()
        t = float(thr[3 % nl]) if np.isfinite(thr[3 % nl]) else 0.0
        whole = _host(torch, *cva.retrieval_join_device(left.gallery, left.norms if normalize else None, right.gallery,
                                                        right.norms if normalize else None, t, keep=_dev(torch, keep_l), other_keep=_dev(torch, keep_r)))
        _assert_same(whole, cva.compute_retrieval_join(sim, t, keep=keep_l, other_keep=keep_r), ("scalar", shape))


def _check_plants():
    """Right rows 63, 64, 127, 128 and the last one, from left rows on both sides of the 63 / 64 tile edge, as far as a shape has them."""
    assert _plants(130, 1000) == [(63, 63), (64, 64), (62, 127), (65, 128), (3, 999)]
    assert _plants(65, 129) == [(63, 63), (64, 64), (62, 127), (3, 128)]
    assert _plants(64, 128) == [(63, 63), (62, 64), (3, 127)] and _plants(1000, 5) == [(63, 4)]
    assert _plants(5, 5) == [(3, 4)] and _plants(1, 300) == [(0, 63)]


@pytest.mark.parametrize("storage,normalize,n,dim", [("bfloat16", True, 1000, 64), ("float32", False, 129, 37), ("float16", True, 130, 64)])
def test_an_index_joined_with_itself_holds_the_self_join(env, storage, normalize, n, dim):
    """index.join(index, thr) returns both orientations and the diagonal; with j <= i dropped on the host it is index.self_join(thr),
    byte for byte, and the same holds with keep given to both sides."""
    torch, cva = env
    index = cva.GalleryIndex(torch.tensor(_rows(n, n, dim)[1], device="cuda"), normalize=normalize, storage=getattr(torch, storage))
    sim = _host(torch, index.search(index.gallery.float(), 1, want_sim=True)[2])[0]
    thr = _thresholds(sim)
    keep = np.random.RandomState(4).rand(n) < 0.7
    for kp in (None, keep):
        got = _host(torch, *index.join(index, _dev(torch, thr), keep=_dev(torch, kp), other_keep=_dev(torch, kp)))
        _assert_same(got, cva.compute_retrieval_join(sim, thr, keep=kp, other_keep=kp), "mirror")
        seg, rows, sc = _pairs(got)
        if kp is None:
            assert all(np.diff(got[0])[i] == n for i in range(0, n, len(KINDS)))  # -inf: the diagonal and both sides of it
        sel = rows > seg
        out = np.zeros(n + 1, np.int64)
        out[1:] = np.cumsum(np.bincount(seg[sel], minlength=n))
        _assert_same((out, rows[sel], sc[sel]), _host(torch, *index.self_join(_dev(torch, thr), keep=_dev(torch, kp))), "self_join")


@pytest.mark.parametrize("sl,sr", [("float32", "float32"), ("bfloat16", "float32"), ("float16", "bfloat16")])
def test_a_scalar_threshold_gives_the_same_pairs_from_either_side(env, sl, sr):
    torch, cva = env
    for normalize in (True, False):
        a, b, sim, _ = _case(torch, cva, sl, sr, normalize, MAIN)
        t = float(np.sort(sim.max(1))[sim.shape[0] // 2])  # the best partner of half the left rows, and whatever else reaches it
        ab, ba = _host(torch, *a.join(b, t)), _host(torch, *b.join(a, t))
        assert ab[0][-1] == ba[0][-1] >= sim.shape[0] // 2
        one = sorted((int(i), int(j), s.tobytes()) for i, j, s in zip(*_pairs(ab)))
        other = sorted((int(i), int(j), s.tobytes()) for j, i, s in zip(*_pairs(ba)))
        assert one == other


SQUARE = (1000, 1000, 64)


def test_the_bytes_do_not_depend_on_the_chunks(env, monkeypatch):
    """1000 left rows in one, three and sixteen chunks (retrieval.JOIN_TABLE_BYTES at its value, 13 824 and 1), in both max_results
    modes, with filters and groups: the same bytes; and two calls give the same bytes."""
    torch, cva = env
    nl, nr, dim = SQUARE
    for sl, sr, normalize in (("bfloat16", "float32", True), ("float32", "float16", False)):
        left, right, sim, thr = _case(torch, cva, sl, sr, normalize, SQUARE)
        rs = np.random.RandomState(5)
        keep_l, keep_r = rs.rand(nl) < 0.8, rs.rand(nr) < 0.8
        gl, gr = _groups(nl, nr, "runs")
        for kp, okp, g, og in ((None, None, None, None), (keep_l, keep_r, gl, gr)):
            want = cva.compute_retrieval_join(sim, thr, keep=kp, other_keep=okp, groups=g, other_groups=og)
            t = int(want[0][-1])
            assert t > 1000
            for budget, chunks in ((1 << 28, 1), (13824, 3), (1, 16)):
                monkeypatch.setattr(cva.retrieval, "JOIN_TABLE_BYTES", budget)
                assert len(cva.retrieval._cross_join_chunks(nl, nr, cva.retrieval.JOIN_TABLE_BYTES)) == chunks
                args = dict(keep=_dev(torch, kp), other_keep=_dev(torch, okp), groups=_dev(torch, g), other_groups=_dev(torch, og))
                _assert_same(_host(torch, *left.join(right, _dev(torch, thr), **args)), want, (budget, "exact"))
                _assert_same(_host(torch, *left.join(right, _dev(torch, thr), **args)), want, (budget, "again"))
                got = _host(torch, *left.join(right, thr, max_results=t + 9, **args))
                _assert_same((got[0], got[1][:t], got[2][:t]), want, (budget, "room"))
                assert (got[1][t:] == -1).all() and (got[2][t:] == NINF).all()
                assert np.array_equal(_host(torch, left.count_join(right, thr, **args))[0], np.diff(want[0]))


def test_max_results_cuts_the_result_and_leaves_the_offsets_exact(env, monkeypatch):
    torch, cva = env
    nl, nr, dim = SQUARE
    left, right, sim, thr = _case(torch, cva, "float16", "bfloat16", True, SQUARE)
    off, rows, sc = cva.compute_retrieval_join(sim, thr)
    t = int(off[nl])
    i = next(i for i in range(nl // 2, nl) if off[i + 1] - off[i] >= 3)
    inside = int(off[i] + (off[i + 1] - off[i]) // 2)  # cuts inside a segment
    for budget in (1 << 28, 13824):
        monkeypatch.setattr(cva.retrieval, "JOIN_TABLE_BYTES", budget)
        for c in (1, inside, t - 1, t, t + 5):
            got = _host(torch, *left.join(right, _dev(torch, thr), max_results=c))
            assert got[1].shape == got[2].shape == (c,) and bytes_equal(got[0], off)
            u = min(t, c)
            assert bytes_equal(got[1][:u], rows[:u]) and bytes_equal(got[2][:u], sc[:u]), c
            assert (got[1][u:] == -1).all() and (got[2][u:] == NINF).all(), c
        got = _host(torch, *left.join(right, float("-inf"), max_results=7))  # every pair, and room for seven
        assert got[0].tolist() == (np.arange(nl + 1) * nr).tolist()
        assert got[1].tolist() == [0, 1, 2, 3, 4, 5, 6] and bytes_equal(got[2], sim[0, :7])


@pytest.mark.parametrize("sl,sr", [("float32", "bfloat16"), ("bfloat16", "float32")])
def test_indexes_that_changed_join_as_fresh_ones(env, sl, sr):
    torch, cva = env
    shape = (130, 1000, 64)
    fresh_l, fresh_r, sim, thr = _case(torch, cva, sl, sr, True, shape)
    rows_l, rows_r = (torch.tensor(r, device="cuda") for r in _rows(*shape))
    junk = torch.tensor(_planted(1, 3, 64, 99)[1], device="cuda")

    def changed(g, storage, n):
        h = torch.cat([g[:50], junk[:1], g[50:n - 20]])
        h[3], h[101] = junk[1], junk[2]  # (row 101 is row 100 once the junk row is gone)
        index = cva.GalleryIndex(h, normalize=True, storage=getattr(torch, storage))
        index.remove([50])
        index.compact()
        index.update([3, 100], g[[3, 100]])
        index.add(g[n - 20:])
        assert index.n == n
        return index

    left, right = changed(rows_l, sl, shape[0]), changed(rows_r, sr, shape[1])
    want = _host(torch, *fresh_l.join(fresh_r, _dev(torch, thr)))
    _assert_same(want, cva.compute_retrieval_join(sim, thr))
    _assert_same(_host(torch, *left.join(right, _dev(torch, thr))), want, "both")
    _assert_same(_host(torch, *left.join(fresh_r, thr)), want, "left")
    _assert_same(_host(torch, *fresh_l.join(right, thr, max_results=len(want[1]))), want, "right")


class _Cross:
    """The library calls through ctypes on buffers with a known fill: the left rows [row0, row0 + rows)."""

    def __init__(self, torch, cva, left, right, thr, row0, rows, room, lkeep=None, rkeep=None, lgroups=None, rgroups=None):
        self.torch, self.lib = torch, cva.lib.load()
        codes = {torch.float32: 0, torch.bfloat16: cva.retrieval.GALLERY_BF16, torch.float16: cva.retrieval.GALLERY_F16}
        self.hold = (left, right, lkeep, rkeep, lgroups, rgroups)
        self.nb = (right.gallery.shape[0] + 127) // 128
        self.table = torch.full((rows, self.nb + 1), -7, dtype=torch.int32, device="cuda")
        self.off = torch.full((rows + 1,), -7, dtype=torch.int64, device="cuda")
        self.out = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((room,), -7.0, device="cuda")
        self.thr = torch.from_numpy(np.array(thr)).cuda()  # (a copy: the shared arrays are read only)
        p = self._p
        self.args = dict(left=p(left.gallery), ldt=codes[left.gallery.dtype], lnorms=p(left.norms if left.normalize else None), right=p(right.gallery),
                         rdt=codes[right.gallery.dtype], rnorms=p(right.norms if right.normalize else None), lkeep=p(lkeep), rkeep=p(rkeep),
                         lgroups=p(lgroups), rgroups=p(rgroups), thr=p(self.thr), row0=row0, rows=rows, nl=left.gallery.shape[0],
                         nr=right.gallery.shape[0], d=left.gallery.shape[1], table=p(self.table), off=p(self.off), capacity=0, out=p(self.out),
                         sc=p(self.sc))
        self.st = torch.cuda.current_stream().cuda_stream
        self.rows, self.nr = rows, right.gallery.shape[0]

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    HEAD = ("left", "ldt", "lnorms", "right", "rdt", "rnorms", "lkeep", "rkeep", "lgroups", "rgroups", "thr", "row0", "rows", "nl", "nr", "d", "table")

    def count(self, **kw):
        a = dict(self.args, **kw)
        return self.lib.coot_retrieval_cross_join_count(*[a[k] for k in self.HEAD], self.st)

    def scan(self):
        return self.lib.coot_retrieval_range_scan(self.table.data_ptr(), self.rows, self.nr, self.off.data_ptr(), None, self.st)

    def fill(self, **kw):
        a = dict(self.args, **kw)
        return self.lib.coot_retrieval_cross_join_fill(*[a[k] for k in self.HEAD + ("off", "capacity", "out", "sc")], self.st)

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.table == -7).all()) and bool((self.off == -7).all()) and bool((self.out == -7).all()) and bool((self.sc == -7.0).all())


def test_the_calls_write_every_slot_of_their_table_and_nothing_beyond_the_capacity(env):
    """The library calls on a chunk that starts inside the left side (rows 256 .. 655 of 1000), on buffers that hold a sentinel: after
    the count call every slot [r][0 .. nb) holds the row's hits in that block, and slot nb, the scan's, still the sentinel; the fill
    writes the chunk's segment of the result below the capacity and nothing else."""
    torch, cva = env
    nl, nr, dim = SQUARE
    row0, rows = 256, 400
    for sl, sr, normalize, with_filters in (("bfloat16", "float32", True, False), ("float32", "float16", False, True)):
        left, right, sim, thr = _case(torch, cva, sl, sr, normalize, SQUARE)
        rs = np.random.RandomState(6)
        keep_l = (rs.rand(nl) < 0.7) if with_filters else None
        keep_r = (rs.rand(nr) < 0.7) if with_filters else None
        if with_filters:
            keep_l[320:384] = False  # a row tile of the chunk in which nothing asks
            keep_r[256:384] = False  # a block in which nothing may be returned
        gl, gr = _groups(nl, nr, "runs" if with_filters else None)
        off, hits, sc = cva.compute_retrieval_join(sim, thr, keep=keep_l, other_keep=keep_r, groups=gl, other_groups=gr)
        lo, hi = int(off[row0]), int(off[row0 + rows])
        t = hi - lo
        assert t > 1000
        seg = np.repeat(np.arange(nl), np.diff(off))[lo:hi]
        per_block = np.zeros((rows, (nr + 127) // 128), np.int32)
        np.add.at(per_block, (seg - row0, hits[lo:hi] // 128), 1)
        for cap in (0, 1, t // 2, t, t + 5):
            c = _Cross(torch, cva, left, right, thr, row0, rows, room=t + 64, lkeep=None if keep_l is None else _dev(torch, keep_l.astype(np.uint8)),
                       rkeep=None if keep_r is None else _dev(torch, keep_r.astype(np.uint8)), lgroups=_dev(torch, gl), rgroups=_dev(torch, gr))
            assert c.count() == 0, c.lib.coot_last_error()
            table = _host(torch, c.table)[0]
            assert bytes_equal(np.ascontiguousarray(table[:, :c.nb]), per_block) and (table[:, c.nb] == -7).all()
            assert c.scan() == 0 and c.fill(capacity=cap) == 0, c.lib.coot_last_error()
            got_off, got_rows, got_sc = _host(torch, c.off, c.out, c.sc)
            assert bytes_equal(got_off, off[row0:row0 + rows + 1] - lo)
            u = min(t, cap)
            assert bytes_equal(got_rows[:u], hits[lo:lo + u]) and bytes_equal(got_sc[:u], sc[lo:lo + u]), cap
            assert (got_rows[u:] == -7).all() and (got_sc[u:] == -7.0).all(), cap


def test_garbage_in_the_wrappers_buffers_does_not_show(env, monkeypatch):
    """The wrapper allocates its table, counts, offsets and result with torch.empty: blocks of exactly those sizes are filled with a
    pattern and freed first, so that the caching allocator hands them out again."""
    torch, cva = env
    nl, nr, dim = SQUARE
    left, right, sim, thr = _case(torch, cva, "bfloat16", "float32", True, SQUARE)
    want = cva.compute_retrieval_join(sim, thr)
    t = int(want[0][-1])
    for budget in (1 << 28, 13824):
        monkeypatch.setattr(cva.retrieval, "JOIN_TABLE_BYTES", budget)
        chunks = cva.retrieval._cross_join_chunks(nl, nr, budget)
        sizes = [4 * max(r for _, r in chunks) * ((nr + 127) // 128 + 1), 4 * nl, 8 * (nl + 1), 4 * t, 4 * t] + [8 * (r + 1) for _, r in chunks]
        for mode in (None, t):
            junk = [torch.full((s,), 0x5A, dtype=torch.uint8, device="cuda") for s in sizes for _ in range(2)]
            torch.cuda.synchronize()
            del junk
            _assert_same(_host(torch, *left.join(right, _dev(torch, thr), max_results=mode)), want, (budget, mode))
            assert np.array_equal(_host(torch, left.count_join(right, _dev(torch, thr)))[0], np.diff(want[0]))


def test_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message naming the entry, and every buffer as it was."""
    torch, cva = env
    nl, nr, dim = 300, 200, 16
    left = cva.GalleryIndex(torch.tensor(_planted(1, nl, dim, 31)[1], device="cuda"), normalize=True)
    right = cva.GalleryIndex(torch.tensor(_planted(1, nr, dim, 32)[1], device="cuda"), normalize=True, storage=torch.bfloat16)
    c = _Cross(torch, cva, left, right, np.zeros(nl, np.float32), 128, 100, room=64)
    ids = torch.zeros(nl, dtype=torch.int32, device="cuda")
    big = 65535 * 64 + 1
    both = [(dict(row0=32), "row0 = 32"), (dict(row0=-64), "row0 = -64"), (dict(rows=0), "rows = 0"), (dict(rows=173), "rows = 173"),
            (dict(row0=320), "row0 = 320"), (dict(rows=big, nl=2 ** 31 - 1), "rows = %d" % big), (dict(nl=0), "N_left = 0"), (dict(nr=0), "N_right = 0"),
            (dict(d=0), "d = 0"), (dict(left=None), "null pointer"), (dict(right=None), "null pointer"), (dict(thr=None), "null pointer"),
            (dict(table=None), "null pointer"), (dict(ldt=7), "left_dtype = 7"), (dict(rdt=-1), "right_dtype = -1"),
            (dict(lnorms=None), "left_norms and right_norms"), (dict(rnorms=None), "left_norms and right_norms"),
            (dict(lgroups=ids.data_ptr()), "left_groups and right_groups"), (dict(rgroups=ids.data_ptr()), "left_groups and right_groups")]
    cases = [("count", kw, part) for kw, part in both] + [("fill", dict(kw, capacity=8), part) for kw, part in both]
    cases += [("fill", dict(capacity=-1), "capacity = -1"), ("fill", dict(capacity=8, out=None), "null pointer"),
              ("fill", dict(capacity=8, sc=None), "null pointer"), ("fill", dict(capacity=8, off=None), "null pointer")]
    for which, kw, part in cases:
        assert getattr(c, which)(**kw) != 0, (which, kw)
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_cross_join_" + which + ":" in msg and part in msg, (which, kw, msg)
        assert c.untouched(), (which, kw)
    assert c.count() == 0, c.lib.coot_last_error()  # the same buffers, accepted as they were made
    torch.cuda.synchronize()
