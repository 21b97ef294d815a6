"""The range search (coot_retrieval_range_count, _scan, _fill; retrieval_range_device, GalleryIndex.search_range, GalleryIndex.count_range)
against its definition: the reference similarities are those that index.search(q, 1, want_sim=True) returns, code that exists without
this search, and (offsets, rows, scores) have to be, byte for byte, the host mirror compute_retrieval_range of those bytes
(tests/test_cpu_range.py checks the mirror against a brute force) — whatever the storage, the mask, the batch and the sweep's splits.
Shapes (N, d): (1000, 64) is eight 128-row blocks with a short last one and 16-byte loads; (130, 37) one block and two rows, no
16-byte loads; (5, 37) fewer rows than lanes.  M: 1, 3, 16 (the accumulator variants), 17 and 33 (across the slices of 16).
The thresholds are taken from the reference bytes, so that scores sit exactly on them."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
SHAPES = [(1000, 64), (130, 37), (5, 37)]
MS = [1, 3, 16, 17, 33]
KINDS = ["-inf", "+inf", "nan", "max", "median", "between"]
NINF = np.float32(-np.inf)


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
        return s[-1]  # one hit (the maximum is unique in these inputs): the >= boundary
    if kind == "median":
        return s[len(s) // 2]  # an exact score: that row and every row above it
    t = np.float32((np.float64(s[-1]) + np.float64(s[-2])) / 2)
    assert s[-2] < t < s[-1], (s[-2], t, s[-1])
    return t


def _thresholds(sim, shift=0):
    return np.array([_threshold(sim[i], KINDS[(i + shift) % len(KINDS)]) for i in range(sim.shape[0])], np.float32)


def _sim(torch, index, tq):
    return _host(torch, index.search(tq, 1, want_sim=True)[2])[0]


def _assert_mirror(got, sim, thr, keep=None, order="row"):
    from coot_videotext_amd import compute_retrieval_range
    want = compute_retrieval_range(sim, thr, keep=keep, order=order)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert bytes_equal(got[0], want[0]), (got[0], want[0])
    assert bytes_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert bytes_equal(got[2], want[2])
    return want


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_range_search_is_the_mirror_of_the_reference_similarities(env, storage, normalize):
    torch, cva = env
    case = 0
    for n, dim in SHAPES:
        tq, index = _index(torch, cva, storage, normalize, n, dim)
        keep = np.random.RandomState(3).rand(n) < 0.6
        gone = np.arange(1, n, 3)
        for m in MS:
            sim = _sim(torch, index, tq[:m])
            assert not np.isnan(sim).any() and sim.shape == (m, n)
            thr = _thresholds(sim, shift=m)
            for kp in (None, keep):
                case += 1
                tt = [thr.tolist(), thr, _dev(torch, thr)][case % 3]  # a host list (doubles that round back), a host array, a device tensor
                got = _host(torch, *index.search_range(tq[:m], tt, keep=_dev(torch, kp)))
                want = _assert_mirror(got, sim, thr, kp)
                kinds = [KINDS[(i + m) % len(KINDS)] for i in range(m)]
                cnt = np.diff(want[0])
                for i, kind in enumerate(kinds):  # what the thresholds are there for
                    kept_n = n if kp is None else int(kp.sum())
                    if kind == "-inf":
                        assert cnt[i] == kept_n
                    elif kind in ("+inf", "nan"):
                        assert cnt[i] == 0
                    elif kp is None:
                        assert cnt[i] == {"max": 1, "between": 1, "median": n - n // 2}[kind], (kind, cnt[i])
                got = _host(torch, *index.search_range(tq[:m], _dev(torch, thr), keep=_dev(torch, kp), order="score"))
                _assert_mirror(got, sim, thr, kp, order="score")
                counts = _host(torch, index.count_range(tq[:m], tt, keep=_dev(torch, kp)))[0]
                assert counts.dtype == np.int32 and np.array_equal(counts, cnt)
            scalar = float(np.sort(sim[0])[n // 2])  # one number for every query: exactly a score of query 0
            _assert_mirror(_host(torch, *index.search_range(tq[:m], scalar)), sim, scalar)
            _assert_mirror(_host(torch, *cva.retrieval_range_device(tq[:m], index.gallery, index.norms, scalar, keep=_dev(torch, keep))), sim, scalar, keep)
            if m in (3, 33):  # the index's own filter, alone and combined with keep
                index.remove(gone.tolist())
                kept = np.ones(n, bool)
                kept[gone] = False
                _assert_mirror(_host(torch, *index.search_range(tq[:m], thr)), sim, thr, kept)
                _assert_mirror(_host(torch, *index.search_range(tq[:m], thr, keep=_dev(torch, keep.astype(np.uint8) * 3), order="score")), sim, thr,
                               kept & keep, order="score")
                assert np.array_equal(_host(torch, index.count_range(tq[:m], thr))[0], np.diff(cva.compute_retrieval_range(sim, thr, keep=kept)[0]))
                index.restore()


@pytest.mark.parametrize("storage", STORAGES)
def test_a_segment_is_the_prefix_of_the_search(env, storage):
    """The definition, on code that exists without this search: for a query with 1 .. 128 hits the segment under order="score" is the
    result of index.search(q[i:i + 1], k = its count, keep=...), and the search's next entry scores below the threshold."""
    torch, cva = env
    n, dim, m = 1000, 64, 17
    tq, index = _index(torch, cva, storage, True, n, dim)
    sim = _sim(torch, index, tq[:m])
    keep = np.random.RandomState(8).rand(n) < 0.6
    ranks = [1, 2, 5, 64, 100, 127, 128]
    for kp in (None, keep):
        cols = np.arange(n) if kp is None else np.nonzero(kp)[0]
        thr = np.array([np.sort(sim[i, cols])[-ranks[i % len(ranks)]] for i in range(m)], np.float32)  # the r-th largest eligible score
        off, rows, sc = _host(torch, *index.search_range(tq[:m], thr, keep=_dev(torch, kp), order="score"))
        tk = _dev(torch, kp)
        for i in range(m):
            c = int(off[i + 1] - off[i])
            assert 1 <= ranks[i % len(ranks)] <= c <= 128, (i, c)
            k = min(c + 1, 128)
            idx, top = _host(torch, *index.search(tq[i:i + 1], k, keep=tk)[:2])
            assert bytes_equal(rows[off[i]:off[i + 1]], idx[0, :c]) and bytes_equal(sc[off[i]:off[i + 1]], top[0, :c]), (i, c)
            if k > c:
                assert top[0, c] < thr[i]


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_a_query_does_not_depend_on_its_batch_mates_or_the_splits(env, storage, splits):
    torch, cva = env
    n, dim, m = 1000, 64, 33
    tq, index = _index(torch, cva, storage, True, n, dim)
    sim = _sim(torch, index, tq)
    thr = _thresholds(sim, shift=3)
    tt = _dev(torch, thr)
    keep = _dev(torch, np.random.RandomState(4).rand(n) < 0.7)
    for kp in (None, keep):
        whole = _host(torch, *index.search_range(tq, tt, keep=kp))
        again = _host(torch, *index.search_range(tq, tt, keep=kp))
        assert all(bytes_equal(a, b) for a, b in zip(whole, again))
        off = whole[0]
        for i in range(m):
            one = _host(torch, *index.search_range(tq[i:i + 1], tt[i:i + 1], keep=kp))
            assert one[0].tolist() == [0, off[i + 1] - off[i]]
            assert bytes_equal(one[1], whole[1][off[i]:off[i + 1]]) and bytes_equal(one[2], whole[2][off[i]:off[i + 1]]), i
        for s in (1, 3):
            splits(s)
            split = _host(torch, *index.search_range(tq, tt, keep=kp))
            assert all(bytes_equal(a, b) for a, b in zip(whole, split)), s
        splits(0)


def test_blocks_without_a_hit_or_a_kept_row_are_skipped_with_the_same_result(env, splits):
    """keep leaves rows in the first and the last of eight blocks only: the count pass leaves the six between them before their first
    load and writes their zeros; the fill pass visits the blocks with a hit.  One workgroup (which walks all eight blocks) and the
    automatic splits give the mirror's bytes."""
    torch, cva = env
    n, dim, m = 1000, 64, 16
    tq, index = _index(torch, cva, "float16", True, n, dim)
    sim = _sim(torch, index, tq[:m])
    keep = np.zeros(n, bool)
    keep[5:120:3] = True
    keep[900:] = True
    thr = _thresholds(sim, shift=0)
    for s in (1, 0):
        splits(s)
        _assert_mirror(_host(torch, *index.search_range(tq[:m], thr, keep=_dev(torch, keep))), sim, thr, keep)
        # a hit in one block only: every query's own maximum
        top = sim.max(axis=1)
        got = _host(torch, *index.search_range(tq[:m], top))
        _assert_mirror(got, sim, top)
        assert got[0].tolist() == list(range(m + 1)) and got[1].tolist() == sim.argmax(axis=1).tolist()


def test_max_results_cuts_the_result_and_leaves_the_offsets(env):
    torch, cva = env
    n, dim, m = 1000, 64, 33
    tq, index = _index(torch, cva, "bfloat16", True, n, dim)
    sim = _sim(torch, index, tq)
    thr = _thresholds(sim, shift=0)
    off, rows, sc = _host(torch, *index.search_range(tq, thr))
    t = int(off[m])
    inside = [i for i in range(m) if off[i] < t // 2 < off[i + 1] - 1]
    assert t > 1000 and inside  # t // 2 cuts inside a segment
    for c in (1, t // 2, t, t + 5):
        got = _host(torch, *index.search_range(tq, _dev(torch, thr), max_results=c))
        assert got[1].shape == got[2].shape == (c,) and bytes_equal(got[0], off)
        u = min(t, c)
        assert bytes_equal(got[1][:u], rows[:u]) and bytes_equal(got[2][:u], sc[:u])
        assert (got[1][u:] == -1).all() and (got[2][u:] == NINF).all()


def test_no_hit_at_all(env):
    torch, cva = env
    tq, index = _index(torch, cva, "float32", True, 130, 37)
    for m in (1, 17):
        for kw in (dict(), dict(order="score")):
            off, rows, sc = _host(torch, *index.search_range(tq[:m], float("inf"), **kw))
            assert off.dtype == np.int64 and off.tolist() == [0] * (m + 1)
            assert rows.dtype == np.int32 and sc.dtype == np.float32 and rows.shape == sc.shape == (0,)
        off, rows, sc = _host(torch, *index.search_range(tq[:m], float("nan"), max_results=4))
        assert off.tolist() == [0] * (m + 1) and rows.tolist() == [-1] * 4 and (sc == NINF).all()
        assert _host(torch, index.count_range(tq[:m], float("inf")))[0].tolist() == [0] * m


class _CCall:
    """The three library calls through ctypes on buffers with a known fill: 16 queries, float32 rows used as they are."""

    def __init__(self, torch, cva, n, dim, room):
        self.torch, self.lib, self.n, self.dim, self.m = torch, cva.lib.load(), n, dim, 16
        q, g = _planted(33, n, dim, 11)
        self.q, self.g = torch.tensor(q[:16], device="cuda"), torch.tensor(g, device="cuda")
        self.size = self.lib.coot_retrieval_range_workspace_bytes(16, n, dim)
        self.ws = torch.zeros(self.size, dtype=torch.uint8, device="cuda")
        self.stride = (n + 127) // 128 + 1
        self.table = torch.full((16, self.stride), -7, dtype=torch.int32, device="cuda")
        self.off = torch.full((17,), -7, dtype=torch.int64, device="cuda")
        self.rows = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((room,), -7.0, device="cuda")
        self.thr = torch.zeros(16, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def count(self, m=16, dt=0, q=-1, table=-1, ws_bytes=None, ws_off=0, n=None, d=None):
        return self.lib.coot_retrieval_range_count(self.q.data_ptr() if q == -1 else q, self.g.data_ptr(), dt, None, None, self.thr.data_ptr(), m,
                                                   self.n if n is None else n, self.dim if d is None else d,
                                                   self.table.data_ptr() if table == -1 else table, self.ws.data_ptr() + ws_off,
                                                   (self.size if ws_bytes is None else ws_bytes) - ws_off, self.st)

    def scan(self, m=16, n=None, table=-1):
        return self.lib.coot_retrieval_range_scan(self.table.data_ptr() if table == -1 else table, m, self.n if n is None else n, self.off.data_ptr(),
                                                  None, self.st)

    def fill(self, capacity, m=16, dt=0, rows=-1, off=-1, ws_bytes=None, ws_off=0):
        return self.lib.coot_retrieval_range_fill(self.q.data_ptr(), self.g.data_ptr(), dt, None, None, self.thr.data_ptr(), m, self.n, self.dim,
                                                  self.table.data_ptr(), self.off.data_ptr() if off == -1 else off, capacity,
                                                  self.rows.data_ptr() if rows == -1 else rows, self.sc.data_ptr(), self.ws.data_ptr() + ws_off,
                                                  (self.size if ws_bytes is None else ws_bytes) - ws_off, self.st)

    def untouched(self):
        self.torch.cuda.synchronize()
        return (bool((self.table == -7).all()) and bool((self.off == -7).all()) and bool((self.rows == -7).all()) and bool((self.sc == -7.0).all())
                and not bool(self.ws.any()))


def test_the_fill_call_writes_nothing_at_or_beyond_the_capacity(env):
    """The library call itself, on buffers larger than the capacity that hold a sentinel: the entries below min(T, capacity) are the
    result's, everything else still holds the sentinel (the call leaves the tail of a cut result to its caller)."""
    torch, cva = env
    n, dim = 1000, 64
    tq = torch.tensor(_planted(33, n, dim, 11)[0][:16], device="cuda")
    index = cva.GalleryIndex(torch.tensor(_planted(33, n, dim, 11)[1], device="cuda"), normalize=False)
    sim = _sim(torch, index, tq)
    thr = _thresholds(sim, shift=4)
    off, rows, sc = _host(torch, *index.search_range(tq, thr))
    t = int(off[16])
    assert t > 1000
    for cap in (0, 1, t // 2, t, t + 5):
        c = _CCall(torch, cva, n, dim, room=t + 64)
        c.thr.copy_(torch.from_numpy(thr))
        assert c.count() == 0 and c.scan() == 0 and c.fill(cap) == 0, c.lib.coot_last_error()
        got_off, got_rows, got_sc = _host(torch, c.off, c.rows, c.sc)
        assert bytes_equal(got_off, off)
        u = min(t, cap)
        assert bytes_equal(got_rows[:u], rows[:u]) and bytes_equal(got_sc[:u], sc[:u]), cap
        assert (got_rows[u:] == -7).all() and (got_sc[u:] == -7.0).all(), cap
        table = _host(torch, c.table)[0]
        assert (table[:, 0] == 0).all() and np.array_equal(table[:, -1], np.diff(off)) and (np.diff(table, axis=1) >= 0).all()


def test_range_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message, and every buffer as it was."""
    torch, cva = env
    n, dim = 300, 16
    c = _CCall(torch, cva, n, dim, room=64)
    exact = c.size - 256  # the layout itself: the reported size has one piece of slack
    cases = [("count", dict(m=17), "M = 17"), ("count", dict(m=0), "M = 0"), ("count", dict(n=0), "N = 0"), ("count", dict(d=0), "d = 0"),
             ("count", dict(q=None), "null pointer"), ("count", dict(table=None), "null pointer"), ("count", dict(dt=7), "dtype = 7"),
             ("count", dict(ws_bytes=exact - 1), "workspace too small"), ("count", dict(ws_off=8), "16-byte aligned"),
             ("scan", dict(m=0), "M = 0"), ("scan", dict(n=0), "N = 0"), ("scan", dict(table=None), "null pointer"),
             ("fill", dict(capacity=-1), "capacity = -1"), ("fill", dict(capacity=8, m=17), "M = 17"), ("fill", dict(capacity=8, rows=None), "null pointer"),
             ("fill", dict(capacity=8, off=None), "null pointer"), ("fill", dict(capacity=8, dt=-1), "dtype = -1"),
             ("fill", dict(capacity=8, ws_bytes=exact - 1), "workspace too small"), ("fill", dict(capacity=8, ws_off=8), "16-byte aligned")]
    for which, kw, part in cases:
        assert getattr(c, which)(**kw) != 0, (which, kw)
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_range_" + which + ":" in msg and part in msg, (which, kw, msg)
        assert c.untouched(), (which, kw)
    assert c.count(ws_bytes=exact) == 0, c.lib.coot_last_error()  # the same buffers, accepted at exactly the layout's size
    torch.cuda.synchronize()


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_range_search_on_a_mutated_index(env, storage):
    """add, update, remove and compact in one sequence: search_range gives the bytes of a fresh index on the same rows."""
    torch, cva = env
    n, extra, dim, m = 600, 150, 64, 17
    q, g = _planted(33, n + extra, dim, 51)
    tq, tg = torch.tensor(q[:m], device="cuda"), torch.tensor(g, device="cuda")
    st = getattr(torch, storage)

    def same(a, b):
        a, b = _host(torch, *a), _host(torch, *b)
        assert all(bytes_equal(x, y) for x, y in zip(a, b))

    index = cva.GalleryIndex(tg[:n], normalize=True, storage=st, capacity=n + 50)
    assert index.add(tg[n:]) == n  # grows past the capacity
    patched = tg.clone()
    moved = [0, 127, 128, 599, 700]
    patched[moved] = tg[[9, 8, 7, 6, 5]]
    index.update(moved, patched[moved])
    fresh = cva.GalleryIndex(patched, normalize=True, storage=st)
    thr = _dev(torch, _thresholds(_sim(torch, fresh, tq), shift=2))
    same(index.search_range(tq, thr), fresh.search_range(tq, thr))
    same(index.search_range(tq, thr), cva.retrieval_range_device(tq, index.gallery, index.norms, thr))
    gone = np.arange(0, n + extra, 4)
    index.remove(gone.tolist())
    kept = np.ones(n + extra, bool)
    kept[gone] = False
    removed = index.search_range(tq, thr)
    same(removed, fresh.search_range(tq, thr, keep=_dev(torch, kept)))
    old = index.compact()
    assert len(index) == len(old) == int(kept.sum())
    fresh = cva.GalleryIndex(patched[old.to(torch.int64)].contiguous(), normalize=True, storage=st)
    got = index.search_range(tq, thr)
    same(got, fresh.search_range(tq, thr))
    same((got[0], old[got[1].to(torch.int64)], got[2]), removed)  # in the old numbering: the search that skipped them
    same((index.count_range(tq, thr),), (torch.diff(removed[0]).to(torch.int32),))


def test_refusals_that_need_a_device(env):
    """The messages of the shared check under the new names, before any launch; there is no k."""
    torch, cva = env
    g = torch.zeros(5, 8, device="cuda")
    index = cva.GalleryIndex(g, normalize=False)
    q = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError, match=r"GalleryIndex.search_range: queries of width 7, gallery of width 8"):
        index.search_range(torch.zeros(2, 7, device="cuda"), 0.5)
    with pytest.raises(ValueError, match=r"GalleryIndex.count_range: queries of width 7, gallery of width 8"):
        index.count_range(torch.zeros(2, 7, device="cuda"), 0.5)
    with pytest.raises(ValueError, match=r"retrieval_range_device: queries of width 7, gallery of width 8"):
        cva.retrieval_range_device(torch.zeros(2, 7, device="cuda"), g, None, 0.5)
    with pytest.raises(ValueError, match=r"GalleryIndex.search_range: threshold of shape \(3,\), 2 queries"):
        index.search_range(q, torch.zeros(3, device="cuda"))
    for bad in (torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                torch.zeros(2, dtype=torch.bfloat16, device="cuda")):
        with pytest.raises(ValueError, match="threshold on the device has to be torch.float32, not " + str(bad.dtype)):
            index.search_range(q, bad)
        with pytest.raises(ValueError, match="GalleryIndex.count_range: threshold on the device has to be torch.float32"):
            index.count_range(q, bad)
    with pytest.raises(ValueError, match=r'retrieval_range_device: order="score" needs max_results=None'):
        cva.retrieval_range_device(q, g, None, 0.5, max_results=3, order="score")
    with pytest.raises(ValueError, match="GalleryIndex.search_range: max_results = 0"):
        index.search_range(q, 0.5, max_results=0)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_range"):
        index.search_range(q.cpu(), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_range"):
        index.search_range(q, 0.5, keep=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="retrieval_range_device: a gallery of dtype torch.float64"):
        cva.retrieval_range_device(q, g.double(), None, 0.5)
    # one query as [d]; zero vectors score +0 everywhere, and -0.0 as a threshold takes them all
    off, rows, sc = index.search_range(q[0], -0.0)
    assert _host(torch, off)[0].tolist() == [0, 5] and _host(torch, rows)[0].tolist() == [0, 1, 2, 3, 4]
    assert _host(torch, index.count_range(q, [0.0, 1e-30]))[0].tolist() == [5, 0]
