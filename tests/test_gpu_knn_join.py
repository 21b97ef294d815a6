"""The K best partners of every row (GalleryIndex.knn_join, knn_graph, retrieval_knn_join_device; coot_retrieval_knn_join) against
its definition: the reference similarities are those that right.search(left.gallery.float(), 1, want_sim=True) returns, code that knows
nothing of this feature, and (idx, scores) have to be, byte for byte, the host mirror compute_retrieval_knn_join of those bytes, the
scoped search of the right index with the widened left rows as queries, and (the graph) index.neighbors with the masked rows blanked.
Shapes (N_left, N_right, d): (130, 1000, 64) is three row tiles, the last with two rows, and eight blocks, the last short; (64, 128,
64): exactly one tile and one block; (65, 129, 37): one row beyond each, d no multiple of 32 and no 16-byte rows; (1000, 5, 64): many
left rows, fewer right rows than a block; (5, 5, 37); (1, 300, 16).
Right rows 63, 64, 127, 128 and the last one are byte copies of left rows from both sides of the 63 / 64 tile edge: exact ties and
best hits on every tile and block edge.  All inputs are finite."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
PAIRS = [(a, b) for a in STORAGES for b in STORAGES]
FEW_PAIRS = [(s, s) for s in STORAGES] + [("float32", "bfloat16"), ("bfloat16", "float32")]
MAIN = (130, 1000, 64)
SHAPES = [MAIN, (64, 128, 64), (65, 129, 37), (1000, 5, 64), (5, 5, 37), (1, 300, 16)]
SPLIT_CAP = 32
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


class _Splits:
    """Sets rt_knn_splits and restores the automatic choice afterwards."""

    def __init__(self, cva, n):
        self.lib, self.n = cva.lib.load(), n

    def __enter__(self):
        assert self.lib.coot_set_option(b"rt_knn_splits", self.n) == 0

    def __exit__(self, *exc):
        assert self.lib.coot_set_option(b"rt_knn_splits", 0) == 0


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


_INDEXES, _CASES = {}, {}


def _index(torch, cva, side, storage, normalize, shape):
    key = (side, storage, normalize, shape)
    if key not in _INDEXES:
        rows = _rows(*shape)[side == "right"]
        _INDEXES[key] = cva.GalleryIndex(torch.tensor(rows, device="cuda"), normalize=normalize, storage=getattr(torch, storage))
    return _INDEXES[key]


def _case(torch, cva, sl, sr, normalize, shape):
    """(left index, right index, the reference similarities [N_left, N_right] on the host): made once and shared, read only.  The
    reference is computed by the top-K search."""
    key = (sl, sr, normalize, shape)
    if key not in _CASES:
        left, right = _index(torch, cva, "left", sl, normalize, shape), _index(torch, cva, "right", sr, normalize, shape)
        sim = _host(torch, right.search(left.gallery.float(), 1, want_sim=True)[2])[0]
        assert sim.shape == shape[:2] and sim.dtype == np.float32 and np.isfinite(sim).all()
        sim.setflags(write=False)
        _CASES[key] = (left, right, sim)
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
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == got[1].shape == want[0].shape, what
    assert bytes_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert bytes_equal(got[1], want[1]), (what, np.argwhere(got[1].view(np.int32) != want[1].view(np.int32))[:5])


def _ks(nr):
    return sorted({1, min(10, nr), min(128, nr)})  # 1, 10, 128 where N_right allows, and K = N_right where it is below


def _check_plants():
    assert _plants(130, 1000) == [(63, 63), (64, 64), (62, 127), (65, 128), (3, 999)]
    assert _plants(65, 129) == [(63, 63), (64, 64), (62, 127), (3, 128)]
    assert _plants(64, 128) == [(63, 63), (62, 64), (3, 127)] and _plants(1000, 5) == [(63, 4)]
    assert _plants(5, 5) == [(3, 4)] and _plants(1, 300) == [(0, 63)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("sl,sr", PAIRS)
def test_knn_join_is_the_mirror_and_the_search_of_the_right_index(env, sl, sr, normalize):
    torch, cva = env
    _check_plants()
    case = 0
    for shape in SHAPES:
        if shape != MAIN and (sl, sr) not in FEW_PAIRS:
            continue  # (the four other mixed pairs run at the main shape: same code, other template arguments)
        nl, nr, dim = shape
        left, right, sim = _case(torch, cva, sl, sr, normalize, shape)
        rs = np.random.RandomState(3)
        keep_l, keep_r = rs.rand(nl) < 0.6, rs.rand(nr) < 0.6
        gone_l, gone_r = np.arange(1, nl, 3) if nl > 1 else np.array([0]), np.arange(0, nr, 4)
        # nothing filtered: a planted copy is its row's best partner (normalised: by a tie at most, and then the later row wins)
        idx = _host(torch, left.knn_join(right, 1)[0])[0]
        for a, b in _plants(nl, nr):
            assert sim[a, b] == sim[a].max() and idx[a, 0] == np.nonzero(sim[a] == sim[a].max())[0][-1], (a, b)
        for k in _ks(nr):
            for kp, okp in ((None, None), (keep_l, keep_r)) if k != min(10, nr) else ((None, None), (keep_l, None), (None, keep_r), (keep_l, keep_r)):
                for gk in (None, "runs", "scattered"):
                    case += 1
                    groups, other_groups = _groups(nl, nr, gk)
                    ask, ok = np.ones(nl, bool), np.ones(nr, bool)
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
                        got = _host(torch, *left.knn_join(right, k, **args))
                        want = cva.compute_retrieval_knn_join(sim, k, keep=ask, other_keep=ok, groups=groups, other_groups=other_groups)
                        _assert_same(got, want, (shape, k, case))
                        assert (got[0][~ask] == -1).all() and (got[1][~ask] == NINF).all()  # a masked row does not ask
                        if gk is None and kp is None:  # the cross case without groups: the tile search on the widened copy
                            ri, rsc, _ = right.search(left.gallery.float(), k, keep=_dev(torch, okp))
                            ri, rsc = _host(torch, ri, rsc)
                            ri[~ask], rsc[~ask] = -1, NINF
                            _assert_same(got, (ri, rsc), ("search", shape, k, case))
                    finally:
                        left.restore()
                        right.restore()
        whole = _host(torch, *cva.retrieval_knn_join_device(left.gallery, left.norms if normalize else None, right.gallery,
                                                            right.norms if normalize else None, min(10, nr), keep=_dev(torch, keep_l),
                                                            other_keep=_dev(torch, keep_r)))
        _assert_same(whole, cva.compute_retrieval_knn_join(sim, min(10, nr), keep=keep_l, other_keep=keep_r), ("bare", shape))


@pytest.mark.parametrize("sl,sr,normalize", [("float32", "float32", True), ("bfloat16", "float16", True), ("float16", "float32", False)])
def test_the_bytes_do_not_depend_on_the_splits(env, sl, sr, normalize):
    """rt_knn_splits forced to 1, 2, 3 and the cap, and automatic: the same bytes, with and without filters, at 8 blocks (main), 3
    blocks ((1, 300, 16)) and one block; 2 and 3 leave shares of unequal length, the cap gives every block a share of its own."""
    torch, cva = env
    for shape in (MAIN, (1, 300, 16), (65, 129, 37), (1000, 5, 64)):
        nl, nr, dim = shape
        left, right, sim = _case(torch, cva, sl, sr, normalize, shape)
        rs = np.random.RandomState(5)
        keep_l, keep_r = rs.rand(nl) < 0.8, rs.rand(nr) < 0.5
        gl, gr = _groups(nl, nr, "scattered")
        for k in sorted({min(10, nr), min(128, nr)}):
            for kp, okp, g, og in ((None, None, None, None), (keep_l, keep_r, gl, gr)):
                want = cva.compute_retrieval_knn_join(sim, k, keep=kp, other_keep=okp, groups=g, other_groups=og)
                args = dict(keep=_dev(torch, kp), other_keep=_dev(torch, okp), groups=_dev(torch, g), other_groups=_dev(torch, og))
                for s in (1, 2, 3, SPLIT_CAP, 0):
                    with _Splits(cva, s):
                        _assert_same(_host(torch, *left.knn_join(right, k, **args)), want, (shape, k, s))


def test_filters_that_empty_tiles_blocks_and_tails(env):
    """keep / other_keep as a contiguous range, all 64 rows of one left tile masked, whole blocks of the right side masked (they are
    not read), fewer than K eligible rows, and no eligible row at all; under one and several splits."""
    torch, cva = env
    nl, nr, dim = MAIN
    for sl, sr, normalize in (("float32", "bfloat16", True), ("float16", "float16", False)):
        left, right, sim = _case(torch, cva, sl, sr, normalize, MAIN)
        tile = np.ones(nl, bool)
        tile[64:128] = False  # the second row tile does not ask
        rng_l, rng_r = np.zeros(nl, bool), np.zeros(nr, bool)
        rng_l[30:100] = True
        rng_r[200:520] = True  # blocks 0, 5, 6, 7 keep nothing; block 1 and block 4 keep a part
        few = np.zeros(nr, bool)
        few[[5, 127, 128, 640, 999]] = True  # five eligible rows: K = 10 has a tail of five
        none = np.zeros(nr, bool)
        gl, gr = _groups(nl, nr, "runs")
        for kp, okp, g, og in ((tile, None, None, None), (tile, rng_r, gl, gr), (rng_l, rng_r, None, None), (None, few, None, None),
                               (rng_l, few, gl, gr), (None, none, None, None), (np.zeros(nl, bool), None, None, None)):
            for k in (10, 128):
                want = cva.compute_retrieval_knn_join(sim, k, keep=kp, other_keep=okp, groups=g, other_groups=og)
                if okp is few:
                    assert (want[0][:, 5:] == -1).all() and (g is not None or (want[0][:, :5] >= 0).all())
                args = dict(keep=_dev(torch, kp), other_keep=_dev(torch, okp), groups=_dev(torch, g), other_groups=_dev(torch, og))
                for s in (0, 1, 3):
                    with _Splits(cva, s):
                        _assert_same(_host(torch, *left.knn_join(right, k, **args)), want, (k, s))
        # every row of one group: nothing is eligible although nothing is masked
        zeros = (np.zeros(nl, np.int64), np.zeros(nr, np.int64))
        got = _host(torch, *left.knn_join(right, 3, groups=_dev(torch, zeros[0]), other_groups=_dev(torch, zeros[1])))
        assert (got[0] == -1).all() and (got[1] == NINF).all()


@pytest.mark.parametrize("storage,normalize,n,dim", [("bfloat16", True, 1000, 64), ("float32", False, 129, 37), ("float16", True, 130, 64)])
def test_knn_graph_is_neighbors_of_every_row(env, storage, normalize, n, dim):
    """Without groups: index.neighbors(arange(N), k), byte for byte, with the masked rows blanked; with groups: search_scoped with
    exclude=groups on the widened gallery; keep applies to both sides and a removed row neither asks nor is returned."""
    torch, cva = env
    index = cva.GalleryIndex(torch.tensor(_rows(n, n, dim)[1], device="cuda"), normalize=normalize, storage=getattr(torch, storage))
    sim = _host(torch, index.search(index.gallery.float(), 1, want_sim=True)[2])[0]
    rs = np.random.RandomState(4)
    keep = rs.rand(n) < 0.7
    gone = np.arange(2, n, 5)
    groups = _groups(n, n, "runs")[0]
    every = torch.arange(n, device="cuda")
    for k in (1, 10, min(n, 128)):
        for kp, removed in ((None, False), (keep, False), (None, True), (keep, True)):
            ask = np.ones(n, bool) if kp is None else kp.copy()
            try:
                if removed:
                    index.remove(gone.tolist())
                    ask[gone] = False
                got = _host(torch, *index.knn_graph(k, keep=_dev(torch, kp)))
                assert not (got[0] == np.arange(n)[:, None]).any()  # a row never returns itself
                _assert_same(got, cva.compute_retrieval_knn_join(sim, k, keep=ask, other_keep=ask, exclude_same_row=True), ("mirror", k))
                ni, nsc = _host(torch, *index.neighbors(every, k, keep=_dev(torch, kp)))
                ni[~ask], nsc[~ask] = -1, NINF  # neighbors lets masked rows ask; the graph does not
                _assert_same(got, (ni, nsc), ("neighbors", k))
                got = _host(torch, *index.knn_graph(k, keep=_dev(torch, kp), groups=_dev(torch, groups)))
                assert not (groups[np.maximum(got[0], 0)] == groups[:, None])[got[0] >= 0].any()  # nor a row of its own group
                _assert_same(got, cva.compute_retrieval_knn_join(sim, k, keep=ask, other_keep=ask, groups=groups, other_groups=groups), ("mirror, groups", k))
                si, ssc, _ = index.search_scoped(index.gallery.float(), k, _dev(torch, groups), exclude=_dev(torch, groups), keep=_dev(torch, kp))
                si, ssc = _host(torch, si, ssc)
                si[~ask], ssc[~ask] = -1, NINF
                _assert_same(got, (si, ssc), ("search_scoped", k))
            finally:
                index.restore()
    if normalize:  # no duplicate rows: an index joined with itself finds every row in slot 0, and the graph is the rest of that list
        with_self = _host(torch, *index.knn_join(index, 11))
        assert np.array_equal(with_self[0][:, 0], np.arange(n))
        graph = _host(torch, *index.knn_graph(10))
        assert bytes_equal(np.ascontiguousarray(with_self[0][:, 1:]), graph[0]) and bytes_equal(np.ascontiguousarray(with_self[1][:, 1:]), graph[1])


def test_rows_at_the_tile_edges_against_the_scoped_search_row_by_row(env):
    """At the main shape, 16 left rows spread over the tile edges: each is, byte for byte, right.search_scoped with that widened row
    alone as the query."""
    torch, cva = env
    nl, nr, dim = MAIN
    rows = [0, 1, 3, 31, 32, 62, 63, 64, 65, 66, 100, 126, 127, 128, 129, 96]
    for sl, sr, normalize in (("float32", "float32", True), ("bfloat16", "float32", True), ("float16", "bfloat16", False)):
        left, right, _ = _case(torch, cva, sl, sr, normalize, MAIN)
        okp = np.random.RandomState(9).rand(nr) < 0.7
        for gk in ("runs", "scattered"):
            gl, gr = _groups(nl, nr, gk)
            dgl, dgr, dk = _dev(torch, gl), _dev(torch, gr), _dev(torch, okp)
            for k in (10, 128):
                got = _host(torch, *left.knn_join(right, k, other_keep=dk, groups=dgl, other_groups=dgr))
                for i in rows:
                    si, ssc, _ = right.search_scoped(left.gallery[i:i + 1].float(), k, dgr, exclude=dgl[i:i + 1], keep=dk)
                    si, ssc = _host(torch, si, ssc)
                    assert bytes_equal(got[0][i:i + 1], si) and bytes_equal(got[1][i:i + 1], ssc), (gk, k, i)


class _Call:
    """The arguments of coot_retrieval_knn_join on buffers that hold a sentinel."""

    NAMES = ("left", "ldt", "lnorms", "right", "rdt", "rnorms", "lkeep", "rkeep", "lgroups", "rgroups", "same", "nl", "nr", "d", "k", "idx", "sc", "ws",
             "ws_bytes")

    def __init__(self, torch, cva, left, right, k):
        self.torch, self.lib = torch, cva.lib.load()
        codes = cva.retrieval._gallery_codes()
        nl, nr = left.gallery.shape[0], right.gallery.shape[0]
        self.idx = torch.full((nl, k), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((nl, k), -7.0, device="cuda")
        self.ws = torch.full((self.lib.coot_retrieval_knn_join_workspace_bytes(nl, nr, k),), 0x5A, dtype=torch.uint8, device="cuda")
        self.args = dict(left=left.gallery.data_ptr(), ldt=codes[left.gallery.dtype], lnorms=left.norms.data_ptr(), right=right.gallery.data_ptr(),
                         rdt=codes[right.gallery.dtype], rnorms=right.norms.data_ptr(), lkeep=None, rkeep=None, lgroups=None, rgroups=None, same=0,
                         nl=nl, nr=nr, d=left.gallery.shape[1], k=k, idx=self.idx.data_ptr(), sc=self.sc.data_ptr(), ws=self.ws.data_ptr(),
                         ws_bytes=self.ws.numel())
        self.st = torch.cuda.current_stream().cuda_stream

    def __call__(self, **kw):
        a = dict(self.args, **kw)
        return self.lib.coot_retrieval_knn_join(*[a[n] for n in self.NAMES], self.st)

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.idx == -7).all()) and bool((self.sc == -7.0).all()) and bool((self.ws == 0x5A).all())


def test_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message naming the entry, and every buffer as it was."""
    torch, cva = env
    nl, nr, dim = 300, 200, 16
    left = cva.GalleryIndex(torch.tensor(_planted(1, nl, dim, 31)[1], device="cuda"), normalize=True)
    right = cva.GalleryIndex(torch.tensor(_planted(1, nr, dim, 32)[1], device="cuda"), normalize=True, storage=torch.bfloat16)
    with _Splits(cva, 2):
        c = _Call(torch, cva, left, right, 10)
        assert c.ws.numel() == nl * 2 * 10 * 8 + 256
        ids = torch.zeros(nl, dtype=torch.int32, device="cuda")
        cases = [(dict(k=0), "K = 0"), (dict(k=201), "K = 201"), (dict(k=129, nr=500), "K = 129"), (dict(nl=0), "N_left = 0"),
                 (dict(nl=65535 * 64 + 1), "N_left = %d" % (65535 * 64 + 1)), (dict(nr=0), "N_right = 0"), (dict(d=0), "d = 0"),
                 (dict(left=None), "null pointer"), (dict(right=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(sc=None), "null pointer"),
                 (dict(ws=None), "null pointer"), (dict(ldt=7), "left_dtype = 7"), (dict(rdt=-1), "right_dtype = -1"),
                 (dict(lnorms=None), "left_norms and right_norms"), (dict(rnorms=None), "left_norms and right_norms"),
                 (dict(lgroups=ids.data_ptr()), "left_groups and right_groups"), (dict(rgroups=ids.data_ptr()), "left_groups and right_groups"),
                 (dict(same=2), "exclude_same_row = 2"), (dict(ws=c.ws.data_ptr() + 8), "not 16-byte aligned"), (dict(ws_bytes=nl * 2 * 10 * 8 - 1), "workspace too small")]
        for kw, part in cases:
            assert c(**kw) != 0, kw
            msg = c.lib.coot_last_error().decode()
            assert "retrieval_knn_join:" in msg and part in msg, (kw, msg)
            assert c.untouched(), kw
        assert c() == 0, c.lib.coot_last_error()  # the same buffers, accepted as they were made
        got = _host(torch, c.idx, c.sc)
    sim = _host(torch, right.search(left.gallery.float(), 1, want_sim=True)[2])[0]
    _assert_same(got, cva.compute_retrieval_knn_join(sim, 10), "accepted")
