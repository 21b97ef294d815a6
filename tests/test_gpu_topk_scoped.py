"""The scoped top-K search (coot_retrieval_topk_scoped; retrieval_topk_scoped_device, GalleryIndex.search_scoped, GalleryIndex.neighbors)
against its definition: the similarities come back with want_sim=True, and idx and scores have to be, byte for byte, the host mirror
compute_retrieval_topk_scoped of those bytes (tests/test_cpu_topk_scoped.py checks the mirror against a brute force) and, query by
query, GalleryIndex.search under the mask of the query's eligible rows — whatever the storage, the mode, the layout of the ids, the
mask and the sweep's row splits.
Shapes (N, d): (1000, 64) is eight 128-row blocks with a short last one and 16-byte loads; (130, 37) one block and two rows, no
16-byte loads; (5, 37) fewer rows than lanes.  (M, K): one query; 3 (4 accumulators); 16 at K = 128; 17 and 33 cross the slices of
16.  K is clipped to N."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
SHAPES = [(1000, 64), (130, 37), (5, 37)]
MK = [(1, 1), (3, 10), (16, 128), (17, 10), (33, 128)]
LAYOUTS = ["runs", "permuted", "one", None]
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


def _groups(n, layout, seed=0):
    """Ids of the n rows on the host (int64), or None.  runs: seven adjacent rows per id, the ids -4, -1, 2, ... (any int32 value is an
    id); permuted: the same ids scattered; one: every row has the id 5."""
    if layout is None:
        return None
    if layout == "one":
        return np.full(n, 5, np.int64)
    g = np.arange(n, dtype=np.int64) // 7 * 3 - 4
    return g[np.random.RandomState(seed).permutation(n)] if layout == "permuted" else g


def _scope(n, groups, m, seed):
    """One id per query: ids that rows carry, and (from three queries on) a negative id and an id above every row's, which none does."""
    ids = np.arange(n) if groups is None else np.unique(groups)
    scope = np.random.RandomState(seed).choice(ids, size=m).astype(np.int64)
    if m >= 3:
        scope[1], scope[m - 1] = -7, int(ids.max()) + 1
    return scope


def _index(torch, cva, storage, normalize, n, dim, seed=11):
    q, g = _planted(33, n, dim, seed)
    return torch.tensor(q, device="cuda"), cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=normalize, storage=getattr(torch, storage))


def _dev(torch, a, dtype=None):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda().to(dtype) if dtype is not None else torch.from_numpy(np.asarray(a)).cuda()


def _assert_mirror(got, k, groups, scope, exclude, keep=None):
    from coot_videotext_amd import compute_retrieval_topk_scoped
    idx, sc, sim = got
    want = compute_retrieval_topk_scoped(sim, k, groups, keep=keep, **({"exclude": scope} if exclude else {"only": scope}))
    assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (sim.shape[0], k)
    assert np.array_equal(idx, want[0]), np.argwhere(idx != want[0])[:5]
    assert bytes_equal(sc, want[1])


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_scoped_search_is_the_mirror_of_its_similarities(env, storage, normalize):
    torch, cva = env
    case = 0
    for n, dim in SHAPES:
        tq, index = _index(torch, cva, storage, normalize, n, dim)
        keep = np.random.RandomState(3).rand(n) < 0.6
        plain = {}
        for layout in LAYOUTS:
            groups = _groups(n, layout, seed=n)
            tg = _dev(torch, groups, torch.int32 if layout == "permuted" else None)
            for m, k in MK:
                k = min(k, n)
                if m not in plain:  # the similarities of the plain search, once per M
                    plain[m] = _host(torch, index.search(tq[:m], 1, want_sim=True)[2])[0]
                for exclude in (False, True):
                    for kp in (None, keep):
                        case += 1
                        scope = _scope(n, groups, m, seed=case)
                        ts = scope.tolist() if case % 5 == 0 else _dev(torch, scope, torch.int32 if case % 2 else torch.int64)
                        kw = {"exclude" if exclude else "only": ts}
                        got = _host(torch, *index.search_scoped(tq[:m], k, tg, keep=_dev(torch, kp), want_sim=True, **kw))
                        _assert_mirror(got, k, groups, scope, exclude, kp)
                        assert bytes_equal(got[2], plain[m]), (n, layout, m, k, exclude)
                        if m >= 3 and not exclude:  # an id that no row carries: nothing
                            assert (got[0][[1, m - 1]] == -1).all() and (got[1][[1, m - 1]] == NINF).all()


@pytest.mark.parametrize("storage", STORAGES)
def test_every_row_is_the_masked_search_of_that_query(env, storage):
    """The definition, on code that exists without this search: row i is index.search(q[i:i + 1], k, keep=eligible_i), the mask built on
    the host from groups and scope."""
    torch, cva = env
    n, dim, k = 1000, 64, 10
    tq, index = _index(torch, cva, storage, True, n, dim)
    groups = _groups(n, "runs")
    tg = _dev(torch, groups)
    for m in (16, 33):
        scope = _scope(n, groups, m, seed=m)
        for exclude in (False, True):
            idx, sc = _host(torch, *index.search_scoped(tq[:m], k, tg, **{"exclude" if exclude else "only": _dev(torch, scope)})[:2])
            for i in range(m):
                eligible = (groups == scope[i]) != exclude
                one = _host(torch, *index.search(tq[i:i + 1], k, keep=_dev(torch, eligible))[:2])
                assert bytes_equal(idx[i:i + 1], one[0]) and bytes_equal(sc[i:i + 1], one[1]), (m, exclude, i)


def test_the_result_does_not_depend_on_the_row_splits(env, splits):
    torch, cva = env
    n, dim = 1000, 64
    tq, index = _index(torch, cva, "bfloat16", True, n, dim)
    keep = _dev(torch, np.random.RandomState(4).rand(n) < 0.7)
    for layout in ("runs", "permuted", None):
        groups = _groups(n, layout, seed=2)
        tg = _dev(torch, groups)
        for m, k in ((16, 128), (3, 10)):
            scope = _dev(torch, _scope(n, groups, m, seed=9))
            for exclude in (False, True):
                runs = []
                for s in (1, 3, 0):
                    splits(s)
                    kw = {"exclude" if exclude else "only": scope}
                    runs.append(_host(torch, *index.search_scoped(tq[:m], k, tg, keep=keep, **kw)[:2]))
                    runs.append(_host(torch, *index.search_scoped(tq[:m], k, tg, keep=keep, want_sim=True, **kw)[:2]))
                for r in runs[1:]:
                    assert bytes_equal(r[0], runs[0][0]) and bytes_equal(r[1], runs[0][1]), (layout, m, exclude)


def test_blocks_without_an_eligible_row_are_skipped_with_the_same_result(env, splits):
    """only, adjacent rows: the wanted videos lie in the first and in the last of eight blocks, so the six between them have no eligible
    row and the sweep without sim leaves them before their first load; with sim every block is computed.  The same idx and scores,
    on one workgroup (which walks all eight blocks) and on the automatic splits.  k is more than a video's seven rows."""
    torch, cva = env
    n, dim, k, m = 1000, 64, 10, 16
    tq, index = _index(torch, cva, "float16", True, n, dim)
    groups = _groups(n, "runs")
    tg = _dev(torch, groups)
    first, last = np.unique(groups[:120]), np.unique(groups[900:])
    scope = np.concatenate([first[:8], last[-8:]])
    assert len(scope) == m and not np.isin(groups[128:896], scope).any()
    for s in (1, 0):
        splits(s)
        skipping = _host(torch, *index.search_scoped(tq[:m], k, tg, only=_dev(torch, scope))[:2])
        full = _host(torch, *index.search_scoped(tq[:m], k, tg, only=_dev(torch, scope), want_sim=True))
        _assert_mirror(full, k, groups, scope, False)
        assert bytes_equal(skipping[0], full[0]) and bytes_equal(skipping[1], full[1])
        for i in range(m):  # a video has seven rows (the last one six): all of them, then the unfilled tail
            c = int((groups == scope[i]).sum())
            assert c in (6, 7) and (groups[full[0][i, :c]] == scope[i]).all() and (full[0][i, c:] == -1).all() and (full[1][i, c:] == NINF).all()
        # every query scoped to an id that no row carries: every block is skipped, every slot unfilled
        idx, sc = _host(torch, *index.search_scoped(tq[:m], k, tg, only=[10 ** 6] * m)[:2])
        assert (idx == -1).all() and (sc == NINF).all()
        idx, sc = _host(torch, *index.search_scoped(tq[:33], k, tg, only=_dev(torch, np.full(33, -7)), keep=_dev(torch, np.ones(n, bool)))[:2])
        assert idx.shape == (33, k) and (idx == -1).all() and (sc == NINF).all()


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_equal_scores_come_back_larger_row_first(env, storage):
    """Rows 100 .. 129 are copies of rows 0 .. 29, in other groups: equal bytes, equal norms, equal scores."""
    torch, cva = env
    n, dim, k, m = 130, 37, 128, 16
    q, g = _planted(33, n, dim, 11)
    g = g.copy()
    g[100:] = g[:30]
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=True, storage=getattr(torch, storage))
    tq = torch.tensor(q[:m], device="cuda")
    groups = _groups(n, "runs")
    assert (groups[100:] != groups[:30]).all()
    # exclude an id that is neither copy's: both are eligible and adjacent, the larger row first
    scope = np.full(m, groups[50])
    got = _host(torch, *index.search_scoped(tq, k, _dev(torch, groups), exclude=_dev(torch, scope), want_sim=True))
    _assert_mirror(got, k, groups, scope, True)
    assert bytes_equal(got[2][:, 100:], got[2][:, :30])
    for i in range(m):
        row = got[0][i].tolist()
        for j in range(30):
            assert row.index(j + 100) + 1 == row.index(j), (i, j)
    # only: two ids per query cannot be asked for, so the copies share an id here
    both = groups.copy()
    both[100:] = groups[:30]
    scope = _scope(n, both[:30], m, seed=1)
    got = _host(torch, *index.search_scoped(tq, 14, _dev(torch, both), only=_dev(torch, scope), want_sim=True))
    _assert_mirror(got, 14, both, scope, False)
    for i in range(m):
        row = got[0][i][got[0][i] >= 0].tolist()
        small = [j for j in row if j < 30]
        assert (len(small) >= 2 or i in (1, m - 1)) and all(row.index(j + 100) + 1 == row.index(j) for j in small), (i, row)  # (1, m - 1: absent ids)


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_scoped_search_on_a_mutated_index(env, storage):
    """Removed rows are never returned; add with an extended table, then compact with groups[old rows]: both equal a fresh index on the
    same rows; and the function on the index's tensors gives the method's bytes."""
    torch, cva = env
    n, extra, dim, k, m = 600, 150, 64, 10, 17
    q, g = _planted(33, n + extra, dim, 51)
    tq, tg = torch.tensor(q[:m], device="cuda"), torch.tensor(g, device="cuda")
    st = getattr(torch, storage)
    groups_h = _groups(n + extra, "permuted", seed=8)
    groups = _dev(torch, groups_h)
    scope_h = _scope(n + extra, groups_h, m, seed=5)
    scope = _dev(torch, scope_h)

    def same(a, b):
        a, b = _host(torch, *a[:2]), _host(torch, *b[:2])
        assert all(bytes_equal(x, y) for x, y in zip(a, b))

    index = cva.GalleryIndex(tg[:n], normalize=True, storage=st, capacity=n + 50)
    assert index.add(tg[n:]) == n  # grows past the capacity
    fresh = cva.GalleryIndex(tg, normalize=True, storage=st)
    for kw in (dict(only=scope), dict(exclude=scope)):
        same(index.search_scoped(tq, k, groups, **kw), fresh.search_scoped(tq, k, groups, **kw))
        same(index.search_scoped(tq, k, groups, **kw), cva.retrieval_topk_scoped_device(tq, index.gallery, index.norms, groups, k, **kw))
    gone = np.arange(0, n + extra, 4)
    index.remove(gone.tolist())
    kept = np.ones(n + extra, bool)
    kept[gone] = False
    user = np.random.RandomState(6).rand(n + extra) < 0.8
    for exclude in (False, True):
        kw = {"exclude" if exclude else "only": scope}
        got = _host(torch, *index.search_scoped(tq, k, groups, want_sim=True, **kw))
        _assert_mirror(got, k, groups_h, scope_h, exclude, keep=kept)
        assert not np.isin(got[0], gone).any()
        got = _host(torch, *index.search_scoped(tq, k, groups, keep=_dev(torch, user), want_sim=True, **kw))
        _assert_mirror(got, k, groups_h, scope_h, exclude, keep=kept & user)
    removed = index.search_scoped(tq, k, groups, exclude=scope)
    old = index.compact()
    assert len(index) == len(old) < n + extra
    old64 = old.to(torch.int64)
    fresh = cva.GalleryIndex(tg[old64].contiguous(), normalize=True, storage=st)
    got = index.search_scoped(tq, k, groups[old64], exclude=scope)
    same(got, fresh.search_scoped(tq, k, groups[old64], exclude=scope))
    back = torch.where(got[0] >= 0, old[got[0].clamp(min=0).to(torch.int64)], got[0])  # in the old numbering: the search that skipped them
    same((back, got[1]), removed)


@pytest.mark.parametrize("storage", STORAGES)
def test_neighbors(env, storage):
    torch, cva = env
    n, dim, k = 1000, 64, 10
    _, g = _planted(33, n, dim, 11)
    g = g.copy()
    g[777] = g[3]  # an exact duplicate of row 3, in another video
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=True, storage=getattr(torch, storage))
    groups_h = _groups(n, "runs")
    groups = _dev(torch, groups_h)
    rows = [3, 0, 999, 500, 777] + list(range(100, 114))  # 19 rows: two slices
    trows = torch.tensor(rows, device="cuda")
    queries = index.gallery[trows].float()
    # groups=None: every row is its own id, so only the row itself is left out, and the duplicate leads
    idx, sc = index.neighbors(rows, k)
    want = index.search_scoped(queries, k, None, exclude=trows.to(torch.int32))
    idx, sc, widx, wsc = _host(torch, idx, sc, want[0], want[1])
    assert bytes_equal(idx, widx) and bytes_equal(sc, wsc)
    assert all(r not in idx[i] for i, r in enumerate(rows)) and (idx >= 0).all()
    assert idx[0, 0] == 777 and idx[4, 0] == 3
    dev_rows = _host(torch, *index.neighbors(trows, k))
    assert bytes_equal(dev_rows[0], idx) and bytes_equal(dev_rows[1], sc)
    # with groups: no row of the query's own video; the duplicate lies in another one and still leads
    keep = _dev(torch, np.random.RandomState(2).rand(n) < 0.9)
    for kp in (None, keep):
        idx, sc = index.neighbors(trows, k, groups=groups, keep=kp)
        want = index.search_scoped(queries, k, groups, exclude=groups[trows], keep=kp)
        idx, sc, widx, wsc = _host(torch, idx, sc, want[0], want[1])
        assert bytes_equal(idx, widx) and bytes_equal(sc, wsc)
        assert (idx >= 0).all() and (groups_h[idx] != groups_h[rows][:, None]).all()
    assert idx[0, 0] == 777 or not bool(keep[777])
    # a removed row may be asked about and is not returned
    index.remove([777])
    idx = _host(torch, index.neighbors([3, 777], k, groups=groups)[0])[0]
    assert 777 not in idx and 3 in idx[1]


class _CCall:
    """coot_retrieval_topk_scoped through ctypes on buffers with a known fill."""

    def __init__(self, torch, cva, n, dim):
        self.lib, self.n, self.dim = cva.lib.load(), n, dim
        q, g = _planted(33, n, dim, 11)
        self.q, self.g = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        self.size = self.lib.coot_retrieval_topk_scoped_workspace_bytes(16, n, dim, 128)
        self.ws = torch.zeros(self.size, dtype=torch.uint8, device="cuda")
        self.idx = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((17, 129), -7.0, device="cuda")
        self.scope = torch.zeros(17, dtype=torch.int32, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def __call__(self, m=16, k=128, dt=0, exclude=0, scope=-1, ws_bytes=None, ws_off=0, idx=-1):
        return self.lib.coot_retrieval_topk_scoped(self.q.data_ptr(), self.g.data_ptr(), dt, None, None, None, self.scope.data_ptr() if scope == -1 else scope,
                                                   exclude, m, self.n, self.dim, k, self.idx.data_ptr() if idx == -1 else idx, self.sc.data_ptr(), None,
                                                   self.ws.data_ptr() + ws_off, (self.size if ws_bytes is None else ws_bytes) - ws_off, self.st)


def test_scoped_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message, and every buffer as it was."""
    torch, cva = env
    n, dim = 300, 16
    c = _CCall(torch, cva, n, dim)
    exact = c.size - 256  # the layout itself: the reported size has one piece of slack
    cases = {"M = 17": (dict(m=17), "M = 17"), "M = 0": (dict(m=0), "M = 0"), "K = 0": (dict(k=0), "K = 0 is outside"),
             "K > N": (None, "K = 101 is outside 1 .. min(N = 100"), "K = 129": (dict(k=129), "K = 129 is outside"),
             "exclude = 2": (dict(exclude=2), "exclude = 2"), "exclude = -1": (dict(exclude=-1), "exclude = -1"), "null scope": (dict(scope=None), "null pointer"),
             "null output": (dict(idx=None), "null pointer"), "dtype": (dict(dt=7), "dtype = 7"), "one byte short": (dict(ws_bytes=exact - 1), "workspace too small"),
             "misaligned": (dict(ws_off=8), "16-byte aligned")}
    for what, (kw, part) in cases.items():
        if what == "K > N":
            small = _CCall(torch, cva, 100, dim)
            assert small(k=101, m=1) != 0, what
        else:
            assert c(**kw) != 0, what
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_topk_scoped:" in msg and part in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((c.idx == -7).all()) and bool((c.sc == -7.0).all()) and not bool(c.ws.any()), what
    assert c(ws_bytes=exact) == 0, c.lib.coot_last_error()  # the same buffers, accepted at exactly the layout's size
    torch.cuda.synchronize()
    idx = c.idx.view(-1)[:16 * 128].cpu().numpy().reshape(16, 128)
    assert (idx[:, 0] == 0).all() and (idx[:, 1:] == -1).all() and bool((c.idx.view(-1)[16 * 128:] == -7).all())  # groups NULL, scope 0: row 0 alone


def test_k_and_width_are_refused_on_the_host(env):
    """The messages of the shared check under the new names, before any launch."""
    torch, cva = env
    g = torch.zeros(5, 8, device="cuda")
    index = cva.GalleryIndex(g, normalize=False)
    groups = torch.zeros(5, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"GalleryIndex.search_scoped: queries of width 7, gallery of width 8"):
        index.search_scoped(torch.zeros(2, 7, device="cuda"), 2, groups, only=[0, 0])
    with pytest.raises(ValueError, match=r"retrieval_topk_scoped_device: queries of width 7, gallery of width 8"):
        cva.retrieval_topk_scoped_device(torch.zeros(2, 7, device="cuda"), g, None, groups, 2, exclude=[0, 0])
    q = torch.zeros(2, 8, device="cuda")
    for k in (0, 6, 129):
        with pytest.raises(ValueError, match=rf"GalleryIndex.search_scoped: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            index.search_scoped(q, k, groups, only=[0, 0])
        with pytest.raises(ValueError, match=rf"retrieval_topk_scoped_device: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            cva.retrieval_topk_scoped_device(q, g, None, None, k, exclude=[0, 0])
        with pytest.raises(ValueError, match=rf"GalleryIndex.neighbors: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            index.neighbors([0, 1], k)
    with pytest.raises(ValueError, match=r"only of shape \(3,\), 2 queries"):
        index.search_scoped(q, 2, groups, only=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="exclude has to hold integers .*not torch.float32"):
        index.search_scoped(q, 2, groups, exclude=torch.zeros(2, device="cuda"))
    with pytest.raises(TypeError, match="GalleryIndex.neighbors: rows of dtype torch.float32"):
        index.neighbors(torch.zeros(2, device="cuda"), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_scoped"):
        index.search_scoped(q, 2, groups.cpu(), only=[0, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_scoped"):
        index.search_scoped(q.cpu(), 2, groups, only=[0, 0])
    # one query as [d], one id
    idx, sc, _ = index.search_scoped(q[0], 2, None, exclude=[4])
    assert _host(torch, idx)[0].tolist() == [[3, 2]]
