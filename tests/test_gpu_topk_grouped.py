"""The grouped top-K search (coot_retrieval_topk_grouped; retrieval_topk_grouped_device, GalleryIndex.search_grouped) against its
definition: the similarities come back with want_sim=True, and group, idx and scores have to be, byte for byte, the host mirror
compute_retrieval_topk_grouped of those bytes (tests/test_cpu_topk_grouped.py checks the mirror against a brute force), whatever the
storage, the group layout, the mask, the sweep's row splits and the ranges of the table selection.  With every row its own group the
result is index.search's, byte for byte."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
# N: several 128-row blocks with a short last one; one block and two rows; fewer rows than lanes.  d = 64: 16-byte loads; d = 37: none,
# and a padded last chunk
SHAPES = [(1000, 64), (130, 37), (5, 37)]
# M = 1, 3, 16: one call; 17 and 33: slices of 16 over one workspace.  K = 1, 10, 128 (clipped to N)
MK = [(1, 1), (3, 10), (16, 128), (17, 10), (33, 128)]


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def splits(env):
    """Sets rt_few_splits (the sweep) and rt_grouped_splits (the table selection) and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(few, table):
        assert lib.coot_set_option(b"rt_few_splits", few) == 0 and lib.coot_set_option(b"rt_grouped_splits", table) == 0
    yield set_
    set_(0, 0)


def _layouts(n, seed):
    """name -> (group ids int64 [N] on the host, G)."""
    rs = np.random.RandomState(seed)
    runs = []
    while sum(runs) < n:
        runs.append(int(rs.randint(1, 10)))
    contiguous = np.repeat(np.arange(len(runs)), runs)[:n].astype(np.int64)
    g_total = int(contiguous.max()) + 1
    return {"contiguous": (contiguous, g_total), "permuted": (contiguous[rs.permutation(n)], g_total),
            "one group": (np.zeros(n, np.int64), 1), "arange": (np.arange(n, dtype=np.int64), n)}


def _search(torch, index, tq, k, groups, g_total, keep=None, dtype=None):
    """(group, idx, scores, sim) on the host; groups / keep are host arrays (keep: bool)."""
    tg = torch.from_numpy(np.asarray(groups)).cuda()
    if dtype is not None:
        tg = tg.to(dtype)
    tk = None if keep is None else torch.from_numpy(keep).cuda()
    return _host(torch, *index.search_grouped(tq, k, tg, num_groups=g_total, keep=tk, want_sim=True))


def _assert_mirror(got, k, groups, g_total, keep=None):
    from coot_videotext_amd import compute_retrieval_topk_grouped
    grp, idx, sc, sim = got
    want = compute_retrieval_topk_grouped(sim, k, groups, num_groups=g_total, keep=keep)
    assert grp.dtype == np.int32 and idx.dtype == np.int32 and sc.dtype == np.float32 and grp.shape == idx.shape == sc.shape == (sim.shape[0], k)
    assert np.array_equal(grp, want[0]), np.argwhere(grp != want[0])[:5]
    assert np.array_equal(idx, want[1]), np.argwhere(idx != want[1])[:5]
    assert bytes_equal(sc, want[2])


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_grouped_search_is_the_mirror_of_its_similarities(env, storage, normalize):
    torch, cva = env
    for n, dim in SHAPES:
        q, g = _planted(33, n, dim, n + dim)
        tq_all, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        index = cva.GalleryIndex(tg, normalize=normalize, storage=getattr(torch, storage))
        keep = np.random.RandomState(n).rand(n) < 0.6
        for li, (name, (groups, g_total)) in enumerate(_layouts(n, n + 1).items()):
            for ci, (m, k) in enumerate(MK):
                k = min(k, n)
                tq = tq_all[:m]
                kp = keep if (li + ci) % 2 else None  # every layout and every (M, K) with and without a mask
                got = _search(torch, index, tq, k, groups, g_total, keep=kp, dtype=torch.int32 if ci % 2 else None)
                _assert_mirror(got, k, groups, g_total, keep=kp)
                tk = None if kp is None else torch.from_numpy(kp).cuda()
                row = _host(torch, *index.search(tq, k, want_sim=True, keep=tk))
                assert bytes_equal(got[3], row[2]), (name, m, k)  # the similarities of the row search
                if name == "arange":  # every row its own group: the row search, byte for byte
                    assert bytes_equal(got[1], row[0]) and bytes_equal(got[2], row[1]) and bytes_equal(got[0], got[1]), (n, m, k)
                if name == "one group" and kp is None:  # slot 0 is the top-1 row, the rest is unfilled
                    top = _host(torch, *index.search(tq, 1)[:2])
                    assert bytes_equal(got[1][:, :1], top[0]) and bytes_equal(got[2][:, :1], top[1]) and (got[0][:, 0] == 0).all()
                    assert (got[0][:, 1:] == -1).all() and (got[1][:, 1:] == -1).all() and np.isneginf(got[2][:, 1:]).all()
    # num_groups=None: max(groups) + 1, one synchronisation; and the function under the method, on the index's own tensors
    groups, g_total = _layouts(n, 3)["permuted"]
    tgr = torch.from_numpy(groups).cuda()
    a = _host(torch, *index.search_grouped(tq_all[:3], 2, tgr, want_sim=True))
    b = _host(torch, *cva.retrieval_topk_grouped_device(tq_all[:3], index.gallery, index.norms if normalize else None, tgr, 2, num_groups=g_total,
                                                        want_sim=True))
    _assert_mirror(a, 2, groups, g_total)
    assert all(bytes_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_result_does_not_depend_on_the_splits(env, splits, storage):
    """Sweep splits 1, 3 and automatic (8 blocks of 128 rows: with 3 splits a group of 300 rows straddles workgroups) x table ranges
    1, 3, 40 (two merge rounds) and automatic, at G = 700 (more than one range) and at 4 large groups."""
    torch, cva = env
    n, dim = 1000, 64
    q, g = _planted(16, n, dim, 11)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    index = cva.GalleryIndex(tg, normalize=True, storage=getattr(torch, storage))
    rs = np.random.RandomState(2)
    layouts = {"runs, G = 700": (np.arange(n, dtype=np.int64) * 700 // n, 700), "scattered, G = 700": (rs.permutation(n).astype(np.int64) % 700, 700),
               "four groups": (np.arange(n, dtype=np.int64) // 300, 4)}
    keep = rs.rand(n) < 0.7
    for name, (groups, g_total) in layouts.items():
        for m, k, kp in ((16, 128, None), (3, 10, keep)):
            first = None
            for few in (1, 3, 0):
                for table in (1, 3, 40, 0):
                    splits(few, table)
                    got = _search(torch, index, tq[:m], k, groups, g_total, keep=kp)
                    if first is None:
                        first = got
                        _assert_mirror(got, k, groups, g_total, keep=kp)
                    assert all(bytes_equal(x, y) for x, y in zip(got, first)), (name, m, k, few, table)


@pytest.mark.parametrize("storage", STORAGES)
def test_ties_the_later_row_is_ahead(env, splits, storage):
    """Small integers: every dot product is exact in every storage, and duplicate rows tie exactly.  Inside a group the later of two
    equal rows represents it; of two groups whose best rows are equal the one with the later row is ahead."""
    torch, cva = env
    n, dim = 300, 37
    rs = np.random.RandomState(9)
    g = rs.randint(-2, 3, size=(n, dim)).astype(np.float32)
    groups = (np.arange(n) // 5).astype(np.int64)  # 60 groups of 5 adjacent rows
    g_total = 60
    big = np.full(dim, 2.0, np.float32)
    g[51] = g[53] = big            # group 10: rows 51 and 53 equal
    g[131] = g[204] = big          # and equal to rows of the groups 26 and 40
    g[7] = g[9]                    # a random duplicate inside group 1
    g[140] = g[290]                # and across the groups 28 and 58
    q = rs.randint(-2, 3, size=(6, dim)).astype(np.float32)
    q[0] = 1.0                     # score 2 dim at the four big rows, below it everywhere else
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=False, storage=getattr(torch, storage))
    tq = torch.tensor(q, device="cuda")
    for few, table in ((0, 0), (3, 3), (1, 1)):
        splits(few, table)
        for layout in (groups, groups[::-1].copy()):
            got = _search(torch, index, tq, 60, layout, g_total)
            _assert_mirror(got, 60, layout, g_total)
            assert np.array_equal(got[3], q @ g.T)  # exact
            for i in range(6):  # every group through its best row, the later of equal ones
                for grp, idx in zip(got[0][i], got[1][i]):
                    rows = np.nonzero(layout == grp)[0]
                    s = got[3][i, rows]
                    assert idx == rows[s == s.max()].max()
        got = _search(torch, index, tq, 60, groups, g_total)
        assert got[0][0, :3].tolist() == [40, 26, 10] and got[1][0, :3].tolist() == [204, 131, 53] and (got[2][0, :3] == 2.0 * dim).all()


def test_mask_and_removed_rows(env):
    torch, cva = env
    n, dim, k = 1000, 64, 10
    q, g = _planted(3, n, dim, 21)
    q, g = q.copy(), g.copy()
    q[0] = g[0] + 0.1 * q[0]
    g[1] = 0.9 * g[0] + 0.1 * g[1]  # query 0 lies on row 0, and row 1 of the same group next to it: the group leads the list with and without its best row
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    index = cva.GalleryIndex(tg, normalize=True)
    groups = (np.arange(n) // 5).astype(np.int64)
    g_total = n // 5
    base = _search(torch, index, tq, k, groups, g_total)
    _assert_mirror(base, k, groups, g_total)
    sim = base[3]
    # without the best row of query 0's best group, the group is represented by its second row
    g0, r0 = int(base[0][0, 0]), int(base[1][0, 0])
    keep = np.ones(n, bool)
    keep[r0] = False
    got = _search(torch, index, tq, k, groups, g_total, keep=keep)
    _assert_mirror(got, k, groups, g_total, keep=keep)
    rows = np.array([r for r in range(g0 * 5, g0 * 5 + 5) if r != r0])
    second = rows[np.argmax(sim[0, rows])]
    at = np.nonzero(got[0][0] == g0)[0]
    assert len(at) == 1 and got[1][0, at[0]] == second and got[2][0, at[0]] == sim[0, second] and r0 not in got[1]
    # a group with every row removed disappears
    keep[g0 * 5:g0 * 5 + 5] = False
    got = _search(torch, index, tq, k, groups, g_total, keep=keep)
    _assert_mirror(got, k, groups, g_total, keep=keep)
    assert g0 not in got[0][0] and got[0][0, 0] == base[0][0, 1]
    # index.remove and a per-search keep combine
    gone = np.arange(0, n, 3)
    index.remove(gone.tolist())
    both = keep.copy()
    both[gone] = False
    got = _search(torch, index, tq, k, groups, g_total, keep=keep)
    _assert_mirror(got, k, groups, g_total, keep=both)
    only = np.ones(n, bool)
    only[gone] = False
    got = _search(torch, index, tq, k, groups, g_total)
    _assert_mirror(got, k, groups, g_total, keep=only)
    index.restore()
    # fewer than k groups left: rows of three groups kept
    few = np.isin(groups, [4, 77, 150])
    got = _search(torch, index, tq, k, groups, g_total, keep=few)
    _assert_mirror(got, k, groups, g_total, keep=few)
    assert (np.sort(got[0][:, :3], axis=1) == [4, 77, 150]).all()
    assert (got[0][:, 3:] == -1).all() and (got[1][:, 3:] == -1).all() and np.isneginf(got[2][:, 3:]).all()
    got = _search(torch, index, tq, k, groups, g_total, keep=np.zeros(n, bool))
    assert (got[0] == -1).all() and (got[1] == -1).all() and np.isneginf(got[2]).all()


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_group_ids_out_of_range_are_never_returned(env, dtype):
    torch, cva = env
    n, dim, k = 1000, 37, 128
    q, g = _planted(16, n, dim, 31)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    index = cva.GalleryIndex(tg, normalize=True, storage=torch.bfloat16)
    rs = np.random.RandomState(4)
    g_total = 150
    groups = rs.randint(0, g_total, size=n).astype(np.int64)
    wild = rs.rand(n) < 0.3
    groups[wild] = rs.choice([-1, g_total, 2 ** 31 - 1, -2 ** 31, g_total + 7], size=int(wild.sum()))
    got = _search(torch, index, tq, k, groups, g_total, dtype=getattr(torch, dtype))
    _assert_mirror(got, k, groups, g_total)
    filled = got[1] >= 0
    assert not wild[got[1][filled]].any() and ((got[0][filled] >= 0) & (got[0][filled] < g_total)).all()
    keep = rs.rand(n) < 0.5
    got = _search(torch, index, tq, k, groups, g_total, keep=keep, dtype=getattr(torch, dtype))
    _assert_mirror(got, k, groups, g_total, keep=keep)
    got = _search(torch, index, tq, 5, np.full(n, -1, np.int64), 3)  # nothing in range
    assert (got[0] == -1).all() and (got[1] == -1).all() and np.isneginf(got[2]).all()


class _CCall:
    """coot_retrieval_topk_grouped on raw buffers: one workspace, outputs filled with a sentinel."""

    def __init__(self, torch, cva, m, n, dim, k, g_total, tail=4096):
        self.torch, self.lib = torch, cva.lib.load()
        self.m, self.n, self.dim, self.k, self.g_total = m, n, dim, k, g_total
        q, g = _planted(17, n, dim, 41)
        self.q, self.g = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        self.gn = torch.empty(n, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        assert self.lib.coot_retrieval_row_norms(self.g.data_ptr(), n, dim, self.gn.data_ptr(), self.st) == 0
        self.size = self.lib.coot_retrieval_topk_grouped_workspace_bytes(m, n, dim, k, g_total)
        self.ws = torch.full((self.size + tail,), 0xA5, dtype=torch.uint8, device="cuda")
        self.grp = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
        self.idx = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((17, 129), -7.0, device="cuda")

    def __call__(self, groups, m=None, k=None, g_total=None, ws_bytes=None, dt=0, grp_ptr=-1, keep=None):
        m, k = self.m if m is None else m, self.k if k is None else k
        return self.lib.coot_retrieval_topk_grouped(self.q.data_ptr(), self.g.data_ptr(), dt, self.gn.data_ptr(), None if keep is None else keep.data_ptr(),
                                                    groups.data_ptr(), self.g_total if g_total is None else g_total, m, self.n, self.dim, k,
                                                    self.grp.data_ptr() if grp_ptr == -1 else grp_ptr, self.idx.data_ptr(), self.sc.data_ptr(), None,
                                                    self.ws.data_ptr(), self.size if ws_bytes is None else ws_bytes, self.st)

    def results(self):
        self.torch.cuda.synchronize()
        e = self.m * self.k
        return [t.view(-1)[:e].cpu().numpy().copy() for t in (self.grp, self.idx, self.sc)]


def test_workspace_bounds_and_no_stale_state(env, splits):
    """The call stays inside the reported workspace size (the tail of a longer tensor keeps its 0xA5 bytes, at the largest list
    layout: 40 ranges), and nothing survives in the workspace: groups A, then B, then A again on one workspace gives A's bytes."""
    torch, cva = env
    n, dim, k, g_total = 1000, 37, 128, 700
    c = _CCall(torch, cva, 16, n, dim, k, g_total)
    rs = np.random.RandomState(6)
    ga = torch.from_numpy((rs.permutation(n) % g_total).astype(np.int32)).cuda()
    gb = torch.from_numpy((np.arange(n) // 2).astype(np.int32)).cuda()
    runs = []
    for few, table in ((0, 0), (3, 40), (1, 1)):
        splits(few, table)
        for groups in (ga, gb, ga):
            assert c(groups) == 0, c.lib.coot_last_error()
            runs.append(c.results())
        assert bool((c.ws[c.size:] == 0xA5).all()), (few, table)
    for r in runs[2::3] + runs[3::3]:
        assert all(bytes_equal(x, y) for x, y in zip(r, runs[0]))  # A, on every split setting and after B
    assert not bytes_equal(runs[1][1], runs[0][1])
    splits(0, 0)
    got = _host(torch, *cva.retrieval_topk_grouped_device(c.q[:16], c.g, c.gn, ga, k, num_groups=g_total)[:3])
    assert all(bytes_equal(x.reshape(-1), y) for x, y in zip(got, runs[0]))


def test_grouped_refusals_write_nothing(env):
    torch, cva = env
    n, dim = 300, 16
    c = _CCall(torch, cva, 16, n, dim, 128, 50, tail=0)
    c.ws.zero_()
    groups = torch.from_numpy((np.arange(n) % 50).astype(np.int32)).cuda()
    cases = {"M = 17": dict(m=17), "M = 0": dict(m=0), "K = 0": dict(k=0), "K = 129": dict(k=129), "num_groups = 0": dict(g_total=0),
             "num_groups = -3": dict(g_total=-3), "workspace": dict(ws_bytes=c.size - 512), "dtype": dict(dt=7), "null output": dict(grp_ptr=None)}
    for what, kw in cases.items():
        assert c(groups, **kw) != 0, what
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_topk_grouped:" in msg, (what, msg)
        part = {"M = 17": "M = 17", "M = 0": "M = 0", "workspace": "workspace too small", "null output": "null pointer", "dtype": "dtype = 7",
                "num_groups = 0": "num_groups = 0", "num_groups = -3": "num_groups = -3"}.get(what, "K = ")
        assert part in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((c.grp == -7).all()) and bool((c.idx == -7).all()) and bool((c.sc == -7.0).all()) and not bool(c.ws.any()), what
    null_groups = c.lib.coot_retrieval_topk_grouped(c.q.data_ptr(), c.g.data_ptr(), 0, None, None, None, 50, 16, n, dim, 10, c.grp.data_ptr(), c.idx.data_ptr(),
                                                    c.sc.data_ptr(), None, c.ws.data_ptr(), c.size, c.st)
    assert null_groups != 0 and "null pointer" in c.lib.coot_last_error().decode()
    misaligned = c.lib.coot_retrieval_topk_grouped(c.q.data_ptr(), c.g.data_ptr(), 0, None, None, groups.data_ptr(), 50, 16, n, dim, 10, c.grp.data_ptr(),
                                                   c.idx.data_ptr(), c.sc.data_ptr(), None, c.ws.data_ptr() + 8, c.size - 8, c.st)
    assert misaligned != 0 and "16-byte aligned" in c.lib.coot_last_error().decode()
    torch.cuda.synchronize()
    assert bool((c.grp == -7).all()) and not bool(c.ws.any())
    assert c(groups) == 0, c.lib.coot_last_error()  # the same buffers, accepted: 50 groups at K = 128
    grp, idx, sc = c.results()
    grp, idx = grp.reshape(16, 128), idx.reshape(16, 128)
    assert (np.sort(grp[:, :50], axis=1) == np.arange(50)).all() and (idx[:, :50] % 50 == grp[:, :50]).all()
    assert (grp[:, 50:] == -1).all() and (idx[:, 50:] == -1).all() and bool((c.grp.view(-1)[16 * 128:] == -7).all())


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_grouped_search_on_a_mutated_index(env, storage):
    """add with an extended row-to-group table, then compact with groups[old rows]: both equal a fresh index on the same rows."""
    torch, cva = env
    n, extra, dim, k = 600, 150, 64, 10
    q, g = _planted(5, n + extra, dim, 51)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    st = getattr(torch, storage)
    rs = np.random.RandomState(8)
    g_total = 120
    groups = torch.from_numpy(rs.randint(0, g_total, size=n + extra).astype(np.int64)).cuda()

    def same(a, b):
        a, b = _host(torch, *a[:3]), _host(torch, *b[:3])
        assert all(bytes_equal(x, y) for x, y in zip(a, b))

    index = cva.GalleryIndex(tg[:n], normalize=True, storage=st, capacity=n + 50)
    assert index.add(tg[n:]) == n  # grows past the capacity
    fresh = cva.GalleryIndex(tg, normalize=True, storage=st)
    same(index.search_grouped(tq, k, groups, num_groups=g_total), fresh.search_grouped(tq, k, groups, num_groups=g_total))
    index.remove(list(range(0, n + extra, 4)))
    removed = index.search_grouped(tq, k, groups, num_groups=g_total)
    old = index.compact()
    assert len(index) == len(old) < n + extra
    old64 = old.to(torch.int64)
    fresh = cva.GalleryIndex(tg[old64].contiguous(), normalize=True, storage=st)
    got = index.search_grouped(tq, k, groups[old64], num_groups=g_total)
    same(got, fresh.search_grouped(tq, k, groups[old64], num_groups=g_total))
    # and in the old numbering it is the search that skipped the removed rows
    back = (got[0], old[got[1].to(torch.int64)], got[2])
    same(back, removed)


def test_width_and_k_are_refused_on_the_host(env):
    """The messages of GalleryIndex.search under the new names, before any launch."""
    torch, cva = env
    g = torch.zeros(5, 8, device="cuda")
    index = cva.GalleryIndex(g, normalize=False)
    groups = torch.zeros(5, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"GalleryIndex.search_grouped: queries of width 7, gallery of width 8"):
        index.search_grouped(torch.zeros(2, 7, device="cuda"), 2, groups, num_groups=1)
    with pytest.raises(ValueError, match=r"retrieval_topk_grouped_device: queries of width 7, gallery of width 8"):
        cva.retrieval_topk_grouped_device(torch.zeros(2, 7, device="cuda"), g, None, groups, 2, num_groups=1)
    q = torch.zeros(2, 8, device="cuda")
    for k in (0, 6, 129):
        with pytest.raises(ValueError, match=rf"GalleryIndex.search_grouped: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            index.search_grouped(q, k, groups, num_groups=1)
        with pytest.raises(ValueError, match=rf"retrieval_topk_grouped_device: k = {k} is outside 1 .. min\(N = 5, 128\)"):
            cva.retrieval_topk_grouped_device(q, g, None, groups, k, num_groups=1)
    with pytest.raises(ValueError, match="one flag per row"):
        index.search_grouped(q, 2, groups, num_groups=1, keep=torch.ones(4, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="bool or torch.uint8"):
        cva.retrieval_topk_grouped_device(q, g, None, groups, 2, num_groups=1, keep=torch.ones(5, device="cuda"))
    with pytest.raises(ValueError, match="at least one group"):
        cva.retrieval_topk_grouped_device(q, g, None, groups, 2, num_groups=0)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_grouped"):
        index.search_grouped(q, 2, groups.cpu(), num_groups=1)
