"""The multi-vector top-K search (coot_retrieval_topk_multi; retrieval_topk_multi_device, GalleryIndex.search_multi) against its
definition: the similarities come back with want_sim=True, and group, scores, rows and row_scores have to be, byte for byte, the host
mirror compute_retrieval_topk_multi of those bytes (tests/test_cpu_topk_multi.py checks the mirror against a brute force), whatever
the storage, the mask, the sweep's row splits, the ranges of the table selection and the way the search is cut into library calls.
Shapes: N = 300 crosses 128-row blocks and row splits; d = 40 (fp32) takes 16-byte loads, d = 33 none; M = 19 sentences in the
paragraphs [0, 1), [1, 1), [1, 6), [6, 17), [17, 19): a single sentence, an empty paragraph, and one across the 16-sentence slices."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
N, M, G = 300, 19, 37
OFFSETS = [0, 1, 1, 6, 17, 19]
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
    """Sets rt_few_splits (the sweep) and rt_grouped_splits (the table selection) and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(few, table):
        assert lib.coot_set_option(b"rt_few_splits", few) == 0 and lib.coot_set_option(b"rt_grouped_splits", table) == 0
    try:
        yield set_
    finally:
        set_(0, 0)


def _dim(storage):
    return 40 if storage == "float32" else 33


def _groups(g_total, seed, wild=False):
    """Group ids of the N rows on the host (int64): runs of adjacent rows, scattered; wild: a fifth of them outside [0, G)."""
    rs = np.random.RandomState(seed)
    groups = (np.arange(N, dtype=np.int64) * g_total // N)[rs.permutation(N)] if seed % 2 else np.arange(N, dtype=np.int64) * g_total // N
    if wild:
        at = rs.rand(N) < 0.2
        groups[at] = rs.choice([-1, g_total, 2 ** 31 - 1, -2 ** 31, g_total + 7], size=int(at.sum()))
    return groups


def _index(torch, cva, storage, normalize, seed=7):
    q, g = _planted(M, N, _dim(storage), seed)
    return torch.tensor(q, device="cuda"), cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=normalize, storage=getattr(torch, storage))


def _search(torch, index, tq, offsets, k, groups, g_total, keep=None, dtype=None):
    """(group, scores, rows, row_scores, sim) on the host; groups / keep are host arrays (keep: bool)."""
    tg = torch.from_numpy(np.asarray(groups)).cuda()
    if dtype is not None:
        tg = tg.to(dtype)
    tk = None if keep is None else torch.from_numpy(keep).cuda()
    return _host(torch, *index.search_multi(tq, offsets, k, tg, num_groups=g_total, keep=tk, want_sim=True))


def _assert_mirror(got, offsets, k, groups, g_total, keep=None):
    from coot_videotext_amd import compute_retrieval_topk_multi
    grp, sc, rows, rsc, sim = got
    want = compute_retrieval_topk_multi(sim, offsets, k, groups, num_groups=g_total, keep=keep)
    assert grp.dtype == np.int32 and rows.dtype == np.int32 and sc.dtype == np.float32 and rsc.dtype == np.float32
    assert grp.shape == sc.shape == (len(offsets) - 1, k) and rows.shape == rsc.shape == (sim.shape[0], k)
    assert np.array_equal(grp, want[0]), np.argwhere(grp != want[0])[:5]
    assert bytes_equal(sc, want[1])
    assert np.array_equal(rows, want[2]), np.argwhere(rows != want[2])[:5]
    assert bytes_equal(rsc, want[3])


def _assert_consistent(got, offsets, groups):
    """What holds whatever the mirror says: the sums of the alignment's scores, in order, are the paragraph's scores, and every row
    named lies in the group of its slot."""
    grp, sc, rows, rsc, _ = got
    for p in range(len(offsets) - 1):
        i0, i1 = offsets[p], offsets[p + 1]
        filled = grp[p] >= 0
        if i1 == i0:
            assert not filled.any() and (sc[p] == NINF).all()
            continue
        s = np.zeros(grp.shape[1], np.float32)
        for i in range(i0, i1):
            s = s + rsc[i]
        assert bytes_equal(s[filled], sc[p][filled]) and (sc[p][~filled] == NINF).all()
        assert (rows[i0:i1][:, filled] >= 0).all() and (groups[rows[i0:i1][:, filled]] == grp[p][filled]).all()
        assert (rows[i0:i1][:, ~filled] == -1).all() and (rsc[i0:i1][:, ~filled] == NINF).all()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_multi_search_is_the_mirror_of_its_similarities(env, storage, normalize):
    torch, cva = env
    tq, index = _index(torch, cva, storage, normalize)
    keep = np.random.RandomState(3).rand(N) < 0.6
    cases = [(1, G, 0, False, None, None), (5, G, 1, False, keep, torch.int32), (5, G, 2, True, None, None), (5, G, 3, True, keep, torch.int32),
             (128, 150, 4, False, None, torch.int32), (128, 150, 5, True, keep, None)]
    for k, g_total, seed, wild, kp, dtype in cases:
        groups = _groups(g_total, seed, wild)
        got = _search(torch, index, tq, OFFSETS, k, groups, g_total, keep=kp, dtype=dtype)
        _assert_mirror(got, OFFSETS, k, groups, g_total, keep=kp)
        _assert_consistent(got, OFFSETS, groups)
        tg = torch.from_numpy(groups).cuda()
        tk = None if kp is None else torch.from_numpy(kp).cuda()
        grouped = _host(torch, *index.search_grouped(tq, min(k, 5), tg, num_groups=g_total, keep=tk, want_sim=True))
        assert bytes_equal(got[4], grouped[3]), (k, g_total)  # the similarities of the grouped search
        if k >= 5 and not wild:  # paragraph 0 is one sentence: where its scores do not tie, the grouped search of that sentence
            if len(set(grouped[2][0].tolist())) == 5:
                assert bytes_equal(got[0][0, :5], grouped[0][0]) and bytes_equal(got[2][0, :5], grouped[1][0]) and bytes_equal(got[1][0, :5], grouped[2][0])
    # index.remove combines with keep; num_groups=None: max(groups) + 1, one synchronisation; and the function under the method
    groups = _groups(G, 1)
    gone = np.arange(0, N, 3)
    index.remove(gone.tolist())
    both = keep.copy()
    both[gone] = False
    _assert_mirror(_search(torch, index, tq, OFFSETS, 5, groups, G, keep=keep), OFFSETS, 5, groups, G, keep=both)
    only = np.ones(N, bool)
    only[gone] = False
    _assert_mirror(_search(torch, index, tq, OFFSETS, 5, groups, G), OFFSETS, 5, groups, G, keep=only)
    index.restore()
    tg = torch.from_numpy(groups).cuda()
    a = _host(torch, *index.search_multi(tq, np.array(OFFSETS), 2, tg, want_sim=True))
    b = _host(torch, *cva.retrieval_topk_multi_device(tq, torch.tensor(OFFSETS), index.gallery, index.norms if normalize else None, tg, 2, num_groups=G,
                                                      want_sim=True))
    _assert_mirror(a, OFFSETS, 2, groups, G)
    assert all(bytes_equal(x, y) for x, y in zip(a, b))
    assert index.search_multi(tq, OFFSETS, 2, tg, num_groups=G)[4] is None
    # a whole group masked out, and nothing left at all
    few = np.isin(groups, [4, 30])
    got = _search(torch, index, tq, OFFSETS, 5, groups, G, keep=few)
    _assert_mirror(got, OFFSETS, 5, groups, G, keep=few)
    assert (np.sort(got[0][[0, 2, 3, 4], :2], axis=1) == [4, 30]).all() and (got[0][:, 2:] == -1).all() and (got[0][1] == -1).all()
    got = _search(torch, index, tq, OFFSETS, 5, groups, G, keep=np.zeros(N, bool))
    assert (got[0] == -1).all() and (got[1] == NINF).all() and (got[2] == -1).all() and (got[3] == NINF).all()


def test_alignment_is_the_grouped_search_inside_the_group(env):
    """rows / row_scores of (sentence i, group g) are search_grouped's best row with keep & (groups == g)."""
    torch, cva = env
    tq, index = _index(torch, cva, "bfloat16", True)
    groups = _groups(G, 1)
    keep = np.random.RandomState(5).rand(N) < 0.7
    grp, sc, rows, rsc, _ = _search(torch, index, tq, OFFSETS, 5, groups, G, keep=keep)
    tg = torch.from_numpy(groups).cuda()
    for i, r in ((0, 0), (3, 4), (15, 2), (16, 2), (18, 1)):
        p = np.searchsorted(OFFSETS, i, side="right") - 1
        g = int(grp[p, r])
        inside = torch.from_numpy(keep & (groups == g)).cuda()
        one = _host(torch, *index.search_grouped(tq[i:i + 1], 1, tg, num_groups=G, keep=inside)[:3])
        assert one[0][0, 0] == g and one[1][0, 0] == rows[i, r] and bytes_equal(one[2][0, 0], rsc[i, r])


@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
def test_result_does_not_depend_on_the_splits(env, splits, storage):
    """Sweep splits 1, 3 and automatic (3 blocks of 128 rows) x table ranges 1, 3, 7 and automatic (G = 150: up to 7 ranges of at least
    16 groups), at K = 5 and at K = 128 > a range's groups."""
    torch, cva = env
    tq, index = _index(torch, cva, storage, True)
    keep = np.random.RandomState(2).rand(N) < 0.7
    for k, g_total, seed, kp in ((5, G, 1, keep), (128, 150, 3, None), (5, 150, 2, None)):
        groups = _groups(g_total, seed)
        first = None
        for few in (0, 1, 3):
            for table in (0, 1, 3, 7):
                splits(few, table)
                got = _search(torch, index, tq, OFFSETS, k, groups, g_total, keep=kp)
                if first is None:
                    first = got
                    _assert_mirror(got, OFFSETS, k, groups, g_total, keep=kp)
                assert all(bytes_equal(x, y) for x, y in zip(got, first)), (k, g_total, few, table)


@pytest.mark.parametrize("storage", STORAGES)
def test_ties_the_larger_group_id_is_ahead(env, splits, storage):
    """Small integers: every dot product and every sum is exact in every storage.  The rows 0 .. 49 are repeated as 50 .. 99, 100 ..
    149 and 150 .. 199.  Group 2 t holds the rows 2 t and 2 t + 1 with their copies 50 + ..., group 2 t + 1 the copies 100 + ... and 150
    + ... of the same two rows: equal sums, so the larger id is ahead, and inside a group the later of equal rows answers."""
    torch, cva = env
    dim = _dim(storage)
    rs = np.random.RandomState(9)
    base = rs.randint(-2, 3, size=(50, dim)).astype(np.float32)
    g = np.concatenate([base, base, base, base, rs.randint(-2, 3, size=(N - 200, dim)).astype(np.float32)])
    groups = np.full(N, -1, np.int64)
    groups[:50] = 2 * (np.arange(50) // 2)          # group 2 t: rows 2 t, 2 t + 1 and their copies 50 + ...
    groups[50:100] = 2 * (np.arange(50) // 2)
    groups[100:150] = 2 * (np.arange(50) // 2) + 1  # group 2 t + 1: the copies 100 + ... and 150 + ... of the same rows
    groups[150:200] = 2 * (np.arange(50) // 2) + 1
    groups[200:] = 50 + np.arange(N - 200) % 7
    g_total = 57
    q = rs.randint(-2, 3, size=(M, dim)).astype(np.float32)
    index = cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=False, storage=getattr(torch, storage))
    tq = torch.tensor(q, device="cuda")
    for few, table in ((0, 0), (3, 3), (1, 1)):
        splits(few, table)
        got = _search(torch, index, tq, OFFSETS, 57, groups, g_total)
        _assert_mirror(got, OFFSETS, 57, groups, g_total)
        _assert_consistent(got, OFFSETS, groups)
        grp, sc, rows, rsc, sim = got
        assert np.array_equal(sim, q @ g.T)  # exact
        for p in (0, 2, 3, 4):
            at = {int(gid): r for r, gid in enumerate(grp[p])}
            for t in range(25):  # equal sums: the odd id directly ahead of the even one
                assert at[2 * t + 1] + 1 == at[2 * t] and sc[p, at[2 * t + 1]] == sc[p, at[2 * t]]
            for i in range(OFFSETS[p], OFFSETS[p + 1]):  # the later copy answers: 50 .. 99 for an even group, 150 .. 199 for an odd one
                assert ((rows[i, [at[2 * t] for t in range(25)]] >= 50) & (rows[i, [at[2 * t] for t in range(25)]] < 100)).all()
                assert (rows[i, [at[2 * t + 1] for t in range(25)]] >= 150).all()


def test_paragraph_split_returns_the_same_bytes(env, monkeypatch):
    """A table budget of 6 sentences x G: the calls [0, 3), [3, 4) (11 sentences: alone above the budget) and [4, 6) with a trailing
    empty paragraph; and of one entry: a call per paragraph, an empty one among them."""
    torch, cva = env
    from coot_videotext_amd import retrieval
    tq, index = _index(torch, cva, "float16", True)
    offsets = OFFSETS + [19]
    groups = _groups(G, 1, wild=True)
    keep = np.random.RandomState(4).rand(N) < 0.8
    whole = _search(torch, index, tq, offsets, 5, groups, G, keep=keep)
    _assert_mirror(whole, offsets, 5, groups, G, keep=keep)
    for budget, calls in ((6 * G, [(0, 3), (3, 4), (4, 6)]), (1, [(p, p + 1) for p in range(6)])):
        monkeypatch.setattr(retrieval, "MULTI_TABLE_ENTRIES", budget)
        assert retrieval._multi_calls(np.array(offsets), G) == calls
        cut = _search(torch, index, tq, offsets, 5, groups, G, keep=keep)
        assert all(bytes_equal(x, y) for x, y in zip(cut, whole)), budget


class _CCall:
    """coot_retrieval_topk_multi on raw buffers: one workspace, outputs filled with a sentinel."""

    def __init__(self, torch, cva, p, k, g_total, dim=33, tail=4096):
        self.torch, self.lib = torch, cva.lib.load()
        self.p, self.k, self.g_total, self.dim = p, k, g_total, dim
        q, g = _planted(M, N, dim, 41)
        self.q, self.g = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        self.gn = torch.empty(N, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        assert self.lib.coot_retrieval_row_norms(self.g.data_ptr(), N, dim, self.gn.data_ptr(), self.st) == 0
        self.size = self.lib.coot_retrieval_topk_multi_workspace_bytes(p, M, N, dim, k, g_total)
        self.ws = torch.full((self.size + tail,), 0xA5, dtype=torch.uint8, device="cuda")
        self.fill()

    def fill(self):
        torch = self.torch
        self.grp = torch.full((self.p + 1, 129), -7, dtype=torch.int32, device="cuda")
        self.sc = torch.full((self.p + 1, 129), -7.0, device="cuda")
        self.rows = torch.full((M + 1, 129), -7, dtype=torch.int32, device="cuda")
        self.rsc = torch.full((M + 1, 129), -7.0, device="cuda")

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.grp == -7).all()) and bool((self.sc == -7.0).all()) and bool((self.rows == -7).all()) and bool((self.rsc == -7.0).all())

    def __call__(self, groups, offsets, p=None, m=M, k=None, g_total=None, ws_bytes=None, dt=0, off_ptr=-1, grp_ptr=-1):
        k = self.k if k is None else k
        return self.lib.coot_retrieval_topk_multi(self.q.data_ptr(), self.g.data_ptr(), dt, self.gn.data_ptr(), None, groups.data_ptr(),
                                                  self.g_total if g_total is None else g_total, offsets.data_ptr() if off_ptr == -1 else off_ptr,
                                                  self.p if p is None else p, m, N, self.dim, k, self.grp.data_ptr() if grp_ptr == -1 else grp_ptr,
                                                  self.sc.data_ptr(), self.rows.data_ptr(), self.rsc.data_ptr(), None, self.ws.data_ptr(),
                                                  self.size if ws_bytes is None else ws_bytes, self.st)

    def results(self):
        self.torch.cuda.synchronize()
        out = []
        for t, n in ((self.grp, self.p), (self.sc, self.p), (self.rows, M), (self.rsc, M)):
            out.append(t.view(-1)[:n * self.k].cpu().numpy().copy().reshape(n, self.k))
        return out


def test_no_stale_state_and_refusals_write_nothing(env, splits):
    """Offsets A, a refused call, offsets B, A again, over one workspace: A's bytes both times, the mirror's; a refused call leaves the
    sentinel in every output; an accepted one stays inside the reported workspace size and the [P, K] / [M, K] it was given."""
    torch, cva = env
    from coot_videotext_amd import compute_retrieval_topk_multi
    p, k = 5, 5
    c = _CCall(torch, cva, p, k, G)
    groups_h = _groups(G, 1)
    groups = torch.from_numpy(groups_h.astype(np.int32)).cuda()
    off_a = torch.tensor(OFFSETS, dtype=torch.int32, device="cuda")
    off_b = torch.tensor([0, 4, 4, 9, 12, 19], dtype=torch.int32, device="cuda")
    runs = []
    for few, table in ((0, 0), (3, 2)):
        splits(few, table)
        for off in (off_a, off_b, off_a):
            c.fill()
            assert c(groups, off) == 0, c.lib.coot_last_error()
            runs.append(c.results())
            assert bool((c.grp.view(-1)[p * k:] == -7).all()) and bool((c.rows.view(-1)[M * k:] == -7).all())
            assert bool((c.sc.view(-1)[p * k:] == -7.0).all()) and bool((c.rsc.view(-1)[M * k:] == -7.0).all())
            if off is off_a:  # between A and B: refused calls on the same buffers
                c.fill()
                cases = {"K = 0": dict(k=0), "K = 129": dict(k=129), "offsets": dict(off_ptr=None), "P = 0": dict(p=0), "M = 0": dict(m=0),
                         "num_groups = 0": dict(g_total=0), "table": dict(g_total=2 ** 26), "workspace": dict(ws_bytes=c.size - 512), "dtype": dict(dt=7),
                         "null output": dict(grp_ptr=None)}
                for what, kw in cases.items():
                    assert c(groups, off, **kw) != 0, what
                    msg = c.lib.coot_last_error().decode()
                    part = {"offsets": "null pointer", "null output": "null pointer", "P = 0": "P = 0", "M = 0": "M = 0", "num_groups = 0": "num_groups = 0",
                            "table": "2^28", "workspace": "workspace too small", "dtype": "dtype = 7"}.get(what, "K = ")
                    assert "retrieval_topk_multi:" in msg and part in msg, (what, msg)
                misaligned = c.lib.coot_retrieval_topk_multi(c.q.data_ptr(), c.g.data_ptr(), 0, None, None, groups.data_ptr(), G, off.data_ptr(), p, M, N, c.dim, k,
                                                             c.grp.data_ptr(), c.sc.data_ptr(), c.rows.data_ptr(), c.rsc.data_ptr(), None, c.ws.data_ptr() + 8,
                                                             c.size - 8, c.st)
                assert misaligned != 0 and "16-byte aligned" in c.lib.coot_last_error().decode()
                assert c.untouched()
        assert bool((c.ws[c.size:] == 0xA5).all()), (few, table)
    for r in (runs[2], runs[3], runs[5]):
        assert all(bytes_equal(x, y) for x, y in zip(r, runs[0]))  # A, after B, and on other splits
    assert all(bytes_equal(x, y) for x, y in zip(runs[4], runs[1])) and not bytes_equal(runs[1][0], runs[0][0])
    splits(0, 0)
    for off, r in ((OFFSETS, runs[0]), ([0, 4, 4, 9, 12, 19], runs[1])):
        got = _host(torch, *cva.retrieval_topk_multi_device(c.q, off, c.g, c.gn, groups, k, num_groups=G, want_sim=True))
        assert all(bytes_equal(x, y) for x, y in zip(got[:4], r))
        want = compute_retrieval_topk_multi(got[4], off, k, groups_h, num_groups=G)
        assert all(bytes_equal(x, y) for x, y in zip(r, want))


def test_refused_calls_leave_the_outputs_untouched(env):
    torch, cva = env
    c = _CCall(torch, cva, 5, 5, G, tail=0)
    groups = torch.from_numpy(_groups(G, 1).astype(np.int32)).cuda()
    off = torch.tensor(OFFSETS, dtype=torch.int32, device="cuda")
    c.ws.zero_()
    for kw in (dict(k=0), dict(off_ptr=None), dict(k=129), dict(p=0), dict(p=65536), dict(m=0), dict(g_total=0), dict(g_total=-3), dict(ws_bytes=c.size - 512),
               dict(dt=7), dict(grp_ptr=None)):
        assert c(groups, off, **kw) != 0, kw
        assert c.untouched() and not bool(c.ws.any()), kw
    assert c(groups, off) == 0, c.lib.coot_last_error()
    assert not c.untouched()


def test_offsets_are_clamped_on_the_device(env):
    """Ordinary bad data for a kernel that clamps it: offsets out of range and out of order.  A paragraph is rows [clamp(off[p], 0, M),
    clamp(off[p + 1], that, M)); every index written is -1 or in range, a sentence that no paragraph holds is -1 / -inf.
    [0, -3, 40, 5]: the paragraphs are empty, all 19 sentences, empty.  [2, 5, 5, 30]: [2, 5), empty, [5, 19): sentences 0 and 1 are
    in none.  [0, 4, 2, 10]: [0, 4), empty, [2, 10): the sentences 10 .. 18 are in none."""
    torch, cva = env
    from coot_videotext_amd import compute_retrieval_topk_multi
    k = 5
    c = _CCall(torch, cva, 3, k, G)
    groups_h = _groups(G, 1, wild=True)
    groups = torch.from_numpy(groups_h.astype(np.int32)).cuda()
    sim = _host(torch, cva.retrieval_topk_multi_device(c.q, [0, M], c.g, c.gn, groups, 1, num_groups=G, want_sim=True)[4])[0]
    for bad, segments, uncovered in (([0, -3, 40, 5], [(0, 0), (0, 19), (19, 19)], []), ([2, 5, 5, 30], [(2, 5), (5, 5), (5, 19)], [0, 1]),
                                     ([0, 4, 2, 10], [(0, 4), (4, 4), (2, 10)], list(range(10, 19))),
                                     ([2 ** 31 - 1, -2 ** 31, -1, 2 ** 31 - 1], [(19, 19), (0, 0), (0, 19)], [])):
        c.fill()
        assert c(groups, torch.tensor(bad, dtype=torch.int32, device="cuda")) == 0, c.lib.coot_last_error()
        grp, sc, rows, rsc = c.results()
        assert ((grp >= -1) & (grp < G)).all() and ((rows >= -1) & (rows < N)).all()
        assert (rows[uncovered] == -1).all() and (rsc[uncovered] == NINF).all()
        # every paragraph is the search on its clamped segment alone; where the segments do not overlap, so is the alignment
        disjoint = all(a[1] <= b[0] or b[1] <= a[0] for x, a in enumerate(segments) for b in segments[x + 1:])
        for p, (i0, i1) in enumerate(segments):
            want = compute_retrieval_topk_multi(sim[i0:i1], [0, i1 - i0], k, groups_h, num_groups=G)
            assert bytes_equal(grp[p:p + 1], want[0]) and bytes_equal(sc[p:p + 1], want[1]), (bad, p)
            if disjoint:
                assert bytes_equal(rows[i0:i1], want[2]) and bytes_equal(rsc[i0:i1], want[3]), (bad, p)
        covered = [i for i in range(M) if i not in uncovered]
        assert (rows[covered] >= 0).any(axis=1).all() and (groups_h[rows[rows >= 0]] >= 0).all()


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_multi_search_on_a_mutated_index(env, storage):
    """add with an extended row-to-group table, then remove and compact with groups[old rows]: both equal a fresh index on the same rows."""
    torch, cva = env
    n, extra, dim, k, g_total = 240, 60, _dim(storage), 5, G
    q, g = _planted(M, n + extra, dim, 51)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    st = getattr(torch, storage)
    groups = torch.from_numpy(np.random.RandomState(8).randint(0, g_total, size=n + extra).astype(np.int64)).cuda()

    def same(a, b):
        a, b = _host(torch, *a[:4]), _host(torch, *b[:4])
        assert all(bytes_equal(x, y) for x, y in zip(a, b))

    index = cva.GalleryIndex(tg[:n], normalize=True, storage=st, capacity=n + 20)
    assert index.add(tg[n:]) == n  # grows past the capacity
    fresh = cva.GalleryIndex(tg, normalize=True, storage=st)
    same(index.search_multi(tq, OFFSETS, k, groups, num_groups=g_total), fresh.search_multi(tq, OFFSETS, k, groups, num_groups=g_total))
    index.remove(list(range(0, n + extra, 4)))
    removed = index.search_multi(tq, OFFSETS, k, groups, num_groups=g_total)
    old = index.compact()
    assert len(index) == len(old) < n + extra
    old64 = old.to(torch.int64)
    fresh = cva.GalleryIndex(tg[old64].contiguous(), normalize=True, storage=st)
    got = index.search_multi(tq, OFFSETS, k, groups[old64], num_groups=g_total)
    same(got, fresh.search_multi(tq, OFFSETS, k, groups[old64], num_groups=g_total))
    # and in the old numbering it is the search that skipped the removed rows
    back_rows = torch.where(got[2] >= 0, old[got[2].clamp(min=0).to(torch.int64)], got[2])
    same((got[0], got[1], back_rows, got[3]), removed)


def test_width_k_and_offsets_are_refused_on_the_host(env):
    torch, cva = env
    g = torch.zeros(5, 8, device="cuda")
    index = cva.GalleryIndex(g, normalize=False)
    groups = torch.zeros(5, dtype=torch.int32, device="cuda")
    q = torch.zeros(2, 8, device="cuda")
    for fn, call in (("GalleryIndex.search_multi", lambda q_, off, k, **kw: index.search_multi(q_, off, k, groups, **kw)),
                     ("retrieval_topk_multi_device", lambda q_, off, k, **kw: cva.retrieval_topk_multi_device(q_, off, g, None, groups, k, **kw))):
        with pytest.raises(ValueError, match=fn + ": offsets live on the host"):
            call(q, torch.tensor([0, 2], device="cuda"), 2, num_groups=1)
        with pytest.raises(ValueError, match=fn + ": offsets runs from 0 to 3"):
            call(q, [0, 3], 2, num_groups=1)
        with pytest.raises(ValueError, match=fn + ": queries of width 7, gallery of width 8"):
            call(torch.zeros(2, 7, device="cuda"), [0, 2], 2, num_groups=1)
        for k in (0, 6, 129):
            with pytest.raises(ValueError, match=fn + rf": k = {k} is outside 1 .. min\(N = 5, 128\)"):
                call(q, [0, 2], k, num_groups=1)
        with pytest.raises(ValueError, match="one flag per row"):
            call(q, [0, 2], 2, num_groups=1, keep=torch.ones(4, dtype=torch.bool, device="cuda"))
        with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_multi"):
            call(q.cpu(), [0, 2], 2, num_groups=1)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_multi"):
        index.search_multi(q, [0, 2], 2, groups.cpu(), num_groups=1)
    with pytest.raises(ValueError, match="at least one group"):
        cva.retrieval_topk_multi_device(q, [0, 2], g, None, groups, 2, num_groups=0)
    from coot_videotext_amd import retrieval
    with pytest.raises(ValueError, match="one paragraph has at most 2\\^28"):
        cva.retrieval_topk_multi_device(q, [0, 2], g, None, groups, 2, num_groups=retrieval.MULTI_TABLE_ENTRIES_MAX // 2 + 1)
    # nothing but empty paragraphs: no sentence, every slot the tail
    got = _host(torch, *index.search_multi(torch.zeros(0, 8, device="cuda"), [0, 0, 0], 2, groups, num_groups=1)[:4])
    assert got[0].shape == (2, 2) and (got[0] == -1).all() and (got[1] == NINF).all() and got[2].shape == (0, 2) and got[3].shape == (0, 2)
