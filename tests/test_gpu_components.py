"""The duplicate clusters (GalleryIndex.components, deduplicate, retrieval_components_device; coot_retrieval_components) against their
definition: the reference similarities are those that index.search(index.gallery.float(), 1, want_sim=True) returns, and labels have to
be, byte for byte, the host mirror compute_retrieval_components of those bytes and a host union-find over the pairs index.self_join
returns for the same arguments.
Shapes, planted copies, thresholds and group tables are those of tests/test_gpu_self_join.py (its helpers, and its cached indexes, by
import), plus (1, 16): copies sit across the 63 / 64 and 127 / 128 edges and in the last rows, thresholds are taken from the reference
bytes (+-inf, NaN, max, median, between).  The graphs of the second part hold only 0 and 1 and are not normalised, so every score is 0,
1 or 2 exactly in every storage: a path of 300 rows in natural, reversed and permuted row order, a star whose centre is the last row,
and two interleaved paths joined by one edge in the last block."""
import numpy as np
import pytest

from tests import test_gpu_self_join as sj
from tests.retrieval_cases import bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = sj.STORAGES
SHAPES = sj.SHAPES + [(1, 16)]
_dev = sj._dev


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


_ONE = {}


def _case(torch, cva, storage, normalize, n, dim):
    """(the index, the reference similarities [N, N] on the host, the thresholds [N]): the self-join tests' cases, and one row."""
    if n > 1:
        return sj._case(torch, cva, storage, normalize, n, dim)
    key = (storage, normalize, dim)
    if key not in _ONE:
        index = cva.GalleryIndex(torch.tensor(_planted(1, 1, dim, 11)[1].copy(), device="cuda"), normalize=normalize, storage=getattr(torch, storage))
        sim = _host(torch, index.search(index.gallery.float(), 1, want_sim=True)[2])[0]
        _ONE[key] = (index, sim, sj._thresholds(sim))
    return _ONE[key]


def _uf_labels(n, off, rows, ok):
    """A host union-find over a CSR pair list; rows with ok false are -1."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        for j in rows[off[i]:off[i + 1]].tolist():
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    lab = np.array([find(i) for i in range(n)], np.int32).reshape(n)
    lab[~ok] = -1
    return lab


def _same(got, want, what=None):
    assert got.dtype == np.int32 and bytes_equal(got, want), (what, np.argwhere(got != want)[:5].ravel(), got[got != want][:5], want[got != want][:5])


class _Blocks:
    """Sets rt_comp_blocks_per_wg and restores the automatic choice afterwards."""

    def __init__(self, cva, n):
        self.lib, self.n = cva.lib.load(), n

    def __enter__(self):
        assert self.lib.coot_set_option(b"rt_comp_blocks_per_wg", self.n) == 0

    def __exit__(self, *exc):
        assert self.lib.coot_set_option(b"rt_comp_blocks_per_wg", 0) == 0


# ---- 1. random galleries with planted copies ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_labels_are_the_mirror_and_a_union_find_over_the_self_join(env, storage, normalize):
    torch, cva = env
    case = 0
    for n, dim in SHAPES:
        index, sim, thr = _case(torch, cva, storage, normalize, n, dim)
        keep = np.random.RandomState(3).rand(n) < 0.6
        gone = np.arange(1, n, 3)
        case += 1  # (seven per shape: what alternates does so from shape to shape too)
        for kp in (None, keep):
            for gk in (None, "runs", "scattered"):
                case += 1
                groups = sj._groups(n, gk)
                own = np.ones(n, bool)
                tt = [thr.tolist(), thr, _dev(torch, thr)][case % 3]  # a host list, a host array, a device tensor
                try:
                    if case % 2:
                        index.remove(gone.tolist())
                        own[gone] = False
                    ok = own if kp is None else own & kp
                    got = _host(torch, index.components(tt, keep=_dev(torch, kp), groups=_dev(torch, groups)))[0]
                    assert got.shape == (n,)
                    _same(got, cva.compute_retrieval_components(sim, thr, keep=ok, groups=groups), ("mirror", n, dim, case))
                    off, rows, _ = _host(torch, *index.self_join(tt, keep=_dev(torch, kp), groups=_dev(torch, groups)))
                    _same(got, _uf_labels(n, off, rows, ok), ("self_join", n, dim, case))
                    assert ((got == -1) == ~ok).all() and (got[ok] <= np.arange(n)[ok]).all() and (got[got[ok]] == got[ok]).all()
                    if n >= 64 and kp is None and gk is None and not case % 2:  # what the planted rows are there for
                        for a, b in sj._dups(n):
                            if sj.KINDS[a % len(sj.KINDS)] not in ("+inf", "nan"):
                                assert got[a] == got[b], (a, b)
                finally:
                    index.restore()
        whole = _host(torch, cva.retrieval_components_device(index.gallery, index.norms if normalize else None, float(thr[n // 2]), keep=_dev(torch, keep)))[0]
        _same(whole, cva.compute_retrieval_components(sim, thr[n // 2], keep=keep), ("scalar", n, dim))
        # one threshold that leaves clusters of a few rows: an exact score, the (N / 8)-th best of all pairs
        upper = np.sort(sim[np.triu_indices(n, 1)])
        few = upper[-max(1, n // 8)] if len(upper) else np.float32(np.inf)
        got = _host(torch, index.components(float(few)))[0]
        _same(got, cva.compute_retrieval_components(sim, few), ("few", n, dim))
        if n >= 64:
            assert n // 2 < len(set(got.tolist())) < n


# ---- 2. graphs built to stress the union-find -----------------------------------------------------------------------------------------

N_G = 300  # three 128-row blocks, the last one short; five row tiles


def _path_rows():
    g = np.zeros((N_G, N_G + 1), np.float32)  # row i = e_i + e_(i + 1): neighbours score 1, a row with itself 2, everything else 0
    g[np.arange(N_G), np.arange(N_G)] = 1
    g[np.arange(N_G), np.arange(N_G) + 1] = 1
    return g


def _edge_rows(edges):
    g = np.zeros((N_G, len(edges)), np.float32)  # one column per edge, 1 in its two rows: rows that share an edge score 1
    for k, (a, b) in enumerate(edges):
        g[a, k] = g[b, k] = 1
    return g


def _graphs():
    """name -> (gallery, a row whose removal leaves exactly `parts` components, parts)."""
    perm = np.random.RandomState(17).permutation(N_G)  # path position perm[r] sits in row r
    path = _path_rows()
    star = _edge_rows([(i, N_G - 1) for i in range(N_G - 1)])
    evens, odds = list(range(0, N_G, 2)), list(range(1, N_G, 2))
    two = _edge_rows(list(zip(evens, evens[1:])) + list(zip(odds, odds[1:])) + [(N_G - 2, N_G - 1)])  # the joint: rows 298 and 299
    return {"path": (path, 150, 2), "reversed": (path[::-1].copy(), 150, 2), "permuted": (path[perm], int(np.argwhere(perm == 150)[0, 0]), 2),
            "star": (star, 150, 1),  # a leaf leaves: the others still meet in the centre
            "two paths": (two, 150, 2)}


_GRAPHS = {}


def _graph_index(torch, cva, name, storage):
    if (name, storage) not in _GRAPHS:
        g, cut, parts = _graphs()[name]
        _GRAPHS[(name, storage)] = (cva.GalleryIndex(torch.tensor(g, device="cuda"), normalize=False, storage=getattr(torch, storage)), cut, parts)
    return _GRAPHS[(name, storage)]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["path", "reversed", "permuted", "star", "two paths"])
def test_long_chains_and_a_star_end_in_one_label(env, name, storage):
    """Every graph is connected: one label, the smallest row.  With one middle row removed the paths fall into exactly two components
    (the star, whose middle rows are leaves, stays one), and the removed row is -1."""
    torch, cva = env
    index, cut, parts = _graph_index(torch, cva, name, storage)
    sim = _host(torch, index.search(index.gallery.float(), 1, want_sim=True)[2])[0]
    assert set(np.unique(sim[np.triu_indices(N_G, 1)]).tolist()) == {0.0, 1.0}
    got = _host(torch, index.components(0.5))[0]
    _same(got, np.zeros(N_G, np.int32), name)
    _same(got, cva.compute_retrieval_components(sim, 0.5), name)
    try:
        index.remove([cut])
        got = _host(torch, index.components(0.5))[0]
        ok = np.arange(N_G) != cut
        _same(got, cva.compute_retrieval_components(sim, 0.5, keep=ok), (name, "cut"))
        assert got[cut] == -1 and len(set(got[ok].tolist())) == parts and got[ok].min() == 0
        assert (got[got[ok]] == got[ok]).all() and (got[ok] <= np.arange(N_G)[ok]).all()  # every label is a root, the smallest of its rows
    finally:
        index.restore()
    if name == "star":  # without its centre nothing is connected
        try:
            index.remove([N_G - 1])
            want = np.arange(N_G, dtype=np.int32)
            want[-1] = -1
            _same(_host(torch, index.components(0.5))[0], want, "centre")
        finally:
            index.restore()


# ---- 3. schedule independence ---------------------------------------------------------------------------------------------------------

def test_the_bytes_do_not_depend_on_the_blocks_a_workgroup_walks(env):
    torch, cva = env
    runs = [(_graph_index(torch, cva, name, "float32")[0], 0.5, {}, name) for name in _graphs()]
    n, dim = 1000, 64
    for storage, normalize in (("bfloat16", True), ("float32", False)):
        index, sim, thr = _case(torch, cva, storage, normalize, n, dim)
        runs.append((index, thr, {}, (storage, "plain")))
        runs.append((index, thr, dict(keep=_dev(torch, np.random.RandomState(5).rand(n) < 0.8), groups=_dev(torch, sj._groups(n, "runs"))), (storage, "filters")))
    for index, thr, kw, what in runs:
        nb = (index.n + 127) // 128
        want = _host(torch, index.components(thr, **kw))[0]  # automatic
        assert len(set(want.tolist())) < index.n
        for per in (1, 3, nb):
            with _Blocks(cva, per):
                for again in range(2):
                    _same(_host(torch, index.components(thr, **kw))[0], want, (what, per, again))
    assert cva.lib.get_option("rt_comp_blocks_per_wg") == 0


# ---- 4. deduplicate -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filtered", [False, True])
def test_deduplicate_keeps_the_smallest_row_of_every_cluster(env, filtered):
    torch, cva = env
    n, dim = 1000, 64
    index, sim, thr = _case(torch, cva, "bfloat16", True, n, dim)
    groups = _dev(torch, sj._groups(n, "runs")) if filtered else None
    # clusters of a few rows: an exact score, the (N / 8)-th best of all pairs, and rows that never ask in between
    thr = np.full(n, np.sort(sim[np.triu_indices(n, 1)])[-(n // 8)], np.float32)
    thr[1::6], thr[2::6] = np.inf, np.nan
    t = _dev(torch, thr)
    try:
        before = np.ones(n, bool)
        if filtered:
            index.remove(np.arange(2, n, 7).tolist())
            before[2::7] = False
        want = _host(torch, index.components(t, groups=groups))[0]
        got = index.deduplicate(t, groups=groups)
        assert got.dtype == torch.int32 and got.is_cuda
        _same(_host(torch, got)[0], want)
        rep = (want >= 0) & (want == np.arange(n))
        assert n // 2 < rep.sum() < before.sum() - 20  # many clusters, and at least twenty rows to withdraw
        assert index.keep.dtype == torch.bool and bytes_equal(_host(torch, index.keep)[0], before & ~((want >= 0) & ~rep))
        assert bytes_equal(_host(torch, index.keep)[0], rep)  # which is: the representatives
        assert int(index.count_self_join(t, groups=groups).sum()) == 0  # two survivors with an edge would have shared a component
        _same(_host(torch, index.components(t, groups=groups))[0], np.where(rep, np.arange(n), -1).astype(np.int32))  # every survivor alone
        index.restore()
        assert index.keep is None
        _same(_host(torch, index.components(t, groups=groups))[0],
              cva.compute_retrieval_components(sim, thr, groups=None if groups is None else sj._groups(n, "runs")))
        assert int(index.count_self_join(t, groups=groups).sum()) > 0
    finally:
        index.restore()


# ---- 5. the C entry -------------------------------------------------------------------------------------------------------------------

class _Entry:
    """coot_retrieval_components through ctypes, parent and labels in the middle of buffers that hold a sentinel."""
    PAD = 64

    def __init__(self, torch, cva, index, thr, keep=None, groups=None):
        self.torch, self.lib = torch, cva.lib.load()
        self.g, self.norms, self.keep, self.groups = index.gallery, index.norms if index.normalize else None, keep, groups
        self.code = {torch.float32: 0, torch.bfloat16: cva.retrieval.GALLERY_BF16, torch.float16: cva.retrieval.GALLERY_F16}[index.gallery.dtype]
        self.n, self.dim = index.gallery.shape
        self.parent = torch.full((self.n + 2 * self.PAD,), -7, dtype=torch.int32, device="cuda")
        self.labels = torch.full((self.n + 2 * self.PAD,), -7, dtype=torch.int32, device="cuda")
        self.thr = torch.from_numpy(np.array(thr, np.float32)).cuda()  # (a copy: the shared arrays are read only)
        self.st = torch.cuda.current_stream().cuda_stream

    def _p(self, t):
        return None if t is None else t.data_ptr()

    def call(self, dt=None, g=-1, thr=-1, parent=-1, labels=-1, n=None, d=None):
        return self.lib.coot_retrieval_components(self.g.data_ptr() if g == -1 else g, self.code if dt is None else dt, self._p(self.norms),
                                                  self._p(self.keep), self._p(self.groups), self.thr.data_ptr() if thr == -1 else thr,
                                                  self.n if n is None else n, self.dim if d is None else d,
                                                  self.parent[self.PAD:].data_ptr() if parent == -1 else parent,
                                                  self.labels[self.PAD:].data_ptr() if labels == -1 else labels, self.st)

    def pads_untouched(self):
        self.torch.cuda.synchronize()
        return all(bool((t[:self.PAD] == -7).all()) and bool((t[self.PAD + self.n:] == -7).all()) for t in (self.parent, self.labels))

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.parent == -7).all()) and bool((self.labels == -7).all())


def test_the_call_writes_its_two_arrays_and_nothing_around_them(env):
    torch, cva = env
    for n, dim, storage, with_filters in ((1000, 64, "bfloat16", False), (129, 37, "float32", True), (1, 16, "float16", False)):
        index, sim, thr = _case(torch, cva, storage, True, n, dim)
        keep = (np.random.RandomState(6).rand(n) < 0.7) if with_filters else None
        groups = sj._groups(n, "runs") if with_filters else None
        c = _Entry(torch, cva, index, thr, keep=None if keep is None else _dev(torch, keep.astype(np.uint8)), groups=_dev(torch, groups))
        assert c.call() == 0, c.lib.coot_last_error()
        assert c.pads_untouched()
        labels, parent = _host(torch, c.labels[c.PAD:c.PAD + n], c.parent[c.PAD:c.PAD + n])
        _same(labels, cva.compute_retrieval_components(sim, thr, keep=keep, groups=groups), (n, dim))
        assert (parent <= np.arange(n)).all() and (parent >= 0).all()  # the workspace holds a forest that only points down


def test_refusals_write_nothing(env):
    """Refused before any launch: the return code, the message naming the entry and the argument, and every buffer as it was."""
    torch, cva = env
    n, dim = 300, 16
    index = cva.GalleryIndex(torch.tensor(sj._gallery(n, dim), device="cuda"), normalize=True)
    c = _Entry(torch, cva, index, np.zeros(n, np.float32))
    big = 65535 * 64 + 1
    cases = [(dict(dt=7), "dtype = 7"), (dict(dt=-1), "dtype = -1"), (dict(g=None), "null pointer"), (dict(thr=None), "null pointer"),
             (dict(parent=None), "null pointer"), (dict(labels=None), "null pointer"), (dict(n=0), "N = 0"), (dict(n=-5), "N = -5"), (dict(d=0), "d = 0"),
             (dict(n=big), "N = %d" % big), (dict(n=2 ** 31 - 1), "N = %d" % (2 ** 31 - 1))]
    for kw, part in cases:
        assert c.call(**kw) != 0, kw
        msg = c.lib.coot_last_error().decode()
        assert "retrieval_components:" in msg and part in msg, (kw, msg)
        assert c.untouched(), kw
    assert c.call() == 0, c.lib.coot_last_error()  # the same buffers, accepted as they were made
    assert c.pads_untouched()
