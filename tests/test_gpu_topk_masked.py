"""The filtered top-K search (coot_retrieval_topk_masked, coot_retrieval_topk_few_masked; keep= of retrieval_topk_device and
GalleryIndex.search, GalleryIndex.remove / restore) against its definition: a similarity is the same FMA chain wherever its row
lies and the order (score descending, then index descending) survives a monotone renumbering, so a filtered search is, bit for
bit, the unfiltered and already tested search on the compacted gallery gallery[keep] with its indices mapped back through
nonzero(keep); with c < k kept rows, the first c columns are those of a k = c call and the rest are -1 / -inf.  Every comparison
is for byte equality.  Helpers and the planted-gallery recipe are those of tests/test_gpu_topk_half.py."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal as _bytes_equal, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

PATHS = ["tile", "float32", "bfloat16", "float16"]  # retrieval_topk_device, and GalleryIndex on the three storages
# N: a partial block and tile; several blocks with a short last one; many tiles; more than 32 sweep splits (two few-merge rounds).
# d: no multiple of 32; no multiple of 8 (the clamped 16-bit loads); the width paired with the largest N
SHAPES = [(130, 72), (300, 30), (1000, 72), (4500, 40)]
# (M, K): M = 1, 3, 16 few queries; 17 = slices on 16-bit storage, the tile call on fp32; 70 = two row tiles.  K = 1, 9, 128
MK = [(1, 1), (1, 128), (3, 9), (16, 9), (16, 128), (17, 9), (17, 128), (70, 9)]
SPLITS = (1, 3, 0)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def splits(env):
    """Sets rt_topk_splits and rt_few_splits and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(n):
        assert lib.coot_set_option(b"rt_topk_splits", n) == 0 and lib.coot_set_option(b"rt_few_splits", n) == 0
    yield set_
    set_(0)


def _masks(n, seed):
    """name -> bool [N] on the host."""
    rs = np.random.RandomState(seed)
    out = {"random half": rs.rand(n) < 0.5, "all": np.ones(n, bool), "none": np.zeros(n, bool)}
    out["last row"] = np.arange(n) == n - 1
    five = np.zeros(n, bool)
    five[[1, 2, n // 2, n // 2 + 1, n - 1]] = True  # 5 kept, fewer than K = 9 and 128: most automatic splits hold none of them
    out["five"] = five
    dead = np.ones(n, bool)
    dead[64:384] = False  # rows [64, 128): a whole tile; [128, 384): two whole few-kernel blocks (and four tiles): the skip path
    out["dead blocks"] = dead
    out["last block"] = np.arange(n) >= (n - 1) // 128 * 128  # only rows of the last, partial block of 128
    return out


class _Searcher:
    """One path on one gallery: the filtered call, and the unfiltered call on a compacted gallery (the oracle)."""

    def __init__(self, torch, path, tg, normalize):
        from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device
        self.torch, self.path, self.tg, self.normalize = torch, path, tg, normalize
        self._topk, self._Index = retrieval_topk_device, GalleryIndex
        self.index = None if path == "tile" else GalleryIndex(tg, normalize=normalize, storage=getattr(torch, path))

    def search(self, tq, k, keep=None, want_sim=False):
        if self.index is None:
            return self._topk(tq, self.tg, k, normalize=self.normalize, want_sim=want_sim, keep=keep)
        return self.index.search(tq, k, want_sim=want_sim, keep=keep)

    def compacted(self, keep_host):
        """The same path on gallery[keep]: code from before the filter existed."""
        sub = self.tg[self.torch.from_numpy(keep_host).cuda()].contiguous()
        return _Searcher(self.torch, self.path, sub, self.normalize)


def _expected(torch, compact, cols, tq, k):
    """The definition on the host: (idx int32 [M, k], scores float32 [M, k])."""
    m, c = tq.shape[0], len(cols)
    idx, sc = np.full((m, k), -1, np.int32), np.full((m, k), -np.inf, np.float32)
    if c:
        kk = min(k, c)
        sub_idx, sub_sc = _host(torch, *compact.search(tq, kk)[:2])
        idx[:, :kk], sc[:, :kk] = cols[sub_idx].astype(np.int32), sub_sc
    return idx, sc


def _keep_tensor(torch, keep_host, as_bytes):
    """The mask as the device sees it: torch.bool, or bytes of which every nonzero value keeps."""
    if as_bytes:
        return torch.from_numpy(keep_host.astype(np.uint8) * np.uint8(0x82)).cuda()
    return torch.from_numpy(keep_host).cuda()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("path", PATHS)
def test_masked_search_is_the_search_on_the_compacted_gallery(env, splits, path, n, dim, normalize):
    torch, cva = env
    q, g = _planted(70, n, dim, n + dim)
    tq_all, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    full = _Searcher(torch, path, tg, normalize)
    unmasked = {}  # M -> (idx, scores, sim) of keep=None at K = 9 / 128, for the all-kept mask and for sim
    for as_bytes, (name, keep_host) in enumerate(_masks(n, n).items()):
        cols = np.nonzero(keep_host)[0]
        compact = full.compacted(keep_host) if len(cols) else None
        keep = _keep_tensor(torch, keep_host, as_bytes % 2 == 1)
        for m, k in MK:
            tq = tq_all[:m]
            want_idx, want_sc = _expected(torch, compact, cols, tq, k)
            for s in SPLITS:
                splits(s)
                idx, sc, none = full.search(tq, k, keep=keep)
                assert none is None
                idx, sc = _host(torch, idx, sc)
                assert idx.dtype == np.int32 and sc.dtype == np.float32
                assert _bytes_equal(idx, want_idx), (name, m, k, s, np.argwhere(idx != want_idx)[:5])
                assert _bytes_equal(sc, want_sc), (name, m, k, s)
            # the no-skip path (sim asked for) returns the same bytes, and sim is not affected by the mask
            if (m, k) not in unmasked:
                unmasked[(m, k)] = _host(torch, *full.search(tq, k, want_sim=True))
            idx, sc, sim = _host(torch, *full.search(tq, k, keep=keep, want_sim=True))
            assert _bytes_equal(idx, want_idx) and _bytes_equal(sc, want_sc), (name, m, k, "want_sim")
            assert _bytes_equal(sim, unmasked[(m, k)][2]), (name, m, k)
            if name == "all":  # the bytes of the keep=None call, scores and indices
                assert _bytes_equal(idx, unmasked[(m, k)][0]) and _bytes_equal(sc, unmasked[(m, k)][1]), (m, k)
            if name == "none":
                assert (idx == -1).all() and np.isneginf(sc).all()
            if name == "random half" and k >= 9:  # the filter had work to do: the unfiltered result holds rows that are masked out
                assert not keep_host[unmasked[(m, k)][0]].all() and keep_host[idx].all(), (m, k)


@pytest.mark.parametrize("path", PATHS)
def test_ties_survive_the_filter(env, splits, path):
    """Every gallery row three times (rows 3 r, 3 r + 1, 3 r + 2 are equal), entries +-1: similarities are small integers and every
    score is tied at least three ways.  Masks remove one, two or all copies of each query's best rows; the device equals the mirror
    on the similarity matrix it returned, at every split count."""
    torch, cva = env
    from coot_videotext_amd.retrieval import compute_retrieval_topk_masked
    m, rows, dim, k = 16, 100, 40, 9
    rs = np.random.RandomState(5)
    base = np.sign(rs.randn(rows, dim)).astype(np.float32)
    g = np.repeat(base, 3, axis=0)
    q = np.sign(base[np.arange(m) * 5 % rows] + 0.8 * rs.randn(m, dim)).astype(np.float32)
    n = len(g)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    full = _Searcher(torch, path, tg, False)
    top = _host(torch, full.search(tq, 1)[0])[0][:, 0] // 3  # the best base row of every query
    for copies in ([2], [2, 0], [0, 1, 2], [1]):
        keep_host = np.ones(n, bool)
        for c in copies:
            keep_host[3 * top + c] = False
        keep = _keep_tensor(torch, keep_host, len(copies) == 2)
        for mm in (16, 3, 17):
            for s in SPLITS:
                splits(s)
                idx, sc, sim = _host(torch, *full.search(tq[:mm], k, keep=keep, want_sim=True))
                want_idx, want_sc = compute_retrieval_topk_masked(sim, k, keep_host)
                assert _bytes_equal(idx, want_idx), (copies, mm, s, np.argwhere(idx != want_idx)[:5])
                assert _bytes_equal(sc, want_sc), (copies, mm, s)
                idx2, sc2 = _host(torch, *full.search(tq[:mm], k, keep=keep)[:2])
                assert _bytes_equal(idx2, idx) and _bytes_equal(sc2, sc), (copies, mm, s)
            assert keep_host[idx].all()


@pytest.mark.parametrize("storage", PATHS[1:])
def test_remove_and_restore(env, storage):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    n, dim, k = 300, 72, 9
    q, g = _planted(70, n, dim, n + dim)
    tq_all, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    index = GalleryIndex(tg, normalize=True, storage=getattr(torch, storage))
    assert index.keep is None
    nbytes, ptr = index.nbytes, index.gallery.data_ptr()
    for m in (3, 17):
        tq = tq_all[:m]
        orig = _host(torch, *index.search(tq, k)[:2])
        # remove(r) == search(keep = mask without r); a host sequence and a device tensor say the same
        r = [5, 299, 130, 5]
        mask = np.ones(n, bool)
        mask[r] = False
        want = _host(torch, *index.search(tq, k, keep=torch.from_numpy(mask).cuda())[:2])
        index.remove(r)
        assert index.keep.dtype is torch.bool and index.keep.is_cuda and index.keep.shape == (n,)
        assert _host(torch, index.keep)[0].tolist() == mask.tolist()
        got = _host(torch, *index.search(tq, k)[:2])
        assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1])
        index.restore()
        index.remove(torch.tensor(r + [n, -1], device="cuda", dtype=torch.int32))  # (a device tensor is not checked: outside rows are ignored)
        assert _host(torch, index.keep)[0].tolist() == mask.tolist()
        # remove combined with a per-search keep: their AND
        other = np.random.RandomState(m).rand(n) < 0.5
        want = _host(torch, *index.search(tq, k, keep=torch.from_numpy(mask & other).cuda())[:2])
        index.restore()
        index.remove(r)
        for keep in (torch.from_numpy(other).cuda(), torch.from_numpy(other.astype(np.uint8) * np.uint8(7)).cuda()):
            got = _host(torch, *index.search(tq, k, keep=keep)[:2])
            assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1])
            assert not np.isin(got[0], r).any() and other[got[0]].all()
        # restore(rows) brings back those rows only; restore() the original bytes
        index.restore([299])
        mask[299] = True
        assert _host(torch, index.keep)[0].tolist() == mask.tolist()
        index.restore()
        assert index.keep is None
        got = _host(torch, *index.search(tq, k)[:2])
        assert _bytes_equal(got[0], orig[0]) and _bytes_equal(got[1], orig[1])
        # removing every query's current best row makes the former second result the new first
        index.remove(torch.from_numpy(orig[0][:, 0].copy()).cuda())
        got = _host(torch, *index.search(tq, k)[:2])
        gone = np.isin(orig[0], orig[0][:, 0])  # (a row that was another query's best is gone for this query too)
        for i in range(m):
            left = orig[0][i][~gone[i]]
            assert left[0] == orig[0][i, 1] or gone[i, 1]
            assert (got[0][i, :len(left)] == left).all() and _bytes_equal(got[1][i, :len(left)], orig[1][i][~gone[i]])
        index.restore()
        with pytest.raises(IndexError):
            index.remove([n])
        assert index.keep is None
    assert index.nbytes == nbytes and index.gallery.data_ptr() == ptr  # removed rows still occupy memory: nothing was rebuilt


def test_masked_refusals_write_nothing(env):
    """Refused calls return before any launch: outputs and workspace pre-filled with a sentinel stay as they are (the pattern of
    tests/test_gpu_topk_half.py::test_half_refusals_write_nothing), and the same buffers are then accepted."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GALLERY_BF16
    lib = cva.lib.load()
    m, n, dim = 16, 300, 16
    q, g = torch.randn(17, dim, device="cuda"), torch.randn(n, dim, device="cuda")
    g16 = g.to(torch.bfloat16)
    gn = torch.empty(n, device="cuda")
    keep = torch.ones(n, dtype=torch.uint8, device="cuda")
    keep[::2] = 0
    st = torch.cuda.current_stream().cuda_stream
    assert lib.coot_retrieval_row_norms(g.data_ptr(), n, dim, gn.data_ptr(), st) == 0
    idx = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((17, 129), -7.0, device="cuda")
    size = max(lib.coot_retrieval_topk_few_workspace_bytes(m, n, dim, 128), lib.coot_retrieval_topk_workspace_bytes(m, n, dim, 128))
    ws = torch.zeros(size + (1 << 20), dtype=torch.uint8, device="cuda")

    def few(mm, nn, k, ws_bytes, idx_ptr, dt=0, gal=g):
        return lib.coot_retrieval_topk_few_masked(q.data_ptr(), gal.data_ptr(), dt, gn.data_ptr(), keep.data_ptr(), mm, nn, dim, k, idx_ptr, sc.data_ptr(),
                                                  None, ws.data_ptr(), ws_bytes, st)

    def tile(mm, nn, k, ws_bytes, idx_ptr):
        return lib.coot_retrieval_topk_masked(q.data_ptr(), g.data_ptr(), keep.data_ptr(), mm, nn, dim, k, 1, idx_ptr, sc.data_ptr(), None, ws.data_ptr(),
                                              ws_bytes, st)
    common = {"K = 0": (m, n, 0, ws.numel(), idx.data_ptr()), "K > N": (m, 100, 101, ws.numel(), idx.data_ptr()),
              "K = 129": (m, n, 129, ws.numel(), idx.data_ptr()), "workspace": (m, n, 10, 64, idx.data_ptr()),
              "null output": (m, n, 10, ws.numel(), None)}
    few_cases = dict(common, **{"M = 17": (17, n, 10, ws.numel(), idx.data_ptr()), "dtype": (m, n, 10, ws.numel(), idx.data_ptr(), 7),
                                "K = 129, bf16": (m, n, 129, ws.numel(), idx.data_ptr(), GALLERY_BF16, g16)})
    for fn, call, cases in (("retrieval_topk_few_masked", few, few_cases), ("retrieval_topk_masked", tile, common)):
        for what, args in cases.items():
            assert call(*args) != 0, (fn, what)
            msg = lib.coot_last_error().decode()
            assert fn + ":" in msg, (what, msg)
            part = {"M = 17": "M = 17", "workspace": "workspace too small", "null output": "null pointer", "dtype": "dtype = 7"}.get(what, "K = ")
            assert part in msg, (what, msg)
            torch.cuda.synchronize()
            assert bool((idx == -7).all()) and bool((sc == -7.0).all()) and not bool(ws.any()), (fn, what)
    for call in (few, tile):  # the same buffers, accepted: 150 rows kept, K = 128
        assert call(m, n, 128, ws.numel(), idx.data_ptr()) == 0, lib.coot_last_error()
        torch.cuda.synchronize()
        got = idx.view(-1)[:m * 128]
        assert bool(((got >= 0) & (got < n) & (got % 2 == 1)).all()) and bool((idx.view(-1)[m * 128:] == -7).all())
        idx.fill_(-7)
