"""The tile search on a prepared gallery (coot_retrieval_topk_index; retrieval.retrieval_topk_index_device, GalleryIndex.search with
more than 16 queries) against its definition: the existing fp32 tile search on the gallery widened to fp32,

    oracle = retrieval_topk_device(q, index.gallery.float(), k, normalize=..., keep=..., want_sim=True),

which computes the gallery's norms itself, reads fp32 rows and knows nothing of an index.  Indices, scores and the similarity matrix
are compared BYTE FOR BYTE (on the device: int32 views, so a NaN or a -0 would count too), for every storage type, with and without
normalisation, under every kind of filter, with and without the similarity matrix, and at every split count.  Inputs and helpers are
those of tests/retrieval_cases.py."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal as _bytes_equal, check_against_mirror as _check_against_mirror, host as _host, planted as _planted

pytestmark = pytest.mark.gpu

STORAGES = ["float32", "bfloat16", "float16"]
# The smallest shapes at which each mechanism can go wrong.  M: the few-query boundary (16 | 17), one full row tile, two row tiles with a
# ragged second.  N: one row; a ragged only tile; a ragged last tile of three; eleven tiles (several per split).  d: 1; not a multiple
# of 8; one element into the second chunk of 32; two full chunks.  K: 1, 9 and 128, clamped to N.
MS, NS, DS, KS = (1, 16, 17, 64, 70), (1, 63, 130, 700), (1, 20, 33, 64), (1, 9, 128)
HUGE = 1 << 20  # a split count beyond every plan: clamped to the most the planner allows


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _same(torch, a, b):
    """Two device tensors hold the same bytes."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _keeps(torch, n, kk, seed):
    """name -> keep [N] on the device (None: no filter).  "few": kk - 1 rows, fewer than the kk asked for: -1 / -inf tails."""
    rs = np.random.RandomState(seed)
    contig = np.zeros(n, bool)
    contig[n // 3:n // 3 + max(1, n // 4)] = True  # N = 700: rows [233, 408), so tiles 0 .. 2 and 7 .. 10 keep nothing and are skipped
    few = np.zeros(n, bool)
    few[rs.permutation(n)[:kk - 1]] = True
    masks = {"ones": np.ones(n, bool), "half": rs.rand(n) < 0.5, "contig": contig, "few": few, "none": np.zeros(n, bool)}
    out = {"null": None}
    for i, (name, mask) in enumerate(masks.items()):  # torch.bool, or bytes of which every nonzero value keeps
        out[name] = torch.from_numpy(mask.astype(np.uint8) * np.uint8(0x82)).cuda() if i % 2 else torch.from_numpy(mask).cuda()
    return out, masks


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_index_call_is_the_fp32_tile_search_on_the_widened_gallery(env, storage, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device, retrieval_topk_index_device
    calls = 0
    for n in NS:
        for dim in DS:
            q, g = _planted(max(MS), n, dim, n + dim)
            tq_all, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
            index = GalleryIndex(tg, normalize=normalize, storage=getattr(torch, storage))
            wide = index.gallery.float()
            norms = index.norms if normalize else None
            for k in KS:
                kk = min(k, n)
                keeps, masks = _keeps(torch, n, kk, n + dim + k)
                for m in MS:
                    tq = tq_all[:m]
                    sim_ref = None
                    for name, keep in keeps.items():
                        what = (n, dim, kk, m, name)
                        want = retrieval_topk_device(tq, wide, kk, normalize=normalize, keep=keep, want_sim=True)
                        got = retrieval_topk_index_device(tq, index.gallery, norms, kk, keep=keep, want_sim=True)
                        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].shape == (m, n), what
                        assert _same(torch, got[2], want[2]), what
                        assert _same(torch, got[0], want[0]) and _same(torch, got[1], want[1]), what
                        sim_ref = got[2] if sim_ref is None else sim_ref
                        assert _same(torch, got[2], sim_ref), what  # the filter does not touch sim
                        # without sim a column tile that keeps nothing is skipped: the same bytes
                        idx, sc, none = retrieval_topk_index_device(tq, index.gallery, norms, kk, keep=keep)
                        assert none is None and _same(torch, idx, want[0]) and _same(torch, sc, want[1]), what
                        if m <= 16:  # the few-query call (coot_retrieval_topk_few_masked), which GalleryIndex.search takes up to 16 queries
                            few = index.search(tq, kk, keep=keep, want_sim=True)
                            assert all(_same(torch, a, b) for a, b in zip(got, few)), what
                        if name in ("few", "none"):  # fewer than kk kept: exactly that many filled slots per row, then -1 / -inf
                            kept = int(masks[name].sum())
                            assert kept < kk and bool((got[0][:, kept:] == -1).all()) and bool(torch.isneginf(got[1][:, kept:]).all()), what
                            assert bool((got[0][:, :kept] >= 0).all()), what
                        calls += 1
    assert calls == len(NS) * len(DS) * len(KS) * len(MS) * 6


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("storage", STORAGES)
def test_ties_at_every_split_count(env, storage, normalize):
    """A gallery and queries of +-1 (both 16-bit formats hold them exactly, and every norm is sqrt(d)): similarities are small integers,
    or their quotient by d, and runs of exact ties cross every split boundary.  1 split (no merge launch), 2, 7, the automatic choice and
    more than the planner allows give identical bytes, which are the numpy mirror's on the returned similarity matrix."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex, compute_retrieval_topk_masked, retrieval_topk_index_device
    lib = cva.lib.load()
    m, n, dim = 70, 700, 64
    q, g = _planted(m, n, dim, 11)
    tq, tg = torch.from_numpy(np.sign(q).astype(np.float32)).cuda(), torch.from_numpy(np.sign(g).astype(np.float32)).cuda()
    index = GalleryIndex(tg, normalize=normalize, storage=getattr(torch, storage))
    norms = index.norms if normalize else None
    keep_host = np.random.RandomState(3).rand(n) < 0.5
    keep = torch.from_numpy(keep_host).cuda()
    try:
        for k in (9, 128):
            first = None
            for s in (1, 2, 7, 0, HUGE):
                assert lib.coot_set_option(b"rt_topk_splits", s) == 0
                got = _host(torch, *retrieval_topk_index_device(tq, index.gallery, norms, k, want_sim=True))
                got_kept = _host(torch, *retrieval_topk_index_device(tq, index.gallery, norms, k, keep=keep)[:2])
                if first is None:
                    first = (got, got_kept)
                    _check_against_mirror(got[0], got[1], got[2], k)
                    assert len(np.unique(got[2])) < 200  # ties everywhere: 49 000 similarities, few distinct values
                    want_idx, want_sc = compute_retrieval_topk_masked(got[2], k, keep_host)
                    assert _bytes_equal(got_kept[0], want_idx) and _bytes_equal(got_kept[1], want_sc)
                assert all(_bytes_equal(a, b) for a, b in zip(got, first[0])), (k, s)
                assert all(_bytes_equal(a, b) for a, b in zip(got_kept, first[1])), (k, s)
    finally:
        assert lib.coot_set_option(b"rt_topk_splits", 0) == 0


@pytest.mark.parametrize("storage", STORAGES)
def test_the_stored_norms_are_what_is_used(env, storage):
    """One row's stored norm doubled: the staged value x / norm halves exactly, and with it every product and every partial sum of that
    row's chains, so exactly that column of sim halves and no other byte of sim changes.  A call that recomputed the norms would
    return the first matrix again."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_index_device
    m, n, dim, k, row = 70, 130, 33, 9, 77
    q, g = _planted(m, n, dim, n + dim)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    index = GalleryIndex(tg, normalize=True, storage=getattr(torch, storage))
    sim = _host(torch, retrieval_topk_index_device(tq, index.gallery, index.norms, k, want_sim=True)[2])[0]
    norms = index.norms.clone()
    norms[row] *= 2
    idx2, sc2, sim2 = _host(torch, *retrieval_topk_index_device(tq, index.gallery, norms, k, want_sim=True))
    want = sim.copy()
    want[:, row] *= np.float32(0.5)
    assert (sim[:, row] != 0).all() and _bytes_equal(sim2, want), np.argwhere(sim2.view(np.int32) != want.view(np.int32))[:5]
    _check_against_mirror(idx2, sc2, sim2, k)  # and the selection ran on those similarities


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("storage", STORAGES)
def test_through_the_index(env, monkeypatch, storage, forced):
    """GalleryIndex.search with more than 16 queries: the index's own filter and a per-search keep, rows added into spare capacity (gallery
    and norms are then views of a larger buffer: the call has to take index.n rows, not the capacity), and no fp32 copy in the
    gallery's place.  forced: a 16-bit index takes the tile call from 17 queries on, wherever the shipped threshold lies."""
    torch, cva = env
    from coot_videotext_amd import retrieval
    from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device
    if forced:
        monkeypatch.setattr(retrieval, "INDEX_TILE_MIN_M_16BIT", 17)
    dtype = getattr(torch, storage)
    n, extra, dim, k = 130, 40, 33, 9
    q, g = _planted(70, n + extra, dim, 5)
    tq_all, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    index = GalleryIndex(tg[:n], normalize=True, storage=dtype, capacity=n + extra + 7)
    ptr = index.gallery.data_ptr()

    def check(keep_host=None, own=None):
        for m in (17, 70):
            tq = tq_all[-m:]
            keep = None if keep_host is None else torch.from_numpy(keep_host).cuda()
            both = keep_host if own is None else own if keep_host is None else own & keep_host
            want = retrieval_topk_device(tq, index.gallery.float(), k, normalize=True, want_sim=True, keep=None if both is None else torch.from_numpy(both).cuda())
            got = index.search(tq, k, want_sim=True, keep=keep)
            assert all(_same(torch, a, b) for a, b in zip(got, want)), (m, len(index))
            idx, sc, none = index.search(tq, k, keep=keep)
            assert none is None and _same(torch, idx, want[0]) and _same(torch, sc, want[1]), (m, len(index))
            assert index.gallery.dtype == dtype and index.gallery.data_ptr() == ptr  # no fp32 copy took its place
        return _host(torch, want[0])[0]

    check()
    removed = np.ones(n, bool)
    removed[[3, 64, 65, 129]] = False
    index.remove([3, 64, 65, 129])
    other = np.random.RandomState(1).rand(n) < 0.5
    got = check(other, removed)
    assert not np.isin(got, [3, 64, 65, 129]).any() and other[got].all()
    check(None, removed)
    index.restore()
    assert index.add(tg[n:]) == n and len(index) == n + extra and index.capacity == n + extra + 7
    assert index.gallery.data_ptr() == ptr and index.norms.shape == (n + extra,)
    got = check()
    assert (got >= n).any() and (got < n + extra).all()  # the added rows are found, and nothing beyond index.n, where the buffer holds whatever was there


def test_index_refusals_write_nothing(env):
    """Every refusal names the function, returns before any launch and leaves poisoned outputs and workspace as they are; the same
    buffers, with exactly the bytes the size query reports, are then accepted."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GALLERY_BF16
    lib = cva.lib.load()
    m, n, dim, k = 70, 300, 16, 10
    q, g = torch.randn(m, dim, device="cuda"), torch.randn(n, dim, device="cuda").to(torch.bfloat16)
    gn = torch.empty(n, device="cuda")
    keep = torch.ones(n, dtype=torch.uint8, device="cuda")
    keep[::2] = 0
    st = torch.cuda.current_stream().cuda_stream
    assert lib.coot_retrieval_row_norms_h(g.data_ptr(), GALLERY_BF16, n, dim, gn.data_ptr(), st) == 0
    idx = torch.full((m, 129), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((m, 129), -7.0, device="cuda")
    need = lib.coot_retrieval_topk_index_workspace_bytes(m, n, dim, k)
    assert need >= m * 4 and need == lib.coot_retrieval_topk_index_workspace_bytes(m, n, dim + 1, k)
    ws = torch.zeros(max(need, lib.coot_retrieval_topk_index_workspace_bytes(m, n, dim, 128)), dtype=torch.uint8, device="cuda")

    def call(q_ptr=q.data_ptr(), g_ptr=g.data_ptr(), dt=GALLERY_BF16, mm=m, nn=n, dd=dim, kk=k, idx_ptr=idx.data_ptr(), sc_ptr=sc.data_ptr(),
             ws_ptr=ws.data_ptr(), ws_bytes=need):
        return lib.coot_retrieval_topk_index(q_ptr, g_ptr, dt, gn.data_ptr(), keep.data_ptr(), mm, nn, dd, kk, idx_ptr, sc_ptr, None, ws_ptr, ws_bytes, st)
    cases = {"null queries": (dict(q_ptr=None), "null pointer"), "null gallery": (dict(g_ptr=None), "null pointer"),
             "null idx": (dict(idx_ptr=None), "null pointer"), "null scores": (dict(sc_ptr=None), "null pointer"),
             "null workspace": (dict(ws_ptr=None), "null pointer"), "M = 0": (dict(mm=0), "M = 0"), "N = 0": (dict(nn=0), "N = 0"),
             "d = 0": (dict(dd=0), "d = 0"), "K = 0": (dict(kk=0), "K = 0"), "K > N": (dict(nn=100, kk=101), "K = 101"),
             "K = 129": (dict(kk=129, ws_bytes=ws.numel()), "K = 129"), "dtype": (dict(dt=7), "gallery_dtype = 7"), "dtype -1": (dict(dt=-1), "gallery_dtype = -1"),
             "one byte short": (dict(ws_bytes=need - 1), "workspace too small")}
    for what, (args, part) in cases.items():
        assert call(**args) != 0, what
        msg = lib.coot_last_error().decode()
        assert "retrieval_topk_index:" in msg and part in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool((sc == -7.0).all()) and not bool(ws.any()), what
    assert call() == 0, lib.coot_last_error()  # exactly the bytes the size query reports
    torch.cuda.synchronize()
    got = idx.view(-1)[:m * k]
    assert bool(((got >= 0) & (got < n) & (got % 2 == 1)).all()) and bool((idx.view(-1)[m * k:] == -7).all())
    assert bool((sc.view(-1)[:m * k] != -7.0).all()) and bool((sc.view(-1)[m * k:] == -7.0).all())
