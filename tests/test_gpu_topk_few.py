"""The few-query search on a prepared gallery (coot_retrieval_row_norms + coot_retrieval_topk_few; retrieval.GalleryIndex) against
the call it has to reproduce, coot_retrieval_topk (retrieval.retrieval_topk_device): indices, scores and the similarity matrix are
compared BYTE FOR BYTE — one gallery row per thread instead of 64 x 64 tiles, but the same fp32 FMA chain per element and the
same total order — and against the host mirror (retrieval.compute_retrieval_topk) on the matrix the kernel handed out.  Every
assertion is an equality.  The one numeric bound is test_gpu_topk.py's 2e-6 of the matrix against the float64 product of the unit
rows (fp32 FMA chains of <= 768 terms on unit-norm rows), repeated for one shape."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal as _bytes_equal, check_against_mirror as _check_against_mirror, host as _host, planted as _planted, unit as _unit

pytestmark = pytest.mark.gpu

HUGE = 1 << 20  # a split count beyond every plan: clamped to the most the planner allows


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


@pytest.fixture
def few_splits(env):
    """Sets rt_few_splits and restores the automatic choice afterwards."""
    _, cva = env
    lib = cva.lib.load()

    def set_(n):
        assert lib.coot_set_option(b"rt_few_splits", n) == 0
    yield set_
    set_(0)


# N below, at and just over a workgroup's 128 rows and no multiple of 64; d below 32 and no multiple of 32; K = 1, N, 128;
# M = 1 and 16; one gallery with many workgroups and two merge rounds (20 000 rows: 157 lists -> 5 -> the result)
SHAPES = [(1, 1, 8, 1), (1, 4099, 384, 128), (3, 257, 40, 7), (16, 255, 96, 128), (16, 1000, 768, 50), (5, 65, 32, 65), (16, 20000, 384, 10)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("m,n,dim,k", SHAPES)
def test_few_equals_the_tile_call(env, m, n, dim, k, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device
    q, g = _planted(m, n, dim, m + n + dim)
    if not normalize:
        q, g = _unit(q), _unit(g)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    index = GalleryIndex(tg, normalize=normalize)
    idx, sc, sim = _host(torch, *index.search(tq, k, want_sim=True))
    want_idx, want_sc, want_sim = _host(torch, *retrieval_topk_device(tq, tg, k, normalize=normalize, want_sim=True))
    assert _bytes_equal(sim, want_sim), np.argwhere(sim.view(np.int32) != want_sim.view(np.int32))[:5]
    assert _bytes_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    assert _bytes_equal(sc, want_sc)
    _check_against_mirror(idx, sc, sim, k)
    if (m, n, dim, k) == (16, 1000, 768, 50):
        a, b = (_unit(q), _unit(g)) if normalize else (q, g)
        err = np.abs(sim - a.astype(np.float64) @ b.astype(np.float64).T).max()
        print(f"[{m} x {n} x {dim}, normalize = {normalize}] max |sim - float64 product| = {err:.3e}")
        assert err < 2e-6
    # without the testing aid: the same bytes
    idx2, sc2, none = index.search(tq, k)
    assert none is None
    idx2, sc2 = _host(torch, idx2, sc2)
    assert _bytes_equal(idx2, idx) and _bytes_equal(sc2, sc)


@pytest.mark.parametrize("m,n,dim,k,normalize", [(2, 300, 30, 9, True), (7, 130, 5, 128, False), (9, 1100, 34, 3, True)])
def test_widths_that_take_the_scalar_loads(env, m, n, dim, k, normalize):
    """d that is no multiple of 4: the gallery rows are not 16-byte aligned and the staging loads one float at a time."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device
    q, g = _planted(m, n, dim, 3 * m + n + dim)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    got = _host(torch, *GalleryIndex(tg, normalize=normalize).search(tq, k, want_sim=True))
    want = _host(torch, *retrieval_topk_device(tq, tg, k, normalize=normalize, want_sim=True))
    for a, b in zip(got, want):
        assert _bytes_equal(a, b)


@pytest.mark.parametrize("m,n,dim,k,signs", [(16, 5000, 96, 128, False), (3, 640, 40, 7, True)])
def test_result_does_not_depend_on_splits(env, few_splits, m, n, dim, k, signs):
    """Every workgroup sweeps a contiguous range of 128-row blocks and the partial lists are merged in rounds: 1 split (no merge
    launch), 2, 7, the automatic choice and the most the planner allows give identical bytes.  The signs gallery (+-1 entries) has
    rows of a few repeated values: whole runs of exact ties cross the split boundaries."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    q, g = _planted(m, n, dim, 7 * m + n)
    if signs:
        q, g = np.sign(q).astype(np.float32), np.sign(g).astype(np.float32)  # similarities are small integers: ties everywhere
    tq = torch.from_numpy(q).cuda()
    index = GalleryIndex(torch.from_numpy(g).cuda(), normalize=False)
    got = []
    for s in (1, 2, 7, 0, HUGE):
        few_splits(s)
        idx, sc, sim = index.search(tq, k, want_sim=(s == 1))
        got.append(tuple(_host(torch, idx, sc)))
        if s == 1:
            _check_against_mirror(got[0][0], got[0][1], _host(torch, sim)[0], k)
    for idx, sc in got[1:]:
        assert _bytes_equal(idx, got[0][0]) and _bytes_equal(sc, got[0][1])


def test_row_norms_are_the_normalising_divisor(env):
    """Through the public route: rows divided on the host by the returned norms (one IEEE division each, as the kernels divide
    while staging) and searched with normalize=False give the bytes of the raw rows searched with the prepared norms.  The query
    norms, which the call computes itself, come from the same function."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device
    lib = cva.lib.load()
    m, n, dim = 4, 300, 72
    q, g = _planted(m, n, dim, 11)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    st = torch.cuda.current_stream().cuda_stream
    index = GalleryIndex(tg, normalize=True)
    qnorm = torch.empty(m, device="cuda")
    assert lib.coot_retrieval_row_norms(tq.data_ptr(), m, dim, qnorm.data_ptr(), st) == 0
    gn, qn = _host(torch, index.norms, qnorm)
    assert gn.dtype == np.float32 and gn.shape == (n,) and (gn > 0).all()
    g_div, q_div = (g / gn[:, None]).astype(np.float32), (q / qn[:, None]).astype(np.float32)
    want = _host(torch, *retrieval_topk_device(torch.from_numpy(q_div).cuda(), torch.from_numpy(g_div).cuda(), 20, normalize=False, want_sim=True))
    got = _host(torch, *index.search(tq, 20, want_sim=True))
    for a, b in zip(got, want):
        assert _bytes_equal(a, b)
    assert lib.coot_retrieval_row_norms(None, n, dim, qnorm.data_ptr(), st) != 0 and "retrieval_row_norms" in lib.coot_last_error().decode()


def test_gallery_index_routes(env):
    torch, cva = env
    from coot_videotext_amd.retrieval import RETRIEVAL_FEW_MAX, GalleryIndex, retrieval_topk_device
    assert RETRIEVAL_FEW_MAX == 16
    q, g = _planted(17, 700, 64, 5)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    index = GalleryIndex(tg, normalize=True)
    assert index.gallery.data_ptr() == tg.data_ptr()  # kept by reference
    norms_ptr = index.norms.data_ptr()
    for m in (16, 17):
        got = _host(torch, *index.search(tq[:m], 10, want_sim=True))
        want = _host(torch, *retrieval_topk_device(tq[:m], tg, 10, normalize=True, want_sim=True))
        assert got[0].shape == (m, 10)
        for a, b in zip(got, want):
            assert _bytes_equal(a, b)
    one = _host(torch, *index.search(tq[3], 10)[:2])
    want = _host(torch, *retrieval_topk_device(tq[3:4], tg, 10, normalize=True)[:2])
    assert one[0].shape == (1, 10) and _bytes_equal(one[0], want[0]) and _bytes_equal(one[1], want[1])
    assert index.norms.data_ptr() == norms_ptr  # computed once
    with pytest.raises(ValueError, match="width"):
        index.search(tq[:2, :32], 10)
    for k in (0, 129, 701):
        with pytest.raises(ValueError, match="k = "):
            index.search(tq[:2], k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search(tq[:2].cpu(), 10)
    raw = GalleryIndex(tg[:, ::2], normalize=False)  # not contiguous: copied
    assert raw.norms is None and raw.gallery.is_contiguous()
    got = _host(torch, *raw.search(tq[:5, ::2], 10)[:2])
    want = _host(torch, *retrieval_topk_device(tq[:5, ::2], tg[:, ::2], 10)[:2])
    assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1])


def test_refusals_write_nothing(env):
    torch, cva = env
    lib = cva.lib.load()
    m, n, dim = 16, 300, 16
    q, g = torch.randn(17, dim, device="cuda"), torch.randn(n, dim, device="cuda")
    gn = torch.empty(n, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.coot_retrieval_row_norms(g.data_ptr(), n, dim, gn.data_ptr(), st) == 0
    idx = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((17, 129), -7.0, device="cuda")
    ws = torch.zeros(lib.coot_retrieval_topk_few_workspace_bytes(m, n, dim, 128) + (1 << 20), dtype=torch.uint8, device="cuda")

    def call(mm, nn, k, ws_bytes, idx_ptr):
        return lib.coot_retrieval_topk_few(q.data_ptr(), g.data_ptr(), gn.data_ptr(), mm, nn, dim, k, idx_ptr, sc.data_ptr(), None, ws.data_ptr(),
                                           ws_bytes, st)
    cases = {"M = 17": (17, n, 10, ws.numel(), idx.data_ptr()), "K = 0": (m, n, 0, ws.numel(), idx.data_ptr()),
             "K > N": (m, 100, 101, ws.numel(), idx.data_ptr()), "K = 129": (m, n, 129, ws.numel(), idx.data_ptr()),
             "workspace": (m, n, 10, 64, idx.data_ptr()), "null output": (m, n, 10, ws.numel(), None)}
    for what, args in cases.items():
        assert call(*args) != 0, what
        msg = lib.coot_last_error().decode()
        assert "retrieval_topk_few" in msg, (what, msg)
        assert {"M = 17": "M = 17", "workspace": "workspace too small", "null output": "null pointer"}.get(what, "K = ") in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool((sc == -7.0).all()) and not bool(ws.any()), what
    assert call(m, n, 128, ws.numel(), idx.data_ptr()) == 0, lib.coot_last_error()  # the same buffers, accepted
    torch.cuda.synchronize()
    got = idx.view(-1)[:m * 128]
    assert bool(((got >= 0) & (got < n)).all()) and bool((idx.view(-1)[m * 128:] == -7).all())
