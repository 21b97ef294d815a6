"""The prepared gallery stored in bfloat16 or IEEE half (coot_retrieval_row_norms_h + coot_retrieval_topk_few_h;
retrieval.GalleryIndex(storage=...)) against its definition: a 16-bit value widens to fp32 exactly, so a search on a 16-bit gallery
is, bit for bit, the fp32 search on that gallery widened back to fp32.  The project's own fp32 call is the oracle,

    oracle(dtype) = retrieval_topk_device(q, g.to(dtype).float(), k, normalize=..., want_sim=True),

and indices, scores and the similarity matrix are compared BYTE FOR BYTE with it and with the host mirror
(retrieval.compute_retrieval_topk) on the matrix the kernel handed out.  Every assertion is an equality, except
test_close_to_the_fp32_search, whose bounds are derived in its docstring.  Helpers and the planted-gallery recipe are those of
tests/test_gpu_topk_few.py."""
import numpy as np
import pytest

from tests.retrieval_cases import bytes_equal as _bytes_equal, check_against_mirror as _check_against_mirror, host as _host, planted as _planted, unit as _unit

pytestmark = pytest.mark.gpu

HUGE = 1 << 20  # a split count beyond every plan: clamped to the most the planner allows
DTYPES = ["bfloat16", "float16"]


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


def _oracle(torch, tq, tg, dtype, k, normalize):
    """The definition: the fp32 tile call on the gallery rounded to dtype and widened back."""
    from coot_videotext_amd.retrieval import retrieval_topk_device
    return _host(torch, *retrieval_topk_device(tq, tg.to(dtype).float(), k, normalize=normalize, want_sim=True))


def _assert_same(got, want):
    idx, sc, sim = got
    want_idx, want_sc, want_sim = want
    assert _bytes_equal(sim, want_sim), np.argwhere(sim.view(np.int32) != want_sim.view(np.int32))[:5]
    assert _bytes_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    assert _bytes_equal(sc, want_sc)


# the shapes of tests/test_gpu_topk_few.py: N below, at and just over a workgroup's 128 rows and no multiple of 64; d below 32 and no
# multiple of 32; K = 1, N, 128; M = 1 and 16; one gallery with many workgroups and two merge rounds (20 000 rows: 157 lists -> 5)
SHAPES = [(1, 1, 8, 1), (1, 4099, 384, 128), (3, 257, 40, 7), (16, 255, 96, 128), (5, 65, 32, 65), (16, 1000, 768, 50), (16, 20000, 384, 10)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("m,n,dim,k", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_index_is_the_fp32_search_on_the_widened_gallery(env, dtype, m, n, dim, k, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    dtype = getattr(torch, dtype)
    q, g = _planted(m, n, dim, m + n + dim)
    if not normalize:
        q, g = _unit(q), _unit(g)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    index = GalleryIndex(tg, normalize=normalize, storage=dtype)
    assert index.storage is dtype and index.gallery.dtype == dtype
    got = _host(torch, *index.search(tq, k, want_sim=True))
    _assert_same(got, _oracle(torch, tq, tg, dtype, k, normalize))
    _check_against_mirror(got[0], got[1], got[2], k)
    # without the testing aid: the same bytes
    idx2, sc2, none = index.search(tq, k)
    assert none is None
    idx2, sc2 = _host(torch, idx2, sc2)
    assert _bytes_equal(idx2, got[0]) and _bytes_equal(sc2, got[1])


# d = 36: a multiple of 4 (the fp32 rows would be 16-byte aligned) but not of 8; 30, 5, 34: rows that are not even 4-byte aligned
@pytest.mark.parametrize("m,n,dim,k,normalize", [(2, 300, 36, 9, True), (2, 300, 30, 9, True), (7, 130, 5, 128, False), (9, 1100, 34, 3, True),
                                                 (9, 1100, 36, 3, False), (7, 130, 30, 128, True)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_widths_that_leave_the_16_byte_loads(env, dtype, m, n, dim, k, normalize):
    """d that is no multiple of 8: the 16-bit rows are not 16-byte aligned and the staging loads one element at a time, clamped
    into the gallery."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    dtype = getattr(torch, dtype)
    q, g = _planted(m, n, dim, 3 * m + n + dim)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    got = _host(torch, *GalleryIndex(tg, normalize=normalize, storage=dtype).search(tq, k, want_sim=True))
    _assert_same(got, _oracle(torch, tq, tg, dtype, k, normalize))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gallery_whose_base_is_not_16_byte_aligned(env, dtype):
    """d = 40 is a multiple of 8, but the gallery starts 44 elements = 88 bytes into its parent: contiguous, kept by reference, and
    no row is 16-byte aligned, so the element loads serve it."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    dtype = getattr(torch, dtype)
    m, n, dim, k = 3, 257, 40, 7
    q, g = _planted(m, n, dim, m + n + dim)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    parent = torch.zeros(n + 2, 41, dtype=dtype, device="cuda")  # an odd-width parent
    sub = parent.view(-1)[40 + 4:][:n * dim].view(n, dim)
    sub.copy_(tg.to(dtype))
    assert sub.is_contiguous() and sub.data_ptr() % 16 == 8
    for normalize in (True, False):
        index = GalleryIndex(sub, normalize=normalize)
        assert index.gallery.data_ptr() == sub.data_ptr()
        got = _host(torch, *index.search(tq, k, want_sim=True))
        _assert_same(got, _oracle(torch, tq, tg, dtype, k, normalize))


def test_both_ways_in(env):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    m, n, dim, k = 5, 300, 72, 10
    q, g = _planted(m, n, dim, 21)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    # a 16-bit tensor passed directly: kept by reference
    g_bf = tg.to(torch.bfloat16)
    index = GalleryIndex(g_bf)
    assert index.gallery.data_ptr() == g_bf.data_ptr() and index.storage is torch.bfloat16
    assert index.nbytes == n * dim * 2 + n * 4
    _assert_same(_host(torch, *index.search(tq, k, want_sim=True)), _oracle(torch, tq, tg, torch.bfloat16, k, True))
    # an fp32 tensor converted once, round to nearest even, the fp32 tensor not kept
    index = GalleryIndex(tg, normalize=False, storage=torch.float16)
    want = tg.to(torch.float16)
    assert index.storage is torch.float16 and index.gallery.dtype == torch.float16 and index.gallery.data_ptr() != tg.data_ptr()
    assert _bytes_equal(*_host(torch, index.gallery.view(torch.int16), want.view(torch.int16)))
    assert index.norms is None and index.nbytes == n * dim * 2
    # an fp32 index says what it holds too, and keeps its tensor
    index = GalleryIndex(tg)
    assert index.storage is torch.float32 and index.gallery.data_ptr() == tg.data_ptr() and index.nbytes == n * dim * 4 + n * 4
    # a 16-bit tensor widened: the fp32 index of the widened tensor
    g_half = tg.to(torch.float16)
    wide = GalleryIndex(g_half, storage=torch.float32)
    assert wide.storage is torch.float32 and wide.gallery.dtype == torch.float32
    want = _host(torch, *GalleryIndex(g_half.float()).search(tq, k, want_sim=True))
    _assert_same(_host(torch, *wide.search(tq, k, want_sim=True)), want)
    _assert_same(want, _oracle(torch, tq, tg, torch.float16, k, True))


@pytest.mark.parametrize("dim", [72, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_norms_are_those_of_the_widened_rows(env, dtype, dim):
    torch, cva = env
    from coot_videotext_amd.retrieval import GALLERY_BF16, GALLERY_F16, GalleryIndex
    lib = cva.lib.load()
    dtype = getattr(torch, dtype)
    n = 300
    _, g = _planted(4, n, dim, 11)
    g16 = torch.from_numpy(g).cuda().to(dtype)
    wide = g16.float()
    st = torch.cuda.current_stream().cuda_stream
    want = torch.empty(n, device="cuda")
    assert lib.coot_retrieval_row_norms(wide.data_ptr(), n, dim, want.data_ptr(), st) == 0
    index = GalleryIndex(g16, normalize=True)
    got, want = _host(torch, index.norms, want)
    assert got.dtype == np.float32 and got.shape == (n,) and (got > 0).all()
    assert _bytes_equal(got, want), np.argwhere(got.view(np.int32) != want.view(np.int32))[:5]
    # the C call refuses a null pointer and a dtype it does not know, and writes nothing
    out = torch.full((n,), -7.0, device="cuda")
    code = GALLERY_BF16 if dtype is torch.bfloat16 else GALLERY_F16
    for args in ((None, code, n, dim, out.data_ptr(), st), (g16.data_ptr(), code, n, dim, None, st), (g16.data_ptr(), 7, n, dim, out.data_ptr(), st)):
        assert lib.coot_retrieval_row_norms_h(*args) != 0
        assert "retrieval_row_norms_h" in lib.coot_last_error().decode(), lib.coot_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.coot_retrieval_row_norms_h(g16.data_ptr(), code, n, dim, out.data_ptr(), st) == 0
    assert _bytes_equal(_host(torch, out)[0], want)


def _representable(kind, m, n, dim, seed):
    """Galleries whose entries both 16-bit formats hold exactly: +-1, and small integers divided by 8 (|entry| <= 4)."""
    q, g = _planted(m, n, dim, seed)
    if kind == "signs":
        return np.sign(q).astype(np.float32), np.sign(g).astype(np.float32)  # similarities are small integers: ties everywhere
    g8 = (np.clip(np.round(g * 8), -32, 32) / 8).astype(np.float32)
    g8[np.abs(g8).sum(-1) == 0, 0] = 0.125  # (no zero row: its norm would divide by zero)
    return q.copy(), g8


@pytest.mark.parametrize("kind", ["signs", "eighths"])
@pytest.mark.parametrize("m,n,dim,k", [(16, 5000, 96, 128), (3, 640, 40, 7)])
def test_representable_galleries_give_the_fp32_index_bytes(env, few_splits, kind, m, n, dim, k):
    """Nothing is rounded when the gallery is stored, so the 16-bit index returns the bytes of the fp32 index on the ORIGINAL
    tensor, with normalisation and without.  On the +-1 gallery whole runs of exact ties cross every split boundary: 1 split (no
    merge launch), 2, 7, the automatic choice and the most the planner allows give identical bytes."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    q, g = _representable(kind, m, n, dim, 7 * m + n)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    for dtype in (torch.bfloat16, torch.float16):
        assert bool((tg.to(dtype).float() == tg).all())  # representable
        for normalize in (True, False):
            want = _host(torch, *GalleryIndex(tg, normalize=normalize).search(tq, k, want_sim=True))
            index = GalleryIndex(tg, normalize=normalize, storage=dtype)
            got = _host(torch, *index.search(tq, k, want_sim=True))
            _assert_same(got, want)
            if kind == "signs":  # (normalised, every norm is sqrt(d): the ties stay)
                _check_against_mirror(got[0], got[1], got[2], k)
                for s in (1, 2, 7, 0, HUGE):
                    few_splits(s)
                    idx, sc = _host(torch, *index.search(tq, k)[:2])
                    assert _bytes_equal(idx, got[0]) and _bytes_equal(sc, got[1]), s
                few_splits(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_than_16_queries_go_in_slices(env, dtype):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    dtype = getattr(torch, dtype)
    n, dim, k = 700, 64, 10
    q, g = _planted(40, n, dim, 5)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    index = GalleryIndex(tg, normalize=True, storage=dtype)
    ptr = index.gallery.data_ptr()
    for m in (17, 40):
        got = _host(torch, *index.search(tq[:m], k, want_sim=True))
        assert got[0].shape == (m, k) and got[2].shape == (m, n)
        _assert_same(got, _oracle(torch, tq[:m], tg, dtype, k, True))
        assert index.gallery.dtype == dtype and index.gallery.data_ptr() == ptr  # no fp32 copy took its place
    one = _host(torch, *index.search(tq[3], k)[:2])
    want = _oracle(torch, tq[3:4], tg, dtype, k, True)
    assert one[0].shape == (1, k) and _bytes_equal(one[0], want[0]) and _bytes_equal(one[1], want[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_refusals_write_nothing(env, dtype):
    torch, cva = env
    from coot_videotext_amd.retrieval import GALLERY_BF16, GALLERY_F16
    lib = cva.lib.load()
    dtype = getattr(torch, dtype)
    code = GALLERY_BF16 if dtype is torch.bfloat16 else GALLERY_F16
    m, n, dim = 16, 300, 16
    q, g = torch.randn(17, dim, device="cuda"), torch.randn(n, dim, device="cuda").to(dtype)
    gn = torch.empty(n, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.coot_retrieval_row_norms_h(g.data_ptr(), code, n, dim, gn.data_ptr(), st) == 0
    idx = torch.full((17, 129), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((17, 129), -7.0, device="cuda")
    ws = torch.zeros(lib.coot_retrieval_topk_few_workspace_bytes(m, n, dim, 128) + (1 << 20), dtype=torch.uint8, device="cuda")

    def call(mm, nn, k, ws_bytes, idx_ptr, dt=code):
        return lib.coot_retrieval_topk_few_h(q.data_ptr(), g.data_ptr(), dt, gn.data_ptr(), mm, nn, dim, k, idx_ptr, sc.data_ptr(), None, ws.data_ptr(),
                                             ws_bytes, st)
    cases = {"M = 17": (17, n, 10, ws.numel(), idx.data_ptr()), "K = 0": (m, n, 0, ws.numel(), idx.data_ptr()),
             "K > N": (m, 100, 101, ws.numel(), idx.data_ptr()), "K = 129": (m, n, 129, ws.numel(), idx.data_ptr()),
             "workspace": (m, n, 10, 64, idx.data_ptr()), "null output": (m, n, 10, ws.numel(), None),
             "dtype": (m, n, 10, ws.numel(), idx.data_ptr(), 7)}
    for what, args in cases.items():
        assert call(*args) != 0, what
        msg = lib.coot_last_error().decode()
        assert "retrieval_topk_few_h" in msg, (what, msg)
        assert {"M = 17": "M = 17", "workspace": "workspace too small", "null output": "null pointer", "dtype": "dtype = 7"}.get(what, "K = ") in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool((sc == -7.0).all()) and not bool(ws.any()), what
    assert call(m, n, 128, ws.numel(), idx.data_ptr()) == 0, lib.coot_last_error()  # the same buffers, accepted
    torch.cuda.synchronize()
    got = idx.view(-1)[:m * 128]
    assert bool(((got >= 0) & (got < n)).all()) and bool((idx.view(-1)[m * 128:] == -7).all())


@pytest.mark.parametrize("m,n,dim", [(16, 20000, 384), (16, 1000, 768)])
@pytest.mark.parametrize("dtype,bound", [("bfloat16", 4e-3), ("float16", 1e-3)])
def test_close_to_the_fp32_search(env, dtype, bound, m, n, dim):
    """How far 16-bit storage moves the result from the fp32 index on the unrounded gallery.  The bounds are derived, not measured:
    rounding a row's entries with relative error u moves the row by at most u times its length, and its normalised image (unit
    rows) by at most 2u / (1 - u); a similarity is a product with a unit query, so it moves by at most that, plus the 2e-6 chain
    bound of tests/test_gpu_topk.py.  bfloat16 (u = 2^-9): 4e-3; IEEE half (u = 2^-11): 1e-3.  On these planted inputs the gap
    between the best and the second best similarity is at least 0.044 on every row (the float64 product on the host), more than
    twice either bound, so the best gallery row cannot change.  Measured on the host: 4.1e-4 and 5.2e-5."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    k = 10
    q, g = _planted(m, n, dim, m + n + dim)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    idx32, _, sim32 = _host(torch, *GalleryIndex(tg, normalize=True).search(tq, k, want_sim=True))
    idx16, _, sim16 = _host(torch, *GalleryIndex(tg, normalize=True, storage=getattr(torch, dtype)).search(tq, k, want_sim=True))
    err = np.abs(sim16.astype(np.float64) - sim32.astype(np.float64)).max()
    top2 = np.sort(sim32, axis=1)[:, -2:]
    print(f"[{m} x {n} x {dim}, {dtype}] max |sim_16 - sim_32| = {err:.3e} (bound {bound:.0e}), smallest top-1 to top-2 gap = {(top2[:, 1] - top2[:, 0]).min():.4f}")
    assert err < bound
    assert np.array_equal(idx16[:, 0], idx32[:, 0])
