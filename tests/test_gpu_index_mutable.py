"""The mutable gallery index (coot_retrieval_rows_put; GalleryIndex.add / update / compact, capacity=) against its definition: the
stored bytes of a put are those of src.to(dtype), its norms those of the norm kernels on the stored rows, and an index that has
been grown, updated and compacted is — gallery, norms and every search — a freshly built index on the same rows.  Every comparison
is for byte equality.  (N, d): d = 72 is no multiple of 32, 30 no multiple of 8 and below 64 (lanes without an element), 40 below
64; N = 130 is a partial block of 128 and tile of 64, 300 and 1000 are several blocks.  R = 1, 3, 200: within a workgroup of four
rows, across one, across blocks of 128 rows and beyond the capacity.  In the growth test N is the size the index starts with."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(130, 72), (300, 30), (1000, 40)]
RS = (1, 3, 200)
STORAGES = ["float32", "bfloat16", "float16"]
PAIRS = [("float32", "float32"), ("float32", "bfloat16"), ("float32", "float16"), ("bfloat16", "bfloat16"), ("bfloat16", "float32"),
         ("float16", "float16"), ("float16", "float32")]  # source -> gallery: every pair the call allows
MK = [(1, 1), (3, 9), (16, 128), (17, 9)]
CODES = {"float32": 0, "bfloat16": 1, "float16": 2}
SENTINEL = {2: 0x5A5A, 4: 0x5A5A5A5A}  # per element size; as a float it is finite in all three types


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _bits(torch, t):
    """The tensor's bytes as integers, on the host."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


def _same(torch, a, b):
    a, b = _bits(torch, a), _bits(torch, b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _specials():
    """Rounding ties and their neighbours for bfloat16 (1 + 2^-8: half an ulp) and IEEE half (1 + 2^-11), signed zeros, values that
    are subnormal or vanish in IEEE half, the last finite half and the tie above it; then what is not finite somewhere."""
    one = np.float32(1)
    t8, t11 = np.float32(2.0 ** -8), np.float32(2.0 ** -11)
    fin = [one + t8, np.nextafter(one + t8, np.float32(2)), np.nextafter(one + t8, np.float32(0)), one + 3 * t8,
           one + t11, np.nextafter(one + t11, np.float32(2)), np.nextafter(one + t11, np.float32(0)), one + 3 * t11,
           0.0, -0.0, 1e-6, 6e-8, -6e-8, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 65519.0, 65520.0]
    wild = [np.inf, -np.inf, 7e4, -7e4, 3e38]
    return np.array(fin, np.float32), np.array(wild, np.float32)


_SRC = {}


def _source(d):
    """The fixed fp32 input [200, d], made once per width: random rows; rows 0, 1, 5 and 199 begin with the finite special values,
    row 1 goes on with the ones that overflow (so R = 1 has finite norms, R = 3 has infinite ones too)."""
    if d not in _SRC:
        fin, wild = _specials()
        x = np.random.RandomState(d).randn(200, d).astype(np.float32)
        for r in (0, 1, 5, 199):
            x[r, :len(fin)] = fin
        x[1, len(fin):len(fin) + len(wild)] = wild
        x.setflags(write=False)
        _SRC[d] = x
    return _SRC[d]


def _row_norms(torch, lib, buf):
    """coot_retrieval_row_norms / _h on a whole buffer."""
    n, d = buf.shape
    out = torch.empty(n, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if buf.dtype is torch.float32:
        assert lib.coot_retrieval_row_norms(buf.data_ptr(), n, d, out.data_ptr(), st) == 0
    else:
        assert lib.coot_retrieval_row_norms_h(buf.data_ptr(), CODES[str(buf.dtype)[6:]], n, d, out.data_ptr(), st) == 0
    return out


def _sentinel_buffer(torch, n, d, dtype):
    buf = torch.empty(n, d, dtype=dtype, device="cuda")
    buf.view(torch.int16 if buf.element_size() == 2 else torch.int32).fill_(SENTINEL[buf.element_size()])
    return buf


@pytest.mark.parametrize("src_t,gal_t", PAIRS)
def test_put_against_its_definition(env, src_t, gal_t):
    torch, cva = env
    lib = cva.lib.load()
    st = torch.cuda.current_stream().cuda_stream
    sdt, gdt = getattr(torch, src_t), getattr(torch, gal_t)
    for n, d in SHAPES:
        src_all = torch.tensor(_source(d), device="cuda").to(sdt)  # (a 16-bit source is the rounded input: itself a fixed input)
        assert not bool(torch.isnan(src_all.float()).any())
        want_all = src_all.to(gdt)  # the definition
        rs = np.random.RandomState(n + d)
        for r in RS:
            r = min(r, n)  # (N = 130: the 200 rows become the whole buffer)
            src, want = src_all[:r].contiguous(), _bits(torch, want_all[:r])
            perm = rs.permutation(n)[:r].astype(np.int32)
            if r >= 3:
                perm[[0, 2]] = [-1, n]  # skipped
            if r > 3:
                perm[[5, 7, r - 1]] = [n + 5, -(2 ** 31), 2 ** 31 - 1]
            for what, row0, dest in (("row0 = 0", 0, None), ("row0 = N - R", n - r, None), ("dest", 0, perm)):
                buf = _sentinel_buffer(torch, n, d, gdt)
                norms = torch.full((n,), -7.0, device="cuda")
                rows = np.arange(row0, row0 + r) if dest is None else dest.astype(np.int64)
                tdest = None if dest is None else torch.from_numpy(dest).cuda()
                rc = lib.coot_retrieval_rows_put(src.data_ptr(), CODES[src_t], r, d, None if dest is None else tdest.data_ptr(), row0,
                                                 buf.data_ptr(), CODES[gal_t], n, norms.data_ptr(), st)
                assert rc == 0, lib.coot_last_error()
                ref = _row_norms(torch, lib, buf)  # the norm kernel on what is stored now
                torch.cuda.synchronize()
                got, got_norms, ref = _bits(torch, buf), _bits(torch, norms), _bits(torch, ref)
                hit = (rows >= 0) & (rows < n)
                exp = np.full_like(got, SENTINEL[buf.element_size()])
                exp[rows[hit]] = want[hit]
                assert got.tobytes() == exp.tobytes(), (n, d, r, what, np.argwhere(got != exp)[:5])
                exp_norms = np.full(n, np.float32(-7.0)).view(np.int32)
                exp_norms[rows[hit]] = ref[rows[hit]]
                assert got_norms.tobytes() == exp_norms.tobytes(), (n, d, r, what, np.argwhere(got_norms != exp_norms)[:5])
                # norms == NULL: the rows alone
                buf2 = _sentinel_buffer(torch, n, d, gdt)
                assert lib.coot_retrieval_rows_put(src.data_ptr(), CODES[src_t], r, d, None if dest is None else tdest.data_ptr(), row0,
                                                   buf2.data_ptr(), CODES[gal_t], n, None, st) == 0
                assert _bits(torch, buf2).tobytes() == exp.tobytes(), (n, d, r, what, "no norms")
        if gal_t != "float32" and src_t == "float32":  # the fixed input did hold ties, and they went to even
            one = _bits(torch, torch.ones(1, device="cuda").to(gdt))[0]
            i = 0 if gal_t == "bfloat16" else 4
            assert _bits(torch, want_all)[0, i] == one and _bits(torch, want_all)[0, i + 1] == one + 1 and _bits(torch, want_all)[0, i + 3] == one + 2


_DATA = {}


def _data(total, d):
    """(queries [17, d], rows [total, d]) on the host, query i planted on row i * 37 mod total.  Made once, read only."""
    if (total, d) not in _DATA:
        rs = np.random.RandomState(total + d)
        g = rs.randn(total, d).astype(np.float32)
        q = (0.35 * g[np.arange(17) * 37 % total] + rs.randn(17, d)).astype(np.float32)
        q.setflags(write=False)
        g.setflags(write=False)
        _DATA[(total, d)] = (q, g)
    return _DATA[(total, d)]


def _searches(torch, index, tq, keep=None):
    """The results of every (M, K) of MK, on the host as integers."""
    out = []
    for m, k in MK:
        idx, sc, _ = index.search(tq[:m], min(k, len(index)), keep=keep)
        out.append((_bits(torch, idx), _bits(torch, sc)))
    return out


def _assert_same_index(torch, index, fresh, tq, what):
    assert len(index) == index.n == len(fresh) and index.gallery.shape == fresh.gallery.shape, what
    assert index.gallery.dtype == fresh.gallery.dtype and index.gallery.is_contiguous(), what
    assert _same(torch, index.gallery, fresh.gallery), what
    assert (index.norms is None) == (fresh.norms is None), what
    if fresh.norms is not None:
        assert index.norms.shape == fresh.norms.shape and _same(torch, index.norms, fresh.norms), what
    for (m, k), got, want in zip(MK, _searches(torch, index, tq), _searches(torch, fresh, tq)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (what, m, k)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n0,d", SHAPES)
@pytest.mark.parametrize("storage", STORAGES)
def test_a_grown_index_is_a_fresh_index(env, storage, n0, d, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    sdt = getattr(torch, storage)
    outgrew = 0
    for r in RS:
        pieces = [r, r, (r + 1) // 2]  # the last piece is a short one
        total = n0 + sum(pieces)
        q, g = _data(total, d)
        tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        fresh = GalleryIndex(tg, normalize=normalize, storage=sdt)
        for capacity in (None, total):
            for piece_t in ((torch.float32,) if storage == "float32" else (torch.float32, sdt)):
                what = (r, capacity, piece_t)
                start = tg[:n0].to(sdt)  # by reference when capacity is None: the caller's tensor
                before = _bits(torch, start).copy()
                index = GalleryIndex(start, normalize=normalize, capacity=capacity)
                assert index.storage is sdt and len(index) == n0 and index.capacity == (capacity or n0), what
                assert (index.gallery.data_ptr() == start.data_ptr()) == (capacity is None), what
                at = n0
                for p in pieces:
                    ptr, cap = index.gallery.data_ptr(), index.capacity
                    first = index.add(tg[at:at + p].to(piece_t) if p > 1 else tg[at].to(piece_t))  # ([d] is one row)
                    assert first == at and len(index) == at + p, what
                    grew = at + p > cap
                    assert (index.gallery.data_ptr() != ptr) == grew, (what, at)  # into spare capacity: in place
                    assert index.capacity == (max(2 * cap, at + p) if grew else cap), (what, at)
                    assert index.nbytes == index.capacity * (d * index.gallery.element_size() + (4 if normalize else 0)), what
                    outgrew += grew
                    at += p
                assert capacity is None or index.capacity == total, what
                assert index.add(tg[:0]) == total and len(index) == total  # R == 0: nothing happens
                _assert_same_index(torch, index, fresh, tq, what)
                assert _bits(torch, start).tobytes() == before.tobytes(), what  # the caller's tensor was never written
                assert index.gallery.data_ptr() != start.data_ptr(), what
    assert outgrew >= 3
    # fp32 rows into 16-bit storage given to the constructor: the same, starting from a converted (owned) copy
    if storage != "float32":
        q, g = _data(n0 + 5, d)
        tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
        index = GalleryIndex(tg[:n0], normalize=normalize, storage=sdt)
        assert index.add(tg[n0:]) == n0
        _assert_same_index(torch, index, GalleryIndex(tg, normalize=normalize, storage=sdt), tq, "converted")
        with pytest.raises(ValueError):
            index.add(tg[:2].to(torch.float16 if storage == "bfloat16" else torch.bfloat16))
    # a filter grows with the buffer and the new rows are kept
    q, g = _data(n0 + 203, d)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda")
    index = GalleryIndex(tg[:n0], normalize=normalize, storage=sdt)
    gone = [0, n0 // 2, n0 - 1]
    index.remove(gone)
    index.add(tg[n0:n0 + 200])
    index.add(tg[n0 + 200:])
    mask = np.ones(n0 + 203, bool)
    mask[gone] = False
    assert index.keep.shape == (n0 + 203,) and index.keep.dtype is torch.bool and index.keep.cpu().numpy().tolist() == mask.tolist()
    fresh = GalleryIndex(tg, normalize=normalize, storage=sdt)
    want = _searches(torch, fresh, tq, keep=torch.from_numpy(mask).cuda())
    for got, exp in zip(_searches(torch, index, tq), want):
        assert got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("storage", STORAGES)
def test_update(env, storage, n, d, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    sdt = getattr(torch, storage)
    q, g = _data(n, d)
    tq = torch.tensor(q, device="cuda")
    rs = np.random.RandomState(n + d + 1)
    model = torch.tensor(g, device="cuda").to(sdt)  # the patched gallery, in the storage type
    start = model.clone()
    before = _bits(torch, start).copy()
    index = GalleryIndex(start, normalize=normalize)  # by reference
    assert index.gallery.data_ptr() == start.data_ptr()
    dev_rows = rs.randint(0, n, size=200)
    dev_rows[[3, 9, 50]] = [-1, n, n + 7]   # ignored
    dev_rows[[10, 60, 199]] = dev_rows[4]   # one row four times: position 199 wins
    plans = [("host list", [int(x) for x in rs.permutation(n)[:3]], torch.float32),
             ("CPU tensor", torch.tensor([n - 1]), sdt),
             ("device tensor", torch.tensor(dev_rows, device="cuda", dtype=torch.int32), torch.float32),
             ("device tensor, storage rows", torch.tensor(dev_rows[::-1].copy(), device="cuda"), sdt)]
    for what, rows, vt in plans:
        host_rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows).reshape(-1)
        values = torch.tensor(rs.randn(len(host_rows), d).astype(np.float32), device="cuda").to(vt)
        index.update(rows, values)
        for p, row in enumerate(host_rows):  # in order: of a repeated row the highest position stays
            if 0 <= row < n:
                model[row] = values[p].to(sdt)
        assert len(index) == n and index.capacity == n and index.keep is None, what
        assert index.gallery.data_ptr() != start.data_ptr(), what
        _assert_same_index(torch, index, GalleryIndex(model.clone(), normalize=normalize), tq, what)
    assert _bits(torch, start).tobytes() == before.tobytes()  # the caller's tensor was never written
    index.update([], torch.empty(0, d, device="cuda"))  # nothing to do
    # a removed row that is updated stays out of the results, and comes back with its new value
    row = int(rs.randint(0, n))
    index.remove([row])
    index.update([row], 3.0 * tq[0])  # query 0's certain best, were it searched
    model[row] = (3.0 * tq[0]).to(sdt)
    assert index.keep is not None and not bool(index.keep[row]) and int(index.keep.sum()) == n - 1
    fresh = GalleryIndex(model.clone(), normalize=normalize)
    mask = torch.ones(n, dtype=torch.bool, device="cuda")
    mask[row] = False
    for got, want in zip(_searches(torch, index, tq), _searches(torch, fresh, tq, keep=mask)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert not (got[0] == row).any()
    index.restore([row])
    _assert_same_index(torch, index, fresh, tq, "restored")
    assert int(index.search(tq[:1], 1)[0][0, 0]) == row
    with pytest.raises(ValueError):
        index.update([1, 1], values[:2])
    with pytest.raises(IndexError):
        index.update([n], values[:1])


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("storage", STORAGES)
def test_compact(env, storage, n, d, normalize):
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    sdt = getattr(torch, storage)
    q, g = _data(n, d)
    tq, tg = torch.tensor(q, device="cuda"), torch.tensor(g, device="cuda").to(sdt)
    rs = np.random.RandomState(n)
    half = np.nonzero(rs.rand(n) < 0.5)[0]
    block = np.arange(128, min(256, n))
    plans = {"random half": [half], "a whole block": [block], "the last row": [[n - 1]], "all three": [half, block, [n - 1]]}
    for what, removals in plans.items():
        for capacity in (None, n + 50):
            index = GalleryIndex(tg, normalize=normalize, capacity=capacity)
            keep = np.ones(n, bool)
            for rows in removals:
                index.remove(torch.tensor(np.asarray(rows), device="cuda"))
                keep[np.asarray(rows)] = False
            kept = int(keep.sum())
            filtered = _searches(torch, index, tq)
            old = index.compact()
            assert old.dtype is torch.int32 and old.is_cuda and old.cpu().numpy().tolist() == np.nonzero(keep)[0].tolist(), what
            assert index.keep is None and len(index) == index.n == index.capacity == kept, what
            fresh = GalleryIndex(tg[torch.from_numpy(keep).cuda()], normalize=normalize)
            _assert_same_index(torch, index, fresh, tq, what)
            assert index.nbytes == fresh.nbytes and index.nbytes < GalleryIndex(tg, normalize=normalize).nbytes, what
            old_host = old.cpu().numpy()
            for (m, k), was, now in zip(MK, filtered, _searches(torch, index, tq)):
                if k <= kept:  # the search before is filtered at this K; with fewer rows kept, _searches lowered K after compact
                    assert old_host[now[0]].tobytes() == was[0].tobytes() and now[1].tobytes() == was[1].tobytes(), (what, m, k)
            again = index.compact()  # no filter: arange(n), nothing moves
            ptr = index.gallery.data_ptr()
            assert again.dtype is torch.int32 and again.cpu().numpy().tolist() == list(range(kept)) and index.gallery.data_ptr() == ptr
            assert index.add(tg[:3]) == kept and len(index) == kept + 3  # and the compacted index goes on growing
    index = GalleryIndex(tg, normalize=normalize)
    index.remove(torch.arange(n, device="cuda"))
    with pytest.raises(ValueError):
        index.compact()
    assert len(index) == n and index.keep is not None and index.gallery.data_ptr() == tg.data_ptr()


def test_a_sequence_of_operations(env):
    """About 30 random operations on a bfloat16 index, mirrored by a numpy model of (rows, keep): after every one the index
    searches as a fresh index on the model's rows searches under the model's keep."""
    torch, cva = env
    from coot_videotext_amd.retrieval import GalleryIndex
    n0, d, k = 130, 40, 9
    rs = np.random.RandomState(16)
    rows = rs.randn(n0, d).astype(np.float32)
    keep = np.ones(n0, bool)
    tq = torch.tensor((0.35 * rows[np.arange(16) * 7] + rs.randn(16, d)).astype(np.float32), device="cuda")
    index = GalleryIndex(torch.tensor(rows, device="cuda"), normalize=True, storage=torch.bfloat16)
    done = {}
    for step in range(32):
        op = ["add", "remove", "restore", "update", "compact"][step % 5] if step < 10 else rs.choice(["add", "remove", "restore", "update", "compact"])
        n = len(rows)
        if op == "add":
            r = int(rs.choice(RS))
            new = rs.randn(r, d).astype(np.float32)
            t = torch.tensor(new, device="cuda")
            if rs.rand() < 0.5:
                t = t.to(torch.bfloat16)
                new = t.float().cpu().numpy()
            assert index.add(t) == n
            rows, keep = np.concatenate([rows, new]), np.concatenate([keep, np.ones(r, bool)])
        elif op == "remove":
            gone = rs.randint(0, n, size=int(rs.randint(1, 8)))
            index.remove(torch.tensor(gone, device="cuda") if rs.rand() < 0.5 else [int(x) for x in gone])
            keep[gone] = False
        elif op == "restore":
            back = np.nonzero(~keep)[0]
            back = back[rs.rand(len(back)) < 0.5]
            index.restore([int(x) for x in back])
            keep[back] = True
        elif op == "update":
            which = rs.permutation(n)[:int(rs.randint(1, 6))]
            new = rs.randn(len(which), d).astype(np.float32)
            index.update(torch.tensor(which, device="cuda") if rs.rand() < 0.5 else [int(x) for x in which], torch.tensor(new, device="cuda"))
            rows = rows.copy()
            rows[which] = new
        else:
            old = index.compact()
            assert old.cpu().numpy().tolist() == np.nonzero(keep)[0].tolist(), step
            rows, keep = rows[keep], np.ones(int(keep.sum()), bool)
            assert index.keep is None and index.capacity == len(rows)
        done[op] = done.get(op, 0) + 1
        assert len(index) == len(rows) and keep.sum() >= k, (step, op)
        fresh = GalleryIndex(torch.tensor(rows, device="cuda"), normalize=True, storage=torch.bfloat16)
        want = fresh.search(tq, k, keep=torch.from_numpy(keep).cuda())
        got = index.search(tq, k)
        assert _same(torch, got[0], want[0]) and _same(torch, got[1], want[1]), (step, op)
        assert _same(torch, index.gallery, fresh.gallery) and _same(torch, index.norms, fresh.norms), (step, op)
    assert len(done) == 5 and min(done.values()) >= 2, done


def test_put_refusals_write_nothing(env):
    """Refused calls return before any launch: a sentinel-filled gallery and norms stay as they are (the pattern of
    tests/test_gpu_topk_masked.py::test_masked_refusals_write_nothing), and the same buffers are then accepted."""
    torch, cva = env
    lib = cva.lib.load()
    n, d, r = 300, 30, 5
    st = torch.cuda.current_stream().cuda_stream
    src = {t: torch.randn(r, d, device="cuda").to(getattr(torch, t)) for t in STORAGES}
    gal = {t: _sentinel_buffer(torch, n, d, getattr(torch, t)) for t in STORAGES}
    norms = torch.full((n,), -7.0, device="cuda")
    dest = torch.arange(r, dtype=torch.int32, device="cuda")

    def put(s="float32", g="float32", rr=r, dd=d, nn=n, row0=0, dst=None, src_ptr=True, gal_ptr=True, scode=None, gcode=None):
        return lib.coot_retrieval_rows_put(src[s].data_ptr() if src_ptr else None, CODES[s] if scode is None else scode, rr, dd,
                                           dst.data_ptr() if dst is not None else None, row0, gal[g].data_ptr() if gal_ptr else None,
                                           CODES[g] if gcode is None else gcode, nn, norms.data_ptr(), st)
    cases = {"null src": (dict(src_ptr=False), "null pointer"), "null gallery": (dict(gal_ptr=False), "null pointer"),
             "R = 0": (dict(rr=0), "R = 0"), "R < 0": (dict(rr=-1), "R = -1"), "d = 0": (dict(dd=0), "d = 0"), "N = 0": (dict(nn=0), "N = 0"),
             "bf16 into f16": (dict(s="bfloat16", g="float16"), "src_dtype = 1, gallery_dtype = 2"),
             "f16 into bf16": (dict(s="float16", g="bfloat16"), "src_dtype = 2, gallery_dtype = 1"),
             "unknown source type": (dict(scode=7), "src_dtype = 7"), "unknown gallery type": (dict(gcode=3), "gallery_dtype = 3"),
             "negative type": (dict(scode=-1), "src_dtype = -1"),
             "row0 < 0": (dict(row0=-1), "are not inside"), "row0 + R > N": (dict(row0=n - r + 1), "are not inside"),
             "row0 = N": (dict(row0=n), "are not inside"), "row0 overflows": (dict(row0=2 ** 31 - 1), "are not inside"),
             "row0 with dest": (dict(row0=1, dst=dest), "row0 = 1 with dest")}
    for what, (kw, part) in cases.items():
        assert put(**kw) != 0, what
        msg = lib.coot_last_error().decode()
        assert msg.startswith("retrieval_rows_put:") and part in msg, (what, msg)
        torch.cuda.synchronize()
        for t in STORAGES:
            assert bool((gal[t].view(torch.int16 if t != "float32" else torch.int32) == SENTINEL[gal[t].element_size()]).all()), (what, t)
        assert bool((norms == -7.0).all()), what
    for kw in (dict(row0=n - r), dict(dst=dest), dict(s="bfloat16", g="bfloat16", row0=7), dict(s="float16", g="float32", dst=dest)):
        assert put(**kw) == 0, lib.coot_last_error()
        torch.cuda.synchronize()
        assert int((norms != -7.0).sum()) == r and not bool((gal[kw.get("g", "float32")] == gal[kw.get("g", "float32")][n // 2]).all())
        norms.fill_(-7.0)
