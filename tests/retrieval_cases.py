"""Inputs and comparisons the retrieval GPU tests share (tests/test_gpu_topk.py, _topk_few.py, _topk_half.py, _topk_masked.py,
_labeled.py): the planted query / gallery pair, byte equality, and the top-K result against the host mirror."""
import numpy as np

_PLANTED = {}


def planted(m, n, dim, seed):
    """The recipe of tests/test_retrieval_device.py (random rows with a planted match, so the best items are neither random nor
    trivial), for M != N: query i is planted on gallery row i mod N.  Made once per shape and seed and shared (read only)."""
    key = (m, n, dim, seed)
    if key not in _PLANTED:
        rs = np.random.RandomState(seed)
        g = rs.randn(n, dim).astype(np.float32)
        q = (0.35 * g[np.arange(m) % n] + rs.randn(m, dim)).astype(np.float32)
        q.setflags(write=False)
        g.setflags(write=False)
        _PLANTED[key] = (q, g)
    return _PLANTED[key]


def unit(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(torch, *tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def check_against_mirror(idx, sc, sim, k):
    from coot_videotext_amd.retrieval import compute_retrieval_topk
    want_idx, want_sc = compute_retrieval_topk(sim, k)
    assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (sim.shape[0], k)
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    assert np.array_equal(sc, want_sc) and np.array_equal(sc, np.take_along_axis(sim, idx.astype(np.int64), axis=1))
