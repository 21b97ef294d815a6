"""The retrieval results for embeddings that live on the MI355X, computed by libcoot_hip.so.  No CPU fallback: CUDA tensors in,
device kernels or an error that names the host mirror.  The mirrors themselves (numpy, the byte-exact definitions of everything
below) are retrieval_mirror.py; their names are re-exported here.

compute_retrieval_device: the dictionaries of compute_retrieval (coot_retrieval_ranks_part + coot_retrieval_metrics: normalisation,
similarities, both rank vectors and the metric dictionaries in four launches, the N x N matrix is never materialised).

retrieval_topk_device: WHICH gallery items a query retrieves (compute_retrieval_topk), M queries against N gallery rows: the tile
search (similarities and selection fused, no M x N matrix).  GalleryIndex: the same search on a gallery that stays on the device, in
float32, bfloat16 or float16, its row norms computed once: a few queries at a time (one sweep of the gallery) or a whole query set
(retrieval_topk_index_device: the tile search on the gallery as the index holds it).  keep= / GalleryIndex.remove: a flag per gallery
row that the selection consults (compute_retrieval_topk_masked).  One library call per search: coot_retrieval_topk_masked (tile),
coot_retrieval_topk_index (tile, on an index), coot_retrieval_topk_few_masked (few queries, any storage).
retrieval_topk_grouped_device / GalleryIndex.search_grouped: the K best GROUPS of gallery rows, each through its best row
(compute_retrieval_topk_grouped): coot_retrieval_topk_grouped.  retrieval_topk_multi_device / GalleryIndex.search_multi: the K best
groups for a PARAGRAPH of queries (compute_retrieval_topk_multi): coot_retrieval_topk_multi.  retrieval_topk_scoped_device /
GalleryIndex.search_scoped: every query inside (only=) or outside (exclude=) the rows with the id it brings
(compute_retrieval_topk_scoped): coot_retrieval_topk_scoped; GalleryIndex.neighbors: a row's neighbours outside its own group.
retrieval_topk_adjusted_device / GalleryIndex.search_adjusted: a number per gallery row taken off its similarity before the selection
(compute_retrieval_topk_adjusted): coot_retrieval_topk_adjusted in slices of 16 and, from ADJUSTED_TILE_MIN_M* queries on, one call of
coot_retrieval_topk_adjusted_tile (_topk_adjusted); GalleryIndex.hubness_offsets: the offsets that make it rank by CSLS
(compute_retrieval_hub_offsets): coot_retrieval_knn_join against a bank of queries, then coot_retrieval_hub_offsets.
retrieval_range_device / GalleryIndex.search_range, count_range: every row at or above a query's threshold, however many, as CSR
(compute_retrieval_range): coot_retrieval_range_count, _scan, _fill for up to RANGE_TILE_MIN_M* - 1 queries, in slices of 16, and
coot_retrieval_range_tile_count, _scan, _tile_fill from there on, one call per pass (_range).
retrieval_self_join_device / GalleryIndex.self_join, count_self_join: the gallery against itself, all pairs (i, j), i < j, at or above
row i's threshold, as the same CSR (compute_retrieval_self_join): coot_retrieval_join_count, _scan, coot_retrieval_join_fill per chunk
of rows, the chunks sized by JOIN_TABLE_BYTES (_self_join).
retrieval_components_device / GalleryIndex.components, deduplicate: the connected components of those pairs, a cluster label per row
(compute_retrieval_components): one call of coot_retrieval_components, one sweep of the upper triangle, no pair list (_components).
retrieval_join_device / GalleryIndex.join, count_join: the rows of one index against the rows of another, all pairs at or above the
left row's threshold, as the same CSR (compute_retrieval_join): coot_retrieval_cross_join_count, _scan, coot_retrieval_cross_join_fill
per chunk of left rows, under the same budget (_cross_join).
retrieval_knn_join_device / GalleryIndex.knn_join, knn_graph: the k best partners of EVERY row of an index, in a second index or in
itself, under the joins' filters (compute_retrieval_knn_join): one call of coot_retrieval_knn_join, both sides read as stored (_knn_join).
The searches on a prepared gallery share one host check (_check_search) and have one implementation per library call (_topk_few,
_topk_tile, _topk_grouped, _topk_multi, _topk_scoped, _topk_adjusted), which the public wrapper and the GalleryIndex method both call.
GalleryIndex.add / update / compact: rows appended or overwritten in place together with their norms (coot_retrieval_rows_put),
removed rows dropped — the index then holds, byte for byte, what a fresh index on the same rows holds.

Sharded validation (data-parallel runs): retrieval_ranks_part_device counts one strip of rows, an integer all-reduce of the
strips is the whole (compute_retrieval_device(dp=...)), retrieval_metrics_device turns rank vectors into the metrics.
Labelled ranking (retrieval_ranks_labeled_device / compute_retrieval_labeled_device): compute_retrieval_labeled on the device; under a
number per gallery row and per query (retrieval_ranks_adjusted_device / compute_retrieval_adjusted_device: compute_retrieval_labeled_adjusted,
coot_retrieval_ranks_adjusted), and compute_retrieval_csls_device: the metrics of a validation pair under CSLS."""
from __future__ import annotations

import numpy as np

from .retrieval_mirror import (VALKEYS, _ahead, _host_offsets, _labeled_metrics, compute_retrieval, compute_retrieval_cosine,  # noqa: F401
                               compute_retrieval_counts_part, compute_retrieval_labeled, compute_retrieval_topk, compute_retrieval_topk_grouped,
                               compute_retrieval_range, compute_retrieval_topk_masked, compute_retrieval_topk_multi, compute_retrieval_topk_scoped,
                               compute_retrieval_self_join, compute_retrieval_components, compute_retrieval_join, compute_retrieval_knn_join,
                               compute_retrieval_topk_adjusted, compute_retrieval_hub_offsets, compute_retrieval_labeled_adjusted, strip_bounds)


def _ptr(t):
    """The address of a tensor for the library, NULL for None."""
    return None if t is None else t.data_ptr()


def _stream():
    """The handle of the current stream: every launch goes there."""
    import torch
    return torch.cuda.current_stream().cuda_stream


def _on_device(fn: str, mirror: str, *tensors):
    """CUDA tensors (None: not given), or the error that names the host mirror."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{fn} needs CUDA tensors (there is no CPU fallback; use {mirror})")


def _check_keep(fn: str, keep, n: int, mirror: str = "compute_retrieval_topk_masked"):
    """The keep argument of a filtered search, checked on the host before anything is launched: a torch.bool or torch.uint8 tensor
    [N] (ValueError), on the device (RuntimeError naming the host mirror; mirror=None: the caller checks the device).  Returns it as
    contiguous bytes (a view where it can be)."""
    import torch
    if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{fn}: keep has to be a torch.bool or torch.uint8 tensor, not {getattr(keep, 'dtype', type(keep).__name__)}")
    if tuple(keep.shape) != (n,):
        raise ValueError(f"{fn}: keep of shape {tuple(keep.shape)}, a gallery of {n} rows (one flag per row: [{n}])")
    if mirror is not None:
        _on_device(fn, mirror, keep)
    keep = keep.contiguous()
    return keep.view(torch.uint8) if keep.dtype is torch.bool else keep


def _device_pair(fn: str, host: str, a, b, dtype, same_shape: bool = True, dim: int = 2):
    """The entry of every *_device wrapper: CUDA tensors or an error naming the host mirror, the dtype and the dimension
    asserted (and equal shapes, unless only the row width has to agree), contiguous copies returned."""
    _on_device(fn, host, a, b)
    assert a.dtype == dtype and b.dtype == dtype and a.dim() == dim and b.dim() == dim, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.shape == b.shape if same_shape else a.shape[1] == b.shape[1], (a.shape, b.shape)
    return a.contiguous(), b.contiguous()


def retrieval_ranks_device(emb1, emb2, normalize: bool = False, want_sim: bool = False):
    """emb1, emb2: cuda float32 [N, d].  Returns (ranks_12 int32 [N], ranks_21 int32 [N], metrics float32 [2, 7], sim or None),
    all on the device (no synchronisation)."""
    import torch
    from . import lib as _lib
    emb1, emb2 = _device_pair("retrieval_ranks_device", "compute_retrieval", emb1, emb2, torch.float32)
    n, d = emb1.shape
    lib = _lib.load()
    ws = torch.empty(lib.coot_retrieval_workspace_bytes(n, d), dtype=torch.uint8, device=emb1.device)
    r12 = torch.empty(n, dtype=torch.int32, device=emb1.device)
    r21 = torch.empty(n, dtype=torch.int32, device=emb1.device)
    met = torch.empty(2, 7, dtype=torch.float32, device=emb1.device)
    sim = torch.empty(n, n, dtype=torch.float32, device=emb1.device) if want_sim else None
    _lib.check(lib.coot_retrieval_ranks(emb1.data_ptr(), emb2.data_ptr(), n, d, int(normalize), r12.data_ptr(), r21.data_ptr(),
                                        met.data_ptr(), _ptr(sim), ws.data_ptr(), ws.numel(), _stream()), "coot_retrieval_ranks")
    return r12, r21, met, sim


def _topk_buffers(ws_bytes: int, m: int, n: int, k: int, want_sim: bool, dev):
    """What a top-K call writes: (workspace bytes, idx int32 [M, k], scores float32 [M, k], sim float32 [M, N] or None), uninitialised."""
    import torch
    return (torch.empty(ws_bytes, dtype=torch.uint8, device=dev), torch.empty(m, max(k, 0), dtype=torch.int32, device=dev),
            torch.empty(m, max(k, 0), dtype=torch.float32, device=dev), torch.empty(m, n, dtype=torch.float32, device=dev) if want_sim else None)


def retrieval_topk_device(queries, gallery, k: int, normalize: bool = False, want_sim: bool = False, keep=None):
    """queries [M, d], gallery [N, d]: cuda float32.  Returns (idx int32 [M, k], scores float32 [M, k], sim [M, N] or None), all
    on the device (no synchronisation): compute_retrieval_topk of the fp32 similarities retrieval_ranks_device counts on, without
    the M x N matrix (want_sim is a testing aid).  1 <= k <= min(N, 128).
    keep: a cuda torch.bool or torch.uint8 tensor [N], nonzero = the row may be returned: the bytes of
    this call on gallery[keep] with the indices mapped back to rows of gallery, compute_retrieval_topk_masked of the similarities;
    k is still checked against N, and with fewer than k kept rows the tail of every row is idx = -1, score = -inf.  sim holds every
    similarity, masked rows included.  keep=None: the unfiltered search.  Either way one call of coot_retrieval_topk_masked, which
    without keep launches the kernels of coot_retrieval_topk."""
    import torch
    from . import lib as _lib
    if keep is not None:
        assert gallery.dim() == 2, gallery.shape
        keep = _check_keep("retrieval_topk_device", keep, gallery.shape[0])
    queries, gallery = _device_pair("retrieval_topk_device", "compute_retrieval_topk" + ("_masked" if keep is not None else ""), queries, gallery,
                                    torch.float32, same_shape=False)
    (m, d), n, k = queries.shape, gallery.shape[0], int(k)
    lib = _lib.load()
    ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_workspace_bytes(m, n, d, k), m, n, k, want_sim, queries.device)
    _lib.check(lib.coot_retrieval_topk_masked(queries.data_ptr(), gallery.data_ptr(), _ptr(keep), m, n, d, k, int(normalize), idx.data_ptr(),
                                              scores.data_ptr(), _ptr(sim), ws.data_ptr(), ws.numel(), _stream()), "coot_retrieval_topk_masked")
    return idx, scores, sim


RETRIEVAL_FEW_MAX = 16  # include/coot_hip.h: COOT_RETRIEVAL_FEW_MAX
GALLERY_BF16, GALLERY_F16 = 1, 2  # include/coot_hip.h: COOT_GALLERY_BF16, COOT_GALLERY_F16
_STORAGE_NAMES = "torch.float32, torch.bfloat16 or torch.float16"


def _gallery_codes():
    """torch dtype -> COOT_GALLERY_* code."""
    import torch
    return {torch.float32: 0, torch.bfloat16: GALLERY_BF16, torch.float16: GALLERY_F16}


# GalleryIndex.search on a 16-bit index: from this many queries on, one tile call (coot_retrieval_topk_index); below it, slices of
# RETRIEVAL_FEW_MAX queries through the few-query call, one sweep of the gallery each.  The tile walk runs at most 64 workgroups per 64
# queries, so up to 256 queries it takes about as long as for 17 (5.9 - 7.7 ms at 200 000 x 768, where a sweep takes 0.3 - 0.45 ms).
# The smallest measured M from which the tile call is no slower than the slices at both measured galleries (profiles/r17_topk_index.json:
# M = 17, 32, 64, 256, 320, 512, 1 024): at 200 000 x 768 it loses up to and including 256 queries (6.94 against 6.79 ms, more than the
# slices' spread) and wins from 320 (6.94 against 9.19); at 18 000 x 384 it already wins from 64 filtered and 256 unfiltered (0.75
# against 2.62 ms), which this one threshold leaves to the slices.  A float32 index takes the tile call from 17 queries on: there the
# alternative was the same walk plus a pass over the gallery for its norms.
INDEX_TILE_MIN_M_16BIT = 320


def retrieval_topk_index_device(queries, gallery, norms, k: int, keep=None, want_sim: bool = False):
    """The tile search on a gallery as a prepared index holds it (coot_retrieval_topk_index): queries cuda float32 [M, d], gallery
    cuda float32, bfloat16 or float16 [N, d], norms cuda float32 [N] = the gallery's row norms as coot_retrieval_row_norms(_h)
    writes them (GalleryIndex.norms), or None: rows used as they are.  Returns (idx int32 [M, k], scores float32 [M, k], sim [M, N] or
    None) on the device, no synchronisation: the bytes of retrieval_topk_device(queries, gallery.float(), k, normalize=norms is not
    None, keep=keep), without the widened copy and without a pass over the gallery for its norms — they are read, not checked.
    Any M >= 1, 1 <= k <= min(N, 128); keep as in retrieval_topk_device."""
    return _topk_tile(queries, gallery, norms, k, keep, want_sim)


def _check_groups(fn: str, groups, n: int, mirror: str = "compute_retrieval_topk_grouped"):
    """The groups argument of a grouped search, checked on the host before anything is launched: a torch.int32 or torch.int64 tensor
    [N] (ValueError), on the device (RuntimeError naming the host mirror; mirror=None: the caller checks the device).  Returns it as
    contiguous int32 (int64 is converted)."""
    import torch
    if not isinstance(groups, torch.Tensor) or groups.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: groups has to be a torch.int32 or torch.int64 tensor, not {getattr(groups, 'dtype', type(groups).__name__)}")
    if tuple(groups.shape) != (n,):
        raise ValueError(f"{fn}: groups of shape {tuple(groups.shape)}, a gallery of {n} rows (one group id per row: [{n}])")
    if mirror is not None:
        _on_device(fn, mirror, groups)
    return groups.to(torch.int32).contiguous()


def _gallery_code(fn: str, gallery):
    """The COOT_GALLERY_* code of the gallery's dtype, or the ValueError."""
    code = _gallery_codes().get(gallery.dtype)
    if code is None:
        raise ValueError(f"{fn}: a gallery of dtype {gallery.dtype}; it has to be {_STORAGE_NAMES}")
    return code


def _check_search(fn: str, mirror: str, queries, gallery, norms, k: int, detail=None, also=(), method=None, held: bool = False):
    """The host checks every search on a prepared gallery ends with.  For a wrapper (fn), in this order: queries, gallery, norms and
    `also` on the device (RuntimeError naming the mirror); the gallery's dtype (ValueError); float32 queries [M, d] (asserted, showing
    `detail`); equal widths, 1 <= k <= min(N, 128) (ValueError); float32 norms [N] or None (asserted).  For a GalleryIndex method
    (method: its name): what the caller brings first, under the method's name, then the index's gallery and norms under the wrapper's;
    held: those are taken as the constructor left them (the few-query route of GalleryIndex.search, which has to stay short).
    Returns the contiguous (queries, gallery, norms), the gallery's COOT_GALLERY_* code (held: None) and (m, n, d, k)."""
    import torch
    who = method or fn
    _on_device(who, mirror, queries, *(() if method else (gallery, norms)), *also)
    code = None if method else _gallery_code(fn, gallery)
    assert queries.dtype == torch.float32 and queries.dim() == 2 and gallery.dim() == 2, detail or (queries.dtype, queries.shape)
    (m, d), n, k = queries.shape, gallery.shape[0], int(k)
    if gallery.shape[1] != d:
        raise ValueError(f"{who}: queries of width {d}, gallery of width {gallery.shape[1]}")
    if not 1 <= k <= min(n, 128):
        raise ValueError(f"{who}: k = {k} is outside 1 .. min(N = {n}, 128)")
    if held:
        return (queries.contiguous(), gallery, norms), None, (m, n, d, k)
    if method is not None:
        _on_device(fn, mirror, gallery, norms)
        code = _gallery_code(fn, gallery)
    assert norms is None or (norms.dtype == torch.float32 and tuple(norms.shape) == (n,)), (norms.dtype, norms.shape, n)
    return (queries.contiguous(), gallery.contiguous(), None if norms is None else norms.contiguous()), code, (m, n, d, k)


def _and_own(own, keep):
    """The checked keep of one search (bytes or None) ANDed with the filter an index holds itself (None: none), as bytes."""
    if own is None:
        return keep
    import torch
    return (own if keep is None else own & (keep != 0)).view(torch.uint8)


def _topk_few(index, queries, k: int, keep, want_sim: bool):
    """coot_retrieval_topk_few_masked on an index (GalleryIndex.search): slices of RETRIEVAL_FEW_MAX queries over one workspace; [d] is one query."""
    from . import lib as _lib
    fn, gallery, norms, code = "GalleryIndex.search", index.gallery, index.norms if index.normalize else None, index._code
    if keep is not None:
        keep = _check_keep(fn, keep, gallery.shape[0])
    queries = queries[None] if queries.dim() == 1 else queries
    (queries, gallery, norms), _, (m, n, d, k) = _check_search(fn, "compute_retrieval_topk", queries, gallery, norms, k, method=fn, held=True)
    keep = _and_own(index.keep, keep)
    lib = _lib.load()
    ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_few_workspace_bytes(min(m, RETRIEVAL_FEW_MAX), n, d, k), m, n, k, want_sim,
                                         queries.device)
    st = _stream()
    for i in range(0, m, RETRIEVAL_FEW_MAX):  # the calls of a stream run in order: one workspace
        mm = min(RETRIEVAL_FEW_MAX, m - i)
        _lib.check(lib.coot_retrieval_topk_few_masked(queries[i:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), mm, n, d, k,
                                                      idx[i:].data_ptr(), scores[i:].data_ptr(), sim[i:].data_ptr() if want_sim else None,
                                                      ws.data_ptr(), ws.numel(), st), "coot_retrieval_topk_few_masked")
    return idx, scores, sim


def _topk_tile(queries, gallery, norms, k: int, keep, want_sim: bool, method=None, own_keep=None):
    """coot_retrieval_topk_index: one call for any M.  method, own_keep: name and own filter of GalleryIndex.search (many queries)."""
    from . import lib as _lib
    if keep is not None:
        assert gallery.dim() == 2, gallery.shape
        keep = _check_keep(method or "retrieval_topk_index_device", keep, gallery.shape[0])
    mirror = "compute_retrieval_topk" + ("_masked" if method is None and keep is not None else "")
    detail = None if method else (queries.dtype, queries.shape, gallery.shape)
    (queries, gallery, norms), code, (m, n, d, k) = _check_search("retrieval_topk_index_device", mirror, queries, gallery, norms, k, detail, method=method)
    keep = _and_own(own_keep, keep)
    lib = _lib.load()
    ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_index_workspace_bytes(m, n, d, k), m, n, k, want_sim, queries.device)
    _lib.check(lib.coot_retrieval_topk_index(queries.data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), m, n, d, k, idx.data_ptr(),
                                             scores.data_ptr(), _ptr(sim), ws.data_ptr(), ws.numel(), _stream()), "coot_retrieval_topk_index")
    return idx, scores, sim


def _topk_grouped(queries, gallery, norms, groups, k: int, num_groups, keep, want_sim: bool, method=None, own_keep=None):
    """coot_retrieval_topk_grouped for any M: slices of RETRIEVAL_FEW_MAX queries over one workspace.  groups is checked before keep, and
    keep names the mirror of the filtered search.  method, own_keep: the name and the own filter of GalleryIndex.search_grouped."""
    import torch
    from . import lib as _lib
    fn = "retrieval_topk_grouped_device"
    assert gallery.dim() == 2, gallery.shape
    groups = _check_groups(method or fn, groups, gallery.shape[0])
    if keep is not None:
        keep = _check_keep(method or fn, keep, gallery.shape[0])
    queries = queries[None] if queries.dim() == 1 else queries
    (queries, gallery, norms), code, (m, n, d, k) = _check_search(fn, "compute_retrieval_topk_grouped", queries, gallery, norms, k, method=method)
    g_total = int(groups.max()) + 1 if num_groups is None else int(num_groups)  # (None: the one synchronisation)
    if g_total < 1:
        raise ValueError(f"{fn}: num_groups = {g_total}; there has to be at least one group")
    keep = _and_own(own_keep, keep)
    lib = _lib.load()
    ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_grouped_workspace_bytes(min(m, RETRIEVAL_FEW_MAX), n, d, k, g_total), m, n, k, want_sim,
                                         queries.device)
    group = torch.empty_like(idx)
    st = _stream()
    for i in range(0, m, RETRIEVAL_FEW_MAX):  # the calls of a stream run in order: one workspace, its table reset by every call
        mm = min(RETRIEVAL_FEW_MAX, m - i)
        _lib.check(lib.coot_retrieval_topk_grouped(queries[i:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), groups.data_ptr(), g_total, mm,
                                                   n, d, k, group[i:].data_ptr(), idx[i:].data_ptr(), scores[i:].data_ptr(),
                                                   sim[i:].data_ptr() if want_sim else None, ws.data_ptr(), ws.numel(), st), "coot_retrieval_topk_grouped")
    return group, idx, scores, sim


def retrieval_topk_grouped_device(queries, gallery, norms, groups, k: int, num_groups=None, keep=None, want_sim: bool = False):
    """The grouped search on a gallery as a prepared index holds it (coot_retrieval_topk_grouped): queries cuda float32 [M, d], gallery
    cuda float32, bfloat16 or float16 [N, d], norms cuda float32 [N] (GalleryIndex.norms) or None: rows used as they are; groups cuda
    torch.int32 or torch.int64 [N] (int64 is converted once), groups[j] = the group of gallery row j.  Returns (group int32 [M, k], idx
    int32 [M, k], scores float32 [M, k], sim [M, N] or None) on the device: the k best groups of every query, each with its best row
    and that row's score — compute_retrieval_topk_grouped of the similarities the other searches select from, byte for byte, without
    the M x N matrix.  Rows that keep masks out and rows with a group id outside [0, num_groups) are never returned; with fewer than k
    groups left the tail is group -1, idx -1, score -inf.  1 <= k <= min(N, 128), whatever groups and keep hold.
    num_groups=None costs one synchronisation with the device (int(groups.max()) + 1): pass num_groups where it is known.  Otherwise
    nothing synchronises.  More than 16 queries run in slices of 16, one sweep of the gallery each, over one workspace."""
    return _topk_grouped(queries, gallery, norms, groups, k, num_groups, keep, want_sim)


def _check_scope(fn: str, only, exclude, m: int):
    """The scope of a scoped search, checked on the host before anything is launched: exactly one of only / exclude (ValueError), one
    id per query: a cuda torch.int32 or torch.int64 tensor [M], or ids on the host (a sequence, a numpy array or a CPU tensor of
    integers inside int32) that the caller uploads once.  Returns (the cuda tensor or an int32 numpy array, exclude as 0 / 1)."""
    import torch
    if (only is None) == (exclude is None):
        raise ValueError(f"{fn}: exactly one of only= and exclude= has to be given, not {'both' if only is not None else 'neither'}")
    scope, name = (exclude, "exclude") if only is None else (only, "only")
    if isinstance(scope, torch.Tensor) and scope.is_cuda:
        if scope.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{fn}: {name} has to hold integers (torch.int32 or torch.int64 on the device), not {scope.dtype}")
        shape = tuple(scope.shape)
    else:
        try:
            scope = np.asarray(scope.numpy() if isinstance(scope, torch.Tensor) else scope)
        except Exception:
            scope = np.asarray(None)
        if scope.dtype.kind not in "iu":
            raise ValueError(f"{fn}: {name} has to hold integers (one id per query), not dtype {scope.dtype}")
        shape = scope.shape
    if shape != (m,):
        raise ValueError(f"{fn}: {name} of shape {tuple(shape)}, {m} queries (one id per query: [{m}])")
    if isinstance(scope, np.ndarray):
        if scope.size and (scope.min() < -2 ** 31 or scope.max() > 2 ** 31 - 1):
            raise ValueError(f"{fn}: {name} holds an id outside int32, which no row carries")
        scope = np.ascontiguousarray(scope.astype(np.int32))
    return scope, int(only is None)


def _topk_scoped(queries, gallery, norms, groups, k: int, only, exclude, keep, want_sim: bool, method=None, own_keep=None):
    """coot_retrieval_topk_scoped for any M: slices of RETRIEVAL_FEW_MAX queries, each with its slice of the scope, over one workspace.
    Checked in this order: only / exclude, groups, keep, the scope's type and shape, then where everything lives.  method, own_keep: the
    name and the own filter of GalleryIndex.search_scoped / neighbors."""
    import torch
    from . import lib as _lib
    fn = "retrieval_topk_scoped_device"
    who = method or fn
    if (only is None) == (exclude is None):
        _check_scope(who, only, exclude, 0)
    assert gallery.dim() == 2, gallery.shape
    if groups is not None:
        groups = _check_groups(who, groups, gallery.shape[0], mirror=None)
    if keep is not None:
        keep = _check_keep(who, keep, gallery.shape[0], mirror=None)
    queries = queries[None] if queries.dim() == 1 else queries
    assert queries.dim() == 2, queries.shape
    scope, excl = _check_scope(who, only, exclude, queries.shape[0])
    (queries, gallery, norms), code, (m, n, d, k) = _check_search(fn, "compute_retrieval_topk_scoped", queries, gallery, norms, k, queries.dtype,
                                                                  also=(groups, keep), method=method)
    scope = torch.from_numpy(scope).to(queries.device) if isinstance(scope, np.ndarray) else scope.to(torch.int32).contiguous()
    keep = _and_own(own_keep, keep)
    lib = _lib.load()
    ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_scoped_workspace_bytes(min(m, RETRIEVAL_FEW_MAX), n, d, k), m, n, k, want_sim,
                                         queries.device)
    st = _stream()
    for i in range(0, m, RETRIEVAL_FEW_MAX):  # the calls of a stream run in order: one workspace
        mm = min(RETRIEVAL_FEW_MAX, m - i)
        _lib.check(lib.coot_retrieval_topk_scoped(queries[i:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), _ptr(groups),
                                                  scope[i:].data_ptr(), excl, mm, n, d, k, idx[i:].data_ptr(), scores[i:].data_ptr(),
                                                  sim[i:].data_ptr() if want_sim else None, ws.data_ptr(), ws.numel(), st), "coot_retrieval_topk_scoped")
    return idx, scores, sim


def retrieval_topk_scoped_device(queries, gallery, norms, groups, k: int, only=None, exclude=None, keep=None, want_sim: bool = False):
    """The scoped search on a gallery as a prepared index holds it (coot_retrieval_topk_scoped): every query has its own slice of the
    gallery.  queries cuda float32 [M, d], gallery cuda float32, bfloat16 or float16 [N, d], norms cuda float32 [N] (GalleryIndex.norms)
    or None: rows used as they are; groups cuda torch.int32 or torch.int64 [N] (int64 is converted once), groups[j] = the id of gallery
    row j, any int32 value, or None: every row is its own id (groups[j] = j).  Exactly one of only= / exclude= (both or neither:
    ValueError): one id per query, [M], a cuda torch.int32 or torch.int64 tensor, or a host sequence, numpy array or CPU tensor of
    integers, which is uploaded once.  Row j is eligible for query i when keep lets it pass and groups[j] == only[i] (within one video:
    which clip of it answers the sentence), or groups[j] != exclude[i] (everything but one video).  Returns (idx int32 [M, k], scores
    float32 [M, k], sim [M, N] or None) on the device: row i is, byte for byte, GalleryIndex.search(queries[i:i + 1], k,
    keep=eligible_i) — compute_retrieval_topk_scoped of the similarities the other searches select from, without M masks, M calls and M
    sweeps.  An id that no row carries selects nothing under only and excludes nothing under exclude; with fewer than k eligible rows
    the tail is idx -1, score -inf.  1 <= k <= min(N, 128), whatever the scopes and keep hold.  sim holds every similarity, eligible
    or not; without it, blocks of 128 rows in which no row is eligible for any query of a slice are not read.  Nothing synchronises.
    More than 16 queries run in slices of 16, one sweep of the gallery each, over one workspace."""
    return _topk_scoped(queries, gallery, norms, groups, k, only, exclude, keep, want_sim)


def _check_offset(fn: str, offset, n: int, dev):
    """The offset of an adjusted search, checked on the host before anything is launched (ValueError): a cuda torch.float32 tensor [N]
    on the gallery's device (dev), or N numbers on the host (a sequence, a numpy array or a CPU tensor).  Returns the cuda tensor, or a
    float32 numpy array [N] that the caller uploads once: a host value is rounded to float32 here, once."""
    import torch
    if isinstance(offset, torch.Tensor) and offset.is_cuda:
        if offset.dtype is not torch.float32:
            raise ValueError(f"{fn}: offset on the device has to be torch.float32, not {offset.dtype}")
        if tuple(offset.shape) != (n,):
            raise ValueError(f"{fn}: offset of shape {tuple(offset.shape)}, a gallery of {n} rows (one number per row: [{n}])")
        if offset.device != dev:
            raise ValueError(f"{fn}: offset lives on {offset.device}, the gallery on {dev}")
        return offset
    try:
        t = np.asarray(offset.numpy() if isinstance(offset, torch.Tensor) else offset)
    except Exception:
        t = np.asarray(None)
    if t.dtype.kind not in "fiu":
        raise ValueError(f"{fn}: offset has to hold one number per gallery row, not dtype {t.dtype}")
    if t.shape != (n,):
        raise ValueError(f"{fn}: offset of shape {tuple(t.shape)}, a gallery of {n} rows (one number per row: [{n}])")
    with np.errstate(over="ignore"):
        return np.array(t.astype(np.float32))  # (a copy: contiguous and writable)


# The adjusted search: from this many queries on, one tile call over all queries (coot_retrieval_topk_adjusted_tile, 64 queries per
# workgroup and read of a gallery block); below it, slices of RETRIEVAL_FEW_MAX queries through the sweep, one sweep of the gallery
# each.  ADJUSTED_TILE_MIN_M: a float32 gallery; ADJUSTED_TILE_MIN_M_16BIT: bfloat16 / float16.  Both routes return the same bytes.
# Read at call time.  ADJUSTED_TILE_NEVER: above every M, the slices always serve.
# Each is the smallest M of the measured ladder (profiles/r35_adjusted_tile.json: M = 17, 32, 64, 128, 256, 320, 512, 1 024; 200 000 x 768
# and 18 000 x 384; K = 10) from which the tile route's median stays below the slices' median by more than the slices' own spread at both
# galleries and at every larger M.  The tile walk takes 5.6 - 6.4 ms at 200 000 x 768 whatever M is up to 512, so it loses up to and
# including 256 queries there (6.37 against 6.05 +- 0.10 ms on float32, 6.37 against 6.67 +- 1.06 ms on bfloat16: inside the spread) and wins
# from 320 (6.41 against 7.49 and 6.39 against 8.59 ms); at 18 000 x 384 it already wins from 128 (0.84 against 1.10 and 1.26 ms), which
# this one threshold leaves to the slices.
ADJUSTED_TILE_NEVER = 1 << 31
ADJUSTED_TILE_MIN_M = 320
ADJUSTED_TILE_MIN_M_16BIT = 320


def _topk_adjusted(queries, gallery, norms, offset, k: int, keep, want_sim: bool, method=None, own_keep=None):
    """coot_retrieval_topk_adjusted for any M: slices of RETRIEVAL_FEW_MAX queries over one workspace; from ADJUSTED_TILE_MIN_M (float32
    gallery) / ADJUSTED_TILE_MIN_M_16BIT queries on, one call of coot_retrieval_topk_adjusted_tile instead.  Checked in this order: keep, the
    offset, then where everything lives, the widths and k.  method, own_keep: the name and the own filter of GalleryIndex.search_adjusted."""
    import torch
    from . import lib as _lib
    fn = "retrieval_topk_adjusted_device"
    who = method or fn
    assert gallery.dim() == 2, gallery.shape
    if keep is not None:
        keep = _check_keep(who, keep, gallery.shape[0], mirror=None)
    offset = _check_offset(who, offset, gallery.shape[0], gallery.device)
    queries = queries[None] if queries.dim() == 1 else queries
    (queries, gallery, norms), code, (m, n, d, k) = _check_search(fn, "compute_retrieval_topk_adjusted", queries, gallery, norms, k, queries.dtype,
                                                                  also=(keep,), method=method)
    offset = torch.from_numpy(offset).to(queries.device) if isinstance(offset, np.ndarray) else offset.contiguous()
    keep = _and_own(own_keep, keep)
    lib = _lib.load()
    st = _stream()
    if m >= (ADJUSTED_TILE_MIN_M_16BIT if code else ADJUSTED_TILE_MIN_M):  # one call, all queries
        ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_adjusted_tile_workspace_bytes(m, n, d, k), m, n, k, want_sim, queries.device)
        _lib.check(lib.coot_retrieval_topk_adjusted_tile(queries.data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), offset.data_ptr(), m, n,
                                                         d, k, idx.data_ptr(), scores.data_ptr(), _ptr(sim), ws.data_ptr(), ws.numel(), st),
                   "coot_retrieval_topk_adjusted_tile")
        return idx, scores, sim
    ws, idx, scores, sim = _topk_buffers(lib.coot_retrieval_topk_adjusted_workspace_bytes(min(m, RETRIEVAL_FEW_MAX), n, d, k), m, n, k, want_sim,
                                         queries.device)
    for i in range(0, m, RETRIEVAL_FEW_MAX):  # the calls of a stream run in order: one workspace
        mm = min(RETRIEVAL_FEW_MAX, m - i)
        _lib.check(lib.coot_retrieval_topk_adjusted(queries[i:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), offset.data_ptr(), mm, n,
                                                    d, k, idx[i:].data_ptr(), scores[i:].data_ptr(), sim[i:].data_ptr() if want_sim else None,
                                                    ws.data_ptr(), ws.numel(), st), "coot_retrieval_topk_adjusted")
    return idx, scores, sim


def retrieval_topk_adjusted_device(queries, gallery, norms, offset, k: int, keep=None, want_sim: bool = False):
    """The adjusted search on a gallery as a prepared index holds it (coot_retrieval_topk_adjusted): every gallery row brings a number
    that is taken off its similarity before the selection.  queries cuda float32 [M, d], gallery cuda float32, bfloat16 or float16
    [N, d], norms cuda float32 [N] (GalleryIndex.norms) or None: rows used as they are; offset: a cuda torch.float32 tensor [N], or N
    numbers on the host (a sequence, a numpy array or a CPU tensor), rounded to float32 once and uploaded once.  Returns (idx int32
    [M, k], scores float32 [M, k], sim [M, N] or None) on the device: the k best rows that keep lets pass by a(i, j) = s(i, j) -
    offset[j], one float32 subtraction on the similarity s the other searches select from, in their order (a descending, then the
    larger row); scores holds the bytes of a, sim (a testing aid) the raw s of every row, kept or not.
    compute_retrieval_topk_adjusted of those similarities, byte for byte; with offset = 0 the bytes of the filtered search.  A row with
    offset +inf scores -inf and is still returned, with its index, once nothing better is left (a masked row never is); -inf puts a
    row first.  With fewer than k kept rows the tail is idx -1, score -inf.  1 <= k <= min(N, 128), whatever keep holds.  Without
    sim, blocks of 128 rows in which keep leaves no row are not read.  Nothing synchronises.  More than 16 queries run in slices of
    16, one sweep of the gallery each, over one workspace; from ADJUSTED_TILE_MIN_M (float32 gallery) / ADJUSTED_TILE_MIN_M_16BIT
    queries on, one call of coot_retrieval_topk_adjusted_tile serves them all, with the same bytes."""
    return _topk_adjusted(queries, gallery, norms, offset, k, keep, want_sim)


RETRIEVAL_RANGE_BLOCK = 128  # include/coot_hip.h: COOT_RETRIEVAL_RANGE_BLOCK

# The range search: from this many queries on, one tile call per pass over all queries (coot_retrieval_range_tile_count / _fill, 64
# queries per workgroup and read of a gallery block); below it, slices of RETRIEVAL_FEW_MAX queries through the sweep, two sweeps of the
# gallery each.  RANGE_TILE_MIN_M: a float32 gallery; RANGE_TILE_MIN_M_16BIT: bfloat16 / float16.  Both routes return the same bytes;
# up to RETRIEVAL_FEW_MAX queries the sweep always serves.  Read at call time.
# Each is the smallest M of the measured ladder (profiles/r25_range_tile.json: M = 17, 32, 64, 128, 256, 512, 1 024; 200 000 x 768 and
# 18 000 x 384; 2 rows, 0.1 % and 10 % of the gallery per query) from which the tile route's median stays below the slices' median by
# more than the slices' own spread in every case.  At 17 queries the one row tile is a quarter full: at 200 000 x 768 the tile route
# then loses on bfloat16 (0.96 against 0.84 ms at 0.1 %) and is inside the spread on float32 (0.95 against 0.99 +- 0.15 ms); at
# 18 000 x 384 it already wins at 17 (0.15 against 0.22 ms), which this one threshold leaves to the slices.
RANGE_TILE_MIN_M = 32
RANGE_TILE_MIN_M_16BIT = 32


def _check_threshold(fn: str, threshold, m: int):
    """The threshold of a range search, checked on the host before anything is launched (ValueError): a Python or numpy number (used
    for every query), M numbers on the host (a sequence, a numpy array or a CPU tensor) or a cuda torch.float32 tensor [M].  Returns
    the cuda tensor, or a float32 numpy array [M] that the caller uploads once: a host value is rounded to float32 here, once."""
    import torch
    if isinstance(threshold, torch.Tensor) and threshold.is_cuda:
        if threshold.dtype is not torch.float32:
            raise ValueError(f"{fn}: threshold on the device has to be torch.float32, not {threshold.dtype}")
        if tuple(threshold.shape) != (m,):
            raise ValueError(f"{fn}: threshold of shape {tuple(threshold.shape)}, {m} queries (one number, or one per query: [{m}])")
        return threshold
    try:
        t = np.asarray(threshold.numpy() if isinstance(threshold, torch.Tensor) else threshold)
    except Exception:
        t = np.asarray(None)
    if t.dtype.kind not in "fiu":
        raise ValueError(f"{fn}: threshold has to be a number or hold one number per query, not dtype {t.dtype}")
    if t.shape not in ((), (m,)):
        raise ValueError(f"{fn}: threshold of shape {tuple(t.shape)}, {m} queries (one number, or one per query: [{m}])")
    with np.errstate(over="ignore"):
        return np.array(np.broadcast_to(t.astype(np.float32), (m,)))  # (a copy: contiguous and writable)


def _check_range_result(fn: str, max_results, order):
    """max_results (None or an integer >= 1) and order ("row" or "score", the latter with max_results=None only), or the ValueError."""
    if order not in ("row", "score"):
        raise ValueError(f"{fn}: order = {order!r}; it has to be \"row\" or \"score\"")
    if max_results is not None and (isinstance(max_results, bool) or not isinstance(max_results, (int, np.integer)) or max_results < 1):
        raise ValueError(f"{fn}: max_results = {max_results!r}; it has to be None (the exact size, one synchronisation) or an integer >= 1")
    if order == "score" and max_results is not None:
        raise ValueError(f"{fn}: order=\"score\" needs max_results=None: a segment that was cut has no defined score order")


def _range(queries, gallery, norms, threshold, keep, max_results, order, method=None, own_keep=None, count_only: bool = False):
    """coot_retrieval_range_count / _scan / _fill for any M: slices of RETRIEVAL_FEW_MAX queries over one workspace and one table of block
    counts; from RANGE_TILE_MIN_M (float32 gallery) / RANGE_TILE_MIN_M_16BIT queries on, coot_retrieval_range_tile_count and _tile_fill
    instead, one call each over all queries on the same table, with the same scan between them.  Checked in this order: max_results and order, keep, the threshold's type and shape, then where everything lives.  method,
    own_keep: the name and the own filter of GalleryIndex.search_range / count_range; count_only: the counts after the scan, no fill."""
    import torch
    from . import lib as _lib
    fn = "retrieval_range_device"
    who = method or fn
    if not count_only:
        _check_range_result(who, max_results, order)
    assert gallery.dim() == 2, gallery.shape
    if keep is not None:
        keep = _check_keep(who, keep, gallery.shape[0], mirror=None)
    queries = queries[None] if queries.dim() == 1 else queries
    assert queries.dim() == 2, queries.shape
    thr = _check_threshold(who, threshold, queries.shape[0])
    (queries, gallery, norms), code, (m, n, d, _) = _check_search(fn, "compute_retrieval_range", queries, gallery, norms, 1, queries.dtype,
                                                                  also=(keep,), method=method)
    dev = queries.device
    if isinstance(thr, np.ndarray):
        thr = torch.from_numpy(thr).to(dev)
    elif thr.device != dev:
        raise ValueError(f"{who}: threshold lives on {thr.device}, the queries on {dev}")
    thr = thr.contiguous()
    keep = _and_own(own_keep, keep)
    lib = _lib.load()
    stride = (n + RETRIEVAL_RANGE_BLOCK - 1) // RETRIEVAL_RANGE_BLOCK + 1
    table = torch.empty(m, stride, dtype=torch.int32, device=dev)
    tile = m >= (RANGE_TILE_MIN_M_16BIT if code else RANGE_TILE_MIN_M)
    st = _stream()
    if tile:  # one call per pass, all queries
        ws = torch.empty(lib.coot_retrieval_range_tile_workspace_bytes(m, n, d), dtype=torch.uint8, device=dev)
        slices = []
        _lib.check(lib.coot_retrieval_range_tile_count(queries.data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), thr.data_ptr(), m, n, d,
                                                       table.data_ptr(), ws.data_ptr(), ws.numel(), st), "coot_retrieval_range_tile_count")
    else:
        ws = torch.empty(lib.coot_retrieval_range_workspace_bytes(min(m, RETRIEVAL_FEW_MAX), n, d), dtype=torch.uint8, device=dev)
        slices = [(i, min(RETRIEVAL_FEW_MAX, m - i)) for i in range(0, m, RETRIEVAL_FEW_MAX)]  # the calls of a stream run in order: one workspace
    for i, mm in slices:
        _lib.check(lib.coot_retrieval_range_count(queries[i:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), thr[i:].data_ptr(), mm, n, d,
                                                  table[i:].data_ptr(), ws.data_ptr(), ws.numel(), st), "coot_retrieval_range_count")
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    offsets = None if count_only else torch.empty(m + 1, dtype=torch.int64, device=dev)
    _lib.check(lib.coot_retrieval_range_scan(table.data_ptr(), m, n, _ptr(offsets), counts.data_ptr(), st), "coot_retrieval_range_scan")
    if count_only:
        return counts
    if max_results is None:
        cap = int(offsets[m])  # (the one synchronisation)
        rows = torch.empty(cap, dtype=torch.int32, device=dev)
        scores = torch.empty(cap, dtype=torch.float32, device=dev)
        if cap == 0:
            return offsets, rows, scores
    else:
        cap = int(max_results)
        rows = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        scores = torch.full((cap,), float("-inf"), dtype=torch.float32, device=dev)
    if tile:
        _lib.check(lib.coot_retrieval_range_tile_fill(queries.data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), thr.data_ptr(), m, n, d,
                                                      table.data_ptr(), offsets.data_ptr(), cap, rows.data_ptr(), scores.data_ptr(), ws.data_ptr(),
                                                      ws.numel(), st), "coot_retrieval_range_tile_fill")
    for i, mm in slices:
        _lib.check(lib.coot_retrieval_range_fill(queries[i:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), thr[i:].data_ptr(), mm, n, d,
                                                 table[i:].data_ptr(), offsets[i:].data_ptr(), cap, rows.data_ptr(), scores.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), st), "coot_retrieval_range_fill")
    if order == "score":
        # the searches' order inside every segment: score descending with -0 as +0, then the larger row.  Stable sorts: reversed, the
        # rows of a segment descend; then by score; then by segment, which keeps both.
        seg = torch.repeat_interleave(torch.arange(m, device=dev), counts.long(), output_size=cap)
        perm = torch.arange(cap - 1, -1, -1, device=dev)
        perm = perm[torch.sort(scores[perm] + 0.0, descending=True, stable=True)[1]]
        perm = perm[torch.sort(seg[perm], stable=True)[1]]
        rows, scores = rows[perm], scores[perm]
    return offsets, rows, scores


def retrieval_range_device(queries, gallery, norms, threshold, keep=None, max_results=None, order: str = "row"):
    """The range search on a gallery as a prepared index holds it (coot_retrieval_range_count, _scan, _fill): every gallery row that
    scores at least a query's threshold, however many there are.  queries cuda float32 [M, d], gallery cuda float32, bfloat16 or
    float16 [N, d], norms cuda float32 [N] (GalleryIndex.norms) or None: rows used as they are.  threshold: a Python number (for every
    query), M numbers on the host (a sequence, a numpy array or a CPU tensor; uploaded once) or a cuda torch.float32 tensor [M]; a host
    value is rounded to float32 once.  Row j is a hit of query i when keep lets it pass and s(i, j) >= threshold[i] in float32, s being
    the similarity the searches rank on, bit for bit (sim of GalleryIndex.search(..., want_sim=True)): a NaN score or threshold is no
    hit, -0 >= +0 holds, -inf returns every kept row whose score is not a NaN, +inf only rows that score +inf.
    Returns (offsets int64 [M + 1], rows int32 [T], scores float32 [T]) on the device, CSR: the hits of query i are
    rows[offsets[i]:offsets[i + 1]], in ascending row order, with their scores — compute_retrieval_range of the similarities, byte for
    byte, whatever the batch-mates of a query, the storage type and the schedule are; no M x N matrix and no top-K cap of 128.
    max_results=None: T = offsets[M] is read back, the one synchronisation, and rows / scores have exactly T entries.  max_results=c >=
    1: nothing synchronises; rows / scores have c entries, the first min(T, c) of the result and then -1 / -inf; offsets is exact
    either way, so offsets[M] > c says that, and where, the result was cut.  order="score" (max_results=None only: ValueError
    otherwise) puts every segment into the searches' order, score descending with -0 as +0, then the larger row, with torch sorts on
    the device.  More than 16 queries run in slices of 16 over one workspace: per slice one sweep of the gallery that counts, and one
    that reads only the blocks of 128 rows in which a query of the slice has a hit.  From RANGE_TILE_MIN_M queries on a float32 gallery
    and RANGE_TILE_MIN_M_16BIT on a 16-bit one (module constants, read at call time) the route changes to two tile calls over all
    queries, 64 queries per read of a block; the bytes of the result do not."""
    return _range(queries, gallery, norms, threshold, keep, max_results, order)


# The self-join works through the gallery in chunks of rows; the table of block counts of one chunk (int32, rows x (blocks at or right
# of the chunk's first block + 1)) holds at most this many bytes.  A chunk starts at a multiple of RETRIEVAL_RANGE_BLOCK rows and holds
# at least that many, whatever the budget.  The result's bytes do not depend on it.  Read at call time.
JOIN_TABLE_BYTES = 1 << 28
_JOIN_ROWS_MAX = 65535 * 64 // RETRIEVAL_RANGE_BLOCK * RETRIEVAL_RANGE_BLOCK  # coot_retrieval_join_count: ceil(rows / 64) <= 65 535


def _join_chunks(n: int, budget: int):
    """The chunks [(row0, rows)] of a self-join of n rows under a table budget in bytes: row0 a multiple of 128, in order and covering
    [0, n) once; as many rows as the chunk's table, rows x (ceil((n - row0) / 128) + 1) int32, fits the budget, in multiples of 128
    and at least 128 (the last chunk: what is left).  Later chunks have narrower tables, so they are longer."""
    blk = RETRIEVAL_RANGE_BLOCK
    chunks, row0 = [], 0
    while row0 < n:
        stride = (n - row0 + blk - 1) // blk + 1
        rows = min(max(blk, int(budget) // (4 * stride) // blk * blk), _JOIN_ROWS_MAX, n - row0)
        chunks.append((row0, rows))
        row0 += rows
    return chunks


def _self_join(gallery, norms, threshold, keep, groups, max_results, method=None, own_keep=None, count_only: bool = False):
    """coot_retrieval_join_count / coot_retrieval_range_scan / coot_retrieval_join_fill per chunk of _join_chunks.  Checked in this
    order: max_results, groups, keep, the threshold's type and shape, then where everything lives.  method, own_keep: the name and the
    own filter of GalleryIndex.self_join / count_self_join; count_only: the counts after the scans, no fill."""
    import torch
    from . import lib as _lib
    fn = "retrieval_self_join_device"
    who = method or fn
    if not count_only:
        _check_range_result(who, max_results, "row")
    assert gallery.dim() == 2, gallery.shape
    n, d = gallery.shape
    if groups is not None:
        groups = _check_groups(who, groups, n, mirror=None)
    if keep is not None:
        keep = _check_keep(who, keep, n, mirror=None)
    thr = _check_threshold(who, threshold, n)
    _on_device(who, "compute_retrieval_self_join", gallery, norms, keep, groups)
    code = _gallery_code(fn, gallery)
    assert norms is None or (norms.dtype == torch.float32 and tuple(norms.shape) == (n,)), (norms.dtype, norms.shape, n)
    gallery, norms, dev = gallery.contiguous(), None if norms is None else norms.contiguous(), gallery.device
    if isinstance(thr, np.ndarray):
        thr = torch.from_numpy(thr).to(dev)
    elif thr.device != dev:
        raise ValueError(f"{who}: threshold lives on {thr.device}, the gallery on {dev}")
    thr = thr.contiguous()
    keep = _and_own(own_keep, keep)
    lib, st, blk = _lib.load(), _stream(), RETRIEVAL_RANGE_BLOCK
    chunks = _join_chunks(n, JOIN_TABLE_BYTES)
    table = torch.empty(max(r * ((n - r0 + blk - 1) // blk + 1) for r0, r in chunks), dtype=torch.int32, device=dev)  # the calls of a stream run in order: one table
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    offsets = None if count_only else torch.empty(n + 1, dtype=torch.int64, device=dev)
    if max_results is not None:
        cap = int(max_results)
        rows_out = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        scores_out = torch.full((cap,), float("-inf"), dtype=torch.float32, device=dev)
    total, parts = 0, []
    for row0, rows in chunks:
        _lib.check(lib.coot_retrieval_join_count(gallery.data_ptr(), code, _ptr(norms), _ptr(keep), _ptr(groups), thr.data_ptr(), row0, rows, n, d,
                                                 table.data_ptr(), st), "coot_retrieval_join_count")
        # the first chunk's offsets are the result's; a later chunk's start at 0 and are shifted by what the chunks before it hold
        off = None if count_only else offsets if row0 == 0 else torch.empty(rows + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.coot_retrieval_range_scan(table.data_ptr(), rows, n - row0, _ptr(off), counts[row0:].data_ptr(), st), "coot_retrieval_range_scan")
        if count_only:
            continue
        if max_results is None:
            cap = int(off[rows])  # (the synchronisation of this chunk)
            rows_out = torch.empty(cap, dtype=torch.int32, device=dev)
            scores_out = torch.empty(cap, dtype=torch.float32, device=dev)
            parts.append((rows_out, scores_out))
            if row0:
                torch.add(off[1:], total, out=offsets[row0 + 1:row0 + rows + 1])
            total += cap
        elif row0:  # on the device: the running total is offsets[row0]
            torch.add(off[1:], offsets[row0], out=offsets[row0 + 1:row0 + rows + 1])
            off = offsets[row0:]
        if cap:
            _lib.check(lib.coot_retrieval_join_fill(gallery.data_ptr(), code, _ptr(norms), _ptr(keep), _ptr(groups), thr.data_ptr(), row0, rows, n, d,
                                                    table.data_ptr(), off.data_ptr(), cap, rows_out.data_ptr(), scores_out.data_ptr(), st),
                       "coot_retrieval_join_fill")
    if count_only:
        return counts
    if max_results is None and len(parts) > 1:
        rows_out, scores_out = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    return offsets, rows_out, scores_out


def retrieval_self_join_device(gallery, norms, threshold, keep=None, groups=None, max_results=None):
    """The self-join of a gallery as a prepared index holds it (coot_retrieval_join_count, coot_retrieval_range_scan,
    coot_retrieval_join_fill): all pairs of rows at or above a threshold.  gallery cuda float32, bfloat16 or float16 [N, d], norms cuda
    float32 [N] (GalleryIndex.norms) or None: rows used as they are.  threshold: a Python number, N numbers on the host or a cuda
    torch.float32 tensor [N], as in retrieval_range_device; keep: cuda torch.bool or torch.uint8 [N]; groups: cuda torch.int32 or
    torch.int64 [N] (int64 is converted once) or None.  Pair (i, j), i < j, is a hit when keep lets BOTH rows pass, groups is None or
    groups[i] != groups[j], and s(i, j) >= threshold[i] in float32, s being the similarity the searches rank on with row i, widened
    to float32, as the query.  Returns (offsets int64 [N + 1], rows int32 [T], scores float32 [T]) on the device: the CSR of
    retrieval_range_device read as pairs — see GalleryIndex.self_join."""
    return _self_join(gallery, norms, threshold, keep, groups, max_results)


COMPONENTS_ROWS_MAX = 65535 * 64  # coot_retrieval_components: one launch covers all rows, ceil(N / 64) <= 65 535


def _components(gallery, norms, threshold, keep, groups, method=None, own_keep=None):
    """One call of coot_retrieval_components.  Checked in this order: the number of rows, then as _self_join: groups, keep, the
    threshold's type and shape, then where everything lives.  method, own_keep: the name and the own filter of
    GalleryIndex.components / deduplicate."""
    import torch
    from . import lib as _lib
    fn = "retrieval_components_device"
    who = method or fn
    assert gallery.dim() == 2, gallery.shape
    n, d = gallery.shape
    if n > COMPONENTS_ROWS_MAX:
        raise ValueError(f"{who}: a gallery of {n} rows; one launch covers all rows, at most {COMPONENTS_ROWS_MAX} (ceil(N / 64) <= 65535)")
    if groups is not None:
        groups = _check_groups(who, groups, n, mirror=None)
    if keep is not None:
        keep = _check_keep(who, keep, n, mirror=None)
    thr = _check_threshold(who, threshold, n)
    _on_device(who, "compute_retrieval_components", gallery, norms, keep, groups)
    code = _gallery_code(fn, gallery)
    assert norms is None or (norms.dtype == torch.float32 and tuple(norms.shape) == (n,)), (norms.dtype, norms.shape, n)
    gallery, norms, dev = gallery.contiguous(), None if norms is None else norms.contiguous(), gallery.device
    if isinstance(thr, np.ndarray):
        thr = torch.from_numpy(thr).to(dev)
    elif thr.device != dev:
        raise ValueError(f"{who}: threshold lives on {thr.device}, the gallery on {dev}")
    thr = thr.contiguous()
    keep = _and_own(own_keep, keep)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().coot_retrieval_components(gallery.data_ptr(), code, _ptr(norms), _ptr(keep), _ptr(groups), thr.data_ptr(), n, d,
                                                     parent.data_ptr(), labels.data_ptr(), _stream()), "coot_retrieval_components")
    return labels


def retrieval_components_device(gallery, norms, threshold, keep=None, groups=None):
    """The connected components of a gallery, as a prepared index holds it, under the pairs of retrieval_self_join_device with the
    same arguments (coot_retrieval_components): labels int32 [N] on the device, no synchronisation.  gallery cuda float32, bfloat16 or
    float16 [N, d], N <= COMPONENTS_ROWS_MAX, norms cuda float32 [N] (GalleryIndex.norms) or None: rows used as they are; threshold,
    keep and groups as in retrieval_self_join_device.  labels[i] is the smallest row of row i's component, i itself without an edge,
    -1 where keep masks the row — see GalleryIndex.components."""
    return _components(gallery, norms, threshold, keep, groups)


_CROSS_JOIN_TILE = 64  # coot_retrieval_cross_join_count: the row tile; a chunk of left rows starts at a multiple of it
_CROSS_JOIN_ROWS_MAX = 65535 * _CROSS_JOIN_TILE  # ceil(rows / 64) <= 65 535


def _cross_join_chunks(n_left: int, n_right: int, budget: int):
    """The chunks [(row0, rows)] of left rows of a join of n_left rows with n_right rows under a table budget in bytes: row0 a
    multiple of 64, in order and covering [0, n_left) once; as many rows as the chunk's table, rows x (ceil(n_right / 128) + 1) int32,
    fits the budget, in multiples of 64 and at least 64 (the last chunk: what is left).  Every chunk's table has the same width."""
    tile = _CROSS_JOIN_TILE
    stride = (n_right + RETRIEVAL_RANGE_BLOCK - 1) // RETRIEVAL_RANGE_BLOCK + 1
    per = min(max(tile, int(budget) // (4 * stride) // tile * tile), _CROSS_JOIN_ROWS_MAX)
    return [(row0, min(per, n_left - row0)) for row0 in range(0, n_left, per)]


def _cross_join(left, left_norms, right, right_norms, threshold, keep, other_keep, groups, other_groups, max_results, method=None,
                own_keep=None, other_own_keep=None, count_only: bool = False):
    """coot_retrieval_cross_join_count / coot_retrieval_range_scan / coot_retrieval_cross_join_fill per chunk of _cross_join_chunks.
    Checked in this order: max_results, the widths, both norms or none, one device for both sides, groups, keep, the threshold's
    type and shape, then where everything lives.  method, own_keep, other_own_keep: the name and the own filters of GalleryIndex.join / count_join; count_only:
    the counts after the scans, no fill."""
    import torch
    from . import lib as _lib
    fn = "retrieval_join_device"
    who = method or fn
    if not count_only:
        _check_range_result(who, max_results, "row")
    assert left.dim() == 2 and right.dim() == 2, (left.shape, right.shape)
    (nl, d), nr = left.shape, right.shape[0]
    if right.shape[1] != d:
        raise ValueError(f"{who}: left rows of width {d}, right rows of width {right.shape[1]}")
    if (left_norms is None) != (right_norms is None):
        raise ValueError(f"{who}: one side brings row norms and the other does not (one similarity needs both norms or none)")
    if right.device != left.device:
        raise ValueError(f"{who}: the right rows live on {right.device}, the left rows on {left.device}")
    if (groups is None) != (other_groups is None):
        raise ValueError(f"{who}: groups and other_groups are given together or not at all (ids of one space, compared by inequality)")
    if groups is not None:
        groups = _check_groups(who, groups, nl, mirror=None)
        other_groups = _check_groups(who, other_groups, nr, mirror=None)
    if keep is not None:
        keep = _check_keep(who, keep, nl, mirror=None)
    if other_keep is not None:
        other_keep = _check_keep(who, other_keep, nr, mirror=None)
    thr = _check_threshold(who, threshold, nl)
    _on_device(who, "compute_retrieval_join", left, left_norms, right, right_norms, keep, other_keep, groups, other_groups)
    dev = left.device
    for name, t in (("the right norms", right_norms), ("keep", keep), ("other_keep", other_keep), ("groups", groups),
                    ("other_groups", other_groups), ("the left norms", left_norms)):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: {name} live on {t.device}, the left rows on {dev}")
    lcode, rcode = _gallery_code(fn, left), _gallery_code(fn, right)
    for norms, n in ((left_norms, nl), (right_norms, nr)):
        assert norms is None or (norms.dtype == torch.float32 and tuple(norms.shape) == (n,)), (norms.dtype, norms.shape, n)
    left, right = left.contiguous(), right.contiguous()
    if left_norms is not None:
        left_norms, right_norms = left_norms.contiguous(), right_norms.contiguous()
    if isinstance(thr, np.ndarray):
        thr = torch.from_numpy(thr).to(dev)
    elif thr.device != dev:
        raise ValueError(f"{who}: threshold lives on {thr.device}, the left rows on {dev}")
    thr = thr.contiguous()
    keep, other_keep = _and_own(own_keep, keep), _and_own(other_own_keep, other_keep)
    lib, st = _lib.load(), _stream()
    stride = (nr + RETRIEVAL_RANGE_BLOCK - 1) // RETRIEVAL_RANGE_BLOCK + 1
    chunks = _cross_join_chunks(nl, nr, JOIN_TABLE_BYTES)
    table = torch.empty(max(r for _, r in chunks) * stride, dtype=torch.int32, device=dev)  # the calls of a stream run in order: one table
    counts = torch.empty(nl, dtype=torch.int32, device=dev)
    offsets = None if count_only else torch.empty(nl + 1, dtype=torch.int64, device=dev)
    if max_results is not None:
        cap = int(max_results)
        rows_out = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        scores_out = torch.full((cap,), float("-inf"), dtype=torch.float32, device=dev)
    head = (left.data_ptr(), lcode, _ptr(left_norms), right.data_ptr(), rcode, _ptr(right_norms), _ptr(keep), _ptr(other_keep), _ptr(groups),
            _ptr(other_groups), thr.data_ptr())
    total, parts = 0, []
    for row0, rows in chunks:
        _lib.check(lib.coot_retrieval_cross_join_count(*head, row0, rows, nl, nr, d, table.data_ptr(), st), "coot_retrieval_cross_join_count")
        # the first chunk's offsets are the result's; a later chunk's start at 0 and are shifted by what the chunks before it hold
        off = None if count_only else offsets if row0 == 0 else torch.empty(rows + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.coot_retrieval_range_scan(table.data_ptr(), rows, nr, _ptr(off), counts[row0:].data_ptr(), st), "coot_retrieval_range_scan")
        if count_only:
            continue
        if max_results is None:
            cap = int(off[rows])  # (the synchronisation of this chunk)
            rows_out = torch.empty(cap, dtype=torch.int32, device=dev)
            scores_out = torch.empty(cap, dtype=torch.float32, device=dev)
            parts.append((rows_out, scores_out))
            if row0:
                torch.add(off[1:], total, out=offsets[row0 + 1:row0 + rows + 1])
            total += cap
        elif row0:  # on the device: the running total is offsets[row0]
            torch.add(off[1:], offsets[row0], out=offsets[row0 + 1:row0 + rows + 1])
            off = offsets[row0:]
        if cap:
            _lib.check(lib.coot_retrieval_cross_join_fill(*head, row0, rows, nl, nr, d, table.data_ptr(), off.data_ptr(), cap, rows_out.data_ptr(),
                                                          scores_out.data_ptr(), st), "coot_retrieval_cross_join_fill")
    if count_only:
        return counts
    if max_results is None and len(parts) > 1:
        rows_out, scores_out = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    return offsets, rows_out, scores_out


def retrieval_join_device(left_gallery, left_norms, right_gallery, right_norms, threshold, keep=None, other_keep=None, groups=None,
                          other_groups=None, max_results=None):
    """The join of two galleries as prepared indexes hold them (coot_retrieval_cross_join_count, coot_retrieval_range_scan,
    coot_retrieval_cross_join_fill): all pairs (left row, right row) at or above the left row's threshold.  left_gallery [N_left, d],
    right_gallery [N_right, d]: cuda float32, bfloat16 or float16, each its own; left_norms / right_norms: cuda float32 [N_left] /
    [N_right] (GalleryIndex.norms), or both None: rows used as they are (one without the other is a ValueError).  threshold: a
    Python number, N_left numbers on the host or a cuda torch.float32 tensor [N_left], as in retrieval_range_device; keep /
    other_keep: cuda torch.bool or torch.uint8 [N_left] / [N_right]; groups / other_groups: cuda torch.int32 or torch.int64 [N_left]
    / [N_right] (int64 is converted once), both or neither.  Pair (i, j) is a hit when keep lets left row i pass, other_keep right
    row j, the groups are None or groups[i] != other_groups[j], and s(i, j) >= threshold[i] in float32, s being the similarity the
    searches rank on with left row i, widened to float32, as the query.  Returns (offsets int64 [N_left + 1], rows int32 [T], scores
    float32 [T]) on the device: the CSR of retrieval_range_device read as pairs — see GalleryIndex.join."""
    return _cross_join(left_gallery, left_norms, right_gallery, right_norms, threshold, keep, other_keep, groups, other_groups, max_results)


KNN_JOIN_ROWS_MAX = 65535 * 64  # coot_retrieval_knn_join: ceil(N_left / 64) <= 65 535


def _knn_join(left, left_norms, right, right_norms, k: int, keep, other_keep, groups, other_groups, exclude_same_row: bool, method=None,
              own_keep=None, other_own_keep=None):
    """coot_retrieval_knn_join: one call for any N_left.  Checked in this order: the widths, both norms or none, one device for both
    sides, groups, keep, k, N_left, then where everything lives.  method, own_keep, other_own_keep: the name and the own filters of
    GalleryIndex.knn_join / knn_graph."""
    import torch
    from . import lib as _lib
    fn = "retrieval_knn_join_device"
    who = method or fn
    assert left.dim() == 2 and right.dim() == 2, (left.shape, right.shape)
    (nl, d), nr, k = left.shape, right.shape[0], int(k)
    if right.shape[1] != d:
        raise ValueError(f"{who}: left rows of width {d}, right rows of width {right.shape[1]}")
    if (left_norms is None) != (right_norms is None):
        raise ValueError(f"{who}: one side brings row norms and the other does not (one similarity needs both norms or none)")
    if right.device != left.device:
        raise ValueError(f"{who}: the right rows live on {right.device}, the left rows on {left.device}")
    if (groups is None) != (other_groups is None):
        raise ValueError(f"{who}: groups and other_groups are given together or not at all (ids of one space, compared by inequality)")
    if groups is not None:
        same = other_groups is groups and nr == nl  # (knn_graph: one table, converted once)
        groups = _check_groups(who, groups, nl, mirror=None)
        other_groups = groups if same else _check_groups(who, other_groups, nr, mirror=None)
    if keep is not None:
        keep = _check_keep(who, keep, nl, mirror=None)
    if other_keep is not None:
        other_keep = _check_keep(who, other_keep, nr, mirror=None)
    if not 1 <= k <= min(nr, 128):
        raise ValueError(f"{who}: k = {k} is outside 1 .. min(N_right = {nr}, 128)")
    if not 1 <= nl <= KNN_JOIN_ROWS_MAX:
        raise ValueError(f"{who}: {nl} left rows; one call takes 1 .. {KNN_JOIN_ROWS_MAX}")
    _on_device(who, "compute_retrieval_knn_join", left, left_norms, right, right_norms, keep, other_keep, groups, other_groups)
    dev = left.device
    for name, t in (("the right norms", right_norms), ("keep", keep), ("other_keep", other_keep), ("groups", groups),
                    ("other_groups", other_groups), ("the left norms", left_norms)):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: {name} live on {t.device}, the left rows on {dev}")
    lcode, rcode = _gallery_code(fn, left), _gallery_code(fn, right)
    for norms, n in ((left_norms, nl), (right_norms, nr)):
        assert norms is None or (norms.dtype == torch.float32 and tuple(norms.shape) == (n,)), (norms.dtype, norms.shape, n)
    left, right = left.contiguous(), right.contiguous()
    if left_norms is not None:
        left_norms, right_norms = left_norms.contiguous(), right_norms.contiguous()
    keep, other_keep = _and_own(own_keep, keep), _and_own(other_own_keep, other_keep)
    lib = _lib.load()
    ws = torch.empty(lib.coot_retrieval_knn_join_workspace_bytes(nl, nr, k), dtype=torch.uint8, device=dev)
    idx = torch.empty(nl, k, dtype=torch.int32, device=dev)
    scores = torch.empty(nl, k, dtype=torch.float32, device=dev)
    _lib.check(lib.coot_retrieval_knn_join(left.data_ptr(), lcode, _ptr(left_norms), right.data_ptr(), rcode, _ptr(right_norms), _ptr(keep),
                                           _ptr(other_keep), _ptr(groups), _ptr(other_groups), int(bool(exclude_same_row)), nl, nr, d, k,
                                           idx.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "coot_retrieval_knn_join")
    return idx, scores


def retrieval_knn_join_device(left_gallery, left_norms, right_gallery, right_norms, k: int, keep=None, other_keep=None, groups=None,
                              other_groups=None, exclude_same_row: bool = False):
    """The k best partners of every left row among the right rows, on galleries as prepared indexes hold them
    (coot_retrieval_knn_join).  left_gallery [N_left, d], right_gallery [N_right, d]: cuda float32, bfloat16 or float16, each its own;
    left_norms / right_norms: cuda float32 [N_left] / [N_right] (GalleryIndex.norms), or both None: rows used as they are (one without
    the other is a ValueError).  keep / other_keep: cuda torch.bool or torch.uint8 [N_left] / [N_right]; groups / other_groups: cuda
    torch.int32 or torch.int64 [N_left] / [N_right] (int64 is converted once), both or neither.  Pair (i, j) is eligible when keep lets
    left row i pass, other_keep right row j, the groups are None or groups[i] != other_groups[j], and, with exclude_same_row, j != i
    (left and right the same rows: a row is not its own neighbour).  Returns (idx int32 [N_left, k], scores float32 [N_left, k]) on the
    device, nothing synchronises: row i holds the k best eligible right rows, score descending, then the larger row, with the bytes of
    the similarity the searches rank on with left row i, widened to float32, as the query; fewer than k eligible rows leave a tail of
    -1 / -inf, and a left row that keep masks is -1 / -inf throughout.  compute_retrieval_knn_join of those similarities, byte for
    byte.  1 <= k <= min(N_right, 128), whatever the filters hold; N_left <= KNN_JOIN_ROWS_MAX — see GalleryIndex.knn_join."""
    return _knn_join(left_gallery, left_norms, right_gallery, right_norms, k, keep, other_keep, groups, other_groups, exclude_same_row)


# retrieval_topk_multi_device: the table best [M][G] of one library call holds at most this many entries (2^25 x 8 bytes = 256 MiB); a
# larger search runs as several calls, split where a paragraph ends, over one workspace.  One paragraph is never split: its own table
# may reach the library's bound.
MULTI_TABLE_ENTRIES = 1 << 25
MULTI_TABLE_ENTRIES_MAX = 1 << 28  # coot_retrieval_topk_multi: M x num_groups of one call
MULTI_PARAGRAPHS_MAX = 65535       # coot_retrieval_topk_multi: P of one call


def _multi_calls(off: np.ndarray, g_total: int):
    """The paragraphs [p0, p1) of each library call: as many as fit the table budget and the paragraph bound, at least one."""
    calls, p0, p_total = [], 0, len(off) - 1
    while p0 < p_total:
        p1 = p0 + 1
        while p1 < p_total and p1 - p0 < MULTI_PARAGRAPHS_MAX and (off[p1 + 1] - off[p0]) * g_total <= MULTI_TABLE_ENTRIES:
            p1 += 1
        calls.append((p0, p1))
        p0 = p1
    return calls


def retrieval_topk_multi_device(queries, offsets, gallery, norms, groups, k: int, num_groups=None, keep=None, want_sim: bool = False):
    """The multi-vector search on a gallery as a prepared index holds it (coot_retrieval_topk_multi): queries cuda float32 [M, d], the
    sentences of P paragraphs concatenated; offsets: P + 1 integers ON THE HOST (a sequence, a numpy array or a CPU integer tensor), 0 =
    offsets[0] <= ... <= offsets[P] = M, paragraph p = queries[offsets[p]:offsets[p + 1]], possibly empty; gallery, norms, groups,
    num_groups and keep as in retrieval_topk_grouped_device.  Returns (group int32 [P, k], scores float32 [P, k], rows int32 [M, k],
    row_scores float32 [M, k], sim [M, N] or None) on the device: the k best groups of every paragraph, a group's score the sum over
    the paragraph's sentences, in order, of the sentence's best row in the group, ties to the larger group id; and for every sentence
    the row that answered it in each of its paragraph's groups, with that row's score — compute_retrieval_topk_multi of the
    similarities the other searches select from, byte for byte, without the M x N matrix.  A group in which some sentence of the
    paragraph has no row left (keep, ids outside [0, num_groups)) is not returned; the tail is -1 / -inf, all of an empty paragraph's
    slots.  1 <= k <= min(N, 128), whatever groups and keep hold.
    offsets is checked here (ValueError) and uploaded, one small copy.  num_groups=None costs one synchronisation with the device
    (int(groups.max()) + 1): pass num_groups where it is known.  Every 16 sentences are one sweep of the gallery into a table of M x
    num_groups entries of 8 bytes; above MULTI_TABLE_ENTRIES entries the search runs as several library calls, split where a paragraph
    ends (paragraphs are independent: the same bytes), and one paragraph above 2^28 entries is refused."""
    return _topk_multi(queries, offsets, gallery, norms, groups, k, num_groups, keep, want_sim)


def _topk_multi(queries, offsets, gallery, norms, groups, k: int, num_groups, keep, want_sim: bool, method=None, own_keep=None):
    """coot_retrieval_topk_multi: the calls _multi_calls cuts, over one workspace.  method, own_keep: those of GalleryIndex.search_multi."""
    import torch
    from . import lib as _lib
    fn = "retrieval_topk_multi_device"
    assert gallery.dim() == 2, gallery.shape
    groups = _check_groups(method or fn, groups, gallery.shape[0], mirror=None)  # types and shapes of all three first, then where they live
    if keep is not None:
        keep = _check_keep(method or fn, keep, gallery.shape[0], mirror=None)
    assert queries.dim() == 2, queries.shape
    off = _host_offsets(method or fn, offsets, queries.shape[0])
    (queries, gallery, norms), code, (m, n, d, k) = _check_search(fn, "compute_retrieval_topk_multi", queries, gallery, norms, k, queries.dtype,
                                                                  also=(groups, keep), method=method)
    g_total = int(groups.max()) + 1 if num_groups is None else int(num_groups)  # (None: the one synchronisation)
    if g_total < 1:
        raise ValueError(f"{fn}: num_groups = {g_total}; there has to be at least one group")
    longest = int(np.diff(off).max())
    if longest * g_total > MULTI_TABLE_ENTRIES_MAX:
        raise ValueError(f"{fn}: a paragraph of {longest} sentences against {g_total} groups is a table of {longest * g_total} entries; "
                         f"one paragraph has at most 2^28")
    keep = _and_own(own_keep, keep)
    dev, p_total = queries.device, len(off) - 1
    group = torch.empty(p_total, k, dtype=torch.int32, device=dev)
    scores = torch.empty(p_total, k, dtype=torch.float32, device=dev)
    rows = torch.empty(m, k, dtype=torch.int32, device=dev)
    row_scores = torch.empty(m, k, dtype=torch.float32, device=dev)
    sim = torch.empty(m, n, dtype=torch.float32, device=dev) if want_sim else None
    lib = _lib.load()
    calls = _multi_calls(off, g_total)
    # every call's offsets from its own first sentence, one after the other in one upload
    rebased = np.concatenate([off[p0:p1 + 1] - off[p0] for p0, p1 in calls]).astype(np.int32)
    dev_off = torch.from_numpy(rebased).to(dev)
    ws = torch.empty(max(lib.coot_retrieval_topk_multi_workspace_bytes(p1 - p0, int(off[p1] - off[p0]), n, d, k, g_total) for p0, p1 in calls),
                     dtype=torch.uint8, device=dev)
    st = _stream()
    nxt = 0
    for p0, p1 in calls:  # the calls of a stream run in order: one workspace, its table reset by every call
        i0, mm = int(off[p0]), int(off[p1] - off[p0])
        at, nxt = nxt, nxt + p1 - p0 + 1
        if mm == 0:  # nothing but empty paragraphs (behind a paragraph that fills a call): no sentence, no table, every slot the tail
            group[p0:p1] = -1
            scores[p0:p1] = float("-inf")
            continue
        _lib.check(lib.coot_retrieval_topk_multi(queries[i0:].data_ptr(), gallery.data_ptr(), code, _ptr(norms), _ptr(keep), groups.data_ptr(), g_total,
                                                 dev_off[at:].data_ptr(), p1 - p0, mm, n, d, k, group[p0:].data_ptr(), scores[p0:].data_ptr(),
                                                 rows[i0:].data_ptr(), row_scores[i0:].data_ptr(), sim[i0:].data_ptr() if want_sim else None,
                                                 ws.data_ptr(), ws.numel(), st), "coot_retrieval_topk_multi")
    return group, scores, rows, row_scores, sim


def _host_rows(fn: str, rows, n: int) -> np.ndarray:
    """Row numbers given on the host (a sequence or a CPU tensor), checked: int64 [R], integers (TypeError) inside [0, n) (IndexError)."""
    r = np.asarray(rows.numpy() if hasattr(rows, "numpy") else rows).reshape(-1)
    if r.size and r.dtype.kind not in "iu":
        raise TypeError(f"GalleryIndex.{fn}: rows of dtype {r.dtype}; row numbers are integers")
    r = r.astype(np.int64)
    bad = r[(r < 0) | (r >= n)]
    if bad.size:
        raise IndexError(f"GalleryIndex.{fn}: row {int(bad[0])} is outside [0, {n})")
    return r


class GalleryIndex:
    """A gallery that stays on the device between searches: a few queries at a time, or a whole query set, against a corpus that changes
    row by row, if at all.

    GalleryIndex(gallery, normalize=True, storage=None, capacity=None): gallery is a cuda float32, bfloat16 or float16 [N, d] tensor.
    storage=None keeps the tensor's own dtype, by reference when contiguous (a copy otherwise).  storage=torch.bfloat16 or
    torch.float16 on a float32 gallery converts it once (gallery.to(storage): round to nearest even) and the float32 tensor is not
    kept: half the bytes resident, half the bytes every search reads.  storage=torch.float32 on a 16-bit tensor widens it.  Any other
    dtype or storage is a ValueError.  float16 overflows above 65 504: rows with larger entries become infinities, as .to() makes
    them, and nothing checks for it on the device, so rows that are not normalised are better kept in bfloat16.  index.storage is
    the dtype held, index.nbytes the bytes of the gallery and its norms.
    normalize=True computes the row norms once (coot_retrieval_row_norms, coot_retrieval_row_norms_h) and every search divides by
    them, as retrieval_topk_device(normalize=True) does.  The index does not watch the tensor: a caller that writes into a gallery kept
    by reference searches with stale norms; rows change through add / update (below).

    search(queries, k, want_sim=False) returns (idx int32 [M, k], scores float32 [M, k], sim [M, N] or None) on the device, no
    synchronisation: the bytes of retrieval_topk_device(queries, gallery, k, normalize=...), where gallery is the stored one widened
    to float32 — a 16-bit value widens exactly, so only the storage differs, not the arithmetic or the order.  queries are float32;
    queries [d] is one query.  1 <= k <= min(N, 128).
    M <= RETRIEVAL_FEW_MAX goes through coot_retrieval_topk_few_masked (any storage; without a filter it launches the kernels of
    coot_retrieval_topk_few / coot_retrieval_topk_few_h) with the stored norms: one sweep of the gallery, one row per thread.
    M > RETRIEVAL_FEW_MAX on a float32 index is one coot_retrieval_topk_index call (retrieval_topk_index_device): the tile search with
    the stored norms, so no pass over the gallery recomputes them.  On a 16-bit index the same call serves M >= INDEX_TILE_MIN_M_16BIT
    (the 16-bit rows are widened as they are staged; no float32 copy of the gallery is made); fewer queries go through the few-query
    call in slices of 16 (a query's result does not depend on its batch-mates): ceil(M / 16) sweeps of the gallery, which up to there
    take less time than the tile walk (measured: see the constant).

    Filtering.  search(..., keep=mask): mask is a cuda torch.bool or torch.uint8 tensor [N], nonzero = the row may be returned; the
    result is the bytes of the search on an index of gallery[mask] with its indices mapped back (compute_retrieval_topk_masked of the
    similarities), routed as above.  k is still checked against N only;
    with fewer than k rows kept, the tail of every row is idx = -1, score = -inf.  sim holds every similarity.  Without sim, blocks
    of 128 rows (64 on the tile path) that keep nothing are not read at all, so a contiguous subset costs about its share of the
    sweep and a scattered one costs the whole sweep.
    remove(rows) / restore(rows=None): a persistent filter held by the index, index.keep: None until the first remove, then a
    torch.bool [N] on the device (True = searched), written with device operations and no synchronisation.  rows is a sequence of
    ints or an int tensor; a host sequence (or CPU tensor) with a row outside [0, N) raises IndexError, a device tensor is not
    checked and its rows outside [0, N) are ignored.  restore() clears the filter.  search combines index.keep with its own keep by
    logical AND.  Removed rows still occupy memory until compact(): the gallery bytes and the norms are untouched, only the selection
    skips them.

    Offsets.  search_adjusted(queries, k, offset) ranks by the similarity minus a number per row, and hubness_offsets(bank) computes
    the numbers that correct hubness (CSLS) from a second index of representative queries: see the methods.

    Range search.  search_range(queries, threshold) returns every row at or above a query's threshold, however many, as CSR (offsets,
    rows, scores), and count_range their number: see the methods.  keep and the index's own filter apply as in search.
    self_join(threshold) is the same question about the gallery itself: all pairs of rows at or above a threshold, each once;
    count_self_join their number per row; components(threshold) the clusters those pairs form, a label per row, and
    deduplicate(threshold) withdraws all but the smallest row of every cluster.  join(right, threshold) asks it about two indexes: all pairs (row of this index, row of
    right) at or above a threshold, with a filter and group ids on either side; count_join their number per left row.

    Growth.  index.n (= len(index)) rows are searched, index.capacity rows fit the buffer; index.gallery, index.norms and index.keep
    are the first n rows of it, reassigned whenever n changes (a reference taken earlier keeps the rows it had).  capacity=None is the
    constructor above (capacity == n); capacity=c >= n allocates [c, d] rows and [c] norms at once and copies the gallery in
    (c < n: ValueError); nbytes counts the capacity.  add(rows) appends, update(rows, values) overwrites, compact() drops the removed
    rows and returns their old numbering: see the methods.  After any sequence of them gallery, norms and every search are, byte for
    byte, those of a fresh index on the same rows.  The index never writes a tensor it did not allocate: the first add or update on
    a gallery kept by reference moves the rows into a buffer of its own (index.gallery.data_ptr() changes, the caller's bytes stay).
    add and update do not synchronise; compact does.  Everything runs on the current stream, allocation and growth included: an
    index is used from one stream at a time."""

    def __init__(self, gallery, normalize: bool = True, storage=None, capacity=None):
        import torch
        from . import lib as _lib
        codes = _gallery_codes()
        if gallery.dtype not in codes:  # (before the device check: the message a caller needs first)
            raise ValueError(f"GalleryIndex: a gallery of dtype {gallery.dtype}; it has to be {_STORAGE_NAMES}")
        if storage is not None and storage not in codes:
            raise ValueError(f"GalleryIndex: storage = {storage}; it has to be {_STORAGE_NAMES} (or None: the gallery's own dtype)")
        if capacity is not None and gallery.dim() == 2 and int(capacity) < gallery.shape[0]:
            raise ValueError(f"GalleryIndex: capacity = {capacity} is less than the {gallery.shape[0]} rows of the gallery")
        if not gallery.is_cuda:
            raise RuntimeError("GalleryIndex needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)")
        assert gallery.dim() == 2 and gallery.shape[0] >= 1 and gallery.shape[1] >= 1, gallery.shape
        self.storage = gallery.dtype if storage is None else storage
        self._code = codes[self.storage]
        self.normalize = bool(normalize)
        self.keep = None
        self.norms = None
        n, d = gallery.shape
        # _buf / _nbuf / _kbuf: the [capacity, d] rows, [capacity] norms and [capacity] keep flags the index allocated itself, of which
        # gallery / norms / keep are the first n.  _buf is None while the gallery is the caller's tensor, kept by reference.
        self._buf = self._nbuf = self._kbuf = None
        if capacity is None:
            self.gallery = gallery.to(self.storage).contiguous()  # (.to() returns the tensor itself when the dtype is its own)
            if self.gallery.data_ptr() != gallery.data_ptr():
                self._buf = self.gallery  # a converted or contiguous copy is the index's own
        else:
            self._buf = torch.empty(int(capacity), d, dtype=self.storage, device=gallery.device)
            self._buf[:n].copy_(gallery)  # (the conversion of gallery.to(storage))
            self.gallery = self._buf[:n]
        if self.normalize:
            self._nbuf = torch.empty(self.capacity, dtype=torch.float32, device=gallery.device)
            self.norms = self._nbuf[:n]
            st = _stream()
            if self._code:
                _lib.check(_lib.load().coot_retrieval_row_norms_h(self.gallery.data_ptr(), self._code, n, d, self.norms.data_ptr(), st),
                           "coot_retrieval_row_norms_h")
            else:
                _lib.check(_lib.load().coot_retrieval_row_norms(self.gallery.data_ptr(), n, d, self.norms.data_ptr(), st), "coot_retrieval_row_norms")

    @property
    def n(self) -> int:
        """The rows that are searched."""
        return self.gallery.shape[0]

    def __len__(self) -> int:
        return self.gallery.shape[0]

    @property
    def capacity(self) -> int:
        """The rows the buffer holds: add() up to here writes the new rows only."""
        buf = getattr(self, "_buf", None)
        return self.gallery.shape[0] if buf is None else buf.shape[0]

    @property
    def nbytes(self) -> int:
        """The bytes the index keeps on the device: the gallery in its storage type and, when normalising, its fp32 row norms —
        all `capacity` rows of them once the index owns its buffer."""
        rows = self.capacity
        return rows * self.gallery.shape[1] * self.gallery.element_size() + (rows * 4 if self.norms is not None else 0)

    def _set_rows(self, n: int):
        """gallery, norms and keep as views of the first n rows of the index's own buffers."""
        self.gallery = self._buf[:n]
        if self.norms is not None:
            self.norms = self._nbuf[:n]
        if self.keep is not None:
            self.keep = self._kbuf[:n]

    def _own(self, rows: int):
        """Makes the gallery (and norms, and keep flags) live in buffers the index allocated, with room for `rows` rows: the first call
        on a gallery kept by reference copies it; too small a buffer grows to at least twice its size.  Allocation and copies are
        ordinary stream-ordered tensor operations on the current stream."""
        import torch
        n, d, dev = self.gallery.shape[0], self.gallery.shape[1], self.gallery.device
        buf, cap = getattr(self, "_buf", None), self.capacity
        if buf is None or rows > cap:
            cap = rows if rows <= cap else max(rows, 2 * cap)
            self._buf = torch.empty(cap, d, dtype=self.gallery.dtype, device=dev)
            self._buf[:n].copy_(self.gallery)
            if self.norms is not None:
                self._nbuf = torch.empty(cap, dtype=torch.float32, device=dev)
                self._nbuf[:n].copy_(self.norms)
            self._kbuf = None
        kbuf = getattr(self, "_kbuf", None)
        if self.keep is not None and (kbuf is None or kbuf.shape[0] < cap or kbuf.data_ptr() != self.keep.data_ptr()):
            self._kbuf = torch.ones(cap, dtype=torch.bool, device=dev)
            self._kbuf[:n].copy_(self.keep)
        self._set_rows(n)

    def _check_values(self, fn: str, values, rows=None):
        """The rows given to add / update: float32 or the storage type, [R, d] (or [d]: one row), R == rows where that is fixed
        (ValueError), on the device (RuntimeError).  Returns them contiguous, as [R, d]."""
        import torch
        d = self.gallery.shape[1]
        if not isinstance(values, torch.Tensor) or values.dtype not in (torch.float32, self.storage):
            raise ValueError(f"GalleryIndex.{fn}: rows of dtype {getattr(values, 'dtype', type(values).__name__)}; an index held in {self.storage} "
                             f"takes torch.float32" + ("" if self.storage is torch.float32 else f" or {self.storage}"))
        if values.dim() == 1:
            values = values[None]
        if values.dim() != 2 or values.shape[1] != d:
            raise ValueError(f"GalleryIndex.{fn}: rows of shape {tuple(values.shape)}, a gallery of width {d} ([R, {d}] or [{d}])")
        if rows is not None and values.shape[0] != rows:
            raise ValueError(f"GalleryIndex.{fn}: {values.shape[0]} rows of values for {rows} row numbers")
        if not values.is_cuda:
            raise RuntimeError(f"GalleryIndex.{fn} needs CUDA tensors (there is no CPU fallback; build a new index on the host's rows)")
        return values.contiguous()

    def _put(self, values, dest, row0: int, n_rows: int):
        from . import lib as _lib
        _lib.check(_lib.load().coot_retrieval_rows_put(values.data_ptr(), _gallery_codes()[values.dtype], values.shape[0], values.shape[1], _ptr(dest),
                                                       row0, self._buf.data_ptr(), self._code, n_rows,
                                                       self._nbuf.data_ptr() if self.norms is not None else None, _stream()), "coot_retrieval_rows_put")

    def add(self, rows) -> int:
        """Appends rows (cuda float32 or index.storage, [R, d] or [d]) as gallery rows n .. n + R - 1 and returns the first new row
        number, a host integer; nothing is synchronised.  The rows are converted as GalleryIndex(storage=...) converts them and their
        norms are the ones a fresh index computes (coot_retrieval_rows_put): the grown index is, byte for byte, a fresh index on all
        rows.  With room in the buffer (index.capacity) this is one launch that writes O(R d) bytes; without, the buffer first grows
        to at least twice its size.  New rows are searched at once, whatever filter is set."""
        values = self._check_values("add", rows)
        n, r = self.gallery.shape[0], values.shape[0]
        if r == 0:
            return n
        self._own(n + r)
        self._put(values, None, n, self._buf.shape[0])
        if self.keep is not None:
            self._kbuf[n:n + r] = True
        self._set_rows(n + r)
        return n

    def update(self, rows, values):
        """Overwrites gallery rows in place: rows follows the conventions of remove() (a host sequence or CPU tensor is checked:
        IndexError outside [0, n), ValueError for a repeated row; a device int tensor is not: rows outside [0, n) are ignored and of a
        repeated row the last position wins), values is [len(rows), d] as add() takes them.  Stored bytes and norms become those of a
        fresh index on the patched gallery.  The filter is not touched: a removed row that is updated stays removed, and comes back with
        its new value when restored.  No synchronisation."""
        import torch
        n, dev = self.gallery.shape[0], self.gallery.device
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            if rows.dtype.is_floating_point or rows.dtype is torch.bool:
                raise TypeError(f"GalleryIndex.update: rows of dtype {rows.dtype}; row numbers are integers")
            dest = rows.reshape(-1)
        else:
            dest = _host_rows("update", rows, n)
            if len(np.unique(dest)) != len(dest):
                raise ValueError("GalleryIndex.update: a row is given more than once")
        values = self._check_values("update", values, rows=len(dest))
        if len(dest) == 0:
            return
        if isinstance(dest, np.ndarray):
            dest = torch.from_numpy(dest.astype(np.int32)).to(dev)
        else:  # of the positions that name one row the highest keeps it and the others become -1; rows outside [0, n) become n: all skipped
            slot = torch.remainder(dest.to(device=dev, dtype=torch.int64).clamp(-1, n), n + 1)  # in [0, n]: -1 and n are slot n
            pos = torch.arange(len(slot), device=dev)
            last = torch.full((n + 1,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, slot, pos, "amax")
            dest = torch.where(last[slot] == pos, slot, -1).to(torch.int32)
        self._own(n)
        self._put(values, dest, 0, n)

    def compact(self):
        """Drops the removed rows physically: gallery rows and norms of the kept rows are gathered (not recomputed) into buffers of
        exactly that size, index.keep becomes None and capacity == n.  Returns old_rows, int32 [n] on the device: the former row
        number of every row, ascending — old_rows[idx] of a later search names the rows as they were numbered before.  This is the one
        call of the index that synchronises with the device: the new size is needed on the host.  Without a filter nothing moves and
        arange(n) is returned; with nothing kept it raises ValueError and changes nothing."""
        import torch
        n, dev = self.gallery.shape[0], self.gallery.device
        if self.keep is None:
            return torch.arange(n, dtype=torch.int32, device=dev)
        old = torch.nonzero(self.keep)[:, 0]
        if old.numel() == 0:
            raise ValueError("GalleryIndex.compact: every row is removed; an index holds at least one row (restore some, or drop the index)")
        self._buf = self.gallery[old]
        self._nbuf = self.norms[old] if self.norms is not None else None
        self._kbuf = self.keep = None
        self._set_rows(old.numel())
        return old.to(torch.int32)

    def _row_flags(self, fn: str, rows):
        """torch.bool [N] on the device, True at the given rows."""
        import torch
        n, dev = self.gallery.shape[0], self.gallery.device
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda):
            rows = torch.from_numpy(_host_rows(fn, rows, n)).to(dev)
        elif rows.dtype.is_floating_point or rows.dtype is torch.bool:
            raise TypeError(f"GalleryIndex.{fn}: rows of dtype {rows.dtype}; row numbers are integers")
        r = rows.reshape(-1).to(device=dev, dtype=torch.int64)
        hit = torch.zeros(n + 1, dtype=torch.bool, device=dev)  # slot N takes the rows outside [0, N) of an unchecked device tensor
        hit[torch.where((r >= 0) & (r < n), r, torch.full_like(r, n))] = True
        return hit[:n]

    def remove(self, rows):
        """Rows that later searches do not return, until they are restored."""
        import torch
        hit = self._row_flags("remove", rows)
        if self.keep is None:
            self.keep = torch.ones(self.gallery.shape[0], dtype=torch.bool, device=self.gallery.device)
        self.keep &= ~hit

    def restore(self, rows=None):
        """Makes removed rows searchable again; without an argument all of them (index.keep is None again)."""
        if rows is None:
            self.keep = None
        elif self.keep is not None:
            self.keep |= self._row_flags("restore", rows)
        else:
            self._row_flags("restore", rows)  # (nothing is removed: the rows are checked all the same)

    def search(self, queries, k: int, want_sim: bool = False, keep=None):
        m = queries.shape[0] if queries.dim() == 2 else 1
        if m <= RETRIEVAL_FEW_MAX or (self._code and m < INDEX_TILE_MIN_M_16BIT):  # one few-query call, or slices of them (16-bit index)
            return _topk_few(self, queries, k, keep, want_sim)
        return _topk_tile(queries, self.gallery, self.norms if self.normalize else None, k, keep, want_sim, method="GalleryIndex.search", own_keep=self.keep)

    def search_grouped(self, queries, k: int, groups, num_groups=None, keep=None, want_sim: bool = False):
        """The k best GROUPS of rows for every query, each through its best row: (group int32 [M, k], idx int32 [M, k], scores float32
        [M, k], sim [M, N] or None) on the device.  groups: a cuda torch.int32 or torch.int64 tensor [index.n], groups[j] = the group
        of gallery row j (the video of a clip, a speaker, a cluster of near-duplicates).  Exact: compute_retrieval_topk_grouped of the
        similarities search() selects from, byte for byte — with groups = arange(n) idx and scores are those of search(queries, k,
        keep=keep) and group == idx; rows with an id outside [0, num_groups) are never returned; with fewer than k groups left the tail
        is group -1, idx -1, score -inf.  keep and the index's own filter (remove) combine as in search.  1 <= k <= min(N, 128).
        num_groups=None costs one synchronisation with the device (int(groups.max()) + 1): pass num_groups where it is known.
        The index does not store groups; the caller owns the row-to-group table: after add() append to it, after compact() remap it
        with the old row numbers compact returns (groups[old_rows]).  Any M: slices of 16 queries, one sweep of the gallery each
        (retrieval_topk_grouped_device)."""
        return _topk_grouped(queries, self.gallery, self.norms if self.normalize else None, groups, k, num_groups, keep, want_sim,
                             method="GalleryIndex.search_grouped", own_keep=self.keep)

    def search_multi(self, queries, offsets, k: int, groups, num_groups=None, keep=None, want_sim: bool = False):
        """The k best GROUPS of rows for every PARAGRAPH of queries, and which row answers each sentence (MaxSim, late interaction):
        (group int32 [P, k], scores float32 [P, k], rows int32 [M, k], row_scores float32 [M, k], sim [M, N] or None) on the device.
        queries cuda float32 [M, d]: the sentences of all paragraphs, concatenated; offsets: P + 1 integers on the host (a sequence, a
        numpy array or a CPU integer tensor) from 0 to M, non-decreasing, paragraph p = queries[offsets[p]:offsets[p + 1]], possibly
        empty; groups as in search_grouped (the video of a clip).  A group's score for a paragraph is the sum, over its sentences in
        order, of the sentence's best row in the group — the score search_grouped gives that group — in float32, ties to the larger
        group id; a group in which a sentence has no row left is not a candidate; the tail is -1 / -inf, all of an empty paragraph's
        slots.  rows[i, r], row_scores[i, r]: the best row of sentence i in group[p, r] of its paragraph, and its score.  Exact:
        compute_retrieval_topk_multi of the similarities search() selects from, byte for byte.  keep and the index's own filter (remove)
        combine as in search.  1 <= k <= min(N, 128).  num_groups=None costs one synchronisation; the caller owns the row-to-group
        table, as in search_grouped.  Any M: 16 sentences are one sweep of the gallery (retrieval_topk_multi_device)."""
        return _topk_multi(queries, offsets, self.gallery, self.norms if self.normalize else None, groups, k, num_groups, keep, want_sim,
                           method="GalleryIndex.search_multi", own_keep=self.keep)

    def search_scoped(self, queries, k: int, groups, only=None, exclude=None, keep=None, want_sim: bool = False):
        """The k best rows for every query INSIDE ITS OWN SLICE of the gallery: (idx int32 [M, k], scores float32 [M, k], sim [M, N] or
        None) on the device.  groups: a cuda torch.int32 or torch.int64 tensor [index.n], groups[j] = the id of gallery row j (the video
        of a clip, a tenant, a split; any int32 value), or None: every row is its own id.  Exactly one of only= / exclude=, one id per
        query ([M]; a cuda int tensor, or a host sequence, array or CPU tensor that is uploaded once): with only, query i sees the rows
        with groups[j] == only[i] — for a sentence and a video, which clip of that video answers it; with exclude, the rows with
        groups[j] != exclude[i] — everything but one video.  Exact: row i is the bytes of search(queries[i:i + 1], k, keep=eligible_i),
        compute_retrieval_topk_scoped of the similarities search() selects from, in one sweep per 16 queries instead of one mask, one
        call and one sweep per query.  An id that no row carries selects nothing under only (the whole row is -1 / -inf) and excludes
        nothing under exclude; with fewer than k eligible rows the tail is idx -1, score -inf.  keep and the index's own filter
        (remove) combine as in search.  1 <= k <= min(N, 128).  Without sim, blocks of 128 rows in which no row is eligible for any
        query of a slice are not read, so only= over adjacent rows costs the blocks those rows lie in.  Nothing synchronises.  The
        index does not store groups; the caller owns the table across add() and compact(), as in search_grouped."""
        return _topk_scoped(queries, self.gallery, self.norms if self.normalize else None, groups, k, only, exclude, keep, want_sim,
                            method="GalleryIndex.search_scoped", own_keep=self.keep)

    def search_adjusted(self, queries, k: int, offset, keep=None, want_sim: bool = False):
        """The k best rows for every query after A NUMBER PER ROW has been taken off its similarity: (idx int32 [M, k], scores
        float32 [M, k], sim [M, N] or None) on the device.  offset: a cuda torch.float32 tensor [index.n], or index.n numbers on the
        host (a sequence, a numpy array or a CPU tensor; rounded to float32 and uploaded once).  Rows are ranked by a(i, j) =
        s(i, j) - offset[j], one float32 subtraction on the similarity search() ranks on, bit for bit, in search()'s order (a
        descending, then the larger row); scores holds the bytes of a, sim the raw s of every row, the bytes of search(queries, k,
        want_sim=True)[2].  Exact: compute_retrieval_topk_adjusted of those similarities, byte for byte, for every storage type and
        whatever else is in the batch; with offset = 0 the bytes of search(queries, k, keep=keep).  What search(queries, 128), a
        subtraction and a re-sort cannot give, because a row outside the raw top 128 may be inside the adjusted top k.
        index.hubness_offsets(bank) is the offset that corrects hubness (CSLS): search_adjusted(q, k, index.hubness_offsets(bank));
        a recency boost, a popularity prior or a calibration constant per source are offsets too.  offset +inf leaves a row with
        score -inf, still a row and returned last (ties to the larger row), unlike a masked one; -inf puts it first.  keep and the
        index's own filter (remove) combine as in search; with fewer than k kept rows the tail is idx -1, score -inf.  1 <= k <=
        min(N, 128).  Nothing synchronises.  Any M: slices of 16 queries, one sweep of the gallery each, or from ADJUSTED_TILE_MIN_M /
        ADJUSTED_TILE_MIN_M_16BIT queries on one tile call, with the same bytes (retrieval_topk_adjusted_device).  The index does not store offsets; the caller owns the vector across add() (append to it)
        and compact() (offset[old_rows]), as for groups in search_grouped."""
        return _topk_adjusted(queries, self.gallery, self.norms if self.normalize else None, offset, k, keep, want_sim,
                              method="GalleryIndex.search_adjusted", own_keep=self.keep)

    def hubness_offsets(self, bank, k: int = 10, keep=None, other_keep=None):
        """The offsets that make search_adjusted rank by CSLS, a correction of HUBNESS (rows close to the common direction of all
        queries, which are top-1 for many queries they do not belong to): a cuda float32 [index.n], offsets[j] = half the mean
        similarity of row j to its k nearest rows of `bank`, a GalleryIndex of representative queries (the training captions) with
        the same width, normalize and device (TypeError / ValueError before anything is launched, as in knn_join).  CSLS is
        2 s(i, j) - r_q(i) - r_g(j); r_q is constant per query, so query i ranks by s(i, j) - r_g(j) / 2.
        self.knn_join(bank, k, keep=keep, other_keep=other_keep), then one launch of coot_retrieval_hub_offsets: per row the scores of
        the filled slots added in rank order in float32, divided by their number and halved; a row that keep or the index's own
        filter masks, and every row when no bank row is eligible, gets 0.  compute_retrieval_hub_offsets of knn_join's output, byte
        for byte.  1 <= k <= min(len(bank), 128).  Nothing synchronises."""
        import torch
        from . import lib as _lib
        who = "GalleryIndex.hubness_offsets"
        self._check_right(who, bank)
        idx, scores = _knn_join(self.gallery, self.norms if self.normalize else None, bank.gallery, bank.norms if bank.normalize else None, k, keep,
                                other_keep, None, None, False, method=who, own_keep=self.keep, other_own_keep=bank.keep)
        out = torch.empty(idx.shape[0], dtype=torch.float32, device=idx.device)
        _lib.check(_lib.load().coot_retrieval_hub_offsets(scores.data_ptr(), idx.data_ptr(), idx.shape[0], idx.shape[1], out.data_ptr(), _stream()),
                   "coot_retrieval_hub_offsets")
        return out

    def search_range(self, queries, threshold, keep=None, max_results=None, order: str = "row"):
        """EVERY row that scores at least the query's threshold, however many there are: (offsets int64 [M + 1], rows int32 [T], scores
        float32 [T]) on the device, CSR — the hits of query i are rows[offsets[i]:offsets[i + 1]], in ascending row order, with their
        scores.  threshold: a Python number, M numbers on the host or a cuda torch.float32 tensor [M].  A hit is a row that keep and
        the index's own filter (remove) let pass with s(i, j) >= threshold[i] in float32, s being the similarity search() ranks on,
        bit for bit: compute_retrieval_range of the sim that search(queries, k, want_sim=True) returns, byte for byte, for every
        storage type and whatever else is in the batch.  What search(queries, 128) filtered by a threshold cannot give once more than
        128 rows qualify, and without the M x N matrix of queries @ gallery.T >= t.  max_results=None reads the size back (the one
        synchronisation) and allocates exactly; max_results=c never synchronises, returns c entries (-1 / -inf behind the result) and
        leaves offsets exact, so offsets[M] > c tells that the result was cut.  order="score": every segment best first, as search()
        orders (max_results=None only).  Up to RANGE_TILE_MIN_M - 1 queries (RANGE_TILE_MIN_M_16BIT - 1 on a 16-bit index) run in
        slices of 16 through the sweep, more in two tile calls over all queries; the bytes are the same.  See retrieval_range_device."""
        return _range(queries, self.gallery, self.norms if self.normalize else None, threshold, keep, max_results, order,
                      method="GalleryIndex.search_range", own_keep=self.keep)

    def count_range(self, queries, threshold, keep=None):
        """How many rows search_range would return per query, int32 [M] on the device: the counting sweep (from RANGE_TILE_MIN_M /
        RANGE_TILE_MIN_M_16BIT queries on: the counting tile call, as in search_range) and the scan, no synchronisation and no second
        sweep.  (The distractors that beat a ground truth: threshold = its score.)"""
        return _range(queries, self.gallery, self.norms if self.normalize else None, threshold, keep, None, "row",
                      method="GalleryIndex.count_range", own_keep=self.keep, count_only=True)

    def self_join(self, threshold, keep=None, groups=None, max_results=None):
        """The gallery against itself: ALL PAIRS of rows at or above a threshold (near-duplicate clips before a split is frozen):
        (offsets int64 [N + 1], rows int32 [T], scores float32 [T]) on the device, the CSR of search_range read as pairs — the hits of
        row i are the rows j > i, rows[offsets[i]:offsets[i + 1]], in ascending j, with the bytes of their scores; every unordered pair
        appears once, under its smaller row.  The i of every pair: counts = offsets[1:] - offsets[:-1]; i =
        torch.repeat_interleave(torch.arange(N, device=rows.device), counts, output_size=T).
        threshold: a Python number, N numbers on the host or a cuda torch.float32 tensor [N], one per row.  Pair (i, j), i < j, is a
        hit when keep (cuda torch.bool or torch.uint8 [N]) and the index's own filter (remove) let BOTH rows pass — a removed row
        neither asks nor is returned, its segment is empty —, groups is None or groups[i] != groups[j] (cuda torch.int32 or
        torch.int64 [N]: the video of a clip, so that the pairs are the near-duplicates ACROSS videos; the caller owns the table, as
        in search_grouped), and s(i, j) >= threshold[i] in float32.  s is, bit for bit, the sim of search(gallery.float(), 1,
        want_sim=True), and s(i, j) == s(j, i) on bytes; NaN, -0 and the infinities behave as in search_range.  Without groups, row
        i's hits are those of search_range(gallery[i].float(), threshold[i], keep=keep) with j <= i dropped, when keep lets row i
        pass: compute_retrieval_self_join of the similarities, byte for byte, for every storage type.
        Both operands are read from the gallery as the index stores it and both norms are the index's: no float32 copy, no norm pass,
        and the blocks left of the diagonal are not visited.  The rows are worked through in chunks whose table of block counts stays
        under retrieval.JOIN_TABLE_BYTES (read at call time; chunks start at multiples of 128 rows and hold at least 128); the bytes
        of the result do not depend on it.  max_results=None reads back one size per chunk and concatenates the chunks' results: one
        synchronisation when the table fits in one chunk.  max_results=c >= 1 never synchronises: the offsets of a chunk are shifted on
        the device by the running total, rows / scores have c entries, the first min(T, c) of the result and then -1 / -inf, and
        offsets stay exact, so offsets[N] > c says that the result was cut.  Segments are in row order; there is no order= here."""
        return _self_join(self.gallery, self.norms if self.normalize else None, threshold, keep, groups, max_results,
                          method="GalleryIndex.self_join", own_keep=self.keep)

    def count_self_join(self, threshold, keep=None, groups=None):
        """How many pairs self_join would return per row, int32 [N] on the device: the count pass and the scan of every chunk, no
        fill and no synchronisation.  Its sum is the number of pairs."""
        return _self_join(self.gallery, self.norms if self.normalize else None, threshold, keep, groups, None,
                          method="GalleryIndex.count_self_join", own_keep=self.keep, count_only=True)

    def components(self, threshold, keep=None, groups=None):
        """DUPLICATE CLUSTERS: the connected components of the gallery under the pairs of self_join(threshold, keep=keep,
        groups=groups), as a label per row, int32 [N] on the device; nothing synchronises.  The edge set is exactly that hit set:
        pair (i, j), i < j, is an edge when keep and the index's own filter (remove) let BOTH rows pass, groups is None or groups[i] !=
        groups[j], and s(i, j) >= threshold[i] in float32, with the bits of s of every search; threshold takes self_join's three forms
        (a Python number, N numbers on the host, a cuda torch.float32 tensor [N]), and NaN, -0 and the infinities follow from the
        same compare.  labels[i] is the smallest row number in the connected component of row i: a row without an edge labels itself; a
        row that the filters mask is -1, and is no vertex, so it does not connect its neighbours.  With groups, two rows of one group
        are never joined directly; they may still land in one component through a row of another group.  The rows to keep when a
        split is frozen are those with labels[i] == i (see deduplicate).
        compute_retrieval_components of the similarities, byte for byte: the result is a function of the edge set only and depends on
        neither the schedule, the storage type (beyond the exact widening) nor a rerun.  One call of coot_retrieval_components: the
        upper triangle is swept once, as count_self_join sweeps it, and each hit is a union in a parent array of N int32 — no table,
        no scan, no fill pass, no pair list, no chunks; 8 bytes per row beyond the index (the workspace and the labels).  N <=
        retrieval.COMPONENTS_ROWS_MAX (ValueError), because one launch covers all rows."""
        return _components(self.gallery, self.norms if self.normalize else None, threshold, keep, groups,
                           method="GalleryIndex.components", own_keep=self.keep)

    def deduplicate(self, threshold, keep=None, groups=None):
        """components(threshold, keep=keep, groups=groups), and every row that is not the smallest of its cluster withdrawn, as
        remove() withdraws it: the rows with labels[i] >= 0 and labels[i] != i leave index.keep, on the device, without a
        synchronisation and without compact().  Returns labels.  Each cluster keeps its smallest row; masked rows (-1) are left as
        they were.  Afterwards count_self_join(threshold, keep=keep, groups=groups).sum() is 0: two surviving rows with an edge would
        have shared a component.  restore() brings every row back."""
        import torch
        labels = _components(self.gallery, self.norms if self.normalize else None, threshold, keep, groups,
                             method="GalleryIndex.deduplicate", own_keep=self.keep)
        n, dev = self.gallery.shape[0], self.gallery.device
        if self.keep is None:
            self.keep = torch.ones(n, dtype=torch.bool, device=dev)
        self.keep &= ~((labels >= 0) & (labels != torch.arange(n, dtype=torch.int32, device=dev)))
        return labels

    def _check_right(self, who: str, other):
        """What two indexes have to share before rows of one meet rows of the other (join, count_join, knn_join)."""
        if not isinstance(other, GalleryIndex):
            raise TypeError(f"{who}: the right side has to be a GalleryIndex, not {type(other).__name__}")
        if other.gallery.shape[1] != self.gallery.shape[1]:
            raise ValueError(f"{who}: this index holds rows of width {self.gallery.shape[1]}, the right one of width {other.gallery.shape[1]}")
        if self.normalize != other.normalize:
            raise ValueError(f"{who}: this index has normalize={self.normalize}, the right one normalize={other.normalize} "
                             "(one similarity needs both norms or none)")
        if other.gallery.device != self.gallery.device:
            raise ValueError(f"{who}: this index lives on {self.gallery.device}, the right one on {other.gallery.device}")

    def _join(self, who: str, other, threshold, keep, other_keep, groups, other_groups, max_results, count_only: bool):
        """join / count_join: what two indexes have to share, then _cross_join on what they hold."""
        self._check_right(who, other)
        return _cross_join(self.gallery, self.norms if self.normalize else None, other.gallery, other.norms if other.normalize else None,
                           threshold, keep, other_keep, groups, other_groups, max_results, method=who, own_keep=self.keep,
                           other_own_keep=other.keep, count_only=count_only)

    def join(self, right, threshold, keep=None, other_keep=None, groups=None, other_groups=None, max_results=None):
        """This index against ANOTHER one: all pairs (row i of this index, row j of `right`) at or above a threshold (does the
        validation split leak into the training split; which rows of an upload the resident corpus already holds): (offsets int64
        [N_left + 1], rows int32 [T], scores float32 [T]) on the device, the CSR of search_range read as pairs — the hits of left
        row i are rows[offsets[i]:offsets[i + 1]], rows of `right` in ascending order, with the bytes of their scores.  The i of
        every pair: counts = offsets[1:] - offsets[:-1]; i = torch.repeat_interleave(torch.arange(N_left, device=rows.device),
        counts, output_size=T).
        threshold: a Python number, N_left numbers on the host or a cuda torch.float32 tensor [N_left], one per left row.  Pair
        (i, j) is a hit when keep (cuda torch.bool or torch.uint8 [N_left]) and this index's own filter (remove) let row i pass — a
        removed left row does not ask, its segment is empty —, other_keep ([N_right]) and right's own filter let row j pass, groups
        and other_groups are both None or groups[i] != other_groups[j] (cuda torch.int32 or torch.int64 [N_left] and [N_right] in one
        id space: the source video of a clip, so that clips of one video in both splits are no leak; the caller owns the tables, as
        in search_grouped; exactly one of them is a ValueError), and s(i, j) >= threshold[i] in float32.  s is, bit for bit, the sim
        of right.search(self.gallery.float(), 1, want_sim=True); NaN, -0 and the infinities behave as in search_range.  Without
        groups, row i's hits are those of right.search_range(self.gallery[i].float(), threshold[i], keep=other_keep) when the left
        filters let row i pass: compute_retrieval_join of the similarities, byte for byte, for all nine pairs of storage types.
        Both operands are read as their index stores them and both norms are the stored ones: no float32 copy of the left side and
        no norm pass.  `right` has to be a GalleryIndex of the same width, the same normalize and on the same device (TypeError /
        ValueError before anything is launched); right may be this index itself, which returns both orientations and the diagonal.
        The left rows are worked through in chunks whose table of block counts, rows x (ceil(N_right / 128) + 1) int32, stays under
        retrieval.JOIN_TABLE_BYTES (read at call time; chunks start at multiples of 64 rows and hold at least 64); the bytes of the
        result do not depend on it.  max_results=None reads back one size per chunk and concatenates the chunks' results: one
        synchronisation when the table fits in one chunk.  max_results=c >= 1 never synchronises: the offsets of a chunk are
        shifted on the device by the running total, rows / scores have c entries, the first min(T, c) of the result and then
        -1 / -inf, and offsets stay exact, so offsets[N_left] > c says that the result was cut.  Segments are in row order; there
        is no order= here."""
        return self._join("GalleryIndex.join", right, threshold, keep, other_keep, groups, other_groups, max_results, False)

    def count_join(self, right, threshold, keep=None, other_keep=None, groups=None, other_groups=None):
        """How many pairs join would return per left row, int32 [N_left] on the device: the count pass and the scan of every chunk,
        no fill and no synchronisation.  Its sum is the number of pairs."""
        return self._join("GalleryIndex.count_join", right, threshold, keep, other_keep, groups, other_groups, None, True)

    def knn_join(self, right, k: int, keep=None, other_keep=None, groups=None, other_groups=None):
        """The k best rows of ANOTHER index for EVERY row of this one (the closest training items of every validation item; each
        clip's hardest negatives in a second split): (idx int32 [N_left, k], scores float32 [N_left, k]) on the device, rows of
        `right`, best first.  Pair (i, j) is eligible when keep (cuda torch.bool or torch.uint8 [N_left]) and this index's own filter
        (remove) let row i pass, other_keep ([N_right]) and right's own filter let row j pass, and groups and other_groups are both
        None or groups[i] != other_groups[j] (cuda torch.int32 or torch.int64 [N_left] and [N_right] in one id space: the source
        video of a clip; the caller owns the tables, as in search_grouped; exactly one of them is a ValueError).  Row i holds the k
        best eligible j in the order of every search, score descending, then the larger row; fewer than k eligible rows leave a
        tail of -1 / -inf, and a row of this index that the left filters mask is -1 / -inf throughout: a removed row does not ask
        (unlike neighbors).  s(i, j) is, bit for bit, the sim of right.search(self.gallery.float(), 1, want_sim=True), so an
        unmasked row i is, byte for byte, right.search_scoped(self.gallery[i:i + 1].float(), k, other_groups,
        exclude=groups[i:i + 1], keep=other_keep), and without groups right.search(self.gallery.float(), k, keep=other_keep):
        compute_retrieval_knn_join of the similarities, for all nine pairs of storage types.  Both operands are read as their index
        stores them and both norms are the stored ones: no float32 copy of the left side, no norm pass, and one pass of 64 left rows
        per workgroup over the right index instead of one sweep per 16 queries.  `right` has to be a GalleryIndex of the same width,
        the same normalize and on the same device (TypeError / ValueError before anything is launched); right may be this index
        itself, and then a row returns itself (see knn_graph).  1 <= k <= min(N_right, 128), checked against N_right whatever the
        filters hold; N_left <= retrieval.KNN_JOIN_ROWS_MAX.  Nothing synchronises."""
        who = "GalleryIndex.knn_join"
        self._check_right(who, right)
        return _knn_join(self.gallery, self.norms if self.normalize else None, right.gallery, right.norms if right.normalize else None, k, keep,
                         other_keep, groups, other_groups, False, method=who, own_keep=self.keep, other_own_keep=right.keep)

    def knn_graph(self, k: int, keep=None, groups=None):
        """The k nearest rows of this index for EVERY one of its rows (a k-NN graph for clustering or de-duplication where no
        threshold is known; hard negatives over a whole split): (idx int32 [N, k], scores float32 [N, k]) on the device.  knn_join
        of the index with itself, keep (cuda torch.bool or torch.uint8 [N]) applying to both sides as in self_join, and a row never
        returns itself: with groups=None row j is eligible for row i when j != i, with groups (cuda torch.int32 or torch.int64 [N])
        when groups[j] != groups[i] — each clip's nearest clips from OTHER videos.  For a row that keep and the index's own filter
        let pass, the bytes of neighbors([i], k, groups, keep=keep); a row that they mask is -1 / -inf throughout (a removed row does
        not ask), and an exact duplicate elsewhere in the index is returned.  Against neighbors(arange(N), k): no float32 copy of the
        gallery and one pass per 64 rows instead of one sweep per 16.  1 <= k <= min(N, 128); nothing synchronises."""
        who = "GalleryIndex.knn_graph"
        norms = self.norms if self.normalize else None
        return _knn_join(self.gallery, norms, self.gallery, norms, k, keep, keep, groups, groups, groups is None, method=who,
                         own_keep=self.keep, other_own_keep=self.keep)

    def neighbors(self, rows, k: int, groups=None, keep=None):
        """More like this: the k best rows for each of the index's own rows, (idx int32 [R, k], scores float32 [R, k]) on the device.
        rows: row numbers, a host sequence or CPU tensor (checked: IndexError outside [0, n)) or a cuda int tensor (not checked: a
        number outside [0, n) is clamped into it).  The queries are gallery[rows] widened to float32 (exact), and the search is
        search_scoped(queries, k, groups, exclude=groups[rows], keep=keep): a row never returns its own group — with groups its own
        video's other clips, with groups=None (every row its own id) just itself.  An exact duplicate of a row elsewhere in the gallery
        is returned, ahead of everything it ties with by the larger row.  Removed rows may be asked about and are never returned."""
        import torch
        n, dev = self.gallery.shape[0], self.gallery.device
        fn = "GalleryIndex.neighbors"
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            if rows.dtype.is_floating_point or rows.dtype is torch.bool:
                raise TypeError(f"{fn}: rows of dtype {rows.dtype}; row numbers are integers")
            r = rows.reshape(-1).to(torch.int64).clamp(0, n - 1)
        else:
            r = _host_rows("neighbors", rows, n)
        if groups is not None:
            groups = _check_groups(fn, groups, n, mirror=None)
        if not self.gallery.is_cuda or (groups is not None and not groups.is_cuda):
            raise RuntimeError(f"{fn} needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_scoped)")
        if isinstance(r, np.ndarray):
            r = torch.from_numpy(r).to(dev)
        scope = r.to(torch.int32) if groups is None else groups[r]
        idx, scores, _ = _topk_scoped(self.gallery[r].float(), self.gallery, self.norms if self.normalize else None, groups, k, None, scope, keep,
                                      False, method=fn, own_keep=self.keep)
        return idx, scores


def retrieval_ranks_labeled_device(queries, gallery, labels, normalize: bool = False, want_sim: bool = False):
    """queries [M, d], gallery [N, d]: cuda float32; labels: cuda int32 [M].  Returns (ranks_q int32 [M], ranks_g int32 [N],
    n_valid int32 [2], metrics float32 [2, 7], sim [M, N] or None), all on the device (no synchronisation): compute_retrieval_labeled
    of the fp32 similarities retrieval_topk_device selects from, without the M x N matrix (want_sim is a testing aid)."""
    import torch
    from . import lib as _lib
    queries, gallery = _device_pair("retrieval_ranks_labeled_device", "compute_retrieval_labeled", queries, gallery, torch.float32, same_shape=False)
    _on_device("retrieval_ranks_labeled_device", "compute_retrieval_labeled", labels)
    (m, d), n = queries.shape, gallery.shape[0]
    assert labels.dtype == torch.int32 and labels.shape == (m,), (labels.dtype, labels.shape, m)
    labels = labels.contiguous()
    lib = _lib.load()
    dev = queries.device
    ws = torch.empty(lib.coot_retrieval_ranks_labeled_workspace_bytes(m, n, d), dtype=torch.uint8, device=dev)
    ranks_q = torch.empty(m, dtype=torch.int32, device=dev)
    ranks_g = torch.empty(n, dtype=torch.int32, device=dev)
    n_valid = torch.empty(2, dtype=torch.int32, device=dev)
    met = torch.empty(2, 7, dtype=torch.float32, device=dev)
    sim = torch.empty(m, n, dtype=torch.float32, device=dev) if want_sim else None
    _lib.check(lib.coot_retrieval_ranks_labeled(queries.data_ptr(), gallery.data_ptr(), labels.data_ptr(), m, n, d, int(normalize),
                                                ranks_q.data_ptr(), ranks_g.data_ptr(), n_valid.data_ptr(), met.data_ptr(), _ptr(sim), ws.data_ptr(),
                                                ws.numel(), _stream()), "coot_retrieval_ranks_labeled")
    return ranks_q, ranks_g, n_valid, met, sim


def _metric_dicts(met):
    """(res_1to2, res_2to1, sum_at_1) with the reference's dictionary keys, from the device's metrics [2, 7]: the one 56-byte D2H copy."""
    m = met.cpu().numpy().astype(np.float64)
    res1 = {k: float(v) for k, v in zip(VALKEYS, m[0])}
    res2 = {k: float(v) for k, v in zip(VALKEYS, m[1])}
    return res1, res2, (res1["r1"] + res2["r1"]) / 2


def compute_retrieval_labeled_device(queries, gallery, labels, normalize: bool = False):
    """Device version of compute_retrieval_labeled for embeddings (not a similarity matrix): (res_q2g, res_g2q, sum_at_1) with the
    reference's dictionary keys, as compute_retrieval_device returns them.  One 56-byte D2H copy."""
    return _metric_dicts(retrieval_ranks_labeled_device(queries, gallery, labels, normalize)[3])


def retrieval_ranks_adjusted_device(queries, gallery, labels, col_offset=None, row_offset=None, normalize: bool = False, want_sim: bool = False):
    """retrieval_ranks_labeled_device under offsets (coot_retrieval_ranks_adjusted): queries [M, d], gallery [N, d]: cuda float32; labels:
    cuda int32 [M]; col_offset: None, a cuda torch.float32 tensor [N] or N numbers on the host (a sequence, a numpy array or a CPU
    tensor, rounded to float32 once and uploaded once), the offset of GalleryIndex.search_adjusted; row_offset: the same with M numbers,
    one per query.  Returns (ranks_q int32 [M], ranks_g int32 [N], n_valid int32 [2], metrics float32 [2, 7], sim [M, N] or None), all
    on the device (no synchronisation): compute_retrieval_labeled_adjusted of the fp32 similarities retrieval_ranks_labeled_device counts
    on, byte for byte, a(i, j) = (s(i, j) - col[j]) - row[i], without the M x N matrix (want_sim is a testing aid and holds the raw s).
    Without offsets, and with zeros, the bytes of retrieval_ranks_labeled_device.  Checked on the host before anything is launched
    (ValueError): two float32 matrices of one width, int32 labels [M], the offsets' type, shape and device; then that everything lives
    on the device (RuntimeError naming the mirror)."""
    import torch
    from . import lib as _lib
    fn, mirror = "retrieval_ranks_adjusted_device", "compute_retrieval_labeled_adjusted"
    for name, t in (("queries", queries), ("gallery", gallery)):
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.float32 or t.dim() != 2:
            raise ValueError(f"{fn}: {name} has to be a torch.float32 tensor of two dimensions, not {getattr(t, 'dtype', type(t).__name__)} "
                             f"of shape {tuple(getattr(t, 'shape', ()))}")
    (m, d), n = queries.shape, gallery.shape[0]
    if gallery.shape[1] != d:
        raise ValueError(f"{fn}: queries of width {d}, gallery of width {gallery.shape[1]}")
    if m < 1 or n < 1 or d < 1:
        raise ValueError(f"{fn}: M = {m}, N = {n}, d = {d}; each has to be at least 1")
    if not isinstance(labels, torch.Tensor) or labels.dtype is not torch.int32 or tuple(labels.shape) != (m,):
        raise ValueError(f"{fn}: labels has to be a torch.int32 tensor [{m}] (one gallery row per query), not "
                         f"{getattr(labels, 'dtype', type(labels).__name__)} of shape {tuple(getattr(labels, 'shape', ()))}")
    col = None if col_offset is None else _check_offset(f"{fn} (col_offset)", col_offset, n, gallery.device)
    row = None if row_offset is None else _check_offset(f"{fn} (row_offset)", row_offset, m, gallery.device)
    _on_device(fn, mirror, queries, gallery, labels)
    if queries.device != gallery.device or labels.device != gallery.device:
        raise ValueError(f"{fn}: queries live on {queries.device}, labels on {labels.device}, the gallery on {gallery.device}")
    queries, gallery, labels = queries.contiguous(), gallery.contiguous(), labels.contiguous()
    dev = queries.device
    col, row = [None if o is None else torch.from_numpy(o).to(dev) if isinstance(o, np.ndarray) else o.contiguous() for o in (col, row)]
    lib = _lib.load()
    ws = torch.empty(lib.coot_retrieval_ranks_adjusted_workspace_bytes(m, n, d), dtype=torch.uint8, device=dev)
    ranks_q = torch.empty(m, dtype=torch.int32, device=dev)
    ranks_g = torch.empty(n, dtype=torch.int32, device=dev)
    n_valid = torch.empty(2, dtype=torch.int32, device=dev)
    met = torch.empty(2, 7, dtype=torch.float32, device=dev)
    sim = torch.empty(m, n, dtype=torch.float32, device=dev) if want_sim else None
    _lib.check(lib.coot_retrieval_ranks_adjusted(queries.data_ptr(), gallery.data_ptr(), labels.data_ptr(), _ptr(row), _ptr(col), m, n, d, int(normalize),
                                                 ranks_q.data_ptr(), ranks_g.data_ptr(), n_valid.data_ptr(), met.data_ptr(), _ptr(sim), ws.data_ptr(),
                                                 ws.numel(), _stream()), "coot_retrieval_ranks_adjusted")
    return ranks_q, ranks_g, n_valid, met, sim


def compute_retrieval_adjusted_device(queries, gallery, labels, col_offset=None, row_offset=None, normalize: bool = False):
    """Device version of compute_retrieval_labeled_adjusted for embeddings (not a similarity matrix): (res_q2g, res_g2q, sum_at_1) with
    the reference's dictionary keys, as compute_retrieval_labeled_device returns them.  One 56-byte D2H copy."""
    return _metric_dicts(retrieval_ranks_adjusted_device(queries, gallery, labels, col_offset, row_offset, normalize)[3])


def compute_retrieval_csls_device(emb1, emb2, k: int = 10, labels=None):
    """The retrieval metrics of a validation pair under CSLS, the hubness correction in both directions: (res_1to2, res_2to1, sum_at_1)
    with the reference's dictionary keys.  emb1 [M, d] (the queries), emb2 [N, d] (the gallery): cuda float32; labels: cuda int32 [M],
    labels[i] = the row of emb2 that belongs to row i of emb1, or None: arange (M == N, the ground truth on the diagonal).  Both sides
    are normalised; CSLS(i, j) = 2 s(i, j) - r_1(i) - r_2(j), r_1(i) the mean similarity of row i of emb1 to its k nearest rows of emb2
    and r_2(j) the same for row j of emb2 in emb1, ranks as (s(i, j) - r_2(j) / 2) - r_1(i) / 2 does: two GalleryIndex(normalize=True)
    that keep the embeddings by reference, row = idx1.hubness_offsets(idx2, k), col = idx2.hubness_offsets(idx1, k), then
    compute_retrieval_adjusted_device(emb1, emb2, labels, col, row, normalize=True).  1 <= k <= min(M, N, 128).  Checked on the host
    before anything is launched (ValueError).  One 56-byte D2H copy."""
    import torch
    fn = "compute_retrieval_csls_device"
    for name, t in (("emb1", emb1), ("emb2", emb2)):
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.float32 or t.dim() != 2:
            raise ValueError(f"{fn}: {name} has to be a torch.float32 tensor of two dimensions, not {getattr(t, 'dtype', type(t).__name__)} "
                             f"of shape {tuple(getattr(t, 'shape', ()))}")
    if emb1.shape[1] != emb2.shape[1]:
        raise ValueError(f"{fn}: emb1 of width {emb1.shape[1]}, emb2 of width {emb2.shape[1]}")
    m, n = emb1.shape[0], emb2.shape[0]
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(m, n, 128):
        raise ValueError(f"{fn}: k = {k!r} is outside 1 .. min(M = {m}, N = {n}, 128)")
    if labels is None and m != n:
        raise ValueError(f"{fn}: labels=None puts the ground truth on the diagonal, which needs as many rows in emb1 ({m}) as in emb2 ({n})")
    if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype is not torch.int32 or tuple(labels.shape) != (m,)):
        raise ValueError(f"{fn}: labels has to be None or a torch.int32 tensor [{m}], not {getattr(labels, 'dtype', type(labels).__name__)} "
                         f"of shape {tuple(getattr(labels, 'shape', ()))}")
    _on_device(fn, "compute_retrieval_labeled_adjusted", emb1, emb2, labels)
    emb1, emb2 = emb1.contiguous(), emb2.contiguous()
    idx1, idx2 = GalleryIndex(emb1, normalize=True), GalleryIndex(emb2, normalize=True)
    row, col = idx1.hubness_offsets(idx2, int(k)), idx2.hubness_offsets(idx1, int(k))
    if labels is None:
        labels = torch.arange(m, dtype=torch.int32, device=emb1.device)
    return compute_retrieval_adjusted_device(emb1, emb2, labels, col, row, normalize=True)


def retrieval_ranks_part_device(emb1, emb2, row0: int, rows: int, normalize: bool = False, want_sim: bool = False):
    """One strip of retrieval_ranks_device: the rows [row0, row0 + rows) of emb1 . emb2^T against all N columns.  Returns
    (counts int32 [2, N], sim [rows, N] or None) on the device: counts[0] holds the final ranks_12 of the strip's rows (0
    elsewhere), counts[1] the strip's share of every column's ranks_21.  The sums over the strips of any partition of [0, N) are
    retrieval_ranks_device's rank vectors exactly (coot_retrieval_ranks_part, include/coot_hip.h); rows == 0 gives zeros."""
    import torch
    from . import lib as _lib
    emb1, emb2 = _device_pair("retrieval_ranks_part_device", "compute_retrieval_counts_part", emb1, emb2, torch.float32)
    n, d = emb1.shape
    row0, rows = int(row0), int(rows)
    assert 0 <= row0 and 0 <= rows and row0 + rows <= n, (row0, rows, n)
    lib = _lib.load()
    ws = torch.empty(lib.coot_retrieval_ranks_part_workspace_bytes(n, d), dtype=torch.uint8, device=emb1.device)
    counts = torch.empty(2, n, dtype=torch.int32, device=emb1.device)
    sim = torch.empty(rows, n, dtype=torch.float32, device=emb1.device) if want_sim else None
    _lib.check(lib.coot_retrieval_ranks_part(emb1.data_ptr(), emb2.data_ptr(), n, d, int(normalize), row0, rows, counts[0].data_ptr(),
                                             counts[1].data_ptr(), _ptr(sim), ws.data_ptr(), ws.numel(), _stream()), "coot_retrieval_ranks_part")
    return counts, sim


def retrieval_metrics_device(ranks_12, ranks_21):
    """The metrics [2, 7] float32 (VALKEYS order, 1 -> 2 then 2 -> 1) of two cuda int32 rank vectors [N] with entries in [0, N):
    the bits retrieval_ranks_device returns for the same ranks (coot_retrieval_metrics).  On the device, no synchronisation."""
    import torch
    from . import lib as _lib
    ranks_12, ranks_21 = _device_pair("retrieval_metrics_device", "compute_retrieval_cosine", ranks_12, ranks_21, torch.int32, dim=1)
    n = ranks_12.shape[0]
    hist = torch.empty(2 * n, dtype=torch.int32, device=ranks_12.device)
    met = torch.empty(2, 7, dtype=torch.float32, device=ranks_12.device)
    _lib.check(_lib.load().coot_retrieval_metrics(ranks_12.data_ptr(), ranks_21.data_ptr(), n, met.data_ptr(), hist.data_ptr(), hist.numel() * 4,
                                                  _stream()), "coot_retrieval_metrics")
    return met


def compute_retrieval_device(emb1, emb2, normalize: bool = False, dp=None):
    """Device version of compute_retrieval (nntrainer/retrieval.py:31-65): (res_1to2, res_2to1, sum_at_1) with the
    reference's dictionary keys.  One 56-byte D2H copy.
    ``dp`` (dist.DataParallelContext) with more than one rank: every rank holds the SAME emb1 / emb2, counts its strip of rows
    (strip_bounds), ONE integer all-reduce of the [2, N] counts makes the rank vectors, and the metrics kernel runs on them —
    the same dictionaries, bit for bit, on every rank.  Without one, or with one rank: the strip is all rows and nothing is reduced."""
    W, R = (dp.world, dp.rank) if dp is not None and dp.world > 1 else (1, 0)
    row0, rows = strip_bounds(emb1.shape[0], W, R)
    counts, _ = retrieval_ranks_part_device(emb1, emb2, row0, rows, normalize)
    if W > 1:
        dp.all_reduce_sum(counts)
    return _metric_dicts(retrieval_metrics_device(counts[0], counts[1]))
