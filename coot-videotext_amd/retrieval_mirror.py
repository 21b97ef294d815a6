"""Host (numpy) mirrors of the retrieval results: the byte-exact definitions the device code in retrieval.py is compared against.
Nothing here touches the device or imports torch; retrieval.py re-exports every name.
Retrieval metrics, nntrainer/retrieval.py:31-98 semantics: rank of the diagonal item in argsort(row)[::-1]; R@K as
fractions; medr = floor(median)+1; meanr = mean+1.
compute_retrieval / compute_retrieval_cosine: mirror of the reference functions, for CPU tensors.
compute_retrieval_topk (_masked, _grouped, _multi, _scoped): WHICH gallery items a query retrieves (the reference returns top1 only),
on a similarity matrix [M, N], M and N independent; under a keep flag per gallery row; the K best GROUPS of rows, each through its
best row; the K best groups for a PARAGRAPH of queries (MaxSim), whose offsets _host_offsets checks for mirror and device wrappers
alike; under a mask per QUERY, the rows with (only) or without (exclude) the id the query brings.
compute_retrieval_topk_adjusted: compute_retrieval_topk_masked after a number per column has been taken off every similarity.
compute_retrieval_hub_offsets: the lists of a k-NN join into such a number per row, half the mean score of its filled slots (CSLS).
compute_retrieval_range: every column at or above a row's threshold, however many, as CSR.
compute_retrieval_self_join: the same on a gallery's similarities with itself, read as pairs: the columns right of the diagonal.
compute_retrieval_components: the connected components of those pairs, a cluster label per row: a plain host union-find.
compute_retrieval_join: the same on the similarities of two galleries, with a filter and group ids on either side.
compute_retrieval_knn_join: the k best partners of every row under those filters, in the order of compute_retrieval_topk.
compute_retrieval_labeled: ranks and metrics without the assumption "square, ground truth on the diagonal": labels[i] = the gallery
row of query i; several queries per row, rows without a query and queries without a row (a label outside [0, N)) are allowed.
compute_retrieval_labeled_adjusted: the same after a number per column and a number per row have been taken off every similarity.
strip_bounds / compute_retrieval_counts_part: one strip of rows of the sharded validation; the sum over the strips is the whole."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

VALKEYS = ["r1", "r5", "r10", "r50", "medr", "meanr", "sum"]  # nntrainer/retrieval.py:12


def compute_retrieval_cosine(dot_product: np.ndarray) -> Tuple[Dict[str, float], np.ndarray, np.ndarray]:
    n = len(dot_product)
    order = np.argsort(dot_product, axis=1)[:, ::-1]
    ranks = np.argmax(order == np.arange(n)[:, None], axis=1).astype(np.float64)
    top1 = order[:, 0].astype(np.float64)
    r1, r5, r10, r50 = [float((ranks < k).mean()) for k in (1, 5, 10, 50)]
    medr = float(np.floor(np.median(ranks)) + 1)
    meanr = float(ranks.mean() + 1)
    return {"r1": r1, "r5": r5, "r10": r10, "r50": r50, "medr": medr, "meanr": meanr, "sum": r1 + r5 + r50}, top1, ranks


def compute_retrieval(emb1: np.ndarray, emb2: np.ndarray):
    d = np.dot(emb1, emb2.T)
    res1, _, _ = compute_retrieval_cosine(d)
    res2, _, _ = compute_retrieval_cosine(d.T)
    return res1, res2, (res1["r1"] + res2["r1"]) / 2


def compute_retrieval_topk(sim: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The k best columns of every row of sim [M, N], best first, and their scores: (idx int32 [M, k], scores [M, k]).  Order:
    score descending, then column descending — a stable ascending argsort reversed, the tie rule of the device ranks (a later
    index is ahead).  Column 0 is compute_retrieval_cosine's top1 wherever the row maximum is unique."""
    sim = np.asarray(sim)
    assert sim.ndim == 2 and 1 <= k <= sim.shape[1], (sim.shape, k)
    idx = np.argsort(sim, axis=1, kind="stable")[:, ::-1][:, :k]
    return idx.astype(np.int32), np.take_along_axis(sim, idx, axis=1)


def compute_retrieval_topk_masked(sim: np.ndarray, k: int, keep) -> Tuple[np.ndarray, np.ndarray]:
    """compute_retrieval_topk restricted to the columns with keep[j] != 0 (keep: [N] booleans or bytes): compute_retrieval_topk of
    sim[:, keep] with its columns mapped back through np.nonzero(keep).  1 <= k <= N whatever the mask holds; with c < k kept
    columns the slots r >= c of every row are idx = -1, score = -inf."""
    sim = np.asarray(sim)
    keep = np.asarray(keep)
    assert sim.ndim == 2 and 1 <= k <= sim.shape[1] and keep.shape == (sim.shape[1],), (sim.shape, k, keep.shape)
    cols = np.nonzero(keep)[0]
    c = min(int(k), len(cols))
    idx = np.full((sim.shape[0], k), -1, np.int32)
    scores = np.full((sim.shape[0], k), -np.inf, sim.dtype)
    if c:
        sub_idx, sub_scores = compute_retrieval_topk(sim[:, cols], c)
        idx[:, :c] = cols[sub_idx]
        scores[:, :c] = sub_scores
    return idx, scores


def compute_retrieval_topk_grouped(sim: np.ndarray, k: int, groups, num_groups: Optional[int] = None, keep=None):
    """The k best GROUPS of columns of every row of sim [M, N], each through its best column: (group int32 [M, k], idx int32 [M, k],
    scores [M, k]).  groups [N] integers: groups[j] is the group of column j; num_groups = G (None: max(groups) + 1).  Per row: the
    ranking of compute_retrieval_topk(sim, N) (score descending, then column descending) without the columns keep masks out (keep [N]
    booleans or bytes, None: none) and without those whose group id lies outside [0, G); the first column of every group stays, and
    the first k of those are the result.  1 <= k <= N whatever groups and keep hold; with fewer than k groups left the tail of a row is
    group -1, idx -1, score -inf.  groups = arange(N): idx and scores of compute_retrieval_topk_masked, group == idx."""
    sim = np.asarray(sim)
    groups = np.asarray(groups).astype(np.int64).reshape(-1)
    m, n = sim.shape
    assert sim.ndim == 2 and 1 <= k <= n and groups.shape == (n,), (sim.shape, k, groups.shape)
    g_total = max(int(groups.max()) + 1, 0) if num_groups is None else int(num_groups)
    ok = (groups >= 0) & (groups < g_total)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (n,), (keep.shape, n)
        ok &= keep != 0
    group = np.full((m, k), -1, np.int32)
    idx = np.full((m, k), -1, np.int32)
    scores = np.full((m, k), -np.inf, sim.dtype)
    order = np.argsort(sim, axis=1, kind="stable")[:, ::-1]
    for i in range(m):
        seen, r = set(), 0
        for j in order[i]:
            if r == k:
                break
            if ok[j] and groups[j] not in seen:
                seen.add(groups[j])
                group[i, r], idx[i, r], scores[i, r] = groups[j], j, sim[i, j]
                r += 1
    return group, idx, scores


def compute_retrieval_topk_scoped(sim: np.ndarray, k: int, groups, only=None, exclude=None, keep=None) -> Tuple[np.ndarray, np.ndarray]:
    """compute_retrieval_topk_masked with a mask of its own for every row of sim [M, N]: (idx int32 [M, k], scores [M, k]).  groups
    [N] integers: groups[j] is the id of column j (None: arange(N), every column its own id).  Exactly one of only / exclude is given,
    [M] integers, one id per row: column j is eligible for row i when keep[j] != 0 (keep [N] booleans or bytes, None: every column)
    and groups[j] == only[i], or groups[j] != exclude[i].  Integer equality, nothing else: an id that no column carries selects nothing
    under only (the whole row is idx -1, score -inf) and excludes nothing under exclude.  1 <= k <= N whatever the scopes hold; with
    fewer than k eligible columns the tail of a row is idx = -1, score = -inf."""
    sim = np.asarray(sim)
    assert sim.ndim == 2, sim.shape
    m, n = sim.shape
    assert (only is None) != (exclude is None), "exactly one of only / exclude"
    groups = np.arange(n) if groups is None else np.asarray(groups).astype(np.int64).reshape(-1)
    scope = np.asarray(exclude if only is None else only).astype(np.int64).reshape(-1)
    assert 1 <= k <= n and groups.shape == (n,) and scope.shape == (m,), (sim.shape, k, groups.shape, scope.shape)
    ok = np.ones(n, bool)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (n,), (keep.shape, n)
        ok = keep != 0
    idx = np.empty((m, k), np.int32)
    scores = np.empty((m, k), sim.dtype)
    for i in range(m):
        idx[i], scores[i] = compute_retrieval_topk_masked(sim[i:i + 1], k, ok & ((groups == scope[i]) == (only is not None)))
    return idx, scores


def compute_retrieval_topk_adjusted(sim: np.ndarray, offset, k: int, keep=None) -> Tuple[np.ndarray, np.ndarray]:
    """The k best columns of every row of sim [M, N] by a(i, j) = sim[i, j] - offset[j], one float32 subtraction: (idx int32 [M, k],
    scores float32 [M, k]), scores the values of a.  offset: [N] numbers, rounded to float32 once.  compute_retrieval_topk_masked of a
    under keep ([N] booleans or bytes), compute_retrieval_topk of a without it: a descending, then column descending; with fewer
    than k kept columns the tail is idx -1, score -inf.  offset +inf gives a = -inf, still a column (unlike a masked one); -inf puts
    the column first.  A NaN in a (inf - inf) is not modelled."""
    sim = np.asarray(sim)
    with np.errstate(over="ignore"):
        offset = np.asarray(offset).astype(np.float32)
    assert sim.ndim == 2 and sim.dtype == np.float32 and offset.shape == (sim.shape[1],), (sim.shape, sim.dtype, offset.shape)
    with np.errstate(invalid="ignore"):
        a = (sim - offset[None, :]).astype(np.float32)
    return compute_retrieval_topk(a, k) if keep is None else compute_retrieval_topk_masked(a, k, keep)


def compute_retrieval_hub_offsets(scores: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """The lists of compute_retrieval_knn_join (scores float32 [N, k], idx [N, k]: every row of a gallery against a bank of queries)
    into one offset per row, float32 [N].  Per row j: c = the number of slots with idx >= 0 (the filled ones, a prefix); c > 0: acc =
    0, acc += scores[j, t] for t = 0 .. c - 1 in that order in float32, out[j] = 0.5 * (acc / c) in float32; c == 0: out[j] = 0.  An
    explicit loop: np.sum and np.mean add pairwise.  With it as the offset compute_retrieval_topk_adjusted ranks by CSLS,
    2 s(i, j) - r_q(i) - r_g(j), for every query i."""
    scores, idx = np.asarray(scores), np.asarray(idx)
    assert scores.ndim == 2 and scores.dtype == np.float32 and idx.shape == scores.shape, (scores.shape, scores.dtype, idx.shape)
    out = np.zeros(scores.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(scores.shape[0]):
            c = int((idx[j] >= 0).sum())
            if c:
                acc = np.float32(0)
                for t in range(c):
                    acc = np.float32(acc + scores[j, t])
                out[j] = np.float32(0.5) * np.float32(acc / np.float32(c))
    return out


def compute_retrieval_range(sim: np.ndarray, threshold, keep=None, order: str = "row") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every column of sim [M, N] that scores at least the row's threshold: (offsets int64 [M + 1], rows int32 [T], scores [T]), CSR:
    the hits of row i are rows[offsets[i]:offsets[i + 1]] with scores = sim[i, rows], T = offsets[M].  threshold: one number or [M]
    numbers, rounded to float32 once.  Column j is a hit of row i when keep[j] != 0 (keep [N] booleans or bytes, None: every column)
    and sim[i, j] >= threshold[i], the IEEE compare: a NaN on either side is no hit, -0 >= +0 holds, -inf takes every kept column that
    is not a NaN, +inf only columns that are +inf.  order="row": a segment's columns ascend.  order="score": the order of
    compute_retrieval_topk_masked inside every segment, score descending (-0 as +0), then column descending."""
    sim = np.asarray(sim)
    assert sim.ndim == 2 and order in ("row", "score"), (sim.shape, order)
    m, n = sim.shape
    with np.errstate(over="ignore"):
        t = np.asarray(threshold).astype(np.float32)
    assert t.shape in ((), (m,)), (t.shape, m)
    t = np.broadcast_to(t, (m,))
    ok = np.ones(n, bool)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (n,), (keep.shape, n)
        ok = keep != 0
    offsets = np.zeros(m + 1, np.int64)
    segs = []
    for i in range(m):
        with np.errstate(invalid="ignore"):
            cols = np.nonzero(ok & (sim[i] >= t[i]))[0]
        if order == "score":  # ascending and stable, reversed: score, then column, descending (no NaN is a hit)
            cols = cols[np.argsort(sim[i, cols], kind="stable")[::-1]]
        segs.append(cols)
        offsets[i + 1] = offsets[i] + len(cols)
    rows = np.concatenate(segs).astype(np.int32) if segs else np.zeros(0, np.int32)
    scores = np.concatenate([sim[i, c] for i, c in enumerate(segs)]) if segs else np.zeros(0, sim.dtype)
    return offsets, rows, scores.astype(sim.dtype)


def compute_retrieval_self_join(sim: np.ndarray, threshold, keep=None, groups=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """All pairs of rows of a gallery at or above a threshold, from its similarities with itself, sim [N, N]: (offsets int64 [N + 1],
    rows int32 [T], scores [T]), the CSR of compute_retrieval_range read as pairs — the hits of row i are the rows j > i, ascending,
    with scores = sim[i, j]; every unordered pair appears once, under its smaller row.  threshold: one number or [N] numbers, rounded
    to float32 once.  Pair (i, j), i < j, is a hit when keep (bytes or booleans [N], None: every row) lets BOTH rows pass (a row that
    does not pass neither asks nor is returned: its segment is empty), groups is None or groups[i] != groups[j] (integers [N]), and
    sim[i, j] >= threshold[i], the IEEE compare of compute_retrieval_range.  Row i is compute_retrieval_range(sim[i:i + 1],
    threshold[i], keep=the rows j > i that are eligible for it)."""
    sim = np.asarray(sim)
    assert sim.ndim == 2 and sim.shape[0] == sim.shape[1], sim.shape
    n = sim.shape[0]
    with np.errstate(over="ignore"):
        t = np.asarray(threshold).astype(np.float32)
    assert t.shape in ((), (n,)), (t.shape, n)
    t = np.broadcast_to(t, (n,))
    ok = np.ones(n, bool)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (n,), (keep.shape, n)
        ok = keep != 0
    if groups is not None:
        groups = np.asarray(groups)
        assert groups.shape == (n,) and groups.dtype.kind in "iu", (groups.shape, groups.dtype)
    right = np.arange(n)
    offsets = np.zeros(n + 1, np.int64)
    rows, scores = [], []
    for i in range(n):
        el = ok & ok[i] & (right > i)
        if groups is not None:
            el &= groups != groups[i]
        _, r, s = compute_retrieval_range(sim[i:i + 1], t[i], keep=el)
        rows.append(r)
        scores.append(s)
        offsets[i + 1] = offsets[i] + len(r)
    return offsets, np.concatenate(rows).astype(np.int32), np.concatenate(scores).astype(sim.dtype)


def compute_retrieval_components(sim: np.ndarray, threshold, keep=None, groups=None) -> np.ndarray:
    """The connected components of a gallery under the pairs of compute_retrieval_self_join(sim, threshold, keep, groups), from its
    similarities with itself, sim [N, N]: labels int32 [N].  Pair (i, j), i < j, is an edge when keep lets BOTH rows pass, groups is
    None or groups[i] != groups[j], and sim[i, j] >= threshold[i], the IEEE compare (a NaN on either side is no edge, -0 >= +0 holds,
    -inf joins every kept pair that is not a NaN).  labels[i] is the smallest row number in row i's component; a row without an edge
    labels itself; a row that keep masks is -1 and is no vertex, so it does not connect its neighbours.  With groups two rows of one
    group are never joined directly, but may land in one component through a row of another group.  A plain host union-find over
    the hit definition: each root is linked below the smaller root, so a root is its set's smallest member."""
    offsets, rows, _ = compute_retrieval_self_join(sim, threshold, keep=keep, groups=groups)
    n = len(offsets) - 1
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        for j in rows[offsets[i]:offsets[i + 1]]:
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.array([find(i) for i in range(n)], np.int32).reshape(n)
    if keep is not None:
        labels[np.asarray(keep) == 0] = -1
    return labels


def compute_retrieval_join(sim: np.ndarray, threshold, keep=None, other_keep=None, groups=None,
                           other_groups=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """All pairs (row of a left gallery, row of a right one) at or above a threshold, from their similarities sim [M, N]: (offsets
    int64 [M + 1], rows int32 [T], scores [T]), the CSR of compute_retrieval_range read as pairs — the hits of left row i are the
    right rows rows[offsets[i]:offsets[i + 1]], ascending, with scores = sim[i, rows].  threshold: one number or [M] numbers, rounded
    to float32 once.  Pair (i, j) is a hit when keep (bytes or booleans [M], None: every row) lets left row i pass (a row that does
    not pass does not ask: its segment is empty), other_keep ([N]) lets right row j pass, groups and other_groups are both None or
    groups[i] != other_groups[j] (integers [M] and [N] in one id space; exactly one of them is an error), and sim[i, j] >=
    threshold[i], the IEEE compare of compute_retrieval_range.  Without filters it is compute_retrieval_range(sim, threshold)."""
    sim = np.asarray(sim)
    assert sim.ndim == 2, sim.shape
    m, n = sim.shape
    with np.errstate(over="ignore"):
        t = np.asarray(threshold).astype(np.float32)
    assert t.shape in ((), (m,)), (t.shape, m)
    t = np.broadcast_to(t, (m,))
    ask, ok = np.ones(m, bool), np.ones(n, bool)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (m,), (keep.shape, m)
        ask = keep != 0
    if other_keep is not None:
        other_keep = np.asarray(other_keep)
        assert other_keep.shape == (n,), (other_keep.shape, n)
        ok = other_keep != 0
    if (groups is None) != (other_groups is None):
        raise ValueError("compute_retrieval_join: groups and other_groups are given together or not at all")
    if groups is not None:
        groups, other_groups = np.asarray(groups), np.asarray(other_groups)
        assert groups.shape == (m,) and groups.dtype.kind in "iu", (groups.shape, groups.dtype)
        assert other_groups.shape == (n,) and other_groups.dtype.kind in "iu", (other_groups.shape, other_groups.dtype)
        groups, other_groups = groups.astype(np.int64), other_groups.astype(np.int64)
    offsets = np.zeros(m + 1, np.int64)
    rows, scores = [np.zeros(0, np.int32)], [np.zeros(0, sim.dtype)]
    for i in range(m):
        el = ok & ask[i]
        if groups is not None:
            el = el & (other_groups != groups[i])
        _, r, s = compute_retrieval_range(sim[i:i + 1], t[i], keep=el)
        rows.append(r)
        scores.append(s)
        offsets[i + 1] = offsets[i] + len(r)
    return offsets, np.concatenate(rows).astype(np.int32), np.concatenate(scores).astype(sim.dtype)


def compute_retrieval_knn_join(sim: np.ndarray, k: int, keep=None, other_keep=None, groups=None, other_groups=None,
                               exclude_same_row: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The k best partners of every row of a left gallery among the rows of a right one, from their similarities sim [M, N]: (idx
    int32 [M, k], scores [M, k]).  Pair (i, j) is eligible when keep (bytes or booleans [M], None: every row) lets left row i pass,
    other_keep ([N]) lets right row j pass, groups and other_groups are both None or groups[i] != other_groups[j] (integers [M] and
    [N] in one id space; exactly one of them is an error), and, with exclude_same_row, j != i (the self case, sim of a gallery with
    itself).  Row i holds the k best eligible columns in the order of compute_retrieval_topk, score descending, then column
    descending; fewer than k eligible columns leave a tail of idx -1, score -inf, and a row that keep masks is -1 / -inf in every
    slot: it does not ask.  1 <= k <= N whatever the filters hold.  Row i is compute_retrieval_topk_masked(sim[i:i + 1], k,
    eligible_i); with groups and no other filter it is compute_retrieval_topk_scoped(sim, k, other_groups, exclude=groups)."""
    sim = np.asarray(sim)
    assert sim.ndim == 2, sim.shape
    m, n = sim.shape
    assert 1 <= k <= n, (sim.shape, k)
    ask, ok = np.ones(m, bool), np.ones(n, bool)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (m,), (keep.shape, m)
        ask = keep != 0
    if other_keep is not None:
        other_keep = np.asarray(other_keep)
        assert other_keep.shape == (n,), (other_keep.shape, n)
        ok = other_keep != 0
    if (groups is None) != (other_groups is None):
        raise ValueError("compute_retrieval_knn_join: groups and other_groups are given together or not at all")
    if groups is not None:
        groups, other_groups = np.asarray(groups), np.asarray(other_groups)
        assert groups.shape == (m,) and groups.dtype.kind in "iu", (groups.shape, groups.dtype)
        assert other_groups.shape == (n,) and other_groups.dtype.kind in "iu", (other_groups.shape, other_groups.dtype)
        groups, other_groups = groups.astype(np.int64), other_groups.astype(np.int64)
    cols = np.arange(n)
    idx = np.empty((m, k), np.int32)
    scores = np.empty((m, k), sim.dtype)
    for i in range(m):
        el = ok & ask[i]
        if groups is not None:
            el = el & (other_groups != groups[i])
        if exclude_same_row:
            el = el & (cols != i)
        idx[i], scores[i] = compute_retrieval_topk_masked(sim[i:i + 1], k, el)
    return idx, scores


def _host_offsets(fn: str, offsets, m: int, exc=ValueError) -> np.ndarray:
    """The offsets of a multi-vector search as int64 [P + 1], checked on the host: a sequence, numpy array or CPU integer tensor of at
    least 2 entries, the first 0, the last M, none smaller than the one before it."""
    if hasattr(offsets, "is_cuda"):
        if offsets.is_cuda:
            raise exc(f"{fn}: offsets live on the host (a sequence, a numpy array or a CPU integer tensor), not on {offsets.device}")
        offsets = offsets.numpy()
    try:
        off = np.asarray(offsets)
    except Exception:
        off = np.asarray(None)
    if off.ndim != 1 or off.dtype.kind not in "iu" or off.size < 2:
        raise exc(f"{fn}: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
                  f"queries[offsets[p]:offsets[p + 1]]), not {type(offsets).__name__} of dtype {off.dtype} and shape {off.shape}")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != m:
        raise exc(f"{fn}: offsets runs from {off[0]} to {off[-1]}; it has to start at 0 and end at M = {m}")
    if (np.diff(off) < 0).any():
        raise exc(f"{fn}: offsets decreases at entry {int(np.argmax(np.diff(off) < 0)) + 1}; it has to be non-decreasing")
    return off


def compute_retrieval_topk_multi(sim: np.ndarray, offsets, k: int, groups, num_groups: Optional[int] = None, keep=None):
    """The k best GROUPS of columns for every PARAGRAPH of rows of sim [M, N] (MaxSim, late interaction): paragraph p is the rows
    offsets[p] .. offsets[p + 1] - 1 (offsets: P + 1 integers from 0 to M, non-decreasing; a paragraph may be empty).  Returns (group
    int32 [P, k], scores [P, k], rows int32 [M, k], row_scores [M, k]).  groups, num_groups = G and keep as in
    compute_retrieval_topk_grouped, and so is the entry of row i in group g: the first column of g in the ranking of row i (score
    descending, then column descending) without the columns keep masks out and those with an id outside [0, G); its score is sim[i, j]
    with -0 as +0.  Group g is a candidate for paragraph p if p is not empty and every row of p has an entry in g; its score is s = +0,
    then s = s + score(i, g) for the rows of p in order — float32 adds in exactly that order; candidates are ordered by score
    descending, then GROUP id descending (the grouped search orders by row; a paragraph has no single row).  group, scores: the first k
    candidates, the tail -1 / -inf.  rows, row_scores, the alignment: for row i of paragraph p, slot r holds the entry of i in
    group[p, r], -1 / -inf where group[p, r] is -1.  1 <= k <= N whatever groups and keep hold."""
    sim = np.asarray(sim)
    groups = np.asarray(groups).astype(np.int64).reshape(-1)
    assert sim.ndim == 2, sim.shape
    m, n = sim.shape
    assert 1 <= k <= n and groups.shape == (n,), (sim.shape, k, groups.shape)
    off = _host_offsets("compute_retrieval_topk_multi", offsets, m, exc=AssertionError)
    g_total = max(int(groups.max()) + 1, 0) if num_groups is None else int(num_groups)
    ok = (groups >= 0) & (groups < g_total)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (n,), (keep.shape, n)
        ok &= keep != 0
    # the table: entry of (row i, group g), -1 = none
    best = np.full((m, g_total), -1, np.int64)
    score = np.zeros((m, g_total), sim.dtype)
    order = np.argsort(sim, axis=1, kind="stable")[:, ::-1]
    for i in range(m):
        o = order[i][ok[order[i]]]
        first_g, first_at = np.unique(groups[o], return_index=True)
        best[i, first_g] = o[first_at]
        score[i, first_g] = sim[i, o[first_at]] + sim.dtype.type(0)  # -0 -> +0
    p_total = len(off) - 1
    group = np.full((p_total, k), -1, np.int32)
    scores = np.full((p_total, k), -np.inf, sim.dtype)
    rows = np.full((m, k), -1, np.int32)
    row_scores = np.full((m, k), -np.inf, sim.dtype)
    for p in range(p_total):
        i0, i1 = int(off[p]), int(off[p + 1])
        if i1 == i0:
            continue
        cand = np.nonzero((best[i0:i1] >= 0).all(axis=0))[0]
        s = np.zeros(g_total, sim.dtype)
        for i in range(i0, i1):  # one add per sentence, in order: np.sum and np.add.reduce add pairwise
            s = s + score[i]
        top = cand[np.argsort(s[cand], kind="stable")[::-1][:k]]  # ascending and stable, reversed: score, then group id, descending
        c = len(top)
        group[p, :c], scores[p, :c] = top, s[top]
        rows[i0:i1, :c], row_scores[i0:i1, :c] = best[i0:i1][:, top], score[i0:i1][:, top]
    return group, scores, rows, row_scores


def _ahead(s, idx, t, a):
    """The device tie rule: entry (s, idx) is ahead of (t, a) when it is larger, or equal with a later index."""
    return (s > t) | ((s == t) & (idx > a))


def _labeled_metrics(ranks: np.ndarray) -> Tuple[Dict[str, float], np.ndarray]:
    """The seven metrics over the entries >= 0 of a rank vector, in the fp32 / fp64 steps of the device kernel, as a dictionary
    and as the float32 [7] the device writes (n == 0: zeros)."""
    r = ranks[ranks >= 0].astype(np.int64)
    n = len(r)
    out = np.zeros(7, np.float32)
    if n:
        nf = np.float32(n)
        r1, r5, r10, r50 = [np.float32((r < k).sum()) / nf for k in (1, 5, 10, 50)]
        r = np.sort(r)
        med = 0.5 * (np.float64(r[(n - 1) // 2]) + np.float64(r[n // 2]))
        out[:] = [r1, r5, r10, r50, np.float32(np.floor(med) + 1.0), np.float32(np.float64(r.sum()) / np.float64(n) + 1.0), (r1 + r5) + r50]
    return {k: float(v) for k, v in zip(VALKEYS, out)}, out


def compute_retrieval_labeled(sim: np.ndarray, labels: np.ndarray):
    """Host mirror of coot_retrieval_ranks_labeled on a similarity matrix sim [M, N] (queries x gallery): labels[i] is the gallery
    row of query i; a label outside [0, N) means "no ground truth" (rank -1, in neither direction's ranks or metrics).  Returns
    (res_q2g, res_g2q, ranks_q int32 [M], ranks_g int32 [N]).
    ranks_q[i] = the entries (s[i, j], j), j != g, ahead of (s[i, g], g), g = labels[i]: the position of g in
    np.argsort(sim[i], kind="stable")[::-1].  ranks_g[j] = the entries (s[i', j], i') of column j ahead of the column's best
    positive, the query with labels[i] == j that is ahead of the other ones: the minimum over the column's ground-truth queries of
    their position in np.argsort(sim[:, j], kind="stable")[::-1]; -1 for gallery rows without a valid query.  The metric
    dictionaries (VALKEYS) are taken over the valid entries of each direction (n == 0: zeros)."""
    sim = np.asarray(sim)
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    m, n = sim.shape
    assert labels.shape == (m,), (sim.shape, labels.shape)
    valid = (labels >= 0) & (labels < n)
    ranks_q, ranks_g = np.full(m, -1, np.int32), np.full(n, -1, np.int32)
    cols = np.arange(n)
    for i in np.nonzero(valid)[0]:
        g = labels[i]
        ranks_q[i] = ((cols != g) & _ahead(sim[i], cols, sim[i, g], g)).sum()
    rows = np.arange(m)
    for j in np.unique(labels[valid]):
        col = sim[:, j]
        t, a = None, -1
        for i in np.nonzero(valid & (labels == j))[0]:  # ascending i: an equal score with a later index is ahead
            if t is None or col[i] >= t:
                t, a = col[i], i
        ranks_g[j] = _ahead(col, rows, t, a).sum()
    res_q, _ = _labeled_metrics(ranks_q)
    res_g, _ = _labeled_metrics(ranks_g)
    return res_q, res_g, ranks_q, ranks_g


def compute_retrieval_labeled_adjusted(sim: np.ndarray, labels: np.ndarray, col_offset=None, row_offset=None):
    """Host mirror of coot_retrieval_ranks_adjusted: compute_retrieval_labeled of the adjusted matrix a, with sim float32 [M, N],
    col_offset [N] and row_offset [M] numbers (rounded to float32 once) or None.  a = sim without offsets; a = sim - col[None, :] with
    col_offset; then a = a - row[:, None] with row_offset: one float32 subtraction each, the column's first.  col_offset is the offset
    of compute_retrieval_topk_adjusted: with it alone ranks_q[i] is the position of labels[i] in compute_retrieval_topk_adjusted(sim,
    col_offset, N)[0][i].  An offset of +inf leaves a = -inf: such a column is still a column and still a valid label.  A NaN in a
    (inf - inf) is not modelled.  Returns (res_q2g, res_g2q, ranks_q int32 [M], ranks_g int32 [N])."""
    sim = np.asarray(sim)
    assert sim.ndim == 2 and sim.dtype == np.float32, (sim.shape, sim.dtype)
    a = sim
    with np.errstate(over="ignore", invalid="ignore"):
        if col_offset is not None:
            col = np.asarray(col_offset).astype(np.float32)
            assert col.shape == (sim.shape[1],), (sim.shape, col.shape)
            a = (a - col[None, :]).astype(np.float32)
        if row_offset is not None:
            row = np.asarray(row_offset).astype(np.float32)
            assert row.shape == (sim.shape[0],), (sim.shape, row.shape)
            a = (a - row[:, None]).astype(np.float32)
    return compute_retrieval_labeled(a, labels)


def strip_bounds(n: int, world: int, rank: int) -> Tuple[int, int]:
    """(row0, rows) of rank's strip of n rows: an even split over the ranks, the remainder to the first ranks."""
    base, rem = divmod(int(n), int(world))
    return rank * base + min(rank, rem), base + (1 if rank < rem else 0)


def compute_retrieval_counts_part(sim: np.ndarray, row0: int, rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of coot_retrieval_ranks_part on a similarity matrix sim [N, N]: (counts_12, counts_21) int32 [N] of the strip
    of rows [row0, row0 + rows).  counts_12[i] = the entries of row i ahead of sim[i, i] (strip rows only, 0 elsewhere),
    counts_21[j] = the strip's entries of column j ahead of sim[j, j]; "ahead" = larger, or equal with a later index (the device
    tie rule).  Summed over the strips of any partition of [0, N) they are the two rank vectors."""
    sim = np.asarray(sim)
    n = sim.shape[0]
    assert sim.shape == (n, n) and 0 <= row0 and 0 <= rows and row0 + rows <= n, (sim.shape, row0, rows)
    c12, c21 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    if rows == 0:
        return c12, c21
    diag = np.diagonal(sim)
    s = sim[row0:row0 + rows]
    i, j = np.arange(row0, row0 + rows)[:, None], np.arange(n)[None, :]
    di, dj = diag[row0:row0 + rows, None], diag[None, :]
    off = i != j
    c12[row0:row0 + rows] = (off & ((s > di) | ((s == di) & (j > i)))).sum(axis=1)
    c21[:] = (off & ((s > dj) | ((s == dj) & (i > j)))).sum(axis=0)
    return c12, c21
