"""Decision-separated inputs, a rounding-exact fp64 reference and the case table of the loss-kernel tests
(tests/test_gpu_loss_kernels.py, tests/test_cpu_loss_cases.py, tools/gen_loss_tolerances.py).

Inputs.  make_pair() draws two sets (a, b) of N rows whose hinge decisions are all far from their threshold: rows belong to K
clusters with centres sqrt(rho) q0 + sqrt(1 - rho) q_c (orthonormal q), a_i = centre + eta u, b_i = a_i + eps u' (u, u' random unit
vectors), every row scaled by its own exp(U(-2, 2)).  With rho = 0.5, eta = 0.3, eps = 0.1 and margin 0.2 a same-cluster pair
violates the margin by ~+0.12 and a cross-cluster pair misses it by ~-0.3, in the alignment term and in both cluster terms.
contrastive_case() asserts |margin + S_ij - S_ii| >= MIN_GAP for every off-diagonal entry of every term it hands out.

Reference.  contrastive_ref() is numpy fp64 that rounds only where csrc/loss_fused.hip rounds: the inverse norm in float32 (with the
kernels' own order of additions, kernel_inv()), the row bf16(x * inv), then S, the diagonals, the hinge sums, G, G.Y and the
-(c1 + c1') diagonal term in fp64 on those bf16 values, and F.normalize backward on the unrounded x * inv as cl_finish does.
mode="exact" is the plain fp64 loss (what coot_contrastive_fwd_bwd_f32 computes).  Because no decision is near its threshold, a
kernel and this reference differ by fp32 round-off only; tools/gen_loss_tolerances.py measures how much that is per case.
"""
import zlib

import numpy as np

from oracle import coot_oracle as O

MARGIN = 0.2
MIN_GAP = 0.02
SET_NAMES = ("vid_emb", "par_emb", "clip_emb", "sent_emb", "vid_context", "par_context")
W_ALL = dict(weight_high=1.0, weight_high_internal=1.0, weight_low=1.0, weight_low_internal=1.0, weight_context=1.0,
             weight_context_internal=0.0)
W_FULL = dict(W_ALL, weight_context_internal=1.0)  # all nine terms


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def clusters_for(N, d):
    return int(min(d - 1, 60, max(1, round(np.sqrt(N)))))


def make_pair(N, d, seed, K=None, rho=0.5, eta=0.3, eps=0.1):
    rs = np.random.RandomState(seed)
    K = clusters_for(N, d) if K is None else K
    assert 1 <= K <= d - 1
    Q, _ = np.linalg.qr(rs.randn(d, K + 1))
    Q = Q.T
    centres = np.sqrt(rho) * Q[0] + np.sqrt(1 - rho) * Q[1:]
    c = rs.randint(0, K, size=N)

    def unit(n):
        z = rs.randn(n, d)
        return z / np.linalg.norm(z, axis=1, keepdims=True)

    a = centres[c] + eta * unit(N)
    b = a + eps * unit(N)
    sa, sb = np.exp(rs.uniform(-2, 2, size=(N, 1))), np.exp(rs.uniform(-2, 2, size=(N, 1)))  # the kernels normalise: norms must differ
    return (a * sa).astype(np.float32), (b * sb).astype(np.float32)


# ---- reference ------------------------------------------------------------------------------------------------------------------
def kernel_inv(x):
    """1 / max(||x||, 1e-12) in float32 with the additions of cl_norm_kernel / cl_small_kernel: lane l of a wave owns the 4-element
    chunks l, l + 64, ..., adds its squares by fma in element order, then the xor butterfly 32, 16, ..., 1 (d % 4 == 0, d <= 1024)."""
    x = np.asarray(x, np.float32)
    N, d = x.shape
    assert d % 4 == 0 and d <= 1024
    xp = np.zeros((N, 1024), np.float32)
    xp[:, :d] = x
    xq = xp.reshape(N, 4, 64, 4)
    s = np.zeros((N, 64), np.float32)
    for q in range(4):
        for j in range(4):
            v = xq[:, q, :, j].astype(np.float64)
            s = (v * v + s.astype(np.float64)).astype(np.float32)  # fmaf: the product of two floats is exact in fp64
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return (np.float32(1) / np.maximum(np.sqrt(s[:, 0]), np.float32(1e-12))).astype(np.float32)


def _mm(A, Bt, seq):
    """A [n, k] . Bt [k, m].  seq: one rank-1 update per k in DESCENDING k, every operation an IEEE one of A's dtype (no BLAS: the
    float32 mirror must give the same bits on every machine, and in an order no kernel uses)."""
    if not seq:
        return A @ Bt
    out = np.zeros((A.shape[0], Bt.shape[1]), A.dtype)
    for k in range(A.shape[1] - 1, -1, -1):
        out += A[:, k, None] * Bt[k][None, :]
    return out


def hinge_term(A, B, margin, seq=False):
    """One ContrastiveLoss term on normalised rows (coot/loss_fn.py:63-100, unscaled).  Returns per-row hinge sums
    (sum_j max(0, m + S_ij - S_ii) + max(0, m + S_ij - S_jj), j != i), d/dA, d/dB and the smallest |m + S_ij - S_ii| off the
    diagonal.  Computes in the dtype of A."""
    N = A.shape[0]
    m = A.dtype.type(margin)
    S = _mm(A, np.ascontiguousarray(B.T), seq)
    dg = np.diag(S).copy()
    off = ~np.eye(N, dtype=bool)
    cs = m + S - dg[:, None]
    ci = m + S - dg[None, :]
    gap = float(min(np.abs(cs[off]).min(), np.abs(ci[off]).min())) if N > 1 else float("inf")
    ms, mi = (cs > 0) & off, (ci > 0) & off
    hs = np.where(ms, cs, 0) + np.where(mi, ci, 0)
    rows = (hs[:, ::-1] if seq else hs).sum(1, dtype=A.dtype)
    G = ms.astype(A.dtype) + mi.astype(A.dtype)
    diag = (ms.sum(1) + mi.sum(0)).astype(A.dtype)  # c1(A, B) + c1(B, A)
    dA = _mm(G, B, seq) - diag[:, None] * B
    dB = _mm(np.ascontiguousarray(G.T), A, seq) - diag[:, None] * A
    return rows, dA, dB, gap


def pair_weights(w):
    """(alignment, cluster) weight of the pairs (high, low, context); the context cluster term is switched by
    weight_context_internal and weighted by weight_low_internal (coot/trainer_retrieval.py:181), with the 1/2 of compute_cluster_loss."""
    return ([w["weight_high"], w["weight_low"], w["weight_context"]],
            [0.5 * w["weight_high_internal"], 0.5 * w["weight_low_internal"],
             0.5 * w["weight_low_internal"] if w["weight_context_internal"] != 0 else 0.0])


def contrastive_ref(sets, w, margin=MARGIN, mode="bf16", dtype=np.float64, inv_ulp=0, seq=False):
    """sets: the six un-normalised float32 sets in SET_NAMES order.  Returns a dict: loss, loss_pair [3], grads [6] (zeros for a
    pair without weights), rows [3] (per-row share of the loss of each pair: rows[p].sum() == loss_pair[p]) and gap."""
    w_pair, w_self = pair_weights(w)
    out = dict(loss_pair=[], grads=[None] * 6, rows=[], gap=float("inf"))
    for p in range(3):
        xs = [np.asarray(sets[2 * p], np.float32), np.asarray(sets[2 * p + 1], np.float32)]
        N = xs[0].shape[0]
        if mode == "bf16":
            invs = [kernel_inv(x) for x in xs]
            if inv_ulp:
                invs = [np.nextafter(i, np.float32(np.inf * inv_ulp)) for i in invs]
            unr = [(x * i[:, None]).astype(np.float32) for x, i in zip(xs, invs)]  # fp32 product, as the kernels
            nrm = [O.bf16_round(u).astype(dtype) for u in unr]
            unr = [u.astype(dtype) for u in unr]
            invs = [i.astype(dtype) for i in invs]
        else:
            xd = [x.astype(dtype) for x in xs]
            invs = [1 / np.maximum(np.sqrt((x * x).sum(1)), dtype(1e-12)) for x in xd]
            unr = [x * i[:, None] for x, i in zip(xd, invs)]
            nrm = unr
        d = [np.zeros_like(nrm[0]), np.zeros_like(nrm[1])]
        rows = np.zeros(N, dtype)
        n2 = dtype(N) * dtype(N)
        if w_pair[p] != 0:
            r, dA, dB, gap = hinge_term(nrm[0], nrm[1], margin, seq)
            c = dtype(w_pair[p]) / n2
            rows += c * r; d[0] += c * dA; d[1] += c * dB
            out["gap"] = min(out["gap"], gap)
        if w_self[p] != 0:
            for s in range(2):
                r, dA, dB, gap = hinge_term(nrm[s], nrm[s], margin, seq)
                c = dtype(w_self[p]) / n2
                rows += c * r; d[s] += c * (dA + dB)
                out["gap"] = min(out["gap"], gap)
        for s in range(2):  # F.normalize backward on the unrounded rows
            dot = (unr[s] * d[s]).sum(1, keepdims=True)
            out["grads"][2 * p + s] = (d[s] - unr[s] * dot) * invs[s][:, None]
        out["rows"].append(rows)
        out["loss_pair"].append(rows.sum())
    out["loss"] = sum(out["loss_pair"])
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def contrastive_case(cid, nh, dh, nl, dl, w=None, mode="bf16"):
    """The six sets of case `cid` (seeded by its name) + its reference.  A draw with a hinge decision closer than MIN_GAP to its
    threshold is not handed out: the next seed is drawn (at most 8), and a case that never separates is an error."""
    w = dict(W_FULL if w is None else w)
    wt = W_FULL  # the gap condition covers all nine terms, whatever the case switches on
    for k in range(8):
        s = _seed(cid) + 7919 * k
        sets = [*make_pair(nh, dh, s), *make_pair(nl, dl, s + 1), *make_pair(nh, dl, s + 2)]
        ref = contrastive_ref(sets, wt, mode=mode)
        if ref["gap"] >= MIN_GAP:
            break
    assert ref["gap"] >= MIN_GAP, f"{cid}: smallest hinge gap {ref['gap']:.4f} < {MIN_GAP}: broken case"
    if w != wt:
        gap = ref["gap"]
        ref = contrastive_ref(sets, w, mode=mode)
        ref["gap"] = gap
    return sets, w, ref


# cl_small_smem() of csrc/loss_fused.hip, restated: LDS bytes of a one-launch workgroup (Y rows + 16 X rows, pitch d + 8, the G strip
# [16][kw + 8] in 16-bit words, the diagonal in fp32) against the 150 KB the launch may ask for; at most 128 padded rows.
def small_path_fits(N, d):
    Np = (N + 15) & ~15
    kw = (Np + 31) & ~31
    return 0 < N and Np <= 128 and ((Np + 16) * (d + 8) + 16 * (kw + 8)) * 2 + Np * 4 <= 150 * 1024


def largest_small_n(d):
    return max(n for n in range(1, 129) if small_path_fits(n, d))


TEMPLATE_D = (32, 256, 288, 512, 544, 768, 800, 1024)
TEMPLATE_N = (1, 2, 15, 16, 17, 100, 128)
SPLIT_N = (496, 497, 512, 513, 767, 769, 2047, 2049, 4100)
DUMMY_LOW = (16, 32)  # a low pair that is not part of a call (part = COOT_CONTRASTIVE_GLOBAL)
W_CASES = {
    "align_only": dict(W_ALL, weight_high_internal=0.0, weight_low_internal=0.0),
    "cluster_only": dict(weight_high=0.0, weight_low=0.0, weight_context=0.0, weight_high_internal=1.0, weight_low_internal=1.0,
                         weight_context_internal=1.0),
    "ctx_internal_quirk": dict(W_ALL, weight_low_internal=0.7, weight_context_internal=0.3),
    "high_pair_off": dict(W_ALL, weight_high=0.0, weight_high_internal=0.0),
}


def contrastive_cases():
    """id -> (nh, dh, nl, dl, weights or None).  One reference serves every `part` of a case: the pairs share nothing but the
    loss word, so the reference of part p is the pairs of p."""
    C = {}
    nd = len(TEMPLATE_D)
    for i, d in enumerate(TEMPLATE_D):  # template selection (d) x padding rows (N); the low / context pairs walk the lists too
        for j, n in enumerate(TEMPLATE_N):
            C[f"tmpl_n{n}_d{d}"] = (n, d, TEMPLATE_N[(j + 3) % len(TEMPLATE_N)], TEMPLATE_D[(i + 3) % nd], W_FULL)
    nmax = largest_small_n(1024)
    for n, d in ((128, 384), (129, 384), (nmax, 1024), (nmax + 1, 1024)):  # the one-launch / three-launch boundary
        C[f"bound_n{n}_d{d}"] = (n, d, *DUMMY_LOW, None)
    C["mixed_small_high_large_low"] = (64, 768, 230, 384, W_FULL)
    for n in SPLIT_N:  # column splits by size
        C[f"split_n{n}_d64"] = (n, 64, *DUMMY_LOW, None)
        if n <= 2049:
            C[f"split_n{n}_d384"] = (n, 384, *DUMMY_LOW, None)
    C["forced_n300_d64"] = (300, 64, *DUMMY_LOW, None)
    C["forced_n40_d128"] = (40, 128, *DUMMY_LOW, None)
    for n in (50, 700):  # load clamps of cl_half: 12 k-blocks / 24 fragments exactly, one more, and the widest row
        for d in (384, 416, 1024):
            C[f"clamp_n{n}_d{d}"] = (n, d, *DUMMY_LOW, None)
    for k, w in W_CASES.items():
        C[f"w_{k}"] = (40, 256, 90, 128, w)
    C["dp_h70_l333"] = (70, 128, 333, 64, W_FULL)
    C["dp_h600_l1500"] = (600, 128, 1500, 64, W_FULL)
    return C


F32_CASES = {f"f32_n{n}_d{d}": (n, d, nl, dl) for n, d, nl, dl in
             ((1, 32, 17, 256), (17, 288, 2, 32), (100, 1024, 128, 544), (129, 384, 50, 416), (300, 64, 513, 64), (64, 768, 230, 384))}

CYCLE_SHAPES = ((64, 64, 384), (64, 1, 32), (1, 64, 1024), (7, 5, 100), (33, 20, 1000), (5, 9, 768))
CYCLE_B = (1, 9)
CYCLE_WEIGHT = 0.01


def cycle_case(Cc, Cs, D, B):
    """clip [B, Cc, D], sent [B, Cs, D] (zero padded), lengths (1 and the full width among them), sampled positions (first, last and
    a middle valid one).  Positions lie along a per-video direction so that the soft nearest neighbours are neither uniform nor
    one-hot: -mean_d (clip_i - sent_j)^2 ~ -(9 (i / Cc - j / Cs)^2 + 0.5)."""
    rs = np.random.RandomState(_seed(f"cycle_{Cc}_{Cs}_{D}_{B}"))
    u = rs.randn(B, 1, D)
    clip = (np.arange(Cc)[None, :, None] / Cc) * 3 * u + 0.5 * rs.randn(B, Cc, D)
    sent = (np.arange(Cs)[None, :, None] / Cs) * 3 * u + 0.5 * rs.randn(B, Cs, D)
    lc, ls = rs.randint(1, Cc + 1, size=B), rs.randint(1, Cs + 1, size=B)
    lc[0], ls[0] = Cc, Cs
    if B > 1:
        lc[1], ls[1] = 1, Cs
        lc[2], ls[2] = Cc, 1
    else:
        lc[0] = 1 if (Cc + Cs + D) % 2 and Cs > 1 else Cc  # the single-video cases alternate between one valid clip and the full width
    cv, sv = np.arange(Cc)[None, :] < lc[:, None], np.arange(Cs)[None, :] < ls[:, None]
    clip[~cv] = 0
    sent[~sv] = 0
    pick = lambda n, b: (0, n - 1, n // 2)[b % 3]
    ic = np.array([pick(lc[b], b) for b in range(B)], np.int64)
    isent = np.array([pick(ls[b], b + 1) for b in range(B)], np.int64)
    return dict(clip=clip.astype(np.float32), sent=sent.astype(np.float32), lc=lc.astype(np.int64), ls=ls.astype(np.int64), cv=cv, sv=sv,
                ic=ic, isent=isent)


def cycle_ref(c, dtype=np.float64):
    clip, sent = c["clip"].astype(dtype), c["sent"].astype(dtype)
    rc = O.cycle_consistency_rows(clip, c["cv"], sent, c["sv"])
    rsent = O.cycle_consistency_rows(sent, c["sv"], clip, c["cv"])
    lcl, lse = O.cycle_consistency_loss(clip, c["cv"], sent, c["sv"], c["ic"], c["isent"])
    dc, ds = O.cycle_consistency_bwd(clip, c["cv"], sent, c["sv"], c["ic"], c["isent"], dtype(CYCLE_WEIGHT))
    return dict(loss=dtype(CYCLE_WEIGHT) * (lcl + lse), rows_clip=rc, rows_sent=rsent, dclip=dc, dsent=ds)


# ---- distances and tolerances (tools/gen_loss_tolerances.py writes them, tests/test_cpu_loss_cases.py regenerates three) ---------
TOL_FLOOR = 1e-6
FACTOR = 4        # summation orders neither mirror reproduces: MFMA accumulation, up to eight column-split partials
CYCLE_FACTOR = 8  # cyclecons_kernel: __expf is the dominant term and the float32 mirror's exp is correctly rounded


def rel_max(x, ref):
    """max |x - ref| relative to max |ref| (0 where both are all-zero)."""
    den = float(np.abs(ref).max()) if np.size(ref) else 0.0
    num = float(np.abs(np.asarray(x, np.float64) - np.asarray(ref, np.float64)).max()) if np.size(ref) else 0.0
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def _dist(x, ref):
    """(loss, grads, rows) distances of a recomputation from the reference: the loss relative to the reference (per pair and in
    total, the largest), each gradient set and each pair's per-row loss shares relative to max |reference|, the largest."""
    dl = max([abs(float(x["loss"]) - float(ref["loss"])) / abs(float(ref["loss"])) if ref["loss"] != 0 else 0.0] +
             [abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(x["loss_pair"], ref["loss_pair"]) if b != 0])
    return dl, max(rel_max(a, b) for a, b in zip(x["grads"], ref["grads"])), max(rel_max(a, b) for a, b in zip(x["rows"], ref["rows"]))


def contrastive_tolerances(cid, nh, dh, nl, dl, w, mode="bf16"):
    """4 x max(a, b), floored: (a) the float32 mirror of the reference (every sum in float32, descending order), (b) the reference
    with every inverse norm one float32 ulp up / down (bf16 mode only: a few bf16 roundings flip)."""
    sets, w, ref = contrastive_case(cid, nh, dh, nl, dl, w, mode)
    a = _dist(contrastive_ref(sets, w, mode=mode, dtype=np.float32, seq=True), ref)
    b = (0.0, 0.0, 0.0)
    if mode == "bf16":
        bs = [_dist(contrastive_ref(sets, w, mode=mode, inv_ulp=u), ref) for u in (1, -1)]
        b = tuple(max(x[i] for x in bs) for i in range(3))
    tol = [max(FACTOR * max(a[i], b[i]), TOL_FLOOR) for i in range(3)]
    return dict(loss=tol[0], grad=tol[1], rows=tol[2], a_loss=a[0], a_grad=a[1], a_rows=a[2], b_loss=b[0], b_grad=b[1], b_rows=b[2],
                gap=ref["gap"])


def cycle_tolerances(Cc, Cs, D, B):
    c = cycle_case(Cc, Cs, D, B)
    ref, m = cycle_ref(c), cycle_ref(c, np.float32)
    assert ref["loss"] > 0, "a cycle case without loss checks nothing"
    a_loss = abs(float(m["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    a_rows = max(rel_max(m[k], ref[k]) for k in ("rows_clip", "rows_sent"))
    a_grad = max(rel_max(m[k], ref[k]) for k in ("dclip", "dsent"))
    return dict(loss=max(CYCLE_FACTOR * a_loss, TOL_FLOOR), rows=max(CYCLE_FACTOR * a_rows, TOL_FLOOR), grad=max(CYCLE_FACTOR * a_grad, TOL_FLOOR),
                a_loss=a_loss, a_rows=a_rows, a_grad=a_grad)


def all_tolerances(only=None, log=None):
    out = {}
    jobs = [(k, lambda v=v, k=k: contrastive_tolerances(k, *v)) for k, v in contrastive_cases().items()]
    jobs += [(k, lambda v=v, k=k: contrastive_tolerances(k, *v, W_FULL, "exact")) for k, v in F32_CASES.items()]
    jobs += [(f"cycle_{s[0]}_{s[1]}_{s[2]}_b{B}", lambda s=s, B=B: cycle_tolerances(*s, B)) for s in CYCLE_SHAPES for B in CYCLE_B]
    for k, f in jobs:
        if only is None or k in only:
            out[k] = f()
            if log:
                log(k, out[k])
    return out


REGENERATED_ON_CPU = ("tmpl_n17_d288", "w_ctx_internal_quirk", "cycle_7_5_100_b9")
