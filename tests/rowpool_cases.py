"""Case table, fp64 references, derived per-element bounds and the checker of the row-wise and pooling kernel tests
(tests/test_gpu_rowpool.py runs the kernels of csrc/rowops.hip and csrc/pool.hip through the coot_debug_* entries,
tests/test_cpu_rowpool_cases.py tests this module without a GPU).

Operations (a case has an "op"; x16 = a 16-bit operand, bf16 or IEEE half as the build has it):
  ln_fwd    y = gain (x - mean) / (std + eps) + bias (+ pe[row % pe_L]) times the keep-scale M[row D + col]; std unbiased, eps = fp32(1e-6)
  ln_bwd    dye = (dy + dy_add) M;  h = dye gain;  dx = (h - mean h) / s - xc <h, xc> / (s^2 (D - 1) std), second term 0 where std == 0;
            dxm = dx Mm[row dxm_drop_ld + col];  dgain += sum_r dye xc / s;  dbias += sum_r dye;  dxcolsum += sum_r dxm (dx without dxm)
  pool_fwd  GenPool: per sequence and channel, scores of the rows >= len are -32752; mx = max, ssum = sum_l exp(s - mx),
            pooled = sum_l exp(s_l - mx) Mw_l z_l / ssum; the hand-over pk_out / pk_mask / pk_lens = pack_by_count(pooled)
  pool_bwd  w = exp(s - smax) / ssum;  ds = w (g z Mw - g pooled) Ms;  dz = g w Mw;  padded rows 0;  ds_colsum += sum_rows ds
  avg_fwd   out = sum over ALL L rows of z / len;   avg_bwd  dz[every one of the L rows] = dpooled / len
  pack_fwd / pack_bwd / pack_join   pack_by_count / unpack_by_count, the join adds dout2 and a context gradient
  colsum    out += sum_r x[r]
The keep-scales (0 or 1 / keep) come from the library's own host generator coot_debug_dropout_scales.

Two references.  mode "exact" is the operation in fp64 on the operands as stored; the kernels are checked against it.  mode "follow"
rounds where the kernels round (fp32 arithmetic in the kernels' summation order, 16-bit stores, __expf as fp32(2^fp32(x log2 e))) and
only shows that the bound is attainable.

Bound (derived, not tuned), per element.  u = 2^-24 (an fp32 rounding), g(n) = n u / (1 - n u) (n roundings in a row), hulp(x) = half a
16-bit ulp of x (bf16: 2^-9 |x| .. 2^-8 |x|), the fp32 division and sqrtf within one ulp (2 u).  A rounding of a sum of which one term is
exactly zero is not counted: that is what makes the bounds below vanish where the result is exact.
The terms below are first order in u.  Every fp32 part of a bound (everything but the hulp of a store) is multiplied by 1 + 2^-10 for the
products of two error terms that the first-order form leaves out: each such product is at most (the largest relative term) times a
term that is counted, and the largest relative terms, eq of the LayerNorm statistics and ew of the pooling kernels, stay below 2^-10 on
every case (asserted where they are computed).  The column sums by atomics use g(n), which holds to all orders, instead.
  LayerNorm statistics.  A row sum is 4 NV serial terms per lane and six butterfly steps: depth d = 4 NV + 6 (NV = 2, 4, 8, 16 for D <=
  512, 1024, 2048, 4096; the row-walking kernel has NV >= 4; the backward NV = 2, 4).
    em   = g(d + 1) sum|x| / D                                   (mean)
    ed_j = em + u (|xc_j| + em)                                  (xc_j = x_j - mean as the kernel holds it)
    eq   = a + g(d + 2) (1 + a),  a = sum_j (2 |xc_j| ed_j + ed_j^2) / sum_j xc_j^2      (relative, of sum xc^2)
    es   = (eq + u) / (2 (1 - eq - u)) + 2 u                     (relative, of std: the division by D - 1, sqrtf)
    er   = es std / s + 3 u                                      (relative, of 1 / s, s = std + eps)
  ln_fwd    e_t = ed / s (1 + er + u) + |xhat| (er + u);  affine: |gain| e_t + u |gain xhat| + u |y|;  pe: + u |y|;  mask: times M, + u |y|;
            + hulp(y) for the 16-bit output.  A zero row has xc = 0 and every term above 0: the reference there is the fp32 chain
            (bias + pe) M itself (and its 16-bit rounding), and the result must be EQUAL.
  ln_bwd    e_dye = 2 u |dye| where dy_add or the mask is applied;  e_h = |gain| e_dye + u |h|;
            e_hm = (sum e_h + g(d + 1) sum|h|) / D;  e_hx = sum (|xc| e_h + |h| ed + u |h xc|) + g(d + 1) sum|h xc|;
            e_k2 = e_hx / (s^2 (D - 1) std) + |k2| (2 er + es + 5 u),  k2 = <h, xc> / (s^2 (D - 1) std)   (0 where std == 0);
            e_dx = (e_h + e_hm + u |h - hm|) / s + |t1| (er + u) + e_k2 |xc| + |k2| ed + u |t2| + u (|t1| + |t2|);
            dx: + hulp;  dxm: Mm e_dx + u |dxm| + hulp;  the column sums: sum_r (error of the addend) + (R + 1) u (sum_r |addend| + |initial
            content|): R addends and the accumulator in NO fixed order (waves, workgroups, atomics or partial rows), addends
            dye xc / s: |xhat| e_dye + |dye| ed / s + |dye xhat| (er + 2 u);  dye: e_dye;  dxm before its store: Mm e_dx + u |dxm|.
  pool_fwd  A thread walks the rows l = rg, rg + rgs, .. of its row group with a running maximum: the weight of row l is a product of at most
            nr + 1 exponentials (nr = ceil(len / rgs) rows per thread, then the merge) whose arguments add up to mx - s_l, and passes
            2 nr + rgs + 2 further roundings:  ew_l = ((mx - s_l) + 2 (nr + 1)) 2^-23 + 2 (nr + rgs + 2) u.  (__expf: the argument is
            multiplied by log2 e in fp32, then v_exp_f32: (|x| + 2) 2^-23, as in attn_cases.py.)
            ssum: sum_l E_l ew_l (+ the masked-fill term's own);  pooled: sum_l E_l Mw_l |z_l| (ew_l + 2 u) / ssum + |pooled| e_ssum / ssum
            + 2 u |pooled|;  smax: 0 — a maximum of 16-bit values (and -32752) is exact;  pk_out: pooled's bound at item rows, 0 (and equal
            to the pooled rows the kernel wrote) elsewhere;  pk_mask, pk_lens: 0.
  pool_bwd  The statistics are fed in fp32: e_fz = u (relative, of ssum), e_fp = u |pooled|; a chained case is fed the forward kernel's
            outputs and takes the forward's bounds instead.   ew = (|s - smax| + 2) 2^-23 + |s - smax| u + 3 u + e_fz;
            ds: Ms (|ds| (ew + 3 u) + w (2 u |g z Mw| + |g| e_fp + u |g pooled|)) + hulp;  dz: |dz| (ew + 2 u) + hulp;  padded rows: 0;
            ds_colsum: sum (error of ds before its store) + (rows + 1) u (sum|ds| + |initial content|).
  avg_fwd   (L - 1) u sum|z| / len + 3 u |out|;   avg_bwd  3 u |dz| + hulp.
  pack_*    0: every element is a copy or takes at most two fp32 additions, which numpy reproduces; the reference is that fp32 chain.
  colsum    (R + 1) u (sum|x| + |initial content|).
Where a bound is zero the result must be equal: zero rows of ln_fwd, padded rows of ds / dz, smax, the pack copies, mask bytes, pk_lens,
pos_out.

Worst |error| / bound per output over all cases; a test passes at <= 1.  "follow": the kernel-following reference against the exact one
(CPU, tests/test_cpu_rowpool_cases.py, bf16); "MI355X": the kernels (tests/test_gpu_rowpool.py, bf16 build).  All of these were measured;
none is an estimate.  The IEEE-half build was run on the same cases and passes; its ratios are not recorded here.
  op        output     follow   MI355X        op        output     follow   MI355X
  ln_fwd    y          1.000    1.000         pool_fwd  pooled     0.125    0.125
  ln_fwd    y32        0.592    0.592         pool_fwd  ssum       0.118    0.118
  ln_bwd    dx         0.999    0.999         pool_fwd  pk_out     0.040    0.040
  ln_bwd    dx32       0.161    0.145         pool_bwd  ds         0.999    0.999
  ln_bwd    dxm        0.999    0.999         pool_bwd  dz         1.000    1.000
  ln_bwd    dgain      0.066    0.066         pool_bwd  ds_colsum  0.294    0.294
  ln_bwd    dbias      0.474    0.474         avg_fwd   out        0.089    0.089
  ln_bwd    dxcolsum   0.175    0.126         avg_bwd   dz         1.000    1.000
  colsum    out        0.500    0.500
smax, pos_out, pk_mask, pk_lens and every pack output are equal to the reference on every case, on the CPU and on the MI355X.  The 16-bit
outputs sit just under 1 by construction: half an ulp is what a correct rounding costs (1.000 is 0.9996 and the like, rounded).  The
kernels agree with the kernel-following reference to the printed digits almost everywhere: they round where the bounds say.  The fp32
outputs use a small part of their bounds because the bounds add the magnitudes of roundings that mostly cancel: the widest margins are
the column sums through atomics, whose bound allows every one of R + 1 roundings its worst sign.

Untouched memory.  Every input and output is a window of a wider allocation: GUARD rows above and below, a column gap where the stride
exceeds the width, the rows between packed sequences and the padded rows nobody may read.  NaNs on the input side, sentinel bytes on the
output side; every sentinel must survive the call, and every input must be unchanged.  Accumulating outputs (dgain, dbias, dxcolsum,
ds_colsum, demb) start from random contents that the reference adds to.
"""
import zlib

import numpy as np

from oracle import coot_oracle as O
from tests.helpers import from_bf16_bits, to_bf16_bits

U = 2.0 ** -24
FILL = -32752.0
EPS = float(np.float32(1e-6))  # csrc/common.h: kLnEps as the kernels hold it
GUARD = 3
UNWRITTEN = np.inf  # in a mutated reference: the wrong kernel does not write the element
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.uint16): 0xA5A5, np.dtype(np.uint32): 0xA5A5A5A5, np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5}
DT = dict(h=np.uint16, f=np.uint32, i32=np.uint32, i64=np.uint64, u8=np.uint8)
SITE, SITE_M, SITE_W, SITE_S = 16 * 3 + 2, 16 * 3 + 3, 16 * 15 + 7, 16 * 15 + 6  # any site words would do
LOG2E32 = np.float32(1.4426950408889634)


def g_(n):
    return n * U / (1.0 - n * U)


# ---- 16-bit formats -----------------------------------------------------------------------------------------------------------------
def enc16(x, fmt):
    x = np.asarray(x, np.float64)
    return to_bf16_bits(x.astype(np.float32)) if fmt == "bf16" else x.astype(np.float32).astype(np.float16).view(np.uint16)


def dec16(b, fmt):
    b = np.ascontiguousarray(b, np.uint16)
    return (from_bf16_bits(b) if fmt == "bf16" else b.view(np.float16)).astype(np.float64)


def rnd16(x, fmt):
    return dec16(enc16(x, fmt), fmt)


def hulp(x, fmt):
    """Half a 16-bit ulp at magnitude |x| (0 at 0; bf16 has 8 significand bits, IEEE half 11 and subnormals below 2^-14)."""
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    h = np.ldexp(1.0, e - 9) if fmt == "bf16" else np.ldexp(1.0, np.maximum(e, -13) - 12)
    return np.where(m > 0, h, 0.0)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def ln_nv(D, kind):
    """NV of the kernel launch_ln_fwd / launch_ln_bwd picks (4 NV 64 >= D elements per wave)."""
    if kind == "bwd":
        return 2 if D <= 512 else 4
    nv = 2 if D <= 512 else 4 if D <= 1024 else 8 if D <= 2048 else 16
    return max(nv, 4) if kind == "stream" else nv


def pool_cpb(D):
    return 16 if D % 128 == 0 else D // 8


def ln_bwd_path(R, D, ws):
    """launch_ln_bwd's dispatch: (workgroups, partial rows through the workspace or 0 for atomics, chunks of the reduction)."""
    blocks = min((R + 3) // 4, 1024)
    part = ws >= blocks * 3 * D
    if not part and blocks > 256:
        blocks = 256
        part = ws >= blocks * 3 * D
    if R <= 512:
        part = False
    chunks = 0
    if part:
        chunks = min((blocks + 63) // 64, 8)
        ppc = (blocks + chunks - 1) // chunks
        chunks = (blocks + ppc - 1) // ppc
    return blocks, blocks if part else 0, chunks


def _lens4(L, batch):
    """1, L - 1, L and a value that ends inside a load batch."""
    mid = batch * (L // (2 * batch)) + batch // 4 + 1 if L > batch + batch // 4 + 1 else max(1, L // 2)
    return [1, max(1, L - 1), L, min(L, mid)]


def _case(op, name, **kw):
    c = dict(op=op, name=name)
    c.update(kw)
    c["seed"] = zlib.crc32(c.get("spec", name).encode()) & 0x7FFFFFFF  # a pool_fwd / pool_bwd pair shares its inputs
    return c


def _ln_fwd_cases():
    cs = []
    Ds = (8, 12, 252, 256, 260, 508, 512, 516, 1024, 1028, 2048, 2052, 4096)
    for i, D in enumerate(Ds):
        R = (1, 4, 5, 9)[i % 4]
        kw = dict(D=D, R=R, x_f32=i % 2 == 0, wide=i % 3 != 0, outs=(("y",), ("y32",), ("y", "y32"))[i % 3], gain=i % 5 != 3,
                  pe_L={1: 2, 3: 4}.get(i % 4, 0), p=0.1 if i % 3 == 1 else 0.0, zero_row=R - 1 if R > 1 else -1)
        cs.append(_case("ln_fwd", f"lnf-D{D}", **kw))
        if R == 1:  # the one row all zero
            cs.append(_case("ln_fwd", f"lnf-D{D}-zero", **dict(kw, zero_row=0)))
    base = dict(x_f32=True, wide=True, outs=("y", "y32"), gain=True, pe_L=0, p=0.0, zero_row=2)
    cs.append(_case("ln_fwd", "lnf-two-src", **dict(base, D=260, R=11, R0=5)))                      # rows 5 .. 10 come from x2; R0 % 4 != 0
    cs.append(_case("ln_fwd", "lnf-two-src-h", **dict(base, D=516, R=9, R0=6, x_f32=False, p=0.1)))
    gather = dict(lens=[3, 1, 5], lens2=[2, 7, 1, 4], L0=5, L1=7)                                     # N0 = 3 padded [3, 5, D], x2 [4, 7, D]
    cs.append(_case("ln_fwd", "lnf-gather", **dict(base, D=256, R=23, pe_L=3, zero_row=4, **gather)))
    cs.append(_case("ln_fwd", "lnf-gather-h", **dict(base, D=1028, R=23, x_f32=False, outs=("y",), **gather)))
    cs.append(_case("ln_fwd", "lnf-srcpacked-f32", **dict(base, D=512, R=23, src_packed=True, **gather)))
    cs.append(_case("ln_fwd", "lnf-srcpacked-h", **dict(base, D=12, R=23, x_f32=False, src_packed=True, p=0.1, **gather)))
    for i, D in enumerate((512, 516, 2052, 4096)):  # the row-walking kernel of the input stages
        w = 1 + i % 2  # max_wgs workgroups walk 8 w + 1 rows: every wave loops, the last trip has one row
        cs.append(_case("ln_fwd", f"lnf-stream-D{D}-loop", **dict(base, D=D, R=8 * w + 1, max_wgs=w, nt=i % 2, gain=i != 1, outs=(("y",), ("y", "y32"))[i % 2], zero_row=8 * w)))
        cs.append(_case("ln_fwd", f"lnf-stream-D{D}-roomy", **dict(base, D=D, R=5, max_wgs=64, nt=1 - i % 2, x_f32=i < 2, p=0.1 if i == 3 else 0.0)))
    cs.append(_case("ln_fwd", "lnf-stream-nt-only", **dict(base, D=516, R=6, max_wgs=0, nt=1, outs=("y",))))
    return cs


def _ln_bwd_cases():
    cs = []
    subsets = (("dx",), ("dx32",), ("dxm",), ("dx", "dx32"), ("dx", "dxm"), ("dx32", "dxm"), ("dx", "dx32", "dxm"))
    for i, D in enumerate((8, 12, 508, 512, 516, 1020, 1024)):
        cs.append(_case("ln_bwd", f"lnb-D{D}", D=D, R=(5, 9, 6)[i % 3], dy32=i % 2 == 1, dy_add=i % 3 == 0, x_f32=i % 2 == 0, p=0.1 if i % 3 != 1 else 0.0,
                        outs=subsets[i], pm=0.1 if i % 2 == 0 else 0.0, drop_ld=D + 6 if i % 4 == 0 else D, sums=tuple(s for j, s in enumerate(("dgain", "dbias", "dxcolsum")) if (i + j) % 4 != 1),
                        wide=i % 2 == 0, ws=0, zero_row=2))
    full = dict(dy32=False, dy_add=True, x_f32=False, p=0.1, outs=("dx", "dxm"), pm=0.1, sums=("dgain", "dbias", "dxcolsum"), wide=False, zero_row=1)
    for R, D, ws, nm in ((1, 516, 0, "R1"), (512, 12, 1 << 20, "R512-ws"), (513, 516, -1, "R513-parts"), (513, 12, 0, "R513-atomics"),
                         (4101, 8, -1, "R4101-cap"), (1029, 8, 256 * 3 * 8, "R1029-fallback"), (1029, 8, 0, "R1029-atomics")):
        blocks = min((R + 3) // 4, 1024)
        cs.append(_case("ln_bwd", f"lnb-{nm}", **dict(full, D=D, R=R, ws=blocks * 3 * D if ws < 0 else ws, drop_ld=D + 2, zero_row=min(1, R - 1))))
    return cs


def _pool_cases():
    specs = []

    def add(name, D, Ls, **kw):
        rgs = 256 // pool_cpb(D)
        s = dict(D=D, segs=[dict(L=L, lens=_lens4(L, 4 * rgs)) for L in Ls], packed=False, p_w=0.0, p_s=None, wide=False, copy=True, counts=None,
                 Cmax=0, colsum="atomics", chained=False, deep=False)
        for k in ("lens", "lens2"):
            if k in kw:
                s["segs"][k == "lens2"]["lens"] = kw.pop(k)
        s.update(kw)
        if s["p_s"] is None:  # without dropout2 a sequence's column sum of ds is zero: a lost partial row would not show
            s["p_s"] = 0.1 if s["colsum"] and not name.startswith("pool-D384-L") else 0.0
        specs.append((name, s))

    modes = ("atomics", "partials", "defer", None)
    for i, D in enumerate((64, 72, 128, 192, 504, 512)):
        add(f"pool-D{D}", D, [(33, 9, 40, 11, 17, 21)[i]], wide=i % 2 == 0, copy=i % 2 == 1, colsum=modes[i % 4])
    for i, L in enumerate((1, 15, 16, 17, 63, 64, 65, 130)):
        add(f"pool-D384-L{L}", 384, [L], wide=i % 2 == 1, copy=i % 3 != 0, colsum=modes[i % 4])
    for i, L in enumerate((1, 4, 16, 17)):
        add(f"pool-D504-L{L}", 504, [L], colsum=modes[(i + 1) % 4])
    add("pool-drop", 384, [65], p_w=0.1, p_s=0.1, colsum="partials")
    add("pool-drop-D72", 72, [30], p_w=0.1, p_s=0.1, wide=True)
    add("pool-seg2", 384, [20, 7], lens2=[7, 1, 6, 3, 7], colsum="partials")
    add("pool-seg2-drop", 128, [9, 33], lens2=[33, 1, 32, 17, 20], p_w=0.1, p_s=0.1, colsum="defer")
    add("pool-packed", 384, [33], lens=[1, 33, 16, 17, 32, 5, 21], packed=True, colsum="partials")
    add("pool-packed-seg2-drop", 192, [20, 80], lens=[20, 1, 13, 19, 16], lens2=[80, 33, 1, 79, 64, 21], packed=True, p_w=0.1, p_s=0.1)
    add("pool-N70", 64, [3], lens=[1 + (7 * n) % 3 for n in range(70)], colsum="partials")  # 70 partial rows: the reduction runs 2 chunks
    add("pool-N70-defer", 64, [3], lens=[1 + (5 * n) % 3 for n in range(70)], colsum="defer", p_s=0.1)
    add("pool-chained", 384, [65], chained=True, p_w=0.1, colsum="partials")
    add("pool-deep", 64, [6], lens=[1, 5, 6, 3], deep=True)  # scores at the masked fill: its term carries the statistics
    # the hand-over into [B, Cmax, D]: zero-count videos at the front, in the middle and at the end; one video; the scan's second trip
    add("pool-pk", 384, [5], lens=[5, 1, 4, 2, 3, 5, 1], counts=[0, 0, 3, 0, 1, 3, 0, 0], Cmax=4, colsum=None)
    add("pool-pk-B1", 72, [4], lens=[4, 1, 3], counts=[3], Cmax=5, colsum=None)
    add("pool-pk-seg2", 128, [6, 3], lens=[6, 1], lens2=[3, 1, 2, 3, 1], counts=[2, 0, 3], Cmax=3, colsum="defer")  # the items are the SECOND segment
    c260 = [(1, 2, 0, 1, 1, 3, 0, 1, 2, 1)[b % 10] for b in range(260)]
    c260[0], c260[259] = 0, 1
    add("pool-pk-B260", 64, [1], lens=[1] * sum(c260), counts=c260, Cmax=3, colsum="partials")
    cs = []
    for name, s in specs:
        for d in ("fwd", "bwd"):
            cs.append(_case("pool_" + d, f"{name}-{d}", spec=name, **s))
    return cs


def _other_cases():
    cs = []
    for i, D in enumerate((2, 510, 512, 514)):
        for L in (1, 9):
            kw = dict(D=D, L=L, lens=[1, L, max(1, L - 1), max(1, L // 2), L][:3 + i % 3], wide=(i + L) % 2 == 0)
            cs.append(_case("avg_fwd", f"avgf-D{D}-L{L}", **kw))
            cs.append(_case("avg_bwd", f"avgb-D{D}-L{L}", **kw))
    c300 = [(2, 0, 1, 3, 1, 0, 0, 2)[b % 8] for b in range(300)]
    for i, (nm, counts, Cmax) in enumerate((("zeros", [0, 0, 3, 0, 1, 2, 0], 3), ("B1", [4], 4), ("B300", c300, 4), ("roomy", [2, 1, 0, 2], 5))):
        for D in (6, 384):
            kw = dict(counts=counts, Cmax=Cmax, D=D)
            cs.append(_case("pack_fwd", f"packf-{nm}-D{D}", **kw))
            cs.append(_case("pack_bwd", f"packb-{nm}-D{D}", **kw))
            cs.append(_case("pack_join", f"packj-{nm}-D{D}", dout2=(i + (D == 6)) % 2 == 0, dctx=(i // 2 + (D == 6)) % 2 == 0, **kw))
    cs.append(_case("pack_join", "packj-plain-D6", counts=[1, 0, 2], Cmax=2, D=6, dout2=False, dctx=False))
    cs.append(_case("pack_join", "packj-both-D6", counts=[1, 0, 2], Cmax=2, D=6, dout2=True, dctx=True))
    for i, C in enumerate((2, 510, 512, 514)):
        for R, ws in ((1, 0), (512, 1 << 16), (513, -1), (513, 0)):
            cs.append(_case("colsum", f"colsum-C{C}-R{R}" + ("-ws" if ws else ""), C=C, R=R, ws=((R + 63) // 64) * C if ws < 0 else ws, wide=(i + R) % 2 == 0))
    return cs


def _cases():
    cs = _ln_fwd_cases() + _ln_bwd_cases() + _pool_cases() + _other_cases()
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def _t(kind, rows, cols, ld=None, role="in", rowmask=None):
    return dict(kind=kind, rows=int(rows), cols=int(cols), ld=int(ld or cols), role=role, rowmask=np.ones(int(rows), bool) if rowmask is None else rowmask)


def pool_rows(c):
    """Per segment: first row of every sequence, rows it occupies (Lp), valid rows, total rows, the mask of the rows that exist."""
    out = []
    for si, sg in enumerate(c["segs"]):
        lens = list(sg["lens"])
        if c["packed"]:
            cu, row = [], 0
            for n, l in enumerate(lens):
                cu.append(row)
                row += l + (n + si) % 3  # 0 .. 2 guard rows between the sequences
            T, Lp = cu[-1] + lens[-1], lens
        else:
            cu, T, Lp = [n * sg["L"] for n in range(len(lens))], len(lens) * sg["L"], [sg["L"]] * len(lens)
        exists, valid = np.zeros(T, bool), np.zeros(T, bool)
        for r0, lp, l in zip(cu, Lp, lens):
            exists[r0:r0 + lp] = True
            valid[r0:r0 + l] = True
        out.append(dict(cu=cu, Lp=Lp, lens=lens, T=T, exists=exists, valid=valid, N=len(lens), L=sg["L"]))
    return out


def ln_gather(c):
    """Packed output rows of ln_fwd: cu [nseq + 1], per output row (source 0 / 1, source row, position)."""
    lens = list(c["lens"]) + list(c["lens2"])
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N0, rows = len(c["lens"]), []
    for n, ln in enumerate(lens):
        for l in range(ln):
            r = len(rows)
            rows.append((0, r, l) if c.get("src_packed") else (0, n * c["L0"] + l, l) if n < N0 else (1, (n - N0) * c["L1"] + l, l))
    return cu, rows


def tensors(c):
    """name -> tensor (kind h: 16-bit operand, f: fp32, i32, i64, u8; rows, cols, ld; role in / out / acc; rowmask: the rows that exist)."""
    op, t = c["op"], {}
    if op == "ln_fwd":
        D, R, g = c["D"], c["R"], 8 if c["wide"] else 0
        kx = "f" if c["x_f32"] else "h"
        if "lens" in c and not c.get("src_packed"):
            _, rows = ln_gather(c)
            for nm, src, T in (("x", 0, len(c["lens"]) * c["L0"]), ("x2", 1, len(c["lens2"]) * c["L1"])):
                m = np.zeros(T, bool)
                m[[r for s, r, _ in rows if s == src]] = True
                t[nm] = _t(kx, T, D, D + g, rowmask=m)
        elif "R0" in c:
            t["x"], t["x2"] = _t(kx, c["R0"], D, D + g), _t(kx, R - c["R0"], D, D + g)
        else:
            t["x"] = _t(kx, R, D, D + g)
        if c["gain"]:
            t["gain"], t["bias"] = _t("f", 1, D), _t("f", 1, D)
        if c["pe_L"]:
            t["pe"] = _t("f", c["pe_L"], D)
        if "y" in c["outs"]:
            t["y"] = _t("h", R, D, D + g, "out")
        if "y32" in c["outs"]:
            t["y32"] = _t("f", R, D, D + 2 * g, "out")
        if "lens" in c:
            t["pos_out"] = _t("i32", 1, R, role="out")
    elif op == "ln_bwd":
        D, R, g = c["D"], c["R"], 8 if c["wide"] else 0
        t["x"] = _t("f" if c["x_f32"] else "h", R, D, D + g)
        t["dy"] = _t("f" if c["dy32"] else "h", R, D, D + g)
        if c["dy_add"]:
            t["dy_add"] = _t("h", R, D, D + 2 * g)
        t["gain"] = _t("f", 1, D)
        for nm in c["outs"]:
            t[nm] = _t("f" if nm == "dx32" else "h", R, D, D + g, "out")
        for nm in c["sums"]:
            t[nm] = _t("f", 1, D, role="acc")
    elif op in ("pool_fwd", "pool_bwd"):
        D, g, back = c["D"], 8 if c["wide"] else 0, c["op"] == "pool_bwd"
        for i, pr in enumerate(pool_rows(c)):
            sfx, N = ("", "2")[i], pr["N"]
            t["s" + sfx], t["z" + sfx] = _t("h", pr["T"], D, D + g, rowmask=pr["valid"]), _t("h", pr["T"], D, D + 2 * g, rowmask=pr["valid"])
            st = "in" if back else "out"
            t["pooled" + sfx] = _t("f", N, D, 2 * D if c["wide"] else D, st)
            t["smax" + sfx], t["ssum" + sfx] = _t("f", N, D, role=st), _t("f", N, D, role=st)
            if back:
                t["dpooled" + sfx] = _t("f", N, D, D + g)
                t["ds" + sfx], t["dz" + sfx] = _t("h", pr["T"], D, D + g, "out", pr["exists"]), _t("h", pr["T"], D, D + 2 * g, "out", pr["exists"])
            elif c["copy"]:
                t["pooled_copy" + sfx] = _t("f", N, D, role="out")
        if back and c["colsum"]:
            t["ds_colsum"] = _t("f", 1, D, role="acc")
        if not back and c["counts"]:
            B, Cm = len(c["counts"]), c["Cmax"]
            t["pk_out"], t["pk_mask"], t["pk_lens"] = _t("f", B * Cm, D, role="out"), _t("u8", 1, B * Cm, role="out"), _t("i64", 1, B, role="out")
    elif op in ("avg_fwd", "avg_bwd"):
        D, L, N, g = c["D"], c["L"], len(c["lens"]), 8 if c["wide"] else 0
        if op == "avg_fwd":
            t["z"], t["out"] = _t("h", N * L, D, D + g), _t("f", N, D, D + g, "out")
        else:
            t["dpooled"], t["dz"] = _t("f", N, D, D + g), _t("h", N * L, D, D + g, "out")
    elif op in ("pack_fwd", "pack_bwd", "pack_join"):
        B, Cm, D, n = len(c["counts"]), c["Cmax"], c["D"], max(1, sum(c["counts"]))
        if op == "pack_fwd":
            t["emb"], t["out"] = _t("f", n, D), _t("f", B * Cm, D, role="out")
            t["mask"], t["lens"] = _t("u8", 1, B * Cm, role="out"), _t("i64", 1, B, role="out")
        else:
            valid = (np.arange(Cm)[None, :] < np.asarray(c["counts"])[:, None]).ravel()
            t["dout"], t["demb"] = _t("f", B * Cm, D, rowmask=valid), _t("f", n, D, role="acc", rowmask=np.arange(n) < sum(c["counts"]))
            if c.get("dout2"):
                t["dout2"] = _t("f", B * Cm, D, rowmask=valid)
            if c.get("dctx"):
                t["dctx"], t["demb_ctx"] = _t("f", B, D), _t("f", B, D, role="acc")
    elif op == "colsum":
        t["x"], t["out"] = _t("h", c["R"], c["C"], c["C"] + (8 if c["wide"] else 0)), _t("f", 1, c["C"], role="acc")
    return t


def outputs(c):
    return [k for k, v in tensors(c).items() if v["role"] != "in"]


def inputs(c, fmt="bf16"):
    """fp64 arrays of representable values: every input tensor in full, and "init_<name>" for the accumulating outputs."""
    T, inp = tensors(c), {}
    for nm, t in T.items():
        if t["role"] == "out" or (c["op"] == "pool_bwd" and nm.rstrip("2") in ("smax", "ssum", "pooled")):
            continue
        rs = np.random.RandomState(zlib.crc32(f"{c['seed']}/{nm}".encode()))  # a tensor's values do not depend on the others
        x = rs.randn(t["rows"], t["cols"])
        if nm in ("gain",):
            x = 1.0 + 0.5 * x
        if nm in ("x", "x2") and c["op"] in ("ln_fwd", "ln_bwd"):
            x = x * np.exp(rs.randn(t["rows"], 1)) + rs.randn(t["rows"], 1)  # rows of different scale and offset
            x[0] = 2.0 ** -10 * rs.randn(t["cols"])                           # and one whose std is of the size of sqrt(eps)
        if nm in ("s", "s2"):
            x = _pool_scores(c, rs, nm == "s2", t)
        if nm in ("dy", "dy_add") and c["zero_row"] >= 0:
            x[c["zero_row"]] *= 2.0 ** -10  # the zero row's dx is h / eps: kept below the largest IEEE half
        inp[("init_" if t["role"] == "acc" else "") + nm] = rnd16(x, fmt) if t["kind"] == "h" else f32(x)
    if c["op"] in ("ln_fwd", "ln_bwd") and c["zero_row"] >= 0:
        if c["op"] == "ln_fwd" and ("lens" in c or "R0" in c):
            if "lens" in c:
                s, r, _ = ln_gather(c)[1][c["zero_row"]]
            else:
                s, r = (0, c["zero_row"]) if c["zero_row"] < c["R0"] else (1, c["zero_row"] - c["R0"])
            inp[("x", "x2")[s]][r] = 0.0
        else:
            inp["x"][c["zero_row"]] = 0.0
    return inp


def _pool_scores(c, rs, second, t):
    """Scores spread over about +-30; per channel (c % 4) the maximum of every sequence sits in the first row group, the last row group, the
    last valid row, or anywhere; channel 5 has all scores equal.  deep: channels 8 .. 15 sit at the masked fill."""
    D = c["D"]
    pr = pool_rows(c)[int(second)]
    rgs = 256 // pool_cpb(D)
    x = np.clip(10.0 * rs.randn(t["rows"], D), -30.0, 29.0)
    ch = np.arange(D)
    for r0, l in zip(pr["cu"], pr["lens"]):
        last_rg = max(r for r in range(l) if r % rgs == min(rgs, l) - 1)  # the last row of the last row group that holds any
        for k, row in ((0, 0), (1, last_rg), (2, l - 1)):
            x[r0 + row, ch[ch % 4 == k]] = 30.0 + rs.rand((ch % 4 == k).sum())
    x[:, 5] = 3.0
    if c["deep"]:
        x[:, 8:16] = -32768.0  # 16 below the fill, which is then the maximum of every padded sequence
    return x


def ints(c):
    """The integer inputs (lens, cu, counts): name -> numpy array of the dtype the kernels read."""
    op = c["op"]
    if op == "ln_fwd" and "lens" in c:
        return dict(cu=ln_gather(c)[0].astype(np.int32))
    if op in ("pool_fwd", "pool_bwd"):
        d = {}
        for i, pr in enumerate(pool_rows(c)):
            d["lens" + ("", "2")[i]] = np.asarray(pr["lens"], np.int64)
            if c["packed"]:
                d["cu" + ("", "2")[i]] = np.asarray(pr["cu"], np.int32)
        if c["counts"]:
            d["counts"] = np.asarray(c["counts"], np.int64)
        return d
    if op in ("avg_fwd", "avg_bwd"):
        return dict(lens=np.asarray(c["lens"], np.int64))
    if op.startswith("pack"):
        return dict(counts=np.asarray(c["counts"], np.int64))
    return {}


# ---- dropout masks ------------------------------------------------------------------------------------------------------------------
def keep_scales(lib, seed, site, p, rows, ld, cols, row0=0):
    """[rows, cols] keep-scales of the elements (row0 + r) ld + col of (seed, site), from the library's host generator."""
    m = np.empty(rows * ld, np.float32)
    rc = lib.coot_debug_dropout_scales(int(seed) & (2 ** 64 - 1), site, int(row0) * int(ld), rows * ld, p, m.ctypes.data)
    assert rc == 0
    return m.reshape(rows, ld)[:, :cols].astype(np.float64)


def pool_seed(c, second):
    return c["seed"] + 977 * int(second)  # api.hip: the second segment's dropout3 draws from seed + 977


def pool_row0(c, second):
    return (pool_rows(c)[0]["T"] + 5) if second else 0  # drop_s_row0: the segment's first token row in the call's token matrix


def masks(c, lib, mut=None):
    """The keep-scales a case multiplies with (ones without dropout); mut: the masks a subtly wrong kernel would draw."""
    op, m = c["op"], {}
    sh = int(mut == "mask_row")
    if op in ("ln_fwd", "ln_bwd"):
        D, R = c["D"], c["R"]
        m["M"] = keep_scales(lib, c["seed"], SITE, c["p"], R, D, D, sh) if c["p"] > 0 else np.ones((R, D))
        if op == "ln_bwd":
            ld = D if mut == "mask_ld" else c["drop_ld"]
            m["Mm"] = keep_scales(lib, c["seed"] + 1, SITE_M, c["pm"], R, ld, D, sh) if c["pm"] > 0 and "dxm" in c["outs"] else np.ones((R, D))
    elif op in ("pool_fwd", "pool_bwd"):
        D = c["D"]
        for i, pr in enumerate(pool_rows(c)):
            sfx = ("", "2")[i]
            one = np.ones((pr["T"], D))
            m["Mw" + sfx] = keep_scales(lib, pool_seed(c, i and mut != "seed2"), SITE_W, c["p_w"], pr["T"], D, D, sh) if c["p_w"] > 0 else one
            ld = D if mut == "mask_ld" else D + 6
            r0 = 0 if mut == "row0" else pool_row0(c, i)
            m["Ms" + sfx] = keep_scales(lib, c["seed"] + 3, SITE_S, c["p_s"], pr["T"], ld, D, r0 + sh) if c["p_s"] > 0 and op == "pool_bwd" else one
    return m


# ---- references and bounds ----------------------------------------------------------------------------------------------------------
def _ln_rows(c, inp):
    """The LayerNorm source rows in output order [R, D]."""
    if c["op"] == "ln_fwd" and "lens" in c:
        return np.stack([inp[("x", "x2")[s]][r] for s, r, _ in ln_gather(c)[1]])
    if c["op"] == "ln_fwd" and "R0" in c:
        return np.concatenate([inp["x"], inp["x2"]])
    return inp["x"]


def _wave_sum32(v):
    """wave_sum of common.h on [rows, 64] fp32: six butterfly steps."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def _lanes(x, NV):
    """[R, D] -> [R, NV, 64, 4] fp32, chunk c = lane + 64 i, zero beyond D."""
    R, D = x.shape
    out = np.zeros((R, NV * 256), np.float32)
    out[:, :D] = x
    return out.reshape(R, NV, 64, 4)


def _rowsum32(v):
    """The kernels' row reduction of per-element fp32 terms v [R, NV, 64, 4]: serial per lane, then the butterfly."""
    s = np.zeros((v.shape[0], 64), np.float32)
    for i in range(v.shape[1]):
        s = s + (((v[:, i, :, 0] + v[:, i, :, 1]) + v[:, i, :, 2]) + v[:, i, :, 3])
    return _wave_sum32(s)


def _rowdot32(a, b):
    """sum of a b accumulated one product at a time per lane (q += d d), then the butterfly."""
    s = np.zeros((a.shape[0], 64), np.float32)
    for i in range(a.shape[1]):
        for j in range(4):
            s = s + a[:, i, :, j] * b[:, i, :, j]
    return _wave_sum32(s)


def _ln_stat_bounds(x, NV):
    """Exact statistics of the rows and the error terms of the module docstring."""
    D = x.shape[1]
    d = 4 * NV + 6
    mean = x.mean(-1, keepdims=True)
    xc = x - mean
    Q = (xc * xc).sum(-1, keepdims=True)
    std = np.sqrt(Q / (D - 1))
    s = std + EPS
    em = g_(d + 1) * np.abs(x).sum(-1, keepdims=True) / D
    ed = em + U * (np.abs(xc) + em)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(Q > 0, (2 * np.abs(xc) * ed + ed * ed).sum(-1, keepdims=True) / np.where(Q > 0, Q, 1.0), 0.0)
    assert ((Q > 0) | (np.abs(x).sum(-1, keepdims=True) == 0)).all(), "a constant non-zero row has no derived bound"
    eq = np.where(Q > 0, a + g_(d + 2) * (1 + a), 0.0)
    assert (eq < 2.0 ** -10).all(), "the first-order bound needs eq < 2^-10"
    es = np.where(Q > 0, (eq + U) / (2 * (1 - eq - U)) + 2 * U, 0.0)
    er = es * std / s + 3 * U
    return dict(xc=xc, std=std, s=s, ed=ed, es=es, er=er, d=d)


def _ln_stats(x, mut):
    D = x.shape[1]
    xc = x - x.mean(-1, keepdims=True)
    var = (xc * xc).sum(-1, keepdims=True) / (D if mut == "biased_var" else D - 1)
    std = np.sqrt(var)
    s = np.sqrt(var + EPS) if mut == "eps_in_sqrt" else std + EPS
    return xc, std, s


def _ln_fwd(c, inp, M, mode, mut, fmt):
    D, R = c["D"], c["R"]
    x = _ln_rows(c, inp)
    gain = inp["gain"][0] if c["gain"] else None
    bias = inp["bias"][0] if c["gain"] else None
    pe = inp["pe"][np.arange(R) % c["pe_L"]] if c["pe_L"] else None
    r = {}
    if "lens" in c:
        r["pos_out"] = np.asarray([[l for _, _, l in ln_gather(c)[1]]], np.float64)
        r["b_pos_out"] = np.zeros_like(r["pos_out"])
    if mode == "follow":
        NV = ln_nv(D, "stream" if c.get("max_wgs") or c.get("nt") else "fwd")
        v = _lanes(x, NV)
        mean = _rowsum32(v) / np.float32(D)
        dd = np.where(np.arange(NV * 256).reshape(NV, 64, 4) < D, v - mean[:, None, None, None], np.float32(0))
        stdv = np.sqrt(_rowdot32(dd, dd) / np.float32(D - 1))
        rs = np.float32(1.0) / (stdv + np.float32(EPS))
        y = dd.reshape(R, -1)[:, :D] * rs[:, None]
        if gain is not None:
            y = y * gain.astype(np.float32) + bias.astype(np.float32)
        if pe is not None:
            y = y + pe.astype(np.float32)
        if c["p"] > 0:
            y = y * M.astype(np.float32)
        assert y.dtype == np.float32
        y = y.astype(np.float64)
        if "y" in c["outs"]:
            r["y"] = rnd16(y, fmt)
        if "y32" in c["outs"]:
            r["y32"] = y
        return r
    xc, std, s = _ln_stats(x, mut)
    xhat = xc / s
    y = xhat if gain is None else gain * xhat + bias
    if pe is not None:
        y = y + pe
    y = y * M
    # the fp32 chain of a zero row: (bias + pe) M, exact in the kernel
    zero = (np.abs(x).sum(-1) == 0)
    yz = np.zeros((R, D), np.float32) if gain is None else np.broadcast_to(bias.astype(np.float32), (R, D)).copy()
    if pe is not None:
        yz = yz + pe.astype(np.float32)
    if c["p"] > 0:
        yz = yz * M.astype(np.float32)
    y[zero] = yz.astype(np.float64)[zero]
    for nm in c["outs"]:
        r[nm] = y.copy()
    if "y" in c["outs"]:
        r["y"][zero] = rnd16(y[zero], fmt)
    if mut is not None:
        return r
    NV = ln_nv(D, "stream" if c.get("max_wgs") or c.get("nt") else "fwd")
    b = _ln_stat_bounds(x, NV)
    e = b["ed"] / b["s"] * (1 + b["er"] + U) + np.abs(xhat) * (b["er"] + U)
    cur = xhat
    if gain is not None:
        cur = gain * xhat + bias
        e = np.abs(gain) * e + U * np.abs(gain * xhat) + U * np.abs(cur)
    if pe is not None:
        cur = cur + pe
        e = e + U * np.abs(cur)
    if c["p"] > 0:
        cur = cur * M
        e = M * e + U * np.abs(cur)
    e = e * (1 + 2.0 ** -10)  # the products of two error terms left out above
    e[zero] = 0.0
    if "y32" in c["outs"]:
        r["b_y32"] = e
    if "y" in c["outs"]:
        r["b_y"] = np.where(zero[:, None], 0.0, e + hulp(np.abs(y) + e, fmt))
    return r


def _colsum32(add, blocks):
    """Column sums of the addends [R, D] (fp32) as ln_bwd_kernel forms them: a wave's rows one after the other, the four waves of a
    workgroup, then the workgroups one after the other (what the atomics or the reduction do in some order)."""
    R, D = add.shape
    per = blocks * 4
    k = (R + per - 1) // per
    a = np.zeros((k * per, D), np.float32)
    a[:R] = add
    a = a.reshape(k, blocks, 4, D)
    w = np.zeros((blocks, 4, D), np.float32)
    for i in range(k):
        w = w + a[i]
    blk = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return blk


def _ln_bwd(c, inp, ms, mode, mut, fmt):
    D, R = c["D"], c["R"]
    x, gain, M, Mm = inp["x"], inp["gain"][0], ms["M"], ms["Mm"]
    dy = inp["dy"] + (inp["dy_add"] if c["dy_add"] else 0.0)
    blocks, parts, _ = ln_bwd_path(R, D, c["ws"])
    r = {}
    if mode == "follow":
        NV = ln_nv(D, "bwd")
        dye = inp["dy"].astype(np.float32)
        if c["dy_add"]:
            dye = dye + inp["dy_add"].astype(np.float32)
        if c["p"] > 0:
            dye = dye * M.astype(np.float32)
        v = _lanes(x, NV)
        inside = np.arange(NV * 256).reshape(NV, 64, 4) < D
        mean = _rowsum32(v) / np.float32(D)
        dd = np.where(inside, v - mean[:, None, None, None], np.float32(0))
        h = _lanes(dye * gain.astype(np.float32), NV)
        q, hs, hx = _rowdot32(dd, dd), _rowsum32(h), _rowdot32(h, dd)
        stdv = np.sqrt(q / np.float32(D - 1))
        rs = np.float32(1.0) / (stdv + np.float32(EPS))
        hmean = hs / np.float32(D)
        with np.errstate(divide="ignore", invalid="ignore"):
            k2 = np.where(stdv > 0, hx * rs * rs / (np.float32(D - 1) * stdv), np.float32(0)).astype(np.float32)
        xc32 = dd.reshape(R, -1)[:, :D]
        dx = (dye * gain.astype(np.float32) - hmean[:, None]) * rs[:, None] - k2[:, None] * xc32
        dm = dx * Mm.astype(np.float32)
        assert dx.dtype == np.float32 and dm.dtype == np.float32
        res = dict(dx=rnd16(dx, fmt), dx32=dx.astype(np.float64), dxm=rnd16(dm, fmt))
        adds = dict(dgain=dye * xc32 * rs[:, None], dbias=dye, dxcolsum=dm)
        for nm in c["outs"]:
            r[nm] = res[nm]
        for nm in c["sums"]:
            acc = inp["init_" + nm][0].astype(np.float32)
            for row in _colsum32(adds[nm], blocks):
                acc = acc + row
            r[nm] = acc.astype(np.float64)[None]
        return r
    dye = dy * M
    xc, std, s = _ln_stats(x, mut)
    n1 = D if mut == "biased_var" else D - 1
    h = dye * gain
    hm = h.mean(-1, keepdims=True)
    t1 = (h - hm) / s
    dot = (h * xc).sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        k2 = np.where(std > 0, dot / (s * s * n1 * np.where(std > 0, std, 1.0)), np.nan if mut == "std0_term" else 0.0)
    t2 = k2 * xc
    dx = t1 - t2
    dxm = dx * Mm
    res = dict(dx=dx, dx32=dx, dxm=dxm)
    adds = dict(dgain=dye * xc / s, dbias=dye, dxcolsum=dxm if "dxm" in c["outs"] else dx)
    for nm in c["outs"]:
        r[nm] = res[nm]
    skip = np.zeros(R, bool)
    if mut == "partial_missing":  # the rows of the last workgroup
        skip[[row for row in range(R) if (row // 4) % blocks == blocks - 1]] = True
    for nm in c["sums"]:
        r[nm] = (0.0 if mut == "colsum_overwrite" else inp["init_" + nm]) + adds[nm][~skip].sum(0, keepdims=True)
    if mut is not None:
        return r
    b = _ln_stat_bounds(x, ln_nv(D, "bwd"))
    ed, es, er, d = b["ed"], b["es"], b["er"], b["d"]
    e_dye = np.abs(dye) * (U * (int(c["dy_add"]) + int(c["p"] > 0)))
    e_h = np.abs(gain) * e_dye + U * np.abs(h)
    e_hm = (e_h.sum(-1, keepdims=True) + g_(d + 1) * np.abs(h).sum(-1, keepdims=True)) / D
    e_hx = (np.abs(xc) * e_h + np.abs(h) * ed + U * np.abs(h * xc)).sum(-1, keepdims=True) + g_(d + 1) * np.abs(h * xc).sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_k2 = np.where(std > 0, e_hx / (s * s * (D - 1) * np.where(std > 0, std, 1.0)) + np.abs(k2) * (2 * er + es + 5 * U), 0.0)
    e_dx = (e_h + e_hm + U * np.abs(h - hm)) / s + np.abs(t1) * (er + U) + e_k2 * np.abs(xc) + np.abs(k2) * ed + U * np.abs(t2) + U * (np.abs(t1) + np.abs(t2))
    e_dx = e_dx * (1 + 2.0 ** -10)
    e_dm = Mm * e_dx + U * np.abs(dxm)
    bd = dict(dx=e_dx + hulp(np.abs(dx) + e_dx, fmt), dx32=e_dx, dxm=e_dm + hulp(np.abs(dxm) + e_dm, fmt))
    xhat = xc / s
    e_add = dict(dgain=(np.abs(xhat) * e_dye + np.abs(dye) * ed / s + np.abs(dye * xhat) * (er + 2 * U)) * (1 + 2.0 ** -10), dbias=e_dye,
                 dxcolsum=e_dm if "dxm" in c["outs"] else e_dx)
    for nm in c["outs"]:
        r["b_" + nm] = bd[nm]
    for nm in c["sums"]:
        r["b_" + nm] = e_add[nm].sum(0, keepdims=True) + g_(R + 1) * (np.abs(adds[nm]).sum(0, keepdims=True) + np.abs(inp["init_" + nm]))
    return r


def _exp32(x):
    """__expf on fp32 x: the argument times log2 e in fp32, then 2^."""
    return np.exp2((x.astype(np.float32) * LOG2E32).astype(np.float64)).astype(np.float32)


def pack_rows(c, rows, fill=0.0):
    """pack_by_count of [sum counts, D] rows into [B Cmax, D]."""
    out, _, _ = O.pack_by_count(rows, np.asarray(c["counts"]), c["Cmax"])
    if fill != 0.0:
        valid = (np.arange(c["Cmax"])[None, :] < np.asarray(c["counts"])[:, None])
        out[~valid] = fill
    return out.reshape(-1, rows.shape[1])


def _pool(c, inp, ms, mode, mut, fmt, fed):
    D, back = c["D"], c["op"] == "pool_bwd"
    cpb = pool_cpb(D)
    rgs = 256 // cpb
    r = {}
    tot_add, tot_err, nrows = np.zeros((1, D)), np.zeros((1, D)), 0
    prs = pool_rows(c)
    for i, pr in enumerate(prs):
        sfx = ("", "2")[i]
        S, Z, Mw, Ms = inp["s" + sfx], inp["z" + sfx], ms["Mw" + sfx], ms["Ms" + sfx]
        N, T = pr["N"], pr["T"]
        out = {k: np.zeros((N, D)) for k in ("pooled", "smax", "ssum", "b_pooled", "b_smax", "b_ssum")}
        ds, dz, b_ds, b_dz = (np.zeros((T, D)) for _ in range(4))
        lens = list(pr["lens"])
        if mut == "lens_next":
            lens = [min(lens[(n + 1) % N], pr["Lp"][n]) for n in range(N)]
        if mut in ("len_plus", "len_minus"):
            lens = [min(max(1, l + (1 if mut == "len_plus" else -1)), lp if not c["packed"] else l) for l, lp in zip(lens, pr["Lp"])]
        for n in range(N):
            r0, Lp, ln = pr["cu"][n], pr["Lp"][n], lens[n]
            with np.errstate(invalid="ignore"):
                s, z, mw = S[r0:r0 + ln], Z[r0:r0 + ln], Mw[r0:r0 + ln]
            npad = Lp - ln
            nr = (ln + rgs - 1) // rgs
            if mode == "follow" and not back:
                m32 = np.full((rgs, D), -np.inf, np.float32)
                z32, a32 = np.zeros((rgs, D), np.float32), np.zeros((rgs, D), np.float32)
                for l in range(ln):
                    g, sl = l % rgs, s[l].astype(np.float32)
                    mn = np.maximum(m32[g], sl)
                    with np.errstate(invalid="ignore"):
                        rr = np.where(np.isinf(m32[g]), np.float32(0), _exp32(np.where(np.isinf(m32[g]), np.float32(0), m32[g] - mn)))
                    e = _exp32(sl - mn)
                    z32[g] = z32[g] * rr + e
                    a32[g] = a32[g] * rr + e * mw[l].astype(np.float32) * z[l].astype(np.float32)
                    m32[g] = mn
                mm = m32.max(0)
                if npad:
                    mm = np.maximum(mm, np.float32(FILL))
                zz, aa = np.zeros(D, np.float32), np.zeros(D, np.float32)
                for g in range(rgs):
                    with np.errstate(invalid="ignore"):
                        rr = np.where(np.isinf(m32[g]), np.float32(0), _exp32(np.where(np.isinf(m32[g]), np.float32(0), m32[g] - mm)))
                    zz = zz + z32[g] * rr
                    aa = aa + a32[g] * rr
                if npad:
                    zz = zz + np.float32(npad) * _exp32(np.float32(FILL) - mm)
                out["pooled"][n], out["smax"][n], out["ssum"][n] = (aa / zz).astype(np.float64), mm.astype(np.float64), zz.astype(np.float64)
                continue
            # exact statistics (also what the backward is fed)
            keep = np.ones(ln, bool)
            if mut == "last_rg":
                keep = np.arange(ln) % rgs != rgs - 1
            mx = s[keep].max(0) if keep.any() else np.full(D, -np.inf)
            if npad and mut != "no_fill":
                mx = np.maximum(mx, FILL)
            E = np.exp(s - mx) * keep[:, None]
            fillt = npad * np.exp(FILL - mx) if (npad and mut != "no_fill") else np.zeros(D)
            ssum = E.sum(0) + fillt
            with np.errstate(divide="ignore", invalid="ignore"):
                pooled = (E * mw * z).sum(0) / ssum
            if not back:
                out["pooled"][n], out["smax"][n], out["ssum"][n] = pooled, mx, ssum
                if mut is None:
                    ew = ((mx - s) + 2 * (nr + 1)) * 2.0 ** -23 + 2 * (nr + rgs + 2) * U
                    assert (ew < 2.0 ** -10).all(), "the first-order bound needs ew < 2^-10"
                    e_z = (E * ew).sum(0) + fillt * (((mx - FILL) + 2) * 2.0 ** -23 + 3 * U)
                    out["b_ssum"][n] = e_z
                    out["b_pooled"][n] = ((E * mw * np.abs(z) * (ew + 2 * U)).sum(0) / ssum + np.abs(pooled) * e_z / ssum + 2 * U * np.abs(pooled)) * (1 + 2.0 ** -10)
                continue
            # backward
            gd = inp["dpooled" + sfx][n]
            if mode == "follow":
                fm, fz, fp = (fed[k + sfx][n].astype(np.float32) for k in ("smax", "ssum", "pooled"))
                g32 = gd.astype(np.float32)
                iz, gp = np.float32(1.0) / fz, g32 * fp
                w = _exp32(s.astype(np.float32) - fm) * iz
                d3, d2 = mw.astype(np.float32), Ms[r0:r0 + ln].astype(np.float32)
                dsv = w * (g32 * z.astype(np.float32) * d3 - gp) * d2
                dzv = g32 * w * d3
                assert dsv.dtype == np.float32 and dzv.dtype == np.float32
                ds[r0:r0 + ln], dz[r0:r0 + ln] = rnd16(dsv, fmt), rnd16(dzv, fmt)
                tot_add = tot_add + 0  # (the follow column sum is formed below from the fp32 ds)
                r.setdefault("_ds32", []).append(dsv)
                continue
            w = E / ssum
            ms_n = Ms[r0:r0 + ln]
            inner = gd * z * mw - gd * pooled
            dsv, dzv = w * inner * ms_n, gd * w * mw
            ds[r0:r0 + ln], dz[r0:r0 + ln] = dsv, dzv
            if mut == "pad_not_zeroed" and npad:
                ds[r0 + ln:r0 + Lp], dz[r0 + ln:r0 + Lp] = UNWRITTEN, UNWRITTEN
            if mut is None:
                x = np.abs(s - mx)
                if c["chained"]:
                    e_fz, e_fp = fed["b_ssum" + sfx][n] / ssum, fed["b_pooled" + sfx][n]
                else:
                    e_fz, e_fp = U, U * np.abs(pooled)
                ew = (x + 2) * 2.0 ** -23 + x * U + 3 * U + e_fz
                assert (ew < 2.0 ** -10).all(), "the first-order bound needs ew < 2^-10"
                e_ds = ms_n * (np.abs(w * inner) * (ew + 3 * U) + w * (2 * U * np.abs(gd * z * mw) + np.abs(gd) * e_fp + U * np.abs(gd * pooled))) * (1 + 2.0 ** -10)
                e_dz = np.abs(dzv) * (ew + 2 * U) * (1 + 2.0 ** -10)
                b_ds[r0:r0 + ln], b_dz[r0:r0 + ln] = e_ds + hulp(np.abs(dsv) + e_ds, fmt), e_dz + hulp(np.abs(dzv) + e_dz, fmt)
                tot_err = tot_err + e_ds.sum(0, keepdims=True)
            if not (mut == "partial_missing" and i == len(prs) - 1 and n == N - 1):
                tot_add = tot_add + dsv.sum(0, keepdims=True)
            r.setdefault("_abs", []).append(np.abs(dsv).sum(0, keepdims=True))
            nrows += ln
        if not back:
            for k in ("pooled", "smax", "ssum"):
                r[k + sfx] = out[k]
                if mut is None and mode == "exact":
                    r["b_" + k + sfx] = out["b_" + k]
            if c["copy"]:
                r["pooled_copy" + sfx] = out["pooled"]
                if mut is None and mode == "exact":
                    r["b_pooled_copy" + sfx] = out["b_pooled"]
        else:
            r["ds" + sfx], r["dz" + sfx] = ds, dz
            if mut is None and mode == "exact":
                r["b_ds" + sfx], r["b_dz" + sfx] = b_ds, b_dz
    if mut == "chan_shift":  # the second 8-channel chunk takes the third's results
        for k in list(r):
            if not k.startswith("_") and r[k].shape[1] == D and k != "ds_colsum":
                r[k] = r[k].copy()
                r[k][:, 8:16] = r[k][:, 16:24]
    if not back and c["counts"]:
        sfx = ("", "2")[len(prs) - 1]  # the items are the last segment
        r["pk_out"] = pack_rows(c, r["pooled" + sfx])
        _, mask, lens = O.pack_by_count(r["pooled" + sfx], np.asarray(c["counts"]), c["Cmax"])
        r["pk_mask"], r["pk_lens"] = mask.reshape(1, -1).astype(np.float64), np.asarray(lens, np.float64)[None]
        if mut == "pk_skip_empty":
            empty = np.repeat(np.asarray(c["counts"]) == 0, c["Cmax"])
            r["pk_out"][empty], r["pk_mask"][0, empty], r["pk_lens"][0, np.asarray(c["counts"]) == 0] = UNWRITTEN, UNWRITTEN, UNWRITTEN
        if mut is None and mode == "exact":
            r["b_pk_out"], r["b_pk_mask"], r["b_pk_lens"] = pack_rows(c, r["b_pooled" + sfx]), np.zeros_like(r["pk_mask"]), np.zeros_like(r["pk_lens"])
    if back and c["colsum"]:
        if mode == "follow":
            acc = inp["init_ds_colsum"][0].astype(np.float32)
            for dsv in r["_ds32"]:
                part = np.zeros((rgs, D), np.float32)
                for l in range(dsv.shape[0]):
                    part[l % rgs] = part[l % rgs] + dsv[l]
                v = np.zeros(D, np.float32)
                for g in range(rgs):
                    v = v + part[g]
                acc = acc + v
            r["ds_colsum"] = acc.astype(np.float64)[None]
        else:
            cs = tot_add
            if mut == "chan_shift":
                cs = cs.copy()
                cs[:, 8:16] = cs[:, 16:24]
            r["ds_colsum"] = (0.0 if mut == "colsum_overwrite" else inp["init_ds_colsum"]) + cs
            if mut is None:
                r["b_ds_colsum"] = tot_err + g_(nrows + 1) * (sum(r["_abs"]) + np.abs(inp["init_ds_colsum"]))
    for k in [k for k in r if k.startswith("_")]:
        del r[k]
    return r


def _others(c, inp, mode, mut, fmt):
    op, r = c["op"], {}
    if op in ("avg_fwd", "avg_bwd"):
        D, L, lens = c["D"], c["L"], np.asarray(c["lens"], np.float64)
        N = len(lens)
        if mut == "lens_next":
            lens = np.roll(lens, -1)
        if mut in ("len_plus", "len_minus"):
            lens = np.maximum(1, lens + (1 if mut == "len_plus" else -1))
        if op == "avg_fwd":
            z = inp["z"].reshape(N, L, D)
            if mode == "follow":
                a = np.zeros((N, D), np.float32)
                for l in range(L):
                    a = a + z[:, l].astype(np.float32)
                r["out"] = (a * (np.float32(1.0) / lens.astype(np.float32))[:, None]).astype(np.float64)
                return r
            zz = z * (np.arange(L)[None, :, None] < lens[:, None, None]) if mut == "avg_valid_only" else z
            r["out"] = zz.sum(1) / lens[:, None]
            r["b_out"] = ((L - 1) * U * np.abs(z).sum(1) / lens[:, None] + 3 * U * np.abs(r["out"])) * (1 + 2.0 ** -10)
        else:
            dp = inp["dpooled"]
            if mode == "follow":
                v = dp.astype(np.float32) * (np.float32(1.0) / lens.astype(np.float32))[:, None]
                r["dz"] = np.repeat(rnd16(v, fmt), L, axis=0)
                return r
            v = np.repeat(dp / lens[:, None], L, axis=0)
            if mut == "avg_valid_only":
                v[(np.arange(L)[None, :] >= lens[:, None]).ravel()] = UNWRITTEN  # only the valid rows written
            r["dz"] = v
            vv = np.repeat(dp / lens[:, None], L, axis=0)
            r["b_dz"] = 3 * U * np.abs(vv) + hulp(np.abs(vv) * (1 + 3 * U), fmt)
    elif op == "colsum":
        x, init = inp["x"], inp["init_out"]
        if mode == "follow":
            acc = init[0].astype(np.float32)
            for r0 in range(0, c["R"], 64):
                a = np.zeros(c["C"], np.float32)
                for row in x[r0:r0 + 64].astype(np.float32):
                    a = a + row
                acc = acc + a
            r["out"] = acc.astype(np.float64)[None]
            return r
        rows = x[:max(0, c["R"] - ((c["R"] - 1) % 64 + 1))] if mut == "partial_missing" else x  # the last workgroup's rows
        r["out"] = (0.0 if mut == "colsum_overwrite" else init) + rows.sum(0, keepdims=True)
        r["b_out"] = g_(c["R"] + 1) * (np.abs(x).sum(0, keepdims=True) + np.abs(init))
    else:  # pack: fp32 copies and additions, reproduced as such; every bound is zero
        counts = np.asarray(c["counts"])
        if op == "pack_fwd":
            emb = inp["emb"][:counts.sum()]
            out, mask, lens = O.pack_by_count(emb, counts, c["Cmax"])
            r["out"], r["mask"], r["lens"] = out.reshape(-1, c["D"]), mask.reshape(1, -1).astype(np.float64), lens.astype(np.float64)[None]
            if mut == "pk_skip_empty":
                empty = np.repeat(counts == 0, c["Cmax"])
                r["out"][empty], r["mask"][0, empty], r["lens"][0, counts == 0] = UNWRITTEN, UNWRITTEN, UNWRITTEN
        else:
            B, Cm, D = len(counts), c["Cmax"], c["D"]
            v = np.nan_to_num(inp["dout"]).astype(np.float32)
            if c.get("dout2"):
                v = v + np.nan_to_num(inp["dout2"]).astype(np.float32)
            un = O.unpack_by_count(v.reshape(B, Cm, D), counts)
            demb = inp["init_demb"].astype(np.float32).copy()
            demb[:counts.sum()] = (0 if mut == "colsum_overwrite" else demb[:counts.sum()]) + un
            r["demb"] = demb.astype(np.float64)
            if c.get("dctx"):
                r["demb_ctx"] = ((0 if mut == "colsum_overwrite" else inp["init_demb_ctx"].astype(np.float32)) + inp["dctx"].astype(np.float32)).astype(np.float64)
        for k in list(r):
            r["b_" + k] = np.zeros_like(r[k])
    return r


def reference(c, inp, ms, mode="exact", mut=None, fmt="bf16", fed=None):
    """mode "exact": the fp64 result per output and, without a mutation, the bounds "b_<output>".  mode "follow": rounded where the
    kernels round.  ms: masks(c, lib).  fed (pool_bwd): smax, ssum, pooled as the backward reads them (and the forward's bounds in a chained
    case).  mut: one of MUTATIONS, the wrong kernel the checker must reject; UNWRITTEN marks an element such a kernel leaves as it was."""
    op = c["op"]
    if op == "ln_fwd":
        return _ln_fwd(c, inp, ms["M"], mode, mut, fmt)
    if op == "ln_bwd":
        return _ln_bwd(c, inp, ms, mode, mut, fmt)
    if op in ("pool_fwd", "pool_bwd"):
        return _pool(c, inp, ms, mode, mut, fmt, fed)
    return _others(c, inp, mode, mut, fmt)


def forward_case(c):
    """The pool_fwd case of a pool_bwd case (same tensors, same seed words)."""
    return BY_NAME[c["name"][:-3] + "fwd"]


def pool_fed(c, lib, fmt="bf16", fwd_out=None):
    """What a pool_bwd case is fed: the exact forward's smax, ssum, pooled rounded to fp32, or (chained) the forward kernel's own outputs
    fwd_out with the forward's bounds."""
    f = forward_case(c)
    inp = inputs(f, fmt)
    ref = reference(f, inp, masks(f, lib), fmt=fmt)
    fed = {}
    for sfx in ("", "2")[:len(c["segs"])]:
        for k in ("smax", "ssum", "pooled"):
            fed[k + sfx] = f32(ref[k + sfx]) if fwd_out is None else fwd_out[k + sfx]
            fed["b_" + k + sfx] = ref["b_" + k + sfx]
    return fed


MUTATIONS = ("biased_var", "eps_in_sqrt", "std0_term", "mask_row", "mask_ld", "row0", "seed2", "lens_next", "len_plus", "len_minus", "no_fill",
             "last_rg", "chan_shift", "pad_not_zeroed", "partial_missing", "colsum_overwrite", "avg_valid_only", "pk_skip_empty")


def mutated(c, inp, lib, mut, fmt="bf16", fed=None):
    """The exact reference of a subtly wrong kernel, or None where the mutation provably changes nothing beyond the reference's own fp64
    rounding (without dropout2 every sequence's column sum of ds is zero: sum_l w_l (g z_l Mw_l - g pooled) = 0)."""
    if mut == "partial_missing" and c["op"] == "pool_bwd" and not c["p_s"] > 0:
        return None
    return reference(c, inp, masks(c, lib, mut if mut in ("mask_row", "mask_ld", "row0", "seed2") else None), mut=mut, fmt=fmt, fed=fed)


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def _encode(t, x, fmt):
    if t["kind"] == "h":
        return enc16(x, fmt)
    if t["kind"] == "f":
        return np.asarray(x, np.float64).astype(np.float32).view(np.uint32)
    return np.asarray(x, np.float64).astype(np.int64).astype(DT[t["kind"]])


def _decode(t, b, fmt):
    if t["kind"] == "h":
        return dec16(b, fmt)
    if t["kind"] == "f":
        return np.ascontiguousarray(b).view(np.float32).astype(np.float64)
    return b.astype(np.int64 if t["kind"] != "i32" else np.int32).astype(np.float64)


def nan_bits(t, fmt):
    return {"h": 0x7FC0 if fmt == "bf16" else 0x7E00, "f": 0x7FC00000}[t["kind"]]


def buffers(c, inp, res=None, fmt="bf16", fed=None):
    """Host images before the call: inputs with NaNs in guard rows, column gaps and the rows nobody may read; outputs full of sentinel bytes,
    accumulating ones with their initial contents in the window.  fed: values for input tensors that inputs() does not draw (pool_bwd's
    statistics).  With res: what a kernel that computes `res` would leave (UNWRITTEN in res: the element is not written)."""
    b = {}
    for nm, t in tensors(c).items():
        dt = np.dtype(DT[t["kind"]])
        img = np.full((GUARD + t["rows"] + GUARD, t["ld"]), SENT[dt] if t["role"] != "in" else nan_bits(t, fmt), dt)
        win = img[GUARD:GUARD + t["rows"], :t["cols"]]
        src = inp.get(nm) if t["role"] == "in" else inp.get("init_" + nm)
        if src is None and t["role"] == "in":
            src = fed[nm]
        if src is not None:
            win[t["rowmask"]] = _encode(t, src, fmt)[t["rowmask"]]
        if res is not None and t["role"] != "in":
            v = np.asarray(res[nm], np.float64)
            w = t["rowmask"][:, None] & ~np.isinf(v)
            with np.errstate(invalid="ignore"):
                win[w] = _encode(t, np.where(np.isinf(v), 0.0, v), fmt)[w]
        b[nm] = img
    return b


def window(c, nm):
    """(element offset of the tensor's first element in its buffer, ld)."""
    t = tensors(c)[nm]
    return GUARD * t["ld"], t["ld"]


# ---- checker ------------------------------------------------------------------------------------------------------------------------
def check(c, ref, got, before=None, fmt="bf16"):
    """got: the buffers after the call.  Returns (violations, worst |error| / bound per output); a violation is (output, element, got,
    reference, bound) for a value out of bound, unequal where the bound is zero or NaN, or (buffer, element, "sentinel" / "input") for a
    moved sentinel or a changed input."""
    T, bad, ratios = tensors(c), [], {}
    for nm, t in T.items():
        img = got[nm]
        inside = np.zeros(img.shape, bool)
        if t["role"] != "in":
            inside[GUARD:GUARD + t["rows"], :t["cols"]][t["rowmask"]] = True
            g = _decode(t, img[GUARD:GUARD + t["rows"], :t["cols"]], fmt)[t["rowmask"]]
            r, b = ref[nm][t["rowmask"]], ref["b_" + nm][t["rowmask"]]
            err = np.abs(g - r)
            with np.errstate(invalid="ignore"):
                wrong = np.isnan(g) | np.where(b == 0, g != r, err > b)
            for i, j in np.argwhere(wrong)[:4]:
                bad.append((nm, (int(i), int(j)), float(g[i, j]), float(r[i, j]), float(b[i, j])))
            if len(np.argwhere(wrong)) > 4:
                bad.append((nm, "more", int(wrong.sum()), 0.0, 0.0))
            nz = (b > 0) & ~np.isnan(g)
            ratios[nm] = float((err[nz] / b[nz]).max()) if nz.any() else 0.0
            moved = (img != SENT[img.dtype]) & ~inside
            if moved.any():
                bad.append((nm, tuple(int(v) for v in np.argwhere(moved)[0]), "sentinel"))
        elif before is not None and (img != before[nm]).any():
            bad.append((nm, tuple(int(v) for v in np.argwhere(img != before[nm])[0]), "input"))
    if c["op"] == "pool_fwd" and c["counts"]:  # the hand-over holds the very rows the kernel wrote to pooled
        sfx = ("", "2")[len(c["segs"]) - 1]
        t = T["pooled" + sfx]
        pooled = np.ascontiguousarray(got["pooled" + sfx][GUARD:GUARD + t["rows"], :t["cols"]]).view(np.float32)
        want = pack_rows(c, pooled).view(np.uint32)
        have = got["pk_out"][GUARD:-GUARD]
        if (have != want).any():
            bad.append(("pk_out", tuple(int(v) for v in np.argwhere(have != want)[0]), "differs from the pooled row"))
    return bad, ratios
