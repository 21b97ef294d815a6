"""Case table, fp64 references, a derived per-element bound and the checker of the attention kernel tests
(tests/test_gpu_attn.py runs the kernels through coot_debug_attn, tests/test_cpu_attn_cases.py tests this module without a GPU).

Operation (csrc/attention.hip; per sequence n and head h, scale = fp32(1 / sqrt(dh))):
  S = scale Q K^T;  S[:, k >= lens[n]] = -32752;  P = softmax over all Lk keys;  lse = log sum exp S;  Pd = P * M;  O = Pd V
with M the dropout keep-scales (0 or 1 / keep) of mask row (n H + h) Lq + q from the library's own host generator
(coot_debug_attn_dropout_scales; n counts within the segment, the second segment draws from seed + SEED2_DELTA, a packed sequence
has Lq = Lk = its own length).  All Lq query rows are computed, padded ones included.  Backward, closed form:
  dV = Pd^T dO;  dP = dO V^T;  g = M * dP - delta,  delta = sum_k P_k M_k dP_k (= <dO, O>);  dS = scale P g, 0 at filled keys;
  dQ = dS K;  dK = dS^T Q.
dK and dV of a filled key are exactly zero (its P underflows to 0 in fp64 as in fp32, lens >= 1).

Two references.  attn_reference(mode="exact") is the above in fp64 on the bf16 operands; the kernels are checked against it.
mode="follow" rounds where the kernels round and only shows that the bound is attainable: P * M to bf16 before P V and P^T dO
and dS to bf16 before it multiplies K or Q (short and chunked kernels; the one-query kernels keep them in fp32), delta = <dO,
bf16(O)> on the short and chunked paths and sum_k Pd_k dP_k on the one-query path, outputs to bf16, lse to fp32.

Bound (derived, not tuned), per element, with hulp(x) = half a bf16 ulp of x (2^-9 |x| .. 2^-8 |x|), e = 2^-24:
  ep   relative error of a recomputed probability in fp32: (dh + 2) e scale sum_c |q_c k_c| for the score, (|S - lse| + 2) 2^-23 for
       __expf (its argument is multiplied by log2 e in fp32, then v_exp_f32), + the same once per 64-key chunk the running maximum
       is rescaled over (chunked forward), + the error of the lse the backward is given (half an fp32 ulp of the fed one; the
       forward's bound in a chained case)
  o    sum_k hulp(Pd_k) |V_kc|  (the kernels round exp(S - max) M: hulp of that over the sum; 2^-8 Pd_k where the maximum is a
       running one)  + sum_k Pd_k ep_k |V_kc| + (sum_k P_k ep_k + (2 Lk + 4) e) sum_k Pd_k |V_kc|  (normaliser, fp32 sums)
       + hulp(o) for the store
  lse  sum_k P_k ep_k + Lk e + (log sum_k exp(S_k - max) + 1) 2^-22 (__logf) + 2^-23 (|max| + |lse|), absolute
  dS   E_qk = |dS| ep + scale P ((dh + 3) e (M sum_c |dO_c V_kc| + sum_c |dO_c O_c|) + R_q) + hulp(dS), with the delta residue
       R_q = sum_c |dO_c O_c| 2^-9 (O is fed as bf16; the forward's bound on O in a chained case); 0 at filled keys
  dq   sum_k E_qk |K_kc| + Lk e sum_k |dS_qk K_kc| + hulp(dq);   dk   the same over q with |Q_qc|
  dv   sum_q (hulp(Pd_qk) + Pd_qk ep_qk) |dO_qc| + Lq e sum_q Pd_qk |dO_qc| + hulp(dv)
The bound is a function of the operands and shapes alone (the one-query kernels, which round less, are held to the same terms;
"running maximum" is decided by family_of, the launcher's own rule).  Where it is zero (dK, dV of filled keys) the result must
be zero.  The delta residue is written with 2^-9, not with hulp(O) <= 2^-8 |O|: a sum over dh channels of roundings of either
sign, and test_cpu_attn_cases.py shows the kernel-following reference inside the bound on every case (worst 0.999: dv with one
query row, where hulp(Pd) |dO| + hulp(dv) is met by two roundings of one product).

Untouched memory.  Inputs and outputs are column windows of wider matrices with 3 guard rows above and below; guard rows, column
gaps and the rows between packed sequences hold bf16 NaNs on the input side and SENTINEL bytes on the output side, and every
sentinel must survive the call.
"""
import ctypes as C
import math
import zlib

import numpy as np

from tests.helpers import from_bf16_bits, to_bf16_bits

EPS32 = 2.0 ** -24
FILL = -32752.0
SENT16, SENT32, NAN16 = 0xA5A5, 0xA5A5A5A5, 0x7FC0
GUARD = 3
SITE = 16 * 3 + 1  # a layer's attention site word (api.hip: site_base + SITE_ATTN); any value would do
SEED2_DELTA = 0x9E3779B97F4A7C15  # csrc/attention.h: kAttnSeed2Delta
OUTPUTS = dict(fwd=("o", "lse"), bwd=("dq", "dk", "dv"))


def family_of(Lq, Lk, Nseq2=0, L2=0):
    """launch_attn_fwd / launch_attn_bwd's choice of kernels (attn_q1_ok, attn_short_ok in csrc/attention.hip)."""
    if Lq == 1 and 1 <= Lk <= 64 and Nseq2 == 0:
        return "q1"
    if Lq == Lk and 1 <= Lk <= 128 and (Nseq2 == 0 or 1 <= L2 <= 128):
        return "short"
    return "chunked"


def _lens4(L):
    """1, L - 1, L and a value that ends inside a 16-key tile."""
    mid = 16 * (L // 32) + 5 if L > 21 else max(1, L // 2)
    return [1, max(1, L - 1), L, mid]


def _case(name, **kw):
    c = dict(name=name, kind="self", H=2, dh=16, Nseq=3, Lq=0, Lk=0, lens=None, Nseq2=0, L2=0, lens2=None, packed=False, p=0.0,
             wide=False, shared=False, chained=False, xcd=None)
    bad = set(kw) - set(c)
    assert not bad, bad
    c.update(kw)
    if c["kind"] == "self":
        c["Lq"] = c["Lk"]
    c["Nseq"] = len(c["lens"])
    c["Nseq2"] = len(c["lens2"]) if c["lens2"] else 0
    c["family"] = family_of(c["Lq"], c["Lk"], c["Nseq2"], c["L2"])
    c["seed"] = zlib.crc32(name.encode()) & 0x7FFFFFFF
    assert all(1 <= l <= c["Lk"] for l in c["lens"]) and all(1 <= l <= c["L2"] for l in (c["lens2"] or []))
    assert c["Nseq"] + c["Nseq2"] <= 11 and not (c["packed"] and c["family"] != "short")
    return c


def _cases():
    cs = []
    DH = (16, 32, 48, 64)
    # short self-attention: one workgroup per (sequence, head), ceil(L / 16) waves
    for i, L in enumerate((2, 15, 16, 17, 33, 80, 127, 128)):
        cs.append(_case(f"short-L{L}", Lk=L, dh=DH[i % 4], lens=_lens4(L)))
    n9 = [33, 1, 32, 21, 16, 17, 5, 33, 28]  # 9 sequences in a grid padded to 16, 3 heads: idle workgroups, H no power of two
    cs.append(_case("short-n9h3", Lk=33, H=3, dh=16, lens=n9))
    cs.append(_case("short-n9h3-xcd0", Lk=33, H=3, dh=16, lens=n9, xcd=0))
    cs.append(_case("short-drop", Lk=80, dh=32, lens=_lens4(80), p=0.1))
    cs.append(_case("short-shared", Lk=80, dh=64, lens=_lens4(80), shared=True))
    cs.append(_case("short-chained", Lk=33, dh=48, lens=_lens4(33), chained=True))
    cs.append(_case("short-wide", Lk=17, dh=32, lens=_lens4(17), wide=True))
    # chunked self-attention: 64 query rows per workgroup, 64-key chunks; lens end in the first, a middle and the last chunk
    for i, L in enumerate((129, 150, 192, 193)):
        cs.append(_case(f"chunked-L{L}", Lk=L, dh=DH[i % 4], lens=[37, 100, L]))
    cs.append(_case("chunked-drop", Lk=150, dh=64, lens=[37, 100, 150], p=0.1))
    cs.append(_case("chunked-shared", Lk=129, dh=32, lens=[37, 100, 129], shared=True))
    cs.append(_case("chunked-chained", Lk=150, dh=16, lens=[37, 100, 149], chained=True))
    # one query per sequence (the context block): q its own matrix, k | v one matrix with ld = 2 D
    for i, Lk in enumerate((1, 20, 63, 64, 65, 130)):
        lens = [1] * 5 if Lk == 1 else [1, Lk - 1, Lk, max(1, Lk // 2 + 3), Lk]
        cs.append(_case(f"cross-Lk{Lk}", kind="cross", Lq=1, Lk=Lk, dh=DH[i % 4], lens=lens))
    cs.append(_case("self-L1", Lk=1, dh=48, lens=[1, 1, 1]))  # self-attention that satisfies attn_q1_ok
    cs.append(_case("cross-drop", kind="cross", Lq=1, Lk=20, dh=64, lens=[1, 19, 20, 13, 7], p=0.1))
    cs.append(_case("cross-shared", kind="cross", Lq=1, Lk=64, dh=16, lens=[64, 63, 35, 64, 50], shared=True))
    cs.append(_case("cross-chained", kind="cross", Lq=1, Lk=63, dh=32, lens=[1, 62, 63, 34, 20], chained=True))
    cs.append(_case("cross-Lk130-drop", kind="cross", Lq=1, Lk=130, dh=48, lens=[1, 129, 130, 70, 64], p=0.1))
    # two segments in one launch of the short kernels, 5 + 6 sequences, the workgroup sized by the longer segment
    cs.append(_case("seg2-80-80", Lk=80, L2=80, dh=64, lens=[80, 1, 37, 79, 64], lens2=[5, 80, 48, 17, 1, 66]))
    cs.append(_case("seg2-20-80-drop", Lk=20, L2=80, dh=16, lens=[20, 1, 13, 19, 16], lens2=[80, 33, 1, 79, 64, 21], p=0.1))
    cs.append(_case("seg2-64-16", Lk=64, L2=16, dh=48, lens=[64, 1, 37, 63, 48], lens2=[16, 1, 15, 8, 16, 3]))
    # packed rows: sequence n starts at row cu[n] and has lens[n] rows (0 .. 2 unused rows between the sequences)
    cs.append(_case("packed-1seg", Lk=33, dh=32, lens=[1, 33, 16, 17, 32, 5, 21], packed=True))
    cs.append(_case("packed-2seg", Lk=20, L2=80, dh=48, lens=[20, 1, 13, 19, 16], lens2=[80, 33, 1, 79, 64, 21], packed=True))
    cs.append(_case("packed-2seg-drop", Lk=80, L2=20, dh=64, lens=[80, 33, 1, 79, 21], lens2=[20, 1, 13, 19, 16, 7], packed=True, p=0.1))
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- rows and columns -----------------------------------------------------------------------------------------------------------
def sequences(c):
    """One dict per sequence of the launch: segment, index within it, first query / key row, Lq, Lk (rows it owns), valid keys,
    dropout seed."""
    out, row = [], 0
    for seg, (N, L, lens) in enumerate(((c["Nseq"], c["Lk"], c["lens"]), (c["Nseq2"], c["L2"], c["lens2"] or []))):
        for n in range(N):
            Lk = lens[n] if c["packed"] else L
            Lq = 1 if c["kind"] == "cross" else Lk
            out.append(dict(seg=seg, n=n, qr0=len(out) if c["kind"] == "cross" else row, Lq=Lq, kr0=row, Lk=Lk, nvalid=lens[n],
                            seed=(c["seed"] + seg * SEED2_DELTA) & (2 ** 64 - 1)))
            row += Lk + ((len(out) % 3) if c["packed"] else 0)
    return out


def layout(c):
    """Buffers name -> (rows, ld, is_output) and operand -> (buffer, first column, ld); Tq / Tk query / key rows."""
    D = c["H"] * c["dh"]
    sq = sequences(c)
    Tk = sq[-1]["kr0"] + sq[-1]["Lk"]
    Tq = len(sq) if c["kind"] == "cross" else Tk
    if c["kind"] == "cross":
        bufs = dict(qin=(Tq, D, 0), kvin=(Tk, 2 * D, 0), oo=(Tq, D + 8, 1), doo=(Tq, D + 8, 0), dqo=(Tq, D + 8, 1), dkvo=(Tk, 2 * D, 1))
        ops = dict(q=("qin", 0), k=("kvin", 0), v=("kvin", D), o=("oo", 0), dout=("doo", 0), dq=("dqo", 0), dk=("dkvo", 0), dv=("dkvo", D))
    else:
        g = 8 if c["wide"] else 0  # a column gap between q | k | v and between dq | dk | dv
        bufs = dict(qkv=(Tk, 3 * D + 3 * g, 0), oo=(Tq, D + 8, 1), doo=(Tq, D + 8 + g, 0), dqkv=(Tk, 3 * D + 3 * g, 1))
        ops = dict(q=("qkv", 0), k=("qkv", D + g), v=("qkv", 2 * D + 2 * g), o=("oo", 0), dout=("doo", 0),
                   dq=("dqkv", 0), dk=("dqkv", D + g), dv=("dqkv", 2 * D + 2 * g))
    qrows, krows = np.zeros(Tq, bool), np.zeros(Tk, bool)
    for s in sq:
        qrows[s["qr0"]:s["qr0"] + s["Lq"]] = True
        krows[s["kr0"]:s["kr0"] + s["Lk"]] = True
    return dict(D=D, Tq=Tq, Tk=Tk, bufs=bufs, ops={k: (b, col, bufs[b][1]) for k, (b, col) in ops.items()}, qrows=qrows, krows=krows)


def _bf(x):
    return from_bf16_bits(to_bf16_bits(x)).astype(np.float64)


def attn_inputs(c):
    """q, k, v, dout as fp64 arrays of bf16 values, [Tq or Tk, D]; dout is random on every query row, padded ones included."""
    rs = np.random.RandomState(c["seed"])
    L = layout(c)
    D, Tq, Tk = L["D"], L["Tq"], L["Tk"]
    k = rs.randn(Tk, D)
    if c["shared"]:  # keys with a large common component (|c| about 2 per channel): the hard case for delta, see attention.hip
        k = np.where(rs.rand(D) < 0.5, -1.0, 1.0) * (2.0 + 0.25 * rs.randn(D)) + 0.25 * k
    return dict(q=_bf(rs.randn(Tq, D)), k=_bf(k), v=_bf(rs.randn(Tk, D)), dout=_bf(rs.randn(Tq, D)))


def drop_masks(c, lib, row_shift=0, same_seed=False):
    """Per sequence the keep-scales [H, Lq, Lk] of the library's host generator (None without dropout)."""
    if not c["p"] > 0:
        return [None] * len(sequences(c))
    lib.coot_debug_attn_dropout_scales.argtypes = [C.c_uint64, C.c_uint, C.c_uint, C.c_int, C.c_float, C.c_void_p]
    out = []
    for s in sequences(c):
        m = np.empty((c["H"], s["Lq"], s["Lk"]), np.float32)
        for h in range(c["H"]):
            for q in range(s["Lq"]):
                row = (s["n"] * c["H"] + h) * s["Lq"] + q + row_shift
                rc = lib.coot_debug_attn_dropout_scales(c["seed"] if same_seed else s["seed"], SITE, row, s["Lk"], c["p"], m[h, q].ctypes.data)
                assert rc == 0
        out.append(m.astype(np.float64))
    return out


# ---- references and bound -----------------------------------------------------------------------------------------------------------
def hulp(x):
    """Half a bf16 ulp at magnitude |x| (0 at 0)."""
    m, e = np.frexp(np.abs(x))
    return np.where(m > 0, np.ldexp(1.0, e - 9), 0.0)


def _heads(x, r0, n, H, dh):
    return x[r0:r0 + n].reshape(n, H, dh).transpose(1, 0, 2)  # [H, n, dh]


def _rows(x):
    return x.transpose(1, 0, 2).reshape(x.shape[1], -1)  # [H, n, dh] -> [n, H dh]


def attn_reference(c, inp, masks, mode="exact", mut=None, fed=None):
    """mode "exact": the fp64 result dict(o, lse, dq, dk, dv) and, without a mutation, the bounds b_o, b_lse, b_dq, b_dk, b_dv.
    mode "follow": rounded where the kernels round (fed: the o / lse the backward reads; default: the exact ones, rounded).
    mut: one of MUTATIONS, the wrong kernels the checker must reject (exact mode)."""
    H, dh, fam = c["H"], c["dh"], c["family"]
    L = layout(c)
    D, Tq, Tk = L["D"], L["Tq"], L["Tk"]
    scale = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
    sq = sequences(c)
    follow, bound = mode == "follow", mode == "exact" and mut is None
    r = dict(o=np.zeros((Tq, D)), lse=np.zeros((Tq, H)), dq=np.zeros((Tq, D)), dk=np.zeros((Tk, D)), dv=np.zeros((Tk, D)))
    if bound:
        r.update({"b_" + k: np.zeros_like(v) for k, v in list(r.items())})
    if follow and fed is None:
        ex = attn_reference(c, inp, masks)
        fed = dict(o=_bf(ex["o"]), lse=ex["lse"].astype(np.float32).astype(np.float64))
    for i, s in enumerate(sq):
        Lq, Lk, nv = s["Lq"], s["Lk"], s["nvalid"]
        if mut in ("lens_plus", "lens_minus") and not c["packed"]:
            nv = min(Lk, nv + 1) if mut == "lens_plus" else max(1, nv - 1)
        if mut == "lens_minus" and c["packed"]:
            nv = max(1, nv - 1)
        if mut == "lens_next":  # sequence n reads lens[n + 1] (the last one of a segment the first one's)
            seg = [t for t in sq if t["seg"] == s["seg"]]
            nv = min(Lk, seg[(s["n"] + 1) % len(seg)]["nvalid"])
        q, k, v, do = (_heads(inp[x], s["qr0"] if x in ("q", "dout") else s["kr0"], Lq if x in ("q", "dout") else Lk, H, dh) for x in ("q", "k", "v", "dout"))
        M = masks[i] if masks[i] is not None else np.ones((H, Lq, Lk))
        filled = np.arange(Lk) >= nv
        S = scale * (q @ k.transpose(0, 2, 1))
        S[:, :, filled] = FILL
        mx = S.max(-1, keepdims=True)
        E = np.exp(S - mx)
        ssum = E.sum(-1, keepdims=True)
        P, lse = E / ssum, (mx + np.log(ssum))[..., 0]
        Pd = P * M
        wk = np.ones(Lk)
        if mut == "skip_tile":  # the 16-key tile that holds the last valid key is left out of P V and dS K
            t = (nv - 1) // 16
            wk[16 * t:16 * t + 16] = 0.0
        if follow and fam != "q1":
            o = _bf((_bf(E * M) * wk) @ v / ssum)
        else:
            o = (Pd * wk) @ v
        if mut == "lse_max":
            lse = mx[..., 0]
        # ---- backward
        dP = do @ v.transpose(0, 2, 1)
        dPd = dP * M
        if follow:
            o_in, lse_in = _heads(fed["o"], s["qr0"], Lq, H, dh), fed["lse"][s["qr0"]:s["qr0"] + Lq].T
            Pb = np.exp(S - lse_in[..., None])
            Pdb = Pb * M
            delta = (Pdb * dP).sum(-1) if fam == "q1" else (do * o_in).sum(-1)
            ds = scale * Pb * (dPd - delta[..., None])
            ds[:, :, filled] = 0.0
            if fam != "q1":
                ds, Pdb = _bf(ds), _bf(Pdb)
            dq, dk, dv = ds @ k, ds.transpose(0, 2, 1) @ q, Pdb.transpose(0, 2, 1) @ do
        else:
            delta = (P * dPd).sum(-1)
            ds = scale * P * (dPd - delta[..., None])
            ds[:, :, filled] = 0.0
            wq = np.ones(Lq)
            if mut == "pad_q_dropped" and c["kind"] == "self":  # padded query rows left out of dK and dV
                wq[nv:] = 0.0
            sc = 1.0 / scale if mut == "no_scale" else 1.0
            dq = sc * (ds * wk) @ k
            dk = sc * (ds * wq[:, None]).transpose(0, 2, 1) @ q
            dv = ((P if mut == "dv_nomask" else Pd) * wq[:, None]).transpose(0, 2, 1) @ do
            if mut == "dk_filled" and filled.any():
                dk[0, int(np.argmax(filled)), 0] = 2.0 ** -20
        res = dict(o=o, dq=dq, dk=dk, dv=dv)
        if mut == "swap_heads":
            res = {x: np.concatenate([y[1:2], y[0:1], y[2:]]) for x, y in res.items()}
            lse = np.concatenate([lse[1:2], lse[0:1], lse[2:]])
        for x, y in res.items():
            r0, n = (s["qr0"], Lq) if x in ("o", "dq") else (s["kr0"], Lk)
            r[x][r0:r0 + n] = _rows(y)
        r["lse"][s["qr0"]:s["qr0"] + Lq] = lse.T
        if not bound:
            continue
        # ---- the bound (module docstring)
        aq, ak, av, ado = np.abs(q), np.abs(k), np.abs(v), np.abs(do)
        nch = (Lk - 1) // 64 if fam == "chunked" else 0  # rescalings of the running maximum
        Sv = np.where(filled, np.nan, S)
        rng = (np.nanmax(Sv, -1) - np.nanmin(Sv, -1))[..., None]
        x = np.where(filled, 0.0, np.abs(S - lse[..., None]))
        Es = (dh + 2) * EPS32 * scale * (aq @ ak.transpose(0, 2, 1))
        epf = np.where(filled, 0.0, Es + (x + 2 + nch * (rng + 2)) * 2.0 ** -23)
        Ao = Pd @ av
        hP = hulp(E * M * (1 + epf)) / ssum if nch == 0 else 2.0 ** -8 * Pd
        t_o = hP @ av + (Pd * epf) @ av + ((P * epf).sum(-1, keepdims=True) + (2 * Lk + 4) * EPS32) * Ao
        b_o = t_o + hulp(np.abs(o) + t_o)
        b_lse = (P * epf).sum(-1) + Lk * EPS32 + (np.log(ssum[..., 0]) + 1) * 2.0 ** -22 + 2.0 ** -23 * (np.abs(mx[..., 0]) + np.abs(lse))
        e_lse = b_lse if c["chained"] else EPS32 * np.abs(lse)
        e_o = b_o if c["chained"] else 2.0 ** -9 * np.abs(o)
        epb = np.where(filled, 0.0, Es + (x + 2) * 2.0 ** -23 + e_lse[..., None])
        AdP, AdO, R = ado @ av.transpose(0, 2, 1), (ado * np.abs(o)).sum(-1)[..., None], (ado * e_o).sum(-1)[..., None]
        Eds = np.where(filled, 0.0, np.abs(ds) * epb + scale * P * ((dh + 3) * EPS32 * (M * AdP + AdO) + R))
        T = Eds + hulp(np.abs(ds) + Eds)
        t_dq = T @ ak + Lk * EPS32 * (np.abs(ds) @ ak)
        t_dk = T.transpose(0, 2, 1) @ aq + Lq * EPS32 * (np.abs(ds).transpose(0, 2, 1) @ aq)
        t_dv = (hulp(Pd * (1 + epb)) + Pd * epb).transpose(0, 2, 1) @ ado + Lq * EPS32 * (Pd.transpose(0, 2, 1) @ ado)
        for x, t, y in (("o", t_o, o), ("dq", t_dq, dq), ("dk", t_dk, dk), ("dv", t_dv, dv)):
            r0, n = (s["qr0"], Lq) if x in ("o", "dq") else (s["kr0"], Lk)
            r["b_" + x][r0:r0 + n] = _rows(t + hulp(np.abs(y) + t))
        r["b_lse"][s["qr0"]:s["qr0"] + Lq] = b_lse.T
    return r


MUTATIONS = ("lens_plus", "lens_minus", "pad_q_dropped", "no_scale", "skip_tile", "swap_heads", "mask_row", "seed2", "dv_nomask",
             "lens_next", "lse_max", "dk_filled")


def mutated(c, inp, lib, mut):
    """The exact reference of a subtly wrong kernel (mask_row: the dropout mask of the next mask row; seed2: segment 2 draws from
    segment 1's key; the rest: attn_reference), or None where the mutation does not apply to the case."""
    if mut in ("mask_row", "seed2"):
        if not c["p"] > 0 or (mut == "seed2" and not c["Nseq2"]):
            return None
        return attn_reference(c, inp, drop_masks(c, lib, row_shift=int(mut == "mask_row"), same_seed=mut == "seed2"), mut=mut)
    return attn_reference(c, inp, drop_masks(c, lib), mut=mut)


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def _image(rows, ld, fill):
    return np.full((GUARD + rows + GUARD, ld), fill, np.uint16)


def _put(img, col, x, rowmask):
    w = img[GUARD:GUARD + x.shape[0], col:col + x.shape[1]]
    w[rowmask] = to_bf16_bits(x)[rowmask]


def buffers(c, inp, fed=None, res=None, direction=None):
    """Host images before the call: inputs (NaN in guard rows, gaps and unused rows), sentinel-filled outputs; `fed` (o, lse as the
    backward reads them) is placed in the o / lse buffers.  With res and direction: what a kernel that computes `res` would leave."""
    L = layout(c)
    b = {name: _image(rows, ld, SENT16 if is_out else NAN16) for name, (rows, ld, is_out) in L["bufs"].items()}
    for x in ("q", "k", "v", "dout"):
        _put(b[L["ops"][x][0]], L["ops"][x][1], inp[x], L["qrows"] if x in ("q", "dout") else L["krows"])
    b["lse"] = np.full((GUARD + L["Tq"] + GUARD, c["H"]), SENT32, np.uint32)
    src = dict(fed or {})
    if res is not None:
        src.update({x: res[x] for x in OUTPUTS[direction]})
    for x, y in src.items():
        if x == "lse":
            b["lse"][GUARD:GUARD + L["Tq"]][L["qrows"]] = y.astype(np.float32).view(np.uint32)[L["qrows"]]
        else:
            _put(b[L["ops"][x][0]], L["ops"][x][1], y, L["qrows"] if x in ("o", "dq") else L["krows"])
    return b


def operand_offset(c, x):
    """Element offset of operand x's first element in its buffer, and its ld."""
    _, col, ld = layout(c)["ops"][x]
    return GUARD * ld + col, ld


# ---- checker --------------------------------------------------------------------------------------------------------------------
def attn_check(c, ref, got, direction, before=None):
    """got: the buffers after the call.  Raises AssertionError on a moved sentinel, a NaN, a nonzero where the bound is zero or an
    element out of bound; returns the worst |error| / bound per output of the direction.  before: the buffers as they were before
    the call (inputs and the outputs of the other direction must not have changed)."""
    L = layout(c)
    outs = OUTPUTS[direction]
    ratios = {}
    touched = {}
    for x in outs:
        rows = L["qrows"] if x in ("o", "dq", "lse") else L["krows"]
        if x == "lse":
            raw, win = got["lse"], got["lse"][GUARD:GUARD + L["Tq"]]
            val = win.view(np.float32).astype(np.float64)
            name = "lse"
        else:
            name, col, _ = L["ops"][x]
            raw, win = got[name], got[name][GUARD:GUARD + len(rows), col:col + L["D"]]
            val = from_bf16_bits(win).astype(np.float64)
        m = touched.setdefault(name, np.zeros(raw.shape, bool))
        mw = m[GUARD:GUARD + len(rows)] if x == "lse" else m[GUARD:GUARD + len(rows), col:col + L["D"]]
        mw[rows] = True
        r, b, g = ref[x][rows], ref["b_" + x][rows], val[rows]
        assert not np.isnan(g).any(), f"{c['name']}: {x} has {int(np.isnan(g).sum())} NaNs"
        zero = b == 0
        assert (r[zero] == 0).all()
        assert (g[zero] == 0).all(), f"{c['name']}: {x} is nonzero at {int((g[zero] != 0).sum())} elements that must be zero (filled keys)"
        err = np.abs(g - r)
        ok = err <= b
        if not ok.all():
            i, j = np.argwhere(~ok)[0]
            raise AssertionError(f"{c['name']}: {x}[{i},{j}] = {g[i, j]!r}, reference {r[i, j]!r}, |error| {err[i, j]:.3e} > bound {b[i, j]:.3e} "
                                 f"({int((~ok).sum())} elements out of bound)")
        ratios[x] = float((err[~zero] / b[~zero]).max()) if (~zero).any() else 0.0
    for name, m in touched.items():
        sent = SENT32 if name == "lse" else SENT16
        moved = (got[name] != sent) & ~m
        assert not moved.any(), f"{c['name']}: {int(moved.sum())} sentinels of buffer {name} moved, first at {tuple(np.argwhere(moved)[0])}"
    if before is not None:
        for name in before:
            if name not in touched:
                assert (got[name] == before[name]).all(), f"{c['name']}: buffer {name} changed"
    return ratios


def dq_cosine(c, ref, got):
    L = layout(c)
    name, col, _ = L["ops"]["dq"]
    g = from_bf16_bits(got[name][GUARD:GUARD + L["Tq"], col:col + L["D"]]).astype(np.float64)[L["qrows"]].ravel()
    r = ref["dq"][L["qrows"]].ravel()
    return float(g @ r / math.sqrt((g @ g) * (r @ r)))
