"""Case tables, an fp64 reference with a derived per-element bound, and the checker of the GEMM kernel tests
(tests/test_gpu_gemm.py runs the kernels, tests/test_cpu_gemm_cases.py tests this module without a GPU).

gemm_nt (csrc/gemm.hip, reached through coot_debug_gemm_nt: the whole GemmNT / GemmEpi descriptor the networks use).
Reference: fp64 on the bf16-rounded operands, following epilogue8 / epilogue4 step by step:
  1 v = acc + bias   2 v *= dropout scale (act != 2)   3 save_pre = bf16(v)   4 act 1: v = gelu(v)   5 v += pe[pos]   6 v += res
  7 act 2: v *= gelu'(aux) * dropout scale   8 out = v   9 colsum += column sums of v (the fp32 value, before a bf16 store).
The kernel keeps the unrounded fp32 v after step 3, so does the reference.  Dropout scales come from the library's own host
generator (coot_debug_dropout_scales) at element index row * drop_ld + z * zOut + col; GELU and its derivative are the erf forms.

Bound (derived, not tuned).  Next to every value the reference carries its magnitude companion A: the same formula with every
operand and intermediate replaced by its magnitude and |gelu'| by its maximum 1.13.  An fp32 output element may differ by
  K * 2^-24 * A      the IEEE worst case of an fp32 sum of K exact products in any order (a bf16 x bf16 product is exact in fp32)
                     plus the few epilogue operations, which K >= 8 covers
  + 1.25e-5 * |v|    common.h: the erfc approximation is within 2.5e-5 on erf, 1.25e-5 on Phi; v = the value that enters GELU
                     (act 1) or that gelu' multiplies (act 2, times the dropout scale).
A bf16 output and save_pre add half a bf16 ulp of the reference, <= 2^-8 |ref|.  colsum (the kernel ADDS to what the buffer holds,
so that value is an operand and its magnitude is part of A): (M + K) * 2^-24 * (|before| + column sum of A) + the column sum of
the GELU terms.  gemm_tn: T * 2^-24 * (|C before| + |A|^T |B|), the bias-gradient column sum T * 2^-24 * (|before| + sum |A|).

Untouched memory.  Every output-side buffer has ld = width + 8 and 16 rows below M and is filled with SENTINEL bytes; after the
call every byte outside the [M, N] window of each group must still be the sentinel.  Input paddings hold bf16 NaNs: a read past a
row poisons the result.
"""
import ctypes as C
import math
import zlib

import numpy as np

from oracle.coot_oracle import gelu, gelu_grad
from tests.helpers import from_bf16_bits, to_bf16_bits

EPS32 = 2.0 ** -24
GELU_ERR = 1.25e-5
GELU_GRAD_MAX = 1.13
SENT16, SENT32 = 0xA5A5, 0xA5A5A5A5
NAN16 = 0x7FC0
ROWS_BELOW = 16
PAD_OUT = 8
DROP_SITE = 16 * 15 + 5  # the site word of the pooler's first dropout (api.hip); any value would do


def _ceil(a, b):
    return (a + b - 1) // b


def nt_variant(M, N, groups=1):
    """launch_gemm_nt's choice of kernel (csrc/gemm.hip)."""
    if M <= 512:
        return "small2" if _ceil(M, 16) * _ceil(N, 32) >= 512 else "small1"
    return "main128" if _ceil(M, 128) * _ceil(N, 128) * groups >= 384 else "main64"


def nt_row_block(case):
    return {"small1": 16, "small2": 16, "main64": 64, "main128": 128}[case["variant"]]


def _case(name, M, N, K, **kw):
    c = dict(name=name, M=M, N=N, K=K, groups=1, bias=True, act=0, out_f32=False, save_pre=False, pe=None, res=False, inplace=False,
             aux=False, colsum=False, part_ws=False, p=0.0, strided=False, xcd=None, control=False)
    bad = set(kw) - set(c)
    assert not bad, bad
    c.update(kw)
    c["aux"] = c["aux"] or c["act"] == 2
    c["variant"] = nt_variant(M, N, c["groups"])
    c["seed"] = zlib.crc32(name.encode()) & 0x7FFFFFFF
    assert N % 8 == 0 and K % 8 == 0 and not (c["inplace"] and (c["out_f32"] or not c["res"]))
    return c


def _nt_cases():
    cs = []
    # the six shapes of tests/test_gpu_kernels.py::test_gemm_nt (held to 2e-5 of max|ref| there): the controls of the bound; those
    # with a bf16 output run a second time with an fp32 output, where the ratio is that of the accumulation + GELU terms alone
    for M, N, K, act, res, f32 in [(128, 128, 64, 0, False, True), (300, 200, 72, 1, True, False), (1000, 384, 384, 0, True, False),
                                   (4096, 1152, 384, 0, False, False), (77, 768, 384, 1, False, True), (2560, 384, 2048, 1, False, False)]:
        cs.append(_case(f"ctl-{M}x{N}x{K}", M, N, K, act=act, res=res, out_f32=f32, control=True))
        if not f32:
            cs.append(_case(f"ctl-{M}x{N}x{K}-f32", M, N, K, act=act, res=res, out_f32=True, control=True))
    # 1. launch variants and their boundaries, bias + bf16 out and again fp32 out
    for M, N, K, g in [(16, 8, 136, 1), (77, 200, 136, 1), (512, 480, 136, 1), (512, 512, 136, 1), (500, 520, 136, 1), (513, 136, 136, 1),
                       (1000, 384, 136, 1), (2944, 2048, 64, 1), (3064, 2040, 64, 1), (3064, 2048, 64, 1), (3100, 2048, 64, 1), (520, 1280, 64, 8)]:
        for f32 in (False, True):
            cs.append(_case(f"var-{M}x{N}x{K}-g{g}-{'f32' if f32 else 'bf16'}", M, N, K, groups=g, out_f32=f32))
    # 2. K tails: the LDS-staged kernels step by 64, the small ones by 32 in batches of 6 (192)
    for K in (8, 56, 64, 72, 136):
        cs.append(_case(f"k-main64-{K}", 513, 136, K, out_f32=True))
        cs.append(_case(f"k-main128-{K}", 520, 1280, K, groups=8, out_f32=True))
    for K in (8, 40, 184, 192, 200, 392):
        cs.append(_case(f"k-small1-{K}", 77, 200, K, out_f32=True))
        cs.append(_case(f"k-small2-{K}", 500, 520, K, out_f32=True))
    # 3. strides (ldx = K + 8, ldw = K + 16, ldres = N + 24, ldaux = ldpre = ldc = N + 8), one forward-style and one backward-style
    # epilogue per variant
    for tag, M, N, K, g in [("small1", 77, 200, 136, 1), ("small2", 500, 520, 136, 1), ("main64", 513, 136, 136, 1), ("main128", 520, 1280, 64, 8)]:
        cs.append(_case(f"ld-{tag}-fwd", M, N, K, groups=g, act=1, save_pre=True, res=True, strided=True))
        cs.append(_case(f"ld-{tag}-bwd", M, N, K, groups=g, bias=False, act=2, res=True, out_f32=True, strided=True))
    # 4. epilogues, on a small-kernel and a main-kernel shape with row and column tails
    for tag, M, N, K, pe in [("s", 77, 200, 136, (5, 37, 7)), ("m", 1000, 392, 136, (20, 613, 13))]:
        cs.append(_case(f"epi-{tag}-pre", M, N, K, act=1, save_pre=True))
        cs.append(_case(f"epi-{tag}-pre-pe", M, N, K, act=1, save_pre=True, pe=pe, out_f32=True))
        cs.append(_case(f"epi-{tag}-bwd-res", M, N, K, bias=False, act=2, res=True))
        cs.append(_case(f"epi-{tag}-inplace", M, N, K, res=True, inplace=True))
        cs.append(_case(f"epi-{tag}-drop-pre", M, N, K, act=1, save_pre=True, p=0.1))
        cs.append(_case(f"epi-{tag}-drop-bwd", M, N, K, bias=False, act=2, res=True, p=0.1, out_f32=True))
    cs.append(_case("epi-colsum-small1", 77, 200, 136, bias=False, act=2, colsum=True))
    cs.append(_case("epi-colsum-small2", 500, 520, 136, bias=False, act=2, colsum=True))
    for part in (True, False):  # per-row-block partials + one reduction (as inside a network call), or atomics
        cs.append(_case(f"epi-colsum-main64-{'part' if part else 'atom'}", 1000, 392, 136, bias=False, act=2, colsum=True, part_ws=part))
        cs.append(_case(f"epi-colsum-main128-{'part' if part else 'atom'}", 3064, 2040, 64, bias=False, act=2, colsum=True, part_ws=part))
    # grouped launches as the attention pooler sets them (api.hip: X [M, groups K] with zX = K, W [groups][N][K], zOut = N):
    # forward (bias, dropout) and backward (act 2, aux, colsum over groups * zOut columns, dropout)
    for tag, M in (("s", 77), ("m", 1000)):
        for g, N, K in ((2, 104, 72), (8, 48, 48)):
            cs.append(_case(f"grp-{tag}-g{g}-fwd", M, N, K, groups=g, p=0.1))
            cs.append(_case(f"grp-{tag}-g{g}-bwd", M, N, K, groups=g, bias=False, act=2, colsum=True, part_ws=(tag == "m"), p=0.1))
    # 5. XCD-aware tile order off / on
    for M, N, K, g in [(3100, 2048, 64, 1), (520, 1280, 64, 8), (1000, 384, 136, 1)]:
        for x in (0, 1):
            cs.append(_case(f"xcd{x}-{M}x{N}-g{g}", M, N, K, groups=g, out_f32=True, xcd=x))
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


NT_CASES = _nt_cases()
NT_BY_NAME = {c["name"]: c for c in NT_CASES}


# ---- layout ---------------------------------------------------------------------------------------------------------------------
def nt_layout(c):
    """Strides and group offsets in elements.  X [M, groups K], W [groups N, K], everything on the output side [M, groups N]."""
    g, N, K = c["groups"], c["N"], c["K"]
    Wd = g * N
    s = c["strided"]
    L = dict(Wd=Wd, ldx=g * K + (8 if s else 0), ldw=K + (16 if s else 0), ldc=Wd + PAD_OUT, ldpre=Wd + PAD_OUT,
             ldaux=Wd + (8 if s else 0), ldres=Wd + (24 if s else 0), zX=K, zOut=N, drop_ld=Wd)
    L["zW"] = N * L["ldw"]
    if c["inplace"]:
        L["ldres"] = L["ldc"]
    return L


def _bf(x):
    return from_bf16_bits(to_bf16_bits(x)).astype(np.float64)


def nt_inputs(c):
    """Operand scale as in test_gemm_nt: X ~ N(0, 1), W ~ N(0, 1/K).  Values are the bf16-rounded ones (fp64 arrays)."""
    rs = np.random.RandomState(c["seed"])
    M, N, K, g = c["M"], c["N"], c["K"], c["groups"]
    Wd = g * N
    inp = dict(X=_bf(rs.randn(M, g * K)), W=_bf(rs.randn(Wd, K) / math.sqrt(K)))
    inp["bias"] = rs.randn(Wd).astype(np.float32).astype(np.float64) if c["bias"] else None
    inp["res"] = _bf(rs.randn(M, Wd)) if c["res"] else None
    inp["aux"] = _bf(rs.randn(M, Wd)) if c["aux"] else None
    inp["pe"] = rs.randn(max(c["pe"][0], c["pe"][2]), N).astype(np.float32).astype(np.float64) if c["pe"] else None
    inp["colsum0"] = rs.randn(Wd).astype(np.float32) if c["colsum"] else None
    return inp


# ---- reference ------------------------------------------------------------------------------------------------------------------
def drop_scales(lib, c, rows, idx_shift=0):
    """[len(rows), groups N] keep-scales of the library's host generator at element index row * drop_ld + z * zOut + col."""
    L = nt_layout(c)
    lib.coot_debug_dropout_scales.argtypes = [C.c_uint64, C.c_uint, C.c_uint64, C.c_int64, C.c_float, C.c_void_p]
    out = np.empty((len(rows), L["Wd"]), np.float32)
    for i, r in enumerate(rows):  # z * zOut + col runs over [0, groups N): one call per row
        rc = lib.coot_debug_dropout_scales(c["seed"], DROP_SITE, int(r) * L["drop_ld"] + idx_shift, L["Wd"], c["p"], out[i].ctypes.data)
        assert rc == 0
    return out.astype(np.float64)


def nt_acc(c, inp):
    """(acc, A): X . W^T per group in fp64, and the same with magnitudes."""
    g, N, K = c["groups"], c["N"], c["K"]
    acc = np.empty((c["M"], g * N))
    A = np.empty_like(acc)
    aX, aW = np.abs(inp["X"]), np.abs(inp["W"])
    for z in range(g):
        acc[:, z * N:(z + 1) * N] = inp["X"][:, z * K:(z + 1) * K] @ inp["W"][z * N:(z + 1) * N].T
        A[:, z * N:(z + 1) * N] = aX[:, z * K:(z + 1) * K] @ aW[z * N:(z + 1) * N].T
    return acc, A


def nt_epilogue(c, inp, acc, A, rows=None, lib=None, bias_shift=0, pe_shift=0, drop_shift=0):
    """Steps 1 .. 8 on the given rows (default: all).  Returns dict(out, tol, pre, tol_pre, gterm, Aout): fp64 [len(rows), groups N];
    tol / tol_pre are for an fp32 output (the bf16 half ulp is added by the checker).  The *_shift arguments build the wrong results
    the checker must reject: the bias of the neighbouring group, pe positions of the second segment off by one, the dropout scales
    of idx0 + 2."""
    M, N, K, g = c["M"], c["N"], c["K"], c["groups"]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    v, Av = acc[rows].copy(), A[rows].copy()
    if c["bias"]:
        b = np.roll(inp["bias"], bias_shift * N)
        v += b
        Av += np.abs(b)
    dsc = drop_scales(lib, c, rows, drop_shift) if c["p"] > 0 else None
    if dsc is not None and c["act"] != 2:
        v *= dsc
        Av *= dsc
    r = dict(pre=None, tol_pre=None)
    if c["save_pre"]:
        r["pre"], r["tol_pre"] = v.copy(), K * EPS32 * Av
    gterm = np.zeros_like(v)
    if c["act"] == 1:
        gterm = GELU_ERR * np.abs(v)
        v, Av = gelu(v), gelu(Av)
    if c["pe"]:
        pl, t0, pl2 = c["pe"]
        pos = np.where(rows < t0, rows % pl, (rows - t0 + pe_shift) % pl2)
        pe = np.tile(inp["pe"][pos], (1, g))  # the table has N columns: every group adds the same rows
        v += pe
        Av += np.abs(pe)
    if c["res"]:
        v += inp["res"][rows]
        Av += np.abs(inp["res"][rows])
    if c["act"] == 2:
        d = dsc if dsc is not None else 1.0
        gterm = GELU_ERR * np.abs(v) * d
        v = v * gelu_grad(inp["aux"][rows]) * d
        Av = Av * GELU_GRAD_MAX * d
    r.update(out=v, tol=K * EPS32 * Av + gterm, gterm=gterm, Aout=Av)
    return r


def nt_reference(c, inp, lib=None):
    acc, A = nt_acc(c, inp)
    ref = nt_epilogue(c, inp, acc, A, lib=lib)
    ref["acc"], ref["A"] = acc, A
    if c["colsum"]:
        ref["colsum"] = ref["out"].sum(0)
        ref["tol_colsum"] = (c["M"] + c["K"]) * EPS32 * (np.abs(inp["colsum0"]) + ref["Aout"].sum(0)) + ref["gterm"].sum(0)
    return ref


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def _pad16(x, ld, fill=NAN16):
    """bf16 bits of x [R, w] in a [R, ld] uint16 array whose padding columns hold `fill`."""
    out = np.full((x.shape[0], ld), fill, np.uint16)
    out[:, :x.shape[1]] = to_bf16_bits(x)
    return out


def nt_device_inputs(c, inp):
    """Host images (numpy) of the input-side buffers, paddings NaN."""
    L = nt_layout(c)
    g, N, K = c["groups"], c["N"], c["K"]
    b = dict(X=_pad16(inp["X"], L["ldx"]), W=_pad16(inp["W"], L["ldw"]))
    if c["bias"]:
        b["bias"] = inp["bias"].astype(np.float32)
    if c["res"] and not c["inplace"]:
        b["res"] = _pad16(inp["res"], L["ldres"])
    if c["aux"]:
        b["aux"] = _pad16(inp["aux"], L["ldaux"])
    if c["pe"]:
        b["pe"] = inp["pe"].astype(np.float32)
    return b


def nt_output_buffers(c, inp):
    """Host images of the output-side buffers before the call: sentinels everywhere, the residual inside the window of an in-place
    call, the random starting values inside the colsum window."""
    L = nt_layout(c)
    R = c["M"] + ROWS_BELOW
    b = {}
    if c["out_f32"]:
        b["out"] = np.full((R, L["ldc"]), SENT32, np.uint32)
    else:
        b["out"] = np.full((R, L["ldc"]), SENT16, np.uint16)
        if c["inplace"]:
            b["out"][:c["M"], :L["Wd"]] = to_bf16_bits(inp["res"])
    if c["save_pre"]:
        b["pre"] = np.full((R, L["ldpre"]), SENT16, np.uint16)
    if c["colsum"]:
        b["colsum"] = np.full(L["Wd"] + PAD_OUT, SENT32, np.uint32)
        b["colsum"][:L["Wd"]] = inp["colsum0"].view(np.uint32)
    return b


def nt_fake_outputs(c, inp, ref):
    """What a kernel that computes the reference exactly would leave in the output buffers."""
    L = nt_layout(c)
    M, Wd = c["M"], L["Wd"]
    b = nt_output_buffers(c, inp)
    if c["out_f32"]:
        b["out"][:M, :Wd] = ref["out"].astype(np.float32).view(np.uint32)
    else:
        b["out"][:M, :Wd] = to_bf16_bits(ref["out"])
    if c["save_pre"]:
        b["pre"][:M, :Wd] = to_bf16_bits(ref["pre"])
    if c["colsum"]:
        b["colsum"][:Wd] = (inp["colsum0"].astype(np.float64) + ref["colsum"]).astype(np.float32).view(np.uint32)
    return b


# ---- checker --------------------------------------------------------------------------------------------------------------------
def _check_window(name, what, raw, M, Wd, ref, tol, is_f32):
    """Sentinels outside [M, Wd], every element inside within tol (+ half a bf16 ulp for a bf16 buffer).  Returns the worst ratio."""
    sent = SENT32 if is_f32 else SENT16
    right, below = raw[:M, Wd:], raw[M:]
    assert (right == sent).all(), f"{name}: {what} written past column {Wd}: {int((right != sent).sum())} elements"
    assert (below == sent).all(), f"{name}: {what} written below row {M}: {int((below != sent).sum())} elements"
    win = raw[:M, :Wd]
    got = (win.view(np.float32) if is_f32 else from_bf16_bits(win)).astype(np.float64)
    full = tol if is_f32 else tol + np.abs(ref) * 2.0 ** -8
    err = np.abs(got - ref)
    ok = err <= full  # (a NaN fails)
    if not ok.all():
        i, j = np.argwhere(~ok)[0]
        raise AssertionError(f"{name}: {what}[{i},{j}] = {got[i, j]!r}, reference {ref[i, j]!r}, |error| {err[i, j]:.3e} > bound {full[i, j]:.3e} "
                             f"({int((~ok).sum())} elements out of bound)")
    return float((err / np.maximum(full, 1e-300)).max())


def nt_check(c, inp, ref, got):
    """got: the output-side buffers after the call (layout of nt_output_buffers).  Raises AssertionError; returns the worst
    error / bound ratio per buffer.  For an fp32 output the ratio is that of the accumulation + GELU terms alone, and "acc" is the
    worst (error - GELU term) / accumulation term: what the summation order of the matrix pipe and the epilogue's roundings take of
    their own term (the erfc polynomial alone reaches 0.87 of the GELU term, a fixed property of its coefficients)."""
    L = nt_layout(c)
    M, Wd = c["M"], L["Wd"]
    ratios = dict(out=_check_window(c["name"], "out", got["out"], M, Wd, ref["out"], ref["tol"], c["out_f32"]))
    if c["out_f32"]:  # the share of the error the GELU term cannot explain, against the accumulation term alone
        err = np.abs(got["out"][:M, :Wd].view(np.float32).astype(np.float64) - ref["out"])
        ratios["acc"] = float((np.maximum(err - ref["gterm"], 0.0) / np.maximum(ref["tol"] - ref["gterm"], 1e-300)).max())
    if c["save_pre"]:
        ratios["pre"] = _check_window(c["name"], "save_pre", got["pre"], M, Wd, ref["pre"], ref["tol_pre"], False)
    if c["colsum"]:
        raw = got["colsum"]
        assert (raw[Wd:] == SENT32).all(), f"{c['name']}: colsum written past column {Wd}"
        d = raw[:Wd].view(np.float32).astype(np.float64) - inp["colsum0"].astype(np.float64)
        err = np.abs(d - ref["colsum"])
        ok = err <= ref["tol_colsum"]
        assert ok.all(), (f"{c['name']}: colsum[{int(np.argmin(ok))}] off by {err[np.argmin(ok)]:.3e} > bound {ref['tol_colsum'][np.argmin(ok)]:.3e} "
                          f"({int((~ok).sum())} columns out of bound)")
        ratios["colsum"] = float((err / ref["tol_colsum"]).max())
    return ratios


# ---- wrong results the checker must reject (tests/test_cpu_gemm_cases.py) ---------------------------------------------------------
def _patch(c, inp, ref, rows, new):
    """Output buffers of the reference with the given rows replaced by another epilogue result (colsum follows)."""
    M, Wd = c["M"], nt_layout(c)["Wd"]
    out, pre = ref["out"].copy(), None if ref["pre"] is None else ref["pre"].copy()
    out[rows] = new["out"]
    if pre is not None:
        pre[rows] = new["pre"]
    r2 = dict(ref, out=out, pre=pre)
    if c["colsum"]:
        r2["colsum"] = ref["colsum"] + (new["out"] - ref["out"][rows]).sum(0)
    return nt_fake_outputs(c, inp, r2)


def nt_corruptions(c, inp, ref, lib=None):
    """name -> output buffers of a subtly wrong kernel.  Every one that applies to the case is returned."""
    M, N, K, g = c["M"], c["N"], c["K"], c["groups"]
    Wd = g * N
    rb = nt_row_block(c)
    rs = np.random.RandomState(c["seed"] ^ 0x5A5A)
    out = {}
    # one 8-element K chunk dropped from one 16 x 16 output tile (the last tile: it holds the row and column tails)
    r0, c0, k0 = (M - 1) // 16 * 16, (Wd - 1) // 16 * 16, int(rs.randint(0, K // 8)) * 8
    rows, cols = np.arange(r0, M), np.arange(c0, Wd)
    z = c0 // N
    acc2 = ref["acc"].copy()
    acc2[np.ix_(rows, cols)] -= inp["X"][rows][:, z * K + k0:z * K + k0 + 8] @ inp["W"][cols][:, k0:k0 + 8].T
    out["k_chunk_dropped"] = _patch(c, inp, ref, rows, nt_epilogue(c, inp, acc2, ref["A"], rows=rows, lib=lib))
    # one output row taken from the row 16 below (above, for the last rows)
    if M > 16:
        r = int(rs.randint(0, M))
        src = r + 16 if r + 16 < M else r - 16
        new = dict(out=ref["out"][[src]], pre=None if ref["pre"] is None else ref["pre"][[src]])
        out["row_from_16_below"] = _patch(c, inp, ref, np.array([r]), new)
    rows = np.arange(min(16, M))
    if g > 1 and c["bias"]:
        out["bias_of_next_group"] = _patch(c, inp, ref, rows, nt_epilogue(c, inp, ref["acc"], ref["A"], rows=rows, lib=lib, bias_shift=1))
    if c["pe"]:
        rows2 = np.arange(c["pe"][1], min(c["pe"][1] + 16, M))
        out["pe_off_by_one"] = _patch(c, inp, ref, rows2, nt_epilogue(c, inp, ref["acc"], ref["A"], rows=rows2, lib=lib, pe_shift=1))
    if c["p"] > 0:
        out["dropout_of_idx_plus_2"] = _patch(c, inp, ref, rows, nt_epilogue(c, inp, ref["acc"], ref["A"], rows=rows, lib=lib, drop_shift=2))
    if c["colsum"]:
        blk = int(rs.randint(0, _ceil(M, rb)))
        r2 = dict(ref, colsum=ref["colsum"] - ref["out"][blk * rb:(blk + 1) * rb].sum(0))
        out["colsum_without_a_row_block"] = nt_fake_outputs(c, inp, r2)
    # one sentinel byte changed past column N / in the row below M, in every output-side buffer in turn
    names = [k for k in ("out", "pre") if k in nt_output_buffers(c, inp)]
    for k in names:
        b = nt_fake_outputs(c, inp, ref)
        b[k].view(np.uint8).reshape(b[k].shape[0], -1)[int(rs.randint(0, M)), Wd * b[k].itemsize] ^= 0x01
        out[f"byte_past_column_N_{k}"] = b
        b = nt_fake_outputs(c, inp, ref)
        b[k].view(np.uint8).reshape(b[k].shape[0], -1)[M, int(rs.randint(0, Wd * b[k].itemsize))] ^= 0x80
        out[f"byte_below_row_M_{k}"] = b
    if c["colsum"]:
        b = nt_fake_outputs(c, inp, ref)
        b["colsum"].view(np.uint8)[Wd * 4] ^= 0x01
        out["byte_past_column_N_colsum"] = b
    return out


# ---- gemm_tn --------------------------------------------------------------------------------------------------------------------
TN_T = (1, 63, 64, 65, 255, 256, 257, 1000)  # around 64 (one k-step) and 256 (where a second split of the t range appears)
TN_SHAPES = ((8, 8), (120, 136), (384, 384))
TN_CASES = [dict(name=f"tn-T{T}-{Mo}x{No}", T=T, Mo=Mo, No=No, groups=1, colsum=False, overwrite=0, zC_pad=0, seed=zlib.crc32(f"tn{T}{Mo}{No}".encode()) & 0x7FFFFFFF)
            for T in TN_T for (Mo, No) in TN_SHAPES]
# coot_gemm_tn_batch: Mo % 384 == 0 takes the wide tiles (register-staged or LDS-DMA), the rest the 128 x 128 ones
TN_BATCH = [dict(name="tnb-ldc", T=257, Mo=384, No=136, groups=1, colsum=False, overwrite=0, zC_pad=0, seed=11),
            dict(name="tnb-groups-zC", T=300, Mo=120, No=136, groups=2, colsum=False, overwrite=0, zC_pad=40, seed=12),
            dict(name="tnb-groups-zC-wide", T=90, Mo=384, No=128, groups=2, colsum=False, overwrite=0, zC_pad=40, seed=13),
            dict(name="tnb-empty-overwrite", T=0, Mo=120, No=136, groups=1, colsum=False, overwrite=1, zC_pad=0, seed=14),
            dict(name="tnb-colsum-lda", T=1000, Mo=384, No=384, groups=1, colsum=True, overwrite=0, zC_pad=0, seed=15),
            dict(name="tnb-colsum-lda-narrow", T=333, Mo=200, No=72, groups=1, colsum=True, overwrite=1, zC_pad=0, seed=16)]


def tn_layout(c):
    g, Mo, No = c["groups"], c["Mo"], c["No"]
    L = dict(lda=g * Mo + 8, ldb=g * No + 16, ldc=No + PAD_OUT, zA=Mo, zB=No)
    L["zC"] = (Mo + ROWS_BELOW) * L["ldc"] + c["zC_pad"]  # every group: its window, 16 sentinel rows, zC_pad more sentinels
    return L


def tn_inputs(c):
    rs = np.random.RandomState(c["seed"])
    g, T, Mo, No = c["groups"], c["T"], c["Mo"], c["No"]
    inp = dict(A=_bf(rs.randn(T, g * Mo)), B=_bf(rs.randn(T, g * No)), C0=rs.randn(g, Mo, No).astype(np.float32))
    inp["cs0"] = rs.randn(Mo).astype(np.float32) if c["colsum"] else None
    return inp


def tn_reference(c, inp):
    g, T, Mo, No = c["groups"], c["T"], c["Mo"], c["No"]
    aA, aB = np.abs(inp["A"]), np.abs(inp["B"])
    prod = np.stack([inp["A"][:, z * Mo:(z + 1) * Mo].T @ inp["B"][:, z * No:(z + 1) * No] for z in range(g)])
    mag = np.stack([aA[:, z * Mo:(z + 1) * Mo].T @ aB[:, z * No:(z + 1) * No] for z in range(g)])
    c0 = np.zeros_like(prod) if c["overwrite"] else inp["C0"].astype(np.float64)
    ref = dict(C=c0 + prod, tol=T * EPS32 * (np.abs(c0) + mag))
    if c["colsum"]:
        ref["cs"] = inp["cs0"].astype(np.float64) + inp["A"][:, :Mo].sum(0)
        ref["tol_cs"] = T * EPS32 * (np.abs(inp["cs0"]) + aA[:, :Mo].sum(0))
    return ref


def tn_device_inputs(c, inp):
    L = tn_layout(c)
    return dict(A=_pad16(inp["A"], L["lda"]), B=_pad16(inp["B"], L["ldb"]))


def tn_output_buffers(c, inp):
    L = tn_layout(c)
    g, Mo, No = c["groups"], c["Mo"], c["No"]
    buf = np.full(g * L["zC"], SENT32, np.uint32)
    for z in range(g):
        buf[z * L["zC"]:z * L["zC"] + (Mo + ROWS_BELOW) * L["ldc"]].reshape(Mo + ROWS_BELOW, L["ldc"])[:Mo, :No] = inp["C0"][z].view(np.uint32)
    b = dict(C=buf)
    if c["colsum"]:
        b["cs"] = np.full(Mo + PAD_OUT, SENT32, np.uint32)
        b["cs"][:Mo] = inp["cs0"].view(np.uint32)
    return b


def tn_fake_outputs(c, inp, ref):
    L = tn_layout(c)
    Mo, No = c["Mo"], c["No"]
    b = tn_output_buffers(c, inp)
    for z in range(c["groups"]):
        b["C"][z * L["zC"]:z * L["zC"] + (Mo + ROWS_BELOW) * L["ldc"]].reshape(Mo + ROWS_BELOW, L["ldc"])[:Mo, :No] = ref["C"][z].astype(np.float32).view(np.uint32)
    if c["colsum"]:
        b["cs"][:Mo] = ref["cs"].astype(np.float32).view(np.uint32)
    return b


def tn_check(c, inp, ref, got):
    L = tn_layout(c)
    Mo, No = c["Mo"], c["No"]
    worst = 0.0
    for z in range(c["groups"]):
        blk = got["C"][z * L["zC"]:(z + 1) * L["zC"]]
        n = (Mo + ROWS_BELOW) * L["ldc"]
        assert (blk[n:] == SENT32).all(), f"{c['name']}: C written between the groups (group {z})"
        worst = max(worst, _check_window(c["name"], f"C[{z}]", blk[:n].reshape(Mo + ROWS_BELOW, L["ldc"]), Mo, No, ref["C"][z],
                                         np.maximum(ref["tol"][z], 0.0), True))
    r = dict(C=worst)
    if c["colsum"]:
        assert (got["cs"][Mo:] == SENT32).all(), f"{c['name']}: a_colsum written past column {Mo}"
        err = np.abs(got["cs"][:Mo].view(np.float32).astype(np.float64) - ref["cs"])
        assert (err <= ref["tol_cs"]).all(), f"{c['name']}: a_colsum off by {err.max():.3e}"
        r["cs"] = float((err / ref["tol_cs"]).max())
    return r
