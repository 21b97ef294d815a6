"""gemm_nt and gemm_tn at every launch variant, stride and epilogue against the fp64 reference and the derived per-element bound of
tests/gemm_cases.py (whose docstring states the bound), with sentinel bytes around every output window.

Measured on an MI355X (worst |error| / bound over the cases of a family; a test passes at <= 1):

  family                                       out            acc            save_pre       colsum
  ctl-*  fp32, no GELU (3 controls)            0.005 - 0.017  0.005 - 0.017
  ctl-*  fp32, GELU (3 controls)               0.008 - 0.517  0.000 - 0.002
  ctl-*  bf16 (4 controls)                     0.799 - 0.985
  var-*  fp32 (12 shapes, 4 kernels)           0.003 - 0.032  0.003 - 0.032
  var-*  bf16                                  0.912 - 0.994
  k-*    fp32, K = 8                           0.168 - 0.234  0.168 - 0.234
  k-*    fp32, K = 40 .. 392                   0.004 - 0.049  0.004 - 0.049
  ld-*, epi-*  fp32 with GELU / GELU'          0.316 - 0.608  0.000 - 0.008
  ld-*, epi-*, grp-*  bf16                     0.951 - 0.993                 0.973 - 0.993  0.000 - 0.070
  xcd0-*, xcd1-*  fp32                         0.011 - 0.032  0.011 - 0.032
  gemm_tn (96 runs) / gemm_tn_batch            C 0.000 - 0.018, a_colsum 0.000

"out" of an fp32 output is |error| / (accumulation term + GELU term); "acc" is (|error| - GELU term) / accumulation term, what
the matrix pipe's summation and the epilogue's roundings take of the IEEE worst case K * 2^-24 * A.  It stays below 0.05 from
K = 40 on; at K = 8, 0.125 of the 0.17 - 0.23 is the fp32 store of the result.  One control, ctl-300x200x72-f32 (GELU, K = 72),
has out = 0.517, above one half: there the GELU term is three times the accumulation term, and the erfc polynomial of common.h
evaluated in fp64 on the same inputs gives 0.516 by itself (it reaches 0.87 of its documented 1.25e-5 |v|); the kernel adds
0.001.  So the controls bear out the assumption about the summation (acc <= 0.017, asserted <= 0.5 below), and the GELU term is
a tight bound, not a generous one.  bf16 stores sit just under 1 by construction: half an ulp is what a correct rounding costs.
"""
import ctypes as C

import numpy as np
import pytest

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    lib = cva.lib.load()
    if cva.lib.operand() != "bf16":
        pytest.skip("the cases round their operands to bf16")
    return torch, cva, lib


def _up(torch, a):
    """numpy image -> device tensor with the same bytes."""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def _down(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def _sp(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", [c["name"] for c in G.NT_CASES])
def test_gemm_nt(env, name):
    torch, cva, lib = env
    c = G.NT_BY_NAME[name]
    L = G.nt_layout(c)
    inp = G.nt_inputs(c)
    ref = G.nt_reference(c, inp, lib)
    host_in, host_out = G.nt_device_inputs(c, inp), G.nt_output_buffers(c, inp)
    din = {k: _up(torch, v) for k, v in host_in.items()}
    dout = {k: _up(torch, v) for k, v in host_out.items()}
    p = lambda d, k: d[k].data_ptr() if k in d else None
    a = cva.lib.GemmNtArgs(X=p(din, "X"), ldx=L["ldx"], W=p(din, "W"), ldw=L["ldw"], M=c["M"], N=c["N"], K=c["K"], groups=c["groups"],
                           zX=L["zX"], zW=L["zW"], zOut=L["zOut"], bias=p(din, "bias"), act=c["act"], aux=p(din, "aux"), ldaux=L["ldaux"],
                           save_pre=p(dout, "pre"), ldpre=L["ldpre"], res=p(dout, "out") if c["inplace"] else p(din, "res"), ldres=L["ldres"],
                           pe=p(din, "pe"), colsum=p(dout, "colsum"), p=c["p"], seed=c["seed"], site=G.DROP_SITE, drop_ld=L["drop_ld"],
                           out=p(dout, "out"), ldc=L["ldc"], out_f32=int(c["out_f32"]))
    if c["pe"]:
        a.pe_L, a.pe_T0, a.pe_L2 = c["pe"]
    if c["part_ws"]:
        ws = torch.empty(-(-c["M"] // 64) * L["Wd"], dtype=torch.float32, device="cuda")
        a.part_ws, a.part_ws_floats = ws.data_ptr(), ws.numel()
    xcd0 = cva.lib.get_option("xcd_order")
    try:
        if c["xcd"] is not None:
            cva.lib.check(lib.coot_set_option(b"xcd_order", (xcd0 & ~1) | c["xcd"]))
        cva.lib.check(lib.coot_debug_gemm_nt(C.byref(a), _sp(torch)), "debug_gemm_nt")
        torch.cuda.synchronize()
    finally:
        lib.coot_set_option(b"xcd_order", xcd0)
    got = {k: _down(dout[k], host_out[k]) for k in host_out}
    ratios = G.nt_check(c, inp, ref, got)
    print(f"gemm_nt {name} {c['variant']} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0
    if c["control"] and c["out_f32"]:  # the matrix pipe's summation is not documented to be IEEE: it must stay far inside the IEEE bound
        assert ratios["acc"] <= 0.5, ratios


@pytest.mark.parametrize("mode,use_ws", [(0, True), (0, False), (1, True), (1, False)])
@pytest.mark.parametrize("name", [c["name"] for c in G.TN_CASES])
def test_gemm_tn(env, name, mode, use_ws):
    """coot_gemm_tn with lda = Mo + 8, ldb = No + 16, ldc = No + 8: the split reduction through a workspace, or atomics / the
    single-split direct path without one, fragments by transposing LDS reads (tn_mode 0) or from a transposed LDS image (1)."""
    torch, cva, lib = env
    c = {c["name"]: c for c in G.TN_CASES}[name]
    L = G.tn_layout(c)
    inp = G.tn_inputs(c)
    ref = G.tn_reference(c, inp)
    host_in, host_out = G.tn_device_inputs(c, inp), G.tn_output_buffers(c, inp)
    dA, dB, dC = _up(torch, host_in["A"]), _up(torch, host_in["B"]), _up(torch, host_out["C"])
    mode0 = cva.lib.get_option("tn_mode")
    cva.lib.check(lib.coot_set_option(b"tn_mode", mode))
    try:
        ws = torch.empty(lib.coot_gemm_tn_workspace_bytes(c["T"], c["Mo"], c["No"]) if use_ws else 0, dtype=torch.uint8, device="cuda")
        cva.lib.check(lib.coot_gemm_tn(dA.data_ptr(), L["lda"], dB.data_ptr(), L["ldb"], c["T"], c["Mo"], c["No"], dC.data_ptr(), L["ldc"],
                                       ws.data_ptr() if use_ws else None, ws.numel(), _sp(torch)), "gemm_tn")
        torch.cuda.synchronize()
    finally:
        lib.coot_set_option(b"tn_mode", mode0)
    r = G.tn_check(c, inp, ref, dict(C=_down(dC, host_out["C"])))
    print(f"gemm_tn {name} mode={mode} ws={use_ws} C={r['C']:.3f}")


@pytest.mark.parametrize("dma", [0, 1])
def test_gemm_tn_batch(env, dma):
    """coot_gemm_tn_batch on strided operands: ldc > No, grouped problems with zC > Mo No (narrow and wide tiles), an empty sum
    that overwrites (C comes back all zeros, its padding untouched), a bias-gradient column sum with lda > Mo (wide: taken by the
    loader waves of the DMA kernel from the landed stages, or by the register-staged kernel; narrow: by the 128 x 128 kernel)."""
    torch, cva, lib = env
    from coot_videotext_amd.lib import TnProblem
    keep, probs, todo = [], [], []
    for c in G.TN_BATCH:
        L = G.tn_layout(c)
        inp = G.tn_inputs(c)
        host_in, host_out = G.tn_device_inputs(c, inp), G.tn_output_buffers(c, inp)
        if c["T"] == 0:  # (an empty tensor has no address to speak of: any valid pointer will do, it is never read)
            host_in = {k: np.full((1, v.shape[1]), G.NAN16, np.uint16) for k, v in host_in.items()}
        d = {k: _up(torch, v) for k, v in dict(host_in, **host_out).items()}
        keep.append(d)
        probs.append(TnProblem(d["A"].data_ptr(), L["lda"], d["B"].data_ptr(), L["ldb"], c["T"], c["Mo"], c["No"], d["C"].data_ptr(), L["ldc"],
                               d["cs"].data_ptr() if c["colsum"] else None, c["overwrite"], c["groups"], L["zA"], L["zB"], L["zC"]))
        todo.append((c, inp, host_out, d))
    arr = (TnProblem * len(probs))(*probs)
    ws = torch.empty(8 * sum(c["Mo"] * c["No"] * c["groups"] for c in G.TN_BATCH), device="cuda")
    dma0 = cva.lib.get_option("tn_dma")
    cva.lib.check(lib.coot_set_option(b"tn_dma", dma))
    try:
        cva.lib.check(lib.coot_gemm_tn_batch(arr, len(probs), ws.data_ptr(), ws.numel() * 4, None, _sp(torch)), "gemm_tn_batch")
        torch.cuda.synchronize()
    finally:
        lib.coot_set_option(b"tn_dma", dma0)
    for c, inp, host_out, d in todo:
        r = G.tn_check(c, inp, G.tn_reference(c, inp), {k: _down(d[k], host_out[k]) for k in host_out})
        print(f"gemm_tn_batch dma={dma} {c['name']} " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
        if c["T"] == 0:
            got = _down(d["C"], host_out["C"])[:(c["Mo"] + G.ROWS_BELOW) * L_ldc(c)].reshape(-1, L_ldc(c))[:c["Mo"], :c["No"]]
            assert (got == 0).all()


def L_ldc(c):
    return G.tn_layout(c)["ldc"]
