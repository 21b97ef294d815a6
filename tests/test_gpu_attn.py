"""The attention kernels alone, forward and backward, on every dispatch path (one-query, short, chunked; two segments, packed
rows, dropout, strides, both workgroup orders) through coot_debug_attn, against the exact fp64 reference and the derived
per-element bound of tests/attn_cases.py (whose docstring states the bound), with sentinels around every output window.

Measured on an MI355X (worst |error| / bound over the cases of a row, forward and backward; a test passes at <= 1; recorded, not
asserted; cos(dq): cosine of dq against the exact reference on the shared-component cases):

  cases (kernels)                                      o              lse            dq             dk             dv             cos(dq)
  short-L*  (8 lengths 2 .. 128)                       0.498 - 0.772  0.013 - 0.068  0.428 - 0.610  0.458 - 0.555  0.517 - 0.833
  short-n9h3, -xcd0  (9 seq., 3 heads, both orders)    0.714 - 0.785  0.070 - 0.079  0.633 - 0.695  0.603 - 0.679  0.667 - 0.703
  short-drop                                           0.689          0.050          0.525          0.513          0.551
  short-shared                                         0.495          0.015          0.310          0.378          0.428          0.999783
  short-chained                                        0.658          0.031          0.187          0.251          0.700
  short-wide                                           0.679          0.040          0.610          0.460          0.774
  seg2-*  (short, two segments, one with dropout)      0.733 - 0.892  0.025 - 0.070  0.521 - 0.767  0.507 - 0.586  0.613 - 0.776
  packed-*  (short, packed rows, one with dropout)     0.664 - 0.818  0.026 - 0.039  0.547 - 0.617  0.554 - 0.595  0.804 - 0.874
  chunked-L*  (129, 150, 192, 193)                     0.437 - 0.544  0.022 - 0.050  0.508 - 0.610  0.439 - 0.580  0.447 - 0.583
  chunked-drop                                         0.527          0.022          0.555          0.480          0.597
  chunked-shared                                       0.383          0.030          0.339          0.335          0.321          0.999837
  chunked-chained                                      0.484          0.049          0.235          0.213          0.481
  cross-Lk65, -Lk130, -Lk130-drop  (chunked, Lq = 1)   0.327 - 0.640  0.019 - 0.038  0.256 - 0.422  0.896 - 0.920  0.983 - 0.999
  cross-Lk1 .. 64, self-L1  (one-query kernels)        0.000 - 0.399  0.003 - 0.021  0.000 - 0.396  0.000 - 0.546  0.000 - 0.651
  cross-drop  (one-query)                              0.545          0.009          0.281          0.479          0.639
  cross-shared  (one-query)                            0.242          0.057          0.037          0.607          0.643          0.999999
  cross-chained  (one-query)                           0.402          0.021          0.116          0.345          0.641

Worst per family: short 0.892 (o), chunked 0.999 (dv), one-query 0.651 (dv).  o, dq, dk and dv agree with the kernel-following
reference of attn_cases.py to the printed digits on every case: the kernels round where the bound says and nowhere else.  With
one query row, dk and dv of the chunked kernels are ONE product rounded twice (P and dS to bf16, then the store), so two half
ulps can add up to the whole bound: 0.999 is that, not a near miss.  The one-query kernels round once and stay below 0.66.
Shared-component keys: the one-query kernels' dq (delta from the products they differentiate) has 1 - cos = 1e-6, the short and
chunked kernels' (delta = <dO, bf16(O)>) 2e-4: inside the bound, which carries that residue, and two orders of magnitude worse.
The all-ones rows (cross-Lk1, self-L1: one key, P = 1) are exact.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import attn_cases as A

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


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Inputs and the exact reference with its bound, computed once per case and shared by both directions (read-only)."""
    import coot_videotext_amd as cva
    c = A.BY_NAME[name]
    inp = A.attn_inputs(c)
    return inp, A.attn_reference(c, inp, A.drop_masks(c, cva.lib.load()))


def _up(torch, a):
    return torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.int32)).cuda()


def _run(env, c, dev, backward):
    torch, cva, lib = env
    L = A.layout(c)
    sq = A.sequences(c)

    def op(x):
        off, ld = A.operand_offset(c, x)
        return dev[L["ops"][x][0]].data_ptr() + 2 * off, ld

    a = cva.lib.AttnArgs(Nseq=c["Nseq"], Lq=c["Lq"], Lk=c["Lk"], H=c["H"], dh=c["dh"], Nseq2=c["Nseq2"], L2=c["L2"],
                         p=c["p"], seed=c["seed"], site=A.SITE)
    for x, (fp, fl) in dict(q=("q", "ldq"), k=("k", "ldk"), v=("v", "ldv"), o=("o", "ldo"), dout=("dout", "lddo"), dq=("dq", "lddq"),
                            dk=("dk", "lddk"), dv=("dv", "lddv")).items():
        p, ld = op(x)
        setattr(a, fp, p)
        setattr(a, fl, ld)
    a.lse = dev["lse"].data_ptr() + 4 * A.GUARD * c["H"]
    keep = [torch.tensor(c["lens"], dtype=torch.int64, device="cuda"), torch.empty(L["Tq"] * c["H"] + 64, dtype=torch.float32, device="cuda")]
    a.lens, a.delta = keep[0].data_ptr(), keep[1].data_ptr()
    if c["Nseq2"]:
        keep.append(torch.tensor(c["lens2"], dtype=torch.int64, device="cuda"))
        a.lens2 = keep[-1].data_ptr()
    if c["packed"]:
        keep.append(torch.tensor([s["kr0"] for s in sq], dtype=torch.int32, device="cuda"))
        a.cu = keep[-1].data_ptr()
    xcd0 = cva.lib.get_option("xcd_order")
    try:
        if c["xcd"] is not None:
            cva.lib.check(lib.coot_set_option(b"xcd_order", (xcd0 & ~4) | (4 if c["xcd"] else 0)))
        cva.lib.check(lib.coot_debug_attn(C.byref(a), int(backward), torch.cuda.current_stream().cuda_stream), "debug_attn")
        torch.cuda.synchronize()
    finally:
        lib.coot_set_option(b"xcd_order", xcd0)


def _down(dev, host):
    return {k: dev[k].cpu().numpy().view(host[k].dtype).reshape(host[k].shape) for k in host}


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("name", [c["name"] for c in A.CASES])
def test_attn(env, name, direction):
    """|error| / bound <= 1 for every element of o and lse (fwd) or dq, dk and dv (bwd); no sentinel moved, no NaN, exact zeros in dK
    and dV of filled keys.  The backward reads o and lse of the fp64 reference, rounded to bf16 / fp32, so that a forward error can
    neither hide nor fake a backward one; a chained case reads what the forward kernel wrote."""
    torch = env[0]
    c = A.BY_NAME[name]
    inp, ref = _reference(name)
    fed = dict(o=ref["o"], lse=ref["lse"]) if direction == "bwd" and not c["chained"] else None
    host = A.buffers(c, inp, fed)
    dev = {k: _up(torch, v) for k, v in host.items()}
    if direction == "bwd" and c["chained"]:
        _run(env, c, dev, False)
        host = _down(dev, host)
    _run(env, c, dev, direction == "bwd")
    got = _down(dev, host)
    ratios = A.attn_check(c, ref, got, direction, before=host)
    extra = f" cos_dq={A.dq_cosine(c, ref, got):.6f}" if direction == "bwd" and c["shared"] else ""
    print(f"attn {name} {c['family']} {direction} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()) + extra)
    assert max(ratios.values()) <= 1.0
