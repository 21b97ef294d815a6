"""The row-wise and pooling kernels alone (csrc/rowops.hip, csrc/pool.hip): LayerNorm forward (every source, the packed gather, pe,
dropout, both outputs, the row-walking kernel of the input stages) and backward (every dispatch path of its column sums), GenPool forward
and backward (every channel blocking, two segments, packed rows, the hand-over to the padded layout, the column sum by atomics, partials
and the deferred reduction), avg_special, the pack kernels and the bf16 column sum, through coot_debug_ln, coot_debug_pool,
coot_debug_avgpool(_bwd), coot_pack_fwd / coot_pack_bwd / coot_debug_pack_bwd_join and coot_debug_colsum_bf16, against the exact fp64
reference and the derived per-element bounds of tests/rowpool_cases.py (whose docstring states the bounds and holds the measured
|error| / bound ratios), with sentinels around every output window and NaNs wherever nothing may be read.  The 16-bit operand format
follows the build (coot_get_option("operand_f16"))."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rowpool_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    return torch, cva, cva.lib.load(), cva.lib.operand()


@functools.lru_cache(maxsize=None)
def _reference(name, fmt):
    """Inputs, masks, what a backward is fed and the exact reference with its bounds: computed once per case, read-only."""
    import coot_videotext_amd as cva
    lib = cva.lib.load()
    c = A.BY_NAME[name]
    inp, ms = A.inputs(c, fmt), A.masks(c, lib)
    fed = A.pool_fed(c, lib, fmt) if c["op"] == "pool_bwd" and not c["chained"] else None
    return inp, ms, fed, (A.reference(c, inp, ms, fmt=fmt, fed=fed) if c["op"] != "pool_bwd" or not c["chained"] else None)


def _up(torch, a):
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def _down(dev, host):
    return {k: dev[k].cpu().numpy().view(host[k].dtype).reshape(host[k].shape) for k in host}


def _run(env, c, dev):
    """One call of the case's kernel on the device images `dev` (current stream), synchronised."""
    torch, cva, lib, _ = env
    T, op, L = A.tensors(c), c["op"], cva.lib
    keep = {k: torch.from_numpy(v).cuda() for k, v in A.ints(c).items()}

    def P(nm):
        if nm not in T:
            return None
        off, _ = A.window(c, nm)
        return dev[nm].data_ptr() + off * dev[nm].element_size()

    def ld(nm):
        return T[nm]["ld"] if nm in T else 0

    def ws(floats):  # a partial-sum workspace of NaNs: a partial row that is read without having been written shows
        if floats <= 0:
            return None, 0
        keep["ws"] = torch.full((floats,), float("nan"), dtype=torch.float32, device="cuda")
        return keep["ws"].data_ptr(), floats

    st = torch.cuda.current_stream().cuda_stream
    if op == "ln_fwd":
        a = L.LnArgs(x=P("x"), x_f32=int(c["x_f32"]), ldx=ld("x"), x2=P("x2"), R0=c.get("R0", 0), R=c["R"], D=c["D"], gain=P("gain"), bias=P("bias"),
                     pe=P("pe"), pe_L=c["pe_L"], y=P("y"), ldy=ld("y"), y32=P("y32"), ldy32=ld("y32"), p=c["p"], seed=c["seed"], site=A.SITE,
                     max_wgs=c.get("max_wgs", 0), nt=c.get("nt", 0))
        if "lens" in c:
            a.cu, a.nseq, a.N0, a.L0, a.L1 = keep["cu"].data_ptr(), len(c["lens"]) + len(c["lens2"]), len(c["lens"]), c["L0"], c["L1"]
            a.pos_out, a.src_packed = P("pos_out"), int(bool(c.get("src_packed")))
        rc = lib.coot_debug_ln(C.byref(a), 0, st)
    elif op == "ln_bwd":
        a = L.LnArgs(x=P("x"), x_f32=int(c["x_f32"]), ldx=ld("x"), R=c["R"], D=c["D"], gain=P("gain"), p=c["p"], seed=c["seed"], site=A.SITE,
                     dy_add=P("dy_add"), lddy_add=ld("dy_add"), dx=P("dx"), lddx=ld("dx"), dx32=P("dx32"), lddx32=ld("dx32"), dxm=P("dxm"), lddxm=ld("dxm"),
                     pm=c["pm"], seed_m=c["seed"] + 1, site_m=A.SITE_M, dxm_drop_ld=c["drop_ld"], dgain=P("dgain"), dbias=P("dbias"), dxcolsum=P("dxcolsum"))
        if c["dy32"]:
            a.dy32, a.lddy32 = P("dy"), ld("dy")
        else:
            a.dy, a.lddy = P("dy"), ld("dy")
        a.part_ws, a.part_ws_floats = ws(c["ws"])
        rc = lib.coot_debug_ln(C.byref(a), 1, st)
    elif op in ("pool_fwd", "pool_bwd"):
        back, prs = op == "pool_bwd", A.pool_rows(c)
        segs = (L.PoolArgs * len(prs))()
        for i, pr in enumerate(prs):
            x, a = ("", "2")[i], segs[i]
            a.s, a.lds, a.z, a.ldz, a.lens, a.N, a.L, a.D = P("s" + x), ld("s" + x), P("z" + x), ld("z" + x), keep["lens" + x].data_ptr(), pr["N"], pr["L"], c["D"]
            if c["packed"]:
                a.cu = keep["cu" + x].data_ptr()
            a.pooled, a.ldp, a.pooled_copy, a.smax, a.ssum = P("pooled" + x), ld("pooled" + x), P("pooled_copy" + x), P("smax" + x), P("ssum" + x)
            a.p_w, a.seed_w, a.site_w = c["p_w"], A.pool_seed(c, i), A.SITE_W
            if back:
                a.dpooled, a.lddp, a.ds, a.ldds, a.dz, a.lddz, a.ds_colsum = P("dpooled" + x), ld("dpooled" + x), P("ds" + x), ld("ds" + x), P("dz" + x), ld("dz" + x), P("ds_colsum")
                a.p_s, a.seed_s, a.site_s, a.drop_s_ld, a.drop_s_row0 = c["p_s"], c["seed"] + 3, A.SITE_S, c["D"] + 6, A.pool_row0(c, i)
            elif c["counts"] and i == len(prs) - 1:
                a.pk_counts, a.pk_B, a.pk_Cmax = keep["counts"].data_ptr(), len(c["counts"]), c["Cmax"]
                a.pk_out, a.pk_mask, a.pk_lens = P("pk_out"), P("pk_mask"), P("pk_lens")
        total = sum(pr["N"] for pr in prs)
        w, n = ws((total * c["D"] + 63) // 64 * 64 + 64 if back and c["colsum"] in ("partials", "defer") else 0)
        rc = lib.coot_debug_pool(segs, len(prs), int(back), w, n, int(back and c["colsum"] == "defer"), st)
    elif op == "avg_fwd":
        rc = lib.coot_debug_avgpool(P("z"), ld("z"), keep["lens"].data_ptr(), len(c["lens"]), c["L"], c["D"], P("out"), ld("out"), st)
    elif op == "avg_bwd":
        rc = lib.coot_debug_avgpool_bwd(P("dpooled"), ld("dpooled"), keep["lens"].data_ptr(), len(c["lens"]), c["L"], c["D"], P("dz"), ld("dz"), st)
    elif op == "pack_fwd":
        rc = lib.coot_pack_fwd(P("emb"), keep["counts"].data_ptr(), len(c["counts"]), c["Cmax"], c["D"], P("out"), P("mask"), P("lens"), st)
    elif op == "pack_bwd":
        rc = lib.coot_pack_bwd(P("dout"), keep["counts"].data_ptr(), len(c["counts"]), c["Cmax"], c["D"], P("demb"), st)
    elif op == "pack_join":
        rc = lib.coot_debug_pack_bwd_join(P("dout"), P("dout2"), P("dctx"), keep["counts"].data_ptr(), len(c["counts"]), c["Cmax"], c["D"], P("demb"), P("demb_ctx"), st)
    else:
        w, n = ws(c["ws"])
        rc = lib.coot_debug_colsum_bf16(P("x"), ld("x"), c["R"], c["C"], P("out"), w, n, st)
    cva.lib.check(rc, op)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES])
def test_rowpool(env, name):
    """Every element of every output within its bound of the exact reference (equal where the bound is zero), no NaN, no sentinel moved,
    no input changed.  A backward reads the statistics of the fp64 reference rounded to fp32, so that a forward error can neither hide nor
    fake a backward one; a chained case reads what the forward kernel wrote."""
    torch, cva, lib, fmt = env
    c = A.BY_NAME[name]
    inp, ms, fed, ref = _reference(name, fmt)
    if c["op"] == "pool_bwd" and c["chained"]:
        f = A.forward_case(c)
        finp = _reference(f["name"], fmt)[0]
        fhost = A.buffers(f, finp, fmt=fmt)
        fdev = {k: _up(torch, v) for k, v in fhost.items()}
        _run(env, f, fdev)
        fgot, FT = _down(fdev, fhost), A.tensors(f)
        out = {k: A._decode(FT[k], fgot[k][A.GUARD:A.GUARD + FT[k]["rows"], :FT[k]["cols"]], fmt) for k in FT if k.rstrip("2") in ("smax", "ssum", "pooled")}
        fed = A.pool_fed(c, lib, fmt, fwd_out=out)
        ref = A.reference(c, inp, ms, fmt=fmt, fed=fed)
    host = A.buffers(c, inp, fmt=fmt, fed=fed)
    dev = {k: _up(torch, v) for k, v in host.items()}
    _run(env, c, dev)
    bad, ratios = A.check(c, ref, _down(dev, host), before=host, fmt=fmt)
    print(f"rowpool {name} {fmt} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert not bad, bad
    assert max(ratios.values()) <= 1.0
