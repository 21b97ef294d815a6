"""tests/rowpool_cases.py without a GPU: the closed-form fp64 references of LayerNorm and GenPool equal float64 autograd on every case (and the
LayerNorm ones oracle.coot_oracle.ln_coot / ln_coot_bwd, which also covers the std == 0 rows where autograd's dx is 0 / 0),
the kernel-following reference stays within the derived bound of the exact one (the bound is attainable), and the checker rejects the
results of subtly wrong kernels on every case where the mutation changes the outputs.  Also: the coot_debug_* entries of the row-wise
and pooling kernels declared, bound, listed, exported by both builds and refusing bad descriptors on the host.

Worst |error| / bound of the kernel-following reference per operation and output (asserted <= 1 below; the 16-bit outputs sit just
under 1 by construction: half an ulp is what a correct rounding costs; measured here, bf16):
  ln_fwd   y 1.000  y32 0.592  pos_out 0                      ln_bwd   dx 0.999  dx32 0.161  dxm 0.999  dgain 0.066  dbias 0.474  dxcolsum 0.175
  pool_fwd pooled 0.125  ssum 0.118  smax 0  pk_out 0.040     pool_bwd ds 0.999  dz 1.000  ds_colsum 0.294
  avg_fwd  out 0.089     avg_bwd dz 1.000     colsum out 0.500     pack_* 0 (equal)

Cases each mutation changes, per operation (of 32 ln_fwd, 14 ln_bwd, 32 pool_fwd, 32 pool_bwd, 8 avg_fwd, 8 avg_bwd, 8 pack_fwd, 8 pack_bwd,
10 pack_join, 16 colsum); asserted below:"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rowpool_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPLIES = dict(
    biased_var=dict(ln_fwd=28, ln_bwd=13),        # D instead of D - 1 (not where the only row is all zero)
    eps_in_sqrt=dict(ln_fwd=28, ln_bwd=14),       # sqrt(var + eps) instead of sqrt(var) + eps (a zero row of the backward divides by it)
    std0_term=dict(ln_bwd=14),                    # the second term of dx on a std == 0 row: 0 / 0
    mask_row=dict(ln_fwd=8, ln_bwd=13, pool_fwd=5, pool_bwd=18),  # the masks of row + 1 (cases with dropout)
    mask_ld=dict(ln_bwd=7, pool_bwd=18),          # the mask indexed with D where dxm_drop_ld / drop_s_ld is meant
    row0=dict(pool_bwd=4),                        # drop_s_row0 ignored (second segments under dropout2)
    seed2=dict(pool_fwd=2, pool_bwd=2),           # the second segment drawing from the first's seed
    lens_next=dict(pool_fwd=29, pool_bwd=29, avg_fwd=4, avg_bwd=4),  # lens[n + 1] read for sequence n (not where all lens are equal)
    len_plus=dict(pool_fwd=27, pool_bwd=27, avg_fwd=8, avg_bwd=8),   # len + 1 (not in packed rows: the row does not exist; not where every len = L)
    len_minus=dict(pool_fwd=29, pool_bwd=29, avg_fwd=4, avg_bwd=4),  # len - 1 (not where every len = 1)
    no_fill=dict(pool_fwd=1, pool_bwd=1),         # the masked-fill term dropped from the statistics (exp(-32752 - max) = 0 unless the scores sit there)
    last_rg=dict(pool_fwd=21, pool_bwd=21),       # the last row group left out of the softmax merge (sequences that reach it)
    chan_shift=dict(pool_fwd=32, pool_bwd=32),    # channels 8 .. 15 take the results of 16 .. 23
    pad_not_zeroed=dict(pool_bwd=27),             # padded rows of ds / dz left as they were (padded layouts with a len < L)
    partial_missing=dict(ln_bwd=14, pool_bwd=15, colsum=16),  # one workgroup's rows missing from a column sum (pool: under dropout2 only)
    colsum_overwrite=dict(ln_bwd=14, pool_bwd=26, pack_bwd=8, pack_join=10, colsum=16),  # = where += is meant
    avg_valid_only=dict(avg_fwd=4, avg_bwd=4),    # avg_special over the valid rows only (cases with a len < L)
    pk_skip_empty=dict(pool_fwd=3, pack_fwd=6))   # zero-count videos skipped in the hand-over (counts with a zero)
NAMES = [c["name"] for c in A.CASES]


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _lib():
    import coot_videotext_amd as m
    return m.lib.load()


CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p,
         "int64_t*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p, "const int*": ctypes.c_void_p, "int*": ctypes.c_void_p, "int64_t": ctypes.c_int64,
         "uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "coot_stream_t": ctypes.c_void_p}
ENTRIES = dict(coot_debug_ln=("const coot_ln_args* a, int backward, coot_stream_t stream", "LnArgs"),
               coot_debug_pool=("const coot_pool_args* segs, int nseg, int backward, float* part_ws, size_t part_ws_floats, int defer, coot_stream_t stream", "PoolArgs"),
               coot_debug_avgpool=("const void* z, int64_t ldz, const int64_t* lens, int N, int L, int D, float* out, int64_t ldo, coot_stream_t stream", None),
               coot_debug_avgpool_bwd=("const float* dpooled, int64_t lddp, const int64_t* lens, int N, int L, int D, void* dz, int64_t lddz, coot_stream_t stream", None),
               coot_debug_pack_bwd_join=("const float* dout1, const float* dout2, const float* dctx, const int64_t* counts, int B, int Cmax, int D, float* demb_items, "
                                         "float* demb_ctx, coot_stream_t stream", None),
               coot_debug_colsum_bf16=("const void* x, int64_t ldx, int R, int C, float* out, float* part_ws, size_t part_ws_floats, coot_stream_t stream", None))


def test_debug_entries_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    docs = {d: open(os.path.join(ROOT, d)).read() for d in ("INTEGRATION.md", "README.md")}
    for name, (params, struct) in ENTRIES.items():
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and " ".join(m.group(1).split()) == params, name
        want = []
        for prm in params.split(", "):
            t = prm.rsplit(" ", 1)[0]
            want.append(ctypes.POINTER(getattr(cva.lib, struct)) if t.startswith("const coot_") else CTYPE[t])
        assert list(getattr(lib, name).argtypes) == want, name
        assert name in cva.lib.EXPORTS and re.search(r"\b%s\b" % name, vs), name
        for d, text in docs.items():
            assert name in text, (name, d)
    for cname, pyname in (("coot_ln_args", "LnArgs"), ("coot_pool_args", "PoolArgs")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            t, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
            fields += [(n.strip(), CTYPE[t]) for n in names.split(",")]
        assert fields == list(getattr(cva.lib, pyname)._fields_), cname
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions and new structs only: the ABI version stays
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, so


def test_debug_entries_refuse_on_the_host(cva):
    """Bad descriptors are refused before anything is launched (no GPU needed)."""
    lib = cva.lib.load()

    def refused(rc, what):
        assert rc != 0 and lib.coot_last_error(), what

    refused(lib.coot_debug_ln(None, 0, None), "ln null")
    ok = dict(x=64, x_f32=1, ldx=16, R=4, D=16, gain=64, bias=64, y=64, ldy=16, dy=64, lddy=16, dx=64, lddx=16)
    fwd = (dict(x=None), dict(y=None), dict(D=4), dict(D=18), dict(D=4100, ldx=4100, ldy=4100), dict(ldx=12), dict(ldx=18), dict(ldy=12), dict(y32=64, ldy32=8),
           dict(bias=None), dict(pe=64, pe_L=0), dict(x2=64, R0=5), dict(x2=64, R0=-1), dict(p=1.0), dict(p=-0.5), dict(R=-1), dict(max_wgs=-1),
           dict(cu=64, nseq=0), dict(cu=64, nseq=3, N0=1, L0=4), dict(cu=64, nseq=3, N0=3, L0=0), dict(pos_out=64), dict(src_packed=1))
    bwd = (dict(x=None), dict(dy=None), dict(gain=None), dict(D=1028, ldx=1028, lddy=1028, lddx=1028), dict(D=4), dict(ldx=12), dict(lddy=12), dict(dy32=64, lddy32=12),
           dict(dy_add=64, lddy_add=8), dict(lddx=12), dict(dx32=64, lddx32=0), dict(dxm=64, lddxm=12), dict(dxm=64, lddxm=16, pm=0.1, dxm_drop_ld=8),
           dict(dxm=64, lddxm=16, pm=0.1, dxm_drop_ld=17), dict(pm=1.0), dict(part_ws=64, part_ws_floats=0))
    for back, bads in ((0, fwd), (1, bwd)):
        for bad in bads:
            refused(lib.coot_debug_ln(ctypes.byref(cva.lib.LnArgs(**dict(ok, **bad))), back, None), (back, bad))
    P = cva.lib.PoolArgs
    ok = dict(s=64, lds=64, z=64, ldz=64, lens=64, N=2, L=3, D=64, pooled=64, ldp=64, smax=64, ssum=64, dpooled=64, lddp=64, ds=64, ldds=64, dz=64, lddz=64)
    one = lambda **kw: (P * 1)(P(**dict(ok, **kw)))
    refused(lib.coot_debug_pool(None, 1, 0, None, 0, 0, None), "pool null")
    for nseg in (0, 3, -1):
        refused(lib.coot_debug_pool(one(), nseg, 0, None, 0, 0, None), nseg)
    refused(lib.coot_debug_pool(one(), 1, 0, None, 0, 1, None), "defer in the forward")
    refused(lib.coot_debug_pool(one(), 1, 1, None, 0, 1, None), "defer without a workspace")
    refused(lib.coot_debug_pool(one(), 1, 1, 64, 0, 0, None), "workspace of no floats")
    both = (dict(s=None), dict(z=None), dict(lens=None), dict(pooled=None), dict(D=56), dict(D=520, lds=520, ldz=520, ldp=520), dict(D=68, lds=72, ldz=72, ldp=72),
            dict(lds=56), dict(lds=68), dict(ldz=60), dict(ldp=32), dict(N=0), dict(L=0), dict(p_w=1.0), dict(ssum=None))
    for back, bads in ((0, both + (dict(pk_out=64), dict(pk_out=64, pk_counts=64, pk_B=0, pk_Cmax=2), dict(pk_out=64, pk_counts=64, pk_B=2, pk_Cmax=0))),
                       (1, both + (dict(dpooled=None), dict(ds=None), dict(dz=None), dict(smax=None, ssum=None), dict(lddp=8), dict(ldds=60), dict(lddz=56),
                                   dict(p_s=0.1, drop_s_ld=32), dict(p_s=0.1, drop_s_ld=65), dict(p_s=0.1, drop_s_ld=64, drop_s_row0=-1),
                                   dict(pk_out=64, pk_counts=64, pk_B=2, pk_Cmax=2)))):
        for bad in bads:
            refused(lib.coot_debug_pool(one(**bad), 1, back, None, 0, 0, None), (back, bad))
    two = (P * 2)(P(**ok), P(**dict(ok, D=128, lds=128, ldz=128, ldp=128)))
    refused(lib.coot_debug_pool(two, 2, 0, None, 0, 0, None), "segments of different D")
    two = (P * 2)(P(**dict(ok, ds_colsum=64)), P(**dict(ok, ds_colsum=128)))
    refused(lib.coot_debug_pool(two, 2, 1, None, 0, 0, None), "segments of different ds_colsum")
    a = dict(z=64, ldz=8, lens=64, N=2, L=3, D=8, out=64, ldo=8)
    for bad in (dict(z=None), dict(lens=None), dict(out=None), dict(D=7), dict(D=0), dict(ldz=6), dict(ldz=9), dict(ldo=4), dict(L=0), dict(N=-1)):
        v = dict(a, **bad)
        refused(lib.coot_debug_avgpool(v["z"], v["ldz"], v["lens"], v["N"], v["L"], v["D"], v["out"], v["ldo"], None), bad)
        refused(lib.coot_debug_avgpool_bwd(v["out"], v["ldo"], v["lens"], v["N"], v["L"], v["D"], v["z"], v["ldz"], None), bad)
    j = dict(d1=64, d2=None, dc=None, counts=64, B=2, Cmax=2, D=8, items=64, ctx=None)
    for bad in (dict(d1=None), dict(counts=None), dict(items=None), dict(dc=64), dict(B=-1), dict(Cmax=0), dict(D=0)):
        v = dict(j, **bad)
        refused(lib.coot_debug_pack_bwd_join(v["d1"], v["d2"], v["dc"], v["counts"], v["B"], v["Cmax"], v["D"], v["items"], v["ctx"], None), bad)
    s = dict(x=64, ldx=8, R=2, C=8, out=64, ws=None, n=0)
    for bad in (dict(x=None), dict(out=None), dict(C=7), dict(C=0), dict(ldx=6), dict(ldx=9), dict(R=-1), dict(ws=64)):
        v = dict(s, **bad)
        refused(lib.coot_debug_colsum_bf16(v["x"], v["ldx"], v["R"], v["C"], v["out"], v["ws"], v["n"], None), bad)


def test_the_table_covers_every_axis():
    by = {}
    for c in A.CASES:
        by.setdefault(c["op"], []).append(c)
    f = by["ln_fwd"]
    plain = [c for c in f if re.fullmatch(r"lnf-D\d+(-zero)?", c["name"])]
    assert {c["D"] for c in plain} == {8, 12, 252, 256, 260, 508, 512, 516, 1024, 1028, 2048, 2052, 4096} and {c["R"] for c in plain} == {1, 4, 5, 9}
    assert {A.ln_nv(c["D"], "fwd") for c in plain} == {2, 4, 8, 16} and {c["x_f32"] for c in plain} == {True, False} and {c["wide"] for c in plain} == {True, False}
    assert {c["outs"] for c in plain} == {("y",), ("y32",), ("y", "y32")} and {c["gain"] for c in plain} == {True, False} and {c["p"] for c in plain} == {0.0, 0.1}
    assert any(c["pe_L"] and c["R"] % c["pe_L"] == 0 and c["R"] > c["pe_L"] for c in plain) and any(c["pe_L"] and c["R"] % c["pe_L"] for c in plain)
    assert all(c["zero_row"] >= 0 or any(d["name"] == c["name"] + "-zero" for d in plain) for c in plain)
    assert any("R0" in c and c["R0"] % 4 for c in f) and any("lens" in c and not c.get("src_packed") and len(set(c["lens"] + c["lens2"])) > 3 for c in f)
    assert {c["x_f32"] for c in f if c.get("src_packed")} == {True, False} and {c["x_f32"] for c in f if "lens" in c and not c.get("src_packed")} == {True, False}
    st = [c for c in f if c.get("max_wgs") or c.get("nt")]
    assert {c["D"] for c in st} == {512, 516, 2052, 4096} and {c["nt"] for c in st} == {0, 1}
    assert {c["max_wgs"] for c in st if c["R"] == 8 * c["max_wgs"] + 1} == {1, 2} and any(c["max_wgs"] > (c["R"] + 3) // 4 for c in st) and any(c["max_wgs"] == 0 for c in st)
    b = by["ln_bwd"]
    assert {c["D"] for c in b if re.fullmatch(r"lnb-D\d+", c["name"])} == {8, 12, 508, 512, 516, 1020, 1024}
    assert {c["outs"] for c in b} >= {("dx",), ("dx32",), ("dxm",), ("dx", "dx32"), ("dx", "dxm"), ("dx32", "dxm"), ("dx", "dx32", "dxm")}
    for k in ("dy32", "dy_add", "x_f32"):
        assert {c[k] for c in b} == {True, False}, k
    assert all(any(s not in c["sums"] for c in b) for s in ("dgain", "dbias", "dxcolsum")) and all(c["zero_row"] >= 0 for c in b)
    assert any("dxm" in c["outs"] and c["pm"] > 0 and c["drop_ld"] != c["D"] for c in b) and any(c["p"] > 0 for c in b)
    paths = {(c["R"], c["D"], bool(c["ws"])): A.ln_bwd_path(c["R"], c["D"], c["ws"]) for c in b}
    assert paths[1, 516, False] == (1, 0, 0) and paths[512, 12, True] == (128, 0, 0) and paths[513, 516, True] == (129, 129, 3) and paths[513, 12, False] == (129, 0, 0)
    assert paths[4101, 8, True] == (1024, 1024, 8) and paths[1029, 8, True] == (256, 256, 4) and paths[1029, 8, False] == (256, 0, 0)
    pf = by["pool_fwd"]
    assert {c["D"] for c in pf} == {64, 72, 128, 192, 384, 504, 512} and {(A.pool_cpb(D), 256 // A.pool_cpb(D)) for D in (64, 72, 192, 504)} == {(8, 32), (9, 28), (24, 10), (63, 4)}
    assert {c["segs"][0]["L"] for c in pf if c["name"].startswith("pool-D384-L")} == {1, 15, 16, 17, 63, 64, 65, 130}
    assert {c["segs"][0]["L"] for c in pf if c["name"].startswith("pool-D504-L")} == {1, 4, 16, 17}
    for c in pf:
        if re.match(r"pool-D\d+-L", c["name"]):
            L = c["segs"][0]["L"]
            assert {1, max(1, L - 1), L} <= set(c["segs"][0]["lens"])
    assert {c["wide"] for c in pf} == {True, False} and {c["copy"] for c in pf} == {True, False} and {c["packed"] for c in pf} == {True, False}
    two = [c for c in pf if len(c["segs"]) == 2]
    assert all(c["segs"][0]["L"] != c["segs"][1]["L"] for c in two) and any(c["p_w"] > 0 for c in two) and any(c["packed"] for c in two)
    assert all(A.pool_seed(c, 1) != A.pool_seed(c, 0) and A.pool_row0(c, 1) > 0 for c in two)
    for c in pf:
        if c["packed"]:  # guard rows between the sequences
            assert any(not pr["exists"].all() for pr in A.pool_rows(c))
    pk = [c for c in pf if c["counts"]]
    assert any(c["counts"][0] == 0 and c["counts"][-1] == 0 and 0 in c["counts"][2:-2] for c in pk) and any(len(c["counts"]) == 1 for c in pk)
    assert all(c["Cmax"] >= max(c["counts"]) for c in pk) and any(c["Cmax"] > max(c["counts"]) for c in pk)
    assert any(len(c["counts"]) == 260 and c["D"] == 64 and sum(c["counts"]) >= 250 for c in pk) and any(len(c["segs"]) == 2 for c in pk)
    assert all(sum(c["counts"]) == len(c["segs"][-1]["lens"]) for c in pk)
    pb = by["pool_bwd"]
    assert {c["colsum"] for c in pb} == {None, "atomics", "partials", "defer"} and sum(c["chained"] for c in pb) == 1
    assert any(len(c["segs"][0]["lens"]) == 70 and c["colsum"] == "partials" for c in pb) and any(c["p_w"] > 0 and c["p_s"] > 0 for c in pb)
    assert {c["D"] for c in by["avg_fwd"]} == {2, 510, 512, 514} == {c["D"] for c in by["avg_bwd"]} and {c["L"] for c in by["avg_fwd"]} == {1, 9}
    assert any(c["wide"] for c in by["avg_fwd"]) and any(min(c["lens"]) < c["L"] for c in by["avg_fwd"])
    for op in ("pack_fwd", "pack_bwd", "pack_join"):
        cs = by[op]
        assert {c["D"] for c in cs} >= {6, 384} and {len(c["counts"]) for c in cs} >= {1, 300}
        assert any(c["counts"][0] == 0 and c["counts"][-1] == 0 and 0 in c["counts"][2:-2] for c in cs)
    assert {(bool(c["dout2"]), bool(c["dctx"])) for c in by["pack_join"]} == {(False, False), (False, True), (True, False), (True, True)}
    cs = by["colsum"]
    assert {c["C"] for c in cs} == {2, 510, 512, 514} and {(c["R"], bool(c["ws"])) for c in cs} == {(1, False), (512, True), (513, True), (513, False)}
    assert any(c["wide"] for c in cs)
    assert len(A.CASES) == 168


def _ln_autograd(c, inp, ms):
    import torch
    t = lambda v, g=True: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=g)
    x, gain = t(A._ln_rows(c, inp)), t(inp["gain"][0] if "gain" in inp else np.ones(c["D"]))
    xc = x - x.mean(-1, keepdim=True)
    std = torch.sqrt((xc * xc).sum(-1, keepdim=True) / (c["D"] - 1))
    xhat = xc / (std + A.EPS)
    if c["op"] == "ln_fwd":
        y = xhat * gain + t(inp["bias"][0], False) if c["gain"] else xhat
        if c["pe_L"]:
            y = y + t(inp["pe"][np.arange(c["R"]) % c["pe_L"]], False)
        return dict(y=(y * t(ms["M"], False)).detach().numpy())
    bias = t(np.zeros(c["D"]))
    y = (xhat * gain + bias) * t(ms["M"], False)
    dy = inp["dy"] + (inp["dy_add"] if c["dy_add"] else 0.0)
    (y * t(dy, False)).sum().backward()
    dx = x.grad.numpy()
    return dict(dx=dx, dx32=dx, dxm=dx * ms["Mm"], dgain=gain.grad.numpy()[None], dbias=bias.grad.numpy()[None], dxcolsum=np.nansum(dx * ms["Mm"], 0, keepdims=True))  # (NaN: the std == 0 rows, left out on both sides)


def _rel(a, b, what):
    """max |a - b| relative to max(1, max |b|); every compared value must be finite, so that no NaN can hide a difference."""
    assert np.isfinite(a).all() and np.isfinite(b).all(), what
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if a.size else 0.0


def _ln_oracle(c, inp, ms):
    """The case through oracle.coot_oracle.ln_coot / ln_coot_bwd (std == 0 rows by the oracle's convention: the first term only)."""
    from oracle import coot_oracle as O
    x, D = A._ln_rows(c, inp), c["D"]
    gain = inp["gain"][0] if "gain" in inp else np.ones(D)
    if c["op"] == "ln_fwd":
        y = O.ln_coot(x, gain, inp["bias"][0] if c["gain"] else np.zeros(D), eps=A.EPS)
        if c["pe_L"]:
            y = y + inp["pe"][np.arange(c["R"]) % c["pe_L"]]
        return dict(y=y * ms["M"], y32=y * ms["M"])
    dye = (inp["dy"] + (inp["dy_add"] if c["dy_add"] else 0.0)) * ms["M"]
    dx, dgain, dbias = O.ln_coot_bwd(dye, x, gain, eps=A.EPS)
    return dict(dx=dx, dx32=dx, dxm=dx * ms["Mm"], dgain=dgain[None], dbias=dbias[None], dxcolsum=(dx * ms["Mm"]).sum(0, keepdims=True))


def _pool_autograd(c, inp, ms):
    import torch
    out = {}
    for i, pr in enumerate(A.pool_rows(c)):
        x = ("", "2")[i]
        s = torch.tensor(inp["s" + x], dtype=torch.float64, requires_grad=True)
        z = torch.tensor(inp["z" + x], dtype=torch.float64, requires_grad=True)
        pooled = []
        for n in range(pr["N"]):
            r0, Lp, ln = pr["cu"][n], pr["Lp"][n], pr["lens"][n]
            sc = torch.cat([s[r0:r0 + ln], torch.full((Lp - ln, c["D"]), A.FILL, dtype=torch.float64)])
            w = torch.softmax(sc, 0)[:ln] * torch.tensor(ms["Mw" + x][r0:r0 + ln])
            pooled.append((w * z[r0:r0 + ln]).sum(0))
        pooled = torch.stack(pooled)
        out["pooled" + x] = pooled.detach().numpy()
        if c["op"] == "pool_bwd":
            (pooled * torch.tensor(inp["dpooled" + x])).sum().backward()
            out["ds" + x], out["dz" + x] = s.grad.numpy() * ms["Ms" + x], z.grad.numpy()
    return out


@functools.lru_cache(maxsize=None)
def _evaluate(name):
    """Everything the tests below assert about one case."""
    c = A.BY_NAME[name]
    lib, T = _lib(), A.tensors(c)
    inp, ms = A.inputs(c), A.masks(c, lib)
    fed = A.pool_fed(c, lib) if c["op"] == "pool_bwd" else None
    if fed is not None and c["chained"]:  # fed what the kernel-following forward leaves
        f = A.forward_case(c)
        fed = A.pool_fed(c, lib, fwd_out=A.reference(f, A.inputs(f), A.masks(f, lib), mode="follow"))
    ref = A.reference(c, inp, ms, fed=fed)
    r = dict(autograd=None, follow={}, stored={}, applies={}, missed=[])
    if c["op"] in ("ln_fwd", "ln_bwd", "pool_fwd", "pool_bwd"):
        ag = (_ln_autograd if c["op"].startswith("ln") else _pool_autograd)(c, inp, ms)
        # a std == 0 row is left out: autograd's sqrt has the gradient 0 / 0 there (dx is NaN), and the forward's reference is the fp32 chain;
        # the oracle comparison below covers those rows
        zero = np.abs(A._ln_rows(c, inp)).sum(-1) == 0 if c["op"].startswith("ln") else None
        r["autograd"] = 0.0
        for k, v in ag.items():
            if k not in ref:
                continue
            if k.startswith("ds_") or k in c.get("sums", ()):  # an accumulating output: without its initial contents
                b = ref[k] - inp["init_" + k]
                if k == "dxcolsum":  # ... and without the zero rows, on both sides
                    b = b - (_ln_oracle(c, inp, ms)["dxm"][zero]).sum(0, keepdims=True)
                a = v
            elif zero is not None:
                assert np.isnan(v[zero]).all() or c["op"] == "ln_fwd", (name, k)
                a, b = v[~zero], ref[k][~zero]
            else:
                a, b = v[T[k]["rowmask"]], ref[k][T[k]["rowmask"]]
            r["autograd"] = max(r["autograd"], _rel(a, b, (name, k)))
        if c["op"].startswith("ln"):
            r["oracle"] = 0.0
            for k, v in _ln_oracle(c, inp, ms).items():
                if k in ref:
                    rows = ~zero if c["op"] == "ln_fwd" else slice(None)
                    b = ref[k] - inp["init_" + k] if k in c.get("sums", ()) else ref[k][rows]
                    r["oracle"] = max(r["oracle"], _rel(v if k in c.get("sums", ()) else v[rows], b, (name, k)))
    before = A.buffers(c, inp, fed=fed)
    fol = A.reference(c, inp, ms, mode="follow", fed=fed)
    for key, res in (("follow", fol), ("stored", ref)):
        bad, ratios = A.check(c, ref, A.buffers(c, inp, res, fed=fed), before)
        assert not bad, (name, key, bad)
        r[key] = ratios
    for mut in A.MUTATIONS:
        wrong = A.mutated(c, inp, lib, mut, fed=fed)
        changed = wrong is not None and any(not np.array_equal(wrong[x][T[x]["rowmask"]], ref[x][T[x]["rowmask"]], equal_nan=True) for x in A.outputs(c))
        r["applies"][mut] = changed
        if changed and not A.check(c, ref, A.buffers(c, inp, wrong, fed=fed), before)[0]:
            r["missed"].append(mut)
    # one sentinel changed above, below and beside an output window; one input element changed; one NaN in an output
    for nm in A.outputs(c):
        t = T[nm]
        for pos in ((A.GUARD - 1, 0), (A.GUARD + t["rows"], t["cols"] - 1)) + (((A.GUARD, t["ld"] - 1),) if t["ld"] > t["cols"] else ()):
            got = A.buffers(c, inp, ref, fed=fed)
            got[nm][pos] ^= 1
            if not A.check(c, ref, got, before)[0]:
                r["missed"].append(("sentinel", nm, pos))
        if t["kind"] in "hf":
            got = A.buffers(c, inp, ref, fed=fed)
            got[nm][A.GUARD + int(np.argmax(t["rowmask"])), 0] = A.nan_bits(t, "bf16")
            if not A.check(c, ref, got, before)[0]:
                r["missed"].append(("nan", nm))
    nm = next(k for k, t in T.items() if t["role"] == "in")
    got = A.buffers(c, inp, ref, fed=fed)
    got[nm][A.GUARD, 0] ^= 1
    if not A.check(c, ref, got, before)[0]:
        r["missed"].append(("input", nm))
    return r


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES if c["op"] in ("ln_fwd", "ln_bwd", "pool_fwd", "pool_bwd")])
def test_closed_form_equals_autograd(name):
    assert _evaluate(name)["autograd"] < 1e-10


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES if c["op"] in ("ln_fwd", "ln_bwd")])
def test_layernorm_reference_equals_the_oracle(name):
    """The module's own closed form (shared with the mutants) against ln_coot / ln_coot_bwd, the std == 0 rows of the backward included."""
    assert _evaluate(name)["oracle"] < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_bound_holds_for_the_kernel_following_reference(name):
    r = _evaluate(name)
    print(name, "follow", {k: round(v, 3) for k, v in r["follow"].items()}, "exact, stored", {k: round(v, 3) for k, v in r["stored"].items()})
    assert set(r["follow"]) == set(A.outputs(A.BY_NAME[name])) and max(r["follow"].values()) <= 1.0
    assert max(r["stored"].values()) <= 1.0  # storing the exact reference costs the store's half ulp at most


@pytest.mark.parametrize("name", NAMES)
def test_wrong_results_are_rejected(name):
    assert _evaluate(name)["missed"] == []


def test_every_mutation_applies_to_the_stated_number_of_cases():
    n = {}
    for c in A.CASES:
        for mut, hit in _evaluate(c["name"])["applies"].items():
            if hit:
                n.setdefault(mut, {}).setdefault(c["op"], 0)
                n[mut][c["op"]] += 1
    assert set(n) == set(A.MUTATIONS)
    assert n == APPLIES


def test_inputs_poison_what_nobody_may_read():
    for name in ("lnf-gather", "pool-packed-seg2-drop-bwd", "packj-zeros-D6", "lnb-D8"):
        c = A.BY_NAME[name]
        lib = _lib()
        fed = A.pool_fed(c, lib) if c["op"] == "pool_bwd" else None
        b = A.buffers(c, A.inputs(c), fed=fed)
        for nm, t in A.tensors(c).items():
            if t["role"] == "in" and t["kind"] in "hf":
                img = A._decode(t, b[nm], "bf16")
                win = img[A.GUARD:-A.GUARD, :t["cols"]]
                assert np.isfinite(win[t["rowmask"]]).all() and np.isnan(win[~t["rowmask"]]).all(), (name, nm)
                assert np.isnan(img[:A.GUARD]).all() and np.isnan(img[-A.GUARD:]).all() and np.isnan(img[:, t["cols"]:]).all(), (name, nm)
    assert not A.tensors(A.BY_NAME["lnf-gather"])["x"]["rowmask"].all() and A.tensors(A.BY_NAME["lnb-D8"])["x"]["ld"] > 8
