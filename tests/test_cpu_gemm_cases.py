"""tests/gemm_cases.py without a GPU: the case table reaches every launch variant of gemm_nt, the reference passes its own checker on
every case, and the checker rejects the results of subtly wrong kernels (a lost K chunk, a row from the wrong tile, the
neighbouring group's bias, a pe position off by one, the dropout mask of another index, a column sum without one row block, one
byte written outside the output window).  Also: coot_debug_gemm_nt declared, bound, listed and exported by both builds."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gemm_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_debug_entry_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    m = re.search(r"\bcoot_debug_gemm_nt\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "const coot_gemm_nt_args* a, coot_stream_t stream"
    assert len(lib.coot_debug_gemm_nt.argtypes) == 2 and "coot_debug_gemm_nt" in cva.lib.EXPORTS
    # the ctypes structure names the header's fields in the header's order, with the header's types
    body = re.search(r"typedef struct coot_gemm_nt_args \{(.*?)\} coot_gemm_nt_args;", hdr, flags=re.S).group(1)
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
             "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float,
             "size_t": ctypes.c_size_t}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
        fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields == list(cva.lib.GemmNtArgs._fields_)
    # the fields of GemmNT / GemmEpi no caller in api.hip sets stay out of the entry
    for name in ("M_dev", "rowscale", "diag_src", "res32", "accumulate", "alpha"):
        assert name not in dict(fields)
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # a new function only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    assert any(fnmatch.fnmatchcase("coot_debug_gemm_nt", p.strip()) for p in pats) and re.search(r"\bcoot_debug_gemm_nt\b", vs)
    for doc in ("INTEGRATION.md", "README.md"):
        assert "coot_debug_gemm_nt" in open(os.path.join(ROOT, doc)).read(), doc
    declared = set(re.findall(r"\b(coot_[a-z0-9_]+)\s*\(", hdr)) - {"coot_stream_t"}
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert "coot_debug_gemm_nt" in exported, so
        assert exported == declared, (so, sorted(exported ^ declared)[:5])  # exactly the header's names


def test_debug_entry_refuses_on_the_host(cva):
    """Bad descriptors are refused before anything is launched (no GPU needed): a null descriptor, act 2 without aux, a pe table
    without segment lengths, an odd dropout row stride, and what launch_gemm_nt itself refuses (null operands, N % 8)."""
    lib = cva.lib.load()
    A = cva.lib.GemmNtArgs
    assert lib.coot_debug_gemm_nt(None, None) != 0
    ok = dict(X=64, ldx=8, W=64, ldw=8, M=16, N=8, K=8, groups=1, out=64, ldc=8)
    for bad in (dict(act=2), dict(pe=64, pe_L=0, pe_T0=4, pe_L2=1), dict(p=0.1, drop_ld=7), dict(X=None), dict(N=12), dict(ldx=12)):
        assert lib.coot_debug_gemm_nt(ctypes.byref(A(**dict(ok, **bad))), None) != 0, bad
        assert lib.coot_last_error()


def test_the_table_reaches_every_launch_variant():
    """The expected kernel of each case comes from the launcher's two formulas; all four kernels are reached, at both sides of both
    thresholds, with and without phantom row slabs, and by every family of cases that is meant to reach them."""
    by = {}
    for c in G.NT_CASES:
        by.setdefault(c["variant"], []).append(c)
    assert set(by) == {"small1", "small2", "main64", "main128"}
    v = lambda M, N, g=1: G.nt_variant(M, N, g)
    assert v(512, 480) == "small1" and v(512, 512) == "small2" and v(500, 520) == "small2" and v(513, 136) == "main64"
    assert v(2944, 2048) == "main64" and v(3064, 2040) == "main128" and v(3064, 2048) == "main128" and v(4096, 1152) == "main64"
    assert v(520, 1280, 8) == "main128" and v(520, 1280, 1) == "main64"
    shapes = {(c["M"], c["N"], c["groups"]) for c in G.NT_CASES}
    assert {(16, 8, 1), (77, 200, 1), (512, 480, 1), (512, 512, 1), (500, 520, 1), (513, 136, 1), (1000, 384, 1), (2944, 2048, 1),
            (3064, 2040, 1), (3100, 2048, 1), (520, 1280, 8)} <= shapes
    # 3100 rows: 25 slabs of 128 in a grid padded to 32 (7 phantom slabs) and a row tail of 28
    assert -(-3100 // 128) == 25 and 3100 % 128 == 28
    for fam, want in (("k-", 4), ("ld-", 4), ("epi-colsum", 4), ("var-", 4), ("xcd", 2)):
        assert len({c["variant"] for c in G.NT_CASES if c["name"].startswith(fam)}) == want, fam
    for var in ("main64", "main128"):
        assert {c["K"] for c in by[var] if c["name"].startswith("k-")} == {8, 56, 64, 72, 136}
    for var in ("small1", "small2"):
        assert {c["K"] for c in by[var] if c["name"].startswith("k-")} == {8, 40, 184, 192, 200, 392}
    for c in G.NT_CASES:
        if c["pe"]:  # the segment boundary falls inside a tile, the two segment lengths differ
            assert c["pe"][1] % G.nt_row_block(c) != 0 and c["pe"][0] != c["pe"][2] and c["pe"][1] < c["M"]
        if c["colsum"] and c["variant"].startswith("main"):
            assert c["M"] > G.nt_row_block(c)  # more than one row block
    assert sum(c["control"] for c in G.NT_CASES) == 10


@pytest.mark.parametrize("name", [c["name"] for c in G.NT_CASES])
def test_nt_reference_passes_and_wrong_results_are_rejected(cva, name):
    c = G.NT_BY_NAME[name]
    lib = cva.lib.load()
    inp = G.nt_inputs(c)
    ref = G.nt_reference(c, inp, lib)
    ratios = G.nt_check(c, inp, ref, G.nt_fake_outputs(c, inp, ref))
    assert max(ratios.values()) <= 1.0
    assert ("acc" in ratios) == c["out_f32"]
    if c["out_f32"]:  # storing the fp64 reference as fp32 costs half an ulp, 2^-24 |v| <= 1 / K of the accumulation term
        assert ratios["out"] <= 1.0 / c["K"] + 1e-3 and ratios["acc"] <= ratios["out"]
    wrong = G.nt_corruptions(c, inp, ref, lib)
    must = {"k_chunk_dropped", "byte_past_column_N_out", "byte_below_row_M_out"}
    must |= {"row_from_16_below"} if c["M"] > 16 else set()
    must |= {"bias_of_next_group"} if c["groups"] > 1 and c["bias"] else set()
    must |= {"pe_off_by_one"} if c["pe"] else set()
    must |= {"dropout_of_idx_plus_2"} if c["p"] > 0 else set()
    must |= {"colsum_without_a_row_block", "byte_past_column_N_colsum"} if c["colsum"] else set()
    must |= {"byte_past_column_N_pre", "byte_below_row_M_pre"} if c["save_pre"] else set()
    assert must == set(wrong)
    for what, got in wrong.items():
        with pytest.raises(AssertionError):
            G.nt_check(c, inp, ref, got)
            pytest.fail(f"{name}: {what} was not rejected", pytrace=False)


def test_nt_inputs_poison_their_paddings():
    c = G.NT_BY_NAME["ld-small1-fwd"]
    b = G.nt_device_inputs(c, G.nt_inputs(c))
    L = G.nt_layout(c)
    assert (L["ldx"], L["ldw"], L["ldc"], L["ldres"], L["ldaux"], L["ldpre"]) == (136 + 8, 136 + 16, 200 + 8, 200 + 24, 200 + 8, 200 + 8)
    for k, w in (("X", 136), ("W", 136), ("res", 200)):
        assert np.isnan(G.from_bf16_bits(b[k][:, w:])).all() and np.isfinite(G.from_bf16_bits(b[k][:, :w])).all()


@pytest.mark.parametrize("name", [c["name"] for c in G.TN_CASES[::5] + G.TN_BATCH])
def test_tn_reference_passes_and_wrong_results_are_rejected(name):
    c = {c["name"]: c for c in G.TN_CASES + G.TN_BATCH}[name]
    inp = G.tn_inputs(c)
    ref = G.tn_reference(c, inp)
    L = G.tn_layout(c)
    assert L["lda"] > c["groups"] * c["Mo"] and L["ldb"] > c["groups"] * c["No"] and L["ldc"] > c["No"] and L["zC"] > c["Mo"] * c["No"]
    assert max(G.tn_check(c, inp, ref, G.tn_fake_outputs(c, inp, ref)).values()) <= 1.0
    Mo, No, T = c["Mo"], c["No"], c["T"]
    wrong = []
    b = G.tn_fake_outputs(c, inp, ref)
    b["C"][No] ^= 1  # first padding column of row 0
    wrong.append(b)
    b = G.tn_fake_outputs(c, inp, ref)
    b["C"][Mo * L["ldc"] + 3] ^= 1 << 31  # the row below the window
    wrong.append(b)
    if T > 0:  # one t row missing from one element's sum; the window not added to (or not written)
        r2 = dict(ref, C=ref["C"].copy())
        r2["C"][-1, Mo - 1, No - 1] -= inp["A"][T - 1, c["groups"] * Mo - 1] * inp["B"][T - 1, c["groups"] * No - 1]
        wrong.append(G.tn_fake_outputs(c, inp, r2))
        wrong.append(G.tn_fake_outputs(c, inp, dict(ref, C=ref["C"] - inp["C0"] * (1 - 2 * c["overwrite"]))))
    else:
        wrong.append(G.tn_output_buffers(c, inp))  # "written" means zeros: the old values must not survive
    if c["colsum"]:
        wrong.append(G.tn_fake_outputs(c, inp, dict(ref, cs=ref["cs"] - inp["A"][T // 2, :Mo])))
    for got in wrong:
        with pytest.raises(AssertionError):
            G.tn_check(c, inp, ref, got)


def test_tn_table():
    assert {c["T"] for c in G.TN_CASES} == {1, 63, 64, 65, 255, 256, 257, 1000}
    assert {(c["Mo"], c["No"]) for c in G.TN_CASES} == {(8, 8), (120, 136), (384, 384)} and len(G.TN_CASES) == 24
    wide = [c for c in G.TN_BATCH if c["Mo"] % 384 == 0]
    assert any(c["colsum"] for c in wide) and any(c["groups"] > 1 and c["zC_pad"] for c in G.TN_BATCH)
    assert any(c["overwrite"] and c["T"] == 0 for c in G.TN_BATCH)
