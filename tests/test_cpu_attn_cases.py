"""tests/attn_cases.py without a GPU: the closed-form fp64 reference equals float64 autograd on every case, the kernel-following
reference stays within the derived bound of the exact one (the bound is attainable), and the checker rejects the results of
subtly wrong kernels on every case where the mutation changes the outputs.  Also: coot_debug_attn declared, bound, listed,
exported by both builds and refusing bad descriptors on the host.

Cases each mutation changes (forward outputs / backward outputs), of 38; asserted below:"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#                  mutation        fwd bwd
APPLIES = dict(lens_plus=(33, 33),      # lens + 1 (not in packed rows: the row does not exist; not where every lens = Lk)
               lens_minus=(36, 36),     # lens - 1 (not where every lens = 1)
               pad_q_dropped=(0, 24),   # padded query rows left out of dK and dV (padded self-attention)
               no_scale=(0, 36),        # scale missing from dS (dS = 0 where every sequence has one valid key)
               skip_tile=(38, 36),      # the 16-key tile with the last valid key skipped in P V and dS K
               swap_heads=(38, 38),     # heads 0 and 1 swapped
               mask_row=(6, 6),         # the dropout mask of the next mask row
               seed2=(2, 2),            # segment 2 drawing from segment 1's key
               dv_nomask=(0, 6),        # the forward mask not applied in dV
               lens_next=(36, 36),      # sequence n reading lens[n + 1]
               lse_max=(36, 0),         # lse replaced by the row maximum (equal where a row has one key)
               dk_filled=(0, 33))       # dK of a filled key not zero (padded layouts with a lens < Lk)


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _lib():
    import coot_videotext_amd as m
    return m.lib.load()


def test_debug_entry_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    m = re.search(r"\bcoot_debug_attn\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "const coot_attn_args* a, int backward, coot_stream_t stream"
    assert len(lib.coot_debug_attn.argtypes) == 3 and "coot_debug_attn" in cva.lib.EXPORTS
    body = re.search(r"typedef struct coot_attn_args \{(.*?)\} coot_attn_args;", hdr, flags=re.S).group(1)
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p,
             "const int*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
             "unsigned": ctypes.c_uint, "float": ctypes.c_float}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
        fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields == list(cva.lib.AttnArgs._fields_)
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # a new function and a new struct only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    assert re.search(r"\bcoot_debug_attn\b", vs)
    for doc in ("INTEGRATION.md", "README.md"):
        assert "coot_debug_attn" in open(os.path.join(ROOT, doc)).read(), doc
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        assert "coot_debug_attn" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, so
    # one quantisation of p and one second-segment seed offset in the sources: the networks, the host mask generator and this entry share them
    csrc = os.path.join(ROOT, "coot-videotext_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    assert sum(s.count("0x9E3779B97F4A7C15") for s in src.values()) == 1 and "kAttnSeed2Delta" in src["api_loss.hip"]
    assert sum(s.count("4294967296.0") for f, s in src.items() if f != "api_loss.hip") == 1 and "make_drop(" in src["api.hip"]
    assert int(A.SEED2_DELTA) == int(re.search(r"kAttnSeed2Delta = (0x[0-9A-Fa-f]+)", src["attention.h"]).group(1), 16)


def test_debug_entry_refuses_on_the_host(cva):
    """Bad descriptors are refused before anything is launched (no GPU needed)."""
    lib = cva.lib.load()
    T = cva.lib.AttnArgs
    assert lib.coot_debug_attn(None, 0, None) != 0
    ok = dict(q=64, ldq=96, k=64, ldk=96, v=64, ldv=96, o=64, ldo=32, lse=64, lens=64, Nseq=2, Lq=20, Lk=20, H=2, dh=16,
              dout=64, lddo=32, delta=64, dq=64, lddq=96, dk=64, lddk=96, dv=64, lddv=96)
    both = (dict(q=None), dict(lse=None), dict(lens=None), dict(dh=24), dict(dh=80), dict(ldq=100), dict(ldo=24), dict(Nseq=0), dict(Lk=0),
            dict(p=1.0), dict(p=-0.5), dict(Nseq2=-1), dict(Nseq2=3, L2=20), dict(Nseq2=3, L2=200, lens2=64), dict(Nseq2=3, L2=20, lens2=64, Lq=150, Lk=150),
            dict(cu=64, Lq=1), dict(cu=64, Lq=130, Lk=130))
    for back, bads in ((0, both), (1, both + (dict(dout=None), dict(delta=None), dict(dq=None), dict(dv=None), dict(lddk=12), dict(lddo=16)))):
        for bad in bads:
            assert lib.coot_debug_attn(ctypes.byref(T(**dict(ok, **bad))), back, None) != 0, (back, bad)
            assert lib.coot_last_error()


def test_the_table_covers_every_axis():
    by = {}
    for c in A.CASES:
        by.setdefault(c["family"], []).append(c)
        assert c["H"] >= 2 and c["Nseq"] + c["Nseq2"] <= 11 and min(c["lens"]) >= 1
    assert set(by) == {"q1", "short", "chunked"}
    fam = A.family_of
    assert fam(1, 64) == "q1" and fam(1, 65) == "chunked" and fam(1, 1) == "q1" and fam(128, 128) == "short" and fam(129, 129) == "chunked"
    assert fam(80, 80, 6, 80) == "short" and fam(1, 20, 2, 20) != "q1"
    for f, cs in by.items():
        assert {c["dh"] for c in cs} == {16, 32, 48, 64}, f
        assert any(c["p"] > 0 for c in cs) and any(c["shared"] for c in cs) and any(c["chained"] for c in cs), f
    assert {c["Lk"] for c in by["short"] if c["name"].startswith("short-L")} == {2, 15, 16, 17, 33, 80, 127, 128}
    for c in by["short"]:
        if c["name"].startswith("short-L"):
            L = c["Lk"]
            assert {1, L - 1 or 1, L} <= set(c["lens"]) and (L < 16 or any(l % 16 for l in c["lens"] if 1 < l < L - 1))
    n9 = [c for c in A.CASES if c["Nseq"] == 9 and c["H"] == 3]
    assert {c["xcd"] for c in n9} == {None, 0} and len(n9) == 2
    assert {c["Lk"] for c in by["chunked"] if c["kind"] == "self"} == {129, 150, 192, 193}
    for c in by["chunked"]:
        if c["kind"] == "self":  # lens end in the first, a middle and the last 64-row chunk
            ch = {(l - 1) // 64 for l in c["lens"]}
            assert 0 in ch and (c["Lk"] - 1) // 64 in ch and len(ch) >= 3
    cross = [c for c in A.CASES if c["kind"] == "cross"]
    assert {c["Lk"] for c in cross if c["family"] == "q1"} >= {1, 20, 63, 64} and {c["Lk"] for c in cross if c["family"] == "chunked"} == {65, 130}
    assert any(c["kind"] == "self" and c["Lk"] == 1 and c["family"] == "q1" for c in A.CASES)
    for c in cross:  # q its own matrix, k and v views of one matrix with ld = 2 D
        ops = A.layout(c)["ops"]
        assert ops["k"][0] == ops["v"][0] != ops["q"][0] and ops["k"][2] == 2 * c["H"] * c["dh"]
    seg2 = [c for c in A.CASES if c["Nseq2"] and not c["packed"]]
    assert {(c["Lk"], c["L2"]) for c in seg2} == {(80, 80), (20, 80), (64, 16)} and any(c["p"] > 0 for c in seg2)
    assert all(c["Nseq"] + c["Nseq2"] == 11 and c["lens"] != c["lens2"] for c in seg2)
    for c in seg2:  # the rows of segment 2 start right behind segment 1
        assert A.sequences(c)[c["Nseq"]]["kr0"] == c["Nseq"] * c["Lk"]
    packed = [c for c in A.CASES if c["packed"]]
    assert {bool(c["Nseq2"]) for c in packed} == {False, True} and any(c["p"] > 0 for c in packed)
    for c in packed:
        assert {1, c["Lk"]} <= set(c["lens"]) and not A.layout(c)["krows"].all()  # unused rows between the sequences
    assert sum(c["wide"] for c in A.CASES) == 1
    for c in A.CASES:
        if c["kind"] == "self":
            ops = A.layout(c)["ops"]
            assert ops["q"][0] == ops["k"][0] == ops["v"][0] and ops["dq"][0] == ops["dk"][0] == ops["dv"][0] != ops["q"][0]
    assert len(A.CASES) == 38


def _autograd(c, inp, masks):
    import torch
    H, dh = c["H"], c["dh"]
    scale = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
    L = A.layout(c)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k != "dout") for k, v in inp.items()}
    o, lse = torch.zeros(L["Tq"], L["D"], dtype=torch.float64), torch.zeros(L["Tq"], H, dtype=torch.float64)
    for s, M in zip(A.sequences(c), masks):
        hd = lambda x, r0, n: x[r0:r0 + n].reshape(n, H, dh).permute(1, 0, 2)
        q, k, v = hd(t["q"], s["qr0"], s["Lq"]), hd(t["k"], s["kr0"], s["Lk"]), hd(t["v"], s["kr0"], s["Lk"])
        S = (q @ k.transpose(1, 2)) * scale
        S = S.masked_fill(torch.arange(s["Lk"]) >= s["nvalid"], A.FILL)
        P = torch.softmax(S, -1)
        if M is not None:
            P = P * torch.tensor(M)
        o[s["qr0"]:s["qr0"] + s["Lq"]] = (P @ v).permute(1, 0, 2).reshape(s["Lq"], -1)
        lse[s["qr0"]:s["qr0"] + s["Lq"]] = torch.logsumexp(S, -1).T
    (o * t["dout"]).sum().backward()
    return dict(o=o.detach().numpy(), lse=lse.detach().numpy(), dq=t["q"].grad.numpy(), dk=t["k"].grad.numpy(), dv=t["v"].grad.numpy())


@functools.lru_cache(maxsize=None)
def _evaluate(name):
    """Everything the tests below assert about one case."""
    c = A.BY_NAME[name]
    lib = _lib()
    inp = A.attn_inputs(c)
    masks = A.drop_masks(c, lib)
    ref = A.attn_reference(c, inp, masks)
    L = A.layout(c)
    r = dict(autograd=0.0, follow={}, fake={}, applies={}, missed=[])
    ag = _autograd(c, inp, masks)
    for x in ("o", "lse", "dq", "dk", "dv"):
        r["autograd"] = max(r["autograd"], float(np.abs(ag[x] - ref[x]).max() / max(1.0, np.abs(ref[x]).max())))
    # the kernel-following reference, fed as the GPU test feeds the kernels
    fed = dict(o=A._bf(ref["o"]), lse=ref["lse"].astype(np.float32).astype(np.float64))
    fol = A.attn_reference(c, inp, masks, mode="follow")
    if c["chained"]:
        fed = dict(o=A._bf(fol["o"]), lse=fol["lse"].astype(np.float32).astype(np.float64))
        fol = A.attn_reference(c, inp, masks, mode="follow", fed=fed)
    for d in ("fwd", "bwd"):
        before = A.buffers(c, inp, fed if d == "bwd" else None)
        r["follow"].update(A.attn_check(c, ref, A.buffers(c, inp, fed if d == "bwd" else None, fol, d), d, before))
        r["fake"].update(A.attn_check(c, ref, A.buffers(c, inp, fed if d == "bwd" else None, ref, d), d, before))
    for mut in A.MUTATIONS:
        wrong = A.mutated(c, inp, lib, mut)
        for d in ("fwd", "bwd"):
            rows = lambda x: L["qrows"] if x in ("o", "lse", "dq") else L["krows"]
            changed = wrong is not None and any((wrong[x][rows(x)] != ref[x][rows(x)]).any() for x in A.OUTPUTS[d])
            r["applies"][mut, d] = changed
            if changed:
                try:
                    A.attn_check(c, ref, A.buffers(c, inp, None, wrong, d), d)
                    r["missed"].append((mut, d))
                except AssertionError:
                    pass
    # one sentinel byte changed next to an output window, one guard row of an input changed
    for d, name in (("fwd", "oo"), ("fwd", "lse"), ("bwd", A.layout(c)["ops"]["dq"][0]), ("bwd", A.layout(c)["ops"]["dk"][0])):
        for pos in ((A.GUARD - 1, 0), (-A.GUARD, -1), (A.GUARD, -1)):
            got = A.buffers(c, inp, None, ref, d)
            if name == "lse" and pos[1] == -1 and pos[0] == A.GUARD:
                continue  # lse has no column gap
            got[name][pos] ^= 0x0100
            try:
                A.attn_check(c, ref, got, d)
                r["missed"].append(("sentinel", name, pos))
            except AssertionError:
                pass
    got = A.buffers(c, inp, None, ref, "fwd")
    got["oo"][A.GUARD + int(np.argmax(L["qrows"])), 0] = A.NAN16
    try:
        A.attn_check(c, ref, got, "fwd")
        r["missed"].append("nan")
    except AssertionError:
        pass
    return r


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES])
def test_closed_form_equals_autograd(name):
    assert _evaluate(name)["autograd"] < 1e-12


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES])
def test_bound_holds_for_the_kernel_following_reference(name):
    r = _evaluate(name)
    print(name, "follow", {k: round(v, 3) for k, v in r["follow"].items()}, "exact, stored", {k: round(v, 3) for k, v in r["fake"].items()})
    assert set(r["follow"]) == {"o", "lse", "dq", "dk", "dv"} and max(r["follow"].values()) <= 1.0
    assert max(r["fake"].values()) <= 1.0  # storing the exact reference costs the store's half ulp at most


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES])
def test_wrong_results_are_rejected(name):
    assert _evaluate(name)["missed"] == []


def test_every_mutation_applies_to_the_stated_number_of_cases():
    n = {m: tuple(sum(_evaluate(c["name"])["applies"][m, d] for c in A.CASES) for d in ("fwd", "bwd")) for m in A.MUTATIONS}
    assert all(max(v) > 0 for v in n.values()), n
    assert n == APPLIES


def test_inputs_poison_their_paddings():
    for name in ("short-wide", "packed-2seg", "cross-Lk20"):
        c = A.BY_NAME[name]
        L = A.layout(c)
        b = A.buffers(c, A.attn_inputs(c))
        for x in ("q", "k", "v", "dout"):
            buf, col, ld = L["ops"][x]
            img = A.from_bf16_bits(b[buf])
            rows = L["qrows"] if x in ("q", "dout") else L["krows"]
            assert np.isfinite(img[A.GUARD:-A.GUARD, col:col + L["D"]][rows]).all()
            assert np.isnan(img[:A.GUARD]).all() and np.isnan(img[-A.GUARD:]).all() and np.isnan(img[A.GUARD:-A.GUARD][~rows]).all()
        if c["wide"]:
            assert np.isnan(A.from_bf16_bits(b["qkv"])[:, L["D"]:L["D"] + 8]).all() and L["ops"]["k"][1] == L["D"] + 8
        off, ld = A.operand_offset(c, "k")
        assert off % 8 == 0 and ld % 8 == 0
