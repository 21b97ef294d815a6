"""CPU side of the loss-kernel tests: the decision-separated generator, the rounding-exact reference and the tolerance file of
tests/loss_cases.py / tools/gen_loss_tolerances.py, and the argument checks of the contrastive entry points (refused on the host,
before any launch: no device needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import coot_oracle as O
from tests import loss_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_PATH = os.path.join(ROOT, "tests", "golden", "loss_tolerances.json")


@pytest.mark.parametrize("N,d", [(7, 32), (300, 64), (129, 1024), (1300, 384)])
def test_generator_separates_every_hinge_decision(N, d):
    """No off-diagonal |margin + S_ij - S_ii| of the alignment term or of either cluster term, on the bf16-rounded normalised
    rows, is within MIN_GAP of zero; margins are violated (the loss is not trivially zero) and row norms differ."""
    sets, w, ref = LC.contrastive_case(f"gen_{N}_{d}", N, d, *LC.DUMMY_LOW)
    assert ref["gap"] >= LC.MIN_GAP
    assert ref["loss_pair"][0] > 0 and np.abs(ref["grads"][0]).max() > 0
    norms = np.linalg.norm(sets[0], axis=1)
    assert norms.max() / norms.min() > 3
    # same-cluster pairs violate, the others do not: between 1 % and 60 % of the entries
    A = O.bf16_round(sets[0] * LC.kernel_inv(sets[0])[:, None]).astype(np.float64)
    B = O.bf16_round(sets[1] * LC.kernel_inv(sets[1])[:, None]).astype(np.float64)
    S = A @ B.T
    share = ((LC.MARGIN + S - np.diag(S)[:, None] > 0).sum() - N) / (N * (N - 1))
    assert 0.01 < share < 0.6, share


def test_a_case_that_does_not_separate_is_an_error(monkeypatch):
    monkeypatch.setattr(LC, "MIN_GAP", 0.5)
    with pytest.raises(AssertionError, match="broken case"):
        LC.contrastive_case("gen_never", 40, 64, *LC.DUMMY_LOW)


def test_kernel_inv_is_the_float32_inverse_norm():
    x = LC.make_pair(50, 416, 3)[0]
    exact = 1 / np.linalg.norm(x.astype(np.float64), axis=1)
    inv = LC.kernel_inv(x)
    assert inv.dtype == np.float32
    assert np.abs(inv / exact - 1).max() < 4 * 2.0 ** -24
    assert LC.kernel_inv(np.zeros((1, 32), np.float32))[0] == np.float32(1e12)  # F.normalize: eps = 1e-12


def test_reference_term_is_the_oracles_contrastive_loss():
    a, b = LC.make_pair(37, 96, 5)
    A, B = (O.bf16_round(x * LC.kernel_inv(x)[:, None]).astype(np.float64) for x in (a, b))
    rows, dA, dB, _ = LC.hinge_term(A, B, LC.MARGIN)
    lo, da, db = O.contrastive_loss(A, B, LC.MARGIN)
    N = A.shape[0]
    assert abs(rows.sum() / N ** 2 - lo) < 1e-13
    assert np.abs(dA / N ** 2 - da).max() < 1e-13 and np.abs(dB / N ** 2 - db).max() < 1e-13
    # the float32 mirror takes the same decisions
    r32, dA32, _, _ = LC.hinge_term(A.astype(np.float32), B.astype(np.float32), LC.MARGIN, seq=True)
    assert LC.rel_max(r32, rows) < 1e-5 and LC.rel_max(dA32, dA) < 1e-5


@pytest.mark.parametrize("wname", list(LC.W_CASES) + ["all"])
def test_reference_equals_the_oracle(wname):
    """mode="exact" is O.total_contrastive_loss to fp64 round-off (weights, the weight_context_internal quirk, per-pair sums);
    mode="bf16" differs from the oracle's bf16 mode only by where the rows are rounded (fp32 norm and product against fp64)."""
    w = LC.W_CASES.get(wname, LC.W_FULL)
    sets, w, ref = LC.contrastive_case(f"w_{wname}", 40, 256, 90, 128, w)
    E = {k: s.astype(np.float64) for k, s in zip(LC.SET_NAMES, sets)}
    ex = LC.contrastive_ref(sets, w, mode="exact")
    lo, dE = O.total_contrastive_loss(E, w, LC.MARGIN)
    assert abs(ex["loss"] - lo) < 1e-12
    assert abs(sum(r.sum() for r in ex["rows"]) - lo) < 1e-12
    for k, g in zip(LC.SET_NAMES, ex["grads"]):
        assert np.abs(g - dE[k]).max() < 1e-12, k
    lb, dB = O.total_contrastive_loss(E, w, LC.MARGIN, O.BF16)
    assert abs(ref["loss"] - lb) < 1e-4 * max(lb, 1e-9)
    for k, g in zip(LC.SET_NAMES, ref["grads"]):
        assert np.abs(g - dB[k]).max() <= 3e-2 * max(np.abs(dB[k]).max(), 1e-30), k
    if wname == "high_pair_off":
        assert ref["loss_pair"][0] == 0 and not ref["grads"][0].any() and not ref["grads"][1].any()


def test_single_row_has_no_loss():
    sets, w, ref = LC.contrastive_case("one_row", 1, 32, *LC.DUMMY_LOW)
    assert ref["loss_pair"][0] == 0 and not ref["grads"][0].any() and not ref["grads"][4].any()


def test_small_path_boundary_is_derived_from_the_lds_formula():
    assert LC.small_path_fits(128, 384) and not LC.small_path_fits(129, 384)
    n = LC.largest_small_n(1024)
    assert n % 16 == 0 and LC.small_path_fits(n, 1024) and not LC.small_path_fits(n + 1, 1024)
    assert f"bound_n{n}_d1024" in LC.contrastive_cases() and f"bound_n{n + 1}_d1024" in LC.contrastive_cases()


def test_tolerance_file_covers_every_case_and_follows_its_rule():
    tol = json.load(open(TOL_PATH))
    ids = set(LC.contrastive_cases()) | set(LC.F32_CASES) | {f"cycle_{s[0]}_{s[1]}_{s[2]}_b{B}" for s in LC.CYCLE_SHAPES for B in LC.CYCLE_B}
    assert set(tol) == ids
    for k, t in tol.items():
        f = LC.CYCLE_FACTOR if k.startswith("cycle_") else LC.FACTOR
        for n in ("loss", "grad", "rows"):
            want = max(f * max(t["a_" + n], t.get("b_" + n, 0.0)), LC.TOL_FLOOR)
            assert abs(t[n] - want) <= 1e-5 * want, (k, n)
            assert t[n] < 0.05, (k, n, t[n])  # (nothing here is as loose as the cosine checks these tests replace)
        if "gap" in t:
            assert t["gap"] >= LC.MIN_GAP


def test_tolerance_file_is_reproduced():
    tol = json.load(open(TOL_PATH))
    again = LC.all_tolerances(only=LC.REGENERATED_ON_CPU)
    assert set(again) == set(LC.REGENERATED_ON_CPU)
    for k, t in again.items():
        for n, x in t.items():
            assert abs(tol[k][n] - x) <= 1e-5 * abs(x), (k, n, tol[k][n], x)


def test_cycle_cases_cover_lengths_and_positions():
    for Cc, Cs, D in LC.CYCLE_SHAPES:
        c = LC.cycle_case(Cc, Cs, D, 9)
        assert (c["lc"] >= 1).all() and (c["lc"] <= Cc).all() and 1 in c["ls"] and Cs in c["ls"] and 1 in c["lc"] and Cc in c["lc"]
        assert (c["ic"] < c["lc"]).all() and (c["isent"] < c["ls"]).all()
        assert (c["ic"] == 0).any() and (c["ic"] == c["lc"] - 1).any()
        assert not c["clip"][~c["cv"]].any() and not c["sent"][~c["sv"]].any()
        r = LC.cycle_ref(c)
        assert r["loss"] > 0 or Cc == 1 or Cs == 1


# ---- argument checks: refused before any launch ---------------------------------------------------------------------------------
def _call(lib, L, nh, nl, dh, dl, short=0, part=3):
    """coot_contrastive_fwd_bwd_part on HOST buffers (never dereferenced by a call that is refused).  Returns rc, the error text
    and whether the loss word and the gradient buffers still hold what they held."""
    cfg = L.ContrastiveConfig(0.2, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5)
    shapes = [(nh, dh), (nh, dh), (nl, dl), (nl, dl), (nh, dl), (nh, dl)]
    rs = np.random.RandomState(0)
    sets = [rs.randn(*s).astype(np.float32) for s in shapes]
    grads = [rs.randn(*s).astype(np.float32) for s in shapes]
    g0 = [g.copy() for g in grads]
    loss = np.array([0.375], np.float32)
    nbytes = lib.coot_contrastive_scratch_bytes(nh, nl, dh, dl) - short
    scratch = np.zeros(nbytes + 1, np.uint8)
    rc = lib.coot_contrastive_fwd_bwd_part(C.byref(cfg), nh, nl, dh, dl, *[s.ctypes.data for s in sets], loss.ctypes.data,
                                           *[g.ctypes.data for g in grads], scratch.ctypes.data, nbytes, part, None)
    same = loss[0] == np.float32(0.375) and all(np.array_equal(a, b) for a, b in zip(grads, g0))
    return rc, lib.coot_last_error().decode(), same


@pytest.mark.parametrize("kw,text", [(dict(dh=48), "multiples of 32"), (dict(dh=1056), "up to 1024"), (dict(dl=48), "multiples of 32"),
                                     (dict(short=1), "scratch too small"), (dict(part=0), "part")])
def test_contrastive_argument_checks(kw, text):
    import coot_videotext_amd as cva
    L = cva.lib
    lib = L.load()
    args = dict(nh=20, nl=40, dh=64, dl=32)
    args.update(kw)
    rc, msg, same = _call(lib, L, **args)
    assert rc != 0 and text in msg, (rc, msg)
    assert same
