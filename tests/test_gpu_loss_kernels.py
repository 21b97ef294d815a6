"""The contrastive and cycle-consistency kernels (csrc/loss_fused.hip, loss_f32.hip, loss.hip) on every dispatch path against a
rounding-exact fp64 reference (tests/loss_cases.py), within the per-case tolerances of tests/golden/loss_tolerances.json
(tools/gen_loss_tolerances.py: 4 x the larger of a float32 mirror's distance and the effect of one float32 ulp on the inverse
norms; 8 x the float32 mirror for the cycle-consistency kernel).  The inputs have no hinge decision within 0.02 of its threshold,
so kernel and reference take the same decisions and differ by round-off only.

Every call starts from random gradient buffers, a non-zero loss word and a scratch buffer full of NaN bit patterns (its content
is unspecified), and the assertions are on output - initial: the kernels ADD to what they are given.

Two gradient bounds are asserted.  The file's tolerance (`grad`) is the issue's 4 x max(a, b); in nine cases out of ten (b), a bf16
rounding of a row flipping under a one-ulp change of its inverse norm, sets it, at 1e-3 .. 2.5e-2 of max |gradient|.  But
tests/loss_cases.py: kernel_inv() adds the squares in the kernels' own order and gives the kernels' inverse norm bit for bit (sqrtf
and the division are correctly rounded on the device), so no rounding flips between kernel and reference, and the gradients (and
the per-row loss shares) are ALSO held to 4 x (a) alone, floored at 1e-6 (_tight()): this is the bound that carries the "fp32
round-off only" claim, the same few 1e-6 in every case.  A failure of the tight bound alone, with errors of a bf16 ulp in a few
rows, would mean that mirror no longer follows the kernels' norm.

COOT_LOSS_TEST_LOG=<file>: every measured error and its tolerance is appended there (they are printed in any case)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import loss_cases as LC

pytestmark = pytest.mark.gpu

TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_tolerances.json")))
CASES = LC.contrastive_cases()
PAIRS_OF_PART = {1: (0,), 2: (1, 2), 3: (0, 1, 2)}  # COOT_CONTRASTIVE_GLOBAL = 1 (vid | par), _LOCAL = 2 (clip | sent, vid_ctx | par_ctx)
_case_cache = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    yield torch, cva
    _case_cache.clear()


def _case(cid, mode="bf16"):
    """inputs + reference of a case, computed once per module (the fp64 reference costs seconds at thousands of rows)."""
    if cid not in _case_cache:
        if mode == "exact":
            _case_cache[cid] = LC.contrastive_case(cid, *LC.F32_CASES[cid], LC.W_FULL, "exact")
        else:
            _case_cache[cid] = LC.contrastive_case(cid, *CASES[cid])
    return _case_cache[cid]


def _record(cid, what, err, tol):
    line = f"[loss-kernels] {cid:34s} {what:28s} err {err:.3e} tol {tol:.3e}"
    print(line)
    path = os.environ.get("COOT_LOSS_TEST_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _cfg(cva, w):
    return cva.lib.ContrastiveConfig(LC.MARGIN, w["weight_high"], w["weight_high_internal"], w["weight_low"], w["weight_low_internal"],
                                     w["weight_context"], w["weight_context_internal"])


def _init_like(torch, ref, seed, shape=None):
    """A non-zero start value for an output the kernel adds to: random, a quarter of the reference's scale (1e-3 where the
    reference is zero), so that adding to it costs the result no more than an ulp of its own size."""
    ref = np.asarray(ref, np.float64)
    scale = 0.25 * float(np.abs(ref).max()) if ref.size and np.abs(ref).max() > 0 else 1e-3
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape if shape is not None else ref.shape), generator=g) * scale).float().cuda()


def _loss_word(torch, ref_loss):
    return torch.tensor([0.25 * float(ref_loss) if ref_loss != 0 else 2.0 ** -10], dtype=torch.float32, device="cuda")


def _scratch(torch, nbytes):
    return torch.full((int(nbytes),), 255, dtype=torch.uint8, device="cuda")


def _delta(out, init):
    return (out.double() - init.double()).cpu().numpy()


def _tight(tol, what):
    """4 x the float32 mirror's distance alone (the reference has the kernels' own inverse norms: module docstring)."""
    return max(LC.FACTOR * tol["a_" + what], LC.TOL_FLOOR)


def _check_loss(cid, what, got, ref, tol):
    if ref == 0:
        assert got == 0, (cid, what, got)
        return
    err = abs(got - ref) / abs(ref)
    _record(cid, what + " loss", err, tol)
    assert err <= tol, (cid, what, got, ref, err, tol)


def _check_grad(cid, what, delta, ref, tol):
    if not np.abs(ref).max() > 0:
        assert not np.any(delta), (cid, what, "the reference gradient is zero: the buffer must stay as it was")
        return 0.0
    err = LC.rel_max(delta, ref)
    assert err <= tol[0], (cid, what, err, tol)
    assert err <= tol[1], (cid, what, err, tol, "within the issue's tolerance but not within 4 x the float32 mirror's distance")
    return err


def _run(env, cid, part=3, fwd_only=False, mode="bf16", what=None):
    """One call of coot_contrastive_fwd_bwd_part (or _f32) on case `cid`; checks the loss and the gradients of the pairs of `part`
    and that the other pairs' gradients were left alone.  Returns the loss word after the call (float)."""
    torch, cva = env
    lib = cva.lib.load()
    sets, w, ref = _case(cid, mode)
    tol = TOL[cid]
    nh, dh, nl, dl = sets[0].shape[0], sets[0].shape[1], sets[2].shape[0], sets[2].shape[1]
    ts = [torch.from_numpy(s).cuda() for s in sets]
    pairs = PAIRS_OF_PART[part]
    ref_loss = float(sum(ref["loss_pair"][p] for p in pairs))
    loss0 = _loss_word(torch, ref_loss)
    loss = loss0.clone()
    g0 = [_init_like(torch, ref["grads"][s], 100 + s) for s in range(6)]
    g = [x.clone() for x in g0]
    gp = [None] * 6 if fwd_only else [x.data_ptr() for x in g]
    sp = torch.cuda.current_stream().cuda_stream
    if mode == "exact":
        scratch = _scratch(torch, lib.coot_contrastive_f32_scratch_bytes(nh, nl, dh, dl))
        cva.lib.check(lib.coot_contrastive_fwd_bwd_f32(C.byref(_cfg(cva, w)), nh, nl, dh, dl, *[t.data_ptr() for t in ts], loss.data_ptr(), *gp,
                                                       scratch.data_ptr(), scratch.numel(), sp), "contrastive_f32")
    else:
        scratch = _scratch(torch, lib.coot_contrastive_scratch_bytes(nh, nl, dh, dl))
        cva.lib.check(lib.coot_contrastive_fwd_bwd_part(C.byref(_cfg(cva, w)), nh, nl, dh, dl, *[t.data_ptr() for t in ts], loss.data_ptr(), *gp,
                                                        scratch.data_ptr(), scratch.numel(), part, sp), "contrastive_part")
    torch.cuda.synchronize()
    what = what or f"part {part}" + (" fwd" if fwd_only else "")
    _check_loss(cid, what, float(_delta(loss, loss0)[0]), ref_loss, tol["loss"])
    worst = 0.0
    for s in range(6):
        if fwd_only or s // 2 not in pairs:
            assert torch.equal(g[s], g0[s]), (cid, what, LC.SET_NAMES[s], "not part of the call, but written")
        else:
            worst = max(worst, _check_grad(cid, f"{what} {LC.SET_NAMES[s]}", _delta(g[s], g0[s]), ref["grads"][s], (tol["grad"], _tight(tol, "grad"))))
    if not fwd_only:
        _record(cid, what + " grads", worst, _tight(tol, "grad"))
    return float(loss)


class _Option:
    """coot_set_option(name, value) for a block, restored to `default` behind it."""

    def __init__(self, cva, name, value, default):
        self.lib, self.name, self.value, self.default = cva.lib.load(), name.encode(), value, default

    def __enter__(self):
        assert self.lib.coot_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        self.lib.coot_set_option(self.name, self.default)
        return False


# ---- bf16 path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("tmpl_")])
def test_template_selection_and_padding_rows(env, cid):
    """cl_small_kernel<1..4> by d, padding rows where N % 16 != 0, N = 1 (loss 0, gradients 0): one pair via `part`, the two
    local pairs, and all three."""
    for part in (1, 2, 3):
        _run(env, cid, part)


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("bound_")])
def test_one_launch_three_launch_boundary(env, cid):
    n, d = CASES[cid][:2]
    nmax = LC.largest_small_n(1024)
    assert LC.small_path_fits(128, 384) and not LC.small_path_fits(129, 384) and LC.small_path_fits(nmax, 1024) and not LC.small_path_fits(nmax + 1, 1024)
    _run(env, cid, 1)


def test_mixed_call_small_high_pair_large_low_pair(env):
    """The high pair qualifies for the one-launch path, the low pair does not: the whole call takes three launches."""
    assert LC.small_path_fits(64, 768) and not LC.small_path_fits(230, 384)
    for part in (3, 1, 2):
        _run(env, "mixed_small_high_large_low", part)


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("split_")])
def test_column_splits_by_size(env, cid):
    _run(env, cid, 1)


@pytest.mark.parametrize("cid", ["forced_n300_d64", "forced_n40_d128"])
@pytest.mark.parametrize("cs", [2, 3, 5, 8])
def test_forced_column_splits(env, cid, cs):
    """coot_set_option("cl_col_split", k), set before the scratch is sized.  The host keeps only splits that have columns (32 per
    split at least): at N = 300 (320 padded columns) the forced 2, 3, 5, 8 become 2, 3, 5, 5 splits; at N = 40 (48 padded columns) all
    four become 2 — that case is about the loop that drops the empty ones.  Eight real splits: test_column_splits_by_size."""
    with _Option(env[1], "cl_col_split", cs, 0):
        _run(env, cid, 1, what=f"col_split {cs}")


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("clamp_")])
def test_load_clamps_of_the_three_launch_path(env, cid):
    """cl_half loads k-blocks in groups of 12 and output fragments in groups of 24, clamping the addresses past the end: d = 384
    fills the groups exactly, d = 416 is one over, d = 1024 the widest."""
    with _Option(env[1], "cl_small", 0, 1):
        _run(env, cid, 1, what="cl_small 0")


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("w_")])
@pytest.mark.parametrize("small", [1, 0])
def test_weights(env, cid, small):
    """Alignment only, cluster only, the context cluster term weighted by weight_low_internal, a pair with all its weights zero
    (its gradients stay as they were)."""
    with _Option(env[1], "cl_small", small, 1):
        _run(env, cid, 3, what=f"cl_small {small}")


@pytest.mark.parametrize("cid", ["tmpl_n100_d512", "mixed_small_high_large_low", "split_n513_d64"])
def test_forward_only_call(env, cid):
    """Null gradient pointers: the same loss word, bit for bit, as the forward + backward call from the same start value."""
    part = 1 if cid.startswith("split_") else 3
    assert _run(env, cid, part, fwd_only=True) == _run(env, cid, part)


# ---- data parallel ----------------------------------------------------------------------------------------------------------------
def _dp_check(cid, what, ref, tol, win, loss_delta, own, own0):
    """win = (high row0, high rows, low row0, low rows); own / own0: the six compact gradient buffers after / before the call,
    each with one guard row behind the window's rows."""
    nh, nl = ref["rows"][0].shape[0], ref["rows"][1].shape[0]
    hs, ls = slice(win[0], win[0] + win[1]), slice(win[2], win[2] + win[3])
    share = float(ref["rows"][0][hs].sum() + ref["rows"][2][hs].sum() + ref["rows"][1][ls].sum())
    if win[1] == nh and win[3] == nl:
        bound = tol["loss"] * share
    else:  # a partial sum of per-row shares, each within 4 x (a) of the largest row of its pair (kernel and reference share their norms)
        bound = _tight(tol, "rows") * (win[1] * (ref["rows"][0].max() + ref["rows"][2].max()) + win[3] * ref["rows"][1].max())
    _record(cid, what + " loss share", abs(loss_delta - share), bound)
    if win[1] == 0 and win[3] == 0:
        assert loss_delta == 0.0, (cid, what, loss_delta)
    assert abs(loss_delta - share) <= bound, (cid, what, loss_delta, share, bound)
    worst = 0.0
    for s in range(6):
        sl = ls if s in (2, 3) else hs
        n = sl.stop - sl.start
        assert np.array_equal(own[s][n:], own0[s][n:]), (cid, what, LC.SET_NAMES[s], "rows behind the window were written")
        if n == 0:
            continue
        err = float(np.abs((own[s][:n].astype(np.float64) - own0[s][:n].astype(np.float64)) - ref["grads"][s][sl]).max() / np.abs(ref["grads"][s]).max())
        assert err <= tol["grad"] and err <= _tight(tol, "grad"), (cid, what, LC.SET_NAMES[s], err, tol["grad"], _tight(tol, "grad"))
        worst = max(worst, err)
    _record(cid, what + " own-row grads", worst, _tight(tol, "grad"))


def _own_buffers(torch, ref, win):
    own0 = []
    for s in range(6):
        n = win[3] if s in (2, 3) else win[1]
        own0.append(_init_like(torch, ref["grads"][s], 200 + s, shape=(n + 1, ref["grads"][s].shape[1])))
    return own0, [x.clone() for x in own0]


@pytest.mark.parametrize("cid", ["dp_h70_l333", "dp_h600_l1500"])
def test_dp_windows_on_strided_views(env, cid):
    """coot_contrastive_fwd_bwd_dp on the trainer's gathered layout ([n, vid | par | vid_ctx | par_ctx] and [n, clip | sent]): a
    one-row window, a window that ends mid-strip, an empty window (loss share 0, nothing written) and the whole batch."""
    torch, cva = env
    lib = cva.lib.load()
    sets, w, ref = _case(cid)
    nh, dh, nl, dl = CASES[cid][:4]
    t = [torch.from_numpy(s).cuda() for s in sets]
    high = torch.cat([t[0], t[1], t[4], t[5]], dim=1).contiguous()
    low = torch.cat([t[2], t[3]], dim=1).contiguous()
    hp, lp = high.data_ptr(), low.data_ptr()
    ptrs = (C.c_void_p * 6)(hp, hp + 4 * dh, lp, lp + 4 * dl, hp + 8 * dh, hp + 8 * dh + 4 * dl)
    lds = (C.c_int64 * 6)(high.shape[1], high.shape[1], low.shape[1], low.shape[1], high.shape[1], high.shape[1])
    scratch = _scratch(torch, lib.coot_contrastive_scratch_bytes(nh, nl, dh, dl))
    for win in ((5, 1, 5, 1), (16, 23, 32, 50), (7, 0, 9, 0), (0, nh, 0, nl)):
        own0, own = _own_buffers(torch, ref, win)
        down = (C.c_void_p * 6)(*[x.data_ptr() for x in own])
        loss0 = _loss_word(torch, ref["loss"])
        loss = loss0.clone()
        cva.lib.check(lib.coot_contrastive_fwd_bwd_dp(C.byref(_cfg(cva, w)), nh, nl, dh, dl, C.byref(ptrs), C.byref(lds), loss.data_ptr(), C.byref(down),
                                                      *win, scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream), "contrastive_dp")
        torch.cuda.synchronize()
        _dp_check(cid, f"window {win}", ref, TOL[cid], win, float(_delta(loss, loss0)[0]), [x.cpu().numpy() for x in own], [x.cpu().numpy() for x in own0])


def test_dp_gathered_blocks_ragged_ranks(env):
    """coot_contrastive_fwd_bwd_dp_blocks: three ranks with ragged row counts, one of them without rows, every rank's call against
    the same reference of the gathered batch."""
    torch, cva = env
    lib = cva.lib.load()
    cid = "dp_h70_l333"
    sets, w, ref = _case(cid)
    nh, dh, nl, dl = CASES[cid][:4]
    ch, cl = [30, 0, 40], [150, 0, 183]
    assert sum(ch) == nh and sum(cl) == nl
    world = 3
    parts, base, off = [], [[0] * world for _ in range(6)], 0
    for r in range(world):  # a rank's block: its rows of the six sets, dense, one after the other
        for s in range(6):
            cnt, r0 = (cl, sum(cl[:r])) if s in (2, 3) else (ch, sum(ch[:r]))
            rows = sets[s][r0:r0 + cnt[r]]
            base[s][r] = off
            parts.append(rows.reshape(-1))
            off += rows.size
    blocks = torch.from_numpy(np.concatenate(parts)).cuda()
    set_base = (C.c_int64 * (6 * world))(*[base[s][r] for s in range(6) for r in range(world)])
    lds = (C.c_int64 * 6)(dh, dh, dl, dl, dl, dl)
    counts_h, counts_l = (C.c_int64 * world)(*ch), (C.c_int64 * world)(*cl)
    scratch = _scratch(torch, lib.coot_contrastive_scratch_bytes(nh, nl, dh, dl))
    total = 0.0
    for r in range(world):
        win = (sum(ch[:r]), ch[r], sum(cl[:r]), cl[r])
        own0, own = _own_buffers(torch, ref, win)
        down = (C.c_void_p * 6)(*[x.data_ptr() for x in own])
        loss0 = _loss_word(torch, ref["loss"])
        loss = loss0.clone()
        cva.lib.check(lib.coot_contrastive_fwd_bwd_dp_blocks(C.byref(_cfg(cva, w)), world, r, counts_h, counts_l, dh, dl, blocks.data_ptr(), set_base,
                                                             C.byref(lds), loss.data_ptr(), C.byref(down), scratch.data_ptr(), scratch.numel(),
                                                             torch.cuda.current_stream().cuda_stream), "contrastive_dp_blocks")
        torch.cuda.synchronize()
        d = float(_delta(loss, loss0)[0])
        total += d
        _dp_check(cid, f"blocks rank {r}", ref, TOL[cid], win, d, [x.cpu().numpy() for x in own], [x.cpu().numpy() for x in own0])
    _check_loss(cid, "blocks, all ranks", total, float(ref["loss"]), TOL[cid]["loss"])


# ---- fp32 path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(LC.F32_CASES))
def test_fp32_path_against_the_exact_loss(env, cid):
    _run(env, cid, 3, mode="exact", what="f32")


# ---- cycle consistency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", LC.CYCLE_B)
@pytest.mark.parametrize("shape", LC.CYCLE_SHAPES)
def test_cycle_consistency(env, shape, B):
    """coot_cyclecons_fwd_bwd (fp32 throughout) against the oracle's rows, loss and gradients: up to 64 x 64 positions, D up to 1024
    and not a multiple of 64, lengths 1 and full, the first / last / a middle valid position selected."""
    torch, cva = env
    lib = cva.lib.load()
    Cc, Cs, D = shape
    cid = f"cycle_{Cc}_{Cs}_{D}_b{B}"
    c = LC.cycle_case(Cc, Cs, D, B)
    ref, tol = LC.cycle_ref(c), TOL[cid]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    clip, sent, lc, ls, ic, isent = (dev(c[k]) for k in ("clip", "sent", "lc", "ls", "ic", "isent"))
    loss0 = _loss_word(torch, ref["loss"])
    loss = loss0.clone()
    d0 = [_init_like(torch, ref["dclip"], 1), _init_like(torch, ref["dsent"], 2)]
    d = [x.clone() for x in d0]
    rows = [torch.full((B, Cc), float("nan"), device="cuda"), torch.full((B, Cs), float("nan"), device="cuda")]
    cva.lib.check(lib.coot_cyclecons_fwd_bwd(clip.data_ptr(), sent.data_ptr(), lc.data_ptr(), ls.data_ptr(), ic.data_ptr(), isent.data_ptr(), B, Cc, Cs, D,
                                             LC.CYCLE_WEIGHT, 1.0 / B, loss.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "cyclecons")
    torch.cuda.synchronize()
    _check_loss(cid, "cyclecons", float(_delta(loss, loss0)[0]), float(ref["loss"]), tol["loss"])
    for k, got in zip(("rows_clip", "rows_sent"), rows):
        err = LC.rel_max(got.double().cpu().numpy(), ref[k])
        _record(cid, k, err, tol["rows"])
        assert err <= tol["rows"], (cid, k, err, tol["rows"])
    for k, got, g0 in zip(("dclip", "dsent"), d, d0):
        err = _check_grad(cid, k, _delta(got, g0), ref[k], (tol["grad"], tol["grad"]))
        _record(cid, k, err, tol["grad"])
    # forward only: the same loss word, nothing else written
    loss_f = loss0.clone()
    cva.lib.check(lib.coot_cyclecons_fwd_bwd(clip.data_ptr(), sent.data_ptr(), lc.data_ptr(), ls.data_ptr(), ic.data_ptr(), isent.data_ptr(), B, Cc, Cs, D,
                                             LC.CYCLE_WEIGHT, 1.0 / B, loss_f.data_ptr(), None, None, None, None, torch.cuda.current_stream().cuda_stream),
                  "cyclecons")
    torch.cuda.synchronize()
    _check_loss(cid, "cyclecons fwd", float(_delta(loss_f, loss0)[0]), float(ref["loss"]), tol["loss"])
