"""Deterministic mode's segment flushes (csrc/api_step.hip: g_det_seg, coot_set_option("det_seg_flush")).

In overwrite mode a backward pass WRITES every weight-matrix gradient, so a deterministic step flushes only the words between those
matrices (biases, LayerNorm parameters), and where it updates it does so inside the update launch; the global networks' early update
runs in this mode too.  Two things make that safe, and both are checked here:
  * after a step EVERY word of the fixed-point shadow is zero — no addend landed outside the flushed segments (a sum left there would
    be lost to this step and added to the next) — on every route of the step: plain, timed (lookahead + deferred join), ragged packed
    rows, no update, the one-rank data-parallel phase calls and a captured step;
  * steps with the switch on and off compute the same bits (parameters and losses).
"""
import pytest

from oracle import coot_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DIMS = (256, 192, 384, 8, 384, 768)  # d_model 384: the fused token-tile chains and the single-launch global networks


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _batches(cva, ragged):
    # 32 videos x 4 clips x 64 frames: the video side has 10 240 token rows, above kEarlyMinTokens — its global network takes the early
    # update; the text side (4 096 rows) updates it at the tail
    if ragged:
        return [cva.synthetic.make_batch(60 + i, 24, cva.synthetic.anet_like_counts(90 + i, 24), 64, 64, 32, 16, DIMS[0], DIMS[1], ragged=True,
                                         packed=True) for i in range(2)]
    return [cva.synthetic.make_batch(60 + i, 32, 4, 64, 64, 32, 16, DIMS[0], DIMS[1], ragged=False) for i in range(2)]


def _set_seg(cva, on):
    lib = cva.lib.load()
    cva.lib.check(lib.coot_set_option(b"det_seg_flush", int(on)), "coot_set_option")


def _steps(torch, cva, batches, steps, seg=True, lookahead=False, defer=False, dp=None, use_graph=False, optimize=True, check=None):
    """`steps` deterministic native steps on one trainer; check(trainer) after each.  Returns (losses, parameters)."""
    from tests.test_gpu_train_parity import _OneRankDP
    cfgs = H.full_cfgs(*DIMS)
    Ps = [O.make_params(cfgs[i], 1 + i, scale=0.02) for i in range(4)]
    torch.manual_seed(4321)
    cfg_x, mgr = H.make_manager(cfgs, Ps, dropout=0.1, cc_weight=0.01)
    mgr.set_all_models_train()
    tr = cva.RetrievalTrainer(cfg_x, mgr)
    tr.lookahead_min_stage_bytes = 0
    _set_seg(cva, seg)
    tr.set_deterministic(True)
    if dp:
        tr.dp = _OneRankDP()
    losses = []
    try:
        for it in range(steps):
            b = batches[it % len(batches)]
            nxt = batches[(it + 1) % len(batches)] if lookahead and it + 1 < steps else None
            kw = {}
            if dp:
                b.global_max_synced = True
                if nxt is not None:
                    nxt.global_max_synced = True
                kw = dict(vid_counts=[int(b.clip_num.shape[0])], clip_counts=[int(b.clip_feat_len.shape[0])])
            if use_graph:
                kw["use_graph"] = True
            else:
                kw.update(seed=500 + it, next_batch=nxt, defer_join=defer)
            if not optimize:
                kw["do_optimizer"] = False
            out = tr.train_step_native(b, **kw)
            tr.join_streams()
            torch.cuda.synchronize()
            losses.append([float(v) for v in out])
            if check is not None:
                check(tr)
        return losses, [n._flat.detach().clone() for n in mgr.model_dict.values()]
    finally:
        tr.set_deterministic(False)
        _set_seg(cva, True)


def _shadow_is_zero(torch):
    def check(tr):
        assert tr.det_bypass_count() == 0
        sh = tr._det_shadow
        assert sh is not None and sh.numel() > 0
        nz = int(torch.count_nonzero(sh))
        assert nz == 0, f"{nz} bytes of the fixed-point shadow still hold a sum after the step"
    return check


@pytest.mark.parametrize("route", ["plain", "timed", "ragged", "no_update", "dp", "graph"])
def test_every_shadow_word_is_flushed_after_a_step(env, route):
    torch, cva = env
    batches = _batches(cva, ragged=route == "ragged")
    kw = dict(timed=dict(lookahead=True, defer=True), no_update=dict(optimize=False), dp=dict(dp=True), graph=dict(use_graph=True)).get(route, {})
    if route == "graph":
        batches = batches[:1]  # one shape: step 0 eager, step 1 captured, step 2 replayed
    zero, cached = _shadow_is_zero(torch), []

    def check(tr):
        zero(tr)
        cached.append(len(getattr(getattr(tr, "_native", None), "graphs", None) or {}))
    losses, params = _steps(torch, cva, batches, 3, check=check, **kw)
    for p in params:
        assert torch.isfinite(p).all()
    if route == "graph":
        assert cached[-1] == 1, cached  # (the last step replayed a captured one)


@pytest.mark.parametrize("ragged", [False, True])
def test_segment_flushes_compute_the_same_bits_as_whole_arena_flushes(env, ragged):
    torch, cva = env
    batches = _batches(cva, ragged)
    la, pa = _steps(torch, cva, batches, 3, seg=True)
    lb, pb = _steps(torch, cva, batches, 3, seg=False)
    assert la == lb, (la, lb)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    assert la[0][0] != la[-1][0]
