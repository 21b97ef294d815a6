"""Text side ahead (include/coot_hip.h: COOT_STEP_TEXT_AHEAD; csrc/api_step.hip: the fork of coot_train_step).

Back-to-back native steps (next_batch + defer_join, no join between them) start their text side behind the text stream's own tail
instead of behind the caller's stream, i.e. without waiting for the video side's update of the previous step.  That removes an
ordering edge, so what has to hold is: the same bits as the plain run (no lookahead, no defer, joined after every step) in
deterministic mode — a race on any buffer the text forward shares with the previous step's tail would show as other bits or as
non-finite values — and the counter `text_ahead_steps` moves on exactly the steps that qualify.

Shapes: those of tests/test_gpu_determinism.py (bit identity of the timed mode's re-orderings is established there), and one lopsided
shape whose text side finishes its tail long before the video side (the text forward then really runs under the video update).
"""
import ctypes as C

import pytest

from oracle import coot_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DIMS = (256, 192, 384, 8, 384, 768)
LOPSIDED = (2048, 192, 384, 8, 384, 768)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _params(dims):
    cfgs = H.full_cfgs(*dims)
    return cfgs, [O.make_params(cfgs[i], 1 + i, scale=0.02) for i in range(4)]


def _batches(cva):
    return [cva.synthetic.make_batch(40 + i, 12, 4, 40, 40, 32, 16, DIMS[0], DIMS[1], ragged=False) for i in range(3)]


def _run(torch, cva, cfgs, Ps, batches, steps, timed, script=None, wrap=False):
    """`steps` deterministic optimizer steps on batches[it % n].  timed: lookahead + deferred join and NO join between the steps (one
    join + synchronise at the end); else the plain run, joined after every step.  script[it] = set of events in front of / at step it:
      "dirty"      mgr.mark_weights_dirty() before the step (both runs: the step then packs at its head)
      "unannounced" the step before announces ANOTHER batch than the one this step gets
      "join"       join_streams() before the step
      "no_defer"   the step runs with defer_join=False
    wrap: the last step announces a next batch too (else it has none, and its gradient zero fill runs on the text stream).
    Returns (losses [steps, 3] on the host, the four parameter arenas, the increment of `text_ahead_steps` over every step)."""
    script = script or {}
    cfg_x, mgr = H.make_manager(cfgs, Ps, dropout=0.1, cc_weight=0.01)
    mgr.set_all_models_train()
    tr = cva.RetrievalTrainer(cfg_x, mgr)
    tr.lookahead_min_stage_bytes = 0
    tr.set_deterministic(True)
    n = len(batches)
    losses, took = [], []
    try:
        for it in range(steps):
            ev = script.get(it, ())
            if "dirty" in ev:
                mgr.mark_weights_dirty()  # (a flag on the host: no parameter is touched, so no join is due)
            if timed and "join" in ev:
                tr.join_streams()
            before = cva.lib.get_option("text_ahead_steps")
            if timed:
                nxt = None
                if it + 1 < steps or wrap:
                    nxt = batches[(it + 2) % n] if "unannounced" in script.get(it + 1, ()) else batches[(it + 1) % n]
                out = tr.train_step_native(batches[it % n], seed=500 + it, next_batch=nxt, defer_join="no_defer" not in ev)
            else:
                out = tr.train_step_native(batches[it % n], seed=500 + it)
                tr.join_streams()
            took.append(cva.lib.get_option("text_ahead_steps") - before)
            losses.append(torch.stack([v.detach() for v in out]).clone())  # (device side: no host synchronisation between the steps)
        tr.join_streams()
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), [m._flat.detach().clone() for m in mgr.model_dict.values()], took
    finally:
        tr.set_deterministic(False)


def _same(torch, a, b):
    la, pa, _ = a
    lb, pb, _ = b
    assert torch.isfinite(la).all() and float(la[0, 0]) != float(la[-1, 0])
    assert torch.equal(la, lb), (la, lb)
    assert len(pa) == 4 and all(torch.equal(x, y) for x, y in zip(pa, pb))


@pytest.fixture(scope="module")
def plain6(env):
    torch, cva = env
    cfgs, Ps = _params(DIMS)
    batches = _batches(cva)
    return cfgs, Ps, batches, _run(torch, cva, cfgs, Ps, batches, 6, timed=False)


def test_back_to_back_steps_start_the_text_side_ahead_with_the_same_bits(env, plain6):
    torch, cva = env
    cfgs, Ps, batches, plain = plain6
    assert plain[2] == [0] * 6
    timed = _run(torch, cva, cfgs, Ps, batches, 6, timed=True)
    _same(torch, plain, timed)
    assert timed[2] == [0, 1, 1, 1, 1, 1], timed[2]  # the first step finds no prepared stage; the last one announces no batch and still qualifies


def test_switch_off_keeps_the_fork_on_the_callers_stream(env, plain6):
    torch, cva = env
    cfgs, Ps, batches, plain = plain6
    lib = cva.lib.load()
    cva.lib.check(lib.coot_set_option(b"text_ahead", 0), "coot_set_option")
    try:
        timed = _run(torch, cva, cfgs, Ps, batches, 6, timed=True)
    finally:
        cva.lib.check(lib.coot_set_option(b"text_ahead", 1), "coot_set_option")
    _same(torch, plain, timed)
    assert timed[2] == [0] * 6


def test_fallbacks_miss_exactly_their_steps(env):
    torch, cva = env
    cfgs, Ps = _params(DIMS)
    batches = _batches(cva)
    script = {2: {"dirty"}, 4: {"unannounced"}, 6: {"join"}, 8: {"no_defer"}}
    plain = _run(torch, cva, cfgs, Ps, batches, 11, timed=False, script=script)
    timed = _run(torch, cva, cfgs, Ps, batches, 11, timed=True, script=script)
    _same(torch, plain, timed)
    # 0: nothing prepared; 2: packs at its head; 4: not the announced batch; 6: joined; 8: runs joined itself; 9: the step before it was
    assert timed[2] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1], timed[2]


def test_lopsided_shape_text_tail_finishes_first(env):
    """Video: 32 videos x 4 clips, 80 frames of 2048 features; text: 16 / 8 tokens of 192 — the text side's update is done long before
    the video side's, so the next text forward runs under the video side's backward and update."""
    torch, cva = env
    cfgs, Ps = _params(LOPSIDED)
    batches = [cva.synthetic.make_batch(60 + i, 32, 4, 80, 80, 16, 8, LOPSIDED[0], LOPSIDED[1], ragged=False) for i in range(2)]
    plain = _run(torch, cva, cfgs, Ps, batches, 4, timed=False)
    timed = _run(torch, cva, cfgs, Ps, batches, 4, timed=True, wrap=True)
    _same(torch, plain, timed)
    assert timed[2] == [0, 1, 1, 1], timed[2]


def test_stamp_of_the_text_forward(env):
    torch, cva = env
    cfgs, Ps = _params(DIMS)
    batches = _batches(cva)
    lib = cva.lib.load()
    cfg_x, mgr = H.make_manager(cfgs, Ps, dropout=0.1, cc_weight=0.01)
    mgr.set_all_models_train()
    tr = cva.RetrievalTrainer(cfg_x, mgr)
    tr.lookahead_min_stage_bytes = 0
    before = cva.lib.get_option("text_ahead_steps")
    tr.train_step_native(batches[0], seed=1, next_batch=batches[1], defer_join=True)
    cva.lib.check(lib.coot_set_option(b"step_stamps", 1), "coot_set_option")
    try:
        tr.train_step_native(batches[1], seed=2, next_batch=batches[2], defer_join=True)
        buf = C.create_string_buffer(8192)
        assert lib.coot_debug_step_stamps(buf, 8192) > 0
    finally:
        cva.lib.check(lib.coot_set_option(b"step_stamps", 0), "coot_set_option")
    tr.join_streams()
    torch.cuda.synchronize()
    assert cva.lib.get_option("text_ahead_steps") == before + 1
    rows = [r.strip() for r in buf.value.decode().splitlines()]
    labels = [r.split(" us ", 1)[1].strip() for r in rows]
    assert "text: forward starts" in labels, rows
    assert labels.index("text: forward starts") < labels.index("text: local forward done")
