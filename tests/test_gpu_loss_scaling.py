"""Dynamic loss scaling of the native step (trainer_retrieval.LossScaler; include/coot_hip.h: coot_step_set_loss_scaler) — the
reference trains its fp16 path under torch.cuda.amp.GradScaler (coot/trainer_retrieval.py:264,277-285).

  * linearity: under a power-of-two scale the backward computes the same numbers times the scale, so three scaled steps must match
    three unscaled ones (deterministic mode; only the fixed-point rounding of the accumulated words moves);
  * the reference trajectories (tests/test_gpu_train_trajectory.py) hold through the scaled single, timed and one-rank data-parallel
    routes; the captured (graph) route computes what the eager scaled step computes;
  * a batch with a NaN feature skips the step: parameters and Adam moments bit-unchanged, scale backed off, the device step count
    unchanged — and clean steps around it are bit-identical to a run that never saw it;
  * the scale / growth-tracker schedule equals torch._amp_update_scale_ (what GradScaler.update calls) for the same found_inf sequence;
  * deterministic mode: a scaled fixed-point word that passes its range skips the step instead of reaching Adam as a finite wrong
    gradient; the device step count stays the trainer's when scaling is switched off and on, or a GradScaler state is loaded;
  * the IEEE-half build (COOT_OPERAND=f16, child process) trains under the scaler: gradients within the bf16 path's parity bounds,
    the trajectory within its bounds through the single and the one-rank data-parallel route; without a scaler its backward still
    refuses ("forward-only").  (The captured route is compared with the eager scaled step, in the bf16 build: it draws its own seeds,
    so it has no reference trajectory.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import coot_oracle as O
from tests import helpers as H
from tests import test_gpu_train_trajectory as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = dict(init_scale=2.0 ** 12, growth_factor=1.0, backoff_factor=1.0)  # a fixed power-of-two scale


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _numpy_batches(g):
    seed, B, Lv, Lc, Lp, Ls, dv, dt = [int(v) for v in g["meta"][:8]]
    return [O.make_batch(seed + 100 + s, B, g["counts"], Lv, Lc, Lp, Ls, dv, dt, ragged=bool(int(g["ragged"])), corr=0.5) for s in range(2)]


def _to_device(cva, g, b):
    bt = cva.synthetic.batch_from_numpy(b, packed=bool(int(g["train_packed"])) if "train_packed" in g else False)
    bt.global_max_synced = True
    return bt


def _step_kw(torch, g, s):
    idx = torch.from_numpy(np.concatenate([g["cc_idx"][s, 0], g["cc_idx"][s, 1]]).astype(np.int64)).cuda()
    return dict(seed=int(g["step_seeds"][s]), cc_indices=idx)


def _flat(mgr):
    return [mgr.model_dict[k]._flat.detach().cpu().numpy().copy() for k in H.NET_KEYS]


def _run(torch, cva, golden_dir, name, steps, scaler=None, deterministic=True, plan=None):
    """`steps` native steps on the fixture's two batches (plan: list of step indices into the fixture's seeds, or "nan" for a step on
    batch 0 with one NaN feature value).  Returns (losses, initial params, final params, trainer)."""
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, name)
    if deterministic:
        trainer.set_deterministic(True)
    if scaler is not None:
        trainer.enable_loss_scaling(**scaler)
    p0 = _flat(mgr)
    nb = None
    losses = []
    for s in (plan if plan is not None else range(steps)):
        if s == "nan":
            if nb is None:
                b = dict(_numpy_batches(g)[0])
                b["vid_feat"] = np.array(b["vid_feat"], copy=True)
                b["vid_feat"][0, 0, 0] = np.nan
                nb = _to_device(cva, g, b)
            out = trainer.train_step_native(nb, **_step_kw(torch, g, 0))
        else:
            out = trainer.train_step_native(batches[s & 1], **_step_kw(torch, g, s))
        losses.append([float(out[1]), float(out[2])])
    torch.cuda.synchronize()
    return np.array(losses), p0, _flat(mgr), trainer


@pytest.mark.parametrize("name", ["traj_small_eps", "traj_anet_eps"])
def test_scaled_steps_equal_unscaled_steps(env, golden_dir, name):
    torch, cva = env
    l0, p0, p_plain, tr = _run(torch, cva, golden_dir, name, 3)
    tr.close()
    l1, q0, p_scaled, tr = _run(torch, cva, golden_dir, name, 3, scaler=FIXED)
    assert tr.loss_scale() == 2.0 ** 12 and tr.skipped_steps() == 0
    assert tr.optimizer_state_dict()["native"]["step"] == 3
    tr.close()
    print(f"[{name}] losses unscaled {l0.tolist()} scaled {l1.tolist()}")
    assert np.allclose(l0, l1, rtol=1e-5, atol=1e-7), (l0, l1)
    assert np.array_equal(l0[0], l1[0])  # the first forward sees the same parameters: the loss words are not scaled
    cmin = 1.0
    for a0, a, b in zip(p0, p_plain, p_scaled):
        da, db = a.astype(np.float64) - a0, b.astype(np.float64) - a0
        c = H.cosine_flat(da, db)
        cmin = min(cmin, c)
        assert c >= 1 - 1e-6, c
        assert abs(np.linalg.norm(db) / np.linalg.norm(da) - 1) < 1e-4
    print(f"[{name}] min parameter-delta cosine scaled vs unscaled: {cmin:.9f}")


@pytest.mark.parametrize("route", ["single", "timed", "dp1"])
@pytest.mark.parametrize("name", ["traj_small_eps", "traj_anet_eps"])
def test_reference_trajectory_under_loss_scaling(env, golden_dir, name, route, monkeypatch):
    torch, cva = env
    made = []
    setup = T._setup

    def scaled_setup(*a, **k):
        out = setup(*a, **k)
        out[4].enable_loss_scaling(**FIXED)
        made.append(out[4])
        return out

    monkeypatch.setattr(T, "_setup", scaled_setup)
    T.test_k_optimizer_steps_vs_the_reference_trainer((torch, cva), golden_dir, name, route)
    tr = made[0]
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    assert tr.skipped_steps() == 0 and tr.loss_scale() == 2.0 ** 12
    assert tr.optimizer_state_dict()["native"]["step"] == int(g["steps"])


def test_graph_replay_under_loss_scaling(env, golden_dir):
    """The captured step (train_step_native(use_graph=True)) with a scaler computes what the eager scaled step computes."""
    torch, cva = env
    res = []
    for use_graph in (False, True):
        g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_small_eps")
        trainer.set_deterministic(True)
        trainer.enable_loss_scaling(init_scale=2.0 ** 10, growth_interval=2)
        p0 = _flat(mgr)
        torch.manual_seed(5)
        ls = [float(trainer.train_step_native(batches[s & 1], use_graph=use_graph)[1]) for s in range(5)]
        torch.cuda.synchronize()
        if use_graph:
            assert trainer._native.graphs, "the step was not captured"
        res.append((ls, p0, _flat(mgr), trainer.loss_scale(), trainer.optimizer_state_dict()["native"]["step"]))
        trainer.close()
    (le, p0, pe, se, ke), (lg, _, pg, sg, kg) = res
    assert ke == kg == 5 and se == sg == 2.0 ** 12, (ke, kg, se, sg)  # grown twice (growth_interval 2)
    assert np.allclose(le, lg, rtol=1e-6), (le, lg)
    for a0, a, b in zip(p0, pe, pg):
        assert H.cosine_flat(a.astype(np.float64) - a0, b.astype(np.float64) - a0) >= 1 - 1e-6


def test_non_finite_gradient_skips_the_step_and_backs_off(env, golden_dir):
    torch, cva = env
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_small_eps")
    trainer.enable_loss_scaling(init_scale=2.0 ** 12, growth_interval=1000)
    trainer.train_step_native(batches[0], **_step_kw(torch, g, 0))
    st = trainer._native
    torch.cuda.synchronize()
    before = (_flat(mgr), [t.cpu().numpy().copy() for t in st.m], [t.cpu().numpy().copy() for t in st.v])
    assert trainer.optimizer_state_dict()["native"]["step"] == 1
    b = dict(_numpy_batches(g)[0])
    b["vid_feat"] = np.array(b["vid_feat"], copy=True)
    b["vid_feat"][0, 0, 0] = np.nan
    trainer.train_step_native(_to_device(cva, g, b), **_step_kw(torch, g, 1))
    torch.cuda.synchronize()
    after = (_flat(mgr), [t.cpu().numpy() for t in st.m], [t.cpu().numpy() for t in st.v])
    for what, xs, ys in zip(("parameters", "first moments", "second moments"), before, after):
        for x, y in zip(xs, ys):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
    assert trainer.loss_scaler.found_inf()
    assert trainer.loss_scale() == 2.0 ** 11 and trainer.skipped_steps() == 1
    sd = trainer.optimizer_state_dict()
    assert sd["native"]["step"] == 1 and sd["loss_scaler"]["step"] == 1 and sd["loss_scaler"]["_growth_tracker"] == 0
    # the next clean step trains again
    trainer.train_step_native(batches[1], **_step_kw(torch, g, 1))
    torch.cuda.synchronize()
    assert not trainer.loss_scaler.found_inf() and trainer.optimizer_state_dict()["native"]["step"] == 2
    assert not np.array_equal(_flat(mgr)[0], before[0][0])
    trainer.close()


def _get_option(cva, name):
    import ctypes as C
    v = C.c_int(0)
    assert cva.lib.load().coot_get_option(name.encode(), C.byref(v)) == 0
    return v.value


def test_fixed_point_word_past_its_range_skips_the_step(env, golden_dir):
    """Deterministic mode keeps accumulated gradient words (biases, LayerNorm vectors) as 64-bit fixed-point sums with a range of
    +-2^23; a scaled word can pass it.  The scale here is chosen from the unscaled gradients so that the largest accumulated word is
    ~2^25 in scaled units (its addends, partial sums of workgroups, stay below the 2^22 bypass).  The wrapped sum must not reach Adam
    as a finite wrong gradient: the word becomes NaN, the step is skipped and the scale backs off."""
    torch, cva = env
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_anet_eps")
    trainer.set_deterministic(True)
    trainer.enable_loss_scaling(init_scale=1.0, growth_factor=1.0, backoff_factor=0.5)
    trainer.train_step_native(batches[0], do_optimizer=False, **_step_kw(torch, g, 0))
    torch.cuda.synchronize()
    assert not trainer.loss_scaler.found_inf() and _get_option(cva, "det_overflow_check") == 1
    gmax = 0.0
    for k in H.NET_KEYS:
        net = mgr.model_dict[k]
        flat = net._grad_flat.detach().cpu().numpy()
        for (pname, off, shape) in net.table:
            if len(shape) == 1:  # the accumulated words
                gmax = max(gmax, float(np.abs(flat[off:off + int(np.prod(shape))]).max()))
    scale = 2.0 ** round(np.log2(2.0 ** 25 / gmax))
    print(f"largest accumulated gradient word {gmax:.3e}: scale {scale:.3e}")
    trainer.train_step_native(batches[0], **_step_kw(torch, g, 0))  # one clean step: moments exist
    trainer.enable_loss_scaling(init_scale=scale, growth_factor=1.0, backoff_factor=0.5)
    st = trainer._native
    torch.cuda.synchronize()
    before = (_flat(mgr), [t.cpu().numpy().copy() for t in st.m], [t.cpu().numpy().copy() for t in st.v])
    wraps = _get_option(cva, "det_overflows")
    trainer.train_step_native(batches[1], **_step_kw(torch, g, 1))
    torch.cuda.synchronize()
    assert _get_option(cva, "det_overflows") > wraps, "no fixed-point word wrapped: the case is not exercised"
    assert trainer.loss_scaler.found_inf() and trainer.skipped_steps() == 1 and trainer.loss_scale() == scale / 2
    assert trainer.optimizer_state_dict()["native"]["step"] == 1
    after = (_flat(mgr), [t.cpu().numpy() for t in st.m], [t.cpu().numpy() for t in st.v])
    for xs, ys in zip(before, after):
        for x, y in zip(xs, ys):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    trainer.close()
    assert _get_option(cva, "det_overflow_check") == 0


def test_device_step_count_follows_the_trainer(env, golden_dir):
    """Adam's step count stays the trainer's when scaling is switched off and on again, and when a GradScaler state (no step) is loaded."""
    torch, cva = env
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_small_eps")
    sc = trainer.enable_loss_scaling(**FIXED)
    for s in range(2):
        trainer.train_step_native(batches[s & 1], **_step_kw(torch, g, s))
    assert sc.state_dict()["step"] == 2
    trainer.disable_loss_scaling()
    trainer.train_step_native(batches[0], **_step_kw(torch, g, 2))
    assert trainer.optimizer_state_dict()["native"]["step"] == 3
    trainer.enable_loss_scaling(sc)
    assert sc.state_dict()["step"] == 3
    trainer.train_step_native(batches[1], **_step_kw(torch, g, 3))
    assert sc.state_dict()["step"] == 4
    sc.load_state_dict({"scale": 256.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 10, "_growth_tracker": 0})
    assert sc.state_dict()["step"] == 4 and sc.get_scale() == 256.0
    assert trainer.optimizer_state_dict()["native"]["step"] == 4
    trainer.close()


def test_skipped_step_leaves_a_deterministic_run_bit_identical(env, golden_dir):
    # (the benchmark-shape fixture: at traj_small_eps' shapes two unscaled deterministic runs already differ in the last bits of the
    # input-FC / input-LayerNorm gradients, with or without a scaler)
    torch, cva = env
    _, _, clean, tr = _run(torch, cva, golden_dir, "traj_anet_eps", 3, scaler=FIXED, plan=[0, 1, 2])
    tr.close()
    _, _, mixed, tr = _run(torch, cva, golden_dir, "traj_anet_eps", 4, scaler=FIXED, plan=[0, "nan", 1, 2])
    assert tr.skipped_steps() == 1 and tr.optimizer_state_dict()["native"]["step"] == 3
    tr.close()
    for a, b in zip(clean, mixed):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_scale_schedule_matches_torch_amp_update_scale(env, golden_dir):
    torch, cva = env
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_small_eps")
    trainer.enable_loss_scaling(init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    b = dict(_numpy_batches(g)[0])
    b["vid_feat"] = np.array(b["vid_feat"], copy=True)
    b["vid_feat"][0, 0, 0] = np.nan
    bad = _to_device(cva, g, b)
    scale = torch.full((1,), 2.0 ** 10, dtype=torch.float32, device="cuda")
    tracker = torch.zeros(1, dtype=torch.int32, device="cuda")
    seq = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0]
    steps = 0
    for i, nan in enumerate(seq):
        trainer.train_step_native(bad if nan else batches[i & 1], **_step_kw(torch, g, i % int(g["steps"])))
        torch._amp_update_scale_(scale, tracker, torch.full((1,), float(nan), device="cuda"), 2.0, 0.5, 2)
        steps += 1 - nan
        sd = trainer.loss_scaler.state_dict()
        want = (float(scale.item()), int(tracker.item()))
        print(f"step {i} found_inf {nan}: device scale {sd['scale']} tracker {sd['_growth_tracker']}  torch {want}")
        assert (sd["scale"], sd["_growth_tracker"]) == want
        assert sd["step"] == steps and sd["skipped_steps"] == sum(seq[:i + 1])
    trainer.close()


CHILD = r'''
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.environ["COOT_ROOT"])
import coot_videotext_amd as cva
from tests import helpers as H
from tests.test_gpu_train_parity import _case, GRAD_COS_MIN, GRAD_NORM_TOL
from tests import test_gpu_train_trajectory as T
golden = os.path.join(os.environ["COOT_ROOT"], "tests", "golden")
out = {"operand": cva.lib.operand()}
name = "bench_yc2_2d3d_2816_train"
g, cfgs, Ps, b = _case(golden, name)
p, seed = float(g["train_p"]), int(g["train_step_seed"])
cfg, mgr = H.make_manager(cfgs, Ps, dropout=p, cc_weight=float(g["cc_weight"]))
mgr.set_all_models_train()
trainer = cva.RetrievalTrainer(cfg, mgr)
batch = cva.synthetic.batch_from_numpy(b, packed=bool(int(g["train_packed"])))
idx = torch.from_numpy(np.concatenate([g["cc_idx_clip"], g["cc_idx_sent"]]).astype(np.int64)).cuda()
# unscaled: still refused
try:
    trainer.train_step_native(batch, do_optimizer=False, seed=seed, cc_indices=idx)
    out["unscaled_refused"] = False
except RuntimeError as e:
    out["unscaled_refused"] = "forward-only" in str(e)
# scaled: GradScaler's default scale first, halved while the half-precision backward overflows (what GradScaler's skipped steps do)
tried = []
for s in (2.0 ** 16, 2.0 ** 14, 2.0 ** 12, 2.0 ** 10):
    trainer.enable_loss_scaling(init_scale=s)
    losses = trainer.train_step_native(batch, do_optimizer=False, seed=seed, cc_indices=idx)
    torch.cuda.synchronize()
    tried.append((s, trainer.loss_scaler.found_inf()))
    if not tried[-1][1]:
        break
out["tried"] = tried
out["losses"] = [float(v) for v in losses]
out["ref_losses"] = [float(g["contr_loss"]), float(g["cc_loss"])]
step = int(g["sub_step"])
gmax = max(float(g[k]) for k in g if k.startswith("gnorm:"))
bad, checked, cmin, nmax = [], 0, 1.0, 0.0
for k in H.NET_KEYS:
    net = mgr.model_dict[k]
    flat = net._grad_flat.detach().cpu().numpy()
    for (pname, off, shape) in net.table:
        got = flat[off:off + int(np.prod(shape))]
        key = f"{k}:{pname}"
        gn = float(g["gnorm:" + key])
        if gn < 1e-6 * gmax:
            if np.linalg.norm(got) > 1e-3 * gmax:
                bad.append((key, "zero-grad", float(np.linalg.norm(got))))
            continue
        ref = g["gsub:" + key]
        c = H.cosine_flat(got[::(1 if ref.size == got.size else step)], ref)
        nr = float(np.linalg.norm(got.astype(np.float64))) / gn
        checked += 1
        cmin, nmax = min(cmin, c), max(nmax, abs(nr - 1))
        if not (c > GRAD_COS_MIN and abs(nr - 1) < GRAD_NORM_TOL):
            bad.append((key, round(c, 4), round(nr, 4)))
out["grad"] = {"checked": checked, "min_cos": cmin, "worst_norm": nmax, "bad": bad}
trainer.close()
# a few full optimizer steps of the reference trajectory
setup = T._setup
def scaled_setup(*a, **k):
    r = setup(*a, **k)
    r[4].enable_loss_scaling(init_scale=2.0 ** 12, growth_factor=1.0, backoff_factor=1.0)
    out["traj_trainer"] = True
    return r
T._setup = scaled_setup
T.test_k_optimizer_steps_vs_the_reference_trainer((torch, cva), golden, "traj_small_eps", "single")
out["traj_ok"] = True
# ... and through the one-rank data-parallel phase calls (coot_step_forward / _backward / _update)
T.test_k_optimizer_steps_vs_the_reference_trainer((torch, cva), golden, "traj_small_eps", "dp1")
out["traj_dp1_ok"] = True
print("RESULT " + json.dumps(out))
'''


def test_f16_build_trains_under_loss_scaling():
    env_ = dict(os.environ, COOT_OPERAND="f16", COOT_ROOT=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env_, capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    print(r.stdout[-4000:])
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    out = json.loads(line[-1][7:])
    assert out["operand"] == "f16"
    assert out["unscaled_refused"]
    assert not out["tried"][-1][1], out["tried"]
    contr, cc = out["losses"][1], out["losses"][2]
    rc, rcc = out["ref_losses"]
    assert abs(contr - rc) < 2e-3 * abs(rc) and abs(cc - rcc) < 5e-3 * abs(rcc) + 1e-6, (out["losses"], out["ref_losses"])
    assert not out["grad"]["bad"] and out["grad"]["checked"] >= 100, out["grad"]
    assert out["traj_ok"] and out["traj_dp1_ok"]
