"""Gradient norm and clipping of the training step (trainer_retrieval.GradClip; include/coot_hip.h: coot_step_set_grad_clip) — the
reference's train.clip_gradient (nntrainer/trainer_base.py:545-554: torch.nn.utils.clip_grad_norm_ over all parameters).

  * the reported norm is the float64 norm of the four gradient arenas, on every route (single, timed, graph, one-rank data parallel,
    under a loss scaler: the unscaled gradients);
  * report-only (the reference's behaviour) changes no parameter, moment or loss bit; clipping with an unreachable max_norm neither;
  * clipping before the update equals the phase calls without a clipper with torch's clip_grad_norm_ between backward and update;
  * the reference's step body with clip_grad_norm_ before opt.step() (tools/gen_golden_clip.py) is reproduced through the single,
    timed and one-rank data-parallel routes, per-step norms included; the same run without clipping falls outside those bounds;
  * loss scaler + clipping: scaled clipped steps equal unscaled clipped steps, a NaN gradient skips the step, the IEEE-half build
    trains with both; two deterministic runs give the same bits; two real ranks report the same norm bits.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_train_trajectory as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = dict(init_scale=2.0 ** 12, growth_factor=1.0, backoff_factor=1.0)
# per-step norm vs the reference (relative), the default build's bf16 operands: measured on MI355X at most 2.0e-3 (traj_small_clip_eps)
# and 5.2e-4 (traj_anet_clip_eps) on every route
NORM_TOL = {"bf16": 5e-3}
# bit-identity needs a problem whose deterministic runs repeat bit for bit: at traj_small_eps' shapes two plain deterministic runs
# already differ in the last bits of the input-FC / input-LayerNorm gradients (tests/test_gpu_loss_scaling.py), at the benchmark's not
BITS = "traj_anet_eps"


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _kw(torch, g, s, route, batches, B, Nc, steps):
    idx = torch.from_numpy(np.concatenate([g["cc_idx"][s, 0], g["cc_idx"][s, 1]]).astype(np.int64)).cuda()
    kw = dict(seed=int(g["step_seeds"][s]), cc_indices=idx)
    if route == "dp1":
        kw.update(vid_counts=[B], clip_counts=[Nc])
    if route == "timed":
        kw.update(defer_join=True, next_batch=batches[(s + 1) & 1] if s + 1 < steps else None)
    if route == "graph":
        kw = dict(use_graph=True)
    return kw


def _arena_norm(mgr):
    return float(np.sqrt(sum(float(np.sum(n._grad_flat.detach().cpu().numpy().astype(np.float64) ** 2)) for n in mgr.model_dict.values())))


def _run(torch, cva, golden_dir, name, steps, route="single", clip=None, scaler=None, deterministic=True, plan=None, check_norm=False):
    """`steps` steps of the fixture's problem on `route`; clip: GradClip kwargs or None.  Returns a dict of losses, parameters,
    moments, per-step reported norms (and the float64 arena norms when check_norm)."""
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, name)
    if deterministic:
        trainer.set_deterministic(True)
    if route == "dp1":
        trainer.dp = T._OneRankDP()
    if route == "timed":
        trainer.lookahead_min_stage_bytes = 0
    if scaler is not None:
        trainer.enable_loss_scaling(**scaler)
    if clip is not None:
        trainer.enable_grad_clipping(max_norm=clip["max_norm"], before_update=clip.get("before_update", False))
    B, Nc = int(batches[0].clip_num.shape[0]), int(batches[0].clip_feat_len.shape[0])
    out = dict(losses=[], norms=[], arena=[], coef=[])
    p0 = [mgr.model_dict[k]._flat.detach().cpu().numpy().astype(np.float64) for k in H.NET_KEYS]
    nb = None
    for s in (plan if plan is not None else range(steps)):
        if s == "nan":
            if nb is None:
                from tests import test_gpu_loss_scaling as LS
                b = dict(LS._numpy_batches(g)[0])
                b["vid_feat"] = np.array(b["vid_feat"], copy=True)
                b["vid_feat"][0, 0, 0] = np.nan
                nb = LS._to_device(cva, g, b)
            res = trainer.train_step_native(nb, **_kw(torch, g, 0, "single", batches, B, Nc, steps))
        else:
            res = trainer.train_step_native(batches[s & 1], **_kw(torch, g, s, route, batches, B, Nc, steps))
        trainer.join_streams()
        torch.cuda.synchronize()
        out["losses"].append([float(res[1]), float(res[2])])
        if clip is not None:
            out["norms"].append(trainer.last_grad_norm())
            out["coef"].append(trainer.grad_clip.coef())
        if check_norm:
            out["arena"].append(_arena_norm(mgr))
    torch.cuda.synchronize()
    st = trainer._native
    out["p"] = [mgr.model_dict[k]._flat.detach().cpu().numpy().copy() for k in H.NET_KEYS]
    out["m"] = [t.detach().cpu().numpy().copy() for t in st.m]
    out["v"] = [t.detach().cpu().numpy().copy() for t in st.v]
    out["p0"] = p0
    out["losses"] = np.array(out["losses"])
    out["trainer"] = trainer
    return out


def _same(a, b, keys=("p", "m", "v")):
    for k in keys:
        for x, y in zip(a[k], b[k]):
            if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                return False
    return np.array_equal(a["losses"], b["losses"])


# ---- 1. the reported norm is the norm of the arenas ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["report", "before"])
@pytest.mark.parametrize("route", ["single", "timed", "graph", "dp1", "scaler"])
def test_reported_norm_is_the_arena_norm(env, golden_dir, route, mode):
    torch, cva = env
    r = _run(torch, cva, golden_dir, "traj_small_eps", 4, route="single" if route == "scaler" else route, deterministic=False,
             clip=dict(max_norm=0.3, before_update=mode == "before"), scaler=FIXED if route == "scaler" else None, check_norm=True)
    got, want = np.array(r["norms"]), np.array(r["arena"])
    print(f"[{route}/{mode}] norms {got.tolist()} arenas {want.tolist()}")
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    assert np.all(np.abs(got - want) <= 1e-6 * want), (got, want)
    coef = np.array(r["coef"])
    assert np.allclose(coef, np.minimum(0.3 / (got + 1e-6), 1.0), rtol=1e-6)
    r["trainer"].close()


# ---- 2./3./7. bit-identity: report-only, an unreachable max_norm, two runs -------------------------------------------------------
@pytest.mark.parametrize("route", ["single", "timed", "graph", "dp1"])
def test_report_only_changes_nothing(env, golden_dir, route):
    torch, cva = env
    a = _run(torch, cva, golden_dir, BITS, 3, route=route)
    a["trainer"].close()
    b = _run(torch, cva, golden_dir, BITS, 3, route=route, clip=dict(max_norm=0.3))
    assert b["trainer"].grad_clip.clipped_steps() == 3  # (the reference would have logged "Clipping gradient" each time)
    b["trainer"].close()
    assert _same(a, b), route


def test_unreachable_max_norm_and_determinism(env, golden_dir):
    torch, cva = env
    a = _run(torch, cva, golden_dir, BITS, 3)
    a["trainer"].close()
    b = _run(torch, cva, golden_dir, BITS, 3, clip=dict(max_norm=1e30, before_update=True))
    assert b["trainer"].grad_clip.clipped_steps() == 0 and b["coef"] == [1.0] * 3
    b["trainer"].close()
    assert _same(a, b)
    c = _run(torch, cva, golden_dir, BITS, 3, clip=dict(max_norm=0.3, before_update=True))
    c["trainer"].close()
    d = _run(torch, cva, golden_dir, BITS, 3, clip=dict(max_norm=0.3, before_update=True))
    d["trainer"].close()
    assert _same(c, d) and np.array(c["norms"]).view(np.uint64).tolist() == np.array(d["norms"]).view(np.uint64).tolist()
    assert not _same(a, c)  # (and clipping does move something)


# ---- 4. fused clip == phase calls + torch clip_grad_norm_ ---------------------------------------------------------------------
class _ClipBetweenPhases(T._OneRankDP):
    """One-rank data parallel whose last gradient 'all-reduce' of a step (the video local bucket, on the main stream, right in front of
    coot_step_update) runs torch.nn.utils.clip_grad_norm_ over the four arenas: coot_step_backward -> clip_grad_norm_ ->
    coot_step_update, with no clipper bound in the library."""

    def __init__(self, trainer, max_norm):
        self.trainer, self.max_norm, self.calls, self.norms = trainer, max_norm, 0, []

    def all_reduce_sum(self, t):
        import torch
        self.calls += 1
        if self.calls % 3:
            return
        st = self.trainer._native
        torch.cuda.current_stream().wait_stream(st.comm)
        arenas = [n._grad_flat for n in st.nets]
        ps = []
        for a in arenas:
            p = torch.nn.Parameter(torch.empty_like(a))
            p.grad = a  # (the arena itself: clip_grad_norm_ scales it in place)
            ps.append(p)
        self.norms.append(float(torch.nn.utils.clip_grad_norm_(ps, self.max_norm)))


def test_fused_clip_matches_torch_between_the_phases(env, golden_dir):
    torch, cva = env
    g = dict(np.load(os.path.join(golden_dir, "traj_small_clip_eps.npz")))
    mn = float(g["clip_max_norm"])
    fused = _run(torch, cva, golden_dir, "traj_small_eps", 4, route="dp1", clip=dict(max_norm=mn, before_update=True))
    assert all(c < 1.0 for c in fused["coef"]) and fused["trainer"].grad_clip.clipped_steps() == 4
    fused["trainer"].close()
    made = {}
    setup = T._setup

    def hooked(*a, **k):
        out = setup(*a, **k)
        made["t"] = out[4]
        return out
    T._setup = hooked
    try:
        g_, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_small_eps")
    finally:
        T._setup = setup
    trainer.set_deterministic(True)
    trainer.dp = _ClipBetweenPhases(trainer, mn)
    B, Nc = int(batches[0].clip_num.shape[0]), int(batches[0].clip_feat_len.shape[0])
    for s in range(4):
        trainer.train_step_native(batches[s & 1], **_kw(torch, g_, s, "dp1", batches, B, Nc, 4))
    torch.cuda.synchronize()
    comp = [mgr.model_dict[k]._flat.detach().cpu().numpy() for k in H.NET_KEYS]
    print(f"norms fused {fused['norms']} torch {trainer.dp.norms}")
    assert np.allclose(fused["norms"], trainer.dp.norms, rtol=1e-6)
    for a, b in zip(fused["p"], comp):
        err = float(np.linalg.norm(a.astype(np.float64) - b)) / float(np.linalg.norm(b.astype(np.float64)))
        print(f"parameter arena relative error fused vs composed: {err:.3e}")
        assert err <= 1e-6, err
    trainer.close()


# ---- 5. the reference's clipped trajectories ---------------------------------------------------------------------------------
CLIP_CASES = {"traj_small_clip_eps": T.CASES["traj_small_eps"], "traj_anet_clip_eps": T.CASES["traj_anet_eps"]}


def _traj(torch, cva, golden_dir, name, route, monkeypatch, clip=True):
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    norms = []
    setup = T._setup

    def clip_setup(*a, **k):
        out = setup(*a, **k)
        tr = out[4]
        if clip:
            tr.enable_grad_clipping(max_norm=float(g["clip_max_norm"]), before_update=True)
        step = tr.train_step_native

        def stepped(*a_, **k_):
            res = step(*a_, **k_)
            if clip:
                norms.append(tr.last_grad_norm())
            return res
        tr.train_step_native = stepped
        return out
    monkeypatch.setattr(T, "_setup", clip_setup)
    monkeypatch.setitem(T.CASES, name, CLIP_CASES[name])
    T.test_k_optimizer_steps_vs_the_reference_trainer((torch, cva), golden_dir, name, route)
    return np.array(norms), g


@pytest.mark.parametrize("route", ["single", "timed", "dp1"])
@pytest.mark.parametrize("name", list(CLIP_CASES))
def test_reference_trajectory_with_clipping(env, golden_dir, name, route, monkeypatch):
    torch, cva = env
    norms, g = _traj(torch, cva, golden_dir, name, route, monkeypatch)
    rel = np.abs(norms - g["grad_norm"]) / g["grad_norm"]
    print(f"[{name}/{route}] norms {norms.tolist()} reference {g['grad_norm'].tolist()} worst relative error {rel.max():.3e}")
    assert len(norms) == int(g["steps"]) and np.all(rel <= NORM_TOL["bf16"]), rel


def test_per_op_route_reports_the_arena_norm(env, golden_dir):
    """The autograd route (train_step): torch's clip_grad_norm_ arithmetic over the flat arenas, stored in the same block."""
    torch, cva = env
    g, cfgs, Ps, mgr, trainer, batches = T._setup(torch, cva, golden_dir, "traj_small_eps")
    gc = trainer.enable_grad_clipping(max_norm=0.3)
    for s in range(2):
        trainer.train_step(batches[s & 1])
        got, want = trainer.last_grad_norm(), _arena_norm(mgr)
        assert abs(got - want) <= 1e-6 * want, (got, want)
        assert abs(gc.coef() - min(0.3 / (got + 1e-6), 1.0)) <= 1e-6
    assert gc.clipped_steps() == 2
    trainer.close()


@pytest.mark.parametrize("name", list(CLIP_CASES))
def test_power_unclipped_run_fails_the_clipped_reference(env, golden_dir, name, monkeypatch):
    torch, cva = env
    with pytest.raises(AssertionError):
        _traj(torch, cva, golden_dir, name, "single", monkeypatch, clip=False)


# ---- 6. loss scaler + clipping ---------------------------------------------------------------------------------------------------
def test_scaled_clipped_steps_equal_unscaled_clipped_steps(env, golden_dir):
    torch, cva = env
    clip = dict(max_norm=0.3, before_update=True)
    a = _run(torch, cva, golden_dir, "traj_small_eps", 3, clip=clip)
    a["trainer"].close()
    b = _run(torch, cva, golden_dir, "traj_small_eps", 3, clip=clip, scaler=FIXED)
    b["trainer"].close()
    assert np.allclose(a["norms"], b["norms"], rtol=1e-5), (a["norms"], b["norms"])
    assert np.allclose(a["losses"], b["losses"], rtol=1e-5, atol=1e-7)
    for p0, x, y in zip(a["p0"], a["p"], b["p"]):
        dx, dy = x.astype(np.float64) - p0, y.astype(np.float64) - p0
        assert H.cosine_flat(dx, dy) >= 1 - 1e-6 and abs(np.linalg.norm(dy) / np.linalg.norm(dx) - 1) < 1e-4


def test_nan_gradient_skips_the_clipped_step(env, golden_dir):
    torch, cva = env
    clip = dict(max_norm=0.3, before_update=True)
    a = _run(torch, cva, golden_dir, BITS, 0, clip=clip, scaler=FIXED, plan=[0, "nan", 1])
    assert a["trainer"].skipped_steps() == 1
    assert not np.isfinite(a["norms"][1]) and np.isfinite(a["norms"][0]) and np.isfinite(a["norms"][2])
    a["trainer"].close()
    b = _run(torch, cva, golden_dir, BITS, 0, clip=clip, scaler=FIXED, plan=[0, 1])
    b["trainer"].close()
    assert a["norms"][0] == b["norms"][0] and a["norms"][2] == b["norms"][1]
    for k in ("p", "m", "v"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.environ["COOT_ROOT"])
import numpy as np, torch
import coot_videotext_amd as cva
from tests import test_gpu_grad_clip as C
out = {"operand": cva.lib.OPERAND_ENV}
golden = os.path.join(os.environ["COOT_ROOT"], "tests", "golden")
r = C._run(torch, cva, golden, "traj_small_eps", 3, deterministic=False, clip=dict(max_norm=0.3, before_update=True), scaler=C.FIXED,
           check_norm=True)
out["norms"], out["arena"], out["coef"] = r["norms"], r["arena"], r["coef"]
out["moved"] = [float(np.linalg.norm(p.astype(np.float64) - p0)) for p, p0 in zip(r["p"], r["p0"])]
out["finite"] = all(bool(np.all(np.isfinite(p))) for p in r["p"])
print("RESULT " + json.dumps(out))
'''


def test_f16_build_trains_with_scaler_and_clipping():
    env_ = dict(os.environ, COOT_OPERAND="f16", COOT_ROOT=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env_, capture_output=True, text=True, timeout=900, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    print(r.stdout[-3000:])
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    out = json.loads(line[-1][7:])
    assert out["operand"] == "f16" and out["finite"]
    assert all(m > 0 for m in out["moved"])
    got, want = np.array(out["norms"]), np.array(out["arena"])
    assert np.all(np.abs(got - want) <= 1e-6 * want), (got, want)
    assert all(c < 1.0 for c in out["coef"])


# ---- 8. two real ranks -------------------------------------------------------------------------------------------------------
def test_two_ranks_report_identical_norms(tmp_path):
    import socket
    import torch
    import coot_videotext_amd as cva
    from oracle import coot_oracle as O
    from tests import dp_worker as W
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    world, seed, cc_weight = 2, 29, 0.01
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_clip_worker.py"), str(r), str(world), str(port), outs[r],
                               str(seed), str(cc_weight)], cwd=ROOT) for r in range(world)]
    try:
        rcs = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world, rcs
    res = [dict(np.load(o)) for o in outs]
    assert np.array_equal(res[0]["norms"].view(np.uint32), res[1]["norms"].view(np.uint32))
    for i in range(4):
        assert np.array_equal(res[0][f"p{i}"], res[1][f"p{i}"])
    # the single-process norm of the union batch (before any update: the first step's gradients)
    b, counts, idx_c, idx_s, vid_counts, clip_counts, _ = W.problem(seed, world)
    cfgs = H.full_cfgs(*W.DIMS)
    Ps = [O.make_params(cfgs[i], 1 + i, scale=0.02) for i in range(4)]
    cfg, mgr = H.make_manager(cfgs, Ps, dropout=0.0, cc_weight=cc_weight)
    mgr.set_all_models_train()
    tr = cva.RetrievalTrainer(cfg, mgr)
    tr.enable_grad_clipping(max_norm=1.0)
    tr.train_step_native(cva.synthetic.batch_from_numpy(b), do_optimizer=False, cc_indices=torch.from_numpy(np.concatenate([idx_c, idx_s])).cuda())
    union = tr.last_grad_norm()
    print(f"two ranks: norms {res[0]['norms'].tolist()} union batch {union}")
    assert abs(float(res[0]["norms"][0]) - union) <= 2e-4 * union
    tr.close()
