"""Golden trajectories of the reference's step body with gradient clipping before the optimizer step.

The step body is oracle/gen_golden.py's gen_train_trajectory (coot/trainer_retrieval.py:253-291) with
torch.nn.utils.clip_grad_norm_ over all parameters of the four networks (nntrainer/trainer_base.py:545-554: the parameters of
model_mgr.get_all_params()) inserted between backward() and opt.step().  The reference itself clips after opt.step(), where the
clipped gradients are thrown away by the next zero_grad(): its parameters do not move differently, and the norm it reports equals
the norm recorded here (the gradients are the same before and after its step).

Stored: the trajectory keys of gen_train_trajectory plus grad_norm[steps] (the norm clip_grad_norm_ returned), clip_coef[steps]
(min(max_norm / (norm + 1e-6), 1)) and clip_max_norm.  max_norm = 0.3 x the first step's norm, so every step clips.  The generator
asserts that the clipped run's losses and parameter deltas leave the trajectory test's bounds around the UNclipped fixture of the
same problem (traj_*_eps.npz), so that the clipped fixture tells clipping from no clipping.

Runs only where the reference tree is (like oracle/gen_golden.py):

    python tools/gen_golden_clip.py                  # both fixtures
    python tools/gen_golden_clip.py traj_small_clip_eps
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (the reference's import shims and the trajectory helpers)

th = G.th
O, DM = G.O, G.DM

# the bounds of tests/test_gpu_train_trajectory.py (CASES) for the unclipped fixtures: (loss rel, min delta cosine, max delta norm error)
BOUNDS = {"traj_small_eps": (5e-3, 0.998, 0.02), "traj_anet_eps": (5e-4, 0.999, 0.01)}


def run(dims, B, counts, Ls, seed, steps, p, step_seed0, max_norm, scale=0.05, ragged=True, adam_eps=None, layers=1):
    """The reference's step body for `steps` steps, clip_grad_norm_(max_norm) between backward and opt.step (max_norm None: no
    clipping, the norm is still taken).  Returns (mgr, init, losses, idxs, seeds, norms, cfg)."""
    dv, dt, hidden, heads, ff, pool_hidden = dims
    Lv, Lc, Lp, Lsent = Ls
    cfg = G.ref_config(*dims, layers=layers, dropout=p)
    if adam_eps is not None:
        cfg.optimizer.adam_eps = adam_eps
    ocfgs = G.oracle_cfgs(*dims, layers=layers)
    th.manual_seed(0)
    mgr = G.model_retrieval.RetrievalModelManager(cfg)
    for i, k in enumerate(G.NET_KEYS):
        G.load_params(mgr.model_dict[k], O.make_params(ocfgs[i], seed + 10 * i, scale=scale))
    mgr.set_all_models_train()
    states = [G.inject_dropout(mgr.model_dict[k], 0, float(p)) for k in G.NET_KEYS]
    params, _names, params_flat = mgr.get_all_params()
    opt = G.optimization.make_optimizer(cfg.optimizer, params)
    init = {(k, n): q.detach().clone() for k in G.NET_KEYS for n, q in mgr.model_dict[k].named_parameters()}
    tr = G._FakeTrainer(cfg)
    losses, idxs, seeds, norms = [], [], [], []
    for s in range(steps):
        step_seed = int(step_seed0) + 7919 * s
        for stt, net_seed in zip(states, DM.step_net_seeds(step_seed)):
            stt.update(seed=net_seed, calls=0, row_next=0, tok_next=0, layout=None)
        batch = G.to_batch(O.make_batch(seed + 100 + (s & 1), B, counts, Lv, Lc, Lp, Lsent, dv, dt, ragged=ragged, corr=0.5))
        opt.zero_grad()
        vis = mgr.encode_visual(batch)
        txt = mgr.encode_text(batch)
        contr = tr.compute_total_constrastive_loss(vis, txt)
        ic, isent = G.draw_cc_indices(seed + 7 + s, vis.clip_emb_mask, txt.sent_emb_mask)
        th.manual_seed(seed + 7 + s)
        cc = tr.compute_cyclecons_loss(vis, txt)
        (contr + cc).backward()
        norm = th.nn.utils.clip_grad_norm_(params_flat, float("inf") if max_norm is None else max_norm)
        opt.step()
        losses.append([float(contr), float(cc)])
        idxs.append(np.stack([ic, isent]))
        seeds.append(step_seed)
        norms.append(float(norm))
    return mgr, init, losses, idxs, seeds, norms, cfg


def gen(name, unclipped, traj, adam_eps=1e-3, full=True, sub_step=29):
    traj = dict(traj)
    traj.pop("full", None)
    first = run(**dict(traj, steps=1), max_norm=None, adam_eps=adam_eps)[5][0]
    max_norm = float(np.float32(0.3 * first))
    mgr, init, losses, idxs, seeds, norms, cfg = run(**traj, max_norm=max_norm, adam_eps=adam_eps)
    coefs = [min(max_norm / (n + 1e-6), 1.0) for n in norms]
    for s, (l_, n_, c_) in enumerate(zip(losses, norms, coefs)):
        print(f"  {name} step {s}: contrastive {l_[0]:.5f} cycle-consistency {l_[1]:.6f} grad norm {n_:.6f} coef {c_:.4f}", flush=True)
    assert all(c < 1.0 for c in coefs), coefs
    dims, Ls = traj["dims"], traj["Ls"]
    dv, dt, hidden, heads, ff, pool_hidden = dims
    Lv, Lc, Lp, Lsent = Ls
    steps, scale, ragged = traj["steps"], traj.get("scale", 0.05), traj.get("ragged", True)
    out = dict(losses=np.array(losses, dtype=np.float64), cc_idx=np.array(idxs, dtype=np.int64), step_seeds=np.array(seeds, dtype=np.uint64),
               meta=np.array([traj["seed"], traj["B"], Lv, Lc, Lp, Lsent, dv, dt, hidden, heads, ff, pool_hidden]), ragged=np.array(int(ragged)),
               cc_weight=np.array(float(cfg.train.loss_cycle_cons)), param_scale=np.array(scale), counts=np.asarray(traj["counts"]),
               layers=np.array(1), train_p=np.array(float(traj["p"])), steps=np.array(steps), sub_step=np.array(sub_step),
               train_packed=np.array(0), opt_name=np.array(cfg.optimizer.name),
               radam_degentosgd=np.array(int(bool(cfg.optimizer.radam_degentosgd))),
               adam=np.array([cfg.optimizer.lr, cfg.optimizer.momentum, cfg.optimizer.adam_beta2, cfg.optimizer.adam_eps,
                              cfg.optimizer.weight_decay, float(cfg.optimizer.weight_decay_for_bias)], dtype=np.float64),
               grad_norm=np.array(norms, dtype=np.float64), clip_coef=np.array(coefs, dtype=np.float64), clip_max_norm=np.array(max_norm))
    for k in G.NET_KEYS:
        for n, q in mgr.model_dict[k].named_parameters():
            d = (q.detach() - init[(k, n)]).numpy()
            out[f"dnorm:{k}:{n}"] = np.array(np.linalg.norm(d.astype(np.float64)))
            out[f"delta:{k}:{n}"] = d if (full or d.size <= 4096) else G.subsample(d, sub_step)

    # power: the clipped run must leave the trajectory test's bounds around the unclipped fixture (and the unclipped one around this)
    ref = dict(np.load(os.path.join(G.OUT, unclipped + ".npz")))
    loss_tol, cos_min, norm_tol = BOUNDS[unclipped]
    assert np.array_equal(ref["step_seeds"], out["step_seeds"]) and np.array_equal(ref["cc_idx"], out["cc_idx"])
    loss_out = int(np.sum(np.abs(out["losses"][:, 0] - ref["losses"][:, 0]) > loss_tol * np.abs(ref["losses"][:, 0])))
    bad = 0
    for key in out:
        if not key.startswith("delta:"):
            continue
        a, b = out[key].reshape(-1).astype(np.float64), ref[key].reshape(-1).astype(np.float64)
        rn = float(ref["dnorm:" + key[6:]])
        if rn == 0.0:
            continue
        c = float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        nr = float(out["dnorm:" + key[6:]]) / rn
        bad += not (c >= cos_min and abs(nr - 1) <= norm_tol)
    print(f"  {name}: vs {unclipped}: {loss_out} of {steps} contrastive losses and {bad} parameter deltas outside the trajectory bounds")
    assert loss_out >= 1 and bad >= 10, (loss_out, bad)
    path = os.path.join(G.OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", name, os.path.getsize(path), "bytes")


def gen_traj_small_clip_eps():
    gen("traj_small_clip_eps", "traj_small_eps", G.TRAJ_SMALL)


def gen_traj_anet_clip_eps():
    gen("traj_anet_clip_eps", "traj_anet_eps", G.TRAJ_ANET, full=False)


if __name__ == "__main__":
    for n in (sys.argv[1:] or ["traj_small_clip_eps", "traj_anet_clip_eps"]):
        globals()["gen_" + n]()
