"""A/B of the gradient norm / clipping cost on the anet training step (bench.py's timed mode: deterministic, two batches in turn, the
next batch announced, the text join deferred), arms alternating in ONE process:

    off          no clipper (what bench.py times)
    report       GradClip(max_norm) report-only: the norm behind the updates, one launch per side
    before       GradClip(max_norm, before_update=True): the norm in front of one update of all four networks
    scaler       LossScaler at a fixed power-of-two scale alone
    scaler+clip  LossScaler + clipping before the update (the norm rides on the scaler's check launch)

    python tools/clip_ab.py --steps 20 --warmup 5 --rounds 5 [--out profiles/rXX_clip_ab.json]

Each round times every arm once (K steps after W warm-up steps, events around the K steps); the median per arm is reported with
the per-round ratios against "off" (and scaler+clip against scaler).  One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ARMS = ("off", "report", "before", "scaler", "scaler+clip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-norm", type=float, default=0.1)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--out")
    args = ap.parse_args()
    import coot_videotext_amd as cva
    from coot_videotext_amd.trainer_retrieval import GradClip, LossScaler
    cva.lib.load()
    w = cva.synthetic.WORKLOADS["anet"]
    arms = args.arms.split(",")
    cfg = cva.load_named_config(*cva.synthetic.WORKLOAD_CONFIG["anet"])
    torch.manual_seed(0)
    mgr = cva.RetrievalModelManager(cfg).cuda()
    tr = cva.RetrievalTrainer(cfg, mgr)
    tr.set_deterministic(True)
    mgr.set_all_models_train()
    batches = []
    for sd in (1234, 9234):
        b = cva.synthetic.make_batch(sd, w["B"], w["C"], w["Lv"], w["Lc"], w["Lp"], w["Ls"], w["Dv"], w["Dt"], ragged=False)
        b.global_max_synced = True
        batches.append(b)
    clips = {"report": GradClip(args.max_norm), "before": GradClip(args.max_norm, before_update=True),
             "scaler+clip": GradClip(args.max_norm, before_update=True)}
    scaler = LossScaler(init_scale=2.0 ** 12, growth_factor=1.0, backoff_factor=1.0)
    turn = [0]

    def arm_on(a):
        tr.disable_grad_clipping()
        tr.disable_loss_scaling()
        if a in ("scaler", "scaler+clip"):
            tr.enable_loss_scaling(scaler)
        if a in clips:
            tr.enable_grad_clipping(clips[a])

    def step():
        cur, nxt = batches[turn[0] & 1], batches[(turn[0] + 1) & 1]
        turn[0] += 1
        return tr.train_step_native(cur, defer_join=True, next_batch=nxt)

    times = {a: [] for a in arms}
    for _r in range(args.rounds):
        for a in arms:
            arm_on(a)
            for _ in range(args.warmup):
                step()
            tr.join_streams()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            tr.join_streams()
            e1.record()
            torch.cuda.synchronize()
            times[a].append(e0.elapsed_time(e1) / args.steps)
    norms = {a: clips[a].norm() for a in clips if a in arms}
    med = {a: statistics.median(v) for a, v in times.items()}
    out = {"workload": "anet", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "max_norm": args.max_norm,
           "ms_per_step_median": med, "ms_per_step": times, "last_norm": norms}
    if "off" in times:
        out["ratio_vs_off"] = {a: [x / y for x, y in zip(times[a], times["off"])] for a in arms if a != "off"}
    if "scaler" in times and "scaler+clip" in times:
        out["scaler+clip_vs_scaler"] = [x / y for x, y in zip(times["scaler+clip"], times["scaler"])]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
