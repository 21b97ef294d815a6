"""One RANK of tests/test_gpu_grad_clip.py's two-process test (not a test module): the data-parallel native step with gradient
clipping before the update, on the problem of tests/dp_worker.py.

    python tests/dp_clip_worker.py <rank> <world> <port> <out.npz> <seed> <cc_weight>

Writes the norm every step reported (after the all-reduce: the same bits on every rank) and the final parameters.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.dp_worker import DIMS, problem, shard_numpy  # noqa: E402


def main():
    rank, world, port, out, seed, cc_weight = sys.argv[1:7]
    rank, world, seed, cc_weight = int(rank), int(world), int(seed), float(cc_weight)
    b, counts, idx_c, idx_s, vid_counts, clip_counts, bounds = problem(seed, world)
    sh = shard_numpy(b, counts, bounds[rank], bounds[rank + 1])
    import torch
    import torch.distributed as dist
    import coot_videotext_amd as cva
    from coot_videotext_amd import dist as cdist
    from oracle import coot_oracle as O
    from tests import helpers as H
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfgs = H.full_cfgs(*DIMS)
    Ps = [O.make_params(cfgs[i], 1 + i, scale=0.02) for i in range(4)]
    cfg, mgr = H.make_manager(cfgs, Ps, dropout=0.0, cc_weight=cc_weight)
    mgr.set_all_models_train()
    tr = cva.RetrievalTrainer(cfg, mgr)
    tr.dp = cdist.DataParallelContext()
    batch = cva.synthetic.batch_from_numpy(sh)
    cc_idx = torch.from_numpy(np.concatenate([idx_c[bounds[rank]:bounds[rank + 1]], idx_s[bounds[rank]:bounds[rank + 1]]])).cuda()
    tr.enable_grad_clipping(max_norm=1e-3, before_update=True)
    norms = []
    for _ in range(3):
        tr.train_step_native(batch, cc_indices=cc_idx)
        norms.append(tr.last_grad_norm())
    torch.cuda.synchronize()
    res = {f"p{i}": n._flat.detach().cpu().numpy() for i, n in enumerate(mgr.model_dict.values())}
    res["norms"] = np.array(norms, dtype=np.float32)
    np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
