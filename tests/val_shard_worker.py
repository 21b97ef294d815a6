"""One RANK of tests/test_gpu_val_shard.py (not a test module): a real process of the sharded validation.

    python tests/val_shard_worker.py <rank> <world> <port> <out.npz> <save_dir> <timing>

All ranks share ONE GPU (the test boxes have one), so the process group is "gloo" and dist.py stages its collectives through
host memory; the kernels and the host logic of validation.validate_epoch are exactly those of an RCCL run.
Every rank builds the same loader (seeded), validates it sharded and writes the flattened dictionary.  timing = 1: the wall time
of the replicated and of the sharded validation of a larger loader as well (several processes on one device: overhead only).
The parent imports loader(), trainer(), validate() and flatten() for its single-process run of the same thing.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (64, 48, 64, 4, 64, 128)
COUNTS = [[1, 2, 3, 4, 2, 1], [2, 5, 1], [3, 3, 1, 2, 4, 1, 2], [1], [4, 1, 2, 2, 3]]  # 5 ragged batches: 5 % 2 != 0, 5 % 3 != 0
TOPK, SEED, CC_WEIGHT = 5, 1234, 0.01


def loader(counts=COUNTS):
    import coot_videotext_amd as cva
    batches = [cva.synthetic.make_batch(40 + i, len(c), c, 12, 10, 9, 6, DIMS[0], DIMS[1], ragged=True) for i, c in enumerate(counts)]
    for i, b in enumerate(batches):
        b.key = [f"vid{i}_{j}" for j in range(len(b.key))]
    return batches


def timing_loader():
    rs = np.random.RandomState(3)
    return loader([rs.randint(1, 8, size=32).tolist() for _ in range(12)])


def trainer():
    import coot_videotext_amd as cva
    from oracle import coot_oracle as O
    from tests import helpers as H
    cfgs = H.full_cfgs(*DIMS)
    Ps = [O.make_params(cfgs[i], 1 + i, scale=0.05) for i in range(4)]
    cfg, mgr = H.make_manager(cfgs, Ps, dropout=0.0, cc_weight=CC_WEIGHT)
    return cva.RetrievalTrainer(cfg, mgr, is_test=True)


def validate(tr, batches, save_path, **kw):
    """The validation under test: clip level, top-K and the embedding export on; the cycle-consistency draws seeded."""
    import torch
    torch.manual_seed(SEED)
    return tr.validate_epoch(batches, val_clips=True, save_embs=True, save_path=save_path, topk=TOPK, **kw)


def flatten(out):
    """The result dictionary as {name: array} (floats as 0-d float64 arrays: compared with ==)."""
    flat = {"loss": np.float64(out["loss"]), "val_score_at_1": np.float64(out["val_score_at_1"]),
            "val_clip_sent_score_at_1": np.float64(out["val_clip_sent_score_at_1"])}
    for d in ("v2p", "p2v", "c2s", "s2c"):
        for k, v in out[d].items():
            flat[f"{d}.{k}"] = np.float64(v)
        flat[f"topk.{d}.idx"], flat[f"topk.{d}.score"] = out["topk"][d]
    for k, v in out["embeddings"].items():
        flat[f"emb.{k}"] = np.array(v)
    flat["has_file"] = np.int64("embeddings_file" in out)
    flat["keys"] = np.array(sorted(out))
    return flat


def main():
    rank, world, port, out_fn, save_dir, timing = sys.argv[1:7]
    rank, world, timing = int(rank), int(world), int(timing)
    import torch
    import torch.distributed as dist
    from coot_videotext_amd import dist as cdist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    tr = trainer()
    tr.dp = cdist.DataParallelContext()
    # (sharded is left at None: a context with more than one rank shards)
    out = validate(tr, loader(), os.path.join(save_dir, f"emb_rank{rank}.npz"))
    torch.cuda.synchronize()
    res = flatten(out)
    res["file_exists"] = np.int64(os.path.exists(os.path.join(save_dir, f"emb_rank{rank}.npz")))
    if timing:
        big = timing_loader()
        for name, sharded in (("replicated", False), ("sharded", True)):
            ts = []
            for it in range(6):
                dist.barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.validate_epoch(big, val_clips=True, sharded=sharded)
                torch.cuda.synchronize()
                dist.barrier()
                if it:  # (the first one warms the shapes up)
                    ts.append(time.perf_counter() - t0)
            res[f"wall_{name}_s"] = np.array(ts)
    np.savez(out_fn, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
