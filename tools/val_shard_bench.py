#!/usr/bin/env python
"""Cost of the strip call of sharded validation on ONE GPU (information and a guard, no scaling claim): coot_retrieval_ranks of a
build of the PARENT commit (--parent-lib: its libcoot_hip.so, loaded next to this tree's) against this tree's whole call, the
strip call covering all rows and one strip of 1/8 of the rows, at the ActivityNet validation shape (4 917 x 768) and the clip
level (18 000 x 384), normalize on (as validate_epoch calls it), no metrics.  HIP events around single calls, the arms alternating
call by call; the parent arm runs TWICE per round (parent_a, parent_b): the difference between the two is the parent's own
run-to-run spread in this session, the bound this tree's whole call and the full-rows strip call are read against.
--validate-wall: also the wall time of validate_epoch replicated against sharded with TWO PROCESSES ON THE ONE DEVICE
(tests/val_shard_worker.py over gloo): the processes share the GPU, so this shows overhead only, never a speed-up.
Usage: python tools/val_shard_bench.py --parent-lib <libcoot_hip.so of the parent> [--calls 20] [--warmup 5] [--validate-wall]
       [--out profiles/<tag>_val_shard.json]"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import coot_videotext_amd as cva

SHAPES = ((4917, 768), (18000, 384))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
            "p25_ms": round(float(np.percentile(v, 25)), 4), "p75_ms": round(float(np.percentile(v, 75)), 4)}


def validate_wall(world=2):
    port_sock = socket.socket()
    port_sock.bind(("127.0.0.1", 0))
    port = port_sock.getsockname()[1]
    port_sock.close()
    with tempfile.TemporaryDirectory() as tmp:
        outs = [os.path.join(tmp, f"rank{r}.npz") for r in range(world)]
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "val_shard_worker.py"), str(r), str(world), str(port), outs[r], tmp, "1"],
                                  cwd=ROOT) for r in range(world)]
        try:
            rcs = [p.wait(timeout=600) for p in procs]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        assert rcs == [0] * world, rcs
        res = [dict(np.load(o)) for o in outs]
    out = {"what": f"validate_epoch(val_clips=True) of 12 batches x 32 videos (tests/val_shard_worker.py timing_loader), {world} PROCESSES ON ONE DEVICE over gloo "
                   "(collectives staged through host memory): overhead only, this cannot show a speed-up", "world": world, "runs": 5}
    for name in ("replicated", "sharded"):
        out[name] = [{k.replace("_ms", "_s"): v for k, v in stats(r[f"wall_{name}_s"]).items()} for r in res]  # per rank, seconds
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--validate-wall", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = cva.lib.load()
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    parent.coot_retrieval_workspace_bytes.restype = C.c_size_t
    parent.coot_retrieval_workspace_bytes.argtypes = lib.coot_retrieval_workspace_bytes.argtypes
    parent.coot_retrieval_ranks.argtypes = lib.coot_retrieval_ranks.argtypes
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
           "timer": "HIP events around one call, arms alternating call by call; normalize = 1, no metrics, no sim_out", "shapes": []}
    st = lambda: torch.cuda.current_stream().cuda_stream
    for n, d in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(n)
        e1 = torch.randn(n, d, device="cuda", generator=gen)
        e2 = 0.35 * e1 + torch.randn(n, d, device="cuda", generator=gen)
        ws = torch.empty(max(parent.coot_retrieval_workspace_bytes(n, d), lib.coot_retrieval_ranks_part_workspace_bytes(n, d)), dtype=torch.uint8, device="cuda")
        out = {a: torch.empty(2, n, dtype=torch.int32, device="cuda") for a in ("parent_a", "parent_b", "whole", "strip_all_rows", "strip_eighth")}
        eighth = (n // 8) * 3, n // 8  # an inner strip, not tile aligned

        def whole(L, o):
            return lambda: cva.lib.check(L.coot_retrieval_ranks(e1.data_ptr(), e2.data_ptr(), n, d, 1, o[0].data_ptr(), o[1].data_ptr(), None, None,
                                                                ws.data_ptr(), ws.numel(), st()), "coot_retrieval_ranks")

        def strip(o, row0, rows):
            return lambda: cva.lib.check(lib.coot_retrieval_ranks_part(e1.data_ptr(), e2.data_ptr(), n, d, 1, row0, rows, o[0].data_ptr(), o[1].data_ptr(), None,
                                                                       ws.data_ptr(), ws.numel(), st()), "coot_retrieval_ranks_part")

        arms = {"parent_a": whole(parent, out["parent_a"]), "whole": whole(lib, out["whole"]), "strip_all_rows": strip(out["strip_all_rows"], 0, n),
                "parent_b": whole(parent, out["parent_b"]), "strip_eighth": strip(out["strip_eighth"], *eighth)}
        ms = {a: [] for a in arms}
        for it in range(args.warmup + args.calls):
            for a, fn in arms.items():
                t = timed(fn)
                if it >= args.warmup:
                    ms[a].append(t)
        torch.cuda.synchronize()
        same = all(torch.equal(out["parent_a"], out[a]) for a in ("parent_b", "whole", "strip_all_rows"))
        row = {"N": n, "d": d, "strip_eighth_rows": list(eighth), "ranks_equal_the_parents": bool(same),
               "strip_eighth_rows_equal": bool(torch.equal(out["strip_eighth"][0, eighth[0]:eighth[0] + eighth[1]], out["parent_a"][0, eighth[0]:eighth[0] + eighth[1]]))}
        for a, v in ms.items():
            row[a] = stats(v)
        pa, pb = row["parent_a"]["median_ms"], row["parent_b"]["median_ms"]
        row["parent_run_to_run_ms"] = round(abs(pa - pb), 4)  # the same code, timed twice in the same rounds
        row["strip_all_rows_minus_parent_ms"] = round(row["strip_all_rows"]["median_ms"] - 0.5 * (pa + pb), 4)
        row["whole_minus_parent_ms"] = round(row["whole"]["median_ms"] - 0.5 * (pa + pb), 4)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del e1, e2, ws, out
        torch.cuda.empty_cache()
    if args.validate_wall:
        res["validate_epoch_wall"] = validate_wall(2)
        print(json.dumps(res["validate_epoch_wall"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
