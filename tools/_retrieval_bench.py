"""What the retrieval bench tools share (topk_bench.py, few_bench.py, half_bench.py, masked_bench.py, labeled_bench.py,
index_mutable_bench.py): HIP events around single calls, the arms alternating call by call in one process, medians; the command
line (--calls, --warmup, --out) and the JSON that --out names."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import coot_videotext_amd as cva


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def spread(v1, v2):
    """The run-to-run spread of an arm timed twice: the gap between its two medians plus its min-max range."""
    return abs(float(np.median(v1)) - float(np.median(v2))) + (max(v1 + v2) - min(v1 + v2))


def same(x, y):
    """(idx, scores) of two searches are the same bytes."""
    return bool((x[0] == y[0]).all()) and bool((x[1].view(torch.int32) == y[1].view(torch.int32)).all())


def alternate(arms, order, calls, warmup):
    """The milliseconds of every arm, name -> [calls], the arms taking turns in `order`.  An arm is a call, or (setup, call): setup
    runs untimed before each call and its result is passed to the call."""
    ms = {a: [] for a in order}
    for it in range(warmup + calls):
        for a in order:
            setup, call = arms[a] if isinstance(arms[a], tuple) else (None, arms[a])
            arg = setup() if setup else None
            t, _ = timed((lambda: call(arg)) if setup else call)
            if it >= warmup:
                ms[a].append(t)
            del arg
    return ms


def start(timer="HIP events around one call, arms alternating", library=False, options=(), **head):
    """(args, lib, res): the command line (options: further flags that take a value), the loaded library and the head of the result."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    for flag in options:
        ap.add_argument(flag, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = cva.lib.load()
    res = {"device": torch.cuda.get_device_name(0), **({"library": os.path.basename(cva.lib.LIB_PATH)} if library else {}), "calls": args.calls,
           "warmup": args.warmup, "timer": timer, **head}
    return args, lib, res


def finish(args, res):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
