#!/usr/bin/env python
"""Device top-K retrieval search (coot_retrieval_topk) against the only thing a user had before it, torch.topk(q @ g.T, k) in fp32
on the same device, at the ActivityNet validation shape (4 917 x 4 917 x 768), the clip level (18 000 x 18 000 x 384) and
1 024 queries x 200 000 clips x 768, K = 10.  HIP events around single calls, the two arms alternating call by call on one box;
medians.  FLOPs = 2 M N d (the similarities; the selection is not counted), share of the fp32 vector peak (157.3 TFLOP/s).
Usage: python tools/topk_bench.py [--calls 20] [--warmup 5] [--out profiles/<tag>_topk.json]"""
import json

from _retrieval_bench import alternate, finish, start
import numpy as np
import torch
from coot_videotext_amd.retrieval import retrieval_topk_device

PEAK_FP32_VALU = 157.3e12
SHAPES = ((4917, 4917, 768, 10), (18000, 18000, 384, 10), (1024, 200000, 768, 10))


def main():
    args, lib, res = start(peak_fp32_valu_tflops=PEAK_FP32_VALU / 1e12, shapes=[])
    for m, n, d, k in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(m + n)
        g = torch.randn(n, d, device="cuda", generator=gen)
        q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[torch.arange(m, device="cuda") % n]
        q = q / (q * q).sum(-1, keepdim=True).sqrt()
        g = g / (g * g).sum(-1, keepdim=True).sqrt()
        arms = {"coot_retrieval_topk": lambda: retrieval_topk_device(q, g, k)[:2],
                "coot_retrieval_topk_normalize": lambda: retrieval_topk_device(q, g, k, normalize=True)[:2],
                "torch_matmul_topk": lambda: torch.topk(q @ g.T, k)}
        ms = alternate(arms, list(arms), args.calls, args.warmup)
        idx, sc = arms["coot_retrieval_topk"]()
        tv, ti = arms["torch_matmul_topk"]()
        torch.cuda.synchronize()
        flops = 2.0 * m * n * d
        row = {"M": m, "N": n, "d": d, "K": k, "workspace_bytes": int(lib.coot_retrieval_topk_workspace_bytes(m, n, d, k)), "matrix_bytes": m * n * 4,
               # the torch product is not the chain the ranks are counted on: its neighbours may differ at near-ties
               "rows_with_the_same_indices_as_torch": float((idx.long() == ti).all(1).float().mean()),
               "max_abs_score_difference_to_torch": float((sc - tv).abs().max())}
        for a, v in ms.items():
            med = float(np.median(v))
            row[a] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "tflops": round(flops / (med * 1e-3) / 1e12, 2),
                      "share_of_fp32_valu_peak": round(flops / (med * 1e-3) / PEAK_FP32_VALU, 4)}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del q, g
        torch.cuda.empty_cache()
    finish(args, res)


if __name__ == "__main__":
    main()
