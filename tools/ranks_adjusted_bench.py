#!/usr/bin/env python
"""retrieval_ranks_adjusted_device (coot_retrieval_ranks_adjusted) against retrieval_ranks_labeled_device (coot_retrieval_ranks_labeled), the
same work without offsets: HIP events around single calls, the arms alternating call by call in one process, medians of --calls
calls.  Square validation sets of 4 917 x 384 and 18 000 x 384, labels = arange, normalize=True, offsets 0.05 randn.  Arms:
  labeled1, labeled2   the labelled ranking, timed twice: its run-to-run spread
  adjusted_none        the ranking under offsets without offsets
  adjusted_col         with the column offset
  adjusted_both        with both
and per case the assertion that without offsets the two calls return the same bytes.

    python tools/ranks_adjusted_bench.py --out profiles/r35_ranks_adjusted.json"""
import json

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd import retrieval

SIZES = [(4917, 384), (18000, 384)]


def main():
    args, _, res = start(timer="HIP events around one call, arms alternating", library=True,
                         spread="|median of the first timing - median of the second| + (max - min over both)")
    res["rows"] = []
    for n, d in SIZES:
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        q = torch.randn(n, d, device="cuda", generator=gen) + 0.35 * g
        lab = torch.arange(n, dtype=torch.int32, device="cuda")
        col, row = 0.05 * torch.randn(n, device="cuda", generator=gen), 0.05 * torch.randn(n, device="cuda", generator=gen)
        a, b = retrieval.retrieval_ranks_labeled_device(q, g, lab, normalize=True), retrieval.retrieval_ranks_adjusted_device(q, g, lab, normalize=True)
        assert all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(a[:4], b[:4])), (n, d)
        labeled = lambda: retrieval.retrieval_ranks_labeled_device(q, g, lab, normalize=True)
        arms = {"labeled1": labeled, "adjusted_none": lambda: retrieval.retrieval_ranks_adjusted_device(q, g, lab, normalize=True),
                "adjusted_col": lambda: retrieval.retrieval_ranks_adjusted_device(q, g, lab, col, normalize=True),
                "adjusted_both": lambda: retrieval.retrieval_ranks_adjusted_device(q, g, lab, col, row, normalize=True), "labeled2": labeled}
        ms = alternate(arms, list(arms), args.calls, args.warmup)
        torch.cuda.synchronize()
        base = float(np.median(ms["labeled1"] + ms["labeled2"]))
        sp = spread(ms["labeled1"], ms["labeled2"])
        out = {"M": n, "N": n, "d": d, "same_bytes_without_offsets": True, "labeled_median_ms": round(base, 4), "labeled_spread_ms": round(sp, 4)}
        for name in arms:
            out[name] = stats(ms[name])
        for name in ("adjusted_none", "adjusted_col", "adjusted_both"):
            out[name + "_over_labeled"] = round(out[name]["median_ms"] / base, 3)
            out[name + "_outside_spread"] = bool(abs(out[name]["median_ms"] - base) > sp)
        res["rows"].append(out)
        print(json.dumps(out), flush=True)
    finish(args, res)


if __name__ == "__main__":
    main()
