#!/usr/bin/env python
"""Labelled retrieval ranking (coot_retrieval_ranks_labeled) against coot_retrieval_ranks, the square call it reduces to with
labels = arange, at the ActivityNet validation shape (4 917 x 4 917 x 768), normalize on, metrics included; and alone at
20 000 queries x 4 917 items x 768 with about 4 queries per item (labels = i mod N).  HIP events around single calls, the arms
alternating call by call in one process; medians.  The square arm is timed twice per round: the difference of its two medians is
the run-to-run spread the labelled call is read against.
Usage: python tools/labeled_bench.py [--calls 20] [--warmup 5] [--out profiles/<tag>_labeled.json]"""
import json

from _retrieval_bench import alternate, finish, start, stats
import torch
from coot_videotext_amd.retrieval import retrieval_ranks_device, retrieval_ranks_labeled_device

SHAPES = ((4917, 4917, 768), (20000, 4917, 768))


def main():
    args, lib, res = start(normalize=True, shapes=[])
    for m, n, d in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(m + n)
        g = torch.randn(n, d, device="cuda", generator=gen)
        lab = (torch.arange(m, device="cuda") % n).to(torch.int32)
        q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[lab.long()]
        arms = {"coot_retrieval_ranks_labeled": lambda: retrieval_ranks_labeled_device(q, g, lab, normalize=True)}
        if m == n:
            arms = {"coot_retrieval_ranks": lambda: retrieval_ranks_device(q, g, normalize=True), **arms,
                    "coot_retrieval_ranks_again": lambda: retrieval_ranks_device(q, g, normalize=True)}
        ms = alternate(arms, list(arms), args.calls, args.warmup)
        row = {"M": m, "N": n, "d": d, "queries_per_item": round(m / n, 2),
               "workspace_bytes": int(lib.coot_retrieval_ranks_labeled_workspace_bytes(m, n, d)), "matrix_bytes": m * n * 4}
        rq, rg, nv, met, _ = arms["coot_retrieval_ranks_labeled"]()
        row["n_valid"] = nv.tolist()
        row["r1"] = [round(float(x), 4) for x in met[:, 0]]
        if m == n:
            r12, r21, met_r, _ = arms["coot_retrieval_ranks"]()
            row["equals_the_square_call"] = bool(torch.equal(rq, r12) and torch.equal(rg, r21) and torch.equal(met, met_r))
        for a, v in ms.items():
            row[a] = stats(v)
        if m == n:
            sq = [row["coot_retrieval_ranks"]["median_ms"], row["coot_retrieval_ranks_again"]["median_ms"]]
            row["square_run_to_run_ms"] = round(abs(sq[0] - sq[1]), 4)
            row["labeled_minus_square_ms"] = round(row["coot_retrieval_ranks_labeled"]["median_ms"] - min(sq), 4)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del q, g
        torch.cuda.empty_cache()
    finish(args, res)


if __name__ == "__main__":
    main()
