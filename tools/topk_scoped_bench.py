#!/usr/bin/env python
"""GalleryIndex.search_scoped (coot_retrieval_topk_scoped) against what a user had before it, in the style of
tools/topk_multi_bench.py: HIP events around single calls, the arms alternating call by call in one process, medians of --calls calls
and the spread of an arm timed twice.  K = 10; galleries of 200 000 x 768 and 18 000 x 384; float32 and bfloat16 storage; G = N / 10
ids of 10 rows, once as adjacent rows and once scattered over the gallery; M = 1, 16 and 64 queries, query i planted on a row of its
own video and scoped to that video's id; both modes.  Arms:
  scoped              index.search_scoped(q, 10, groups, only=scope) resp. exclude=scope
  loop                (a) what the parent offers: M calls index.search(q[i:i + 1], 10, keep=mask_i), the M masks built beforehand
                      (not timed): M masks of N bytes, M launch chains, M sweeps
  plain1, plain2      (b) index.search(q, 10): no scope at all (timed twice: its run-to-run spread).  Up to 16 queries, and for any M
                      on 16-bit storage, this is the same sweep without the eligibility word; 64 queries on a float32 index take
                      the tile search
and per case whether scoped and (a) returned the same bytes.

    python tools/topk_scoped_bench.py --out profiles/r23_topk_scoped.json"""
import json

from _retrieval_bench import alternate, finish, same, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768), (18000, 384)]
STORAGES = ("float32", "bfloat16")
QUERIES = (1, 16, 64)
K = 10


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True, K=K,
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    res["rows"] = []
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        adjacent = (torch.arange(n, device="cuda") // 10).to(torch.int32)
        layouts = {"adjacent": adjacent, "scattered": adjacent[torch.randperm(n, device="cuda", generator=gen)].contiguous()}
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            for m in QUERIES:
                rows = torch.arange(m, device="cuda") * 9710 % n
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[rows]
                for layout, groups in layouts.items():
                    scope = groups[rows].contiguous()
                    for mode in ("only", "exclude"):
                        masks = (groups[None] == scope[:, None]) != (mode == "exclude")  # [M, N] bool, one mask per query
                        plain = lambda: index.search(q, K)[:2]

                        def loop():
                            out = [index.search(q[i:i + 1], K, keep=masks[i])[:2] for i in range(m)]
                            return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
                        arms = {"plain1": plain, "scoped": lambda: index.search_scoped(q, K, groups, **{mode: scope})[:2], "plain2": plain, "loop": loop}
                        ms = alternate(arms, list(arms), args.calls, args.warmup)
                        got, want = arms["scoped"](), arms["loop"]()
                        torch.cuda.synchronize()
                        row = {"N": n, "d": d, "storage": storage, "M": m, "groups": n // 10, "layout": layout, "mode": mode,
                               "same_bytes_as_loop": same(got, want)}
                        for a in arms:
                            row[a] = stats(ms[a])
                        floor = float(np.median(ms["plain1"] + ms["plain2"]))
                        med = row["scoped"]["median_ms"]
                        row.update({"plain_median_ms": round(floor, 4), "plain_spread_ms": round(spread(ms["plain1"], ms["plain2"]), 4),
                                    "scoped_over_plain": round(med / floor, 3), "scoped_minus_plain_ms": round(med - floor, 4),
                                    "scoped_over_loop": round(med / row["loop"]["median_ms"], 3),
                                    "workspace_bytes": int(lib.coot_retrieval_topk_scoped_workspace_bytes(min(m, 16), n, d, K))})
                        res["rows"].append(row)
                        print(json.dumps(row), flush=True)
                        del masks
            del index
    finish(args, res)


if __name__ == "__main__":
    main()
