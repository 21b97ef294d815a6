#!/usr/bin/env python
"""GalleryIndex.search_adjusted (coot_retrieval_topk_adjusted) and GalleryIndex.hubness_offsets against what a user had before them,
in the style of tools/topk_scoped_bench.py: HIP events around single calls, the arms alternating call by call in one process, medians
of --calls calls and the spread of an arm timed twice.  K = 10; galleries of 200 000 x 768 and 18 000 x 384; float32 and bfloat16
storage; M = 1, 16, 64 and 1 024 queries, query i planted on a gallery row; offset = 0.05 randn, about the spread of the similarities
of unrelated rows.  Arms:
  adjusted            index.search_adjusted(q, 10, offset)
  plain1, plain2      (a) index.search(q, 10): no offset at all (timed twice: its run-to-run spread).  Up to 16 queries, and for up to
                      319 queries on 16-bit storage, this is the same sweep without the offset; more queries take the tile search
  resort              (b) the workaround: index.search(q, 128), scores - offset[idx], the 10 best of those 128 — inexact: a row
                      outside the raw top 128 may be inside the adjusted top 10 (differ_from_exact: the queries whose idx differ)
  dense               (c) ((unit(q) @ unit(g).T) - offset).topk(10) on a float32 unit(g) made beforehand (not timed), with the peak
                      memory it allocates; its order of equal scores and its rounding are torch's, not the searches'
and, per gallery and storage, hubness_offsets(bank, 10) against knn_join(bank, 10) alone for banks of 2 000 and 18 000 rows (the
added launch), knn_join timed twice.

    python tools/topk_adjusted_bench.py --out profiles/r34_topk_adjusted.json"""
import json

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768), (18000, 384)]
STORAGES = ("float32", "bfloat16")
QUERIES = (1, 16, 64, 1024)
BANKS = (2000, 18000)
K = 10


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True, K=K, offset="0.05 * randn(N)",
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    res["rows"], res["hubness"] = [], []
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        offset = 0.05 * torch.randn(n, device="cuda", generator=gen)
        unit_g = torch.nn.functional.normalize(g, dim=1)
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            for m in QUERIES:
                rows = torch.arange(m, device="cuda") * 9710 % n
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[rows]
                plain = lambda: index.search(q, K)[:2]

                def resort():
                    idx, sc, _ = index.search(q, 128)
                    best = (sc - offset[idx.long()]).topk(K, dim=1)
                    return torch.gather(idx, 1, best.indices), best.values

                def dense():
                    best = (torch.nn.functional.normalize(q, dim=1) @ unit_g.T - offset).topk(K, dim=1)
                    return best.indices.to(torch.int32), best.values
                arms = {"plain1": plain, "adjusted": lambda: index.search_adjusted(q, K, offset)[:2], "plain2": plain, "resort": resort, "dense": dense}
                ms = alternate(arms, list(arms), args.calls, args.warmup)
                exact, approx = arms["adjusted"](), arms["resort"]()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                full = arms["dense"]()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                row = {"N": n, "d": d, "storage": storage, "M": m, "resort_differ_from_exact": int((exact[0] != approx[0]).any(dim=1).sum()),
                       "dense_differ_from_exact": int((exact[0] != full[0]).any(dim=1).sum()), "dense_peak_bytes": int(peak)}
                for a in arms:
                    row[a] = stats(ms[a])
                floor = float(np.median(ms["plain1"] + ms["plain2"]))
                med = row["adjusted"]["median_ms"]
                row.update({"plain_median_ms": round(floor, 4), "plain_spread_ms": round(spread(ms["plain1"], ms["plain2"]), 4),
                            "adjusted_over_plain": round(med / floor, 3), "adjusted_minus_plain_ms": round(med - floor, 4),
                            "adjusted_over_resort": round(med / row["resort"]["median_ms"], 3), "adjusted_over_dense": round(med / row["dense"]["median_ms"], 3),
                            "workspace_bytes": int(lib.coot_retrieval_topk_adjusted_workspace_bytes(min(m, 16), n, d, K))})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                del exact, approx, full
            for b in BANKS:
                bank = GalleryIndex(torch.randn(b, d, device="cuda", generator=gen) + 0.35 * g[torch.arange(b, device="cuda") * 7 % n], storage=torch.float32)
                calls = args.calls if n * b <= 10 ** 9 else min(args.calls, 5)  # (the large join takes a good part of a second)
                join = lambda: index.knn_join(bank, K)
                arms = {"join1": join, "offsets": lambda: index.hubness_offsets(bank, K), "join2": join}
                ms = alternate(arms, list(arms), calls, min(args.warmup, 2))
                floor = float(np.median(ms["join1"] + ms["join2"]))
                row = {"N": n, "d": d, "storage": storage, "bank_rows": b, "calls": calls, "offsets": stats(ms["offsets"]), "join1": stats(ms["join1"]),
                       "join2": stats(ms["join2"]), "join_median_ms": round(floor, 4), "join_spread_ms": round(spread(ms["join1"], ms["join2"]), 4),
                       "offsets_minus_join_ms": round(float(np.median(ms["offsets"])) - floor, 4)}
                res["hubness"].append(row)
                print(json.dumps(row), flush=True)
                del bank
            del index
        del unit_g
    finish(args, res)


if __name__ == "__main__":
    main()
