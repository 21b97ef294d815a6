#!/usr/bin/env python
"""GalleryIndex.search_range (coot_retrieval_range_count, _scan, _fill) against what a user had before it, in the style of
tools/topk_scoped_bench.py: HIP events around single calls, the arms alternating call by call in one process, medians of --calls calls
and the spread of an arm timed twice.  Galleries of 200 000 x 768 and 18 000 x 384; float32 and bfloat16 storage; M = 1, 16 and 64
queries, query i planted on a gallery row; per query a threshold taken from its own similarities so that exactly 2 rows, 0.1 % and
10 % of the gallery qualify.  Arms:
  range_cap           index.search_range(q, t, max_results=T): no synchronisation (T = the exact size, known from an untimed call)
  range_exact         index.search_range(q, t): reads the size back, allocates exactly
  count               index.count_range(q, t): the counting sweep and the scan alone
  search1, search2    (a) index.search(q, 10): the same sweep with a selection (timed twice: its run-to-run spread).  Up to 16 queries,
                      and for any M on 16-bit storage, this is the sweep the range kernel was derived from; 64 queries on a float32
                      index take the tile search
  dense               (b) torch.nonzero((unit(q) @ G.T) >= t[:, None]), G = an fp32 normalised copy of the gallery made beforehand (not
                      timed; its bytes and those of the M x N matrix are reported): not the chain the searches rank on
  top128              (c) the workaround: index.search(q, 128) filtered by the threshold; `top128_short_queries` counts the queries
                      for which it returns fewer rows than the exact answer
and per case whether range_cap and range_exact returned the same bytes.

    python tools/topk_range_bench.py --out profiles/r24_topk_range.json"""
import json

from _retrieval_bench import alternate, finish, spread, start, stats
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
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            unit_g = torch.nn.functional.normalize(index.gallery.float(), dim=1)  # the dense arm's copy
            for m in QUERIES:
                rows = torch.arange(m, device="cuda") * 9710 % n
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[rows]
                unit_q = torch.nn.functional.normalize(q, dim=1)
                sim = torch.cat([index.search(q[i:i + 16], 1, want_sim=True)[2] for i in range(0, m, 16)])
                ranked = torch.sort(sim, dim=1, descending=True)[0]
                del sim
                for label, hits in (("2 rows", 2), ("0.1 %", n // 1000), ("10 %", n // 10)):
                    thr = ranked[:, hits - 1].contiguous()
                    off, ex_rows, ex_scores = index.search_range(q, thr)
                    counts = torch.diff(off)
                    total = int(off[-1])

                    def top128():
                        idx, sc = index.search(q, 128)[:2]
                        hit = sc >= thr[:, None]
                        return idx[hit], sc[hit]

                    def dense():
                        return torch.nonzero((unit_q @ unit_g.T) >= thr[:, None])
                    search = lambda: index.search(q, K)[:2]
                    arms = {"search1": search, "range_cap": lambda: index.search_range(q, thr, max_results=total), "search2": search,
                            "range_exact": lambda: index.search_range(q, thr), "count": lambda: index.count_range(q, thr), "dense": dense,
                            "top128": top128}
                    ms = alternate(arms, list(arms), args.calls, args.warmup)
                    cap = arms["range_cap"]()
                    torch.cuda.synchronize()
                    row = {"N": n, "d": d, "storage": storage, "M": m, "selectivity": label, "hits_per_query": hits, "hits_total": total,
                           "counts_are_exact": bool((counts == hits).all()),
                           "cap_same_bytes_as_exact": bool((cap[0] == off).all() and (cap[1] == ex_rows).all()
                                                           and (cap[2].view(torch.int32) == ex_scores.view(torch.int32)).all()),
                           "top128_short_queries": int((counts > 128).sum()), "dense_rows_found": int(dense().shape[0])}
                    for a in arms:
                        row[a] = stats(ms[a])
                    floor = float(np.median(ms["search1"] + ms["search2"]))
                    row.update({"search_median_ms": round(floor, 4), "search_spread_ms": round(spread(ms["search1"], ms["search2"]), 4),
                                "range_cap_over_search": round(row["range_cap"]["median_ms"] / floor, 3),
                                "range_exact_over_search": round(row["range_exact"]["median_ms"] / floor, 3),
                                "count_over_search": round(row["count"]["median_ms"] / floor, 3),
                                "range_cap_over_dense": round(row["range_cap"]["median_ms"] / row["dense"]["median_ms"], 3),
                                "range_cap_over_top128": round(row["range_cap"]["median_ms"] / row["top128"]["median_ms"], 3),
                                "dense_extra_bytes": int(unit_g.numel() * 4 + m * n * 4),
                                "range_extra_bytes": int(m * ((n + 127) // 128 + 1) * 4 + (m + 1) * 8 + m * 4
                                                         + lib.coot_retrieval_range_workspace_bytes(min(m, 16), n, d))})
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                del ranked
            del index, unit_g
    finish(args, res)


if __name__ == "__main__":
    main()
