#!/usr/bin/env python
"""GalleryIndex.search_adjusted for many queries: the tile route (coot_retrieval_topk_adjusted_tile) against the slices of 16 queries
through the sweep (coot_retrieval_topk_adjusted), in the style of tools/range_tile_bench.py: HIP events around single calls, the arms
alternating call by call in one process, medians.  A route is forced through retrieval.ADJUSTED_TILE_MIN_M / ADJUSTED_TILE_MIN_M_16BIT
(1: tile, ADJUSTED_TILE_NEVER: slices).  Galleries of 200 000 x 768 (medians of 5 calls) and 18 000 x 384 (medians of 20); float32 and
bfloat16 storage; K = 10; M = 17, 32, 64, 128, 256, 320, 512, 1 024 queries, query i planted on a gallery row; offsets 0.05 randn.  Arms:
  slices1, slices2    index.search_adjusted(q, 10, offset) through the slices, timed twice: its run-to-run spread
  tile                the same call through the tile route
  search              index.search(q, 10): the floor without offsets
  dense               ((unit(q) @ G.T) - offset).topk(10), G = an fp32 normalised copy of the gallery made beforehand (not timed): not
                      the chain the searches rank on
and per case the assertion that both routes returned the same bytes.  `tile_wins` is what sets the thresholds: the tile median lies
below the slices' median by more than the slices' spread.  --calls is not used: the calls per gallery are fixed above.

    python tools/adjusted_tile_bench.py --out profiles/r35_adjusted_tile.json
    python tools/adjusted_tile_bench.py --gallery 1      the second gallery only"""
import json

from _retrieval_bench import alternate, finish, same, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd import retrieval
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768, 5), (18000, 384, 20)]  # N, d, calls
STORAGES = ("float32", "bfloat16")
QUERIES = (17, 32, 64, 128, 256, 320, 512, 1024)
K = 10
TILE, SLICES = 1, retrieval.ADJUSTED_TILE_NEVER


def routed(v, fn):
    def call():
        retrieval.ADJUSTED_TILE_MIN_M = retrieval.ADJUSTED_TILE_MIN_M_16BIT = v
        return fn()
    return call


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True, options=("--gallery",),
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    shipped = (retrieval.ADJUSTED_TILE_MIN_M, retrieval.ADJUSTED_TILE_MIN_M_16BIT)
    res["shipped_thresholds"] = {"ADJUSTED_TILE_MIN_M": shipped[0], "ADJUSTED_TILE_MIN_M_16BIT": shipped[1]}
    res["calls"] = {f"{n} x {d}": c for n, d, c in GALLERIES}
    res["rows"] = []
    for n, d, calls in GALLERIES if args.gallery is None else [GALLERIES[int(args.gallery)]]:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        offset = 0.05 * torch.randn(n, device="cuda", generator=gen)
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            unit_g = torch.nn.functional.normalize(index.gallery.float(), dim=1)  # the dense arm's copy
            for m in QUERIES:
                rows = torch.arange(m, device="cuda") * 9710 % n
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[rows]
                unit_q = torch.nn.functional.normalize(q, dim=1)
                adjusted = lambda: index.search_adjusted(q, K, offset)
                ref, got = routed(SLICES, adjusted)(), routed(TILE, adjusted)()
                assert same(ref, got), (n, d, storage, m)  # both routes return the same bytes
                arms = {"slices1": routed(SLICES, adjusted), "tile": routed(TILE, adjusted), "slices2": routed(SLICES, adjusted),
                        "search": lambda: index.search(q, K), "dense": lambda: ((unit_q @ unit_g.T) - offset).topk(K)}
                ms = alternate(arms, list(arms), calls, args.warmup)
                torch.cuda.synchronize()
                sl = float(np.median(ms["slices1"] + ms["slices2"]))
                sp = spread(ms["slices1"], ms["slices2"])
                row = {"N": n, "d": d, "storage": storage, "M": m, "K": K, "calls": calls, "tile_same_bytes_as_slices": True}
                for a in arms:
                    row[a] = stats(ms[a])
                row.update({"slices_median_ms": round(sl, 4), "slices_spread_ms": round(sp, 4), "tile_over_slices": round(row["tile"]["median_ms"] / sl, 3),
                            "tile_wins": bool(row["tile"]["median_ms"] < sl - sp),
                            "tile_over_search": round(row["tile"]["median_ms"] / row["search"]["median_ms"], 3),
                            "slices_over_search": round(sl / row["search"]["median_ms"], 3),
                            "tile_over_dense": round(row["tile"]["median_ms"] / row["dense"]["median_ms"], 3),
                            "dense_extra_bytes": int(unit_g.numel() * 4 + m * n * 4),
                            "tile_extra_bytes": int(lib.coot_retrieval_topk_adjusted_tile_workspace_bytes(m, n, d, K))})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            del index, unit_g
    retrieval.ADJUSTED_TILE_MIN_M, retrieval.ADJUSTED_TILE_MIN_M_16BIT = shipped
    # each constant: the smallest measured M from which the tile route wins at every gallery measured here and at every larger M
    for name, storage in (("ADJUSTED_TILE_MIN_M", "float32"), ("ADJUSTED_TILE_MIN_M_16BIT", "bfloat16")):
        wins = {m: all(r["tile_wins"] for r in res["rows"] if r["storage"] == storage and r["M"] == m) for m in QUERIES}
        rung = next((m for m in QUERIES if all(wins[x] for x in QUERIES if x >= m)), None)
        res.setdefault("measured_thresholds", {})[name] = rung
    print(json.dumps(res["measured_thresholds"]), flush=True)
    finish(args, res)


if __name__ == "__main__":
    main()
