#!/usr/bin/env python
"""GalleryIndex.search_range / count_range for many queries: the tile route (coot_retrieval_range_tile_count, _scan, _tile_fill)
against the slices of 16 queries through the sweep (coot_retrieval_range_count, _scan, _fill), in the style of
tools/topk_range_bench.py: HIP events around single calls, the arms alternating call by call in one process, medians of --calls calls.
A route is forced through retrieval.RANGE_TILE_MIN_M / RANGE_TILE_MIN_M_16BIT (1: tile, 10^9: slices).  Galleries of 200 000 x 768 and
18 000 x 384; float32 and bfloat16 storage; M = 17, 32, 64, 128, 256, 512, 1 024 queries, query i planted on a gallery row; per query a
threshold taken from its own similarities so that exactly 2 rows, 0.1 % and 10 % of the gallery qualify.  Arms:
  slices1, slices2    index.search_range(q, t, max_results=T) through the slices (T = the exact size, known from an untimed call: no
                      synchronisation), timed twice: its run-to-run spread
  tile                the same call through the tile route
  count_slices, count_tile   index.count_range(q, t) through either route
  dense               torch.nonzero((unit(q) @ G.T) >= t[:, None]), G = an fp32 normalised copy of the gallery made beforehand (not
                      timed): not the chain the searches rank on
and per case whether both routes returned the same bytes.  `tile_wins` is what sets the thresholds: the tile median lies below the
slices' median by more than the slices' spread.

    python tools/range_tile_bench.py --out profiles/r25_range_tile.json
    python tools/range_tile_bench.py --trace-case 1      one case only (64 bfloat16 queries, 200 000 x 768, 0.1 %), for a kernel trace"""
import json

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd import retrieval
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768), (18000, 384)]
STORAGES = ("float32", "bfloat16")
QUERIES = (17, 32, 64, 128, 256, 512, 1024)
TILE, SLICES = 1, 10 ** 9


def routed(v, fn):
    def call():
        retrieval.RANGE_TILE_MIN_M = retrieval.RANGE_TILE_MIN_M_16BIT = v
        return fn()
    return call


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True, options=("--trace-case",),
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    shipped = (retrieval.RANGE_TILE_MIN_M, retrieval.RANGE_TILE_MIN_M_16BIT)
    res["shipped_thresholds"] = {"RANGE_TILE_MIN_M": shipped[0], "RANGE_TILE_MIN_M_16BIT": shipped[1]}
    res["rows"] = []
    trace = args.trace_case is not None
    for n, d in GALLERIES[:1] if trace else GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        for storage in ("bfloat16",) if trace else STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            unit_g = torch.nn.functional.normalize(index.gallery.float(), dim=1)  # the dense arm's copy
            for m in (64,) if trace else QUERIES:
                rows = torch.arange(m, device="cuda") * 9710 % n
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[rows]
                unit_q = torch.nn.functional.normalize(q, dim=1)
                sim = torch.cat([index.search(q[i:i + 16], 1, want_sim=True)[2] for i in range(0, m, 16)])
                ranked = torch.sort(sim, dim=1, descending=True)[0]
                del sim
                for label, hits in (("0.1 %", n // 1000),) if trace else (("2 rows", 2), ("0.1 %", n // 1000), ("10 %", n // 10)):
                    thr = ranked[:, hits - 1].contiguous()
                    ref = routed(SLICES, lambda: index.search_range(q, thr))()
                    total = int(ref[0][-1])
                    got = routed(TILE, lambda: index.search_range(q, thr))()
                    same = bool((got[0] == ref[0]).all() and (got[1] == ref[1]).all() and (got[2].view(torch.int32) == ref[2].view(torch.int32)).all())
                    search = lambda: index.search_range(q, thr, max_results=total)
                    count = lambda: index.count_range(q, thr)
                    arms = {"slices1": routed(SLICES, search), "tile": routed(TILE, search), "slices2": routed(SLICES, search),
                            "count_slices": routed(SLICES, count), "count_tile": routed(TILE, count),
                            "dense": lambda: torch.nonzero((unit_q @ unit_g.T) >= thr[:, None])}
                    if trace:
                        arms = {a: arms[a] for a in ("slices1", "tile")}
                    ms = alternate(arms, list(arms), args.calls, args.warmup)
                    torch.cuda.synchronize()
                    row = {"N": n, "d": d, "storage": storage, "M": m, "selectivity": label, "hits_per_query": hits, "hits_total": total,
                           "counts_are_exact": bool((torch.diff(ref[0]) == hits).all()), "tile_same_bytes_as_slices": same}
                    for a in arms:
                        row[a] = stats(ms[a])
                    if not trace:
                        sl = float(np.median(ms["slices1"] + ms["slices2"]))
                        sp = spread(ms["slices1"], ms["slices2"])
                        row.update({"slices_median_ms": round(sl, 4), "slices_spread_ms": round(sp, 4),
                                    "tile_over_slices": round(row["tile"]["median_ms"] / sl, 3),
                                    "tile_wins": bool(row["tile"]["median_ms"] < sl - sp),
                                    "count_tile_over_count_slices": round(row["count_tile"]["median_ms"] / row["count_slices"]["median_ms"], 3),
                                    "tile_over_dense": round(row["tile"]["median_ms"] / row["dense"]["median_ms"], 3),
                                    "dense_extra_bytes": int(unit_g.numel() * 4 + m * n * 4),
                                    "tile_extra_bytes": int(m * ((n + 127) // 128 + 1) * 4 + (m + 1) * 8 + m * 4
                                                            + lib.coot_retrieval_range_tile_workspace_bytes(m, n, d))})
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                del ranked
            del index, unit_g
    retrieval.RANGE_TILE_MIN_M, retrieval.RANGE_TILE_MIN_M_16BIT = shipped
    finish(args, res)


if __name__ == "__main__":
    main()
