#!/usr/bin/env python
"""GalleryIndex.search with more than 16 queries, before and after coot_retrieval_topk_index, in the style of tools/masked_bench.py:
HIP events around single index.search calls, the arms alternating call by call, medians of --calls calls.  K = 10; M = 17, 32, 64,
256, 320, 512 and 1 024 queries; galleries of 200 000 x 768 and 18 000 x 384; float32, bfloat16 and float16 storage; without a filter and with
10 % of the rows kept as one contiguous range.

The tool runs on either commit and writes its timings under --label into the JSON that --out names, keeping what another label left
there, so the parent's run and this commit's end up side by side:
    (on the parent commit, this file and the JSON copied into it)
                            python tools/index_tile_bench.py --label parent --out profiles/r17_topk_index.json
    (on this commit)        python tools/index_tile_bench.py --label branch --out profiles/r17_topk_index.json
Arms, in two rounds per case so that the first is the same sequence of calls on both commits (with other arms in between, the
200 000-row sweeps of the slices come out 4 to 8 % slower than back to back: what the caches hold differs):
  search1, search2  index.search as the commit routes it, timed twice per round so that its own run-to-run spread is on file
then, where retrieval.INDEX_TILE_MIN_M_16BIT exists, alternating with each other:
  old    the parent's route through this build, whose kernels are the parent's instruction for instruction: retrieval_topk_device on
         a float32 index (the gallery norms recomputed), slices of 16 queries through the few-query call on a 16-bit one
  tile   (16-bit storage) one coot_retrieval_topk_index call whatever the threshold says: what the threshold is chosen from
With both labels on file the tool adds "comparison": per case the parent's median and spread, this commit's median as routed, and
whether it is slower than the parent by more than the parent's own spread (|median 1 - median 2| + (max - min over both))."""
import json
import os

from _retrieval_bench import alternate, finish, same, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd import retrieval
from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device

GALLERIES = [(200000, 768), (18000, 384)]
QUERIES = (17, 32, 64, 256, 320, 512, 1024)
STORAGES = ("float32", "bfloat16", "float16")
K = 10
THRESHOLD = "INDEX_TILE_MIN_M_16BIT"


def with_threshold(value, fn):
    """fn() with the 16-bit routing threshold set to value."""
    def run():
        shipped = getattr(retrieval, THRESHOLD)
        setattr(retrieval, THRESHOLD, value)
        try:
            return fn()
        finally:
            setattr(retrieval, THRESHOLD, shipped)
    return run


def key(row):
    return (row["N"], row["d"], row["storage"], row["M"], row["filter"])


def compare(parent, branch):
    rows, by = [], {key(r): r for r in parent}
    for b in branch:
        p = by.get(key(b))
        if p is None:
            continue
        p_ms, b_ms = p["search_median_ms"], b["search_median_ms"]
        row = {k: b[k] for k in ("N", "d", "storage", "M", "filter")}
        row.update({"parent_ms": p_ms, "parent_spread_ms": p["search_spread_ms"], "branch_ms": b_ms, "branch_route": b.get("route", "?"),
                    "branch_over_parent": round(b_ms / p_ms, 3), "slower_than_the_parent_by_more_than_its_spread": bool(b_ms - p_ms > p["search_spread_ms"])})
        if "tile" in b:
            row["tile_ms"] = b["tile"]["median_ms"]
            row["tile_no_slower_than_the_parents_slices"] = bool(b["tile"]["median_ms"] <= p_ms)
        rows.append(row)
    return rows


def main():
    args, _, res = start(timer="HIP events around one GalleryIndex.search call, arms alternating", library=True, options=["--label"], K=K,
                         spread="|median of the first timing - median of the second| + (max - min over both)")
    assert args.label, "--label parent | branch"
    has_tile = hasattr(retrieval, THRESHOLD)
    res["threshold_16bit"] = getattr(retrieval, THRESHOLD, None)
    res["rows"] = []
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        contig = torch.zeros(n, dtype=torch.bool, device="cuda")
        contig[int(0.45 * n):int(0.55 * n)] = True
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            for m in QUERIES:
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[torch.arange(m, device="cuda") * 7 % n]
                for name, keep in (("none", None), ("contig 10 %", contig)):
                    search = lambda: index.search(q, K, keep=keep)[:2]
                    arms, order = {"search1": search, "search2": search}, []
                    row = {"N": n, "d": d, "storage": storage, "M": m, "filter": name}
                    if has_tile:
                        if storage == "float32":
                            arms["old"] = lambda: retrieval_topk_device(q, index.gallery, K, normalize=index.normalize, keep=keep)[:2]
                            row["route"] = "tile"
                        else:
                            arms["old"] = with_threshold(1 << 30, search)
                            arms["tile"] = with_threshold(17, search)
                            row["route"] = "tile" if m >= getattr(retrieval, THRESHOLD) else "slices"
                        order = ["old"] + (["tile"] if "tile" in arms else [])
                        row["same_bytes_on_every_route"] = all(same(arms[a](), search()) for a in order)
                    ms = alternate(arms, ["search1", "search2"], args.calls, args.warmup)
                    if order:
                        ms.update(alternate(arms, order, args.calls, args.warmup))
                    torch.cuda.synchronize()
                    for a in ["search1", "search2"] + order:
                        row[a] = stats(ms[a])
                    row["search_median_ms"] = round(float(np.median(ms["search1"] + ms["search2"])), 4)
                    row["search_spread_ms"] = round(spread(ms["search1"], ms["search2"]), 4)
                    if "old" in arms:
                        row["search_over_old"] = round(row["search_median_ms"] / row["old"]["median_ms"], 3)
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
            del index
    out = {"runs": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out["runs"][args.label] = res
    if "parent" in out["runs"] and "branch" in out["runs"]:
        out["comparison"] = compare(out["runs"]["parent"]["rows"], out["runs"]["branch"]["rows"])
    finish(args, out)


if __name__ == "__main__":
    main()
