#!/usr/bin/env python
"""GalleryIndex.search_grouped (coot_retrieval_topk_grouped) against what a user had before it, in the style of
tools/index_tile_bench.py: HIP events around single calls, the arms alternating call by call in one process, medians of --calls
calls and the spread of an arm timed twice.  K = 10; M = 1 and 16 queries; galleries of 200 000 x 768 and 18 000 x 384; float32 and
bfloat16 storage; G = N / 10 groups of 10 rows, once as adjacent rows and once scattered over the gallery; without a filter and with
10 % of the rows kept as one contiguous range.  Arms:
  search1, search2   index.search(q, 10): the floor, the same sweep without the table (timed twice: its run-to-run spread)
  grouped            index.search_grouped(q, 10, groups, num_groups=G)
  workaround         index.search(q, 128) and a de-duplication in torch on the device (first row of every group, the first 10 of them)
and per case how many of the M queries the workaround answers with fewer than 10 groups, or with other (group, row) pairs than
search_grouped (it sees the 128 best rows only).

    python tools/topk_grouped_bench.py --out profiles/r18_topk_grouped.json

--label parent | branch runs something else: the ungrouped index.search cases of profiles/r13_topk_few.json (tools/few_bench.py, arm b)
on whatever commit the tool is started from, each timed twice, stored under that label in --out next to what is already there; with
both labels on file a "comparison" says whether this commit's search is slower than the parent's by more than the parent's own spread."""
import json
import os

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768), (18000, 384)]
QUERIES = (1, 16)
STORAGES = ("float32", "bfloat16")
K = 10
UNGROUPED = [(m, 200000, 768, 10) for m in (1, 4, 16)] + [(16, 200000, 768, 128)] + [(m, 18000, 384, 10) for m in (1, 4, 16)]  # tools/few_bench.py


def queries(g, m, gen):
    return torch.randn(m, g.shape[1], device="cuda", generator=gen) + 0.35 * g[torch.arange(m, device="cuda") * 7 % g.shape[0]]


def dedup(idx, scores, groups, k):
    """The workaround: of the rows a row search returned, the first of every group, the first k of those: (group, idx, scores)
    [M, k], -1 / -1 / -inf where they run out.  Device operations only."""
    m, w = idx.shape
    grp = torch.where(idx >= 0, groups[idx.clamp(min=0).long()], torch.full_like(idx, -1))
    earlier = torch.ones(w, w, dtype=torch.bool, device=idx.device).tril(-1)  # [r, c]: c < r
    dup = ((grp[:, :, None] == grp[:, None, :]) & earlier).any(-1) | (grp < 0)
    rank = torch.cumsum(~dup, 1) - 1
    take = ~dup & (rank < k)
    out = [torch.full((m, k + 1), -1, dtype=torch.int32, device=idx.device) for _ in range(2)] + [torch.full((m, k + 1), float("-inf"), device=idx.device)]
    slot = torch.where(take, rank, torch.full_like(rank, k))  # slot k: a bin for everything not taken
    for o, v in zip(out, (grp, idx, scores)):
        o.scatter_(1, slot, v)
    return [o[:, :k] for o in out]


def ungrouped(args, res):
    res["shapes"] = []
    made = {}
    for m, n, d, k in UNGROUPED:
        if (n, d) not in made:
            made.clear()
            torch.cuda.empty_cache()
            gen = torch.Generator(device="cuda").manual_seed(n + d)
            g = torch.randn(n, d, device="cuda", generator=gen)
            made[(n, d)] = (g, GalleryIndex(g, normalize=True), gen)
        g, index, gen = made[(n, d)]
        q = queries(g, m, gen)
        search = lambda: index.search(q, k)[:2]
        ms = alternate({"search1": search, "search2": search}, ["search1", "search2"], args.calls, args.warmup)
        row = {"M": m, "N": n, "d": d, "K": k, "search1": stats(ms["search1"]), "search2": stats(ms["search2"]),
               "search_median_ms": round(float(np.median(ms["search1"] + ms["search2"])), 4), "search_spread_ms": round(spread(ms["search1"], ms["search2"]), 4)}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)


def compare(parent, branch):
    rows, by = [], {(r["M"], r["N"], r["d"], r["K"]): r for r in parent}
    for b in branch:
        p = by[(b["M"], b["N"], b["d"], b["K"])]
        rows.append({"M": b["M"], "N": b["N"], "d": b["d"], "K": b["K"], "parent_ms": p["search_median_ms"], "parent_spread_ms": p["search_spread_ms"],
                     "branch_ms": b["search_median_ms"], "branch_over_parent": round(b["search_median_ms"] / p["search_median_ms"], 3),
                     "slower_than_the_parent_by_more_than_its_spread": bool(b["search_median_ms"] - p["search_median_ms"] > p["search_spread_ms"])})
    return rows


def grouped(args, res):
    res["rows"] = []
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        contig = torch.zeros(n, dtype=torch.bool, device="cuda")
        contig[int(0.45 * n):int(0.55 * n)] = True
        g_total = n // 10
        adjacent = (torch.arange(n, device="cuda") // 10).to(torch.int32)
        layouts = {"adjacent": adjacent, "scattered": adjacent[torch.randperm(n, device="cuda", generator=gen)].contiguous()}
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            for m in QUERIES:
                q = queries(g, m, gen)
                for layout, groups in layouts.items():
                    for name, keep in (("none", None), ("contig 10 %", contig)):
                        search = lambda: index.search(q, K, keep=keep)[:2]
                        arms = {"search1": search, "grouped": lambda: index.search_grouped(q, K, groups, num_groups=g_total, keep=keep)[:3],
                                "search2": search, "workaround": lambda: dedup(*index.search(q, 128, keep=keep)[:2], groups, K)}
                        ms = alternate(arms, list(arms), args.calls, args.warmup)
                        got, alt = arms["grouped"](), arms["workaround"]()
                        torch.cuda.synchronize()
                        short = (alt[0] < 0).any(1)
                        wrong = ((alt[0] != got[0]) | (alt[1] != got[1])).any(1)
                        row = {"N": n, "d": d, "storage": storage, "M": m, "groups": g_total, "layout": layout, "filter": name}
                        for a in arms:
                            row[a] = stats(ms[a])
                        floor = float(np.median(ms["search1"] + ms["search2"]))
                        row.update({"search_median_ms": round(floor, 4), "search_spread_ms": round(spread(ms["search1"], ms["search2"]), 4),
                                    "grouped_over_search": round(row["grouped"]["median_ms"] / floor, 3),
                                    "grouped_over_workaround": round(row["grouped"]["median_ms"] / row["workaround"]["median_ms"], 3),
                                    "workaround_queries_short_of_10_groups": int(short.sum()), "workaround_queries_wrong": int(wrong.sum()),
                                    "workspace_bytes": int(res["lib"].coot_retrieval_topk_grouped_workspace_bytes(m, n, d, K, g_total))})
                        res["rows"].append(row)
                        print(json.dumps(row), flush=True)
            del index
    del res["lib"]


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True, options=["--label"], K=K,
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    out = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    if args.label:
        ungrouped(args, res)
        runs = out.setdefault("ungrouped_search", {})
        runs[args.label] = res
        if "parent" in runs and "branch" in runs:
            runs["comparison"] = compare(runs["parent"]["shapes"], runs["branch"]["shapes"])
    else:
        res["lib"] = lib
        grouped(args, res)
        out.update(res)
    finish(args, out)


if __name__ == "__main__":
    main()
