#!/usr/bin/env python
"""GalleryIndex.search_multi (coot_retrieval_topk_multi) against what a user had before it, in the style of
tools/topk_grouped_bench.py: HIP events around single calls, the arms alternating call by call in one process, medians of --calls
calls and the spread of an arm timed twice.  K = 10; galleries of 200 000 x 768 and 18 000 x 384; float32 and bfloat16 storage; G = N /
10 groups of 10 rows, once as adjacent rows and once scattered over the gallery; P = 1, 8 and 64 paragraphs of 8 sentences.  Arms:
  multi               index.search_multi(q, offsets, 10, groups, num_groups=G)
  sweep1, sweep2      (a) index.search_grouped(q, 10, groups, num_groups=G) on the same sentences: ceil(M / 16) library calls, the same
                      sweeps without the one table, the sums and the alignment (timed twice: its run-to-run spread)
  dense               (b) the exact formulation in torch on the dense matrix: q @ g.T on the normalised fp32 gallery (made once, not
                      timed), scatter_reduce(amax) into [M, G], the sum over a paragraph's sentences, topk
  workaround          (c) the inexact one: index.search_grouped(q, 128) per sentence, combined in torch: a group counts for a paragraph
                      if it is in every sentence's list
  reset               a memset of the table's M x G x 8 bytes (torch zero_ on a buffer of that size): what the one table reset costs
and per case in how many paragraphs (c) returns another set of groups than search_multi, and whether (b) does (it adds pairwise).

    python tools/topk_multi_bench.py --out profiles/r19_topk_multi.json

--trace N,storage,paragraphs,layout (e.g. 200000,bfloat16,64,adjacent) runs that case's search_multi alone, for
`rocprofv3 --kernel-trace -- python tools/topk_multi_bench.py --trace ...` and tools/rocpd_stats.py: where the time of a call goes.

--label parent | branch runs something else, on whatever commit the tool is started from (copy the tool there): the ungrouped
index.search cases of profiles/r13_topk_few.json and index.search_grouped at M = 16, each timed twice, stored under that label in --out
next to what is already there; with both labels on file a "comparison" says whether this commit's calls are slower than the parent's
by more than the parent's own spread: the grouped search now launches its sweep through the function search_multi shares."""
import json
import os

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd.retrieval import GalleryIndex
from topk_grouped_bench import compare, ungrouped

GALLERIES = [(200000, 768), (18000, 384)]
STORAGES = ("float32", "bfloat16")
PARAGRAPHS = (1, 8, 64)
SENTENCES = 8
K = 10


def sentences(g, p_total, gen):
    """Paragraph p: 8 sentences planted on 8 consecutive gallery rows (with adjacent groups: the clips of one video)."""
    rows = (torch.arange(p_total, device="cuda")[:, None] * 9710 + torch.arange(SENTENCES, device="cuda")[None]).reshape(-1) % g.shape[0]
    return torch.randn(p_total * SENTENCES, g.shape[1], device="cuda", generator=gen) + 0.35 * g[rows]


def dense(q, gn, groups64, g_total, p_total):
    sim = torch.nn.functional.normalize(q, dim=1) @ gn.T
    best = torch.full((q.shape[0], g_total), float("-inf"), device=q.device).scatter_reduce(1, groups64.expand(q.shape[0], -1), sim, "amax")
    return best.view(p_total, SENTENCES, g_total).sum(1).topk(K, dim=1)


def combine(grp, scores, g_total, p_total):
    """The workaround: per sentence the 128 best groups; a group counts for a paragraph if every sentence lists it."""
    m = grp.shape[0]
    table = torch.full((m, g_total + 1), float("-inf"), device=grp.device)
    table.scatter_(1, torch.where(grp >= 0, grp, torch.full_like(grp, g_total)).long(), scores)
    return table[:, :g_total].view(p_total, SENTENCES, g_total).sum(1).topk(K, dim=1)


def multi(args, res):
    res["rows"] = []
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        g_total = n // 10
        adjacent = (torch.arange(n, device="cuda") // 10).to(torch.int32)
        layouts = {"adjacent": adjacent, "scattered": adjacent[torch.randperm(n, device="cuda", generator=gen)].contiguous()}
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            gn = torch.nn.functional.normalize(index.gallery.float(), dim=1)
            for p_total in PARAGRAPHS:
                q = sentences(g, p_total, gen)
                m = q.shape[0]
                offsets = np.arange(0, m + 1, SENTENCES)
                table = torch.empty(m * g_total, dtype=torch.int64, device="cuda")
                for layout, groups in layouts.items():
                    groups64 = groups.long()[None]
                    sweep = lambda: index.search_grouped(q, K, groups, num_groups=g_total)[:3]

                    def workaround():
                        grp, _, sc, _ = index.search_grouped(q, 128, groups, num_groups=g_total)
                        return combine(grp, sc, g_total, p_total)
                    arms = {"sweep1": sweep, "multi": lambda: index.search_multi(q, offsets, K, groups, num_groups=g_total)[:4], "sweep2": sweep,
                            "dense": lambda: dense(q, gn, groups64, g_total, p_total), "workaround": workaround, "reset": lambda: table.zero_()}
                    ms = alternate(arms, list(arms), args.calls, args.warmup)
                    got, exact, alt = arms["multi"](), arms["dense"](), arms["workaround"]()
                    torch.cuda.synchronize()
                    mine = got[0].long().sort(1).values
                    row = {"N": n, "d": d, "storage": storage, "paragraphs": p_total, "sentences": SENTENCES, "M": m, "groups": g_total, "layout": layout}
                    for a in arms:
                        row[a] = stats(ms[a])
                    floor = float(np.median(ms["sweep1"] + ms["sweep2"]))
                    med = row["multi"]["median_ms"]
                    row.update({"sweep_median_ms": round(floor, 4), "sweep_spread_ms": round(spread(ms["sweep1"], ms["sweep2"]), 4),
                                "multi_over_sweep": round(med / floor, 3), "multi_over_dense": round(med / row["dense"]["median_ms"], 3),
                                "multi_over_workaround": round(med / row["workaround"]["median_ms"], 3),
                                "multi_minus_sweep_ms": round(med - floor, 4),
                                "workaround_paragraphs_with_other_groups": int((alt.indices.sort(1).values != mine).any(1).sum()),
                                "dense_paragraphs_with_other_groups": int((exact.indices.sort(1).values != mine).any(1).sum()),
                                "workspace_bytes": int(res["lib"].coot_retrieval_topk_multi_workspace_bytes(p_total, m, n, d, K, g_total))})
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                del table
            del index, gn
    del res["lib"]


def trace(args):
    """--trace N,storage,paragraphs,layout: that case's search_multi alone, --warmup + --calls times, for a kernel trace."""
    n, storage, p_total, layout = args.trace.split(",")
    n, p_total = int(n), int(p_total)
    d = dict(GALLERIES)[n]
    gen = torch.Generator(device="cuda").manual_seed(n + d)
    g = torch.randn(n, d, device="cuda", generator=gen)
    groups = (torch.arange(n, device="cuda") // 10).to(torch.int32)
    if layout == "scattered":
        groups = groups[torch.randperm(n, device="cuda", generator=gen)].contiguous()
    index = GalleryIndex(g, storage=getattr(torch, storage))
    q = sentences(g, p_total, gen)
    offsets = np.arange(0, q.shape[0] + 1, SENTENCES)
    for _ in range(args.warmup + args.calls):
        index.search_multi(q, offsets, K, groups, num_groups=n // 10)
    torch.cuda.synchronize()


def grouped16(args, res):
    """index.search_grouped at M = 16, K = 10, adjacent groups of 10 rows, float32 storage, timed twice."""
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        index = GalleryIndex(g, normalize=True)
        groups = (torch.arange(n, device="cuda") // 10).to(torch.int32)
        q = sentences(g, 2, gen)
        call = lambda: index.search_grouped(q, K, groups, num_groups=n // 10)[:3]
        ms = alternate({"search1": call, "search2": call}, ["search1", "search2"], args.calls, args.warmup)
        row = {"M": 16, "N": n, "d": d, "K": K, "search1": stats(ms["search1"]), "search2": stats(ms["search2"]),
               "search_median_ms": round(float(np.median(ms["search1"] + ms["search2"])), 4), "search_spread_ms": round(spread(ms["search1"], ms["search2"]), 4)}
        res["grouped_shapes"].append(row)
        print(json.dumps(row), flush=True)


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True, options=["--label", "--trace"], K=K,
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    if args.trace:
        return trace(args)
    out = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    if args.label:
        ungrouped(args, res)
        res["grouped_shapes"] = []
        grouped16(args, res)
        runs = out.setdefault("parent_check", {})
        runs[args.label] = res
        if "parent" in runs and "branch" in runs:
            runs["comparison"] = {"search": compare(runs["parent"]["shapes"], runs["branch"]["shapes"]),
                                  "search_grouped": compare(runs["parent"]["grouped_shapes"], runs["branch"]["grouped_shapes"])}
    else:
        res["lib"] = lib
        multi(args, res)
        out.update(res)
    finish(args, out)


if __name__ == "__main__":
    main()
