#!/usr/bin/env python
"""The filtered top-K search (keep= of GalleryIndex.search: coot_retrieval_topk_few_masked, coot_retrieval_topk_masked) against the
unfiltered one, in the style of tools/half_bench.py: HIP events around single GalleryIndex.search calls, the arms alternating call
by call on one box, medians of --calls calls.  Shapes: 200 000 x 768 and 18 000 x 384, K = 10, M = 1, 16 (the few-query sweep) and
1 024 (fp32: the tile call; bfloat16: 64 slices of the sweep), on an fp32 and on a bfloat16 index.

Arms:
  a1, a2  keep=None on this build, timed twice per round so that its own run-to-run spread is on file
  p1, p2  (with --parent-lib) keep=None through another build of the library, e.g. the parent commit's: the same Python path, only
          the shared object differs.  The unmasked kernels are meant to be the parent's instruction for instruction, so the
          acceptance is |median(a) - median(p)| <= the parent's own spread = |median p1 - median p2| + (max - min over p1 and p2)
  ones    keep all ones: what consulting the mask costs when it filters nothing
  contig  10 % kept as one contiguous range in the middle: 90 % of the blocks are dead and are skipped
  random  10 % kept at random: almost no block of 64 / 128 rows is dead, nothing is skipped
An arm counts as faster than the unfiltered search only when it beats min(a1, a2) by more than (a)'s spread, defined as above.
Every filtered arm is checked once per shape against its definition (the unfiltered search on gallery[keep], indices mapped back).
Usage: python tools/masked_bench.py [--calls 20] [--warmup 5] [--parent-lib path/libcoot_hip.so] [--out profiles/<tag>_topk_masked.json]"""
import ctypes
import json

from _retrieval_bench import alternate, finish, same, spread, start, stats
import numpy as np
import torch
import coot_videotext_amd as cva
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768), (18000, 384)]
QUERIES = (1, 16, 1024)
K = 10
STORAGES = ("float32", "bfloat16")
SEARCH_CALLS = ("coot_retrieval_topk_workspace_bytes", "coot_retrieval_topk_masked", "coot_retrieval_topk_few_workspace_bytes",
                "coot_retrieval_topk_few_masked")  # what an unfiltered search calls (keep = NULL)


def other_build(path):
    """Another build of the library with the search calls bound as lib.load() binds them."""
    here = cva.lib.load()
    lib = ctypes.CDLL(path)
    for name in SEARCH_CALLS:
        getattr(lib, name).argtypes = getattr(here, name).argtypes
        getattr(lib, name).restype = getattr(here, name).restype
    return lib


def through(lib, fn):
    """fn() with cva.lib.load() answering lib: the wrappers' own Python path on another shared object."""
    def run():
        mine, cva.lib._lib = cva.lib._lib, lib
        try:
            return fn()
        finally:
            cva.lib._lib = mine
    return run


def definition(index, q, keep):
    """The unfiltered search on an index of gallery[keep], indices mapped back."""
    cols = torch.nonzero(keep)[:, 0]
    sub = GalleryIndex(index.gallery[keep], normalize=index.normalize)
    idx, sc, _ = sub.search(q, K)
    return cols[idx.long()].int(), sc


def main():
    args, _, res = start(timer="HIP events around one GalleryIndex.search call, arms alternating", library=True, options=["--parent-lib"], K=K,
                         spread="|median of the first timing - median of the second| + (max - min over both)", shapes=[])
    parent = other_build(args.parent_lib) if args.parent_lib else None
    res["parent_library_timed"] = parent is not None
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        keeps = {"ones": torch.ones(n, dtype=torch.bool, device="cuda"), "contig": torch.zeros(n, dtype=torch.bool, device="cuda"),
                 "random": torch.rand(n, device="cuda", generator=gen) < 0.1}
        keeps["contig"][int(0.45 * n):int(0.55 * n)] = True
        for storage in STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            for m in QUERIES:
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[torch.arange(m, device="cuda") * 7 % n]
                plain = lambda: index.search(q, K)[:2]
                arms = {"a1": plain, "a2": plain}
                for name, keep in keeps.items():
                    arms[name] = (lambda keep: lambda: index.search(q, K, keep=keep)[:2])(keep)
                order = ["a1", "ones", "contig", "random", "a2"]
                if parent is not None:
                    arms["p1"] = arms["p2"] = through(parent, plain)
                    order = ["p1"] + order + ["p2"]
                ms = alternate(arms, order, args.calls, args.warmup)
                row = {"M": m, "N": n, "d": d, "storage": storage, "kept": {k: int(v.sum()) for k, v in keeps.items()}}
                row["same_bytes_as_the_unfiltered_search_on_the_compacted_gallery"] = {k: same(arms[k](), definition(index, q, v)) for k, v in keeps.items()}
                if parent is not None:
                    row["parent_build_returns_the_same_bytes"] = same(arms["p1"](), plain())
                torch.cuda.synchronize()
                for a in order:
                    row[a] = stats(ms[a])
                a_med, a_best, a_spread = float(np.median(ms["a1"] + ms["a2"])), min(row["a1"]["median_ms"], row["a2"]["median_ms"]), spread(ms["a1"], ms["a2"])
                row["a_spread_ms"] = round(a_spread, 4)
                if parent is not None:
                    p_med, p_spread = float(np.median(ms["p1"] + ms["p2"])), spread(ms["p1"], ms["p2"])
                    row.update({"p_spread_ms": round(p_spread, 4), "a_minus_p_ms": round(a_med - p_med, 4),
                                "unfiltered_within_the_parents_spread": bool(abs(a_med - p_med) <= p_spread)})
                for name in keeps:
                    row[name + "_over_unfiltered"] = round(row[name]["median_ms"] / a_best, 3)
                    row[name + "_faster_than_unfiltered_by_more_than_its_spread"] = bool(a_best - row[name]["median_ms"] > a_spread)
                row["random_over_contig"] = round(row["random"]["median_ms"] / row["contig"]["median_ms"], 2)
                res["shapes"].append(row)
                print(json.dumps(row), flush=True)
            del index
    finish(args, res)


if __name__ == "__main__":
    main()
