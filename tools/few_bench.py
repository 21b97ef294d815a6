#!/usr/bin/env python
"""The few-query search on a prepared gallery (GalleryIndex.search -> coot_retrieval_topk_few) against the call that served this
case before it, retrieval_topk_device(..., normalize=True), for M = 1, 4, 16 queries against 200 000 x 768 and 18 000 x 384,
K = 10, and M = 16 with K = 128 at the large gallery.  HIP events around single calls, the arms alternating call by call on one
box; medians.  Arms: (a) the tile call, timed TWICE per round so that its own run-to-run spread is on record (a1, a2);
(b) GalleryIndex.search with the norms prepared once; (c) torch.topk(q @ g.T, k) on rows normalised beforehand, for context only
(not the chain the ranks are counted on).  hbm_floor_ms = the bytes of one gallery sweep / 6.29 TB/s (the streaming-copy rate of
the microarchitecture notes); the small gallery (27.6 MB) fits the caches, so its floor is reported but proves nothing.
Acceptance is (b) against (a): faster by more than (a)'s spread = |median a1 - median a2|, and than its min-max range.
Usage: python tools/few_bench.py [--calls 20] [--warmup 5] [--out profiles/<tag>_topk_few.json]"""
import json

from _retrieval_bench import alternate, finish, same, start, stats
import torch
from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device

HBM_STREAM_BYTES_PER_S = 6.29e12
SHAPES = [(m, 200000, 768, 10) for m in (1, 4, 16)] + [(16, 200000, 768, 128)] + [(m, 18000, 384, 10) for m in (1, 4, 16)]


def main():
    args, lib, res = start(hbm_stream_tb_per_s=HBM_STREAM_BYTES_PER_S / 1e12, shapes=[])
    made = {}
    for m, n, d, k in SHAPES:
        if (n, d) not in made:
            made.clear()
            torch.cuda.empty_cache()
            gen = torch.Generator(device="cuda").manual_seed(n + d)
            g = torch.randn(n, d, device="cuda", generator=gen)
            made[(n, d)] = (g, GalleryIndex(g, normalize=True), g / (g * g).sum(-1, keepdim=True).sqrt(), gen)
        g, index, g_unit, gen = made[(n, d)]
        q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[torch.arange(m, device="cuda") * 7 % n]
        q_unit = q / (q * q).sum(-1, keepdim=True).sqrt()
        arms = {"a1_retrieval_topk_device": lambda: retrieval_topk_device(q, g, k, normalize=True)[:2],
                "b_gallery_index_search": lambda: index.search(q, k)[:2],
                "a2_retrieval_topk_device": lambda: retrieval_topk_device(q, g, k, normalize=True)[:2],
                "c_torch_matmul_topk": lambda: torch.topk(q_unit @ g_unit.T, k)}
        ms = alternate(arms, list(arms), args.calls, args.warmup)
        want, got = arms["a1_retrieval_topk_device"](), arms["b_gallery_index_search"]()
        torch.cuda.synchronize()
        row = {"M": m, "N": n, "d": d, "K": k, "workspace_bytes": int(lib.coot_retrieval_topk_few_workspace_bytes(m, n, d, k)),
               "gallery_bytes": n * d * 4, "same_bytes_as_retrieval_topk_device": same(want, got)}
        for a, v in ms.items():
            row[a] = stats(v)
        a1, a2, b = (row[x]["median_ms"] for x in ("a1_retrieval_topk_device", "a2_retrieval_topk_device", "b_gallery_index_search"))
        floor = n * d * 4 / HBM_STREAM_BYTES_PER_S * 1e3
        a_all = ms["a1_retrieval_topk_device"] + ms["a2_retrieval_topk_device"]
        row.update({"a_spread_ms": round(abs(a1 - a2), 4), "a_range_ms": round(max(a_all) - min(a_all), 4), "a_over_b": round(min(a1, a2) / b, 2),
                    "b_faster_than_a_by_more_than_its_spread": bool(min(a1, a2) - b > max(abs(a1 - a2), max(a_all) - min(a_all))),
                    "hbm_floor_ms": round(floor, 4), "b_over_hbm_floor": round(b / floor, 2)})
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    finish(args, res)


if __name__ == "__main__":
    main()
