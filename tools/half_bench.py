#!/usr/bin/env python
"""GalleryIndex.search on a gallery stored in bfloat16 and in IEEE half (coot_retrieval_topk_few_h) against the fp32 index
(coot_retrieval_topk_few, whose kernels are instruction for instruction the parent commit's), at the shapes of tools/few_bench.py:
M = 1, 4, 16 queries against 200 000 x 768 and 18 000 x 384, K = 10, and M = 16 with K = 128 at the large gallery.  The same timer:
HIP events around single calls, the arms alternating call by call on one box; medians.  Arms: (a) the fp32 index, timed TWICE per
round so that its own run-to-run spread is on record (a1, a2); (b) the bfloat16 index; (c) the half index.  The three indices hold
the same rows (the fp32 one the unrounded ones).  hbm_floor_ms = the bytes of one gallery sweep / 6.29 TB/s, for the fp32 and for
the 16-bit gallery; the small gallery fits the caches, so its floors are reported but prove nothing.  An arm counts as faster only
when it beats min(a1, a2) by more than (a)'s spread = |median a1 - median a2| and than its min-max range.
Usage: python tools/half_bench.py [--calls 20] [--warmup 5] [--out profiles/<tag>_topk_half.json]"""
import json

from _retrieval_bench import alternate, finish, same, start, stats
import torch
from coot_videotext_amd.retrieval import GalleryIndex, retrieval_topk_device

HBM_STREAM_BYTES_PER_S = 6.29e12
SHAPES = [(m, 200000, 768, 10) for m in (1, 4, 16)] + [(16, 200000, 768, 128)] + [(m, 18000, 384, 10) for m in (1, 4, 16)]
ARMS = ("a1_fp32_index", "b_bf16_index", "c_half_index", "a2_fp32_index")


def main():
    args, _, res = start(library=True, hbm_stream_tb_per_s=HBM_STREAM_BYTES_PER_S / 1e12, shapes=[])
    made = {}
    for m, n, d, k in SHAPES:
        if (n, d) not in made:
            made.clear()
            torch.cuda.empty_cache()
            gen = torch.Generator(device="cuda").manual_seed(n + d)
            g = torch.randn(n, d, device="cuda", generator=gen)
            made[(n, d)] = (g, GalleryIndex(g), GalleryIndex(g, storage=torch.bfloat16), GalleryIndex(g, storage=torch.float16), gen)
        g, i32, ibf, ihf, gen = made[(n, d)]
        q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * g[torch.arange(m, device="cuda") * 7 % n]
        arms = {"a1_fp32_index": lambda: i32.search(q, k)[:2], "b_bf16_index": lambda: ibf.search(q, k)[:2],
                "c_half_index": lambda: ihf.search(q, k)[:2], "a2_fp32_index": lambda: i32.search(q, k)[:2]}
        ms = alternate(arms, ARMS, args.calls, args.warmup)
        # the definition, once per shape: the 16-bit index returns the bytes of the fp32 tile call on the widened gallery
        ok = {}
        for name, idx in (("bf16", ibf), ("half", ihf)):
            want = retrieval_topk_device(q, idx.gallery.float(), k, normalize=True)[:2]
            ok[name] = same(idx.search(q, k)[:2], want)
            del want
        torch.cuda.synchronize()
        row = {"M": m, "N": n, "d": d, "K": k, "nbytes_fp32": i32.nbytes, "nbytes_16": ibf.nbytes,
               "same_bytes_as_fp32_search_on_widened_gallery": ok}
        for a in ARMS:
            row[a] = stats(ms[a])
        a1, a2, b, c = (row[x]["median_ms"] for x in ARMS[:1] + ARMS[3:] + ARMS[1:3])
        a_all = ms["a1_fp32_index"] + ms["a2_fp32_index"]
        spread, rng = abs(a1 - a2), max(a_all) - min(a_all)
        floor32, floor16 = (n * d * e / HBM_STREAM_BYTES_PER_S * 1e3 for e in (4, 2))
        row.update({"a_spread_ms": round(spread, 4), "a_range_ms": round(rng, 4),
                    "fp32_over_bf16": round(min(a1, a2) / b, 2), "fp32_over_half": round(min(a1, a2) / c, 2),
                    "bf16_faster_than_fp32_by_more_than_its_spread": bool(min(a1, a2) - b > max(spread, rng)),
                    "half_faster_than_fp32_by_more_than_its_spread": bool(min(a1, a2) - c > max(spread, rng)),
                    "hbm_floor_fp32_ms": round(floor32, 4), "hbm_floor_16_ms": round(floor16, 4),
                    "fp32_over_its_floor": round(min(a1, a2) / floor32, 2), "bf16_over_its_floor": round(b / floor16, 2),
                    "half_over_its_floor": round(c / floor16, 2)})
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    finish(args, res)


if __name__ == "__main__":
    main()
