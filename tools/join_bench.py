#!/usr/bin/env python
"""GalleryIndex.join (coot_retrieval_cross_join_count, _scan, coot_retrieval_cross_join_fill per chunk of left rows) against the route
the range search offers for the same question and against the dense formulation, in the style of tools/self_join_bench.py: HIP events
around single calls, the arms alternating call by call in one process, medians.  Right indexes of 18 000 x 384 (--calls, default 20)
and 200 000 x 768 (--calls-large, default 5); left indexes of 2 000 rows and of the right index's size; float32 x float32, bfloat16 x
bfloat16 and bfloat16 (left) x float32 (right); one threshold for all left rows, taken from the similarities of a sample of left rows
so that about 2 rows and about 0.1 % of the right index qualify per left row.  Arms:
  join                left.join(right, t, max_results=T)  (T = the exact size, known from an untimed call: no synchronisation)
  count_join          left.count_join(right, t)
  range_copy          right.search_range(left.gallery.float(), t, max_results=T): what the index offered before, the float32 copy of
                      the left rows made inside the timed call
  range1, range2      the same with the copy made beforehand (not timed), timed twice: its run-to-run spread
  dense               torch.nonzero(A[r0:r1] @ B.T >= t) in row chunks of --dense-rows, A and B = fp32 normalised copies made beforehand
                      (not timed): another chain, other bytes at the threshold
and per case torch.cuda.max_memory_allocated over one call of join, range_copy and dense (above what is resident before it).  Every
case asserts that the range search's result is the join's result byte for byte, and again under a random keep on the left rows, the
segments of the masked rows emptied.  `join_within_spread`: the join's median is not above range1/2's median by more than their spread.

    python tools/join_bench.py --out profiles/r28_cross_join.json
    python tools/join_bench.py --gallery 1 --out ...    one right index only (0: 18 000 x 384, 1: 200 000 x 768)"""
import json

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd import retrieval
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(18000, 384), (200000, 768)]
PAIRS = (("float32", "float32"), ("bfloat16", "bfloat16"), ("bfloat16", "float32"))  # (left, right)
LEFT_SMALL = 2000
SAMPLE = 512


def peak(fn):
    """Bytes allocated at the peak of one call above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - base)


def same_bytes(a, b):
    return bool(a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].shape == b[1].shape and (a[1] == b[1]).all()
                and (a[2].view(torch.int32) == b[2].view(torch.int32)).all())


def emptied(res, ask):
    """A range search (offsets, rows, scores) with the segments of the queries i with ask[i] false emptied."""
    off, rows, sc = res
    m = off.numel() - 1
    seg = torch.repeat_interleave(torch.arange(m, device=rows.device), off[1:] - off[:-1], output_size=rows.numel())
    sel = ask[seg]
    out = torch.zeros(m + 1, dtype=torch.int64, device=rows.device)
    out[1:] = torch.cumsum(torch.bincount(seg[sel], minlength=m), 0)
    return out, rows[sel], sc[sel]


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True,
                           options=("--gallery", "--calls-large", "--dense-rows"),
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    calls_large, dense_rows = int(args.calls_large or 5), int(args.dense_rows or 1024)
    res.update({"calls_large": calls_large, "dense_rows": dense_rows, "JOIN_TABLE_BYTES": retrieval.JOIN_TABLE_BYTES, "rows": []})
    for n, d in GALLERIES if args.gallery is None else [GALLERIES[int(args.gallery)]]:
        large = n >= 100000
        calls, warmup = (calls_large, min(args.warmup, 1)) if large else (args.calls, args.warmup)
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        b = torch.randn(n, d, device="cuda", generator=gen)
        a = torch.randn(n, d, device="cuda", generator=gen)
        for sl, sr in PAIRS:
            right = GalleryIndex(b, storage=getattr(torch, sr))
            unit_b = torch.nn.functional.normalize(right.gallery.float(), dim=1)  # the dense arm's copy
            for nl in (LEFT_SMALL, n):
                left = GalleryIndex(a[:nl], storage=getattr(torch, sl))
                unit_a = torch.nn.functional.normalize(left.gallery.float(), dim=1)
                flat = torch.sort((unit_a[torch.arange(SAMPLE, device="cuda") * 9710 % nl] @ unit_b.T).flatten(), descending=True)[0]
                for label, hits in (("2 rows", 2), ("0.1 %", n // 1000)):
                    t = float(flat[SAMPLE * hits - 1])
                    total = int(left.count_join(right, t).sum(dtype=torch.int64))
                    wide = left.gallery.float()
                    got = left.join(right, t)
                    assert got[1].numel() == total and same_bytes(right.search_range(wide, t), got), (n, nl, sl, sr, label)
                    ask = torch.rand(nl, device="cuda", generator=gen) < 0.5
                    assert same_bytes(emptied(right.search_range(wide, t), ask), left.join(right, t, keep=ask)), (n, nl, sl, sr, label, "keep")
                    del got, ask

                    def dense():
                        out = []
                        for r0 in range(0, nl, dense_rows):
                            out.append(torch.nonzero(unit_a[r0:r0 + dense_rows] @ unit_b.T >= t))
                        return out
                    dense_pairs = sum(p.shape[0] for p in dense())
                    ranged = lambda: right.search_range(wide, t, max_results=total)
                    arms = {"range1": ranged, "join": lambda: left.join(right, t, max_results=total), "range2": ranged,
                            "range_copy": lambda: right.search_range(left.gallery.float(), t, max_results=total),
                            "count_join": lambda: left.count_join(right, t), "dense": dense}
                    ms = alternate(arms, list(arms), calls, warmup)
                    torch.cuda.synchronize()
                    del wide
                    row = {"N_left": nl, "N_right": n, "d": d, "left": sl, "right": sr, "selectivity": label, "threshold": t, "calls": calls,
                           "pairs": total, "hits_per_left_row": round(total / nl, 2), "dense_pairs": dense_pairs,
                           "chunks": len(retrieval._cross_join_chunks(nl, n, retrieval.JOIN_TABLE_BYTES)), "range_same_bytes_as_join": True}
                    for arm in arms:
                        row[arm] = stats(ms[arm])
                    rg = float(np.median(ms["range1"] + ms["range2"]))
                    sp = spread(ms["range1"], ms["range2"])
                    mem = {"join": peak(arms["join"]), "range_copy": peak(arms["range_copy"]), "dense": peak(dense)}
                    row.update({"range_median_ms": round(rg, 4), "range_spread_ms": round(sp, 4),
                                "join_over_range": round(row["join"]["median_ms"] / rg, 3),
                                "join_over_range_copy": round(row["join"]["median_ms"] / row["range_copy"]["median_ms"], 3),
                                "join_within_spread": bool(row["join"]["median_ms"] <= rg + sp),
                                "join_over_dense": round(row["join"]["median_ms"] / row["dense"]["median_ms"], 3),
                                "peak_bytes": mem, "fp32_copy_bytes": nl * d * 4,
                                "range_table_bytes": 4 * nl * ((n + 127) // 128 + 1)})
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    finish(args, res)  # (after every case: a run that is cut short leaves what it measured)
                del left, unit_a, flat
            del right, unit_b
    finish(args, res)


if __name__ == "__main__":
    main()
