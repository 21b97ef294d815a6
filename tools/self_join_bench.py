#!/usr/bin/env python
"""GalleryIndex.self_join (coot_retrieval_join_count, _scan, coot_retrieval_join_fill per chunk of rows) against the route the range
search offers for the same question and against the dense formulation, in the style of tools/range_tile_bench.py: HIP events around
single calls, the arms alternating call by call in one process, medians.  Galleries of 18 000 x 384 (--calls, default 20) and
200 000 x 768 (--calls-large, default 5); float32 and bfloat16 storage; one threshold for all rows, taken from the similarities of a
sample of rows so that about 2 rows and about 0.1 % of the gallery qualify per row (both sides of the diagonal counted).  Arms:
  join                index.self_join(t, max_results=T)  (T = the exact size, known from an untimed call: no synchronisation)
  count_join          index.count_self_join(t)
  range_copy          index.search_range(index.gallery.float(), t, max_results=Ta): what the index offered before, the float32 copy of
                      the gallery made inside the timed call
  range1, range2      the same with the copy made beforehand (not timed), timed twice: its run-to-run spread
  dense               torch.nonzero(torch.triu(U[r0:r1] @ U.T, r0 + 1) >= t) in row chunks of --dense-rows, U = an fp32 normalised copy of
                      the gallery made beforehand (not timed): another chain, other bytes at the threshold
and per case torch.cuda.max_memory_allocated over one call of join, range_copy and dense (above what is resident before it), and whether
the range search's result with j <= i dropped is the join's result byte for byte.  `join_wins`: the join's median lies below range1/2's
median by more than their spread.

    python tools/self_join_bench.py --out profiles/r27_self_join.json
    python tools/self_join_bench.py --trace-case 1      one case only (bfloat16, 200 000 x 768, 0.1 %), join and range1, for a kernel trace"""
import json

from _retrieval_bench import alternate, finish, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd import retrieval
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(18000, 384), (200000, 768)]
STORAGES = ("float32", "bfloat16")
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


def as_pairs(res):
    """A range search of the gallery against itself with j <= i dropped: (counts per row, rows, scores)."""
    off, rows, sc = res
    n = off.numel() - 1
    seg = torch.repeat_interleave(torch.arange(n, device=rows.device), off[1:] - off[:-1], output_size=rows.numel())
    sel = rows > seg
    return torch.bincount(seg[sel], minlength=n), rows[sel], sc[sel]


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True,
                           options=("--trace-case", "--calls-large", "--dense-rows"),
                           spread="|median of the first timing - median of the second| + (max - min over both)")
    calls_large, dense_rows = int(args.calls_large or 5), int(args.dense_rows or 1024)
    res.update({"calls_large": calls_large, "dense_rows": dense_rows, "JOIN_TABLE_BYTES": retrieval.JOIN_TABLE_BYTES, "rows": []})
    trace = args.trace_case is not None
    for n, d in GALLERIES[1:] if trace else GALLERIES:
        large = n >= 100000
        calls, warmup = (calls_large, min(args.warmup, 1)) if large else (args.calls, args.warmup)
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        for storage in ("bfloat16",) if trace else STORAGES:
            index = GalleryIndex(g, storage=getattr(torch, storage))
            unit = torch.nn.functional.normalize(index.gallery.float(), dim=1)  # the dense arm's copy
            some = torch.arange(SAMPLE, device="cuda") * 9710 % n
            sample = unit[some] @ unit.T
            sample[torch.arange(SAMPLE, device="cuda"), some] = -2.0  # a row is not its own partner
            flat = torch.sort(sample.flatten(), descending=True)[0]
            del sample
            for label, hits in (("0.1 %", n // 1000),) if trace else (("2 rows", 2), ("0.1 %", n // 1000)):
                t = float(flat[SAMPLE * hits - 1])
                total = int(index.count_self_join(t).sum(dtype=torch.int64))
                wide = index.gallery.float()
                total_range = int(index.count_range(wide, t).sum(dtype=torch.int64))
                ref = index.search_range(wide, t)
                got = index.self_join(t)
                cnt, rows, sc = as_pairs(ref)
                same = bool((torch.diff(got[0]) == cnt).all() and rows.numel() == got[1].numel() and (rows == got[1]).all()
                            and (sc.view(torch.int32) == got[2].view(torch.int32)).all())
                del ref, got, cnt, rows, sc

                def dense():
                    out = []
                    for r0 in range(0, n, dense_rows):
                        out.append(torch.nonzero(torch.triu(unit[r0:r0 + dense_rows] @ unit.T, r0 + 1) >= t))
                    return out
                dense_pairs = sum(p.shape[0] for p in dense())
                ranged = lambda: index.search_range(wide, t, max_results=total_range)
                arms = {"range1": ranged, "join": lambda: index.self_join(t, max_results=total), "range2": ranged,
                        "range_copy": lambda: index.search_range(index.gallery.float(), t, max_results=total_range),
                        "count_join": lambda: index.count_self_join(t), "dense": dense}
                if trace:
                    arms = {a: arms[a] for a in ("range1", "join")}
                ms = alternate(arms, list(arms), calls, warmup)
                torch.cuda.synchronize()
                row = {"N": n, "d": d, "storage": storage, "selectivity": label, "threshold": t, "calls": calls, "pairs": total,
                       "hits_per_row_both_sides": round(total_range / n - 1, 2), "range_hits_total": total_range, "dense_pairs": dense_pairs,
                       "chunks": len(retrieval._join_chunks(n, retrieval.JOIN_TABLE_BYTES)), "range_right_of_diagonal_same_bytes_as_join": same}
                for a in arms:
                    row[a] = stats(ms[a])
                if not trace:
                    del wide
                    rg = float(np.median(ms["range1"] + ms["range2"]))
                    sp = spread(ms["range1"], ms["range2"])
                    mem = {"join": peak(arms["join"]), "range_copy": peak(arms["range_copy"]), "dense": peak(dense)}
                    row.update({"range_median_ms": round(rg, 4), "range_spread_ms": round(sp, 4),
                                "join_over_range": round(row["join"]["median_ms"] / rg, 3),
                                "join_over_range_copy": round(row["join"]["median_ms"] / row["range_copy"]["median_ms"], 3),
                                "join_wins": bool(row["join"]["median_ms"] < rg - sp),
                                "join_over_dense": round(row["join"]["median_ms"] / row["dense"]["median_ms"], 3),
                                "peak_bytes": mem, "fp32_copy_bytes": n * d * 4,
                                "join_saves_at_least_the_copy": bool(mem["range_copy"] - mem["join"] >= n * d * 4)})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                finish(args, res)  # (after every case: a run that is cut short leaves what it measured)
            del index, unit, flat
    finish(args, res)


if __name__ == "__main__":
    main()
