#!/usr/bin/env python
"""GalleryIndex.components (coot_retrieval_components: one sweep of the upper triangle, every hit a union) against the route a user had
for duplicate clusters, against its floor and against the dense formulation, in the style of tools/self_join_bench.py: HIP events
around single calls, the arms alternating call by call in one process, medians.  Galleries of 18 000 x 384 (--calls, default 20) and
200 000 x 768 (--calls-large, default 5); float32 and bfloat16 storage.  Cases: the two thresholds of profiles/r27_self_join.json, one
threshold for all rows taken from the similarities of a sample of rows so that about 2 rows and about 0.1 % of the gallery qualify per
row (both sides of the diagonal counted), on a random gallery; and `copies`: 5 % of the rows overwritten with copies of other rows, at
the threshold 0.999.  Arms:
  components          index.components(t)
  join_propagate (a)  index.self_join(t), then label propagation on the device in torch: the smaller label of an edge's two rows goes
                      to both (scatter_reduce amin) and labels jump to their label's label, to a fixed point (one synchronisation per
                      round).  The tool asserts that its labels are those of components.
  count_join (b)      index.count_self_join(t): the same arithmetic with nothing behind it, the floor
  dense (c)           torch.nonzero(torch.triu(U[r0:r1] @ U.T, r0 + 1) >= t) in row chunks of --dense-rows, U = an fp32 normalised copy of
                      the gallery made beforehand (not timed), then the same propagation: another chain, other bytes at the threshold
and per case torch.cuda.max_memory_allocated over one call of each arm (above what is resident before it).

    python tools/components_bench.py --out profiles/r31_components.json
    python tools/components_bench.py --trace-case 1     one case only (bfloat16, 200 000 x 768, 0.1 %), components alone, for a kernel trace"""
import json

from _retrieval_bench import alternate, finish, start, stats
import torch
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(18000, 384), (200000, 768)]
STORAGES = ("float32", "bfloat16")
SAMPLE = 512
COPIES_THRESHOLD = 0.999


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


def propagate(n, i, j):
    """Min-label propagation over the edges (i, j) to a fixed point: (labels int32 [n], rounds)."""
    lab = torch.arange(n, device=i.device)
    rounds = 0
    while True:
        rounds += 1
        m = torch.minimum(lab[i], lab[j])
        new = lab.scatter_reduce(0, i, m, "amin").scatter_reduce(0, j, m, "amin")
        new = new[new]
        if torch.equal(new, lab):  # (the synchronisation of this round)
            return lab.to(torch.int32), rounds
        lab = new


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True,
                           options=("--trace-case", "--calls-large", "--dense-rows"))
    calls_large, dense_rows = int(args.calls_large or 5), int(args.dense_rows or 1024)
    res.update({"calls_large": calls_large, "dense_rows": dense_rows, "copies_threshold": COPIES_THRESHOLD, "rows": []})
    trace = args.trace_case is not None
    for n, d in GALLERIES[1:] if trace else GALLERIES:
        large = n >= 100000
        calls, warmup = (calls_large, min(args.warmup, 1)) if large else (args.calls, args.warmup)
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        planted = g.clone()  # 5 % of the rows become copies of rows of the other 95 %
        dst = torch.randperm(n, device="cuda", generator=gen)[:n // 20]
        src = torch.randint(0, n, (n // 20,), device="cuda", generator=gen)
        src = torch.where(torch.isin(src, dst), (src + 1) % n, src)
        planted[dst] = g[src]
        for storage in ("bfloat16",) if trace else STORAGES:
            for kind in ("random",) if trace else ("random", "copies"):
                index = GalleryIndex(g if kind == "random" else planted, storage=getattr(torch, storage))
                unit = torch.nn.functional.normalize(index.gallery.float(), dim=1)  # the dense arm's copy
                if kind == "random":
                    some = torch.arange(SAMPLE, device="cuda") * 9710 % n
                    sample = unit[some] @ unit.T
                    sample[torch.arange(SAMPLE, device="cuda"), some] = -2.0  # a row is not its own partner
                    flat = torch.sort(sample.flatten(), descending=True)[0]
                    del sample
                    cases = [(label, float(flat[SAMPLE * hits - 1])) for label, hits in (("2 rows", 2), ("0.1 %", n // 1000))]
                    cases = cases[1:] if trace else cases
                    del flat
                else:
                    cases = [("copies", COPIES_THRESHOLD)]
                for label, t in cases:
                    def comp():
                        return index.components(t)

                    def join_propagate():
                        off, rows, _ = index.self_join(t)
                        i = torch.repeat_interleave(torch.arange(n, device="cuda"), off[1:] - off[:-1], output_size=rows.numel())
                        return propagate(n, i, rows.long())

                    def count_join():
                        return index.count_self_join(t)

                    def dense():
                        out = []
                        for r0 in range(0, n, dense_rows):
                            p = torch.nonzero(torch.triu(unit[r0:r0 + dense_rows] @ unit.T, r0 + 1) >= t)
                            p[:, 0] += r0
                            out.append(p)
                        p = torch.cat(out)
                        return propagate(n, p[:, 0], p[:, 1])

                    labels = comp()
                    if trace:
                        ms = alternate({"components": comp}, ["components"], calls, warmup)
                        row = {"N": n, "d": d, "storage": storage, "case": label, "threshold": t, "calls": calls, "components": stats(ms["components"])}
                        res["rows"].append(row)
                        print(json.dumps(row), flush=True)
                        continue
                    want, rounds = join_propagate()
                    assert bool((labels == want).all()), (n, d, storage, label)  # (a)'s labels are the new call's
                    pairs = int(count_join().sum(dtype=torch.int64))
                    dense_labels, dense_rounds = dense()
                    clusters = int((labels == torch.arange(n, device="cuda", dtype=torch.int32)).sum())
                    sizes = torch.bincount(labels.long(), minlength=n)
                    row = {"N": n, "d": d, "storage": storage, "case": label, "threshold": t, "calls": calls, "pairs": pairs,
                           "clusters": clusters, "rows_in_clusters_of_two_or_more": int(sizes[sizes > 1].sum()), "largest_cluster": int(sizes.max()),
                           "propagation_rounds": rounds, "dense_propagation_rounds": dense_rounds,
                           "dense_labels_equal": bool((dense_labels == labels).all())}  # (another chain: they need not be)
                    del want, dense_labels, sizes
                    arms = {"count_join": count_join, "components": comp, "join_propagate": join_propagate, "dense": dense}
                    ms = alternate(arms, list(arms), calls, warmup)
                    torch.cuda.synchronize()
                    for a in arms:
                        row[a] = stats(ms[a])
                    c = row["components"]["median_ms"]
                    row.update({"components_over_join_propagate": round(c / row["join_propagate"]["median_ms"], 3),
                                "components_over_count_join": round(c / row["count_join"]["median_ms"], 3),
                                "components_over_dense": round(c / row["dense"]["median_ms"], 3),
                                "peak_bytes": {a: peak(arms[a]) for a in arms}})
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    finish(args, res)  # (after every case: a run that is cut short leaves what it measured)
                del index, unit
    finish(args, res)


if __name__ == "__main__":
    main()
