#!/usr/bin/env python
"""GalleryIndex.knn_join / knn_graph (coot_retrieval_knn_join) against the routes the index offered for the same question, against the
same arithmetic without a selection, and against the dense formulation, in the style of tools/join_bench.py: HIP events around single
calls, the arms alternating call by call in one process, medians.  Right indexes of 18 000 x 384 (--calls, default 20) and 200 000 x
768 (--calls-large, default 5); float32 x float32 and bfloat16 x bfloat16; K = 10.  Cases per right index: the graph (the index against
itself) and the cross case with left indexes of 2 000 rows and of the right index's size.  Arms:
  knn                 index.knn_graph(k)  /  left.knn_join(right, k)
  parent (a)          graph: index.neighbors(arange(N), k);  cross: right.search(left.gallery.float(), k), the float32 copy made inside
                      the timed call — the tool asserts that (a) returns the bytes of knn
  count (b)           graph: index.count_join(index, t) (the whole square, as the graph walks it) and count_self (the triangle);
                      cross: left.count_join(right, t); t = the value at which a sample of 512 left rows has 2 partners on average:
                      the same chain and staging with no selection behind it, the floor
  dense (c)           torch.topk(A[r0:r0 + rows] @ B.T, k) in row chunks of --dense-rows, A and B = fp32 normalised copies made beforehand
                      (not timed): a matrix-pipe GEMM on another chain, other bytes
and per case torch.cuda.max_memory_allocated over one call of knn, (a) and (c) (above what is resident before it).
--sweep: instead of the arms, knn alone under coot_set_option("rt_knn_splits", S), S = 1, 2, 4, 8, 16, 32 and 0 (automatic), alternating,
for every case with fewer than 1 024 row tiles: what the split cap and the target number of workgroups are picked from.

    python tools/knn_join_bench.py --out profiles/r30_knn_join.json
    python tools/knn_join_bench.py --gallery 1 --out ...    one right index only (0: 18 000 x 384, 1: 200 000 x 768)
    python tools/knn_join_bench.py --sweep 1 --out profiles/r30_knn_join_sweep.json"""
import json

from _retrieval_bench import alternate, finish, same, start, stats
import torch
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(18000, 384), (200000, 768)]
STORAGES = ("float32", "bfloat16")
LEFT_SMALL = 2000
SAMPLE = 512
K = 10
SPLITS = (1, 2, 4, 8, 16, 32, 0)


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


def main():
    args, lib, res = start(timer="HIP events around one call, arms alternating", library=True,
                           options=("--gallery", "--calls-large", "--dense-rows", "--sweep"))
    calls_large, dense_rows, sweep = int(args.calls_large or 5), int(args.dense_rows or 1024), bool(int(args.sweep or 0))
    res.update({"calls_large": calls_large, "dense_rows": dense_rows, "K": K, "sweep": sweep, "rows": []})
    for n, d in GALLERIES if args.gallery is None else [GALLERIES[int(args.gallery)]]:
        large = n >= 100000
        calls, warmup = (calls_large, min(args.warmup, 1)) if large else (args.calls, args.warmup)
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        b = torch.randn(n, d, device="cuda", generator=gen)
        a = torch.randn(n, d, device="cuda", generator=gen)
        for storage in STORAGES:
            right = GalleryIndex(b, storage=getattr(torch, storage))
            unit_b = torch.nn.functional.normalize(right.gallery.float(), dim=1)  # the dense arm's copy
            for case, nl in (("graph", n), ("cross", LEFT_SMALL), ("cross", n)):
                graph = case == "graph"
                if sweep and (nl + 63) // 64 >= 1024:
                    continue  # (the row tiles alone fill the device: the automatic choice is one share)
                left = right if graph else GalleryIndex(a[:nl], storage=getattr(torch, storage))
                unit_a = unit_b if graph else torch.nn.functional.normalize(left.gallery.float(), dim=1)
                knn = (lambda: right.knn_graph(K)) if graph else (lambda: left.knn_join(right, K))
                row = {"case": case, "N_left": nl, "N_right": n, "d": d, "storage": storage, "K": K, "calls": calls}
                if sweep:
                    arms = {}
                    for s in SPLITS:
                        def one(s=s):
                            assert lib.coot_set_option(b"rt_knn_splits", s) == 0
                            try:
                                return knn()
                            finally:
                                assert lib.coot_set_option(b"rt_knn_splits", 0) == 0
                        arms["S=%d" % s if s else "auto"] = one
                    want = arms["S=1"]()
                    for name, arm in arms.items():
                        assert same(arm(), want), (case, nl, n, storage, name)  # the bytes do not depend on the split
                    ms = alternate(arms, list(arms), calls, warmup)
                    row.update({"row_tiles": (nl + 63) // 64, "blocks": (n + 127) // 128, "splits_same_bytes": True})
                    for arm in arms:
                        row[arm] = stats(ms[arm])
                else:
                    every = torch.arange(n, device="cuda")
                    parent = (lambda: right.neighbors(every, K)) if graph else (lambda: right.search(left.gallery.float(), K)[:2])
                    assert same(parent(), knn()), (case, nl, n, storage)
                    flat = torch.sort((unit_a[torch.arange(SAMPLE, device="cuda") * 9710 % nl] @ unit_b.T).flatten(), descending=True)[0]
                    t = float(flat[SAMPLE * 2 - 1])
                    del flat

                    def dense():
                        out = []
                        for r0 in range(0, nl, dense_rows):
                            out.append(torch.topk(unit_a[r0:r0 + dense_rows] @ unit_b.T, K + 1 if graph else K))
                        return out
                    arms = {"knn": knn, "parent": parent, "count": lambda: left.count_join(right, t), "dense": dense}
                    if graph:
                        arms["count_self"] = lambda: right.count_self_join(t)
                    ms = alternate(arms, list(arms), calls, warmup)
                    torch.cuda.synchronize()
                    for arm in arms:
                        row[arm] = stats(ms[arm])
                    row.update({"threshold": t, "count_hits_per_left_row": round(float(left.count_join(right, t).sum(dtype=torch.int64)) / nl, 2),
                                "parent_same_bytes_as_knn": True,
                                "knn_over_parent": round(row["knn"]["median_ms"] / row["parent"]["median_ms"], 3),
                                "knn_over_count": round(row["knn"]["median_ms"] / row["count"]["median_ms"], 3),
                                "knn_over_dense": round(row["knn"]["median_ms"] / row["dense"]["median_ms"], 3),
                                "peak_bytes": {"knn": peak(knn), "parent": peak(parent), "dense": peak(dense)}, "fp32_copy_bytes": nl * d * 4})
                    del every
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                finish(args, res)  # (after every case: a run that is cut short leaves what it measured)
                if not graph:
                    del left, unit_a
            del right, unit_b
    finish(args, res)


if __name__ == "__main__":
    main()
