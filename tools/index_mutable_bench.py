#!/usr/bin/env python
"""A gallery index that changes (GalleryIndex.add / update / compact: coot_retrieval_rows_put) against what there was before it, a new
index on the changed rows, in the style of tools/masked_bench.py: HIP events around single calls, the arms alternating call by call
on one box, medians of --calls calls.  Galleries 200 000 x 768 and 18 000 x 384, held in float32 and in bfloat16; R = 1, 1 000 and
10 % of N new or changed rows, given in float32.

Arms, per (gallery, storage, R):
  a         add(rows) into spare capacity: one put launch, O(R d) bytes.  One index with room for every call of the run; N grows by R
            per call (the put does not depend on N)
  b         add(rows) on an index without spare rows (built for every call, untimed, on the stored gallery by reference): the buffer
            is allocated at twice the size, the N rows are copied, then the put
  c         update(R distinct random rows, a device tensor) on an index that owns its buffer
  d_add     the same end state as (a) and (b) without add: GalleryIndex(torch.cat([gallery, rows]), storage=...) on the float32 rows
            (a bfloat16 index does not keep them: the caller has to)
  d_update  the same end state as (c) without update: the R rows written into the caller's float32 gallery in place, then
            GalleryIndex(gallery, storage=...)
Per (gallery, storage):
  e         compact() after remove() of a random half (index and removal rebuilt for every call, untimed), against
            e_parent = GalleryIndex(stored_gallery[keep]); both synchronise (the kept count is needed on the host)
  search    K = 10, M = 1 and 16, on an index grown from 90 % of the rows by add (g) and on a fresh index on the same rows, timed
            twice per round (f1, f2).  Same kernels, same bytes: |median g - median f| is reported next to the fresh index's own
            spread = |median f1 - median f2| + (max - min over f1 and f2), and the results are checked to be the same bytes.
The timer brackets the whole Python call, allocation included: what a caller waits for on an otherwise idle stream.
Usage: python tools/index_mutable_bench.py [--calls 20] [--warmup 5] [--out profiles/<tag>_index_mutable.json]"""
import json

from _retrieval_bench import alternate as run, finish, same, spread, start, stats
import numpy as np
import torch
from coot_videotext_amd.retrieval import GalleryIndex

GALLERIES = [(200000, 768), (18000, 384)]
STORAGES = ("float32", "bfloat16")
QUERIES = (1, 16)
K = 10


def same_index(a, b):
    """Gallery and norms of two indexes, as integers."""
    it = torch.int32 if a.gallery.element_size() == 4 else torch.int16
    return (a.gallery.shape == b.gallery.shape and bool((a.gallery.view(it) == b.gallery.view(it)).all())
            and bool((a.norms.view(torch.int32) == b.norms.view(torch.int32)).all()))


def main():
    args, _, res = start(timer="HIP events around one Python call (allocation included), arms alternating", library=True, K=K,
                         spread="|median of the first timing - median of the second| + (max - min over both)", changes=[], compact=[], search=[])
    rounds = args.calls + args.warmup
    for n, d in GALLERIES:
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n + d)
        g = torch.randn(n, d, device="cuda", generator=gen)
        for storage in STORAGES:
            sdt = getattr(torch, storage)
            stored = g.to(sdt)  # what an index of this storage holds (float32: the tensor itself)
            es = stored.element_size()
            for r in (1, 1000, n // 10):
                rows = torch.randn(r, d, device="cuda", generator=gen)
                which = torch.randperm(n, device="cuda", generator=gen)[:r].int()
                roomy = GalleryIndex(stored, capacity=n + r * (rounds + 1))
                owned = GalleryIndex(stored, capacity=n)
                mine = g.clone()  # the caller's float32 gallery, which d_update patches

                def d_update():
                    mine[which.long()] = rows
                    return GalleryIndex(mine, storage=sdt)
                arms = {"a": (None, lambda: roomy.add(rows)),
                        "b": (lambda: GalleryIndex(stored), lambda index: index.add(rows)),
                        "c": (None, lambda: owned.update(which, rows)),
                        "d_add": (None, lambda: GalleryIndex(torch.cat([g, rows]), storage=sdt)),
                        "d_update": (None, d_update)}
                order = ["a", "b", "c", "d_add", "d_update"]
                ms = run(arms, order, args.calls, args.warmup)
                # the end states are the same bytes
                grown = GalleryIndex(stored)
                grown.add(rows)
                patched = GalleryIndex(stored.clone())
                patched.update(which, rows)
                row = {"N": n, "d": d, "storage": storage, "R": r,
                       "add_is_the_rebuilt_index": same_index(grown, GalleryIndex(torch.cat([stored.float(), rows]), storage=sdt)),
                       "update_is_the_rebuilt_index": same_index(patched, d_update()),
                       "bytes_a_writes": r * d * es + 4 * r, "bytes_a_reads": r * d * 4,
                       "bytes_d_add_writes_at_least": (n + r) * d * 4 + ((n + r) * d * es if es == 2 else 0) + 4 * (n + r)}
                torch.cuda.synchronize()
                for a in order:
                    row[a] = stats(ms[a])
                for a, ref in (("a", "d_add"), ("b", "d_add"), ("c", "d_update")):
                    row[f"{ref}_over_{a}"] = round(row[ref]["median_ms"] / row[a]["median_ms"], 2)
                    row[f"{a}_faster_than_{ref}"] = bool(row[a]["median_ms"] < row[ref]["median_ms"])
                res["changes"].append(row)
                print(json.dumps(row), flush=True)
                del roomy, owned, grown, patched, mine
                torch.cuda.empty_cache()
            # compact after removing a random half
            keep = torch.rand(n, device="cuda", generator=gen) < 0.5
            gone = torch.nonzero(~keep)[:, 0]

            def removed():
                index = GalleryIndex(stored)
                index.remove(gone)
                return index
            ms = run({"e": (removed, lambda index: index.compact()), "e_parent": (None, lambda: GalleryIndex(stored[keep]))}, ["e", "e_parent"],
                     args.calls, args.warmup)
            index = removed()
            old = index.compact()
            row = {"N": n, "d": d, "storage": storage, "kept": int(keep.sum()), "e": stats(ms["e"]), "e_parent": stats(ms["e_parent"]),
                   "compact_is_the_rebuilt_index": same_index(index, GalleryIndex(stored[keep])) and bool((old == torch.nonzero(keep)[:, 0]).all())}
            row["e_parent_over_e"] = round(row["e_parent"]["median_ms"] / row["e"]["median_ms"], 2)
            res["compact"].append(row)
            print(json.dumps(row), flush=True)
            del index
            # search on a grown index against a fresh one on the same rows
            n0 = n - n // 10
            grown = GalleryIndex(stored[:n0].clone())
            grown.add(stored[n0:])
            fresh = GalleryIndex(stored)
            for m in QUERIES:
                q = torch.randn(m, d, device="cuda", generator=gen) + 0.35 * stored[torch.arange(m, device="cuda") * 7 % n].float()
                f, gr = (lambda: fresh.search(q, K)[:2]), (lambda: grown.search(q, K)[:2])
                ms = run({"f1": (None, f), "g": (None, gr), "f2": (None, f)}, ["f1", "g", "f2"], args.calls, args.warmup)
                f_med, f_spread = float(np.median(ms["f1"] + ms["f2"])), spread(ms["f1"], ms["f2"])
                row = {"M": m, "N": n, "d": d, "storage": storage, "grown_from": n0, "same_bytes": same(f(), gr()) and same_index(grown, fresh),
                       "f1": stats(ms["f1"]), "g": stats(ms["g"]), "f2": stats(ms["f2"]), "f_spread_ms": round(f_spread, 4),
                       "g_minus_f_ms": round(float(np.median(ms["g"])) - f_med, 4)}
                row["grown_within_the_fresh_index_spread"] = bool(abs(row["g_minus_f_ms"]) <= f_spread)
                res["search"].append(row)
                print(json.dumps(row), flush=True)
            del grown, fresh, stored
    finish(args, res)


if __name__ == "__main__":
    main()
