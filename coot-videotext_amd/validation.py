"""Validation of the retrieval trainer (coot/trainer_retrieval.py:312-477, metric part and embedding export): ONE function for
one process and for the ranks of a data-parallel run.  A validation that is not sharded is the one-rank case of the sharded one:
it runs the same body over a stand-in context whose collectives are the identity (_OneRank), so the two cannot drift apart."""
from __future__ import annotations

import contextlib
import os
from typing import Any, Dict, List

import numpy as np
import torch

from . import loss_fn
from .retrieval import compute_retrieval_device, retrieval_topk_device, strip_bounds


class _OneRank:
    """The context of a validation that is not sharded: one rank, every collective the identity."""
    world, rank = 1, 0

    def exchange_shapes(self, values):
        return [list(values)]

    def gather_rows_nograd(self, x, counts):
        return x

    def all_reduce_sum(self, t):
        return None


@contextlib.contextmanager
def _global_max_hook_set_aside(model_mgr):
    hook, model_mgr.global_max_fn = model_mgr.global_max_fn, None
    try:
        yield
    finally:
        model_mgr.global_max_fn = hook


@torch.no_grad()
def validate_epoch(trainer, data_loader, val_clips, save_embs, save_path, topk, sharded):
    """RetrievalTrainer.validate_epoch (its docstring has the options and the returned dictionary), written once over a context
    ``ctx`` of W ranks: ``trainer.dp`` when the work is split over its ranks (``sharded`` resolves true and it has more than one),
    otherwise _OneRank — no attribute of ``trainer.dp`` beyond ``world`` is touched then and no collective is entered.
    The returned dictionary is the one a single rank computes, bit for bit, and the same on every rank (check_is_new_best, the
    plateau scheduler and early stopping decide alike everywhere).
    EVERY RANK IS GIVEN THE SAME LOADER: the same batches in the same order, the same length.  Rank r encodes the batches
    at positions ≡ r (mod W) (shard_batch_indices).  A batch is never split: its embeddings and losses are the ones a
    single rank computes (avg_special pools over the batch's own padding), and when sharding the eval encode takes no part in the
    step's global-max collective (the model manager's hook is set aside for the loop and put back) — ranks hold different
    batches, and len(loader) % W may be non-zero.  Every collective comes after the loop, the same sequence on every rank:
      one exchange of host integers (rows per batch), one gather of the per-video sets, one of the per-clip sets and one of
      the per-batch losses, each put back into loader order by an index permutation on the device
      (loader_order_permutation);
      per retrieval level one integer all-reduce of the [2, N] rank counts of this rank's strip of rows
      (retrieval.compute_retrieval_device(dp=));
      ``topk``: this rank's strip of queries against the whole gallery, the [n, k] results gathered;
      ``save_embs``: the gathered arrays; only rank 0 writes ``save_path``, the others return the same dictionary without
      ``embeddings_file``.
    The cycle-consistency loss draws its positions from the trainer's generator: for a batch another rank encodes, the draws
    are made and dropped, so the generator moves as it does on one rank."""
    dp = getattr(trainer, "dp", None)
    if sharded is None:
        sharded = dp is not None and dp.world > 1
    if sharded:
        assert dp is not None, "validate_epoch(sharded=True) needs a data-parallel context (self.dp)"
    sharding = bool(sharded) and dp.world > 1
    ctx = dp if sharding else _OneRank()
    W, R = ctx.world, ctx.rank
    mgr = trainer.model_mgr
    trainer.join_streams()
    mgr.set_all_models_eval()
    keys = ["vid_emb", "par_emb", "clip_emb", "sent_emb"] + (["vid_context", "par_context"] if save_embs else [])
    high_keys, low_keys = [k for k in keys if k[:3] in ("vid", "par")], ["clip_emb", "sent_emb"]  # one row per video / per clip
    high, low, losses, save_clip_num, save_key, mine = [], [], [], [], [], []
    use_cc = float(trainer.cfg.train.loss_cycle_cons) != 0
    # (the hook is a per-batch collective: not inside a loop in which the ranks hold different batches)
    with _global_max_hook_set_aside(mgr) if sharding else contextlib.nullcontext():
        n_batches = 0
        for pos, batch in enumerate(data_loader):
            n_batches += 1
            if save_embs:
                save_clip_num.append(batch.clip_num)
                save_key.extend(batch.key)
            if pos % W != R:
                if use_cc:  # the two draws of compute_cyclecons_loss, dropped
                    loss_fn.sample_cycle_indices(batch.clip_num, trainer.cc_generator)
                    loss_fn.sample_cycle_indices(batch.sent_num, trainer.cc_generator)
                continue
            visual_data = mgr.encode_visual(batch)
            text_data = mgr.encode_text(batch)
            contr = trainer.compute_total_constrastive_loss(visual_data, text_data)
            cc = trainer.compute_cyclecons_loss(visual_data, text_data)
            losses.append((contr + cc).float().reshape(1, 1))
            both = {**visual_data.__dict__, **text_data.__dict__}
            high.append(torch.cat([both[k].float() for k in high_keys], dim=1))
            low.append(torch.cat([both[k].float() for k in low_keys], dim=1))
            mine.append(pos)
    assert mine == shard_batch_indices(n_batches, W, R)
    dev = torch.device("cuda", torch.cuda.current_device())
    # ---- rows per batch and the widths of the packed sets (a rank without a batch learns them here): host integers ----------
    per, nk = (n_batches + W - 1) // W, len(keys)
    msg = [n_batches] + [both[k].shape[1] if mine else 0 for k in keys]
    for q in range(per):
        msg += [high[q].shape[0], low[q].shape[0]] if q < len(mine) else [0, 0]
    got = ctx.exchange_shapes(msg)
    assert all(g[0] == n_batches for g in got), f"sharded validation: the ranks' loaders differ in length ({[g[0] for g in got]})"
    width = {k: max(g[1 + i] for g in got) for i, k in enumerate(keys)}
    dh, dl = sum(width[k] for k in high_keys), sum(width[k] for k in low_keys)
    vid_rows, clip_rows = [0] * n_batches, [0] * n_batches
    for r in range(W):
        for q, b in enumerate(shard_batch_indices(n_batches, W, r)):
            vid_rows[b], clip_rows[b] = got[r][1 + nk + 2 * q], got[r][2 + nk + 2 * q]
    none = lambda w: [torch.zeros(0, w, dtype=torch.float32, device=dev)]  # a rank that encoded no batch
    high_all = gather_in_loader_order(ctx, torch.cat(high or none(dh), 0), vid_rows)
    low_all = gather_in_loader_order(ctx, torch.cat(low or none(dl), 0), clip_rows)
    loss_all = gather_in_loader_order(ctx, torch.cat(losses or none(1), 0), [1] * n_batches)
    data = {}
    for packed, ks in ((high_all, high_keys), (low_all, low_keys)):
        c = 0
        for k in ks:
            data[k] = packed[:, c:c + width[k]].contiguous()
            c += width[k]
    # ---- metrics: this rank's strip of rows, one integer all-reduce per level ---------------------------------------------------
    # The reference moves every batch to the host, normalises there (manual L2 without eps, :397-402) and ranks with one
    # numpy argsort per row (nntrainer/retrieval.py:68-98).  Here the embeddings never leave the GPU: normalisation,
    # similarities, ranks and the metric dictionaries are libcoot_hip.so kernels (coot_retrieval_ranks_part).
    v2p, p2v, vp_sum = compute_retrieval_device(data["vid_emb"], data["par_emb"], normalize=True, dp=ctx)
    out = {"v2p": v2p, "p2v": p2v, "val_score_at_1": vp_sum}
    if val_clips:
        c2s, s2c, cs_sum = compute_retrieval_device(data["clip_emb"], data["sent_emb"], normalize=True, dp=ctx)
        out.update({"c2s": c2s, "s2c": s2c, "val_clip_sent_score_at_1": cs_sum})
    out["loss"] = float(loss_all.reshape(-1).mean())
    if topk is not None:
        pairs = [("v2p", "vid_emb", "par_emb"), ("p2v", "par_emb", "vid_emb")]
        if val_clips:
            pairs += [("c2s", "clip_emb", "sent_emb"), ("s2c", "sent_emb", "clip_emb")]
        out["topk"] = {}
        for name, q, g in pairs:
            n = data[q].shape[0]
            bounds = [strip_bounds(n, W, r) for r in range(W)]
            row0, rows = bounds[R]
            if rows:
                idx, sc = retrieval_topk_device(data[q][row0:row0 + rows], data[g], topk, normalize=True)[:2]
            else:
                idx, sc = (torch.zeros(0, topk, dtype=t, device=dev) for t in (torch.int32, torch.float32))
            cnt = [b[1] for b in bounds]
            # one D2H copy per array
            out["topk"][name] = (ctx.gather_rows_nograd(idx, cnt).cpu().numpy(), ctx.gather_rows_nograd(sc, cnt).cpu().numpy())
    if save_embs:
        clip_num = torch.cat(save_clip_num).cpu().numpy()
        emb: Dict[str, Any] = {"clip_num": clip_num, "sent_num": clip_num.copy(), "key": list(save_key)}
        for k in keys:  # one D2H copy per tensor, after the last batch (the reference copies every batch of every key)
            x = data[k]
            emb[k] = (x / (x * x).sum(dim=-1).sqrt().unsqueeze(-1)).cpu().numpy()
            emb[f"{k}_before_norm"] = x.cpu().numpy()
        out["embeddings"] = emb
        if save_path is not None and R == 0:
            out["embeddings_file"] = save_embeddings(emb, save_path)
    return out


def shard_batch_indices(n_batches: int, world: int, rank: int) -> List[int]:
    """The loader positions rank encodes in a sharded validation: those ≡ rank (mod world).  Whole batches only."""
    return list(range(int(rank), int(n_batches), int(world)))


def loader_order_permutation(rows_per_batch, world: int) -> np.ndarray:
    """rows_per_batch[b]: the rows batch b contributes (loader order).  Returns the int64 index vector p with
    gathered[p] = the rows in loader order, where ``gathered`` is the rank-major concatenation an all-gather delivers: rank 0's
    batches (shard_batch_indices order), then rank 1's, ..."""
    rows = [int(r) for r in rows_per_batch]
    start = [0] * len(rows)
    off = 0
    for r in range(int(world)):
        for b in shard_batch_indices(len(rows), world, r):
            start[b] = off
            off += rows[b]
    if not rows:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(start[b], start[b] + rows[b], dtype=np.int64) for b in range(len(rows))])


def gather_in_loader_order(dp, x: torch.Tensor, rows_per_batch) -> torch.Tensor:
    """x: the rows of this rank's batches (shard_batch_indices order), rows_per_batch[b]: the rows of batch b of the whole
    loader.  All-gathers the ranks' blocks (dp.gather_rows_nograd) and returns all rows in loader order, on every rank."""
    W = dp.world
    counts = [sum(int(rows_per_batch[b]) for b in shard_batch_indices(len(rows_per_batch), W, r)) for r in range(W)]
    assert x.shape[0] == counts[dp.rank], (x.shape, counts, dp.rank)
    if max(counts, default=0) == 0:
        return x
    perm = torch.from_numpy(loader_order_permutation(rows_per_batch, W)).to(x.device)
    return dp.gather_rows_nograd(x.contiguous(), counts).index_select(0, perm)


def save_embeddings(emb: Dict[str, Any], path: str) -> str:
    """Write the export dictionary of validate_epoch(save_embs=True): HDF5 with the reference's dataset names when h5py is
    importable (coot/trainer_retrieval.py:404-415), else numpy ``.npz`` with the same keys (``key`` as a unicode array)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    try:
        import h5py  # noqa: F401
    except ImportError:
        h5py = None
    base = path[:-3] if path.endswith(".h5") else (path[:-4] if path.endswith(".npz") else path)
    if h5py is not None:
        fn = base + ".h5"
        with h5py.File(fn, mode="w") as h5:
            for k, v in emb.items():
                h5[k] = v
        return fn
    fn = base + ".npz"
    np.savez(fn, **{k: (np.array(v) if k == "key" else v) for k, v in emb.items()})
    return fn
