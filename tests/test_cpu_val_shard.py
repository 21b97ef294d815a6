"""Host side of sharded validation (include/coot_hip.h: coot_retrieval_ranks_part, coot_retrieval_metrics): the new functions
are declared, bound and exported by both builds under the unchanged ABI version; the numpy mirror of a strip adds up to the
reference's ranks over any partition; the batch sharding and the loader-order permutation are what they say; and the int32
all-reduce and the gather-and-restore path work over gloo with two and three ranks."""
import ctypes
import itertools
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_ranks_part_workspace_bytes": 2, "coot_retrieval_ranks_part": 13, "coot_retrieval_metrics": 7}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_val_shard_abi_matches_the_header(cva):
    text = open(os.path.join(ROOT, "include", "coot_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert lib.coot_retrieval_ranks_part_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    assert "STRIP CONTRACT" in text and "Neither call retains a pointer" in text
    # exports.map: every name matches a global pattern of the version script
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.search(r"global:(.*?);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S), flags=re.S).group(1).split()
    import fnmatch
    assert all(any(fnmatch.fnmatchcase(name, p) for p in pats) for name in NEW)
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7
    # the strip call needs what the whole call needs (all columns normalised, all diagonals)
    assert lib.coot_retrieval_ranks_part_workspace_bytes(4917, 768) == lib.coot_retrieval_workspace_bytes(4917, 768)


def test_device_entries_refuse_cpu_tensors(cva):
    from coot_videotext_amd.retrieval import retrieval_metrics_device, retrieval_ranks_part_device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval_ranks_part_device(torch.zeros(3, 8), torch.zeros(3, 8), 0, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval_metrics_device(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))


def test_direct_rccl_datatype_follows_the_tensor(cva):
    from coot_videotext_amd.dist import DirectRccl
    assert DirectRccl.datatype(torch.float32) == 7 and DirectRccl.datatype(torch.int32) == 2  # ncclFloat32, ncclInt32 (rccl.h)
    with pytest.raises(TypeError):
        DirectRccl.datatype(torch.float64)


# ---- strips against the whole on the host ----------------------------------------------------------------------------------------

def _tied_matrix(n, seed, diag_ties):
    """Similarities quantised to 1/8 with duplicated rows: exact ties everywhere.  diag_ties False: the diagonal sits between
    the grid points (odd multiples of 1/16), so no entry of row i or column i ties with sim[i, i] — there the reference's
    unstable argsort and the device rule agree on every row.  True: the diagonal is on the grid too (the device rule decides)."""
    rs = np.random.RandomState(seed)
    sim = (rs.randint(-8, 9, size=(n, n)) / 8.0).astype(np.float32)
    for _ in range(max(1, n // 4)):  # duplicated rows
        a, b = rs.randint(0, n, size=2)
        sim[b] = sim[a]
    if not diag_ties:
        sim[np.arange(n), np.arange(n)] = ((2 * rs.randint(-8, 8, size=n) + 1) / 16.0).astype(np.float32)
    return sim


def _partitions(n, strips, rs):
    """Cut vectors 0 = c_0 <= c_1 <= ... <= c_strips = n (equal neighbours = an empty strip): all of them where that is at
    most 1 000, else the even split, the two one-sided ones and random ones with forced empty strips."""
    total = 1
    for q in range(strips - 1):
        total = total * (n + 1 + q) // (q + 1)
    if total <= 1000:
        return [(0,) + c + (n,) for c in itertools.combinations_with_replacement(range(n + 1), strips - 1)]
    out = [tuple(np.linspace(0, n, strips + 1).astype(int)), (0,) * strips + (n,), (0,) + (n,) * strips]
    for _ in range(4):
        cuts = np.sort(rs.randint(0, n + 1, size=strips - 1))
        if strips > 2:
            cuts[rs.randint(1, strips - 1)] = cuts[0]  # at least one empty strip
            cuts = np.sort(cuts)
        out.append((0,) + tuple(int(c) for c in cuts) + (n,))
    return out


@pytest.mark.parametrize("n", [1, 5, 64, 65, 200])
def test_counts_part_sums_to_the_reference_ranks(cva, n):
    from coot_videotext_amd.retrieval import compute_retrieval_cosine, compute_retrieval_counts_part
    rs = np.random.RandomState(100 + n)
    sim = _tied_matrix(n, n, diag_ties=False)
    assert n == 1 or sum((sim[i] == sim[j]).sum() >= n - 2 for i in range(n) for j in range(i)) > 0  # duplicated rows are there
    ranks12 = compute_retrieval_cosine(sim)[2]
    ranks21 = compute_retrieval_cosine(np.ascontiguousarray(sim.T))[2]
    # the reference and the device rule agree where a row has no tie with its diagonal: here that is every row and column
    agree = [i for i in range(n) if (sim[i] == sim[i, i]).sum() == 1 and (sim[:, i] == sim[i, i]).sum() == 1]
    assert len(agree) == n
    tested = 0
    for strips in sorted({1, 2, 3, 8, n}):
        for cuts in _partitions(n, strips, rs):
            assert len(cuts) == strips + 1 and cuts[0] == 0 and cuts[-1] == n
            s12, s21 = np.zeros(n, np.int64), np.zeros(n, np.int64)
            for a, b in zip(cuts[:-1], cuts[1:]):
                c12, c21 = compute_retrieval_counts_part(sim, a, b - a)
                assert c12.dtype == np.int32 and c21.dtype == np.int32 and c12.shape == (n,) and c21.shape == (n,)
                assert not c12[:a].any() and not c12[b:].any()  # row counts only inside the strip
                if a == b:
                    assert not c12.any() and not c21.any()
                s12 += c12
                s21 += c21
            assert (s12 == ranks12).all() and (s21 == ranks21).all(), (n, cuts)
            assert len(s12) == n and len(ranks12) == n  # every row compared
            tested += 1
    assert tested >= 5 or n == 1


@pytest.mark.parametrize("n", [1, 5, 64, 65, 200])
def test_counts_part_follows_the_device_tie_rule(cva, n):
    """Ties WITH the diagonal: the rule is the reversal of a stable ascending sort (a later index is ahead), as
    tests/test_retrieval_device.py states it for the whole call."""
    from coot_videotext_amd.retrieval import compute_retrieval_counts_part, strip_bounds
    sim = _tied_matrix(n, 7 * n, diag_ties=True)
    stable = np.array([np.where(np.argsort(sim[r], kind="stable")[::-1] == r)[0][0] for r in range(n)])
    stable_t = np.array([np.where(np.argsort(sim.T[r], kind="stable")[::-1] == r)[0][0] for r in range(n)])
    assert n < 5 or sum((sim[r] == sim[r, r]).sum() > 1 for r in range(n)) > 0
    for world in (1, 2, 3, 8, n):
        bounds = [strip_bounds(n, world, r) for r in range(world)]
        assert bounds[0][0] == 0 and sum(b[1] for b in bounds) == n and all(bounds[r][0] + bounds[r][1] == bounds[r + 1][0] for r in range(world - 1))
        assert max(b[1] for b in bounds) - min(b[1] for b in bounds) <= 1 and [b[1] for b in bounds] == sorted((b[1] for b in bounds), reverse=True)
        parts = [compute_retrieval_counts_part(sim, *b) for b in bounds]
        assert (sum(p[0].astype(np.int64) for p in parts) == stable).all()
        assert (sum(p[1].astype(np.int64) for p in parts) == stable_t).all()


# ---- which rank encodes which batch, and how the gathered rows get back into loader order ---------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 5, 16])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shards_partition_the_loader_and_the_permutation_restores_it(cva, n, world):
    from coot_videotext_amd.validation import loader_order_permutation, shard_batch_indices
    shards = [shard_batch_indices(n, world, r) for r in range(world)]
    assert sorted(b for s in shards for b in s) == list(range(n))
    assert all(s == sorted(s) and all(b % world == r for b in s) for r, s in enumerate(shards))
    rs = np.random.RandomState(10 * n + world)
    rows = rs.randint(0, 5, size=n).tolist()  # ragged, an empty batch included
    loader = [np.stack([np.full(rows[b], b), np.arange(rows[b])], 1).reshape(-1, 2) for b in range(n)]
    rank_major = np.concatenate([loader[b] for s in shards for b in s] + [np.zeros((0, 2), int)])
    perm = loader_order_permutation(rows, world)
    assert perm.dtype == np.int64 and sorted(perm.tolist()) == list(range(sum(rows)))
    assert np.array_equal(rank_major[perm], np.concatenate(loader + [np.zeros((0, 2), int)]))


# ---- the collectives of sharded validation over gloo -----------------------------------------------------------------------------------

def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


ROWS = [3, 1, 4, 2, 5]  # five ragged batches: divisible by neither world size


def _worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import coot_videotext_amd  # noqa: F401  (registers the package alias)
    from coot_videotext_amd import dist as cdist
    from coot_videotext_amd.retrieval import compute_retrieval_counts_part, strip_bounds
    from coot_videotext_amd.validation import gather_in_loader_order, shard_batch_indices
    dp = cdist.DataParallelContext()
    # the rank counts: one int32 all-reduce of [2, N] is the whole, as integers
    n = 37
    sim = _tied_matrix(n, 3, diag_ties=True)
    c = torch.from_numpy(np.stack(compute_retrieval_counts_part(sim, *strip_bounds(n, world, rank))))
    assert c.dtype == torch.int32
    dp.all_reduce_sum(c)
    assert c.dtype == torch.int32
    whole = np.stack(compute_retrieval_counts_part(sim, 0, n))
    assert np.array_equal(c.numpy(), whole)
    # gather and restore: every rank ends with the loader's rows in loader order
    loader = [torch.arange(r * 3, dtype=torch.float32).view(r, 3) + 100 * b for b, r in enumerate(ROWS)]
    mine = shard_batch_indices(len(ROWS), world, rank)
    x = torch.cat([loader[b] for b in mine], 0)
    got = gather_in_loader_order(dp, x, ROWS)
    assert torch.equal(got, torch.cat(loader, 0))
    losses = torch.tensor([[0.5 + b] for b in mine], dtype=torch.float32)
    assert torch.equal(gather_in_loader_order(dp, losses, [1] * len(ROWS)).reshape(-1), torch.arange(5, dtype=torch.float32) + 0.5)
    # a loader shorter than the world: ranks without a batch send an empty block
    short = [torch.full((2, 3), 7.0)]
    xs = short[0] if rank == 0 else torch.zeros(0, 3)
    assert torch.equal(gather_in_loader_order(dp, xs, [2]), short[0])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_int32_allreduce_and_loader_order_gather_over_gloo(world):
    mp.spawn(_worker, args=(world, _free_port()), nprocs=world, join=True)
