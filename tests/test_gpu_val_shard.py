"""Sharded validation on the MI355X (coot_retrieval_ranks_part, coot_retrieval_metrics, RetrievalTrainer.validate_epoch(sharded=)).

Integer work on top of one fixed similarity chain, so everything is compared bit for bit: the strips of any partition add up to
coot_retrieval_ranks' rank vectors, the stacked similarity strips are its similarity matrix, the metrics of the summed ranks are
its 14 floats; and with REAL processes (two / three ranks sharing the one GPU through gloo, as tests/test_gpu_dp_procs.py runs
the step) every rank returns the dictionary a single process computes for the same loader."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import val_shard_worker as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _cuts(n, strips, rs):
    """Partitions of [0, n) into `strips` strips as cut vectors: the even split, and uneven ones with empty strips."""
    out = [np.linspace(0, n, strips + 1).astype(int).tolist()]
    if strips > 1:
        c = np.sort(rs.randint(0, n + 1, size=strips - 1))
        out.append([0] + c.tolist() + [n])
        c = c.copy()
        c[-1] = c[0]  # an empty strip for certain (and equal cuts when strips > n)
        out.append([0] + np.sort(c).tolist() + [n])
    return out


def _check_strips(torch, e1, e2, normalize, rs, strip_counts=(1, 2, 3, 8, 64)):
    from coot_videotext_amd.retrieval import retrieval_metrics_device, retrieval_ranks_device, retrieval_ranks_part_device
    n = e1.shape[0]
    r12, r21, met, sim = retrieval_ranks_device(e1, e2, normalize=normalize, want_sim=True)
    lib = __import__("coot_videotext_amd").lib
    ws_bytes = lib.load().coot_retrieval_ranks_part_workspace_bytes(n, e1.shape[1])
    for strips in strip_counts:
        for cuts in _cuts(n, strips, rs):
            total = torch.zeros(2, n, dtype=torch.int32, device="cuda")
            sims = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                counts, s = retrieval_ranks_part_device(e1, e2, a, b - a, normalize=normalize, want_sim=True)
                assert counts.dtype == torch.int32 and counts.shape == (2, n) and s.shape == (b - a, n)
                assert not counts[0, :a].any() and not counts[0, b:].any()
                if a == b:
                    assert not counts.any()
                total += counts
                sims.append(s)
            assert torch.equal(total[0], r12) and torch.equal(total[1], r21), (n, normalize, cuts)
            assert torch.equal(torch.cat(sims, 0), sim), (n, normalize, cuts)
            assert torch.equal(retrieval_metrics_device(total[0], total[1]), met), (n, normalize, cuts)
    # the call zeroes its outputs itself: poisoned buffers, an uneven strip, nothing left over
    a, rows = n // 3, n - n // 3 - n // 4
    want, _ = retrieval_ranks_part_device(e1, e2, a, rows, normalize=normalize)
    c12 = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c21 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    a1, a2 = e1.contiguous(), e2.contiguous()
    lib.check(lib.load().coot_retrieval_ranks_part(a1.data_ptr(), a2.data_ptr(), n, e1.shape[1], int(normalize), a, rows, c12.data_ptr(), c21.data_ptr(),
                                                   None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "coot_retrieval_ranks_part")
    assert torch.equal(c12, want[0]) and torch.equal(c21, want[1])
    assert int(c12.max()) < n and int(c21.min()) >= 0
    # ... and the metrics call its histogram
    m = torch.full((14,), float("nan"), device="cuda")
    lib.check(lib.load().coot_retrieval_metrics(r12.data_ptr(), r21.data_ptr(), n, m.data_ptr(), ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream), "coot_retrieval_metrics")
    assert torch.equal(m.view(2, 7), met)


def test_strips_on_the_golden_matrices(env, golden_dir):
    """emb2 = identity makes the similarity matrix exactly the reference-written matrix d (case 1 has forced exact ties)."""
    torch, cva = env
    g = np.load(os.path.join(golden_dir, "retrieval_metrics.npz"))
    rs = np.random.RandomState(0)
    for i in range(3):
        d = torch.from_numpy(g[f"d{i}"].astype(np.float32)).cuda()
        _check_strips(torch, d, torch.eye(len(d), device="cuda"), False, rs)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4917])
def test_strips_add_up_to_the_whole(env, n, dim, normalize):
    """Planted-match random embeddings, and a quantised set with duplicated rows: sums of small integers / 8 are exact in fp32, so
    equal rows give exactly equal similarities — ties with the diagonal and between columns in every strip."""
    torch, cva = env
    rs = np.random.RandomState(n + dim + int(normalize))
    e1 = rs.randn(n, dim).astype(np.float32)
    e2 = (0.35 * e1 + rs.randn(n, dim)).astype(np.float32)
    _check_strips(torch, torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda(), normalize, rs)
    q1 = (rs.randint(-2, 3, size=(n, dim)) / 8.0).astype(np.float32)
    q1[:, 0] = 0.125  # (no zero row: the normalisation has no eps)
    q2 = q1.copy()
    for _ in range(max(1, n // 3)):  # duplicated rows: whole groups of exactly tied columns and rows
        a, b = rs.randint(0, n, size=2)
        q1[b], q2[b] = q1[a], q2[a]
    _check_strips(torch, torch.from_numpy(q1).cuda(), torch.from_numpy(q2).cuda(), normalize, rs, strip_counts=(2, 3, 64) if n > 1000 else (1, 2, 3, 8, 64))
    if n > 1:
        r12 = cva.retrieval.retrieval_ranks_device(torch.from_numpy(q1).cuda(), torch.from_numpy(q2).cuda(), normalize=normalize)[0]
        assert int(r12.max()) > 0  # the ties were counted (a later duplicate is ahead)


# ---- validate_epoch: real processes ------------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _run_ranks(world, tmp_path, timing=0):
    port = _free_port()
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "val_shard_worker.py"), str(r), str(world), str(port), outs[r],
                               str(tmp_path), str(timing)], cwd=ROOT) for r in range(world)]
    try:
        rcs = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world, rcs
    return [dict(np.load(o)) for o in outs]


@pytest.fixture(scope="module")
def single(env, tmp_path_factory):
    """validate_epoch of one process without a data-parallel context: what every rank must return."""
    tr = W.trainer()
    out = W.validate(tr, W.loader(), str(tmp_path_factory.mktemp("single") / "emb.npz"))
    assert "embeddings_file" in out
    return W.flatten(out)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_validation_real_processes_equal_one_process(env, single, tmp_path, world):
    res = _run_ranks(world, tmp_path)
    n_vid, n_clip = sum(len(c) for c in W.COUNTS), sum(sum(c) for c in W.COUNTS)
    assert single["emb.vid_emb"].shape[0] == n_vid and single["emb.clip_emb"].shape[0] == n_clip
    assert single["topk.v2p.idx"].shape == (n_vid, W.TOPK) and single["topk.c2s.score"].shape == (n_clip, W.TOPK)
    assert single["emb.key"].tolist() == [f"vid{i}_{j}" for i, c in enumerate(W.COUNTS) for j in range(len(c))]
    for r, out in enumerate(res):
        assert int(out.pop("has_file")) == int(r == 0) and int(out.pop("file_exists")) == int(r == 0), r  # only rank 0 writes
        want = dict(single)
        want.pop("has_file")
        assert out["keys"].tolist() == [k for k in want["keys"].tolist() if r == 0 or k != "embeddings_file"]
        out.pop("keys"), want.pop("keys")
        assert set(out) == set(want), (r, set(out) ^ set(want))
        diff = [k for k in want if not (out[k].shape == want[k].shape and out[k].dtype == want[k].dtype and np.array_equal(out[k], want[k]))]
        assert not diff, (r, world, diff, [(k, out[k], want[k]) for k in diff if want[k].ndim == 0])


class _NoCollectives:
    """A data-parallel context of two ranks on which every collective raises."""
    world, rank, group = 2, 0, None

    def __getattr__(self, name):
        raise AssertionError(f"validate_epoch(sharded=False) entered a collective: {name}")


def test_replicated_validation_enters_no_collective(env, single, tmp_path):
    tr = W.trainer()
    tr.dp = _NoCollectives()
    out = W.flatten(W.validate(tr, W.loader(), str(tmp_path / "a.npz"), sharded=False))
    assert set(out) == set(single) and all(np.array_equal(out[k], single[k]) for k in single)
    with pytest.raises(AssertionError, match="entered a collective"):
        W.validate(tr, W.loader(), str(tmp_path / "b.npz"))  # sharded=None: a context with two ranks shards
    tr.dp = None  # no context: sharded=None is the replicated path
    out = W.flatten(W.validate(tr, W.loader(), str(tmp_path / "c.npz")))
    assert all(np.array_equal(out[k], single[k]) for k in single)
    with pytest.raises(AssertionError, match="needs a data-parallel context"):
        W.validate(tr, W.loader(), str(tmp_path / "d.npz"), sharded=True)

    class OneRank(_NoCollectives):  # a context of one rank has nothing to shard over: sharded=True reads ``world`` and nothing else
        world = 1

    tr.dp = OneRank()
    out = W.flatten(W.validate(tr, W.loader(), str(tmp_path / "e.npz"), sharded=True))
    assert set(out) == set(single) and all(np.array_equal(out[k], single[k]) for k in single)


def test_global_max_hook_is_not_entered_by_sharded_validation(env):
    """The model manager's data-parallel hook (a per-batch collective) is set aside inside the sharded loop and put back."""
    tr = W.trainer()

    def hook(v):
        raise AssertionError("global max collective inside the validation loop")

    tr.dp, tr.model_mgr.global_max_fn = _NoCollectives(), hook  # the loop runs, the first collective after it raises
    with pytest.raises(AssertionError, match="entered a collective: exchange_shapes"):
        tr.validate_epoch(W.loader(), True, False, None, None)
    assert tr.model_mgr.global_max_fn is hook
