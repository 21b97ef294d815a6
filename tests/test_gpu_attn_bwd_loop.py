"""The switches of the short attention backward against the kernel as it was (attn_bwd_loop=0, attn_bwd_share=0: one workgroup per
(sequence, head), every lane hashes its own dropout masks): dq, dk and dv must be BYTE-equal on the same inputs with
  attn_bwd_share=1  two of a phase-B tile's four mask hashes come from the neighbouring lane, phase A hashes per key pair (default)
  attn_bwd_loop=1   a fixed grid of workgroups loops over the items with the next item's loads in flight (default 0)
and with both.  The switches rearrange loads and share hashes and do nothing else, so there is no tolerance; the per-element tests
of tests/test_gpu_attn.py hold the kernels to the fp64 reference.

The loop runs every case at the automatic grid (all of these launches have fewer items than it, so every workgroup takes one item)
and with the grid forced to 8 workgroups through the test-only option attn_bwd_grid: a workgroup then takes every head of its
sequences, 8 to 16 items, so the two prefetch halves alternate many times, items of both segments and of different lengths follow
each other in one workgroup, and the padding ids of a ragged last group of 8 sequences end a workgroup's list.

The whole output images are compared, guard rows, column gaps and the rows between packed sequences included, and the images must
have changed from their sentinel fill (a launch that wrote nothing would compare equal).
"""
import ctypes as C

import numpy as np
import pytest

from tests import attn_cases as A

pytestmark = pytest.mark.gpu


def _cases():
    cs = []
    for p in (0.0, 0.1):
        d = "-drop" if p else ""
        # head size 48, 8 heads: 9 sequences (the last group of 8 is ragged), 3 sequences, one sequence (8 items)
        cs.append(A._case(f"loop-L80-n9{d}", Lk=80, H=8, dh=48, lens=[80, 1, 37, 79, 64, 80, 16, 17, 48], p=p))
        cs.append(A._case(f"loop-L80-n3{d}", Lk=80, H=8, dh=48, lens=[80, 79, 33], p=p))
        cs.append(A._case(f"loop-L80-n1{d}", Lk=80, H=8, dh=48, lens=[80], p=p))
        # nvalid of 1, L - 1 and L in one launch
        cs.append(A._case(f"loop-nvalid{d}", Lk=80, H=8, dh=48, lens=[1, 79, 80], p=p))
        # packed rows
        cs.append(A._case(f"loop-packed{d}", Lk=128, H=8, dh=48, lens=[1, 16, 17, 80, 128], packed=True, p=p))
        # the other head sizes at one, four and eight waves
        for dh in (16, 32, 64):
            for L in (16, 64, 128):
                cs.append(A._case(f"loop-dh{dh}-L{L}{d}", Lk=L, H=2, dh=dh, lens=[L, 1, max(1, L - 1)], p=p))
    # two segments, 5 x 80 rows then 3 x 16, with dropout: the second segment's seed delta (and, without dropout, its geometry)
    cs.append(A._case("loop-seg2-drop", Lk=80, L2=16, H=8, dh=48, lens=[80, 1, 37, 79, 64], lens2=[16, 1, 15], p=0.1))
    cs.append(A._case("loop-seg2", Lk=80, L2=16, H=8, dh=48, lens=[80, 1, 37, 79, 64], lens2=[16, 1, 15]))
    cs.append(A._case("loop-seg2-packed-drop", Lk=80, L2=16, H=8, dh=48, lens=[80, 1, 37, 79, 64], lens2=[16, 1, 15], packed=True, p=0.1))
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
OUT_BUFS = ("dqkv",)


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    lib = cva.lib.load()
    if cva.lib.operand() != "bf16":
        pytest.skip("the cases round their operands to bf16")
    return torch, cva, lib


def _up(torch, a):
    return torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.int32)).cuda()


class _Launch:
    """Device images of one case and its descriptor; forward run once (o, lse), backward on demand."""

    def __init__(self, env, c):
        torch, cva, lib = env
        self.env, self.c = env, c
        self.host = A.buffers(c, A.attn_inputs(c))
        self.dev = {k: _up(torch, v) for k, v in self.host.items()}
        L, sq = A.layout(c), A.sequences(c)
        a = cva.lib.AttnArgs(Nseq=c["Nseq"], Lq=c["Lq"], Lk=c["Lk"], H=c["H"], dh=c["dh"], Nseq2=c["Nseq2"], L2=c["L2"],
                             p=c["p"], seed=c["seed"], site=A.SITE)
        for x, (fp, fl) in dict(q=("q", "ldq"), k=("k", "ldk"), v=("v", "ldv"), o=("o", "ldo"), dout=("dout", "lddo"), dq=("dq", "lddq"),
                                dk=("dk", "lddk"), dv=("dv", "lddv")).items():
            off, ld = A.operand_offset(c, x)
            setattr(a, fp, self.dev[L["ops"][x][0]].data_ptr() + 2 * off)
            setattr(a, fl, ld)
        a.lse = self.dev["lse"].data_ptr() + 4 * A.GUARD * c["H"]
        self.keep = [torch.tensor(c["lens"], dtype=torch.int64, device="cuda"), torch.empty(L["Tq"] * c["H"] + 64, dtype=torch.float32, device="cuda")]
        a.lens, a.delta = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        if c["Nseq2"]:
            self.keep.append(torch.tensor(c["lens2"], dtype=torch.int64, device="cuda"))
            a.lens2 = self.keep[-1].data_ptr()
        if c["packed"]:
            self.keep.append(torch.tensor([s["kr0"] for s in sq], dtype=torch.int32, device="cuda"))
            a.cu = self.keep[-1].data_ptr()
        self.a = a
        self._call(False)
        self.fresh = {k: self.dev[k].clone() for k in OUT_BUFS}

    def _call(self, backward):
        torch, cva, lib = self.env
        cva.lib.check(lib.coot_debug_attn(C.byref(self.a), int(backward), torch.cuda.current_stream().cuda_stream), "debug_attn")
        torch.cuda.synchronize()

    def backward(self, loop, share, grid):
        """Bytes of the output images after one backward launch from sentinel-filled outputs."""
        torch, cva, lib = self.env
        new = dict(attn_bwd_loop=loop, attn_bwd_share=share, attn_bwd_grid=grid)
        old = {k: cva.lib.get_option(k) for k in new}
        for k in OUT_BUFS:
            self.dev[k].copy_(self.fresh[k])
        try:
            for k, v in new.items():
                cva.lib.check(lib.coot_set_option(k.encode(), v))
            self._call(True)
        finally:
            for k, v in old.items():
                lib.coot_set_option(k.encode(), v)
        return {k: self.dev[k].cpu().numpy().tobytes() for k in OUT_BUFS}


_LAUNCHES = {}


def _launch(env, name):
    """One launch object and its reference bytes (attn_bwd_loop=0, attn_bwd_share=0) per case, shared by the parameters of the case."""
    if name not in _LAUNCHES:
        ln = _Launch(env, BY_NAME[name])
        ref = ln.backward(0, 0, 0)
        for k in OUT_BUFS:
            assert ref[k] != ln.fresh[k].cpu().numpy().tobytes(), "the reference launch wrote nothing"
        _LAUNCHES[name] = (ln, ref)
    return _LAUNCHES[name]


def test_defaults(env):
    """Shared hashes on; the loop off (it is slower in the train step: DESIGN.md §8); automatic grid."""
    get = env[1].lib.get_option
    assert (get("attn_bwd_loop"), get("attn_bwd_share"), get("attn_bwd_grid")) == (0, 1, 0)


# (loop, share, grid): without the loop there is no grid to force
@pytest.mark.parametrize("loop,share,grid", [(1, 1, 0), (1, 1, 8), (1, 0, 0), (1, 0, 8), (0, 1, 0)])
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_bytes_equal(env, name, loop, share, grid):
    """dq, dk, dv (the whole dq | dk | dv image) of the setting, byte for byte those of attn_bwd_loop=0, attn_bwd_share=0."""
    ln, ref = _launch(env, name)
    got = ln.backward(loop, share, grid)
    for k in OUT_BUFS:
        assert got[k] == ref[k], f"{name}: {k} differs between loop={loop} share={share} (grid {grid}) and the kernel as it was"


@pytest.mark.parametrize("grid", [0, 8, 16])
def test_loop_twice_same_bytes(env, grid):
    """The same launch twice on the same inputs: a missing barrier between the items of a workgroup shows up as a difference."""
    ln, ref = _launch(env, "loop-L80-n3-drop")
    first, second = ln.backward(1, 1, grid), ln.backward(1, 1, grid)
    for k in OUT_BUFS:
        assert first[k] == second[k] == ref[k]
