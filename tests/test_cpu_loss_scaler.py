"""Host side of dynamic loss scaling (trainer_retrieval.LossScaler; include/coot_hip.h: coot_step_set_loss_scaler): the scaler's
state_dict round trip and constructor checks, and the new C-ABI entry points against the header (no GPU needed)."""
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as cva
    return cva


def test_loss_scaler_state_dict_round_trip(cva):
    from coot_videotext_amd.trainer_retrieval import LossScaler
    sc = LossScaler()
    sd = sc.state_dict()
    # torch.cuda.amp.GradScaler's defaults and state_dict keys
    assert (sd["scale"], sd["growth_factor"], sd["backoff_factor"], sd["growth_interval"], sd["_growth_tracker"]) == (65536.0, 2.0, 0.5, 2000, 0)
    assert sd["skipped_steps"] == 0 and sd["step"] is None
    want = {"scale": 1024.0, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 3, "skipped_steps": 2, "step": 41}
    sc.load_state_dict(want)
    assert sc.state_dict() == want
    other = LossScaler(init_scale=8.0)
    other.load_state_dict(sc.state_dict())
    assert other.state_dict() == want
    # a GradScaler.state_dict() (no skipped-step count, no step) loads too; the optimizer steps already taken stay
    other.load_state_dict({"scale": 32.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 100, "_growth_tracker": 9})
    assert other.state_dict()["scale"] == 32.0 and other.state_dict()["step"] == 41 and other.state_dict()["skipped_steps"] == 0
    fresh = LossScaler()
    fresh.load_state_dict({"scale": 32.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 100, "_growth_tracker": 9})
    assert fresh.state_dict()["step"] is None  # (seeded from the trainer at its first native step)
    fresh._set_step(7)
    assert fresh.state_dict()["step"] == 7
    for bad in (dict(init_scale=0.0), dict(growth_factor=0.5), dict(backoff_factor=1.5), dict(backoff_factor=0.0), dict(growth_interval=0)):
        with pytest.raises(ValueError):
            LossScaler(**bad)


def test_loss_scaler_abi_matches_the_header(cva):
    from coot_videotext_amd.trainer_retrieval import LossScaler
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    want = {"coot_step_loss_scaler_bytes": 0, "coot_step_set_loss_scaler": 1, "coot_step_unscale_grads": 3}
    lib = cva.lib.load()
    for name, n in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        assert (0 if args in ("", "void") else args.count(",") + 1) == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    # the block: the documented header words + 32 bytes of optimizer scalars
    assert lib.coot_step_loss_scaler_bytes() == struct.calcsize(LossScaler._FMT) + 32 == 80
