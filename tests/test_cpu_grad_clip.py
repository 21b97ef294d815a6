"""Host side of the gradient norm / clipping (trainer_retrieval.GradClip; include/coot_hip.h: coot_step_set_grad_clip): how
train.clip_gradient maps onto a clipper, the clipper's checks and state_dict round trip, and the new C-ABI entry points against the
header (no GPU needed)."""
import copy
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as cva
    return cva


def _raw(cva, clip_gradient=None):
    from tests import helpers as H
    from oracle import coot_oracle as O
    cfgs = H.full_cfgs(64, 48, 64, 4, 64, 128)
    raw = dict(train=dict(batch_size=4, loss_func="contrastive", contrastive_loss_config=dict(margin=0.2, **H.ANET_W), loss_cycle_cons=0.01),
               dataset_train=dict(vid_feat_dim=64, text_feat_dim=48),
               optimizer=dict(name="adam", lr=1e-3, weight_decay=2e-5, weight_decay_for_bias=True, momentum=0.9, adam_beta2=0.999, adam_eps=1e-8))
    if clip_gradient is not None:
        raw["train"]["clip_gradient"] = clip_gradient
    for k, c in zip(H.NET_KEYS, cfgs):
        raw[k] = H.ocfg_to_dict(c, dropout=0.0)
    return raw, O


def _trainer(cva, raw, **kw):
    cfg = cva.RetrievalConfig(copy.deepcopy(raw))
    mgr = cva.RetrievalModelManager(cfg)
    return cva.RetrievalTrainer(cfg, mgr, **kw)


def test_config_clip_gradient_maps_onto_the_trainer(cva):
    from coot_videotext_amd.trainer_retrieval import GradClip
    raw, _ = _raw(cva)
    assert _trainer(cva, raw).grad_clip is None  # key absent: off
    raw, _ = _raw(cva, -1)
    assert _trainer(cva, raw).grad_clip is None  # every shipped config: off, nothing new runs
    raw, _ = _raw(cva, 0.5)
    tr = _trainer(cva, raw)
    assert isinstance(tr.grad_clip, GradClip) and tr.grad_clip.max_norm == 0.5 and not tr.grad_clip.before_update  # report-only
    assert tr.optimizer_state_dict()["grad_clip"] == {"max_norm": 0.5, "before_update": False, "clipped_steps": 0}
    mine = GradClip(2.0, before_update=True)
    assert _trainer(cva, raw, grad_clip=mine).grad_clip is mine  # an explicit clipper wins over the key
    for bad in (-2, -1.5, "1", True):
        raw, _ = _raw(cva, bad)
        with pytest.raises(ValueError):
            cva.RetrievalConfig(raw)
    for name in ("anet_coot", "yc2_100m_coot", "yc2_2d3d_coot"):  # the shipped configurations keep clipping off
        assert cva.load_named_config(name).train.clip_gradient == -1
    # enable / disable on a trainer without a GPU step yet
    raw, _ = _raw(cva)
    tr = _trainer(cva, raw)
    gc = tr.enable_grad_clipping(max_norm=3.0, before_update=True)
    assert tr.grad_clip is gc and gc.before_update and gc.max_norm == 3.0
    with pytest.raises(ValueError):
        tr.enable_grad_clipping(GradClip(1.0), max_norm=2.0)
    tr.disable_grad_clipping()
    assert tr.grad_clip is None and tr.last_grad_norm() == 0.0  # the reference's state.last_grad_norm with clipping off


def test_grad_clip_validation_and_state_dict_round_trip(cva):
    from coot_videotext_amd.trainer_retrieval import GradClip
    for bad in (-0.1, float("nan"), float("inf"), "1.0"):
        with pytest.raises(ValueError):
            GradClip(bad)
    gc = GradClip(1.5)
    assert gc.state_dict() == {"max_norm": 1.5, "before_update": False, "clipped_steps": 0}
    assert gc.norm() != gc.norm()  # NaN before any step
    want = {"max_norm": 0.25, "before_update": True, "clipped_steps": 7}
    gc.load_state_dict(want)
    assert gc.state_dict() == want and gc.before_update
    other = GradClip(9.0)
    other.load_state_dict(gc.state_dict())
    assert other.state_dict() == want
    with pytest.raises(ValueError):
        other.load_state_dict(dict(want, max_norm=-3.0))
    other.set_max_norm(4.0)
    assert other.max_norm == 4.0
    with pytest.raises(ValueError):
        other.set_max_norm(-1.0)
    # the host copy of the device block: header words in the documented order
    blk = other._ensure("cpu", 32 + 8 * 5 + 128)  # (five partials and their group ticket's line)
    v = struct.unpack(GradClip._FMT, bytes(blk[:32].numpy().tobytes()))
    assert v[0] == 4.0 and v[1] == 1 and v[4] == 7 and v[5] == 0 and v[6] == 5
    assert other.state_dict() == dict(want, max_norm=4.0)
    other.set_max_norm(0.5)  # rewrites the device word in place
    assert struct.unpack("<f", bytes(other.block[:4].numpy().tobytes()))[0] == 0.5


def test_grad_clip_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    want = {"coot_step_grad_clip_bytes": 1, "coot_step_set_grad_clip": 2, "coot_step_grad_norm": 3}
    lib = cva.lib.load()
    for name, n in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        assert (0 if args in ("", "void") else args.count(",") + 1) == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert "COOT_ABI_VERSION 7" in hdr  # new functions only: the ABI version stays
