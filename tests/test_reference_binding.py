"""The drop-in boundary against what the reference's own RetrievalModelManager exposes, as
recorded from it by oracle/gen_golden.py (tests/golden/manager_contract.json: state-dict entries, get_all_params, the TransformerConfig
objects it hands each network): the HIP networks load the reference's state strictly and keep the BaseModelManager contract
(get_all_params names and decay_mult, get / set_model_state incl. the legacy renames), and the config adapter of
coot_videotext_amd.integration maps the reference's config objects to the kernels' fields.  The two constructor flags of the
reference's ContrastiveLoss that no configuration reaches are pinned by tests/golden/contrastive_flags.npz.

No GPU: the parameter layout is host code of the library."""
import copy
import json
import os
import types

import numpy as np
import pytest


def _namespace(d):
    """A recorded config object (nested attribute dicts) back as an object with those attributes."""
    if isinstance(d, dict):
        return types.SimpleNamespace(**{k: _namespace(v) for k, v in d.items()})
    return d


def test_hip_manager_keeps_the_reference_manager_contract(golden_dir):
    import torch
    import coot_videotext_amd as cva
    from coot_videotext_amd import integration
    from coot_videotext_amd.nets import TransformerHip
    with open(os.path.join(golden_dir, "manager_contract.json")) as f:
        rec = json.load(f)
    torch.manual_seed(0)
    hip_mgr = cva.RetrievalModelManager(cva.load_named_config("anet_coot"))
    assert list(hip_mgr.model_dict) == list(rec["state"])
    assert all(isinstance(m, TransformerHip) for m in hip_mgr.model_dict.values())
    # the adapter: the reference's config OBJECT (transformer_legacy.py:26-97) -> the fields the kernels take
    ref_cfgs = {net: _namespace(c) for net, c in rec["model_cfgs"].items()}
    for c in ref_cfgs.values():  # what `-o net_video_local.name=transformer_hip,...` does
        c.name = integration.HIP_NAME
    c = integration.hip_config_from_reference(ref_cfgs["net_video_global"], 384)
    assert (c.hidden_dim, c.num_heads, c.ff_dim, c.use_context, c.use_input_fc, c.pooler, c.dropout, c.ctx_dropout) == \
        (384, 8, 384, True, False, "avg_special", 0.025, 0.025)
    c = integration.hip_config_from_reference(ref_cfgs["net_text_local"], 1536)
    assert (c.input_dim, c.pooler, c.pool_hidden, c.pool_heads, c.pool_dropout) == (1536, "atn", 768, 2, 0.025)

    # 1. state dicts: a state with the reference's entries and shapes loads STRICTLY (load_state_dict default) and round-trips
    g = torch.Generator().manual_seed(1)
    state = {net: {k: (torch.randn(shape, generator=g) if dt == "float32" else torch.zeros(shape, dtype=getattr(torch, dt)))
                   for k, shape, dt in entries} for net, entries in rec["state"].items()}
    assert not hip_mgr.was_loaded
    hip_mgr.set_model_state(copy.deepcopy(state))
    assert hip_mgr.was_loaded
    back = hip_mgr.get_model_state()
    for net in state:
        assert sorted(back[net].keys()) == sorted(state[net].keys()), net  # same entries (buffers included); the order is the module tree's
        for k in state[net]:
            assert torch.equal(back[net][k].cpu(), state[net][k]), (net, k)
    # ... with the "module." prefix of nn.DataParallel checkpoints too (utils_torch.edit_moduledot_in_state_keys)
    hip_mgr.set_model_state({net: {"module." + k: v for k, v in sd.items()} for net, sd in state.items()})

    # 2. legacy checkpoints of the first coot-videotext release: a LIST of state dicts with the old parameter names
    #    (model_manager_base.py:96-113 renames input_norm. / input_fc. / pooler.genpool)
    inverse = [("norm_input.", "input_norm."), ("input_fc.mlp.", "input_fc."), ("pooler.pools.0.genpool", "pooler.genpool")]
    legacy = []
    for net in state:
        sd = {}
        for k, v in state[net].items():
            for new, old in inverse:
                k = k.replace(new, old)
            sd[k] = v + 1.0  # different values, so that the load is visible
        legacy.append(sd)
    assert any("input_norm." in k for k in legacy[0]) and any("pooler.genpool" in k for k in legacy[0])
    hip_mgr.set_model_state(legacy)
    for net in state:
        for k, v in hip_mgr.model_dict[net].state_dict().items():
            assert torch.equal(v.cpu(), state[net][k] + 1.0), (net, k)

    # 3. optimizer-facing contract.  The reference's get_all_params (get_params_opt_simple) lists EVERY named parameter of the four
    #    networks — 118, the two requires_grad=False pooler.pools.0.genpool_one included — with decay_mult 0 for biases
    #    (weight_decay_for_bias); the drop-in route (integration.reference_manager_class) inherits that method, so over the HIP networks
    #    it returns exactly this list: names, count, shapes, order and decay_mult are checked in full.  This package's own manager
    #    differs from the reference on purpose (model_retrieval.py: get_all_params): it leaves the non-trainable parameters out (116),
    #    so its list is the trainable subset of the reference's, with the reference's decay_mult.
    ref = rec["all_params"]
    named = [(k, v) for m in hip_mgr.model_dict.values() for k, v in m.named_parameters()]
    assert [k for k, _ in named] == ref["names"] and len(named) == len(ref["shapes"]) == 118
    assert [list(v.shape) for _, v in named] == ref["shapes"]
    wd_bias = hip_mgr.cfg.optimizer.weight_decay_for_bias
    assert [0.0 if (wd_bias and "bias" in k) else 1.0 for k, _ in named] == ref["decay_mult"]
    trainable = [i for i, (_, v) in enumerate(named) if v.requires_grad]
    assert len(trainable) == 116 and all("genpool_one" in ref["names"][i] for i in range(118) if i not in trainable)
    p_hip, n_hip, f_hip = hip_mgr.get_all_params()
    assert n_hip == [ref["names"][i] for i in trainable]
    assert [p["decay_mult"] for p in p_hip] == [ref["decay_mult"][i] for i in trainable]
    assert sum(int(np.prod(t.shape)) for t in f_hip if t.requires_grad) == 7604224
    # 4. train / eval switches reach the networks
    hip_mgr.set_all_models_eval()
    assert not hip_mgr.is_train and not any(m.training for m in hip_mgr.model_dict.values())
    hip_mgr.set_all_models_train()
    assert hip_mgr.is_train and all(m.training for m in hip_mgr.model_dict.values())


def test_own_manager_loads_legacy_list_checkpoints():
    """The standalone RetrievalModelManager honours the same legacy renames (weak point of round 1: only 'module.' was stripped)."""
    import torch
    import coot_videotext_amd as cva
    mgr = cva.RetrievalModelManager(cva.load_named_config("anet_coot"))
    state = {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in mgr.model_dict.items()}
    inverse = [("norm_input.", "input_norm."), ("input_fc.mlp.", "input_fc."), ("pooler.pools.0.genpool", "pooler.genpool")]
    legacy = []
    for net in state:
        sd = {}
        for k, v in state[net].items():
            for new, old in inverse:
                k = k.replace(new, old)
            sd["module." + k] = v * 0.5
        legacy.append(sd)
    mgr.set_model_state(legacy)
    for net in state:
        for k, v in mgr.model_dict[net].state_dict().items():
            assert torch.equal(v, state[net][k] * 0.5), (net, k)


@pytest.mark.parametrize("max_violation,norm", [(True, True), (False, False), (True, False)])
def test_contrastive_loss_constructor_flags_match_the_reference_module(golden_dir, max_violation, norm):
    """ContrastiveLoss(margin, max_violation, norm) (coot/loss_fn.py:51-100): the two constructor flags no configuration reaches — the
    hardest negative per query only, the un-normalised sum — against the reference's module on the same normalised embeddings: loss and
    gradients wrt both inputs (tests/golden/contrastive_flags.npz).  (The default flags are the fused HIP loss, pinned on the GPU by
    test_losses_vs_oracle and the fixtures.)"""
    import torch
    import coot_videotext_amd as cva
    fx = np.load(os.path.join(golden_dir, "contrastive_flags.npz"))
    tag = f"{int(max_violation)}{int(norm)}"
    lr, gar, gbr = float(fx["loss_" + tag]), torch.from_numpy(fx["grad_im_" + tag]), torch.from_numpy(fx["grad_s_" + tag])
    a, b = torch.from_numpy(fx["im"]).requires_grad_(True), torch.from_numpy(fx["s"]).requires_grad_(True)
    loss = cva.ContrastiveLoss(0.2, max_violation=max_violation, norm=norm, use_cuda=False)(a, b)
    loss.backward()
    lo, gao, gbo = float(loss), a.grad, b.grad
    assert lr > 0 and abs(lr - lo) <= 1e-6 * abs(lr)
    assert torch.allclose(gar, gao, rtol=1e-5, atol=1e-7) and torch.allclose(gbr, gbo, rtol=1e-5, atol=1e-7)
