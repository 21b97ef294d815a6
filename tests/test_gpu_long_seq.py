"""The networks at sequence lengths above 128 rows (they accept up to 1000: csrc/api.hip, coot_net_fwd), where the attention dispatch
changes (csrc/attention.hip: attn_fwd_t / attn_bwd_t; csrc/api.hip: attention_all):

  self-attention, L <= 128         attn_short_fwd / attn_short_bwd (one workgroup per sequence and head)
  self-attention, L >= 129         attn_fwd_kernel; attn_bwd_kernel = dQ tiles and dK / dV tiles in one launch, the key tiles recompute delta
  two segments, either L > 128     one launch per segment, with row offsets into q / k / v / o, lse and delta, and a per-segment dropout seed
  context attention (Lq = 1)       attn_q1 up to 64 keys, above that the chunked kernels with a one-row query tile
  global networks                  one launch up to 32 items per sequence, the per-op kernels above

A paragraph is the concatenation of its sentences' words (dataset_retrieval.py), so real text batches have Lp > 128; every other test
that checks a gradient stops at L <= 80 (global networks: <= 32 against the per-op path).  Packed rows end at 128: a batch with a longer
sequence runs in the padded layout, whatever `packed=` says.

What is checked, per case (inputs, E and K: tests/long_seq_cases.py):
  * forward: pooled rows cosine > 1 - 1e-3 against the fp64 oracle, rel. error < 2e-2 against the bf16-emulating oracle (tokens 3e-2);
  * every parameter gradient against the fp64 oracle: helpers.grad_report, cosine > 0.999 and norm within 1.5 % (the bounds
    test_gpu_train_parity.py justifies);
  * row by row (helpers.row_report), the gradient wrt the input rows — and wrt the hidden state of a context network — within K * E of
    the fp64 oracle: one wrong tile, mask edge or segment offset makes single rows wrong by O(1), which a flat cosine does not see.

Measured on the MI355X, worst row error e_gpu / E per case (E from the oracle alone, about 1 %):
  local_dh16_L128      control  E = 0.00820   e_gpu = 0.00948   e_gpu / E = 1.16
  local_dh32_L128      control  E = 0.00859   e_gpu = 0.01242   e_gpu / E = 1.45
  local_dh48_L128      control  E = 0.00818   e_gpu = 0.01068   e_gpu / E = 1.31
  local_dh64_L128      control  E = 0.00739   e_gpu = 0.01023   e_gpu / E = 1.38
  local_dh32_L40       control  E = 0.00847   e_gpu = 0.01164   e_gpu / E = 1.37
  local_dh64_L40       control  E = 0.00742   e_gpu = 0.00945   e_gpu / E = 1.27
  small_global_L32     control  E = 0.00879   e_gpu = 0.01254   e_gpu / E = 1.43
  anet_global_L32      control  E = 0.00632   e_gpu = 0.00829   e_gpu / E = 1.31
  local_dh16_L129      long     E = 0.00865   e_gpu = 0.01055   e_gpu / E = 1.22
  local_dh16_L192      long     E = 0.00877   e_gpu = 0.01076   e_gpu / E = 1.23
  local_dh16_L200      long     E = 0.01158   e_gpu = 0.01206   e_gpu / E = 1.04
  local_dh32_L129      long     E = 0.01058   e_gpu = 0.01201   e_gpu / E = 1.13
  local_dh32_L192      long     E = 0.01040   e_gpu = 0.01091   e_gpu / E = 1.05
  local_dh32_L200      long     E = 0.00969   e_gpu = 0.01097   e_gpu / E = 1.13
  local_dh48_L129      long     E = 0.00763   e_gpu = 0.00967   e_gpu / E = 1.27
  local_dh48_L192      long     E = 0.00946   e_gpu = 0.01020   e_gpu / E = 1.08
  local_dh48_L200      long     E = 0.00926   e_gpu = 0.01032   e_gpu / E = 1.11
  local_dh64_L129      long     E = 0.00734   e_gpu = 0.00981   e_gpu / E = 1.34
  local_dh64_L192      long     E = 0.01158   e_gpu = 0.00911   e_gpu / E = 0.79
  local_dh64_L200      long     E = 0.00734   e_gpu = 0.00942   e_gpu / E = 1.28
  small_global_L33     long     E = 0.00925   e_gpu = 0.01803   e_gpu / E = 1.95
  small_global_L64     long     E = 0.00847   e_gpu = 0.01080   e_gpu / E = 1.27
  small_global_L65     long     E = 0.01409   e_gpu = 0.02563   e_gpu / E = 1.82
  small_global_L128    long     E = 0.00857   e_gpu = 0.01139   e_gpu / E = 1.33
  small_global_L129    long     E = 0.01429   e_gpu = 0.01648   e_gpu / E = 1.15
  anet_global_L33      long     E = 0.00875   e_gpu = 0.01000   e_gpu / E = 1.14
  anet_global_L65      long     E = 0.00940   e_gpu = 0.01089   e_gpu / E = 1.16
  anet_global_L130     long     E = 0.00978   e_gpu = 0.01487   e_gpu / E = 1.52
Worst control ratio 1.45: K = 2 x 1.45 rounded up to a power of two = 4.  Worst long-path ratio 1.95.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import coot_oracle as O
from tests import helpers as H
from tests import long_seq_cases as LC
from tests import test_gpu_train_parity as TP
from tests.test_gpu_bench_parity import _case, _check_embeddings, _check_grads

pytestmark = pytest.mark.gpu

GRAD_COS_MIN, GRAD_NORM_TOL = 0.999, 0.015


@pytest.fixture(scope="module")
def env():
    import torch
    import coot_videotext_amd as cva
    assert torch.cuda.is_available()
    cva.lib.load()
    return torch, cva


def _run_net(torch, cfg, P, x, lens, hid, R):
    """One TransformerHip call + backward of sum(pooled * R): pooled, tokens, parameter gradients, dfeats (networks without input FC), dhidden."""
    net = H.make_hip_net(cfg, P).eval()
    xt = torch.from_numpy(x).float().cuda().requires_grad_(not cfg.use_input_fc)
    ht = torch.from_numpy(hid).float().cuda().requires_grad_(True) if hid is not None else None
    L = x.shape[1]
    mask = torch.from_numpy(np.arange(L)[None, :] >= lens[:, None]).cuda()
    pooled, tok = net(xt, mask, torch.from_numpy(lens).cuda(), ht)
    (pooled * torch.from_numpy(R).float().cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in net.named_parameters() if p.requires_grad}
    return (pooled.detach().cpu().numpy(), tok.detach().cpu().numpy(), grads, xt.grad.cpu().numpy() if not cfg.use_input_fc else None,
            ht.grad.cpu().numpy() if ht is not None else None)


def _check_forward(tag, pooled, pooled_exact, pooled_emu, tok=None, tok_emu=None):
    cos = H.cosine_rows(pooled, pooled_exact).min()
    err = H.rel_err(pooled, pooled_emu)
    err_tok = H.rel_err(tok, tok_emu) if tok is not None else 0.0
    print(f"[{tag}] pooled: cos vs fp64 oracle {cos:.6f}, rel err vs bf16-emulating oracle {err:.2e}, tokens {err_tok:.2e}")
    assert cos > 1 - 1e-3, cos
    assert err < 2e-2 and err_tok < 3e-2, (err, err_tok)


def _describe(rows_by_tensor, L):
    """offending rows as (sequence, row, 64-row tile)"""
    out = {}
    for k, rows in rows_by_tensor.items():
        out[k] = [(int(r) // L, int(r) % L, (int(r) % L) // 64) for r in rows[:12]] if k == "dfeats" else [int(r) for r in rows]
    return out


@pytest.mark.parametrize("name", LC.CONTROLS + LC.LONG)
def test_single_segment_rows_against_the_oracle(env, name):
    torch, cva = env
    c = LC.oracle_case(name)
    cfg, N, L, control = LC.SINGLE[name]
    pooled, tok, grads, dx, dh = _run_net(torch, cfg, c["P"], c["x"], c["lens"], c["hid"], c["R"])
    valid = c["valid"]
    _check_forward(name, pooled, c["pooled"], c["pooled_e"], tok[valid], c["tok_e"][valid])
    bound = LC.K * c["E"]
    e, bad, _ = LC.worst_row_error(dx, dh, c["dx"], c["dhid"], c["lens"], bound)
    print(f"[{name}] {'control' if control else 'long'}: E = {c['E']:.5f}  worst row error {e:.5f}  ratio e / E = {e / c['E']:.2f}  (bound K = {LC.K})")
    bad_p, table = H.grad_report(list(grads.items()), c["G"], cos_min=GRAD_COS_MIN, ratio_tol=GRAD_NORM_TOL)
    if bad_p:
        print(f"[{name}] parameter gradients:\n{table}")
    assert e <= bound, (e, bound, _describe(bad, L))
    assert not bad_p, "\n".join(bad_p)


@pytest.mark.parametrize("dh", sorted(LC.LOCAL_NOFC))
def test_repadding_across_the_dispatch_boundary_changes_nothing(env, dh):
    """The same sequences at L = 128 (short kernels) and re-padded to L = 144 with unchanged lengths (chunked kernels, third tile fully
    masked): pooled outputs and gradients agree within the packed-against-padded bounds of test_gpu_varlen.py."""
    torch, cva = env
    name = f"local_dh{dh}_L128"
    c = LC.oracle_case(name)
    cfg = c["cfg"]
    p0, t0, g0, dx0, _ = _run_net(torch, cfg, c["P"], c["x"], c["lens"], None, c["R"])
    p1, t1, g1, dx1, _ = _run_net(torch, cfg, c["P"], LC.repad(c["x"], 144), c["lens"], None, c["R"])
    ep = H.rel_err(p1, p0)
    print(f"[{name}] L = 144 against L = 128: pooled rel err {ep:.2e}")
    assert ep < 2e-3
    bad, table = H.grad_report([(n, g) for n, g in g1.items() if "key_projection.bias" not in n], g0, cos_min=0.999, ratio_tol=0.01)
    assert not bad, "\n".join(bad)
    # row by row the two runs may differ by what each may differ from the oracle, K * E (measured: 1.0 ... 1.25 E), not by a lost tile
    e, rows, _ = H.row_report(dx1[:, :128], dx0, c["valid"], LC.K * c["E"])
    print(f"[{name}] L = 144 against L = 128: worst dfeats row {e:.5f} (E = {c['E']:.5f})")
    assert rows.size == 0, (e, _describe({"dfeats": rows}, 128))
    assert np.isfinite(dx1).all()


PAIRS = {"small_long_first": (LC.SMALL_LOCAL, 2, 144, 5, 16), "small_long_second": (LC.SMALL_LOCAL, 5, 16, 2, 130),
         "text_1152_tokens": (LC.TEXT_LOCAL, 4, 144, 36, 16)}
_pair_cache = {}


def _pair(name):
    """Inputs of a two-segment case and the oracle's answer (each segment through O.net_fwd / O.net_bwd, the parameter gradients added)."""
    if name not in _pair_cache:
        cfg, N1, L1, N2, L2 = PAIRS[name]
        P = O.make_params(cfg, LC.PARAM_SEED)
        segs, pooled, pooled_e, G = [], [], [], {}
        for i, (N, L) in enumerate(((N1, L1), (N2, L2))):
            x, lens, _, R = LC.make_inputs(cfg, N, L, LC.INPUT_SEED + 100 * i + L)
            po, _, cache = O.net_fwd(P, cfg, x, lens)
            pe, _, _ = O.net_fwd(P, cfg, x, lens, None, O.BF16)
            Gs, _, _ = O.net_bwd(P, cfg, R, cache)
            for k, v in Gs.items():
                G[k] = G.get(k, 0) + v
            segs.append((x, lens, R))
            pooled.append(po)
            pooled_e.append(pe)
        _pair_cache[name] = (cfg, P, segs, np.concatenate(pooled), np.concatenate(pooled_e), G)
    return _pair_cache[name]


def _run_pair(torch, cva, cfg, P, segs, packed):
    lib = cva.lib.load()
    (x1, l1, R1), (x2, l2, R2) = segs
    net = H.make_hip_net(cfg, P).eval()
    t1, t2 = torch.from_numpy(x1).float().cuda(), torch.from_numpy(x2).float().cuda()
    pk = None
    if packed:
        pk = cva.packed_index(torch.from_numpy(l1), torch.from_numpy(l2))
        pk = (pk[0].cuda(), pk[1])
    lib.coot_timing_enable(1)
    try:
        a, b = net.forward_pair(t1, torch.from_numpy(l1).cuda(), t2, torch.from_numpy(l2).cuda(), seed=99, packed=pk)
        torch.cuda.synchronize()
        ms, by, nl = C.c_double(), C.c_double(), C.c_int()
        cva.lib.check(lib.coot_timing_collect(7, C.byref(ms), C.byref(by), C.byref(nl)), "timing_collect")
    finally:
        lib.coot_timing_enable(0)
    rows = int(round(by.value / (6.0 * cfg.input_dim)))  # the input LayerNorm reports 6 bytes per element it touches
    pooled = torch.cat([a, b], 0)
    (pooled * torch.from_numpy(np.concatenate([R1, R2])).float().cuda()).sum().backward()
    torch.cuda.synchronize()
    return pooled.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.requires_grad}, rows


@pytest.mark.parametrize("name", list(PAIRS))
def test_two_segments_one_of_them_long(env, name):
    """forward_pair with one segment above 128 rows: the per-segment attention launches at their row offsets (the long segment first, and
    at a non-zero offset).  The d = 384 case has 1152 tokens: the fused chains run, with the attention as launches of their own — and
    with `packed=` given the call must fall back to the padded layout and give what the unpacked call gives."""
    torch, cva = env
    cfg, P, segs, pooled_o, pooled_e, G = _pair(name)
    _, N1, L1, N2, L2 = PAIRS[name]
    assert max(L1, L2) > 128 and any(1 in s[1] for s in segs) and any(l % 64 == 0 for s in segs for l in s[1] if l >= 64)
    n0 = cva.lib.get_option("fused_attn_launches")
    pooled, grads, rows = _run_pair(torch, cva, cfg, P, segs, packed=False)
    assert rows == N1 * L1 + N2 * L2
    _check_forward(name, pooled.cpu().numpy(), pooled_o, pooled_e)
    bad, table = H.grad_report([(n, g.cpu().numpy()) for n, g in grads.items()], G, cos_min=GRAD_COS_MIN, ratio_tol=GRAD_NORM_TOL)
    if bad:
        print(f"[{name}] parameter gradients:\n{table}")
    assert not bad, "\n".join(bad)
    if cfg is LC.TEXT_LOCAL:
        assert N1 * L1 + N2 * L2 >= 1024
        pooled_p, grads_p, rows_p = _run_pair(torch, cva, cfg, P, segs, packed=True)
        assert rows_p == N1 * L1 + N2 * L2, "a call with a sequence above 128 rows must run the padded layout"
        assert torch.equal(pooled_p, pooled)
        for n, g in grads.items():  # (the same launches on the same data; a few gradients are accumulated with fp32 atomics)
            assert float((grads_p[n] - g).abs().max()) <= 1e-4 * float(g.abs().max()) + 1e-9, n
    assert cva.lib.get_option("fused_attn_launches") == n0, "the in-chain attention covers fixed lengths <= 80 only"


def test_two_segments_without_input_fc_are_refused_in_the_backward(env):
    """coot_net_bwd runs the input LayerNorm's backward of a network without input FC as one launch over all token rows of `feats`: with
    a second segment it would run past the end of that tensor (and sum a wrong gain gradient).  No shipped network is built that way;
    TransformerHip refuses the backward of such a call before anything is launched.  The forward is unaffected."""
    torch, cva = env
    cfg = LC.LOCAL_NOFC[16]
    net = H.make_hip_net(cfg, O.make_params(cfg, LC.PARAM_SEED)).eval()
    rs = np.random.RandomState(3)
    t1, t2 = torch.from_numpy(rs.randn(2, 144, 64)).float().cuda(), torch.from_numpy(rs.randn(5, 16, 64)).float().cuda()
    a, b = net.forward_pair(t1, torch.tensor([144, 128]).cuda(), t2, torch.tensor([16, 8, 1, 6, 4]).cuda())
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    with pytest.raises(RuntimeError, match="needs a network with input_fc"):
        (a.sum() + b.sum()).backward()
    torch.cuda.synchronize()


def test_native_step_with_paragraphs_above_128_rows_matches_autograd_path(env):
    """test_native_step_matches_autograd_path (tests/test_gpu_path.py) with that test's bounds on a ragged batch that carries packed row
    starts and has videos of up to 144 frames and paragraphs of up to 160 words: both routes run the padded layout, the video / paragraph
    segment on the chunked attention kernels and the clip / sentence segment on the short ones, inside the fused chains."""
    torch, cva = env
    dims = (256, 192, 384, 8, 384, 768)
    cfgs = H.full_cfgs(*dims)
    Ps = [O.make_params(cfgs[i], 1 + i, scale=0.02) for i in range(4)]
    batch = cva.synthetic.make_batch(20, 12, cva.synthetic.anet_like_counts(70, 12), 144, 20, 160, 12, dims[0], dims[1], ragged=True, packed=True)
    assert int(batch.vid_feat_len.max()) == 144 and int(batch.par_feat_len.max()) == 160 and min(batch.tok_vis, batch.tok_txt) >= 1024
    cfg_a, mgr_a = H.make_manager(cfgs, Ps, dropout=0.0, cc_weight=0.0)
    cfg_b, mgr_b = H.make_manager(cfgs, Ps, dropout=0.0, cc_weight=0.0)
    mgr_a.set_all_models_train(); mgr_b.set_all_models_train()
    ta, tb = cva.RetrievalTrainer(cfg_a, mgr_a), cva.RetrievalTrainer(cfg_b, mgr_b)
    l_nat = ta.train_step_native(batch, do_optimizer=False)
    nets_b = list(mgr_b.model_dict.values())
    for n in nets_b:
        n.bind_flat_grads().zero_()
        n.accumulate_into_flat = True
    v, t = mgr_b.encode_visual(batch), mgr_b.encode_text(batch)
    loss_b = tb.compute_total_constrastive_loss(v, t)
    loss_b.backward()
    torch.cuda.synchronize()
    assert abs(float(l_nat[0]) - float(loss_b)) < 1e-5 * max(1.0, abs(float(loss_b)))
    for na, nb in zip(mgr_a.model_dict.values(), nets_b):
        ga, gb = na._grad_flat, nb._grad_flat
        d = float((ga - gb).abs().max())
        print(f"[native, Lp = 160] max |g_native - g_autograd| = {d:.3e} of max |g| = {float(gb.abs().max()):.3e}")
        assert d <= 1e-4 * float(gb.abs().max()) + 1e-9
        nb.accumulate_into_flat = False
    ta.train_step_native(batch)
    tb.train_step(batch)
    torch.cuda.synchronize()
    for na, nb in zip(mgr_a.model_dict.values(), mgr_b.model_dict.values()):
        gmax = float(nb._grad_flat.abs().max())
        for (name, off, shape) in na.table:
            n = int(np.prod(shape))
            if float(nb._grad_flat[off:off + n].abs().max()) < 1e-5 * gmax:  # zero true gradient: +-lr noise in both (see the original)
                continue
            diff = (na._flat[off:off + n] - nb._flat[off:off + n]).abs()
            sig = nb._grad_flat[off:off + n].abs() > 1e-2 * gmax
            if bool(sig.any()):
                d = float(diff[sig].max())
                assert d < 2e-4, (name, d)
            assert float(diff.max()) <= 2.05e-3, (name, float(diff.max()))


@pytest.mark.parametrize("route", ["autograd", "native"])
def test_long_paragraphs_against_the_reference_fixture(env, golden_dir, route):
    """bench_long_par (8 videos x 4 clips, up to 144 frames / 160 words next to 80-frame clips and 30-word sentences) against what the
    unmodified reference computed: embeddings, losses and every parameter gradient, at the tolerances of test_gpu_bench_parity.py.
    The native route is given packed row starts as well: a batch with a sequence above 128 rows runs the padded layout."""
    torch, cva = env
    g, cfgs, Ps, b = _case(golden_dir, "bench_long_par")
    assert int(g["meta"][2]) == 144 and int(g["meta"][4]) == 160
    batch = cva.synthetic.batch_from_numpy(b, packed=(route == "native"))
    idx_c, idx_s = torch.from_numpy(g["cc_idx_clip"]).cuda(), torch.from_numpy(g["cc_idx_sent"]).cuda()
    if route == "autograd":
        cfg, mgr = H.make_manager(cfgs, Ps, cc_weight=float(g["cc_weight"]))
        mgr.set_all_models_eval()
        trainer = cva.RetrievalTrainer(cfg, mgr, is_test=True)
        vis, txt = mgr.encode_visual(batch), mgr.encode_text(batch)
        contr = trainer.compute_total_constrastive_loss(vis, txt)
        cc = trainer.compute_cyclecons_loss(vis, txt, idx_c, idx_s)
        (contr + cc).backward()
        torch.cuda.synchronize()
        _check_embeddings(g, {"vid_emb": vis.vid_emb.detach().cpu().numpy(), "clip_emb": vis.clip_emb.detach().cpu().numpy(),
                              "vid_context": vis.vid_context.detach().cpu().numpy(), "par_emb": txt.par_emb.detach().cpu().numpy(),
                              "sent_emb": txt.sent_emb.detach().cpu().numpy(), "par_context": txt.par_context.detach().cpu().numpy()}, "long_par")
        contr, cc = float(contr), float(cc)
        grads = {k: {n: p.grad.detach().cpu().numpy() for n, p in mgr.model_dict[k].named_parameters() if p.requires_grad} for k in H.NET_KEYS}
    else:
        cfg, mgr = H.make_manager(cfgs, Ps, dropout=0.0, cc_weight=float(g["cc_weight"]))
        mgr.set_all_models_train()
        trainer = cva.RetrievalTrainer(cfg, mgr)
        losses = trainer.train_step_native(batch, do_optimizer=False, cc_indices=torch.cat([idx_c, idx_s]))
        torch.cuda.synchronize()
        _, contr, cc = (float(v) for v in losses)
        grads = {}
        for k in H.NET_KEYS:
            net = mgr.model_dict[k]
            flat = net._grad_flat.detach().cpu().numpy()
            grads[k] = {n: flat[off:off + int(np.prod(shape))].reshape(shape) for (n, off, shape) in net.table}
    rc, rcc = float(g["contr_loss"]), float(g["cc_loss"])
    print(f"[long_par {route}] contrastive {contr:.5f} vs {rc:.5f}; cycle-consistency {cc:.6f} vs {rcc:.6f}")
    assert abs(contr - rc) < 1e-3 * abs(rc) and abs(cc - rcc) < 2e-3 * abs(rcc) + 1e-6
    _check_grads(g, grads, f"long_par {route}")


def test_long_paragraphs_train_mode_against_the_reference_with_injected_masks(env, golden_dir):
    """bench_long_par_train: the reference in train mode with the library's dropout masks (p = 0.1) injected — pins the chunked kernels'
    attention-dropout masks, forward against backward and segment by segment; the same step under another seed must fail the bound
    (tests/test_gpu_train_parity.py, whose test body this runs)."""
    TP.test_train_mode_native_step_vs_reference_with_injected_masks(env, golden_dir, "bench_long_par_train")
