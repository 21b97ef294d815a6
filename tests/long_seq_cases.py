"""Inputs, oracle results and the derived bound of the long-sequence tests (tests/test_cpu_long_seq.py, tests/test_gpu_long_seq.py).

A sequence of more than 128 rows leaves the short attention kernels (csrc/attention.hip: attn_short_path): the chunked forward kernel
and the merged dQ | dK/dV backward launch take over, two segments in one call go through the per-segment loop (csrc/api.hip:
attention_all), the context attention leaves attn_q1 above 64 keys, and the global networks leave their single launch above 32 items.

Every case here has lens[0] = L (the tail tile has valid rows), one sequence whose length is a multiple of 64 below L (a later 64-row
tile is fully masked; below 65 rows, where no such length exists, half of L) and one sequence of length 1.

THE BOUND.  Networks without an input FC return the gradient wrt their input rows; a token's row carries its own dQ / dK / dV
contribution, so a lost tile, a mask edge or a segment offset makes specific rows wrong by O(1).  helpers.row_report compares row by
row.  Per case, from the oracle alone,

    E = worst per-row ||g_bf16 - g_exact|| / ||g_exact||,   g_bf16 = O.net_bwd on the cache of O.net_fwd(..., O.BF16),

i.e. how far the bf16 rounding of the forward's stored activations ALONE moves a gradient row (dfeats rows and, for context networks,
dhidden rows).  The library's backward rounds its own intermediate gradients to bf16 as well, which E does not contain: the bound on
the GPU is K * E, with ONE K for all cases — 2 x the worst ratio e_gpu / E over the control cases (the same networks at L <= 128,
global ones at L <= 32: kernels other tests already hold to the oracle), rounded up to a power of two, and refused above 32.
"""
import functools

import numpy as np

from oracle import coot_oracle as O
from tests import helpers as H

# K: see above.  Measured on the MI355X (the table in tests/test_gpu_long_seq.py): worst control ratio e_gpu / E = 1.45
# (local_dh32_L128), 2 x 1.45 = 2.9 -> 4.  The long cases measured 0.79 ... 1.95.
K = 4
# the magnitude-only rows of row_report (||ref|| < 1 % of the largest row norm) may not exceed this share of the valid rows
MAX_MAG_ONLY = 0.01


def _nofc(hidden, heads):
    return O.NetConfig(input_dim=hidden, hidden_dim=hidden, num_heads=heads, ff_dim=hidden, use_input_fc=False, pool_hidden=2 * hidden,
                       pool_heads=2)


# local networks without an input FC (they return dfeats), one per head size the attention kernels are instantiated for
LOCAL_NOFC = {16: _nofc(64, 4), 32: _nofc(64, 2), 48: _nofc(96, 2), 64: _nofc(128, 2)}
SMALL_LOCAL = O.NetConfig(input_dim=40, hidden_dim=64, num_heads=4, ff_dim=64, pool_hidden=128, pool_heads=2)
TEXT_LOCAL = O.NetConfig(input_dim=1536, hidden_dim=384, num_heads=8, ff_dim=384, pool_hidden=768, pool_heads=2)
SMALL_GLOBAL = O.NetConfig(input_dim=64, hidden_dim=64, num_heads=4, ff_dim=64, use_input_fc=False, use_context=True, pooler="avg_special")
ANET_GLOBAL = O.NetConfig(input_dim=384, hidden_dim=384, num_heads=8, ff_dim=384, use_input_fc=False, use_context=True,
                          pooler="avg_special")

# name -> (config, N, L, control?)
SINGLE = {}
for _dh, _cfg in LOCAL_NOFC.items():
    for _L in (129, 192, 200):
        SINGLE[f"local_dh{_dh}_L{_L}"] = (_cfg, 3, _L, False)
    SINGLE[f"local_dh{_dh}_L128"] = (_cfg, 3, 128, True)
for _dh in (32, 64):  # (the short backward kernel at these head sizes had no test either)
    SINGLE[f"local_dh{_dh}_L40"] = (LOCAL_NOFC[_dh], 3, 40, True)
for _L in (33, 64, 65, 128, 129):
    SINGLE[f"small_global_L{_L}"] = (SMALL_GLOBAL, 4, _L, False)
SINGLE["small_global_L32"] = (SMALL_GLOBAL, 4, 32, True)
for _L in (32, 33, 65, 130):
    SINGLE[f"anet_global_L{_L}"] = (ANET_GLOBAL, 3, _L, _L == 32)
CONTROLS = [n for n, c in SINGLE.items() if c[3]]
LONG = [n for n, c in SINGLE.items() if not c[3]]
PARAM_SEED = 11
# (the seed base of the inputs is one at which no case has a magnitude-only row: a condition on the inputs, asserted in test_cpu_long_seq.py)
INPUT_SEED = 4000


def masked_len(L):
    """The multiple of 64 below L (a later tile of that sequence is fully masked); half of L where there is none."""
    return 64 * ((L - 1) // 64) if L > 64 else max(1, L // 2)


def make_lens(rs, N, L):
    lens = rs.randint(1, L + 1, size=N)
    lens[0] = L
    if N > 1:
        lens[1] = masked_len(L)
    if N > 2:
        lens[2] = 1
    return lens


def make_inputs(cfg, N, L, seed):
    """(x [N, L, Din] zero in the padding, lens, hidden [N, D] or None, R: the weights of the scalar sum(pooled * R) that is differentiated)"""
    rs = np.random.RandomState(seed)
    lens = make_lens(rs, N, L)
    x = rs.randn(N, L, cfg.input_dim)
    x[np.arange(L)[None, :] >= lens[:, None]] = 0
    hid = rs.randn(N, cfg.hidden_dim) if cfg.use_context else None
    # A pooled vector's gradient is shared out among the rows of its sequence (average pooling: 1 / len each), so with weights of one
    # size the single row of the length-1 sequence would carry 100 x the gradient of a row of a long one and the long sequences' rows
    # would all fall under row_report's magnitude floor: the weights of sequence n are scaled by len[n].
    R = rs.randn(N, cfg.hidden_dim * (2 if cfg.use_context else 1)) * lens[:, None]
    return x, lens, hid, R


def repad(x, L):
    """The same sequences padded to L rows."""
    out = np.zeros((x.shape[0], L, x.shape[2]), x.dtype)
    out[:, :x.shape[1]] = x
    return out


def worst_row_error(got_dx, got_dh, ref_dx, ref_dh, lens, bound=None):
    """row_report over the token rows of dfeats and, for a context network, the rows of dhidden (row n of dhidden divided by len[n] on
    both sides: e is unchanged, and the magnitude floor then compares rows of one size — see make_inputs).
    Returns (worst e, {tensor: offending rows}, largest share of magnitude-only rows)."""
    lens = np.asarray(lens)
    valid = np.arange(ref_dx.shape[1])[None, :] < lens[:, None]
    e, rows, share = H.row_report(got_dx, ref_dx, valid, bound)
    bad = {"dfeats": rows}
    if ref_dh is not None:
        eh, rh, sh = H.row_report(np.asarray(got_dh, np.float64) / lens[:, None], ref_dh / lens[:, None], np.ones(len(lens), bool), bound)
        bad["dhidden"] = rh
        e, share = max(e, eh), max(share, sh)
    return e, bad, share


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """Everything the oracle says about one single-segment case, computed once per process and shared (treat as read-only)."""
    cfg, N, L, _ = SINGLE[name]
    P = O.make_params(cfg, PARAM_SEED)
    x, lens, hid, R = make_inputs(cfg, N, L, INPUT_SEED + L)
    pooled, tok, cache = O.net_fwd(P, cfg, x, lens, hid)
    pooled_e, tok_e, cache_e = O.net_fwd(P, cfg, x, lens, hid, O.BF16)
    G, dhid, dx = O.net_bwd(P, cfg, R, cache, need_dfeats=True)
    G_e, dhid_e, dx_e = O.net_bwd(P, cfg, R, cache_e, need_dfeats=True)
    valid = np.arange(L)[None, :] < lens[:, None]
    E, _, share = worst_row_error(dx_e, dhid_e, dx, dhid, lens)
    return dict(cfg=cfg, P=P, x=x, lens=lens, hid=hid, R=R, valid=valid, pooled=pooled, tok=tok, pooled_e=pooled_e, tok_e=tok_e, G=G,
                dhid=dhid, dx=dx, dhid_e=dhid_e, dx_e=dx_e, E=E, mag_only=share)
