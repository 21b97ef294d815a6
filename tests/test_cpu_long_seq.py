"""The checker of tests/test_gpu_long_seq.py tested on the CPU: helpers.row_report at the committed bound K * E must reject the three
ways a long attention path goes wrong locally — a lost 1-row tail tile, rows of another sequence offset, a wrong scale behind the
128-row boundary — and accept the oracle's own gradients; and the conditions on the inputs hold (tests/long_seq_cases.py)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import long_seq_cases as LC

MUTATED = ["local_dh16_L129", "local_dh32_L129", "local_dh48_L129", "local_dh64_L129"]


def test_k_is_a_power_of_two_of_at_most_32():
    assert LC.K in (1, 2, 4, 8, 16, 32)


@pytest.mark.parametrize("name", MUTATED)
def test_row_report_rejects_local_errors_and_accepts_the_oracle(name):
    c = LC.oracle_case(name)
    cfg, N, L, _ = LC.SINGLE[name]
    assert (N, L) == (3, 129) and not cfg.use_input_fc
    bound = LC.K * c["E"]
    dx, valid = c["dx"], c["valid"]
    e, rows, _ = H.row_report(dx.copy(), dx, valid, bound)
    assert e == 0.0 and rows.size == 0
    e, rows, _ = H.row_report(c["dx_e"], dx, valid, bound)  # (the bf16-cache gradients: e = E by definition)
    assert e <= c["E"] < bound and rows.size == 0

    lost = dx.copy()          # (a) the tail tile of sequence 0 (its row 128, the only row of the third 64-row tile) never written
    lost[0, 128] = 0
    e, rows, _ = H.row_report(lost, dx, valid, bound)
    assert e > bound and rows.tolist() == [0 * L + 128], (e, rows)

    shifted = dx.copy()       # (b) sequence 1 read at a row offset that is off by one
    shifted[1] = np.roll(dx[1], 1, axis=0)
    e, rows, _ = H.row_report(shifted, dx, valid, bound)
    n_bad = rows.size
    assert e > bound and n_bad >= 0.9 * c["lens"][1] and set(rows // L) == {1}, (e, n_bad)

    halved = dx.copy()        # (c) a wrong scale on the rows behind the dispatch boundary
    halved[:, 128:] *= 0.5
    e, rows, _ = H.row_report(halved, dx, valid, bound)
    assert e > bound and rows.tolist() == [0 * L + 128], (e, rows)

    nan = dx.copy()           # a NaN row is the worst row, not an ignored one
    nan[0, 5, 3] = np.nan
    e, rows, _ = H.row_report(nan, dx, valid, bound)
    assert e == np.inf and rows.tolist() == [5]


def test_row_report_checks_small_rows_by_magnitude():
    rs = np.random.RandomState(0)
    ref = rs.randn(10, 8)
    ref[3] *= 1e-4            # a row far below 1 % of the largest: its direction is noise
    got = ref.copy()
    got[3] = -ref[3]
    e, rows, share = H.row_report(got, ref, np.ones(10, bool), 0.05)
    assert share == 0.1 and e < 0.05 and rows.size == 0      # opposite direction, negligible magnitude: passes
    got[3] = ref[0]
    e, rows, share = H.row_report(got, ref, np.ones(10, bool), 0.05)
    assert e > 1 and rows.tolist() == [3]                     # ... but a full-size row in its place does not
    got[3] = ref[3]
    got[7] = 0
    valid = np.ones(10, bool)
    valid[7] = False
    assert H.row_report(got, ref, valid, 0.05)[0] == 0.0      # rows outside the mask are not looked at


@pytest.mark.parametrize("name", list(LC.SINGLE))
def test_input_conditions(name):
    """lens[0] = L, a sequence that ends on a 64-row tile edge (above 64 rows), a sequence of one row, at most 1 % of the rows checked
    by magnitude only, and E — from the oracle alone — of the size bf16 rounding explains (2^-9 per element and a few stores)."""
    cfg, N, L, control = LC.SINGLE[name]
    c = LC.oracle_case(name)
    lens = c["lens"]
    assert lens[0] == L and lens.max() == L and 1 in lens and len(lens) == N
    if L > 64:
        assert any(l % 64 == 0 and l < L for l in lens), lens
    assert control == (L <= (32 if cfg.use_context else 128))
    assert (c["x"][~c["valid"]] == 0).all()
    print(f"[{name}] E = {c['E']:.5f}, magnitude-only rows {c['mag_only']:.4f}")
    assert c["mag_only"] <= LC.MAX_MAG_ONLY, c["mag_only"]
    assert 2e-3 < c["E"] < 3e-2, c["E"]
