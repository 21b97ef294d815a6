"""Host side of COOT_STEP_TEXT_AHEAD (include/coot_hip.h; csrc/api_step.hip: the fork of coot_train_step): the flag's value in the
header and in lib.py, its A/B switch and counter, their place in the integration notes, and that the next free bit is still refused
before anything is launched.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_flag_value_in_header_and_bindings(cva):
    hdr = open(os.path.join(ROOT, "include", "coot_hip.h")).read()
    assert re.search(r"#define COOT_STEP_TEXT_AHEAD 64\b", hdr)
    assert cva.lib.STEP_TEXT_AHEAD == 64
    bits = [int(v) for v in re.findall(r"#define COOT_STEP_[A-Z_]+ (\d+)", hdr)]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32, 64]
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # a new flag only: the ABI version stays
    # the deferred join's comment points at the flag that builds on it
    defer = hdr[hdr.index("#define COOT_STEP_DEFER_TEXT_JOIN"):hdr.index("#define COOT_STEP_TEXT_AHEAD")]
    assert "COOT_STEP_TEXT_AHEAD" in defer


def test_switch_counter_and_integration_notes(cva):
    lib = cva.lib.load()
    assert cva.lib.get_option("text_ahead") == 1
    assert cva.lib.get_option("text_ahead_steps") >= 0
    try:
        assert lib.coot_set_option(b"text_ahead", 0) == 0 and cva.lib.get_option("text_ahead") == 0
    finally:
        assert lib.coot_set_option(b"text_ahead", 1) == 0
    assert lib.coot_set_option(b"text_ahead_steps", 0) != 0  # a counter: read-only
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    para = text[text.index("A/B and profiling switches"):]
    switches, reads = para[:para.index("`coot_get_option` reads")], para[para.index("`coot_get_option` reads"):]
    assert "`text_ahead`" in switches
    assert "`text_ahead_steps`" in reads[:reads.index("back.")]


def test_next_free_bit_is_still_refused_on_the_host(cva):
    """Bit 128 is not a flag: coot_train_step refuses it in its argument checks, before it looks at a buffer or a stream."""
    L = cva.lib
    lib = L.load()
    sc = L.StepConfig()
    for i, oc in enumerate(H.full_cfgs(256, 192, 384, 8, 384, 768)):
        sc.net[i] = cva.TransformerConfig(H.ocfg_to_dict(oc), oc.input_dim).to_c()
    d = L.StepDims(4, 8, 8, 8, 8, 8, 2, 2, 0, 0, L.SOURCE_PADDED)
    bufs, x = L.StepBuffers(), L.StepBatch()
    dummy = C.c_void_p(4096)
    rc = lib.coot_train_step(C.byref(sc), C.byref(bufs), C.byref(x), C.byref(d), dummy, dummy, 1 << 20, 1, 1, 1,
                             L.STEP_OPTIMIZER | 128, None, None, dummy)
    assert rc != 0 and b"unknown bits" in lib.coot_last_error()
