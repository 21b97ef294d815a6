"""Host side of the prepared gallery stored in 16-bit floats (include/coot_hip.h: coot_retrieval_row_norms_h,
coot_retrieval_topk_few_h; retrieval.GalleryIndex(storage=...)): the two new functions are declared, bound and exported by both
builds under the unchanged ABI version, the dtype codes of the header are the ones the Python side passes, and the constructor
refuses on the host what it cannot serve — the dtype first (a ValueError that names the allowed types), then the device.  The device
results are compared with the fp32 search on the widened gallery byte for byte in tests/test_gpu_topk_half.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_row_norms_h": 6, "coot_retrieval_topk_few_h": 14}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)


def test_half_abi_matches_the_header(cva):
    hdr = _header()
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):  # the storage formats do not depend on the operand format of the build
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7
    codes = {k: int(v) for k, v in re.findall(r"#define\s+COOT_GALLERY_(BF16|F16)\s+(\d+)", hdr)}
    assert codes == {"BF16": cva.retrieval.GALLERY_BF16, "F16": cva.retrieval.GALLERY_F16} and codes["BF16"] != codes["F16"]
    assert 0 not in codes.values()  # 0 is the fp32 gallery on the Python side


def test_gallery_index_checks_dtype_then_device(cva):
    """Nothing here needs a GPU: every tensor is a CPU tensor.  The dtype check comes first, so a CPU tensor of a dtype that cannot
    be stored gets the ValueError, and one of an allowed dtype gets "no CPU fallback"."""
    import torch
    from coot_videotext_amd import GalleryIndex
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for kw in ({}, {"normalize": False}, {"storage": torch.bfloat16}, {"storage": torch.float32}):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                GalleryIndex(torch.zeros(5, 8, dtype=dt), **kw)
    names = r"torch\.float32, torch\.bfloat16 or torch\.float16"
    for dt in (torch.int8, torch.float64):
        with pytest.raises(ValueError, match=names):
            GalleryIndex(torch.zeros(5, 8, dtype=dt))
    for dt in (torch.float32, torch.float16):
        with pytest.raises(ValueError, match=names):
            GalleryIndex(torch.zeros(5, 8, dtype=dt), storage=torch.int8)
    with pytest.raises(ValueError, match=names):
        GalleryIndex(torch.zeros(5, 8, dtype=torch.int8), storage=torch.bfloat16)  # the gallery's own dtype is checked too
