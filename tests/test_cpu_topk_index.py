"""Host side of the tile search on a prepared gallery (include/coot_hip.h: coot_retrieval_topk_index and its size query;
retrieval.retrieval_topk_index_device, GalleryIndex.search with more than 16 queries): the two functions declared, bound and
exported by both builds under the unchanged ABI version, and the wrappers refusing on the host what they cannot serve.  The device
results are compared with the fp32 tile search on the widened gallery in tests/test_gpu_topk_index.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_topk_index_workspace_bytes": 4, "coot_retrieval_topk_index": 15}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_index_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    args = re.search(r"\bcoot_retrieval_topk_index\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S).group(1)
    for part in ("const void* gallery", "int gallery_dtype", "const float* gallery_norms", "const uint8_t* keep"):
        assert part in args, part
    assert lib.coot_retrieval_topk_index_workspace_bytes.restype is ctypes.c_size_t
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # new functions only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def test_size_query_needs_no_device(cva):
    """The size query is host arithmetic: nothing for arguments no call accepts, and at least the M query norms otherwise."""
    lib = cva.lib.load()
    assert lib.coot_retrieval_topk_index_workspace_bytes(0, 10, 8, 1) == 0 and lib.coot_retrieval_topk_index_workspace_bytes(4, 0, 8, 1) == 0
    assert lib.coot_retrieval_topk_index_workspace_bytes(4, 10, 8, 0) == 0
    one = lib.coot_retrieval_topk_index_workspace_bytes(70, 64, 8, 10)  # one column tile: one split, no partial lists
    assert 70 * 4 <= one <= 70 * 4 + 256
    many = lib.coot_retrieval_topk_index_workspace_bytes(70, 6400, 8, 10)  # 100 column tiles: up to 64 splits of partial lists
    assert one + 2 * 70 * 10 * 8 <= many <= one + 64 * 70 * 10 * 8 + 256


class _OnDevice:
    """What a wrapper looks at before it touches the device: a float32 tensor [m, d] that says it is a CUDA tensor."""
    is_cuda = True

    def __init__(self, m, d):
        import torch
        self.shape, self.dtype = (m, d), torch.float32

    def dim(self):
        return len(self.shape)

    def contiguous(self):
        raise AssertionError("the wrapper went past its host checks")


def test_wrapper_refuses_on_the_host(cva):
    import torch
    from coot_videotext_amd import retrieval_topk_index_device
    q, g, norms = torch.zeros(20, 8), torch.zeros(5, 8), torch.ones(5)
    with pytest.raises(RuntimeError, match=r"no CPU fallback; use compute_retrieval_topk\)"):
        retrieval_topk_index_device(q, g, norms, 2)
    with pytest.raises(RuntimeError, match=r"no CPU fallback; use compute_retrieval_topk\)"):
        retrieval_topk_index_device(q, g.to(torch.bfloat16), None, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback; use compute_retrieval_topk_masked"):
        retrieval_topk_index_device(q, g, norms, 2, keep=torch.ones(5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # one host tensor among device ones is enough
        retrieval_topk_index_device(_OnDevice(20, 8), _OnDevice(5, 8), norms, 2)
    for msg, keeps in {"bool or torch.uint8": (torch.ones(5), torch.ones(5, dtype=torch.int32), [1] * 5),
                       "one flag per row": (torch.ones(4, dtype=torch.bool), torch.ones(6, dtype=torch.uint8), torch.ones(5, 1, dtype=torch.bool))}.items():
        for keep in keeps:
            with pytest.raises(ValueError, match=msg):
                retrieval_topk_index_device(q, g, norms, 2, keep=keep)
    dq, dg = _OnDevice(20, 8), _OnDevice(5, 8)
    for k in (0, 6, -1):
        with pytest.raises(ValueError, match=r"k = -?\d+ is outside 1 \.\. min\(N = 5, 128\)"):
            retrieval_topk_index_device(dq, dg, None, k)
    with pytest.raises(ValueError, match=r"k = 129 is outside 1 \.\. min\(N = 500, 128\)"):
        retrieval_topk_index_device(dq, _OnDevice(500, 8), None, 129)
    with pytest.raises(ValueError, match="queries of width 7, gallery of width 8"):
        retrieval_topk_index_device(_OnDevice(20, 7), dg, None, 2)
    dg.dtype = torch.float64
    with pytest.raises(ValueError, match="a gallery of dtype torch.float64"):
        retrieval_topk_index_device(dq, dg, None, 2)


@pytest.mark.parametrize("storage", ["float32", "bfloat16", "float16"])
def test_search_with_many_queries_refuses_on_the_host(cva, storage):
    """An index cannot be built without a device, so its search is reached through an instance made by hand (as in
    tests/test_cpu_topk_masked.py), here with more than 16 queries: the route this change adds."""
    import torch
    from coot_videotext_amd import GalleryIndex
    from coot_videotext_amd.retrieval import _gallery_codes
    dtype = getattr(torch, storage)
    index = object.__new__(GalleryIndex)
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = torch.zeros(5, 8, dtype=dtype), None, False, None, _gallery_codes()[dtype], dtype
    q = torch.zeros(70, 8)
    with pytest.raises(RuntimeError, match=r"GalleryIndex.search needs CUDA tensors \(there is no CPU fallback; use compute_retrieval_topk\)"):
        index.search(q, 2)
    with pytest.raises(ValueError, match="one flag per row"):
        index.search(q, 2, keep=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or torch.uint8"):
        index.search(q, 2, keep=torch.ones(5))
    with pytest.raises(RuntimeError, match="compute_retrieval_topk_masked"):
        index.search(q, 2, keep=torch.ones(5, dtype=torch.bool))
    for k in (0, 6):
        with pytest.raises(ValueError, match=rf"GalleryIndex.search: k = {k} is outside 1 \.\. min\(N = 5, 128\)"):
            index.search(_OnDevice(70, 8), k)
    with pytest.raises(ValueError, match="GalleryIndex.search: queries of width 7, gallery of width 8"):
        index.search(_OnDevice(70, 7), 2)


def test_routing_constant(cva):
    from coot_videotext_amd import RETRIEVAL_FEW_MAX
    from coot_videotext_amd.retrieval import INDEX_TILE_MIN_M_16BIT
    assert isinstance(INDEX_TILE_MIN_M_16BIT, int) and INDEX_TILE_MIN_M_16BIT > RETRIEVAL_FEW_MAX  # up to 16 queries the few-query call serves every storage
