"""Host side of the mutable gallery index (include/coot_hip.h: coot_retrieval_rows_put; GalleryIndex.add / update / compact and the
capacity= argument): the new function declared, bound and exported by both builds under the unchanged ABI version, and the methods
refusing on the host what they cannot serve, on an instance made by hand as in tests/test_cpu_topk_masked.py.  What the device
writes is compared with a freshly built index in tests/test_gpu_index_mutable.py."""
import ctypes
import fnmatch
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"coot_retrieval_rows_put": 11}


@pytest.fixture(scope="module")
def cva():
    import coot_videotext_amd as m
    return m


def test_rows_put_abi_matches_the_header(cva):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coot_hip.h")).read(), flags=re.S)
    lib = cva.lib.load()
    for name, n in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n, name
        assert "const int32_t* dest" in m.group(1) and "float* norms" in m.group(1), name
        assert len(getattr(lib, name).argtypes) == n, name
        assert name in cva.lib.EXPORTS
    assert "COOT_ABI_VERSION 7" in hdr and cva.lib.ABI_VERSION == 7  # a new function only: the ABI version stays
    vs = open(os.path.join(ROOT, "coot-videotext_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", " ", vs, flags=re.S))
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), (name, pats)
        assert name in vs, name
    libdir = os.path.dirname(cva.lib.LIB_PATH)
    for so in ("libcoot_hip.so", "libcoot_hip_f16.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, so)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW) <= exported, so
        assert ctypes.CDLL(os.path.join(libdir, so)).coot_version() == 7


def _by_hand(torch, storage=None):
    """An index cannot be built without a device: an instance made by hand with the six attributes of the existing host test."""
    from coot_videotext_amd import GalleryIndex
    storage = storage or torch.float32
    index = object.__new__(GalleryIndex)
    index.gallery, index.keep, index.normalize, index.norms = torch.zeros(5, 8, dtype=storage), None, False, None
    index._code, index.storage = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[storage], storage
    return index


def test_add_refuses_on_the_host(cva):
    import torch
    index = _by_hand(torch)
    assert len(index) == 5 and index.n == 5 and index.capacity == 5
    with pytest.raises(ValueError, match="width 8"):
        index.add(torch.zeros(2, 7))
    with pytest.raises(ValueError, match="width 8"):
        index.add(torch.zeros(7))
    with pytest.raises(ValueError, match="torch.int64"):
        index.add(torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="torch.float16"):
        _by_hand(torch, torch.bfloat16).add(torch.zeros(2, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="torch.bfloat16"):
        index.add(torch.zeros(2, 8, dtype=torch.bfloat16))  # (16-bit rows go into an index of their own type only)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.add(torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _by_hand(torch, torch.bfloat16).add(torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.add(torch.zeros(0, 8))  # the device is checked before the row count
    assert len(index) == 5 and index.capacity == 5 and index.gallery.shape == (5, 8)


def test_update_refuses_on_the_host(cva):
    import torch
    index = _by_hand(torch)
    ptr = index.gallery.data_ptr()
    with pytest.raises(ValueError, match="more than once"):
        index.update([1, 1], torch.zeros(2, 8))
    with pytest.raises(IndexError, match=r"row 5 is outside \[0, 5\)"):
        index.update([5], torch.zeros(1, 8))
    with pytest.raises(IndexError, match="row -1"):
        index.update(torch.tensor([-1]), torch.zeros(1, 8))
    with pytest.raises(TypeError, match="integers"):
        index.update([0.5], torch.zeros(1, 8))
    with pytest.raises(ValueError, match="3 rows of values for 2 row numbers"):
        index.update([0, 1], torch.zeros(3, 8))
    with pytest.raises(ValueError, match="width 8"):
        index.update([0, 1], torch.zeros(2, 9))
    with pytest.raises(ValueError, match="torch.float64"):
        index.update([0], torch.zeros(1, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.update([0, 4], torch.zeros(2, 8))
    assert index.gallery.data_ptr() == ptr and len(index) == 5  # refused: nothing was moved into a buffer of the index's own


def test_compact_on_the_host(cva):
    import torch
    index = _by_hand(torch)
    old = index.compact()  # no filter: nothing moves
    assert old.dtype is torch.int32 and old.tolist() == [0, 1, 2, 3, 4] and len(index) == 5 and index.keep is None
    index.remove([0, 1, 2, 3, 4])
    assert len(index) == 5
    with pytest.raises(ValueError, match="every row is removed"):
        index.compact()
    assert len(index) == 5 and index.keep.tolist() == [False] * 5 and index.capacity == 5
    # (gathering rows is plain tensor indexing: the stand-in shows the bookkeeping)
    index.gallery = torch.arange(40, dtype=torch.float32).reshape(5, 8)
    index.restore([1, 4])
    old = index.compact()
    assert old.dtype is torch.int32 and old.tolist() == [1, 4] and index.keep is None
    assert len(index) == 2 and index.capacity == 2 and index.gallery[:, 0].tolist() == [8.0, 32.0]
    assert index.nbytes == 2 * 8 * 4


def test_capacity_is_checked_before_the_device(cva):
    import torch
    from coot_videotext_amd import GalleryIndex
    g = torch.zeros(5, 8)
    with pytest.raises(ValueError, match="capacity = 4"):
        GalleryIndex(g, capacity=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GalleryIndex(g, capacity=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GalleryIndex(g)
