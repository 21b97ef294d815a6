"""What the prepared-gallery searches refuse on the host, as one table: the four wrappers (retrieval_topk_device,
retrieval_topk_index_device, retrieval_topk_grouped_device, retrieval_topk_multi_device) and the three GalleryIndex methods (search at
its three routes, search_grouped, search_multi), every single fault of their arguments that can be reached without a GPU, each with the
exception's type and its whole text.  A row starts from arguments that pass every host check (stand-ins that say they are on the device and
whose contiguous() raises: a wrapper that walks past its checks fails the row) and changes one of them.  The index methods are reached
through an instance made by hand, as in tests/test_cpu_topk_index.py, whose gallery and norms are varied too.
Faults that need real device tensors: tests/test_gpu_topk_grouped.py::test_width_and_k_are_refused_on_the_host and
tests/test_gpu_topk_multi.py::test_width_k_and_offsets_are_refused_on_the_host."""
import pytest
import torch

N, D = 5, 8


class _OnDevice:
    """What a wrapper looks at before it touches the device: a tensor of the given shape that says it is a CUDA tensor."""
    is_cuda = True
    device = "cuda:0"

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.dtype = shape, dtype

    def dim(self):
        return len(self.shape)

    def contiguous(self):
        raise AssertionError("the wrapper went past its host checks")


class _SaysCuda(torch.Tensor):
    """A CPU tensor that says it is a CUDA tensor: keep and groups have to be torch tensors, so no stand-in passes for them.  Its
    address is never handed to the library."""
    is_cuda = True

    def data_ptr(self):
        raise AssertionError("the wrapper went past its host checks")


def _dev(t):
    return t.as_subclass(_SaysCuda)


def _index(gallery, code=0, norms=None):
    from coot_videotext_amd import GalleryIndex
    index = object.__new__(GalleryIndex)
    index.gallery, index.keep, index.normalize, index.norms, index._code, index.storage = gallery, None, norms is not None, norms, code, gallery.dtype
    return index


def _call(entry, a):
    import coot_videotext_amd as cva
    q = {"cpu": lambda: torch.zeros(a["m"], D), "1d": lambda: _OnDevice(D), "device": lambda: _OnDevice(a["m"], a["width"]),
         "float64": lambda: _OnDevice(a["m"], D, dtype=torch.float64), "tensor": lambda: _dev(torch.zeros(a["m"], D))}[a["queries"]]()
    g = {"cpu": lambda: torch.zeros(N, D), "device": lambda: _OnDevice(N, D, dtype=a["storage"]), "tensor": lambda: _dev(torch.zeros(N, D))}[a["gallery"]]()
    k, keep, norms, groups, offsets, num_groups = (a[x] for x in ("k", "keep", "norms", "groups", "offsets", "num_groups"))
    if entry == "retrieval_topk_device":
        return cva.retrieval_topk_device(q, g, k, keep=keep)
    if entry == "retrieval_topk_index_device":
        return cva.retrieval_topk_index_device(q, g, norms, k, keep=keep)
    if entry == "retrieval_topk_grouped_device":
        return cva.retrieval_topk_grouped_device(q, g, norms, groups, k, num_groups=num_groups, keep=keep)
    if entry == "retrieval_topk_multi_device":
        return cva.retrieval_topk_multi_device(q, offsets, g, norms, groups, k, num_groups=num_groups, keep=keep)
    if entry == "GalleryIndex.search":  # (norms: those of the hand-made index)
        return _index(g, a["code"], norms).search(q, k, keep=keep)
    if entry == "GalleryIndex.search_grouped":
        return _index(g, 0, norms).search_grouped(q, k, groups, num_groups=num_groups, keep=keep)
    assert entry == "GalleryIndex.search_multi", entry
    return _index(g, 0, norms).search_multi(q, offsets, k, groups, num_groups=num_groups, keep=keep)


GOOD = {"m": 3, "width": D, "queries": "device", "gallery": "device", "storage": torch.float32, "code": 0, "norms": None, "keep": None, "k": 2,
        "groups": _dev(torch.zeros(N, dtype=torch.int32)), "offsets": [0, 3], "num_groups": 1}
CPU, ONE_D, F64, NARROW, Q64 = {"queries": "cpu"}, {"queries": "1d"}, {"storage": torch.float64}, {"width": 7}, {"queries": "float64"}
CPU_GALLERY, CPU_NORMS = {"gallery": "cpu"}, {"norms": torch.ones(N)}
KEEP_LIST, KEEP_F32, KEEP_SHORT = {"keep": [1] * N}, {"keep": _dev(torch.ones(N))}, {"keep": _dev(torch.ones(N - 1, dtype=torch.bool))}
KEEP_CPU, KEEP_OK = {"keep": torch.ones(N, dtype=torch.bool)}, {"keep": _dev(torch.ones(N, dtype=torch.uint8))}
GROUPS_LIST, GROUPS_F32 = {"groups": [0] * N}, {"groups": _dev(torch.zeros(N))}
GROUPS_SHORT, GROUPS_CPU = {"groups": _dev(torch.zeros(N - 1, dtype=torch.int64))}, {"groups": torch.zeros(N, dtype=torch.int32)}
# the two refusals behind contiguous(): on tensors that have one
NO_GROUP, HUGE = ({"queries": "tensor", "gallery": "tensor", "num_groups": g} for g in (0, 1 << 27))


def _k(k):
    return {"k": k}


def _off(offsets):
    return {"offsets": offsets}


ROWS = [
    # ---- retrieval_topk_device: the tile search on two plain tensors (k is left to the library)
    ("retrieval_topk_device", CPU, RuntimeError, "retrieval_topk_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("retrieval_topk_device", CPU_GALLERY, RuntimeError, "retrieval_topk_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("retrieval_topk_device", {**CPU, **KEEP_OK}, RuntimeError,
     "retrieval_topk_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
    ("retrieval_topk_device", ONE_D, AssertionError, "(torch.float32, torch.float32, (8,), (5, 8))"),
    ("retrieval_topk_device", KEEP_LIST, ValueError, "retrieval_topk_device: keep has to be a torch.bool or torch.uint8 tensor, not list"),
    ("retrieval_topk_device", KEEP_F32, ValueError, "retrieval_topk_device: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
    ("retrieval_topk_device", KEEP_SHORT, ValueError, "retrieval_topk_device: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
    ("retrieval_topk_device", KEEP_CPU, RuntimeError,
     "retrieval_topk_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
    ("retrieval_topk_device", F64, AssertionError, "(torch.float32, torch.float64, (3, 8), (5, 8))"),
    ("retrieval_topk_device", NARROW, AssertionError, "((3, 7), (5, 8))"),
    # ---- retrieval_topk_index_device: the tile search on a gallery as an index holds it
    ("retrieval_topk_index_device", CPU, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("retrieval_topk_index_device", CPU_GALLERY, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("retrieval_topk_index_device", CPU_NORMS, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("retrieval_topk_index_device", {**CPU, **KEEP_OK}, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
    ("retrieval_topk_index_device", ONE_D, AssertionError, "(torch.float32, (8,), (5, 8))"),
    ("retrieval_topk_index_device", KEEP_LIST, ValueError, "retrieval_topk_index_device: keep has to be a torch.bool or torch.uint8 tensor, not list"),
    ("retrieval_topk_index_device", KEEP_F32, ValueError,
     "retrieval_topk_index_device: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
    ("retrieval_topk_index_device", KEEP_SHORT, ValueError,
     "retrieval_topk_index_device: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
    ("retrieval_topk_index_device", KEEP_CPU, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
    ("retrieval_topk_index_device", F64, ValueError,
     "retrieval_topk_index_device: a gallery of dtype torch.float64; it has to be torch.float32, torch.bfloat16 or torch.float16"),
    ("retrieval_topk_index_device", NARROW, ValueError, "retrieval_topk_index_device: queries of width 7, gallery of width 8"),
    ("retrieval_topk_index_device", _k(0), ValueError, "retrieval_topk_index_device: k = 0 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_index_device", _k(N + 1), ValueError, "retrieval_topk_index_device: k = 6 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_index_device", _k(129), ValueError, "retrieval_topk_index_device: k = 129 is outside 1 .. min(N = 5, 128)"),
    # ---- retrieval_topk_grouped_device: groups first, then keep (which names the mirror of the filtered search), then the rest
    ("retrieval_topk_grouped_device", GROUPS_LIST, ValueError,
     "retrieval_topk_grouped_device: groups has to be a torch.int32 or torch.int64 tensor, not list"),
    ("retrieval_topk_grouped_device", GROUPS_F32, ValueError,
     "retrieval_topk_grouped_device: groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"),
    ("retrieval_topk_grouped_device", GROUPS_SHORT, ValueError,
     "retrieval_topk_grouped_device: groups of shape (4,), a gallery of 5 rows (one group id per row: [5])"),
    ("retrieval_topk_grouped_device", GROUPS_CPU, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("retrieval_topk_grouped_device", KEEP_LIST, ValueError, "retrieval_topk_grouped_device: keep has to be a torch.bool or torch.uint8 tensor, not list"),
    ("retrieval_topk_grouped_device", KEEP_F32, ValueError,
     "retrieval_topk_grouped_device: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
    ("retrieval_topk_grouped_device", KEEP_SHORT, ValueError,
     "retrieval_topk_grouped_device: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
    ("retrieval_topk_grouped_device", KEEP_CPU, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
    ("retrieval_topk_grouped_device", CPU, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("retrieval_topk_grouped_device", {**CPU, **KEEP_OK}, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("retrieval_topk_grouped_device", CPU_GALLERY, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("retrieval_topk_grouped_device", CPU_NORMS, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("retrieval_topk_grouped_device", F64, ValueError,
     "retrieval_topk_grouped_device: a gallery of dtype torch.float64; it has to be torch.float32, torch.bfloat16 or torch.float16"),
    ("retrieval_topk_grouped_device", NARROW, ValueError, "retrieval_topk_grouped_device: queries of width 7, gallery of width 8"),
    ("retrieval_topk_grouped_device", _k(0), ValueError, "retrieval_topk_grouped_device: k = 0 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_grouped_device", _k(N + 1), ValueError, "retrieval_topk_grouped_device: k = 6 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_grouped_device", _k(129), ValueError, "retrieval_topk_grouped_device: k = 129 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_grouped_device", NO_GROUP, ValueError, "retrieval_topk_grouped_device: num_groups = 0; there has to be at least one group"),
    # ---- retrieval_topk_multi_device: types and shapes of groups, keep and offsets first, then every device at once
    ("retrieval_topk_multi_device", GROUPS_LIST, ValueError, "retrieval_topk_multi_device: groups has to be a torch.int32 or torch.int64 tensor, not list"),
    ("retrieval_topk_multi_device", GROUPS_F32, ValueError,
     "retrieval_topk_multi_device: groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"),
    ("retrieval_topk_multi_device", GROUPS_SHORT, ValueError,
     "retrieval_topk_multi_device: groups of shape (4,), a gallery of 5 rows (one group id per row: [5])"),
    ("retrieval_topk_multi_device", GROUPS_CPU, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("retrieval_topk_multi_device", KEEP_LIST, ValueError, "retrieval_topk_multi_device: keep has to be a torch.bool or torch.uint8 tensor, not list"),
    ("retrieval_topk_multi_device", KEEP_F32, ValueError,
     "retrieval_topk_multi_device: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
    ("retrieval_topk_multi_device", KEEP_SHORT, ValueError, "retrieval_topk_multi_device: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
    ("retrieval_topk_multi_device", KEEP_CPU, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("retrieval_topk_multi_device", CPU, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("retrieval_topk_multi_device", CPU_GALLERY, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("retrieval_topk_multi_device", CPU_NORMS, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("retrieval_topk_multi_device", ONE_D, AssertionError, "(8,)"),
    ("retrieval_topk_multi_device", _off(_OnDevice(2, dtype=torch.int64)), ValueError,
     "retrieval_topk_multi_device: offsets live on the host (a sequence, a numpy array or a CPU integer tensor), not on cuda:0"),
    ("retrieval_topk_multi_device", _off([0.0, 3.0]), ValueError,
     "retrieval_topk_multi_device: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not list of dtype float64 and shape (2,)"),
    ("retrieval_topk_multi_device", _off([0]), ValueError,
     "retrieval_topk_multi_device: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not list of dtype int64 and shape (1,)"),
    ("retrieval_topk_multi_device", _off([[0, 3]]), ValueError,
     "retrieval_topk_multi_device: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not list of dtype int64 and shape (1, 2)"),
    ("retrieval_topk_multi_device", _off(None), ValueError,
     "retrieval_topk_multi_device: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not NoneType of dtype object and shape ()"),
    ("retrieval_topk_multi_device", _off(torch.tensor([0.0, 3.0])), ValueError,
     "retrieval_topk_multi_device: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not ndarray of dtype float32 and shape (2,)"),
    ("retrieval_topk_multi_device", _off([1, 3]), ValueError,
     "retrieval_topk_multi_device: offsets runs from 1 to 3; it has to start at 0 and end at M = 3"),
    ("retrieval_topk_multi_device", _off([0, 2]), ValueError,
     "retrieval_topk_multi_device: offsets runs from 0 to 2; it has to start at 0 and end at M = 3"),
    ("retrieval_topk_multi_device", _off([0, 2, 1, 3]), ValueError,
     "retrieval_topk_multi_device: offsets decreases at entry 2; it has to be non-decreasing"),
    ("retrieval_topk_multi_device", F64, ValueError,
     "retrieval_topk_multi_device: a gallery of dtype torch.float64; it has to be torch.float32, torch.bfloat16 or torch.float16"),
    ("retrieval_topk_multi_device", NARROW, ValueError, "retrieval_topk_multi_device: queries of width 7, gallery of width 8"),
    ("retrieval_topk_multi_device", _k(0), ValueError, "retrieval_topk_multi_device: k = 0 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_multi_device", _k(N + 1), ValueError, "retrieval_topk_multi_device: k = 6 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_multi_device", _k(129), ValueError, "retrieval_topk_multi_device: k = 129 is outside 1 .. min(N = 5, 128)"),
    ("retrieval_topk_multi_device", NO_GROUP, ValueError, "retrieval_topk_multi_device: num_groups = 0; there has to be at least one group"),
    ("retrieval_topk_multi_device", HUGE, ValueError,
     "retrieval_topk_multi_device: a paragraph of 3 sentences against 134217728 groups is a table of 402653184 entries; one paragraph has at most 2^28"),
]

# ---- GalleryIndex.search at its three routes: one few-query call, the tile call (more than 16 queries on a float32 index), slices of 16
# (fewer than INDEX_TILE_MIN_M_16BIT queries on a 16-bit index).  With CPU queries it names compute_retrieval_topk whatever keep is.
for route in ({}, {"m": 20}, {"m": 70, "storage": torch.bfloat16, "code": 1}):
    ROWS += [("GalleryIndex.search", {**route, **change}, exc, text) for change, exc, text in (
        (CPU, RuntimeError, "GalleryIndex.search needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
        ({**CPU, **KEEP_OK}, RuntimeError, "GalleryIndex.search needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
        (KEEP_LIST, ValueError, "GalleryIndex.search: keep has to be a torch.bool or torch.uint8 tensor, not list"),
        (KEEP_F32, ValueError, "GalleryIndex.search: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
        (KEEP_SHORT, ValueError, "GalleryIndex.search: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
        (KEEP_CPU, RuntimeError, "GalleryIndex.search needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
        (NARROW, ValueError, "GalleryIndex.search: queries of width 7, gallery of width 8"),
        ({**NARROW, **KEEP_OK}, ValueError, "GalleryIndex.search: queries of width 7, gallery of width 8"),
        (_k(0), ValueError, "GalleryIndex.search: k = 0 is outside 1 .. min(N = 5, 128)"),
        (_k(N + 1), ValueError, "GalleryIndex.search: k = 6 is outside 1 .. min(N = 5, 128)"),
        (_k(129), ValueError, "GalleryIndex.search: k = 129 is outside 1 .. min(N = 5, 128)"))]

ROWS += [
    # ---- GalleryIndex.search_grouped: the messages of the wrapper under the method's name; num_groups is the wrapper's own refusal
    ("GalleryIndex.search_grouped", GROUPS_LIST, ValueError, "GalleryIndex.search_grouped: groups has to be a torch.int32 or torch.int64 tensor, not list"),
    ("GalleryIndex.search_grouped", GROUPS_F32, ValueError,
     "GalleryIndex.search_grouped: groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"),
    ("GalleryIndex.search_grouped", GROUPS_SHORT, ValueError,
     "GalleryIndex.search_grouped: groups of shape (4,), a gallery of 5 rows (one group id per row: [5])"),
    ("GalleryIndex.search_grouped", GROUPS_CPU, RuntimeError,
     "GalleryIndex.search_grouped needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("GalleryIndex.search_grouped", KEEP_LIST, ValueError, "GalleryIndex.search_grouped: keep has to be a torch.bool or torch.uint8 tensor, not list"),
    ("GalleryIndex.search_grouped", KEEP_F32, ValueError,
     "GalleryIndex.search_grouped: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
    ("GalleryIndex.search_grouped", KEEP_SHORT, ValueError, "GalleryIndex.search_grouped: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
    ("GalleryIndex.search_grouped", KEEP_CPU, RuntimeError,
     "GalleryIndex.search_grouped needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_masked)"),
    ("GalleryIndex.search_grouped", CPU, RuntimeError,
     "GalleryIndex.search_grouped needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("GalleryIndex.search_grouped", {**CPU, **KEEP_OK}, RuntimeError,
     "GalleryIndex.search_grouped needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("GalleryIndex.search_grouped", NARROW, ValueError, "GalleryIndex.search_grouped: queries of width 7, gallery of width 8"),
    ("GalleryIndex.search_grouped", {**NARROW, "m": 20}, ValueError, "GalleryIndex.search_grouped: queries of width 7, gallery of width 8"),
    ("GalleryIndex.search_grouped", _k(0), ValueError, "GalleryIndex.search_grouped: k = 0 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_grouped", _k(N + 1), ValueError, "GalleryIndex.search_grouped: k = 6 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_grouped", _k(129), ValueError, "GalleryIndex.search_grouped: k = 129 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_grouped", NO_GROUP, ValueError, "retrieval_topk_grouped_device: num_groups = 0; there has to be at least one group"),
    # ---- GalleryIndex.search_multi: likewise; num_groups and the table bound are the wrapper's own refusals
    ("GalleryIndex.search_multi", GROUPS_LIST, ValueError, "GalleryIndex.search_multi: groups has to be a torch.int32 or torch.int64 tensor, not list"),
    ("GalleryIndex.search_multi", GROUPS_F32, ValueError, "GalleryIndex.search_multi: groups has to be a torch.int32 or torch.int64 tensor, not torch.float32"),
    ("GalleryIndex.search_multi", GROUPS_SHORT, ValueError, "GalleryIndex.search_multi: groups of shape (4,), a gallery of 5 rows (one group id per row: [5])"),
    ("GalleryIndex.search_multi", GROUPS_CPU, RuntimeError,
     "GalleryIndex.search_multi needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("GalleryIndex.search_multi", KEEP_LIST, ValueError, "GalleryIndex.search_multi: keep has to be a torch.bool or torch.uint8 tensor, not list"),
    ("GalleryIndex.search_multi", KEEP_F32, ValueError, "GalleryIndex.search_multi: keep has to be a torch.bool or torch.uint8 tensor, not torch.float32"),
    ("GalleryIndex.search_multi", KEEP_SHORT, ValueError, "GalleryIndex.search_multi: keep of shape (4,), a gallery of 5 rows (one flag per row: [5])"),
    ("GalleryIndex.search_multi", KEEP_CPU, RuntimeError,
     "GalleryIndex.search_multi needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("GalleryIndex.search_multi", CPU, RuntimeError, "GalleryIndex.search_multi needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("GalleryIndex.search_multi", ONE_D, AssertionError, "(8,)"),
    ("GalleryIndex.search_multi", _off(_OnDevice(2, dtype=torch.int64)), ValueError,
     "GalleryIndex.search_multi: offsets live on the host (a sequence, a numpy array or a CPU integer tensor), not on cuda:0"),
    ("GalleryIndex.search_multi", _off([0.0, 3.0]), ValueError,
     "GalleryIndex.search_multi: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not list of dtype float64 and shape (2,)"),
    ("GalleryIndex.search_multi", _off([0]), ValueError,
     "GalleryIndex.search_multi: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not list of dtype int64 and shape (1,)"),
    ("GalleryIndex.search_multi", _off([[0, 3]]), ValueError,
     "GalleryIndex.search_multi: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not list of dtype int64 and shape (1, 2)"),
    ("GalleryIndex.search_multi", _off(None), ValueError,
     "GalleryIndex.search_multi: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not NoneType of dtype object and shape ()"),
    ("GalleryIndex.search_multi", _off(torch.tensor([0.0, 3.0])), ValueError,
     "GalleryIndex.search_multi: offsets has to be a sequence, numpy array or CPU tensor of at least 2 integers (P + 1 of them, paragraph p = "
     "queries[offsets[p]:offsets[p + 1]]), not ndarray of dtype float32 and shape (2,)"),
    ("GalleryIndex.search_multi", _off([1, 3]), ValueError, "GalleryIndex.search_multi: offsets runs from 1 to 3; it has to start at 0 and end at M = 3"),
    ("GalleryIndex.search_multi", _off([0, 2]), ValueError, "GalleryIndex.search_multi: offsets runs from 0 to 2; it has to start at 0 and end at M = 3"),
    ("GalleryIndex.search_multi", _off([0, 2, 1, 3]), ValueError, "GalleryIndex.search_multi: offsets decreases at entry 2; it has to be non-decreasing"),
    ("GalleryIndex.search_multi", NARROW, ValueError, "GalleryIndex.search_multi: queries of width 7, gallery of width 8"),
    ("GalleryIndex.search_multi", _k(0), ValueError, "GalleryIndex.search_multi: k = 0 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_multi", _k(N + 1), ValueError, "GalleryIndex.search_multi: k = 6 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_multi", _k(129), ValueError, "GalleryIndex.search_multi: k = 129 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_multi", NO_GROUP, ValueError, "retrieval_topk_multi_device: num_groups = 0; there has to be at least one group"),
    ("GalleryIndex.search_multi", HUGE, ValueError,
     "retrieval_topk_multi_device: a paragraph of 3 sentences against 134217728 groups is a table of 402653184 entries; one paragraph has at most 2^28"),
]


# ---- what a hand-made index holds: a method that goes through a wrapper's call refuses the gallery and the norms under the wrapper's name,
# after everything the caller brought; the few-query routes of search (16 queries at most, or slices) take them as the constructor left them
TILE = {"m": 20}
ROWS += [
    ("GalleryIndex.search", {**TILE, **CPU_GALLERY}, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("GalleryIndex.search", {**TILE, **CPU_NORMS}, RuntimeError,
     "retrieval_topk_index_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk)"),
    ("GalleryIndex.search", {**TILE, **F64}, ValueError,
     "retrieval_topk_index_device: a gallery of dtype torch.float64; it has to be torch.float32, torch.bfloat16 or torch.float16"),
    ("GalleryIndex.search", {**TILE, **CPU_GALLERY, **_k(0)}, ValueError, "GalleryIndex.search: k = 0 is outside 1 .. min(N = 5, 128)"),
    ("GalleryIndex.search_grouped", CPU_GALLERY, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("GalleryIndex.search_grouped", CPU_NORMS, RuntimeError,
     "retrieval_topk_grouped_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_grouped)"),
    ("GalleryIndex.search_grouped", F64, ValueError,
     "retrieval_topk_grouped_device: a gallery of dtype torch.float64; it has to be torch.float32, torch.bfloat16 or torch.float16"),
    ("GalleryIndex.search_grouped", {**CPU_GALLERY, **NARROW}, ValueError, "GalleryIndex.search_grouped: queries of width 7, gallery of width 8"),
    ("GalleryIndex.search_multi", CPU_GALLERY, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("GalleryIndex.search_multi", CPU_NORMS, RuntimeError,
     "retrieval_topk_multi_device needs CUDA tensors (there is no CPU fallback; use compute_retrieval_topk_multi)"),
    ("GalleryIndex.search_multi", F64, ValueError,
     "retrieval_topk_multi_device: a gallery of dtype torch.float64; it has to be torch.float32, torch.bfloat16 or torch.float16"),
    ("GalleryIndex.search_multi", {**CPU_GALLERY, **_k(N + 1)}, ValueError, "GalleryIndex.search_multi: k = 6 is outside 1 .. min(N = 5, 128)"),
    # ---- queries that are not float32: asserted, with what each entry point shows
    ("retrieval_topk_device", Q64, AssertionError, "(torch.float64, torch.float32, (3, 8), (5, 8))"),
    ("retrieval_topk_index_device", Q64, AssertionError, "(torch.float64, (3, 8), (5, 8))"),
    ("retrieval_topk_grouped_device", Q64, AssertionError, "(torch.float64, (3, 8))"),
    ("retrieval_topk_multi_device", Q64, AssertionError, "torch.float64"),
    ("GalleryIndex.search", Q64, AssertionError, "(torch.float64, (3, 8))"),
    ("GalleryIndex.search", {**TILE, **Q64}, AssertionError, "(torch.float64, (20, 8))"),
    ("GalleryIndex.search", {"m": 70, "storage": torch.bfloat16, "code": 1, **Q64}, AssertionError, "(torch.float64, (70, 8))"),
    ("GalleryIndex.search_grouped", Q64, AssertionError, "(torch.float64, (3, 8))"),
    ("GalleryIndex.search_multi", Q64, AssertionError, "torch.float64"),
]


def test_the_arguments_every_row_starts_from_pass_the_host_checks():
    """Unchanged, they reach contiguous(): a row's refusal comes from the one argument it changes."""
    for entry in dict.fromkeys(r[0] for r in ROWS):
        with pytest.raises(AssertionError) as e:
            _call(entry, GOOD)
        assert str(e.value) == "the wrapper went past its host checks", entry


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{ROWS[i][0]}-{i}")
def test_refusal(row):
    entry, change, exc, text = ROWS[row]
    with pytest.raises(Exception) as e:
        _call(entry, {**GOOD, **change})
    print(f"{entry} {change}: {type(e.value).__name__}: {e.value}")
    assert type(e.value) is exc and str(e.value) == text
