"""The device-side layout builder without a GPU: vptq_sliced_layout_plan / vptq_sliced_layout_fill (added within ABI 11) are declared,
exported and bound, they validate before launching, and the public `prepare` step exists and leaves a CPU layer untouched."""
import ctypes as C
import os
import re

import torch

import vptq_amd
from vptq_amd import VQuantLinear
from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _family_desc(I, O, v, k, kr):
    """descriptor of a large-codebook layer (fake aligned pointers, never dereferenced)"""
    d = B.LayerDesc()
    ib, rb = k.bit_length() - 1, (kr.bit_length() - 1 if kr else 0)
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = k, kr, ib, rb
    d.row_words, d.num_indices, d.dtype = (I * (ib + rb) + 31) // 32, (O + v - 1) // v, 0
    d.indices, d.centroids, d.res_centroids = 1 << 20, 2 << 20, (3 << 20 if kr else None)
    d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    return d


def _spec(flags, slices, table=0, whole=0, side=0, parts=1, part=0):
    return B.SlicedLayoutSpec(flags, slices, table, whole, side, parts, part, 0)


def test_builder_symbols_are_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    lib = B.lib()
    assert lib.vptq_abi_version() == B.ABI_VERSION == 12
    for name in ("vptq_sliced_layout_plan", "vptq_sliced_layout_fill"):
        assert re.search(r"VPTQ_API int %s\(" % name, hdr), name
        assert name in B.EXPORTS
        assert getattr(lib, name).argtypes == B.EXPORTS[name][1] and getattr(lib, name).restype is C.c_int
    assert re.search(r"#define VPTQ_LAYOUT_ANY_SHAPE \(1 << 16\)", hdr) and B.LAYOUT_ANY_SHAPE == 1 << 16
    # the spec struct: eight int32 in the header's order
    body = re.search(r"typedef struct VptqSlicedLayoutSpec \{(.*?)\} VptqSlicedLayoutSpec;", hdr, re.S).group(1)
    assert re.findall(r"int32_t (\w+);", body) == [f[0] for f in B.SlicedLayoutSpec._fields_]
    assert C.sizeof(B.SlicedLayoutSpec) == 32


def test_builder_validation_errors_without_gpu():
    lib = B.lib()
    plan, fill = lib.vptq_sliced_layout_plan, lib.vptq_sliced_layout_fill
    err = lib.vptq_last_error
    buf = (C.c_char * 1024)()
    p = (C.addressof(buf) + 255) & ~255
    d = _family_desc(8192, 8192, 8, 65536, 256)
    n = lib.vptq_sliced_layout_supported_for(d, B.GEMV_EXACT)
    assert n == 16 and lib.vptq_sliced_layout_supported_for(d, 0) == 8
    ok = _spec(B.GEMV_EXACT, n, side=1)
    lay = lambda e=p, r=p, s=n: B.SlicedLayout(e, p, p, r, 1, 1, s, 0, p)   # noqa: E731
    # NULL outputs / spec
    assert plan(d, None, p, p, p, p, None) == B.E_NULL and b"NULL" in err()
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert plan(d, ok, *a, None) == B.E_NULL and b"NULL" in err()
    assert fill(d, ok, None, 1, None) == B.E_NULL and b"NULL" in err()
    assert fill(d, ok, lay(e=None), 1, None) == B.E_NULL and b"NULL" in err()
    assert fill(d, ok, lay(r=None), 1, None) == B.E_NULL and b"res" in err()
    # a slice count other than the layer's (exact: 16, folded: 8)
    assert plan(d, _spec(B.GEMV_EXACT, 8, side=1), p, p, p, p, None) == B.E_SHAPE and b"n_slices" in err()
    assert plan(d, _spec(0, 16, side=1), p, p, p, p, None) == B.E_SHAPE and b"n_slices" in err()
    assert plan(d, _spec(B.GEMV_EXACT, 12, side=1), p, p, p, p, None) == B.E_SHAPE
    assert fill(d, ok, lay(s=8), 1, None) == B.E_SHAPE and b"n_slices" in err()
    # a format without a layout
    assert plan(_family_desc(8192, 8192, 8, 8192, 0), _spec(B.GEMV_EXACT, 8), p, p, p, p, None) == B.E_UNSUPPORTED
    assert plan(_family_desc(8192, 8192, 8, 8192, 0), _spec(0, 8), p, p, p, p, None) == B.E_UNSUPPORTED
    # a side stream / table / whole_table the layer's layouts do not have
    assert plan(d, _spec(B.GEMV_EXACT, n, side=2), p, p, p, p, None) == B.E_UNSUPPORTED and b"side_bytes" in err()
    assert plan(d, _spec(B.GEMV_EXACT, n, table=1), p, p, p, p, None) == B.E_UNSUPPORTED
    assert plan(d, _spec(0, 8, side=1, whole=1), p, p, p, p, None) == B.E_UNSUPPORTED and b"whole_table" in err()
    # misaligned outputs
    assert fill(d, ok, lay(e=p + 4), 1, None) == B.E_ALIGN and b"aligned" in err()
    assert plan(d, ok, p + 2, p, p, p, None) == B.E_ALIGN and b"aligned" in err()
    assert plan(d, ok, p, p, p, p + 4, None) == B.E_ALIGN
    # a part count other than the layer's: an 8192-column layer fits in one piece, a 28672-column one takes two
    assert plan(d, _spec(B.GEMV_EXACT, n, side=1, parts=2), p, p, p, p, None) == B.E_SHAPE and b"part" in err()
    w = _family_desc(28672, 8192, 8, 65536, 256)
    nw = lib.vptq_sliced_layout_supported_for(_family_desc(14336, 8192, 8, 65536, 256), B.GEMV_EXACT)
    assert plan(w, _spec(B.GEMV_EXACT, nw, side=1), p, p, p, p, None) == B.E_SHAPE and b"2 column part" in err()
    assert plan(w, _spec(B.GEMV_EXACT, nw, side=1, parts=3), p, p, p, p, None) == B.E_SHAPE
    assert plan(w, _spec(B.GEMV_EXACT, nw, side=1, parts=2, part=2), p, p, p, p, None) == B.E_SHAPE
    assert plan(w, _spec(0, 16, side=1, parts=2), p, p, p, p, None) == B.E_SHAPE   # (column parts: exact layouts only)
    # a descriptor without indices
    d.indices = None
    assert plan(d, ok, p, p, p, p, None) == B.E_NULL


def test_prepare_exists_and_leaves_a_cpu_layer_untouched():
    assert callable(vptq_amd.prepare_model) and "prepare_model" in vptq_amd.__all__ and callable(VQuantLinear.prepare)
    m = VQuantLinear(64, 32, [0, 8], [0, 65536], [-1, 256], 1, 64, 0, False, enable_norm=True, is_indice_packed=True,
                     enable_proxy_error=False, dtype=torch.float16)
    before = {k: (v.data_ptr(), v._version, v.device) for k, v in m.state_dict().items()}   # (same storages, never written)
    keys = set(m.__dict__)
    rep = m.prepare()
    assert rep["built"] == "indices are not on a ROCm device" and rep["bytes"] == 0 and rep["seconds"] >= 0
    assert set(m.__dict__) == keys and "_sliced" not in m.__dict__ and "_desc_cache" not in m.__dict__
    after = m.state_dict()
    assert after.keys() == before.keys() and all((after[k].data_ptr(), after[k]._version, after[k].device) == before[k] for k in before)
    model = torch.nn.Sequential(m, torch.nn.ReLU())
    rep = vptq_amd.prepare_model(model)
    assert set(rep["layers"]) == {"0"} and rep["built"] == 0 and rep["bytes"] == 0
    assert rep["layers"]["0"]["built"] == "indices are not on a ROCm device"
