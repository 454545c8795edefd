"""vptq_dequant_sliced without a GPU (added within ABI 11): the dense W straight from a layer's exact sliced layouts.  The header
declares the entry, the library exports it, the binding table carries it, the ABI number stays 11, and every validation error is
answered before anything is launched - over fake descriptors and layout structs, nothing dereferenced."""
import ctypes as C
import os
import re

from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _family_desc(I, O, v, k, kr, dt=0):
    """descriptor of a one-codebook layer with scale and bias (fake aligned pointers, never dereferenced)"""
    d = B.LayerDesc()
    ib, rb = k.bit_length() - 1, (kr.bit_length() - 1 if kr else 0)
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = k, kr, ib, rb
    d.row_words, d.num_indices, d.dtype = (I * (ib + rb) + 31) // 32, (O + v - 1) // v, dt
    d.indices, d.centroids, d.res_centroids = 1 << 20, 2 << 20, (3 << 20 if kr else None)
    d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    return d


def _layouts(buf, n, slices, res=True, whole=0):
    p = (C.addressof(buf) + 255) & ~255
    return (B.SlicedLayout * n)(*[B.SlicedLayout(p, p, p, p if res else None, 1, 1, slices, whole, None) for _ in range(n)]), p


def test_symbol_is_declared_exported_and_bound_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    assert re.search(r"VPTQ_API int vptq_dequant_sliced\(const VptqLayerDesc\* desc, const VptqSlicedLayout\* layouts, int parts, "
                     r"void\* W, void\* stream\);", hdr)
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    assert "vptq_dequant_sliced" in B.EXPORTS
    lib = B.lib()
    assert lib.vptq_abi_version() == B.ABI_VERSION == 12
    assert lib.vptq_dequant_sliced.argtypes == B.EXPORTS["vptq_dequant_sliced"][1]
    assert lib.vptq_dequant_sliced.argtypes == B.EXPORTS["vptq_sliced_layout_repack"][1]   # (what repack takes, W for the indices)


def test_validation_errors_without_gpu():
    lib = B.lib()
    dq = lib.vptq_dequant_sliced
    buf = (C.c_char * 1024)()
    d = _family_desc(8192, 8192, 8, 65536, 256)
    n = lib.vptq_sliced_layout_supported_for(d, B.GEMV_EXACT)
    assert n == 16
    lay, p = _layouts(buf, 3, n)

    def refused(rc, code, word):
        return rc == code and word in lib.vptq_last_error()

    assert refused(dq(d, None, 1, p, None), B.E_NULL, b"NULL")
    assert refused(dq(d, lay, 1, None, None), B.E_NULL, b"NULL")
    assert refused(dq(d, lay, 2, p, None), B.E_SHAPE, b"part")        # an 8192-column layer fits in one piece
    assert refused(dq(d, lay, 0, p, None), B.E_SHAPE, b"part")
    assert refused(dq(d, lay, 1, p + 8, None), B.E_ALIGN, b"aligned")
    bad, _ = _layouts(buf, 1, 8)
    assert refused(dq(d, bad, 1, p, None), B.E_SHAPE, b"n_slices")
    nores, _ = _layouts(buf, 1, n, res=False)
    assert refused(dq(d, nores, 1, p, None), B.E_NULL, b"res")
    # layouts of the folded form do not hold the packed stream: a whole table; the slice count of the folded answer
    whole, _ = _layouts(buf, 1, n, whole=1)
    assert refused(dq(d, whole, 1, p, None), B.E_UNSUPPORTED, b"whole_table")
    folded = lib.vptq_sliced_layout_supported(d)
    assert folded == 8 != n
    fl, _ = _layouts(buf, 1, folded)
    assert refused(dq(d, fl, 1, p, None), B.E_SHAPE, b"n_slices")
    # a 28672-column layer: two column parts, nothing else
    w = _family_desc(28672, 8192, 8, 65536, 256)
    nw = lib.vptq_sliced_layout_supported_for(_family_desc(14336, 8192, 8, 65536, 256), B.GEMV_EXACT)
    lay2, _ = _layouts(buf, 3, nw)
    assert refused(dq(w, lay2, 1, p, None), B.E_SHAPE, b"2 column part")
    assert dq(w, lay2, 3, p, None) == B.E_SHAPE
    # the second part's struct is checked too
    mixed = (B.SlicedLayout * 2)(lay2[0], bad[0])
    assert refused(dq(w, mixed, 2, p, None), B.E_SHAPE, b"n_slices")
    # formats without an exact layout: the canonical one, a small main codebook
    assert refused(dq(_family_desc(8192, 8192, 8, 256, 256), lay, 1, p, None), B.E_UNSUPPORTED, b"exact sliced layout")
    assert dq(_family_desc(8192, 8192, 8, 8192, 0), lay, 1, p, None) == B.E_UNSUPPORTED
    # a descriptor without indices pointer (a compacted layer passes its stand-in)
    d.indices = None
    assert dq(d, lay, 1, p, None) == B.E_NULL and lib.vptq_last_error()
