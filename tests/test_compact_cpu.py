"""Compact mode without a GPU: the repack entry point (vptq_sliced_layout_repack, added within ABI 11) is exported and validates
before launching, and the pure-torch model of the repack (`sliced.repack_reference`) rebuilds the packed indices bit for bit from
the exact layouts `layout_from_indices` builds - every total index width from 14 to 32 bits, 1 / 2 / 3 column parts."""
import ctypes as C
import os
import re

import pytest
import torch

from vptq_amd import _backend as B
from vptq_amd.utils.pack import pack_index
from vptq_amd.utils.sliced import layout_from_indices, repack_reference, tail_bits_clear

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


def test_repack_symbol_is_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    assert re.search(r"VPTQ_API int vptq_sliced_layout_repack\(", hdr)
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    assert "vptq_sliced_layout_repack" in B.EXPORTS
    lib = B.lib()
    assert lib.vptq_abi_version() == B.ABI_VERSION == 12
    assert lib.vptq_sliced_layout_repack.argtypes == B.EXPORTS["vptq_sliced_layout_repack"][1]


def _layouts(buf, n, slices, res=True):
    p = (C.addressof(buf) + 255) & ~255
    return (B.SlicedLayout * n)(*[B.SlicedLayout(p, p, p, p if res else None, 1, 1, slices, 0, None) for _ in range(n)]), p


def test_repack_validation_errors_without_gpu():
    lib = B.lib()
    rp = lib.vptq_sliced_layout_repack
    buf = (C.c_char * 1024)()
    d = _family_desc(8192, 8192, 8, 65536, 256)
    n = lib.vptq_sliced_layout_supported_for(d, B.GEMV_EXACT)
    assert n == 16
    lay, p = _layouts(buf, 3, n)
    assert rp(d, None, 1, p, None) == B.E_NULL and b"NULL" in lib.vptq_last_error()
    assert rp(d, lay, 1, None, None) == B.E_NULL and b"NULL" in lib.vptq_last_error()
    assert rp(d, lay, 2, p, None) == B.E_SHAPE and b"part" in lib.vptq_last_error()   # an 8192-column layer fits in one piece
    assert rp(d, lay, 1, p + 4, None) == B.E_ALIGN and b"aligned" in lib.vptq_last_error()
    bad, _ = _layouts(buf, 1, 8)
    assert rp(d, bad, 1, p, None) == B.E_SHAPE and b"n_slices" in lib.vptq_last_error()
    nores, _ = _layouts(buf, 1, n, res=False)
    assert rp(d, nores, 1, p, None) == B.E_NULL and b"res" in lib.vptq_last_error()
    # a 28672-column layer: two column parts, nothing else
    w = _family_desc(28672, 8192, 8, 65536, 256)
    nw = lib.vptq_sliced_layout_supported_for(_family_desc(14336, 8192, 8, 65536, 256), B.GEMV_EXACT)
    lay2, _ = _layouts(buf, 3, nw)
    assert rp(w, lay2, 1, p, None) == B.E_SHAPE and b"2 column part" in lib.vptq_last_error()
    assert rp(w, lay2, 3, p, None) == B.E_SHAPE
    # a format without an exact layout; a descriptor without indices pointer
    assert rp(_family_desc(8192, 8192, 8, 8192, 0), lay, 1, p, None) == B.E_UNSUPPORTED
    d.indices = None
    assert rp(d, lay, 1, p, None) == B.E_NULL


def _random_layer(N, G, ib, rb, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 1 << ib, (N, G), generator=g, dtype=torch.int64)
    # a few rows skewed onto one slice: lists that end in partial blocks of very different lengths
    idx[0, : G // 2] &= (1 << (ib - 3)) - 1
    ridx = torch.randint(0, 1 << rb, (N, G), generator=g, dtype=torch.int64) if rb else None
    as16 = lambda t: torch.where(t >= 32768, t - 65536, t).to(torch.int16)   # noqa: E731
    packed = pack_index(as16(idx)[None], ib, None if ridx is None else as16(ridx)[None], rb)
    return idx, ridx, packed


@pytest.mark.parametrize("ib,rb,side", [(14, 0, None), (16, 0, None), (14, 8, torch.uint8), (16, 8, torch.uint8),
                                        (16, 12, torch.int16), (16, 16, torch.int16), (15, 8, torch.int16)])
@pytest.mark.parametrize("G,parts,slices", [(8192, 1, 16), (200, 1, 8), (1032, 2, 16), (216, 3, 8), (96, 3, 32)])
def test_reference_repack_is_bit_exact(ib, rb, side, G, parts, slices):
    """T = 14, 16, 22, 24, 28, 32, 23: fields straddle words; G = 200 / 216 / 1032 are not multiples of 32, so parts share words"""
    N = 37
    idx, ridx, packed = _random_layer(N, G, ib, rb, seed=ib * 100 + rb + G)
    w = G // parts
    lays = [layout_from_indices(idx[:, p * w:(p + 1) * w].contiguous(), slices,
                                None if ridx is None else ridx[:, p * w:(p + 1) * w].contiguous(), ib,
                                side_dtype=side or torch.uint8) for p in range(parts)]
    assert bool(((lays[0][0] & 0xFFFF) == w).any())   # (lists that end in partial blocks: padding words to skip)
    got = repack_reference(lays, G, ib, rb, packed.shape[-1], slices)
    assert got.dtype == torch.int32 and got.shape == packed.shape
    assert torch.equal(got, packed)


def test_tail_bits_refusal():
    """bits past G T in a row cannot be held by a layout: compact() refuses such a layer, untouched"""
    from vptq_amd import VQuantLinear
    G, T = 200, 24
    _, _, packed = _random_layer(8, G, 16, 8, seed=3)
    assert tail_bits_clear(packed, G, T) and packed.shape[-1] == 150   # 200 x 24 bits = 150 whole words
    longer = torch.cat([packed, torch.zeros(1, 8, 1, dtype=torch.int32)], -1)
    assert tail_bits_clear(longer, G, T)
    longer[0, 3, -1] = 1                  # a word past the stream
    assert not tail_bits_clear(longer, G, T)
    G2 = 198                              # 198 x 24 = 4752 bits: the last word holds 16 of them, its bits 16 ... 31 must be zero
    _, _, p2 = _random_layer(4, G2, 16, 8, seed=4)
    assert tail_bits_clear(p2, G2, T)
    p2b = p2.clone()
    p2b[0, 2, -1] |= 1 << 20
    assert not tail_bits_clear(p2b, G2, T)
    m = VQuantLinear(G2, 32, [0, 8], [0, 65536], [-1, 256], 1, G2, 0, False, enable_norm=True, is_indice_packed=True,
                     enable_proxy_error=False, dtype=torch.float16)
    m.indices.data = p2b
    assert m.compact() == 0 and "past" in m.compact_skipped
    assert torch.equal(m.indices, p2b) and not m.is_compact()
    m.indices.data = p2
    assert m.compact() == 0 and "device" in m.compact_skipped   # (the next check: a layer on the CPU)
    m8 = VQuantLinear(64, 32, [0, 8], [0, 256], [-1, 256], 1, 64, 0, False, enable_norm=True, is_indice_packed=True,
                      enable_proxy_error=False, dtype=torch.float16)
    assert m8.compact() == 0 and "format" in m8.compact_skipped
