"""Host side of vptq_quant_gemm_gather (gemm_gather.hip; added within ABI 12), without a GPU: the symbols, the `_supported` truth
table, the entry's validation order (every error returns before a launch), the instance line printed from the launcher's own
decision, a census of the 2 x 3 x 2 instantiations against the lines, and the Python route function."""
import ctypes
import itertools
import math
import os
import re

from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gather_supported", "vptq_quant_gemm_gather", "vptq_quant_gemm_gather_instance")
TILE, R, WG_PER_CU, CUS = 1024, 2, 4, 256   # the kernel's column tile, vector-rows per row group, workgroups per CU; CUs without a device
X, Y = 9 << 20, 10 << 20                     # fake, aligned, never dereferenced


def desc(kr=256, I=4096, O=4096, v=8, k=65536, C=1, outliers=0, norm=True, dtype=0, perm=False):
    """a descriptor with fake aligned pointers (nothing is dereferenced by host logic)"""
    d = B.LayerDesc()
    ib, rb = int(math.log2(k)), (int(math.log2(kr)) if kr else 0)
    G = (I - outliers) // C
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, C, G
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = k, kr, ib, rb
    d.row_words, d.num_indices, d.dtype = (G * (ib + rb) + 31) // 32, (O + v - 1) // v, dtype
    d.indices, d.centroids = 1 << 20, 2 << 20
    d.res_centroids = (3 << 20) if kr else None
    if norm:
        d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    if perm:
        d.perm, d.scale_permuted, d.bias_permuted = 6 << 20, 7 << 20, 8 << 20
    if outliers:
        d.outlier_size, d.outlier_vector_len, d.num_outlier_centroids = outliers, v, 1024
        d.num_outlier_indices = d.num_indices
        d.outlier_indices, d.outlier_centroids = 11 << 20, 12 << 20
    return d


def line(d, tokens, flags=0):
    buf = ctypes.create_string_buffer(256)
    rc = B.lib().vptq_quant_gemm_gather_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"


def test_supported_truth_table():
    sup = B.lib().vptq_quant_gemm_gather_supported
    for kr, tokens in itertools.product((0, 256, 65536), (1, 16)):
        assert sup(desc(kr), tokens) == 1, (kr, tokens)
        assert sup(desc(kr, perm=True, dtype=1), tokens) == 1
    assert sup(None, 1) == 0
    for tokens in (0, 17, -1):
        assert sup(desc(256), tokens) == 0
    assert sup(desc(65536, v=16, O=16 * 256), 16) == 0                # v = 16
    assert sup(desc(256, k=256), 16) == 0                             # the canonical format
    assert sup(desc(4096), 16) == 0 and sup(desc(256, k=32768), 16) == 0   # other codebook sizes
    assert sup(desc(256, outliers=128), 16) == 0                      # outlier columns
    assert sup(desc(256, C=2), 16) == 0                               # two codebook groups
    assert sup(desc(256, norm=False), 16) == 0                        # no scale / bias
    assert sup(desc(0, I=4100), 16) == 0                              # G % 8 != 0
    for field in ("indices", "centroids", "res_centroids"):           # a table that is not 16-byte aligned
        d = desc(256)
        setattr(d, field, getattr(d, field) + 8)
        assert sup(d, 16) == 0, field
    d = desc(256, perm=True)
    d.scale_permuted = None                                           # a permutation without scale / bias in column order
    assert sup(d, 16) == 0
    # ... and the queries of the route it sits beside are what they were
    lib = B.lib()
    for kr in (0, 256, 65536):
        assert lib.vptq_quant_gemv_max_tokens(desc(kr)) == 8
        assert lib.vptq_quant_gemv_kernel_name(desc(kr), 16, 0) == b"gemv_gather_kernel"
        buf = ctypes.create_string_buffer(256)
        assert lib.vptq_quant_gemv_instance(desc(kr), 16, 0, buf, len(buf)) == 0 and b" tok=8 " in buf.value


def test_validation_order_null_tokens_unsupported():
    """every error is a VPTQ_E_* code: returned before a launch (there is no device here - a launch would answer with a HIP error)"""
    call = B.lib().vptq_quant_gemm_gather
    d, bad = desc(256), desc(256, k=256)
    assert call(None, X, Y, 4, 0, None) == B.E_NULL
    assert call(d, None, Y, 4, 0, None) == B.E_NULL and call(d, X, None, 4, 0, None) == B.E_NULL
    assert call(bad, None, Y, 17, 0, None) == B.E_NULL          # NULL before tokens before unsupported
    for tokens in (0, 17, -3):
        assert call(d, X, Y, tokens, 0, None) == B.E_TOKENS
        assert call(bad, X, Y, tokens, 0, None) == B.E_TOKENS   # tokens before unsupported
    assert call(bad, X, Y, 4, 0, None) == B.E_UNSUPPORTED
    assert call(desc(256, C=2), X, Y, 16, 0, None) == B.E_UNSUPPORTED
    for off in (2, 4, 8):
        assert call(d, X + off, Y, 4, 0, None) == B.E_UNSUPPORTED   # x not 16-byte aligned
    assert b"16-byte" in B.lib().vptq_last_error()
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(d, X + 8, Y, 4, flags, None) == B.E_UNSUPPORTED and call(d, X, Y, 17, flags, None) == B.E_TOKENS


def _want(d, T, tokens):
    groups = (d.num_indices + R - 1) // R
    grid = min(groups, CUS * WG_PER_CU)
    return (f"gemm_gather dt={'f16' if d.dtype == 0 else 'bf16'} t={T} perm={int(bool(d.perm))} tok={tokens} "
            f"tiles={(d.group_size + TILE - 1) // TILE} rgs={(groups + grid - 1) // grid}")


def test_instance_line_fields():
    cases = [(desc(0), 16, 1), (desc(256, I=8192, O=8192, dtype=1), 24, 9), (desc(65536, I=1032, O=20, perm=True), 32, 16),
             (desc(256, I=8, O=5), 24, 5), (desc(0, I=28672, O=8192 * 4, dtype=1, perm=True), 16, 12),
             (desc(65536, I=64, O=8 * (R * WG_PER_CU * CUS + 3) - 4), 32, 8)]
    for d, T, tokens in cases:
        rc, text = line(d, tokens)
        assert rc == 0 and text == _want(d, T, tokens), (text, _want(d, T, tokens))
    assert line(cases[0][0], 1)[1] == "gemm_gather dt=f16 t=16 perm=0 tok=1 tiles=4 rgs=1"
    assert line(cases[-1][0], 8)[1].endswith("tiles=1 rgs=2")       # more row groups than workgroups of the launch
    # flags that change nothing leave the line as it is
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert line(cases[1][0], 9, flags) == line(cases[1][0], 9)
    # the call's own errors, and a buffer that is too small
    assert line(desc(256), 17)[0] == B.E_TOKENS and line(desc(256, k=256), 4)[0] == B.E_UNSUPPORTED
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gather_instance(desc(256), 4, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""
    assert B.lib().vptq_quant_gemm_gather_instance(desc(256), 4, 0, None, 0) == B.E_NULL


def test_census_of_the_instantiations():
    """gemm_gather_kernel<DT, T, PERM>: 2 x 3 x 2 instantiations in the source, each reachable and named by a line"""
    src = open(os.path.join(ROOT, "vptq_amd", "csrc", "gemm_gather.hip")).read()
    assert re.search(r"template <typename DT, int T, bool PERM>\s*__global__", src)
    launched = set(re.findall(r"gemm_gather_kernel<DT, T, (true|false)>", src))
    assert launched == {"true", "false"}
    assert set(re.findall(r"case (\d+): return launch_mg<DT, \1>", src)) == {"16", "24", "32"}
    assert "launch_mg_dt<F16>" in src and "launch_mg_dt<BF16>" in src
    seen = set()
    for dtype, kr, perm in itertools.product((0, 1), (0, 256, 65536), (False, True)):
        rc, text = line(desc(kr, dtype=dtype, perm=perm), 16)
        assert rc == 0
        m = re.fullmatch(r"gemm_gather dt=(f16|bf16) t=(16|24|32) perm=([01]) tok=16 tiles=4 rgs=1", text)
        assert m, text
        assert m.groups() == ("f16" if dtype == 0 else "bf16", str({0: 16, 256: 24, 65536: 32}[kr]), str(int(perm)))
        seen.add(m.groups())
    assert len(seen) == 2 * 3 * 2
    assert "gemm_gather.hip" in open(os.path.join(ROOT, "vptq_amd", "csrc", "Makefile")).read()


def test_route_function_is_pure_and_bounded(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gather_route
    # formats the kernel does not have never route, whatever the shape and token count
    for tokens in range(0, 20):
        assert not route(16, 65536, 65536, 8192, 8192, tokens)
        assert not route(8, 256, 256, 8192, 8192, tokens)
        assert not route(8, 65536, 4096, 8192, 8192, tokens)
        assert not route(8, 32768, 0, 8192, 8192, tokens)
    for kr in (0, 256, 65536):
        for O, I in ((8192, 8192), (4096, 4096), (14336, 4096), (4096, 14336), (8192, 28672), (1024, 4096), (512, 2048)):
            for tokens in (0, 1, 4, 17, 64):
                assert not route(8, 65536, kr, O, I, tokens)       # outside 5 .. 16: never
            on = [t for t in range(5, 17) if route(8, 65536, kr, O, I, t)]
            assert on == list(range(on[0], 17)) if on else True      # from some token count on, up to 16
    # the knob: every supported format from 5 tokens / none
    monkeypatch.setattr(bd, "_GEMM_GATHER_MODE", "1")
    assert all(route(8, 65536, 256, 512, 2048, t) for t in range(5, 17)) and not route(8, 65536, 256, 512, 2048, 4)
    assert not route(8, 65536, 256, 512, 2048, 17) and not route(16, 65536, 0, 512, 2048, 12)
    monkeypatch.setattr(bd, "_GEMM_GATHER_MODE", "0")
    assert not any(route(8, 65536, kr, 8192, 8192, t) for kr in (0, 256, 65536) for t in range(0, 20))
