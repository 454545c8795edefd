"""Host side of vptq_quant_gemm_k256w (gemm_k256w_kernel in gemm_k256.hip; added within ABI 12), without a GPU: the symbols, the
`_supported` truth table, the entry's validation (every error returns before a launch), the instance line printed from the launcher's
own decision for every token-block count and pass shape, the Python route function, and the contract of vptq_quant_gemv beside it."""
import ctypes
import itertools
import os
import re

from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_k256w_supported", "vptq_quant_gemm_k256w", "vptq_quant_gemm_k256w_instance")
TILE, ROWS, CUS = 1024, 4, 256   # the kernel's column tile, vector-rows per row group; CUs without a device
X, Y = 9 << 20, 10 << 20         # fake, aligned, never dereferenced


def desc(I=4096, O=4096, k=256, kr=256, dtype=0, perm=False, perm_sb=True, norm=True):
    """a descriptor with fake aligned pointers (nothing is dereferenced by host logic)"""
    d = B.LayerDesc()
    ib, rb = k.bit_length() - 1, (kr.bit_length() - 1 if kr else 0)
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, 8, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = k, kr, ib, rb
    d.row_words, d.num_indices, d.dtype = (I * (ib + rb) + 31) // 32, (O + 7) // 8, dtype
    d.indices, d.centroids = 1 << 20, 2 << 20
    d.res_centroids = (3 << 20) if kr else None
    if norm:
        d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    if perm:
        d.perm = 6 << 20
        if perm_sb:
            d.scale_permuted, d.bias_permuted = 7 << 20, 8 << 20
    return d


def line(d, tokens, flags=0):
    buf = ctypes.create_string_buffer(256)
    rc = B.lib().vptq_quant_gemm_k256w_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def want_line(d, tokens, cus=CUS):
    """the line of (d, tokens): tb token blocks, one row group per pass"""
    groups = (d.num_indices + ROWS - 1) // ROWS
    grid = min(groups, cus)
    rgs, tb = (groups + grid - 1) // grid, (tokens + 15) // 16
    return f"gemm_k256w dt={'f16' if d.dtype == 0 else 'bf16'} perm={int(bool(d.perm))} tok={tokens} tb={tb} rgs={rgs} pass=1x{tb}"


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
    from vptq_amd import ops
    assert callable(ops.quant_gemm_k256w)


def test_supported_truth_table():
    sup = B.lib().vptq_quant_gemm_k256w_supported
    for dtype, perm, tokens in itertools.product((0, 1), (False, True), (17, 32, 33, 48, 49, 64)):
        assert sup(desc(dtype=dtype, perm=perm), tokens) == 1, (dtype, perm, tokens)
    assert sup(None, 32) == 0
    for tokens in (-1, 0, 1, 16, 65, 128):
        assert sup(desc(), tokens) == 0 and sup(desc(dtype=1), tokens) == 0, tokens
    assert sup(desc(k=65536), 32) == 0 and sup(desc(k=65536, kr=0), 32) == 0   # the large-codebook formats
    assert sup(desc(I=4100), 32) == 0                                          # group_size % 8 != 0
    assert sup(desc(perm=True, perm_sb=False), 32) == 0                        # a permutation without scale / bias in column order
    assert sup(desc(norm=False), 32) == 0                                      # no scale / bias


def test_validation_returns_before_a_launch():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error)"""
    call = B.lib().vptq_quant_gemm_k256w
    d, bad = desc(), desc(k=65536)
    assert call(None, X, Y, 32, 0, None) == B.E_NULL
    assert call(d, None, Y, 32, 0, None) == B.E_NULL and call(d, X, None, 32, 0, None) == B.E_NULL
    assert b"NULL" in B.lib().vptq_last_error()
    for tokens in (0, 1, 16, 65, -3):
        assert call(d, X, Y, tokens, 0, None) == B.E_TOKENS
        assert b"[17, 64]" in B.lib().vptq_last_error()
        assert call(bad, X, Y, tokens, 0, None) == B.E_TOKENS   # tokens before unsupported
    assert call(bad, X, Y, 32, 0, None) == B.E_UNSUPPORTED and b"gemm_k256w serves" in B.lib().vptq_last_error()
    assert call(desc(I=4100), X, Y, 32, 0, None) == B.E_UNSUPPORTED
    for off in (2, 4, 8):
        assert call(d, X + off, Y, 32, 0, None) == B.E_TOKENS   # x not 16-byte aligned
        assert b"16-byte" in B.lib().vptq_last_error()
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(d, X + 8, Y, 32, flags, None) == B.E_TOKENS and call(d, X, Y, 65, flags, None) == B.E_TOKENS


def test_instance_line_for_every_token_block_count_and_pass_shape():
    seen = set()
    # heights of 1, 2, 3, 4 and 5 row groups per workgroup on the 256 CUs assumed without a device, and two small layers
    shapes = [(4096, 32 * CUS * h) for h in (1, 2, 3, 4, 5)] + [(8, 5), (TILE + 8, 36), (64, 32 * CUS + 4)]
    for (I, O), tokens, dtype, perm in itertools.product(shapes, (17, 32, 33, 48, 49, 64), (0, 1), (False, True)):
        d = desc(I=I, O=O, dtype=dtype, perm=perm)
        rc, text = line(d, tokens)
        assert rc == 0 and text == want_line(d, tokens), (text, want_line(d, tokens))
        seen.add(text.split("pass=")[1])
    assert seen == {"1x2", "1x3", "1x4"}
    assert line(desc(I=8192, O=8192), 40)[1] == "gemm_k256w dt=f16 perm=0 tok=40 tb=3 rgs=1 pass=1x3"
    assert line(desc(I=4096, O=32 * CUS * 3, dtype=1, perm=True), 32)[1] == "gemm_k256w dt=bf16 perm=1 tok=32 tb=2 rgs=3 pass=1x2"
    assert line(desc(I=64, O=32 * CUS + 4), 64)[1].endswith("tb=4 rgs=2 pass=1x4")   # more row groups than workgroups
    # the name is not gemm_k256's: the views that count that kernel's lines do not see this one
    assert not line(desc(), 32)[1].startswith("gemm_k256 ")
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert line(desc(), 40, flags) == line(desc(), 40)
    # the call's own errors, and a buffer that is too small
    assert line(desc(), 16)[0] == B.E_TOKENS and line(desc(), 65)[0] == B.E_TOKENS and line(desc(k=65536), 32)[0] == B.E_UNSUPPORTED
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_k256w_instance(desc(), 32, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""
    assert B.lib().vptq_quant_gemm_k256w_instance(desc(), 32, 0, None, 0) == B.E_NULL


def test_census_of_the_instantiations():
    """gemm_k256w_kernel<DT, PERM, TB>: 2 x 2 x 3 instantiations, each launched from the decision the line prints"""
    src = open(os.path.join(ROOT, "vptq_amd", "csrc", "gemm_k256.hip")).read()
    assert re.search(r"template <typename DT, bool PERM, int TB>\s*__global__", src)
    assert set(re.findall(r"case (\d): return launch_gw<DT, PERM, \1>", src)) == {"2", "3", "4"}
    assert set(re.findall(r"launch_gw_tb<(\w+), (true|false)>", src)) == set(itertools.product(("F16", "BF16"), ("true", "false")))
    assert set(re.findall(r"gemm_k256_pass<DT, PERM, (\d), TB>", src)) == {"1"}


def test_route_function_is_pure_and_follows_the_cells(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_k256w_route
    shapes = ((8192, 8192), (4096, 4096), (14336, 4096), (4096, 14336), (28672, 8192), (512, 2048), (36, 1032))
    for O, I in shapes:
        for tokens in (-1, 0, 1, 5, 16, 65, 128, 512):
            assert not route(O, I, tokens)                         # outside 17 .. 64: never
        on = [t for t in range(17, 65) if route(O, I, t)]
        assert on == list(range(on[0], on[-1] + 1)) if on else True   # the routed token counts of a layer are one interval
        n_el = ((O + 7) // 8) * I
        for t in range(17, 65):                                     # auto: the committed cells, nothing else
            assert route(O, I, t) == any(n_el >= e and lo <= t <= hi for e, lo, hi in bd._GEMM_K256W_CELLS)
    monkeypatch.setattr(bd, "_GEMM_K256W_MODE", "1")
    assert all(route(36, 1032, t) for t in range(17, 65)) and not route(36, 1032, 16) and not route(8192, 8192, 65)
    monkeypatch.setattr(bd, "_GEMM_K256W_MODE", "0")
    assert not any(route(O, I, t) for O, I in shapes for t in range(0, 70))


def test_the_contract_of_vptq_quant_gemv_is_what_it_was():
    lib = B.lib()
    for dtype in (0, 1):
        d = desc(I=8192, O=8192, dtype=dtype)
        assert lib.vptq_quant_gemv_max_tokens(d) == 48
        for tokens in (17, 40):
            assert lib.vptq_quant_gemv_kernel_name(d, tokens, B.GEMV_EXACT) == b"gemm_k256_kernel"
        buf = ctypes.create_string_buffer(256)
        assert lib.vptq_quant_gemv_instance(d, 40, B.GEMV_EXACT, buf, len(buf)) == 0
        assert buf.value.decode() == f"gemm_k256 dt={'f16' if dtype == 0 else 'bf16'} perm=0 tok=16 passes=1"
