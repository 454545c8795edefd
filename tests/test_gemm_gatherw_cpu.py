"""Host side of vptq_quant_gemm_gatherw (gemm_gatherw_kernel in gemm_gatherw.hip; added within ABI 12), without a GPU: the symbols,
the `_supported` truth table, the entry's validation (every error returns before a launch), the instance line printed from the
launcher's own decision for every (T, TB, perm, dtype), the census of the 24 instantiations, the Python route function, and the
contract of vptq_quant_gemm_gather beside it."""
import ctypes
import itertools
import os
import re

from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gatherw_supported", "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gatherw_instance")
TILE, ROWS, CUS, WG_PER_CU = 1024, 2, 256, 4   # the kernel's column tile, vector-rows per row group; CUs without a device
X, Y = 9 << 20, 10 << 20                       # fake, aligned, never dereferenced
KRS = (0, 256, 65536)


def desc(I=4096, O=4096, v=8, k=65536, kr=256, dtype=0, perm=False, perm_sb=True, norm=True):
    """a descriptor with fake aligned pointers (nothing is dereferenced by host logic)"""
    d = B.LayerDesc()
    ib, rb = k.bit_length() - 1, (kr.bit_length() - 1 if kr else 0)
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = k, kr, ib, rb
    d.row_words, d.num_indices, d.dtype = (I * (ib + rb) + 31) // 32, (O + v - 1) // v, dtype
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
    rc = B.lib().vptq_quant_gemm_gatherw_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def want_line(d, tokens, cus=CUS):
    groups = (d.num_indices + ROWS - 1) // ROWS
    grid = min(groups, cus * WG_PER_CU)
    rgs, tb = (groups + grid - 1) // grid, (tokens + 15) // 16
    T = {0: 16, 256: 24, 65536: 32}[d.num_res_centroids]
    return (f"gemm_gatherw dt={'f16' if d.dtype == 0 else 'bf16'} t={T} perm={int(bool(d.perm))} tok={tokens} tb={tb} "
            f"tiles={(d.group_size + TILE - 1) // TILE} rgs={rgs}")


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
    import sys
    assert callable(ops.quant_gemm_gatherw) and "quant_gemm_gatherw" in sys.modules["vptq_amd.ops.quant_gemm"].__all__


def test_supported_truth_table():
    sup = B.lib().vptq_quant_gemm_gatherw_supported
    for dtype, kr, perm, tokens in itertools.product((0, 1), KRS, (False, True), (17, 32, 33, 48)):
        assert sup(desc(dtype=dtype, kr=kr, perm=perm), tokens) == 1, (dtype, kr, perm, tokens)
    assert sup(None, 32) == 0
    for tokens, kr in itertools.product((-1, 0, 1, 16, 49, 64), KRS):
        assert sup(desc(kr=kr), tokens) == 0 and sup(desc(kr=kr, dtype=1), tokens) == 0, (tokens, kr)
    assert sup(desc(k=256, kr=256), 32) == 0                                   # the canonical format
    assert sup(desc(v=16), 32) == 0 and sup(desc(v=16, kr=65536), 32) == 0     # gemm_gatherx's formats
    assert sup(desc(kr=4096), 32) == 0
    assert sup(desc(I=4100), 32) == 0                                          # in_features % 8 != 0
    assert sup(desc(perm=True, perm_sb=False), 32) == 0                        # a permutation without scale / bias in column order
    assert sup(desc(norm=False), 32) == 0                                      # no scale / bias


def test_validation_returns_before_a_launch():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error)"""
    call = B.lib().vptq_quant_gemm_gatherw
    d, bad = desc(), desc(k=256)
    assert call(None, X, Y, 32, 0, None) == B.E_NULL
    assert call(d, None, Y, 32, 0, None) == B.E_NULL and call(d, X, None, 32, 0, None) == B.E_NULL
    assert b"NULL" in B.lib().vptq_last_error()
    for tokens in (0, 1, 16, 49, 64, -3):
        assert call(d, X, Y, tokens, 0, None) == B.E_TOKENS
        assert b"[17, 48]" in B.lib().vptq_last_error()
        assert call(bad, X, Y, tokens, 0, None) == B.E_TOKENS   # tokens before unsupported
    assert call(bad, X, Y, 32, 0, None) == B.E_UNSUPPORTED and b"gemm_gatherw serves" in B.lib().vptq_last_error()
    assert call(desc(I=4100), X, Y, 32, 0, None) == B.E_UNSUPPORTED and call(desc(v=16), X, Y, 32, 0, None) == B.E_UNSUPPORTED
    for off in (2, 4, 8):
        assert call(d, X + off, Y, 32, 0, None) == B.E_TOKENS   # x not 16-byte aligned
        assert b"16-byte" in B.lib().vptq_last_error()
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(d, X + 8, Y, 32, flags, None) == B.E_TOKENS and call(d, X, Y, 49, flags, None) == B.E_TOKENS


def test_instance_line_for_every_instantiation():
    seen = set()
    # heights of 1, 2 and 3 row groups per workgroup on the 256 CUs (4 workgroups each) assumed without a device, and small layers
    per_wave = 8 * ROWS * CUS * WG_PER_CU   # outputs of one full grid of row groups
    shapes = [(4096, per_wave * h) for h in (1, 2, 3)] + [(8, 5), (TILE + 8, 20), (64, per_wave + 4), (2 * TILE + 264, 36)]
    for (I, O), kr, tokens, dtype, perm in itertools.product(shapes, KRS, (17, 32, 33, 48), (0, 1), (False, True)):
        d = desc(I=I, O=O, kr=kr, dtype=dtype, perm=perm)
        rc, text = line(d, tokens)
        assert rc == 0 and text == want_line(d, tokens), (text, want_line(d, tokens))
        f = dict(p.split("=") for p in text.split()[1:])
        seen.add((f["dt"], f["t"], f["perm"], f["tb"]))
    assert seen == set(itertools.product(("f16", "bf16"), ("16", "24", "32"), ("0", "1"), ("2", "3"))) and len(seen) == 24
    assert line(desc(I=8192, O=8192), 40)[1] == "gemm_gatherw dt=f16 t=24 perm=0 tok=40 tb=3 tiles=8 rgs=1"
    assert line(desc(I=4096, O=per_wave * 3, kr=65536, dtype=1, perm=True), 32)[1] == "gemm_gatherw dt=bf16 t=32 perm=1 tok=32 tb=2 tiles=4 rgs=3"
    assert line(desc(I=64, O=per_wave + 4, kr=0), 17)[1] == "gemm_gatherw dt=f16 t=16 perm=0 tok=17 tb=2 tiles=1 rgs=2"
    # the name is not gemm_gather's: the views that count that kernel's lines do not see this one
    assert not line(desc(), 32)[1].startswith("gemm_gather ") and line(desc(), 32)[1].startswith("gemm_gatherw ")
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert line(desc(), 40, flags) == line(desc(), 40)
    # the call's own errors, and a buffer that is too small
    assert line(desc(), 16)[0] == B.E_TOKENS and line(desc(), 49)[0] == B.E_TOKENS and line(desc(k=256), 32)[0] == B.E_UNSUPPORTED
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gatherw_instance(desc(), 32, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""
    assert B.lib().vptq_quant_gemm_gatherw_instance(desc(), 32, 0, None, 0) == B.E_NULL
    assert B.lib().vptq_quant_gemm_gatherw_instance(None, 32, 0, small, len(small)) == B.E_NULL


def test_census_of_the_instantiations_and_the_makefile_entry():
    """gemm_gatherw_kernel<DT, T, PERM, TB>: 2 x 3 x 2 x 2 instantiations in a compile unit of its own, each launched from the
    decision the line prints; gemm_gather.hip does not know it"""
    csrc = os.path.join(ROOT, "vptq_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_gatherw.hip")).read()
    assert re.search(r"template <typename DT, int T, bool PERM, int TB>\s*__global__", src)
    assert set(re.findall(r"gemm_gatherw_kernel<DT, T, (true|false), TB>", src)) == {"true", "false"}
    assert set(re.findall(r"case (\d+): return launch_gw<DT, \1, TB>", src)) == {"16", "24", "32"}
    assert set(re.findall(r"launch_gw_t<DT, (\d)>", src)) == {"2", "3"}
    assert set(re.findall(r"launch_gw_dt<(\w+)>", src)) == {"F16", "BF16"}
    assert "static_assert(TB == 2 || TB == 3" in src
    for phase in ("gt_dcol", "gt_load_sb", "gt_load_a1", "gt_rebuild", "gt_write_tile", "gt_epilogue", "mfma16x16x32<DT>"):
        assert phase in src, phase
    assert "atomic" not in src.split("#include")[1]
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert srcs.count("gemm_gatherw.hip") == 1
    assert "gatherw" not in open(os.path.join(csrc, "gemm_gather.hip")).read()


def test_route_function_is_pure_and_follows_the_cells(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gatherw_route
    assert (vq.GEMM_GATHERW_MIN_TOKENS, vq.GEMM_GATHERW_MAX_TOKENS) == (17, 48)
    assert all(len(c) == 4 and c[0] in KRS and c[1] >= 4 << 20 and 17 <= c[2] <= c[3] <= 48 for c in bd._GEMM_GATHERW_CELLS)
    shapes = ((8192, 8192), (4096, 4096), (14336, 4096), (4096, 14336), (28672, 8192), (512, 2048), (36, 1032))
    for (O, I), kr in itertools.product(shapes, KRS):
        for tokens in (-1, 0, 1, 5, 16, 49, 64, 128):
            assert not route(8, 65536, kr, O, I, tokens)               # outside 17 .. 48: never
        on = [t for t in range(17, 49) if route(8, 65536, kr, O, I, t)]
        assert on == list(range(on[0], on[-1] + 1)) if on else True   # the routed token counts of a layer are one interval
        n_el = ((O + 7) // 8) * I
        if n_el < 4 << 20:
            assert not on, (O, I, kr)                                  # no cell under 4 M index elements
        for t in range(17, 49):                                        # auto: the committed cells, nothing else
            assert route(8, 65536, kr, O, I, t) == any(
                c == kr and n_el >= max(e, 4 << 20) and lo <= t <= hi for c, e, lo, hi in bd._GEMM_GATHERW_CELLS)
    for t in range(17, 49):   # other formats: never
        assert not route(8, 256, 256, 8192, 8192, t) and not route(16, 65536, 0, 8192, 8192, t) and not route(8, 65536, 4096, 8192, 8192, t)
    monkeypatch.setattr(bd, "_GEMM_GATHERW_MODE", "1")
    assert all(route(8, 65536, kr, 36, 1032, t) for kr in KRS for t in range(17, 49))
    assert not route(8, 65536, 256, 36, 1032, 16) and not route(8, 65536, 256, 8192, 8192, 49) and not route(16, 65536, 0, 8192, 8192, 32)
    monkeypatch.setattr(bd, "_GEMM_GATHERW_MODE", "0")
    assert not any(route(8, 65536, kr, O, I, t) for O, I in shapes for kr in KRS for t in range(0, 70))


def test_the_16_token_entry_and_its_route_are_what_they_were():
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    lib = B.lib()
    for dtype, kr in itertools.product((0, 1), KRS):
        d = desc(I=8192, O=8192, kr=kr, dtype=dtype)
        assert lib.vptq_quant_gemm_gather_supported(d, 16) == 1 and lib.vptq_quant_gemm_gather_supported(d, 17) == 0
        assert lib.vptq_quant_gemm_gather(d, X, Y, 17, 0, None) == B.E_TOKENS
        assert not vq.gemm_gather_route(8, 65536, kr, 8192, 8192, 17) and not vq.gemm_gather_route(8, 65536, kr, 8192, 8192, 64)
        buf = ctypes.create_string_buffer(256)
        assert lib.vptq_quant_gemm_gather_instance(d, 16, 0, buf, len(buf)) == 0 and buf.value.startswith(b"gemm_gather dt=")
