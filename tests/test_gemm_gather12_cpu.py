"""Host side of vptq_quant_gemm_gather12 (gemm_gather12.hip; added within ABI 12), without a GPU: symbols, `_supported`, the workspace
query, validation before any launch, the instance line, the route function and the third route table."""
import ctypes
import itertools
import os
import re

from test_gemm_gather_cpu import desc, X, Y, CUS   # the descriptor with fake aligned pointers; nothing is dereferenced by host logic
from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gather12_supported", "vptq_quant_gemm_gather12_workspace_bytes", "vptq_quant_gemm_gather12",
           "vptq_quant_gemm_gather12_instance")
TILE, TILE_BYTES, RES_LDS_MAX, LDS_PER_CU, REG_WG_PER_CU = 512, 49152, 32768, 160 * 1024, 2   # the kernel's constants
FORMATS = [(65536, 0), (65536, 256), (32768, 1024), (65536, 4096)]                             # (main, residual centroids) of v = 12
WS = 1 << 24                                                                                   # a fake, aligned workspace


def fdesc(k, kr, v=12, **kw):
    kw.setdefault("O", 4092)
    return desc(kr, v=v, k=k, **kw)


def line(d, tokens, flags=0):
    buf = ctypes.create_string_buffer(256)
    rc = B.lib().vptq_quant_gemm_gather12_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def want(d, tokens, cus=CUS):
    """the launches (gemm_gather_px_decide, gemm_gather12_decide), restated"""
    res_bytes = d.num_res_centroids * 24
    res = "none" if res_bytes == 0 else "lds" if res_bytes <= RES_LDS_MAX else "l2"
    wgcu = min(REG_WG_PER_CU, LDS_PER_CU // (TILE_BYTES + (res_bytes if res == "lds" else 0)))
    groups = (d.num_indices + 3) // 4
    grid = min(groups, cus * wgcu)
    G = d.group_size
    px = f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + 63) // 64}x{(tokens + 3) // 4} tpt=4 | " if d.perm else ""
    return (f"{px}gemm_gather12 dt={'f16' if d.dtype == 0 else 'bf16'} ib={d.index_bits} rb={d.res_bits} res={res} tok={tokens} "
            f"tiles={(G + TILE - 1) // TILE} wgcu={wgcu} rgs={(groups + grid - 1) // grid}")


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    from vptq_amd import ops
    assert callable(ops.quant_gemm_gather12)
    assert "gemm_gather12.hip" in open(os.path.join(ROOT, "vptq_amd", "csrc", "Makefile")).read()


def test_supported_truth_table_and_workspace_query():
    sup, ws = B.lib().vptq_quant_gemm_gather12_supported, B.lib().vptq_quant_gemm_gather12_workspace_bytes
    for (k, kr), tokens in itertools.product(FORMATS, range(-1, 19)):
        inside = 1 <= tokens <= 16
        assert sup(fdesc(k, kr), tokens) == int(inside) and sup(fdesc(k, kr, perm=True, dtype=1), tokens) == int(inside), (k, kr, tokens)
        assert ws(fdesc(k, kr), tokens) == 0
        assert ws(fdesc(k, kr, perm=True), tokens) == (((tokens * 4096 * 2 + 255) // 256) * 256 if inside else 0)
    assert ws(fdesc(65536, 4096, I=4104, perm=True), 5) == 41216 and sup(None, 1) == 0 and ws(None, 1) == 0   # (5 x 4104 x 2 = 41040, rounded)
    assert sup(fdesc(65536, 4096, v=8, O=4096), 16) == 0 and sup(fdesc(65536, 1024, v=16, O=4096), 16) == 0   # v = 8 / 16
    assert sup(fdesc(8192, 256), 16) == 0 and sup(fdesc(256, 256), 16) == 0      # k < 16384
    assert sup(fdesc(65536, 4096, C=2), 16) == 0                                 # two codebook groups
    assert sup(fdesc(65536, 4096, outliers=128), 16) == 0                        # outlier columns
    assert sup(fdesc(65536, 4096, norm=False), 16) == 0                          # no scale / bias
    assert sup(fdesc(65536, 0, I=4100), 16) == 0                                 # G % 8 != 0
    d = fdesc(65536, 4096, perm=True)
    d.scale_permuted = None                                                      # a permutation without scale / bias in column order
    assert sup(d, 16) == 0 and ws(d, 16) == 0
    d = fdesc(65536, 4096)
    d.row_words -= 1                                                             # a row shorter than its G x T bits
    assert sup(d, 16) == 0
    for field, off, ok in (("centroids", 8, 1), ("res_centroids", 8, 1), ("centroids", 4, 0), ("res_centroids", 4, 0), ("indices", 8, 0)):
        d = fdesc(65536, 4096)                                                   # entries are 8-byte aligned, indices 16
        setattr(d, field, getattr(d, field) + off)
        assert sup(d, 16) == ok, (field, off)
    # the entries beside it are what they were: none of them takes v = 12, and one to four tokens stay gemv_gatherx's
    lib = B.lib()
    for k, kr in FORMATS:
        assert lib.vptq_quant_gemm_gatherx_supported(fdesc(k, kr), 16) == 0 and lib.vptq_quant_gemm_gather_supported(fdesc(k, kr), 16) == 0
        assert lib.vptq_quant_gemm_gather_px_supported(fdesc(k, kr, perm=True), 16) == 0
        assert lib.vptq_quant_gemv_kernel_name(fdesc(k, kr), 4, 0) == b"gemv_gatherx_kernel"


def test_validation_order_before_any_launch():
    """every error is a VPTQ_E_* code: returned before a launch (there is no device here - a launch would answer with a HIP error)"""
    call = B.lib().vptq_quant_gemm_gather12
    d, p, bad = fdesc(65536, 4096), fdesc(65536, 4096, perm=True), fdesc(65536, 4096, v=8, O=4096)
    need = B.lib().vptq_quant_gemm_gather12_workspace_bytes(p, 12)
    assert call(None, X, Y, 4, 0, None, 0, None) == B.E_NULL
    assert call(d, None, Y, 4, 0, None, 0, None) == B.E_NULL and call(d, X, None, 4, 0, None, 0, None) == B.E_NULL
    assert call(bad, None, Y, 17, 0, None, 0, None) == B.E_NULL        # NULL before tokens before unsupported
    for tokens in (0, 17, -3):
        assert call(d, X, Y, tokens, 0, None, 0, None) == B.E_TOKENS and call(bad, X, Y, tokens, 0, None, 0, None) == B.E_TOKENS
    assert call(bad, X + 8, Y, 4, 0, None, 0, None) == B.E_UNSUPPORTED   # unsupported before x alignment
    for flags in (0, B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(d, X + 8, Y, 4, flags, None, 0, None) == B.E_ALIGN and b"x must be 16-byte" in B.lib().vptq_last_error()
        assert call(p, X, Y, 12, flags, None, 0, None) == B.E_WORKSPACE and call(p, X, Y, 12, flags, WS, need - 1, None) == B.E_WORKSPACE
        assert call(p, X, Y, 12, flags, WS + 8, need, None) == B.E_ALIGN
    assert line(d, 17)[0] == B.E_TOKENS and line(bad, 4)[0] == B.E_UNSUPPORTED
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gather12_instance(d, 4, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""


def test_instance_line_fields():
    cases = [(fdesc(65536, 0), 1), (fdesc(65536, 256, I=8192, O=8192, dtype=1), 9), (fdesc(32768, 1024, I=520, O=56, perm=True), 16),
             (fdesc(65536, 4096, I=28672, O=8184, dtype=1, perm=True), 12), (fdesc(65536, 4096, I=8, O=5), 5),
             (fdesc(65536, 0, I=64, O=48 * (2 * CUS + 3) - 8), 8)]
    for d, tokens in cases:
        assert line(d, tokens) == (0, want(d, tokens)), (line(d, tokens), want(d, tokens))
    assert line(*cases[0])[1] == "gemm_gather12 dt=f16 ib=16 rb=0 res=none tok=1 tiles=8 wgcu=2 rgs=1"       # the register bound, not 48 KiB
    assert line(*cases[2])[1] == "permute_x_tokens g=520 tok=16 grid=2x4 tpt=4 | gemm_gather12 dt=f16 ib=15 rb=10 res=lds tok=16 tiles=2 wgcu=2 rgs=1"
    assert " res=l2 " in line(*cases[3])[1] and line(*cases[5])[1].endswith("tiles=1 wgcu=2 rgs=2")          # a 96 KiB table: from L2


SHAPES = ((8184, 8192), (4092, 4096), (14328, 4096), (4092, 14336), (8184, 28672), (516, 2048))


def test_route_function_and_the_third_table(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gather12_route
    assert bd._GEMM_GATHER12_MODE == "auto"          # (the knob is read with VPTQ_TUNING=1 only)
    assert '_GEMM_GATHER12_MODE = (B.tune_env("VPTQ_GEMM_GATHER12", "auto") or "auto").strip().lower()' in open(bd.__file__).read()
    for mode, perm in itertools.product(("auto", "1", "0"), (None, False, True)):
        monkeypatch.setattr(bd, "_GEMM_GATHER12_MODE", mode)
        for tokens in range(0, 20):
            assert not route(8, 65536, 4096, 8192, 8192, tokens, perm) and not route(16, 65536, 1024, 8192, 8192, tokens, perm)
            assert not route(6, 65536, 4096, 8190, 8192, tokens, perm) and not route(12, 8192, 256, 8184, 8192, tokens, perm)
            assert not route(12, 65536, 4096, 8184, 8196, tokens, perm) and not route(12, 65536, 1000, 8184, 8192, tokens, perm)
        for (k, kr), (O, I), tokens in itertools.product(FORMATS, SHAPES, (0, 1, 4, 17, 48)):
            assert not route(12, k, kr, O, I, tokens, perm)          # outside 5 .. 16: never
    # auto: exactly the cells, one interval of token counts per layer; pure
    monkeypatch.setattr(bd, "_GEMM_GATHER12_MODE", "auto")
    for cells in (bd._GEMM_GATHER12_CELLS, ((65536, 4096, 1, 4 << 20, 9, 16), (65536, 4096, 1, 16 << 20, 5, 16), (65536, 0, 0, 0, 5, 12))):
        monkeypatch.setattr(bd, "_GEMM_GATHER12_CELLS", cells)
        for (k, kr), (O, I), perm in itertools.product(FORMATS, SHAPES, (False, True)):
            on = [t for t in range(0, 20) if route(12, k, kr, O, I, t, perm)]
            assert on == list(range(on[0], on[-1] + 1)) if on else True
            assert on == [t for t in range(0, 20) if route(12, k, kr, O, I, t, perm)]
            said = sorted({t for c in cells if c[:3] == (k, kr, int(perm)) and ((O + 11) // 12) * I >= c[3] for t in range(c[4], c[5] + 1)})
            assert on == said and all(len(c) == 6 and c[4] >= 5 and c[5] <= 16 for c in cells)
            assert [t for t in range(0, 20) if route(12, k, kr, O, I, t)] == sorted(
                set(on) | {t for t in range(0, 20) if route(12, k, kr, O, I, t, not perm)})   # has_perm = None: either state
    # the knob: every format from 5 to 16 tokens / none
    monkeypatch.setattr(bd, "_GEMM_GATHER12_MODE", "1")
    for (k, kr), perm in itertools.product(FORMATS, (None, False, True)):
        assert [t for t in range(0, 20) if route(12, k, kr, 516, 2048, t, perm)] == list(range(5, 17))
    monkeypatch.setattr(bd, "_GEMM_GATHER12_MODE", "0")
    assert not any(route(12, k, kr, 8184, 8192, t) for k, kr in FORMATS for t in range(0, 20))
    # the third table: one record; the first two tables and `_batched_decode_entry` answer for v = 12 what they did
    (r,) = bd.BATCHED_DECODE_V12_ROUTES
    assert (r.entry, r.min_tokens, r.max_tokens, r.perm, r.workspace, r.perm_cells, r.off_flags, r.exact_only, r.knob) == \
        ("vptq_quant_gemm_gather12", 5, 16, None, True, True, B.GEMV_FORCE_GENERIC, False, "_GEMM_GATHER12_MODE")
    assert r.route is bd.gemm_gather12_route
    assert len(bd.BATCHED_DECODE_ROUTES) == 5 and len(bd.BATCHED_DECODE_WIDE_ROUTES) == 1
    for (k, kr), perm in itertools.product(FORMATS, (False, True)):
        static = (12, k, kr, 1, False, True, perm)
        assert bd._batched_decode_entry(12, k, kr) is None
        assert bd.batched_decode_routes(*static) == () and bd.batched_decode_wide_routes(*static) == ()
        assert bd.batched_decode_v12_routes(*static) == (r,)
        assert bd.batched_decode_v12_routes(12, k, kr, 2, False, True, perm) == () and bd.batched_decode_v12_routes(12, k, kr, 1, True, True, perm) == ()
        assert bd.batched_decode_v12_routes(12, k, kr, 1, False, False, perm) == ()
    for v, k, kr in ((8, 65536, 256), (16, 65536, 1024), (8, 256, 256), (6, 65536, 4096)):
        assert bd.batched_decode_v12_routes(v, k, kr, 1, False, True, True) == ()
    monkeypatch.setattr(bd, "_GEMM_GATHER12_MODE", "1")
    assert bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 12, 0, True) and bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 5, 0, False)
    assert not bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 17, 0, True)
    assert not bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 12, B.GEMV_FORCE_GENERIC, True)
