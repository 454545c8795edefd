"""Host side of vptq_quant_gemm_gather_px (gemm_gather_px.hip; added within ABI 12), without a GPU: the four symbols, the `_supported`
truth table held cell by cell to the three sibling queries, the workspace formula, the entry's validation (every error returns
before a launch, fake pointers), the instance line - the permute launch's shape, then the inner kernel's own line for the descriptor
without its permutation -, the Python route function with its own cells and knob, the sibling route functions as they were, and the
census of the new compile unit."""
import ctypes
import itertools
import os
import re

from vptq_amd import _backend as B
from test_gemm_gatherw_cpu import desc, want_line as want_gatherw, TILE, ROWS, CUS, WG_PER_CU, X, Y, KRS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gather_px_workspace_bytes", "vptq_quant_gemm_gather_px_supported", "vptq_quant_gemm_gather_px",
           "vptq_quant_gemm_gather_px_instance")
WS = 11 << 20                     # fake, 256-byte aligned, never dereferenced
PX_THREADS, PX_TOK = 64, 4        # the permute launch: chunks of 8 columns per workgroup, tokens per thread
# (vector length, main centroids, residual centroids): gemm_gather's three, four of gemm_gatherx's, two that have no batched decode
GATHER = [(8, 65536, kr) for kr in KRS]
GATHERX = [(16, 65536, 0), (16, 65536, 1024), (8, 32768, 0), (8, 65536, 4096)]
OTHER = [(8, 256, 256), (8, 4096, 0)]
TOKENS = (-1, 0, 1, 5, 16, 17, 48, 49)


def ws_bytes(d, tokens):
    return (tokens * d.group_size * 2 + 255) // 256 * 256 if d.perm else 0


def line(d, tokens, flags=0, size=256):
    buf = ctypes.create_string_buffer(size)
    rc = B.lib().vptq_quant_gemm_gather_px_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def inner_line(d, tokens):
    """what the layer's own `_instance` prints for the descriptor WITHOUT its permutation"""
    p = desc(I=d.in_features, O=d.out_features, v=d.vector_len, k=d.num_centroids, kr=d.num_res_centroids, dtype=d.dtype, perm=False)
    lib = B.lib()
    name = "vptq_quant_gemm_gatherw" if tokens > 16 else \
        "vptq_quant_gemm_gather" if lib.vptq_quant_gemm_gather_supported(p, tokens) else "vptq_quant_gemm_gatherx"
    buf = ctypes.create_string_buffer(256)
    assert getattr(lib, name + "_instance")(p, tokens, 0, buf, len(buf)) == 0
    return buf.value.decode()


def want_line(d, tokens):
    head = "none" if not d.perm else \
        (f"permute_x_tokens g={d.group_size} tok={tokens} grid={(d.group_size // 8 + PX_THREADS - 1) // PX_THREADS}x"
         f"{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK}")
    return head + " | " + inner_line(d, tokens)


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
    vp, D = ctypes.c_void_p, ctypes.POINTER(B.LayerDesc)
    assert B.EXPORTS["vptq_quant_gemm_gather_px_workspace_bytes"] == (ctypes.c_size_t, [D, ctypes.c_int])
    assert B.EXPORTS["vptq_quant_gemm_gather_px_supported"] == (ctypes.c_int, [D, ctypes.c_int])
    assert B.EXPORTS["vptq_quant_gemm_gather_px"] == (ctypes.c_int, [D, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp])
    assert B.EXPORTS["vptq_quant_gemm_gather_px_instance"] == (ctypes.c_int, [D, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t])
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    from vptq_amd import ops
    import sys
    assert callable(ops.quant_gemm_gather_px) and "quant_gemm_gather_px" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    # the header documents the entry and its alignment rule beside the three entries it builds on
    doc = hdr[hdr.index("gemm_gather_px.hip"):hdr.index("VPTQ_API size_t vptq_quant_gemm_gather_px_workspace_bytes")]
    assert "Alignment:" in doc and "VPTQ_E_WORKSPACE" in doc and "VPTQ_E_ALIGN" in doc


def test_supported_agrees_with_the_three_sibling_queries_cell_by_cell():
    lib = B.lib()
    served = 0
    for (v, k, kr), dtype, perm, tokens in itertools.product(GATHER + GATHERX + OTHER, (0, 1), (False, True), TOKENS):
        d = desc(v=v, k=k, kr=kr, dtype=dtype, perm=perm)
        sib = lib.vptq_quant_gemm_gatherw_supported(d, tokens) if tokens > 16 else \
            (lib.vptq_quant_gemm_gather_supported(d, tokens) or lib.vptq_quant_gemm_gatherx_supported(d, tokens))
        assert lib.vptq_quant_gemm_gather_px_supported(d, tokens) == sib, (v, k, kr, dtype, perm, tokens)
        assert lib.vptq_quant_gemm_gather_px_workspace_bytes(d, tokens) == (ws_bytes(d, tokens) if sib else 0)
        served += sib
    # the table is not trivially empty: gemm_gather's formats at 1 - 48 tokens, gemm_gatherx's at 1 - 16, both with and without perm
    assert served == 2 * 2 * (len(GATHER) * 5 + len(GATHERX) * 3)
    assert lib.vptq_quant_gemm_gather_px_supported(None, 8) == 0 and lib.vptq_quant_gemm_gather_px_workspace_bytes(None, 8) == 0
    for bad in (desc(I=4100), desc(perm=True, perm_sb=False), desc(norm=False), desc(I=4100, perm=True)):
        for tokens in (5, 32):
            assert lib.vptq_quant_gemm_gather_px_supported(bad, tokens) == 0 and lib.vptq_quant_gemm_gather_px_workspace_bytes(bad, tokens) == 0


def test_workspace_bytes_formula():
    q = B.lib().vptq_quant_gemm_gather_px_workspace_bytes
    for I, tokens in itertools.product((8, 64, TILE + 8, 2 * TILE + 264, 4096, 28672), (1, 5, 16, 17, 33, 48)):
        d = desc(I=I, O=64, perm=True)
        assert q(d, tokens) == (tokens * I * 2 + 255) // 256 * 256 and q(d, tokens) % 256 == 0 and q(d, tokens) >= tokens * I * 2
        assert q(desc(I=I, O=64), tokens) == 0                       # no permutation: no workspace
    assert q(desc(I=28672, O=8192, perm=True), 48) == 2752512 > 2 << 20   # (more than the stream buffer's default size)
    assert q(desc(I=8, O=8, perm=True), 1) == 256


def test_validation_returns_before_a_launch():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error), in the sibling entries'
    order: NULL, tokens, unsupported, x alignment; then the workspace's size, then its alignment"""
    call = B.lib().vptq_quant_gemm_gather_px
    for perm in (False, True):
        d, bad = desc(perm=perm), desc(k=256, perm=perm)
        need = ws_bytes(d, 48)
        assert call(None, X, Y, 32, 0, WS, need, None) == B.E_NULL
        assert call(d, None, Y, 32, 0, WS, need, None) == B.E_NULL and call(d, X, None, 32, 0, WS, need, None) == B.E_NULL
        assert b"NULL" in B.lib().vptq_last_error()
        for tokens in (0, 49, 64, -3):
            assert call(d, X, Y, tokens, 0, WS, need, None) == B.E_TOKENS
            assert b"[1, 48]" in B.lib().vptq_last_error()
            assert call(bad, X, Y, tokens, 0, WS, need, None) == B.E_TOKENS      # tokens before unsupported
            assert call(d, X + 2, Y, tokens, 0, None, 0, None) == B.E_TOKENS      # ... before alignment and workspace
        for tokens in (1, 5, 16, 17, 48):
            assert call(bad, X, Y, tokens, 0, WS, need, None) == B.E_UNSUPPORTED and b"gemm_gather_px serves" in B.lib().vptq_last_error()
            assert call(bad, X + 2, Y, tokens, 0, None, 0, None) == B.E_UNSUPPORTED   # unsupported before alignment and workspace
            assert call(desc(I=4100, perm=perm), X, Y, tokens, 0, WS, need, None) == B.E_UNSUPPORTED
        assert call(desc(v=16, perm=perm), X, Y, 17, 0, WS, need, None) == B.E_UNSUPPORTED   # gemm_gatherx's formats stop at 16
        # x that is not 16-byte aligned: the code of the layer's own entry, before the workspace is looked at
        for off in (2, 4, 8):
            assert call(d, X + off, Y, 16, 0, None, 0, None) == B.E_UNSUPPORTED and b"16-byte" in B.lib().vptq_last_error()
            assert call(d, X + off, Y, 17, 0, None, 0, None) == B.E_TOKENS and b"16-byte" in B.lib().vptq_last_error()
            assert call(desc(v=16, perm=perm), X + off, Y, 5, 0, None, 0, None) == B.E_UNSUPPORTED
    # the workspace of a layer with a permutation: NULL, one byte short; the exact size passes this check (and meets the next)
    for d, tokens in ((desc(perm=True), 5), (desc(perm=True), 48), (desc(v=16, kr=0, perm=True), 16), (desc(I=TILE + 8, O=20, perm=True), 33)):
        need = B.lib().vptq_quant_gemm_gather_px_workspace_bytes(d, tokens)
        assert need == ws_bytes(d, tokens) > 0
        assert call(d, X, Y, tokens, 0, None, need, None) == B.E_WORKSPACE and call(d, X, Y, tokens, 0, None, 0, None) == B.E_WORKSPACE
        assert call(d, X, Y, tokens, 0, WS, need - 1, None) == B.E_WORKSPACE and b"workspace" in B.lib().vptq_last_error()
        assert call(d, X, Y, tokens, 0, WS, 0, None) == B.E_WORKSPACE
        assert call(d, X, Y, tokens, 0, WS + 8, need - 1, None) == B.E_WORKSPACE       # size before alignment
        for off in (1, 2, 4, 8):   # the exact size is accepted: the NEXT check answers
            assert call(d, X, Y, tokens, 0, WS + off, need, None) == B.E_ALIGN and b"16-byte" in B.lib().vptq_last_error()
            assert call(d, X, Y, tokens, 0, WS + off, need + 4096, None) == B.E_ALIGN
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        d = desc(perm=True)
        assert call(d, X + 8, Y, 32, flags, WS, 1 << 20, None) == B.E_TOKENS and call(d, X, Y, 49, flags, WS, 1 << 20, None) == B.E_TOKENS
        assert call(d, X, Y, 32, flags, WS, 8, None) == B.E_WORKSPACE and call(d, X, Y, 32, flags, WS + 4, 1 << 20, None) == B.E_ALIGN


def test_instance_line_is_the_permute_shape_and_the_inner_kernels_own_line():
    per_wave = 8 * ROWS * CUS * WG_PER_CU   # outputs of one full grid of row groups (test_gemm_gatherw_cpu's shapes)
    shapes = [(4096, per_wave * h) for h in (1, 2, 3)] + [(8, 5), (TILE + 8, 20), (64, per_wave + 4), (2 * TILE + 264, 36)]
    seen = set()
    for (I, O), (v, k, kr), tokens, dtype, perm in itertools.product(shapes, GATHER + GATHERX, (1, 5, 16, 17, 32, 33, 48), (0, 1), (False, True)):
        d = desc(I=I, O=O, v=v, k=k, kr=kr, dtype=dtype, perm=perm)
        rc, text = line(d, tokens)
        if tokens > 16 and (v, k, kr) in GATHERX:
            assert rc == B.E_UNSUPPORTED and text == ""
            continue
        assert rc == 0 and text == want_line(d, tokens), (text, want_line(d, tokens))
        head, inner = text.split(" | ")
        assert (head == "none") == (not perm) and " perm=0 " in inner     # the inner kernel never has the permutation
        seen.add((inner.split()[0], perm))
        if tokens > 16:   # the inner part is gemm_gatherw's line for perm = 0, as that file's own test writes it
            assert inner == want_gatherw(desc(I=I, O=O, kr=kr, dtype=dtype), tokens)
    assert seen == set(itertools.product(("gemm_gather", "gemm_gatherx", "gemm_gatherw"), (False, True)))
    assert line(desc(I=8, O=5, perm=True), 48)[1] == "permute_x_tokens g=8 tok=48 grid=1x12 tpt=4 | gemm_gatherw dt=f16 t=24 perm=0 tok=48 tb=3 tiles=1 rgs=1"
    assert line(desc(I=TILE + 8, O=20, kr=0, dtype=1, perm=True), 5)[1] == \
        "permute_x_tokens g=1032 tok=5 grid=3x2 tpt=4 | gemm_gather dt=bf16 t=16 perm=0 tok=5 tiles=2 rgs=1"
    assert line(desc(I=2 * TILE + 264, O=36, kr=65536, perm=True), 17)[1] == \
        "permute_x_tokens g=2312 tok=17 grid=5x5 tpt=4 | gemm_gatherw dt=f16 t=32 perm=0 tok=17 tb=2 tiles=3 rgs=1"
    assert line(desc(I=4096, O=4096, perm=True), 17)[1].startswith("permute_x_tokens g=4096 tok=17 grid=8x5 tpt=4 | ")
    assert line(desc(I=8192, O=8192), 40)[1] == "none | gemm_gatherw dt=f16 t=24 perm=0 tok=40 tb=3 tiles=8 rgs=1"
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert line(desc(perm=True), 40, flags) == line(desc(perm=True), 40)
    # the call's own errors, and a buffer that is too small
    assert line(desc(), 0)[0] == B.E_TOKENS and line(desc(perm=True), 49)[0] == B.E_TOKENS and line(desc(k=256), 32)[0] == B.E_UNSUPPORTED
    assert line(desc(k=256), 49)[0] == B.E_TOKENS
    for size in (4, 16, 60):   # (shorter than "none | ", than the permute part, than the whole line)
        small = ctypes.create_string_buffer(size)
        assert B.lib().vptq_quant_gemm_gather_px_instance(desc(perm=True), 32, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gather_px_instance(desc(), 32, 0, None, 0) == B.E_NULL
    assert B.lib().vptq_quant_gemm_gather_px_instance(None, 32, 0, small, len(small)) == B.E_NULL


def test_route_function_is_pure_follows_its_own_cells_and_obeys_its_knob(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gather_px_route
    assert (vq.GEMM_GATHER_PX_MIN_TOKENS, vq.GEMM_GATHER_PX_MAX_TOKENS) == (5, 48)
    assert bd._GEMM_GATHER_PX_MODE == "auto"
    shapes = ((8192, 8192), (4096, 4096), (14336, 4096), (4096, 14336), (28672, 8192), (512, 2048), (36, 1032))

    def by_the_cells(cells, v, k, kr, O, I, t):
        n_el = ((O + v - 1) // v) * I
        return any((cv, ck, ckr) == (v, k, kr) and n_el >= max(e, 4 << 20) and lo <= t <= hi for cv, ck, ckr, e, lo, hi in cells)

    def check(cells):
        for (O, I), (v, k, kr) in itertools.product(shapes, GATHER + GATHERX + OTHER):
            for t in (-1, 0, 1, 4, 49, 64, 128):
                assert not route(v, k, kr, O, I, t)                         # outside 5 .. 48: never
            for t in range(5, 49):
                want = by_the_cells(cells, v, k, kr, O, I, t) and (v, k, kr) not in OTHER and (t <= 16 or (v, k, kr) in GATHER)
                assert route(v, k, kr, O, I, t) == want, (v, k, kr, O, I, t)
            on = [t for t in range(5, 49) if route(v, k, kr, O, I, t)]
            assert on == list(range(on[0], on[-1] + 1)) if on else True     # the routed token counts of a layer are one interval
            if ((O + v - 1) // v) * I < 4 << 20:
                assert not on, (O, I, v, k, kr)                             # no cell under 4 M index elements

    # the committed table: well-formed, nothing under the floor `GEMM_GATHERW_MIN_ELEMENTS` states, and followed exactly
    assert bd.GEMM_GATHERW_MIN_ELEMENTS == 4 << 20
    assert all(len(c) == 6 and c[3] >= 4 << 20 and 5 <= c[4] <= c[5] <= 48 for c in bd._GEMM_GATHER_PX_CELLS)
    check(bd._GEMM_GATHER_PX_CELLS)
    # a monkeypatched table is followed exactly - cells of other formats, sizes under the floor and inner kernels that end at 16 included
    cells = ((8, 65536, 256, 7 << 20, 9, 40), (8, 65536, 0, 1 << 20, 17, 48), (16, 65536, 0, 4 << 20, 5, 48), (8, 32768, 0, 28 << 20, 12, 16),
             (8, 256, 256, 4 << 20, 5, 48))
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_CELLS", cells)
    check(cells)
    assert route(8, 65536, 256, 8192, 8192, 9) and route(8, 65536, 256, 8192, 8192, 40) and not route(8, 65536, 256, 8192, 8192, 41)
    assert not route(8, 65536, 256, 4096, 4096, 20) and not route(8, 65536, 0, 4096, 4096, 20)      # 2 M elements: under the floor
    assert route(16, 65536, 0, 8192, 8192, 16) and not route(16, 65536, 0, 8192, 8192, 17)          # gemm_gatherx ends at 16 tokens
    assert not route(8, 65536, 256, 8192, 8196, 20)                                                   # in_features % 8
    # the knob: 1 - every layer of the three kernels from 5 tokens; 0 - none
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", "1")
    assert all(route(8, 65536, kr, 36, 1032, t) for kr in KRS for t in range(5, 49))
    assert all(route(v, k, kr, 36, 1032, t) for v, k, kr in GATHERX for t in range(5, 17))
    assert not any(route(v, k, kr, 8192, 8192, t) for v, k, kr in GATHERX for t in range(17, 49))
    assert not any(route(v, k, kr, 8192, 8192, t) for v, k, kr in OTHER for t in range(0, 70))
    assert not route(8, 65536, 256, 8192, 8192, 4) and not route(8, 65536, 256, 8192, 8192, 49)
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", "0")
    assert not any(route(v, k, kr, O, I, t) for O, I in shapes for v, k, kr in GATHER + GATHERX for t in range(0, 70))


def test_the_knob_is_read_through_tune_env_only():
    src = open(os.path.join(ROOT, "vptq_amd", "batched_decode.py")).read()
    assert src.count("VPTQ_GEMM_GATHER_PX\"") == 1
    assert '_GEMM_GATHER_PX_MODE = (B.tune_env("VPTQ_GEMM_GATHER_PX", "auto") or "auto").strip().lower()' in src
    for f in ("vptq_amd/layers/vqlinear.py", "vptq_amd/ops/quant_gemm.py", "vptq_amd/_backend.py", "vptq_amd/csrc/gemm_gather_px.hip", "vptq_amd/csrc/abi.hip"):
        assert "VPTQ_GEMM_GATHER_PX" not in open(os.path.join(ROOT, f)).read(), f


def test_the_sibling_route_functions_answer_as_before():
    """gemm_gather_route, gemm_gatherx_route and gemm_gatherw_route do not know the new table: their answers are their own cells'"""
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    assert bd._GEMM_GATHER_CELLS == ((8, 65536, 0, 2 << 20, 9), (8, 65536, 256, 2 << 20, 9), (8, 65536, 65536, 2 << 20, 9))
    assert bd._GEMM_GATHERX_CELLS == ((16, 65536, 0, 1 << 20, 5), (16, 65536, 1024, 1 << 20, 5), (8, 32768, 0, 2 << 20, 9), (8, 32768, 0, 8 << 20, 5),
                                      (8, 65536, 4096, 2 << 20, 9), (8, 65536, 4096, 8 << 20, 5))
    assert bd._GEMM_GATHERW_CELLS == tuple((kr, el, lo, hi) for kr in KRS for el, lo, hi in ((7 << 20, 17, 24), (28 << 20, 17, 48)))
    shapes = ((8192, 8192), (4096, 4096), (14336, 4096), (28672, 8192), (512, 2048))
    for (O, I), (v, k, kr), t in itertools.product(shapes, GATHER + GATHERX + OTHER, range(0, 66)):
        n_el = ((O + v - 1) // v) * I
        g = (v, k, kr) in GATHER and 5 <= t <= 16 and any(c[:3] == (v, k, kr) and n_el >= c[3] and t >= c[4] for c in bd._GEMM_GATHER_CELLS)
        gx = (v, k, kr) in GATHERX and 5 <= t <= 16 and any(c[:3] == (v, k, kr) and n_el >= c[3] and t >= c[4] for c in bd._GEMM_GATHERX_CELLS)
        gw = (v, k, kr) in GATHER and any(c[0] == kr and n_el >= max(c[1], 4 << 20) and c[2] <= t <= c[3] for c in bd._GEMM_GATHERW_CELLS)
        assert vq.gemm_gather_route(v, k, kr, O, I, t) == g and vq.gemm_gatherx_route(v, k, kr, O, I, t) == gx, (v, k, kr, O, I, t)
        assert vq.gemm_gatherw_route(v, k, kr, O, I, t) == gw, (v, k, kr, O, I, t)


def test_census_of_the_compile_unit_and_the_makefile_entry():
    """gemm_gather_px.hip: one permute kernel, plain vector stores, no kernel of the tile pipeline instantiated (the PERM = false
    forms it launches are the three units' own, reached through their launchers over a descriptor without the permutation)"""
    csrc = os.path.join(ROOT, "vptq_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_gather_px.hip")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert srcs.count("gemm_gather_px.hip") == 1
    assert "atomic" not in src and "__shared__" not in src and "asm" not in src
    assert len(re.findall(r"__global__", src)) == 1 and "permute_x_tokens_kernel" in src
    assert not re.search(r"gemm_gather\w*_kernel\s*<", src) and '#include "gemm_gather_tile.h"' not in src     # no kernel of the pipeline, PERM or not
    assert not re.search(r"<[^<>;]*\btrue\b[^<>;]*>", src)
    assert not re.search(r"^\s*#\s*if", src, re.M) and "getenv" not in src and "hipFuncSetAttribute" not in src
    assert f"kPxThreads = {PX_THREADS}" in src and f"kPxTok = {PX_TOK}" in src
    # the entry strips the permutation before the inner launch and its line: scale / bias in column order, perm NULL
    assert re.search(r"p\.weight_scale = d\.scale_permuted;\s*p\.weight_bias = d\.bias_permuted;\s*p\.perm = nullptr;", src)
    abi = open(os.path.join(csrc, "abi.hip")).read()
    body = abi[abi.index("int vptq_quant_gemm_gather_px("):abi.index("int vptq_quant_gemm_gather_px_instance(")]
    assert body.index("launch_permute_x_tokens") < body.index("gemm_gather_px_plain") < body.rindex("k->launch(")
    assert body.index("VPTQ_E_WORKSPACE") < body.index("VPTQ_E_ALIGN") < body.index("launch_permute_x_tokens")   # validation before any launch
    # the three kernel units do not know the new one
    for f in ("gemm_gather.hip", "gemm_gatherw.hip", "gemm_gatherx.hip", "gemm_gather_tile.h", "gemm_gather_host.h"):
        assert "_px" not in open(os.path.join(csrc, f)).read(), f
