"""Host side of vptq_quant_gemm_gatherxw (gemm_gatherxw_kernel in gemm_gatherxw.hip; added within ABI 12), without a GPU: the symbols,
the `_supported` truth table, the workspace query, the entry's validation (every error returns before a launch), two hand-computed
instance lines, and the Python route with its record in the second route table."""
import ctypes
import itertools
import os
import re

import pytest

from test_gemm_gather_cpu import X, Y, CUS
from test_gemm_gatherx_cpu import fdesc, want as want16, FORMATS, GATHER_OWNED
from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gatherxw_supported", "vptq_quant_gemm_gatherxw_workspace_bytes", "vptq_quant_gemm_gatherxw",
           "vptq_quant_gemm_gatherxw_instance")
WS = 11 << 20   # fake, aligned, never dereferenced
ENTRY = "vptq_quant_gemm_gatherxw"


def line(d, tokens, flags=0):
    buf = ctypes.create_string_buffer(256)
    rc = B.lib().vptq_quant_gemm_gatherxw_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def ws_bytes(d, tokens):
    return (tokens * d.group_size * 2 + 255) // 256 * 256 if d.perm else 0


def want(d, tokens, cus=CUS):
    """the launches (gemm_gather_px_decide, gemm_gatherxw_decide), restated from the 16-token line of the same layer"""
    f = dict(p.split("=") for p in want16(d, 16, cus).split()[1:])
    px = f"permute_x_tokens g={d.group_size} tok={tokens} grid={(d.group_size // 8 + 63) // 64}x{(tokens + 3) // 4} tpt=4 | " if d.perm else ""
    return px + (f"gemm_gatherxw dt={f['dt']} v={f['v']} ib={f['ib']} rb={f['rb']} res={f['res']} tok={tokens} tb={(tokens + 15) // 16} "
                 f"tiles={f['tiles']} wgcu={f['wgcu']} rgs={f['rgs']}")


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and hasattr(raw, s), f"{s} not declared / exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12 and re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    from vptq_amd import ops
    assert callable(ops.quant_gemm_gatherxw)
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(ROOT, "vptq_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert srcs.count("gemm_gatherxw.hip") == 1


def test_supported_and_workspace_bytes():
    sup, ws = B.lib().vptq_quant_gemm_gatherxw_supported, B.lib().vptq_quant_gemm_gatherxw_workspace_bytes
    for (v, k, kr), perm, dtype in itertools.product(FORMATS, (False, True), (0, 1)):
        d = fdesc(v, k, kr, perm=perm, dtype=dtype, I=4104)
        assert [t for t in range(-1, 70) if sup(d, t)] == list(range(17, 49)), (v, k, kr)   # exactly 17 .. 48
        assert [ws(d, t) for t in (16, 17, 33, 48, 49)] == [0, ws_bytes(d, 17), ws_bytes(d, 33), ws_bytes(d, 48), 0]
    assert ws(fdesc(16, 65536, 1024, perm=True, I=4104), 17) == 139776 and ws(fdesc(8, 32768, 0, perm=True, I=8), 48) == 768
    for v, k, kr in GATHER_OWNED + [(8, 256, 256), (16, 8192, 0), (12, 65536, 4096)]:   # gemm_gather's, the canonical, other formats
        assert not any(sup(fdesc(v, k, kr, perm=p), t) or ws(fdesc(v, k, kr, perm=p), t) for t in range(0, 70) for p in (False, True))
    assert sup(None, 32) == 0 and ws(None, 32) == 0
    assert sup(fdesc(16, 65536, 1024, C=2), 32) == 0 and sup(fdesc(16, 65536, 0, I=4100), 32) == 0 and sup(fdesc(16, 65536, 0, norm=False), 32) == 0
    d = fdesc(16, 65536, 1024, perm=True)
    d.scale_permuted = None
    assert sup(d, 32) == 0 and ws(d, 32) == 0
    # the entries beside it are what they were: the 16-token window, px's refusal of these formats from 17 tokens
    assert B.lib().vptq_quant_gemm_gatherx_supported(fdesc(16, 65536, 0), 17) == 0
    assert B.lib().vptq_quant_gemm_gather_px_supported(fdesc(16, 65536, 0, perm=True), 17) == 0


def test_validation_returns_before_a_launch():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error)"""
    call, err = B.lib().vptq_quant_gemm_gatherxw, B.lib().vptq_last_error
    d, p, bad, owned = fdesc(16, 65536, 1024), fdesc(8, 65536, 4096, perm=True), fdesc(8, 256, 256), fdesc(8, 65536, 256)
    assert call(None, X, Y, 32, 0, WS, 1 << 20, None) == B.E_NULL
    assert call(d, None, Y, 32, 0, None, 0, None) == B.E_NULL and call(d, X, None, 32, 0, None, 0, None) == B.E_NULL and b"NULL" in err()
    for tokens in (0, 1, 16, 49, 64, -3):
        assert call(d, X, Y, tokens, 0, None, 0, None) == B.E_TOKENS and b"[17, 48]" in err()
        assert call(bad, X, Y, tokens, 0, None, 0, None) == B.E_TOKENS   # tokens before unsupported
    for layer in (bad, owned, fdesc(16, 65536, 1024, C=2)):
        assert call(layer, X, Y, 32, 0, WS, 1 << 20, None) == B.E_UNSUPPORTED and b"gemm_gatherxw serves" in err()
    for off in (2, 4, 8):
        assert call(d, X + off, Y, 32, 0, None, 0, None) == B.E_UNSUPPORTED and b"x must be 16-byte aligned" in err()
    need = ws_bytes(p, 32)
    assert call(p, X, Y, 32, 0, None, need, None) == B.E_UNSUPPORTED and f"workspace of {need} bytes needed".encode() in err()
    assert call(p, X, Y, 32, 0, WS, need - 1, None) == B.E_UNSUPPORTED and b"bytes needed" in err()
    assert call(p, X, Y, 32, 0, WS + 8, need, None) == B.E_UNSUPPORTED and b"workspace must be 16-byte aligned" in err()
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(d, X + 8, Y, 32, flags, None, 0, None) == B.E_UNSUPPORTED and call(d, X, Y, 49, flags, None, 0, None) == B.E_TOKENS


def test_instance_lines():
    # 8192 x 8192 v16-k65536-1024 bf16: 512 row groups of one vector-row, 32 + 32 KiB of LDS -> 2 workgroups per CU
    a = fdesc(16, 65536, 1024, I=8192, O=8192, dtype=1)
    assert line(a, 40) == (0, "gemm_gatherxw dt=bf16 v=16 ib=16 rb=10 res=lds tok=40 tb=3 tiles=8 wgcu=2 rgs=1")
    # a permuted v8-k65536-4096 layer of 64 columns with 2 x 4 x 256 + 3 row groups: 8 chunks in one workgroup x 5 token slices
    b = fdesc(8, 65536, 4096, I=64, O=8 * (2 * 4 * CUS + 3) - 4, perm=True)
    assert line(b, 17) == (0, "permute_x_tokens g=64 tok=17 grid=1x5 tpt=4 | gemm_gatherxw dt=f16 v=8 ib=16 rb=12 res=l2 tok=17 tb=2 tiles=1 wgcu=4 rgs=2")
    seen = set()
    for (v, k, kr), dtype, perm, tokens in itertools.product(FORMATS, (0, 1), (False, True), (17, 32, 33, 48)):
        d = fdesc(v, k, kr, dtype=dtype, perm=perm, I=2 * 1024 + 264, O=3 * v - 4)
        assert line(d, tokens) == (0, want(d, tokens))
        f = dict(q.split("=") for q in line(d, tokens)[1].split(" | ")[-1].split()[1:])
        seen.add((f["dt"], f["v"], f["res"], f["tb"]))
    assert len(seen) == 24   # every instantiation of gemm_gatherxw_kernel<DT, V, RES, TB> is named by a line
    assert line(a, 16)[0] == B.E_TOKENS and line(a, 49)[0] == B.E_TOKENS and line(fdesc(8, 65536, 256), 32)[0] == B.E_UNSUPPORTED
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gatherxw_instance(a, 32, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""
    assert B.lib().vptq_quant_gemm_gatherxw_instance(a, 32, 0, None, 0) == B.E_NULL


SHAPES = ((8192, 8192), (4096, 4096), (14336, 4096), (4096, 14336), (28672, 8192), (8192, 28672), (512, 2048), (28, 1032))


@pytest.mark.parametrize("cells", [None, ((16, 65536, 1024, 0, 0, 17, 24), (16, 65536, 1024, 0, 16 << 20, 17, 48), (8, 32768, 0, 1, 7 << 20, 20, 40))])
def test_route_function_is_pure_and_follows_the_cells(cells, monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gatherxw_route
    assert (vq.GEMM_GATHERXW_MIN_TOKENS, vq.GEMM_GATHERXW_MAX_TOKENS) == (17, 48) and bd._GEMM_GATHERXW_MODE == "auto"
    assert '_GEMM_GATHERXW_MODE = (B.tune_env("VPTQ_GEMM_GATHERXW", "auto") or "auto").strip().lower()' in open(bd.__file__).read()
    if cells is not None:
        monkeypatch.setattr(bd, "_GEMM_GATHERXW_CELLS", cells)
    cells = bd._GEMM_GATHERXW_CELLS
    assert all(len(c) == 7 and bd._batched_decode_entry(*c[:3]) == "vptq_quant_gemm_gatherx" and 17 <= c[5] <= c[6] <= 48 for c in cells)
    for (v, k, kr), (O, I), perm in itertools.product(FORMATS, SHAPES, (False, True)):
        n_el = ((O + v - 1) // v) * I
        on = [t for t in range(-1, 70) if route(v, k, kr, O, I, t, perm)]
        assert on == (list(range(on[0], on[-1] + 1)) if on else []) and (not on or (on[0] >= 17 and on[-1] <= 48))   # one interval in 17 .. 48
        assert not on or n_el >= 4 << 20                                                                           # the floor
        assert on == [t for t in range(17, 49) if any((v, k, kr, perm) == (c[0], c[1], c[2], bool(c[3])) and n_el >= max(c[4], 4 << 20) and
                                                      c[5] <= t <= c[6] for c in cells)]
        assert all(route(v, k, kr, O, I, t) == (route(v, k, kr, O, I, t, False) or route(v, k, kr, O, I, t, True)) for t in (17, 24, 48))
    for mode, perm in itertools.product(("auto", "1", "0"), (False, True)):
        monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", mode)
        for v, k, kr in FORMATS:
            assert [t for t in range(0, 70) if route(v, k, kr, 28, 1032, t, perm)] == (list(range(17, 49)) if mode == "1" else [])
            assert not route(v, k, kr, 8192, 8196, 32, perm)                                        # columns % 8
        for v, k, kr in GATHER_OWNED + [(8, 256, 256), (12, 65536, 4096), (16, 65536, 1000)]:       # never a format of another kernel
            assert not any(route(v, k, kr, 8192, 8192, t, perm) for t in range(0, 70))


def test_committed_cells_keep_the_floor():
    from vptq_amd import batched_decode as bd
    assert all(c[4] >= bd.GEMM_GATHERW_MIN_ELEMENTS == 4 << 20 for c in bd._GEMM_GATHERXW_CELLS)


def test_the_record_sits_in_the_second_table_and_the_first_is_what_it_was(monkeypatch):
    from vptq_amd import batched_decode as bd
    assert [r.entry for r in bd.BATCHED_DECODE_ROUTES] == ["vptq_quant_gemm_gather_px", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx",
                                                           "vptq_quant_gemm_k256w", "vptq_quant_gemm_gatherw"]
    (r,) = bd.BATCHED_DECODE_WIDE_ROUTES
    assert (r.entry, r.min_tokens, r.max_tokens, r.knob, r.perm, r.off_flags, r.exact_only, r.workspace) == \
        (ENTRY, 17, 48, "_GEMM_GATHERXW_MODE", None, B.GEMV_FORCE_GENERIC, False, True) and r.route is bd.gemm_gatherxw_route
    for (v, k, kr), perm in itertools.product(FORMATS + GATHER_OWNED + [(8, 256, 256)], (False, True)):
        first = [x.entry for x in bd.batched_decode_routes(v, k, kr, 1, False, True, perm)]
        entry = bd._batched_decode_entry(v, k, kr)
        own = {"vptq_quant_gemm_gather": ["vptq_quant_gemm_gather", "vptq_quant_gemm_gatherw"], "vptq_quant_gemm_gatherx": ["vptq_quant_gemm_gatherx"],
               None: ["vptq_quant_gemm_k256w"]}[entry]
        assert first == (["vptq_quant_gemm_gather_px"] if perm and entry else []) + own and ENTRY not in first
        wide = bd.batched_decode_wide_routes(v, k, kr, 1, False, True, perm)
        assert wide == ((r,) if entry == "vptq_quant_gemm_gatherx" else ())
        assert bd.batched_decode_wide_routes(v, k, kr, 2, False, True, perm) == bd.batched_decode_wide_routes(v, k, kr, 1, True, True, perm) == \
            bd.batched_decode_wide_routes(v, k, kr, 1, False, False, perm) == ()
    # the per-call decision: the window, the off-flag, the knob; a permuted layer and a plain one alike
    for mode, perm in itertools.product(("auto", "1", "0"), (False, True)):
        monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", mode)
        takes = [t for t in range(0, 70) if bd.batched_decode_takes(r, 16, 65536, 1024, 512, 2048, t, 0, perm)]
        assert takes == (list(range(17, 49)) if mode == "1" else [])
        assert not bd.batched_decode_takes(r, 16, 65536, 1024, 512, 2048, 24, B.GEMV_FORCE_GENERIC, perm)
    monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", "auto")
    monkeypatch.setattr(bd, "_GEMM_GATHERXW_CELLS", ((16, 65536, 1024, 1, 4 << 20, 17, 32),))   # a cell of permuted layers only
    assert bd.batched_decode_takes(r, 16, 65536, 1024, 8192, 8192, 24, 0, True) and not bd.batched_decode_takes(r, 16, 65536, 1024, 8192, 8192, 24, 0, False)
