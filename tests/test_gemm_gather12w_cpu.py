"""Host side of vptq_quant_gemm_gather12w (gemm_gather12w.hip; added within ABI 12), without a GPU: the partition arithmetic behind
`_supported`, the workspace query and the instance line, validation before any launch, the route function and the fifth table."""
import ctypes
import itertools

import pytest

from test_gemm_gather_cpu import X, Y, CUS   # fake aligned pointers; nothing is dereferenced by host logic
from test_gemm_gather12_cpu import fdesc, want as want12, FORMATS, SHAPES, WS
from vptq_amd import _backend as B

ENTRY, TILE, MAX_PARTS = "vptq_quant_gemm_gather12w", 512, 16


def line(d, tokens, parts, flags=0):
    buf = ctypes.create_string_buffer(320)
    rc = B.lib().vptq_quant_gemm_gather12w_instance(d, tokens, flags, parts, buf, len(buf))
    return rc, buf.value.decode()


def RULE(groups, tiles, slots):
    """parts == 0 (g12w_rule_parts), restated"""
    if 4 * groups > 5 * slots:
        return 1
    for even in (True, False):
        for tpp in range(1, tiles + 1):
            S = -(-tiles // tpp)
            if S <= MAX_PARTS and not (even and tiles % tpp) and 2 * groups * S <= 5 * slots:
                return S
    return 1


def split(d, tokens, parts, cus=CUS):
    """(S, tiles per part, wgcu, row groups, token blocks) of gemm_gather12w_decide, restated"""
    tiles, groups, tb = (d.group_size + TILE - 1) // TILE, (d.num_indices + 3) // 4, (tokens + 15) // 16
    by_lds = int(want12(d, 1, cus).split("wgcu=")[1].split()[0])
    wgcu = 1 if tb == 3 and d.num_res_centroids else by_lds   # (g12w_min_wg)
    ask = parts if parts else RULE(groups, tiles, cus * by_lds)   # (the rule counts the LDS bound's slots for every instantiation)
    tpp = -(-tiles // max(1, min(ask, tiles, MAX_PARTS)))
    return -(-tiles // tpp), tpp, wgcu, groups, tb


def want(d, tokens, parts, cus=CUS):
    """the launches (gemm_gather_px_decide, gemm_gather12w_decide), restated"""
    S, tpp, wgcu, groups, tb = split(d, tokens, parts, cus)
    grid = min(groups * S, cus * wgcu)
    head, tail = want12(d, tokens, cus).replace("gemm_gather12 ", "gemm_gather12w ").split(" tiles=")
    dt = "f16" if d.dtype == 0 else "bf16"
    text = f"{head} tb={tb} tiles={tail.split()[0]} parts={S} tpp={tpp} wgcu={wgcu} rgs={(groups * S + grid - 1) // grid}"
    return text + (f" | gemm_gather12w_sum dt={dt} parts={S} grid={(d.out_features + 255) // 256}x{tokens}" if S >= 2 else "")


def test_symbols_partition_arithmetic_supported_and_workspace():
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in (ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY, ENTRY + "_instance"):
        assert hasattr(raw, s) and s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], s
    from vptq_amd import ops
    assert callable(ops.quant_gemm_gather12w) and B.lib().vptq_abi_version() == 12
    sup, ws = B.lib().vptq_quant_gemm_gather12w_supported, B.lib().vptq_quant_gemm_gather12w_workspace_bytes
    for I, parts, S, tpp in ((4096, 1, 1, 8), (4096, 2, 2, 4), (4096, 3, 3, 3), (4096, 5, 4, 2), (4096, 99, 8, 1),      # 8 tiles
                             (2312, 2, 2, 3), (2312, 3, 3, 2), (2312, 5, 5, 1), (14336, 16, 14, 2), (520, 2, 2, 1), (504, 2, 1, 1)):
        d = fdesc(65536, 4096, I=I, O=56, perm=True)
        for tokens in (17, 32, 33, 48):
            assert split(d, tokens, parts)[:2] == (S, tpp) and sup(d, tokens, parts) == 1, (I, parts)
            assert line(d, tokens, parts) == (0, want(d, tokens, parts)), (line(d, tokens, parts), want(d, tokens, parts))
            xp = ((tokens * I * 2 + 255) // 256) * 256
            part_bytes = S * tokens * 2 * 48 * 4 if S >= 2 else 0            # 56 outputs: 5 vector-rows, two row groups
            assert ws(d, tokens, parts) == xp + part_bytes
            d.perm = None
            assert ws(d, tokens, parts) == part_bytes                        # one part, no permutation: no workspace at all
            d = fdesc(65536, 4096, I=I, O=56, perm=True)
    for (k, kr), dtype in itertools.product(FORMATS, (0, 1)):
        assert sup(fdesc(k, kr, dtype=dtype), 24, -1) == 0 and ws(fdesc(k, kr), 24, -1) == 0
        for tokens in range(14, 52):
            assert sup(fdesc(k, kr, perm=True, dtype=dtype), tokens, 0) == int(17 <= tokens <= 48)
    assert sup(None, 24, 2) == 0 and sup(fdesc(65536, 4096, v=8, O=4096), 24, 2) == 0 and sup(fdesc(65536, 0, I=4100), 24, 2) == 0


def test_the_rule_and_instance_lines():
    cases = [(fdesc(65536, 0), 17), (fdesc(65536, 256, I=4096, O=1024, dtype=1), 32), (fdesc(65536, 4096, I=14336, O=4096, perm=True), 48),
             (fdesc(65536, 4096, I=8192, O=8184, dtype=1, perm=True), 24), (fdesc(65536, 4096, I=8192, O=8184), 40),
             (fdesc(65536, 0, I=8192, O=48 * 650 - 4), 48), (fdesc(32768, 1024, I=520, O=48 * (CUS + 2) - 8), 33)]
    for d, tokens in cases:
        assert line(d, tokens, 0) == (0, want(d, tokens, 0)), (line(d, tokens, 0), want(d, tokens, 0))
    assert split(cases[5][0], 48, 0)[0] == 1 and " | gemm_gather12w_sum" not in line(cases[5][0], 48, 0)[1]   # 650 row groups > 1.25 x 512 slots: one part
    assert split(cases[0][0], 17, 0)[0] >= 2                                       # 4096 x 4092: 86 row groups are split
    d = cases[6][0]   # a residual table in LDS: 2 workgroups per CU at two token blocks, 1 at three
    assert line(d, 32, 2)[1] == ("gemm_gather12w dt=f16 ib=15 rb=10 res=lds tok=32 tb=2 tiles=2 parts=2 tpp=1 wgcu=2 rgs=2 | "
                                 f"gemm_gather12w_sum dt=f16 parts=2 grid={(48 * (CUS + 2) - 8 + 255) // 256}x32")
    assert " tb=3 tiles=2 parts=2 tpp=1 wgcu=1 rgs=3 | " in line(d, 33, 2)[1]
    assert line(cases[2][0], 48, 4)[1].startswith("permute_x_tokens g=14336 tok=48 grid=28x12 tpt=4 | gemm_gather12w dt=f16 ib=16 rb=12 res=l2 "
                                                  "tok=48 tb=3 tiles=28 parts=4 tpp=7 wgcu=1 rgs=2 | gemm_gather12w_sum dt=f16 parts=4 grid=16x48")


def test_validation_order_before_any_launch():
    call = B.lib().vptq_quant_gemm_gather12w
    d, p, bad = fdesc(65536, 4096), fdesc(65536, 4096, perm=True), fdesc(65536, 4096, v=8, O=4096)
    need_d, need_p = (B.lib().vptq_quant_gemm_gather12w_workspace_bytes(q, 24, 4) for q in (d, p))
    assert call(None, X, Y, 24, 0, 4, WS, need_d, None) == B.E_NULL and call(d, None, Y, 24, 0, 4, WS, need_d, None) == B.E_NULL
    assert call(bad, None, Y, 16, 0, 4, None, 0, None) == B.E_NULL             # NULL before tokens before unsupported
    for tokens in (0, 16, 49, -3):
        assert call(d, X, Y, tokens, 0, 4, WS, need_d, None) == B.E_TOKENS and call(bad, X, Y, tokens, 0, 4, None, 0, None) == B.E_TOKENS
    assert call(bad, X + 8, Y, 24, 0, 4, None, 0, None) == B.E_UNSUPPORTED     # unsupported before x alignment
    assert call(d, X + 8, Y, 24, 0, -1, None, 0, None) == B.E_UNSUPPORTED
    for flags in (0, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert call(d, X + 8, Y, 24, flags, 4, WS, need_d, None) == B.E_ALIGN
        for q, need in ((d, need_d), (p, need_p)):
            assert call(q, X, Y, 24, flags, 4, None, 0, None) == B.E_WORKSPACE and call(q, X, Y, 24, flags, 4, WS, need - 1, None) == B.E_WORKSPACE
            assert call(q, X, Y, 24, flags, 4, WS + 8, need, None) == B.E_ALIGN
        assert call(p, X, Y, 24, flags, 1, None, 0, None) == B.E_WORKSPACE     # one part: a permuted layer still needs x[perm]
    assert line(d, 16, 4)[0] == B.E_TOKENS and line(bad, 24, 4)[0] == B.E_UNSUPPORTED and line(d, 24, -1)[0] == B.E_UNSUPPORTED


@pytest.mark.parametrize("cells", [None, ((65536, 4096, 1, 1 << 20, 5 << 20, 17, 48), (65536, 0, 0, 0, 2 << 20, 24, 33))])
def test_route_function_and_the_fifth_table(cells, monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gather12w_route
    assert bd._GEMM_GATHER12W_MODE == "auto" and '_GEMM_GATHER12W_MODE = (B.tune_env("VPTQ_GEMM_GATHER12W", "auto") or "auto").strip().lower()' in open(bd.__file__).read()
    # every shipped cell: seven fields, a most bound, nothing under 1 M index elements, inside 17 .. 48 tokens
    assert all(len(c) == 7 and (1 << 20) <= c[3] <= c[4] and 17 <= c[5] <= c[6] <= 48 for c in bd._GEMM_GATHER12W_CELLS)
    cells = bd._GEMM_GATHER12W_CELLS if cells is None else cells
    monkeypatch.setattr(bd, "_GEMM_GATHER12W_CELLS", cells)
    for (k, kr), (O, I), perm in itertools.product(FORMATS, SHAPES + ((1020, 4096),), (False, True)):
        n_el = ((O + 11) // 12) * I
        said = sorted({t for c in cells if c[:3] == (k, kr, int(perm)) and max(c[3], 1 << 20) <= n_el <= c[4] for t in range(c[5], c[6] + 1)})
        assert [t for t in range(0, 52) if route(12, k, kr, O, I, t, perm)] == said
        assert said == list(range(said[0], said[-1] + 1)) if said else True          # one interval of token counts
        assert [t for t in range(0, 52) if route(12, k, kr, O, I, t)] == sorted(
            set(said) | {t for t in range(0, 52) if route(12, k, kr, O, I, t, not perm)})
    monkeypatch.setattr(bd, "_GEMM_GATHER12W_MODE", "1")
    for (k, kr), perm in itertools.product(FORMATS, (None, False, True)):
        assert [t for t in range(0, 52) if route(12, k, kr, 1020, 4096, t, perm)] == list(range(17, 49))
        assert not any(route(v, k, kr, 4096, 4096, 24, perm) for v in (6, 8, 16)) and not route(12, k, kr, 4092, 4100, 24, perm)
    monkeypatch.setattr(bd, "_GEMM_GATHER12W_MODE", "0")
    assert not any(route(12, k, kr, O, I, t) for k, kr in FORMATS for O, I in SHAPES for t in range(0, 52))
    # the fifth table: one record, behind the four others in what the callers walk; the four older tables are what they were
    (r,) = bd.BATCHED_DECODE_V12_WIDE_ROUTES
    assert (r.entry, r.min_tokens, r.max_tokens, r.perm, r.workspace, r.perm_cells, r.off_flags, r.exact_only, r.knob, r.extra) == \
        (ENTRY, 17, 48, None, True, True, B.GEMV_FORCE_GENERIC, False, "_GEMM_GATHER12W_MODE", (0,))
    assert r.route is bd.gemm_gather12w_route and r.owns is bd._v12_owns
    older = (bd.BATCHED_DECODE_ROUTES, bd.BATCHED_DECODE_WIDE_ROUTES, bd.BATCHED_DECODE_V12_ROUTES, bd.BATCHED_DECODE_V12_COLUMN_ROUTES)
    assert [len(t) for t in older] == [5, 1, 1, 1] and [t[-1].entry for t in older] == [
        "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gatherxw", "vptq_quant_gemm_gather12", "vptq_quant_gemm_gather12c"]
    for (k, kr), perm in itertools.product(FORMATS, (False, True)):
        static = (12, k, kr, 1, False, True, perm)
        assert bd.batched_decode_v12_wide_routes(*static) == (r,) and bd.batched_decode_v12_routes(*static) == bd.BATCHED_DECODE_V12_ROUTES
        assert bd.batched_decode_v12_column_routes(*static) == bd.BATCHED_DECODE_V12_COLUMN_ROUTES
        assert bd.batched_decode_routes(*static) == () and bd.batched_decode_wide_routes(*static) == ()
        assert bd.batched_decode_v12_wide_routes(12, k, kr, 2, False, True, perm) == ()
    assert bd.batched_decode_v12_wide_routes(8, 65536, 256, 1, False, True, True) == bd.batched_decode_v12_wide_routes(16, 65536, 1024, 1, False, True, False) == ()
    monkeypatch.setattr(bd, "_GEMM_GATHER12W_MODE", "1")
    assert bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 24, 0, True) and not bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 16, 0, True)
    assert not bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 24, B.GEMV_FORCE_GENERIC, False)
