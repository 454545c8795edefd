"""Host side of vptq_quant_gemm_gather12c (gemm_gather12c.hip; added within ABI 12), without a GPU: symbols, the partition arithmetic
behind `_supported`, the workspace query and the instance line, validation before any launch, the route function and the fourth table."""
import ctypes
import itertools

from test_gemm_gather_cpu import X, Y, CUS   # fake aligned pointers; nothing is dereferenced by host logic
from test_gemm_gather12_cpu import fdesc, want as want12, FORMATS, SHAPES, WS
from vptq_amd import _backend as B

ENTRY = "vptq_quant_gemm_gather12c"
TILE, MAX_PARTS = 512, 16


def line(d, tokens, parts, flags=0):
    buf = ctypes.create_string_buffer(320)
    rc = B.lib().vptq_quant_gemm_gather12c_instance(d, tokens, flags, parts, buf, len(buf))
    return rc, buf.value.decode()


def split(d, parts, cus=CUS):
    """(S, tiles per part) of gemm_gather12c_decide, restated; wgcu is the parent's, 2 or what the LDS leaves"""
    tiles, groups = (d.group_size + TILE - 1) // TILE, (d.num_indices + 3) // 4
    wgcu = int(want12(d, 1, cus).split("wgcu=")[1].split()[0])
    ask = parts if parts else RULE(groups, tiles, cus * wgcu)
    tpp = -(-tiles // max(1, min(ask, tiles, MAX_PARTS)))
    return -(-tiles // tpp), tpp, wgcu, groups


def RULE(groups, tiles, slots):
    """parts == 0 (g12c_rule_parts): the smallest tiles-per-part that divides the tile count, gives at most 16 parts and keeps the items
    within 2.5 x the resident slots; without such a divisor the smallest tiles-per-part that keeps the bound; else two parts"""
    for even in (True, False):
        for tpp in range(1, tiles):
            S = -(-tiles // tpp)
            if S <= MAX_PARTS and not (even and tiles % tpp) and 2 * groups * S <= 5 * slots:
                return S
    return 2


def want(d, tokens, parts, cus=CUS):
    """the launches (gemm_gather_px_decide, gemm_gather12c_decide), restated"""
    S, tpp, wgcu, groups = split(d, parts, cus)
    grid = min(groups * S, cus * wgcu)
    head, tail = want12(d, tokens, cus).replace("gemm_gather12 ", "gemm_gather12c ").split(" wgcu=")
    dt = "f16" if d.dtype == 0 else "bf16"
    return (f"{head} parts={S} tpp={tpp} wgcu={wgcu} rgs={(groups * S + grid - 1) // grid} | "
            f"gemm_gather12c_sum dt={dt} parts={S} grid={(d.out_features + 255) // 256}x{tokens}")


def test_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in (ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY, ENTRY + "_instance"):
        assert hasattr(raw, s) and s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], s
    from vptq_amd import ops
    assert callable(ops.quant_gemm_gather12c) and B.lib().vptq_abi_version() == 12


def test_partition_arithmetic_supported_and_workspace():
    sup, ws = B.lib().vptq_quant_gemm_gather12c_supported, B.lib().vptq_quant_gemm_gather12c_workspace_bytes
    for I, parts, S, tpp in ((4096, 2, 2, 4), (4096, 3, 3, 3), (4096, 5, 4, 2), (4096, 6, 4, 2), (4096, 8, 8, 1), (4096, 99, 8, 1),   # 8 tiles
                             (2312, 2, 2, 3), (2312, 3, 3, 2), (2312, 4, 3, 2), (2312, 5, 5, 1),            # 5 tiles: 3 + 2, 2 + 2 + 1
                             (14336, 16, 14, 2), (14336, 99, 14, 2), (14336, 6, 6, 5), (520, 2, 2, 1), (520, 16, 2, 1)):
        d = fdesc(65536, 4096, I=I, O=56, perm=True)
        assert split(d, parts)[:2] == (S, tpp) and sup(d, 9, parts) == 1, (I, parts)
        assert f" parts={S} tpp={tpp} " in line(d, 9, parts)[1] and line(d, 9, parts) == (0, want(d, 9, parts))
        xp = ((9 * I * 2 + 255) // 256) * 256
        assert ws(d, 9, parts) == xp + S * 9 * 2 * 48 * 4                       # 56 outputs: 5 vector-rows, two row groups
        d.perm = None
        assert ws(d, 9, parts) == S * 9 * 2 * 48 * 4                            # a plain layer needs the partials too
    for (k, kr), dtype in itertools.product(FORMATS, (0, 1)):
        for I in (8, 504, 512):                                                 # one tile: nothing to split
            assert all(sup(fdesc(k, kr, I=I, dtype=dtype), 9, p) == 0 and ws(fdesc(k, kr, I=I), 9, p) == 0 for p in (0, 2, 16))
        assert sup(fdesc(k, kr, dtype=dtype), 9, 1) == 0 and sup(fdesc(k, kr), 9, -1) == 0 and ws(fdesc(k, kr), 9, 1) == 0   # parts == 1
        for tokens in range(-1, 19):
            assert sup(fdesc(k, kr, perm=True), tokens, 2) == int(1 <= tokens <= 16)
    assert sup(None, 9, 2) == 0 and sup(fdesc(65536, 4096, v=8, O=4096), 9, 2) == 0 and sup(fdesc(65536, 0, I=4100), 9, 2) == 0


def test_the_rule_and_instance_lines():
    cases = [(fdesc(65536, 0), 5), (fdesc(65536, 256, I=4096, O=1024, dtype=1), 9), (fdesc(65536, 4096, I=14336, O=4096, perm=True), 16),
             (fdesc(65536, 4096, I=8192, O=8184, dtype=1, perm=True), 12), (fdesc(32768, 1024, I=520, O=48 * (CUS + 2) - 8), 8),
             (fdesc(65536, 4096, I=4096, O=14328), 8)]
    for d, tokens in cases:
        assert B.lib().vptq_quant_gemm_gather12c_supported(d, tokens, 0) == (split(d, 0)[0] >= 2)
        if split(d, 0)[0] >= 2:
            assert line(d, tokens, 0) == (0, want(d, tokens, 0)), (line(d, tokens, 0), want(d, tokens, 0))
    d, tokens = cases[4]   # CUS + 2 row groups x 2 parts on 2 CUS slots: a workgroup walks two items
    assert line(d, tokens, 2)[1] == ("gemm_gather12c dt=f16 ib=15 rb=10 res=lds tok=8 tiles=2 parts=2 tpp=1 wgcu=2 rgs=2 | "
                                     f"gemm_gather12c_sum dt=f16 parts=2 grid={(48 * (CUS + 2) - 8 + 255) // 256}x8")
    assert line(cases[2][0], 16, 4)[1].startswith("permute_x_tokens g=14336 tok=16 grid=28x4 tpt=4 | gemm_gather12c dt=f16 ib=16 rb=12 res=l2 "
                                                  "tok=16 tiles=28 parts=4 tpp=7 wgcu=2 rgs=1 | gemm_gather12c_sum dt=f16 parts=4 grid=16x16")


def test_validation_order_before_any_launch():
    call = B.lib().vptq_quant_gemm_gather12c
    d, p, bad = fdesc(65536, 4096), fdesc(65536, 4096, perm=True), fdesc(65536, 4096, v=8, O=4096)
    need_d, need_p = (B.lib().vptq_quant_gemm_gather12c_workspace_bytes(q, 12, 4) for q in (d, p))
    assert call(None, X, Y, 4, 0, 4, WS, need_d, None) == B.E_NULL and call(d, None, Y, 4, 0, 4, WS, need_d, None) == B.E_NULL
    assert call(bad, None, Y, 17, 0, 4, None, 0, None) == B.E_NULL             # NULL before tokens before unsupported
    for tokens in (0, 17, -3):
        assert call(d, X, Y, tokens, 0, 4, WS, need_d, None) == B.E_TOKENS and call(bad, X, Y, tokens, 0, 4, None, 0, None) == B.E_TOKENS
    assert call(bad, X + 8, Y, 4, 0, 4, None, 0, None) == B.E_UNSUPPORTED      # unsupported before x alignment
    assert call(d, X + 8, Y, 4, 0, 1, None, 0, None) == B.E_UNSUPPORTED and call(fdesc(65536, 0, I=512), X, Y, 4, 0, 0, None, 0, None) == B.E_UNSUPPORTED
    for flags in (0, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert call(d, X + 8, Y, 12, flags, 4, WS, need_d, None) == B.E_ALIGN
        for q, need in ((d, need_d), (p, need_p)):                             # a plain layer has a workspace to check too
            assert call(q, X, Y, 12, flags, 4, None, 0, None) == B.E_WORKSPACE and call(q, X, Y, 12, flags, 4, WS, need - 1, None) == B.E_WORKSPACE
            assert call(q, X, Y, 12, flags, 4, WS + 8, need, None) == B.E_ALIGN
    assert line(d, 17, 4)[0] == B.E_TOKENS and line(bad, 4, 4)[0] == B.E_UNSUPPORTED and line(d, 4, 1)[0] == B.E_UNSUPPORTED


def test_route_function_and_the_fourth_table(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gather12c_route
    assert bd._GEMM_GATHER12C_MODE == "auto"
    assert '_GEMM_GATHER12C_MODE = (B.tune_env("VPTQ_GEMM_GATHER12C", "auto") or "auto").strip().lower()' in open(bd.__file__).read()
    # every shipped cell: seven fields, a most bound, nothing under 1 M index elements, inside 5 .. 16 tokens
    assert all(len(c) == 7 and (1 << 20) <= c[3] <= c[4] and 5 <= c[5] <= c[6] <= 16 for c in bd._GEMM_GATHER12C_CELLS)
    for cells in (bd._GEMM_GATHER12C_CELLS, ((65536, 4096, 1, 1 << 20, 5 << 20, 5, 16), (65536, 0, 0, 0, 2 << 20, 9, 12))):
        monkeypatch.setattr(bd, "_GEMM_GATHER12C_CELLS", cells)
        monkeypatch.setattr(bd, "_GEMM_GATHER12C_MODE", "auto")
        for (k, kr), (O, I), perm in itertools.product(FORMATS, SHAPES + ((1020, 4096),), (False, True)):
            n_el = ((O + 11) // 12) * I
            said = sorted({t for c in cells if c[:3] == (k, kr, int(perm)) and max(c[3], 1 << 20) <= n_el <= c[4] for t in range(c[5], c[6] + 1)})
            assert [t for t in range(0, 20) if route(12, k, kr, O, I, t, perm)] == said
            assert said == list(range(said[0], said[-1] + 1)) if said else True          # one interval of token counts
            assert [t for t in range(0, 20) if route(12, k, kr, O, I, t)] == sorted(
                set(said) | {t for t in range(0, 20) if route(12, k, kr, O, I, t, not perm)})
        monkeypatch.setattr(bd, "_GEMM_GATHER12C_MODE", "1")
        for (k, kr), perm in itertools.product(FORMATS, (None, False, True)):
            assert [t for t in range(0, 20) if route(12, k, kr, 1020, 4096, t, perm)] == list(range(5, 17))
            assert not any(route(v, k, kr, 4096, 4096, 8, perm) for v in (6, 8, 16)) and not route(12, k, kr, 4092, 4100, 8, perm)
        monkeypatch.setattr(bd, "_GEMM_GATHER12C_MODE", "0")
        assert not any(route(12, k, kr, O, I, t) for k, kr in FORMATS for O, I in SHAPES for t in range(0, 20))
    # the fourth table: one record, in front of the third's in what the callers walk; the three older tables are what they were
    (r,) = bd.BATCHED_DECODE_V12_COLUMN_ROUTES
    assert (r.entry, r.min_tokens, r.max_tokens, r.perm, r.workspace, r.perm_cells, r.off_flags, r.exact_only, r.knob, r.extra) == \
        (ENTRY, 5, 16, None, True, True, B.GEMV_FORCE_GENERIC, False, "_GEMM_GATHER12C_MODE", (0,))
    assert r.route is bd.gemm_gather12c_route
    assert [len(t) for t in (bd.BATCHED_DECODE_ROUTES, bd.BATCHED_DECODE_WIDE_ROUTES, bd.BATCHED_DECODE_V12_ROUTES)] == [5, 1, 1]
    assert all(q.extra == () for t in (bd.BATCHED_DECODE_ROUTES, bd.BATCHED_DECODE_WIDE_ROUTES, bd.BATCHED_DECODE_V12_ROUTES) for q in t)
    assert bd.BATCHED_DECODE_V12_ROUTES[0].entry == "vptq_quant_gemm_gather12"
    for (k, kr), perm in itertools.product(FORMATS, (False, True)):
        static = (12, k, kr, 1, False, True, perm)
        assert bd.batched_decode_v12_column_routes(*static) == (r,) and bd.batched_decode_v12_routes(*static) == bd.BATCHED_DECODE_V12_ROUTES
        assert bd.batched_decode_routes(*static) == () and bd.batched_decode_wide_routes(*static) == ()
        assert bd.batched_decode_v12_column_routes(12, k, kr, 2, False, True, perm) == ()
    assert bd.batched_decode_v12_column_routes(8, 65536, 256, 1, False, True, True) == ()
    monkeypatch.setattr(bd, "_GEMM_GATHER12C_MODE", "1")
    assert bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 12, 0, True) and not bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 17, 0, True)
    assert not bd.batched_decode_takes(r, 12, 65536, 4096, 4092, 4096, 12, B.GEMV_FORCE_GENERIC, False)
