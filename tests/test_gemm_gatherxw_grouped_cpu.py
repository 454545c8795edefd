"""The route of vptq_quant_gemm_gatherxw_grouped (gemm_gatherxw_grouped.hip) without a GPU: the pure route function of
vptq_amd/grouped_decode.py with its knob, window, format ownership and floor; the committed cells; the record
`GROUPED_DECODE_X_WIDE_ROUTES` behind the reader `sibling_group_routes`; the older tables and readers as they were."""
from vptq_amd import _backend as B
from test_gemm_gatherx_cpu import FORMATS, GATHER_OWNED

ENTRY = "vptq_quant_gemm_gatherxw_grouped"
CANONICAL = (8, 256, 256)
QKV, GU = (8192, 1024, 1024), (14336, 14336)


def test_route_function_knob_window_ownership_and_floor(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route, cells = gd.gemm_gatherxw_grouped_route, gd._GEMM_GATHERXW_GROUPED_CELLS
    assert (gd.GEMM_GATHERXW_GROUPED_MIN_TOKENS, gd.GEMM_GATHERXW_GROUPED_MAX_TOKENS, gd.GEMM_GATHERXW_GROUPED_MIN_ELEMENTS) == (17, 48, 2 << 20)
    # every committed cell: gemm_gatherx_grouped's format, a format of the kernel, inside the window, at or above the floor
    assert isinstance(cells, tuple) and all(len(c) == 9 and c[:3] in FORMATS and c[3] in (False, True) and 2 <= c[4] <= 4 and c[5] >= 2 << 20 and
                                            (c[6] is None or c[6] >= c[5]) and 17 <= c[7] <= c[8] <= 48 for c in cells)
    # auto follows a table exactly: member count, both size columns, the token interval, has_perm; None and a size under the floor never
    monkeypatch.setattr(gd, "_GEMM_GATHERXW_GROUPED_CELLS", ((16, 65536, 1024, True, 3, 1 << 20, 5 << 20, 17, 40), (8, 32768, 0, False, 2, 14 << 20, None, 33, 48)))
    assert [t for t in range(60) if route(16, 65536, 1024, QKV, 8192, t, True)] == list(range(17, 41))
    assert gd.gemm_gatherxw_grouped_tokens(16, 65536, 1024, QKV, 8192, True) == tuple(range(17, 41))
    assert not any(route(16, 65536, 1024, QKV, 8192, 24, p) for p in (False, None)) and not route(16, 65536, 1024, GU, 4096, 24, True)
    assert not route(16, 65536, 1024, (4096, 1024, 1024), 4096, 24, True)                 # 1.5 M elements: under the 2 M floor
    assert [t for t in range(60) if route(8, 32768, 0, GU, 4096, t, False)] == list(range(33, 49)) and route(8, 32768, 0, (28672, 28672), 8192, 48, False)
    # the knob at 1: every group of gemm_gatherx's formats in 17 .. 48, whatever its size and permutations - and no other format
    monkeypatch.setattr(gd, "_GEMM_GATHERXW_GROUPED_MODE", "1")
    assert all(route(v, k, kr, (36, 12), 1032, t, p) for v, k, kr in FORMATS for t in (17, 32, 48) for p in (False, True, None))
    assert not any(route(16, 65536, 1024, QKV, 8192, t, True) for t in (0, 5, 16, 49, 64))
    assert not any(route(v, k, kr, QKV, 8192, 24, True) for v, k, kr in GATHER_OWNED + [CANONICAL, (8, 4096, 256), (4, 65536, 0)])
    assert not route(16, 65536, 1024, (4096,), 4096, 24, True) and not route(16, 65536, 1024, QKV + GU, 4096, 24, True) and not route(16, 65536, 1024, QKV, 4100, 24, True)
    monkeypatch.setattr(gd, "_GEMM_GATHERXW_GROUPED_MODE", "0")
    assert not any(route(v, k, kr, QKV, 8192, t, True) for v, k, kr in FORMATS for t in range(60))


def test_the_new_record_sits_behind_the_reader_and_the_older_tables_answer_as_before():
    from vptq_amd import grouped_decode as gd
    assert [(r.entry, r.min_tokens, r.max_tokens, r.off_flags, r.exact_only) for r in gd.GROUPED_DECODE_X_WIDE_ROUTES] == \
        [(ENTRY, 17, 48, B.GEMV_FORCE_GENERIC, False)]
    new = gd.GROUPED_DECODE_X_WIDE_ROUTES[0]
    for v, k, kr in [(16, 65536, 1024), (8, 32768, 0), (8, 65536, 4096), (8, 65536, 256), (8, 65536, 0), CANONICAL, (8, 4096, 256), (4, 65536, 0)]:
        old, got = gd.sibling_decode_routes(v, k, kr), gd.sibling_group_routes(v, k, kr)
        assert got[:len(old)] == old and got[len(old):] == ((new,) if (v, k, kr) in FORMATS else ())
        assert new.owns(v, k, kr) == ((v, k, kr) in FORMATS)
    # the older tables and readers: a handful of their answers
    assert [r.entry for r in gd.sibling_decode_routes(16, 65536, 1024)] == ["vptq_quant_gemm_gatherx_grouped"]
    assert [r.entry for r in gd.sibling_group_routes(8, 65536, 256)] == ["vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gatherw_grouped"]
    assert [r.entry for r in gd.sibling_group_routes(*CANONICAL)] == ["vptq_quant_gemm_k256_grouped"] and gd.sibling_group_routes(8, 4096, 256) == ()
    assert [r.entry for r in gd.GROUPED_DECODE_X_ROUTES] == ["vptq_quant_gemm_gatherx_grouped"] and gd.grouped_decode_routes(16, 65536, 1024) == ()
    assert (gd.GROUPED_DECODE_MIN_TOKENS, gd.GROUPED_DECODE_MAX_TOKENS) == (5, 48)        # the callers' guard holds the new window

