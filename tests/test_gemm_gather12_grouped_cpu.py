"""Host side of vptq_quant_gemm_gather12_grouped (gemm_gather12_grouped.hip; added within ABI 12), without a GPU: the instance line and
the workspace layout restated, `_supported` and the return codes with fake pointers, the route function, the record
`GROUPED_DECODE_V12_ROUTES` behind its reader, and the four older readers as they were."""
import ctypes

import pytest

from test_gemm_gather_cpu import X, Y, CUS   # fake aligned pointers; nothing is dereferenced by host logic
from test_gemm_gather12_cpu import fdesc, want as want12, WS
from vptq_amd import _backend as B

ENTRY = "vptq_quant_gemm_gather12_grouped"
TILE, MAX_PARTS = 512, 16
V12 = [(12, 65536, 0), (12, 65536, 256), (12, 65536, 4096)]
QKV, KV = (4096, 1024, 1024), (1024, 1024)


def group(ds):
    return (B.LayerDesc * len(ds))(*ds)


def ys(n, null=None):
    return (ctypes.c_void_p * n)(*[None if m == null else Y + (m << 16) for m in range(n)])


def line(ds, tokens, parts):
    buf = ctypes.create_string_buffer(384)
    rc = getattr(B.lib(), ENTRY + "_instance")(group(ds), len(ds), tokens, 0, parts, buf, len(buf))
    return rc, buf.value.decode()


def RULE(tiles, groups, slots):
    """parts == 0: gemm_gather12w's rule, the v = 12 rule that allows one part (gemm_gather12w.hip), restated"""
    if 4 * groups > 5 * slots:
        return 1
    for even in (True, False):
        for tpp in range(1, tiles + 1):
            S = -(-tiles // tpp)
            if S <= MAX_PARTS and not (even and tiles % tpp) and 2 * groups * S <= 5 * slots:
                return S
    return 1


def split(ds, parts, cus=CUS):
    """(S, tiles per part, wgcu, row groups per member) of gemm_gather12_grouped_decide, restated"""
    tiles, groups = (ds[0].group_size + TILE - 1) // TILE, [(d.num_indices + 3) // 4 for d in ds]
    wgcu = int(want12(ds[0], 1, cus).split("wgcu=")[1].split()[0])
    ask = parts if parts else RULE(tiles, sum(groups), cus * wgcu)
    tpp = -(-tiles // max(1, min(ask, tiles, MAX_PARTS)))
    return -(-tiles // tpp), tpp, wgcu, groups


def want(ds, tokens, parts, cus=CUS):
    """the launches (grouped_gather_decide, gemm_gather12_grouped_decide), restated"""
    S, tpp, wgcu, groups = split(ds, parts, cus)
    k, G = len({d.perm for d in ds if d.perm}), ds[0].group_size
    head = f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + 63) // 64}x{(tokens + 3) // 4} tpt=4 perms={k}" if k else "none"
    plain = B.LayerDesc.from_buffer_copy(ds[0])
    plain.perm = None
    fmt = want12(plain, tokens, cus).split(" tiles=")[0].replace("gemm_gather12 ", "gemm_gather12_grouped ")
    items = sum(groups) * S
    grid = min(items, cus * wgcu)
    dt = "f16" if ds[0].dtype == 0 else "bf16"
    tail = f" | gemm_gather12_grouped_sum dt={dt} parts={S} grid={sum((d.out_features + 255) // 256 for d in ds)}x{tokens}" if S >= 2 else ""
    return (f"{head} | {fmt} n={len(ds)} groups={'+'.join(map(str, groups))} tiles={(G + TILE - 1) // TILE} parts={S} tpp={tpp} wgcu={wgcu} "
            f"items={items} grid={grid} rgs={(items + grid - 1) // grid}{tail}")


def want_bytes(ds, tokens, parts, cus=CUS):
    S, _, _, groups = split(ds, parts, cus)
    xp = len({d.perm for d in ds if d.perm}) * ((tokens * ds[0].group_size * 2 + 255) // 256 * 256)
    return xp + (sum((S * tokens * g * 48 * 4 + 255) // 256 * 256 for g in groups) if S >= 2 else 0)


def members(k, kr, I, outs, perms=(), dtype=0):
    """members of one format; perms: per member 0 (none) or the id of its permutation (equal ids share one perm pointer)"""
    ds = [fdesc(k, kr, I=I, O=O, dtype=dtype, perm=bool(m < len(perms) and perms[m])) for m, O in enumerate(outs)]
    for m, d in enumerate(ds):
        if d.perm:
            d.perm += perms[m] << 12
    return ds


CASES = [   # (members, tokens, parts): S = 1 against S >= 2, the rule, 2 - 4 members, 0 / 1 / 2 distinct permutations, every RES
    (members(65536, 4096, 4096, QKV, (1, 1, 1)), 8, 0), (members(65536, 4096, 4096, KV), 16, 0), (members(65536, 0, 4096, (14336, 14336), dtype=1), 5, 0),
    (members(65536, 256, 2312, (56, 20, 100), (1, 0, 2)), 9, 3), (members(65536, 256, 2312, (56, 20, 100, 56), (0, 1, 1)), 15, 1),
    (members(32768, 1024, 520, (48 * 200 - 4, 48 * 150, 48 * 180 - 40), dtype=1), 5, 2), (members(65536, 0, 504, (56, 20)), 1, 5),
    (members(65536, 4096, 8192, (8192, 1024, 1024), (1, 1, 1), dtype=1), 16, 99)]


@pytest.mark.parametrize("ds,tokens,parts", CASES)
def test_instance_line_and_workspace_layout(ds, tokens, parts):
    lib, n = B.lib(), len(ds)
    assert getattr(lib, ENTRY + "_supported")(group(ds), n, tokens, parts) == 1
    assert line(ds, tokens, parts) == (0, want(ds, tokens, parts)), (line(ds, tokens, parts), want(ds, tokens, parts))
    assert getattr(lib, ENTRY + "_workspace_bytes")(group(ds), n, tokens, parts) == want_bytes(ds, tokens, parts)
    assert (" | gemm_gather12_grouped_sum " in line(ds, tokens, parts)[1]) == (split(ds, parts)[0] >= 2)


def test_the_rule_cuts_the_8b_groups_into_one_tile_parts():
    assert split(members(65536, 4096, 4096, QKV), 0)[:2] == (8, 1) and split(members(65536, 4096, 4096, KV), 0)[:2] == (8, 1)   # 130 / 44 row groups
    assert split(members(65536, 0, 8192, (28672, 28672)), 0)[0] == 1 and split(members(65536, 0, 504, KV), 7)[:2] == (1, 1)    # 1196 row groups; one tile
    assert line(members(65536, 256, 2312, (56, 20), dtype=1), 16, 1)[1] == \
        "none | gemm_gather12_grouped dt=bf16 ib=16 rb=8 res=lds tok=16 n=2 groups=2+1 tiles=5 parts=1 tpp=5 wgcu=2 items=3 grid=3 rgs=1"


def test_supported_and_return_codes_before_any_launch():
    lib = B.lib()
    sup, ws, call = (getattr(lib, ENTRY + s) for s in ("_supported", "_workspace_bytes", ""))
    good = members(65536, 4096, 4096, QKV, (1, 0, 1))
    for n in (1, 5):
        ds = members(65536, 4096, 4096, (1024,) * n)
        assert sup(group(ds), n, 8, 0) == 0 and ws(group(ds), n, 8, 0) == 0 and call(group(ds), n, X, ys(n), 8, 0, 0, WS, 1 << 30, None) == B.E_UNSUPPORTED
    for tokens in (0, 17):
        assert sup(group(good), 3, tokens, 0) == 0 and call(group(good), 3, X, ys(3), tokens, 0, 0, WS, 1 << 30, None) == B.E_TOKENS
        assert line(good, tokens, 0)[0] == B.E_TOKENS
    assert sup(group(good), 3, 8, -1) == 0 and call(group(good), 3, X, ys(3), 8, 0, -1, WS, 1 << 30, None) == B.E_UNSUPPORTED
    mixed = {"format": members(65536, 4096, 4096, KV)[:1] + members(65536, 256, 4096, KV)[:1],
             "dtype": members(65536, 0, 4096, KV)[:1] + members(65536, 0, 4096, KV, dtype=1)[:1],
             "width": members(65536, 0, 4096, KV)[:1] + members(65536, 0, 2048, KV)[:1],
             "v = 8": members(65536, 4096, 4096, KV)[:1] + [fdesc(65536, 4096, v=8, O=1024)]}
    for what, ds in mixed.items():
        assert sup(group(ds), 2, 8, 0) == 0 and ws(group(ds), 2, 8, 0) == 0, what
        assert call(group(ds), 2, X, ys(2), 8, 0, 0, WS, 1 << 30, None) == B.E_UNSUPPORTED and line(ds, 8, 0)[0] == B.E_UNSUPPORTED, what
        assert b"member 1" in lib.vptq_last_error(), (what, lib.vptq_last_error())
    g, need = group(good), ws(group(good), 3, 8, 2)
    assert need == want_bytes(good, 8, 2) and sup(g, 3, 8, 2) == 1 and sup(None, 3, 8, 2) == 0
    assert call(None, 3, X, ys(3), 8, 0, 2, WS, need, None) == B.E_NULL and call(g, 3, None, ys(3), 8, 0, 2, WS, need, None) == B.E_NULL
    assert call(g, 3, X, None, 8, 0, 2, WS, need, None) == B.E_NULL and call(g, 3, X, ys(3, null=1), 8, 0, 2, WS, need, None) == B.E_NULL
    assert call(g, 3, X + 8, ys(3), 8, 0, 2, WS, need, None) == B.E_UNSUPPORTED
    assert call(g, 3, X, ys(3), 8, 0, 2, None, 0, None) == B.E_WORKSPACE and call(g, 3, X, ys(3), 8, 0, 2, WS, need - 1, None) == B.E_WORKSPACE
    assert call(g, 3, X, ys(3), 8, 0, 2, WS + 8, need, None) == B.E_ALIGN
    plain = members(65536, 4096, 4096, KV)                                                # no permutation: a workspace only where split
    assert ws(group(plain), 2, 8, 1) == 0 and ws(group(plain), 2, 8, 2) == 2 * (2 * 8 * 22 * 48 * 4)
    assert call(group(plain), 2, X, ys(2), 8, 0, 2, None, 0, None) == B.E_WORKSPACE


def test_route_function_knob_window_ownership_and_floor(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route = gd.gemm_gather12_grouped_route
    assert gd._GEMM_GATHER12_GROUPED_MODE == "auto"
    assert '_GEMM_GATHER12_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHER12_GROUPED", "auto") or "auto").strip().lower()' in open(gd.__file__).read()
    assert (gd.GEMM_GATHER12_GROUPED_MIN_TOKENS, gd.GEMM_GATHER12_GROUPED_MAX_TOKENS, gd.GEMM_GATHER12_GROUPED_MIN_ELEMENTS) == (5, 16, 1 << 20)
    cells = gd._GEMM_GATHER12_GROUPED_CELLS
    assert isinstance(cells, tuple) and all(len(c) == 8 and (12,) + c[:2] in V12 and c[2] in (False, True) and 2 <= c[3] <= 4 and c[4] >= 1 << 20 and
                                            (c[5] is None or c[5] >= c[4]) and 5 <= c[6] <= c[7] <= 16 for c in cells)
    # auto follows a table exactly: member count, both size columns, the token interval, has_perm; None and a size under the floor never
    monkeypatch.setattr(gd, "_GEMM_GATHER12_GROUPED_CELLS", ((65536, 4096, True, 3, 1 << 19, 3 << 20, 5, 12), (65536, 0, False, 2, 9 << 20, None, 9, 16)))
    assert [t for t in range(24) if route(12, 65536, 4096, QKV, 4096, t, True)] == list(range(5, 13))       # 2.1 M elements
    assert gd.gemm_gather12_grouped_tokens(12, 65536, 4096, QKV, 4096, True) == tuple(range(5, 13))
    assert not any(route(12, 65536, 4096, QKV, 4096, 8, p) for p in (False, None)) and not route(12, 65536, 4096, (8192, 1024, 1024), 8192, 8, True)
    assert not route(12, 65536, 4096, (1024, 1024, 512), 4096, 8, True)                   # 215 x 4096 = 0.84 M elements: under the 1 M floor
    assert [t for t in range(24) if route(12, 65536, 0, (14336, 14336), 4096, t, False)] == list(range(9, 17)) and not route(12, 65536, 0, KV, 4096, 9, False)
    # the knob at 1: every group of the v = 12 formats in 5 .. 16, whatever its size and permutations - and no other format
    monkeypatch.setattr(gd, "_GEMM_GATHER12_GROUPED_MODE", "1")
    assert all(route(v, k, kr, (56, 20), 520, t, p) for v, k, kr in V12 + [(12, 32768, 1024)] for t in (5, 9, 16) for p in (False, True, None))
    assert not any(route(12, 65536, 4096, QKV, 4096, t, True) for t in (0, 4, 17, 48))
    assert not any(route(v, k, kr, QKV, 4096, 8, True) for v, k, kr in [(8, 65536, 256), (8, 256, 256), (16, 65536, 1024), (8, 65536, 4096), (6, 65536, 0)])
    assert not route(12, 65536, 0, (4096,), 4096, 8, True) and not route(12, 65536, 0, QKV + KV, 4096, 8, True) and not route(12, 65536, 0, QKV, 4100, 8, True)
    monkeypatch.setattr(gd, "_GEMM_GATHER12_GROUPED_MODE", "0")
    assert not any(route(v, k, kr, QKV, 4096, t, True) for v, k, kr in V12 for t in range(24))


def test_the_new_record_sits_behind_its_reader_and_the_older_readers_answer_as_before():
    from vptq_amd import grouped_decode as gd
    from vptq_amd import ops
    assert [(r.entry, r.min_tokens, r.max_tokens, r.off_flags, r.exact_only, r.extra) for r in gd.GROUPED_DECODE_V12_ROUTES] == \
        [(ENTRY, 5, 16, B.GEMV_FORCE_GENERIC, False, (0,))]
    new = gd.GROUPED_DECODE_V12_ROUTES[0]
    import sys
    assert callable(ops.quant_gemm_gather12_grouped) and "quant_gemm_gather12_grouped" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    tables = (gd.GROUPED_DECODE_ROUTES, gd.GROUPED_DECODE_WIDE_ROUTES, gd.GROUPED_DECODE_X_ROUTES, gd.GROUPED_DECODE_X_WIDE_ROUTES)
    assert [len(t) for t in tables] == [2, 1, 1, 1] and all(r.extra == () for t in tables for r in t)
    # test_gemm_gatherxw_grouped_cpu's formats + the published v = 12 one: the four older readers know no v = 12 record
    for v, k, kr in [(16, 65536, 1024), (8, 32768, 0), (8, 65536, 4096), (8, 65536, 256), (8, 65536, 0), (8, 256, 256), (8, 4096, 256), (4, 65536, 0),
                     (12, 65536, 4096)]:
        old, got = gd.sibling_group_routes(v, k, kr), gd.sibling_group_v12_routes(v, k, kr)
        assert got[:len(old)] == old and got[len(old):] == ((new,) if v == 12 else ()) and new.owns(v, k, kr) == (v == 12)
        assert new not in old + gd.sibling_decode_routes(v, k, kr) + gd.grouped_decode_routes(v, k, kr) and gd.grouped_decode_route(v, k, kr) is not new
    assert gd.sibling_group_routes(12, 65536, 4096) == gd.sibling_decode_routes(12, 65536, 4096) == gd.grouped_decode_routes(12, 65536, 4096) == ()
    assert gd.grouped_decode_route(12, 65536, 4096) is None
    assert [r.entry for r in gd.sibling_group_routes(8, 65536, 256)] == ["vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gatherw_grouped"]
    assert [r.entry for r in gd.sibling_group_routes(16, 65536, 1024)] == ["vptq_quant_gemm_gatherx_grouped", "vptq_quant_gemm_gatherxw_grouped"]
    assert [r.entry for r in gd.sibling_group_routes(8, 256, 256)] == ["vptq_quant_gemm_k256_grouped"]
    assert (gd.GROUPED_DECODE_MIN_TOKENS, gd.GROUPED_DECODE_MAX_TOKENS) == (5, 48)        # the callers' guard holds the new window
