"""Host side of vptq_quant_gemm_gather12w_grouped (gemm_gather12w_grouped.hip; added within ABI 12), without a GPU: the instance line and
the workspace layout restated, `_supported` and the return codes with fake pointers, the route function, the record
`GROUPED_DECODE_V12_WIDE_ROUTES` behind its reader, the older readers as they were, and what a `SiblingGroup` answers as shipped."""
import ctypes

import pytest

from test_gemm_gather_cpu import X, Y, CUS   # fake aligned pointers; nothing is dereferenced by host logic
from test_gemm_gather12_cpu import fdesc, want as want12, WS
from test_gemm_gather12_grouped_cpu import RULE, group, ys, members, V12, QKV, KV, TILE, MAX_PARTS
from vptq_amd import _backend as B

ENTRY = "vptq_quant_gemm_gather12w_grouped"


def line(ds, tokens, parts):
    buf = ctypes.create_string_buffer(384)
    rc = getattr(B.lib(), ENTRY + "_instance")(group(ds), len(ds), tokens, 0, parts, buf, len(buf))
    return rc, buf.value.decode()


def split(ds, tokens, parts, cus=CUS):
    """(S, tiles per part, wgcu, row groups per member, token blocks) of gemm_gather12w_grouped_decide, restated"""
    tiles, groups, tb = (ds[0].group_size + TILE - 1) // TILE, [(d.num_indices + 3) // 4 for d in ds], (tokens + 15) // 16
    by_lds = int(want12(ds[0], 1, cus).split("wgcu=")[1].split()[0])
    wgcu = 1 if tb == 3 and ds[0].num_res_centroids else by_lds   # (g12wg_min_wg)
    ask = parts if parts else RULE(tiles, sum(groups), cus * wgcu)   # (the slots of the instantiation that runs)
    tpp = -(-tiles // max(1, min(ask, tiles, MAX_PARTS)))
    return -(-tiles // tpp), tpp, wgcu, groups, tb


def want(ds, tokens, parts, cus=CUS):
    """the launches (grouped_gather_decide, gemm_gather12w_grouped_decide), restated"""
    S, tpp, wgcu, groups, tb = split(ds, tokens, parts, cus)
    k, G = len({d.perm for d in ds if d.perm}), ds[0].group_size
    head = f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + 63) // 64}x{(tokens + 3) // 4} tpt=4 perms={k}" if k else "none"
    plain = B.LayerDesc.from_buffer_copy(ds[0])
    plain.perm = None
    fmt = want12(plain, tokens, cus).split(" tiles=")[0].replace("gemm_gather12 ", "gemm_gather12w_grouped ")
    items = sum(groups) * S
    grid = min(items, cus * wgcu)
    dt = "f16" if ds[0].dtype == 0 else "bf16"
    tail = f" | gemm_gather12w_grouped_sum dt={dt} parts={S} grid={sum((d.out_features + 255) // 256 for d in ds)}x{tokens}" if S >= 2 else ""
    return (f"{head} | {fmt} tb={tb} n={len(ds)} groups={'+'.join(map(str, groups))} tiles={(G + TILE - 1) // TILE} parts={S} tpp={tpp} "
            f"wgcu={wgcu} items={items} grid={grid} rgs={(items + grid - 1) // grid}{tail}")


def want_bytes(ds, tokens, parts, cus=CUS):
    S, groups = split(ds, tokens, parts, cus)[0], split(ds, tokens, parts, cus)[3]
    xp = len({d.perm for d in ds if d.perm}) * ((tokens * ds[0].group_size * 2 + 255) // 256 * 256)
    return xp + (sum((S * tokens * g * 48 * 4 + 255) // 256 * 256 for g in groups) if S >= 2 else 0)


CASES = [   # (members, tokens, parts): S = 1 against S >= 2, the rule, 2 - 4 members, 0 / 1 / 2 distinct permutations, every RES, W = 1 and 2
    (members(65536, 4096, 4096, QKV, (1, 1, 1)), 24, 0), (members(65536, 4096, 4096, QKV, (1, 1, 1)), 48, 0), (members(65536, 4096, 4096, KV), 33, 0),
    (members(65536, 0, 4096, (14336, 14336), dtype=1), 48, 0), (members(65536, 256, 2312, (56, 20, 100), (1, 0, 2)), 17, 3),
    (members(65536, 256, 2312, (56, 20, 100, 56), (0, 1, 1)), 47, 1), (members(32768, 1024, 520, (48 * 200 - 4, 48 * 150, 48 * 180 - 40), dtype=1), 40, 2),
    (members(65536, 0, 504, (56, 20)), 32, 5), (members(65536, 4096, 8192, (8192, 1024, 1024), (1, 1, 1), dtype=1), 33, 99)]


@pytest.mark.parametrize("ds,tokens,parts", CASES)
def test_instance_line_and_workspace_layout(ds, tokens, parts):
    lib, n = B.lib(), len(ds)
    assert getattr(lib, ENTRY + "_supported")(group(ds), n, tokens, parts) == 1
    assert line(ds, tokens, parts) == (0, want(ds, tokens, parts)), (line(ds, tokens, parts), want(ds, tokens, parts))
    assert getattr(lib, ENTRY + "_workspace_bytes")(group(ds), n, tokens, parts) == want_bytes(ds, tokens, parts)
    assert (" | gemm_gather12w_grouped_sum " in line(ds, tokens, parts)[1]) == (split(ds, tokens, parts)[0] >= 2)


def test_symbols_and_the_two_residencies():
    raw = ctypes.CDLL(B.LIB_PATH)
    header = open(B.LIB_PATH.rsplit("/vptq_amd/", 1)[0] + "/include/vptq_hip.h").read()
    for s in (ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY, ENTRY + "_instance"):
        assert hasattr(raw, s) and s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1] and f" {s}(const VptqLayerDesc* descs" in header, s
    assert B.lib().vptq_abi_version() == 12
    # W = 2 (512 slots at 256 CUs), and W = 1 with a residual table and three token blocks: the grid and the rule's slots halve
    assert split(members(65536, 4096, 4096, QKV), 32, 0)[:3] == (8, 1, 2) and split(members(65536, 4096, 4096, QKV), 33, 0)[:3] == (4, 2, 1)
    assert line(members(65536, 256, 2312, (56, 20), dtype=1), 48, 1)[1] == \
        "none | gemm_gather12w_grouped dt=bf16 ib=16 rb=8 res=lds tok=48 tb=3 n=2 groups=2+1 tiles=5 parts=1 tpp=5 wgcu=1 items=3 grid=3 rgs=1"


def test_supported_and_return_codes_before_any_launch():
    lib = B.lib()
    sup, ws, call = (getattr(lib, ENTRY + s) for s in ("_supported", "_workspace_bytes", ""))
    good = members(65536, 4096, 4096, QKV, (1, 0, 1))
    assert [sup(group(good), 3, t, 0) for t in (16, 17, 48, 49)] == [0, 1, 1, 0]
    for n in (1, 5):
        ds = members(65536, 4096, 4096, (1024,) * n)
        assert sup(group(ds), n, 24, 0) == 0 and ws(group(ds), n, 24, 0) == 0 and call(group(ds), n, X, ys(n), 24, 0, 0, WS, 1 << 30, None) == B.E_UNSUPPORTED
    for tokens in (16, 49):                                   # the token window is checked before the group
        assert call(group(good), 3, X, ys(3), tokens, 0, 0, WS, 1 << 30, None) == B.E_TOKENS and line(good, tokens, 0)[0] == B.E_TOKENS
    assert sup(group(good), 3, 24, -1) == 0 and call(group(good), 3, X, ys(3), 24, 0, -1, WS, 1 << 30, None) == B.E_UNSUPPORTED
    mixed = {"format": members(65536, 4096, 4096, KV)[:1] + members(65536, 256, 4096, KV)[:1],
             "dtype": members(65536, 0, 4096, KV)[:1] + members(65536, 0, 4096, KV, dtype=1)[:1],
             "width": members(65536, 0, 4096, KV)[:1] + members(65536, 0, 2048, KV)[:1],
             "v = 8": members(65536, 4096, 4096, KV)[:1] + [fdesc(65536, 4096, v=8, O=1024)]}
    for what, ds in mixed.items():
        assert sup(group(ds), 2, 24, 0) == 0 and ws(group(ds), 2, 24, 0) == 0, what
        assert call(group(ds), 2, X, ys(2), 24, 0, 0, WS, 1 << 30, None) == B.E_UNSUPPORTED and line(ds, 24, 0)[0] == B.E_UNSUPPORTED, what
        assert b"member 1" in lib.vptq_last_error(), (what, lib.vptq_last_error())
    g, need = group(good), ws(group(good), 3, 24, 2)
    assert need == want_bytes(good, 24, 2) and sup(g, 3, 24, 2) == 1 and sup(None, 3, 24, 2) == 0
    assert call(None, 3, X, ys(3), 24, 0, 2, WS, need, None) == B.E_NULL and call(g, 3, None, ys(3), 24, 0, 2, WS, need, None) == B.E_NULL
    assert call(g, 3, X, None, 24, 0, 2, WS, need, None) == B.E_NULL and call(g, 3, X, ys(3, null=1), 24, 0, 2, WS, need, None) == B.E_NULL
    assert call(g, 3, X + 8, ys(3), 24, 0, 2, WS, need, None) == B.E_UNSUPPORTED
    assert call(g, 3, X, ys(3), 24, 0, 2, None, 0, None) == B.E_WORKSPACE and call(g, 3, X, ys(3), 24, 0, 2, WS, need - 1, None) == B.E_WORKSPACE
    assert call(g, 3, X, ys(3), 24, 0, 2, WS + 8, need, None) == B.E_ALIGN
    plain = members(65536, 4096, 4096, KV)                                                # no permutation: a workspace only where split
    assert ws(group(plain), 2, 24, 1) == 0 and ws(group(plain), 2, 24, 2) == 2 * (2 * 24 * 22 * 48 * 4)


def test_route_function_knob_window_ownership_and_floor(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route = gd.gemm_gather12w_grouped_route
    assert gd._GEMM_GATHER12W_GROUPED_MODE == "auto"
    assert (gd.GEMM_GATHER12W_GROUPED_MIN_TOKENS, gd.GEMM_GATHER12W_GROUPED_MAX_TOKENS, gd.GEMM_GATHER12W_GROUPED_MIN_ELEMENTS, gd.GEMM_GATHER12W_GROUPED_MAX_MEMBERS) == (17, 48, 1 << 20, 4)
    # auto follows a table exactly: member count, both size columns, the token interval, has_perm; None and a size under the floor never
    monkeypatch.setattr(gd, "_GEMM_GATHER12W_GROUPED_CELLS", ((65536, 4096, True, 3, 1 << 19, 3 << 20, 17, 40), (65536, 0, False, 2, 9 << 20, None, 24, 48)))
    assert [t for t in range(64) if route(12, 65536, 4096, QKV, 4096, t, True)] == list(range(17, 41))       # 2.1 M elements
    assert gd.gemm_gather12w_grouped_tokens(12, 65536, 4096, QKV, 4096, True) == tuple(range(17, 41))
    assert not any(route(12, 65536, 4096, QKV, 4096, 24, p) for p in (False, None)) and not route(12, 65536, 4096, (8192, 1024, 1024), 8192, 24, True)
    assert not route(12, 65536, 4096, (1024, 1024, 512), 4096, 24, True)                  # 215 x 4096 = 0.84 M elements: under the 1 M floor
    assert [t for t in range(64) if route(12, 65536, 0, (14336, 14336), 4096, t, False)] == list(range(24, 49)) and not route(12, 65536, 0, KV, 4096, 24, False)
    # the knob at 1: every group of the v = 12 formats in 17 .. 48, whatever its size and permutations - and no other format
    monkeypatch.setattr(gd, "_GEMM_GATHER12W_GROUPED_MODE", "1")
    assert all(route(v, k, kr, (56, 20), 520, t, p) for v, k, kr in V12 + [(12, 32768, 1024)] for t in (17, 33, 48) for p in (False, True, None))
    assert not any(route(12, 65536, 4096, QKV, 4096, t, True) for t in (0, 5, 16, 49, 64))
    assert not any(route(v, k, kr, QKV, 4096, 24, True) for v, k, kr in [(8, 65536, 256), (8, 256, 256), (16, 65536, 1024), (8, 65536, 4096), (6, 65536, 0)])
    assert not route(12, 65536, 0, (4096,), 4096, 24, True) and not route(12, 65536, 0, QKV + KV, 4096, 24, True) and not route(12, 65536, 0, QKV, 4100, 24, True)
    monkeypatch.setattr(gd, "_GEMM_GATHER12W_GROUPED_MODE", "0")
    assert not any(route(v, k, kr, QKV, 4096, t, True) for v, k, kr in V12 for t in range(64))


def test_the_new_record_sits_behind_its_reader_and_the_older_readers_answer_as_before():
    import sys
    from vptq_amd import grouped_decode as gd
    from vptq_amd import ops
    assert [(r.entry, r.min_tokens, r.max_tokens, r.off_flags, r.exact_only, r.extra) for r in gd.GROUPED_DECODE_V12_WIDE_ROUTES] == \
        [(ENTRY, 17, 48, B.GEMV_FORCE_GENERIC, False, (0,))]
    new = gd.GROUPED_DECODE_V12_WIDE_ROUTES[0]
    assert callable(ops.quant_gemm_gather12w_grouped) and "quant_gemm_gather12w_grouped" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    tables = (gd.GROUPED_DECODE_ROUTES, gd.GROUPED_DECODE_WIDE_ROUTES, gd.GROUPED_DECODE_X_ROUTES, gd.GROUPED_DECODE_X_WIDE_ROUTES, gd.GROUPED_DECODE_V12_ROUTES)
    assert [len(t) for t in tables] == [2, 1, 1, 1, 1] and all(new not in t for t in tables)
    for v, k, kr in [(16, 65536, 1024), (8, 32768, 0), (8, 65536, 4096), (8, 65536, 256), (8, 256, 256), (4, 65536, 0), (12, 65536, 4096), (12, 65536, 0)]:
        old, got = gd.sibling_group_v12_routes(v, k, kr), gd.sibling_group_v12_wide_routes(v, k, kr)
        assert got[:len(old)] == old and got[len(old):] == ((new,) if v == 12 else ()) and new.owns(v, k, kr) == (v == 12)
        assert new not in old + gd.sibling_group_routes(v, k, kr) + gd.sibling_decode_routes(v, k, kr) + gd.grouped_decode_routes(v, k, kr)
    assert [r.entry for r in gd.sibling_group_v12_wide_routes(12, 65536, 256)] == ["vptq_quant_gemm_gather12_grouped", ENTRY]
    assert (gd.GROUPED_DECODE_MIN_TOKENS, gd.GROUPED_DECODE_MAX_TOKENS) == (5, 48)        # the callers' guard holds the new window


def test_a_v12_sibling_group_answers_what_the_cells_say(monkeypatch):
    import types
    from vptq_amd import grouped_decode as gd
    from vptq_amd.layers.vqlinear import SiblingGroup

    def answers(outs, I=4096, kr=4096):
        ms = [types.SimpleNamespace(vector_len=12, num_centroids=65536, num_res_centroids=kr, in_features=I, out_features=O, num_codebooks=1,
                                    enable_outlier=False, enable_norm=True, enable_perm=True, enable_residual=kr > 0) for O in outs]
        g = SiblingGroup(ms)
        st = g._batched_static()
        return st, [t for t in range(17, 49) if (r := g._batched_route(t)) is not None and r.route(*st[:5], t, st[5])]
    st, got = answers(QKV)
    assert st == (12, 65536, 4096, QKV, 4096, True) and got == list(gd.gemm_gather12w_grouped_tokens(*st))
    assert got == [t for t in range(17, 49) if any((k, kr) == (65536, 4096) and p and n == 3 and lo <= t <= hi
                                                   for k, kr, p, n, _, _, lo, hi in gd._GEMM_GATHER12W_GROUPED_CELLS)]
    monkeypatch.setattr(gd, "_GEMM_GATHER12W_GROUPED_MODE", "1")
    assert answers(QKV)[1] == list(range(17, 49)) and answers((56, 20), 520, 0)[1] == list(range(17, 49))
