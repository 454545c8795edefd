"""Host side of vptq_quant_gemm_k256_grouped (gemm_k256_grouped_kernel in gemm_k256.hip; added within ABI 12), without a GPU: the four
symbols, the `_supported` truth table held cell by cell to the member rule and the same-dtype / width rule, the workspace formula over
0 - 3 distinct perm pointers, the entry's validation (every error returns before a launch, fake pointers), the instance line computed
independently from the CU count the library reports, the pure route function of vptq_amd/grouped_decode.py with its cells and knob, the
record of the group routes, the routes of before as they were, and `SiblingGroup.forward_batched`'s host protocol over stub members of
the canonical format and a stubbed launch."""
import ctypes
import itertools
import os
import re
import types

import torch

from vptq_amd import _backend as B
from test_gemm_k256w_cpu import desc, TILE, ROWS, CUS, X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "vptq_quant_gemm_k256_grouped"
SYMBOLS = (ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY, ENTRY + "_instance")
WS = 11 << 20                     # fake, 256-byte aligned, never dereferenced
PX_THREADS, PX_TOK = 64, 4        # the permute launch: chunks of 8 columns per workgroup, tokens per thread


def arr(*ds):
    return (B.LayerDesc * len(ds))(*ds)


def ys(n, base=12 << 20):
    return (ctypes.c_void_p * n)(*[base + (i << 20) for i in range(n)])


def with_perm(d, ptr):
    d.perm, d.scale_permuted, d.bias_permuted = ptr, 7 << 20, 8 << 20
    return d


def line(ds, tokens, flags=0, size=256):
    buf = ctypes.create_string_buffer(size)
    rc = getattr(B.lib(), ENTRY + "_instance")(arr(*ds), len(ds), tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
    vp, D, i = ctypes.c_void_p, ctypes.POINTER(B.LayerDesc), ctypes.c_int
    assert B.EXPORTS[ENTRY + "_supported"] == (i, [D, i, i])
    assert B.EXPORTS[ENTRY + "_workspace_bytes"] == (ctypes.c_size_t, [D, i, i])
    assert B.EXPORTS[ENTRY] == (i, [D, i, vp, ctypes.POINTER(vp), i, i, vp, ctypes.c_size_t, vp])
    assert B.EXPORTS[ENTRY + "_instance"] == (i, [D, i, i, i, ctypes.c_char_p, ctypes.c_size_t])
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    from vptq_amd import ops
    import sys
    assert callable(ops.quant_gemm_k256_grouped) and "quant_gemm_k256_grouped" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    # the header documents the entry beside the gather group's, with its alignment rule, error codes and the bit contract
    assert hdr.index("vptq_quant_gemm_gather_grouped_instance(") < hdr.index(f"VPTQ_API int {ENTRY}_supported") < hdr.index("VPTQ_API int vptq_dequant(")
    doc = hdr[hdr.index("Batched decode of SIBLING layers of the CANONICAL format"):hdr.index(f"VPTQ_API int {ENTRY}_supported")]
    for word in ("Alignment:", "VPTQ_E_NULL", "VPTQ_E_TOKENS", "VPTQ_E_UNSUPPORTED", "VPTQ_E_WORKSPACE", "VPTQ_E_ALIGN", "BIT-IDENTICAL", "perms=K",
                 "VPTQ_GEMV_EXACT", "vptq_quant_gemm_k256w", "reference's roundings only", "VPTQ_GEMV_OUT_F32", "passes="):
        assert word in doc, word


def _member_ok(d):
    """the member rule, from the descriptor's fields: the canonical format with scale and bias, group_size = in_features a multiple of 8,
    with a permutation its scale and bias in column order"""
    return ((d.vector_len, d.num_centroids, d.num_res_centroids, d.num_codebooks) == (8, 256, 256, 1) and bool(d.weight_scale) and bool(d.weight_bias) and
            d.group_size == d.in_features and d.group_size % 8 == 0 and (not d.perm or (bool(d.scale_permuted) and bool(d.bias_permuted))))


def test_supported_is_the_member_rule_and_the_same_dtype_and_width_rule():
    lib = B.lib()
    sup = getattr(lib, ENTRY + "_supported")
    members = [desc(O=O, k=k, kr=kr, dtype=dt, perm=p, I=I)
               for (k, kr), dt, p, (I, O) in itertools.product(((256, 256), (65536, 256), (65536, 0), (256, 0)), (0, 1), (False, True),
                                                               ((4096, 4096), (4096, 1024), (8192, 1024)))]
    members += [desc(perm=True, perm_sb=False), desc(norm=False), desc(I=4100), desc(I=4100, dtype=1)]
    served = 0
    for a, b in itertools.product(members, members):
        for tokens in (0, 1, 16, 17, 48, 49):
            want = int(1 <= tokens <= 48 and _member_ok(a) and _member_ok(b) and a.dtype == b.dtype and a.group_size == b.group_size)
            assert sup(arr(a, b), 2, tokens) == want, (a.out_features, b.out_features, a.num_centroids, b.num_centroids, tokens)
            # the members are layers the single entries serve at their own token counts
            if want:
                assert all(lib.vptq_quant_gemm_k256w_supported(m, 17) == 1 and lib.vptq_quant_gemv_kernel_name(m, 16, B.GEMV_EXACT) == b"gemm_k256_kernel"
                           for m in (a, b))
            served += want
    assert served > 0
    # n = -1 .. 5; a third member that breaks the rule
    q, k, v = desc(O=4096), desc(O=1024, perm=True), desc(O=1024)
    for n, want in ((-1, 0), (0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 0)):
        assert sup(arr(q, k, v, q, k), n, 5) == want, n
    for bad in (desc(dtype=1), desc(k=65536), desc(kr=0), desc(I=8192), desc(I=4100), desc(norm=False), desc(perm=True, perm_sb=False)):
        assert sup(arr(q, k, bad), 3, 5) == 0 and sup(arr(bad, q), 2, 5) == 0
        assert sup(arr(q, k, bad), 2, 5) == 1                        # (only descs[0 .. n) are read)
    assert sup(None, 2, 5) == 0 and getattr(lib, ENTRY + "_workspace_bytes")(None, 2, 5) == 0


def test_workspace_is_one_block_per_distinct_perm_pointer():
    q = getattr(B.lib(), ENTRY + "_workspace_bytes")
    P1, P2, P3 = 6 << 20, 6 << 20 | 4096, 6 << 20 | 8192
    for I, tokens in itertools.product((8, 64, TILE + 8, 2 * TILE + 264, 4096), (1, 5, 16, 17, 33, 48)):
        block = (tokens * I * 2 + 255) // 256 * 256
        mk = lambda O, ptr: with_perm(desc(I=I, O=O), ptr) if ptr else desc(I=I, O=O)
        cases = (((0, 0), 0), ((0, 0, 0, 0), 0),                                 # no permutation: no workspace
                 ((P1, P1), 1), ((P1, P1, P1), 1), ((P1, 0), 1), ((0, P1, 0, P1), 1),   # one distinct pointer, the mixed case included
                 ((P1, P2), 2), ((P1, P2, P1), 2), ((0, P2, P1, P2), 2),
                 ((P1, P2, P3), 3), ((P3, 0, P2, P1), 3), ((P1, P2, P3, P2), 3))
        for ptrs, k in cases:
            ds = arr(*[mk(O, p) for O, p in zip((72, 24, 36, 8), ptrs)])
            assert q(ds, len(ptrs), tokens) == k * block, (I, tokens, ptrs)
        assert q(arr(mk(72, P1), mk(24, P2)), 2, 49) == 0 and q(arr(mk(72, P1), mk(24, P2)), 1, 5) == 0     # not served: 0
    assert q(arr(with_perm(desc(I=8, O=8), P1), desc(I=8, O=8)), 2, 1) == 256


def test_validation_returns_before_a_launch_in_the_stated_order():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error): NULL, tokens, n and
    unsupported, a NULL y[m], x alignment, then the workspace's size, then its alignment"""
    lib = B.lib()
    call, err = getattr(lib, ENTRY), lib.vptq_last_error
    P1, P2 = 6 << 20, 6 << 20 | 4096
    good = arr(with_perm(desc(O=4096), P1), with_perm(desc(O=1024), P2), desc(O=1024))
    bad = arr(desc(O=4096), desc(O=1024, dtype=1), desc(O=1024))
    need = getattr(lib, ENTRY + "_workspace_bytes")(good, 3, 48)
    assert need == 2 * 48 * 4096 * 2
    assert call(None, 3, X, ys(3), 5, 0, WS, need, None) == B.E_NULL and call(good, 3, None, ys(3), 5, 0, WS, need, None) == B.E_NULL
    assert call(good, 3, X, None, 5, 0, WS, need, None) == B.E_NULL and b"NULL" in err()
    for tokens in (0, 49, 64, -3):
        assert call(good, 3, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS and b"[1, 48]" in err()
        assert call(bad, 3, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS       # tokens before unsupported
        assert call(good, 7, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS      # ... before n
        assert call(good, 3, X + 2, ys(3), tokens, 0, None, 0, None) == B.E_TOKENS   # ... before alignment and workspace
    for n in (-1, 0, 1, 5):
        assert call(good, n, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"2 - 4 members" in err()
    assert call(bad, 3, X + 2, ys(3), 5, 0, None, 0, None) == B.E_UNSUPPORTED and b"member 1: another dtype" in err()
    assert call(arr(desc(), desc(I=8192), desc(k=65536)), 3, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another group_size" in err()
    assert call(arr(desc(), desc(), desc(k=65536)), 3, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 2: not a layer of the canonical format" in err()
    assert b"gemm_k256_grouped (n = 3)" in err()
    holes = ys(3)
    holes[1] = None
    assert call(good, 3, X, holes, 5, 0, WS, need, None) == B.E_NULL and b"y[1]" in err()
    for off in (2, 4, 8):   # x that is not 16-byte aligned: the gather group's code, before the workspace is looked at
        assert call(good, 3, X + off, ys(3), 16, 0, None, 0, None) == B.E_UNSUPPORTED and b"16-byte" in err()
    for tokens in (1, 5, 16, 17, 48):
        need = getattr(lib, ENTRY + "_workspace_bytes")(good, 3, tokens)
        assert need == 2 * ((tokens * 4096 * 2 + 255) // 256 * 256)
        assert call(good, 3, X, ys(3), tokens, 0, None, need, None) == B.E_WORKSPACE and call(good, 3, X, ys(3), tokens, 0, None, 0, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), tokens, 0, WS, need - 1, None) == B.E_WORKSPACE and b"workspace" in err()
        assert call(good, 3, X, ys(3), tokens, 0, WS + 8, need - 1, None) == B.E_WORKSPACE       # size before alignment
        assert call(good, 3, X, ys(3), tokens, 0, WS, need // 2, None) == B.E_WORKSPACE           # one block is not enough for two permutations
        for off in (1, 2, 4, 8):   # the exact size is accepted: the NEXT check answers
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need, None) == B.E_ALIGN and b"16-byte" in err()
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need + 4096, None) == B.E_ALIGN
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(good, 3, X + 8, ys(3), 49, flags, WS, 1 << 20, None) == B.E_TOKENS and call(good, 3, X, ys(3), 5, flags, WS, 8, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), 5, flags, WS + 4, 1 << 20, None) == B.E_ALIGN


def _cus():
    """the CU count the library reports, read off single layers' lines (vptq_quant_gemm_k256w_instance: grid = min(row groups, CUs),
    rgs = ceil(row groups / grid)): the most row groups that still run one per workgroup.  Without a device the library takes 256."""
    def rgs(groups):
        buf = ctypes.create_string_buffer(256)
        assert B.lib().vptq_quant_gemm_k256w_instance(desc(I=8, O=32 * groups), 17, 0, buf, len(buf)) == 0
        return int(re.search(r"rgs=(\d+)", buf.value.decode()).group(1))
    lo, hi = 1, 1 << 14
    assert rgs(lo) == 1 and rgs(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if rgs(mid) == 1 else (lo, mid)
    if not torch.cuda.is_available():
        assert lo == CUS
    return lo


def want_line(ds, tokens, cus):
    """the line from the launch-shape arithmetic, written out per workgroup: workgroup w owns the global row groups w, w + grid, ...;
    inside a member its row groups run as passes of 4, 2, 1 (tb = 1) or one by one (tb > 1).  -> (line, per-workgroup [(member, passes)])"""
    groups = [(d.num_indices + ROWS - 1) // ROWS for d in ds]
    first = [sum(groups[:m]) for m in range(len(ds) + 1)]
    grid, tb = min(first[-1], cus), (tokens + 15) // 16
    rgs, seen, per_wg = 0, set(), []
    for w in range(grid):
        mine = []
        for m in range(len(ds)):
            left = sum(1 for g in range(w, first[-1], grid) if first[m] <= g < first[m + 1])
            if left:
                ps = (1,) * left if tb > 1 else (4,) * (left // 4) + (2,) * (left % 4 // 2) + (1,) * (left % 2)
                seen |= set(ps)
                mine.append((m, ps))
        rgs = max(rgs, len(range(w, first[-1], grid)))
        per_wg.append(tuple(mine))
    k = len({d.perm for d in ds if d.perm})
    G = ds[0].group_size
    head = "none" if k == 0 else \
        f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK} perms={k}"
    passes = f"1x{tb}" if tb > 1 else "+".join(str(p) for p in (4, 2, 1) if p in seen)
    return (f"{head} | gemm_k256_grouped dt={'f16' if ds[0].dtype == 0 else 'bf16'} tok={tokens} tb={tb} n={len(ds)} "
            f"groups={'+'.join(map(str, groups))} grid={grid} rgs={rgs} passes={passes}"), per_wg


def test_instance_line_from_the_cu_count_the_library_reports():
    P1, P2 = 6 << 20, 6 << 20 | 4096
    cus = _cus()
    # q / k / v of the 8B shapes with one shared permutation: 128 + 32 + 32 row groups, one per workgroup
    qkv = [with_perm(desc(O=O), P1) for O in (4096, 1024, 1024)]
    if cus == 256:
        assert line(qkv, 5) == (0, "permute_x_tokens g=4096 tok=5 grid=8x2 tpt=4 perms=1 | gemm_k256_grouped dt=f16 tok=5 tb=1 n=3 groups=128+32+32 grid=192 rgs=1 passes=1")
        assert line([desc(O=14336, dtype=1)] * 2, 17) == (0, "none | gemm_k256_grouped dt=bf16 tok=17 tb=2 n=2 groups=448+448 grid=256 rgs=4 passes=1x2")
        assert line([desc(O=14336)] * 2, 16)[1].endswith("groups=448+448 grid=256 rgs=4 passes=2+1")   # (workgroups 0 .. 127: 2 | 2; 128 .. 191: 2 | 1; 192 .. 255: 1 | 2 - passes are per member)
    qkv[2].perm = P2
    assert line(qkv, 33)[1].startswith("permute_x_tokens g=4096 tok=33 grid=8x9 tpt=4 perms=2 | gemm_k256_grouped dt=f16 tok=33 tb=3 n=3 ")
    # a group whose workgroups run passes 4, 2 and 1, with a member no workgroup visits twice: 4 CUs + 2, 3 and 2 CUs + 1 row groups
    sw = [desc(I=64, O=4 * 32 * cus + 40), desc(I=64, O=72, dtype=0), desc(I=64, O=2 * 32 * cus + 8)]
    text, per_wg = want_line(sw, 15, cus)
    assert per_wg[0] == ((0, (4, 1)), (2, (2,))) and per_wg[2] == ((0, (4,)), (1, (1,)), (2, (2,))) and per_wg[5] == ((0, (4,)), (2, (2, 1)))
    assert all(ps == (1,) for w in per_wg for m, ps in w if m == 1)                    # member 1: at most one row group per workgroup
    assert text.endswith(f"groups={4 * cus + 2}+3+{2 * cus + 1} grid={cus} rgs=7 passes=4+2+1") and line(sw, 15) == (0, text)
    assert line(sw, 40) == (0, want_line(sw, 40, cus)[0]) and line(sw, 40)[1].endswith("rgs=7 passes=1x3")
    # ragged shapes: a partial last row group per member, a last column tile of 264 columns, four members, a mixed group
    rag = [desc(I=2 * TILE + 264, O=O) for O in (72, 24, 36, 8)]
    with_perm(rag[1], P1)
    assert line(rag, 15) == (0, "permute_x_tokens g=2312 tok=15 grid=5x4 tpt=4 perms=1 | gemm_k256_grouped dt=f16 tok=15 tb=1 n=4 groups=3+1+2+1 grid=7 rgs=1 passes=1")
    # the general form
    for outs, I, dt, tokens in itertools.product(((4096, 1024, 1024), (72, 24), (32 * 700, 32 * 300 + 4, 32 * 100), (32 * cus * 7, 8), (32 * (cus * 6 + 1), 40, 32 * cus)),
                                                 (64, TILE + 8), (0, 1), (1, 5, 16, 17, 32, 48)):
        ds = [desc(I=I, O=O, dtype=dt) for O in outs]
        want = want_line(ds, tokens, cus)[0]
        assert line(ds, tokens) == (0, want)
        for flags in (B.GEMV_FAST_MATH, B.GEMV_EXACT, B.GEMV_OUT_F32):
            assert line(ds, tokens, flags) == (0, want)
    # the call's own errors, a buffer that is too small, NULL
    assert line(qkv, 0)[0] == B.E_TOKENS and line(qkv, 49)[0] == B.E_TOKENS and line(qkv[:1], 5)[0] == B.E_UNSUPPORTED
    assert line([desc(), desc(k=65536)], 5) == (B.E_UNSUPPORTED, "")
    for size in (4, 16, 60, 100):   # (shorter than "none | ", than the permute part, than the whole line)
        assert line(qkv, 5, size=size) == (B.E_WORKSPACE, "")
    small = ctypes.create_string_buffer(16)
    assert getattr(B.lib(), ENTRY + "_instance")(arr(*qkv), 3, 5, 0, None, 0) == B.E_NULL
    assert getattr(B.lib(), ENTRY + "_instance")(None, 3, 5, 0, small, len(small)) == B.E_NULL


def test_route_function_is_pure_follows_its_cells_and_obeys_its_knob(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route = gd.gemm_k256_grouped_route
    assert (gd.GEMM_K256_GROUPED_MIN_TOKENS, gd.GEMM_K256_GROUPED_MAX_TOKENS, gd.GEMM_K256_GROUPED_MIN_ELEMENTS) == (5, 48, 2 << 20)
    assert gd._GEMM_K256_GROUPED_MODE == "auto"
    groups = (((4096, 1024, 1024), 4096), ((8192, 1024, 1024), 8192), ((14336, 14336), 4096), ((28672, 28672), 8192), ((1024, 1024), 4096),
              ((72, 24, 36, 8), 2 * TILE + 264), ((512, 512), 2048), ((11200, 4804, 1600), 64))

    def by_the_cells(cells, outs, I, t, perm):
        n_el = sum((o + 7) // 8 for o in outs) * I
        return perm is not None and any(cp == perm and cn == len(outs) and n_el >= max(lo_el, 2 << 20) and (hi_el is None or n_el <= hi_el) and lo <= t <= hi
                                        for cp, cn, lo_el, hi_el, lo, hi in cells)

    def check(cells):
        for (outs, I), perm in itertools.product(groups, (False, True, None)):
            for t in (-1, 0, 1, 4, 49, 64):
                assert not route(outs, I, t, perm)                              # outside 5 .. 48: never
            on = [t for t in range(5, 49) if route(outs, I, t, perm)]
            assert on == [t for t in range(5, 49) if by_the_cells(cells, outs, I, t, perm)], (outs, I, perm)
            assert gd.gemm_k256_grouped_tokens(outs, I, perm) == tuple(on)
            if sum((o + 7) // 8 for o in outs) * I < 2 << 20:
                assert not on, (outs, I)                                        # nothing under 2 M total index elements

    # the committed table: well-formed, nothing under the floor, one interval of token counts per group, and followed exactly
    for c in gd._GEMM_K256_GROUPED_CELLS:
        assert len(c) == 6 and c[0] in (False, True) and 2 <= c[1] <= 4 and c[2] >= 2 << 20 and (c[3] is None or c[3] >= c[2]) and 5 <= c[4] <= c[5] <= 48
    check(gd._GEMM_K256_GROUPED_CELLS)
    # what the committed table says of the measured groups (profiles/r32): q / k / v with and without a permutation, gate / up with one
    for outs, I in (((4096, 1024, 1024), 4096), ((8192, 1024, 1024), 8192)):
        assert gd.gemm_k256_grouped_tokens(outs, I, True) == gd.gemm_k256_grouped_tokens(outs, I, False) == tuple(range(5, 49))
    for outs, I in (((14336, 14336), 4096), ((28672, 28672), 8192)):
        assert gd.gemm_k256_grouped_tokens(outs, I, True) == tuple(range(5, 49)) and gd.gemm_k256_grouped_tokens(outs, I, False) == ()
    for (outs, I), perm in itertools.product(groups, (False, True)):
        on = gd.gemm_k256_grouped_tokens(outs, I, perm)
        assert list(on) == list(range(on[0], on[-1] + 1)) if on else True
    # a monkeypatched table is followed exactly - the member count, a most size, a cell under the floor and the has_perm column included
    qkv, gu, gu70 = (4096, 1024, 1024), (14336, 14336), (28672, 28672)
    cells = ((True, 3, 3 << 20, 12 << 20, 5, 16), (False, 2, 7 << 20, 20 << 20, 17, 48), (True, 2, 1 << 10, None, 5, 8), (False, 3, 3 << 20, None, 12, 12))
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_CELLS", cells)
    check(cells)
    assert route(qkv, 4096, 5, True) and not route(qkv, 4096, 5, False) and not route(qkv, 4096, 5, None) and not route(qkv, 4096, 17, True)
    # q / k / v routed WITHOUT the 70B gate / up pair, and gate / up of the 8B shapes without that of the 70B shapes: what a least size alone cannot say
    assert route(gu, 4096, 17, False) and not route(gu70, 8192, 17, False) and not route(gu, 4096, 16, False)
    assert route((8192, 1024, 1024), 8192, 9, True) and not route((8192, 1024, 1024), 8192, 9, False)
    assert route(gu70, 8192, 8, True) and not route(gu70, 8192, 9, True)               # (a cell without a most size)
    assert route(gu, 4096, 8, True) and not route((512, 512), 2048, 8, True)           # the floor wins over a smaller cell
    assert not route(qkv, 4100, 5, True) and not route((4096,), 4096, 5, True) and not route(qkv + gu, 4096, 5, True)
    # pure: the same answer twice, nothing but the arguments, the table and the knob is read
    assert [route(qkv, 4096, t, True) for t in range(60)] == [route(qkv, 4096, t, True) for t in range(60)]
    # the knob: 1 - every group of 2 - 4 members from 5 to 48 tokens, whatever its size and permutations; 0 - none
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "1")
    assert all(route((72, 24), 1032, t, p) for t in range(5, 49) for p in (False, True, None))
    assert not route(qkv, 4096, 4, True) and not route(qkv, 4096, 49, True) and not route((72,), 1032, 5, True) and not route(qkv, 4100, 5, True)
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "0")
    assert not any(route(outs, I, t, p) for (outs, I) in groups for t in range(0, 60) for p in (False, True, None))


def test_the_knob_is_read_through_tune_env_only_in_its_module():
    src = open(os.path.join(ROOT, "vptq_amd", "grouped_decode.py")).read()
    assert src.count("VPTQ_GEMM_K256_GROUPED\"") == 1
    assert '_GEMM_K256_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_K256_GROUPED", "auto") or "auto").strip().lower()' in src
    assert "os.environ" not in src and "import torch" not in src and "getenv" not in src        # pure: no device, no tensors
    for f in ("vptq_amd/layers/vqlinear.py", "vptq_amd/ops/quant_gemm.py", "vptq_amd/_backend.py", "vptq_amd/batched_decode.py",
              "vptq_amd/csrc/gemm_k256.hip", "vptq_amd/csrc/abi.hip"):
        assert "VPTQ_GEMM_K256_GROUPED" not in open(os.path.join(ROOT, f)).read(), f


def test_the_record_of_the_group_routes():
    from vptq_amd import grouped_decode as gd
    from vptq_amd.layers import vqlinear as vq
    assert [r.entry for r in gd.GROUPED_DECODE_ROUTES] == ["vptq_quant_gemm_gather_grouped", ENTRY]
    assert [(r.min_tokens, r.max_tokens, r.exact_only, r.off_flags) for r in gd.GROUPED_DECODE_ROUTES] == \
        [(5, 16, False, B.GEMV_FORCE_GENERIC), (5, 48, True, B.GEMV_FORCE_ANY)]
    assert (gd.GROUPED_DECODE_MIN_TOKENS, gd.GROUPED_DECODE_MAX_TOKENS) == (5, 48) == (vq.GROUPED_DECODE_MIN_TOKENS, vq.GROUPED_DECODE_MAX_TOKENS)
    formats = [(8, 65536, 0), (8, 65536, 256), (8, 65536, 65536), (16, 65536, 0), (8, 32768, 0), (8, 256, 256), (8, 256, 0), (8, 4096, 256)]
    owners = {f: [r.entry for r in gd.GROUPED_DECODE_ROUTES if r.owns(*f)] for f in formats}
    assert all(len(o) <= 1 for o in owners.values())                                   # the formats are disjoint
    assert owners[(8, 256, 256)] == [ENTRY] and all(owners[(8, 65536, kr)] == ["vptq_quant_gemm_gather_grouped"] for kr in (0, 256, 65536))
    assert [gd.grouped_decode_route(*f) for f in formats[3:5] + formats[6:]] == [None] * 4
    # every record has its library entry with `_supported` and `_workspace_bytes`, and its op
    from vptq_amd import ops
    for r in gd.GROUPED_DECODE_ROUTES:
        assert all(name in B.EXPORTS for name in (r.entry, r.entry + "_supported", r.entry + "_workspace_bytes")) and callable(getattr(ops, r.entry[5:]))


def test_the_routes_of_before_answer_as_before(monkeypatch):
    """the layers' route table and the gather group's route, for every argument tuple the cpu tests of before ask them with"""
    from vptq_amd import batched_decode as bd, grouped_decode as gd
    assert [r.entry for r in bd.BATCHED_DECODE_ROUTES] == ["vptq_quant_gemm_gather_px", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx",
                                                          "vptq_quant_gemm_k256w", "vptq_quant_gemm_gatherw"]
    assert (bd.BATCHED_DECODE_MIN_TOKENS, bd.BATCHED_DECODE_MAX_TOKENS) == (5, 64)
    assert "grouped" not in open(os.path.join(ROOT, "vptq_amd", "batched_decode.py")).read()
    assert bd._GEMM_K256W_CELLS == ((2 << 20, 17, 48),)
    for (O, I), t in itertools.product(((8192, 8192), (4096, 4096), (14336, 4096), (1024, 4096), (512, 2048), (36, 1032)), range(0, 70)):
        assert bd.gemm_k256w_route(O, I, t) == (17 <= t <= 48 and ((O + 7) // 8) * I >= 2 << 20)
        assert [r.entry for r in bd.batched_decode_routes(8, 256, 256, 1, False, True, True)] == ["vptq_quant_gemm_k256w"]
    # the gather group: its committed cells and its answers (tests/test_gemm_gather_grouped_cpu.py's groups and formats)
    assert gd._GEMM_GATHER_GROUPED_CELLS == ((256, False, 3 << 20, 5, 8),)
    assert (gd.GEMM_GATHER_GROUPED_MIN_TOKENS, gd.GEMM_GATHER_GROUPED_MAX_TOKENS, gd.GEMM_GATHER_GROUPED_MIN_ELEMENTS) == (5, 16, 2 << 20)
    groups = (((4096, 1024, 1024), 4096), ((8192, 1024, 1024), 8192), ((14336, 14336), 4096), ((28672, 28672), 8192), ((1024, 1024), 4096),
              ((36, 12, 20, 4), 2 * TILE + 264), ((512, 512), 2048), ((11200, 4804, 1600), 64))
    formats = [(8, 65536, kr) for kr in (0, 256, 65536)] + [(16, 65536, 0), (8, 32768, 0), (8, 256, 256)]
    for (outs, I), (v, k, kr), perm, t in itertools.product(groups, formats, (False, True, None), range(-1, 50)):
        n_el = sum((o + v - 1) // v for o in outs) * I
        want = (v, k, kr) == (8, 65536, 256) and perm is False and n_el >= 3 << 20 and 5 <= t <= 8
        assert gd.gemm_gather_grouped_route(v, k, kr, outs, I, t, perm) == want
        r = gd.grouped_decode_route(v, k, kr)
        if r is not None and r.entry == "vptq_quant_gemm_gather_grouped":              # ... and through the record
            assert r.route(v, k, kr, outs, I, t, perm) == want
    # the canonical group's knob does not reach the gather group, nor the other way round
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "1")
    assert not gd.gemm_gather_grouped_route(8, 65536, 0, (4096, 1024, 1024), 4096, 9, True)
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "auto")
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    assert not gd.gemm_k256_grouped_route((72, 24), 1032, 9, True)                     # (a group no committed cell holds)
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "0")
    assert not gd.gemm_k256_grouped_route((4096, 1024, 1024), 4096, 9, True)


def test_census_of_the_compile_unit():
    """gemm_k256.hip: the two kernels of before as they were, exactly one more `__global__` with <typename DT, int TB>, no static LDS"""
    csrc = os.path.join(ROOT, "vptq_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_k256.hip")).read()
    assert len(re.findall(r"__global__", src)) == 3
    assert re.search(r"template <typename DT, bool PERM>\s*__global__ __launch_bounds__\(kGThreads\) void gemm_k256_kernel\(const GemmK256Params P\)", src)
    assert re.search(r"template <typename DT, bool PERM, int TB>\s*__global__ __launch_bounds__\(kGThreads\) void gemm_k256w_kernel\(const GemmK256Params P\)", src)
    assert re.search(r"template <typename DT, int TB>\s*__global__ __launch_bounds__\(kGThreads\) void gemm_k256_grouped_kernel\(const GemmK256GroupedParams GP\)", src)
    body = src[src.index("void gemm_k256_grouped_kernel("):src.index("// ---- host side")]
    assert "extern __shared__" in body and not re.search(r"(?<!extern )__shared__", body)      # the dynamic block only: the image's base must stay 0
    assert set(re.findall(r"gemm_k256_pass<DT, false, (\d)>", body)) == {"4", "2", "1"} and "gemm_k256_pass<DT, false, 1, TB>" in body
    assert set(re.findall(r"case (\d): return launch_gg<DT, \1>", src)) == {"1", "2", "3"}
    assert "launch_gg_tb<F16>" in src and "launch_gg_tb<BF16>" in src and "allow_dynamic_lds<gemm_k256_grouped_kernel<DT, TB>>(kGLds)" in src
    assert "atomic" not in src and "asm" not in src and "getenv" not in src
    # the entry: validation before any launch, one permute launch per distinct permutation, then ONE kernel launch over the plain forms
    abi = open(os.path.join(csrc, "abi.hip")).read()
    body = abi[abi.index(f"int {ENTRY}("):abi.index(f"int {ENTRY}_instance(")]
    assert body.index("VPTQ_E_WORKSPACE") < body.index("VPTQ_E_ALIGN") < body.index("launch_permute_x_tokens") < body.index("launch_gemm_k256_grouped")
    assert body.count("launch_gemm_k256_grouped(") == 1 and "G.plain" in body


# ---- SiblingGroup.forward_batched over the canonical route: the host protocol, over stub members and a stubbed launch --------------------

class _Member:
    """what `SiblingGroup.forward_batched` reads of a layer: its static configuration, `_descriptor()`, `_parameters`"""
    _gen = 5000

    def __init__(self, O, perm=None, I=64, dtype=torch.float16, flags=B.GEMV_EXACT):
        self.vector_len, self.num_centroids, self.num_res_centroids, self.enable_residual = 8, 256, 256, True
        self.in_features, self.out_features, self.num_codebooks, self.enable_outlier, self.enable_norm = I, O, 1, False, True
        self.enable_perm, self._parameters = perm is not None, {"perm": perm}
        d = desc(I=I, O=O, dtype=0 if dtype == torch.float16 else 1)
        if perm is not None:
            with_perm(d, (6 << 20) + 4096 * (_Member._gen - 4999))   # every member's own perm pointer
        _Member._gen += 1
        self.cache = types.SimpleNamespace(generation=_Member._gen, desc=d, device=torch.device("cpu"), dtype=dtype, device_index=0, arithmetic_flags=flags)

    def _descriptor(self):
        return self.cache

    def rebuild(self, flags=None):
        _Member._gen += 1
        self.cache.generation = _Member._gen
        if flags is not None:
            self.cache.arithmetic_flags = flags


def _group(monkeypatch, members, mode="1"):
    from vptq_amd import grouped_decode as gd, ops
    from vptq_amd.layers.vqlinear import SiblingGroup
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", mode)
    calls = []

    def launch(x, descs, outs, out_f32=False):
        calls.append((x, [descs[i].perm for i in range(len(outs))], tuple(outs)))
        return [torch.full(x.shape[:-1] + (o,), float(len(calls) * 10 + i)) for i, o in enumerate(outs)]

    def wrong(*a, **kw):
        raise AssertionError("the gather group's launch for a canonical-format group")
    monkeypatch.setattr(ops, "quant_gemm_k256_grouped", launch)
    monkeypatch.setattr(ops, "quant_gemm_gather_grouped", wrong)
    return SiblingGroup(members), calls


def test_forward_batched_leader_followers_and_a_stale_follower(monkeypatch):
    q, k, v = _Member(64), _Member(32), _Member(40)
    g, calls = _group(monkeypatch, [q, k, v])
    assert g._batched_route().entry == ENTRY and g._batched_static() == (8, 256, 256, (64, 32, 40), 64, False)
    for tokens in (5, 16, 17, 48):                      # the whole window of the route, one launch each
        x = torch.zeros(tokens, 64, dtype=torch.float16)
        n = len(calls)
        yq = g.forward_batched(q, x, tokens)
        assert len(calls) == n + 1 and calls[-1][0] is x and calls[-1][2] == (64, 32, 40) and yq.shape == (tokens, 64) and float(yq[0, 0]) == 10.0 * (n + 1)
        yk, yv = g.forward_batched(k, x, tokens), g.forward_batched(v, x, tokens)
        assert len(calls) == n + 1 and float(yk[0, 0]) == 10.0 * (n + 1) + 1 and float(yv[0, 0]) == 10.0 * (n + 1) + 2    # the followers pick their share up
        assert g._bx is None and not g._bout                                               # ... once: nothing is held afterwards
    for tokens in (4, 49, 64):
        assert g.forward_batched(q, torch.zeros(tokens, 64, dtype=torch.float16), tokens) is None
    n = len(calls)
    # a follower is the leader of the next tensor; outputs left unconsumed are stale: a new leader call drops them
    x2 = torch.zeros(24, 64, dtype=torch.float16)
    assert float(g.forward_batched(v, x2, 24)[0, 0]) == 10.0 * (n + 1) + 2 and set(g._bout) == {id(q), id(k)}
    x3 = torch.zeros(24, 64, dtype=torch.float16)
    assert float(g.forward_batched(q, x3, 24)[0, 0]) == 10.0 * (n + 2) and len(calls) == n + 2 and set(g._bout) == {id(k), id(v)}
    assert float(g.forward_batched(k, x2, 24)[0, 0]) == 10.0 * (n + 3) + 1 and len(calls) == n + 3          # k with the OLD tensor: stale, it launches
    # the same member again with the same tensor: it has no share left, so it launches
    assert float(g.forward_batched(k, x2, 24)[0, 0]) == 10.0 * (n + 4) + 1 and len(calls) == n + 4


def test_forward_batched_an_x_rewritten_in_place_and_tensors_without_a_version(monkeypatch):
    from vptq_amd import grouped_decode as gd
    q, k = _Member(64), _Member(32)
    g, calls = _group(monkeypatch, [q, k])
    x = torch.zeros(8, 64, dtype=torch.float16)
    g.forward_batched(q, x, 8)
    x.add_(1)                                            # x rewritten in place between the sibling calls: the follower launches for itself
    assert float(g.forward_batched(k, x, 8)[0, 0]) == 21.0 and len(calls) == 2
    assert float(g.forward_batched(q, x, 8)[0, 0]) == 20.0 and len(calls) == 2       # (and q is now ITS follower)
    with torch.inference_mode():
        xi = torch.zeros(8, 64, dtype=torch.float16)
    assert B.tensor_version(xi) == -1
    assert g.forward_batched(q, xi, 8) is None and g.forward_batched(k, xi, 8) is None and len(calls) == 2      # never shared, never launched
    # an x that is not what the entry takes
    assert g.forward_batched(q, torch.zeros(5, 72, dtype=torch.float16)[:, 8:], 5) is not None     # (made contiguous: aligned again)
    assert g.forward_batched(q, torch.zeros(5 * 64 + 4, dtype=torch.float16)[4:].view(5, 64), 5) is None     # 8 bytes off
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.bfloat16), 5) is None and g.forward_batched(q, torch.zeros(5, 32, dtype=torch.float16), 5) is None
    # the knob at 0, and the committed cells (nothing this small)
    n = len(calls)
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "0")
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.float16), 5) is None and len(calls) == n
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "auto")
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.float16), 5) is None and len(calls) == n
    # the gather group's knob does not reach a canonical-format group
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.float16), 5) is None and len(calls) == n
    # launch flags that force another kernel switch the route off
    from vptq_amd import ops
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "1")
    monkeypatch.setattr(ops, "quant_gemm_flags", lambda: B.GEMV_FORCE_MFMA)
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.float16), 5) is None and len(calls) == n


def test_forward_batched_steps_aside_without_the_reference_roundings_and_for_mixed_groups(monkeypatch):
    x = torch.zeros(5, 64, dtype=torch.float16)
    # a member whose arithmetic is not the reference's roundings (set_arithmetic("folded" / "selective"), or only this member moved)
    for flags in (0, B.GEMV_SELECTIVE):
        q, k = _Member(64), _Member(32, flags=flags)
        g, calls = _group(monkeypatch, [q, k])
        assert g.forward_batched(q, x, 5) is None and g.forward_batched(k, x, 5) is None and not calls and g._bx is None
        assert g._batched_workspace_bytes() is None
        k.rebuild(flags=B.GEMV_EXACT)                     # (set_arithmetic renews the descriptor)
        assert g.forward_batched(q, x, 5) is not None and len(calls) == 1
        q.rebuild(flags=flags)
        x2 = torch.zeros(5, 64, dtype=torch.float16)
        assert g.forward_batched(q, x2, 5) is None and len(calls) == 1
    # mixed dtypes, mixed formats, a compacted member, a group the library does not serve
    a, b = _Member(64), _Member(32, dtype=torch.bfloat16)
    g2, calls2 = _group(monkeypatch, [a, b])
    assert g2.forward_batched(a, x, 5) is None and not calls2
    c, d = _Member(64), _Member(32)
    d.num_centroids = 65536
    g3, calls3 = _group(monkeypatch, [c, d])
    assert g3._batched_route() is None and g3.forward_batched(c, x, 5) is None and not calls3
    e, f = _Member(64), _Member(32)
    g4, calls4 = _group(monkeypatch, [e, f])
    f.__dict__["_compact"] = {}
    assert g4.forward_batched(e, x, 5) is None and not calls4
    h, i = _Member(64), _Member(32)
    i.cache.desc.weight_scale = None                                 # (no scale: the library says no)
    i.cache.desc.weight_bias = None
    g5, calls5 = _group(monkeypatch, [h, i])
    assert g5.forward_batched(h, x, 5) is None and not calls5
    # a capture with too small a workspace: the launch wrapper answers None, nothing is shared
    from vptq_amd import ops
    m, n = _Member(64), _Member(32)
    g6, calls6 = _group(monkeypatch, [m, n])
    monkeypatch.setattr(ops, "quant_gemm_k256_grouped", lambda *a, **kw: None)
    assert g6.forward_batched(m, x, 5) is None and g6.forward_batched(n, x, 5) is None and g6._bx is None


def test_forward_batched_shares_one_perm_pointer_and_sizes_the_workspace(monkeypatch):
    p = torch.randperm(64).to(torch.int16)
    q, k, v, o = _Member(64, perm=p), _Member(32, perm=p.clone()), _Member(40, perm=torch.arange(64).to(torch.int16)), _Member(8)
    g, calls = _group(monkeypatch, [q, k, v, o])
    x = torch.zeros(33, 64, dtype=torch.float16)
    assert g.forward_batched(q, x, 33) is not None
    ptrs = calls[0][1]
    own = [m.cache.desc.perm for m in (q, k, v, o)]
    assert len({own[0], own[1], own[2]}) == 3 and own[3] is None
    assert ptrs[0] == own[0] and ptrs[1] == own[0] and ptrs[2] == own[2] and ptrs[3] is None    # equal tensors: the leader's pointer; others their own
    assert g._batched_static()[5] is None                                                       # (a mixed group: some members have a permutation)
    # `prepare_model`'s question: the largest routed token count (48 with the knob on), two distinct permutations
    assert g._batched_workspace_bytes() == (torch.device("cpu"), 0, 2 * 48 * 64 * 2)
    from vptq_amd import grouped_decode as gd
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_CELLS", ((None, 4, 1 << 10, None, 5, 24),))       # (no cell routes a mixed group)
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "auto")
    assert g._batched_workspace_bytes() is None
