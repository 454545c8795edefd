"""Host side of vptq_quant_gemm_gather_grouped (the grouped kernel of gemm_gather.hip; added within ABI 12), without a GPU: the four
symbols, the `_supported` truth table held cell by cell to the member query and the same-dtype / width / T rule, the workspace formula
over 0 - 3 distinct perm pointers, the entry's validation (every error returns before a launch, fake pointers), the instance line,
the pure route function of vptq_amd/grouped_decode.py with its cells and knob, the layers' routes as they were, the census of the
compile unit, and `SiblingGroup.forward_batched`'s host protocol over stub members and a stubbed launch."""
import ctypes
import itertools
import os
import re
import types

import torch

from vptq_amd import _backend as B
from test_gemm_gatherw_cpu import desc, TILE, ROWS, CUS, WG_PER_CU, X, KRS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gather_grouped_supported", "vptq_quant_gemm_gather_grouped_workspace_bytes", "vptq_quant_gemm_gather_grouped",
           "vptq_quant_gemm_gather_grouped_instance")
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
    rc = B.lib().vptq_quant_gemm_gather_grouped_instance(arr(*ds), len(ds), tokens, flags, buf, len(buf))
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
    assert B.EXPORTS["vptq_quant_gemm_gather_grouped_supported"] == (i, [D, i, i])
    assert B.EXPORTS["vptq_quant_gemm_gather_grouped_workspace_bytes"] == (ctypes.c_size_t, [D, i, i])
    assert B.EXPORTS["vptq_quant_gemm_gather_grouped"] == (i, [D, i, vp, ctypes.POINTER(vp), i, i, vp, ctypes.c_size_t, vp])
    assert B.EXPORTS["vptq_quant_gemm_gather_grouped_instance"] == (i, [D, i, i, i, ctypes.c_char_p, ctypes.c_size_t])
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    from vptq_amd import ops
    import sys
    assert callable(ops.quant_gemm_gather_grouped) and "quant_gemm_gather_grouped" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    # the header documents the entry beside vptq_quant_gemm_gather_px, with its alignment rule and error codes
    assert hdr.index("vptq_quant_gemm_gather_px_instance(") < hdr.index("VPTQ_API int vptq_quant_gemm_gather_grouped_supported") < hdr.index("VPTQ_API int vptq_dequant(")
    doc = hdr[hdr.index("Batched decode of SIBLING layers"):hdr.index("VPTQ_API int vptq_quant_gemm_gather_grouped_supported")]
    for word in ("Alignment:", "VPTQ_E_NULL", "VPTQ_E_TOKENS", "VPTQ_E_UNSUPPORTED", "VPTQ_E_WORKSPACE", "VPTQ_E_ALIGN", "BIT-IDENTICAL", "perms=K"):
        assert word in doc, word


def test_supported_is_the_member_query_and_the_same_dtype_width_and_t_rule():
    lib = B.lib()
    sup, one = lib.vptq_quant_gemm_gather_grouped_supported, lib.vptq_quant_gemm_gather_supported
    members = [desc(O=O, v=v, k=k, kr=kr, dtype=dt, perm=p, I=I)
               for (v, k, kr), dt, p, (I, O) in itertools.product([(8, 65536, kr) for kr in KRS] + [(16, 65536, 0), (8, 256, 256)], (0, 1),
                                                                  (False, True), ((4096, 4096), (4096, 1024), (8192, 1024)))]
    served = 0
    for a, b in itertools.product(members, members):
        for tokens in (0, 1, 16, 17):
            want = int(1 <= tokens <= 16 and all(one(m, tokens) for m in (a, b)) and a.dtype == b.dtype and a.group_size == b.group_size and
                       a.num_res_centroids == b.num_res_centroids)
            assert sup(arr(a, b), 2, tokens) == want, (a.out_features, b.out_features, tokens)
            served += want
    assert served > 0
    # n = 1 .. 5; a third member that breaks the rule; a member the single entry refuses
    q, k, v = desc(O=4096), desc(O=1024, perm=True), desc(O=1024)
    for n, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 0), (-1, 0)):
        assert sup(arr(q, k, v, q, k), n, 5) == want, n
    for bad in (desc(dtype=1), desc(kr=0), desc(kr=65536), desc(I=8192), desc(I=4100), desc(norm=False), desc(perm=True, perm_sb=False), desc(v=16)):
        assert sup(arr(q, k, bad), 3, 5) == 0 and sup(arr(bad, q), 2, 5) == 0
        assert sup(arr(q, k, bad), 2, 5) == 1                        # (only descs[0 .. n) are read)
    assert sup(None, 2, 5) == 0 and lib.vptq_quant_gemm_gather_grouped_workspace_bytes(None, 2, 5) == 0


def test_workspace_is_one_block_per_distinct_perm_pointer():
    q = B.lib().vptq_quant_gemm_gather_grouped_workspace_bytes
    P1, P2, P3 = 6 << 20, 6 << 20 | 4096, 6 << 20 | 8192
    for I, tokens in itertools.product((8, 64, TILE + 8, 2 * TILE + 264, 4096), (1, 5, 15, 16)):
        block = (tokens * I * 2 + 255) // 256 * 256
        mk = lambda O, ptr: with_perm(desc(I=I, O=O), ptr) if ptr else desc(I=I, O=O)
        cases = (((0, 0), 0), ((0, 0, 0, 0), 0),                                 # no permutation: no workspace
                 ((P1, P1), 1), ((P1, P1, P1), 1), ((P1, 0), 1), ((0, P1, 0, P1), 1),   # one distinct pointer, the mixed case included
                 ((P1, P2), 2), ((P1, P2, P1), 2), ((0, P2, P1, P2), 2),
                 ((P1, P2, P3), 3), ((P3, 0, P2, P1), 3), ((P1, P2, P3, P2), 3))
        for ptrs, k in cases:
            ds = arr(*[mk(O, p) for O, p in zip((36, 12, 20, 4), ptrs)])
            assert q(ds, len(ptrs), tokens) == k * block, (I, tokens, ptrs)
        assert q(arr(mk(36, P1), mk(12, P2)), 2, 17) == 0 and q(arr(mk(36, P1), mk(12, P2)), 1, 5) == 0     # not served: 0
    assert q(arr(with_perm(desc(I=8, O=8), P1), desc(I=8, O=8)), 2, 1) == 256


def test_validation_returns_before_a_launch_in_the_stated_order():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error): NULL, tokens, n and
    unsupported, x alignment, then the workspace's size, then its alignment"""
    lib = B.lib()
    call, err = lib.vptq_quant_gemm_gather_grouped, lib.vptq_last_error
    P1, P2 = 6 << 20, 6 << 20 | 4096
    good = arr(with_perm(desc(O=4096), P1), with_perm(desc(O=1024), P2), desc(O=1024))
    bad = arr(desc(O=4096), desc(O=1024, dtype=1), desc(O=1024))
    need = lib.vptq_quant_gemm_gather_grouped_workspace_bytes(good, 3, 16)
    assert need == 2 * 16 * 4096 * 2
    assert call(None, 3, X, ys(3), 5, 0, WS, need, None) == B.E_NULL and call(good, 3, None, ys(3), 5, 0, WS, need, None) == B.E_NULL
    assert call(good, 3, X, None, 5, 0, WS, need, None) == B.E_NULL and b"NULL" in err()
    for tokens in (0, 17, 48, -3):
        assert call(good, 3, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS and b"[1, 16]" in err()
        assert call(bad, 3, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS       # tokens before unsupported
        assert call(good, 7, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS      # ... before n
        assert call(good, 3, X + 2, ys(3), tokens, 0, None, 0, None) == B.E_TOKENS   # ... before alignment and workspace
    for n in (-1, 0, 1, 5):
        assert call(good, n, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"2 - 4 members" in err()
    assert call(bad, 3, X + 2, ys(3), 5, 0, None, 0, None) == B.E_UNSUPPORTED and b"member 1: another dtype" in err()
    assert call(arr(desc(), desc(I=8192), desc(k=256)), 3, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1" in err()
    assert call(arr(desc(), desc(), desc(k=256)), 3, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 2: not a layer vptq_quant_gemm_gather serves" in err()
    assert call(arr(desc(kr=0), desc(kr=65536)), 2, X, ys(2), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"residual" in err()
    holes = ys(3)
    holes[1] = None
    assert call(good, 3, X, holes, 5, 0, WS, need, None) == B.E_NULL and b"y[1]" in err()
    for off in (2, 4, 8):   # x that is not 16-byte aligned: the single entry's code, before the workspace is looked at
        assert call(good, 3, X + off, ys(3), 16, 0, None, 0, None) == B.E_UNSUPPORTED and b"16-byte" in err()
    for tokens in (1, 5, 16):
        need = lib.vptq_quant_gemm_gather_grouped_workspace_bytes(good, 3, tokens)
        assert need == 2 * ((tokens * 4096 * 2 + 255) // 256 * 256)
        assert call(good, 3, X, ys(3), tokens, 0, None, need, None) == B.E_WORKSPACE and call(good, 3, X, ys(3), tokens, 0, None, 0, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), tokens, 0, WS, need - 1, None) == B.E_WORKSPACE and b"workspace" in err()
        assert call(good, 3, X, ys(3), tokens, 0, WS + 8, need - 1, None) == B.E_WORKSPACE       # size before alignment
        assert call(good, 3, X, ys(3), tokens, 0, WS, need // 2, None) == B.E_WORKSPACE           # one block is not enough for two permutations
        for off in (1, 2, 4, 8):   # the exact size is accepted: the NEXT check answers
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need, None) == B.E_ALIGN and b"16-byte" in err()
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need + 4096, None) == B.E_ALIGN
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(good, 3, X + 8, ys(3), 17, flags, WS, 1 << 20, None) == B.E_TOKENS and call(good, 3, X, ys(3), 5, flags, WS, 8, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), 5, flags, WS + 4, 1 << 20, None) == B.E_ALIGN


def test_instance_line_against_hand_written_strings():
    P1, P2 = 6 << 20, 6 << 20 | 4096
    slots = CUS * WG_PER_CU
    # q / k / v of 8B shapes with one shared permutation: 256 + 64 + 64 row groups in one grid
    qkv = [with_perm(desc(O=O), P1) for O in (4096, 1024, 1024)]
    assert line(qkv, 5) == (0, "permute_x_tokens g=4096 tok=5 grid=8x2 tpt=4 perms=1 | gemm_gather_grouped dt=f16 t=24 tok=5 n=3 groups=256+64+64 tiles=4 grid=384 rgs=1")
    qkv[2].perm = P2
    assert line(qkv, 16)[1].startswith("permute_x_tokens g=4096 tok=16 grid=8x4 tpt=4 perms=2 | gemm_gather_grouped dt=f16 t=24 tok=16 n=3 ")
    # gate / up without a permutation: 2 x 896 row groups over 1024 workgroups
    assert line([desc(O=14336, kr=0, dtype=1)] * 2, 9) == (0, "none | gemm_gather_grouped dt=bf16 t=16 tok=9 n=2 groups=896+896 tiles=4 grid=1024 rgs=2")
    # ragged shapes: an odd last vector-row per member, a last column tile of 264 columns, four members, a mixed group
    rag = [desc(I=2 * TILE + 264, O=O, kr=65536) for O in (36, 12, 20, 4)]
    with_perm(rag[1], P1)
    assert line(rag, 15) == (0, "permute_x_tokens g=2312 tok=15 grid=5x4 tpt=4 perms=1 | gemm_gather_grouped dt=f16 t=32 tok=15 n=4 groups=3+1+2+1 tiles=3 grid=7 rgs=1")
    assert line([desc(I=8, O=5), desc(I=8, O=16 * slots)], 1) == (0, f"none | gemm_gather_grouped dt=f16 t=24 tok=1 n=2 groups=1+{slots} tiles=1 grid={slots} rgs=2")
    # the general form, from the launch-shape arithmetic
    for outs, I, kr, dt, tokens in itertools.product(((4096, 1024, 1024), (36, 12), (16 * 700, 16 * 300 + 4, 16 * 100)), (64, TILE + 8), KRS, (0, 1), (1, 5, 16)):
        ds = [desc(I=I, O=O, kr=kr, dtype=dt) for O in outs]
        groups = [((O + 7) // 8 + ROWS - 1) // ROWS for O in outs]
        grid = min(sum(groups), slots)
        want = (f"none | gemm_gather_grouped dt={'f16' if dt == 0 else 'bf16'} t={ {0: 16, 256: 24, 65536: 32}[kr]} tok={tokens} n={len(outs)} "
                f"groups={'+'.join(map(str, groups))} tiles={(I + TILE - 1) // TILE} grid={grid} rgs={(sum(groups) + grid - 1) // grid}")
        assert line(ds, tokens) == (0, want)
        for flags in (B.GEMV_FAST_MATH, B.GEMV_EXACT, B.GEMV_OUT_F32):
            assert line(ds, tokens, flags) == (0, want)
    # the call's own errors, a buffer that is too small, NULL
    assert line(qkv, 0)[0] == B.E_TOKENS and line(qkv, 17)[0] == B.E_TOKENS and line(qkv[:1], 5)[0] == B.E_UNSUPPORTED
    assert line([desc(), desc(k=256)], 5) == (B.E_UNSUPPORTED, "")
    for size in (4, 16, 60, 100):   # (shorter than "none | ", than the permute part, than the whole line)
        assert line(qkv, 5, size=size) == (B.E_WORKSPACE, "")
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gather_grouped_instance(arr(*qkv), 3, 5, 0, None, 0) == B.E_NULL
    assert B.lib().vptq_quant_gemm_gather_grouped_instance(None, 3, 5, 0, small, len(small)) == B.E_NULL


def test_route_function_is_pure_follows_its_cells_and_obeys_its_knob(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route = gd.gemm_gather_grouped_route
    assert (gd.GEMM_GATHER_GROUPED_MIN_TOKENS, gd.GEMM_GATHER_GROUPED_MAX_TOKENS, gd.GEMM_GATHER_GROUPED_MIN_ELEMENTS) == (5, 16, 2 << 20)
    assert gd._GEMM_GATHER_GROUPED_MODE == "auto"
    groups = (((4096, 1024, 1024), 4096), ((8192, 1024, 1024), 8192), ((14336, 14336), 4096), ((28672, 28672), 8192), ((1024, 1024), 4096),
              ((36, 12, 20, 4), 2 * TILE + 264), ((512, 512), 2048), ((11200, 4804, 1600), 64))
    formats = [(8, 65536, kr) for kr in KRS] + [(16, 65536, 0), (8, 32768, 0), (8, 256, 256)]

    def by_the_cells(cells, v, k, kr, outs, I, t, perm):
        n_el = sum((o + v - 1) // v for o in outs) * I
        return (v, k) == (8, 65536) and kr in KRS and perm is not None and \
            any((ckr, cp) == (kr, perm) and n_el >= max(e, 2 << 20) and lo <= t <= hi for ckr, cp, e, lo, hi in cells)

    def check(cells):
        for (outs, I), (v, k, kr), perm in itertools.product(groups, formats, (False, True, None)):
            for t in (-1, 0, 1, 4, 17, 48):
                assert not route(v, k, kr, outs, I, t, perm)                   # outside 5 .. 16: never
            on = [t for t in range(5, 17) if route(v, k, kr, outs, I, t, perm)]
            assert on == [t for t in range(5, 17) if by_the_cells(cells, v, k, kr, outs, I, t, perm)], (v, k, kr, outs, I, perm)
            assert on == list(range(on[0], on[-1] + 1)) if on else True         # the routed token counts of a group are one interval
            assert gd.gemm_gather_grouped_tokens(v, k, kr, outs, I, perm) == tuple(on)
            if sum((o + v - 1) // v for o in outs) * I < 2 << 20:
                assert not on, (outs, I)                                        # nothing under 2 M total index elements

    # the committed table: well-formed, nothing under the floor, and followed exactly
    assert all(len(c) == 5 and c[0] in KRS and c[1] in (False, True) and c[2] >= 2 << 20 and 5 <= c[3] <= c[4] <= 16 for c in gd._GEMM_GATHER_GROUPED_CELLS)
    check(gd._GEMM_GATHER_GROUPED_CELLS)
    # a monkeypatched table is followed exactly - a cell under the floor and the has_perm column included
    cells = ((256, True, 3 << 20, 5, 16), (256, False, 7 << 20, 9, 16), (0, True, 1 << 10, 5, 8), (65536, False, 28 << 20, 12, 12))
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_CELLS", cells)
    check(cells)
    qkv, gu = (4096, 1024, 1024), (14336, 14336)
    assert route(8, 65536, 256, qkv, 4096, 5, True) and not route(8, 65536, 256, qkv, 4096, 5, False) and not route(8, 65536, 256, qkv, 4096, 5, None)
    assert route(8, 65536, 256, gu, 4096, 9, False) and not route(8, 65536, 256, gu, 4096, 8, False) and not route(8, 65536, 256, qkv, 4096, 9, False)
    assert route(8, 65536, 0, qkv, 4096, 8, True) and not route(8, 65536, 0, (512, 512), 2048, 8, True)     # the floor wins over a smaller cell
    assert not route(8, 65536, 256, qkv, 4100, 5, True) and not route(8, 65536, 256, (4096,), 4096, 5, True) and not route(8, 65536, 256, qkv + gu, 4096, 5, True)
    # pure: the same answer twice, nothing but the arguments, the table and the knob is read
    assert [route(8, 65536, 256, qkv, 4096, t, True) for t in range(20)] == [route(8, 65536, 256, qkv, 4096, t, True) for t in range(20)]
    # the knob: 1 - every group of the kernel's format from 5 to 16 tokens, whatever its size and permutations; 0 - none
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    assert all(route(8, 65536, kr, (36, 12), 1032, t, p) for kr in KRS for t in range(5, 17) for p in (False, True, None))
    assert not any(route(v, k, kr, qkv, 4096, t, True) for v, k, kr in formats[3:] for t in range(0, 20))
    assert not route(8, 65536, 256, qkv, 4096, 4, True) and not route(8, 65536, 256, qkv, 4096, 17, True)
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "0")
    assert not any(route(v, k, kr, outs, I, t, p) for (outs, I) in groups for v, k, kr in formats for t in range(0, 20) for p in (False, True, None))


def test_the_knob_is_read_through_tune_env_only_in_its_module():
    src = open(os.path.join(ROOT, "vptq_amd", "grouped_decode.py")).read()
    assert src.count("VPTQ_GEMM_GATHER_GROUPED\"") == 1
    assert '_GEMM_GATHER_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHER_GROUPED", "auto") or "auto").strip().lower()' in src
    assert "os.environ" not in src and "import torch" not in src and "getenv" not in src        # pure: no device, no tensors
    for f in ("vptq_amd/layers/vqlinear.py", "vptq_amd/ops/quant_gemm.py", "vptq_amd/_backend.py", "vptq_amd/batched_decode.py",
              "vptq_amd/csrc/gemm_gather.hip", "vptq_amd/csrc/abi.hip"):
        assert "VPTQ_GEMM_GATHER_GROUPED" not in open(os.path.join(ROOT, f)).read(), f


def test_the_layers_routes_answer_as_before():
    """this route is a group's: the layers' route table and cell tables do not know it"""
    from vptq_amd import batched_decode as bd
    assert [r.entry for r in bd.BATCHED_DECODE_ROUTES] == ["vptq_quant_gemm_gather_px", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx",
                                                          "vptq_quant_gemm_k256w", "vptq_quant_gemm_gatherw"]
    assert (bd.BATCHED_DECODE_MIN_TOKENS, bd.BATCHED_DECODE_MAX_TOKENS) == (5, 64)
    assert "grouped" not in open(os.path.join(ROOT, "vptq_amd", "batched_decode.py")).read()
    assert bd._GEMM_GATHER_CELLS == ((8, 65536, 0, 2 << 20, 9), (8, 65536, 256, 2 << 20, 9), (8, 65536, 65536, 2 << 20, 9))
    assert bd._GEMM_GATHERW_CELLS == tuple((kr, el, lo, hi) for kr in KRS for el, lo, hi in ((7 << 20, 17, 24), (28 << 20, 17, 48)))
    assert bd._GEMM_GATHER_PX_CELLS[:2] == ((8, 65536, 0, 7 << 20, 5, 40), (8, 65536, 0, 8 << 20, 5, 48)) and len(bd._GEMM_GATHER_PX_CELLS) == 9
    for (O, I), kr, t in itertools.product(((8192, 8192), (4096, 4096), (14336, 4096), (1024, 4096)), KRS, range(0, 50)):
        n_el = (O // 8) * I
        assert bd.gemm_gather_route(8, 65536, kr, O, I, t) == (9 <= t <= 16 and n_el >= 2 << 20)
        assert bd.gemm_gather_px_route(8, 65536, kr, O, I, t) == \
            any(c[:3] == (8, 65536, kr) and n_el >= max(c[3], 4 << 20) and c[4] <= t <= c[5] for c in bd._GEMM_GATHER_PX_CELLS)
        assert [r.entry for r in bd.batched_decode_routes(8, 65536, kr, 1, False, True, True)] == \
            ["vptq_quant_gemm_gather_px", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherw"]


def test_census_of_the_compile_unit():
    """gemm_gather.hip: the single kernel's template as it was, exactly one more `__global__` with <typename DT, int T>, plain stores"""
    csrc = os.path.join(ROOT, "vptq_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_gather.hip")).read()
    assert re.search(r"template <typename DT, int T, bool PERM>\s*__global__ __launch_bounds__\(kGTThreads\) void gemm_gather_kernel\(const GemmGatherParams P\)", src)
    assert len(re.findall(r"__global__", src)) == 2
    assert re.search(r"template <typename DT, int T>\s*__global__ __launch_bounds__\(kGTThreads\) void gemm_gather_grouped_kernel\(", src)
    assert "atomic" not in src and "asm" not in src and "getenv" not in src and not re.search(r"^\s*#\s*if", src, re.M)
    assert "kGGMembers = 4" in src and "hipFuncSetAttribute" not in src
    assert set(re.findall(r"gemm_gather_grouped_kernel<DT, (\d+)>", src)) == {"16", "24", "32"}
    assert "launch_mgg_dt<F16>" in src and "launch_mgg_dt<BF16>" in src
    # T = 24: a barrier on either side of the residual table's re-staging at a member switch
    assert re.search(r"__syncthreads\(\);[^\n]*\n\s*rtab\[tid\] = [^\n]*\n\s*__syncthreads\(\);", src[src.index("void gemm_gather_grouped_kernel("):])
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert srcs.count("gemm_gather.hip") == 1
    # the entry: validation before any launch, one permute launch per distinct permutation, then ONE kernel launch over the plain forms
    abi = open(os.path.join(csrc, "abi.hip")).read()
    body = abi[abi.index("int vptq_quant_gemm_gather_grouped("):abi.index("int vptq_quant_gemm_gather_grouped_instance(")]
    assert body.index("VPTQ_E_WORKSPACE") < body.index("VPTQ_E_ALIGN") < body.index("launch_permute_x_tokens") < body.index("launch_gemm_gather_grouped")
    assert body.count("launch_gemm_gather_grouped(") == 1 and "G.plain" in body


# ---- SiblingGroup.forward_batched: the host protocol, over stub members and a stubbed launch ----------------------------------------

class _Member:
    """what `SiblingGroup.forward_batched` reads of a layer: its static configuration, `_descriptor()`, `_parameters`"""
    _gen = 1000

    def __init__(self, O, perm=None, kr=256, I=64):
        self.vector_len, self.num_centroids, self.num_res_centroids, self.enable_residual = 8, 65536, kr, kr > 0
        self.in_features, self.out_features, self.num_codebooks, self.enable_outlier, self.enable_norm = I, O, 1, False, True
        self.enable_perm, self._parameters = perm is not None, {"perm": perm}
        d = desc(I=I, O=O, kr=kr)
        if perm is not None:
            with_perm(d, (6 << 20) + 4096 * (_Member._gen - 999))   # every member's own perm pointer
        _Member._gen += 1
        self.cache = types.SimpleNamespace(generation=_Member._gen, desc=d, device=torch.device("cpu"), dtype=torch.float16, device_index=0)

    def _descriptor(self):
        return self.cache

    def rebuild(self):
        _Member._gen += 1
        self.cache.generation = _Member._gen


def _group(monkeypatch, members):
    from vptq_amd import grouped_decode as gd, ops
    from vptq_amd.layers.vqlinear import SiblingGroup
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    calls = []

    def launch(x, descs, outs, out_f32=False):
        calls.append((x, [descs[i].perm for i in range(len(outs))], tuple(outs)))
        return [torch.full(x.shape[:-1] + (o,), float(len(calls) * 10 + i)) for i, o in enumerate(outs)]
    monkeypatch.setattr(ops, "quant_gemm_gather_grouped", launch)
    return SiblingGroup(members), calls


def test_forward_batched_leader_and_followers(monkeypatch):
    q, k, v = _Member(32), _Member(16), _Member(16)
    g, calls = _group(monkeypatch, [q, k, v])
    x = torch.zeros(5, 64, dtype=torch.float16)
    yq = g.forward_batched(q, x, 5)
    assert len(calls) == 1 and calls[0][0] is x and calls[0][2] == (32, 16, 16) and yq.shape == (5, 32) and float(yq[0, 0]) == 10.0
    yk, yv = g.forward_batched(k, x, 5), g.forward_batched(v, x, 5)
    assert len(calls) == 1 and float(yk[0, 0]) == 11.0 and float(yv[0, 0]) == 12.0     # the followers pick their share up
    assert g._bx is None and not g._bout                                               # ... once: nothing is held afterwards
    # a follower is the leader of the next tensor; another order of calls; outputs left unconsumed are stale
    x2 = torch.zeros(5, 64, dtype=torch.float16)
    assert float(g.forward_batched(v, x2, 5)[0, 0]) == 22.0 and float(g.forward_batched(q, x2, 5)[0, 0]) == 20.0 and len(calls) == 2
    x3 = torch.zeros(5, 64, dtype=torch.float16)
    assert float(g.forward_batched(q, x3, 5)[0, 0]) == 30.0 and len(calls) == 3 and set(g._bout) == {id(k), id(v)}
    # the same member again with the same tensor: it has no share left, so it launches
    assert float(g.forward_batched(q, x3, 5)[0, 0]) == 40.0 and len(calls) == 4


def test_forward_batched_version_mismatch_and_tensors_without_a_version(monkeypatch):
    q, k = _Member(32), _Member(16)
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
    # not this group's route: the route function says no (knob 0, a token count outside 5 .. 16), a misaligned or mismatched x
    from vptq_amd import grouped_decode as gd
    assert g.forward_batched(q, torch.zeros(4, 64, dtype=torch.float16), 4) is None and g.forward_batched(q, torch.zeros(17, 64, dtype=torch.float16), 17) is None
    assert g.forward_batched(q, torch.zeros(5, 72, dtype=torch.float16)[:, 8:], 5) is not None     # (made contiguous: aligned again)
    assert g.forward_batched(q, torch.zeros(5 * 64 + 4, dtype=torch.float16)[4:].view(5, 64), 5) is None     # 8 bytes off
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.bfloat16), 5) is None and g.forward_batched(q, torch.zeros(5, 32, dtype=torch.float16), 5) is None
    n = len(calls)
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "0")
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.float16), 5) is None and len(calls) == n
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "auto")      # the committed cells: nothing this small
    assert g.forward_batched(q, torch.zeros(5, 64, dtype=torch.float16), 5) is None and len(calls) == n


def test_forward_batched_steps_aside_for_compacted_mixed_and_unserved_groups(monkeypatch):
    q, k = _Member(32), _Member(16)
    g, calls = _group(monkeypatch, [q, k])
    x = torch.zeros(5, 64, dtype=torch.float16)
    k.__dict__["_compact"] = {}
    assert g.forward_batched(q, x, 5) is None and g.forward_batched(k, x, 5) is None and not calls
    del k.__dict__["_compact"]
    assert g.forward_batched(q, x, 5) is None and not calls         # (remembered for these descriptors ...)
    k.rebuild()                                                      # (... compacting / uncompacting a layer rebuilds its descriptor)
    assert g.forward_batched(q, x, 5) is not None and len(calls) == 1
    # a capture with too small a workspace: the launch wrapper answers None, nothing is shared
    from vptq_amd import ops
    monkeypatch.setattr(ops, "quant_gemm_gather_grouped", lambda *a, **kw: None)
    x2 = torch.zeros(5, 64, dtype=torch.float16)
    assert g.forward_batched(q, x2, 5) is None and g.forward_batched(k, x2, 5) is None and g._bx is None
    # mixed formats, mixed dtypes, a group the library does not serve
    g2, calls2 = _group(monkeypatch, [_Member(32, kr=256), _Member(16, kr=0)])
    assert g2.forward_batched(g2.members[0], x, 5) is None and not calls2
    a, b = _Member(32), _Member(16)
    b.cache.dtype = torch.bfloat16
    g3, calls3 = _group(monkeypatch, [a, b])
    assert g3.forward_batched(a, x, 5) is None and not calls3
    c, d = _Member(32), _Member(16)
    d.cache.desc.weight_scale = None                                 # (no scale: vptq_quant_gemm_gather_supported says no)
    d.cache.desc.weight_bias = None
    g4, calls4 = _group(monkeypatch, [c, d])
    assert g4.forward_batched(c, x, 5) is None and not calls4


def test_forward_batched_shares_one_perm_pointer_among_equal_permutations(monkeypatch):
    p = torch.randperm(64).to(torch.int16)
    q, k, v, o = _Member(32, perm=p), _Member(16, perm=p.clone()), _Member(16, perm=torch.arange(64).to(torch.int16)), _Member(8)
    g, calls = _group(monkeypatch, [q, k, v, o])
    x = torch.zeros(5, 64, dtype=torch.float16)
    assert g.forward_batched(q, x, 5) is not None
    ptrs = calls[0][1]
    own = [m.cache.desc.perm for m in (q, k, v, o)]
    assert len({own[0], own[1], own[2]}) == 3 and own[3] is None
    assert ptrs[0] == own[0] and ptrs[1] == own[0] and ptrs[2] == own[2] and ptrs[3] is None    # equal tensors: the leader's pointer; others their own
    assert [m.cache.desc.perm for m in (q, k, v, o)] == own                                     # the members' own descriptors are untouched
    assert g._batched_static()[5] is None                                                       # (a mixed group: some members have a permutation)
    # decided once per descriptor generation: a rebuilt descriptor is looked at again
    plan = g._batched_plan()
    assert g._batched_plan() is plan
    k._parameters["perm"] = torch.arange(64).flip(0).to(torch.int16)
    k.rebuild()
    x2 = torch.zeros(5, 64, dtype=torch.float16)
    g.forward_batched(q, x2, 5)
    assert calls[-1][1][1] == own[1] and calls[-1][1][0] == own[0]
