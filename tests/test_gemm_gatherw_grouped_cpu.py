"""Host side of vptq_quant_gemm_gatherw_grouped (gemm_gatherw_grouped.hip; added within ABI 12), without a GPU: the four symbols and the
op, the `_supported` truth table held to the member query and the same-dtype / width / T rule, the workspace formula over 0 - 3
distinct perm pointers, the entry's validation in its documented order (every error returns before a launch, fake pointers), the
instance line, the census of the compile unit, the pure route function of vptq_amd/grouped_decode.py with its cells and knob, the
route records (the first-window records as they were, the wide record behind them) and `SiblingGroup.forward_batched`'s host
protocol over stub members and stubbed launches."""
import ctypes
import itertools
import os
import re

import torch

from vptq_amd import _backend as B
from test_gemm_gatherw_cpu import desc, TILE, ROWS, CUS, WG_PER_CU, X, KRS
from test_gemm_gather_grouped_cpu import arr, ys, with_perm, WS, _Member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "vptq_quant_gemm_gatherw_grouped"
SYMBOLS = (ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY, ENTRY + "_instance")
T_OF = {0: 16, 256: 24, 65536: 32}


def line(ds, tokens, flags=0, size=256):
    buf = ctypes.create_string_buffer(size)
    rc = B.lib().vptq_quant_gemm_gatherw_grouped_instance(arr(*ds), len(ds), tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
        assert B.EXPORTS[s] == B.EXPORTS[s.replace("gatherw_grouped", "gather_grouped")]       # the namesakes' signatures
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    from vptq_amd import ops
    import sys
    assert callable(ops.quant_gemm_gatherw_grouped) and "quant_gemm_gatherw_grouped" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    doc = hdr[hdr.index("Batched decode of SIBLING layers of the large-codebook formats for 17 - 48"):hdr.index("VPTQ_API int " + SYMBOLS[0])]
    for word in ("Alignment:", "VPTQ_E_NULL", "VPTQ_E_TOKENS", "VPTQ_E_UNSUPPORTED", "VPTQ_E_WORKSPACE", "VPTQ_E_ALIGN", "BIT-IDENTICAL", "perms=K",
                 "tb=2|3", "[17, 48]"):
        assert word in doc, word


def test_supported_is_the_member_query_and_the_same_dtype_width_and_t_rule():
    lib = B.lib()
    sup, one = lib.vptq_quant_gemm_gatherw_grouped_supported, lib.vptq_quant_gemm_gatherw_supported
    members = [desc(O=O, v=v, k=k, kr=kr, dtype=dt, perm=p, I=I)
               for (v, k, kr), dt, p, (I, O) in itertools.product([(8, 65536, kr) for kr in KRS] + [(16, 65536, 0), (8, 256, 256)], (0, 1),
                                                                  (False, True), ((4096, 4096), (4096, 1024), (8192, 1024)))]
    served = 0
    for a, b in itertools.product(members, members):
        for tokens in (16, 17, 32, 33, 48, 49):
            want = int(17 <= tokens <= 48 and all(one(m, tokens) for m in (a, b)) and a.dtype == b.dtype and a.group_size == b.group_size and
                       a.num_res_centroids == b.num_res_centroids)
            assert sup(arr(a, b), 2, tokens) == want, (a.out_features, b.out_features, tokens)
            served += want
    assert served > 0
    q, k, v = desc(O=4096), desc(O=1024, perm=True), desc(O=1024)
    for n, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 0), (-1, 0)):
        assert sup(arr(q, k, v, q, k), n, 17) == want, n
    # mixed dtype, kr, group_size; members gemm_gatherw does not serve (k = 256; v = 16; no scale; a width that is no multiple of 8)
    for bad in (desc(dtype=1), desc(kr=0), desc(kr=65536), desc(I=8192), desc(I=4100), desc(norm=False), desc(perm=True, perm_sb=False), desc(v=16),
                desc(k=256)):
        for tokens in (17, 32, 48):
            assert sup(arr(q, k, bad), 3, tokens) == 0 and sup(arr(bad, q), 2, tokens) == 0
            assert sup(arr(q, k, bad), 2, tokens) == 1                        # (only descs[0 .. n) are read)
    assert sup(None, 2, 17) == 0 and lib.vptq_quant_gemm_gatherw_grouped_workspace_bytes(None, 2, 17) == 0


def test_workspace_is_one_block_per_distinct_perm_pointer():
    q = B.lib().vptq_quant_gemm_gatherw_grouped_workspace_bytes
    P1, P2, P3 = 6 << 20, 6 << 20 | 4096, 6 << 20 | 8192
    for I, tokens in itertools.product((8, 64, TILE + 8, 2 * TILE + 264, 4096), (17, 32, 33, 48)):
        block = (tokens * I * 2 + 255) // 256 * 256
        mk = lambda O, ptr: with_perm(desc(I=I, O=O), ptr) if ptr else desc(I=I, O=O)
        cases = (((0, 0), 0), ((0, 0, 0, 0), 0),                                 # no permutation: no workspace
                 ((P1, P1), 1), ((P1, P1, P1), 1), ((P1, 0), 1), ((0, P1, 0, P1), 1),   # shared, and the mixed case
                 ((P1, P2), 2), ((P1, P2, P1), 2), ((0, P2, P1, P2), 2),               # distinct
                 ((P1, P2, P3), 3), ((P3, 0, P2, P1), 3), ((P1, P2, P3, P2), 3))
        for ptrs, k in cases:
            ds = arr(*[mk(O, p) for O, p in zip((36, 12, 20, 4), ptrs)])
            assert q(ds, len(ptrs), tokens) == k * block, (I, tokens, ptrs)
        for bad_tokens in (16, 49):
            assert q(arr(mk(36, P1), mk(12, P2)), 2, bad_tokens) == 0            # not served: 0
        assert q(arr(mk(36, P1), mk(12, P2)), 1, tokens) == 0 and q(arr(mk(36, P1), mk(12, P2), mk(12, P2), mk(12, P2), mk(12, P2)), 5, tokens) == 0
    assert q(arr(with_perm(desc(I=8, O=8), P1), desc(I=8, O=8)), 2, 17) == 512     # 17 x 8 x 2 = 272 bytes, rounded up to 256s


def test_validation_returns_before_a_launch_in_the_stated_order():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error): NULL, tokens, n and
    unsupported, NULL y[m], x alignment (the single entry's code at 17+ tokens), then the workspace's size, then its alignment"""
    lib = B.lib()
    call, err = lib.vptq_quant_gemm_gatherw_grouped, lib.vptq_last_error
    P1, P2 = 6 << 20, 6 << 20 | 4096
    good = arr(with_perm(desc(O=4096), P1), with_perm(desc(O=1024), P2), desc(O=1024))
    bad = arr(desc(O=4096), desc(O=1024, dtype=1), desc(O=1024))
    need = lib.vptq_quant_gemm_gatherw_grouped_workspace_bytes(good, 3, 48)
    assert need == 2 * 48 * 4096 * 2
    assert call(None, 3, X, ys(3), 17, 0, WS, need, None) == B.E_NULL and call(good, 3, None, ys(3), 17, 0, WS, need, None) == B.E_NULL
    assert call(good, 3, X, None, 17, 0, WS, need, None) == B.E_NULL and b"NULL" in err()
    for tokens in (0, 1, 16, 49, 64, -3):
        assert call(good, 3, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS and b"[17, 48]" in err()
        assert call(bad, 3, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS       # tokens before unsupported
        assert call(good, 7, X, ys(3), tokens, 0, WS, need, None) == B.E_TOKENS      # ... before n
        assert call(good, 3, X + 2, ys(3), tokens, 0, None, 0, None) == B.E_TOKENS   # ... before alignment and workspace
    for n in (-1, 0, 1, 5):
        assert call(good, n, X, ys(3), 17, 0, WS, need, None) == B.E_UNSUPPORTED and b"2 - 4 members" in err()
    assert call(bad, 3, X + 2, ys(3), 17, 0, None, 0, None) == B.E_UNSUPPORTED and b"member 1: another dtype" in err()
    assert call(arr(desc(), desc(I=8192), desc(k=256)), 3, X, ys(3), 17, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another group_size" in err()
    assert call(arr(desc(), desc(), desc(k=256)), 3, X, ys(3), 32, 0, WS, need, None) == B.E_UNSUPPORTED and \
        b"gemm_gatherw_grouped (n = 3): member 2: not a layer vptq_quant_gemm_gatherw serves" in err()
    assert call(arr(desc(v=16), desc()), 2, X, ys(2), 32, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 0: not a layer" in err()
    assert call(arr(desc(kr=0), desc(kr=65536)), 2, X, ys(2), 48, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another residual" in err()
    holes = ys(3)
    holes[1] = None
    assert call(good, 3, X, holes, 17, 0, WS, need, None) == B.E_NULL and b"y[1]" in err()
    assert call(bad, 3, X, holes, 17, 0, WS, need, None) == B.E_UNSUPPORTED         # unsupported before a NULL y[m]
    for off in (2, 4, 8):   # x that is not 16-byte aligned: the single entry's code, before the workspace is looked at
        assert call(good, 3, X + off, ys(3), 48, 0, None, 0, None) == B.E_TOKENS and b"gemm_gatherw_grouped: x must be 16-byte" in err()
        assert call(good, 3, X + off, holes, 48, 0, None, 0, None) == B.E_NULL      # a NULL y[m] before the alignment
        assert lib.vptq_quant_gemm_gatherw(desc(), X + off, ys(1)[0], 48, 0, None) == B.E_TOKENS
    for tokens in (17, 32, 33, 48):
        need = lib.vptq_quant_gemm_gatherw_grouped_workspace_bytes(good, 3, tokens)
        assert need == 2 * ((tokens * 4096 * 2 + 255) // 256 * 256)
        assert call(good, 3, X, ys(3), tokens, 0, None, need, None) == B.E_WORKSPACE and call(good, 3, X, ys(3), tokens, 0, None, 0, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), tokens, 0, WS, need - 1, None) == B.E_WORKSPACE and b"gemm_gatherw_grouped: workspace" in err()
        assert call(good, 3, X, ys(3), tokens, 0, WS + 8, need - 1, None) == B.E_WORKSPACE       # size before alignment
        assert call(good, 3, X, ys(3), tokens, 0, WS, need // 2, None) == B.E_WORKSPACE           # one block is not enough for two permutations
        for off in (1, 2, 4, 8):   # the exact size is accepted: the NEXT check answers
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need, None) == B.E_ALIGN and b"16-byte" in err()
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need + 4096, None) == B.E_ALIGN
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(good, 3, X + 8, ys(3), 16, flags, WS, 1 << 20, None) == B.E_TOKENS and call(good, 3, X, ys(3), 17, flags, WS, 8, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), 17, flags, WS + 4, 1 << 20, None) == B.E_ALIGN


def test_instance_line_against_hand_written_strings():
    P1, P2 = 6 << 20, 6 << 20 | 4096
    slots = CUS * WG_PER_CU
    # q / k / v of the 8B shapes with one shared permutation: 256 + 64 + 64 row groups in one grid
    qkv = [with_perm(desc(O=O), P1) for O in (4096, 1024, 1024)]
    assert line(qkv, 17) == (0, "permute_x_tokens g=4096 tok=17 grid=8x5 tpt=4 perms=1 | gemm_gatherw_grouped dt=f16 t=24 tok=17 tb=2 n=3 groups=256+64+64 tiles=4 grid=384 rgs=1")
    qkv[2].perm = P2
    assert line(qkv, 48)[1].startswith("permute_x_tokens g=4096 tok=48 grid=8x12 tpt=4 perms=2 | gemm_gatherw_grouped dt=f16 t=24 tok=48 tb=3 n=3 ")
    assert line([desc(O=14336, kr=0, dtype=1)] * 2, 32) == (0, "none | gemm_gatherw_grouped dt=bf16 t=16 tok=32 tb=2 n=2 groups=896+896 tiles=4 grid=1024 rgs=2")
    # ragged shapes: an odd last vector-row per member, a last column tile of 264 columns, four members, a mixed group
    rag = [desc(I=2 * TILE + 264, O=O, kr=65536) for O in (4, 12, 20, 36)]
    with_perm(rag[1], P1)
    assert line(rag, 33) == (0, "permute_x_tokens g=2312 tok=33 grid=5x9 tpt=4 perms=1 | gemm_gatherw_grouped dt=f16 t=32 tok=33 tb=3 n=4 groups=1+1+2+3 tiles=3 grid=7 rgs=1")
    # a list longer than 1024 row groups at 256 CUs
    assert line([desc(I=64, O=O) for O in (11200, 4804, 1600)], 40) == \
        (0, "none | gemm_gatherw_grouped dt=f16 t=24 tok=40 tb=3 n=3 groups=700+301+100 tiles=1 grid=1024 rgs=2")
    # the general form, from the launch-shape arithmetic: every T, both dtypes, tb = 2 and 3
    seen = set()
    for outs, I, kr, dt, tokens in itertools.product(((4096, 1024, 1024), (4, 12, 20, 36), (16 * 700, 16 * 300 + 4, 16 * 100)), (64, TILE + 8), KRS, (0, 1),
                                                     (17, 32, 33, 48)):
        ds = [desc(I=I, O=O, kr=kr, dtype=dt) for O in outs]
        groups = [((O + 7) // 8 + ROWS - 1) // ROWS for O in outs]
        grid, tb = min(sum(groups), slots), (tokens + 15) // 16
        want = (f"none | gemm_gatherw_grouped dt={'f16' if dt == 0 else 'bf16'} t={T_OF[kr]} tok={tokens} tb={tb} n={len(outs)} "
                f"groups={'+'.join(map(str, groups))} tiles={(I + TILE - 1) // TILE} grid={grid} rgs={(sum(groups) + grid - 1) // grid}")
        assert line(ds, tokens) == (0, want)
        for flags in (B.GEMV_FAST_MATH, B.GEMV_EXACT, B.GEMV_OUT_F32):
            assert line(ds, tokens, flags) == (0, want)
        seen.add((dt, T_OF[kr], tb))
    assert len(seen) == 12
    # the call's own errors, a buffer that is too small, NULL
    assert line(qkv, 16)[0] == B.E_TOKENS and line(qkv, 49)[0] == B.E_TOKENS and line(qkv[:1], 17)[0] == B.E_UNSUPPORTED
    assert line([desc(), desc(k=256)], 17) == (B.E_UNSUPPORTED, "")
    for size in (4, 16, 60, 100):   # (shorter than "none | ", than the permute part, than the whole line)
        assert line(qkv, 17, size=size) == (B.E_WORKSPACE, "")
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gatherw_grouped_instance(arr(*qkv), 3, 17, 0, None, 0) == B.E_NULL
    assert B.lib().vptq_quant_gemm_gatherw_grouped_instance(None, 3, 17, 0, small, len(small)) == B.E_NULL


def test_census_of_the_compile_unit():
    """gemm_gatherw_grouped.hip: one `__global__` with <typename DT, int T, int TB>, 12 instantiations, gemm_gather_tile.h's phases,
    plain stores; the single kernels' units do not know it"""
    csrc = os.path.join(ROOT, "vptq_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_gatherw_grouped.hip")).read()
    assert len(re.findall(r"__global__", src)) == 1
    assert re.search(r"template <typename DT, int T, int TB>\s*__global__ __launch_bounds__\(kGTThreads, 2\) void gemm_gatherw_grouped_kernel\(", src)
    assert set(re.findall(r"gemm_gatherw_grouped_kernel<DT, T, (\d)>", src)) == {"2", "3"}
    assert set(re.findall(r"launch_gwg_t<DT, (\d+)>", src)) == {"16", "24", "32"}
    assert "launch_gwg_dt<F16>" in src and "launch_gwg_dt<BF16>" in src
    for phase in ("gt_load_a1<false>", "gt_rebuild<DT, RES>", "gt_write_tile(", "gt_epilogue<DT>", "gt_load_sb(", "gt_dcol("):
        assert phase in src, phase
    code = re.sub(r"//[^\n]*", "", src)   # (the comments say "no atomics")
    assert "atomic" not in code and "asm" not in code and "getenv" not in code and "hipFuncSetAttribute" not in code and not re.search(r"^\s*#\s*if", code, re.M)
    assert "kWGMembers = 4" in src and "kWGWgPerCu = 4" in src
    # T = 24: a barrier on either side of the residual table's re-staging at a member switch
    assert re.search(r"__syncthreads\(\);[^\n]*\n\s*rtab\[tid\] = [^\n]*\n\s*__syncthreads\(\);", src[src.index("void gemm_gatherw_grouped_kernel("):])
    # both copies of the row-group body say that a change to one belongs in the other ... and the single kernels' units are as they were
    assert "A change to one copy belongs in the other" in src
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert srcs.count("gemm_gatherw_grouped.hip") == 1 and srcs.count("gemm_gatherw.hip") == 1 and srcs.count("gemm_gather.hip") == 1
    for f in ("gemm_gatherw.hip", "gemm_gather.hip", "gemm_gather_tile.h"):
        assert "gatherw_grouped" not in open(os.path.join(csrc, f)).read(), f
    # the entry: validation before any launch, one permute launch per distinct permutation, then ONE kernel launch over the plain forms
    abi = open(os.path.join(csrc, "abi.hip")).read()
    body = abi[abi.index("int vptq_quant_gemm_gatherw_grouped("):abi.index("int vptq_quant_gemm_gatherw_grouped_instance(")]
    assert body.index("VPTQ_E_WORKSPACE") < body.index("VPTQ_E_ALIGN") < body.index("launch_permute_x_tokens") < body.index("launch_gemm_gatherw_grouped")
    assert body.count("launch_gemm_gatherw_grouped(") == 1 and "G.plain" in body and "grouped_gather_decide(" in body


GROUPS = (((4096, 1024, 1024), 4096), ((8192, 1024, 1024), 8192), ((14336, 14336), 4096), ((28672, 28672), 8192), ((1024, 1024), 4096),
          ((4, 12, 20, 36), 2 * TILE + 264), ((512, 512), 2048), ((11200, 4804, 1600), 64))
FORMATS = [(8, 65536, kr) for kr in KRS] + [(16, 65536, 0), (8, 32768, 0), (8, 256, 256)]


def test_route_function_is_pure_follows_its_cells_and_obeys_its_knob(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route = gd.gemm_gatherw_grouped_route
    assert (gd.GEMM_GATHERW_GROUPED_MIN_TOKENS, gd.GEMM_GATHERW_GROUPED_MAX_TOKENS, gd.GEMM_GATHERW_GROUPED_MIN_ELEMENTS,
            gd.GEMM_GATHERW_GROUPED_MAX_MEMBERS) == (17, 48, 2 << 20, 4)
    assert gd._GEMM_GATHERW_GROUPED_MODE == "auto"

    def by_the_cells(cells, v, k, kr, outs, I, t, perm):
        n_el = sum((o + v - 1) // v for o in outs) * I
        return (v, k) == (8, 65536) and kr in KRS and perm is not None and \
            any((ckr, cp, cn) == (kr, perm, len(outs)) and n_el >= max(lo_el, 2 << 20) and (hi_el is None or n_el <= hi_el) and lo <= t <= hi
                for ckr, cp, cn, lo_el, hi_el, lo, hi in cells)

    def check(cells):
        for (outs, I), (v, k, kr), perm in itertools.product(GROUPS, FORMATS, (False, True, None)):
            for t in (-1, 0, 1, 5, 16, 49, 64):
                assert not route(v, k, kr, outs, I, t, perm)                   # outside 17 .. 48: never
            on = [t for t in range(17, 49) if route(v, k, kr, outs, I, t, perm)]
            assert on == [t for t in range(17, 49) if by_the_cells(cells, v, k, kr, outs, I, t, perm)], (v, k, kr, outs, I, perm)
            assert on == list(range(on[0], on[-1] + 1)) if on else True         # the routed token counts of a group are one interval
            assert gd.gemm_gatherw_grouped_tokens(v, k, kr, outs, I, perm) == tuple(on)
            if (v, k) != (8, 65536) or sum((o + v - 1) // v for o in outs) * I < 2 << 20:
                assert not on, (outs, I)                                        # only the gather formats, nothing under 2 M elements

    # the committed table: well-formed, nothing under the floor, one interval per (kr, perm, members, size range), followed exactly
    cells = gd._GEMM_GATHERW_GROUPED_CELLS
    assert all(len(c) == 7 and c[0] in KRS and c[1] in (False, True) and 2 <= c[2] <= 4 and c[3] >= 2 << 20 and (c[4] is None or c[4] >= c[3]) and
               17 <= c[5] <= c[6] <= 48 for c in cells)
    check(cells)
    # a monkeypatched table is followed exactly - a cell under the floor, the member count and the most-elements column included
    cells = ((256, True, 3, 3 << 20, 10 << 20, 17, 48), (256, False, 2, 7 << 20, None, 24, 40), (0, True, 3, 1 << 10, None, 17, 32),
             (65536, False, 2, 14 << 20, 14 << 20, 33, 33))
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_CELLS", cells)
    check(cells)
    qkv, gu = (4096, 1024, 1024), (14336, 14336)
    assert route(8, 65536, 256, qkv, 4096, 17, True) and not route(8, 65536, 256, qkv, 4096, 17, False) and not route(8, 65536, 256, qkv, 4096, 17, None)
    assert route(8, 65536, 256, gu, 4096, 24, False) and not route(8, 65536, 256, gu, 4096, 23, False) and not route(8, 65536, 256, gu, 4096, 24, True)
    assert not route(8, 65536, 256, (16384, 4096, 4096), 8192, 17, True)                               # above the region's largest group
    assert route(8, 65536, 0, qkv, 4096, 32, True) and not route(8, 65536, 0, (512, 512, 512), 2048, 32, True)     # the floor wins over a smaller cell
    assert route(8, 65536, 65536, gu, 4096, 33, False) and not route(8, 65536, 65536, (28672, 28672), 8192, 33, False)
    assert not route(8, 65536, 256, qkv, 4100, 17, True) and not route(8, 65536, 256, (4096,), 4096, 17, True) and not route(8, 65536, 256, qkv + gu, 4096, 17, True)
    assert [route(8, 65536, 256, qkv, 4096, t, True) for t in range(60)] == [route(8, 65536, 256, qkv, 4096, t, True) for t in range(60)]
    # the knob: 1 - every group of the kernel's format from 17 to 48 tokens, whatever its size and permutations; 0 - none
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    assert all(route(8, 65536, kr, (36, 12), 1032, t, p) for kr in KRS for t in range(17, 49) for p in (False, True, None))
    assert not any(route(v, k, kr, qkv, 4096, t, True) for v, k, kr in FORMATS[3:] for t in range(0, 60))
    assert not route(8, 65536, 256, qkv, 4096, 16, True) and not route(8, 65536, 256, qkv, 4096, 49, True)
    assert not route(8, 65536, 256, qkv + gu, 4096, 17, True) and not route(8, 65536, 256, qkv, 4100, 17, True)
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "0")
    assert not any(route(v, k, kr, outs, I, t, p) for (outs, I) in GROUPS for v, k, kr in FORMATS for t in range(0, 60) for p in (False, True, None))


def test_the_knob_is_read_once_through_tune_env_and_the_group_knobs_do_not_reach_each_other(monkeypatch):
    src = open(os.path.join(ROOT, "vptq_amd", "grouped_decode.py")).read()
    assert src.count("VPTQ_GEMM_GATHERW_GROUPED\"") == 1
    assert '_GEMM_GATHERW_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHERW_GROUPED", "auto") or "auto").strip().lower()' in src
    assert "os.environ" not in src and "import torch" not in src and "getenv" not in src        # pure: no device, no tensors
    for f in ("vptq_amd/layers/vqlinear.py", "vptq_amd/ops/quant_gemm.py", "vptq_amd/_backend.py", "vptq_amd/batched_decode.py",
              "vptq_amd/csrc/gemm_gatherw_grouped.hip", "vptq_amd/csrc/abi.hip"):
        assert "VPTQ_GEMM_GATHERW_GROUPED" not in open(os.path.join(ROOT, f)).read(), f
    from vptq_amd import grouped_decode as gd
    qkv = (4096, 1024, 1024)
    before = [(gd.gemm_gather_grouped_route(8, 65536, kr, qkv, 4096, t, p), gd.gemm_k256_grouped_route(qkv, 4096, t, p))
              for kr in KRS for t in range(0, 60) for p in (False, True, None)]
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    assert before == [(gd.gemm_gather_grouped_route(8, 65536, kr, qkv, 4096, t, p), gd.gemm_k256_grouped_route(qkv, 4096, t, p))
                      for kr in KRS for t in range(0, 60) for p in (False, True, None)]
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "0")
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "1")
    assert not any(gd.gemm_gatherw_grouped_route(8, 65536, kr, qkv, 4096, t, True) for kr in KRS for t in range(0, 60))
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "auto")
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_CELLS", ())
    assert not any(gd.gemm_gatherw_grouped_route(8, 65536, kr, qkv, 4096, t, True) for kr in KRS for t in range(0, 60))


def test_route_records_the_first_window_as_it_was_and_the_wide_record_behind_it():
    from vptq_amd import grouped_decode as gd
    assert [r.entry for r in gd.GROUPED_DECODE_ROUTES] == ["vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_k256_grouped"]
    assert (gd.GROUPED_DECODE_MIN_TOKENS, gd.GROUPED_DECODE_MAX_TOKENS) == (5, 48)
    assert [(r.entry, r.min_tokens, r.max_tokens, r.off_flags, r.exact_only) for r in gd.GROUPED_DECODE_WIDE_ROUTES] == \
        [(ENTRY, 17, 48, B.GEMV_FORCE_GENERIC, False)]
    wide = gd.GROUPED_DECODE_WIDE_ROUTES[0]
    for v, k, kr in FORMATS + [(8, 256, 0), (8, 4096, 4096)]:
        first = gd.grouped_decode_route(v, k, kr)
        gather = (v, k) == (8, 65536) and kr in KRS
        assert first is (gd.GROUPED_DECODE_ROUTES[0] if gather else gd.GROUPED_DECODE_ROUTES[1] if (v, k, kr) == (8, 256, 256) else None)
        assert wide.owns(v, k, kr) == gather
        routes = gd.grouped_decode_routes(v, k, kr)
        assert routes == ((first, wide) if gather else (first,) if first is not None else ())
        windows = [(r.min_tokens, r.max_tokens) for r in routes]
        assert windows == sorted(windows) and all(a[1] < b[0] for a, b in zip(windows, windows[1:]))      # window order, disjoint
    # the record's functions are the module's
    qkv = (4096, 1024, 1024)
    assert wide.route(8, 65536, 256, qkv, 4096, 17, True) == gd.gemm_gatherw_grouped_route(8, 65536, 256, qkv, 4096, 17, True)
    assert wide.tokens(8, 65536, 256, qkv, 4096, True) == gd.gemm_gatherw_grouped_tokens(8, 65536, 256, qkv, 4096, True)
    # the first-window group tables: their constants and committed cells as they were
    assert gd._GEMM_GATHER_GROUPED_CELLS == ((256, False, 3 << 20, 5, 8),)
    assert gd._GEMM_K256_GROUPED_CELLS == ((True, 3, 3 << 20, 10 << 20, 5, 48), (False, 3, 3 << 20, 10 << 20, 5, 48), (True, 2, 14 << 20, 56 << 20, 5, 48))
    for (outs, I), kr, t, p in itertools.product(GROUPS, KRS, range(0, 60), (False, True, None)):
        n_el = sum((o + 7) // 8 for o in outs) * I
        assert gd.gemm_gather_grouped_route(8, 65536, kr, outs, I, t, p) == (kr == 256 and p is False and n_el >= 3 << 20 and 5 <= t <= 8)
        assert gd.gemm_k256_grouped_route(outs, I, t, p) == \
            any(cp == p and cn == len(outs) and lo_el <= n_el <= hi_el and lo <= t <= hi for cp, cn, lo_el, hi_el, lo, hi in gd._GEMM_K256_GROUPED_CELLS)


# ---- SiblingGroup.forward_batched: the host protocol, over stub members and stubbed launches ----------------------------------------

def _group(monkeypatch, members, mode="1", first="1"):
    from vptq_amd import grouped_decode as gd, ops
    from vptq_amd.layers.vqlinear import SiblingGroup
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", mode)
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", first)
    calls, narrow = [], []

    def launcher(log):
        def launch(x, descs, outs, out_f32=False):
            log.append((x, [descs[i].perm for i in range(len(outs))], tuple(outs)))
            return [torch.full(x.shape[:-1] + (o,), float(len(log) * 10 + i)) for i, o in enumerate(outs)]
        return launch

    def wrong(*a, **kw):
        raise AssertionError("the canonical group's launch for a large-codebook group")
    monkeypatch.setattr(ops, "quant_gemm_gatherw_grouped", launcher(calls))
    monkeypatch.setattr(ops, "quant_gemm_gather_grouped", launcher(narrow))
    monkeypatch.setattr(ops, "quant_gemm_k256_grouped", wrong)
    return SiblingGroup(members), calls, narrow


def test_forward_batched_leader_followers_and_a_stale_follower(monkeypatch):
    q, k, v = _Member(32), _Member(16), _Member(16)
    g, calls, narrow = _group(monkeypatch, [q, k, v])
    assert g._batched_route().entry == "vptq_quant_gemm_gather_grouped" and g._batched_static() == (8, 65536, 256, (32, 16, 16), 64, False)
    assert [g._batched_route(t).entry if g._batched_route(t) else None for t in (4, 5, 16, 17, 48, 49)] == \
        [None, "vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gather_grouped", ENTRY, ENTRY, None]
    for tokens in (17, 48):
        x = torch.zeros(tokens, 64, dtype=torch.float16)
        n = len(calls)
        yq = g.forward_batched(q, x, tokens)
        assert len(calls) == n + 1 and calls[-1][0] is x and calls[-1][2] == (32, 16, 16) and yq.shape == (tokens, 32) and float(yq[0, 0]) == 10.0 * (n + 1)
        yk, yv = g.forward_batched(k, x, tokens), g.forward_batched(v, x, tokens)
        assert len(calls) == n + 1 and float(yk[0, 0]) == 10.0 * (n + 1) + 1 and float(yv[0, 0]) == 10.0 * (n + 1) + 2    # the followers pick their share up
        assert g._bx is None and not g._bout and not narrow                                # ... once: nothing is held afterwards
    # 16 tokens still reach the first-window entry, 17 the new one; outside 5 .. 48 nothing
    assert g.forward_batched(q, torch.zeros(16, 64, dtype=torch.float16), 16) is not None and len(narrow) == 1 and len(calls) == 2
    assert g.forward_batched(q, torch.zeros(17, 64, dtype=torch.float16), 17) is not None and len(narrow) == 1 and len(calls) == 3
    for tokens in (4, 49, 64):
        assert g.forward_batched(q, torch.zeros(tokens, 64, dtype=torch.float16), tokens) is None
    n = len(calls)
    # a follower is the leader of the next tensor; outputs left unconsumed are stale: a new leader call drops them
    x2 = torch.zeros(24, 64, dtype=torch.float16)
    assert float(g.forward_batched(v, x2, 24)[0, 0]) == 10.0 * (n + 1) + 2 and set(g._bout) == {id(q), id(k)}
    x3 = torch.zeros(24, 64, dtype=torch.float16)
    assert float(g.forward_batched(q, x3, 24)[0, 0]) == 10.0 * (n + 2) and len(calls) == n + 2 and set(g._bout) == {id(k), id(v)}
    assert float(g.forward_batched(k, x2, 24)[0, 0]) == 10.0 * (n + 3) + 1 and len(calls) == n + 3          # k with the OLD tensor: stale, it launches
    assert float(g.forward_batched(k, x2, 24)[0, 0]) == 10.0 * (n + 4) + 1 and len(calls) == n + 4          # no share left: it launches


def test_forward_batched_an_x_rewritten_in_place_tensors_without_a_version_and_the_knobs(monkeypatch):
    from vptq_amd import grouped_decode as gd, ops
    q, k = _Member(32), _Member(16)
    g, calls, narrow = _group(monkeypatch, [q, k])
    x = torch.zeros(20, 64, dtype=torch.float16)
    g.forward_batched(q, x, 20)
    x.add_(1)                                            # x rewritten in place between the sibling calls: the follower launches for itself
    assert float(g.forward_batched(k, x, 20)[0, 0]) == 21.0 and len(calls) == 2
    assert float(g.forward_batched(q, x, 20)[0, 0]) == 20.0 and len(calls) == 2       # (and q is now ITS follower)
    with torch.inference_mode():
        xi = torch.zeros(20, 64, dtype=torch.float16)
    assert B.tensor_version(xi) == -1
    assert g.forward_batched(q, xi, 20) is None and g.forward_batched(k, xi, 20) is None and len(calls) == 2      # never shared, never launched
    # an x that is not what the entry takes
    assert g.forward_batched(q, torch.zeros(17, 72, dtype=torch.float16)[:, 8:], 17) is not None     # (made contiguous: aligned again)
    assert g.forward_batched(q, torch.zeros(17 * 64 + 4, dtype=torch.float16)[4:].view(17, 64), 17) is None     # 8 bytes off
    assert g.forward_batched(q, torch.zeros(17, 64, dtype=torch.bfloat16), 17) is None and g.forward_batched(q, torch.zeros(17, 32, dtype=torch.float16), 17) is None
    n = len(calls)
    # the knob at 0 and at "auto" (nothing this small is in a cell); the first window's knob does not reach the new window
    for i, mode in enumerate(("0", "auto")):
        monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", mode)
        assert g.forward_batched(q, torch.zeros(17, 64, dtype=torch.float16), 17) is None and len(calls) == n and len(narrow) == i
        assert g.forward_batched(q, torch.zeros(16, 64, dtype=torch.float16), 16) is not None      # ... and the first window is untouched by it
    assert len(narrow) == 2
    # launch flags that force another kernel switch the route off
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    monkeypatch.setattr(ops, "quant_gemm_flags", lambda: B.GEMV_FORCE_GENERIC)
    assert g.forward_batched(q, torch.zeros(17, 64, dtype=torch.float16), 17) is None and len(calls) == n


def test_forward_batched_steps_aside_for_compacted_mixed_and_unserved_groups(monkeypatch):
    from vptq_amd import ops
    q, k = _Member(32), _Member(16)
    g, calls, narrow = _group(monkeypatch, [q, k])
    x = torch.zeros(32, 64, dtype=torch.float16)
    k.__dict__["_compact"] = {}
    assert g.forward_batched(q, x, 32) is None and g.forward_batched(k, x, 32) is None and not calls
    del k.__dict__["_compact"]
    assert g.forward_batched(q, x, 32) is None and not calls         # (remembered for these descriptors ...)
    k.rebuild()                                                       # (... compacting / uncompacting a layer rebuilds its descriptor)
    assert g.forward_batched(q, x, 32) is not None and len(calls) == 1
    # the plan is kept per entry and per set of descriptor generations
    wide, first = g._batched_route(32), g._batched_route()
    assert g._batched_plan(wide) is g._batched_plan(wide) and g._batched_plan() is g._batched_plan(first) and g._batched_plan(wide) is not g._batched_plan(first)
    old = g._batched_plan(wide)
    q.rebuild()
    assert g._batched_plan(wide) is not old
    # a capture with too small a workspace: the launch wrapper answers None, nothing is shared
    monkeypatch.setattr(ops, "quant_gemm_gatherw_grouped", lambda *a, **kw: None)
    x2 = torch.zeros(32, 64, dtype=torch.float16)
    assert g.forward_batched(q, x2, 32) is None and g.forward_batched(k, x2, 32) is None and g._bx is None
    # mixed formats, mixed dtypes, a group the library does not serve
    g2, calls2, _ = _group(monkeypatch, [_Member(32, kr=256), _Member(16, kr=0)])
    assert g2._batched_route(32) is None and g2.forward_batched(g2.members[0], x, 32) is None and not calls2
    a, b = _Member(32), _Member(16)
    b.cache.dtype = torch.bfloat16
    g3, calls3, _ = _group(monkeypatch, [a, b])
    assert g3.forward_batched(a, x, 32) is None and not calls3
    c, d = _Member(32), _Member(16)
    d.cache.desc.weight_scale = None                                 # (no scale: vptq_quant_gemm_gatherw_supported says no)
    d.cache.desc.weight_bias = None
    g4, calls4, _ = _group(monkeypatch, [c, d])
    assert g4.forward_batched(c, x, 32) is None and not calls4
    # a library that lacks the new entry: the 17 - 48 window steps aside, the first window answers as it did
    real = B.lib()

    class Old:
        def __getattr__(self, name):
            if "gatherw_grouped" in name:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(B, "lib", lambda: Old())
    e, f = _Member(32), _Member(16)
    g5, calls5, narrow5 = _group(monkeypatch, [e, f])
    assert g5.forward_batched(e, x, 32) is None and not calls5
    assert g5.forward_batched(e, torch.zeros(8, 64, dtype=torch.float16), 8) is not None and len(narrow5) == 1
    assert g5._batched_workspace_bytes() == (torch.device("cpu"), 0, 0)


def test_forward_batched_shares_one_perm_pointer_and_sizes_the_workspace_over_both_records(monkeypatch):
    from vptq_amd import grouped_decode as gd
    p = torch.randperm(64).to(torch.int16)
    q, k, v, o = _Member(32, perm=p), _Member(16, perm=p.clone()), _Member(16, perm=torch.arange(64).to(torch.int16)), _Member(8)
    g, calls, narrow = _group(monkeypatch, [q, k, v, o])
    x = torch.zeros(33, 64, dtype=torch.float16)
    assert g.forward_batched(q, x, 33) is not None
    ptrs = calls[0][1]
    own = [m.cache.desc.perm for m in (q, k, v, o)]
    assert len({own[0], own[1], own[2]}) == 3 and own[3] is None
    assert ptrs[0] == own[0] and ptrs[1] == own[0] and ptrs[2] == own[2] and ptrs[3] is None    # equal tensors: the leader's pointer; others their own
    assert [m.cache.desc.perm for m in (q, k, v, o)] == own                                     # the members' own descriptors are untouched
    assert g._batched_static()[5] is None                                                       # (a mixed group: some members have a permutation)
    # `prepare_model`'s question: the largest need over both records - two distinct permutations at 48 tokens with both knobs on,
    # at 16 with the first window alone, none with neither
    assert g._batched_workspace_bytes() == (torch.device("cpu"), 0, 2 * 48 * 64 * 2)
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "auto")                               # (no cell routes a mixed group)
    assert g._batched_workspace_bytes() == (torch.device("cpu"), 0, 2 * 16 * 64 * 2)
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "0")
    assert g._batched_workspace_bytes() is None
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    assert g._batched_workspace_bytes() == (torch.device("cpu"), 0, 2 * 48 * 64 * 2)
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_CELLS", ((256, True, 2, 1 << 10, None, 17, 24),))
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "auto")
    assert g._batched_workspace_bytes() is None                                                 # (under the floor, and a mixed group)
