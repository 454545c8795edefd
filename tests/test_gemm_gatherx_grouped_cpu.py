"""Host side of vptq_quant_gemm_gatherx_grouped (gemm_gatherx_grouped.hip; added within ABI 12), without a GPU: the four symbols and
the op, the `_supported` truth table held to the member query and the same-dtype / width / format rule, the workspace formula, the
entry's validation in its documented order (every error returns before a launch, fake pointers), the instance line (groups sums,
wgcu per residual size, perms=K), the census of the compile unit, the pure route function of vptq_amd/grouped_decode.py with its cells
and knob, the route records (`GROUPED_DECODE_X_ROUTES` behind `sibling_decode_routes`; the older tables as they were) and
`SiblingGroup.forward_batched`'s host protocol over stub members and a stubbed launch."""
import ctypes
import itertools
import os
import re

import torch

from vptq_amd import _backend as B
from test_gemm_gather_cpu import desc, X, CUS
from test_gemm_gatherx_cpu import fdesc, FORMATS, GATHER_OWNED, TILE, TILE_BYTES, RES_LDS_MAX, LDS_PER_CU, MAX_WG_PER_CU
from test_gemm_gather_grouped_cpu import arr, ys, with_perm, WS, _Member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "vptq_quant_gemm_gatherx_grouped"
SYMBOLS = (ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY, ENTRY + "_instance")
CANONICAL = (8, 256, 256)


def line(ds, tokens, flags=0, size=256):
    buf = ctypes.create_string_buffer(size)
    rc = B.lib().vptq_quant_gemm_gatherx_grouped_instance(arr(*ds), len(ds), tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    C = ctypes
    vp, pd = C.c_void_p, C.POINTER(B.LayerDesc)
    argtypes = {ENTRY + "_supported": (C.c_int, [pd, C.c_int, C.c_int]), ENTRY + "_workspace_bytes": (C.c_size_t, [pd, C.c_int, C.c_int]),
                ENTRY: (C.c_int, [pd, C.c_int, vp, C.POINTER(vp), C.c_int, C.c_int, vp, C.c_size_t, vp]),
                ENTRY + "_instance": (C.c_int, [pd, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t])}
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
        assert B.EXPORTS[s] == argtypes[s] == B.EXPORTS[s.replace("gatherx_grouped", "gather_grouped")]    # the namesakes' signatures
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    assert re.search(r"#define VPTQ_ABI_VERSION (\d+)", hdr).group(1) == "12"
    from vptq_amd import ops
    import sys
    assert callable(ops.quant_gemm_gatherx_grouped) and "quant_gemm_gatherx_grouped" in sys.modules["vptq_amd.ops.quant_gemm"].__all__
    doc = hdr[hdr.index("Batched decode of SIBLING layers of the large-codebook formats vptq_quant_gemm_gatherx serves"):
              hdr.index("VPTQ_API int " + SYMBOLS[0])]
    for word in ("Alignment:", "Workspace:", "VPTQ_E_NULL", "VPTQ_E_TOKENS", "VPTQ_E_UNSUPPORTED", "VPTQ_E_WORKSPACE", "VPTQ_E_ALIGN",
                 "BIT-IDENTICAL", "perms=K", "res=none|lds|l2", "wgcu=N", "[1, 16]", "vptq_quant_gemm_gather_px", "added within ABI 12"):
        assert word in doc, word


def test_supported_is_the_member_query_and_the_same_dtype_width_and_format_rule():
    lib = B.lib()
    sup, one = lib.vptq_quant_gemm_gatherx_grouped_supported, lib.vptq_quant_gemm_gatherx_supported
    fmts = [(16, 65536, 65536), (16, 65536, 1024), (16, 65536, 0), (8, 65536, 4096), (8, 32768, 0), (8, 65536, 256), CANONICAL]
    members = [fdesc(v, k, kr, O=O, dtype=dt, perm=p, I=I)
               for (v, k, kr), dt, p, (I, O) in itertools.product(fmts, (0, 1), (False, True), ((4096, 4096), (4096, 1024), (8192, 1024)))]
    served = 0
    for a, b in itertools.product(members, members):
        for tokens in (0, 1, 16, 17):
            want = int(1 <= tokens <= 16 and all(one(m, tokens) for m in (a, b)) and a.dtype == b.dtype and a.group_size == b.group_size and
                       (a.vector_len, a.num_centroids, a.num_res_centroids) == (b.vector_len, b.num_centroids, b.num_res_centroids))
            assert sup(arr(a, b), 2, tokens) == want, (a.out_features, b.out_features, tokens)
            served += want
    assert served > 0
    for v, k, kr in FORMATS:                                 # every format of the single entry, as a q / k / v group
        q, kk, vv = fdesc(v, k, kr, O=4096), fdesc(v, k, kr, O=1024, perm=True), fdesc(v, k, kr, O=1024)
        for n, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 0), (-1, 0)):
            assert sup(arr(q, kk, vv, q, kk), n, 5) == want, (v, k, kr, n)
    for v, k, kr in GATHER_OWNED + [CANONICAL]:              # gemm_gather's formats and the canonical format: never
        assert sup(arr(fdesc(v, k, kr), fdesc(v, k, kr, O=1024)), 2, 8) == 0
    q, kk = fdesc(16, 65536, 1024), fdesc(16, 65536, 1024, O=1024, perm=True)
    for bad in (fdesc(16, 65536, 1024, dtype=1), fdesc(16, 65536, 0), fdesc(16, 65536, 65536), fdesc(16, 65536, 1024, I=8192), fdesc(8, 65536, 1024),
                fdesc(16, 32768, 1024), fdesc(16, 65536, 1024, I=4100), fdesc(16, 65536, 1024, norm=False), fdesc(8, 65536, 256), fdesc(*CANONICAL)):
        for tokens in (1, 5, 16):
            assert sup(arr(q, kk, bad), 3, tokens) == 0 and sup(arr(bad, q), 2, tokens) == 0
            assert sup(arr(q, kk, bad), 2, tokens) == 1                      # (only descs[0 .. n) are read)
    assert sup(None, 2, 5) == 0 and lib.vptq_quant_gemm_gatherx_grouped_workspace_bytes(None, 2, 5) == 0


def test_workspace_is_one_block_per_distinct_perm_pointer():
    q = B.lib().vptq_quant_gemm_gatherx_grouped_workspace_bytes
    P1, P2, P3 = 6 << 20, 6 << 20 | 4096, 6 << 20 | 8192
    for I, tokens, (v, k, kr) in itertools.product((8, 64, TILE + 8, 2 * TILE + 264, 4096), (1, 5, 15, 16), ((16, 65536, 1024), (8, 32768, 0))):
        block = (tokens * I * 2 + 255) // 256 * 256
        mk = lambda O, ptr: with_perm(fdesc(v, k, kr, I=I, O=O), ptr) if ptr else fdesc(v, k, kr, I=I, O=O)
        cases = (((0, 0), 0), ((0, 0, 0, 0), 0),
                 ((P1, P1), 1), ((P1, P1, P1), 1), ((P1, 0), 1), ((0, P1, 0, P1), 1),
                 ((P1, P2), 2), ((P1, P2, P1), 2), ((0, P2, P1, P2), 2),
                 ((P1, P2, P3), 3), ((P3, 0, P2, P1), 3), ((P1, P2, P3, P2), 3))
        for ptrs, n_perms in cases:
            ds = arr(*[mk(O, p) for O, p in zip((36, 12, 20, 4), ptrs)])
            assert q(ds, len(ptrs), tokens) == n_perms * block, (I, tokens, ptrs)
        for bad_tokens in (0, 17):
            assert q(arr(mk(36, P1), mk(12, P2)), 2, bad_tokens) == 0            # not served: 0
        assert q(arr(mk(36, P1), mk(12, P2)), 1, tokens) == 0 and q(arr(*[mk(12, P2)] * 5), 5, tokens) == 0
    assert q(arr(with_perm(desc(I=64, O=8), P1), desc(I=64, O=8)), 2, 5) == 0     # gemm_gather's layers: not this entry's


def test_validation_returns_before_a_launch_in_the_stated_order():
    """every error is a VPTQ_E_* code (there is no device here - a launch would answer with a HIP error): NULL, tokens, n and
    unsupported, NULL y[m], x alignment, then the workspace's size, then its alignment"""
    lib = B.lib()
    call, err = lib.vptq_quant_gemm_gatherx_grouped, lib.vptq_last_error
    P1, P2 = 6 << 20, 6 << 20 | 4096
    f = lambda **kw: fdesc(16, 65536, 1024, **kw)
    good = arr(with_perm(f(O=4096), P1), with_perm(f(O=1024), P2), f(O=1024))
    bad = arr(f(O=4096), f(O=1024, dtype=1), f(O=1024))
    need = lib.vptq_quant_gemm_gatherx_grouped_workspace_bytes(good, 3, 16)
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
    assert call(arr(f(), f(I=8192), fdesc(*CANONICAL)), 3, X, ys(3), 5, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another group_size" in err()
    assert call(arr(f(), f(), fdesc(*CANONICAL)), 3, X, ys(3), 9, 0, WS, need, None) == B.E_UNSUPPORTED and \
        b"gemm_gatherx_grouped (n = 3): member 2: not a layer vptq_quant_gemm_gatherx serves" in err()
    assert call(arr(fdesc(8, 65536, 256), f()), 2, X, ys(2), 9, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 0: not a layer" in err()
    assert call(arr(f(), fdesc(16, 65536, 0)), 2, X, ys(2), 16, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another residual" in err()
    assert call(arr(f(), fdesc(8, 65536, 1024)), 2, X, ys(2), 16, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another vector length" in err()
    assert call(arr(f(), fdesc(16, 32768, 1024)), 2, X, ys(2), 16, 0, WS, need, None) == B.E_UNSUPPORTED and b"member 1: another main codebook" in err()
    holes = ys(3)
    holes[1] = None
    assert call(good, 3, X, holes, 5, 0, WS, need, None) == B.E_NULL and b"y[1]" in err()
    assert call(bad, 3, X, holes, 5, 0, WS, need, None) == B.E_UNSUPPORTED          # unsupported before a NULL y[m]
    for off in (2, 4, 8):   # x that is not 16-byte aligned: before the workspace is looked at
        assert call(good, 3, X + off, ys(3), 16, 0, None, 0, None) == B.E_UNSUPPORTED and b"gemm_gatherx_grouped: x must be 16-byte" in err()
        assert call(good, 3, X + off, holes, 16, 0, None, 0, None) == B.E_NULL      # a NULL y[m] before the alignment
    for tokens in (1, 5, 15, 16):
        need = lib.vptq_quant_gemm_gatherx_grouped_workspace_bytes(good, 3, tokens)
        assert need == 2 * ((tokens * 4096 * 2 + 255) // 256 * 256)
        assert call(good, 3, X, ys(3), tokens, 0, None, need, None) == B.E_WORKSPACE and call(good, 3, X, ys(3), tokens, 0, None, 0, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), tokens, 0, WS, need - 1, None) == B.E_WORKSPACE and b"gemm_gatherx_grouped: workspace" in err()
        assert call(good, 3, X, ys(3), tokens, 0, WS + 8, need - 1, None) == B.E_WORKSPACE       # size before alignment
        assert call(good, 3, X, ys(3), tokens, 0, WS, need // 2, None) == B.E_WORKSPACE           # one block is not enough for two permutations
        for off in (1, 2, 4, 8):   # the exact size is accepted: the NEXT check answers
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need, None) == B.E_ALIGN and b"16-byte" in err()
            assert call(good, 3, X, ys(3), tokens, 0, WS + off, need + 4096, None) == B.E_ALIGN
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(good, 3, X + 8, ys(3), 17, flags, WS, 1 << 20, None) == B.E_TOKENS and call(good, 3, X, ys(3), 5, flags, WS, 8, None) == B.E_WORKSPACE
        assert call(good, 3, X, ys(3), 5, flags, WS + 4, 1 << 20, None) == B.E_ALIGN


def inner(ds, tokens, cus=CUS):
    """the launcher's decision (gemm_gatherx_grouped_decide), restated: gemm_gatherx_decide's format fields of the first member, the
    members' row groups as one list, the grid over the whole list"""
    d = ds[0]
    v, kr = d.vector_len, d.num_res_centroids
    res_bytes = kr * v * 2
    res = "none" if res_bytes == 0 else "lds" if res_bytes <= RES_LDS_MAX else "l2"
    lds = TILE_BYTES + (res_bytes if res == "lds" else 0)
    wgcu = min(MAX_WG_PER_CU, LDS_PER_CU // lds)
    rows = 16 // v
    groups = [(m.num_indices + rows - 1) // rows for m in ds]
    grid = min(sum(groups), cus * wgcu)
    return (f"gemm_gatherx_grouped dt={'f16' if d.dtype == 0 else 'bf16'} v={v} ib={d.index_bits} rb={d.res_bits} res={res} tok={tokens} n={len(ds)} "
            f"groups={'+'.join(map(str, groups))} tiles={(d.group_size + TILE - 1) // TILE} wgcu={wgcu} grid={grid} rgs={(sum(groups) + grid - 1) // grid}")


def test_instance_line_groups_wgcu_and_perms():
    P1, P2, P3 = 6 << 20, 6 << 20 | 4096, 6 << 20 | 8192
    # q / k / v of the 8B shapes, v16-k65536-1024 (a 32 KiB table in LDS: 64 KiB, two workgroups per CU) with one shared permutation
    qkv = [with_perm(fdesc(16, 65536, 1024, O=O), P1) for O in (4096, 1024, 1024)]
    assert line(qkv, 5) == (0, "permute_x_tokens g=4096 tok=5 grid=8x2 tpt=4 perms=1 | gemm_gatherx_grouped dt=f16 v=16 ib=16 rb=10 res=lds tok=5 n=3 "
                               "groups=256+64+64 tiles=4 wgcu=2 grid=384 rgs=1")
    qkv[2].perm = P2                                                     # distinct
    assert line(qkv, 16)[1].startswith("permute_x_tokens g=4096 tok=16 grid=8x4 tpt=4 perms=2 | gemm_gatherx_grouped dt=f16 v=16 ib=16 rb=10 res=lds tok=16 n=3 ")
    qkv[1].perm = P3
    assert " perms=3 | " in line(qkv, 16)[1]
    mixed = [fdesc(16, 65536, 1024, O=4096), with_perm(fdesc(16, 65536, 1024, O=1024), P1), with_perm(fdesc(16, 65536, 1024, O=1024), P1)]
    assert " perms=1 | " in line(mixed, 9)[1] and line(mixed, 9)[1].endswith(inner(mixed, 9))
    # gate / up of the 8B shapes in bf16, v8-k32768-0: no table, four workgroups per CU, more row groups than workgroups
    assert line([fdesc(8, 32768, 0, O=14336, dtype=1)] * 2, 12) == \
        (0, "none | gemm_gatherx_grouped dt=bf16 v=8 ib=15 rb=0 res=none tok=12 n=2 groups=896+896 tiles=4 wgcu=4 grid=1024 rgs=2")
    # a 64 KiB table (v8-k65536-4096) and a 2 MiB one (v16-k65536-65536): gathered from L2, four workgroups per CU
    assert line([fdesc(8, 65536, 4096, O=O) for O in (8192, 1024, 1024)], 8)[1].endswith("rb=12 res=l2 tok=8 n=3 groups=512+64+64 tiles=4 wgcu=4 grid=640 rgs=1")
    assert line([fdesc(16, 65536, 65536, I=8192, O=O) for O in (8192, 1024, 1024)], 8)[1].endswith("rb=16 res=l2 tok=8 n=3 groups=512+64+64 tiles=8 wgcu=4 grid=640 rgs=1")
    # the LDS steps: 8 KiB table (v16 kr = 256: 40 KiB) 4 per CU, 16 KiB (v8 kr = 1024: 48 KiB) 3 per CU, 32 KiB (64 KiB) 2 per CU
    wide = (16 * 700, 16 * 300 + 4, 16 * 100)                             # 700 + 301 + 100 row groups
    for (v, k, kr), wgcu in (((16, 65536, 256), 4), ((8, 65536, 1024), 3), ((16, 65536, 1024), 2), ((8, 65536, 2048), 2), ((16, 65536, 64), 4)):
        text = line([fdesc(v, k, kr, I=64, O=O) for O in wide], 7)[1]
        grid = min(1101, CUS * wgcu)
        assert text.endswith(f"res=lds tok=7 n=3 groups=700+301+100 tiles=1 wgcu={wgcu} grid={grid} rgs={(1101 + grid - 1) // grid}"), text
    # ragged shapes: an odd last vector-row per member, a last column tile of 264 columns, four members, a mixed group
    rag = [fdesc(8, 65536, 4096, I=2 * TILE + 264, O=O) for O in (4, 12, 20, 36)]
    with_perm(rag[1], P1)
    assert line(rag, 15) == (0, "permute_x_tokens g=2312 tok=15 grid=5x4 tpt=4 perms=1 | gemm_gatherx_grouped dt=f16 v=8 ib=16 rb=12 res=l2 tok=15 n=4 "
                                "groups=1+1+2+3 tiles=3 wgcu=4 grid=7 rgs=1")
    rag16 = [fdesc(16, 65536, 0, I=TILE + 8, O=O) for O in (4, 12, 20, 36)]
    assert line(rag16, 1) == (0, "none | gemm_gatherx_grouped dt=f16 v=16 ib=16 rb=0 res=none tok=1 n=4 groups=1+1+2+3 tiles=2 wgcu=4 grid=7 rgs=1")
    # the general form, from the launch-shape arithmetic: every format of the single entry, both dtypes
    seen = set()
    for outs, I, (v, k, kr), dt, tokens in itertools.product(((4096, 1024, 1024), (4, 12, 20, 36), wide, (14336, 14336)), (64, TILE + 8), FORMATS, (0, 1), (1, 5, 16)):
        ds = [fdesc(v, k, kr, I=I, O=O, dtype=dt) for O in outs]
        want = "none | " + inner(ds, tokens)
        assert line(ds, tokens) == (0, want)
        for flags in (B.GEMV_FAST_MATH, B.GEMV_EXACT, B.GEMV_OUT_F32):
            assert line(ds, tokens, flags) == (0, want)
        seen.add((dt, v, re.search(r"res=(\w+)", want).group(1)))
    assert len(seen) == 12                                                # every (dtype, V, RES)
    # the call's own errors, a buffer that is too small, NULL
    assert line(qkv, 0)[0] == B.E_TOKENS and line(qkv, 17)[0] == B.E_TOKENS and line(qkv[:1], 5)[0] == B.E_UNSUPPORTED
    assert line([fdesc(16, 65536, 1024), fdesc(8, 65536, 256)], 5) == (B.E_UNSUPPORTED, "")
    for size in (4, 16, 60, 120):   # (shorter than "none | ", than the permute part, than the whole line)
        assert line(qkv, 5, size=size) == (B.E_WORKSPACE, "")
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gatherx_grouped_instance(arr(*qkv), 3, 5, 0, None, 0) == B.E_NULL
    assert B.lib().vptq_quant_gemm_gatherx_grouped_instance(None, 3, 5, 0, small, len(small)) == B.E_NULL


def test_census_of_the_compile_unit():
    """gemm_gatherx_grouped.hip: one `__global__` with <typename DT, int V, int RES>, 12 instantiations, gemm_gather_tile.h's phases,
    plain stores; gemm_gatherx.hip does not know it"""
    csrc = os.path.join(ROOT, "vptq_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_gatherx_grouped.hip")).read()
    assert len(re.findall(r"__global__", src)) == 1
    assert re.search(r"template <typename DT, int V, int RES>\s*__global__ __launch_bounds__\(kGTThreads\) void gemm_gatherx_grouped_kernel\(", src)
    assert set(re.findall(r"gemm_gatherx_grouped_kernel<DT, V, (\d)>", src)) == {"0", "1", "2"}
    assert set(re.findall(r"launch_gxg_v<DT, (\d+)>", src)) == {"8", "16"}
    assert "launch_gxg_dt<F16>" in src and "launch_gxg_dt<BF16>" in src
    for phase in ("gt_load_a<false>", "gt_rebuild<DT, RES != 0>", "gt_write_tile(", "gt_epilogue<DT>", "gt_load_sb(", "gt_dcol("):
        assert phase in src, phase
    code = re.sub(r"//[^\n]*", "", src)   # (the comments say "no atomics")
    assert "atomic" not in code and "asm" not in code and "getenv" not in code and "hipFuncSetAttribute" not in code and not re.search(r"^\s*#\s*if", code, re.M)
    assert "PERM" not in code and "kGXGMembers = 4" in src
    # RES = 1: a barrier on either side of the residual table's re-staging at a member switch
    kernel = src[src.index("void gemm_gatherx_grouped_kernel("):src.index("// ---- host side")]
    assert re.search(r"if constexpr \(RES == 1\) \{\s*__syncthreads\(\);[^\n]*\n(?:[^\n]*\n){1,4}?\s*__syncthreads\(\);\s*\}", kernel)
    assert "A change to one copy belongs in the other" in src
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert srcs.count("gemm_gatherx_grouped.hip") == 1 and srcs.count("gemm_gatherx.hip") == 1
    for f in ("gemm_gatherx.hip", "gemm_gather.hip", "gemm_gather_tile.h", "gemm_gather_host.h"):
        assert "gatherx_grouped" not in open(os.path.join(csrc, f)).read(), f
    # the entry: validation before any launch, one permute launch per distinct permutation, then ONE kernel launch over the plain forms
    abi = open(os.path.join(csrc, "abi.hip")).read()
    body = abi[abi.index("int vptq_quant_gemm_gatherx_grouped("):abi.index("int vptq_quant_gemm_gatherx_grouped_instance(")]
    assert body.index("VPTQ_E_WORKSPACE") < body.index("VPTQ_E_ALIGN") < body.index("launch_permute_x_tokens") < body.index("launch_gemm_gatherx_grouped")
    assert body.count("launch_gemm_gatherx_grouped(") == 1 and "G.plain" in body and "grouped_gather_decide(" in body


GROUPS = (((4096, 1024, 1024), 4096), ((8192, 1024, 1024), 8192), ((14336, 14336), 4096), ((28672, 28672), 8192), ((1024, 1024), 4096),
          ((4, 12, 20, 36), 2 * TILE + 264), ((512, 512), 2048), ((11200, 4804, 1600), 64), ((4096, 1024, 1024, 1024), 4096))
ROUTE_FORMATS = FORMATS + GATHER_OWNED + [CANONICAL, (8, 4096, 256), (4, 65536, 0)]


def test_route_function_is_pure_follows_its_cells_and_obeys_its_knob(monkeypatch):
    from vptq_amd import grouped_decode as gd
    route = gd.gemm_gatherx_grouped_route
    assert (gd.GEMM_GATHERX_GROUPED_MIN_TOKENS, gd.GEMM_GATHERX_GROUPED_MAX_TOKENS, gd.GEMM_GATHERX_GROUPED_MIN_ELEMENTS,
            gd.GEMM_GATHERX_GROUPED_MAX_MEMBERS) == (5, 16, 2 << 20, 4)
    assert gd._GEMM_GATHERX_GROUPED_MODE == "auto"

    def by_the_cells(cells, v, k, kr, outs, I, t, perm):
        """the rule, restated by hand"""
        n_el = sum((o + v - 1) // v for o in outs) * I
        return (v, k, kr) in FORMATS and perm is not None and 2 <= len(outs) <= 4 and I % 8 == 0 and \
            any((cv, ck, ckr, cp, cn) == (v, k, kr, perm, len(outs)) and n_el >= max(lo_el, 2 << 20) and (hi_el is None or n_el <= hi_el) and
                lo <= t <= hi for cv, ck, ckr, cp, cn, lo_el, hi_el, lo, hi in cells)

    def check(cells):
        for (outs, I), (v, k, kr), perm in itertools.product(GROUPS, ROUTE_FORMATS, (False, True, None)):
            for t in (-1, 0, 1, 4, 17, 18, 19, 20):
                assert not route(v, k, kr, outs, I, t, perm)                   # outside 5 .. 16: never
            on = [t for t in range(-1, 21) if route(v, k, kr, outs, I, t, perm)]
            assert on == [t for t in range(5, 17) if by_the_cells(cells, v, k, kr, outs, I, t, perm)], (v, k, kr, outs, I, perm)
            assert on == list(range(on[0], on[-1] + 1)) if on else True         # the routed token counts of a group are one interval
            assert gd.gemm_gatherx_grouped_tokens(v, k, kr, outs, I, perm) == tuple(on)
            if (v, k, kr) not in FORMATS or sum((o + v - 1) // v for o in outs) * I < 2 << 20:
                assert not on, (outs, I)                                        # only gemm_gatherx's formats, nothing under 2 M elements

    # the committed table: well-formed, nothing under the floor, followed exactly (it may be empty)
    cells = gd._GEMM_GATHERX_GROUPED_CELLS
    assert isinstance(cells, tuple)
    assert all(len(c) == 9 and c[:3] in FORMATS and c[3] in (False, True) and 2 <= c[4] <= 4 and c[5] >= 2 << 20 and (c[6] is None or c[6] >= c[5]) and
               5 <= c[7] <= c[8] <= 16 for c in cells)
    check(cells)
    # a monkeypatched table is followed exactly - a cell under the floor, the member count and the most-elements column included
    cells = ((16, 65536, 1024, True, 3, 1 << 20, 5 << 20, 5, 16), (16, 65536, 65536, False, 2, 3 << 20, None, 5, 8), (8, 32768, 0, True, 3, 1 << 10, None, 9, 12),
             (8, 65536, 4096, False, 2, 14 << 20, 14 << 20, 16, 16))
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_CELLS", cells)
    check(cells)
    qkv, gu = (4096, 1024, 1024), (14336, 14336)
    assert not route(16, 65536, 1024, qkv, 4096, 5, True)                                                # 1.5 M elements of v = 16: under the floor
    assert route(16, 65536, 1024, (8192, 1024, 1024), 8192, 5, True) and not route(16, 65536, 1024, (8192, 1024, 1024), 8192, 5, False)
    assert not route(16, 65536, 1024, (8192, 1024, 1024), 8192, 5, None) and not route(16, 65536, 1024, (28672, 28672, 28672), 8192, 5, True)
    assert route(16, 65536, 65536, gu, 4096, 8, False) and not route(16, 65536, 65536, gu, 4096, 9, False) and not route(16, 65536, 65536, gu, 4096, 8, True)
    assert route(8, 32768, 0, qkv, 4096, 9, True) and not route(8, 32768, 0, qkv, 4096, 8, True) and not route(8, 32768, 0, (512, 512, 512), 2048, 9, True)
    assert route(8, 65536, 4096, gu, 4096, 16, False) and not route(8, 65536, 4096, (28672, 28672), 8192, 16, False)
    assert not route(8, 32768, 0, qkv, 4100, 9, True) and not route(8, 32768, 0, (4096,), 4096, 9, True) and not route(8, 32768, 0, qkv + gu, 4096, 9, True)
    assert [route(8, 32768, 0, qkv, 4096, t, True) for t in range(30)] == [route(8, 32768, 0, qkv, 4096, t, True) for t in range(30)]
    # the knob: 1 - every group of the kernel's formats from 5 to 16 tokens, whatever its size and permutations; 0 - none
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "1")
    assert all(route(v, k, kr, (36, 12), 1032, t, p) for v, k, kr in FORMATS for t in range(5, 17) for p in (False, True, None))
    assert not any(route(v, k, kr, qkv, 4096, t, True) for v, k, kr in GATHER_OWNED + [CANONICAL, (8, 4096, 256), (4, 65536, 0)] for t in range(0, 30))
    assert not route(16, 65536, 1024, qkv, 4096, 4, True) and not route(16, 65536, 1024, qkv, 4096, 17, True)
    assert not route(16, 65536, 1024, qkv + gu, 4096, 5, True) and not route(16, 65536, 1024, (4096,), 4096, 5, True) and not route(16, 65536, 1024, qkv, 4100, 5, True)
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "0")
    assert not any(route(v, k, kr, outs, I, t, p) for (outs, I) in GROUPS for v, k, kr in ROUTE_FORMATS for t in range(0, 30) for p in (False, True, None))


def test_the_knob_is_read_once_through_tune_env_and_the_group_knobs_do_not_reach_each_other(monkeypatch):
    src = open(os.path.join(ROOT, "vptq_amd", "grouped_decode.py")).read()
    assert src.count("VPTQ_GEMM_GATHERX_GROUPED\"") == 1
    assert '_GEMM_GATHERX_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHERX_GROUPED", "auto") or "auto").strip().lower()' in src
    assert "os.environ" not in src and "import torch" not in src and "getenv" not in src        # pure: no device, no tensors
    for f in ("vptq_amd/layers/vqlinear.py", "vptq_amd/ops/quant_gemm.py", "vptq_amd/_backend.py", "vptq_amd/batched_decode.py",
              "vptq_amd/csrc/gemm_gatherx_grouped.hip", "vptq_amd/csrc/abi.hip"):
        assert "VPTQ_GEMM_GATHERX_GROUPED" not in open(os.path.join(ROOT, f)).read(), f
    from vptq_amd import grouped_decode as gd
    qkv = (4096, 1024, 1024)

    def others():
        return [(gd.gemm_gather_grouped_route(8, 65536, kr, qkv, 4096, t, p), gd.gemm_gatherw_grouped_route(8, 65536, kr, qkv, 4096, t, p),
                 gd.gemm_k256_grouped_route(qkv, 4096, t, p)) for kr in (0, 256, 65536) for t in range(0, 60) for p in (False, True, None)]
    before = others()
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "1")
    assert before == others()
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "0")
    for knob in ("_GEMM_GATHER_GROUPED_MODE", "_GEMM_GATHERW_GROUPED_MODE", "_GEMM_K256_GROUPED_MODE"):
        monkeypatch.setattr(gd, knob, "1")
    assert not any(gd.gemm_gatherx_grouped_route(v, k, kr, qkv, 4096, t, True) for v, k, kr in FORMATS for t in range(0, 30))


def test_route_records_the_older_tables_as_they_were_and_the_new_record_behind_the_reader():
    from vptq_amd import grouped_decode as gd
    assert [r.entry for r in gd.GROUPED_DECODE_ROUTES] == ["vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_k256_grouped"]
    assert [r.entry for r in gd.GROUPED_DECODE_WIDE_ROUTES] == ["vptq_quant_gemm_gatherw_grouped"]
    assert (gd.GROUPED_DECODE_MIN_TOKENS, gd.GROUPED_DECODE_MAX_TOKENS) == (5, 48)
    assert [(r.entry, r.min_tokens, r.max_tokens, r.off_flags, r.exact_only) for r in gd.GROUPED_DECODE_X_ROUTES] == \
        [(ENTRY, 5, 16, B.GEMV_FORCE_GENERIC, False)]
    new = gd.GROUPED_DECODE_X_ROUTES[0]
    assert gd.GROUPED_DECODE_MIN_TOKENS <= new.min_tokens and new.max_tokens <= gd.GROUPED_DECODE_MAX_TOKENS     # inside the callers' guard
    for v, k, kr in ROUTE_FORMATS:
        old = gd.grouped_decode_routes(v, k, kr)
        got = gd.sibling_decode_routes(v, k, kr)
        if old:
            assert got == old and not new.owns(v, k, kr)                   # wherever the older reader answers: its answer
        else:
            assert got == ((new,) if (v, k, kr) in FORMATS else ())
            assert gd.grouped_decode_route(v, k, kr) is None
        assert bool(old) == ((v, k, kr) in GATHER_OWNED + [CANONICAL])
        assert new.owns(v, k, kr) == ((v, k, kr) in FORMATS)
    assert gd.grouped_decode_routes(16, 65536, 0) == () and gd.grouped_decode_routes(8, 32768, 0) == ()
    assert gd.grouped_decode_route(16, 65536, 0) is None and gd.grouped_decode_route(8, 32768, 0) is None
    assert gd.sibling_decode_routes(8, 4096, 256) == () and gd.sibling_decode_routes(4, 65536, 0) == ()
    # the record's functions are the module's
    qkv = (8192, 1024, 1024)
    for t, p in itertools.product((4, 5, 16, 17), (False, True, None)):
        assert new.route(16, 65536, 1024, qkv, 8192, t, p) == gd.gemm_gatherx_grouped_route(16, 65536, 1024, qkv, 8192, t, p)
    assert new.tokens(16, 65536, 1024, qkv, 8192, True) == gd.gemm_gatherx_grouped_tokens(16, 65536, 1024, qkv, 8192, True)
    # the older group tables: their committed cells as they were
    assert gd._GEMM_GATHER_GROUPED_CELLS == ((256, False, 3 << 20, 5, 8),)
    assert gd._GEMM_K256_GROUPED_CELLS == ((True, 3, 3 << 20, 10 << 20, 5, 48), (False, 3, 3 << 20, 10 << 20, 5, 48), (True, 2, 14 << 20, 56 << 20, 5, 48))


# ---- SiblingGroup.forward_batched: the host protocol, over stub members and a stubbed launch ----------------------------------------

class _XMember(_Member):
    """a stub layer of one of gemm_gatherx's formats (default v16-k65536-1024)"""

    def __init__(self, O, perm=None, fmt=(16, 65536, 1024), I=64):
        super().__init__(O, perm=perm, I=I)
        v, k, kr = fmt
        self.vector_len, self.num_centroids, self.num_res_centroids, self.enable_residual = v, k, kr, kr > 0
        d = fdesc(v, k, kr, I=I, O=O)
        if perm is not None:
            with_perm(d, self.cache.desc.perm)
        self.cache.desc = d


def _group(monkeypatch, members, mode="1"):
    from vptq_amd import grouped_decode as gd, ops
    from vptq_amd.layers.vqlinear import SiblingGroup
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", mode)
    for knob in ("_GEMM_GATHER_GROUPED_MODE", "_GEMM_GATHERW_GROUPED_MODE", "_GEMM_K256_GROUPED_MODE"):
        monkeypatch.setattr(gd, knob, "1")
    calls = []

    def launch(x, descs, outs, out_f32=False):
        calls.append((x, [descs[i].perm for i in range(len(outs))], tuple(outs)))
        return [torch.full(x.shape[:-1] + (o,), float(len(calls) * 10 + i)) for i, o in enumerate(outs)]

    def wrong(*a, **kw):
        raise AssertionError("another format's group launch for a gemm_gatherx group")
    monkeypatch.setattr(ops, "quant_gemm_gatherx_grouped", launch)
    for other in ("quant_gemm_gather_grouped", "quant_gemm_gatherw_grouped", "quant_gemm_k256_grouped"):
        monkeypatch.setattr(ops, other, wrong)
    return SiblingGroup(members), calls


def test_forward_batched_leader_followers_and_a_stale_follower(monkeypatch):
    q, k, v = _XMember(32), _XMember(16), _XMember(16)
    g, calls = _group(monkeypatch, [q, k, v])
    assert g._batched_static() == (16, 65536, 1024, (32, 16, 16), 64, False) and g._batched_route().entry == ENTRY
    assert [g._batched_route(t).entry if g._batched_route(t) else None for t in (4, 5, 16, 17, 48)] == [None, ENTRY, ENTRY, None, None]
    for tokens in (5, 16):
        x = torch.zeros(tokens, 64, dtype=torch.float16)
        n = len(calls)
        yq = g.forward_batched(q, x, tokens)
        assert len(calls) == n + 1 and calls[-1][0] is x and calls[-1][2] == (32, 16, 16) and yq.shape == (tokens, 32) and float(yq[0, 0]) == 10.0 * (n + 1)
        yk, yv = g.forward_batched(k, x, tokens), g.forward_batched(v, x, tokens)
        assert len(calls) == n + 1 and float(yk[0, 0]) == 10.0 * (n + 1) + 1 and float(yv[0, 0]) == 10.0 * (n + 1) + 2    # the followers pick their share up
        assert g._bx is None and not g._bout                                               # ... once: nothing is held afterwards
    for tokens in (4, 17, 48):                                                             # outside the window: nothing
        assert g.forward_batched(q, torch.zeros(tokens, 64, dtype=torch.float16), tokens) is None and len(calls) == 2
    # a follower is the leader of the next tensor; outputs left unconsumed are stale: a new leader call drops them
    x2, x3 = torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8, 64, dtype=torch.float16)
    assert float(g.forward_batched(v, x2, 8)[0, 0]) == 32.0 and set(g._bout) == {id(q), id(k)}
    assert float(g.forward_batched(q, x3, 8)[0, 0]) == 40.0 and len(calls) == 4 and set(g._bout) == {id(k), id(v)}
    assert float(g.forward_batched(k, x2, 8)[0, 0]) == 51.0 and len(calls) == 5          # k with the OLD tensor: stale, it launches
    # an x rewritten in place between the sibling calls: the follower launches for itself
    x4 = torch.zeros(9, 64, dtype=torch.float16)
    g.forward_batched(q, x4, 9)
    x4.add_(1)
    assert float(g.forward_batched(k, x4, 9)[0, 0]) == 71.0 and len(calls) == 7
    with torch.inference_mode():
        xi = torch.zeros(9, 64, dtype=torch.float16)
    assert B.tensor_version(xi) == -1
    assert g.forward_batched(q, xi, 9) is None and g.forward_batched(k, xi, 9) is None and len(calls) == 7        # never shared, never launched
    # an x that is not what the entry takes
    assert g.forward_batched(q, torch.zeros(9 * 64 + 4, dtype=torch.float16)[4:].view(9, 64), 9) is None          # 8 bytes off
    assert g.forward_batched(q, torch.zeros(9, 64, dtype=torch.bfloat16), 9) is None and g.forward_batched(q, torch.zeros(9, 32, dtype=torch.float16), 9) is None


def test_forward_batched_steps_aside_for_the_knob_off_flags_a_missing_entry_and_a_compacted_member(monkeypatch):
    from vptq_amd import grouped_decode as gd, ops
    q, k = _XMember(32), _XMember(16)
    g, calls = _group(monkeypatch, [q, k])
    x = torch.zeros(12, 64, dtype=torch.float16)
    for mode in ("0", "auto"):                                           # the knob at 0 and at "auto" (nothing this small is in a cell)
        monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", mode)
        assert g.forward_batched(q, x, 12) is None and not calls
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "1")
    monkeypatch.setattr(ops, "quant_gemm_flags", lambda: B.GEMV_FORCE_GENERIC)      # launch flags that force another kernel
    assert g.forward_batched(q, x, 12) is None and not calls
    monkeypatch.setattr(ops, "quant_gemm_flags", lambda: 0)
    k.__dict__["_compact"] = {}                                          # a compacted member: the group steps aside
    assert g.forward_batched(q, x, 12) is None and g.forward_batched(k, x, 12) is None and not calls
    del k.__dict__["_compact"]
    assert g.forward_batched(q, x, 12) is None and not calls             # (remembered for these descriptors ...)
    k.rebuild()                                                          # (... compacting / uncompacting a layer rebuilds its descriptor)
    assert g.forward_batched(q, x, 12) is not None and len(calls) == 1
    old = g._batched_plan()
    assert old is g._batched_plan(g._batched_route(12))
    q.rebuild()
    assert g._batched_plan() is not old
    # a capture with too small a workspace: the launch wrapper answers None, nothing is shared
    monkeypatch.setattr(ops, "quant_gemm_gatherx_grouped", lambda *a, **kw: None)
    x2 = torch.zeros(12, 64, dtype=torch.float16)
    assert g.forward_batched(q, x2, 12) is None and g.forward_batched(k, x2, 12) is None and g._bx is None
    # mixed formats, mixed dtypes, a group the library does not serve
    g2, calls2 = _group(monkeypatch, [_XMember(32), _XMember(16, fmt=(16, 65536, 0))])
    assert g2._batched_route(12) is None and g2.forward_batched(g2.members[0], x, 12) is None and not calls2
    a, b = _XMember(32), _XMember(16)
    b.cache.dtype = torch.bfloat16
    g3, calls3 = _group(monkeypatch, [a, b])
    assert g3.forward_batched(a, x, 12) is None and not calls3
    c, d = _XMember(32), _XMember(16)
    d.cache.desc.weight_scale = None                                     # (no scale: vptq_quant_gemm_gatherx_supported says no)
    d.cache.desc.weight_bias = None
    g4, calls4 = _group(monkeypatch, [c, d])
    assert g4.forward_batched(c, x, 12) is None and not calls4
    # a library that lacks the entry: the group steps aside
    real = B.lib()

    class Old:
        def __getattr__(self, name):
            if "gatherx_grouped" in name:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(B, "lib", lambda: Old())
    e, f = _XMember(32), _XMember(16)
    g5, calls5 = _group(monkeypatch, [e, f])
    assert g5.forward_batched(e, x, 12) is None and not calls5 and g5._batched_workspace_bytes() is None


def test_forward_batched_shares_one_perm_pointer_and_sizes_the_workspace(monkeypatch):
    from vptq_amd import grouped_decode as gd
    p = torch.randperm(64).to(torch.int16)
    q, k, v, o = _XMember(32, perm=p), _XMember(16, perm=p.clone()), _XMember(16, perm=torch.arange(64).to(torch.int16)), _XMember(8)
    g, calls = _group(monkeypatch, [q, k, v, o])
    x = torch.zeros(16, 64, dtype=torch.float16)
    assert g.forward_batched(q, x, 16) is not None
    ptrs = calls[0][1]
    own = [m.cache.desc.perm for m in (q, k, v, o)]
    assert len({own[0], own[1], own[2]}) == 3 and own[3] is None
    assert ptrs[0] == own[0] and ptrs[1] == own[0] and ptrs[2] == own[2] and ptrs[3] is None    # equal tensors: the leader's pointer; others their own
    assert [m.cache.desc.perm for m in (q, k, v, o)] == own                                     # the members' own descriptors are untouched
    assert g._batched_static()[5] is None                                                       # (a mixed group: some members have a permutation)
    # `prepare_model`'s question: two distinct permutations at 16 tokens with the knob on, nothing with it at auto / off
    assert g._batched_workspace_bytes() == (torch.device("cpu"), 0, 2 * 16 * 64 * 2)
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "auto")
    assert g._batched_workspace_bytes() is None
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "0")
    assert g._batched_workspace_bytes() is None
    # a routed cell sizes it at the cell's largest token count
    ms = [_XMember(4096, perm=p, I=4096) for _ in range(3)]
    g2, _ = _group(monkeypatch, ms, mode="auto")
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_CELLS", ((16, 65536, 1024, True, 3, 2 << 20, None, 5, 12),))
    assert g2._batched_workspace_bytes() == (torch.device("cpu"), 0, 12 * 4096 * 2)


def test_the_gpu_bit_rows_cover_every_instantiation_group_size_and_permutation_case():
    """the parametrisation of tests/test_gemm_gatherx_grouped_gpu.py's bit rows, checked here because it needs no device: every
    (V, RES, dtype), group size, permutation case, (columns, tokens) pair and member output is among the rows"""
    from test_gemm_gatherx_grouped_gpu import _bit_rows, FMTS, FMT, RES, PERM_CASES, GS, TOKS, OUTS
    rows = [e.values[0] for e in _bit_rows()]
    assert {(e["fmt"], e["dt"]) for e in rows} == set(itertools.product(FMTS, ("f16", "bf16")))
    assert {(FMT[e["fmt"]][0], RES[e["fmt"]], e["dt"]) for e in rows} == set(itertools.product((8, 16), (0, 1, 2), ("f16", "bf16")))
    assert {(e["fmt"], e["dt"]) for e in rows if e["model"]} == set(itertools.product(FMTS, ("f16", "bf16")))
    assert {(e["fmt"], e["case"]) for e in rows} == set(itertools.product(FMTS, PERM_CASES))
    assert {(len(e["outs"]), e["case"]) for e in rows} == set(itertools.product((2, 3, 4), PERM_CASES))
    assert {(e["G"], e["tokens"]) for e in rows} == set(itertools.product(GS, TOKS))
    assert {(FMT[e["fmt"]][0], o) for e in rows for o in e["outs"]} == set(itertools.product((8, 16), OUTS))
    assert {e["bias"] for e in rows} == {0, 1}
