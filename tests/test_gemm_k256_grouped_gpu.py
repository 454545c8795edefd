"""vptq_quant_gemm_k256_grouped (gemm_k256_grouped_kernel in gemm_k256.hip): 1 - 48 tokens of 2 - 4 sibling layers of the canonical
format in ONE launch, one x[perm] gather per distinct permutation - on the GPU.

The contract is BITS, no tolerance: the order of every sum of gemm_k256_pass depends neither on the grid nor on the workgroup that runs a
row group, so member m's y equals, bit for bit, what the member's OWN entry gives on the same descriptor and x.  The own entry is
vptq_quant_gemv with VPTQ_GEMV_EXACT up to 16 tokens (vptq_quant_gemv_kernel_name asserted to be "gemm_k256_kernel") and
vptq_quant_gemm_k256w for 17 - 48.  That comparison is the parent's code.  vptq_quant_gemv gives 1 - 4 tokens to the GEMV kernels, so
for those counts the own entry runs on 5 tokens - the call's rows first, rows of another seed behind them - and its first rows are the
comparison: the tokens are the M rows of the MFMA and a token's bits do not depend on its batch (tests/test_gemm_k256w_gpu.py, 5).

TILE = 1024 columns per tile and ROWS = 4 vector-rows (32 outputs) per row group are the kernel's.  Columns 8, 64, TILE + 8 and
2 TILE + 264, member outputs from {8, 24, 36, 72} (a partial last row group, padded outputs), tokens 1 / 5 / 15 / 16 / 17 / 32 / 33 / 48.

  1. bits: every member, 16-bit and fp32 outputs, groups of 2 / 3 / 4, every permutation case; every row against the float64 model
  2. member switches and every pass size inside one workgroup: more row groups than CUs, members of 4 CUs + 2, 3 and 2 CUs + 1 row groups
  3. weights: one-hot activations read vptq_dequant's bits for every member
  4. placement: every operand in an arena of its own, guarded y, the workspace exactly the query's bytes at 16-byte alignment
  5. graph capture of the entry, replayed on new activations
  6. the module: link_siblings, leader / followers, an x rewritten in place, the knob at 0, the folded arithmetic, prepare_model + capture"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_k256w_gpu import call as k256w_call, TILE, ROWS, GUARD, SENTINEL, F32, EXACT, _bits
from test_gemm_gather_px_gpu import _stream_without_a_workspace
from test_gemm_gather_grouped_gpu import group_descs, distinct_perms, _x, _Block, QKV, GU, PX_THREADS, PX_TOK
import _arena as ar
import _arith_model as am
from _gpu_util import spec_to_module, gemv_abi, module_desc

pytestmark = pytest.mark.gpu

GS = (8, 64, TILE + 8, 2 * TILE + 264)
OUTS = (8, 24, 36, 72)
TOKS = (1, 5, 15, 16, 17, 32, 33, 48)
PERM_CASES = ("shared", "distinct", "mixed", "none")
ENTRY = "vptq_quant_gemm_k256_grouped"
LAUNCHES = (ENTRY, "vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_k256w", "vptq_quant_gemv", "vptq_quant_gemv_grouped", "vptq_dequant")


def make_group(G, outs, dt, perms, bias=1):
    """-> [LayerSpec] of the canonical format: members of different seeds (their codebooks, scales and biases differ); perms: "shared" -
    every member has the first member's permutation, "distinct" - its own, "mixed" - every other member has one (the first member's),
    "none"; member 1 has no output bias"""
    from oracle import vptq_oracle as vo
    Ls, shared = [], None
    for i, O in enumerate(outs):
        has = perms in ("shared", "distinct") or (perms == "mixed" and i % 2 == 0)
        L = vo.make_layer(G, O, dist="llm", seed=G + O + 1000 * i, dtype=dt, enable_perm=has, bias=bool(bias) and i != 1)
        assert (L.vector_len, L.num_centroids, L.num_res_centroids) == (8, 256, 256)
        if has and perms in ("shared", "mixed"):
            if shared is None:
                shared = L.perm
            L.perm = shared.copy()
        Ls.append(L)
    return Ls


def instance(descs, n, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(320)
    B.check(getattr(B.lib(), ENTRY + "_instance")(descs, n, tokens, 0, buf, len(buf)), ENTRY + "_instance")
    return buf.value.decode()


def walk(groups, grid, tb):
    """-> (rgs, passes text, per-workgroup list of (member, passes)) from the launch-shape arithmetic: workgroup w owns the global row
    groups w, w + grid, ...; inside a member its `left` row groups run as passes of 4, 2, 1 (tb = 1) or one by one (tb > 1)"""
    first = [sum(groups[:m]) for m in range(len(groups) + 1)]
    rgs, seen, per_wg = 0, set(), []
    for w in range(grid):
        mine, total = [], 0
        for m in range(len(groups)):
            left = sum(1 for g in range(w, first[-1], grid) if first[m] <= g < first[m + 1])
            if left == 0:
                continue
            total += left
            ps = [1] * left if tb > 1 else [4] * (left // 4) + [2] * ((left % 4) // 2) + [1] * (left % 2)
            seen |= set(ps)
            mine.append((m, tuple(ps)))
        rgs = max(rgs, total)
        per_wg.append(tuple(mine))
    return rgs, (f"1x{tb}" if tb > 1 else "+".join(str(p) for p in (4, 2, 1) if p in seen)), per_wg


def expect_instance(descs, ds, Ls, tokens):
    from vptq_amd import _backend as B
    n, G = len(ds), Ls[0].in_features
    assert getattr(B.lib(), ENTRY + "_supported")(descs, n, tokens) == 1
    k = distinct_perms(ds)
    need = k * ((tokens * G * 2 + 255) // 256 * 256)
    assert getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens) == need
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = [(L.num_indices + ROWS - 1) // ROWS for L in Ls]
    grid, tb = min(sum(groups), cus), (tokens + 15) // 16
    rgs, passes, _ = walk(groups, grid, tb)
    head = "none" if k == 0 else \
        f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK} perms={k}"
    want = (f"{head} | gemm_k256_grouped dt={Ls[0].dtype} tok={tokens} tb={tb} n={n} groups={'+'.join(map(str, groups))} "
            f"grid={grid} rgs={rgs} passes={passes}")
    text = instance(descs, n, tokens)
    assert text == want, (text, want)
    return need


def grouped_call(descs, n, xt, outs, out_f32=False, ws=None):
    """the entry with every y's token rows NaN between guard rows and a workspace of EXACTLY the query's bytes (0xFF bytes unless one
    is handed in); -> [y_m [tokens, O_m]] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens)
    if ws is None and need:
        ws = torch.full((need,), 255, dtype=torch.uint8, device=xt.device)
    bufs = [torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device) for O in outs]
    for b in bufs:
        b[GUARD:GUARD + tokens] = float("nan")
    ys = [b[GUARD:GUARD + tokens] for b in bufs]
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    B.check(getattr(B.lib(), ENTRY)(descs, n, xt.data_ptr(), yp, tokens, F32 if out_f32 else 0, None if ws is None else ws.data_ptr(),
                                    0 if ws is None else ws.numel(), B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return [y.clone() for y in ys]


def own_entry(mod, d, xt, O, out_f32=False):
    """the member's own entry on the same descriptor and x: the comparison (the parent's code)"""
    from vptq_amd import _backend as B
    tokens = xt.shape[0]
    if tokens > 16:
        assert B.lib().vptq_quant_gemm_k256w_supported(d, tokens) == 1
        return k256w_call(d, xt, O, out_f32=out_f32)
    assert B.lib().vptq_quant_gemv_kernel_name(d, max(tokens, 5), EXACT) == b"gemm_k256_kernel"
    if tokens >= 5:
        return gemv_abi(mod, xt, EXACT, out_f32=out_f32)
    # 1 - 4 tokens: the batched kernel starts at 5 - the call's rows in front of rows of another seed (the module docstring)
    pad = torch.flip(xt, dims=(1,))[:1].expand(5 - tokens, -1) * 0.5
    return gemv_abi(mod, torch.cat([xt, pad]).contiguous(), EXACT, out_f32=out_f32)[:tokens]


def check_bits(ys, ms, ds, xt, outs, f32, what=""):
    for m, (y, mod, d, O) in enumerate(zip(ys, ms, ds, outs)):
        assert not bool(torch.isnan(y).any()), (what, m)
        want = own_entry(mod, d, xt, O, out_f32=f32)
        assert torch.equal(_bits(y), _bits(want)), f"{what} member {m}: {int((_bits(y) != _bits(want)).sum())} of {y.numel()} outputs differ from its own entry"


# ---------------------------------------------------------------------------------------------- 1. bits and sums
def _bit_rows():
    rows = []
    for i, (G, tokens) in enumerate(itertools.product(GS, TOKS)):
        # 32 rows: every (columns, tokens); permutation case, members, dtype and bias advance at strides of their own.  GUARANTEED (the
        # test below asserts them): every (token-block count, dtype), (token-block count, permutation case), (group size, permutation
        # case) and (columns, tokens) pair, and every member output
        case = PERM_CASES[(i + i // 5) % 4]
        n = (2, 3, 4)[(i + i // 3) % 3]
        outs = tuple(OUTS[(i + j) % 4] for j in range(n))
        rows.append(pytest.param(dict(G=G, tokens=tokens, case=case, outs=outs, dt=("f16", "bf16")[(i + i // 4) % 2], bias=(i // 3) % 2),
                                 id=f"G{G}-tok{tokens}-{case}-n{n}-i{i}"))
    return rows


def test_the_bit_rows_cover_every_tb_dtype_group_size_and_permutation_case():
    rows = [e.values[0] for e in _bit_rows()]
    tb = lambda e: (e["tokens"] + 15) // 16
    assert {(tb(e), e["dt"]) for e in rows} == set(itertools.product((1, 2, 3), ("f16", "bf16")))
    assert {(tb(e), e["case"]) for e in rows} == set(itertools.product((1, 2, 3), PERM_CASES))
    assert {(len(e["outs"]), e["case"]) for e in rows} == set(itertools.product((2, 3, 4), PERM_CASES))
    assert {(e["G"], e["tokens"]) for e in rows} == set(itertools.product(GS, TOKS))
    assert {o for e in rows for o in e["outs"]} == set(OUTS)


@pytest.mark.parametrize("e", _bit_rows())
def test_bits_equal_every_members_own_entry_and_sums_hold_the_model(e, dev):
    G, tokens, outs = e["G"], e["tokens"], e["outs"]
    Ls = make_group(G, outs, e["dt"], e["case"], bias=e["bias"])
    descs, ds, ms, keep = group_descs(Ls, dev)
    want_perms = {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[e["case"]]
    assert distinct_perms(ds) == want_perms and [bool(d.perm) for d in ds] == [L.perm is not None for L in Ls]
    expect_instance(descs, ds, Ls, tokens)
    x, xt = _x(G, tokens, e["dt"], G + tokens, dev)
    out = {}
    for f32 in (False, True):
        out[f32] = grouped_call(descs, len(ds), xt, outs, out_f32=f32)
        check_bits(out[f32], ms, ds, xt, outs, f32)
    for m, L in enumerate(Ls):
        mm, aa = am.model(am.pieces(L), x, arith="exact")
        am.check_both(_np(out[False][m]), _np(out[True][m]), mm, aa, L.dtype, what=f"member {m} of {instance(descs, len(ds), tokens)}")


# ---------------------------------------------------------------------------------------------- 2. member switches, every pass size
def _switch_outs(cus):
    """4 cus + 2, 3 and 2 cus + 1 row groups over a grid of cus workgroups (first row groups 0, 4 cus + 2, 4 cus + 5): workgroups 0 and 1
    run passes 4, 1 in member 0 and 2 in member 2; workgroups 2 .. 4 run 4 | 1 | 2 - a member they visit once between two image
    rebuilds; workgroup 5 runs 4 | 2, 1; the others 4 | 2.  Every member's last row group is partial (40, 8 and 8 outputs)"""
    return (4 * 32 * cus + 40, 72, 2 * 32 * cus + 8)


@pytest.mark.parametrize("G,dt,case,tokens", [(8, "f16", "none", 15), (64, "bf16", "shared", 16), (64, "f16", "mixed", 5), (8, "bf16", "distinct", 9),
                                              (8, "bf16", "none", 17), (64, "f16", "shared", 32), (64, "bf16", "distinct", 24)])
def test_member_switches_and_every_pass_size_inside_a_workgroup(G, dt, case, tokens, dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    outs = _switch_outs(cus)
    Ls = make_group(G, outs, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    groups = [(L.num_indices + ROWS - 1) // ROWS for L in Ls]
    assert groups == [4 * cus + 2, 3, 2 * cus + 1]
    tb = (tokens + 15) // 16
    rgs, passes, per_wg = walk(groups, cus, tb)
    if tb == 1:
        assert per_wg[0] == ((0, (4, 1)), (2, (2,))) and per_wg[2] == ((0, (4,)), (1, (1,)), (2, (2,))) and per_wg[5] == ((0, (4,)), (2, (2, 1)))
        assert (rgs, passes) == (7, "4+2+1")
    else:
        assert per_wg[2] == ((0, (1,) * 4), (1, (1,)), (2, (1,) * 2)) and (rgs, passes) == (7, f"1x{tb}")
    for a, b in ((0, 1), (1, 2)):   # members differ in codebooks, scale, bias and output bias
        assert not np.array_equal(np.asarray(Ls[a].centroids), np.asarray(Ls[b].centroids))
        assert not np.array_equal(np.asarray(Ls[a].res_centroids), np.asarray(Ls[b].res_centroids))
        assert not np.array_equal(np.asarray(Ls[a].weight_scale), np.asarray(Ls[b].weight_scale))
        assert not np.array_equal(np.asarray(Ls[a].weight_bias), np.asarray(Ls[b].weight_bias))
    assert Ls[0].bias is not None and Ls[1].bias is None and Ls[2].bias is not None
    expect_instance(descs, ds, Ls, tokens)
    x, xt = _x(G, tokens, dt, 7, dev)
    out = {}
    for f32 in (False, True):
        out[f32] = grouped_call(descs, 3, xt, outs, out_f32=f32)
        check_bits(out[f32], ms, ds, xt, outs, f32)
    for m, L in enumerate(Ls):
        mm, aa = am.model(am.pieces(L), x, arith="exact")
        am.check_both(_np(out[False][m]), _np(out[True][m]), mm, aa, L.dtype, what=f"member {m} of {instance(descs, 3, tokens)}")
    # two launches give the same bits
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 3, xt, outs), out[False]))


@pytest.mark.parametrize("dt,tokens", [("f16", 16), ("bf16", 40)])
def test_member_switches_over_three_column_tiles(dt, tokens, dev):
    """the same group at 2 TILE + 264 columns (three tiles, a clamped last one): bits against the own entries only"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    outs, G = _switch_outs(cus), 2 * TILE + 264
    Ls = make_group(G, outs, dt, "shared")
    descs, ds, ms, keep = group_descs(Ls, dev)
    expect_instance(descs, ds, Ls, tokens)
    _, xt = _x(G, tokens, dt, 8, dev)
    check_bits(grouped_call(descs, 3, xt, outs), ms, ds, xt, outs, False)


# ---------------------------------------------------------------------------------------------- 3. weights bit for bit
G1 = TILE + 8
_EDGE = [0, 1, 7, 8, 63, 64, 300, 511, 512, TILE - 2, TILE - 1, TILE, TILE + 1, G1 - 3, G1 - 2, G1 - 1]


def _cols(tokens):
    rest = [c for c in range(15, G1, 17) if c not in _EDGE]
    cols = (_EDGE + rest)[:tokens]
    return [cols[(i % 16) * (tokens // 16) + i // 16] for i in range(tokens)]   # every token block holds some of the edges


@pytest.mark.parametrize("dt,case,tokens", [("f16", "distinct", 16), ("bf16", "mixed", 32), ("bf16", "shared", 48), ("f16", "none", 48)])
def test_one_hot_activations_read_dequant_bits_for_every_member(dt, case, tokens, dev):
    outs = (24, 72, 36)
    Ls = make_group(G1, outs, dt, case, bias=0)          # (no output bias: y is a column of W)
    descs, ds, ms, keep = group_descs(Ls, dev)
    cols = _cols(tokens)
    assert len(set(cols)) == tokens and set(_EDGE) <= set(cols)
    x = torch.zeros(tokens, G1, dtype=ms[0].centroids.weight.dtype, device=dev)
    x[torch.arange(tokens), torch.tensor(cols)] = 1.0    # input feature j: it reaches stored column c with perm[c] == j
    ys = grouped_call(descs, 3, x, outs)
    for m, (y, mod) in enumerate(zip(ys, ms)):
        want = mod.dequant()[:, torch.tensor(cols, device=dev)].t()
        assert not bool(torch.isnan(y).any())
        assert bool((y == want).all()), f"member {m}: {int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 4. placement
# the least alignment the entry accepts for every operand: 16 bytes for everything the canonical-format kernels read in 16-byte pieces
# (part of "supported": gemv_k256_eligible), the output bias element-aligned
HOSTILE_OFFSETS = {"indices": 16, "centroids": 16, "res_centroids": 16, "weight_scale": 16, "weight_bias": 16, "perm": 16, "bias": 2}


def _placed_call(Ls, xt, tokens, outs, fill, offsets, x_off, y_off, f32, dev):
    from vptq_amd import _backend as B
    ms = [spec_to_module(L, dev) for L in Ls]
    arenas = {}
    for i, m in enumerate(ms):
        for k, a in ar.place_module(m, fill, {k: v for k, v in offsets.items() if k in ar._module_params(m)}).items():
            arenas[f"member {i} {k}"] = a
    pairs = [module_desc(m) for m in ms]
    ds = [d for d, _ in pairs]
    descs = (B.LayerDesc * len(ds))(*ds)
    xv, xa = ar.place(xt, fill, x_off)
    outs_placed = [ar.guarded_out((tokens, O), torch.float32 if f32 else xt.dtype, dev, y_off) for O in outs]
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, len(ds), tokens)
    assert need == distinct_perms(ds) * ((tokens * Ls[0].in_features * 2 + 255) // 256 * 256) > 0
    ws, wa = ar.guarded_workspace(need, False, dev, align=16)
    assert ws.numel() == need and ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 != 0
    assert xv.data_ptr() % 16 == 0 and (x_off == 0 or xv.data_ptr() % 32 != 0)
    yp = (C.c_void_p * len(ds))(*[y.data_ptr() for y, _ in outs_placed])
    B.check(getattr(B.lib(), ENTRY)(descs, len(ds), xv.data_ptr(), yp, tokens, F32 if f32 else 0, ws.data_ptr(), need, B.current_stream_ptr(dev)), ENTRY)
    torch.cuda.synchronize(dev)
    for name, a in list(arenas.items()) + [("x", xa)]:
        assert a.intact(), (name, a.damage())                    # the inputs' margins
    for i, (y, ya) in enumerate(outs_placed):
        assert ya.intact(), (f"y[{i}]", ya.damage())             # a store outside y
        assert not bool(torch.isnan(y).any())
    assert wa.intact(), ("workspace", wa.damage())               # a store outside the query's bytes
    assert torch.equal(xv, xt)
    return [y.clone() for y, _ in outs_placed]


@pytest.mark.parametrize("dt,G,tokens", [("f16", TILE + 8, 5), ("bf16", 2 * TILE + 264, 16), ("f16", 64, 33), ("bf16", TILE + 8, 24)])
def test_same_bits_under_every_placement(dt, G, tokens, dev):
    outs = (24, 8, 36)
    Ls = make_group(G, outs, dt, "distinct")      # (three x gathers: three blocks of the workspace)
    _, xt = _x(G, tokens, dt, 3, dev)
    for f32 in (False, True):
        benign = _placed_call(Ls, xt, tokens, outs, ar.BENIGN, {}, 0, 0, f32, dev)
        hostile = _placed_call(Ls, xt, tokens, outs, ar.HOSTILE, HOSTILE_OFFSETS, 16, 4 if f32 else 2, f32, dev)
        descs, ds, ms, keep = group_descs(Ls, dev)
        plain = grouped_call(descs, 3, xt, outs, out_f32=f32)     # torch's allocator
        for m, (a, b, c) in enumerate(zip(benign, hostile, plain)):
            assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)), m
        check_bits(plain, ms, ds, xt, outs, f32)


# ---------------------------------------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("dt,case,tokens", [("f16", "mixed", 12), ("bf16", "distinct", 16), ("f16", "none", 40), ("bf16", "shared", 24)])
def test_a_captured_call_replays_on_new_activations(dt, case, tokens, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (24, 36, 72)
    Ls = make_group(G, outs, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    xs = [_x(G, tokens, dt, s, dev)[1] for s in (1, 2, 3)]
    eager = [grouped_call(descs, 3, x, outs) for x in xs]
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, 3, tokens)
    ws = torch.full((max(need, 16),), 255, dtype=torch.uint8, device=dev)   # (sized before the capture: nothing is allocated inside it)
    xg = xs[0].clone()
    yg = [torch.full((tokens, O), float("nan"), dtype=xg.dtype, device=dev) for O in outs]
    yp = (C.c_void_p * 3)(*[y.data_ptr() for y in yg])
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            # (one stream, the permute launch(es) and one kernel launch in stream order: a linear graph)
            B.check(getattr(B.lib(), ENTRY)(descs, 3, xg.data_ptr(), yp, tokens, 0, ws.data_ptr() if need else None, need, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    for x, want in zip(xs, eager):
        xg.copy_(x)
        for y in yg:
            y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize(dev)
        assert all(torch.equal(_bits(y), _bits(w)) for y, w in zip(yg, want))


# ---------------------------------------------------------------------------------------------- 6. the module
class _Spy:
    """B.lib() with the names of the launching entries called through it recorded"""
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in LAUNCHES:
            return fn

        def spy(*a):
            self._calls.append(name)
            return fn(*a)
        return spy


def _spied(fn, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    try:
        y = fn()
    finally:
        monkeypatch.setattr(B, "lib", lambda: real)
    return y, calls


def _block(names, Ls, dev, link=True):
    from vptq_amd.layers import link_siblings
    blk = _Block(names, [spec_to_module(L, dev) for L in Ls])
    if link:
        assert link_siblings(blk) == 1
    return blk


@pytest.mark.parametrize("names,outs,dt,case,tokens", [(QKV, (512, 128, 136), "f16", "shared", 16), (GU, (264, 256), "bf16", "none", 5),
                                                       (QKV, (128, 512, 136), "bf16", "mixed", 24), (GU, (256, 264), "f16", "distinct", 48)])
def test_linked_siblings_take_one_grouped_launch_with_their_own_bits(names, outs, dt, case, tokens, dev, monkeypatch):
    import vptq_amd
    from vptq_amd import grouped_decode as gd
    I = 2048
    assert vptq_amd.arithmetic() == "reference"
    Ls = make_group(I, outs, dt, case)
    x, xt = _x(I, tokens, dt, 9, dev)
    xt = xt.reshape(1, tokens, I)
    twins = _block(names, Ls, dev, link=False)
    # the committed cells never hold a group this small: the routes of before, no grouped launch - linked or not
    assert not gd.gemm_k256_grouped_route(outs, I, tokens, {"shared": True, "distinct": True, "none": False, "mixed": None}[case])
    y_today, today = _spied(lambda: twins(xt), monkeypatch)
    assert ENTRY not in today and len(today) >= len(outs)
    y_linked, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y_linked, y_today))
    # the knob on: ONE grouped launch, the followers pick their outputs up, every member has the bits of its un-linked twin's own entry
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "1")
    blk = _block(names, Ls, dev)
    ys, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == [ENTRY], calls
    group = blk.__dict__["_modules"][names[0]].__dict__["_siblings"]
    assert group._bx is None and not group._bout
    descs, caches = group._batched_plan()
    assert distinct_perms([descs[i] for i in range(len(outs))]) == {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[case]
    for m, (y, n, L, O) in enumerate(zip(ys, names, Ls, outs)):
        mod = getattr(twins, n)
        d, keep = module_desc(mod)
        want = own_entry(mod, d, xt.reshape(tokens, I), O)
        assert y.shape == (1, tokens, O) and torch.equal(_bits(y.reshape(tokens, O)), _bits(want)), m
        assert torch.equal(_bits(y), _bits(y_today[m])), m           # ... which are the bits the member's route of before gives
        mm, aa = am.model(am.pieces(L), x, arith="exact")
        am.check_outputs(_np(y).reshape(mm.shape), mm, aa, dt, False, what=f"VQuantLinear.forward, {tokens} tokens, grouped, member {m}")
    # x rewritten in place between the sibling calls: the follower launches for itself (the whole group again), same bits
    x2 = xt.clone()

    def rewritten_between_the_calls():
        y0 = getattr(blk, names[0])(x2)
        x2.add_(0)
        return y0, getattr(blk, names[1])(x2)
    (y0, y1), calls = _spied(rewritten_between_the_calls, monkeypatch)
    assert calls == [ENTRY] * 2, calls
    assert torch.equal(_bits(y0), _bits(ys[0])) and torch.equal(_bits(y1), _bits(ys[1]))
    # tensors without a version counter are never shared: every member goes on alone over the routes of before
    with torch.inference_mode():
        xi = xt.clone()
        yi, calls = _spied(lambda: blk(xi), monkeypatch)
    assert ENTRY not in calls and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(yi, y_today))
    # the folded arithmetic: the kernel has the reference's roundings only - the group steps aside, outputs equal the ungrouped model's
    vptq_amd.set_arithmetic("folded")
    try:
        folded_twins, folded = _block(names, Ls, dev, link=False), _block(names, Ls, dev)
        y_ft, before = _spied(lambda: folded_twins(xt), monkeypatch)
        y_f, calls = _spied(lambda: folded(xt), monkeypatch)
        assert not all(getattr(folded, n)._descriptor().arithmetic_flags & EXACT for n in names), "a member must pass the folded form's gate for this test"
        assert ENTRY not in calls and calls == before, (calls, before)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y_f, y_ft))
    finally:
        vptq_amd.set_arithmetic("reference")
    # the knob at 0: the routes and the bits of before
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "0")
    y0s, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y0s, y_today))


@pytest.mark.parametrize("tokens", [8, 24])
def test_prepare_model_sizes_the_workspace_and_a_captured_step_keeps_the_group_route(tokens, dev, monkeypatch):
    import vptq_amd
    from vptq_amd import _backend as B, grouped_decode as gd, ops
    I, outs = 2 * TILE + 264, (72, 24, 36)
    Ls = make_group(I, outs, "f16", "distinct")
    monkeypatch.setattr(gd, "_GEMM_K256_GROUPED_MODE", "1")
    blk = _block(QKV, Ls, dev)
    group = blk.q_proj.__dict__["_siblings"]
    need = 3 * ((48 * I * 2 + 255) // 256 * 256)        # the largest routed token count: 48
    assert group._batched_workspace_bytes()[2] == need
    s = _stream_without_a_workspace(dev)
    key = (blk.q_proj._descriptor().device_index, s.cuda_stream)
    assert key not in B._GEMV_WS
    vptq_amd.prepare_model(blk, s)
    assert key in B._GEMV_WS and B._GEMV_WS[key].numel() >= need
    _, xt = _x(I, tokens, "f16", 2, dev)
    xt = xt.reshape(1, tokens, I)
    eager, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == [ENTRY]
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ys, calls = _spied(lambda: blk(xt), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert calls == [ENTRY], calls          # the captured step keeps the group's route
    g.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, eager))
    # a capture on a stream whose workspace was not sized: the op answers None, nothing is launched or allocated
    descs, caches = group._batched_plan()
    s2 = _stream_without_a_workspace(dev)
    key2 = (key[0], s2.cuda_stream)
    g2 = torch.cuda.CUDAGraph()
    s2.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s2):
        with torch.cuda.graph(g2, stream=s2):
            doubled = xt * 2                                           # (so that the graph is not empty)
            got, calls = _spied(lambda: ops.quant_gemm_k256_grouped(xt, descs, outs), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s2)
    assert got is None and calls == [] and key2 not in B._GEMV_WS
