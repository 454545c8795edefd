"""vptq_quant_gemm_gatherw_grouped (gemm_gatherw_grouped.hip): 17 - 48 tokens of 2 - 4 sibling layers of the large-codebook formats in
ONE launch, one x[perm] gather per distinct permutation - on the GPU.

The contract is BITS: a row group of 16 outputs does not depend on the grid, so member m's y equals, bit for bit, what the member's
own entry gives on the same descriptor and x at the same token count - vptq_quant_gemm_gather_px for a member with a permutation,
vptq_quant_gemm_gatherw for one without.  That comparison is the parent's code.

TILE = 1024 columns per tile and R = 2 vector-rows (16 outputs) per row group are the kernel's.  Columns 8, 64, TILE + 8 and
2 TILE + 264, member outputs from {4, 12, 20, 36} (partial row groups, an odd last vector-row), tokens 17 / 31 / 32 / 33 / 48: one live
token in block 1 and in block 2, and full blocks.

  1. bits: every member, 16-bit and fp32 outputs, groups of 2 / 3 / 4, every permutation case; every row against the float64 model
  2. a member switch inside a workgroup: more row groups than the grid, members with different residual tables, scales and biases
  3. weights: one-hot activations read vptq_dequant's bits for every member, at 17 and 48 tokens
  4. placement: every operand in an arena of its own, guarded y, the workspace exactly the query's bytes at 16-byte alignment
  5. the workspace's contents do not matter; graph capture of the entry, replayed on new activations
  6. the module: link_siblings at 17 / 48 tokens, 16 tokens on the first-window entry, a compacted member, prepare_model + capture"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import KR, TILE, R, GUARD, SENTINEL, F32
from test_gemm_gather_px_gpu import px_call, _stream_without_a_workspace
from test_gemm_gatherw_gpu import call as call_w, COLS1 as COLS48, _bits
from test_gemm_gather_grouped_gpu import (make_group, group_descs, distinct_perms, _x, _switch_outs, _block, _Block, HOSTILE_OFFSETS, PX_THREADS,  # noqa: F401
                                          PX_TOK, GS, OUTS, PERM_CASES, QKV, GU, G1)
import _arena as ar
import _arith_model as am
from _gpu_util import spec_to_module, module_desc

pytestmark = pytest.mark.gpu

ENTRY = "vptq_quant_gemm_gatherw_grouped"
TOKS = (17, 31, 32, 33, 48)
LAUNCHES = (ENTRY, "vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gather_px", "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather",
            "vptq_quant_gemm_gatherx", "vptq_quant_gemv", "vptq_quant_gemv_grouped", "vptq_dequant")


def instance(descs, n, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(320)
    B.check(B.lib().vptq_quant_gemm_gatherw_grouped_instance(descs, n, tokens, 0, buf, len(buf)), ENTRY + "_instance")
    return buf.value.decode()


def expect_instance(descs, ds, Ls, tokens, T):
    from vptq_amd import _backend as B
    n, G = len(ds), Ls[0].in_features
    assert B.lib().vptq_quant_gemm_gatherw_grouped_supported(descs, n, tokens) == 1
    k = distinct_perms(ds)
    need = k * ((tokens * G * 2 + 255) // 256 * 256)
    assert B.lib().vptq_quant_gemm_gatherw_grouped_workspace_bytes(descs, n, tokens) == need
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = [(L.num_indices + R - 1) // R for L in Ls]
    grid = min(sum(groups), 4 * cus)
    head = "none" if k == 0 else \
        f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK} perms={k}"
    want = (f"{head} | gemm_gatherw_grouped dt={Ls[0].dtype} t={T} tok={tokens} tb={(tokens + 15) // 16} n={n} groups={'+'.join(map(str, groups))} "
            f"tiles={(G + TILE - 1) // TILE} grid={grid} rgs={(sum(groups) + grid - 1) // grid}")
    text = instance(descs, n, tokens)
    assert text == want, (text, want)
    return need


def grouped_call(descs, n, xt, outs, out_f32=False, ws=None):
    """the entry with every y's token rows NaN between guard rows and a workspace of EXACTLY the query's bytes (0xFF bytes unless one
    is handed in); -> [y_m [tokens, O_m]] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = B.lib().vptq_quant_gemm_gatherw_grouped_workspace_bytes(descs, n, tokens)
    if ws is None and need:
        ws = torch.full((need,), 255, dtype=torch.uint8, device=xt.device)
    bufs = [torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device) for O in outs]
    for b in bufs:
        b[GUARD:GUARD + tokens] = float("nan")
    ys = [b[GUARD:GUARD + tokens] for b in bufs]
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    B.check(B.lib().vptq_quant_gemm_gatherw_grouped(descs, n, xt.data_ptr(), yp, tokens, F32 if out_f32 else 0, None if ws is None else ws.data_ptr(),
                                                    0 if ws is None else ws.numel(), B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return [y.clone() for y in ys]


def own_entry(d, xt, O, out_f32=False):
    """the member's own entry on the same descriptor and x: the comparison (the parent's code)"""
    return px_call(d, xt, O, out_f32=out_f32) if d.perm else call_w(d, xt, O, out_f32=out_f32)


# ---------------------------------------------------------------------------------------------- 1. bits and sums
def _bit_rows():
    rows = []
    for i, (G, T, case) in enumerate(itertools.product(GS, (16, 24, 32), PERM_CASES)):
        # 48 rows: every (columns, T, permutation case); members, token count, dtype and bias advance at strides of their own.
        # GUARANTEED (the test below asserts them): every (T, dtype, token blocks) - the 12 instantiations -, every (T, permutation
        # case), (group size, permutation case) and (columns, tokens) pair, and every member output.  NOT guaranteed: triples beyond
        # those; the kernel's paths depend on (DT, T, TB) and on columns / tokens separately
        n = (2, 3, 4)[(i + i // 3) % 3]
        outs = tuple(OUTS[(i + j) % 4] for j in range(n))
        rows.append(pytest.param(dict(G=G, T=T, case=case, outs=outs, tokens=TOKS[(i + i // 12) % 5], dt=("f16", "bf16")[(i + i // 12 + i // 4) % 2],
                                      bias=(i // 2) % 2), id=f"G{G}-t{T}-{case}-n{n}-i{i}"))
    return rows


def test_the_bit_rows_cover_every_instantiation_group_size_and_permutation_case():
    rows = [e.values[0] for e in _bit_rows()]
    assert {(e["T"], e["dt"], (e["tokens"] + 15) // 16) for e in rows} == set(itertools.product((16, 24, 32), ("f16", "bf16"), (2, 3)))
    assert {(e["T"], e["case"]) for e in rows} == set(itertools.product((16, 24, 32), PERM_CASES))
    assert {(len(e["outs"]), e["case"]) for e in rows} == set(itertools.product((2, 3, 4), PERM_CASES))
    assert {(e["G"], e["tokens"]) for e in rows} == set(itertools.product(GS, TOKS))
    assert {o for e in rows for o in e["outs"]} == set(OUTS)


@pytest.mark.parametrize("e", _bit_rows())
def test_bits_equal_every_members_own_entry_and_sums_hold_the_model(e, dev):
    G, T, tokens, outs = e["G"], e["T"], e["tokens"], e["outs"]
    Ls = make_group(G, outs, T, e["dt"], e["case"], bias=e["bias"])
    descs, ds, ms, keep = group_descs(Ls, dev)
    want_perms = {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[e["case"]]
    assert distinct_perms(ds) == want_perms and [bool(d.perm) for d in ds] == [L.perm is not None for L in Ls]
    expect_instance(descs, ds, Ls, tokens, T)
    x, xt = _x(G, tokens, e["dt"], G + tokens, dev)
    out = {}
    for f32 in (False, True):   # (VPTQ_GEMV_OUT_F32: bit-equal to the own entry's fp32 sums)
        ys = grouped_call(descs, len(ds), xt, outs, out_f32=f32)
        for m, (y, d, O) in enumerate(zip(ys, ds, outs)):
            assert not bool(torch.isnan(y).any()), m
            want = own_entry(d, xt, O, out_f32=f32)
            assert torch.equal(_bits(y), _bits(want)), f"member {m}: {int((_bits(y) != _bits(want)).sum())} of {y.numel()} outputs differ from its own entry"
        out[f32] = ys
    for m, L in enumerate(Ls):
        mm, aa = am.model(am.pieces(L), x, arith="exact")
        am.check_both(_np(out[False][m]), _np(out[True][m]), mm, aa, L.dtype, what=f"member {m} of {instance(descs, len(ds), tokens)}")


# ---------------------------------------------------------------------------------------------- 2. a member switch inside a workgroup
@pytest.mark.parametrize("walk", ["ends", "three"])
@pytest.mark.parametrize("T,dt,case,tokens", [(24, "f16", "none", 33), (24, "bf16", "shared", 17), (16, "bf16", "mixed", 48), (32, "f16", "distinct", 32)])
def test_member_switch_inside_a_workgroup_keeps_every_members_bits(T, dt, case, tokens, walk, dev):
    """more row groups than workgroups: a workgroup walks row groups of several members, with another residual table (T = 24: in
    LDS, re-staged at the switch), other scales and biases in each, and its per-block x offsets recomputed from the member's x"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    outs, rgs = _switch_outs(walk, cus)
    G = 64
    Ls = make_group(G, outs, T, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    groups = [(L.num_indices + R - 1) // R for L in Ls]
    first = [0, groups[0], groups[0] + groups[1], sum(groups)]
    member = lambda g: max(m for m in range(3) if first[m] <= g)
    walks = {tuple(sorted({member(g) for g in range(w, first[3], 4 * cus)})) for w in range(4 * cus)}
    assert sum(groups) > 4 * cus and groups[0] < 4 * cus, "the grid must end inside the member list"
    assert ({(0, 2)} if walk == "ends" else {(0, 1, 2), (1, 2)}) <= walks, walks
    if T > 16:
        tabs = [np.asarray(L.res_centroids) for L in Ls]
        assert not np.array_equal(tabs[0], tabs[1]) and not np.array_equal(tabs[1], tabs[2])
    assert not np.array_equal(np.asarray(Ls[0].weight_scale), np.asarray(Ls[1].weight_scale))
    text = instance(descs, 3, tokens)
    assert f"grid={4 * cus} rgs={rgs}" in text and f"groups={'+'.join(map(str, groups))}" in text, text
    x, xt = _x(G, tokens, dt, 7, dev)
    for f32 in (False, True):
        ys = grouped_call(descs, 3, xt, outs, out_f32=f32)
        for m, (y, d, O) in enumerate(zip(ys, ds, outs)):
            want = own_entry(d, xt, O, out_f32=f32)
            assert not bool(torch.isnan(y).any()), m
            assert torch.equal(_bits(y), _bits(want)), f"member {m}: {int((_bits(y) != _bits(want)).sum())} of {y.numel()} outputs differ"
    # two launches give the same bits
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 3, xt, outs), grouped_call(descs, 3, xt, outs)))


# ---------------------------------------------------------------------------------------------- 3. weights bit for bit
@pytest.mark.parametrize("tokens", [17, 48])
@pytest.mark.parametrize("T,dt,case", [(24, "f16", "distinct"), (16, "bf16", "mixed"), (32, "bf16", "shared"), (24, "bf16", "none")])
def test_one_hot_activations_read_dequant_bits_for_every_member(T, dt, case, tokens, dev):
    outs = (20, 36, 12)
    Ls = make_group(G1, outs, T, dt, case, bias=0)          # (no output bias: y is a column of W)
    descs, ds, ms, keep = group_descs(Ls, dev)
    cols = COLS48[:tokens]                                   # (17: one live token in block 1)
    assert len(set(cols)) == tokens
    x = torch.zeros(tokens, G1, dtype=ms[0].centroids.weight.dtype, device=dev)
    x[torch.arange(tokens), torch.tensor(cols)] = 1.0        # input feature j: it reaches stored column c with perm[c] == j
    ys = grouped_call(descs, 3, x, outs)
    for m, (y, mod) in enumerate(zip(ys, ms)):
        want = mod.dequant()[:, torch.tensor(cols, device=dev)].t()
        assert not bool(torch.isnan(y).any())
        assert bool((y == want).all()), f"member {m}: {int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 4. placement
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
    need = B.lib().vptq_quant_gemm_gatherw_grouped_workspace_bytes(descs, len(ds), tokens)
    assert need == distinct_perms(ds) * ((tokens * Ls[0].in_features * 2 + 255) // 256 * 256) > 0
    ws, wa = ar.guarded_workspace(need, False, dev, align=16)
    assert ws.numel() == need and ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 != 0
    yp = (C.c_void_p * len(ds))(*[y.data_ptr() for y, _ in outs_placed])
    B.check(B.lib().vptq_quant_gemm_gatherw_grouped(descs, len(ds), xv.data_ptr(), yp, tokens, F32 if f32 else 0, ws.data_ptr(), need,
                                                    B.current_stream_ptr(dev)), ENTRY)
    torch.cuda.synchronize(dev)
    for name, a in list(arenas.items()) + [("x", xa)]:
        assert a.intact(), (name, a.damage())                    # the inputs' margins
    for i, (y, ya) in enumerate(outs_placed):
        assert ya.intact(), (f"y[{i}]", ya.damage())             # a store outside y
        assert not bool(torch.isnan(y).any())
    assert wa.intact(), ("workspace", wa.damage())               # a store outside the query's bytes
    assert torch.equal(xv, xt)
    return [y.clone() for y, _ in outs_placed]


@pytest.mark.parametrize("T,dt,G,tokens", [(24, "f16", TILE + 8, 17), (32, "bf16", 2 * TILE + 264, 48), (16, "f16", 64, 33)])
def test_same_bits_under_every_placement(T, dt, G, tokens, dev):
    outs = (20, 4, 36)
    Ls = make_group(G, outs, T, dt, "distinct")      # (three x gathers: three blocks of the workspace)
    _, xt = _x(G, tokens, dt, 3, dev)
    for f32 in (False, True):
        benign = _placed_call(Ls, xt, tokens, outs, ar.BENIGN, {}, 0, 0, f32, dev)
        hostile = _placed_call(Ls, xt, tokens, outs, ar.HOSTILE, HOSTILE_OFFSETS, 16, 4 if f32 else 2, f32, dev)
        descs, ds, ms, keep = group_descs(Ls, dev)
        for m, (a, b, d, O) in enumerate(zip(benign, hostile, ds, outs)):
            assert torch.equal(_bits(a), _bits(b)), m
            assert torch.equal(_bits(a), _bits(own_entry(d, xt, O, out_f32=f32))), m   # torch's allocator: the own entry's bits


# ---------------------------------------------------------------------------------------------- 5. workspace, capture
@pytest.mark.parametrize("T,dt", [(24, "f16"), (32, "bf16")])
def test_workspace_contents_do_not_matter_and_calls_share_it(T, dt, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (12, 36)
    Ls = make_group(G, outs, T, dt, "distinct")
    descs, ds, ms, keep = group_descs(Ls, dev)
    _, x48 = _x(G, 48, dt, 5, dev)
    _, x17 = _x(G, 17, dt, 6, dev)
    fresh48, fresh17 = grouped_call(descs, 2, x48, outs), grouped_call(descs, 2, x17, outs)
    need = B.lib().vptq_quant_gemm_gatherw_grouped_workspace_bytes(descs, 2, 48)
    for pattern in (0x7E00, 0x7FC0, 0xFFFF, 0):   # NaN patterns of both dtypes, 0xFF bytes, zeros
        ws = torch.full((need // 2,), pattern - (1 << 16) if pattern >= 1 << 15 else pattern, dtype=torch.int16, device=dev).view(torch.uint8)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 2, x48, outs, ws=ws), fresh48)), hex(pattern)
    # two groups (the same members in the other order, another token count) share one workspace on one stream
    rev = (B.LayerDesc * 2)(ds[1], ds[0])
    ws = torch.full((need,), 255, dtype=torch.uint8, device=dev)
    for xt, fresh in ((x48, fresh48), (x17, fresh17), (x48, fresh48)):
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 2, xt, outs, ws=ws), fresh))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(rev, 2, xt, outs[::-1], ws=ws), fresh[::-1]))
    # the workspace holds x[:, perm_m] of the last call, one block per distinct permutation in member order
    block = need // 2
    for m, L in enumerate(Ls[::-1]):
        xp = x48[:, torch.from_numpy(L.perm.astype(np.int64)).to(dev)]
        assert torch.equal(ws[m * block:m * block + 48 * G * 2].view(torch.int16).reshape(48, G), xp.contiguous().view(torch.int16))


@pytest.mark.parametrize("T,dt,case,tokens", [(24, "f16", "mixed", 33), (32, "bf16", "distinct", 48), (16, "f16", "none", 17)])
def test_a_captured_call_replays_on_new_activations(T, dt, case, tokens, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (20, 36, 12)
    Ls = make_group(G, outs, T, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    xs = [_x(G, tokens, dt, s, dev)[1] for s in (1, 2, 3)]
    eager = [grouped_call(descs, 3, x, outs) for x in xs]
    need = B.lib().vptq_quant_gemm_gatherw_grouped_workspace_bytes(descs, 3, tokens)
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
            B.check(B.lib().vptq_quant_gemm_gatherw_grouped(descs, 3, xg.data_ptr(), yp, tokens, 0, ws.data_ptr() if need else None, need,
                                                            B.current_stream_ptr(dev)), "capture")
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


@pytest.mark.parametrize("names,outs,T,dt,case,tokens", [(QKV, (512, 128, 132), 24, "f16", "shared", 17), (GU, (264, 260), 32, "bf16", "none", 48),
                                                         (QKV, (128, 512, 136), 16, "bf16", "mixed", 48), (GU, (260, 264), 24, "f16", "distinct", 17)])
def test_linked_siblings_take_one_grouped_launch_with_their_own_bits(names, outs, T, dt, case, tokens, dev, monkeypatch):
    from vptq_amd import grouped_decode as gd
    I = 2048
    Ls = make_group(I, outs, T, dt, case)
    x, xt = _x(I, tokens, dt, 9, dev)
    xt = xt.reshape(1, tokens, I)
    twins = _block(names, Ls, dev, link=False)
    # the committed cells never hold a group this small: the routes of before, no grouped launch - linked or not
    assert not gd.gemm_gatherw_grouped_route(8, 65536, KR[T], outs, I, tokens, {"shared": True, "distinct": True, "none": False, "mixed": None}[case])
    y_today, today = _spied(lambda: twins(xt), monkeypatch)
    assert ENTRY not in today and "vptq_quant_gemm_gather_grouped" not in today
    y_linked, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y_linked, y_today))
    # the knob on: ONE grouped launch, the followers pick their outputs up, every member has the bits of its un-linked twin's own entry
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    blk = _block(names, Ls, dev)
    ys, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == [ENTRY], calls
    group = blk.__dict__["_modules"][names[0]].__dict__["_siblings"]
    assert group._bx is None and not group._bout
    descs, caches = group._batched_plan(group._batched_route(tokens))
    assert distinct_perms([descs[i] for i in range(len(outs))]) == {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[case]
    for m, (y, n, L, O) in enumerate(zip(ys, names, Ls, outs)):
        d, keep = module_desc(getattr(twins, n))
        want = own_entry(d, xt.reshape(tokens, I), O)
        assert y.shape == (1, tokens, O) and torch.equal(_bits(y.reshape(tokens, O)), _bits(want)), m
        mm, aa = am.model(am.pieces(L), x, arith="exact")
        am.check_outputs(_np(y).reshape(mm.shape), mm, aa, dt, False, what=f"VQuantLinear.forward, {tokens} tokens, grouped, member {m}")
    # at 16 tokens the group still takes the first window's entry (its knob on), never the new one
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    _, x16 = _x(I, 16, dt, 10, dev)
    _, calls = _spied(lambda: blk(x16.reshape(1, 16, I)), monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_grouped"], calls
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "auto")
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
    # the knob at 0: the routes and the bits of before
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "0")
    y0s, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y0s, y_today))


def test_a_compacted_member_makes_the_group_step_aside(dev, monkeypatch):
    from vptq_amd import grouped_decode as gd
    I, outs, tokens = 2048, (512, 128, 132), 24
    Ls = make_group(I, outs, 24, "f16", "shared")
    _, xt = _x(I, tokens, "f16", 4, dev)
    xt = xt.reshape(1, tokens, I)
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    twins, blk = _block(QKV, Ls, dev, link=False), _block(QKV, Ls, dev)
    for b in (twins, blk):
        b.k_proj.compact(force=True)
        assert b.k_proj.is_compact()
    y_twins, before = _spied(lambda: twins(xt), monkeypatch)
    ys, calls = _spied(lambda: blk(xt), monkeypatch)
    assert ENTRY not in calls and calls == before, (calls, before)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, y_twins))
    # uncompacted again (a rebuilt descriptor): the group takes the call
    blk.k_proj.uncompact()
    ys2, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == [ENTRY], calls


def test_prepare_model_sizes_the_workspace_and_a_captured_step_keeps_the_group_route(dev, monkeypatch):
    import vptq_amd
    from vptq_amd import _backend as B, grouped_decode as gd, ops
    I, outs, tokens = 2 * TILE + 264, (36, 20, 12), 32
    Ls = make_group(I, outs, 24, "f16", "distinct")
    monkeypatch.setattr(gd, "_GEMM_GATHERW_GROUPED_MODE", "1")
    blk = _block(QKV, Ls, dev)
    group = blk.q_proj.__dict__["_siblings"]
    need = 3 * ((48 * I * 2 + 255) // 256 * 256)             # the largest routed token count of the wide record
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
    descs, caches = group._batched_plan(group._batched_route(tokens))
    s2 = _stream_without_a_workspace(dev)
    key2 = (key[0], s2.cuda_stream)
    g2 = torch.cuda.CUDAGraph()
    s2.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s2):
        with torch.cuda.graph(g2, stream=s2):
            doubled = xt * 2                                           # (so that the graph is not empty)
            got, calls = _spied(lambda: ops.quant_gemm_gatherw_grouped(xt, descs, outs), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s2)
    assert got is None and calls == [] and key2 not in B._GEMV_WS
