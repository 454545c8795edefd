"""vptq_quant_gemm_gatherx_grouped (gemm_gatherx_grouped.hip): 1 - 16 tokens of 2 - 4 sibling layers of gemm_gatherx's formats in ONE
launch, one x[perm] gather per distinct permutation - on the GPU.  Modelled on tests/test_gemm_gather_grouped_gpu.py.

The contract is BITS: a row group of 16 outputs depends neither on the grid nor on the workgroup that runs it, so member m's y equals,
bit for bit, what the member's own entry gives on the same descriptor and x - vptq_quant_gemm_gather_px for a member with a
permutation, vptq_quant_gemm_gatherx for one without.  That comparison is the parent's code.  No tolerance, no row left out.

TILE = 1024 columns per tile and 16 outputs per row group (V = 8: two vector-rows, V = 16: one) are tests/test_gemm_gatherx_gpu.py's,
as are the layer recipes.  Formats by what the kernel's paths depend on: v16-k65536-0 (T = 16, no table), v16-k65536-1024 (T = 26,
table in LDS - re-staged at a member switch), v16-k65536-65536 (T = 32, table from L2), v16-k65536-32768 (T = 31, the 9-word
window), v8-k65536-4096 (T = 28), v8-k32768-0 (T = 15), and v8-k65536-4 (T = 18: V = 8 with a table in LDS, so that all 12 instantiations
run).  Columns 8, 64, TILE + 8 and 2 TILE + 264, member outputs from {4, 12, 20, 36} (ragged last vector-rows of V = 8 and V = 16),
tokens 1 / 5 / 15 / 16.

  1. bits: every member, 16-bit and fp32 outputs, groups of 2 / 3 / 4, every permutation case; one row per (format, dtype) against
     the float64 model of the single-layer test
  2. a member switch inside a workgroup: more row groups than the grid, members with different residual tables, scales and biases
  3. weights: one-hot activations read vptq_dequant's bits for every member
  4. placement: every operand in an arena of its own, guarded y, the workspace exactly the query's bytes at 16-byte alignment
  5. workspace contents; graph capture of the entry, replayed on new activations
  6. the module: link_siblings, leader / followers, a compacted member, the knob at 0, prepare_model + capture"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import GUARD, SENTINEL, F32
from test_gemm_gatherx_gpu import call, FMT, BITS, TILE
from test_gemm_gather_px_gpu import px_call, _stream_without_a_workspace
from test_gemm_gatherw_gpu import _bits
from test_gemm_gather_grouped_gpu import group_descs, distinct_perms, _x, _Block, QKV, GU, G1, COLS16, HOSTILE_OFFSETS, PX_THREADS, PX_TOK
from test_gemm_gatherx_grouped_cpu import inner
import _arena as ar
import _arith_model as am
from _gpu_util import spec_to_module, module_desc

pytestmark = pytest.mark.gpu

ENTRY = "vptq_quant_gemm_gatherx_grouped"
FMTS = ("v16-k65536-0", "v16-k65536-1024", "v16-k65536-65536", "v16-k65536-32768", "v8-k65536-4096", "v8-k32768-0", "v8-k65536-4")
RES = {"v16-k65536-0": 0, "v16-k65536-1024": 1, "v16-k65536-65536": 2, "v16-k65536-32768": 2, "v8-k65536-4096": 2, "v8-k32768-0": 0, "v8-k65536-4": 1}
WGCU = {f: (2 if f == "v16-k65536-1024" else 4) for f in FMTS}   # 32 KiB tile + a 32 KiB table: two workgroups per CU; else four
GS = (8, 64, TILE + 8, 2 * TILE + 264)
OUTS = (4, 12, 20, 36)
TOKS = (1, 5, 15, 16)
PERM_CASES = ("shared", "distinct", "mixed", "none")
LAUNCHES = (ENTRY, "vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gatherw_grouped", "vptq_quant_gemm_gather_px", "vptq_quant_gemm_gatherw",
            "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx", "vptq_quant_gemv", "vptq_quant_gemv_grouped", "vptq_dequant")


def make_group(G, outs, fmt, dt, perms, bias=1):
    """-> [LayerSpec]: members of one format and different seeds (their tables, scales and biases differ); perms: "shared" - every
    member has the first member's permutation, "distinct" - its own, "mixed" - every other member has one (the first member's), "none\""""
    from oracle import vptq_oracle as vo
    v, k, kr = FMT[fmt]
    Ls, shared = [], None
    for i, O in enumerate(outs):
        has = perms in ("shared", "distinct") or (perms == "mixed" and i % 2 == 0)
        # (test_gemm_gatherx_gpu.layer's recipe with a seed per member; member 1 has no output bias)
        L = vo.make_layer(G, O, dist="llm", seed=G + O + BITS[fmt] + 1000 * i, dtype=dt, vector_len=v, num_centroids=k, num_res_centroids=kr,
                          enable_perm=has, bias=bool(bias) and i != 1, enable_norm=True)
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


def expect_instance(descs, ds, Ls, tokens, fmt):
    from vptq_amd import _backend as B
    n, G = len(ds), Ls[0].in_features
    assert getattr(B.lib(), ENTRY + "_supported")(descs, n, tokens) == 1
    assert all(d.index_bits + d.res_bits == BITS[fmt] and d.vector_len == FMT[fmt][0] for d in ds)
    k = distinct_perms(ds)
    need = k * ((tokens * G * 2 + 255) // 256 * 256)
    assert getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens) == need
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    head = "none" if k == 0 else \
        f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK} perms={k}"
    want = f"{head} | {inner(ds, tokens, cus)}"
    text = instance(descs, n, tokens)
    assert text == want, (text, want)
    assert f" res={('none', 'lds', 'l2')[RES[fmt]]} " in text and f" wgcu={WGCU[fmt]} " in text
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


def own_entry(d, xt, O, out_f32=False):
    """the member's own entry on the same descriptor and x: the comparison (the parent's code)"""
    return px_call(d, xt, O, out_f32=out_f32) if d.perm else call(d, xt, O, out_f32=out_f32)


def assert_own_bits(ys, ds, xt, outs, f32):
    for m, (y, d, O) in enumerate(zip(ys, ds, outs)):
        assert not bool(torch.isnan(y).any()), m
        want = own_entry(d, xt, O, out_f32=f32)
        assert torch.equal(_bits(y), _bits(want)), f"member {m}: {int((_bits(y) != _bits(want)).sum())} of {y.numel()} outputs differ from its own entry"


# ---------------------------------------------------------------------------------------------- 1. bits and sums
def _bit_rows():
    rows, modelled = [], set()
    for i, (G, fmt, case) in enumerate(itertools.product(GS, FMTS, PERM_CASES)):
        # 112 rows: every (columns, format, permutation case); members, token count, dtype and bias advance at strides of their own.
        # GUARANTEED (tests/test_gemm_gatherx_grouped_cpu.py asserts them: the check needs no device): every (format, dtype) - hence every (V, RES, dtype) -, (format, permutation case),
        # (group size, permutation case) and (columns, tokens) pair, every member output for both vector lengths, both bias settings
        n = (2, 3, 4)[(i + i // 3) % 3]
        outs = tuple(OUTS[(i + j) % 4] for j in range(n))
        dt = ("f16", "bf16")[(i + i // 4 + i // 24) % 2]
        model = (fmt, dt) not in modelled   # one row per (format, dtype) is also held to the float64 model
        modelled.add((fmt, dt))
        rows.append(pytest.param(dict(G=G, fmt=fmt, case=case, outs=outs, tokens=TOKS[(i + i // 4) % 4], dt=dt, bias=(i // 2) % 2, model=model),
                                 id=f"G{G}-{fmt}-{case}-n{n}-i{i}"))
    return rows


@pytest.mark.parametrize("e", _bit_rows())
def test_bits_equal_every_members_own_entry(e, dev):
    G, fmt, tokens, outs = e["G"], e["fmt"], e["tokens"], e["outs"]
    Ls = make_group(G, outs, fmt, e["dt"], e["case"], bias=e["bias"])
    descs, ds, ms, keep = group_descs(Ls, dev)
    want_perms = {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[e["case"]]
    assert distinct_perms(ds) == want_perms and [bool(d.perm) for d in ds] == [L.perm is not None for L in Ls]
    expect_instance(descs, ds, Ls, tokens, fmt)
    x, xt = _x(G, tokens, e["dt"], G + tokens, dev)
    out = {}
    for f32 in (False, True):
        out[f32] = grouped_call(descs, len(ds), xt, outs, out_f32=f32)
        assert_own_bits(out[f32], ds, xt, outs, f32)
    if e["model"]:
        for m, L in enumerate(Ls):
            mm, aa = am.model(am.pieces(L), x, arith="exact")
            am.check_both(_np(out[False][m]), _np(out[True][m]), mm, aa, L.dtype, what=f"member {m} of {instance(descs, len(ds), tokens)}")


# ---------------------------------------------------------------------------------------------- 2. a member switch inside a workgroup
def _switch_outs(walk, slots):
    """member outputs at 64 columns over a grid of `slots` = CUs x wgcu workgroups.  "ends": slots - 324 (at least 100) + 301 + 100 row
    groups - the grid ends inside member 1, the first workgroups go from member 0 to member 2.  "three": 40 + (slots + 77) + (slots -
    24) row groups - workgroups 0 .. 39 walk g, g + slots, g + 2 slots through members 0, 1 and 2 (two CONSECUTIVE switches each, a
    table in LDS re-staged twice), the others switch from member 1 to member 2"""
    if walk == "ends":
        return (16 * max(100, slots - 324), 16 * 300 + 4, 16 * 100), 2
    return (16 * 40, 16 * (slots + 76) + 4, 16 * (slots - 24)), 3


@pytest.mark.parametrize("walk", ["ends", "three"])
@pytest.mark.parametrize("fmt,dt,case", [("v16-k65536-1024", "f16", "none"), ("v16-k65536-1024", "bf16", "shared"), ("v8-k65536-4", "f16", "mixed"),
                                         ("v8-k32768-0", "bf16", "mixed"), ("v16-k65536-32768", "f16", "distinct")])
def test_member_switch_inside_a_workgroup_keeps_every_members_bits(fmt, dt, case, walk, dev):
    """more row groups than workgroups: a workgroup walks row groups of several members, with another residual table (RES = 1: in LDS,
    re-staged at the switch - v16-k65536-1024's 32 KiB and v8-k65536-4's 64 bytes), other scales and biases in each"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    v, _, kr = FMT[fmt]
    wgcu = 2 if fmt == "v16-k65536-1024" else 4
    slots = cus * wgcu
    outs, rgs = _switch_outs(walk, slots)
    G, tokens = 64, 15
    Ls = make_group(G, outs, fmt, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    rows = 16 // v
    groups = [(L.num_indices + rows - 1) // rows for L in Ls]
    first = [0, groups[0], groups[0] + groups[1], sum(groups)]
    member = lambda g: max(m for m in range(3) if first[m] <= g)
    walks = {tuple(sorted({member(g) for g in range(w, first[3], slots)})) for w in range(slots)}
    assert sum(groups) > slots and groups[0] < slots, "the grid must end inside the member list"
    assert ({(0, 2)} if walk == "ends" else {(0, 1, 2), (1, 2)}) <= walks, walks
    if kr:
        tabs = [np.asarray(L.res_centroids) for L in Ls]
        assert not np.array_equal(tabs[0], tabs[1]) and not np.array_equal(tabs[1], tabs[2])
    assert not np.array_equal(np.asarray(Ls[0].weight_scale), np.asarray(Ls[1].weight_scale))
    text = instance(descs, 3, tokens)
    assert f"wgcu={wgcu} grid={slots} rgs={rgs}" in text and f"groups={'+'.join(map(str, groups))}" in text, text
    assert (" res=lds " in text) == (fmt in ("v16-k65536-1024", "v8-k65536-4"))
    x, xt = _x(G, tokens, dt, 7, dev)
    for f32 in (False, True):
        assert_own_bits(grouped_call(descs, 3, xt, outs, out_f32=f32), ds, xt, outs, f32)
    # two launches give the same bits
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 3, xt, outs), grouped_call(descs, 3, xt, outs)))


# ---------------------------------------------------------------------------------------------- 3. weights bit for bit
@pytest.mark.parametrize("fmt,dt,case", [("v16-k65536-1024", "f16", "distinct"), ("v8-k32768-0", "bf16", "mixed"), ("v16-k65536-65536", "bf16", "shared"),
                                         ("v16-k65536-32768", "f16", "none"), ("v8-k65536-4096", "f16", "shared"), ("v16-k65536-0", "bf16", "none")])
def test_one_hot_activations_read_dequant_bits_for_every_member(fmt, dt, case, dev):
    outs = (20, 36, 12)
    Ls = make_group(G1, outs, fmt, dt, case, bias=0)          # (no output bias: y is a column of W)
    descs, ds, ms, keep = group_descs(Ls, dev)
    x = torch.zeros(16, G1, dtype=ms[0].centroids.weight.dtype, device=dev)
    x[torch.arange(16), torch.tensor(COLS16)] = 1.0           # input feature j: it reaches stored column c with perm[c] == j
    ys = grouped_call(descs, 3, x, outs)
    for m, (y, mod) in enumerate(zip(ys, ms)):
        want = mod.dequant()[:, torch.tensor(COLS16, device=dev)].t()
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
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, len(ds), tokens)
    assert need == distinct_perms(ds) * ((tokens * Ls[0].in_features * 2 + 255) // 256 * 256) > 0
    ws, wa = ar.guarded_workspace(need, False, dev, align=16)
    assert ws.numel() == need and ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 != 0
    yp = (C.c_void_p * len(ds))(*[y.data_ptr() for y, _ in outs_placed])
    B.check(getattr(B.lib(), ENTRY)(descs, len(ds), xv.data_ptr(), yp, tokens, F32 if f32 else 0, ws.data_ptr(), need,
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


@pytest.mark.parametrize("fmt,dt,G,tokens", [("v16-k65536-1024", "f16", TILE + 8, 5), ("v16-k65536-65536", "bf16", 2 * TILE + 264, 16),
                                             ("v8-k32768-0", "f16", 64, 15), ("v16-k65536-32768", "bf16", TILE + 8, 16)])
def test_same_bits_under_every_placement(fmt, dt, G, tokens, dev):
    outs = (20, 4, 36)
    Ls = make_group(G, outs, fmt, dt, "distinct")      # (three x gathers: three blocks of the workspace)
    _, xt = _x(G, tokens, dt, 3, dev)
    for f32 in (False, True):
        benign = _placed_call(Ls, xt, tokens, outs, ar.BENIGN, {}, 0, 0, f32, dev)
        hostile = _placed_call(Ls, xt, tokens, outs, ar.HOSTILE, HOSTILE_OFFSETS, 16, 4 if f32 else 2, f32, dev)
        descs, ds, ms, keep = group_descs(Ls, dev)
        for m, (a, b, d, O) in enumerate(zip(benign, hostile, ds, outs)):
            assert torch.equal(_bits(a), _bits(b)), m
            assert torch.equal(_bits(a), _bits(own_entry(d, xt, O, out_f32=f32))), m   # torch's allocator: the own entry's bits


# ---------------------------------------------------------------------------------------------- 5. workspace, capture
@pytest.mark.parametrize("fmt,dt", [("v16-k65536-1024", "f16"), ("v8-k65536-4096", "bf16")])
def test_workspace_contents_do_not_matter_and_calls_share_it(fmt, dt, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (12, 36)
    Ls = make_group(G, outs, fmt, dt, "distinct")
    descs, ds, ms, keep = group_descs(Ls, dev)
    _, x16 = _x(G, 16, dt, 5, dev)
    _, x5 = _x(G, 5, dt, 6, dev)
    fresh16, fresh5 = grouped_call(descs, 2, x16, outs), grouped_call(descs, 2, x5, outs)
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, 2, 16)
    for pattern in (0x7E00, 0x7FC0, 0xFFFF, 0):   # NaN patterns of both dtypes, 0xFF bytes, zeros
        ws = torch.full((need // 2,), pattern - (1 << 16) if pattern >= 1 << 15 else pattern, dtype=torch.int16, device=dev).view(torch.uint8)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 2, x16, outs, ws=ws), fresh16)), hex(pattern)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=dev)
    for xt, fresh in ((x16, fresh16), (x5, fresh5), (x16, fresh16)):   # 16 tokens, then 5 through the SAME (larger) workspace
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grouped_call(descs, 2, xt, outs, ws=ws), fresh))
    # the workspace holds x[:, perm_m] of the last call, one block per distinct permutation in member order
    block = need // 2
    for m, L in enumerate(Ls):
        xp = x16[:, torch.from_numpy(L.perm.astype(np.int64)).to(dev)]
        assert torch.equal(ws[m * block:m * block + 16 * G * 2].view(torch.int16).reshape(16, G), xp.contiguous().view(torch.int16))


@pytest.mark.parametrize("fmt,dt,case,tokens", [("v16-k65536-1024", "f16", "mixed", 12), ("v16-k65536-65536", "bf16", "distinct", 16),
                                                ("v8-k32768-0", "f16", "none", 5)])
def test_a_captured_call_replays_on_new_activations(fmt, dt, case, tokens, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (20, 36, 12)
    Ls = make_group(G, outs, fmt, dt, case)
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
            B.check(getattr(B.lib(), ENTRY)(descs, 3, xg.data_ptr(), yp, tokens, 0, ws.data_ptr() if need else None, need,
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


def _block(names, Ls, dev, link=True):
    from vptq_amd.layers import link_siblings
    blk = _Block(names, [spec_to_module(L, dev) for L in Ls])
    if link:
        assert link_siblings(blk) == 1
    return blk


def _spied(fn, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    try:
        y = fn()
    finally:
        monkeypatch.setattr(B, "lib", lambda: real)
    return y, calls


@pytest.mark.parametrize("names,outs,fmt,dt,case,tokens", [(QKV, (512, 128, 132), "v16-k65536-1024", "f16", "shared", 16),
                                                           (GU, (264, 260), "v16-k65536-65536", "bf16", "none", 5),
                                                           (QKV, (128, 512, 136), "v8-k32768-0", "bf16", "mixed", 9),
                                                           (GU, (260, 264), "v8-k65536-4096", "f16", "distinct", 12)])
def test_linked_siblings_take_one_grouped_launch_with_their_own_bits(names, outs, fmt, dt, case, tokens, dev, monkeypatch):
    from vptq_amd import grouped_decode as gd
    I = 2048
    v, k, kr = FMT[fmt]
    Ls = make_group(I, outs, fmt, dt, case)
    x, xt = _x(I, tokens, dt, 9, dev)
    xt = xt.reshape(1, tokens, I)
    twins = _block(names, Ls, dev, link=False)
    # the committed cells never hold a group this small: the routes of before, no grouped launch - linked or not
    assert not gd.gemm_gatherx_grouped_route(v, k, kr, outs, I, tokens, {"shared": True, "distinct": True, "none": False, "mixed": None}[case])
    y_today, today = _spied(lambda: twins(xt), monkeypatch)
    assert ENTRY not in today and len(today) >= len(outs)
    y_linked, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y_linked, y_today))
    # the knob on: ONE grouped launch, the followers pick their outputs up, every member has the bits of its un-linked twin's own entry
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "1")
    blk = _block(names, Ls, dev)
    ys, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == [ENTRY], calls
    group = blk.__dict__["_modules"][names[0]].__dict__["_siblings"]
    assert group._bx is None and not group._bout
    descs, caches = group._batched_plan()
    assert distinct_perms([descs[i] for i in range(len(outs))]) == {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[case]
    for m, (y, n, L, O) in enumerate(zip(ys, names, Ls, outs)):
        d, keep = module_desc(getattr(twins, n))
        want = own_entry(d, xt.reshape(tokens, I), O)
        assert y.shape == (1, tokens, O) and torch.equal(_bits(y.reshape(tokens, O)), _bits(want)), m
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
    # the knob at 0: the routes and the bits of before
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "0")
    y0s, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y0s, y_today))


def test_a_compacted_member_makes_the_group_step_aside(dev, monkeypatch):
    from vptq_amd import grouped_decode as gd
    I, outs, tokens = 2048, (512, 128, 132), 8
    Ls = make_group(I, outs, "v16-k65536-0", "f16", "shared")      # (v16-k65536-0 has exact sliced layouts: it can be compacted)
    _, xt = _x(I, tokens, "f16", 4, dev)
    xt = xt.reshape(1, tokens, I)
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "1")
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
    I, outs, tokens = 2 * TILE + 264, (36, 20, 12), 16
    Ls = make_group(I, outs, "v16-k65536-1024", "f16", "distinct")
    monkeypatch.setattr(gd, "_GEMM_GATHERX_GROUPED_MODE", "1")
    blk = _block(QKV, Ls, dev)
    group = blk.q_proj.__dict__["_siblings"]
    need = 3 * ((16 * I * 2 + 255) // 256 * 256)
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
            got, calls = _spied(lambda: ops.quant_gemm_gatherx_grouped(xt, descs, outs), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s2)
    assert got is None and calls == [] and key2 not in B._GEMV_WS
    # ... and the op answers None for a group the library does not serve
    mixed = (B.LayerDesc * 2)(descs[0], module_desc(spec_to_module(make_group(I, (36,), "v16-k65536-0", "f16", "none")[0], dev))[0])
    assert ops.quant_gemm_gatherx_grouped(xt, mixed, (36, 36)) is None
