"""vptq_quant_gemm_gather_grouped (the grouped kernel of gemm_gather.hip): 1 - 16 tokens of 2 - 4 sibling layers in ONE launch, one
x[perm] gather per distinct permutation - on the GPU.

The contract is BITS: a row group of 16 outputs does not depend on the grid, so member m's y equals, bit for bit, what the member's
own entry gives on the same descriptor and x - vptq_quant_gemm_gather_px for a member with a permutation, vptq_quant_gemm_gather for
one without.  That comparison is the parent's code.

TILE = 1024 columns per tile and R = 2 vector-rows (16 outputs) per row group are the kernel's.  Columns 8, 64, TILE + 8 and
2 TILE + 264, member outputs from {4, 12, 20, 36} (an odd last vector-row lands in a row group), tokens 1 / 5 / 15 / 16.

  1. bits: every member, 16-bit and fp32 outputs, groups of 2 / 3 / 4, every permutation case; every row against the float64 model
  2. a member switch inside a workgroup: more row groups than the grid, members with different residual tables, scales and biases
  3. weights: one-hot activations read vptq_dequant's bits for every member
  4. placement: every operand in an arena of its own, guarded y, the workspace exactly the query's bytes at 16-byte alignment
  5. graph capture of the entry, replayed on new activations
  6. the module: link_siblings, leader / followers, an x rewritten in place, a compacted member, the knob at 0, prepare_model + capture"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import call, KR, TILE, R, GUARD, SENTINEL, F32
from test_gemm_gather_px_gpu import px_call, stripped, _stream_without_a_workspace
from test_gemm_gatherw_gpu import _bits
import _arena as ar
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu

PX_THREADS, PX_TOK = 64, 4
GS = (8, 64, TILE + 8, 2 * TILE + 264)
OUTS = (4, 12, 20, 36)
TOKS = (1, 5, 15, 16)
PERM_CASES = ("shared", "distinct", "mixed", "none")
LAUNCHES = ("vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gather_px", "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather",
            "vptq_quant_gemm_gatherx", "vptq_quant_gemv", "vptq_quant_gemv_grouped", "vptq_dequant")


def make_group(G, outs, T, dt, perms, bias=1):
    """-> [LayerSpec]: members of different seeds (their tables, scales and biases differ); perms: "shared" - every member has the
    first member's permutation, "distinct" - its own, "mixed" - every other member has one (the first member's), "none\""""
    from oracle import vptq_oracle as vo
    Ls, shared = [], None
    for i, O in enumerate(outs):
        has = perms in ("shared", "distinct") or (perms == "mixed" and i % 2 == 0)
        # (test_gemm_gather_gpu.layer's recipe with a seed per member; member 1 has no output bias)
        L = vo.make_layer(G, O, dist="llm", seed=G + O + T + 1000 * i, dtype=dt, vector_len=8, num_centroids=65536, num_res_centroids=KR[T],
                          enable_perm=has, bias=bool(bias) and i != 1, enable_norm=True)
        if has and perms in ("shared", "mixed"):
            if shared is None:
                shared = L.perm
            L.perm = shared.copy()
        Ls.append(L)
    return Ls


def group_descs(Ls, dev):
    """-> (ctypes array of the members' descriptors, [own descriptor copies], modules, keep): members whose permutations are equal
    carry ONE perm pointer (the first such member's), as `SiblingGroup.forward_batched` hands them over"""
    from vptq_amd import _backend as B
    ms = [spec_to_module(L, dev) for L in Ls]
    pairs = [module_desc(m) for m in ms]
    ds = [B.LayerDesc.from_buffer_copy(d) for d, _ in pairs]
    first = []
    for L, d in zip(Ls, ds):
        if L.perm is None:
            continue
        for p, ptr in first:
            if np.array_equal(p, L.perm):
                d.perm = ptr
                break
        else:
            first.append((L.perm, d.perm))
    return (B.LayerDesc * len(ds))(*ds), ds, ms, pairs


def distinct_perms(ds):
    return len({d.perm for d in ds if d.perm})


def instance(descs, n, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(320)
    B.check(B.lib().vptq_quant_gemm_gather_grouped_instance(descs, n, tokens, 0, buf, len(buf)), "vptq_quant_gemm_gather_grouped_instance")
    return buf.value.decode()


def expect_instance(descs, ds, Ls, tokens, T):
    from vptq_amd import _backend as B
    n, G = len(ds), Ls[0].in_features
    assert B.lib().vptq_quant_gemm_gather_grouped_supported(descs, n, tokens) == 1
    k = distinct_perms(ds)
    need = k * ((tokens * G * 2 + 255) // 256 * 256)
    assert B.lib().vptq_quant_gemm_gather_grouped_workspace_bytes(descs, n, tokens) == need
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = [(L.num_indices + R - 1) // R for L in Ls]
    grid = min(sum(groups), 4 * cus)
    head = "none" if k == 0 else \
        f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK} perms={k}"
    want = (f"{head} | gemm_gather_grouped dt={Ls[0].dtype} t={T} tok={tokens} n={n} groups={'+'.join(map(str, groups))} "
            f"tiles={(G + TILE - 1) // TILE} grid={grid} rgs={(sum(groups) + grid - 1) // grid}")
    text = instance(descs, n, tokens)
    assert text == want, (text, want)
    return need


def grouped_call(descs, n, xt, outs, out_f32=False, ws=None):
    """the entry with every y's token rows NaN between guard rows and a workspace of EXACTLY the query's bytes (0xFF bytes unless one
    is handed in); -> [y_m [tokens, O_m]] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = B.lib().vptq_quant_gemm_gather_grouped_workspace_bytes(descs, n, tokens)
    if ws is None and need:
        ws = torch.full((need,), 255, dtype=torch.uint8, device=xt.device)
    bufs = [torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device) for O in outs]
    for b in bufs:
        b[GUARD:GUARD + tokens] = float("nan")
    ys = [b[GUARD:GUARD + tokens] for b in bufs]
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    B.check(B.lib().vptq_quant_gemm_gather_grouped(descs, n, xt.data_ptr(), yp, tokens, F32 if out_f32 else 0, None if ws is None else ws.data_ptr(),
                                                   0 if ws is None else ws.numel(), B.current_stream_ptr(xt.device)), "vptq_quant_gemm_gather_grouped")
    torch.cuda.current_stream(xt.device).synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return [y.clone() for y in ys]


def own_entry(d, xt, O, out_f32=False):
    """the member's own entry on the same descriptor and x: the comparison (the parent's code)"""
    return px_call(d, xt, O, out_f32=out_f32) if d.perm else call(d, xt, O, out_f32=out_f32)


def _x(G, tokens, dt, seed, dev):
    x = _dense(G, tokens, dt, seed)[0]
    return x, bits_to_tensor(x, dt, dev).reshape(tokens, G)


# ---------------------------------------------------------------------------------------------- 1. bits and sums
def _bit_rows():
    rows = []
    for i, (G, T, case) in enumerate(itertools.product(GS, (16, 24, 32), PERM_CASES)):
        # 48 rows: every (columns, T, permutation case); members, token count, dtype and bias advance at strides of their own.
        # GUARANTEED (the test below asserts them): every (T, dtype), (T, permutation case), (group size, permutation case) and
        # (columns, tokens) pair, and every member output.  NOT guaranteed: triples beyond (columns, T, case) - e.g. T = 24 with bf16,
        # 4 members and 2 TILE + 264 columns may not meet; the kernel's paths depend on (DT, T) and on columns / tokens separately
        n = (2, 3, 4)[(i + i // 3) % 3]
        outs = tuple(OUTS[(i + j) % 4] for j in range(n))
        rows.append(pytest.param(dict(G=G, T=T, case=case, outs=outs, tokens=TOKS[(i + i // 4) % 4], dt=("f16", "bf16")[(i + i // 12 + i // 4) % 2],
                                      bias=(i // 2) % 2), id=f"G{G}-t{T}-{case}-n{n}-i{i}"))
    return rows


def test_the_bit_rows_cover_every_t_dtype_group_size_and_permutation_case():
    rows = [e.values[0] for e in _bit_rows()]
    assert {(e["T"], e["dt"]) for e in rows} == set(itertools.product((16, 24, 32), ("f16", "bf16")))
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
    for f32 in (False, True):
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
def _switch_outs(walk, cus):
    """member outputs at 64 columns over a grid of 4 cus workgroups (256 CUs: 1024).  "ends": the issue's example, 700 + 301 + 100
    row groups - the grid ends inside member 1, workgroups 0 .. 76 go from member 0 to member 2.  "three": 40 + 1101 + 1000 row
    groups - workgroups 0 .. 39 walk g, g + 1024, g + 2048 through members 0, 1 and 2 (two CONSECUTIVE switches each, the table
    re-staged twice), the others switch from member 1 to member 2"""
    if walk == "ends":
        return (16 * max(100, 4 * cus - 324), 16 * 300 + 4, 16 * 100), 2
    return (16 * 40, 16 * (4 * cus + 76) + 4, 16 * (4 * cus - 24)), 3


@pytest.mark.parametrize("walk", ["ends", "three"])
@pytest.mark.parametrize("T,dt,case", [(24, "f16", "none"), (24, "bf16", "shared"), (16, "bf16", "mixed"), (32, "f16", "distinct")])
def test_member_switch_inside_a_workgroup_keeps_every_members_bits(T, dt, case, walk, dev):
    """more row groups than workgroups: a workgroup walks row groups of several members, with another residual table (T = 24: in
    LDS, re-staged at the switch), other scales and biases in each"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    outs, rgs = _switch_outs(walk, cus)
    G, tokens = 64, 15
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
G1 = TILE + 8
COLS16 = [0, 1, 7, 8, 63, 64, 300, 511, 512, TILE - 2, TILE - 1, TILE, TILE + 1, G1 - 3, G1 - 2, G1 - 1]


@pytest.mark.parametrize("T,dt,case", [(24, "f16", "distinct"), (16, "bf16", "mixed"), (32, "bf16", "shared"), (24, "bf16", "none")])
def test_one_hot_activations_read_dequant_bits_for_every_member(T, dt, case, dev):
    outs = (20, 36, 12)
    Ls = make_group(G1, outs, T, dt, case, bias=0)          # (no output bias: y is a column of W)
    descs, ds, ms, keep = group_descs(Ls, dev)
    x = torch.zeros(16, G1, dtype=ms[0].centroids.weight.dtype, device=dev)
    x[torch.arange(16), torch.tensor(COLS16)] = 1.0           # input feature j: it reaches stored column c with perm[c] == j
    ys = grouped_call(descs, 3, x, outs)
    for m, (y, mod) in enumerate(zip(ys, ms)):
        want = mod.dequant()[:, torch.tensor(COLS16, device=dev)].t()
        assert not bool(torch.isnan(y).any())
        assert bool((y == want).all()), f"member {m}: {int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 4. placement
HOSTILE_OFFSETS = {"indices": 16, "centroids": 16, "res_centroids": 16, "weight_scale": 4, "weight_bias": 4, "perm": 4, "bias": 2}


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
    need = B.lib().vptq_quant_gemm_gather_grouped_workspace_bytes(descs, len(ds), tokens)
    assert need == distinct_perms(ds) * ((tokens * Ls[0].in_features * 2 + 255) // 256 * 256) > 0
    ws, wa = ar.guarded_workspace(need, False, dev, align=16)
    assert ws.numel() == need and ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 != 0
    yp = (C.c_void_p * len(ds))(*[y.data_ptr() for y, _ in outs_placed])
    B.check(B.lib().vptq_quant_gemm_gather_grouped(descs, len(ds), xv.data_ptr(), yp, tokens, F32 if f32 else 0, ws.data_ptr(), need,
                                                   B.current_stream_ptr(dev)), "vptq_quant_gemm_gather_grouped")
    torch.cuda.synchronize(dev)
    for name, a in list(arenas.items()) + [("x", xa)]:
        assert a.intact(), (name, a.damage())                    # the inputs' margins
    for i, (y, ya) in enumerate(outs_placed):
        assert ya.intact(), (f"y[{i}]", ya.damage())             # a store outside y
        assert not bool(torch.isnan(y).any())
    assert wa.intact(), ("workspace", wa.damage())               # a store outside the query's bytes
    assert torch.equal(xv, xt)
    return [y.clone() for y, _ in outs_placed], ds, pairs, ms


@pytest.mark.parametrize("T,dt,G,tokens", [(24, "f16", TILE + 8, 5), (32, "bf16", 2 * TILE + 264, 16), (16, "f16", 64, 15)])
def test_same_bits_under_every_placement(T, dt, G, tokens, dev):
    outs = (20, 4, 36)
    Ls = make_group(G, outs, T, dt, "distinct")      # (three x gathers: three blocks of the workspace)
    _, xt = _x(G, tokens, dt, 3, dev)
    for f32 in (False, True):
        benign, _, _, _ = _placed_call(Ls, xt, tokens, outs, ar.BENIGN, {}, 0, 0, f32, dev)
        hostile, _, _, _ = _placed_call(Ls, xt, tokens, outs, ar.HOSTILE, HOSTILE_OFFSETS, 16, 4 if f32 else 2, f32, dev)
        descs, ds, ms, keep = group_descs(Ls, dev)
        for m, (a, b, d, O) in enumerate(zip(benign, hostile, ds, outs)):
            assert torch.equal(_bits(a), _bits(b)), m
            assert torch.equal(_bits(a), _bits(own_entry(d, xt, O, out_f32=f32))), m   # torch's allocator: the own entry's bits


@pytest.mark.parametrize("T,dt", [(24, "f16"), (32, "bf16")])
def test_workspace_contents_do_not_matter_and_calls_share_it(T, dt, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (12, 36)
    Ls = make_group(G, outs, T, dt, "distinct")
    descs, ds, ms, keep = group_descs(Ls, dev)
    _, x16 = _x(G, 16, dt, 5, dev)
    _, x5 = _x(G, 5, dt, 6, dev)
    fresh16, fresh5 = grouped_call(descs, 2, x16, outs), grouped_call(descs, 2, x5, outs)
    need = B.lib().vptq_quant_gemm_gather_grouped_workspace_bytes(descs, 2, 16)
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


# ---------------------------------------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("T,dt,case,tokens", [(24, "f16", "mixed", 12), (32, "bf16", "distinct", 16), (16, "f16", "none", 5)])
def test_a_captured_call_replays_on_new_activations(T, dt, case, tokens, dev):
    from vptq_amd import _backend as B
    G, outs = 2 * TILE + 264, (20, 36, 12)
    Ls = make_group(G, outs, T, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    xs = [_x(G, tokens, dt, s, dev)[1] for s in (1, 2, 3)]
    eager = [grouped_call(descs, 3, x, outs) for x in xs]
    need = B.lib().vptq_quant_gemm_gather_grouped_workspace_bytes(descs, 3, tokens)
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
            B.check(B.lib().vptq_quant_gemm_gather_grouped(descs, 3, xg.data_ptr(), yp, tokens, 0, ws.data_ptr() if need else None, need,
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


class _Block(torch.nn.Module):
    def __init__(self, names, mods):
        super().__init__()
        for n, m in zip(names, mods):
            setattr(self, n, m)
        self.names = names

    def forward(self, x):
        return [getattr(self, n)(x) for n in self.names]


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


QKV, GU = ("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj")


@pytest.mark.parametrize("names,outs,T,dt,case,tokens", [(QKV, (512, 128, 132), 24, "f16", "shared", 16), (GU, (264, 260), 32, "bf16", "none", 5),
                                                         (QKV, (128, 512, 136), 16, "bf16", "mixed", 9), (GU, (260, 264), 24, "f16", "distinct", 12)])
def test_linked_siblings_take_one_grouped_launch_with_their_own_bits(names, outs, T, dt, case, tokens, dev, monkeypatch):
    from vptq_amd import grouped_decode as gd
    I = 2048
    Ls = make_group(I, outs, T, dt, case)
    x, xt = _x(I, tokens, dt, 9, dev)
    xt = xt.reshape(1, tokens, I)
    twins = _block(names, Ls, dev, link=False)
    # the committed cells never hold a group this small: the routes of before, no grouped launch - linked or not
    assert not gd.gemm_gather_grouped_route(8, 65536, KR[T], outs, I, tokens, {"shared": True, "distinct": True, "none": False, "mixed": None}[case])
    y_today, today = _spied(lambda: twins(xt), monkeypatch)
    assert "vptq_quant_gemm_gather_grouped" not in today and len(today) >= len(outs)
    y_linked, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y_linked, y_today))
    # the knob on: ONE grouped launch, the followers pick their outputs up, every member has the bits of its un-linked twin's own entry
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    blk = _block(names, Ls, dev)
    ys, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_grouped"], calls
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
    assert calls == ["vptq_quant_gemm_gather_grouped"] * 2, calls
    assert torch.equal(_bits(y0), _bits(ys[0])) and torch.equal(_bits(y1), _bits(ys[1]))
    # tensors without a version counter are never shared: every member goes on alone over the routes of before
    # (the grouped entry is looked up at every call, so the spy would see it; a member's own launch may go through a function its
    # descriptor kept, so the other names are not compared here)
    with torch.inference_mode():
        xi = xt.clone()
        yi, calls = _spied(lambda: blk(xi), monkeypatch)
    assert "vptq_quant_gemm_gather_grouped" not in calls and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(yi, y_today))
    # the knob at 0: the routes and the bits of before
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "0")
    y0s, calls = _spied(lambda: _block(names, Ls, dev)(xt), monkeypatch)
    assert calls == today and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(y0s, y_today))


def test_a_compacted_member_makes_the_group_step_aside(dev, monkeypatch):
    from vptq_amd import grouped_decode as gd
    I, outs, tokens = 2048, (512, 128, 132), 8
    Ls = make_group(I, outs, 24, "f16", "shared")
    _, xt = _x(I, tokens, "f16", 4, dev)
    xt = xt.reshape(1, tokens, I)
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
    twins, blk = _block(QKV, Ls, dev, link=False), _block(QKV, Ls, dev)
    for b in (twins, blk):
        b.k_proj.compact(force=True)
        assert b.k_proj.is_compact()
    y_twins, before = _spied(lambda: twins(xt), monkeypatch)
    ys, calls = _spied(lambda: blk(xt), monkeypatch)
    assert "vptq_quant_gemm_gather_grouped" not in calls and calls == before, (calls, before)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, y_twins))
    # uncompacted again (a rebuilt descriptor): the group takes the call
    blk.k_proj.uncompact()
    ys2, calls = _spied(lambda: blk(xt), monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_grouped"], calls


def test_prepare_model_sizes_the_workspace_and_a_captured_step_keeps_the_group_route(dev, monkeypatch):
    import vptq_amd
    from vptq_amd import _backend as B, grouped_decode as gd
    I, outs, tokens = 2 * TILE + 264, (36, 20, 12), 16
    Ls = make_group(I, outs, 24, "f16", "distinct")
    monkeypatch.setattr(gd, "_GEMM_GATHER_GROUPED_MODE", "1")
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
    assert calls == ["vptq_quant_gemm_gather_grouped"]
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ys, calls = _spied(lambda: blk(xt), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert calls == ["vptq_quant_gemm_gather_grouped"], calls          # the captured step keeps the group's route
    g.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, eager))
    # a capture on a stream whose workspace was not sized: the op answers None, nothing is launched or allocated
    from vptq_amd import ops
    descs, caches = group._batched_plan()
    s2 = _stream_without_a_workspace(dev)
    key2 = (key[0], s2.cuda_stream)
    g2 = torch.cuda.CUDAGraph()
    s2.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s2):
        with torch.cuda.graph(g2, stream=s2):
            doubled = xt * 2                                           # (so that the graph is not empty)
            got, calls = _spied(lambda: ops.quant_gemm_gather_grouped(xt, descs, outs), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s2)
    assert got is None and calls == [] and key2 not in B._GEMV_WS
