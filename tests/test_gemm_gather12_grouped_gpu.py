"""vptq_quant_gemm_gather12_grouped (gemm_gather12_grouped.hip) on the GPU: 1 - 16 tokens of 2 - 4 sibling v = 12 layers in one launch.
Widths are gemm_gather12c's (TILE + 8: 1 + 1 parts, the second of 8 columns; 2 TILE; 4 TILE + 264: 3 + 2, 2 + 2 + 1, five of one tile, the last
ragged); the members' 56 / 20 / 100 / 32 outputs end in ragged vector-rows and row groups.  The contract is BIT IDENTITY with the member's own
entry (gemm_gather12c at the same parts, gemm_gather12 at one part): no tolerance.  Every call asserts its instance line first."""
import ctypes as C
import itertools

import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gather_grouped_gpu import group_descs, distinct_perms, _Block
from test_gemm_gather12_gpu import FMT, BITS, TILE, call as call12
from test_gemm_gather12c_gpu import call as call12c, COLS1, G5
from test_gemm_gather12_grouped_cpu import want, want_bytes, split
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu

ENTRY = "vptq_quant_gemm_gather12_grouped"
FMTS = ("v12-k65536-0", "v12-k65536-256", "v12-k65536-4096")    # RES = none / table in LDS / table from L2
WIDTHS = (TILE + 8, 2 * TILE, G5)
OUTS = (56, 20, 100, 32)
CASES = ("none", "distinct", "shared", "some")
TOKS = (1, 5, 8, 9, 15, 16)


def make_group(G, outs, fmt, dt, case, bias=1):
    """-> [LayerSpec]: members of one format and a seed each (their tables, scales and biases differ); case: "distinct" - every member
    has a permutation of its own, "shared" - members 0 and 1 share one, the others have their own, "some" - members 0, 2 have one"""
    from oracle import vptq_oracle as vo
    k, kr = FMT[fmt]
    Ls = []
    for i, O in enumerate(outs):
        has = case in ("distinct", "shared") or (case == "some" and i % 2 == 0)
        L = vo.make_layer(G, O, dist="llm", seed=G + O + BITS[fmt] + 1000 * i, dtype=dt, vector_len=12, num_centroids=k, num_res_centroids=kr,
                          enable_perm=has, bias=bool(bias) and i != 1, enable_norm=True)
        if case == "shared" and i == 1:
            L.perm = Ls[0].perm.copy()
        Ls.append(L)
    return Ls


def expect_instance(descs, ds, tokens, parts):
    """the instance line and the workspace query against their restatement; -> (S, line)"""
    from vptq_amd import _backend as B
    cus, n = torch.cuda.get_device_properties(0).multi_processor_count, len(ds)
    assert getattr(B.lib(), ENTRY + "_supported")(descs, n, tokens, parts) == 1
    buf = C.create_string_buffer(384)
    B.check(getattr(B.lib(), ENTRY + "_instance")(descs, n, tokens, 0, parts, buf, len(buf)), ENTRY + "_instance")
    assert buf.value.decode() == want(ds, tokens, parts, cus), (buf.value.decode(), want(ds, tokens, parts, cus))
    assert getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens, parts) == want_bytes(ds, tokens, parts, cus)
    return split(ds, parts, cus)[0], buf.value.decode()


def grouped_call(descs, n, xt, outs, parts, out_f32=False, fill=0xAB):
    """the entry with every y's token rows NaN between guard rows; -> [y_m [tokens, O_m]] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens, parts)
    ws = torch.full((max(need, 16),), fill, dtype=torch.uint8, device=xt.device)
    bufs = [torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device) for O in outs]
    for b in bufs:
        b[GUARD:GUARD + tokens] = float("nan")
    ys = [b[GUARD:GUARD + tokens] for b in bufs]
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    B.check(getattr(B.lib(), ENTRY)(descs, n, xt.data_ptr(), yp, tokens, F32 if out_f32 else 0, parts, ws.data_ptr() if need else None, need,
                                    B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return [y.clone() for y in ys]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_own_bits(ys, ds, xt, outs, S, f32=False):
    """every member against its own entry on its own descriptor and the same x: gemm_gather12c at S parts, gemm_gather12 at one"""
    for m, (y, d, O) in enumerate(zip(ys, ds, outs)):
        own = call12c(d, xt, O, S, out_f32=f32) if S >= 2 else call12(d, xt, O, out_f32=f32)
        assert not bool(torch.isnan(y).any()), m
        assert torch.equal(_bits(y), _bits(own)), f"member {m}: {int((_bits(y) != _bits(own)).sum())} of {y.numel()} outputs differ from its own entry (S = {S})"


def _rows():
    rows = []
    for i, (fmt, dt, G) in enumerate(list(itertools.product(FMTS, ("f16", "bf16"), WIDTHS)) * 2):
        # 36 rows: every (format, dtype, width) twice; the other axes cycle with short periods at strides of their own
        n = (2, 3, 4)[(i + i // 3) % 3]
        rows.append(pytest.param(dict(fmt=fmt, dt=dt, G=G, outs=tuple(OUTS[(i + j) % 4] for j in range(n)), case=CASES[(i + i // 4) % 4],
                                      parts=(1, 2, 3, 5)[(i // 2 + i // 5) % 4], tokens=TOKS[(i + i // 6) % 6], bias=(i // 3) % 2, f32=i % 5 == 0,
                                      model=i % 3 == 0, x=("dense", "planted")[(i // 3) % 2]), id=f"{fmt}-{dt}-G{G}-n{n}-i{i}"))
    return rows


@pytest.mark.parametrize("e", _rows())
def test_every_member_has_the_bits_of_its_own_entry(e, dev):
    Ls = make_group(e["G"], e["outs"], e["fmt"], e["dt"], e["case"], bias=e["bias"])
    descs, ds, ms, keep = group_descs(Ls, dev)
    n, tokens, outs = len(ds), e["tokens"], e["outs"]
    assert distinct_perms(ds) == {"none": 0, "distinct": n, "shared": n - 1, "some": (n + 1) // 2}[e["case"]]
    S, text = expect_instance(descs, ds, tokens, e["parts"])
    kw = dict(perm=Ls[0].perm) if e["x"] == "planted" and Ls[0].perm is not None else {}
    x = (_planted if e["x"] == "planted" else _dense)(e["G"], tokens, e["dt"], e["G"] + tokens, **kw)[0]
    xt = bits_to_tensor(x, e["dt"], dev).reshape(tokens, e["G"])
    ys = grouped_call(descs, n, xt, outs, e["parts"], out_f32=e["f32"])
    assert_own_bits(ys, ds, xt, outs, S, f32=e["f32"])
    if e["model"]:
        y16 = ys if not e["f32"] else grouped_call(descs, n, xt, outs, e["parts"])
        y32 = ys if e["f32"] else grouped_call(descs, n, xt, outs, e["parts"], out_f32=True)
        for m, L in enumerate(Ls):
            mm, aa = am.model(am.pieces(L), x, arith="exact")
            am.check_both(_np(y16[m]), _np(y32[m]), mm, aa, e["dt"], what=f"member {m}: {text}")


# (one row per RES kind below; the rows of a table are walked inside ONE test each, to keep the suite's test count down)
def test_one_hot_activations_read_dequant_bits(dev):
    for fmt, dt, parts in (("v12-k65536-0", "bf16", 2), ("v12-k65536-256", "f16", 3), ("v12-k65536-4096", "bf16", 5)):
        _one_hot_row(fmt, dt, parts, dev)


def _one_hot_row(fmt, dt, parts, dev):
    outs = (56, 20, 100)
    Ls = make_group(G5, outs, fmt, dt, "none", bias=0)        # (no output bias: y is the weight itself)
    descs, ds, ms, keep = group_descs(Ls, dev)
    assert expect_instance(descs, ds, 16, parts)[0] == parts
    if FMT[fmt][1]:   # members with DIFFERENT residual tables: a switch that kept the previous member's table would show
        tabs = [m.res_centroids.weight.detach().reshape(-1) for m in ms]
        assert not torch.equal(tabs[0], tabs[1]) and not torch.equal(tabs[1], tabs[2])
    x = torch.zeros(16, G5, dtype=ms[0].centroids.weight.dtype, device=dev)
    x[torch.arange(16), torch.tensor(COLS1)] = 1.0          # both sides of every part boundary of 3 + 2, 2 + 2 + 1 and 1 x 5
    for m, (y, mod) in enumerate(zip(grouped_call(descs, 3, x, outs, parts), ms)):
        want_w = mod.dequant()[:, torch.tensor(COLS1, device=dev)].t()
        assert not bool(torch.isnan(y).any())
        assert bool((y == want_w).all()), f"{fmt} {dt}, member {m}: {int((y != want_w).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


def test_workgroups_walk_items_of_more_than_one_member(dev):
    for fmt, dt in (("v12-k65536-0", "f16"), ("v12-k65536-256", "bf16"), ("v12-k65536-4096", "f16")):
        _member_switch_row(fmt, dt, dev)


def _member_switch_row(fmt, dt, dev):
    outs = (48 * 200 - 4, 48 * 150, 48 * 180 - 40)             # 200 / 150 / 180 row groups x 2 parts: 1060 items on 512 slots
    Ls = make_group(TILE + 8, outs, fmt, dt, "some")
    descs, ds, ms, keep = group_descs(Ls, dev)
    S, text = expect_instance(descs, ds, 9, 2)
    inner = text.split("gemm_gather12_grouped ")[1].split(" | ")[0]     # (the permute and sum launches have a grid= of their own)
    grid, rgs = (int(inner.split(f" {k}=")[1].split()[0]) for k in ("grid", "rgs"))
    assert S == 2 and " groups=200+150+180 " in text and rgs >= 2 and 2 * grid <= 1060

    def member(it):
        return sum(it >= first for first in (400, 700))
    assert all(member(b) != member(b + grid) for b in range(grid))   # every workgroup's first two items lie in different members
    xt = bits_to_tensor(_dense(TILE + 8, 9, dt, 7)[0], dt, dev).reshape(9, TILE + 8)
    assert_own_bits(grouped_call(descs, 3, xt, outs, 2), ds, xt, outs, 2)


def test_two_launches_and_graph_replays_give_the_same_bits(dev):
    for parts in (3, 1):
        _relaunch_and_capture(parts, dev)


def _relaunch_and_capture(parts, dev):
    from vptq_amd import _backend as B
    outs = (56, 20, 100)
    Ls = make_group(G5, outs, "v12-k65536-256", "f16", "shared")
    descs, ds, ms, keep = group_descs(Ls, dev)
    expect_instance(descs, ds, 13, parts)
    xt = bits_to_tensor(_dense(G5, 13, "f16", 5)[0], "f16", dev).reshape(13, G5)
    a, b = grouped_call(descs, 3, xt, outs, parts), grouped_call(descs, 3, xt, outs, parts, fill=0x5C)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, 3, 13, parts)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=dev)
    yg = [torch.full((13, O), float("nan"), dtype=xt.dtype, device=dev) for O in outs]
    yp = (C.c_void_p * 3)(*[y.data_ptr() for y in yg])
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(getattr(B.lib(), ENTRY)(descs, 3, xt.data_ptr(), yp, 13, 0, parts, ws.data_ptr(), need, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    for _ in range(2):
        for y in yg:
            y.fill_(float("nan"))
        ws.fill_(0xCD)
        g.replay()
        torch.cuda.synchronize(dev)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, yg))


def test_linked_siblings_take_the_grouped_launch_with_the_knob_on(dev, monkeypatch):
    from vptq_amd import _backend as B, batched_decode as bd, grouped_decode as gd
    from vptq_amd.layers import link_siblings
    names, outs, I, tokens = ("q_proj", "k_proj", "v_proj"), (516, 128, 132), 2048, 12
    # a member's own forward takes gemm_gather12c (its knob on: layers this small are in no cell), whose rule cuts the 4 tiles into 4
    # parts, as the group's rule does: the bit contract then holds between the grouped launch and the members' own forward
    monkeypatch.setattr(bd, "_GEMM_GATHER12C_MODE", "1")
    Ls = make_group(I, outs, "v12-k65536-4096", "bf16", "shared")
    xt = bits_to_tensor(_dense(I, tokens, "bf16", 9)[0], "bf16", dev).reshape(1, tokens, I)
    launches = (ENTRY, "vptq_quant_gemm_gather12", "vptq_quant_gemm_gather12c", "vptq_quant_gemm_gatherx", "vptq_quant_gemm_gather_px", "vptq_quant_gemv",
                "vptq_dequant")
    real = B.lib()

    def spied(knob, link):
        monkeypatch.setattr(gd, "_GEMM_GATHER12_GROUPED_MODE", knob)
        blk = _Block(names, [spec_to_module(L, dev) for L in Ls])
        assert not link or link_siblings(blk) == 1
        calls = []
        monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
        try:
            ys = blk(xt)
        finally:
            monkeypatch.setattr(B, "lib", lambda: real)
        return ys, [c for c in calls if c in launches]
    y_today, today = spied("0", link=False)
    assert today == ["vptq_quant_gemm_gather12c"] * 3, today
    y_off, off = spied("0", link=True)
    assert off == today and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(y_off, y_today))      # the knob at 0: today's launches
    y_on, on = spied("1", link=True)
    assert on == [ENTRY], on                                                                         # one grouped call, nothing else
    assert all(y.shape == (1, tokens, O) and torch.equal(_bits(y), _bits(t)) for y, t, O in zip(y_on, y_today, outs))
