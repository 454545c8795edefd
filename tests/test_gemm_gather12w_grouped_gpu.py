"""vptq_quant_gemm_gather12w_grouped (gemm_gather12w_grouped.hip) on the GPU: 17 - 48 tokens of 2 - 4 sibling v = 12 layers in one launch.
Widths are gemm_gather12c's (TILE + 8: 1 + 1 parts, the second of 8 columns; 2 TILE; 4 TILE + 264: five tiles, the last ragged); the
members' 56 / 20 / 100 / 32 outputs end in ragged vector-rows and row groups; tokens 17 (one live token in the last block), 31, 32 (a full
TB = 2), 33 (the first TB = 3), 47, 48.  The contract is BIT IDENTITY with vptq_quant_gemm_gather12w on the member's own descriptor at the
same tokens and split: no tolerance.  Every call asserts its instance line first.
The rows of a table are walked inside ONE test each, to keep the suite's test count down (tests/test_gemm_gather12_grouped_gpu.py does so
for its side tables; here the main table too): every row runs whatever another row does, and the test fails with the list of failing
rows by id."""
import ctypes as C
import itertools

import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import GUARD, SENTINEL, F32
from test_gemm_gather_grouped_gpu import group_descs, distinct_perms, _Block
from test_gemm_gather12_gpu import FMT, TILE
from test_gemm_gather12c_gpu import G5
from test_gemm_gather12_grouped_gpu import make_group, _bits
from test_gemm_gather12w_gpu import call as call12w, COLS
from test_gemm_gatherxw_grouped_gpu import _spied, _stream_without_a_workspace
from test_gemm_gather12w_grouped_cpu import want, want_bytes, split
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor

pytestmark = pytest.mark.gpu

ENTRY = "vptq_quant_gemm_gather12w_grouped"
FMTS = ("v12-k65536-0", "v12-k65536-256", "v12-k65536-4096")    # RES = none / table in LDS / table from L2
WIDTHS = (TILE + 8, 2 * TILE, G5)
OUTS = (56, 20, 100, 32)
CASES = ("none", "distinct", "shared", "some")
TOKS = (17, 31, 32, 33, 47, 48)


def expect_instance(descs, ds, tokens, parts):
    """the instance line and the workspace query against their restatement; -> (S, line)"""
    from vptq_amd import _backend as B
    cus, n = torch.cuda.get_device_properties(0).multi_processor_count, len(ds)
    assert getattr(B.lib(), ENTRY + "_supported")(descs, n, tokens, parts) == 1
    buf = C.create_string_buffer(384)
    B.check(getattr(B.lib(), ENTRY + "_instance")(descs, n, tokens, 0, parts, buf, len(buf)), ENTRY + "_instance")
    assert buf.value.decode() == want(ds, tokens, parts, cus), (buf.value.decode(), want(ds, tokens, parts, cus))
    assert getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens, parts) == want_bytes(ds, tokens, parts, cus)
    return split(ds, tokens, parts, cus)[0], buf.value.decode()


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


def assert_own_bits(ys, ds, xt, outs, S, f32=False):
    """every member against vptq_quant_gemm_gather12w on its own descriptor, the same x and tokens, S parts"""
    for m, (y, d, O) in enumerate(zip(ys, ds, outs)):
        own = call12w(d, xt, O, S, out_f32=f32)
        assert not bool(torch.isnan(y).any()), m
        assert torch.equal(_bits(y), _bits(own)), f"member {m}: {int((_bits(y) != _bits(own)).sum())} of {y.numel()} outputs differ from its own entry (S = {S})"


def _rows():
    rows = []
    for i, (fmt, dt, G) in enumerate((list(itertools.product(FMTS, ("f16", "bf16"), WIDTHS)) * 2)[:27]):
        # 27 rows: every (format, dtype, width), half of them twice; the other axes cycle with short periods at strides of their own: all
        # 12 instantiations (dtype, RES, TB) run, 8 of them both with one part and with a split; the model rows meet every width
        n = (2, 3, 4)[(i + i // 3) % 3]
        rows.append(dict(fmt=fmt, dt=dt, G=G, outs=tuple(OUTS[(i + j) % 4] for j in range(n)), case=CASES[(i + i // 4) % 4],
                         parts=(1, 2, 3, 5)[(i + i // 5) % 4], tokens=TOKS[(i + i // 6) % 6], bias=(i // 3) % 2, f32=i % 5 == 0,
                         model=(i + i // 2) % 3 == 0, x=("dense", "planted")[(i // 3) % 2], id=f"{fmt}-{dt}-G{G}-n{n}-i{i}"))
    return rows


def test_every_member_has_the_bits_of_its_own_entry(dev):
    failed = []
    for e in _rows():
        try:
            _bits_row(e, dev)
        except AssertionError as err:
            failed.append(f"row {e['id']} (tokens {e['tokens']}, parts {e['parts']}, {e['case']}): {err}")
    assert not failed, "\n".join(failed)


def _bits_row(e, dev):
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
    if e["model"]:   # a third of the rows: the weights are vptq_dequant's bits, the sums lie within the fp64 model's bounds
        y16 = ys if not e["f32"] else grouped_call(descs, n, xt, outs, e["parts"])
        y32 = ys if e["f32"] else grouped_call(descs, n, xt, outs, e["parts"], out_f32=True)
        for m, L in enumerate(Ls):
            mm, aa = am.model(am.pieces(L), x, arith="exact")
            am.check_both(_np(y16[m]), _np(y32[m]), mm, aa, e["dt"], what=f"member {m}: {text}")
        # (G5: both sides of every tile (= part) boundary first)
        cols = COLS[:tokens] if e["G"] == G5 else [c % e["G"] for c in range(0, 8 * tokens, 8)][:tokens - 2] + [e["G"] - 1, TILE - 1]
        one = torch.zeros(tokens, e["G"], dtype=xt.dtype, device=dev)
        for m, (L, mod) in enumerate(zip(Ls, ms)):
            if L.bias is not None:                             # (member 1 never has an output bias: y is the weight itself)
                continue
            src = torch.tensor([int(L.perm[c]) for c in cols] if L.perm is not None else cols)
            one.zero_()
            one[torch.arange(tokens), src] = 1.0
            ym, want_w = grouped_call(descs, n, one, outs, e["parts"])[m], mod.dequant()[:, src.to(dev)].t()
            assert bool((ym == want_w).all()), f"member {m}: {int((ym != want_w).sum())} of {ym.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


def test_every_workgroup_changes_member_and_linked_siblings_take_the_launch(dev, monkeypatch):
    for fmt, dt, tokens in (("v12-k65536-0", "f16", 33), ("v12-k65536-256", "bf16", 48), ("v12-k65536-4096", "f16", 17), ("v12-k65536-256", "f16", 32)):
        _member_change_row(fmt, dt, tokens, dev)
    # (516, 128, 132): 4 parts of one tile at every token count.  (4800, 2400, 2400), 200 row groups with a residual table: 4 parts up to 32
    # tokens, 2 from 33 (one workgroup per CU), so the 32-token step needs MORE workspace than the 48-token one prepare_model must cover
    for tokens, outs in ((17, (516, 128, 132)), (48, (516, 128, 132)), (32, (4800, 2400, 2400))):
        with monkeypatch.context() as mp:
            _module_route_row(tokens, outs, dev, mp)


def _member_change_row(fmt, dt, tokens, dev):
    outs = (48 * 200 - 4, 48 * 150, 48 * 180 - 40)             # 200 / 150 / 180 row groups x 2 parts: 1060 items on 512 / 256 slots
    Ls = make_group(TILE + 8, outs, fmt, dt, "some")
    descs, ds, ms, keep = group_descs(Ls, dev)
    S, text = expect_instance(descs, ds, tokens, 2)
    inner = text.split("gemm_gather12w_grouped ")[1].split(" | ")[0]     # (the permute and sum launches have a grid= of their own)
    grid, rgs = (int(inner.split(f" {k}=")[1].split()[0]) for k in ("grid", "rgs"))
    assert S == 2 and " groups=200+150+180 " in text and rgs >= 2 and 2 * grid <= 1060
    if FMT[fmt][1]:   # members with DIFFERENT residual tables: a switch that kept the previous member's table would show
        tabs = [m.res_centroids.weight.detach().reshape(-1) for m in ms]
        assert not torch.equal(tabs[0], tabs[1]) and not torch.equal(tabs[1], tabs[2])

    def member(it):
        return sum(it >= first for first in (400, 700))
    assert all(len({member(it) for it in range(b, 1060, grid)}) >= 2 for b in range(grid))   # every workgroup walks items of two members or more
    xt = bits_to_tensor(_dense(TILE + 8, tokens, dt, 7)[0], dt, dev).reshape(tokens, TILE + 8)
    a, b = grouped_call(descs, 3, xt, outs, 2), grouped_call(descs, 3, xt, outs, 2, fill=0x5C)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    assert_own_bits(a, ds, xt, outs, 2)


def _module_route_row(tokens, outs, dev, monkeypatch):
    import vptq_amd
    from vptq_amd import _backend as B, batched_decode as bd, grouped_decode as gd
    from vptq_amd.layers import link_siblings
    names, I = ("q_proj", "k_proj", "v_proj"), 2048
    # a member's own forward takes gemm_gather12w (its knob on), whose rule cuts the 4 tiles into 4 parts, as the group's rule does at
    # these token counts: the bit contract then holds between the grouped launch and the members' own forward
    monkeypatch.setattr(bd, "_GEMM_GATHER12W_MODE", "1")
    Ls = make_group(I, outs, "v12-k65536-4096", "bf16", "shared")
    xs = [bits_to_tensor(_dense(I, tokens, "bf16", s)[0], "bf16", dev).reshape(1, tokens, I) for s in (9, 10)]
    twins, blk = (_Block(names, [spec_to_module(L, dev) for L in Ls]) for _ in range(2))
    assert link_siblings(blk) == 1
    y_own, own = _spied(lambda: twins(xs[0]), monkeypatch)
    assert own == ["vptq_quant_gemm_gather12w"] * 3, own
    monkeypatch.setattr(gd, "_GEMM_GATHER12W_GROUPED_MODE", "0")
    assert _spied(lambda: blk(xs[0]), monkeypatch)[1] == own                                          # the knob at 0: today's launches
    monkeypatch.setattr(gd, "_GEMM_GATHER12W_GROUPED_MODE", "1")
    blk2 = _Block(names, [spec_to_module(L, dev) for L in Ls])   # (a group reads its knob once)
    assert link_siblings(blk2) == 1
    ys, calls = _spied(lambda: blk2(xs[0]), monkeypatch)
    assert calls == [ENTRY], calls                                                                   # one grouped call, nothing else
    assert all(y.shape == (1, tokens, O) and torch.equal(_bits(y), _bits(t)) for y, t, O in zip(ys, y_own, outs))
    group = blk2.q_proj.__dict__["_siblings"]
    descs = group._batched_plan(group._batched_route(tokens))[0]
    need = [getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, 3, t, 0) for t in (32, 48)]
    assert (need[0] > need[1]) == (outs[0] == 4800) and group._batched_workspace_bytes()[2] >= max(need), need
    # a fresh stream, its workspace sized by prepare_model: the captured step keeps the route (its branches are sequential on one stream)
    s = _stream_without_a_workspace(dev)
    vptq_amd.prepare_model(blk2, s)
    xg, g = xs[0].clone(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            yg, calls = _spied(lambda: blk2(xg), monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert calls == [ENTRY], calls
    for x in (xs[1], xs[0]):   # replays on new activations: the un-linked forward's bits
        xg.copy_(x)
        g.replay()
        torch.cuda.synchronize(dev)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(yg, twins(x)))
