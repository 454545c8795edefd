"""vptq_quant_gemm_gather12c (gemm_gather12c.hip): gemm_gather12's layers with the work split over (row group, column part) and the
parts' fp32 sums added by a second kernel, on the GPU.  TILE = 512 columns; the shapes are the smallest that reach each part shape:
TILE + 8 (two parts, the second of 8 columns), 2 TILE (1 + 1), 4 TILE + 264 (3 + 2, 2 + 2 + 1, five of one tile; the last tile ragged).
Every call asserts its instance string first and writes into NaN token rows between sentinel guard rows, with a 0xAB-filled workspace."""
import ctypes as C
import itertools

import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gather_px_gpu import _op_keywords
from test_gemm_gather12_gpu import layer, FMT, BITS, TILE
from test_gemm_gather12c_cpu import want, split
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu

ENTRY = "vptq_quant_gemm_gather12c"


def instance(desc, tokens, parts):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(320)
    B.check(B.lib().vptq_quant_gemm_gather12c_instance(desc, tokens, 0, parts, buf, len(buf)), ENTRY + "_instance")
    return buf.value.decode()


def expect_instance(m, tokens, parts, fmt):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    desc, keep = module_desc(m)
    assert desc.index_bits + desc.res_bits == BITS[fmt] and desc.vector_len == 12
    assert B.lib().vptq_quant_gemm_gather12c_supported(desc, tokens, parts) == 1
    text = instance(desc, tokens, parts)
    assert text == want(desc, tokens, parts, cus), (text, want(desc, tokens, parts, cus))
    return desc, keep


def workspace(desc, tokens, parts, dev, fill=0xAB):
    from vptq_amd import _backend as B
    need = B.lib().vptq_quant_gemm_gather12c_workspace_bytes(desc, tokens, parts)
    assert need > 0
    return torch.full((need,), fill, dtype=torch.uint8, device=dev), need


def call(desc, xt, O, parts, out_f32=False):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    ws, need = workspace(desc, tokens, parts, xt.device)
    B.check(B.lib().vptq_quant_gemm_gather12c(desc, xt.data_ptr(), y.data_ptr(), tokens, F32 if out_f32 else 0, parts, ws.data_ptr(), need,
                                              B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


G5, O1 = 4 * TILE + 264, 56   # five tiles, the last ragged; five vector-rows: two row groups, the second holds one ragged row
# both sides of every part boundary of 3 + 2 (1536), 2 + 2 + 1 (1024, 2048) and 1 x 5 (512 ... 2048), the last column, 5 more
COLS1 = [0, 7, 300, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 1100, 3 * TILE - 1, 3 * TILE, 1800, 4 * TILE - 1, 4 * TILE, G5 - 3, G5 - 2, G5 - 1]


@pytest.mark.parametrize("i,fmt,dt,perm", [(i,) + c for i, c in enumerate(itertools.product(FMT, ("f16", "bf16"), (0, 1)))])
def test_one_hot_activations_read_dequant_bits(i, fmt, dt, perm, dev):
    parts = (2, 3, 5)[(i + i // 4) % 3]
    L = layer(G5, O1, fmt, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, 16, parts, fmt)
    assert split(desc, parts)[0] == parts
    W = m.dequant()
    # the kernel's column c is x's column perm[c]: the hot columns sit at COLS1 in the kernel's order
    cols = torch.tensor([int(L.perm[c]) for c in COLS1] if perm else COLS1)
    x = torch.zeros(16, G5, dtype=W.dtype, device=dev)
    x[torch.arange(16), cols] = 1.0
    y = call(desc, x, O1, parts)
    want_w = W[:, cols.to(dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want_w).all()), f"{int((y != want_w).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


SHAPES = [(TILE + 8, 2), (2 * TILE, 2), (G5, 2), (G5, 3), (G5, 5)]   # (G, parts): every part shape reachable at these widths
TOKS = [1, 5, 8, 9, 15, 16]


def _sum_rows():
    rows = []
    for i, (fmt, dt, (G, parts)) in enumerate(itertools.product(FMT, ("f16", "bf16"), SHAPES)):
        # the other axes cycle with short periods at different strides, as in test_gemm_gather12_gpu._sum_rows
        tokens = TOKS[(i + i // 6) % 6]
        N = (1, 2, 5)[(i // 2 + i // 10) % 3]
        rows.append(pytest.param(dict(fmt=fmt, dt=dt, G=G, parts=parts, tokens=tokens, perm=(i + i // 5) % 2, bias=(i // 3 + i // 15) % 2,
                                      O=12 * N - (0, 4, 8)[(i // 4 + i // 7) % 3], x=("dense", "planted")[(i + i // 2) % 2]),
                                 id=f"{fmt}-{dt}-G{G}-p{parts}-tok{tokens}-i{i}"))
    return rows


def _check_vs_model(L, desc, tokens, parts, kind, dev, seed):
    kw = dict(perm=L.perm) if kind is _planted else {}
    x = kind(L.in_features, tokens, L.dtype, seed, **kw)[0]
    xt = bits_to_tensor(x, L.dtype, dev).reshape(tokens, L.in_features)
    y16, y32 = _np(call(desc, xt, L.out_features, parts)), _np(call(desc, xt, L.out_features, parts, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, tokens, parts))


@pytest.mark.parametrize("e", _sum_rows())
def test_sums_vs_the_exact_model(e, dev):
    L = layer(e["G"], e["O"], e["fmt"], e["dt"], perm=e["perm"], bias=e["bias"])
    desc, keep = expect_instance(spec_to_module(L, dev), e["tokens"], e["parts"], e["fmt"])
    _check_vs_model(L, desc, e["tokens"], e["parts"], _dense if e["x"] == "dense" else _planted, dev, L.in_features + e["tokens"])


def test_more_items_than_resident_workgroups(dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 4 * (cus + 2) - 1                        # CUs + 2 row groups x 2 parts on 2 CUs slots; a ragged last group
    L = layer(TILE + 8, N * 12 - 4, "v12-k65536-256", "bf16", bias=1)
    desc, keep = expect_instance(spec_to_module(L, dev), 9, 2, "v12-k65536-256")
    assert " parts=2 tpp=1 wgcu=2 rgs=2 | " in instance(desc, 9, 2)
    _check_vs_model(L, desc, 9, 2, _dense, dev, 7)


def test_two_launches_and_graph_replays_give_the_same_bits(dev):
    from vptq_amd import _backend as B
    L = layer(G5, 56, "v12-k65536-4096", "f16", perm=1, bias=1)
    desc, keep = expect_instance(spec_to_module(L, dev), 13, 3, "v12-k65536-4096")
    xt = bits_to_tensor(_dense(L.in_features, 13, "f16", 5)[0], "f16", dev).reshape(13, L.in_features)
    a, b = call(desc, xt, 56, 3), call(desc, xt, 56, 3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    yg = torch.full((13, 56), float("nan"), dtype=xt.dtype, device=dev)
    ws, need = workspace(desc, 13, 3, dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_gather12c(desc, xt.data_ptr(), yg.data_ptr(), 13, 0, 3, ws.data_ptr(), need, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    for _ in range(3):
        yg.fill_(float("nan"))
        ws.fill_(0xCD)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(a.view(torch.int16), yg.view(torch.int16))


def test_module_and_op_take_the_entry_with_the_knob_on(dev, monkeypatch):
    from vptq_amd import _backend as B, batched_decode as bd, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = layer(2048, 516, "v12-k65536-4096", "bf16", perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, 12, 0, "v12-k65536-4096")
    S = split(desc, 0, cus)[0]
    assert S >= 2 and f" parts={S} tpp={-(-4 // S)} " in instance(desc, 12, 0)          # the rule's split of the 4 tiles
    xt = bits_to_tensor(_dense(2048, 12, "bf16", 9)[0], "bf16", dev).reshape(1, 12, 2048)
    own = call(desc, xt.reshape(12, 2048), 516, 0)
    launches = (ENTRY, "vptq_quant_gemm_gather12", "vptq_quant_gemm_gatherx", "vptq_quant_gemm_gather_px", "vptq_quant_gemv", "vptq_dequant")
    real = B.lib()
    for knob, took in (("0", False), ("1", True)):
        monkeypatch.setattr(bd, "_GEMM_GATHER12C_MODE", knob)
        for run in (lambda: m(xt), lambda: ops.quant_gemm(xt, **_op_keywords(m))):
            calls = []
            monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
            y = run()
            monkeypatch.setattr(B, "lib", lambda: real)
            assert ([c for c in calls if c in launches] == [ENTRY]) == took and (ENTRY in calls) == took, calls
            if took:
                assert y.shape == (1, 12, 516) and torch.equal(y.view(torch.int16).reshape(12, 516), own.view(torch.int16))
    assert torch.equal(ops.quant_gemm_gather12c(xt, desc, 516).view(torch.int16).reshape(12, 516), own.view(torch.int16))
    assert torch.equal(ops.quant_gemm_gather12c(xt, desc, 516, parts=S).view(torch.int16).reshape(12, 516), own.view(torch.int16))
