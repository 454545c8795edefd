"""vptq_quant_gemm_gather12w (gemm_gather12w.hip): 17 - 48 tokens of gemm_gather12's layers as 2 / 3 token blocks over (row group, column
part) items, on the GPU.  Widths TILE + 8, 2 TILE and 4 TILE + 264 (five tiles, the last ragged); tokens 17 (a block with one live
token), 24 / 47 (a ragged last block), 32 / 48 (a full one), 33.  Every call asserts its instance string, writes into NaN token rows
between sentinel guard rows and has a 0xAB-filled workspace."""
import ctypes as C
import itertools

import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gather_px_gpu import _op_keywords
from test_gemm_gather12_gpu import layer, FMT, BITS, TILE, call as call12
from test_gemm_gather12c_gpu import call as call12c
from test_gemm_gather12w_cpu import want, split
import _arith_model as am
from vptq_amd import _backend as B
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu

ENTRY, G5 = "vptq_quant_gemm_gather12w", 4 * TILE + 264


def instance(desc, tokens, parts):
    buf = C.create_string_buffer(320)
    B.check(B.lib().vptq_quant_gemm_gather12w_instance(desc, tokens, 0, parts, buf, len(buf)), ENTRY + "_instance")
    return buf.value.decode()


def expect_instance(m, tokens, parts, fmt):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    desc, keep = module_desc(m)
    assert desc.index_bits + desc.res_bits == BITS[fmt] and desc.vector_len == 12 and B.lib().vptq_quant_gemm_gather12w_supported(desc, tokens, parts) == 1
    text = instance(desc, tokens, parts)
    assert text == want(desc, tokens, parts, cus), (text, want(desc, tokens, parts, cus))
    return desc, keep


def workspace(desc, tokens, parts, dev, fill=0xAB):
    need = B.lib().vptq_quant_gemm_gather12w_workspace_bytes(desc, tokens, parts)
    assert (need > 0) == (bool(desc.perm) or split(desc, tokens, parts)[0] >= 2)
    return torch.full((max(need, 16),), fill, dtype=torch.uint8, device=dev), need


def call(desc, xt, O, parts, out_f32=False):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    ws, need = workspace(desc, tokens, parts, xt.device)
    B.check(B.lib().vptq_quant_gemm_gather12w(desc, xt.data_ptr(), y.data_ptr(), tokens, F32 if out_f32 else 0, parts, ws.data_ptr(), need,
                                              B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


# both sides of every tile (= part) boundary, the first chunk, the ragged tile's last columns, then others: the first 32 serve two blocks
COLS = [c for b in range(TILE, G5, TILE) for c in (b - 1, b)] + [0, 7, G5 - 3, G5 - 2, G5 - 1, 300] + \
       [c for b in range(TILE, G5, TILE) for c in (b - 9, b - 8, b + 7, b + 8)] + [8, 100, 700, 1100, 1300, 1800, 1900, 2100, 2200, 2250, 2290, G5 - 9, G5 - 8, 411, 1500, 63, 64, 130]
WEIGHT_ROWS = [(48,) + c for c in itertools.product(FMT, ("f16", "bf16"), (0, 1))] + \
              [(32, f, d, i % 2) for i, (f, d) in enumerate(itertools.product(("v12-k65536-0", "v12-k65536-256", "v12-k65536-4096"), ("f16", "bf16")))]


@pytest.mark.parametrize("i,tokens,fmt,dt,perm", [(i,) + c for i, c in enumerate(WEIGHT_ROWS)])
def test_one_hot_activations_read_dequant_bits(i, tokens, fmt, dt, perm, dev):
    parts = (1, 2, 3, 5)[(i + i // 4) % 4]
    L = layer(G5, 56, fmt, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, tokens, parts, fmt)
    assert split(desc, tokens, parts)[0] == parts and len(set(COLS)) == len(COLS) == 48
    W = m.dequant()
    cols = torch.tensor([int(L.perm[c]) for c in COLS[:tokens]] if perm else COLS[:tokens])
    x = torch.zeros(tokens, G5, dtype=W.dtype, device=dev)
    x[torch.arange(tokens), cols] = 1.0
    y = call(desc, x, 56, parts)
    want_w = W[:, cols.to(dev)].t()
    assert not bool(torch.isnan(y).any()) and bool((y == want_w).all()), f"{int((y != want_w).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


SHAPES, TOKS = [(TILE + 8, 1), (TILE + 8, 2), (2 * TILE, 2), (G5, 1), (G5, 3), (G5, 5)], [17, 24, 32, 33, 47, 48]   # SHAPES: (G, parts)


def _sum_rows():
    rows = []
    for i, (fmt, dt, (G, parts)) in enumerate(itertools.product(FMT, ("f16", "bf16"), SHAPES)):
        # the other axes cycle (test_gemm_gather12c_gpu._sum_rows); every (dtype, residual form, token blocks) meets one part and a split
        tokens = TOKS[(i + i // 6 + 3 * (i // 12)) % 6]
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


@pytest.mark.parametrize("fmt,dt,G,parts,tokens,perm,bias", [
    ("v12-k65536-4096", "f16", G5, 1, 48, 1, 1), ("v12-k65536-256", "bf16", G5, 3, 47, 0, 1), ("v12-k65536-0", "f16", TILE + 8, 2, 33, 1, 0),
    ("v12-k32768-1024", "bf16", 2 * TILE, 1, 24, 0, 0), ("v12-k65536-4096", "bf16", G5, 5, 32, 0, 1), ("v12-k65536-0", "bf16", G5, 2, 17, 1, 1)])
def test_a_token_has_the_bits_of_the_16_token_entries(fmt, dt, G, parts, tokens, perm, bias, dev):
    L = layer(G, 56, fmt, dt, perm=perm, bias=bias)
    desc, keep = expect_instance(spec_to_module(L, dev), tokens, parts, fmt)
    xt = bits_to_tensor(_dense(G, tokens, dt, 11)[0], dt, dev).reshape(tokens, G)
    y = call(desc, xt, 56, parts)
    for b in range(0, tokens, 16):
        xs = xt[b:b + 16].contiguous()
        other = call12(desc, xs, 56) if parts == 1 else call12c(desc, xs, 56, parts)
        assert torch.equal(y[b:b + 16].view(torch.int16), other.view(torch.int16)), (b, instance(desc, tokens, parts))


def test_more_items_than_resident_workgroups(dev):
    fmt, probe = "v12-k65536-256", module_desc(spec_to_module(layer(TILE + 8, 56, "v12-k65536-256", "bf16"), dev))[0]
    slots = torch.cuda.get_device_properties(0).multi_processor_count * int(instance(probe, 33, 2).split(" wgcu=")[1].split()[0])
    N = 4 * (slots // 2 + 2) - 1                 # slots / 2 + 2 row groups x 2 parts; a ragged last group
    L = layer(TILE + 8, N * 12 - 4, fmt, "bf16", bias=1)
    desc, keep = expect_instance(spec_to_module(L, dev), 33, 2, fmt)
    assert " parts=2 tpp=1 " in instance(desc, 33, 2) and " rgs=2 | " in instance(desc, 33, 2)
    _check_vs_model(L, desc, 33, 2, _dense, dev, 7)


def test_two_launches_and_graph_replays_give_the_same_bits(dev):
    L = layer(G5, 56, "v12-k65536-4096", "f16", perm=1, bias=1)
    desc, keep = expect_instance(spec_to_module(L, dev), 37, 3, "v12-k65536-4096")
    xt = bits_to_tensor(_dense(L.in_features, 37, "f16", 5)[0], "f16", dev).reshape(37, L.in_features)
    a, b = call(desc, xt, 56, 3), call(desc, xt, 56, 3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    yg = torch.full((37, 56), float("nan"), dtype=xt.dtype, device=dev)
    ws, need = workspace(desc, 37, 3, dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_gather12w(desc, xt.data_ptr(), yg.data_ptr(), 37, 0, 3, ws.data_ptr(), need, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    for _ in range(3):
        yg.fill_(float("nan"))
        ws.fill_(0xCD)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(a.view(torch.int16), yg.view(torch.int16))


def test_module_and_op_take_the_entry_with_the_knob_on(dev, monkeypatch):
    from vptq_amd import batched_decode as bd, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = layer(2048, 516, "v12-k65536-4096", "bf16", perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, 40, 0, "v12-k65536-4096")
    S = split(desc, 40, 0, cus)[0]
    assert S >= 2 and f" parts={S} tpp={-(-4 // S)} " in instance(desc, 40, 0)          # the rule's split of the 4 tiles
    xt = bits_to_tensor(_dense(2048, 40, "bf16", 9)[0], "bf16", dev).reshape(1, 40, 2048)
    own = call(desc, xt.reshape(40, 2048), 516, 0)
    launches = (ENTRY, "vptq_quant_gemm_gather12", "vptq_quant_gemm_gather12c", "vptq_quant_gemm_gatherxw", "vptq_quant_gemm_gather_px",
                "vptq_quant_gemv", "vptq_dequant")
    real = B.lib()
    for knob, took in (("0", False), ("1", True)):
        monkeypatch.setattr(bd, "_GEMM_GATHER12W_MODE", knob)
        for run in (lambda: m(xt), lambda: ops.quant_gemm(xt, **_op_keywords(m))):
            calls = []
            monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
            y = run()
            monkeypatch.setattr(B, "lib", lambda: real)
            assert ([c for c in calls if c in launches] == [ENTRY]) == took and (ENTRY in calls) == took, calls
            if took:
                assert y.shape == (1, 40, 516) and torch.equal(y.view(torch.int16).reshape(40, 516), own.view(torch.int16))
    assert torch.equal(ops.quant_gemm_gather12w(xt, desc, 516).view(torch.int16).reshape(40, 516), own.view(torch.int16))
    assert torch.equal(ops.quant_gemm_gather12w(xt, desc, 516, parts=S).view(torch.int16).reshape(40, 516), own.view(torch.int16))
