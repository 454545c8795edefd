"""vptq_quant_gemm_gather12 (gemm_gather12.hip): 1 - 16 tokens of the vector-length-12 large-codebook formats in one launch, on the GPU.
TILE = 512 columns and 48 outputs per row group (4 vector-rows = three MFMA N blocks) are the kernel's; the shapes are the smallest
that reach each edge.  T = 16 (no residual), 24 (6 KiB table in LDS), 25 (odd: windows at every byte offset; 24 KiB in LDS), 28 (the
published v12-k65536-4096: 96 KiB from L2).  Every call writes into NaN token rows between sentinel guard rows, and asserts its instance
string first: weights bit for bit, sums against the fp64 model, rgs = 2, repeatability, the public path."""
import ctypes as C
import itertools

import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gather_px_gpu import _op_keywords
from test_gemm_gather12_cpu import want
from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu

TILE = 512
FMT = {"v12-k65536-0": (65536, 0), "v12-k65536-256": (65536, 256), "v12-k32768-1024": (32768, 1024), "v12-k65536-4096": (65536, 4096)}
BITS = {"v12-k65536-0": 16, "v12-k65536-256": 24, "v12-k32768-1024": 25, "v12-k65536-4096": 28}
ENTRY = "vptq_quant_gemm_gather12"


def layer(I, O, fmt, dt, perm=0, bias=0):
    k, kr = FMT[fmt]
    return vo.make_layer(I, O, dist="llm", seed=I + O + BITS[fmt], dtype=dt, vector_len=12, num_centroids=k, num_res_centroids=kr,
                         enable_perm=bool(perm), bias=bool(bias), enable_norm=True)


def instance(desc, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_gather12_instance(desc, tokens, 0, buf, len(buf)), ENTRY + "_instance")
    return buf.value.decode()


def expect_instance(m, tokens, fmt):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    desc, keep = module_desc(m)
    assert desc.index_bits + desc.res_bits == BITS[fmt] and desc.vector_len == 12
    assert B.lib().vptq_quant_gemm_gather12_supported(desc, tokens) == 1
    text = instance(desc, tokens)
    assert text == want(desc, tokens, cus), (text, want(desc, tokens, cus))
    return desc, keep


def workspace(desc, tokens, dev):
    from vptq_amd import _backend as B
    need = B.lib().vptq_quant_gemm_gather12_workspace_bytes(desc, tokens)
    assert (need > 0) == bool(desc.perm)
    return torch.full((max(need, 16),), 0xAB, dtype=torch.uint8, device=dev), need


def call(desc, xt, O, out_f32=False):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    ws, need = workspace(desc, tokens, xt.device)
    B.check(B.lib().vptq_quant_gemm_gather12(desc, xt.data_ptr(), y.data_ptr(), tokens, F32 if out_f32 else 0, ws.data_ptr(), need,
                                             B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


G1, O1 = TILE + 8, 56   # five vector-rows: two row groups, the second holds one ragged row
COLS1 = [0, 1, 7, 8, 63, 64, 130, 300, 411, TILE - 2, TILE - 1, TILE, TILE + 1, G1 - 3, G1 - 2, G1 - 1]


@pytest.mark.parametrize("fmt,dt,perm", list(itertools.product(FMT, ("f16", "bf16"), (0, 1))))
def test_one_hot_activations_read_dequant_bits(fmt, dt, perm, dev):
    m = spec_to_module(layer(G1, O1, fmt, dt, perm=perm), dev)
    desc, keep = expect_instance(m, 16, fmt)
    W = m.dequant()
    x = torch.zeros(16, G1, dtype=W.dtype, device=dev)
    x[torch.arange(16), torch.tensor(COLS1)] = 1.0
    y = call(desc, x, O1)
    want_w = W[:, torch.tensor(COLS1, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want_w).all()), f"{int((y != want_w).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


GS = [8, TILE - 8, TILE, TILE + 8, 2 * TILE + 264]
TOKS = [1, 5, 8, 9, 15, 16]


def _sum_rows():
    rows = []
    for i, (fmt, dt, G) in enumerate(itertools.product(FMT, ("f16", "bf16"), GS)):
        # the other axes cycle with short periods at different strides, so that every value meets every format, G and dtype
        tokens = TOKS[(i + i // 6) % 6]
        N = (1, 2, 5)[(i // 2 + i // 10) % 3]
        rows.append(pytest.param(dict(fmt=fmt, dt=dt, G=G, tokens=tokens, perm=(i + i // 5) % 2, bias=(i // 3 + i // 15) % 2,
                                      O=12 * N - (0, 4, 8)[(i // 4 + i // 7) % 3], x=("dense", "planted")[(i + i // 2) % 2]),
                                 id=f"{fmt}-{dt}-G{G}-tok{tokens}-i{i}"))
    return rows


@pytest.mark.parametrize("e", _sum_rows())
def test_sums_vs_the_exact_model(e, dev):
    L = layer(e["G"], e["O"], e["fmt"], e["dt"], perm=e["perm"], bias=e["bias"])
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, e["tokens"], e["fmt"])
    kind, kw = (_dense, {}) if e["x"] == "dense" else (_planted, dict(perm=L.perm))
    x = kind(L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"], **kw)[0]
    xt = bits_to_tensor(x, L.dtype, dev).reshape(e["tokens"], L.in_features)
    y16, y32 = _np(call(desc, xt, e["O"])), _np(call(desc, xt, e["O"], out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, e["tokens"]))


def test_more_row_groups_than_resident_workgroups(dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 4 * 2 * cus + 3                          # more row groups (of 4 vector-rows) than the 2 workgroups per CU; a ragged last group
    L = layer(64, N * 12 - 4, "v12-k65536-256", "bf16", bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, 9, "v12-k65536-256")
    assert instance(desc, 9).endswith("wgcu=2 rgs=2")
    x = _dense(64, 9, "bf16", 7)[0]
    xt = bits_to_tensor(x, "bf16", dev).reshape(9, 64)
    y16, y32 = _np(call(desc, xt, L.out_features)), _np(call(desc, xt, L.out_features, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, "bf16", what=instance(desc, 9))


def test_two_launches_and_graph_replays_give_the_same_bits(dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 56, "v12-k65536-4096", "f16", perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, 13, "v12-k65536-4096")
    xt = bits_to_tensor(_dense(L.in_features, 13, "f16", 5)[0], "f16", dev).reshape(13, L.in_features)
    a, b = call(desc, xt, 56), call(desc, xt, 56)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    yg = torch.full((13, 56), float("nan"), dtype=xt.dtype, device=dev)
    ws, need = workspace(desc, 13, dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_gather12(desc, xt.data_ptr(), yg.data_ptr(), 13, 0, ws.data_ptr(), need, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    for _ in range(3):
        yg.fill_(float("nan"))
        ws.fill_(0xCD)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(a.view(torch.int16), yg.view(torch.int16))


def test_module_and_op_take_the_entry_with_the_knob_on(dev, monkeypatch):
    from vptq_amd import _backend as B, batched_decode as bd, ops
    L = layer(2048, 516, "v12-k65536-4096", "bf16", perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, 12, "v12-k65536-4096")
    xt = bits_to_tensor(_dense(2048, 12, "bf16", 9)[0], "bf16", dev).reshape(1, 12, 2048)
    own = call(desc, xt.reshape(12, 2048), 516)
    launches = ("vptq_quant_gemm_gather12", "vptq_quant_gemm_gatherx", "vptq_quant_gemm_gather_px", "vptq_quant_gemv", "vptq_dequant")
    real = B.lib()
    for knob, took in (("0", False), ("1", True)):
        monkeypatch.setattr(bd, "_GEMM_GATHER12_MODE", knob)
        for run in (lambda: m(xt), lambda: ops.quant_gemm(xt, **_op_keywords(m))):
            calls = []
            monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
            y = run()
            monkeypatch.setattr(B, "lib", lambda: real)
            assert ([c for c in calls if c in launches] == [ENTRY]) == took, calls
            if took:
                assert y.shape == (1, 12, 516) and torch.equal(y.view(torch.int16).reshape(12, 516), own.view(torch.int16))
    assert torch.equal(ops.quant_gemm_gather12(xt, desc, 516).view(torch.int16).reshape(12, 516), own.view(torch.int16))
