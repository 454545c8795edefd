"""vptq_quant_gemm_gatherx (gemm_gatherx.hip): 1 - 16 tokens of the large-codebook formats vptq_quant_gemm_gather does not own (vector
length 8 / 16, any total index width) in one launch, on the GPU.  Modelled on tests/test_gemm_gather_gpu.py.

TILE = 1024 columns per tile and 16 outputs per row group (V = 8: two vector-rows, V = 16: one, its two 16-byte half-entries in the two
thread halves) are the kernel's; the shapes are the smallest that reach each edge.  The formats are chosen by what the index path can
get wrong - T = index_bits + res_bits: 16 (whole words), 32 (one word per element), 31 (the 9-word window), 26 / 22 / 28 / 18 (windows
at every byte offset; residual tables in LDS, 64 bytes ... 32 KiB, and from L2), 15 (no residual, odd width).  Every call writes into
a buffer whose token rows are NaN and sit between sentinel guard rows.

  1. weights bit for bit: one-hot activations pick columns of W, which must be vptq_dequant's bits (-0 == +0)
  2. sums: dense and planted activations against the per-output float64 model of the reference's roundings (tests/_arith_model.py,
     check_both, its bounds unchanged), 16-bit and VPTQ_GEMV_OUT_F32 outputs; token rows past `tokens` do not leak
  3. more row groups than resident workgroups (rgs=2)
  4. agreement with vptq_quant_gemv (both the reference's roundings; only the summation order differs, so the fp32 outputs are within
     twice the model's fp32 bound of each other)
  5. two launches and a graph replay give identical bits
  6. VQuantLinear.forward with 12 tokens takes the entry where gemm_gatherx_route says so; a compact layer gives its packed twin's bits
Each row asserts its instance string first."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gatherx_cpu import want
from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, gemv_abi, module_desc

pytestmark = pytest.mark.gpu

TILE = 1024
# name -> (vector length, main centroids, residual centroids); T = log2 k + log2 kr
FMT = {"v16-k65536-0": (16, 65536, 0), "v16-k65536-65536": (16, 65536, 65536), "v16-k65536-32768": (16, 65536, 32768),
       "v16-k65536-1024": (16, 65536, 1024), "v16-k65536-64": (16, 65536, 64), "v8-k65536-4096": (8, 65536, 4096),
       "v8-k65536-4": (8, 65536, 4), "v8-k32768-0": (8, 32768, 0)}
BITS = {"v16-k65536-0": 16, "v16-k65536-65536": 32, "v16-k65536-32768": 31, "v16-k65536-1024": 26, "v16-k65536-64": 22,
        "v8-k65536-4096": 28, "v8-k65536-4": 18, "v8-k32768-0": 15}


def layer(I, O, fmt, dt, perm=0, bias=0, dist="llm"):
    v, k, kr = FMT[fmt]
    L = vo.make_layer(I, O, dist=dist, seed=I + O + BITS[fmt], dtype=dt, vector_len=v, num_centroids=k, num_res_centroids=kr,
                      enable_perm=bool(perm), bias=bool(bias), enable_norm=True)
    return L


def instance(desc, tokens, flags=0):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_gatherx_instance(desc, tokens, flags, buf, len(buf)), "vptq_quant_gemm_gatherx_instance")
    return buf.value.decode()


def expect_instance(m, L, tokens, fmt):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    desc, keep = module_desc(m)
    assert desc.index_bits + desc.res_bits == BITS[fmt] and desc.vector_len == FMT[fmt][0]
    assert B.lib().vptq_quant_gemm_gatherx_supported(desc, tokens) == 1 and B.lib().vptq_quant_gemm_gather_supported(desc, tokens) == 0
    text = instance(desc, tokens)
    assert text == want(desc, tokens, cus), (text, want(desc, tokens, cus))
    return desc, keep


def call(desc, xt, O, out_f32=False, flags=0):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    B.check(B.lib().vptq_quant_gemm_gatherx(desc, xt.data_ptr(), y.data_ptr(), tokens, flags | (F32 if out_f32 else 0),
                                            B.current_stream_ptr(xt.device)), "vptq_quant_gemm_gatherx")
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


# ---------------------------------------------------------------------------------------------- 1. weights bit for bit
G1, O1 = TILE + 8, 20   # V = 8: three vector-rows, the last ragged; V = 16: two, the upper half-entry of the second wholly masked
COLS1 = [0, 1, 7, 8, 63, 64, 300, 511, 512, TILE - 2, TILE - 1, TILE, TILE + 1, G1 - 3, G1 - 2, G1 - 1]


@pytest.mark.parametrize("fmt,dt,perm", list(itertools.product(FMT, ("f16", "bf16"), (0, 1))))
def test_one_hot_activations_read_dequant_bits(fmt, dt, perm, dev):
    L = layer(G1, O1, fmt, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 16, fmt)
    W = m.dequant()
    x = torch.zeros(16, G1, dtype=W.dtype, device=dev)
    x[torch.arange(16), torch.tensor(COLS1)] = 1.0
    y = call(desc, x, O1)
    want_w = W[:, torch.tensor(COLS1, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want_w).all()), f"{int((y != want_w).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 2. sums against the float64 model
GS = [8, TILE - 8, TILE, TILE + 8, 2 * TILE + 264]
TOKS = [1, 5, 8, 9, 15, 16]


def _sum_rows():
    rows = []
    for i, (fmt, dt, G) in enumerate(itertools.product(FMT, ("f16", "bf16"), GS)):
        # the other axes cycle with short periods at different strides, so that every value meets every format, G and dtype
        v = FMT[fmt][0]
        tokens = TOKS[(i + i // 6) % 6]
        N = (1, 3)[(i // 2 + i // 10) % 2]
        cut = ((0, 4), (0, 4, 12))[v == 16]   # O = V N, V N - 4 (a ragged last row), V = 16: V N - 12 (the upper half-entry wholly masked)
        rows.append(pytest.param(dict(fmt=fmt, dt=dt, G=G, tokens=tokens, perm=(i + i // 5) % 2, bias=(i // 3 + i // 15) % 2, N=N,
                                      O=N * v - cut[(i // 4 + i // 7) % len(cut)], x=("dense", "planted")[(i + i // 2) % 2]),
                                 id=f"{fmt}-{dt}-G{G}-tok{tokens}-i{i}"))
    return rows


def _x(e, L):
    kind = _dense if e["x"] == "dense" else _planted
    kw = dict(perm=L.perm) if e["x"] == "planted" else {}
    return kind(L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"], **kw)[0]


@pytest.mark.parametrize("e", _sum_rows())
def test_sums_vs_the_exact_model(e, dev):
    L = layer(e["G"], e["O"], e["fmt"], e["dt"], perm=e["perm"], bias=e["bias"])
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, e["tokens"], e["fmt"])
    x = _x(e, L)
    xt = bits_to_tensor(x, L.dtype, dev).reshape(e["tokens"], L.in_features)
    y16, y32 = _np(call(desc, xt, e["O"])), _np(call(desc, xt, e["O"], out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, e["tokens"]))


@pytest.mark.parametrize("fmt,dt", [("v8-k32768-0", "f16"), ("v16-k65536-1024", "bf16")])
def test_more_row_groups_than_resident_workgroups(fmt, dt, dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    v = FMT[fmt][0]
    wgcu = 4 if fmt == "v8-k32768-0" else 2      # 32 KiB of LDS / 32 + 32 KiB
    N = (16 // v) * wgcu * cus + 3               # more row groups than workgroups of the launch; spare rows
    L = layer(64, N * v - 4, fmt, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 9, fmt)
    assert instance(desc, 9).endswith(f"wgcu={wgcu} rgs=2")
    x = _dense(64, 9, dt, 7)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(9, 64)
    y16, y32 = _np(call(desc, xt, L.out_features)), _np(call(desc, xt, L.out_features, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, dt, what=instance(desc, 9))


@pytest.mark.parametrize("fmt,dt", [("v16-k65536-0", "bf16"), ("v16-k65536-1024", "f16"), ("v16-k65536-32768", "f16"), ("v8-k65536-4096", "bf16")])
def test_token_rows_past_tokens_do_not_leak(fmt, dt, dev):
    L = layer(TILE + 8, 20, fmt, dt, perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 5, fmt)
    x = bits_to_tensor(_dense(L.in_features, 16, dt, 3)[0], dt, dev).reshape(16, L.in_features)
    x[5:] *= 1000.0   # (what rows 5 .. 15 hold must not matter to rows 0 .. 4)
    for f32 in (False, True):
        y5, y16 = call(desc, x[:5].contiguous(), L.out_features, out_f32=f32), call(desc, x, L.out_features, out_f32=f32)
        assert torch.equal(y5.view(torch.int16 if not f32 else torch.int32), y16[:5].view(torch.int16 if not f32 else torch.int32))


# ---------------------------------------------------------------------------------------------- 4. the route it replaces
@pytest.mark.parametrize("fmt,dt,tokens,perm", [("v16-k65536-0", "f16", 4, 0), ("v16-k65536-1024", "bf16", 3, 1), ("v16-k65536-65536", "f16", 1, 1),
                                                ("v16-k65536-32768", "bf16", 2, 0), ("v16-k65536-64", "f16", 4, 1),
                                                ("v8-k65536-4096", "f16", 8, 0), ("v8-k65536-4", "bf16", 5, 1), ("v8-k32768-0", "f16", 7, 1)])
def test_agrees_with_gemv_gatherx(fmt, dt, tokens, perm, dev):
    from vptq_amd import _backend as B
    v = FMT[fmt][0]
    L = layer(2 * TILE + 264, v * 3 - 4, fmt, dt, perm=perm, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, fmt)
    assert B.lib().vptq_quant_gemv_kernel_name(desc, tokens, 0) == b"gemv_gatherx_kernel"
    x = _dense(L.in_features, tokens, dt, 11)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(tokens, L.in_features)
    new = _np(call(desc, xt, L.out_features, out_f32=True))
    old = _np(gemv_abi(m, xt, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_outputs(new, mm, aa, dt, True, what="gemm_gatherx [fp32]")
    am.check_outputs(old, mm, aa, dt, True, what="gemv_gatherx [fp32]")
    assert (np.abs(new - old) <= 2 * am.REL * aa).all()


# ---------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("fmt,dt", [("v16-k65536-0", "f16"), ("v16-k65536-1024", "bf16"), ("v16-k65536-65536", "f16"), ("v8-k65536-4", "bf16")])
def test_two_launches_and_a_graph_replay_give_the_same_bits(fmt, dt, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, FMT[fmt][0] * 3, fmt, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 13, fmt)
    xt = bits_to_tensor(_dense(L.in_features, 13, dt, 5)[0], dt, dev).reshape(13, L.in_features)
    a, b = call(desc, xt, L.out_features), call(desc, xt, L.out_features)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    yg = torch.full((13, L.out_features), float("nan"), dtype=xt.dtype, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_gatherx(desc, xt.data_ptr(), yg.data_ptr(), 13, 0, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(a.view(torch.int16), yg.view(torch.int16))


# ---------------------------------------------------------------------------------------------- 6. the module
@pytest.mark.parametrize("fmt,dt", [("v16-k65536-1024", "f16"), ("v16-k65536-0", "bf16"), ("v8-k65536-4096", "bf16")])
def test_module_takes_the_entry_where_the_route_says_so(fmt, dt, dev, monkeypatch):
    from vptq_amd import _backend as B
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    v, k, kr = FMT[fmt]
    L = layer(2048, 512, fmt, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 12, fmt)
    x = _dense(2048, 12, dt, 9)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(1, 12, 2048)
    routed = vq.gemm_gatherx_route(v, k, kr, 512, 2048, 12)
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    y = m(xt)
    monkeypatch.undo()
    launches = [c for c in calls if c in ("vptq_quant_gemm_gatherx", "vptq_quant_gemm_gather", "vptq_quant_gemv", "vptq_dequant")]
    assert launches == (["vptq_quant_gemm_gatherx"] if routed else ["vptq_dequant"]), launches
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    if routed:
        am.check_outputs(_np(y), mm, aa, dt, False, what="VQuantLinear.forward, 12 tokens")
    # the route function on: always the entry itself ...
    monkeypatch.setattr(bd, "_GEMM_GATHERX_MODE", "1")
    calls1 = []
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls1))
    y1 = m(xt)
    monkeypatch.setattr(B, "lib", lambda: real)
    assert [c for c in calls1 if c in ("vptq_quant_gemm_gatherx", "vptq_quant_gemm_gather", "vptq_quant_gemv", "vptq_dequant")] == ["vptq_quant_gemm_gatherx"]
    am.check_outputs(_np(y1), mm, aa, dt, False, what="VQuantLinear.forward, 12 tokens, routed")
    if fmt != "v16-k65536-0":
        return
    # ... and a compacted layer (v16-k65536-0 has exact sliced layouts) against its packed twin, without vptq_dequant
    m2 = spec_to_module(L, dev)
    m2.compact(force=True)
    assert m2.is_compact()
    calls2 = []
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls2))
    y2 = m2(xt)
    monkeypatch.setattr(B, "lib", lambda: real)
    assert "vptq_quant_gemm_gatherx" in calls2 and "vptq_dequant" not in calls2
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
