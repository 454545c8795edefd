"""vptq_quant_gemm_gather (gemm_gather.hip): 1 - 16 tokens of the large-codebook formats in one launch, on the GPU.

TILE = 1024 columns per tile and R = 2 vector-rows per row group are the kernel's; the shapes are the smallest that reach each edge.
Every call writes into a buffer whose token rows are NaN and sit between sentinel guard rows: an output the launch does not write
stays NaN, a store outside the rows breaks a guard.

  1. weights bit for bit: one-hot activations pick columns of W, which must be vptq_dequant's bits (-0 == +0)
  2. sums: dense and spiky activations against the per-output float64 model of the reference's roundings (tests/_arith_model.py,
     check_both, its bounds unchanged), 16-bit and VPTQ_GEMV_OUT_F32 outputs; token rows past `tokens` do not leak
  3. tokens <= 8: agreement with vptq_quant_gemv (both the reference's roundings; only the summation order differs, so the fp32
     outputs are within twice the model's fp32 bound of each other)
  4. two launches and a graph replay give identical bits
  5. VQuantLinear.forward with 12 tokens takes the entry where gemm_gather_route says so; a compact layer gives its packed twin's bits
Each row asserts its instance string first."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, gemv_abi, module_desc

pytestmark = pytest.mark.gpu

TILE, R = 1024, 2
GUARD = 2
SENTINEL = 12345.0
KR = {16: 0, 24: 256, 32: 65536}
F32 = 1 << 5


def layer(I, O, T, dt, perm=0, bias=0, dist="llm"):
    return vo.make_layer(I, O, dist=dist, seed=I + O + T, dtype=dt, vector_len=8, num_centroids=65536, num_res_centroids=KR[T],
                         enable_perm=bool(perm), bias=bool(bias), enable_norm=True)


def instance(desc, tokens, flags=0):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_gather_instance(desc, tokens, flags, buf, len(buf)), "vptq_quant_gemm_gather_instance")
    return buf.value.decode()


def expect_instance(m, L, tokens, T):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = (L.num_indices + R - 1) // R
    grid = min(groups, 4 * cus)
    want = (f"gemm_gather dt={L.dtype} t={T} perm={int(L.perm is not None)} tok={tokens} tiles={(L.in_features + TILE - 1) // TILE} "
            f"rgs={(groups + grid - 1) // grid}")
    desc, keep = module_desc(m)
    assert B.lib().vptq_quant_gemm_gather_supported(desc, tokens) == 1
    assert instance(desc, tokens) == want
    return desc, keep


def call(desc, xt, O, out_f32=False, flags=0, stream=None):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    B.check(B.lib().vptq_quant_gemm_gather(desc, xt.data_ptr(), y.data_ptr(), tokens, flags | (F32 if out_f32 else 0),
                                           B.current_stream_ptr(xt.device)), "vptq_quant_gemm_gather")
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


# ---------------------------------------------------------------------------------------------- 1. weights bit for bit
G1, O1 = TILE + 8, 8 * R + 4
COLS1 = [0, 1, 7, 8, 63, 64, 300, 511, 512, TILE - 2, TILE - 1, TILE, TILE + 1, G1 - 3, G1 - 2, G1 - 1]


@pytest.mark.parametrize("T,dt,perm", list(itertools.product((16, 24, 32), ("f16", "bf16"), (0, 1))))
def test_one_hot_activations_read_dequant_bits(T, dt, perm, dev):
    L = layer(G1, O1, T, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 16, T)
    W = m.dequant()
    x = torch.zeros(16, G1, dtype=W.dtype, device=dev)
    x[torch.arange(16), torch.tensor(COLS1)] = 1.0
    y = call(desc, x, O1)
    want = W[:, torch.tensor(COLS1, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want).all()), f"{int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 2. sums against the float64 model
GS = [8, TILE - 8, TILE, TILE + 8, 2 * TILE + 264]
TOKS = [1, 5, 8, 9, 15, 16]


def _sum_rows():
    rows = []
    for i, (T, dt, G) in enumerate(itertools.product((16, 24, 32), ("f16", "bf16"), GS)):
        # the other axes cycle with periods 6, 2, 2, 2, 2, 2 at different strides, so that every value meets every T and dtype
        tokens = TOKS[(i + i // 6) % 6]
        N = (1, R + 1)[(i // 2 + i // 10) % 2]   # (R - 1 = 1)
        rows.append(pytest.param(dict(T=T, dt=dt, G=G, tokens=tokens, perm=(i + i // 5) % 2, bias=(i // 3 + i // 15) % 2, N=N,
                                      O=N * 8 - 4 * ((i // 4 + i // 7) % 2), x=("dense", "planted")[(i + i // 2) % 2]),
                                 id=f"t{T}-{dt}-G{G}-tok{tokens}-i{i}"))
    return rows


def _x(e, L):
    kind = _dense if e["x"] == "dense" else _planted
    kw = dict(perm=L.perm) if e["x"] == "planted" else {}
    return kind(L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"], **kw)[0]


@pytest.mark.parametrize("e", _sum_rows())
def test_sums_vs_the_exact_model(e, dev):
    L = layer(e["G"], e["O"], e["T"], e["dt"], perm=e["perm"], bias=e["bias"])
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, e["tokens"], e["T"])
    x = _x(e, L)
    xt = bits_to_tensor(x, L.dtype, dev).reshape(e["tokens"], L.in_features)
    y16, y32 = _np(call(desc, xt, e["O"])), _np(call(desc, xt, e["O"], out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, e["tokens"]))


@pytest.mark.parametrize("T,dt", [(24, "f16"), (32, "bf16")])
def test_more_row_groups_than_resident_workgroups(T, dt, dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = R * 4 * cus + 3                     # more row groups than workgroups of the launch (and than 2 x the CU count); a spare row
    L = layer(64, N * 8 - 4, T, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 9, T)
    assert instance(desc, 9).endswith("rgs=2")
    x = _dense(64, 9, dt, 7)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(9, 64)
    y16, y32 = _np(call(desc, xt, L.out_features)), _np(call(desc, xt, L.out_features, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, dt, what=instance(desc, 9))


@pytest.mark.parametrize("T,dt", [(16, "bf16"), (24, "f16"), (32, "f16")])
def test_token_rows_past_tokens_do_not_leak(T, dt, dev):
    L = layer(TILE + 8, 8 * R + 4, T, dt, perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 5, T)
    x = bits_to_tensor(_dense(L.in_features, 16, dt, 3)[0], dt, dev).reshape(16, L.in_features)
    x[5:] *= 1000.0   # (what rows 5 .. 15 hold must not matter to rows 0 .. 4)
    for f32 in (False, True):
        y5, y16 = call(desc, x[:5].contiguous(), L.out_features, out_f32=f32), call(desc, x, L.out_features, out_f32=f32)
        assert torch.equal(y5.view(torch.int16 if not f32 else torch.int32), y16[:5].view(torch.int16 if not f32 else torch.int32))


# ---------------------------------------------------------------------------------------------- 3. the route it replaces
@pytest.mark.parametrize("T,dt,tokens,perm", [(16, "f16", 8, 0), (24, "bf16", 5, 1), (32, "f16", 1, 1), (24, "f16", 8, 0), (32, "bf16", 8, 0),
                                              (16, "bf16", 5, 1)])
def test_agrees_with_gemv_gather(T, dt, tokens, perm, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 8 * (R + 1) - 4, T, dt, perm=perm, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, T)
    assert B.lib().vptq_quant_gemv_kernel_name(desc, tokens, 0) == b"gemv_gather_kernel"
    x = _dense(L.in_features, tokens, dt, 11)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(tokens, L.in_features)
    new = _np(call(desc, xt, L.out_features, out_f32=True))
    old = _np(gemv_abi(m, xt, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_outputs(new, mm, aa, dt, True, what="gemm_gather [fp32]")
    am.check_outputs(old, mm, aa, dt, True, what="gemv_gather [fp32]")
    assert (np.abs(new - old) <= 2 * am.REL * aa).all()


# ---------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("T,dt", [(16, "f16"), (24, "bf16"), (32, "f16")])
def test_two_launches_and_a_graph_replay_give_the_same_bits(T, dt, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 8 * (R + 1), T, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 13, T)
    xt = bits_to_tensor(_dense(L.in_features, 13, dt, 5)[0], dt, dev).reshape(13, L.in_features)
    a, b = call(desc, xt, L.out_features), call(desc, xt, L.out_features)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    yg = torch.full((13, L.out_features), float("nan"), dtype=xt.dtype, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_gather(desc, xt.data_ptr(), yg.data_ptr(), 13, 0, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(a.view(torch.int16), yg.view(torch.int16))


# ---------------------------------------------------------------------------------------------- 5. the module
class _Spy:
    """B.lib() with the names of the entries called through it recorded"""
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("vptq_quant_gemm_gather") and name not in ("vptq_quant_gemv", "vptq_dequant"):
            return fn

        def spy(*a):
            self._calls.append(name)
            return fn(*a)
        return spy


@pytest.mark.parametrize("T,dt", [(24, "f16"), (16, "bf16")])
def test_module_takes_the_entry_where_the_route_says_so(T, dt, dev, monkeypatch):
    from vptq_amd import _backend as B
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    L = layer(2048, 512, T, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 12, T)
    x = _dense(2048, 12, dt, 9)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(1, 12, 2048)
    routed = vq.gemm_gather_route(8, 65536, KR[T], 512, 2048, 12)
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    y = m(xt)
    monkeypatch.undo()
    launches = [c for c in calls if c in ("vptq_quant_gemm_gather", "vptq_quant_gemv", "vptq_dequant")]
    assert launches == (["vptq_quant_gemm_gather"] if routed else ["vptq_dequant"]), launches
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    if routed:
        am.check_outputs(_np(y), mm, aa, dt, False, what="VQuantLinear.forward, 12 tokens")
    # the route function on: the entry itself, and a compact layer against its packed twin
    monkeypatch.setattr(bd, "_GEMM_GATHER_MODE", "1")
    y1 = m(xt)
    am.check_outputs(_np(y1), mm, aa, dt, False, what="VQuantLinear.forward, 12 tokens, routed")
    m2 = spec_to_module(L, dev)
    m2.compact(force=True)
    assert m2.is_compact()
    calls2 = []
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls2))
    y2 = m2(xt)
    monkeypatch.undo()
    assert "vptq_quant_gemm_gather" in calls2 and "vptq_dequant" not in calls2
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
