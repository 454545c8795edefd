"""vptq_quant_gemm_k256w (gemm_k256w_kernel in gemm_k256.hip): 17 - 64 tokens of the canonical format in one launch, on the GPU.

TILE = 1024 columns per tile and ROWS = 4 vector-rows (32 outputs) per row group are the kernel's; the shapes are the smallest that
reach each edge.  Every call writes into a buffer whose token rows are NaN and sit between sentinel guard rows: an output the launch
does not write stays NaN, a store outside the rows breaks a guard.

  1. weights bit for bit: one-hot activations in all four token blocks pick columns of W, which must be vptq_dequant's bits
  2. sums: dense and spiky activations against the per-output float64 model of the reference's roundings (tests/_arith_model.py,
     check_both, its bounds unchanged), 16-bit and VPTQ_GEMV_OUT_F32 outputs
  3. one launch shape per pass instantiation <NRG, TB> = <1, 2>, <1, 3>, <1, 4> with 2 and 3 row groups on the busiest workgroup
     (more row groups than workgroups), and one with a single row group
  4. token rows past `tokens` do not leak into the rows before them
  5. batch invariance: a token's bits do not depend on its slot or on the batch's size
  6. the route it replaces: the kernel keeps gemm_k256_kernel's K-step -> wave mapping and order of sums, so 40 tokens give the BITS
     of vptq_quant_gemv(VPTQ_GEMV_EXACT)'s three launches (asserted as equality, and both against the model)
  7. two launches and a graph replay give identical bits
  8. the real reference's outputs for 64 tokens through a 4096 x 4096 layer (tests/golden/big)
  9. VQuantLinear.forward takes the entry where gemm_k256w_route says so, and never in the folded arithmetic
Each row asserts its instance string first."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from oracle import vptq_oracle as vo
import _arith_model as am
from _cases import load_big, stored_rows, rel_err
from _gpu_util import spec_to_module, bits_to_tensor, tensor_to_bits, gemv_abi, module_desc

pytestmark = pytest.mark.gpu

TILE, ROWS = 1024, 4
GUARD = 2
SENTINEL = 12345.0
F32 = 1 << 5
EXACT = 1 << 2
TOL = {"f16": 1e-3, "bf16": 8e-3}   # (tests/test_hip_parity.py: the parity bound against the real reference)


def layer(I, O, dt, perm=0, bias=0, seed=None):
    return vo.make_layer(I, O, dist="llm", seed=I + O if seed is None else seed, dtype=dt, enable_perm=bool(perm), bias=bool(bias))


def instance(desc, tokens, flags=0):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_k256w_instance(desc, tokens, flags, buf, len(buf)), "vptq_quant_gemm_k256w_instance")
    return buf.value.decode()


def expect_instance(m, L, tokens):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = (L.num_indices + ROWS - 1) // ROWS
    grid = min(groups, cus)
    rgs, tb = (groups + grid - 1) // grid, (tokens + 15) // 16
    want = f"gemm_k256w dt={L.dtype} perm={int(L.perm is not None)} tok={tokens} tb={tb} rgs={rgs} pass=1x{tb}"
    desc, keep = module_desc(m)
    assert B.lib().vptq_quant_gemm_k256w_supported(desc, tokens) == 1
    assert instance(desc, tokens) == want
    return desc, keep


def call(desc, xt, O, out_f32=False, flags=0):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    B.check(B.lib().vptq_quant_gemm_k256w(desc, xt.data_ptr(), y.data_ptr(), tokens, flags | (F32 if out_f32 else 0),
                                          B.current_stream_ptr(xt.device)), "vptq_quant_gemm_k256w")
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


def _bits(y):
    return y.view(torch.int32 if y.dtype == torch.float32 else torch.int16)


def _xt(x, dt, dev, tokens, I):
    return bits_to_tensor(x, dt, dev).reshape(tokens, I)


# ---------------------------------------------------------------------------------------------- 1. weights bit for bit
G1, O1 = TILE + 8, 8 * ROWS + 4
_EDGE = [0, 1, 7, 8, 63, 64, 511, 512, TILE - 1, TILE, TILE + 1, G1 - 1]
# 64 columns: the edges first, the rest spread over the row; dealt round-robin so that every token block holds some of the edges
_REST = [c for c in range(15, G1, 17) if c not in _EDGE][:64 - len(_EDGE)]
COLS1 = [(_EDGE + _REST)[(i % 16) * 4 + i // 16] for i in range(64)]


@pytest.mark.parametrize("dt,perm", list(itertools.product(("f16", "bf16"), (0, 1))))
def test_one_hot_activations_read_dequant_bits(dt, perm, dev):
    assert len(set(COLS1)) == 64 and all(any(c in COLS1[16 * b:16 * b + 16] for c in _EDGE) for b in range(4))
    L = layer(G1, O1, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 64)
    W = m.dequant()
    x = torch.zeros(64, G1, dtype=W.dtype, device=dev)
    x[torch.arange(64), torch.tensor(COLS1)] = 1.0
    y = call(desc, x, O1)
    want = W[:, torch.tensor(COLS1, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want).all()), f"{int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 2. sums against the float64 model
GS = [8, TILE - 8, TILE, TILE + 8, 2 * TILE + 264]
TOKS = [17, 31, 32, 33, 47, 48, 49, 63, 64]


def _sum_rows():
    rows = []
    for i, (dt, G, tokens) in enumerate(itertools.product(("f16", "bf16"), GS, TOKS)):
        # 2 x 5 x 9 rows: every (dtype, G, tokens); the other axes cycle at different strides, so that every value of perm, bias,
        # N, O and the activation kind meets every dtype and every token-block count
        N = (1, 5)[(i // 2 + i // 9) % 2]
        rows.append(pytest.param(dict(dt=dt, G=G, tokens=tokens, perm=(i + i // 5) % 2, bias=(i // 3 + i // 7) % 2, N=N,
                                      O=N * 8 - 4 * ((i // 4 + i // 11) % 2), x=("dense", "planted")[(i + i // 2) % 2]),
                                 id=f"{dt}-G{G}-tok{tokens}-i{i}"))
    return rows


def _x(e, L):
    kind = _dense if e["x"] == "dense" else _planted
    kw = dict(perm=L.perm) if e["x"] == "planted" else {}
    return kind(L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"], **kw)[0]


@pytest.mark.parametrize("e", _sum_rows())
def test_sums_vs_the_exact_model(e, dev):
    L = layer(e["G"], e["O"], e["dt"], perm=e["perm"], bias=e["bias"])
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, e["tokens"])
    x = _x(e, L)
    xt = _xt(x, L.dtype, dev, e["tokens"], L.in_features)
    y16, y32 = _np(call(desc, xt, e["O"])), _np(call(desc, xt, e["O"], out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, e["tokens"]))


# ---------------------------------------------------------------------------------------------- 3. every pass instantiation
@pytest.mark.parametrize("dt,tokens,height,passes", [("f16", 32, 2, "1x2"), ("bf16", 24, 3, "1x2"), ("bf16", 40, 2, "1x3"), ("f16", 48, 3, "1x3"),
                                                     ("f16", 64, 2, "1x4"), ("bf16", 49, 3, "1x4"), ("bf16", 17, 1, "1x2")])
def test_launch_shapes_reach_every_pass(dt, tokens, height, passes, dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = ROWS * cus * (height - 1) + 3 if height > 1 else 3   # the busiest workgroup walks `height` row groups; a short last group
    L = layer(64, N * 8 - 4, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens)
    assert instance(desc, tokens).endswith(f"rgs={height} pass={passes}")
    x = _dense(64, tokens, dt, 7)[0]
    xt = _xt(x, dt, dev, tokens, 64)
    y16, y32 = _np(call(desc, xt, L.out_features)), _np(call(desc, xt, L.out_features, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, dt, what=instance(desc, tokens))


# ---------------------------------------------------------------------------------------------- 4. rows past `tokens`
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_token_rows_past_tokens_do_not_leak(dt, dev):
    L = layer(TILE + 8, 8 * ROWS + 4, dt, perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 17)
    x = _xt(_dense(L.in_features, 64, dt, 3)[0], dt, dev, 64, L.in_features)
    x[17:] *= 1000.0   # (what rows 17 .. 63 hold must not matter to rows 0 .. 16)
    for f32 in (False, True):
        y17, y64 = call(desc, x[:17].contiguous(), L.out_features, out_f32=f32), call(desc, x, L.out_features, out_f32=f32)
        assert torch.equal(_bits(y17), _bits(y64[:17]))


# ---------------------------------------------------------------------------------------------- 5. batch invariance
@pytest.mark.parametrize("dt,perm", [("f16", 1), ("bf16", 0)])
def test_a_token_has_the_same_bits_in_every_slot_of_every_batch(dt, perm, dev):
    L = layer(2 * TILE + 264, 8 * (ROWS + 1) - 4, dt, perm=perm, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 64)
    I, O = L.in_features, L.out_features
    others = _xt(_dense(I, 64, dt, 21)[0], dt, dev, 64, I)
    token = _xt(_dense(I, 1, dt, 22)[0], dt, dev, 1, I)[0]
    for f32 in (False, True):
        seen = []
        for slot in (0, 16, 33, 63):
            x = others.clone()
            x[slot] = token
            seen.append(_bits(call(desc, x, O, out_f32=f32)[slot]))
        x17 = others[:17].clone()
        x17[9] = token
        seen.append(_bits(call(desc, x17, O, out_f32=f32)[9]))
        assert all(torch.equal(seen[0], s) for s in seen[1:])


# ---------------------------------------------------------------------------------------------- 6. the route it replaces
@pytest.mark.parametrize("dt,perm", [("f16", 0), ("bf16", 1)])
def test_forty_tokens_give_the_bits_of_the_launches_of_sixteen(dt, perm, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 8 * (ROWS + 1) - 4, dt, perm=perm, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 40)
    assert B.lib().vptq_quant_gemv_kernel_name(desc, 40, EXACT) == b"gemm_k256_kernel"
    x = _dense(L.in_features, 40, dt, 11)[0]
    xt = _xt(x, dt, dev, 40, L.in_features)
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    for f32 in (False, True):
        new, old = call(desc, xt, L.out_features, out_f32=f32), gemv_abi(m, xt, EXACT, out_f32=f32)
        am.check_outputs(_np(new), mm, aa, dt, f32, what=f"gemm_k256w [fp32={f32}]")
        am.check_outputs(_np(old), mm, aa, dt, f32, what=f"gemm_k256 x 3 [fp32={f32}]")
        assert torch.equal(_bits(new), _bits(old))   # (the same order of sums: the same bits, not only within the bound)


# ---------------------------------------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("dt,tokens", [("f16", 45), ("bf16", 29)])
def test_two_launches_and_a_graph_replay_give_the_same_bits(dt, tokens, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 8 * (ROWS + 1), dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens)
    xt = _xt(_dense(L.in_features, tokens, dt, 5)[0], dt, dev, tokens, L.in_features)
    a, b = call(desc, xt, L.out_features), call(desc, xt, L.out_features)
    assert torch.equal(_bits(a), _bits(b))
    yg = torch.full((tokens, L.out_features), float("nan"), dtype=xt.dtype, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_k256w(desc, xt.data_ptr(), yg.data_ptr(), tokens, 0, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(_bits(a), _bits(yg))


# ---------------------------------------------------------------------------------------------- 8. the real reference
@pytest.mark.parametrize("name", ["h4096_f16_llm_t64", "h4096_bf16_llm_t64"])
def test_reference_goldens_of_64_tokens(name, dev):
    L, x, y, cfg, W_head = load_big(name)
    dt, T = cfg["dtype"], cfg["tokens"]
    assert T == 64
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, T)
    xt = _xt(x, dt, dev, T, L.in_features)
    out = stored_rows(tensor_to_bits(call(desc, xt, L.out_features)).reshape(1, T, -1), cfg)
    err = rel_err(out, y, dt)
    print(name, f"{err:.2e}")
    assert err <= TOL[dt], err


# ---------------------------------------------------------------------------------------------- 9. the module
LAUNCHES = ("vptq_quant_gemm_k256w", "vptq_quant_gemv", "vptq_dequant")


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


def _spied(m, xt, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    y = m(xt)
    monkeypatch.setattr(B, "lib", lambda: real)
    return y, calls


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_module_takes_the_entry_where_the_route_says_so(dt, dev, monkeypatch):
    import vptq_amd
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    L = layer(2048, 512, dt, bias=1)
    assert vptq_amd.arithmetic() == "reference"
    for tokens in (24, 64):
        x = _dense(2048, tokens, dt, 9 + tokens)[0]
        xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, 2048)
        mm, aa = am.model(am.pieces(L), x, arith="exact")
        # auto: what the route function says - the entry, or the launches of before (vptq_quant_gemv up to 48 tokens, dense from 49)
        m = spec_to_module(L, dev)
        expect_instance(m, L, tokens)
        routed = vq.gemm_k256w_route(512, 2048, tokens)
        y, calls = _spied(m, xt, monkeypatch)
        assert calls == (["vptq_quant_gemm_k256w"] if routed else ["vptq_quant_gemv"] if tokens <= 48 else ["vptq_dequant"]), calls
        # the knob on: the entry and nothing else
        monkeypatch.setattr(bd, "_GEMM_K256W_MODE", "1")
        y1, calls = _spied(m, xt, monkeypatch)
        assert calls == ["vptq_quant_gemm_k256w"], calls
        am.check_outputs(_np(y1).reshape(mm.shape), mm, aa, dt, False, what=f"VQuantLinear.forward, {tokens} tokens, routed")
        # ... but never in the folded arithmetic (a layer the load-time gate passes: its flags are not the reference's roundings)
        vptq_amd.set_arithmetic("folded")
        try:
            m2 = spec_to_module(L, dev)
            y2, calls = _spied(m2, xt, monkeypatch)
            assert not (m2._descriptor().arithmetic_flags & EXACT), "the layer must pass the folded form's gate for this test"
            assert "vptq_quant_gemm_k256w" not in calls and calls, calls
        finally:
            vptq_amd.set_arithmetic("reference")
        monkeypatch.setattr(bd, "_GEMM_K256W_MODE", "auto")
