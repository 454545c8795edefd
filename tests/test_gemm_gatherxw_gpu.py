"""vptq_quant_gemm_gatherxw (gemm_gatherxw_kernel in gemm_gatherxw.hip): 17 - 48 tokens of vptq_quant_gemm_gatherx's formats in one
launch, with and without a column permutation, on the GPU.  On the pattern of tests/test_gemm_gatherw_gpu.py, with its helpers and
those of tests/test_gemm_gatherx_gpu.py.

TILE = 1024 columns per tile and 16 outputs per row group are the kernel's; the shapes are the smallest that reach each edge.  Every
call writes into a buffer whose token rows are NaN and sit between sentinel guard rows, with a workspace of exactly the query's bytes.

  1. weights bit for bit: one-hot activations in all three token blocks pick columns of W, which must be vptq_dequant's bits
  2. sums against the per-output float64 model of the reference's roundings (tests/_arith_model.py, check_both, its bounds unchanged)
  3. the bit contract: 40 tokens in one launch give the BITS of the 16-token entry on tokens 0 - 15, 16 - 31, 32 - 39; a token keeps
     its bits in another slot of another batch size; token rows past `tokens` do not leak
  4. more row groups than resident workgroups (rgs=2)
  5. VQuantLinear.forward: the knob on / off / auto, a permuted layer, a compacted twin
Each row asserts its instance string first."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gatherw_gpu import COLS1 as COLS48, _bits, _xt
from test_gemm_gatherx_gpu import layer, call as call16, FMT, BITS, TILE
from test_gemm_gather_px_gpu import px_call
from test_gemm_gatherxw_cpu import want
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu

# one per (V, RES) plus an odd width and T = 32; with v8-k32768-0 the (V = 8, no residual) instantiations
FMT6 = ("v16-k65536-0", "v16-k65536-1024", "v16-k65536-32768", "v16-k65536-65536", "v8-k65536-4096", "v8-k65536-4")
FMT7 = FMT6 + ("v8-k32768-0",)


def instance(desc, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_gatherxw_instance(desc, tokens, 0, buf, len(buf)), "vptq_quant_gemm_gatherxw_instance")
    return buf.value.decode()


def expect_instance(m, L, tokens, fmt):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    desc, keep = module_desc(m)
    assert desc.index_bits + desc.res_bits == BITS[fmt] and desc.vector_len == FMT[fmt][0] and bool(desc.perm) == (L.perm is not None)
    assert B.lib().vptq_quant_gemm_gatherxw_supported(desc, tokens) == 1
    assert B.lib().vptq_quant_gemm_gatherx_supported(desc, tokens) == 0 and B.lib().vptq_quant_gemm_gather_px_supported(desc, tokens) == 0
    assert instance(desc, tokens) == want(desc, tokens, cus), (instance(desc, tokens), want(desc, tokens, cus))
    return desc, keep


def call(desc, xt, O, out_f32=False):
    """the entry with y's token rows NaN between guard rows and a workspace of EXACTLY the query's bytes (0xFF bytes; NULL without a
    permutation); -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = B.lib().vptq_quant_gemm_gatherxw_workspace_bytes(desc, tokens)
    assert need == ((tokens * xt.shape[-1] * 2 + 255) // 256 * 256 if desc.perm else 0)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=xt.device) if need else None
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    B.check(B.lib().vptq_quant_gemm_gatherxw(desc, xt.data_ptr(), y.data_ptr(), tokens, F32 if out_f32 else 0, ws.data_ptr() if need else None,
                                             need, B.current_stream_ptr(xt.device)), "vptq_quant_gemm_gatherxw")
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


# ---------------------------------------------------------------------------------------------- 1. weights bit for bit
G1 = TILE + 8


@pytest.mark.parametrize("fmt,dt,perm", list(itertools.product(FMT6, ("f16", "bf16"), (0, 1))))
def test_one_hot_activations_read_dequant_bits(fmt, dt, perm, dev):
    edges = (0, 7, 8, TILE - 1, TILE, TILE + 1, G1 - 1)
    assert len(set(COLS48)) == 48 and all(any(c in COLS48[16 * b:16 * b + 16] for c in edges) for b in range(3))
    O = 28 if FMT[fmt][0] == 16 else 20   # V = 16: two vector-rows, V = 8: three; the last partial
    L = layer(G1, O, fmt, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 48, fmt)
    W = m.dequant()
    x = torch.zeros(48, G1, dtype=W.dtype, device=dev)
    x[torch.arange(48), torch.tensor(COLS48)] = 1.0
    y = call(desc, x, O)
    want_w = W[:, torch.tensor(COLS48, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want_w).all()), f"{int((y != want_w).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 2. sums against the float64 model
GS = [8, TILE - 8, TILE, TILE + 8, 2 * TILE + 264]
TOKS = [17, 31, 32, 33, 47, 48]


def _sum_rows():
    rows = []
    for i, (dt, G, tokens) in enumerate(itertools.product(("f16", "bf16"), GS, TOKS)):
        # 2 x 5 x 6 rows: every (dtype, G, tokens); the format (period 7 against the tokens' 6) and the other axes cycle at strides of
        # their own, so that all 24 instantiations and both permutation states are met: test_the_sum_rows_cover_every_instantiation
        fmt = FMT7[i % 7]
        v = FMT[fmt][0]
        N = (1, 3)[(i // 2 + i // 9) % 2]
        cut = ((0, 4), (0, 4, 12))[v == 16]   # O = V N, V N - 4 (a ragged last row), V = 16: V N - 12 (the upper half-entry wholly masked)
        rows.append(pytest.param(dict(fmt=fmt, dt=dt, G=G, tokens=tokens, perm=(i + i // 2) % 2, bias=(i // 3 + i // 7) % 2,
                                      O=N * v - cut[(i // 4 + i // 11) % len(cut)], x=("dense", "planted")[(i + i // 5) % 2]),
                                 id=f"{fmt}-{dt}-G{G}-tok{tokens}-i{i}"))
    return rows


def test_the_sum_rows_cover_every_instantiation():
    def res(fmt):
        b = FMT[fmt][2] * FMT[fmt][0] * 2
        return 0 if not b else 1 if b <= 32768 else 2
    es = [p.values[0] for p in _sum_rows()]
    assert {(e["dt"], FMT[e["fmt"]][0], res(e["fmt"]), (e["tokens"] + 15) // 16) for e in es} == \
        set(itertools.product(("f16", "bf16"), (8, 16), (0, 1, 2), (2, 3)))
    assert {(e["perm"], (e["tokens"] + 15) // 16) for e in es} == set(itertools.product((0, 1), (2, 3)))


@pytest.mark.parametrize("e", _sum_rows())
def test_sums_vs_the_exact_model(e, dev):
    L = layer(e["G"], e["O"], e["fmt"], e["dt"], perm=e["perm"], bias=e["bias"])
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, e["tokens"], e["fmt"])
    kind, kw = (_dense, {}) if e["x"] == "dense" else (_planted, dict(perm=L.perm))
    x = kind(L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"], **kw)[0]
    xt = _xt(x, L.dtype, dev, e["tokens"], L.in_features)
    y16, y32 = _np(call(desc, xt, e["O"])), _np(call(desc, xt, e["O"], out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, e["tokens"]))


# ---------------------------------------------------------------------------------------------- 3. the bit contract
@pytest.mark.parametrize("fmt,dt,perm", [("v16-k65536-0", "bf16", 0), ("v16-k65536-1024", "f16", 1), ("v16-k65536-32768", "f16", 0),
                                         ("v16-k65536-65536", "bf16", 1), ("v8-k65536-4096", "f16", 1), ("v8-k65536-4", "bf16", 0),
                                         ("v8-k32768-0", "f16", 1)])
def test_a_token_has_the_bits_of_the_sixteen_token_entry_in_every_slot(fmt, dt, perm, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 3 * 16 - 4, fmt, dt, perm=perm, bias=1)   # three row groups
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 40, fmt)
    I, O = L.in_features, L.out_features
    x = np.ascontiguousarray(_dense(I, 48, dt, 11)[0]).reshape(48, I)
    xt = _xt(x, dt, dev, 48, I)
    mm, aa = am.model(am.pieces(L), x[:40], arith="exact")
    partner = px_call if perm else call16   # the 16-token entry of the layer: vptq_quant_gemm_gather_px / vptq_quant_gemm_gatherx
    assert B.lib().vptq_quant_gemm_gatherx_supported(desc, 16) == 1
    for f32 in (False, True):
        new = call(desc, xt[:40], O, out_f32=f32)
        am.check_outputs(_np(new), mm, aa, dt, f32, what=f"gemm_gatherxw [fp32={f32}]")
        old = torch.cat([partner(desc, xt[a:b], O, out_f32=f32) for a, b in ((0, 16), (16, 32), (32, 40))])
        assert torch.equal(_bits(new), _bits(old))   # (the same order of sums: the same bits, not only within the bound)
        # a token in another slot of another batch size
        want_bits = _bits(new[5])
        for tokens, slot in ((48, 0), (48, 16), (48, 33), (48, 47), (17, 16), (33, 32)):
            xs = xt[48 - tokens:].clone()
            xs[slot] = xt[5]
            assert torch.equal(_bits(call(desc, xs, O, out_f32=f32)[slot]), want_bits), (tokens, slot)
        # token rows past `tokens`, huge and infinite, do not change the rows before them
        xh = xt.clone()
        xh[33:] *= 1000.0
        xh[33:35] = float("inf")
        few = call(desc, xh[:33], O, out_f32=f32)   # (a view of the first rows: the launch reads next to the huge rows)
        assert not bool(torch.isnan(few).any()) and not bool(torch.isinf(few).any())
        assert torch.equal(_bits(few), _bits(call(desc, xh, O, out_f32=f32)[:33])) and torch.equal(_bits(few), _bits(new[:33]))


# ---------------------------------------------------------------------------------------------- 4. more row groups than workgroups
@pytest.mark.parametrize("fmt,dt,tokens,wgcu", [("v8-k32768-0", "f16", 20, 4), ("v16-k65536-1024", "bf16", 41, 2)])
def test_more_row_groups_than_resident_workgroups(fmt, dt, tokens, wgcu, dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    v = FMT[fmt][0]
    N = (16 // v) * wgcu * cus + 3               # more row groups than workgroups of the launch; spare rows
    L = layer(64, N * v - 4, fmt, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, fmt)
    assert instance(desc, tokens).endswith(f"tb={(tokens + 15) // 16} tiles=1 wgcu={wgcu} rgs=2")
    x = _dense(64, tokens, dt, 7)[0]
    xt = _xt(x, dt, dev, tokens, 64)
    y16, y32 = _np(call(desc, xt, L.out_features)), _np(call(desc, xt, L.out_features, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, dt, what=instance(desc, tokens))


# ---------------------------------------------------------------------------------------------- 5. the module
ENTRY = "vptq_quant_gemm_gatherxw"
LAUNCHES = (ENTRY, "vptq_quant_gemm_gatherx", "vptq_quant_gemm_gather_px", "vptq_quant_gemm_gather", "vptq_quant_gemv", "vptq_dequant")


def _spied(m, xt, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    y = m(xt)
    monkeypatch.setattr(B, "lib", lambda: real)
    return y, [c for c in calls if c in LAUNCHES]


@pytest.mark.parametrize("fmt,dt,perm", [("v16-k65536-1024", "f16", 0), ("v16-k65536-0", "bf16", 0), ("v8-k65536-4096", "bf16", 1),
                                         ("v16-k65536-0", "f16", 1)])
def test_module_takes_the_entry_where_the_route_says_so(fmt, dt, perm, dev, monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    v, k, kr = FMT[fmt]
    L = layer(2048, 512, fmt, dt, perm=perm, bias=1)
    tokens = 24
    x = _dense(2048, tokens, dt, 9)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, 2048)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, fmt)
    # auto: what the route function says - the entry, or the dense route of before
    routed = vq.gemm_gatherxw_route(v, k, kr, 512, 2048, tokens, bool(perm))
    y, calls = _spied(m, xt, monkeypatch)
    assert calls == ([ENTRY] if routed else ["vptq_dequant"]), calls
    # the knob on: the entry and nothing else, and the bits of the direct call
    monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", "1")
    y1, calls = _spied(m, xt, monkeypatch)
    assert calls == [ENTRY], calls
    assert torch.equal(_bits(y1.reshape(tokens, 512)), _bits(call(desc, xt.reshape(tokens, 2048), 512)))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_outputs(_np(y1).reshape(mm.shape), mm, aa, dt, False, what=f"VQuantLinear.forward, {tokens} tokens, routed")
    if fmt == "v16-k65536-0" and not perm:
        # a compacted copy (v16-k65536-0 has exact sliced layouts): the entry over the repacked stream, its twin's bits
        m2 = spec_to_module(L, dev)
        m2.compact(force=True)
        assert m2.is_compact()
        y2, calls = _spied(m2, xt, monkeypatch)
        assert ENTRY in calls and "vptq_dequant" not in calls, calls
        assert torch.equal(_bits(y1), _bits(y2))
    # the knob off: never (a fresh module: `m` holds the first spy's vptq_dequant in its dense-route cache)
    monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", "0")
    y0, calls = _spied(spec_to_module(L, dev), xt, monkeypatch)
    assert calls == ["vptq_dequant"], calls
    monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", "auto")
