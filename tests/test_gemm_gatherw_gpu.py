"""vptq_quant_gemm_gatherw (gemm_gatherw_kernel in gemm_gatherw.hip): 17 - 48 tokens of the large-codebook formats v8-k65536-0 / -256 /
-65536 in one launch, on the GPU.

TILE = 1024 columns per tile and R = 2 vector-rows (16 outputs) per row group are the kernel's; the shapes are the smallest that reach
each edge.  Every call writes into a buffer whose token rows are NaN and sit between sentinel guard rows: an output the launch does
not write stays NaN, a store outside the rows breaks a guard.

  1. weights bit for bit: one-hot activations in all three token blocks pick columns of W, which must be vptq_dequant's bits
  2. sums: dense and spiky activations against the per-output float64 model of the reference's roundings (tests/_arith_model.py,
     check_both, its bounds unchanged), 16-bit and VPTQ_GEMV_OUT_F32 outputs
  3. more row groups than workgroups (rgs=2), one TB = 2 row and one TB = 3 row
  4. token rows past `tokens` do not leak into the rows before them
  5. the bit contract: 40 tokens in one launch give the BITS of vptq_quant_gemm_gather on tokens 0 - 15, 16 - 31, 32 - 39; a token
     keeps its bits in another slot of another batch size
  6. two launches and a graph replay give identical bits
  7. the real reference's outputs.  tests/golden/k65536_r256_t24.npz ("t24": 24 index bits) holds ONE token, and no committed
     fixture of these formats holds 17: the fixtures' tokens are repeated to fill 20 - 36 rows, every row held to the reference's
     output of its token
  8. VQuantLinear.forward takes the entry where gemm_gatherw_route says so; a compacted copy gives its twin's bits; a layer with a
     column permutation is never routed unless the knob is on
Each row asserts its instance string first."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import layer, call as call16, KR, TILE, R, GUARD, SENTINEL, F32
import _arith_model as am
from _cases import load_golden, load_fmt, stored_rows, rel_err
from _gpu_util import spec_to_module, bits_to_tensor, tensor_to_bits, module_desc

pytestmark = pytest.mark.gpu

TOL = {"f16": 1e-3, "bf16": 8e-3}   # (tests/test_hip_parity.py: the parity bound against the real reference)
T_OF = {kr: T for T, kr in KR.items()}


def instance(desc, tokens, flags=0):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_gatherw_instance(desc, tokens, flags, buf, len(buf)), "vptq_quant_gemm_gatherw_instance")
    return buf.value.decode()


def expect_instance(m, L, tokens, T):
    from vptq_amd import _backend as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = (L.num_indices + R - 1) // R
    grid = min(groups, 4 * cus)
    want = (f"gemm_gatherw dt={L.dtype} t={T} perm={int(L.perm is not None)} tok={tokens} tb={(tokens + 15) // 16} "
            f"tiles={(L.in_features + TILE - 1) // TILE} rgs={(groups + grid - 1) // grid}")
    desc, keep = module_desc(m)
    assert B.lib().vptq_quant_gemm_gatherw_supported(desc, tokens) == 1
    assert B.lib().vptq_quant_gemm_gather_supported(desc, tokens) == 0   # (the 16-token entry still refuses them)
    assert instance(desc, tokens) == want
    return desc, keep


def call(desc, xt, O, out_f32=False, flags=0):
    """the entry with y's token rows NaN between guard rows; -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    B.check(B.lib().vptq_quant_gemm_gatherw(desc, xt.data_ptr(), y.data_ptr(), tokens, flags | (F32 if out_f32 else 0),
                                            B.current_stream_ptr(xt.device)), "vptq_quant_gemm_gatherw")
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


def _bits(y):
    return y.view(torch.int32 if y.dtype == torch.float32 else torch.int16)


def _xt(x, dt, dev, tokens, I):
    return bits_to_tensor(x, dt, dev).reshape(tokens, I)


# ---------------------------------------------------------------------------------------------- 1. weights bit for bit
G1, O1 = TILE + 8, 8 * R + 4
_EDGE = [0, 1, 7, 8, 63, 64, 511, 512, TILE - 1, TILE, TILE + 1, G1 - 1]
# 48 columns: the edges first, the rest spread over the row; dealt round-robin so that every token block holds four of the edges
_REST = [c for c in range(15, G1, 23) if c not in _EDGE][:48 - len(_EDGE)]
COLS1 = [(_EDGE + _REST)[(i % 16) * 3 + i // 16] for i in range(48)]


@pytest.mark.parametrize("T,dt,perm", list(itertools.product((16, 24, 32), ("f16", "bf16"), (0, 1))))
def test_one_hot_activations_read_dequant_bits(T, dt, perm, dev):
    assert len(set(COLS1)) == 48 and all(sum(c in COLS1[16 * b:16 * b + 16] for c in _EDGE) == 4 for b in range(3))
    L = layer(G1, O1, T, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 48, T)
    W = m.dequant()
    x = torch.zeros(48, G1, dtype=W.dtype, device=dev)
    x[torch.arange(48), torch.tensor(COLS1)] = 1.0
    y = call(desc, x, O1)
    want = W[:, torch.tensor(COLS1, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want).all()), f"{int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 2. sums against the float64 model
GS = [8, TILE - 8, TILE, TILE + 8, 2 * TILE + 264]
TOKS = [17, 31, 32, 33, 47, 48]


def _sum_rows():
    rows = []
    for i, (dt, G, tokens) in enumerate(itertools.product(("f16", "bf16"), GS, TOKS)):
        # 2 x 5 x 6 rows: every (dtype, G, tokens); T, perm and the other axes cycle at strides of their own, so that all 24
        # instantiations (dtype, T, perm, token blocks) are met: test_the_sum_rows_cover_every_instantiation
        T = (16, 24, 32)[(i + i // 3) % 3]
        N = (1, R + 1)[(i // 2 + i // 9) % 2]
        rows.append(pytest.param(dict(T=T, dt=dt, G=G, tokens=tokens, perm=(i + i // 2) % 2, bias=(i // 3 + i // 7) % 2, N=N,
                                      O=N * 8 - 4 * ((i // 4 + i // 11) % 2), x=("dense", "planted")[(i + i // 5) % 2]),
                                 id=f"t{T}-{dt}-G{G}-tok{tokens}-i{i}"))
    return rows


def test_the_sum_rows_cover_every_instantiation():
    seen = {(e.values[0]["dt"], e.values[0]["T"], e.values[0]["perm"], (e.values[0]["tokens"] + 15) // 16) for e in _sum_rows()}
    assert seen == set(itertools.product(("f16", "bf16"), (16, 24, 32), (0, 1), (2, 3)))


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
    xt = _xt(x, L.dtype, dev, e["tokens"], L.in_features)
    y16, y32 = _np(call(desc, xt, e["O"])), _np(call(desc, xt, e["O"], out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, L.dtype, what=instance(desc, e["tokens"]))


# ---------------------------------------------------------------------------------------------- 3. more row groups than workgroups
@pytest.mark.parametrize("T,dt,tokens", [(24, "f16", 20), (32, "bf16", 41)])
def test_more_row_groups_than_resident_workgroups(T, dt, tokens, dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = R * 4 * cus + 3                     # more row groups than workgroups of the launch; a spare row
    L = layer(64, N * 8 - 4, T, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, T)
    assert instance(desc, tokens).endswith("rgs=2")
    x = _dense(64, tokens, dt, 7)[0]
    xt = _xt(x, dt, dev, tokens, 64)
    y16, y32 = _np(call(desc, xt, L.out_features)), _np(call(desc, xt, L.out_features, out_f32=True))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(y16, y32, mm, aa, dt, what=instance(desc, tokens))


# ---------------------------------------------------------------------------------------------- 4. rows past `tokens`
@pytest.mark.parametrize("T,dt,tokens", [(16, "bf16", 17), (24, "f16", 33), (32, "f16", 17), (32, "bf16", 33)])
def test_token_rows_past_tokens_do_not_leak(T, dt, tokens, dev):
    L = layer(TILE + 8, 8 * R + 4, T, dt, perm=1, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, T)
    x = _xt(_dense(L.in_features, 48, dt, 3)[0], dt, dev, 48, L.in_features)
    x[tokens:] *= 1000.0   # (what the rows from `tokens` on hold must not matter to the rows before them)
    x[tokens:tokens + 2] = float("inf")
    for f32 in (False, True):
        # (a view of the first rows: the launch of `tokens` tokens reads next to the huge rows)
        few, all48 = call(desc, x[:tokens], L.out_features, out_f32=f32), call(desc, x, L.out_features, out_f32=f32)
        assert not bool(torch.isnan(few).any()) and not bool(torch.isinf(few).any())
        assert torch.equal(_bits(few), _bits(all48[:tokens]))


# ---------------------------------------------------------------------------------------------- 5. the bit contract
@pytest.mark.parametrize("T,dt,perm", list(itertools.product((16, 24, 32), ("f16", "bf16"), (0, 1))))
def test_a_token_has_the_bits_of_the_sixteen_token_kernel_in_every_slot(T, dt, perm, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 8 * (R + 1) - 4, T, dt, perm=perm, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, 40, T)
    I, O = L.in_features, L.out_features
    x = np.ascontiguousarray(_dense(I, 48, dt, 11)[0]).reshape(48, I)
    xt = _xt(x, dt, dev, 48, I)
    mm, aa = am.model(am.pieces(L), x[:40], arith="exact")
    for f32 in (False, True):
        new = call(desc, xt[:40], O, out_f32=f32)
        am.check_outputs(_np(new), mm, aa, dt, f32, what=f"gemm_gatherw [fp32={f32}]")
        assert B.lib().vptq_quant_gemm_gather_supported(desc, 16) == 1
        old = torch.cat([call16(desc, xt[a:b], O, out_f32=f32) for a, b in ((0, 16), (16, 32), (32, 40))])
        assert torch.equal(_bits(new), _bits(old))   # (the same order of sums: the same bits, not only within the bound)
        # a token in another slot of another batch size
        token = xt[5]
        want = _bits(new[5])
        for tokens, slot in ((48, 0), (48, 16), (48, 33), (48, 47), (17, 16), (17, 9), (33, 32)):
            xs = xt[48 - tokens:].clone()
            xs[slot] = token
            assert torch.equal(_bits(call(desc, xs, O, out_f32=f32)[slot]), want), (tokens, slot)


# ---------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("T,dt,tokens", [(16, "f16", 45), (24, "bf16", 29), (32, "f16", 33)])
def test_two_launches_and_a_graph_replay_give_the_same_bits(T, dt, tokens, dev):
    from vptq_amd import _backend as B
    L = layer(2 * TILE + 264, 8 * (R + 1), T, dt, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, T)
    xt = _xt(_dense(L.in_features, tokens, dt, 5)[0], dt, dev, tokens, L.in_features)
    a, b = call(desc, xt, L.out_features), call(desc, xt, L.out_features)
    assert torch.equal(_bits(a), _bits(b))
    yg = torch.full((tokens, L.out_features), float("nan"), dtype=xt.dtype, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.check(B.lib().vptq_quant_gemm_gatherw(desc, xt.data_ptr(), yg.data_ptr(), tokens, 0, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(_bits(a), _bits(yg))


# ---------------------------------------------------------------------------------------------- 7. the real reference
@pytest.mark.parametrize("name,load,rows", [("k65536_r256_t24", load_golden, 24), ("t8_k65536_r256", load_fmt, 24),
                                            ("t5_k65536_r65536_perm", load_fmt, 20), ("t4_k65536_r0_8192x2048_perm", load_fmt, 36)])
def test_reference_goldens(name, load, rows, dev):
    L, x, y, cfg, W_head = load(name)
    dt = cfg["dtype"]
    x = np.ascontiguousarray(x).reshape(-1, L.in_features)
    y = np.ascontiguousarray(y).reshape(x.shape[0], -1)
    assert y.shape[1] == L.out_features, "the fixture stores every output of every token"
    pick = np.arange(rows) % x.shape[0]   # the fixture's tokens, repeated to fill the launch
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, rows, T_OF[L.num_res_centroids])
    out = tensor_to_bits(call(desc, _xt(x[pick], dt, dev, rows, L.in_features), L.out_features))
    err = rel_err(out, y[pick], dt)
    print(name, f"{err:.2e}")
    assert err <= TOL[dt], err


# ---------------------------------------------------------------------------------------------- 8. the module
LAUNCHES = ("vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather", "vptq_quant_gemv", "vptq_dequant")


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


@pytest.mark.parametrize("T,dt", [(24, "f16"), (16, "bf16"), (32, "f16")])
def test_module_takes_the_entry_where_the_route_says_so(T, dt, dev, monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    L = layer(2048, 512, T, dt, bias=1)
    tokens = 24
    x = _dense(2048, tokens, dt, 9)[0]
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, 2048)
    m = spec_to_module(L, dev)
    desc, keep = expect_instance(m, L, tokens, T)
    # auto: what the route function says - the entry, or the dense route of before
    routed = vq.gemm_gatherw_route(8, 65536, KR[T], 512, 2048, tokens)
    y, calls = _spied(m, xt, monkeypatch)
    assert calls == (["vptq_quant_gemm_gatherw"] if routed else ["vptq_dequant"]), calls
    # the knob on: the entry and nothing else, and the bits of the direct call
    monkeypatch.setattr(bd, "_GEMM_GATHERW_MODE", "1")
    y1, calls = _spied(m, xt, monkeypatch)
    assert calls == ["vptq_quant_gemm_gatherw"], calls
    direct = call(desc, xt.reshape(tokens, 2048), 512)
    assert torch.equal(_bits(y1.reshape(tokens, 512)), _bits(direct))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_outputs(_np(y1).reshape(mm.shape), mm, aa, dt, False, what=f"VQuantLinear.forward, {tokens} tokens, routed")
    # a compacted copy: the entry over the repacked stream, its twin's bits
    m2 = spec_to_module(L, dev)
    m2.compact(force=True)
    assert m2.is_compact()
    y2, calls = _spied(m2, xt, monkeypatch)
    assert "vptq_quant_gemm_gatherw" in calls and "vptq_dequant" not in calls, calls
    assert torch.equal(_bits(y1), _bits(y2))
    # the knob off: never (a fresh module: `m` holds the first spy's vptq_dequant in its dense-route cache)
    monkeypatch.setattr(bd, "_GEMM_GATHERW_MODE", "0")
    y0, calls = _spied(spec_to_module(L, dev), xt, monkeypatch)
    assert "vptq_quant_gemm_gatherw" not in calls and calls == ["vptq_dequant"], calls
    monkeypatch.setattr(bd, "_GEMM_GATHERW_MODE", "auto")


def test_module_never_routes_a_permuted_layer_unless_the_knob_is_on(dev, monkeypatch):
    """the permuted forms were measured at 1.8 - 6.8 times the dense route (profiles/r23): with cells that route every size, a layer
    without a permutation takes the entry and its permuted twin keeps the dense route; the knob reaches both"""
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    monkeypatch.setattr(bd, "GEMM_GATHERW_MIN_ELEMENTS", 0)
    monkeypatch.setattr(bd, "_GEMM_GATHERW_CELLS", ((256, 0, 17, 48),))
    tokens = 24
    xt = bits_to_tensor(_dense(2048, tokens, "f16", 9)[0], "f16", dev).reshape(1, tokens, 2048)
    plain, permuted = (spec_to_module(layer(2048, 512, 24, "f16", perm=p, bias=1), dev) for p in (0, 1))
    assert vq.gemm_gatherw_route(8, 65536, 256, 512, 2048, tokens)
    assert _spied(plain, xt, monkeypatch)[1] == ["vptq_quant_gemm_gatherw"]
    y0, calls = _spied(permuted, xt, monkeypatch)
    assert calls == ["vptq_dequant"], calls
    monkeypatch.setattr(bd, "_GEMM_GATHERW_MODE", "1")
    y1, calls = _spied(permuted, xt, monkeypatch)
    assert calls == ["vptq_quant_gemm_gatherw"], calls
    assert rel_err(tensor_to_bits(y1), tensor_to_bits(y0), "f16") <= TOL["f16"]
