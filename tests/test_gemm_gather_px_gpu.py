"""vptq_quant_gemm_gather_px (gemm_gather_px.hip): batched decode of layers WITH a column permutation - x[perm] written once into a
workspace (permute_x_tokens_kernel), then the layer's own kernel in its form without a permutation - on the GPU.

The contract is BITS: the permuted forms of gemm_gather / gemm_gatherx / gemm_gatherw read x[t][perm[c]] two bytes at a time, the
plain forms read xp[t][c] = x[t][perm[c]] sixteen bytes at a time; the products and the order of the sums are the same.  The
comparison is the existing entry (the parent's code) on the same descriptor.

TILE = 1024 columns per tile and R = 2 vector-rows (16 outputs) per row group are the kernels'; a permute workgroup spans 64 chunks
of 8 columns = 512 columns and a thread 4 tokens.  Columns 8, 64, TILE + 8 and 2 TILE + 264 (2312 = 4.5 workgroup spans), outputs
8 R + 4 = 8 (R + 1) - 4 = 20 and 4, token counts on both sides of every slice of 4 and block of 16.

  1. bits and sums: px == the layer's own entry on the same descriptor == the own entry on the descriptor stripped of its permutation
     over torch's x[:, perm]; 16-bit and fp32 outputs; every row also against the float64 model (tests/_arith_model.py)
  2. weights: one-hot activations read vptq_dequant's bits
  3. placement: every operand in an arena of its own (tests/_arena.py), the workspace exactly the query's bytes at 16-byte alignment
  4. the workspace's contents do not matter; calls share it; a layer without a permutation needs none
  5. graph capture of the entry (linear: two kernel nodes), replayed on new activations; the module under a capture with too small a
     workspace
  6. VQuantLinear.forward: the route, its knob, a compacted twin, an unpermuted twin; prepare_model sizes the stream's workspace"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_route_models_gpu import _dense, _planted, _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import layer as layer_g, call as call16, KR, TILE, R, GUARD, SENTINEL, F32
from test_gemm_gatherw_gpu import call as call_w, COLS1 as COLS48, _bits
from test_gemm_gatherx_gpu import layer as layer_x, call as call_x, FMT
import _arena as ar
import _arith_model as am
from _cases import rel_err
from _gpu_util import spec_to_module, bits_to_tensor, tensor_to_bits, module_desc

pytestmark = pytest.mark.gpu

PX_THREADS, PX_TOK = 64, 4
GS = (8, 64, TILE + 8, 2 * TILE + 264)
OS = (8 * R + 4, 8 * (R + 1) - 4, 4)
XFMTS = ("v16-k65536-1024", "v8-k32768-0")
PERMS = ("random", "identity", "reversal")
TOL = {"f16": 1e-3, "bf16": 8e-3}   # (tests/test_hip_parity.py: the parity bound against the real reference)


def make_layer(kind, G, O, dt, perm="random", bias=0):
    """kind: 16 / 24 / 32 (gemm_gather's and gemm_gatherw's formats by index width) or a gemm_gatherx format name; perm: None or
    one of PERMS"""
    L = layer_g(G, O, kind, dt, perm=perm is not None, bias=bias) if isinstance(kind, int) else layer_x(G, O, kind, dt, perm=perm is not None, bias=bias)
    if perm == "identity":
        L.perm = np.arange(G, dtype=np.uint16)
    elif perm == "reversal":
        L.perm = np.arange(G, dtype=np.uint16)[::-1].copy()
    return L


def own_call(kind, tokens):
    """the existing entry that serves (kind, tokens): the comparison"""
    return call_w if tokens > 16 else call16 if isinstance(kind, int) else call_x


def instance(desc, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(256)
    B.check(B.lib().vptq_quant_gemm_gather_px_instance(desc, tokens, 0, buf, len(buf)), "vptq_quant_gemm_gather_px_instance")
    return buf.value.decode()


def expect_instance(desc, L, kind, tokens):
    from vptq_amd import _backend as B
    assert B.lib().vptq_quant_gemm_gather_px_supported(desc, tokens) == 1
    G = L.in_features
    need = (tokens * G * 2 + 255) // 256 * 256 if L.perm is not None else 0
    assert B.lib().vptq_quant_gemm_gather_px_workspace_bytes(desc, tokens) == need
    text = instance(desc, tokens)
    head, inner = text.split(" | ")
    want = "none" if L.perm is None else f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK}"
    assert head == want, text
    name = "gemm_gatherw" if tokens > 16 else "gemm_gather" if isinstance(kind, int) else "gemm_gatherx"
    assert inner.startswith(name + " dt=") and " perm=0 " in inner and f" tok={tokens} " in inner, text
    return need


def px_call(desc, xt, O, out_f32=False, ws=None, flags=0):
    """the entry with y's token rows NaN between guard rows and a workspace of EXACTLY the query's bytes (0xFF bytes unless one is
    handed in; ws=False: NULL); -> y [tokens, O] after the guards were checked"""
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = B.lib().vptq_quant_gemm_gather_px_workspace_bytes(desc, tokens)
    if ws is None and need:
        ws = torch.full((need,), 255, dtype=torch.uint8, device=xt.device)
    buf = torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device)
    buf[GUARD:GUARD + tokens] = float("nan")
    y = buf[GUARD:GUARD + tokens]
    B.check(B.lib().vptq_quant_gemm_gather_px(desc, xt.data_ptr(), y.data_ptr(), tokens, flags | (F32 if out_f32 else 0),
                                              None if ws is None or ws is False else ws.data_ptr(), 0 if ws is None or ws is False else ws.numel(),
                                              B.current_stream_ptr(xt.device)), "vptq_quant_gemm_gather_px")
    torch.cuda.current_stream(xt.device).synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return y.clone()


def stripped(desc):
    """the descriptor without its permutation: scale / bias in the quantised matrix's column order, as the inner launch sees it"""
    from vptq_amd import _backend as B
    p = B.LayerDesc.from_buffer_copy(desc)
    p.weight_scale, p.weight_bias = desc.scale_permuted, desc.bias_permuted
    p.perm, p.inv_perm, p.scale_permuted, p.bias_permuted = None, None, None, None
    return p


def _xbits(L, tokens, kind, seed):
    if kind == "dense":
        return _dense(L.in_features, tokens, L.dtype, seed)[0]
    return _planted(L.in_features, tokens, L.dtype, seed, perm=L.perm)[0]


def _xt(x, dt, dev, tokens, I):
    return bits_to_tensor(x, dt, dev).reshape(tokens, I)


# ---------------------------------------------------------------------------------------------- 1. bits and sums
# (kind, tokens): gemm_gather 1 / 5 / 16, gemm_gatherw 17 / 32 / 33 / 48, two gemm_gatherx formats 5 / 16
KERNEL_ROWS = [(T, t) for T, t in zip((16, 24, 32), (1, 5, 16))] + [(T, t) for T, t in zip((24, 32, 16, 24), (17, 32, 33, 48))] + \
    [(f, t) for f in XFMTS for t in (5, 16)]


def _bit_rows():
    rows = []
    for i, (G, (kind, tokens)) in enumerate(itertools.product(GS, KERNEL_ROWS)):
        # 4 x 11 rows: every (G, kernel, token count); the other axes advance with the row r and, at strides of their own, with G
        gi, r = divmod(i, len(KERNEL_ROWS))
        if isinstance(kind, int):
            kind = (16, 24, 32)[((16, 24, 32).index(kind) + gi) % 3]
        rows.append(pytest.param(dict(kind=kind, dt=("f16", "bf16")[(r + gi) % 2], G=G, tokens=tokens, O=OS[(r + 2 * gi) % 3], perm=PERMS[(r + gi) % 3],
                                      bias=(r + gi // 2) % 2, x=("dense", "planted")[(r // 2 + gi) % 2]), id=f"{kind}-G{G}-tok{tokens}-i{i}"))
    return rows


def test_the_bit_rows_cover_every_kernel_dtype_and_permutation():
    rows = [e.values[0] for e in _bit_rows()]
    fam = lambda e: "w" if e["tokens"] > 16 else "g" if isinstance(e["kind"], int) else "x"
    assert {(fam(e), e["dt"]) for e in rows} == set(itertools.product("gwx", ("f16", "bf16")))
    assert {(fam(e), e["perm"]) for e in rows} == set(itertools.product("gwx", PERMS))
    assert {(e["G"], e["tokens"]) for e in rows} >= set(itertools.product(GS, (1, 5, 16, 17, 32, 33, 48)))
    assert {e["O"] for e in rows} == set(OS) and {e["kind"] for e in rows} == {16, 24, 32, *XFMTS}


@pytest.mark.parametrize("e", _bit_rows())
def test_bits_equal_the_layers_own_entry_and_sums_hold_the_model(e, dev):
    L = make_layer(e["kind"], e["G"], e["O"], e["dt"], perm=e["perm"], bias=e["bias"])
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    tokens, O, G = e["tokens"], e["O"], e["G"]
    expect_instance(desc, L, e["kind"], tokens)
    x = _xbits(L, tokens, e["x"], G + tokens)
    xt = _xt(x, L.dtype, dev, tokens, G)
    own = own_call(e["kind"], tokens)
    plain = stripped(desc)
    xp = xt[:, torch.from_numpy(L.perm.astype(np.int64)).to(dev)].contiguous()   # torch's x[:, perm]
    out = {}
    for f32 in (False, True):
        y = px_call(desc, xt, O, out_f32=f32)
        assert not bool(torch.isnan(y).any())
        want = own(desc, xt, O, out_f32=f32)                        # the parent's code on the same descriptor
        assert torch.equal(_bits(y), _bits(want)), f"{int((_bits(y) != _bits(want)).sum())} of {y.numel()} outputs differ from the layer's own entry"
        assert torch.equal(_bits(y), _bits(own(plain, xp, O, out_f32=f32)))   # ... and on the stripped descriptor over x[:, perm]
        out[f32] = _np(y)
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_both(out[False], out[True], mm, aa, L.dtype, what=instance(desc, tokens))


# ---------------------------------------------------------------------------------------------- 2. weights bit for bit
G1, O1 = TILE + 8, 8 * R + 4
COLS16 = [0, 1, 7, 8, 63, 64, 300, 511, 512, TILE - 2, TILE - 1, TILE, TILE + 1, G1 - 3, G1 - 2, G1 - 1]


@pytest.mark.parametrize("kind,dt,tokens,perm", [(24, "f16", 48, "random"), (16, "bf16", 33, "reversal"), (32, "bf16", 16, "random"),
                                                 ("v16-k65536-1024", "f16", 16, "random"), ("v8-k32768-0", "bf16", 16, "identity")])
def test_one_hot_activations_read_dequant_bits(kind, dt, tokens, perm, dev):
    L = make_layer(kind, G1, O1, dt, perm=perm)
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    expect_instance(desc, L, kind, tokens)
    W = m.dequant()
    cols = (COLS48 if tokens > 16 else COLS16)[:tokens]
    assert len(set(cols)) == tokens
    x = torch.zeros(tokens, G1, dtype=W.dtype, device=dev)
    x[torch.arange(tokens), torch.tensor(cols)] = 1.0           # input feature j: it reaches stored column c with perm[c] == j
    y = px_call(desc, x, O1)
    want = W[:, torch.tensor(cols, device=dev)].t()
    assert not bool(torch.isnan(y).any())
    assert bool((y == want).all()), f"{int((y != want).sum())} of {y.numel()} weights differ from vptq_dequant's"   # (-0 == +0)


# ---------------------------------------------------------------------------------------------- 3. placement
# the least alignment the entry accepts (include/vptq_hip.h, "Alignment:"): indices and codebooks 16 bytes, scale / bias / perm 4,
# the output bias 2; x 16; y element-aligned; the workspace 16
HOSTILE_OFFSETS = {"indices": 16, "centroids": 16, "res_centroids": 16, "weight_scale": 4, "weight_bias": 4, "perm": 4, "bias": 2}


def _placed_call(L, xt, tokens, O, fill, offsets, x_off, y_off, f32, dev):
    from vptq_amd import _backend as B
    m = spec_to_module(L, dev)
    arenas = ar.place_module(m, fill, {k: v for k, v in offsets.items() if k in ar._module_params(m)})
    desc, keep = module_desc(m)
    xv, xa = ar.place(xt, fill, x_off)
    y, ya = ar.guarded_out((tokens, O), torch.float32 if f32 else xt.dtype, dev, y_off)
    need = B.lib().vptq_quant_gemm_gather_px_workspace_bytes(desc, tokens)
    assert need == (tokens * L.in_features * 2 + 255) // 256 * 256
    ws, wa = ar.guarded_workspace(need, False, dev, align=16)
    assert ws.numel() == need and ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 != 0
    B.check(B.lib().vptq_quant_gemm_gather_px(desc, xv.data_ptr(), y.data_ptr(), tokens, F32 if f32 else 0, ws.data_ptr(), need,
                                              B.current_stream_ptr(dev)), "vptq_quant_gemm_gather_px")
    torch.cuda.synchronize(dev)
    for name, a in list(arenas.items()) + [("x", xa)]:
        assert a.intact(), (name, a.damage())                    # the inputs' margins
    assert ya.intact(), ("y", ya.damage())                       # a store outside y
    assert wa.intact(), ("workspace", wa.damage())               # a store outside the query's bytes
    assert not bool(torch.isnan(y).any())
    return y.clone()


@pytest.mark.parametrize("kind,dt,G,tokens", [(24, "f16", TILE + 8, 5), (32, "bf16", 2 * TILE + 264, 33), (16, "f16", 64, 48),
                                              ("v16-k65536-1024", "bf16", 2 * TILE + 264, 16)])
def test_same_bits_under_every_placement(kind, dt, G, tokens, dev):
    O = 8 * R + 4
    L = make_layer(kind, G, O, dt, perm="random", bias=1)
    xt = _xt(_xbits(L, tokens, "dense", 3), dt, dev, tokens, G)
    for f32 in (False, True):
        benign = _placed_call(L, xt, tokens, O, ar.BENIGN, {}, 0, 0, f32, dev)
        hostile = _placed_call(L, xt, tokens, O, ar.HOSTILE, HOSTILE_OFFSETS, 16, 4 if f32 else 2, f32, dev)
        assert torch.equal(_bits(benign), _bits(hostile))
        m = spec_to_module(L, dev)
        desc, keep = module_desc(m)
        assert torch.equal(_bits(benign), _bits(own_call(kind, tokens)(desc, xt, O, out_f32=f32)))   # torch's allocator: the own entry's bits


# ---------------------------------------------------------------------------------------------- 4. the workspace's contents
@pytest.mark.parametrize("kind,dt", [(24, "f16"), (32, "bf16")])
def test_workspace_contents_do_not_matter_and_calls_share_it(kind, dt, dev):
    from vptq_amd import _backend as B
    G, O = 2 * TILE + 264, 8 * (R + 1) - 4
    L = make_layer(kind, G, O, dt, perm="random", bias=1)
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    x48 = _xt(_xbits(L, 48, "dense", 5), dt, dev, 48, G)
    x5 = _xt(_xbits(L, 5, "dense", 6), dt, dev, 5, G)
    fresh48, fresh5 = px_call(desc, x48, O), px_call(desc, x5, O)
    need = B.lib().vptq_quant_gemm_gather_px_workspace_bytes(desc, 48)
    # NaN patterns of both dtypes, 0xFF bytes, zeros
    for pattern in (0x7E00, 0x7FC0, 0xFFFF, 0):
        ws = torch.full((need // 2,), pattern - (1 << 16) if pattern >= 1 << 15 else pattern, dtype=torch.int16, device=dev).view(torch.uint8)
        assert torch.equal(_bits(px_call(desc, x48, O, ws=ws)), _bits(fresh48)), hex(pattern)
    # 48 tokens, then 5 through the SAME (larger) workspace: the rows the first call left behind do not reach the second
    ws = torch.full((need,), 255, dtype=torch.uint8, device=dev)
    assert torch.equal(_bits(px_call(desc, x48, O, ws=ws)), _bits(fresh48))
    assert torch.equal(_bits(px_call(desc, x5, O, ws=ws)), _bits(fresh5))
    assert torch.equal(_bits(px_call(desc, x48, O, ws=ws)), _bits(fresh48))
    # the workspace holds x[:, perm] of the last call in its first rows (what the inner kernel read)
    xp = x48[:, torch.from_numpy(L.perm.astype(np.int64)).to(dev)]
    assert torch.equal(ws[:48 * G * 2].view(torch.int16).reshape(48, G), xp.contiguous().view(torch.int16))


@pytest.mark.parametrize("kind,dt,tokens", [(24, "f16", 5), (16, "bf16", 33), ("v16-k65536-1024", "f16", 16)])
def test_a_layer_without_a_permutation_needs_no_workspace(kind, dt, tokens, dev):
    G, O = TILE + 8, 8 * R + 4
    L = make_layer(kind, G, O, dt, perm=None, bias=1)
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    assert expect_instance(desc, L, kind, tokens) == 0
    xt = _xt(_xbits(L, tokens, "dense", 4), dt, dev, tokens, G)
    for f32 in (False, True):
        assert torch.equal(_bits(px_call(desc, xt, O, out_f32=f32, ws=False)), _bits(own_call(kind, tokens)(desc, xt, O, out_f32=f32)))


# ---------------------------------------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("kind,dt,tokens", [(24, "f16", 12), (32, "bf16", 40), ("v8-k32768-0", "f16", 9)])
def test_a_captured_call_replays_on_new_activations(kind, dt, tokens, dev):
    from vptq_amd import _backend as B
    G, O = 2 * TILE + 264, 8 * (R + 1) - 4
    L = make_layer(kind, G, O, dt, perm="random", bias=1)
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    xs = [_xt(_xbits(L, tokens, "dense", s), dt, dev, tokens, G) for s in (1, 2, 3)]
    eager = [px_call(desc, x, O) for x in xs]
    need = B.lib().vptq_quant_gemm_gather_px_workspace_bytes(desc, tokens)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=dev)   # (sized before the capture: nothing is allocated inside it)
    xg = xs[0].clone()
    yg = torch.full((tokens, O), float("nan"), dtype=xg.dtype, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            # (one stream, two launches in stream order: a linear graph)
            B.check(B.lib().vptq_quant_gemm_gather_px(desc, xg.data_ptr(), yg.data_ptr(), tokens, 0, ws.data_ptr(), need, B.current_stream_ptr(dev)), "capture")
    torch.cuda.current_stream(dev).wait_stream(s)
    for x, want in zip(xs, eager):
        xg.copy_(x)
        yg.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(_bits(yg), _bits(want))


PX_LAUNCHES = ("vptq_quant_gemm_gather_px", "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx", "vptq_quant_gemv", "vptq_dequant")


class _Spy:
    """B.lib() with the names of the launching entries called through it recorded"""
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in PX_LAUNCHES:
            return fn

        def spy(*a):
            self._calls.append(name)
            return fn(*a)
        return spy


def _spied(m, xt, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    try:
        y = m(xt)
    finally:
        monkeypatch.setattr(B, "lib", lambda: real)
    return y, calls


def _route_everything(monkeypatch):
    """cells that hand every layer of the three kernels to px (the committed cells lie over 4 M index elements: test layers are small)"""
    from vptq_amd import batched_decode as bd
    monkeypatch.setattr(bd, "GEMM_GATHERW_MIN_ELEMENTS", 0)
    cells = tuple((8, 65536, kr, 0, 5, 48) for kr in (0, 256, 65536)) + tuple(FMT[f] + (0, 5, 16) for f in XFMTS)
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_CELLS", cells)
    return bd


def _stream_without_a_workspace(dev):
    """a side stream whose `B.gemv_workspace` does not exist (torch hands out pooled stream handles: a buffer an earlier test left
    under this handle is retired, as the backend retires an outgrown one)"""
    from vptq_amd import _backend as B
    s = torch.cuda.Stream(dev)
    old = B._GEMV_WS.pop((dev.index if dev.index is not None else torch.cuda.current_device(), s.cuda_stream), None)
    if old is not None:
        B._GEMV_WS_RETIRED.append(old)
    return s


def test_module_under_a_capture_with_too_small_a_workspace_takes_the_dense_route(dev, monkeypatch):
    from vptq_amd import _backend as B
    bd = _route_everything(monkeypatch)
    tokens, I, O = 24, 2048, 512
    L = make_layer(24, I, O, "f16", perm="random", bias=1)
    m = spec_to_module(L, dev)
    xt = _xt(_xbits(L, tokens, "dense", 9), "f16", dev, tokens, I).reshape(1, tokens, I)
    # ONE spy for the whole test: the dense route keeps the library functions it first saw (`_desc_dense`)
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    y_px = m(xt)                                                   # eager, on the current stream: px
    assert calls == ["vptq_quant_gemm_gather_px"], calls
    s = _stream_without_a_workspace(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", "0")
    del calls[:]
    with torch.cuda.stream(s):
        y_dense = m(xt)                                            # the dense route warmed up on s, no px call: no workspace grows
    assert calls == ["vptq_dequant"], calls
    assert (m._descriptor().device_index, s.cuda_stream) not in B._GEMV_WS
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", "auto")
    del calls[:]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        s.synchronize()
        with torch.cuda.graph(g, stream=s):
            y_cap = m(xt)                                          # raises nothing
    torch.cuda.current_stream(dev).wait_stream(s)
    assert calls == ["vptq_dequant"], calls                        # px was asked, had no workspace, and stepped aside
    assert (m._descriptor().device_index, s.cuda_stream) not in B._GEMV_WS   # nothing was allocated during the capture
    g.replay()
    torch.cuda.synchronize(dev)
    assert not bool(torch.isnan(y_cap).any())
    assert rel_err(tensor_to_bits(y_cap), tensor_to_bits(y_dense), "f16") <= TOL["f16"]
    assert rel_err(tensor_to_bits(y_cap), tensor_to_bits(y_px), "f16") <= TOL["f16"]


# ---------------------------------------------------------------------------------------------- 6. the module
@pytest.mark.parametrize("kind,dt,tokens", [(24, "f16", 24), (16, "bf16", 12), (32, "f16", 48), ("v16-k65536-1024", "bf16", 5)])
def test_module_takes_px_where_its_route_says_so(kind, dt, tokens, dev, monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    I, O = 2048, 512
    L = make_layer(kind, I, O, dt, perm="random", bias=1)
    x = _xbits(L, tokens, "dense", 9)
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, I)
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    # the committed cells never contain a layer this small: today's routes, no px
    v, k, kr = (8, 65536, KR[kind]) if isinstance(kind, int) else FMT[kind]
    assert not vq.gemm_gather_px_route(v, k, kr, O, I, tokens)
    y_today, today = _spied(m, xt, monkeypatch)
    assert "vptq_quant_gemm_gather_px" not in today and len(today) >= 1, today
    # cells that route everything: px and nothing else, the bits of the direct call (and so of the layer's own entry)
    _route_everything(monkeypatch)
    assert vq.gemm_gather_px_route(v, k, kr, O, I, tokens)
    m1 = spec_to_module(L, dev)
    y1, calls = _spied(m1, xt, monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_px"], calls
    direct = px_call(desc, xt.reshape(tokens, I), O)
    assert torch.equal(_bits(y1.reshape(tokens, O)), _bits(direct))
    assert torch.equal(_bits(direct), _bits(own_call(kind, tokens)(desc, xt.reshape(tokens, I), O)))
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    am.check_outputs(_np(y1).reshape(mm.shape), mm, aa, dt, False, what=f"VQuantLinear.forward, {tokens} tokens, px")
    # the functional op routes the same way
    from vptq_amd import ops, _backend as B
    real, seen = B.lib(), []
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, seen))
    try:
        yo = ops.quant_gemm(xt, **_op_keywords(m1))
    finally:
        monkeypatch.setattr(B, "lib", lambda: real)
    assert seen == ["vptq_quant_gemm_gather_px"], seen
    assert torch.equal(_bits(yo), _bits(y1))
    # a compacted twin: px over the repacked stream, its twin's bits
    m2 = spec_to_module(L, dev)
    m2.compact(force=True)
    assert m2.is_compact()
    y2, calls = _spied(m2, xt, monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_px"], calls
    assert torch.equal(_bits(y1), _bits(y2))
    # the knob off: the calls of today (a fresh module: routes cache what they built)
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", "0")
    y0, calls = _spied(spec_to_module(L, dev), xt, monkeypatch)
    assert calls == today, (calls, today)
    assert torch.equal(_bits(y0), _bits(y_today))
    # the knob on, the committed cells: px again
    monkeypatch.undo()
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", "1")
    y3, calls = _spied(spec_to_module(L, dev), xt, monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_px"], calls
    assert torch.equal(_bits(y3), _bits(y1))


def _op_keywords(m):
    return dict(bias=m.bias, indices=m.packed_indices(), centroids=m.centroids.weight, outlier_indices=m.outlier_indices,
                outlier_centroids=m.outlier_centroids.weight if m.enable_outlier else None, residual_indices=None,
                residual_centroids=m.res_centroids.weight if m.enable_residual else None, perm=m.perm if m.enable_perm else None,
                weight_scale=m.weight_scale, weight_bias=m.weight_bias, vector_len=m.vector_len, outlier_vector_len=m.outlier_vector_len,
                num_codebooks=m.num_codebooks, num_centroids=m.num_centroids, num_outlier_centroids=m.num_outlier_centroids,
                num_res_centroids=m.num_res_centroids, is_indice_packed=True, group_size=m.group_size, outlier_size=m.outlier_size,
                in_features=m.in_features, out_features=m.out_features, padding=m.padding, outlier_padding=m.outlier_padding)


@pytest.mark.parametrize("kind,dt,tokens", [(24, "f16", 24), (24, "f16", 12), ("v16-k65536-1024", "bf16", 5)])
def test_an_unpermuted_twin_never_calls_px(kind, dt, tokens, dev, monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    I, O = 2048, 512
    plain = make_layer(kind, I, O, dt, perm=None, bias=1)
    xt = _xt(_xbits(plain, tokens, "dense", 9), dt, dev, tokens, I).reshape(1, tokens, I)
    y_today, today = _spied(spec_to_module(plain, dev), xt, monkeypatch)
    for mode in ("auto", "1"):
        _route_everything(monkeypatch)
        monkeypatch.setattr(bd, "_GEMM_GATHER_PX_MODE", mode)
        y, calls = _spied(spec_to_module(plain, dev), xt, monkeypatch)
        assert calls == today and "vptq_quant_gemm_gather_px" not in calls, (mode, calls, today)
        assert torch.equal(_bits(y), _bits(y_today))
        monkeypatch.undo()


def test_prepare_model_sizes_the_streams_workspace_for_a_later_capture(dev, monkeypatch):
    import vptq_amd
    from vptq_amd import _backend as B
    _route_everything(monkeypatch)
    tokens, I, O = 48, 2 * TILE + 264, 8 * (R + 1) - 4
    Ls = [make_layer(24, I, O, "f16", perm="random", bias=1), make_layer(32, 64, O, "f16", perm="random"), make_layer(16, I, O, "f16", perm=None)]
    model = torch.nn.Sequential(*[spec_to_module(L, dev) for L in Ls])
    need = (48 * I * 2 + 255) // 256 * 256
    assert [m._gemm_gather_px_workspace_bytes() for m in model] == [need, (48 * 64 * 2 + 255) // 256 * 256, 0]
    s = _stream_without_a_workspace(dev)
    key = (model[0]._descriptor().device_index, s.cuda_stream)
    assert key not in B._GEMV_WS
    vptq_amd.prepare_model(model, s)
    assert key in B._GEMV_WS and B._GEMV_WS[key].numel() >= need
    xt = _xt(_xbits(Ls[0], tokens, "dense", 2), "f16", dev, tokens, I).reshape(1, tokens, I)
    eager, calls = _spied(model[0], xt, monkeypatch)
    assert calls == ["vptq_quant_gemm_gather_px"]
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            y, calls = _spied(model[0], xt, monkeypatch)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert calls == ["vptq_quant_gemm_gather_px"], calls          # the captured step keeps the px route
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(_bits(y), _bits(eager))
    # a buffer that must outgrow the 2 MiB default: the query of a 28672-column layer at 48 tokens (no layer of that size is built here)
    d = B.LayerDesc.from_buffer_copy(model[0]._descriptor().desc)
    d.in_features = d.group_size = 28672
    d.row_words = 28672 * 24 // 32
    assert B.lib().vptq_quant_gemm_gather_px_workspace_bytes(d, 48) == 2752512 > 2 << 20
