"""Every GEMV route against a float64 model of its OWN arithmetic, output by output (tests/_arith_model.py): the reference's
roundings (exact), the folded form, the selective form, column ranges.  A table of routes; each entry asserts the kernel it
reaches, then checks the 16-bit output and the VPTQ_GEMV_OUT_F32 output (where the route has one) of a dense and / or a
planted activation - 2 - 4 columns at >= 50 x the rms of the others, in distinct blocks of 128 columns, the others within
3 x rms: every hot-block rule agrees on the hot set.  The last tests hold the table's kernel list and the sliced entry
points' handling of VPTQ_GEMV_SELECTIVE and of sums beyond the accumulator word's range."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, gemv_abi, kernel_name, module_desc

pytestmark = pytest.mark.gpu

EXACT, MFMA, VALU, F32 = 1 << 2, 1 << 3, 1 << 4, 1 << 5
GENERIC, BATCHED, SEL = 1 << 1, 1 << 7, 1 << 9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vptq_amd import _backend as B
    B.lib()
    return torch.device("cuda", 0)


def _dense(I, tokens, dt, seed):
    x = np.random.default_rng(seed).standard_normal((1, tokens, I))
    return vo.from_f32(x.astype(np.float32), dt), ()


def _planted(I, tokens, dt, seed, n=3, perm=None, clip=2.5):
    """-> (x bits, hot blocks): the others within `clip` = 2.5 (~2.5 x their rms), n columns of magnitude 60 in distinct 128-column blocks
    (the same columns for every token).  Where the last 512-column window is short of columns, one of them is planted too: the
    per-window rule (gemv_k256m.hip) counts the missing columns as zeros, so a short window's threshold is low and its own ordinary
    columns could turn hot - with a planted column in it every rule has the same hot set (_hot_rules_agree).
    perm (the layer's uint16 permutation): blocks and windows are those of the STORED column order - stored column c reads input
    feature perm[c] - so the column planted for stored position c is x[..., perm[c]]"""
    rng = np.random.default_rng(seed)
    x = np.clip(rng.standard_normal((1, tokens, I)), -clip, clip)
    nb = (I + 127) // 128
    blocks = set(int(b) for b in rng.choice(nb, min(n, nb), replace=False))
    if I % SEL_WINDOW and I % SEL_WINDOW < SEL_WINDOW // 2 and not any(b * 128 >= I - I % SEL_WINDOW for b in blocks):
        blocks.add(nb - 1)
    blocks = sorted(blocks)
    feature = np.arange(I) if perm is None else np.ascontiguousarray(perm).view(np.uint16).astype(np.int64)
    for b in blocks:
        col = b * 128 + int(rng.integers(0, min(128, I - b * 128)))
        x[..., feature[col]] = 60.0 * rng.choice([-1.0, 1.0], size=tokens)
    return vo.from_f32(x.astype(np.float32), dt), tuple(blocks)


XKIND = {"dense": _dense, "planted": _planted}
SEL_WINDOW, SEL_KAPPA = 512, 6.0   # the hot-block rules: kappa x rms of f16(s x) over the layer / over each 512-column window


SEL_STAGE = 8192   # gemv_k256m stages 8192 columns per phase: beyond that a wave's rms runs over its 512 columns of BOTH phases


def _hot_rules_agree(P, x, hot, perm=None):
    """the hot blocks by every documented rule - over the layer's columns (gemv_hot, the chain launch), over each 512-column
    window, missing columns counted as zeros (gemv_k256m up to 8192 columns) and, beyond 8192 columns, over the 1024 columns of
    window w and window w + 16 together (gemv_k256m from 5 sweeps on: two staging phases, one threshold per wave) - are the
    planted ones, every column clear of every threshold by 25 %.  Columns, blocks and windows are those of the STORED order
    (perm: stored column c = input feature perm[c])"""
    dt = P["dtype"]
    I = P["W"].shape[1]
    sx = np.abs(vo.round_to((P["s"] * vo.to_f32(np.asarray(x), dt).reshape(-1, I)).astype(np.float32), dt).astype(np.float64))
    if perm is not None:
        sx = sx[:, np.ascontiguousarray(perm).view(np.uint16).astype(np.int64)]
    pad = np.concatenate([sx, np.zeros((sx.shape[0], (-I) % SEL_WINDOW))], axis=1)
    sq = (pad.reshape(sx.shape[0], -1, SEL_WINDOW) ** 2).mean(axis=2)
    win = np.sqrt(sq)
    thresholds = {"layer": SEL_KAPPA * np.sqrt((sx ** 2).mean(axis=1, keepdims=True)),
                  "window": SEL_KAPPA * np.repeat(win, SEL_WINDOW, axis=1)[:, :I]}
    if SEL_STAGE < I <= 2 * SEL_STAGE:   # (wider layers are not staged: no selective form in gemv_k256m)
        per = SEL_STAGE // SEL_WINDOW
        both = np.concatenate([sq, np.zeros((sq.shape[0], 2 * per - sq.shape[1]))], axis=1)
        pair = np.sqrt((both[:, :per] + both[:, per:]) / 2)
        thresholds["window pair"] = SEL_KAPPA * np.repeat(np.concatenate([pair, pair], axis=1), SEL_WINDOW, axis=1)[:, :I]
    for rule, thr in thresholds.items():
        ratio = sx / thr
        assert not ((ratio > 0.8) & (ratio < 1.25)).any(), f"{rule} rule: a column near the threshold"
        got = sorted({int(j) // 128 for j in np.nonzero((ratio >= 1).any(axis=0))[0]})
        assert got == sorted(hot), f"{rule} rule: hot blocks {got}, planted {sorted(hot)}"


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _check(y16, y32, L, x, e, hot, extra=0.0, P=None, what=""):
    """y16 / y32 (either None) against the entry's model; a failure names the models the output WOULD meet"""
    P = P or am.pieces(L)
    T = x.size // L.in_features
    kw = dict(rounded=e.get("rounded", False), round_sx=e.get("round_sx", True),
              hot_cols=am.hot_mask_for(L.in_features, hot, L.perm) if e["arith"] == "selective" else None)
    if e["arith"] == "selective":
        _hot_rules_agree(P, x, hot, L.perm)
    mm, aa = am.model(P, x, e["arith"], **kw)
    try:
        if y16 is not None:
            am.check_outputs(y16.reshape(T, -1), mm, aa, L.dtype, False, extra, what=what + " [16-bit]")
        if y32 is not None:
            am.check_outputs(y32.reshape(T, -1), mm, aa, L.dtype, True, extra, what=what + " [fp32]")
    except AssertionError as err:
        meets = []
        for name, arith, kw2 in (("exact", "exact", {}), ("folded", "folded", {}), ("folded r16(c+r)", "folded", dict(rounded=True)),
                                 ("folded unrounded s x", "folded", dict(round_sx=False)),
                                 ("folded r16(c+r), unrounded s x", "folded", dict(rounded=True, round_sx=False)),
                                 ("selective", "selective", dict(hot_cols=am.hot_mask_for(L.in_features, hot, L.perm)))):
            m2, a2 = am.model(P, x, arith, **kw2)
            y = y32 if y32 is not None else y16
            if not am.violations(y.reshape(T, -1), m2, a2, L.dtype, y is y32, extra)[0].any():
                meets.append(name)
        raise AssertionError(f"{err}  (the output meets: {meets or 'no model'})") from None


# ---------------------------------------------------------------------------------------------- the table of one-layer routes
# layer: (I, O, make_layer kwargs); flags of the call; the kernel name vptq_quant_gemv_kernel_name must give; the model; for the
# canonical format's kernels the instance vptq_quant_gemv_instance must give (every instantiation of those kernels has its row in
# tests/test_route_models_k256_gpu.py, which tests/test_instance_census_cpu.py holds to what the dispatch can produce).
# Tail shapes: O not a multiple of v x row group (264, 1032, 72, 40, 8200), I not a multiple of the sweep / block (4104, 1000,
# 520, 8192 + 512).
def E(route, layer, dt, tokens, flags, arith, xkinds=("dense",), **kw):
    e = dict(route=route, layer=layer, dt=dt, tokens=tokens, flags=flags, arith=arith, xkinds=xkinds, **kw)
    return pytest.param(e, id=f"{route}-{dt}-{layer[0]}x{layer[1]}-t{tokens}-f{flags}")


# gemv_k256_kernel<fast> (gemv_k256.hip): w = f16(c + r) by one packed add, times s x in fp32 (not rounded), + sum b x - the folded
# form of vptq_hip.h, "(c + r) * (scale_g * x_g)"; the matrix-pipe kernels stage f16(s x) and keep c + r exact (separate products)
VALU_FOLDED = dict(rounded=True, round_sx=False)


LLM = dict(dist="llm")
ONE_LAYER = [
    # VALU kernel of the canonical format: the reference's roundings; the folded form (fp16, 1 - 2 tokens)
    E("gemv_k256_kernel", (4104, 264, dict(LLM, bias=True)), "f16", 1, EXACT, "exact", ("dense", "planted"),
      instance="gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=0 fast=0 entry=1"),
    E("gemv_k256_kernel", (4104, 264, dict(LLM)), "bf16", 3, EXACT, "exact",
      instance="gemv_k256 dt=bf16 rows=1 tok=4 sw=1 perm=0 fast=0 entry=0"),
    E("gemv_k256_kernel", (1024, 72, dict(LLM, bias=True)), "f16", 4, EXACT | VALU, "exact",
      instance="gemv_k256 dt=f16 rows=1 tok=4 sw=1 perm=0 fast=0 entry=0"),
    E("gemv_k256_kernel<fast>", (4104, 264, dict(LLM, bias=True)), "f16", 1, 0, "folded", ("planted",), **VALU_FOLDED,
      instance="gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=0 fast=1 entry=1"),
    E("gemv_k256_kernel<fast>", (2048, 1032, dict(LLM)), "f16", 2, VALU, "folded", ("planted",), **VALU_FOLDED,
      instance="gemv_k256 dt=f16 rows=1 tok=2 sw=1 perm=0 fast=1 entry=0"),
    # persistent MFMA kernel: exact / folded / selective, 1 - 4 tokens, fp16 and bf16
    E("gemv_k256m_kernel", (2048, 4608, dict(LLM)), "f16", 1, EXACT | MFMA, "exact", ("dense", "planted"),
      instance="gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel", (2048, 1032, dict(LLM, bias=True)), "f16", 4, EXACT | MFMA, "exact",
      instance="gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel", (8192 + 512, 40, dict(LLM)), "bf16", 1, EXACT | MFMA, "exact",
      instance="gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel", (2048, 1032, dict(LLM, bias=True)), "bf16", 3, EXACT | MFMA, "exact",
      instance="gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel<fast>", (4104, 264, dict(LLM, bias=True)), "f16", 1, MFMA, "folded", ("planted",),
      instance="gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel<fast>", (2048, 1032, dict(LLM)), "f16", 2, MFMA, "folded", ("planted",),
      instance="gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel<fast>", (4104, 264, dict(LLM)), "bf16", 1, MFMA, "folded", ("planted",),
      instance="gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel<fast>", (2048, 1032, dict(LLM, bias=True)), "bf16", 4, MFMA, "folded", ("planted",),
      instance="gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    E("gemv_k256m_kernel<selective>", (4104, 264, dict(LLM, bias=True)), "f16", 1, SEL | MFMA, "selective", ("planted",),
      instance="gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    E("gemv_k256m_kernel<selective>", (2048, 4608, dict(LLM)), "f16", 1, SEL, "selective", ("planted",),
      instance="gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    E("gemv_k256m_kernel<selective>", (4104, 264, dict(LLM)), "bf16", 1, SEL | MFMA, "selective", ("planted",),
      instance="gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    E("gemv_k256m_kernel<selective>", (2048, 1032, dict(LLM)), "f16", 1, SEL | MFMA, "selective", ("planted",),
      instance="gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    # the one-pass batched-decode kernel (folded form), 1 - 16 tokens
    E("gemm_k256t_kernel", (4104, 264, dict(LLM, bias=True)), "f16", 1, BATCHED, "folded", ("planted",),
      instance="gemm_k256t dt=f16 perm=0 tok=1 sweeps=3 rgs=1"),
    E("gemm_k256t_kernel", (2048, 1032, dict(LLM)), "f16", 7, 0, "folded", ("planted",),
      instance="gemm_k256t dt=f16 perm=0 tok=7 sweeps=1 rgs=1"),
    E("gemm_k256t_kernel", (1000 + 24, 200, dict(LLM, bias=True)), "bf16", 16, 0, "folded", ("planted",),
      instance="gemm_k256t dt=bf16 perm=0 tok=16 sweeps=1 rgs=1"),
    # the batched-decode kernel in the reference's roundings, 5 - 16 tokens
    E("gemm_k256_kernel", (4104, 264, dict(LLM, bias=True)), "f16", 5, EXACT, "exact",
      instance="gemm_k256 dt=f16 perm=0 tok=5 passes=1"),
    E("gemm_k256_kernel", (2048, 1032, dict(LLM)), "f16", 16, EXACT, "exact",
      instance="gemm_k256 dt=f16 perm=0 tok=16 passes=1"),
    E("gemm_k256_kernel", (4104, 264, dict(LLM, bias=True)), "bf16", 9, EXACT, "exact",
      instance="gemm_k256 dt=bf16 perm=0 tok=9 passes=1"),
    # LDS-resident codebooks (256 < k <= 8192): the reference's roundings; the matrix-pipe one-token kernel (folded)
    E("gemv_lds_kernel", (520, 136, dict(num_centroids=4096, num_res_centroids=512, enable_perm=True)), "f16", 3, 0, "exact"),
    E("gemv_lds_kernel", (4096 + 8, 264, dict(num_centroids=8192, num_res_centroids=512)), "f16", 1, 0, "exact"),
    E("gemv_lds_mfma_kernel", (1000, 8200, dict(num_centroids=8192, num_res_centroids=0, bias=True)), "f16", 1, 0, "folded",
      ("planted",)),
    E("gemv_lds_mfma_kernel", (1024, 8192, dict(LLM, num_centroids=8192, num_res_centroids=256)), "bf16", 1, 0, "folded", ("planted",)),
    # cache gathers (k = 65536), L2 gathers of any format, the generic kernel
    E("gemv_gather_kernel", (2048, 1032, dict(num_centroids=65536, num_res_centroids=0, bias=True)), "f16", 1, 0, "exact"),
    E("gemv_gather_kernel", (4104, 264, dict(LLM, num_centroids=65536, num_res_centroids=256)), "bf16", 3, 0, "exact"),
    E("gemv_gatherx_kernel", (1024, 264, dict(LLM, vector_len=8, num_centroids=32768, num_res_centroids=512, bias=True)), "f16", 7, 0,
      "exact"),
    E("gemv_gatherx_kernel", (1032, 96, dict(LLM, vector_len=6, num_centroids=4096, num_res_centroids=4096, num_codebooks=2)), "bf16",
      6, 0, "exact"),
    E("gemv_generic_kernel", (4104, 264, dict(LLM, bias=True)), "f16", 2, GENERIC, "exact"),
    E("gemv_generic_kernel", (512 + 64, 128, dict(vector_len=8, num_centroids=4096, num_res_centroids=4096, outlier_size=64,
                                                    outlier_vector_len=4, num_outlier_centroids=256, enable_perm=True)), "bf16", 3,
      GENERIC, "exact"),
]


def _layer(e, seed=0):
    I, O, kw = e["layer"]
    kw = dict(kw)
    dist = kw.pop("dist", "ref-test")
    return vo.make_layer(I, O, dist=dist, seed=I + O + seed, dtype=e["dt"], **kw)


@pytest.mark.parametrize("e", ONE_LAYER)
def test_one_layer_route_vs_its_model(e, dev):
    L = _layer(e)
    m = spec_to_module(L, dev)
    assert kernel_name(m, e["tokens"], e["flags"]) == e["route"]
    if "instance" in e:   # (the canonical format's kernels: which instantiation, tests/test_route_models_k256_gpu.py)
        from test_route_models_k256_gpu import instance_of
        assert instance_of([module_desc(m)[0]], e["tokens"], e["flags"]) == e["instance"]
    P = am.pieces(L)
    for kind in e["xkinds"]:
        x, hot = XKIND[kind](L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"])
        xt = bits_to_tensor(x, L.dtype, dev).reshape(x.shape)
        y16 = _np(gemv_abi(m, xt, e["flags"]))
        y32 = _np(gemv_abi(m, xt, e["flags"], out_f32=True))
        _check(y16, y32, L, x, e, hot, P=P, what=f"{e['route']} {kind}")


# ---------------------------------------------------------------------------------------------- grouped launches
GROUPS = [
    # (layers, dtype, tokens, flags, route, arith): equal layers in one launch; unequal ones (the launch split by cost)
    ([(2048, 1032, dict(LLM)), (2048, 264, dict(LLM, bias=True))], "f16", 1, EXACT, "gemv_k256_kernel", "exact"),
    ([(4104, 264, dict(LLM))] * 4, "f16", 1, EXACT | MFMA, "gemv_k256m_kernel", "exact"),
    ([(2048, 4608, dict(LLM)), (2048, 72, dict(LLM, bias=True)), (2048, 1032, dict(LLM))], "bf16", 2, EXACT | MFMA, "gemv_k256m_kernel",
     "exact"),
    ([(4104, 264, dict(LLM, bias=True)), (4104, 1032, dict(LLM))], "f16", 1, SEL | MFMA, "gemv_k256m_kernel<selective>", "selective"),
]


@pytest.mark.parametrize("g", GROUPS, ids=[f"{g[4]}-{g[1]}-n{len(g[0])}" for g in GROUPS])
def test_grouped_launch_vs_its_model(g, dev):
    from vptq_amd import _backend as B
    shapes, dt, tokens, flags, route, arith = g
    Ls = [_layer(dict(layer=s, dt=dt), seed=i) for i, s in enumerate(shapes)]
    ms = [spec_to_module(L, dev) for L in Ls]
    keep = [module_desc(m) for m in ms]
    descs = (B.LayerDesc * len(ms))(*[k[0] for k in keep])
    name = B.lib().vptq_quant_gemv_grouped_kernel_name(descs, len(ms), tokens, flags)
    assert name is not None and name.decode() == route
    I = Ls[0].in_features
    x, hot = (_planted if arith != "exact" else _dense)(I, tokens, dt, 5 + tokens)
    xt = bits_to_tensor(x, dt, dev).reshape(x.shape)
    outs = {}
    for f32 in (False, True):
        ys = [torch.empty(1, tokens, L.out_features, dtype=torch.float32 if f32 else xt.dtype, device=dev) for L in Ls]
        xp = (C.c_void_p * len(ms))(*([xt.data_ptr()] * len(ms)))
        yp = (C.c_void_p * len(ms))(*[y.data_ptr() for y in ys])
        B.check(B.lib().vptq_quant_gemv_grouped(descs, len(ms), xp, yp, tokens, flags | (F32 if f32 else 0), B.current_stream_ptr(dev)),
                "vptq_quant_gemv_grouped")
        torch.cuda.synchronize()
        outs[f32] = [_np(y) for y in ys]
    for i, L in enumerate(Ls):
        _check(outs[False][i], outs[True][i], L, x, dict(arith=arith), hot, what=f"grouped {route} layer {i}")


# ---------------------------------------------------------------------------------------------- the persistent chain launch
# (more than 8 layers: the persistent launch; none that the load-time gate would hand to the reference's roundings - fewer than 32
# vector-rows)
CHAIN_SHAPES = [(1024, 512, dict(LLM)), (4104, 264, dict(LLM, bias=True)), (8192 + 512, 264, dict(LLM)), (512, 1000, dict(LLM, bias=True)),
                (2048, 2048 * 3, dict(LLM)), (6144, 520, dict(LLM)), (256, 1032, dict(LLM)), (4096, 264, dict(LLM)), (1024, 1032, dict(LLM)),
                (2048, 2048, dict(LLM, bias=True))]


CHAIN_INDEPENDENT = ["exact", "folded", "selective"]
CHAIN_DEPENDENT = ["folded"]   # (dependent lists take the persistent launch in the folded form)


@pytest.mark.parametrize("arith", CHAIN_INDEPENDENT)
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_independent_chain_vs_its_model(arith, dt, dev):
    import vptq_amd
    from vptq_amd.ops.chain import GemvChain
    before = vptq_amd.arithmetic()
    vptq_amd.set_arithmetic({"exact": "reference"}.get(arith, arith))
    try:
        Ls = [_layer(dict(layer=s, dt=dt), seed=i) for i, s in enumerate(CHAIN_SHAPES)]
        ms = [spec_to_module(L, dev) for L in Ls]
        xs = [(_planted if arith != "exact" else _dense)(L.in_features, 1, dt, 40 + i) for i, L in enumerate(Ls)]
        xt = [bits_to_tensor(x, dt, dev).reshape(x.shape) for x, _ in xs]
        chain = GemvChain(ms)
        flags = MFMA | (EXACT if arith == "exact" else SEL if arith == "selective" else 0)
        assert chain.kernel_name(1, flags) == "gemv_k256c_kernel"
        y16 = [_np(y) for y in chain(xt, flags=flags)]
        y32 = [_np(y) for y in chain(xt, flags=flags | F32)]
        torch.cuda.synchronize()
    finally:
        vptq_amd.set_arithmetic(before)
    for i, L in enumerate(Ls):
        try:
            _check(y16[i], y32[i], L, xs[i][0], dict(arith=arith), xs[i][1], what=f"chain {arith} layer {i}")
        except AssertionError:
            if arith != "selective":
                raise
            # (vptq_hip.h: a layer the selective chain launch does not implement takes VPTQ_GEMV_EXACT - then every output meets
            # the exact model)
            _check(y16[i], y32[i], L, xs[i][0], dict(arith="exact"), (), what=f"chain selective layer {i}, exact fallback")


@pytest.mark.parametrize("arith", CHAIN_DEPENDENT)
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_dependent_chain_vs_its_model(arith, dt, dev):
    """layer i + 1 reads layer i's 16-bit output: each layer is checked on the input it actually read (dependent lists take the
    persistent launch in the folded form)"""
    import vptq_amd
    from vptq_amd.ops.chain import GemvChain
    from _gpu_util import tensor_to_bits
    before = vptq_amd.arithmetic()
    vptq_amd.set_arithmetic("reference" if arith == "exact" else "folded")
    try:
        dims = [1024, 2048, 1032, 4096, 512, 1024, 2048, 1024, 264, 1024]
        Ls = [vo.make_layer(dims[i], dims[i + 1], dist="llm", seed=70 + i, dtype=dt, bias=i % 3 == 0) for i in range(len(dims) - 1)]
        ms = [spec_to_module(L, dev) for L in Ls]
        x0, _ = _dense(dims[0], 1, dt, 3)
        chain = GemvChain(ms, dependent=True)
        flags = MFMA | (EXACT if arith == "exact" else 0)
        assert chain.kernel_name(1, flags) == "gemv_k256c_kernel"
        ys = chain([bits_to_tensor(x0, dt, dev).reshape(x0.shape)], flags=flags)
        torch.cuda.synchronize()
        ybits = [tensor_to_bits(y) for y in ys]
    finally:
        vptq_amd.set_arithmetic(before)
    xin = x0
    for i, L in enumerate(Ls):
        _check(vo.to_f32(ybits[i], dt), None, L, xin, dict(arith=arith), (), what=f"dependent chain {arith} layer {i}")
        xin = ybits[i]


# ---------------------------------------------------------------------------------------------- fused dequant + GEMM
FUSED = [
    (1024, 1000, "f16", 77, "exact", dict(bias=True)),          # ragged tiles: the tile holds the reference's bits
    (4104, 264, "f16", 20, "exact", dict(LLM)),                  # K not a multiple of the 64-column step
    (2048, 520, "bf16", 40, "folded", dict(LLM, bias=True)),     # bf16: bf16(c + r) x bf16(s x) + sum b x
]


@pytest.mark.parametrize("I,O,dt,tokens,arith,kw", FUSED)
def test_fused_gemm_vs_its_model(I, O, dt, tokens, arith, kw, dev):
    """vptq_quant_gemm (no fp32 output: the call has one output type)"""
    from vptq_amd import _backend as B
    from vptq_amd import ops
    L = _layer(dict(layer=(I, O, kw), dt=dt), seed=tokens)
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m)
    assert B.lib().vptq_quant_gemm_supported(desc) == 1
    x, hot = (_dense if arith == "exact" else _planted)(I, tokens, dt, tokens)
    y = _np(ops.quant_gemm_fused(bits_to_tensor(x, dt, dev).reshape(x.shape), desc, O))
    _check(y, None, L, x, dict(arith=arith, rounded=arith == "folded"), hot, what=f"vptq_quant_gemm {dt}")


# ---------------------------------------------------------------------------------------------- sliced layouts
def _sliced(L, dev, **kw):
    from vptq_amd.utils.sliced import SlicedGemv
    m = spec_to_module(L, dev)
    return m, SlicedGemv(m, **kw)


def _arrivals(sl):
    tables = 1 if sl.exact else len(sl._tensors)
    return sl.slices * tables * sl.parts


SLICED = [
    # (I, O, kw, dt, exact, slices, parts, instance): folded one- and two-table; EX; EX + RG (16-bit residual side stream); column parts;
    # the instance vptq_quant_gemv_sliced_instance must give (every instantiation has its row in tests/test_route_models_sliced_gpu.py)
    (2048, 1032, dict(bias=True), "f16", False, 8, 1,
     "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0"),
    (4104, 264, dict(LLM, num_res_centroids=65536), "bf16", False, 8, 1,
     "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0"),
    (8192, 512, dict(LLM, bias=True), "f16", True, 16, 1,
     "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0"),
    (4712, 136, dict(LLM, num_res_centroids=256), "bf16", True, 16, 1,
     "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0"),
    (2048, 520, dict(LLM, vector_len=8, num_res_centroids=4096, enable_perm=True, bias=True), "f16", True, 8, 1,
     "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=1 corr=0"),
    (1024, 256, dict(LLM, vector_len=16, num_res_centroids=65536), "bf16", True, 16, 1,
     "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0"),
    (16392, 72, dict(LLM), "f16", True, 16, 3,
     "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=0 perm=0 corr=0"),
    (28672, 136, dict(LLM, bias=True), "bf16", True, 16, 2,
     "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0"),
]


def _sliced_instance(sl, tokens):
    """the library's answer for this object's own descriptors and layout structs (a layer in column parts: the grouped entries)"""
    from vptq_amd import _backend as B
    from test_route_models_sliced_gpu import sliced_instance_of, PARTS
    if sl.parts > 1:
        return sliced_instance_of(sl._part_descs, sl._lay_ref, sl.parts, tokens, sl._flags | PARTS)
    return sliced_instance_of((B.LayerDesc * 1)(sl.desc), sl._lay_ref, 1, tokens, sl._flags)


# (ids: the ones these cases had before they carried their instance string)
@pytest.mark.parametrize("I,O,kw,dt,exact,slices,parts,instance", SLICED,
                         ids=[f"{r[0]}-{r[1]}-kw{i}-{r[3]}-{r[4]}-{r[5]}-{r[6]}" for i, r in enumerate(SLICED)])
def test_sliced_one_token_vs_its_model(I, O, kw, dt, exact, slices, parts, instance, dev):
    kw = dict(kw)
    dist = kw.pop("dist", "ref-test")
    kw.setdefault("num_res_centroids", 0)
    L = vo.make_layer(I, O, dist=dist, seed=I + O + 1, dtype=dt, num_centroids=65536, **kw)
    m, sl = _sliced(L, dev, exact=exact)
    assert (sl.exact, sl.slices, sl.parts) == (exact, slices, parts)
    assert _sliced_instance(sl, 1) == instance
    P = am.pieces(L)
    extra = am.sliced_extra_abs(dt, _arrivals(sl))
    for kind in (("dense",) if exact else ("planted",)):
        x, hot = XKIND[kind](I, 1, dt, I)
        xt = bits_to_tensor(x, dt, dev).reshape(x.shape)
        y16, y32 = _np(sl(xt)), _np(sl(xt, flags=F32))
        _check(y16, y32, L, x, dict(arith="exact" if exact else "folded"), hot, extra, P, what=f"sliced {I}x{O} {kind}")


SLICED_TOKENS = [
    # (I, O, kw, dt, exact, tokens, one pass, window parts): the column-phase kernel (folded / EX, 2 - 8 tokens); one pass of the
    # one-token kernel for 2 / 3 tokens (whole columns; window parts); column parts in one pass
    (2048, 1032, dict(bias=True), "f16", False, 2, False, 0,
     "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0"),
    (4104, 264, dict(LLM), "bf16", False, 4, False, 0,
     "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0"),
    (2048, 520, dict(LLM, bias=True), "f16", False, 8, False, 0,
     "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=8 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0"),
    (4104, 264, dict(LLM, bias=True), "f16", True, 5, False, 0,
     "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=8 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0"),
    (2048, 1032, dict(LLM), "bf16", True, 8, False, 0,
     "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=8 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0"),
    (8192, 512, dict(LLM, bias=True), "f16", True, 2, True, 1,
     "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0"),
    (8192, 264, dict(LLM), "bf16", True, 3, True, 1,
     "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0"),
    (4096, 256, dict(LLM), "f16", True, 2, True, 2,
     "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=0 perm=0 corr=0"),
    (14336, 72, dict(LLM), "bf16", True, 3, True, 2,
     "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=0 perm=0 corr=0"),
    (28672, 136, dict(LLM, bias=True), "f16", True, 2, True, 2,
     "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=2 n=1 rpw=2 arrivals=64 whole1=0 side=0 perm=0 corr=0"),
]


@pytest.mark.parametrize("I,O,kw,dt,exact,tokens,one_pass,wparts,instance", SLICED_TOKENS,
                         ids=[f"{r[0]}-{r[1]}-kw{i}-{r[3]}-{r[4]}-{r[5]}-{r[6]}-{r[7]}" for i, r in enumerate(SLICED_TOKENS)])
def test_sliced_tokens_vs_its_model(I, O, kw, dt, exact, tokens, one_pass, wparts, instance, dev):
    kw = dict(kw)
    dist = kw.pop("dist", "ref-test")
    L = vo.make_layer(I, O, dist=dist, seed=I + O + tokens, dtype=dt, num_centroids=65536, num_res_centroids=0, **kw)
    m, sl = _sliced(L, dev, exact=exact)
    assert sl.tokens_supported(tokens)
    assert sl.tokens_one_pass(tokens) == one_pass
    if one_pass:
        assert sl.tokens_window_parts(tokens) == wparts
    assert _sliced_instance(sl, tokens) == instance
    x, hot = (_dense if exact else _planted)(I, tokens, dt, I + tokens)
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, I)
    y16, y32 = sl.forward_tokens(xt), sl.forward_tokens(xt, flags=F32)
    assert y16 is not None and y32 is not None
    # (one pass: the accumulator words, slices x window parts x column parts arrivals; the column-phase kernel adds its partial
    # sums in fp32 in a fixed order - no fixed point)
    extra = am.sliced_extra_abs(dt, _arrivals(sl) * max(wparts, 1)) if one_pass else 0.0
    _check(_np(y16), _np(y32), L, x, dict(arith="exact" if exact else "folded"), hot, extra, what=f"sliced tokens {I}x{O} t{tokens}")


@pytest.mark.parametrize("dt,exact", [("f16", False), ("bf16", True)])
def test_sliced_grouped_siblings_vs_their_models(dt, exact, dev):
    from vptq_amd.utils.sliced import SlicedGroupGemv
    I = 2048
    Ls = [vo.make_layer(I, O, dist="llm", seed=O, dtype=dt, num_centroids=65536, num_res_centroids=0, bias=O == 264)
          for O in (1032, 264, 520)]
    members = [_sliced(L, dev, exact=exact)[1] for L in Ls]
    g = SlicedGroupGemv(members)
    x, hot = (_dense if exact else _planted)(I, 1, dt, 9)
    ys = g(bits_to_tensor(x, dt, dev).reshape(1, 1, I))
    torch.cuda.synchronize()
    for L, sl, y in zip(Ls, members, ys):
        _check(_np(y), None, L, x, dict(arith="exact" if exact else "folded"), hot, am.sliced_extra_abs(dt, _arrivals(sl)),
               what="sliced grouped")


def test_selective_two_table_sliced_vs_its_model(dev):
    """gemv_hot (the hot blocks' exact products) + the folded two-table launch over the rest"""
    I, O = 4096, 520
    L = vo.make_layer(I, O, dist="llm", seed=5, dtype="f16", num_centroids=65536, num_res_centroids=65536, bias=True)
    m, sl = _sliced(L, dev, selective=True)
    assert sl.selective and not sl.exact and len(sl._tensors) == 2
    x, hot = _planted(I, 1, "f16", 17)
    xt = bits_to_tensor(x, "f16", dev).reshape(1, 1, I)
    y16, y32 = _np(sl(xt)), _np(sl(xt, flags=F32))
    _check(y16, y32, L, x, dict(arith="selective"), hot, am.sliced_extra_abs("f16", _arrivals(sl)), what="selective sliced")


# ---------------------------------------------------------------------------------------------- row-parallel shards
SHARD_WORLDS = [2, 4]


@pytest.mark.parametrize("world", SHARD_WORLDS)
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_row_parallel_partials_vs_column_range_model(world, dt, dev):
    """each rank's fp32 partial sum against the model of its column range (output bias on rank 0 only), and their sum against
    the whole layer's"""
    from vptq_amd.utils.shard import shard_in_features, forward_partial_f32
    I, O, T = 4096, 1032, 2
    L = vo.make_layer(I, O, dist="llm", seed=world, dtype=dt, bias=True)
    m = spec_to_module(L, dev)
    P = am.pieces(L)
    x, _ = _dense(I, T, dt, world)
    xt = bits_to_tensor(x, dt, dev).reshape(1, T, I)
    acc = np.zeros((T, O))
    for r in range(world):
        s = shard_in_features(m, r, world)
        c0, c1 = s.shard[1], s.shard[2]
        part = _np(forward_partial_f32(s, xt[..., c0:c1].contiguous())).reshape(T, O)
        mm, aa = am.model(P, x, "exact", cols=(c0, c1), with_bias=r == 0)
        am.check_outputs(part, mm, aa, dt, True, what=f"rank {r} of {world}")
        acc += part
    mm, aa = am.model(P, x, "exact")
    am.check_outputs(acc, mm, aa, dt, True, what=f"sum of {world} partials")


# ---------------------------------------------------------------------------------------------- coverage of the table
# every route of the issue's table; a table entry reaches it only through a test that asserts the route before it checks outputs
# (kernel-name queries, the chain / grouped name queries, the sliced objects' slice count, form, parts and one-pass answer)
REQUIRED = {"gemv_k256_kernel", "gemv_k256_kernel<fast>", "gemv_k256m_kernel", "gemv_k256m_kernel<fast>", "gemv_k256m_kernel<selective>",
            "gemv_k256c_kernel", "vptq_quant_gemv_grouped", "gemm_k256t_kernel", "gemm_k256_kernel", "vptq_quant_gemm",
            "gemv_lds_kernel", "gemv_lds_mfma_kernel", "gemv_gather_kernel", "gemv_gatherx_kernel", "gemv_generic_kernel",
            "gemv_sliced_kernel", "gemv_sliced_tok_kernel", "gemv_hot_kernel", "row-parallel shards",
            "gemv_v2_kernel", "vptq_quant_gemv_v2"}


def _reached():
    """-> {route: set of (form, dtype, tokens, ...) cases} over every table of this file"""
    r = {}

    def add(route, *case):
        r.setdefault(route, set()).add(case)
    for p in ONE_LAYER:
        e = p.values[0]
        add(e["route"], e["arith"], e["dt"], e["tokens"])
    # (every instantiation of the remaining families and the v2 entry: tests/test_route_models_other_gpu.py)
    import test_route_models_other_gpu as other
    for p in other.ALL_ROWS:
        e = p.values[0]
        add(e["instance"].split()[0] + "_kernel", e["arith"], e["dt"], e["tokens"])
        if e["entry"] == "v2":
            add("vptq_quant_gemv_v2", e["instance"].split()[0], e["dt"], e["tokens"])
    for shapes, dt, tokens, flags, route, arith in GROUPS:
        add("vptq_quant_gemv_grouped", route, arith, dt, len(shapes), len({repr(sh) for sh in shapes}) == 1)
    for dt in ("f16", "bf16"):
        for arith in CHAIN_INDEPENDENT:
            add("gemv_k256c_kernel", "independent", arith, dt)
        for arith in CHAIN_DEPENDENT:
            add("gemv_k256c_kernel", "dependent", arith, dt)
    for I, O, dt, tokens, arith, kw in FUSED:
        add("vptq_quant_gemm", arith, dt)
    for I, O, kw, dt, exact, slices, parts, _ in SLICED:
        kr = kw.get("num_res_centroids", 0)
        add("gemv_sliced_kernel", "folded" if not exact else "EX+RG" if kr and not (kw.get("vector_len", 8) == 8 and kr == 256) else "EX",
            dt, 1, "column parts" if parts > 1 else "whole")
    for I, O, kw, dt, exact, tokens, one_pass, wparts, _ in SLICED_TOKENS:
        if one_pass:
            add("gemv_sliced_kernel", "EX", dt, tokens, f"one pass, {wparts} window part(s)")
        else:
            add("gemv_sliced_tok_kernel", "EX" if exact else "folded", dt, tokens)
    add("gemv_sliced_kernel", "grouped")                            # test_sliced_grouped_siblings_vs_their_models
    add("gemv_hot_kernel", "selective", "f16", "two-table")         # test_selective_two_table_sliced_vs_its_model
    for w in SHARD_WORLDS:
        add("row-parallel shards", w)
    return r


def test_route_table_reaches_every_kernel():
    """the routes the tables reach include every route of the list above, in the forms, dtypes and token counts asked for:
    coverage cannot shrink unnoticed"""
    r = _reached()
    assert REQUIRED <= set(r), sorted(REQUIRED - set(r))
    has = lambda route, pred: any(pred(c) for c in r[route])   # noqa: E731
    for name in ("gemv_k256m_kernel", "gemv_k256m_kernel<fast>", "gemv_k256m_kernel<selective>"):
        assert {c[1] for c in r[name]} == {"f16", "bf16"}, name
    assert {c[2] for c in r["gemv_k256m_kernel"] | r["gemv_k256m_kernel<fast>"]} >= {1, 2, 3, 4}
    assert {c[2] for c in r["gemm_k256t_kernel"]} >= {1, 16}
    assert all(5 <= c[2] <= 16 for c in r["gemm_k256_kernel"]) and {c[1] for c in r["gemm_k256_kernel"]} == {"f16", "bf16"}
    assert {("exact", "f16"), ("folded", "bf16")} <= r["vptq_quant_gemm"]
    assert {(k, a) for k, a, _ in r["gemv_k256c_kernel"]} >= {("independent", "exact"), ("independent", "folded"),
                                                               ("independent", "selective"), ("dependent", "folded")}
    assert has("vptq_quant_gemv_grouped", lambda c: c[4]) and has("vptq_quant_gemv_grouped", lambda c: not c[4])
    sl = r["gemv_sliced_kernel"]
    for form in ("folded", "EX", "EX+RG"):
        assert has("gemv_sliced_kernel", lambda c: c[0] == form), form
    assert has("gemv_sliced_kernel", lambda c: len(c) > 3 and c[3] == "column parts")
    assert {c[2] for c in sl if len(c) > 3 and str(c[3]).startswith("one pass")} >= {2, 3}
    assert has("gemv_sliced_kernel", lambda c: len(c) > 3 and str(c[3]).startswith("one pass, 2"))
    assert ("grouped",) in sl
    tok = r["gemv_sliced_tok_kernel"]
    assert {c[0] for c in tok} == {"folded", "EX"} and min(c[2] for c in tok) == 2 and max(c[2] for c in tok) == 8
    assert {c[0] for c in r["row-parallel shards"]} >= {2, 4}
    assert {c[0] for c in r["vptq_quant_gemv_v2"]} == {"gemv_lds", "gemv_lds_mfma", "gemv_v2"}
    assert {c[1] for c in r["gemv_v2_kernel"]} == {"f16", "bf16"} and {c[2] for c in r["gemv_v2_kernel"]} >= {1, 2, 3, 4, 7, 9}


# ---------------------------------------------------------------------------------------------- the sliced entry points' flags
def _tok_call(sl, x, tokens, flags):
    """vptq_quant_gemv_sliced_tokens / _tokens_grouped (column parts) with exactly `flags`: -> (rc, y)"""
    from vptq_amd import _backend as B
    sp = B.current_stream_ptr(sl.dev)
    ws = sl._tokens_workspace(sp, tokens)
    y = torch.empty(1, tokens, sl.layer.out_features, dtype=x.dtype, device=sl.dev)
    if sl.parts > 1:
        yp = (C.c_void_p * sl.parts)(*([y.data_ptr()] * sl.parts))
        wp = (C.c_void_p * sl.parts)(*([ws.data_ptr()] * sl.parts))
        wb = (C.c_size_t * sl.parts)(*([ws.numel()] * sl.parts))
        rc = B.lib().vptq_quant_gemv_sliced_tokens_grouped(sl._part_descs, sl._lay_ref, sl.parts, x.data_ptr(), yp, tokens,
                                                           flags | B.GEMV_COLUMN_PARTS, wp, wb, sp)
    else:
        rc = B.lib().vptq_quant_gemv_sliced_tokens(sl.desc, sl._lay_ref, x.data_ptr(), y.data_ptr(), tokens, flags, ws.data_ptr(),
                                                   ws.numel(), sp)
    torch.cuda.synchronize()
    return rc, y


def _grouped_call(sl, x, flags):
    """vptq_quant_gemv_sliced_grouped of one layer (or its column parts) with exactly `flags`"""
    from vptq_amd import _backend as B
    sp = B.current_stream_ptr(sl.dev)
    ws = sl._workspace(sp)
    y = torch.empty(1, 1, sl.layer.out_features, dtype=x.dtype, device=sl.dev)
    n = sl.parts
    descs = sl._part_descs if n > 1 else (B.LayerDesc * 1)(sl.desc)
    yp = (C.c_void_p * n)(*([y.data_ptr()] * n))
    wp = (C.c_void_p * n)(*([ws.data_ptr()] * n))
    wb = (C.c_size_t * n)(*([sl._ws_bytes] * n))
    rc = B.lib().vptq_quant_gemv_sliced_grouped(descs, sl._lay_ref, n, x.data_ptr(), yp, flags | (B.GEMV_COLUMN_PARTS if n > 1 else 0),
                                                wp, wb, sp)
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("entry", ["tokens", "grouped", "tokens_grouped"])
def test_sliced_entry_points_take_selective_as_exact(entry, dev):
    """VPTQ_GEMV_SELECTIVE on vptq_quant_gemv_sliced_tokens / _grouped / _tokens_grouped, which implement no selective form: over an
    EXACT layout the call gives the exact result, bit-identical to the VPTQ_GEMV_EXACT call, never the folded form"""
    from vptq_amd import _backend as B
    dt = "f16"
    if entry == "tokens_grouped":   # (column parts of one layer, 2 tokens in one pass)
        I, O, tokens = 28672, 136, 2
    else:
        I, O, tokens = 4096, 264, (3 if entry == "tokens" else 1)
    L = vo.make_layer(I, O, dist="llm", seed=I + 3, dtype=dt, num_centroids=65536, num_res_centroids=0, bias=True)
    m, sl = _sliced(L, dev, exact=True)
    x, hot = _planted(I, tokens, dt, 4)
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, I)
    call = (lambda f: _grouped_call(sl, xt, f)) if entry == "grouped" else (lambda f: _tok_call(sl, xt, tokens, f))
    rc, want = call(EXACT)
    assert rc == 0
    extra = am.sliced_extra_abs(dt, _arrivals(sl) * max(sl.tokens_window_parts(tokens), 1))
    _check(_np(want), None, L, x, dict(arith="exact"), hot, extra, what=f"{entry} EXACT")
    for flags in (SEL, SEL | EXACT):
        rc, y = call(flags)
        assert rc == 0, (flags, rc, B.lib().vptq_last_error())
        _check(_np(y), None, L, x, dict(arith="exact"), hot, extra, what=f"{entry} flags {flags}")
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)), f"{entry} flags {flags}: not the EXACT call's bits"


@pytest.mark.parametrize("entry", ["tokens", "grouped"])
def test_sliced_entry_points_never_return_folded_for_selective(entry, dev):
    """VPTQ_GEMV_SELECTIVE over a FOLDED layout: VPTQ_E_UNSUPPORTED or the exact result, never the folded output"""
    from vptq_amd import _backend as B
    dt = "f16"
    I, O, tokens = 4096, 264, (2 if entry == "tokens" else 1)
    L = vo.make_layer(I, O, dist="llm", seed=I + 4, dtype=dt, num_centroids=65536, num_res_centroids=0, bias=True)
    m, sl = _sliced(L, dev, exact=False)
    x, hot = _planted(I, tokens, dt, 6)
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, I)
    rc, y = _grouped_call(sl, xt, SEL) if entry == "grouped" else _tok_call(sl, xt, tokens, SEL)
    if rc == B.E_UNSUPPORTED:
        return
    assert rc == 0, B.lib().vptq_last_error()
    extra = am.sliced_extra_abs(dt, 32)
    _check(_np(y), None, L, x, dict(arith="exact"), hot, extra, what=f"{entry} SELECTIVE over a folded layout")


# ---------------------------------------------------------------------------------------------- the accumulator word's range
@pytest.mark.parametrize("dt,slices", [("f16", 8), ("bf16", 8), ("f16", 16), ("bf16", 16)])
def test_sliced_sums_beyond_the_accumulator_range(dt, slices, dev):
    """VPTQ_GEMV_OUT_F32 with every slice's partial sum below the per-partial limit (2^17 fp16 / 2^19 bf16) and the total above the
    50-bit field (2^19 / 2^21): each output meets the model or is NaN - never a wrong finite value; 16-bit outputs never an inf of
    the wrong sign.  Sums inside the range still meet the model."""
    F = am.FIX_F[dt]
    I = 4096 if slices == 8 else 16384                         # (folded: 16 slices of 4096 entries beyond 14336 columns)
    O = 72
    L = vo.make_layer(I, O, dist="llm", seed=slices, dtype=dt, num_centroids=65536, num_res_centroids=0)
    # every centroid entry positive near 1, scale 1, bias 0: each slice holds ~I / slices elements of every row, whose terms add up
    L.weight_scale = vo.from_f32(np.ones(I, np.float32), dt)
    L.weight_bias = vo.from_f32(np.zeros(I, np.float32), dt)
    rng = np.random.default_rng(1)
    L.centroids = vo.from_f32(rng.uniform(0.9, 1.1, L.centroids.shape).astype(np.float32), dt)
    m, sl = _sliced(L, dev)
    assert sl.slices == slices and len(sl._tensors) == 1
    P = am.pieces(L)
    extra = am.sliced_extra_abs(dt, slices)
    lim_partial, field = 2.0 ** (47 - F), 2.0 ** (49 - F)
    for total in (0.25 * field, 1.5 * field):       # inside the field / beyond it, each partial ~total / slices < lim_partial
        assert total / slices < 0.8 * lim_partial
        xv = total / I
        x = vo.from_f32(np.full((1, 1, I), xv, np.float32), dt)
        xt = bits_to_tensor(x, dt, dev).reshape(1, 1, I)
        mm, aa = am.model(P, x, "folded")
        y32, y16 = _np(sl(xt, flags=F32)), _np(sl(xt))
        am.check_outputs(y32, mm, aa, dt, True, extra, allow_nan=total > field, what=f"fp32 total {total:.3g}")
        am.check_outputs(y16, mm, aa, dt, False, extra, allow_nan=total > field, what=f"16-bit total {total:.3g}")
