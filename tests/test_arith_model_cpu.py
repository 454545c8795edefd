"""The per-output models of tests/_arith_model.py are sharp (no GPU): fp32 sums of the model's own terms in every order a
kernel uses pass the checker, and each kind of kernel bug the max-normalised parity bar lets through is rejected."""
import numpy as np
import pytest

from oracle import vptq_oracle as vo
import _arith_model as am


def _x(I, tokens, dt, kind, seed):
    """dense N(0, 1) activations, or 'massive': two channels at 60 - 80 x rms, the rest within 3 x rms"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((tokens, I))
    if kind == "massive":
        x = np.clip(x, -3, 3)
        for t in range(tokens):
            cols = rng.choice(I, 2, replace=False)
            x[t, cols] = rng.uniform(60, 80, 2) * rng.choice([-1, 1], 2)
    return vo.from_f32(x.astype(np.float32), dt).reshape(1, tokens, I)


def _terms(P, x_bits):
    """the exact model's products x_j w_oj as fp32 (16 x 16-bit products are exact in fp32): [tokens, O, I]"""
    I = P["W"].shape[1]
    x = vo.to_f32(np.asarray(x_bits), P["dtype"]).reshape(-1, I).astype(np.float32)
    return x[:, None, :] * P["W"].astype(np.float32)[None, :, :]


def _seq(t):
    acc = np.zeros(t.shape[:-1], np.float32)
    for j in range(t.shape[-1]):
        acc = acc + t[..., j]
    return acc


def _blocked(t, lanes=64):
    K = t.shape[-1]
    pad = (-K) % lanes
    u = np.concatenate([t, np.zeros(t.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(t.shape[:-1] + (-1, lanes))
    acc = np.zeros(u.shape[:-2] + (lanes,), np.float32)
    for k in range(u.shape[-2]):
        acc = acc + u[..., k, :]
    return _pairwise(acc)


def _pairwise(t):
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,), np.float32)], axis=-1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _fixed(t, arrivals, dt, wrap=False):
    """sliced kernels: `arrivals` fp32 partial sums (columns dealt round-robin), each truncated towards zero to units of 2^-F,
    added as integers (wrap: in a 50-bit two's-complement field, as the accumulator word does), one conversion back"""
    F = am.FIX_F[dt]
    q = np.zeros(t.shape[:-1], dtype=object)
    for s in range(arrivals):
        part = _seq(t[..., s::arrivals]).astype(np.float64)
        q = q + np.vectorize(lambda v: int(np.trunc(v * 2.0 ** F)), otypes=[object])(part)
    if wrap:
        q = np.vectorize(lambda v: ((v + 2 ** 49) % 2 ** 50) - 2 ** 49, otypes=[object])(q)
    return np.vectorize(lambda v: float(v), otypes=[np.float64])(q) * 2.0 ** -F


def _finish(s, P, out_f32, dt):
    y = (np.asarray(s, np.float32) + P["bias"].astype(np.float32)[None, :]).astype(np.float32)
    return y if out_f32 else vo.round_to(y, dt)


def _layer(I, O, dt, seed, bias=True):
    return vo.make_layer(I, O, dist="llm", seed=seed, dtype=dt, bias=bias)


SUMS = {
    "sequential": _seq,
    "blocked64": _blocked,
    "pairwise": _pairwise,
}


@pytest.mark.parametrize("kind", ["dense", "massive"])
@pytest.mark.parametrize("I", [64, 8192, 28672])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_correct_fp32_sums_pass_in_every_order(dt, I, kind):
    O = 64 if I > 64 else 72
    L = _layer(I, O, dt, I + 3)
    P = am.pieces(L)
    x = _x(I, 2, dt, kind, I)
    m, a = am.model(P, x)
    t = _terms(P, x)
    for name, fn in SUMS.items():
        s = fn(t)
        for out_f32 in (True, False):
            am.check_outputs(_finish(s, P, out_f32, dt), m, a, dt, out_f32, what=f"{name} {dt} I={I} {kind}")
    for arrivals in (8, 16, 32):
        s = _fixed(t, arrivals, dt)
        extra = am.sliced_extra_abs(dt, arrivals)
        for out_f32 in (True, False):
            am.check_outputs(_finish(s, P, out_f32, dt), m, a, dt, out_f32, extra, what=f"fixed x{arrivals} {dt} I={I} {kind}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_folded_and_selective_models_pass_their_own_sums(dt):
    """fp32 sums of the folded form's terms pass the folded model; the selective model with no hot block is the folded one,
    with every block hot the exact one"""
    I, O = 1024, 96
    L = _layer(I, O, dt, 77)
    P = am.pieces(L)
    x = _x(I, 1, dt, "massive", 5)
    xf = vo.to_f32(x, dt).reshape(1, I).astype(np.float64)
    sx = vo.round_to((P["s"] * xf).astype(np.float32), dt)
    t = np.concatenate([sx[:, None, :] * P["c"].astype(np.float32)[None], sx[:, None, :] * P["r"].astype(np.float32)[None],
                        np.broadcast_to((xf * P["b"]).astype(np.float32)[:, None, :], (1, O, I))], axis=-1)
    m, a = am.model(P, x, "folded")
    for fn in SUMS.values():
        for out_f32 in (True, False):
            am.check_outputs(_finish(fn(t), P, out_f32, dt), m, a, dt, out_f32, what="folded")
    ms, as_ = am.model(P, x, "selective", hot_blocks=())
    assert np.array_equal(ms, m) and np.array_equal(as_, a)
    me, ae = am.model(P, x, "exact")
    ms, as_ = am.model(P, x, "selective", hot_blocks=range(I // am.BLOCK))
    assert np.allclose(ms, me, rtol=0, atol=1e-12) and np.allclose(as_, ae, rtol=0, atol=1e-12)
    # column ranges add up to the whole layer; the bias counted once
    parts = [am.model(P, x, "exact", cols=(c0, c0 + 256), with_bias=c0 == 0)[0] for c0 in range(0, I, 256)]
    assert np.allclose(sum(parts), me, rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- mutants
def _rejected(y, m, a, dt, out_f32, extra=0.0):
    bad, _, _ = am.violations(y, m, a, dt, out_f32, extra)
    with pytest.raises(AssertionError):
        am.check_outputs(y, m, a, dt, out_f32, extra)
    return bad


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_mutants_are_rejected(dt, out_f32):
    I, O, T = 8192, 64, 2
    L = _layer(I, O, dt, 11)
    L.bias[-1] = vo.from_f32(np.array([0.75], np.float32), dt)[0]   # (a bias well above the output's ulp)
    P = am.pieces(L)
    x = _x(I, T, dt, "dense", 12)
    m, a = am.model(P, x)
    t = _terms(P, x)
    good = _finish(_seq(t), P, out_f32, dt)
    am.check_outputs(good, m, a, dt, out_f32)

    # one column's term dropped (the column of the largest |x| of token 0): rejected on nearly every output
    j = int(np.argmax(np.abs(vo.to_f32(x, dt).reshape(T, I)[0])))
    t1 = t.copy()
    t1[:, :, j] = 0
    bad = _rejected(_finish(_seq(t1), P, out_f32, dt), m, a, dt, out_f32)
    assert bad[0].mean() >= (0.99 if out_f32 else 0.8), bad[0].mean()   # (bf16 outputs: the term is a few ulps)

    # one output row replaced by its neighbour
    y = good.copy()
    y[:, 5] = y[:, 6]
    _rejected(y, m, a, dt, out_f32)

    # bias missing on the last output
    assert abs(P["bias"][-1]) > 8 * am.ulp16(m[:, -1], dt).max()
    s = _seq(t)
    y = _finish(s, P, out_f32, dt)
    y[:, -1] = (s[:, -1] if out_f32 else vo.round_to(s[:, -1], dt))
    _rejected(y, m, a, dt, out_f32)

    # the residual entry missing for one element (the column of the largest |x|, the output whose residual entry there is largest)
    o = int(np.argmax(np.abs(P["r"][:, j])))
    c, r = P["c"][o, j], P["r"][o, j]
    w_no_r = vo.round_to(vo.round_to(np.float32(c) * np.float32(P["s"][j]), dt) + np.float32(P["b"][j]), dt)
    assert r != 0 and w_no_r != P["W"][o, j]
    t1 = t.copy()
    t1[:, o, j] = vo.to_f32(x, dt).reshape(T, I)[:, j] * np.float32(w_no_r)
    bad = _rejected(_finish(_seq(t1), P, out_f32, dt), m, a, dt, out_f32)
    assert bad[0, o]

    # the wrong token's activation for one block of 128 columns (token 0 reads token 1's block 7)
    xm = np.asarray(x).reshape(T, I).copy()
    xm[0, 7 * 128:8 * 128] = xm[1, 7 * 128:8 * 128]
    y = _finish(_seq(_terms(P, xm)), P, out_f32, dt)
    bad = _rejected(y, m, a, dt, out_f32)
    assert bad[0].mean() >= 0.9 and not bad[1].any()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_folded_output_is_not_the_exact_arithmetic(dt):
    """on massive-channel activations the folded form's (exactly evaluated) outputs fail the exact model: the models tell the
    arithmetics apart, so a route that drifts from one to the other is caught"""
    I, O = 4096, 256
    L = _layer(I, O, dt, 21)
    P = am.pieces(L)
    x = _x(I, 1, dt, "massive", 22)
    mf, af = am.model(P, x, "folded")
    me, ae = am.model(P, x, "exact")
    y = vo.round_to(mf.astype(np.float32), dt)
    am.check_outputs(y, mf, af, dt, False)
    bad = _rejected(y, me, ae, dt, False)
    assert bad.sum() >= 4


@pytest.mark.parametrize("dt,arrivals", [("f16", 8), ("bf16", 8), ("f16", 16), ("bf16", 16)])
def test_wrapped_fixed_point_sum_is_rejected(dt, arrivals):
    """partial sums each inside the sliced accumulator's per-partial limit (2^17 / 2^19) whose total leaves the 50-bit field
    (2^19 / 2^21): the wrapped total is a wrong finite value, and the checker says so"""
    F = am.FIX_F[dt]
    part = 0.75 * 2.0 ** (47 - F)                    # below the per-partial limit
    assert arrivals * part >= 2.0 ** (49 - F)         # the total is not representable
    t = np.full((1, 1, arrivals), part, np.float32)
    m = np.array([[arrivals * part]])
    a = m.copy()
    y = _fixed(t, arrivals, dt, wrap=True).astype(np.float32)
    assert np.isfinite(y).all() and y[0, 0] != m[0, 0]
    _rejected(y, m, a, dt, True, am.sliced_extra_abs(dt, arrivals))
    # ... and the unwrapped total passes
    am.check_outputs(_fixed(t, arrivals, dt).astype(np.float32), m, a, dt, True, am.sliced_extra_abs(dt, arrivals))


def test_overflow_and_nan_rules():
    m = np.array([[7e4, -7e4, 100.0, 65000.0]])
    a = np.abs(m)
    y = np.array([[np.inf, -np.inf, 100.0, 65024.0]])
    am.check_outputs(y, m, a, "f16", False)
    for bad in ([[-np.inf, -np.inf, 100.0, 65024.0]], [[65504.0, -np.inf, 100.0, 65024.0]], [[np.inf, -np.inf, np.nan, 65024.0]],
                [[np.inf, -np.inf, 100.0, np.inf]]):
        with pytest.raises(AssertionError):
            am.check_outputs(np.array(bad), m, a, "f16", False)
    am.check_outputs(np.array([[np.inf, -np.inf, np.nan, 65024.0]]), m, a, "f16", False, allow_nan=True)


# ---------------------------------------------------------------------------------------------- the row-block form, the v2 pieces
BLOCK_LAYERS = [
    dict(I=520, O=100, kw=dict(num_centroids=4096, num_res_centroids=256, bias=True, enable_perm=True)),
    dict(I=4 * 260 + 8, O=98, kw=dict(vector_len=8, num_centroids=4096, num_res_centroids=16, num_codebooks=4, outlier_size=8,
                                      outlier_vector_len=4, num_outlier_centroids=256, bias=True)),
    dict(I=264, O=85, kw=dict(vector_len=12, num_centroids=256, num_res_centroids=0, outlier_size=4, outlier_vector_len=12,
                              num_outlier_centroids=256, enable_norm=False)),
]


@pytest.mark.parametrize("spec", BLOCK_LAYERS, ids=[f"{s['I']}x{s['O']}" for s in BLOCK_LAYERS])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_blocked_model_equals_the_whole_model_bit_for_bit(spec, dt):
    """pieces_blocks / model_blocks (row blocks of a few vector-rows: index rows, outlier index rows and output bias sliced,
    the rest shared) give the values of pieces + model, bit for bit, for every arithmetic - a large row checked block by block is
    checked against the same numbers"""
    L = vo.make_layer(spec["I"], spec["O"], dist="llm", seed=3, dtype=dt, **spec["kw"])
    P = am.pieces(L)
    x = _x(spec["I"], 3, dt, "massive", 5)
    limit = 3 * L.vector_len * L.in_features          # three vector-rows per block: several blocks, a short last one
    blocks = list(am.pieces_blocks(L, limit))
    assert len(blocks) > 2 and blocks[0][0] == (0, 3) and blocks[-1][1][1] == spec["O"]
    for (n0, n1), (o0, o1), Pb in blocks:
        for key in ("c", "r", "W"):
            assert np.array_equal(Pb[key], P[key][o0:o1]), key
        assert np.array_equal(Pb["bias"], P["bias"][o0:o1]) and np.array_equal(Pb["s"], P["s"]) and np.array_equal(Pb["b"], P["b"])
    for arith, kw in (("exact", {}), ("folded", {}), ("folded", dict(rounded=True)), ("folded", dict(round_sx=False))):
        m, a = am.model(P, x, arith, **kw)
        got = list(am.model_blocks(L, x, arith, limit, **kw))
        assert [r for r, _, _ in got] == [b[1] for b in blocks]
        assert np.array_equal(np.concatenate([mb for _, mb, _ in got], axis=1), m), arith
        assert np.array_equal(np.concatenate([ab for _, _, ab in got], axis=1), a), arith


@pytest.mark.parametrize("dt,kr,rb", [("f16", 256, np.uint8), ("bf16", 512, np.uint16), ("f16", 0, None)])
def test_v2_pieces_are_the_packed_layers_pieces(dt, kr, rb):
    """pieces_v2 of a packed layer's own ids and tables (one codebook, no permutation: the same weights in the v2 wire format)
    equals pieces(L) - c, r, s, b, bias and the exact W - so model() and check_outputs() take the v2 rows unchanged"""
    I, O, v = 264, 72, 8
    L = vo.make_layer(I, O, dist="ref-test", seed=9, dtype=dt, num_centroids=1024, num_res_centroids=kr, bias=True)
    idx, ridx = vo.unpack_indices(L.indices, L.index_bits, I, L.res_bits, False)
    P2 = am.pieces_v2(dt, I, O, v, idx[0].reshape(-1).astype(np.uint16), L.centroids, None if not kr else ridx[0].reshape(-1).astype(rb),
                      L.res_centroids if kr else None, L.weight_scale.reshape(I, 1), L.weight_bias.reshape(I, 1), L.bias.reshape(1, O))
    P = am.pieces(L)
    for key in ("c", "r", "s", "b", "bias", "W"):
        assert np.array_equal(P2[key], P[key]), key
    x = _x(I, 2, dt, "dense", 1)
    for arith in ("exact", "folded"):
        assert all(np.array_equal(u, w) for u, w in zip(am.model(P2, x, arith), am.model(P, x, arith)))


# ---------------------------------------------------------------------------------------------- bf16 gemv_lds: which arithmetic ran
def _bf16_lds_rows():
    import test_route_models_other_gpu as other
    return [p for p in other.ALL_ROWS if p.values[0]["instance"].startswith("gemv_lds ") and p.values[0]["dt"] == "bf16"
            and not p.values[0].get("big")]


@pytest.mark.parametrize("e", _bf16_lds_rows())
def test_bf16_lds_rows_tell_the_two_arithmetics_apart(e):
    """gemv_lds computes bf16 in the folded form with s x unrounded and c + r kept in fp32; every bf16 row of it (packed and v2) must
    be able to tell that from the reference's roundings: on the row's own planted input the exact model's values violate the
    folded-unrounded bounds at some output, and the folded-unrounded model's values violate the exact bounds at some output (the
    fp32 output's bounds: the row checks that output too)"""
    import test_route_models_other_gpu as other
    assert e["arith"] == "folded" and e["rounded"] is False and e["round_sx"] is False and e["x"] == "planted"
    if e["entry"] == "v2":
        P, perm = other.v2_pieces(e, other.v2_tensors(e)), None
    else:
        L = other.layer_of(e)
        P, perm = am.pieces(L), L.perm
    x, _ = other.x_of(e, perm)
    mf, af = am.model(P, x, "folded", **other.FOLDED_UNROUNDED)
    me, ae = am.model(P, x, "exact")
    assert am.violations(me, mf, af, "bf16", True)[0].any(), "the exact values pass as folded-unrounded ones"
    assert am.violations(mf, me, ae, "bf16", True)[0].any(), "the folded-unrounded values pass as exact ones"
