"""The special-value layers (tests/_dequant_specials.py) without a GPU: what the oracle makes of them is what torch's own CPU
arithmetic makes of them - through the restatement of the reference's tensor ops in oracle/torch_ref.py - NaN by position, every
other element bit for bit.  The GPU rows then hold the kernels to the reference's semantics, not to the oracle's opinion of them.
The C oracle agrees on the same layers, and the tables still reach every class they were written for.  The finite table of the
GEMV tests (tests/test_weight_bits_gpu.py) and the overflow layer are pinned the same way, and the finite table's POWER: each of
nine wrong arithmetics - a fused multiply-add, an unrounded sum, a flush or a truncation in one of the three roundings - must
change at least 100 of its weights."""
import numpy as np
import pytest
import torch

from oracle import vptq_oracle as vo
from oracle import c_oracle, torch_ref
import _dequant_specials as sp

# (numpy reports the overflows and invalid operations the tables are there to provoke)
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
# (v, k, kr): the layers of test_dequant_models_gpu.py (TAB 1, 2, 0) and of test_dequant_sliced_gpu.py
LAYERS = [(8, 16, 16), (8, 65536, 16), (8, 65536, 2048), (8, 65536, 0), (8, 65536, 256), (16, 65536, 65536)]


def _t(bits, dt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(TORCH_DT[dt])


def torch_dequant(L):
    dt = L.dtype
    W = torch_ref.dequant(torch.from_numpy(np.ascontiguousarray(L.indices).view(np.int32).copy()), _t(L.centroids, dt),
                          _t(L.res_centroids, dt) if L.num_res_centroids > 0 else None, _t(L.weight_scale, dt), _t(L.weight_bias, dt),
                          num_centroids=L.num_centroids, num_res_centroids=L.num_res_centroids, vector_len=L.vector_len,
                          group_size=L.group_size, out_features=L.out_features)
    return W.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("v,k,kr", LAYERS, ids=lambda p: str(p))
def test_oracle_is_torch_cpu_arithmetic_on_the_special_values(v, k, kr, dt):
    L = sp.special_layer(dt, v, k, kr)
    want = torch_dequant(L)
    sp.same_bits(vo.dequant(L, ref_residual_mask_quirk=False), want, dt, "oracle against torch")
    # (res_bits <= index_bits in every layer: the reference's residual mask is the same)
    sp.same_bits(vo.dequant(L, ref_residual_mask_quirk=True), want, dt, "oracle (reference's mask) against torch")
    if c_oracle.available():
        sp.same_bits(c_oracle.dequant(L, quirk=False), want, dt, "C oracle against torch")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_table_reaches_its_classes(dt):
    """every (centroid, residual) pair meets every (scale, bias) pair, and W holds NaNs, infinities from overflow, both zeros and
    subnormals - counted on the oracle's result"""
    L = sp.special_layer(dt)
    idx, ridx = vo.unpack_indices(L.indices, L.index_bits, L.group_size, L.res_bits, False)
    sb = np.arange(L.in_features) // sp.COLS_PER_SB
    seen = {(int(c), int(r), int(p)) for n in range(sp.ROWS) for c, r, p in zip(idx[0, n], ridx[0, n], sb)}
    assert len(seen) == 16 * 16 * 64
    cov = sp.coverage(L)
    assert all(cov[key] > 0 for key in ("nan", "inf", "pos_zero", "neg_zero", "subnormal", "finite")), cov
    cent, res, scale, bias = sp.tables(dt)
    f = sp.FMT[dt]
    r16 = lambda x: float(vo.round_to(np.array([x], np.float32), dt)[0])   # noqa: E731
    # the ties the table was written for are ties: the exact sum lies halfway between two neighbours, and both parities occur
    one, nxt = 1.0, 1.0 + f["eps"]
    assert r16(one + f["eps"] / 2) == one and r16(nxt + f["eps"] / 2) == nxt + f["eps"]
    assert r16(one + 3 * f["eps"] / 2) == nxt + f["eps"] and r16(nxt + 3 * f["eps"] / 2) == nxt + f["eps"]
    assert r16(f["big"] + f["half_ulp_big"]) == float("inf") and r16(f["big"] + f["half_ulp_big"] / 2) == f["big"]
    assert r16(3 * f["sub"] * 0.5) == 2 * f["sub"] and r16(f["sub"] * 0.5) == 0.0 and r16(f["root"] * f["root"]) == float("inf")
    assert r16(nxt * 1.5) == 1.5 + 2 * f["eps"]
    for need, have in ((one, cent), (nxt, cent), (f["eps"] / 2, res[0]), (3 * f["eps"] / 2, res[0]), (f["half_ulp_big"], res[0]),
                       (3 * f["sub"], cent), (f["sub"], cent), (f["root"], cent), (0.5, scale), (1.5, scale), (f["root"], scale),
                       (f["eps"] / 2, bias)):
        assert need in have


# ---------------------------------------------------------------------------------------------- the finite table and its power
# coverage() of special_layer(dt, finite=True) and of overflow_layer(dt): a table that lost an edge case fails its pin
FINITE_COVERAGE = {
    "f16": dict(nan=0, inf=0, pos_zero=1732, neg_zero=228, subnormal=7480, finite=133632),
    "bf16": dict(nan=0, inf=0, pos_zero=1808, neg_zero=228, subnormal=7360, finite=133632),
}
OVERFLOW_COVERAGE = {
    "f16": dict(nan=0, inf=64, pos_zero=0, neg_zero=0, subnormal=26, finite=18368),
    "bf16": dict(nan=0, inf=64, pos_zero=9, neg_zero=0, subnormal=0, finite=18368),
}
# the share of the finite table's weights a bf16 GEMV may read as a zero (tests/test_weight_bits_gpu.py): weights in the subnormal
# range (the dot-block kernels), non-zero weights below 2^-21 (the sliced routes' 2^-28 accumulator unit).  Below 15 % of the table.
SHARE_LIMIT = 0.15
MIN_DIFFERENT = 100       # weights in which every mutant must differ from the reference's three roundings


def _r16(x, dt):
    with np.errstate(over="ignore", invalid="ignore"):
        return vo.to_f32(vo.from_f32(np.asarray(x, np.float64).astype(np.float32), dt), dt).astype(np.float64)


def _rtz(x, dt):
    """x (float64) truncated to the 16-bit grid: the nearest value, one step towards zero where that one is larger in magnitude"""
    with np.errstate(over="ignore", invalid="ignore"):
        bits = vo.from_f32(np.asarray(x, np.float64).astype(np.float32), dt)
    q = vo.to_f32(bits, dt).astype(np.float64)
    return vo.to_f32(np.where(np.abs(q) > np.abs(x), bits - 1, bits).astype(np.uint16), dt).astype(np.float64)


def _flush(x, dt):
    """subnormal values of the 16-bit format -> zero of the same sign"""
    return np.where(np.abs(x) < sp.FMT[dt]["norm"], np.copysign(0.0, x), x)


def mutants(L):
    """-> {name: W as float64}: the reference's chain with one thing wrong.  Computed in float64 (sums and products of 16-bit values
    are exact there but for a few of the widest exponent gaps) and rounded with the oracle's own from_f32."""
    dt = L.dtype
    c, r, s, b = sp.operands(L)
    r16, rtz, fl = (lambda x: _r16(x, dt)), (lambda x: _rtz(x, dt)), (lambda x: _flush(x, dt))   # noqa: E731
    q = r16(c + r)
    return {
        "fma of scale and bias": r16(q * s + b),
        "unrounded c + r": r16(r16((c + r) * s) + b),
        "everything fused": r16((c + r) * s + b),
        "result flushed": fl(r16(r16(q * s) + b)),
        "sum flushed": r16(r16(fl(q) * s) + b),
        "product flushed": r16(fl(r16(q * s)) + b),
        "sum truncated": r16(r16(rtz(c + r) * s) + b),
        "product truncated": r16(rtz(q * s) + b),
        "bias add truncated": rtz(r16(q * s) + b),
    }


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_finite_table_is_finite_and_reaches_its_classes(dt):
    L = sp.special_layer(dt, finite=True)
    for part in sp.finite_tables(dt):
        assert np.isfinite(np.array(part, dtype=np.float64)).all()
    idx, ridx = vo.unpack_indices(L.indices, L.index_bits, L.group_size, L.res_bits, False)
    sb = np.arange(L.in_features) // sp.COLS_PER_SB
    assert len({(int(c), int(r), int(p)) for n in range(sp.ROWS) for c, r, p in zip(idx[0, n], ridx[0, n], sb)}) == 16 * 16 * 64
    W = vo.dequant(L, ref_residual_mask_quirk=False)
    assert sp.coverage(L) == FINITE_COVERAGE[dt]
    assert W.size == FINITE_COVERAGE[dt]["finite"], "a weight of the finite table is not finite"
    sp.same_bits(W, torch_dequant(L), dt, "oracle against torch")
    # the float64 restatement the mutants are variations of is the oracle
    c, r, s, b = sp.operands(L)
    want = vo.to_f32(W, dt).astype(np.float64)
    assert np.array_equal(_r16(_r16(_r16(c + r, dt) * s, dt) + b, dt), want)
    f = sp.FMT[dt]
    cent, res, scale, bias = sp.finite_tables(dt)
    r16 = lambda x: float(_r16(np.array([x]), dt)[0])   # noqa: E731
    one, nxt = 1.0, 1.0 + f["eps"]
    assert r16(one + f["eps"] / 2) == one and r16(nxt + f["eps"] / 2) == nxt + f["eps"]          # behind the sum and the bias add
    assert r16(one + 3 * f["eps"] / 2) == nxt + f["eps"] and r16(one - f["eps"] / 4) == one
    assert r16(nxt * 1.5) == 1.5 + 2 * f["eps"] and r16(3 * f["sub"] * 0.5) == 2 * f["sub"] and r16(f["sub"] * 0.5) == 0.0   # the product
    for need, have in ((one, cent), (nxt, cent), (f["eps"] / 2, res[0]), (3 * f["eps"] / 2, res[0]), (-f["eps"] / 4, res[0]), (3 * f["sub"], cent),
                       (f["sub"], cent), (f["norm"], cent), (f["norm"] - f["sub"], cent), (0.5, scale), (1.5, scale), (f["norm"], scale),
                       (f["eps"] / 2, bias)):
        assert need in have
    # what a bf16 route may read as a zero stays a small share of the table
    W0 = vo.dequant(sp.special_layer(dt, k=65536, kr=0, finite=True), ref_residual_mask_quirk=False)   # (no residual codebook: more of them)
    shares = dict(subnormal=float(sp.subnormal_mask(W, dt).mean()), below_2_21=float(sp.tiny_mask(W, dt, 2.0 ** -21).mean()),
                  subnormal_kr0=float(sp.subnormal_mask(W0, dt).mean()), below_2_21_kr0=float(sp.tiny_mask(W0, dt, 2.0 ** -21).mean()))
    print(dt, shares)
    assert all(0 < v < SHARE_LIMIT for v in shares.values()), shares


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_finite_table_tells_every_mutant_from_the_reference(dt):
    L = sp.special_layer(dt, finite=True)
    want = vo.to_f32(vo.dequant(L, ref_residual_mask_quirk=False), dt).astype(np.float64)
    counts = {name: int((W != want).sum()) for name, W in mutants(L).items()}   # (float compare: -0 == +0, nothing is NaN)
    print(dt, counts)
    assert all(n >= MIN_DIFFERENT for n in counts.values()), counts


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("v,k,kr,cols,perm", [(8, 256, 256, 11008, 0), (8, 65536, 0, 4096, 1), (16, 65536, 256, 1856 + 64, 1)])
def test_finite_table_in_other_formats_and_widths(v, k, kr, cols, perm, dt):
    """cols repeats the pattern, a permutation keeps each stored column's (scale, bias) pair: the same weights, in another order"""
    L = sp.special_layer(dt, v, k, kr, finite=True, cols=cols, perm=bool(perm))
    W = vo.dequant(L, ref_residual_mask_quirk=False)
    assert W.shape == (sp.ROWS * v, cols) and (W & 0x7fff).max() < 0x7c00
    if not perm:   # (oracle/torch_ref.py restates the reference without its permutation)
        sp.same_bits(W, torch_dequant(L), dt, "oracle against torch")
    assert c_oracle.available(), "the C oracle is built when the session starts (tests/conftest.py)"
    sp.same_bits(c_oracle.dequant(L, quirk=False), W, dt, "C oracle against the oracle")
    stored = W if not perm else W[:, L.perm.astype(np.int64)]     # stored column c is W's column perm[c]
    base = vo.dequant(sp.special_layer(dt, v, k, kr, finite=True), ref_residual_mask_quirk=False)
    assert np.array_equal(stored, np.tile(base, (1, -(-cols // sp.width())))[:, :cols])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_overflow_layer_has_finite_parameters_and_planted_infinities(dt):
    L, planted = sp.overflow_layer(dt)
    for t in (L.centroids, L.res_centroids, L.weight_scale, L.weight_bias):
        assert np.isfinite(vo.to_f32(t, dt)).all()
    assert sp.coverage(L) == OVERFLOW_COVERAGE[dt]
    sp.same_bits(vo.dequant(L, ref_residual_mask_quirk=False), torch_dequant(L), dt, "oracle against torch")
    W = vo.to_f32(vo.dequant(L, ref_residual_mask_quirk=False), dt).reshape(sp.OVERFLOW_ROWS, L.vector_len, -1)
    assert np.isfinite(W[0]).all() and np.isfinite(W[4:]).all(), "vector-rows 0 and 4 - 8 are free of overflows"
    inf = np.zeros(W.shape, bool)
    for row, col, sign in planted:
        assert (W[row, :, col] == sign * np.inf).all()
        inf[row, :, col] = True
    assert np.array_equal(np.isinf(W), inf), "an overflow that was not planted"
    signs = [{s for r, _, s in planted if r == row} for row in range(sp.OVERFLOW_ROWS)]
    assert signs[1] == {1, -1} and signs[2] == {1} and signs[3] == {1, -1} and all(not s for s in signs[:1] + signs[4:])
    # the variants: one more infinity in the last chunk of 8 columns; entries 0 that would overflow together and that nothing reads
    Lt, planted_t = sp.overflow_layer(dt, tail=True)
    assert [p for p in planted_t if p not in planted] == [(2, L.in_features - 2, 1)]
    L0, _ = sp.overflow_layer(dt, entry0=True)
    assert np.array_equal(vo.dequant(L0, ref_residual_mask_quirk=False), vo.dequant(L, ref_residual_mask_quirk=False))
    idx0, ridx0 = vo.unpack_indices(L0.indices, L0.index_bits, L0.group_size, L0.res_bits, False)
    assert idx0.min() > 0 and ridx0.min() > 0
    for kw in (dict(kr=0, k=65536), dict(v=16, k=65536, kr=65536, perm=True)):
        L2, planted2 = sp.overflow_layer(dt, **kw)
        W2 = vo.to_f32(vo.dequant(L2, ref_residual_mask_quirk=False), dt)
        assert np.isinf(W2).sum() == len(planted2) * L2.vector_len and np.isfinite(W2[:L2.vector_len]).all()
