"""The special-value layers of the dequant tests: codebooks, scale and bias written by hand instead of drawn - signed zeros,
subnormals, the smallest normal, the largest finite value, infinities, a NaN, sums and products that land exactly on a rounding
tie (both parities), that overflow, and that underflow into the subnormal range - and indices laid out so that every pair
(centroid, residual centroid) of the table meets every pair (scale, bias) of the table at least once.

special_layer() builds the oracle LayerSpec; tests/test_dequant_specials_cpu.py pins what the oracle makes of it against torch's own
CPU arithmetic, the GPU tests (test_dequant_models_gpu.py, test_dequant_sliced_gpu.py) hold the kernels to it with same_bits()."""
import numpy as np

from oracle import vptq_oracle as vo

# per dtype: ulp of 1, smallest subnormal, smallest normal, largest finite, half an ulp of the largest finite, a value whose square overflows
FMT = {
    "f16": dict(eps=2.0 ** -10, sub=2.0 ** -24, norm=2.0 ** -14, big=65504.0, half_ulp_big=16.0, root=256.0),
    "bf16": dict(eps=2.0 ** -7, sub=2.0 ** -133, norm=2.0 ** -126, big=float(np.float32(2.0 ** 127 * (2 - 2.0 ** -7))), half_ulp_big=2.0 ** 119,
                 root=2.0 ** 64),
}
N_SPECIAL = 16            # special entries per codebook
ROWS = 9                  # vector-rows of a special layer (out_features = ROWS x v)
COLS_PER_SB = 29          # columns per (scale, bias) pair: 29 x 9 = 261 >= 256 (centroid, residual) pairs


def _bits(values, dt):
    with np.errstate(over="ignore", invalid="ignore"):
        return vo.from_f32(np.array(values, dtype=np.float64).astype(np.float32), dt)


def tables(dt):
    """-> (cent [16], res [2][16], scale [8], bias [8]) as floats.  A centroid vector carries its value in every element; a residual
    vector carries res[0] in its even and res[1] in its odd elements: 16 x 32 (centroid, residual) value pairs."""
    f = FMT[dt]
    eps, sub, norm, big, hub, root = f["eps"], f["sub"], f["norm"], f["big"], f["half_ulp_big"], f["root"]
    inf, nan = float("inf"), float("nan")
    cent = [0.0, -0.0, sub, norm - sub, norm, big, -big, inf, -inf, nan,
            1.0, 1.0 + eps,          # + eps / 2, + 3 eps / 2: ties, to even downwards and upwards
            root,                    # root x root overflows; root + root does not
            3 * sub,                 # x 0.5: the tie 1.5 sub -> 2 sub;   sub x 0.5: the tie 0.5 sub -> 0
            -1.0, 0.375]
    res0 = [0.0, -0.0, sub, -sub, norm - sub, norm, -norm, big, -big, inf, -inf, nan,
            eps / 2, 3 * eps / 2,    # the ties with 1 and 1 + eps
            hub,                     # big + half an ulp of big: the tie between big (odd) and the overflow
            -hub]
    res1 = [1.0, -1.0, -eps / 2, eps, 2 * sub, 5 * sub, -(norm - sub), norm / 2, root, -root, big / 2, -big / 2,
            0.5, -0.375, 2.0 ** -5, -3.0]
    scale = [1.0, -1.0, 0.5,         # 0.5: products that underflow into the subnormal range, ties among them
             1.5,                    # (1 + eps) x 1.5 = 1.5 + 1.5 eps: a product on a tie
             root,                   # products that overflow
             norm,                   # products that underflow to zero or the smallest subnormals
             0.0, inf]
    bias = [0.0, -0.0, eps / 2,      # 1 + eps / 2, (1 + eps) + eps / 2: ties behind the product
            big, -inf,               # inf + -inf: NaN behind the product
            nan, sub, -1.0]
    assert len(cent) == len(res0) == len(res1) == N_SPECIAL and len(scale) == len(bias) == 8
    return cent, [res0, res1], scale, bias


def width():
    return 8 * 8 * COLS_PER_SB   # every (scale, bias) pair of 8 x 8


def special_layer(dt, v=8, k=16, kr=16, seed=5):
    """the LayerSpec: `width()` columns, ROWS vector-rows, one codebook group.  k / kr beyond 16 entries: the special entries sit
    k / 16 (kr / 16) apart - spread over the whole index range - between ordinary values, and every index element points at a
    special entry.  kr = 0: no residual codebook (the centroid meets every (scale, bias) pair)."""
    cent, res, scale, bias = tables(dt)
    rng = np.random.default_rng(seed)
    I, O = width(), ROWS * v
    L = vo.LayerSpec(I, O, v, k, kr, 1, I, 0, -1, -1, dt)

    def table(n, vectors):
        t = vo.from_f32((rng.standard_normal((n, v)) * 0.02).astype(np.float32), dt)
        for i, vec in enumerate(vectors):
            t[i * (n // N_SPECIAL)] = vec
        return t.reshape(1, n, v)

    L.centroids = table(k, [_bits([c] * v, dt) for c in cent])
    if kr:
        L.res_centroids = table(kr, [_bits([res[t & 1][j] for t in range(v)], dt) for j in range(N_SPECIAL)])
    # column j carries (scale, bias) pair j // COLS_PER_SB; its ROWS elements the pairs (j % COLS_PER_SB) x ROWS + n, mod 256
    j = np.arange(I)
    pair = ((j % COLS_PER_SB)[None, :] * ROWS + np.arange(ROWS)[:, None]) % (N_SPECIAL * N_SPECIAL)      # [ROWS, I]
    ci, ri = pair // N_SPECIAL, pair % N_SPECIAL
    idx = (ci * (k // N_SPECIAL))[None]
    ridx = (ri * (kr // N_SPECIAL))[None] if kr else None
    L.indices = vo.pack_indices(idx, L.index_bits, ridx, L.res_bits)
    sb = j // COLS_PER_SB
    L.weight_scale = _bits([scale[p // 8] for p in sb], dt)
    L.weight_bias = _bits([bias[p % 8] for p in sb], dt)
    return L


def is_nan(bits, dt):
    b = np.ascontiguousarray(bits).view(np.uint16)
    return (b & 0x7fff) > (0x7c00 if dt == "f16" else 0x7f80)


def same_bits(got, want, dt, what=""):
    """NaN by position - the same elements are NaN on both sides, whatever their payload - everything else bit for bit, signed
    zeros and subnormals included"""
    got, want = np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(want).view(np.uint16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = is_nan(got, dt), is_nan(want, dt)
    bad = (gn != wn) | (~wn & (got != want))
    if bad.any():
        at = np.argwhere(bad)[:8]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, e.g. " +
                             ", ".join(f"[{r},{c}] got {got[r, c]:#06x} want {want[r, c]:#06x}" for r, c in at))


def coverage(L):
    """the classes the layer's dense W reaches, from the oracle's own result (a table that lost its edge cases fails its pin)"""
    W = vo.dequant(L, ref_residual_mask_quirk=False)
    dt = L.dtype
    mag = W & 0x7fff
    exp_mask, inf_bits = (0x7c00, 0x7c00) if dt == "f16" else (0x7f80, 0x7f80)
    return dict(nan=int(is_nan(W, dt).sum()), inf=int((mag == inf_bits).sum()), pos_zero=int((W == 0).sum()), neg_zero=int((W == 0x8000).sum()),
                subnormal=int(((mag & exp_mask) == 0).sum() - (mag == 0).sum()), finite=int((mag < inf_bits).sum()))
