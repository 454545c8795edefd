"""The special-value layers of the dequant tests: codebooks, scale and bias written by hand instead of drawn - signed zeros,
subnormals, the smallest normal, the largest finite value, infinities, a NaN, sums and products that land exactly on a rounding
tie (both parities), that overflow, and that underflow into the subnormal range - and indices laid out so that every pair
(centroid, residual centroid) of the table meets every pair (scale, bias) of the table at least once.

special_layer() builds the oracle LayerSpec; tests/test_dequant_specials_cpu.py pins what the oracle makes of it against torch's own
CPU arithmetic, the GPU tests (test_dequant_models_gpu.py, test_dequant_sliced_gpu.py) hold the kernels to it with same_bits().

For the GEMV kernels, which can only be asked for a weight through a sum: finite_tables() / special_layer(finite=True) - the same
classes without anything that is or becomes infinite or NaN, at any width (cols=) and with a permutation - and overflow_layer(),
whose finite parameters overflow in a few planted weights (tests/test_weight_bits_gpu.py)."""
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


def finite_tables(dt):
    """tables() without an infinity, a NaN or anything that overflows: every weight r16(r16(r16(c + r) s) + b) of the 16 x 32 x 8 x 8
    combinations is finite, so that a GEMV can read the weights one by one (a one-hot activation times a non-finite weight of the
    same row would spoil the read).  Kept: signed zeros, subnormals, the smallest normal and its neighbours, ties behind the sum,
    the product and the bias add in both parities, products that underflow into the subnormal range and to zero, and ordinary
    values whose sums and products are inexact (what tells round-to-nearest from truncation)."""
    f = FMT[dt]
    eps, sub, norm = f["eps"], f["sub"], f["norm"]
    g = lambda x: float(vo.round_to(np.array([x], np.float32), dt)[0])   # noqa: E731  (an ordinary value on the grid)
    cent = [0.0, -0.0, sub, norm - sub, norm, norm + sub,
            3 * sub,                 # x 0.5: the tie 1.5 sub -> 2 sub;   sub x 0.5: the tie 0.5 sub -> 0
            1.0, 1.0 + eps,          # + eps / 2, + 3 eps / 2: ties, to even downwards and upwards
            -1.0, 0.375, g(0.3379), g(-1.7113), g(2.6181), g(-0.0418), g(0.0917)]
    res0 = [0.0, -0.0, sub, -sub, norm - sub, -norm,
            eps / 2, 3 * eps / 2,    # the ties with 1 and 1 + eps
            -eps / 4,                # 1 - eps / 4: the tie below 1, where the grid is twice as fine
            g(0.0123), g(-0.7071), g(0.2113), g(-0.0061), g(1.3371), 0.5, -1.0]
    res1 = [1.0, -1.0, eps, -3 * eps / 2, 2 * sub, 5 * sub, -(norm - sub), norm / 2, 3.0, -3.0,
            g(1.2345), g(-0.0813), g(0.0049), -0.375, 2.0 ** -5, g(-0.5577)]
    scale = [1.0, -1.0, 0.5,         # 0.5: products that underflow into the subnormal range, ties among them
             1.5,                    # (1 + eps) x 1.5 = 1.5 + 1.5 eps: a product on a tie
             norm,                   # products that underflow to zero or the smallest subnormals
             g(0.7313), g(-1.2871), g(0.1563)]
    bias = [0.0, -0.0, eps / 2,      # 1 + eps / 2, (1 + eps) + eps / 2: ties behind the product
            -3 * sub,                # sums within the subnormal range
            -1.0,                    # cancellation: 1 x 1 - 1, (1 + eps) - 1
            g(0.0391), g(-0.2719), g(1.0623)]
    assert len(cent) == len(res0) == len(res1) == N_SPECIAL and len(scale) == len(bias) == 8
    return cent, [res0, res1], scale, bias


def width():
    return 8 * 8 * COLS_PER_SB   # every (scale, bias) pair of 8 x 8


def special_layer(dt, v=8, k=16, kr=16, seed=5, finite=False, cols=None, perm=False):
    """the LayerSpec: `width()` columns, ROWS vector-rows, one codebook group.  k / kr beyond 16 entries: the special entries sit
    k / 16 (kr / 16) apart - spread over the whole index range - between ordinary values, and every index element points at a
    special entry.  kr = 0: no residual codebook (the centroid meets every (scale, bias) pair).
    finite: finite_tables() instead of tables().  cols: that many columns, the pattern of `width()` columns repeated (and cut).
    perm: with an input permutation; scale and bias follow it, so that a stored column keeps its (scale, bias) pair."""
    cent, res, scale, bias = finite_tables(dt) if finite else tables(dt)
    rng = np.random.default_rng(seed)
    I, O = cols or width(), ROWS * v
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
    j = np.arange(I) % width()
    pair = ((j % COLS_PER_SB)[None, :] * ROWS + np.arange(ROWS)[:, None]) % (N_SPECIAL * N_SPECIAL)      # [ROWS, I]
    ci, ri = pair // N_SPECIAL, pair % N_SPECIAL
    idx = (ci * (k // N_SPECIAL))[None]
    ridx = (ri * (kr // N_SPECIAL))[None] if kr else None
    L.indices = vo.pack_indices(idx, L.index_bits, ridx, L.res_bits)
    sb = j // COLS_PER_SB
    if perm:   # (W's column i is stored column argsort(perm)[i]: vo.dequant)
        L.perm = rng.permutation(I).astype(np.uint16)
        sb = sb[np.argsort(L.perm.astype(np.int64), kind="stable")]
    L.weight_scale = _bits([scale[p // 8] for p in sb], dt)
    L.weight_bias = _bits([bias[p % 8] for p in sb], dt)
    return L


OVERFLOW_ROWS = ROWS      # vector-rows of overflow_layer: rows 1 - 3 hold the overflows, the others are free of them


def overflow_layer(dt, v=8, k=256, kr=256, cols=256, seed=9, perm=False, tail=False, entry0=False):
    """a small layer whose codebooks, scale and bias are finite and ordinary but for a few entries - big, -big, root, -root among the
    centroids, half an ulp of big and its negative among the residual centroids, root among the scales - that meet in a few planted
    places: big + half_ulp_big (a sum that rounds to +inf), its negative, root x root (a product that overflows) and -root x root.
    Vector-rows 0 and 4 - 8 draw ordinary entries only: none of their weights overflows.  Vector-row 1 holds +inf and -inf (sum and product),
    row 2 +inf only, row 3 -inf and +inf from the product alone.  kr = 0: the product cases only.
    Where the overflows are NOT: entry 0 of either codebook (the sliced layouts' padding elements rebuild entry 0 of a slice and
    residual entry 0 against a scale of zero) and the last 8 columns (the tail lanes of gemv_k256 / gemv_gather read the last chunk
    again against zero activations) - 0 x inf is NaN, in a kernel's padding as for a zero activation in the reference; vptq_hip.h
    states both beside VPTQ_GEMV_EXACT.  The two variants that pin those statements (tests/test_weight_bits_gpu.py): tail = one more
    big + half_ulp_big in vector-row 2 at the last column but one; entry0 = big as entry 0 of the main codebook and half_ulp_big
    as entry 0 of the residual one, which no index of the layer points at (W is what it is without them).
    -> (LayerSpec, planted): planted = [(vector-row, stored column, sign)]."""
    assert k >= 32 and (kr == 0 or kr >= 32)
    f = FMT[dt]
    rng = np.random.default_rng(seed)
    I, O = cols, OVERFLOW_ROWS * v
    L = vo.LayerSpec(I, O, v, k, kr, 1, I, 0, -1, -1, dt)
    cstep, rstep = k // N_SPECIAL, max(kr // N_SPECIAL, 1)

    def table(n, step, specials):   # special entry i at i x step + 1 (entry 0 stays ordinary: the sliced layouts' padding reads it)
        t = vo.from_f32((rng.standard_normal((n, v)) * 0.02).astype(np.float32), dt)
        for i, val in enumerate(specials):
            t[i * step + 1] = _bits([val] * v, dt)
        return t.reshape(1, n, v)

    L.centroids = table(k, cstep, [f["big"], -f["big"], f["root"], -f["root"]])
    if kr:
        L.res_centroids = table(kr, rstep, [f["half_ulp_big"], -f["half_ulp_big"], 0.0])

    def ordinary(n, step, count):   # never a special entry
        i = rng.integers(0, n, size=(OVERFLOW_ROWS, I))
        special = (i % step == 1 % step) & (i // step < count)
        i = np.where(special, (i + 1) % n if step > 2 else (count * step + 1 + i % (n - count * step - 1)), i)
        return np.where(i == 0, 2, i)   # (nor entry 0)

    idx = ordinary(k, cstep, 4)
    ridx = ordinary(kr, rstep, 3) if kr else None
    scale = np.abs(rng.standard_normal(I)) * 0.5 + 0.75
    hot = [I // 5, (3 * I) // 5]                  # the two columns whose scale is root
    scale[hot] = f["root"]
    planted = []

    def plant(row, col, c, r, sign):
        idx[row, col] = c * cstep + 1
        if kr:
            ridx[row, col] = r * rstep + 1
        planted.append((row, col, sign))

    if kr:
        plant(1, 3, 0, 0, +1)                     # big + half_ulp_big
        plant(1, I - 12, 1, 1, -1)                # -big - half_ulp_big (not in the last chunk of 8: see above)
        plant(2, I // 2 + 1, 0, 0, +1)
        if tail:
            plant(2, I - 2, 0, 0, +1)
    plant(1, hot[0], 2, 2, +1)                    # root x root
    plant(1, hot[1], 3, 2, -1)                    # -root x root
    plant(2, hot[0], 2, 2, +1)
    plant(3, hot[0], 3, 2, -1)
    plant(3, hot[1], 2, 2, +1)
    if entry0:
        L.centroids[0, 0], L.res_centroids[0, 0] = _bits([f["big"]] * v, dt), _bits([f["half_ulp_big"]] * v, dt)
    L.indices = vo.pack_indices(idx[None], L.index_bits, ridx[None] if kr else None, L.res_bits)
    bias = rng.standard_normal(I) * 0.01
    if perm:
        L.perm = rng.permutation(I).astype(np.uint16)
        order = np.argsort(L.perm.astype(np.int64), kind="stable")
        scale, bias = scale[order], bias[order]
    L.weight_scale, L.weight_bias = _bits(scale, dt), _bits(bias, dt)
    return L, planted


def operands(L):
    """-> (c, r, s, b) of every weight of a one-group layer without permutation and outliers, float64 [O, I] (r = None without a
    residual codebook): what the mutants of test_dequant_specials_cpu.py are computed from"""
    assert L.perm is None and not L.enable_outlier and L.num_codebooks == 1
    dt, v, N, G = L.dtype, L.vector_len, L.num_indices, L.group_size
    idx, ridx = vo.unpack_indices(L.indices, L.index_bits, G, L.res_bits, False)

    def gather(table, ix):   # [n, v], [N, G] -> [N v, G]
        return vo.to_f32(table, dt).reshape(-1, v)[ix].transpose(0, 2, 1).reshape(N * v, G).astype(np.float64)[:L.out_features]

    c = gather(L.centroids, idx[0])
    r = gather(L.res_centroids, ridx[0]) if L.num_res_centroids > 0 else None
    s = np.broadcast_to(vo.to_f32(L.weight_scale, dt).astype(np.float64)[None, :], c.shape)
    b = np.broadcast_to(vo.to_f32(L.weight_bias, dt).astype(np.float64)[None, :], c.shape)
    return c, r, s, b


def subnormal_mask(W, dt):
    """the elements of W (bits) in the format's subnormal range (zeros are not)"""
    mag = np.ascontiguousarray(W).view(np.uint16) & 0x7fff
    return ((mag & (0x7c00 if dt == "f16" else 0x7f80)) == 0) & (mag != 0)


def tiny_mask(W, dt, below):
    """the non-zero elements of W (bits) smaller than `below` in magnitude"""
    a = np.abs(vo.to_f32(W, dt).astype(np.float64))
    return (a > 0) & (a < below)


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
