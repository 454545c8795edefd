"""Per-output float64 models of the arithmetics the GEMV kernels implement, and one checker that holds EVERY output to them.

The parity metric of the older tests, max|d| / max|ref| against the reference's rounding, lets a kernel drop a column, read the
wrong token for a block or write one small wrong output unnoticed.  Here each kernel is compared with a model of ITS OWN
arithmetic, output by output:

  exact      w = the reference's bits (vptq_dequant / vo.dequant), m = sum_j w_j x_j + bias
  folded     m = sum_j (c + r)_j r16(s_j x_j) + sum_j b_j x_j + bias      (c + r exact: separate products of c and r)
             m = sum_j r16(c + r)_j r16(s_j x_j) + ...                      (rounded=True: c + r rounded to 16 bits first)
  selective  exact on the given blocks of 128 columns, folded elsewhere.  The blocks are blocks of the STORED column order
             (column c of the quantised matrix multiplies input feature perm[c]; without a permutation the two orders are
             one): the kernels stage x[perm] and find the hot blocks there.  hot_cols = the same as a mask over the input
             features (hot_mask_for)
  cols       a column range [c0, c1) of any of them (row-parallel shards, column parts); the output bias only where asked

and with every model the magnitude a = sum_j |term_j| + |bias| that bounds an fp32 summation's error in any order:

  fp32 outputs    |y - m| <= 2^-20 a + extra_abs
  16-bit outputs  |y - m| <= ulp(m) + 2^-20 a + extra_abs;  m beyond the type's range: an inf of m's sign
  no NaN unless allowed.

extra_abs covers fixed-point accumulation (the sliced kernels' accumulator words: arrivals x 2^-F truncation).
Everything is numpy float64 on the CPU; the GPU tests hand over the kernel's output."""
import numpy as np

from oracle import vptq_oracle as vo

BLOCK = 128          # the selective arithmetic's block of input columns
REL = 2.0 ** -20     # fp32 summation allowance relative to sum |terms|
FIX_F = {"f16": 30, "bf16": 28}   # fraction bits of the sliced kernels' accumulator words
# smallest magnitude that rounds to inf (max + half an ulp of the top binade)
OVER16 = {"f16": 65520.0, "bf16": float(2.0 ** 128 - 2.0 ** 103)}


def sliced_extra_abs(dtype, arrivals):
    """truncation of the sliced kernels' fixed-point accumulator: one unit of 2^-F per arrival"""
    return arrivals * 2.0 ** -FIX_F[dtype]


def ulp16(m, dtype):
    """spacing of the 16-bit grid at |m| (subnormal spacing below the normal range)"""
    m = np.abs(np.asarray(m, dtype=np.float64))
    mant, emin = (10, -14) if dtype == "f16" else (7, -126)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(m > 0, m, 1.0)))
    e = np.maximum(e, emin)
    return np.ldexp(1.0, (e - mant).astype(np.int64))


# ---------------------------------------------------------------------------------------------- the layer's pieces
def pieces(L):
    """-> dict of float64 arrays in INPUT-FEATURE column order (the order x is indexed in):
    c [O, I] main (or outlier) entries, r [O, I] residual entries (0 where none), s [I], b [I] (1 / 0 without norm),
    bias [O] (0 without), W [O, I] the reference's bits (exact)."""
    dt = L.dtype
    C, G, v, N = L.num_codebooks, L.group_size, L.vector_len, L.num_indices
    O = L.out_features
    idx, ridx = vo.unpack_indices(L.indices, L.index_bits, G, L.res_bits, False)
    cent = vo.to_f32(L.centroids, dt).reshape(C, L.num_centroids, v).astype(np.float64)
    cb = np.arange(C)[:, None, None]
    c = cent[cb, idx].transpose(1, 3, 0, 2).reshape(N * v, C * G)[:O]
    if L.num_res_centroids > 0:
        rc = vo.to_f32(L.res_centroids, dt).reshape(C, L.num_res_centroids, v).astype(np.float64)
        r = rc[cb, ridx].transpose(1, 3, 0, 2).reshape(N * v, C * G)[:O]
    else:
        r = np.zeros_like(c)
    if L.enable_outlier:
        ov, S = L.outlier_vector_len, L.outlier_size
        oc = vo.to_f32(L.outlier_centroids, dt).reshape(L.num_outlier_centroids, ov).astype(np.float64)
        oi = np.ascontiguousarray(L.outlier_indices).view(np.uint16).reshape(-1, S).astype(np.int64)
        qo = oc[oi].transpose(0, 2, 1).reshape(-1, S)[:O]
        c = np.concatenate([qo, c], axis=1)
        r = np.concatenate([np.zeros_like(qo), r], axis=1)
    if L.perm is not None:
        inv = np.argsort(np.ascontiguousarray(L.perm).view(np.uint16).astype(np.int64), kind="stable")
        c, r = c[:, inv], r[:, inv]
    I = L.in_features
    if L.weight_scale is not None:
        s = vo.to_f32(L.weight_scale, dt).astype(np.float64)
        b = vo.to_f32(L.weight_bias, dt).astype(np.float64)
    else:
        s, b = np.ones(I), np.zeros(I)
    bias = vo.to_f32(L.bias, dt).astype(np.float64) if L.bias is not None else np.zeros(O)
    W = vo.to_f32(vo.dequant(L, ref_residual_mask_quirk=False), dt).astype(np.float64)
    return dict(c=c, r=r, s=s, b=b, bias=bias, W=W, dtype=dt, norm=L.weight_scale is not None)


def pieces_v2(dtype, I, O, v, indices, centroids, res_indices=None, res_centroids=None, scale=None, sbias=None, bias=None):
    """the same dict as pieces(L) from the tensors of the v2 wire format (ids [N * I], one codebook, uint16 bit patterns; there is
    no permutation): W by vo.dequant_v2, so model() / check_outputs() take the v2 rows unchanged"""
    N = O // v
    ids = np.asarray(indices).reshape(N, I).astype(np.int64)
    cent = vo.to_f32(np.asarray(centroids), dtype).reshape(-1, v).astype(np.float64)
    c = cent[ids].transpose(0, 2, 1).reshape(N * v, I)
    if res_indices is not None:
        rc = vo.to_f32(np.asarray(res_centroids), dtype).reshape(-1, v).astype(np.float64)
        r = rc[np.asarray(res_indices).reshape(N, I).astype(np.int64)].transpose(0, 2, 1).reshape(N * v, I)
    else:
        r = np.zeros_like(c)
    s = vo.to_f32(np.asarray(scale), dtype).reshape(I).astype(np.float64) if scale is not None else np.ones(I)
    b = vo.to_f32(np.asarray(sbias), dtype).reshape(I).astype(np.float64) if sbias is not None else np.zeros(I)
    bb = vo.to_f32(np.asarray(bias), dtype).reshape(O).astype(np.float64) if bias is not None else np.zeros(O)
    W = vo.dequant_v2(indices, centroids, res_indices, res_centroids, scale, sbias, I, O, v, dtype).astype(np.float64).T
    return dict(c=c, r=r, s=s, b=b, bias=bb, W=np.ascontiguousarray(W), dtype=dtype, norm=scale is not None)


MAX_WEIGHTS = 16 << 20   # float64 weights one step of a blocked model holds (the size limit of the route tables' cases)


def row_blocks(L, max_weights=MAX_WEIGHTS):
    """-> [(n0, n1)]: ranges of vector-rows of at most max_weights weights each (at least one vector-row)"""
    rows = max(1, max_weights // (L.vector_len * L.in_features))
    return [(n0, min(n0 + rows, L.num_indices)) for n0 in range(0, L.num_indices, rows)]


def slice_rows(L, n0, n1):
    """the layer of the vector-rows [n0, n1) of L: the index rows, the outlier index rows and the output bias sliced; codebooks,
    scale, bias and permutation shared"""
    import dataclasses
    v, O = L.vector_len, L.out_features
    o0, o1 = n0 * v, min(n1 * v, O)
    S = dataclasses.replace(L, out_features=o1 - o0, indices=np.ascontiguousarray(np.asarray(L.indices)[:, n0:n1]))
    if L.enable_outlier:
        ov = L.outlier_vector_len
        assert o0 % ov == 0, "a row block must start on an outlier vector"
        oi = np.ascontiguousarray(L.outlier_indices).view(np.uint16).reshape(1, -1, L.outlier_size)
        S.outlier_indices = np.ascontiguousarray(oi[:, o0 // ov:(o1 + ov - 1) // ov])
    if L.bias is not None:
        S.bias = np.ascontiguousarray(np.asarray(L.bias).reshape(-1)[o0:o1])
    return S


def pieces_blocks(L, max_weights=MAX_WEIGHTS):
    """the row-block form of pieces(L): yields ((n0, n1) vector-rows, (o0, o1) outputs, pieces of that slice of the layer), so that
    no step holds more than max_weights float64 weights per array"""
    for n0, n1 in row_blocks(L, max_weights):
        yield (n0, n1), (n0 * L.vector_len, min(n1 * L.vector_len, L.out_features)), pieces(slice_rows(L, n0, n1))


def model_blocks(L, x_bits, arith="exact", max_weights=MAX_WEIGHTS, **kw):
    """model() block by block: yields ((o0, o1), m, a) with m, a [tokens, o1 - o0]"""
    for _, orange, P in pieces_blocks(L, max_weights):
        m, a = model(P, x_bits, arith, **kw)
        yield orange, m, a


def _x64(x_bits, dtype, I):
    return vo.to_f32(np.asarray(x_bits), dtype).astype(np.float64).reshape(-1, I)


def _cols(I, cols):
    c0, c1 = (0, I) if cols is None else cols
    mask = np.zeros(I, bool)
    mask[c0:c1] = True
    return mask


def _hot_mask(I, hot_blocks):
    """hot_blocks: indices of blocks of 128 input columns (one set for every token)"""
    mk = np.zeros(I, bool)
    for k in hot_blocks:
        mk[k * BLOCK:(k + 1) * BLOCK] = True
    return mk


def hot_mask_for(I, hot_blocks, perm=None):
    """mask over the INPUT FEATURES of the blocks of 128 STORED columns `hot_blocks`: feature perm[c] for every stored column c of
    a hot block (perm: the layer's uint16 permutation, None: stored order = input-feature order)"""
    stored = _hot_mask(I, hot_blocks)
    if perm is None:
        return stored
    mk = np.zeros(I, bool)
    mk[np.ascontiguousarray(perm).view(np.uint16).astype(np.int64)[stored]] = True
    return mk


def model(P, x_bits, arith="exact", *, rounded=False, round_sx=True, hot_blocks=(), hot_cols=None, cols=None, with_bias=True):
    """-> (m, a), float64 [tokens, O].  P = pieces(L).
    arith: "exact" | "folded" | "selective" (exact on hot_blocks - or on the input features hot_cols, a mask: a permuted layer's
    blocks are blocks of its stored column order, hot_mask_for - folded elsewhere).  rounded: the folded form with r16(c + r);
    round_sx=False: the folded form with s x unrounded.  cols: [c0, c1) of the input columns (shards, column parts);
    with_bias: add the output bias (rank 0 of a row-parallel shard only)."""
    dt = P["dtype"]
    I = P["W"].shape[1]
    x = _x64(x_bits, dt, I)
    inside = _cols(I, cols)
    if arith == "exact":
        ex_cols, fo_cols = inside, np.zeros(I, bool)
    elif arith == "folded":
        ex_cols, fo_cols = np.zeros(I, bool), inside
    elif arith == "selective":
        hot = _hot_mask(I, hot_blocks) if hot_cols is None else np.asarray(hot_cols, bool)
        ex_cols, fo_cols = inside & hot, inside & ~hot
    else:
        raise ValueError(arith)
    m = np.zeros((x.shape[0], P["W"].shape[0]))
    a = np.zeros_like(m)
    if ex_cols.any():
        W, xe = P["W"][:, ex_cols], x[:, ex_cols]
        m += xe @ W.T
        a += np.abs(xe) @ np.abs(W).T
    if fo_cols.any():
        cr = P["c"][:, fo_cols] + P["r"][:, fo_cols]
        if rounded:
            cr = vo.round_to(cr.astype(np.float32), dt).astype(np.float64)
        sx = P["s"][fo_cols] * x[:, fo_cols]
        if round_sx:
            sx = vo.round_to(sx.astype(np.float32), dt).astype(np.float64)
        bx = x[:, fo_cols] * P["b"][fo_cols]
        m += sx @ cr.T + bx.sum(axis=1, keepdims=True)
        a += np.abs(sx) @ np.abs(cr).T + np.abs(bx).sum(axis=1, keepdims=True)
    if with_bias:
        m += P["bias"][None, :]
        a += np.abs(P["bias"])[None, :]
    return m, a


# ---------------------------------------------------------------------------------------------- the checker
def violations(got, m, a, dtype, out_f32, extra_abs=0.0, allow_nan=False):
    """-> (bad mask, bound, excess) for every output; see check_outputs"""
    y = np.asarray(got, dtype=np.float64).reshape(np.shape(m))
    m = np.asarray(m, dtype=np.float64)
    bound = REL * np.asarray(a, dtype=np.float64) + extra_abs
    if not out_f32:
        bound = bound + ulp16(m, dtype)
    nan = np.isnan(y)
    with np.errstate(invalid="ignore"):
        err = np.abs(y - m)
    bad = ~nan & ~(err <= bound)
    if not out_f32:
        # beyond the 16-bit range: an inf of m's sign; near the edge either that or a finite value within the bound
        over = np.abs(m) - bound >= OVER16[dtype]
        edge = ~over & (np.abs(m) + bound >= OVER16[dtype])
        right_inf = np.isinf(y) & (np.sign(y) == np.sign(m))
        bad = np.where(over, ~right_inf & ~nan, np.where(edge, ~(right_inf | (err <= bound)) & ~nan, bad))
    if not allow_nan:
        bad = bad | nan
    excess = np.where(nan, np.inf, np.nan_to_num(err - bound, nan=np.inf, posinf=np.inf))
    return bad, bound, excess


def check_outputs(got, m, a, dtype, out_f32, extra_abs=0.0, allow_nan=False, what=""):
    """assert every output of `got` meets the model (m, a); on failure report how many do not and the worst one"""
    bad, bound, excess = violations(got, m, a, dtype, out_f32, extra_abs, allow_nan)
    if bad.any():
        y = np.asarray(got, dtype=np.float64).reshape(np.shape(m))
        ex = np.where(bad, excess, -np.inf)
        i = np.unravel_index(int(np.argmax(ex)), ex.shape)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} outputs off the model ({'fp32' if out_f32 else dtype}); worst at {tuple(int(k) for k in i)}:"
            f" got {y[i]!r}, model {float(np.asarray(m)[i])!r}, |d| {abs(y[i] - float(np.asarray(m)[i])):.3e} > bound {float(bound[i]):.3e}")


def check_both(y16, y32, m, a, dtype, extra_abs=0.0, what=""):
    """a route's 16-bit output and its VPTQ_GEMV_OUT_F32 output against one model"""
    check_outputs(y16, m, a, dtype, False, extra_abs, what=what + " [16-bit]")
    check_outputs(y32, m, a, dtype, True, extra_abs, what=what + " [fp32]")
