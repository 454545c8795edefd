"""The batched-decode routes (5 - 64 tokens in ONE launch of a library entry): which (format, shape, token count) takes which entry.

Pure rules - no device, no tensors: the five route functions with their knobs and measured cells, one ordered table of what differs
between the routes (`BATCHED_DECODE_ROUTES`) and the two functions that read it, the static `batched_decode_routes` (per layer) and
the per-call `batched_decode_takes`.  `VQuantLinear.forward` and `ops.quant_gemm` both decide through them.  A new route is a
record in the table, a route function and a knob.  Behind the first table stands `BATCHED_DECODE_WIDE_ROUTES` (read by
`batched_decode_wide_routes`, walked after the first table's routes): a format's route beyond its first window - `gemm_gatherxw_route`,
17 - 48 tokens of gemm_gatherx's formats - and behind that `BATCHED_DECODE_V12_ROUTES` (`batched_decode_v12_routes`): `gemm_gather12_route`,
5 - 16 tokens of the vector-length-12 formats, which no record of the first two tables owns.  IN FRONT OF that third table a caller walks
`BATCHED_DECODE_V12_COLUMN_ROUTES` (`batched_decode_v12_column_routes`): `gemm_gather12c_route`, the column-parts form of the same
kernel for v = 12 layers with few outputs.  BEHIND all four stands `BATCHED_DECODE_V12_WIDE_ROUTES` (`batched_decode_v12_wide_routes`):
`gemm_gather12w_route`, 17 - 48 tokens of the v = 12 formats (token blocks over the column-parts walk), a window no other record has.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

from vptq_amd import _backend as B


# WHICH (format, shape, token count) take a batched-decode kernel of the large-codebook formats (1 - 16 tokens in one launch) in place
# of the route they had: the one rule, read by `VQuantLinear.forward` and `ops.quant_gemm`.
# A layer has ONE such kernel: v = 8, 65536 main centroids, 0 / 256 / 65536 residual centroids belong to `vptq_quant_gemm_gather`
# (gemm_gather.hip), every other vector length 8 / 16, 16384 ... 65536 main centroids, any residual codebook to
# `vptq_quant_gemm_gatherx` (gemm_gatherx.hip); `_batched_decode_entry` says which.  Each has a knob and a table of cells; a cell is
# (vector length, main centroids, residual centroids, least index elements = vector-rows x columns, least tokens).  A cell is routed
# only where the kernel was MEASURED to beat the route it replaces (5 - 8 tokens: the gemv_gather / gemv_gatherx launches; 9 - 16:
# the dense route) by more than the larger of 5 % and three times the run-to-run spread, both in one process on one box
# (tools/gemm_gather_bench.py writes the tables); a region is routed only where EVERY measured cell in it wins in both dtypes.
# VPTQ_GEMM_GATHER=1 / 0, VPTQ_GEMM_GATHERX=1 / 0 (with VPTQ_TUNING=1): every supported layer of that kernel from 5 tokens / none -
# what the bench tool, the tests and a user who has measured their own shapes use.
#
# gemm_gather (profiles/r15/table.md, profiles/r15/README.md: one MI355X, fp16 and bf16, 4096 x 4096 ... 8192 x 28672, tokens 5 / 8 /
# 9 / 12 / 16): from 9 tokens the kernel beats the dense route in every measured cell of the three formats (0.51 - 0.86 of its time),
# so 9 - 16 tokens are routed from the smallest measured layer (4096 x 4096 = 2 M index elements) up; at 5 - 8 tokens it is level
# with gemv_gather in most cells (0.84 - 1.12), which stays.
#
# gemm_gatherx (profiles/r16/table.md: one MI355X, 4096 x 4096 ... 8192 x 28672, tokens 5 / 8 / 9 / 12 / 16):
#   v16-k65536-0, v16-k65536-1024     every cell wins (0.48 - 0.93 of the parent's time): 5 - 16 tokens from 4096 x 4096 (1 M elements) up
#   v8-k32768-0, v8-k65536-4096       9 - 16 tokens: every cell (0.53 - 0.91); 5 - 8 tokens: only from 8192 x 8192 (8 M elements) up (0.73 - 0.94)
#   v16-k65536-65536                  wins at 5 - 8 tokens (0.66 - 0.88) but is level with the dense route at 9 - 16 on the larger
#                                     layers (0.94 - 1.05 at 8192 x 8192): a route has to be monotone in tokens, so nothing is routed
# Formats that were not measured (v16-k65536-32768 / -256 / -64, v8-k65536-4, v8-k16384-0) and smaller layers are not routed.
GEMM_GATHER_MAX_TOKENS = 16
_GEMM_GATHER_MODE = (B.tune_env("VPTQ_GEMM_GATHER", "auto") or "auto").strip().lower()
_GEMM_GATHER_CELLS = ((8, 65536, 0, 2 << 20, 9), (8, 65536, 256, 2 << 20, 9), (8, 65536, 65536, 2 << 20, 9))
_GEMM_GATHERX_MODE = (B.tune_env("VPTQ_GEMM_GATHERX", "auto") or "auto").strip().lower()
_GEMM_GATHERX_CELLS = (
    (16, 65536, 0, 1 << 20, 5), (16, 65536, 1024, 1 << 20, 5),
    (8, 32768, 0, 2 << 20, 9), (8, 32768, 0, 8 << 20, 5),
    (8, 65536, 4096, 2 << 20, 9), (8, 65536, 4096, 8 << 20, 5),
)


def _pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


def _batched_decode_entry(vector_len: int, num_centroids: int, num_res_centroids: int):
    """the library entry whose kernel has this format ("vptq_quant_gemm_gather" / "vptq_quant_gemm_gatherx"), or None"""
    if vector_len == 8 and num_centroids == 65536 and num_res_centroids in (0, 256, 65536):
        return "vptq_quant_gemm_gather"
    if vector_len in (8, 16) and _pow2(num_centroids) and 16384 <= num_centroids <= 65536 and \
            (not num_res_centroids or (_pow2(num_res_centroids) and num_res_centroids <= 65536)):
        return "vptq_quant_gemm_gatherx"
    return None


def _batched_decode_route(mode, cells, vector_len, num_centroids, num_res_centroids, out_features, in_features, tokens) -> bool:
    """the tail both route functions share: the knob, the token window, the measured cells"""
    if mode in ("0", "off") or not 5 <= tokens <= GEMM_GATHER_MAX_TOKENS:
        return False
    if mode in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any((v, k, kr) == (vector_len, num_centroids, num_res_centroids) and n_el >= min_el and tokens >= min_tok
               for v, k, kr, min_el, min_tok in cells)


def gemm_gather_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int) -> bool:
    """does a layer of this format (vector length, main / residual codebook entries) and shape take `vptq_quant_gemm_gather` for
    `tokens` tokens?  Pure: no device, no library (whether the library serves the layer - one codebook group, no outliers, scale and
    bias, alignment - is `vptq_quant_gemm_gather_supported`'s answer)."""
    return _batched_decode_entry(vector_len, num_centroids, num_res_centroids) == "vptq_quant_gemm_gather" and \
        _batched_decode_route(_GEMM_GATHER_MODE, _GEMM_GATHER_CELLS, vector_len, num_centroids, num_res_centroids, out_features, in_features, tokens)


def gemm_gatherx_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int) -> bool:
    """does a layer of this format and shape take `vptq_quant_gemm_gatherx` for `tokens` tokens?  Pure: no device, no library (one
    codebook group, no outliers, scale and bias, alignment: `vptq_quant_gemm_gatherx_supported`'s answer).  Never for the formats
    `gemm_gather_route` owns (v = 8, 65536 main centroids, 0 / 256 / 65536 residual centroids): a layer has one batched-decode kernel."""
    return _batched_decode_entry(vector_len, num_centroids, num_res_centroids) == "vptq_quant_gemm_gatherx" and in_features % 8 == 0 and \
        _batched_decode_route(_GEMM_GATHERX_MODE, _GEMM_GATHERX_CELLS, vector_len, num_centroids, num_res_centroids, out_features, in_features, tokens)


# WHICH (shape, token count) of the canonical format (v = 8, 256 + 256 centroids) take `vptq_quant_gemm_k256w` - 17 - 64 tokens in ONE
# launch (gemm_k256w_kernel, gemm_k256.hip) - in place of the route they had (17 - 48 tokens: launches of 16 of gemm_k256_kernel; 49 -
# 64: the dense route): the one rule, read by `VQuantLinear.forward` and `ops.quant_gemm`.  Only layers whose arithmetic is the
# reference's roundings (`LayerCache.arithmetic_flags` has GEMV_EXACT) are asked: the kernel has no other.  A cell is (least index
# elements = vector-rows x columns, least tokens, most tokens), routed by the rule above (beats its parent by more than the larger of
# 5 % and three times the larger spread, in every measured cell of the region, in both dtypes; the routed token counts of a layer
# are one interval); tools/gemm_k256w_bench.py writes the table.  VPTQ_GEMM_K256W=1 / 0 (with VPTQ_TUNING=1): every supported layer
# from 17 to 64 tokens / none.
#
# profiles/r19/table.md, profiles/r19/README.md (one MI355X, fp16 and bf16, 4096 x 4096 ... 8192 x 28672, tokens 17 / 24 / 32 / 33 / 48 /
# 49 / 64): at 17 - 48 tokens the kernel beats the launches of 16 in every measured cell (0.47 - 0.79 of their time), so 17 - 48 tokens
# are routed from the smallest measured layer (4096 x 4096 = 2 M index elements) up.  At 49 - 64 tokens (four token blocks, 23 - 41
# registers spilled) it beats the dense route at 8192 x 8192 and 8192 x 28672 in fp16 (0.68 - 0.83) but not by the rule in bf16 at 64
# tokens (0.94 - 0.96), and loses on the 14336-wide layers (0.95 - 1.40): no region wins in every cell, so 49 - 64 keep the dense route.
_GEMM_K256W_CELLS = ((2 << 20, 17, 48),)
GEMM_K256W_MIN_TOKENS, GEMM_K256W_MAX_TOKENS = 17, 64
_GEMM_K256W_MODE = (B.tune_env("VPTQ_GEMM_K256W", "auto") or "auto").strip().lower()


def gemm_k256w_route(out_features: int, in_features: int, tokens: int) -> bool:
    """does a canonical-format layer of this shape take `vptq_quant_gemm_k256w` for `tokens` tokens?  Pure: no device, no library
    (whether the library serves the layer is `vptq_quant_gemm_k256w_supported`'s answer, the arithmetic the caller's)."""
    if _GEMM_K256W_MODE in ("0", "off") or not GEMM_K256W_MIN_TOKENS <= tokens <= GEMM_K256W_MAX_TOKENS:
        return False
    if _GEMM_K256W_MODE in ("1", "on"):
        return True
    n_el = ((out_features + 7) // 8) * in_features
    return any(n_el >= min_el and min_tok <= tokens <= max_tok for min_el, min_tok, max_tok in _GEMM_K256W_CELLS)


# WHICH (format, shape, token count) of gemm_gather's formats (v = 8, 65536 main centroids, 0 / 256 / 65536 residual centroids) take
# `vptq_quant_gemm_gatherw` - 17 - 48 tokens in ONE launch (gemm_gatherw_kernel, gemm_gatherw.hip) - in place of the dense route
# they had: the one rule, read by `VQuantLinear.forward` and `ops.quant_gemm`.  A cell is (residual centroids, least index elements
# = vector-rows x columns, least tokens, most tokens), routed by the rule above `_GEMM_GATHER_CELLS` (beats its parent by more than
# the larger of 5 % and three times the run-to-run spread, in every measured cell of the region, in both dtypes; the routed token
# counts of a layer are one interval); tools/gemm_gatherw_bench.py writes the table.  No cell starts below 4 M index elements: a
# compacted 4096 x 4096 layer keeps its dense route, which needs no repack there (`sliced_routes.dense_from_layout`).  VPTQ_GEMM_GATHERW=1 / 0
# (with VPTQ_TUNING=1): every supported layer from 17 to 48 tokens / none.
#
# profiles/r23/table.md, profiles/r23/README.md (one MI355X, fp16 and bf16, 4096 x 4096 ... 8192 x 28672, tokens 17 / 24 / 32 / 33 / 40 /
# 48, layers without a permutation): at 17 - 24 tokens the kernel beats the dense route in every measured cell of the three formats
# (0.66 - 0.92 of its time), so 17 - 24 tokens are routed from the smallest measured layer above 4 M elements (14336 x 4096 = 7 M) up.
# From 32 tokens it does not win on 14336 x 4096 (0.98 - 1.25) and is level at 8192 x 8192 (0.88 - 1.13), and wins in every cell only at
# 8192 x 28672 (28 M elements: 0.70 - 0.88 at 32 - 48 tokens), so 25 - 48 tokens are routed from that size up.  LAYERS WITH A COLUMN
# PERMUTATION ARE NEVER ROUTED (only the knob reaches them): the kernel gathers a permuted x two bytes at a time in every row group and
# took 1.8 - 6.8 times the dense route's time at 8192 x 8192 and 14336 x 4096 (profiles/r23/table_perm.md).
_GEMM_GATHERW_CELLS = tuple((kr, el, lo, hi) for kr in (0, 256, 65536) for el, lo, hi in ((7 << 20, 17, 24), (28 << 20, 17, 48)))
GEMM_GATHERW_MIN_TOKENS, GEMM_GATHERW_MAX_TOKENS = 17, 48
GEMM_GATHERW_MIN_ELEMENTS = 4 << 20
_GEMM_GATHERW_MODE = (B.tune_env("VPTQ_GEMM_GATHERW", "auto") or "auto").strip().lower()


def gemm_gatherw_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int) -> bool:
    """does a layer of this format and shape take `vptq_quant_gemm_gatherw` for `tokens` tokens?  Pure: no device, no library
    (whether the library serves the layer is `vptq_quant_gemm_gatherw_supported`'s answer)."""
    if _GEMM_GATHERW_MODE in ("0", "off") or not GEMM_GATHERW_MIN_TOKENS <= tokens <= GEMM_GATHERW_MAX_TOKENS or \
            _batched_decode_entry(vector_len, num_centroids, num_res_centroids) != "vptq_quant_gemm_gather":
        return False
    if _GEMM_GATHERW_MODE in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any(kr == num_res_centroids and n_el >= max(min_el, GEMM_GATHERW_MIN_ELEMENTS) and min_tok <= tokens <= max_tok
               for kr, min_el, min_tok, max_tok in _GEMM_GATHERW_CELLS)


# WHICH (format, shape, token count) of the three kernels' layers WITH A COLUMN PERMUTATION take `vptq_quant_gemm_gather_px` - x[perm]
# written once per call into the stream's workspace, then the layer's kernel in its form without a permutation (gemm_gather_px.hip),
# 5 - 48 tokens - in place of the route a permuted layer has: the one rule, read by `VQuantLinear.forward` and `ops.quant_gemm`
# ahead of the three route functions above (which are what they were; layers without a permutation never come here).  A cell is
# (vector length, main centroids, residual centroids, least index elements, least tokens, most tokens), routed by the rule above
# `_GEMM_GATHER_CELLS`: px beats the route a permuted layer takes WITHOUT it (5 - 8 tokens: the gemv_gather / gemv_gatherx launches;
# 9 - 16: the in-kernel permuted gemm_gather / gemm_gatherx where their cells route it, else the dense route; 17 - 48: the dense
# route) by more than the larger of 5 % and three times the larger run-to-run spread, in every measured cell of the region, in both
# dtypes; the routed token counts of a layer are one interval; no cell lies under GEMM_GATHERW_MIN_ELEMENTS (4 M index elements).
# tools/gemm_gather_px_bench.py writes the table.  VPTQ_GEMM_GATHER_PX=1 / 0 (with VPTQ_TUNING=1): every supported permuted layer
# from 5 to 48 tokens / none.
#
# profiles/r25/table.md, profiles/r25/README.md (one MI355X, fp16 and bf16, permuted layers of 4096 x 4096 ... 8192 x 28672, tokens 5 / 8 /
# 9 / 12 / 16 / 17 / 24 / 32 / 33 / 40 / 48; 530 cells, px has the bits of the layer's own entry in every one, 526 win; run-to-run spreads
# under 3 % in all but two cells):
#   v8-k65536-0 / -256 / -65536   5 - 8 tokens 0.16 - 0.77 of the gemv_gather launches, 9 - 16 tokens 0.18 - 0.64 of the in-kernel permuted
#                                 gemm_gather (itself 1.05 - 2.6 times the dense route), 17 - 40 tokens 0.37 - 0.93 of the dense route: every
#                                 cell of every shape wins.  48 tokens: 4096 x 14336 (7 M elements) loses or is level in -0 and -256
#                                 (0.92 - 1.09), the other layers from 7 M up win (0.49 - 0.81), -65536 wins everywhere (0.54 - 0.93).  So
#                                 5 - 40 tokens from 7 M index elements, 5 - 48 from 8 M (8192 x 8192); -65536: 5 - 48 from 7 M.
#   v16-k65536-0 / -1024          5 - 16 tokens 0.17 - 0.69 of the in-kernel permuted gemm_gatherx in every cell: routed from the floor
#                                 (8192 x 8192 = 4 M elements of v = 16) up
#   v8-k32768-0, v8-k65536-4096   5 - 16 tokens 0.19 - 0.72 of gemv_gatherx (5 - 8, under 8 M) / the permuted gemm_gatherx: from 7 M up
# 4096 x 4096 (and the 3.5 M-element v = 16 layers) win too (0.30 - 0.88; one bf16 cell at 48 tokens short of the rule) but lie under the
# floor: they keep their routes - at 9 - 16 tokens that is the in-kernel permuted kernel, measured here at 1.05 - 3.0 times the dense route
# (STATUS.md, item 4c(b)).
_GEMM_GATHER_PX_CELLS = (
    (8, 65536, 0, 7 << 20, 5, 40), (8, 65536, 0, 8 << 20, 5, 48), (8, 65536, 256, 7 << 20, 5, 40), (8, 65536, 256, 8 << 20, 5, 48),
    (8, 65536, 65536, 7 << 20, 5, 48),
    (16, 65536, 0, 4 << 20, 5, 16), (16, 65536, 1024, 4 << 20, 5, 16), (8, 32768, 0, 7 << 20, 5, 16), (8, 65536, 4096, 7 << 20, 5, 16),
)
GEMM_GATHER_PX_MIN_TOKENS, GEMM_GATHER_PX_MAX_TOKENS = 5, 48
_GEMM_GATHER_PX_MODE = (B.tune_env("VPTQ_GEMM_GATHER_PX", "auto") or "auto").strip().lower()


def gemm_gather_px_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int) -> bool:
    """does a layer WITH a column permutation of this format and shape take `vptq_quant_gemm_gather_px` for `tokens` tokens?  Pure:
    no device, no library (whether the library serves the layer is `vptq_quant_gemm_gather_px_supported`'s answer; that the layer
    has a permutation is the caller's)."""
    if _GEMM_GATHER_PX_MODE in ("0", "off") or not GEMM_GATHER_PX_MIN_TOKENS <= tokens <= GEMM_GATHER_PX_MAX_TOKENS:
        return False
    entry = _batched_decode_entry(vector_len, num_centroids, num_res_centroids)
    if entry is None or (tokens > GEMM_GATHER_MAX_TOKENS and entry != "vptq_quant_gemm_gather") or in_features % 8:
        return False   # (17 - 48 tokens: gemm_gatherw's formats only)
    if _GEMM_GATHER_PX_MODE in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any((v, k, kr) == (vector_len, num_centroids, num_res_centroids) and n_el >= max(min_el, GEMM_GATHERW_MIN_ELEMENTS) and
               min_tok <= tokens <= max_tok for v, k, kr, min_el, min_tok, max_tok in _GEMM_GATHER_PX_CELLS)


# WHICH (format, shape, token count) of gemm_gatherx's formats (v = 8 / 16, 16384 ... 65536 main centroids, any residual codebook -
# the formats for which `_batched_decode_entry` says `vptq_quant_gemm_gatherx`) take `vptq_quant_gemm_gatherxw` - 17 - 48 tokens in
# ONE launch (gemm_gatherxw_kernel, gemm_gatherxw.hip; a layer with a column permutation: x[perm] written once into the stream's
# workspace in front of it) - in place of the dense route they had, permuted or not: the one rule, read by `VQuantLinear.forward` and
# `ops.quant_gemm`.  A cell is (vector length, main centroids, residual centroids, has a permutation, least index elements = vector-rows
# x columns, least tokens, most tokens), routed by the rule above `_GEMM_GATHER_CELLS` (beats its parent by more than the larger of
# 5 % and three times the larger run-to-run spread, in every measured cell of the region, in both dtypes; the routed token counts of a
# layer are one interval; no cell lies under GEMM_GATHERW_MIN_ELEMENTS, 4 M index elements); tools/gemm_gatherxw_bench.py writes the
# table.  VPTQ_GEMM_GATHERXW=1 / 0 (with VPTQ_TUNING=1): every supported layer from 17 to 48 tokens / none.
#
# profiles/r35/table.md, profiles/r35/README.md (one MI355X, fp16 and bf16, 4096 x 4096 ... 8192 x 28672 and 28672 x 8192, tokens 17 / 24 /
# 32 / 33 / 40 / 48, with and without a permutation; 864 cells, the 16-token entry's bits in every one, 516 win; spreads over 3 % in 17
# cells).  v = 16 layers have 4 M index elements at 8192 x 8192 and 14 M at 8192 x 28672 / 28672 x 8192 (their 14336-wide layers, 3.5 M,
# lie under the floor); v = 8 layers 7 M (14336-wide), 8 M and 28 M.  A cell's region is every measured layer from its size up:
#   WITH a permutation (the parent gathers W's columns while it rebuilds it, and x[perm] costs 3 - 7 us here): v16-k65536-1024 /
#     -32768 / -65536 win in every cell from 4 M up (0.46 - 0.94); v16-k65536-0 at 4 M only at 17 - 24 tokens (0.74 - 0.88; 0.91 - 1.21
#     from 32), from 14 M everywhere (0.54 - 0.91); v8-k32768-0 from 7 M at 17 - 24 (0.57 - 0.87; 4096 x 14336 loses from 32: 1.01 -
#     1.23), from 8 M everywhere (0.45 - 0.94); v8-k65536-4096 from 7 M up to 33 tokens (0.55 - 0.93; 4096 x 14336 at 40: 0.93 / 0.96),
#     from 8 M everywhere (0.47 - 0.78)
#   WITHOUT one: v16-k65536-0 only from 14 M, 17 - 40 tokens (0.68 - 0.94; 8192 x 28672 at 48: 1.02 / 1.05); v16-k65536-1024 from 4 M at
#     17 - 24 (0.82 - 0.89), from 14 M at 17 - 40 (0.64 - 0.93); v16-k65536-32768 from 14 M at 17 - 24 (0.78 - 0.90); v16-k65536-65536
#     nowhere (8192 x 8192: 1.08 - 1.37; 28672 x 8192: 0.93 - 1.11); v8-k32768-0 from 7 M at 17 tokens (0.82 - 0.89), from 8 M at 17 - 24
#     (0.63 - 0.88), from 28 M at 17 - 40 (0.63 - 0.94); v8-k65536-4096 from 8 M at 17 tokens (4096 x 14336 does not win: 0.93 / 0.97),
#     from 28 M at 17 - 24 (0.80 - 0.87)
# Formats that were not measured (v16-k65536-256 / -64, v8-k65536-4, v8-k16384-0) are not routed.
_GEMM_GATHERXW_CELLS = (
    (16, 65536, 0, 1, 4 << 20, 17, 24), (16, 65536, 0, 1, 14 << 20, 17, 48), (16, 65536, 0, 0, 14 << 20, 17, 40),
    (16, 65536, 1024, 1, 4 << 20, 17, 48), (16, 65536, 1024, 0, 4 << 20, 17, 24), (16, 65536, 1024, 0, 14 << 20, 17, 40),
    (16, 65536, 32768, 1, 4 << 20, 17, 48), (16, 65536, 32768, 0, 14 << 20, 17, 24),
    (16, 65536, 65536, 1, 4 << 20, 17, 48),
    (8, 32768, 0, 1, 7 << 20, 17, 24), (8, 32768, 0, 1, 8 << 20, 17, 48),
    (8, 32768, 0, 0, 7 << 20, 17, 17), (8, 32768, 0, 0, 8 << 20, 17, 24), (8, 32768, 0, 0, 28 << 20, 17, 40),
    (8, 65536, 4096, 1, 7 << 20, 17, 33), (8, 65536, 4096, 1, 8 << 20, 17, 48),
    (8, 65536, 4096, 0, 8 << 20, 17, 17), (8, 65536, 4096, 0, 28 << 20, 17, 24),
)
GEMM_GATHERXW_MIN_TOKENS, GEMM_GATHERXW_MAX_TOKENS = 17, 48
_GEMM_GATHERXW_MODE = (B.tune_env("VPTQ_GEMM_GATHERXW", "auto") or "auto").strip().lower()


def gemm_gatherxw_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int,
                        has_perm: Optional[bool] = None) -> bool:
    """does a layer of this format and shape take `vptq_quant_gemm_gatherxw` for `tokens` tokens?  has_perm: whether the layer has a
    column permutation (the cells are measured per state); None: a layer of either state, i.e. whether ANY cell takes it - what a
    caller that sizes a workspace asks.  Pure: no device, no library (whether the library serves the layer is
    `vptq_quant_gemm_gatherxw_supported`'s answer).  Never for the formats `gemm_gather_route` owns."""
    if _GEMM_GATHERXW_MODE in ("0", "off") or not GEMM_GATHERXW_MIN_TOKENS <= tokens <= GEMM_GATHERXW_MAX_TOKENS or in_features % 8 or \
            _batched_decode_entry(vector_len, num_centroids, num_res_centroids) != "vptq_quant_gemm_gatherx":
        return False
    if _GEMM_GATHERXW_MODE in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any((v, k, kr) == (vector_len, num_centroids, num_res_centroids) and (has_perm is None or bool(p) == bool(has_perm)) and
               n_el >= max(min_el, GEMM_GATHERW_MIN_ELEMENTS) and min_tok <= tokens <= max_tok
               for v, k, kr, p, min_el, min_tok, max_tok in _GEMM_GATHERXW_CELLS)


# WHICH (format, shape, token count) of the large-codebook formats of VECTOR LENGTH 12 (16384 ... 65536 main centroids, any residual
# codebook: "v12-k65536-4096" of the published checkpoints) take `vptq_quant_gemm_gather12` - 5 - 16 tokens in ONE launch
# (gemm_gather12_kernel, gemm_gather12.hip: row groups of 48 outputs = three MFMA N blocks; a layer with a column permutation: x[perm]
# written once into the stream's workspace in front of it) - in place of the route they had (5 - 8 tokens: two gemv_gatherx launches,
# which stops at 4 token slots for v = 12; 9 - 16: the dense route): the one rule, read by `VQuantLinear.forward` and `ops.quant_gemm`.
# `_batched_decode_entry` keeps answering None for v = 12 (the first two tables are what they were); the format test is `_v12_owns`.
# A cell is (main centroids, residual centroids, has a permutation, least index elements = vector-rows x columns, least tokens, most
# tokens), routed by the rule above `_GEMM_GATHER_CELLS` (beats its parent by more than the larger of 5 % and three times the larger
# run-to-run spread, in every measured cell of the region, in both dtypes; the routed token counts of a layer are one interval);
# tools/gemm_gather12_bench.py writes the table.  VPTQ_GEMM_GATHER12=1 / 0 (with VPTQ_TUNING=1): every supported layer from 5 to 16
# tokens / none.
#
# profiles/r37/table.md, profiles/r37/README.md (one MI355X, fp16 and bf16, 4096 x 4096 ... 8192 x 28672, tokens 5 / 8 / 9 / 12 / 16, with
# and without a permutation; 300 cells, the entry's bits checked in every one, 178 win; spreads over 3 % in 9 cells).  v = 12 layers
# have 1.3 M index elements at 4096 x 4096, 4.7 M at 4096 x 14336 and 14336 x 4096 (columns x outputs), 5.3 M at 8192 x 8192 and 18.7 M
# at 8192 x 28672.  A cell's region is every measured layer from its size up:
#   4096 x 4096 loses nearly everywhere (1.03 - 1.65 of the parent's time; 29 row groups on 512 workgroup slots) and 14336 x 4096 (86
#     row groups) loses at 9 - 16 tokens in every format (0.99 - 2.11), so no region reaches below 8192 x 8192 at 9 - 16 tokens
#   WITH a permutation (the parents gather x or W's columns in every launch): all three formats win at 5 - 8 tokens from 4096 x 14336 /
#     14336 x 4096 up (0.28 - 0.90) and at 5 - 16 tokens from 8192 x 8192 up (0.28 - 0.84)
#   WITHOUT one: v12-k65536-4096 wins at 5 - 8 tokens from 8192 x 8192 up (0.50 - 0.92; 9 - 16 there: fp16 0.91, bf16 1.24) and at
#     5 - 16 at 8192 x 28672 (0.50 - 0.79); v12-k65536-0 and -256 only at 8192 x 28672 (0.54 - 0.77; 8192 x 8192: -0 0.87 - 0.98 with
#     one winning token count, -256 0.85 - 1.14)
# v12-k32768-1024 and the other formats of the kernel were not measured and are not routed.
_GEMM_GATHER12_CELLS = tuple(c for kr in (0, 256, 4096) for c in ((65536, kr, 1, 4 << 20, 5, 8), (65536, kr, 1, 5 << 20, 5, 16))) + (
    (65536, 0, 0, 18 << 20, 5, 16), (65536, 256, 0, 18 << 20, 5, 16), (65536, 4096, 0, 5 << 20, 5, 8), (65536, 4096, 0, 18 << 20, 5, 16))
GEMM_GATHER12_MIN_TOKENS, GEMM_GATHER12_MAX_TOKENS = 5, 16
_GEMM_GATHER12_MODE = (B.tune_env("VPTQ_GEMM_GATHER12", "auto") or "auto").strip().lower()


def _v12_owns(vector_len: int, num_centroids: int, num_res_centroids: int) -> bool:
    """is the format `vptq_quant_gemm_gather12`'s?"""
    return vector_len == 12 and _pow2(num_centroids) and 16384 <= num_centroids <= 65536 and \
        (not num_res_centroids or (_pow2(num_res_centroids) and num_res_centroids <= 65536))


def gemm_gather12_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int,
                        has_perm: Optional[bool] = None) -> bool:
    """does a layer of this format and shape take `vptq_quant_gemm_gather12` for `tokens` tokens?  has_perm: whether the layer has a
    column permutation (the cells are measured per state); None: a layer of either state, i.e. whether ANY cell takes it.  Pure: no
    device, no library (whether the library serves the layer is `vptq_quant_gemm_gather12_supported`'s answer)."""
    if _GEMM_GATHER12_MODE in ("0", "off") or not GEMM_GATHER12_MIN_TOKENS <= tokens <= GEMM_GATHER12_MAX_TOKENS or in_features % 8 or \
            not _v12_owns(vector_len, num_centroids, num_res_centroids):
        return False
    if _GEMM_GATHER12_MODE in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any((k, kr) == (num_centroids, num_res_centroids) and (has_perm is None or bool(p) == bool(has_perm)) and n_el >= min_el and
               min_tok <= tokens <= max_tok for k, kr, p, min_el, min_tok, max_tok in _GEMM_GATHER12_CELLS)


# WHICH v = 12 layers take `vptq_quant_gemm_gather12c` (gemm_gather12c.hip: gemm_gather12's kernel with the work split over (row group,
# column part) and a second small kernel that adds the parts' fp32 sums in a fixed order) for 5 - 16 tokens, in place of the route they
# have at the knob's "0" (`gemm_gather12_route`'s cells, else two gemv_gatherx launches / the dense route).  Whether a split helps is
# decided by the ROW-GROUP count (few outputs: the parent kernel leaves most resident workgroups idle), so a cell carries a MOST bound
# on the index elements beside the least one, like the canonical group's cells: (main centroids, residual centroids, has a permutation,
# least index elements, most index elements, least tokens, most tokens).  No cell lies under 1 M index elements.  Routed by the rule
# above `_GEMM_GATHER_CELLS`; tools/gemm_gather12c_bench.py writes the table.  VPTQ_GEMM_GATHER12C=1 / 0 (with VPTQ_TUNING=1): every
# layer the library splits (`vptq_quant_gemm_gather12c_supported`: at least two 512-column tiles) from 5 to 16 tokens / none.
#
# profiles/r38/table.md, profiles/r38/README.md (one MI355X, v12-k65536-4096 / -256 / -0, fp16 and bf16, with and without a permutation,
# 4096 x 4096 (1.3 M index elements, 86 row groups), 4096 x 1024 (0.3 M, 22), 14336 x 4096 (4.7 M, 86), 4096 x 14336 (4.7 M, 299) and 8192 x
# 8192 (5.3 M, 171) (columns x outputs), tokens 5 / 8 / 9 / 12 / 16, parts = 0; 300 cells, the entry's bits checked in every one; spreads
# over 3 % in 9 cells, the largest 5.8 %).  EVERY cell wins by the rule, in both dtypes: 0.40 - 0.93 of the parent-commit route -
#   4096 x 4096 0.45 - 0.82 (v12-k65536-4096 fp16 with a permutation, 5 / 8 / 16 tokens: 25.2 / 25.2 / 25.7 us against 47.7 / 55.7 / 35.8)
#   14336 x 4096 0.40 - 0.92 (64.3 / 64.1 / 65.1 against 137.4 / 137.6 (gemm_gather12, its routed cell) / 138.4 (dense))
#   4096 x 14336 0.52 - 0.88, 8192 x 8192 0.64 - 0.93 (against gemm_gather12 where it is routed: 0.68 - 0.83)
#   4096 x 1024 0.43 - 0.67, but 0.3 M index elements: under the 1 M floor of every cell, so only the knob reaches it
# so one region per (format, permutation state): 1 M - 6 M index elements (the largest measured layer has 5.3 M), 5 - 16 tokens.  8192 x
# 28672 (18.7 M, 598 row groups: more than the resident workgroups, nothing to fill) was not measured and stays with `gemm_gather12`;
# so do v12-k32768-1024 and the other unmeasured formats.  The regions are by index elements, as every table of this file: a layer of
# 1 - 6 M elements with many more row groups than the measured ones (2048 columns x 28672 outputs) is routed without having been measured.
_GEMM_GATHER12C_CELLS = tuple((65536, kr, p, 1 << 20, 6 << 20, 5, 16) for kr in (0, 256, 4096) for p in (0, 1))
_GEMM_GATHER12C_MODE = (B.tune_env("VPTQ_GEMM_GATHER12C", "auto") or "auto").strip().lower()


def gemm_gather12c_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int,
                         has_perm: Optional[bool] = None) -> bool:
    """does a layer of this format and shape take `vptq_quant_gemm_gather12c` (parts = 0: the library's rule) for `tokens` tokens?
    has_perm as in `gemm_gather12_route`.  Pure: no device, no library (whether the library splits the layer is
    `vptq_quant_gemm_gather12c_supported`'s answer)."""
    if _GEMM_GATHER12C_MODE in ("0", "off") or not GEMM_GATHER12_MIN_TOKENS <= tokens <= GEMM_GATHER12_MAX_TOKENS or in_features % 8 or \
            not _v12_owns(vector_len, num_centroids, num_res_centroids):
        return False
    if _GEMM_GATHER12C_MODE in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any((k, kr) == (num_centroids, num_res_centroids) and (has_perm is None or bool(p) == bool(has_perm)) and
               max(min_el, 1 << 20) <= n_el <= max_el and min_tok <= tokens <= max_tok
               for k, kr, p, min_el, max_el, min_tok, max_tok in _GEMM_GATHER12C_CELLS)


# WHICH v = 12 layers take `vptq_quant_gemm_gather12w` (gemm_gather12w.hip: 2 / 3 blocks of 16 tokens over gemm_gather12c's walk of (row
# group, column part) items; one part: the kernel writes y itself, else a second small kernel adds the parts' fp32 sums in a fixed
# order; a layer with a column permutation: x[perm] written once into the stream's workspace in front) for 17 - 48 tokens, in place of
# the dense route (vptq_dequant + F.linear) they have at the knob's "0".  A cell is `_GEMM_GATHER12C_CELLS`' (main centroids, residual
# centroids, has a permutation, least index elements, most index elements, least tokens, most tokens); none lies under 1 M index
# elements; routed by the rule above `_GEMM_GATHER_CELLS` (beats the dense route by more than the larger of 5 % and three times the
# larger run-to-run spread, in every measured cell of the region, in both dtypes; the routed token counts of a layer are one interval);
# tools/gemm_gather12c_bench.py --wide writes the table.  VPTQ_GEMM_GATHER12W=1 / 0 (with VPTQ_TUNING=1): every layer
# `vptq_quant_gemm_gather12w_supported` accepts from 17 to 48 tokens / none.
#
# profiles/r39/table.md, profiles/r39/README.md (one MI355X, v12-k65536-4096 / -256 / -0, fp16 and bf16, with and without a permutation, 4096 x
# 4096, 14336 x 4096, 4096 x 1024, 4096 x 14336, 8192 x 8192 and 8192 x 28672 (columns x outputs), tokens 17 / 24 / 32 / 33 / 40 / 48, parts = 0;
# 432 cells, the entry's bits checked in every one, 370 win; spreads over 3 % in 20 cells, the largest 6.5 %):
#   17 - 32 tokens (two token blocks): 0.39 - 0.93 of the dense route; every cell wins except v12-k65536-4096 bf16 WITHOUT a permutation on
#     8192 x 8192 and 14336 x 4096 (0.96 - 0.99) and on 4096 x 14336 at 32 tokens (0.95), and one fp16 cell of v12-k65536-0 on 4096 x 4096
#     (0.82, by its spread)
#   33 - 48 tokens (three): v12-k65536-0 wins everywhere from 4.7 M index elements (0.46 - 0.82); with a residual table the kernel runs at
#     ONE workgroup per CU there: without a permutation 0.89 - 1.21 on the layers up to 5.3 M (bf16 loses in every such cell) and 0.72 - 1.01 at
#     8192 x 28672; 4096 x 4096 0.93 - 1.18 with or without one; with a permutation it wins from 4.7 M up (0.53 - 0.93; one bf16 cell at 48
#     tokens 0.96)
# NO CELL IS SHIPPED YET: the regions that win in every measured cell are listed in profiles/r39/README.md, but the suite was not run
# with them in place, so the entry is reached by the knob (and `ops.quant_gemm_gather12w`) alone.
_GEMM_GATHER12W_CELLS = ()
GEMM_GATHER12W_MIN_TOKENS, GEMM_GATHER12W_MAX_TOKENS = 17, 48
_GEMM_GATHER12W_MODE = (B.tune_env("VPTQ_GEMM_GATHER12W", "auto") or "auto").strip().lower()


def gemm_gather12w_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int, tokens: int,
                         has_perm: Optional[bool] = None) -> bool:
    """does a layer of this format and shape take `vptq_quant_gemm_gather12w` (parts = 0: the library's rule) for `tokens` tokens?
    has_perm as in `gemm_gather12_route`.  Pure: no device, no library (whether the library serves the layer is
    `vptq_quant_gemm_gather12w_supported`'s answer)."""
    if _GEMM_GATHER12W_MODE in ("0", "off") or not GEMM_GATHER12W_MIN_TOKENS <= tokens <= GEMM_GATHER12W_MAX_TOKENS or in_features % 8 or \
            not _v12_owns(vector_len, num_centroids, num_res_centroids):
        return False
    if _GEMM_GATHER12W_MODE in ("1", "on"):
        return True
    n_el = ((out_features + vector_len - 1) // vector_len) * in_features
    return any((k, kr) == (num_centroids, num_res_centroids) and (has_perm is None or bool(p) == bool(has_perm)) and
               max(min_el, 1 << 20) <= n_el <= max_el and min_tok <= tokens <= max_tok
               for k, kr, p, min_el, max_el, min_tok, max_tok in _GEMM_GATHER12W_CELLS)


class BatchedDecodeRoute(NamedTuple):
    """what differs between the batched-decode routes; everything else is one code path in both callers"""
    entry: str                    # the library entry (`entry + "_supported"`: does the library serve this descriptor?)
    min_tokens: int               # the token window of the entry
    max_tokens: int
    owns: Callable[[int, int, int], bool]   # (vector length, main centroids, residual centroids): is the format this route's?
    route: Callable[..., bool]    # (vector length, main centroids, residual centroids, out_features, in_features, tokens): the route function
    knob: str                     # the module global that holds the route's knob
    perm: Optional[bool]          # True: only layers WITH a column permutation; False: only layers without one, unless the knob is on; None: either
    off_flags: int                # launch flags that switch the route off
    exact_only: bool = False      # the kernel has the reference's roundings only: the CALLER asks the layer's arithmetic, last (it may cost a read-back)
    workspace: bool = False       # the entry takes (workspace, workspace_bytes) in front of the stream (`entry + "_workspace_bytes"` sizes it)
    perm_cells: bool = False      # the route function takes whether the layer has a permutation as a seventh argument: cells per state
    extra: tuple = ()             # integer arguments the entry takes behind the tokens (`_supported`, `_workspace_bytes`) / the flags (the launch)


def _entry_is(*entries):
    return lambda v, k, kr: _batched_decode_entry(v, k, kr) in entries


# In priority order: a call takes the first route that accepts it and whose launch does not step aside.  gemm_k256w's format is
# disjoint from every other route's, so its place among them changes no answer: (px, gather, gatherx, k256w, gatherw) and (px, gather,
# gatherx, gatherw, k256w) are the same order.
BATCHED_DECODE_ROUTES = (
    BatchedDecodeRoute("vptq_quant_gemm_gather_px", GEMM_GATHER_PX_MIN_TOKENS, GEMM_GATHER_PX_MAX_TOKENS,
                       _entry_is("vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx"), gemm_gather_px_route, "_GEMM_GATHER_PX_MODE",
                       True, B.GEMV_FORCE_GENERIC, workspace=True),
    BatchedDecodeRoute("vptq_quant_gemm_gather", 5, GEMM_GATHER_MAX_TOKENS, _entry_is("vptq_quant_gemm_gather"), gemm_gather_route,
                       "_GEMM_GATHER_MODE", None, B.GEMV_FORCE_GENERIC),
    BatchedDecodeRoute("vptq_quant_gemm_gatherx", 5, GEMM_GATHER_MAX_TOKENS, _entry_is("vptq_quant_gemm_gatherx"), gemm_gatherx_route,
                       "_GEMM_GATHERX_MODE", None, B.GEMV_FORCE_GENERIC),
    BatchedDecodeRoute("vptq_quant_gemm_k256w", GEMM_K256W_MIN_TOKENS, GEMM_K256W_MAX_TOKENS, lambda v, k, kr: (v, k, kr) == (8, 256, 256),
                       lambda v, k, kr, out_features, in_features, tokens: gemm_k256w_route(out_features, in_features, tokens),
                       "_GEMM_K256W_MODE", None, B.GEMV_FORCE_ANY, exact_only=True),
    # (a permuted layer: 1.8 - 6.8 times the dense route, the comment above `_GEMM_GATHERW_CELLS` - only the knob reaches it)
    BatchedDecodeRoute("vptq_quant_gemm_gatherw", GEMM_GATHERW_MIN_TOKENS, GEMM_GATHERW_MAX_TOKENS, _entry_is("vptq_quant_gemm_gather"),
                       gemm_gatherw_route, "_GEMM_GATHERW_MODE", False, B.GEMV_FORCE_GENERIC),
)
# The single-layer counterpart of `GROUPED_DECODE_WIDE_ROUTES`: routes a caller walks AFTER those of `BATCHED_DECODE_ROUTES`, in a table
# of their own (the first table's records are what they were).  gemm_gatherxw owns gemm_gatherx's formats from the 17th token on, where
# the only first-table route of those formats (px) ends at 16: no call is taken from a route above.  A permuted layer and a plain one
# take the same entry (perm=None), which gathers x[perm] into the workspace itself.
BATCHED_DECODE_WIDE_ROUTES = (
    BatchedDecodeRoute("vptq_quant_gemm_gatherxw", GEMM_GATHERXW_MIN_TOKENS, GEMM_GATHERXW_MAX_TOKENS, _entry_is("vptq_quant_gemm_gatherx"),
                       gemm_gatherxw_route, "_GEMM_GATHERXW_MODE", None, B.GEMV_FORCE_GENERIC, workspace=True, perm_cells=True),
)
# A third table, walked after the two above: the formats of vector length 12, which no record above owns (`_batched_decode_entry`
# answers None for them), so no call is taken from a route above.  A permuted layer and a plain one take the same entry (perm=None),
# which gathers x[perm] into the workspace itself.  17 - 48 tokens are the fifth table's; sibling groups and v = 6 have no record: they keep
# their routes.
BATCHED_DECODE_V12_ROUTES = (
    BatchedDecodeRoute("vptq_quant_gemm_gather12", GEMM_GATHER12_MIN_TOKENS, GEMM_GATHER12_MAX_TOKENS, _v12_owns, gemm_gather12_route,
                       "_GEMM_GATHER12_MODE", None, B.GEMV_FORCE_GENERIC, workspace=True, perm_cells=True),
)
# A fourth table, walked IN FRONT OF the third: the column-parts form of the v = 12 kernel for layers with few outputs.  It owns the
# third table's formats; a call it takes would otherwise go to the third table's record or to the routes behind it, and with its knob
# at "0" every answer is that.  extra = (0,): `parts` = the library's rule.
BATCHED_DECODE_V12_COLUMN_ROUTES = (
    BatchedDecodeRoute("vptq_quant_gemm_gather12c", GEMM_GATHER12_MIN_TOKENS, GEMM_GATHER12_MAX_TOKENS, _v12_owns, gemm_gather12c_route,
                       "_GEMM_GATHER12C_MODE", None, B.GEMV_FORCE_GENERIC, workspace=True, perm_cells=True, extra=(0,)),
)
# A fifth table, walked BEHIND the four above: the v = 12 formats from the 17th token on, a window no record above has, so no call is
# taken from a route above and with its knob at "0" every answer is what it was.  extra = (0,): `parts` = the library's rule.
BATCHED_DECODE_V12_WIDE_ROUTES = (
    BatchedDecodeRoute("vptq_quant_gemm_gather12w", GEMM_GATHER12W_MIN_TOKENS, GEMM_GATHER12W_MAX_TOKENS, _v12_owns, gemm_gather12w_route,
                       "_GEMM_GATHER12W_MODE", None, B.GEMV_FORCE_GENERIC, workspace=True, perm_cells=True, extra=(0,)),
)
BATCHED_DECODE_MIN_TOKENS = min(r.min_tokens for r in BATCHED_DECODE_ROUTES)   # the union of the windows: what a caller guards with
BATCHED_DECODE_MAX_TOKENS = max(r.max_tokens for r in BATCHED_DECODE_ROUTES)


def batched_decode_routes(vector_len: int, num_centroids: int, num_res_centroids: int, num_codebooks: int, outliers: bool, norm: bool,
                          has_perm: bool) -> tuple:
    """the routes that can EVER serve a layer of this static configuration, in priority order (possibly none): one codebook, no
    outliers, scale and bias, the format the route's, a permutation where the route takes nothing else.  No knob is read."""
    return _static_routes(BATCHED_DECODE_ROUTES, vector_len, num_centroids, num_res_centroids, num_codebooks, outliers, norm, has_perm)


def batched_decode_wide_routes(vector_len: int, num_centroids: int, num_res_centroids: int, num_codebooks: int, outliers: bool, norm: bool,
                               has_perm: bool) -> tuple:
    """`batched_decode_routes` over `BATCHED_DECODE_WIDE_ROUTES`: the same static filters; a caller walks these after the first
    table's."""
    return _static_routes(BATCHED_DECODE_WIDE_ROUTES, vector_len, num_centroids, num_res_centroids, num_codebooks, outliers, norm, has_perm)


def batched_decode_v12_routes(vector_len: int, num_centroids: int, num_res_centroids: int, num_codebooks: int, outliers: bool, norm: bool,
                              has_perm: bool) -> tuple:
    """`batched_decode_routes` over `BATCHED_DECODE_V12_ROUTES`: the same static filters; a caller walks these after the other two
    tables'."""
    return _static_routes(BATCHED_DECODE_V12_ROUTES, vector_len, num_centroids, num_res_centroids, num_codebooks, outliers, norm, has_perm)


def batched_decode_v12_column_routes(vector_len: int, num_centroids: int, num_res_centroids: int, num_codebooks: int, outliers: bool,
                                     norm: bool, has_perm: bool) -> tuple:
    """`batched_decode_routes` over `BATCHED_DECODE_V12_COLUMN_ROUTES`: the same static filters; a caller walks these in front of
    `batched_decode_v12_routes`'."""
    return _static_routes(BATCHED_DECODE_V12_COLUMN_ROUTES, vector_len, num_centroids, num_res_centroids, num_codebooks, outliers, norm,
                          has_perm)


def batched_decode_v12_wide_routes(vector_len: int, num_centroids: int, num_res_centroids: int, num_codebooks: int, outliers: bool,
                                   norm: bool, has_perm: bool) -> tuple:
    """`batched_decode_routes` over `BATCHED_DECODE_V12_WIDE_ROUTES`: the same static filters; a caller walks these behind the four
    other tables'."""
    return _static_routes(BATCHED_DECODE_V12_WIDE_ROUTES, vector_len, num_centroids, num_res_centroids, num_codebooks, outliers, norm,
                          has_perm)


def _static_routes(table, vector_len, num_centroids, num_res_centroids, num_codebooks, outliers, norm, has_perm) -> tuple:
    if num_codebooks != 1 or outliers or not norm:
        return ()
    return tuple(r for r in table if r.owns(vector_len, num_centroids, num_res_centroids) and (has_perm or r.perm is not True))


def batched_decode_takes(route, vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int,
                         tokens: int, flags: int, has_perm: bool) -> bool:
    """the per-call decision: do `route`'s token window, off-flags, permutation rule and route function accept this call of a layer
    whose `batched_decode_routes` hold it?  A caller walks its routes in order and tries those that do: `exact_only`, `_supported`
    and the launch itself may still step aside (the caller's), and then the next route is asked."""
    if not route.min_tokens <= tokens <= route.max_tokens or (flags & route.off_flags):
        return False
    if route.perm is not None and route.perm != has_perm and (route.perm or globals()[route.knob] not in ("1", "on")):
        return False
    args = (vector_len, num_centroids, num_res_centroids, out_features, in_features, tokens)
    return route.route(*args, has_perm) if route.perm_cells else route.route(*args)

