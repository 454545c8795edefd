"""The batched-decode routes (5 - 64 tokens in ONE launch of a library entry): which (format, shape, token count) takes which entry.

Pure rules - no device, no tensors: the five route functions with their knobs and measured cells, one ordered table of what differs
between the routes (`BATCHED_DECODE_ROUTES`) and the two functions that read it, the static `batched_decode_routes` (per layer) and
the per-call `batched_decode_takes`.  `VQuantLinear.forward` and `ops.quant_gemm` both decide through them.  A new route is a
record in the table, a route function and a knob.
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
BATCHED_DECODE_MIN_TOKENS = min(r.min_tokens for r in BATCHED_DECODE_ROUTES)   # the union of the windows: what a caller guards with
BATCHED_DECODE_MAX_TOKENS = max(r.max_tokens for r in BATCHED_DECODE_ROUTES)


def batched_decode_routes(vector_len: int, num_centroids: int, num_res_centroids: int, num_codebooks: int, outliers: bool, norm: bool,
                          has_perm: bool) -> tuple:
    """the routes that can EVER serve a layer of this static configuration, in priority order (possibly none): one codebook, no
    outliers, scale and bias, the format the route's, a permutation where the route takes nothing else.  No knob is read."""
    if num_codebooks != 1 or outliers or not norm:
        return ()
    return tuple(r for r in BATCHED_DECODE_ROUTES
                 if r.owns(vector_len, num_centroids, num_res_centroids) and (has_perm or r.perm is not True))


def batched_decode_takes(route, vector_len: int, num_centroids: int, num_res_centroids: int, out_features: int, in_features: int,
                         tokens: int, flags: int, has_perm: bool) -> bool:
    """the per-call decision: do `route`'s token window, off-flags, permutation rule and route function accept this call of a layer
    whose `batched_decode_routes` hold it?  A caller walks its routes in order and tries those that do: `exact_only`, `_supported`
    and the launch itself may still step aside (the caller's), and then the next route is asked."""
    if not route.min_tokens <= tokens <= route.max_tokens or (flags & route.off_flags):
        return False
    if route.perm is not None and route.perm != has_perm and (route.perm or globals()[route.knob] not in ("1", "on")):
        return False
    return route.route(vector_len, num_centroids, num_res_centroids, out_features, in_features, tokens)

