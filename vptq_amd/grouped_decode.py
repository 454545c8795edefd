"""The batched-decode route of a GROUP of sibling layers (q / k / v, gate / up): which (format, shapes, token count) take
`vptq_quant_gemm_gather_grouped` - the members' row groups as one list in ONE launch, one x gather per distinct permutation - in
place of one launch (and one x gather) per member; for the canonical format, `vptq_quant_gemm_k256_grouped`; for 17 - 48 tokens of
the large-codebook formats, `vptq_quant_gemm_gatherw_grouped`; for 5 - 16 tokens of the other large-codebook formats (gemm_gatherx's),
`vptq_quant_gemm_gatherx_grouped`.

Pure rules - no device, no tensors, in the style of vptq_amd/batched_decode.py: per route one route function, its knob and its
measured cells, and `GROUPED_DECODE_ROUTES`, the ordered record of the group routes (`GROUPED_DECODE_WIDE_ROUTES`: a format's routes
beyond its first window; `GROUPED_DECODE_X_ROUTES`: the routes of formats the first table has no owner for; `sibling_decode_routes`
reads all three).  These routes are a group's, not a layer's: `BATCHED_DECODE_ROUTES` and the layers' cell tables do not know it, and a group that
is not routed here leaves every member on the routes it had.  `SiblingGroup.forward_batched` (vptq_amd/layers/vqlinear.py) and
`prepare_model` decide through it.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence

from vptq_amd import _backend as B
from vptq_amd.batched_decode import _batched_decode_entry

# WHICH groups take the grouped launch.  The kernel is gemm_gather's (v = 8, 65536 main centroids, 0 / 256 / 65536 residual
# centroids), 5 - 16 tokens (1 - 4 tokens are `SiblingGroup.forward` / `forward_sliced`'s).  A cell is (residual centroids, has_perm,
# least TOTAL index elements of the group = the sum of vector-rows x columns over its members, least tokens, most tokens); has_perm:
# True - every member has a column permutation, False - none has (a group of both is measured nowhere and is never routed by a
# cell).  A cell is routed by the rule above `_GEMM_GATHER_CELLS` of vptq_amd/batched_decode.py: the grouped launch beats the SUM of
# what the members take without it by more than the larger of 5 % and three times the larger run-to-run spread, in every measured cell
# of the region, in both dtypes; the routed token counts of a group are one interval; no cell starts under
# GEMM_GATHER_GROUPED_MIN_ELEMENTS (2 M total index elements: the small layers of tests keep their routes).
# tools/gemm_gather_grouped_bench.py writes the table.  VPTQ_GEMM_GATHER_GROUPED=1 / 0 (with VPTQ_TUNING=1): every group of the
# kernel's format from 5 to 16 tokens / none.
#
# profiles/r31/table.md, profiles/r31/README.md (one MI355X, fp16 and bf16, q / k / v and gate / up of the 8B and 70B shapes = 3 M, 10 M,
# 14 M and 56 M total index elements, tokens 5 / 8 / 9 / 12 / 16, with one shared permutation and without; 240 cells, every member has
# the bits of its own entry in every one, 161 win; run-to-run spreads under 4 % in all but one cell):
#   q / k / v        every cell of the 8B shapes wins (with a permutation 0.28 - 0.60 of the parent, without 0.42 - 0.89), and of the 70B
#                    shapes in -0 / -256 (0.49 - 0.88); -65536 at 70B is level from 9 tokens without a permutation and at 16 with one
#   gate / up        8B shapes: -0 / -256 win by 4 - 18 % (not by the rule at 16 tokens in fp16 without a permutation), -65536 is
#                    level; 70B shapes (2 x 1792 row groups, 56 M elements): level with two launches (0.88 - 1.09, 7 of 60 cells
#                    win), -256 without a permutation at 5 - 8 tokens among them (0.88 - 0.90)
# A cell has a LEAST size only, so every region contains the 70B gate / up pair, and the one region that wins in every measured cell
# in both dtypes is v8-k65536-256 without a permutation at 5 - 8 tokens (0.54 - 0.90; parent: the members' gemv_gather launches), from
# the smallest measured group (3 M elements) up.  The q / k / v groups with a permutation - what published checkpoints have - win by
# far more but share their region with gate / up: routing them needs a cell that can say so (a most-elements or a member-count
# column), which this table does not have; until then the knob reaches them.
_GEMM_GATHER_GROUPED_CELLS = ((256, False, 3 << 20, 5, 8),)
GEMM_GATHER_GROUPED_MIN_TOKENS, GEMM_GATHER_GROUPED_MAX_TOKENS = 5, 16
GEMM_GATHER_GROUPED_MIN_ELEMENTS = 2 << 20
GEMM_GATHER_GROUPED_MAX_MEMBERS = 4
_GEMM_GATHER_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHER_GROUPED", "auto") or "auto").strip().lower()


def gemm_gather_grouped_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                              in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of sibling layers of this format (shared by its members) with these output widths take
    `vptq_quant_gemm_gather_grouped` for `tokens` tokens?  has_perm: True - every member has a column permutation, False - none,
    None - some.  Pure: no device, no library (whether the library serves the group is `vptq_quant_gemm_gather_grouped_supported`'s
    answer)."""
    if _GEMM_GATHER_GROUPED_MODE in ("0", "off") or not GEMM_GATHER_GROUPED_MIN_TOKENS <= tokens <= GEMM_GATHER_GROUPED_MAX_TOKENS:
        return False
    if not 2 <= len(out_features_tuple) <= GEMM_GATHER_GROUPED_MAX_MEMBERS or in_features % 8 or \
            _batched_decode_entry(vector_len, num_centroids, num_res_centroids) != "vptq_quant_gemm_gather":
        return False
    if _GEMM_GATHER_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + vector_len - 1) // vector_len for o in out_features_tuple) * in_features
    return any(kr == num_res_centroids and perm == has_perm and n_el >= max(min_el, GEMM_GATHER_GROUPED_MIN_ELEMENTS) and
               min_tok <= tokens <= max_tok for kr, perm, min_el, min_tok, max_tok in _GEMM_GATHER_GROUPED_CELLS)


def gemm_gather_grouped_tokens(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                               in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_GATHER_GROUPED_MIN_TOKENS, GEMM_GATHER_GROUPED_MAX_TOKENS + 1)
                 if gemm_gather_grouped_route(vector_len, num_centroids, num_res_centroids, out_features_tuple, in_features, t, has_perm))


# WHICH groups of the CANONICAL format (v = 8, 256 + 256 centroids) take `vptq_quant_gemm_k256_grouped` (gemm_k256.hip's grouped
# kernel: one persistent workgroup per CU over the members' row groups of 32 outputs as one list), 5 - 48 tokens (1 - 4 tokens are
# `SiblingGroup.forward`'s; 49 - 64 are not the kernel's).  The kernel has the reference's roundings only, so the CALLER asks every
# member's arithmetic (`exact_only` in the record below).  A cell is (has_perm, member count, least TOTAL index elements of the group
# = the sum of vector-rows x columns over its members, most total index elements or None, least tokens, most tokens); has_perm as
# above.  With a member count and a most size, a cell can route q / k / v without routing the 70B gate / up pair - what the gather
# table above cannot say.  Routed by the same rule: the grouped launch beats the SUM of what the members take without it by more than
# the larger of 5 % and three times the larger run-to-run spread, in every measured cell of the region, in both dtypes; the routed
# token counts of a group are one interval; no cell lies under GEMM_K256_GROUPED_MIN_ELEMENTS (2 M total index elements).
# tools/gemm_k256_grouped_bench.py writes the table.  VPTQ_GEMM_K256_GROUPED=1 / 0 (with VPTQ_TUNING=1): every group of the canonical
# format from 5 to 48 tokens / none.
#
# profiles/r32/table.md, profiles/r32/README.md (one MI355X, fp16 and bf16, q / k / v and gate / up of the 8B and 70B shapes = 3 M, 10 M,
# 14 M and 56 M total index elements, tokens 5 / 8 / 16 / 17 / 32 / 48, with one shared permutation and without; 96 cells, every member has
# the bits of its own entry in every one, 77 win; run-to-run spreads under 8 % in all but one cell, 11 %):
#   q / k / v        every cell wins: with a permutation 0.07 - 0.32 of the parent (three launches that gather x two bytes at a time),
#                    without 0.25 - 0.67 (k and v alone keep 32 of 256 CUs busy)
#   gate / up        with a permutation every cell wins (0.08 - 0.67); without one the 8B shapes are level (0.98 - 1.01, 0 of 12 cells) and
#                    the 70B shapes gain 6 - 12 %, by the rule in 5 of 12 cells
# A region reaches from its smallest to its largest MEASURED group (3 M ... 10 M for three members, 14 M ... 56 M for two) and no
# further: a q / k / v group above 10 M, a group of four and a pair without a permutation are behind the knob.
_GEMM_K256_GROUPED_CELLS = ((True, 3, 3 << 20, 10 << 20, 5, 48), (False, 3, 3 << 20, 10 << 20, 5, 48), (True, 2, 14 << 20, 56 << 20, 5, 48))
GEMM_K256_GROUPED_MIN_TOKENS, GEMM_K256_GROUPED_MAX_TOKENS = 5, 48
GEMM_K256_GROUPED_MIN_ELEMENTS = 2 << 20
GEMM_K256_GROUPED_MAX_MEMBERS = 4
_GEMM_K256_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_K256_GROUPED", "auto") or "auto").strip().lower()


def gemm_k256_grouped_route(out_features_tuple: Sequence[int], in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of canonical-format sibling layers with these output widths take `vptq_quant_gemm_k256_grouped` for `tokens`
    tokens?  has_perm: True - every member has a column permutation, False - none, None - some.  Pure: no device, no library (whether
    the library serves the group is `vptq_quant_gemm_k256_grouped_supported`'s answer, the arithmetic the caller's)."""
    if _GEMM_K256_GROUPED_MODE in ("0", "off") or not GEMM_K256_GROUPED_MIN_TOKENS <= tokens <= GEMM_K256_GROUPED_MAX_TOKENS:
        return False
    n = len(out_features_tuple)
    if not 2 <= n <= GEMM_K256_GROUPED_MAX_MEMBERS or in_features % 8:
        return False
    if _GEMM_K256_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + 7) // 8 for o in out_features_tuple) * in_features
    return any(perm == has_perm and members == n and n_el >= max(min_el, GEMM_K256_GROUPED_MIN_ELEMENTS) and
               (max_el is None or n_el <= max_el) and min_tok <= tokens <= max_tok
               for perm, members, min_el, max_el, min_tok, max_tok in _GEMM_K256_GROUPED_CELLS)


def gemm_k256_grouped_tokens(out_features_tuple: Sequence[int], in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_K256_GROUPED_MIN_TOKENS, GEMM_K256_GROUPED_MAX_TOKENS + 1)
                 if gemm_k256_grouped_route(out_features_tuple, in_features, t, has_perm))


# WHICH groups of the large-codebook formats take `vptq_quant_gemm_gatherw_grouped` (gemm_gatherw_grouped.hip: gemm_gatherw's pass
# behind gemm_gather_grouped's member walk), 17 - 48 tokens - the window beyond `vptq_quant_gemm_gather_grouped`'s.  Without it every
# member goes out alone from the 17th token on: gemm_gatherw, gemm_gather_px (a permute launch, then gemm_gatherw) or vptq_dequant + a
# dense GEMM, whichever `BATCHED_DECODE_ROUTES` gives a layer of its size.  A cell is the canonical group's plus the residual size:
# (residual centroids, has_perm, member count, least TOTAL index elements of the group = the sum of vector-rows x columns over its
# members, most total index elements or None, least tokens, most tokens); has_perm as above.  With the member count and the most size
# q / k / v can be routed without the gate / up pair.  Routed by the rule of the two tables above: the grouped launch beats the SUM
# of what the members take without it by more than the larger of 5 % and three times the larger run-to-run spread, in every measured
# cell of the region, in both dtypes; a region reaches from its smallest to its largest measured group and no further; the routed
# token counts of a group are one interval; no cell lies under GEMM_GATHERW_GROUPED_MIN_ELEMENTS (2 M total index elements).
# tools/gemm_gatherw_grouped_bench.py writes the table.  VPTQ_GEMM_GATHERW_GROUPED=1 / 0 (with VPTQ_TUNING=1): every group of the
# kernel's format from 17 to 48 tokens / none.
#
# profiles/r33/table.md, profiles/r33/README.md (one MI355X, fp16 and bf16, q / k / v and gate / up of the 8B and 70B shapes = 3 M, 10 M,
# 14 M and 56 M total index elements, tokens 17 / 24 / 32 / 40 / 48, with one shared permutation and without; 240 cells, every member has
# the bits of its own entry in every one, 141 win; run-to-run spreads under 3 % in all but two cells, 4.1 % the largest):
#   q / k / v        8B shapes (the parent: three dense routes): every cell wins, -0 / -256 0.38 - 0.64 of the parent, -65536 0.58 - 0.80.
#                    70B shapes: -0 / -256 with a permutation every cell (0.72 - 0.92), without one up to 40 tokens (0.76 - 0.90; level at
#                    48, 0.96 - 1.03); -65536 is level (0.95 - 1.02 with a permutation, 0.98 - 1.20 without)
#   gate / up        8B shapes with a permutation: -0 / -256 every cell (0.82 - 0.94), -65536 up to 32 tokens (0.90 - 0.94); without one
#                    -0 up to 40 tokens and -256 up to 32 (0.86 - 0.93), beyond them the parent's dense route is faster (1.08 - 1.25 at
#                    48), -65536 never (0.96 - 1.17).  70B shapes: level with two launches (0.94 - 1.04, 3 of 60 cells win)
# A region reaches from its smallest to its largest MEASURED group (3 M ... 10 M for three members, or one of the two alone; 14 M for
# two) and no further: a q / k / v group above 10 M, a group of four, a group of which only some members have a permutation and the
# 70B gate / up pair are behind the knob.
_GEMM_GATHERW_GROUPED_CELLS = (
    (0, True, 3, 3 << 20, 10 << 20, 17, 48), (0, False, 3, 3 << 20, 10 << 20, 17, 40), (0, False, 3, 3 << 20, 3 << 20, 17, 48),
    (256, True, 3, 3 << 20, 10 << 20, 17, 48), (256, False, 3, 3 << 20, 10 << 20, 17, 40), (256, False, 3, 3 << 20, 3 << 20, 17, 48),
    (65536, True, 3, 3 << 20, 3 << 20, 17, 48), (65536, False, 3, 3 << 20, 3 << 20, 17, 48),
    (0, True, 2, 14 << 20, 14 << 20, 17, 48), (0, False, 2, 14 << 20, 14 << 20, 17, 40),
    (256, True, 2, 14 << 20, 14 << 20, 17, 48), (256, False, 2, 14 << 20, 14 << 20, 17, 32),
    (65536, True, 2, 14 << 20, 14 << 20, 17, 32))
GEMM_GATHERW_GROUPED_MIN_TOKENS, GEMM_GATHERW_GROUPED_MAX_TOKENS = 17, 48
GEMM_GATHERW_GROUPED_MIN_ELEMENTS = 2 << 20
GEMM_GATHERW_GROUPED_MAX_MEMBERS = 4
_GEMM_GATHERW_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHERW_GROUPED", "auto") or "auto").strip().lower()


def gemm_gatherw_grouped_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                               in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of sibling layers of this format (shared by its members) with these output widths take
    `vptq_quant_gemm_gatherw_grouped` for `tokens` tokens?  has_perm: True - every member has a column permutation, False - none,
    None - some.  Pure: no device, no library (whether the library serves the group is `vptq_quant_gemm_gatherw_grouped_supported`'s
    answer)."""
    if _GEMM_GATHERW_GROUPED_MODE in ("0", "off") or not GEMM_GATHERW_GROUPED_MIN_TOKENS <= tokens <= GEMM_GATHERW_GROUPED_MAX_TOKENS:
        return False
    n = len(out_features_tuple)
    if not 2 <= n <= GEMM_GATHERW_GROUPED_MAX_MEMBERS or in_features % 8 or \
            _batched_decode_entry(vector_len, num_centroids, num_res_centroids) != "vptq_quant_gemm_gather":
        return False
    if _GEMM_GATHERW_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + vector_len - 1) // vector_len for o in out_features_tuple) * in_features
    return any(kr == num_res_centroids and perm == has_perm and members == n and
               n_el >= max(min_el, GEMM_GATHERW_GROUPED_MIN_ELEMENTS) and (max_el is None or n_el <= max_el) and
               min_tok <= tokens <= max_tok for kr, perm, members, min_el, max_el, min_tok, max_tok in _GEMM_GATHERW_GROUPED_CELLS)


def gemm_gatherw_grouped_tokens(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_GATHERW_GROUPED_MIN_TOKENS, GEMM_GATHERW_GROUPED_MAX_TOKENS + 1)
                 if gemm_gatherw_grouped_route(vector_len, num_centroids, num_res_centroids, out_features_tuple, in_features, t, has_perm))


# WHICH groups of the large-codebook formats `vptq_quant_gemm_gatherx` serves (vector length 8 / 16, 16384 ... 65536 main centroids, any
# residual codebook but gemm_gather's three formats: v16-k65536-65536 / -32768 / -1024 / -0, v8-k65536-4096, v8-k32768-0, ...) take
# `vptq_quant_gemm_gatherx_grouped` (gemm_gatherx_grouped.hip: gemm_gatherx's row-group body behind gemm_gather_grouped's member
# walk), 5 - 16 tokens (1 - 4 tokens are `SiblingGroup.forward` / `forward_sliced`'s; there is no wide kernel for these formats, so 17 -
# 48 tokens keep the members' routes).  Without it every member goes out alone: gemm_gatherx, gemm_gather_px (a permute launch, then
# gemm_gatherx), gemv_gatherx or vptq_dequant + a dense GEMM, whichever `BATCHED_DECODE_ROUTES` gives a layer of its format and size.
# A cell is the wide group's plus the format: (vector length, main centroids, residual centroids, has_perm, member count, least TOTAL
# index elements of the group = the sum of vector-rows x columns over its members, most total index elements or None, least tokens,
# most tokens); has_perm as above.  Routed by the rule of the tables above: the grouped launch beats the SUM of what the members take
# without it by more than the larger of 5 % and three times the larger run-to-run spread, in every measured cell of the region, in
# both dtypes; a region reaches from its smallest to its largest measured group and no further; the routed token counts of a group
# are one interval; no cell lies under GEMM_GATHERX_GROUPED_MIN_ELEMENTS (2 M total index elements).
# tools/gemm_gatherx_grouped_bench.py writes the table.  VPTQ_GEMM_GATHERX_GROUPED=1 / 0 (with VPTQ_TUNING=1): every group of the
# kernel's formats from 5 to 16 tokens / none.
#
# profiles/r34/table.md, profiles/r34/README.md (one MI355X, fp16 and bf16, q / k / v and gate / up of the 8B and 70B shapes = 1.5 M, 5 M,
# 7 M and 28 M total index elements for v = 16 and 3 M, 10 M, 14 M and 56 M for v = 8, tokens 5 / 8 / 9 / 12 / 16, with one shared
# permutation and without; 400 cells, every member has the bits of its own entry in every one, 316 win; run-to-run spreads under 1 %
# in 95 % of the cells, 6.8 % the largest):
#   q / k / v        every cell wins.  8B shapes 0.28 - 0.76 of the parent (one gemm_gatherx or gemm_gather_px launch plus two gemv_gatherx
#                    launches or two dense routes; v16-k65536-65536: three of them), 70B shapes 0.40 - 0.89 - but v16-k65536-65536
#                    without a permutation is level there from 9 tokens (0.99 - 1.07).  The 8B q / k / v of v = 16 (1.5 M elements)
#                    lies under the floor and keeps its routes
#   gate / up        8B shapes: v16-k65536-0 / -1024 with a permutation 0.22 - 0.46 (the parent is the in-kernel permuted gemm_gatherx:
#                    7 M elements of v = 16 are under px's floor), without 0.84 - 0.93; v8-k32768-0 and v8-k65536-4096 0.78 - 0.90 (-4096
#                    in fp16 without a permutation not by the rule at 12 tokens); v16-k65536-65536 0.57 - 0.82 with a permutation, without
#                    only at 5 - 8 tokens (0.74 - 0.75; 1.04 - 1.10 from 9: the dense routes are faster).  70B shapes: level with two
#                    launches (0.97 - 1.11) except v16-k65536-65536 (with a permutation 0.56 - 0.68; without 0.85 - 0.93 up to 12
#                    tokens) and v8-k65536-4096 in bf16 alone (0.88 - 0.90; fp16 0.98 - 1.00: not routed)
# A region reaches from its smallest to its largest MEASURED group of its member count (or is one of the two alone) and no further.
_GEMM_GATHERX_GROUPED_CELLS = (
    (16, 65536, 0, True, 3, 5 << 20, 5 << 20, 5, 16), (16, 65536, 0, False, 3, 5 << 20, 5 << 20, 5, 16),
    (16, 65536, 0, True, 2, 7 << 20, 7 << 20, 5, 16), (16, 65536, 0, False, 2, 7 << 20, 7 << 20, 5, 16),
    (16, 65536, 1024, True, 3, 5 << 20, 5 << 20, 5, 16), (16, 65536, 1024, False, 3, 5 << 20, 5 << 20, 5, 16),
    (16, 65536, 1024, True, 2, 7 << 20, 7 << 20, 5, 16), (16, 65536, 1024, False, 2, 7 << 20, 7 << 20, 5, 16),
    (16, 65536, 65536, True, 3, 5 << 20, 5 << 20, 5, 16), (16, 65536, 65536, False, 3, 5 << 20, 5 << 20, 5, 8),
    (16, 65536, 65536, True, 2, 7 << 20, 28 << 20, 5, 16), (16, 65536, 65536, False, 2, 7 << 20, 28 << 20, 5, 8),
    (16, 65536, 65536, False, 2, 28 << 20, 28 << 20, 5, 12),
    (8, 32768, 0, True, 3, 3 << 20, 10 << 20, 5, 16), (8, 32768, 0, False, 3, 3 << 20, 10 << 20, 5, 16),
    (8, 32768, 0, True, 2, 14 << 20, 14 << 20, 5, 16), (8, 32768, 0, False, 2, 14 << 20, 14 << 20, 5, 16),
    (8, 65536, 4096, True, 3, 3 << 20, 10 << 20, 5, 16), (8, 65536, 4096, False, 3, 3 << 20, 10 << 20, 5, 16),
    (8, 65536, 4096, True, 2, 14 << 20, 14 << 20, 5, 16), (8, 65536, 4096, False, 2, 14 << 20, 14 << 20, 5, 9))
GEMM_GATHERX_GROUPED_MIN_TOKENS, GEMM_GATHERX_GROUPED_MAX_TOKENS = 5, 16
GEMM_GATHERX_GROUPED_MIN_ELEMENTS = 2 << 20
GEMM_GATHERX_GROUPED_MAX_MEMBERS = 4
_GEMM_GATHERX_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHERX_GROUPED", "auto") or "auto").strip().lower()


def gemm_gatherx_grouped_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                               in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of sibling layers of this format (shared by its members) with these output widths take
    `vptq_quant_gemm_gatherx_grouped` for `tokens` tokens?  has_perm: True - every member has a column permutation, False - none,
    None - some.  Pure: no device, no library (whether the library serves the group is `vptq_quant_gemm_gatherx_grouped_supported`'s
    answer).  Never for the formats `gemm_gather_grouped_route` owns or the canonical format: a group has one route."""
    if _GEMM_GATHERX_GROUPED_MODE in ("0", "off") or not GEMM_GATHERX_GROUPED_MIN_TOKENS <= tokens <= GEMM_GATHERX_GROUPED_MAX_TOKENS:
        return False
    n = len(out_features_tuple)
    if not 2 <= n <= GEMM_GATHERX_GROUPED_MAX_MEMBERS or in_features % 8 or \
            _batched_decode_entry(vector_len, num_centroids, num_res_centroids) != "vptq_quant_gemm_gatherx":
        return False
    if _GEMM_GATHERX_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + vector_len - 1) // vector_len for o in out_features_tuple) * in_features
    return any((v, k, kr) == (vector_len, num_centroids, num_res_centroids) and perm == has_perm and members == n and
               n_el >= max(min_el, GEMM_GATHERX_GROUPED_MIN_ELEMENTS) and (max_el is None or n_el <= max_el) and
               min_tok <= tokens <= max_tok for v, k, kr, perm, members, min_el, max_el, min_tok, max_tok in _GEMM_GATHERX_GROUPED_CELLS)


def gemm_gatherx_grouped_tokens(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_GATHERX_GROUPED_MIN_TOKENS, GEMM_GATHERX_GROUPED_MAX_TOKENS + 1)
                 if gemm_gatherx_grouped_route(vector_len, num_centroids, num_res_centroids, out_features_tuple, in_features, t, has_perm))


class GroupedDecodeRoute(NamedTuple):
    """what differs between the group routes; everything else is one code path in `SiblingGroup` (a third route is a record and a
    route function).  `route` and `tokens` take the group's static configuration as `SiblingGroup._batched_static` states it:
    (vector length, main centroids, residual centroids, output widths, input width, has_perm)."""
    entry: str                                # the library entry (+ "_supported", "_workspace_bytes"); ops.<entry without "vptq_"> launches it
    owns: Callable[[int, int, int], bool]     # (vector length, main centroids, residual centroids): is the format this route's?
    route: Callable[..., bool]                # (v, k, kr, output widths, input width, tokens, has_perm)
    tokens: Callable[..., tuple]              # (v, k, kr, output widths, input width, has_perm): the routed token counts, ascending
    min_tokens: int                           # the token window of the route
    max_tokens: int
    off_flags: int                            # launch flags that switch the route off
    exact_only: bool = False                  # the kernel has the reference's roundings only: every member's arithmetic must be GEMV_EXACT


# (the formats are disjoint: a group has at most one route, and the order changes no answer)
GROUPED_DECODE_ROUTES = (
    GroupedDecodeRoute("vptq_quant_gemm_gather_grouped", lambda v, k, kr: _batched_decode_entry(v, k, kr) == "vptq_quant_gemm_gather",
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_gather_grouped_route(v, k, kr, outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_gather_grouped_tokens(v, k, kr, outs, width, has_perm),
                       GEMM_GATHER_GROUPED_MIN_TOKENS, GEMM_GATHER_GROUPED_MAX_TOKENS, B.GEMV_FORCE_GENERIC),
    GroupedDecodeRoute("vptq_quant_gemm_k256_grouped", lambda v, k, kr: (v, k, kr) == (8, 256, 256),
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_k256_grouped_route(outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_k256_grouped_tokens(outs, width, has_perm),
                       GEMM_K256_GROUPED_MIN_TOKENS, GEMM_K256_GROUPED_MAX_TOKENS, B.GEMV_FORCE_ANY, exact_only=True),
)
GROUPED_DECODE_MIN_TOKENS = min(r.min_tokens for r in GROUPED_DECODE_ROUTES)   # the union of the windows: what a caller guards with
GROUPED_DECODE_MAX_TOKENS = max(r.max_tokens for r in GROUPED_DECODE_ROUTES)


def grouped_decode_route(vector_len: int, num_centroids: int, num_res_centroids: int) -> Optional[GroupedDecodeRoute]:
    """the group route whose kernel has this format, or None.  No knob is read."""
    for r in GROUPED_DECODE_ROUTES:
        if r.owns(vector_len, num_centroids, num_res_centroids):
            return r
    return None


# a format's routes BEYOND its first window, in window order: the large-codebook formats' 17 - 48 tokens behind
# `vptq_quant_gemm_gather_grouped`'s 5 - 16.  The windows of one format are disjoint, so a token count has at most one record.
GROUPED_DECODE_WIDE_ROUTES = (
    GroupedDecodeRoute("vptq_quant_gemm_gatherw_grouped", lambda v, k, kr: _batched_decode_entry(v, k, kr) == "vptq_quant_gemm_gather",
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_gatherw_grouped_route(v, k, kr, outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_gatherw_grouped_tokens(v, k, kr, outs, width, has_perm),
                       GEMM_GATHERW_GROUPED_MIN_TOKENS, GEMM_GATHERW_GROUPED_MAX_TOKENS, B.GEMV_FORCE_GENERIC),
)


def grouped_decode_routes(vector_len: int, num_centroids: int, num_res_centroids: int) -> tuple:
    """every group route whose kernel has this format, in window order: the owner of `GROUPED_DECODE_ROUTES`, then the records of
    `GROUPED_DECODE_WIDE_ROUTES` (possibly none at all).  No knob is read."""
    first = grouped_decode_route(vector_len, num_centroids, num_res_centroids)
    if first is None:
        return ()
    return (first,) + tuple(r for r in GROUPED_DECODE_WIDE_ROUTES if r.owns(vector_len, num_centroids, num_res_centroids))


# the routes of formats `GROUPED_DECODE_ROUTES` has no owner for: gemm_gatherx's formats, 5 - 16 tokens.  (A table of its own: the two
# tables above and their readers keep every answer they gave before these formats had a group route.)  The window lies inside
# GROUPED_DECODE_MIN_TOKENS ... GROUPED_DECODE_MAX_TOKENS, the guard callers already apply.
GROUPED_DECODE_X_ROUTES = (
    GroupedDecodeRoute("vptq_quant_gemm_gatherx_grouped", lambda v, k, kr: _batched_decode_entry(v, k, kr) == "vptq_quant_gemm_gatherx",
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_gatherx_grouped_route(v, k, kr, outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_gatherx_grouped_tokens(v, k, kr, outs, width, has_perm),
                       GEMM_GATHERX_GROUPED_MIN_TOKENS, GEMM_GATHERX_GROUPED_MAX_TOKENS, B.GEMV_FORCE_GENERIC),
)


def sibling_decode_routes(vector_len: int, num_centroids: int, num_res_centroids: int) -> tuple:
    """every group route a `SiblingGroup` of this format can take, in window order: `grouped_decode_routes` where that is non-empty,
    else the records of `GROUPED_DECODE_X_ROUTES` that own the format (possibly none at all).  The formats of the tables are
    disjoint.  No knob is read."""
    routes = grouped_decode_routes(vector_len, num_centroids, num_res_centroids)
    if routes:
        return routes
    return tuple(r for r in GROUPED_DECODE_X_ROUTES if r.owns(vector_len, num_centroids, num_res_centroids))
