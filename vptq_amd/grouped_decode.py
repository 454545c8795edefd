"""The batched-decode route of a GROUP of sibling layers (q / k / v, gate / up): which (format, shapes, token count) take
`vptq_quant_gemm_gather_grouped` - the members' row groups as one list in ONE launch, one x gather per distinct permutation - in
place of one launch (and one x gather) per member; for the canonical format, `vptq_quant_gemm_k256_grouped`; for 17 - 48 tokens of
the large-codebook formats, `vptq_quant_gemm_gatherw_grouped`; for 5 - 16 tokens of the other large-codebook formats (gemm_gatherx's),
`vptq_quant_gemm_gatherx_grouped`, and for their 17 - 48 tokens `vptq_quant_gemm_gatherxw_grouped`.

Pure rules - no device, no tensors, in the style of vptq_amd/batched_decode.py: per route one route function, its knob and its
measured cells, and `GROUPED_DECODE_ROUTES`, the ordered record of the group routes (`GROUPED_DECODE_WIDE_ROUTES`: a format's routes
beyond its first window; `GROUPED_DECODE_X_ROUTES`: the routes of formats the first table has no owner for; `sibling_decode_routes`
reads all three; `GROUPED_DECODE_X_WIDE_ROUTES`: those formats' routes beyond their first window, read behind the others by
`sibling_group_routes`; `GROUPED_DECODE_V12_ROUTES`: the v = 12 formats' `vptq_quant_gemm_gather12_grouped`, 5 - 16 tokens, read behind
all of them by `sibling_group_v12_routes`; `GROUPED_DECODE_V12_WIDE_ROUTES`: their `vptq_quant_gemm_gather12w_grouped`, 17 - 48 tokens, read
behind that by `sibling_group_v12_wide_routes`).  These routes are a group's, not a layer's: `BATCHED_DECODE_ROUTES` and the layers' cell tables do not know it, and a group that
is not routed here leaves every member on the routes it had.  `SiblingGroup.forward_batched` (vptq_amd/layers/vqlinear.py) and
`prepare_model` decide through it.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence

from vptq_amd import _backend as B
from vptq_amd.batched_decode import _batched_decode_entry, _v12_owns

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
# walk), 5 - 16 tokens (1 - 4 tokens are `SiblingGroup.forward` / `forward_sliced`'s; 17 -
# 48 tokens are `vptq_quant_gemm_gatherxw_grouped`'s, below).  Without it every member goes out alone: gemm_gatherx, gemm_gather_px (a permute launch, then
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


# WHICH groups of `vptq_quant_gemm_gatherx`'s formats take `vptq_quant_gemm_gatherxw_grouped` (gemm_gatherxw_grouped.hip: gemm_gatherxw's
# token-block pass behind gemm_gatherx_grouped's member walk), 17 - 48 tokens - the window beyond `vptq_quant_gemm_gatherx_grouped`'s.
# Without it every member goes out alone from the 17th token on: gemm_gatherxw (behind a permute launch of its own when permuted) or
# vptq_dequant + a dense GEMM, whichever `BATCHED_DECODE_WIDE_ROUTES` gives a layer of its format and size.  A cell has
# `_GEMM_GATHERX_GROUPED_CELLS`' format: (vector length, main centroids, residual centroids, has_perm, member count, least TOTAL index
# elements of the group, most total index elements or None, least tokens, most tokens).  Routed by the rule of the tables above: the
# grouped launch beats the SUM of what the members take without it by more than the larger of 5 % and three times the larger
# run-to-run spread, in every measured cell of the region, in both dtypes; a region reaches from its smallest to its largest measured
# group and no further; the routed token counts of a group are one interval; no cell lies under GEMM_GATHERXW_GROUPED_MIN_ELEMENTS (2 M
# total index elements).  tools/gemm_gatherx_grouped_bench.py --entry gatherxw writes the table.  VPTQ_GEMM_GATHERXW_GROUPED=1 / 0 (with
# VPTQ_TUNING=1): every group of the kernel's formats from 17 to 48 tokens / none.
#
# profiles/r36/table.md, profiles/r36/README.md (one MI355X, fp16 and bf16, the five formats of profiles/r34, q / k / v and gate / up of the
# 8B and 70B shapes = 1.5 M, 5 M, 7 M and 28 M total index elements for v = 16 and 3 M, 10 M, 14 M and 56 M for v = 8, tokens 17 / 24 / 32 /
# 33 / 40 / 48, with one shared permutation and without; 480 cells, every member has the bits of its own entry in every one, 275 win;
# run-to-run spreads under 1.3 % in 95 % of the cells, 3.6 % the largest):
#   q / k / v        8B shapes (the parent: three dense routes): every cell wins, 0.41 - 0.80 of the parent (v16-k65536-65536 0.67 - 0.94).
#                    The 8B q / k / v of v = 16 (1.5 M elements) lies under the floor and keeps its routes.  70B shapes (the parent: one
#                    gemm_gatherxw launch and two dense routes): with a permutation 0.77 - 0.95 up to 40 tokens (v16-k65536-1024 and
#                    v8-k32768-0 up to 48), without one 0.78 - 0.91 up to 24 tokens (v16-k65536-1024 up to 32, v8-k32768-0 up to 40), level or
#                    slower beyond; v16-k65536-65536 never (0.96 - 1.36)
#   gate / up        8B shapes: with a permutation v16-k65536-1024 and v8-k65536-4096 in every cell (0.62 - 0.94), v8-k32768-0 up to 40
#                    tokens, v16-k65536-65536 up to 32, v16-k65536-0 up to 24 (0.75 - 0.85); without one 17 - 24 tokens only (0.77 - 0.93; the
#                    dense routes are faster from 32, up to 1.34) and v16-k65536-65536 never (1.09 - 1.42).  70B shapes: level with two
#                    launches (0.85 - 1.20); in both dtypes only v16-k65536-1024 with a permutation wins by the rule, at 17 - 24 tokens (0.93 - 0.94)
# A region reaches from its smallest to its largest MEASURED group of its member count (or is one of the two alone) and no further.
_GEMM_GATHERXW_GROUPED_CELLS = (
    (16, 65536, 0, True, 3, 5 << 20, 5 << 20, 17, 40), (16, 65536, 0, False, 3, 5 << 20, 5 << 20, 17, 24),
    (16, 65536, 0, True, 2, 7 << 20, 7 << 20, 17, 24), (16, 65536, 0, False, 2, 7 << 20, 7 << 20, 17, 24),
    (16, 65536, 1024, True, 3, 5 << 20, 5 << 20, 17, 48), (16, 65536, 1024, False, 3, 5 << 20, 5 << 20, 17, 32),
    (16, 65536, 1024, True, 2, 7 << 20, 28 << 20, 17, 24), (16, 65536, 1024, True, 2, 7 << 20, 7 << 20, 17, 48),
    (16, 65536, 1024, False, 2, 7 << 20, 7 << 20, 17, 24),
    (16, 65536, 65536, True, 2, 7 << 20, 7 << 20, 17, 32),
    (8, 32768, 0, True, 3, 3 << 20, 10 << 20, 17, 48), (8, 32768, 0, False, 3, 3 << 20, 10 << 20, 17, 40), (8, 32768, 0, False, 3, 3 << 20, 3 << 20, 17, 48),
    (8, 32768, 0, True, 2, 14 << 20, 14 << 20, 17, 40), (8, 32768, 0, False, 2, 14 << 20, 14 << 20, 17, 24),
    (8, 65536, 4096, True, 3, 3 << 20, 10 << 20, 17, 40), (8, 65536, 4096, True, 3, 3 << 20, 3 << 20, 17, 48),
    (8, 65536, 4096, False, 3, 3 << 20, 10 << 20, 17, 24), (8, 65536, 4096, False, 3, 3 << 20, 3 << 20, 17, 48),
    (8, 65536, 4096, True, 2, 14 << 20, 14 << 20, 17, 48), (8, 65536, 4096, False, 2, 14 << 20, 14 << 20, 17, 24))
GEMM_GATHERXW_GROUPED_MIN_TOKENS, GEMM_GATHERXW_GROUPED_MAX_TOKENS = 17, 48
GEMM_GATHERXW_GROUPED_MIN_ELEMENTS = 2 << 20
GEMM_GATHERXW_GROUPED_MAX_MEMBERS = 4
_GEMM_GATHERXW_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHERXW_GROUPED", "auto") or "auto").strip().lower()


def gemm_gatherxw_grouped_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of sibling layers of this format (shared by its members) with these output widths take
    `vptq_quant_gemm_gatherxw_grouped` for `tokens` tokens?  has_perm: True - every member has a column permutation, False - none,
    None - some.  Pure: no device, no library (whether the library serves the group is `vptq_quant_gemm_gatherxw_grouped_supported`'s
    answer).  Only for the formats `gemm_gatherx_grouped_route` owns: a group has one route per window."""
    if _GEMM_GATHERXW_GROUPED_MODE in ("0", "off") or not GEMM_GATHERXW_GROUPED_MIN_TOKENS <= tokens <= GEMM_GATHERXW_GROUPED_MAX_TOKENS:
        return False
    n = len(out_features_tuple)
    if not 2 <= n <= GEMM_GATHERXW_GROUPED_MAX_MEMBERS or in_features % 8 or \
            _batched_decode_entry(vector_len, num_centroids, num_res_centroids) != "vptq_quant_gemm_gatherx":
        return False
    if _GEMM_GATHERXW_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + vector_len - 1) // vector_len for o in out_features_tuple) * in_features
    return any((v, k, kr) == (vector_len, num_centroids, num_res_centroids) and perm == has_perm and members == n and
               n_el >= max(min_el, GEMM_GATHERXW_GROUPED_MIN_ELEMENTS) and (max_el is None or n_el <= max_el) and
               min_tok <= tokens <= max_tok for v, k, kr, perm, members, min_el, max_el, min_tok, max_tok in _GEMM_GATHERXW_GROUPED_CELLS)


def gemm_gatherxw_grouped_tokens(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                 in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_GATHERXW_GROUPED_MIN_TOKENS, GEMM_GATHERXW_GROUPED_MAX_TOKENS + 1)
                 if gemm_gatherxw_grouped_route(vector_len, num_centroids, num_res_centroids, out_features_tuple, in_features, t, has_perm))


# WHICH groups of the large-codebook formats of VECTOR LENGTH 12 (`vptq_quant_gemm_gather12`'s: v12-k65536-4096 / -256 / -0, `_v12_owns` of
# vptq_amd/batched_decode.py) take `vptq_quant_gemm_gather12_grouped` (gemm_gather12_grouped.hip: gemm_gather12c's (row group, column
# part) items of every member as one list, one sum launch for the group where the columns are split), 5 - 16 tokens (1 - 4 tokens are
# `SiblingGroup.forward` / `forward_sliced`'s; 17 - 48 tokens are `vptq_quant_gemm_gather12w_grouped`'s, below).  Without it every member goes out alone: gemm_gather12,
# gemm_gather12c, two gemv_gatherx launches or vptq_dequant + a dense GEMM, whichever `BATCHED_DECODE_V12_ROUTES` /
# `BATCHED_DECODE_V12_COLUMN_ROUTES` give a layer of its format and size, each behind an x gather of its own when permuted.  A cell has
# `_GEMM_GATHERXW_GROUPED_CELLS`' format without the vector length: (main centroids, residual centroids, has_perm, member count, least
# TOTAL index elements of the group, most total index elements or None, least tokens, most tokens).  Routed by the rule of the tables
# above: the grouped launch beats the SUM of what the members take without it by more than the larger of 5 % and three times the
# larger run-to-run spread, in every measured cell of the region, in both dtypes; no cell lies under
# GEMM_GATHER12_GROUPED_MIN_ELEMENTS (1 M total index elements: gemm_gather12c's floor).  tools/gemm_gather12_grouped_bench.py writes the
# table.  VPTQ_GEMM_GATHER12_GROUPED=1 / 0 (with VPTQ_TUNING=1): every group of the kernel's formats from 5 to 16 tokens / none.
#
# profiles/r40/table.md, profiles/r40/README.md (one MI355X, fp16 and bf16, v12-k65536-4096 / -256 / -0, q / k / v and gate / up of the 8B and
# 70B shapes = 2.0 M, 6.7 M, 9.3 M and 37.3 M total index elements, tokens 5 / 8 / 16, parts = 0, with one shared permutation and without; 144
# cells, every member has the bits of its own entry in every one, ALL win by the rule; run-to-run spreads at most 2 %):
#   q / k / v        8B shapes (1040 items of one tile; the parent: gemm_gather12c for q, two gemv_gatherx launches each for k / v up to 8
#                    tokens and two dense routes from 9) 0.35 - 0.61 of the parent - v12-k65536-4096 fp16 with a permutation, 5 / 8 / 16
#                    tokens: 42.2 / 42.5 / 43.2 us against 92.2 / 100.5 / 77.8; 70B shapes (4 parts of 4 tiles) 0.41 - 0.90, the closest at 16
#                    tokens without a permutation (v12-k65536-4096: 0.90)
#   gate / up        8B shapes (two gemm_gather12c calls: four launches; here 2 parts, two launches) 0.86 - 0.95; 70B shapes (two
#                    gemm_gather12 launches; here one part, one launch) 0.84 - 0.91
# A region reaches from its smallest to its largest MEASURED group of its member count and no further: a group of four, a group of
# which only some members have a permutation, v12-k32768-1024 and q / k / v groups above 7 M elements are behind the knob.
_GEMM_GATHER12_GROUPED_CELLS = tuple((65536, kr, perm, members, min_el, max_el, 5, 16) for kr in (0, 256, 4096) for perm in (True, False)
                                     for members, min_el, max_el in ((3, 2 << 20, 7 << 20), (2, 9 << 20, 38 << 20)))
GEMM_GATHER12_GROUPED_MIN_TOKENS, GEMM_GATHER12_GROUPED_MAX_TOKENS = 5, 16
GEMM_GATHER12_GROUPED_MIN_ELEMENTS = 1 << 20
GEMM_GATHER12_GROUPED_MAX_MEMBERS = 4
_GEMM_GATHER12_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHER12_GROUPED", "auto") or "auto").strip().lower()


def gemm_gather12_grouped_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of sibling layers of this format (shared by its members) with these output widths take
    `vptq_quant_gemm_gather12_grouped` (parts = 0: the library's rule) for `tokens` tokens?  has_perm: True - every member has a
    column permutation, False - none, None - some.  Pure: no device, no library (whether the library serves the group is
    `vptq_quant_gemm_gather12_grouped_supported`'s answer).  Only for the v = 12 formats, which no other group route owns."""
    if _GEMM_GATHER12_GROUPED_MODE in ("0", "off") or not GEMM_GATHER12_GROUPED_MIN_TOKENS <= tokens <= GEMM_GATHER12_GROUPED_MAX_TOKENS:
        return False
    n = len(out_features_tuple)
    if not 2 <= n <= GEMM_GATHER12_GROUPED_MAX_MEMBERS or in_features % 8 or not _v12_owns(vector_len, num_centroids, num_res_centroids):
        return False
    if _GEMM_GATHER12_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + vector_len - 1) // vector_len for o in out_features_tuple) * in_features
    return any((k, kr) == (num_centroids, num_res_centroids) and perm == has_perm and members == n and
               n_el >= max(min_el, GEMM_GATHER12_GROUPED_MIN_ELEMENTS) and (max_el is None or n_el <= max_el) and
               min_tok <= tokens <= max_tok for k, kr, perm, members, min_el, max_el, min_tok, max_tok in _GEMM_GATHER12_GROUPED_CELLS)


def gemm_gather12_grouped_tokens(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                 in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_GATHER12_GROUPED_MIN_TOKENS, GEMM_GATHER12_GROUPED_MAX_TOKENS + 1)
                 if gemm_gather12_grouped_route(vector_len, num_centroids, num_res_centroids, out_features_tuple, in_features, t, has_perm))


# WHICH groups of the v = 12 formats take `vptq_quant_gemm_gather12w_grouped` (gemm_gather12w_grouped.hip: gemm_gather12w's token-block
# pass behind gemm_gather12_grouped's member walk), 17 - 48 tokens - the window beyond `vptq_quant_gemm_gather12_grouped`'s.  Without it
# every member goes out alone from the 17th token on: vptq_dequant + a dense GEMM or, behind its knob, gemm_gather12w (one to two
# launches and an x gather per member), whichever `BATCHED_DECODE_V12_WIDE_ROUTES` gives a layer of its format and size.  A cell has
# `_GEMM_GATHER12_GROUPED_CELLS`' format: (main centroids, residual centroids, has_perm, member count, least TOTAL index elements of the
# group, most total index elements or None, least tokens, most tokens).  Routed by the rule of the tables above: the grouped launch
# beats the SUM of what the members take without it by more than the larger of 5 % and three times the larger run-to-run spread, in
# every measured cell of the region, in both dtypes; a region reaches from its smallest to its largest measured group of its member
# count and no further; no cell lies under GEMM_GATHER12W_GROUPED_MIN_ELEMENTS (1 M total index elements).
# tools/gemm_gather12_grouped_bench.py --wide writes the table.  VPTQ_GEMM_GATHER12W_GROUPED=1 / 0 (with VPTQ_TUNING=1): every group of
# the kernel's formats from 17 to 48 tokens / none.
#
# profiles/r41/table.md, profiles/r41/README.md (one MI355X, fp16 and bf16, v12-k65536-4096 / -256 / -0, q / k / v and gate / up of the 8B and
# 70B shapes = 2.0 M, 6.7 M, 9.3 M and 37.3 M total index elements, tokens 17 / 24 / 32 / 33 / 40 / 48, parts = 0, with one shared permutation
# and without; 288 cells, every member has the bits of its own entry in every one, 266 win; run-to-run spreads at most 2.4 %; the
# parent is the members' dense routes):
#   17 - 32 tokens   all 144 cells win: 8B q / k / v 0.41 - 0.61 of the parent, 70B q / k / v 0.48 - 0.87, 8B gate / up 0.52 - 0.89, 70B gate / up
#                    0.37 - 0.78
#   33 - 48 tokens   v12-k65536-0 wins everywhere (0.41 - 0.77); with a residual table the kernel runs at ONE workgroup per CU: with a
#                    permutation 0.48 - 0.86 except the 8B gate / up pair of -4096 in bf16 (0.96 - 1.00); without one the 8B gate / up pair
#                    is level or slower (0.95 - 1.27) and bf16 does not win on the 70B q / k / v (0.96 - 1.15)
# NO CELL IS SHIPPED YET: the regions that win in every measured cell are listed in profiles/r41/README.md, but the suites were not run
# with them in place, so the tuple is empty and the entry is reached by the knob (and `ops.quant_gemm_gather12w_grouped`) alone.
_GEMM_GATHER12W_GROUPED_CELLS = ()
GEMM_GATHER12W_GROUPED_MIN_TOKENS, GEMM_GATHER12W_GROUPED_MAX_TOKENS = 17, 48
GEMM_GATHER12W_GROUPED_MIN_ELEMENTS = 1 << 20
GEMM_GATHER12W_GROUPED_MAX_MEMBERS = 4
_GEMM_GATHER12W_GROUPED_MODE = (B.tune_env("VPTQ_GEMM_GATHER12W_GROUPED", "auto") or "auto").strip().lower()


def gemm_gather12w_grouped_route(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                 in_features: int, tokens: int, has_perm: Optional[bool]) -> bool:
    """does a group of sibling layers of this format (shared by its members) with these output widths take
    `vptq_quant_gemm_gather12w_grouped` (parts = 0: the library's rule) for `tokens` tokens?  has_perm: True - every member has a
    column permutation, False - none, None - some.  Pure: no device, no library (whether the library serves the group is
    `vptq_quant_gemm_gather12w_grouped_supported`'s answer).  Only for the v = 12 formats: a group has one route per window."""
    if _GEMM_GATHER12W_GROUPED_MODE in ("0", "off") or not GEMM_GATHER12W_GROUPED_MIN_TOKENS <= tokens <= GEMM_GATHER12W_GROUPED_MAX_TOKENS:
        return False
    n = len(out_features_tuple)
    if not 2 <= n <= GEMM_GATHER12W_GROUPED_MAX_MEMBERS or in_features % 8 or not _v12_owns(vector_len, num_centroids, num_res_centroids):
        return False
    if _GEMM_GATHER12W_GROUPED_MODE in ("1", "on"):
        return True
    if has_perm is None:
        return False
    n_el = sum((o + vector_len - 1) // vector_len for o in out_features_tuple) * in_features
    return any((k, kr) == (num_centroids, num_res_centroids) and perm == has_perm and members == n and
               n_el >= max(min_el, GEMM_GATHER12W_GROUPED_MIN_ELEMENTS) and (max_el is None or n_el <= max_el) and
               min_tok <= tokens <= max_tok for k, kr, perm, members, min_el, max_el, min_tok, max_tok in _GEMM_GATHER12W_GROUPED_CELLS)


def gemm_gather12w_grouped_tokens(vector_len: int, num_centroids: int, num_res_centroids: int, out_features_tuple: Sequence[int],
                                  in_features: int, has_perm: Optional[bool]) -> tuple:
    """the token counts the route function gives to the grouped launch for this group, ascending (possibly none): `prepare_model`
    sizes the stream's workspace to the largest"""
    return tuple(t for t in range(GEMM_GATHER12W_GROUPED_MIN_TOKENS, GEMM_GATHER12W_GROUPED_MAX_TOKENS + 1)
                 if gemm_gather12w_grouped_route(vector_len, num_centroids, num_res_centroids, out_features_tuple, in_features, t, has_perm))


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
    extra: tuple = ()                         # integer arguments the entry takes behind the tokens (`_supported`, `_workspace_bytes`) / the output widths (the op)


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


# the routes of `GROUPED_DECODE_X_ROUTES`' formats BEYOND their first window, in window order: gemm_gatherx's formats, 17 - 48 tokens
# behind `vptq_quant_gemm_gatherx_grouped`'s 5 - 16.  (Again a table of its own: the three tables above and their readers keep every
# answer they gave before.)  The window lies inside GROUPED_DECODE_MIN_TOKENS ... GROUPED_DECODE_MAX_TOKENS.
GROUPED_DECODE_X_WIDE_ROUTES = (
    GroupedDecodeRoute("vptq_quant_gemm_gatherxw_grouped", lambda v, k, kr: _batched_decode_entry(v, k, kr) == "vptq_quant_gemm_gatherx",
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_gatherxw_grouped_route(v, k, kr, outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_gatherxw_grouped_tokens(v, k, kr, outs, width, has_perm),
                       GEMM_GATHERXW_GROUPED_MIN_TOKENS, GEMM_GATHERXW_GROUPED_MAX_TOKENS, B.GEMV_FORCE_GENERIC),
)


def sibling_group_routes(vector_len: int, num_centroids: int, num_res_centroids: int) -> tuple:
    """every group route a `SiblingGroup` of this format can take, in window order: `sibling_decode_routes`' answer, then the records
    of `GROUPED_DECODE_X_WIDE_ROUTES` that own the format (none for any format but gemm_gatherx's).  What `SiblingGroup` reads.  No
    knob is read."""
    return sibling_decode_routes(vector_len, num_centroids, num_res_centroids) + \
        tuple(r for r in GROUPED_DECODE_X_WIDE_ROUTES if r.owns(vector_len, num_centroids, num_res_centroids))


# the routes of the v = 12 formats, which none of the four tables above has an owner for: `vptq_quant_gemm_gather12_grouped`, 5 - 16
# tokens.  (Once more a table and a reader of its own: the four tables above and their four readers keep every answer they gave
# before.)  extra = (0,): `parts` = the library's rule.  The window lies inside GROUPED_DECODE_MIN_TOKENS ... GROUPED_DECODE_MAX_TOKENS.
GROUPED_DECODE_V12_ROUTES = (
    GroupedDecodeRoute("vptq_quant_gemm_gather12_grouped", _v12_owns,
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_gather12_grouped_route(v, k, kr, outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_gather12_grouped_tokens(v, k, kr, outs, width, has_perm),
                       GEMM_GATHER12_GROUPED_MIN_TOKENS, GEMM_GATHER12_GROUPED_MAX_TOKENS, B.GEMV_FORCE_GENERIC, extra=(0,)),
)


def sibling_group_v12_routes(vector_len: int, num_centroids: int, num_res_centroids: int) -> tuple:
    """every group route a `SiblingGroup` of this format can take, in window order: `sibling_group_routes`' answer, then the records of
    `GROUPED_DECODE_V12_ROUTES` that own the format (none for any format but the v = 12 ones, for which the first part is empty).
    What `SiblingGroup` reads.  No knob is read."""
    return sibling_group_routes(vector_len, num_centroids, num_res_centroids) + \
        tuple(r for r in GROUPED_DECODE_V12_ROUTES if r.owns(vector_len, num_centroids, num_res_centroids))


# the v = 12 formats' route BEYOND their first window: `vptq_quant_gemm_gather12w_grouped`, 17 - 48 tokens behind
# `vptq_quant_gemm_gather12_grouped`'s 5 - 16.  (A table and a reader of its own: the five tables above and their five readers keep every
# answer they gave before.)  extra = (0,): `parts` = the library's rule.  The window lies inside GROUPED_DECODE_MIN_TOKENS ...
# GROUPED_DECODE_MAX_TOKENS.
GROUPED_DECODE_V12_WIDE_ROUTES = (
    GroupedDecodeRoute("vptq_quant_gemm_gather12w_grouped", _v12_owns,
                       lambda v, k, kr, outs, width, tokens, has_perm: gemm_gather12w_grouped_route(v, k, kr, outs, width, tokens, has_perm),
                       lambda v, k, kr, outs, width, has_perm: gemm_gather12w_grouped_tokens(v, k, kr, outs, width, has_perm),
                       GEMM_GATHER12W_GROUPED_MIN_TOKENS, GEMM_GATHER12W_GROUPED_MAX_TOKENS, B.GEMV_FORCE_GENERIC, extra=(0,)),
)


def sibling_group_v12_wide_routes(vector_len: int, num_centroids: int, num_res_centroids: int) -> tuple:
    """every group route a `SiblingGroup` of this format can take, in window order: `sibling_group_v12_routes`' answer, then the records
    of `GROUPED_DECODE_V12_WIDE_ROUTES` that own the format (none for any format but the v = 12 ones).  What `SiblingGroup` reads.  No
    knob is read."""
    return sibling_group_v12_routes(vector_len, num_centroids, num_res_centroids) + \
        tuple(r for r in GROUPED_DECODE_V12_WIDE_ROUTES if r.owns(vector_len, num_centroids, num_res_centroids))
