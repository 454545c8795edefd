"""The batched-decode route of a GROUP of sibling layers (q / k / v, gate / up): which (format, shapes, token count) take
`vptq_quant_gemm_gather_grouped` - the members' row groups as one list in ONE launch, one x gather per distinct permutation - in
place of one launch (and one x gather) per member.

Pure rules - no device, no tensors, in the style of vptq_amd/batched_decode.py: one route function, its knob and its measured
cells.  This route is a group's, not a layer's: `BATCHED_DECODE_ROUTES` and the layers' cell tables do not know it, and a group that
is not routed here leaves every member on the routes it had.  `SiblingGroup.forward_batched` (vptq_amd/layers/vqlinear.py) and
`prepare_model` decide through it.
"""
from __future__ import annotations

from typing import Optional, Sequence

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
