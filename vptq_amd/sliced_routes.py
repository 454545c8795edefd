"""The sliced-layout routes (1 - 4 tokens over the load-time derived "sliced" layouts of the large-codebook formats): which layer gets
which kind of layout, and which token counts it then serves how.

Pure rules - no device, no tensors, no library call: functions of plain int / bool / str values with their knobs and measured tables.
`VQuantLinear` (vptq_amd/layers/vqlinear.py) gathers the values - the layer's format and shape, the layout's slices, the library's
answers - and reads the rules through this module; the knobs that tests and tools assign to (`_SLICED_ONE_LAUNCH`, `_SLICED_TOKENS_ENV`,
`_DEQUANT_SLICED_MODE`) are read here at call time and are not re-exported (an alias would keep the old value).
"""
import os

from vptq_amd import _backend as B


_KNOB_OFF = ("0", "off", "false", "no")             # what VPTQ_SLICED_LAYOUT and VPTQ_SLICED_ONE_LAUNCH accept as "never" ...
_KNOB_ON = ("1", "on", "true", "yes", "always")     # ... and as "always"; anything else is "auto"

# VPTQ_SLICED_LAYOUT: "auto" (default) = every eligible large-codebook layer (v8-k65536-0 / -256) builds the sliced
# layout at its first one-token call while that leaves a quarter of the device memory free (MI355X: 288 GB - the
# layouts of a 70B 3-bit model are 45 GB); "1" = always; "0" = never (VQuantLinear.enable_sliced_layout per layer)
_SLICED_LAYOUT_MODE = os.environ.get("VPTQ_SLICED_LAYOUT", "auto").strip().lower() or "auto"
_SLICED_LAYOUT_ENV = _SLICED_LAYOUT_MODE not in _KNOB_OFF
_SLICED_LAYOUT_ALWAYS = _SLICED_LAYOUT_MODE in _KNOB_ON   # ("1": build whatever the free device memory)
_SLICED_MIN_FREE_FRACTION = 0.25
_SLICED_EXACT_MIN_ELEMENTS = 1 << 20   # vector-rows x columns from which the exact sliced kernel beats the gather kernel
_SLICED_EXACT_RG_MIN_ELEMENTS = 2 << 20   # ... with the residual entries gathered from L2 (two-table formats)
# most tokens served as one sliced launch PER TOKEN: decided per layer (`sliced_token_limit`);
# VPTQ_SLICED_TOKENS="one-table,two-table" overrides it (tools/sliced_tokens_bench.py)
_SLICED_TOKENS_ENV = tuple(int(v) for v in B.tune_env("VPTQ_SLICED_TOKENS").split(",")) if B.tune_env("VPTQ_SLICED_TOKENS") else None
_SLICED_MAX_TOKENS = max(max(_SLICED_TOKENS_ENV) if _SLICED_TOKENS_ENV else 3, 4)
# 2 - 4 tokens in ONE sliced launch (gemv_sliced_tok.hip): "auto" (default) = per layer where it was measured faster than the
# gather kernels and than one sliced launch per token (`sliced_one_launch`); "1" = wherever the library takes the
# layer; "0" = never
_SLICED_ONE_LAUNCH = B.tune_env("VPTQ_SLICED_ONE_LAUNCH", "auto").strip().lower() or "auto"


_SLICED_SELECTIVE_MIN_ELEMENTS = 6 << 20   # selective roundings over the folded sliced layouts (two-table formats): from 6 M index elements on
_SLICED_OOM_RETRY_CALLS = 256   # calls of a layer before a sliced-layout build that ran out of memory is tried again
_SLICED_FORMATS = "v = 8 / 16, 16384 ... 65536 main centroids, one codebook, no outliers, scale / bias"   # `has_sliced_format` in words
_SLICED_TORCH_BUILDER_BYTES = 8 * 20   # per index element: the int64 / float64 temporaries of the torch recipe (the HIP builder has none)


# WHICH compacted layers build their dense W straight from the layout (`vptq_dequant_sliced`) instead of repack + `vptq_dequant`: the one
# rule, read by `_dense_cached` and `dequant()`.  Measured on one MI355X, graph replays over a ring of 4 layers, the two routes in turns,
# median us per layer, new / repack route (tools/dequant_sliced_bench.py, profiles/r12; spread of the repack route 0.2 - 1.3 us):
#   rows x columns    v8-k65536-256     v8-k65536-0       v8-k65536-65536   v16-k65536-65536      (fp16 | bf16)
#   4096 x 4096       0.70 | 0.83       0.74 | 0.85       0.72 | 0.84       0.84 | 0.87
#   14336 x 4096      0.89 | 0.98       0.98 | 1.07       0.85 | 0.97       1.12 | 1.12
#   4096 x 14336      1.01 | 1.04       1.09 | 1.13       0.98 | 1.01       1.02 | 1.06
#   8192 x 8192       1.01 | 1.05       1.09 | 1.12       1.00 | 1.03       1.02 | 1.03
#   4096 x 28672      0.99 | 1.03       1.21 | 1.27       0.96 | 1.01       1.16 | 1.22
# The new kernel wins in every format and dtype only on layers of up to 4096 x 4096 (one round of workgroups: its gather and store
# phases do not overlap inside a workgroup); larger layers keep the repack route.  VPTQ_DEQUANT_SLICED=1 / 0 (with VPTQ_TUNING=1):
# every compacted layer / none (A/B, and a model that must not hold the repack scratch).
_DEQUANT_SLICED_MAX_ROWS = 4096
_DEQUANT_SLICED_MAX_COLS = 4096
_DEQUANT_SLICED_MODE = (B.tune_env("VPTQ_DEQUANT_SLICED", "auto") or "auto").strip().lower()


def dense_from_layout(out_features: int, in_features: int, has_entry: bool) -> bool:
    """does a COMPACTED layer of this shape build its dense W with `vptq_dequant_sliced`?  (has_entry: the library has it - one
    without the entry, added within ABI 11: never - the repack route stays)"""
    if not has_entry or _DEQUANT_SLICED_MODE in ("0", "off"):
        return False
    return _DEQUANT_SLICED_MODE in ("1", "on") or (out_features <= _DEQUANT_SLICED_MAX_ROWS and in_features <= _DEQUANT_SLICED_MAX_COLS)


def sliced_build_bytes(index_elements: int, two_tables: bool, device_builder: bool) -> int:
    """device bytes a layout build needs: the layout (5 / 4 bytes per element, one layout per table) and, with the torch recipe,
    its int64 / float64 temporaries (the HIP builder has none)"""
    return index_elements * ((8 if two_tables else 5) + (0 if device_builder else _SLICED_TORCH_BUILDER_BYTES))


def has_sliced_format(vector_len: int, num_centroids: int, num_codebooks: int, outliers: bool, norm: bool) -> bool:
    """can a layer of this format have a sliced layout at all?  Static module configuration (a permutation may still be absorbed
    later; the library decides: vptq_sliced_layout_supported)."""
    return bool(num_centroids >= 16384 and vector_len in (8, 16) and num_codebooks == 1 and not outliers and norm)


def exact_route_is_large(vector_len: int, res_centroids: int, index_elements: int) -> bool:
    """The one-token size rule of the reference arithmetic: is the layer large enough for the exact sliced kernel to beat the
    gather kernel?  (`enable_sliced_layout()` asks for the layout on any layer: `sliced_layout_kind` adds that opt-in.)"""
    if res_centroids > 0 and not (vector_len == 8 and res_centroids == 256):
        # any other residual codebook: its entries are gathered from L2 behind the LDS-local main gathers (2 blocks per
        # queue stage: the CU's L1 miss path is the limit) - us per layer, gather kernels -> sliced, profiles/r05/
        # sliced_exact_two_table_queue_ab.txt: v8-k65536-65536 8192^2 78.0 -> 59.9, 14336 x 4096 68.5 -> 52.2, 4096^2 21.6 ->
        # 21.2; v8-k65536-4096 69.9 -> 50.6 / 59.8 -> 44.3 / 20.5 -> 18.4; v16-k65536-65536 53.9 -> 46.7 / 52.3 -> 40.9 / 19.2 ->
        # 18.3; small residual tables (v16-k65536-1024: the gather kernel holds them in LDS) stay there
        return res_centroids >= 4096 and index_elements >= _SLICED_EXACT_RG_MIN_ELEMENTS
    # (reference roundings, us per layer, gather -> exact sliced, profiles/r05/sliced_exact.txt: 8192^2 39.4 -> 17.2,
    # 4096 x 14336 34.5 -> 17.0, 14336 x 4096 34.9 -> 14.7, 4096^2 12.6 -> 9.0, 4096 x 1024 7.8 -> 8.3: from 1 M index elements -
    # 8 M weights - on)
    return index_elements >= _SLICED_EXACT_MIN_ELEMENTS


def sliced_layout_kind(arithmetic_flags: int, vector_len: int, res_centroids: int, index_elements: int, opted: bool,
                       selective_served: bool, exact_served: bool, folded_served: bool):
    """(kind, wanted): the layer's arithmetic (`LayerCache.arithmetic_flags`) decides the kind of layout - "selective" / "exact" /
    "folded" -, the kind's own rule whether one is wanted.  opted: `enable_sliced_layout()` asks for a layout on any layer.  The
    three `*_served` are the library's answers: `vptq_quant_gemv_sliced_selective_supported and vptq_sliced_layout_supported_for(desc,
    0)`, `exact_column_parts(...)[0]`, `vptq_sliced_layout_supported_for(desc, 0)`."""
    if arithmetic_flags & B.GEMV_SELECTIVE and not arithmetic_flags & B.GEMV_EXACT and res_centroids >= 4096 and \
            (index_elements >= _SLICED_SELECTIVE_MIN_ELEMENTS or opted) and selective_served:
        # selective roundings, two-table formats (v8-k65536-65536, v16-k65536-65536, ...: 59 / 46 us in the reference's roundings, the
        # residual entry an L2 gather per element): the FOLDED layouts with VPTQ_GEMV_SELECTIVE - a pre-pass zeroes the blocks an activation
        # dominates and hands their exact products to the folded launch (gemv_hot.hip): ~21 us (the pre-pass is a launch of its own, ~9 us
        # at 8192^2: it pays on the large layers - from 6 M index elements on -; smaller two-table layers keep the exact layouts)
        return "selective", True
    if arithmetic_flags & (B.GEMV_EXACT | B.GEMV_SELECTIVE):
        # the reference's roundings (the default; selective: its one-table and smaller two-table layers) take the EXACT sliced kernel
        # where the layer is large enough and served - too wide for the LDS in one piece, 28672 columns: as equal column parts
        return "exact", bool((exact_route_is_large(vector_len, res_centroids, index_elements) or opted) and exact_served)
    return "folded", bool(folded_served)   # the opt-in folded form: the folded layouts wherever the library has them


def sliced_token_limit(vector_len: int, kr: int, n_el: int, exact: bool, slices: int, tables: int) -> int:
    """most tokens served as one sliced launch per token (measured, profiles/r04/sliced_tokens.txt: 8192^2 / 4096 x 14336 /
    4096^2, us per layer, gather kernel against T sliced launches - v8-k65536-0: 2 tokens 39.6 / 36.2 / 13.2 against 26.4 /
    27.1 / 17.0; v8-k65536-256: 41.4 / 36.7 / 13.4 against 34.0 / 34.5 / 19.5; v8-k65536-65536: 2 tokens 78.6 / 66.6 / 22.0
    against 42.1 / 41.3 / 23.5, 3 tokens 80.9 / 69.1 against 62.2 / 61.7; v16-k65536-65536: 2 tokens 52.9 / 52.0 / 19.6
    against 40.2 / 44.0 / 24.1; small residual tables of v = 16: never).  kr: entries of the residual codebook, 0 without one; n_el: index
    elements per table (vector-rows x columns); tables: layouts of the layer (2: one per table)."""
    if exact:
        # the reference's roundings: the gather kernels take 2 - 8 tokens for the price of one; TWO exact sliced launches beat
        # them on large v = 8 one-table layers only (profiles/r05/sliced_tokens_exact.txt, gather -> 2 launches, v8-k65536-256 /
        # -0: 8192^2 41.8 -> 40.0 / 41.4 -> 32.9; 14336 x 4096 37.0 -> 32.6 / 37.1 -> 27.9; 8192 x 28672 148.7 -> 94.8 / 135.1 ->
        # 80.9; but 4096 x 14336 36.7 -> 37.4, 4096^2 13.5 -> 19.5)
        return 2 if (vector_len == 8 and kr in (0, 256) and slices >= 16 and n_el >= 6 << 20) else 1
    if _SLICED_TOKENS_ENV is not None:
        return _SLICED_TOKENS_ENV[1 if tables == 2 else 0]
    if vector_len == 8 and kr in (0, 256) and n_el >= 6 << 20:
        return 2
    if kr >= 16384 and n_el >= 3 << 20:
        return 3 if (vector_len == 8 and kr == 65536 and n_el >= 6 << 20) else 2
    return 1


def sliced_one_launch(vector_len: int, kr: int, n_el: int, out_features: int, tokens: int, exact: bool, slices: int, supported: bool,
                      window_parts: int) -> bool:
    """2 - 4 tokens in ONE launch over the layouts (column phases; 3 - 4 tokens - in the reference's roundings: 2 - 4 - the
    contraction on the matrix pipe - gemv_sliced_tok.hip)?  Measured against the gather kernels (profiles/r04/sliced_tokens_one_launch.txt; us per 8192^2 /
    4096^2 / 14336 x 4096 layer, gather -> one launch): v8-k65536-0: 2 tokens 40.8 / 12.9 / 36.6 -> 21.4 / 11.5 / 19.0, 4 tokens
    41.1 / 13.4 / 36.9 -> 26.0 / 13.5 / 22.8; -256: 40.9 / 13.2 / 36.8 -> 23.7 / 12.4 / 20.4 and 44.0 / 16.0 / 42.9 -> 29.4 / 14.8 / 23.9;
    -65536: 78.2 / 21.5 / 68.8 -> 33.7 / 15.9 / 28.5 and 80.0 / 23.6 / 72.0 -> 39.8 / 18.5 / 43.6; v16-k65536-0: 27.7 / 13.7 / 33.5 ->
    23.4 / 12.8 / 19.5 and 31.1 / 15.2 -> 25.6 / 14.4; v16-k65536-65536: 53.0 / 19.6 / 53.9 -> 37.7 / 17.8 / 36.1 and 55.8 / 21.0 ->
    46.0 / 20.5 (4096 x 14336: 7 rows per wave - their sums in LDS, two rounds of workgroups: 57.2 -> 58.0, not taken).
    v = 16 with a residual table of <= 1024 entries stays on the gather kernel, which holds that table in LDS (v16-k65536-1024,
    2 tokens: 28.3 -> 36.1).
    kr, n_el: as in `sliced_token_limit`; supported: `SlicedGemv.tokens_supported(tokens)`; window_parts: `SlicedGemv.tokens_window_parts(tokens)` - 0 outside 2 / 3 exact
    tokens, >= 1 where the library takes them in ONE PASS of the one-token kernel."""
    if _SLICED_ONE_LAUNCH in _KNOB_OFF or not supported:
        return False
    if _SLICED_ONE_LAUNCH in _KNOB_ON:
        return True
    if exact:
        # the reference's roundings (gemv_sliced_tok.hip, EX; profiles/r05/sliced_tokens_exact.txt, gather -> one launch, us per
        # layer, v8-k65536-256): 8192^2: 2 / 3 / 4 tokens 41.5 / 43.7 / 42.0 -> 37.5 / 36.0 / 36.8; 14336 x 4096: 36.7 / 41.0 / 41.3 ->
        # 37.4 / 37.5 / 38.0; 8192 x 28672: 148.7 / 146.6 / 147.9 -> 122.0 / 124.5 / 127.0 (-0: 135 -> 82 - 86); but 4096^2: 13.5 / 15.8 / 15.7 -> 20.9 / 20.7 / 20.8 and 4096 x 14336: 36.7 / 36.8 / 37.0 -> 41.1 / 41.3 /
        # 41.9 (8 slices of 128 KiB leave room for a quarter of the columns: 4 phases); v = 16: 28.5 -> 36.0.  5 - 8 tokens: never
        # (8192^2: 44 - 46 -> 54 - 55)
        # 2 tokens there: two launches of the one-token kernel are as fast or faster (`sliced_token_limit`).
        # 2 / 3 tokens of layers whose slice leaves room for (2 tokens + 4) bytes per column - 16-slice layouts up to ~12000 /
        # ~9700 columns - take ONE PASS of the one-token kernel (gemv_sliced.hip, TOK; profiles/r05/sliced_exact_tokens_one_pass.txt,
        # gather -> one pass, 2 / 3 tokens): 8192^2 42.1 / 44.9 -> 25.1 / 28.3; 8192 x 28672 149 / 147 -> 62 / 76; 8192 x 1024 13.0 / 18.0
        # -> 11.0 / 12.9 (k65536-0: 41.3 / 42.2 -> 22.2 / 25.9, 134 / 135 -> 53 / 66); narrow layers that fit with 8 slices: parity
        # (2048 x 8192: 13.5 / 16.0 -> 13.5 / 15.5), v = 16: slower (8192^2 28.6 -> 30.3) - both stay on the gather kernel
        if vector_len != 8:
            return False
        if kr not in (0, 256):
            # two tables (v8-k65536-65536, -4096: the residual entries gathered from L2 ONCE for all tokens; profiles/r05/
            # sliced_exact_tokens_one_pass.txt): 8192^2 77.8 -> 61.5 / 63.4, 8192 x 28672 255 -> 202 / 206, kr = 4096: 68 -> 53 / 54; small
            # layers lose (8192 x 1024: 18.8 -> 21.1): the one-token rule's sizes
            return slices >= 16 and tokens <= 3 and kr >= 4096 and n_el >= _SLICED_EXACT_RG_MIN_ELEMENTS and window_parts >= 1
        # ... in WINDOW PARTS where only half of the columns' operands fit beside the slice (WPT; profiles/r05/
        # sliced_exact_tokens_window_parts.txt, gather -> one pass, 2 / 3 tokens, k65536-256 / -0): 14336 x 4096 37.0 / 42.6 -> 24.9 / 28.4
        # and 36.9 / 35.3 -> 21.7 / 26.2; 4096 x 14336 37.1 / 38.2 -> 31.5 / 37.1 and 36.2 / 35.0 -> 27.9 / 34.2; smaller layers lose
        # (4096^2 13.6 / 16.2 -> 14.8 / 16.7): from 6 M index elements on
        wparts = window_parts if tokens <= 3 else 0
        if wparts == 1:
            return slices >= 16
        if wparts > 1:
            return n_el >= 6 << 20
        return slices >= 16 and 3 <= tokens <= 4 and n_el >= 6 << 20
    if n_el < 1 << 19:       # (smaller layers are launch-bound on every route and were not measured)
        return False
    if vector_len == 8 or kr == 0:
        return True
    if kr <= 1024:
        return False
    return tokens == 2 or out_features <= 8192
