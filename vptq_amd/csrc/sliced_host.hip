// The host side of the sliced-layout GEMV family (kernels: gemv_sliced.hip - one token, and 2 / 3 tokens in one pass; gemv_sliced_tok.hip -
// 2 - 8 tokens in column phases).  No device code: compiled once, an edit to a rule here recompiles no kernel.  Three sections:
//   1. the LAYOUT-SET RULES the whole library reads (abi.hip, repack.hip, dequant_sliced.hip, layout_build.hip and, through
//      vptq_sliced_layout_set, vptq_amd/utils/sliced.py): which sliced layouts serve a layer (gemv_sliced_eligible, gemv_sliced_slices,
//      gemv_sliced_whole_table, sl_piece_set, sl_part_desc, sl_layout_set) and what makes a VptqSlicedLayout valid (sl_check_layouts);
//   2. ONE TOKEN (and 2 / 3 tokens in one pass of the one-token kernel): sl_fill, sl_decide, launch_gemv_sliced_group, gemv_sliced_instance;
//   3. SEVERAL TOKENS in column phases: the workspace layout, st_plan (the LDS map and the phase count), st_decide,
//      launch_gemv_sliced_tok_group, gemv_sliced_tok_instance.
// The kernels are reached through the instantiation dispatchers of sliced.h (launch_sl_* / launch_st_*) only.
#include <cstring>

#include "sliced.h"

namespace vptq {

// ---- 1. layout-set rules -----------------------------------------------------------
// Large-codebook layers: v = 8 or 16, 16384 ... 65536 main centroids, one codebook group, no outlier columns, norm on.
// Residual codebook: none; v = 8 with 256 entries (one launch, the table beside the slice, a byte per element); any other
// size (2 ... 65536 entries) as a SECOND TABLE with a layout of its own in the same launch.
static bool sl_pow2(int k) { return k > 0 && (k & (k - 1)) == 0; }
bool sl_res256(const VptqLayerDesc& d) { return d.vector_len == 8 && d.num_res_centroids == 256; }
bool sl_two(const VptqLayerDesc& d) { return d.num_res_centroids > 0 && !sl_res256(d); }
int gemv_sliced_tables(const VptqLayerDesc& d) { return sl_two(d) ? 2 : 1; }
static bool sl_shape_ok(const VptqLayerDesc& d, bool exact);
bool gemv_sliced_eligible(const VptqLayerDesc& d, bool exact) {
  const int T = d.index_bits + d.res_bits;
  // the reference's roundings: bias in column order (c and r meet in one lane: a residual codebook other than v8's 256-entry
  // one is gathered from L2 by a side stream of 16-bit indices - ONE layout, bucketed by the main index)
  if (exact && d.perm != nullptr && (d.bias_permuted == nullptr || (((uintptr_t)d.bias_permuted) & 15) != 0)) return false;
  return sl_shape_ok(d, exact) && (d.vector_len == 8 || d.vector_len == 16) && d.num_codebooks == 1 && d.outlier_size == 0 &&
         d.num_centroids >= 16384 && d.num_centroids <= 65536 && sl_pow2(d.num_centroids) && (1 << d.index_bits) == d.num_centroids &&
         (d.num_res_centroids == 0 || (d.num_res_centroids >= 2 && d.num_res_centroids <= 65536 && sl_pow2(d.num_res_centroids) &&
                                       (1 << d.res_bits) == d.num_res_centroids)) &&
         d.weight_scale != nullptr && d.weight_bias != nullptr &&
         (d.perm == nullptr || d.scale_permuted != nullptr) && (d.group_size % 8) == 0 && d.group_size == d.in_features &&
         d.group_size <= kSLMaxG16 && T <= 32 && (long long)d.row_words * 32 >= (long long)d.group_size * T &&
         (((uintptr_t)d.centroids | (uintptr_t)d.res_centroids | (uintptr_t)d.weight_scale | (uintptr_t)d.weight_bias |
           (uintptr_t)d.perm | (uintptr_t)d.scale_permuted) & 15) == 0;
}

// bytes of LDS behind the table: f16(s x) of every column (+ 64 padding columns) + 16 floats; the reference's roundings
// stage x and a word {scale, bias} per column instead: 6 bytes per column; + the 4 KiB residual table of the 256-entry path
static int sl_window_cols(const VptqLayerDesc& d) { return (d.group_size + kSLWindows * 8 - 1) / (kSLWindows * 8) * 8; }   // (the layout's window width)
static uint32_t sl_operand_bytes(const VptqLayerDesc& d, bool exact, int tokens = 1, int columns = 0) {
  return (uint32_t)((columns ? columns : d.group_size) + 64) * (exact ? 4u + 2u * (uint32_t)tokens : 2u) + 64u + (sl_res256(d) ? 4096u : 0u);
}
// slices a layout of this layer must have: the slice (table entries / slices, 2 v bytes each) + the staged operands must fit
// the 160 KiB of LDS.  Folded arithmetic: v = 8: 8 slices up to 14336 columns (14080 with the 256-entry table), else 16;
// v = 16: 16 slices up to 14336 columns, else 32.  Reference roundings (6 bytes per column): v = 8: 8 slices up to 5376 columns
// (4704), 16 up to 16288 (15616); v = 16: 16 / 32 at the same widths; wider layers: 0 (not served: gemv_gather)
int gemv_sliced_slices(const VptqLayerDesc& d, bool exact) {
  static const int force16 = tune_int("VPTQ_SLICED_SLICES", 0) == 16;   // =16: the larger slice count for every layer (A/B)
  const int small = d.vector_len == 16 ? 16 : 8;
  if (!exact) {
    if (force16 == 1) return 2 * small;
    return d.group_size <= (sl_res256(d) ? kSLMaxG8Res : kSLMaxG8) ? small : 2 * small;
  }
  if (d.num_centroids <= 0 || d.vector_len <= 0) return 0;
  // VPTQ_SLICED_SLICES=room2 (process-wide opt-in, v = 8): the smaller count only where the slice leaves room for TWO tokens'
  // operands, so that 2 / 3 tokens take one pass of the one-token kernel (TOK) on 4096-column layers too - they miss that by 0.5 KiB
  // with 128 KiB slices.  Measured on the Llama-3-8B shapes in v8-k65536-256 (profiles/r05/sliced_exact_slices_16_for_narrow_layers.txt):
  // 2 sequences 198.6 -> 210.7 tokens/s, 3: 270.6 -> 277.3, ONE: 127.1 -> 125.4 (the layers' own time +5 %) - one token is the
  // default's business, so the default stays "8 slices wherever one token fits".
  static const int room2 = [] { const char* e = tune_env("VPTQ_SLICED_SLICES"); return e && strcmp(e, "room2") == 0; }();
  for (int nsl = (force16 == 1 ? 2 * small : small); nsl <= 2 * small; nsl *= 2) {
    const uint32_t tab = (uint32_t)(d.num_centroids / nsl) * (uint32_t)d.vector_len * 2u;
    if ((tab + 15u) / 16u * 16u + sl_operand_bytes(d, true, (nsl == small && room2 == 1 && d.vector_len == 8) ? 2 : 1) <= kSLLdsLimit) return nsl;
  }
  return 0;
}
// bytes a workgroup of a table with k entries holds: its slice, or (whole != 0) the whole table
uint32_t sl_tab_bytes(const VptqLayerDesc& d, int k, int whole, bool exact) {
  const int nsl = gemv_sliced_slices(d, exact);
  return (uint32_t)(whole || nsl == 0 ? k : k / nsl) * (uint32_t)d.vector_len * 2u;
}
// Does every workgroup of table t (0 main, 1 residual-as-second-table) hold the WHOLE table (element words then carry the
// full index and a row's elements are split into column ranges)?  Only a second table whose slice would be under 16 KiB -
// copied in 1 KiB pieces by 16 waves, a smaller slice is mostly partial pieces and its lists are short - and only while the
// whole table still fits beside the staged activations.
int gemv_sliced_whole_table(const VptqLayerDesc& d, int t) {
  if (t != 1 || !sl_two(d)) return 0;
  const uint32_t slice = sl_tab_bytes(d, d.num_res_centroids, 0), whole = sl_tab_bytes(d, d.num_res_centroids, 1);
  const uint32_t main_slice = sl_tab_bytes(d, d.num_centroids, 0);
  const uint32_t x_bytes = (uint32_t)(d.group_size + 64) * 2u + 64u;
  if (d.num_res_centroids < gemv_sliced_slices(d)) return 1;   // (fewer entries than slices: no other way)
  return slice < 16384u && ((whole > main_slice ? whole : main_slice) + 15u) / 16u * 16u + x_bytes <= kSLLdsLimit ? 1 : 0;
}

// the tables' parts + the staged operands fit the LDS
static bool sl_shape_ok(const VptqLayerDesc& d, bool exact) {
  if (!(d.vector_len == 8 || d.vector_len == 16) || d.group_size <= 0 || d.group_size > kSLMaxG16 || d.num_centroids < 16384) return false;
  if (exact) return gemv_sliced_slices(d, true) != 0;
  uint32_t tab = sl_tab_bytes(d, d.num_centroids, 0);
  if (sl_two(d)) {
    const uint32_t t1 = sl_tab_bytes(d, d.num_res_centroids, gemv_sliced_whole_table(d, 1));
    tab = t1 > tab ? t1 : tab;
  }
  return (tab + 15u) / 16u * 16u + sl_operand_bytes(d, false) <= kSLLdsLimit;
}

// one 64-bit accumulator word per output (N x v of them), which must be ZERO before the first launch; every launch leaves
// them zero.  (Rounds 3-4 kept [tables x slices][N x v] float partial sums + arrival counters here; the size the ABI asks for
// is still that one - callers' buffers stay valid, tools/sliced_trace.py stamps into the rest.)
size_t gemv_sliced_workspace_bytes(const VptqLayerDesc& d) {
  const size_t parts = (size_t)gemv_sliced_slices(d) * (sl_two(d) ? 2 : 1);
  const size_t partial = (parts * d.num_indices * d.vector_len * sizeof(float) + 255) / 256 * 256;
  const size_t counters = (((size_t)(d.num_indices + kSLWaves - 1) / kSLWaves) * sizeof(uint32_t) + 255) / 256 * 256;
  return partial + counters;
}

SlicedLayoutSet sl_piece_set(const VptqLayerDesc& d, bool exact) {
  // (the reference's roundings need c and r in one lane: always ONE layout, bucketed by the main index)
  SlicedLayoutSet S = {};
  S.parts = 1, S.tables = !exact && sl_two(d) ? 2 : 1, S.slices = gemv_sliced_slices(d, exact), S.exact = exact;
  S.whole[1] = S.tables == 2 ? gemv_sliced_whole_table(d, 1) : 0;
  S.side_bytes = d.num_res_centroids == 0 || S.tables == 2 ? 0 : (sl_res256(d) ? 1 : 2);
  return S;
}
VptqLayerDesc sl_part_desc(const VptqLayerDesc& d, int parts, int p) {
  VptqLayerDesc q = d;
  const int w = d.group_size / parts;
  q.in_features = q.group_size = w;
  const size_t off = (size_t)2 * p * w;   // (16-bit column-order tensors)
  if (q.weight_scale) q.weight_scale = (const char*)q.weight_scale + off;
  if (q.weight_bias) q.weight_bias = (const char*)q.weight_bias + off;
  if (q.perm) q.perm = (const uint16_t*)((const char*)q.perm + off);
  if (q.scale_permuted) q.scale_permuted = (const char*)q.scale_permuted + off;
  if (q.bias_permuted) q.bias_permuted = (const char*)q.bias_permuted + off;
  return q;
}
// the column parts the reference's roundings are served with: 1 where the layer fits in one piece, else 2 or 3 equal parts of a
// multiple of 8 columns whose slices' arrivals one accumulator word counts; 0 = none
static int sl_exact_parts(const VptqLayerDesc& d) {
  static const int knob = tune_int("VPTQ_SLICED_PARTS", 1);   // (A/B: at least this many parts where the columns divide)
  const int least = knob > 1 ? knob : 1;
  const bool whole = gemv_sliced_eligible(d, true);
  if (whole && least <= 1) return 1;
  for (int parts = 2; parts <= 3; ++parts) {
    if (parts < least || d.group_size % (8 * parts) != 0) continue;
    const VptqLayerDesc q = sl_part_desc(d, parts, 0);
    if (gemv_sliced_eligible(q, true) && gemv_sliced_slices(q, true) * parts <= 127) return parts;
  }
  return least > 1 && whole ? 1 : 0;
}
SlicedLayoutSet sl_layout_set(const VptqLayerDesc& d, bool exact) {
  const int parts = exact ? sl_exact_parts(d) : (gemv_sliced_eligible(d, false) ? 1 : 0);
  if (parts == 0) return SlicedLayoutSet{};
  SlicedLayoutSet S = sl_piece_set(parts > 1 ? sl_part_desc(d, parts, 0) : d, exact);   // (equal parts: one answer)
  S.parts = parts;
  return S;
}

unsigned sl_check_layouts(const VptqLayerDesc& d, const SlicedLayoutSet& S, const VptqSlicedLayout* L, int n, unsigned needs,
                          int rows_per_wave, int* which) {
  const bool launch = (needs & kSLNeedLaunch) != 0;
  for (int i = 0; i < n; ++i) {
    const VptqSlicedLayout& l = L[i];
    const int t = S.tables == 2 ? i : 0;
    const bool side = t == 0 && S.side_bytes != 0;
    const uintptr_t e = (uintptr_t)l.elems, r = (uintptr_t)l.res;
    unsigned f = 0;
    if (!l.elems || !l.blocks || !l.first || ((needs & kSLNeedWstart) && !l.wstart)) f |= kSLFaultTensors;
    if (((needs & kSLNeedRows) && l.n_slices == 0 ? 8 : l.n_slices) != S.slices) f |= kSLFaultSlices;
    if ((needs & kSLNeedWhole) && l.whole_table != S.whole[t]) f |= kSLFaultWhole;
    if (needs & kSLNeedBuilt) {
      if (side != (l.res != nullptr)) f |= kSLFaultRes;
      const uintptr_t words = (uintptr_t)l.blocks | (uintptr_t)l.first | r | ((needs & kSLNeedWstart) ? (uintptr_t)l.wstart : 0);
      if ((e & 15) != 0 || (words & 3) != 0 || ((needs & kSLNeedRes8) && S.side_bytes == 2 && (r & 7) != 0)) f |= kSLFaultAlign;
    } else if (side && (S.exact || launch)) {
      // (WHO ASKS decides, as it did while each had its own copy: an entry holds the exact arithmetic's stream, uint8 or uint16, to "set,
      // at an even address" and does not look at a folded one; the launch behind it needs every stream set and the uint16 one even)
      if (!l.res || ((r & 1) != 0 && (!launch || S.side_bytes == 2))) f |= kSLFaultRes;
    }
    if ((needs & kSLNeedRows) && (l.rows_per_wave < 1 || l.rows_per_wave > kSLMaxRowsPerWave ||
                                  (rows_per_wave != 0 && l.rows_per_wave != rows_per_wave)))
      f |= kSLFaultRows;
    if (launch) {
      if (l.elems_per_lane != 0 && l.elems_per_lane != 1) f |= kSLFaultElemsPerLane;
      if ((e & 3) != 0) f |= kSLFaultAlign;
      // (a sliced table needs at least one entry per slice; whole = every workgroup of the table holds all of it)
      if (!l.whole_table && (t ? d.num_res_centroids : d.num_centroids) < S.slices) f |= kSLFaultFewEntries;
    }
    if (f && which) *which = i;
    if (f) return f;
  }
  return 0;
}
bool sl_parts_share(const VptqLayerDesc* d, void* const* y, void* const* ws, int n) {
  for (int i = 1; i < n; ++i)
    if (y[i] != y[0] || ws[i] != ws[0] || d[i].out_features != d[0].out_features || d[i].num_indices != d[0].num_indices ||
        d[i].bias != d[0].bias || d[i].in_features != d[0].in_features)
      return false;
  return true;
}

// ---- 2. one token (and 2 / 3 tokens in one pass) -------------------------------------
// L: one layout (residual none / the 256-entry path of v = 8) or TWO consecutive ones (any other residual codebook: [0]
// bucketed by the main index, [1] by the residual index).  (c + r) f16(s x) = c f16(s x) + r f16(s x): the residual table's
// (slice, row block) workgroups run beside the main table's in the SAME launch and meet them in the output's accumulator
// word - two launches, one per table, cost a second boundary, a second epilogue and half the workgroups in flight (8192^2: 27.2 us
// against 21.2; 4096^2: 17.8 against 12.0)
static hipError_t sl_fill(const VptqLayerDesc& d, const SlicedLayoutSet& S, const VptqSlicedLayout* L, const void* x, void* y, int flags,
                          void* ws, SlicedParams& P, uint32_t& lds, int tokens = 1) {
  const bool exact = S.exact;
  if (tokens != 1 && !gemv_sliced_exact_tokens_ok(d, tokens)) return hipErrorInvalidValue;
  const bool res = S.side_bytes == 1, rg = S.side_bytes == 2, two = S.tables == 2;
  if (S.slices == 0 || sl_check_layouts(d, S, L, S.tables, kSLNeedRows | kSLNeedWhole | kSLNeedLaunch, L[0].rows_per_wave) != 0 ||
      !ws || (((uintptr_t)x) & 15) != 0)
    return hipErrorInvalidValue;
  P = SlicedParams{};
  P.elems = (const uint32_t*)L[0].elems;
  P.res = (res || rg) ? (const uint8_t*)L[0].res : nullptr;   // (rg: uint16 per element)
  P.rcent = (res || rg) ? (const uint32_t*)d.res_centroids : nullptr;
  P.blocks = (const int32_t*)L[0].blocks;
  P.first = (const int32_t*)L[0].first;
  P.cent = (const uint32_t*)d.centroids;
  P.tab0 = sl_tab_bytes(d, d.num_centroids, L[0].whole_table, exact);
  P.stride0 = L[0].whole_table ? 0u : P.tab0;
  if (two) {
    P.elems2 = (const uint32_t*)L[1].elems;
    P.blocks2 = (const int32_t*)L[1].blocks;
    P.first2 = (const int32_t*)L[1].first;
    P.cent2 = (const uint32_t*)d.res_centroids;
    P.tab1 = sl_tab_bytes(d, d.num_res_centroids, L[1].whole_table);
    P.stride1 = L[1].whole_table ? 0u : P.tab1;
  }
  P.x_off = ((P.tab0 > P.tab1 ? P.tab0 : P.tab1) + 15u) & ~15u;
  P.x = (const uint16_t*)x;
  P.scale = (const uint16_t*)(d.perm ? d.scale_permuted : d.weight_scale);
  P.wbias = (const uint16_t*)d.weight_bias;
  P.cbias = (const uint16_t*)(d.perm ? d.bias_permuted : d.weight_bias);
  P.perm = (const uint16_t*)d.perm;
  P.bias = (const uint16_t*)d.bias;
  P.partial = (float*)ws;
  P.y = y;
  P.N = d.num_indices; P.G = d.group_size; P.O = d.out_features;
  P.rows_per_wave = L[0].rows_per_wave;
  const int rows_per_wg = kSLWaves * L[0].rows_per_wave;
  P.n_rowblocks = (d.num_indices + rows_per_wg - 1) / rows_per_wg;
  P.out_f32 = (flags & VPTQ_GEMV_OUT_F32) ? 1 : 0;
  P.x_stride = d.in_features; P.y_stride = d.out_features; P.acc_stride = d.num_indices * d.vector_len;
  P.wparts = 1;
  if (tokens != 1) {
    P.wparts = gemv_sliced_exact_tokens_parts(d, tokens);
    if (P.wparts > 1) {
      if (!L[0].wstart) return hipErrorInvalidValue;
      P.wstart = (const int32_t*)L[0].wstart;
      P.wcols = sl_window_cols(d);
      P.wstage = (kSLWindows / P.wparts) * P.wcols < d.group_size ? (kSLWindows / P.wparts) * P.wcols : d.group_size;
      // (one round of workgroups: the rows per wave grow with the parts)
      const int rpw = L[0].rows_per_wave * P.wparts;
      P.rows_per_wave = rpw > kSLMaxRowsPerWave ? kSLMaxRowsPerWave : rpw;
      const int rows_per_wg2 = kSLWaves * P.rows_per_wave;
      P.n_rowblocks = (d.num_indices + rows_per_wg2 - 1) / rows_per_wg2;
    }
  }
  lds = P.x_off + sl_operand_bytes(d, exact, tokens, P.wparts > 1 ? P.wstage : 0);
  return lds > kSLLdsLimit ? hipErrorInvalidValue : hipSuccess;
}

// n <= kSLMaxGroup layers of ONE format (vector length, slices, residual kind, dtype) and one input width reading the same x:
// layouts = the layers' layout structs one after the other (1 or 2 each); one launch
bool gemv_sliced_groupable(const VptqLayerDesc* d, int n, bool exact) {
  if (n < 1 || n > kSLMaxGroup) return false;
  for (int i = 0; i < n; ++i) {
    if (!gemv_sliced_eligible(d[i], exact)) return false;
    if (d[i].dtype != d[0].dtype || d[i].vector_len != d[0].vector_len || d[i].group_size != d[0].group_size ||
        gemv_sliced_slices(d[i], exact) != gemv_sliced_slices(d[0], exact) || sl_res256(d[i]) != sl_res256(d[0]) || sl_two(d[i]) != sl_two(d[0]))
      return false;
  }
  return true;
}
// 2 / 3 tokens in one pass of the exact kernel (TOK): one-table formats whose slice + (2 tokens + 4) bytes per column fit the LDS.
// Measured (profiles/r05/sliced_exact_tokens_one_pass.txt) where the 16 (v = 16: 32) slice layouts are: wider than ~5000 columns.
// ... in how many WINDOW PARTS (workgroups per (slice, row block), each staging its column windows alone): 1 where all columns
// fit, else - v = 8, one table; the layout must carry `wstart` - 2 or 4; 0 = not served.  VPTQ_SLICED_WINDOW_PARTS=0: never more than 1 (A/B)
int gemv_sliced_exact_tokens_parts(const VptqLayerDesc& d, int tokens) {
  if (tokens < 2 || tokens > (d.vector_len == 16 ? 2 : 3) || !gemv_sliced_eligible(d, true) || (sl_two(d) && d.vector_len != 8)) return 0;
  const int nsl = gemv_sliced_slices(d, true);
  if (nsl == 0) return 0;
  const uint32_t tab = (sl_tab_bytes(d, d.num_centroids, 0, true) + 15u) / 16u * 16u;
  if (tab + sl_operand_bytes(d, true, tokens) <= kSLLdsLimit) return 1;
  static const bool on = [] { const char* e = tune_env("VPTQ_SLICED_WINDOW_PARTS"); return !(e && e[0] == '0'); }();
  if (!on || d.vector_len != 8 || sl_two(d)) return 0;
  const int wc = sl_window_cols(d);
  for (int wparts = 2; wparts <= kSLWindows; wparts *= 2) {
    const int wmax = (kSLWindows / wparts) * wc < d.group_size ? (kSLWindows / wparts) * wc : d.group_size;
    if (tab + sl_operand_bytes(d, true, tokens, wmax) <= kSLLdsLimit && nsl * wparts <= 127) return wparts;
  }
  return 0;
}
bool gemv_sliced_exact_tokens_ok(const VptqLayerDesc& d, int tokens) { return gemv_sliced_exact_tokens_parts(d, tokens) >= 1; }
// accumulator words of such a launch: [tokens][N x v], zero before the first launch, left zero by every launch
size_t gemv_sliced_exact_tokens_workspace_bytes(const VptqLayerDesc& d, int tokens) {
  return ((size_t)tokens * d.num_indices * d.vector_len * sizeof(unsigned long long) + 255) / 256 * 256;
}
// VPTQ_GEMV_COLUMN_PARTS: the n "layers" are the column ranges [i G / n, (i + 1) G / n) of ONE layer too wide for the LDS (28672
// columns in the reference's roundings: 6 bytes per column) - descriptors with in_features = group_size = G / n and the column
// order tensors (scale, bias, permutation) advanced to the part's first column, a layout per part built from those columns of
// the index matrix; x is the WHOLE activation (part i reads it from column i G / n on, or through its slice of the permutation),
// y and the accumulator words are shared: an output is complete after n x slices arrivals.
// ---- decide, then launch (as gemv_k256.hip): sl_decide says what one call is - the parameter blocks, the LDS, the instantiation's
// template arguments and the launch shape; launch_gemv_sliced_group launches exactly that and gemv_sliced_instance prints it, so the
// two cannot disagree.  Nothing is dereferenced: the query passes placeholder x / y / workspace pointers.
static hipError_t sl_decide(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, const void* x, void* const* y, int flags,
                            void* const* ws, int tokens, const float* corr, SlicedGroupParams& GP, uint32_t& lds, SlicedDecision& D) {
  const bool exact = (flags & VPTQ_GEMV_EXACT) != 0;
  const bool parts = (flags & VPTQ_GEMV_COLUMN_PARTS) != 0;
  if (!gemv_sliced_groupable(d, n, exact) || (tokens != 1 && !exact)) return hipErrorInvalidValue;
  // (the folded form stages 32768 columns in one piece: no parts needed)
  if (parts && (!exact || !sl_parts_share(d, y, ws, n))) return hipErrorInvalidValue;
  GP = SlicedGroupParams{};
  GP.n = n;
  lds = 0;
  const SlicedLayoutSet S0 = sl_piece_set(d[0], exact);   // (one format: one table and slice count for every member)
  const int tables = S0.tables, nsl = S0.slices, nslt = nsl * tables;
  bool perm = false;
  for (int i = 0; i < n; ++i) {
    uint32_t l = 0;
    // (a part without a permutation reads its own columns of x; with one, its slice of `perm` indexes the whole activation)
    const void* const xi = (parts && d[i].perm == nullptr) ? (const void*)((const uint16_t*)x + (size_t)i * d[i].in_features) : x;
    const hipError_t e = sl_fill(d[i], i ? sl_piece_set(d[i], exact) : S0, L + (size_t)i * tables, xi, y[i], flags, ws[i], GP.p[i], l, tokens);
    if (e != hipSuccess) return e;
    if (parts) GP.p[i].x_stride = n * d[i].in_features;   // (tokens of the WHOLE activation: a part's columns lie one row of all parts apart)
    GP.p[i].corr = (n == 1 && tokens == 1 && !exact) ? corr : nullptr;   // (selective roundings: one layer, one token, folded form)
    lds = l > lds ? l : lds;
    GP.start[i + 1] = GP.start[i] + nslt * GP.p[i].wparts * GP.p[i].n_rowblocks;
    if (GP.p[i].wparts != GP.p[0].wparts) return hipErrorInvalidValue;   // (one input width: one answer)
    perm = perm || d[i].perm != nullptr;
  }
  for (int i = n; i < kSLMaxGroup; ++i) GP.start[i + 1] = GP.start[n];
  GP.arrivals = nslt * (parts ? n : 1) * GP.p[0].wparts;
  if (GP.arrivals > 127) return hipErrorInvalidValue;   // (7 bits of the accumulator word count them)
  D = SlicedDecision{};
  D.f16 = d[0].dtype == VPTQ_DTYPE_F16;
  D.nsl = nsl; D.v = d[0].vector_len; D.tok = tokens;
  D.res = sl_res256(d[0]); D.two = !exact && sl_two(d[0]); D.ex = exact; D.rg = exact && sl_two(d[0]);
  D.wpt = tokens != 1 && GP.p[0].wparts > 1;
  D.wparts = GP.p[0].wparts; D.parts = parts ? n : 1; D.n = parts ? 1 : n;
  D.rpw = GP.p[0].rows_per_wave; D.arrivals = GP.arrivals;
  D.whole1 = tables == 2 ? L[1].whole_table : 0; D.side = S0.side_bytes;
  D.perm = perm; D.corr = GP.p[0].corr != nullptr;
  return hipSuccess;
}
hipError_t launch_gemv_sliced_group(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, const void* x, void* const* y,
                                    int flags, void* const* ws, hipStream_t st, int tokens, const float* corr) {
  SlicedGroupParams GP;
  SlicedDecision D;
  uint32_t lds = 0;
  if (const hipError_t e = sl_decide(d, L, n, x, y, flags, ws, tokens, corr, GP, lds, D); e != hipSuccess) return e;
  if (D.wpt) return launch_sl_tokens_wpt(D, GP, lds, st);
  if (D.tok != 1) return launch_sl_tokens(D, GP, lds, st);
  return launch_sl_one(D, GP, lds, st);
}
// the instantiation launch_gemv_sliced_group would launch for (d, L, n, tokens, flags), as text; corr: with the hot blocks' products of
// the selective pre-pass.  0, -1: no launch, -2: buffer too small
int gemv_sliced_instance(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, int tokens, int flags, bool corr, char* buf, size_t bytes) {
  if (n < 1 || n > kSLMaxGroup) return -1;
  // placeholders: aligned, never dereferenced (column parts share one y and one workspace, as the call requires)
  void* const some = (void*)(uintptr_t)4096;
  void* ys[kSLMaxGroup] = {some, some, some};
  void* wss[kSLMaxGroup] = {some, some, some};
  SlicedGroupParams GP;
  SlicedDecision D;
  uint32_t lds = 0;
  if (sl_decide(d, L, n, some, ys, flags, wss, tokens, corr ? (const float*)some : nullptr, GP, lds, D) != hipSuccess) return -1;
  Text t = {buf, bytes, 0, true};
  t.add("gemv_sliced dt=%s nsl=%d res=%d v=%d two=%d ex=%d rg=%d tok=%d wpt=%d wparts=%d parts=%d n=%d rpw=%d "
        "arrivals=%d whole1=%d side=%d perm=%d corr=%d", dt_text(D.f16), D.nsl, (int)D.res, D.v, (int)D.two, (int)D.ex,
        (int)D.rg, D.tok, (int)D.wpt, D.wparts, D.parts, D.n, D.rpw, D.arrivals, D.whole1, D.side, (int)D.perm, (int)D.corr);
  return text_done(t);
}
hipError_t launch_gemv_sliced(const VptqLayerDesc& d, const VptqSlicedLayout* L, const void* x, void* y, int flags,
                              void* ws, hipStream_t st, const float* corr) {
  void* const ys[1] = {y};
  void* const wss[1] = {ws};
  return launch_gemv_sliced_group(&d, L, 1, x, ys, flags, wss, st, 1, corr);
}

// ---- 3. several tokens in column phases ----------------------------------------------
static bool st_exact_ok(const VptqLayerDesc& d) { return !sl_two(d) && gemv_sliced_eligible(d, true); }
static size_t st_partial_bytes(const VptqLayerDesc& d, int tokens, bool exact) {
  const SlicedLayoutSet S = sl_piece_set(d, exact);
  const size_t parts = (size_t)S.slices * S.tables;
  return ((size_t)tokens * parts * d.num_indices * d.vector_len * sizeof(float) + 255) / 256 * 256;
}
static size_t st_counter_bytes(const VptqLayerDesc& d) {
  return (((size_t)(d.num_indices + kSLWaves - 1) / kSLWaves) * sizeof(uint32_t) + 255) / 256 * 256;
}
// ... + (a layer with an input permutation) x[perm] of every token: the kernel stages activations in COLUMN order and a load
// the compiler can see inside its stream loop costs it the counted waits, so the gather is a pre-pass (gemv_k256c.hip:
// permute_x_kernel, one workgroup per 2048 columns and token)
static size_t st_perm_bytes(const VptqLayerDesc& d, int tokens) { return (size_t)tokens * gemv_k256c_perm_bytes(d); }
// (one size for both arithmetics: the exact layouts may have twice the slices)
static size_t st_partial_bytes_max(const VptqLayerDesc& d, int tokens) {
  const size_t a = gemv_sliced_eligible(d) ? st_partial_bytes(d, tokens, false) : 0, b = st_exact_ok(d) ? st_partial_bytes(d, tokens, true) : 0;
  return a > b ? a : b;
}
// ... and, in front of the partial sums (a fixed place whatever the token count), the accumulator words of the ONE-PASS route:
// 2 / 3 tokens in the reference's roundings through the one-token kernel (gemv_sliced.hip, TOK), zero between launches
static size_t st_acc_bytes(const VptqLayerDesc& d) { return gemv_sliced_eligible(d, true) ? gemv_sliced_exact_tokens_workspace_bytes(d, 3) : 0; }
size_t gemv_sliced_tok_workspace_bytes(const VptqLayerDesc& d, int tokens) {
  return st_counter_bytes(d) + st_acc_bytes(d) + st_partial_bytes_max(d, tokens) + st_perm_bytes(d, tokens);
}
// VPTQ_SLICED_ONE_PASS=0: 2 / 3 exact tokens through the column-phase kernel as well (A/B runs)
static bool st_one_pass(const VptqLayerDesc& d, int tokens, bool exact) {
  static const bool on = [] { const char* e = tune_env("VPTQ_SLICED_ONE_PASS"); return !(e && atoi(e) == 0 && e[0] == '0'); }();
  return exact && on && gemv_sliced_exact_tokens_ok(d, tokens);
}

// rows per wave: one round of workgroups (slices x tables x row blocks of 16 waves ~ the CUs)
static int st_rows_per_wave(const VptqLayerDesc& d, bool exact) {
  const SlicedLayoutSet S = sl_piece_set(d, exact);
  const long long nslt = (long long)S.slices * S.tables;
  long long r = ((long long)d.num_indices * nslt + kSLWaves * 256 - 1) / (kSLWaves * 256);
  return (int)(r < 1 ? 1 : r > kSLMaxRowsPerWave ? kSLMaxRowsPerWave : r);
}

struct StPlan { int tok, phases, rpw, reg_sums; uint32_t x_off, bd_off, res_off, sum_off, sb_off, lds; };
// the template's token count (2 or 4), the fewest phases whose activations fit beside the table, and the LDS map.  The rows'
// sums (16 waves x rows per wave x tokens x v floats) must fit too: where one round of workgroups does not leave room for
// them even with 4 phases (v = 16 with two tables: 64 floats per row), fewer rows per wave - more workgroups - do.
static bool st_plan(const VptqLayerDesc& d, const VptqSlicedLayout* L, int tokens, bool exact, StPlan& pl, int rpw0 = 0) {
  if (tokens < 2 || tokens > 8) return false;
  const bool res = sl_res256(d), two = sl_two(d);
  if (exact && !st_exact_ok(d)) return false;
  static const bool tok4 = tune_flag("VPTQ_SLICED_TOK4");   // =1: 2 tokens through the 4-slot (matrix-pipe) kernel too (A/B runs)
  pl.tok = tokens > 4 ? 8 : (tokens == 2 && !tok4 && !exact) ? 2 : 4;   // (the reference's roundings: matrix-pipe mode only)
  uint32_t tab = sl_tab_bytes(d, d.num_centroids, 0, exact);
  if (two) {
    const uint32_t t1 = sl_tab_bytes(d, d.num_res_centroids, L[1].whole_table);
    tab = t1 > tab ? t1 : tab;
  }
  pl.x_off = (tab + 15u) & ~15u;
  const int G = d.group_size;
  const int wcols = (G + kSTWindows * 8 - 1) / (kSTWindows * 8) * 8;
  static const int phases_knob = tune_int("VPTQ_SLICED_MIN_PHASES", 1);   // =2 / 4: more phases than the LDS asks for (A/B runs)
  const int min_phases = (phases_knob == 2 || phases_knob == 4) ? phases_knob : 1;
  static const bool no_reg_sums = tune_flag("VPTQ_SLICED_LDS_SUMS");  // =1: the rows' sums in LDS in every mode (A/B runs)
  for (int rpw = rpw0 > 0 ? rpw0 : st_rows_per_wave(d, exact); rpw >= 1; rpw = rpw > 1 ? (rpw + 1) / 2 : 0) {
    for (int phases = min_phases; phases <= kSTWindows; phases *= 2) {
      const int wmax = (kSTWindows / phases) * wcols < G ? (kSTWindows / phases) * wcols : G;   // columns of the widest phase
      uint32_t o = pl.x_off + (uint32_t)(wmax + 8) * (uint32_t)pl.tok * 2u;
      o = (o + 15u) & ~15u;
      pl.sb_off = o; o += exact ? (uint32_t)(wmax + 8) * 8u : 0u;
      pl.bd_off = o; o += (uint32_t)pl.tok * kSLWaves * 4u;
      pl.res_off = o; o += res ? 4096u : 0u;
      const int reg_sums = pl.tok >= 4 && rpw <= kSTRegRows && !no_reg_sums;   // (matrix-pipe mode: 4 registers per row)
      pl.sum_off = o; o += reg_sums ? 0u : (uint32_t)kSLWaves * (uint32_t)rpw * (uint32_t)(pl.tok * d.vector_len) * 4u;
      if (o <= kSLLdsLimit) { pl.phases = phases; pl.rpw = rpw; pl.reg_sums = reg_sums; pl.lds = o; return true; }
    }
  }
  return false;
}

int gemv_sliced_tok_one_pass_parts(const VptqLayerDesc& d, int tokens, bool exact) { return st_one_pass(d, tokens, exact) ? gemv_sliced_exact_tokens_parts(d, tokens) : 0; }
bool gemv_sliced_tok_eligible(const VptqLayerDesc& d, const VptqSlicedLayout* L, int tokens, bool exact) {
  StPlan pl;
  if (!L) return false;
  // (ONE pass of the one-token kernel: also the two-table formats of v = 8, their residual entries gathered once for all tokens)
  // (no column windows needed - unless the columns are taken in window parts)
  if (st_one_pass(d, tokens, exact))
    return L[0].n_slices == gemv_sliced_slices(d, true) && (!sl_two(d) || L[0].res) && (gemv_sliced_exact_tokens_parts(d, tokens) == 1 || L[0].wstart);
  if (!(exact ? st_exact_ok(d) : gemv_sliced_eligible(d))) return false;
  const int n = exact ? 1 : gemv_sliced_tables(d);
  for (int i = 0; i < n; ++i)
    if (!L[i].wstart || L[i].n_slices != gemv_sliced_slices(d, exact)) return false;   // (the arithmetic's own slice count)
  return st_plan(d, L, tokens, exact, pl);
}

// one layer's parameter block (its permutation pre-pass is queued into perm_*: one launch for the whole group)
struct StPermJobs { VptqLayerDesc d[8 * kSTMaxGroup]; const void* xin[8 * kSTMaxGroup]; void* xout[8 * kSTMaxGroup]; int n; };
static hipError_t st_fill(const VptqLayerDesc& d, const VptqSlicedLayout* L, const void* x, void* y, int tokens, int flags, void* ws,
                          int rpw0, SlicedTokParams& TP, StPlan& pl, StPermJobs& jobs) {
  const bool exact = (flags & VPTQ_GEMV_EXACT) != 0;
  if (!gemv_sliced_tok_eligible(d, L, tokens, exact) || !st_plan(d, L, tokens, exact, pl, rpw0)) return hipErrorInvalidValue;
  const SlicedLayoutSet S = sl_piece_set(d, exact);
  const bool res = S.side_bytes == 1, two = S.tables == 2;
  // (the kernel takes its rows per wave from the plan: the structs' own need not agree)
  if (sl_check_layouts(d, S, L, S.tables, kSLNeedRows | kSLNeedWhole | kSLNeedLaunch) != 0 || !ws || (((uintptr_t)x) & 15) != 0 || (d.in_features % 8) != 0)
    return hipErrorInvalidValue;
  TP = SlicedTokParams{};
  SlicedParams& P = TP.p;
  P.elems = (const uint32_t*)L[0].elems;
  P.res = res ? (const uint8_t*)L[0].res : nullptr;
  P.rcent = res ? (const uint32_t*)d.res_centroids : nullptr;
  P.blocks = (const int32_t*)L[0].blocks;
  P.first = (const int32_t*)L[0].first;
  P.cent = (const uint32_t*)d.centroids;
  P.tab0 = sl_tab_bytes(d, d.num_centroids, 0, exact);
  P.stride0 = P.tab0;
  TP.wstart = (const int32_t*)L[0].wstart;
  if (two) {
    P.elems2 = (const uint32_t*)L[1].elems;
    P.blocks2 = (const int32_t*)L[1].blocks;
    P.first2 = (const int32_t*)L[1].first;
    P.cent2 = (const uint32_t*)d.res_centroids;
    P.tab1 = sl_tab_bytes(d, d.num_res_centroids, L[1].whole_table);
    P.stride1 = L[1].whole_table ? 0u : P.tab1;
    TP.wstart2 = (const int32_t*)L[1].wstart;
  }
  P.x_off = pl.x_off;
  P.x = (const uint16_t*)x;
  P.scale = (const uint16_t*)(d.perm ? d.scale_permuted : d.weight_scale);
  P.wbias = (const uint16_t*)d.weight_bias;
  P.cbias = (const uint16_t*)(d.perm ? d.bias_permuted : d.weight_bias);
  P.perm = nullptr;
  TP.xs = (const uint16_t*)x;
  TP.x_stride = d.in_features;
  if (d.perm) {
    char* const base = (char*)ws + st_counter_bytes(d) + st_acc_bytes(d) + st_partial_bytes_max(d, tokens);
    for (int t = 0; t < tokens; ++t) {
      jobs.d[jobs.n] = d;
      jobs.xin[jobs.n] = (const uint16_t*)x + (size_t)t * d.in_features;
      jobs.xout[jobs.n] = base + (size_t)t * gemv_k256c_perm_bytes(d);
      ++jobs.n;
    }
    TP.xs = (const uint16_t*)base;
    TP.x_stride = (int)(gemv_k256c_perm_bytes(d) / 2);
  }
  P.bias = (const uint16_t*)d.bias;
  // (the arrival counters FIRST: a workspace sized - and zeroed once - for 4 tokens serves 2 and 3 as well)
  P.arrived = (uint32_t*)ws;
  P.partial = (float*)((char*)ws + st_counter_bytes(d) + st_acc_bytes(d));
  P.y = y;
  P.N = d.num_indices; P.G = d.group_size; P.O = d.out_features;
  P.rows_per_wave = pl.rpw;
  const int rows_per_wg = kSLWaves * pl.rpw;
  P.n_rowblocks = (d.num_indices + rows_per_wg - 1) / rows_per_wg;
  P.out_f32 = (flags & VPTQ_GEMV_OUT_F32) ? 1 : 0;
  TP.tokens = tokens;
  TP.phases = pl.phases;
  TP.wcols = (d.group_size + kSTWindows * 8 - 1) / (kSTWindows * 8) * 8;
  TP.x_in_stride = d.in_features;
  TP.y_stride = d.out_features;
  TP.bd_off = pl.bd_off; TP.res_off = pl.res_off; TP.sum_off = pl.sum_off; TP.sb_off = pl.sb_off;
  TP.reg_sums = pl.reg_sums;
  return hipSuccess;
}

// n <= kSTMaxGroup layers of ONE format (vector length, slices, residual kind, dtype) and one input width reading the same x
bool gemv_sliced_tok_groupable(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, int tokens, bool exact) {
  if (n < 1 || n > kSTMaxGroup || !gemv_sliced_groupable(d, n, exact)) return false;
  const int tables = exact ? 1 : gemv_sliced_tables(d[0]);
  for (int i = 0; i < n; ++i)
    if (!gemv_sliced_tok_eligible(d[i], L + (size_t)i * tables, tokens, exact)) return false;
  return true;
}

// ---- decide, then launch (as sl_decide above): what one call is.  one_pass: the call is a launch of the one-token kernel over
// the accumulator words acc[] (2 / 3 tokens in the reference's roundings) - nothing else is filled; else the column-phase kernel's
// parameter blocks, the permutation pre-pass's jobs, grid, LDS and the instantiation.  Nothing is dereferenced.
static hipError_t st_decide(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, const void* x, void* const* y, int tokens, int flags,
                            void* const* ws, bool& one_pass, void** acc, SlicedTokGroupParams& GP, StPermJobs& jobs, uint32_t& lds,
                            SlicedTokDecision& D) {
  const bool exact = (flags & VPTQ_GEMV_EXACT) != 0;
  if (!gemv_sliced_tok_groupable(d, L, n, tokens, exact)) return hipErrorInvalidValue;
  {   // 2 / 3 tokens in the reference's roundings: ONE pass of the one-token kernel where every member's operands fit its LDS
    one_pass = true;
    for (int i = 0; i < n; ++i) one_pass = one_pass && st_one_pass(d[i], tokens, exact);
    if (one_pass) {
      for (int i = 0; i < n; ++i) acc[i] = (char*)ws[i] + st_counter_bytes(d[i]);
      return hipSuccess;
    }
    // (column parts of one layer share their output and accumulator words: the one pass only - the column-phase kernel below keeps
    // partial sums and counters per layer)
    if (flags & VPTQ_GEMV_COLUMN_PARTS) return hipErrorInvalidValue;
  }
  GP = SlicedTokGroupParams{};
  GP.n = n;
  jobs.n = 0;
  const SlicedLayoutSet S0 = sl_piece_set(d[0], exact);
  const int tables = S0.tables, nsl = S0.slices, nslt = nsl * tables;
  // rows per wave: one round of workgroups over ALL members
  long long rows = 0;
  for (int i = 0; i < n; ++i) rows += d[i].num_indices;
  long long r0 = (rows * nslt + kSLWaves * 256 - 1) / (kSLWaves * 256);
  int rpw0 = n == 1 ? 0 : (int)(r0 < 1 ? 1 : r0 > kSLMaxRowsPerWave ? kSLMaxRowsPerWave : r0);
  // (3 - 4 tokens: rather a second round of workgroups than the rows' sums out of the registers - gate / up of an 8B model,
  // 2 x 14336 outputs, v8-k65536-256: 7 rows per wave 55.5 us, 4 rows per wave 52.3 - but not a third and fourth round: the
  // two-table format of the same layers, 14 rows per wave 72.9 us, 4 rows per wave 90.9)
  if (tokens > 2 && rpw0 > kSTRegRows && rpw0 <= 2 * kSTRegRows) rpw0 = kSTRegRows;
  lds = 0;
  D = SlicedTokDecision{};
  for (int i = 0; i < n; ++i) {
    StPlan pl;
    const hipError_t e = st_fill(d[i], L + (size_t)i * tables, x, y[i], tokens, flags, ws[i], rpw0, GP.p[i], pl, jobs);
    if (e != hipSuccess) return e;
    lds = pl.lds > lds ? pl.lds : lds;
    D.tok = pl.tok;
    if (i == 0) { D.phases = pl.phases; D.rpw = pl.rpw; D.reg_sums = pl.reg_sums; }
    GP.start[i + 1] = GP.start[i] + nslt * GP.p[i].p.n_rowblocks;
  }
  for (int i = n; i < kSTMaxGroup; ++i) GP.start[i + 1] = GP.start[n];
  D.f16 = d[0].dtype == VPTQ_DTYPE_F16;
  D.nsl = nsl; D.v = d[0].vector_len;
  D.res = S0.side_bytes == 1; D.two = S0.tables == 2; D.ex = exact;
  D.n = n; D.whole1 = tables == 2 ? L[1].whole_table : 0;
  D.perm = jobs.n > 0;
  return hipSuccess;
}

// x: [tokens][in_features], y[i]: [tokens][out_features of layer i] (fp32 with VPTQ_GEMV_OUT_F32); ws[i]:
// gemv_sliced_tok_workspace_bytes of layer i, zero before its first use (every launch leaves the counters zero)
hipError_t launch_gemv_sliced_tok_group(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, const void* x, void* const* y,
                                        int tokens, int flags, void* const* ws, hipStream_t st) {
  SlicedTokGroupParams GP;
  StPermJobs jobs = {};
  SlicedTokDecision D;
  uint32_t lds = 0;
  bool one_pass = false;
  void* acc[kSTMaxGroup];
  if (const hipError_t e = st_decide(d, L, n, x, y, tokens, flags, ws, one_pass, acc, GP, jobs, lds, D); e != hipSuccess) return e;
  if (one_pass) return launch_gemv_sliced_group(d, L, n, x, y, flags, acc, st, tokens);
  if (jobs.n > 0) {
    const hipError_t e = launch_permute_x(jobs.d, jobs.n, jobs.xin, jobs.xout, st);
    if (e != hipSuccess) return e;
  }
  const int grid = GP.start[n];
  if (D.ex) return D.tok == 8 ? launch_st_ex8(D, GP, grid, lds, st) : launch_st_ex4(D, GP, grid, lds, st);
  if (D.tok == 8) return launch_st_tok8(D, GP, grid, lds, st);
  return launch_st_tok24(D, GP, grid, lds, st);
}
// what launch_gemv_sliced_tok_group would launch, as text: the column-phase kernel's instance, or (one pass) gemv_sliced's
int gemv_sliced_tok_instance(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, int tokens, int flags, char* buf, size_t bytes) {
  if (n < 1 || n > kSTMaxGroup) return -1;
  void* const some = (void*)(uintptr_t)4096;   // placeholders: aligned, never dereferenced
  void* ys[kSTMaxGroup] = {some, some, some};
  void* wss[kSTMaxGroup] = {some, some, some};
  SlicedTokGroupParams GP;
  StPermJobs jobs = {};
  SlicedTokDecision D;
  uint32_t lds = 0;
  bool one_pass = false;
  void* acc[kSTMaxGroup];
  if (st_decide(d, L, n, some, ys, tokens, flags, wss, one_pass, acc, GP, jobs, lds, D) != hipSuccess) return -1;
  if (one_pass) return gemv_sliced_instance(d, L, n, tokens, flags, false, buf, bytes);
  Text t = {buf, bytes, 0, true};
  t.add("gemv_sliced_tok dt=%s nsl=%d res=%d v=%d two=%d tok=%d ex=%d phases=%d rpw=%d regsums=%d n=%d whole1=%d perm=%d", dt_text(D.f16),
        D.nsl, (int)D.res, D.v, (int)D.two, D.tok, (int)D.ex, D.phases, D.rpw, D.reg_sums, D.n, D.whole1, (int)D.perm);
  return text_done(t);
}
hipError_t launch_gemv_sliced_tok(const VptqLayerDesc& d, const VptqSlicedLayout* L, const void* x, void* y, int tokens, int flags,
                                  void* ws, hipStream_t st) {
  void* const ys[1] = {y};
  void* const wss[1] = {ws};
  return launch_gemv_sliced_tok_group(&d, L, 1, x, ys, tokens, flags, wss, st);
}

}  // namespace vptq
