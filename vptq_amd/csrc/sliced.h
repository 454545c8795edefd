// Shared by gemv_sliced.hip (one token) and gemv_sliced_tok.hip (2 - 4 tokens): launch constants, the parameter block of
// one layer and the host-side helpers that say what a layer's layout looks like.
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace vptq {

constexpr int kSLThreads = 1024;
constexpr int kSLWaves = kSLThreads / 64;
// 8 slices of 8192 entries (128 KiB of LDS) while the staged activations fit beside them, else 16 slices of 4096
// (64 KiB): 8 slices hold f16(s x) of 14336 columns (14080 with the 4 KiB residual codebook), 16 slices of 32768
constexpr int kSLMaxG8 = 14336, kSLMaxG8Res = 14080, kSLMaxG16 = 32768;
constexpr uint32_t kSLLdsLimit = 163840;
constexpr int kSLMaxRowsPerWave = 64;                    // (their block counts sit in the lanes of one register)

struct SlicedParams {
  const uint32_t* elems;
  const uint8_t* res;       // residual index per element (same order and padding), or null
  const uint32_t* rcent;    // [256][8] halves, or null
  const int32_t* blocks;    // [8][N]
  const int32_t* first;     // [8][N]
  const uint32_t* cent;     // [65536][8] halves
  const uint16_t* x;
  const uint16_t* scale;
  const uint16_t* wbias;    // input-feature order (folded arithmetic: sum b x)
  const uint16_t* cbias;    // COLUMN order (reference roundings: w = f16(f16(u * s) + b) per weight): bias_permuted or weight_bias
  const uint16_t* perm;     // column c of the quantised matrix multiplies input feature perm[c]; `scale` is then in column order
  const uint16_t* bias;
  const float* corr;        // [N x v] float32 added to the sums before the one rounding, or null: the hot blocks' exact products of
                            // VPTQ_GEMV_SELECTIVE (gemv_hot.hip), whose activations this launch reads as zeros
  // TWO tables in one launch (65536 residual centroids): the residual table's layout and codebook; its workgroups are
  // "slices" NSL .. 2 NSL - 1 of the same row blocks
  const uint32_t* elems2;
  const int32_t* blocks2;
  const int32_t* first2;
  const uint32_t* cent2;
  // what a workgroup of table t copies into LDS: tab_t bytes from cent + slice x stride_t (stride = tab: its slice of
  // the table, element words carry the index inside the slice; stride = 0: the WHOLE table - small residual tables -,
  // element words carry the full index); the staged activations start at x_off >= max(tab)
  uint32_t tab0, tab1, stride0, stride1, x_off;
  float* partial;           // [slices][N * 8]
  uint32_t* arrived;        // [row blocks] workgroups of the row block that have stored their partial sums (0 between launches)
  void* y;
  int N, G, O, rows_per_wave, n_rowblocks, out_f32;
  // several tokens in one pass (gemv_sliced.hip, TOK > 1): elements between two tokens of x / y, words between their accumulators
  int x_stride, y_stride, acc_stride;
  // ... in WINDOW PARTS (WPT): the layout's window table [slices][N][windows + 1], workgroups per (slice, row block) (2 or 4), columns
  // per layout window, columns the LDS map is laid out for (the widest part)
  const int32_t* wstart;
  int wparts, wcols, wstage;
};
constexpr int kSLWindows = VPTQ_SLICED_WINDOWS;

// ---- host side (gemv_sliced.hip)
bool sl_res256(const VptqLayerDesc& d);   // v = 8 with the 256-entry residual table: a byte per element beside the main layout
bool sl_two(const VptqLayerDesc& d);      // any other residual table: a second table with a layout of its own
uint32_t sl_tab_bytes(const VptqLayerDesc& d, int k, int whole, bool exact = false);   // bytes a workgroup of a k-entry table holds

// WHICH LAYOUTS a layer is served from in one arithmetic (the one statement the entries, the builder and vptq_sliced_layout_set read):
// parts: column parts with a layout each (0 = not served); per part `tables` consecutive structs of `slices` slices; whole[t]: every
// workgroup of table t holds all of it; side_bytes: the `res` stream beside table 0's words - 0 none / 1 uint8 / 2 uint16
// A set comes from sl_layout_set / sl_piece_set, never from a caller's own arithmetic (the one hand-built set is that of
// vptq_sliced_layout_fill, which holds its struct to the caller's SPEC); name the members when building one: their order may change.
struct SlicedLayoutSet { int parts, tables, slices, whole[2], side_bytes; bool exact; };
SlicedLayoutSet sl_layout_set(const VptqLayerDesc& d, bool exact);
// ... of a descriptor taken IN ONE PIECE (what a GEMV entry is handed: a layer, or one column part) that is gemv_sliced_eligible
SlicedLayoutSet sl_piece_set(const VptqLayerDesc& d, bool exact);
VptqLayerDesc sl_part_desc(const VptqLayerDesc& d, int parts, int p);   // column part p of `parts`: widths, column-order tensors advanced

// IS THIS VptqSlicedLayout ARRAY VALID for (d, set)?  L: n consecutive structs of one piece (repack: the parts' structs).  Returns 0,
// or the kSLFault* reasons the first bad struct (*which) is turned down for.  needs: what the caller requires of the structs -
enum : unsigned {
  kSLNeedRows = 1,      // GEMV entries: rows_per_wave in [1, 64] (and = rows_per_wave if != 0); n_slices 0 reads as 8; the `res` of an EXACT
                        // set's side stream (uint8 or uint16) set, at an even address - a folded set's `res` is not looked at
  kSLNeedLaunch = 2,    // + what only a launch's parameter fill asks: elems_per_lane 0 / 1, elems 4-byte aligned, an entry per slice; `res` set
                        // for EVERY side stream (the folded uint8 one too), an even address only of the uint16 one (the uint8 one is read by bytes)
  kSLNeedWhole = 4,     // whole_table as the set has it (the builder does not read it)
  kSLNeedBuilt = 8,     // repack / fill: `res` set IFF the set has a side stream; elems 16-byte, blocks / first / res 4-byte aligned
  kSLNeedWstart = 16,   // fill: wstart set and 4-byte aligned
  kSLNeedRes8 = 32,     // repack: a uint16 side stream 8-byte aligned (read four at a time)
};
enum : unsigned { kSLFaultTensors = 1, kSLFaultSlices = 2, kSLFaultWhole = 4, kSLFaultRes = 8, kSLFaultRows = 16, kSLFaultAlign = 32,
                  kSLFaultElemsPerLane = 64, kSLFaultFewEntries = 128 };
unsigned sl_check_layouts(const VptqLayerDesc& d, const SlicedLayoutSet& set, const VptqSlicedLayout* L, int n, unsigned needs,
                          int rows_per_wave = 0, int* which = nullptr);
// VPTQ_GEMV_COLUMN_PARTS: the parts have one y, workspace, output bias and width
bool sl_parts_share(const VptqLayerDesc* d, void* const* y, void* const* ws, int n);

}  // namespace vptq
