// Shared by gemv_sliced.hip (one token), gemv_sliced_tok.hip (2 - 8 tokens) and sliced_host.hip (the family's host side: which layouts
// serve a layer, what makes one valid, what one launch is): launch constants, the kernels' parameter blocks, the host rules the rest
// of the library reads and the instantiation dispatchers the host side launches through.
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
// Up to kSLMaxGroup layers that read the SAME activation (q / k / v, gate / up) in one launch: layer l owns the workgroups
// [start[l], start[l + 1]).  One launch instead of n: the fixed part of a launch (boundary, slice copy, staging, the
// cross-slice hand-over: ~7 of the 10 us of a 4096 x 4096 layer) is paid once.
constexpr int kSLMaxGroup = 3;
struct SlicedGroupParams {
  int n;
  int arrivals;   // workgroups that add into an output's accumulator word: (tables x) slices - x n where the "layers" are COLUMN PARTS of one
  int start[kSLMaxGroup + 1];
  SlicedParams p[kSLMaxGroup];
};

// ---- gemv_sliced_tok.hip: 2 - 8 tokens in column phases
constexpr int kSTWindows = VPTQ_SLICED_WINDOWS;
constexpr int kSTRegRows = 4;   // rows per wave whose sums (4 registers each in matrix-pipe mode) are kept in registers
struct SlicedTokParams {
  SlicedParams p;            // as for one token; x / y: token 0, rows_per_wave / n_rowblocks: this launch's
  const int32_t* wstart;     // [slices][N][kSTWindows + 1]
  const int32_t* wstart2;    // second table
  const uint16_t* xs;        // the activations in COLUMN order: p.x, or the pre-pass's x[perm] (p.scale is in column order too)
  int tokens;                // 2 .. TOK
  int phases;                // 1, 2 or 4
  int wcols;                 // columns per layout window
  int x_stride, x_in_stride, y_stride;    // elements between two tokens of xs / p.x / y
  uint32_t bd_off, res_off, sum_off;   // LDS: sum b x parts [TOK][16 waves] floats; 256-entry residual table; row sums
  uint32_t sb_off;           // EX: LDS, per staged column 8 bytes {s, b, s, b} (and the zero column's zeros)
  int reg_sums;              // (matrix-pipe mode, <= kSTRegRows rows per wave) the rows' sums stay in registers: no LDS for them
};
// Up to kSTMaxGroup layers that read the SAME activations (q / k / v, gate / up) in one launch, as in gemv_sliced.hip: layer l
// owns the workgroups [start[l], start[l + 1]); the fixed part of a launch is paid once.
constexpr int kSTMaxGroup = 3;
struct SlicedTokGroupParams {
  int n;
  int start[kSTMaxGroup + 1];
  SlicedTokParams p[kSTMaxGroup];
};

// ---- instantiation dispatchers: the ONLY way from the host side (sliced_host.hip) into the kernel files.  Each launches the
// instantiation the decision names (and turns a decision down that names none of its own); gemv_sliced.hip, parts 1 / 2 / 3 ...
hipError_t launch_sl_one(const SlicedDecision& D, const SlicedGroupParams& P, uint32_t lds, hipStream_t st);          // one token
hipError_t launch_sl_tokens(const SlicedDecision& D, const SlicedGroupParams& P, uint32_t lds, hipStream_t st);       // 2 / 3 tokens, reference roundings
hipError_t launch_sl_tokens_wpt(const SlicedDecision& D, const SlicedGroupParams& P, uint32_t lds, hipStream_t st);   // ... in window parts
// ... gemv_sliced_tok.hip, parts 1 / 2 / 3 / 4: 2 and 4 token slots, 8 slots, 4 / 8 slots in the reference's roundings
hipError_t launch_st_tok24(const SlicedTokDecision& D, const SlicedTokGroupParams& P, int grid, uint32_t lds, hipStream_t st);
hipError_t launch_st_tok8(const SlicedTokDecision& D, const SlicedTokGroupParams& P, int grid, uint32_t lds, hipStream_t st);
hipError_t launch_st_ex4(const SlicedTokDecision& D, const SlicedTokGroupParams& P, int grid, uint32_t lds, hipStream_t st);
hipError_t launch_st_ex8(const SlicedTokDecision& D, const SlicedTokGroupParams& P, int grid, uint32_t lds, hipStream_t st);

// ---- host side (sliced_host.hip)
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
