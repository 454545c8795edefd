// Internal launcher prototypes (one per .hip translation unit).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vptq_hip.h"
#include "launch.h"

namespace vptq {

// What one launch of the remaining GEMV families IS - the instantiation's template arguments and the launch-shape facts: each
// family's *_decide is read by its launcher AND printed by vptq_quant_gemv_instance / vptq_quant_gemv_v2_instance (abi.hip), so the
// text is the launch's own decision.  tokens (and flags): those of ONE launch, as the entries hand them over.
struct GenericDecision { bool f16; int v, tok; };                         // gemv_generic_kernel<DT, V, TOK>
struct V2Decision { bool f16; int v, tok; };                              // gemv_v2_kernel<DT, V, TOK>
struct GatherDecision { bool f16, perm, wide; int T, rows, tok; };        // gemv_gather_kernel<DT, T, ROWS, TOK, PERM, WIDE>
struct GatherXDecision {                                                  // gemv_gatherx_kernel<DT, V, TOK, PERM>
  bool f16, perm, res_lds;   // res_lds: the residual table (<= 32 KiB) gathered from LDS, else from L2
  int v, tok, ov, groups;    // ov: the outlier codebook's vector length (0: no outlier columns); codebook groups
};
struct LdsDecision {         // gemv_lds_kernel<DT, FMT, TOK> / gemv_lds_mfma_kernel<DT, FMT>
  bool ok, mfma, f16, dma, perm;   // ok: a launch exists; dma: the main table copied by LDS-DMA (k a multiple of 64), else through registers
  int fmt, tok, rw, n_groups, grid, lds, stages;   // rw vector-rows per row group; stages: staging passes of 8192 columns (MFMA kernel)
};
GenericDecision gemv_generic_decide(const VptqLayerDesc& d, int tokens);
V2Decision gemv_v2_decide(const VptqV2Desc& d, int tokens);
GatherDecision gemv_gather_decide(const VptqLayerDesc& d, int tokens);
GatherXDecision gemv_gatherx_decide(const VptqLayerDesc& d, int tokens);
LdsDecision gemv_lds_decide(const VptqLayerDesc& d, int tokens, int flags, const void* x = nullptr);   // x = NULL: assumed aligned
LdsDecision gemv_lds_v2_decide(const VptqV2Desc& d, int tokens, int flags, const void* x = nullptr);
const char* gemv_lds_fmt_text(int fmt);   // "12" ... "22", "v2", "v2u8", "v2u16"

// gemv_generic.hip — every configuration
hipError_t launch_gemv_generic(const VptqLayerDesc& d, const void* x, void* y, int tokens,
                               bool out_f32, hipStream_t st);

// gemv_k256.hip — v=8, k=256 (+ kr=256), C=1, no outliers: LDS-resident,
// bank-conflict-free replicated codebooks.
bool gemv_k256_eligible(const VptqLayerDesc& d, int tokens);
const char* gemv_k256_name(const VptqLayerDesc& d, int tokens, int flags);
const char* gemv_k256_group_name(const VptqLayerDesc* descs, int n, int tokens, int flags);
// the instantiation(s) launch_gemv_k256 would launch, as text (vptq_quant_gemv_grouped_instance); 0, -1: no kernel, -2: buffer too small
int gemv_k256_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes);
hipError_t launch_gemv_k256(const VptqLayerDesc* descs, int n, const void* const* x,
                            void* const* y, int tokens, int flags, hipStream_t st);

// gemv_k256c.hip - the same format, one token, no permutation: ONE persistent launch that walks a
// chain of layers (next layer's codebook image, activations and index words requested while the current
// one streams).  n <= 32 layers of one dtype per launch.  The rules and launchers declared here are its host side's
// (k256c_host.hip; the dispatchers into the kernel files, for that unit's own use, in k256c.h).
bool gemv_k256c_eligible(const VptqLayerDesc& d, int tokens);
bool gemv_k256c_fills_device(const VptqLayerDesc* descs, int n, bool dependent);
bool gemv_k256c_exact_ok(const VptqLayerDesc& d, bool dependent);
bool gemv_k256c_selective_ok(const VptqLayerDesc& d, bool dependent);
size_t gemv_k256c_selective_bytes(const VptqLayerDesc* descs, int n);
// layers with an input permutation in an independent chain: x[perm] gathered into a workspace in front of the launch
size_t gemv_k256c_perm_bytes(const VptqLayerDesc& d);
hipError_t launch_permute_x(const VptqLayerDesc* descs, int n, const void* const* x, void* const* out, hipStream_t st);   // VPTQ_GEMV_EXACT inside the chain launch
hipError_t launch_gemv_k256c(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y,
                             int flags, bool dependent, uint32_t* sync, hipStream_t st);
// what that launch is: MODE of gemv_k256c_kernel<DT, DEP, MODE> for these flags (0 folded, 1 reference roundings, 2 selective;
// -1: no such launch) and a layer's sweeps of 2048 columns
int gemv_k256c_mode(int flags, bool dependent);
int gemv_k256c_sweeps(const VptqLayerDesc& d);
// how that launch deals its row groups (vptq_quant_gemv_chain_plan); workgroups = 0: what a launch uses
hipError_t gemv_k256c_plan(const VptqLayerDesc* descs, int n, bool dependent, int workgroups, int* visit, int* grid,
                           int* first_wg, int* rows_per_wg);
// the launch's second geometry, "rows per wave" (gemv_k256c_rows_kernel, gemv_k256r.hip): does a launch of these layers take it
// (the rule: k256c_host.hip, gemv_k256c_rows_plan), and how it would deal its workgroup-tasks
// (vptq_quant_gemv_chain_rows_plan; hipErrorInvalidValue: the geometry does not serve this launch).  Any out pointer may be null.
bool gemv_k256c_rows(const VptqLayerDesc* descs, int n, int flags, bool dependent);
hipError_t gemv_k256c_rows_plan(const VptqLayerDesc* descs, int n, int flags, bool dependent, int workgroups, int* taken,
                                int* grid, int* first_wg, int* tasks, int* steps, int* longest);

// gemv_gather.hip — v=8, k=65536 (+ residual 0 / 256 / 65536), C=1, no outliers:
// centroid rows gathered from L2.
// max_tokens: the most tokens one launch takes - 8 here, 16 for gemm_gather.hip over the same layers
bool gemv_gather_eligible(const VptqLayerDesc& d, int tokens, int max_tokens = 8);
hipError_t launch_gemv_gather(const VptqLayerDesc& d, const void* x, void* y, int tokens,
                              bool out_f32, hipStream_t st);

// gemv_gatherx.hip - every vector length, any codebook sizes (any total index width), several codebook
// groups, outlier columns of the same vector length: codebook rows gathered from L2 (what gemv_gather / gemv_lds do not take)
bool gemv_gatherx_eligible(const VptqLayerDesc& d, int tokens);
int gemv_gatherx_max_chunk(const VptqLayerDesc& d);   // token slots of one launch: 8 (v <= 8) or 4
hipError_t launch_gemv_gatherx(const VptqLayerDesc& d, const void* x, void* y, int tokens,
                               bool out_f32, hipStream_t st);

// gemv_lds.hip - v=8, one codebook, 256 < k <= 8192, kr <= 512: both codebooks LDS-resident,
// packed bit stream (T in {12, 13, 20, 21, 22}) or the v2 wire format
bool gemv_lds_eligible(const VptqLayerDesc& d, int tokens, int flags);
int gemv_lds_max_chunk(int dtype);
const char* gemv_lds_name(const VptqLayerDesc& d, int tokens, int flags);
// flags: VPTQ_GEMV_EXACT keeps one-token launches on the kernel with the reference's roundings
hipError_t launch_gemv_lds(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32,
                           int flags, hipStream_t st);
bool gemv_lds_v2_eligible(const VptqV2Desc& d, int tokens);
hipError_t launch_gemv_lds_v2(const VptqV2Desc& d, const void* x, void* y, int tokens, bool out_f32,
                              int flags, hipStream_t st);

// gemv_sliced.hip - v8-k65536-0, one token, over the load-time derived sliced layout (LDS-local gathers); the rules and launchers
// declared here are its host side's (sliced_host.hip; more of them, for the library's own use, in sliced.h)
// exact: the reference's roundings per weight (VPTQ_GEMV_EXACT) - scale and bias staged per column beside the activations
// (6 instead of 2 bytes of LDS per column: more slices for wide layers), one table only
bool gemv_sliced_eligible(const VptqLayerDesc& d, bool exact = false);
int gemv_sliced_slices(const VptqLayerDesc& d, bool exact = false);
int gemv_sliced_tables(const VptqLayerDesc& d);
int gemv_sliced_whole_table(const VptqLayerDesc& d, int table);   // VptqSlicedLayout::whole_table the layout of `table` must have   // layouts the layer needs: 1, or 2 (a residual codebook served as a second table)
size_t gemv_sliced_workspace_bytes(const VptqLayerDesc& d);
// gemv_hot.hip - VPTQ_GEMV_SELECTIVE over the sliced layouts: thresholds, x with the hot blocks zeroed, the hot blocks' exact products
bool gemv_hot_eligible(const VptqLayerDesc& d);
// the threshold factor kappa of VPTQ_GEMV_SELECTIVE (here and in gemv_k256c.hip): 6, or VPTQ_SELECTIVE_KAPPA (to a thousandth)
inline float selective_kappa() {
  static const int milli = [] { const char* e = tune_env("VPTQ_SELECTIVE_KAPPA"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? (int)(v * 1000.0) : 6000; }();
  return (float)milli * 1e-3f;
}
size_t gemv_hot_bytes(const VptqLayerDesc& d);
hipError_t launch_gemv_hot(const VptqLayerDesc& d, const void* x, void* extra, const void** x_masked, const float** corr, hipStream_t st);
hipError_t launch_gemv_sliced(const VptqLayerDesc& d, const VptqSlicedLayout* L, const void* x, void* y, int flags,
                              void* ws, hipStream_t st, const float* corr = nullptr);
// up to 3 layers of one format reading the same x (q / k / v, gate / up) in one launch
// gemv_sliced_tok.hip - 2 - 8 tokens over the same layouts (column windows of every list, phase by phase); host side: sliced_host.hip
bool gemv_sliced_tok_eligible(const VptqLayerDesc& d, const VptqSlicedLayout* L, int tokens, bool exact = false);
int gemv_sliced_tok_one_pass_parts(const VptqLayerDesc& d, int tokens, bool exact);   // 0: column phases / not served; 1, 2, 4: one pass, that many window parts
size_t gemv_sliced_tok_workspace_bytes(const VptqLayerDesc& d, int tokens);
hipError_t launch_gemv_sliced_tok(const VptqLayerDesc& d, const VptqSlicedLayout* L, const void* x, void* y, int tokens, int flags,
                                  void* ws, hipStream_t st);
bool gemv_sliced_tok_groupable(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, int tokens, bool exact = false);
hipError_t launch_gemv_sliced_tok_group(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, const void* x, void* const* y,
                                        int tokens, int flags, void* const* ws, hipStream_t st);
bool gemv_sliced_groupable(const VptqLayerDesc* d, int n, bool exact = false);
hipError_t launch_gemv_sliced_group(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, const void* x, void* const* y,
                                    int flags, void* const* ws, hipStream_t st, int tokens = 1, const float* corr = nullptr);
// what one launch of the sliced family IS - the instantiation's template arguments and the launch shape: decided once per call
// (sliced_host.hip: sl_decide, st_decide; gemv_hot_decide), checked by the launchers against their template arguments
// and printed by the *_instance functions (vptq_quant_gemv_sliced_instance / _tokens_instance): 0, -1: no launch, -2: buffer too small
struct SlicedDecision {
  bool f16, res, two, ex, rg, wpt;   // gemv_sliced_kernel<DT, NSL, RES, V, TWO, EX, RG, TOK, WPT>
  int nsl, v, tok;
  int wparts, parts, n, rpw, arrivals, whole1, side;   // window parts, column parts, members, rows per wave, arrivals per accumulator
  bool perm, corr;                                     // word, the second table held whole, bytes of the side stream; a permutation; SELECTIVE's products
};
struct SlicedTokDecision {
  bool f16, res, two, ex;            // gemv_sliced_tok_kernel<DT, NSL, RES, V, TWO, TOK, EX>
  int nsl, v, tok;
  int phases, rpw, reg_sums, n, whole1;
  bool perm;                         // the permute_x pre-pass runs
};
struct HotDecision { bool ok, f16; int v; };   // gemv_hot_kernel<DT, V>
HotDecision gemv_hot_decide(const VptqLayerDesc& d);
int gemv_hot_instance(const VptqLayerDesc& d, char* buf, size_t bytes);
int gemv_sliced_instance(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, int tokens, int flags, bool corr, char* buf, size_t bytes);
int gemv_sliced_tok_instance(const VptqLayerDesc* d, const VptqSlicedLayout* L, int n, int tokens, int flags, char* buf, size_t bytes);
// (VPTQ_GEMV_EXACT) 2 / 3 tokens in ONE pass of the one-token kernel: x [tokens][in], y[i] [tokens][out], ws[i]: accumulator words
bool gemv_sliced_exact_tokens_ok(const VptqLayerDesc& d, int tokens);
int gemv_sliced_exact_tokens_parts(const VptqLayerDesc& d, int tokens);   // 0: not served; 1: all columns staged; 2 / 4: window parts (needs wstart)
size_t gemv_sliced_exact_tokens_workspace_bytes(const VptqLayerDesc& d, int tokens);
// repack.hip - the packed index stream of a layer rebuilt from its exact sliced layout(s) (vptq_sliced_layout_repack)
size_t sliced_repack_lds_bytes(const VptqLayerDesc& d);
hipError_t launch_sliced_repack(const VptqLayerDesc& d, const VptqSlicedLayout* L, int parts, int side_bytes, void* out, hipStream_t st);   // side_bytes: SlicedLayoutSet's
// dequant_sliced.hip - the dense W straight from a layer's exact sliced layout(s) (vptq_dequant_sliced); reads d.perm, not d.inv_perm
bool dequant_sliced_eligible(const VptqLayerDesc& d);
hipError_t launch_dequant_sliced(const VptqLayerDesc& d, const VptqSlicedLayout* L, int parts, int side_bytes, void* W, hipStream_t st);   // side_bytes: SlicedLayoutSet's
// layout_build.hip - a sliced layout built from the packed index stream (vptq_sliced_layout_plan / vptq_sliced_layout_fill)
struct LayoutBuildParams {
  const uint32_t* packed;   // [N][row_words]
  int32_t* blocks;          // [S][N]
  int32_t* first;           // [S][N]
  int32_t* wstart;          // [S][N][VPTQ_SLICED_WINDOWS + 1]
  long long* total;         // plan: the number of blocks (device)
  uint32_t* elems;          // fill
  void* res;                // fill: uint8 / uint16 side stream, or NULL
  long long total_blocks;   // fill: blocks `elems` (and `res`) have room for - nothing is stored past them
  int N, row_words, T;
  int c0, W;                // the columns [c0, c0 + W) of the row this layout is for (a column part, or all of them)
  int wcols, cap;           // window width; the widest window
  int S, slice_bits;        // slices; bits of the index inside a slice
  int bucket_shift;         // the bucket index = (field >> bucket_shift) & bucket_mask: the main index, or the residual one
  uint32_t bucket_mask;
  int whole;                // slices are equal column ranges, the word carries the whole bucket index
  int side, side_shift;     // side stream: 0 none, 1 uint8, 2 uint16 = field >> side_shift
};
size_t layout_fill_lds_bytes(const LayoutBuildParams& a);
hipError_t launch_layout_plan(const LayoutBuildParams& a, hipStream_t st);
hipError_t launch_layout_fill(const LayoutBuildParams& a, hipStream_t st);
// gemm_k256t.hip - canonical format, fp16 / bf16, up to 16 tokens in one pass over the indices (transposing
// gather -> 16x16x32 MFMA with tokens as M; folded arithmetic; needs a workspace for the operand-ordered activations)
bool gemm_k256t_eligible(const VptqLayerDesc& d, int tokens, int flags);
size_t gemm_k256t_workspace_bytes(const VptqLayerDesc& d);
struct GemmK256TDecision { bool f16, perm; int n_groups, n_sweeps, grid, groups_per_wg; };   // what launch_gemm_k256t launches
GemmK256TDecision gemm_k256t_decide(const VptqLayerDesc& d);
hipError_t launch_gemm_k256t(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, void* ws,
                             hipStream_t st);
// gemm_k256.hip - canonical format, fp16, up to 16 tokens in one launch (tokens = MFMA M)
bool gemm_k256_eligible(const VptqLayerDesc& d, int tokens, int flags);
// what launch_gemm_k256 launches; passes: bit mask of the NRG = 4 / 2 / 1 passes the busiest workgroup runs
struct GemmK256Decision { bool f16, perm; int n_groups, grid, passes; };
GemmK256Decision gemm_k256_decide(const VptqLayerDesc& d);
hipError_t launch_gemm_k256(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32,
                            hipStream_t st);
// the same file: gemm_k256_eligible's layers, 17 - 64 tokens in one launch as tb = 2 ... 4 blocks of 16 tokens of gemm_k256's pass
// (reference roundings; gemm_k256's K-step -> wave mapping and order of sums: a token's bits are the 16-token kernel's)
bool gemm_k256w_eligible(const VptqLayerDesc& d, int tokens);
// what launch_gemm_k256w launches: gemm_k256w_kernel<DT, PERM, TB>, whose passes are gemm_k256_pass<DT, PERM, 1, TB>; rgs: the row
// groups the busiest workgroup walks
struct GemmK256WDecision { bool f16, perm; int tok, tb, n_groups, grid, rgs; };
GemmK256WDecision gemm_k256w_decide(const VptqLayerDesc& d, int tokens);
hipError_t launch_gemm_k256w(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st);
// the same file: 2 - 4 sibling layers of gemm_k256_eligible (one dtype and width), 1 - 48 tokens, in ONE launch of
// gemm_k256_grouped_kernel<DT, TB>, whose workgroups walk the members' row groups as one list; plain form only - the caller hands a
// member with a permutation over as gemm_gather_px_plain(d), with x[perm] for its x.  groups: row groups per member, first_group: their
// running sum; total and grid = min(total, CUs) over the whole list; rgs: the most row groups of any workgroup; passes: bit mask of every
// NRG = 4 / 2 / 1 pass any workgroup runs in any member (tb > 1: 1)
struct GemmK256GroupedDecision { bool f16; int tok, tb, n, total, grid, rgs, passes, groups[4], first_group[5]; };
GemmK256GroupedDecision gemm_k256_grouped_decide(const VptqLayerDesc* descs, int n, int tokens);
hipError_t launch_gemm_k256_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                    hipStream_t st);

// gemm_gather.hip - gemv_gather's layers (v = 8, k = 65536, residual 0 / 256 / 65536), up to 16 tokens in one launch (tokens = MFMA M;
// centroid rows gathered from L2, the rebuilt tile in LDS in operand order; reference roundings; no workspace).  The kernels'
// argument block, its fill and the launch-shape arithmetic are gemm_gather_host.h's, the device phases gemm_gather_tile.h's: shared with gemm_gatherx.hip
bool gemm_gather_eligible(const VptqLayerDesc& d, int tokens);
// what launch_gemm_gather launches: gemm_gather_kernel<DT, T, PERM>; tiles: column tiles per row group; rgs: the most row groups
// one workgroup walks
struct GemmGatherDecision { bool f16, perm; int T, tok, tiles, n_groups, grid, rgs; };
GemmGatherDecision gemm_gather_decide(const VptqLayerDesc& d, int tokens);
hipError_t launch_gemm_gather(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st);
// the same file: 2 - 4 sibling layers (one dtype, width and index width T) in ONE launch of gemm_gather_grouped_kernel<DT, T>, whose
// workgroups walk the members' row groups as one list; plain form only - the caller hands a member with a permutation over as its
// descriptor without one, with x[perm] for its x.  groups: row groups per member, first_group: their running sum; total, grid, rgs
// over the whole list
struct GemmGatherGroupedDecision { bool f16; int T, tok, n, tiles, total, grid, rgs, groups[4], first_group[5]; };
GemmGatherGroupedDecision gemm_gather_grouped_decide(const VptqLayerDesc* descs, int n, int tokens);
hipError_t launch_gemm_gather_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                      hipStream_t st);

// gemm_gatherw.hip - gemm_gather's layers, 17 - 48 tokens in one launch as tb = 2 / 3 blocks of 16 tokens over gemm_gather's tile
// pipeline (its K-step -> wave mapping and order of sums: a token's bits are the 16-token kernel's)
bool gemm_gatherw_eligible(const VptqLayerDesc& d, int tokens);
// what launch_gemm_gatherw launches: gemm_gatherw_kernel<DT, T, PERM, TB>; tiles and rgs as above
struct GemmGatherWDecision { bool f16, perm; int T, tok, tb, tiles, n_groups, grid, rgs; };
GemmGatherWDecision gemm_gatherw_decide(const VptqLayerDesc& d, int tokens);
hipError_t launch_gemm_gatherw(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st);
// gemm_gatherw_grouped.hip - 2 - 4 sibling layers of gemm_gatherw (one dtype, width and index width T), 17 - 48 tokens, in ONE launch
// of gemm_gatherw_grouped_kernel<DT, T, TB>: gemm_gatherw's pass behind gemm_gather_grouped's member walk; plain form only - the caller
// hands a member with a permutation over as its descriptor without one, with x[perm] for its x.  groups, first_group, total as
// GemmGatherGroupedDecision's; grid = min(total, CUs x 4), rgs over the whole list
struct GemmGatherWGroupedDecision { bool f16; int T, tok, tb, n, tiles, total, grid, rgs, groups[4], first_group[5]; };
GemmGatherWGroupedDecision gemm_gatherw_grouped_decide(const VptqLayerDesc* descs, int n, int tokens);
hipError_t launch_gemm_gatherw_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                       hipStream_t st);

// gemm_gatherx.hip - the large-codebook layers gemm_gather does not take (v = 8 / 16, 16384 ... 65536 main centroids, any residual
// codebook, any total index width), up to 16 tokens in one launch: gemm_gather's structure with gemv_gatherx's index path
bool gemm_gatherx_eligible(const VptqLayerDesc& d, int tokens);
// what launch_gemm_gatherx launches: gemm_gatherx_kernel<DT, V, RES, PERM> (res: 0 none, 1 table in LDS, 2 gathered from L2) with the
// run-time index widths ib / rb; lds: dynamic LDS bytes (tile + table), wgcu: the workgroups per CU that LDS leaves; rgs as above
struct GemmGatherXDecision { bool f16, perm; int v, ib, rb, res, res_bytes, tok, tiles, lds, wgcu, n_groups, grid, rgs; };
GemmGatherXDecision gemm_gatherx_decide(const VptqLayerDesc& d, int tokens);
hipError_t launch_gemm_gatherx(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st);
// gemm_gatherx_grouped.hip - 2 - 4 sibling layers of gemm_gatherx (one dtype, width and format: v, main and residual codebook size),
// 1 - 16 tokens, in ONE launch of gemm_gatherx_grouped_kernel<DT, V, RES>: gemm_gatherx's row-group body behind gemm_gather_grouped's
// member walk; plain form only - the caller hands a member with a permutation over as its descriptor without one, with x[perm] for
// its x.  v ... wgcu: gemm_gatherx_decide's of the first member; groups, first_group, total as GemmGatherGroupedDecision's; grid =
// min(total, CUs x wgcu), rgs over the whole list
struct GemmGatherXGroupedDecision { bool f16; int v, ib, rb, res, res_bytes, tok, n, tiles, lds, wgcu, total, grid, rgs, groups[4], first_group[5]; };
GemmGatherXGroupedDecision gemm_gatherx_grouped_decide(const VptqLayerDesc* descs, int n, int tokens);
hipError_t launch_gemm_gatherx_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                       hipStream_t st);

// gemm_gather_px.hip - a layer with a column permutation through the three kernels above in their forms WITHOUT one: xp[t][c] =
// x[t][perm[c]] written once per call into a workspace (permute_x_tokens_kernel), then the layer's kernel over gemm_gather_px_plain(d)
// - scale_permuted / bias_permuted as scale / bias, no permutation - with x = xp: the bits of the layer's own entry
size_t gemm_gather_px_workspace_bytes(const VptqLayerDesc& d, int tokens);   // 0 without a permutation
// what launch_permute_x_tokens launches: grid_x workgroups of 64 chunks of 8 columns x grid_y slices of tpt tokens
struct GemmGatherPxDecision { bool perm; int g, tok, tpt, grid_x, grid_y; };
GemmGatherPxDecision gemm_gather_px_decide(const VptqLayerDesc& d, int tokens);
VptqLayerDesc gemm_gather_px_plain(const VptqLayerDesc& d);
hipError_t launch_permute_x_tokens(const VptqLayerDesc& d, const void* x, void* xp, int tokens, hipStream_t st);

// gemm_fused.hip - canonical format, many tokens: dequantised tile -> LDS -> 32x32x16 MFMA
bool gemm_fused_eligible(const VptqLayerDesc& d);
size_t gemm_fused_workspace_bytes(const VptqLayerDesc& d, int tokens);
hipError_t launch_gemm_fused(const VptqLayerDesc& d, const void* x, void* y, int tokens, void* workspace,
                             size_t workspace_bytes, hipStream_t st);

// dequant.hip; dequant_instance: the instantiation and the per-chunk paths launch_dequant(d, W) takes, as text (vptq_dequant_instance;
// 0, -2: buffer too small) - the launch decision and the kernel's own predicates (dequant_paths.h)
hipError_t launch_dequant(const VptqLayerDesc& d, void* W, hipStream_t st);
int dequant_instance(const VptqLayerDesc& d, const void* W, char* buf, size_t bytes);

// gemv_v2.hip
hipError_t launch_gemv_v2(const VptqV2Desc& d, const void* x, void* y, int tokens,
                          bool out_f32, hipStream_t st);

}  // namespace vptq
