// The host side of the persistent chain launch (gemv_k256c.hip, gemv_k256r.hip): which layers and flags it takes, how a launch deals
// its row groups (or, in the second geometry, its workgroup-tasks) to the workgroups, the rule that picks the geometry, the
// workspace sizes, and the fill of the kernel arguments.  No device code: compiled once, an edit to a rule here recompiles neither
// kernel file.  The kernels are reached through the dispatchers of k256c.h only.
#include <vector>

#include "common.h"
#include "kernels.h"
#include "k256.h"
#include "k256c.h"

namespace vptq {

bool gemv_k256c_eligible(const VptqLayerDesc& d, int tokens) {
  return tokens == 1 && d.perm == nullptr && gemv_k256_eligible(d, 1) &&
         (((uintptr_t)d.centroids | (uintptr_t)d.res_centroids) & 15) == 0 &&
         d.num_indices <= 0xffffff && d.group_size <= 0xff * kCSweepCols;   // (the search header's fields)
}

// Row groups are dealt to the workgroups in blocks of consecutive ones, `rpw` per workgroup and
// layer.  Independent layers: at least kCMinSteps sweeps per visit of a layer (the next layer's
// image is requested at the start of the visit and lands kCLand sweeps later; a layer that gives every
// workgroup one short row group would make all of them wait for it), so a small layer occupies
// only some of the workgroups and the next layers run beside it.  Dependent layers follow each
// other anyway: every layer is spread over all workgroups.
// Longer visits, up to kCMaxSteps sweeps, while the blocks still give every workgroup two: every visit ends in a layer
// switch - the layer's last sums stored at once, its image buffer handed over, and the fast waves waiting at the next
// layer for the slowest one's part of its image (tools/chain_prof.py --exact: ~22 % of the wave time at 8 sweeps per
// visit).  Ring of 32 8192^2 layers, reference roundings: 8 -> 16 -> 32 sweeps per visit 6.2 -> 5.8 -> 5.7 us per layer.
static int c_groups(const VptqLayerDesc& d) { return (d.num_indices + kCRows - 1) / kCRows; }
// sweeps of 2048 columns of one layer: the header field every wave's column loop runs to
int gemv_k256c_sweeps(const VptqLayerDesc& d) { return (d.group_size + kCSweepCols - 1) / kCSweepCols; }
// visit = sweeps per visit a block is sized for (0: the layer's row groups spread over all workgroups)
static int c_rows_per_wg(const VptqLayerDesc& d, int cus, int visit) {
  const int ng = c_groups(d), ns = gemv_k256c_sweeps(d);
  int rpw = (ng + cus - 1) / cus;
  if (visit > 0) {
    const int want = (visit + ns - 1) / ns;
    rpw = want > rpw ? want : rpw;
  }
  return rpw < 1 ? 1 : rpw;
}
static long long c_blocks(const VptqLayerDesc* descs, int n, int cus, int visit) {
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    const int rpw = c_rows_per_wg(descs[i], cus, visit);
    total += (c_groups(descs[i]) + rpw - 1) / rpw;
  }
  return total;
}

// workgroups > 0: that many (a plan query); 0: what a launch uses
static int c_workgroups(bool dependent, int workgroups = 0) {
  static const int fw = tune_int("VPTQ_K256C_WGS", 0);  // tuning override of the workgroup count
  const int cus = workgroups > 0 ? workgroups : fw > 0 ? fw : device_cus();
  return dependent && cus > kCFlagStride ? kCFlagStride : cus;
}

// wide blocks: the longest visit of kCMaxSteps, kCMaxSteps / 2, ... kCMinSteps sweeps whose blocks still give every
// workgroup twice its share; 0 below that, and for a dependent chain
static int c_visit(const VptqLayerDesc* descs, int n, int cus, bool dependent) {
  if (dependent) return 0;
  for (int v = kCMaxSteps; v >= kCMinSteps; v /= 2)
    if (c_blocks(descs, n, cus, v) >= 2ll * cus) return v;
  return 0;
}
// does one launch of these layers fill the device (>= 3/4 of the workgroups busy)?
bool gemv_k256c_fills_device(const VptqLayerDesc* descs, int n, bool dependent) {
  const int cus = c_workgroups(dependent);
  return 4 * c_blocks(descs, n, cus, c_visit(descs, n, cus, dependent)) >= 3ll * cus;
}

// How one launch deals its row groups: the grid, the visit length, and per layer the workgroup that owns block 0 and
// the row groups per block (block k of layer i goes to workgroup (first[i] + k) mod grid).  The launch and the plan
// query (gemv_k256c_plan) take their numbers from here.
static hipError_t c_plan(const VptqLayerDesc* descs, int n, bool dependent, int cus, int* visit_out, int* grid_out,
                         int* first_wg, int* rows_per_wg) {
  if (n < 1 || n > kMaxGroup || cus < 1) return hipErrorInvalidValue;
  const int visit = c_visit(descs, n, cus, dependent);
  const long long total = c_blocks(descs, n, cus, visit);
  const int grid = (int)(total < cus ? total : cus);
  if (grid > 0xffff) return hipErrorInvalidValue;
  long long first = 0;   // running total of blocks: the layers continue each other's round robin
  for (int i = 0; i < n; ++i) {
    const int rpw = c_rows_per_wg(descs[i], cus, visit);
    const int ng = c_groups(descs[i]), ns = gemv_k256c_sweeps(descs[i]);
    if (rpw > 0xffff || ng > 0xffffff || ns > 0xff) return hipErrorInvalidValue;
    first_wg[i] = (int)(first % grid);
    rows_per_wg[i] = rpw;
    // dependent chain: every layer starts at workgroup 0 (all of its row groups wait anyway)
    first = dependent ? 0 : first + (ng + rpw - 1) / rpw;
  }
  *visit_out = visit;
  *grid_out = grid;
  return hipSuccess;
}
hipError_t gemv_k256c_plan(const VptqLayerDesc* descs, int n, bool dependent, int workgroups, int* visit, int* grid,
                           int* first_wg, int* rows_per_wg) {
  return c_plan(descs, n, dependent, c_workgroups(dependent, workgroups), visit, grid, first_wg, rows_per_wg);
}

// ---- the second geometry of the launch, "rows per wave" (gemv_k256r.hip): a wave owns a row group across the
// layer's whole width, so no sum crosses the waves.  A workgroup-task = kRTaskGroups consecutive row groups of one layer (one
// per wave; the last task of a layer may leave waves idle), r_steps(layer) steps of 128 columns long; the tasks are dealt
// round-robin over ALL `cus` workgroups, the layers continuing each other's round robin as above.
static int r_tasks(const VptqLayerDesc& d) { return (c_groups(d) + kRTaskGroups - 1) / kRTaskGroups; }
static int r_steps(const VptqLayerDesc& d) { return (d.group_size + kRStepCols - 1) / kRStepCols; }
// fp16, the reference's roundings, independent layers, 16-bit outputs (and the build's geometry constants the kernel restates)
static bool r_servable(const VptqLayerDesc* descs, int n, int flags, bool dependent) {
  if (!kRBuildServes) return false;
  if (n < 1 || n > kMaxGroup || dependent || (flags & VPTQ_GEMV_OUT_F32) || gemv_k256c_mode(flags, dependent) != kCModeExact) return false;
  for (int i = 0; i < n; ++i)
    if (descs[i].dtype != VPTQ_DTYPE_F16 || r_steps(descs[i]) > 0xffff) return false;
  return true;
}
// steps of the busiest workgroup: a step is 128 columns x 8 vector-rows per wave in both geometries
static long long r_longest(const VptqLayerDesc* descs, int n, int cus, int* first_wg, long long* total_out) {
  std::vector<long long> steps((size_t)cus, 0);
  long long first = 0;
  for (int i = 0; i < n; ++i) {
    if (first_wg) first_wg[i] = (int)(first % cus);
    const int nt = r_tasks(descs[i]);
    for (int k = 0; k < nt; ++k) steps[(size_t)((first + k) % cus)] += r_steps(descs[i]);
    first += nt;
  }
  *total_out = first;
  long long m = 0;
  for (long long s : steps) m = s > m ? s : m;
  return m;
}
static long long c_longest(const VptqLayerDesc* descs, int n, int cus, bool dependent) {
  int visit = 0, grid = 0, first_wg[kMaxGroup], rpws[kMaxGroup];
  if (c_plan(descs, n, dependent, cus, &visit, &grid, first_wg, rpws) != hipSuccess || grid < 1) return -1;
  std::vector<long long> steps((size_t)grid, 0);
  for (int i = 0; i < n; ++i) {
    const int ng = c_groups(descs[i]), ns = gemv_k256c_sweeps(descs[i]);
    for (int k = 0; k * rpws[i] < ng; ++k) {
      const int rows = (k + 1) * rpws[i] <= ng ? rpws[i] : ng - k * rpws[i];
      steps[(size_t)((first_wg[i] + k) % grid)] += (long long)rows * ns;
    }
  }
  long long m = 0;
  for (long long s : steps) m = s > m ? s : m;
  return m;
}
// THE RULE.  The rows geometry takes a launch it can serve when (a) there are at least as many workgroup-tasks as workgroups -
// the launch fills the device in this geometry - and (b) its busiest workgroup walks no more steps than the busiest one of the
// schedule above would for the same launch; both counts from the plans.  VPTQ_K256C_ROWS (VPTQ_TUNING=1): 0 never, 1 whenever
// servable; VPTQ_K256C_WGS is honoured through c_workgroups.
hipError_t gemv_k256c_rows_plan(const VptqLayerDesc* descs, int n, int flags, bool dependent, int workgroups, int* taken,
                                int* grid, int* first_wg, int* tasks, int* steps, int* longest) {
  if (!r_servable(descs, n, flags, dependent)) return hipErrorInvalidValue;
  const int cus = c_workgroups(dependent, workgroups);
  if (cus < 1 || cus > 0xffff) return hipErrorInvalidValue;
  long long total = 0;
  const long long lr = r_longest(descs, n, cus, first_wg, &total), lc = c_longest(descs, n, cus, dependent);
  if (lc < 0 || lr > 0x7fffffff || lc > 0x7fffffff) return hipErrorInvalidValue;
  for (int i = 0; i < n; ++i) {
    if (tasks) tasks[i] = r_tasks(descs[i]);
    if (steps) steps[i] = r_steps(descs[i]);
  }
  if (taken) *taken = (total >= cus && lr <= lc) ? 1 : 0;
  if (grid) *grid = cus;
  if (longest) { longest[0] = (int)lr; longest[1] = (int)lc; }
  return hipSuccess;
}
// What a LAUNCH does: the rule above (headline ring, python bench.py, same box in turns: 2825 -> 2876 GB/s, + 1.8 %, the first
// geometry's own spread 0.1 %; kernel mean 190.1 -> 186.9 us per 32 layers; profiles/r28/README.md).
// VPTQ_K256C_ROWS (VPTQ_TUNING=1): 0 = never, 1 = whenever the geometry serves the launch, 2 / unset = the rule.
bool gemv_k256c_rows(const VptqLayerDesc* descs, int n, int flags, bool dependent) {
  static const int knob = tune_int("VPTQ_K256C_ROWS", 2);
  if (knob != 1 && knob != 2) return false;
  int rule = 0;
  if (gemv_k256c_rows_plan(descs, n, flags, dependent, 0, &rule, nullptr, nullptr, nullptr, nullptr, nullptr) != hipSuccess) return false;
  return knob == 1 || rule != 0;
}

// the reference's roundings inside the chain launch: fp16, independent layers
bool gemv_k256c_exact_ok(const VptqLayerDesc& d, bool dependent) {
  (void)d;   // (bf16 since the end of round 6: its roundings on the matrix pipe)
  return !dependent && VPTQ_K256C_PROF < 2;
}
// ... and where an activation column dominates only (VPTQ_GEMV_SELECTIVE): the same, + workspace (gemv_k256c_selective_bytes)
bool gemv_k256c_selective_ok(const VptqLayerDesc& d, bool dependent) {
  return !dependent && VPTQ_K256C_PROF == 0 && d.group_size <= kHotMaxBlocks * kCBlockCols;   // (fp16 and bf16: the corrections are VALU arithmetic)
}

// bytes of a SEL launch's workspace: 16 per layer, then 4 per output
size_t gemv_k256c_selective_bytes(const VptqLayerDesc* descs, int n) {
  size_t b = ((size_t)n * 16 + 255) / 256 * 256;
  for (int i = 0; i < n; ++i) b += ((size_t)descs[i].num_indices * 8 * 4 + 255) / 256 * 256;
  return b;
}

// layers with an input permutation: x is gathered once into the caller's workspace by permute_x_kernel, in front of the chain
// launch (gemv_k256c.hip has the account)
size_t gemv_k256c_perm_bytes(const VptqLayerDesc& d) { return d.perm ? ((size_t)d.in_features * 2 + 255) / 256 * 256 : 0; }
hipError_t launch_permute_x(const VptqLayerDesc* descs, int n, const void* const* x, void* const* out, hipStream_t st) {
  PermXParams P = {};
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (!descs[i].perm) continue;
    if (P.n == kMaxGroup) return hipErrorInvalidValue;
    P.start[P.n] = blocks;
    P.x[P.n] = (const uint16_t*)x[i];
    P.perm[P.n] = (const uint16_t*)descs[i].perm;
    P.out[P.n] = (uint16_t*)out[i];
    P.I[P.n] = descs[i].in_features;
    blocks += (descs[i].in_features / 8 + 255) / 256;
    ++P.n;
  }
  if (P.n == 0) return hipSuccess;
  for (int i = P.n; i <= kMaxGroup; ++i) P.start[i] = blocks;
  return k256c_permute_x(P, blocks, st);
}

// MODE of the instantiation gemv_k256c_kernel<DT, DEP, MODE> a launch with these flags takes: 0 folded, 1 the reference's
// roundings, 2 selective; -1: none (the caller routes such a list elsewhere)
int gemv_k256c_mode(int flags, bool dependent) {
  if ((flags & VPTQ_GEMV_SELECTIVE) && !(flags & VPTQ_GEMV_EXACT)) return !dependent && VPTQ_K256C_PROF == 0 ? kCModeSel : -1;
  if (flags & VPTQ_GEMV_EXACT) return !dependent && VPTQ_K256C_PROF < 2 ? kCModeExact : -1;
  return kCModeFolded;
}

// n <= kMaxGroup layers, all gemv_k256c_eligible and of one dtype; sync = kCFlagStride flags per
// layer (zeroed by the caller's memset node) when dependent
hipError_t launch_gemv_k256c(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y,
                             int flags, bool dependent, uint32_t* sync, hipStream_t st) {
  int visit = 0, grid = 0, first_wg[kMaxGroup], rpws[kMaxGroup];
  int r_tasks_of[kMaxGroup];
  const bool rows = gemv_k256c_rows(descs, n, flags, dependent) &&
                    gemv_k256c_rows_plan(descs, n, flags, dependent, 0, nullptr, &grid, first_wg, r_tasks_of, rpws, nullptr) == hipSuccess;
  if (!rows) {
    const hipError_t e = c_plan(descs, n, dependent, c_workgroups(dependent), &visit, &grid, first_wg, rpws);
    if (e != hipSuccess) return e;
  }
  K256CParams P;
  P.n_layers = n;
  P.tokens = 1 | ((flags & VPTQ_GEMV_OUT_F32) ? kOutF32Bit : 0);
  P.sync = sync;
  for (int i = 0; i < kMaxGroup + kCHeadPad; ++i) P.head[i][0] = P.head[i][1] = 0u;
  for (int i = 0; i < n; ++i) {
    const VptqLayerDesc& d = descs[i];
    CLayerArgs& Ly = P.layer[i];
    Ly.idx = (const uint32_t*)d.indices;
    Ly.cent = (const uint32_t*)d.centroids;
    Ly.rcent = (const uint32_t*)d.res_centroids;
    Ly.x = (const uint16_t*)x[i];
    Ly.y = (uint16_t*)y[i];
    Ly.scale = (const uint16_t*)d.weight_scale;
    Ly.wbias = (const uint16_t*)d.weight_bias;
    Ly.bias = (const uint16_t*)d.bias;
    Ly.N = d.num_indices;
    Ly.G = d.group_size;
    Ly.O = d.out_features;
    Ly.row_words = d.row_words;
    const int ng = c_groups(d), ns = gemv_k256c_sweeps(d);
    Ly.wgs = first_wg[i];
    Ly.rpw = rpws[i];
    P.head[i][0] = (uint32_t)Ly.wgs | ((uint32_t)Ly.rpw << 16);
    P.head[i][1] = rows ? (uint32_t)r_tasks_of[i] : (uint32_t)ng | ((uint32_t)ns << 24);
  }
  if (rows) return launch_gemv_k256c_rows(P, grid, st);
  const bool f16 = descs[0].dtype == VPTQ_DTYPE_F16;
  const int mode = gemv_k256c_mode(flags, dependent);
  if (mode < 0) return hipErrorInvalidValue;   // (the caller routes those layer by layer / asks for EXACT)
  if (mode == kCModeSel) {
    // sync = n thresholds, written by the launch in front of the chain launch (same stream)
    if (!sync) return hipErrorInvalidValue;
    CHotArgs H = {};
    size_t off = ((size_t)n * 16 + 255) / 256 * 256;
    int max_rows = 1;
    for (int i = 0; i < n; ++i) {
      if (descs[i].group_size > kHotMaxBlocks * kCBlockCols || off > 0xffffffffull) return hipErrorInvalidValue;
      H.corr_off[i] = (uint32_t)off;
      off += ((size_t)descs[i].num_indices * 8 * 4 + 255) / 256 * 256;
      max_rows = descs[i].num_indices > max_rows ? descs[i].num_indices : max_rows;
    }
    H.kappa = selective_kappa();
    const hipError_t e = k256c_hot(P, H, f16, (max_rows + kHotRows - 1) / kHotRows, st);
    if (e != hipSuccess) return e;
  }
  return k256c_chain(P, f16, dependent, mode, grid, st);
}

}  // namespace vptq
