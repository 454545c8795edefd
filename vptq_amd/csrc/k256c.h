// What the kernels of the persistent chain launch (gemv_k256c.hip: waves split the columns of a sweep; gemv_k256r.hip: waves own
// their rows across the full width) and their host side (k256c_host.hip) share: the build's knobs and geometry constants, the
// kernel-argument blocks and their scalar loads, the device phases both geometries run, and the dispatchers into the kernel files.
#pragma once
#include <stddef.h>

#include "common.h"
#include "k256.h"

namespace vptq {

constexpr uint32_t kCImgBytes = 65536;               // one codebook image: 256 rows x 16 units x 16 B

// profiling build (tools/chain_prof.py): every wave adds up the shader-clock cycles it spends
// waiting for its index words, consuming a sweep, requesting the next one and in the rare paths,
// and stores them at P.sync[(workgroup * waves + wave) * kCProfWords ...] (non-dependent launches); 2: + a timeline
#ifndef VPTQ_K256C_PROF
#define VPTQ_K256C_PROF 0
#endif
// waves per workgroup (= per CU): 16 (4 per SIMD, 128 registers each) or 8 (2 per SIMD, 256 registers: room for 4 row
// subgroups per sweep and a deeper gather lookahead; a step then covers twice the indices per wave)
#ifndef VPTQ_K256C_WAVES
#define VPTQ_K256C_WAVES 16
#endif
constexpr int kCWaves = VPTQ_K256C_WAVES;
constexpr int kCThreads = 64 * kCWaves;
static_assert(kCWaves == 16 || kCWaves == 8, "waves per workgroup");
constexpr int kCBlockCols = 128;                     // columns of one wave per sweep
// The waves of a workgroup as kCSplit row parts x kCColWaves column blocks: a sweep covers kCColWaves x 128 columns
// of kCSplit x 8 vector-rows.  2 parts: a row group of an 8192-column layer is 8 sweeps instead of 4, so the sums
// at the end of a row group (cross-lane reduction, deposit, hand-over: ~1500 clocks per wave) come half as often;
// the sum over the waves is over 8 instead of 16 partial sums.
#ifndef VPTQ_K256C_SPLIT
#define VPTQ_K256C_SPLIT 1
#endif
constexpr int kCSplit = VPTQ_K256C_SPLIT;
static_assert(kCSplit == 1 || kCSplit == 2 || kCSplit == 4, "row parts");
constexpr int kCColWaves = kCWaves / kCSplit;
static_assert(kCColWaves >= 4, "the sum over the waves is a tree of groups of 4");
constexpr int kCSweepCols = kCColWaves * kCBlockCols;   // 2048
#ifndef VPTQ_K256C_SUB
#define VPTQ_K256C_SUB 2
#endif
constexpr int kCSub = VPTQ_K256C_SUB;                // row subgroups (4 vector-rows each) per row group
constexpr int kCRowsW = 4 * kCSub;                   // vector-rows of one wave
constexpr int kCOutW = 8 * kCRowsW;                  // outputs of one wave
constexpr int kCRows = kCRowsW * kCSplit;            // vector-rows per row group
constexpr int kCOut = 8 * kCRows;                    // outputs per row group
static_assert(kCSub == 1 || kCSub == 2 || kCSub == 4, "row subgroups per sweep");
static_assert(kCSub != 1 || (kCWaves == 16 && kCSplit == 1), "1 subgroup: the 16-wave sum");
// gathers requested ahead of the arithmetic, in units (one index of one subgroup)
#ifndef VPTQ_K256C_AHEAD
#define VPTQ_K256C_AHEAD 2
#endif
// sweeps in flight per wave: bandwidth x latency is ~48 KiB per CU
#ifndef VPTQ_K256C_DEPTH
#define VPTQ_K256C_DEPTH 3
#endif
constexpr int kCDepth = VPTQ_K256C_DEPTH;
static_assert(kCDepth >= 2 && kCDepth <= 6, "queue depth");
constexpr int kCSlots = 4;                           // cross-wave partial-sum slots
constexpr uint32_t kCXsOff = 2 * kCImgBytes;         // wave-private activation slots
// arithmetic of a launch: folded (sum (c + r) f16(s x) + sum b x), the reference's roundings per weight, or SELECTIVE:
// the folded form, with the reference's roundings wherever an activation column dominates (kCModeSel below)
constexpr int kCModeFolded = 0, kCModeExact = 1, kCModeSel = 2;
// folded form (and selective): 256 bytes per wave (f16(s x) of its 128 columns); reference roundings: x, scale, bias side by side
constexpr uint32_t c_xs_wave(int mode) { return mode == kCModeExact ? 768u : 256u; }
constexpr uint32_t c_red_off(int mode) { return kCXsOff + kCWaves * c_xs_wave(mode); }
constexpr uint32_t c_redb_off(int mode) { return c_red_off(mode) + kCSlots * kCWaves * kCOutW * 4; }
constexpr uint32_t c_cnt_off(int mode) { return c_redb_off(mode) + kCSlots * kCWaves * 4; }
// profiling build 2: consume start / end stamps of kCTlSteps steps per wave (a timeline of who computes when)
[[maybe_unused]] constexpr int kCTlFirst = 16, kCTlSteps = 32;
constexpr uint32_t c_tl_off(int mode) { return c_cnt_off(mode) + 64; }
constexpr uint32_t c_lds_bytes(int mode) {
#if VPTQ_K256C_PROF >= 2
  return c_tl_off(mode) + kCWaves * kCTlSteps * 8;
#else
  return c_cnt_off(mode) + 64;
#endif
}
[[maybe_unused]] constexpr int kCProfWords = 64;   // 8-byte words of profile output per wave
static_assert(c_lds_bytes(kCModeFolded) <= 163840 && (VPTQ_K256C_PROF >= 2 || c_lds_bytes(kCModeExact) <= 163840), "LDS");
constexpr int kCFlagStride = 256;   // DEP: arrival flags per layer (one per workgroup)

// timing-only ablations (results wrong): bit 0 no MFMAs, bit 1 no gathers, bit 2 no x / scale /
// bias loads, bit 3 no waits for the image hand-over between the waves, bit 4 no index loads
#ifndef VPTQ_K256C_ABLATE
#define VPTQ_K256C_ABLATE 0
#endif
// bring-up builds: give up a wait after that many polls, so that a protocol error shows as wrong
// results instead of a hung GPU
#ifndef VPTQ_K256C_SPIN_LIMIT
#define VPTQ_K256C_SPIN_LIMIT 0
#endif
// sweeps per visit of a layer the blocks of row groups are sized for, at least (k256c_host.hip: c_rows_per_wg, c_visit)
#ifndef VPTQ_K256C_MIN_STEPS
#define VPTQ_K256C_MIN_STEPS 8
#endif
constexpr int kCMinSteps = VPTQ_K256C_MIN_STEPS;
constexpr int kCMaxSteps = 4 * kCMinSteps;

// SEL: what k256c_hot_kernel and the host side agree on
constexpr int kHotRows = 64;          // vector-rows per workgroup: 4 rounds of 16 (16 lanes per row, 8 columns per lane and hot block);
                                      // every workgroup repeats the threshold / hot-block search (64 KiB out of the L2): 16 rows per
                                      // workgroup made that search 10 us per launch of 32 layers (rocprofv3, round 6), 64: a quarter
constexpr int kHotMaxBlocks = 256;    // 32768 columns
struct CHotArgs {
  uint32_t corr_off[kMaxGroup];   // byte offset of layer l's corrections from P.sync
  float kappa;
};

// ---- the second geometry, "rows per wave" (gemv_k256r.hip): a workgroup-task = kRTaskGroups consecutive row groups of 8
// vector-rows of one layer, one per wave, walked in steps of kRStepCols columns across the layer's whole width
constexpr int kRTaskGroups = 16;
constexpr int kRStepCols = 128;
// the geometry constants of this build that gemv_k256r.hip restates: a build with others (VPTQ_K256C_WAVES=8, a row split, 4
// subgroups) or with the profile output keeps the first geometry for every launch (k256c_host.hip: r_servable)
constexpr bool kRBuildServes = VPTQ_K256C_PROF == 0 && kCWaves == kRTaskGroups && kCRows == 8 && kCBlockCols == kRStepCols;

// One layer of the launch: 88 bytes of kernel arguments (the K256Layer of the other kernels carries
// fields this one has no use for, and 32 of those + the search table would not fit 4 KiB).
struct CLayerArgs {
  const uint32_t* idx;
  const uint32_t* cent;
  const uint32_t* rcent;
  const uint16_t* x;
  uint16_t* y;
  const uint16_t* scale;
  const uint16_t* wbias;
  const uint16_t* bias;
  int N, G, O, row_words;
  int wgs;   // workgroup that owns block 0 of the layer (rows geometry: task 0)
  int rpw;   // row groups per block (rows geometry: steps of 128 columns per task)
};
constexpr int kCHeadPad = 4;   // the layer search reads 4 headers at a time
struct K256CParams {
  int n_layers;
  int tokens;        // token count | kOutF32Bit
  uint32_t* sync;    // DEP: kCFlagStride arrival flags per layer (zeroed before the launch)
  CLayerArgs layer[kMaxGroup];
  // what the search for a workgroup's next layer needs, 8 bytes per layer:
  // {first workgroup | row groups per block << 16, row groups | sweeps per row group << 24}
  // (rows geometry: {first workgroup | steps per task << 16, tasks})
  uint32_t head[kMaxGroup + kCHeadPad][2];
};
static_assert(sizeof(CLayerArgs) == 88 && offsetof(K256CParams, layer) == 16 &&
              offsetof(K256CParams, head) == 16 + kMaxGroup * 88 && sizeof(K256CParams) <= 4096, "kernarg layout");

typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef const char __attribute__((address_space(4)))* kernarg_ptr_t;

// Layer L of the kernel arguments in one batch of scalar loads.  Everything a wave looks up on its
// way through the stream comes out of the kernel-argument segment through the scalar cache: the
// LDS is the busiest unit of this kernel (a read issued behind 16 waves' gathers comes back late),
// and indexing the by-value argument struct with a run-time index makes the compiler copy it to
// scratch memory.
static __device__ __forceinline__ CLayerArgs c_load_layer(int L) {
  typedef int i16_t __attribute__((ext_vector_type(16)));
  typedef int i4_t __attribute__((ext_vector_type(4)));
  typedef int i2_t __attribute__((ext_vector_type(2)));
  L = __builtin_amdgcn_readfirstlane(L);   // (wave-uniform by construction; the compiler cannot always prove it)
  const kernarg_ptr_t lp = (kernarg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr() + 16 + (size_t)L * sizeof(CLayerArgs);
  i16_t a; i4_t b; i2_t c;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile(
      "s_load_dwordx16 %0, %3, 0x0\n\t"
      "s_load_dwordx4 %1, %3, 0x40\n\t"
      "s_load_dwordx2 %2, %3, 0x50\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(a), "=&s"(b), "=&s"(c)
      : "s"(lp)
      : "memory");
#else
  a = i16_t{}; b = i4_t{}; c = i2_t{}; (void)lp;
#endif
  CLayerArgs Ly;
  __builtin_memcpy((char*)&Ly, &a, 64);
  __builtin_memcpy((char*)&Ly + 64, &b, 16);
  __builtin_memcpy((char*)&Ly + 80, &c, 8);
  Ly.idx = as_global(Ly.idx); Ly.cent = as_global(Ly.cent); Ly.rcent = as_global(Ly.rcent);
  Ly.x = as_global(Ly.x); Ly.y = as_global(Ly.y); Ly.scale = as_global(Ly.scale);
  Ly.wbias = as_global(Ly.wbias); Ly.bias = as_global(Ly.bias);
  return Ly;
}
// the two codebook pointers of layer L
struct CFillL { const uint32_t* cent; const uint32_t* rcent; };
static __device__ __forceinline__ CFillL c_load_fill(int L) {
  typedef int i4_t __attribute__((ext_vector_type(4)));
  L = __builtin_amdgcn_readfirstlane(L);
  const kernarg_ptr_t lp = (kernarg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr() + 16 + (size_t)L * sizeof(CLayerArgs);
  i4_t a;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_load_dwordx4 %0, %1, 0x8\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a) : "s"(lp) : "memory");
#else
  a = i4_t{}; (void)lp;
#endif
  CFillL F;
  __builtin_memcpy((char*)&F, &a, 16);
  F.cent = as_global(F.cent); F.rcent = as_global(F.rcent);
  return F;
}
// search headers of layers L .. L + 3 (the table is padded with kCHeadPad empty layers)
typedef int c_head4_t __attribute__((ext_vector_type(8)));
static __device__ __forceinline__ c_head4_t c_load_heads(int L) {
  L = __builtin_amdgcn_readfirstlane(L);
  const kernarg_ptr_t hp = (kernarg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(K256CParams, head) + (size_t)L * 8;
  c_head4_t h;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(h) : "s"(hp) : "memory");
#else
  h = c_head4_t{}; (void)hp;
#endif
  return h;
}

// the fields of a layer each side of a wave's stream needs (the rest of a CLayerArgs dies right after the load)
struct CIssueL { const uint32_t* idx; const uint16_t* x; const uint16_t* scale; const uint16_t* wbias; int N, G, row_words; };
struct CConsL { uint16_t* y; const uint16_t* bias; int N, G, O; };
static __device__ __forceinline__ CIssueL c_issue_of(const CLayerArgs& L) {
  return CIssueL{L.idx, L.x, L.scale, L.wbias, L.N, L.G, L.row_words};
}
static __device__ __forceinline__ CConsL c_cons_of(const CLayerArgs& L) { return CConsL{L.y, L.bias, L.N, L.G, L.O}; }

// ---- the phases both geometries run, stated once ----

// f(slot 0), f(slot 1), ... f(slot kCDepth - 1) with the slot as a compile-time constant.  (Not common.h's for_slots<kCDepth>: its
// halving recursion leaves the compiler another order of a few scalar instructions in these kernels - profiles/r18/README.md.)
template <typename F>
static __device__ __forceinline__ void c_for_slots(F&& f) {
  f(std::integral_constant<int, 0>{});
  f(std::integral_constant<int, 1>{});
  if constexpr (kCDepth > 2) f(std::integral_constant<int, (kCDepth > 2 ? 2 : 0)>{});
  if constexpr (kCDepth > 3) f(std::integral_constant<int, (kCDepth > 3 ? 3 : 0)>{});
  if constexpr (kCDepth > 4) f(std::integral_constant<int, (kCDepth > 4 ? 4 : 0)>{});
  if constexpr (kCDepth > 5) f(std::integral_constant<int, (kCDepth > 5 ? 5 : 0)>{});
}

// ---- image fill by LDS-DMA: wave w of WAVES brings rows 16 w .. 16 w + 15 (4 instructions of 4 rows; 8 waves: 32 rows, 8;
// lane l = unit l & 15 of row l >> 4: 16 bytes of entry (row) of table (unit >> 3)).  Invisible
// loads can only make the compiler's counted waits stricter, never looser (vmcnt retires in order).
template <int WAVES>
static __device__ __forceinline__ void c_fill_image(const CFillL& F, uint32_t buf, int lane, int wave) {
  const uint32_t unit = (uint32_t)lane & 15u, r4 = (uint32_t)lane >> 4;
  // (table choice by arithmetic: as a per-lane select of two pointers the compiler built a two-entry
  // array in scratch memory and indexed it - a scratch load, waited for with vmcnt(0))
  const uint64_t tc = (uint64_t)(uintptr_t)F.cent, tr = (uint64_t)(uintptr_t)F.rcent;
  const uint64_t pick = (unit >> 3) ? ~0ull : 0ull;
  constexpr uint32_t kRowsW = 256u / (uint32_t)WAVES;   // image rows per wave
  const uint64_t va = tc + ((tr - tc) & pick) + (uint64_t)(((uint32_t)wave * kRowsW + r4) * 16u);
  const uint32_t dst = buf * kCImgBytes + (uint32_t)wave * kRowsW * 256u;
#pragma unroll
  for (int i = 0; i < (int)(kRowsW / 4u); ++i) {
    const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)(dst + (uint32_t)i * 1024u));
    const uint64_t v = va + (uint64_t)(i * 64);
    lds_dma16(d, v);
  }
}

// "everything but the youngest n sweeps' loads has landed", LPS vector loads per sweep.  vmcnt retires in order: at the end
// of the j-th step after a fill the fill is older than j + 1 sweeps; at j = kCLand - 1 those are
// the kCLand youngest of the kCDepth sweeps in flight.
template <int LPS>
static __device__ __forceinline__ void c_wait_all_but(int steps) {
  static_assert(LPS * kCDepth <= 63, "vmcnt is a 6-bit counter");
  switch (steps) {
    case 1: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPS * 1) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPS * 2) : "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPS * 3) : "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPS * 4) : "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPS * 5) : "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPS * 6) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// Hand-over between the waves goes through LDS only, and a wave's LDS operations execute in
// order: fences restricted to the local address space.  An ordinary workgroup-scope release also
// waits for every global load in flight (s_waitcnt vmcnt(0)) - here the whole queue of index
// words requested ahead.
// (the release as a compiler barrier only - the LDS executes one wave's operations in the order they were issued,
// so the counter update cannot overtake the writes - saved nothing: profiles/r03/chain_rowsplit_ldsfence_ab.txt)
// A kernel declares `CLdsRelease lds_release; CLdsAcquire lds_acquire; CLdsInc lds_inc{lds_release, lane};` and its lambdas capture
// them.  (Function objects, not functions: they were lambdas of the kernels, and with plain functions in their place the closures
// of the lambdas that call them lose a member - the listings of both kernels then differ in the order of scalar copies.)
struct CLdsRelease { __device__ void operator()() const { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); } };
struct CLdsAcquire { __device__ void operator()() const { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } };
// count this wave in at *p, everything it wrote to LDS before visible to whoever sees the count
struct CLdsInc {
  CLdsRelease& lds_release;
  const int& lane;
  __device__ __attribute__((always_inline)) void operator()(uint32_t* p) const {
    lds_release();
    if (lane == 0) __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
// poll until *p >= need (bring-up builds: or VPTQ_K256C_SPIN_LIMIT polls have passed); the caller's acquire follows
static __device__ __forceinline__ void c_lds_spin_ge(uint32_t* p, uint32_t need) {
#if VPTQ_K256C_SPIN_LIMIT
  for (int it = 0; it < VPTQ_K256C_SPIN_LIMIT; ++it) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= need) break;
    __builtin_amdgcn_s_sleep(1);
  }
#else
  while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need)
    __builtin_amdgcn_s_sleep(1);
#endif
}

// ---- lane = (column chunk blk = lane >> 2, vector-row j = lane & 3).  The two gathers of an index
// are split across the lanes: in gather A the lanes with bit 3 clear fetch the main entry (unit
// lane & 7 of image row e), the others the residual entry (unit 8 + (lane & 7)); gather B is the
// complement: every 16-lane group of a ds_read_b128 touches 16 different units (gemv_k256m.hip).
// address = {0, base.byte2 = image buffer, index byte, base.byte0}; dword q of the index words holds
// columns 2q (bytes 0 = main, 1 = residual index) and 2q + 1 (bytes 2, 3)
// selA / selB: the x operand of the 4x4x4 MFMA, x' * e_j as two packed pairs, cut out of a packed x' register
// (out-parameters into the kernel's own locals: gathered into one struct, the constants cost both kernels their listings)
static __device__ __forceinline__ void c_lane_constants(int lane, uint32_t& jrow, uint32_t& baseA, uint32_t& baseB, uint32_t (&selGA)[2],
                                                        uint32_t (&selGB)[2], uint32_t (&selA)[2], uint32_t (&selB)[2]) {
  jrow = (uint32_t)lane & 3u;
  const uint32_t hi8 = ((uint32_t)lane >> 3) & 1u;
  baseA = ((hi8 << 3) | ((uint32_t)lane & 7u)) << 4;
  baseB = (((hi8 ^ 1u) << 3) | ((uint32_t)lane & 7u)) << 4;
  selGA[0] = 0x0c020400u | (hi8 << 8); selGA[1] = 0x0c020600u | (hi8 << 8);
  selGB[0] = 0x0c020400u | ((hi8 ^ 1u) << 8); selGB[1] = 0x0c020600u | ((hi8 ^ 1u) << 8);
  selA[0] = jrow == 0 ? 0x0c0c0504u : jrow == 1 ? 0x05040c0cu : 0x0c0c0c0cu;
  selA[1] = jrow == 0 ? 0x0c0c0706u : jrow == 1 ? 0x07060c0cu : 0x0c0c0c0cu;
  selB[0] = jrow == 2 ? 0x0c0c0504u : jrow == 3 ? 0x05040c0cu : 0x0c0c0c0cu;
  selB[1] = jrow == 2 ? 0x0c0c0706u : jrow == 3 ? 0x07060c0cu : 0x0c0c0c0cu;
}

// The two gathers of one index, column u of the 8 a lane holds in its index words iw: 2 perms for the addresses (selectors and
// bases: the lane constants at the head of the kernels), main entry to c, residual entry to r
static __device__ __forceinline__ void c_gather_index(const u32x4& iw, int u, uint32_t baseA, uint32_t baseB, const uint32_t (&selGA)[2],
                                                      const uint32_t (&selGB)[2], u32x4& c, u32x4& r) {
  const uint32_t w = iw[u >> 1];
  const uint32_t aC = __builtin_amdgcn_perm(w, baseA, selGA[u & 1]);
  const uint32_t aR = __builtin_amdgcn_perm(w, baseB, selGB[u & 1]);
  if constexpr ((VPTQ_K256C_ABLATE & 2) != 0) {
    asm volatile("" :: "v"(aC), "v"(aR));
    c = iw; r = iw;
  } else {
    c = lds_load16(aC);
    r = lds_load16(aR);
  }
}

// fp16, the reference's roundings: both row subgroups (main / residual entries c, r and c1, r1) of one column together, stage-major
// over 8 independent chains (dependent packed operations back to back cost wait states); the scale / bias half h of the column's
// pair register is picked by op_sel.  w = r16(r16(r16(c + r) s) + b), then acc += x w by 4 MFMAs.
template <typename DT>
static __device__ __forceinline__ void c_round_pair(u32x4 c, u32x4 r, u32x4 c1, u32x4 r1, uint32_t spair, uint32_t bpair, int h, u32x2 xo,
                                                    f32x4 (&a)[2], f32x4 (&a1)[2]) {
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) { w[k] = DT::add2(c[k], r[k]); w[4 + k] = DT::add2(c1[k], r1[k]); }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = DT::mul2_bcast(w[k], spair, h);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = DT::add2_bcast(w[k], bpair, h);
  a[0] = DT::mfma4(xo, u32x2{w[0], w[1]}, a[0]);
  a[1] = DT::mfma4(xo, u32x2{w[2], w[3]}, a[1]);
  a1[0] = DT::mfma4(xo, u32x2{w[4], w[5]}, a1[0]);
  a1[1] = DT::mfma4(xo, u32x2{w[6], w[7]}, a1[1]);
}

// the kernel arguments of permute_x_kernel (gemv_k256c.hip; filled by launch_permute_x)
struct PermXParams {
  int n;
  int start[kMaxGroup + 1];          // first workgroup of layer l
  const uint16_t* x[kMaxGroup];
  const uint16_t* perm[kMaxGroup];
  uint16_t* out[kMaxGroup];
  int I[kMaxGroup];
};

// ---- the dispatchers of the kernel files: the only way from k256c_host.hip to a kernel; each launches filled arguments
// gemv_k256c_kernel<DT, DEP, MODE> (hipErrorInvalidValue: this build has no such instantiation; dependent: the residency check)
hipError_t k256c_chain(const K256CParams& P, bool f16, bool dependent, int mode, int grid, hipStream_t st);
// k256c_hot_kernel<DT>, in front of a kCModeSel launch: `chunks` workgroups of kHotRows vector-rows per layer
hipError_t k256c_hot(const K256CParams& P, const CHotArgs& H, bool f16, int chunks, hipStream_t st);
// gemv_k256c_rows_kernel (gemv_k256r.hip): fp16, reference roundings, independent layers, 16-bit outputs; P.head /
// CLayerArgs::wgs, rpw in the rows geometry's meaning
hipError_t launch_gemv_k256c_rows(const K256CParams& P, int grid, hipStream_t st);
// permute_x_kernel
hipError_t k256c_permute_x(const PermXParams& P, int blocks, hipStream_t st);

}  // namespace vptq
