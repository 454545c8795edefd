// What the kernels of the persistent chain launch share (gemv_k256c.hip: waves split the columns of a sweep; gemv_k256r.hip: waves
// own their rows across the full width): the kernel-argument block, its scalar loads, and the launcher of the second geometry.
#pragma once
#include <stddef.h>

#include "common.h"
#include "k256.h"

namespace vptq {

constexpr uint32_t kCImgBytes = 65536;               // one codebook image: 256 rows x 16 units x 16 B

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

// ---- the second geometry, "rows per wave" (gemv_k256r.hip): a workgroup-task = kRTaskGroups consecutive row groups of 8
// vector-rows of one layer, one per wave, walked in steps of kRStepCols columns across the layer's whole width
constexpr int kRTaskGroups = 16;
constexpr int kRStepCols = 128;
// fp16, reference roundings, independent layers, 16-bit outputs; P.head / CLayerArgs::wgs, rpw in the rows geometry's meaning
hipError_t launch_gemv_k256c_rows(const K256CParams& P, int grid, hipStream_t st);

}  // namespace vptq
