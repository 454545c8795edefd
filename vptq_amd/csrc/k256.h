// Launch parameters shared by the two k=256 GEMV kernels (gemv_k256.hip: packed-f16 VALU
// accumulate; gemv_k256m.hip: MFMA accumulate).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace vptq {

constexpr int kMaxGroup = 32;
constexpr int kTableBytes = 65536;        // gemv_k256: 256 rows x 256 B
constexpr int kScratchOff = kTableBytes;

struct K256Layer {
  const uint32_t* idx;    // [N, row_words]
  const uint32_t* cent;   // [256, 8] as 4 dwords per entry
  const uint32_t* rcent;  // [256, 8]
  const uint16_t* x;      // [tokens, I]
  uint16_t* y;            // [tokens, O]
  const uint16_t* scale;  // [I]
  const uint16_t* wbias;  // [I]
  const uint16_t* bias;   // [O] or null
  const uint16_t* perm;   // [I] or null
  const char* pf;         // read-ahead range (next layer's indices) or null
  long long pf_bytes;
  int N, G, O, row_words;
  int wgs;       // gemv_k256m: persistent workgroups walking this layer's row groups
  int pf_chunk;  // read-ahead stride per workgroup in bytes (multiple of 128)
  int pf_len;    // bytes actually touched per workgroup (<= pf_chunk)
  int slots;      // gemv_k256m: cross-wave partial-sum slots in LDS (bits 0-7) | bit 8: VPTQ_GEMV_SELECTIVE
};

// K256Params::tokens: token count in the low 16 bits; kOutF32Bit set = y is float32
// [tokens, O] (VPTQ_GEMV_OUT_F32: un-rounded sums, e.g. the partial outputs of a row-parallel
// shard that are rounded once after the all-reduce)
constexpr int kOutF32Bit = 1 << 16;

struct K256Params {
  int n_layers;
  int tokens;
  K256Layer layer[kMaxGroup];
};

// This workgroup's layer (blockIdx.y) and the token count, fetched from the kernel-argument
// segment with ONE batch of scalar loads and one wait (inside the same asm statement, so no
// register is read before it has landed).  Left to the compiler, the fields are loaded where
// they are first used: four dependent kernarg round trips before the first vector load can be
// issued (measured: 1.3-1.7 us median, tools/trace_k256m.py).
static __device__ __forceinline__ K256Layer load_layer_args(int& tokens) {
  static_assert(sizeof(K256Layer) == 120 && offsetof(K256Params, layer) == 8, "kernarg layout");
  typedef int i16_t __attribute__((ext_vector_type(16)));
  typedef int i8_t __attribute__((ext_vector_type(8)));
  typedef int i4_t __attribute__((ext_vector_type(4)));
  typedef int i2_t __attribute__((ext_vector_type(2)));
  const char __attribute__((address_space(4)))* base =
      (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  const char __attribute__((address_space(4)))* lp = base + 8 + (size_t)blockIdx.y * sizeof(K256Layer);
  i16_t a; i8_t b; i4_t c; i2_t d; int tk;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile(
      "s_load_dwordx16 %0, %5, 0x0\n\t"
      "s_load_dwordx8 %1, %5, 0x40\n\t"
      "s_load_dwordx4 %2, %5, 0x60\n\t"
      "s_load_dwordx2 %3, %5, 0x70\n\t"
      "s_load_dword %4, %6, 0x4\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d), "=&s"(tk)
      : "s"(lp), "s"(base)
      : "memory");
#else
  a = i16_t{}; b = i8_t{}; c = i4_t{}; d = i2_t{}; tk = 0; (void)lp;
#endif
  K256Layer L;
  __builtin_memcpy((char*)&L, &a, 64);
  __builtin_memcpy((char*)&L + 64, &b, 32);
  __builtin_memcpy((char*)&L + 96, &c, 16);
  __builtin_memcpy((char*)&L + 112, &d, 8);
  L.idx = as_global(L.idx); L.cent = as_global(L.cent); L.rcent = as_global(L.rcent);
  L.x = as_global(L.x); L.y = as_global(L.y); L.scale = as_global(L.scale);
  L.wbias = as_global(L.wbias); L.bias = as_global(L.bias); L.perm = as_global(L.perm);
  L.pf = as_global(L.pf);
  tokens = tk;
  return L;
}

// -DVPTQ_K256_TRACE (make trace; tools/trace_k256m.py): every wave stamps the 100 MHz wall
// clock at its phase boundaries into the buffer passed as the read-ahead range:
// [workgroup][wave][8] x u64.
#ifdef VPTQ_K256_TRACE
#define K256_STAMP(nwaves, k, dep)                                                              \
  do {                                                                                          \
    unsigned long long t_;                                                                      \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory");  \
    if (lane == 0) ((unsigned long long*)Ly.pf)[((size_t)bid * (nwaves) + wave) * 8 + (k)] = t_; \
  } while (0)
#else
#define K256_STAMP(nwaves, k, dep) do { } while (0)
#endif

// ---- gemv_k256m.hip (the kernel) and k256m_host.hip (its host side): what both read
constexpr int kMRows = 4;  // vector-rows per workgroup of the MFMA kernel
constexpr int kMThreads = 1024;
constexpr int kMWaves = kMThreads / 64;
constexpr int kMSweepCols = kMWaves * 16 * 8;  // 2048: 16 blocks (column chunks of 8) per wave
constexpr int kMTableBytes = 65536;  // 256 rows x (8 main + 8 residual replicas) x 16 B
constexpr int kMMaxLds = 163840;   // 160 KiB per CU
constexpr int kMMaxCols = 14336;   // staged activations must fit beside the image
constexpr int kMXBytes = 2;        // staged bytes per column and token
constexpr int kMRedSlot = kMWaves * 32 * 4;   // one row group's cross-wave partials, per token
constexpr int kMMaxSlots = 4;
// VPTQ_GEMV_SELECTIVE inside the launch (gemv_k256m.hip has the account): the LDS it takes and the launches it covers
constexpr int kMSelBit = 0x100;            // K256Layer::slots: selective roundings
constexpr int kMSelMaxBlocks = 128;        // 16384 columns (staged: <= 14336)
constexpr int kMSelRowGroups = 16;         // row groups per workgroup the corrections cover (16 waves = 4 x 4 rows per round; gate / up of an
                                           // 8B model in one grouped launch: 14 per workgroup)
constexpr int kMSelBytes = 2 * kMSelMaxBlocks + 4 * kMSelRowGroups * 32 * 4;   // block magnitudes + corr [4 quarters of the hot blocks][row groups][32]
// VPTQ_K256M_SB_ALL (A/B, no result on record): every exact instantiation stages scale and bias in LDS (default: bf16, and fp16 from 6 sweeps on)
#ifndef VPTQ_K256M_SB_ALL
#define VPTQ_K256M_SB_ALL 0
#endif
// LDS bytes before the partial-sum slots: image + per token the staged activations (0 columns:
// unstaged) and the per-wave sum b * x + slot counters
// sb: scale and bias planes behind the activations (bf16 exact form)
inline int lds_fixed_bytes(int staged_cols, int tok, bool sb) {
  return kMTableBytes + (staged_cols > 0 ? (tok + (sb ? 2 : 0)) * (staged_cols * kMXBytes + 32) : 0) + tok * kMWaves * 4 + 64 + (tok == 1 && !sb ? kMSelBytes : 0);   // (sb: no selective form, no corrections)
}
// partial-sum slots that fit beside everything else (0: the shape does not fit at all)
inline int lds_slots(int tok, int max_cols, bool sb) {
  const int left = kMMaxLds - lds_fixed_bytes(max_cols > kMMaxCols ? 0 : max_cols, tok, sb);
  const int slots = left < 0 ? 0 : left / (kMRedSlot * tok);
  return slots > kMMaxSlots ? kMMaxSlots : slots;
}
bool gemv_k256m_supported(int tok, bool f16, bool fast, int max_cols, bool perm);
int gemv_k256m_row_groups(int n_rows);
// What one launch of the persistent MFMA kernel is: the template arguments of the instantiation and the launch-shape facts.
// gemv_k256m_decide fills it in (host arithmetic only); launch_gemv_k256m launches exactly that - every launcher checks its own
// template arguments against it - and vptq_quant_gemv*_instance prints it.
struct K256MDecision {
  bool ok;             // the kernel takes the launch at all
  bool f16, fast, perm, selective;
  bool sb;             // scale and bias staged in LDS (kSB in the kernel)
  int tok;             // token slots of the instantiation: 1, 2 or 4
  int ns, nst;         // sweeps of 2048 columns; staging phases (0: the unstaged wide form)
  int max_cols;
  int entry;           // 1: gemv_k256m_kernel_1 (preloaded arguments: one layer, one token), 0: the grouped entry
  int slots;           // cross-wave partial-sum slots in LDS
  int units;           // most row groups any workgroup walks
  int gx;              // grid.x
  int share[kMaxGroup];   // workgroups per layer
};
K256MDecision gemv_k256m_decide(const int* n_rows, int n, int tok, bool f16, bool fast, int max_cols, bool perm, bool selective);
hipError_t launch_gemv_k256m(K256Params& P, const K256MDecision& D, hipStream_t st);
// the instantiation dispatchers of gemv_k256m.hip, one family of instantiations each (its six compile parts): the only way from
// launch_gemv_k256m into the kernel file; each launches the instantiation the decision names
hipError_t k256m_f16_fast(const K256Params& P, const K256MDecision& D, hipStream_t st);            // part 1
hipError_t k256m_f16_exact(const K256Params& P, const K256MDecision& D, hipStream_t st);           // part 2
hipError_t k256m_bf16(const K256Params& P, const K256MDecision& D, hipStream_t st);                // part 2
hipError_t k256m_f16_tokens(const K256Params& P, const K256MDecision& D, hipStream_t st);          // part 3
hipError_t k256m_bf16_tokens(const K256Params& P, const K256MDecision& D, hipStream_t st);         // part 4
hipError_t k256m_bf16_exact(const K256Params& P, const K256MDecision& D, hipStream_t st);          // part 4
hipError_t k256m_f16_tokens_exact(const K256Params& P, const K256MDecision& D, hipStream_t st);    // part 5
hipError_t k256m_bf16_tokens_exact(const K256Params& P, const K256MDecision& D, hipStream_t st);   // part 6
bool gemv_k256m_selective_ok(const int* n_rows, int n, bool f16, int tok, int max_cols, bool perm);
// most row groups any workgroup of one launch of these layers walks (the launch's duration in units of one row group)
int gemv_k256m_launch_units(const int* n_rows, int n);

}  // namespace vptq
