// C ABI of libvptq_hip.so (declared in include/vptq_hip.h): argument validation,
// kernel selection, launch.  No allocation, no synchronisation, no torch.
#include <vector>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "kernels.h"
#include "sliced.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s (hipError %d)", what, hipGetErrorString(e), (int)e);
  return (int)e;
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
int ilog2(int v) { int b = 0; while ((1 << b) < v) ++b; return b; }

// Shape / pointer checks shared by gemv and dequant.  Mirrors what the reference
// asserts with TORCH_CHECK (csrc/quant_gemv.cu:252-282, csrc/dequant.cu:239-275)
// plus the shape algebra of VQuantLinear.__init__ (vptq/layers/vqlinear.py:97-240).
int validate_layer(const VptqLayerDesc* d) {
  if (!d) return fail(VPTQ_E_NULL, "desc is NULL");
  if (!d->indices || !d->centroids) return fail(VPTQ_E_NULL, "indices/centroids is NULL");
  if (d->dtype != VPTQ_DTYPE_F16 && d->dtype != VPTQ_DTYPE_BF16)
    return fail(VPTQ_E_UNSUPPORTED, "dtype %d: only f16 (0) / bf16 (1)", d->dtype);
  const int v = d->vector_len;
  if (!(v == 2 || v == 4 || v == 6 || v == 8 || v == 10 || v == 12 || v == 16))
    return fail(VPTQ_E_UNSUPPORTED, "un-supported vector_len %d", v);
  if (d->in_features <= 0 || d->out_features <= 0 || d->num_codebooks <= 0 || d->group_size <= 0)
    return fail(VPTQ_E_SHAPE, "non-positive dimension");
  if (d->outlier_size < 0 ||
      d->in_features != d->outlier_size + d->num_codebooks * d->group_size)
    return fail(VPTQ_E_SHAPE, "in_features %d != outlier_size %d + %d*%d", d->in_features,
                d->outlier_size, d->num_codebooks, d->group_size);
  if (!pow2(d->num_centroids) || d->num_centroids > 65536)
    return fail(VPTQ_E_SHAPE, "num_centroids %d must be a power of two <= 65536",
                d->num_centroids);
  if (d->index_bits != ilog2(d->num_centroids))
    return fail(VPTQ_E_SHAPE, "index_bits %d != log2(num_centroids)", d->index_bits);
  if (d->num_res_centroids < 0 ||
      (d->num_res_centroids > 0 &&
       (!pow2(d->num_res_centroids) || d->num_res_centroids > 65536)))
    return fail(VPTQ_E_SHAPE, "num_res_centroids %d must be 0 or a power of two <= 65536",
                d->num_res_centroids);
  if (d->res_bits != (d->num_res_centroids > 0 ? ilog2(d->num_res_centroids) : 0))
    return fail(VPTQ_E_SHAPE, "res_bits %d != log2(num_res_centroids)", d->res_bits);
  if ((d->num_res_centroids > 0) != (d->res_centroids != nullptr))
    return fail(VPTQ_E_NULL, "res_centroids must be set iff num_res_centroids > 0");
  const int T = d->index_bits + d->res_bits;
  if (T < 1 || T > 32) return fail(VPTQ_E_SHAPE, "total index bits %d outside [1, 32]", T);
  const long long need_words = ((long long)d->group_size * T + 31) / 32;
  if (d->row_words < need_words)
    return fail(VPTQ_E_SHAPE, "row_words %d < ceil(group_size*bits/32) = %lld", d->row_words,
                need_words);
  if (d->num_indices != (d->out_features + v - 1) / v)
    return fail(VPTQ_E_SHAPE, "num_indices %d != ceil(out_features/vector_len)", d->num_indices);
  // the kernels address the packed indices with 32-bit byte offsets
  if ((unsigned long long)d->num_codebooks * (unsigned long long)d->num_indices * (unsigned long long)d->row_words * 4ull >=
      (1ull << 32))
    return fail(VPTQ_E_SHAPE, "packed indices of %d x %d x %d words: 4 GiB or more are not supported", d->num_codebooks,
                d->num_indices, d->row_words);
  if (d->outlier_size > 0) {
    if (!d->outlier_indices || !d->outlier_centroids)
      return fail(VPTQ_E_NULL, "outlier tensors required when outlier_size > 0");
    if (d->outlier_vector_len < 1 || d->num_outlier_centroids < 1 ||
        d->num_outlier_centroids > 65536)
      return fail(VPTQ_E_SHAPE, "bad outlier codebook shape");
    if (d->num_outlier_indices !=
        (d->out_features + d->outlier_vector_len - 1) / d->outlier_vector_len)
      return fail(VPTQ_E_SHAPE, "num_outlier_indices != ceil(out_features/outlier_vector_len)");
  }
  if ((d->weight_scale != nullptr) != (d->weight_bias != nullptr))
    return fail(VPTQ_E_NULL, "weight_scale and weight_bias must both be set or both NULL");
  if (d->perm && d->in_features > 65536)
    return fail(VPTQ_E_SHAPE, "perm is uint16: in_features must be <= 65536");
  if (((uintptr_t)d->indices | (uintptr_t)d->centroids | (uintptr_t)d->res_centroids) & 3)
    return fail(VPTQ_E_ALIGN, "indices / codebooks must be 4-byte aligned");
  return VPTQ_OK;
}

// VPTQ_GEMV_SELECTIVE where a kernel does not implement it = VPTQ_GEMV_EXACT (always at least as close to the reference);
// EXACT wins when both are set
int selective_as_exact(int flags) {
  return (flags & VPTQ_GEMV_SELECTIVE) ? ((flags & ~VPTQ_GEMV_SELECTIVE) | VPTQ_GEMV_EXACT) : flags;
}
int drop_redundant_selective(int flags) {
  return (flags & VPTQ_GEMV_EXACT) ? (flags & ~VPTQ_GEMV_SELECTIVE) : flags;
}

// Why vptq::sl_check_layouts turned a struct down, as the entries report it: the first reason of `faults` in this order.  The GEMV
// entries answer VPTQ_E_UNSUPPORTED for every one of them (the caller takes another route), repack / fill the code listed.
const struct { unsigned fault; int code; const char* text; } kLayoutFaults[] = {
  {vptq::kSLFaultTensors, VPTQ_E_NULL, "elems / blocks / first (building: wstart too) is NULL"},
  {vptq::kSLFaultSlices, VPTQ_E_SHAPE, "n_slices is not this layer's"},
  {vptq::kSLFaultWhole, VPTQ_E_UNSUPPORTED, "whole_table is not this table's"},
  {vptq::kSLFaultRes, VPTQ_E_NULL, "the `res` side stream must be set where the layouts carry one (building / repacking: and only there), uint16 at an even address"},
  {vptq::kSLFaultRows, VPTQ_E_UNSUPPORTED, "rows_per_wave in [1, 64], the same in every struct of the call"},
  {vptq::kSLFaultAlign, VPTQ_E_ALIGN, "elems 16-byte, blocks / first / wstart / res 4-byte (repacking a uint16 res: 8-byte) aligned"},
};
int layout_fail(unsigned faults, bool gemv, const char* who, int layer, int which, const vptq::SlicedLayoutSet& S,
                const char* whose = "vptq_sliced_layout_set") {
  for (const auto& f : kLayoutFaults)
    if (faults & f.fault)
      return fail(gemv ? VPTQ_E_UNSUPPORTED : f.code, "%s: layer / part %d, layout %d: %s (%s: n_slices %d, whole_table %d / %d, "
                  "side stream of %d byte(s))", who, layer, which, f.text, whose, S.slices, S.whole[0], S.whole[1], S.side_bytes);
  return VPTQ_OK;
}
const char* const kNoExactLayout = "no exact sliced layout serves this layer (vptq_sliced_layout_set(desc, VPTQ_GEMV_EXACT): in one piece, or as 2 / 3 column parts)";
const char* const kPartsShare = "column parts go with VPTQ_GEMV_EXACT, share y, the workspace, the output bias and have one width (tokens: and take them in one pass)";

}  // namespace

extern "C" {

int vptq_abi_version(void) { return VPTQ_ABI_VERSION; }

const char* vptq_last_error(void) { return g_err; }

int vptq_quant_gemv_max_tokens(const VptqLayerDesc* d) {
  if (validate_layer(d) != VPTQ_OK) return 0;
  if (vptq::gemm_k256_eligible(*d, 16, 0)) return 48;
  // bf16: 15.6 us per launch of 16 tokens (gemm_k256t) against ~55 us for dequant + GEMM at 8192^2
  if (vptq::gemm_k256t_eligible(*d, 16, 0)) return 48;
  return vptq::gemv_k256_eligible(*d, 4) ? VPTQ_GEMV_MAX_TOKENS_ANY : 8;
}

// ---- which kernel family serves (layer, tokens, flags): ONE decision for vptq_quant_gemv and for
// vptq_quant_gemv_kernel_name (x = NULL there: the activation pointer is assumed aligned) ----
enum Route { kRouteNone, kRouteGemmK256T, kRouteGemmK256, kRouteK256, kRouteGather, kRouteLds, kRouteGatherX, kRouteGeneric };

static int batch_min_tokens() {
  // smallest token count that takes the batched-decode kernel (at most 16: vptq_quant_gemv_max_tokens promises the batched
  // kernel for 17+ tokens of such layers)
  static const int w = vptq::tune_int("VPTQ_GEMM_MIN_TOKENS", 5);
  return w > 16 ? 16 : (w < 1 ? 1 : w);
}

// Smallest token count that takes the one-pass batched-decode kernel (gemm_k256t.hip).  Measured at 8192^2 / 4096^2
// (profiles/r03/tokens_*): 13.5 / 9.3 us at 5 tokens ... 15.6 / 10.3 us at 16 for either dtype (its pre-pass is 4.8 us
// of that) against 9.0-10.3 / 5.2-6.6 us for 2-4 tokens on the GEMV kernels, 17.8-18.5 / 10.4-10.8 us for 5-16 fp16
// tokens on gemm_k256 and 18-39 us for bf16 as launches of <= 4 tokens: the default route from 5 tokens for both
// dtypes.  VPTQ_GEMMT_MIN_TOKENS_F16 / _BF16 override (tuning), VPTQ_GEMV_FORCE_BATCHED forces.
static int batch_t_min_tokens(int dtype) {
  static const int wf = vptq::tune_int("VPTQ_GEMMT_MIN_TOKENS_F16", 5), wb = vptq::tune_int("VPTQ_GEMMT_MIN_TOKENS_BF16", 5);
  const int w = dtype == VPTQ_DTYPE_F16 ? wf : wb;
  return w < 1 ? 1 : w;
}

// gemv_lds.hip: every token of one call in the same arithmetic - the one-token MFMA form only for one-token calls
static int lds_launch_flags(int tokens, int flags) { return tokens > 1 ? (flags | VPTQ_GEMV_EXACT) : flags; }

// have_ws: the caller's workspace holds vptq_quant_gemv_workspace_bytes (kernel-name queries: assumed)
static Route route_gemv(const VptqLayerDesc& d, int tokens, int flags, const void* x, bool have_ws) {
  const uintptr_t xa = (uintptr_t)x;   // 0 when unknown
  const bool forced_generic = (flags & VPTQ_GEMV_FORCE_GENERIC) != 0;
  // canonical format, folded arithmetic: up to 16 tokens in ONE pass over the indices (launches of 16)
  if (have_ws && !(flags & (VPTQ_GEMV_FORCE_GENERIC | VPTQ_GEMV_FORCE_VALU | VPTQ_GEMV_FORCE_MFMA)) &&
      ((flags & VPTQ_GEMV_FORCE_BATCHED) || tokens >= batch_t_min_tokens(d.dtype)) &&
      vptq::gemm_k256t_eligible(d, tokens > 16 ? 16 : tokens, flags) && (xa & 1) == 0)
    return kRouteGemmK256T;
  // canonical format, fp16, 5-16 tokens: ONE launch of the batched-decode kernel per 16 tokens
  if (!(flags & (VPTQ_GEMV_FORCE_GENERIC | VPTQ_GEMV_FORCE_VALU | VPTQ_GEMV_FORCE_MFMA)) &&
      tokens >= batch_min_tokens() && vptq::gemm_k256_eligible(d, tokens > 16 ? 16 : tokens, flags) && (xa & 15) == 0)
    return kRouteGemmK256;
  if (tokens > VPTQ_GEMV_MAX_TOKENS_ANY) return kRouteNone;
  const int chunk4 = tokens > 4 ? 4 : tokens;
  if (!forced_generic && vptq::gemv_k256_eligible(d, chunk4) && (xa & 15) == 0 &&
      (tokens <= 4 || (d.in_features % 8) == 0))
    return kRouteK256;
  if (!forced_generic && vptq::gemv_gather_eligible(d, tokens > 8 ? 8 : tokens) && (xa & 3) == 0) return kRouteGather;
  if (!forced_generic && vptq::gemv_lds_eligible(d, chunk4, flags) && (xa & 15) == 0) return kRouteLds;
  if (!forced_generic && vptq::gemv_gatherx_eligible(d, chunk4) && (xa & 3) == 0) return kRouteGatherX;   // (4 fits every launch size)
  return kRouteGeneric;
}

size_t vptq_quant_gemv_workspace_bytes(const VptqLayerDesc* d, int tokens, int flags) {
  if (validate_layer(d) != VPTQ_OK || tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS) return 0;
  flags = selective_as_exact(flags);
  return route_gemv(*d, tokens, flags, nullptr, true) == kRouteGemmK256T ? vptq::gemm_k256t_workspace_bytes(*d) : 0;
}

const char* vptq_quant_gemv_kernel_name(const VptqLayerDesc* d, int tokens, int flags) {
  if (validate_layer(d) != VPTQ_OK || tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS) return nullptr;
  const int kflags = drop_redundant_selective(flags);
  flags = selective_as_exact(flags);
  switch (route_gemv(*d, tokens, flags, nullptr, true)) {
    case kRouteGemmK256T: return "gemm_k256t_kernel";
    case kRouteGemmK256: return "gemm_k256_kernel";
    case kRouteK256: return vptq::gemv_k256_name(*d, tokens, tokens == 1 ? kflags : flags);
    case kRouteGather: return "gemv_gather_kernel";
    case kRouteLds: return vptq::gemv_lds_name(*d, tokens, flags);
    case kRouteGatherX: return "gemv_gatherx_kernel";
    case kRouteGeneric: return "gemv_generic_kernel";
    default: return nullptr;
  }
}

const char* vptq_quant_gemv_grouped_kernel_name(const VptqLayerDesc* descs, int n, int tokens,
                                                int flags) {
  if (!descs || n < 1 || n > VPTQ_GROUP_MAX || tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS_ANY) return nullptr;
  bool one_launch = !(flags & VPTQ_GEMV_FORCE_GENERIC);
  for (int i = 0; i < n; ++i) {
    if (validate_layer(&descs[i]) != VPTQ_OK) return nullptr;
    one_launch = one_launch && descs[i].dtype == descs[0].dtype &&
                 vptq::gemv_k256_eligible(descs[i], tokens) &&
                 ((descs[i].perm != nullptr) == (descs[0].perm != nullptr));
  }
  return one_launch ? vptq::gemv_k256_group_name(descs, n, tokens, flags) : "per-layer";
}

int vptq_quant_gemv(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags,
                    void* workspace, size_t workspace_bytes, void* stream) {
  int rc = validate_layer(d);
  if (rc) return rc;
  // SELECTIVE: the canonical format's kernels decide (gemv_k256.hip:choose_kernel - the persistent MFMA kernel at one token, else
  // the reference's roundings); every other route takes the reference's roundings
  const int kflags = drop_redundant_selective(flags);
  flags = selective_as_exact(flags);
  if (!x || !y) return fail(VPTQ_E_NULL, "x / y is NULL");
  // (a workspace is never required: without it the call takes the kernels that need none)
  const bool have_ws = workspace && (((uintptr_t)workspace) & 15) == 0 &&
                       workspace_bytes >= vptq::gemm_k256t_workspace_bytes(*d);
  if (tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d]: use vptq_dequant + GEMM", tokens,
                VPTQ_GEMV_MAX_TOKENS);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  const bool out_f32 = (flags & VPTQ_GEMV_OUT_F32) != 0;
  const size_t yes = out_f32 ? 4 : 2;  // bytes per output element
  const size_t xrow = (size_t)d->in_features * 2, yrow = (size_t)d->out_features * yes;
  // tokens are served in launches of `step` tokens (more tokens = more launches; up to 16 tokens still
  // cheaper than a dense dequant + GEMM for the canonical format, tools/tokens_crossover.py)
  auto chunks = [&](int step, const char* what, auto&& launch) -> int {
    for (int t0 = 0; t0 < tokens; t0 += step) {
      const int m = tokens - t0 < step ? tokens - t0 : step;
      e = launch((const char*)x + (size_t)t0 * xrow, (char*)y + (size_t)t0 * yrow, m);
      if (e != hipSuccess) return hip_fail(e, what);
    }
    return VPTQ_OK;
  };
  switch (route_gemv(*d, tokens, flags, x, have_ws)) {
    case kRouteGemmK256T:  // tokens = the M dimension of a 16x16x32 MFMA fed by transposing gathers; folded arithmetic.
      // (launches of one call share the workspace: they are ordered on the stream)
      return chunks(16, "gemm_k256t launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemm_k256t(*d, xc, yc, m, out_f32, workspace, st); });
    case kRouteGemmK256:   // tokens = the M dimension of a 16x16x16 MFMA; reference arithmetic
      return chunks(16, "gemm_k256 launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemm_k256(*d, xc, yc, m, out_f32, st); });
    case kRouteK256:
      return chunks(4, "gemv_k256 launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemv_k256(d, 1, &xc, &yc, m, tokens == 1 ? kflags : flags, st); });
    case kRouteGather:     // up to 8 tokens per pass over the indices
      return chunks(8, "gemv_gather launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemv_gather(*d, xc, yc, m, out_f32, st); });
    case kRouteLds: {
      const int lflags = lds_launch_flags(tokens, flags);
      return chunks(vptq::gemv_lds_max_chunk(d->dtype), "gemv_lds launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemv_lds(*d, xc, yc, m, out_f32, lflags, st); });
    }
    case kRouteGatherX:    // 8 token slots for v <= 8, else 4
      return chunks(vptq::gemv_gatherx_max_chunk(*d), "gemv_gatherx launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemv_gatherx(*d, xc, yc, m, out_f32, st); });
    case kRouteGeneric:    // the generic kernel takes up to 8 tokens per launch
      return chunks(8, "gemv_generic launch", [&](const void* xc, void* yc, int m) {
        return vptq::launch_gemv_generic(*d, xc, yc, m, out_f32, st); });
    default:
      return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d] for this layer: use vptq_dequant + GEMM", tokens,
                  VPTQ_GEMV_MAX_TOKENS_ANY);
  }
}

// How a grouped call is executed: ONE decision for vptq_quant_gemv_grouped and vptq_quant_gemv_grouped_instance (x = NULL
// there: the activation pointers are assumed aligned).  flags: as the call has normalised them.
enum GroupRoute { kGroupEachK256, kGroupLaunches, kGroupPerLayer };
static GroupRoute group_route(const VptqLayerDesc* descs, int n, const void* const* x, int tokens, int flags) {
  bool all_fast = !(flags & VPTQ_GEMV_FORCE_GENERIC);
  bool same_perm = true;  // one instantiation serves the whole group
  for (int i = 0; i < n; ++i) {
    all_fast = all_fast && vptq::gemv_k256_eligible(descs[i], tokens) && (!x || (((uintptr_t)x[i]) & 15) == 0);
    same_perm = same_perm && ((descs[i].perm != nullptr) == (descs[0].perm != nullptr));
  }
  if (all_fast && !same_perm) return kGroupEachK256;   // one launch of the canonical format's kernels per layer
  return all_fast ? kGroupLaunches : kGroupPerLayer;   // one launch for up to 32 layers / vptq_quant_gemv per layer
}
static int group_flags(int tokens, int flags) {
  return tokens == 1 ? drop_redundant_selective(flags) : selective_as_exact(flags);   // (one token: gemv_k256.hip:choose_kernel decides)
}

int vptq_quant_gemv_grouped(const VptqLayerDesc* descs, int n, const void* const* x,
                            void* const* y, int tokens, int flags, void* stream) {
  if (!descs || !x || !y) return fail(VPTQ_E_NULL, "descs / x / y is NULL");
  if (n < 1 || n > VPTQ_GROUP_MAX) return fail(VPTQ_E_SHAPE, "n %d outside [1, %d]", n, VPTQ_GROUP_MAX);
  if (tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS_ANY)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d]", tokens, VPTQ_GEMV_MAX_TOKENS_ANY);
  flags = group_flags(tokens, flags);
  for (int i = 0; i < n; ++i) {
    int rc = validate_layer(&descs[i]);
    if (rc) return rc;
    if (!x[i] || !y[i]) return fail(VPTQ_E_NULL, "x[%d] / y[%d] is NULL", i, i);
    if (descs[i].dtype != descs[0].dtype)
      return fail(VPTQ_E_UNSUPPORTED, "grouped layers must share one dtype");
  }
  hipStream_t st = (hipStream_t)stream;
  switch (group_route(descs, n, x, tokens, flags)) {
    case kGroupEachK256:
      for (int i = 0; i < n; ++i) {
        hipError_t e = vptq::launch_gemv_k256(descs + i, 1, x + i, y + i, tokens, flags, st);
        if (e != hipSuccess) return hip_fail(e, "gemv_k256 launch");
      }
      return VPTQ_OK;
    case kGroupLaunches:
      // one launch for up to 32 layers
      for (int i0 = 0; i0 < n; i0 += 32) {
        const int m = n - i0 < 32 ? n - i0 : 32;
        hipError_t e = vptq::launch_gemv_k256(descs + i0, m, x + i0, y + i0, tokens, flags, st);
        if (e != hipSuccess) return hip_fail(e, "gemv_k256 grouped launch");
      }
      return VPTQ_OK;
    default:
      break;
  }
  for (int i = 0; i < n; ++i) {
    const int rc = vptq_quant_gemv(&descs[i], x[i], y[i], tokens, flags, nullptr, 0, stream);
    if (rc) return rc;
  }
  return VPTQ_OK;
}

// ---- which instantiation a call would launch, as text (vptq_quant_gemv*_instance): the decisions above and the kernels' own
// decide functions (gemv_k256.hip:k256_decide, gemv_k256m_decide, gemm_k256_decide, gemm_k256t_decide, gemv_k256c_mode), printed
namespace {
using vptq::Text;
using vptq::dt_text;
int instance_done(const Text& t) { return text_done(t) == 0 ? VPTQ_OK : fail(VPTQ_E_WORKSPACE, "instance: buffer of %zu bytes too small", t.bytes); }

// launches of the canonical format's one-layer kernels for (descs, n, tokens): appended to t
int add_k256(Text& t, const VptqLayerDesc* descs, int n, int tokens, int flags) {
  char one[1024];
  const int rc = vptq::gemv_k256_instance(descs, n, tokens, flags, one, sizeof(one));
  if (rc == -2) { t.fits = false; return VPTQ_OK; }
  if (rc) return fail(VPTQ_E_UNSUPPORTED, "instance: no gemv_k256 / gemv_k256m instantiation for this launch");
  t.add("%s", one);
  return VPTQ_OK;
}

// a launch of gemv_lds.hip (packed or v2 layers)
void add_lds(Text& t, const vptq::LdsDecision& D) {
  if (!D.ok) { t.add("none"); return; }
  if (D.mfma)
    t.add("gemv_lds_mfma dt=%s fmt=%s rw=%d stages=%d dma=%d perm=%d", dt_text(D.f16), vptq::gemv_lds_fmt_text(D.fmt), D.rw, D.stages,
          (int)D.dma, (int)D.perm);
  else
    t.add("gemv_lds dt=%s fmt=%s tok=%d rw=%d dma=%d perm=%d", dt_text(D.f16), vptq::gemv_lds_fmt_text(D.fmt), D.tok, D.rw, (int)D.dma,
          (int)D.perm);
}

// what vptq_quant_gemv(d, tokens, flags) launches (the first launch of a call that is served in several)
int add_one(Text& t, const VptqLayerDesc& d, int tokens, int flags) {
  const int kflags = drop_redundant_selective(flags);
  flags = selective_as_exact(flags);
  const Route r = route_gemv(d, tokens, flags, nullptr, true);
  const char* const dt = dt_text(d.dtype == VPTQ_DTYPE_F16);
  switch (r) {
    case kRouteGemmK256T: {
      const vptq::GemmK256TDecision D = vptq::gemm_k256t_decide(d);
      t.add("gemm_k256t dt=%s perm=%d tok=%d sweeps=%d rgs=%d", dt, (int)D.perm, tokens > 16 ? 16 : tokens, D.n_sweeps,
            D.groups_per_wg);
      return VPTQ_OK;
    }
    case kRouteGemmK256: {
      const vptq::GemmK256Decision D = vptq::gemm_k256_decide(d);
      t.add("gemm_k256 dt=%s perm=%d tok=%d passes=", dt, (int)D.perm, tokens > 16 ? 16 : tokens);
      bool first = true;
      for (int nrg = 4; nrg >= 1; nrg >>= 1)
        if (D.passes & nrg) { t.add("%s%d", first ? "" : "+", nrg); first = false; }
      return VPTQ_OK;
    }
    case kRouteK256: {
      const VptqLayerDesc* dp = &d;
      return add_k256(t, dp, 1, tokens > 4 ? 4 : tokens, tokens == 1 ? kflags : flags);
    }
    case kRouteNone:
      return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d] for this layer", tokens, VPTQ_GEMV_MAX_TOKENS_ANY);
    // the other families: the first launch of the call, as vptq_quant_gemv's own switch chunks it
    case kRouteGather: {
      const vptq::GatherDecision D = vptq::gemv_gather_decide(d, tokens > 8 ? 8 : tokens);
      t.add("gemv_gather dt=%s t=%d rows=%d tok=%d perm=%d wide=%d", dt, D.T, D.rows, D.tok, (int)D.perm, (int)D.wide);
      return VPTQ_OK;
    }
    case kRouteLds: {
      const int step = vptq::gemv_lds_max_chunk(d.dtype);
      add_lds(t, vptq::gemv_lds_decide(d, tokens > step ? step : tokens, lds_launch_flags(tokens, flags)));
      return VPTQ_OK;
    }
    case kRouteGatherX: {
      const int step = vptq::gemv_gatherx_max_chunk(d);
      const vptq::GatherXDecision D = vptq::gemv_gatherx_decide(d, tokens > step ? step : tokens);
      t.add("gemv_gatherx dt=%s v=%d tok=%d perm=%d reslds=%d outl=", dt, D.v, D.tok, (int)D.perm, (int)D.res_lds);
      if (D.ov == 0) t.add("0");
      else if (D.ov == D.v) t.add("same");
      else t.add("%d", D.ov);
      t.add(" groups=%d", D.groups);
      return VPTQ_OK;
    }
    case kRouteGeneric: {
      const vptq::GenericDecision D = vptq::gemv_generic_decide(d, tokens > 8 ? 8 : tokens);
      t.add("gemv_generic dt=%s v=%d tok=%d", dt, D.v, D.tok);
      return VPTQ_OK;
    }
  }
  return fail(VPTQ_E_UNSUPPORTED, "instance: no route");
}
}  // namespace

int vptq_quant_gemv_instance(const VptqLayerDesc* d, int tokens, int flags, char* buf, size_t bytes) {
  if (!d || !buf || bytes < 1) return fail(VPTQ_E_NULL, "desc / buf is NULL");
  buf[0] = 0;
  int rc = validate_layer(d);
  if (rc) return rc;
  if (tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS) return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d]", tokens, VPTQ_GEMV_MAX_TOKENS);
  Text t = {buf, bytes, 0, true};
  rc = add_one(t, *d, tokens, flags);
  return rc ? rc : instance_done(t);
}

int vptq_quant_gemv_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes) {
  if (!descs || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / buf is NULL");
  buf[0] = 0;
  if (n < 1 || n > VPTQ_GROUP_MAX) return fail(VPTQ_E_SHAPE, "n %d outside [1, %d]", n, VPTQ_GROUP_MAX);
  if (tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS_ANY)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d]", tokens, VPTQ_GEMV_MAX_TOKENS_ANY);
  flags = group_flags(tokens, flags);
  for (int i = 0; i < n; ++i) {
    const int rc = validate_layer(&descs[i]);
    if (rc) return rc;
    if (descs[i].dtype != descs[0].dtype) return fail(VPTQ_E_UNSUPPORTED, "grouped layers must share one dtype");
  }
  Text t = {buf, bytes, 0, true};
  const GroupRoute route = group_route(descs, n, nullptr, tokens, flags);
  const int step = route == kGroupLaunches ? 32 : 1;
  for (int i0 = 0; i0 < n; i0 += step) {
    if (i0) t.add(" | ");
    const int m = n - i0 < step ? n - i0 : step;
    const int rc = route == kGroupPerLayer ? add_one(t, descs[i0], tokens, flags) : add_k256(t, descs + i0, m, tokens, flags);
    if (rc) return rc;
  }
  return instance_done(t);
}

// ---- chain: one persistent launch per <= 32 layers (gemv_k256c.hip), else layer by layer ----
// can the persistent launch serve these layers with these flags (whether it is the faster route aside)?
static bool chain_kernel_takes(const VptqLayerDesc* descs, int n, const void* const* x, int tokens, int flags) {
  if (tokens != 1 || (flags & (VPTQ_GEMV_FORCE_GENERIC | VPTQ_GEMV_FORCE_VALU))) return false;
  const bool exact = (flags & VPTQ_GEMV_EXACT) != 0, dep = (flags & VPTQ_GEMV_CHAIN_DEPENDENT) != 0;
  const bool sel = !exact && (flags & VPTQ_GEMV_SELECTIVE) != 0;
  for (int i = 0; i < n; ++i) {
    if (descs[i].dtype != descs[0].dtype || !vptq::gemv_k256c_eligible(descs[i], tokens)) return false;
    if (exact && !vptq::gemv_k256c_exact_ok(descs[i], dep)) return false;   // (bf16 / dependent: layer by layer)
    if (sel && !vptq::gemv_k256c_selective_ok(descs[i], dep)) return false;
    if (x && (((uintptr_t)x[i]) & 3) != 0) return false;
  }
  return true;
}
static bool chain_one_kernel(const VptqLayerDesc* descs, int n, const void* const* x, int tokens, int flags) {
  if (!chain_kernel_takes(descs, n, x, tokens, flags)) return false;
  // a chain that cannot keep the workgroups busy (one small layer, q / k / v of a small model) is better
  // served by the per-layer kernels; VPTQ_GEMV_FORCE_MFMA takes the chain kernel regardless (tests)
  if (!(flags & VPTQ_GEMV_FORCE_MFMA)) {
    const bool dependent = (flags & VPTQ_GEMV_CHAIN_DEPENDENT) != 0;
    for (int i0 = 0; i0 < n; i0 += 32)
      if (!vptq::gemv_k256c_fills_device(descs + i0, n - i0 < 32 ? n - i0 : 32, dependent)) return false;
  }
  return true;
}

// SELECTIVE (independent lists): per launch of <= 32 layers a header + one float per output (gemv_k256c.hip), in front of
// everything else
static size_t chain_sel_bytes(const VptqLayerDesc* descs, int n, int flags) {
  flags = drop_redundant_selective(flags);
  if (!(flags & VPTQ_GEMV_SELECTIVE) || (flags & VPTQ_GEMV_CHAIN_DEPENDENT) || !descs || n < 1) return 0;
  size_t b = 0;
  for (int i0 = 0; i0 < n; i0 += 32) b += vptq::gemv_k256c_selective_bytes(descs + i0, n - i0 < 32 ? n - i0 : 32);
  return b;
}
size_t vptq_quant_gemv_chain_workspace_bytes(int n, int flags) {
  return (flags & VPTQ_GEMV_CHAIN_DEPENDENT) && n > 0 ? (size_t)n * 1024 : 0;   // 256 arrival flags per layer
}
// ... and, for an INDEPENDENT list, room for x[perm] of every layer that has an input permutation (optional: without it
// such a list is served by grouped / single launches, which take permutations themselves)
size_t vptq_quant_gemv_chain_workspace_bytes_for(const VptqLayerDesc* descs, int n, int flags) {
  size_t b = vptq_quant_gemv_chain_workspace_bytes(n, flags);
  if (!descs || n < 1 || (flags & VPTQ_GEMV_CHAIN_DEPENDENT)) return b;
  b += chain_sel_bytes(descs, n, flags);
  for (int i = 0; i < n; ++i) b += vptq::gemv_k256c_perm_bytes(descs[i]);
  return b;
}

// How a chain call is executed.  The persistent launch pays its prologue (first codebook image, queue fill: ~7 us)
// once per call and wins from ~16 independent layers on; up to 8 it loses to ONE grouped launch of the one-layer
// kernels (layer = blockIdx.y; 8192^2, us per layer at 2 / 4 / 8 layers: 7.72 / 6.06 / 5.31 against 5.86 / 5.45 / 5.01,
// profiles/r03/chain_vs_grouped_by_length.txt), and a list that cannot fill the device with the persistent kernel
// (q / k / v of a small model) is still better served by one grouped launch than by one launch per layer.
enum ChainRoute { kChainPersistent, kChainGrouped, kChainPerLayer };
constexpr int kChainGroupedMax = 8;
static ChainRoute chain_route(const VptqLayerDesc* descs, int n, const void* const* x, int tokens, int flags) {
  const bool dependent = (flags & VPTQ_GEMV_CHAIN_DEPENDENT) != 0;
  const bool persistent_ok = chain_one_kernel(descs, n, x, tokens, flags);
  if (n == 1 && !(flags & VPTQ_GEMV_FORCE_MFMA)) return kChainPerLayer;   // (the one-layer kernels: arguments preloaded, short prologue)
  if (persistent_ok && (dependent || n > kChainGroupedMax || (flags & VPTQ_GEMV_FORCE_MFMA))) return kChainPersistent;
  if (!dependent && n >= 2 && n <= VPTQ_GROUP_MAX && tokens <= VPTQ_GEMV_MAX_TOKENS_ANY &&
      (n <= kChainGroupedMax || !persistent_ok)) {
    for (int i = 1; i < n; ++i)
      if (descs[i].dtype != descs[0].dtype) return kChainPerLayer;
    return kChainGrouped;
  }
  return persistent_ok ? kChainPersistent : kChainPerLayer;
}

// Layers with an input permutation in an independent one-token list: the persistent launch runs on (x[perm], scale_permuted,
// bias_permuted) without a permutation.  dd = the descriptors it is given; 0: no layer has one, 1: all of them can, -1: not all
static int chain_absorb_perms(const VptqLayerDesc* descs, int n, std::vector<VptqLayerDesc>& dd) {
  dd.assign(descs, descs + n);
  bool any = false, ok = true;
  for (int i = 0; i < n; ++i) {
    if (!dd[i].perm) continue;
    any = true;
    ok = ok && dd[i].scale_permuted && dd[i].bias_permuted && (dd[i].in_features % 8) == 0 && (((uintptr_t)dd[i].perm) & 15) == 0;
    dd[i].weight_scale = dd[i].scale_permuted;
    dd[i].weight_bias = dd[i].bias_permuted;
    dd[i].perm = nullptr; dd[i].inv_perm = nullptr; dd[i].scale_permuted = nullptr; dd[i].bias_permuted = nullptr;
  }
  return !any ? 0 : ok ? 1 : -1;
}

// How a chain call is executed: ONE decision for vptq_quant_gemv_chain and vptq_quant_gemv_chain_instance.  The call hands over
// its activation pointers and workspace; the query passes x = NULL and assume_ws (the workspace ..._workspace_bytes_for asks
// for, aligned, as vptq_quant_gemv_chain_kernel_name assumes).
struct ChainDecision {
  int flags;            // normalised: SELECTIVE dropped beside EXACT, and turned into EXACT where the call cannot carry its thresholds
  bool dependent;
  size_t sel_bytes;     // > 0: the selective thresholds take the first sel_bytes of the workspace
  ChainRoute route;
  bool absorbed;        // persistent launch with the permuted layers on (x[perm], scale_permuted, bias_permuted): x[perm] is
                        // gathered into the workspace (behind the thresholds) by one small launch in front
  std::vector<VptqLayerDesc> run;   // absorbed: the descriptors the persistent launch is given
  std::vector<const void*> xx;      // absorbed, x given: its activation pointers ...
  std::vector<void*> xp;            // ... and where x[perm] of each permuted layer goes (NULL: no permutation)
};
static ChainDecision chain_decide(const VptqLayerDesc* descs, int n, const void* const* x, int tokens, int flags, bool assume_ws,
                                  void* workspace, size_t workspace_bytes) {
  ChainDecision D = {};
  D.dependent = (flags & VPTQ_GEMV_CHAIN_DEPENDENT) != 0;
  flags = drop_redundant_selective(flags);
  char* ws = (char*)workspace;
  auto ws_holds = [&](size_t need) { return assume_ws || (ws && workspace_bytes >= need && (((uintptr_t)ws) & 255) == 0); };
  // SELECTIVE: the thresholds live in front of the workspace; without it (or for a dependent list) the call takes the
  // reference's roundings everywhere
  if (flags & VPTQ_GEMV_SELECTIVE) {
    const size_t tb = chain_sel_bytes(descs, n, flags);
    if (tb > 0 && ws_holds(tb)) {
      D.sel_bytes = tb;
      if (ws) { ws += tb; workspace_bytes -= tb; }
    } else {
      flags = selective_as_exact(flags);
    }
  }
  D.flags = flags;
  // Layers with an input permutation in an independent list: with enough workspace for x[perm] the list still runs in the
  // persistent launch
  if (!D.dependent && tokens == 1) {
    size_t need = 0;
    for (int i = 0; i < n; ++i) need += vptq::gemv_k256c_perm_bytes(descs[i]);
    if (need > 0 && ws_holds(need) && chain_absorb_perms(descs, n, D.run) == 1) {
      if (x) {
        D.xx.assign(x, x + n);
        D.xp.assign(n, nullptr);
        char* w = ws;
        for (int i = 0; i < n; ++i) {
          if (!descs[i].perm) continue;
          D.xp[i] = w;
          D.xx[i] = w;
          w += vptq::gemv_k256c_perm_bytes(descs[i]);
        }
      }
      if (chain_route(D.run.data(), n, x ? D.xx.data() : nullptr, tokens, flags) == kChainPersistent) {
        D.absorbed = true;
        D.route = kChainPersistent;
        return D;
      }
    }
  }
  D.run.clear();
  D.route = chain_route(descs, n, x, tokens, flags);
  return D;
}

const char* vptq_quant_gemv_chain_kernel_name(const VptqLayerDesc* descs, int n, int tokens, int flags) {
  if (!descs || n < 1 || n > VPTQ_CHAIN_MAX || tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS) return nullptr;
  for (int i = 0; i < n; ++i)
    if (validate_layer(&descs[i]) != VPTQ_OK) return nullptr;
  if (!(flags & VPTQ_GEMV_CHAIN_DEPENDENT) && tokens == 1) {
    // (as vptq_quant_gemv_kernel_name: assuming the caller hands over the workspace ..._workspace_bytes_for asks for -
    // layers with an input permutation then stay in the persistent launch)
    std::vector<VptqLayerDesc> dd;
    if (chain_absorb_perms(descs, n, dd) == 1 && chain_route(dd.data(), n, nullptr, tokens, flags) == kChainPersistent)
      return "gemv_k256c_kernel";
  }
  switch (chain_route(descs, n, nullptr, tokens, flags)) {
    case kChainPersistent: return "gemv_k256c_kernel";
    case kChainGrouped: return "grouped";
    default: return "per-layer";
  }
}

int vptq_quant_gemv_chain_plan(const VptqLayerDesc* descs, int n, int flags, int workgroups, int* visit, int* grid,
                               int* first_wg, int* rows_per_wg) {
  if (!descs || !visit || !grid || !first_wg || !rows_per_wg) return fail(VPTQ_E_NULL, "descs / visit / grid / first_wg / rows_per_wg is NULL");
  if (n < 1 || n > 32) return fail(VPTQ_E_SHAPE, "n %d outside [1, 32] (one persistent launch)", n);
  if (workgroups < 0) return fail(VPTQ_E_SHAPE, "workgroups %d < 0", workgroups);
  for (int i = 0; i < n; ++i) {
    const int rc = validate_layer(&descs[i]);
    if (rc) return rc;
  }
  flags = drop_redundant_selective(flags);
  if (!chain_kernel_takes(descs, n, nullptr, 1, flags))
    return fail(VPTQ_E_UNSUPPORTED, "the persistent chain launch does not take these layers with flags 0x%x", flags);
  const hipError_t e = vptq::gemv_k256c_plan(descs, n, (flags & VPTQ_GEMV_CHAIN_DEPENDENT) != 0, workgroups, visit, grid,
                                             first_wg, rows_per_wg);
  if (e != hipSuccess) return fail(VPTQ_E_UNSUPPORTED, "no persistent chain launch for these layers (%s)", hipGetErrorString(e));
  return VPTQ_OK;
}

int vptq_quant_gemv_chain_rows_plan(const VptqLayerDesc* descs, int n, int flags, int workgroups, int* taken, int* grid,
                                    int* first_wg, int* tasks, int* steps, int* longest) {
  if (!descs || !taken || !grid || !first_wg || !tasks || !steps || !longest)
    return fail(VPTQ_E_NULL, "descs / taken / grid / first_wg / tasks / steps / longest is NULL");
  if (n < 1 || n > 32) return fail(VPTQ_E_SHAPE, "n %d outside [1, 32] (one persistent launch)", n);
  if (workgroups < 0) return fail(VPTQ_E_SHAPE, "workgroups %d < 0", workgroups);
  for (int i = 0; i < n; ++i) {
    const int rc = validate_layer(&descs[i]);
    if (rc) return rc;
  }
  flags = drop_redundant_selective(flags);
  if (!chain_kernel_takes(descs, n, nullptr, 1, flags))
    return fail(VPTQ_E_UNSUPPORTED, "the persistent chain launch does not take these layers with flags 0x%x", flags);
  const hipError_t e = vptq::gemv_k256c_rows_plan(descs, n, flags & ~VPTQ_GEMV_CHAIN_DEPENDENT, (flags & VPTQ_GEMV_CHAIN_DEPENDENT) != 0,
                                                  workgroups, taken, grid, first_wg, tasks, steps, longest);
  if (e != hipSuccess) return fail(VPTQ_E_UNSUPPORTED, "the rows geometry does not serve these layers with flags 0x%x", flags);
  return VPTQ_OK;
}

// (chain_decide with the workspace ..._workspace_bytes_for asks for assumed, as vptq_quant_gemv_chain_kernel_name does)
int vptq_quant_gemv_chain_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes) {
  if (!descs || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / buf is NULL");
  buf[0] = 0;
  if (n < 1 || n > VPTQ_CHAIN_MAX) return fail(VPTQ_E_SHAPE, "n %d outside [1, %d]", n, VPTQ_CHAIN_MAX);
  if (tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS) return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d]", tokens, VPTQ_GEMV_MAX_TOKENS);
  for (int i = 0; i < n; ++i) {
    const int rc = validate_layer(&descs[i]);
    if (rc) return rc;
  }
  const ChainDecision D = chain_decide(descs, n, nullptr, tokens, flags, true, nullptr, 0);
  const bool dependent = D.dependent;
  flags = D.flags;
  const int lflags = flags & ~VPTQ_GEMV_CHAIN_DEPENDENT;
  Text t = {buf, bytes, 0, true};
  const VptqLayerDesc* run = D.absorbed ? D.run.data() : descs;   // what the persistent launch is given
  const ChainRoute route = D.route;
  if (route == kChainGrouped) {
    char one[2048];
    const int rc = vptq_quant_gemv_grouped_instance(descs, n, tokens, lflags & ~VPTQ_GEMV_FORCE_MFMA, one, sizeof(one));
    if (rc) return rc;
    t.add("grouped: %s", one);
    return instance_done(t);
  }
  if (route == kChainPerLayer) {
    t.add("per-layer: ");
    for (int i = 0; i < n; ++i) {
      if (i) t.add(" | ");
      const int rc = add_one(t, descs[i], tokens, lflags & ~VPTQ_GEMV_FORCE_MFMA);
      if (rc) return rc;
    }
    return instance_done(t);
  }
  static const char* const mode_text[3] = {"folded", "exact", "selective"};
  for (int i0 = 0; i0 < n; i0 += 32) {   // one persistent launch per <= 32 layers
    const int m = n - i0 < 32 ? n - i0 : 32;
    const int mode = vptq::gemv_k256c_mode(lflags, dependent);
    if (mode < 0 || mode > 2) return fail(VPTQ_E_UNSUPPORTED, "instance: no gemv_k256c instantiation for flags 0x%x", flags);
    t.add("%sgemv_k256c dt=%s dep=%d mode=%s layers=%d sweeps=", i0 ? " | " : "", dt_text(descs[0].dtype == VPTQ_DTYPE_F16), (int)dependent, mode_text[mode], m);
    for (int i = 0; i < m; ++i) t.add("%s%d", i ? "," : "", vptq::gemv_k256c_sweeps(run[i0 + i]));
    t.add(" perm=");
    for (int i = 0; i < m; ++i) t.add("%s%d", i ? "," : "", descs[i0 + i].perm ? 1 : 0);
    // (only where the launch takes its second geometry, gemv_k256c_rows_kernel: every other launch's text is what it was)
    if (vptq::gemv_k256c_rows(run + i0, m, lflags, dependent)) t.add(" geom=rows");
  }
  return instance_done(t);
}

int vptq_quant_gemv_chain(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y,
                          int tokens, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (!descs || !x || !y) return fail(VPTQ_E_NULL, "descs / x / y is NULL");
  if (n < 1 || n > VPTQ_CHAIN_MAX) return fail(VPTQ_E_SHAPE, "n %d outside [1, %d]", n, VPTQ_CHAIN_MAX);
  if (tokens < 1 || tokens > VPTQ_GEMV_MAX_TOKENS)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [1, %d]", tokens, VPTQ_GEMV_MAX_TOKENS);
  for (int i = 0; i < n; ++i) {
    const int rc = validate_layer(&descs[i]);
    if (rc) return rc;
    if (!x[i] || !y[i]) return fail(VPTQ_E_NULL, "x[%d] / y[%d] is NULL", i, i);
  }
  const ChainDecision D = chain_decide(descs, n, x, tokens, flags, false, workspace, workspace_bytes);
  const bool dependent = D.dependent;
  flags = D.flags;
  char* thr_ws = nullptr;
  if (D.sel_bytes) {
    thr_ws = (char*)workspace;
    workspace = (char*)workspace + D.sel_bytes;
    workspace_bytes -= D.sel_bytes;
  }
  const int lflags = flags & ~VPTQ_GEMV_CHAIN_DEPENDENT;
  hipStream_t st = (hipStream_t)stream;
  if (D.absorbed) {
    for (int i0 = 0; i0 < n; i0 += 32) {
      const int m = n - i0 < 32 ? n - i0 : 32;
      hipError_t e = vptq::launch_permute_x(descs + i0, m, x + i0, D.xp.data() + i0, st);
      if (e != hipSuccess) return hip_fail(e, "permute_x launch");
      e = vptq::launch_gemv_k256c(D.run.data() + i0, m, D.xx.data() + i0, y + i0, lflags, false, (uint32_t*)thr_ws, st);
      if (thr_ws) thr_ws += vptq::gemv_k256c_selective_bytes(D.run.data() + i0, m);
      if (e != hipSuccess) return hip_fail(e, "gemv_k256c launch");
    }
    return VPTQ_OK;
  }
  const ChainRoute route = D.route;
  if (route == kChainGrouped)   // independent layers, one launch (it serves members it has no kernel for one by one)
    return vptq_quant_gemv_grouped(descs, n, x, y, tokens, lflags & ~VPTQ_GEMV_FORCE_MFMA, stream);
  if (route == kChainPerLayer) {
    // stream order is the dependency
    const int pflags = lflags & ~VPTQ_GEMV_FORCE_MFMA;
    for (int i = 0; i < n; ++i) {
      const int rc = vptq_quant_gemv(&descs[i], x[i], y[i], tokens, pflags, nullptr, 0, stream);
      if (rc) return rc;
    }
    return VPTQ_OK;
  }
  if (dependent) {
    const size_t need = vptq_quant_gemv_chain_workspace_bytes(n, flags);
    if (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 3) != 0)
      return fail(VPTQ_E_WORKSPACE, "dependent chain: workspace of %zu bytes (4-byte aligned) needed", need);
    const hipError_t e = hipMemsetAsync(workspace, 0, need, st);
    if (e != hipSuccess) return hip_fail(e, "chain workspace clear");
  }
  // VPTQ_K256C_PROF builds write per-wave profile words to the workspace of a non-dependent launch: only when the
  // caller handed over enough of it (256 workgroups x 16 waves x 64 words of 8 bytes)
  const bool prof_ws = !dependent && vptq::tune_env("VPTQ_K256C_PROF") && workspace && workspace_bytes >= (size_t)256 * 16 * 64 * 8;
  for (int i0 = 0; i0 < n; i0 += 32) {
    const int m = n - i0 < 32 ? n - i0 : 32;
    const hipError_t e = vptq::launch_gemv_k256c(descs + i0, m, x + i0, y + i0, lflags, dependent,
                                                 dependent ? (uint32_t*)workspace + (size_t)i0 * 256
                                                           : thr_ws ? (uint32_t*)thr_ws
                                                           : (prof_ws ? (uint32_t*)workspace : nullptr), st);
    if (thr_ws) thr_ws += vptq::gemv_k256c_selective_bytes(descs + i0, m);
    if (dependent && e == hipErrorCooperativeLaunchTooLarge) {
      // the runtime does not confirm that every workgroup of the dependent chain is resident at once (gemv_k256c.hip:launch_c, behind k256c_chain):
      // one launch per layer, stream order is the dependency - slower, never wrong (layers already walked are walked again)
      (void)hipGetLastError();
      const int pflags = lflags & ~VPTQ_GEMV_FORCE_MFMA;
      for (int i = 0; i < n; ++i) {
        const int rc = vptq_quant_gemv(&descs[i], x[i], y[i], tokens, pflags, nullptr, 0, stream);
        if (rc) return rc;
      }
      return VPTQ_OK;
    }
    if (e != hipSuccess) return hip_fail(e, "gemv_k256c launch");
  }
  return VPTQ_OK;
}

int vptq_quant_gemm_supported(const VptqLayerDesc* d) {
  return validate_layer(d) == VPTQ_OK && vptq::gemm_fused_eligible(*d) ? 1 : 0;
}

int vptq_sliced_layout_supported(const VptqLayerDesc* d) {
  return validate_layer(d) == VPTQ_OK && vptq::gemv_sliced_eligible(*d) ? vptq::gemv_sliced_slices(*d) : 0;
}

int vptq_sliced_layout_supported_for(const VptqLayerDesc* d, int flags) {
  const bool exact = (flags & VPTQ_GEMV_EXACT) != 0;
  if (flags & VPTQ_GEMV_FORCE_GENERIC) return 0;
  return validate_layer(d) == VPTQ_OK && vptq::gemv_sliced_eligible(*d, exact) ? vptq::gemv_sliced_slices(*d, exact) : 0;
}

int vptq_sliced_layout_tables(const VptqLayerDesc* d) {
  return validate_layer(d) == VPTQ_OK && vptq::gemv_sliced_eligible(*d) ? vptq::gemv_sliced_tables(*d) : 0;
}

int vptq_sliced_layout_whole_table(const VptqLayerDesc* d, int table) {
  return validate_layer(d) == VPTQ_OK && vptq::gemv_sliced_eligible(*d) ? vptq::gemv_sliced_whole_table(*d, table) : 0;
}

int vptq_sliced_layout_set(const VptqLayerDesc* d, int flags, VptqSlicedLayoutSet* out) {
  if (int rc = validate_layer(d)) return rc;
  if (!out) return fail(VPTQ_E_NULL, "out is NULL");
  const vptq::SlicedLayoutSet S = (flags & VPTQ_GEMV_FORCE_GENERIC) ? vptq::SlicedLayoutSet{} : vptq::sl_layout_set(*d, (flags & VPTQ_GEMV_EXACT) != 0);
  *out = VptqSlicedLayoutSet{S.parts, S.tables, S.slices, {S.whole[0], S.whole[1]}, S.side_bytes, {0, 0}};
  return VPTQ_OK;
}

size_t vptq_quant_gemv_sliced_workspace_bytes(const VptqLayerDesc* d) {
  return validate_layer(d) == VPTQ_OK && vptq::gemv_sliced_eligible(*d) ? vptq::gemv_sliced_workspace_bytes(*d) : 0;
}

// ---- the sliced entries' check sequences: ONE per entry shape (one token; several tokens), run by the launching entries AND by their
// *_instance queries, so a check cannot be added to one and forgotten in the other.  io: the call's x / y / workspaces - NULL in a
// query, which skips the lines that read them; everything else runs for both, in the order the launching entries have always tested
// things (their return codes depend on it).  single: the one-layer entry, whose differences from the grouped one stand here, line by
// line.  *flags: in as the caller passed them, out as the launch takes them.
struct SlicedBuffers { const void* x; void* const* y; void* const* ws; const size_t* ws_bytes; };
static bool x_misaligned(const SlicedBuffers* io) { return io && (((uintptr_t)io->x) & 15) != 0; }
static const char* const kGroupNull = "descs / layouts / x / y / workspaces is NULL";

// tokens: the query's own argument (the launching entries have none: 1)
static int check_sliced_one(const char* who, bool single, const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, int tokens,
                            int* flags, const SlicedBuffers* io) {
  if (!single) {
    if (!descs || !layouts || (io && (!io->x || !io->y || !io->ws || !io->ws_bytes))) return fail(VPTQ_E_NULL, kGroupNull);
    if (n < 1 || n > 3) return fail(VPTQ_E_SHAPE, "n %d outside [1, 3]", n);
  }
  if (tokens != 1) return fail(VPTQ_E_TOKENS, "tokens %d: the one-token entries (several tokens: vptq_quant_gemv_sliced_tokens_instance)", tokens);
  for (int i = 0; i < n; ++i) {
    if (int rc = validate_layer(&descs[i])) return rc;
    if (!single && io && !io->y[i]) return fail(VPTQ_E_NULL, "y[%d] is NULL", i);
  }
  if (single && (!layouts || (io && (!io->x || !io->y[0])))) return fail(VPTQ_E_NULL, "x / y / layout is NULL");
  // (the one-layer entry has a selective form; the grouped launch has none: the reference's roundings)
  *flags = single ? drop_redundant_selective(*flags) : selective_as_exact(*flags);
  const bool exact = (*flags & VPTQ_GEMV_EXACT) != 0, sel = (*flags & VPTQ_GEMV_SELECTIVE) != 0;
  if (*flags & VPTQ_GEMV_FORCE_GENERIC) return fail(VPTQ_E_UNSUPPORTED, "VPTQ_GEMV_FORCE_GENERIC: use vptq_quant_gemv");
  if (single) {
    if (sel && !vptq::gemv_hot_eligible(descs[0]))
      return fail(VPTQ_E_UNSUPPORTED, "VPTQ_GEMV_SELECTIVE over a sliced layout: fp16 layers the folded sliced kernel serves, with scale and bias "
                                      "(vptq_quant_gemv_sliced_selective_supported); ask for VPTQ_GEMV_EXACT over an exact layout instead");
    if (!vptq::gemv_sliced_eligible(descs[0], exact))
      return fail(VPTQ_E_UNSUPPORTED, exact ? "VPTQ_GEMV_EXACT over a sliced layout: v = 8 / 16, 16384 ... 65536 main centroids, no residual "
                                              "codebook or the 256-entry one of v = 8, scale / bias / x of every column beside a slice in LDS "
                                              "(vptq_sliced_layout_supported_for)"
                                            : "the sliced layout serves v = 8 / 16 layers with 16384 ... 65536 main centroids, group_size <= 32768");
  } else {
    if ((*flags & VPTQ_GEMV_COLUMN_PARTS) && (!exact || (io && !vptq::sl_parts_share(descs, io->y, io->ws, n)))) return fail(VPTQ_E_UNSUPPORTED, kPartsShare);
    if (!vptq::gemv_sliced_groupable(descs, n, exact))
      return fail(VPTQ_E_UNSUPPORTED, "a sliced group takes layers of ONE format, dtype and input width that vptq_sliced_layout_supported_for() accepts");
    if (x_misaligned(io)) return fail(VPTQ_E_UNSUPPORTED, "x must be 16-byte aligned");
  }
  for (int i = 0; i < n; ++i) {
    if (io) {   // (selective: the pre-pass's buffers behind the accumulator words, 256-byte aligned)
      const size_t acc = vptq::gemv_sliced_workspace_bytes(descs[i]);
      const size_t need = sel ? (acc + 255) / 256 * 256 + vptq::gemv_hot_bytes(descs[i]) : acc;
      if (!io->ws[i] || io->ws_bytes[i] < need || (((uintptr_t)io->ws[i]) & (sel ? 255 : 15)) != 0)
        return single ? fail(VPTQ_E_WORKSPACE, "workspace of %zu bytes (%d-byte aligned) needed", need, sel ? 256 : 16)
                      : fail(VPTQ_E_WORKSPACE, "layer %d: workspace of %zu bytes (16-byte aligned) needed", i, need);
    }
    // (folded, two tables: one layout per table, consecutive structs; the reference's roundings: always ONE layout; one format: the
    // same table count for every member)
    const vptq::SlicedLayoutSet S = vptq::sl_piece_set(descs[i], exact);
    int which = 0;
    if (const unsigned faults = vptq::sl_check_layouts(descs[i], S, layouts + (size_t)i * S.tables, S.tables, vptq::kSLNeedRows | vptq::kSLNeedWhole,
                                                       layouts[0].rows_per_wave, &which))
      return layout_fail(faults, true, who, i, which, S);
  }
  if (single && x_misaligned(io)) return fail(VPTQ_E_UNSUPPORTED, "x must be 16-byte aligned");
  return VPTQ_OK;
}

int vptq_quant_gemv_sliced(const VptqLayerDesc* d, const VptqSlicedLayout* layout, const void* x, void* y, int flags,
                           void* workspace, size_t workspace_bytes, void* stream) {
  void* const ys[1] = {y};
  void* const wss[1] = {workspace};
  const SlicedBuffers io = {x, ys, wss, &workspace_bytes};
  if (int rc = check_sliced_one("vptq_quant_gemv_sliced", true, d, layout, 1, 1, &flags, &io)) return rc;
  if (flags & VPTQ_GEMV_SELECTIVE) {
    const size_t acc_bytes = (vptq::gemv_sliced_workspace_bytes(*d) + 255) / 256 * 256;
    // the pre-pass (gemv_hot.hip): threshold, x with the hot blocks' features zeroed, the hot blocks' exact products - behind the
    // accumulator words of the same workspace; then the folded launch over x_masked, which adds the products before its rounding
    const void* xm = nullptr;
    const float* corr = nullptr;
    hipError_t e = vptq::launch_gemv_hot(*d, x, (char*)workspace + acc_bytes, &xm, &corr, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gemv_hot launch");
    e = vptq::launch_gemv_sliced(*d, layout, xm, y, flags & ~VPTQ_GEMV_SELECTIVE, workspace, (hipStream_t)stream, corr);
    return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemv_sliced launch");
  }
  const hipError_t e = vptq::launch_gemv_sliced(*d, layout, x, y, flags, workspace, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemv_sliced launch");
}

int vptq_sliced_layout_repack(const VptqLayerDesc* d, const VptqSlicedLayout* layouts, int parts, void* indices_out, void* stream) {
  if (int rc = validate_layer(d)) return rc;
  if (!layouts || !indices_out) return fail(VPTQ_E_NULL, "layouts / indices_out is NULL");
  const vptq::SlicedLayoutSet S = vptq::sl_layout_set(*d, true);
  if (S.parts == 0) return fail(VPTQ_E_UNSUPPORTED, kNoExactLayout);
  if (parts != S.parts) return fail(VPTQ_E_SHAPE, "parts %d: the exact layouts of this layer come in %d column part(s)", parts, S.parts);
  if ((((uintptr_t)indices_out) & 15) != 0) return fail(VPTQ_E_ALIGN, "indices_out must be 16-byte aligned");
  if (vptq::sliced_repack_lds_bytes(*d) > 163840) return fail(VPTQ_E_UNSUPPORTED, "row_words %d: a row's image exceeds the LDS", d->row_words);
  int which = 0;   // (folded layouts - two tables, whole tables - do not hold the packed stream)
  if (const unsigned faults = vptq::sl_check_layouts(*d, S, layouts, parts, vptq::kSLNeedBuilt | vptq::kSLNeedWhole | vptq::kSLNeedRes8, 0, &which))
    return layout_fail(faults, false, "vptq_sliced_layout_repack", which, 0, S);
  const hipError_t e = vptq::launch_sliced_repack(*d, layouts, parts, S.side_bytes, indices_out, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "sliced_repack launch");
}

int vptq_dequant_sliced(const VptqLayerDesc* d, const VptqSlicedLayout* layouts, int parts, void* W, void* stream) {
  if (int rc = validate_layer(d)) return rc;
  if (!layouts || !W) return fail(VPTQ_E_NULL, "layouts / W is NULL");
  const vptq::SlicedLayoutSet S = vptq::sl_layout_set(*d, true);
  if (S.parts == 0) return fail(VPTQ_E_UNSUPPORTED, kNoExactLayout);
  if (parts != S.parts) return fail(VPTQ_E_SHAPE, "parts %d: the exact layouts of this layer come in %d column part(s)", parts, S.parts);
  if ((((uintptr_t)W) & 15) != 0) return fail(VPTQ_E_ALIGN, "W must be 16-byte aligned");
  if (!vptq::dequant_sliced_eligible(*d)) return fail(VPTQ_E_UNSUPPORTED, "vptq_dequant_sliced: v = 8 / 16 layers of one codebook group with scale and bias, a multiple of 8 columns");
  int which = 0;   // (the checks of vptq_sliced_layout_repack: folded layouts - two tables, whole tables - do not hold the packed stream)
  if (const unsigned faults = vptq::sl_check_layouts(*d, S, layouts, parts, vptq::kSLNeedBuilt | vptq::kSLNeedWhole | vptq::kSLNeedRes8, 0, &which))
    return layout_fail(faults, false, "vptq_dequant_sliced", which, 0, S);
  for (int p = 0; p < parts; ++p)   // (optional here, read where set: the lists' window order bounds a tile's walk)
    if ((((uintptr_t)layouts[p].wstart) & 3) != 0) return fail(VPTQ_E_ALIGN, "vptq_dequant_sliced: part %d: wstart must be 4-byte aligned", p);
  const hipError_t e = vptq::launch_dequant_sliced(*d, layouts, parts, S.side_bytes, W, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "dequant_sliced launch");
}

// what vptq_sliced_layout_plan / _fill build for (desc, spec): validation of the spec against the layouts the GEMV entries take for
// the layer (VPTQ_LAYOUT_ANY_SHAPE: against the index widths alone), then the kernel's parameters
static int layout_build_params(const VptqLayerDesc* d, const VptqSlicedLayoutSpec* spec, vptq::LayoutBuildParams* P) {
  if (int rc = validate_layer(d)) return rc;
  if (!spec) return fail(VPTQ_E_NULL, "spec is NULL");
  const VptqSlicedLayoutSpec& s = *spec;
  if (s.flags & ~(VPTQ_GEMV_EXACT | VPTQ_LAYOUT_ANY_SHAPE)) return fail(VPTQ_E_UNSUPPORTED, "spec flags 0x%x: VPTQ_GEMV_EXACT and VPTQ_LAYOUT_ANY_SHAPE only", s.flags);
  const bool exact = (s.flags & VPTQ_GEMV_EXACT) != 0, any = (s.flags & VPTQ_LAYOUT_ANY_SHAPE) != 0;
  if (d->num_codebooks != 1 || d->outlier_size != 0 || d->group_size != d->in_features || d->group_size > 32768)
    return fail(VPTQ_E_UNSUPPORTED, "a sliced layout is built for layers of one codebook group without outlier columns, group_size <= 32768");
  if (s.parts < 1 || s.parts > 3 || s.part < 0 || s.part >= s.parts || d->group_size % s.parts != 0)
    return fail(VPTQ_E_SHAPE, "part %d of %d parts: 1 - 3 equal column parts of the layer's %d columns", s.part, s.parts, d->group_size);
  if (s.n_slices != 8 && s.n_slices != 16 && s.n_slices != 32) return fail(VPTQ_E_SHAPE, "n_slices %d: 8, 16 or 32", s.n_slices);
  if (s.table < 0 || s.table > 1 || (s.table == 1 && d->num_res_centroids == 0))
    return fail(VPTQ_E_UNSUPPORTED, "table %d: 0, or 1 for a layer with a residual codebook", s.table);
  if (s.side_bytes < 0 || s.side_bytes > 2 || (s.side_bytes && (d->num_res_centroids == 0 || s.table != 0)) || (s.side_bytes == 1 && d->res_bits > 8))
    return fail(VPTQ_E_UNSUPPORTED, "side_bytes %d: 1 (up to 256 residual centroids) or 2 beside a table-0 layout of a layer with a residual codebook, else 0", s.side_bytes);
  if (s.whole_table != 0 && s.whole_table != 1) return fail(VPTQ_E_UNSUPPORTED, "whole_table %d: 0 or 1", s.whole_table);
  const int lg = s.n_slices == 8 ? 3 : (s.n_slices == 16 ? 4 : 5);
  const int bits = s.table ? d->res_bits : d->index_bits;
  if (!any) {
    // the layouts the GEMV entries take for the layer
    const vptq::SlicedLayoutSet S = vptq::sl_layout_set(*d, exact);
    if (S.parts == 0)
      return fail(VPTQ_E_UNSUPPORTED, exact ? kNoExactLayout : "the sliced layout serves v = 8 / 16 layers with 16384 ... 65536 main centroids, group_size <= 32768");
    if (s.parts != S.parts)
      return exact ? fail(VPTQ_E_SHAPE, "parts %d: the exact layouts of this layer come in %d column part(s)", s.parts, S.parts)
                   : fail(VPTQ_E_SHAPE, "parts %d: column parts are layouts of the reference's roundings (VPTQ_GEMV_EXACT)", s.parts);
    if (s.n_slices != S.slices) return fail(VPTQ_E_SHAPE, "n_slices %d: this layout of the layer has %d (vptq_sliced_layout_set)", s.n_slices, S.slices);
    if (s.table >= S.tables) return fail(VPTQ_E_UNSUPPORTED, "table %d: this arithmetic serves the layer from %d layout(s) per part (vptq_sliced_layout_set)", s.table, S.tables);
    if (s.whole_table != S.whole[s.table]) return fail(VPTQ_E_UNSUPPORTED, "whole_table %d: must be %d (vptq_sliced_layout_set)", s.whole_table, S.whole[s.table]);
    if (s.side_bytes != S.side_bytes) return fail(VPTQ_E_UNSUPPORTED, "side_bytes %d: this layout carries %d", s.side_bytes, S.side_bytes);
  }
  vptq::LayoutBuildParams a = {};
  a.packed = (const uint32_t*)d->indices;
  a.N = d->num_indices;
  a.row_words = d->row_words;
  a.T = d->index_bits + d->res_bits;
  a.W = d->group_size / s.parts;
  a.c0 = s.part * a.W;
  a.wcols = (a.W + VPTQ_SLICED_WINDOWS * 8 - 1) / (VPTQ_SLICED_WINDOWS * 8) * 8;
  const int last = a.W - (VPTQ_SLICED_WINDOWS - 1) * a.wcols;
  a.cap = a.wcols < a.W ? a.wcols : a.W;
  if (last > a.cap) a.cap = last;
  a.S = s.n_slices;
  a.slice_bits = s.whole_table || bits < lg ? 0 : bits - lg;   // (fewer entries than slices: slice = index, as the recipe has it)
  a.bucket_shift = s.table ? d->index_bits : 0;
  a.bucket_mask = (1u << bits) - 1u;
  a.whole = s.whole_table;
  a.side = s.side_bytes;
  a.side_shift = d->index_bits;
  *P = a;
  return VPTQ_OK;
}

int vptq_sliced_layout_plan(const VptqLayerDesc* d, const VptqSlicedLayoutSpec* spec, void* blocks, void* first, void* wstart,
                            void* total_blocks, void* stream) {
  vptq::LayoutBuildParams a;
  if (int rc = layout_build_params(d, spec, &a)) return rc;
  if (!blocks || !first || !wstart || !total_blocks) return fail(VPTQ_E_NULL, "blocks / first / wstart / total_blocks is NULL");
  if ((((uintptr_t)blocks | (uintptr_t)first | (uintptr_t)wstart) & 3) != 0 || (((uintptr_t)total_blocks) & 7) != 0)
    return fail(VPTQ_E_ALIGN, "blocks / first / wstart 4-byte, total_blocks 8-byte aligned");
  a.blocks = (int32_t*)blocks;
  a.first = (int32_t*)first;
  a.wstart = (int32_t*)wstart;
  a.total = (long long*)total_blocks;
  const hipError_t e = vptq::launch_layout_plan(a, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "sliced layout plan launch");
}

int vptq_sliced_layout_fill(const VptqLayerDesc* d, const VptqSlicedLayoutSpec* spec, const VptqSlicedLayout* out, int64_t total_blocks,
                            void* stream) {
  vptq::LayoutBuildParams a;
  if (int rc = layout_build_params(d, spec, &a)) return rc;
  if (!out) return fail(VPTQ_E_NULL, "out is NULL");
  // (`out` is held to the SPEC - with VPTQ_LAYOUT_ANY_SHAPE that need not be a layout of the layer's set; whole_table is not read)
  vptq::SlicedLayoutSet S = {};
  S.parts = spec->parts, S.tables = 1, S.slices = spec->n_slices, S.whole[0] = spec->whole_table, S.side_bytes = a.side;
  const unsigned faults = vptq::sl_check_layouts(*d, S, out, 1, vptq::kSLNeedBuilt | vptq::kSLNeedWstart);
  // this entry's order of reasons: NULL tensors, `res`, n_slices, then total_blocks, then the alignments
  for (const unsigned first : {vptq::kSLFaultTensors, vptq::kSLFaultRes, vptq::kSLFaultSlices})
    if (faults & first) return layout_fail(first, false, "vptq_sliced_layout_fill", spec->part, 0, S, "the spec");
  if (total_blocks < 0 || total_blocks >= (1ll << 31)) return fail(VPTQ_E_SHAPE, "total_blocks %lld outside [0, 2^31)", (long long)total_blocks);
  if (faults) return layout_fail(faults, false, "vptq_sliced_layout_fill", spec->part, 0, S, "the spec");
  a.blocks = (int32_t*)out->blocks;
  a.first = (int32_t*)out->first;
  a.wstart = (int32_t*)out->wstart;
  a.elems = (uint32_t*)out->elems;
  a.res = (void*)out->res;
  a.total_blocks = total_blocks;
  const hipError_t e = vptq::launch_layout_fill(a, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "sliced layout fill launch");
}

int vptq_quant_gemv_sliced_selective_supported(const VptqLayerDesc* d) {
  return validate_layer(d) == VPTQ_OK && vptq::gemv_hot_eligible(*d) ? 1 : 0;
}
size_t vptq_quant_gemv_sliced_workspace_bytes_for(const VptqLayerDesc* d, int flags) {
  if (validate_layer(d) != VPTQ_OK || !vptq::gemv_sliced_eligible(*d, (flags & VPTQ_GEMV_EXACT) != 0)) return 0;
  flags = drop_redundant_selective(flags);
  if (!(flags & VPTQ_GEMV_SELECTIVE)) return vptq::gemv_sliced_workspace_bytes(*d);
  return vptq::gemv_hot_eligible(*d) ? (vptq::gemv_sliced_workspace_bytes(*d) + 255) / 256 * 256 + vptq::gemv_hot_bytes(*d) : 0;
}

int vptq_quant_gemv_sliced_tokens_supported(const VptqLayerDesc* d, const VptqSlicedLayout* layout, int tokens) {
  return vptq_quant_gemv_sliced_tokens_supported_for(d, layout, tokens, 0);
}
int vptq_quant_gemv_sliced_tokens_supported_for(const VptqLayerDesc* d, const VptqSlicedLayout* layout, int tokens, int flags) {
  flags = selective_as_exact(flags);
  if (flags & ~(VPTQ_GEMV_EXACT | VPTQ_GEMV_OUT_F32)) return 0;
  return validate_layer(d) == VPTQ_OK && layout && vptq::gemv_sliced_tok_eligible(*d, layout, tokens, (flags & VPTQ_GEMV_EXACT) != 0) ? 1 : 0;
}

int vptq_quant_gemv_sliced_tokens_one_pass(const VptqLayerDesc* d, int tokens, int flags) {
  flags = selective_as_exact(flags);
  if (validate_layer(d) != VPTQ_OK || (flags & ~(VPTQ_GEMV_EXACT | VPTQ_GEMV_OUT_F32))) return 0;
  return vptq::gemv_sliced_tok_one_pass_parts(*d, tokens, (flags & VPTQ_GEMV_EXACT) != 0);
}

size_t vptq_quant_gemv_sliced_tokens_workspace_bytes(const VptqLayerDesc* d, int tokens) {
  return validate_layer(d) == VPTQ_OK && (vptq::gemv_sliced_eligible(*d) || vptq::gemv_sliced_eligible(*d, true)) && tokens >= 2 && tokens <= 8
             ? vptq::gemv_sliced_tok_workspace_bytes(*d, tokens) : 0;
}

// ... for several tokens (as check_sliced_one: one sequence for the launching entries and the query).  The query names what the
// launching entries turn down together with everything else their kernels do not take: n as VPTQ_E_SHAPE, the token count as VPTQ_E_TOKENS.
static int check_sliced_tokens(bool single, const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, int tokens, int* flags,
                               const SlicedBuffers* io) {
  *flags = selective_as_exact(*flags);   // (no selective form over several tokens: the reference's roundings)
  if (!single) {
    if (!descs || !layouts || (io && (!io->x || !io->y || !io->ws || !io->ws_bytes))) return fail(VPTQ_E_NULL, kGroupNull);
    if (n < 1 || n > 3) return io ? fail(VPTQ_E_UNSUPPORTED, "a sliced group takes 1 .. 3 layers") : fail(VPTQ_E_SHAPE, "n %d outside [1, 3]", n);
  }
  if (!io && (tokens < 2 || tokens > 8)) return fail(VPTQ_E_TOKENS, "tokens %d outside [2, 8]", tokens);
  for (int i = 0; i < n; ++i) {
    if (int rc = validate_layer(&descs[i])) return rc;
    if (!single && io && !io->y[i]) return fail(VPTQ_E_NULL, "y[%d] is NULL", i);
  }
  if (single && (!layouts || (io && (!io->x || !io->y[0])))) return fail(VPTQ_E_NULL, "layout, x and y must be set");
  if (*flags & VPTQ_GEMV_FORCE_GENERIC) return fail(VPTQ_E_UNSUPPORTED, "the sliced path is not the generic kernel: use vptq_quant_gemv");
  const bool exact = (*flags & VPTQ_GEMV_EXACT) != 0;
  if (!single && (*flags & VPTQ_GEMV_COLUMN_PARTS)) {   // (as vptq_quant_gemv_sliced_grouped: parts of ONE layer; 2 / 3 tokens, where every part takes them in one pass)
    if (!exact || (io && !vptq::sl_parts_share(descs, io->y, io->ws, n))) return fail(VPTQ_E_UNSUPPORTED, kPartsShare);
    for (int i = 0; i < n; ++i)
      if (!vptq::gemv_sliced_tok_one_pass_parts(descs[i], tokens, true)) return fail(VPTQ_E_UNSUPPORTED, kPartsShare);
  }
  // (one layer: gemv_sliced_eligible and gemv_sliced_tok_eligible, which is what a group of one is held to)
  if (!vptq::gemv_sliced_tok_groupable(descs, layouts, n, tokens, exact))
    return fail(VPTQ_E_UNSUPPORTED, single ? "sliced layouts with column windows (wstart), 2 - 8 tokens, and activations that fit the LDS beside the slice"
                                             " (VPTQ_GEMV_EXACT: one-table formats, a layout of vptq_sliced_layout_supported_for(desc, VPTQ_GEMV_EXACT) slices)"
                                           : "a sliced group of 2 - 4 tokens takes layers of ONE format, dtype and input width whose layouts carry wstart");
  if (!single && x_misaligned(io)) return fail(VPTQ_E_UNSUPPORTED, "x must be 16-byte aligned");
  for (int i = 0; io && i < n; ++i) {
    const size_t need = vptq::gemv_sliced_tok_workspace_bytes(descs[i], tokens);
    if (!io->ws[i] || io->ws_bytes[i] < need || (((uintptr_t)io->ws[i]) & 15) != 0)
      return single ? fail(VPTQ_E_WORKSPACE, "the sliced path for %d tokens needs %zu bytes of 16-byte aligned, zero-initialised workspace", tokens, need)
                    : fail(VPTQ_E_WORKSPACE, "layer %d: workspace of %zu bytes (16-byte aligned, zero-initialised) needed for %d tokens", i, need, tokens);
  }
  if (single && x_misaligned(io)) return fail(VPTQ_E_UNSUPPORTED, "x must be 16-byte aligned");
  return VPTQ_OK;
}

int vptq_quant_gemv_sliced_tokens(const VptqLayerDesc* d, const VptqSlicedLayout* layout, const void* x, void* y, int tokens,
                                  int flags, void* workspace, size_t workspace_bytes, void* stream) {
  void* const ys[1] = {y};
  void* const wss[1] = {workspace};
  const SlicedBuffers io = {x, ys, wss, &workspace_bytes};
  if (int rc = check_sliced_tokens(true, d, layout, 1, tokens, &flags, &io)) return rc;
  const hipError_t e = vptq::launch_gemv_sliced_tok(*d, layout, x, y, tokens, flags, workspace, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemv_sliced_tok launch");
}

int vptq_quant_gemv_sliced_grouped(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, const void* x,
                                   void* const* y, int flags, void* const* workspaces, const size_t* workspace_bytes, void* stream) {
  const SlicedBuffers io = {x, y, workspaces, workspace_bytes};
  if (int rc = check_sliced_one("vptq_quant_gemv_sliced_grouped", false, descs, layouts, n, 1, &flags, &io)) return rc;
  const hipError_t e = vptq::launch_gemv_sliced_group(descs, layouts, n, x, y, flags, workspaces, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemv_sliced grouped launch");
}

int vptq_quant_gemv_sliced_tokens_grouped(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, const void* x,
                                          void* const* y, int tokens, int flags, void* const* workspaces, const size_t* workspace_bytes,
                                          void* stream) {
  const SlicedBuffers io = {x, y, workspaces, workspace_bytes};
  if (int rc = check_sliced_tokens(false, descs, layouts, n, tokens, &flags, &io)) return rc;
  const hipError_t e = vptq::launch_gemv_sliced_tok_group(descs, layouts, n, x, y, tokens, flags, workspaces, (hipStream_t)stream);
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemv_sliced_tok grouped launch");
}

// ---- which instantiation a sliced call would launch (vptq_quant_gemv_sliced_instance / _tokens_instance): the launching entries' own
// check sequence (check_sliced_one / check_sliced_tokens without x, y and the workspaces), then the text of the very decide functions
// the launches run (sliced_host.hip: sl_decide, st_decide; gemv_hot_decide)
static int sliced_instance_rc(int rc, size_t bytes) {
  if (rc == -2) return fail(VPTQ_E_WORKSPACE, "instance: buffer of %zu bytes too small", bytes);
  return rc ? fail(VPTQ_E_UNSUPPORTED, "instance: no sliced launch serves this call") : VPTQ_OK;
}
int vptq_quant_gemv_sliced_instance(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, int tokens, int flags, char* buf,
                                    size_t bytes) {
  if (!descs || !layouts || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / layouts / buf is NULL");
  buf[0] = 0;
  const bool single = n == 1 && !(flags & VPTQ_GEMV_COLUMN_PARTS);   // vptq_quant_gemv_sliced, else vptq_quant_gemv_sliced_grouped
  if (int rc = check_sliced_one("vptq_quant_gemv_sliced_instance", single, descs, layouts, n, tokens, &flags, nullptr)) return rc;
  const bool sel = (flags & VPTQ_GEMV_SELECTIVE) != 0;
  Text t = {buf, bytes, 0, true};
  char one[384];
  if (sel) {
    if (const int rc = vptq::gemv_hot_instance(descs[0], one, sizeof(one))) return sliced_instance_rc(rc, bytes);
    t.add("%s | ", one);
  }
  if (const int rc = vptq::gemv_sliced_instance(descs, layouts, n, 1, flags & ~VPTQ_GEMV_SELECTIVE, sel, one, sizeof(one)))
    return sliced_instance_rc(rc, bytes);
  t.add("%s", one);
  return instance_done(t);
}

int vptq_quant_gemv_sliced_tokens_instance(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, int tokens, int flags,
                                           char* buf, size_t bytes) {
  if (!descs || !layouts || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / layouts / buf is NULL");
  buf[0] = 0;
  if (int rc = check_sliced_tokens(false, descs, layouts, n, tokens, &flags, nullptr)) return rc;
  char one[384];
  if (const int rc = vptq::gemv_sliced_tok_instance(descs, layouts, n, tokens, flags, one, sizeof(one))) return sliced_instance_rc(rc, bytes);
  Text t = {buf, bytes, 0, true};
  t.add("%s", one);
  return instance_done(t);
}

size_t vptq_quant_gemm_workspace_bytes(const VptqLayerDesc* d, int tokens) {
  if (validate_layer(d) != VPTQ_OK || tokens < 1) return 0;
  return vptq::gemm_fused_workspace_bytes(*d, tokens);
}

int vptq_quant_gemm(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* workspace,
                    size_t workspace_bytes, void* stream) {
  (void)flags;
  int rc = validate_layer(d);
  if (rc) return rc;
  if (!x || !y) return fail(VPTQ_E_NULL, "x / y is NULL");
  if (tokens < 1) return fail(VPTQ_E_TOKENS, "tokens %d < 1", tokens);
  if (!vptq::gemm_fused_eligible(*d))
    return fail(VPTQ_E_UNSUPPORTED, "no fused GEMM for this layer: use vptq_dequant + a dense GEMM");
  if ((((uintptr_t)x) & 15) != 0) return fail(VPTQ_E_ALIGN, "x must be 16-byte aligned");
  if (workspace_bytes < vptq::gemm_fused_workspace_bytes(*d, tokens) ||
      (vptq::gemm_fused_workspace_bytes(*d, tokens) > 0 && !workspace))
    return fail(VPTQ_E_WORKSPACE, "workspace of %zu bytes needed", vptq::gemm_fused_workspace_bytes(*d, tokens));
  hipError_t e = vptq::launch_gemm_fused(*d, x, y, tokens, workspace, workspace_bytes, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "gemm_fused launch");
  return VPTQ_OK;
}

// ---- gemm_gather.hip / gemm_gatherx.hip: 1 - 16 tokens of the large-codebook formats in one launch (added within ABI 12).  A layer
// has one of the two kernels; the entries of both are the three shapes below, given the kernel's name, what it serves, its
// eligibility function and its launcher.  gemm_k256w (gemm_k256.hip): the same three shapes for 17 - 64 tokens of the canonical format;
// gemm_gatherw (gemm_gatherw.hip): for 17 - 48 tokens of gemm_gather's layers
struct BatchedDecode {
  const char* name;
  int tok_lo, tok_hi;        // the token counts of one launch
  int misaligned;            // the code of an x that is not 16-byte aligned
  const char* launch_what;   // hip_fail's "what" of a failed launch
  const char* serves;
  bool (*eligible)(const VptqLayerDesc&, int);
  hipError_t (*launch)(const VptqLayerDesc&, const void*, void*, int, bool, hipStream_t);
  void (*print)(Text&, const VptqLayerDesc&, int);   // the kernel's own decision as its instance line
};
static void print_gemm_gather(Text& t, const VptqLayerDesc& d, int tokens) {
  const vptq::GemmGatherDecision D = vptq::gemm_gather_decide(d, tokens);
  t.add("gemm_gather dt=%s t=%d perm=%d tok=%d tiles=%d rgs=%d", dt_text(D.f16), D.T, (int)D.perm, D.tok, D.tiles, D.rgs);
}
static void print_gemm_gatherx(Text& t, const VptqLayerDesc& d, int tokens) {
  const vptq::GemmGatherXDecision D = vptq::gemm_gatherx_decide(d, tokens);
  t.add("gemm_gatherx dt=%s v=%d ib=%d rb=%d res=%s perm=%d tok=%d tiles=%d wgcu=%d rgs=%d", dt_text(D.f16), D.v, D.ib, D.rb,
        D.res == 0 ? "none" : D.res == 1 ? "lds" : "l2", (int)D.perm, D.tok, D.tiles, D.wgcu, D.rgs);
}
static void print_gemm_k256w(Text& t, const VptqLayerDesc& d, int tokens) {
  const vptq::GemmK256WDecision D = vptq::gemm_k256w_decide(d, tokens);
  t.add("gemm_k256w dt=%s perm=%d tok=%d tb=%d rgs=%d pass=1x%d", dt_text(D.f16), (int)D.perm, D.tok, D.tb, D.rgs, D.tb);
}
static void print_gemm_gatherw(Text& t, const VptqLayerDesc& d, int tokens) {
  const vptq::GemmGatherWDecision D = vptq::gemm_gatherw_decide(d, tokens);
  t.add("gemm_gatherw dt=%s t=%d perm=%d tok=%d tb=%d tiles=%d rgs=%d", dt_text(D.f16), D.T, (int)D.perm, D.tok, D.tb, D.tiles, D.rgs);
}
static const BatchedDecode kGemmGather = {
  "gemm_gather", 1, 16, VPTQ_E_UNSUPPORTED, "gemm_gather launch", "v = 8, 65536 main centroids, 0 / 256 / 65536 residual centroids, one codebook, no outlier columns, scale and bias, "
  "group_size == in_features (a multiple of 8), 16-byte aligned tables", vptq::gemm_gather_eligible, vptq::launch_gemm_gather,
  print_gemm_gather};
static const BatchedDecode kGemmGatherX = {
  "gemm_gatherx", 1, 16, VPTQ_E_UNSUPPORTED, "gemm_gatherx launch", "v = 8 / 16, 16384 ... 65536 main centroids, any residual codebook (index_bits + res_bits <= 32), one codebook, no "
  "outlier columns, scale and bias, group_size == in_features (a multiple of 8), 16-byte aligned tables - and not the layers gemm_gather "
  "serves", vptq::gemm_gatherx_eligible, vptq::launch_gemm_gatherx, print_gemm_gatherx};

static const BatchedDecode kGemmK256W = {
  "gemm_k256w", 17, 64, VPTQ_E_TOKENS, "gemm_k256w launch", "the canonical format (v = 8, 256 + 256 centroids, one codebook, no outlier columns, "
  "scale and bias, group_size == in_features (a multiple of 8), with perm: scale_permuted and bias_permuted)", vptq::gemm_k256w_eligible,
  vptq::launch_gemm_k256w, print_gemm_k256w};

// gemm_gatherw (gemm_gatherw.hip): gemm_gather's layers, 17 - 48 tokens
static const BatchedDecode kGemmGatherW = {
  "gemm_gatherw", 17, 48, VPTQ_E_TOKENS, "gemm_gatherw launch", "v = 8, 65536 main centroids, 0 / 256 / 65536 residual centroids, one codebook, no outlier columns, scale and bias, "
  "group_size == in_features (a multiple of 8), 16-byte aligned tables", vptq::gemm_gatherw_eligible, vptq::launch_gemm_gatherw,
  print_gemm_gatherw};

static int batched_supported(const BatchedDecode& k, const VptqLayerDesc* d, int tokens) {
  return validate_layer(d) == VPTQ_OK && k.eligible(*d, tokens) ? 1 : 0;
}

// the checks of an entry and its `_instance` on the token count and the layer
static int batched_validate(const BatchedDecode& k, const VptqLayerDesc* d, int tokens) {
  if (tokens < k.tok_lo || tokens > k.tok_hi) return fail(VPTQ_E_TOKENS, "tokens %d outside [%d, %d]", tokens, k.tok_lo, k.tok_hi);
  if (!k.eligible(*d, tokens)) return fail(VPTQ_E_UNSUPPORTED, "%s serves %s", k.name, k.serves);
  return VPTQ_OK;
}

static int batched_launch(const BatchedDecode& k, const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* stream) {
  // (VPTQ_GEMV_FAST_MATH / _SELECTIVE / _EXACT: the kernels have the reference's roundings only)
  if (const int rc = validate_layer(d)) return rc;
  if (!x || !y) return fail(VPTQ_E_NULL, "x / y is NULL");
  if (const int rc = batched_validate(k, d, tokens)) return rc;
  if ((((uintptr_t)x) & 15) != 0) return fail(k.misaligned, "%s: x must be 16-byte aligned", k.name);
  const hipError_t e = k.launch(*d, x, y, tokens, (flags & VPTQ_GEMV_OUT_F32) != 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, k.launch_what);
  return VPTQ_OK;
}

static int batched_instance(const BatchedDecode& k, const VptqLayerDesc* d, int tokens, char* buf, size_t bytes) {
  if (!d || !buf || bytes < 1) return fail(VPTQ_E_NULL, "desc / buf is NULL");
  buf[0] = 0;
  if (const int rc = validate_layer(d)) return rc;
  if (const int rc = batched_validate(k, d, tokens)) return rc;
  Text t = {buf, bytes, 0, true};
  k.print(t, *d, tokens);
  if (!t.fits) buf[0] = 0;
  return instance_done(t);
}

int vptq_quant_gemm_gather_supported(const VptqLayerDesc* d, int tokens) { return batched_supported(kGemmGather, d, tokens); }
int vptq_quant_gemm_gather(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* stream) { return batched_launch(kGemmGather, d, x, y, tokens, flags, stream); }
int vptq_quant_gemm_gather_instance(const VptqLayerDesc* d, int tokens, int, char* buf, size_t bytes) { return batched_instance(kGemmGather, d, tokens, buf, bytes); }
int vptq_quant_gemm_gatherx_supported(const VptqLayerDesc* d, int tokens) { return batched_supported(kGemmGatherX, d, tokens); }
int vptq_quant_gemm_gatherx(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* stream) { return batched_launch(kGemmGatherX, d, x, y, tokens, flags, stream); }
int vptq_quant_gemm_gatherx_instance(const VptqLayerDesc* d, int tokens, int, char* buf, size_t bytes) { return batched_instance(kGemmGatherX, d, tokens, buf, bytes); }
int vptq_quant_gemm_k256w_supported(const VptqLayerDesc* d, int tokens) { return batched_supported(kGemmK256W, d, tokens); }
int vptq_quant_gemm_k256w(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* stream) { return batched_launch(kGemmK256W, d, x, y, tokens, flags, stream); }
int vptq_quant_gemm_k256w_instance(const VptqLayerDesc* d, int tokens, int, char* buf, size_t bytes) { return batched_instance(kGemmK256W, d, tokens, buf, bytes); }
int vptq_quant_gemm_gatherw_supported(const VptqLayerDesc* d, int tokens) { return batched_supported(kGemmGatherW, d, tokens); }
int vptq_quant_gemm_gatherw(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* stream) { return batched_launch(kGemmGatherW, d, x, y, tokens, flags, stream); }
int vptq_quant_gemm_gatherw_instance(const VptqLayerDesc* d, int tokens, int, char* buf, size_t bytes) { return batched_instance(kGemmGatherW, d, tokens, buf, bytes); }

// ---- gemm_gather_px.hip (added within ABI 12): 1 - 48 tokens of a layer of the three entries above with x[perm] written once into a
// workspace, then the layer's own kernel in its form without a permutation.  The entry of a (layer, token count): gemm_gather or
// gemm_gatherx up to 16 tokens (a layer has one of the two), gemm_gatherw from 17; NULL where none serves it
static const BatchedDecode* px_inner(const VptqLayerDesc& d, int tokens) {
  if (tokens > kGemmGather.tok_hi) return kGemmGatherW.eligible(d, tokens) ? &kGemmGatherW : nullptr;
  if (kGemmGather.eligible(d, tokens)) return &kGemmGather;
  return kGemmGatherX.eligible(d, tokens) ? &kGemmGatherX : nullptr;
}
// the checks of the entry and its `_instance` on the token count and the layer; *k: the inner entry
static int px_validate(const VptqLayerDesc* d, int tokens, const BatchedDecode** k) {
  if (tokens < kGemmGather.tok_lo || tokens > kGemmGatherW.tok_hi)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [%d, %d]", tokens, kGemmGather.tok_lo, kGemmGatherW.tok_hi);
  *k = px_inner(*d, tokens);
  if (!*k) return fail(VPTQ_E_UNSUPPORTED, "gemm_gather_px serves the layers of gemm_gather / gemm_gatherx (1 - 16 tokens) and gemm_gatherw (17 - 48)");
  return VPTQ_OK;
}

size_t vptq_quant_gemm_gather_px_workspace_bytes(const VptqLayerDesc* d, int tokens) {
  if (validate_layer(d) != VPTQ_OK || tokens < kGemmGather.tok_lo || tokens > kGemmGatherW.tok_hi || !px_inner(*d, tokens)) return 0;
  return vptq::gemm_gather_px_workspace_bytes(*d, tokens);
}

int vptq_quant_gemm_gather_px_supported(const VptqLayerDesc* d, int tokens) {
  return validate_layer(d) == VPTQ_OK && tokens >= kGemmGather.tok_lo && tokens <= kGemmGatherW.tok_hi && px_inner(*d, tokens) ? 1 : 0;
}

int vptq_quant_gemm_gather_px(const VptqLayerDesc* d, const void* x, void* y, int tokens, int flags, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (const int rc = validate_layer(d)) return rc;
  if (!x || !y) return fail(VPTQ_E_NULL, "x / y is NULL");
  const BatchedDecode* k = nullptr;
  if (const int rc = px_validate(d, tokens, &k)) return rc;
  if ((((uintptr_t)x) & 15) != 0) return fail(k->misaligned, "gemm_gather_px (%s): x must be 16-byte aligned", k->name);
  const size_t need = vptq::gemm_gather_px_workspace_bytes(*d, tokens);
  if (need > 0) {
    if (!workspace || workspace_bytes < need) return fail(VPTQ_E_WORKSPACE, "gemm_gather_px: workspace of %zu bytes needed", need);
    if ((((uintptr_t)workspace) & 15) != 0) return fail(VPTQ_E_ALIGN, "gemm_gather_px: the workspace must be 16-byte aligned");
  }
  const hipStream_t st = (hipStream_t)stream;
  const bool out_f32 = (flags & VPTQ_GEMV_OUT_F32) != 0;
  if (need == 0) {   // no permutation: the layer's own launch, the workspace is not touched
    const hipError_t e = k->launch(*d, x, y, tokens, out_f32, st);
    return e == hipSuccess ? VPTQ_OK : hip_fail(e, k->launch_what);
  }
  hipError_t e = vptq::launch_permute_x_tokens(*d, x, workspace, tokens, st);
  if (e != hipSuccess) return hip_fail(e, "permute_x_tokens launch");
  const VptqLayerDesc plain = vptq::gemm_gather_px_plain(*d);
  e = k->launch(plain, workspace, y, tokens, out_f32, st);   // (stream order is the dependency)
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, k->launch_what);
}

int vptq_quant_gemm_gather_px_instance(const VptqLayerDesc* d, int tokens, int, char* buf, size_t bytes) {
  if (!d || !buf || bytes < 1) return fail(VPTQ_E_NULL, "desc / buf is NULL");
  buf[0] = 0;
  if (const int rc = validate_layer(d)) return rc;
  const BatchedDecode* k = nullptr;
  if (const int rc = px_validate(d, tokens, &k)) return rc;
  Text t = {buf, bytes, 0, true};
  const vptq::GemmGatherPxDecision D = vptq::gemm_gather_px_decide(*d, tokens);
  if (D.perm) t.add("permute_x_tokens g=%d tok=%d grid=%dx%d tpt=%d | ", D.g, D.tok, D.grid_x, D.grid_y, D.tpt);
  else t.add("none | ");
  k->print(t, vptq::gemm_gather_px_plain(*d), tokens);
  if (!t.fits) buf[0] = 0;
  return instance_done(t);
}

// ---- gemm_gather.hip's grouped launch (added within ABI 12): 2 - 4 sibling layers of vptq_quant_gemm_gather, 1 - 16 tokens, in ONE
// launch of gemm_gather_grouped_kernel, behind one permute launch per DISTINCT perm pointer of the members.
// What a grouped call IS, decided once for the workspace query, the launcher and the `_instance`: which xp block a member reads (-1:
// the call's x), the members as the kernel takes them (without a permutation), the first member of every distinct permutation
struct GroupedGatherPlan {
  int n_perms;             // distinct non-NULL perm pointers
  int slot[4];             // member -> xp block, -1 without a permutation
  int owner[4];            // xp block -> the first member with that permutation
  size_t block_bytes;      // one xp block (gemm_gather_px_workspace_bytes of any permuted member: the members share group_size)
  VptqLayerDesc plain[4];
};
static GroupedGatherPlan grouped_gather_decide(const VptqLayerDesc* descs, int n, int tokens) {
  GroupedGatherPlan G = {};
  for (int m = 0; m < n; ++m) {
    G.slot[m] = -1;
    G.plain[m] = vptq::gemm_gather_px_plain(descs[m]);
    if (!descs[m].perm) continue;
    for (int j = 0; j < G.n_perms && G.slot[m] < 0; ++j)
      if (descs[G.owner[j]].perm == descs[m].perm) G.slot[m] = j;
    if (G.slot[m] < 0) { G.owner[G.n_perms] = m; G.slot[m] = G.n_perms++; }
    G.block_bytes = vptq::gemm_gather_px_workspace_bytes(descs[m], tokens);
  }
  return G;
}
// the first reason the group is not served, or NULL: member and text for the message
static const char* grouped_gather_refusal(const VptqLayerDesc* descs, int n, int tokens, int* member) {
  *member = 0;
  if (n < 2 || n > 4) return "a group has 2 - 4 members";
  for (int m = 0; m < n; ++m) {
    *member = m;
    if (validate_layer(&descs[m]) != VPTQ_OK) return "not a valid layer";
    if (!kGemmGather.eligible(descs[m], tokens)) return "not a layer vptq_quant_gemm_gather serves";
    if (descs[m].dtype != descs[0].dtype) return "another dtype than member 0";
    if (descs[m].group_size != descs[0].group_size) return "another group_size than member 0";
    if (descs[m].num_res_centroids != descs[0].num_res_centroids) return "another residual codebook size than member 0";
  }
  return nullptr;
}
static int grouped_gather_validate(const VptqLayerDesc* descs, int n, int tokens) {
  if (tokens < kGemmGather.tok_lo || tokens > kGemmGather.tok_hi)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [%d, %d]", tokens, kGemmGather.tok_lo, kGemmGather.tok_hi);
  int member = 0;
  if (const char* why = grouped_gather_refusal(descs, n, tokens, &member))
    return fail(VPTQ_E_UNSUPPORTED, "gemm_gather_grouped (n = %d): member %d: %s", n, member, why);
  return VPTQ_OK;
}

int vptq_quant_gemm_gather_grouped_supported(const VptqLayerDesc* descs, int n, int tokens) {
  int member = 0;
  return descs && tokens >= kGemmGather.tok_lo && tokens <= kGemmGather.tok_hi && !grouped_gather_refusal(descs, n, tokens, &member) ? 1 : 0;
}

size_t vptq_quant_gemm_gather_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens) {
  if (!vptq_quant_gemm_gather_grouped_supported(descs, n, tokens)) return 0;
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  return G.block_bytes * (size_t)G.n_perms;
}

int vptq_quant_gemm_gather_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!descs || !x || !y) return fail(VPTQ_E_NULL, "descs / x / y is NULL");
  if (const int rc = grouped_gather_validate(descs, n, tokens)) return rc;
  for (int m = 0; m < n; ++m)
    if (!y[m]) return fail(VPTQ_E_NULL, "y[%d] is NULL", m);
  if ((((uintptr_t)x) & 15) != 0) return fail(kGemmGather.misaligned, "gemm_gather_grouped: x must be 16-byte aligned");
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  const size_t need = G.block_bytes * (size_t)G.n_perms;
  if (need > 0) {
    if (!workspace || workspace_bytes < need) return fail(VPTQ_E_WORKSPACE, "gemm_gather_grouped: workspace of %zu bytes needed", need);
    if ((((uintptr_t)workspace) & 15) != 0) return fail(VPTQ_E_ALIGN, "gemm_gather_grouped: the workspace must be 16-byte aligned");
  }
  const hipStream_t st = (hipStream_t)stream;
  for (int j = 0; j < G.n_perms; ++j) {   // one x gather per distinct permutation (block_bytes is a multiple of 256)
    const hipError_t e = vptq::launch_permute_x_tokens(descs[G.owner[j]], x, (char*)workspace + (size_t)j * G.block_bytes, tokens, st);
    if (e != hipSuccess) return hip_fail(e, "permute_x_tokens launch");
  }
  const void* xs[4] = {};
  for (int m = 0; m < n; ++m) xs[m] = G.slot[m] < 0 ? x : (const char*)workspace + (size_t)G.slot[m] * G.block_bytes;
  const hipError_t e = vptq::launch_gemm_gather_grouped(G.plain, n, xs, y, tokens, (flags & VPTQ_GEMV_OUT_F32) != 0, st);   // (stream order is the dependency)
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemm_gather_grouped launch");
}

int vptq_quant_gemm_gather_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int, char* buf, size_t bytes) {
  if (!descs || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / buf is NULL");
  buf[0] = 0;
  if (const int rc = grouped_gather_validate(descs, n, tokens)) return rc;
  Text t = {buf, bytes, 0, true};
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  if (G.n_perms > 0) {
    const vptq::GemmGatherPxDecision D = vptq::gemm_gather_px_decide(descs[G.owner[0]], tokens);
    t.add("permute_x_tokens g=%d tok=%d grid=%dx%d tpt=%d perms=%d | ", D.g, D.tok, D.grid_x, D.grid_y, D.tpt, G.n_perms);
  } else {
    t.add("none | ");
  }
  const vptq::GemmGatherGroupedDecision D = vptq::gemm_gather_grouped_decide(G.plain, n, tokens);
  t.add("gemm_gather_grouped dt=%s t=%d tok=%d n=%d groups=", dt_text(D.f16), D.T, D.tok, D.n);
  for (int m = 0; m < D.n; ++m) t.add(m ? "+%d" : "%d", D.groups[m]);
  t.add(" tiles=%d grid=%d rgs=%d", D.tiles, D.grid, D.rgs);
  if (!t.fits) buf[0] = 0;
  return instance_done(t);
}

// ---- gemm_k256.hip's grouped launch (added within ABI 12): 2 - 4 sibling layers of the canonical format, 1 - 48 tokens, in ONE launch
// of gemm_k256_grouped_kernel, behind one permute launch per DISTINCT perm pointer of the members.  The plan - which xp block a member
// reads, the members in their plain form, the first member of every distinct permutation - is the gather group's
// (grouped_gather_decide: it reads group_size and the perm pointers only).  The reference's roundings only, like vptq_quant_gemm_k256w.
constexpr int kGemmK256GroupedTokLo = 1, kGemmK256GroupedTokHi = 48;   // TB = 1 ... 3 blocks of 16 tokens
static const char* grouped_k256_refusal(const VptqLayerDesc* descs, int n, int* member) {
  *member = 0;
  if (n < 2 || n > 4) return "a group has 2 - 4 members";
  for (int m = 0; m < n; ++m) {
    *member = m;
    if (validate_layer(&descs[m]) != VPTQ_OK) return "not a valid layer";
    if (!vptq::gemm_k256_eligible(descs[m], 16, 0)) return "not a layer of the canonical format gemm_k256 serves";
    if (descs[m].dtype != descs[0].dtype) return "another dtype than member 0";
    if (descs[m].group_size != descs[0].group_size) return "another group_size than member 0";
  }
  return nullptr;
}
static int grouped_k256_validate(const VptqLayerDesc* descs, int n, int tokens) {
  if (tokens < kGemmK256GroupedTokLo || tokens > kGemmK256GroupedTokHi)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [%d, %d]", tokens, kGemmK256GroupedTokLo, kGemmK256GroupedTokHi);
  int member = 0;
  if (const char* why = grouped_k256_refusal(descs, n, &member))
    return fail(VPTQ_E_UNSUPPORTED, "gemm_k256_grouped (n = %d): member %d: %s", n, member, why);
  return VPTQ_OK;
}

int vptq_quant_gemm_k256_grouped_supported(const VptqLayerDesc* descs, int n, int tokens) {
  int member = 0;
  return descs && tokens >= kGemmK256GroupedTokLo && tokens <= kGemmK256GroupedTokHi && !grouped_k256_refusal(descs, n, &member) ? 1 : 0;
}

size_t vptq_quant_gemm_k256_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens) {
  if (!vptq_quant_gemm_k256_grouped_supported(descs, n, tokens)) return 0;
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  return G.block_bytes * (size_t)G.n_perms;
}

int vptq_quant_gemm_k256_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  // (VPTQ_GEMV_FAST_MATH / _SELECTIVE / _EXACT: the kernel has the reference's roundings only)
  if (!descs || !x || !y) return fail(VPTQ_E_NULL, "descs / x / y is NULL");
  if (const int rc = grouped_k256_validate(descs, n, tokens)) return rc;
  for (int m = 0; m < n; ++m)
    if (!y[m]) return fail(VPTQ_E_NULL, "y[%d] is NULL", m);
  if ((((uintptr_t)x) & 15) != 0) return fail(VPTQ_E_UNSUPPORTED, "gemm_k256_grouped: x must be 16-byte aligned");
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  const size_t need = G.block_bytes * (size_t)G.n_perms;
  if (need > 0) {
    if (!workspace || workspace_bytes < need) return fail(VPTQ_E_WORKSPACE, "gemm_k256_grouped: workspace of %zu bytes needed", need);
    if ((((uintptr_t)workspace) & 15) != 0) return fail(VPTQ_E_ALIGN, "gemm_k256_grouped: the workspace must be 16-byte aligned");
  }
  const hipStream_t st = (hipStream_t)stream;
  for (int j = 0; j < G.n_perms; ++j) {   // one x gather per distinct permutation (block_bytes is a multiple of 256)
    const hipError_t e = vptq::launch_permute_x_tokens(descs[G.owner[j]], x, (char*)workspace + (size_t)j * G.block_bytes, tokens, st);
    if (e != hipSuccess) return hip_fail(e, "permute_x_tokens launch");
  }
  const void* xs[4] = {};
  for (int m = 0; m < n; ++m) xs[m] = G.slot[m] < 0 ? x : (const char*)workspace + (size_t)G.slot[m] * G.block_bytes;
  const hipError_t e = vptq::launch_gemm_k256_grouped(G.plain, n, xs, y, tokens, (flags & VPTQ_GEMV_OUT_F32) != 0, st);   // (stream order is the dependency)
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemm_k256_grouped launch");
}

int vptq_quant_gemm_k256_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int, char* buf, size_t bytes) {
  if (!descs || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / buf is NULL");
  buf[0] = 0;
  if (const int rc = grouped_k256_validate(descs, n, tokens)) return rc;
  Text t = {buf, bytes, 0, true};
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  if (G.n_perms > 0) {
    const vptq::GemmGatherPxDecision D = vptq::gemm_gather_px_decide(descs[G.owner[0]], tokens);
    t.add("permute_x_tokens g=%d tok=%d grid=%dx%d tpt=%d perms=%d | ", D.g, D.tok, D.grid_x, D.grid_y, D.tpt, G.n_perms);
  } else {
    t.add("none | ");
  }
  const vptq::GemmK256GroupedDecision D = vptq::gemm_k256_grouped_decide(G.plain, n, tokens);
  t.add("gemm_k256_grouped dt=%s tok=%d tb=%d n=%d groups=", dt_text(D.f16), D.tok, D.tb, D.n);
  for (int m = 0; m < D.n; ++m) t.add(m ? "+%d" : "%d", D.groups[m]);
  t.add(" grid=%d rgs=%d passes=", D.grid, D.rgs);
  if (D.tb > 1) {
    t.add("1x%d", D.tb);
  } else {
    bool any = false;
    for (int p = 4; p >= 1; p >>= 1)
      if (D.passes & p) { t.add(any ? "+%d" : "%d", p); any = true; }
  }
  if (!t.fits) buf[0] = 0;
  return instance_done(t);
}

// ---- gemm_gatherw_grouped.hip (added within ABI 12): 2 - 4 sibling layers of vptq_quant_gemm_gatherw, 17 - 48 tokens, in ONE launch of
// gemm_gatherw_grouped_kernel, behind one permute launch per DISTINCT perm pointer of the members.  The plan is the gather group's
// (grouped_gather_decide), the checks are its checks with gemm_gatherw's window and eligibility.
static const char* grouped_gatherw_refusal(const VptqLayerDesc* descs, int n, int tokens, int* member) {
  *member = 0;
  if (n < 2 || n > 4) return "a group has 2 - 4 members";
  for (int m = 0; m < n; ++m) {
    *member = m;
    if (validate_layer(&descs[m]) != VPTQ_OK) return "not a valid layer";
    if (!kGemmGatherW.eligible(descs[m], tokens)) return "not a layer vptq_quant_gemm_gatherw serves";
    if (descs[m].dtype != descs[0].dtype) return "another dtype than member 0";
    if (descs[m].group_size != descs[0].group_size) return "another group_size than member 0";
    if (descs[m].num_res_centroids != descs[0].num_res_centroids) return "another residual codebook size than member 0";
  }
  return nullptr;
}
static int grouped_gatherw_validate(const VptqLayerDesc* descs, int n, int tokens) {
  if (tokens < kGemmGatherW.tok_lo || tokens > kGemmGatherW.tok_hi)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [%d, %d]", tokens, kGemmGatherW.tok_lo, kGemmGatherW.tok_hi);
  int member = 0;
  if (const char* why = grouped_gatherw_refusal(descs, n, tokens, &member))
    return fail(VPTQ_E_UNSUPPORTED, "gemm_gatherw_grouped (n = %d): member %d: %s", n, member, why);
  return VPTQ_OK;
}

int vptq_quant_gemm_gatherw_grouped_supported(const VptqLayerDesc* descs, int n, int tokens) {
  int member = 0;
  return descs && tokens >= kGemmGatherW.tok_lo && tokens <= kGemmGatherW.tok_hi && !grouped_gatherw_refusal(descs, n, tokens, &member) ? 1 : 0;
}

size_t vptq_quant_gemm_gatherw_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens) {
  if (!vptq_quant_gemm_gatherw_grouped_supported(descs, n, tokens)) return 0;
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  return G.block_bytes * (size_t)G.n_perms;
}

int vptq_quant_gemm_gatherw_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  // (VPTQ_GEMV_FAST_MATH / _SELECTIVE / _EXACT: the kernel has the reference's roundings only)
  if (!descs || !x || !y) return fail(VPTQ_E_NULL, "descs / x / y is NULL");
  if (const int rc = grouped_gatherw_validate(descs, n, tokens)) return rc;
  for (int m = 0; m < n; ++m)
    if (!y[m]) return fail(VPTQ_E_NULL, "y[%d] is NULL", m);
  if ((((uintptr_t)x) & 15) != 0) return fail(kGemmGatherW.misaligned, "gemm_gatherw_grouped: x must be 16-byte aligned");
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  const size_t need = G.block_bytes * (size_t)G.n_perms;
  if (need > 0) {
    if (!workspace || workspace_bytes < need) return fail(VPTQ_E_WORKSPACE, "gemm_gatherw_grouped: workspace of %zu bytes needed", need);
    if ((((uintptr_t)workspace) & 15) != 0) return fail(VPTQ_E_ALIGN, "gemm_gatherw_grouped: the workspace must be 16-byte aligned");
  }
  const hipStream_t st = (hipStream_t)stream;
  for (int j = 0; j < G.n_perms; ++j) {   // one x gather per distinct permutation (block_bytes is a multiple of 256)
    const hipError_t e = vptq::launch_permute_x_tokens(descs[G.owner[j]], x, (char*)workspace + (size_t)j * G.block_bytes, tokens, st);
    if (e != hipSuccess) return hip_fail(e, "permute_x_tokens launch");
  }
  const void* xs[4] = {};
  for (int m = 0; m < n; ++m) xs[m] = G.slot[m] < 0 ? x : (const char*)workspace + (size_t)G.slot[m] * G.block_bytes;
  const hipError_t e = vptq::launch_gemm_gatherw_grouped(G.plain, n, xs, y, tokens, (flags & VPTQ_GEMV_OUT_F32) != 0, st);   // (stream order is the dependency)
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemm_gatherw_grouped launch");
}

int vptq_quant_gemm_gatherw_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int, char* buf, size_t bytes) {
  if (!descs || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / buf is NULL");
  buf[0] = 0;
  if (const int rc = grouped_gatherw_validate(descs, n, tokens)) return rc;
  Text t = {buf, bytes, 0, true};
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  if (G.n_perms > 0) {
    const vptq::GemmGatherPxDecision D = vptq::gemm_gather_px_decide(descs[G.owner[0]], tokens);
    t.add("permute_x_tokens g=%d tok=%d grid=%dx%d tpt=%d perms=%d | ", D.g, D.tok, D.grid_x, D.grid_y, D.tpt, G.n_perms);
  } else {
    t.add("none | ");
  }
  const vptq::GemmGatherWGroupedDecision D = vptq::gemm_gatherw_grouped_decide(G.plain, n, tokens);
  t.add("gemm_gatherw_grouped dt=%s t=%d tok=%d tb=%d n=%d groups=", dt_text(D.f16), D.T, D.tok, D.tb, D.n);
  for (int m = 0; m < D.n; ++m) t.add(m ? "+%d" : "%d", D.groups[m]);
  t.add(" tiles=%d grid=%d rgs=%d", D.tiles, D.grid, D.rgs);
  if (!t.fits) buf[0] = 0;
  return instance_done(t);
}

// ---- gemm_gatherx_grouped.hip (added within ABI 12): 2 - 4 sibling layers of vptq_quant_gemm_gatherx, 1 - 16 tokens, in ONE launch of
// gemm_gatherx_grouped_kernel, behind one permute launch per DISTINCT perm pointer of the members.  The plan is the gather group's
// (grouped_gather_decide), the checks are its checks with gemm_gatherx's eligibility and the whole format shared.
static const char* grouped_gatherx_refusal(const VptqLayerDesc* descs, int n, int tokens, int* member) {
  *member = 0;
  if (n < 2 || n > 4) return "a group has 2 - 4 members";
  for (int m = 0; m < n; ++m) {
    *member = m;
    if (validate_layer(&descs[m]) != VPTQ_OK) return "not a valid layer";
    if (!kGemmGatherX.eligible(descs[m], tokens)) return "not a layer vptq_quant_gemm_gatherx serves";
    if (descs[m].dtype != descs[0].dtype) return "another dtype than member 0";
    if (descs[m].group_size != descs[0].group_size) return "another group_size than member 0";
    if (descs[m].vector_len != descs[0].vector_len) return "another vector length than member 0";
    if (descs[m].num_centroids != descs[0].num_centroids) return "another main codebook size than member 0";
    if (descs[m].num_res_centroids != descs[0].num_res_centroids) return "another residual codebook size than member 0";
  }
  return nullptr;
}
static int grouped_gatherx_validate(const VptqLayerDesc* descs, int n, int tokens) {
  if (tokens < kGemmGatherX.tok_lo || tokens > kGemmGatherX.tok_hi)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [%d, %d]", tokens, kGemmGatherX.tok_lo, kGemmGatherX.tok_hi);
  int member = 0;
  if (const char* why = grouped_gatherx_refusal(descs, n, tokens, &member))
    return fail(VPTQ_E_UNSUPPORTED, "gemm_gatherx_grouped (n = %d): member %d: %s", n, member, why);
  return VPTQ_OK;
}

int vptq_quant_gemm_gatherx_grouped_supported(const VptqLayerDesc* descs, int n, int tokens) {
  int member = 0;
  return descs && tokens >= kGemmGatherX.tok_lo && tokens <= kGemmGatherX.tok_hi && !grouped_gatherx_refusal(descs, n, tokens, &member) ? 1 : 0;
}

size_t vptq_quant_gemm_gatherx_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens) {
  if (!vptq_quant_gemm_gatherx_grouped_supported(descs, n, tokens)) return 0;
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  return G.block_bytes * (size_t)G.n_perms;
}

int vptq_quant_gemm_gatherx_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  // (VPTQ_GEMV_FAST_MATH / _SELECTIVE / _EXACT: the kernel has the reference's roundings only)
  if (!descs || !x || !y) return fail(VPTQ_E_NULL, "descs / x / y is NULL");
  if (const int rc = grouped_gatherx_validate(descs, n, tokens)) return rc;
  for (int m = 0; m < n; ++m)
    if (!y[m]) return fail(VPTQ_E_NULL, "y[%d] is NULL", m);
  if ((((uintptr_t)x) & 15) != 0) return fail(kGemmGatherX.misaligned, "gemm_gatherx_grouped: x must be 16-byte aligned");
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  const size_t need = G.block_bytes * (size_t)G.n_perms;
  if (need > 0) {
    if (!workspace || workspace_bytes < need) return fail(VPTQ_E_WORKSPACE, "gemm_gatherx_grouped: workspace of %zu bytes needed", need);
    if ((((uintptr_t)workspace) & 15) != 0) return fail(VPTQ_E_ALIGN, "gemm_gatherx_grouped: the workspace must be 16-byte aligned");
  }
  const hipStream_t st = (hipStream_t)stream;
  for (int j = 0; j < G.n_perms; ++j) {   // one x gather per distinct permutation (block_bytes is a multiple of 256)
    const hipError_t e = vptq::launch_permute_x_tokens(descs[G.owner[j]], x, (char*)workspace + (size_t)j * G.block_bytes, tokens, st);
    if (e != hipSuccess) return hip_fail(e, "permute_x_tokens launch");
  }
  const void* xs[4] = {};
  for (int m = 0; m < n; ++m) xs[m] = G.slot[m] < 0 ? x : (const char*)workspace + (size_t)G.slot[m] * G.block_bytes;
  const hipError_t e = vptq::launch_gemm_gatherx_grouped(G.plain, n, xs, y, tokens, (flags & VPTQ_GEMV_OUT_F32) != 0, st);   // (stream order is the dependency)
  return e == hipSuccess ? VPTQ_OK : hip_fail(e, "gemm_gatherx_grouped launch");
}

int vptq_quant_gemm_gatherx_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int, char* buf, size_t bytes) {
  if (!descs || !buf || bytes < 1) return fail(VPTQ_E_NULL, "descs / buf is NULL");
  buf[0] = 0;
  if (const int rc = grouped_gatherx_validate(descs, n, tokens)) return rc;
  Text t = {buf, bytes, 0, true};
  const GroupedGatherPlan G = grouped_gather_decide(descs, n, tokens);
  if (G.n_perms > 0) {
    const vptq::GemmGatherPxDecision D = vptq::gemm_gather_px_decide(descs[G.owner[0]], tokens);
    t.add("permute_x_tokens g=%d tok=%d grid=%dx%d tpt=%d perms=%d | ", D.g, D.tok, D.grid_x, D.grid_y, D.tpt, G.n_perms);
  } else {
    t.add("none | ");
  }
  const vptq::GemmGatherXGroupedDecision D = vptq::gemm_gatherx_grouped_decide(G.plain, n, tokens);
  t.add("gemm_gatherx_grouped dt=%s v=%d ib=%d rb=%d res=%s tok=%d n=%d groups=", dt_text(D.f16), D.v, D.ib, D.rb,
        D.res == 0 ? "none" : D.res == 1 ? "lds" : "l2", D.tok, D.n);
  for (int m = 0; m < D.n; ++m) t.add(m ? "+%d" : "%d", D.groups[m]);
  t.add(" tiles=%d wgcu=%d grid=%d rgs=%d", D.tiles, D.wgcu, D.grid, D.rgs);
  if (!t.fits) buf[0] = 0;
  return instance_done(t);
}

// the checks of vptq_dequant and vptq_dequant_instance
static int validate_dequant(const VptqLayerDesc* d, const void* W) {
  int rc = validate_layer(d);
  if (rc) return rc;
  if (!W) return fail(VPTQ_E_NULL, "W is NULL");
  if (d->perm && !d->inv_perm)
    return fail(VPTQ_E_NULL, "dequant needs inv_perm = argsort(perm) when perm is set");
  return VPTQ_OK;
}

int vptq_dequant(const VptqLayerDesc* d, void* W, void* stream) {
  if (const int rc = validate_dequant(d, W)) return rc;
  hipError_t e = vptq::launch_dequant(*d, W, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "dequant launch");
  return VPTQ_OK;
}

int vptq_dequant_instance(const VptqLayerDesc* d, const void* W, char* buf, size_t bytes) {
  if (!d || !buf || bytes < 1) return fail(VPTQ_E_NULL, "desc / buf is NULL");
  buf[0] = 0;
  if (const int rc = validate_dequant(d, W)) return rc;
  if (vptq::dequant_instance(*d, W, buf, bytes)) {
    buf[0] = 0;
    return fail(VPTQ_E_WORKSPACE, "instance: buffer of %zu bytes too small", bytes);
  }
  return VPTQ_OK;
}

// the checks of vptq_quant_gemv_v2 and vptq_quant_gemv_v2_instance on the descriptor and the token count
static int validate_v2(const VptqV2Desc* d, int tokens) {
  if (!d) return fail(VPTQ_E_NULL, "desc is NULL");
  if (!d->indices || !d->centroids) return fail(VPTQ_E_NULL, "indices / centroids is NULL");
  if (d->dtype != VPTQ_DTYPE_F16 && d->dtype != VPTQ_DTYPE_BF16)
    return fail(VPTQ_E_UNSUPPORTED, "dtype %d", d->dtype);
  // the reference instantiates v in {4, 8, 16} (csrc/dispatch_macros.h:12-89)
  if (!(d->vector_len == 4 || d->vector_len == 8 || d->vector_len == 16))
    return fail(VPTQ_E_UNSUPPORTED, "un-supported vector_len %d (v2: 4, 8, 16)", d->vector_len);
  if (d->in_features <= 0 || d->out_features <= 0 || d->out_features % d->vector_len)
    return fail(VPTQ_E_SHAPE, "out_features must be a positive multiple of vector_len");
  if (d->num_centroids < 1 || d->num_centroids > 65536)
    return fail(VPTQ_E_SHAPE, "num_centroids %d", d->num_centroids);
  if (d->num_res_centroids > 0) {
    if (!d->res_indices || !d->res_centroids)
      return fail(VPTQ_E_NULL, "residual tensors required when num_res_centroids > 0");
    if (d->res_index_bytes != 1 && d->res_index_bytes != 2)
      return fail(VPTQ_E_SHAPE, "res_index_bytes must be 1 or 2");
    if (d->res_index_bytes == 1 && d->num_res_centroids > 256)
      return fail(VPTQ_E_SHAPE, "uint8 residual ids need num_res_centroids <= 256");
  }
  // reference: "tokens < 16" (vptq/ops/quant_gemm.py:338, csrc/quant_gemv_v2.cu:58)
  if (tokens < 1 || tokens >= 16)
    return fail(VPTQ_E_TOKENS, "tokens %d outside [1, 15]", tokens);
  return VPTQ_OK;
}

// ONE decision for vptq_quant_gemv_v2 and vptq_quant_gemv_v2_instance: codebooks LDS-resident (what the reference's kernel does,
// quant_gemv_v2.cuh:85-94), else gathered through L1 / L2 (x = NULL: assumed aligned)
static bool v2_takes_lds(const VptqV2Desc& d, const void* x, int tokens, int flags) {
  return !(flags & VPTQ_GEMV_FORCE_GENERIC) && vptq::gemv_lds_v2_eligible(d, tokens > 4 ? 4 : tokens) && (((uintptr_t)x) & 15) == 0;
}

int vptq_quant_gemv_v2(const VptqV2Desc* d, const void* x, void* y, int tokens, int flags,
                       void* stream) {
  const bool out_f32 = (flags & VPTQ_GEMV_OUT_F32) != 0;
  if (!d) return fail(VPTQ_E_NULL, "desc is NULL");
  if (!d->indices || !d->centroids || !x || !y)
    return fail(VPTQ_E_NULL, "indices / centroids / x / y is NULL");
  if (const int rc = validate_v2(d, tokens)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t es = 2;
  if (v2_takes_lds(*d, x, tokens, flags)) {
    const int step = vptq::gemv_lds_max_chunk(d->dtype);
    const int lflags = lds_launch_flags(tokens, flags);
    for (int t0 = 0; t0 < tokens; t0 += step) {
      const int m = tokens - t0 < step ? tokens - t0 : step;
      hipError_t e = vptq::launch_gemv_lds_v2(*d, (const char*)x + (size_t)t0 * d->in_features * es,
                                              (char*)y + (size_t)t0 * d->out_features * (out_f32 ? 4 : es),
                                              m, out_f32, lflags, st);
      if (e != hipSuccess) return hip_fail(e, "gemv_lds (v2) launch");
    }
    return VPTQ_OK;
  }
  for (int t0 = 0; t0 < tokens; t0 += 8) {
    const int m = tokens - t0 < 8 ? tokens - t0 : 8;
    hipError_t e = vptq::launch_gemv_v2(*d, (const char*)x + (size_t)t0 * d->in_features * es,
                                        (char*)y + (size_t)t0 * d->out_features * (out_f32 ? 4 : es), m,
                                        out_f32, st);
    if (e != hipSuccess) return hip_fail(e, "gemv_v2 launch");
  }
  return VPTQ_OK;
}

int vptq_quant_gemv_v2_instance(const VptqV2Desc* d, int tokens, int flags, char* buf, size_t bytes) {
  if (!d || !buf || bytes < 1) return fail(VPTQ_E_NULL, "desc / buf is NULL");
  buf[0] = 0;
  if (const int rc = validate_v2(d, tokens)) return rc;
  Text t = {buf, bytes, 0, true};
  if (v2_takes_lds(*d, nullptr, tokens, flags)) {
    const int step = vptq::gemv_lds_max_chunk(d->dtype);
    add_lds(t, vptq::gemv_lds_v2_decide(*d, tokens > step ? step : tokens, lds_launch_flags(tokens, flags)));
  } else {
    const vptq::V2Decision D = vptq::gemv_v2_decide(*d, tokens > 8 ? 8 : tokens);
    t.add("gemv_v2 dt=%s v=%d tok=%d", dt_text(D.f16), D.v, D.tok);
  }
  return instance_done(t);
}

}  // extern "C"
