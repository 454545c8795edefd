/*
 * vptq_hip.h — C ABI of libvptq_hip.so: the MI355X (gfx950) replacement for the
 * native extension behind microsoft/VPTQ's `vptq.ops` hot path.
 *
 * Drop-in boundary.  The reference binds three C++/CUDA entry points through
 * pybind11 (csrc/ops.cc:44-55); each function below replaces one of them:
 *
 *   vptq_quant_gemv     <- `quant_gemv`    = wquant_act16_gemv     csrc/ops.cc:20-30,
 *                                            csrc/quant_gemv.cu:241-294
 *   vptq_dequant        <- `dequant`                                csrc/ops.cc:9-18,
 *                                            csrc/dequant.cu:227-287
 *   vptq_quant_gemv_v2  <- `quant_gemv_v2`                          csrc/ops.cc:32-38,
 *                                            csrc/quant_gemv_v2.cu:25-180
 *
 * Plain C: raw device pointers + sizes, no torch / pybind / C++ types.
 *
 * Ownership ... the caller owns every buffer (inputs, outputs, workspace); the
 *               library allocates nothing and keeps no per-call state.  The
 *               reference ops allocate their own output (quant_gemv.cu:206).
 * Streams ..... every launch goes to the hipStream_t passed as `stream`
 *               (NULL = the default stream).  Asynchronous, no host sync, no
 *               host read of device data => hipGraph-capturable.  The reference
 *               uses at::cuda::getCurrentCUDAStream() (quant_gemv.cu:180).
 * Errors ...... return 0 on success; < 0 = VPTQ_E_* validation error (nothing
 *               launched); > 0 = hipError_t from the launch.  A message is kept
 *               per thread in vptq_last_error().  The reference throws
 *               c10::Error via TORCH_CHECK (csrc/util/common.h:11-19).
 * Threading ... re-entrant; no globals besides one-time kernel attribute setup.
 * Alignment ... every pointer is aligned to its ELEMENT at least (2 bytes for fp16 / bf16 / uint16, 4 for int32 / float32, 1 for
 *               uint8); `indices`, `centroids` and `res_centroids` of a VptqLayerDesc to 4 bytes (VPTQ_E_ALIGN).  What an entry or
 *               one of its kernels needs beyond that is stated at the entry ("Alignment:").  Where a kernel's rule is not met the
 *               call does not fail: it takes the next kernel that can read the operands (the order is given there), down to one
 *               that takes element alignment - same results within that kernel's arithmetic.  No kernel reads or writes outside
 *               the tensors' extents as declared here, whatever surrounds them, and results do not depend on the alignment beyond
 *               the rule of the kernel that runs (tests/test_operand_placement_gpu.py holds every entry to both).
 */
#ifndef VPTQ_HIP_H
#define VPTQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPTQ_ABI_VERSION 12

#if defined(__GNUC__)
#define VPTQ_API __attribute__((visibility("default")))
#else
#define VPTQ_API
#endif

/* element type of activations / codebooks / scales / outputs */
enum { VPTQ_DTYPE_F16 = 0, VPTQ_DTYPE_BF16 = 1 };

/* error codes (negative) */
enum {
  VPTQ_OK = 0,
  VPTQ_E_NULL = -1,        /* required pointer is NULL            */
  VPTQ_E_SHAPE = -2,       /* inconsistent shapes / sizes         */
  VPTQ_E_UNSUPPORTED = -3, /* valid but no kernel for this combo  */
  VPTQ_E_ALIGN = -4,       /* pointer not aligned as required     */
  VPTQ_E_TOKENS = -5,      /* tokens outside [1, VPTQ_GEMV_MAX_TOKENS] */
  VPTQ_E_WORKSPACE = -6    /* workspace too small                 */
};

/* flags for vptq_quant_gemv / vptq_quant_gemv_v2 */
enum {
  /* Default arithmetic of the fused GEMV (ABI >= 3), where a kernel implements it (the
   * canonical v=8 / 256+256 format: fp16 with 1-2 tokens on any launch and with 3-4 tokens on
   * launches of >= 576 vector-rows, bf16 with 1-4 tokens on launches of >= 128 vector-rows;
   * the LDS-resident formats v=8, 256 < k <= 8192, kr <= 512: one-token calls on layers of
   * >= 1024 vector-rows, bf16 always):
   * the folded form
   *   y = sum_g (c + r) * (scale_g * x_g) + sum_g bias_g * x_g + bias,   fp32 accumulate,
   * inside the parity bar of <= 1e-3 (max-normalised) against the reference CPU path, but
   * its weights are not rounded to 16 bits step by step.  FAST_MATH asks for it explicitly
   * (what ABI 2 required); it is accepted and changes nothing. */
  VPTQ_GEMV_FAST_MATH = 1 << 0,
  /* force the generic kernel (testing / A-B) */
  VPTQ_GEMV_FORCE_GENERIC = 1 << 1,
  /* Reproduce the reference CPU path's roundings: every weight is rebuilt as
   * r16(r16(r16(c+r)*scale)+bias) in the 16-bit type (bit-identical to vptq_dequant and to
   * the reference's torch path), then x*w is accumulated in fp32 and rounded once.  All
   * other kernels (other formats, small layers with 3+ tokens or bf16) always work this way;
   * bf16 layers of the LDS-resident formats are routed to the L2-gather kernel for it.
   * Held weight by weight (tests/test_weight_bits_gpu.py: one-hot activations read W back through every kernel and compare it
   * with vptq_dequant's bits - signed zeros apart - on a table of subnormals, ties and underflowing products).  What a kernel may
   * read differently, all of it bf16: the dot-instruction kernels (gemv_k256, gemm_k256, gemm_k256w, gemm_gather, gemm_gatherx)
   * may flush a weight in the bf16 subnormal range to zero (on an MI355X they do not); the one-pass sliced kernel (gemv_sliced)
   * reads a weight below 2^-21 as zero - its accumulator word counts in units of 2^-28.  fp16 subnormal weights and activations
   * are exact in every kernel, the 16-bit MFMA operands of gemv_k256m, gemv_k256c, gemm_k256 and gemv_sliced_tok included.
   * Weights that are not finite (finite codebooks whose sum or product overflows the 16-bit type): the outputs of a row that
   * holds one are not finite and every other output is unaffected, but where the reference has an infinity a kernel may have
   * NaN - wherever it pairs the rebuilt weight with a ZERO (0 x inf): the one-hot MFMA operands of gemv_k256m / gemv_k256c, the
   * zero column of gemv_sliced_tok (lanes without a token, elements of another column phase), the other half of a bf16 dot
   * instruction's pair, the accumulator word of gemv_sliced (which holds no infinity), and the tail lanes of gemv_k256 /
   * gemv_gather, which read the last chunk of 8 columns again against zero activations.  The padding elements of the sliced
   * layouts rebuild entry 0 of a slice plus residual entry 0 against a scale of zero: a layer in which THAT sum overflows has
   * NaN in every output of the rows that carry padding. */
  VPTQ_GEMV_EXACT = 1 << 2,
  /* canonical format only: pick the persistent MFMA kernel wherever it is instantiated /
   * never pick it (testing / A-B; the default chooses by launch size) */
  VPTQ_GEMV_FORCE_MFMA = 1 << 3,
  VPTQ_GEMV_FORCE_VALU = 1 << 4,
  /* y is float32 [tokens, O]: the fp32 sums (output bias included when desc->bias is set) are
   * stored un-rounded.  For callers that combine several launches before the one rounding of
   * the reference's F.linear - the partial outputs of a row-parallel (input-column) shard,
   * summed by an all-reduce.  Every kernel honours it (ABI >= 4).
   * Range of the sliced routes (vptq_quant_gemv_sliced*, whose arrivals - slices x tables x window / column parts - meet in a
   * fixed-point accumulator word of 2^-30 units for fp16, 2^-28 for bf16): each arrival's partial sum must stay below
   * 2^19 / arrivals (fp16) or 2^21 / arrivals (bf16) - 8 slices: 65536 / 262144; at worst (127 arrivals) ~4.1e3 / ~1.65e4 - so
   * that the total fits the word; an output with a partial sum beyond that is NaN (even where the total itself would fit), never a
   * wrong finite value.  Every other kernel sums in fp32 (range of fp32). */
  VPTQ_GEMV_OUT_F32 = 1 << 5,
  /* vptq_quant_gemv_chain only: layer i + 1 reads what layer i wrote (x[i + 1] aliases y[i]);
   * without it the layers of a chain must be independent of each other (ABI >= 6) */
  VPTQ_GEMV_CHAIN_DEPENDENT = 1 << 6,
  /* take the one-pass batched-decode kernel (gemm_k256t: canonical format, 1-16 tokens per launch,
   * needs the workspace) wherever it is eligible, not only where it is the fastest (bf16, 5+
   * tokens): testing / A-B */
  VPTQ_GEMV_FORCE_BATCHED = 1 << 7,
  /* vptq_quant_gemv_sliced_grouped (ABI >= 9): the n descriptors are COLUMN PARTS of one layer - see there */
  VPTQ_GEMV_COLUMN_PARTS = 1 << 8,
  /* SELECTIVE roundings (ABI >= 10): the folded form, with the reference's three roundings per weight (VPTQ_GEMV_EXACT's
   * arithmetic) on the activation columns that dominate the token - |f16(scale_g x_g)| >= 6 x the rms of f16(scale x) over the
   * layer's columns.  The folded form's distance to the reference is a sum of per-column rounding errors that average out over
   * thousands of columns when the activations are dense and do not when a handful of channels carry the token (massive
   * activations): the blocks of 128 columns that hold such a column are rebuilt bit-exactly, the rest stays folded.  The blocks
   * (and the 512-column windows below) are those of the STORED column order - column c of the quantised matrix, which multiplies
   * input feature perm[c]: the kernels stage x[perm] and look for the hot columns there; without a permutation the two orders
   * are one.  The rule above is the chain launch's.  The persistent MFMA kernel of one-layer / grouped launches takes one
   * threshold per wave, 6 x the rms over the columns that wave stages, columns past the last one counted as zeros: up to 8192
   * columns that is window w = columns [512 w, 512 w + 512); from 8193 columns on (5 - 7 sweeps) the kernel stages in two phases
   * of 8192 columns and a wave's threshold runs over its 512 columns of BOTH - windows w and w + 16, 1024 columns - so a window
   * whose partner lies past the last column has a threshold lower by sqrt(2) and turns hot sooner (never later: more exact
   * blocks, not fewer).  Kernels
   * that implement it (fp16 and bf16): the persistent chain launch (independent layers; needs the workspace
   * vptq_quant_gemv_chain_workspace_bytes_for(descs, n, flags) asks for - 16 bytes per layer + 4 per output: thresholds and
   * the hot blocks' exact products) and the persistent MFMA kernel of one-layer / grouped launches (1 token, up to
   * 14336 columns, at most 16 row groups per workgroup; thresholds over the 512 / 1024 columns a wave stages, as above, then the 16 most
   * dominant blocks);
   * every other kernel / layer / token count takes VPTQ_GEMV_EXACT instead (always at least as close to the reference).
   * With VPTQ_GEMV_EXACT set as well, EXACT wins.  Not bit-equivalent (55 - 65 % of the outputs bit-identical); counted on
   * checkpoint-like layers: 2 of 12 300 above the 1e-3 bar at 1.00e-3 / 1.09e-3 through the chain launch (folded form: 30
   * of 4100; the reference's roundings: 0 by construction) - an opt-in, not the default. */
  VPTQ_GEMV_SELECTIVE = 1 << 9
};

/* most tokens vptq_quant_gemv accepts (fp16 layers of the canonical format; every other layer:
 * VPTQ_GEMV_MAX_TOKENS_ANY); whether the fused path is also the FASTER one for a layer at a
 * token count is what vptq_quant_gemv_max_tokens() answers */
#define VPTQ_GEMV_MAX_TOKENS 64
#define VPTQ_GEMV_MAX_TOKENS_ANY 16

/*
 * One VQuantLinear layer in the reference's on-disk tensor formats
 * (vptq/layers/vqlinear.py:97-240).  All pointers are DEVICE pointers; nullable
 * ones are marked.  I = outlier_size + num_codebooks * group_size.
 *
 *   Wq[n*v+t, S + cb*G + g] = centroids[cb, idx, t] + res_centroids[cb, ridx, t]
 *   Wq[m*ov+t, g]           = outlier_centroids[0, outlier_indices[0,m,g], t]   (g < S)
 *   W[o, j] = Wq[o, inv_perm[j]] * weight_scale[j] + weight_bias[j]
 *   y[., o] = sum_j x[., j] * W[o, j] + bias[o]
 *
 * indices: int32 [C, N, row_words]; each (cb, n) row is a little-endian bit
 * stream, element g = bits [g*T, (g+1)*T), T = index_bits + res_bits,
 * value = (ridx << index_bits) | idx   (vptq/utils/pack.py:26-67).
 */
typedef struct VptqLayerDesc {
  int32_t in_features;           /* I */
  int32_t out_features;          /* O */
  int32_t vector_len;            /* v: even, 2..16 */
  int32_t num_codebooks;         /* C = group_num */
  int32_t group_size;            /* G */
  int32_t num_centroids;         /* k (power of two, <= 65536) */
  int32_t num_res_centroids;     /* kr; 0 = no residual codebook */
  int32_t index_bits;            /* log2 k  */
  int32_t res_bits;              /* log2 kr */
  int32_t row_words;             /* ceil(G*T/32) */
  int32_t num_indices;           /* N = ceil(O / v) */
  int32_t outlier_size;          /* S; 0 = no outliers */
  int32_t outlier_vector_len;    /* ov */
  int32_t num_outlier_centroids; /* ko */
  int32_t num_outlier_indices;   /* M = ceil(O / ov) */
  int32_t dtype;                 /* VPTQ_DTYPE_* */

  const int32_t* indices;          /* [C, N, row_words]                        */
  const void* centroids;           /* [C, k, v]                                 */
  const void* res_centroids;       /* [C, kr, v]            NULL iff kr == 0    */
  const uint16_t* outlier_indices; /* [1, M, S]             NULL iff S == 0     */
  const void* outlier_centroids;   /* [1, ko, ov]           NULL iff S == 0     */
  const uint16_t* perm;            /* [I] uint16            NULL = identity     */
  const uint16_t* inv_perm;        /* [I] argsort(perm)     needed by dequant when perm != NULL */
  const void* weight_scale;        /* [I]   NULL (with weight_bias) = no norm   */
  const void* weight_bias;         /* [I]                                       */
  const void* bias;                /* [O]                   NULL = none         */
  /* Optional derived state (all nullable; results never depend on them): */
  const void* scale_permuted;      /* [I] weight_scale[perm[c]]: lets the GEMV read scale in  */
  const void* bias_permuted;       /* [I] weight_bias[perm[c]]   column order (perm != NULL)  */
  const void* prefetch;            /* read-only range the GEMV may touch to warm L2 / Infinity  */
  int64_t prefetch_bytes;          /* Cache for the NEXT launch (e.g. the next layer's indices) */
} VptqLayerDesc;

/*
 * v2 wire format (tests/test_quant_gemv.py:49-109, csrc/quant_gemv_v2.cu:25-180):
 * UNPACKED indices laid out [N][I]; one codebook; residual ids uint8 or uint16.
 *   W^T[i, n*v+t] = centroids[ids[n*I+i], t] + res_centroids[rids[n*I+i], t]
 *   W^T = scale[i] * W^T + sbias[i];  y = x @ W^T + bias
 */
typedef struct VptqV2Desc {
  int32_t in_features;
  int32_t out_features;
  int32_t vector_len;
  int32_t num_centroids;
  int32_t num_res_centroids; /* 0 = none */
  int32_t res_index_bytes;   /* 1 (uint8) or 2 (uint16) */
  int32_t dtype;
  int32_t reserved;
  const uint16_t* indices;     /* [N * I] */
  const void* centroids;       /* [1, k, v] */
  const void* res_indices;     /* [N * I] uint8/uint16, NULL iff kr == 0 */
  const void* res_centroids;   /* [1, kr, v] */
  const void* scale_weights;   /* [I] nullable */
  const void* scale_bias;      /* [I] nullable */
  const void* bias;            /* [O] nullable */
} VptqV2Desc;

VPTQ_API int vptq_abi_version(void);

/* thread-local message for the last non-zero return on this thread */
VPTQ_API const char* vptq_last_error(void);

/*
 * y[tokens, O] = x[tokens, I] @ W^T + bias, fused dequant, tokens in
 * [1, VPTQ_GEMV_MAX_TOKENS].  x, y dense row-major in desc->dtype.
 * workspace: optional, never required.  vptq_quant_gemv_workspace_bytes() tells how many bytes
 * (16-byte aligned, device memory, contents don't matter) let the call take its fastest kernel: for
 * 2+ tokens of the canonical 256 + 256 format that is gemm_k256t_kernel (up to 16 tokens in ONE pass
 * over the indices, fp16 and bf16; its pre-pass writes the operand-ordered activations there).
 * With NULL / fewer bytes the call uses the kernels that need none (same results within the
 * parity bar).  Launches of one call and calls on one stream may share a workspace.
 * Alignment: the entry takes element-aligned x, y (2 bytes; float32 y: 4), weight_scale, weight_bias, bias, perm, outlier_indices and
 * outlier_centroids and 4-byte indices / codebooks - served by gemv_generic.  The kernels in front of it, in the order they are tried,
 * and what each needs (a rule that is not met hands the call to the next one; y and bias are element-aligned for all of them):
 *   gemm_k256t, gemm_k256, gemv_k256, gemv_k256m   indices, centroids, res_centroids, weight_scale, weight_bias, perm (and
 *                 scale_permuted, bias_permuted) 16 bytes; x 16 bytes (gemm_k256t: 2); the workspace 16 bytes
 *   gemv_gather   indices, centroids, res_centroids 16 bytes; weight_scale, weight_bias, perm (scale_permuted, bias_permuted), x 4
 *   gemv_lds, gemv_lds_mfma   centroids, res_centroids, weight_scale, weight_bias, perm (scale_permuted, bias_permuted), x 16 bytes
 *   gemv_gatherx  centroids, res_centroids, outlier_centroids: the largest power of two that divides an entry (2 v bytes), at most 16;
 *                 indices, weight_scale, weight_bias, perm (scale_permuted, bias_permuted), x 4 bytes; outlier_indices 2
 * vptq_quant_gemv_instance / _kernel_name see the descriptor only: they answer for an x that meets the rule.
 */
VPTQ_API int vptq_quant_gemv(const VptqLayerDesc* desc, const void* x, void* y, int tokens,
                    int flags, void* workspace, size_t workspace_bytes, void* stream);

VPTQ_API size_t vptq_quant_gemv_workspace_bytes(const VptqLayerDesc* desc, int tokens, int flags);

/*
 * Largest token count for which vptq_quant_gemv is the path to take for this layer; above it
 * vptq_dequant + a dense GEMM is faster (the reference switches at 3 for every format,
 * vptq/ops/quant_gemm.py:213).  48 for fp16 layers of the canonical v=8 / 256+256 format (5+
 * tokens = launches of the batched-decode kernel, 16 tokens each: 18 us per 8192^2 layer and
 * launch against 76-80 us for dequant + GEMM; measured crossover 48-64 tokens,
 * tools/tokens_crossover.py), 16 for its bf16 layers (launches of <= 4 tokens), 8 for every
 * other format.  0 if desc is invalid.
 */
VPTQ_API int vptq_quant_gemv_max_tokens(const VptqLayerDesc* desc);

/*
 * n independent layers in ONE launch (q/k/v or gate/up projections of a decoder
 * layer, or any batch of VQuantLinear GEMVs).  descs is a HOST array; x[i], y[i]
 * are device pointers for layer i.  Every layer must be eligible for the same
 * kernel family (checked); n <= VPTQ_GROUP_MAX.
 * Alignment: per layer as vptq_quant_gemv states it - the group takes gemv_k256 / gemv_k256m where EVERY member and every x[i] meets
 * their rule (16 bytes), else the members are served one by one ("per-layer"); y[i] and bias element-aligned.
 */
#define VPTQ_GROUP_MAX 64
VPTQ_API int vptq_quant_gemv_grouped(const VptqLayerDesc* descs, int n, const void* const* x,
                            void* const* y, int tokens, int flags, void* stream);

/*
 * n layers walked ONE AFTER THE OTHER by a single persistent launch (ABI >= 6): what the reference
 * does as n calls of `quant_gemv` (vptq/ops/quant_gemm.py:214-228, one per VQuantLinear of a decode
 * step), each of which pays a launch boundary, a prologue (codebooks into shared memory,
 * activations) and an epilogue.  Here every workgroup streams layer i's index words and, while it
 * does, requests layer i + 1's codebooks, activations and first index words, so HBM never idles
 * between layers.  Results are those of n vptq_quant_gemv calls in order (same arithmetic).
 *   - independent layers (default): no layer reads another layer's output (q / k / v, gate / up,
 *     a ring of benchmark layers): the layers overlap freely.
 *   - VPTQ_GEMV_CHAIN_DEPENDENT: x[i + 1] may be y[i]; a device-scope arrival counter per layer
 *     orders them.  Needs workspace of vptq_quant_gemv_chain_workspace_bytes(n, flags) bytes (the
 *     call clears it on the stream).
 * Served by one persistent launch per <= 32 layers when every layer is of the canonical v=8 / 256+256 format,
 * one dtype, without a permutation (absorb it first), tokens == 1 and the list has more than 8 layers
 * (vptq_quant_gemv_chain_kernel_name says "gemv_k256c_kernel"; with VPTQ_GEMV_EXACT: fp16, independent layers).
 * Shorter lists of independent layers - and lists the persistent kernel does not take - go out as ONE
 * vptq_quant_gemv_grouped launch ("grouped": faster than the persistent launch up to 8 layers; it serves members it
 * has no common kernel for one by one); a single layer, mixed dtypes and dependent lists the persistent kernel does
 * not take are executed as n vptq_quant_gemv calls ("per-layer").  descs is a HOST array; x[i], y[i] device pointers.
 * Alignment: the persistent launch takes layers that meet gemv_k256's rule (indices, codebooks, weight_scale, weight_bias, perm,
 * scale_permuted, bias_permuted 16 bytes) with every x[i] 4-byte aligned - in a dependent list that holds for y[i] = x[i + 1] too;
 * y[i] otherwise and bias element-aligned.  A list that misses the rule goes to the grouped / per-layer calls and their rules.
 * Workspace: dependent lists 4-byte aligned (VPTQ_E_WORKSPACE otherwise), contents don't matter (cleared by the call); the
 * permutation / selective workspace of vptq_quant_gemv_chain_workspace_bytes_for 256-byte aligned, contents don't matter - with a
 * smaller or less aligned one the call takes the routes that need none.  vptq_quant_gemv_chain_instance / _kernel_name see the
 * descriptors only: they answer for x[i] and a workspace that meet the rules.
 */
#define VPTQ_CHAIN_MAX 1024
VPTQ_API int vptq_quant_gemv_chain(const VptqLayerDesc* descs, int n, const void* const* x,
                          void* const* y, int tokens, int flags, void* workspace,
                          size_t workspace_bytes, void* stream);
VPTQ_API size_t vptq_quant_gemv_chain_workspace_bytes(int n, int flags);
/* the same + (independent lists, ABI >= 7) room for x[perm] of every layer with an input permutation: with that much
 * 256-byte aligned workspace such layers stay in the persistent launch (x is gathered by one small launch in front of
 * it); with less they are served by grouped / single launches, which apply permutations themselves.
 * flags | VPTQ_GEMV_SELECTIVE (ABI >= 10): + per launch of <= 32 layers 16 bytes per layer and 4 per output, in front of the
 * rest; with less (or NULL) the call takes VPTQ_GEMV_EXACT for every layer */
VPTQ_API size_t vptq_quant_gemv_chain_workspace_bytes_for(const VptqLayerDesc* descs, int n, int flags);
VPTQ_API const char* vptq_quant_gemv_chain_kernel_name(const VptqLayerDesc* descs, int n, int tokens,
                                              int flags);
/* Diagnostic (ABI >= 11): how ONE persistent chain launch of these n <= 32 layers (one token) deals its row groups of 8
 * vector-rows to its workgroups - the numbers the launch itself uses.  workgroups = 0: what a call would use (the device's
 * CUs; a dependent list at most 256); workgroups > 0: the plan for that many, no device needed.  Out: *visit = sweeps of
 * 2048 columns a block is sized for (32, 16 or 8: the longest whose blocks number at least 2 x the workgroups; 0: every
 * layer spread over all of them, and always for a dependent list), *grid = workgroups launched = min(blocks, workgroups),
 * and per layer i first_wg[i] (the workgroup that owns block 0; block k goes to (first_wg[i] + k) mod *grid) and
 * rows_per_wg[i] (row groups per block; the last block of a layer may be shorter).  Returns VPTQ_E_UNSUPPORTED for a list
 * the persistent launch does not take with these flags (whether the chain call would pick it is
 * vptq_quant_gemv_chain_kernel_name's answer). */
VPTQ_API int vptq_quant_gemv_chain_plan(const VptqLayerDesc* descs, int n, int flags, int workgroups, int* visit,
                                        int* grid, int* first_wg, int* rows_per_wg);
/* Diagnostic (added within ABI 12): the launch's SECOND geometry, "rows per wave" (gemv_k256c_rows_kernel; reported under the
 * family name "gemv_k256c_kernel", vptq_quant_gemv_chain_instance appends " geom=rows").  A wave owns a row group of 8
 * vector-rows across the layer's whole width, so no sum crosses the waves; a workgroup-task = 16 consecutive row groups of one
 * layer, one per wave, walked in steps of 128 columns; task k of layer i goes to workgroup (first_wg[i] + k) mod *grid, *grid =
 * the workgroups.  It serves fp16 layers, VPTQ_GEMV_EXACT, independent lists, 16-bit outputs (VPTQ_E_UNSUPPORTED otherwise, and
 * for a list the persistent launch does not take); vptq_quant_gemv_chain_plan goes on describing the first geometry for every
 * launch.  *taken = the rule's answer for a launch with `workgroups` workgroups (0: the device's): 1 where the tasks number at
 * least the workgroups AND the busiest workgroup's steps longest[0] (a step = 128 columns x 8 vector-rows per wave in both
 * geometries) do not exceed longest[1], those of the first geometry's plan for the same launch.  A launch follows the rule; the tuning
 * knob VPTQ_K256C_ROWS (with VPTQ_TUNING=1) overrides it: 0 = never, 1 = wherever the geometry serves the launch.  Out per layer:
 * tasks[i], steps[i] (per task).  An output's fp32 sum is formed per lane over all of its column blocks, then over 16 lanes in the first geometry's
 * tree: the weights are bit for bit vptq_dequant's, the outputs need not equal the first geometry's to the bit.  Alignment:
 * that of the chain call; y[i] is stored in 2-byte pieces. */
VPTQ_API int vptq_quant_gemv_chain_rows_plan(const VptqLayerDesc* descs, int n, int flags, int workgroups, int* taken,
                                             int* grid, int* first_wg, int* tasks, int* steps, int* longest);

/*
 * Many tokens (prefill): y[tokens, O] = x[tokens, I] @ W^T + bias with the dequantisation FUSED
 * into the GEMM - replaces `dequant` + F.linear of the reference (vptq/ops/quant_gemm.py:231-274),
 * which materialises the dense W (2 O I bytes) on every call.  Canonical v=8 / 256+256 format
 * without a permutation (absorb it first); fp16: the tile holds the reference's bits
 * r16(r16(r16(c+r)*s)+b), fp32 accumulate; bf16: folded form.  bf16 needs a workspace of
 * vptq_quant_gemm_workspace_bytes() (tokens floats).  vptq_quant_gemm_supported() = 1 when a
 * fused kernel exists for the layer; otherwise use vptq_dequant + a dense GEMM.
 * Alignment: the layer by gemv_k256's rule (indices, codebooks, weight_scale, weight_bias 16 bytes: part of "supported"); x 16 bytes
 * (VPTQ_E_ALIGN); the workspace 16 bytes, contents don't matter; y and bias element-aligned.
 */
VPTQ_API int vptq_quant_gemm_supported(const VptqLayerDesc* desc);
VPTQ_API size_t vptq_quant_gemm_workspace_bytes(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm(const VptqLayerDesc* desc, const void* x, void* y, int tokens, int flags,
                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * One token over a LOAD-TIME DERIVED LAYOUT of a large-codebook layer (k = 65536 main centroids; v = 8 with residual none,
 * 256 or 65536: "v8-k65536-0" / "-256" / "-65536"; v = 16 with residual none or 65536: "v16-k65536-0" / "-65536" - the
 * formats of most published checkpoints; ABI >= 6, the 65536-residual and v = 16 formats since round 4).  The reference
 * gathers centroid rows from a 1 - 2 MiB codebook through the caches (csrc/kernels/quant_gemv.cuh:11-186); here every row's
 * elements are bucketed ONCE per layer by the top bits of their index, so that a workgroup holds its slice of the codebook
 * in LDS:
 *   elems  : uint32, for slice s = 0..S-1 (E = 65536 / S entries per slice), for row n = 0..N-1
 *            (N = desc->num_indices): the elements of row n whose index / E == s, in any order, padded to a
 *            multiple of 64 with the word (column = group_size, local = 0);
 *            element word = column | (index mod E) << 16
 *   blocks : int32 [S][N], 64-element blocks of (s, n);  first : int32 [S][N], index of its first block
 *            (prefix sum of `blocks` in (s, n) order)
 *   rows_per_wave : 1 .. 64 consecutive rows per wave (16 waves per workgroup); the layout does not
 *            depend on it
 * (vptq_sliced_layout_plan / _fill below build it on the device; vptq_amd/utils/sliced.py:layout_from_indices is the torch model of
 * that builder and serves CPU tensors.)  It costs 2x (residual 256: 1.7x) the packed indices in device memory on
 * top of them; the state-dict tensors are untouched.  A layer with 65536 RESIDUAL centroids is served table by table
 * - (c + r) s x = c s x + r s x: the residual table's (slice, row block) workgroups run beside the main table's in the same
 * launch - and `layout` then points to TWO consecutive structs with the same rows_per_wave: [0] built from the main
 * indices, [1] from the residual indices (`res` unused).  workspace: vptq_quant_gemv_sliced_workspace_bytes, 16-byte aligned,
 * ZERO-FILLED ONCE by the caller before its first use - one 64-bit accumulator word per output (fixed-point sum | arrivals)
 * that the slices' partial sums are added to with returning atomics; the last arriver of an output rounds, stores y and
 * puts the word back to zero: every call leaves the workspace zero.  One workspace per layer and STREAM (two calls in flight
 * on different streams must not share one).  Arithmetic: flags = 0 the folded form (parity bar for dense activations, not
 * bit-equivalent); VPTQ_GEMV_EXACT (ABI >= 8) the reference's roundings per weight over a layout with the slice count
 * vptq_sliced_layout_supported_for(desc, VPTQ_GEMV_EXACT) answers.
 * Layers this path takes: group_size <= 32768; a permutation is applied while the activations are staged.
 * Alignment (every sliced entry: vptq_quant_gemv_sliced, _tokens, _grouped, _tokens_grouped): centroids, res_centroids, weight_scale,
 * weight_bias, perm and scale_permuted 16 bytes (VPTQ_GEMV_EXACT with a permutation: bias_permuted too) - a layer that misses this has
 * no layout (vptq_sliced_layout_supported* answer 0, the calls VPTQ_E_UNSUPPORTED); indices 4 bytes (set, not read); bias and y
 * element-aligned; x 16 bytes (VPTQ_E_UNSUPPORTED: take vptq_quant_gemv); the layout's elems, blocks, first and wstart 4 bytes, res
 * at an even address (uint8 and uint16 alike; a folded layout's uint8 res: any address), VPTQ_E_UNSUPPORTED otherwise; the workspace 16 bytes -
 * the VPTQ_GEMV_SELECTIVE one 256 - (VPTQ_E_WORKSPACE).  The column parts of VPTQ_GEMV_COLUMN_PARTS advance weight_scale, weight_bias,
 * perm, scale_permuted and bias_permuted by 2 x the part's first column bytes: a multiple of 16, so the parts keep the layer's alignment.
 */
typedef struct VptqSlicedLayout {
  const void* elems;
  const void* blocks;
  const void* first;
  const void* res;          /* uint8 per element (same order, padding = 0): residual index of v = 8's 256-entry table; NULL without
                             * residual codebook.  VPTQ_GEMV_EXACT layouts (ABI >= 8) of layers with ANY OTHER residual codebook:
                             * uint16 per element - the residual entry is gathered from the codebook in device memory */
  int32_t rows_per_wave;
  int32_t elems_per_lane;   /* 1 (or 0): a block = 64 elements */
  int32_t n_slices;         /* 8 (or 0) / 16 / 32: what vptq_sliced_layout_supported() answers for the layer */
  int32_t whole_table;      /* 0: element words carry the index INSIDE the slice (the workgroup holds its slice of the table);
                             * 1: the full index (every workgroup of this table holds all of it: small residual tables) */
  const void* wstart;       /* int32 [S][N][VPTQ_SLICED_WINDOWS + 1], or NULL (one token only): every (s, n) list is ordered by
                             * COLUMN WINDOW - window w = columns [w C, (w + 1) C), C = group_size / 4 rounded up to a multiple
                             * of 8, the last window taking what is left - and wstart[s][n][w] is the position inside the list
                             * at which window w begins, [VPTQ_SLICED_WINDOWS] the list's length without padding.  What
                             * vptq_quant_gemv_sliced_tokens walks; one token ignores it */
} VptqSlicedLayout;
#define VPTQ_SLICED_WINDOWS 4
/* 0 = not a layer of this path; else the number of slices its layout(s) must have: v = 8: 8 slices of 8192 entries while
 * the activations fit in LDS beside them (group_size <= 14336, 14080 with the 256-entry residual codebook), else 16 of
 * 4096; v = 16 (32-byte entries): 16 slices of 4096 entries, beyond 14336 columns 32 of 2048 */
VPTQ_API int vptq_sliced_layout_supported(const VptqLayerDesc* desc);
/* ... and for the arithmetic a call will ask for (ABI >= 8): flags = 0 as above; VPTQ_GEMV_EXACT - the reference's roundings per
 * weight, w = f16(f16(f16(c + r) * s) + b) (vptq/ops/quant_gemm.py:121,155-156), what gemv_gather computes through the caches -
 * needs c and r in one lane, so it always takes ONE layout, bucketed by the main index (vptq_sliced_layout_tables() is the folded
 * form's answer): no residual codebook; v = 8 with 256 residual centroids (`res` bytes, table in LDS); any other residual
 * codebook: `res` = uint16 residual indices, the entry gathered from device memory (one of the gather kernel's two cache
 * gathers per element).  Scale, bias and x of every column sit beside the slice, 6 instead of 2 bytes of LDS per column:
 * v = 8: 8 slices up to 5376 columns (4704 with the 256-entry table), 16 up to 16288 (15616); v = 16: 16 / 32; wider layers: 0.
 * A layout built with THAT slice count serves vptq_quant_gemv_sliced(..., flags | VPTQ_GEMV_EXACT, ...) and - one-table formats,
 * ABI >= 9 - vptq_quant_gemv_sliced_tokens(..., flags | VPTQ_GEMV_EXACT, ...). */
VPTQ_API int vptq_sliced_layout_supported_for(const VptqLayerDesc* desc, int flags);
/* 0, or how many consecutive VptqSlicedLayout structs vptq_quant_gemv_sliced takes for this layer: 1 (no residual codebook;
 * v = 8 with 256 residual centroids: `res` bytes), 2 (any other residual codebook: a second table with a layout of its own) */
VPTQ_API int vptq_sliced_layout_tables(const VptqLayerDesc* desc);
/* the `whole_table` value the layout of table 0 / 1 must be built with (1: a small residual table every workgroup holds whole) */
VPTQ_API int vptq_sliced_layout_whole_table(const VptqLayerDesc* desc, int table);
/* ALL of the above in one answer (added within ABI 11; present when the symbol is): the layouts a layer is served from in the
 * arithmetic of `flags` (0: the folded form; VPTQ_GEMV_EXACT: the reference's roundings) - what every sliced entry, the builder and
 * vptq_sliced_layout_repack hold the structs they are handed to.
 *   parts          0: the layer is not served (every other field 0).  Folded: 1.  Exact: 1 where the layer fits in one piece, else 2 or 3
 *                  equal COLUMN PARTS of a multiple of 8 columns (layers wider than ~16300 columns; VPTQ_GEMV_COLUMN_PARTS) whose
 *                  parts x n_slices arrivals one accumulator word counts (<= 127).  The tuning knob VPTQ_SLICED_PARTS = 2 / 3 (read
 *                  here and nowhere else): at least that many parts where the columns divide.
 *   tables         consecutive structs per part: 1, or 2 (folded form, a residual codebook other than v = 8's 256-entry one)
 *   n_slices       of every struct (a part's: what vptq_sliced_layout_supported_for answers for the part's descriptor)
 *   whole_table[t] the value table t's struct carries
 *   side_bytes     the `res` stream beside table 0's element words: 0 none; 1 uint8 (v = 8 with 256 residual centroids); 2 uint16
 *                  (exact layouts of any other residual codebook); folded two-table layouts: 0
 * Returns VPTQ_OK - also for a layer that is not served -, an error only for a bad descriptor or out = NULL. */
typedef struct VptqSlicedLayoutSet {
  int32_t parts, tables, n_slices, whole_table[2], side_bytes, reserved[2];
} VptqSlicedLayoutSet;
VPTQ_API int vptq_sliced_layout_set(const VptqLayerDesc* desc, int flags /* VPTQ_GEMV_EXACT or 0 */, VptqSlicedLayoutSet* out);
VPTQ_API size_t vptq_quant_gemv_sliced_workspace_bytes(const VptqLayerDesc* desc);
VPTQ_API int vptq_quant_gemv_sliced(const VptqLayerDesc* desc, const VptqSlicedLayout* layout, const void* x,
                           void* y, int flags, void* workspace, size_t workspace_bytes, void* stream);
/* flags | VPTQ_GEMV_SELECTIVE (ABI >= 10; the FOLDED layouts, i.e. without VPTQ_GEMV_EXACT): the folded form over the layouts, with the
 * reference's roundings on the blocks of 128 columns an activation dominates.  A small launch in front (gemv_hot.hip) finds the
 * threshold, writes the activation with those blocks' input features zeroed - what the folded launch then reads - and the blocks'
 * exact products per output (entries gathered from the codebooks in device memory: few columns), which the folded launch adds before
 * its one rounding.  fp16 layers with scale and bias (vptq_quant_gemv_sliced_selective_supported); workspace:
 * vptq_quant_gemv_sliced_workspace_bytes_for(desc, flags) bytes, 256-byte aligned, zero-filled once (the accumulator words come first).
 * What it buys: the two-table formats (v8-k65536-65536, v16-k65536-65536) at the folded form's speed - 8192^2: 59 / 46 us in the
 * reference's roundings, ~21 / ~22 here - without the folded form's activation-dependent failures; opt-in, like every use of the flag. */
VPTQ_API int vptq_quant_gemv_sliced_selective_supported(const VptqLayerDesc* desc);
VPTQ_API size_t vptq_quant_gemv_sliced_workspace_bytes_for(const VptqLayerDesc* desc, int flags);

/* 2 - 4 tokens (5 - 8 where 16 bytes of activations per column still fit the LDS in 4 phases: layers of up to ~4600 columns)
 * over the same layouts (ABI >= 7; needs `wstart`): x [tokens][in_features], y [tokens][out_features]
 * (float32 with VPTQ_GEMV_OUT_F32), one launch.  The activations of T tokens do not fit beside a slice, so the kernel takes
 * the columns in 1, 2 or 4 phases (as few as the LDS allows: 4096-column layers need one for 2 - 3 tokens) and walks the
 * phase's column windows of every list.  workspace: vptq_quant_gemv_sliced_tokens_workspace_bytes(desc, tokens), zero-filled
 * once, one per layer and stream, not shared with the one-token call; a workspace for T tokens serves fewer as well (the
 * arrival counters sit in front).  VPTQ_E_UNSUPPORTED where the layer, the layout
 * (no wstart) or the token count is not served: take vptq_quant_gemv.  Replaces the same reference kernel for
 * 1 < tokens < 16 (vptq/ops/quant_gemm.py:213, csrc/kernels/quant_gemv.cuh:11-186).
 * flags | VPTQ_GEMV_EXACT (ABI >= 9): the reference's roundings per weight over an EXACT layout (vptq_sliced_layout_supported_for(desc,
 * VPTQ_GEMV_EXACT) slices) of a one-table format (no residual codebook; v = 8 with 256 residual centroids): scale and bias of a
 * column are staged beside its activations (8 more bytes of LDS per column and phase), every weight is rebuilt as
 * f16(f16(f16(c + r) s) + b) in the matrix pipe's operand layout; vptq_quant_gemv_sliced_tokens_supported_for says whether the
 * layer's columns fit (4 phases x (2 x token slots + 8) bytes beside the slice: 5 - 8 tokens up to ~16000 columns).  2 / 3 tokens (v = 16:
 * 2) of a layer whose slice leaves room for 2 x tokens + 4 bytes per column take ONE PASS of the one-token kernel instead (no `wstart`
 * needed; accumulator words behind the arrival counters of the same workspace). */
VPTQ_API int vptq_quant_gemv_sliced_tokens_supported(const VptqLayerDesc* desc, const VptqSlicedLayout* layout, int tokens);
VPTQ_API int vptq_quant_gemv_sliced_tokens_supported_for(const VptqLayerDesc* desc, const VptqSlicedLayout* layout, int tokens, int flags);
/* 0, or in how many WINDOW PARTS vptq_quant_gemv_sliced_tokens(..., flags) takes these tokens in ONE PASS of the one-token kernel (ABI >= 9,
 * flags | VPTQ_GEMV_EXACT, 2 / 3 tokens): 1 = every column's operands fit beside the slice (no `wstart` needed); 2 / 4 = v = 8 one-table layers
 * whose slice leaves room for half / a quarter of the columns (4096 columns beside a 128 KiB slice, 14336 beside 64 KiB): that many workgroups
 * per (slice, row block), each staging its column windows alone and walking their part of every list (`wstart` needed) */
VPTQ_API int vptq_quant_gemv_sliced_tokens_one_pass(const VptqLayerDesc* desc, int tokens, int flags);
VPTQ_API size_t vptq_quant_gemv_sliced_tokens_workspace_bytes(const VptqLayerDesc* desc, int tokens);
/* VPTQ_GEMV_SELECTIVE here (and on vptq_quant_gemv_sliced_grouped / _tokens_grouped, which have no selective form either) is taken
 * as VPTQ_GEMV_EXACT: the layout must then be one of the EXACT slice count, otherwise the call returns VPTQ_E_UNSUPPORTED. */
VPTQ_API int vptq_quant_gemv_sliced_tokens(const VptqLayerDesc* desc, const VptqSlicedLayout* layout, const void* x, void* y,
                                  int tokens, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* ... and for up to 3 sibling layers (one format, dtype and input width, the SAME x [tokens][in_features]) in one launch, as
 * vptq_quant_gemv_sliced_grouped does for one token: y / workspaces / workspace_bytes one per layer
 * (vptq_quant_gemv_sliced_tokens_workspace_bytes each) */
VPTQ_API int vptq_quant_gemv_sliced_tokens_grouped(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, const void* x,
                                          void* const* y, int tokens, int flags, void* const* workspaces,
                                          const size_t* workspace_bytes, void* stream);

/* Up to 3 layers of ONE format, dtype and input width that read the SAME activation (q / k / v, gate / up) in one launch
 * (ABI >= 7): layouts = the layers' structs one after the other (vptq_sliced_layout_tables() each; give every struct the
 * group's rows_per_wave - one round of workgroups over ALL layers), y / workspaces / workspace_bytes one per layer.  The
 * fixed part of a sliced launch (boundary, slice copy, staging, cross-slice hand-over: ~7 of the 10 us of a 4096 x 4096
 * layer) is paid once.
 * flags | VPTQ_GEMV_EXACT | VPTQ_GEMV_COLUMN_PARTS (ABI >= 9): the n descriptors are the COLUMN RANGES [i G / n, (i + 1) G / n) of ONE
 * layer that is too wide for the reference's roundings in one piece (6 bytes of LDS per column: 28672-column layers) - copies of
 * the layer's descriptor with in_features = group_size = G / n (a multiple of 8) and weight_scale / weight_bias / perm /
 * scale_permuted / bias_permuted advanced to the part's first column, a layout per part built from those columns of the index
 * matrix (columns counted from the part's first); x = the WHOLE activation, y[i] = y[0], workspaces[i] = workspaces[0]: the parts
 * meet in the output's accumulator word (n x slices arrivals; at most 127).  vptq_quant_gemv_sliced_tokens_grouped takes the same flags for
 * 2 / 3 tokens where every part takes them in one pass (vptq_quant_gemv_sliced_tokens_one_pass(part, tokens, flags) != 0): x [tokens][G]. */
VPTQ_API int vptq_quant_gemv_sliced_grouped(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n,
                                   const void* x, void* const* y, int flags, void* const* workspaces,
                                   const size_t* workspace_bytes, void* stream);

/* Rebuild a layer's packed int32 indices [1][N][row_words] from its EXACT sliced layout(s): `parts` consecutive structs,
 * part p covering columns [p G / parts, (p + 1) G / parts) (vptq_sliced_layout_set(desc, VPTQ_GEMV_EXACT).parts of them).
 * Output is bit-identical to the packed stream the layout was built from, with zero bits past G*T in each row's last word.
 * desc is validated like the sliced entries': its `indices` must be non-NULL but is not read.
 *
 * Added within ABI 11; present when the symbol is.  An exact layout (vptq_sliced_layout_supported_for(desc, VPTQ_GEMV_EXACT)
 * slices, whole_table = 0) holds every bit of the packed stream: the element word gives the column (+ the part's first column)
 * and the index inside the slice, the (slice, row) list it sits in the slice and the row - index = slice << (index_bits -
 * log2(slices)) | local -, and `res` the residual index (uint8: v = 8 with 256 residual centroids; uint16: any other residual
 * codebook).  Padding words (column = part width) are skipped.  So a layer served from such a layout needs no packed copy: the
 * paths that read the stream (the gather kernels; vptq_dequant where vptq_dequant_sliced below is not taken) get it from here, into
 * a scratch buffer.  Folded layouts (two
 * tables, whole tables) are not taken.  Errors: NULL layouts / out (VPTQ_E_NULL), `parts` other than the layer's
 * (VPTQ_E_SHAPE), a part's n_slices other than vptq_sliced_layout_supported_for(part, VPTQ_GEMV_EXACT) (VPTQ_E_SHAPE), an out
 * pointer not 16-byte aligned (VPTQ_E_ALIGN); nothing is launched then.  One workgroup per row, the row assembled in LDS.
 * Alignment: the descriptor as the sliced entries take it; indices_out 16 bytes; elems 16 bytes, blocks / first / wstart 4 bytes, a
 * uint8 res 4 bytes, a uint16 res 8 bytes (VPTQ_E_ALIGN). */
VPTQ_API int vptq_sliced_layout_repack(const VptqLayerDesc* desc, const VptqSlicedLayout* layouts, int parts, void* indices_out,
                                       void* stream);

/* W[O, I] dense, row-major, desc->dtype, STRAIGHT FROM the layer's EXACT sliced layout(s): bit for bit what vptq_dequant writes for
 * the packed indices the layouts were built from (= vptq_sliced_layout_repack + vptq_dequant, without the packed stream, its scratch
 * buffer and one launch) - the many-token route and dequant() of a layer that holds its indices in the layout only.
 * Added within ABI 11; present when the symbol is.  `layouts`, `parts`: as vptq_sliced_layout_repack takes them, and validated the
 * same way - NULL layouts / W (VPTQ_E_NULL), `parts` other than the layer's (VPTQ_E_SHAPE), a part's n_slices other than the exact
 * answer (VPTQ_E_SHAPE), folded or whole-table layouts and layers without an exact layout (VPTQ_E_UNSUPPORTED), W - or a pointer of the
 * layout - not aligned as repack asks (W: 16 bytes; VPTQ_E_ALIGN); nothing is launched then.  desc->indices must be non-NULL and is
 * not read.  The kernel reads desc->perm (column g of the quantised matrix is column perm[g] of W), never desc->inv_perm: any
 * descriptor of the layer that its exact layouts are valid for serves, the one of the sliced entries and the dense one alike.  A
 * layout's `wstart`, where set (4-byte aligned), bounds the walk of a column tile; NULL is accepted.  One workgroup per vector-row
 * and column tile, the tile assembled in LDS and stored in 16-byte pieces; no workspace, no allocation: graph-capturable.
 * Alignment: the descriptor as the sliced entries take it; W 16 bytes; the layout
 * tensors as vptq_sliced_layout_repack takes them (elems 16, blocks / first / wstart 4, uint8 res 4, uint16 res 8 bytes: VPTQ_E_ALIGN). */
VPTQ_API int vptq_dequant_sliced(const VptqLayerDesc* desc, const VptqSlicedLayout* layouts, int parts, void* W, void* stream);

/* Build a sliced layout from the packed indices ON THE DEVICE: the forward direction of vptq_sliced_layout_repack, and byte for
 * byte what the torch recipe vptq_amd/utils/sliced.py:layout_from_indices builds (the recipe stays the model and serves CPU tensors).
 * Added within ABI 11; present when the symbols are.
 *
 * `spec` names the layout wanted - every one vptq_amd/utils/sliced.py:SlicedGemv builds:
 *   flags       0: a layout of the folded form; VPTQ_GEMV_EXACT: one of the reference's roundings
 *   n_slices    what vptq_sliced_layout_supported_for(desc - or the column part of it -, flags) answers
 *   table       0: bucketed by the main index; 1 (folded two-table formats, vptq_sliced_layout_tables() == 2): the residual
 *               codebook as a second table, bucketed by the residual index
 *   whole_table what vptq_sliced_layout_whole_table(desc, table) answers (folded; exact layouts: 0): slice = column * S / G, the
 *               element word carries the whole index
 *   side_bytes  the `res` side stream beside the element words: 0 none; 1 uint8 residual indices (v = 8 with 256 residual
 *               centroids, table 0, one-table layouts); 2 uint16 (exact layouts of any other residual codebook)
 *   parts, part 1, 0 - or (exact) the layer's 2 - 3 column parts and which of them: columns [part G / parts, (part + 1) G / parts),
 *               counted from the part's first; two parts may share a 32-bit word of the packed row
 * The layout's size depends on the data (lists are padded to blocks of 64 elements), so the build has two steps with one
 * device -> host read between them:
 *   plan : blocks int32 [S][N], first int32 [S][N], wstart int32 [S][N][VPTQ_SLICED_WINDOWS + 1] and *total_blocks (int64, device)
 *   fill : elems uint32 x 64 x max(total, 1) and, with side_bytes, res (uint8 / uint16 per element) - `out` carries the five
 *          pointers (n_slices as in spec; the other fields are not read), total_blocks is the number read back, past which nothing
 *          is stored
 * Order inside a list: rows of 16 different LDS bank classes (local & 15) first, the surplus spread evenly behind them by the
 * recipe's float64 key, evaluated in the same order; equal keys (the recipe leaves their order open) by class, then column.
 * Errors, before any launch: NULL pointers (VPTQ_E_NULL); n_slices / parts / part other than the layer's (VPTQ_E_SHAPE); formats
 * without a layout, a table / whole_table / side_bytes the layer's layouts do not have (VPTQ_E_UNSUPPORTED); blocks / first /
 * wstart / res not 4-byte, total_blocks not 8-byte, elems not 16-byte aligned (VPTQ_E_ALIGN).  No allocation, no synchronisation.
 * flags | VPTQ_LAYOUT_ANY_SHAPE: the spec is taken as written - any slice count of 8 / 16 / 32, any 1 - 3 parts that divide the
 * columns, any table, whole_table and side_bytes the index widths allow - for layouts no GEMV entry of this
 * library takes (tests of the builder against its model, tools); everything that guards memory is still checked.
 * Alignment: desc->indices 4 bytes (the only tensor of the descriptor the builder reads); the outputs as listed under Errors. */
#define VPTQ_LAYOUT_ANY_SHAPE (1 << 16)
typedef struct VptqSlicedLayoutSpec {
  int32_t flags;
  int32_t n_slices;
  int32_t table;
  int32_t whole_table;
  int32_t side_bytes;
  int32_t parts;
  int32_t part;
  int32_t reserved;   /* 0 */
} VptqSlicedLayoutSpec;
VPTQ_API int vptq_sliced_layout_plan(const VptqLayerDesc* desc, const VptqSlicedLayoutSpec* spec, void* blocks, void* first,
                                     void* wstart, void* total_blocks, void* stream);
VPTQ_API int vptq_sliced_layout_fill(const VptqLayerDesc* desc, const VptqSlicedLayoutSpec* spec, const VptqSlicedLayout* out,
                                     int64_t total_blocks, void* stream);

/* Batched decode of the large-codebook formats: 1 - 16 tokens in ONE launch (gemm_gather.hip; added within ABI 12; present when the
 * symbols are).  The layers vptq_quant_gemv serves with gemv_gather_kernel - v = 8, 65536 main centroids, 0 / 256 / 65536 residual
 * centroids ("v8-k65536-0", "-256", "-65536"), one codebook group, no outlier columns, weight_scale and weight_bias set, group_size ==
 * in_features (a multiple of 8), indices and codebooks 16-byte aligned - with the tokens as the M dimension of a 16x16x32 MFMA: one
 * pass over the packed indices and one gather per index for any token count, where vptq_quant_gemv takes 8 tokens per pass.  The
 * reference's roundings per weight (bit-identical to vptq_dequant's W), fp32 sums added in a fixed order (two calls give the same
 * bits), one rounding of the output, the output bias added in fp32.  No workspace, no atomics; graph-capturable.
 *   x [tokens][in_features], y [tokens][out_features], desc->dtype; flags: VPTQ_GEMV_OUT_F32 stores the fp32 sums (y is float32);
 *   VPTQ_GEMV_FAST_MATH / _EXACT / _SELECTIVE are accepted and change nothing.
 * vptq_quant_gemm_gather_supported: 1 where the call serves (desc, tokens), else 0; host logic.
 * vptq_quant_gemm_gather: NULL desc / x / y VPTQ_E_NULL; tokens outside [1, 16] VPTQ_E_TOKENS; a layer it does not serve, or an x that
 *   is not 16-byte aligned, VPTQ_E_UNSUPPORTED; nothing is launched then.
 * vptq_quant_gemm_gather_instance: the instantiation of gemm_gather_kernel<DT, T, PERM> and the launch shape, as one line (the
 *   launcher's own decision; host logic, without a device the CU count is taken as 256):
 *   gemm_gather dt=f16|bf16 t=16|24|32 perm=0|1 tok=N tiles=N rgs=N
 *       t the index width, tok the tokens of the launch, tiles the column tiles (1024 columns) per row group (2 vector-rows), rgs the
 *       most row groups one workgroup walks.  Returns VPTQ_OK, the call's own validation error, or VPTQ_E_WORKSPACE (buf too small).
 * vptq_quant_gemv, vptq_quant_gemv_max_tokens and vptq_quant_gemv_kernel_name do not route here: callers choose this entry.
 * Alignment (vptq_quant_gemm_gather, _gatherx, _gatherw): indices, centroids, res_centroids 16 bytes and weight_scale, weight_bias, perm,
 * scale_permuted, bias_permuted 4 bytes (part of "supported"); x 16 bytes (the code given above); y and bias element-aligned. */
VPTQ_API int vptq_quant_gemm_gather_supported(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm_gather(const VptqLayerDesc* desc, const void* x, void* y, int tokens, int flags, void* stream);
VPTQ_API int vptq_quant_gemm_gather_instance(const VptqLayerDesc* desc, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of the large-codebook formats vptq_quant_gemm_gather does not serve: 1 - 16 tokens in ONE launch (gemm_gatherx.hip;
 * added within ABI 12; present when the symbols are).  Vector length 8 or 16, 16384 ... 65536 main centroids, any residual codebook or
 * none (index_bits + res_bits <= 32: "v16-k65536-65536", "-32768", "-1024", "-256", "-64", "-0", "v8-k65536-4096", "-4", "v8-k32768-0",
 * "v8-k16384-0"), one codebook group, no outlier columns, weight_scale and weight_bias set (with perm: scale_permuted and
 * bias_permuted), group_size == in_features (a multiple of 8), row_words * 32 >= group_size * (index_bits + res_bits), indices and
 * codebooks 16-byte aligned - and NOT a layer vptq_quant_gemm_gather_supported accepts: a layer has one batched-decode kernel.  The same
 * arithmetic and guarantees as vptq_quant_gemm_gather: the reference's roundings per weight (bit-identical to vptq_dequant's W), fp32
 * sums added in a fixed order, one rounding of the output, the output bias added in fp32; no workspace, no atomics; graph-capturable.
 * A residual table of at most 32 KiB is held in LDS, a larger one is gathered from L2.
 *   x [tokens][in_features], y [tokens][out_features], desc->dtype; flags: VPTQ_GEMV_OUT_F32 stores the fp32 sums (y is float32);
 *   VPTQ_GEMV_FAST_MATH / _EXACT / _SELECTIVE are accepted and change nothing.
 * vptq_quant_gemm_gatherx_supported: 1 where the call serves (desc, tokens), else 0; host logic.
 * vptq_quant_gemm_gatherx: NULL desc / x / y VPTQ_E_NULL; tokens outside [1, 16] VPTQ_E_TOKENS; a layer it does not serve, or an x that
 *   is not 16-byte aligned, VPTQ_E_UNSUPPORTED; nothing is launched then.
 * vptq_quant_gemm_gatherx_instance: the instantiation of gemm_gatherx_kernel<DT, V, RES, PERM>, the run-time index widths and the
 *   launch shape, as one line (the launcher's own decision; host logic, without a device the CU count is taken as 256):
 *   gemm_gatherx dt=f16|bf16 v=8|16 ib=N rb=N res=none|lds|l2 perm=0|1 tok=N tiles=N wgcu=N rgs=N
 *       ib / rb the main / residual index widths, res where the residual entries come from, tok the tokens of the launch, tiles the
 *       column tiles (1024 columns) per row group (16 outputs), wgcu the workgroups per CU the LDS in use (32 KiB + an LDS-held
 *       table) leaves, rgs the most row groups one workgroup walks.  Returns as vptq_quant_gemm_gather_instance does.
 * vptq_quant_gemv, vptq_quant_gemv_max_tokens, vptq_quant_gemv_kernel_name and vptq_quant_gemm_gather* are what they were. */
VPTQ_API int vptq_quant_gemm_gatherx_supported(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm_gatherx(const VptqLayerDesc* desc, const void* x, void* y, int tokens, int flags, void* stream);
VPTQ_API int vptq_quant_gemm_gatherx_instance(const VptqLayerDesc* desc, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of the canonical format for 17 - 64 tokens in ONE launch (gemm_k256w_kernel in gemm_k256.hip; added within ABI 12;
 * present when the symbols are).  The layers vptq_quant_gemv serves with gemm_k256_kernel - v = 8, 256 main + 256 residual centroids,
 * one codebook group, no outlier columns, weight_scale and weight_bias set (with perm: scale_permuted and bias_permuted), group_size ==
 * in_features (a multiple of 8) - with the tokens as tb = ceil(tokens / 16) blocks of the M dimension of a 16x16x16 MFMA: the indices
 * are read, gathered and rebuilt once for all blocks, where vptq_quant_gemv runs tb launches of 16 tokens.  The reference's roundings
 * per weight (w = r16(r16(r16(c + r) * s) + b): vptq_dequant's bits); the K-step -> wave mapping and the order of the fp32 sums are
 * gemm_k256_kernel's and do not depend on the token count or on a token's slot: a token's output bits are the same in every slot of
 * every batch, and equal those of vptq_quant_gemv where it launches gemm_k256_kernel.  No workspace, no atomics; graph-capturable.
 *   x [tokens][in_features], y [tokens][out_features], desc->dtype; flags: VPTQ_GEMV_OUT_F32 stores the fp32 sums (y is float32);
 *   VPTQ_GEMV_FAST_MATH / _EXACT / _SELECTIVE are accepted and change nothing.
 * vptq_quant_gemm_k256w_supported: 1 where the call serves (desc, tokens) - such a layer and 17 <= tokens <= 64 - else 0; host logic.
 * vptq_quant_gemm_k256w: NULL desc / x / y VPTQ_E_NULL; tokens outside [17, 64], or an x that is not 16-byte aligned, VPTQ_E_TOKENS; a
 *   layer it does not serve VPTQ_E_UNSUPPORTED; nothing is launched then.
 * vptq_quant_gemm_k256w_instance: the instantiation of gemm_k256w_kernel<DT, PERM, TB> and the launch shape, as one line (the launcher's
 *   own decision; host logic, without a device the CU count is taken as 256):
 *   gemm_k256w dt=f16|bf16 perm=0|1 tok=N tb=2|3|4 rgs=N pass=1x2|1x3|1x4
 *       tok the tokens of the launch, tb its token blocks, rgs the most row groups (4 vector-rows) one workgroup walks, pass the
 *       instantiation <NRG, TB> of gemm_k256's pass it runs per row group (NRG row groups x TB token blocks share the 32 accumulator
 *       registers; NRG is 1).  Returns as vptq_quant_gemm_gather_instance does.
 * vptq_quant_gemv, vptq_quant_gemv_max_tokens (48) and vptq_quant_gemv_kernel_name do not route here: callers choose this entry.
 * Alignment: the layer by gemv_k256's rule (indices, codebooks, weight_scale, weight_bias, perm, scale_permuted, bias_permuted 16 bytes:
 * part of "supported"); x 16 bytes (VPTQ_E_TOKENS, as above); y and bias element-aligned. */
VPTQ_API int vptq_quant_gemm_k256w_supported(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm_k256w(const VptqLayerDesc* desc, const void* x, void* y, int tokens, int flags, void* stream);
VPTQ_API int vptq_quant_gemm_k256w_instance(const VptqLayerDesc* desc, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of the large-codebook formats for 17 - 48 tokens in ONE launch (gemm_gatherw_kernel in gemm_gatherw.hip; added within
 * ABI 12; present when the symbols are).  The layers vptq_quant_gemm_gather serves - v = 8, 65536 main centroids, 0 / 256 / 65536
 * residual centroids, one codebook group, no outlier columns, weight_scale and weight_bias set (with perm: scale_permuted and
 * bias_permuted), group_size == in_features (a multiple of 8), indices and codebooks 16-byte aligned - with the tokens as tb =
 * ceil(tokens / 16) blocks of the M dimension of a 16x16x32 MFMA: the indices are read, gathered and rebuilt once for all blocks,
 * where 17+ tokens had no kernel (vptq_dequant + a dense GEMM).  The reference's roundings per weight (bit-identical to
 * vptq_dequant's W), fp32 sums added in a fixed order, one rounding of the output, the output bias added in fp32.  The order of the
 * sums is gemm_gather_kernel's and does not depend on the token count or on a token's slot: a token's output bits are the same in
 * every slot of every batch, and equal those vptq_quant_gemm_gather gives that token in a launch of up to 16.  No workspace, no
 * atomics; graph-capturable.
 *   x [tokens][in_features], y [tokens][out_features], desc->dtype; flags: VPTQ_GEMV_OUT_F32 stores the fp32 sums (y is float32);
 *   VPTQ_GEMV_FAST_MATH / _EXACT / _SELECTIVE are accepted and change nothing.
 * vptq_quant_gemm_gatherw_supported: 1 where the call serves (desc, tokens) - such a layer and 17 <= tokens <= 48 - else 0; host logic.
 * vptq_quant_gemm_gatherw: NULL desc / x / y VPTQ_E_NULL; tokens outside [17, 48], or an x that is not 16-byte aligned, VPTQ_E_TOKENS
 *   (the tokens are checked before the layer); a layer it does not serve VPTQ_E_UNSUPPORTED; nothing is launched then.
 * vptq_quant_gemm_gatherw_instance: the instantiation of gemm_gatherw_kernel<DT, T, PERM, TB> and the launch shape, as one line (the
 *   launcher's own decision; host logic, without a device the CU count is taken as 256):
 *   gemm_gatherw dt=f16|bf16 t=16|24|32 perm=0|1 tok=N tb=2|3 tiles=N rgs=N
 *       t the index width, tok the tokens of the launch, tb its token blocks, tiles the column tiles (1024 columns) per row group (2
 *       vector-rows), rgs the most row groups one workgroup walks.  Returns as vptq_quant_gemm_gather_instance does.
 * vptq_quant_gemv, vptq_quant_gemv_max_tokens, vptq_quant_gemv_kernel_name and vptq_quant_gemm_gather* (1 - 16 tokens) are what they
 * were: callers choose this entry. */
VPTQ_API int vptq_quant_gemm_gatherw_supported(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm_gatherw(const VptqLayerDesc* desc, const void* x, void* y, int tokens, int flags, void* stream);
VPTQ_API int vptq_quant_gemm_gatherw_instance(const VptqLayerDesc* desc, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of layers WITH a column permutation: x[perm] gathered once per call into a workspace (gemm_gather_px.hip; added
 * within ABI 12; present when the symbols are).  The three entries above read a permuted x two bytes at a time in every row group of
 * 16 outputs.  This entry writes xp[t][c] = x[t][perm[c]] once (permute_x_tokens_kernel: a thread owns 8 columns and up to 4 tokens,
 * one 16-byte store per token) and then launches the layer's own kernel - gemm_gather_kernel or gemm_gatherx_kernel for 1 - 16 tokens,
 * gemm_gatherw_kernel for 17 - 48 - in its form WITHOUT a permutation over xp, scale_permuted and bias_permuted.  Both launches go to
 * `stream`; nothing is allocated: graph-capturable.  The outputs are BIT-IDENTICAL to those vptq_quant_gemm_gather / _gatherx /
 * _gatherw give for the same descriptor, and carry their guarantees.  A layer without a permutation is served too: the plain launch
 * alone, the workspace is not touched and may be NULL.
 *   x [tokens][in_features], y [tokens][out_features], desc->dtype; flags as the three entries take them.
 * vptq_quant_gemm_gather_px_workspace_bytes: tokens * group_size * 2 rounded up to 256; 0 for a layer without a permutation and
 *   where vptq_quant_gemm_gather_px_supported answers 0.
 * vptq_quant_gemm_gather_px_supported: 1 exactly where the layer's own entry answers 1 for that token count
 *   (vptq_quant_gemm_gather_supported or vptq_quant_gemm_gatherx_supported for 1 - 16 tokens, vptq_quant_gemm_gatherw_supported for
 *   17 - 48), else 0; host logic.
 * vptq_quant_gemm_gather_px: NULL desc / x / y VPTQ_E_NULL; tokens outside [1, 48] VPTQ_E_TOKENS; a layer it does not serve
 *   VPTQ_E_UNSUPPORTED; an x that is not 16-byte aligned the code of the layer's own entry (VPTQ_E_UNSUPPORTED up to 16 tokens,
 *   VPTQ_E_TOKENS from 17); then, for a layer with a permutation, a NULL workspace or fewer workspace_bytes than the query answers
 *   VPTQ_E_WORKSPACE and a workspace that is not 16-byte aligned VPTQ_E_ALIGN; nothing is launched then.
 * vptq_quant_gemm_gather_px_instance: both launches as one line (host logic, without a device the CU count is taken as 256):
 *   permute_x_tokens g=N tok=N grid=XxY tpt=4 | <inner>      with a permutation
 *   none | <inner>                                           without one
 *       g the columns, tok the tokens, grid X workgroups of 64 threads (8 columns each) x Y token slices, tpt the tokens per thread;
 *       <inner> the line vptq_quant_gemm_gather_instance / _gatherx_instance / _gatherw_instance prints for the descriptor without
 *       its permutation (always perm=0).  Returns as vptq_quant_gemm_gather_instance does.
 * Workspace: contents do not matter before a call and are undefined after it; calls on one stream may share it.
 * Alignment: the layer as vptq_quant_gemm_gather, _gatherx, _gatherw take it (indices, centroids, res_centroids 16 bytes and
 * weight_scale, weight_bias, perm, scale_permuted, bias_permuted 4 bytes: part of "supported"); x 16 bytes (the code given above); the
 * workspace 16 bytes (VPTQ_E_ALIGN); y and bias element-aligned. */
VPTQ_API size_t vptq_quant_gemm_gather_px_workspace_bytes(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm_gather_px_supported(const VptqLayerDesc* desc, int tokens);
VPTQ_API int vptq_quant_gemm_gather_px(const VptqLayerDesc* desc, const void* x, void* y, int tokens, int flags, void* workspace,
                                       size_t workspace_bytes, void* stream);
VPTQ_API int vptq_quant_gemm_gather_px_instance(const VptqLayerDesc* desc, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of SIBLING layers - layers applied to the same activations, q / k / v or gate / up - in one launch (the grouped
 * kernel of gemm_gather.hip; added within ABI 12; present when the symbols are).  descs[0 .. n) are 2 - 4 layers
 * vptq_quant_gemm_gather serves, of one dtype, one group_size and one residual codebook size; they may differ in out_features, in
 * every tensor, and in whether they have a column permutation.  gemm_gather_grouped_kernel<DT, T> walks the members' row groups of
 * 16 outputs as ONE list (member 0's, then member 1's, ...): a row group does not depend on the grid, so y[m] is BIT-IDENTICAL to what
 * member m's own entry gives for the same descriptor and x - vptq_quant_gemm_gather_px for a member with a permutation,
 * vptq_quant_gemm_gather for one without - and carries its guarantees.  Members with a permutation are read in the form without one
 * (scale_permuted, bias_permuted) over xp = x[perm] in the workspace, written by one permute_x_tokens launch per DISTINCT perm
 * pointer: members whose `perm` pointers are equal share one xp.  All launches go to `stream`; nothing is allocated: graph-capturable.
 *   x [tokens][in_features] (one x for every member), y[m] [tokens][descs[m].out_features], the members' dtype; flags:
 *   VPTQ_GEMV_OUT_F32 stores the fp32 sums (every y[m] is float32); every other flag is accepted and changes nothing.
 * vptq_quant_gemm_gather_grouped_supported: 1 where 2 <= n <= 4, 1 <= tokens <= 16, vptq_quant_gemm_gather_supported answers 1 for
 *   every member and the members share dtype, group_size and num_res_centroids, else 0; host logic.
 * vptq_quant_gemm_gather_grouped_workspace_bytes: k blocks of tokens * group_size * 2 rounded up to 256, k the number of distinct
 *   non-NULL perm pointers among the members; 0 where no member has a permutation and where `_supported` answers 0.
 * vptq_quant_gemm_gather_grouped: NULL descs / x / y VPTQ_E_NULL; tokens outside [1, 16] VPTQ_E_TOKENS; n outside [2, 4] or a group
 *   it does not serve VPTQ_E_UNSUPPORTED (vptq_last_error names the first member that rules it out and why); a NULL y[m] VPTQ_E_NULL;
 *   an x that is not 16-byte aligned VPTQ_E_UNSUPPORTED; then, where a member has a permutation, a NULL workspace or fewer
 *   workspace_bytes than the query answers VPTQ_E_WORKSPACE and a workspace that is not 16-byte aligned VPTQ_E_ALIGN; nothing is
 *   launched then.
 * vptq_quant_gemm_gather_grouped_instance: the launches as one line (host logic, without a device the CU count is taken as 256):
 *   permute_x_tokens g=N tok=N grid=XxY tpt=4 perms=K | <inner>      K distinct permutations: K such launches
 *   none | <inner>                                                  no member has a permutation
 *   <inner> = gemm_gather_grouped dt=f16|bf16 t=16|24|32 tok=N n=N groups=A+B[+C[+D]] tiles=N grid=N rgs=N
 *       groups the row groups (2 vector-rows) of every member, tiles the column tiles (1024 columns) per row group, grid the
 *       workgroups (at most 4 per CU), rgs the most row groups one workgroup walks.  Returns as vptq_quant_gemm_gather_instance does.
 * Workspace: contents do not matter before a call and are undefined after it; calls on one stream may share it.
 * Alignment: every member as vptq_quant_gemm_gather takes it (part of "supported"); x 16 bytes (VPTQ_E_UNSUPPORTED); the workspace 16
 * bytes (VPTQ_E_ALIGN); every y[m] and bias element-aligned. */
VPTQ_API int vptq_quant_gemm_gather_grouped_supported(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API size_t vptq_quant_gemm_gather_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API int vptq_quant_gemm_gather_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags,
                                            void* workspace, size_t workspace_bytes, void* stream);
VPTQ_API int vptq_quant_gemm_gather_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of SIBLING layers of the CANONICAL format (v = 8, 256 + 256 centroids) in one launch (gemm_k256_grouped_kernel in
 * gemm_k256.hip; added within ABI 12; present when the symbols are).  descs[0 .. n) are 2 - 4 layers vptq_quant_gemm_k256w serves, of
 * one dtype and one group_size; they may differ in out_features, in every tensor, and in whether they have a column permutation.
 * gemm_k256_grouped_kernel<DT, TB> (TB = 1 / 2 / 3 blocks of 16 tokens for 1 - 16 / 17 - 32 / 33 - 48 tokens) walks the members' row
 * groups of 32 outputs as ONE list (member 0's, then member 1's, ...) with one persistent workgroup per CU, which rebuilds its
 * codebook image when it moves on to the next member.  The order of every sum depends neither on the grid nor on the workgroup that
 * runs a row group, so y[m] is BIT-IDENTICAL to what member m's own entry gives for the same descriptor and x: vptq_quant_gemv with
 * VPTQ_GEMV_EXACT for 1 - 16 tokens (where vptq_quant_gemv_kernel_name says "gemm_k256_kernel"), vptq_quant_gemm_k256w for 17 - 48.
 * The entry has the reference's roundings only (w = r16(r16(r16(c + r) * s) + b), vptq_dequant's bits), like vptq_quant_gemm_k256w.
 * Members with a permutation are read in the form without one (scale_permuted, bias_permuted) over xp = x[perm] in the workspace,
 * written by one permute_x_tokens launch per DISTINCT perm pointer: members whose `perm` pointers are equal share one xp.  All launches
 * go to `stream`; nothing is allocated: graph-capturable.
 *   x [tokens][in_features] (one x for every member), y[m] [tokens][descs[m].out_features], the members' dtype; flags:
 *   VPTQ_GEMV_OUT_F32 stores the fp32 sums (every y[m] is float32); every other flag is accepted and changes nothing.
 * vptq_quant_gemm_k256_grouped_supported: 1 where 2 <= n <= 4, 1 <= tokens <= 48, every member is a valid layer of the canonical format
 *   as vptq_quant_gemm_k256w takes it (with perm: scale_permuted and bias_permuted) and the members share dtype and group_size, else 0;
 *   host logic.
 * vptq_quant_gemm_k256_grouped_workspace_bytes: k blocks of tokens * group_size * 2 rounded up to 256, k the number of distinct
 *   non-NULL perm pointers among the members; 0 where no member has a permutation and where `_supported` answers 0.
 * vptq_quant_gemm_k256_grouped: NULL descs / x / y VPTQ_E_NULL; tokens outside [1, 48] VPTQ_E_TOKENS; n outside [2, 4] or a group it
 *   does not serve VPTQ_E_UNSUPPORTED (vptq_last_error names the first member that rules it out and why); a NULL y[m] VPTQ_E_NULL; an x
 *   that is not 16-byte aligned VPTQ_E_UNSUPPORTED; then, where a member has a permutation, a NULL workspace or fewer workspace_bytes
 *   than the query answers VPTQ_E_WORKSPACE and a workspace that is not 16-byte aligned VPTQ_E_ALIGN; nothing is launched then.
 * vptq_quant_gemm_k256_grouped_instance: the launches as one line (host logic, without a device the CU count is taken as 256):
 *   permute_x_tokens g=N tok=N grid=XxY tpt=4 perms=K | <inner>      K distinct permutations: K such launches
 *   none | <inner>                                                  no member has a permutation
 *   <inner> = gemm_k256_grouped dt=f16|bf16 tok=N tb=1|2|3 n=N groups=A+B[+C[+D]] grid=N rgs=N passes=P
 *       groups the row groups (4 vector-rows) of every member, grid the workgroups (at most one per CU), rgs the most row groups one
 *       workgroup walks, passes every gemm_k256_pass any workgroup runs in any member: tb = 1 the row groups per pass, largest first
 *       ("4+2+1", "4+1", "1", ...), tb = 2 / 3 "1x2" / "1x3".  Returns as vptq_quant_gemm_gather_instance does.
 * Workspace: contents do not matter before a call and are undefined after it; calls on one stream may share it.
 * Alignment: every member as vptq_quant_gemm_k256w takes it (part of "supported"); x 16 bytes (VPTQ_E_UNSUPPORTED); the workspace 16
 * bytes (VPTQ_E_ALIGN); every y[m] and bias element-aligned. */
VPTQ_API int vptq_quant_gemm_k256_grouped_supported(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API size_t vptq_quant_gemm_k256_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API int vptq_quant_gemm_k256_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags,
                                          void* workspace, size_t workspace_bytes, void* stream);
VPTQ_API int vptq_quant_gemm_k256_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of SIBLING layers of the large-codebook formats for 17 - 48 tokens in one launch (gemm_gatherw_grouped_kernel in
 * gemm_gatherw_grouped.hip; added within ABI 12; present when the symbols are).  descs[0 .. n) are 2 - 4 layers vptq_quant_gemm_gatherw
 * serves, of one dtype, one group_size and one residual codebook size; they may differ in out_features, in every tensor, and in
 * whether they have a column permutation.  gemm_gatherw_grouped_kernel<DT, T, TB> (TB = 2 / 3 blocks of 16 tokens for 17 - 32 / 33 - 48
 * tokens) walks the members' row groups of 16 outputs as ONE list (member 0's, then member 1's, ...): a row group does not depend on
 * the grid, so y[m] is BIT-IDENTICAL to what member m's own entry gives for the same descriptor and x at the same token count -
 * vptq_quant_gemm_gather_px for a member with a permutation, vptq_quant_gemm_gatherw for one without - and carries its guarantees: a
 * token's bits are the 16-token kernel's in any slot of any batch.  Members with a permutation are read in the form without one
 * (scale_permuted, bias_permuted) over xp = x[perm] in the workspace, written by one permute_x_tokens launch per DISTINCT perm
 * pointer: members whose `perm` pointers are equal share one xp.  All launches go to `stream`; nothing is allocated: graph-capturable.
 *   x [tokens][in_features] (one x for every member), y[m] [tokens][descs[m].out_features], the members' dtype; flags:
 *   VPTQ_GEMV_OUT_F32 stores the fp32 sums (every y[m] is float32); every other flag is accepted and changes nothing.
 * vptq_quant_gemm_gatherw_grouped_supported: 1 where 2 <= n <= 4, 17 <= tokens <= 48, vptq_quant_gemm_gatherw_supported answers 1 for
 *   every member and the members share dtype, group_size and num_res_centroids, else 0; host logic.
 * vptq_quant_gemm_gatherw_grouped_workspace_bytes: k blocks of tokens * group_size * 2 rounded up to 256, k the number of distinct
 *   non-NULL perm pointers among the members; 0 where no member has a permutation and where `_supported` answers 0.
 * vptq_quant_gemm_gatherw_grouped: NULL descs / x / y VPTQ_E_NULL; tokens outside [17, 48] VPTQ_E_TOKENS; n outside [2, 4] or a group
 *   it does not serve VPTQ_E_UNSUPPORTED (vptq_last_error names the first member that rules it out and why); a NULL y[m] VPTQ_E_NULL;
 *   an x that is not 16-byte aligned VPTQ_E_TOKENS (vptq_quant_gemm_gatherw's code); then, where a member has a permutation, a NULL
 *   workspace or fewer workspace_bytes than the query answers VPTQ_E_WORKSPACE and a workspace that is not 16-byte aligned
 *   VPTQ_E_ALIGN; nothing is launched then.
 * vptq_quant_gemm_gatherw_grouped_instance: the launches as one line (host logic, without a device the CU count is taken as 256):
 *   permute_x_tokens g=N tok=N grid=XxY tpt=4 perms=K | <inner>      K distinct permutations: K such launches
 *   none | <inner>                                                  no member has a permutation
 *   <inner> = gemm_gatherw_grouped dt=f16|bf16 t=16|24|32 tok=N tb=2|3 n=N groups=A+B[+C[+D]] tiles=N grid=N rgs=N
 *       groups the row groups (2 vector-rows) of every member, tiles the column tiles (1024 columns) per row group, grid the
 *       workgroups (at most 4 per CU), rgs the most row groups one workgroup walks.  Returns as vptq_quant_gemm_gather_instance does.
 * Workspace: contents do not matter before a call and are undefined after it; calls on one stream may share it.
 * Alignment: every member as vptq_quant_gemm_gatherw takes it (part of "supported"); x 16 bytes (VPTQ_E_TOKENS); the workspace 16
 * bytes (VPTQ_E_ALIGN); every y[m] and bias element-aligned. */
VPTQ_API int vptq_quant_gemm_gatherw_grouped_supported(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API size_t vptq_quant_gemm_gatherw_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API int vptq_quant_gemm_gatherw_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags,
                                             void* workspace, size_t workspace_bytes, void* stream);
VPTQ_API int vptq_quant_gemm_gatherw_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes);

/* Batched decode of SIBLING layers of the large-codebook formats vptq_quant_gemm_gatherx serves (v = 8 / 16, 16384 ... 65536 main
 * centroids, any residual codebook: v16-k65536-65536 / -32768 / -1024 / -0, v8-k65536-4096, v8-k32768-0, ...) in one launch
 * (gemm_gatherx_grouped_kernel in gemm_gatherx_grouped.hip; added within ABI 12; present when the symbols are).  descs[0 .. n) are 2 - 4
 * layers vptq_quant_gemm_gatherx serves, of one dtype, one group_size and one format (vector_len, num_centroids, num_res_centroids);
 * they may differ in out_features, in every tensor, and in whether they have a column permutation.
 * gemm_gatherx_grouped_kernel<DT, V, RES> (RES: no residual table / table in LDS / table gathered from L2) walks the members' row
 * groups of 16 outputs as ONE list (member 0's, then member 1's, ...); a workgroup that moves on to the next member reloads its
 * pointers, scale and bias and (table in LDS) stages its residual table.  A row group depends neither on the grid nor on the
 * workgroup that runs it, so y[m] is BIT-IDENTICAL to what member m's own entry gives for the same descriptor and x -
 * vptq_quant_gemm_gather_px for a member with a permutation, vptq_quant_gemm_gatherx for one without - and carries its guarantees.
 * The entry has the reference's roundings only, like vptq_quant_gemm_gatherx.  Members with a permutation are read in the form
 * without one (scale_permuted, bias_permuted) over xp = x[perm] in the workspace, written by one permute_x_tokens launch per DISTINCT
 * perm pointer: members whose `perm` pointers are equal share one xp.  All launches go to `stream`; nothing is allocated, no atomics:
 * graph-capturable.
 *   x [tokens][in_features] (one x for every member), y[m] [tokens][descs[m].out_features], the members' dtype; flags:
 *   VPTQ_GEMV_OUT_F32 stores the fp32 sums (every y[m] is float32); every other flag is accepted and changes nothing.
 * vptq_quant_gemm_gatherx_grouped_supported: 1 where 2 <= n <= 4, 1 <= tokens <= 16, vptq_quant_gemm_gatherx_supported answers 1 for
 *   every member and the members share dtype, group_size, vector_len, num_centroids and num_res_centroids, else 0; host logic.
 * vptq_quant_gemm_gatherx_grouped_workspace_bytes: k blocks of tokens * group_size * 2 rounded up to 256, k the number of distinct
 *   non-NULL perm pointers among the members; 0 where no member has a permutation and where `_supported` answers 0.
 * vptq_quant_gemm_gatherx_grouped: NULL descs / x / y VPTQ_E_NULL; tokens outside [1, 16] VPTQ_E_TOKENS; n outside [2, 4] or a group
 *   it does not serve VPTQ_E_UNSUPPORTED (vptq_last_error names the first member that rules it out and why); a NULL y[m] VPTQ_E_NULL;
 *   an x that is not 16-byte aligned VPTQ_E_UNSUPPORTED; then, where a member has a permutation, a NULL workspace or fewer
 *   workspace_bytes than the query answers VPTQ_E_WORKSPACE and a workspace that is not 16-byte aligned VPTQ_E_ALIGN; nothing is
 *   launched then.
 * vptq_quant_gemm_gatherx_grouped_instance: the launches as one line (host logic, without a device the CU count is taken as 256):
 *   permute_x_tokens g=N tok=N grid=XxY tpt=4 perms=K | <inner>      K distinct permutations: K such launches
 *   none | <inner>                                                  no member has a permutation
 *   <inner> = gemm_gatherx_grouped dt=f16|bf16 v=8|16 ib=N rb=N res=none|lds|l2 tok=N n=N groups=A+B[+C[+D]] tiles=N wgcu=N grid=N rgs=N
 *       ib / rb the main / residual index widths, groups the row groups (16 outputs: one vector-row of v = 16, two of v = 8) of
 *       every member, tiles the column tiles (1024 columns) per row group, wgcu the workgroups per CU the LDS need leaves (4 / 3 / 2 up
 *       to 40 / 48 / 64 KiB: the 32 KiB tile + a table in LDS), grid = min(total row groups, CUs * wgcu) the workgroups, rgs the most
 *       row groups one workgroup walks.  Returns as vptq_quant_gemm_gather_instance does.
 * Workspace: contents do not matter before a call and are undefined after it; calls on one stream may share it.
 * Alignment: every member as vptq_quant_gemm_gatherx takes it (part of "supported"); x 16 bytes (VPTQ_E_UNSUPPORTED); the workspace 16
 * bytes (VPTQ_E_ALIGN); every y[m] and bias element-aligned. */
VPTQ_API int vptq_quant_gemm_gatherx_grouped_supported(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API size_t vptq_quant_gemm_gatherx_grouped_workspace_bytes(const VptqLayerDesc* descs, int n, int tokens);
VPTQ_API int vptq_quant_gemm_gatherx_grouped(const VptqLayerDesc* descs, int n, const void* x, void* const* y, int tokens, int flags,
                                             void* workspace, size_t workspace_bytes, void* stream);
VPTQ_API int vptq_quant_gemm_gatherx_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf, size_t bytes);

/* W[O, I] dense, row-major, desc->dtype: the reference CPU path's bits.
 * Alignment: indices and codebooks 4 bytes; everything else - W included - element-aligned.  16-byte aligned W, weight_scale /
 * weight_bias and indices let the kernel store, read the norm tensors and read the index stream in 16-byte pieces (store= / norm= / idx=
 * of vptq_dequant_instance); the bits written do not depend on it. */
VPTQ_API int vptq_dequant(const VptqLayerDesc* desc, void* W, void* stream);
/* Diagnostic (ABI 12): WHICH INSTANTIATION of dequant_kernel<DT, V, TAB> vptq_dequant(desc, W) would launch and which paths its
 * threads take, as one line of `dequant key=value ...` - the launcher's own decision and the kernel's own predicates, evaluated on
 * the host for the chunks of 8 columns of one vector-row.  Host logic: nothing is launched or dereferenced, no device is needed; W
 * is read for its alignment only.
 *   dequant dt=f16|bf16 v=2|4|6|8|10|12|16 tab=0|1|2 lds=N colblocks=N t=1..32 norm=vec|scalar|none store=vec|scalar
 *       idx=vec:N,win:N,win5:N,elem:N perm=0|1 outl=0|N groups=N ragged=0|1
 *       tab: both codebooks in LDS (1), the residual one only (2), neither (0); lds: bytes of LDS; colblocks: workgroups of 2048
 *       columns per vector-row; t: bits per index element; norm: scale / bias as 16-byte loads, element loads, or absent; store: 16-byte
 *       or element stores; idx: the chunks that read their 8 index elements as one 16-byte piece (vec), as two windows of 4 (win), the
 *       same with a fifth word (win5), element by element (elem) - classes with no chunk are left out; outl: the outlier codebook's
 *       vector length (0: no outlier columns); groups: codebook groups; ragged: in_features is no multiple of 8.
 * Returns VPTQ_OK, vptq_dequant's own validation error, or VPTQ_E_WORKSPACE when buf (bytes long, NUL included) is too small. */
VPTQ_API int vptq_dequant_instance(const VptqLayerDesc* desc, const void* W, char* buf, size_t bytes);

/* Alignment: every pointer element-aligned (gemv_v2).  The LDS-resident kernels (gemv_lds / gemv_lds_mfma fmt=v2*: v = 8, k <= 8192,
 * kr <= 512, in_features a multiple of 8) are taken where indices, centroids and res_centroids are 16-byte, res_indices 8-byte and x
 * 16-byte aligned (gemv_lds_mfma: scale_weights and scale_bias 16 bytes too); vptq_quant_gemv_v2_instance answers for such an x. */
VPTQ_API int vptq_quant_gemv_v2(const VptqV2Desc* desc, const void* x, void* y, int tokens,
                       int flags, void* stream);

/* name of the kernel vptq_quant_gemv would launch for (desc, tokens, flags);
 * static string, for tests / profiles.  NULL if unsupported. */
VPTQ_API const char* vptq_quant_gemv_kernel_name(const VptqLayerDesc* desc, int tokens, int flags);
/* same for vptq_quant_gemv_grouped (the kernel choice depends on the whole group); "per-layer"
 * when the group is not served by one launch */
VPTQ_API const char* vptq_quant_gemv_grouped_kernel_name(const VptqLayerDesc* descs, int n, int tokens,
                                                int flags);
/* Diagnostic (added within ABI 11; present when the symbols are): WHICH INSTANTIATION of that kernel the call would launch.  A
 * kernel name above is a family of separately compiled instantiations, picked by the layer's shape; these write the template
 * arguments and launch-shape facts the dispatch decided into buf as one line of `name key=value ...`, stable and parseable,
 * produced by the very host functions that pick the launch (nothing is decided twice).  Host logic: nothing is launched, no
 * device is needed (without one the CU count is taken as 256).  One launch per line item; a call served by several launches
 * joins them with " | " (a split grouped launch, the members of a group served one by one, launches of 32 chain layers).
 *   gemv_k256m dt=f16|bf16 ns=1..7 nst=0|1|2 perm=0|1 fast=0|1 tok=1|2|4 sb=0|1 entry=0|1 slots=1..4 units=N sel=0|1
 *       ns sweeps of 2048 columns, nst staging phases (0: the unstaged form beyond 14336 columns), tok token slots, sb scale and
 *       bias staged in LDS, entry 1 = the preloaded-argument entry (one layer, one token), slots partial-sum slots, units the most
 *       row groups (of 4 vector-rows) one workgroup walks, sel the selective corrections
 *   gemv_k256 dt= rows=1|2 tok=1|2|4 sw=1|2 perm= fast= entry=
 *   gemm_k256 dt= perm= tok=N passes=4+2+1      (the passes of 4 / 2 / 1 row groups the busiest workgroup runs)
 *   gemm_k256t dt= perm= tok=N sweeps=N rgs=N    (rgs: the most row groups one workgroup walks)
 *   gemv_k256c dt= dep=0|1 mode=folded|exact|selective layers=N sweeps=a,b,... perm=a,b,...   (per layer, in list order)
 *   gemv_gather dt= t=16|24|32 rows=1|2 tok=1|2|4|8 perm= wide=0|1
 *       <DT, T, ROWS, TOK, PERM, WIDE>: t the index width, rows vector-rows per workgroup, wide 8 elements per lane and piece
 *   gemv_gatherx dt= v=2|4|6|8|10|12|16 tok=1|2|4|8 perm= reslds=0|1 outl=0|same|4 groups=N
 *       <DT, V, TOK, PERM>, then the forks inside the kernel: the residual table gathered from LDS (<= 32 KiB) or from L2, outlier
 *       columns (none, a codebook of the layer's vector length, of length 4), codebook groups
 *   gemv_generic dt= v= tok=1|2|4|8
 *   gemv_lds dt= fmt=12|13|20|21|22|v2|v2u8|v2u16 tok=1|2|4 rw=1|2|4|8|16 dma=0|1 perm=
 *       <DT, FMT, TOK>: fmt the packed stream's index width or the v2 wire format (no / uint8 / uint16 residual ids); rw vector-rows
 *       per row group (by the CU count), dma the main table copied by LDS-DMA (k a multiple of 64) or through registers
 *   gemv_lds_mfma dt= fmt= rw=4|8|16 stages=1..4 dma= perm=      (stages: staging passes of 8192 columns)
 *   gemv_v2 dt= v=4|8|16 tok=1|2|4|8                             (vptq_quant_gemv_v2_instance only)
 * vptq_quant_gemv_chain_instance puts "grouped: " / "per-layer: " in front where the chain call hands the list to those.
 * tok: the token slots of the FIRST launch where a call is served in several.  vptq_quant_gemv_v2_instance answers for
 * vptq_quant_gemv_v2: a gemv_lds / gemv_lds_mfma line (fmt=v2*) or a gemv_v2 line.  Returns VPTQ_OK, the validation error of the call
 * itself, or VPTQ_E_WORKSPACE when buf (bytes long, NUL included) is too small. */
VPTQ_API int vptq_quant_gemv_instance(const VptqLayerDesc* desc, int tokens, int flags, char* buf, size_t bytes);
VPTQ_API int vptq_quant_gemv_grouped_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf,
                                              size_t bytes);
VPTQ_API int vptq_quant_gemv_chain_instance(const VptqLayerDesc* descs, int n, int tokens, int flags, char* buf,
                                            size_t bytes);
VPTQ_API int vptq_quant_gemv_v2_instance(const VptqV2Desc* desc, int tokens, int flags, char* buf, size_t bytes);
/* The same for the SLICED entries (added within ABI 11; present when the symbols are): which instantiation of gemv_sliced_kernel /
 * gemv_sliced_tok_kernel / gemv_hot_kernel a call over these layouts would launch.  descs, layouts, n, flags: as the call takes them
 * (VPTQ_GEMV_COLUMN_PARTS included); of the VptqSlicedLayout structs only the scalar fields and the pointers' being set and their
 * alignment are read - nothing is dereferenced, no device is needed.
 *   vptq_quant_gemv_sliced_instance: n == 1 without VPTQ_GEMV_COLUMN_PARTS answers for vptq_quant_gemv_sliced (VPTQ_GEMV_SELECTIVE:
 *       the pre-pass in front), else for vptq_quant_gemv_sliced_grouped - which launches the same for one layer, SELECTIVE read as
 *       EXACT; tokens must be 1.
 *   vptq_quant_gemv_sliced_tokens_instance: vptq_quant_gemv_sliced_tokens (n == 1 without column parts) / _tokens_grouped; 2 - 8
 *       tokens; a call that takes the one pass of the one-token kernel answers with that kernel's line.
 *   gemv_sliced dt=f16|bf16 nsl=8|16|32 res=0|1 v=8|16 two=0|1 ex=0|1 rg=0|1 tok=1|2|3 wpt=0|1 wparts=1|2|4 parts=1..3 n=1..3 rpw=N
 *       arrivals=N whole1=0|1 side=0|1|2 perm=0|1 corr=0|1
 *       the template arguments <DT, NSL, RES, V, TWO, EX, RG, TOK, WPT>, then the launch shape: window parts, column parts, group
 *       members, rows per wave, arrivals per accumulator word (slices x tables x column parts x window parts), the second table held
 *       whole, bytes per element of the residual side stream, any member with a permutation, the selective pre-pass's products added
 *   gemv_sliced_tok dt= nsl= res= v= two= tok=2|4|8 ex= phases=1|2|4 rpw=N regsums=0|1 n=1..3 whole1= perm=
 *       <DT, NSL, RES, V, TWO, TOK (token slots), EX>, column phases, rows per wave, the rows' sums in registers (else LDS), members,
 *       perm: the permute_x pre-pass runs
 *   gemv_hot dt= v=        the selective pre-pass, in front of the folded launch: "gemv_hot dt=f16 v=8 | gemv_sliced ... corr=1"
 * Returns VPTQ_OK, the call's own validation error (VPTQ_E_NULL, VPTQ_E_SHAPE for n, VPTQ_E_TOKENS, VPTQ_E_UNSUPPORTED, the layout
 * errors), or VPTQ_E_WORKSPACE when buf is too small. */
VPTQ_API int vptq_quant_gemv_sliced_instance(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, int tokens, int flags,
                                             char* buf, size_t bytes);
VPTQ_API int vptq_quant_gemv_sliced_tokens_instance(const VptqLayerDesc* descs, const VptqSlicedLayout* layouts, int n, int tokens,
                                                    int flags, char* buf, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* VPTQ_HIP_H */
