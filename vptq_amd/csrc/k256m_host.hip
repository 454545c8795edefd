// The host side of the persistent MFMA kernel (gemv_k256m.hip): which launches it takes, how the workgroups are shared between the
// layers of a grouped launch, the decision for one launch and the launch itself.  No device code: compiled once, an edit to a rule
// here recompiles none of the kernel file's six parts.  The kernel is reached through the k256m_* dispatchers of k256.h only.
// (A unit of its own rather than a section of gemv_k256.hip: that file's 56 kernels would be rebuilt with every rule here.)
#include "common.h"
#include "kernels.h"
#include "k256.h"

namespace vptq {

// exact form with scale and bias staged in LDS (kSB in the kernel): bf16, and fp16 from 6 sweeps on
static bool sb_staged(bool f16, bool fast, int max_cols, int tok) {
  return !fast && (!f16 || max_cols > 5 * kMSweepCols || tok > 1 || VPTQ_K256M_SB_ALL);
}
// tok = token slots of the instantiation (1, 2 or 4)
bool gemv_k256m_supported(int tok, bool f16, bool fast, int max_cols, bool perm) {
  // (the fp16 exact form queues scale and bias with the index words up to 5 sweeps; 6 and 7 sweeps - and bf16 - stage them in LDS: kSB)
  // more columns than fit beside the image: unstaged variant (folded form, no permutation)
  if (max_cols > kMMaxCols && (!fast || perm || tok > 1)) return false;
  // several tokens: one staged copy of the activations per token slot (the reference's roundings: scale and bias staged as well)
  if (tok != 1 && !(tok == 2 || tok == 4)) return false;
  // ... in the reference's roundings (round 6): the 4-slot instantiations keep 32 accumulator registers and spill from 3 (fp16) /
  // 2 (bf16) sweeps on; two passes of the 2-slot kernel lose against the VALU kernel (tools/tokens_exact_check.py: 4096 x 14336
  // bf16 30.2 vs 26.7 us, 4096^2 17.8 vs 10.0)
  if (tok == 4 && !fast && max_cols > (f16 ? 2 : 1) * kMSweepCols) return false;
  if (lds_slots(tok, max_cols, sb_staged(f16, fast, max_cols, tok)) < 1) return false;
  return true;
}

int gemv_k256m_row_groups(int n_rows) { return (n_rows + kMRows - 1) / kMRows; }

// All layers of a grouped launch must have the same number of columns (checked by the
// caller, launch_gemv_k256).  Fills in K256Layer::wgs: one workgroup per CU, shared out
// between the layers in proportion to their row groups.
// Workgroups per layer of one launch: one workgroup per CU (the LDS holds one), shared out in proportion to the layers' row
// groups - and never more than `cus` in total: rounding every share up gave 3 x 86 = 258 workgroups for three equal layers
// (q / k / v of an MHA model), two of which waited for a CU to come free (round 6).  While the sum is too large, the layer that
// loses least - whose row groups per workgroup stay the lowest after giving one up - gives one up.
static void m_shares(const int* groups, int n, int cus, int* share) {
  long long total = 0;
  for (int i = 0; i < n; ++i) total += groups[i];
  long long sum = 0;
  for (int i = 0; i < n; ++i) {
    long long sh = total > cus ? ((long long)groups[i] * cus + total - 1) / total : groups[i];
    if (sh < 1) sh = 1;
    if (sh > groups[i]) sh = groups[i];
    share[i] = (int)sh;
    sum += sh;
  }
  while (sum > cus) {
    int best = -1, best_units = 0;
    for (int i = 0; i < n; ++i) {
      if (share[i] <= 1) continue;
      const int units = (groups[i] + share[i] - 2) / (share[i] - 1);   // row groups per workgroup with one workgroup less
      if (best < 0 || units < best_units || (units == best_units && share[i] > share[best])) { best = i; best_units = units; }
    }
    if (best < 0) break;   // (more layers than CUs: cannot happen with kMaxGroup layers)
    --share[best];
    --sum;
  }
}
static int m_cus() {
  static const int fw = tune_int("VPTQ_K256M_WGS", 0);  // tuning override of the CU count
  return fw > 0 ? fw : device_cus();
}
int gemv_k256m_launch_units(const int* n_rows, int n) {
  if (n < 1 || n > kMaxGroup) return 0;
  int groups[kMaxGroup], share[kMaxGroup], units = 0;
  for (int i = 0; i < n; ++i) groups[i] = gemv_k256m_row_groups(n_rows[i]);
  m_shares(groups, n, m_cus(), share);
  for (int i = 0; i < n; ++i) {
    const int u = (groups[i] + share[i] - 1) / share[i];
    units = u > units ? u : units;
  }
  return units;
}
// VPTQ_GEMV_SELECTIVE in this kernel: one token, fp16, staged activations, the folded instantiation; every workgroup's row groups
// must fit the corrections' LDS (kMSelRowGroups)
bool gemv_k256m_selective_ok(const int* n_rows, int n, bool f16, int tok, int max_cols, bool perm) {
  if (tok != 1 || max_cols > kMMaxCols || max_cols > kMSelMaxBlocks * 128 || !gemv_k256m_supported(1, f16, true, max_cols, perm)) return false;
  if (n > kMaxGroup) return false;
  int groups[kMaxGroup], share[kMaxGroup];
  for (int i = 0; i < n; ++i) groups[i] = gemv_k256m_row_groups(n_rows[i]);
  m_shares(groups, n, m_cus(), share);
  for (int i = 0; i < n; ++i)
    if ((groups[i] + share[i] - 1) / share[i] > kMSelRowGroups) return false;
  return true;
}

// The decision for one launch: which instantiation (launch_m_shape picks exactly it) and how the launch is shaped.  Host
// arithmetic and the CU-count look-up only.
K256MDecision gemv_k256m_decide(const int* n_rows, int n, int tok, bool f16, bool fast, int max_cols, bool perm, bool selective) {
  K256MDecision D = {};
  D.f16 = f16; D.fast = fast; D.perm = perm; D.selective = selective; D.tok = tok; D.max_cols = max_cols;
  if (n < 1 || n > kMaxGroup || !gemv_k256m_supported(tok, f16, fast, max_cols, perm)) return D;
  if (selective && !(fast && tok == 1 && max_cols <= kMMaxCols)) return D;
  const bool wide = max_cols > kMMaxCols;   // unstaged: column blocks of 2 sweeps
  D.ns = wide ? 2 : (max_cols + kMSweepCols - 1) / kMSweepCols;
  D.nst = wide ? 0 : D.ns <= 4 ? 1 : 2;
  D.sb = sb_staged(f16, fast, max_cols, tok);
  D.slots = lds_slots(tok, max_cols, D.sb);
  D.entry = tok == 1 && n == 1 ? 1 : 0;
  int groups[kMaxGroup];
  for (int i = 0; i < n; ++i) groups[i] = gemv_k256m_row_groups(n_rows[i]);
  m_shares(groups, n, m_cus(), D.share);
  for (int i = 0; i < n; ++i) {
    const int u = (groups[i] + D.share[i] - 1) / D.share[i];
    D.units = u > D.units ? u : D.units;
    D.gx = D.share[i] > D.gx ? D.share[i] : D.gx;
  }
  D.ok = D.ns >= 1 && D.ns <= 7 && D.slots >= 1;
  return D;
}

hipError_t launch_gemv_k256m(K256Params& P, const K256MDecision& D, hipStream_t st) {
  if (!D.ok || P.n_layers < 1 || P.n_layers > kMaxGroup) return hipErrorInvalidValue;
  for (int i = 0; i < P.n_layers; ++i) {
    P.layer[i].wgs = D.share[i];
    P.layer[i].slots = D.slots | (D.selective ? kMSelBit : 0);
  }
  if (D.tok != 1) {
    if (!D.fast) return D.f16 ? k256m_f16_tokens_exact(P, D, st) : k256m_bf16_tokens_exact(P, D, st);
    return D.f16 ? k256m_f16_tokens(P, D, st) : k256m_bf16_tokens(P, D, st);
  }
  if (!D.f16) return D.fast ? k256m_bf16(P, D, st) : k256m_bf16_exact(P, D, st);
  return D.fast ? k256m_f16_fast(P, D, st) : k256m_f16_exact(P, D, st);
}

}  // namespace vptq
