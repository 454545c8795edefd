// Host-side check of gemm_gatherx_eligible / gemm_gatherx_decide (vptq_amd/csrc/gemm_gatherx.hip) as a stand-alone program: sweeps
// descriptors (formats x shapes x alignments x token counts; nothing is dereferenced, nothing is launched) and checks every decision
// against the invariants the launcher relies on.  Meant for a host sanitizer build - no device is needed (the CU count is then 256):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/gemm_gatherx_host_check.cpp vptq_amd/csrc/gemm_gatherx.hip vptq_amd/csrc/gemm_gather.hip vptq_amd/csrc/gemv_gather.hip \
//       -o build/gemm_gatherx_host_check && build/gemm_gatherx_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../vptq_amd/csrc/kernels.h"

static int ilog2i(int n) { int b = 0; while ((1 << b) < n) ++b; return b; }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s (v=%d k=%d kr=%d I=%d O=%d tokens=%d)\n", __LINE__, #c, d.vector_len, \
                                               d.num_centroids, d.num_res_centroids, d.in_features, d.out_features, tokens); return 1; } } while (0)

int main() {
  const int vs[] = {4, 8, 12, 16}, ks[] = {256, 8192, 16384, 32768, 65536}, krs[] = {0, 4, 64, 256, 1024, 2048, 4096, 32768, 65536};
  const int Is[] = {8, 64, 1016, 1024, 1032, 2312, 4100, 8192, 28672}, Os[] = {1, 4, 5, 16, 20, 36, 4096, 14336, 16 * 1027 - 12, 8 * 2051 - 4};
  long eligible = 0, decisions = 0, owned = 0;
  for (int v : vs) for (int k : ks) for (int kr : krs) for (int I : Is) for (int O : Os)
    for (int variant = 0; variant < 8; ++variant) for (int tokens = 0; tokens <= 17; ++tokens) {
      VptqLayerDesc d = {};
      d.in_features = I; d.out_features = O; d.vector_len = v; d.num_codebooks = 1; d.group_size = I;
      d.num_centroids = k; d.num_res_centroids = kr; d.index_bits = ilog2i(k); d.res_bits = kr ? ilog2i(kr) : 0;
      const int T = d.index_bits + d.res_bits;
      d.row_words = (int)(((long long)I * T + 31) / 32); d.num_indices = (O + v - 1) / v; d.dtype = variant & 1;
      d.indices = (const int32_t*)(uintptr_t)(1 << 20); d.centroids = (const void*)(uintptr_t)(2 << 20);
      d.res_centroids = kr ? (const void*)(uintptr_t)(3 << 20) : nullptr;
      d.weight_scale = (const void*)(uintptr_t)(4 << 20); d.weight_bias = (const void*)(uintptr_t)(5 << 20);
      if (variant & 2) { d.perm = (const uint16_t*)(uintptr_t)(6 << 20); d.scale_permuted = (const void*)(uintptr_t)(7 << 20); d.bias_permuted = (const void*)(uintptr_t)(8 << 20); }
      if (variant == 4) d.centroids = (const void*)((uintptr_t)(2 << 20) + 8);
      if (variant == 5) d.weight_scale = nullptr;
      if (variant == 6) d.row_words += 3;
      if (variant == 7) d.row_words -= 1;
      const bool e = vptq::gemm_gatherx_eligible(d, tokens), g = vptq::gemm_gather_eligible(d, tokens);
      CHECK(!(e && g));   // a layer has one batched-decode kernel
      owned += g;
      if (!e) continue;
      ++eligible;
      CHECK(T <= 32 && (v == 8 || v == 16) && k >= 16384 && tokens >= 1 && tokens <= 16 && I % 8 == 0 && variant != 4 && variant != 5 && variant != 7);
      const vptq::GemmGatherXDecision D = vptq::gemm_gatherx_decide(d, tokens);
      ++decisions;
      const int rows = 16 / v, res_bytes = kr * v * 2;
      CHECK(D.v == v && D.ib == d.index_bits && D.rb == d.res_bits && D.tok == tokens && D.f16 == (d.dtype == 0) && D.perm == (d.perm != nullptr));
      CHECK(D.res_bytes == res_bytes && D.res == (res_bytes == 0 ? 0 : res_bytes <= 32768 ? 1 : 2));
      CHECK(D.lds == 32768 + (D.res == 1 ? res_bytes : 0) && D.lds <= 65536);
      CHECK(D.wgcu >= 2 && D.wgcu <= 4 && D.wgcu * D.lds <= 160 * 1024);
      CHECK(D.tiles == (I + 1023) / 1024 && D.tiles >= 1);
      CHECK(D.n_groups == (d.num_indices + rows - 1) / rows && D.n_groups * 16 >= O);
      CHECK(D.grid >= 1 && D.grid <= D.n_groups);
      CHECK((long long)D.rgs * D.grid >= D.n_groups && (long long)(D.rgs - 1) * D.grid < D.n_groups);
    }
  std::printf("gemm_gatherx host check: %ld eligible descriptors, %ld decisions checked, %ld owned by gemm_gather, no violation\n", eligible,
              decisions, owned);
  return 0;
}
