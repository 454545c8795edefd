from vptq_amd.ops.quant_gemm import (dequant, fused_gemm_max_tokens, quant_gemm, quant_gemm_batched_launch, quant_gemm_flags, quant_gemm_fused,
                                     quant_gemm_gather, quant_gemm_gather_grouped, quant_gemm_gather_px, quant_gemm_gatherw, quant_gemm_gatherw_grouped, quant_gemm_gatherx, quant_gemm_gatherx_grouped, quant_gemm_k256_grouped, quant_gemm_k256w,
                                     quant_gemv_v2)

__all__ = ["dequant", "quant_gemm", "quant_gemv_v2"]
