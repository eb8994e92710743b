// 256 x 256 LDS-DMA GEMM: what both host sides (gemm.hip through gemm256_host.h, gemm_p.hip) need - the eligibility rule of the
// family, and the persistent kernel (gemm256p.h / gemm_p.hip) as seen from muse_gemm
#pragma once
#include "gemm_core.h"

// eligibility: bf16 operands; 16-byte aligned output rows; whole 16-byte chunks along the contiguous operand dimension;
// split-K only through the workspace (atomics stay with the 128^2 kernel)
template <typename TC>
static inline bool gemm256_ok(const GemmParams& p, int la, int lb) {
  constexpr int EPC = 16 / (int)sizeof(TC);
  if (p.split_k > 1 && p.split_stride == 0) return false;
  if (p.act != 0) return false;  // (GELU epilogue stays with the 128^2 kernel)
  if ((la == 0 || lb == 0) && (p.K % 8)) return false;
  if ((la == 1 && (p.M % 8)) || (lb == 1 && (p.N % 8))) return false;
  return (p.N % EPC) == 0 && (p.ldc % EPC) == 0 && ((((uintptr_t)p.C) & 15) == 0) && (p.sC0 % EPC) == 0 &&
         (p.sC1 % EPC) == 0 && (p.split_stride % EPC) == 0 &&
         (p.residual == nullptr || (((p.ldr % EPC) == 0) && ((((uintptr_t)p.residual) & 15) == 0)));
}

bool gemm256p_takes(const GemmParams& p, int la, int lb, int batch, bool f32_out);
// -1: no queue slot for this stream (the caller falls back to the launch-per-tile kernel); otherwise a hipError_t
// half_ops: the operands are IEEE half (muse_gemm dtype MUSE_F16; f32 output, both operands k-contiguous)
int launch_gemm256p(const GemmParams& p, int la, int lb, bool f32_out, hipStream_t stream, bool half_ops = false);
