// Host side of the launch-per-tile 256 x 256 LDS-DMA GEMM (gemm256.h): the cost model that picks the tile, and the launchers.
// Included by the translation units that launch these kernels (gemm.hip, scripts/exp/gemm256g.hip): every g256:: kernel named here is
// instantiated where this header is included - the half-operand ones, named by the non-template launch_gemm256_f16, even where nothing
// is called (gemm_p.hip includes it for exactly that, see there).  Eligibility (gemm256_ok) is in gemm_p.h, which the persistent kernel's host side shares.
#pragma once
#include "gemm256.h"
#include "gemm_p.h"

// (Peeling the short ragged last row-tile of M = 16448 = 64 * 256 + 64 off to the 128 x 128 kernel was tried and measured: the
// extra launch costs more (~20 us) than the round it saves on [16448x768]x[6144x768]^T (14 us).)
// Pick the tile by estimated time (microseconds on MI355X, fitted to scripts/exp/gemm256g.hip and scripts/gemm_shapes.py):
//   256^2: one block per CU (256 slots); a round costs nk * 1.8 + 6        (K loop ~1000 TFLOP/s + prologue / epilogue)
//   128^2: 3 (k-contiguous x k-contiguous, one stage) or 2 blocks per CU; a round costs nk * 1.7 + 2.5 / nk * 1.25 + 2.5
// MUSE_GEMM256 = 0 never, 1 whenever eligible, 2 (default) by the estimate.
static inline bool gemm256_preferred(const GemmParams& p, int la, int lb, int batch, bool persistent = false) {
  const char* e = getenv("MUSE_GEMM256");  // read per call (cheap) so tests can force either kernel
  const int mode = e ? (e[0] - '0') : 2;
  if (mode == 0) return false;
  if (mode == 1) return true;
  if (p.K < 128 || p.M < 256 || p.N < 256) return false;
  const long sk = p.split_k > 1 ? p.split_k : 1;
  const long t128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128) * batch * sk;
  const long t256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256) * batch * sk;
  const double nk = (double)((p.K + 63) / 64) / (double)sk;
  const bool nn = la == 0 && lb == 0;
  const long slots128 = nn ? 768 : 512;
  // persistent form (gemm256p.h): tiles are handed out dynamically and a tile change costs neither prologue nor a staged epilogue -
  // rounds count fractionally beyond the first (MI355X: [16448x768]x[2048x768]^T 61.7 us against 70.5 us on the 128^2 kernel)
  const double rounds = persistent ? (t256 <= 256 ? 1.0 : (double)t256 / 256.0) : (double)((t256 + 255) / 256);
  const double cost256 = persistent ? rounds * (nk * 1.8 + 2.0) + 4.0 : rounds * (nk * 1.8 + 6.0);
  const double cost128 = (double)((t128 + slots128 - 1) / slots128) * (nk * (nn ? 1.7 : 1.25) + 2.5);
  return cost256 < cost128;
}

template <typename TC, int AL, int BL, int BKV, bool H = false>
static inline int launch_gemm256_lb(const GemmParams& p, int batch, hipStream_t stream) {
  const int ntm = (p.M + 255) / 256, ntn = (p.N + 255) / 256;
  constexpr int lds = BKV == 64 ? g256::LDS_BYTES : g256::LDS_BYTES32;
  auto kern = g256::kernel<TC, AL, BL, BKV, H>;
  set_max_dynamic_lds((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3(ntm * ntn, p.split_k > 1 ? p.split_k : 1, batch), dim3(512), lds, stream, p);
  return (int)hipGetLastError();
}
template <typename TC, int AL, int BL>
static inline int launch_gemm256_x3_l(const GemmParams& p, hipStream_t stream) {
  const int ntm = (p.M + 255) / 256, ntn = (p.N + 255) / 256;
  auto kern = g256::kernel_x3<TC, AL, BL>;
  set_max_dynamic_lds((const void*)kern, g256::LDS_BYTES_X3);
  hipLaunchKernelGGL(kern, dim3(ntm * ntn, p.split_k > 1 ? p.split_k : 1, 1), dim3(512), g256::LDS_BYTES_X3, stream, p);
  return (int)hipGetLastError();
}
template <typename TC>
static inline int launch_gemm256_x3(const GemmParams& p, int la, int lb, hipStream_t stream) {
  if (la == 0 && lb == 0) return launch_gemm256_x3_l<TC, 0, 0>(p, stream);
  if (la == 0 && lb == 1) return launch_gemm256_x3_l<TC, 0, 1>(p, stream);
  if (la == 1 && lb == 1) return launch_gemm256_x3_l<TC, 1, 1>(p, stream);
  return launch_gemm256_x3_l<TC, 1, 0>(p, stream);
}
// MUSE_G256_BK = 64 (default): two 64 KiB stages of 64-wide K-tiles; 32: five 32 KiB stages of 32-wide K-tiles.  Measured
// equal within 2-3 % (BK = 64 ahead: 574 vs 586 us on [16384x3072]x[6144x3072]^T): the LDS-DMA stream is throughput-bound
// (~28 B/clk per CU whatever the depth), so more tiles in flight buy nothing and twice the barriers cost a little.
template <typename TC, int AL, int BL>
static inline int launch_gemm256_l(const GemmParams& p, int batch, hipStream_t stream) {
  const char* e = getenv("MUSE_G256_BK");
  if (e && e[0] == '3') return launch_gemm256_lb<TC, AL, BL, 32>(p, batch, stream);
  return launch_gemm256_lb<TC, AL, BL, 64>(p, batch, stream);
}
template <typename TC>
static inline int launch_gemm256(const GemmParams& p, int la, int lb, int batch, hipStream_t stream) {
  if (la == 0 && lb == 0) return launch_gemm256_l<TC, 0, 0>(p, batch, stream);
  if (la == 0 && lb == 1) return launch_gemm256_l<TC, 0, 1>(p, batch, stream);
  if (la == 1 && lb == 1) return launch_gemm256_l<TC, 1, 1>(p, batch, stream);
  return launch_gemm256_l<TC, 1, 0>(p, batch, stream);
}

// half operands (muse_gemm with dtype MUSE_F16: the TF32-class product of the tape engines' "f16" compute mode): f32 output, the 64-wide
// K loop
static inline int launch_gemm256_f16(const GemmParams& p, int la, int lb, int batch, hipStream_t stream) {
  if (la == 0 && lb == 0) return launch_gemm256_lb<float, 0, 0, 64, true>(p, batch, stream);
  if (la == 0 && lb == 1) return launch_gemm256_lb<float, 0, 1, 64, true>(p, batch, stream);
  if (la == 1 && lb == 1) return launch_gemm256_lb<float, 1, 1, 64, true>(p, batch, stream);
  return launch_gemm256_lb<float, 1, 0, 64, true>(p, batch, stream);
}
