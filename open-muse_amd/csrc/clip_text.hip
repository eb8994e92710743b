// CLIP text tower (transformers CLIPTextModel / CLIPTextModelWithProjection: the `type: "clip"` text encoder of the reference's
// configs, called every step at training/train_muse.py:647-649) - the kernels it needs beyond the transformer ones:
//   1. fused CAUSAL self-attention (every published tower has 77 tokens): the Causal policy of the one-tile encoder attention, which
//      lives in csrc/attention_enc.hip
//   2. causal row softmax of materialised f32 score matrices (the exact-f32 mode, between two muse_gemm products)
//   3. bias + quick-GELU behind the FC1 product, LayerNorm WITH bias in one pass
//   4. the pooled ("EOS") position of every id row, on the device
#include "common.h"
#include "../../include/muse_hip.h"

namespace clip {

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. causal softmax of [mats][S][ld] score matrices: row i keeps columns 0..i, every other column of [0, ld) is written as 0.
// y may be x (no __restrict__ on the pair): column c of a row is read and written by lane c & 63 alone, its last read before its store.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void causal_softmax_kernel(const T* x, T* y, long rows, int S, long ld) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cols = (int)(row % S) + 1;
  const T* xr = x + row * ld;
  T* yr = y + row * ld;
  float m = -INFINITY;
  for (int c = lane; c < cols; c += 64) m = fmaxf(m, Elem<T>::load(xr + c));
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += expf(Elem<T>::load(xr + c) - m);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int c = lane; c < (int)ld; c += 64) {
    const float v = c < cols ? expf(Elem<T>::load(xr + c) - m) * inv : 0.f;
    Elem<T>::store(yr + c, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. y = v * sigmoid(1.702 v), v = x + b[col]  (transformers QuickGELUActivation behind CLIPMLP.fc1); y may be x (no __restrict__ on
// the pair)
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bias_quick_gelu_kernel(const T* x, const float* __restrict__ b, T* y, long n, int cols) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = Elem<T>::load(x + i) + b[i % cols];
    const float s = 1.0f / (1.0f + expf(-(1.702f * v)));
    Elem<T>::store(y + i, v * s);
  }
}

// LayerNorm with weight AND bias (nn.LayerNorm: CLIPEncoderLayer.layer_norm1 / 2, final_layer_norm), f32 in, one wave per row:
// mean, then the variance of the centred values, then (x - mean) * rstd * w + b in one pass over the row.  Everything is taken
// relative to the row's first element: d = x - x[0] is exact for a row whose values lie within a factor of two of each other, so a
// row with |mean| >> std (1e3 + N(0, 1)) keeps the digits an f32 mean of the raw values cannot hold (the mean alone would be off by
// up to ulp(1e3) / 2 = 3e-5 of the std); the centred value is d - mean(d).  A constant row gives d = 0 and the bias, exactly.
template <typename T>
__global__ __launch_bounds__(256) void layernorm_bias_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                             T* __restrict__ y, long rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * cols;
  const float x0 = xr[0];
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += xr[c] - x0;
  const float dmean = wave_sum(s) / (float)cols;   // mean - x0
  float q = 0.f;
  for (int c = lane; c < cols; c += 64) { const float t = (xr[c] - x0) - dmean; q = fmaf(t, t, q); }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)cols + eps);
  for (int c = lane; c < cols; c += 64) Elem<T>::store(y + row * cols + c, ((xr[c] - x0) - dmean) * rstd * w[c] + b[c]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. pooled position of every id row (transformers CLIPTextTransformer.forward): eos_token_id == 2 (the legacy rule) -> first position
// of the row maximum; else first position whose id is eos_token_id, 0 when there is none (what argmax of an all-zero row gives)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eos_index_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ idx, int64_t* __restrict__ flat,
                                                        int batch, int S, int64_t eos) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= batch) return;
  const int64_t* r = ids + (long)row * S;
  const bool legacy = eos == 2;
  int64_t best = INT64_MIN; int pos = 0x7fffffff;      // legacy: (largest id, first position); else: first match
  for (int c = lane; c < S; c += 64) {
    const int64_t v = r[c];
    if (legacy) { if (v > best) { best = v; pos = c; } }
    else if (v == eos && c < pos) pos = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t ov = __shfl_xor(best, o, 64); const int op = __shfl_xor(pos, o, 64);
    if (legacy) { if (ov > best || (ov == best && op < pos)) { best = ov; pos = op; } }
    else if (op < pos) pos = op;
  }
  if (lane == 0) {
    const int64_t at = pos == 0x7fffffff ? 0 : pos;
    idx[row] = at;
    if (flat) flat[row] = (int64_t)row * S + at;
  }
}

}  // namespace clip

extern "C" int muse_causal_softmax_fwd(const void* x, void* y, int32_t dtype, int64_t mats, int32_t seq, int64_t ld, void* stream) {
  if (mats <= 0 || seq <= 0) return 0;
  if (ld < seq || (dtype != MUSE_F32 && dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  const long rows = (long)mats * seq;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(clip::causal_softmax_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, (float*)y, rows, seq, (long)ld);
  else hipLaunchKernelGGL(clip::causal_softmax_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, rows, seq, (long)ld);
  return (int)hipGetLastError();
}

extern "C" int muse_bias_quick_gelu(const void* x, const float* bias, void* y, int32_t dtype, int64_t rows, int32_t cols, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (dtype != MUSE_F32 && dtype != MUSE_BF16) return MUSE_ERR_BAD_ARG;
  const long n = (long)rows * cols;
  const dim3 grid((unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(clip::bias_quick_gelu_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, bias, (float*)y, n, cols);
  else hipLaunchKernelGGL(clip::bias_quick_gelu_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, bias, (bf16_t*)y, n, cols);
  return (int)hipGetLastError();
}

extern "C" int muse_layernorm_bias_fwd(const float* x, const float* w, const float* b, void* y, int32_t y_dtype, int64_t rows, int32_t cols,
                                       float eps, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (y_dtype != MUSE_F32 && y_dtype != MUSE_BF16) return MUSE_ERR_BAD_ARG;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (y_dtype == MUSE_F32) hipLaunchKernelGGL(clip::layernorm_bias_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x, w, b, (float*)y, (long)rows, cols, eps);
  else hipLaunchKernelGGL(clip::layernorm_bias_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, x, w, b, (bf16_t*)y, (long)rows, cols, eps);
  return (int)hipGetLastError();
}

extern "C" int muse_eos_index(const int64_t* ids, int64_t* idx, int64_t* flat_idx, int32_t batch, int32_t seq, int64_t eos_token_id,
                              void* stream) {
  if (batch <= 0) return 0;
  if (seq <= 0) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(clip::eos_index_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, idx, flat_idx, batch, seq,
                     eos_token_id);
  return (int)hipGetLastError();
}
