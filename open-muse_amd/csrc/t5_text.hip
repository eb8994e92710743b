// T5 text encoder (transformers T5EncoderModel: the `type: "t5"` text encoder of the reference's configs, loaded at
// training/train_muse.py:341-343 and called every step at :651 as `text_encoder(ids)[0]`) - the kernels it needs beyond the transformer
// and CLIP ones:
//   1. fused BIDIRECTIONAL self-attention with an additive relative-position bias: the RelBias policy of the one-tile encoder attention,
//      which lives in csrc/attention_enc.hip.  No score scale (T5 folds it into its initialisation), no mask; the bias of (query i,
//      key j) is rel[head][j - i + S - 1].
//   2. bias + row softmax of materialised f32 score matrices (the exact-f32 mode at any length, both modes for 128 < S <= 512)
//   3. the gated tanh-GELU behind the packed wi_0 | wi_1 product
//   4. RMSNorm (T5LayerNorm) with a bf16 result: the f32 result is muse_norm_res_fwd mode 0 (csrc/uvit.hip)
//   5. rel[head][t] = relative_attention_bias.weight[bucket[t]][head], the bucket map computed on the host
#include "common.h"
#include "../../include/muse_hip.h"

namespace t5 {

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. bias + softmax of [mats][S][ld] f32 score matrices: row i of matrix z becomes softmax_j(x[i][j] + rel[z % heads][j - i + S - 1])
// over j < S, columns [S, ld) are written as 0.  One wave per row.  y (f32, may be NULL) may be x (no __restrict__ on the pair): column
// c of a row is read and written by lane c & 63 alone, its last read before its store.  yb (may be NULL): the same values rounded to
// bf16, same ld - the A operand of the second product of the bf16 mode.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bias_softmax_kernel(const float* x, float* y, bf16_t* __restrict__ yb, const float* __restrict__ rel,
                                                           long rows, int S, long ld, int heads) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long mat = row / S;
  const int i = (int)(row - mat * S);
  const float* xr = x + row * ld;
  const float* br = rel + (mat % heads) * (2 * S - 1) + (S - 1 - i);
  float m = -INFINITY;
  for (int c = lane; c < S; c += 64) m = fmaxf(m, xr[c] + br[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < S; c += 64) s += expf(xr[c] + br[c] - m);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int c = lane; c < (int)ld; c += 64) {
    const float v = c < S ? expf(xr[c] + br[c] - m) * inv : 0.f;
    if (y) y[row * ld + c] = v;
    if (yb) yb[row * ld + c] = f32_to_bf16(v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. y[r][c] = gelu_new(ab[r][c]) * ab[r][F + c]  (transformers NewGELUActivation on wi_0, times wi_1: T5 v1.1's "gated-gelu").  The
// expression is F.gelu(approximate="tanh")'s, operation for operation, in f32.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_tanh(float x) {
  const float x3 = x * x * x;
  const float inner = 0.79788456080286535588f * (x + 0.044715f * x3);     // sqrt(2 / pi)
  return 0.5f * x * (1.0f + tanhf(inner));
}

template <typename T>
__global__ __launch_bounds__(256) void gated_gelu_tanh_kernel(const T* __restrict__ ab, T* __restrict__ y, long rows, int F) {
  const long n = rows * F;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / F;
    const int c = (int)(i - r * F);
    const T* row = ab + r * 2 * F;
    const float g = gelu_tanh(Elem<T>::load(row + c));
    Elem<T>::store(y + i, g * Elem<T>::load(row + F + c));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. y = bf16(x * rsqrt(mean(x^2) + eps) * w), x f32 [rows, cols], one wave per row: the expressions of norm_res_fwd_kernel mode 0
// (csrc/uvit.hip), whose result is f32 only
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmsnorm_bf16_kernel(const float* __restrict__ x, const float* __restrict__ w, bf16_t* __restrict__ y,
                                                           long rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * cols;
  float q = 0.f;
  for (int c = lane; c < cols; c += 64) q = fmaf(xr[c], xr[c], q);
  const float rstd = rsqrtf(wave_sum(q) / (float)cols + eps);
  for (int c = lane; c < cols; c += 64) y[row * cols + c] = f32_to_bf16(xr[c] * rstd * w[c]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 5. rel[h][t] = table[bucket[t]][h]: table = relative_attention_bias.weight [buckets, heads], t = the signed distance j - i + S - 1
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rel_bias_gather_kernel(const float* __restrict__ table, const int64_t* __restrict__ bucket,
                                                              float* __restrict__ rel, int heads, int n, int buckets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= heads * n) return;
  const int h = i / n, t = i - h * n;
  const int64_t b = bucket[t];
  rel[i] = (b >= 0 && b < buckets) ? table[b * heads + h] : 0.f;
}

}  // namespace t5

extern "C" int muse_bias_softmax_fwd(const float* x, float* y, void* y_bf16, const float* rel, int64_t mats, int32_t heads, int32_t seq,
                                     int64_t ld, void* stream) {
  if (mats <= 0 || seq <= 0) return 0;
  if (!x || !rel || (!y && !y_bf16) || heads <= 0 || ld < seq) return MUSE_ERR_BAD_ARG;
  const long rows = (long)mats * seq;
  hipLaunchKernelGGL(t5::bias_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (bf16_t*)y_bf16, rel,
                     rows, seq, (long)ld, heads);
  return (int)hipGetLastError();
}

extern "C" int muse_gated_gelu_tanh(const void* ab, void* y, int32_t dtype, int64_t rows, int32_t cols, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!ab || !y || (dtype != MUSE_F32 && dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  const dim3 grid((unsigned)ew_grid((long)rows * cols));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(t5::gated_gelu_tanh_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)ab, (float*)y, (long)rows, cols);
  else hipLaunchKernelGGL(t5::gated_gelu_tanh_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)ab, (bf16_t*)y, (long)rows, cols);
  return (int)hipGetLastError();
}

extern "C" int muse_rmsnorm_bf16_fwd(const float* x, const float* w, void* y, int64_t rows, int32_t cols, float eps, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!x || !w || !y) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(t5::rmsnorm_bf16_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, w, (bf16_t*)y, (long)rows,
                     cols, eps);
  return (int)hipGetLastError();
}

extern "C" int muse_rel_bias_gather(const float* table, const int64_t* bucket, float* rel, int32_t heads, int32_t n, int32_t buckets,
                                    void* stream) {
  if (heads <= 0 || n <= 0) return 0;
  if (!table || !bucket || !rel || buckets <= 0) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(t5::rel_bias_gather_kernel, dim3((unsigned)((heads * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, bucket, rel,
                     heads, n, buckets);
  return (int)hipGetLastError();
}
