// CLIP image tower (transformers CLIPVisionModelWithProjection / CLIPModel.get_image_features: the scorer of
// scripts/gen_sdxl_synthetic_dataset.py:34-36,98-105 and the "CLIP Score" of benchmark/model_quality.py:32-111) - the kernels a ViT
// needs beyond the transformer ones (the encoder layers run on muse_gemm, muse_attention_fwd_ex, muse_layernorm_bias_fwd and
// muse_bias_quick_gelu as they are):
//   1. antialiased bicubic resize of f32 NCHW images + (v - mean[c]) / std[c], both passes in one launch
//   2. non-overlapping P x P patches as the rows of a GEMM operand, K padded to a multiple of 8
//   3. class token / position embedding / pre-LayerNorm assembly in one pass
//   4. row-wise L2 normalisation with an optional multiplier (the two sides of the similarity product)
// All four are HBM-bound row / gather kernels.  Value and memory contracts: include/muse_hip.h.
//
// This file is built with -ffp-contract=off and IEEE division (csrc/Makefile): the resize weights follow ATen's antialias computation
// one rounded f32 operation at a time (aten/src/ATen/native/cpu/UpSampleKernel.cpp, _compute_indices_min_size_weights_aa with
// HelperInterpCubic::aa_filter), and the normalisation of an unresized image must be the bits of (x - mean) / std.  Accumulations use
// fmaf explicitly.
#include "common.h"
#include "../../include/muse_hip.h"

namespace clipv {

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. resize + normalise.  Work shape as csrc/resize.hip: one workgroup of 256 threads = one image x RV_TR output rows x RV_TC output
// columns; a thread owns one output column and RV_TR / 4 output rows of it, the source rows the tile needs are streamed in chunks of
// RV_SR rows (tap counts and image sizes are not bounded by LDS):
//   a. horizontal pass: tmp[r][c][ox] = sum_s src[c][y0 + r][s] * wx_s  (a wave shares one source row: its lanes read neighbouring floats)
//   b. the chunk's vertical weights wy[oy][r] (0 outside a row's taps), one thread each
//   c. vertical pass: acc[oy][ox] += tmp[r][c][ox] * wy[oy][r], chunk rows ascending
// then out = (acc - mean[c]) / std[c].  Nothing is clamped: the cubic's overshoot is kept, as ATen keeps it for float input.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int RV_TR = 16;
constexpr int RV_TC = 64;
constexpr int RV_SR = 16;
constexpr int RV_RPT = RV_TR / 4;

struct Norm3 { float mean[3], std[3]; };

// Keys' cubic convolution kernel with a = -0.5 (ATen cubic_convolution1 / cubic_convolution2)
__device__ __forceinline__ float cubic_aa(float x) {
  const float a = -0.5f;
  x = fabsf(x);
  if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return ((a * x - 5.0f * a) * x + 8.0f * a) * x - 4.0f * a;
  return 0.0f;
}

// one axis of ATen's antialias index / weight computation
struct Axis {
  float scale, support, inv;
  int in, max_taps;
  __device__ __forceinline__ Axis(int in_, int out_) : in(in_) {
    scale = (float)in_ / (float)out_;
    support = scale >= 1.0f ? 2.0f * scale : 2.0f;
    inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    max_taps = (int)ceilf(support) * 2 + 1;
  }
  __device__ __forceinline__ float center(int i) const { return scale * ((float)i + 0.5f); }
  __device__ __forceinline__ int lo(float c) const { const int v = (int)((c - support) + 0.5f); return v > 0 ? v : 0; }
  __device__ __forceinline__ int hi(float c) const {
    int v = (int)((c + support) + 0.5f);
    v = v < in ? v : in;
    const int cap = lo(c) + max_taps;
    return v < cap ? v : cap;
  }
  __device__ __forceinline__ float raw(int s, float c) const { return cubic_aa((((float)s - c) + 0.5f) * inv); }
  __device__ __forceinline__ float total(int lo_, int hi_, float c) const {
    float t = 0.0f;
    for (int s = lo_; s < hi_; ++s) t = t + raw(s, c);
    return t;
  }
};

__global__ __launch_bounds__(256) void resize_bicubic_norm_kernel(const float* __restrict__ x, float* __restrict__ out, int R, int I,
                                                                  const Norm3 nm) {
  __shared__ float tmp[RV_SR][3][RV_TC];
  __shared__ float wyl[RV_TR][RV_SR];

  const int t = threadIdx.x, lane = t & 63, grp = t >> 6;
  const int b = blockIdx.z, oy0 = blockIdx.y * RV_TR, ox = blockIdx.x * RV_TC + lane;
  const long splane = (long)R * R;
  const float* img = x + (long)b * 3 * splane;

  const Axis ax(R, I);      // both axes share one geometry (square to square)
  const bool col_ok = ox < I;
  const float cx = ax.center(col_ok ? ox : 0);
  const int xlo = ax.lo(cx), xhi = col_ok ? ax.hi(cx) : xlo;
  const float xtot = ax.total(xlo, xhi, cx);

  const int oy_last = (oy0 + RV_TR < I ? oy0 + RV_TR : I) - 1;
  const int y_begin = ax.lo(ax.center(oy0)), y_end = ax.hi(ax.center(oy_last));
  int ylo[RV_RPT], yhi[RV_RPT];
  float acc[RV_RPT][3];
#pragma unroll
  for (int i = 0; i < RV_RPT; ++i) {
    const int oy = oy0 + grp + 4 * i;
    const float c = ax.center(oy < I ? oy : oy_last);
    ylo[i] = ax.lo(c);
    yhi[i] = oy < I ? ax.hi(c) : ylo[i];
    acc[i][0] = acc[i][1] = acc[i][2] = 0.0f;
  }
  const int wrow = t >> 4, wr = t & 15;
  const bool wrow_ok = oy0 + wrow < I;
  const float wc = ax.center(wrow_ok ? oy0 + wrow : oy_last);
  const int wlo = ax.lo(wc), whi = wrow_ok ? ax.hi(wc) : wlo;
  const float wtot = ax.total(wlo, whi, wc);

  for (int y0 = y_begin; y0 < y_end; y0 += RV_SR) {
    float h[RV_RPT][3];
#pragma unroll
    for (int i = 0; i < RV_RPT; ++i) h[i][0] = h[i][1] = h[i][2] = 0.0f;
    for (int s = xlo; s < xhi; ++s) {
      const float w = ax.raw(s, cx) / xtot;
#pragma unroll
      for (int i = 0; i < RV_RPT; ++i) {
        const int y = y0 + grp + 4 * i;
        if (y < y_end) {                               // y < y_end <= R and s < xhi <= R: inside the plane
          const float* p = img + (long)y * R + s;
          h[i][0] = fmaf(p[0], w, h[i][0]);
          h[i][1] = fmaf(p[splane], w, h[i][1]);
          h[i][2] = fmaf(p[2 * splane], w, h[i][2]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RV_RPT; ++i) {
      tmp[grp + 4 * i][0][lane] = h[i][0];
      tmp[grp + 4 * i][1][lane] = h[i][1];
      tmp[grp + 4 * i][2][lane] = h[i][2];
    }
    {
      const int y = y0 + wr;
      wyl[wrow][wr] = (y >= wlo && y < whi) ? ax.raw(y, wc) / wtot : 0.0f;
    }
    __syncthreads();
    const int nrow = y_end - y0 < RV_SR ? y_end - y0 : RV_SR;
    for (int r = 0; r < nrow; ++r) {
      const int y = y0 + r;
#pragma unroll
      for (int i = 0; i < RV_RPT; ++i) {
        if (y >= ylo[i] && y < yhi[i]) {
          const float w = wyl[grp + 4 * i][r];
          acc[i][0] = fmaf(tmp[r][0][lane], w, acc[i][0]);
          acc[i][1] = fmaf(tmp[r][1][lane], w, acc[i][1]);
          acc[i][2] = fmaf(tmp[r][2][lane], w, acc[i][2]);
        }
      }
    }
    __syncthreads();
  }

  if (col_ok) {
    const long plane = (long)I * I;
    float* o = out + (long)b * 3 * plane + ox;
#pragma unroll
    for (int i = 0; i < RV_RPT; ++i) {
      const int oy = oy0 + grp + 4 * i;
      if (oy < I) {
        o[(long)oy * I] = (acc[i][0] - nm.mean[0]) / nm.std[0];
        o[plane + (long)oy * I] = (acc[i][1] - nm.mean[1]) / nm.std[1];
        o[2 * plane + (long)oy * I] = (acc[i][2] - nm.mean[2]) / nm.std[2];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. patch rows: y[(b, gy, gx)][(c, ky, kx)] = x[b][c][gy P + ky][gx P + kx], columns >= 3 P^2 = 0.  A thread writes four consecutive
// columns of one row with one vector store (Kp % 8 == 0: a group never straddles rows); consecutive lanes write consecutive groups and
// read runs of P consecutive floats.  A pure gather: the f32 path moves bits.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ x, T* __restrict__ y, long groups, int I, int P, int G,
                                                         int K, int Kp) {
  const int gpr = Kp >> 2;                             // groups of four columns per row
  const int PP = P * P;
  const long plane = (long)I * I;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    const long row = g / gpr;
    const int col0 = (int)(g - row * gpr) * 4;
    const long b = row / (G * G);
    const int cell = (int)(row - b * (G * G));
    const int gy = cell / G, gx = cell - gy * G;
    const float* base = x + b * 3 * plane + (long)(gy * P) * I + gx * P;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = col0 + e;
      float val = 0.0f;
      if (col < K) {
        const int c = col / PP, r = col - c * PP;
        const int ky = r / P, kx = r - ky * P;
        val = base[c * plane + (long)ky * I + kx];
      }
      v[e] = val;
    }
    V4<T>::store(y + row * Kp + col0, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. embeddings + pre-LayerNorm: row (b, t) = LN((t == 0 ? class : patch[b G^2 + t - 1]) + pos[t]) * w + bias.  One wave per row, the
// row lives in registers (H % 4 == 0, H <= 2048: up to eight 16-byte vectors per lane), so every operand is read once and the
// un-normalised encoder input never exists in memory.  Mean, then the variance of the centred values, as muse_layernorm_bias_fwd.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int EV_MAXV = 8;

__global__ __launch_bounds__(256) void vision_embed_ln_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y, long rows, int T, int H,
                                                              float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / T;
  const int t = (int)(row - b * T);
  const float* src = t == 0 ? cls : patch + (b * (T - 1) + (t - 1)) * (long)H;
  const float* pr = pos + (long)t * H;
  f32x4 v[EV_MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < EV_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < H) {
      const f32x4 a = *(const f32x4*)(src + c), p = *(const f32x4*)(pr + c);
      v[i] = f32x4{a[0] + p[0], a[1] + p[1], a[2] + p[2], a[3] + p[3]};
      s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
  }
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < EV_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; q = fmaf(d, d, q); }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
  for (int i = 0; i < EV_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      const f32x4 ww = *(const f32x4*)(w + c), bb = *(const f32x4*)(bias + c);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * ww[e] + bb[e];
      *(f32x4*)(y + row * H + c) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. y[r] = x[r] / ||x[r]||_2 (* mult) (* exp(*log_mult)), one wave per row.  No epsilon: a zero row is 0 / 0 = NaN, as
// x / x.norm(dim=-1, keepdim=True).  The second sweep over the row (<= a few KiB) is served by the cache: HBM sees the row once.
// y may be x (no __restrict__ on the pair): element c is read and written by lane c & 63 alone.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* x, float* y, long rows, int D, float mult, int has_mult,
                                                                const float* __restrict__ log_mult) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * D;
  float q = 0.f;
  for (int c = lane; c < D; c += 64) q = fmaf(xr[c], xr[c], q);
  const float norm = sqrtf(wave_sum(q));
  float m = mult;
  if (log_mult) m = m * expf(*log_mult);
  const bool scale = has_mult || log_mult != nullptr;
  for (int c = lane; c < D; c += 64) {
    const float u = xr[c] / norm;
    y[row * D + c] = scale ? u * m : u;
  }
}

}  // namespace clipv

extern "C" int muse_resize_bicubic_norm_f32(const float* x, float* out, int32_t B, int32_t R, int32_t I, const float* mean3,
                                            const float* std3, void* stream) {
  if (B < 1 || R < 1 || I < 1 || !x || !out || !mean3 || !std3) return MUSE_ERR_BAD_ARG;
  if (((uintptr_t)x | (uintptr_t)out) & 3) return MUSE_ERR_ALIGN;
  const long gx = ((long)I + clipv::RV_TC - 1) / clipv::RV_TC, gy = ((long)I + clipv::RV_TR - 1) / clipv::RV_TR;
  if (gy > 65535 || B > 65535 || R >= (1 << 24) || I >= (1 << 24)) return MUSE_ERR_UNSUPPORTED;
  clipv::Norm3 nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = mean3[c]; nm.std[c] = std3[c]; }      // host pointers: six floats by value
  hipLaunchKernelGGL(clipv::resize_bicubic_norm_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     x, out, R, I, nm);
  return (int)hipGetLastError();
}

extern "C" int muse_clip_patch_rows(const float* x, void* y, int32_t y_dtype, int32_t B, int32_t I, int32_t P, int32_t Kp, void* stream) {
  if (B < 1 || I < 1 || P < 1 || !x || !y || (y_dtype != MUSE_F32 && y_dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  if (I % P) return MUSE_ERR_BAD_ARG;
  const long K = 3L * P * P;
  if (K > (1L << 30) || Kp != (int32_t)((K + 7) & ~7L)) return MUSE_ERR_BAD_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)y & 15)) return MUSE_ERR_ALIGN;
  const int G = I / P;
  const long groups = (long)B * G * G * (Kp / 4);
  const long blocks = (groups + 255) / 256;
  const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks));
  if (y_dtype == MUSE_F32)
    hipLaunchKernelGGL(clipv::patch_rows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x, (float*)y, groups, I, P, G, (int)K, Kp);
  else
    hipLaunchKernelGGL(clipv::patch_rows_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, groups, I, P, G, (int)K, Kp);
  return (int)hipGetLastError();
}

extern "C" int muse_clip_vision_embed_ln(const float* patch, const float* class_embedding, const float* position_embedding, const float* w,
                                         const float* b, float* y, int32_t batch, int32_t tokens, int32_t hidden, float eps, void* stream) {
  if (batch <= 0) return 0;
  if (tokens < 1 || hidden < 1 || !class_embedding || !position_embedding || !w || !b || !y || (tokens > 1 && !patch)) return MUSE_ERR_BAD_ARG;
  if (hidden % 4 || hidden > 256 * clipv::EV_MAXV) return MUSE_ERR_UNSUPPORTED;
  if (((uintptr_t)patch | (uintptr_t)class_embedding | (uintptr_t)position_embedding | (uintptr_t)w | (uintptr_t)b | (uintptr_t)y) & 15)
    return MUSE_ERR_ALIGN;
  const long rows = (long)batch * tokens;
  hipLaunchKernelGGL(clipv::vision_embed_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, patch,
                     class_embedding, position_embedding, w, b, y, rows, tokens, hidden, eps);
  return (int)hipGetLastError();
}

extern "C" int muse_l2_normalize_rows(const float* x, float* y, int64_t rows, int32_t cols, float mult, int32_t has_mult,
                                      const float* log_mult, void* stream) {
  if (rows <= 0) return 0;
  if (cols < 1 || !x || !y) return MUSE_ERR_BAD_ARG;
  if ((rows + 3) / 4 > 0x7fffffffL) return MUSE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(clipv::l2_normalize_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (long)rows,
                     cols, mult, has_mult ? 1 : 0, log_mult);
  return (int)hipGetLastError();
}
