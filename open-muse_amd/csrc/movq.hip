// MoVQ tokenizer (muse/modeling_movq.py): SpatialNorm over NHWC as ONE apply pass.
//
//   new_f = GroupNorm(f) * conv_y(nearest(zq)) + conv_b(nearest(zq))        (reference modeling_movq.py:21-49)
//
// zq is the Z-channel quantised latent at [zh, zw]; nearest() brings it to the feature map's [H, W] (integer factors H / zh, W / zw),
// conv_y / conv_b are 1x1 convolutions Z -> C.  Per element that is a Z-term dot product per modulation tensor on top of the GroupNorm
// apply pass of vqgan.hip; built from separate ops, the two modulation tensors are written and read back at the activation's size.
// Here a thread keeps one 4-channel vector: its scale / shift and its 4 x (2Z + 2) modulation weights stay in registers, it strides over
// the pixels of its chunk (128 to 1024 pixels, so that a small batch still fills the chip; four pixels in flight), and fetches the pixel's
// zq row (<= 32 bytes, the same address for every lane of the pixel: one broadcast load per wave and pixel, served by the cache - a row
// is reused by factor^2 pixels).
// Statistics: the two-pass f64 scheme of vqgan.hip (same chunking, same fold -> the same mean / rstd floats), or a producer's partial sums.
#include "common.h"
#include "../../include/muse_hip.h"
#include <limits.h>

#define SN_PIX_PER_CHUNK 1024   // == GN_PIX_PER_CHUNK of vqgan.hip: muse_groupnorm_nchunk sizes `partial` for both

// n / d for a divisor that is usually a power of two (image sides and up-sampling factors): block-uniform branch, no division then
struct SnDiv { int d, shift; };
static inline SnDiv sn_div(int d) {
  SnDiv r = {d, -1};
  if (d > 0 && (d & (d - 1)) == 0) { r.shift = 0; while ((1 << r.shift) < d) ++r.shift; }
  return r;
}
__device__ __forceinline__ int sn_quot(int n, const SnDiv& v) { return v.shift >= 0 ? (n >> v.shift) : (n / v.d); }

// pass 1 (f32, four channels per thread): per (image, pixel chunk) sum / sum of squares per group in f64 -> partial [B, nchunk, G, 2]
__global__ __launch_bounds__(256) void sn_stats_kernel(const float* __restrict__ x, double* __restrict__ partial, int HW, int C, int G) {
  __shared__ double gs[64], gq[64];
  const int chunk = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
  if (threadIdx.x < G) { gs[threadIdx.x] = 0.0; gq[threadIdx.x] = 0.0; }
  __syncthreads();
  const int vpp = C / 4, cpg = C / G;
  const int p0 = chunk * SN_PIX_PER_CHUNK, p1 = min(HW, p0 + SN_PIX_PER_CHUNK);
  if (vpp <= 256) {
    const int vc = threadIdx.x % vpp, ppi = 256 / vpp;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + threadIdx.x / vpp; p < p1; p += ppi) {
      const f32x4 v = *(const f32x4*)(x + ((long)b * HW + p) * C + vc * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j] += (double)v[j]; q[j] += (double)v[j] * (double)v[j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = (vc * 4 + j) / cpg;
      atomicAdd(&gs[g], s[j]); atomicAdd(&gq[g], q[j]);
    }
  } else {  // more than 1024 channels: walk the channel vectors too
    for (int p = p0; p < p1; ++p)
      for (int v0 = threadIdx.x; v0 < vpp; v0 += 256) {
        const f32x4 v = *(const f32x4*)(x + ((long)b * HW + p) * C + v0 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int g = (v0 * 4 + j) / cpg;
          atomicAdd(&gs[g], (double)v[j]); atomicAdd(&gq[g], (double)v[j] * (double)v[j]);
        }
      }
  }
  __syncthreads();
  if (threadIdx.x < G) {
    double* o = partial + (((long)b * nchunk + chunk) * G + threadIdx.x) * 2;
    o[0] = gs[threadIdx.x]; o[1] = gq[threadIdx.x];
  }
}

// a zq row: whole 16-byte vectors when Z is a multiple of 4 (the entry point checks the pointer), single floats otherwise - a 12-byte
// row is never read with a 16-byte load (the last row would reach past the tensor)
template <int Z>
__device__ __forceinline__ void sn_load_zq(const float* __restrict__ p, float (&z)[Z]) {
  if constexpr (Z % 4 == 0) {
#pragma unroll
    for (int k = 0; k < Z; k += 4) {
      const f32x4 t = *(const f32x4*)(p + k);
      z[k] = t[0]; z[k + 1] = t[1]; z[k + 2] = t[2]; z[k + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < Z; ++k) z[k] = p[k];
  }
}

// one element: o = fma(fma(x, scale, shift), m, a), m = by + sum_k wy[k] zq[k], a = bb + sum_k wb[k] zq[k] (k ascending), then SiLU
template <int Z>
__device__ __forceinline__ float sn_element(float xv, float scale, float shift, const float* wy, float by, const float* wb, float bb,
                                            const float (&z)[Z], int silu, bool planes) {
  float m = by, a = bb;
#pragma unroll
  for (int k = 0; k < Z; ++k) { m = fmaf(wy[k], z[k], m); a = fmaf(wb[k], z[k], a); }
  float t = fmaf(fmaf(xv, scale, shift), m, a);
  // operand planes of the bf16x3 convolution: the hardware-reciprocal SiLU of the GroupNorm plane route (common.h gn_silu); the f32
  // tensor (the exact-f32 mode among its users) keeps the correctly rounded division
  if (silu) t = planes ? gn_silu(t) : t / (1.0f + __expf(-t));
  return t;
}

__device__ __forceinline__ void sn_store(float* __restrict__ y, bf16_t* __restrict__ y_hi, bf16_t* __restrict__ y_lo, long off,
                                         const float (&o)[4]) {
  if (y_hi) {
    u32x2 hi, lo;
    split4_values(o[0], o[1], o[2], o[3], hi, lo);
    *(u32x2*)(y_hi + off) = hi;
    *(u32x2*)(y_lo + off) = lo;
  } else {
    *(f32x4*)(y + off) = f32x4{o[0], o[1], o[2], o[3]};
  }
}

template <int Z>
__global__ __launch_bounds__(256) void sn_apply_kernel(const float* __restrict__ x, float* __restrict__ y, bf16_t* __restrict__ y_hi,
                                                       bf16_t* __restrict__ y_lo, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ zq,
                                                       const float* __restrict__ wy, const float* __restrict__ by,
                                                       const float* __restrict__ wb, const float* __restrict__ bb,
                                                       const double* __restrict__ partial, int HW, int C, int G, int nchunk, float eps,
                                                       int silu, int zw, int zhw, int apix, SnDiv dw, SnDiv dfy, SnDiv dfx) {
  __shared__ float sc[2048], sh[2048];
  __shared__ float gmean[64], grstd[64];
  __shared__ double gs_[64], gq_[64];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int cpg = C / G;
  {
    // fold the image's partials: 256 / G threads per group, each a strided subset in a fixed order, then a lane tree (the fold of
    // vqgan.hip's apply kernels: the same doubles in the same order)
    const int tpg = 256 / G, g = threadIdx.x / tpg, sub = threadIdx.x % tpg;
    double s = 0.0, q = 0.0;
    for (int c = sub; c < nchunk; c += tpg) {
      const double* o = partial + (((long)b * nchunk + c) * G + g) * 2;
      s += o[0]; q += o[1];
    }
    for (int o = 1; o < tpg; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
    if (sub == 0) { gs_[g] = s; gq_[g] = q; }
  }
  __syncthreads();
  if (threadIdx.x < G) {
    const double s = gs_[threadIdx.x], q = gq_[threadIdx.x];
    const double n = (double)HW * (double)cpg;
    const double mean = s / n;
    double var = q / n - mean * mean;
    if (var < 0.0) var = 0.0;
    gmean[threadIdx.x] = (float)mean;
    grstd[threadIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const int g = c / cpg;
    const float scale = grstd[g] * gamma[c];
    sc[c] = scale;
    sh[c] = beta[c] - scale * gmean[g];
  }
  __syncthreads();
  const int vpp = C / 4;
  const int p0 = chunk * apix, p1 = min(HW, p0 + apix);   // the apply pass's own chunk (`nchunk` counts the statistics' chunks)
  const float* zqb = zq + (long)b * zhw * Z;
  const bool planes = y_hi != nullptr;
  if (vpp <= 256) {
    const int vc = threadIdx.x % vpp, ppi = 256 / vpp;
    float scv[4], shv[4], wyv[4][Z], wbv[4][Z], byv[4], bbv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = vc * 4 + j;
      scv[j] = sc[c]; shv[j] = sh[c]; byv[j] = by[c]; bbv[j] = bb[c];
#pragma unroll
      for (int k = 0; k < Z; ++k) { wyv[j][k] = wy[(long)c * Z + k]; wbv[j][k] = wb[(long)c * Z + k]; }
    }
    constexpr int UN = 4;   // pixels in flight per thread, their loads issued together (see gn_apply_kernel)
    for (int pb = p0 + threadIdx.x / vpp; pb < p1; pb += UN * ppi) {
      f32x4 v[UN];
      float z[UN][Z];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int p = pb + u * ppi;
        if (p < p1) {
          v[u] = *(const f32x4*)(x + ((long)b * HW + p) * C + vc * 4);
          const int oy = sn_quot(p, dw), ox = p - oy * dw.d;
          sn_load_zq<Z>(zqb + ((long)sn_quot(oy, dfy) * zw + sn_quot(ox, dfx)) * Z, z[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int p = pb + u * ppi;
        if (p >= p1) break;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = sn_element<Z>(v[u][j], scv[j], shv[j], wyv[j], byv[j], wbv[j], bbv[j], z[u], silu, planes);
        sn_store(y, y_hi, y_lo, ((long)b * HW + p) * C + vc * 4, o);
      }
    }
  } else {
    // more than 1024 channels: a thread walks (pixel, channel vector) pairs and reads its weights where it needs them
    const long nv = (long)(p1 - p0) * vpp;
    for (long i = threadIdx.x; i < nv; i += 256) {
      const int p = p0 + (int)(i / vpp), vc = (int)(i % vpp);
      const long off = ((long)b * HW + p) * C + vc * 4;
      const f32x4 v = *(const f32x4*)(x + off);
      const int oy = sn_quot(p, dw), ox = p - oy * dw.d;
      float z[Z];
      sn_load_zq<Z>(zqb + ((long)sn_quot(oy, dfy) * zw + sn_quot(ox, dfx)) * Z, z);
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = vc * 4 + j;
        o[j] = sn_element<Z>(v[j], sc[c], sh[c], wy + (long)c * Z, by[c], wb + (long)c * Z, bb[c], z, silu, planes);
      }
      sn_store(y, y_hi, y_lo, off, o);
    }
  }
}

template <int Z>
static void sn_launch(dim3 grid, hipStream_t s, const float* x, float* y, void* y_hi, void* y_lo, const float* gamma, const float* beta,
                      const float* zq, const float* wy, const float* by, const float* wb, const float* bb, const double* partial, int HW,
                      int C, int G, int nchunk, float eps, int silu, int zw, int zhw, int apix, SnDiv dw, SnDiv dfy, SnDiv dfx) {
  hipLaunchKernelGGL(sn_apply_kernel<Z>, grid, dim3(256), 0, s, x, y, (bf16_t*)y_hi, (bf16_t*)y_lo, gamma, beta, zq, wy, by, wb, bb, partial,
                     HW, C, G, nchunk, eps, silu, zw, zhw, apix, dw, dfy, dfx);
}

extern "C" int muse_spatial_norm_nhwc(const float* x, float* y, void* y_hi, void* y_lo, const float* gamma, const float* beta,
                                      const float* zq, const float* wy, const float* by, const float* wb, const float* bb, double* partial,
                                      int32_t stats_nchunk, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t zh, int32_t zw, int32_t Z,
                                      int32_t groups, float eps, int32_t apply_silu, void* stream) {
  if ((groups != 32 && groups != 64) || C <= 0 || C > 2048 || (C % groups) || (C % 4)) return MUSE_ERR_UNSUPPORTED;
  const int vpp = C / 4;
  if (vpp <= 256 && (256 % vpp)) return MUSE_ERR_UNSUPPORTED;
  if (Z < 1 || Z > 8) return MUSE_ERR_UNSUPPORTED;
  if (H <= 0 || W <= 0 || zh <= 0 || zw <= 0 || (H % zh) || (W % zw) || stats_nchunk < 0) return MUSE_ERR_BAD_ARG;
  if ((y_hi == nullptr) != (y_lo == nullptr) || (y != nullptr) == (y_hi != nullptr)) return MUSE_ERR_BAD_ARG;   // exactly one output form
  if (!x || !gamma || !beta || !zq || !wy || !by || !wb || !bb || !partial) return MUSE_ERR_BAD_ARG;
  if ((long)H * W > INT_MAX || batch > 65535) return MUSE_ERR_UNSUPPORTED;
  if ((((uintptr_t)x) | ((uintptr_t)y)) & 15) return MUSE_ERR_ALIGN;
  if ((((uintptr_t)y_hi) | ((uintptr_t)y_lo)) & 7) return MUSE_ERR_ALIGN;
  if ((Z % 4) == 0 && (((uintptr_t)zq) & 15)) return MUSE_ERR_ALIGN;
  if (batch <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W, nchunk = muse_groupnorm_nchunk(HW);
  if (stats_nchunk == 0) hipLaunchKernelGGL(sn_stats_kernel, dim3(nchunk, batch), dim3(256), 0, s, x, partial, HW, C, groups);
  const int fold = stats_nchunk > 0 ? stats_nchunk : nchunk;
  // the apply pass cuts an image into chunks of its own: 1024 pixels when that gives every CU two workgroups, else halved down to 128.
  // Measured on the MI355X at batch 8, planes output, producer statistics: 128 x 128 x 256 in 128 chunks of 1024 pixels (half the CUs
  // idle) 1.9 TB/s, in 1024 chunks of 128 pixels 5.0 TB/s; 256 x 256 x 128 in 512 chunks of 1024 pixels 4.6 TB/s, in 2048 chunks of 256
  // pixels 3.9 TB/s (every workgroup folds the image's partial sums first - 256 producer chunks there - so smaller is not better)
  int cus = device_cus();
  if (cus <= 0) cus = 256;
  int apix = SN_PIX_PER_CHUNK;
  while (apix > 128 && (long)batch * ((HW + apix - 1) / apix) < 2L * cus) apix >>= 1;
  dim3 grid((HW + apix - 1) / apix, batch);
  const SnDiv dw = sn_div(W), dfy = sn_div(H / zh), dfx = sn_div(W / zw);
#define SN_CASE(ZZ) case ZZ: sn_launch<ZZ>(grid, s, x, y, y_hi, y_lo, gamma, beta, zq, wy, by, wb, bb, partial, HW, C, groups, fold, eps, \
                                            apply_silu, zw, zh * zw, apix, dw, dfy, dfx); break;
  switch (Z) { SN_CASE(1) SN_CASE(2) SN_CASE(3) SN_CASE(4) SN_CASE(5) SN_CASE(6) SN_CASE(7) SN_CASE(8) }
#undef SN_CASE
  return (int)hipGetLastError();
}
