// Paella VQ tokenizer (reference muse/modeling_paella_vq.py: `vq_model.type: "paella_vq"`) - the kernels it needs beyond the GEMM,
// LayerNorm and gather kernels the other tokenizers already use.  Forward only, f32, channels-last rows [B*H*W, C], C % 4 == 0.
//   1. the first half of ResBlock.forward (:141-142) in one pass over x:
//        y = x + g2 * (dwconv3x3_replicate(LN(x) * (1 + g0) + g1) + bias)
//      as a statistics pass ([pixels, 2] floats: mean, rstd) and an apply pass that normalises the nine neighbours in registers - the
//      normalised tensor never exists in memory
//   2. zero-padded KS x KS patch rows (KS 2 | 4, any stride / top-left pad): the operand that turns Conv2d(4, 2, 1) and the four
//      output phases of ConvTranspose2d(4, 2, 1) into plain products on muse_gemm
//   3. nearest codebook row for narrow codebooks (D <= 8): direct squared distances and the argmin in one kernel, no distance matrix
//   4. in_block (PixelUnshuffle(2) + 1x1 convolution 12 -> C, reading the NCHW image) and out_block (1x1 convolution C -> 12 +
//      PixelShuffle(2), writing the NCHW image) as direct kernels: 12 channels are no matrix-core problem
// Every element offset is computed in 64 bits; the int32 arguments are sides and channel counts, never products.
#include "common.h"
#include "../../include/muse_hip.h"

namespace paella {

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. LayerNorm statistics + modulated replicate-padded depthwise 3x3 + residual
// ---------------------------------------------------------------------------------------------------------------------------------
// G lanes per pixel (a power of two <= 64, >= C / 4 unless that exceeds 64; then a lane holds up to four vectors: C <= 1024).
// Two-pass variance on the registers (the biased variance of nn.LayerNorm), eps inside the square root.
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, float* __restrict__ stats, long rows, int C4, int G,
                                                       float eps) {
  const int sub = threadIdx.x & (G - 1);
  const long row = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
  const bool live = row < rows;
  f32x4 v[4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = sub + j * G;
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live && i < C4) v[j] = *(const f32x4*)(x + (row * C4 + i) * 4);
    s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  }
  for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float inv_c = 1.0f / (float)(C4 * 4);
  const float mean = s * inv_c;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (sub + j * G < C4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float d = v[j][k] - mean; q = fmaf(d, d, q); }
    }
  }
  for (int o = G >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  if (live && sub == 0) {
    stats[row * 2] = mean;
    stats[row * 2 + 1] = 1.0f / sqrtf(q * inv_c + eps);
  }
}

// one thread per (pixel, 4 channels); w9 is tap-major [9][C]; g = the block's gammas (device): g[0], g[1], g[2] are read here
__global__ __launch_bounds__(256) void mix_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ w9,
                                                  const float* __restrict__ bias, const float* __restrict__ g, float* __restrict__ y, int H,
                                                  int W, int C4, long n4) {
  const float ga = 1.0f + g[0], gb = g[1], g2 = g[2];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    const long p = i / C4;
    const int xx = (int)(p % W);
    const long r = p / W;
    const int yy = (int)(r % H);
    const long row0 = r - yy;                  // image * H
    f32x4 acc = *(const f32x4*)(bias + cv * 4);
    f32x4 xc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = min(max(yy + ky - 1, 0), H - 1);      // ReplicationPad2d(1): an out-of-range coordinate clamps to the border
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = min(max(xx + kx - 1, 0), W - 1);
        const long q = (row0 + iy) * W + ix;
        const float mean = stats[q * 2], rstd = stats[q * 2 + 1];
        const f32x4 v = *(const f32x4*)(x + (q * C4 + cv) * 4);
        const f32x4 wv = *(const f32x4*)(w9 + ((long)(ky * 3 + kx) * C4 + cv) * 4);
        if (ky == 1 && kx == 1) xc = v;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(fmaf((v[k] - mean) * rstd, ga, gb), wv[k], acc[k]);
      }
    }
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = fmaf(g2, acc[k], xc[k]);
    *(f32x4*)(y + i * 4) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. patch rows: y[(b, oy, ox)][(ky, kx, c)] = x[b, oy * stride - pad_top + ky, ox * stride - pad_left + kx, c], 0 outside the image
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C4, int KS,
                                                         int stride, int pt, int pl, int Ho, int Wo, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    long t = i / C4;
    const int kx = (int)(t % KS); t /= KS;
    const int ky = (int)(t % KS); t /= KS;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    const long iy = (long)oy * stride - pt + ky, ix = (long)ox * stride - pl + kx;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const f32x4*)(x + (((b * H + iy) * W + ix) * C4 + cv) * 4);
    *(f32x4*)(y + i * 4) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. nearest codebook row, D <= 8.  A workgroup owns 64 rows of z (one per lane, z in registers); the codebook streams through LDS in
// chunks of 32 KiB and wave s scans the s-th quarter of every chunk (all lanes of a wave read the same code: LDS broadcast).  The
// distance is the direct sum d = fma(t_k, t_k, d), t_k = z_k - e_k, ascending k from d = 0; columns >= D are zeros on both sides and
// add exact zeros.  A thread meets its codes in ascending order and replaces only on `<`; the four quarters are merged on
// (distance, index): the lowest index among equal distances wins, like torch.argmin.  A row of NaNs returns index 0.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void vq_small_kernel(const float* __restrict__ z, long ldz, const float* __restrict__ cb,
                                                       int64_t* __restrict__ idx, float* __restrict__ dist, long N, int D, int Kc) {
  constexpr int CH = 8192 / DP;
  __shared__ __attribute__((aligned(16))) float e[CH * DP];
  __shared__ float bd[4][64];
  __shared__ int bi[4][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 64 + lane;
  float zr[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) zr[k] = (row < N && k < D) ? z[row * ldz + k] : 0.f;
  float best = INFINITY;
  int besti = 0;
  for (int c0 = 0; c0 < Kc; c0 += CH) {
    const int nc = min(CH, Kc - c0);
    __syncthreads();
    for (int t = threadIdx.x; t < nc * DP; t += 256) {
      const int code = t / DP, k = t % DP;
      e[t] = k < D ? cb[(long)(c0 + code) * D + k] : 0.f;
    }
    __syncthreads();
    const int per = (nc + 3) >> 2, lo = sl * per, hi = min(lo + per, nc);
#pragma unroll 4
    for (int c = lo; c < hi; ++c) {
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < DP; ++k) { const float t = zr[k] - e[c * DP + k]; d = fmaf(t, t, d); }
      if (d < best) { best = d; besti = c0 + c; }
    }
  }
  bd[sl][lane] = best;
  bi[sl][lane] = besti;
  __syncthreads();
  if (sl == 0 && row < N) {
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      const float d = bd[s][lane];
      const int j = bi[s][lane];
      if (d < best || (d == best && j < besti)) { best = d; besti = j; }
    }
    idx[row] = besti;
    if (dist) dist[row] = best;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. in_block / out_block.  PixelUnshuffle(2) channel order: k = c * 4 + dy * 2 + dx (c = image channel).  w12 is [12][C] (k-major).
// ---------------------------------------------------------------------------------------------------------------------------------
// one thread per (low-resolution pixel, 4 output channels); img [B, 3, 2 H2, 2 W2] f32
__global__ __launch_bounds__(256) void in_block_kernel(const float* __restrict__ img, const float* __restrict__ w12, const float* __restrict__ bias,
                                                       float* __restrict__ y, int H2, int W2, int C4, long n4) {
  const long Wf = 2L * W2, plane = 4L * H2 * W2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    const long p = i / C4;
    const int ox = (int)(p % W2);
    const long r = p / W2;
    const int oy = (int)(r % H2);
    const long b = r / H2;
    f32x4 acc = *(const f32x4*)(bias + cv * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const float* src = img + (b * 3 + c) * plane + (2L * oy + dy) * Wf + 2L * ox;
        const float u0 = src[0], u1 = src[1];
        const int k = c * 4 + dy * 2;
        const f32x4 w0 = *(const f32x4*)(w12 + ((long)k * C4 + cv) * 4), w1 = *(const f32x4*)(w12 + ((long)(k + 1) * C4 + cv) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(u1, w1[j], fmaf(u0, w0[j], acc[j]));
      }
    }
    *(f32x4*)(y + i * 4) = acc;
  }
}

// one thread per horizontal pair of image pixels (dx = 0, 1 of one low-resolution pixel): consecutive threads write consecutive 8 bytes
__global__ __launch_bounds__(256) void out_block_kernel(const float* __restrict__ x, const float* __restrict__ w12, const float* __restrict__ bias,
                                                        float* __restrict__ img, int H2, int W2, int C4, long n2) {
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n2; j += (long)gridDim.x * 256) {
    const int ox = (int)(j % W2);
    long t = j / W2;
    const int oy = (int)(t % (2 * H2)); t /= 2 * H2;
    const int c = (int)(t % 3);
    const long b = t / 3;
    const long p = (b * H2 + (oy >> 1)) * W2 + ox;
    const int k0 = c * 4 + (oy & 1) * 2;
    const float* xr = x + p * C4 * 4;
    const float* wa = w12 + (long)k0 * C4 * 4;
    const float* wb = wa + (long)C4 * 4;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < C4; ++v) {
      const f32x4 xv = *(const f32x4*)(xr + v * 4), w0 = *(const f32x4*)(wa + v * 4), w1 = *(const f32x4*)(wb + v * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { a0[k] = fmaf(xv[k], w0[k], a0[k]); a1[k] = fmaf(xv[k], w1[k], a1[k]); }
    }
    img[j * 2] = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + bias[k0];
    img[j * 2 + 1] = ((a1[0] + a1[1]) + (a1[2] + a1[3])) + bias[k0 + 1];
  }
}

static inline unsigned grid_for(long n) { const long g = (n + 255) / 256; return (unsigned)(g > 32768 ? 32768 : g); }
static inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) != 0;
}

}  // namespace paella

extern "C" int muse_paella_mix_fwd(const float* x, const float* w9, const float* bias, const float* gammas, float* stats, float* y,
                                   int32_t batch, int32_t H, int32_t W, int32_t C, void* stream) {
  if (batch < 0 || H <= 0 || W <= 0 || C <= 0) return MUSE_ERR_BAD_ARG;
  if (batch == 0) return 0;
  if (!x || !w9 || !bias || !gammas || !stats || !y || x == y) return MUSE_ERR_BAD_ARG;
  if ((C & 3) || C > 1024) return MUSE_ERR_UNSUPPORTED;
  if (paella::misaligned16(x, w9, bias, y) || (((uintptr_t)stats) & 7)) return MUSE_ERR_ALIGN;
  const long rows = (long)batch * H * W;
  const int C4 = C >> 2;
  int G = 1;
  while (G < C4 && G < 64) G <<= 1;
  const long sblocks = (rows + 256 / G - 1) / (256 / G);
  if (sblocks > 0x7fffffffL) return MUSE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(paella::ln_stats_kernel, dim3((unsigned)sblocks), dim3(256), 0, (hipStream_t)stream, x, stats, rows, C4, G, 1e-6f);
  MUSE_CHECK_LAUNCH();
  const long n4 = rows * C4;
  hipLaunchKernelGGL(paella::mix_kernel, dim3(paella::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x, (const float*)stats, w9, bias,
                     gammas, y, H, W, C4, n4);
  return (int)hipGetLastError();
}

extern "C" int muse_patch_rows_nhwc(const float* x, float* y, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t KS, int32_t stride,
                                    int32_t pad_top, int32_t pad_left, int32_t Hout, int32_t Wout, void* stream) {
  if (batch < 0 || H <= 0 || W <= 0 || C <= 0 || Hout <= 0 || Wout <= 0 || stride <= 0 || pad_top < 0 || pad_left < 0) return MUSE_ERR_BAD_ARG;
  if (batch == 0) return 0;
  if (!x || !y) return MUSE_ERR_BAD_ARG;
  if ((KS != 2 && KS != 4) || (C & 3)) return MUSE_ERR_UNSUPPORTED;
  if (paella::misaligned16(x, y)) return MUSE_ERR_ALIGN;
  const long n4 = (long)batch * Hout * Wout * KS * KS * (C >> 2);
  hipLaunchKernelGGL(paella::patch_rows_kernel, dim3(paella::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C >> 2, KS, stride,
                     pad_top, pad_left, Hout, Wout, n4);
  return (int)hipGetLastError();
}

extern "C" int muse_vq_nearest_small(const float* z, int64_t ldz, const float* codebook, int64_t* idx, float* dist, int64_t N, int32_t D,
                                     int32_t Kc, void* stream) {
  if (N < 0 || D <= 0 || Kc <= 0 || ldz < D) return MUSE_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!z || !codebook || !idx) return MUSE_ERR_BAD_ARG;
  if (D > 8) return MUSE_ERR_UNSUPPORTED;
  const long blocks = (N + 63) / 64;
  if (blocks > 0x7fffffffL) return MUSE_ERR_UNSUPPORTED;
  if (D <= 4) hipLaunchKernelGGL(paella::vq_small_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, (long)ldz, codebook, idx, dist, (long)N, D, Kc);
  else hipLaunchKernelGGL(paella::vq_small_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, (long)ldz, codebook, idx, dist, (long)N, D, Kc);
  return (int)hipGetLastError();
}

extern "C" int muse_paella_in_block(const float* img, const float* w12, const float* bias, float* y, int32_t batch, int32_t H, int32_t W,
                                    int32_t C, void* stream) {
  if (batch < 0 || H <= 0 || W <= 0 || C <= 0) return MUSE_ERR_BAD_ARG;
  if (batch == 0) return 0;
  if (!img || !w12 || !bias || !y) return MUSE_ERR_BAD_ARG;
  if (((H | W) & 1) || (C & 3)) return MUSE_ERR_UNSUPPORTED;
  if (paella::misaligned16(w12, bias, y) || (((uintptr_t)img) & 3)) return MUSE_ERR_ALIGN;
  const long n4 = (long)batch * (H >> 1) * (W >> 1) * (C >> 2);
  hipLaunchKernelGGL(paella::in_block_kernel, dim3(paella::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, img, w12, bias, y, H >> 1, W >> 1,
                     C >> 2, n4);
  return (int)hipGetLastError();
}

extern "C" int muse_paella_out_block(const float* x, const float* w12, const float* bias, float* img, int32_t batch, int32_t H, int32_t W,
                                     int32_t C, void* stream) {
  if (batch < 0 || H <= 0 || W <= 0 || C <= 0) return MUSE_ERR_BAD_ARG;
  if (batch == 0) return 0;
  if (!x || !w12 || !bias || !img) return MUSE_ERR_BAD_ARG;
  if (((H | W) & 1) || (C & 3)) return MUSE_ERR_UNSUPPORTED;
  if (paella::misaligned16(x, w12) || (((uintptr_t)img) & 3)) return MUSE_ERR_ALIGN;
  const long n2 = (long)batch * 3 * H * (W >> 1);
  hipLaunchKernelGGL(paella::out_block_kernel, dim3(paella::grid_for(n2)), dim3(256), 0, (hipStream_t)stream, x, w12, bias, img, H >> 1, W >> 1,
                     C >> 2, n2);
  return (int)hipGetLastError();
}
