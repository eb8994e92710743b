// Antialiased bilinear resize + crop (+ horizontal flip) of a ragged batch of packed uint8 HWC images into one [B, 3, R, R] f32 NCHW
// tensor, one launch per batch: the GPU stage scripts/pre_encode.py:449-489 runs per image in front of get_code (to(cuda), permute,
// div(255), TF.resize(BILINEAR, antialias=True), TF.center_crop, stack).  Value and memory contract: include/muse_hip.h.
//
// This file is built with -ffp-contract=off (csrc/Makefile): the weights must be ATen's f32 operation for operation
// (aten/src/ATen/native/cpu/UpSampleKernel.cpp, HelperInterpBase::_compute_indices_min_size_weights_aa with the bilinear aa_filter), and
// one contracted multiply-add in `scale * (i + 0.5) - support` moves a tap boundary.  The two accumulations use fmaf explicitly.
//
// Work shape.  One workgroup of 256 threads = one image x one tile of RS_TR output rows x RS_TC output columns; a thread owns one
// output column and RS_TR / 4 output rows of it.  The source rows the tile needs (ymin of its first row .. ymax of its last) are
// streamed in chunks of RS_SR rows, so neither the tap count nor the image size is capped by LDS:
//   1. horizontal pass: tmp[r][c][ox] = sum_j src[y0 + r][xmin(ox) + j][c] * wx_j, bytes read straight from the packed buffer (the
//      lanes of a wave read neighbouring bytes of one source row), through a 256-entry LDS table of f32(v) / 255;
//   2. the chunk's vertical weights wy[oy][r] (0 outside a row's taps) are written by one thread each;
//   3. vertical pass: out[oy][ox] += tmp[r][c][ox] * wy[oy][r] over the chunk's rows in ascending order, only inside the row's taps.
// Chunks ascend, so every sum runs from tap 0 upwards as ATen's does.  Stores: one f32 per lane, consecutive along x in each plane.
#include "common.h"
#include "../../include/muse_hip.h"

namespace rsz {

constexpr int RS_TR = 16;   // output rows per workgroup
constexpr int RS_TC = 64;   // output columns per workgroup (one wave wide)
constexpr int RS_SR = 16;   // source rows per streamed chunk
constexpr int RS_RPT = RS_TR / 4;   // output rows (and chunk rows) per thread: 4 waves share a tile

// one axis of ATen's antialias index / weight computation, every step one rounded f32 operation
struct Axis {
  float scale, support, inv;
  int in;
  __device__ __forceinline__ Axis(int in_, int out_) : in(in_) {
    scale = (float)in_ / (float)out_;
    support = scale >= 1.0f ? scale : 1.0f;
    inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
  }
  __device__ __forceinline__ float center(int i) const { return scale * ((float)i + 0.5f); }
  __device__ __forceinline__ int lo(float c) const { const int v = (int)((c - support) + 0.5f); return v > 0 ? v : 0; }
  __device__ __forceinline__ int hi(float c) const { const int v = (int)((c + support) + 0.5f); return v < in ? v : in; }
  // un-normalised weight of source index s for the output whose centre is c
  __device__ __forceinline__ float raw(int s, float c) const {
    const float w = 1.0f - fabsf((((float)s - c) + 0.5f) * inv);
    return w > 0.0f ? w : 0.0f;
  }
  __device__ __forceinline__ float total(int lo_, int hi_, float c) const {
    float t = 0.0f;
    for (int s = lo_; s < hi_; ++s) t = t + raw(s, c);
    return t;
  }
};

__global__ __launch_bounds__(256) void resize_crop_u8_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ table,
                                                             float* __restrict__ out, int R) {
  __shared__ float u8f[256];
  __shared__ float tmp[RS_SR][3][RS_TC];
  __shared__ float wyl[RS_TR][RS_SR];

  const int t = threadIdx.x, lane = t & 63, grp = t >> 6;
  const int b = blockIdx.z, oy0 = blockIdx.y * RS_TR, ox = blockIdx.x * RS_TC + lane;
  const int64_t* row = table + (long)b * 8;
  const uint8_t* img = packed + row[0];
  const int H = (int)row[1], W = (int)row[2], oh = (int)row[3], ow = (int)row[4], top = (int)row[5], left = (int)row[6];
  const bool flip = row[7] != 0;

  u8f[t] = (float)t / 255.0f;

  const Axis ax(W, ow), ay(H, oh);
  // this thread's column: output column ox shows window column R - 1 - ox when flipped
  const bool col_ok = ox < R;
  const float cx = ax.center(left + (col_ok ? (flip ? R - 1 - ox : ox) : 0));
  const int xlo = ax.lo(cx), xhi = col_ok ? ax.hi(cx) : xlo;
  const float xtot = ax.total(xlo, xhi, cx);

  // the tile's source rows, and the taps of this thread's output rows grp, grp + 4, ..
  const int oy_last = (oy0 + RS_TR < R ? oy0 + RS_TR : R) - 1;
  const int y_begin = ay.lo(ay.center(top + oy0)), y_end = ay.hi(ay.center(top + oy_last));
  int ylo[RS_RPT], yhi[RS_RPT];
  float acc[RS_RPT][3];
#pragma unroll
  for (int i = 0; i < RS_RPT; ++i) {
    const int oy = oy0 + grp + 4 * i;
    const float c = ay.center(top + (oy < R ? oy : oy_last));
    ylo[i] = ay.lo(c);
    yhi[i] = oy < R ? ay.hi(c) : ylo[i];
    acc[i][0] = acc[i][1] = acc[i][2] = 0.0f;
  }
  // the output row whose chunk weights this thread writes (step 2)
  const int wrow = t >> 4, wr = t & 15;
  const bool wrow_ok = oy0 + wrow < R;
  const float wc = ay.center(top + (wrow_ok ? oy0 + wrow : oy_last));
  const int wlo = ay.lo(wc), whi = wrow_ok ? ay.hi(wc) : wlo;
  const float wtot = ay.total(wlo, whi, wc);
  __syncthreads();

  for (int y0 = y_begin; y0 < y_end; y0 += RS_SR) {
    // 1. horizontal pass over chunk rows grp, grp + 4, .. (a wave shares one source row: its lanes read neighbouring bytes)
    float h[RS_RPT][3];
#pragma unroll
    for (int i = 0; i < RS_RPT; ++i) h[i][0] = h[i][1] = h[i][2] = 0.0f;
    for (int s = xlo; s < xhi; ++s) {
      const float w = ax.raw(s, cx) / xtot;
#pragma unroll
      for (int i = 0; i < RS_RPT; ++i) {
        const int y = y0 + grp + 4 * i;
        if (y < y_end) {
          const uint8_t* p = img + ((long)y * W + s) * 3;
          h[i][0] = fmaf(u8f[p[0]], w, h[i][0]);
          h[i][1] = fmaf(u8f[p[1]], w, h[i][1]);
          h[i][2] = fmaf(u8f[p[2]], w, h[i][2]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RS_RPT; ++i) {
      tmp[grp + 4 * i][0][lane] = h[i][0];
      tmp[grp + 4 * i][1][lane] = h[i][1];
      tmp[grp + 4 * i][2][lane] = h[i][2];
    }
    // 2. vertical weights of (output row wrow, chunk row wr)
    {
      const int y = y0 + wr;
      wyl[wrow][wr] = (y >= wlo && y < whi) ? ay.raw(y, wc) / wtot : 0.0f;
    }
    __syncthreads();
    // 3. vertical pass, chunk rows ascending
    const int nrow = y_end - y0 < RS_SR ? y_end - y0 : RS_SR;
    for (int r = 0; r < nrow; ++r) {
      const int y = y0 + r;
#pragma unroll
      for (int i = 0; i < RS_RPT; ++i) {
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
    const long plane = (long)R * R;
    float* o = out + (long)b * 3 * plane + ox;
#pragma unroll
    for (int i = 0; i < RS_RPT; ++i) {
      const int oy = oy0 + grp + 4 * i;
      if (oy < R) {
        o[(long)oy * R] = acc[i][0];
        o[plane + (long)oy * R] = acc[i][1];
        o[2 * plane + (long)oy * R] = acc[i][2];
      }
    }
  }
}

}  // namespace rsz

extern "C" int muse_resize_crop_u8(const void* packed, const void* table, void* out, int32_t B, int32_t R, void* stream) {
  if (B < 1 || R < 1 || !packed || !table || !out) return MUSE_ERR_BAD_ARG;
  if (((uintptr_t)table & 7) || ((uintptr_t)out & 3)) return MUSE_ERR_ALIGN;
  const long gx = ((long)R + rsz::RS_TC - 1) / rsz::RS_TC, gy = ((long)R + rsz::RS_TR - 1) / rsz::RS_TR;
  if (gy > 65535 || B > 65535) return MUSE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rsz::resize_crop_u8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)packed, (const int64_t*)table, (float*)out, R);
  return (int)hipGetLastError();
}
