// Gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_, norm_type 2; the reference reaches it through
// accelerator.clip_grad_norm_, training/train_muse.py:758-759, training/train_maskgit_imagenet.py:435-436) and the per-parameter norms
// of log_grad_norm (training/train_muse.py:1309-1314), without a host round trip:
//   1. sum of squares per (parameter, 4096-element chunk counted from the parameter's own start) -> a slab of f64 partials, one plain
//      store per chunk: no floating-point atomics, so the slab does not depend on how the gradient is cut into calls or on their order;
//   2. finalize (one launch): the chunks of a parameter folded in chunk order, the parameters in parameter order, norm / coefficient /
//      scale / per-parameter norms written to device memory - the AdamW kernels read the scale from there (optim.hip, *_dev);
//   3. in-place scale of the gradients by a device-side factor, for loops that clip and then step in the reference's order.
// Squares and sums are f64: an f32 square is exact in f64 and the kernel streams 4 bytes per element, far from the f64 FMA rate.
#include "common.h"
#include "../../include/muse_hip.h"
#include <math.h>

#define GN_CHUNK 4096   // the chunk of opt_multi_kernel (OPT_CHUNK of optim.hip): FusedAdamW's chunk_first table serves both

// Sum of squares of g[0, cnt), cnt <= GN_CHUNK, by one workgroup of 256 -> *out.  Element i belongs to lane (i / 4) % 256, slot i % 4,
// whether it is read by a 16-byte load or (unaligned start, ragged end) alone: the partial is a function of the values only.
__device__ __forceinline__ void chunk_sumsq(const float* __restrict__ g, long cnt, double* __restrict__ out) {
  const bool vec = !(((uintptr_t)g) & 15);
  float x[GN_CHUNK / 1024][4];
#pragma unroll
  for (int r = 0; r < GN_CHUNK / 1024; ++r) {
    const long i = (long)(r * 256 + (int)threadIdx.x) * 4;
    if (vec && i + 3 < cnt) {
      const f32x4 t = *(const f32x4*)(g + i);
      x[r][0] = t[0]; x[r][1] = t[1]; x[r][2] = t[2]; x[r][3] = t[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[r][j] = i + j < cnt ? g[i + j] : 0.f;
    }
  }
  double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < GN_CHUNK / 1024; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = fma((double)x[r][j], (double)x[r][j], a[j]);
  }
  // (the xor butterfly adds the same pairs in every lane: a fixed tree)
  const double s = wave_sum_d((a[0] + a[1]) + (a[2] + a[3]));
  __shared__ double w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (w[0] + w[1]) + (w[2] + w[3]);
}

// Flat form: g is element 0 of the model's flat gradient buffer, ptab {offset, n} per parameter (absolute element offsets; the alignment
// padding between parameters belongs to nobody), chunk_first the exclusive prefix sum of ceil(n / 4096).  Block b owns chunk chunk0 + b,
// a chunk of one of the parameters [t0, t1).
__global__ __launch_bounds__(256) void gradnorm_flat_kernel(const float* __restrict__ g, const long* __restrict__ ptab,
                                                            const int* __restrict__ chunk_first, int t0, int t1, int chunk0,
                                                            double* __restrict__ slab) {
  const int id = chunk0 + (int)blockIdx.x;
  const int t = tensor_of_chunk(chunk_first, t0, t1, id);
  const long off = ptab[2 * t], n = ptab[2 * t + 1], s = (long)(id - chunk_first[t]) * GN_CHUNK;
  const long cnt = n - s < GN_CHUNK ? n - s : GN_CHUNK;
  chunk_sumsq(g + off + s, cnt, slab + id);
}

// Multi-tensor form over muse_adamw_multi's table (`ncol` x int64 per tensor, gradient pointer in column 1, n in column 5) and its
// chunk_first: block b owns chunk b.
__global__ __launch_bounds__(256) void gradnorm_multi_kernel(const long* __restrict__ table, int ncol, const int* __restrict__ chunk_first,
                                                             int nt, double* __restrict__ slab) {
  const int id = (int)blockIdx.x;
  const int t = tensor_of_chunk(chunk_first, 0, nt, id);
  const long* e = table + (long)t * ncol;
  const float* g = (const float*)e[1];
  const long n = e[5], s = (long)(id - chunk_first[t]) * GN_CHUNK;
  const long cnt = n - s < GN_CHUNK ? n - s : GN_CHUNK;
  chunk_sumsq(g + s, cnt, slab + id);
}

// out: [0] norm = grad_scale * sqrt(total) rounded once to f32, [1] coef = min(1, max_norm / (norm + 1e-6)) in f32 (torch's formula;
// a NaN norm gives a NaN coefficient as torch.clamp does), [2] scale = grad_scale * coef, [3 + t] grad_scale * sqrt(sum of parameter t).
// One workgroup per parameter: its partials are staged in LDS by all lanes (coalesced; a lane that folded them straight from memory
// paid one load latency per chunk, 240 us for config B's 1024-chunk matrices) and folded in chunk order by lane 0.  The workgroup that
// finishes last (an integer ticket in psum[nt]; zero before the first launch, left zero) folds the parameters in parameter order.
#define GN_TILE 2048
__device__ __forceinline__ double fold_in_order(const double* __restrict__ src, int n, double* __restrict__ sh, double s, bool coherent) {
  for (int b = 0; b < n; b += GN_TILE) {
    const int m = n - b < GN_TILE ? n - b : GN_TILE;
    for (int i = threadIdx.x; i < m; i += 256)
      sh[i] = coherent ? __hip_atomic_load(src + b + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : src[b + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) s += sh[i];
    __syncthreads();
  }
  return s;
}
__global__ __launch_bounds__(256) void gradnorm_finalize_kernel(const double* __restrict__ slab, const int* __restrict__ chunk_first, int nt,
                                                                double* psum, float grad_scale, float max_norm, float* __restrict__ out) {
  __shared__ double sh[GN_TILE];
  __shared__ int last;
  const int t = blockIdx.x;
  const int c0 = chunk_first[t];
  const double s = fold_in_order(slab + c0, chunk_first[t + 1] - c0, sh, 0.0, false);
  unsigned* ticket = (unsigned*)(psum + nt);
  if (threadIdx.x == 0) {
    out[3 + t] = (float)((double)grad_scale * sqrt(s));
    __hip_atomic_store(psum + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = atomicAdd(ticket, 1u) == (unsigned)nt - 1u;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  const double tot = fold_in_order(psum, nt, sh, 0.0, true);      // (written by the other workgroups: read past this CU's L1)
  if (threadIdx.x == 0) {
    const float norm = (float)((double)grad_scale * sqrt(tot));
    const float c = max_norm / (norm + 1e-6f);
    const float coef = c > 1.0f ? 1.0f : c;
    out[0] = norm;
    out[1] = coef;
    out[2] = grad_scale * coef;
    *ticket = 0u;
  }
}

__device__ __forceinline__ float scale1(float x, float s) {
#pragma clang fp contract(off)
  return x * s;
}
// g[0, n) *= *scale; block b owns elements [4096 b, 4096 b + 4096)
__device__ __forceinline__ void chunk_scale(float* __restrict__ g, long cnt, float s) {
  const bool vec = !(((uintptr_t)g) & 15);
  if (vec) {
    for (long i = threadIdx.x * 4; i + 3 < cnt; i += 1024) {
      f32x4 t = *(const f32x4*)(g + i);
      t[0] = scale1(t[0], s); t[1] = scale1(t[1], s); t[2] = scale1(t[2], s); t[3] = scale1(t[3], s);
      *(f32x4*)(g + i) = t;
    }
  }
  for (long i = (vec ? (cnt & ~3L) : 0) + threadIdx.x; i < cnt; i += 256) g[i] = scale1(g[i], s);
}
__global__ __launch_bounds__(256) void grad_scale_flat_kernel(float* __restrict__ g, long n, const float* __restrict__ scale) {
  const long c0 = (long)blockIdx.x * GN_CHUNK;
  chunk_scale(g + c0, n - c0 < GN_CHUNK ? n - c0 : GN_CHUNK, *scale);
}
__global__ __launch_bounds__(256) void grad_scale_multi_kernel(const long* __restrict__ table, int ncol, const int* __restrict__ chunk_first,
                                                               int nt, const float* __restrict__ scale) {
  const int id = (int)blockIdx.x;
  const int t = tensor_of_chunk(chunk_first, 0, nt, id);
  const long* e = table + (long)t * ncol;
  float* g = (float*)e[1];
  const long n = e[5], s = (long)(id - chunk_first[t]) * GN_CHUNK;
  chunk_scale(g + s, n - s < GN_CHUNK ? n - s : GN_CHUNK, *scale);
}

extern "C" int muse_gradnorm_flat(const float* g_flat, int64_t base, int64_t n, const int64_t* ptab_host, const int32_t* chunk_first_host,
                                  const int64_t* ptab, const int32_t* chunk_first, int32_t num_params, double* slab, void* stream) {
  if (n <= 0) return 0;
  if (!g_flat || !ptab_host || !chunk_first_host || !ptab || !chunk_first || !slab || num_params < 1 || base < 0) return MUSE_ERR_BAD_ARG;
  // the range must start at a parameter and end at the next one's start (or behind the last): a cut parameter is refused
  int t0 = 0, t1 = 0;
  while (t0 < num_params && ptab_host[2 * t0] < base) ++t0;
  if (t0 == num_params || ptab_host[2 * t0] != base) return MUSE_ERR_BAD_ARG;
  for (t1 = t0; t1 < num_params && ptab_host[2 * t1] < base + n; ++t1) {
    if (ptab_host[2 * t1 + 1] < 0 || chunk_first_host[t1 + 1] - chunk_first_host[t1] != (ptab_host[2 * t1 + 1] + GN_CHUNK - 1) / GN_CHUNK)
      return MUSE_ERR_BAD_ARG;
    if (t1 > t0 && ptab_host[2 * t1] < ptab_host[2 * (t1 - 1)] + ptab_host[2 * (t1 - 1) + 1]) return MUSE_ERR_BAD_ARG;
  }
  if (ptab_host[2 * (t1 - 1)] + ptab_host[2 * (t1 - 1) + 1] > base + n) return MUSE_ERR_BAD_ARG;
  const int chunk0 = chunk_first_host[t0], nchunks = chunk_first_host[t1] - chunk0;
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(gradnorm_flat_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, g_flat, (const long*)ptab, chunk_first,
                     t0, t1, chunk0, slab);
  return (int)hipGetLastError();
}

extern "C" int muse_gradnorm_multi(const int64_t* table, int32_t ncol, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                   double* slab, void* stream) {
  if (num_tensors <= 0 || num_chunks <= 0) return 0;
  if (!table || !chunk_first || !slab || ncol < 6) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(gradnorm_multi_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, ncol, chunk_first,
                     num_tensors, slab);
  return (int)hipGetLastError();
}

extern "C" int muse_gradnorm_finalize(const double* slab, const int32_t* chunk_first, int32_t num_tensors, double* psum, float grad_scale,
                                      float max_norm, float* out, void* stream) {
  if (num_tensors <= 0 || !slab || !chunk_first || !psum || !out) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(gradnorm_finalize_kernel, dim3((unsigned)num_tensors), dim3(256), 0, (hipStream_t)stream, slab, chunk_first, num_tensors, psum, grad_scale,
                     max_norm, out);
  return (int)hipGetLastError();
}

extern "C" int muse_grad_scale_flat(float* g, int64_t n, const float* scale, void* stream) {
  if (n <= 0) return 0;
  if (!g || !scale) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_scale_flat_kernel, dim3((unsigned)((n + GN_CHUNK - 1) / GN_CHUNK)), dim3(256), 0, (hipStream_t)stream, g, (long)n, scale);
  return (int)hipGetLastError();
}

extern "C" int muse_grad_scale_multi(const int64_t* table, int32_t ncol, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                     const float* scale, void* stream) {
  if (num_tensors <= 0 || num_chunks <= 0) return 0;
  if (!table || !chunk_first || !scale || ncol < 6) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_scale_multi_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, ncol, chunk_first,
                     num_tensors, scale);
  return (int)hipGetLastError();
}
