// Streaming first and second moments of f32 feature rows in f64, for the Frechet distance on CLIP image embeds (muse/frechet.py:
// FeatureStats.update).  One entry, one kernel, contract in include/muse_hip.h:
//   sum[i]      += sum_n (double)x[n][i]
//   outer[i][j] += sum_n (double)x[n][i] * (double)x[n][j]      for j >= i; the strict lower triangle is neither read nor written
// Every product of two converted f32 values is exact in f64 (24 + 24 significant bits < 53): only the additions round.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/muse_hip.h"

namespace moments {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 64;        // a workgroup owns one TILE x TILE tile of the upper triangle; wave w its rows [16 w, 16 w + 16)
constexpr int UN = 4;           // row groups (of four rows = one MFMA's K) whose loads are issued before the first of their MFMAs

// ---------------------------------------------------------------------------------------------------------------------------------
// v_mfma_f64_16x16x4_f64, D[16 x 16] = A[16 x 4] B[4 x 16] + C.  Its lane maps are NOT those of the f32-result MFMAs (gemm_core.h):
//   A, B: one f64 per lane; lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]
//   C, D: four f64 per lane; register r of lane l holds D[row (l >> 4) + 4 r][col l & 15]
// Here A = x^T and B = x over one group of four rows n0 .. n0 + 3: lane l loads x[n0 + (l >> 4)][i0 + (l & 15)] as its A value and
// x[n0 + (l >> 4)][j0 + 16 c + (l & 15)] as its B value of column block c = 0 .. 3, and register r of accumulator c is
// outer[i0 + (l >> 4) + 4 r][j0 + 16 c + (l & 15)].  A wave's 16 lanes with equal l >> 4 read 64 contiguous bytes of one row.
// The column sums ride on the diagonal tiles as a fifth product against a B of ones: every column of that result is sum[i0 + ..], the
// lanes of column 0 keep it.  Rows are consumed in ascending order, four at a time, from row 0 of THIS call; a row >= n or a column >= d
// is a predicated-off load that yields 0.0f (no clamped address), and a group that starts at or past n is skipped: the additions an
// element sees, and their order, are a function of (n, d) and the call sequence alone, so equal sequences give equal bits.
// No LDS, no atomics: every output element is read once, accumulated in registers and written once by the one lane that owns it.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float load_or_zero(const float* __restrict__ x, long row, long n, int col, int d, long ldx) {
  return (row < n && col < d) ? x[row * ldx + col] : 0.f;
}

__global__ __launch_bounds__(256) void moments_f64_kernel(const float* __restrict__ x, long n, int d, long ldx, double* __restrict__ sum,
                                                          double* __restrict__ outer, int T) {
  // blockIdx.x enumerates the tiles (ti, tj), tj >= ti, row by row: row ti has T - ti of them
  int ti = 0, rem = (int)blockIdx.x;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lc = lane & 15, lk = lane >> 4;
  const int i0 = ti * TILE + w * 16, j0 = tj * TILE;
  const int ia = i0 + lc;                                     // the column of x this lane feeds as A: an output ROW

  f64x4 acc[4], accs;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + lk + 4 * r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + 16 * c + lc;
      acc[c][r] = (i < d && j < d && j >= i) ? outer[(long)i * d + j] : 0.0;
    }
    accs[r] = (diag && lc == 0 && i < d) ? sum[i] : 0.0;
  }

  for (long n0 = 0; n0 < n; n0 += 4 * UN) {
    float a[UN], b[UN][4];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const long row = n0 + 4 * u + lk;
      a[u] = load_or_zero(x, row, n, ia, d, ldx);
#pragma unroll
      for (int c = 0; c < 4; ++c) b[u][c] = load_or_zero(x, row, n, j0 + 16 * c + lc, d, ldx);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (n0 + 4 * u < n) {                                   // wave-uniform
        const double da = (double)a[u];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(da, (double)b[u][c], acc[c], 0, 0, 0);
        if (diag) accs = __builtin_amdgcn_mfma_f64_16x16x4f64(da, 1.0, accs, 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + lk + 4 * r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + 16 * c + lc;
      if (i < d && j < d && j >= i) outer[(long)i * d + j] = acc[c][r];
    }
    if (diag && lc == 0 && i < d) sum[i] = accs[r];
  }
}

}  // namespace moments

extern "C" int muse_moments_f64(const float* x, int64_t n, int32_t d, int64_t ldx, double* sum, double* outer, void* stream) {
  if (d <= 0 || d % 4 || n < 0 || ldx < d || !x || !sum || !outer) return MUSE_ERR_BAD_ARG;
  if ((uintptr_t)x & 15) return MUSE_ERR_ALIGN;
  if (((uintptr_t)sum | (uintptr_t)outer) & 7) return MUSE_ERR_ALIGN;
  const long T = ((long)d + moments::TILE - 1) / moments::TILE;
  const long tiles = T * (T + 1) / 2;
  if (tiles > 0x7fffffffL) return MUSE_ERR_UNSUPPORTED;
  if (n == 0) return 0;
  hipLaunchKernelGGL(moments::moments_f64_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, x, (long)n, d, (long)ldx, sum,
                     outer, (int)T);
  return (int)hipGetLastError();
}
