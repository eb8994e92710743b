// Sums of a Gaussian kernel over all pairs of two sets of f32 feature rows, in f64, for the maximum mean discrepancy on CLIP image embeds
// (muse/mmd.py: mmd_distance, cmmd_distance).  Contract in include/muse_hip.h:
//   muse_row_norms_f64     sumsq[i] = sum_k (double)x_ik^2, rinv[i] = 1 / sqrt(sumsq[i])
//   muse_rbf_pair_sums_f64 sum over pairs of k_ij = exp(-gamma (a_i + b_j - 2 c_ij)),  c_ij = rx_i ry_j sum_k x_ik y_jk,
//                          a_i = rx_i^2 sum_k x_ik^2, b_j = ry_j^2 sum_k y_jk^2 - without ever writing the n x m matrix
// Every product of two converted f32 values is exact in f64 (24 + 24 significant bits < 53): inside a dot product only the additions round.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/muse_hip.h"

namespace mmd {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 64;        // a workgroup owns one TILE x TILE tile of pairs; wave w its rows [16 w, 16 w + 16)
constexpr int KC = 16;          // features per step: every lane loads one float4 of its row, the four lanes of a row 64 contiguous bytes
constexpr int FIN = 1024;       // threads of the one workgroup that adds the partials

// a lane's 16 bytes of row `row` at feature k, or zeros: a row >= rows or a feature >= d is a predicated-off load, never a clamped address
__device__ __forceinline__ float4 load4_or_zero(const float* __restrict__ p, long row, long rows, int k, int d, long ld) {
  return (row < rows && k < d) ? *reinterpret_cast<const float4*>(p + row * ld + k) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// sum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (one row's four K slots), the same bits in all four
__device__ __forceinline__ double sum_over_k_slots(double v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One wave per row, a workgroup of four rows.  Lane l adds the squares of features 4 l + 256 t + (0 .. 3), t ascending, onto its own
// f64 sum (fma of an exact product: one rounding per addition), then the 64 lane sums are added by a butterfly: the order is a
// function of d alone.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_norms_f64_kernel(const float* __restrict__ x, long n, int d, long ldx, double* __restrict__ sumsq,
                                                            double* __restrict__ rinv) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                       // wave-uniform
  double s = 0.0;
  for (int k = 4 * lane; k < d; k += 256) {
    const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + k);
    s = fma((double)v.x, (double)v.x, s);
    s = fma((double)v.y, (double)v.y, s);
    s = fma((double)v.z, (double)v.z, s);
    s = fma((double)v.w, (double)v.w, s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    sumsq[row] = s;
    if (rinv) rinv[row] = 1.0 / sqrt(s);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// v_mfma_f64_16x16x4_f64, D[16 x 16] = A[16 x 4] B[4 x 16] + C (lane maps: moments.hip):
//   A, B: one f64 per lane; lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]
//   C, D: four f64 per lane; register r of lane l holds D[row (l >> 4) + 4 r][col l & 15]
// Here K runs along the FEATURE axis, so both operands are read along rows: in a step of 16 features k0 .. k0 + 15, lane l loads the
// float4 x[i0 + (l & 15)][k0 + 4 (l >> 4) .. + 3] and, for column block c = 0 .. 3, y[j0 + 16 c + (l & 15)][the same features], and element g
// of those float4s feeds the g-th of four MFMAs - whose K slot l >> 4 is then feature k0 + 4 (l >> 4) + g for A and B alike: a fixed
// permutation of k inside the dot product.  Register r of accumulator c is the dot product of rows i0 + (l >> 4) + 4 r and
// j0 + 16 c + (l & 15).  The four lanes of a row read 64 contiguous bytes per load instruction.
// The squared norms ride along: every lane adds the squares of what it loaded (fma of exact products), the four K-slot lanes of a row are
// added by a butterfly; b_j then sits in the lane that needs it (column l & 15), a_i is fetched from lane (l >> 4) + 4 r.
// Epilogue, per pair: k = exp(-gamma (a_i + b_j - 2 c_ij)), counted only where i < n and j < m BY PREDICATE (a padded zero row would
// contribute exp(-gamma b_j), not 0); in the symmetric form j > i goes to the upper sum and j == i to the diagonal sum.  A lane adds its
// 16 values in the order c outer, r inner, the wave adds its 64 lanes by a butterfly and lane 0 writes the wave's partial(s) to
// `ws[4 tile + wave]` (and `ws[P + 4 tile + wave]`): no LDS, no atomics, no barrier.
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool SYM>
__global__ __launch_bounds__(256) void rbf_pair_sums_kernel(const float* __restrict__ x, long n, long ldx, const double* __restrict__ rx,
                                                            const float* __restrict__ y, long m, long ldy, const double* __restrict__ ry, int d,
                                                            double gamma, int Tm, long P, double* __restrict__ ws) {
  int ti, tj;
  if (SYM) {                    // blockIdx.x enumerates the tiles (ti, tj), tj >= ti, row by row: row ti has Tm - ti of them
    int rem = (int)blockIdx.x;
    ti = 0;
    while (rem >= Tm - ti) { rem -= Tm - ti; ++ti; }
    tj = ti + rem;
  } else {
    ti = (int)(blockIdx.x / (unsigned)Tm);
    tj = (int)(blockIdx.x % (unsigned)Tm);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lc = lane & 15, lk = lane >> 4;
  const long i0 = (long)ti * TILE + w * 16, j0 = (long)tj * TILE;
  const long slot = (long)blockIdx.x * 4 + w;

  double upper = 0.0, diagonal = 0.0;
  if (i0 < n) {                                               // wave-uniform: a wave whose 16 rows are all padding has no pair
    f64x4 acc[4];
    double sa = 0.0, sb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
      sb[c] = 0.0;
    }
    // the loads of step k0 + KC are issued before the MFMAs of step k0 (past d they are predicated off)
    float4 a_next = load4_or_zero(x, i0 + lc, n, 4 * lk, d, ldx), b_next[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b_next[c] = load4_or_zero(y, j0 + 16 * c + lc, m, 4 * lk, d, ldy);
    for (int k0 = 0; k0 < d; k0 += KC) {
      const int k = k0 + KC + 4 * lk;
      const float4 a = a_next;
      float4 b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = b_next[c];
      a_next = load4_or_zero(x, i0 + lc, n, k, d, ldx);
#pragma unroll
      for (int c = 0; c < 4; ++c) b_next[c] = load4_or_zero(y, j0 + 16 * c + lc, m, k, d, ldy);
      const double ad[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
#pragma unroll
      for (int g = 0; g < 4; ++g) sa = fma(ad[g], ad[g], sa);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double bd[4] = {(double)b[c].x, (double)b[c].y, (double)b[c].z, (double)b[c].w};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          sb[c] = fma(bd[g], bd[g], sb[c]);
          acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[g], bd[g], acc[c], 0, 0, 0);
        }
      }
    }
    // a_i of row i0 + lc and b_j of rows j0 + 16 c + lc, scaled; a NULL rx / ry is a factor of exactly 1.0
    const long ia = i0 + lc;
    const double rxa = (rx && ia < n) ? rx[ia] : 1.0;
    const double a_mine = (rxa * rxa) * sum_over_k_slots(sa);
    double ryb[4], bj[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long j = j0 + 16 * c + lc;
      ryb[c] = (ry && j < m) ? ry[j] : 1.0;
      bj[c] = (ryb[c] * ryb[c]) * sum_over_k_slots(sb[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long j = j0 + 16 * c + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int src = lk + 4 * r;                           // the lane (with K slot 0) that holds row i0 + lk + 4 r
        const long i = i0 + src;
        const double ai = __shfl(a_mine, src), rxi = __shfl(rxa, src);
        const double cij = (rxi * ryb[c]) * acc[c][r];
        const double kij = exp(-gamma * ((ai + bj[c]) - 2.0 * cij));
        const bool in = i < n && j < m;
        if (SYM) {
          if (in && j > i) upper += kij;
          if (in && j == i) diagonal += kij;
        } else if (in) {
          upper += kij;
        }
      }
    }
    upper = wave_sum(upper);
    if (SYM) diagonal = wave_sum(diagonal);
  }
  if (lane == 0) {
    ws[slot] = upper;
    if (SYM) ws[P + slot] = diagonal;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One workgroup of FIN threads: thread t adds partials t, t + FIN, t + 2 FIN, .. in that order, a binary tree in LDS adds the FIN
// thread sums.  out[0] from ws[0 .. P), out[1] from ws[P .. 2 P) (symmetric) or 0.  The longest chain of additions a partial goes
// through here is ceil(P / FIN) + 10; with the 16 of a lane and the 6 of a wave in the pair kernel: A = ceil(P / 1024) + 32.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIN) void rbf_finalize_kernel(const double* __restrict__ ws, long P, int nsums, double* __restrict__ out) {
  __shared__ double red[FIN];
  const int t = threadIdx.x;
  for (int s = 0; s < 2; ++s) {
    double v = 0.0;
    if (s < nsums)
      for (long p = t; p < P; p += FIN) v += ws[(long)s * P + p];
    red[t] = v;
    __syncthreads();
    for (int o = FIN / 2; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    if (t == 0) out[s] = red[0];
    __syncthreads();
  }
}

static inline long tiles_1d(int64_t rows) { return (long)((rows + TILE - 1) / TILE); }

// number of tiles, or -1 where the grid does not fit an int
static long tile_count(int64_t n, int64_t m, bool symmetric) {
  const long tn = tiles_1d(n), tm = tiles_1d(symmetric ? n : m);
  if (tn > 0x7fffffffL || tm > 0x7fffffffL) return -1;
  const __int128 tiles = symmetric ? (__int128)tn * (tn + 1) / 2 : (__int128)tn * tm;
  return tiles > 0x7fffffffL ? -1 : (long)tiles;
}

}  // namespace mmd

extern "C" int muse_row_norms_f64(const float* x, int64_t n, int32_t d, int64_t ldx, double* sumsq, double* rinv, void* stream) {
  if (d <= 0 || d % 4 || n < 0 || ldx < d || !x || !sumsq) return MUSE_ERR_BAD_ARG;
  if (((uintptr_t)x & 15) || ldx % 4) return MUSE_ERR_ALIGN;
  if (((uintptr_t)sumsq | (uintptr_t)rinv) & 7) return MUSE_ERR_ALIGN;
  const int64_t blocks = (n + 3) / 4;
  if (blocks > 0x7fffffffL) return MUSE_ERR_UNSUPPORTED;
  if (n == 0) return 0;
  hipLaunchKernelGGL(mmd::row_norms_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)n, d, (long)ldx, sumsq, rinv);
  return (int)hipGetLastError();
}

extern "C" int64_t muse_rbf_pair_sums_workspace(int64_t n, int64_t m, int32_t symmetric) {
  if (n < 0 || (!symmetric && m < 0)) return MUSE_ERR_BAD_ARG;
  const long tiles = mmd::tile_count(n, m, symmetric != 0);
  if (tiles < 0) return MUSE_ERR_UNSUPPORTED;
  return (int64_t)tiles * 4 * (symmetric ? 2 : 1);
}

extern "C" int muse_rbf_pair_sums_f64(const float* x, int64_t n, int64_t ldx, const double* rx, const float* y, int64_t m, int64_t ldy,
                                      const double* ry, int32_t d, const double* gamma, double* workspace, double* out, void* stream) {
  const bool sym = y == nullptr;
  if (d <= 0 || d % 4 || n < 0 || ldx < d || !x || !gamma || !workspace || !out) return MUSE_ERR_BAD_ARG;
  if (!sym && (m < 0 || ldy < d)) return MUSE_ERR_BAD_ARG;
  if (((uintptr_t)x & 15) || ldx % 4) return MUSE_ERR_ALIGN;
  if (!sym && (((uintptr_t)y & 15) || ldy % 4)) return MUSE_ERR_ALIGN;
  if (((uintptr_t)rx | (uintptr_t)(sym ? nullptr : ry) | (uintptr_t)workspace | (uintptr_t)out) & 7) return MUSE_ERR_ALIGN;
  if (sym) { m = n; ldy = ldx; }
  const long tiles = mmd::tile_count(n, m, sym);
  if (tiles < 0) return MUSE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || m == 0) return (int)hipMemsetAsync(out, 0, 2 * sizeof(double), s);
  const long P = tiles * 4;
  const int Tm = (int)mmd::tiles_1d(m);
  const double g = *gamma;
  if (sym)
    hipLaunchKernelGGL(mmd::rbf_pair_sums_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, s, x, (long)n, (long)ldx, rx, x, (long)n, (long)ldx, rx, d,
                       g, Tm, P, workspace);
  else
    hipLaunchKernelGGL(mmd::rbf_pair_sums_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, s, x, (long)n, (long)ldx, rx, y, (long)m, (long)ldy, ry, d,
                       g, Tm, P, workspace);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(mmd::rbf_finalize_kernel, dim3(1), dim3(mmd::FIN), 0, s, workspace, P, sym ? 2 : 1, out);
  return (int)hipGetLastError();
}
