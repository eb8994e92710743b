// Masked-token logging diagnostics (muse/training_utils.py): per-token entropy + logsumexp in ONE pass over the logits, and the per-image
// mean predicted distribution over the masked tokens (+ its entropy) in one pass over the MASKED rows only.  Both are row kernels that move
// each row they need once: wave64, 16-byte loads, f32 accumulation whatever the storage type, no atomics, no logits-sized temporary.
//
// Canonical column groups.  A row's columns are cut into groups of G = 16 / sizeof(T) columns BY COLUMN INDEX (group k = columns
// [G k, G k + G)), never by address, and every sum below is a fixed function of (group, position in the group).  So a row's results do
// not depend on where the row lies in memory - which other rows share the batch, or what `ld` is - and are the same bits from run to
// run.  How a group is LOADED does depend on the row base (load_group): one 16-byte load where the base is 16-byte aligned; where it
// is not (vocab = ld = 2025: three of four f32 rows), the two aligned 16-byte vectors that cover the group, funnel-shifted in
// registers; and element loads under a column predicate for the peeled head (group 0 of an unaligned row: its lower vector would
// start before the row) and tail (the last groups, whose upper vector or own end would pass column `vocab`).  Nothing outside
// [row, row + vocab) is ever read.
#include "common.h"
#include "../../include/muse_hip.h"

namespace {

template <typename T> struct Grp;
template <> struct Grp<float> { static constexpr int G = 4; };
template <> struct Grp<bf16_t> { static constexpr int G = 8; };

template <typename T> __device__ __forceinline__ void unpack16(const u32x4& w, float (&v)[Grp<T>::G]);
template <> __device__ __forceinline__ void unpack16<float>(const u32x4& w, float (&v)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(w[i]);
}
template <> __device__ __forceinline__ void unpack16<bf16_t>(const u32x4& w, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}

// the row base's offset behind a 16-byte boundary, in elements (0 = aligned)
template <typename T> __device__ __forceinline__ int base_skew(const T* xr) { return (int)(((uintptr_t)xr & 15) / sizeof(T)); }

// columns [G k, G k + G) of the row at xr -> v (columns >= vocab: 0, not read); skew = base_skew(xr).  k and skew are what decide the
// route, the values delivered are the same on every route.
template <typename T>
__device__ __forceinline__ void load_group(const T* __restrict__ xr, int k, int vocab, int skew, float (&v)[Grp<T>::G]) {
  constexpr int G = Grp<T>::G;
  const int c0 = k * G;
  if (skew == 0) {
    if (c0 + G <= vocab) { unpack16<T>(*(const u32x4*)(xr + c0), v); return; }
  } else if (k >= 1 && c0 - skew + 2 * G <= vocab) {
    // aligned vectors A = columns [c0 - skew, c0 - skew + G) and B = the next G: the group is elements skew .. skew + G - 1 of (A, B)
    const u32x4 A = *(const u32x4*)(xr + c0 - skew);
    const u32x4 B = *(const u32x4*)(xr + c0 - skew + G);
    const int sd = sizeof(T) == 4 ? skew : skew >> 1;   // whole dwords to drop (wave-uniform: one row per wave / per load)
    uint32_t w0, w1, w2, w3, w4;
    switch (sd) {
      case 0: w0 = A[0]; w1 = A[1]; w2 = A[2]; w3 = A[3]; w4 = B[0]; break;
      case 1: w0 = A[1]; w1 = A[2]; w2 = A[3]; w3 = B[0]; w4 = B[1]; break;
      case 2: w0 = A[2]; w1 = A[3]; w2 = B[0]; w3 = B[1]; w4 = B[2]; break;
      default: w0 = A[3]; w1 = B[0]; w2 = B[1]; w3 = B[2]; w4 = B[3]; break;
    }
    if (sizeof(T) == 2 && (skew & 1)) {                  // bf16 at an odd element: shift the five dwords right by one half
      w0 = (w0 >> 16) | (w1 << 16); w1 = (w1 >> 16) | (w2 << 16); w2 = (w2 >> 16) | (w3 << 16); w3 = (w3 >> 16) | (w4 << 16);
    }
    unpack16<T>(u32x4{w0, w1, w2, w3}, v);
    return;
  }
  // peeled head / tail: element loads, columns past vocab not touched
#pragma unroll
  for (int i = 0; i < G; ++i) v[i] = c0 + i < vocab ? Elem<T>::load(xr + c0 + i) : 0.f;
}

// ---- online (max, sum e, sum e d) with d = x - max: lse = m + log s, entropy = log s - t / s (that is lse - sum(e x) / sum(e) with
// the max taken out of both terms, so no large lse and mean logit cancel) ----------------------------------------------------------------
struct Mst { float m, s, t; };

// fold one group (n valid columns, 1 <= n <= G) into a lane's state.  One rescale per group; explicit fmaf so that every inlined copy
// rounds alike.
template <int G>
__device__ __forceinline__ void fold_group(Mst& a, const float (&v)[G], int n) {
  float cm = v[0];
#pragma unroll
  for (int i = 1; i < G; ++i) cm = i < n ? fmaxf(cm, v[i]) : cm;
  if (cm > a.m) {
    if (a.m > -INFINITY) {
      const float dm = a.m - cm, c = expf(dm);
      a.t = fmaf(dm, a.s, a.t) * c;
      a.s = a.s * c;
    }
    a.m = cm;
  }
  float se = 0.f, st = 0.f;
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const float d = v[i] - a.m, e = expf(d);
    if (i < n) { se += e; st = fmaf(e, d, st); }
  }
  a.s += se;
  a.t += st;
}

// a (+) b; an empty state (m = -inf, s = t = 0) contributes nothing.  Symmetric in its arguments bit for bit.
__device__ __forceinline__ Mst merge(const Mst& a, const Mst& b) {
  const float M = fmaxf(a.m, b.m);
  const float da = a.m - M, db = b.m - M;
  const float ca = a.m > -INFINITY ? expf(da) : 0.f, cb = b.m > -INFINITY ? expf(db) : 0.f;
  const float ta = a.m > -INFINITY ? fmaf(da, a.s, a.t) * ca : 0.f, tb = b.m > -INFINITY ? fmaf(db, b.s, b.t) * cb : 0.f;
  Mst r;
  r.m = M;
  r.s = a.s * ca + b.s * cb;
  r.t = ta + tb;
  return r;
}

// one wave per row, four rows per block.  Lane l folds groups l, l + 64, ... in ascending order (two loads in flight), then a
// butterfly merges the 64 states.
template <typename T>
__global__ __launch_bounds__(256) void token_stats_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ row_mask,
                                                          float* __restrict__ lse_o, float* __restrict__ ent_o, float* __restrict__ max_o,
                                                          float* __restrict__ sum_o, long rows, int vocab, long ld) {
  constexpr int G = Grp<T>::G;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (row_mask && !row_mask[row]) {          // wave-uniform: a row that is not selected is not loaded
    if (lane == 0) {
      lse_o[row] = 0.f; ent_o[row] = 0.f;
      if (max_o) { max_o[row] = 0.f; sum_o[row] = 1.f; }
    }
    return;
  }
  const T* xr = logits + row * ld;
  const int skew = base_skew(xr);
  const int ngroups = (vocab + G - 1) / G;
  Mst a{-INFINITY, 0.f, 0.f};
  float v0[G], v1[G];
  int k = lane;
  for (; k + 64 < ngroups; k += 128) {
    load_group<T>(xr, k, vocab, skew, v0);
    load_group<T>(xr, k + 64, vocab, skew, v1);
    fold_group<G>(a, v0, G);                                       // k is not the last group here
    fold_group<G>(a, v1, min(G, vocab - (k + 64) * G));
  }
  if (k < ngroups) {
    load_group<T>(xr, k, vocab, skew, v0);
    fold_group<G>(a, v0, min(G, vocab - k * G));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Mst b;
    b.m = __shfl_xor(a.m, o, 64); b.s = __shfl_xor(a.s, o, 64); b.t = __shfl_xor(a.t, o, 64);
    a = merge(a, b);
  }
  if (lane == 0) {
    const float ls = logf(a.s);
    lse_o[row] = a.m + ls;
    ent_o[row] = ls - a.t / a.s;
    if (max_o) { max_o[row] = a.m; sum_o[row] = a.s; }
  }
}

// ---- mean predicted distribution over an image's masked tokens ---------------------------------------------------------------------
// grid (ceil(groups / 64), B), 16 waves per block: the block owns 64 column groups of one image (lane = group: a wave reads 1 KiB of a
// row at a time), and its waves share the image's masked rows - wave w takes the w-th sixteenth of the masked-row list, in ascending
// order, and the sixteen partial sums are added in wave order through LDS.  Which rows a wave takes depends on the image's own masked
// count alone, so the result does not depend on the batch.  Each term is softmax(x) = exp(x - max) * (1 / sum) with (max, sum) as
// muse_token_stats left them, NOT exp(x - lse): lse carries its own rounding, half an ulp of a number near 10, which is a relative
// error of 5e-7 common to every probability of the row and shows in the entropy of an image with few masked tokens; max and sum are
// what torch's softmax divides by.  The masked rows of a segment of kSeg rows are first compacted into LDS (ballot + prefix count),
// so the row loop only ever touches masked rows and keeps kUnroll row loads in flight per wave.
constexpr int kSeg = 2048, kUnroll = 8, kWaves = 16, kChunks = kSeg / 64;
static_assert(kChunks % kWaves == 0, "every wave takes the same number of 64-row chunks of a segment");

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void masked_mean_probs_kernel(const T* __restrict__ logits, const int64_t* __restrict__ ids,
                                                                        const float* __restrict__ row_max, const float* __restrict__ sum_exp,
                                                                        float* __restrict__ out, int S, int vocab, long ld, int64_t mask_id) {
  constexpr int G = Grp<T>::G;
  __shared__ int list[kSeg];
  __shared__ int chunk_n[kChunks];
  __shared__ float red[kWaves][G][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int k = blockIdx.x * 64 + lane;
  const int ngroups = (vocab + G - 1) / G;
  const bool own = k < ngroups;
  const int64_t* idr = ids + (long)b * S;
  const float* mr = row_max + (long)b * S;
  const float* sr = sum_exp + (long)b * S;
  const T* xb = logits + (long)b * S * ld;
  float acc[G];
#pragma unroll
  for (int i = 0; i < G; ++i) acc[i] = 0.f;
  int total = 0;
  for (int s0 = 0; s0 < S; s0 += kSeg) {
    __syncthreads();                                   // the previous segment's list is no longer read
    // wave w looks at the segment's 64-row chunks w and w + 16 (all id loads of the block in flight at once), the chunk counts go
    // through LDS, and every wave places its hits behind the hits of the chunks before its own
    const int send = min(S, s0 + kSeg);
    unsigned long long bal[kChunks / kWaves];
#pragma unroll
    for (int c = 0; c < kChunks / kWaves; ++c) {
      const int s = s0 + (w + c * kWaves) * 64 + lane;
      bal[c] = __ballot(s < send && idr[s] == mask_id);
      if (lane == 0) chunk_n[w + c * kWaves] = __popcll(bal[c]);
    }
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int c = 0; c < kChunks / kWaves; ++c) {
      const int chunk = w + c * kWaves;
      int base = 0;
      for (int j = 0; j < chunk; ++j) base += chunk_n[j];
      if ((bal[c] >> lane) & 1ull) list[base + __popcll(bal[c] & ((1ull << lane) - 1ull))] = s0 + chunk * 64 + lane;
    }
    for (int j = 0; j < kChunks; ++j) n += chunk_n[j];
    __syncthreads();
    total += n;
    if (own) {
      int i = (int)((long)n * w / kWaves);
      const int iend = (int)((long)n * (w + 1) / kWaves);
      for (; i + kUnroll <= iend; i += kUnroll) {
        float v[kUnroll][G], mx[kUnroll], rs[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int s = list[i + u];
          const T* xr = xb + (long)s * ld;
          load_group<T>(xr, k, vocab, base_skew(xr), v[u]);
          mx[u] = mr[s];
          rs[u] = 1.0f / sr[s];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
          for (int j = 0; j < G; ++j) acc[j] += expf(v[u][j] - mx[u]) * rs[u];
      }
      for (; i < iend; ++i) {
        const int s = list[i];
        const T* xr = xb + (long)s * ld;
        float v[G];
        load_group<T>(xr, k, vocab, base_skew(xr), v);
        const float mx = mr[s], rs = 1.0f / sr[s];
#pragma unroll
        for (int j = 0; j < G; ++j) acc[j] += expf(v[j] - mx) * rs;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < G; ++j) red[w][j][lane] = acc[j];
  __syncthreads();
  if (w == 0 && own) {
    const float cnt = (float)total;                    // no masked token: 0 / 0 = NaN, as the reference's division
#pragma unroll
    for (int j = 0; j < G; ++j) {
      float t = red[0][j][lane];
#pragma unroll
      for (int u = 1; u < kWaves; ++u) t += red[u][j][lane];
      if (k * G + j < vocab) out[(long)b * vocab + k * G + j] = t / cnt;
    }
  }
}

// entropy of each row of p [rows, cols] f32: -sum p log p as written (p = 0 gives 0 * -inf = NaN, like p.log()).  One block per row, a
// fixed order: thread t adds columns t, t + 256, ...; the 64 lanes of a wave by butterfly; the four waves in order.
__global__ __launch_bounds__(256) void prob_entropy_kernel(const float* __restrict__ p, float* __restrict__ out, int cols) {
  __shared__ float part[4];
  const float* pr = p + (long)blockIdx.x * cols;
  float s = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) { const float q = pr[c]; s = fmaf(q, logf(q), s); }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = -(((part[0] + part[1]) + part[2]) + part[3]);
}

// out[b] = (sum_s values[b, s]) / #{s : ids[b, s] == mask_id}: the per-image mean of the masked tokens' entropies (the rows that are not
// masked hold exact zeros).  One block per image and the order of prob_entropy_kernel, so an image's mean does not depend on the batch -
// which a library reduction over [B, S] does not promise.  No masked token: 0 / 0 = NaN, as the reference's division.
__global__ __launch_bounds__(256) void masked_row_mean_kernel(const float* __restrict__ values, const int64_t* __restrict__ ids,
                                                              float* __restrict__ out, int S, int64_t mask_id) {
  __shared__ float part[4];
  __shared__ int cnt[4];
  const float* vr = values + (long)blockIdx.x * S;
  const int64_t* idr = ids + (long)blockIdx.x * S;
  float s = 0.f;
  int n = 0;
  for (int c = threadIdx.x; c < S; c += 256) { s += vr[c]; n += idr[c] == mask_id; }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = s; cnt[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
}

}  // namespace

extern "C" int muse_masked_row_mean(const float* values, const int64_t* input_ids, float* out, int32_t batch, int32_t seq, int64_t mask_id,
                                    void* stream) {
  if (batch <= 0 || seq <= 0 || !values || !input_ids || !out) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(masked_row_mean_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, values, input_ids, out, seq, mask_id);
  return (int)hipGetLastError();
}

extern "C" int muse_token_stats(const void* logits, int32_t dtype, const uint8_t* row_mask, float* lse, float* entropy, float* row_max,
                                float* sum_exp, int64_t rows, int32_t vocab, int64_t ld, void* stream) {
  if (rows <= 0 || vocab <= 0 || ld < vocab || !logits || !lse || !entropy || !row_max != !sum_exp ||
      (dtype != MUSE_F32 && dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  if ((rows + 3) / 4 > 0x7fffffffL) return MUSE_ERR_UNSUPPORTED;
  if ((uintptr_t)logits % (dtype == MUSE_F32 ? 4 : 2)) return MUSE_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(token_stats_kernel<float>, grid, dim3(256), 0, s, (const float*)logits, row_mask, lse, entropy, row_max, sum_exp, (long)rows, vocab, (long)ld);
  else hipLaunchKernelGGL(token_stats_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)logits, row_mask, lse, entropy, row_max, sum_exp, (long)rows, vocab, (long)ld);
  return (int)hipGetLastError();
}

extern "C" int muse_masked_mean_probs(const void* logits, int32_t dtype, const int64_t* input_ids, const float* row_max, const float* sum_exp,
                                      float* mean_probs, float* entropy, int32_t batch, int32_t seq, int32_t vocab, int64_t ld,
                                      int64_t mask_id, void* stream) {
  if (batch <= 0 || seq <= 0 || vocab <= 0 || ld < vocab || !logits || !input_ids || !row_max || !sum_exp || !mean_probs ||
      (dtype != MUSE_F32 && dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  if (batch > 65535) return MUSE_ERR_UNSUPPORTED;
  if ((uintptr_t)logits % (dtype == MUSE_F32 ? 4 : 2)) return MUSE_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int G = dtype == MUSE_F32 ? 4 : 8, ngroups = (vocab + G - 1) / G;
  const dim3 grid((unsigned)((ngroups + 63) / 64), (unsigned)batch), block(64 * kWaves);
  if (dtype == MUSE_F32) hipLaunchKernelGGL(masked_mean_probs_kernel<float>, grid, block, 0, s, (const float*)logits, input_ids, row_max, sum_exp, mean_probs, seq, vocab, (long)ld, mask_id);
  else hipLaunchKernelGGL(masked_mean_probs_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)logits, input_ids, row_max, sum_exp, mean_probs, seq, vocab, (long)ld, mask_id);
  MUSE_CHECK_LAUNCH();
  if (entropy) hipLaunchKernelGGL(prob_entropy_kernel, dim3((unsigned)batch), dim3(256), 0, s, (const float*)mean_probs, entropy, vocab);
  return (int)hipGetLastError();
}
