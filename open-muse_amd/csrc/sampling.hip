// Token-level sampling / masking kernels around the transformer (the "next" rows f2 / f3 of SURVEY.md section 8):
//   muse_sample_step   - one iteration of MaskGit parallel decoding (muse/modeling_transformer.py:1409-1454 and
//                        muse/modeling_transformer_v2.py:434-474 with muse/sampling.py:30-35): classifier-free-guidance mix,
//                        softmax, categorical sample, confidence with Gumbel noise, k-th-smallest threshold, re-mask
//   muse_sample_step_filtered - the same step sampling from a top-k / nucleus (top-p) truncated distribution
//   muse_mask_tokens   - training/train_muse.py:149-226 mask_or_random_replace_tokens (random or contiguous-region masks,
//                        labels / loss weights variants)
//   muse_cond_dropout  - training/train_muse.py:715-731 (conditioning dropout for classifier-free guidance)
// All are latency-class kernels (a few MB at most); the point is one launch instead of ~10 ATen launches per decoding step and
// bit-exact agreement with the reference when the random draws are supplied by the caller.
#include "common.h"
#include "philox.h"   // Philox4x32-10, used when the caller supplies no random draws
#include "../../include/muse_hip.h"
#include <float.h>

__device__ __forceinline__ float clamp_log(float t) { return logf(fmaxf(t, 1e-20f)); }   // muse/sampling.py:9-10

// =================================================================================================================
// truncated sampling (muse_sample_step_filtered): the per-row cutoff of top-k / nucleus filtering, found without sorting the row
// =================================================================================================================
// order-preserving 32-bit key of a logit: a > b  <=>  key(a) > key(b)  (-0 shares +0's key, as it compares equal)
__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// a wave's histogram lives in its own 256 bins: its lanes run in lockstep and the LDS serves one wave's instructions in order,
// so the fence (no reordering by the compiler, LDS counter drained) is all the synchronisation there is
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// sum over the lanes above this one (lane 63: 0) of a per-lane value
template <typename T> __device__ __forceinline__ T lanes_above_sum(T own, int lane) {
  T incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_down(incl, o, 64);
    if (lane + o < 64) incl += t;
  }
  return incl - own;
}

// The cutoff tau of one row, kept set = {j : logit_j >= tau}; one wave, `cnt` / `mass` its 256 LDS bins.  Radix descent over
// order_key, one byte per level: each level re-reads the row (L2), histograms the byte below the prefix found so far over the codes
// that carry the prefix, and picks one bin; lane l owns bins 4 l .. 4 l + 3.  Everything is integer arithmetic, so the result does not
// depend on the order the LDS adds land in:
//   top-k    the bin that holds the k-th largest key (counts);
//   nucleus  over the codes the top-k set keeps, with mass e_j = trunc(exp(logit_j - max) * 2^40) (at most 2^54 a row): the lowest
//            non-empty bin whose mass above it, A, has A < top_p * sum_j e_j - its largest code has M_gt < top_p, the largest code
//            of the next non-empty bin below has not.  Tied logits share a key, hence a bin at every level.
template <typename L>
__device__ __forceinline__ float filter_cutoff(L logit, int V, int lane, int top_k, float top_p, float m, unsigned* cnt,
                                               unsigned long long* mass) {
  uint32_t kmin = 0;   // keys below are filtered
  if (top_k == 1) kmin = order_key(m);
  else if (top_k > 0) {
    uint32_t prefix = 0;
    int need = top_k;   // rank still to descend among the codes that carry the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
      *(uint4*)(cnt + 4 * lane) = uint4{0u, 0u, 0u, 0u};
      wave_lds_sync();
      for (int j = lane; j < V; j += 64) {
        const uint32_t key = order_key(logit(j));
        if (shift == 24 || (key >> (shift + 8)) == prefix) atomicAdd(cnt + ((key >> shift) & 255u), 1u);
      }
      wave_lds_sync();
      const uint4 h4 = *(const uint4*)(cnt + 4 * lane);
      const int h[4] = {(int)h4.x, (int)h4.y, (int)h4.z, (int)h4.w};
      int above = lanes_above_sum(h[0] + h[1] + h[2] + h[3], lane);
      int b = -1, nb = 0;
#pragma unroll
      for (int i = 3; i >= 0; --i) {
        if (above < need && need <= above + h[i]) { b = 4 * lane + i; nb = need - above; }
        above += h[i];
      }
      const unsigned long long hit = __ballot(b >= 0);   // exactly one lane: 1 <= need <= the number of codes under the prefix
      const int src = hit ? __ffsll(hit) - 1 : 0;
      b = max(__shfl(b, src, 64), 0);
      need = __shfl(nb, src, 64);
      prefix = (prefix << 8) | (uint32_t)b;
    }
    kmin = prefix;
  }
  if (top_p < 1.0f) {
    const uint32_t kk = kmin;
    uint32_t prefix = 0;
    unsigned long long base = 0;   // mass of the codes above every code that carries the prefix
    double target = 0.0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      *(uint4*)(cnt + 4 * lane) = uint4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 4; ++i) mass[4 * lane + i] = 0ull;
      wave_lds_sync();
      for (int j = lane; j < V; j += 64) {
        const float l = logit(j);
        const uint32_t key = order_key(l);
        if (key >= kk && (shift == 24 || (key >> (shift + 8)) == prefix)) {
          const uint32_t bin = (key >> shift) & 255u;
          atomicAdd(cnt + bin, 1u);
          atomicAdd(mass + bin, (unsigned long long)(expf(l - m) * 0x1p40f));
        }
      }
      wave_lds_sync();
      const uint4 h4 = *(const uint4*)(cnt + 4 * lane);
      const unsigned h[4] = {h4.x, h4.y, h4.z, h4.w};
      unsigned long long e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = mass[4 * lane + i];
      const unsigned long long own = e[0] + e[1] + e[2] + e[3];
      unsigned long long a = lanes_above_sum(own, lane);
      if (shift == 24) target = (double)top_p * (double)__shfl(a + own, 0, 64);   // lane 0's inclusive sum: the whole row
      a += base;
      int b = -1;
      unsigned long long ab = 0;
#pragma unroll
      for (int i = 3; i >= 0; --i) {   // high to low: the lowest bin that qualifies stays
        if (h[i] && (double)a < target) { b = 4 * lane + i; ab = a; }
        a += e[i];
      }
      const unsigned long long hit = __ballot(b >= 0);   // never empty: the bin of the row's (or the prefix's) largest code qualifies
      const int src = hit ? __ffsll(hit) - 1 : 0;        // the lowest lane owns the lowest bins
      b = max(__shfl(b, src, 64), 0);
      base = __shfl(ab, src, 64);
      prefix = (prefix << 8) | (uint32_t)b;
    }
    kmin = prefix;
  }
  return key_value(kmin);
}

// =================================================================================================================
// phase 1: one wave per (image, position) row.  FILTERED (muse_sample_step_filtered with a filter on): codes below the row's
// cutoff take the logit -inf - probability exactly 0 in the sum, the race and the confidence; top_k 0 / top_p 1: that filter is off
// =================================================================================================================
template <bool FILTERED>
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ cond, const float* __restrict__ uncond, float guidance,
                                                          int64_t img_stride, int64_t ld, int seq, int V, const int64_t* __restrict__ input_ids, int64_t mask_id,
                                                          const float* __restrict__ noise_exp, const float* __restrict__ noise_u,
                                                          uint64_t seed, uint32_t step, float temperature, int64_t rows,
                                                          int64_t* __restrict__ raw_ids, int64_t* __restrict__ ids, float* __restrict__ conf,
                                                          int top_k, float top_p, float* __restrict__ cutoff) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t img = row / seq, pos = row - img * seq;
  const float* c = cond + img * img_stride + pos * ld;
  const float* u = uncond ? uncond + img * img_stride + pos * ld : nullptr;
  auto mixed = [&](int j) {
    if (!u) return c[j];
    const float uu = u[j];
    // uncond + scale * (cond - uncond) (:403).  (The _rn forms are plain operators in HIP: the multiply and the add compile to one fma.)
    return __fadd_rn(uu, __fmul_rn(guidance, __fsub_rn(c[j], uu)));
  };
  float m = -INFINITY;
  for (int j = lane; j < V; j += 64) m = fmaxf(m, mixed(j));
  m = wave_max(m);
  float tau = -INFINITY;
  if constexpr (FILTERED) {
    __shared__ alignas(16) unsigned cnt[4][256];
    __shared__ alignas(16) unsigned long long mass[4][256];
    tau = filter_cutoff(mixed, V, lane, top_k, top_p, m, cnt[threadIdx.x >> 6], mass[threadIdx.x >> 6]);
  }
  if (cutoff && lane == 0) cutoff[row] = tau;
  auto logit = [&](int j) {
    const float l = mixed(j);
    if constexpr (FILTERED) return l < tau ? -INFINITY : l;
    else return l;
  };
  float s = 0.f;
  for (int j = lane; j < V; j += 64) s += expf(logit(j) - m);
  s = wave_sum(s);
  // categorical sample the way torch.multinomial(num_samples = 1) draws it: argmax_j p_j / q_j with q_j ~ Exp(1) (first index on ties)
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int j = lane; j < V; j += 64) {
    const float p = expf(logit(j) - m) / s;
    float q;
    if (noise_exp) q = noise_exp[row * V + j];
    else {
      const u4 r = philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), (uint32_t)j, step * 2u, (uint32_t)seed, (uint32_t)(seed >> 32));
      // u == 1 (the top 24 bits all ones, 2^-24 of the draws) has no positive q: -logf(1.0f) is -0.0f and p / q = -inf, so that token
      // could not be sampled whatever its probability (and with +0 it would always win).  torch's exponential_ never returns 0 either;
      // 2^-25 lies below the next smallest draw, -log(1 - 2^-24)
      const float uq = u01_open_low(r.x);
      q = uq < 1.0f ? -logf(uq) : 0x1p-25f;
    }
    const float v = p / q;
    if (v > best) { best = v; besti = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  if (lane == 0) {
    const int64_t cur = input_ids[row];
    const bool unknown = cur == mask_id;
    const int64_t fin = unknown ? (int64_t)besti : cur;
    if (raw_ids) raw_ids[row] = besti;
    ids[row] = fin;
    // confidence (muse/sampling.py:30-31): log(clamp(p_selected)) + temperature * gumbel;  known tokens carry FLT_MAX as their p
    float psel = FLT_MAX;
    if (unknown) psel = expf(logit(besti) - m) / s;
    float un;
    if (noise_u) un = noise_u[row];
    else {
      const u4 r = philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), 0u, step * 2u + 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
      un = u01_open_high(r.x);
    }
    const float gumbel = -clamp_log(-clamp_log(un));
    conf[row] = __fadd_rn(clamp_log(psel), __fmul_rn(temperature, gumbel));
  }
}

// =================================================================================================================
// phase 2: one workgroup per image: mask_len = max(1, min(#unknown - 1, scheduled)), threshold = the mask_len-th smallest
// confidence (0-based, torch.sort ascending + gather), next input = masked where confidence < threshold
// =================================================================================================================
__global__ __launch_bounds__(256) void remask_kernel(const int64_t* __restrict__ input_ids, const int64_t* __restrict__ ids,
                                                     const float* __restrict__ conf, int64_t* __restrict__ next_ids, int seq,
                                                     int64_t mask_id, int sched_len) {
  __shared__ float cf[4096];
  __shared__ int cnt;
  __shared__ float cut;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int local = 0;
  for (int i = threadIdx.x; i < seq; i += 256) {
    cf[i] = conf[(long)b * seq + i];
    local += input_ids[(long)b * seq + i] == mask_id;
  }
  local = (int)wave_sum((float)local);
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, local);
  __syncthreads();
  int k = min(cnt - 1, sched_len);
  k = max(1, k);
  k = min(k, seq - 1);   // (torch.gather would raise past the end; seq >= 2 on every path that reaches here)
  // the element of ascending rank k: value v with  #(x < v) <= k < #(x <= v)
  for (int i = threadIdx.x; i < seq; i += 256) {
    const float v = cf[i];
    int lt = 0, le = 0;
    for (int j = 0; j < seq; ++j) { const float x = cf[j]; lt += x < v; le += x <= v; }
    if (lt <= k && k < le) cut = v;   // every thread that qualifies writes the same value
  }
  __syncthreads();
  const float c = cut;
  for (int i = threadIdx.x; i < seq; i += 256) {
    const long o = (long)b * seq + i;
    next_ids[o] = cf[i] < c ? mask_id : ids[o];
  }
}

static int sample_step_launch(bool filtered, const float* cond_logits, const float* uncond_logits, float guidance_scale, int64_t img_stride,
                              int64_t ld, int32_t vocab, const int64_t* input_ids, int64_t mask_id, const float* noise_exp,
                              const float* noise_u, uint64_t seed, uint32_t step, float temperature, int32_t sched_mask_len, int32_t batch,
                              int32_t seq, int64_t* raw_sampled, int64_t* sampled, int64_t* next_ids, float* conf_scratch, int top_k,
                              float top_p, float* cutoff, void* stream) {
  if (!cond_logits || !input_ids || !sampled || !next_ids || !conf_scratch || vocab <= 0) return MUSE_ERR_BAD_ARG;
  if (seq > 4096 || seq < 2) return MUSE_ERR_UNSUPPORTED;
  if (batch <= 0) return 0;
  const int64_t rows = (int64_t)batch * seq;
  hipStream_t st = (hipStream_t)stream;
  const auto rows_kernel = filtered ? sample_rows_kernel<true> : sample_rows_kernel<false>;
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st,
                     cond_logits, uncond_logits, guidance_scale, img_stride, ld, seq, vocab, input_ids, mask_id, noise_exp, noise_u, seed, step,
                     temperature, rows, raw_sampled, sampled, conf_scratch, top_k, top_p, cutoff);
  MUSE_CHECK_LAUNCH();
  hipLaunchKernelGGL(remask_kernel, dim3(batch), dim3(256), 0, st, input_ids, (const int64_t*)sampled, (const float*)conf_scratch,
                     next_ids, seq, mask_id, sched_mask_len);
  return (int)hipGetLastError();
}

extern "C" int muse_sample_step(const float* cond_logits, const float* uncond_logits, float guidance_scale, int64_t img_stride, int64_t ld,
                                int32_t vocab,
                                const int64_t* input_ids, int64_t mask_id, const float* noise_exp, const float* noise_u,
                                uint64_t seed, uint32_t step, float temperature, int32_t sched_mask_len, int32_t batch, int32_t seq,
                                int64_t* raw_sampled, int64_t* sampled, int64_t* next_ids, float* conf_scratch, void* stream) {
  return sample_step_launch(false, cond_logits, uncond_logits, guidance_scale, img_stride, ld, vocab, input_ids, mask_id, noise_exp, noise_u,
                            seed, step, temperature, sched_mask_len, batch, seq, raw_sampled, sampled, next_ids, conf_scratch, 0, 1.0f,
                            nullptr, stream);
}

// The semantics of top_k / top_p / cutoff are stated once, at the prototype in include/muse_hip.h.  With both filters off this is
// muse_sample_step's own kernel (plus the -inf cutoff), so the two agree bit for bit.
extern "C" int muse_sample_step_filtered(const float* cond_logits, const float* uncond_logits, float guidance_scale, int64_t img_stride,
                                         int64_t ld, int32_t vocab, const int64_t* input_ids, int64_t mask_id, const float* noise_exp,
                                         const float* noise_u, uint64_t seed, uint32_t step, float temperature, int32_t sched_mask_len,
                                         int32_t batch, int32_t seq, int64_t* raw_sampled, int64_t* sampled, int64_t* next_ids,
                                         float* conf_scratch, int32_t top_k, float top_p, float* cutoff, void* stream) {
  if (top_k < 1 || !(top_p > 0.0f && top_p <= 1.0f)) return MUSE_ERR_BAD_ARG;   // (a NaN top_p fails the comparison)
  if (vocab > 16384) return MUSE_ERR_UNSUPPORTED;   // the row's fixed-point mass, at most vocab * 2^40, stays far inside 64 bits
  const int k = top_k >= vocab ? 0 : top_k;
  return sample_step_launch(k > 0 || top_p < 1.0f, cond_logits, uncond_logits, guidance_scale, img_stride, ld, vocab, input_ids, mask_id,
                            noise_exp, noise_u, seed, step, temperature, sched_mask_len, batch, seq, raw_sampled, sampled, next_ids,
                            conf_scratch, k, top_p, cutoff, stream);
}

// =================================================================================================================
// training/train_muse.py:149-226 mask_or_random_replace_tokens
// =================================================================================================================
// One workgroup per image.  mask source: rects != NULL: rectangle (y0, x0, h, w) on the sqrt(seq) grid (the contiguous-region
// branch; the reference draws it with Python's `random` on the host, so does the caller); else the argsort-threshold rule
// mask[j] = argsort(noise)[j] < k (k = round(seq * p) clamped to >= 1) of :175-176, the same rule as muse_mask_sample.
__global__ __launch_bounds__(256) void mask_tokens_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ timesteps,
                                                          const float* __restrict__ mask_prob_in, const float* __restrict__ noise,
                                                          const int32_t* __restrict__ rects, int64_t* __restrict__ input_ids,
                                                          int64_t* __restrict__ labels, float* __restrict__ loss_weight,
                                                          float* __restrict__ mask_prob, int seq, int side, int64_t mask_id,
                                                          float min_rate, int all_labels, float weight_min) {
  __shared__ float nz[4096];
  __shared__ int perm[4096];
  const int b = blockIdx.x;
  float prob;
  if (mask_prob_in) prob = mask_prob_in[b];   // eval_mask_ratios branch (:152-154): no schedule, no clip
  else {
    const float arg = (timesteps[b] * 3.14159265358979323846f) * 0.5f;   // cosine_schedule (muse/sampling.py:38-39), see muse_mask_sample
    prob = fmaxf((float)cos((double)arg), min_rate);
  }
  if (!rects) {
    for (int i = threadIdx.x; i < seq; i += 256) nz[i] = noise[(long)b * seq + i];
    __syncthreads();
    for (int i = threadIdx.x; i < seq; i += 256) {
      const float v = nz[i];
      int r = 0;
      for (int j = 0; j < seq; ++j) { const float u = nz[j]; r += (u < v) || (u == v && j < i); }
      perm[r] = i;
    }
    __syncthreads();
  }
  const int k = (int)fmaxf(rintf((float)seq * prob), 1.0f);
  if (threadIdx.x == 0) mask_prob[b] = prob;
  const float wk = __fmul_rn(__fsub_rn(1.0f, prob), __fsub_rn(1.0f, weight_min));   // (1 - t) * (1 - min_val) (:145-146, t = mask_prob)
  for (int j = threadIdx.x; j < seq; j += 256) {
    bool masked;
    if (rects) {
      const int y = j / side, x = j - y * side;
      const int32_t* r = rects + 4 * b;
      masked = y >= r[0] && y < r[0] + r[2] && x >= r[1] && x < r[1] + r[3];
    } else masked = perm[j] < k;
    const long o = (long)b * seq + j;
    const int64_t t = tokens[o];
    input_ids[o] = masked ? mask_id : t;
    labels[o] = (all_labels || masked) ? t : (int64_t)-100;
    if (loss_weight) loss_weight[o] = __fsub_rn(1.0f, __fmul_rn(masked ? 0.0f : 1.0f, wk));
  }
}

extern "C" int muse_mask_tokens(const int64_t* tokens, const float* timesteps, const float* mask_prob_in, const float* noise,
                                const int32_t* rects, int64_t* input_ids, int64_t* labels, float* loss_weight, float* mask_prob,
                                int32_t batch, int32_t seq, int64_t mask_id, float min_masking_rate, int32_t all_labels,
                                float weight_min, void* stream) {
  if (!tokens || !input_ids || !labels || !mask_prob || (!timesteps && !mask_prob_in) || (!noise && !rects)) return MUSE_ERR_BAD_ARG;
  if (seq > 4096 || seq <= 0) return MUSE_ERR_UNSUPPORTED;
  int side = 0;
  if (rects) {
    while (side * side < seq) ++side;
    if (side * side != seq) return MUSE_ERR_BAD_ARG;
  }
  if (batch <= 0) return 0;
  hipLaunchKernelGGL(mask_tokens_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, tokens, timesteps, mask_prob_in, noise, rects,
                     input_ids, labels, loss_weight, mask_prob, seq, side, mask_id, min_masking_rate, all_labels, weight_min);
  return (int)hipGetLastError();
}

// =================================================================================================================
// training/train_muse.py:715-731: per image keep = (u < p); out = (x * keep != 0) ? x : empty   (the reference's expression:
// an element that is exactly zero takes the empty embedding's value even when the image is kept)
// =================================================================================================================
__global__ void cond_dropout_kernel(const float* __restrict__ x, const float* __restrict__ empty, const float* __restrict__ u,
                                    float* __restrict__ out, long per_image, long total, float p) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / per_image, j = i - b * per_image;
    const float keep = u[b] < p ? 1.0f : 0.0f;
    const float v = x[i];
    out[i] = (v * keep != 0.0f) ? v : empty[j];   // (NaN * 1 != 0 is true, as `.bool()` of NaN is)
  }
}
extern "C" int muse_cond_dropout(const float* x, const float* empty, const float* uniforms, float* out, int32_t batch,
                                 int64_t per_image, float prob, void* stream) {
  if (!x || !empty || !uniforms || !out || per_image <= 0) return MUSE_ERR_BAD_ARG;
  if (batch <= 0) return 0;
  const long total = (long)batch * per_image;
  const unsigned grid = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(cond_dropout_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, empty, uniforms, out, (long)per_image,
                     total, prob);
  return (int)hipGetLastError();
}

// =================================================================================================================
// Dropout (nn.Dropout of muse/modeling_transformer.py:177,237 attention probabilities, :779,797 feed-forward, :933,956
// embeddings): y = x * keep / (1 - p), keep_i = [u_i >= p], u_i the Philox stream (seed, offset + i).  No mask tensor: the
// backward pass calls the same function on the gradient with the same (seed, offset).  One Philox block serves 4 elements.
// =================================================================================================================
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, long n, float p, float scale, uint64_t seed, uint64_t offset) {
  const long n4 = (n + 3) >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const uint64_t c = offset + (uint64_t)i;
    const u4 r = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), MUSE_DROPOUT_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = i * 4 + j;
      if (e < n) Elem<T>::store(y + e, u01_open_high(rr[j]) >= p ? Elem<T>::load(x + e) * scale : 0.0f);
    }
  }
}
extern "C" int muse_dropout(const void* x, void* y, int32_t dtype, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream) {
  if (!x || !y || p < 0.0f || p >= 1.0f) return MUSE_ERR_BAD_ARG;
  if (n <= 0) return 0;
  const long n4 = (n + 3) / 4;
  const unsigned grid = (unsigned)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
  const float scale = 1.0f / (1.0f - p);
  if (dtype == MUSE_F32) hipLaunchKernelGGL(dropout_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, (float*)y, (long)n, p, scale, seed, offset);
  else if (dtype == MUSE_BF16) hipLaunchKernelGGL(dropout_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, (long)n, p, scale, seed, offset);
  else return MUSE_ERR_BAD_ARG;
  return (int)hipGetLastError();
}
