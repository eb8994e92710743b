// CLIP text tower (transformers CLIPTextModel / CLIPTextModelWithProjection: the `type: "clip"` text encoder of the reference's
// configs, called every step at training/train_muse.py:647-649) - the kernels it needs beyond the transformer ones:
//   1. fused CAUSAL self-attention, forward only: bf16 q / k / v / o, f32 softmax and accumulation, MFMA products.  The whole sequence
//      (<= 128 tokens; every published tower has 77) is ONE tile: a workgroup owns one (image, head), K and V^T live in LDS, wave w owns
//      query rows 16 w .. 16 w + 15 and only the key tiles <= w.  No online softmax, no S x S matrix in memory.
//   2. causal row softmax of materialised f32 score matrices (the exact-f32 mode, between two muse_gemm products)
//   3. bias + quick-GELU behind the FC1 product, LayerNorm WITH bias in one pass
//   4. the pooled ("EOS") position of every id row, on the device
#include "common.h"
#include "../../include/muse_hip.h"

namespace clip {

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. fused causal attention.
// Products as TRANSPOSES so that the score tile comes out of the first MFMA in the operand layout of the second:
//   S^T[key][query] = K Q^T   v_mfma_f32_16x16x32_bf16, A = K rows from LDS, B = Q rows from global memory (each read once)
//     -> lane (n = lane & 15, g = lane >> 4) holds S^T[16 kt + 4 g + i][query n], i = 0..3, for every key tile kt <= its query tile
//   O^T[d][query]   = V^T P^T  the same MFMA over PAIRS of key tiles: k slot j of lane group g is key 16 (2u) + 4 g + j (j < 4) or
//     16 (2u + 1) + 4 g + j - 4 (j >= 4) - a permutation of the 32 keys of the pair, applied to both operands (the V^T fragment is two
//     8-byte LDS reads at those keys), so the lane's own probabilities are its B fragment with no lane movement.
// Masking: key j takes part in query i iff j <= i and j < S.  A masked probability is the literal 0.f (never exp of anything); K / V rows
// and Q rows >= S are zero-filled registers / LDS, never memory reads (the last image's rows >= S lie outside the caller's allocation),
// and every query row - padding rows too - sees key 0, so its maximum is finite and its sum >= 1: no NaN anywhere.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int LDS_PAD = 8;   // bf16 elements behind every LDS row (16 bytes: keeps 16-byte alignment, spreads rows over the banks)

struct AttnArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
  long ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;
  int heads, S;
  float alpha;
};

template <int HD>
__global__ __launch_bounds__(512) void causal_attn_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KROW = HD + LDS_PAD;                 // K image: [Sp16][KROW]
  constexpr int CPR = HD / 8;                        // 16-byte chunks per row
  const int S = a.S;
  const int nt = (S + 15) >> 4;                      // query / key tiles = waves of this block
  const int Sp16 = nt * 16, Sp32 = (S + 31) & ~31;
  const int VROW = Sp32 + LDS_PAD;                   // V^T image: [HD][VROW]
  bf16_t* Ks = (bf16_t*)smem;
  bf16_t* Vt = Ks + Sp16 * KROW;
  const int b = blockIdx.x / a.heads, h = blockIdx.x - b * a.heads;
  const bf16_t* qb = a.q + (long)b * a.bsq + h * HD;
  const bf16_t* kb = a.k + (long)b * a.bsk + h * HD;
  const bf16_t* vb = a.v + (long)b * a.bsv + h * HD;
  bf16_t* ob = a.o + (long)b * a.bso + h * HD;
  const int nthr = nt * 64;

  for (int c = threadIdx.x; c < Sp16 * CPR; c += nthr) {
    const int row = c / CPR, cc = c - row * CPR;
    u32x4 val = {0u, 0u, 0u, 0u};
    if (row < S) val = *(const u32x4*)(kb + (long)row * a.ldk + cc * 8);
    *(u32x4*)(Ks + row * KROW + cc * 8) = val;
  }
  for (int c = threadIdx.x; c < Sp32 * CPR; c += nthr) {
    const int cc = c / Sp32, row = c - cc * Sp32;    // consecutive lanes: consecutive keys of one 8-column chunk
    u32x4 val = {0u, 0u, 0u, 0u};
    if (row < S) val = *(const u32x4*)(vb + (long)row * a.ldv + cc * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(cc * 8 + e) * VROW + row] = (bf16_t)((val[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
  }

  const int lane = threadIdx.x & 63, qt = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int qr = qt * 16 + n;                        // this lane's query row
  bf16x8 qf[HD / 32];
#pragma unroll
  for (int ks = 0; ks < HD / 32; ++ks) {
    u32x4 val = {0u, 0u, 0u, 0u};
    if (qr < S) val = *(const u32x4*)(qb + (long)qr * a.ldq + ks * 32 + g * 8);
    qf[ks] = __builtin_bit_cast(bf16x8, val);
  }
  __syncthreads();

  float p[8][4];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    if (kt <= qt) {                                  // wave-uniform
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < HD / 32; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(Ks + (kt * 16 + n) * KROW + ks * 32 + g * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt * 16 + g * 4 + i;
        const bool on = key <= qr && key < S;
        p[kt][i] = on ? acc[i] * a.alpha : -INFINITY;
        m = fmaxf(m, p[kt][i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) p[kt][i] = -INFINITY;
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = p[kt][i] == -INFINITY ? 0.f : __expf(p[kt][i] - m);
      p[kt][i] = e;
      sum += e;
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;

  f32x4 oacc[HD / 16];
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (2 * u <= qt) {                               // wave-uniform; tile 2u + 1 may lie beyond qt: its probabilities are 0, its V^T columns zeros or real rows
      const u32x4 pw = {pack2_bf16(p[2 * u][0], p[2 * u][1]), pack2_bf16(p[2 * u][2], p[2 * u][3]),
                        pack2_bf16(p[2 * u + 1][0], p[2 * u + 1][1]), pack2_bf16(p[2 * u + 1][2], p[2 * u + 1][3])};
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) {
        const bf16_t* vr = Vt + (dt * 16 + n) * VROW + g * 4;
        const u32x2 lo = *(const u32x2*)(vr + (2 * u) * 16), hi = *(const u32x2*)(vr + (2 * u + 1) * 16);
        const u32x4 vw = {lo[0], lo[1], hi[0], hi[1]};
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vw), pf, oacc[dt], 0, 0, 0);
      }
    }
  }
  if (qr < S) {
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) {
      const u32x2 w = {pack2_bf16(oacc[dt][0] * inv, oacc[dt][1] * inv), pack2_bf16(oacc[dt][2] * inv, oacc[dt][3] * inv)};
      *(u32x2*)(ob + (long)qr * a.ldo + dt * 16 + g * 4) = w;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. causal softmax of [mats][S][ld] score matrices: row i keeps columns 0..i, every other column of [0, ld) is written as 0.
// y may be x (no __restrict__ on the pair): column c of a row is read and written by lane c & 63 alone, its last read before its store.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void causal_softmax_kernel(const T* x, T* y, long rows, int S, long ld) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cols = (int)(row % S) + 1;
  const T* xr = x + row * ld;
  T* yr = y + row * ld;
  float m = -INFINITY;
  for (int c = lane; c < cols; c += 64) m = fmaxf(m, Elem<T>::load(xr + c));
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += expf(Elem<T>::load(xr + c) - m);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int c = lane; c < (int)ld; c += 64) {
    const float v = c < cols ? expf(Elem<T>::load(xr + c) - m) * inv : 0.f;
    Elem<T>::store(yr + c, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. y = v * sigmoid(1.702 v), v = x + b[col]  (transformers QuickGELUActivation behind CLIPMLP.fc1); y may be x (no __restrict__ on
// the pair)
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bias_quick_gelu_kernel(const T* x, const float* __restrict__ b, T* y, long n, int cols) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = Elem<T>::load(x + i) + b[i % cols];
    const float s = 1.0f / (1.0f + expf(-(1.702f * v)));
    Elem<T>::store(y + i, v * s);
  }
}

// LayerNorm with weight AND bias (nn.LayerNorm: CLIPEncoderLayer.layer_norm1 / 2, final_layer_norm), f32 in, one wave per row:
// mean, then the variance of the centred values, then (x - mean) * rstd * w + b in one pass over the row
template <typename T>
__global__ __launch_bounds__(256) void layernorm_bias_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                             T* __restrict__ y, long rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * cols;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)cols;
  float q = 0.f;
  for (int c = lane; c < cols; c += 64) { const float t = xr[c] - mean; q = fmaf(t, t, q); }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)cols + eps);
  for (int c = lane; c < cols; c += 64) Elem<T>::store(y + row * cols + c, (xr[c] - mean) * rstd * w[c] + b[c]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. pooled position of every id row (transformers CLIPTextTransformer.forward): eos_token_id == 2 (the legacy rule) -> first position
// of the row maximum; else first position whose id is eos_token_id, 0 when there is none (what argmax of an all-zero row gives)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eos_index_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ idx, int64_t* __restrict__ flat,
                                                        int batch, int S, int64_t eos) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= batch) return;
  const int64_t* r = ids + (long)row * S;
  const bool legacy = eos == 2;
  int64_t best = INT64_MIN; int pos = 0x7fffffff;      // legacy: (largest id, first position); else: first match
  for (int c = lane; c < S; c += 64) {
    const int64_t v = r[c];
    if (legacy) { if (v > best) { best = v; pos = c; } }
    else if (v == eos && c < pos) pos = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t ov = __shfl_xor(best, o, 64); const int op = __shfl_xor(pos, o, 64);
    if (legacy) { if (ov > best || (ov == best && op < pos)) { best = ov; pos = op; } }
    else if (op < pos) pos = op;
  }
  if (lane == 0) {
    const int64_t at = pos == 0x7fffffff ? 0 : pos;
    idx[row] = at;
    if (flat) flat[row] = (int64_t)row * S + at;
  }
}

}  // namespace clip

extern "C" int muse_causal_attention_fwd(const muse_attn_desc* d, void* stream) {
  if (!d || !d->q || !d->k || !d->v || !d->o || d->batch < 0 || d->heads <= 0) return MUSE_ERR_BAD_ARG;
  if (d->seq_q != d->seq_kv || d->seq_q < 1 || d->seq_q > 128 || (d->head_dim != 32 && d->head_dim != 64)) return MUSE_ERR_UNSUPPORTED;
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->o) & 15) return MUSE_ERR_ALIGN;
  if ((d->ldq | d->ldk | d->ldv | d->ldo | d->bsq | d->bsk | d->bsv | d->bso) & 7) return MUSE_ERR_ALIGN;
  if (d->ldq < 0 || d->ldk < 0 || d->ldv < 0 || d->ldo < 0) return MUSE_ERR_BAD_ARG;
  if (d->batch == 0) return 0;
  const int S = d->seq_q, nt = (S + 15) >> 4, Sp32 = (S + 31) & ~31, HD = d->head_dim;
  const size_t lds = ((size_t)nt * 16 * (HD + clip::LDS_PAD) + (size_t)HD * (Sp32 + clip::LDS_PAD)) * sizeof(bf16_t);   // <= 35840 bytes
  const clip::AttnArgs a{(const bf16_t*)d->q, (const bf16_t*)d->k, (const bf16_t*)d->v, (bf16_t*)d->o, d->ldq, d->ldk, d->ldv, d->ldo,
                         d->bsq, d->bsk, d->bsv, d->bso, d->heads, S, d->alpha};
  const dim3 grid((unsigned)((long)d->batch * d->heads)), block(64 * nt);
  if (HD == 64) hipLaunchKernelGGL(clip::causal_attn_kernel<64>, grid, block, lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(clip::causal_attn_kernel<32>, grid, block, lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int muse_causal_softmax_fwd(const void* x, void* y, int32_t dtype, int64_t mats, int32_t seq, int64_t ld, void* stream) {
  if (mats <= 0 || seq <= 0) return 0;
  if (ld < seq || (dtype != MUSE_F32 && dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  const long rows = (long)mats * seq;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(clip::causal_softmax_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, (float*)y, rows, seq, (long)ld);
  else hipLaunchKernelGGL(clip::causal_softmax_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, rows, seq, (long)ld);
  return (int)hipGetLastError();
}

extern "C" int muse_bias_quick_gelu(const void* x, const float* bias, void* y, int32_t dtype, int64_t rows, int32_t cols, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (dtype != MUSE_F32 && dtype != MUSE_BF16) return MUSE_ERR_BAD_ARG;
  const long n = (long)rows * cols;
  const dim3 grid((unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(clip::bias_quick_gelu_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, bias, (float*)y, n, cols);
  else hipLaunchKernelGGL(clip::bias_quick_gelu_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, bias, (bf16_t*)y, n, cols);
  return (int)hipGetLastError();
}

extern "C" int muse_layernorm_bias_fwd(const float* x, const float* w, const float* b, void* y, int32_t y_dtype, int64_t rows, int32_t cols,
                                       float eps, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (y_dtype != MUSE_F32 && y_dtype != MUSE_BF16) return MUSE_ERR_BAD_ARG;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (y_dtype == MUSE_F32) hipLaunchKernelGGL(clip::layernorm_bias_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x, w, b, (float*)y, (long)rows, cols, eps);
  else hipLaunchKernelGGL(clip::layernorm_bias_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, x, w, b, (bf16_t*)y, (long)rows, cols, eps);
  return (int)hipGetLastError();
}

extern "C" int muse_eos_index(const int64_t* ids, int64_t* idx, int64_t* flat_idx, int32_t batch, int32_t seq, int64_t eos_token_id,
                              void* stream) {
  if (batch <= 0) return 0;
  if (seq <= 0) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(clip::eos_index_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, idx, flat_idx, batch, seq,
                     eos_token_id);
  return (int)hipGetLastError();
}
