// T5 text encoder (transformers T5EncoderModel: the `type: "t5"` text encoder of the reference's configs, loaded at
// training/train_muse.py:341-343 and called every step at :651 as `text_encoder(ids)[0]`) - the kernels it needs beyond the transformer
// and CLIP ones:
//   1. fused BIDIRECTIONAL self-attention with an additive relative-position bias, forward only: bf16 q / k / v / o, f32 softmax and
//      accumulation, MFMA products.  The one-tile design of clip::causal_attn_kernel (csrc/clip_text.hip): a workgroup owns one
//      (image, head), K and V^T live in LDS, wave w owns query rows 16 w .. 16 w + 15 - and here every key tile.  No score scale (T5
//      folds it into its initialisation), no mask; the bias of (query i, key j) is rel[head][j - i + S - 1], the head's 2 S - 1 values
//      staged in LDS.
//   2. bias + row softmax of materialised f32 score matrices (the exact-f32 mode at any length, both modes for 128 < S <= 512)
//   3. the gated tanh-GELU behind the packed wi_0 | wi_1 product
//   4. RMSNorm (T5LayerNorm) with a bf16 result: the f32 result is muse_norm_res_fwd mode 0 (csrc/uvit.hip)
//   5. rel[head][t] = relative_attention_bias.weight[bucket[t]][head], the bucket map computed on the host
#include "common.h"
#include "../../include/muse_hip.h"

namespace t5 {

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. fused attention with relative-position bias.  Products as TRANSPOSES, as in clip::causal_attn_kernel:
//   S^T[key][query] = K Q^T   v_mfma_f32_16x16x32_bf16, A = K rows from LDS, B = Q rows from global memory (each read once)
//     -> lane (n = lane & 15, g = lane >> 4) holds S^T[16 kt + 4 g + i][query n], i = 0..3, for every key tile kt
//   O^T[d][query]   = V^T P^T  the same MFMA over PAIRS of key tiles with the k slots permuted alike in both operands, so the lane's own
//     probabilities are its B fragment with no lane movement.
// Key j takes part in query i iff j < S.  A masked probability is the literal 0.f (never exp of anything); K / V rows and Q rows >= S
// are zero-filled registers / LDS, never memory reads (the last image's rows >= S lie outside the caller's allocation); the bias is
// read only for (query < S, key < S), i.e. inside the 2 S - 1 staged values; every query row - padding rows too - sees key 0, so its
// maximum is finite and its sum >= 1: no NaN anywhere.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int LDS_PAD = 8;   // bf16 elements behind every LDS row (16 bytes: keeps 16-byte alignment, spreads rows over the banks)
constexpr int REL_MAX = 256; // floats of LDS for the head's 2 S - 1 <= 255 bias values

struct AttnArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
  const float* rel;
  long ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;
  int heads, S;
};

template <int HD>
__global__ __launch_bounds__(512) void bias_attn_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KROW = HD + LDS_PAD;                 // K image: [Sp16][KROW]
  constexpr int CPR = HD / 8;                        // 16-byte chunks per row
  const int S = a.S;
  const int nt = (S + 15) >> 4;                      // query / key tiles = waves of this block
  const int Sp16 = nt * 16, Sp32 = (S + 31) & ~31;
  const int VROW = Sp32 + LDS_PAD;                   // V^T image: [HD][VROW]
  bf16_t* Ks = (bf16_t*)smem;
  bf16_t* Vt = Ks + Sp16 * KROW;
  float* rels = (float*)(Vt + HD * VROW);            // (both images are multiples of 16 bytes)
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
  const float* relh = a.rel + (long)h * (2 * S - 1);
  for (int c = threadIdx.x; c < 2 * S - 1; c += nthr) rels[c] = relh[c];

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

  const float* relq = rels + (S - 1 - qr);           // bias of key j: relq[j]; dereferenced only where qr < S and j < S
  float p[8][4];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    if (kt < nt) {                                   // block-uniform
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < HD / 32; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(Ks + (kt * 16 + n) * KROW + ks * 32 + g * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt * 16 + g * 4 + i;
        const bool on = key < S;
        const float bias = (on && qr < S) ? relq[key] : 0.f;
        p[kt][i] = on ? acc[i] + bias : -INFINITY;
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
    if (2 * u < nt) {                                // block-uniform; tile 2u + 1 may lie beyond nt: its probabilities are 0, its V^T columns zeros
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
// 2. bias + softmax of [mats][S][ld] f32 score matrices: row i of matrix z becomes softmax_j(x[i][j] + rel[z % heads][j - i + S - 1])
// over j < S, columns [S, ld) are written as 0.  One wave per row.  y (f32, may be NULL) may be x (no __restrict__ on the pair): column
// c of a row is read and written by lane c & 63 alone, its last read before its store.  yb (may be NULL): the same values rounded to
// bf16, same ld - the A operand of the second product of the bf16 mode.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bias_softmax_kernel(const float* x, float* y, bf16_t* __restrict__ yb, const float* __restrict__ rel,
                                                           long rows, int S, long ld, int heads) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long mat = row / S;
  const int i = (int)(row - mat * S);
  const float* xr = x + row * ld;
  const float* br = rel + (mat % heads) * (2 * S - 1) + (S - 1 - i);
  float m = -INFINITY;
  for (int c = lane; c < S; c += 64) m = fmaxf(m, xr[c] + br[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < S; c += 64) s += expf(xr[c] + br[c] - m);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int c = lane; c < (int)ld; c += 64) {
    const float v = c < S ? expf(xr[c] + br[c] - m) * inv : 0.f;
    if (y) y[row * ld + c] = v;
    if (yb) yb[row * ld + c] = f32_to_bf16(v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. y[r][c] = gelu_new(ab[r][c]) * ab[r][F + c]  (transformers NewGELUActivation on wi_0, times wi_1: T5 v1.1's "gated-gelu").  The
// expression is F.gelu(approximate="tanh")'s, operation for operation, in f32.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_tanh(float x) {
  const float x3 = x * x * x;
  const float inner = 0.79788456080286535588f * (x + 0.044715f * x3);     // sqrt(2 / pi)
  return 0.5f * x * (1.0f + tanhf(inner));
}

template <typename T>
__global__ __launch_bounds__(256) void gated_gelu_tanh_kernel(const T* __restrict__ ab, T* __restrict__ y, long rows, int F) {
  const long n = rows * F;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / F;
    const int c = (int)(i - r * F);
    const T* row = ab + r * 2 * F;
    const float g = gelu_tanh(Elem<T>::load(row + c));
    Elem<T>::store(y + i, g * Elem<T>::load(row + F + c));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4. y = bf16(x * rsqrt(mean(x^2) + eps) * w), x f32 [rows, cols], one wave per row: the expressions of norm_res_fwd_kernel mode 0
// (csrc/uvit.hip), whose result is f32 only
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmsnorm_bf16_kernel(const float* __restrict__ x, const float* __restrict__ w, bf16_t* __restrict__ y,
                                                           long rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * cols;
  float q = 0.f;
  for (int c = lane; c < cols; c += 64) q = fmaf(xr[c], xr[c], q);
  const float rstd = rsqrtf(wave_sum(q) / (float)cols + eps);
  for (int c = lane; c < cols; c += 64) y[row * cols + c] = f32_to_bf16(xr[c] * rstd * w[c]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 5. rel[h][t] = table[bucket[t]][h]: table = relative_attention_bias.weight [buckets, heads], t = the signed distance j - i + S - 1
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rel_bias_gather_kernel(const float* __restrict__ table, const int64_t* __restrict__ bucket,
                                                              float* __restrict__ rel, int heads, int n, int buckets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= heads * n) return;
  const int h = i / n, t = i - h * n;
  const int64_t b = bucket[t];
  rel[i] = (b >= 0 && b < buckets) ? table[b * heads + h] : 0.f;
}

}  // namespace t5

extern "C" int muse_bias_attention_fwd(const muse_attn_desc* d, const float* rel, void* stream) {
  if (!d || !d->q || !d->k || !d->v || !d->o || !rel || d->batch < 0 || d->heads <= 0) return MUSE_ERR_BAD_ARG;
  if (d->seq_q != d->seq_kv || d->seq_q < 1 || d->seq_q > 128 || (d->head_dim != 32 && d->head_dim != 64)) return MUSE_ERR_UNSUPPORTED;
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->o) & 15) return MUSE_ERR_ALIGN;
  if ((uintptr_t)rel & 3) return MUSE_ERR_ALIGN;
  if ((d->ldq | d->ldk | d->ldv | d->ldo | d->bsq | d->bsk | d->bsv | d->bso) & 7) return MUSE_ERR_ALIGN;
  if (d->ldq < 0 || d->ldk < 0 || d->ldv < 0 || d->ldo < 0) return MUSE_ERR_BAD_ARG;
  if (d->batch == 0) return 0;
  const int S = d->seq_q, nt = (S + 15) >> 4, Sp32 = (S + 31) & ~31, HD = d->head_dim;
  const size_t lds = ((size_t)nt * 16 * (HD + t5::LDS_PAD) + (size_t)HD * (Sp32 + t5::LDS_PAD)) * sizeof(bf16_t)
                     + t5::REL_MAX * sizeof(float);                                                               // <= 36864 bytes
  const t5::AttnArgs a{(const bf16_t*)d->q, (const bf16_t*)d->k, (const bf16_t*)d->v, (bf16_t*)d->o, rel, d->ldq, d->ldk, d->ldv, d->ldo,
                       d->bsq, d->bsk, d->bsv, d->bso, d->heads, S};
  const dim3 grid((unsigned)((long)d->batch * d->heads)), block(64 * nt);
  if (HD == 64) hipLaunchKernelGGL(t5::bias_attn_kernel<64>, grid, block, lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(t5::bias_attn_kernel<32>, grid, block, lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int muse_bias_softmax_fwd(const float* x, float* y, void* y_bf16, const float* rel, int64_t mats, int32_t heads, int32_t seq,
                                     int64_t ld, void* stream) {
  if (mats <= 0 || seq <= 0) return 0;
  if (!x || !rel || (!y && !y_bf16) || heads <= 0 || ld < seq) return MUSE_ERR_BAD_ARG;
  const long rows = (long)mats * seq;
  hipLaunchKernelGGL(t5::bias_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (bf16_t*)y_bf16, rel,
                     rows, seq, (long)ld, heads);
  return (int)hipGetLastError();
}

extern "C" int muse_gated_gelu_tanh(const void* ab, void* y, int32_t dtype, int64_t rows, int32_t cols, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!ab || !y || (dtype != MUSE_F32 && dtype != MUSE_BF16)) return MUSE_ERR_BAD_ARG;
  const dim3 grid((unsigned)ew_grid((long)rows * cols));
  if (dtype == MUSE_F32) hipLaunchKernelGGL(t5::gated_gelu_tanh_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)ab, (float*)y, (long)rows, cols);
  else hipLaunchKernelGGL(t5::gated_gelu_tanh_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)ab, (bf16_t*)y, (long)rows, cols);
  return (int)hipGetLastError();
}

extern "C" int muse_rmsnorm_bf16_fwd(const float* x, const float* w, void* y, int64_t rows, int32_t cols, float eps, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!x || !w || !y) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(t5::rmsnorm_bf16_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, w, (bf16_t*)y, (long)rows,
                     cols, eps);
  return (int)hipGetLastError();
}

extern "C" int muse_rel_bias_gather(const float* table, const int64_t* bucket, float* rel, int32_t heads, int32_t n, int32_t buckets,
                                    void* stream) {
  if (heads <= 0 || n <= 0) return 0;
  if (!table || !bucket || !rel || buckets <= 0) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(t5::rel_bias_gather_kernel, dim3((unsigned)((heads * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, bucket, rel,
                     heads, n, buckets);
  return (int)hipGetLastError();
}
