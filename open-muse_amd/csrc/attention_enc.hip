// Fused one-tile self-attention of the frozen encoder towers, forward only: bf16 q / k / v / o, f32 softmax and accumulation, MFMA
// products.  ONE kernel body, two score policies:
//   Causal   muse_causal_attention_fwd  CLIP text tower (muse.CLIPTextEncoder): score = acc * alpha, key j takes part in query i iff j <= i
//   RelBias  muse_bias_attention_fwd    T5 encoder (muse.T5TextEncoder): score = acc + rel[head][j - i + S - 1], every key j < S takes part
// The whole sequence (<= 128 tokens) is ONE tile: a workgroup owns one (image, head), K and V^T live in LDS, wave w owns query rows
// 16 w .. 16 w + 15.  No online softmax, no S x S matrix in memory.
#include "common.h"
#include "../../include/muse_hip.h"

namespace enc {

// ---------------------------------------------------------------------------------------------------------------------------------
// Products as TRANSPOSES so that the score tile comes out of the first MFMA in the operand layout of the second:
//   S^T[key][query] = K Q^T   v_mfma_f32_16x16x32_bf16, A = K rows from LDS, B = Q rows from global memory (each read once)
//     -> lane (n = lane & 15, g = lane >> 4) holds S^T[16 kt + 4 g + i][query n], i = 0..3, for every key tile kt its wave takes
//   O^T[d][query]   = V^T P^T  the same MFMA over PAIRS of key tiles: k slot j of lane group g is key 16 (2u) + 4 g + j (j < 4) or
//     16 (2u + 1) + 4 g + j - 4 (j >= 4) - a permutation of the 32 keys of the pair, applied to both operands (the V^T fragment is two
//     8-byte LDS reads at those keys), so the lane's own probabilities are its B fragment with no lane movement.
// A pair is multiplied when the policy takes its FIRST tile; its second tile may lie beyond what the wave takes: its probabilities are
// 0 then, its V^T columns zeros or real rows.
// Never read: K / V rows and Q rows >= S are zero-filled registers / LDS, never memory reads (the last image's rows >= S lie outside
// the caller's allocation); the bias is read only for (query < S, key < S), i.e. inside the 2 S - 1 staged values.
// No NaN: a masked score is -INFINITY and its probability the literal 0.f (never exp of anything); every query row - padding rows too -
// sees key 0 under both policies, so its maximum is finite and its sum >= 1.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int LDS_PAD = 8;   // bf16 elements behind every LDS row (16 bytes: keeps 16-byte alignment, spreads rows over the banks)
constexpr int REL_MAX = 256; // floats of LDS for a head's 2 S - 1 <= 255 bias values

struct AttnArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
  long ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;
  int heads, S;
};

// A score policy: LDS_EXTRA bytes behind the two images; stage() fills them before the barrier; takes() - does this wave multiply key
// tile kt (qt: its own tile, nt: the block's tiles); score() - the softmax input of one (key, query qr), -INFINITY for a masked key.
// misaligned() is the host's check of the policy's own pointer, made between launch()'s pointer and stride checks so that the
// return codes keep their order.
// score() takes S by reference on purpose: a by-value int is `noundef`, the `&&` of the causal mask then folds into a bitwise and, and
// the compiler packs the 32 score multiplies in pairs (v_pk_mul_f32, one more VGPR) - the same bits, 0.1 % more time at S = 77.
struct Causal {
  float alpha;
  static constexpr size_t LDS_EXTRA = 0;
  bool misaligned() const { return false; }
  __device__ void stage(float*, int, int, int) const {}
  __device__ bool takes(int kt, int qt, int) const { return kt <= qt; }                       // wave-uniform
  __device__ float score(float acc, int key, int qr, const int& S, const float*) const {
    const bool on = key <= qr && key < S;
    return on ? acc * alpha : -INFINITY;
  }
};

struct RelBias {
  const float* rel;            // [heads][2 S - 1]
  static constexpr size_t LDS_EXTRA = REL_MAX * sizeof(float);
  bool misaligned() const { return (uintptr_t)rel & 3; }
  __device__ void stage(float* rels, int h, int S, int nthr) const {
    const float* relh = rel + (long)h * (2 * S - 1);
    for (int c = threadIdx.x; c < 2 * S - 1; c += nthr) rels[c] = relh[c];
  }
  __device__ bool takes(int kt, int, int nt) const { return kt < nt; }                        // block-uniform
  __device__ float score(float acc, int key, int qr, const int& S, const float* rels) const {
    const float* relq = rels + (S - 1 - qr);         // bias of key j: relq[j]; dereferenced only where qr < S and j < S
    const bool on = key < S;
    const float bias = (on && qr < S) ? relq[key] : 0.f;
    return on ? acc + bias : -INFINITY;
  }
};

template <int HD, class Score>
__global__ __launch_bounds__(512) void attn_kernel(const AttnArgs a, const Score sc) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KROW = HD + LDS_PAD;                 // K image: [Sp16][KROW]
  constexpr int CPR = HD / 8;                        // 16-byte chunks per row
  const int S = a.S;
  const int nt = (S + 15) >> 4;                      // query / key tiles = waves of this block
  const int Sp16 = nt * 16, Sp32 = (S + 31) & ~31;
  const int VROW = Sp32 + LDS_PAD;                   // V^T image: [HD][VROW]
  bf16_t* Ks = (bf16_t*)smem;
  bf16_t* Vt = Ks + Sp16 * KROW;
  float* extra = (float*)(Vt + HD * VROW);           // the policy's LDS_EXTRA bytes (both images are multiples of 16 bytes)
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
  sc.stage(extra, h, S, nthr);

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
    if (sc.takes(kt, qt, nt)) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < HD / 32; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(Ks + (kt * 16 + n) * KROW + ks * 32 + g * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[kt][i] = sc.score(acc[i], kt * 16 + g * 4 + i, qr, S, extra);
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
    if (sc.takes(2 * u, qt, nt)) {
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

template <class Score>
static int launch(const muse_attn_desc* d, const Score sc, void* stream) {
  if (!d || !d->q || !d->k || !d->v || !d->o || d->batch < 0 || d->heads <= 0) return MUSE_ERR_BAD_ARG;
  if (d->seq_q != d->seq_kv || d->seq_q < 1 || d->seq_q > 128 || (d->head_dim != 32 && d->head_dim != 64)) return MUSE_ERR_UNSUPPORTED;
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->o) & 15 || sc.misaligned()) return MUSE_ERR_ALIGN;
  if ((d->ldq | d->ldk | d->ldv | d->ldo | d->bsq | d->bsk | d->bsv | d->bso) & 7) return MUSE_ERR_ALIGN;
  if (d->ldq < 0 || d->ldk < 0 || d->ldv < 0 || d->ldo < 0) return MUSE_ERR_BAD_ARG;
  if (d->batch == 0) return 0;
  const int S = d->seq_q, nt = (S + 15) >> 4, Sp32 = (S + 31) & ~31, HD = d->head_dim;
  // <= 35840 bytes of images, + 1024 for RelBias
  const size_t lds = ((size_t)nt * 16 * (HD + LDS_PAD) + (size_t)HD * (Sp32 + LDS_PAD)) * sizeof(bf16_t) + Score::LDS_EXTRA;
  const AttnArgs a{(const bf16_t*)d->q, (const bf16_t*)d->k, (const bf16_t*)d->v, (bf16_t*)d->o, d->ldq, d->ldk, d->ldv, d->ldo,
                   d->bsq, d->bsk, d->bsv, d->bso, d->heads, S};
  const dim3 grid((unsigned)((long)d->batch * d->heads)), block(64 * nt);
  if (HD == 64) hipLaunchKernelGGL((attn_kernel<64, Score>), grid, block, lds, (hipStream_t)stream, a, sc);
  else hipLaunchKernelGGL((attn_kernel<32, Score>), grid, block, lds, (hipStream_t)stream, a, sc);
  return (int)hipGetLastError();
}

}  // namespace enc

extern "C" int muse_causal_attention_fwd(const muse_attn_desc* d, void* stream) {
  if (!d) return MUSE_ERR_BAD_ARG;
  return enc::launch(d, enc::Causal{d->alpha}, stream);
}

extern "C" int muse_bias_attention_fwd(const muse_attn_desc* d, const float* rel, void* stream) {
  if (!rel) return MUSE_ERR_BAD_ARG;
  return enc::launch(d, enc::RelBias{rel}, stream);
}
