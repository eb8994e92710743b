/* libmuse_hip — C-ABI of the MI355X (gfx950) kernels behind the open-muse MaskGit hot path.
 *
 * The reference (huggingface/open-muse) has no first-party native code: its hot path reaches native kernels only
 * through torch / xformers / apex / flash_attn call sites.  Each entry point below names
 * the reference call site it replaces (paths relative to the reference repo root).  INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates; the library holds no memory);
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and never synchronises;
 *   - return 0 on success, a hipError_t (> 0) for launch errors, or a negative MUSE_ERR_* for argument errors;
 *   - bf16 tensors are raw uint16 storage; "f32" is IEEE binary32; indices are int64 like torch.long;
 *   - activations are row-major [tokens, features] (transformer) or NHWC (VQGAN).
 */
#ifndef MUSE_HIP_H
#define MUSE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MUSE_F32 = 0, MUSE_BF16 = 1, MUSE_F16 = 2 /* IEEE half: GEMM operands only (muse_gemm, muse_gemm_group) */ };
enum { MUSE_ERR_BAD_ARG = -1, MUSE_ERR_ALIGN = -2, MUSE_ERR_UNSUPPORTED = -3 };

int muse_version(void); /* ABI version of this header */

/* ------------------------------------------------------------------------------------------------------------
 * muse_gemm — C = epilogue(alpha * A * B^T), strided-batched, MFMA (bf16: v_mfma_f32_16x16x32_bf16,
 * f32: v_mfma_f32_16x16x4_f32 = exact fp32 fma chain).
 * layout_x = 0: X(r,k) at X + r*ld + k ("k-contiguous", the nn.Linear weight layout);
 * layout_x = 1: X(r,k) at X + k*ld + r ("k-major", the transposed view backward needs).
 * Replaces: every nn.Linear on the path (muse/modeling_transformer.py:198-200,218,789-798,979-984) and their
 * autograd backward, torch.baddbmm / torch.matmul of Attention.attention (:226-238), and the VQ addmm
 * (muse/modeling_maskgit_vqgan.py:310-315, via rowvec/bias: C = (zn[m] + en[n]) - 2 z.e).
 * Batch index z in [0,batch) addresses X + (z / zdiv) * sX0 + (z % zdiv) * sX1  (e.g. (image, head)).
 * Requirements: A, B 16-byte aligned; lda/ldb and batch strides multiples of 16 bytes; for a k-contiguous operand
 * with K % (16/elsize) != 0 the row must be physically padded with zeros up to the next 16-byte chunk.
 * dtype MUSE_F16 (round 6): IEEE-half operands on v_mfma_f32_16x16x32_f16 with f32 accumulation and f32 output - 11 significant bits
 * per operand = the TF32 operand format `enable_tf32` of configs/cc12m_uvit_clip.yaml:103 multiplies in (gfx950 has no xf32 MFMA), at
 * the bf16 matrix rate; the narrower exponent is the caller's business (muse_cast_f32_to_f16 scales by a power of two, alpha undoes
 * it).  Only the 256 x 256 LDS-DMA kernels carry it: M, N >= 128, K >= 64, no activation, batch / split_k as for bf16 operands with
 * f32 output; anything else MUSE_ERR_UNSUPPORTED (muse_gemm_tile says so beforehand).
 */
typedef struct muse_gemm_desc {
  const void* A;
  const void* B;
  void* C;
  const void* bias;     /* f32 [N] or NULL: added per output column                       */
  const void* rowvec;   /* f32 [M] or NULL: added per output row                          */
  const void* residual; /* out_dtype [M, ldr] or NULL: added after the activation         */
  int32_t dtype;        /* MUSE_F32 | MUSE_BF16 | MUSE_F16 (A and B)                       */
  int32_t out_dtype;    /* MUSE_F32 | MUSE_BF16 (bf16 only with bf16 inputs)               */
  int32_t layout_a, layout_b;
  int32_t M, N, K;
  int32_t batch, zdiv;
  int64_t lda, ldb, ldc, ldr;
  int64_t sA0, sA1, sB0, sB1, sC0, sC1;
  float alpha;
  int32_t accumulate; /* C += ...                                                          */
  int32_t act;        /* 0 none, 1 erf-GELU (F.gelu)                                       */
  int32_t split_k;    /* > 1: K is cut into that many slices (f32 output, no epilogue extras)                    */
  int64_t split_stride; /* != 0: slice s stores its partial result at C + s*split_stride elements (workspace, plain
                         stores; reduce with muse_sum_slices - deterministic); == 0: slices are added to C with hardware
                         f32 atomics, the caller pre-initialises C (zeros, or the value to accumulate into)          */
} muse_gemm_desc;
int muse_gemm(const muse_gemm_desc* d, void* stream);
/* Block-tile edge muse_gemm will use for this descriptor: 256 (LDS-DMA kernel, one block per CU) or 128 (two / three
 * blocks per CU); < 0 = the error muse_gemm would return.  Host code sizes split_k with it (ops.wgrad_splits). */
int muse_gemm_tile(const muse_gemm_desc* d);
/* The f32-class "bf16x3" product as ONE kernel on four bf16 operand planes: C = alpha (A_hi B_hi^T + A_hi B_lo^T + A_lo B_hi^T) with f32
 * accumulation, where x ~= hi + lo (muse_split_f32_to_bf16x2; 2^-16 relative per product: at or above the TF32 products
 * configs/cc12m_uvit_clip.yaml:102-103 trains with).  d describes the product as for muse_gemm with dtype MUSE_BF16, out_dtype MUSE_F32,
 * A / B = the hi planes; the lo planes sit a_lo / b_lo ELEMENTS behind them with the same leading dimensions (multiples of 8).  Every
 * layout, bias / rowvec / residual / accumulate, split_k through a workspace; batch 1, no activation, M, N >= 128, K >= 64 and the
 * 256-tile kernel's alignment rules - otherwise MUSE_ERR_UNSUPPORTED (the caller runs three muse_gemm products or one over
 * K-concatenated operands, muse_split_f32_to_bf16_cat3). */
int muse_gemm_x3(const muse_gemm_desc* d, int64_t a_lo, int64_t b_lo, void* stream);
/* Kernel form behind that tile: 128, 256 (launch-per-tile LDS-DMA kernel) or 257 (the persistent tile-walking form of the 256 kernel,
 * csrc/gemm256p.h: bf16 operands, one batch, no split-K, no bias / activation; k-contiguous A); < 0 = muse_gemm's error.  Pure host
 * logic (tests assert that the train step's products take the persistent form; MUSE_G256P=0 turns it off). */
int muse_gemm_path(const muse_gemm_desc* d);

/* GROUPED weight gradients: n <= 8 products C_i[M_i, N_i] = A_i^T B_i (layout_a = layout_b = 1: k-major bf16 operands, k = the token
 * dimension; f32 output; the four dW = dY^T X of a transformer layer, muse/modeling_transformer.py:770-778,973-977 under autograd)
 * in ONE launch of the 256^2 LDS-DMA kernel over the concatenated tile lists.  `split_k` (the same for every product) cuts K into
 * slices written to C_i + s * split_stride_i (reduce with muse_sum_multi: deterministic); split_k = 1 writes (or, accumulate = 1,
 * adds to) C_i directly.  muse_gemm_group_ok: 0 if muse_gemm_group would take the list, else the error it would return (products
 * the 256^2 kernel does not take: MUSE_ERR_UNSUPPORTED - the caller then uses muse_gemm per product). */
int muse_gemm_group_ok(const muse_gemm_desc* d, int32_t n, int32_t split_k);
int muse_gemm_group(const muse_gemm_desc* d, int32_t n, int32_t split_k, void* stream);

/* 2-D transpose out[c, r] = in[r, c] (strided-batched); used only by the fallback that feeds k-major operands to
 * the k-contiguous GEMM path (MUSE_GEMM_TR=0).  More than 65535 row tiles of 32, or more than 65535 matrices: MUSE_ERR_UNSUPPORTED
 * before a launch.  65535 is this library's own limit for gridDim.y / .z (the portable one), not a figure asked of the runtime, which
 * may accept more. */
int muse_transpose(const void* in, void* out, int32_t dtype, int32_t rows, int32_t cols, int64_t ld_in, int64_t ld_out,
                   int32_t batch, int64_t stride_in, int64_t stride_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Transformer element/row kernels.
 * muse_layernorm_fwd: y = LayerNorm(x) * w (+ residual), weight-only LN (muse/modeling_transformer.py:124-137 at
 *   :878,:883,:786,:796,:1269,:983) with the residual add of :884 / :903 fused.  mean/rstd [rows] f32 are saved.
 * muse_layernorm_bwd: dx = LN'(dy) (+ dres);  dw_partial [nblk, cols] f32 holds per-block column sums of dy*xhat,
 *   reduced into dw by muse_colsum (deterministic two-stage reduction).  dx_bf16 (may be NULL): a second, bf16 copy of dx
 *   for the GEMMs that consume it next (the f32 dx stays the residual-stream gradient).
 */
int muse_layernorm_fwd(const void* x, int32_t x_dtype, const float* w, const float* residual, void* y, int32_t y_dtype,
                       float* mean, float* rstd, int32_t rows, int32_t cols, float eps, void* stream);
int muse_layernorm_bwd(const void* dy, int32_t dy_dtype, const void* x, int32_t x_dtype, const float* w,
                       const float* mean, const float* rstd, const float* dres, void* dx, int32_t dx_dtype,
                       void* dx_bf16, float* dw_partial, int32_t nblk, int32_t rows, int32_t cols, void* stream);
int muse_layernorm_bwd_nblk(int32_t rows);
/* The two back-to-back LayerNorms of a NormFormer layer (muse/modeling_transformer.py:882-884 then :785-789) in one pass:
 *   fwd: x1 = x + LN(ao) * w_post (f32) ; ln2 = LN(x1) * w_pre (bf16); statistics of both rows.   ao bf16 [rows, cols], cols <= 1024.
 *   bwd: dx1 = LN_pre'(dln2) + dres (f32) ; dao = LN_post'(dx1) (bf16); dw partials [nblk, cols] for both weights
 *        (nblk = muse_layernorm_bwd_nblk(rows), reduced by muse_colsum).
 * Bit-identical to two muse_layernorm_fwd / _bwd calls; saves the write + re-read of x1 / dx1. */
int muse_layernorm_pair_fwd(const void* ao, const float* x, const float* w_post, const float* w_pre, float* x1, void* ln2,
                            float* mean_post, float* rstd_post, float* mean_pre, float* rstd_pre, int32_t rows, int32_t cols,
                            float eps, void* stream);
int muse_layernorm_pair_bwd(const void* dln2, const float* x1, const float* w_pre, const float* mean_pre, const float* rstd_pre,
                            const float* dres, const void* ao, const float* w_post, const float* mean_post, const float* rstd_post,
                            float* dx1, void* dao, float* dw_partial_pre, float* dw_partial_post, int32_t nblk, int32_t rows,
                            int32_t cols, void* stream);
/* out[c] (+)= sum_r in[r, c], f32 */
int muse_colsum(const float* in, float* out, int32_t rows, int32_t cols, int32_t accumulate, void* stream);
/* Biases of `use_bias=True` models (muse/modeling_transformer.py:130 LayerNorm bias, :170-176 / :770-778 / :973-977 / :1155
 * nn.Linear biases; the Linear bias itself rides in muse_gemm's `bias` epilogue):
 *   muse_add_rowvec: x[r, c] += b[c], f32 in place (the LayerNorm bias behind muse_norm_res_fwd / muse_layernorm_fwd).
 *   muse_bias_grad_partial: partial[k, c] = sum of dy[r, c] over the k-th chunk of muse_bias_grad_rows_per_block() rows (dy f32 or
 *   bf16 with row stride ld); muse_colsum over the ceil(rows / R) partial rows gives d(bias), in a fixed order. */
int muse_add_rowvec(float* x, const float* b, int64_t rows, int32_t cols, void* stream);
int muse_bias_grad_rows_per_block(void);
int muse_bias_grad_partial(const void* dy, int32_t dtype, float* partial, int64_t rows, int32_t cols, int64_t ld, void* stream);

/* softmax over the last dim of [rows, ld] (first `cols` valid, pad columns written as 0), in place capable.
 * Replaces F.softmax at muse/modeling_transformer.py:236.  bwd: ds = p * (dp - sum(p*dp)). */
int muse_softmax_fwd(const void* x, void* y, int32_t dtype, int64_t rows, int32_t cols, int64_t ld, void* stream);
int muse_softmax_bwd(const void* p, const void* dp, void* ds, int32_t dtype, int64_t rows, int32_t cols, int64_t ld,
                     void* stream);

/* Fused full-visibility attention (bf16 in/out, f32 softmax / accumulation), head_dim in {16,32,48,64}, any query and
 * key length: replaces Attention.attention (muse/modeling_transformer.py:221-241: baddbmm -> softmax -> matmul), the
 * xformers memory_efficient_attention seam (:206-210; muse/modeling_transformer_v2.py:881-889, self- and cross-attention)
 * and their autograd backward, without materialising the S x S matrix.  K / V stream through LDS in tiles of <= 288 keys
 * (online softmax across tiles), so seq 257 / 256 / 1024 and the 77-token text cross-attention run on the same kernels.
 * Token t of image b, head h of tensor X lives at X + b*bsX + t*ldX + h*head_dim (elements); all strides multiples of 8.
 * lse / dsum are f32 [batch*heads, muse_attention_seq_pad(seq_q)].  alpha = 1/sqrt(head_dim) (the baddbmm alpha, :168,:230). */
typedef struct muse_attn_desc {
  const void* q;
  const void* k;
  const void* v;
  void* o;                       /* forward output (ctx); read by the backward */
  int64_t ldq, ldk, ldv, ldo;    /* elements between consecutive tokens        */
  int64_t bsq, bsk, bsv, bso;    /* elements between consecutive images        */
  int32_t batch, heads, head_dim, seq_q, seq_kv;
  float alpha;
} muse_attn_desc;
int muse_attention_seq_pad(int32_t seq);
int muse_attention_fwd_ex(const muse_attn_desc* d, float* lse, void* stream);
/* backward: d_o = upstream gradient of o; writes dq / dk / dv (bf16, own strides) and the scratch row constants dsum */
int muse_attention_bwd_ex(const muse_attn_desc* d, const void* d_o, int64_t lddo, int64_t bsdo, const float* lse, float* dsum,
                          void* dq, int64_t lddq, int64_t bsdq, void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv,
                          int64_t bsdv, void* stream);
/* The same with nn.Dropout on the attention probabilities (muse/modeling_transformer.py:237) applied inside the kernels: no
 * probability tensor and no mask tensor exist.  The keep bit of (image * heads + head = bh, query q, key k) is the bit
 * muse_dropout(seed, offset) produces for flat element e = (bh * seq_q + q) * ld_mask + k of a [batch*heads, seq_q, ld_mask] tensor
 * (Philox block offset + (e >> 2), word e & 3, kept iff u >= p), so with ld_mask = the materialised route's row pitch (seq_kv rounded
 * up to 8) both routes drop the same elements.  ld_mask: a multiple of 4, >= seq_kv.  Arithmetic: lse and the softmax row sum use the
 * undropped P; o = sum_k bf16(P keep / (1 - p)) v (one rounding of the f32 product); backward dsum = sum_d d_o o,
 * dS = P (keep / (1 - p) dP - dsum), dV = bf16(P keep / (1 - p))^T d_o.  The backward is given the same (p, seed, offset, ld_mask).
 * p == 0 is muse_attention_fwd_ex / _bwd_ex (bit-identical); p < 0, p >= 1 or a bad ld_mask: MUSE_ERR_BAD_ARG. */
int muse_attention_drop_fwd_ex(const muse_attn_desc* d, float* lse, float p, uint64_t seed, uint64_t offset, int64_t ld_mask,
                               void* stream);
int muse_attention_drop_bwd_ex(const muse_attn_desc* d, const void* d_o, int64_t lddo, int64_t bsdo, const float* lse, float* dsum,
                               void* dq, int64_t lddq, int64_t bsdq, void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv,
                               int64_t bsdv, float p, uint64_t seed, uint64_t offset, int64_t ld_mask, void* stream);
/* The same seam for the "bf16x3" compute mode (f32 tensors, TF32-class products: configs/cc12m_uvit_clip.yaml:102-103 trains with
 * mixed_precision "no" + enable_tf32): q / k / v / o / d_o / dq / dk / dv are FLOAT tensors (strides in elements, multiples of 4),
 * every product of the forward and the backward is three bf16 MFMA products of (hi, lo) operand planes the kernel makes itself
 * (<= 2^-16 relative per product), softmax and accumulation in f32.  head_dim 64, seq_q = 256, seq_kv in 225..256 or 65..96
 * (self-attention of config 4's 16 x 16 grid; its 77 text states); anything else: MUSE_ERR_UNSUPPORTED (the caller keeps the
 * materialised route: muse_gemm batched + muse_softmax_*).  lse is f32 [batch*heads, 256]. */
int muse_attention_x3_fwd(const muse_attn_desc* d, float* lse, void* o_planes, int64_t o_lo, int32_t half, float scale, int32_t* stats,
                          void* stream);
int muse_attention_x3_bwd(const muse_attn_desc* d, const void* d_o, int64_t lddo, int64_t bsdo, const float* lse, void* dq,
                          int64_t lddq, int64_t bsdq, void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv, int64_t bsdv,
                          void* dq_planes, int64_t dq_lo, void* dk_planes, int64_t dk_lo, void* dv_planes, int64_t dv_lo, int32_t half,
                          float scale, int32_t* stats, void* stream);
/* (dq / dk / dv may be NULL when their planes are given: a gradient that only weight GEMMs read exists as planes alone.)
 * (*_planes, optional: the result ALSO as the bf16 operand planes of the products that read it - muse_gemm_x3 - so that no split pass
 *  runs over it: the hi plane is addressed exactly like the f32 tensor (same strides, in elements), the lo plane sits *_lo elements
 *  behind it; NULL = f32 only) */
/* muse_attention_x3_fwd / _bwd with nn.Dropout(p) on the probabilities applied inside the kernels (the bf16x3 / f16 modes' counterpart of
 * muse_attention_drop_fwd_ex / _bwd_ex; the same mask contract): the keep bit of (bh, query q, key k) of this launch is the bit
 * muse_dropout(seed, offset) produces for flat element (bh * sq_total + q0 + q) * ld_mask + k0 + k of the FULL-sequence
 * [batch * heads, sq_total, ld_mask] mask - q0 / k0 are the global indices of the launch's first query / key, so the block-by-block routes of
 * the longer sequences (256-query blocks against <= 96 text states; block pairs merged by their log-sum-exps) draw the full-sequence mask.
 * Row maximum, row sum and lse use the undropped P; P keep / (1 - p) is formed in f32, then split into planes / converted to half;
 * backward: dsum = dO . O of the (dropped) final context, dP_eff = keep / (1 - p) dP in f32, dS = P (dP_eff - dsum), dV from the dropped P.
 * ld_mask % 4 == 0, k0 % 4 == 0, k0 + seq_kv <= ld_mask, q0 + seq_q <= sq_total, 0 <= p < 1: else MUSE_ERR_BAD_ARG. */
int muse_attention_x3_drop_fwd(const muse_attn_desc* d, float* lse, void* o_planes, int64_t o_lo, float p, uint64_t seed, uint64_t offset,
                               int64_t ld_mask, int64_t q0, int64_t k0, int64_t sq_total, int32_t half, float scale, int32_t* stats, void* stream);
int muse_attention_x3_drop_bwd(const muse_attn_desc* d, const void* d_o, int64_t lddo, int64_t bsdo, const float* lse, void* dq, int64_t lddq,
                               int64_t bsdq, void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv, int64_t bsdv, void* dq_planes,
                               int64_t dq_lo, void* dk_planes, int64_t dk_lo, void* dv_planes, int64_t dv_lo, float p, uint64_t seed,
                               uint64_t offset, int64_t ld_mask, int64_t q0, int64_t k0, int64_t sq_total, int32_t half, float scale,
                               int32_t* stats, void* stream);
/* Streaming forms for sequences of whole 256-row blocks on BOTH sides (round 6: the self-attention of BASELINE config 4's 1024 tokens;
 * reference modeling_transformer_v2.py:881-915).  d describes the FULL sequences (seq_q, seq_kv multiples of 256, head_dim 64; batch
 * strides of the whole tensors).  _fwd_stream: a workgroup keeps 256 queries and streams the key blocks through LDS with an online
 * softmax - context and lse [seq_q/256][batch*heads][256] written once (o_planes as for muse_attention_x3_fwd).  _bwd_stream: dQ per
 * query block over the streamed key blocks (it also writes dO.O per query into dsum, a workspace shaped like lse), then dK / dV per
 * key block over the streamed query blocks; every gradient written once (f32 and / or operand images, as for muse_attention_x3_bwd). */
int muse_attention_x3_fwd_stream(const muse_attn_desc* d, float* lse, void* o_planes, int64_t o_lo, int32_t half, float scale,
                                 int32_t* stats, void* stream);
int muse_attention_x3_bwd_stream(const muse_attn_desc* d, const float* d_o, int64_t lddo, int64_t bsdo, const float* lse, float* dsum,
                                 float* dq, int64_t lddq, int64_t bsdq, float* dk, int64_t lddk, int64_t bsdk, float* dv, int64_t lddv,
                                 int64_t bsdv, void* dq_planes, int64_t dq_lo, void* dk_planes, int64_t dk_lo, void* dv_planes, int64_t dv_lo,
                                 int32_t half, float scale, int32_t* stats, void* stream);
/* Block-by-block form of the longer sequences (round 6; reference modeling_transformer_v2.py:757-792 at the 1024 tokens of BASELINE config 4):
 * muse_attention_x3_fwd / _bwd run per (256 query rows, <= 256 keys) block pair, these two put the pieces together.
 * _merge: part[j] [batch*seq, heads*64] f32 (j < nk <= 8, part_stride elements apart) = key block j's softmax times its values, lp[j]
 *   [seq/256][batch*heads][256] (lp_stride apart) its log-sum-exp: lse = log sum_j exp(lp_j), out = sum_j exp(lp_j - lse) part_j; writes out,
 *   lse [seq/256][batch*heads][256] and optionally out's (hi, lo) bf16 operand planes (out_planes, lo plane out_lo elements behind).
 * muse_sum_parts_strided: out[r, 0..cols) (row pitch ldo, += when accumulate) = sum over j < n of parts[j*part_stride + r*cols + c]. */
int muse_attention_x3_merge(const float* part, int64_t part_stride, const float* lp, int64_t lp_stride, int32_t nk, float* out, float* lse,
                            void* out_planes, int64_t out_lo, int32_t batch, int32_t seq, int32_t heads, int32_t half, float scale,
                            int32_t* stats, void* stream);
int muse_sum_parts_strided(const float* parts, int64_t part_stride, int32_t n, int64_t rows, int32_t cols, float* out, int64_t ldo,
                           int32_t accumulate, void* stream);
/* packed self-attention: qkv [B*S, 3*H] (q | k | v, H = heads*head_dim: the fused QKV projection), ctx [B*S, H], dqkv [B*S, 3*H] */
int muse_attention_fwd(const void* qkv, void* ctx, float* lse, int32_t batch, int32_t seq, int32_t heads,
                       int32_t head_dim, float alpha, void* stream);
int muse_attention_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* dsum, void* dqkv,
                       int32_t batch, int32_t seq, int32_t heads, int32_t head_dim, float alpha, void* stream);

/* GLU: h = gelu_erf(a) * b with ab = [rows, 2*inter] (a = first half).  muse/modeling_transformer.py:789-792. */
int muse_glu_fwd(const void* ab, void* h, int32_t dtype, int64_t rows, int32_t inter, void* stream);
int muse_glu_bwd(const void* ab, const void* dh, void* dab, int32_t dtype, int64_t rows, int32_t inter, void* stream);
/* The f32 GLU of the "bf16x3" compute mode: the same f32 results, written ALSO as the (hi, lo) bf16 operand planes muse_gemm_x3 reads
 * (planes = [2][rows][cols] bf16, hi plane first; the bits muse_split_f32_to_bf16x2 would produce from the f32 result).  h / dab may be
 * NULL: planes only (a result that nothing but weight GEMMs reads - the GLU output and its input gradient inside an MLP). */
int muse_glu_fwd_x3(const float* ab, float* h, void* planes, int64_t rows, int32_t inter, int32_t half, float scale, int32_t* stats,
                    void* stream);
int muse_glu_bwd_x3(const float* ab, const float* dh, float* dab, void* planes, int64_t rows, int32_t inter, int32_t half, float scale,
                    int32_t* stats, void* stream);
/* GLU followed by nn.Dropout (MaskGiTUViT's `hidden_dropout`, reference muse/modeling_transformer_v2.py:933,947) in ONE pass: the keep
 * bit of element r * inter + c of the [rows, inter] result is the bit muse_dropout(seed, offset) produces for that flat element (Philox
 * block offset + (e >> 2), word e & 3, kept iff u >= p; scale 1 / (1 - p) in f32).  forward: h = keep * s * (gelu_erf(a) * b), one f32
 * product before the output rounding / the plane split / the half image;  backward: keep * s * dh in f32, then muse_glu_bwd's
 * expressions.  The _x3 forms write the operand image like muse_glu_fwd_x3 / _bwd_x3 (h / dab may be NULL: image only).  p = 0 keeps
 * every element (the caller uses the plain entry points).  inter % 4 != 0: MUSE_ERR_UNSUPPORTED (a thread's four columns are one Philox
 * block; the caller then applies muse_dropout to the plain result);  p < 0 or p >= 1: MUSE_ERR_BAD_ARG. */
int muse_glu_drop_fwd(const void* ab, void* h, int32_t dtype, int64_t rows, int32_t inter, float p, uint64_t seed, uint64_t offset,
                      void* stream);
int muse_glu_drop_bwd(const void* ab, const void* dh, void* dab, int32_t dtype, int64_t rows, int32_t inter, float p, uint64_t seed,
                      uint64_t offset, void* stream);
int muse_glu_drop_fwd_x3(const float* ab, float* h, void* planes, int64_t rows, int32_t inter, float p, uint64_t seed, uint64_t offset,
                         int32_t half, float scale, int32_t* stats, void* stream);
int muse_glu_drop_bwd_x3(const float* ab, const float* dh, float* dab, void* planes, int64_t rows, int32_t inter, float p, uint64_t seed,
                         uint64_t offset, int32_t half, float scale, int32_t* stats, void* stream);
/* Fused middle of the NormFormer GLU MLP (muse/modeling_transformer.py:789-797), one pass over ab = [rows, 2*inter]:
 *   fwd: h = gelu_erf(a) * b, hm = LayerNorm(h) * w (mean/rstd saved);
 *   bwd: dh = LN'(dhm) never leaves the CU, dab = (dh*b*gelu'(a), dh*gelu(a)); dw_partial [ceil(rows/R), inter] f32 with
 *        R = muse_ffn_mid_rows_per_block(), reduced by muse_colsum.
 * `h` may be NULL in both: the forward then does not write it and the backward recomputes gelu_erf(a) * b (rounded to the storage
 * type, i.e. exactly the tensor the forward normalised) from ab. */
int muse_ffn_mid_rows_per_block(void);
int muse_ffn_mid_fwd(const void* ab, const float* w, void* h, void* hm, float* mean, float* rstd, int32_t dtype,
                     int32_t rows, int32_t inter, float eps, void* stream);
int muse_ffn_mid_bwd(const void* dhm, const void* h, const void* ab, const float* w, const float* mean, const float* rstd,
                     void* dab, float* dw_partial, int32_t dtype, int32_t rows, int32_t inter, void* stream);
/* y = gelu_erf(x); dx = dy * gelu'(x).  muse/modeling_transformer.py:981. */
int muse_gelu_fwd(const void* x, void* y, int32_t dtype, int64_t n, void* stream);
int muse_gelu_bwd(const void* x, const void* dy, void* dx, int32_t dtype, int64_t n, void* stream);
/* ... from f32 x / dy with the result written as bf16 (the dY operand of the next weight GEMMs in the bf16 compute mode) */
int muse_gelu_bwd_f32_bf16(const float* x, const float* dy, void* dx_bf16, int64_t n, void* stream);

/* Embed.forward (muse/modeling_transformer.py:942-957): out[b,s,:] = word[ids[b,s],:] + pos[s,:], f32 out.
 * bwd: deterministic (sorted by id on device, no float atomics): dword[v,:] (+)= sum over positions with id v,
 * dpos[s,:] (+)= sum_b dout[b,s,:].  `scratch` needs muse_embed_bwd_scratch_floats(hidden, vocab) f32. */
int muse_embed_fwd(const int64_t* ids, const float* word, const float* pos, float* out, int32_t batch, int32_t seq,
                   int32_t hidden, int32_t vocab, void* stream);
int muse_embed_bwd(const int64_t* ids, const float* dout, float* dword, float* dpos, float* scratch, int32_t batch,
                   int32_t seq, int32_t hidden, int32_t vocab, int32_t accumulate, void* stream);
int64_t muse_embed_bwd_scratch_floats(int32_t hidden, int32_t vocab);
/* The same gradients by a stable (token id, position) sort and segmented row sums (csrc/embed.hip): every gradient row is read
 * once, rows with many hits (the mask token) are shared by several blocks, the summation order is fixed.  `scratch`: 256-byte
 * aligned, muse_embed_bwd2_scratch_bytes(batch, seq, hidden, vocab) bytes.  Ids outside [0, vocab) are ignored. */
int muse_embed_bwd2(const int64_t* ids, const float* dout, float* dword, float* dpos, void* scratch, int64_t scratch_bytes,
                    int32_t batch, int32_t seq, int32_t hidden, int32_t vocab, int32_t accumulate, void* stream);
int64_t muse_embed_bwd2_scratch_bytes(int32_t batch, int32_t seq, int32_t hidden, int32_t vocab);

/* F.cross_entropy(logits, labels, ignore_index=-100, label_smoothing) (muse/modeling_transformer.py:1276-1279).
 * fwd: row_loss[r], lse[r] per row, then loss = sum(row_loss over valid) / n_valid into loss_out[0], n_valid into
 * loss_out[1] (f32).  bwd: dlogits = (softmax - target) * gscale / n_valid, 0 for ignored rows. */
int muse_cross_entropy_fwd(const void* logits, int32_t dtype, const int64_t* labels, float* row_loss, float* lse,
                           float* loss_out, int64_t rows, int32_t vocab, int64_t ld, float label_smoothing, void* stream);
int muse_cross_entropy_bwd(const void* logits, int32_t dtype, const int64_t* labels, const float* lse,
                           const float* loss_out, const float* grad_out, void* dlogits, int32_t dl_dtype, int64_t rows,
                           int32_t vocab, int64_t ld, float label_smoothing, void* stream);
/* soft_target_cross_entropy (training/train_maskgit_imagenet.py:101-117) on the class-conditional layout.  logits f32 [rows, ld]
 * with rows = B * seq1 (seq1 = S + 1, position 0 = class token), labels int64 [rows], soft f32 [B * S, K], K <= ld: only the first
 * K columns take part.  Row r = (b, s) is active iff s >= 1 and labels[r] != -100; its soft row is b * S + s - 1.
 * fwd: row_loss / lse / psum per row (0 for inactive rows), row_loss = psum * lse - sum(p * l); then
 * loss_out = (sum(row_loss) / n_active, n_active), one block in a fixed order.
 * bwd: dlogits [rows, ldo] (MUSE_F32 or MUSE_BF16) = grad_out[0] / loss_out[1] * (softmax * psum - p) on the first K columns of
 * active rows, exact 0 on every other element of [0, ldo); no host synchronisation. */
int muse_soft_ce_fwd(const float* logits, const int64_t* labels, const float* soft, float* row_loss, float* lse, float* psum,
                     float* loss_out, int64_t rows, int32_t seq1, int32_t K, int64_t ld, void* stream);
int muse_soft_ce_bwd(const float* logits, const int64_t* labels, const float* soft, const float* lse, const float* psum,
                     const float* loss_out, const float* grad_out, void* dlogits, int32_t dl_dtype, int64_t rows, int32_t seq1,
                     int32_t K, int64_t ld, int64_t ldo, void* stream);

/* AdamW over one flat f32 buffer (torch.optim.AdamW / apex FusedAdam(adam_w_mode) semantics,
 * training/train_maskgit_imagenet.py:242-261,438); optionally refreshes the bf16 compute copy of the weights.  p, g, m, v 16-byte
 * aligned, p_bf16 (when given) 8-byte aligned: MUSE_ERR_ALIGN otherwise, nothing launched.  The arithmetic of one element is pinned,
 * rounding by rounding, at adam_update1 of csrc/optim.hip and is the same in every AdamW entry point. */
int muse_adamw_flat(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* skip, void* stream);
/* Exponential moving average of the weights, every tracked tensor in ONE launch (EMAModel.step, reference muse/modeling_ema.py:118-137,
 * called behind the optimizer step at training/train_muse.py:779-780): shadow = shadow - one_minus_decay * (shadow - param), the three
 * f32 roundings of the reference's tensor expression kept.  `table` (device): 4 x int64 per tensor {shadow, param, n, mode}, mode 0 =
 * update, 1 = copy (requires_grad == False, :134-135); `chunk_first` as for muse_adamw_multi. */
int muse_ema_multi(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, float one_minus_decay,
                   void* stream);
/* The same update for many separate f32 tensors in ONE launch (models whose parameters are ordinary tensors: MaskGiTUViT_v2,
 * muse/modeling_transformer_v2.py; the reference reaches this through apex FusedAdam's multi_tensor_apply).  `table` (device):
 * 6 x int64 per tensor {p, g, m, v, p_bf16 or 0, n}; `chunk_first` (device, num_tensors + 1 x int32): exclusive prefix sum of
 * ceil(n / 4096); num_chunks = chunk_first[num_tensors]. */
int muse_adamw_multi(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* skip,
                     void* stream);
/* AdamW with PARAMETER GROUPS (training/train_muse.py:425-445 builds two: weight decay on the matrices, none on bias / LayerNorm /
 * embedding weights; torch.optim semantics - each group its own lr / betas / eps / weight_decay).  `group_hyper` (HOST memory, read
 * during the call): ngroups <= 8 rows of {lr, beta1, beta2, eps, weight_decay}.
 * _flat_groups: the flat buffer is cut into segments, seg_end[s] (device int64, ascending ABSOLUTE element offsets of the flat
 * buffer) closes segment s and seg_group[s] (device int32) names its group; the call updates elements [base, base + n) - p, g, m, v,
 * p_bf16 point at element `base` - so range-wise updates (inside backward, behind an all-reduce bucket) share one table.
 * _multi_groups: muse_adamw_multi's table with a seventh column, the tensor's group in its low 8 bits; above them (optional, round 6) the
 *   element distance from p_bf16 to a second bf16 plane: p_bf16 then receives hi = bf16(p) and that plane lo = bf16(p - hi), the
 *   bf16x3 operand planes of the updated weight (muse_gemm_x3 reads them next step; 0 = plain bf16 copy).
 * A one-group call is bit-identical to muse_adamw_flat / muse_adamw_multi.
 * skip (every AdamW entry point; the overflow guard of the "f16" mode): NULL = unguarded; else a device int32 (the overflow counter the
 * producer entry points and muse_cast_f32_to_f16 increment) read by the kernel, which leaves parameters and moments untouched when it
 * is non-zero - GradScaler's found_inf without a host round trip. */
int muse_adamw_flat_groups(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                           const int64_t* seg_end, const int32_t* seg_group, int32_t nseg, const float* group_hyper,
                           int32_t ngroups, int32_t step, float grad_scale, const int32_t* skip, void* stream);
int muse_adamw_multi_groups(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                            const float* group_hyper, int32_t ngroups, int32_t step, float grad_scale, const int32_t* skip, void* stream);

/* ---- gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_ with norm_type 2, which the reference reaches through
 * accelerator.clip_grad_norm_: training/train_muse.py:758-759, training/train_maskgit_imagenet.py:435-436) and the per-parameter norms
 * of log_grad_norm (training/train_muse.py:1309-1314), all on the device.
 * Sum of squares: one f64 partial per (parameter, 4096-element chunk counted from the parameter's own start) stored to
 * slab[chunk_first[t] + c] by a plain store - no floating-point atomics, so the slab is the same bits however the gradient is cut
 * into calls and in whatever order they run.  chunk_first (device int32, num + 1 entries): exclusive
 * prefix sum of ceil(n_t / 4096) - muse_adamw_multi's table.
 * _flat: parameters [offset_t, offset_t + n_t) of a flat f32 gradient buffer whose element 0 is g_flat; `ptab` = {offset, n} x int64
 *   per parameter, ascending, once in DEVICE memory (the kernel's) and once in HOST memory with chunk_first (`*_host`, read during the
 *   call).  The call covers the parameters inside [base, base + n); alignment padding between parameters belongs to no norm.  base
 *   must be a parameter's offset and base + n must not cut one: MUSE_ERR_BAD_ARG otherwise.  Offsets need no alignment.
 * _multi: muse_adamw_multi's / _multi_groups' pointer table (`ncol` = 6 or 7 int64 per tensor: gradient pointer in column 1, n in
 *   column 5) - every tensor in one launch. */
int muse_gradnorm_flat(const float* g_flat, int64_t base, int64_t n, const int64_t* ptab_host, const int32_t* chunk_first_host,
                       const int64_t* ptab, const int32_t* chunk_first, int32_t num_params, double* slab, void* stream);
int muse_gradnorm_multi(const int64_t* table, int32_t ncol, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                        double* slab, void* stream);
/* One small launch: the chunks of each parameter folded in chunk order, the parameters in parameter order (f64).  psum: num_tensors
 * + 1 doubles of scratch; the last one is the launch's ticket counter and must be ZERO before the first call (every call leaves it zero).  out (device f32, 3 + num_tensors): [0] norm = grad_scale * sqrt(total), rounded once to f32 - grad_scale is
 * the host factor the AdamW entry points multiply the gradient by (1 / world under a SUM reduction), so this is the norm of the
 * gradient the update uses; [1] coef = min(1, max_norm / (norm + 1e-6)) in f32 (clip_grad_norm_'s formula; a NaN norm gives a NaN
 * coefficient, like torch.clamp); [2] scale = grad_scale * coef; [3 + t] = grad_scale * sqrt(sum of parameter t). */
int muse_gradnorm_finalize(const double* slab, const int32_t* chunk_first, int32_t num_tensors, double* psum, float grad_scale,
                           float max_norm, float* out, void* stream);
/* g *= *scale in place (clip_grad_norm_'s `g.mul_(clip_coef_clamped)`, applied also when the coefficient is 1, as torch does):
 * n elements of a flat buffer / every gradient of a pointer table as for muse_gradnorm_multi. */
int muse_grad_scale_flat(float* g, int64_t n, const float* scale, void* stream);
int muse_grad_scale_multi(const int64_t* table, int32_t ncol, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                          const float* scale, void* stream);
/* The four AdamW entry points with the gradient factor read ON THE DEVICE (`scale_dev`: out + 2 of muse_gradnorm_finalize) in place
 * of the host's grad_scale: clipping (training/train_muse.py:758-759 followed by optimizer.step(), :761) without a host round trip or
 * a write pass over the gradient.  Same update arithmetic, same skip guard.  The product g * *scale_dev is rounded once to f32 before
 * the update (the host-factor entry points feed the unrounded product into `g - m` through an fma, invisible for their power-of-two
 * factors), so the result is bit-identical to muse_grad_scale_* followed by the host-factor entry point with grad_scale 1. */
int muse_adamw_flat_dev(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int32_t step, const float* scale_dev, const int32_t* skip, void* stream);
int muse_adamw_multi_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* scale_dev,
                         const int32_t* skip, void* stream);
int muse_adamw_flat_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                               const int64_t* seg_end, const int32_t* seg_group, int32_t nseg, const float* group_hyper,
                               int32_t ngroups, int32_t step, const float* scale_dev, const int32_t* skip, void* stream);
int muse_adamw_multi_groups_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                const float* group_hyper, int32_t ngroups, int32_t step, const float* scale_dev, const int32_t* skip,
                                void* stream);
/* Lion (the reference's `lion` optimizer choice, training/optimizer.py:57-79) in AdamW's eight forms: the same kernels instantiated with
 * another update rule, so tables (6 / 7 columns; column 3, AdamW's v, is ignored and may be 0), chunk_first, segments, images, `skip`,
 * `scale_dev` and the error codes are exactly those of the muse_adamw_* entry point of the same name.  There is no eps, no step count and
 * no second moment: the state is m alone (20 B of traffic per parameter against AdamW's 28).
 * Hyper-parameters are DOUBLE and travel as HOST rows of {lr, beta1, beta2, weight_decay}, read during the call (`hyper`: one row;
 * `group_hyper`: ngroups <= 8 rows; NULL: MUSE_ERR_BAD_ARG): each constant is computed in double from the Python floats and rounded
 * ONCE to f32 -
 *   decay = f32(1 - lr * wd)   b1 = f32(beta1)   omb1 = f32(1 - beta1)   b2 = f32(beta2)   omb2 = f32(1 - beta2)   nlr = f32(-lr)
 * - and the update of one element is pinned at lion_update1 of csrc/optim.hip (contraction off, every operator rounds to f32, fma is
 * one rounding, f32 denormals kept; s = grad_scale or *scale_dev):
 *   gr = round(g * s)                       s == 1 leaves g's bits
 *   p1 = round(p * decay)                   p.data.mul_(1 - lr * wd): the decayed parameter is rounded on its own
 *   u  = round(round(m * b1) + round(gr * omb1))
 *   p' = round(p1 + nlr * sign(u))          sign: +1, -1, 0 for u == +-0 (p' then has p1's bits, also for p1 == -0.0), NaN for NaN
 *   m' = fma(omb2, gr, round(m * b2))       exp_avg.mul_(beta2).add_(grad, alpha=1 - beta2)
 * u uses the OLD m; m' does not reuse round(m * b1).  On the CPU this is the reference class bit for bit (tests/golden/lion_steps.npz).
 * A one-group grouped call is bit-identical to the single-set call.  A *_dev call is bit-identical to muse_grad_scale_* followed by the
 * host-factor call with grad_scale 1. */
int muse_lion_flat(float* p, const float* g, float* m, void* p_bf16, int64_t n, const double* hyper, float grad_scale,
                   const int32_t* skip, void* stream);
int muse_lion_flat_dev(float* p, const float* g, float* m, void* p_bf16, int64_t n, const double* hyper, const float* scale_dev,
                       const int32_t* skip, void* stream);
int muse_lion_flat_groups(float* p, const float* g, float* m, void* p_bf16, int64_t n, int64_t base, const int64_t* seg_end,
                          const int32_t* seg_group, int32_t nseg, const double* group_hyper, int32_t ngroups, float grad_scale,
                          const int32_t* skip, void* stream);
int muse_lion_flat_groups_dev(float* p, const float* g, float* m, void* p_bf16, int64_t n, int64_t base, const int64_t* seg_end,
                              const int32_t* seg_group, int32_t nseg, const double* group_hyper, int32_t ngroups,
                              const float* scale_dev, const int32_t* skip, void* stream);
int muse_lion_multi(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, const double* hyper,
                    float grad_scale, const int32_t* skip, void* stream);
int muse_lion_multi_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, const double* hyper,
                        const float* scale_dev, const int32_t* skip, void* stream);
int muse_lion_multi_groups(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                           const double* group_hyper, int32_t ngroups, float grad_scale, const int32_t* skip, void* stream);
int muse_lion_multi_groups_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                               const double* group_hyper, int32_t ngroups, const float* scale_dev, const int32_t* skip, void* stream);
/* out[i] (+)= sum over s < nslices of ws[s*stride + i]: reduction of split-K partial results (n, stride % 4 == 0) */
int muse_sum_slices(const float* ws, float* out, int32_t nslices, int64_t n, int64_t stride, int32_t accumulate, void* stream);
/* njobs <= 16 reductions in ONE launch, each bit-identical to the single-job kernel it stands for: kind 0 = muse_sum_slices
 * (ws[i] -> out[i], nslices[i] slices of n[i] elements stride[i] apart), kind 1 = muse_colsum (out[i][c] (+)= sum over the
 * nslices[i] rows of the [nslices[i], n[i]] f32 matrix ws[i]).  All arrays are HOST arrays read during the call. */
int muse_sum_multi(const void* const* ws, void* const* out, const int32_t* nslices, const int64_t* n, const int64_t* stride,
                   const int32_t* accumulate, const int32_t* kind, int32_t njobs, void* stream);
/* hi = bf16(in), lo = bf16(in - hi): the operand planes of a bf16x3 product (in ~= hi + lo to 2^-16 relative) */
int muse_split_f32_to_bf16x2(const float* in, void* hi, void* lo, int64_t n, void* stream);
/* out[r, c] = sum over nslices of ws[s * stride + r * cols + c] (+ bias[c]) (+ residual[r, c]) written as out_dtype (f32 / bf16; the
 * residual has the output's dtype, like muse_gemm's): reduction of a forward product's K-slice workspace fused with the Linear's
 * epilogue - the small-batch decoding path (ops.gemm: products of <= 2048 rows whose tiles would fill a fraction of the chip). */
int muse_sum_slices_epilogue(const float* ws, int32_t nslices, int64_t stride, const float* bias, const void* residual, int64_t ldr,
                             void* out, int32_t out_dtype, int64_t ldc, int64_t rows, int32_t cols, void* stream);
/* The same split written as ONE GEMM operand of three times the K length: the bf16x3 product hi*hi + hi*lo + lo*hi is a single product
 * of A' = (hi | hi | lo) and B' = (hi | lo | hi) along K.  in [rows, cols] f32 (row stride ld_in); mode 0: planes concatenated along the
 * columns, out [rows, 3 cols] (k-contiguous operand), mode 1: stacked along the rows, out [3 rows, cols] (k-major operand), both with row
 * stride ld_out; lo_pos = 1 | 2: the third that carries the lo plane.  cols % 4 == 0. */
int muse_split_f32_to_bf16_cat3(const float* in, void* out, int64_t rows, int32_t cols, int64_t ld_in, int64_t ld_out, int32_t mode,
                                int32_t lo_pos, void* stream);
int muse_cast_f32_to_bf16(const float* in, void* out, int64_t n, void* stream);
/* out = half(in * scale): the operand image of a MUSE_F16 product (round to nearest even, subnormals kept; a finite value beyond half's
 * range becomes inf - the product turns NaN rather than silently wrong).  stats: NULL or int32[2], incremented by [0] the number of
 * ELEMENTS whose half is inf or NaN (an inf / NaN input and an f32-overflowing in * scale included), [1] the number of finite non-zero
 * inputs whose half is +-0. */
int muse_cast_f32_to_f16(const float* in, void* out, int64_t n, float scale, int32_t* stats, void* stream);
/* (half, scale, stats): the last three arguments before `stream` of the producer entry points that write operand images next to (or
 * instead of) their f32 result - muse_glu_fwd_x3 / _bwd_x3, muse_norm_adaln_fwd_x3 / _bwd_x3, muse_attention_x3_fwd / _bwd / _fwd_stream /
 * _bwd_stream / _merge - say what that image is.  half = 0: the (hi, lo) bf16 planes of the "bf16x3" mode, as documented with each.
 * half = 1 ("f16" mode): ONE IEEE-half image [rows][cols] at the plane pointer = half(result * scale), the bits muse_cast_f32_to_f16 makes
 * of the f32 result; the caller passes scale = 1 for forward results and the pass's gradient scale for the gradients the backward entry
 * points produce (a power of two either way, else MUSE_ERR_BAD_ARG); lo-plane distances are ignored; the muse_attention_x3_* entry points
 * also COMPUTE in that format, planes or not (one half plane per operand, one half MFMA per K step; dO and dS times scale, results divided
 * by it); stats (device int32[2], NULL unless half): [0] is incremented per 4-element group that holds an inf / NaN half
 * (muse_cast_f32_to_f16's overflow counter: a dynamic gradient scale backs off on it). */
int muse_cast_bf16_to_f32(const void* in, float* out, int64_t n, void* stream);

/* prepare_inputs_and_labels (training/train_maskgit_imagenet.py:371-394) given the two uniform draws.
 * tokens [B,S] i64, class_ids [B] i64, timesteps [B] f32, noise [B,S] f32 ->
 * input_ids, labels [B,S+1] i64, mask_prob [B] f32.  S <= 1024. */
int muse_mask_sample(const int64_t* tokens, const int64_t* class_ids, const float* timesteps, const float* noise,
                     int64_t* input_ids, int64_t* labels, float* mask_prob, int32_t batch, int32_t seq, int64_t mask_id,
                     int64_t codebook_size, float min_masking_rate, void* stream);

/* One iteration of MaskGit parallel decoding on the device (muse/modeling_transformer.py:1409-1454, :generate2;
 * muse/modeling_transformer_v2.py:434-474; muse/sampling.py:30-35 mask_by_random_topk): replaces ~10 ATen launches per step
 * (softmax, multinomial, where, gather, log, sort, gather, compare, where).
 *   the logits of image b, position s start at logits + b*img_stride + s*ld (f32; lets the caller skip a class-token row);
 *   logits = uncond + guidance_scale * (cond - uncond) over the first `vocab` columns (uncond_logits NULL: logits = cond);
 *   p = softmax(logits);  sampled = argmax_j p_j / q_j, q ~ Exp(1) (how torch.multinomial(num_samples = 1) draws), known
 *   tokens (input_ids != mask_id) are kept;  confidence = log(clamp(p_sampled, 1e-20)) + temperature * gumbel(u) (FLT_MAX as p
 *   for known tokens);  mask_len = max(1, min(#unknown - 1, sched_mask_len));  next_ids = mask_id where confidence < the
 *   mask_len-th smallest confidence of the image (0-based), else the sampled id.
 * noise_exp [batch*seq, vocab] / noise_u [batch, seq]: the caller's random draws (parity tests replay the reference's CPU
 * generator) and are used verbatim; NULL: Philox4x32-10 with counter (row, row >> 32, j, 2 * step) for token j of row = b * seq + s
 * (2 * step + 1 and j = 0 for the row's Gumbel draw) and key (seed, seed >> 32); the first output word r gives
 * u = ((r >> 8) + 1) * 2^-24 in (0, 1] and q = -log(u), except that u == 1 (2^-24 of the draws) gives q = 2^-25 instead of 0: q stays
 * strictly positive, as torch's exponential_ is, so that no token wins or loses a row by p / 0 whatever its probability.  raw_sampled (may be
 * NULL) receives the samples before known tokens are restored (the reference's `intermediate` list).  conf_scratch: f32 [batch*seq].
 * 2 <= seq <= 4096. */
int muse_sample_step(const float* cond_logits, const float* uncond_logits, float guidance_scale, int64_t img_stride, int64_t ld,
                     int32_t vocab,
                     const int64_t* input_ids, int64_t mask_id, const float* noise_exp, const float* noise_u, uint64_t seed,
                     uint32_t step, float temperature, int32_t sched_mask_len, int32_t batch, int32_t seq, int64_t* raw_sampled,
                     int64_t* sampled, int64_t* next_ids, float* conf_scratch, void* stream);

/* muse_sample_step sampling from a truncated distribution: top-k and / or nucleus (top-p) filtering inside the same launch pair.
 * l_j is the logit of code j < vocab after the guidance mix uncond + scale * (cond - uncond), rounded exactly as muse_sample_step
 * rounds it (the same instructions: f32 difference, then the multiply-add).
 *   top_k (integer, 1 <= top_k): keep j iff l_j >= v_k, v_k the k-th largest value of the row; all ties at v_k are kept;
 *     top_k >= vocab means off.
 *   top_p (float, 0 < top_p <= 1): with p_j = softmax(l)_j over the codes that survive top_k, keep j iff the mass strictly above it,
 *     M_gt(j) = sum over {i : l_i > l_j} of p_i, is < top_p; a group of tied logits is kept or dropped as a whole; the largest logit
 *     is always kept; top_p == 1 means off.
 *   Both given: top_k first, then the nucleus over the distribution renormalised on the top-k set.
 *   Filtered codes behave exactly as if their logit were -inf before muse_sample_step: probability exactly 0 in the categorical race
 *     (index-first tie-breaking unchanged), the confidence of a sampled code uses the renormalised probability, and everything after
 *     the draw is unchanged (known tokens kept, FLT_MAX confidence for them, mask_len, the k-th-smallest threshold, re-mask).
 *   Both filters reduce to one per-row cutoff tau, the kept set being {j : l_j >= tau}; cutoff (f32 [batch*seq], may be NULL) receives
 *     tau, -inf for a row with both filters off.
 * The nucleus mass is summed in 64-bit fixed point (exp(l_j - max) * 2^40, truncated), so the result is the same bits run to run.
 * The Philox stream is muse_sample_step's: a draw belongs to (row, code, step) whether the code is kept or not, and with both
 * filters off the results are muse_sample_step's bit for bit.  2 <= seq <= 4096 and vocab <= 16384 (else MUSE_ERR_UNSUPPORTED);
 * top_k < 1, or top_p outside (0, 1] or NaN: MUSE_ERR_BAD_ARG. */
int muse_sample_step_filtered(const float* cond_logits, const float* uncond_logits, float guidance_scale, int64_t img_stride, int64_t ld,
                              int32_t vocab, const int64_t* input_ids, int64_t mask_id, const float* noise_exp, const float* noise_u,
                              uint64_t seed, uint32_t step, float temperature, int32_t sched_mask_len, int32_t batch, int32_t seq,
                              int64_t* raw_sampled, int64_t* sampled, int64_t* next_ids, float* conf_scratch, int32_t top_k, float top_p,
                              float* cutoff, void* stream);

/* training/train_muse.py:149-226 mask_or_random_replace_tokens on the device.  mask_prob = cos(pi/2 t) clipped to
 * min_masking_rate (timesteps given) or mask_prob_in as is (the eval_mask_ratios branch); k = round(seq * mask_prob) >= 1;
 * mask = argsort(noise) < k (noise given) or the rectangle rects[b] = (y0, x0, h, w) on the sqrt(seq) grid (contiguous-region
 * branch, drawn on the host like the reference does); input_ids = mask_id where masked (the reference's `noise_type` test at
 * :202 is always true, so "random_replace" also masks: kept); labels = tokens where masked else -100, or all tokens when
 * all_labels (predict_all_tokens / random_replace), with loss_weight = 1 - (1 - mask) * (1 - mask_prob) * (1 - weight_min)
 * (:145-146; loss_weight may be NULL). */
int muse_mask_tokens(const int64_t* tokens, const float* timesteps, const float* mask_prob_in, const float* noise,
                     const int32_t* rects, int64_t* input_ids, int64_t* labels, float* loss_weight, float* mask_prob,
                     int32_t batch, int32_t seq, int64_t mask_id, float min_masking_rate, int32_t all_labels, float weight_min,
                     void* stream);

/* nn.Dropout (muse/modeling_transformer.py:237 attention probabilities, :797 feed-forward, :956 embeddings): y = x * keep / (1 - p),
 * keep_i = [Philox(seed, offset + i / 4) lane (i % 4) >= p]; in place capable.  There is no mask tensor: the backward pass applies
 * the same call (same seed / offset) to the gradient. */
int muse_dropout(const void* x, void* y, int32_t dtype, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream);

/* training/train_muse.py:715-731 conditioning dropout: keep_b = uniforms[b] < prob;  out = (x * keep != 0) ? x : empty
 * (x [batch, per_image] f32, empty [per_image] f32) - the reference's expression verbatim. */
int muse_cond_dropout(const float* x, const float* empty, const float* uniforms, float* out, int32_t batch, int64_t per_image,
                      float prob, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * MaskGitVQGAN kernels (NHWC activations).
 * muse_conv2d_nhwc: stride-1 SAME convolution (Conv2dSame, muse/modeling_maskgit_vqgan.py:33-45) as implicit GEMM
 *   on MFMA; weight pre-permuted to [Cout][KS][KS][Cin]; optional bias (f32 [Cout]), optional residual add
 *   (ResnetBlock :85), optional nearest x2 upsample of the input folded into the gather (UpsamplingBlock :146-147).
 *   H, W are the OUTPUT spatial dims.  Cin must be a multiple of 16/elsize.
 *   upsample: 0 = stride 1;  1 = input is [H/2, W/2], nearest x2 upsampled on the fly;  2 = input is [2H, 2W], stride-2
 *   3x3 convolution over it zero-padded by one row / column at the bottom / right (taming-VQGAN Downsample,
 *   muse/modeling_taming_vqgan.py:53-59: F.pad(0,1,0,1) + Conv2d(3, stride 2, padding 0)).  Same meaning in
 *   muse_conv2d_nhwc_split.
 *   Span limit (both entries; the loaders address with 32-bit byte offsets): the input tensor - [batch, H, W, Cin] for upsample 0,
 *   [batch, H/2, W/2, Cin] for 1, [batch, 2H, 2W, Cin] for 2 - and the weight image [Cout][KS][KS][Cin] must each stay below
 *   4 GiB - 64 bytes, and batch * H * W below 2^31 - 256; anything larger returns MUSE_ERR_UNSUPPORTED before a launch (split the batch).
 */
int muse_conv2d_nhwc(const void* in, const void* weight, const float* bias, const void* residual, void* out,
                     int32_t dtype, int32_t batch, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS,
                     int32_t upsample, void* stream);
/* f32-class convolution on the bf16 matrix cores by hi/lo operand splitting (3 bf16 MFMAs per product, f32 accumulate,
 * error <= 2^-16 |a||b| per product: tighter than the TF32 the reference's cuDNN path uses by PyTorch default).
 * in / out / residual f32 NHWC, w_hi / w_lo bf16 [Cout][KS][KS][Cin] with w ~= w_hi + w_lo; Cin % 8 == 0. */
int muse_conv2d_nhwc_split(const float* in, const void* w_hi, const void* w_lo, const float* bias, const float* residual,
                           float* out, double* gn_partial, int32_t gn_groups, int32_t batch, int32_t H, int32_t W,
                           int32_t Cin, int32_t Cout, int32_t KS, int32_t upsample, void* stream);
/*   gn_partial != NULL (conv_in :168, the 1x1 nin_shortcut :82-85): GroupNorm(gn_groups) sum / sum-of-squares of the output
 *   per (image, 128-pixel tile, group), [B, H*W/128, gn_groups, 2] f64, as for muse_conv2d_nhwc_split2 below.  Needs
 *   H*W % 128 == 0 and Cout/gn_groups a power of two in [4, 32]. */
/* The same convolution for the 3x3 layers whose input comes out of GroupNorm+SiLU (conv1 / conv2 of every ResnetBlock
 * :73-80, conv_out :189): the activation arrives pre-split as two bf16 NHWC planes (muse_groupnorm_silu_nhwc_split) and all
 * operands go global -> LDS by DMA (csrc/conv_dma.hip).  Results are bit-identical to muse_conv2d_nhwc_split on the f32
 * tensor hi + lo came from.  KS == 3, Cin % 32 == 0, Cout % 4 == 0, each plane < 4 GiB. */
int muse_conv2d_nhwc_split2(const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* bias,
                            const float* residual, float* out, double* gn_partial, int32_t gn_groups, int32_t batch,
                            int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, void* stream);
/*   gn_partial != NULL: the epilogue also writes the GroupNorm(gn_groups) sum / sum-of-squares of its output (bias and
 *   residual included) per (image, 256-pixel tile, group) as [B, H*W/256, gn_groups, 2] f64 - the statistics pass of the
 *   GroupNorm that consumes this tensor (muse_groupnorm_silu_nhwc_split with stats_nchunk = H*W/256) then never reads it.
 *   Needs H*W % 256 == 0 and Cout/gn_groups a power of two in [4, 128]. */
/* GroupNorm(32, eps, affine) + SiLU (muse/modeling_maskgit_vqgan.py:61,73-78,186-187,236-237).
 * stats: partial [B, nchunk, G, 2] f64 -> apply.  `partial` needs B*nchunk*G*2 doubles (nchunk from _nchunk). */
int muse_groupnorm_silu_nhwc(const void* x, void* y, int32_t dtype, const float* gamma, const float* beta,
                             double* partial, int32_t batch, int32_t HW, int32_t C, int32_t groups, float eps,
                             int32_t apply_silu, void* stream);
int muse_groupnorm_nchunk(int32_t HW);
/* GroupNorm(groups) + SiLU of the INPUT fused into the 3x3 bf16x3 convolution (muse/modeling_maskgit_vqgan.py:73-80 norm1 -> swish
 * -> conv1, norm2 -> swish -> conv2; :186-189 norm_out -> swish -> conv_out): `x` is the f32 NHWC activation, gn_scale / gn_shift
 * [batch][Cin] f32 the affine form of its normalisation (muse_groupnorm_scale_shift: rstd * gamma, beta - rstd * gamma * mean from
 * the [B, nchunk, groups, 2] f64 partial sums a producer's epilogue left).  The kernel normalises, activates and splits the
 * activation into the hi / lo bf16 operands while it stages them in LDS: bit-identical to muse_groupnorm_silu_nhwc_split followed
 * by muse_conv2d_nhwc_split2, without the write and re-read of the two planes.  Shapes: muse_conv2d_nhwc_gn_split2_ok (3x3, H and W
 * multiples of 16, Cin a multiple of 64); others return MUSE_ERR_UNSUPPORTED.  bias / residual / gn_partial as for _split2. */
int muse_conv2d_nhwc_gn_split2_ok(int32_t batch, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS);
/* persistent = 1: the persistent form may run (one workgroup per CU walks the tiles; bit-identical; 6-8 % faster when the convolution
 * has the chip to itself, slower for a step that shares the chip with it); 0: the launch-per-tile kernel (round 6). */
int muse_conv2d_nhwc_gn_split2(const float* x, const float* gn_scale, const float* gn_shift, const void* w_hi, const void* w_lo,
                               const float* bias, const float* residual, float* out, double* gn_partial, int32_t gn_groups,
                               int32_t batch, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t persistent,
                               void* stream);
/* muse_conv2d_nhwc_gn_split2 + F.avg_pool2d(2, 2) of its output in one kernel (the 2 x 2 average is taken in the convolution's epilogue:
 * a quarter of the stores, no pooling pass).  out [batch, H/2, W/2, Cout] f32, the same bits as muse_avgpool2x2_nhwc_stats of the
 * un-pooled output; residual stays [batch, H, W, Cout]; gn_partial (optional): [batch, H * W / 256, gn_groups, 2] f64 sums of the POOLED
 * values, one chunk per convolution tile - muse_groupnorm_scale_shift with nchunk = H * W / 256, HW = (H / 2) * (W / 2). */
int muse_conv2d_nhwc_gn_split2_pool(const float* x, const float* gn_scale, const float* gn_shift, const void* w_hi, const void* w_lo,
                                    const float* bias, const float* residual, float* out, double* gn_partial, int32_t gn_groups,
                                    int32_t batch, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t persistent,
                                    void* stream);
int muse_groupnorm_scale_shift(const double* partial, int32_t nchunk, const float* gamma, const float* beta, float* scale,
                               float* shift, int32_t batch, int32_t HW, int32_t C, int32_t groups, float eps, void* stream);
/* Encoder.conv_in (muse/modeling_maskgit_vqgan.py:175; taming :380): 3x3, padding 1, Cin <= 4 image channels -> Cout, as a direct
 * exact-f32 convolution (K = 9 * Cin is no matrix-core problem; the output write is what costs).  x [B, H, W, Cpad] f32 NHWC (Cpad a
 * multiple of 4, channels >= 4 ignored), w4 [Cout][9][4] f32 (tap-major, input channels zero-padded to 4), bias f32 [Cout] or NULL.
 * gn_partial (optional, needs gn_groups * 4 == Cout): [B, H, gn_groups, 2] f64 sum / sum of squares of the output per image row -
 * the `partial` / nchunk = H a following GroupNorm consumes.  Cout % 4 == 0, Cout / 4 divides 256. */
int muse_conv_in_direct(const float* x, const float* w4, const float* bias, float* out, double* gn_partial, int32_t gn_groups,
                        int32_t batch, int32_t H, int32_t W, int32_t Cin, int32_t Cpad, int32_t Cout, void* stream);
/* The same convolution reading the image as it arrives: x [batch, Cin, H, W] f32 contiguous (NCHW), no channel-padded NHWC copy.
 * Output and gn_partial are the same bits as muse_nchw_to_nhwc + muse_conv_in_direct. */
int muse_conv_in_direct_nchw(const float* x, const float* w4, const float* bias, float* out, double* gn_partial, int32_t gn_groups,
                             int32_t batch, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stream);
/* Decoder.conv_out behind norm_out + swish (muse/modeling_maskgit_vqgan.py:236-240; hidden_channels -> 3 image channels) as ONE
 * direct exact-f32 convolution: x [B, H, W, C] f32 is normalised with the per-image affine form of the GroupNorm (scale / shift
 * [B, C] f32 from muse_groupnorm_scale_shift), activated (SiLU) and convolved 3x3 / padding 1 (zero padding after the activation)
 * with w [Cout][9][C] f32 (+ bias [Cout]) -> out [B, H, W, Cout] f32.  H, W % 16 == 0, C % 32 == 0, Cout <= 4. */
int muse_conv_out_direct(const float* x, const float* scale, const float* shift, const float* w, const float* bias, float* out,
                         int32_t batch, int32_t H, int32_t W, int32_t C, int32_t Cout, void* stream);
/* F.interpolate(scale_factor=2, mode="nearest") of an NHWC tensor (f32, C % 4 == 0; bf16, C % 8 == 0): the taming Upsample without
 * its convolution (muse/modeling_taming_vqgan.py:36-47, resample_with_conv = False) -> y [B, 2H, 2W, C] */
int muse_upsample2x_nhwc(const void* x, void* y, int32_t dtype, int32_t batch, int32_t H, int32_t W, int32_t C, void* stream);
/* F.interpolate(scale_factor=2, "nearest") of x [B, H, W, C] f32 written as the (hi, lo) bf16 operand planes [B, 2H, 2W, C] of
 * muse_conv2d_nhwc_split2 (UpsamplingBlock, :141-149): hi = bf16(x), lo = bf16(x - hi).  C % 8 == 0. */
int muse_upsample2x_split_nhwc(const float* x, void* y_hi, void* y_lo, int32_t batch, int32_t H, int32_t W, int32_t C, void* stream);
/* f32 in; output as y_hi = bf16(y), y_lo = bf16(y - y_hi) (two [B, HW, C] bf16 planes) for muse_conv2d_nhwc_split2.
 * stats_nchunk == 0: statistics computed here into `partial`; > 0: `partial` = [B, stats_nchunk, G, 2] already filled. */
int muse_groupnorm_silu_nhwc_split(const float* x, void* y_hi, void* y_lo, const float* gamma, const float* beta,
                                   double* partial, int32_t stats_nchunk, int32_t batch, int32_t HW, int32_t C,
                                   int32_t groups, float eps, int32_t apply_silu, void* stream);
int muse_avgpool2x2_nhwc(const void* x, void* y, int32_t dtype, int32_t batch, int32_t H, int32_t W, int32_t C,
                         void* stream); /* F.avg_pool2d(2,2), :112; H,W = input dims */
/* f32 avg_pool2d(2,2) that also leaves the GroupNorm(groups) statistics of its OUTPUT in `partial`
 * ([B, muse_groupnorm_nchunk(H/2*W/2), groups, 2] f64): the first norm of the next encoder level (:73) skips its own pass. */
int muse_avgpool2x2_nhwc_stats(const float* x, float* y, double* partial, int32_t groups, int32_t batch, int32_t H, int32_t W,
                               int32_t C, void* stream);
/* layout / dtype conversion: NCHW f32 <-> NHWC (f32|bf16), channel padding with zeros up to Cpad */
int muse_nchw_to_nhwc(const float* in, void* out, int32_t out_dtype, int32_t batch, int32_t C, int32_t HW, int32_t Cpad,
                      void* stream);
int muse_nhwc_to_nchw(const void* in, int32_t in_dtype, float* out, int32_t batch, int32_t C, int32_t HW, int32_t Cpad,
                      void* stream);
/* argmin over codes of dist [rows, ncodes] f32, :279/:346.  idx[r] is always in [0, ncodes): the lowest index of the smallest non-NaN
 * value (-0.0 == +0.0; a row of +inf gives 0 like torch.argmin); a NaN never wins - a row of nothing but NaN gives 0, where torch.argmin
 * returns the first NaN's index.  ncodes <= 0: MUSE_ERR_BAD_ARG. */
int muse_argmin_rows(const float* dist, int64_t* idx, int64_t rows, int32_t ncodes, int64_t ld, void* stream);
/* sum of squares per row, f32 in / f32 out (VectorQuantizer.compute_distances :308-309) */
int muse_row_sumsq(const float* x, float* out, int64_t rows, int32_t cols, int64_t ld, void* stream);
/* codebook gather (get_codebook_entry :318-324): out[r, :] = codebook[idx[r], :] (f32 -> out_dtype) */
int muse_gather_rows(const float* table, const int64_t* idx, void* out, int32_t out_dtype, int64_t rows, int32_t cols,
                     void* stream);

/* Probe used by the test-suite to pin the ds_read_b64_tr_b16 lane mapping this library relies on:
 * out[lane*4 + j] for a 64-lane wave reading lds[i] = i (uint16) with per-lane byte address addr[lane]. */
int muse_probe_tr16(const int32_t* addr, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MaskGiTUViT_v2 (muse/modeling_transformer_v2.py) - the kernels that model needs beyond the
 * MaskGit ones.  f32.  (csrc/uvit.hip)
 * muse_norm_res_fwd: v = x (+ res); pre = v (optional); y = RMSNorm(v) * w (mode 0, unfused_rms_norm :673-691) or
 *   LayerNorm(v) * w (mode 1, unfused_layer_norm :726-737); w may be NULL.  cols % 4 == 0.
 * muse_adaln_fwd: AdaLNModulation :1025-1037, y[b,r,:] = x[b,r,:] * (1 + ss[b,:C]) + ss[b,C:], ss = mapper(silu(cond)).
 * muse_dwconv3x3_nhwc: ResBlock.depthwise :596-603 (groups = C, padding 1), weight [C][3][3].
 * muse_grn_fwd: GlobalResponseNorm :741-751 on [B, S, C]; scratch 2*B*C floats, returns [G | N] for the backward.
 * muse_sinusoidal_encode: sinusoidal_encode :59-76, out [n, dim].
 * muse_weighted_mean: out[0] = sum(v*w) / sum(w)  (per-token loss weighting :311-316). */
int muse_norm_res_fwd(const float* x, const float* res, const float* w, float* y, float* pre, int64_t rows, int32_t cols,
                      float eps, int32_t mode, void* stream);
int muse_adaln_fwd(const float* x, const float* ss, float* y, int32_t batch, int64_t rows_per_batch, int32_t C, void* stream);
/* ... with the f32 result and / or its bf16 copy (the next GEMM's operand in the bf16 compute mode); either pointer may be null */
int muse_adaln_fwd_ex(const float* x, const float* ss, float* y, void* y_bf16, int32_t batch, int64_t rows_per_batch, int32_t C,
                      void* stream);
int muse_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int muse_dwconv3x3_nhwc(const float* x, const float* w, float* y, int32_t batch, int32_t H, int32_t W, int32_t C, void* stream);
/* 2x2 space-to-depth (inverse = 0: x full [B, H, W, C] -> y packed [B, H/2, W/2, 4C], channel order (di, dj, c)) and its inverse
 * (inverse = 1: x packed -> y full); H, W are the FULL-resolution sides in both directions (even), C % 4 == 0.  With it the stride-2
 * 2x2 convolution of DownsampleBlock (reference muse/modeling_transformer_v2.py:510-514) and the stride-2 2x2 transposed convolution
 * of UpsampleBlock (:558-562) are single products on muse_gemm; each direction is the other's backward. */
int muse_space_to_depth2_nhwc(const float* x, float* y, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t inverse, void* stream);
int muse_grn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* scratch, int32_t batch, int64_t S,
                 int32_t C, void* stream);
/* ... with the f32 result and / or its bf16 copy (the next GEMM's operand in the bf16 compute mode); either pointer may be null */
int muse_grn_fwd_ex(const float* x, const float* gamma, const float* beta, float* y, void* y_bf16, float* scratch, int32_t batch,
                    int64_t S, int32_t C, void* stream);
/* muse_grn_fwd_ex followed by nn.Dropout (ResBlock.channelwise[3], reference :607) in the same pass: the statistics see the undropped
 * input, the result is multiplied by muse_dropout(seed, offset)'s keep bit of flat element (b * S + s) * C + c, scale 1 / (1 - p).
 * muse_grn_drop_bwd: muse_grn_bwd with that mask, redrawn, applied to dy before everything else (the dgamma / dbeta sums included).
 * C % 4 != 0 (or a shape the four-channel kernels do not index): MUSE_ERR_UNSUPPORTED, nothing launched - the caller runs the plain
 * entry point and muse_dropout.  Pointers 16-byte aligned (y_bf16: 8), else MUSE_ERR_ALIGN. */
int muse_grn_drop_fwd_ex(const float* x, const float* gamma, const float* beta, float* y, void* y_bf16, float* scratch, int32_t batch,
                         int64_t S, int32_t C, float p, uint64_t seed, uint64_t offset, void* stream);
int muse_grn_drop_bwd(const float* dy, const float* x, const float* gamma, const float* stats, float* dx, float* work, int32_t batch,
                      int64_t S, int32_t C, float p, uint64_t seed, uint64_t offset, void* stream);
int muse_sinusoidal_encode(const float* f, float* out, int64_t n, int32_t dim, float max_positions, void* stream);
int muse_weighted_mean(const float* v, const float* w, float* out, int64_t n, void* stream);
/* backward of the above (f32).  v = the forward's pre-norm sum x (+ res); dv = dx = dres; dw_partial [nblk, cols] is folded
 * with muse_colsum (nblk from _nblk; cols <= 4096).  muse_adaln_bwd: dx and dss [B, 2C] = (sum_r dy x | sum_r dy).
 * muse_dwconv3x3_bwd: dx and dw_partial [nchunk, C*9] (muse_colsum -> dw [C][3][3]; nchunk > 65535, the library's own limit for gridDim.y whatever the runtime accepts: MUSE_ERR_UNSUPPORTED before a launch).  muse_grn_bwd: `stats` = the forward's
 * scratch [G | N]; work 4*B*C floats, on return work[0:B*C] = per-image dbeta terms, work[B*C:2*B*C] = per-image dgamma terms
 * (muse_colsum over the B rows).  muse_scale_rows: x[r, :cols] *= w[r] * num[0] / den[0] (weighted-loss gradient). */
int muse_norm_res_bwd_nblk(int64_t rows);
int muse_norm_res_bwd(const float* dy, const float* dpre, const float* v, const float* w, float* dv, float* dw_partial,
                      int64_t rows, int32_t cols, float eps, int32_t mode, void* stream);
/* ... also writing a bf16 copy of dv (may be null) */
int muse_norm_res_bwd_ex(const float* dy, const float* dpre, const float* v, const float* w, float* dv, void* dv_bf16,
                         float* dw_partial, int64_t rows, int32_t cols, float eps, int32_t mode, void* stream);
/* Norm + AdaLN as one op (every norm of a MaskGiTUViT_v2 TransformerLayer feeds an AdaLNModulation, :757-792):
 *   fwd: v = x (+ res); pre = v (optional); n = Norm(v) * w (mode 0 RMSNorm / 1 LayerNorm); m[b,r,:] = n * (1 + ss[b,:C]) + ss[b,C:],
 *        written as f32 (m) and / or bf16 (m_bf16); n itself is not written.  cols % 4 == 0, cols <= 1024.
 *   bwd: dm = d(m), dpre = the gradient that reached `pre` directly (optional), v = pre.  dv = d(x) = d(res) (+ bf16 copy, optional);
 *        dw_partial [nblk, cols] (muse_colsum -> d(w)); dss_partial [nblk, 2 cols] = (sum dm n | sum dm) over each block's 16 rows,
 *        nblk = muse_norm_res_bwd_nblk(rows); rows_per_batch % 16 == 0, so image b owns rows_per_batch / 16 consecutive blocks:
 *        muse_colsum_segments(dss_partial, dss, batch, rows_per_batch / 16, 2 cols) gives d(ss) [batch, 2 cols].
 * muse_colsum_segments: out[s, c] = sum_{k < seg_rows} part[s * seg_rows + k, c], fixed order. */
int muse_norm_adaln_fwd(const float* x, const float* res, const float* w, const float* ss, float* pre, float* m, void* m_bf16,
                        int32_t batch, int64_t rows_per_batch, int32_t cols, float eps, int32_t mode, void* stream);
int muse_norm_adaln_bwd(const float* dm, const float* dpre, const float* v, const float* w, const float* ss, float* dv, void* dv_bf16,
                        float* dw_partial, float* dss_partial, int32_t batch, int64_t rows_per_batch, int32_t cols, float eps,
                        int32_t mode, void* stream);
/* "bf16x3" mode forms: the f32 result AND its (hi, lo) bf16 operand planes [2][rows][cols] (what muse_split_f32_to_bf16x2 makes of it),
 * so that the products reading m / dv (muse_gemm_x3) need no split pass */
int muse_norm_adaln_fwd_x3(const float* x, const float* res, const float* w, const float* ss, float* pre, float* m, void* planes,
                           int32_t batch, int64_t rows_per_batch, int32_t cols, float eps, int32_t mode, int32_t half, float scale,
                           int32_t* stats, void* stream);
int muse_norm_adaln_bwd_x3(const float* dm, const float* dpre, const float* v, const float* w, const float* ss, float* dv, void* planes,
                           float* dw_partial, float* dss_partial, int32_t batch, int64_t rows_per_batch, int32_t cols, float eps,
                           int32_t mode, int32_t half, float scale, int32_t* stats, void* stream);
int muse_colsum_segments(const float* part, float* out, int32_t nseg, int32_t seg_rows, int32_t cols, void* stream);
int muse_adaln_bwd(const float* dy, const float* x, const float* ss, float* dx, float* dss, int32_t batch,
                   int64_t rows_per_batch, int32_t C, void* stream);
int muse_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
int muse_dwconv3x3_bwd_nchunk(int64_t pixels);
int muse_dwconv3x3_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw_partial, int32_t batch, int32_t H,
                       int32_t W, int32_t C, void* stream);
int muse_grn_bwd(const float* dy, const float* x, const float* gamma, const float* stats, float* dx, float* work,
                 int32_t batch, int64_t S, int32_t C, void* stream);
int muse_scale_rows(float* x, const float* w, const float* num, const float* den, int64_t rows, int32_t cols, int64_t ld,
                    void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CLIP text tower (transformers CLIPTextModel / CLIPTextModelWithProjection, the `type: "clip"` text encoder of the reference's
 * configs: training/train_muse.py:331-338, called every step at :647-649).  Forward only.  (csrc/clip_text.hip)
 * muse_causal_attention_fwd: fused CAUSAL self-attention, bf16 q / k / v / o addressed as for muse_attention_fwd_ex (row strides
 *   free: slices of one packed q | k | v projection; all strides multiples of 8, pointers 16-byte aligned), f32 softmax and
 *   accumulation, MFMA products.  Key j takes part in query i iff j <= i.  seq_q == seq_kv in 1..128 (the sequence is one tile: one
 *   workgroup per (image, head), no S x S matrix in memory), head_dim 32 or 64; anything else MUSE_ERR_UNSUPPORTED.  Rows >= seq of an
 *   image are never read.  Replaces CLIPAttention.forward with the causal mask (transformers models/clip/modeling_clip.py).
 * muse_causal_softmax_fwd: the same mask on materialised scores, [mats][seq][ld] (f32 or bf16): row i of each matrix = softmax over
 *   its columns 0..i, every other column of [0, ld) written as 0; in place capable.  (The exact-f32 mode: between two muse_gemm products.)
 * muse_bias_quick_gelu: y = v * sigmoid(1.702 v), v = x + bias[col], on [rows, cols] f32 or bf16, in place capable
 *   (QuickGELUActivation behind CLIPMLP.fc1, `hidden_act: "quick_gelu"`).
 * muse_layernorm_bias_fwd: y = LayerNorm(x) * w + b in one pass, x f32 [rows, cols], y f32 or bf16 (nn.LayerNorm with its bias:
 *   layer_norm1 / layer_norm2 / final_layer_norm).
 * muse_eos_index: idx[b] = the pooled position of ids[b, :] (int64 [batch, seq]): the first position equal to eos_token_id, or - when
 *   eos_token_id == 2, the legacy rule the openai checkpoints carry - the first position of the row maximum; 0 when nothing matches.
 *   flat_idx (may be NULL) receives b * seq + idx[b], the row muse_gather_rows picks from the [batch * seq, hidden] states. */
int muse_causal_attention_fwd(const muse_attn_desc* d, void* stream);
int muse_causal_softmax_fwd(const void* x, void* y, int32_t dtype, int64_t mats, int32_t seq, int64_t ld, void* stream);
int muse_bias_quick_gelu(const void* x, const float* bias, void* y, int32_t dtype, int64_t rows, int32_t cols, void* stream);
int muse_layernorm_bias_fwd(const float* x, const float* w, const float* b, void* y, int32_t y_dtype, int64_t rows, int32_t cols,
                            float eps, void* stream);
int muse_eos_index(const int64_t* ids, int64_t* idx, int64_t* flat_idx, int32_t batch, int32_t seq, int64_t eos_token_id, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * T5 text encoder (transformers T5EncoderModel, the `type: "t5"` text encoder of the reference's configs:
 * training/train_muse.py:341-343, called every step at :651 as `text_encoder(ids)[0]`).  Forward only.  (csrc/t5_text.hip)
 * muse_bias_attention_fwd: fused BIDIRECTIONAL self-attention with an additive relative-position bias, bf16 q / k / v / o addressed
 *   as for muse_causal_attention_fwd (all strides multiples of 8, pointers 16-byte aligned), f32 softmax and accumulation, MFMA
 *   products.  score(query i, key j) = q_i . k_j + rel[head][j - i + seq - 1] - no scale (d->alpha is not read), no mask: every query
 *   sees every key < seq.  rel: f32 [heads, 2 seq - 1].  seq_q == seq_kv in 1..128 (one tile: one workgroup per (image, head), no
 *   S x S matrix in memory), head_dim 32 or 64; anything else MUSE_ERR_UNSUPPORTED.  Rows >= seq of an image are never read.
 *   Replaces T5Attention.forward of the encoder (transformers models/t5/modeling_t5.py).
 * muse_bias_softmax_fwd: the same bias on materialised f32 scores, [mats][seq][ld]: row i of matrix z = softmax over j < seq of
 *   x[i][j] + rel[z % heads][j - i + seq - 1], columns [seq, ld) written as 0.  y (f32, may be x: in place) and / or y_bf16 (the same
 *   values rounded to bf16, same ld) receive the result; one of them may be NULL.  (Between two muse_gemm products: the exact-f32
 *   mode, and both modes for seq > 128.)
 * muse_gated_gelu_tanh: y[r][c] = gelu_new(ab[r][c]) * ab[r][cols + c] for ab [rows, 2 cols], y [rows, cols], both f32 or both bf16;
 *   gelu_new(x) = 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) (NewGELUActivation behind T5DenseGatedActDense.wi_0, times wi_1).
 * muse_rmsnorm_bf16_fwd: y = bf16(x * rsqrt(mean(x^2) + eps) * w), x f32 [rows, cols] (T5LayerNorm as the bf16 operand of the next
 *   product; the f32 result is muse_norm_res_fwd mode 0).
 * muse_rel_bias_gather: rel[h][t] = table[bucket[t]][h] for t < n: table = relative_attention_bias.weight f32 [buckets, heads],
 *   bucket int64 [n] = the bucket of every signed distance -(seq - 1) .. seq - 1 (computed on the host), rel f32 [heads, n]. */
int muse_bias_attention_fwd(const muse_attn_desc* d, const float* rel, void* stream);
int muse_bias_softmax_fwd(const float* x, float* y, void* y_bf16, const float* rel, int64_t mats, int32_t heads, int32_t seq, int64_t ld,
                          void* stream);
int muse_gated_gelu_tanh(const void* ab, void* y, int32_t dtype, int64_t rows, int32_t cols, void* stream);
int muse_rmsnorm_bf16_fwd(const float* x, const float* w, void* y, int64_t rows, int32_t cols, float eps, void* stream);
int muse_rel_bias_gather(const float* table, const int64_t* bucket, float* rel, int32_t heads, int32_t n, int32_t buckets, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Paella VQ tokenizer (muse/modeling_paella_vq.py, `vq_model.type: "paella_vq"`).  Forward only, f32, channels-last rows
 * [batch*H*W, C] with C % 4 == 0.  Every element offset inside these kernels is 64-bit; int32 arguments are sides and channel counts.
 * (csrc/paella.hip)
 * muse_paella_mix_fwd: the first half of ResBlock.forward (:141-142) over x [batch*H*W, C], C <= 1024:
 *     y = x + g2 * (dwconv3x3_replicate(LN(x) * (1 + g0) + g1) + bias)
 *   LN = LayerNorm over the C channels of a pixel, no affine, eps 1e-6, biased variance; the depthwise 3x3 reads its neighbours with
 *   edge replication (ReplicationPad2d(1): an out-of-range coordinate clamps to the border, H == 1 / W == 1 included).  w9 [9][C]
 *   (tap-major: depthwise.1.weight [C, 1, 3, 3] permuted once), bias [C], gammas = DEVICE pointer to the block's six floats (g0, g1, g2
 *   are read by the kernel: no host read).  stats: [batch*H*W, 2] f32 workspace (mean, rstd of every pixel, written by a first pass; the
 *   normalised tensor itself is never written).  y must not alias x.
 * muse_patch_rows_nhwc: y[(b, oy, ox)][(ky, kx, c)] = x[b, oy*stride - pad_top + ky, ox*stride - pad_left + kx, c], zero outside the
 *   image; KS 2 | 4; y [batch*Hout*Wout, KS*KS*C].  Conv2d(4, 2, 1) (:163) = this with (4, 2, 1, 1) + one product with K = 16 Cin;
 *   ConvTranspose2d(4, 2, 1) (:185-187) = four output phases (a, b), each this with KS 2, stride 1, pad (1 - a, 1 - b), Hout = H,
 *   Wout = W + one product with the taps (3 - a - 2 ky, 3 - b - 2 kx), interleaved by muse_space_to_depth2_nhwc(inverse).
 * muse_vq_nearest_small: idx[r] = argmin_j sum_k (z[r, k] - codebook[j, k])^2 for D <= 8 (VectorQuantizer.get_code :103-109 at
 *   c_latent 4), the sum taken directly with fma in ascending k; the lowest index wins among exactly equal distances.  z [N, D] f32 with
 *   row stride ldz, codebook [Kc, D] f32 contiguous, idx int64 [N], dist (may be NULL) f32 [N] = the winning squared distance.  No
 *   [N, Kc] distance matrix exists.
 * muse_paella_in_block: in_block (:159) = PixelUnshuffle(2) + 1x1 convolution 12 -> C of img [batch, 3, H, W] f32 NCHW (H, W even)
 *   -> y [batch*(H/2)*(W/2), C]; w12 [12][C] (in_block.1.weight transposed; unshuffled channel k = c*4 + dy*2 + dx), bias [C].
 * muse_paella_out_block: out_block (:190-193) = 1x1 convolution C -> 12 + PixelShuffle(2): x [batch*(H/2)*(W/2), C] -> img [batch, 3,
 *   H, W] f32 NCHW; w12 [12][C] (out_block.0.weight as it is), bias [12].  H, W are the IMAGE sides in both. */
int muse_paella_mix_fwd(const float* x, const float* w9, const float* bias, const float* gammas, float* stats, float* y, int32_t batch,
                        int32_t H, int32_t W, int32_t C, void* stream);
int muse_patch_rows_nhwc(const float* x, float* y, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t KS, int32_t stride,
                         int32_t pad_top, int32_t pad_left, int32_t Hout, int32_t Wout, void* stream);
int muse_vq_nearest_small(const float* z, int64_t ldz, const float* codebook, int64_t* idx, float* dist, int64_t N, int32_t D, int32_t Kc,
                          void* stream);
int muse_paella_in_block(const float* img, const float* w12, const float* bias, float* y, int32_t batch, int32_t H, int32_t W, int32_t C,
                         void* stream);
int muse_paella_out_block(const float* x, const float* w12, const float* bias, float* img, int32_t batch, int32_t H, int32_t W, int32_t C,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MoVQ tokenizer (muse/modeling_movq.py, `vq_model.type: "movq"`): SpatialNorm (:21-49) over NHWC in one apply pass (csrc/movq.hip)
 *     out = GroupNorm(x) * conv_y(nearest(zq)) + conv_b(nearest(zq)), then SiLU when apply_silu
 * x [batch, H, W, C] f32; zq [batch, zh, zw, Z] f32 (the quantised latent, 1 <= Z <= 8; H % zh == 0 and W % zw == 0: output pixel
 * (oy, ox) reads source pixel (oy / (H / zh), ox / (W / zw)), F.interpolate(mode="nearest") for integer factors; the two factors are
 * independent); gamma / beta [C] the GroupNorm affine; wy [C][Z], by [C] = conv_y, wb [C][Z], bb [C] = conv_b (1x1 convolutions).
 * Per element, all f32: n = fma(x, rstd * gamma, beta - rstd * gamma * mean); m = by + sum_k wy[k] zq[k] and a = bb + sum_k wb[k] zq[k]
 * (fma, k ascending); out = fma(n, m, a).  mean / rstd come from f64 partial sums folded as muse_groupnorm_silu_nhwc_split folds them.
 * Exactly one output form: y (f32 tensor; SiLU with the correctly rounded division) or y_hi AND y_lo (the bf16 operand planes of
 * muse_conv2d_nhwc_split2: hi = bf16(out), lo = bf16(out - hi); SiLU with the hardware reciprocal, as the GroupNorm plane route) -
 * both or neither: MUSE_ERR_BAD_ARG.  partial / stats_nchunk as for muse_groupnorm_silu_nhwc_split (0: the statistics pass runs here
 * and `partial` needs batch * muse_groupnorm_nchunk(H * W) * groups * 2 doubles; > 0: `partial` holds a producer's [batch,
 * stats_nchunk, groups, 2] sums and x is read once).  groups 32 or 64, C % groups == 0, C % 4 == 0, C <= 2048 and C / 4 a divisor of
 * 256 or larger than it, else MUSE_ERR_UNSUPPORTED; x / y / zq (Z % 4 == 0) 16-byte aligned.  Every element offset is 64-bit. */
int muse_spatial_norm_nhwc(const float* x, float* y, void* y_hi, void* y_lo, const float* gamma, const float* beta, const float* zq,
                           const float* wy, const float* by, const float* wb, const float* bb, double* partial, int32_t stats_nchunk,
                           int32_t batch, int32_t H, int32_t W, int32_t C, int32_t zh, int32_t zw, int32_t Z, int32_t groups, float eps,
                           int32_t apply_silu, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Pre-encode image stage (muse/pre_encode.py resize_center_crop; csrc/resize.hip): what scripts/pre_encode.py:449-489 does per image in
 * front of get_code - uint8 HWC -> CHW f32 / 255 -> TF.resize(BILINEAR, antialias=True) -> crop (-> flip) -> stack - for a ragged
 * batch in ONE launch.
 * Value.  Image b is `H x W x 3` uint8; its resized size (oh, ow) and its window origin (top, left) come from the table (the host
 * computes them: torchvision's _compute_resized_output_size / center_crop, or a random crop).  Per axis (in = source length, out =
 * resized length, i = resized index), every step ONE rounded f32 operation, none contracted into a multiply-add:
 *     scale = f32(in) / f32(out);  support = scale >= 1 ? scale : 1;  inv = scale >= 1 ? 1 / scale : 1;  center = scale * (i + 0.5)
 *     lo = max(trunc((center - support) + 0.5), 0);  hi = min(trunc((center + support) + 0.5), in)
 *     w_s = max(0, 1 - |((f32(s) - center) + 0.5) * inv|) for s = lo .. hi - 1;  w_s /= (w_lo + w_lo+1 + ..., in this order)
 *   i.e. ATen's antialias bilinear weights of F.interpolate(mode="bilinear", antialias=True, align_corners=False) bit for bit.
 *     src = f32(u8) / 255 (correctly rounded);  tmp[y][x] = sum_s src[y][s] * wx_s;  res[i][x] = sum_s tmp[s][x] * wy_s
 *   both sums from the lowest tap upwards with fma, tmp rounded to f32 (horizontal pass first, as ATen's separable kernel).
 *     out[b][c][y][x] = res[top + y][left + (flip ? R - 1 - x : x)]  for 0 <= y, x < R: a flip AFTER the crop.
 *   Tap counts are not capped (source rows are streamed), sizes are not bounded by LDS.
 * What is read and written.  packed: device bytes; image b occupies [offset, offset + 3 H W) as HWC, at ANY byte offset, gaps between
 * images allowed; no byte outside the listed images is read.  table: device int64 [B][8] = (offset, H, W, oh, ow, top, left, flip),
 * 8-byte aligned; the rows are NOT validated here (they live on the device): the caller guarantees H, W >= 1, oh, ow >= R,
 * 0 <= top <= oh - R, 0 <= left <= ow - R and that the image lies inside `packed` (muse.ops.resize_crop_u8 checks every row on the
 * host).  out: f32 [B][3][R][R] contiguous, 4-byte aligned; nothing else is written.
 * B < 1, R < 1 or a NULL pointer: MUSE_ERR_BAD_ARG, nothing is launched.  B > 65535 or R > 16 * 65535: MUSE_ERR_UNSUPPORTED. */
int muse_resize_crop_u8(const void* packed, const void* table, void* out, int32_t B, int32_t R, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CLIP image tower (muse/modeling_clip_vision.py: transformers CLIPVisionModelWithProjection, and the image / text similarity of
 * CLIPModel - the scorer of scripts/gen_sdxl_synthetic_dataset.py:34-36,98-105 and benchmark/model_quality.py:32-111).  Forward only,
 * f32 in.  The encoder layers run on muse_gemm, muse_attention_fwd_ex, muse_layernorm_bias_fwd and muse_bias_quick_gelu.
 * (csrc/clip_vision.hip)
 * muse_resize_bicubic_norm_f32: x f32 [B, 3, R, R] -> out f32 [B, 3, I, I] = (resize(x) - mean[c]) / std[c], both contiguous, 4-byte
 *   aligned.  resize is the separable antialiased bicubic of F.interpolate(x, (I, I), mode="bicubic", antialias=True,
 *   align_corners=False): per axis, every step one rounded f32 operation,
 *     scale = f32(R) / f32(I);  support = 2 max(scale, 1);  inv = scale >= 1 ? 1 / scale : 1;  center = scale * (i + 0.5)
 *     lo = max(trunc((center - support) + 0.5), 0);  hi = min(trunc((center + support) + 0.5), R, lo + 2 ceil(support) + 1)
 *     w_s = k(((f32(s) - center) + 0.5) * inv) for s = lo .. hi - 1, k = Keys' cubic with a = -0.5;  w_s /= (w_lo + w_lo+1 + ...)
 *   horizontal pass first, both sums from the lowest tap upwards with fma, the intermediate rounded to f32 and NOT clamped (the cubic's
 *   overshoot below 0 / above 1 is kept), no intermediate image in memory.  R > I, R < I and R == I all run; for R == I the weights are
 *   exactly (.., 0, 1, 0, ..) and the output is (x - mean[c]) / std[c] with the correctly rounded f32 quotient.  mean3 / std3 are HOST
 *   pointers to three floats each.  B > 65535, I > 16 * 65535 or a side >= 2^24: MUSE_ERR_UNSUPPORTED.
 * muse_clip_patch_rows: x f32 [B, 3, I, I] -> y [B * G * G, Kp] (f32 or bf16, round to nearest even), G = I / P, Kp = 3 P P rounded up
 *   to a multiple of 8 (any other Kp, or I % P != 0: MUSE_ERR_BAD_ARG): y[(b, gy, gx)][(c, ky, kx)] = x[b][c][gy P + ky][gx P + kx],
 *   columns >= 3 P P written as 0 - the (c, ky, kx) flattening of Conv2d(3, H, P, stride=P).weight, so the patch embedding is one
 *   muse_gemm against the weight padded to [H, Kp].  y 16-byte aligned; nothing outside [y, y + B G G Kp) is written.
 * muse_clip_vision_embed_ln: y[(b, t)] = LayerNorm((t == 0 ? class_embedding : patch[b (tokens - 1) + t - 1]) + position_embedding[t])
 *   * w + b for t < tokens: patch f32 [batch * (tokens - 1), hidden], position_embedding [tokens, hidden], y f32 [batch * tokens, hidden];
 *   biased variance of the centred values, eps inside the square root (nn.LayerNorm: CLIPVisionEmbeddings + pre_layrnorm in one pass).
 *   hidden % 4 == 0 and hidden <= 2048 (the row lives in registers), else MUSE_ERR_UNSUPPORTED; all pointers 16-byte aligned.
 * muse_l2_normalize_rows: y[r] = x[r] / sqrt(sum_c x[r][c]^2) for x f32 [rows, cols] contiguous, then * mult when has_mult, then
 *   * exp(*log_mult) when log_mult (a DEVICE pointer to one float: CLIPModel.logit_scale, no host read) is not NULL.  No epsilon: a
 *   zero row becomes NaN, as x / x.norm(dim=-1, keepdim=True).  In place capable. */
int muse_resize_bicubic_norm_f32(const float* x, float* out, int32_t B, int32_t R, int32_t I, const float* mean3, const float* std3,
                                 void* stream);
int muse_clip_patch_rows(const float* x, void* y, int32_t y_dtype, int32_t B, int32_t I, int32_t P, int32_t Kp, void* stream);
int muse_clip_vision_embed_ln(const float* patch, const float* class_embedding, const float* position_embedding, const float* w,
                              const float* b, float* y, int32_t batch, int32_t tokens, int32_t hidden, float eps, void* stream);
int muse_l2_normalize_rows(const float* x, float* y, int64_t rows, int32_t cols, float mult, int32_t has_mult, const float* log_mult,
                           void* stream);

/* ---- masked-token logging diagnostics (diag.hip): muse/training_utils.py:299-397 of the reference, called by training/train_muse.py
 * :812-847 on the step's own logits.  Both read logits [rows, ld] (f32 or bf16, first `vocab` columns valid, any element-aligned base
 * and any ld >= vocab: rows off 16-byte alignment are read through a peeled head and tail, never past column `vocab`), accumulate in
 * f32, use no atomics and allocate nothing.  A row's results are a function of the row's values alone - not of its address, `ld` or
 * the other rows - and the same bits on every run.  vocab > ld, a NULL required pointer or another dtype: MUSE_ERR_BAD_ARG.
 * muse_token_stats: per row, lse[r] = logsumexp(x[r]) and entropy[r] = -sum_v p log p with p = softmax(x[r]), from ONE read of the row:
 *   an online (max m, s = sum e^(x - m), t = sum e^(x - m) (x - m)) gives lse = m + log s and entropy = log s - t / s (which is
 *   lse - sum(e x) / sum(e) with m taken out of both terms).  row_mask (NULL = every row) holds one byte per row: a row whose byte is 0
 *   is not loaded, its entropy is written as 0 and its lse is unspecified.  row_max, sum_exp (both or neither; NULL = not wanted)
 *   receive m and s themselves, for muse_masked_mean_probs.  Replaces the softmax, log_softmax and their product of
 *   pixel_entropy_per_percent_masked_bucket (:304-307).
 * muse_masked_mean_probs: per image b, mean_probs[b, v] = (sum over s with input_ids[b, s] == mask_id, ascending, of
 *   exp(x[b, s, v] - lse[b S + s])) / n_masked[b], logits seen as [batch * seq, ld]; rows that are not masked are not loaded.  The
 *   row's lse comes in as the pair (row_max, sum_exp) of muse_token_stats, valid for at least the masked rows, and the term is
 *   evaluated as exp(x - max) * (1 / sum): a rounded lse near 10 would put a common relative error of 5e-7 on a row's probabilities.
 *   mean_probs f32 [batch, vocab] contiguous.  entropy (NULL = skip) f32 [batch]: -sum_v mean_probs log(mean_probs) by a second small
 *   launch over mean_probs (one block per image, fixed summation order).  The reference's expression as it stands (:329-336): an image
 *   with no masked token gives NaN (0 / 0), a code whose mean probability is exactly 0 gives NaN (0 * -inf).  batch <= 65535, else
 *   MUSE_ERR_UNSUPPORTED.
 * muse_masked_row_mean: out[b] = (sum_s values[b, s]) / #{s : input_ids[b, s] == mask_id} for values f32 [batch, seq] contiguous -
 *   entropy_per_pixel.sum(-1) / num_masked_pixels (:312-313) on muse_token_stats' entropies (exact zeros where not masked).  One block
 *   per image, a fixed summation order: an image's mean is the same bits in any batch.  No masked token: NaN (0 / 0). */
int muse_masked_row_mean(const float* values, const int64_t* input_ids, float* out, int32_t batch, int32_t seq, int64_t mask_id,
                         void* stream);
int muse_token_stats(const void* logits, int32_t dtype, const uint8_t* row_mask, float* lse, float* entropy, float* row_max, float* sum_exp,
                     int64_t rows, int32_t vocab, int64_t ld, void* stream);
int muse_masked_mean_probs(const void* logits, int32_t dtype, const int64_t* input_ids, const float* row_max, const float* sum_exp,
                           float* mean_probs, float* entropy, int32_t batch, int32_t seq, int32_t vocab, int64_t ld, int64_t mask_id,
                           void* stream);

/* ---- feature statistics for the Frechet distance on CLIP image embeds (moments.hip; muse/frechet.py: FeatureStats.update) - the
 * accumulation behind the reference's fid.compute_fid (scripts/calculate_fid.py:215-220, tabulated by benchmark/model_quality.py:18-60), on the features of
 * muse.CLIPImageEncoder instead of an Inception network.
 * muse_moments_f64: for x f32 [n, d] with row stride ldx >= d (elements), IN PLACE,
 *     sum[i]      += sum_n (double)x[n][i]                        sum f64 [d]
 *     outer[i][j] += sum_n (double)x[n][i] * (double)x[n][j]      outer f64 [d, d] row-major, j >= i only
 *   The strict lower triangle of outer is neither read nor written.  Products are formed in f64 from the converted f32 values and are
 *   therefore exact (24 + 24 < 53 bits); only the additions round, one rounding each, on v_mfma_f64_16x16x4_f64.  One workgroup per
 *   64 x 64 tile of the upper triangle, every output element owned by one lane, no atomics, no workspace.  Rows are consumed in ascending
 *   order in groups of four counted from row 0 of the call, a ragged last group padded with zeros (not with clamped addresses): equal
 *   call sequences give equal bits.  inf / NaN propagate as in x^T x.  No byte of x outside the n rows' first d columns is read.
 *   d <= 0, d % 4 != 0, n < 0, ldx < d or a NULL pointer: MUSE_ERR_BAD_ARG.  x not 16-byte aligned, sum or outer not 8-byte aligned:
 *   MUSE_ERR_ALIGN.  More than 2^31 - 1 tiles (d > 4,194,240): MUSE_ERR_UNSUPPORTED.  A refused call launches and writes nothing.
 *   n == 0 (with valid arguments) returns 0 and launches nothing. */
int muse_moments_f64(const float* x, int64_t n, int32_t d, int64_t ldx, double* sum, double* outer, void* stream);

/* ---- Gaussian-kernel pair sums for the maximum mean discrepancy on CLIP image embeds (mmd.hip; muse/mmd.py: mmd_distance,
 * cmmd_distance - CMMD of Jayasumana et al., "Rethinking FID", CVPR 2024).  All arithmetic is f64 on the converted f32 features; a
 * product of two converted values is exact, so inside a dot product only the additions round.  No n x m matrix is ever written.
 * muse_row_norms_f64: x f32 [n, d], row stride ldx >= d (elements).  sumsq[i] = sum_k (double)x_ik^2 (one wave per row: lane l adds
 *   features 4 l + 256 t + (0 .. 3), t ascending, by fma of the exact squares, then a butterfly over the 64 lanes - an order fixed by d
 *   alone); rinv (NULL = skip) [i] = 1.0 / sqrt(sumsq[i]), IEEE sqrt and quotient.  A zero row gives rinv = inf, and NaN in whatever
 *   multiplies it by that row: not guarded.
 * muse_rbf_pair_sums_f64: with c_ij = (rx_i ry_j) sum_k (double)x_ik (double)y_jk, a_i = (rx_i rx_i) sum_k x_ik^2, b_j likewise from y,
 *   k_ij = exp(-gamma ((a_i + b_j) - 2 c_ij)) - no clamp of the squared distance at 0.  rx / ry f64 [n] / [m]; NULL = a factor of 1,
 *   bit-identical to an array of ones.
 *     y != NULL (rectangular): out[0] = sum_{i < n, j < m} k_ij, out[1] = 0
 *     y == NULL (symmetric; ry, m, ldy ignored): only tiles on or above the diagonal are computed, out[0] = sum_{i < j} k_ij,
 *       out[1] = sum_i k_ii as computed (not assumed 1): the full sum is 2 out[0] + out[1]
 *   One workgroup of four waves per 64 x 64 tile of pairs on v_mfma_f64_16x16x4_f64 with K along the feature axis (a lane loads 16
 *   contiguous bytes of its row per step of 16 features; the order of k in a dot product is a fixed permutation, the same for both
 *   operands).  A row >= n or a column >= m is excluded from the sums by predicate; loads beyond n, m or d are predicated off, never a
 *   clamped address.  Every wave writes its partial(s) to `workspace` (muse_rbf_pair_sums_workspace(n, m, symmetric) doubles: 4 per
 *   tile, twice that when symmetric), a second launch of one workgroup adds them in a fixed order: no floating-point atomics, equal
 *   calls give equal bits, and the bits do not depend on ldx / ldy.  inf / NaN features give NaN sums.
 *   gamma is read from HOST memory at the call (one f64; the prototype check of this header knows no by-value double).
 *   Because a lane loads a float4, rows must start 16-byte aligned: x, y 16-byte aligned AND ldx, ldy multiples of 4, else MUSE_ERR_ALIGN;
 *   rx, ry, workspace, out (sumsq, rinv) 8-byte aligned, else MUSE_ERR_ALIGN.  d <= 0, d % 4 != 0, n < 0, m < 0, a stride < d, a NULL x /
 *   gamma / workspace / out (sumsq): MUSE_ERR_BAD_ARG.  More than 2^31 - 1 tiles (or row blocks): MUSE_ERR_UNSUPPORTED.  A refused call
 *   launches and writes nothing.  n == 0 or m == 0 (with valid arguments): out = {0, 0}, no pair kernel.
 * muse_rbf_pair_sums_workspace: the number of f64 partials, or a negative MUSE_ERR_* for negative sizes / too many tiles. */
int muse_row_norms_f64(const float* x, int64_t n, int32_t d, int64_t ldx, double* sumsq, double* rinv, void* stream);
int64_t muse_rbf_pair_sums_workspace(int64_t n, int64_t m, int32_t symmetric);
int muse_rbf_pair_sums_f64(const float* x, int64_t n, int64_t ldx, const double* rx, const float* y, int64_t m, int64_t ldy,
                           const double* ry, int32_t d, const double* gamma, double* workspace, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSE_HIP_H */
