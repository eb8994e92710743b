// The optimizer step and the weight average behind it: AdamW (torch.optim.AdamW / apex FusedAdam adam_w_mode) and Lion (the reference's
// training/optimizer.py) in their flat-buffer, flat-buffer with parameter groups and multi-tensor forms, and the exponential moving
// average of the weights.  All HBM-bound: 7 x 4 B per parameter of traffic for AdamW, 5 x 4 B for Lion (+ 2 B for a bf16 copy, + 4 B for
// operand planes), 16-byte accesses where the pointers allow them.
//
// An update RULE (AdamRule | LionRule) is one statement of the update of one element (adam_update1 | lion_update1), the constants it
// reads (AdamHyper | LionHyper, filled on the host by adam_hyper | lion_hyper) and whether it owns a second moment `v`.  Everything else
// is written once and instantiated per rule: ONE routine that covers a span of a tensor by a workgroup (adam_span), the image stores, the
// skip guard, and three kernels, each in a host-factor and a device-factor (*_dev) instantiation:
//   opt_flat_kernel           one hyper-parameter set over a flat f32 buffer, grid-stride over quads (the kernel inside the benched step:
//                             it runs range by range from backward on the weight-gradient stream)
//   opt_flat_groups_kernel    a flat buffer cut into segments of different parameter groups; block b owns elements [4096 b, 4096 b + 4096)
//   opt_multi_kernel          ONE launch over a device-side table of tensors (models whose parameters are ordinary tensors, not views of
//                             a flat buffer: MaskGiTUViT has ~500, and 500 launches of 9 us each were 4 % of its step); block b owns chunk b
// A one-group call of the grouped forms is bit-identical to the single-set forms: they run the same statements.
// The Lion instantiations never load or store `v`: the pointer (the flat forms' argument, column 3 of the tables) may be NULL.
//
// Parameter groups (training/train_muse.py:425-445: no weight decay on bias / LayerNorm / embedding weights).  torch.optim semantics: every
// group carries its own lr / betas / eps / weight_decay.  The per-group constants are computed on the host exactly like the single set and
// travel BY VALUE in the kernel arguments (they change every step with the lr schedule: no host -> device copy).
//
// Tables of the multi-tensor form.  6 x int64 per tensor: {p, g, m, v, p_bf16 or 0, n} (muse_adamw_multi: group 0, p_bf16 a plain bf16 copy);
// 7 x int64 per tensor: {p, g, m, v, p_bf16 or 0, n, group | lo_plane_distance << 8} (muse_adamw_multi_groups).  `chunk_first[t]` = index of
// tensor t's first 4096-element chunk (exclusive prefix sum, nt + 1 entries); block b owns chunk b: binary search -> (tensor, offset).
// Column 6 above bit 8: p_bf16 is the HI plane of the parameter's bf16x3 operand planes and the lo plane sits that many elements behind
// it (hi = bf16(p), lo = bf16(p - hi): split_f2bb_kernel's arithmetic) - the planes the next step's weight GEMMs read; 0 = a plain bf16 copy
// ... and a NEGATIVE value there: p_bf16 is an IEEE-half copy instead (the weight's operand image of the "f16" compute mode).
//
// Overflow guard of the "f16" compute mode (the `skip` argument of every AdamW entry point): when non-NULL, every AdamW kernel (flat, flat
// groups, multi-tensor) reads *skip first and leaves every tensor untouched if it is non-zero - the gradients of a backward pass whose operand
// images overflowed half's range are NaN, and the update is skipped ON THE DEVICE (torch.cuda.amp.GradScaler's found_inf, without a host
// round trip).  NULL = no guard.
#include "common.h"
#include "../../include/muse_hip.h"
#include <math.h>
#include <type_traits>

#define OPT_CHUNK 4096   // elements a workgroup of the chunked kernels owns (GN_CHUNK of gradnorm.hip: one chunk_first table serves both)
#define MUSE_ADAMW_MAX_GROUPS 8
struct AdamHyper { float b2, eps, decay, omb1, omb2, step_size, bc2_sqrt, pad; };
struct LionHyper { float decay, b1, omb1, b2, omb2, nlr, pad[2]; };
template <class R> struct OptGroups { typename R::Hyper h[MUSE_ADAMW_MAX_GROUPS]; };

// ---- host: the constants of one hyper-parameter set at step `step`, in double precision, each rounded once --------------------------------
static AdamHyper adam_hyper(float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
  const auto bias_correction = [step](float beta) { return 1.0 - pow((double)beta, (double)step); };
  const double bc1 = bias_correction(beta1), bc2 = bias_correction(beta2);
  AdamHyper h;
  h.step_size = (float)((double)lr / bc1);
  h.bc2_sqrt = (float)sqrt(bc2);
  h.decay = (float)(1.0 - (double)lr * (double)weight_decay);
  h.omb1 = (float)(1.0 - (double)beta1); h.omb2 = (float)(1.0 - (double)beta2);
  h.b2 = beta2; h.eps = eps; h.pad = 0.f;
  return h;
}
// Lion has no step count and no bias correction.  The hyper-parameters cross the C ABI as DOUBLE, one row {lr, beta1, beta2, weight_decay}:
// decay is f32(1 - lr * wd) of the Python floats (`p.data.mul_(1 - lr * wd)`), which a lr already rounded to f32 does not reproduce.
static LionHyper lion_hyper(const double* row) {
  const double lr = row[0], beta1 = row[1], beta2 = row[2], weight_decay = row[3];
  LionHyper h;
  h.decay = (float)(1.0 - lr * weight_decay);
  h.b1 = (float)beta1; h.omb1 = (float)(1.0 - beta1);
  h.b2 = (float)beta2; h.omb2 = (float)(1.0 - beta2);
  h.nlr = (float)(-lr); h.pad[0] = h.pad[1] = 0.f;
  return h;
}

// ---- device: the update of one element ----------------------------------------------------------------------------------------------------
// Every rounding is written out: the statements below run with contraction OFF, each `fmaf` is one fused multiply-add (one rounding) and
// every other operator rounds its own result to f32.  sqrtf and `/` are the correctly rounded sequences, f32 denormals are kept.
//   gr = round(g * s)                                  the gradient times its factor
//   d  = round(gr - m)          (device factor)        |  fma(g, s, -m)   (host factor: the unrounded product, one rounding)
//   m' = fma(omb1, d, m)                               exp_avg.lerp_(grad, 1 - beta1)
//   v' = fma(omb2, round(gr * gr), round(v * b2))      exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
//   denom = round(round(sqrt(v') / bc2_sqrt) + eps)
//   p' = fma(decay, p, round(-step_size * round(m' / denom)))
// The last line is NOT param.mul_(1 - lr * weight_decay) followed by param.addcdiv_: the decayed parameter is never rounded on its own.
// It is what the compiler made of the two source statements before the roundings were written down, kept so that no weight changes; it
// is the more accurate of the two (one rounding less).
// The host-factor form fuses g * s into the difference only (invisible for a power of two, which the host's grad_scale is); the device
// factor (grad_scale * clip coefficient written by muse_gradnorm_finalize) is applied as one rounded product everywhere, so "scale
// inside the kernel" and "scale the buffer, then step" are the same bits.  adam_quad and adam_one both run exactly this.
template <bool DEV> __device__ __forceinline__ float grad_times(float g, float s) {
#pragma clang fp contract(off)
  float r = g * s;
  if constexpr (DEV) asm volatile("" : "+v"(r));  // (no longer needed for the rounding: it keeps the *_dev kernels' instruction selection as it was)
  return r;
}
template <bool DEV> __device__ __forceinline__ void adam_update1(float& pp, float g, float s, float& mm, float& vv, const AdamHyper& h) {
#pragma clang fp contract(off)
  const float gr = grad_times<DEV>(g, s);
  const float d = DEV ? gr - mm : fmaf(g, s, -mm);
  mm = fmaf(h.omb1, d, mm);
  const float g2 = gr * gr, vb = vv * h.b2;
  vv = fmaf(h.omb2, g2, vb);
  const float denom = sqrtf(vv) / h.bc2_sqrt + h.eps;
  const float t = -h.step_size * (mm / denom);     // (the sign on the uniform factor: negating m or t costs a vector instruction)
  pp = fmaf(h.decay, pp, t);
}
// Lion (training/optimizer.py:57-79), under the same conventions; host and device factor run the same statements:
//   gr = round(g * s)                     s == 1 leaves g's bits
//   p1 = round(p * decay)                 p.data.mul_(1 - lr * wd): here the decayed parameter IS rounded on its own
//   u  = round(round(m * b1) + round(gr * omb1))
//   p' = round(p1 + nlr * sign(u))        sign: +1, -1, +0 for u == +-0 (p' then has p1's bits, -0.0 included), NaN for NaN
//   m' = fma(omb2, gr, round(m * b2))     exp_avg.mul_(beta2).add_(grad, alpha=1 - beta2): ATen's add-with-alpha is a fused multiply-add
// u is made of the OLD m, m' does not reuse round(m * b1), and there is no second moment: vv is neither read nor written.
__device__ __forceinline__ void lion_update1(float& pp, float g, float s, float& mm, const LionHyper& h) {
#pragma clang fp contract(off)
  const float gr = g * s;
  const float p1 = pp * h.decay;
  const float a = mm * h.b1, b = gr * h.omb1;
  const float u = a + b;
  const float sg = u > 0.f ? 1.f : (u < 0.f ? -1.f : (u == 0.f ? 0.f : u));
  const float t = h.nlr * sg;
  pp = p1 + t;
  const float mb = mm * h.b2;
  mm = fmaf(h.omb2, gr, mb);
}
// the two rules: the constants, whether there is a second moment, the update of one element
struct AdamRule {
  typedef AdamHyper Hyper;
  typedef float HostScalar;            // element type of a row of its group table
  static constexpr bool HAS_V = true;
  template <bool DEV> static __device__ __forceinline__ void update1(float& pp, float g, float s, float& mm, float& vv, const Hyper& h) {
    adam_update1<DEV>(pp, g, s, mm, vv, h);
  }
};
struct LionRule {
  typedef LionHyper Hyper;
  typedef double HostScalar;
  static constexpr bool HAS_V = false;
  template <bool DEV> static __device__ __forceinline__ void update1(float& pp, float g, float s, float& mm, float&, const Hyper& h) {
    lion_update1(pp, g, s, mm, h);
  }
};
// the kernel argument that carries the factor: the value itself, or (DEV) where to read it on the device
template <bool DEV> using GradFactor = std::conditional_t<DEV, const float*, float>;
// every kernel begins here: false = `skip` (the f16 mode's overflow guard) says leave everything untouched; else the factor -> gscale
template <bool DEV> __device__ __forceinline__ bool adam_begin(GradFactor<DEV> factor, const int* __restrict__ skip, float& gscale) {
  if (skip && *skip != 0) return false;
  if constexpr (DEV) gscale = *factor; else gscale = factor;
  return true;
}

// The copy of the updated parameter that the update refreshes: none (pb == NULL), a bf16 copy (plo == 0), the bf16 hi plane at pb with the lo
// plane plo elements behind it, or (half) an IEEE-half copy.
struct AdamImage { bf16_t* pb; long plo; bool half; };
// elements [i, i + 4) by 16-byte accesses (8-byte for the image): i and every pointer aligned to that
template <class R, bool DEV> __device__ __forceinline__ void adam_quad(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                       float* __restrict__ v, const AdamImage& im, long i,
                                                                       const typename R::Hyper& h, float gscale) {
  float pp[4], gg[4], mm[4], vv[4];
  V4<float>::load(p + i, pp); V4<float>::load(g + i, gg); V4<float>::load(m + i, mm);
  if constexpr (R::HAS_V) V4<float>::load(v + i, vv);
#pragma unroll
  for (int j = 0; j < 4; ++j) R::template update1<DEV>(pp[j], gg[j], gscale, mm[j], vv[j], h);
  V4<float>::store(p + i, pp); V4<float>::store(m + i, mm);
  if constexpr (R::HAS_V) V4<float>::store(v + i, vv);
  if (im.pb && im.half) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    *(h4*)(im.pb + i) = h4{(_Float16)pp[0], (_Float16)pp[1], (_Float16)pp[2], (_Float16)pp[3]};
  } else if (im.pb) {
    V4<bf16_t>::store(im.pb + i, pp);
    if (im.plo) {
      float rr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) rr[j] = pp[j] - bf16_to_f32(f32_to_bf16(pp[j]));
      V4<bf16_t>::store(im.pb + im.plo + i, rr);
    }
  }
}
// element i alone
template <class R, bool DEV> __device__ __forceinline__ void adam_one(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                      float* __restrict__ v, const AdamImage& im, long i,
                                                                      const typename R::Hyper& h, float gscale) {
  float pp = p[i], mm = m[i], vv;
  if constexpr (R::HAS_V) vv = v[i];
  R::template update1<DEV>(pp, g[i], gscale, mm, vv, h);
  p[i] = pp; m[i] = mm;
  if constexpr (R::HAS_V) v[i] = vv;
  if (im.pb && im.half) {
    ((_Float16*)im.pb)[i] = (_Float16)pp;
  } else if (im.pb) {
    const bf16_t hi = f32_to_bf16(pp);
    im.pb[i] = hi;
    if (im.plo) im.pb[im.plo + i] = f32_to_bf16(pp - bf16_to_f32(hi));
  }
}
// Elements [lo, hi) of one tensor by one workgroup of 256 (lo a multiple of 4, hi - lo <= OPT_CHUNK): quads, then the (hi - lo) % 4 tail
// alone - or every element alone when a pointer (or the plane distance) does not allow the vector accesses.
// (a rule without a second moment does not look at v at all)
template <class R, bool DEV> __device__ __forceinline__ void adam_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                       float* __restrict__ v, const AdamImage& im, long lo, long hi,
                                                                       const typename R::Hyper& h, float gscale) {
  const uintptr_t vbits = R::HAS_V ? (uintptr_t)v : 0;
  const bool vec = !((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | vbits) & 15) && !(((uintptr_t)im.pb) & 7) && !(im.plo & 3);
  if (vec)
    for (long i = lo + threadIdx.x * 4; i + 3 < hi; i += 1024) adam_quad<R, DEV>(p, g, m, v, im, i, h, gscale);
  for (long i = (vec ? lo + ((hi - lo) & ~3L) : lo) + threadIdx.x; i < hi; i += 256) adam_one<R, DEV>(p, g, m, v, im, i, h, gscale);
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------
template <class R, bool DEV>
__global__ __launch_bounds__(256) void opt_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, bf16_t* __restrict__ pb, long n, typename R::Hyper h,
                                                       GradFactor<DEV> factor, const int* __restrict__ skip) {
  float gscale;
  if (!adam_begin<DEV>(factor, skip, gscale)) return;
  const AdamImage im = {pb, 0, false};
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) adam_quad<R, DEV>(p, g, m, v, im, i * 4, h, gscale);
  // tail (n % 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) adam_one<R, DEV>(p, g, m, v, im, (n4 << 2) + threadIdx.x, h, gscale);
}

// Flat buffer cut into segments: seg_end[s] (ascending, ABSOLUTE element offsets in the flat buffer) closes segment s, seg_group[s]
// names its parameter group.  The call covers elements [base, base + n) of the flat buffer (p, g, m, v, pb point at element `base`):
// any slice, so the in-backward / behind-the-all-reduce range updates share the table.  Block b owns elements [4096 b, 4096 b + 4096)
// of the slice; its first / last segment are found once per block (uniform binary searches), a lane then only steps inside that range.
template <class R, bool DEV>
__global__ __launch_bounds__(256) void opt_flat_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, bf16_t* __restrict__ pb, long n, long base,
                                                              const long* __restrict__ seg_end, const int* __restrict__ seg_group, int nseg,
                                                              OptGroups<R> G, GradFactor<DEV> factor, const int* __restrict__ skip) {
  float gscale;
  if (!adam_begin<DEV>(factor, skip, gscale)) return;
  const AdamImage im = {pb, 0, false};
  const long c0 = (long)blockIdx.x * OPT_CHUNK, c1 = c0 + OPT_CHUNK < n ? c0 + OPT_CHUNK : n;
  auto seg_of = [&](long pos) {   // smallest s with seg_end[s] > pos (positions beyond the last end: the last segment)
    int lo = 0, hi = nseg - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg_end[mid] > pos) hi = mid; else lo = mid + 1; }
    return lo;
  };
  const int s0 = seg_of(base + c0), s1 = seg_of(base + c1 - 1);
  if (s0 == s1) {                 // the common case: one group for the whole chunk
    adam_span<R, DEV>(p, g, m, v, im, c0, c1, G.h[seg_group[s0] & (MUSE_ADAMW_MAX_GROUPS - 1)], gscale);
    return;
  }
  for (long k = c0 + threadIdx.x; k < c1; k += 256) {   // a chunk with a segment boundary inside: element-wise, group per element
    int s = s0;
    while (s < s1 && seg_end[s] <= base + k) ++s;
    adam_one<R, DEV>(p, g, m, v, im, k, G.h[seg_group[s] & (MUSE_ADAMW_MAX_GROUPS - 1)], gscale);
  }
}

// Multi-tensor form over either table layout: ncol == 6 -> group 0 and a plain bf16 copy, ncol == 7 -> column 6 names both.
template <class R, bool DEV>
__global__ __launch_bounds__(256) void opt_multi_kernel(const long* __restrict__ table, int ncol, const int* __restrict__ chunk_first, int nt,
                                                        OptGroups<R> G, GradFactor<DEV> factor, const int* __restrict__ skip) {
  float gscale;
  if (!adam_begin<DEV>(factor, skip, gscale)) return;
  const int t = tensor_of_chunk(chunk_first, 0, nt, (int)blockIdx.x);
  const long* e = table + (long)t * ncol;
  const long col6 = ncol > 6 ? e[6] : 0, plo = col6 >> 8;
  const AdamImage im = {(bf16_t*)e[4], plo < 0 ? 0 : plo, plo < 0};
  const long n = e[5], lo = (long)((int)blockIdx.x - chunk_first[t]) * OPT_CHUNK;
  adam_span<R, DEV>((float*)e[0], (const float*)e[1], (float*)e[2], (float*)e[3], im, lo, lo + OPT_CHUNK < n ? lo + OPT_CHUNK : n,
                 G.h[(int)col6 & (MUSE_ADAMW_MAX_GROUPS - 1)], gscale);
}

// Exponential moving average of the weights (reference muse/modeling_ema.py:118-137, called right behind the optimizer step,
// training/train_muse.py:779-780): shadow -= (1 - decay) * (shadow - param) over EVERY tracked tensor in one launch - the reference
// issues three elementwise kernels per tensor.  Table: 4 x int64 per tensor {shadow, param, n, mode}; mode 0 = the update, mode 1 =
// plain copy (a parameter with requires_grad == False, :134-135).  chunk_first as in opt_multi_kernel.  The three roundings of the
// reference's expression (subtract, multiply, subtract - each an f32 tensor op there) are kept: no contraction into an fma.
__device__ __forceinline__ float ema_update1(float s, float p, float omd) {
#pragma clang fp contract(off)
  const float t = s - p;
  const float u = omd * t;
  return s - u;
}
__global__ __launch_bounds__(256) void ema_multi_kernel(const long* __restrict__ table, const int* __restrict__ chunk_first, int nt, float omd) {
  const int t = tensor_of_chunk(chunk_first, 0, nt, (int)blockIdx.x);
  const long* e = table + (long)t * 4;
  float* s = (float*)e[0]; const float* p = (const float*)e[1];
  const long n = e[2], base = (long)((int)blockIdx.x - chunk_first[t]) * OPT_CHUNK;
  const bool copy = e[3] != 0;
  const long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
  const bool vec = !((((uintptr_t)s) | ((uintptr_t)p)) & 15);
  if (vec) {
    for (long i = base + threadIdx.x * 4; i + 3 < end; i += 1024) {
      float ss[4], pp[4];
      V4<float>::load(s + i, ss); V4<float>::load(p + i, pp);
#pragma unroll
      for (int j = 0; j < 4; ++j) ss[j] = copy ? pp[j] : ema_update1(ss[j], pp[j], omd);
      V4<float>::store(s + i, ss);
    }
  }
  const long s0 = vec ? base + ((end - base) & ~3L) : base;
  for (long i = s0 + threadIdx.x; i < end; i += 256) s[i] = copy ? p[i] : ema_update1(s[i], p[i], omd);
}

// ---- launches, once per rule: scale_dev != NULL selects the *_dev instantiation (the factor is read on the device and takes grad_scale's place)
// One row of a rule's group table (HOST memory): AdamW 5 x float {lr, beta1, beta2, eps, weight_decay}, taken at step `step`; Lion 4 x double
// {lr, beta1, beta2, weight_decay}.
static AdamHyper hyper_row(AdamRule, const float* rows, int k, int step) {
  const float* r = rows + k * 5;
  return adam_hyper(r[0], r[1], r[2], r[3], r[4], step);
}
static LionHyper hyper_row(LionRule, const double* rows, int k, int) {
  return lion_hyper(rows + k * 4);
}
template <class R> static int fill_groups(OptGroups<R>& G, const typename R::HostScalar* hyper, int ngroups, int step) {
  if (ngroups < 1 || ngroups > MUSE_ADAMW_MAX_GROUPS || !hyper) return MUSE_ERR_BAD_ARG;
  for (int k = 0; k < ngroups; ++k) G.h[k] = hyper_row(R(), hyper, k, step);
  for (int k = ngroups; k < MUSE_ADAMW_MAX_GROUPS; ++k) G.h[k] = G.h[0];
  return 0;
}
// the flat forms' pointer check (a rule without a second moment takes any v, NULL included)
template <class R> static bool flat_misaligned(const float* p, const float* g, const float* m, const float* v) {
  return ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | (R::HAS_V ? (uintptr_t)v : 0)) & 15) != 0;
}
template <class R>
static int opt_flat_launch(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const typename R::Hyper& h, float grad_scale,
                           const float* scale_dev, const int32_t* skip, void* stream) {
  if (n <= 0) return 0;
  if (flat_misaligned<R>(p, g, m, v)) return MUSE_ERR_ALIGN;
  if (p_bf16 && (((uintptr_t)p_bf16) & 7)) return MUSE_ERR_ALIGN;
  const dim3 grid(ew_grid((n + 3) / 4));
  if (scale_dev)
    hipLaunchKernelGGL((opt_flat_kernel<R, true>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, (long)n, h, scale_dev, skip);
  else
    hipLaunchKernelGGL((opt_flat_kernel<R, false>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, (long)n, h, grad_scale, skip);
  return (int)hipGetLastError();
}
template <class R>
static int opt_flat_groups_launch(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base, const int64_t* seg_end,
                                  const int32_t* seg_group, int32_t nseg, const typename R::HostScalar* group_hyper, int32_t ngroups, int32_t step,
                                  float grad_scale, const float* scale_dev, const int32_t* skip, void* stream) {
  if (n <= 0) return 0;
  if (nseg < 1 || !seg_end || !seg_group) return MUSE_ERR_BAD_ARG;
  if (flat_misaligned<R>(p, g, m, v)) return MUSE_ERR_ALIGN;
  if (p_bf16 && (((uintptr_t)p_bf16) & 7)) return MUSE_ERR_ALIGN;
  OptGroups<R> G;
  const int rc = fill_groups<R>(G, group_hyper, ngroups, step);
  if (rc) return rc;
  const dim3 grid((unsigned)((n + OPT_CHUNK - 1) / OPT_CHUNK));
  if (scale_dev)
    hipLaunchKernelGGL((opt_flat_groups_kernel<R, true>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, (long)n, (long)base,
                       (const long*)seg_end, seg_group, nseg, G, scale_dev, skip);
  else
    hipLaunchKernelGGL((opt_flat_groups_kernel<R, false>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, (long)n, (long)base,
                       (const long*)seg_end, seg_group, nseg, G, grad_scale, skip);
  return (int)hipGetLastError();
}
template <class R>
static int opt_multi_launch(const int64_t* table, int ncol, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                            const typename R::HostScalar* group_hyper, int32_t ngroups, int32_t step, float grad_scale, const float* scale_dev,
                            const int32_t* skip, void* stream) {
  if (num_tensors <= 0 || num_chunks <= 0) return 0;
  OptGroups<R> G;
  const int rc = fill_groups<R>(G, group_hyper, ngroups, step);
  if (rc) return rc;
  if (scale_dev)
    hipLaunchKernelGGL((opt_multi_kernel<R, true>), dim3(num_chunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, ncol, chunk_first,
                       num_tensors, G, scale_dev, skip);
  else
    hipLaunchKernelGGL((opt_multi_kernel<R, false>), dim3(num_chunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, ncol, chunk_first,
                       num_tensors, G, grad_scale, skip);
  return (int)hipGetLastError();
}

// ---- entry points (include/muse_hip.h) ------------------------------------------------------------------------------------------------------
extern "C" int muse_adamw_flat(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* skip, void* stream) {
  return opt_flat_launch<AdamRule>(p, g, m, v, p_bf16, n, adam_hyper(lr, beta1, beta2, eps, weight_decay, step), grad_scale, nullptr, skip, stream);
}
extern "C" int muse_adamw_flat_dev(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int32_t step, const float* scale_dev, const int32_t* skip,
                                   void* stream) {
  return scale_dev ? opt_flat_launch<AdamRule>(p, g, m, v, p_bf16, n, adam_hyper(lr, beta1, beta2, eps, weight_decay, step), 0.f, scale_dev, skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_adamw_flat_groups(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                                      const int64_t* seg_end, const int32_t* seg_group, int32_t nseg, const float* group_hyper,
                                      int32_t ngroups, int32_t step, float grad_scale, const int32_t* skip, void* stream) {
  return opt_flat_groups_launch<AdamRule>(p, g, m, v, p_bf16, n, base, seg_end, seg_group, nseg, group_hyper, ngroups, step, grad_scale, nullptr, skip,
                                          stream);
}
extern "C" int muse_adamw_flat_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                                          const int64_t* seg_end, const int32_t* seg_group, int32_t nseg, const float* group_hyper,
                                          int32_t ngroups, int32_t step, const float* scale_dev, const int32_t* skip, void* stream) {
  return scale_dev ? opt_flat_groups_launch<AdamRule>(p, g, m, v, p_bf16, n, base, seg_end, seg_group, nseg, group_hyper, ngroups, step, 0.f, scale_dev,
                                                      skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_adamw_multi(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* skip, void* stream) {
  const float one_group[5] = {lr, beta1, beta2, eps, weight_decay};
  return opt_multi_launch<AdamRule>(table, 6, chunk_first, num_tensors, num_chunks, one_group, 1, step, grad_scale, nullptr, skip, stream);
}
extern "C" int muse_adamw_multi_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* scale_dev,
                                    const int32_t* skip, void* stream) {
  const float one_group[5] = {lr, beta1, beta2, eps, weight_decay};
  return scale_dev ? opt_multi_launch<AdamRule>(table, 6, chunk_first, num_tensors, num_chunks, one_group, 1, step, 0.f, scale_dev, skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_adamw_multi_groups(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                       const float* group_hyper, int32_t ngroups, int32_t step, float grad_scale, const int32_t* skip,
                                       void* stream) {
  return opt_multi_launch<AdamRule>(table, 7, chunk_first, num_tensors, num_chunks, group_hyper, ngroups, step, grad_scale, nullptr, skip, stream);
}
extern "C" int muse_adamw_multi_groups_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                           const float* group_hyper, int32_t ngroups, int32_t step, const float* scale_dev,
                                           const int32_t* skip, void* stream) {
  return scale_dev ? opt_multi_launch<AdamRule>(table, 7, chunk_first, num_tensors, num_chunks, group_hyper, ngroups, step, 0.f, scale_dev, skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
// Lion: the same eight with double hyper-parameters (`hyper`: ONE host row, `group_hyper`: ngroups of them), no eps, no step and no v
extern "C" int muse_lion_flat(float* p, const float* g, float* m, void* p_bf16, int64_t n, const double* hyper, float grad_scale,
                              const int32_t* skip, void* stream) {
  return hyper ? opt_flat_launch<LionRule>(p, g, m, nullptr, p_bf16, n, lion_hyper(hyper), grad_scale, nullptr, skip, stream) : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_lion_flat_dev(float* p, const float* g, float* m, void* p_bf16, int64_t n, const double* hyper, const float* scale_dev,
                                  const int32_t* skip, void* stream) {
  return scale_dev && hyper ? opt_flat_launch<LionRule>(p, g, m, nullptr, p_bf16, n, lion_hyper(hyper), 0.f, scale_dev, skip, stream)
                            : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_lion_flat_groups(float* p, const float* g, float* m, void* p_bf16, int64_t n, int64_t base, const int64_t* seg_end,
                                     const int32_t* seg_group, int32_t nseg, const double* group_hyper, int32_t ngroups, float grad_scale,
                                     const int32_t* skip, void* stream) {
  return opt_flat_groups_launch<LionRule>(p, g, m, nullptr, p_bf16, n, base, seg_end, seg_group, nseg, group_hyper, ngroups, 0, grad_scale, nullptr, skip,
                                          stream);
}
extern "C" int muse_lion_flat_groups_dev(float* p, const float* g, float* m, void* p_bf16, int64_t n, int64_t base, const int64_t* seg_end,
                                         const int32_t* seg_group, int32_t nseg, const double* group_hyper, int32_t ngroups,
                                         const float* scale_dev, const int32_t* skip, void* stream) {
  return scale_dev ? opt_flat_groups_launch<LionRule>(p, g, m, nullptr, p_bf16, n, base, seg_end, seg_group, nseg, group_hyper, ngroups, 0, 0.f, scale_dev,
                                                      skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_lion_multi(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, const double* hyper,
                               float grad_scale, const int32_t* skip, void* stream) {
  return opt_multi_launch<LionRule>(table, 6, chunk_first, num_tensors, num_chunks, hyper, 1, 0, grad_scale, nullptr, skip, stream);
}
extern "C" int muse_lion_multi_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks, const double* hyper,
                                   const float* scale_dev, const int32_t* skip, void* stream) {
  return scale_dev ? opt_multi_launch<LionRule>(table, 6, chunk_first, num_tensors, num_chunks, hyper, 1, 0, 0.f, scale_dev, skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_lion_multi_groups(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                      const double* group_hyper, int32_t ngroups, float grad_scale, const int32_t* skip, void* stream) {
  return opt_multi_launch<LionRule>(table, 7, chunk_first, num_tensors, num_chunks, group_hyper, ngroups, 0, grad_scale, nullptr, skip, stream);
}
extern "C" int muse_lion_multi_groups_dev(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                                          const double* group_hyper, int32_t ngroups, const float* scale_dev, const int32_t* skip,
                                          void* stream) {
  return scale_dev ? opt_multi_launch<LionRule>(table, 7, chunk_first, num_tensors, num_chunks, group_hyper, ngroups, 0, 0.f, scale_dev, skip, stream)
                   : MUSE_ERR_BAD_ARG;
}
extern "C" int muse_ema_multi(const int64_t* table, const int32_t* chunk_first, int32_t num_tensors, int32_t num_chunks,
                              float one_minus_decay, void* stream) {
  if (num_tensors <= 0 || num_chunks <= 0) return 0;
  if (!table || !chunk_first) return MUSE_ERR_BAD_ARG;
  hipLaunchKernelGGL(ema_multi_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, chunk_first, num_tensors,
                     one_minus_decay);
  return (int)hipGetLastError();
}
