"""CPU side of the spatial / layout / VQ edge tests (tests/test_gpu_spatial_edges.py, tests/test_spatial_cpu.py): float64 references written
as index arithmetic, the probes, the storage builders, the checks, the derived rounding bounds, and a small model of each kernel route's
read / write contract with switchable defects (DEFECTS).  The guards, the sentinel pattern and the contiguous checks are conv_cpu's.

Probes.  coordinate: every element holds a seeded id its type carries exactly (conv_cpu.coord_ids), so an output of a data-movement kernel,
or of a depthwise convolution with one-hot taps, is ONE named input element (or +0).  dense: small integers with every partial sum below
2^24 - the f32 (or f64) result does not depend on the summation order.  pick: dy is one-hot per (64-pixel chunk, channel), so a dw partial
slot is one element of x.

Read contract: every kernel here masks what lies outside the image (a tap) or the tensor (a tail) by not loading it.  `place` /
`place_shifted` / `place_ld` put NaN in front of an operand, behind it and into every ld > cols gap: a stray read makes an output NaN, a
tap taken from the neighbouring row or image is a wrong id.  Write contract: `alloc_out` pre-fills outputs and partial buffers with a NaN
bit pattern no result has, guard bands included; `check_out` / `check_index` want the guards (and gaps) back bit for bit and every slot
written.
"""
import math

import torch

from conv_cpu import GUARD, LEAD, SENTINEL, alloc_out, check_out, check_same_bits, place  # noqa: F401  (re-exported to the tests)
from conv_cpu import F64, U32, UBF, bound_act, coord_ids, exact_in, sentinel, silu64
from gemm_cpu import BF, F32, bits, ints

NAN = float("nan")
TINY = 1e-30
DW_PIX = 64               # csrc/uvit.hip DW_PIX: pixels per dw partial chunk
GN_PIX = 1024             # csrc/vqgan.hip GN_PIX_PER_CHUNK


def gen(seed):
    return torch.Generator().manual_seed(seed & 0x7FFFFFFF)


def randn(shape, seed, shift=0.0):
    """seeded N(0, 1) (+ shift), rounded to f32: what the kernel is given"""
    return (torch.randn(shape, generator=gen(seed), dtype=F64) + shift).float()


# ---- storage ---------------------------------------------------------------------------------------------------------------------------
def place_shifted(t, dtype, shift):
    """`place` with the operand `shift` elements further in: shift = 1 puts an f32 operand 4 bytes off its 16-byte alignment (the scalar
    routes).  The operand starts at element LEAD + shift."""
    body = torch.cat([torch.full((shift,), NAN, dtype=dtype), exact_in(t, dtype).flatten()])
    return place(body, dtype, exact=False)


def place_ld(t, dtype, ld):
    """[rows, cols] stored with row stride ld >= cols, NaN in the gap"""
    rows, cols = t.shape
    body = torch.full((rows, ld), NAN, dtype=dtype)
    body[:, :cols] = t.to(dtype)                             # (the argmin rows carry NaN themselves: compared with the NaN mapped away)
    assert torch.equal(body[:, :cols].double().nan_to_num(nan=0.5), t.double().nan_to_num(nan=0.5)), f"values are not exact in {dtype}"
    return place(body, dtype, exact=False)


def ld_index(rows, cols, ld, batch=1, stride=0):
    """flat positions of a [batch, rows, cols] result with row stride ld and batch stride `stride`"""
    i = (torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).flatten()
    return (torch.arange(batch)[:, None] * stride + i[None, :]).flatten()


def check_index(st, index, expected, what, guard=GUARD, exact=True, bound=None):
    """the strided form of conv_cpu.check_out: `index` are the result slots' positions behind the output pointer (storage element guard +
    index), in `expected`'s order.  Every OTHER element of the storage - guards and ld gaps - keeps its sentinel bit for bit; every slot is
    written, no NaN, and the values are exact (or within `bound`)."""
    s = bits(sentinel(1, st.dtype))[0]
    b = bits(st)
    slot = torch.zeros(st.numel(), dtype=torch.bool)
    slot[guard + index] = True
    stray = ~slot & (b != s)
    assert not bool(stray.any()), f"{what}: {int(stray.sum())} elements outside the result were written (guard or ld gap), first {int(stray.nonzero()[0]) - guard}"
    unwritten = slot & (b == s)
    assert not bool(unwritten.any()), f"{what}: {int(unwritten.sum())} result slots were never written, first {int(unwritten.nonzero()[0]) - guard}"
    got, exp = st[guard + index].double(), expected.double().flatten()
    assert not bool(got.isnan().any()), f"{what}: {int(got.isnan().sum())} NaN results (a read outside the operands)"
    if exact:
        bad = got != exp
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {got.numel()} elements differ from the exact reference, first at "
                                     f"{int(bad.nonzero()[0])}: got {float(got[bad][0])}, expected {float(exp[bad][0])}")
    else:
        err = (got - exp).abs() / bound.double().flatten()
        assert float(err.max()) <= 1.0, f"{what}: error {float(err.max()):.3f} x its bound at {int(err.argmax())}"
    return st[guard + index]


def check_zero_sign(body, expected, what):
    """zero padding is +0: where the reference is 0 the result's bits are all clear"""
    z = expected.flatten() == 0
    assert not bool((bits(body.flatten())[z] != 0).any()), f"{what}: a zero that is not +0"


def check_untouched(st, what):
    """a refused call launches nothing: the whole storage still holds its sentinel"""
    assert bool((bits(st) == bits(sentinel(1, st.dtype))[0]).all()), f"{what}: the refused call wrote to its output"


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; a NaN or infinite difference is inf, never a pass"""
    d = (got.double().flatten() - ref.double().flatten()).abs()
    r = torch.where(d > 0, d / bound.double().flatten().clamp(min=1e-300), torch.zeros_like(d))
    r = torch.where(torch.isfinite(d), r, torch.full_like(d, math.inf))
    return float(r.max()) if r.numel() else 0.0


def measure(got, ref, scale):
    """E_ref's figure: max |got - ref| / scale, scale = the sum of the absolute terms the element sums"""
    return float(((got.double() - ref.double()).abs() / scale.double().clamp(min=TINY)).max())


# ---- pure data movement ----------------------------------------------------------------------------------------------------------------
def ref_space_to_depth(x, inverse=False, defect=None):
    """full [B, H, W, C] <-> packed [B, H/2, W/2, (di, dj, c)]   (csrc/uvit.hip space_depth2_kernel)"""
    order = (0, 1, 3, 4, 2, 5) if defect == "didj_swapped" else (0, 1, 3, 2, 4, 5)
    if not inverse:
        B, H, W, C = x.shape
        return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(*order).reshape(B, H // 2, W // 2, 4 * C)
    B, h, w, C4 = x.shape
    v = x.reshape(B, h, w, 2, 2, C4 // 4)
    if defect == "didj_swapped":
        v = v.transpose(3, 4)
    return v.permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, C4 // 4)


def ref_upsample2x(x):
    """nearest x2 of [B, H, W, C]: out[b, y, x] = in[b, y // 2, x // 2]"""
    B, H, W, C = x.shape
    return x[:, torch.arange(2 * H) // 2][:, :, torch.arange(2 * W) // 2]


def ref_nchw_to_nhwc(x, Cpad):
    """[B, C, HW] -> [B, HW, Cpad], channels C .. Cpad - 1 are +0"""
    B, C, HW = x.shape
    out = torch.zeros(B, HW, Cpad, dtype=x.dtype)
    out[:, :, :C] = x.transpose(1, 2)
    return out


def model_nchw_to_nhwc(x, Cpad, out_dtype, defect=None):
    """the output storage a kernel leaves; "pad_not_zeroed": the loop runs over c < C only"""
    B, C, HW = x.shape
    n = B * HW * Cpad
    st = alloc_out(n, out_dtype)
    body = st[GUARD:GUARD + n].view(B, HW, Cpad)
    body[:, :, :C] = x.transpose(1, 2).to(out_dtype)
    if defect != "pad_not_zeroed":
        body[:, :, C:] = 0.0
    return st


def ref_nhwc_to_nchw(x, C):
    """[B, HW, Cpad] -> [B, C, HW], the padding channels are never read"""
    return x[:, :, :C].transpose(1, 2).contiguous()


def to_bf16(t, defect=None):
    """round to nearest even (the cast every kernel here makes); "bf16_trunc": the low 16 bits dropped"""
    if defect == "bf16_trunc":
        return (t.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF)
    return t.float().to(BF)


def ref_split(x, defect=None):
    """(hi, lo) operand planes: bf16(x), bf16(x - hi)   (csrc/common.h split4)"""
    hi = to_bf16(x, defect)
    return hi, to_bf16(x.float() - hi.float(), defect)


# ---- depthwise 3 x 3 -------------------------------------------------------------------------------------------------------------------
def shifted(x, dy, dx):
    """out[b, y, x] = in[b, y + dy, x + dx], 0 outside the image"""
    B, H, W, C = x.shape
    out = torch.zeros_like(x)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def ref_dwconv(x, w):
    """x [B, H, W, C], w [C, 3, 3]: y = sum_t x[p + tap t] w[t], padding 1, float64"""
    x, w = x.double(), w.double()
    return sum(shifted(x, ky - 1, kx - 1) * w[:, ky, kx] for ky in range(3) for kx in range(3))


def ref_dwconv_dx(dy, w):
    """dx[p] = sum_t dy[p - tap t] w[t]"""
    dy, w = dy.double(), w.double()
    return sum(shifted(dy, 1 - ky, 1 - kx) * w[:, ky, kx] for ky in range(3) for kx in range(3))


def dw_nchunk(pixels):
    return (pixels + DW_PIX - 1) // DW_PIX


def ref_dwconv_dw(dy, x, terms=False):
    """partials [nchunk, C, 9]: slot (k, c, t) = sum over the pixels p of chunk k (64 consecutive pixels of the flat [B * H * W] order,
    across image boundaries) of dy[p, c] x[p + tap t, c].  terms: the sum of |products| instead (the rounding bound's S)"""
    B, H, W, C = x.shape
    dy, x = dy.double(), x.double()
    pr = torch.stack([dy * shifted(x, ky - 1, kx - 1) for ky in range(3) for kx in range(3)], -1).view(B * H * W, C, 9)
    if terms:
        pr = pr.abs()
    nch = dw_nchunk(B * H * W)
    pad = torch.zeros(nch * DW_PIX - B * H * W, C, 9, dtype=F64)
    return torch.cat([pr, pad]).view(nch, DW_PIX, C, 9).sum(1)


def onehot_taps(C, seed):
    """w [C, 3, 3] with a single 1 per channel at tap (c + seed) % 9"""
    w = torch.zeros(C, 9)
    w[torch.arange(C), (torch.arange(C) + seed) % 9] = 1.0
    return w.view(C, 3, 3)


def pick_dy(B, H, W, C, seed):
    """dy one-hot per (chunk, channel): in every 64-pixel chunk each channel has ONE pixel with dy = 1 (seeded), so a dw partial slot is one
    element of x (or 0 past the border)"""
    pixels = B * H * W
    dy = torch.zeros(pixels, C)
    for k in range(dw_nchunk(pixels)):
        n = min(DW_PIX, pixels - k * DW_PIX)
        p = k * DW_PIX + torch.randint(0, n, (C,), generator=gen(seed + k))
        dy[p, torch.arange(C)] = 1.0
    return dy.view(B, H, W, C)


def dwconv_case(probe, B, H, W, C, seed):
    """a (the forward's input / the backward's saved x), g (the backward's dy), w - and what each output must be.  exact: which of
    (y, dx, dw) the probe determines exactly."""
    if probe == "coord":        # y and dx are one element each; dw sums 64 products of ids and is not exact
        a, g, w = coord_ids((B, H, W, C), "f32", seed).float(), coord_ids((B, H, W, C), "f32", seed + 1).float(), onehot_taps(C, seed)
        exact = dict(y=True, dx=True, dw=False)
    elif probe == "pick":
        a, g, w = coord_ids((B, H, W, C), "f32", seed).float(), pick_dy(B, H, W, C, seed), onehot_taps(C, seed + 4)
        exact = dict(y=True, dx=True, dw=True)
    elif probe == "dense":      # 9 * 7 * 1023 and 64 * 7 * 1023 < 2^24
        a, g, w = ints((B, H, W, C), 1023, seed).float(), ints((B, H, W, C), 7, seed + 1).float(), ints((C, 3, 3), 7, seed + 2).float()
        exact = dict(y=True, dx=True, dw=True)
    else:
        assert probe == "randn"
        a, g, w = randn((B, H, W, C), seed), randn((B, H, W, C), seed + 1), randn((C, 3, 3), seed + 2)
        exact = dict(y=False, dx=False, dw=False)
    if probe != "randn":
        assert float(ref_dwconv(a.abs(), w.abs()).max()) < 2 ** 24 and float(ref_dwconv_dx(g.abs(), w.abs()).max()) < 2 ** 24
        assert not exact["dw"] or float(ref_dwconv_dw(g, a, terms=True).max()) < 2 ** 24
    return dict(probe=probe, B=B, H=H, W=W, C=C, a=a, g=g, w=w, exact=exact, y=ref_dwconv(a, w), dx=ref_dwconv_dx(g, w), dw=ref_dwconv_dw(g, a))


def model_dwconv(x_st, w, B, H, W, C, flip=False, defect=None, lead=LEAD):
    """the output storage of a kernel that addresses the way dwconv3x3_v4_kernel does: row = b * H + y over ALL images, a tap reads flat
    pixel (row + ky - 1) * W + x + kx - 1 of the operand at x_st[lead], masked by the row WITHIN the image and the column - so a wrong
    mask reads the neighbouring row / image (a wrong id) or the NaN around the operand.  flip: the backward's dx (taps 8 - t).
    defects: "tap_flip", "border_off_by_one" (x + kx - 1 <= W passes), "image_boundary" (the row mask tests b * H + y against B * H)"""
    rows = B * H
    r, xx, c = torch.arange(rows).view(rows, 1, 1), torch.arange(W).view(1, W, 1), torch.arange(C).view(1, 1, C)
    yy = r % H
    X = x_st.double()
    out = torch.zeros(rows, W, C, dtype=F64)
    wf = w.double().view(C, 9)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            ts = 8 - t if flip != (defect == "tap_flip") else t
            iy, ix = yy + ky - 1, xx + kx - 1
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            if defect == "border_off_by_one":
                ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix <= W)
            if defect == "image_boundary":
                ok = (r + ky - 1 >= 0) & (r + ky - 1 < rows) & (ix >= 0) & (ix < W)
            src = lead + ((r + ky - 1) * W + ix) * C + c
            v = X[src.clamp(0, X.numel() - 1)]
            out += torch.where(ok.expand_as(v), v * wf[:, ts].view(1, 1, C), torch.zeros_like(v))
    st = alloc_out(out.numel(), F32)
    st[GUARD:GUARD + out.numel()] = out.flatten().float()
    return st


def model_dwconv_dw(dy, x, defect=None):
    """the partial storage of dwconv3x3_bwd_dw*_kernel: wave wv of the block of chunk k takes pixels p0 + wv, p0 + wv + 4, ... < p1 and the
    four waves' sums are folded.  defects: "chunk_last_pixel" (p < p1 - 1), "wave_skipped" (the fold leaves wave 3 out)"""
    B, H, W, C = x.shape
    pixels = B * H * W
    p = torch.arange(pixels)
    keep = torch.ones(pixels, dtype=torch.bool)
    if defect == "chunk_last_pixel":
        keep &= ~((p % DW_PIX == DW_PIX - 1) | (p == pixels - 1))
    if defect == "wave_skipped":
        keep &= (p % DW_PIX) % 4 != 3
    pr = ref_dwconv_dw(dy.double() * keep.view(B, H, W, 1), x)
    st = alloc_out(pr.numel(), F32)
    st[GUARD:GUARD + pr.numel()] = pr.flatten().float()
    return st


def bound_dw(dy, x):
    """a partial slot sums <= 16 fma per wave and folds four waves: 18 roundings of partial sums <= S = sum |dy x|"""
    return 1.01 * 18 * U32 * ref_dwconv_dw(dy, x, terms=True) + TINY


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------
def ref_avgpool(x):
    """(((v00 + v01) + v10) + v11) * 0.25 in x's dtype - exact for the integer probe (multiples of 4)"""
    return (((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2]) * 0.25


def ref_gn_partials(x, groups, terms=False):
    """f64 [B, nchunk, groups, 2]: sum / sum of squares of x [B, HW, C] per 1024-pixel chunk and group (gn_stats_kernel, avgpool_stats_kernel).
    terms: the sums of |v| and v^2 (what the f64 rounding allowance is taken from)"""
    B, HW, C = x.shape
    nch = (HW + GN_PIX - 1) // GN_PIX
    v = torch.cat([x.double(), torch.zeros(B, nch * GN_PIX - HW, C, dtype=F64)], 1).view(B, nch, GN_PIX, groups, C // groups)
    return torch.stack([(v.abs() if terms else v).sum((2, 4)), (v * v).sum((2, 4))], -1)


# ---- argmin ----------------------------------------------------------------------------------------------------------------------------
def ref_argmin(d):
    """the contract of muse_argmin_rows on d [rows, n]: the lowest index of the smallest non-NaN value (-0.0 == +0.0); 0 for a row of NaN"""
    x = d.double()
    nan = x.isnan()
    m = torch.where(nan, torch.full_like(x, math.inf), x).amin(1, keepdim=True)
    cand = ~nan & (x == m)
    first = torch.where(cand, torch.arange(x.shape[1]).expand_as(x), torch.full(x.shape, x.shape[1])).amin(1)
    return torch.where(cand.any(1), first, torch.zeros_like(first))


def model_argmin(st, rows, n, ld, defect=None, lead=LEAD):
    """argmin_rows_kernel lane by lane: lane l scans columns l, l + 64, ... keeping the first smallest value (its first +inf too), then the
    lanes are folded, ties to the lower index.  defects: "tie_high" (the fold prefers the higher index), "lane_stride_tie" (a lane
    replaces on <=, so column c + 64 beats c)"""
    d = st[lead:lead + rows * ld].double().view(rows, ld)[:, :n]
    out = torch.zeros(rows, dtype=torch.int64)
    for r in range(rows):
        best = None                                        # (value, index)
        for lane in range(min(64, n)):
            lb = None
            for c in range(lane, n, 64):
                v = float(d[r, c])
                if v != v:
                    continue
                if lb is None or v < lb[0] or (defect == "lane_stride_tie" and v == lb[0]):
                    lb = (v, c)
            if lb is None:
                continue
            if best is None or lb[0] < best[0] or (lb[0] == best[0] and (lb[1] > best[1] if defect == "tie_high" else lb[1] < best[1])):
                best = lb
        out[r] = 0 if best is None else best[1]
    return out


def argmin_rows_case(n, rows, seed):
    """distance rows [rows, n] with every tie and special value the contract names, cycling with the row number.  Finite rows are small
    integers (many exact ties)"""
    g = gen(seed)
    d = torch.randint(1, 50, (rows, n), generator=g).float()
    for r in range(rows):
        kind = (r + seed) % 10
        lo = float(d[r].min()) - 1.0
        c = int(torch.randint(0, n, (1,), generator=g))
        if kind == 0:                                      # ties across lanes: the minimum three times
            d[r, torch.randint(0, n, (3,), generator=g)] = lo
        elif kind == 1 and n > 64:                         # inside one lane: columns c and c + 64 (and nowhere else)
            c = c % (n - 64)
            d[r, c] = d[r, c + 64] = lo
        elif kind == 2:                                    # -0.0 against +0.0 (the rest of the row is >= 1): equal, the lower index wins
            d[r, c], d[r, (c * 7 + 3) % n] = -0.0, 0.0
        elif kind == 3:
            d[r, 0] = lo                                   # the minimum in the first column
        elif kind == 4:
            d[r, n - 1] = lo                               # ... in the last
        elif kind == 5:
            d[r, c] = -math.inf
        elif kind == 6:
            d[r] = math.inf
        elif kind == 7:
            d[r] = NAN
        elif kind == 8:                                    # NaN in front of and between finite values
            d[r, torch.randint(0, n, (max(1, n // 3),), generator=g)] = NAN
            d[r, 0] = NAN if n > 1 else d[r, 0]
        elif kind == 9:                                    # NaN and +inf only: the first +inf
            d[r] = NAN
            d[r, torch.randint(0, n, (2,), generator=g)] = math.inf
    return d


# ---- GlobalResponseNorm ----------------------------------------------------------------------------------------------------------------
def ref_grn(x, gamma, beta, defect=None):
    """x [B, S, C] -> (y, G, N) float64: G = ||x[b, :, c]||, N = G / (mean_c G + 1e-6), y = gamma (x N) + beta + x.
    "grn_mean_c1": the mean divides by C + 1"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    C = x.shape[2]
    G = (x * x).sum(1).sqrt()
    N = G / (G.sum(1, keepdim=True) / (C + 1 if defect == "grn_mean_c1" else C) + 1e-6)
    return gamma * (x * N[:, None]) + beta + x, G, N


def bound_grn(x, gamma, beta):
    """grn_colnorm_kernel: each of four waves chains L = ceil(S / 4) fma (one rounding of a partial sum <= sum x^2 each), two levels of
    adds fold them: (L + 2) u relative on the sum, half of it on the root, which rounds once more (2 u allowed for sqrtf):
        eG = ((L + 2) / 2 + 2) u
    grn_scale_kernel: a lane adds ceil(C / 256) values, wave_sum 6 levels, 3 adds across the waves, / C, + 1e-6, then G / (.): the mean
    carries eG (every G does) and (ceil(C / 256) + 11) u, the quotient rounds once (2 u allowed):
        eN = 2 eG + (ceil(C / 256) + 13) u
    apply: gamma * (x * N) + beta + x is four roundings of values <= A = |gamma x N| + |beta| + |x|:
        |dy| <= |gamma x N| eN + 4 u A.       (first order; 1 % on top)"""
    _, S, C = x.shape
    y, G, N = ref_grn(x, gamma, beta)
    eG = ((math.ceil(S / 4) + 2) / 2 + 2) * U32
    eN = 2 * eG + (math.ceil(C / 256) + 13) * U32
    t = (gamma.double() * (x.double() * N[:, None])).abs()
    return dict(G=1.01 * eG * G + TINY, N=1.01 * eN * N + TINY, y=1.01 * (t * eN + 4 * U32 * (t + beta.double().abs() + x.double().abs())) + TINY)


def ref_grn_bwd(dy, x, gamma, G, N):
    """what muse_grn_bwd computes from the SAVED statistics G, N [B, C] (taken as given): S0 = sum_s dy, S1 = sum_s dy x, a = gamma S1,
    K = (a - mean_c(a N)) / (mean_c G + 1e-6) / G (0 where G = 0), dx = dy (gamma N + 1) + x K; the per-image dgamma / dbeta terms are
    N S1 and S0.  float64"""
    dy, x, gamma, G, N = dy.double(), x.double(), gamma.double(), G.double(), N.double()
    S0, S1 = dy.sum(1), (dy * x).sum(1)
    a = gamma * S1
    man = (a * N).mean(1, keepdim=True)
    den = G.mean(1, keepdim=True) + 1e-6
    K = torch.where(G > 0, (a - man) / den / G.clamp(min=TINY), torch.zeros_like(G))
    return dict(S0=S0, NS1=N * S1, K=K, dx=dy * (gamma * N + 1.0)[:, None] + x * K[:, None])


def bound_grn_bwd(dy, x, gamma, G, N):
    """grn_bwd_reduce_kernel sums like grn_colnorm_kernel: eS = (L + 2) u of T0 = sum |dy| and T1 = sum |dy x|.
    grn_bwd_coef_kernel: a = gamma * s1 rounds once: da = |gamma| eS T1 + u |a|.  mean_c(a N) chains ceil(C / 256) fma per lane, 6 + 3 adds
    and a division: dm = mean_c(N da) + (ceil(C / 256) + 10) u mean_c |a N|.  The denominator is relative (ceil(C / 256) + 11) u = eD.
    K = ((a - m) / den) / G: three roundings of a value <= (|a| + |m|) / (den G):
        dK = (da + dm + (|a| + |m|) (eD + 3 u)) / (den G)
    N S1 rounds once: |N| eS T1 + u |N S1|.   dx = dy (gamma N + 1) + x K: four roundings of values <= |dy| (|gamma N| + 1) + |x K|, and x dK."""
    _, S, C = x.shape
    dy, x, gamma, G, N = dy.double(), x.double(), gamma.double(), G.double(), N.double()
    r = ref_grn_bwd(dy, x, gamma, G, N)
    eS = (math.ceil(S / 4) + 2) * U32
    cq = math.ceil(C / 256)
    T0, T1 = dy.abs().sum(1), (dy * x).abs().sum(1)
    a = gamma * (dy * x).sum(1)
    da = gamma.abs() * eS * T1 + U32 * a.abs()
    man = (a * N).mean(1, keepdim=True)
    dm = (N * da).mean(1, keepdim=True) + (cq + 10) * U32 * (a * N).abs().mean(1, keepdim=True)
    den = G.mean(1, keepdim=True) + 1e-6
    dK = torch.where(G > 0, (da + dm + (a.abs() + man.abs()) * (cq + 14) * U32) / (den * G.clamp(min=TINY)), torch.zeros_like(G))
    ddx = x.abs() * dK[:, None] + 4 * U32 * (dy.abs() * ((gamma * N).abs() + 1.0)[:, None] + (x * r["K"][:, None]).abs())
    return dict(S0=1.01 * eS * T0 + TINY, NS1=1.01 * (N.abs() * eS * T1 + U32 * r["NS1"].abs()) + TINY, K=1.01 * dK + TINY, dx=1.01 * ddx + TINY)


# ---- GroupNorm (+ SiLU) ----------------------------------------------------------------------------------------------------------------
def ref_groupnorm(x, gamma, beta, groups, eps, silu):
    """x [B, HW, C] -> (y, t, scale) float64: t = (x - mean) rstd gamma + beta per (image, group), y = silu(t) or t; scale = |x sc| + |sh|
    with sc = rstd gamma, sh = beta - sc mean: the two terms gn_apply_kernel's fma adds (what E_ref is normalised by)"""
    B, HW, C = x.shape
    v = x.double().view(B, HW, groups, C // groups)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v * v).mean((1, 3), keepdim=True) - mean * mean).clamp(min=0.0)
    rstd = 1.0 / (var + eps).sqrt()
    sc = (rstd * gamma.double().view(1, 1, groups, -1))
    sh = beta.double().view(1, 1, groups, -1) - sc * mean
    t = (v * sc + sh).view(B, HW, C)
    scale = ((v * sc).abs() + sh.abs()).view(B, HW, C)
    return (silu64(t) if silu else t), t, scale


def gn_stats(x, groups, eps):
    """float64 (v, mean, var, rstd) of x [B, HW, C] per (image, group): v [B, HW, groups, cpg], the statistics [B, 1, groups, 1]"""
    B, HW, C = x.shape
    v = x.double().view(B, HW, groups, C // groups)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v * v).mean((1, 3), keepdim=True) - mean * mean).clamp(min=0.0)
    return v, mean, var, 1.0 / (var + eps).sqrt()


def model_groupnorm(x, gamma, beta, groups, eps, defect=None):
    """t as gn_apply_kernel forms it (no SiLU), in float64 rounded to f32 where the kernel rounds: statistics in f64, gmean = f32(mean),
    grstd = f32(rstd), sc = f32(grstd gamma), sh = f32(beta - sc gmean), t = f32(fma(x, sc, sh)).  (A product of two f32 is exact in f64, so
    f32(f64 expression) is the fused operation up to a double rounding.)
    defects: "gn_eps_x10" (eps ten times too large), "gn_f32_stats" (mean and E[x^2] - mean^2 in float32)"""
    B, HW, C = x.shape
    v, mean, var, rstd = gn_stats(x, groups, eps * (10.0 if defect == "gn_eps_x10" else 1.0))
    if defect == "gn_f32_stats":
        vf = v.float()
        mean = vf.mean((1, 3), keepdim=True)
        rstd = (1.0 / (((vf * vf).mean((1, 3), keepdim=True) - mean * mean).clamp(min=0.0) + eps).sqrt()).double()
        mean = mean.double()
    f = lambda a: a.float().double()
    sc = f(f(rstd) * gamma.double().view(1, 1, groups, -1))
    sh = f(beta.double().view(1, 1, groups, -1) - sc * f(mean))
    return f(v * sc + sh).view(B, HW, C).float()


def bound_groupnorm(x, gamma, beta, groups, eps, silu, bf16, fused=True):
    """Derived from what the kernels do (csrc/vqgan.hip gn_stats_kernel, gn_apply_kernel), first order, 1 % on top; u = 2^-24.
    Statistics: sums and sums of squares in f64, at most L = pixels * cpg additions per chunk slot (one LDS atomicAdd each on the wide
    route) and nchunk to fold: relative e64 = (L + nchunk + 4) 2^-53 of mean |v| and mean v^2, so
        dmean <= e64 mean|v|,   dvar <= e64 mean v^2 + 2 |mean| dmean,   er = dvar / (2 (var + eps)) + 4 * 2^-53   (relative, of rstd)
    Apply: gmean = f32(mean) and grstd = f32(rstd) round once each, sc = grstd * gamma once more, sh = beta - sc * gmean rounds the
    product (unless contracted) and the difference, t = fmaf(x, sc, sh) once.  sc's relative error d, |d| <= 2 u + er, is common to x sc
    and sc gmean, so it moves t by d (x - mean) sc = d (t - beta); gmean's rounding and the product's move sh by u |sc mean| each:
        |dt| <= (2 u + er) |t - beta| + |sc| dmean + 2 u |sc mean| + u |sh| + u |t|     (+ u |x sc| where C / vec > 256: a product and a sum)
    Behind a SiLU that error passes a slope <= 1.1 and the activation t / (1 + __expf(-t)) adds its own (conv_cpu.bound_act: the hardware
    exp2 moves with |t|); a bf16 result rounds once more (half an ulp <= 2^-8 |y|).  Where mean = 0 this is about 4 u |t|; on 1e3 +
    N(0, 1) inputs u |sc mean| ~ 1e3 u |gamma| dominates: the affine form sc x + sh itself costs that much, whatever the statistics."""
    B, HW, C = x.shape
    v, mean, var, rstd = gn_stats(x, groups, eps)
    g, b_ = gamma.double().view(1, 1, groups, -1), beta.double().view(1, 1, groups, -1)
    sc = rstd * g
    sh = b_ - sc * mean
    t = v * sc + sh
    nch = (HW + GN_PIX - 1) // GN_PIX
    e64 = (min(HW, GN_PIX) * (C // groups) + nch + 4) * 2.0 ** -53
    dmean = e64 * v.abs().mean((1, 3), keepdim=True)
    dvar = e64 * (v * v).mean((1, 3), keepdim=True) + 2.0 * mean.abs() * dmean
    er = dvar / (2.0 * (var + eps)) + 4 * 2.0 ** -53
    b = (2 * U32 + er) * (t - b_).abs() + sc.abs() * dmean + 2 * U32 * (sc * mean).abs() + U32 * sh.abs() + U32 * t.abs()
    if not fused:
        b = b + U32 * (v * sc).abs()
    b, t = 1.01 * b.view(B, HW, C), t.view(B, HW, C)
    if silu:
        b = 1.1 * b + bound_act(t)
    if bf16:
        b = b + UBF * (silu64(t) if silu else t).abs() + 2.0 ** -133
    return b + TINY


# ---- small reductions ------------------------------------------------------------------------------------------------------------------
def ref_adaln_bwd(dy, x, ss, B, R, C):
    """dx = dy (1 + scale[b]); dss[b, :C] = sum_r dy x, dss[b, C:] = sum_r dy   (float64)"""
    dy, x, ss = dy.double().view(B, R, C), x.double().view(B, R, C), ss.double().view(B, 2 * C)
    return dy * (1.0 + ss[:, None, :C]), torch.cat([(dy * x).sum(1), dy.sum(1)], 1)


def ref_sinusoid(f, dim, maxpos):
    """out[i, j] = cos(f_i w_j), out[i, half + j] = sin(f_i w_j), w_j = exp(-ln(maxpos) / half * j); +0 in the last column of an odd dim.
    Returns (out, scale): scale = 1 + |angle| - an f32 angle is only known to |angle| 2^-24"""
    half = dim // 2
    ang = f.double()[:, None] * torch.exp(-math.log(maxpos) / half * torch.arange(half, dtype=F64))[None, :]
    out = torch.zeros(f.numel(), dim, dtype=F64)
    out[:, :half], out[:, half:2 * half] = ang.cos(), ang.sin()
    scale = torch.ones(f.numel(), dim, dtype=F64)
    scale[:, :half] += ang.abs()
    scale[:, half:2 * half] += ang.abs()
    return out, scale


def ref_silu_bwd(x, dy):
    """(dx, scale): dx = dy s (1 + x (1 - s)), scale = |dy| s (1 + |x| (1 - s)) - the factor 1 + x (1 - s) cancels near x = -1.28"""
    x, dy = x.double(), dy.double()
    s = torch.sigmoid(x)
    return dy * s * (1.0 + x * (1.0 - s)), dy.abs() * s * (1.0 + x.abs() * (1.0 - s))


# ---- seeded defects --------------------------------------------------------------------------------------------------------------------
DEFECTS = ["tap_flip", "border_off_by_one", "image_boundary", "chunk_last_pixel", "wave_skipped", "tie_high", "lane_stride_tie",
           "pad_not_zeroed", "didj_swapped", "bf16_trunc", "grn_mean_c1", "gn_eps_x10", "gn_f32_stats"]
