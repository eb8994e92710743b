"""CPU side of the tokenizer edge tests (tests/test_gpu_tokenizer_edges.py, tests/test_tokenizer_cpu.py) for the six entry points of
csrc/paella.hip and csrc/movq.hip: float64 references written as index arithmetic, the probes, a float32 contract model of each kernel
(operation for operation from the .hip comments and include/muse_hip.h) with switchable defects (DEFECTS), the checks and the derived
bounds.  Storage builders, guards, sentinels, `check_index`, `check_untouched`, `worst_ratio` and `bound_groupnorm` are spatial_cpu's.

Every reference and bound here is device-agnostic torch code: the GPU test evaluates the large SpatialNorm cases in float64 on the
device (16.8 M elements at the 1024-pixel apply chunk), the CPU test everything on the host.

Probes.  coordinate: every element holds a seeded id f32 carries exactly (conv_cpu.coord_ids), so the output of a data-movement kernel,
or of a product with one-hot weights, is ONE named input element.  integer: small integers with every partial sum below 2^24 - the f32
result does not depend on the summation order.  The rounding legs are judged per element against float64, normalised by the sum of the
absolute terms the element adds up.
"""
import math

import torch

import spatial_cpu as S
from conv_cpu import SPLIT_RES, U32, UBF, bound_act, coord_ids, silu64
from spatial_cpu import F32, F64, GUARD, TINY, alloc_out, gen, randn
from gemm_cpu import ints

NAN = float("nan")
SN_PIX = 1024             # csrc/movq.hip SN_PIX_PER_CHUNK: pixels per statistics chunk
CAP_BLOCKS = 32768        # csrc/paella.hip grid_for: blocks of 256 threads before the grid-stride loop takes over
LN_EPS = 1e-6


def f32r(a):
    """round a float64 expression to f32 and carry on in float64: a product of two f32 is exact in f64, so f32r(a * b + c) is the fused
    operation up to a double rounding"""
    return a.float().double()


def storage_of(t, dtype=F32):
    st = alloc_out(t.numel(), dtype)
    st[GUARD:GUARD + t.numel()] = t.flatten().to(dtype)
    return st


# =========================================================================================================================================
# muse_spatial_norm_nhwc
# =========================================================================================================================================
def sn_apix(batch, HW, cus):
    """the host's apply-chunk rule (csrc/movq.hip muse_spatial_norm_nhwc): 1024 pixels, halved down to 128 until batch * chunks >= 2 CUs"""
    if cus <= 0:
        cus = 256
    apix = SN_PIX
    while apix > 128 and batch * ((HW + apix - 1) // apix) < 2 * cus:
        apix >>= 1
    return apix


def sn_batch_for(apix, HW, cus):
    """the smallest batch at which sn_apix(batch, HW, cus) == apix, or None"""
    for b in range(1, 65536):
        a = sn_apix(b, HW, cus)
        if a == apix:
            return b
        if a > apix:
            return None
    return None


def sn_source(H, W, zh, zw, defect=None, device=None):
    """flat source pixel of zq [zh, zw] for every flat pixel p of [H, W]: (oy // (H / zh)) * zw + ox // (W / zw).
    "sn_src_off_f3": a factor of 3 taken as a shift by one (ox >> 1): one source pixel off wherever the two differ"""
    p = torch.arange(H * W, device=device)
    oy, ox = p // W, p % W
    fy, fx = H // zh, W // zw
    sy, sx = oy // fy, ox // fx
    if defect == "sn_src_off_f3":
        if fy == 3:
            sy = (oy >> 1).clamp(max=zh - 1)
        if fx == 3:
            sx = (ox >> 1).clamp(max=zw - 1)
    return sy * zw + sx


def sn_inputs(B, H, W, C, zh, zw, Z, seed, kind="randn", coord_zq=False):
    """x [B, HW, C], zq [B, zh, zw, Z] and the eight parameter vectors, f32.  kind: "randn" N(0, 1), "1e3" 1e3 + N(0, 1), "const" one
    constant per image (the variance clamps to 0).  coord_zq: a distinct exact value per (image, source pixel, channel), spaced 1 / 4"""
    x = randn((B, H * W, C), seed, 1e3 if kind == "1e3" else 0.0)
    if kind == "const":
        x = (torch.arange(B, dtype=torch.float32).view(B, 1, 1) * 0.5 + 1.25).expand(B, H * W, C).contiguous()
    if coord_zq:
        n = B * zh * zw * Z
        zq = ((torch.arange(n, dtype=F64) * 7919 % n) / 4.0 - n / 8.0).float().view(B, zh, zw, Z)
    else:
        zq = randn((B, zh, zw, Z), seed + 1)
    return dict(x=x, zq=zq, gamma=1 + 0.1 * randn((C,), seed + 2), beta=0.1 * randn((C,), seed + 3), wy=randn((C, Z), seed + 4) / math.sqrt(Z),
                by=1 + 0.1 * randn((C,), seed + 5), wb=randn((C, Z), seed + 6) / math.sqrt(Z), bb=0.1 * randn((C,), seed + 7))


def ref_spatial_norm(t, H, W, groups, eps, silu, src=None):
    """float64: n = GroupNorm(x), m = by + sum_k wy[k] zq[k], a = bb + sum_k wb[k] zq[k] at the pixel's source row, out = n m + a, then
    SiLU.  Also the sums of absolute terms Sm, Sa the two dot products add up (what their rounding is taken from)"""
    x = t["x"]
    B, HW, C = x.shape
    zq = t["zq"].double().reshape(B, -1, t["zq"].shape[-1])
    if src is None:
        src = sn_source(H, W, t["zq"].shape[1], t["zq"].shape[2], device=x.device)
    z = zq[:, src]                                                   # [B, HW, Z]
    wy, wb, by, bb = t["wy"].double(), t["wb"].double(), t["by"].double(), t["bb"].double()
    m, a = by + z @ wy.t(), bb + z @ wb.t()
    Sm, Sa = by.abs() + z.abs() @ wy.abs().t(), bb.abs() + z.abs() @ wb.abs().t()
    n = S.ref_groupnorm(x, t["gamma"], t["beta"], groups, eps, 0)[1]
    out = n * m + a
    return dict(y=silu64(out) if silu else out, t=out, n=n, m=m, a=a, Sm=Sm, Sa=Sa)


def bound_spatial_norm(t, r, groups, eps, silu, planes=False, stat_len=None, stat_parts=0):
    """spatial_cpu.bound_groupnorm (f64 statistics; one f32 rounding each of mean, rstd, sc, sh and the fma) gives |dn| of the normalised
    value n.  sn_element then forms m and a by Z fmas each from the bias upwards (k ascending): every fma rounds a partial sum <= Sm (Sa)
    once, u = 2^-24: |dm| <= Z u Sm, |da| <= Z u Sa; the outer fma(n, m, a) rounds once more:
        |dout| <= |dn| |m| + |n| Z u Sm + Z u Sa + u |out|                        (first order, 1 % on top)
    Behind the SiLU that passes a slope <= 1.1 and the activation adds its own error (conv_cpu.bound_act; the planes carry the
    hardware-reciprocal form it describes); planes read back as hi + lo drop at most 2^-17 of the value (SPLIT_RES).
    A producer's statistics: partial sums of up to stat_len pixels each, stat_parts of them folded - the same f64 allowance again with
    that length (bound_groupnorm's own allowance assumes the kernel's 1024-pixel chunks)."""
    x, gamma, beta = t["x"], t["gamma"], t["beta"]
    Z = t["zq"].shape[-1]
    bn = S.bound_groupnorm(x, gamma, beta, groups, eps, False, False)
    if stat_len is not None:
        B, HW, C = x.shape
        v, mean, var, rstd = S.gn_stats(x, groups, eps)
        e64 = (stat_len * (C // groups) + stat_parts + 4) * 2.0 ** -53
        dmean = e64 * v.abs().mean((1, 3), keepdim=True)
        dvar = e64 * (v * v).mean((1, 3), keepdim=True) + 2.0 * mean.abs() * dmean
        er = dvar / (2.0 * (var + eps))
        sc = rstd * gamma.double().view(1, 1, groups, -1)
        nb = (r["n"].view(B, HW, groups, -1) - beta.double().view(1, 1, groups, -1)).abs()
        bn = bn + 1.01 * (er * nb + sc.abs() * dmean).view(B, HW, C)
    b = 1.01 * (bn * r["m"].abs() + r["n"].abs() * Z * U32 * r["Sm"] + Z * U32 * r["Sa"] + U32 * r["t"].abs())
    if silu:
        b = 1.1 * b + bound_act(r["t"], planes)
    elif planes:
        b = b + SPLIT_RES * r["t"].abs()
    return b + TINY


def ref_sn_partials(x, groups, terms=False):
    """f64 [B, nchunk, groups, 2]: sum / sum of squares of x [B, HW, C] per 1024-pixel chunk and group (sn_stats_kernel; the layout of
    spatial_cpu.ref_gn_partials, without padding every image to whole chunks).  terms: the sums of |v| and v^2"""
    B, HW, C = x.shape
    v = x.double().view(B, HW, groups, C // groups)
    parts = [torch.stack([(v[:, a:a + SN_PIX].abs() if terms else v[:, a:a + SN_PIX]).sum((1, 3)), (v[:, a:a + SN_PIX] ** 2).sum((1, 3))], -1)
             for a in range(0, HW, SN_PIX)]
    return torch.stack(parts, 1)


def sn_producer_partials(x, groups, cuts):
    """f64 [B, len(cuts) + 1, groups, 2]: sum / sum of squares per group over the pixel ranges the sorted `cuts` divide [0, HW) into - a
    producer's statistics, any partition.  Returns (partials, the longest range)"""
    B, HW, C = x.shape
    edges = [0] + list(cuts) + [HW]
    v = x.double().view(B, HW, groups, C // groups)
    parts = [torch.stack([v[:, a:b].sum((1, 3)), (v[:, a:b] ** 2).sum((1, 3))], -1) for a, b in zip(edges[:-1], edges[1:])]
    return torch.stack(parts, 1), max(b - a for a, b in zip(edges[:-1], edges[1:]))


def model_spatial_norm(t, H, W, groups, eps, silu, apix, defect=None):
    """the output storage sn_apply_kernel leaves, in float64 rounded to f32 where the kernel rounds: f64 statistics, gmean = f32(mean),
    grstd = f32(rstd), sc = f32(grstd gamma), sh = f32(beta - sc gmean), n = fma(x, sc, sh), m / a by Z fmas from the bias (k ascending),
    out = fma(n, m, a), SiLU.  defects: "gn_eps_x10", "sn_swap_convs" (conv_y and conv_b exchanged), "sn_src_off_f3" (sn_source),
    "sn_chunk_last_pixel" (the last pixel of every apply chunk is never stored), "gn_group_off" (the statistics' group boundary one
    channel late: channel c is counted in the group of c - 1)"""
    x = t["x"]
    B, HW, C = x.shape
    Z = t["zq"].shape[-1]
    xs = torch.roll(x, 1, dims=2) if defect == "gn_group_off" else x
    _, mean, _, rstd = S.gn_stats(xs, groups, eps * (10.0 if defect == "gn_eps_x10" else 1.0))
    sc = f32r(f32r(rstd) * t["gamma"].double().view(1, 1, groups, -1))
    sh = f32r(t["beta"].double().view(1, 1, groups, -1) - sc * f32r(mean))
    n = f32r(x.double().view(B, HW, groups, -1) * sc + sh).view(B, HW, C)
    z = t["zq"].double().reshape(B, -1, Z)[:, sn_source(H, W, t["zq"].shape[1], t["zq"].shape[2], defect)]
    ky, kb = ("wb", "bb") if defect == "sn_swap_convs" else ("wy", "by")
    ka, kab = ("wy", "by") if defect == "sn_swap_convs" else ("wb", "bb")
    m, a = t[kb].double().expand(B, HW, C), t[kab].double().expand(B, HW, C)
    for k in range(Z):
        m = f32r(t[ky].double()[:, k] * z[:, :, k:k + 1] + m)
        a = f32r(t[ka].double()[:, k] * z[:, :, k:k + 1] + a)
    out = f32r(n * m + a)
    if silu:
        out = f32r(silu64(out))
    st = storage_of(out)
    if defect == "sn_chunk_last_pixel":
        p = torch.arange(HW)
        lost = (p % apix == apix - 1) | (p == HW - 1)
        body = st[GUARD:GUARD + out.numel()].view(B, HW, C)
        body[:, lost] = alloc_out(1, F32)[0]
    return st


# =========================================================================================================================================
# muse_paella_mix_fwd
# =========================================================================================================================================
def mix_lanes(C):
    """lanes per pixel of ln_stats_kernel: the power of two >= C / 4, at most 64"""
    G = 1
    while G < C // 4 and G < 64:
        G <<= 1
    return G


def mix_inputs(B, H, W, C, seed, shift=0.0, onehot=False):
    """x [B, H, W, C], w9 [9, C] tap-major, bias [C], the six gammas.  onehot: a single unit tap per group of four channels, walking all
    nine taps with the group number (the neighbour probe), no bias"""
    x = randn((B, H, W, C), seed, shift)
    g = 0.5 * randn((6,), seed + 3)
    if onehot:
        w9 = torch.zeros(9, C)
        c = torch.arange(C)
        w9[(c // 4 + seed) % 9, c] = 1.0
        return x, w9, torch.zeros(C), g
    return x, randn((9, C), seed + 1) / 3.0, 0.1 * randn((C,), seed + 2), g


def ln_stats64(x, eps=LN_EPS):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / (var + eps).sqrt()


def _tap_index(n, k, mode):
    """source coordinate of tap offset k - 1 along an axis of n: replicate (clamp), or wrap"""
    i = torch.arange(n) + k - 1
    return i % n if mode == "wrap" else i.clamp(0, n - 1)


def ref_mix(x, w9, bias, g):
    """float64: y = x + g2 (bias + sum_t w9[t] T[clamp(p + t)]), T = LN(x) (1 + g0) + g1 - index arithmetic, replicate border.
    Returns (y, stats [pixels, 2], scale): scale = |x| + |g2| (|bias| + sum_t |w| (|LN| |1 + g0| + |g1|)), the sum of the absolute terms"""
    B, H, W, C = x.shape
    xd, w9, bias, g = x.double(), w9.double(), bias.double(), g.double()
    mean, rstd = ln_stats64(xd)
    ln = (xd - mean) * rstd
    T, Ta = ln * (1 + g[0]) + g[1], ln.abs() * (1 + g[0]).abs() + g[1].abs()
    acc, acca = bias.expand(B, H, W, C).clone(), bias.abs().expand(B, H, W, C).clone()
    for ky in range(3):
        iy = _tap_index(H, ky, "clamp")
        for kx in range(3):
            ix = _tap_index(W, kx, "clamp")
            acc += w9[ky * 3 + kx] * T[:, iy][:, :, ix]
            acca += w9[ky * 3 + kx].abs() * Ta[:, iy][:, :, ix]
    return xd + g[2] * acc, torch.cat([mean, rstd], -1).view(-1, 2), xd.abs() + g[2].abs() * acca


def model_mix(x, w9, bias, g, defect=None):
    """(y storage, stats storage) as the two kernels of muse_paella_mix_fwd leave them.  ln_stats_kernel: mean = f32(sum) * f32(1 / C),
    q = sum of fma(d, d, q) with d = f32(v - mean), rstd = 1 / sqrtf(q / C + eps) - the sums are taken in float64 and rounded once (the
    lane tree's order is not modelled).  mix_kernel: acc = bias, then per tap (ky, kx ascending)
    acc = fma(fma(f32((v - mean) * rstd), 1 + g0, g1), w, acc) with the neighbour clamped WITHIN the image, y = fma(g2, acc, x).
    defects: "mix_zero_pad" (a tap outside the image adds nothing), "mix_wrap", "mix_clamp_image" (the row clamp runs over B * H: a border
    tap reads the neighbouring image), "mix_kykx" (the weight of tap (kx, ky)), "ln_eps_1e5", "mix_centre_stats" (every tap is
    normalised with the centre pixel's mean and rstd)"""
    B, H, W, C = x.shape
    xd = x.double()
    inv_c = f32r(torch.tensor(1.0 / C, dtype=F64))
    mean = f32r(f32r(xd.sum(-1, keepdim=True)) * inv_c)
    d = f32r(xd - mean)
    q = f32r((d * d).sum(-1, keepdim=True))
    eps = 1e-5 if defect == "ln_eps_1e5" else LN_EPS
    rstd = f32r(1.0 / f32r(f32r(f32r(q * inv_c) + torch.tensor(eps).double()).sqrt()))
    ga, gb, g2 = f32r(1.0 + g.double()[0]), g.double()[1], g.double()[2]
    rows = xd.view(B * H, W, C)
    mrow, rrow = mean.view(B * H, W, 1), rstd.view(B * H, W, 1)
    r = torch.arange(B * H)
    yy, row0 = r % H, r - r % H
    acc = bias.double().expand(B * H, W, C).clone()
    for ky in range(3):
        iy = yy + ky - 1
        inside_y = (iy >= 0) & (iy < H)
        if defect == "mix_clamp_image":
            src_r = (r + ky - 1).clamp(0, B * H - 1)
        elif defect == "mix_wrap":
            src_r = row0 + iy % H
        else:
            src_r = row0 + iy.clamp(0, H - 1)
        for kx in range(3):
            ixr = torch.arange(W) + kx - 1
            inside = inside_y.view(-1, 1, 1) & ((ixr >= 0) & (ixr < W)).view(1, -1, 1)
            ix = ixr % W if defect == "mix_wrap" else ixr.clamp(0, W - 1)
            v = rows[src_r][:, ix]
            mu, rs = (mrow, rrow) if defect == "mix_centre_stats" else (mrow[src_r][:, ix], rrow[src_r][:, ix])
            tv = f32r(f32r(f32r(v - mu) * rs) * ga + gb)
            wv = w9.double()[kx * 3 + ky if defect == "mix_kykx" else ky * 3 + kx]
            new = f32r(tv * wv + acc)
            acc = torch.where(inside.expand_as(new), new, acc) if defect == "mix_zero_pad" else new
    y = f32r(g2 * acc + rows)
    return storage_of(y), storage_of(torch.cat([mean, rstd], -1))


# =========================================================================================================================================
# muse_patch_rows_nhwc
# =========================================================================================================================================
def ref_patch_rows(x, KS, stride, pt, pl, Ho, Wo):
    """y[(b, oy, ox)][(ky, kx, c)] = x[b, oy stride - pt + ky, ox stride - pl + kx, c], +0 outside the image; x [B, H, W, C], bit for bit"""
    B, H, W, C = x.shape
    out = torch.zeros(B, Ho, Wo, KS, KS, C, dtype=x.dtype)
    for ky in range(KS):
        iy = torch.arange(Ho) * stride - pt + ky
        for kx in range(KS):
            ix = torch.arange(Wo) * stride - pl + kx
            ok = ((iy >= 0) & (iy < H)).view(1, Ho, 1, 1) & ((ix >= 0) & (ix < W)).view(1, 1, Wo, 1)
            v = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            out[:, :, :, ky, kx] = torch.where(ok, v, torch.zeros_like(v))
    return out.view(B * Ho * Wo, KS * KS * C)


def patch_ramp(B, H, W, C, seed):
    """a coordinate ramp with every 13th element -0.0 (a copy keeps the sign, a sum with +0 would not)"""
    x = coord_ids((B, H, W, C), "f32", seed).float()
    x.view(-1)[::13] = -0.0
    return x


# =========================================================================================================================================
# muse_vq_nearest_small
# =========================================================================================================================================
def vq_chunk(D):
    """codes per LDS chunk: 8192 / DP with DP = 4 for D <= 4, else 8"""
    return 2048 if D <= 4 else 1024


def vq_margin(D):
    """two squared distances d = sum of D fma(t, t, d), t = f32(z - e): t rounds once (2 u on t^2), each fma once more: (D + 2) u per
    distance of the distance itself (all terms are positive), two distances compared: (D + 2) 2^-23"""
    return (D + 2) * 2.0 ** -23


def ref_vq(z, cb):
    """float64 direct squared distances [N, Kc] -> (idx: the lowest index of the smallest distance, or 0 for a row with no finite distance
    - NaN or +inf throughout; the winning distance; the distances)"""
    d = torch.zeros(z.shape[0], cb.shape[0], dtype=F64)
    d32 = torch.zeros(z.shape[0], cb.shape[0])                       # where the f32 kernel overflows to +inf
    for k in range(z.shape[1]):
        t = z.double()[:, k:k + 1] - cb.double()[None, :, k]
        d += t * t
        d32 += t.float() ** 2
    dead = ~(torch.isfinite(d) & torch.isfinite(d32)).any(1)
    idx = S.ref_argmin(d)
    idx = torch.where(dead, torch.zeros_like(idx), idx)
    best = torch.where(dead, torch.full((z.shape[0],), math.inf, dtype=F64), d[torch.arange(z.shape[0]), idx])
    return idx, best, d


def vq_quarter_edges(Kc, D):
    """the first and last code of each wave's quarter, in the first and in the last chunk"""
    CH = vq_chunk(D)
    out = set()
    for c0 in {0, ((Kc - 1) // CH) * CH}:
        nc = min(CH, Kc - c0)
        per = (nc + 3) >> 2
        for s in range(4):
            lo, hi = s * per, min(s * per + per, nc)
            if lo < hi:
                out |= {c0 + lo, c0 + hi - 1}
    return sorted(out)


def vq_tie_pairs(Kc, D, edge_ties=False):
    """code pairs that receive one vector: across a quarter boundary of chunk 0, across the chunk boundary, and in a late quarter of
    chunk 0 and an early quarter of chunk 1.  By default none of them is a quarter edge (those keep their unique winners), so a pair
    exists only where the codebook is large enough; edge_ties: the codes directly at the boundaries, which are quarter edges"""
    CH = vq_chunk(D)
    per = (min(CH, Kc) + 3) >> 2
    if edge_ties:
        pairs = [(per - 1, per), (CH - 1, CH), (3 * per + 1, CH + 1)]
        return [p for p in pairs if 0 <= p[0] < p[1] < Kc]
    edges, used, out = set(vq_quarter_edges(Kc, D)), set(), []
    for a, b in [(per - 2, per + 1), (CH - 2, CH + 1), (3 * per + 1, CH + 2)]:
        if 0 <= a < b < Kc and not {a, b} & (edges | used):
            out.append((a, b))
            used |= {a, b}
    return out


def vq_exact_case(N, D, Kc, seed, edge_ties=False):
    """small-integer z and codes (|v| <= 7: every distance is an integer <= 8 * 14^2, exact in f32), with planted winners on the quarter
    edges (row i's own vector, carrying a 9 no seeded code has, at edge i) and planted ties (vq_tie_pairs: the row's vector at both codes
    of a pair, each pair a row of its own).  edge_ties: the ties sit on quarter edges and replace the winners planted there"""
    z, cb = ints((N, D), 7, seed).float(), ints((Kc, D), 7, seed + 1).float()
    plant = [(e,) for e in vq_quarter_edges(Kc, D)] + vq_tie_pairs(Kc, D, edge_ties)
    for i, codes in enumerate(plant[:N]):
        row = N - 1 - i                                              # from the last row down: row 0 keeps a seeded vector
        z[row] = ints((D,), 7, seed + 10 + i).float()
        z[row, i % D] = 9.0 + (i // D)
        for c in codes:
            cb[c] = z[row]
    return z, cb


def model_vq(z_st, lead, ldz, cb, N, D, Kc, defect=None):
    """vq_small_kernel thread by thread, vectorised over rows: z row = z_st[lead + row ldz + k], k < D; per chunk of CH codes wave s scans
    codes [s per, min(s per + per, nc)), per = (nc + 3) >> 2, in ascending order with d = fma(t, t, d), t = f32(z - e), replacing on `<`
    (a NaN distance never replaces); the four waves are merged on (distance, index).  Returns (idx int64 [N], dist f32 [N]).
    defects: "vq_tie_high" (the merge prefers the higher index), "vq_chunk_last" (the last code of every chunk is not scanned),
    "vq_quarter_floor" (per = nc >> 2: up to three codes of a chunk are skipped)"""
    CH = vq_chunk(D)
    rows = torch.arange(N)
    zr = z_st[(lead + rows[:, None] * ldz + torch.arange(D)[None, :])].double()
    best = torch.full((4, N), math.inf, dtype=F64)
    besti = torch.zeros((4, N), dtype=torch.int64)
    for c0 in range(0, Kc, CH):
        nc = min(CH, Kc - c0)
        per = nc >> 2 if defect == "vq_quarter_floor" else (nc + 3) >> 2
        for s in range(4):
            lo, hi = s * per, min(s * per + per, nc)
            if defect == "vq_chunk_last":
                hi = min(hi, nc - 1)
            if lo >= hi:
                continue
            e = cb[c0 + lo:c0 + hi].double()
            d = torch.zeros(N, hi - lo, dtype=F64)
            for k in range(D):
                tk = f32r(zr[:, k:k + 1] - e[None, :, k])
                d = f32r(tk * tk + d)
            d = torch.where(d.isnan(), torch.full_like(d, math.inf), d)
            qd, qi = d.min(1)
            qi = (d == qd[:, None]).float().argmax(1)             # the first of the smallest
            take = qd < best[s]
            best[s] = torch.where(take, qd, best[s])
            besti[s] = torch.where(take, c0 + lo + qi, besti[s])
    b, bi = best[0].clone(), besti[0].clone()
    for s in range(1, 4):
        tie = (besti[s] > bi) if defect == "vq_tie_high" else (besti[s] < bi)
        take = (best[s] < b) | ((best[s] == b) & tie)
        b, bi = torch.where(take, best[s], b), torch.where(take, besti[s], bi)
    return bi, b.float()


def check_vq_exact(idx, dist, z, cb, what):
    """exact leg: idx is the float64 argmin with the lowest index on ties (0 for a NaN / all-inf row), dist its distance bit for bit"""
    ri, rd, _ = ref_vq(z, cb)
    Kc = cb.shape[0]
    assert bool(((idx >= 0) & (idx < Kc)).all()), f"{what}: index out of [0, {Kc})"
    bad = idx != ri
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} rows differ from the float64 argmin, first row {int(bad.nonzero()[0])}: got "
                                 f"{int(idx[bad][0])}, expected {int(ri[bad][0])}")
    assert torch.equal(dist.double(), rd), f"{what}: a distance differs from the exact value (+inf on a NaN / all-inf row)"


def check_vq_seeded(idx, dist, z, cb, what, cap=0.01):
    """seeded leg: on every row whose float64 best / second-best gap exceeds vq_margin(D) of the second-best distance, idx is the float64
    argmin; at most `cap` of the rows fall under the margin, and those return one of the two candidates; dist is within the margin"""
    N, D = z.shape
    _, _, d = ref_vq(z, cb)
    Kc = cb.shape[0]
    assert bool(((idx >= 0) & (idx < Kc)).all()), f"{what}: index out of [0, {Kc})"
    two = torch.topk(d, min(2, Kc), dim=1, largest=False)
    best_i, best_d = two.indices[:, 0], two.values[:, 0]
    if Kc > 1:
        clear = (two.values[:, 1] - best_d) > vq_margin(D) * two.values[:, 1]
        second = two.indices[:, 1]
    else:
        clear, second = torch.ones(N, dtype=torch.bool), best_i
    assert int((~clear).sum()) <= cap * N, f"{what}: {int((~clear).sum())} of {N} rows under the margin: choose another seed"
    bad = clear & (idx != best_i)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} rows with a clear float64 winner differ, first row {int(bad.nonzero()[0])}"
    stray = ~clear & (idx != best_i) & (idx != second)
    assert not bool(stray.any()), f"{what}: a near-tie row returned neither candidate"
    got = d[torch.arange(N), idx]
    w = S.worst_ratio(dist, got, vq_margin(D) * got + TINY)
    assert w <= 1.0, f"{what}: distance error {w:.3f} x the margin"
    return w


# =========================================================================================================================================
# muse_paella_in_block / muse_paella_out_block
# =========================================================================================================================================
def unshuffle_rows(img, defect=None):
    """[B, 3, H, W] -> [B, H/2, W/2, 12] with k = c * 4 + dy * 2 + dx ("unshuffle_dydx": dx * 2 + dy; "unshuffle_corder": (dy, dx, c))"""
    B, _, H, W = img.shape
    v = img.reshape(B, 3, H // 2, 2, W // 2, 2)                      # b c oy dy ox dx
    if defect == "unshuffle_dydx":
        v = v.permute(0, 2, 4, 1, 5, 3)
    elif defect == "unshuffle_corder":
        v = v.permute(0, 2, 4, 3, 5, 1)
    else:
        v = v.permute(0, 2, 4, 1, 3, 5)
    return v.reshape(B, H // 2, W // 2, 12)


def ref_in_block(img, w12, bias, defect=None):
    """float64 (y [B, H/2, W/2, C], scale = |bias| + sum |u| |w|): y = bias + sum_k u_k w12[k]"""
    u = unshuffle_rows(img.double(), defect)
    return bias.double() + u @ w12.double(), bias.double().abs() + u.abs() @ w12.double().abs()


def model_in_block(img, w12, bias, defect=None):
    """in_block_kernel: acc = bias, then for c, dy ascending acc = fma(u1, w[k + 1], fma(u0, w[k], acc)) - k ascending, one fma each"""
    u = unshuffle_rows(img.double(), defect)
    acc = bias.double().expand(*u.shape[:3], w12.shape[1])
    for k in range(12):
        acc = f32r(u[..., k:k + 1] * w12.double()[k] + acc)
    return storage_of(acc)


def shuffle_img(o, defect=None):
    """[B, H2, W2, 12] (k = c * 4 + dy * 2 + dx) -> [B, 3, 2 H2, 2 W2]"""
    B, H2, W2, _ = o.shape
    v = o.reshape(B, H2, W2, 3, 2, 2)                                # b oy ox c dy dx
    if defect == "unshuffle_dydx":
        v = v.transpose(4, 5)
    return v.permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 2 * H2, 2 * W2)


def ref_out_block(x, w12, bias, defect=None):
    """float64 (img [B, 3, H, W], scale): x [B, H2, W2, C], w12 [12, C]: o_k = bias[k] + sum_c x_c w12[k, c], PixelShuffle(2)"""
    xd, w, b = x.double(), w12.double(), bias.double()
    return shuffle_img(xd @ w.t() + b), shuffle_img(xd.abs() @ w.abs().t() + b.abs())


def model_out_block(x, w12, bias, defect=None):
    """out_block_kernel: four chains (channel c feeds chain c % 4) of fmas over the channel vectors, ((a0 + a1) + (a2 + a3)) + bias[k].
    defects: "out_bias_swapped" (bias[k0 + 1] on the dx = 0 pixel and bias[k0] on dx = 1), "unshuffle_dydx" (shuffle_img)"""
    xd, w = x.double(), w12.double()
    B, H2, W2, C = x.shape
    a = torch.zeros(B, H2, W2, 12, 4, dtype=F64)
    for v in range(C // 4):
        a = f32r(xd[..., None, v * 4:v * 4 + 4] * w[:, v * 4:v * 4 + 4] + a)
    b = bias.double()
    if defect == "out_bias_swapped":
        b = b.view(6, 2).flip(1).reshape(12)
    o = f32r(f32r(f32r(a[..., 0] + a[..., 1]) + f32r(a[..., 2] + a[..., 3])) + b)
    return storage_of(shuffle_img(o, defect))


def block_case(probe, B, H, W, C, seed):
    """operands of both kernels for image [B, 3, H, W] and width C.  "int": small integers, every partial sum below 2^24.  "coord":
    in_block gets a coordinate image and a one-hot w12 (output channel c reads k = (c + seed) % 12) - y is ONE image pixel plus an integer
    bias; out_block gets one-hot x rows (pixel p holds a single 1 at channel (p + seed) % C) and coordinate weights and bias, so an image
    pixel is w12[k, that channel] + bias[k].  "randn": the rounding leg"""
    H2, W2 = H // 2, W // 2
    if probe == "int":
        c = dict(img=ints((B, 3, H, W), 255, seed).float(), w_in=ints((12, C), 63, seed + 1).float(), b_in=ints((C,), 1000, seed + 2).float(),
                 x=ints((B, H2, W2, C), 63, seed + 3).float(), w_out=ints((12, C), 63, seed + 4).float(), b_out=ints((12,), 1000, seed + 5).float())
        assert 12 * 255 * 63 + 1000 < 2 ** 24 and C * 63 * 63 + 1000 < 2 ** 24
    elif probe == "coord":
        w_in = torch.zeros(12, C)
        w_in[(torch.arange(C) + seed) % 12, torch.arange(C)] = 1.0
        x = torch.zeros(B * H2 * W2, C)
        x[torch.arange(B * H2 * W2), (torch.arange(B * H2 * W2) + seed) % C] = 1.0
        m = 1 << 22
        c = dict(img=(coord_ids((B, 3, H, W), "f32", seed) % m).float(), w_in=w_in, b_in=ints((C,), 1000, seed + 2).float(),
                 x=x.view(B, H2, W2, C), w_out=(coord_ids((12, C), "f32", seed + 4) % m).float(), b_out=(coord_ids((12,), "f32", seed + 5) % m).float())
    else:
        assert probe == "randn"
        c = dict(img=randn((B, 3, H, W), seed), w_in=randn((12, C), seed + 1) / 12 ** 0.5, b_in=0.1 * randn((C,), seed + 2),
                 x=randn((B, H2, W2, C), seed + 3), w_out=randn((12, C), seed + 4) / C ** 0.5, b_out=0.1 * randn((12,), seed + 5))
    c.update(probe=probe, exact=probe != "randn")
    return c


# =========================================================================================================================================
# the value check of a rounding leg, and the seeded defects
# =========================================================================================================================================
def check_rounding(st, n, ref, bound, what, guard=GUARD):
    """storage checks (guards, every slot written, no NaN), then per element |got - ref| <= bound; returns the worst ratio"""
    body = S.check_out(st, n, ref, what, guard=guard, values=False)
    w = S.worst_ratio(body, ref, bound)
    assert w <= 1.0, f"{what}: error {w:.3f} x its bound"
    return w


DEFECTS = ["mix_zero_pad", "mix_wrap", "mix_clamp_image", "mix_kykx", "ln_eps_1e5", "mix_centre_stats", "vq_tie_high", "vq_chunk_last",
           "vq_quarter_floor", "unshuffle_dydx", "unshuffle_corder", "out_bias_swapped", "sn_src_off_f3", "sn_chunk_last_pixel", "gn_eps_x10",
           "sn_swap_convs", "gn_group_off"]
