"""CPU side of the optimizer edge tests (tests/test_optim_cpu.py, tests/test_gpu_optim_edges.py): an exact numpy model of csrc/optim.hip and
csrc/gradnorm.hip - the arithmetic of one element, and who updates which element - with switchable seeded defects (DEFECTS), the case lists
both test modules walk, and the builders of their inputs.

Everything here is judged bit for bit.  f32 `+ - * / sqrt` of numpy float32 arrays are the IEEE operations (round to nearest even, denormals
kept), which is what the kernels execute; the one operation numpy lacks, a fused multiply-add, is `fmaf` below.

The pinned update of one element (adam_update1 of csrc/optim.hip; s = the gradient factor):
    gr = round(g * s)
    d  = round(gr - m)  with a device factor  |  fma(g, s, -m)  with a host factor
    m' = fma(omb1, d, m)
    v' = fma(omb2, round(gr * gr), round(v * b2))
    denom = round(round(sqrt(v') / bc2_sqrt) + eps)
    p' = fma(decay, p, round(-step_size * round(m' / denom)))

Buffers.  Every tensor of a case lives in an `Arena`: one array per element size, filled with a sentinel, in which the tensors are placed at
chosen byte offsets with at least GUARD untouched elements on either side.  The model works on a copy of the arena in place; the GPU test
uploads the arena, runs the kernel on views of it, downloads it and compares ALL of it - so a write outside a tensor is a failure as well.
"""
import functools
import math

import numpy as np

F = np.float32
CHUNK = 4096
GUARD = 16
SENT32 = 0x7FC0DEAD          # quiet NaNs with a payload: no kernel result has these bits
SENT16 = 0x7FC1
INT_MIN = -(1 << 31)

DEFECTS = (
    # the update
    "eps_inside_bias_correction", "no_second_bias_correction", "beta1_for_one_minus_beta1", "decay_after_step", "uncontracted_last",
    "device_factor_contracted",
    # dispatch
    "flat_tail_dropped", "span_last_quad_dropped", "span_tail_from_hi", "no_second_sweep", "boundary_chunk_first_group", "base_ignored",
    "seg_of_off_by_one", "tensor_of_chunk_empty", "group_wrong_row",
    # images and the skip guard
    "lo_from_p", "lo_wrong_distance", "half_through_bf16", "image_on_skip", "skip_vector_only",
    # EMA
    "ema_contracted", "ema_copy_updates",
    # chunk_sumsq
    "sumsq_wave3_left_out", "sumsq_ragged_twice", "sumsq_padding_counted", "sumsq_fold_pairwise",
    # finalize
    "finalize_second_tile_dropped", "finalize_ticket_not_reset",
)


def rup(x, m):
    return (x + m - 1) // m * m


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """fma(a, b, c) of float32 arrays with ONE rounding.  The product of two f32 is exact in float64; the sum with c is taken in float64
    with TwoSum; the float64 sum rounds to f32 correctly unless it is an f32 midpoint while the residual is not zero - then the residual,
    not the tie rule, decides the direction."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        pr = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = pr + c64
        bb = s - pr
        e = (pr - (s - bb)) + (c64 - bb)
        r = s.astype(F)
        r64 = r.astype(np.float64)
        other = np.nextafter(r, np.where(s > r64, F(np.inf), F(-np.inf)).astype(F))
        mid = np.isfinite(r64) & (r64 != s) & ((s - r64) == (other.astype(np.float64) - s)) & (e != 0) & np.isfinite(e)
        r = np.where(mid, np.where(e > 0, np.maximum(r, other), np.minimum(r, other)), r)
    return r.astype(F)


def bf16_bits(x):
    """f32 -> bf16, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F)


def half_bits(x):
    """f32 -> IEEE half, round to nearest even, overflow to inf, subnormals"""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(x, F).astype(np.float16).view(np.uint16)


def adam_hyper(lr, beta1, beta2, eps, weight_decay, step):
    """the host's constants (adam_hyper of csrc/optim.hip): the arguments arrive as f32, the arithmetic is double, each constant rounds once"""
    lr, beta1, beta2, eps, weight_decay = (float(F(x)) for x in (lr, beta1, beta2, eps, weight_decay))
    bc1, bc2 = 1.0 - math.pow(beta1, float(step)), 1.0 - math.pow(beta2, float(step))
    return dict(step_size=F(lr / bc1), bc2_sqrt=F(math.sqrt(bc2)), decay=F(1.0 - lr * weight_decay), omb1=F(1.0 - beta1),
                omb2=F(1.0 - beta2), b1=F(beta1), b2=F(beta2), eps=F(eps))


def fill_groups(groups, step):
    """adam_fill_groups: eight rows, rows >= ngroups are row 0"""
    H = [adam_hyper(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], step) for g in groups]
    return H + [H[0]] * (8 - len(H))


def update1(p, g, m, v, h, s, dev, defect=None):
    """one AdamW update of float32 arrays -> (p', m', v')"""
    s = F(s)
    with np.errstate(all="ignore"):
        gr = g * s
        d = (gr - m) if (dev and defect != "device_factor_contracted") else fmaf(g, s, -m)
        m1 = fmaf(h["b1"] if defect == "beta1_for_one_minus_beta1" else h["omb1"], d, m)
        v1 = fmaf(h["omb2"], gr * gr, v * h["b2"])
        if defect == "eps_inside_bias_correction":
            denom = (np.sqrt(v1) + h["eps"]) / h["bc2_sqrt"]
        elif defect == "no_second_bias_correction":
            denom = np.sqrt(v1) + h["eps"]
        else:
            denom = np.sqrt(v1) / h["bc2_sqrt"] + h["eps"]
        t = -h["step_size"] * (m1 / denom)
        if defect == "decay_after_step":
            p1 = (p + t) * h["decay"]
        elif defect == "uncontracted_last":
            p1 = p * h["decay"] + t
        else:
            p1 = fmaf(h["decay"], p, t)
    return p1.astype(F), m1.astype(F), v1.astype(F)


def ema1(s, p, omd, defect=None):
    omd = F(omd)
    with np.errstate(all="ignore"):
        if defect == "ema_contracted":
            return fmaf(-omd, s - p, s)
        return (s - omd * (s - p)).astype(F)


# ---- arenas -------------------------------------------------------------------------------------------------------------------------------
class Arena:
    """tensors placed in one array of `itemsize`-byte elements; the array's own start is at least 256-byte aligned on the device"""

    def __init__(self, itemsize):
        self.itemsize, self.n = itemsize, GUARD

    def place(self, n, off_bytes=0, align=16):
        assert off_bytes % self.itemsize == 0
        start = rup(self.n, align // self.itemsize) + off_bytes // self.itemsize
        self.n = start + n + GUARD
        return start

    def build(self):
        if self.itemsize == 4:
            return np.full(rup(self.n, 64), SENT32, dtype=np.uint32)
        return np.full(rup(self.n, 64), SENT16, dtype=np.uint16)


def f32view(A, off, n):
    return A[off:off + n].view(F)


@functools.lru_cache(maxsize=4)
def state_values(n, seed):
    """p, g, m, v of one tensor.  m, v start non-zero; g and v run from 2^-70 to 2^40 (v' = omb2 g^2 + b2 v then reaches sqrtf's scaled
    branch below 2^-96, subnormals and, with g = 0 and v = 0, zero)."""
    r = np.random.default_rng(seed)
    p = (r.standard_normal(n) * np.exp2(r.integers(-6, 5, n))).astype(F)
    m = ((r.random(n) + 0.25) * np.where(r.random(n) < 0.5, -1, 1) * np.exp2(r.integers(-12, 3, n))).astype(F)
    g = ((r.random(n) + 1.0) * np.where(r.random(n) < 0.5, -1, 1) * np.exp2(r.integers(-70, 41, n).astype(np.float64))).astype(F)
    v = ((r.random(n) + 1.0) * np.exp2(r.integers(-70, 41, n).astype(np.float64))).astype(F)
    kind = r.integers(0, 16, n)
    g[kind == 0] = 0.0
    tiny = (kind == 0) | (kind == 1)
    v[tiny] = ((r.random(n) + 1.0) * np.exp2(r.integers(-149, -100, n).astype(np.float64))).astype(F)[tiny]   # subnormal / scaled-sqrt range
    v[(kind == 0) & (r.random(n) < 0.5)] = 0.0
    m[kind == 2] = F(1e-30) * m[kind == 2]
    return p, g, m, v


# ---- who updates which element ---------------------------------------------------------------------------------------------------------
def span_cover(lo, hi, vec, defect=None):
    """adam_span: elements [lo, hi) of a tensor by one workgroup -> (indices on the quad path, indices on the one-element path)"""
    if not vec:
        return np.arange(0), np.arange(lo, hi)
    nq = (hi - lo) >> 2
    if defect == "span_last_quad_dropped" and nq and ((hi - lo) & 3) == 0:      # `i + 4 < hi` in place of `i + 3 < hi`
        nq -= 1
    tail = lo + (hi & ~3) if defect == "span_tail_from_hi" else lo + ((hi - lo) & ~3)
    return np.arange(lo, lo + 4 * nq), np.arange(tail, max(tail, hi))


def ew_grid(n):
    g = (n + 255) // 256
    return 4096 if g > 4096 else (1 if g < 1 else g)


def flat_cover(n, defect=None):
    """adamw_flat_kernel: grid-stride over the n >> 2 quads with at most 4096 blocks of 256, the n & 3 tail by block 0"""
    n4 = n >> 2
    threads = ew_grid((n + 3) // 4) * 256
    nq = min(n4, threads) if defect == "no_second_sweep" else n4
    return slice(0, 4 * nq), (slice(0, 0) if defect == "flat_tail_dropped" else slice(4 * n4, n))


def seg_of(seg_end, pos, defect=None):
    lo, hi = 0, len(seg_end) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if (seg_end[mid] >= pos) if defect == "seg_of_off_by_one" else (seg_end[mid] > pos):
            hi = mid
        else:
            lo = mid + 1
    return lo


def tensor_of_chunk(cf, lo, hi, cid, defect=None):
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if cf[mid] <= cid:
            lo = mid
        else:
            hi = mid
    if defect == "tensor_of_chunk_empty":            # the FIRST tensor that starts at this chunk: an empty one, where there is one
        while lo > 0 and cf[lo - 1] == cf[lo]:
            lo -= 1
    return lo


def chunk_first(sizes):
    first = [0]
    for n in sizes:
        first.append(first[-1] + (n + CHUNK - 1) // CHUNK)
    return first


# ---- AdamW over arenas ------------------------------------------------------------------------------------------------------------------
class Img:
    """the copy a tensor's update refreshes: pb = element offset of the (hi) image in the 16-bit arena, plo = distance of the lo plane"""

    def __init__(self, pb, plo=0, half=False):
        self.pb, self.plo, self.half = pb, plo, half


def _write_image(I, im, sel, pnew, defect):
    idx = np.arange(sel.start, sel.stop) if isinstance(sel, slice) else sel
    if im.half:
        I[im.pb + idx] = half_bits(bf16_f32(bf16_bits(pnew))) if defect == "half_through_bf16" else half_bits(pnew)
        return
    hi = bf16_bits(pnew)
    I[im.pb + idx] = hi
    if im.plo:
        with np.errstate(all="ignore"):
            lo = bf16_bits(pnew) if defect == "lo_from_p" else bf16_bits(pnew - bf16_f32(hi))
        I[im.pb + im.plo + (1 if defect == "lo_wrong_distance" else 0) + idx] = lo


def _apply(T, I, im, sel, on_vec, h, s, dev, skip, defect):
    """the update of the elements `sel` (one group, one path) of the tensor T = (p, g, m, v) views, in place"""
    p, g, m, v = T
    if skip is not None and int(np.int32(skip)) != 0:
        if defect == "image_on_skip" and im is not None:
            _write_image(I, im, sel, p[sel], defect)
        if not (defect == "skip_vector_only" and not on_vec):
            return
    p1, m1, v1 = update1(p[sel], g[sel], m[sel], v[sel], h, s, dev, defect)
    p[sel], m[sel], v[sel] = p1, m1, v1
    if im is not None:
        _write_image(I, im, sel, p1, defect)


def _aligned(offs, im):
    """adam_span's vector condition from the byte addresses"""
    return all((o * 4) % 16 == 0 for o in offs) and (im is None or ((im.pb * 2) % 8 == 0 and im.plo % 4 == 0))


def _views(A, rec):
    return tuple(f32view(A, rec[k], rec["n"]) for k in "pgmv")


def model_flat(A, I, rec, hyper, step, s, dev, skip=None, defect=None):
    """muse_adamw_flat[_dev] on the tensor `rec` ({p, g, m, v: offsets, n, img})"""
    n = rec["n"]
    if n <= 0:
        return
    h = adam_hyper(*hyper, step)
    quads, tail = flat_cover(n, defect)
    T = _views(A, rec)
    _apply(T, I, rec["img"], quads, True, h, s, dev, skip, defect)
    _apply(T, I, rec["img"], tail, False, h, s, dev, skip, defect)


def model_flat_groups(A, I, rec, base, n, seg_end, seg_group, groups, step, s, dev, skip=None, defect=None):
    """muse_adamw_flat_groups[_dev] on elements [base, base + n) of the flat tensor `rec`"""
    if n <= 0:
        return
    H = fill_groups(groups, step)
    T = tuple(f32view(A, rec[k] + base, n) for k in "pgmv")
    im = None if rec["img"] is None else Img(rec["img"].pb + base)
    vec = _aligned([rec[k] + base for k in "pgmv"], im)
    b = 0 if defect == "base_ignored" else base
    ends = np.asarray(seg_end, np.int64)
    for c0 in range(0, n, CHUNK):
        c1 = min(c0 + CHUNK, n)
        s0, s1 = seg_of(seg_end, b + c0, defect), seg_of(seg_end, b + c1 - 1, defect)
        if s0 == s1 or defect == "boundary_chunk_first_group":
            qv, qo = span_cover(c0, c1, vec, defect)
            h = H[seg_group[s0] & 7]
            _apply(T, I, im, qv, True, h, s, dev, skip, defect)
            _apply(T, I, im, qo, False, h, s, dev, skip, defect)
            continue
        k = np.arange(c0, c1)
        seg = s0 + np.minimum.accumulate(ends[s0:s1][None, :] <= (b + k)[:, None], axis=1).sum(1)   # `while (s < s1 && seg_end[s] <= pos) ++s`
        for sg in np.unique(seg):
            _apply(T, I, im, k[seg == sg], False, H[seg_group[sg] & 7], s, dev, skip, defect)


def model_multi(A, I, recs, ncol, groups, step, s, dev, skip=None, defect=None):
    """muse_adamw_multi[_groups][_dev] over the table of `recs` ({p, g, m, v, n, img, group}); ncol 6: group 0 and a plain bf16 copy"""
    H = fill_groups(groups, step)
    nt = len(recs)
    cf = chunk_first([r["n"] for r in recs])
    for cid in range(cf[-1]):
        t = tensor_of_chunk(cf, 0, nt, cid, defect)
        rec = recs[t]
        grp = (recs[(t + 1) % nt] if defect == "group_wrong_row" else rec)["group"] if ncol > 6 else 0
        im = rec["img"]
        if ncol == 6 and im is not None:
            assert not im.half and not im.plo
        n, lo = rec["n"], (cid - cf[t]) * CHUNK
        hi = min(lo + CHUNK, n)
        vec = _aligned([rec[k] for k in "pgmv"], im)
        qv, qo = span_cover(lo, hi, vec, defect)
        T = _views(A, rec)
        _apply(T, I, im, qv, True, H[grp & 7], s, dev, skip, defect)
        _apply(T, I, im, qo, False, H[grp & 7], s, dev, skip, defect)


def col6(rec):
    """column 6 of the 7-column table: group | lo plane distance << 8, a negative plane field = an IEEE-half image"""
    im = rec["img"]
    field = 0 if im is None else (-1 if im.half else im.plo)
    return (field << 8) | rec["group"]


def model_ema(A, recs, omd, defect=None):
    """muse_ema_multi over {s, p: offsets, n, copy}"""
    for r in recs:
        s, p = f32view(A, r["s"], r["n"]), f32view(A, r["p"], r["n"])
        if r["copy"] and defect != "ema_copy_updates":
            s[:] = p
        else:
            s[:] = ema1(s, p, omd, defect)


# ---- gradient norm ------------------------------------------------------------------------------------------------------------------------
def chunk_sumsq(x, cnt, defect=None, behind=None):
    """chunk_sumsq of csrc/gradnorm.hip for ONE chunk: x = its cnt <= 4096 values (f32); behind: the values that follow it in memory"""
    full = np.zeros(CHUNK, np.float64)
    full[:cnt] = np.asarray(x[:cnt], F).astype(np.float64)
    if defect == "sumsq_ragged_twice" and cnt & 3:
        full[cnt] = full[cnt - 1]
    if defect == "sumsq_padding_counted" and cnt & 3 and behind is not None:
        k = min(4 - (cnt & 3), len(behind))
        full[cnt:cnt + k] = np.asarray(behind[:k], F).astype(np.float64)
    with np.errstate(all="ignore"):
        sq = (full * full).reshape(4, 256, 4)                    # [r, lane, slot]: element i -> r = i / 1024, lane (i / 4) % 256, slot i % 4
        if defect == "sumsq_fold_pairwise":
            a = (sq[0] + sq[1]) + (sq[2] + sq[3])
        else:
            a = ((sq[0] + sq[1]) + sq[2]) + sq[3]                # a = 0; a = fma(x, x, a) for r = 0..3 (0 + x^2 is exact)
        lane = ((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])).reshape(4, 64)
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, idx ^ o]
        w = lane[:, 0]
        if defect == "sumsq_wave3_left_out":
            return (w[0] + w[1]) + w[2]
        return (w[0] + w[1]) + (w[2] + w[3])


def tensor_slab(x, defect=None, behind=None):
    """the slab entries of one parameter: one per 4096-element chunk counted from its own start"""
    n = len(x)
    return np.array([chunk_sumsq(x[c:c + CHUNK], min(CHUNK, n - c), defect, behind if c + CHUNK >= n else None) for c in range(0, n, CHUNK)],
                    np.float64)


def fold(x, defect=None):
    """lane 0's sequential fold, 2048 entries staged at a time"""
    x = np.asarray(x, np.float64)
    if defect == "finalize_second_tile_dropped":
        x = x[:2048]
    with np.errstate(all="ignore"):
        return np.float64(0.0) if len(x) == 0 else np.add.accumulate(np.concatenate([[0.0], x]))[-1]


def coef_scale(norm, grad_scale, max_norm):
    """out[1], out[2] from the f32 norm: c = max_norm / (norm + 1e-6f), coef = c > 1 ? 1 : c (a NaN stays), scale = grad_scale * coef"""
    with np.errstate(all="ignore"):
        c = F(max_norm) / (F(norm) + F(1e-6))
        coef = F(1.0) if c > F(1.0) else c
        return F(coef), F(F(grad_scale) * coef)


def norm_set(total, grad_scale):
    """the f32 values grad_scale * r can round to for r = the float64 sqrt of `total` and its two neighbours"""
    with np.errstate(all="ignore"):
        r = np.sqrt(np.float64(total))
        cands = [r, np.nextafter(r, np.float64(np.inf)), np.nextafter(r, np.float64(-np.inf))] if np.isfinite(r) and r > 0 else [r]
        return {F(np.float64(F(grad_scale)) * c).tobytes() for c in cands}


def model_finalize(slab, cf, grad_scale, max_norm, ticket=0, defect=None):
    """gradnorm_finalize_kernel -> dict(psum [nt], total, per-parameter norm sets, norm set, ticket afterwards, wrote: out[0..2] written)"""
    nt = len(cf) - 1
    psum = np.array([fold(slab[cf[t]:cf[t + 1]], defect) for t in range(nt)], np.float64)
    wrote = ticket == 0                     # the workgroup that draws ticket nt - 1 folds the parameters; tickets start where they were left
    total = fold(psum, defect)
    after = 0 if (wrote and defect != "finalize_ticket_not_reset") else ticket + nt
    return dict(psum=psum, total=total, per=[norm_set(s, grad_scale) for s in psum], norm=norm_set(total, grad_scale), ticket=after, wrote=wrote)


def grad_scale1(x, s):
    with np.errstate(all="ignore"):
        return (np.asarray(x, F) * F(s)).astype(F)


# ---- the case lists -----------------------------------------------------------------------------------------------------------------------
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)                 # lr, beta1, beta2, eps, weight_decay
GROUPS8 = [dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd) for lr, b1, b2, eps, wd in (
    (1e-3, 0.9, 0.999, 1e-8, 0.01), (3e-4, 0.9, 0.95, 1e-6, 0.0), (1e-2, 0.8, 0.99, 1e-8, 0.1), (5e-4, 0.95, 0.98, 1e-3, 0.05),
    (2e-3, 0.5, 0.9, 1e-8, 0.0), (1e-4, 0.99, 0.9999, 1e-10, 0.3), (7e-3, 0.0, 0.999, 1e-8, 0.01), (1e-3, 0.9, 0.5, 1e-5, 1.0))]
STEPS = (1, 7, 100000)
BIG = 4 * 256 * 4096 + 7                                # the flat kernel's 4096 x 256 lanes take 4 x that many elements in one sweep
SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 4093, 4095, 4096, 4097, 8191, 8192, 8193)
IMAGES = ("none", "bf16", "x3", "half")


def _place_tensor(A32, A16, n, seed, image="none", mis=None, img_off=0, plo_extra=0, group=0):
    """one tensor in the arenas: mis = {role: bytes off 16-byte alignment}; image planes img_off bytes off 8-byte alignment; the lo plane
    rup(n, 4) + 8 + plo_extra elements behind the hi plane"""
    mis = mis or {}
    rec = dict(n=n, seed=seed, group=group, img=None)
    for k in "pgmv":
        rec[k] = A32.place(n, mis.get(k, 0))
    if image != "none":
        if image == "x3":
            plo = rup(n, 4) + 8 + plo_extra
            pb = A16.place(plo + n, img_off, 8)
            rec["img"] = Img(pb, plo)
        else:
            rec["img"] = Img(A16.place(n, img_off, 8), 0, image == "half")
    return rec


def fill_tensor(A, rec, values=None):
    p, g, m, v = values if values is not None else state_values(rec["n"], rec["seed"])
    for k, x in zip("pgmv", (p, g, m, v)):
        f32view(A, rec[k], rec["n"])[:] = x


def _finish(case, A32, A16, recs):
    A, I = A32.build(), A16.build()
    for r in recs:
        fill_tensor(A, r, r.get("values"))
    case.update(A=A, I=I, recs=recs)
    return case


# adamw_flat: (name, n, image, factor, dev)
FLAT_CASES = [dict(name=f"flat-n{n}-{'bf16' if img else 'none'}-{'dev' if dev else 'host'}{f}", n=n, image=img, factor=f, dev=dev,
                   steps=(1, 100000) if n == BIG else STEPS)
              for n in (1, 2, 3, 4, 5, 1023, 1024, 1025) for img in (False, True) for f, dev in ((1.0, False), (0.5, False), (0.3, False), (0.3, True))]
FLAT_CASES += [dict(name="flat-big-bf16-host0.3", n=BIG, image=True, factor=0.3, dev=False, steps=(1, 100000)),
               dict(name="flat-big-none-dev0.3", n=BIG, image=False, factor=0.3, dev=True, steps=(100000,))]


def build_flat(case):
    A32, A16 = Arena(4), Arena(2)
    rec = _place_tensor(A32, A16, case["n"], 1000 + case["n"] % 977, "bf16" if case["image"] else "none")
    return _finish(dict(case), A32, A16, [rec])


def run_flat(case, defect=None, steps=None):
    """-> [(A, I) after each step]"""
    c = build_flat(case)
    out = []
    for step in (steps or case["steps"]):
        model_flat(c["A"], c["I"], c["recs"][0], HYPER, step, case["factor"], case["dev"], None, defect)
        out.append((c["A"].copy(), c["I"].copy()))
    return out


# adam_span through the multi-tensor forms
def _multi(name, tensors, ncol=7, groups=GROUPS8, factor=0.3, dev=False, steps=(1, 100000)):
    return dict(name=name, tensors=tensors, ncol=ncol, groups=groups, factor=factor, dev=dev, steps=steps)


def _t(n, image="none", group=0, mis=None, img_off=0, plo_extra=0):
    return dict(n=n, image=image, group=group, mis=mis, img_off=img_off, plo_extra=plo_extra)


MULTI_CASES = [
    _multi("multi7-sizes-8groups", [_t(n, IMAGES[i % 4], i % 8) for i, n in enumerate(SIZES)], steps=STEPS),
    _multi("multi7-sizes-8groups-dev", [_t(n, IMAGES[(i + 2) % 4], (i + 3) % 8) for i, n in enumerate(SIZES)], dev=True),
    _multi("multi6-sizes", [_t(n, IMAGES[i % 2]) for i, n in enumerate(SIZES)], ncol=6, groups=GROUPS8[:1], factor=0.5),
    _multi("multi6-sizes-dev", [_t(n, IMAGES[(i + 1) % 2]) for i, n in enumerate(SIZES)], ncol=6, groups=GROUPS8[:1], dev=True),
    _multi("multi7-misaligned", [_t(n, IMAGES[(i + j) % 4], (i + j) % 8, mis={k: 4})
                                 for i, n in enumerate((5, 1027, 4096, 4097, 8193)) for j, k in enumerate("pgmv")]),
    _multi("multi7-misaligned-8-12", [_t(n, "bf16", i, mis={k: 8 + 4 * (i & 1)}) for i, (n, k) in enumerate(zip((7, 1025, 4097, 4096), "pgmv"))],
           steps=(1,)),
    _multi("multi7-image-misaligned", [_t(n, im, (i + j) % 8, img_off=off) for i, n in enumerate((4, 5, 1024, 4096, 4097))
                                       for j, (im, off) in enumerate((("bf16", 2), ("bf16", 4), ("x3", 2), ("x3", 4), ("half", 2), ("half", 4)))],
           steps=(1,)),
    _multi("multi7-plane-distance", [_t(n, "x3", i % 8, plo_extra=e) for i, (n, e) in enumerate(((4, 1), (1024, 2), (4096, 3), (4097, 1), (8193, 2), (7, 3)))],
           steps=(7,)),
    _multi("multi7-one-tensor", [_t(4097, "x3", 5)], steps=(1,)),
    _multi("multi7-two-tensors", [_t(3, "half", 1), _t(4096, "bf16", 2)], steps=(1,)),
    _multi("multi7-three-tensors", [_t(8193, "none", 7), _t(1, "x3", 6), _t(1023, "half", 4)], steps=(100000,)),
    _multi("multi7-257-tensors", [_t(1 + i % 7, IMAGES[i % 4], i % 8) for i in range(257)], steps=(1,)),
    _multi("multi6-257-tensors", [_t(1 + (5 * i) % 9, IMAGES[i % 2]) for i in range(257)], ncol=6, groups=GROUPS8[:1], steps=(1,)),
    _multi("multi7-empty-head-middle-tail", [_t(0, "none", 1), _t(4097, "bf16", 2), _t(0, "x3", 3), _t(0, "none", 4), _t(5, "half", 5), _t(4096, "x3", 6),
                                             _t(0, "bf16", 7)], steps=(1,)),
    _multi("multi6-empty-head-middle-tail", [_t(0), _t(0), _t(1025, "bf16"), _t(0), _t(4096), _t(0)], ncol=6, groups=GROUPS8[:1], steps=(1,)),
    _multi("multi7-half-with-group", [_t(n, "half", g) for n, g in ((4, 7), (5, 1), (4096, 3), (4097, 6))], steps=(1,)),
    _multi("multi7-group-past-ngroups", [_t(1024, "bf16", 5), _t(5, "x3", 2), _t(4097, "none", 7), _t(7, "half", 3)], groups=GROUPS8[1:4], steps=(1,)),
]


def build_multi(case):
    A32, A16 = Arena(4), Arena(2)
    recs = [_place_tensor(A32, A16, t["n"], 2000 + 31 * i + t["n"] % 911, t["image"], t["mis"], t["img_off"], t["plo_extra"], t["group"])
            for i, t in enumerate(case["tensors"])]
    return _finish(dict(case), A32, A16, recs)


def run_multi(case, defect=None, skip=None):
    c = build_multi(case)
    out = []
    for step in case["steps"]:
        model_multi(c["A"], c["I"], c["recs"], case["ncol"], case["groups"], step, case["factor"], case["dev"], skip, defect)
        out.append((c["A"].copy(), c["I"].copy()))
    return out


# image rounding alone: lr = 0, weight_decay = 0, g = 0 -> p' = p exactly
def rounding_patterns():
    """f32 bit patterns at the rounding edges of the three images"""
    u = []
    for top in (0x3F80, 0x3F81, 0xBF80, 0xC2FF, 0x0080, 0x0001, 0x0000, 0x7F7F, 0x7F7E):          # even / odd upper halves, subnormals, the largest
        for low in (0x7FFF, 0x8000, 0x8001, 0x0000, 0xFFFF):
            u.append((top << 16) | low)
    for hi7 in (0x00, 0x01, 0x7F):                                                                     # the same edges in p - bf16(p)
        for ub in (0x01, 0x02, 0x03, 0x40, 0x41, 0x7E, 0x7F, 0x80, 0x81, 0xFE, 0xFF):
            for lb in (0x7F, 0x80, 0x81, 0x00):
                u.append(0x3F800000 | (hi7 << 16) | (ub << 8) | lb)
                u.append(0xC1000000 | (hi7 << 16) | (ub << 8) | lb)
    x = np.array(u, np.uint32).view(F)
    h = [65504.0, np.nextafter(F(65520.0), F(0)), 65520.0, 65519.0, 65536.0, 2.0 ** -24, 2.0 ** -25, np.nextafter(F(2.0 ** -25), F(0)),
         np.nextafter(F(2.0 ** -25), F(1)), 1.5 * 2.0 ** -24, 2.0 ** -14, np.nextafter(F(2.0 ** -14), F(0)), 0.0, -0.0, 1.0 + 2.0 ** -11,
         1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23]
    h = np.array(h + [-a for a in h], F)
    x = np.concatenate([x, h])
    x = x[np.isfinite(x)]
    return np.concatenate([x, x[: (-len(x)) % 4]])                                                     # a multiple of 4: no tail on the quad path


ROUNDING_HYPER = (0.0, 0.9, 0.999, 1e-8, 0.0)
ROUNDING_CASES = [dict(name=f"rounding-{im}-{path}", image=im, path=path) for im in ("bf16", "x3", "half") for path in ("quad", "one")]


def build_rounding(case):
    p = rounding_patterns()
    n = len(p)
    r = np.random.default_rng(77)
    values = (p, np.zeros(n, F), (r.random(n) + 0.5).astype(F), (r.random(n) + 0.5).astype(F))         # m > 0: -t is -0 and p' = p, -0 included
    A32, A16 = Arena(4), Arena(2)
    rec = _place_tensor(A32, A16, n, 0, case["image"], {"p": 4} if case["path"] == "one" else None, group=3)
    rec["values"] = values
    return _finish(dict(case, ncol=7, groups=[dict(lr=0.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)] * 4, factor=1.0, dev=False,
                        steps=(1,)), A32, A16, [rec])


def run_rounding(case, defect=None):
    c = build_rounding(case)
    model_multi(c["A"], c["I"], c["recs"], 7, c["groups"], 1, 1.0, False, None, defect)
    return [(c["A"].copy(), c["I"].copy())]


# adamw_flat_groups: (name, total, seg_end, seg_group, slices)
def _groups(name, total, seg_end, seg_group, slices=None, image=True, groups=GROUPS8, factor=0.3, dev=False, steps=(1, 100000)):
    return dict(name=name, total=total, seg_end=list(seg_end), seg_group=list(seg_group), slices=slices or [(0, total)], image=image, groups=groups,
                factor=factor, dev=dev, steps=steps)


GROUP_CASES = [
    _groups("groups-ends-4095-4096-4097", 3 * CHUNK + 5, (4095, 4096, 4097, 8192, 3 * CHUNK + 5), (0, 1, 2, 3, 4)),
    _groups("groups-end-inside-quad", 2 * CHUNK, (1022, 4098, 2 * CHUNK), (5, 6, 7), dev=True),
    _groups("groups-many-boundaries", CHUNK + 100, (10, 13, 14, 2000, 2001, 4000, CHUNK + 100), (0, 1, 2, 3, 4, 5, 6), steps=(1,)),
    _groups("groups-two-boundaries", CHUNK, (1000, 3000, CHUNK), (7, 0, 3), image=False, steps=(1,)),
    _groups("groups-empty-segment", 2 * CHUNK + 3, (100, 100, 5000, 5000, 5000, 2 * CHUNK + 3), (1, 2, 3, 4, 5, 6), steps=(1,)),
    _groups("groups-one-segment", CHUNK + 7, (CHUNK + 7,), (4,), steps=(7,)),
    _groups("groups-slices", 4 * CHUNK, (4096, 8192, 9000, 4 * CHUNK), (1, 2, 3, 4), slices=[(0, 2052), (2052, 8188), (10240, 4 * CHUNK - 10240)], steps=(1,)),
    _groups("groups-slice-ends-inside-segment", 3 * CHUNK, (5000, 3 * CHUNK), (6, 2), slices=[(1000, 3000), (4000, 4097)], dev=True, steps=(1,)),
    _groups("groups-past-last-end", 2 * CHUNK + 9, (100, 4096, 5000), (1, 2, 3), steps=(1,)),
    _groups("groups-past-last-end-slice", 3 * CHUNK, (4096, 6000), (7, 5), slices=[(4100, 2 * CHUNK - 4)], steps=(1,)),
    _groups("groups-eight", 2 * CHUNK + 1, (1000, 2000, 3000, 4000, 5000, 6000, 8191, 2 * CHUNK + 1), (7, 6, 5, 4, 3, 2, 1, 0), steps=(1,)),
]


def build_groups(case):
    A32, A16 = Arena(4), Arena(2)
    rec = _place_tensor(A32, A16, case["total"], 3000 + case["total"] % 907, "bf16" if case["image"] else "none")
    return _finish(dict(case), A32, A16, [rec])


def run_groups(case, defect=None, skip=None):
    c = build_groups(case)
    out = []
    for step in case["steps"]:
        for base, n in case["slices"]:
            model_flat_groups(c["A"], c["I"], c["recs"][0], base, n, case["seg_end"], case["seg_group"], case["groups"], step, case["factor"],
                              case["dev"], skip, defect)
        out.append((c["A"].copy(), c["I"].copy()))
    return out


# the skip guard: form x factor kind, at an aligned and a misaligned tensor (flat forms refuse misaligned tensors: aligned only)
SKIP_VALUES = (1, -1, INT_MIN)
SKIP_MULTI = _multi("skip-multi", [_t(4097, "x3", 1), _t(1027, "half", 2, mis={"m": 4}), _t(5, "bf16", 3, mis={"p": 4}), _t(8, "bf16", 4)], steps=(1,))
SKIP_MULTI6 = _multi("skip-multi6", [_t(4097, "bf16"), _t(1027, "bf16", mis={"v": 4}), _t(8, "none")], ncol=6, groups=GROUPS8[:1], steps=(1,))
SKIP_GROUPS = _groups("skip-groups", CHUNK + 9, (1000, CHUNK + 9), (1, 2), steps=(1,))
SKIP_FLAT = dict(name="skip-flat", n=1027, image=True, factor=0.3, dev=False, steps=(1,))


# ema_multi
def _ema(name, tensors, omd):
    return dict(name=name, tensors=tensors, omd=omd)


EMA_CASES = [_ema(f"ema-sizes-omd{omd}", [dict(n=n, copy=(i % 5 == 4), mis=({}, {"s": 4}, {"p": 4}, {"s": 8, "p": 12})[i % 4])
                                         for i, n in enumerate(SIZES + (0, 4096, 0, 5))], omd) for omd in (0.0, 1.0, 1e-4)]
EMA_CASES.append(_ema("ema-empty-head-tail", [dict(n=n, copy=c, mis={}) for n, c in ((0, False), (4097, False), (0, True), (7, True), (0, False))], 1e-4))


def build_ema(case):
    A32 = Arena(4)
    recs = []
    for i, t in enumerate(case["tensors"]):
        rec = dict(n=t["n"], copy=t["copy"], s=A32.place(t["n"], t["mis"].get("s", 0)), p=A32.place(t["n"], t["mis"].get("p", 0)))
        recs.append(rec)
    A = A32.build()
    for i, rec in enumerate(recs):
        p, g, m, v = state_values(rec["n"], 4000 + i)
        f32view(A, rec["s"], rec["n"])[:] = p
        f32view(A, rec["p"], rec["n"])[:] = (p + m).astype(F) if i % 3 else g
    return dict(case, A=A, recs=recs)


def run_ema(case, defect=None):
    c = build_ema(case)
    model_ema(c["A"], c["recs"], case["omd"], defect)
    return [(c["A"].copy(),)]


# gradient norm: values with a 2^60 spread around a band of comparable magnitudes (so that the order of the sum shows), FLT_MAX, subnormals
GN_COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4093, 4095, 4096, 4097)
GN_STARTS = (0, 4, 8, 12)


def grad_values(n, seed):
    r = np.random.default_rng(seed)
    e = np.where(r.random(n) < 0.7, 30, r.integers(-30, 31, n)).astype(np.float64)
    x = ((r.random(n) + 1.0) * np.where(r.random(n) < 0.5, -1, 1) * np.exp2(e)).astype(F)
    x[r.random(n) < 0.02] = F(1e-41)
    return x


def order_probe(n, seed):
    """values on which the order of the four-deep fold of one lane shows in the chunk's sum: lane 0, slot 0 holds 2^30, 0, 10, 10 (squares
    2^60, 0, 100, 100: added one by one each 100 is less than half an ulp of 2^60 and vanishes; added as a pair they round up to 256) and
    every other value is small enough for the chunk's sum to stay below 2^61"""
    r = np.random.default_rng(seed)
    x = ((r.random(n) + 1.0) * np.where(r.random(n) < 0.5, -1, 1)).astype(F)
    x[[0, 1024, 2048, 3072]] = (2.0 ** 30, 0.0, 10.0, -10.0)
    return x


def build_gradnorm_multi():
    """one table: every count at every start; the last tensors hold FLT_MAX and the order probe"""
    A32 = Arena(4)
    recs = [dict(n=n, g=A32.place(n, st)) for n in GN_COUNTS for st in GN_STARTS]
    recs += [dict(n=4097, g=A32.place(4097, 4)), dict(n=4096, g=A32.place(4096, 0)), dict(n=4095, g=A32.place(4095, 8))]
    A = A32.build()
    for i, r in enumerate(recs):
        f32view(A, r["g"], r["n"])[:] = grad_values(r["n"], 5300 + i) if i < len(recs) - 2 else order_probe(r["n"], 5300 + i)
    f32view(A, recs[-3]["g"], 4097)[[0, 4095, 4096]] = np.finfo(F).max
    return dict(A=A, recs=recs, cf=chunk_first([r["n"] for r in recs]))


def model_gradnorm_multi(c, defect=None):
    out = []
    for r in c["recs"]:
        end = r["g"] + r["n"]
        out.append(tensor_slab(f32view(c["A"], r["g"], r["n"]), defect, c["A"][end:end + 4].view(F)))
    return np.concatenate(out)


GN_FLAT_SIZES = (5, 1023, 4096, 3, 4097, 8, 4093, 1, 8193)
GN_FLAT_PADS = (0, 1, 0, 5, 3, 0, 7, 2, 0)
GN_FLAT_RANGES = ([(0, 9)], [(0, 3), (3, 6), (6, 9)], [(6, 9), (0, 1), (1, 6)])      # (t0, t1): head, middle, tail in several cuts and orders


def build_gradnorm_flat(pad_value=3.0e30):
    offs, o = [], 1                                        # odd offsets: parameter starts aligned to nothing
    for sz, pd in zip(GN_FLAT_SIZES, GN_FLAT_PADS):
        offs.append(o)
        o += sz + pd
    g = np.full(o + 8, pad_value, F)
    for i, (sz, off) in enumerate(zip(GN_FLAT_SIZES, offs)):
        g[off:off + sz] = order_probe(sz, 6000 + i) if sz == 4096 else grad_values(sz, 6000 + i)
    return dict(g=g, offs=offs, end=o, cf=chunk_first(GN_FLAT_SIZES))


def model_gradnorm_flat(c, defect=None):
    return np.concatenate([tensor_slab(c["g"][o:o + n], defect, c["g"][o + n:o + n + 4]) for o, n in zip(c["offs"], GN_FLAT_SIZES)])


# finalize on synthetic slabs
FIN_CHUNKS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 4097)
FIN_NT = (1, 2, 255, 256, 257, 2048, 2049)
FIN_SPECIAL = ("zero", "inf", "nan", "overflow")
FIN_MAX_NORMS = (0.5, 1e9, float("inf"))


def slab_values(n, seed):
    """non-negative f64 partials: a band of comparable magnitudes (each add rounds) under a 2^80 spread"""
    r = np.random.default_rng(seed)
    e = np.where(r.random(n) < 0.8, 0, r.integers(-60, 21, n)).astype(np.float64)
    return (r.random(n) + 0.5) * np.exp2(e)


def finalize_cases():
    """-> [dict(name, cf, slab, grad_scale)]"""
    cases = [dict(name="fin-chunks", cf=chunk_first([c * CHUNK for c in FIN_CHUNKS]), grad_scale=1.0)]
    for nt in FIN_NT:
        cases.append(dict(name=f"fin-nt{nt}", cf=chunk_first([CHUNK * (1 + (t % 3 == 1)) for t in range(nt)]), grad_scale=0.25 if nt % 2 else 1.0))
    for i, c in enumerate(cases):
        c["slab"] = slab_values(c["cf"][-1], 7000 + i)
    for kind in FIN_SPECIAL:
        slab = slab_values(5, 7100)
        if kind == "zero":
            slab[:] = 0.0
        elif kind == "inf":
            slab[2] = np.inf
        elif kind == "nan":
            slab[3] = np.nan
        else:
            slab[1] = 1e80                                  # finite in f64, its root times grad_scale overflows f32
        cases.append(dict(name=f"fin-{kind}", cf=[0, 2, 2, 5], slab=slab, grad_scale=1.0))
    return cases


# grad_scale
GS_SIZES = SIZES + (4096 * 3 - 1, 4096 * 3 + 1)
GS_FACTORS = (0.3, 0.0, 1.0)


def build_grad_scale():
    A32 = Arena(4)
    recs = [dict(n=n, g=A32.place(n, st)) for n in GS_SIZES for st in GN_STARTS]
    A = A32.build()
    for i, r in enumerate(recs):
        f32view(A, r["g"], r["n"])[:] = grad_values(r["n"], 8000 + i)
    return dict(A=A, recs=recs, cf=chunk_first([r["n"] for r in recs]))


def model_grad_scale(c, factor):
    A = c["A"].copy()
    for r in c["recs"]:
        f32view(A, r["g"], r["n"])[:] = grad_scale1(f32view(A, r["g"], r["n"]), factor)
    return A


# ---- which cases catch which defect (tests/test_optim_cpu.py asserts every entry; profiles/optim_edges.md lists them) ----------------------
CATCH = {
    "eps_inside_bias_correction": ["flat-n1024-none-host1.0", "multi7-sizes-8groups"],
    "no_second_bias_correction": ["flat-n1024-none-host1.0", "multi7-sizes-8groups"],
    "beta1_for_one_minus_beta1": ["flat-n5-none-host1.0", "groups-eight"],
    "decay_after_step": ["flat-n1024-none-host1.0", "multi7-sizes-8groups"],
    "uncontracted_last": ["flat-n1024-none-host1.0", "multi6-sizes"],
    "device_factor_contracted": ["flat-n1024-none-dev0.3", "multi7-sizes-8groups-dev", "groups-end-inside-quad"],
    "flat_tail_dropped": ["flat-n1-none-host1.0", "flat-n1025-bf16-host0.5", "flat-big-bf16-host0.3"],
    "span_last_quad_dropped": ["multi7-sizes-8groups", "groups-one-segment", "multi7-two-tensors"],
    "span_tail_from_hi": ["multi7-sizes-8groups", "groups-one-segment", "multi7-one-tensor"],
    "no_second_sweep": ["flat-big-bf16-host0.3", "flat-big-none-dev0.3"],
    "boundary_chunk_first_group": ["groups-ends-4095-4096-4097", "groups-many-boundaries", "groups-two-boundaries"],
    "base_ignored": ["groups-slices", "groups-slice-ends-inside-segment", "groups-past-last-end-slice"],
    "seg_of_off_by_one": ["groups-ends-4095-4096-4097", "groups-eight"],
    "tensor_of_chunk_empty": ["multi7-empty-head-middle-tail", "multi6-empty-head-middle-tail"],
    "group_wrong_row": ["multi7-sizes-8groups", "multi7-257-tensors", "multi7-half-with-group"],
    "lo_from_p": ["multi7-sizes-8groups", "rounding-x3-quad", "rounding-x3-one"],
    "lo_wrong_distance": ["multi7-plane-distance", "rounding-x3-quad"],
    "half_through_bf16": ["multi7-half-with-group", "rounding-half-quad", "rounding-half-one"],
    "image_on_skip": ["skip-multi", "skip-multi6", "skip-groups", "skip-flat"],
    "skip_vector_only": ["skip-multi", "skip-multi6", "skip-groups", "skip-flat"],
    "ema_contracted": ["ema-sizes-omd0.0001", "ema-empty-head-tail"],
    "ema_copy_updates": ["ema-sizes-omd0.0001", "ema-sizes-omd1.0", "ema-empty-head-tail"],
    "sumsq_wave3_left_out": ["gradnorm-multi", "gradnorm-flat"],
    "sumsq_ragged_twice": ["gradnorm-multi", "gradnorm-flat"],
    "sumsq_padding_counted": ["gradnorm-multi", "gradnorm-flat"],
    "sumsq_fold_pairwise": ["gradnorm-multi", "gradnorm-flat"],
    "finalize_second_tile_dropped": ["fin-chunks", "fin-nt2049"],
    "finalize_ticket_not_reset": ["fin-chunks", "fin-nt1"],
}


def run_case(name, defect=None):
    """the model's outputs for the case `name` as a list of arrays (the skip cases run with the guard set)"""
    for cases, run in ((FLAT_CASES, run_flat), (MULTI_CASES, run_multi), (GROUP_CASES, run_groups), (ROUNDING_CASES, run_rounding), (EMA_CASES, run_ema)):
        for c in cases:
            if c["name"] == name:
                if cases is FLAT_CASES and c["n"] == BIG:
                    return [a for pair in run(c, defect, steps=c["steps"][:1]) for a in pair]
                return [a for pair in run(c, defect) for a in pair]
    if name in ("skip-multi", "skip-multi6"):
        return [a for pair in run_multi(SKIP_MULTI if name == "skip-multi" else SKIP_MULTI6, defect, skip=1) for a in pair]
    if name == "skip-groups":
        return [a for pair in run_groups(SKIP_GROUPS, defect, skip=-1) for a in pair]
    if name == "skip-flat":
        c = build_flat(SKIP_FLAT)
        model_flat(c["A"], c["I"], c["recs"][0], HYPER, 1, 0.3, False, INT_MIN, defect)
        return [c["A"], c["I"]]
    if name == "gradnorm-multi":
        return [model_gradnorm_multi(build_gradnorm_multi(), defect)]
    if name == "gradnorm-flat":
        return [model_gradnorm_flat(build_gradnorm_flat(), defect)]
    for c in finalize_cases():
        if c["name"] == name:
            first = model_finalize(c["slab"], c["cf"], c["grad_scale"], 1e9, 0, defect)
            second = model_finalize(c["slab"], c["cf"], c["grad_scale"], 1e9, first["ticket"], defect)
            return [first["psum"], np.float64([first["total"]]), np.array([first["wrote"], second["wrote"], second["ticket"]], np.float64)]
    raise KeyError(name)
