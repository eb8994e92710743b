"""CPU side of the convolution edge tests (tests/test_gpu_conv_edges.py, tests/test_conv_cpu.py): the float64 reference, the two exact
probes, the storage builders with their NaN / sentinel guards, the check functions, the per-path GroupNorm partial maps, the derived
rounding bounds, and a small model of the kernels' read / write contract with switchable defects.

Why integers: with integer operands and every partial sum below 2^24 the f32 result does not depend on the accumulation order, the tile
shape, the K order (tap, channel) or (chunk, tap, channel), or the pipeline depth - every path must return the float64 reference exactly.
`assert_exact` guards that bound on the operands of every case.

Read contract (csrc/gemm_core.h ConvLoader / PlainLoader, csrc/conv_dma.hip conv_dma_kernel / conv_slab_kernel, csrc/vqgan.hip direct
kernels): every loader masks a tap that falls into the padding (or a row past M / Cout) to an out-of-range buffer offset, so a kernel reads
the operand tensors and nothing else.  `place` therefore puts NaN in front of the operand's offset and behind its end; weight storage
continues with NaN rows past Cout; conv_in_direct's x holds NaN in channels Cin .. Cpad - 1.  One stray read makes an output NaN.
Write contract: out[B, H, W, Cout] (pooled: [B, H/2, W/2, Cout]) and, where asked, the f64 partials - `alloc_out` pre-fills both with a
NaN bit pattern no result has, guard bands included; the guards must come back bit for bit and every slot must be written.
"""
import math

import torch

from gemm_cpu import BF, F32, bits, ints, split_hi_lo

F64 = torch.float64
SENTINEL = {BF: 0x7FC1, F32: 0x7FC0DEAD, F64: 0x7FF8DEADDEADDEAD}
LIMIT = 1 << 24
LEAD = 64            # elements of NaN in front of every operand (a multiple of 8: the operand stays 16-byte aligned)
GUARD = 128          # sentinel elements on either side of an output


def in_dims(H, W, ups):
    """input height / width for OUTPUT dims H, W"""
    return (H // 2, W // 2) if ups == 1 else (2 * H, 2 * W) if ups == 2 else (H, W)


def silu64(t):
    t = t.double()
    return t / (1.0 + torch.exp(-t))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def tap_source(H, W, KS, ups, ky, kx):
    """for output pixel (y, x) and tap (ky, kx): source row / column in the input and whether the tap is inside it (else: zero)"""
    Hin, Win = in_dims(H, W, ups)
    pad = (KS - 1) // 2
    y, x = torch.arange(H), torch.arange(W)
    if ups == 2:                                   # stride 2 over the input padded by one zero row / column at the bottom / right
        iy, ix = 2 * y + ky, 2 * x + kx
        return iy, ix, iy < Hin, ix < Win
    uy, ux = y + ky - pad, x + kx - pad            # position in the (upsampled) SAME-padded plane
    oky, okx = (uy >= 0) & (uy < H), (ux >= 0) & (ux < W)
    if ups == 1:                                   # nearest x2: source = floor(u / 2)
        uy, ux = torch.div(uy, 2, rounding_mode="floor"), torch.div(ux, 2, rounding_mode="floor")
    return uy, ux, oky, okx


def ref_conv(x, w, H, W, KS, ups=0, bias=None, residual=None, scale=None, shift=None, pool=False):
    """float64 NHWC convolution written out over its taps: x [B, Hin, Win, Cin], w [Cout, KS, KS, Cin] -> [B, H, W, Cout]
    (pool: the 2 x 2 average of that, [B, H/2, W/2, Cout]).  scale / shift [B, Cin]: the input is silu(x * scale + shift), zero padded
    AFTER the activation."""
    x, w = x.double(), w.double()
    B, Cout = x.shape[0], w.shape[0]
    assert tuple(x.shape[1:3]) == in_dims(H, W, ups), (x.shape, H, W, ups)
    if scale is not None:
        x = silu64(x * scale.double()[:, None, None, :] + shift.double()[:, None, None, :])
    out = torch.zeros(B, H, W, Cout, dtype=F64)
    for ky in range(KS):
        for kx in range(KS):
            iy, ix, oky, okx = tap_source(H, W, KS, ups, ky, kx)
            g = x[:, iy.clamp(0, x.shape[1] - 1)][:, :, ix.clamp(0, x.shape[2] - 1)]
            g = g * (oky[:, None] & okx[None, :]).double()[None, :, :, None]
            out += g @ w[:, ky, kx, :].T
    if bias is not None:
        out += bias.double()
    if residual is not None:
        out += residual.double()
    return pool2(out) if pool else out


def pool2(o):
    """(((v0 + v1) + v2) + v3) * 0.25 over each 2 x 2 window, in o's dtype (v0 v1 / v2 v3 row-major)"""
    return (((o[:, 0::2, 0::2] + o[:, 0::2, 1::2]) + o[:, 1::2, 0::2]) + o[:, 1::2, 1::2]) * 0.25


def ref_x3(xh, xl, wh, wl, H, W, KS, ups=0, **kw):
    """the three-term bf16x3 sum hi hi + lo hi + hi lo - no lo lo term"""
    return ref_conv(xh.double() + xl.double(), wh, H, W, KS, ups, **kw) + ref_conv(xh, wl, H, W, KS, ups)


# ---- probes ----------------------------------------------------------------------------------------------------------------------------
COORD_MOD = {"bf16": 251, "x3": 65521, "f32": LIMIT - 4096}


def coord_ids(shape, kind, seed):
    """element ids the path's operands hold exactly: 1 .. mod - 1 (never 0: a padding tap is told from every element), scrambled so
    that neighbours in any direction differ"""
    n = math.prod(shape)
    lin = torch.arange(n, dtype=torch.int64)
    m = COORD_MOD[kind] - 1
    return (1 + (lin * 2654435761 + (seed % 1000003) * 40503) % m).view(shape)


def onehot_weights(Cout, KS, Cin, seed):
    """w [Cout, KS, KS, Cin] with a single 1 per output channel at (tap(co), ci(co)): the first min(Cout, taps * chunks) channels walk every
    tap and every 32-channel chunk, the rest are seeded.  Returns (w, tap, ci)."""
    taps, nch = KS * KS, (Cin + 31) // 32
    g = torch.Generator().manual_seed(seed & 0x7FFFFFFF)
    co = torch.arange(Cout)
    tap = torch.where(co < taps * nch, co % taps, torch.randint(0, taps, (Cout,), generator=g))
    chunk = torch.where(co < taps * nch, (co // taps) % nch, torch.randint(0, nch, (Cout,), generator=g))
    ci = torch.minimum(chunk * 32 + torch.randint(0, 32, (Cout,), generator=g), torch.tensor(Cin - 1))
    w = torch.zeros(Cout, taps, Cin, dtype=torch.int64)
    w[co, tap, ci] = 1
    return w.view(Cout, KS, KS, Cin), tap, ci


def sparse_pm1(Cout, K, nnz, seed):
    """[Cout, K] with at most nnz entries of +-1 per row (dense probe of the bf16-output path: results stay <= 256)"""
    g = torch.Generator().manual_seed(seed & 0x7FFFFFFF)
    w = torch.zeros(Cout, K, dtype=torch.int64)
    idx = torch.randint(0, K, (Cout, min(nnz, K)), generator=g)
    w.scatter_(1, idx, torch.randint(0, 2, idx.shape, generator=g) * 2 - 1)
    return w


def assert_exact(terms, bias=None, residual=None, out_dtype=F32):
    """the conditions that make a probe exact, checked on the operands themselves.  terms: list of (x, w) integer tensor pairs that are
    summed (one for f32 / bf16, three for bf16x3); w [Cout, ...].  Every partial sum is an integer below 2^24; a bf16 result is at most
    256 in magnitude (every such integer is a bf16 value), so neither the order nor a second rounding can show."""
    worst = 0.0
    for x, w in terms:
        for t in (x, w):
            assert torch.equal(t.double(), t.double().round()), "probe operands must be integers"
        worst += float(x.double().abs().max()) * float(w.double().abs().flatten(1).sum(1).max())
    for t in (bias, residual):
        if t is not None:
            assert torch.equal(t.double(), t.double().round()), "probe operands must be integers"
            worst += float(t.double().abs().max())
    assert worst < LIMIT, f"probe too large: a partial sum may reach {worst:.0f} >= 2^24"
    if out_dtype == BF:
        assert worst <= 256, f"bf16 output probe may reach {worst:.0f} > 256: not every such integer is a bf16 value"
    return worst


def exact_in(t, dtype):
    y = t.to(dtype)
    assert torch.equal(y.double(), t.double()), f"probe values are not exact in {dtype}"
    return y


# ---- storage ---------------------------------------------------------------------------------------------------------------------------
def place(t, dtype, lead=LEAD, tail=LEAD, exact=True):
    """flat storage: NaN x lead | the operand | NaN x tail.  The operand starts `lead` elements in (16-byte aligned).
    exact = False: the operand itself carries NaN (ignored channels) and is stored as it is."""
    assert lead % 8 == 0
    st = torch.full((lead + t.numel() + tail,), float("nan"), dtype=dtype)
    st[lead:lead + t.numel()] = (exact_in(t, dtype) if exact else t.to(dtype)).flatten()
    return st


def place_weights(w, dtype, extra_rows=2):
    """weight image [Cout, K] followed by NaN rows (a loader that does not mask rows past Cout reads them)"""
    return place(w.flatten(1), dtype, tail=LEAD + extra_rows * w[0].numel())


def sentinel(n, dtype):
    it = {BF: torch.int16, F32: torch.int32, F64: torch.int64}[dtype]
    v = SENTINEL[dtype]
    if dtype == BF:
        v -= 1 << 16 if v >= 1 << 15 else 0
    return torch.full((n,), v, dtype=it).view(dtype)


def alloc_out(n, dtype, guard=GUARD):
    """guard | n result slots | guard, all the sentinel NaN"""
    return sentinel(n + 2 * guard, dtype)


def check_same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), f"{what}: two launches from the same initial output differ"


def check_out(st, n, expected, what, guard=GUARD, exact=True, bound=None, values=True):
    """st: the storage after the launch.  Guards bit for bit, every slot written, no NaN, then the values: exact (torch.equal to the
    float64 reference) or |got - expected| <= bound per element.  values = False: the storage checks alone (the caller judges the values
    itself and wants the figure first); returns the result slots."""
    s = bits(sentinel(1, st.dtype))[0]
    b = bits(st)
    assert bool((b[:guard] == s).all()), f"{what}: wrote in front of the output"
    assert bool((b[guard + n:] == s).all()), f"{what}: wrote behind the output ({int((b[guard + n:] != s).sum())} elements)"
    body = st[guard:guard + n]
    unwritten = b[guard:guard + n] == s
    assert not bool(unwritten.any()), f"{what}: {int(unwritten.sum())} of {n} result slots were never written, first {int(unwritten.nonzero()[0])}"
    got, exp = body.double(), expected.double().flatten()
    nan = got.isnan()
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} NaN results (a read outside the operands), first at {int(nan.nonzero()[0])}"
    if not values:
        return body
    if exact:
        bad = got != exp
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {n} elements differ from the exact reference, first at "
                                     f"{int(bad.nonzero()[0])}: got {float(got[bad][0])}, expected {float(exp[bad][0])}")
    else:
        err = (got - exp).abs() / bound.double().flatten()
        assert float(err.max()) <= 1.0, f"{what}: error {float(err.max()):.3f} x its bound at {int(err.argmax())}"
    return body


# ---- GroupNorm partials ----------------------------------------------------------------------------------------------------------------
def partials_ref(out, path, groups):
    """f64 [B, nchunk, groups, 2] sum / sum of squares of `out` [B, H, W, Cout] (the tensor the partials describe: the pooled one for
    "pool") with each path's chunk-to-pixel map"""
    o = out.double()
    B, H, W, Cc = o.shape
    cpg = Cc // groups
    if path == "split":                       # conv_split_kernel: 128 consecutive pixels
        v = o.reshape(B, H * W // 128, 128, groups, cpg)
    elif path == "tap":                       # conv_dma_kernel: the 256-pixel tile
        v = o.reshape(B, H * W // 256, 256, groups, cpg)
    elif path in ("slab", "pool"):            # conv_slab*_kernel: patch img * tpi + prem, 16 x 16 pixels (8 x 8 pooled ones)
        e = 16 if path == "slab" else 8
        v = o.reshape(B, H // e, e, W // e, e, groups, cpg).permute(0, 1, 3, 2, 4, 5, 6).reshape(B, (H // e) * (W // e), e * e, groups, cpg)
    elif path == "row":                       # conv_in_direct: one image row
        v = o.reshape(B, H, W, groups, cpg)
    else:
        raise ValueError(path)
    return torch.stack([v.sum((2, 4)), (v * v).sum((2, 4))], -1)


def check_partials(st, expected, what, guard=GUARD):
    """per chunk slot, torch.equal (integer outputs: the f64 sums are exact in any order); guards bit for bit"""
    n = expected.numel()
    s = bits(sentinel(1, F64))[0]
    b = bits(st)
    assert bool((b[:guard] == s).all()) and bool((b[guard + n:] == s).all()), f"{what}: partials written outside their buffer"
    assert not bool((b[guard:guard + n] == s).any()), f"{what}: {int((b[guard:guard + n] == s).sum())} partial slots never written"
    got = st[guard:guard + n].view(expected.shape)
    bad = (got != expected).any(-1).any(-1)
    assert not bool(bad.any()), f"{what}: GroupNorm partials differ in (image, chunk) slots {bad.nonzero().tolist()[:6]}"


# ---- rounding bounds (test_gpu_conv_edges.py, rounding leg) -----------------------------------------------------------------------------
U32, UBF = 2.0 ** -24, 2.0 ** -8          # unit round-off of f32 (24 significant bits) and bf16 (8 significant bits)
# The hi / lo split of |x| in [2^e, 2^(e+1)): hi = bf16(x) leaves |x - hi| <= 2^(e-8) (half a bf16 ulp of that binade).  A remainder of
# exactly 2^(e-8) is a bf16 value (lo exact); a smaller one lies in the binade below, where half an ulp is 2^(e-17).  So
#   |x - hi - lo| <= 2^(e-17) <= 2^-17 |x|,   |lo| <= 2^-8 |x|.
# 2^-17 is attained (x = 1 + 2^-8 + 2^-17, tests/test_conv_cpu.py), so the often quoted 2^-18 is typical, not a bound.
SPLIT_RES = 2.0 ** -17


def abs_terms(x, w, H, W, KS, ups=0, bias=None, residual=None):
    """S = sum |x_i| |w_i| + |bias| + |res| per output element"""
    return ref_conv(x.double().abs(), w.double().abs(), H, W, KS, ups, bias=None if bias is None else bias.abs(),
                    residual=None if residual is None else residual.abs())


def bound_f32(S, K):
    """K exact-product f32 accumulations, bias and residual: every addition rounds a partial sum <= S: (K + 2) u S (first order, 1 % on top)"""
    return 1.01 * (K + 2) * U32 * S


def bound_bf16(S, K):
    """bf16 operands: products exact in f32, f32 accumulation as above; the bf16 output rounds once, and once more behind a staged bf16
    tile when a residual is added: 2 * 2^-8 S"""
    return bound_f32(S, K) + 2 * UBF * S


def bound_x3(S, K):
    """bf16x3: x = hi + lo + r with |r| <= 2^-17 |x| (SPLIT_RES), the same for w: 2 * 2^-17 per product; the dropped lo lo product is
    <= 2^-8 |x| 2^-8 |w| = 2^-16; 3 K f32 accumulations + bias + residual: (3 K + 2) u S"""
    return 1.01 * (2 * SPLIT_RES + 2.0 ** -16 + (3 * K + 2) * U32) * S


def bound_act(t, planes=False):
    """|gn_silu(fmaf(x, sc, sh)) - silu(t)| in f32, from its ingredients (csrc/common.h gn_silu): the fmaf rounds t once (2^-24 |t|; |silu'|
    <= 1.1); __expf(-t) is exp2(-t log2 e): the f32 product moves the exponent by <= 1.45 |t| 2^-24, i.e. e by a relative |t| 2^-24, and
    v_exp_f32 adds one ulp; 1 + e rounds once; v_rcp_f32 is good to one ulp; the final product rounds once.  With a = silu(t):
        |err| <= 2^-23 ((4 + 2 |t|) |a| + |t|)
    planes: the value is read back as hi + lo, which drops at most 2^-17 |a| (SPLIT_RES)."""
    t = t.double()
    a = silu64(t).abs()
    return 2.0 ** -23 * ((4 + 2 * t.abs()) * a + t.abs()) + (SPLIT_RES * a if planes else 0.0) + 1e-30


def silu32(x, sc, sh):
    """the f32 CPU evaluation of the same expression (E_ref of the activation)"""
    t = torch.addcmul(sh.float()[:, None, None, :], x.float(), sc.float()[:, None, None, :])
    return t / (1.0 + torch.exp(-t))


# ---- the contract model ----------------------------------------------------------------------------------------------------------------
DEFECTS = ["hborder", "vborder", "korder", "drop_chunk", "double_tail", "pad_before_act", "stride2_br", "ups_round", "ragged", "pool_shift",
           "partial_slot"]


def model_conv(planes, wimgs, H, W, KS, ups, Cin, Cout, *, order="tap", bias=None, residual=None, scale=None, shift=None, pool=False,
               gn=None, defect=None, out_dtype=F32, lead=LEAD):
    """What a kernel that follows the contract - or breaks it in ONE way - leaves in the output and partial storage.
    planes: flat input storages (`place`) that are summed (f32 / bf16: one; bf16x3: hi, lo); wimgs: flat weight storages [Cout, KS*KS*Cin]
    tap-major (`place_weights`), products taken as planes[0] x wimgs[0] (+ planes[1] x wimgs[0] + planes[0] x wimgs[1]).
    The model addresses the way the kernels do: a pixel index relative to the operand's start, a tap mask, and a buffer range that
    returns zero outside [0, size) - so an unmasked tap reads the neighbouring row / image, exactly as the hardware would.
    order: "tap" (k = tap * Cin + c: ConvLoader, conv_dma_kernel) or "slab" (k = (chunk * 9 + tap) * 32 + c: conv_slab*_kernel).
    gn = (path, groups): also the f64 partials.  Returns (out storage, partial storage or None)."""
    Hin, Win = in_dims(H, W, ups)
    taps, K = KS * KS, KS * KS * Cin
    B = (planes[0].numel() - 2 * lead) // (Hin * Win * Cin)
    npix = B * Hin * Win
    X = [p[lead:lead + npix * Cin].double().view(npix, Cin) for p in planes]
    pad = (KS - 1) // 2
    bb = torch.arange(B).view(B, 1, 1)
    A = [torch.zeros(B, H, W, taps, Cin, dtype=F64) for _ in X]
    for t in range(taps):
        ky, kx = t // KS, t % KS
        iy, ix, oky, okx = tap_source(H, W, KS, ups, ky, kx)
        if defect == "hborder" and ups == 0:
            okx = torch.ones_like(okx)
        if defect == "vborder" and ups == 0:
            oky = torch.ones_like(oky)
        if defect == "stride2_br" and ups == 2:
            oky, okx = torch.ones_like(oky), torch.ones_like(okx)
        if defect == "ups_round" and ups == 1:                 # trunc instead of floor, mask taken from the source index
            uy, ux = torch.arange(H) + ky - pad, torch.arange(W) + kx - pad
            iy, ix = torch.div(uy, 2, rounding_mode="trunc"), torch.div(ux, 2, rounding_mode="trunc")
            oky, okx = (iy >= 0) & (uy < H), (ix >= 0) & (ux < W)
        pix = (bb * Hin + iy.view(1, H, 1)) * Win + ix.view(1, 1, W)              # 32-bit offset arithmetic, no clamping
        ok = (oky.view(1, H, 1) & okx.view(1, 1, W)) & (pix >= 0) & (pix < npix)  # outside the buffer range: zero
        for Xi, Ai in zip(X, A):
            v = Xi[pix.clamp(0, npix - 1)]
            if scale is not None:
                sc, sh = scale.double()[:, None, None, :], shift.double()[:, None, None, :]
                v = silu64(v * sc + sh)
                if defect == "pad_before_act":
                    v = torch.where(ok[..., None], v, silu64(sh).expand_as(v))
                    Ai[:, :, :, t] = v
                    continue
            Ai[:, :, :, t] = v * ok[..., None].double()
    # K order of the activation and of the weight image
    nchunk = (Cin + 31) // 32

    def korder(o):
        k = torch.arange(K)
        if o == "tap":
            return k // Cin, k % Cin
        assert Cin % 32 == 0
        return (k // 32) % taps, (k // (32 * taps)) * 32 + k % 32
    ta, ca = korder(order)
    tw, cw = korder("tap" if defect == "korder" else order)
    M = B * H * W
    Wst = [wi[lead:lead + Cout * K].double().view(Cout, K) for wi in wimgs]
    Af = [Ai.view(M, taps, Cin)[:, ta, ca] for Ai in A]
    Wf = [Wi[:, tw * Cin + cw] for Wi in Wst]
    if defect == "drop_chunk":
        keep = (ca < (nchunk - 1) * 32).double()
        Af = [a * keep for a in Af]
    acc = Af[0] @ Wf[0].T
    if len(Af) > 1:
        acc = acc + Af[1] @ Wf[0].T
    if len(Wf) > 1:
        acc = acc + Af[0] @ Wf[1].T
    if defect == "double_tail":                                  # the padded loop runs the last K-tile of 32 once more
        acc = acc + Af[0][:, -32:] @ Wf[0][:, -32:].T
    if bias is not None:
        acc = acc + bias.double()
    if residual is not None:
        acc = acc + residual.double().view(M, Cout)
    o = acc.view(B, H, W, Cout)
    if pool:
        if defect == "pool_shift":
            o = torch.roll(o, -1, 1)
        o = pool2(o)
    n = o.numel()
    st = alloc_out(n, out_dtype)
    if defect == "ragged" and Cout % 128:                       # the last column tile stores all 128 columns of every row
        rows = o.reshape(-1, Cout).shape[0]
        spill = (torch.arange(rows)[:, None] * Cout + torch.arange(Cout, (Cout + 127) // 128 * 128)[None, :]).flatten()
        st[GUARD + spill[spill < n + GUARD]] = 0.0
    st[GUARD:GUARD + n] = o.flatten().to(out_dtype)
    part = None
    if gn is not None:
        path, groups = gn
        pr = partials_ref(st[GUARD:GUARD + n].view(o.shape), path, groups)
        if defect == "partial_slot":
            pr = torch.roll(pr, 1, 1)
        part = alloc_out(pr.numel(), F64)
        part[GUARD:GUARD + pr.numel()] = pr.flatten()
    return st, part


# ---- cases shared by the CPU and the GPU test ------------------------------------------------------------------------------------------
PATH_KIND = {"f32": "f32", "bf16": "bf16", "split": "x3", "split2": "x3"}


def build_case(path, probe, B, H, W, Cin, Cout, KS=3, ups=0, bias=False, res=False, seed=0):
    """operands, poisoned storage and the exact float64 expectation of one probe.  path: "f32" / "bf16" (muse_conv2d_nhwc), "split"
    (muse_conv2d_nhwc_split: f32 x, hi / lo weight images), "split2" (muse_conv2d_nhwc_split2: hi / lo planes and images)"""
    kind = PATH_KIND[path]
    Hin, Win = in_dims(H, W, ups)
    K = KS * KS * Cin
    dt = BF if path == "bf16" else F32
    small = path == "bf16"
    bvec = ints((Cout,), 2 if small else 50, seed + 5) if bias else None
    rten = ints((B, H, W, Cout), 3 if small else 1000, seed + 6) if res else None
    wl = None
    if probe == "coord":
        x = coord_ids((B, Hin, Win, Cin), kind, seed)
        w, _, _ = onehot_weights(Cout, KS, Cin, seed + 1)
        if kind == "x3":                                      # every fifth channel takes its 1 from the lo image: it sees hi(x) alone
            lo_rows = (torch.arange(Cout) % 5 == 4).view(Cout, 1, 1, 1)
            wl = w * lo_rows
            w = w * ~lo_rows
    else:
        assert probe == "dense"
        if path == "bf16":
            x = ints((B, Hin, Win, Cin), 3, seed + 1)
            w = sparse_pm1(Cout, K, 64, seed + 2).view(Cout, KS, KS, Cin)
        elif path == "split2":
            x = None
            w, wl = ints((Cout, KS, KS, Cin), 7, seed + 2), ints((Cout, KS, KS, Cin), 7, seed + 3)
        else:
            x = ints((B, Hin, Win, Cin), 1023 if K <= 720 else 255, seed + 1)
            w = ints((Cout, KS, KS, Cin), 7, seed + 2)
            wl = ints((Cout, KS, KS, Cin), 7, seed + 3) if kind == "x3" else None
    c = dict(path=path, probe=probe, B=B, H=H, W=W, Cin=Cin, Cout=Cout, KS=KS, ups=ups, dt=dt, out_dtype=dt, bias=bvec, res=rten)
    if kind == "x3":
        if probe == "dense" and path == "split2":
            xh, xl = exact_in(ints((B, Hin, Win, Cin), 15, seed + 1), BF), exact_in(ints((B, Hin, Win, Cin), 7, seed + 4), BF)
        else:
            xh, xl = split_hi_lo(exact_in(x, F32))
            assert torch.equal(xh.double() + xl.double(), x.double()), "hi + lo does not carry the probe"
        assert_exact([(xh, w), (xl, w), (xh, wl)], bvec, rten)
        c["expected"] = ref_x3(xh, xl, w, wl, H, W, KS, ups, bias=bvec, residual=rten)
        c["planes"] = [place(xh, BF), place(xl, BF)]
        c["w_st"] = [place_weights(w, BF), place_weights(wl, BF)]
        if path == "split":
            c["x_st"] = place(x, F32)
    else:
        assert_exact([(x, w)], bvec, rten, out_dtype=dt)
        c["expected"] = ref_conv(x, w, H, W, KS, ups, bias=bvec, residual=rten)
        c["planes"] = [place(x, dt)]
        c["w_st"] = [place_weights(w, dt)]
    c["bias_t"] = bvec.float() if bias else None
    c["res_st"] = place(rten, dt) if res else None
    return c


def model_case(c, order="tap", gn=None, defect=None):
    """the contract model on a case of build_case"""
    return model_conv(c["planes"], c["w_st"], c["H"], c["W"], c["KS"], c["ups"], c["Cin"], c["Cout"], order=order, bias=c["bias"],
                      residual=c["res"], gn=gn, defect=defect, out_dtype=c["out_dtype"])
