"""Plain torch restatement of the fused attention kernels' operation (csrc/attention.hip, attention2.hip, attention3.hip and the causal
policy of attention_enc.hip), for tests/test_gpu_attention_edges.py and tests/test_attention_cpu.py.  Imports without a GPU.

Five layers:
  * `reference`: ctx, lse, dq, dk, dv of softmax(alpha q k^T) v in float64 on the rounded inputs, full visibility or causal, and the
    per-element "terms" normalisers: a result is judged against the sum of the magnitudes it adds up, not against the tensor's largest
    entry.  With p = softmax(alpha q k^T), dp = dO v^T and dsum = rowsum(dO * O):
        ctx  p |v|          dv  p^T |dO|          dq  alpha (p (|dp| + |dsum|)) |k|          dk  alpha (p (|dp| + |dsum|))^T |q|
    each with the 2^-102 floor of tests/test_gpu_row_edges.py; the log-sum-exp is judged by its absolute error;
  * `contract_model`: the same operation in float32 torch at the precision class the bf16 kernels document - bf16 operands into each
    of the five products, P and dS rounded to bf16 once, the row sum taken over the rounded P, f32 accumulation, everything else f32.
    It fixes where bf16 rounding is allowed; it is neither a copy of the kernels nor the code under test.  Its error against float64 is
    E_ref.  It also takes the three classic defects (`defect=`) that tests/test_attention_cpu.py seeds to prove that the checks can fail;
  * `core3_model` (`model_h16`, `model_x3`): the same for the two TF32-class cores of attention3.hip, f32 in and out - every product one
    IEEE-half product (gradient operands times the power-of-two scale S) or three bf16 products of hi / lo planes; with the defects of
    tests/test_gpu_attention_x3_edges.py (a missing 1 / S, an unscaled dsum, a skipped middle key block) besides the dropped / leaked key;
  * probe builders, every value exact in bf16 (asserted):
      - `address_probe`: key j carries its base-16 digits (a, b, c), their squares and three ones in nine feature columns, the query
        aimed at key t carries c' (2 a_t, 2 b_t, 2 c_t, -1, -1, -1, -a_t^2, -b_t^2, -c_t^2) with c' a power of two and alpha c' >= 32.
        The scores are -alpha c' (digit distance)^2: exactly 0 at the target, <= -32 everywhere else, all partial sums integers below
        2^24.  v is a small non-zero signed integer pattern that differs between neighbouring keys in every column.  So ctx = v[t]
        exactly, lse = 0, dv[j] = the sum of dO over the queries aimed at j, and dq, dk are bounded by the e^-32 leakage.  A leaked
        zero pad key ties the target at score 0 (ctx halves, lse = log 2); a dropped key returns a neighbour's row;
      - `uniform_probe`: q = 0, k random, v and dO small integers: lse = log(Skv) (one key too many or too few moves it by at least
        1 / (Skv + 1)), ctx the column mean, dv the same for every key, dk exactly 0, dq non-trivial and judged per element;
  * the checks the GPU tests apply (`check_address`, `check_uniform`, `check_random`): they raise AssertionError.

Tensors: operands and results are float32 / float64 [B * S, H] "row" tensors (H = heads * head_dim) as the entry points take them, lse is
[B * heads, Sq].  A case is a dict: B, Sq, Skv, nh, hd, alpha, causal, q, k, v, do (+ what its builder adds).
"""
import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TINY = 2.0 ** -102          # absolute floor of every normaliser (tests/test_gpu_row_edges.py)
BF16_SUB = 2.0 ** -133      # spacing of bf16 subnormals
BF16_ULP = 2.0 ** -8        # one bf16 rounding, relative (the spacing just below a power of two is 2^-8 of the value)
PROBE_LSE_TOL = 1e-5        # |lse| (address) and |lse - log Skv| (uniform); the smallest defect shift is log(1026 / 1025) = 9.7e-4
X3_TOL = 2.0 ** -14         # bf16x3 results of the uniform probe: 2^-16 per product (the documented class), two chained products, x 2
KINDS = ("ctx", "lse", "dq", "dk", "dv")
DEFECTS = ("drop_last", "leak_pad", "causal_plus", "causal_minus", "no_unscale", "dsum_unscaled", "skip_middle")
HALF = torch.float16
HALF_ULP = 2.0 ** -11       # one rounding to IEEE half, relative (normal range)
HALF_SUB_HALF = 2.0 ** -25  # half the spacing of half's subnormals: a magnitude at or below it rounds to 0, rounding into them is off by this much


def bf(t):
    """round to bf16, keep float32"""
    return t.to(BF).to(F32)


def hf(t):
    """round to IEEE half (nearest even, overflow to inf), keep float32"""
    return t.to(HALF).to(F32)


def assert_bf16_exact(**tensors):
    for name, t in tensors.items():
        assert torch.equal(t.to(BF).to(t.dtype), t), f"{name}: not exact in bf16"


def assert_half_exact(**tensors):
    for name, t in tensors.items():
        assert torch.equal(t.to(HALF).to(t.dtype), t), f"{name}: not exact in IEEE half"


def to_heads(t, B, S, nh, hd):
    """[B * S, nh * hd] -> [B, nh, S, hd]"""
    return t.reshape(B, S, nh, hd).permute(0, 2, 1, 3)


def to_rows(t):
    """[B, nh, S, hd] -> [B * S, nh * hd]"""
    B, nh, S, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, nh * hd)


def default_alpha(hd):
    return 1.0 / float(torch.sqrt(torch.tensor(hd, dtype=F32)))


def make_case(B, Sq, Skv, nh, hd, q, k, v, do, alpha=None, causal=False, **extra):
    c = dict(B=B, Sq=Sq, Skv=Skv, nh=nh, hd=hd, alpha=default_alpha(hd) if alpha is None else alpha, causal=causal, q=q, k=k, v=v, do=do)
    c.update(extra)
    return c


def bf_half(t):
    """round to bf16, then to half (a bf16 value below 2^-14 loses bits there); the result is exact in both formats (asserted)"""
    t = hf(bf(t))
    assert_bf16_exact(t=t)
    assert_half_exact(t=t)
    return t


def random_case(B, Sq, Skv, nh, hd, seed, causal=False, rnd=bf):
    """seeded N(0, 1) operands, rounded to bf16 (rnd = bf_half: exact in bf16 and half, the H16 cases; rnd = None: plain f32, both planes
    of the bf16x3 kernels in use)"""
    g = torch.Generator().manual_seed(seed)
    H = nh * hd
    rnd = rnd or (lambda t: t)
    q, do = (rnd(torch.randn((B * Sq, H), generator=g)) for _ in range(2))
    k, v = (rnd(torch.randn((B * Skv, H), generator=g)) for _ in range(2))
    return make_case(B, Sq, Skv, nh, hd, q, k, v, do, causal=causal)


def visible(Sq, Skv, causal, shift=0):
    """[Sq, Skv] bool: key j takes part in query i (causal: j <= i + shift; key 0 always, as in the kernel, so that no row is empty)"""
    if not causal:
        return None
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    return (j <= i + shift) | (j == 0)


def _operands(c, dt):
    B, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    return (to_heads(c["q"].to(dt), B, Sq, nh, hd), to_heads(c["k"].to(dt), B, Skv, nh, hd), to_heads(c["v"].to(dt), B, Skv, nh, hd),
            to_heads(c["do"].to(dt), B, Sq, nh, hd))


def reference(c):
    """float64 on the rounded inputs -> dict of row tensors: ctx, lse, dq, dk, dv and the normalisers t_ctx, t_dq, t_dk, t_dv"""
    q, k, v, do = _operands(c, F64)
    a = float(c["alpha"])
    s = (q @ k.transpose(-1, -2)) * a
    vis = visible(c["Sq"], c["Skv"], c["causal"])
    if vis is not None:
        s = s.masked_fill(~vis, -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    ctx = p @ v
    dp = do @ v.transpose(-1, -2)
    dsum = (do * ctx).sum(-1, keepdim=True)
    ds = p * (dp - dsum)
    w = p * (dp.abs() + dsum.abs())
    out = dict(ctx=ctx, dq=a * (ds @ k), dk=a * (ds.transpose(-1, -2) @ q), dv=p.transpose(-1, -2) @ do,
               t_ctx=p @ v.abs(), t_dq=a * (w @ k.abs()), t_dk=a * (w.transpose(-1, -2) @ q.abs()), t_dv=p.transpose(-1, -2) @ do.abs())
    out = {n: to_rows(t) for n, t in out.items()}
    for n in ("t_ctx", "t_dq", "t_dk", "t_dv"):
        out[n] = out[n].clamp(min=TINY)
    out["lse"] = lse.reshape(c["B"] * c["nh"], c["Sq"])
    return out


def contract_model(c, defect=None, bf16_out=True):
    """float32 at the kernels' documented precision class (module docstring) -> ctx, lse, dq, dk, dv BEFORE the final output rounding (the
    backward reads the context as the kernels do: rounded to the output type).  defect: None or one of DEFECTS, seeded into the
    visibility only - "drop_last" hides the last key, "leak_pad" appends one zero key / value row that every query sees, "causal_plus" /
    "causal_minus" move the causal mask edge by one key."""
    assert defect is None or defect in DEFECTS
    q, k, v, do = _operands(c, F32)
    assert_bf16_exact(q=q, k=k, v=v, do=do)
    B, Sq, Skv, nh = c["B"], c["Sq"], c["Skv"], c["nh"]
    a = float(c["alpha"])
    vis = visible(Sq, Skv, c["causal"], {"causal_plus": 1, "causal_minus": -1}.get(defect, 0))
    if defect == "drop_last":
        vis = torch.ones((Sq, Skv), dtype=torch.bool) if vis is None else vis.clone()
        vis[:, Skv - 1] = False
        assert Skv > 1
    if defect == "leak_pad":
        pad = torch.zeros_like(k[..., :1, :])
        k, v = torch.cat([k, pad], -2), torch.cat([v, pad], -2)
        if vis is not None:
            vis = torch.cat([vis, torch.ones((Sq, 1), dtype=torch.bool)], -1)
    s = (q @ k.transpose(-1, -2)) * a
    if vis is not None:
        s = s.masked_fill(~vis, -math.inf)
    m = s.amax(-1, keepdim=True)
    pb = bf(torch.exp(s - m))
    l = pb.sum(-1, keepdim=True)
    ctx = (pb @ v) / l
    lse = m + torch.log(l)
    o = bf(ctx) if bf16_out else ctx
    p = torch.exp(s - lse)
    dv = bf(p).transpose(-1, -2) @ do
    dsb = bf(p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True)))
    dq, dk = a * (dsb @ k), a * (dsb.transpose(-1, -2) @ q)
    if defect == "leak_pad":
        dk, dv = dk[..., :Skv, :], dv[..., :Skv, :]
    out = {n: to_rows(t) for n, t in dict(ctx=ctx, dq=dq, dk=dk, dv=dv).items()}
    out["lse"] = lse.reshape(B * nh, Sq)
    return out


def rounded_outputs(out, dtype=BF):
    """a model's outputs as an entry point returns them: ctx and the gradients rounded to the output type, lse float32"""
    return {n: (t if n == "lse" else t.to(dtype)) for n, t in out.items()}


# ---- the two TF32-class cores of csrc/attention3.hip (f32 tensors in and out) ------------------------------------------------------------
def prod_h16(a, b):
    """one half product: both operands rounded to IEEE half, exact products, f32 accumulation (half8 / split_raw<true> / fill_two<.., true>
    convert, mma_rows3 / mma_seq3 issue one v_mfma_f32_32x32x16_f16 per K step)"""
    return hf(a) @ hf(b)


def split_bf16(t):
    hi = bf(t)
    return hi, bf(t - hi)


def prod_x3(a, b):
    """bf16x3: hi = bf16(x), lo = bf16(x - hi); lo*hi + hi*lo + hi*hi in f32 (split8 / pack8x3; the dropped lo*lo term and the 16 bits an
    operand keeps are 2^-16 per product, X3_TOL's class)"""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    return al @ bh + ah @ bl + ah @ bh


def core3_model(c, prod, S=1.0, defect=None, ctx_bwd=None):
    """float32 at the precision class of attention3.hip's kernels, `prod` = prod_h16 (the H16 instantiations) or prod_x3:
      forward   s = prod(q, k^T); m = rowmax(s); p = exp(alpha (s - m)) in f32; l = rowsum(p) over the UNROUNDED p (the kernels add the f32
                p before mma_seq3 converts it); ctx = prod(p, v) / l; lse = alpha m + log l
      backward  dsum = S (dO . O) in f32 from the f32 tensors (O: the f32 context, or ctx_bwd); p = exp(alpha s - lse);
                dS = p (prod(S dO, v^T) - dsum) in f32; dq = prod(dS, k) alpha / S, dk = prod(dS^T, q) alpha / S, dv = prod(p^T, S dO) / S
    S (a power of two) is the H16 backward's gradient scale (the bf16x3 kernels have none: S = 1).  Operands of an H16 case must be exact in
    bf16 and half (asserted; dO times S in half).  defect: "drop_last" / "leak_pad" as contract_model; "skip_middle" hides keys 256 .. 511 (the
    middle block of a 768-key stream); "no_unscale" leaves the 1 / S off dq, dk, dv; "dsum_unscaled" applies S to dO but not to dsum."""
    assert defect is None or defect in DEFECTS
    q, k, v, do = _operands(c, F32)
    if prod is prod_h16:
        assert_bf16_exact(q=q, k=k, v=v)
        assert_half_exact(q=q, k=k, v=v, do_scaled=do * S)
    B, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    a = float(c["alpha"])
    vis = None
    if defect == "drop_last":
        vis = torch.ones((Sq, Skv), dtype=torch.bool)
        vis[:, Skv - 1] = False
    if defect == "skip_middle":
        assert Skv == 768
        vis = torch.ones((Sq, Skv), dtype=torch.bool)
        vis[:, 256:512] = False
    if defect == "leak_pad":
        pad = torch.zeros_like(k[..., :1, :])
        k, v = torch.cat([k, pad], -2), torch.cat([v, pad], -2)
    s = prod(q, k.transpose(-1, -2))
    if vis is not None:
        s = s.masked_fill(~vis, -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp((s - m) * a)
    l = p.sum(-1, keepdim=True)
    ctx = prod(p, v) / l
    lse = m * a + torch.log(l)
    o = ctx if ctx_bwd is None else to_heads(ctx_bwd.to(F32), B, Sq, nh, hd)
    dos = do * S
    dsum = (do * o).sum(-1, keepdim=True) * (1.0 if defect == "dsum_unscaled" else S)
    pb = torch.exp(s * a - lse)
    ds = pb * (prod(dos, v.transpose(-1, -2)) - dsum)
    un = 1.0 if defect == "no_unscale" else 1.0 / S
    dq, dk, dv = prod(ds, k) * (a * un), prod(ds.transpose(-1, -2), q) * (a * un), prod(pb.transpose(-1, -2), dos) * un
    if defect == "leak_pad":
        dk, dv = dk[..., :Skv, :], dv[..., :Skv, :]
    out = {n: to_rows(t) for n, t in dict(ctx=ctx, dq=dq, dk=dk, dv=dv).items()}
    out["lse"] = lse.reshape(B * nh, Sq)
    return out


def model_h16(c, S=1.0, defect=None, ctx_bwd=None):
    return core3_model(c, prod_h16, S, defect, ctx_bwd)


def model_x3(c, defect=None, ctx_bwd=None):
    return core3_model(c, prod_x3, 1.0, defect, ctx_bwd)


# =====================================================================================================================================
# probe values
# =====================================================================================================================================
def _signed_pattern(idx, col, salt, mul, mod):
    """small non-zero signed integers [.., len(idx), len(col)]: ((mul idx + 3 col + 5 salt) mod `mod`) - mod // 2, the non-negative half moved
    up by one.  mul is coprime to mod, so neighbouring idx differ in every column."""
    x = (mul * idx[..., :, None] + 3 * col[None, :] + 5 * salt[..., None, None]) % mod - mod // 2
    return (x + (x >= 0)).to(F32)


def _values(B, S, nh, hd, mul, mod):
    salt = torch.arange(B * nh).reshape(B, nh)
    return to_rows(_signed_pattern(torch.arange(S).expand(B, nh, S), torch.arange(hd), salt, mul, mod))


V_MAX, DO_MAX = 7.0, 5.0


def probe_v(B, S, nh, hd):
    return _values(B, S, nh, hd, 7, 13)       # -6 .. -1, 1 .. 7


def probe_do(B, S, nh, hd):
    return _values(B, S, nh, hd, 5, 9)        # -4 .. -1, 1 .. 5


def _digits(j):
    return j >> 8, (j >> 4) & 15, j & 15


def address_scale(alpha):
    """c': the smallest power of two with alpha c' >= 32"""
    return 2.0 ** math.ceil(math.log2(32.0 / alpha))


def address_probe(B, Sq, Skv, nh, hd, targets, alpha=None, causal=False):
    """targets: int64 [B, nh, Sq], the key each query is aimed at.  The nine feature columns start at column (3 h + b) mod (hd - 8) of
    head h in image b; every other column of q and k is 0."""
    assert Skv <= 4096 and hd >= 9 and targets.shape == (B, nh, Sq) and int(targets.min()) >= 0 and int(targets.max()) < Skv
    alpha = default_alpha(hd) if alpha is None else alpha
    cp = address_scale(alpha)
    a, b, c = _digits(torch.arange(Skv))
    kf = torch.stack([a, b, c, a * a, b * b, c * c, torch.ones_like(a), torch.ones_like(a), torch.ones_like(a)], -1).to(F32)
    ta, tb, tc = _digits(targets)
    one = torch.ones_like(ta)
    qf = cp * torch.stack([2 * ta, 2 * tb, 2 * tc, -one, -one, -one, -ta * ta, -tb * tb, -tc * tc], -1).to(F32)
    q, k = torch.zeros((B, nh, Sq, hd)), torch.zeros((B, nh, Skv, hd))
    for bi in range(B):
        for h in range(nh):
            off = (3 * h + bi) % (hd - 8)
            q[bi, h, :, off:off + 9] = qf[bi, h]
            k[bi, h, :, off:off + 9] = kf
    q, k, v, do = to_rows(q), to_rows(k), probe_v(B, Skv, nh, hd), probe_do(B, Sq, nh, hd)
    assert_bf16_exact(q=q, k=k, v=v, do=do)
    assert float(cp) * 2000 < 2 ** 24                     # every partial sum of a score is an integer below 2^24
    return make_case(B, Sq, Skv, nh, hd, q, k, v, do, alpha=alpha, causal=causal, targets=targets, probe="address")


def _scatter_to_keys(c, rows):
    """[B * Sq, H] -> [B * Skv, H]: the sum of the query rows aimed at each key"""
    B, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    idx = c["targets"][..., None].expand(B, nh, Sq, hd)
    return to_rows(torch.zeros((B, nh, Skv, hd)).scatter_add_(2, idx, to_heads(rows, B, Sq, nh, hd).contiguous()))


def address_expected(c):
    """ctx = v[target] and dv = the scatter-sum of dO over the targets, exact (small integers), as row tensors"""
    B, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    idx = c["targets"][..., None].expand(B, nh, Sq, hd)
    return to_rows(torch.gather(to_heads(c["v"], B, Skv, nh, hd), 2, idx)), _scatter_to_keys(c, c["do"])


def address_leak_bounds(c):
    """what the keys beside the target may contribute: each has p <= e^-(alpha c') <= e^-32 (times one bf16 rounding), |dp - dsum| <=
    2 hd max|dO| max|v|, |k| <= 225, |q| <= 225 c'.  The target's own dS is exactly 0 (p = 1, dp = dsum = dO . v[t], integers)."""
    a, cp = float(c["alpha"]), address_scale(c["alpha"])
    e = math.exp(-a * cp) * (1 + 2 * BF16_ULP)
    d = 2 * c["hd"] * V_MAX * DO_MAX * (1 + 2 * BF16_ULP)
    return dict(ctx=e * c["Skv"] * V_MAX, dv=e * c["Sq"] * DO_MAX, dq=a * c["Skv"] * e * d * 225.0, dk=a * c["Sq"] * e * d * 225.0 * cp)


def address_leak_bounds_h16(c, S):
    """address_leak_bounds for the H16 core.  Every key beside the target has p <= e^-32 (f32, one rounding of exp2's argument and result:
    1 + 2^-20), which is 0 as a half: NOTHING leaks into P V or into dV.  dS is rounded to half AFTER the product with dP - dsum, in
    the scaled domain: |S dS| <= x = e^-32 S 2 hd max|dO| max|v| becomes 0 when x <= 2^-25 and at most x (1 + 2^-11) + 2^-25 otherwise (a
    half subnormal is off by up to half its spacing); the results are divided by S again.  The target's own dS is exactly 0."""
    a, cp = float(c["alpha"]), address_scale(c["alpha"])
    x = math.exp(-a * cp) * (1 + 2.0 ** -20) * 2 * c["hd"] * V_MAX * DO_MAX * S
    ds = 0.0 if x <= HALF_SUB_HALF else (x * (1 + HALF_ULP) + HALF_SUB_HALF) / S
    return dict(ctx=0.0, dv=0.0, dq=a * c["Skv"] * ds * 225.0, dk=a * c["Sq"] * ds * 225.0 * cp)


def uniform_probe(B, Sq, Skv, nh, hd, seed, alpha=None, rnd=bf):
    g = torch.Generator().manual_seed(seed)
    H = nh * hd
    q, k = torch.zeros((B * Sq, H)), rnd(torch.randn((B * Skv, H), generator=g))
    v, do = probe_v(B, Skv, nh, hd), probe_do(B, Sq, nh, hd)
    assert_bf16_exact(q=q, k=k, v=v, do=do)
    return make_case(B, Sq, Skv, nh, hd, q, k, v, do, alpha=alpha, probe="uniform")


# ---- target maps ------------------------------------------------------------------------------------------------------------------
def _coprime_near(n, want):
    p = max(1, want % n) if n > 1 else 1
    while math.gcd(p, n) != 1:
        p += 1
    return p % n if n > 1 else 0


def address_maps(Sq, Skv, per_call):
    """-> list of int64 [per_call, Sq] target maps t(i) = (p i + r) mod Skv, p coprime to Skv.  Map 0 aims query 0 (the first query
    tile) at the last key, map 1 the last query (the last query tile); the others cover every key: one coprime stride when Sq >= Skv,
    contiguous blocks of Sq keys otherwise - as many calls as that takes."""
    i = torch.arange(Sq)
    maps = [(Skv - 1 - i) % Skv, (i - (Sq - 1) + (Skv - 1)) % Skv]
    if Sq >= Skv:
        for n, want in enumerate((7, 37, 101, 211)):
            maps.append((_coprime_near(Skv, want) * i + 5 * n + 3) % Skv)
    else:
        for r in range(0, Skv, Sq):
            maps.append((i + r) % Skv)
    n = 0
    while len(maps) % per_call:
        maps.append((_coprime_near(Skv, 11 + 6 * n) * i + n) % Skv)
        n += 1
    covered = torch.zeros(Skv, dtype=torch.bool)
    for t in maps:
        covered[t] = True
    assert bool(covered.all()) and int(maps[0][0]) == Skv - 1 and int(maps[1][Sq - 1]) == Skv - 1
    return [torch.stack(maps[j:j + per_call]) for j in range(0, len(maps), per_call)]


def causal_maps(S):
    """the causal kernel's maps: the diagonal t(i) = i (the mask edge), t(i) = 0, t(i) = 16 floor(i / 16) (the first key of the query's own
    tile), and `masked`: t(i) = i + 1, a key the mask hides (the last query, which has no key behind it, is aimed at itself)"""
    i = torch.arange(S)
    return dict(diagonal=i, first=torch.zeros_like(i), tile=16 * (i // 16), masked=torch.where(i + 1 < S, i + 1, i))


# =====================================================================================================================================
# checks (raise AssertionError)
# =====================================================================================================================================
def bf16_ulp(ref):
    return (ref.abs() * BF16_ULP).clamp(min=BF16_SUB)


def _worst(d, bound):
    return float(torch.where(d > 0, d / bound.clamp(min=1e-300), torch.zeros_like(d)).max()) if d.numel() else 0.0


def _finite(name, t):
    assert bool(torch.isfinite(t.float()).all()), f"{name}: non-finite output"


def mfma_slack(n, mag):
    """The MFMA's f32 accumulation is not correctly rounded: an addend far below the last place of the running sum can still move the sum
    by one unit in that place (the MI355X returns 4 - 2^-22 for 4 + (-1e-13), the probe's leakage).  A bf16 result of magnitude >= 1
    rounds that away; an f32 result, or a sum of integers that cancels to 0, keeps it.  Bound: one unit in the last place of the largest
    partial sum `mag` for each chained MFMA over the n rows summed - at most three per 16 rows (the bf16x3 kernels) - and 8 more for the
    merges of partial results."""
    return (3 * math.ceil(n / 16) + 8) * 2.0 ** -23 * mag


def check_address(c, out, tag="address", bf16_out=True, h16=None, ctx_slack=False):
    """out: dict of CPU row tensors, any subset of ctx, lse, dq, dk, dv.  Targets every query sees: ctx == v[target] bit for bit (an f32
    context: within mfma_slack), |lse| < 1e-5, dv within the leakage (+ mfma_slack) of the exact scatter-sum, dq / dk within the
    leakage of 0.  A map with hidden targets (causal, `masked`): ctx within one bf16 rounding (+ the leakage) of the float64 masked
    reference.
    h16 = the gradient scale S of a run of the H16 core: the other keys' P is 0 as a half, so ctx == v[target] AND dv == the scatter-sum
    bit for bit, dq / dk within address_leak_bounds_h16.  ctx_slack (the streamed H16 forward): the key blocks before the target's were
    added at the running maximum of their time - the nearest key of each with P = 1 - and scaled down by e^-32 or less when the target
    arrived, so the MFMA that adds v[target] finds that remainder in its C operand: ctx within mfma_slack, as an f32 bf16x3 context."""
    ctx_e, dv_e = address_expected(c)
    if h16 is None:
        lk = address_leak_bounds(c)
        lk["dv"] += mfma_slack(c["Sq"], float(_scatter_to_keys(c, c["do"].abs()).max()))   # (the largest per-key sum of |dO|)
    else:
        lk = address_leak_bounds_h16(c, h16)
    vis = visible(c["Sq"], c["Skv"], c["causal"])
    hidden = vis is not None and not bool(torch.gather(vis.expand(c["B"], c["nh"], -1, -1), 3, c["targets"][..., None]).all())
    for n in out:
        _finite(f"{tag} {n}", out[n])
    if "ctx" in out:
        got = out["ctx"]
        if hidden:
            ref = reference(c)["ctx"]
            d = (got.double() - ref).abs()
            w = _worst(d, bf16_ulp(ref) + lk["ctx"])
            assert w <= 1.0, f"{tag} ctx: {w:.3g} x (one bf16 rounding + leakage) from the float64 masked reference"
        elif not bf16_out and (h16 is None or ctx_slack):
            e = float((got.double() - ctx_e).abs().max())
            assert e <= mfma_slack(c["Skv"], V_MAX), f"{tag} ctx: max |ctx - v[target]| = {e:.3e}, allowed {mfma_slack(c['Skv'], V_MAX):.1e}"
        else:
            bad = (got.float() != ctx_e).any(-1)
            if bool(bad.any()):
                r = int(bad.nonzero()[0])
                raise AssertionError(f"{tag} ctx: {int(bad.sum())} of {bad.numel()} rows are not v[target]: max |ctx - v[target]| = "
                                     f"{float((got.double() - ctx_e).abs().max()):.3e}; row {r} holds {got[r, :4].tolist()} .., v[target] is "
                                     f"{ctx_e[r, :4].tolist()} ..")
    if "lse" in out and not hidden:
        e = float(out["lse"].double().abs().max())
        assert e < PROBE_LSE_TOL, f"{tag} lse: |lse| = {e:.3e}, expected 0"
    if "dv" in out:
        d = (out["dv"].double() - dv_e).abs()
        e, r = float(d.max()), int(d.amax(-1).argmax())
        assert e <= lk["dv"], (f"{tag} dv: {e:.3e} from the scatter-sum of dO (leakage bound {lk['dv']:.1e}) in {int((d > lk['dv']).sum())} elements; "
                               f"row {r} holds {out['dv'][r, :4].tolist()} .., the sum is {dv_e[r, :4].tolist()} ..")
    for n in ("dq", "dk"):
        if n in out:
            e = float(out[n].double().abs().max())
            assert e <= lk[n], f"{tag} {n}: |{n}| = {e:.3e}, leakage bound {lk[n]:.1e}"


def _rows_identical(t, B, S, nh, hd):
    h = to_heads(t, B, S, nh, hd)
    return bool((h == h[:, :, :1]).all())


def check_uniform(c, out, ref, e_ref_dq, bf16_out=True, tag="uniform", h16=False):
    """q = 0: |lse - log Skv| < 1e-5; ctx the column mean of v (one rounding to the output type; P = 1 and the integer sums are exact in any
    order, so with a bf16 kernel every query's row is the same bit pattern); dk exactly 0; dv the same for every key (bit for bit for a bf16
    kernel: p is one bf16 number, its products with small integers and their sums are exact) and within one rounding of p and one of the
    output of colsum(dO) / Skv; dq per element over its terms: 4 E_ref (the contract model on the uniform cases) + one bf16 rounding.
    The bf16x3 kernels (f32 results): X3_TOL of the terms instead.  h16 (the H16 core, f32 results): the forward's P = 1 is exact in
    half (ctx as for bf16), the backward's p = 1 / Skv is rounded to half once (2^-11 of every term of dv; v and S dO are integers, exact),
    dk exactly 0, dq 4 E_ref of the H16 model (e_ref_dq)."""
    B, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    for n in out:
        _finite(f"{tag} {n}", out[n])
    if "lse" in out:
        e = float((out["lse"].double() - math.log(Skv)).abs().max())
        assert e < PROBE_LSE_TOL, f"{tag} lse: |lse - log {Skv}| = {e:.3e}"

    def judge(n, extra_terms):
        d = (out[n].double() - ref[n]).abs()
        bound = extra_terms * ref["t_" + n] + (bf16_ulp(ref[n]) if bf16_out else 0.0)
        w = _worst(d, bound)
        assert w <= 1.0, f"{tag} {n}: {w:.3g} x its bound"
    if "ctx" in out:
        judge("ctx", 1e-6 if bf16_out or h16 else X3_TOL)                  # (bf16: P = 1 exactly, integer sums, an f32 reciprocal and product)
        if bf16_out:
            assert _rows_identical(out["ctx"], B, Sq, nh, hd), f"{tag} ctx: the queries of a head do not all hold the same row"
    if "dk" in out:
        assert not bool((out["dk"] != 0).any()), f"{tag} dk: not exactly 0 with q = 0"
    if "dv" in out:
        judge("dv", BF16_ULP + 1e-6 if bf16_out else HALF_ULP + 1e-6 if h16 else X3_TOL)        # (bf16: one rounding of p; 1e-6: exp and the f32 lse it reads)
        if bf16_out:
            assert _rows_identical(out["dv"], B, Skv, nh, hd), f"{tag} dv: the keys of a head do not all hold the same row"
    if "dq" in out:
        judge("dq", 4.0 * e_ref_dq if bf16_out or h16 else X3_TOL)


def measure(got, ref, scale):
    return float(((got.double() - ref).abs() / scale).max()) if ref.numel() else 0.0


def model_errors(c, ref=None, kinds=KINDS, model=contract_model):
    """E_ref of one case: the contract model (before its output rounding; model_h16 / model_x3: the f32 results) against float64, per
    output kind, over the terms"""
    ref = reference(c) if ref is None else ref
    m = model(c)
    return {n: measure(m[n], ref[n], 1.0 if n == "lse" else ref["t_" + n]) for n in kinds}


def check_random(c, out, ref, e_ref, tag="random", report=None):
    """|got - ref| <= 4 E_ref[kind] terms (+ one bf16 rounding of ref for a bf16 result), element by element; lse: 4 E_ref['lse'] absolute.
    e_ref: dict kind -> E_ref.  Prints the worst figures first; report (a dict) collects them."""
    fails = []
    for n in out:
        got = out[n]
        _finite(f"{tag} {n}", got)
        assert got.shape == ref[n].shape, (tag, n, got.shape, ref[n].shape)
        d = (got.double() - ref[n]).abs()
        if n == "lse":
            bound = torch.full_like(d, 4.0 * e_ref[n])
            err = float(d.max())
        else:
            bound = 4.0 * e_ref[n] * ref["t_" + n]
            err = measure(got, ref[n], ref["t_" + n])
            if got.dtype == BF:
                bound = bound + bf16_ulp(ref[n])
        w = _worst(d, bound)
        print(f"[attention_edges] {tag} {n} err={err:.3e} E_ref={e_ref[n]:.3e} err/bound={w:.3f}")
        if report is not None:
            report.setdefault(n, []).append((err, w))
        if w > 1.0:
            fails.append(f"{n}: {w:.3f} x its bound (4 * {e_ref[n]:.3e}" + (" + 1 bf16 ulp)" if got.dtype == BF else ")"))
    assert not fails, f"{tag}: " + "; ".join(fails)
