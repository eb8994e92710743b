"""GPU (-m gpu): the transformer's row and token kernels (csrc/rowops.hip, uvit.hip, embed.hip, sampling.hip) per element / per row
at every dispatch edge, against float64 torch on the same rounded inputs and, for the random streams, tests/philox_cpu.py.

How the floating point bounds are made (profiles/row_edges.md has the table):
  * a point-wise kernel (softmax forward, cross-entropy gradient, GELU, GLU) is judged per element, a row kernel (the norms, softmax
    backward, the embedding gradient) per row: |error| divided by that row's own largest reference magnitude.  One wrong small element or
    one wrong row cannot hide behind a large neighbour, which max|a - b| / max|b| over the tensor allows;
  * the constants are not invented: E_REF[kernel] is the worst normalised error of torch's own float32 CPU implementation of the same
    operation on the same inputs against float64, measured by `python tests/test_gpu_row_edges.py` (no GPU needed: it walks the same
    case lists as the tests).  An f32 output may err by 4 * E_REF (a different summation tree, a few ulp of expf / erff / rsqrt); a
    bf16 output by that plus one bf16 ulp of the reference, max(2^-8 |ref|, 2^-133) - the second term is bf16's subnormal spacing,
    without which no implementation could meet the bound on the subnormal results of the exhaustive GELU sweep;
  * normalisers.  A plain relative error is meaningless where the result is a difference of two larger terms, so those are judged
    against the terms' magnitudes: the cross-entropy gradient (softmax - target) against softmax + target, gelu(x) = x/2 + x/2 erf
    against |x| and its derivative against 1 + |x| (the form of the bf16 bounds below).  Every normaliser carries an absolute floor of
    2^-102 = 2^-126 / 2^-24: below f32's smallest normal number a result has no relative precision left (or is flushed to zero), and
    that floor turns the loss into at most one unit of f32 relative precision;
  * the bf16 GELU approximation (common.h erf_rsqrt2<true>) has its own derived bound: 2^-8 |ref| + 0.5 |x| E with E = 1e-6 (the
    formula itself errs by 5.4e-7 in erf when evaluated in float32 over all finite bf16 inputs; the rest is room for the hardware
    reciprocal and exponential), and 2^-8 |ref| + E (1 + |x|) for the derivative.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import philox_cpu as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32

TINY = 2.0 ** -102          # absolute floor of every normaliser (see above)
BF16_SUB = 2.0 ** -133      # spacing of bf16 subnormals
F32_SUB = 2.0 ** -149       # spacing of f32 subnormals
GELU_E = 1e-6               # bf16 GELU approximation: 5.4e-7 (the formula in float32 arithmetic) + room for the hardware rcp / exp

# Worst normalised error of torch's float32 CPU implementation against float64 over the case lists below (E_ref), as printed by
# `python tests/test_gpu_row_edges.py`.  The bound of a kernel is 4 * E_REF[kernel] (+ one bf16 ulp for bf16 outputs).
E_REF = {                            # bound = 4 * E_ref; what sets E_ref
    "layernorm_fwd": 1.104e-04,      # 4.4e-04  the 1e3 + N(0, 1) row of the 33 x 4 input: an f32 mean of values near 1e3 against std 1
    "layernorm_mean": 8.832e-08,     # 3.5e-07  |mean error| over the row's largest |x|
    "layernorm_rstd": 1.047e-07,     # 4.2e-07  relative
    "layernorm_bwd_dx": 2.955e-04,   # 1.2e-03  the -1e3 + N(0, 1) row in bf16 (values 996 / 1000 / 1004), 4 columns
    "layernorm_bwd_dw": 1.279e-04,   # 5.1e-04  the same row; over the largest column sum of |dy|
    "norm_res_fwd": 3.580e-05,       # 1.4e-04
    "norm_res_bwd_dv": 5.937e-05,    # 2.4e-04
    "norm_res_bwd_dw": 6.223e-05,    # 2.5e-04  a lone constant row: torch's f32 mean of 260 threes is not 3
    "norm_adaln_fwd": 9.937e-06,     # 4.0e-05
    "norm_adaln_bwd_dv": 2.158e-06,  # 8.6e-06
    "norm_adaln_bwd_dw": 1.174e-05,  # 4.7e-05
    "norm_adaln_bwd_dss": 3.655e-06, # 1.5e-05
    "softmax_fwd": 6.386e-07,        # 2.6e-06  per element, relative: the spread-200 row (|x - max| 2^-24 in the exponent)
    "softmax_bwd": 1.595e-05,        # 6.4e-05  a nearly one-hot row: p (dp - sum p dp) cancels
    "cross_entropy_loss": 1.161e-07, # 4.6e-07  relative
    "cross_entropy_bwd": 1.586e-06,  # 6.3e-06  per element over gscale (softmax + target)
    "gelu_fwd": 2.465e-07,           # 9.9e-07  over |x|, every finite bf16 value below 2^127 (torch's f32 kernel overflows above)
    "gelu_bwd": 2.153e-07,           # 8.6e-07  over 1 + |x|
    "embed_bwd": 3.012e-07,          # 1.2e-06  128 rows added in sequence
}


def _ops():
    from muse import ops
    return ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed)) * scale


def rounded(t, dtype):
    """the tensor as the kernel sees it: rounded to its storage type"""
    return t.to(dtype)


def bf16_ulp(ref):
    return (ref.abs() * 2.0 ** -8).clamp(min=BF16_SUB)


def row_scale(ref):
    return ref.abs().amax(-1, keepdim=True).clamp(min=TINY).expand_as(ref)


def elem_scale(ref):
    return ref.abs() + TINY


def colsum_scale(dy, like):
    """normaliser of a weight gradient dw[c] = sum_r dy[r, c] xhat[r, c] (xhat = O(1)): the largest column sum of |dy|.  max|dw| would
    do for many rows, but a single constant row has xhat = 0 and dw = 0 exactly, which leaves nothing to divide by"""
    return dy.double().abs().sum(0).amax().clamp(min=TINY).expand_as(like)


def measure(got, ref, scale):
    return float(((got.double() - ref).abs() / scale).max()) if ref.numel() else 0.0


def check(name, got, ref, scale):
    """|got - ref| <= 4 E_ref scale (+ one bf16 ulp of ref for a bf16 result), element by element; prints the worst figures first"""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite output"
    e_ref = E_REF[name]
    d = (got.double() - ref).abs()
    bound = 4.0 * e_ref * scale
    if got.dtype == BF:
        bound = bound + bf16_ulp(ref)
    ratio = torch.where(d > 0, d / bound.clamp(min=1e-300), torch.zeros_like(d))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    err = measure(got, ref, scale) if got.dtype != BF else float("nan")
    print(f"[row_edges] {name} {str(got.dtype)[6:]} shape={tuple(got.shape)} err={err:.3e} E_ref={e_ref:.3e} err/bound={worst:.3f}")
    assert worst <= 1.0, f"{name}: error {worst:.3f} x its bound (4 * {e_ref:.3e}" + (" + 1 bf16 ulp)" if got.dtype == BF else ")")


# =====================================================================================================================================
# norm kernels
# =====================================================================================================================================
NORM_COLS = [4, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048, 2052, 3072, 3076, 4096]   # both sides of every NIT threshold
LN_EPS, NR_EPS = 1e-5, 1e-6


def norm_input(rows, cols, seed):
    """33 rows = a full 16-row block + a one-row block.  Row 0 is constant (variance 0; 3.0 so that every partial sum is exact in f32
    and the normalised row is exactly 0 in any summation order), rows 1 and 32 are +-1e3 + N(0, 1) (mean >> std: a one-pass variance
    loses the row), the others 2 N(0, 1).  rows == 1 keeps one of the three kinds, chosen by the seed."""
    x = randn((33, cols), seed, 2.0)
    x[0] = 3.0
    x[1] = 1e3 + randn((cols,), seed + 1)
    x[32] = -1e3 + randn((cols,), seed + 2)
    if rows == 1:
        return x[seed % 3:seed % 3 + 1].clone()
    return x[:rows].clone()


def ln_case(rows, cols, dx_t, dy_t, x_t, seed):
    x = rounded(norm_input(rows, cols, seed), x_t)
    return dict(x=x, w=1.0 + 0.1 * randn((cols,), 11), res=randn((rows, cols), 12), dy=rounded(randn((rows, cols), 13), dy_t),
                dres=randn((rows, cols), 14), y_t=dx_t)


def ln_ref(c, dt, with_res):
    """y = LN(x) w (+ res), dx = LN'(dy) + dres, dw in `dt` arithmetic (float64: the reference, float32: torch's own kernel for E_ref)"""
    x = c["x"].to(dt).requires_grad_(True)
    w = c["w"].to(dt).requires_grad_(True)
    y = F.layer_norm(x, (x.shape[1],), w, None, LN_EPS)
    y.backward(c["dy"].to(dt))
    return dict(y=(y + c["res"].to(dt) if with_res else y).detach(), dx=x.grad + c["dres"].to(dt), dw=w.grad,
                mean=x.detach().mean(-1), rstd=1.0 / torch.sqrt(x.detach().var(-1, unbiased=False) + LN_EPS),
                xmax=c["x"].double().abs().amax(-1))        # the mean of a row is judged against the row's largest magnitude


def ln_run(c):
    ops = _ops()
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    with_res = c["y_t"] == F32
    y, mean, rstd = ops.layernorm_fwd(x, w, LN_EPS, c["y_t"], residual=c["res"].to(DEV) if with_res else None)
    dw = torch.empty(x.shape[1], device=DEV)
    dx, dxb = ops.layernorm_bwd(c["dy"].to(DEV), x, w, mean, rstd, c["y_t"], dw, False, dres=c["dres"].to(DEV), also_bf16=True)
    return dict(y=y, dx=dx, dxb=dxb, dw=dw, mean=mean, rstd=rstd), with_res


def ln_check(c):
    out, with_res = ln_run(c)
    ref = ln_ref(c, torch.float64, with_res)
    check("layernorm_fwd", out["y"], ref["y"], row_scale(ref["y"]))
    check("layernorm_mean", out["mean"], ref["mean"], ref["xmax"])
    check("layernorm_rstd", out["rstd"], ref["rstd"], elem_scale(ref["rstd"]))
    check("layernorm_bwd_dx", out["dx"], ref["dx"], row_scale(ref["dx"]))
    check("layernorm_bwd_dw", out["dw"], ref["dw"], colsum_scale(c["dy"], ref["dw"]))
    assert torch.equal(out["dxb"], out["dx"].to(BF)), "the bf16 copy of dx is not dx rounded to bf16"
    if float(c["x"][0].float().std()) == 0.0:                      # the constant row: exactly 0 (+ the residual), not merely small
        assert torch.equal(out["y"][0].cpu(), c["res"][0] if with_res else torch.zeros_like(c["res"][0], dtype=c["y_t"]))


LN_WIDTH_CASES = [(r, cols, t) for cols in NORM_COLS for t in (F32, BF) for r in (1, 33)]
LN_KEY_COLS = 772                                                     # NIT = 4, one vector past the 768 threshold
LN_KEY_CASES = [(dy_t, x_t, dx_t) for dy_t in (F32, BF) for x_t in (F32, BF) for dx_t in (F32, BF)]


def ln_all_cases():
    for i, (rows, cols, t) in enumerate(LN_WIDTH_CASES):
        yield ln_case(rows, cols, t, t, t, 100 + i)
    for i, (dy_t, x_t, dx_t) in enumerate(LN_KEY_CASES):
        yield ln_case(33, LN_KEY_COLS, dx_t, dy_t, x_t, 300 + i)


@pytest.mark.parametrize("t", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", NORM_COLS)
def test_layernorm_every_width(cols, t):
    """ln_fwd_kernel and every NIT instance of ln_bwd_kernel (1, 2, 3, 4, 8, 12, 16; 16 holds exactly 64 KiB of LDS), on and one vector
    past each threshold, 1 row and 16 + 1 rows, with dres, per row: a wrong threshold drops the columns past it, a one-pass variance
    loses the 1e3 + N(0, 1) rows"""
    for i, (rows, c_, t_) in enumerate(LN_WIDTH_CASES):
        if c_ == cols and t_ == t:
            ln_check(ln_case(rows, cols, t, t, t, 100 + i))


@pytest.mark.parametrize("dy_t,x_t,dx_t", LN_KEY_CASES, ids=lambda t: str(t)[6:])
def test_layernorm_bwd_every_dtype_key(dy_t, x_t, dx_t):
    i = LN_KEY_CASES.index((dy_t, x_t, dx_t))
    ln_check(ln_case(33, LN_KEY_COLS, dx_t, dy_t, x_t, 300 + i))


def test_layernorm_bwd_without_dres():
    ops = _ops()
    c = ln_case(33, 516, F32, F32, F32, 77)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, w, LN_EPS, F32)
    dw = torch.empty(516, device=DEV)
    dx = ops.layernorm_bwd(c["dy"].to(DEV), x, w, mean, rstd, F32, dw, False)
    ref = ln_ref(c, torch.float64, False)
    check("layernorm_bwd_dx", dx, ref["dx"] - c["dres"].double(), row_scale(ref["dx"] - c["dres"].double()))


def nr_case(rows, cols, mode, seed):
    x = norm_input(rows, cols, seed)
    r = randn(x.shape, seed + 5, 0.5)
    if float(x[0].std()) == 0.0:
        r[0] = 0.0                                         # keeps the constant row constant after the residual add
    return dict(x=x, r=r, w=1.0 + 0.1 * randn((cols,), 3), dy=randn(x.shape, seed + 6), dpre=randn(x.shape, seed + 7), mode=mode)


def nr_norm(v, w, mode, eps=NR_EPS):
    if mode == 0:
        return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w
    return F.layer_norm(v, (v.shape[1],), w, None, eps)


def nr_ref(c, dt, bwd=True):
    v = (c["x"].to(dt) + c["r"].to(dt)).requires_grad_(True)
    w = c["w"].to(dt).requires_grad_(True)
    y = nr_norm(v, w, c["mode"])
    if not bwd:
        return dict(y=y.detach())
    y.backward(c["dy"].to(dt))
    return dict(y=y.detach(), dv=v.grad + c["dpre"].to(dt), dw=w.grad)


NR_CASES = [(rows, cols, mode) for cols in NORM_COLS + [4100] for mode in (0, 1) for rows in (1, 33)]


def nr_all_cases():
    for i, (rows, cols, mode) in enumerate(NR_CASES):
        yield nr_case(rows, cols, mode, 500 + i)


@pytest.mark.parametrize("mode", [0, 1], ids=["rms", "ln"])
@pytest.mark.parametrize("cols", NORM_COLS + [4100])
def test_norm_res_every_width(cols, mode):
    """muse_norm_res_fwd (register kernels NIT 1..4 up to 1024, the general kernel above; 4100 only exists there) and every instance of
    norm_res_bwd_kernel (1, 2, 4, 8, 16) with the residual and dpre, per row"""
    ops = _ops()
    for i, (rows, c_, m_) in enumerate(NR_CASES):
        if c_ != cols or m_ != mode:
            continue
        c = nr_case(rows, cols, mode, 500 + i)
        bwd = cols <= 4096
        ref = nr_ref(c, torch.float64, bwd)
        x, r, w = c["x"].to(DEV), c["r"].to(DEV), c["w"].to(DEV)
        y, pre = ops.norm_res_fwd(x, w, NR_EPS, mode, residual=r, want_pre=True)
        assert torch.equal(pre.cpu(), c["x"] + c["r"])
        check("norm_res_fwd", y, ref["y"], row_scale(ref["y"]))
        if bwd:
            dv, dw, dvb = ops.norm_res_bwd(c["dy"].to(DEV), pre, w, NR_EPS, mode, dpre=c["dpre"].to(DEV), also_bf16=True)
            check("norm_res_bwd_dv", dv, ref["dv"], row_scale(ref["dv"]))
            check("norm_res_bwd_dw", dw, ref["dw"], colsum_scale(c["dy"], ref["dw"]))
            assert torch.equal(dvb, dv.to(BF))


def adaln_case(mode):
    B, S, C = 2, 16, 512
    x = norm_input(33, C, 40 + mode)[:32]
    r = randn(x.shape, 46, 0.5)
    r[0] = 0.0
    return dict(x=x, r=r, w=1.0 + 0.2 * randn((C,), 63), ss=0.3 * randn((B, 2 * C), 64), dm=randn(x.shape, 65), dpre=randn(x.shape, 66),
                mode=mode, B=B, S=S, C=C)


def adaln_ref(c, dt):
    v = (c["x"].to(dt) + c["r"].to(dt)).requires_grad_(True)
    w, ss = c["w"].to(dt).requires_grad_(True), c["ss"].to(dt).requires_grad_(True)
    rows = ss.repeat_interleave(c["S"], 0)
    m = nr_norm(v, w, c["mode"]) * (1 + rows[:, :c["C"]]) + rows[:, c["C"]:]
    m.backward(c["dm"].to(dt))
    return dict(m=m.detach(), dv=v.grad + c["dpre"].to(dt), dw=w.grad, dss=ss.grad)


@pytest.mark.parametrize("mode", [0, 1], ids=["rms", "ln"])
def test_norm_adaln_512(mode):
    """the NIT = 2 instance of muse_norm_adaln_fwd / _bwd (cols 512): per row against float64, bit for bit against the two-kernel route"""
    ops = _ops()
    c = adaln_case(mode)
    B = c["B"]
    x, r, w, ss = c["x"].to(DEV), c["r"].to(DEV), c["w"].to(DEV), c["ss"].to(DEV)
    assert ops.norm_adaln_ok(x.shape[0], c["C"], B)
    m, v = ops.norm_adaln_fwd(x, w, ss, B, NR_EPS, mode, residual=r)
    ref = adaln_ref(c, torch.float64)
    check("norm_adaln_fwd", m, ref["m"], row_scale(ref["m"]))
    n, pre = ops.norm_res_fwd(x, w, NR_EPS, mode, residual=r, want_pre=True)
    assert torch.equal(v, pre) and torch.equal(m, ops.adaln_fwd(n, ss, B))
    mb, _ = ops.norm_adaln_fwd(x, w, ss, B, NR_EPS, mode, residual=r, out_dtype=BF)
    check("norm_adaln_fwd", mb, ref["m"], row_scale(ref["m"]))
    dv, dw, dss, dvb = ops.norm_adaln_bwd(c["dm"].to(DEV), v, w, ss, B, NR_EPS, mode, dpre=c["dpre"].to(DEV), also_bf16=True)
    check("norm_adaln_bwd_dv", dv, ref["dv"], row_scale(ref["dv"]))
    check("norm_adaln_bwd_dw", dw, ref["dw"], row_scale(ref["dw"]))
    check("norm_adaln_bwd_dss", dss, ref["dss"], row_scale(ref["dss"]))
    assert torch.equal(dvb, dv.to(BF))


def test_backward_norms_refuse_4100_columns_and_write_nothing():
    """cols > 4096 has no ln_bwd_kernel / norm_res_bwd_kernel instance: MUSE_ERR_UNSUPPORTED, no kernel launched"""
    from muse import _hip
    ops = _ops()
    rows, cols = 3, 4100
    x, dy, w = randn((rows, cols), 1).to(DEV), randn((rows, cols), 2).to(DEV), torch.ones(cols, device=DEV)
    st = torch.ones(rows, device=DEV)
    with pytest.raises(_hip.MuseHipError, match="unsupported"):
        ops.layernorm_bwd(dy, x, w, st, st, F32, torch.empty(cols, device=DEV), False)
    with pytest.raises(_hip.MuseHipError, match="unsupported"):
        ops.norm_res_bwd(dy, x, w, NR_EPS, 1)
    lib = _hip.lib()
    dx, dxb, part = torch.full((rows, cols), 7.0, device=DEV), torch.full((rows, cols), 7.0, device=DEV, dtype=BF), torch.full((1, cols), 7.0, device=DEV)
    code = lib.muse_layernorm_bwd(dy.data_ptr(), 0, x.data_ptr(), 0, w.data_ptr(), st.data_ptr(), st.data_ptr(), None, dx.data_ptr(), 0,
                                  dxb.data_ptr(), part.data_ptr(), lib.muse_layernorm_bwd_nblk(rows), rows, cols, _hip.stream())
    assert code == -3
    code = lib.muse_norm_res_bwd_ex(dy.data_ptr(), None, x.data_ptr(), w.data_ptr(), dx.data_ptr(), dxb.data_ptr(), part.data_ptr(), rows,
                                    cols, NR_EPS, 1, _hip.stream())
    assert code == -3
    torch.cuda.synchronize()
    assert bool((dx == 7).all()) and bool((dxb == 7).all()) and bool((part == 7).all())


# =====================================================================================================================================
# softmax
# =====================================================================================================================================
SOFTMAX_SHAPES = [(1, 1, 8), (3, 63, 64), (5, 64, 64), (6, 65, 72), (2, 4097, 4104)]     # rows, cols, ld


def softmax_case(rows, cols, ld, t, seed):
    """row 0 carries -inf entries (exact zeros there), row 1 a spread of 200 (the small end underflows), row 2 an offset of 1e4"""
    x = randn((rows, cols), seed, 2.0)
    if cols > 1:
        x[0, 1::3] = -math.inf
    if rows > 1:
        x[1] = torch.linspace(0.0, -200.0, cols)[torch.randperm(cols, generator=gen(seed))]
    if rows > 2:
        x[2] = 1e4 + randn((cols,), seed + 1)
    x = rounded(x, t)
    p = rounded(torch.softmax(x.double(), -1), t)           # the probabilities the backward reads, in its storage type
    return dict(x=x, p=p, dp=rounded(randn((rows, cols), seed + 2), t), ld=ld, t=t)


def softmax_ref(c, dt):
    p, dp = c["p"].to(dt), c["dp"].to(dt)
    if dt == torch.float64:
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    else:
        ds = torch._softmax_backward_data(dp, p, -1, dt)
    return dict(y=torch.softmax(c["x"].to(dt), -1), ds=ds)


SOFTMAX_CASES = [(s, t) for s in SOFTMAX_SHAPES for t in (F32, BF)]


def softmax_all_cases():
    for i, ((rows, cols, ld), t) in enumerate(SOFTMAX_CASES):
        yield softmax_case(rows, cols, ld, t, 700 + i)


def padded(t, ld, fill=float("nan")):
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


@pytest.mark.parametrize("t", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,ld", SOFTMAX_SHAPES)
def test_softmax_per_element_in_place(rows, cols, ld, t):
    """forward per element (a wrong tail probability shows), backward per row, both in place; NaN in the pad columns [cols, ld) must
    not leak into the row and the pad comes back as exact zeros"""
    ops = _ops()
    c = softmax_case(rows, cols, ld, t, 700 + SOFTMAX_CASES.index(((rows, cols, ld), t)))
    ref = softmax_ref(c, torch.float64)
    y = ops.softmax_(padded(c["x"], ld).to(DEV), rows, cols, ld).cpu()
    assert bool((y[:, cols:] == 0).all()), "pad columns are not exact zeros"
    check("softmax_fwd", y[:, :cols], ref["y"], elem_scale(ref["y"]))
    assert bool((y[:, :cols][torch.isinf(c["x"].float())] == 0).all()), "-inf logits must give exact zeros"
    ds = ops.softmax_bwd_(padded(c["p"], ld).to(DEV), padded(c["dp"], ld).to(DEV), rows, cols, ld).cpu()
    assert bool((ds[:, cols:] == 0).all())
    check("softmax_bwd", ds[:, :cols], ref["ds"], row_scale(ref["ds"]))


# =====================================================================================================================================
# cross entropy
# =====================================================================================================================================
CE_SHAPES = [(1, 8), (63, 64), (65, 72), (2049, 2056)]   # V, ld
CE_DTYPES = [(F32, F32), (F32, BF), (BF, F32), (BF, BF)]  # logits, dlogits
CE_GOUT = 0.75


def ce_case(V, ld, rows, ls, lt, seed):
    x = randn((rows, V), seed)
    labels = torch.randint(0, V, (rows,), generator=gen(seed + 1))
    labels[0] = 0 if (seed + rows) % 2 == 0 or rows > 1 else V - 1
    if rows > 1:
        labels[1] = V - 1
        x[2, V // 2] = 1e4                 # outliers: the softmax of row 2 is one-hot, row 3 has an exact zero
        x[3, V // 3] = -1e4
        labels[4] = -100                   # an ignored row among valid ones
        labels[5] = V // 2
        x[5, V // 2] = 12.0                # a confident correct row: softmax - 1 cancels
    return dict(x=rounded(x, lt), labels=labels, ls=float(np.float32(ls)), V=V, ld=ld)


def ce_ref(c, dt):
    """-> loss, dlogits, and the normaliser of the gradient: gscale * (softmax + target), the magnitudes of the two terms it subtracts"""
    x = c["x"].to(dt).requires_grad_(True)
    loss = F.cross_entropy(x, c["labels"], ignore_index=-100, label_smoothing=c["ls"])
    (loss * CE_GOUT).backward()
    valid = c["labels"] >= 0
    n = int(valid.sum())
    tgt = torch.full(x.shape, c["ls"] / c["V"], dtype=torch.float64)
    tgt[valid, c["labels"][valid]] += 1.0 - c["ls"]
    mag = (torch.softmax(c["x"].double(), -1) + tgt) * valid[:, None] * (CE_GOUT / max(n, 1))
    return dict(loss=loss.detach().reshape(1), dl=x.grad, mag=mag + TINY, n=n)


CE_CASES = [(V, ld, lt, rows, ls) for (V, ld) in CE_SHAPES for lt in (F32, BF) for rows in (1, 7) for ls in (0.0, 0.1)]


def ce_all_cases():
    for i, (V, ld, lt, rows, ls) in enumerate(CE_CASES):
        yield ce_case(V, ld, rows, ls, lt, 900 + i)


@pytest.mark.parametrize("lt,dt", CE_DTYPES, ids=lambda t: str(t)[6:])
@pytest.mark.parametrize("V,ld", CE_SHAPES)
def test_cross_entropy_gradient_per_element(V, ld, lt, dt):
    """all four (logits, dlogits) instances of ce_bwd_kernel; labels 0 and V - 1, a +-1e4 outlier, label smoothing 0 and 0.1; the
    gradient of an unlikely class is judged against its own probability, not against the row's largest entry"""
    ops = _ops()
    for i, (V_, ld_, lt_, rows, ls) in enumerate(CE_CASES):
        if (V_, ld_, lt_) != (V, ld, lt):
            continue
        c = ce_case(V, ld, rows, ls, lt, 900 + i)
        ref = ce_ref(c, torch.float64)
        logits, labels = padded(c["x"], ld).to(DEV), c["labels"].to(DEV)
        loss_out, lse = ops.cross_entropy_fwd(logits, labels, c["ls"], vocab=V)
        assert float(loss_out[1]) == ref["n"]
        check("cross_entropy_loss", loss_out[:1], ref["loss"], elem_scale(ref["loss"]))
        dl = ops.cross_entropy_bwd(logits, labels, lse, loss_out, torch.tensor([CE_GOUT], device=DEV), c["ls"], dt, vocab=V).cpu()
        assert dl.dtype == dt and bool((dl[:, V:] == 0).all()), "pad columns of dlogits are not exact zeros"
        check("cross_entropy_bwd", dl[:, :V], ref["dl"], ref["mag"])
        assert bool((dl[c["labels"] < 0] == 0).all())


@pytest.mark.parametrize("lt,dt", CE_DTYPES, ids=lambda t: str(t)[6:])
def test_cross_entropy_all_rows_ignored(lt, dt):
    ops = _ops()
    V, ld, rows = 65, 72, 7
    logits = padded(rounded(randn((rows, V), 5), lt), ld).to(DEV)
    labels = torch.full((rows,), -100, dtype=torch.long, device=DEV)
    loss_out, lse = ops.cross_entropy_fwd(logits, labels, 0.1, vocab=V)
    assert math.isnan(float(loss_out[0])) and float(loss_out[1]) == 0.0          # 0 / 0, as torch
    dl = ops.cross_entropy_bwd(logits, labels, lse, loss_out, torch.ones(1, device=DEV), 0.1, dt, vocab=V)
    assert bool((dl.view(torch.int16 if dt == BF else torch.int32) == 0).all()), "dlogits of ignored rows must be exact +0, not NaN"


# =====================================================================================================================================
# GELU / GLU over every finite bf16 value
# =====================================================================================================================================
def all_finite_bf16():
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80].astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(BF)                   # 65280 values, subnormals and both zeros included


def gelu_ref(x, dt):
    """-> gelu(x), gelu'(x).  float64 uses erfc (no cancellation in the negative tail); float32 is torch's own kernel and its autograd"""
    x = x.to(dt)
    if dt == torch.float64:
        cdf = 0.5 * torch.special.erfc(-x * math.sqrt(0.5))
        return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    x = x.requires_grad_(True)
    y = F.gelu(x)
    y.backward(torch.ones_like(y))
    return y.detach(), x.grad


def gelu_check(name, got, ref, x, deriv):
    """bf16 storage: the derived bound of the approximation; f32 storage: 4 E_ref against |x| (1 + |x| for the derivative) + one f32
    subnormal.  For both: finite everywhere (x * x overflows for |x| > 1.8e19) and never positive left of zero"""
    got = got.detach().cpu().reshape(-1)
    xd = x.double().reshape(-1)
    assert bool(torch.isfinite(got.float()).all()), f"{name}: NaN / inf for a finite input"
    if not deriv:
        assert bool((got.float()[xd < 0] <= 0).all()), f"{name}: positive result for a negative input"
    scale = (1.0 + xd.abs()) if deriv else xd.abs()
    d = (got.double() - ref).abs()
    if got.dtype == BF:
        bound = bf16_ulp(ref) + (GELU_E if deriv else 0.5 * GELU_E) * scale
        e_txt = f"E={GELU_E:.1e}"
    else:
        bound = 4.0 * E_REF[name] * scale + F32_SUB
        e_txt = f"E_ref={E_REF[name]:.3e}"
    ratio = torch.where(d > 0, d / bound.clamp(min=1e-300), torch.zeros_like(d))
    worst = float(ratio.max())
    excess = float(((d - (bf16_ulp(ref) if got.dtype == BF else 0.0)).clamp(min=0) / scale.clamp(min=TINY)).max())
    key = name + ("_bf16" if got.dtype == BF else "")
    print(f"[row_edges] {key} err={excess:.3e} {e_txt} err/bound={worst:.3f} (at x = {float(xd[int(ratio.argmax())]):.6g})")
    assert worst <= 1.0, f"{key}: error {worst:.3f} x its bound at x = {float(xd[int(ratio.argmax())])!r}"


@pytest.mark.parametrize("t", [BF, F32], ids=["bf16", "f32"])
def test_gelu_every_finite_bf16_value(t):
    ops = _ops()
    x = all_finite_bf16()
    ref, dref = gelu_ref(x, torch.float64)
    xd = x.to(t).to(DEV)
    gelu_check("gelu_fwd", ops.gelu_fwd(xd), ref, x, False)
    gelu_check("gelu_bwd", ops.gelu_bwd(xd, torch.ones_like(xd)), dref, x, True)


@pytest.mark.parametrize("t", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("inter", [240, 4], ids=["wide8", "generic4"])
def test_glu_every_finite_bf16_value(inter, t):
    """h = gelu(a) * b with b = 1 and dab = (dh b gelu'(a), dh gelu(a)) with dh = 1 are GELU and its derivative themselves: the 8-wide
    bf16 kernels (inter % 8 == 0) and the generic ones (inter = 4) over every finite bf16 value of a"""
    ops = _ops()
    x = all_finite_bf16()
    ref, dref = gelu_ref(x, torch.float64)
    a = x.to(t).view(-1, inter)
    ab = torch.cat([a, torch.ones_like(a)], 1).contiguous().to(DEV)
    gelu_check("gelu_fwd", ops.glu_fwd(ab), ref, x, False)
    dab = ops.glu_bwd(ab, torch.ones(a.shape, dtype=t, device=DEV))
    gelu_check("gelu_bwd", dab[:, :inter].contiguous(), dref, x, True)
    gelu_check("gelu_fwd", dab[:, inter:].contiguous(), ref, x, False)


def test_glu_unaligned_view_takes_the_fallback_with_the_same_bits():
    """a bf16 view that is 8-byte but not 16-byte aligned cannot use the 16-byte accesses of glu_fwd8 / glu_bwd8: the generic kernel
    runs instead and gives the same bits"""
    ops = _ops()
    rows, inter = 5, 48
    ab = rounded(randn((rows, 2 * inter), 21, 2.0), BF).to(DEV)
    dh = rounded(randn((rows, inter), 22), BF).to(DEV)

    def shifted(t):
        buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
        v = buf[4:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8
        return v

    h, dab = ops.glu_fwd(ab), ops.glu_bwd(ab, dh)
    assert ab.data_ptr() % 16 == 0 and dh.data_ptr() % 16 == 0
    assert torch.equal(ops.glu_fwd(shifted(ab)), h)
    assert torch.equal(ops.glu_bwd(shifted(ab), dh), dab)
    assert torch.equal(ops.glu_bwd(ab, shifted(dh)), dab)


# =====================================================================================================================================
# dropout against the CPU Philox
# =====================================================================================================================================
DROPOUT_SEED = 0xDEADBEEFCAFEF00D


@pytest.mark.parametrize("t", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("offset", [0, 2 ** 32 - 2, 3 << 40], ids=["off0", "carry", "high"])
def test_dropout_matches_the_cpu_philox(offset, t):
    """keep masks, lane-to-element mapping, the 64-bit counter (2^32 - 2: the carry into counter word 1 falls inside the n = 1027
    tensor) and the arithmetic, bit for bit: y = x * fl32(1 / (1 - p)) where kept (rounded once more for bf16), +0 where dropped"""
    ops = _ops()
    bits = torch.int32 if t == F32 else torch.int16
    for n in (1, 3, 4, 5, 1027):
        x = rounded(randn((n,), 31 + n, 3.0), t)
        x[0] = -0.0 if n > 1 else x[0]
        for p in (0.0, 0.1, 0.5, 0.999):
            keep = torch.from_numpy(P.dropout_keep(n, p, DROPOUT_SEED, offset))
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
            exp = torch.where(keep, (x.float() * float(scale)).to(t), torch.zeros(n, dtype=t))
            y = ops.dropout(x.to(DEV), p, DROPOUT_SEED, offset)
            assert torch.equal(y.cpu().view(bits), exp.view(bits)), (n, p, offset)
            if p == 0.0:
                assert torch.equal(y.cpu().view(bits), x.view(bits))
            xi = x.to(DEV)
            assert ops.dropout(xi, p, DROPOUT_SEED, offset, out=xi) is xi and torch.equal(xi.view(bits), y.view(bits)), "in place differs"


# =====================================================================================================================================
# embedding backward
# =====================================================================================================================================
def embed_case(V, H=8, B=2, S=200):
    """ids with exactly 64, 65 and 128 hits (one, two and two full segments of SEG = 64), ids outside [0, V) that must be ignored"""
    g = gen(V)
    hot = {0: 64, V - 1: 65, V // 2: 128}
    ids = []
    for v, n in hot.items():
        ids += [v] * n
    ids += [-1, V, 2 ** 40]
    others = [v for v in range(1, V - 1) if v != V // 2]
    ids += [others[int(j)] for j in torch.randperm(len(others), generator=g)[:B * S - len(ids)]]     # every other id at most once
    ids = torch.tensor(ids)[torch.randperm(B * S, generator=g)].view(B, S)
    return dict(ids=ids, dout=randn((B * S, H), V + 1), V=V, H=H, B=B, S=S)


def embed_ref(c, dt):
    ids, dout = c["ids"].reshape(-1), c["dout"].to(dt)
    ok = (ids >= 0) & (ids < c["V"])
    dword = torch.zeros((c["V"], c["H"]), dtype=dt).index_add_(0, ids[ok], dout[ok])
    return dict(dword=dword, dpos=dout.view(c["B"], c["S"], c["H"]).sum(0))


EMBED_VOCABS = [1023, 1024, 1025]


def embed_all_cases():
    for V in EMBED_VOCABS:
        yield embed_case(V)


@pytest.mark.parametrize("V", EMBED_VOCABS)
def test_embed_bwd_scan_step_segments_and_bad_ids(V):
    """V on both sides of table_kernel's 1024-wide scan step; rows on both sides of the 64-hit segment; ids -1, V and 2^40 ignored"""
    ops = _ops()
    c = embed_case(V)
    flat = c["ids"].reshape(-1)
    counts = torch.bincount(flat[(flat >= 0) & (flat < V)], minlength=V)
    assert int(counts[0]) == 64 and int(counts[V - 1]) == 65 and int(counts[V // 2]) == 128
    dword, dpos = torch.full((V, c["H"]), 9.0, device=DEV), torch.full((c["S"], c["H"]), 9.0, device=DEV)
    ops.embed_bwd(c["ids"].to(DEV), c["dout"].to(DEV), dword, dpos, False)
    ref = embed_ref(c, torch.float64)
    check("embed_bwd", dword, ref["dword"], row_scale(ref["dword"]))
    check("embed_bwd", dpos, ref["dpos"], row_scale(ref["dpos"]))
    assert bool((dword[counts.to(DEV) == 0] == 0).all()), "rows without a hit must be exact zeros"


def test_embed_bwd_hidden_limit():
    from muse import _hip
    ops = _ops()
    B, S, V = 1, 8, 5
    ids = torch.tensor([[0, 4, 4, 2, 0, 4, 1, 0]])
    for H, ok in ((4096, True), (4100, False)):
        dout = randn((B * S, H), H)
        dword, dpos = torch.full((V, H), 9.0, device=DEV), torch.full((S, H), 9.0, device=DEV)
        if ok:
            ops.embed_bwd(ids.to(DEV), dout.to(DEV), dword, dpos, False)
            ref = torch.zeros((V, H), dtype=torch.float64).index_add_(0, ids.reshape(-1), dout.double())
            check("embed_bwd", dword, ref, row_scale(ref))
            assert torch.equal(dpos.cpu(), dout)
        else:
            with pytest.raises(_hip.MuseHipError, match="unsupported"):
                ops.embed_bwd(ids.to(DEV), dout.to(DEV), dword, dpos, False)
            torch.cuda.synchronize()
            assert bool((dword == 9).all()) and bool((dpos == 9).all())


# =====================================================================================================================================
# sample_step
# =====================================================================================================================================
@pytest.mark.parametrize("S", [2, 3, 257, 4096])
def test_sample_step_edges_vs_oracle(S):
    """supplied draws, bit-exact against oracle.maskgit_oracle.sample_step: an image without unknown tokens, one with exactly one,
    sched_mask_len >= S, and temperature 0 over duplicated rows (tied confidences among unknown tokens)"""
    from oracle import maskgit_oracle as O
    ops = _ops()
    B, V = 2, 8
    mask_id = V + 3
    g = gen(4000 + S)
    logits = torch.randn(B, S, V, generator=g) * 2.0
    q = torch.empty(B * S, V).exponential_(1, generator=g)
    u = torch.rand(B, S, generator=g)
    known = torch.randint(0, V, (B, S), generator=g)
    ids_a = torch.where(torch.rand(B, S, generator=g) < 0.7, torch.full((B, S), mask_id), known)
    ids_a[0] = known[0]                                     # image 0: nothing left to decode
    ids_b = known.clone()
    ids_b[0, S // 2] = mask_id                              # image 0: exactly one unknown token
    ids_b[1] = mask_id                                      # image 1: everything unknown, and sched_mask_len >= S below
    period = max(1, S // 4)
    dup = torch.arange(S) % period                          # rows repeat with this period: equal logits and equal draws -> equal confidences
    logits_c, q_c = logits[:, dup], q.view(B, S, V)[:, dup].reshape(B * S, V)
    ids_c = torch.full((B, S), mask_id)
    for name, lg, ids, qq, temperature, sched in (("none unknown", logits, ids_a, q, 1.3, S // 2), ("one unknown, sched >= S", logits, ids_b, q, 4.5, S + 5),
                                                  ("ties", logits_c, ids_c, q_c, 0.0, S // 2)):
        raw_o, samp_o, next_o = O.sample_step(lg, ids, mask_id, temperature, sched, qq, u)
        samp, nxt, raw = ops.sample_step(lg.contiguous().to(DEV), ids.to(DEV), mask_id, V, temperature, sched, noise_exp=qq.to(DEV),
                                         noise_u=u.to(DEV), want_raw=True)
        assert torch.equal(raw.cpu(), raw_o), name
        assert torch.equal(samp.cpu(), samp_o), name
        assert torch.equal(nxt.cpu(), next_o), name


def sample_replica(logits, seed, step):
    """the CPU restatement of the device-RNG categorical draw: float64 softmax, argmax of p / q with tests/philox_cpu.py's q.
    -> (choice [rows], exempt [rows]: the two largest p / q lie within 1e-3 relative, where f32 arithmetic may pick the other)"""
    rows, V = logits.shape
    p = torch.softmax(logits.double(), -1).numpy()
    v = p / P.sample_step_q(rows, V, seed, step)
    top = np.sort(v, -1)[:, -2:]
    return torch.from_numpy(v.argmax(-1)), torch.from_numpy((top[:, 1] - top[:, 0]) <= 1e-3 * top[:, 1])


def test_sample_step_device_rng_matches_the_cpu_philox():
    """the categorical draw of muse_sample_step without supplied noise, row by row against the CPU replica of its documented stream
    (counter (row, row >> 32, j, 2 step), key = seed): a swapped multiplier, counter word or key word changes nearly every row"""
    ops = _ops()
    B, S, V, seed, step = 4, 64, 64, 42, 3
    logits = randn((B, S, V), 8, 2.0)
    choice, exempt = sample_replica(logits.view(B * S, V), seed, step)
    assert int(exempt.sum()) <= (B * S) // 100, "too many near-ties in the chosen inputs: pick another seed"     # 1 of 256 here
    ids = torch.full((B, S), V + 1, dtype=torch.long, device=DEV)
    samp, _, raw = ops.sample_step(logits.to(DEV), ids, V + 1, V, 1.0, S // 2, seed=seed, step=step, want_raw=True)
    raw = raw.cpu().view(-1)
    assert torch.equal(raw[~exempt], choice[~exempt]), f"{int((raw != choice)[~exempt].sum())} of {B * S} rows differ"
    assert torch.equal(samp.cpu().view(-1), raw)


UNIT_DRAW = dict(B=1, S=256, V=512, seed=36, step=0, row=216, tok=502)


def unit_draw_rows(logit):
    """N(0, 1) logits with the logit of the token that draws u == 1 set to `logit` -> (raw samples of the kernel, replica's choice, exempt)"""
    ops = _ops()
    B, S, V, seed, step, row, tok = (UNIT_DRAW[k] for k in ("B", "S", "V", "seed", "step", "row", "tok"))
    assert int(P.sample_step_r0(S, V, seed, step)[row, tok]) >> 8 == 0xFFFFFF, "the reproducing draw moved: search again on the CPU"
    logits = randn((B, S, V), 9)
    logits[0, row, tok] = logit
    choice, exempt = sample_replica(logits.view(S, V), seed, step)
    assert not bool(exempt[row])
    ids = torch.full((B, S), V + 1, dtype=torch.long, device=DEV)
    _, _, raw = ops.sample_step(logits.to(DEV), ids, V + 1, V, 1.0, S // 2, seed=seed, step=step, want_raw=True)
    return raw.cpu().view(-1), choice, exempt


def test_sample_step_unit_draw_does_not_win():
    """seed 36, step 0, row 216, token 502 draws u == 1 (top 24 bits of the Philox word all ones), where q = -log(u) is no positive
    number.  With q = 2^-25 there, a token of probability e^-40 loses the row like it should"""
    row, tok = UNIT_DRAW["row"], UNIT_DRAW["tok"]
    raw, choice, exempt = unit_draw_rows(-40.0)
    assert int(choice[row]) != tok
    assert int(raw[row]) != tok, "the u == 1 draw wins the row whatever its probability"
    assert int(raw[row]) == int(choice[row])
    assert torch.equal(raw[~exempt], choice[~exempt])


def test_sample_step_unit_draw_keeps_its_probability():
    """the other side of the same draw: q = -logf(1.0f) is -0.0f, so p / q was -inf and the token could NOT be sampled whatever its
    probability (measured: the e^-40 case above passes on the unguarded kernel, this one does not).  With q = 2^-25 > 0 a token of
    probability ~1 wins the row, as in the replica"""
    row, tok = UNIT_DRAW["row"], UNIT_DRAW["tok"]
    raw, choice, exempt = unit_draw_rows(40.0)
    assert int(choice[row]) == tok
    assert int(raw[row]) == tok, "a u == 1 draw excludes its token from the row"
    assert torch.equal(raw[~exempt], choice[~exempt])


# =====================================================================================================================================
# E_ref: torch's float32 CPU kernels against float64 over the same cases (python tests/test_gpu_row_edges.py; no GPU)
# =====================================================================================================================================
def measure_e_ref():
    E = {}

    def put(name, got, ref, scale):
        E[name] = max(E.get(name, 0.0), measure(got, ref, scale))

    for c in ln_all_cases():
        with_res = c["y_t"] == F32
        r64, r32 = ln_ref(c, torch.float64, with_res), ln_ref(c, torch.float32, with_res)
        put("layernorm_fwd", r32["y"], r64["y"], row_scale(r64["y"]))
        put("layernorm_mean", r32["mean"], r64["mean"], r64["xmax"])
        put("layernorm_rstd", r32["rstd"], r64["rstd"], elem_scale(r64["rstd"]))
        put("layernorm_bwd_dx", r32["dx"], r64["dx"], row_scale(r64["dx"]))
        put("layernorm_bwd_dw", r32["dw"], r64["dw"], colsum_scale(c["dy"], r64["dw"]))
    for c in nr_all_cases():
        bwd = c["x"].shape[1] <= 4096
        r64, r32 = nr_ref(c, torch.float64, bwd), nr_ref(c, torch.float32, bwd)
        put("norm_res_fwd", r32["y"], r64["y"], row_scale(r64["y"]))
        if bwd:
            put("norm_res_bwd_dv", r32["dv"], r64["dv"], row_scale(r64["dv"]))
            put("norm_res_bwd_dw", r32["dw"], r64["dw"], colsum_scale(c["dy"], r64["dw"]))
    for mode in (0, 1):
        c = adaln_case(mode)
        r64, r32 = adaln_ref(c, torch.float64), adaln_ref(c, torch.float32)
        put("norm_adaln_fwd", r32["m"], r64["m"], row_scale(r64["m"]))
        for k in ("dv", "dw", "dss"):
            put("norm_adaln_bwd_" + k, r32[k], r64[k], row_scale(r64[k]))
    for c in softmax_all_cases():
        r64, r32 = softmax_ref(c, torch.float64), softmax_ref(c, torch.float32)
        put("softmax_fwd", r32["y"], r64["y"], elem_scale(r64["y"]))
        put("softmax_bwd", r32["ds"], r64["ds"], row_scale(r64["ds"]))
    for c in ce_all_cases():
        r64, r32 = ce_ref(c, torch.float64), ce_ref(c, torch.float32)
        put("cross_entropy_loss", r32["loss"], r64["loss"], elem_scale(r64["loss"]))
        put("cross_entropy_bwd", r32["dl"], r64["dl"], r64["mag"])
    x = all_finite_bf16()
    (y64, d64), (y32, d32) = gelu_ref(x, torch.float64), gelu_ref(x.float(), torch.float32)
    ok = torch.isfinite(y32)      # torch's f32 kernel forms x * (1 + erf) before halving it and overflows for x >= 2^127; left out of E_ref
    put("gelu_fwd", y32[ok], y64[ok], x.double().abs().clamp(min=TINY)[ok])
    put("gelu_bwd", d32, d64, 1.0 + x.double().abs())
    for c in embed_all_cases():
        r64, r32 = embed_ref(c, torch.float64), embed_ref(c, torch.float32)
        put("embed_bwd", r32["dword"], r64["dword"], row_scale(r64["dword"]))
        put("embed_bwd", r32["dpos"], r64["dpos"], row_scale(r64["dpos"]))
    return E


if __name__ == "__main__":
    torch.set_num_threads(8)
    for k, v in measure_e_ref().items():
        print(f'    "{k}": {v:.3e},')
    _, exempt = sample_replica(randn((256, 64), 8, 2.0), 42, 3)
    print("device-RNG near-ties:", int(exempt.sum()), "of 256 rows")
