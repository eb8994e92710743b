"""GPU (-m gpu): the row kernels of the three encoder towers (csrc/clip_text.hip, t5_text.hip, clip_vision.hip) at the shapes their own
tests leave out: past the grid cap of the element-wise kernels (where the grid-stride loop wraps and `i % cols` / `i / F` see a wrapped
index), at every column count around a wave (64) and two (128), at row counts around the four-row block, the bf16 instantiation of the
causal softmax, buckets outside the relative-bias table, and the row-in-registers limit of the CLIP vision embedding.

Every bar is the one the project already set for the kernel in tests/test_gpu_clip_text.py, test_gpu_t5_text.py and
test_gpu_clip_vision.py (they have MI355X measurements behind them); this file adds shapes, not tolerances.  The norms are judged per
row - the error over that row's largest reference magnitude - so that one wrong row cannot hide behind another.

Outputs sit inside sentinel-filled allocations that must come back unchanged outside the tensor; inputs that a kernel promises not to
read (masked and pad columns of the causal softmax) hold NaN.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import clip_vision_cpu as CV

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
PAD = 64
SENTINEL = 7.0
UNSUPPORTED = -3
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])


def _ops():
    from muse import ops
    return ops


def _lib():
    from muse import _hip
    return _hip.lib(), _hip.stream(), _hip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(shape, dtype, body=None, fill=SENTINEL):
    """a contiguous device tensor of `shape` inside a larger allocation filled with `fill` -> (tensor view, intact()): intact() says
    whether the PAD elements in front of it and behind it still hold `fill`"""
    n = math.prod(shape)
    buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=DEV)
    t = buf[PAD:PAD + n].view(shape)
    if body is not None:
        t.copy_(body)

    def intact():
        g = torch.cat([buf[:PAD], buf[PAD + n:]])
        return bool(torch.isnan(g.float()).all()) if math.isnan(fill) else bool((g == fill).all())
    return t, intact


def ulps(got, want, mant):
    """|got - want| in units of the spacing of a `mant`-bit-mantissa format at want (tests/test_gpu_t5_text.py)"""
    one = torch.exp2(torch.floor(torch.log2(want.float().abs().clamp_min(1e-30))) - mant)
    return float(((got.float() - want.float()).abs() / one).max())


# =====================================================================================================================================
# element-wise kernels past their grid cap
# =====================================================================================================================================
QUICK_GELU_SHAPES = [(1, 1), (4, 63), (37, 200), (2049, 1024), (2731, 769)]       # 8192 blocks of 256 = 2048 x 1024 elements
GATED_GELU_SHAPES = [(1, 1), (3, 63), (37, 200), (1025, 1024), (1367, 769)]       # 4096 blocks of 256 = 1024 x 1024 elements


@DTYPES
@pytest.mark.parametrize("rows,cols", QUICK_GELU_SHAPES)
def test_bias_quick_gelu_past_the_grid(rows, cols, dtype):
    """v = x + b[col]; y = v sigmoid(1.702 v) in place: at most 1 ulp of the storage type from torch's f32 expression on the device.
    The last two shapes are one row and a few elements past the 8192-block grid: the bias differs per column, so a wrong `i % cols`
    after the wrap moves every element."""
    ops = _ops()
    assert (rows * cols > 8192 * 256) == (rows > 2000)
    g = gen(rows + cols)
    x, intact = guarded((rows, cols), dtype, (torch.randn((rows, cols), generator=g) * 3).to(dtype))
    b = (torch.randn(cols, generator=g) * 0.5 + torch.arange(cols) % 7 * 0.25).to(DEV)
    v = x.float() + b
    want = (v * torch.sigmoid(1.702 * v)).to(dtype)
    got = ops.bias_quick_gelu_(x, b)
    torch.cuda.synchronize()
    assert got is x and got.dtype == dtype and intact()
    u = ulps(got, want, 23 if dtype == F32 else 7)
    print(f"[tower_row_edges] bias_quick_gelu {rows} x {cols} {dtype}: {u:.2f} ulp from torch")
    assert u <= 1.0


@DTYPES
@pytest.mark.parametrize("rows,cols", GATED_GELU_SHAPES)
def test_gated_gelu_tanh_past_the_grid(rows, cols, dtype):
    """gelu_new(ab[:, :F]) * ab[:, F:]: the bits of F.gelu(a, approximate="tanh") * b on the device (the bar measured at 0 ulp).  The
    last two shapes are past the 4096-block grid: `i / F` and `i - r F` see the wrapped index."""
    lib, stream, _hip = _lib()
    assert (rows * cols > 4096 * 256) == (rows > 1000)
    ab = (torch.randn((rows, 2 * cols), generator=gen(rows * 3 + cols)) * 3).to(dtype).to(DEV)
    a, b = ab[:, :cols].float(), ab[:, cols:].float()
    want = (F.gelu(a, approximate="tanh") * b).to(dtype)
    y, intact = guarded((rows, cols), dtype)
    assert lib.muse_gated_gelu_tanh(ab.data_ptr(), y.data_ptr(), 0 if dtype == F32 else 1, rows, cols, stream) == 0
    torch.cuda.synchronize()
    assert intact()
    u = ulps(y, want, 23 if dtype == F32 else 7)
    print(f"[tower_row_edges] gated_gelu_tanh {rows} x {cols} {dtype}: {u:.2f} ulp from torch")
    assert u == 0.0
    assert torch.equal(_ops().gated_gelu_tanh(ab), y)


# =====================================================================================================================================
# the one-wave-per-row norms
# =====================================================================================================================================
NORM_COLS = [1, 3, 63, 64, 65, 127, 128, 129, 768, 1000]
NORM_ROWS = [1, 3, 4, 5, 9]
NORM_TOL = 2e-6             # of the row's largest |y| (tests/test_gpu_clip_text.py::test_layernorm_with_bias_kernel), + 2^-8 |y| in bf16
ROW_KINDS = ["n01", "1e3+n01", "constant", "one_large"]


def norm_input(rows, cols, seed):
    """row r is of kind ROW_KINDS[(r + rows) % 4]: N(0, 1); 1e3 + N(0, 1) (mean >> std); constant 3.0 (variance 0: every partial sum
    is exact, LayerNorm gives the bias alone); N(0, 1) with one element of 1e4.  Nine rows hold every kind twice."""
    g = gen(seed)
    x = torch.randn((rows, cols), generator=g)
    for r in range(rows):
        kind = ROW_KINDS[(r + rows) % 4]
        if kind == "1e3+n01":
            x[r] += 1e3
        elif kind == "constant":
            x[r] = 3.0
        elif kind == "one_large":
            x[r, (r * 37) % cols] = 1e4
    return x, 1.0 + 0.3 * torch.randn(cols, generator=g), 0.5 * torch.randn(cols, generator=g)


def check_rows(name, got, want, rows, cols):
    """per row: |error| <= NORM_TOL * the row's largest |reference| (+ one bf16 rounding of the reference for a bf16 result)"""
    assert got.shape == want.shape and bool(torch.isfinite(got.float()).all()), name
    d = (got.double().cpu() - want).abs()
    bound = NORM_TOL * want.abs().amax(-1, keepdim=True).expand_as(want)
    if got.dtype == BF:
        bound = bound + want.abs() * 2.0 ** -8
    ratio = torch.where(d > 0, d / bound.clamp(min=1e-300), torch.zeros_like(d))
    worst_f32 = float((d / want.abs().amax(-1, keepdim=True).clamp(min=1e-300)).max())
    kinds = [ROW_KINDS[(r + rows) % 4] for r in range(rows)]
    per_kind = {k: max(float(ratio[r].max()) for r in range(rows) if kinds[r] == k) for k in set(kinds)}
    print(f"[tower_row_edges] {name} {rows} x {cols} {str(got.dtype)[6:]}: err / row max {worst_f32:.2e}, err / bound "
          + " ".join(f"{k}={v:.3f}" for k, v in sorted(per_kind.items())))
    return per_kind


@DTYPES
@pytest.mark.parametrize("cols", NORM_COLS)
def test_layernorm_bias_rows(cols, dtype):
    """muse_layernorm_bias_fwd at 1 .. 1000 columns (below, at and over one and two waves' worth) and 1 .. 9 rows (every remainder of the
    four-row block) against F.layer_norm in float64.  cols = 1: x - mean = 0 and the output is the bias; the constant row likewise,
    exactly."""
    ops = _ops()
    worst = {}
    for rows in NORM_ROWS:
        x, w, b = norm_input(rows, cols, 31 * cols + rows)
        want = F.layer_norm(x.double(), (cols,), w.double(), b.double(), 1e-5)
        got = ops.layernorm_bias_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, dtype)
        assert got.dtype == dtype
        for k, v in check_rows("layernorm_bias_fwd", got, want, rows, cols).items():
            worst[k] = max(worst.get(k, 0.0), v)
        for r in range(rows):
            if ROW_KINDS[(r + rows) % 4] == "constant" or cols == 1:
                assert torch.equal(got[r].cpu(), b.to(dtype)), "a row without variance must give the bias alone"
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("cols", NORM_COLS)
def test_rmsnorm_bf16_rows(cols):
    """muse_rmsnorm_bf16_fwd (x rsqrt(mean(x^2) + eps) w -> bf16) over the same columns, rows and row kinds, against float64"""
    ops = _ops()
    worst = {}
    for rows in NORM_ROWS:
        x, w, _ = norm_input(rows, cols, 37 * cols + rows)
        xd = x.double()
        want = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
        got = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), 1e-6, BF)
        assert got.dtype == BF
        for k, v in check_rows("rmsnorm_bf16_fwd", got, want, rows, cols).items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert max(worst.values()) <= 1.0, worst


def test_layernorm_bias_refuses_weights_it_would_misread():
    """w and b go to the kernel as raw pointers: anything but contiguous f32 [cols] tensors is refused"""
    from muse._hip import MuseHipError
    ops = _ops()
    cols = 96
    x = torch.randn(5, cols, device=DEV)
    w, b = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
    wide = torch.ones(cols, 2, device=DEV)
    assert ops.layernorm_bias_fwd(x, w, b, 1e-5, F32).shape == (5, cols)
    for bad in (w.double(), w.to(BF), torch.ones(cols - 1, device=DEV), torch.ones(cols + 1, device=DEV), wide[:, 0], w.view(1, cols),
                torch.ones(2 * cols, device=DEV)):
        with pytest.raises(MuseHipError):
            ops.layernorm_bias_fwd(x, bad, b, 1e-5, F32)
        with pytest.raises(MuseHipError):
            ops.layernorm_bias_fwd(x, w, bad, 1e-5, BF)


# =====================================================================================================================================
# causal softmax, bf16
# =====================================================================================================================================
@pytest.mark.parametrize("S", [1, 7, 33, 77, 128])
def test_causal_softmax_bf16(S):
    """the bf16 instantiation of muse_causal_softmax_fwd, in place, NaN in the masked and pad columns of the input: those columns come
    back as exact zeros, no NaN anywhere, and every kept entry is within one bf16 ulp + 6.5 eps (eps = 2^-23: the f32 test's accounting
    of expf, the sum, 1 / sum and the product) of the float64 softmax of the bf16 inputs"""
    ops = _ops()
    ld, mats = (S + 7) & ~7, 5
    keep = torch.tril(torch.ones(S, ld, dtype=torch.bool))
    x = (torch.randn((mats, S, ld), generator=gen(S)) * 4).to(BF)
    x64 = x.double().masked_fill(~keep, float("-inf"))
    want = torch.softmax(x64, -1)
    xin, intact = guarded((mats, S, ld), BF, x.masked_fill(~keep, NAN).to(DEV), fill=NAN)
    got = ops.causal_softmax_(xin, mats, S, ld)
    torch.cuda.synchronize()
    assert got is xin and got.dtype == BF and intact()
    got = got.cpu()
    assert not bool(torch.isnan(got.float()).any())
    assert not bool(got.view(torch.int16)[:, ~keep].any()), "masked and pad columns are not exact +0"
    k = keep.expand_as(want)
    ulp = torch.exp2(torch.floor(torch.log2(want.clamp_min(1e-300))) - 7)
    bound = ulp + 6.5 * 2.0 ** -23 * want
    ratio = ((got.double() - want).abs() / bound)[k].max()
    print(f"[tower_row_edges] causal softmax bf16 S={S}: err / bound {float(ratio):.3f}")
    assert float(ratio) <= 1.0


# =====================================================================================================================================
# relative-position bias gather
# =====================================================================================================================================
@pytest.mark.parametrize("heads,n", [(1, 1), (3, 255), (3, 256), (16, 1023)])
def test_rel_bias_gather_exact_and_out_of_table(heads, n):
    """rel[h][t] = table[bucket[t]][h], exact; a bucket outside the table (-1, 32, a large id) gives 0"""
    lib, stream, _hip = _lib()
    buckets = 32
    g = gen(heads * n)
    table = torch.randn(buckets, heads, generator=g)
    bucket = torch.randint(0, buckets, (n,), generator=g)
    if n > 1:
        bucket[0], bucket[n // 2], bucket[n - 1] = -1, buckets, 2 ** 40 + 5
        bucket[1], bucket[n - 2] = 0, buckets - 1
    ok = (bucket >= 0) & (bucket < buckets)
    want = torch.where(ok[None, :], table[bucket.clamp(0, buckets - 1)].t(), torch.zeros(()))
    rel, intact = guarded((heads, n), F32)
    table_d, bucket_d = table.to(DEV), bucket.to(DEV)
    assert lib.muse_rel_bias_gather(table_d.data_ptr(), bucket_d.data_ptr(), rel.data_ptr(), heads, n, buckets, stream) == 0
    torch.cuda.synchronize()
    assert intact()
    assert torch.equal(rel.cpu().view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(_ops().rel_bias_gather(table_d, bucket_d), rel)


# =====================================================================================================================================
# CLIP vision: row normalisation and the embedding LayerNorm
# =====================================================================================================================================
@pytest.mark.parametrize("D", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("N", [1, 4, 5])
def test_l2_normalize_rows_edges(N, D):
    """x / ||x|| per row, out of place and in place, with the float multiplier and with the device log-multiplier, against float64 at
    the bar of tests/test_gpu_clip_vision.py (4 x torch's own f32 gap, at least 2^-24); from four rows on, row 2 is zero and becomes
    NaN - that row only"""
    ops = _ops()
    x = torch.randn(N, D, generator=gen(N * D + 1))
    zero = 2 if N >= 4 else None
    if zero is not None:
        x[zero] = 0.0
    live = [r for r in range(N) if r != zero]
    want = (x.double() / x.double().norm(dim=-1, keepdim=True))[live]
    ref = (x / x.norm(dim=-1, keepdim=True))[live]
    bar = 4.0 * max(CV.gap(ref, want), 2.0 ** -24)
    ls = torch.tensor([1.25], device=DEV)
    runs = [(dict(), 1.0), (dict(mult=3.0), 3.0), (dict(log_mult=ls), math.exp(1.25))]
    for kw, scale in runs:
        out, intact = guarded((N, D), F32)
        got = ops.l2_normalize_rows(x.to(DEV), out=out, **kw)
        torch.cuda.synchronize()
        assert got is out and intact()
        assert CV.gap(got[live], scale * want) <= bar, (kw, CV.gap(got[live], scale * want), bar)
        if zero is not None:
            assert bool(torch.isnan(got[zero]).all()) and not bool(torch.isnan(got[live]).any())
        y, intact = guarded((N, D), F32, x)
        assert ops.l2_normalize_rows(y, out=y, **kw) is y
        torch.cuda.synchronize()
        assert intact() and torch.equal(y.view(torch.int32), got.view(torch.int32)), "in place differs from out of place"


EMBED_H = [4, 252, 256, 260, 1024, 2044, 2048]     # 2048 = the row-in-registers limit; 260 / 2044: one vector past / short of a 256 group


def distinct_rows(T, H, seed):
    """the row-mapping probe of tests/test_gpu_clip_vision.py: LayerNorm weight 1 / bias 0, zero patch embeddings, a position table that
    is a permutation of distinct integers and a class embedding make every (b, t) row a known vector; re-drawn (deterministically) until
    the T rows and the decoy - pos[0] without the class token - are pairwise more than 0.1 apart"""
    for k in range(64):
        g = gen(seed + 1000 * k)
        pos = torch.randperm(T * H, generator=g).view(T, H).float()
        cls = torch.arange(H).flip(0).float() * float(T) + torch.randperm(H, generator=g).float()
        one, nil = torch.ones(H), torch.zeros(H)
        want, _ = CV.embed_ln(torch.zeros(T - 1, H), cls, pos, one, nil, 1e-5, 1)
        decoy, _ = CV.embed_ln(torch.zeros(T - 1, H), torch.zeros(H), pos, one, nil, 1e-5, 1)
        rows = torch.cat([want[:T], decoy[:1]])
        dist = (rows[:, None] - rows[None]).abs().amax(-1) + torch.eye(T + 1) * 9.0
        if float(dist.min()) > 0.1:
            return pos, cls, rows
    raise AssertionError("no probe with pairwise distinct rows")


@pytest.mark.parametrize("H", EMBED_H)
def test_clip_vision_embed_ln_edges(H):
    """muse_clip_vision_embed_ln at both ends of its width range and around its 256-column vector groups, T = 1 (no patch row at all), 2
    and 5, batch 1 and 3 (rows % 4 = 1, 2, 3): the bar of tests/test_gpu_clip_vision.py (4 x the gap of torch's own f32 F.layer_norm
    from float64) and its row-mapping probe"""
    ops = _ops()
    eps = 1e-5
    for T in (1, 2, 5):
        for B in (1, 3):
            g = gen(7 * T + H + B)
            patch, cls, pos = torch.randn(B * (T - 1), H, generator=g), torch.randn(H, generator=g), torch.randn(T, H, generator=g) * 0.5
            w, b = 1.0 + 0.3 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
            want, _ = CV.embed_ln(patch, cls, pos, w, b, eps, B)
            _, x32 = CV.embed_ln(patch, cls, pos, w, b, eps, B, F32)
            torch32 = F.layer_norm(x32, (H,), w, b, eps)
            got = ops.clip_vision_embed_ln(*(t.to(DEV) for t in (patch, cls, pos, w, b)), eps, B)
            assert got.dtype == F32 and got.shape == (B * T, H)
            bar, err = 4.0 * CV.gap(torch32, want), CV.gap(got, want)
            print(f"[tower_row_edges] embed_ln H={H} T={T} B={B}: torch f32-f64 gap {bar / 4:.3e} achieved {err:.3e} err / bar {err / bar:.2f}")
            assert err <= bar
            pos, cls, rows = distinct_rows(T, H, 11 * T + H)
            zero, one, nil = torch.zeros(B * (T - 1), H), torch.ones(H), torch.zeros(H)
            want, _ = CV.embed_ln(zero, cls, pos, one, nil, eps, B)
            got = ops.clip_vision_embed_ln(*(t.to(DEV) for t in (zero, cls, pos, one, nil)), eps, B).cpu().double()
            assert float((got - want).abs().max()) < 1e-4
            for bt in range(B * T):
                assert int((rows - got[bt]).abs().amax(-1).argmin()) == bt % T, bt


@pytest.mark.parametrize("H", [6, 2052])
def test_clip_vision_embed_ln_refuses_and_writes_nothing(H):
    """hidden not a multiple of 4, or one vector past the 2048 columns a wave holds in registers: MUSE_ERR_UNSUPPORTED, nothing written"""
    lib, stream, _hip = _lib()
    B, T = 2, 3
    t = lambda *s: torch.ones(*s, device=DEV)   # noqa: E731
    patch, cls, pos, w, b = t(B * (T - 1), H), t(H), t(T, H), t(H), t(H)
    y, intact = guarded((B * T, H), F32)
    code = lib.muse_clip_vision_embed_ln(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, T, H,
                                         1e-5, stream)
    torch.cuda.synchronize()
    assert code == UNSUPPORTED
    assert bool((y == SENTINEL).all()) and intact()
    with pytest.raises(_hip.MuseHipError):
        _ops().clip_vision_embed_ln(patch, cls, pos, w, b, 1e-5, B)
