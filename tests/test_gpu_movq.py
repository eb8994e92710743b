"""The MoVQ tokenizer on the GPU: the spatial-norm kernel of csrc/movq.hip against the float64 CPU restatement (tests/movq_cpu.py), and
muse.modeling_movq.MOVQ against the real reference's goldens (tests/golden/movq_*.npz, make_golden_movq.py) in both compute modes, plus
the shipped geometry against the restatement in float64."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import movq_cpu as P  # noqa: E402
import movq_weights as MW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).float().contiguous().to(DEV)


def nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2)


# ---- kernel: spatial_norm -----------------------------------------------------------------------------------------------------------
def _sn_inputs(B, H, W, C, zh, zw, Z, seed):
    """NCHW CPU tensors: x with a per-channel offset and spread (so the statistics matter), zq N(0,1), the modulation weights of a
    1x1 convolution (N / sqrt(Z), bias 1 + 0.1 N for conv_y - the scale sits around one - and 0.1 N for conv_b)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen)   # noqa: E731
    x = r(B, C, H, W) * (0.5 + torch.rand((1, C, 1, 1), generator=gen)) + r(1, C, 1, 1)
    return dict(x=x, zq=r(B, Z, zh, zw), gamma=1 + 0.1 * r(C), beta=0.1 * r(C), wy=r(C, Z) / math.sqrt(Z), by=1 + 0.1 * r(C),
                wb=r(C, Z) / math.sqrt(Z), bb=0.1 * r(C))


def _sn_want(t, silu, groups=32, shift=(0, 0)):
    d = {k: v.double() for k, v in t.items()}
    return P.spatial_norm(d["x"], d["zq"], d["gamma"], d["beta"], d["wy"], d["by"], d["wb"], d["bb"], groups=groups, silu=silu, shift=shift)


def _sn_gpu(t, silu, groups=32, split=False, stats=None, x_dev=None):
    from muse import ops
    B, C, H, W = t["x"].shape
    _, Z, zh, zw = t["zq"].shape
    w = [t[k].float().contiguous().to(DEV) for k in ("gamma", "beta", "wy", "by", "wb", "bb")]
    x = nhwc(t["x"]) if x_dev is None else x_dev
    return ops.spatial_norm(x, nhwc(t["zq"]), *w, B, H, W, C, zh, zw, groups=groups, eps=1e-6, silu=silu, stats=stats, split=split)


SN_SHAPES = [
    (1, 4, 6, 32, 4, 6, 4),        # factor 1
    (2, 8, 12, 64, 4, 6, 4),       # factor 2, two images with different zq
    (1, 16, 8, 128, 2, 1, 4),      # factor 8
    (1, 12, 8, 32, 3, 4, 4),       # factors 4 and 2 differ
    (1, 40, 36, 64, 10, 9, 4),     # 1440 pixels: a second, ragged 1024-pixel chunk whose boundary falls mid-row
    (1, 4, 4, 512, 2, 2, 4),       # widest shipped channel count
    (2, 8, 8, 64, 4, 4, 3),        # 12-byte zq rows
    (1, 4, 4, 32, 2, 2, 8),        # Z = 8
    (1, 6, 2, 1056, 3, 1, 4),      # more than 1024 channels: the kernel's other loop (a thread walks channel vectors); W no power of two
]
SHIPPED_SEED = 1800
SN_BAR = 2e-6   # of the output's largest magnitude: what test_groupnorm_silu_and_pool holds the f32 GroupNorm apply pass to


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("shape", SN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spatial_norm_against_float64(shape, silu):
    """f32 output against the float64 restatement: the GroupNorm apply (one fma) plus about ten f32 fmas of modulation per element"""
    t = _sn_inputs(*shape, seed=sum(shape))
    want = _sn_want(t, silu)
    got = nchw(_sn_gpu(t, silu))
    err = maxrel(got, want)
    print("spatial_norm", shape, "silu" if silu else "plain", "maxrel %.3e" % err)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert err < SN_BAR


def test_spatial_norm_groups_64():
    t = _sn_inputs(2, 8, 8, 128, 4, 4, 4, seed=64)
    assert maxrel(nchw(_sn_gpu(t, True, groups=64)), _sn_want(t, True, groups=64)) < SN_BAR


def test_spatial_norm_reads_the_right_source_pixel():
    """x4 / x2: zq holds a distinct value per source pixel, so a map that is one source pixel off along either axis is far from the true
    one; the kernel meets the bar of the test above against the true map"""
    B, H, W, C, zh, zw, Z = 1, 12, 8, 32, 3, 4, 4
    t = _sn_inputs(B, H, W, C, zh, zw, Z, seed=7)
    t["zq"] = (torch.arange(zh * zw, dtype=torch.float32).view(1, 1, zh, zw) - 5.5).repeat(B, Z, 1, 1) * torch.tensor([1.0, -0.5, 0.25, 2.0]).view(1, Z, 1, 1)
    want = _sn_want(t, True)
    for shift in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        assert maxrel(_sn_want(t, True, shift=shift), want) > 1e-2
    err = maxrel(nchw(_sn_gpu(t, True)), want)
    print("spatial_norm index map maxrel %.3e" % err)
    assert err < SN_BAR


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("shape", [(2, 8, 12, 64, 4, 6, 4), (1, 40, 36, 64, 10, 9, 4), (1, 16, 16, 128, 2, 2, 4), (1, 6, 2, 1056, 3, 1, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_spatial_norm_planes_output(shape, silu):
    """split=True writes the operand planes of conv2d_nhwc_split2.  They carry the hardware-reciprocal SiLU of the GroupNorm plane route
    while the tensor output keeps the correctly rounded division: the two agree to an f32 ulp before the split, so hi is the same bf16
    except at a rounding boundary and hi + lo reproduces the tensor to the split's 2^-16 (the two conditions test_gpu_kernels.py holds
    groupnorm_silu_nhwc_split to)"""
    from muse import ops
    t = _sn_inputs(*shape, seed=3 + sum(shape))
    y = _sn_gpu(t, silu)
    hi, lo = _sn_gpu(t, silu, split=True)
    assert hi.dtype == lo.dtype == torch.bfloat16 and hi.shape == y.shape == lo.shape
    assert float(((hi.float() + lo.float()) - y).abs().max()) <= 2.0 ** -15 * float(y.abs().max())
    e_hi, _ = ops.split_bf16(y)
    hi_diff = float((hi.view(torch.int16) != e_hi.view(torch.int16)).float().mean())
    print("spatial_norm planes", shape, "hi words differing: %.2e" % hi_diff)
    assert hi_diff < 5e-3
    if not silu:    # no reciprocal in the chain: the planes are the split of the tensor output, bit for bit
        e_lo = ops.split_bf16(y)[1]
        assert torch.equal(hi.view(torch.int16), e_hi.view(torch.int16)) and torch.equal(lo.view(torch.int16), e_lo.view(torch.int16))


def test_spatial_norm_takes_a_producers_statistics():
    """stats= from the epilogue of the convolution that produced x: the result agrees with the self-computed statistics up to the f64
    summation order.  128 channels: the narrowest output for which conv2d_nhwc_split2 leaves GroupNorm(32) statistics (its epilogue needs
    at least four channels per group, ops.conv_gn_stats_ok; at 64 channels it leaves none and there is nothing to hand over)"""
    from muse import ops
    B, H, W, C = 2, 16, 16, 128
    gen = torch.Generator().manual_seed(41)
    xin = torch.randn((B, H, W, C), generator=gen).to(DEV)
    w_hi, w_lo = ops.split_bf16((torch.randn((C, 3, 3, C), generator=gen) / math.sqrt(9 * C)).to(DEV))
    x_hi, x_lo = ops.split_f32(xin)
    x = ops.conv2d_nhwc_split2(x_hi, x_lo, w_hi, w_lo, B, H, W, C, C, bias=torch.randn(C, generator=gen).to(DEV), gn_groups=32)
    assert x._gn_stats[1] == H * W // 256
    t = _sn_inputs(B, H, W, C, 4, 4, 4, seed=42)
    for split in (False, True):
        a = _sn_gpu(t, True, split=split, x_dev=x)
        b = _sn_gpu(t, True, split=split, x_dev=x, stats=x._gn_stats)
        if split:
            a, b = a[0].float() + a[1].float(), b[0].float() + b[1].float()
        assert maxrel(b, a) < 1e-6
    t["x"] = nchw(x).cpu()
    assert maxrel(nchw(_sn_gpu(t, True, x_dev=x, stats=x._gn_stats)), _sn_want(t, True)) < SN_BAR


def test_spatial_norm_refusals():
    from muse import ops
    from muse._hip import MuseHipError, lib
    t = _sn_inputs(1, 8, 8, 64, 4, 4, 4, seed=1)
    w = [t[k].to(DEV) for k in ("gamma", "beta", "wy", "by", "wb", "bb")]
    x, zq = nhwc(t["x"]), nhwc(t["zq"])
    ok = ops.spatial_norm(x, zq, *w, 1, 8, 8, 64, 4, 4)
    with pytest.raises(MuseHipError):       # H % zh != 0
        ops.spatial_norm(x, nhwc(torch.zeros((1, 4, 3, 4))), *w, 1, 8, 8, 64, 3, 4)
    with pytest.raises(MuseHipError):       # Z = 9
        ops.spatial_norm(x, nhwc(torch.zeros((1, 9, 4, 4))), w[0], w[1], torch.zeros((64, 9), device=DEV), w[3], torch.zeros((64, 9), device=DEV), w[5],
                         1, 8, 8, 64, 4, 4)
    t48 = _sn_inputs(1, 8, 8, 48, 4, 4, 4, seed=2)
    with pytest.raises(MuseHipError):       # C = 48 with 32 groups
        ops.spatial_norm(nhwc(t48["x"]), zq, *[t48[k].to(DEV) for k in ("gamma", "beta", "wy", "by", "wb", "bb")], 1, 8, 8, 48, 4, 4)
    with pytest.raises(MuseHipError):       # bf16 x
        ops.spatial_norm(x.to(torch.bfloat16), zq, *w, 1, 8, 8, 64, 4, 4)
    with pytest.raises(MuseHipError):       # a transposed weight
        ops.spatial_norm(x, zq, w[0], w[1], w[2].t().contiguous().t(), w[3], w[4], w[5], 1, 8, 8, 64, 4, 4)
    # the entry point itself: both output forms, or neither, is a bad argument; nothing was launched (the stream is still healthy)
    y, part = torch.empty_like(x), torch.empty(64, dtype=torch.float64, device=DEV)
    hi, lo = torch.empty_like(x, dtype=torch.bfloat16), torch.empty_like(x, dtype=torch.bfloat16)
    base = [x.data_ptr()], [w[0].data_ptr(), w[1].data_ptr(), zq.data_ptr(), w[2].data_ptr(), w[3].data_ptr(), w[4].data_ptr(), w[5].data_ptr(),
                            part.data_ptr(), 0, 1, 8, 8, 64, 4, 4, 4, 32, 1e-6, 1, None]
    assert lib().muse_spatial_norm_nhwc(*base[0], y.data_ptr(), hi.data_ptr(), lo.data_ptr(), *base[1]) == -1
    assert lib().muse_spatial_norm_nhwc(*base[0], None, None, None, *base[1]) == -1
    assert lib().muse_spatial_norm_nhwc(*base[0], None, hi.data_ptr(), None, *base[1]) == -1
    torch.cuda.synchronize()
    assert torch.equal(ops.spatial_norm(x, zq, *w, 1, 8, 8, 64, 4, 4), ok)
    # an empty batch is no error
    assert lib().muse_spatial_norm_nhwc(*base[0], y.data_ptr(), None, None, *base[1][:9], 0, *base[1][10:]) == 0


# ---- the model against the reference goldens ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = MW.FIXTURES[name]
    seed, side = int(g["seed"]), cfg["resolution"]
    return g, cfg, MW.fill_movq(MW.movq_shapes(cfg), seed), MW.movq_images(int(g["batch"]), side, side, seed + 1), \
        MW.movq_images(1, *MW.NONSQUARE, seed + 2)


@pytest.mark.parametrize("cd", [torch.float32, "bf16x3"], ids=str)
@pytest.mark.parametrize("name", sorted(MW.FIXTURES))
def test_movq_vs_reference_golden(golden_dir, name, cd):
    from muse.modeling_movq import MOVQ
    g, cfg, sd, px, px_ns = _fixture(golden_dir, name)
    v = MOVQ(**cfg)
    v.load_state_dict(sd, strict=True)
    v.to(DEV).eval().set_compute_dtype(cd)
    px = px.to(DEV)
    z_rows, (B, H, W) = v._encode_nhwc(px)
    err_z = maxrel(nchw(z_rows.view(B, H, W, -1)), torch.from_numpy(g["z"]))
    enc = v.encode(px)
    assert len(enc) == 2
    z_q, idx = enc
    rec, rec_decode = v.decode_code(idx), v.decode(z_q)
    err_rec, err_dec = maxrel(rec, torch.from_numpy(g["rec"])), maxrel(rec_decode, torch.from_numpy(g["rec_decode"]))
    print(name, cd, "z %.3e rec %.3e rec_decode %.3e" % (err_z, err_rec, err_dec))
    assert err_z < (2e-5 if cd == torch.float32 else 1e-4)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == g["indices"].shape
    assert np.array_equal(idx.cpu().numpy(), g["indices"])              # bit-exact token indices (margin recorded in the fixture)
    assert np.array_equal(z_q.cpu().numpy(), g["z_q"])
    tol = 1e-4 if cd == torch.float32 else 2e-4        # the bars of test_taming_vqgan_vs_reference_golden (the same engine)
    assert err_rec < tol and err_dec < tol
    assert np.array_equal(v.get_code(px_ns.to(DEV)).cpu().numpy(), g["code_nonsquare"])
    assert torch.equal(v.get_code(px), idx)
    out = v(px)
    assert isinstance(out, tuple) and len(out) == 2
    assert torch.equal(out[0], rec_decode) and torch.equal(out[1], idx)
    if cd == "bf16x3":      # the decoder's 3x3 layers took the planes route
        from muse import ops
        ops.profile_start()
        v.decode_code(idx)
        names = [n for n, *_ in ops.profile_stop(with_kind=True)]
        # (every decoder norm of the fixtures runs: their attention levels hold num_res_blocks + 1 >= 2 blocks)
        assert names.count("spatial_norm") == sum(1 for k in sd if k.endswith("conv_y.weight"))
        assert "conv_bf16x3_dma" in names and "groupnorm_silu" not in names


def test_movq_shipped_geometry_bf16x3_against_float64():
    """hidden 128, multipliers (1, 2, 2, 4), 2 blocks per level, attention at resolution 32, 16384 codes on one 64 x 64 image: latent
    8 x 8, every factor x1 .. x8, channels 512 / 256 / 256 / 128, attention over 64 tokens.  Seed 1800: the f32 restatement picks the
    float64 indices on every token (checked on the CPU; smallest float64 relative gap of the squared distances 6.2e-3)."""
    from muse.modeling_movq import MOVQ
    cfg = MW.MOVQ_SHIPPED
    sd = MW.fill_movq(MW.movq_shapes(cfg), SHIPPED_SEED)
    px = MW.movq_images(1, 64, 64, SHIPPED_SEED + 1)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count()))
    try:
        with torch.no_grad():
            z64 = P.encoder(sd, cfg, px, torch.float64)
            idx64, d64 = P.nearest_code(z64, sd["quantize.embedding.weight"])
            rec64 = P.decode_code(sd, cfg, idx64, torch.float64)
    finally:
        torch.set_num_threads(threads)
    v = MOVQ(**cfg)
    v.load_state_dict(sd, strict=True)
    v.to(DEV).eval().half()
    assert v.compute_dtype == "bf16x3"
    z_rows, (B, H, W) = v._encode_nhwc(px.to(DEV))
    idx = v.get_code(px.to(DEV)).cpu()
    rec = v.decode_code(idx64.to(DEV))
    err_z, err_rec = maxrel(nchw(z_rows.view(B, H, W, -1)), z64), maxrel(rec, rec64)
    bad = (idx != idx64).view(-1)
    print("shipped geometry bf16x3: z %.3e rec %.3e index disagreements %d" % (err_z, err_rec, int(bad.sum())))
    assert (B, H, W) == (1, 8, 8) and tuple(rec.shape) == (1, 3, 64, 64)
    assert err_z < 1e-4 and err_rec < 3e-4
    ar = torch.arange(idx64.numel())
    best, got = d64[ar, idx64.view(-1)], d64[ar, idx.view(-1)]
    assert bool(((got - best)[bad] < 1e-3 * got[bad]).all()) and int(bad.sum()) <= 2

