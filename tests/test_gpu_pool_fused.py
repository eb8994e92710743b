"""GPU (-m gpu): the encoder's pooling and layout passes folded into their neighbours -
muse_conv2d_nhwc_gn_split2_pool (avg_pool2d(2, 2) + the next GroupNorm's statistics in the patch-slab convolution's epilogue) and
muse_conv_in_direct_nchw (conv_in staging its rows from the NCHW image) - against the routes they replace.

Tensors are compared bit for bit; the only tolerances are on f64 partial sums that the two routes add up in different groupings.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import weights as W

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from muse import ops
    return ops


def rnd(shape, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


POOL_CASES = [(2, 32, 32, 128, 128, True, True), (1, 16, 16, 512, 512, False, True), (3, 16, 48, 64, 132, True, False),
              (1, 64, 32, 256, 256, True, True), (2, 256, 256, 128, 128, True, True)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,res,gn", POOL_CASES)
def test_pooled_convolution_matches_convolution_then_pooling(B, H, W, Cin, Cout, res, gn):
    """muse_conv2d_nhwc_gn_split2_pool against muse_conv2d_nhwc_gn_split2 -> muse_avgpool2x2_nhwc_stats on the same seeded inputs: the
    pooled tensor bit for bit; the GroupNorm partials, summed over their chunks, within 1e-12 relative of the float64 group sums of
    the pooled tensor (test_avgpool_fused_groupnorm_stats' bound: the routes chunk the image differently, 64 pooled pixels per
    convolution tile here, 1024 per pooling block there).  Several channel chunks, image-border patches, a ragged Cout tile without
    statistics, two N tiles, the benched level-0 shape."""
    ops = _ops()
    x = rnd((B, H, W, Cin), 11, 1.5).to(DEV)
    gamma, beta = (1.0 + 0.2 * rnd((Cin,), 12)).to(DEV), (0.3 * rnd((Cin,), 13)).to(DEV)
    w = rnd((Cout, 3, 3, Cin), 14, 1.0 / math.sqrt(9 * Cin)).to(DEV)
    w_hi, w_lo = ops.split_bf16(w.contiguous())
    bias = rnd((Cout,), 15, 0.1).to(DEV)
    resid = rnd((B, H, W, Cout), 16).to(DEV) if res else None
    groups = 32 if gn else 0
    assert ops.conv_gn_split2_pool_ok(B, H, W, Cin, Cout, 3, groups)
    # statistics of x the way a producer leaves them
    from muse.ops import check, lib, stream
    nchunk = lib().muse_groupnorm_nchunk(H * W)
    part = torch.empty(B * nchunk * 32 * 2, dtype=torch.float64, device=DEV)
    hi = torch.empty(x.shape, dtype=torch.bfloat16, device=DEV)
    lo = torch.empty_like(hi)
    check(lib().muse_groupnorm_silu_nhwc_split(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                               part.data_ptr(), 0, B, H * W, Cin, 32, 1e-6, 1, stream()), "gn split")
    del hi, lo
    sc, sh = ops.groupnorm_scale_shift((part, nchunk), gamma, beta, B, H * W, Cin)
    full = ops.conv2d_nhwc_gn_split2(x, sc, sh, w_hi, w_lo, B, H, W, Cin, Cout, bias=bias, residual=resid, gn_groups=groups)
    ref = ops.avgpool2x2_nhwc(full, B, H, W, Cout, gn_groups=groups)
    del full
    got = ops.conv2d_nhwc_gn_split2_pool(x, sc, sh, w_hi, w_lo, B, H, W, Cin, Cout, bias=bias, residual=resid, gn_groups=groups)
    assert got.shape == (B, H // 2, W // 2, Cout) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    if gn:
        assert hasattr(ref, "_gn_stats")
        gpart, gchunk = got._gn_stats
        assert gchunk == (H * W) // 256
        ohw = (H // 2) * (W // 2)
        st = gpart.view(B, gchunk, 32, 2).sum(1).cpu()
        o = ref.cpu().double().view(B, ohw, 32, Cout // 32)
        e_s, e_q = rel_err(st[..., 0], o.sum((1, 3))), rel_err(st[..., 1], (o * o).sum((1, 3)))
        print(f"pooled partials vs f64 group sums: sum {e_s:.2e}, sum of squares {e_q:.2e}")
        assert e_s < 1e-12 and e_q < 1e-12
        # and the (partial, nchunk) pair drives the consumer's affine form with the POOLED pixel count
        g2, b2 = (1 + 0.1 * rnd((Cout,), 17)).to(DEV), (0.1 * rnd((Cout,), 18)).to(DEV)
        sa = ops.groupnorm_scale_shift(ref._gn_stats, g2, b2, B, ohw, Cout)
        sb = ops.groupnorm_scale_shift(got._gn_stats, g2, b2, B, ohw, Cout)
        assert rel_err(sb[0], sa[0]) < 1e-6 and rel_err(sb[1], sa[1]) < 1e-6
    else:
        assert not hasattr(got, "_gn_stats")


@pytest.mark.parametrize("env", [{}, {"MUSE_CONV_PERSIST_GRID": "3"}, {"MUSE_CONV_PERSIST_GRID": "8"},
                                 {"MUSE_CONV_PERSIST_TILES": "2"}])
def test_persistent_pooled_convolution_matches(env):
    """conv_slab_persist_kernel<true, true>: the cases above with the persistent kernel taking every shape it can (Cin <= 256) - one
    workgroup per CU, workgroups that walk many tiles across image and N-tile changes (grid 3, grid 8), k-tile workgroups.  The
    library reads its switches once per process, so the cases run in a child interpreter."""
    e = dict(os.environ, MUSE_CONV_PERSIST="1", MUSE_CONV_PERSIST_MIN="0")
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_pooled_convolution_matches_convolution_then_pooling"], capture_output=True, text=True, timeout=900, env=e)
    assert r.returncode == 0 and f"{len(POOL_CASES)} passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_launch_per_tile_pooled_convolution_matches():
    """the same cases with the persistent kernel switched off (what muse.TrainStep does around the tokenizer pass beside a step)"""
    ops = _ops()
    with ops.conv_persistent(False):
        for c in POOL_CASES:
            test_pooled_convolution_matches_convolution_then_pooling(*c)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 256, 256, 3, 128), (3, 10, 23, 3, 128), (1, 6, 300, 2, 128), (2, 8, 40, 4, 256),
                                            (2, 5, 7, 1, 32)])
def test_conv_in_from_nchw_is_bit_identical(B, H, W, Cin, Cout):
    """muse_conv_in_direct_nchw against muse_nchw_to_nhwc + muse_conv_in_direct: output and GroupNorm partials bit for bit (the
    arithmetic behind the staging loop is shared), at 256 x 256 and at widths that are no multiple of 16"""
    ops = _ops()
    x = rnd((B, Cin, H, W), 21).to(DEV)
    w = rnd((Cout, Cin, 3, 3), 22, 0.3)
    bias = rnd((Cout,), 23, 0.1).to(DEV)
    w4 = torch.zeros(Cout, 9, 4)
    w4[:, :, :Cin] = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)
    w4 = w4.to(DEV)
    groups = Cout // 4 if Cout // 4 in (32, 64) else 0
    for cpad in (4, 8):
        ref = ops.conv_in_direct(ops.nchw_to_nhwc(x, torch.float32, cpad), w4, B, H, W, Cin, cpad, Cout, bias=bias, gn_groups=groups)
        got = ops.conv_in_direct_nchw(x, w4, B, H, W, Cin, Cout, bias=bias, gn_groups=groups)
        assert torch.equal(got, ref)
        if groups:
            assert got._gn_stats[1] == ref._gn_stats[1] and torch.equal(got._gn_stats[0], ref._gn_stats[0])
        else:
            assert not hasattr(got, "_gn_stats")


class _CountingLib:
    """the native library with a count of the entry points called through it"""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("muse_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("persistent", [True, False])
def test_tokenizer_with_fused_pooling_and_layout(monkeypatch, persistent):
    """MaskGitVQGAN f16-256 (seeded weights) in bf16x3 mode on 16 seeded images, fuse_pool + conv_in_nchw on against both off: token
    ids identical; z within 1e-6 relative (the pooled tensors are the same bits, the next GroupNorm's f64 sums are added in another
    grouping: the bound the project accepts between two statistics routes, test_avgpool_fused_groupnorm_stats); with the switches on
    get_code calls neither pooling entry point nor muse_nchw_to_nhwc, and the pooled convolution four times (levels 0-3)."""
    import muse
    ops = _ops()
    cfg = W.VQGAN_F16
    v = muse.MaskGitVQGAN(**cfg)
    v.load_state_dict(W.fill_state_dict(W.vqgan_shapes(cfg), 600, "vqgan"))
    v.to(DEV).eval().set_compute_dtype("bf16x3")
    px = W.images(16, 256, 612).to(DEV)
    assert v.fuse_pool and v.conv_in_nchw          # the defaults
    counting = _CountingLib(ops.lib())
    with ops.conv_persistent(persistent):
        z1, _ = v._encode_nhwc(px)
        monkeypatch.setattr(ops, "lib", lambda: counting)
        ids1 = v.get_code(px)
        monkeypatch.undo()
        v.fuse_pool = v.conv_in_nchw = False
        z0, _ = v._encode_nhwc(px)
        off = _CountingLib(ops.lib())
        monkeypatch.setattr(ops, "lib", lambda: off)
        ids0 = v.get_code(px)
        monkeypatch.undo()
    c = counting.calls
    assert c.get("muse_conv2d_nhwc_gn_split2_pool", 0) == 4 and c.get("muse_conv_in_direct_nchw", 0) == 1, c
    assert not [k for k in c if k.startswith("muse_avgpool2x2_nhwc") or k == "muse_nchw_to_nhwc"], c
    assert off.calls.get("muse_avgpool2x2_nhwc_stats", 0) == 4 and off.calls.get("muse_nchw_to_nhwc", 0) == 1, off.calls
    assert "muse_conv2d_nhwc_gn_split2_pool" not in off.calls and "muse_conv_in_direct_nchw" not in off.calls
    assert torch.equal(ids1, ids0)
    e = rel_err(z1, z0)
    print(f"z, switches on vs off (persistent={persistent}): {e:.2e}")
    assert e < 1e-6
