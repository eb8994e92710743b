"""The dropped forms of the GLU and GlobalResponseNorm kernels (nn.Dropout of MaskGiTUViT's `hidden_dropout` applied inside the row
kernels: muse_glu_drop_fwd / _bwd / _fwd_x3 / _bwd_x3, muse_grn_drop_fwd_ex / muse_grn_drop_bwd), forward and backward, in every variant
the U-ViT calls: f32, bf16, operand planes next to the f32 result (bf16x3 step), operand image only (`planes_only`), the f16 step's half
image.

  * keep bits are exact: the zero pattern is philox_cpu's mask of (seed, offset) over the row-major [rows, cols] result, at p = 0.5 and
    0.1, offsets 3 << 40 and 2^32 - 5 (the block counter carries into its high word inside the tensor);
  * the f32 results of the GLU (both directions) and of GRN's forward are the bits of the two-pass composition (plain kernel, then
    muse_dropout on its result / on the incoming gradient): the dropped kernels add one f32 multiplication to the plain kernels'
    expressions.  GRN's backward is held to the float64 bounds only: its dx expression is free to contract differently around the
    extra multiplication;
  * values against float64 (tests/rowdrop_cpu.py, spatial_cpu's GRN references) are held to the bounds of the p = 0 tests of the same
    kernels: GLU 1e-6 forward / 2e-6 backward of the largest element in f32, 1e-2 in bf16 (test_gpu_kernels.test_softmax_glu_gelu);
    GRN per element spatial_cpu.bound_grn / bound_grn_bwd (test_gpu_spatial_edges), the forward's times the scale plus the one rounding
    of the extra multiplication;
  * shapes: rows 1, 63, 257 (one thread row, an odd count, more than one block at 8 columns), cols 8 and 2816 (config 4's
    intermediate_size), 256 rows for the operand-only forms (planes_only_ok wants whole 8-row groups); cols % 4 != 0 is refused by the
    entry points and served by ops through the two-pass route;
  * a thread's second trip through each GLU loop, plain and dropped: 2049 x 2052 and 2056 x 2048 (more four-column groups than the grid
    cap of 4096 x 256 threads), 16385 x 8 bf16 (one row more than the 8-wide kernels' 16384 blocks)."""
import numpy as np
import pytest
import torch

import rowdrop_cpu as R
import spatial_cpu as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
DROPS = [(0.5, 0x1234567, 3 << 40), (0.1, (1 << 61) + 99, 2 ** 32 - 5)]
SHAPES = [(rows, cols) for rows in (1, 63, 257) for cols in (8, 2816)]


def _ops():
    from muse import ops
    return ops


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def zeros_are(t, keep):
    """the zero pattern of a result whose undropped values are non-zero: exactly the dropped positions"""
    return bool(np.array_equal(t.detach().float().cpu().numpy() != 0.0, keep))


@pytest.mark.parametrize("rows,inter", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_glu_dropped(rows, inter, dtype):
    ops = _ops()
    ab, dh = rnd((rows, 2 * inter), 900 + rows).to(dtype), rnd((rows, inter), 901 + rows).to(dtype)
    abd, dhd = ab.to(DEV), dh.to(DEV)
    plain = ops.glu_fwd(abd)
    assert bool((plain != 0).all()) and bool((dh != 0).all())
    f32 = dtype == torch.float32
    for p, seed, offset in DROPS:
        keep, m = R.keep_mask(rows, inter, p, seed, offset), R.mult(rows, inter, p, seed, offset)
        h = ops.glu_fwd(abd, drop=(p, seed, offset))
        assert h.dtype == dtype and zeros_are(h, keep), (p, offset)
        e = rel_err(h, R.glu_drop_fwd(ab.float().numpy(), m))
        print(f"glu_drop_fwd {rows}x{inter} {dtype} p {p}: {e:.2e}")
        assert e < (1e-6 if f32 else 1e-2)
        dab = ops.glu_bwd(abd, dhd, drop=(p, seed, offset))
        assert dab.dtype == dtype and zeros_are(dab, np.concatenate([keep, keep], axis=1)), (p, offset)
        e = rel_err(dab, R.glu_drop_bwd(ab.float().numpy(), dh.float().numpy(), m))
        print(f"glu_drop_bwd {rows}x{inter} {dtype} p {p}: {e:.2e}")
        assert e < (2e-6 if f32 else 1e-2)
        if f32:
            assert torch.equal(h, ops.dropout(plain, p, seed, offset))
            assert torch.equal(dab, ops.glu_bwd(abd, ops.dropout(dhd, p, seed, offset)))


def test_glu_dropped_p0_keeps_everything_and_bad_arguments_are_refused():
    ops = _ops()
    from muse import _hip
    L = _hip.lib()
    ab, dh = rnd((63, 16), 910).to(DEV), rnd((63, 8), 911).to(DEV)
    assert torch.equal(ops.glu_fwd(ab, drop=(0.0, 5, 1 << 40)), ops.glu_fwd(ab))
    assert torch.equal(ops.glu_bwd(ab, dh, drop=(0.0, 5, 1 << 40)), ops.glu_bwd(ab, dh))
    with pytest.raises(ValueError):
        ops.glu_fwd(ab, drop=(1.0, 5, 0))
    # inter % 4 != 0: the entry points refuse before a launch, ops serves the width through the plain kernel and muse_dropout
    ab6, dh6 = rnd((5, 12), 912).to(DEV), rnd((5, 6), 913).to(DEV)
    out = torch.full((5, 6), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert L.muse_glu_drop_fwd(ab6.data_ptr(), out.data_ptr(), 0, 5, 6, 0.5, 1, 0, st) == -3          # MUSE_ERR_UNSUPPORTED
    assert L.muse_glu_drop_bwd(ab6.data_ptr(), dh6.data_ptr(), out.data_ptr(), 0, 5, 6, 0.5, 1, 0, st) == -3
    assert L.muse_glu_drop_fwd(ab.data_ptr(), out.data_ptr(), 0, 5, 8, 1.0, 1, 0, st) == -1           # MUSE_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("rows,inter", SHAPES + [(256, 128), (256, 2816)])
def test_glu_dropped_operand_images_are_the_split_or_cast_of_the_f32_result(mode, rows, inter):
    """inside a bf16x3 / f16 step the dropped GLU writes the operand image of its DROPPED result (and of the dropped gradient's d(ab))
    next to the f32 tensor, or alone (planes_only, the route config 4's feed-forward takes): bit for bit the split / half cast of the
    f32 result of the same call outside a step"""
    ops = _ops()
    ab, dh = rnd((rows, 2 * inter), 920 + rows).to(DEV), (rnd((rows, inter), 921 + rows) * 1e-3).to(DEV)
    p, seed, offset = DROPS[1]
    h0, dab0 = ops.glu_fwd(ab, drop=(p, seed, offset)), ops.glu_bwd(ab, dh, drop=(p, seed, offset))
    gs = 2.0 ** 10
    for bwd in (False, True):
        if mode == "f16":
            im = ops.F16Images()
            im.backward = bwd
            im.set_grad_scale(gs)
            scope = ops.f32_gemms_as_f16(True, im)
        else:
            im = ops.X3Images()
            im.backward = bwd
            scope = ops.f32_gemms_as_bf16x3(True, im)
        want = dab0 if bwd else h0
        scale = gs if (bwd and mode == "f16") else 1.0
        image = (lambda t: ops.cast_to_f16(t, scale)) if mode == "f16" else ops._split_planes_now
        with scope:
            got = ops.glu_bwd(ab, dh, drop=(p, seed, offset)) if bwd else ops.glu_fwd(ab, drop=(p, seed, offset))
            assert torch.equal(got, want)
            if want.shape[1] % 8 == 0 and (not bwd or want.shape[1] % 16 == 0):
                misses = im.misses
                seen = im.image(got, scale) if mode == "f16" else ops.split_planes(got)
                assert im.misses == misses, "the product reading the result would split / cast it again"
                assert torch.equal(seen, image(want))
            if ops.planes_only_ok(rows, inter):
                only = (ops.glu_bwd(ab, dh, planes_only=True, drop=(p, seed, offset)) if bwd
                        else ops.glu_fwd(ab, planes_only=True, drop=(p, seed, offset)))
                assert isinstance(only, ops.OperandOnly) and tuple(only.shape) == tuple(want.shape)
                assert torch.equal(only.planes[0] if mode == "f16" else only.planes, image(want))
            else:
                assert rows != 256


def _halves(fn, cut, *tensors):
    """fn on the rows [0, cut) and [cut, rows) of its arguments, concatenated: a GLU row depends on nothing but itself"""
    return torch.cat([fn(*(t[:cut] for t in tensors)), fn(*(t[cut:] for t in tensors))])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_glu_second_trip_through_the_grid_stride_loop(dtype):
    """2049 x 2052: 1,051,137 four-column groups against the generic kernels' 4096 x 256 = 1,048,576 threads (inter % 8 == 4 keeps
    bf16 on them too), so the last groups are a thread's second trip.  Plain: the bits of the same call on two row halves (one trip
    each).  Dropped at p = 0.5 (the scale 2 is exact, so bf16 composes bit for bit as well): the plain kernel and ops.dropout."""
    ops = _ops()
    rows, inter, d = 2049, 2052, DROPS[0]
    assert d[0] == 0.5 and rows * (inter // 4) > 4096 * 256 >= 1025 * (inter // 4) and inter % 8 == 4
    ab, dh = rnd((rows, 2 * inter), 950).to(dtype).to(DEV), rnd((rows, inter), 951).to(dtype).to(DEV)
    h, dab = ops.glu_fwd(ab), ops.glu_bwd(ab, dh)
    assert torch.equal(h, _halves(ops.glu_fwd, 1024, ab))
    assert torch.equal(dab, _halves(ops.glu_bwd, 1024, ab, dh))
    assert torch.equal(ops.glu_fwd(ab, drop=d), ops.dropout(h, *d))
    assert torch.equal(ops.glu_bwd(ab, dh, drop=d), ops.glu_bwd(ab, ops.dropout(dh, *d)))


@pytest.mark.parametrize("drop", [None, DROPS[0]], ids=["plain", "dropped"])
@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
def test_glu_operand_images_on_a_second_trip_through_the_loop(mode, drop):
    """2056 x 2048: 1,052,672 groups, the operand-image kernels' second trip.  The result written next to its image is the result
    outside the step; the image, next to it or alone (planes_only), is the split / half cast of that result."""
    ops = _ops()
    rows, inter = 2056, 2048
    assert rows * (inter // 4) > 4096 * 256
    ab, dh = rnd((rows, 2 * inter), 952).to(DEV), (rnd((rows, inter), 953) * 1e-3).to(DEV)
    h0, dab0 = ops.glu_fwd(ab, drop=drop), ops.glu_bwd(ab, dh, drop=drop)
    # the reference itself stands on calls of one trip each (dropped: the two-pass composition; its keep bits depend on the row offset)
    h1, dab1 = _halves(ops.glu_fwd, 1024, ab), _halves(ops.glu_bwd, 1024, ab, dh if drop is None else ops.dropout(dh, *drop))
    assert torch.equal(h0, h1 if drop is None else ops.dropout(h1, *drop)) and torch.equal(dab0, dab1)
    gs = 2.0 ** 10
    for bwd in (False, True):
        if mode == "f16":
            im = ops.F16Images()
            im.backward = bwd
            im.set_grad_scale(gs)
            scope = ops.f32_gemms_as_f16(True, im)
        else:
            im = ops.X3Images()
            im.backward = bwd
            scope = ops.f32_gemms_as_bf16x3(True, im)
        want = dab0 if bwd else h0
        scale = gs if (bwd and mode == "f16") else 1.0
        image = (lambda t: ops.cast_to_f16(t, scale)) if mode == "f16" else ops._split_planes_now
        with scope:
            got = ops.glu_bwd(ab, dh, drop=drop) if bwd else ops.glu_fwd(ab, drop=drop)
            assert torch.equal(got, want)
            misses = im.misses
            seen = im.image(got, scale) if mode == "f16" else ops.split_planes(got)
            assert im.misses == misses, "the product reading the result would split / cast it again"
            assert torch.equal(seen, image(want))
            assert ops.planes_only_ok(*want.shape)
            only = ops.glu_bwd(ab, dh, planes_only=True, drop=drop) if bwd else ops.glu_fwd(ab, planes_only=True, drop=drop)
            assert isinstance(only, ops.OperandOnly) and tuple(only.shape) == tuple(want.shape)
            assert torch.equal(only.planes[0] if mode == "f16" else only.planes, image(want))


def test_glu_eight_wide_kernels_walk_more_rows_than_their_grid():
    """bf16, inter 8: the 8-wide kernels' grid is 1 x 16384, so row 16384 of 16385 is block 0's second trip"""
    ops = _ops()
    rows, inter = 16385, 8
    ab, dh = rnd((rows, 2 * inter), 954).to(torch.bfloat16).to(DEV), rnd((rows, inter), 955).to(torch.bfloat16).to(DEV)
    assert torch.equal(ops.glu_fwd(ab), _halves(ops.glu_fwd, 16384, ab))
    assert torch.equal(ops.glu_bwd(ab, dh), _halves(ops.glu_bwd, 16384, ab, dh))


GRN_SHAPES = [(B, S_, C) for (B, S_) in ((1, 1), (3, 21), (1, 257)) for C in (8, 2816)]


@pytest.mark.parametrize("B,S_,C", GRN_SHAPES)
def test_grn_dropped(B, S_, C):
    ops = _ops()
    sd = 930 + B * 1000 + S_
    x, dy, gamma, beta = S.randn((B, S_, C), sd), S.randn((B, S_, C), sd + 1), S.randn((C,), sd + 2), S.randn((C,), sd + 3)
    xd, dyd, gd, bd_ = x.view(B * S_, C).to(DEV), dy.view(B * S_, C).to(DEV), gamma.to(DEV), beta.to(DEV)
    y_plain, stats_plain = ops.grn_fwd(xd, gd, bd_, B, S_, want_stats=True)
    ref, G64, N64 = S.ref_grn(x, gamma, beta)
    by = S.bound_grn(x, gamma, beta)["y"]
    assert bool((y_plain != 0).all())
    for p, seed, offset in DROPS:
        keep, m = R.keep_mask(B * S_, C, p, seed, offset), R.mult(B * S_, C, p, seed, offset)
        s = float(R.scale_of(p))
        y, stats = ops.grn_fwd(xd, gd, bd_, B, S_, want_stats=True, drop=(p, seed, offset))
        assert torch.equal(stats, stats_plain)                       # the statistics see the undropped input
        assert zeros_are(y, keep), (p, offset)
        want = torch.from_numpy(R.grn_drop_fwd(ref.numpy(), m))
        bound = by * s + S.U32 * want.abs()
        r = S.worst_ratio(y.cpu().view(B, S_, C), want, bound)
        print(f"grn_drop_fwd B{B} S{S_} C{C} p {p}: worst error / bound {r:.3f}")
        assert r <= 1.0
        assert torch.equal(y, ops.dropout(y_plain, p, seed, offset))
        yb = ops.grn_fwd(xd, gd, bd_, B, S_, out_dtype=torch.bfloat16, drop=(p, seed, offset))
        assert yb.dtype == torch.bfloat16 and torch.equal(yb, y.to(torch.bfloat16))     # the bf16 operand: one rounding of the dropped f32 result
        # backward: the gradient is dropped before the sums and dx read it
        dx, dgamma, dbeta = ops.grn_bwd(dyd, xd, gd, stats, B, S_, drop=(p, seed, offset))
        dye = torch.from_numpy(R.dropped_gradient(dy.view(B * S_, C).numpy(), m)).view(B, S_, C)
        st = stats.cpu()
        Gs, Ns = st[:B * C].view(B, C), st[B * C:].view(B, C)
        rb, bb = S.ref_grn_bwd(dye, x, gamma, Gs, Ns), S.bound_grn_bwd(dye, x, gamma, Gs, Ns)
        r = S.worst_ratio(dx.cpu().view(B, S_, C), rb["dx"], bb["dx"])
        print(f"grn_drop_bwd dx B{B} S{S_} C{C} p {p}: worst error / bound {r:.3f}")
        assert bool(torch.isfinite(dx).all()) and r <= 1.0
        for got, key in ((dgamma, "NS1"), (dbeta, "S0")):
            bound = bb[key].sum(0) + B * S.U32 * rb[key].abs().sum(0)
            assert got.shape == (C,) and S.worst_ratio(got.cpu(), rb[key].sum(0), bound) <= 1.0, key


def test_grn_dropped_refuses_a_width_that_is_no_multiple_of_four():
    ops = _ops()
    from muse import _hip
    L = _hip.lib()
    B, S_, C = 2, 5, 10
    x, dy, gamma, beta = (S.randn(sh, 940 + i).to(DEV) for i, sh in enumerate([(B * S_, C), (B * S_, C), (C,), (C,)]))
    y, stats, work = (torch.full((n,), 7.0, device=DEV) for n in (B * S_ * C, 2 * B * C, 4 * B * C))
    st = torch.cuda.current_stream().cuda_stream
    assert L.muse_grn_drop_fwd_ex(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), None, stats.data_ptr(), B, S_, C, 0.5, 1, 0, st) == -3
    assert L.muse_grn_drop_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), stats.data_ptr(), y.data_ptr(), work.data_ptr(), B, S_, C, 0.5, 1, 0, st) == -3
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, stats, work))     # nothing was launched
    # ops serves the width: plain kernels and a muse_dropout pass
    d = (0.5, 77, 3 << 40)
    yp, stp = ops.grn_fwd(x, gamma, beta, B, S_, want_stats=True)
    yd = ops.grn_fwd(x, gamma, beta, B, S_, drop=d)
    assert torch.equal(yd, ops.dropout(yp, *d))
    got, want = ops.grn_bwd(dy, x, gamma, stp, B, S_, drop=d), ops.grn_bwd(ops.dropout(dy, *d), x, gamma, stp, B, S_)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
