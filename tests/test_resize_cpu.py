"""The pre-encode image stage without a GPU: the numpy f32 restatement of muse_resize_crop_u8's value (tests/resize_cpu.py) against
torch's own CPU operator, the host arithmetic of sizes and windows, and the argument checks of muse.pre_encode.resize_center_crop."""
import numpy as np
import pytest
import torch

import resize_cpu as RC


@pytest.mark.parametrize("shape", RC.UPSCALE + RC.DOWNSCALE + RC.FAR_WINDOW + RC.HALF_EVEN + RC.TILES, ids=str)
def test_restatement_equals_aten_bitwise_on_one_hot_images(shape):
    """every output of a one-hot image is one product of two weights: equality pins the weights of both axes bit for bit"""
    H, W, R = shape
    for (y, x, c) in RC.one_hot_probes(H, W, R, seed=H * 1000 + W):
        img = RC.one_hot(H, W, y, x, c)
        got, _, _ = RC.resize_crop(img, R)
        want = RC.oracle(img, R).numpy()
        assert want[c].max() > 0 and not want[[k for k in range(3) if k != c]].any()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (shape, y, x, c, float(np.abs(got - want).max()))


@pytest.mark.parametrize("shape", RC.SHAPES + [(500, 375, 256)], ids=str)
def test_restatement_within_tolerance_on_random_images(shape):
    H, W, R = shape
    img = RC.random_image(H, W, seed=7 + H + W)
    for flip in (False, True):
        got, Kh, Kw = RC.resize_crop(img, R, flip=flip)
        err = float(np.abs(got - RC.oracle(img, R, flip=flip).numpy()).max())
        print(shape, "flip", flip, "taps", Kh, Kw, "err", err, "bound", RC.tolerance(Kh, Kw))
        assert err <= RC.tolerance(Kh, Kw)
    if shape in RC.IDENTITY:
        assert np.array_equal(got[:, :, ::-1], (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_tap_counts():
    assert RC.resize_crop(RC.random_image(150, 131, 1), 16)[1:] == (17, 17)
    Kh, Kw = RC.resize_crop(RC.random_image(37, 53, 1), 16)[1:]
    assert 4 <= Kh <= 5 and 4 <= Kw <= 6
    assert RC.resize_crop(RC.random_image(9, 13, 1), 16)[1:] == (2, 2)


def test_size_and_crop_arithmetic():
    from muse import pre_encode as PE
    for H, W, R in RC.SHAPES + [(500, 375, 256), (375, 500, 256), (3, 1000, 7)]:
        oh, ow = PE._resized_size(H, W, R)
        assert (oh, ow) == RC.resized_size(H, W, R) and min(oh, ow) == R
        assert (oh == R and ow == int(R * W / H)) if H <= W else (ow == R and oh == int(R * H / W))
        assert PE._center_offsets(oh, ow, R) == RC.center_offsets(oh, ow, R)
    # Python's round goes to even on a half: an excess of 1 starts at 0, an excess of 3 at 2
    assert PE._resized_size(35, 33, 32) == (33, 32) and PE._center_offsets(33, 32, 32) == (0, 0)
    assert PE._resized_size(19, 16, 16) == (19, 16) and PE._center_offsets(19, 16, 16) == (2, 0)
    assert PE._center_offsets(16, 21, 16) == (0, 2) and PE._center_offsets(18, 16, 16) == (1, 0)
    assert PE._resized_size(500, 375, 256) == (341, 256) and PE._center_offsets(341, 256, 256) == (42, 0)


def test_random_crop_offsets_draw_for_draw():
    from muse import pre_encode as PE
    sizes = [(37, 53), (16, 16), (53, 37), (150, 131), (32, 32), (16, 400)]
    R = 16
    got = PE.random_crop_offsets(sizes, R, generator=torch.Generator().manual_seed(1234))
    g = torch.Generator().manual_seed(1234)
    want = []
    for H, W in sizes:                                      # RandomCrop.get_params on the resized (h, w)
        h, w = RC.resized_size(H, W, R)
        if h == R and w == R:
            want.append([0, 0])
            continue
        i = torch.randint(0, h - R + 1, size=(1,), generator=g).item()
        j = torch.randint(0, w - R + 1, size=(1,), generator=g).item()
        want.append([i, j])
    assert got.dtype == torch.int64 and got.tolist() == want
    assert any(t or l for t, l in want) and want[1] == [0, 0] and want[4] == [0, 0]
    for (H, W), (t, l) in zip(sizes, want):
        h, w = RC.resized_size(H, W, R)
        assert 0 <= t <= h - R and 0 <= l <= w - R


def test_surface_exports_and_argument_checks():
    from muse import _hip, ops, pre_encode as PE
    for name in ("resize_center_crop", "random_crop_offsets", "image_batches"):
        assert callable(getattr(PE, name)), name
    assert callable(ops.resize_crop_u8) and "muse_resize_crop_u8" in _hip.SIGNATURES
    from PIL import Image
    ok = np.zeros((20, 30, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="mode 'L'"):
        PE.resize_center_crop([Image.new("L", (8, 8))], 16)
    with pytest.raises(ValueError, match="mode 'RGBA'"):
        PE.resize_center_crop([ok, Image.new("RGBA", (8, 8))], 16)
    with pytest.raises(ValueError, match=r"\(20, 30, 4\)"):
        PE.resize_center_crop([np.zeros((20, 30, 4), dtype=np.uint8)], 16)
    with pytest.raises(ValueError, match="float32"):
        PE.resize_center_crop([torch.zeros(20, 30, 3)], 16)
    with pytest.raises(ValueError, match="float64"):
        PE.resize_center_crop([np.zeros((20, 30, 3))], 16)
    # 20 x 30 -> 16 x 24: top in [0, 0], left in [0, 8]
    for bad in ([[0, 9]], [[1, 0]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(ValueError, match="crop_offsets"):
            PE.resize_center_crop([ok], 16, crop_offsets=bad)
    with pytest.raises(ValueError, match="crop_offsets"):
        PE.resize_center_crop([ok], 16, crop_offsets=[[0, 0], [0, 0]])
    with pytest.raises(ValueError, match="flip"):
        PE.resize_center_crop([ok], 16, flip=[True, False])
