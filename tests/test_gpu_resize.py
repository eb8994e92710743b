"""muse_resize_crop_u8 / muse.pre_encode.resize_center_crop on the GPU against torch's own CPU operator: F.interpolate(mode="bilinear",
antialias=True) on u8.float().div(255), sliced at the window and flipped where asked (tests/resize_cpu.py: oracle, shapes, tolerance).

One-hot images pin the weights bit for bit (each output is one product of two weights; a contracted multiply-add in the weight
arithmetic fails here); random images stay within (Kh + Kw + 2) * 2^-23 (derivation: resize_cpu.tolerance).  Shapes (H, W, R) are the
smallest at which each branch can go wrong: identity, up-scaling (support 1), non-integer down-scaling, 17 taps per axis (ten streamed
source-row chunks), a window 192 pixels from the image start, the two half-to-even crop origins, and R = 80 for a second column tile."""
import functools
import os
import tarfile

import numpy as np
import pytest
import torch

import resize_cpu as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def random_case(shape, seed=0):
    """(image, oracle, bound) of one seeded random image, computed once and shared (read-only) by the tests that use it"""
    H, W, R = shape
    img = RC.random_image(H, W, seed=100 * seed + 7 + H + W)
    img.setflags(write=False)
    _, Kh, Kw = RC.resize_crop(img, R)
    return img, RC.oracle(img.copy(), R), RC.tolerance(Kh, Kw)


R16 = [s for s in RC.SHAPES if s[2] == 16]


@pytest.mark.parametrize("shape", RC.UPSCALE + RC.DOWNSCALE + RC.FAR_WINDOW + RC.HALF_EVEN + RC.TILES, ids=str)
def test_one_hot_probes_are_exact(shape):
    """a zero image with a single 255 (first corner / last row / last column of the window's source extent, two seeded interior
    positions): output == oracle bit for bit, and the channels that were not set are exactly 0"""
    from muse import pre_encode as PE
    H, W, R = shape
    probes = RC.one_hot_probes(H, W, R, seed=H * 1000 + W)
    imgs = [RC.one_hot(H, W, y, x, c) for (y, x, c) in probes]
    got = PE.resize_center_crop(imgs, R).cpu()
    for b, (y, x, c) in enumerate(probes):
        want = RC.oracle(imgs[b], R)
        assert float(want[c].max()) > 0
        assert torch.equal(bits(got[b]), bits(want)), (shape, y, x, c, float((got[b] - want).abs().max()))
        assert not got[b][[k for k in range(3) if k != c]].any()


@pytest.mark.parametrize("shape", RC.SHAPES, ids=str)
def test_random_images_within_the_derived_tolerance(shape):
    from muse import pre_encode as PE
    H, W, R = shape
    img, want, bound = random_case(shape)
    got = PE.resize_center_crop([img.copy()], R)
    assert got.shape == (1, 3, R, R) and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
    err = float((got[0].cpu() - want).abs().max())
    print(shape, "err", err, "bound", bound)
    assert err <= bound
    if shape in RC.IDENTITY:       # scale 1: taps (1, 0) on both axes, the output is u8 / 255 itself
        assert torch.equal(bits(got[0]), bits(torch.from_numpy(img.copy()).permute(2, 0, 1).float().div(255)))


def test_ragged_batch_in_one_launch():
    """the nine R = 16 shapes plus two more images of the 5- and 17-tap shapes (B = 11) in one call, in a seeded order, as a mix of CPU
    tensors and numpy arrays: image b equals the same image processed alone bit for bit, and the batch is within the tolerance"""
    from muse import pre_encode as PE
    cases = [(s, 0) for s in R16] + [((37, 53, 16), 1), ((150, 131, 16), 1)]
    assert len(cases) == 11
    order = np.random.default_rng(5).permutation(len(cases))
    cases = [cases[i] for i in order]
    imgs = [random_case(s, seed)[0].copy() for s, seed in cases]
    imgs = [torch.from_numpy(im) if i % 3 == 0 else im for i, im in enumerate(imgs)]
    got = PE.resize_center_crop(imgs, 16)
    assert got.shape == (11, 3, 16, 16)
    for b, (s, seed) in enumerate(cases):
        alone = PE.resize_center_crop([imgs[b]], 16)
        assert torch.equal(bits(got[b]), bits(alone[0])), (b, s)
        _, want, bound = random_case(s, seed)
        assert float((got[b].cpu() - want).abs().max()) <= bound, (b, s)


@pytest.mark.parametrize("image_value, gap_value", [(0, 255), (255, 0)])
def test_unaligned_gapped_packing(image_value, gap_value):
    """ops.resize_crop_u8 directly: images at odd byte offsets with 7- and 13-byte gaps before, between and after them.  Zero images
    between gaps of 255 give exactly 0 (no byte outside an image is read); images of 255 between gaps of 0 give 1 within 2^-22"""
    from muse import ops
    R = 16
    shapes, gaps = [(37, 53), (53, 37), (9, 13)], [7, 13, 7, 13]
    parts, rows = [], []
    off = 0
    for i, (H, W) in enumerate(shapes):
        parts.append(torch.full((gaps[i],), gap_value, dtype=torch.uint8))
        off += gaps[i]
        assert off % 2 == 1
        oh, ow = RC.resized_size(H, W, R)
        rows.append([off, H, W, oh, ow, *RC.center_offsets(oh, ow, R), i % 2])
        parts.append(torch.full((3 * H * W,), image_value, dtype=torch.uint8))
        off += 3 * H * W
    parts.append(torch.full((gaps[-1],), gap_value, dtype=torch.uint8))
    packed, table = torch.cat(parts).to(DEV), torch.tensor(rows, dtype=torch.int64).to(DEV)
    got = ops.resize_crop_u8(packed, table, len(shapes), R).cpu()
    if image_value == 0:
        assert not got.any()
    else:
        assert float((got - 1).abs().max()) <= 2.0 ** -22


def test_output_guard():
    """`out` = the middle of a larger tensor filled with a sentinel: the sentinel is unchanged on both sides"""
    from muse import ops
    shape = (37, 53, 16)
    H, W, R = shape
    img, want, bound = random_case(shape)
    oh, ow = RC.resized_size(H, W, R)
    table = torch.tensor([[o, H, W, oh, ow, *RC.center_offsets(oh, ow, R), 0] for o in (0, 3 * H * W)], dtype=torch.int64).to(DEV)
    packed = torch.from_numpy(img.copy()).reshape(-1).repeat(2).to(DEV)
    big = torch.full((4, 3, R, R), -7.5, dtype=torch.float32, device=DEV)
    out = ops.resize_crop_u8(packed, table, 2, R, out=big[1:3])
    assert out.data_ptr() == big[1].data_ptr()
    assert bool((big[0] == -7.5).all()) and bool((big[3] == -7.5).all())
    assert float((big[1].cpu() - want).abs().max()) <= bound and torch.equal(big[1], big[2])


def test_offsets_flip_and_meta():
    from muse import pre_encode as PE
    R = 16
    shapes = [(37, 53, 16), (53, 37, 16), (150, 131, 16), (16, 16, 16)]
    imgs = [random_case(s)[0].copy() for s in shapes]
    sizes = [RC.resized_size(*s) for s in shapes]
    corner0 = [[0, 0]] * 4
    corner1 = [[oh - R, ow - R] for oh, ow in sizes]
    flip = [True, False, True, False]
    for offs in (corner0, corner1):
        got, orig, coords = PE.resize_center_crop(imgs, R, crop_offsets=offs, flip=torch.tensor(flip), return_meta=True)
        assert orig.tolist() == [[s[1], s[0]] for s in shapes] and coords.tolist() == [list(o) for o in offs]
        for b, s in enumerate(shapes):
            want = RC.oracle(imgs[b], R, top=offs[b][0], left=offs[b][1], flip=flip[b])
            assert float((got[b].cpu() - want).abs().max()) <= random_case(s)[2], (b, s, offs[b])
    # the centred default is the explicit centred window, bit for bit; a flip mirrors the same bits
    centred = [list(RC.center_offsets(oh, ow, R)) for oh, ow in sizes]
    a, orig, coords = PE.resize_center_crop(imgs, R, return_meta=True)
    b_ = PE.resize_center_crop(imgs, R, crop_offsets=torch.tensor(centred))
    assert coords.tolist() == centred and torch.equal(bits(a), bits(b_))
    f = PE.resize_center_crop(imgs, R, flip=[True] * 4)
    assert torch.equal(bits(f), bits(a.flip(-1)))
    # GPU-resident images are concatenated on the device behind the CPU ones
    mixed = [torch.from_numpy(im).to(DEV) if i % 2 else im for i, im in enumerate(imgs)]
    assert torch.equal(bits(PE.resize_center_crop(mixed, R)), bits(a))
    assert torch.equal(bits(PE.resize_center_crop([torch.from_numpy(im).to(DEV) for im in imgs], R)), bits(a))


def test_refuses_bad_arguments_without_launching():
    from muse import _hip, ops
    L = _hip.lib()
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    assert L.muse_resize_crop_u8(t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 16, None) == -1
    assert L.muse_resize_crop_u8(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 0, None) == -1
    assert L.muse_resize_crop_u8(None, t.data_ptr(), t.data_ptr(), 1, 16, None) == -1
    assert L.muse_resize_crop_u8(t.data_ptr(), None, t.data_ptr(), 1, 16, None) == -1
    assert L.muse_resize_crop_u8(t.data_ptr(), t.data_ptr(), None, 1, 16, None) == -1
    packed = torch.zeros(3 * 20 * 30, dtype=torch.uint8, device=DEV)
    good = [0, 20, 30, 16, 24, 0, 4, 0]
    for col, val in ((0, 1), (0, -1), (1, 21), (5, 1), (6, 9), (3, 15), (7, 2)):      # one entry of a valid row made invalid
        row = list(good)
        row[col] = val
        with pytest.raises(_hip.MuseHipError):
            ops.resize_crop_u8(packed, torch.tensor([row], dtype=torch.int64, device=DEV), 1, 16)
    assert ops.resize_crop_u8(packed, torch.tensor([good], dtype=torch.int64, device=DEV), 1, 16).shape == (1, 3, 16, 16)


def test_images_to_token_shards_through_the_tokenizer(tmp_path):
    """pre_encode(vq, image_batches(samples, 16, 4), ..) writes one shard whose tokens are vq.get_code(resize_center_crop(..)) of the same
    images; the ragged tail batch is there with drop_last=False and gone with drop_last=True"""
    import muse
    import weights as W
    from muse import pre_encode as PE
    vq = muse.MaskGitVQGAN(**W.VQGAN_TINY)
    vq.load_state_dict(W.fill_state_dict(W.vqgan_shapes(W.VQGAN_TINY), 5, "vqgan"))
    vq.to(DEV).eval()
    shapes = [(37, 53, 16), (53, 37, 16), (150, 131, 16), (16, 16, 16), (9, 13, 16), (19, 16, 16)]
    samples = [(f"{i:04d}", random_case(s)[0].copy()) for i, s in enumerate(shapes)]
    batches = list(PE.image_batches(iter(samples), 16, 4))
    assert [len(k) for k, _ in batches] == [4, 2] and [tuple(p.shape) for _, p in batches] == [(4, 3, 16, 16), (2, 3, 16, 16)]
    assert [len(k) for k, _ in PE.image_batches(iter(samples), 16, 4, drop_last=True)] == [4]
    pattern = str(tmp_path / "%05d.tar")
    assert PE.pre_encode(vq, PE.image_batches(iter(samples), 16, 4), pattern, "tiny/vqgan") == 6
    assert sorted(os.listdir(tmp_path)) == ["00000.tar"]
    got = list(PE.read_token_shard(pattern % 0, "tiny/vqgan"))
    assert [s["__key__"] for s in got] == [k for k, _ in samples]
    want = torch.cat([vq.get_code(PE.resize_center_crop([im for _, im in samples[a:b]], 16)).cpu() for a, b in ((0, 4), (4, 6))])
    assert torch.equal(torch.stack([s["image_input_ids"] for s in got]), want.to(torch.int64))
    assert len(tarfile.open(pattern % 0).getnames()) == 12
