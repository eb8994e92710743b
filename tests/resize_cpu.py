"""numpy float32 restatement of the value muse_resize_crop_u8 computes (include/muse_hip.h), written from the formula - not from the
kernel and not from ATen's source: every step one IEEE f32 operation, multiply and add rounded separately, sums from tap 0 upwards.

    resized_size / center_offsets   torchvision's _compute_resized_output_size and center_crop (Python true division, int, round)
    axis(n_in, n_out, idx)          [(lo, weights f32 [hi - lo])] for the resized indices idx of one axis
    resize_crop(u8, R, ...)         (out f32 [3, R, R], Kh, Kw): the window of the antialiased bilinear resize, flipped when asked;
                                    Kh / Kw = the largest tap count over the rows / columns the window uses
    oracle(u8, R, ...)              the same window from torch's own CPU operator (F.interpolate(antialias=True) on u8.float().div(255))
    tolerance(Kh, Kw)               (Kh + Kw + 2) * 2^-23: with bit-identical weights that sum to 1 and values in [0, 1], each side (the
                                    kernel, the oracle) rounds at most twice per tap (the product, the sum) and each rounding is at most
                                    2^-25 (half an ulp of a value below 1): 2 (Kh + Kw) 2^-25 per side, two sides, and 2 * 2^-23 of room for
                                    the weights' sums being 1 only to rounding.  Contracting product and sum into one fma rounds less
"""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


def resized_size(H, W, R):
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def center_offsets(oh, ow, R):
    return int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))


def axis(n_in, n_out, idx):
    scale = f32(n_in) / f32(n_out)
    support = scale if scale >= f32(1) else f32(1)
    inv = f32(1) / scale if scale >= f32(1) else f32(1)
    taps = []
    for i in idx:
        center = scale * (f32(i) + f32(0.5))
        lo = max(int((center - support) + f32(0.5)), 0)          # int() truncates toward zero, as the cast does
        hi = min(int((center + support) + f32(0.5)), n_in)
        w = np.zeros(hi - lo, dtype=f32)
        total = f32(0)
        for j in range(hi - lo):
            w[j] = max(f32(0), f32(1) - abs(((f32(j + lo) - center) + f32(0.5)) * inv))
            total = total + w[j]
        taps.append((lo, w / total))
    return taps


def resize_crop(u8, R, top=None, left=None, flip=False):
    u8 = np.asarray(u8)
    H, W, _ = u8.shape
    oh, ow = resized_size(H, W, R)
    ctop, cleft = center_offsets(oh, ow, R)
    top, left = ctop if top is None else top, cleft if left is None else left
    src = u8.astype(f32) / f32(255)
    tx, ty = axis(W, ow, range(left, left + R)), axis(H, oh, range(top, top + R))
    tmp = np.zeros((H, R, 3), dtype=f32)
    for ox, (lo, w) in enumerate(tx):
        for j in range(len(w)):
            tmp[:, ox] = tmp[:, ox] + src[:, lo + j] * w[j]
    out = np.zeros((R, R, 3), dtype=f32)
    for oy, (lo, w) in enumerate(ty):
        for k in range(len(w)):
            out[oy] = out[oy] + tmp[lo + k] * w[k]
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1)), max(len(w) for _, w in ty), max(len(w) for _, w in tx)


def oracle(u8, R, top=None, left=None, flip=False):
    u8 = torch.as_tensor(np.asarray(u8))
    H, W, _ = u8.shape
    oh, ow = resized_size(H, W, R)
    ctop, cleft = center_offsets(oh, ow, R)
    top, left = ctop if top is None else top, cleft if left is None else left
    x = u8.permute(2, 0, 1).contiguous().float().div(255)
    y = F.interpolate(x[None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0]
    y = y[:, top:top + R, left:left + R]
    return (y.flip(-1) if flip else y).contiguous()


def tolerance(Kh, Kw):
    return (Kh + Kw + 2) * 2.0 ** -23


# (H, W, R): the smallest shapes at which each branch of the kernel can go wrong
IDENTITY = [(16, 16, 16), (17, 17, 17)]
UPSCALE = [(9, 13, 16), (23, 10, 17), (1, 5, 16)]
DOWNSCALE = [(37, 53, 16), (53, 37, 16), (40, 61, 24), (150, 131, 16)]
FAR_WINDOW = [(16, 400, 16), (400, 16, 16)]
HALF_EVEN = [(35, 33, 32), (19, 16, 16)]
TILES = [(97, 131, 80)]      # more than one 64-column tile and five 16-row tiles, the last of both partial
SHAPES = IDENTITY + UPSCALE + DOWNSCALE + FAR_WINDOW + HALF_EVEN + TILES


def random_image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def window_extent(H, W, R):
    """(y0, y1, x0, x1): the source rows [y0, y1) and columns [x0, x1) that the centred window has NON-ZERO taps on (at scale 1 the
    second of the two taps weighs exactly 0)"""
    oh, ow = resized_size(H, W, R)
    top, left = center_offsets(oh, ow, R)
    ty, tx = axis(H, oh, (top, top + R - 1)), axis(W, ow, (left, left + R - 1))
    first = lambda t: t[0] + int(np.flatnonzero(t[1])[0])
    last = lambda t: t[0] + int(np.flatnonzero(t[1])[-1])
    return first(ty[0]), last(ty[1]) + 1, first(tx[0]), last(tx[1]) + 1


def one_hot_probes(H, W, R, seed):
    """(y, x, channel) of the single 255, all inside the source extent of the centred window (a probe that the crop discards shows
    nothing): its first corner, its last row, its last column and two seeded interior positions"""
    y0, y1, x0, x1 = window_extent(H, W, R)
    rng = np.random.default_rng(seed)
    pos = [(y0, x0, 0), (y1 - 1, (x0 + x1) // 2, 1), ((y0 + y1) // 2, x1 - 1, 2)]
    for c in (1, 2):
        pos.append((int(rng.integers(y0, y1)), int(rng.integers(x0, x1)), c))
    return pos


def one_hot(H, W, y, x, c):
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[y, x, c] = 255
    return img
