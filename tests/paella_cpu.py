"""Functional CPU restatement of the Paella VQ tokenizer's forward over a state dict (torch CPU ops, any float dtype): the
float64-capable oracle of tests/test_gpu_paella.py for shapes that have no golden, pinned against the real reference's outputs by
tests/test_paella_surface.py (tests/golden/paella_*.npz).

Two layers:
  * the model: `encoder`, `encode`, `decode`, `decode_code`, `get_code` over {name: tensor} in NCHW, with torch's own convolutions;
  * the pieces the HIP kernels are tested against one by one: `mix` (first half of a block), `patch_rows` / `conv_down_by_rows` /
    `conv_up_by_rows` (the gather layout and the transposed convolution's tap table, built from index operations), `unshuffle2`,
    `sqdist` (direct squared distances).
"""
import torch
import torch.nn.functional as F


def _sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _ln(x):
    """LayerNorm over the channels of an NCHW tensor: no affine, eps 1e-6, biased variance"""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6)


def mix(x, w, b, g):
    """x + g[2] * (depthwise3x3(replicate_pad(LN(x) * (1 + g[0]) + g[1])) + b); x NCHW, w [C, 1, 3, 3]"""
    t = F.pad(_ln(x) * (1 + g[0]) + g[1], (1, 1, 1, 1), mode="replicate")
    return x + g[2] * F.conv2d(t, w, b, groups=x.shape[1])


def res_block(sd, p, x):
    g = sd[p + "gammas"]
    x = mix(x, sd[p + "depthwise.1.weight"], sd[p + "depthwise.1.bias"], g)
    t = (_ln(x) * (1 + g[3]) + g[4]).permute(0, 2, 3, 1)
    t = F.gelu(t @ sd[p + "channelwise.0.weight"].t() + sd[p + "channelwise.0.bias"])
    t = t @ sd[p + "channelwise.2.weight"].t() + sd[p + "channelwise.2.bias"]
    return x + g[5] * t.permute(0, 3, 1, 2)


def unshuffle2(x):
    """PixelUnshuffle(2): [B, C, 2h, 2w] -> [B, 4C, h, w], channel c * 4 + dy * 2 + dx"""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 4 * C, H // 2, W // 2)


def shuffle2(x):
    """PixelShuffle(2): the inverse of unshuffle2"""
    B, C4, h, w = x.shape
    return x.reshape(B, C4 // 4, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(B, C4 // 4, 2 * h, 2 * w)


def encoder(sd, cfg, px, dtype=torch.float32):
    """images [B, 3, H, W] -> the encoder output before quantisation [B, c_latent, H / 2^levels, W / 2^levels]"""
    sd, x = _sd(sd, dtype), px.to(dtype)
    x = F.conv2d(unshuffle2(x), sd["in_block.1.weight"], sd["in_block.1.bias"])
    n = 0
    for i in range(cfg["levels"]):
        if i > 0:
            x = F.conv2d(x, sd[f"down_blocks.{n}.weight"], sd[f"down_blocks.{n}.bias"], stride=2, padding=1)
            n += 1
        x = res_block(sd, f"down_blocks.{n}.", x)
        n += 1
    p = f"down_blocks.{n}."
    x = F.conv2d(x, sd[p + "0.weight"])
    shape = (1, -1, 1, 1)
    x = (x - sd[p + "1.running_mean"].view(shape)) / torch.sqrt(sd[p + "1.running_var"].view(shape) + 1e-5)
    return x * sd[p + "1.weight"].view(shape) + sd[p + "1.bias"].view(shape)


def sqdist(z_rows, codebook):
    """[N, D] x [Kc, D] -> squared distances [N, Kc] as the direct sum over k of (z_k - e_k)^2, ascending k"""
    d = torch.zeros((z_rows.shape[0], codebook.shape[0]), dtype=z_rows.dtype)
    for k in range(z_rows.shape[1]):
        d = d + (z_rows[:, k:k + 1] - codebook[None, :, k]) ** 2
    return d


def nearest(z, codebook):
    """z [B, D, h, w] -> indices [B, h*w] (first index among equal distances) and the distance rows"""
    rows = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    d = sqdist(rows, codebook.to(z.dtype))
    return d.argmin(1).view(z.shape[0], -1), d


def encode(sd, cfg, px, dtype=torch.float32):
    """-> (z, z_q / scale_factor, indices): what PaellaVQModel.encode returns, preceded by the unquantised latent"""
    z = encoder(sd, cfg, px, dtype)
    idx, _ = nearest(z, sd["vquantizer.codebook.weight"])
    B, D, h, w = z.shape
    zq = sd["vquantizer.codebook.weight"].to(dtype)[idx.view(-1)].view(B, h, w, D).permute(0, 3, 1, 2).contiguous()
    return z, zq / cfg["scale_factor"], idx


def get_code(sd, cfg, px, dtype=torch.float32):
    return nearest(encoder(sd, cfg, px, dtype), sd["vquantizer.codebook.weight"])[0]


def _decoder(sd, cfg, x):
    x = F.conv2d(x, sd["up_blocks.0.0.weight"], sd["up_blocks.0.0.bias"])
    n, L = 1, cfg["levels"]
    for i in range(L):
        for _ in range(cfg["bottleneck_blocks"] if i == 0 else 1):
            x = res_block(sd, f"up_blocks.{n}.", x)
            n += 1
        if i < L - 1:
            x = F.conv_transpose2d(x, sd[f"up_blocks.{n}.weight"], sd[f"up_blocks.{n}.bias"], stride=2, padding=1)
            n += 1
    return shuffle2(F.conv2d(x, sd["out_block.0.weight"], sd["out_block.0.bias"]))


def decode(sd, cfg, zq, dtype=torch.float32):
    """PaellaVQModel.decode: the input is multiplied by scale_factor first"""
    return _decoder(_sd(sd, dtype), cfg, zq.to(dtype) * cfg["scale_factor"])


def decode_code(sd, cfg, idx, dtype=torch.float32):
    """PaellaVQModel.decode_code: codebook rows on a square grid, NO scale_factor"""
    B, T = idx.shape
    side = int(round(T ** 0.5))
    cb = sd["vquantizer.codebook.weight"].to(dtype)
    return _decoder(_sd(sd, dtype), cfg, cb[idx.reshape(-1)].view(B, side, side, -1).permute(0, 3, 1, 2))


# ---- the gather layout of the resampling convolutions, from index operations ------------------------------------------------------
def patch_rows(x, KS, stride, pad_top, pad_left, Hout, Wout):
    """x [B, H, W, C] channels-last -> [B*Hout*Wout, KS*KS*C]: element (ky, kx, c) of row (b, oy, ox) is
    x[b, oy*stride - pad_top + ky, ox*stride - pad_left + kx, c], zero outside the image"""
    B, H, W, C = x.shape
    oy, ox = torch.arange(Hout), torch.arange(Wout)
    out = torch.zeros((B, Hout, Wout, KS, KS, C), dtype=x.dtype)
    for ky in range(KS):
        iy = oy * stride - pad_top + ky
        for kx in range(KS):
            ix = ox * stride - pad_left + kx
            ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            v = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            out[:, :, :, ky, kx] = v * ok[None, :, :, None].to(x.dtype)
    return out.reshape(B * Hout * Wout, KS * KS * C)


def down_weight_rows(w):
    """Conv2d(4, 2, 1) weight [Cout, Cin, 4, 4] -> [Cout, (ky, kx, cin)]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


UP_TAPS = {(a, j): 3 - a - 2 * j for a in (0, 1) for j in (0, 1)}    # output phase a, patch row j -> kernel tap: {0: (3, 1), 1: (2, 0)}


def up_weight_rows(w, a, b):
    """ConvTranspose2d(4, 2, 1) weight [Cin, Cout, 4, 4] -> the [Cout, (j, i, cin)] matrix of output phase (a, b)"""
    taps = w[:, :, [UP_TAPS[a, 0], UP_TAPS[a, 1]]][:, :, :, [UP_TAPS[b, 0], UP_TAPS[b, 1]]]
    return taps.permute(1, 2, 3, 0).reshape(w.shape[1], -1)


def conv_down_by_rows(x, w, bias):
    """Conv2d(4, 2, 1) of x [B, H, W, Cin] channels-last as gather + product -> [B, H/2, W/2, Cout]"""
    B, H, W, _ = x.shape
    y = patch_rows(x, 4, 2, 1, 1, H // 2, W // 2) @ down_weight_rows(w).t() + bias
    return y.view(B, H // 2, W // 2, -1)


def conv_up_by_rows(x, w, bias):
    """ConvTranspose2d(4, 2, 1) of x [B, H, W, Cin] channels-last as four phase gathers + products -> [B, 2H, 2W, Cout]"""
    B, H, W, _ = x.shape
    out = torch.zeros((B, 2 * H, 2 * W, w.shape[1]), dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            y = patch_rows(x, 2, 1, 1 - a, 1 - b, H, W) @ up_weight_rows(w, a, b).t() + bias
            out[:, a::2, b::2] = y.view(B, H, W, -1)
    return out
