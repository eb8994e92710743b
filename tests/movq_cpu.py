"""The MoVQ tokenizer (reference muse/modeling_movq.py) restated functionally on a state dict, in f32 or f64 on the CPU: the pin the
HIP kernels and muse.modeling_movq.MOVQ are tested against.  Written against the reference's behaviour (its goldens,
tests/golden/movq_*.npz, hold this file to 1e-5), not its text: tensors are NCHW, every block is a plain function."""
import torch
import torch.nn.functional as F


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def group_norm(x, w, b, groups=32, eps=1e-6):
    return F.group_norm(x, groups, w, b, eps)


def nearest(zq, H, W, shift=(0, 0)):
    """nearest up-sampling of zq [B, Z, zh, zw] to [H, W]: output pixel (oy, ox) reads source (oy * zh // H, ox * zw // W); `shift` moves
    the source index by whole pixels (clamped) - the WRONG maps the index test tells apart from the true one"""
    if tuple(shift) == (0, 0):      # torch's own op: same values as the index map below (test_movq_surface pins that), and it keeps the
        return F.interpolate(zq, size=(H, W), mode="nearest")      # input's memory format, which selects the CPU kernels downstream
    zh, zw = zq.shape[-2:]
    iy = (torch.arange(H) * zh // H + shift[0]).clamp(0, zh - 1)
    ix = (torch.arange(W) * zw // W + shift[1]).clamp(0, zw - 1)
    return zq[:, :, iy][:, :, :, ix]


def spatial_norm(f, zq, gamma, beta, wy, by, wb, bb, groups=32, eps=1e-6, silu=False, shift=(0, 0)):
    """f [B, C, H, W], zq [B, Z, zh, zw], wy / wb [C, Z]: GroupNorm(f) * (wy . zq_up + by) + (wb . zq_up + bb), then SiLU"""
    up = nearest(zq, f.shape[-2], f.shape[-1], shift)
    m, a = F.conv2d(up, wy[:, :, None, None], by), F.conv2d(up, wb[:, :, None, None], bb)
    out = group_norm(f, gamma, beta, groups, eps) * m + a
    return F.silu(out) if silu else out


def _conv(sd, p, x, stride=1, padding=0):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=stride, padding=padding)


def _norm(sd, p, x, zq, silu):
    if zq is None:
        out = group_norm(x, sd[p + ".weight"], sd[p + ".bias"])
        return F.silu(out) if silu else out
    C = x.shape[1]
    return spatial_norm(x, zq, sd[p + ".norm_layer.weight"], sd[p + ".norm_layer.bias"], sd[p + ".conv_y.weight"].reshape(C, -1),
                        sd[p + ".conv_y.bias"], sd[p + ".conv_b.weight"].reshape(C, -1), sd[p + ".conv_b.bias"], silu=silu)


def _res(sd, p, x, zq):
    h = _conv(sd, p + ".conv1", _norm(sd, p + ".norm1", x, zq, True), padding=1)
    h = _conv(sd, p + ".conv2", _norm(sd, p + ".norm2", h, zq, True), padding=1)
    if p + ".nin_shortcut.weight" in sd:
        x = _conv(sd, p + ".nin_shortcut", x)
    return x + h


def _attn(sd, p, x, zq):
    B, C, H, W = x.shape
    h = _norm(sd, p + ".norm", x, zq, False).reshape(B, C, H * W).transpose(1, 2)       # [B, HW, C]
    q, k, v = (F.linear(h, sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"]) for n in ("q", "k", "v"))
    # (alpha inside the product, as torch.baddbmm applies it: scaling the finished scores rounds differently, and the f32 run is held
    # to 1e-5 of the reference through every attention block)
    scores = torch.baddbmm(torch.zeros((B, H * W, H * W), dtype=x.dtype), q, k.transpose(1, 2), beta=0, alpha=C ** -0.5)
    probs = torch.softmax(scores, dim=-1)
    out = F.linear(probs @ v, sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"])
    # (a strided view first, as in the reference: torch's sum then takes that operand's channels-last strides, and the next block's CPU
    # kernels - whose f32 rounding the 1e-5 comparison with the reference's goldens sees - are chosen by the memory format)
    return out.transpose(1, 2).view(B, C, H, W) + x


def _count(sd, prefix):
    n = 0
    while f"{prefix}.{n}.norm1.weight" in sd or f"{prefix}.{n}.norm1.norm_layer.weight" in sd or f"{prefix}.{n}.norm.weight" in sd \
            or f"{prefix}.{n}.norm.norm_layer.weight" in sd:
        n += 1
    return n


def _level(sd, p, x, zq):
    nblocks, nattn = _count(sd, p + ".block"), _count(sd, p + ".attn")
    for j in range(nblocks):
        x = _res(sd, f"{p}.block.{j}", x, zq)
        if nattn > 1:                       # a lone attention block holds weights and never runs
            x = _attn(sd, f"{p}.attn.{j}", x, zq)
    return x


def _mid(sd, p, x, zq):
    x = _res(sd, p + ".block_1", x, zq)
    x = _attn(sd, p + ".attn_1", x, zq)
    return _res(sd, p + ".block_2", x, zq)


def encoder(sd, cfg, px, dtype=torch.float32):
    """pixels [B, 3, H, W] -> quant_conv(encoder(px)) [B, Z, h, w]"""
    sd, x = _cast(sd, dtype), px.to(dtype)
    nres = len(cfg["channel_mult"])
    x = _conv(sd, "encoder.conv_in", x, padding=1)
    for i in range(nres):
        x = _level(sd, f"encoder.down.{i}", x, None)
        if i != nres - 1:
            if cfg["resample_with_conv"]:
                x = _conv(sd, f"encoder.down.{i}.downsample.conv", F.pad(x, (0, 1, 0, 1)), stride=2)
            else:
                x = F.avg_pool2d(x, 2, 2)
    x = _mid(sd, "encoder.mid", x, None)
    x = _conv(sd, "encoder.conv_out", _norm(sd, "encoder.norm_out", x, None, True), padding=1)
    return _conv(sd, "quant_conv", x)


def sqdist(z, cb):
    return ((z[:, None, :] - cb[None, :, :]) ** 2).sum(-1)


def nearest_code(z, cb):
    """z [B, Z, h, w] -> (indices [B, h*w], squared distances [B*h*w, Kc]) in z's dtype"""
    B, Z, h, w = z.shape
    d = sqdist(z.permute(0, 2, 3, 1).reshape(-1, Z), cb.to(z.dtype))
    return d.argmin(1).view(B, h * w), d


def lookup(sd, idx, h, w, dtype=torch.float32):
    """indices [B, h*w] -> z_q [B, Z, h, w]"""
    return sd["quantize.embedding.weight"].to(dtype)[idx].view(idx.shape[0], h, w, -1).permute(0, 3, 1, 2)


def decode(sd, cfg, zq, dtype=torch.float32):
    """z_q [B, Z, h, w] -> image"""
    sd, zq = _cast(sd, dtype), zq.to(dtype)
    nres = len(cfg["channel_mult"])
    x = _conv(sd, "decoder.conv_in", _conv(sd, "post_quant_conv", zq), padding=1)
    x = _mid(sd, "decoder.mid", x, zq)
    for i in reversed(range(nres)):
        x = _level(sd, f"decoder.up.{i}", x, zq)
        if i != 0:
            x = nearest(x, 2 * x.shape[-2], 2 * x.shape[-1])
            if cfg["resample_with_conv"]:
                x = _conv(sd, f"decoder.up.{i}.upsample.conv", x, padding=1)
    return _conv(sd, "decoder.conv_out", _norm(sd, "decoder.norm_out", x, zq, True), padding=1)


def encode(sd, cfg, px, dtype=torch.float32):
    """-> (z, z_q, indices)"""
    z = encoder(sd, cfg, px, dtype)
    idx, _ = nearest_code(z, sd["quantize.embedding.weight"])
    return z, lookup(sd, idx, z.shape[-2], z.shape[-1], dtype).contiguous(), idx


def get_code(sd, cfg, px, dtype=torch.float32):
    return nearest_code(encoder(sd, cfg, px, dtype), sd["quantize.embedding.weight"])[0]


def decode_code(sd, cfg, idx, dtype=torch.float32):
    side = int(idx.shape[1] ** 0.5)
    return decode(sd, cfg, lookup(sd, idx, side, side, dtype), dtype)
