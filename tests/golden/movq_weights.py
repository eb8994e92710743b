"""Seeded fills and configurations of the MoVQ tokenizer fixtures (reference muse/modeling_movq.py).

`movq_shapes(cfg)` restates the state-dict template {name: shape} from the constructor arguments; `fill_movq(shapes, seed)` fills it
in sorted-key order:
  codebook N(0,1)              (the reference's +-1/num_embeddings initialisation makes every token a near-tie)
  biases 0.1 N(0,1), 1-D norm weights 1 + 0.1 N(0,1), everything else N(0,1) / sqrt(fan_in)
"""
import numpy as np
import torch

_BASE = dict(num_channels=3, out_channels=3, z_channels=4, double_z=False, num_embeddings=64, quantized_embed_dim=4, dropout=0.0,
             resample_with_conv=True, commitment_cost=0.25)
# attention runs in the last encoder level (2 blocks) and the last decoder level (3 blocks); zq factors x1 and x2
MOVQ_TINY = dict(_BASE, resolution=32, hidden_channels=32, channel_mult=(1, 2), num_res_blocks=2, attn_resolutions=(16,))
# the encoder's last level holds ONE attention block, which must not run; the decoder's two do; factors x1, x2, x4; channels 32 / 64 / 128
MOVQ_TINY3 = dict(_BASE, resolution=64, hidden_channels=32, channel_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=(16,))
FIXTURES = {"movq_tiny": MOVQ_TINY, "movq_tiny3": MOVQ_TINY3}
# the shipped geometry (openMUSE/movq-lion-high-res-f8-16384)
MOVQ_SHIPPED = dict(_BASE, resolution=256, hidden_channels=128, channel_mult=(1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(32,),
                    num_embeddings=16384)
BATCH = 2
NONSQUARE = (24, 40)


def movq_shapes(cfg: dict) -> dict:
    hc, mult, nb, zc, zq = cfg["hidden_channels"], tuple(cfg["channel_mult"]), cfg["num_res_blocks"], cfg["z_channels"], cfg["quantized_embed_dim"]
    nres, attn_res, with_conv = len(mult), tuple(cfg["attn_resolutions"]), cfg["resample_with_conv"]
    s = {}

    def conv(p, cin, cout, k):
        s[p + ".weight"], s[p + ".bias"] = (cout, cin, k, k), (cout,)

    def norm(p, c, spatial):
        if spatial:
            s[p + ".norm_layer.weight"], s[p + ".norm_layer.bias"] = (c,), (c,)
            conv(p + ".conv_y", zq, c, 1)
            conv(p + ".conv_b", zq, c, 1)
        else:
            s[p + ".weight"], s[p + ".bias"] = (c,), (c,)

    def res(p, cin, cout, spatial):
        norm(p + ".norm1", cin, spatial)
        conv(p + ".conv1", cin, cout, 3)
        norm(p + ".norm2", cout, spatial)
        conv(p + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(p + ".nin_shortcut", cin, cout, 1)

    def attn(p, c, spatial):
        norm(p + ".norm", c, spatial)
        for n in ("q", "k", "v", "proj_out"):
            s[f"{p}.{n}.weight"], s[f"{p}.{n}.bias"] = (c, c), (c,)

    def mid(p, c, spatial):
        res(p + ".block_1", c, c, spatial)
        attn(p + ".attn_1", c, spatial)
        res(p + ".block_2", c, c, spatial)

    def level(p, cin, cout, nblocks, has_attn, resample, spatial):
        for j in range(nblocks):
            res(f"{p}.block.{j}", cin if j == 0 else cout, cout, spatial)
            if has_attn:
                attn(f"{p}.attn.{j}", cout, spatial)
        if resample and with_conv:
            conv(f"{p}.{resample}.conv", cout, cout, 3)

    top = hc * mult[-1]
    conv("encoder.conv_in", cfg["num_channels"], hc, 3)
    in_mult, cur = (1,) + mult, cfg["resolution"]
    for i in range(nres):
        last = i == nres - 1
        level(f"encoder.down.{i}", hc * in_mult[i], hc * mult[i], nb, cur in attn_res, None if last else "downsample", False)
        if not last:
            cur //= 2
    mid("encoder.mid", top, False)
    norm("encoder.norm_out", top, False)
    conv("encoder.conv_out", top, zc, 3)

    conv("decoder.conv_in", zc, top, 3)
    mid("decoder.mid", top, True)
    for i in reversed(range(nres)):      # cur is the lowest resolution here
        level(f"decoder.up.{i}", top if i == nres - 1 else hc * mult[i + 1], hc * mult[i], nb + 1, cur in attn_res, "upsample" if i else None, True)
        if i:
            cur *= 2
    norm("decoder.norm_out", hc * mult[0], True)
    conv("decoder.conv_out", hc * mult[0], cfg["num_channels"], 3)

    s["quantize.embedding.weight"] = (cfg["num_embeddings"], zq)
    conv("quant_conv", zc, zq, 1)
    conv("post_quant_conv", zq, zc, 1)
    return s


def fill_movq(shapes: dict, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    sd = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        x = rng.standard_normal(shp).astype(np.float32)
        if k == "quantize.embedding.weight":
            pass
        elif k.endswith("bias"):
            x = 0.1 * x
        elif len(shp) == 1:            # GroupNorm weight
            x = 1.0 + 0.1 * x
        else:                          # Linear [out, in]; Conv2d [out, in, k, k]
            x = x / np.float32(np.sqrt(int(np.prod(shp[1:]))))
        sd[k] = torch.from_numpy(np.ascontiguousarray(x.astype(np.float32)))
    return sd


def movq_images(batch: int, h: int, w: int, seed: int) -> torch.Tensor:
    """seeded images in [0, 1], [batch, 3, h, w] f32"""
    return torch.from_numpy(np.random.default_rng(seed).random((batch, 3, h, w)).astype(np.float32))
