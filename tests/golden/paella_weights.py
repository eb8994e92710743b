"""Seeded fills and configurations of the Paella VQ tokenizer fixtures (reference muse/modeling_paella_vq.py).

`paella_shapes(cfg)` restates the state-dict template {name: shape} from the constructor arguments; `fill_paella(shapes, seed)` fills it
in sorted-key order:
  gammas 0.5 N(0,1)            (the reference initialises them to zero: every block would be the identity)
  codebook N(0,1)              (the reference's +-1/codebook_size initialisation makes every token a near-tie)
  running_var U[0.5, 1.5], running_mean 0.3 N(0,1), BatchNorm weight 1 + 0.1 N(0,1)
  weights N(0,1) / sqrt(fan_in), biases 0.1 N(0,1)
"""
import numpy as np
import torch

PAELLA_TINY = dict(levels=2, bottleneck_blocks=2, c_hidden=48, c_latent=4, codebook_size=64, scale_factor=0.3764)
PAELLA_TINY3 = dict(levels=3, bottleneck_blocks=2, c_hidden=96, c_latent=4, codebook_size=64, scale_factor=0.3764)
FIXTURES = {"paella_tiny": (PAELLA_TINY, 32), "paella_tiny3": (PAELLA_TINY3, 64)}     # name: (config, image side)
BATCH = 2
NONSQUARE = (24, 40)


def c_levels(cfg):
    return [cfg["c_hidden"] // 2 ** i for i in reversed(range(cfg["levels"]))]


def paella_shapes(cfg: dict) -> dict:
    cl, L, cz = c_levels(cfg), cfg["levels"], cfg["c_latent"]
    s = {}

    def res(prefix, c):
        s[prefix + "gammas"] = (6,)
        s[prefix + "depthwise.1.weight"], s[prefix + "depthwise.1.bias"] = (c, 1, 3, 3), (c,)
        s[prefix + "channelwise.0.weight"], s[prefix + "channelwise.0.bias"] = (4 * c, c), (4 * c,)
        s[prefix + "channelwise.2.weight"], s[prefix + "channelwise.2.bias"] = (c, 4 * c), (c,)

    s["in_block.1.weight"], s["in_block.1.bias"] = (cl[0], 12, 1, 1), (cl[0],)
    n = 0
    for i in range(L):
        if i > 0:
            s[f"down_blocks.{n}.weight"], s[f"down_blocks.{n}.bias"] = (cl[i], cl[i - 1], 4, 4), (cl[i],)
            n += 1
        res(f"down_blocks.{n}.", cl[i])
        n += 1
    s[f"down_blocks.{n}.0.weight"] = (cz, cl[-1], 1, 1)
    for k in ("weight", "bias", "running_mean", "running_var"):
        s[f"down_blocks.{n}.1.{k}"] = (cz,)
    s[f"down_blocks.{n}.1.num_batches_tracked"] = ()
    s["vquantizer.codebook.weight"] = (cfg["codebook_size"], cz)
    s["up_blocks.0.0.weight"], s["up_blocks.0.0.bias"] = (cl[-1], cz, 1, 1), (cl[-1],)
    n = 1
    for i in range(L):
        c = cl[L - 1 - i]
        for _ in range(cfg["bottleneck_blocks"] if i == 0 else 1):
            res(f"up_blocks.{n}.", c)
            n += 1
        if i < L - 1:
            s[f"up_blocks.{n}.weight"], s[f"up_blocks.{n}.bias"] = (c, cl[L - 2 - i], 4, 4), (cl[L - 2 - i],)
            n += 1
    s["out_block.0.weight"], s["out_block.0.bias"] = (12, cl[0], 1, 1), (12,)
    return s


def fill_paella(shapes: dict, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    sd = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
            continue
        x = rng.standard_normal(shp).astype(np.float32)
        if k.endswith("gammas"):
            x = 0.5 * x
        elif k == "vquantizer.codebook.weight":
            pass
        elif k.endswith("running_var"):
            x = rng.uniform(0.5, 1.5, size=shp).astype(np.float32)
        elif k.endswith("running_mean"):
            x = 0.3 * x
        elif k.endswith("bias"):
            x = 0.1 * x
        elif len(shp) == 1:            # BatchNorm weight
            x = 1.0 + 0.1 * x
        else:                           # Linear [out, in]; Conv2d [out, in / groups, k, k]; ConvTranspose2d [in, out, k, k]: 4 of 16 taps per output
            fan_in = int(np.prod(shp[1:])) if not (len(shp) == 4 and shp[2] == 4 and k.startswith("up_blocks")) else shp[0] * 4
            x = x / np.float32(np.sqrt(fan_in))
        sd[k] = torch.from_numpy(np.ascontiguousarray(x.astype(np.float32)))
    return sd


def paella_images(batch: int, h: int, w: int, seed: int) -> torch.Tensor:
    """seeded images in [0, 1], [batch, 3, h, w] f32"""
    return torch.from_numpy(np.random.default_rng(seed).random((batch, 3, h, w)).astype(np.float32))
