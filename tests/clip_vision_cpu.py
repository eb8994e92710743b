"""CPU side of the CLIP image-tower tests: the oracle towers (transformers' own CLIP models, built from a config under a fixed seed),
their cached runs, and the restatements of the four kernels of csrc/clip_vision.hip written from their formulas (include/muse_hip.h).
Everything returned from a cached function is shared between tests and never modified."""
import copy
import functools

import torch
import torch.nn.functional as F

LAYERS, BATCH, PROJ = 2, 3, 48
GEOMETRIES = [(64, 2), (128, 2), (96, 3)]                              # (hidden, heads): head_dim 32, 64 and 32 with three heads
GRIDS = [(28, 14), (224, 32), (224, 16), (224, 14), (336, 14)]         # (image, patch): 5, 50, 197, 257 and 577 tokens
ACTS = ["quick_gelu", "gelu"]
CASES = [(h, n, i, p) for (h, n) in GEOMETRIES for (i, p) in GRIDS if i != 336 or h == 64]      # 577 tokens at hidden 64 only
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def _trained_like(m):
    """2-D weights x 4, biases ~ N(0, 0.1): attention and LayerNorm are then not near-identity (tower() of test_gpu_clip_text.py)"""
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 2 and "embedding" not in name:
                p.mul_(4.0)
            elif name.endswith(".bias"):
                p.normal_(0.0, 0.1)
    return m


def vision_config(hidden, heads, image, patch, act="quick_gelu"):
    from transformers import CLIPVisionConfig
    return CLIPVisionConfig(hidden_size=hidden, intermediate_size=4 * hidden, num_hidden_layers=LAYERS, num_attention_heads=heads,
                            image_size=image, patch_size=patch, projection_dim=PROJ, hidden_act=act)


@functools.lru_cache(maxsize=None)
def tower(hidden, heads, image, patch, act="quick_gelu", seed=5):
    """-> (transformers CLIPVisionModelWithProjection on the CPU in f32, its f64 copy)"""
    from transformers import CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    m = _trained_like(CLIPVisionModelWithProjection(vision_config(hidden, heads, image, patch, act)).eval())
    return m, copy.deepcopy(m).double()


def make_pixels(image, seed=0, batch=BATCH):
    """normalised-image-like input: N(0, 1) per pixel"""
    return torch.randn(batch, 3, image, image, generator=torch.Generator().manual_seed(40 + image + seed))


def _run(m, px):
    """name -> tensor for every tensor the tests compare.  CLIPVisionModelWithProjection.forward returns no pooler_output: the inner
    model's outputs + the projection, as it computes them"""
    inner = m.vision_model(pixel_values=px, output_hidden_states=True, return_dict=True)
    out = {f"hidden_states[{i}]": h for i, h in enumerate(inner.hidden_states)}
    out.update(last_hidden_state=inner.last_hidden_state, pooler_output=inner.pooler_output,
               image_embeds=m.visual_projection(inner.pooler_output))
    return out


@functools.lru_cache(maxsize=None)
def oracle(hidden, heads, image, patch, act):
    """the oracle's f32, f64 and bf16-autocast runs on make_pixels(image), computed once"""
    m32, m64 = tower(hidden, heads, image, patch, act)
    px = make_pixels(image)
    with torch.no_grad():
        o32, o64 = _run(m32, px), _run(m64, px.double())
        with torch.autocast("cpu", dtype=torch.bfloat16):
            o16 = _run(m32, px)
    return o32, o64, {k: v.float() for k, v in o16.items()}


def gap(a, b):
    """max abs error over max |x|"""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


# ---- the kernels, restated ------------------------------------------------------------------------------------------------------------
def ramp(B, I):
    """per-element ramp b 10^6 + c 10^5 + y 10^3 + x: every value is an integer below 2^24 (exact in f32; also exact in bf16's source)
    and names its own position"""
    b = torch.arange(B).view(B, 1, 1, 1) * 1_000_000
    c = torch.arange(3).view(1, 3, 1, 1) * 100_000
    y = torch.arange(I).view(1, 1, I, 1) * 1000
    x = torch.arange(I).view(1, 1, 1, I)
    return (b + c + y + x).to(torch.float32)


def patch_rows(px, P):
    """[B, 3, I, I] -> [B G G, 3 P P]: unfold into non-overlapping patches, (b, gy, gx) rows, (c, ky, kx) columns"""
    B = px.shape[0]
    u = px.unfold(2, P, P).unfold(3, P, P)             # [B, 3, G, G, P(ky), P(kx)]
    return u.permute(0, 2, 3, 1, 4, 5).reshape(B * u.shape[2] * u.shape[3], 3 * P * P)


def embed_ln(patch, cls, pos, w, b, eps, batch, dtype=torch.float64):
    """rows (b, t): (t == 0 ? class : patch[b, t - 1]) + pos[t], then LayerNorm * w + b, written from the formula in `dtype`"""
    T, H = pos.shape
    x = torch.cat([cls.to(dtype).expand(batch, 1, H), patch.to(dtype).view(batch, T - 1, H)], 1) + pos.to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return ((x - mean) / torch.sqrt(var + eps) * w.to(dtype) + b.to(dtype)).view(batch * T, H), x.view(batch * T, H)


def normalise(x, mean=MEAN, std=STD):
    m, s = (torch.tensor(v, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1) for v in (mean, std))
    return (x - m) / s


def resize_norm(x, size, mean=MEAN, std=STD):
    """ATen's antialiased bicubic, then the normalisation, in x's dtype; mean / std are the f32 values in both precisions"""
    if x.shape[-1] != size:
        x = F.interpolate(x, (size, size), mode="bicubic", antialias=True, align_corners=False)
    return normalise(x, mean, std)


def smooth_images(B, R, seed=0):
    """images in [0, 1]: a few random low-frequency waves per channel; image 0 carries a hard vertical + horizontal step edge (the
    cubic overshoots there)"""
    g = torch.Generator().manual_seed(900 + R + seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, R), torch.linspace(0, 1, R), indexing="ij")
    img = torch.zeros(B, 3, R, R)
    for _ in range(4):
        f = torch.rand(B, 3, 2, generator=g) * 6.0
        ph = torch.rand(B, 3, 1, generator=g) * 6.28
        img += torch.sin(f[..., :1, None] * xx * 6.28 + f[..., 1:, None] * yy * 6.28 + ph[..., None]) / 8.0
    img = (img + 0.5).clamp(0.0, 1.0)
    img[0] = ((xx > 0.37) ^ (yy > 0.61)).float()
    return img.contiguous()
