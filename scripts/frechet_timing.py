"""Cost of muse.FeatureStats.update next to the tower forward that feeds it, and the distance between the tower's two compute modes.

1. Timing.  For (batch, width) = (64, 512), (64, 768), (64, 1024), (1024, 1024): `stats.update(embeds)` (one muse_moments_f64 launch)
   against `CLIPImageEncoder(pixel_values)` in bf16 mode at the same batch, seeded random weights - ViT-B/16 geometry (12 layers, hidden
   768) for width 512, ViT-L/14 geometry (24 layers, hidden 1024) for widths 768 and 1024.  The two alternate in one process: each is
   warmed up, then timed in rounds of device-event pairs around blocks of iterations; the median block gives the figure.  The claim under
   test: the accumulation costs under one tenth of the forward (the flop ratio is below 1 / 1000; a tenth is the allowance for launch
   latency).
2. Modes.  The Frechet distance between the statistics of the SAME images embedded in exact-f32 mode and in bf16 mode, next to the
   distance between two different sets of images in f32 mode (the scale to read it against): on a tiny tower (hidden 64, 2 layers, width
   48, 28 x 28 input), on the ViT-B/16 geometry with random weights, and on a real checkpoint with `--clip LOCAL_DIR`.

    python scripts/frechet_timing.py [--out profiles/frechet_timing.json] [--clip LOCAL_DIR]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

VIT_B = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224, patch_size=16,
             hidden_act="quick_gelu")
VIT_L = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
             hidden_act="quick_gelu")
TINY = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14,
            hidden_act="quick_gelu")
SHAPES = [(64, 512, "ViT-B/16", VIT_B), (64, 768, "ViT-L/14", VIT_L), (64, 1024, "ViT-L/14", VIT_L), (1024, 1024, "ViT-L/14", VIT_L)]


def block_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def tower(geom, width, seed=0, trained_like=False):
    import muse
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(**geom, projection_dim=width)).eval().requires_grad_(False)
    if trained_like:                       # 2-D weights x 4, biases ~ N(0, 0.1): attention and LayerNorm are then not near-identity
        for name, p in hf.named_parameters():
            if p.dim() == 2 and "embedding" not in name:
                p.mul_(4.0)
            elif name.endswith(".bias"):
                p.normal_(0.0, 0.1)
    return muse.CLIPImageEncoder.from_transformers(hf).to("cuda")


_TOWERS = {}


def time_shape(batch, width, name, geom, seconds):
    import muse
    if (name, width) not in _TOWERS:
        _TOWERS.clear()                    # one big tower at a time
        _TOWERS[(name, width)] = tower(geom, width).to(dtype=torch.bfloat16)
    enc = _TOWERS[(name, width)]
    px = torch.randn(batch, 3, geom["image_size"], geom["image_size"], generator=torch.Generator().manual_seed(2)).cuda()
    stats = muse.FeatureStats(width, "cuda")
    with torch.no_grad():
        embeds = enc(px).image_embeds
        contenders = {"update": lambda: stats.update(embeds), "forward": lambda: enc(px).image_embeds}
        once = {}
        for key, fn in contenders.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            once[key] = block_ms(fn, 2)
        iters = {k: max(2, min(20000, int(100.0 / once[k]))) for k in contenders}          # ~0.1 s blocks
        rounds = max(3, int(round(seconds / 0.1)))
        samples = {k: [] for k in contenders}
        for _ in range(rounds):                                                            # alternated
            for key, fn in contenders.items():
                samples[key].append(block_ms(fn, iters[key]))
    row = dict(batch=batch, width=width, tower=name, rounds=rounds)
    for key in contenders:
        row[f"{key}_ms"] = round(statistics.median(samples[key]), 5)
        row[f"{key}_ms_min_max"] = [round(min(samples[key]), 5), round(max(samples[key]), 5)]
        row[f"{key}_iters_per_block"] = iters[key]
    row["update_over_forward"] = round(row["update_ms"] / row["forward_ms"], 6)
    row["under_one_tenth"] = row["update_over_forward"] < 0.1
    return row


def mode_distance(enc, name, n_images, batch, source):
    """the same n_images embedded in f32 mode and in bf16 mode, and a second set in f32 mode"""
    import muse
    scorer = muse.CLIPScorer(enc)
    width = int(enc.config.projection_dim)
    made = {}
    for key, dtype, seed in (("f32", torch.float32, 10), ("bf16", torch.bfloat16, 10), ("other_f32", torch.float32, 11)):
        enc.to(dtype=dtype)
        gen = torch.Generator().manual_seed(seed)
        st = muse.FeatureStats(width, "cuda")
        for _ in range(n_images // batch):
            low = torch.rand(batch, 3, 8, 8, generator=gen)                   # smooth random images: an 8 x 8 pattern, enlarged
            scorer.accumulate(st, torch.nn.functional.interpolate(low, (source, source), mode="bilinear").clamp(0, 1).cuda())
        made[key] = st
    enc.to(dtype=torch.float32)
    import numpy as np
    return dict(tower=name, width=width, images=made["f32"].n, trace=float(np.trace(made["f32"].cov())),
                f32_against_bf16=muse.frechet_distance(made["f32"], made["bf16"]),
                f32_against_itself=muse.frechet_distance(made["f32"], made["f32"]),
                f32_against_other_images=muse.frechet_distance(made["f32"], made["other_f32"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--clip", default=None, help="a LOCAL transformers CLIP checkpoint directory for the mode comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frechet_timing.py measures on the GPU; there is none")
    import muse
    result = dict(device=torch.cuda.get_device_name(0), timing=[], modes=[])
    for batch, width, name, geom in SHAPES:
        row = time_shape(batch, width, name, geom, args.seconds)
        result["timing"].append(row)
        print(json.dumps(row), flush=True)
    _TOWERS.clear()
    with torch.no_grad():
        runs = [(tower(TINY, 48, seed=5, trained_like=True), "tiny (hidden 64, 2 layers), seeded random weights", 2048, 256, 40),
                (tower(VIT_B, 512, seed=6), "ViT-B/16 geometry, seeded random weights", 2048, 256, 256)]
        if args.clip:
            runs.append((muse.CLIPImageEncoder.from_pretrained(args.clip).to("cuda"), f"checkpoint {os.path.basename(os.path.normpath(args.clip))}", 2048, 256, 256))
        for enc, name, n_images, batch, source in runs:
            row = mode_distance(enc, name, n_images, batch, source)
            result["modes"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
