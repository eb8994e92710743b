"""Images per second of muse.CLIPImageEncoder against transformers' CLIPVisionModelWithProjection on the same GPU.

ViT-L/14 geometry (24 layers, width 1024, 16 heads, 4096 intermediate, 224 / 14 = 257 tokens, projection 768), seeded random weights,
batch 64, from [64, 3, 256, 256] f32 images in [0, 1] to `image_embeds`:
  native     ops.resize_bicubic_norm (one launch) -> CLIPImageEncoder in bf16 mode
  yardstick  F.interpolate(bicubic, antialias=True) + normalisation -> the transformers model under torch.autocast(bfloat16)
and the towers alone from the same pixel_values.  The two alternate in one process: each is warmed up, then timed in rounds of
device-event pairs around blocks of iterations until about `--seconds` of GPU time per contender is filled; the median block gives
the figure.  A per-kernel profile of the native path (ops.profile_start / profile_stop, a run of its own) follows: launches, time, and
the rate against each kernel's algorithmic flops or bytes.

    python scripts/clip_vision_throughput.py [--out profiles/clip_vision_throughput.json]
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

GEOM = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
            projection_dim=768, hidden_act="quick_gelu")
BATCH, SOURCE = 64, 256


def block_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--layers", type=int, default=GEOM["num_hidden_layers"], help="fewer layers: a rehearsal, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_vision_throughput.py measures on the GPU; there is none")
    import muse
    from muse import ops
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    geom = dict(GEOM, num_hidden_layers=args.layers)
    torch.manual_seed(0)
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(**geom)).eval().requires_grad_(False)
    native = muse.CLIPImageEncoder.from_transformers(hf).to("cuda", dtype=torch.bfloat16)
    scorer = muse.CLIPScorer(native)
    eager = hf.to("cuda")
    images = torch.rand(BATCH, 3, SOURCE, SOURCE, generator=torch.Generator().manual_seed(1)).cuda()
    mean = torch.tensor(native.image_mean, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(native.image_std, device="cuda").view(1, 3, 1, 1)
    size = geom["image_size"]

    def eager_pre(x):
        return (F.interpolate(x, (size, size), mode="bicubic", antialias=True, align_corners=False) - mean) / std

    def eager_tower(px):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return eager(pixel_values=px).image_embeds

    with torch.no_grad():
        px = scorer.preprocess(images)
        contenders = {"native": lambda: native(scorer.preprocess(images)).image_embeds,
                      "yardstick": lambda: eager_tower(eager_pre(images)),
                      "native_tower": lambda: native(px).image_embeds,
                      "yardstick_tower": lambda: eager_tower(px)}
        a, b = contenders["native"]().float(), contenders["yardstick"]().float()
        agreement = float((a - b).abs().max() / b.abs().max())          # two bf16 pipelines on the same weights and images
        once = {}
        for name, fn in contenders.items():           # warm-up: packing, first-use work, clocks
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            once[name] = block_ms(fn, 2)
        iters = {n: max(2, int(200.0 / once[n])) for n in contenders}          # ~0.2 s blocks
        rounds = max(3, int(round(args.seconds / 0.2)))
        samples = {n: [] for n in contenders}
        for _ in range(rounds):                                                 # alternated
            for name, fn in contenders.items():
                samples[name].append(block_ms(fn, iters[name]))
        row = dict(batch=BATCH, source=SOURCE, tokens=native.tokens, layers=args.layers, rounds=rounds, max_rel_difference=round(agreement, 5))
        for name in contenders:
            ms = statistics.median(samples[name])
            row[f"{name}_ms"] = round(ms, 3)
            row[f"{name}_ms_min_max"] = [round(min(samples[name]), 3), round(max(samples[name]), 3)]
            row[f"{name}_images_per_s"] = round(BATCH / ms * 1e3, 1)
        row["native_over_yardstick"] = round(row["native_images_per_s"] / row["yardstick_images_per_s"], 3)
        print(json.dumps(row), flush=True)
        # per-kernel profile of the native path, in a run of its own
        reps = 5
        ops.profile_start()
        for _ in range(reps):
            contenders["native"]()
        agg = collections.OrderedDict()
        for name, work, ms, kind in ops.profile_stop(with_kind=True):
            e = agg.setdefault(name, dict(kind=kind, launches=0, ms=0.0, work=0.0))
            e["launches"] += 1
            e["ms"] += ms
            e["work"] += work
        total = sum(e["ms"] for e in agg.values())
        profile = []
        print(f"{'kernel':28s} {'launches/fwd':>12s} {'ms/fwd':>9s} {'share':>7s} {'rate':>14s}")
        for name, e in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
            rate = e["work"] / (e["ms"] * 1e-3) / 1e12
            unit = "TFLOP/s" if e["kind"] == "flop" else "TB/s"
            profile.append(dict(kernel=name, launches=e["launches"] // reps, ms=round(e["ms"] / reps, 4), share=round(e["ms"] / total, 4),
                                rate=round(rate, 3), unit=unit))
            print(f"{name:28s} {e['launches'] // reps:12d} {e['ms'] / reps:9.3f} {100 * e['ms'] / total:6.1f}% {rate:9.2f} {unit}")
        rest = row["native_ms"] - total / reps
        print(f"{'listed kernels, total':28s} {'':12s} {total / reps:9.3f}")
        print(f"{'forward minus listed':28s} {'':12s} {rest:9.3f}  (LayerNorm, quick-GELU, casts, the class-row gather - launches without a "
              "profile name - and launch gaps)")
        profile.append(dict(kernel="(forward minus listed)", ms=round(rest, 4)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(geometry=geom, device=torch.cuda.get_device_name(0), result=row, profile=profile), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
