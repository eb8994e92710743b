"""Frechet distance on CLIP image embeds between two sets of images: the `--do compute_fid` half of the reference's
scripts/calculate_fid.py (:215-220), on muse.CLIPImageEncoder features instead of an Inception network.

    python scripts/frechet_eval.py --clip CLIP_DIR --images generated/ --reference real/ [--save-reference-stats real_stats.npz]
    python scripts/frechet_eval.py --clip CLIP_DIR --images generated/ --reference real_stats.npz [--save-stats generated_stats.npz]
    python scripts/frechet_eval.py --clip CLIP_DIR --images generated/ --reference real/ --cmmd [--save-reference-embeds real_embeds.npz]

CLIP_DIR is a LOCAL transformers snapshot (config.json + weights; a vision-only checkpoint or a full CLIPModel one); nothing is fetched.
Images are read with PIL, resized and centre-cropped to --resolution on the GPU (muse.pre_encode.resize_center_crop), then resized to the
tower's input and normalised by the scorer's own preprocess, embedded and accumulated batch by batch (muse.CLIPScorer.accumulate ->
muse.FeatureStats: nothing but the file bytes visits the host).

The number printed is NOT "FID": it is not comparable with Inception FID values (the reference's 38.57 among them), and it differs from
clean-fid's CLIP mode by the resize (ATen's antialiased bicubic in f32 here).  Compare it only with numbers this script made with the same
tower, --resolution and --dtype.

--cmmd keeps the embeds of both folders in two muse.FeatureBank during the same pass and prints one more line: CMMD (Jayasumana et al.,
CVPR 2024; muse.cmmd_distance, whose docstring says what the value can be compared with - use the ViT-L/14@336 tower for values meant to be
read next to published ones).  With a statistics file as --reference, the reference embeds come from --reference-embeds (an .npz written
by --save-reference-embeds, or a plain [n, d] .npy array)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def image_files(directory):
    found = []
    for base, _, names in os.walk(directory):
        found += [os.path.join(base, n) for n in names if n.lower().endswith(EXTENSIONS)]
    if not found:
        raise SystemExit(f"frechet_eval.py: no {'/'.join(EXTENSIONS)} image under {directory}")
    return sorted(found)


class Both:
    """what CLIPScorer.accumulate feeds: the statistics, and the bank when there is one"""

    def __init__(self, stats, bank):
        self.stats, self.bank = stats, bank

    def update(self, features):
        self.stats.update(features)
        if self.bank is not None:
            self.bank.update(features)
        return self


def directory_stats(scorer, directory, resolution, batch_size, keep_embeds=False):
    """-> (FeatureStats, FeatureBank or None) of the images under `directory`, from one pass"""
    import muse
    from PIL import Image
    files = image_files(directory)
    width = int(scorer.image_encoder.config.projection_dim)
    sink = Both(muse.FeatureStats(width, "cuda"), muse.FeatureBank(width, "cuda") if keep_embeds else None)
    samples = ((f, Image.open(f).convert("RGB")) for f in files)
    for _, pixel_values in muse.pre_encode.image_batches(samples, resolution, batch_size):
        scorer.accumulate(sink, pixel_values)
    return sink.stats, sink.bank


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clip", required=True, help="local directory of a transformers CLIP checkpoint")
    ap.add_argument("--images", required=True, help="directory of generated images")
    ap.add_argument("--reference", required=True, help="directory of real images, or a statistics file written by this script")
    ap.add_argument("--save-stats", default=None, help="write the statistics of --images here (.npz)")
    ap.add_argument("--save-reference-stats", default=None, help="write the statistics of a --reference directory here (.npz)")
    ap.add_argument("--cmmd", action="store_true", help="also keep the embeds and print CMMD (muse.cmmd_distance)")
    ap.add_argument("--reference-embeds", default=None, help="--cmmd with a statistics file as --reference: the reference embeds (.npz / .npy)")
    ap.add_argument("--save-reference-embeds", default=None, help="--cmmd: write the embeds of a --reference directory here (.npz)")
    ap.add_argument("--resolution", type=int, default=256, help="side of the centre crop taken from every image before the tower's own resize")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32", help="the tower's compute mode (INTEGRATION.md: evaluate in one mode)")
    args = ap.parse_args()
    for name in ("clip", "images", "reference"):
        if not os.path.exists(getattr(args, name)):
            raise SystemExit(f"frechet_eval.py: --{name} {getattr(args, name)} is not a local path (nothing is fetched)")
    if args.cmmd and not os.path.isdir(args.reference) and not (args.reference_embeds and os.path.exists(args.reference_embeds)):
        raise SystemExit("frechet_eval.py: --cmmd needs the reference's embeds: a directory as --reference, or a local --reference-embeds file")
    if not torch.cuda.is_available():
        raise SystemExit("frechet_eval.py embeds on the GPU; there is none")
    import muse
    encoder = muse.CLIPImageEncoder.from_pretrained(args.clip).to("cuda", dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)
    scorer = muse.CLIPScorer(encoder)
    generated, generated_bank = directory_stats(scorer, args.images, args.resolution, args.batch_size, args.cmmd)
    if os.path.isdir(args.reference):
        reference, reference_bank = directory_stats(scorer, args.reference, args.resolution, args.batch_size, args.cmmd)
        if args.save_reference_stats:
            reference.save(args.save_reference_stats)
        if args.cmmd and args.save_reference_embeds:
            reference_bank.save(args.save_reference_embeds)
    else:
        reference = muse.FeatureStats.load(args.reference)
        reference_bank = muse.FeatureBank.load(args.reference_embeds, device="cuda") if args.cmmd else None
    if args.save_stats:
        generated.save(args.save_stats)
    distance = muse.frechet_distance(generated, reference)
    print(f"Frechet distance on CLIP image embeds ({generated.n} images against {reference.n}, width {generated.dim}, {args.dtype}): {distance:.6f}")
    if args.cmmd:
        print(f"CMMD on L2-normalised CLIP image embeds ({generated_bank.n} images against {reference_bank.n}, width {generated_bank.dim}, "
              f"{args.dtype}): {muse.cmmd_distance(generated_bank, reference_bank):.6f}")


if __name__ == "__main__":
    main()
