"""Time the Paella VQ tokenizer at the f8 geometry of the reference's configs (levels 3, c_hidden 384, 12 bottleneck blocks, 8192
codes, 256 x 256 images, batch 64): `get_code` and `decode_code` in both compute modes, and next to them the same model with
  * the fused first half of a block (ops.paella_mix_fwd) replaced by the unfused composition (stand-alone LayerNorm kernel, a
    replicate-padded copy, the zero-padding depthwise kernel, crop, scale and residual), and
  * ops.vq_nearest_small replaced by ops.vq_nearest (the [tokens, 8192] distance matrix).
Device events, warm-up, variants alternated inside every repetition, median over the repetitions; a second pass with per-launch
events (ops.profile_start) gives each instrumented kernel family's share.  Writes one JSON file.

    python scripts/exp/paella_encode.py --out profiles/paella_encode.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "open-muse_amd"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

import paella_weights as PW  # noqa: E402
from muse import ops  # noqa: E402
from muse.modeling_paella_vq import PaellaVQModel  # noqa: E402


def mix_unfused(x, p, B, H, W):
    """the composition ops.paella_mix_fwd replaces: stand-alone LayerNorm kernel (with the modulation as its weight / bias), a
    replicate-padded copy, the zero-padding depthwise kernel on it, crop, bias / gamma / residual"""
    C = x.shape[1]
    one = torch.ones(C, dtype=torch.float32, device=x.device)
    n = ops.layernorm_bias_fwd(x, one * (1.0 + p["g"][0]), one * p["g"][1], 1e-6, torch.float32)
    pad = torch.nn.functional.pad(n.view(B, H, W, C).permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1).contiguous()
    wdw = p["w9"].t().contiguous().view(C, 1, 3, 3)
    d = ops.dwconv3x3_nhwc(pad.view(-1, C), wdw, B, H + 2, W + 2, C).view(B, H + 2, W + 2, C)[:, 1:-1, 1:-1]
    return x + p["g"][2] * (d.reshape(-1, C) + p["b9"])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def shares(fn):
    ops.profile_start()
    total = timed(fn)
    fam = {}
    for name, work, ms, kind in ops.profile_stop(with_kind=True):
        f = fam.setdefault(name, dict(launches=0, ms=0.0, work=0.0, kind=kind))
        f["launches"] += 1
        f["ms"] += ms
        f["work"] += work
    out = {}
    for name, f in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
        rate = f["work"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0          # TFLOP/s (algorithmic) or TB/s (algorithmic bytes)
        out[name] = dict(launches=f["launches"], ms=round(f["ms"], 3), share=round(f["ms"] / total, 4),
                         **{"tflops" if f["kind"] == "flop" else "tbytes_per_s": round(rate, 2)})
    seen = sum(f["ms"] for f in fam.values())
    # (LayerNorm, GELU, gather, depth-to-space and the gaps between launches carry no per-launch events: the remainder)
    return dict(total_ms_with_events=round(total, 3), uninstrumented_ms=round(total - seen, 3), per_family=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paella_encode.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    cfg = dict(levels=3, bottleneck_blocks=12, c_hidden=384, c_latent=4, codebook_size=8192, scale_factor=0.3764)
    model = PaellaVQModel(**cfg)
    model.load_state_dict(PW.fill_paella(PW.paella_shapes(cfg), 1500), strict=True)
    model.to("cuda:0").eval()
    px = PW.paella_images(a.batch, a.side, a.side, 1501).to("cuda:0")
    result = dict(config=cfg, batch=a.batch, side=a.side, reps=a.reps, modes={})
    variants = {"fused": (True, True), "mix_unfused": (False, True), "vq_unfused": (True, False)}

    def run(kind, variant, ids=None):
        fuse_mix, fuse_vq = variants[variant]
        if not fuse_mix:
            model._mix = mix_unfused                                           # instance attributes shadow the class's methods
        if not fuse_vq:
            model._nearest = lambda z: ops.vq_nearest(z, model._codebook())
        try:
            return model.get_code(px) if kind == "get_code" else model.decode_code(ids)
        finally:
            model.__dict__.pop("_mix", None)
            model.__dict__.pop("_nearest", None)

    for mode in (torch.float32, "bf16x3"):
        model.set_compute_dtype(mode)
        ids = model.get_code(px)
        jobs = [("get_code", v) for v in variants] + [("decode_code", "fused"), ("decode_code", "mix_unfused")]
        same = {f"{k}/{v}": bool(torch.equal(run(k, v, ids), run(k, "fused", ids))) if k == "get_code"
                else float((run(k, v, ids) - run(k, "fused", ids)).abs().max()) for k, v in jobs if v != "fused"}
        for _ in range(a.warmup):
            for k, v in jobs:
                run(k, v, ids)
        torch.cuda.synchronize()
        times = {f"{k}/{v}": [] for k, v in jobs}
        for _ in range(a.reps):
            for k, v in jobs:
                times[f"{k}/{v}"].append(timed(lambda: run(k, v, ids)))
        entry = dict(agreement_with_fused=same)
        for key, ts in times.items():
            med = statistics.median(ts)
            entry[key] = dict(median_ms=round(med, 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), images_per_s=round(a.batch / med * 1e3, 1))
        entry["shares_get_code"] = shares(lambda: run("get_code", "fused"))
        entry["shares_decode_code"] = shares(lambda: run("decode_code", "fused", ids))
        result["modes"][str(mode)] = entry
        print(mode, json.dumps({k: v for k, v in entry.items() if "/" in k}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
