"""Throughput of muse.modeling_movq.MOVQ at the shipped geometry, and the fused spatial-norm kernel against the same layer composed
from separate ops.

Shipped geometry (hidden 128, multipliers (1, 2, 2, 4), 2 blocks per level, attention at 32, 16384 codes), 256 x 256 images, "bf16x3"
mode, seeded random weights.  After warm-up everything is timed with device-event pairs around blocks of iterations (about 0.1 s per
block), contenders alternating; the median block gives the figure.

  * images/s of `get_code` and of `decode_code` at batch 8 and batch 64;
  * for the two widest spatial-norm layers (256^2 x 128 and 128^2 x 256 channels, batch 8, planes output, the producing convolution's
    statistics given): the fused kernel's time, its algorithmic bytes (x read once, the two bf16 planes written, zq and the weights)
    and the resulting fraction of 8 TB/s - against the time of the layer composed from nearest up-sampling of zq, two 1x1
    convolutions, the GroupNorm apply pass without SiLU, torch multiply / add / SiLU and the bf16 split.

    python scripts/bench_movq.py [--out profiles/movq_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

HBM_BYTES_PER_S = 8e12
SIDE = 256


def block_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(contenders, seconds):
    """{name: fn} -> {name: (median, min, max) ms per call}"""
    once = {}
    for name, fn in contenders.items():       # warm-up: packing, first-use work, clocks
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        once[name] = block_ms(fn, 2)
    iters = {n: max(2, int(100.0 / once[n])) for n in contenders}
    rounds = max(3, int(round(seconds / 0.1)))
    samples = {n: [] for n in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            samples[name].append(block_ms(fn, iters[name]))
    return {n: (statistics.median(s), min(s), max(s)) for n, s in samples.items()}


def layer_row(v, ops, norm, B, H, C, zside, seconds):
    """one decoder spatial norm (+ SiLU) feeding a 3x3 convolution: fused kernel against the composition of existing ops"""
    g = torch.Generator().manual_seed(H + C)
    xin = torch.randn((B, H, H, C), generator=g).cuda()
    w_hi, w_lo = ops.split_bf16((torch.randn((C, 3, 3, C), generator=g) / (9 * C) ** 0.5).cuda())
    x = ops.conv2d_nhwc_split2(*ops.split_f32(xin), w_hi, w_lo, B, H, H, C, C, gn_groups=32)        # the producer leaves the statistics
    del xin
    assert getattr(x, "_gn_stats", None) is not None
    zq = torch.randn((B, zside, zside, 4), generator=g).cuda()
    gamma, beta, wy, by, wb, bb = v._sn_weights(norm)
    factor = H // zside

    def fused():
        return ops.spatial_norm(x, zq, gamma, beta, wy, by, wb, bb, B, H, H, C, zside, zside, stats=x._gn_stats, split=True)

    def composed():
        up, s = zq, zside
        while s < H:                                                             # nearest up-sampling of zq
            up, s = ops.upsample2x(up, B, s, s, 4), 2 * s
        m = v._conv(up, norm.conv_y, B, H, H, "bf16x3")                          # two 1x1 convolutions 4 -> C
        a = v._conv(up, norm.conv_b, B, H, H, "bf16x3")
        n = ops.groupnorm_silu_nhwc(x, gamma, beta, B, H * H, C, groups=32, eps=1e-6, silu=False)
        return ops.split_f32(F.silu(n.mul_(m).add_(a)))

    hi, lo = fused()
    chi, clo = composed()
    agree = float(((hi.float() + lo.float()) - (chi.float() + clo.float())).abs().max() / (chi.float().abs().max()))
    t = alternate({"fused": fused, "composed": composed}, seconds)
    nbytes = x.numel() * 4 + 2 * x.numel() * 2 + zq.numel() * 4 + 4 * (gamma.numel() + beta.numel() + wy.numel() + by.numel() + wb.numel() + bb.numel())
    ms = t["fused"][0]
    return dict(layer=f"{H}x{H}x{C}", batch=B, zq_factor=factor, fused_ms=round(ms, 4), fused_ms_min=round(t["fused"][1], 4),
                fused_ms_max=round(t["fused"][2], 4), composed_ms=round(t["composed"][0], 4), composed_ms_min=round(t["composed"][1], 4),
                composed_ms_max=round(t["composed"][2], 4), composed_over_fused=round(t["composed"][0] / ms, 3), algorithmic_bytes=nbytes,
                tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3), fraction_of_8_tb_per_s=round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 3),
                fused_vs_composed_maxrel=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    args = ap.parse_args()
    from muse import ops
    from muse.modeling_movq import MOVQ
    assert torch.cuda.is_available(), "bench_movq.py measures on the GPU"
    torch.manual_seed(0)
    v = MOVQ()
    v.quantize.embedding.weight.data.normal_()      # (the +-1/n initialisation makes every token a near-tie)
    v.cuda().eval().half()
    assert v.compute_dtype == "bf16x3"
    model, layers = [], []
    with torch.no_grad():
        for batch in args.batches:
            px = torch.rand((batch, 3, SIDE, SIDE), generator=torch.Generator().manual_seed(batch)).cuda()
            idx = v.get_code(px)
            t = alternate({"get_code": lambda: v.get_code(px), "decode_code": lambda: v.decode_code(idx)}, args.seconds)
            row = dict(batch=batch, side=SIDE, tokens=int(idx.shape[1]))
            for name, (med, lo, hi) in t.items():
                row[f"{name}_ms"], row[f"{name}_ms_min"], row[f"{name}_ms_max"] = round(med, 3), round(lo, 3), round(hi, 3)
                row[f"{name}_images_per_s"] = round(batch / (med * 1e-3), 1)
            model.append(row)
            print(json.dumps(row), flush=True)
            del px, idx
            torch.cuda.empty_cache()
        dec = v.decoder
        for norm, H, C in ((dec.norm_out, 256, 128), (dec.up[1].block[2].norm2, 128, 256)):
            row = layer_row(v, ops, norm, 8, H, C, SIDE // 8, args.seconds)
            layers.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), mode="bf16x3", geometry=dict(v.config), model=model, spatial_norm_layers=layers),
                      f, indent=1, default=lambda o: list(o) if isinstance(o, tuple) else str(o))
            f.write("\n")


if __name__ == "__main__":
    main()
