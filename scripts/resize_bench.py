"""The pre-encode image stage, two ways on the same GPU in one process (warm-up, interleaved repetitions, medians of a host clock around
work that ends in a device synchronise - host overhead is the point of the comparison):

  (a) the reference's loop (scripts/pre_encode.py:449-489) restated in torch: per image to(cuda), permute, float().div(255),
      F.interpolate(bilinear, antialias=True), the centre slice; then torch.stack
  (b) muse.pre_encode.resize_center_crop on the same host arrays: one packed copy, one launch of muse_resize_crop_u8

on a batch of 64 images of 500 x 375 -> 256 and on a seeded mixed-size batch -> 256, each from pageable host arrays and from pinned
host tensors ((b) gathers into its own pinned staging buffer either way: ragged images are separate allocations).  Also prints
max |a - b|, the kernel's own time (device events) and, from one profiled pass each, the number of device kernels and copies.

    python scripts/resize_bench.py > profiles/resize_bench.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
import numpy as np
import torch
import torch.nn.functional as F
from muse import ops, pre_encode as PE


def reference_loop(images, R):
    out = []
    for im in images:
        t = (torch.from_numpy(im) if isinstance(im, np.ndarray) else im).to("cuda", non_blocking=True)
        H, W = t.shape[0], t.shape[1]
        t = t.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        oh, ow = PE._resized_size(H, W, R)
        t = F.interpolate(t[None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0]
        top, left = PE._center_offsets(oh, ow, R)
        out.append(t[:, top:top + R, left:left + R])
    return torch.stack(out)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ops(fn):
    """(kernels, copies) the device ran during one call, from torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = sum(1 for e in dev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower())
    return len(dev) - copies, copies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resize_bench.py measures on the GPU; there is nothing to measure without one"
    B, R = args.batch, args.resolution
    rng = np.random.default_rng(0)
    sizes = {"uniform 500x375": [(500, 375)] * B,
             "mixed 256..800": [(int(h), int(w)) for h, w in rng.integers(256, 801, size=(B, 2))]}
    results = []
    for name, hw in sizes.items():
        pageable = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in hw]
        pinned = [torch.from_numpy(im).pin_memory() for im in pageable]
        mbytes = sum(im.nbytes for im in pageable) / 1e6
        for memory, imgs in (("pageable", pageable), ("pinned", pinned)):
            fa, fb = (lambda: reference_loop(imgs, R)), (lambda: PE.resize_center_crop(imgs, R))
            for _ in range(args.warmup):
                a, b = fa(), fb()
            torch.cuda.synchronize()
            diff = float((a - b).abs().max())
            ta, tb = [], []
            for _ in range(args.reps):                     # interleaved: (a), (b), (a), (b), ..
                ta.append(timed(fa)[0])
                tb.append(timed(fb)[0])
            ma, mb = statistics.median(ta), statistics.median(tb)
            rec = dict(workload=name, memory=memory, batch=B, resolution=R, input_mb=round(mbytes, 1), reps=args.reps,
                       torch_loop_ms=round(ma, 3), torch_loop_min_ms=round(min(ta), 3), torch_loop_max_ms=round(max(ta), 3),
                       fused_ms=round(mb, 3), fused_min_ms=round(min(tb), 3), fused_max_ms=round(max(tb), 3),
                       ratio=round(ma / mb, 2), max_abs_diff=diff)
            results.append(rec)
            print(f"{name:16s} {memory:8s} B={B} -> {R}  ({mbytes:.1f} MB in):  (a) torch loop {ma:8.3f} ms [{min(ta):.3f} .. {max(ta):.3f}]   "
                  f"(b) resize_center_crop {mb:8.3f} ms [{min(tb):.3f} .. {max(tb):.3f}]   (a)/(b) {ma / mb:6.2f}   max|a-b| {diff:.2e}",
                  flush=True)
        kt = []
        for _ in range(5):                                 # the launch alone, device events (ops.profile_*)
            ops.profile_start()
            PE.resize_center_crop(pageable, R)
            kt += [t for n, w, t, k in ops.profile_stop(with_kind=True) if n == "resize_crop_u8"]
        print(f"{name:16s} muse_resize_crop_u8 alone: median {statistics.median(kt) * 1e3:.1f} us of {len(kt)} launches", flush=True)
        results.append(dict(workload=name, kernel_us=round(statistics.median(kt) * 1e3, 1)))
        try:
            ka, kb = device_ops(lambda: reference_loop(pageable, R)), device_ops(lambda: PE.resize_center_crop(pageable, R))
            print(f"{name:16s} device work of one call: (a) {ka[0]} kernels + {ka[1]} copies   (b) {kb[0]} kernels + {kb[1]} copies", flush=True)
            results.append(dict(workload=name, torch_loop_kernels=ka[0], torch_loop_copies=ka[1], fused_kernels=kb[0], fused_copies=kb[1]))
        except Exception as e:                             # the timings above stand without the count
            print(f"{name:16s} device work not counted: {type(e).__name__}: {e}", flush=True)
    print(json.dumps({"resize_bench": results}))


if __name__ == "__main__":
    main()
