"""Cost of muse.mmd_distance (csrc/mmd.hip) at evaluation sizes, next to the same quantity by PyTorch in f64 with the n x m matrices
materialised, written as a markdown table.

For n = m in {2048, 8192, 32768} at d = 768 (the projection width of CLIP ViT-L/14): seeded random f32 features resident on the device;
each contender is warmed up, then timed call by call between device events (mmd_distance ends in its one copy to the host, the PyTorch
form in `.item()`: both are whole calls); the median call gives the figure, the minimum and maximum are written next to it.  The two
alternate in one process.  The PyTorch form is skipped, and the table says so, at a size where its three f64 matrices do not fit.

The share of the f64 MFMA peak is a whole-call figure: the multiply-adds of the dot products the three launches compute (64 x 64 tiles
on or above the diagonal for the two symmetric sums, all tiles for the rectangular one; 2 d flop per pair) over the median call time, over
--peak-tflops (78.6, the vendor's figure for the MI355X's f64 matrix rate).  exp, the squared norms and the launches are in the time and
not in the operation count.

    python scripts/mmd_timing.py [--out profiles/mmd.md] [--sizes 2048 8192 32768]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

TILE = 64


def call_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    value = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), value


def torch_f64(a, b, sigma=10.0, scale=1000.0):
    """the V-statistic on L2-normalised rows, every n x m matrix materialised in f64"""
    gamma = 1.0 / (2.0 * sigma ** 2)
    x, y = a.double(), b.double()
    x, y = x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)
    xx, yy = (x * x).sum(1), (y * y).sum(1)

    def mean_kernel(p, q, pp, qq):
        return torch.exp(-gamma * (pp[:, None] + qq[None, :] - 2.0 * (p @ q.T))).mean()

    return float((scale * (mean_kernel(x, x, xx, xx) + mean_kernel(y, y, yy, yy) - 2.0 * mean_kernel(x, y, xx, yy))).item())


def flops(n, m, d):
    tn, tm = -(-n // TILE), -(-m // TILE)
    pairs = (tn * (tn + 1) // 2 + tm * (tm + 1) // 2 + tn * tm) * TILE * TILE
    return 2.0 * d * pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmd.md"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192, 32768])
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mmd_timing.py measures on the GPU; there is none")
    import muse
    d = args.width
    rows = []
    for n in args.sizes:
        gen = torch.Generator(device="cuda").manual_seed(n)
        a = torch.randn(n, d, device="cuda", generator=gen)
        b = torch.randn(n, d, device="cuda", generator=gen) + 0.05
        contenders = {"hip": lambda: muse.mmd_distance(a, b)}
        try:
            torch_f64(a, b)
            contenders["torch"] = lambda: torch_f64(a, b)
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
        muse.mmd_distance(a, b)
        samples, values = {k: [] for k in contenders}, {}
        for _ in range(args.calls):                             # alternated
            for key, fn in contenders.items():
                ms, values[key] = call_ms(fn)
                samples[key].append(ms)
        row = dict(n=n, hip=statistics.median(samples["hip"]), hip_range=(min(samples["hip"]), max(samples["hip"])), value=values["hip"])
        row["share"] = flops(n, n, d) / (row["hip"] * 1e-3) / (args.peak_tflops * 1e12)
        if "torch" in contenders:
            row.update(torch=statistics.median(samples["torch"]), torch_range=(min(samples["torch"]), max(samples["torch"])), torch_value=values["torch"])
        rows.append(row)
        print(row, flush=True)
        del a, b
        torch.cuda.empty_cache()
    lines = ["# muse.mmd_distance: time per call", "",
             f"Device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}) - one MI355X, shared host, clocks not pinned.  Written by `scripts/mmd_timing.py` (its docstring says how each figure is taken): n = m rows of",
             f"width {d}, seeded random f32 features resident on the device, {args.calls} alternated calls per contender, device events around",
             "whole calls (row norms, three pair-sum launches, the copy of six f64 numbers; the PyTorch form ends in `.item()`).", "",
             "| n = m | mmd_distance, median ms (min .. max) | PyTorch f64, matrices materialised, median ms (min .. max) | PyTorch / HIP | "
             f"dot-product flop of the call over time, share of {args.peak_tflops:g} TFLOP/s | value (HIP) | value (PyTorch) |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        hip = f"{r['hip']:.3f} ({r['hip_range'][0]:.3f} .. {r['hip_range'][1]:.3f})"
        if "torch" in r:
            other, ratio, tv = f"{r['torch']:.3f} ({r['torch_range'][0]:.3f} .. {r['torch_range'][1]:.3f})", f"{r['torch'] / r['hip']:.2f}", f"{r['torch_value']!r}"
        else:
            other, ratio, tv = "does not fit", "-", "-"
        lines.append(f"| {r['n']} | {hip} | {other} | {ratio} | {100.0 * r['share']:.1f} % | {r['value']!r} | {tv} |")
    lines += ["", "The share is a whole-call rate over the peak, not a kernel's share of peak: exp, the squared norms, the finalize launches and the",
              "copy are in the time and not in the flop count.  No kernel trace was taken.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
