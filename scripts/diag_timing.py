"""Time and peak memory of the masked-token logging diagnostics (muse.training_utils) on their kernel path against the torch formulation
the module keeps as `_*_torch`, on the same CUDA tensors: B = 16, S = 1024, V = 8192 f32 logits (512 MiB, the coyo_f8 geometry), the
images' masked shares spread evenly over 0.05 ... 0.95.  Device events around each call, warm-up first, the two paths alternating,
median of the repeats; torch.cuda.max_memory_allocated above the level before the call.  Also the two kernels' own launch times
(ops.profile_start) with the bytes they move, and muse_token_stats over ALL rows (no row mask) for its rate.  A measurement, not a
test and not bench.py; needs the GPU.

    python scripts/diag_timing.py [--out profiles/diag_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
import torch
from muse import ops
from muse import training_utils as TU

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_timing.json"))
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--seq", type=int, default=1024)
ap.add_argument("--vocab", type=int, default=8192)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
assert torch.cuda.is_available(), "diag_timing.py measures on the GPU"
B, S, V, LS = args.batch, args.seq, args.vocab, 0.1
mask_id = V - 1
g = torch.Generator().manual_seed(0)
logits = (torch.randn(B, S, V, generator=g) * 2).cuda()
tokens = torch.randint(0, V - 1, (B, S), generator=g)
ids = torch.where(torch.rand(B, S, generator=g) < torch.linspace(0.05, 0.95, B)[:, None], torch.full_like(tokens, mask_id), tokens)
labels = torch.where(ids == mask_id, tokens, torch.full_like(tokens, -100)).cuda()
ids = ids.cuda()
masked_rows = int((ids == mask_id).sum())


def three_torch():
    return (TU._pixel_entropy_torch(logits, ids, mask_id), TU._image_entropy_torch(logits, ids, mask_id),
            TU._cross_entropy_torch(logits, labels, ids, mask_id, V, LS))


def three_kernel():
    return (TU.pixel_entropy_per_percent_masked_bucket(logits, ids, mask_id), TU.image_entropy_per_percent_masked_bucket(logits, ids, mask_id),
            TU.cross_entropy_per_percent_masked_bucket(logits, labels, ids, mask_id, V, LS))


PAIRS = {   # name -> (torch formulation, kernel path)
    "pixel_entropy": (lambda: TU._pixel_entropy_torch(logits, ids, mask_id), lambda: TU.pixel_entropy_per_percent_masked_bucket(logits, ids, mask_id)),
    "image_entropy": (lambda: TU._image_entropy_torch(logits, ids, mask_id), lambda: TU.image_entropy_per_percent_masked_bucket(logits, ids, mask_id)),
    "cross_entropy": (lambda: TU._cross_entropy_torch(logits, labels, ids, mask_id, V, LS),
                      lambda: TU.cross_entropy_per_percent_masked_bucket(logits, labels, ids, mask_id, V, LS)),
    "all_three": (three_torch, lambda: TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)),
    "three_calls": (three_torch, three_kernel),
}


def measure(fn):
    """-> (milliseconds, peak bytes above the level before the call, the call's result)"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out


result = {"shape": {"B": B, "S": S, "V": V, "dtype": "float32", "logits_bytes": logits.numel() * 4, "masked_rows": masked_rows, "rows": B * S},
          "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "calls": {}}
for name, (ref, new) in PAIRS.items():
    for _ in range(args.warmup):
        ref(); new()
    t = {"torch": [], "kernel": []}
    peak = {}
    for _ in range(args.repeats):
        for which, fn in (("torch", ref), ("kernel", new)):
            ms, pk, out = measure(fn)
            t[which].append(ms)
            peak[which] = max(peak.get(which, 0), pk)
            del out
    a, b = ref(), new()
    a, b = (a if isinstance(a, tuple) else (a,)), ((b.pixel_entropy, b.image_entropy, b.cross_entropy) if hasattr(b, "buckets") else b if isinstance(b, tuple) else (b,))
    result["calls"][name] = {"torch_ms": statistics.median(t["torch"]), "kernel_ms": statistics.median(t["kernel"]),
                             "torch_ms_min_max": [min(t["torch"]), max(t["torch"])], "kernel_ms_min_max": [min(t["kernel"]), max(t["kernel"])],
                             "torch_peak_bytes": peak["torch"], "kernel_peak_bytes": peak["kernel"],
                             "max_abs_difference": max(float((x.double() - y.double()).abs().nan_to_num().max()) for x, y in zip(a, b))}
    print(name, json.dumps(result["calls"][name]))

# the kernels' own launches: time and the bytes they move (logits rows read once + the small results)
x = TU._logit_rows(logits)
mask = (ids == mask_id)
launches = {}
for name, fn, nbytes in (
        ("token_stats_masked_rows", lambda: ops.token_stats(x, row_mask=mask.view(-1), want_max_sum=True), masked_rows * V * 4.0 + B * S * 17.0),
        ("token_stats_all_rows", lambda: ops.token_stats(x), B * S * V * 4.0 + B * S * 8.0),
        ("masked_mean_probs", None, masked_rows * V * 4.0 + B * V * 8.0)):
    if fn is None:
        _, _, mx, sm = ops.token_stats(x, row_mask=mask.view(-1), want_max_sum=True)
        fn = lambda: ops.masked_mean_probs(x, ids, mx, sm, mask_id)      # noqa: E731
    for _ in range(args.warmup):
        fn()
    ops.profile_start()
    for _ in range(args.repeats):
        fn()
    ms = statistics.median(t_ for _, _, t_, _ in ops.profile_stop(with_kind=True))
    launches[name] = {"ms": ms, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6}
    print(name, json.dumps(launches[name]))
result["launches"] = launches
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
