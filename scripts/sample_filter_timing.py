"""Time of one fused MaskGit decoding step (muse_sample_step, muse_sample_step_filtered) with the truncation filters off and on:
batch * seq = 2048 rows x 8192 codes of f32 logits, classifier-free guidance on (two logit tensors), the in-kernel Philox draws.
Configurations: the plain entry point; the filtered one with both filters off, top_k = 64, top_p = 0.9, and both.  Device events
around `--calls` back-to-back steps (one step is a launch pair of ~0.1 ms), warm-up first, the configurations alternating, median
of the repeats.  `--parent-lib` names a libmuse_hip.so built from another commit: its muse_sample_step is timed in the same
alternation, on the same tensors.  A measurement, not a test and not bench.py; needs the GPU.

    python scripts/sample_filter_timing.py [--parent-lib PATH] [--out profiles/sample_filter_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
import torch
from muse import _hip

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_filter_timing.json"))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--seq", type=int, default=1024)
ap.add_argument("--vocab", type=int, default=8192)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
assert torch.cuda.is_available(), "sample_filter_timing.py measures on the GPU"
B, S, V = args.batch, args.seq, args.vocab
mask_id = V + 7
g = torch.Generator().manual_seed(0)
cond = (torch.randn(B, S, V, generator=g) * 2).cuda()
unc = (torch.randn(B, S, V, generator=g) * 2).cuda()
ids = torch.full((B, S), mask_id, dtype=torch.long).cuda()
sampled, nxt = torch.empty_like(ids), torch.empty_like(ids)
conf = torch.empty(B * S, dtype=torch.float32, device="cuda")
step_args = (cond.data_ptr(), unc.data_ptr(), 3.0, S * V, V, V, ids.data_ptr(), mask_id, None, None, 1234, 0, 2.0, S // 2, B, S, None,
             sampled.data_ptr(), nxt.data_ptr(), conf.data_ptr())
lib = _hip.lib()
stream = _hip.stream()


def plain(handle):
    return lambda: _hip.check(handle.muse_sample_step(*step_args, stream), "muse_sample_step")


def filtered(top_k, top_p):
    return lambda: _hip.check(lib.muse_sample_step_filtered(*step_args, top_k, top_p, None, stream), "muse_sample_step_filtered")


configs = {"plain": plain(lib), "filters_off": filtered(V, 1.0), "top_k_64": filtered(64, 1.0), "top_p_0.9": filtered(V, 0.9),
           "top_k_64_top_p_0.9": filtered(64, 0.9)}
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    parent.muse_sample_step.argtypes = _hip.SIGNATURES["muse_sample_step"]
    parent.muse_sample_step.restype = C.c_int
    configs = {"parent_plain": plain(parent), **configs}


def measure(fn):
    """-> milliseconds per step"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls


for _ in range(args.warmup):
    for fn in configs.values():
        measure(fn)
times = {name: [] for name in configs}
for _ in range(args.repeats):
    for name, fn in configs.items():
        times[name].append(measure(fn))
result = {"shape": {"rows": B * S, "vocab": V, "guided": True, "dtype": "float32"}, "device": torch.cuda.get_device_name(0),
          "calls_per_window": args.calls, "repeats": args.repeats, "warmup": args.warmup,
          "ms_per_step": {n: {"median": statistics.median(t), "min": min(t), "max": max(t)} for n, t in times.items()}}
base = result["ms_per_step"]["parent_plain" if args.parent_lib else "plain"]["median"]
result["ratio_to_" + ("parent_plain" if args.parent_lib else "plain")] = {n: v["median"] / base for n, v in result["ms_per_step"].items()}
for n, v in result["ms_per_step"].items():
    print(n, json.dumps(v))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
