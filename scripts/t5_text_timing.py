"""Single-run figures of muse.T5TextEncoder from one process, for orientation (not a benchmark, no comparison against transformers):
the encoder forward (device events, median of five) and the per-launch times from ops.profile_start / profile_stop at T5-large geometry
(24 layers, d_model 1024, 16 heads of 64, d_ff 2816, seeded random weights), batch 16, S = 32 and 128, bf16 and exact f32.

    python scripts/t5_text_timing.py > profiles/t5_text_timing.txt
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
import torch
import muse
from muse import ops

torch.manual_seed(0)
cfg = dict(vocab_size=32128, d_model=1024, d_kv=64, d_ff=2816, num_layers=24, num_heads=16)
enc = muse.T5TextEncoder(cfg).to("cuda")
B = 16
for dtype in (torch.bfloat16, torch.float32):
    enc.set_compute_dtype(dtype)
    for S in (32, 128):
        ids = torch.randint(2, 32000, (B, S), device="cuda")
        for _ in range(3):
            out = enc(ids)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(5):
            e0.record(); out = enc(ids); e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ops.profile_start()
        out = enc(ids)
        rec = ops.profile_stop(with_kind=True)
        by = {}
        for n, w, t, k in rec:
            by.setdefault(n, []).append(t)
        line = ", ".join(f"{n} x{len(v)} median {statistics.median(v) * 1e3:.1f} us" for n, v in sorted(by.items()))
        print(f"{dtype} B={B} S={S}: forward median {statistics.median(times):.3f} ms (min {min(times):.3f}) finite={bool(torch.isfinite(out.last_hidden_state).all())}")
        print(f"    per launch: {line}")
