"""MaskGiTUViT dropout: what it costs, device events, legs alternated in one process.

    python scripts/uvit_dropout_ab.py glu  [--iters 30] [--repeats 3]      # the dropped GLU kernel alone against GLU + muse_dropout
    python scripts/uvit_dropout_ab.py step [--steps 10] [--repeats 2]      # config 4 forward + backward, batch 64, 256 tokens

glu: config 4's feed-forward at batch 64 (16384 rows, intermediate_size 2816), f32 and bf16, forward and backward:
  dropped      muse_glu_drop_fwd / _bwd (the keep bit applied inside the kernel)
  two passes   muse_glu_fwd then muse_dropout on its result | muse_dropout on the gradient then muse_glu_bwd
  p = 0        muse_glu_fwd / _bwd (what the kernel costs without the Philox rounds)
step: weights.UVIT_CC12M in modes bf16 / bf16x3 / f16, legs p = 0 and hidden_dropout = attention_dropout = 0.1 of the same weights (the
config value is switched between legs), median [min .. max] of the timed steps and peak device memory.  In the bf16x3 / f16 modes the
dropout leg runs twice: attention dropout inside csrc/attention3.hip's kernels, and on the materialised route (MUSE_X3_ATTN_DROPOUT_FUSED=0)."""
import argparse
import os
import statistics
import sys

ROOT = os.environ.get("MUSE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "open-muse_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import muse  # noqa: E402
import weights as W  # noqa: E402
from muse import ops  # noqa: E402

DEV = "cuda"
P_DROP, SEED, OFFSET = 0.1, 0x5EED, 3 << 40


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def run_glu(args):
    rows, inter = 64 * 256, 2816
    d = (P_DROP, SEED, OFFSET)
    for dtype in (torch.float32, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(0)
        ab = torch.randn(rows, 2 * inter, device=DEV, generator=g).to(dtype)
        dh = torch.randn(rows, inter, device=DEV, generator=g).to(dtype)
        legs = [("dropped", lambda: ops.glu_fwd(ab, drop=d), lambda: ops.glu_bwd(ab, dh, drop=d)),
                ("two passes", lambda: ops.dropout(ops.glu_fwd(ab), *d), lambda: ops.glu_bwd(ab, ops.dropout(dh, *d))),
                ("p = 0", lambda: ops.glu_fwd(ab), lambda: ops.glu_bwd(ab, dh))]
        print(f"GLU [{rows}, 2 x {inter}] {dtype}; us per call, {args.iters} calls per figure")
        for rep in range(args.repeats):
            for leg, fwd, bwd in legs:
                tf, tb = timed(fwd, args.iters), timed(bwd, args.iters)
                print(f"  repeat {rep}  {leg:11s} fwd {tf:8.1f}  bwd {tb:8.1f}  fwd+bwd {tf + tb:8.1f}", flush=True)


def run_step(args):
    from muse import modeling_transformer_v2 as M
    init = M.MaskGiTUViT_v2._init_weights
    M.MaskGiTUViT_v2._init_weights = lambda self: None      # (every tensor is loaded below)
    try:
        model = muse.MaskGiTUViT(**W.UVIT_CC12M)
    finally:
        M.MaskGiTUViT_v2._init_weights = init
    model.load_state_dict(W.fill_by_shapes({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7), strict=True)
    model.to(DEV).train()
    ids, enc, cond, micro, labels = (t.to(DEV) for t in W.uvit_inputs(args.batch, 256, 77, 8))
    print(f"config 4 (weights.UVIT_CC12M), batch {args.batch}, 256 tokens, 77 text states; forward + backward, ms per step, {args.steps} timed steps per figure")
    for mode in (torch.bfloat16, "bf16x3", "f16"):
        model.set_compute_dtype(mode)
        for rep in range(args.repeats):
            legs = [("p = 0", 0.0, "1"), (f"p = {P_DROP} fused", P_DROP, "1")]
            if mode != torch.bfloat16:       # the attention cores of csrc/attention3.hip against the materialised route
                legs.append((f"p = {P_DROP} materialised", P_DROP, "0"))
            for leg, p, env in legs:
                os.environ["MUSE_X3_ATTN_DROPOUT_FUSED"] = env
                model.register_to_config(hidden_dropout=p, attention_dropout=p)

                def step():
                    model.zero_grad(set_to_none=True)
                    _, loss = model(ids, enc, cond, micro, labels=labels)
                    loss.backward()
                    return loss
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                ev = []
                for _ in range(args.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    loss = step()
                    e1.record()
                    ev.append((e0, e1))
                torch.cuda.synchronize()
                ms = [a.elapsed_time(b) for a, b in ev]
                print(f"  {str(mode):15s} repeat {rep}  {leg:20s} median {statistics.median(ms):8.3f} [{min(ms):8.3f} .. {max(ms):8.3f}]  loss {float(loss.detach()):.4f}  "
                      f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["glu", "step"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    (run_glu if a.what == "glu" else run_step)(a)
