"""Soft-target training (config.training.use_soft_code_target) at config B, measured by hand on one GPU.

  python scripts/soft_target_step.py step [--steps 20 --warmup 5 --batch 64 --reps 2 --soft-only]
      images/s of muse.TrainStep with hard labels and with soft targets, alternated (bench.py's headline setup: bf16x3 tokenizer,
      bf16 transformer, the next batch's tokenizer pass prefetched on the side stream)
  python scripts/soft_target_step.py kernels [--iters 50]
      the two soft-CE kernels at config-B size (16 448 rows, K = 1024, row stride 2032; every row past the class token active) and the
      plain-torch composition of the reference's soft_target_cross_entropy + its backward, timed with device events.  For kernel
      times run it under the profiler:
          rocprofv3 --kernel-trace --stats -d <dir> -o soft -- python scripts/soft_target_step.py kernels
      and divide the byte counts printed here by the soft_ce_fwd_kernel / soft_ce_bwd_kernel averages of the stats file.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-muse_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12


def step_rate(soft, steps, warmup, batch, dev):
    import muse
    from bench import build_models, synthetic_batch
    vq, model, opt, _ = build_models("B", "bf16x3", dev, seed=1234)
    step = muse.TrainStep(vq, model, opt, use_soft_code_target=soft)
    px, cls = synthetic_batch(batch, dev, seed=1000)
    for _ in range(warmup):
        step(px, cls, next_pixel_values=px)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, _ = step(px, cls, next_pixel_values=px)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return batch * steps / el, el / steps * 1e3, float(loss)


def torch_soft_ce(logits, labels, soft):
    """the reference's soft_target_cross_entropy in plain torch (generic ROCm kernels): the comparison point"""
    logits = logits[:, 1:][..., :soft.shape[-1]]
    labels = labels[:, 1:]
    logp = torch.nn.functional.log_softmax(logits, dim=-1)
    pad = labels.eq(-100)
    loss = torch.sum(-soft * logp, dim=-1)
    loss.masked_fill_(pad, 0.0)
    return loss.sum() / (pad.numel() - pad.long().sum())


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def kernels(iters, dev):
    from muse import ops
    B, S1, V, ld, K = 64, 257, 2025, 2032, 1024
    rows = B * S1
    gen = torch.Generator(device=dev).manual_seed(0)
    buf = torch.randn(rows, ld, device=dev, generator=gen)
    logits = buf[:, :V]
    soft = torch.softmax(torch.randn(B * (S1 - 1), K, device=dev, generator=gen), dim=-1)
    labels = torch.randint(0, K, (B, S1), device=dev, generator=gen)
    labels[:, 0] = -100
    labels = labels.view(-1).contiguous()
    g = torch.ones(1, device=dev)
    active = B * (S1 - 1)
    fwd_bytes = active * K * 4 * 2                                  # logits + soft of every active row
    bwd_bytes = {torch.float32: active * K * 8 + rows * ld * 4, torch.bfloat16: active * K * 8 + rows * ld * 2}
    state = {}

    def fwd():
        state["f"] = ops.soft_ce_fwd(logits, labels, soft, S1)

    fwd()
    lo, lse, ps = state["f"]
    us_f = timed(fwd, iters)
    print(f"soft_ce_fwd: {fwd_bytes / 1e6:.1f} MB, {us_f:.1f} us incl. reduce (events), {fwd_bytes / us_f / 1e3:.0f} GB/s, "
          f"{fwd_bytes / us_f * 1e6 / HBM_BYTES_PER_S:.2f} of 8 TB/s")
    for dt in (torch.float32, torch.bfloat16):
        us_b = timed(lambda: ops.soft_ce_bwd(logits, labels, soft, S1, lse, ps, lo, g, out_dtype=dt, width=ld), iters)
        nb = bwd_bytes[dt]
        print(f"soft_ce_bwd ({str(dt)[6:]} out): {nb / 1e6:.1f} MB, {us_b:.1f} us (events), {nb / us_b / 1e3:.0f} GB/s, "
              f"{nb / us_b * 1e6 / HBM_BYTES_PER_S:.2f} of 8 TB/s")
    # the plain-torch composition on the model's logits layout [B, S+1, V] (contiguous, as model(input_ids) returns it)
    x = logits.contiguous().view(B, S1, V).requires_grad_(True)
    lab, sft = labels.view(B, S1), soft.view(B, S1 - 1, K)

    def torch_step():
        x.grad = None
        torch_soft_ce(x, lab, sft).backward()

    def muse_step():
        from muse.training import soft_target_cross_entropy
        x.grad = None
        soft_target_cross_entropy(x, lab, sft).backward()

    print(f"loss + backward on [64, 257, 2025]: plain torch {timed(torch_step, iters):.1f} us, muse {timed(muse_step, iters):.1f} us (events)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["step", "kernels"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--soft-only", action="store_true", help="step: only the soft-target step (for a kernel trace of it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_target_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.mode == "kernels":
        kernels(args.iters, dev)
        return
    for rep in range(args.reps):
        for soft in ((True,) if args.soft_only else (False, True)):
            ips, ms, loss = step_rate(soft, args.steps, args.warmup, args.batch, dev)
            print(f"rep {rep} {'soft' if soft else 'hard'}: {ips:.1f} images/s, {ms:.2f} ms/step, loss {loss:.4f}")


if __name__ == "__main__":
    main()
