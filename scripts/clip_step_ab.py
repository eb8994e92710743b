"""What gradient clipping costs per training step (config B, pre-encoded tokens so the tokenizer does not blur it):

    python scripts/clip_step_ab.py [--batch 64] [--warmup 3] [--steps 20] [--repeats 3] [--step-limit 120]
    python scripts/clip_step_ab.py --norm-kernel 10      # only the flat norm kernel over config B's gradient (for a kernel trace)

Legs, alternated in ONE process, the set repeated `--repeats` times to show the spread; device events around every step:
  A  muse.TrainStep without clipping (AdamW inside backward)
  B  what clipping took before FusedAdamW had max_grad_norm: forward, backward(), torch.nn.utils.clip_grad_norm_, FusedAdamW.step()
  C  muse.TrainStep(max_grad_norm=1.0): sums of squares inside backward, finalize, one AdamW launch reading the scale from the device
Every step runs under a host-side time limit of its own (the process is ended with a traceback if one step exceeds it)."""
import argparse
import faulthandler
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "open-muse_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import muse  # noqa: E402
import weights as W  # noqa: E402
from muse import training  # noqa: E402

HYPER = dict(lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, eps=1e-8)


def build(seed, max_grad_norm=None):
    torch.manual_seed(seed)
    model = muse.MaskGitTransformer(**W.TRANSFORMER_B)
    model.to("cuda").train().set_compute_dtype(torch.bfloat16)
    return model, muse.FusedAdamW(model.parameters(), max_grad_norm=max_grad_norm, **HYPER)


def norm_kernel_only(iters):
    model, _ = build(1234)
    g = model.flat_grads()
    g.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    st = training._FlatNormState.of(model)
    for _ in range(iters):
        out = st.finish(g, [], 1.0, 1.0)
    torch.cuda.synchronize()
    n = sum(p.numel() for p in model.parameters())
    print(f"flat norm kernel x{iters} over {g.numel()} elements ({n} in parameters, {4 * n / 1e6:.2f} MB read per launch); norm {float(out[0]):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds one step may take before the process is ended")
    ap.add_argument("--norm-kernel", type=int, default=0, metavar="N", help="only launch the flat norm kernel N times")
    args = ap.parse_args()
    if args.norm_kernel:
        return norm_kernel_only(args.norm_kernel)
    cfg = W.TRANSFORMER_B
    g = torch.Generator().manual_seed(7)
    tokens = torch.randint(0, cfg["codebook_size"], (args.batch, cfg["num_vq_tokens"]), generator=g).cuda()
    cls = torch.randint(0, cfg["num_classes"], (args.batch,), generator=g).cuda()
    (ma, oa), (mb, ob), (mc, oc) = build(1234), build(1234), build(1234)
    step_a = muse.TrainStep(None, ma, oa)
    step_c = muse.TrainStep(None, mc, oc, max_grad_norm=1.0)

    def leg_a():
        return step_a(None, cls, image_tokens=tokens)[0]

    def leg_b():
        ids, labels, _, _ = muse.prepare_inputs_and_labels(None, None, cls, mb.config.mask_token_id, image_tokens=tokens,
                                                           codebook_size=mb.config.codebook_size)
        _, loss = mb(input_ids=ids, labels=labels)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(mb.parameters(), 1.0)
        ob.step()
        ob.zero_grad(set_to_none=True)
        return loss.detach()

    def leg_c():
        return step_c(None, cls, image_tokens=tokens)[0]
    legs = [("A TrainStep, no clipping", leg_a), ("B backward + torch clip_grad_norm_ + step", leg_b), ("C TrainStep(max_grad_norm=1.0)", leg_c)]

    def guarded(fn):
        faulthandler.dump_traceback_later(args.step_limit, exit=True)
        try:
            return fn()
        finally:
            faulthandler.cancel_dump_traceback_later()
    print(f"config B, batch {args.batch}, bf16, pre-encoded tokens; {args.warmup} warm-up + {args.steps} timed steps per leg and repeat; ms per step")
    medians = {name: [] for name, _ in legs}
    for rep in range(args.repeats):
        for name, fn in legs:
            for _ in range(args.warmup):
                guarded(fn)
            torch.cuda.synchronize()
            events = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = guarded(fn)
                e1.record()
                events.append((e0, e1))
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in events]
            medians[name].append(statistics.median(ms))
            extra = f"  coef {float(oc.last_clip_coef):.4f} norm {float(oc.last_grad_norm):.3f}" if fn is leg_c else ""
            print(f"repeat {rep}  {name:44s} median {statistics.median(ms):7.3f}  mean {statistics.fmean(ms):7.3f}  min {min(ms):7.3f}  "
                  f"max {max(ms):7.3f}  loss {float(loss):.4f}{extra}")
    print("medians of the repeats (ms):")
    for name, _ in legs:
        v = medians[name]
        print(f"  {name:44s} {'  '.join(f'{x:7.3f}' for x in v)}   spread {max(v) - min(v):.3f}")
    a, b, c = (statistics.median(medians[name]) for name, _ in legs)
    print(f"C - B = {c - b:+.3f} ms   C - A = {c - a:+.3f} ms   B - A = {b - a:+.3f} ms")


if __name__ == "__main__":
    main()
