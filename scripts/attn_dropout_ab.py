"""Attention dropout: inside the fused kernels against the materialised route (MUSE_ATTN_DROPOUT_FUSED=0), device events.

    python scripts/attn_dropout_ab.py attn [--iters 30] [--repeats 3]       # one layer's attention, forward and backward
    python scripts/attn_dropout_ab.py step [--steps 20] [--repeats 3]       # whole train step, config A with the reference's default dropouts

attn: B 64, S 257, config A (8 heads of 64) and config B (16 heads of 48); legs alternated in one process, the set repeated:
  fused p=0.1      attention_drop_fwd_ex / _bwd_ex on the packed projection
  material. p=0.1  the flat engine's materialised route: scores GEMM, softmax_, dropout, P V GEMM | dV, dP GEMMs, dropout, softmax_bwd_,
                   dQ, dK GEMMs, with P and the dropped P kept
  fused p=0        attention_fwd / attention_bwd (what the kernels cost without the Philox rounds)
step: muse.TrainStep on pre-encoded tokens, hidden_dropout = attention_dropout = 0.1 (the reference constructor's defaults), bf16, batch
64; legs "fused" and "materialised" are the same model under the two settings of the switch, alternated.
MUSE_ROOT=<checkout> runs another checkout's package (one without the switch runs the materialised route in both step legs and has no
fused p=0.1 leg)."""
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
BF = torch.bfloat16
P_DROP, SEED, OFFSET = 0.1, 0x5EED, 3 << 40
HAS_FUSED = hasattr(ops, "attention_drop_fwd_ex")


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


def attn_legs(B, S, nh, hd):
    H, T, Sp, al = nh * hd, B * S, (S + 7) // 8 * 8, hd ** -0.5
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(T, 3 * H, device=DEV, generator=g).to(BF)
    dctx = torch.randn(T, H, device=DEV, generator=g).to(BF)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    sQ, sP, sX = (S * 3 * H, hd), (nh * S * Sp, S * Sp), (S * H, hd)
    st = {}

    def mat_fwd():
        P = torch.empty((B * nh, S, Sp), dtype=BF, device=DEV)
        ops.gemm(qkv, qkv, P, S, S, hd, la=0, lb=0, lda=3 * H, ldb=3 * H, ldc=Sp, a_off=0, b_off=H, alpha=al, batch=B * nh, zdiv=nh,
                 sA=sQ, sB=sQ, sC=sP)
        ops.softmax_(P, B * nh * S, S, Sp)
        Pd = ops.dropout(P, P_DROP, SEED, OFFSET)
        ctx = torch.empty((T, H), dtype=BF, device=DEV)
        ops.gemm(Pd, qkv, ctx, S, hd, S, la=0, lb=1, lda=Sp, ldb=3 * H, ldc=H, b_off=2 * H, batch=B * nh, zdiv=nh, sA=sP, sB=sQ, sC=sX)
        st["mat"] = (P, Pd)

    def mat_bwd():
        P, Pd = st["mat"]
        dqkv = torch.empty((T, 3 * H), dtype=BF, device=DEV)
        ops.gemm(Pd, dctx, dqkv, S, hd, S, la=1, lb=1, lda=Sp, ldb=H, ldc=3 * H, c_off=2 * H, batch=B * nh, zdiv=nh, sA=sP, sB=sX, sC=sQ)
        dP = torch.empty((B * nh, S, Sp), dtype=BF, device=DEV)
        ops.gemm(dctx, qkv, dP, S, S, hd, la=0, lb=0, lda=H, ldb=3 * H, ldc=Sp, b_off=2 * H, batch=B * nh, zdiv=nh, sA=sX, sB=sQ, sC=sP)
        ops.dropout(dP, P_DROP, SEED, OFFSET, out=dP)
        ops.softmax_bwd_(P, dP, B * nh * S, S, Sp)
        ops.gemm(dP, qkv, dqkv, S, hd, S, la=0, lb=1, lda=Sp, ldb=3 * H, ldc=3 * H, b_off=H, c_off=0, alpha=al, batch=B * nh, zdiv=nh,
                 sA=sP, sB=sQ, sC=sQ)
        ops.gemm(dP, qkv, dqkv, S, hd, S, la=1, lb=1, lda=Sp, ldb=3 * H, ldc=3 * H, b_off=0, c_off=H, alpha=al, batch=B * nh, zdiv=nh,
                 sA=sP, sB=sQ, sC=sQ)

    def f0_fwd():
        st["f0"] = ops.attention_fwd(qkv, B, S, nh, hd, al)

    def f0_bwd():
        ops.attention_bwd(qkv, st["f0"][0], dctx, st["f0"][1], B, S, nh, hd, al)
    legs = [("material. p=0.1", mat_fwd, mat_bwd), ("fused p=0", f0_fwd, f0_bwd)]
    if HAS_FUSED:
        drop = (P_DROP, SEED, OFFSET, Sp)
        dqkv = torch.empty_like(qkv)

        def fd_fwd():
            st["fd"] = ops.attention_drop_fwd_ex(q, k, v, B, S, S, nh, hd, al, *drop)

        def fd_bwd():
            ops.attention_drop_bwd_ex(q, k, v, st["fd"][0], dctx, st["fd"][1], B, S, S, nh, hd, al, *drop, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H],
                                      dv=dqkv[:, 2 * H:])
        legs.insert(0, ("fused p=0.1", fd_fwd, fd_bwd))
    return legs


def run_attn(args):
    for name, nh, hd in (("config A: 8 heads of 64", 8, 64), ("config B: 16 heads of 48", 16, 48)):
        legs = attn_legs(64, 257, nh, hd)
        print(f"{name}, B 64, S 257, bf16; us per launch set, {args.iters} launches per figure")
        for rep in range(args.repeats):
            for leg, fwd, bwd in legs:
                tf = timed(fwd, args.iters)
                tb = timed(bwd, args.iters)
                print(f"  repeat {rep}  {leg:16s} fwd {tf:8.1f}  bwd {tb:8.1f}  fwd+bwd {tf + tb:8.1f}", flush=True)


def run_step(args):
    cfg = dict(W.TRANSFORMER_A, hidden_dropout=0.1, attention_dropout=0.1)
    g = torch.Generator().manual_seed(7)
    tokens = torch.randint(0, cfg["codebook_size"], (args.batch, cfg["num_vq_tokens"]), generator=g).cuda()
    cls = torch.randint(0, cfg["num_classes"], (args.batch,), generator=g).cuda()
    torch.manual_seed(1234)
    model = muse.MaskGitTransformer(**cfg)
    model.to(DEV).train().set_compute_dtype(BF)
    opt = muse.FusedAdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, eps=1e-8)
    step = muse.TrainStep(None, model, opt)
    print(f"config A, hidden_dropout 0.1, attention_dropout 0.1, batch {args.batch}, bf16, pre-encoded tokens; ms per step, {args.steps} timed steps "
          f"per figure; fused attention dropout {'available' if HAS_FUSED else 'NOT in this checkout: both legs materialise'}")
    medians = {"fused": [], "materialised": []}
    for rep in range(args.repeats):
        for leg, env in (("fused", "1"), ("materialised", "0")):
            os.environ["MUSE_ATTN_DROPOUT_FUSED"] = env
            for _ in range(3):
                step(None, cls, image_tokens=tokens)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ev = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = step(None, cls, image_tokens=tokens)[0]
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in ev]
            medians[leg].append(statistics.median(ms))
            print(f"  repeat {rep}  {leg:13s} median {statistics.median(ms):7.3f}  min {min(ms):7.3f}  max {max(ms):7.3f}  loss {float(loss):.4f}  "
                  f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB", flush=True)
    f, m = (statistics.median(medians[k]) for k in ("fused", "materialised"))
    print(f"median of the repeats: fused {f:.3f} ms, materialised {m:.3f} ms, materialised / fused = {m / f:.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["attn", "step"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    (run_attn if a.what == "attn" else run_step)(a)
