"""CPU, world_size 2 over gloo: gradient clipping in the data-parallel step - muse.FusedAdamW(max_grad_norm=...) with the sums of
squares accumulated behind each bucket's all-reduce (begin_norm_in_reducer / GradReducer.post_reduce).  The HIP entry points are
replaced by their CPU restatements (tests/grad_clip_cpu.py); what is under test is the protocol."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.05, eps=1e-8)
CLIP = 0.5


def _grad(n, step, rank, micro=0):
    return torch.sin(torch.arange(n, dtype=torch.float32) * 0.01 * (step + 1) + micro) * 3.0 * (rank + 1)


def _worker(rank, world, port, out):
    for p in (os.path.join(ROOT, "open-muse_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, p)
    import muse
    import weights as W
    from muse import ops
    from oracle import maskgit_oracle as O
    from grad_clip_cpu import Recorder
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rec = Recorder(O.adamw_step).install(ops)
    torch.manual_seed(300 + rank)
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    m.set_compute_dtype(torch.float32)
    red = muse.GradReducer(m, bucket_bytes=4 * 14000)              # a bucket spans layers, the last one is ragged
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=CLIP, **HYPER)
    n = m.flat_params().numel()
    p0 = m.flat_params().clone()
    off, L = m._offsets, m.num_hidden_layers
    t0 = 2 + L * 11

    def backward(skip_layer=None):
        """backward's report order replayed: head, layers last -> first, embeddings"""
        m.grad_ready_hook(off[t0], n)
        for li in reversed(range(L)):
            if li != skip_layer:
                m.grad_ready_hook(off[2 + li * 11], off[2 + li * 11 + 11])
        m.grad_ready_hook(off[0], off[2])
    coefs, norms, calls, nosync_calls = [], [], [], None
    for step in range(3):
        g = m.flat_grads()
        for p in m.parameters():
            if p.grad is None:
                p.grad = m._grad_views[[id(q) for q in m._param_order()].index(id(p))]
        if step == 2:      # gradient accumulation: the first micro-batch under no_sync() - nothing is reduced, no norm is accumulated
            g.copy_(_grad(n, step, rank, micro=1))
            assert opt.begin_norm_in_reducer(m, red)
            rec.norm_calls.clear()
            with red.no_sync():
                backward()
                red.finish()
            opt.end_norm_in_reducer(red)
            nosync_calls = list(rec.norm_calls)
            g.add_(_grad(n, step, rank))
        else:
            g.copy_(_grad(n, step, rank))
        assert opt.begin_norm_in_reducer(m, red)
        rec.norm_calls.clear()
        backward(skip_layer=0 if step == 1 else None)               # one layer unreported in step 1: step() must cover it
        red.finish()
        opt.end_norm_in_reducer(red)
        in_reducer = list(rec.norm_calls)
        if step == 1:   # the unreported range still holds this rank's own gradient: average it the plain way before step()
            lo, hi = off[2], off[2 + 11]
            g[lo:hi].mul_(1.0 / world)
            dist.all_reduce(g[lo:hi], op=dist.ReduceOp.SUM)
        opt.step()
        calls.append((in_reducer, list(rec.norm_calls)))
        coefs.append(opt.last_clip_coef.clone())
        norms.append(opt.last_grad_norm.clone())
    torch.save({"p0": p0, "p": m.flat_params().clone(), "coefs": coefs, "norms": norms, "calls": calls, "n": n, "nosync_calls": nosync_calls,
                "adamw_calls": rec.adamw_calls, "offsets": list(off), "sizes": [p.numel() for p in m._param_order()],
                "layer0": (off[2], off[2 + 11])}, os.path.join(out, f"c{rank}.pt"))
    dist.destroy_process_group()


def test_clipping_in_reducer_world2(tmp_path):
    sys.path.insert(0, ROOT)
    from oracle import maskgit_oracle as O
    world = 2
    port = 35500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rs = [torch.load(tmp_path / f"c{r}.pt") for r in range(world)]
    n = rs[0]["n"]
    # ranks with different gradients end with the same parameters, norms and coefficients, bit for bit
    assert torch.equal(rs[0]["p"], rs[1]["p"]) and torch.equal(rs[0]["p0"], rs[1]["p0"])
    for a, b in zip(rs[0]["coefs"] + rs[0]["norms"], rs[1]["coefs"] + rs[1]["norms"]):
        assert torch.equal(a, b)
    assert all(float(c) < 0.5 for c in rs[0]["coefs"]), "these steps are meant to clip"
    # single-process reference: torch's clipping + AdamW on the rank-averaged gradient (padding between parameters is no parameter)
    p = rs[0]["p0"].clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    mask = torch.zeros(n, dtype=torch.bool)
    for o, s in zip(rs[0]["offsets"], rs[0]["sizes"]):
        mask[o:o + s] = True
    for step in range(3):
        g = torch.zeros(n)
        for rank in range(world):
            gr = torch.sin(torch.arange(n, dtype=torch.float32) * 0.01 * (step + 1)) * 3.0 * (rank + 1)
            if step == 2:
                gr = torch.sin(torch.arange(n, dtype=torch.float32) * 0.01 * (step + 1) + 1) * 3.0 * (rank + 1) + gr
            g += gr * (1.0 / world)
        t = torch.nn.Parameter(torch.zeros(int(mask.sum())))
        t.grad = g[mask].clone()
        norm = torch.nn.utils.clip_grad_norm_([t], CLIP)
        assert abs(float(rs[0]["norms"][step]) - float(norm)) <= 2.0 ** -20 * float(norm)
        g = g * torch.clamp(CLIP / (norm + 1e-6), max=1.0)
        O.adamw_step(p, g, m, v, step + 1, 1e-2, 0.9, 0.99, 1e-8, 0.05)
    assert torch.allclose(rs[0]["p"], p, rtol=0, atol=2e-6), float((rs[0]["p"] - p).abs().max())
    # protocol: under no_sync() nothing was accumulated; in the reducer the ranges never overlap; step() covered exactly the rest;
    # the update ran once per step, over the whole buffer, with the device-side scale
    assert rs[0]["nosync_calls"] == []
    for step, (in_reducer, all_calls) in enumerate(rs[0]["calls"]):
        assert len(in_reducer) >= 2 and all_calls[:len(in_reducer)] == in_reducer
        ranges = sorted(all_calls)
        assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (step, ranges)
        covered = sum(e - b for b, e in in_reducer)
        assert covered == n if step != 1 else covered == n - (rs[0]["layer0"][1] - rs[0]["layer0"][0])
    assert rs[0]["adamw_calls"] == [(n, True)] * 3
