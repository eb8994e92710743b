"""Attention dropout inside the bf16x3 / f16 attention cores (csrc/attention3.hip: muse_attention_x3_drop_fwd / _bwd).

Geometry: B = 2, 3 heads of 64.  Shapes: 256 x 65 / 77 / 96 (NKB = 3, masked and full last block), 256 x 225 / 256 (NKB = 8), 512 x 77 (q0
non-zero: one launch per 256-query block), 512 x 512 and 256 x 768 (block pairs merged by their log-sum-exps: k0 non-zero).
  (a) every keep bit of every (bh, q, k) read back from the forward, the dQ phase and the dK / dV phase with one-hot operands (q = 0 makes
      the probabilities uniform and strictly positive, so "non-zero" / "the larger of two values" is exact), against tests/philox_cpu.py with
      5i's contract e = (bh * S_q + q) * round_up(S_kv, 8) + k, at p = 0.5 and 0.1, offsets 3 << 40 and 2^32 - 5;
  (b) seeded random operands (tests/attention_x3_dropout_cpu.random_case) against float64 with the CPU mask, per element over the terms within
      4 * E_REF_X3_DROP / E_REF_H16_DROP (that file's models of these kernels; lse absolute), both drop settings; lse additionally within the
      p = 0 bound of the cores and, where p = 0 takes the same launches (S_kv <= 256), the p = 0 kernel's lse bit for bit;
  (c) fused versus materialised (uniform P, muse_dropout with the same (seed, offset), P V): the identical zero pattern of the context probes;
  (d) the operand planes / half image written next to the f32 context equal its split / cast bit for bit."""
import numpy as np
import pytest
import torch

import attention_cpu as A
import attention_dropout_cpu as D
import attention_x3_dropout_cpu as X
import philox_cpu as PH

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NH, HD = 2, 3, 64
H = NH * HD
SHAPES = [(256, 65), (256, 77), (256, 96), (256, 225), (256, 256), (512, 77), (512, 512), (256, 768)]
DROPS = [(0.5, 0x1234567, 3 << 40), (0.1, (1 << 61) + 99, 2 ** 32 - 5)]


def _ops():
    from muse import ops
    return ops


def scope(ops, mode, backward=False, grad_scale=2.0 ** 10):
    if mode == "f16":
        im = ops.F16Images()
        im.backward = backward
        im.set_grad_scale(grad_scale)
        return ops.f32_gemms_as_f16(True, im), im
    im = ops.X3Images()
    im.backward = backward
    return ops.f32_gemms_as_bf16x3(True, im), im


def keep_mask(Sq, Skv, p, seed, offset):
    ld = (Skv + 7) // 8 * 8
    return PH.dropout_keep(B * NH * Sq * ld, p, seed, offset).reshape(B * NH, Sq, ld)[:, :, :Skv]


def heads_first(t, S):
    """[B * S, H] -> [B * NH, S, HD]"""
    return t.view(B, S, NH, HD).permute(0, 2, 1, 3).reshape(B * NH, S, HD)


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("Sq,Skv", SHAPES)
def test_every_keep_bit_from_all_three_phases(mode, Sq, Skv):
    ops = _ops()
    alpha = 0.125
    q = torch.zeros((B * Sq, H), device=DEV)
    for p, seed, offset in DROPS:
        keep = keep_mask(Sq, Skv, p, seed, offset)
        s = 1.0 / (1.0 - p)
        drop = (p, seed, offset, (Skv + 7) // 8 * 8)
        a_q = torch.from_numpy((keep * s).mean(-1)).to(DEV)                              # [B*NH, Sq]: dO . O of the dQ probe
        got_f, got_v, got_q = (np.zeros_like(keep) for _ in range(3))
        for c0 in range(0, Skv, HD):
            n = min(HD, Skv - c0)
            hot = torch.zeros((Skv, HD))
            hot[c0 + torch.arange(n), torch.arange(n)] = 1.0
            hot_kv = hot.repeat(B, NH).to(DEV)                                            # [B * Skv, H]: every head the same one-hot chunk
            rows1 = torch.zeros((B * Skv, H), device=DEV)
            rows1.view(B * Skv, NH, HD)[:, :, 0] = 1.0                                     # every V row sums to 1 per head
            with scope(ops, mode)[0]:
                ctx, lse = ops.attention_x3_fwd(q, hot_kv, hot_kv, B, Sq, Skv, NH, HD, alpha, drop=drop)
            got_f[:, :, c0:c0 + n] = heads_first(ctx, Sq)[:, :, :n].cpu().numpy() != 0.0
            # (c) the materialised route with the same (seed, offset): uniform P in the [B * nh, Sq, round_up(Skv, 8)] tensor, muse_dropout, P V -
            # the identical zero pattern of the context probe
            Pm = torch.zeros((B * NH, Sq, drop[3]), device=DEV)
            Pm[:, :, :Skv] = 1.0 / Skv
            ctx_m = ops.dropout(Pm, p, seed, offset)[:, :, :Skv] @ heads_first(hot_kv, Skv)
            assert torch.equal(ctx_m != 0.0, heads_first(ctx, Sq) != 0.0), f"{mode} {Sq} x {Skv} p {p}: fused and materialised context probes differ"
            # dQ phase: dO = ones, V rows summing to 1 -> dP = 1, dS = (keep s - a_q) / Skv, dQ[q, d] = alpha dS[q, c0 + d]
            with scope(ops, mode)[0]:
                ctx1, lse1 = ops.attention_x3_fwd(q, hot_kv, rows1, B, Sq, Skv, NH, HD, alpha, drop=drop)
            do = torch.zeros((B * Sq, H), device=DEV)
            do.view(B * Sq, NH, HD)[:, :, 0] = 1.0                                         # dO . V[k] = 1 for every key
            with scope(ops, mode, True)[0]:
                dq, _, _ = ops.attention_x3_bwd(q, hot_kv, rows1, ctx1, do, lse1, B, Sq, Skv, NH, HD, alpha, drop=drop)
            val = heads_first(dq, Sq)[:, :, :n] * (Skv / alpha) + a_q[:, :, None]          # keep s (kept) or 0 (dropped)
            got_q[:, :, c0:c0 + n] = (val > 0.5 * s).cpu().numpy()
        # dK / dV phase: dO one-hot over a chunk of queries -> dV[k, d] = P_dropped[q0 + d, k]
        v0 = torch.zeros((B * Skv, H), device=DEV)
        k0 = torch.zeros((B * Skv, H), device=DEV)
        with scope(ops, mode)[0]:
            ctx0, lse0 = ops.attention_x3_fwd(q, k0, v0, B, Sq, Skv, NH, HD, alpha, drop=drop)
        for c0 in range(0, Sq, HD):
            hot = torch.zeros((Sq, HD))
            hot[c0 + torch.arange(HD), torch.arange(HD)] = 1.0
            do = hot.repeat(B, NH).to(DEV)
            with scope(ops, mode, True)[0]:
                _, _, dv = ops.attention_x3_bwd(q, k0, v0, ctx0, do, lse0, B, Sq, Skv, NH, HD, alpha, drop=drop)
            got_v[:, c0:c0 + HD, :] = (heads_first(dv, Skv) != 0.0).permute(0, 2, 1).cpu().numpy()
        for name, got in (("forward", got_f), ("dQ", got_q), ("dK/dV", got_v)):
            bad = int((got != keep).sum())
            assert bad == 0, f"{mode} {Sq} x {Skv} p {p} offset {offset}: {bad} keep bits differ in the {name} phase"


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("Sq,Skv", SHAPES)
def test_random_operands_against_float64_with_the_cpu_mask(mode, Sq, Skv):
    """(b): per element over the terms within 4 * E_REF_X3_DROP / E_REF_H16_DROP (tests/attention_x3_dropout_cpu.py: the CPU models of these
    kernels against the same float64 reference), lse absolute - and lse also within the p = 0 bound of the cores (4 * E_REF_X3 / E_REF_H16 of
    tests/test_gpu_attention_x3_edges.py): dropout must not touch it"""
    import test_gpu_attention_x3_edges as E0
    ops = _ops()
    m = "h16" if mode == "f16" else "x3"
    c = X.random_case(Sq, Skv, m)
    q, k, v, do = (c[n].to(DEV) for n in ("q", "k", "v", "do"))
    alpha = float(c["alpha"])
    for p, offset in X.DROPS:
        keep = X.keep_mask(Sq, Skv, p, offset)
        drop = (p, X.SEED, offset, (Skv + 7) // 8 * 8)
        with scope(ops, mode, grad_scale=1.0)[0]:
            ctx, lse = ops.attention_x3_fwd(q, k, v, B, Sq, Skv, NH, HD, alpha, drop=drop)
            ctx_p0, lse_p0 = ops.attention_x3_fwd(q, k, v, B, Sq, Skv, NH, HD, alpha)
        with scope(ops, mode, True, grad_scale=1.0)[0]:
            dq, dk, dv = ops.attention_x3_bwd(q, k, v, ctx, do, lse, B, Sq, Skv, NH, HD, alpha, drop=drop)
        if Skv <= 256:        # the same launches as p = 0: row maximum, row sum and lse come from the undropped P, bit for bit
            assert torch.equal(lse, lse_p0)
        lse_rows = (lse if lse.dim() == 2 else lse.permute(1, 0, 2).reshape(B * NH, Sq)).cpu()
        out = dict(ctx=ctx.cpu(), lse=lse_rows, dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
        ref = D.reference(c, keep, p)
        A.check_random(c, out, ref, X.e_ref_for(m, Sq, Skv), tag=f"random {mode} drop {Sq}x{Skv} p={p}")
        A.check_random(c, dict(lse=lse_rows), ref, E0.e_ref_for(E0.E_REF_H16 if m == "h16" else E0.E_REF_X3, Sq, Skv), tag=f"lse at the p = 0 bound {mode} {Sq}x{Skv}")
        assert float((ctx - ctx_p0).abs().max()) > 1e-2                       # (the mask matters)


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("Sq,Skv", [(256, 77), (256, 256), (512, 77), (512, 512)])
def test_operand_image_next_to_the_context_is_its_split_or_cast(mode, Sq, Skv):
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn((B * S_, H), generator=g).to(DEV) for S_ in (Sq, Skv, Skv))
    p, seed, offset = DROPS[0]
    sc, im = scope(ops, mode)
    with sc:
        ctx, _ = ops.attention_x3_fwd(q, k, v, B, Sq, Skv, NH, HD, 0.125, drop=(p, seed, offset, (Skv + 7) // 8 * 8))
        misses = im.misses
        seen = im.image(ctx, 1.0) if mode == "f16" else ops.split_planes(ctx)
        assert im.misses == misses
        assert torch.equal(seen, ops.cast_to_f16(ctx) if mode == "f16" else ops._split_planes_now(ctx))
