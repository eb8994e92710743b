"""GPU (-m gpu): soft-target training of the class-conditional MaskGitTransformer (config.training.use_soft_code_target):
the muse_soft_ce_fwd / muse_soft_ce_bwd kernels at config-B size against a float64 restatement, muse.training.soft_target_cross_entropy
and the soft-target TrainStep against the real reference's golden (tests/golden/soft_target_tiny.npz) and against the hand-written
loop body of training/train_maskgit_imagenet.py.

Tolerances: those of test_gpu_models.py - f32 loss rel <= 1e-4, gradients <= 1e-3 * max|grad| per tensor; bf16 loss rel <= 1e-3;
"f16" mode loss rel <= 1e-4 with no operand overflowed."""
import json
import os

import numpy as np
import pytest
import torch

import weights as W
from objective_cpu import f64_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "soft_target_tiny.npz"))


def _vq(seed):
    import muse
    v = muse.MaskGitVQGAN(**W.VQGAN_TINY)
    v.load_state_dict(W.fill_state_dict(W.vqgan_shapes(W.VQGAN_TINY), seed, "vqgan"))
    return v.to(DEV).eval()


def _transformer(cfg, seed, cd):
    import muse
    m = muse.MaskGitTransformer(**cfg)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), seed, "transformer"))
    m.to(DEV).train().set_compute_dtype(cd)
    return m


def _case(g, c):
    t = lambda k: torch.from_numpy(np.asarray(g[c + "." + k])).to(DEV)   # noqa: E731
    return json.loads(str(g[c + ".config"])), int(g[c + ".seed"]), float(g[c + ".temp"]), t


@pytest.mark.parametrize("case", ["tiny", "a_width"])
def test_soft_codes_and_masks_match_the_reference_golden(golden_dir, case):
    """get_soft_code: soft targets within 2e-5 of the reference's, argmin tokens bit-exact; prepare_inputs_and_labels with
    use_soft_code_target gives the recorded input_ids / labels from the recorded uniforms and hands the soft targets on"""
    import muse
    g = _golden(golden_dir)
    cfg, seed, temp, t = _case(g, case)
    v = _vq(seed)
    soft, tokens = v.get_soft_code(t("pixel_values"), temp=temp)
    assert float((soft - t("soft_targets")).abs().max()) < 2e-5
    assert torch.equal(tokens, t("tokens"))
    ids, labels, soft2, _ = muse.prepare_inputs_and_labels(v, t("pixel_values"), t("class_ids"), cfg["vocab_size"] - 1, 0.0,
                                                           t("timesteps"), t("noise"), use_soft_code_target=True, soft_code_temp=temp)
    assert torch.equal(ids, t("input_ids")) and torch.equal(labels, t("labels"))
    assert torch.equal(soft2, soft)
    # defaults: no soft targets, the same masks
    ids0, labels0, none, _ = muse.prepare_inputs_and_labels(v, t("pixel_values"), t("class_ids"), cfg["vocab_size"] - 1, 0.0,
                                                            t("timesteps"), t("noise"))
    assert none is None and torch.equal(ids0, ids) and torch.equal(labels0, labels)


@pytest.mark.parametrize("case", ["tiny", "a_width"])
@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16, "f16"])
def test_soft_target_loss_and_gradients_vs_reference_golden(golden_dir, case, cd):
    """the reference's loop body with muse parts: logits = model(input_ids); soft_target_cross_entropy; backward"""
    from muse.training import soft_target_cross_entropy
    g = _golden(golden_dir)
    cfg, seed, _, t = _case(g, case)
    m = _transformer(cfg, seed + 5, cd)
    logits = m(input_ids=t("input_ids"))
    loss = soft_target_cross_entropy(logits, t("labels"), t("soft_targets"))
    loss.backward()
    torch.cuda.synchronize()
    ref = float(g[case + ".loss"])
    lrel = abs(float(loss) - ref) / ref
    full = bool(g[case + ".full_grads"])
    errs = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got = p.grad.detach().float() if full else W.subsample(p.grad.detach().float(), 1024)
        errs[k] = float((got.cpu() - torch.from_numpy(g[case + ".grad." + k])).abs().max()) / float(g[case + ".absmax." + k])
    print(f"{case} {cd}: loss rel {lrel:.1e}, worst gradient {max(errs.values()):.1e}")
    if cd == torch.float32:
        assert lrel <= 1e-4, lrel
        assert max(errs.values()) <= 1e-3, errs
    elif cd == torch.bfloat16:
        assert lrel <= 1e-3, lrel
    else:
        overflowed, _ = m.f16_stats()
        assert overflowed == 0
        assert m.__dict__["_loss_rows"] == logits.shape[0] * logits.shape[1]   # the gradient scale sees the loss's row count
        assert lrel <= 1e-4, lrel
        assert max(errs.values()) <= 6e-3, errs


def _config_b_inputs(seed=3):
    B, S1, V, ld, K = 64, 257, 2025, 2032, 1024
    gen = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randn(B * S1, ld, device=DEV, generator=gen) * 2.0
    logits = buf[:, :V]
    soft = torch.softmax(torch.randn(B * (S1 - 1), K, device=DEV, generator=gen) * 1.5, dim=-1)
    labels = torch.randint(0, K, (B, S1), device=DEV, generator=gen)
    labels[torch.rand(B, S1, device=DEV, generator=gen) < 0.5] = -100
    labels[::2, 0] = -100
    labels[1::2, 0] = 7              # a label at the class position: still left out (position 0 is dropped)
    labels[5, 1:] = -100             # a sequence without any active row
    return logits, labels.view(-1).contiguous(), soft, S1, K


def _f64_reference(logits, labels, soft, S1, K, g):
    """the float64 restatement of the documented contract, shared with tests/test_gpu_objective_edges.py"""
    ref = f64_reference(logits, labels, soft, S1, K, g)
    return ref["loss"], ref["grad"], ref["active"]


def test_soft_ce_kernels_at_config_b_size():
    """[64, 257, 2025] logits in a 2032-wide buffer, soft rows [64 * 256, 1024], about half the labels -100: loss within 1e-6 rel of
    float64, gradient within 1e-6 * max|grad|, exact zeros outside the active [rows, :K] block, bit-identical reruns"""
    from muse import ops
    logits, labels, soft, S1, K = _config_b_inputs()
    gout = torch.tensor([1.75], device=DEV)
    loss_out, lse, psum = ops.soft_ce_fwd(logits, labels, soft, S1)
    dl = ops.soft_ce_bwd(logits, labels, soft, S1, lse, psum, loss_out, gout, width=2032)
    want, grad, active = _f64_reference(logits, labels, soft, S1, K, 1.75)
    torch.cuda.synchronize()
    assert int(loss_out[1]) == int(active.sum())
    assert abs(float(loss_out[0]) - want) <= 1e-6 * abs(want), (float(loss_out[0]), want)
    err = float((dl[:, :K].double() - grad).abs().max()) / float(grad.abs().max())
    print(f"soft CE at config B: loss rel {abs(float(loss_out[0]) - want) / want:.1e}, gradient {err:.1e}")
    assert err <= 1e-6, err
    assert not bool(dl[:, K:].any())                               # columns K .. ld
    assert not bool(dl[~active].any())                             # s = 0 rows and label -100 rows
    assert not bool(dl.view(64, S1, -1)[:, 0].any())
    # fixed reduction order: two runs give the same bits
    loss_out2, lse2, psum2 = ops.soft_ce_fwd(logits, labels, soft, S1)
    dl2 = ops.soft_ce_bwd(logits, labels, soft, S1, lse2, psum2, loss_out2, gout, width=2032)
    assert torch.equal(loss_out, loss_out2) and torch.equal(lse, lse2) and torch.equal(psum, psum2) and torch.equal(dl, dl2)
    # bf16 gradient output: the same values rounded, the same zeros
    db = ops.soft_ce_bwd(logits, labels, soft, S1, lse, psum, loss_out, gout, out_dtype=torch.bfloat16, width=2032)
    assert torch.equal(db, dl.to(torch.bfloat16))
    # a contiguous 2025-wide copy (rows not 16-byte aligned: the dword path) and the generic-K path
    lc = logits.contiguous()
    lo, ls_, ps = ops.soft_ce_fwd(lc, labels, soft, S1)
    dc = ops.soft_ce_bwd(lc, labels, soft, S1, ls_, ps, lo, gout)
    assert abs(float(lo[0]) - want) <= 1e-6 * abs(want) and float((dc[:, :K].double() - grad).abs().max()) <= 1e-6 * float(grad.abs().max())
    assert not bool(dc[:, K:].any()) and dc.shape == (logits.shape[0], 2025)
    K2 = 1000
    soft2 = torch.softmax(soft[:, :K2] * 3.0, dim=-1).contiguous()
    lo2, ls2, ps2 = ops.soft_ce_fwd(logits, labels, soft2, S1)
    d2 = ops.soft_ce_bwd(logits, labels, soft2, S1, ls2, ps2, lo2, gout, width=2032)
    want2, grad2, _ = _f64_reference(logits, labels, soft2, S1, K2, 1.75)
    assert abs(float(lo2[0]) - want2) <= 1e-6 * abs(want2)
    assert float((d2[:, :K2].double() - grad2).abs().max()) <= 1e-6 * float(grad2.abs().max())
    assert not bool(d2[:, K2:].any())


def test_soft_target_cross_entropy_function_and_its_checks():
    """the public function on the model's logits layout [B, S+1, V]: the kernels' loss and gradient, shaped like logits; shapes that
    do not match [B, S+1, V] / [B, S+1] / [B, S, K <= V] and non-f32 inputs are refused; no active row gives nan like the reference"""
    from muse._hip import MuseHipError
    from muse.training import soft_target_cross_entropy
    logits, labels, soft, S1, K = _config_b_inputs(11)
    x = logits.contiguous().view(64, S1, -1).detach().requires_grad_(True)
    lab, sft = labels.view(64, S1), soft.view(64, S1 - 1, K)
    loss = soft_target_cross_entropy(x, lab, sft)
    loss.backward()
    want, grad, _ = _f64_reference(logits, labels, soft, S1, K, 1.0)
    assert abs(float(loss) - want) <= 1e-6 * want
    assert x.grad.shape == x.shape
    assert float((x.grad.view(-1, 2025)[:, :K].double() - grad).abs().max()) <= 1e-6 * float(grad.abs().max())
    with pytest.raises(ValueError):
        soft_target_cross_entropy(x, lab[:, 1:], sft)                  # labels [B, S]
    with pytest.raises(ValueError):
        soft_target_cross_entropy(x, lab, sft[:, 1:])                  # soft targets [B, S - 1, K]: no broadcasting
    with pytest.raises(ValueError):
        soft_target_cross_entropy(x[:2], lab[:2], torch.full((2, S1 - 1, 2026), 1 / 2026, device=DEV))   # K > V
    with pytest.raises(ValueError):
        soft_target_cross_entropy(x, lab.int(), sft)
    with pytest.raises(MuseHipError):
        soft_target_cross_entropy(x.detach().to(torch.bfloat16), lab, sft)
    empty = torch.full_like(lab, -100)
    assert bool(torch.isnan(soft_target_cross_entropy(x.detach(), empty, sft)))


def _train_parts(cd, seed=700):
    import muse
    vcfg, tcfg = W.VQGAN_TINY, dict(W.TRANSFORMER_TINY)
    v = _vq(seed)
    m = _transformer(tcfg, seed + 1, cd)
    opt = muse.FusedAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, eps=1e-8)
    return v, m, opt


def _batch(seed, B=4):
    px = W.images(B, 16, seed).to(DEV)
    cls = torch.from_numpy(np.random.default_rng(seed + 1).integers(0, 10, size=B)).to(DEV)
    return px, cls, W.uniforms((B,), seed + 2).to(DEV), W.uniforms((B, 16), seed + 3).to(DEV)


def test_soft_target_train_step_matches_the_reference_loop_body():
    """f32: TrainStep(use_soft_code_target=True) leaves the parameters the hand-written loop body leaves (muse parts, FusedAdamW.step),
    bit for bit; with the next batch prefetched on the side stream the losses and parameters equal encoding inline"""
    import muse
    from muse.training import soft_target_cross_entropy
    b1, b2 = _batch(30), _batch(40)
    v, m, opt = _train_parts(torch.float32)
    step = muse.TrainStep(v, m, opt, use_soft_code_target=True, soft_code_temp=0.7)
    l1, _ = step(*b1)
    l2, _ = step(*b2)
    torch.cuda.synchronize()
    p_step = m.flat_params().clone()

    v, m, opt = _train_parts(torch.float32)
    losses = []
    for px, cls, t, nz in (b1, b2):
        ids, labels, soft, _ = muse.prepare_inputs_and_labels(v, px, cls, m.config.mask_token_id, 0.0, t, nz,
                                                              use_soft_code_target=True, soft_code_temp=0.7)
        logits = m(input_ids=ids)
        loss = soft_target_cross_entropy(logits, labels, soft)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(loss.detach())
    torch.cuda.synchronize()
    assert torch.equal(l1, losses[0]) and torch.equal(l2, losses[1])
    assert torch.equal(m.flat_params(), p_step)

    v, m, opt = _train_parts(torch.float32)
    step = muse.TrainStep(v, m, opt, use_soft_code_target=True, soft_code_temp=0.7)
    k1, _ = step(*b1, next_pixel_values=b2[0])
    k2, _ = step(*b2)
    torch.cuda.synchronize()
    assert torch.equal(k1, l1) and torch.equal(k2, l2)
    assert torch.equal(m.flat_params(), p_step)


def test_soft_target_train_step_bf16_optimizer_in_backward_and_descent():
    """bf16: AdamW armed inside backward gives the parameters of the step after backward; eight f32 steps on one batch lower the loss"""
    import muse
    b = _batch(50)

    def run(in_backward):
        v, m, opt = _train_parts(torch.bfloat16)
        step = muse.TrainStep(v, m, opt, use_soft_code_target=True, soft_code_temp=0.7)
        step.optimizer_in_backward = in_backward
        for _ in range(3):
            step(*b)
        torch.cuda.synchronize()
        return m.flat_params().clone()

    p0, p1 = run(False), run(True)
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    v, m, opt = _train_parts(torch.float32)
    step = muse.TrainStep(v, m, opt, use_soft_code_target=True, soft_code_temp=0.7)
    losses = [float(step(*b)[0]) for _ in range(8)]
    print("soft-target loss over eight steps:", [f"{x:.4f}" for x in losses])
    assert losses[-1] < losses[0] - 0.05, losses


def test_stochastic_soft_codes():
    """use_stochastic_code: one categorical draw per token from the soft codes - ids in [0, K), reproducible under torch.manual_seed,
    and at temp 10 different from the argmin on some tokens"""
    import muse
    v = _vq(80)
    px, cls, _, nz = _batch(81)
    t = torch.zeros(4, device=DEV)       # mask_prob 1: every token is a label

    def draw(temp, stochastic):
        _, labels, soft, _ = muse.prepare_inputs_and_labels(v, px, cls, 47, 0.0, t, nz, use_soft_code_target=True, soft_code_temp=temp,
                                                            use_stochastic_code=stochastic)
        return labels[:, 1:], soft

    hard, _ = draw(10.0, False)
    torch.manual_seed(5)
    a, soft = draw(10.0, True)
    torch.manual_seed(5)
    b, _ = draw(10.0, True)
    assert int(a.min()) >= 0 and int(a.max()) < W.VQGAN_TINY["num_embeddings"]
    assert torch.equal(a, b)
    assert bool((a != hard).any())
    assert torch.equal(hard, v.get_code(px))
