"""Gradient clipping by global norm inside muse.FusedAdamW / muse.TrainStep and muse.clip_grad_norm_: the HOST logic, without a GPU.
The HIP entry points are replaced by their CPU restatements (tests/grad_clip_cpu.py; the pattern of
test_fused_adamw_parameter_groups_host_logic) - what is under test is the protocol: which ranges the norm kernel is asked for, what
step() covers itself, what a raising backward leaves behind, what reaches ops.adamw_* with clipping on and off.  The kernels are tested on
the GPU (test_gpu_grad_clip.py)."""
import os
import sys

import pytest
import torch

import weights as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_clip_cpu import Recorder  # noqa: E402

HYPER = dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.05, eps=1e-8)


def _model(seed=5):
    import muse
    torch.manual_seed(seed)
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    m.set_compute_dtype(torch.float32)
    return m


def _set_grads(m, step, amp=1.0):
    g = m.flat_grads()
    n = g.numel()
    g.copy_(torch.sin(torch.arange(n, dtype=torch.float32) * 0.01 * (step + 1)) * amp)
    for p, gv in zip(m._param_order(), m._grad_views):
        p.grad = gv
    return g


def _recorder(monkeypatch):
    from muse import ops
    from oracle import maskgit_oracle as O
    return Recorder(O.adamw_step).install(ops, monkeypatch.setattr)


def _torch_twin_steps(m, start, grads_per_step, max_norm):
    """the reference's statements on twins that start from the flat parameters `start`: torch.nn.utils.clip_grad_norm_ +
    torch.optim.AdamW -> (parameters by name, [norms])"""
    names = {id(p): n for n, p in m.named_parameters()}
    twins = {names[id(p)]: torch.nn.Parameter(start[o:o + p.numel()].view(p.shape).clone()) for p, o in zip(m._param_order(), m._offsets)}
    ref = torch.optim.AdamW(list(twins.values()), **HYPER)
    names = {id(p): n for n, p in m.named_parameters()}
    norms = []
    for flat in grads_per_step:
        for p, o in zip(m._param_order(), m._offsets):
            twins[names[id(p)]].grad = flat[o:o + p.numel()].view(p.shape).clone()
        norms.append(torch.nn.utils.clip_grad_norm_(list(twins.values()), max_norm))
        ref.step()
    return twins, norms


def test_range_bookkeeping_unreported_ranges_and_torch_parity(monkeypatch):
    """three clipped steps: step 0 all in step(); step 1 with the norm accumulated range by range as backward reports (tail first), one
    part never reported and covered by step(); step 2 fully reported.  Every step: one finalize, ONE AdamW call over the whole buffer with
    the device-side scale, never a partial update; the norm calls tile the buffer exactly once; result = torch's clip + AdamW."""
    import muse
    rec = _recorder(monkeypatch)
    m = _model()
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=0.5, **HYPER)
    n = m.flat_params().numel()
    off = m._offsets
    mid, late = off[len(off) // 2], off[len(off) - 4]
    used, start = [], m.flat_params().clone()
    for step in range(3):
        g = _set_grads(m, step, amp=3.0)
        used.append(g.clone())
        rec.norm_calls.clear()
        if step >= 1:
            assert opt.begin_norm_in_backward(m) and m.grad_ready_hook is not None
            m.grad_ready_hook(late, n)
            if step == 2:
                m.grad_ready_hook(mid, late)
                m.grad_ready_hook(0, mid)
            opt.end_norm_in_backward(m)
            assert m.grad_ready_hook is None
        opt.step()
        assert float(opt.last_clip_coef) < 0.5, "this case is meant to clip"
        expect = {0: [(0, n)], 1: [(late, n), (0, late)], 2: [(late, n), (mid, late), (0, mid)]}[step]
        assert rec.norm_calls == expect, (step, rec.norm_calls)
        assert rec.adamw_calls[-1] == (n, True) and len(rec.adamw_calls) == step + 1 and rec.finalize_calls == step + 1
        assert torch.equal(g, used[-1]), "p.grad is left unscaled by the clipped step"
    twins, norms = _torch_twin_steps(m, start, used, 0.5)
    for k, p in m.named_parameters():
        assert float((p.detach() - twins[k].detach()).abs().max()) < 2e-6, k
    assert abs(float(opt.last_grad_norm) - float(norms[-1])) <= 2.0 ** -20 * float(norms[-1])
    assert not rec.scale_calls                                   # no write pass over the gradient


def test_norm_is_independent_of_the_cut(monkeypatch):
    """the same gradients, norm taken in one piece and in reported ranges: same norm, same coefficient, same parameters bit for bit"""
    import muse
    rec = _recorder(monkeypatch)
    res = []
    for cut in (False, True):
        m = _model()
        opt = muse.FusedAdamW(m.parameters(), max_grad_norm=0.5, **HYPER)
        n, off = m.flat_params().numel(), m._offsets
        _set_grads(m, 0, amp=3.0)
        if cut:
            assert opt.begin_norm_in_backward(m)
            for i in reversed(range(0, len(off), 5)):
                m.grad_ready_hook(off[i], off[i + 5] if i + 5 < len(off) else n)
            opt.end_norm_in_backward(m)
        opt.step()
        assert float(opt.last_clip_coef) < 0.5
        res.append((opt.last_grad_norm.clone(), opt.last_clip_coef.clone(), m.flat_params().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert len(rec.norm_calls) > 2


def test_a_range_that_cuts_a_parameter_is_refused(monkeypatch):
    import muse
    from muse import training
    _recorder(monkeypatch)
    m = _model()
    _set_grads(m, 0)
    st = training._FlatNormState.of(m)
    with pytest.raises(muse._hip.MuseHipError):
        st.accumulate(m.flat_grads(), m._offsets[1] + 1, m._offsets[3])
    with pytest.raises(muse._hip.MuseHipError):
        st.accumulate(m.flat_grads(), m._offsets[1], m._offsets[3] - 1 - (m._offsets[3] - m._offsets[2] - m._param_order()[2].numel()))


def test_raising_backward_leaves_a_retryable_step(monkeypatch):
    """backward raises after part of the norm was accumulated: nothing was applied, so - unlike the in-backward UPDATE, which poisons
    the optimizer (_partial_step) - the step can simply be taken again and equals an undisturbed one bit for bit"""
    import muse
    rec = _recorder(monkeypatch)
    m, m2 = _model(), _model()
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=0.5, **HYPER)
    opt2 = muse.FusedAdamW(m2.parameters(), max_grad_norm=0.5, **HYPER)
    n, off = m.flat_params().numel(), m._offsets
    before = m.flat_params().clone()
    _set_grads(m, 0, amp=3.0)
    assert opt.begin_norm_in_backward(m)
    m.grad_ready_hook(off[-3], n)
    opt.end_norm_in_backward(m, failed=True)               # what TrainStep's `finally` does when backward raised
    assert opt._norm_done is None and not getattr(opt, "_partial_step", False) and opt._step == 0
    assert torch.equal(m.flat_params(), before) and not rec.adamw_calls
    _set_grads(m, 0, amp=3.0)                               # the retried backward
    rec.norm_calls.clear()
    opt.step()
    assert rec.norm_calls == [(0, n)] and float(opt.last_clip_coef) < 0.5
    _set_grads(m2, 0, amp=3.0)
    opt2.step()
    assert torch.equal(m.flat_params(), m2.flat_params()) and torch.equal(opt._m, opt2._m) and torch.equal(opt._v, opt2._v)


def test_stale_reports_of_another_step_are_not_used(monkeypatch):
    """sums of squares delivered for a step that was never taken must not count for a later one"""
    import muse
    rec = _recorder(monkeypatch)
    m = _model()
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=0.5, **HYPER)
    n, off = m.flat_params().numel(), m._offsets
    _set_grads(m, 0, amp=3.0)
    opt.step()
    opt._norm_done = (1, [(off[4], n)])                     # left over from step 1; the next step is 2
    _set_grads(m, 1, amp=3.0)
    rec.norm_calls.clear()
    opt.step()
    assert rec.norm_calls == [(0, n)]


def test_pass_through_is_bit_identical_and_clipping_off_passes_no_new_keyword(monkeypatch):
    """max_grad_norm so large that coef == 1: same parameters and moments as without, bit for bit.  And with clipping off nothing new
    reaches ops.adamw_flat (a stand-in that only knows the old arguments keeps working) and no norm kernel is asked for."""
    import muse
    from muse import ops
    from oracle import maskgit_oracle as O
    rec = _recorder(monkeypatch)
    m = _model()
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=1e9, **HYPER)
    for step in range(3):
        _set_grads(m, step)
        opt.step()
        assert float(opt.last_clip_coef) == 1.0, "this case is meant to pass through"
    assert rec.finalize_calls == 3

    def old_adamw(p, g, m_, v, p_bf16, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        assert grad_scale == 1.0
        O.adamw_step(p, g, m_, v, int(step), lr, beta1, beta2, eps, weight_decay)

    def never(*a, **k):
        raise AssertionError("a norm kernel was asked for with clipping off")
    monkeypatch.setattr(ops, "adamw_flat", old_adamw)
    monkeypatch.setattr(ops, "gradnorm_flat", never)
    monkeypatch.setattr(ops, "gradnorm_finalize", never)
    m2 = _model()
    opt2 = muse.FusedAdamW(m2.parameters(), **HYPER)
    assert opt2.max_grad_norm is None
    assert not opt2.begin_norm_in_backward(m2) and m2.grad_ready_hook is None
    for step in range(3):
        _set_grads(m2, step)
        opt2.step()
    assert opt2.last_grad_norm is None
    assert torch.equal(m.flat_params(), m2.flat_params()) and torch.equal(opt._m, opt2._m) and torch.equal(opt._v, opt2._v)


def test_state_dict_keeps_torch_layout_and_the_update_never_runs_inside_backward(monkeypatch):
    import muse
    _recorder(monkeypatch)
    m, m2 = _model(), _model()
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=0.5, **HYPER)
    plain = muse.FusedAdamW(m2.parameters(), **HYPER)
    for o, mm in ((opt, m), (plain, m2)):
        _set_grads(mm, 0, amp=3.0)
        o.step()
    sd, sd0 = opt.state_dict(), plain.state_dict()
    assert sd.keys() == sd0.keys() and [g.keys() for g in sd["param_groups"]] == [g.keys() for g in sd0["param_groups"]]
    assert all("max_grad_norm" not in g for g in opt.param_groups) and "max_grad_norm" not in opt.defaults
    assert sd["state"].keys() == sd0["state"].keys() and all(sd["state"][i].keys() == sd0["state"][i].keys() for i in sd["state"])
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in m.parameters()], **HYPER)
    ref.load_state_dict(sd)
    assert int(ref.state_dict()["state"][0]["step"]) == 1
    # with clipping the update cannot start before the last gradient exists: the in-backward / in-reducer UPDATE refuses to arm
    assert opt.begin_step_in_backward(m) is False and m.grad_ready_hook is None
    opt.max_grad_norm = None                                 # settable as an attribute
    assert opt.begin_norm_in_backward(m) is False
    with pytest.raises(muse._hip.MuseHipError):
        muse.TrainStep(None, m, torch.optim.AdamW(m.parameters()), max_grad_norm=1.0)
    ts = muse.TrainStep(None, m, opt, max_grad_norm=2.0)
    assert opt.max_grad_norm == 2.0 and ts.optimizer is opt
    assert muse.TrainStep(None, m2, plain).optimizer.max_grad_norm is None


def test_clip_grad_norm_and_log_grad_norm_host_logic(monkeypatch):
    """muse.clip_grad_norm_ on a flat-buffer model: norm + in-place scale, == torch.nn.utils.clip_grad_norm_ on twins; then a plain
    step equals the clipped step.  log_grad_norm: the reference's formula (train_muse.py:1313)."""
    import muse
    from muse import training_utils as TU
    rec = _recorder(monkeypatch)
    m, m2 = _model(), _model()
    n = m.flat_params().numel()
    g = _set_grads(m, 0, amp=3.0)
    raw = g.clone()
    logged = TU.log_grad_norm(m)
    names = [k for k, _ in m.named_parameters()]
    assert sorted(logged) == sorted("grad_norm/" + k for k in names)
    for k, p in m.named_parameters():
        want = float(p.grad.double().norm() / p.grad.numel())
        assert abs(logged["grad_norm/" + k] - want) <= 2.0 ** -22 * want, k
    assert not rec.scale_calls
    norm, coef = muse.clip_grad_norm_(m, 0.5, return_coef=True)
    assert float(coef) < 0.5 and rec.scale_calls == [n]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in m._param_order()]
    for t, p, o in zip(twins, m._param_order(), m._offsets):
        t.grad = raw[o:o + p.numel()].view(p.shape).clone()
    tn = torch.nn.utils.clip_grad_norm_(twins, 0.5)
    assert abs(float(norm) - float(tn)) <= 2.0 ** -20 * float(tn)
    for t, p in zip(twins, m._param_order()):
        assert torch.allclose(p.grad, t.grad, rtol=2e-7, atol=0)
    assert torch.equal(g, raw * coef)                         # (padding included: one pass over the flat buffer)
    plain = muse.FusedAdamW(m.parameters(), **HYPER)
    plain.step()
    _set_grads(m2, 0, amp=3.0)
    opt2 = muse.FusedAdamW(m2.parameters(), max_grad_norm=0.5, **HYPER)
    opt2.step()
    assert torch.equal(opt2.last_clip_coef, coef) and torch.equal(m.flat_params(), m2.flat_params())
