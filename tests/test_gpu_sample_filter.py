"""GPU (-m gpu): top-k / nucleus (top-p) filtering inside the fused MaskGit decoding step (muse_sample_step_filtered, csrc/sampling.hip),
from the kernel up to generate2 and the pipelines.

The oracle for ids is oracle.maskgit_oracle.sample_step on logits whose filtered entries are -inf; the oracle for the kept set is
tests/sample_filter_cpu.py (float64), both applied to the f32 logits exactly as the kernel mixes them.  All kernel cases are seeded
CPU `randn * 2` logits with replayed draws, built the way tests/test_gpu_sampling.py::test_sample_step_vs_oracle builds them.

DELTA = 1e-4 is how close a code's float64 M_gt may come to top_p before the test stops saying on which side the kernel has to
put it.  It is derived, not measured: an f32 sum of at most 16384 non-negative terms totalling at most 1, added 256 per lane and then
by a wave tree, is off by at most about 256 * 2^-24 = 1.5e-5 relative, expf adds a few ulp per term, and 1e-4 is six times that.  (The
kernel sums the mass in 64-bit fixed point and stays well inside.)
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import sample_filter_cpu as F
import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTA = 1e-4
SCALE = 3.0
STEPS = ((4.5, None), (0.0, -1), (1.3, 3))      # (temperature, scheduled mask length; None: S // 2) of test_sample_step_vs_oracle

SMALL = (3, 16, 32, 48, False)
MID = (2, 64, 1024, 2048, True)
LIMIT = (1, 8, 16384, 16384, False)             # the vocabulary limit
WORK = (2, 256, 8192, 8192, True)               # the workload's vocabulary


def _ops():
    from muse import ops
    return ops


@functools.lru_cache(maxsize=None)
def _case(B, S, V, ld, guided, seed=None, quantum=None):
    """inputs of one step, the statements of test_sample_step_vs_oracle in its order; `quantum` rounds the logits to its multiples
    (ties).  Shared by the tests and never written to."""
    g = torch.Generator().manual_seed(1234 + S + V if seed is None else seed)
    cond = torch.randn(B, S, ld, generator=g) * 2.0
    unc = torch.randn(B, S, ld, generator=g) * 2.0 if guided else None
    if quantum:
        cond = torch.round(cond / quantum) * quantum
    mask_id = V + 7
    ids = torch.where(torch.rand(B, S, generator=g) < 0.7, torch.full((B, S), mask_id), torch.randint(0, V, (B, S), generator=g))
    ids[0, :] = mask_id
    q = torch.empty(B * S, V).exponential_(1, generator=g)
    u = torch.rand(B, S, generator=g)
    # the f32 logits the kernel filters, bit for bit: the compiled guidance mix is f32(cond - unc) and then ONE fused multiply-add
    # (the multiply and the add of uncond + scale * (cond - uncond) contract), restated in float64 - the product of two f32 values is
    # exact there, and the sum is for operands whose exponents lie within 2^27 of each other
    logits = ((unc.double() + SCALE * (cond - unc).double()).float() if guided else cond)[..., :V].contiguous()
    dev = dict(cond=cond.to(DEV), unc=unc.to(DEV) if guided else None, ids=ids.to(DEV), q=q.to(DEV), u=u.to(DEV))
    return dict(B=B, S=S, V=V, mask_id=mask_id, ids=ids, q=q, u=u, logits=logits, dev=dev)


def _step(c, temperature, sched, q=None, **kw):
    """one device step on the case's inputs -> CPU tensors (sampled, next, raw[, cutoff])"""
    d = c["dev"]
    out = _ops().sample_step(d["cond"], d["ids"], c["mask_id"], c["V"], temperature, c["S"] // 2 if sched is None else sched,
                             uncond_logits=d["unc"], guidance_scale=SCALE if d["unc"] is not None else 0.0,
                             noise_exp=d["q"] if q is None else q.to(DEV), noise_u=d["u"], want_raw=True, **kw)
    return tuple(t.cpu() for t in out)


def _assert_ids_equal_oracle(c, kept, got, temperature, sched, q=None):
    from oracle import maskgit_oracle as O
    raw_o, samp_o, next_o = O.sample_step(F.filtered_logits(c["logits"], kept), c["ids"], c["mask_id"], temperature,
                                          c["S"] // 2 if sched is None else sched, c["q"] if q is None else q, c["u"])
    samp, nxt, raw = got[:3]
    assert torch.equal(raw, raw_o) and torch.equal(samp, samp_o) and torch.equal(nxt, next_o), (temperature, sched)


def _margin(m_gt, k_set, top_p):
    """the float64 distance from top_p of the nearest M_gt among the codes the nucleus decides about"""
    return float((m_gt[k_set] - top_p).abs().min())


# ---- 1. filters off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, MID])
def test_filters_off_is_todays_step_bit_for_bit(shape):
    c = _case(*shape)
    V = c["V"]
    for temperature, sched in STEPS:
        plain = _step(c, temperature, sched)
        for kw in (dict(top_k=V), dict(top_p=1.0), dict(top_k=V, top_p=1.0), dict(top_k=V + 5)):
            got = _step(c, temperature, sched, want_cutoff=True, **kw)
            assert all(torch.equal(a, b) for a, b in zip(plain, got[:3])), (temperature, kw)
            assert bool(torch.isneginf(got[3]).all()) and got[3].shape == c["ids"].shape


# ---- 2. top_k, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, MID, LIMIT, WORK])
def test_top_k_cutoff_and_ids_are_exact(shape):
    c = _case(*shape)
    V, l = c["V"], c["logits"]
    srt = torch.sort(l, dim=-1, descending=True).values
    for i, k in enumerate(k for k in (1, 2, 63, 64, 65, V - 1) if k < V):      # the lane-count edges
        temperature, sched = STEPS[i % 3]
        got = _step(c, temperature, sched, top_k=k, want_cutoff=True)
        assert torch.equal(got[3], srt[..., k - 1]), k                           # the k-th largest f32 logit, exactly
        _assert_ids_equal_oracle(c, F.kept_mask(l, top_k=k)[0], got, temperature, sched)
        if k == 1:
            assert torch.equal(got[2], l.argmax(-1))                             # whatever the noise


def test_top_k_keeps_every_tie_at_the_kth_value():
    c = _case(*SMALL, quantum=0.25)
    l, k = c["logits"], 4
    vk = torch.sort(l, dim=-1, descending=True).values[..., k - 1]
    kept = F.kept_mask(l, top_k=k)[0]
    assert bool((kept.sum(-1) > k).any())                                        # rows where the k-th value is shared
    got = _step(c, 1.3, 3, top_k=k, want_cutoff=True)
    assert torch.equal(got[3], vk)
    _assert_ids_equal_oracle(c, kept, got, 1.3, 3)
    # samplable: the LAST code equal to the k-th value wins every row once its exponential draw is the smallest by far
    last = (l == vk[..., None]).int().cumsum(-1).argmax(-1)
    q = torch.ones_like(c["q"])
    q.view(c["B"], c["S"], -1).scatter_(-1, last[..., None], 1e-6)
    got = _step(c, 1.3, 3, q=q, top_k=k)
    assert torch.equal(got[2], last)
    _assert_ids_equal_oracle(c, kept, got, 1.3, 3, q=q)


# ---- 3. top_p, small and exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,top_p", [(4, 0.9), (None, 0.5)])
def test_top_p_small_kept_set_and_ids_are_exact(seed, top_p):
    c = _case(*SMALL, seed=seed)
    l = c["logits"]
    kept, m_gt = F.kept_mask(l, top_p=top_p)
    margin = _margin(m_gt, torch.ones_like(kept), top_p)
    print(f"seed {seed} top_p {top_p}: margin {margin:.3e}")
    assert margin >= DELTA
    for temperature, sched in STEPS:
        got = _step(c, temperature, sched, top_p=top_p, want_cutoff=True)
        assert torch.equal(l >= got[3][..., None], kept)
        _assert_ids_equal_oracle(c, kept, got, temperature, sched)


# ---- 4. top_p at the workload's vocabulary --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,top_p", [(WORK, 0.5), (WORK, 0.9), (LIMIT, 0.9)])
def test_top_p_workload_vocabulary(shape, top_p):
    c = _case(*shape)
    l = c["logits"]
    _, m_gt = F.kept_mask(l, top_p=top_p)
    band = ((m_gt - top_p).abs() <= DELTA).sum(-1)
    print(f"{shape} top_p {top_p}: at most {int(band.max())} codes per row inside the band")
    assert int(band.max()) <= 8                                                  # the band cannot swallow a wrong cutoff
    temperature, sched = STEPS[0]
    got = _step(c, temperature, sched, top_p=top_p, want_cutoff=True)
    kept = l >= got[3][..., None]                                                # a threshold set by construction
    assert bool(kept[m_gt < top_p - DELTA].all())
    assert not bool(kept[m_gt > top_p + DELTA].any())
    assert bool(kept.gather(-1, l.argmax(-1, keepdim=True)).all())
    _assert_ids_equal_oracle(c, kept, got, temperature, sched)


# ---- 5. combined ----------------------------------------------------------------------------------------------------------------------
def test_top_k_then_top_p_is_exact():
    c = _case(*SMALL)
    l, k, top_p = c["logits"], 8, 0.9
    k_set = F.kept_mask(l, top_k=k)[0]
    kept, m_gt = F.kept_mask(l, top_k=k, top_p=top_p)                            # the nucleus over the renormalised top-8
    margin = _margin(m_gt, k_set, top_p)
    print(f"top_k {k} top_p {top_p}: margin {margin:.3e}")
    assert margin >= DELTA
    assert not torch.equal(kept, k_set) and not torch.equal(kept, k_set & F.kept_mask(l, top_p=top_p)[0])
    for temperature, sched in STEPS:
        got = _step(c, temperature, sched, top_k=k, top_p=top_p, want_cutoff=True)
        assert torch.equal(l >= got[3][..., None], kept)
        _assert_ids_equal_oracle(c, kept, got, temperature, sched)


# ---- 6. device RNG --------------------------------------------------------------------------------------------------------------------
def test_top_k_with_the_device_rng():
    """the 16-code distribution of test_sample_step_device_rng, top_k=2: only codes 0 and 1, in the ratio 0.4 : 0.2"""
    ops = _ops()
    B, S, V = 64, 256, 16
    logits = torch.log(torch.tensor([0.4, 0.2, 0.1, 0.1] + [0.2 / 12] * 12)).repeat(B, S, 1).contiguous().to(DEV)
    ids = torch.full((B, S), 99, dtype=torch.long, device=DEV)
    a, na, _ = ops.sample_step(logits, ids, 99, V, 1.0, S // 2, seed=42, step=3, top_k=2)
    b, nb, _ = ops.sample_step(logits, ids, 99, V, 1.0, S // 2, seed=42, step=3, top_k=2)
    d, _, _ = ops.sample_step(logits, ids, 99, V, 1.0, S // 2, seed=43, step=3, top_k=2)
    assert torch.equal(a, b) and torch.equal(na, nb) and not torch.equal(a, d)
    freq = torch.bincount(a.flatten().cpu(), minlength=V).double() / (B * S)
    assert float(freq[2:].sum()) == 0.0
    assert abs(float(freq[0]) - 2 / 3) < 0.02 and abs(float(freq[1]) - 1 / 3) < 0.02


# ---- 7. generate2 ---------------------------------------------------------------------------------------------------------------------
def _class_model():
    import muse
    cfg = W.TRANSFORMER_TINY
    m = muse.MaskGitTransformer(**cfg)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), 11, "transformer"))
    m.to(DEV).eval().set_compute_dtype(torch.float32)
    return lambda seed, **kw: m.generate2(class_ids=torch.tensor([3, 7, 1], device=DEV), timesteps=4,
                                          generator=torch.Generator(device=DEV).manual_seed(seed), **kw)


def _uvit(golden_dir):
    import muse
    gp = np.load(os.path.join(golden_dir, "uvit_tiny.npz"))
    u = muse.MaskGiTUViT(**json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json"))))
    u.load_state_dict({k[len("param."):]: torch.from_numpy(gp[k]) for k in gp.files if k.startswith("param.")}, strict=True)
    u.to(DEV).eval()
    return u, np.load(os.path.join(golden_dir, "uvit_generate2_tiny.npz"))


def _uvit_model(golden_dir):
    u, gu = _uvit(golden_dir)
    args = [torch.from_numpy(gu[k]).to(DEV) for k in ("encoder_hidden_states", "cond_embeds", "micro_conds", "empty_embeds", "empty_cond_embeds")]

    def run(seed, temperature=2.0, **kw):
        # (MaskGiTUViT.generate2 ramps a scalar temperature down to 0.01, not to 0: the (start, end) form is what makes it 0 at every step)
        t = (temperature, temperature) if temperature == 0.0 else (temperature, 0.0)
        return u.generate2(*args, timesteps=4, temperature=t, guidance_scale=3.0, seq_len=int(gu["seq"]),
                           generator=torch.Generator(device=DEV).manual_seed(seed), **kw)
    return run


@pytest.mark.parametrize("model", ["class_conditional", "uvit"])
def test_generate2_takes_the_filters(golden_dir, model):
    run = _class_model() if model == "class_conditional" else _uvit_model(golden_dir)
    greedy = [run(seed, top_k=1, temperature=0.0) for seed in (5, 6)]
    assert torch.equal(greedy[0], greedy[1])                    # the only kept code wins whatever the draws, and no Gumbel noise
    free = [run(seed, temperature=2.0) for seed in (5, 6)]
    assert not torch.equal(free[0], free[1])
    eager = run(9, temperature=2.0, top_p=0.9, hip_graph=False)
    graph = run(9, temperature=2.0, top_p=0.9, hip_graph=True)
    assert torch.equal(eager, graph)
    assert not torch.equal(eager, run(9, temperature=2.0))      # the filter acts


# ---- 8. pipelines ---------------------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    ops = _ops()
    seen, orig = [], ops.sample_step

    def spy(*a, **k):
        seen.append((k.get("top_k"), k.get("top_p")))
        return orig(*a, **k)
    monkeypatch.setattr(ops, "sample_step", spy)
    return seen


def test_pipelines_hand_the_filters_to_every_step(golden_dir, monkeypatch):
    import muse
    seen = _spy(monkeypatch)
    v = muse.MaskGitVQGAN(**W.VQGAN_TINY)
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    pipe = muse.PipelineMuse(vae=v, transformer=m, is_class_conditioned=True).to(DEV)
    m.eval()
    pipe(class_ids=[3, 7], timesteps=3, top_k=5, top_p=0.8, output_type="np")
    assert seen == [(5, 0.8)] * 3
    del seen[:]
    pipe(class_ids=[3, 7], timesteps=3, topk_filter_thres=0.5, output_type="np")
    assert seen == [(None, None)] * 3                           # the reference's legacy argument stays without effect
    del seen[:]
    u, gu = _uvit(golden_dir)
    pipe_u = muse.PipelineMuse(vae=v, transformer=u).to(DEV)
    u.eval()
    t = lambda k: torch.from_numpy(gu[k])   # noqa: E731
    kw = dict(prompt_embeds=t("encoder_hidden_states"), pooled_embeds=t("cond_embeds"), empty_embeds=t("empty_embeds"),
              empty_pooled_embeds=t("empty_cond_embeds"), timesteps=3, guidance_scale=2.0, transformer_seq_len=int(gu["seq"]), output_type="np")
    pipe_u(top_k=5, top_p=0.8, **kw)
    assert seen == [(5, 0.8)] * 3
    del seen[:]
    pipe_u(topk_filter_thres=0.5, **kw)
    assert seen == [(None, None)] * 3
    del seen[:]
    # text-conditioned MaskGitTransformer on pre-computed states
    cfg = W.TRANSFORMER_TEXT_TINY
    mt = muse.MaskGitTransformer(**cfg)
    pipe_t = muse.PipelineMuse(vae=v, transformer=mt).to(DEV)
    mt.eval()
    _, _, enc = W.transformer_text_inputs(cfg, 2, 5, 3)
    pipe_t(prompt_embeds=enc, timesteps=3, guidance_scale=2.5, top_k=5, top_p=0.8, output_type="np")
    assert seen == [(5, 0.8)] * 3
    del seen[:]
    # the inpainting pipeline shares _generate
    pipe_i = muse.PipelineMuseInpainting(vae=v, transformer=m, is_class_conditioned=True).to(DEV)
    mask = torch.zeros(16, dtype=torch.bool)
    mask[[1, 5, 6]] = True
    pipe_i(torch.rand(3, 16, 16), mask, class_ids=3, timesteps=3, image_size=16, top_k=5, top_p=0.8, output_type="np")
    assert seen == [(5, 0.8)] * 3
