"""GPU (MI355X): muse.CLIPImageEncoder, muse.CLIPScorer / clip_scores and the kernels of csrc/clip_vision.hip against transformers' own
CLIP models on the CPU and against restatements written from the kernels' formulas (tests/clip_vision_cpu.py).

The tiny towers are built from CLIPVisionConfig under a fixed seed and made to behave like trained ones (2-D weights x 4, biases
~ N(0, 0.1)); 2 layers, intermediate = 4 x hidden, projection 48, batch 3.  Token counts 5, 50, 197, 257 and 577 are those of the
published B/32, B/16, L/14 and L/14@336 grids (and the smallest grid, 2 x 2)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_vision_cpu as CV
import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from muse import ops
    return ops


def native(hidden, heads, image, patch, act, dtype):
    import muse
    return muse.CLIPImageEncoder.from_transformers(CV.tower(hidden, heads, image, patch, act)[0]).to(DEV, dtype=dtype)


def native_outputs(o):
    out = {f"hidden_states[{i}]": h for i, h in enumerate(o.hidden_states)}
    out.update(last_hidden_state=o.last_hidden_state, pooler_output=o.pooler_output, image_embeds=o.image_embeds)
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("hidden,heads,image,patch", CV.CASES)
def test_f32_mode_against_the_oracle(hidden, heads, image, patch):
    """exact-f32 mode vs transformers on the CPU in f32: every hidden state + last_hidden_state + pooler_output + image_embeds.  Bar per
    tensor: 4 x the oracle's own float32-vs-float64 gap on the same input (max abs error over max |x|), computed here - the rule and
    factor of test_gpu_clip_text.py::test_f32_mode_against_the_oracle; the factor covers the summation order of the MFMA f32 chains.
    Measured on MI355X (hidden 128, 224 / 14 = 257 tokens, quick_gelu, per tensor): oracle f32-vs-f64 gap 0.95e-6 .. 4.39e-6 of max |x|,
    achieved error 1.05e-6 .. 4.72e-6, i.e. 0.7 .. 1.4 x the gap.  Over all 156 (case, activation, tensor) triples: gap 5.7e-7 .. 8.1e-6,
    achieved 7.9e-7 .. 1.18e-5; the worst ratio was 2.96 x (hidden 96, 28 / 14 = 5 tokens, quick_gelu, last_hidden_state: gap 9.0e-7,
    achieved 2.66e-6 - the maximum over 5 x 96 values, where the oracle's own gap is a small sample)."""
    for act in CV.ACTS:
        o32, o64, _ = CV.oracle(hidden, heads, image, patch, act)
        enc = native(hidden, heads, image, patch, act, torch.float32)
        out = enc(CV.make_pixels(image).to(DEV), output_hidden_states=True)
        assert len(out.hidden_states) == CV.LAYERS + 1
        got = native_outputs(out)
        for name, want in o32.items():
            assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
            bar, err = 4.0 * CV.gap(want, o64[name]), CV.gap(got[name], want)
            print(f"f32 {hidden}/{heads} {image}/{patch} {act} {name}: oracle f32-f64 gap {bar / 4:.3e} achieved {err:.3e} ratio {4 * err / bar:.2f}")
            assert err <= bar, (name, act, err, bar)
        assert torch.equal(out[0], out.image_embeds) and torch.equal(out[1], out.last_hidden_state)
        assert enc(CV.make_pixels(image).to(DEV)).hidden_states is None


@pytest.mark.parametrize("hidden,heads,image,patch", CV.CASES)
def test_bf16_mode_against_the_oracle(hidden, heads, image, patch):
    """bf16 mode vs the oracle's f32 run, the same tensors.  Bar per tensor: 2 x the oracle's own torch.autocast("cpu", bfloat16) gap
    from its f32 run on the same input, computed here (the rule of test_gpu_clip_text.py::test_bf16_mode_against_the_oracle: two
    bf16-operand, f32-accumulate pipelines with different rounding points).  The fused attention kernel runs once per layer, no score
    matrix and no f32 product exists, and the bf16 products are the patch embedding, four per layer and the projection.
    Measured on MI355X (hidden 128, 257 tokens, quick_gelu, per tensor): autocast gap 0.36e-2 .. 4.19e-2 of max |x|, achieved
    0.28e-2 .. 2.77e-2, i.e. 0.66 .. 1.2 x the gap.  Over all 156 triples: gap 0.30e-2 .. 4.19e-2, achieved 0.22e-2 .. 3.34e-2; the worst
    ratio was 1.78 x (hidden 64, 5 tokens, quick_gelu, last_hidden_state: gap 1.77e-2, achieved 3.16e-2)."""
    ops = _ops()
    for act in CV.ACTS:
        o32, _, o16 = CV.oracle(hidden, heads, image, patch, act)
        enc = native(hidden, heads, image, patch, act, torch.bfloat16)
        px = CV.make_pixels(image).to(DEV)
        enc(px)                                    # packs the operands outside the profiled run
        ops.profile_start()
        out = enc(px, output_hidden_states=True)
        names = [r[0] for r in ops.profile_stop(with_kind=True)]
        assert names.count("attn_fwd_bf16") == CV.LAYERS, names
        assert not any("softmax" in n for n in names) and not any(n.startswith("gemm_f32") for n in names), names
        assert sum(n.startswith("gemm_bf16") for n in names) == 4 * CV.LAYERS + 2, names
        got = native_outputs(out)
        for name, want in o32.items():
            assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
            bar, err = 2.0 * CV.gap(o16[name], want), CV.gap(got[name], want)
            print(f"bf16 {hidden}/{heads} {image}/{patch} {act} {name}: autocast gap {bar / 2:.3e} achieved {err:.3e} ratio {2 * err / bar:.2f}")
            assert err <= bar, (name, act, err, bar)


@pytest.mark.parametrize("P", [14, 16, 32])
def test_patch_rows_exactly(P):
    """muse_clip_patch_rows against unfold: f32 output bit for bit, bf16 output = .to(bfloat16) of it bit for bit, pad columns (K 588 ->
    592 at P 14) zero, and the bytes in front of and behind the output - allocated inside a sentinel-filled buffer - untouched.  The
    input is the ramp b 10^6 + c 10^5 + y 10^3 + x: a misplaced element names where it came from."""
    ops = _ops()
    K, Kp = 3 * P * P, (3 * P * P + 7) & ~7
    assert (Kp == 592) if P == 14 else (Kp == K)
    for G in (1, 2, 7, 16):
        for B in (1, 3):
            I = G * P
            px = CV.ramp(B, I)
            want = CV.patch_rows(px, P)
            rows, pad = B * G * G, 64
            for dtype, sentinel in ((torch.float32, -12345.0), (torch.bfloat16, -7.0)):
                buf = torch.full((rows * Kp + 2 * pad,), sentinel, dtype=dtype, device=DEV)
                out = buf[pad:pad + rows * Kp].view(rows, Kp)
                assert ops.clip_patch_rows(px.to(DEV), P, out=out) is out
                got = out.cpu()
                ref = want.to(dtype)
                assert torch.equal(got[:, :K].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   ref.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (P, G, B, dtype)
                assert bool((got[:, K:] == 0).all())
                assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + rows * Kp:] == sentinel).all()), (P, G, B, dtype)
            fresh = ops.clip_patch_rows(px.to(DEV), P, torch.bfloat16)
            assert fresh.dtype == torch.bfloat16 and fresh.shape == (rows, Kp) and torch.equal(fresh.cpu()[:, :K], want.to(torch.bfloat16))


@pytest.mark.parametrize("H", [64, 96, 1024])
@pytest.mark.parametrize("T", [2, 5, 50, 257])
def test_embed_ln_against_float64(T, H):
    """muse_clip_vision_embed_ln against the formula in float64.  Bar: 4 x the gap of torch's own f32 F.layer_norm (on the f32 sum
    class | patch + pos) from that float64 value.  Separately the row mapping: LayerNorm weight 1 / bias 0, zero patch embeddings and a
    position table that is a permutation of distinct integers make every (b, t) row a known, pairwise distinct vector - the class row
    (class + pos[0]) differs from pos[0] alone and from every patch row."""
    ops = _ops()
    B, eps = 3, 1e-5
    g = torch.Generator().manual_seed(7 * T + H)
    patch, cls, pos = torch.randn(B * (T - 1), H, generator=g), torch.randn(H, generator=g), torch.randn(T, H, generator=g) * 0.5
    w, b = 1.0 + 0.3 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    want, _ = CV.embed_ln(patch, cls, pos, w, b, eps, B)
    _, x32 = CV.embed_ln(patch, cls, pos, w, b, eps, B, torch.float32)
    torch32 = F.layer_norm(x32, (H,), w, b, eps)
    got = ops.clip_vision_embed_ln(*(t.to(DEV) for t in (patch, cls, pos, w, b)), eps, B)
    assert got.dtype == torch.float32 and got.shape == (B * T, H)
    bar, err = 4.0 * CV.gap(torch32, want), CV.gap(got, want)
    print(f"embed_ln T={T} H={H}: torch f32-f64 gap {bar / 4:.3e} achieved {err:.3e} ratio {4 * err / bar:.2f}")
    assert err <= bar
    # the row mapping
    pos = torch.randperm(T * H, generator=g).view(T, H).float()
    cls = torch.arange(H).flip(0).float() * float(T)
    zero, one, nil = torch.zeros(B * (T - 1), H), torch.ones(H), torch.zeros(H)
    want, _ = CV.embed_ln(zero, cls, pos, one, nil, eps, B)
    decoy, _ = CV.embed_ln(zero[:T - 1], torch.zeros(H), pos, one, nil, eps, 1)              # row 0 = pos[0] without the class token
    rows = torch.cat([want[:T], decoy[:1]])
    dist = (rows[:, None] - rows[None]).abs().amax(-1) + torch.eye(T + 1) * 9.0
    assert float(dist.min()) > 0.1                                                   # the candidates are pairwise distinct
    got = ops.clip_vision_embed_ln(*(t.to(DEV) for t in (zero, cls, pos, one, nil)), eps, B).cpu().double()
    assert float((got - want).abs().max()) < 1e-4
    for bt in range(B * T):
        assert int((rows - got[bt]).abs().amax(-1).argmin()) == bt % T, bt


RESIZES = [(256, 224), (512, 224), (64, 28), (20, 28), (225, 224)]


@functools.lru_cache(maxsize=None)
def resize_case(R, I):
    img = CV.smooth_images(CV.BATCH, R)
    return img, CV.resize_norm(img, I), CV.resize_norm(img.double(), I)


@pytest.mark.parametrize("R,I", RESIZES)
def test_resize_bicubic_norm_against_aten(R, I):
    """muse_resize_bicubic_norm_f32 against F.interpolate(mode="bicubic", antialias=True, align_corners=False) + normalisation on the CPU.
    Bar: 4 x the f32-vs-f64 gap of the oracle itself.  Image 0 is a step edge: the cubic overshoots, the oracle holds values outside
    the normalised images of 0 and 1, and so does the kernel - nothing clamps."""
    ops = _ops()
    img, o32, o64 = resize_case(R, I)
    got = ops.resize_bicubic_norm(img.to(DEV), I, CV.MEAN, CV.STD)
    assert got.dtype == torch.float32 and got.shape == (CV.BATCH, 3, I, I)
    bar, err = 4.0 * CV.gap(o32, o64), CV.gap(got, o32)
    print(f"resize {R}->{I}: oracle f32-f64 gap {bar / 4:.3e} achieved {err:.3e} ratio {4 * err / bar:.2f}")
    assert err <= bar
    lo, hi = CV.normalise(torch.zeros(1, 3, 1, 1)), CV.normalise(torch.ones(1, 3, 1, 1))
    below, above = (o32 < lo - 1e-3), (o32 > hi + 1e-3)
    assert bool(below.any()) and bool(above.any())                                   # the oracle overshoots on both sides ...
    g = got.cpu()
    assert bool((g[below] < lo.expand_as(g)[below]).all()) and bool((g[above] > hi.expand_as(g)[above]).all())       # ... and so does the kernel


@pytest.mark.parametrize("R", [28, 224])
def test_resize_to_the_same_size_is_the_normalisation_bit_for_bit(R):
    ops = _ops()
    img = CV.smooth_images(2, R, seed=1)
    got = ops.resize_bicubic_norm(img.to(DEV), R, CV.MEAN, CV.STD)
    assert torch.equal(bits(got), bits(CV.normalise(img)))
    other = ops.resize_bicubic_norm(img.to(DEV), R, (0.5, 0.25, 0.125), (0.3, 0.7, 1.1))
    assert torch.equal(bits(other), bits(CV.normalise(img, (0.5, 0.25, 0.125), (0.3, 0.7, 1.1))))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hidden,heads,image,patch", [(64, 2, 28, 14), (96, 3, 224, 32), (128, 2, 224, 14)])
def test_batch_permutation_bit_for_bit(hidden, heads, image, patch, dtype):
    """permuting the batch permutes every output bit for bit, in both modes; no output lane is NaN / inf"""
    enc = native(hidden, heads, image, patch, "quick_gelu", dtype)
    px = CV.make_pixels(image).to(DEV)
    perm = torch.tensor([2, 0, 1], device=DEV)
    a = native_outputs(enc(px, output_hidden_states=True))
    b = native_outputs(enc(px[perm].contiguous(), output_hidden_states=True))
    for name in a:
        assert bool(torch.isfinite(a[name]).all()), name
        assert torch.equal(a[name][perm], b[name]), name


@functools.lru_cache(maxsize=None)
def clip_pair():
    """a tiny CLIPModel (both towers, trained-like) on the CPU in f32 and f64; 3 images and 3 captions"""
    import copy
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(21)
    text = dict(vocab_size=600, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
                bos_token_id=598, eos_token_id=599, pad_token_id=599)
    m = CV._trained_like(CLIPModel(CLIPConfig(text_config=text, vision_config=CV.vision_config(64, 2, 28, 14).to_dict(),
                                              projection_dim=CV.PROJ)).eval()).requires_grad_(False)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(3, 598, (3, 12), generator=g)
    ids[:, 0] = 598
    ids[0, 5:], ids[1, 11], ids[2, 2:] = 599, 599, 599
    return m, copy.deepcopy(m).double(), CV.smooth_images(3, 64, seed=2), ids


def clip_run(m, px, ids):
    """(image_embeds, text_embeds) as the towers return them, un-normalised, and CLIPModel.forward's logits_per_image"""
    with torch.no_grad():
        ie = m.visual_projection(m.vision_model(pixel_values=px).pooler_output)
        te = m.text_projection(m.text_model(input_ids=ids).pooler_output)
        return ie, te, m(input_ids=ids, pixel_values=px).logits_per_image


def test_scorer_against_clip_model():
    """muse.CLIPScorer (GPU resize -> image tower -> text tower -> normalised similarity) against transformers' CLIPModel on the CPU,
    fed with the CPU resize of the same images.  Bars: the f32-mode rule of test_f32_mode_against_the_oracle (4 x the oracle's own
    f32-vs-f64 gap of the same tensor)."""
    import muse
    m32, m64, imgs, ids = clip_pair()
    ie32, te32, l32 = clip_run(m32, CV.resize_norm(imgs, 28), ids)
    _, _, l64 = clip_run(m64, CV.resize_norm(imgs.double(), 28), ids)
    bar = 4.0 * CV.gap(l32, l64)
    enc = muse.CLIPImageEncoder.from_transformers(m32).to(DEV)
    txt = muse.CLIPTextEncoder.from_transformers(_text_tower(m32)).to(DEV)
    assert float(enc.logit_scale) == float(m32.logit_scale)
    scorer = muse.CLIPScorer(enc, txt)
    s = scorer(imgs.to(DEV), input_ids=ids[:2].to(DEV))                      # 3 images x 2 captions
    assert s.logits_per_image.shape == s.cosine.shape == (3, 2) and s.logits_per_image.dtype == torch.float32
    err = CV.gap(s.logits_per_image, l32[:, :2])
    print(f"scorer logits_per_image: oracle f32-f64 gap {bar / 4:.3e} achieved {err:.3e} ratio {4 * err / bar:.2f}")
    assert err <= bar
    assert float(s.cosine.abs().max()) <= 1.0 + bar
    assert CV.gap(s.cosine * float(m32.logit_scale.exp()), l32[:, :2]) <= bar
    with pytest.raises(ValueError):
        s.pairwise()
    sq = scorer(imgs.to(DEV), input_ids=ids.to(DEV))                         # 3 x 3
    assert torch.equal(sq.pairwise(), torch.diagonal(sq.cosine)) and sq.pairwise().shape == (3,)
    assert torch.equal(sq.cosine[:, :2], s.cosine)
    # pixel_values bypass the resize stage; pre-computed text_embeds and a plain callable bypass the text tower
    via_px = scorer(pixel_values=CV.resize_norm(imgs, 28).to(DEV), text_embeds=sq.text_embeds)
    assert CV.gap(via_px.logits_per_image, l32) <= bar
    via_fn = muse.CLIPScorer(enc, lambda i: sq.text_embeds)(imgs.to(DEV), input_ids=ids)
    assert torch.equal(via_fn.logits_per_image, sq.logits_per_image)
    # clip_scores on the oracle's own embeddings
    cos, logits = muse.clip_scores(ie32.to(DEV), te32.to(DEV), m32.logit_scale)
    err = CV.gap(logits, l32)
    print(f"clip_scores on the oracle's embeds: achieved {err:.3e}")
    assert err <= bar and CV.gap(cos * float(m32.logit_scale.exp()), l32) <= bar
    cos0, logits0 = muse.clip_scores(ie32.to(DEV), te32.to(DEV))             # default multiplier 1 / 0.07
    assert torch.equal(cos0, cos) and CV.gap(logits0, cos.cpu() / 0.07) <= bar
    # a zero embedding: NaN in its row only
    z = ie32.clone()
    z[1] = 0.0
    cz, lz = muse.clip_scores(z.to(DEV), te32.to(DEV), m32.logit_scale)
    for t, ref in ((cz, cos), (lz, logits)):
        assert bool(torch.isnan(t[1]).all()) and torch.equal(t[[0, 2]], ref[[0, 2]])


def _text_tower(clip):
    """the text half of a CLIPModel as a CLIPTextModelWithProjection (what muse.CLIPTextEncoder.from_transformers takes)"""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    t = CLIPTextModelWithProjection(CLIPTextConfig(**{**clip.config.text_config.to_dict(), "projection_dim": clip.config.projection_dim})).eval()
    sd = clip.state_dict()
    t.load_state_dict({k: sd[k] for k in t.state_dict()})
    return t


def test_l2_normalize_rows():
    """x / ||x|| per row against torch in f64, with the float multiplier, with the device log-multiplier, in place; cols not a multiple
    of 64 or 4"""
    ops = _ops()
    for N, D in ((1, 3), (5, 48), (7, 130), (3, 768)):
        x = torch.randn(N, D, generator=torch.Generator().manual_seed(N * D))
        want = x.double() / x.double().norm(dim=-1, keepdim=True)
        ref = x / x.norm(dim=-1, keepdim=True)
        bar = 4.0 * max(CV.gap(ref, want), 2.0 ** -24)
        assert CV.gap(ops.l2_normalize_rows(x.to(DEV)), want) <= bar
        assert CV.gap(ops.l2_normalize_rows(x.to(DEV), mult=3.0), 3.0 * want) <= bar
        ls = torch.tensor([1.25], device=DEV)
        assert CV.gap(ops.l2_normalize_rows(x.to(DEV), log_mult=ls), float(np.exp(1.25)) * want) <= bar
        y = x.to(DEV)
        assert ops.l2_normalize_rows(y, out=y) is y and torch.equal(y, ops.l2_normalize_rows(x.to(DEV)))


def test_pipeline_output_type_pt_feeds_the_scorer():
    """PipelineMuse(..., output_type="pt") on the tiny class-conditional model: the clamped [B, 3, H, W] f32 device tensor, equal to
    output_type="np" bit for bit after permute / cpu / numpy; a CLIPScorer behind it returns a finite [B, Bt] matrix"""
    import muse
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(W.TRANSFORMER_TINY), 830, "transformer"))
    pipe = muse.PipelineMuse(vae=muse.MaskGitVQGAN(**W.VQGAN_TINY), transformer=m, is_class_conditioned=True).to(DEV, dtype=torch.float32)
    cls = torch.tensor([3, 7], device=DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)   # noqa: E731
    a = pipe(class_ids=cls.clone(), timesteps=3, generator=gen(), output_type="np")
    t = pipe(class_ids=cls.clone(), timesteps=3, generator=gen(), output_type="pt")
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.shape == (2, 3) + a.shape[1:3]
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    assert np.array_equal(t.permute(0, 2, 3, 1).cpu().numpy(), a)
    scorer = muse.CLIPScorer(native(64, 2, 28, 14, "quick_gelu", torch.float32))
    te = torch.randn(3, CV.PROJ, generator=torch.Generator().manual_seed(1)).to(DEV)
    s = scorer(t, text_embeds=te)
    assert s.cosine.shape == s.logits_per_image.shape == (2, 3) and bool(torch.isfinite(s.logits_per_image).all())
    assert float(s.cosine.abs().max()) <= 1.0 + 1e-5
