"""GPU (MI355X): muse.CLIPTextEncoder and the kernels of csrc/clip_text.hip and csrc/attention_enc.hip against transformers' own CLIP text model on the CPU.

The tiny towers are built here from CLIPTextConfig under a fixed seed and made to behave like trained ones (2-D non-embedding
weights x 4, biases ~ N(0, 0.1)): the softmax is not flat, so a missing or misplaced mask shows.  3 layers, intermediate = 4 x hidden,
vocab 600, batch 3.  Ids: BOS first; the EOS / pad fill (id 599, the largest) starts at position 10 in row 0 (position 4 at S = 7, which
has no position 10), sits only at the last position in row 1 and starts at position 1 in row 2."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOCAB, BOS, EOS, LAYERS, BATCH = 600, 598, 599, 3, 3
GEOMETRIES = [(128, 2), (96, 3), (64, 2)]          # (hidden, heads): head_dim 64, 64, 32
LENGTHS = [7, 33, 77]                              # shorter than one MFMA tile, one past a 32 boundary, the real length


def _ops():
    from muse import ops
    return ops


@functools.lru_cache(maxsize=None)
def tower(hidden, heads, act="quick_gelu", eos_token_id=EOS, seed=3):
    """-> (transformers CLIPTextModelWithProjection on the CPU in f32, its f64 copy), shared and never modified"""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    torch.manual_seed(seed)
    cfg = CLIPTextConfig(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=4 * hidden, num_hidden_layers=LAYERS,
                         num_attention_heads=heads, max_position_embeddings=77, projection_dim=48, hidden_act=act, bos_token_id=BOS,
                         eos_token_id=eos_token_id, pad_token_id=EOS)
    m = CLIPTextModelWithProjection(cfg).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 2 and "embedding" not in name:
                p.mul_(4.0)
            elif name.endswith(".bias"):
                p.normal_(0.0, 0.1)
    import copy
    return m, copy.deepcopy(m).double()


def fill_start(S):
    return 10 if S > 10 else 4


def make_ids(S, seed=0):
    g = torch.Generator().manual_seed(100 + S + seed)
    ids = torch.randint(3, BOS, (BATCH, S), generator=g)
    ids[:, 0] = BOS
    ids[0, fill_start(S):] = EOS
    ids[1, S - 1] = EOS
    ids[2, 1:] = EOS
    return ids


def outputs_of(o):
    """name -> tensor for every tensor the issue compares"""
    out = {f"hidden_states[{i}]": h for i, h in enumerate(o.hidden_states)}
    out.update(last_hidden_state=o.last_hidden_state, text_embeds=o.text_embeds)
    return out


@functools.lru_cache(maxsize=None)
def oracle(hidden, heads, act, eos_token_id, S):
    """the oracle's f32, f64 and bf16-autocast runs on the ids of make_ids(S), computed once"""
    m32, m64 = tower(hidden, heads, act, eos_token_id)
    ids = make_ids(S)
    with torch.no_grad():
        o32 = m32(ids, return_dict=True, output_hidden_states=True)
        o64 = m64(ids, return_dict=True, output_hidden_states=True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            o16 = m32(ids, return_dict=True, output_hidden_states=True)
        pooled = m32.text_model(ids).pooler_output
    return outputs_of(o32), outputs_of(o64), outputs_of(o16), pooled


def native(hidden, heads, act, eos_token_id, dtype):
    import muse
    enc = muse.CLIPTextEncoder.from_transformers(tower(hidden, heads, act, eos_token_id)[0])
    return enc.to(DEV, dtype=dtype)


def gap(a, b):
    """max abs error over max |x|"""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


VARIANTS = [("quick_gelu", EOS), ("quick_gelu", 2), ("gelu", EOS), ("gelu", 2)]       # both activations, both pooling rules


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("hidden,heads", GEOMETRIES)
def test_f32_mode_against_the_oracle(hidden, heads, S):
    """exact-f32 mode vs transformers on the CPU in f32, every hidden state + last_hidden_state + pooler_output + text_embeds.  Bar per
    tensor: 4 x the oracle's own float32-vs-float64 gap on the same inputs (max abs error over max |x|), measured here; the factor covers
    the different summation order of the MFMA f32 chains.  Pooled positions agree exactly.
    Measured on MI355X (hidden 128, S 77, quick_gelu, per tensor): oracle f32-vs-f64 gap 0.95e-6 .. 1.22e-6 of max |x| (3.0e-8 for the
    embeddings, which come out bit-equal), achieved error 1.04e-6 .. 1.26e-6, i.e. 0.9 .. 1.2 x the gap; the worst ratio over every
    case and tensor was 1.82 x (hidden 96, S 33, gelu, text_embeds: gap 9.2e-7, achieved 1.68e-6)."""
    ops = _ops()
    for act, eos in VARIANTS:
        o32, o64, _, pooled32 = oracle(hidden, heads, act, eos, S)
        enc = native(hidden, heads, act, eos, torch.float32)
        ids = make_ids(S).to(DEV)
        out = enc(ids, return_dict=True, output_hidden_states=True)
        assert len(out.hidden_states) == LAYERS + 1
        idx, flat = ops.eos_index(ids, eos)
        assert idx.tolist() == [fill_start(S), S - 1, 1] and flat.tolist() == [b * S + p for b, p in enumerate(idx.tolist())]
        got = dict(outputs_of(out), pooler_output=out.pooler_output)
        o32p = dict(o32, pooler_output=pooled32)
        o64p = dict(o64, pooler_output=o64["last_hidden_state"][torch.arange(BATCH), idx.cpu()])
        for name, want in o32p.items():
            assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
            bar, err = 4.0 * gap(want, o64p[name]), gap(got[name], want)
            print(f"f32 {hidden}/{heads} S={S} {act} eos={eos} {name}: oracle f32-f64 gap {bar / 4:.3e} achieved {err:.3e}")
            assert err <= bar, (name, act, eos, err, bar)
        assert torch.equal(out[0], out.text_embeds) and torch.equal(out[1], out.last_hidden_state)


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("hidden,heads", GEOMETRIES)
def test_bf16_mode_against_the_oracle(hidden, heads, S):
    """bf16 mode vs the oracle's f32 run: every hidden state + last_hidden_state + pooler_output + text_embeds.  Bar per tensor: 2 x the oracle's own torch.autocast("cpu", bfloat16) gap from its f32 run on
    the same inputs, computed here (two bf16-operand, f32-accumulate pipelines with different rounding points).  The fused causal
    kernel runs once per layer and no score matrix is materialised.
    Measured on MI355X (hidden 128, S 77, quick_gelu, per tensor): autocast gap 0.95e-2 .. 1.30e-2 of max |x| (0 for the embeddings:
    bit-equal), achieved 0.99e-2 .. 1.19e-2, i.e. 0.9 .. 1.15 x the gap; the worst ratio over every case and tensor was 1.51 x
    (hidden 96, S 33, quick_gelu, text_embeds: gap 1.04e-2, achieved 1.57e-2)."""
    ops = _ops()
    for act, eos in VARIANTS:
        o32, _, o16, pooled32 = oracle(hidden, heads, act, eos, S)
        enc = native(hidden, heads, act, eos, torch.bfloat16)
        ids = make_ids(S).to(DEV)
        enc(ids)                                   # packs the operands outside the profiled run
        ops.profile_start()
        out = enc(ids, return_dict=True, output_hidden_states=True)
        names = [r[0] for r in ops.profile_stop(with_kind=True)]
        assert names.count("attn_causal_fwd_bf16") == LAYERS, names
        assert "causal_softmax_fwd" not in names and not any(n.startswith("gemm_f32") for n in names), names
        assert sum(n.startswith("gemm_bf16") for n in names) == 4 * LAYERS + 1, names       # qkv, out, fc1, fc2 per layer + the projection
        at = (torch.arange(BATCH), torch.tensor([fill_start(S), S - 1, 1]))          # pooler_output = last_hidden_state at the pooled positions
        got_all = dict(outputs_of(out), pooler_output=out.pooler_output)
        o32p, o16p = dict(o32, pooler_output=pooled32), dict(o16, pooler_output=o16["last_hidden_state"][at])
        for name, want in o32p.items():
            got = got_all[name]
            assert got.dtype == torch.float32 and got.shape == want.shape, name
            bar, err = 2.0 * gap(o16p[name], want), gap(got, want)
            print(f"bf16 {hidden}/{heads} S={S} {act} eos={eos} {name}: autocast gap {bar / 2:.3e} achieved {err:.3e}")
            assert err <= bar, (name, act, eos, err, bar)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("hidden,heads", GEOMETRIES)
def test_causality_bit_for_bit(hidden, heads, S, dtype):
    """changing the ids at positions >= p leaves every hidden state at positions < p bit-identical, for p in {1, 16, 32, 33, S - 1};
    permuting the batch permutes the outputs bit for bit; no output lane is NaN / inf"""
    enc = native(hidden, heads, "quick_gelu", EOS, dtype)
    ids = make_ids(S).to(DEV)

    def run(i):
        o = enc(i, return_dict=True, output_hidden_states=True)
        return list(o.hidden_states) + [o.last_hidden_state], o

    base, o = run(ids)
    for t in base + [o.text_embeds, o.pooler_output]:
        assert bool(torch.isfinite(t).all())
    for p in sorted({1, 16, 32, 33, S - 1}):
        if not 1 <= p < S:
            continue
        other = ids.clone()
        other[:, p:] = (other[:, p:] + 7) % (BOS - 3) + 3
        changed, _ = run(other)
        for a, b in zip(base, changed):
            assert torch.equal(a[:, :p], b[:, :p]), (p, float((a[:, :p] - b[:, :p]).abs().max()))
        assert not torch.equal(base[-1][:, p:], changed[-1][:, p:])         # ... and the change does show behind p
    perm = torch.tensor([2, 0, 1], device=DEV)
    permuted, op = run(ids[perm].contiguous())
    for a, b in zip(base, permuted):
        assert torch.equal(a[perm], b)
    assert torch.equal(o.text_embeds[perm], op.text_embeds) and torch.equal(o.pooler_output[perm], op.pooler_output)


@pytest.mark.parametrize("S", [1, 7, 16, 33, 77, 128])
@pytest.mark.parametrize("heads,hd", [(3, 64), (3, 32)])
def test_fused_causal_attention_kernel(heads, hd, S):
    """the fused causal kernel vs a float64 masked softmax on the same bf16 inputs: q / k / v are slices of ONE packed [B*S, 3H] tensor
    whose last row is the last row of its storage, B * heads = 9 is odd.  Tolerance: rel_err < 1.5e-2, the bar
    test_gpu_kernels.py::test_fused_attention_fwd_bwd sets for the bf16 fused forward at head_dim 64 and 32 (bf16 P and bf16 output).
    A second run over image 0 alone, with the rows behind its last token NaN, must give the same bits.  That shows a V row >= S that
    reached the second product (0 * NaN) and nothing else: a K row >= S would be overwritten by the mask, a Q row >= S is never stored,
    and the caching allocator rounds a block up, so a read behind the tensor's last row need not fault.  That K, V and Q rows >= S
    are not READ rests on the predicates `row < S` / `qr < S` in front of the three loads of enc::attn_kernel (csrc/attention_enc.hip), checked by reading.
    Measured on MI355X: rel_err 1.5e-3 .. 3.0e-3 (0 at S = 1)."""
    ops = _ops()
    B, H = 3, heads * hd
    alpha = float(hd) ** -0.5
    rng = np.random.default_rng(40 + S + hd)
    qkv = torch.from_numpy(rng.standard_normal((B * S, 3 * H)).astype(np.float32) * 1.5).to(torch.bfloat16)
    x = qkv.double().view(B, S, 3, heads, hd)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    sc = q @ k.transpose(-1, -2) * alpha
    sc = sc.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B * S, H)
    g = qkv.to(DEV)
    ctx = ops.causal_attention_fwd(g[:, :H], g[:, H:2 * H], g[:, 2 * H:], B, S, heads, hd, alpha)
    assert ctx.dtype == torch.bfloat16 and bool(torch.isfinite(ctx.float()).all())
    err = float((ctx.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"causal attention hd={hd} S={S}: rel_err {err:.3e}")
    assert err < 1.5e-2
    # image 0 alone, the rows behind it NaN: the same bits (a V row >= S in the second product would show)
    poisoned = g.clone()
    poisoned[S:] = float("nan")
    one = ops.causal_attention_fwd(poisoned[:, :H], poisoned[:, H:2 * H], poisoned[:, 2 * H:], 1, S, heads, hd, alpha)
    assert torch.equal(one[:S], ctx[:S])
    with pytest.raises(Exception, match="code -3"):
        ops.causal_attention_fwd(g[:, :48], g[:, 48:96], g[:, 96:144], B, S, 1, 48, alpha)


def test_fused_causal_attention_refuses_long_sequences():
    ops = _ops()
    g = torch.zeros((129, 192), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(Exception, match="code -3"):
        ops.causal_attention_fwd(g[:, :64], g[:, 64:128], g[:, 128:], 1, 129, 1, 64, 0.125)


def ulp_of(t):
    """spacing of float32 at every entry of t (t normal, non-zero)"""
    return torch.ldexp(torch.ones_like(t), torch.frexp(t)[1] - 24)


def kernel_order_softmax(x, keep):
    """torch, f32, in causal_softmax_kernel's own order: m = the row maximum, e = exp(x - m), lane l adds columns l and l + 64, six
    xor-butterfly steps (32 .. 1) add the 64 lanes, y = e * (1 / sum).  exp on the device (the device library's, as the kernel's), the
    IEEE operations on the CPU.  -> (y [mats, S, ld], x - m)"""
    ld = x.shape[-1]
    d = torch.where(keep, x - x.masked_fill(~keep, float("-inf")).amax(-1, keepdim=True), torch.zeros(()))
    e = torch.where(keep, torch.exp(d.to(DEV)).cpu(), torch.zeros(()))
    e128 = torch.nn.functional.pad(e, (0, 128 - ld))
    v = e128[..., :64] + e128[..., 64:]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    inv = torch.ones_like(v) / v
    return (e128 * torch.cat([inv, inv], -1))[..., :ld], d


@pytest.mark.parametrize("S", [1, 7, 33, 77, 128])
def test_causal_softmax_kernel(S):
    """row i of each [S, ld] matrix = softmax over columns 0..i; masked and pad columns exactly 0.  Every kept entry is bounded in units
    of THAT entry (the scores span +-16, so the probabilities of a row span many orders of magnitude):
    (a) at most 1 ulp of the entry from torch.softmax of the masked row on the same device, which adds the row in another order;
    (b) at most 1 ulp of the entry from the same f32 expression evaluated with torch in the kernel's summation order
        (kernel_order_softmax), where the order cannot excuse anything;
    (c) at most 6.5 eps (eps = 2^-23) relative from the float64 softmax of the same f32 differences x - m: eps for expf (1 ulp, the
        device library's documented accuracy) + 4.5 eps for the sum (eps from its terms, 7 roundings of eps / 2 on the way: 1 in the
        lane, 6 in the butterfly; all terms positive) + eps / 2 each for 1 / sum and the product.  An ulp is between eps / 2 and eps
        of the entry, so this is <= 13 ulp in the worst case; the bound is independent of any f32 order.
    Measured on MI355X over S = 1 .. 128: (a) 1.00 ulp (0 at S = 1), (b) 0 - the same bits, (c) 1.34 .. 2.82 eps (0 at S = 1)."""
    ops = _ops()
    ld, mats = (S + 3) & ~3, 5
    x = torch.randn((mats, S, ld), generator=torch.Generator().manual_seed(S)) * 4
    keep = torch.tril(torch.ones(S, ld, dtype=torch.bool))
    got = ops.causal_softmax_(x.to(DEV), mats, S, ld).cpu()
    assert bool((got[:, ~keep] == 0).all())
    assert bool((got[:, keep] > 0).all())
    want, d = kernel_order_softmax(x, keep)
    e64 = torch.where(keep, torch.exp(d.double()), torch.zeros((), dtype=torch.float64))
    want64 = e64 / e64.sum(-1, keepdim=True)
    lib = torch.softmax(x.to(DEV).masked_fill(~keep.to(DEV), float("-inf")), -1).cpu()
    k = keep.expand_as(got)
    in_ulp = ((got - want).abs() / ulp_of(want))[k].max()
    rel64 = ((got.double() - want64).abs() / want64)[k].max() / torch.finfo(torch.float32).eps
    lib_ulp = ((got - lib).abs() / ulp_of(lib))[k].max()
    print(f"causal softmax S={S}: {float(lib_ulp):.2f} ulp from torch.softmax, {float(in_ulp):.2f} ulp from the kernel-order torch "
          f"expression, {float(rel64):.2f} eps from f64")
    assert float(lib_ulp) <= 1.0
    assert float(in_ulp) <= 1.0
    assert float(rel64) <= 6.5
    assert bool(((got.sum(-1) - 1).abs() < 1e-5).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_quick_gelu_kernel(dtype):
    """y = v sigmoid(1.702 v), v = x + b[col], in place, against torch's own f32 expression on the device: at most 1 ulp of the
    storage type apart (f32: the same operations in the same order; bf16: torch's f32 result rounded once)"""
    ops = _ops()
    rows, cols = 37, 200                             # several blocks, no multiple of the block
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((rows, cols), generator=g) * 3).to(dtype).to(DEV)
    b = (torch.randn(cols, generator=g) * 0.5).to(DEV)
    v = x.float() + b
    want = (v * torch.sigmoid(1.702 * v)).to(dtype)
    got = ops.bias_quick_gelu_(x.clone(), b)
    assert got.dtype == dtype
    mant = 23 if dtype == torch.float32 else 7
    one_ulp = torch.exp2(torch.floor(torch.log2(want.float().abs().clamp_min(1e-30))) - mant)
    assert bool(((got.float() - want.float()).abs() <= one_ulp).all()), float(((got.float() - want.float()).abs() / one_ulp).max())


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_layernorm_with_bias_kernel(out_dtype):
    """LayerNorm(x) w + b in one pass vs F.layer_norm in f64: 2e-6 of max |y| in f32 (a few ulp: mean, variance and the affine map in
    f32), one bf16 rounding (2^-8 relative) + that in bf16"""
    ops = _ops()
    rows, cols = 23, 96
    g = torch.Generator().manual_seed(6)
    x = torch.randn((rows, cols), generator=g) * 5 + 2
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (cols,), w.double(), b.double(), 1e-5)
    got = ops.layernorm_bias_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, out_dtype).double().cpu()
    tol = 2e-6 * float(want.abs().max())
    if out_dtype == torch.bfloat16:
        assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + tol).all())
    else:
        assert float((got - want).abs().max()) <= tol


def test_eos_index_kernel():
    """exact against torch's argmax forms (transformers CLIPTextTransformer.forward): rows without an EOS, rows with repeated maxima, a
    row longer than a wave, both rules"""
    ops = _ops()
    for S in (5, 77, 130):
        g = torch.Generator().manual_seed(S)
        ids = torch.randint(3, 500, (9, S), generator=g)
        ids[0, S // 2:] = EOS                        # repeated EOS = repeated maximum
        ids[1, S - 1] = EOS
        ids[2, 0] = EOS
        ids[3, :] = 7                                # no EOS, every position the maximum
        ids[4, 2] = ids[4, 4] = 550                  # no EOS, the maximum twice
        ids[5, 1:] = EOS
        for eos in (EOS, 2):
            want = ids.argmax(-1) if eos == 2 else (ids == eos).int().argmax(-1)
            idx, flat = ops.eos_index(ids.to(DEV), eos)
            assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), want), (S, eos, idx.tolist(), want.tolist())
            assert torch.equal(flat.cpu(), want + torch.arange(9) * S)


def test_pipeline_with_the_native_text_encoder(golden_dir, tmp_path):
    """PipelineMuse.from_pretrained(dir, native_text_encoder=True) loads the text tower as muse.CLIPTextEncoder; pipe(prompts) equals
    pipe(prompt_embeds=...) on the states computed by calling that encoder directly (the pattern of
    test_gpu_sampling.py::test_pipeline_from_pretrained_text_to_image_with_a_real_clip_tower).  The tower has hidden 64 / 2 heads
    (head_dim 32; the golden U-ViT expects 24 text features), so the U-ViT takes the golden weights except a seeded [32, 64] encoder_proj."""
    import muse
    import weights as W
    gp = np.load(os.path.join(golden_dir, "uvit_tiny.npz"))
    cfg = dict(json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json"))), encoder_hidden_size=64)
    u = muse.MaskGiTUViT(**cfg)
    sd = {k[len("param."):]: torch.from_numpy(gp[k]) for k in gp.files if k.startswith("param.")}
    sd["encoder_proj.weight"] = torch.randn((32, 64), generator=torch.Generator().manual_seed(9)) * 0.2
    u.load_state_dict(sd, strict=True)
    enc, tok = W.tiny_clip(str(tmp_path / "clip_src"), hidden=64, pooled=cfg["cond_embed_dim"])
    muse.PipelineMuse(vae=muse.MaskGitVQGAN(**W.VQGAN_TINY), transformer=u, text_encoder=enc, tokenizer=tok).save_pretrained(str(tmp_path / "ckpt"))
    pipe = muse.PipelineMuse.from_pretrained(str(tmp_path / "ckpt"), native_text_encoder=True).to(DEV, dtype=torch.float32)
    assert isinstance(pipe.text_encoder, muse.CLIPTextEncoder) and next(pipe.text_encoder.parameters()).is_cuda
    assert pipe.text_encoder.compute_dtype == torch.float32
    prompts = ["a red fox", "two cats on a sofa"]
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)   # noqa: E731
    kw = dict(timesteps=3, guidance_scale=1.5, output_type="np", transformer_seq_len=16)
    imgs = pipe(prompts, generator=gen(), **kw)
    assert imgs.shape == (2, 16, 16, 3) and np.isfinite(imgs).all()

    def states(texts):
        ids = pipe.tokenizer(texts, return_tensors="pt", padding="max_length", truncation=True, max_length=pipe.tokenizer.model_max_length).input_ids
        o = pipe.text_encoder(ids.to(DEV), return_dict=True, output_hidden_states=True)
        return o.hidden_states[-2].float(), o.text_embeds.float()
    (h, pooled), (nh, npooled) = states(prompts), states(["", ""])
    want = pipe(prompt_embeds=h, pooled_embeds=pooled, negative_prompt_embeds=nh, negative_pooled_embeds=npooled, generator=gen(), **kw)
    assert np.array_equal(imgs, want)
    assert not np.array_equal(imgs, pipe(["a blue whale", "two cats on a sofa"], generator=gen(), **kw))       # the prompt matters
