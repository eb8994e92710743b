"""GPU (MI355X): muse.T5TextEncoder and the kernels of csrc/t5_text.hip and csrc/attention_enc.hip against transformers' own T5EncoderModel on the CPU.

The tiny encoders come from tests/t5_tiny.py (T5Config under a fixed seed, made to behave like trained ones: the bias table ~ N(0, 2),
the other non-embedding 2-D weights x 2, norm weights 1 + 0.2 N(0, 1)): 3 layers, 2 heads of d_kv 64, d_ff 320, vocab 600, batch 3, with
d_model 128 (= heads x d_kv) and 96 (!= heads x d_kv)."""
import functools

import numpy as np
import pytest
import torch

import t5_tiny
from t5_tiny import GEOMETRIES, LAYERS, make_ids, tower

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = [7, 33, 128, 160]         # shorter than one MFMA tile, one past a 32 boundary, the fused kernel's longest, the materialised route
EPS = float(torch.finfo(torch.float32).eps)


def _ops():
    from muse import ops
    return ops


def outputs_of(o):
    """name -> tensor for every tensor the tests compare"""
    out = {f"hidden_states[{i}]": h for i, h in enumerate(o.hidden_states)}
    out.update(last_hidden_state=o.last_hidden_state)
    return out


@functools.lru_cache(maxsize=None)
def oracle(d_model, S):
    """the oracle's f32, f64 and bf16-autocast runs on the ids of make_ids(S), computed once"""
    m32, m64 = tower(d_model)
    ids = make_ids(S)
    with torch.no_grad():
        o32 = m32(ids, return_dict=True, output_hidden_states=True)
        o64 = m64(ids, return_dict=True, output_hidden_states=True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            o16 = m32(ids, return_dict=True, output_hidden_states=True)
    return outputs_of(o32), outputs_of(o64), outputs_of(o16)


def native(d_model, dtype):
    import muse
    return muse.T5TextEncoder.from_transformers(tower(d_model)[0]).to(DEV, dtype=dtype)


def gap(a, b):
    """max abs error over max |x|"""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("d_model", GEOMETRIES)
def test_f32_mode_against_the_oracle(d_model, S):
    """exact-f32 mode vs transformers on the CPU in f32, every hidden state + last_hidden_state.  Bar per tensor: 4 x the oracle's own
    float32-vs-float64 gap on the same inputs (max abs error over max |x|), measured here - the factor tests/test_gpu_clip_text.py uses
    for the same pair of pipelines; it covers the different summation order of the MFMA f32 chains.  hidden_states has num_layers + 1
    entries, the last one the final-normed state (= last_hidden_state), as in transformers; the embeddings come out bit-equal.
    Measured on MI355X: worst achieved / gap over every case and tensor 1.64 (d_model 128, S 7); per case in MEASURED at the end of this file."""
    o32, o64, _ = oracle(d_model, S)
    enc = native(d_model, torch.float32)
    out = enc(make_ids(S).to(DEV), return_dict=True, output_hidden_states=True)
    assert len(out.hidden_states) == LAYERS + 1 and torch.equal(out.hidden_states[-1], out.last_hidden_state)
    assert out[0] is out.last_hidden_state and out[1] is out.hidden_states
    got = outputs_of(out)
    worst = 0.0
    for name, want in o32.items():
        assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
        bar, err = 4.0 * gap(want, o64[name]), gap(got[name], want)
        print(f"f32 d_model={d_model} S={S} {name}: oracle f32-f64 gap {bar / 4:.3e} achieved {err:.3e}")
        worst = max(worst, err / (bar / 4)) if bar else worst
        assert err <= bar, (name, err, bar)
    print(f"f32 d_model={d_model} S={S}: worst ratio achieved / gap {worst:.2f}")
    only_last = enc(make_ids(S).to(DEV))
    assert only_last.hidden_states is None and torch.equal(only_last.last_hidden_state, out.last_hidden_state)
    assert torch.equal(enc(make_ids(S).to(DEV), return_dict=False)[0], out.last_hidden_state)


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("d_model", GEOMETRIES)
def test_bf16_mode_against_the_oracle(d_model, S):
    """bf16 mode vs the oracle's f32 run, every hidden state + last_hidden_state.  Bar per tensor: 2 x the oracle's own
    torch.autocast("cpu", bfloat16) gap from its f32 run on the same inputs, computed here (two bf16-operand, f32-accumulate pipelines
    with different rounding points).  S <= 128: the fused bias attention kernel runs once per layer, no score matrix is materialised,
    no f32 product runs and a layer is exactly 4 bf16 products (qkv, o, wi, wo).  S = 160: the bias + softmax kernel runs once per layer
    between two batched products, the fused kernel not at all.
    Measured on MI355X: worst achieved / gap over every case and tensor 1.17 (d_model 96, S 33); per case in MEASURED at the end of this file."""
    ops = _ops()
    o32, _, o16 = oracle(d_model, S)
    enc = native(d_model, torch.bfloat16)
    ids = make_ids(S).to(DEV)
    enc(ids)                                   # packs the operands and builds the bias outside the profiled run
    ops.profile_start()
    out = enc(ids, return_dict=True, output_hidden_states=True)
    names = [r[0] for r in ops.profile_stop(with_kind=True)]
    assert not any(n.startswith("gemm_f32") for n in names), names
    if S <= 128:
        assert names.count("attn_bias_fwd_bf16") == LAYERS, names
        assert "bias_softmax_fwd" not in names, names
        assert sum(n.startswith("gemm_bf16") for n in names) == 4 * LAYERS, names
    else:
        assert names.count("bias_softmax_fwd") == LAYERS and "attn_bias_fwd_bf16" not in names, names
        assert sum(n.startswith("gemm_bf16") for n in names) == 6 * LAYERS, names
    got = outputs_of(out)
    worst = 0.0
    for name, want in o32.items():
        assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
        bar, err = 2.0 * gap(o16[name], want), gap(got[name], want)
        print(f"bf16 d_model={d_model} S={S} {name}: autocast gap {bar / 2:.3e} achieved {err:.3e}")
        worst = max(worst, err / (bar / 2)) if bar else worst
        assert err <= bar, (name, err, bar)
    print(f"bf16 d_model={d_model} S={S}: worst ratio achieved / gap {worst:.2f}")


def bias_matrix(rel, S):
    """rel [heads, 2 S - 1] -> [heads, S, S]: entry (i, j) = rel[h][j - i + S - 1]"""
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return rel[:, j - i + S - 1]


@pytest.mark.parametrize("S", [1, 7, 16, 17, 32, 33, 77, 128])
@pytest.mark.parametrize("heads,hd", [(3, 64), (3, 32)])
def test_fused_bias_attention_kernel(heads, hd, S):
    """the fused kernel vs a float64 softmax(q k^T + bias) v on the same bf16 inputs, at every dispatch edge (the wave count changes at
    multiples of 16, the V^T image's width at multiples of 32): q / k / v are slices of ONE packed [B*S, 3 inner] tensor whose last row
    is the last row of its storage, B * heads = 9 is odd, rel ~ N(0, 2).  No score scale.  Tolerance: rel_err < 1.5e-2, the bar the
    project sets for its bf16 fused forwards (bf16 P and bf16 output).  A second run over image 0 alone, with the rows behind its last
    token NaN, must give the same bits: a V row >= S that reached the second product (0 * NaN) would show.  That K, V and Q rows >= S
    are not READ rests on the predicates `row < S` / `qr < S` in front of the three loads of enc::attn_kernel (csrc/attention_enc.hip), checked by reading.
    Measured on MI355X: rel_err 2.0e-3 .. 3.7e-3 (0 at S = 1); per case in MEASURED at the end of this file."""
    ops = _ops()
    B, H = 3, heads * hd
    rng = np.random.default_rng(40 + S + hd)
    qkv = torch.from_numpy(rng.standard_normal((B * S, 3 * H)).astype(np.float32) * 0.6).to(torch.bfloat16)
    rel = torch.from_numpy(rng.standard_normal((heads, 2 * S - 1)).astype(np.float32) * 2.0)
    x = qkv.double().view(B, S, 3, heads, hd)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    sc = q @ k.transpose(-1, -2) + bias_matrix(rel.double(), S)
    ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B * S, H)
    g, r = qkv.to(DEV), rel.to(DEV)
    ctx = ops.bias_attention_fwd(g[:, :H], g[:, H:2 * H], g[:, 2 * H:], r, B, S, heads, hd)
    assert ctx.dtype == torch.bfloat16 and bool(torch.isfinite(ctx.float()).all())
    err = float((ctx.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"bias attention hd={hd} S={S}: rel_err {err:.3e}")
    assert err < 1.5e-2
    # image 0 alone, the rows behind it NaN: the same bits
    poisoned = g.clone()
    poisoned[S:] = float("nan")
    one = ops.bias_attention_fwd(poisoned[:, :H], poisoned[:, H:2 * H], poisoned[:, 2 * H:], r, 1, S, heads, hd)
    assert torch.equal(one[:S], ctx[:S])


def test_fused_bias_attention_refusals():
    """S = 129 and head_dim 48 return MUSE_ERR_UNSUPPORTED (-3)"""
    ops = _ops()
    g = torch.zeros((129, 192), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(Exception, match="code -3"):
        ops.bias_attention_fwd(g[:, :64], g[:, 64:128], g[:, 128:], torch.zeros((1, 257), device=DEV), 1, 129, 1, 64)
    g = torch.zeros((16, 144), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(Exception, match="code -3"):
        ops.bias_attention_fwd(g[:, :48], g[:, 48:96], g[:, 96:144], torch.zeros((1, 31), device=DEV), 1, 16, 1, 48)


@pytest.mark.parametrize("S", [17, 33, 128])
def test_exact_bias_probe(S):
    """q = 0, so the scores are the bias alone.  For every bucket b of the (32, 128) map, head h probes bucket (b + h) mod 32: rel[h] is
    30.0 at the signed distances of that bucket and 0 elsewhere.  v[j][d] = ((7 j + d) mod 13) - 6 (d = the column of the packed v
    slice, so the three heads see different values), exact in bf16.  Expected row i of head h: the plain mean of v[j] over the keys
    j < S whose distance j - i falls in the probed bucket, or over all j < S when there is none.
    Bound, derived: |got - want| <= 2^-8 * 6 - one bf16 rounding of the probabilities and one of the output, 2^-9 each, relative to
    max |v| = 6 (the probed keys' exponentials are exp(0) = 1, exact in bf16; the leakage of the others, S e^-30, is below 1e-10).
    S = 128 reaches every bucket the map can produce: all 32 but bucket 16, which would be a key AFTER the query at distance 0 (probing
    it takes the no-key branch at every length).  A swapped sign, an off-by-one in j - i + S - 1, a head stride error or a key >= S that is not masked
    each move whole rows by O(1)."""
    from muse.modeling_t5_text import rel_buckets
    ops = _ops()
    heads, hd, NB = 3, 64, 32
    H = heads * hd
    bucket = rel_buckets(S, NB, 128)                                 # [2 S - 1]
    if S == 128:
        assert sorted(set(bucket.tolist())) == [b for b in range(NB) if b != 16]
    j, c = torch.arange(S)[:, None], torch.arange(H)[None, :]
    v = ((7 * j + c) % 13 - 6).double()                              # [S, H]
    g = torch.Generator().manual_seed(S)
    qkv = torch.cat([torch.zeros(S, H), torch.randn((S, H), generator=g), v.float()], 1).to(torch.bfloat16).to(DEV)
    assert torch.equal(qkv[:, 2 * H:].double().cpu(), v)
    i_, j_ = torch.arange(S)[:, None], torch.arange(S)[None, :]
    dist_bucket = bucket[j_ - i_ + S - 1]                            # [S, S]: bucket of (query i, key j)
    worst = 0.0
    for b in range(NB):
        probe = [(b + h) % NB for h in range(heads)]
        rel = torch.stack([(bucket == p).float() * 30.0 for p in probe])          # [heads, 2 S - 1]
        got = ops.bias_attention_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], rel.to(DEV), 1, S, heads, hd).double().cpu()
        for h, p in enumerate(probe):
            hit = (dist_bucket == p).double()
            hit[hit.sum(-1) == 0] = 1.0                                          # no key in the bucket: every key
            want = hit @ v[:, h * hd:(h + 1) * hd] / hit.sum(-1, keepdim=True)
            err = float((got[:, h * hd:(h + 1) * hd] - want).abs().max())
            worst = max(worst, err)
            assert err <= 2.0 ** -8 * 6, (b, h, p, err)
    print(f"exact bias probe S={S}: worst |got - want| {worst:.3e} (bound {2.0 ** -8 * 6:.3e})")


@pytest.mark.parametrize("S", [1, 7, 33, 128, 129, 512])
def test_bias_softmax_kernel(S):
    """row i of matrix z = softmax_j(x[i][j] + rel[z % heads][j - i + S - 1]) over j < S, ld = (S + 3) & ~3; pad columns exactly 0, row
    sums within 1e-5 of 1.  Two bounds per entry, in units of THAT entry (the exponents span +-25, so the probabilities of a row span
    many orders of magnitude), eps = 2^-23:
    (a) <= 6.5 eps relative from the float64 softmax of the kernel's own f32 exponents d = (x + bias) - m (both f32 operations are
        IEEE and reproduced here with torch): the accounting of test_gpu_clip_text.py::test_causal_softmax_kernel - eps for expf, 4.5
        eps for the sum, eps / 2 each for 1 / sum and the product.  (At S = 129 and 512 a lane adds up to 3 and 8 terms instead of 2,
        which that worst-case count would price at 5 and 7.5 eps for the sum; the bar stays 6.5 eps at every length);
    (b) against torch.softmax(x + bias) in float64 on the EXACT sums: the two f32 roundings in front of the exponential (the bias add
        and the subtraction of the maximum) are absolute errors of the exponent, eps / 2 of |x + bias| and of |x + bias - m|, i.e.
        RELATIVE errors of that size in the exponential - not half an eps of the entry when the exponent is far from 0.  So the bound
        is 6.5 eps + delta_j + sum_k p_k delta_k with delta = eps / 2 (|x + bias| + |x + bias - m|): the entry's own exponent and the
        probability-weighted ones of the row's sum.
    The bf16 copy is the f32 result rounded once, and leaves x as it was.
    Measured on MI355X: (a) 1.77 .. 3.42 eps (0 at S = 1), (b) at most 0.75 of its bound; per case in MEASURED at the end of this file."""
    ops = _ops()
    ld, mats, heads = (S + 3) & ~3, 5, 3
    g = torch.Generator().manual_seed(S)
    x = torch.randn((mats, S, ld), generator=g) * 4
    rel = torch.randn((heads, 2 * S - 1), generator=g) * 2
    bias = bias_matrix(rel, S)[torch.arange(mats) % heads]                           # [mats, S, S]
    got = ops.bias_softmax_(x.to(DEV), rel.to(DEV), mats, heads, S, ld).cpu()
    assert bool((got[..., S:] == 0).all()) and bool((got[..., :S] > 0).all())
    assert bool(((got.sum(-1) - 1).abs() < 1e-5).all())
    t = x[..., :S] + bias                                                            # f32, as the kernel adds
    m = t.amax(-1, keepdim=True)
    d = t - m                                                                        # f32, as the kernel subtracts
    e64 = torch.exp(d.double())
    want_a = e64 / e64.sum(-1, keepdim=True)
    rel_a = float(((got[..., :S].double() - want_a).abs() / want_a).max()) / EPS
    exact = x[..., :S].double() + bias.double()
    want_b = torch.softmax(exact, -1)
    delta = 0.5 * EPS * (t.double().abs() + d.double().abs())
    bound_b = 6.5 * EPS + delta + (want_b * delta).sum(-1, keepdim=True)
    err_b = (got[..., :S].double() - want_b).abs() / want_b
    print(f"bias softmax S={S}: {rel_a:.2f} eps from f64 on the f32 exponents, {float(err_b.max()) / EPS:.2f} eps from f64 on the exact sums "
          f"(worst fraction of its bound {float((err_b / bound_b).max()):.2f})")
    assert rel_a <= 6.5
    assert bool((err_b <= bound_b).all())
    xg = x.to(DEV)
    yb = ops.bias_softmax_(xg, rel.to(DEV), mats, heads, S, ld, bf16_copy=True)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb.cpu(), got.to(torch.bfloat16)) and torch.equal(xg.cpu(), x)


def ulps(got, want, mant):
    """|got - want| in units of the spacing of a `mant`-bit-mantissa format at want"""
    one = torch.exp2(torch.floor(torch.log2(want.float().abs().clamp_min(1e-30))) - mant)
    return float(((got.float() - want.float()).abs() / one).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gated_tanh_gelu_kernel(dtype):
    """y = gelu_new(a) * b for the packed [rows, 2 F] product, against torch's own f32 expression on the device,
    F.gelu(a, approximate="tanh") * b (bf16: on the values as f32, rounded once, as the kernel does).  The bar started at 2 ulp of the
    storage type (tanhf on the device and in torch might differ by 1 ulp); measured on MI355X it is 0 ulp in both types - the same
    operations in the same order on the same device library - so the bar is that: the same bits.  37 x 200: several blocks, no
    multiple of the block."""
    ops = _ops()
    rows, F = 37, 200
    g = torch.Generator().manual_seed(5)
    ab = (torch.randn((rows, 2 * F), generator=g) * 3).to(dtype).to(DEV)
    a, b = ab[:, :F].float(), ab[:, F:].float()
    want = (torch.nn.functional.gelu(a, approximate="tanh") * b).to(dtype)
    got = ops.gated_gelu_tanh(ab)
    assert got.dtype == dtype and got.shape == (rows, F)
    u = ulps(got.cpu(), want.cpu(), 23 if dtype == torch.float32 else 7)
    print(f"gated tanh-GELU {dtype}: {u:.2f} ulp from torch")
    assert u == 0.0


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_rmsnorm_kernel(out_dtype):
    """x * rsqrt(mean(x^2) + eps) * w (T5LayerNorm: no mean subtraction, no bias) vs the same formula in f64: 2e-6 of max |y| in f32,
    one bf16 rounding (2^-8 relative) + that in bf16 - the bar of test_gpu_clip_text.py::test_layernorm_with_bias_kernel.  The f32
    result is muse_norm_res_fwd mode 0, the bf16 result the kernel of csrc/t5_text.hip."""
    ops = _ops()
    rows, cols = 23, 96
    g = torch.Generator().manual_seed(6)
    x = torch.randn((rows, cols), generator=g) * 5 + 2
    w = torch.randn(cols, generator=g)
    xd = x.double()
    want = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
    got = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), 1e-6, out_dtype)
    assert got.dtype == out_dtype
    got = got.double().cpu()
    tol = 2e-6 * float(want.abs().max())
    print(f"rmsnorm {out_dtype}: max error {float((got - want).abs().max()) / float(want.abs().max()):.3e} of max |y|")
    if out_dtype == torch.bfloat16:
        assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + tol).all())
    else:
        assert float((got - want).abs().max()) <= tol


def test_rel_bias_is_gathered_per_head_and_distance():
    """rel[h][t] = relative_attention_bias.weight[bucket[t]][h], exact; built once per length and kept with the packed operands"""
    from muse.modeling_t5_text import rel_buckets
    enc = native(128, torch.float32)
    table = tower(128)[0].encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.detach()
    for S in (1, 33, 160):
        rel = enc._rel(S)
        assert rel.shape == (2, 2 * S - 1) and torch.equal(rel.cpu(), table[rel_buckets(S, 32, 128)].t())
        assert enc._rel(S) is rel
    enc.set_compute_dtype(torch.bfloat16)
    assert not enc._packed


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", [33, 160])
def test_batch_permutation_bit_for_bit(S, dtype):
    """permuting the batch permutes every output bit for bit; no output is NaN / inf (both attention routes, both modes)"""
    enc = native(96, dtype)
    ids = make_ids(S).to(DEV)

    def run(i):
        o = enc(i, return_dict=True, output_hidden_states=True)
        return list(o.hidden_states) + [o.last_hidden_state]

    base = run(ids)
    for t in base:
        assert bool(torch.isfinite(t).all())
    perm = torch.tensor([2, 0, 1], device=DEV)
    for a, b in zip(base, run(ids[perm].contiguous())):
        assert torch.equal(a[perm], b)
    assert not torch.equal(base[-1][0], base[-1][1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_longest_sequence_runs_and_one_more_is_refused(dtype):
    """S = 512 (the T5 tokenizer's model_max_length, which PipelineMuse pads to) gives a finite result, S = 513 a ValueError"""
    enc = native(128, dtype)
    out = enc(make_ids(512, batch=2).to(DEV))
    assert out.last_hidden_state.shape == (2, 512, 128) and bool(torch.isfinite(out.last_hidden_state).all())
    with pytest.raises(ValueError, match="513"):
        enc(make_ids(513, batch=1).to(DEV))


def test_pipeline_with_the_native_t5_encoder(tmp_path):
    """PipelineMuse.from_pretrained(dir, native_text_encoder=True) reads `model_type: "t5"` from text_encoder/config.json and loads the
    encoder as muse.T5TextEncoder; pipe(prompts) equals pipe(prompt_embeds=...) on the states computed by calling that encoder directly
    (`last_hidden_state`: the branch the reference takes for an encoder without `text_embeds`, muse/pipeline_muse.py:133,154), and a
    different prompt changes the image.  The tokenizer is a `tokenizers` Unigram model built offline (tests/t5_tiny.py), saved with
    the pipeline and reloaded by AutoTokenizer; the transformer is the text-conditioned MaskGitTransformer taking 64 text features."""
    import muse
    import weights as W
    hf, tok, tcfg = t5_tiny.pipeline_parts()
    m = muse.MaskGitTransformer(**tcfg)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(tcfg), 830, "transformer"))
    muse.PipelineMuse(vae=muse.MaskGitVQGAN(**W.VQGAN_TINY), transformer=m, text_encoder=hf, tokenizer=tok).save_pretrained(str(tmp_path / "ckpt"))
    pipe = muse.PipelineMuse.from_pretrained(str(tmp_path / "ckpt"), native_text_encoder=True).to(DEV, dtype=torch.float32)
    assert isinstance(pipe.text_encoder, muse.T5TextEncoder) and next(pipe.text_encoder.parameters()).is_cuda
    assert pipe.text_encoder.compute_dtype == torch.float32
    prompts = ["a red fox", "two cats on a sofa"]
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)   # noqa: E731
    kw = dict(timesteps=3, guidance_scale=1.5, output_type="np")
    imgs = pipe(prompts, generator=gen(), **kw)
    assert imgs.shape == (2, 16, 16, 3) and np.isfinite(imgs).all()

    def states(texts):
        ids = pipe.tokenizer(texts, return_tensors="pt", padding="max_length", truncation=True, max_length=pipe.tokenizer.model_max_length).input_ids
        return pipe.text_encoder(ids.to(DEV)).last_hidden_state.float()
    h, nh = states(prompts), states(["", ""])
    with torch.no_grad():
        ids = tok(prompts, return_tensors="pt", padding="max_length", truncation=True, max_length=tok.model_max_length).input_ids
        assert gap(h, hf(ids).last_hidden_state) < 1e-4                                  # ... and they are the oracle's states
    want = pipe(prompt_embeds=h, negative_prompt_embeds=nh, generator=gen(), **kw)
    assert np.array_equal(imgs, want)
    assert not np.array_equal(imgs, pipe(["a blue whale", "two cats on a sofa"], generator=gen(), **kw))       # the prompt matters


# MEASURED (MI355X, one run of this file):
MEASURED = """
f32 mode, achieved error / the oracle's own f32-vs-f64 gap, worst tensor per case (bar 4):
    d_model 128: S=7 1.64, S=33 1.49, S=128 1.08, S=160 1.33;  d_model 96: S=7 1.48, S=33 1.45, S=128 1.33, S=160 1.32
    (the embeddings, hidden_states[0], are bit-equal: gap 0, error 0)
bf16 mode, achieved error / the oracle's own bf16-autocast gap, worst tensor per case (bar 2):
    d_model 128: S=7 0.93, S=33 1.00, S=128 1.06, S=160 0.97;  d_model 96: S=7 0.93, S=33 1.17, S=128 0.92, S=160 1.12
fused bias attention, rel_err against float64 (bar 1.5e-2):
    head_dim 64: S=1 0, S=7 2.4e-3, S=16 2.1e-3, S=17 2.3e-3, S=32 2.0e-3, S=33 2.7e-3, S=77 3.7e-3, S=128 3.7e-3
    head_dim 32: S=1 0, S=7 3.4e-3, S=16 2.7e-3, S=17 2.4e-3, S=32 2.3e-3, S=33 2.1e-3, S=77 2.5e-3, S=128 2.4e-3
exact bias probe, worst |got - want| (bound 2.34e-2): S=17 5.2e-3, S=33 6.3e-3, S=128 6.3e-3
bias softmax, (a) eps from f64 on the f32 exponents (bar 6.5) / (b) worst fraction of the derived bound on the exact sums (bar 1):
    S=1 0 / 0, S=7 1.77 / 0.42, S=33 1.99 / 0.63, S=128 2.57 / 0.71, S=129 2.57 / 0.72, S=512 3.42 / 0.75
    ((b) in eps of the entry: 9.9 .. 28.6 - the exponent's own f32 roundings, which is why (b) cannot be a flat 7 eps)
gated tanh-GELU: 0 ulp from torch in f32 and in bf16 (bit-equal; the bar was tightened from 2 ulp to that)
RMSNorm: f32 5.3e-8 of max |y| (bar 2e-6); bf16 within one bf16 rounding + that
"""
