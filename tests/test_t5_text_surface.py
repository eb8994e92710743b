"""muse.T5TextEncoder without a device: construction, the transformers parameter names, loading and saving transformers directories,
copying a live module, the host's relative-position bucket map and every refusal.  (Numerics: tests/test_gpu_t5_text.py.)

`shared.weight` and `encoder.embed_tokens.weight` are one tensor under two names in T5EncoderModel.state_dict(); a checkpoint file
stores it under one of them (safetensors refuses aliases), so loading takes either or both."""
import json
import os

import pytest
import torch

CFG = dict(vocab_size=600, d_model=128, d_kv=64, d_ff=320, num_layers=3, num_heads=2, feed_forward_proj="gated-gelu", dropout_rate=0.0)
EMBED = ("shared.weight", "encoder.embed_tokens.weight")


def _hf(**over):
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(11)
    return T5EncoderModel(T5Config(**{**CFG, **over})).eval()


def _same(own, want):
    return set(own) == set(want) and all(torch.equal(own[k], want[k]) for k in want)


@pytest.mark.parametrize("over", [{}, dict(d_model=96)])        # num_heads * d_kv == d_model and != d_model
def test_state_dict_names_shapes_and_dtypes_are_those_of_transformers(over):
    import muse
    assert "T5TextEncoder" in muse.__all__ and muse.T5TextEncoder is muse.modeling_t5_text.T5TextEncoder
    want = _hf(**over).state_dict()
    enc = muse.T5TextEncoder({**CFG, **over})
    own = enc.state_dict()
    assert set(own) == set(want), set(own) ^ set(want)
    assert all(tuple(own[k].shape) == tuple(want[k].shape) and own[k].dtype == want[k].dtype == torch.float32 for k in want)
    assert set(EMBED) <= set(own) and own[EMBED[0]].data_ptr() == own[EMBED[1]].data_ptr()          # one tensor, two names
    assert [k for k in own if "relative_attention_bias" in k] == ["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    assert not enc.training and not any(p.requires_grad for p in enc.parameters())
    by_kwargs = muse.T5TextEncoder(**{**CFG, **over})
    assert by_kwargs.config.d_ff == 320 and by_kwargs.config.model_type == "t5" and by_kwargs.compute_dtype == torch.float32


def test_a_transformers_directory_loads_bit_equal(tmp_path):
    import muse
    from safetensors.torch import load_file, save_file
    hf = _hf()
    want = hf.state_dict()
    d = str(tmp_path / "safe")
    hf.save_pretrained(d)
    assert _same(muse.T5TextEncoder.from_pretrained(d).state_dict(), want)
    stored = load_file(os.path.join(d, "model.safetensors"))
    assert len([k for k in EMBED if k in stored]) == 1            # what transformers writes: the tied tensor once
    # pytorch_model.bin with both names, and a checkpoint with only one of the two - either one
    cfg_text = open(os.path.join(d, "config.json")).read()
    for tag, drop in (("bin_both", None), ("bin_shared", EMBED[1]), ("bin_embed", EMBED[0])):
        b = str(tmp_path / tag)
        os.makedirs(b)
        open(os.path.join(b, "config.json"), "w").write(cfg_text)
        torch.save({k: v.clone() for k, v in want.items() if k != drop}, os.path.join(b, "pytorch_model.bin"))
        enc = muse.T5TextEncoder.from_pretrained(b)
        assert _same(enc.state_dict(), want), tag
        assert enc.config.d_ff == 320 and enc.compute_dtype == torch.float32
    for drop in EMBED:
        s = str(tmp_path / ("safe_without_" + drop.split(".")[0]))
        os.makedirs(s)
        open(os.path.join(s, "config.json"), "w").write(cfg_text)
        save_file({k: v.clone() for k, v in want.items() if k != drop}, os.path.join(s, "model.safetensors"))
        assert _same(muse.T5TextEncoder.from_pretrained(s).state_dict(), want), drop
    # the subfolder form PipelineMuse uses, and torch_dtype selecting the compute mode (masters stay f32)
    root = str(tmp_path / "ckpt")
    hf.save_pretrained(os.path.join(root, "text_encoder"))
    enc = muse.T5TextEncoder.from_pretrained(root, subfolder="text_encoder", torch_dtype=torch.bfloat16)
    assert _same(enc.state_dict(), want) and enc.compute_dtype == torch.bfloat16
    # two DIFFERENT tensors under the two names cannot both be the embedding
    bad = dict(want)
    bad[EMBED[1]] = want[EMBED[0]] + 1
    with pytest.raises(ValueError, match="one tensor"):
        muse.T5TextEncoder(CFG).load_state_dict(bad)


def test_save_pretrained_writes_what_transformers_loads(tmp_path):
    import muse
    from transformers import T5EncoderModel
    for over in ({}, dict(d_model=96)):
        hf = _hf(**over)
        enc = muse.T5TextEncoder.from_transformers(hf)
        d = str(tmp_path / f"t5_{len(over)}")
        enc.save_pretrained(d)
        back, info = T5EncoderModel.from_pretrained(d, output_loading_info=True)
        assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
        assert _same(back.state_dict(), hf.state_dict())
        assert back.config.feed_forward_proj == "gated-gelu" and back.config.d_kv == 64 and back.config.d_model == hf.config.d_model
        assert _same(muse.T5TextEncoder.from_pretrained(d).state_dict(), hf.state_dict())            # and reads its own directory
        assert json.load(open(os.path.join(d, "config.json")))["dtype"] == "float32"


def test_from_transformers_copies_the_weights():
    import muse
    hf = _hf()
    enc = muse.T5TextEncoder.from_transformers(hf)
    want, own = hf.state_dict(), enc.state_dict()
    assert _same(own, want)
    assert all(own[k].data_ptr() != want[k].data_ptr() for k in want)       # a copy, not a view
    assert enc.config.relative_attention_num_buckets == 32 and enc.config.relative_attention_max_distance == 128


@pytest.mark.parametrize("num_buckets,max_distance", [(32, 128), (16, 64)])
def test_the_host_bucket_map_is_that_of_transformers(num_buckets, max_distance):
    """every signed distance j - i in -511 .. 511 (S = 512, the longest sequence), and the shorter vectors are its middle"""
    from muse.modeling_t5_text import rel_buckets
    from transformers.models.t5.modeling_t5 import T5Attention
    d = torch.arange(-511, 512)
    want = T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=num_buckets, max_distance=max_distance)
    got = rel_buckets(512, num_buckets, max_distance)
    assert got.dtype == torch.int64 and got.shape == (1023,) and torch.equal(got, want)
    assert int(got.min()) == 0 and int(got.max()) == num_buckets - 1
    for S in (1, 7, 33, 128):
        assert torch.equal(rel_buckets(S, num_buckets, max_distance), want[511 - (S - 1):511 + S])
    # as the [S, S] matrix transformers builds: memory position j minus query position i
    S = 40
    ctx, mem = torch.arange(S)[:, None], torch.arange(S)[None, :]
    full = T5Attention._relative_position_bucket(mem - ctx, bidirectional=True, num_buckets=num_buckets, max_distance=max_distance)
    assert torch.equal(rel_buckets(S, num_buckets, max_distance)[mem - ctx + S - 1], full)


@pytest.mark.parametrize("override", [dict(feed_forward_proj="relu"), dict(feed_forward_proj="gated-silu"), dict(d_kv=48), dict(d_kv=128),
                                      dict(d_model=100)])
def test_constructor_refusals(override):
    import muse
    with pytest.raises(NotImplementedError, match="outside the MI355X hot-path build"):
        muse.T5TextEncoder({**CFG, **override})


def test_loading_and_forward_refusals_need_no_device(tmp_path):
    import muse
    from muse._hip import MuseHipError
    enc = muse.T5TextEncoder(CFG)
    ids = torch.zeros((1, 5), dtype=torch.long)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        enc(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(ValueError, match="513"):
        enc(torch.zeros((1, 513), dtype=torch.long))
    with pytest.raises(MuseHipError):       # no CPU compute path: ops.require_gpu, as the CLIP class
        enc(ids)
    with pytest.raises(MuseHipError):
        enc(torch.zeros((1, 512), dtype=torch.long))
    # a sharded checkpoint: the index file is enough to refuse
    d = str(tmp_path / "sharded")
    _hf().save_pretrained(d)
    for index in ("model.safetensors.index.json", "pytorch_model.bin.index.json"):
        open(os.path.join(d, index), "w").write(json.dumps({"metadata": {}, "weight_map": {}}))
        with pytest.raises(NotImplementedError, match="sharded"):
            muse.T5TextEncoder.from_pretrained(d)
        os.remove(os.path.join(d, index))
    assert muse.T5TextEncoder.from_pretrained(d).config.num_layers == 3
    with pytest.raises(EnvironmentError):
        muse.T5TextEncoder.from_pretrained(str(tmp_path / "nothing_here"))


def test_casts_select_the_compute_mode_and_masters_stay_f32():
    import muse
    enc = muse.T5TextEncoder(CFG)
    for cast, want in ((lambda m: m.half(), torch.bfloat16), (lambda m: m.to(torch.float32), torch.float32),
                       (lambda m: m.to(dtype=torch.bfloat16), torch.bfloat16), (lambda m: m.float(), torch.float32),
                       (lambda m: m.set_compute_dtype(torch.bfloat16), torch.bfloat16)):
        assert cast(enc) is enc and enc.compute_dtype == want
        assert all(p.dtype == torch.float32 for p in enc.parameters())
    with pytest.raises(ValueError):
        enc.set_compute_dtype("bf16x3")
    # the cache of packed operands (the per-length bias included) is dropped when the mode changes or weights are loaded
    enc._packed[("rel", 7)] = torch.zeros(1)
    enc.set_compute_dtype(torch.float32)
    assert not enc._packed
    enc._packed[("rel", 7)] = torch.zeros(1)
    enc.load_state_dict(muse.T5TextEncoder(CFG).state_dict())
    assert not enc._packed
    enc._packed[("rel", 7)] = torch.zeros(1)
    enc.to("cpu")
    assert not enc._packed


def test_the_output_answers_by_attribute_key_and_position():
    from muse.modeling_t5_text import T5TextOutput
    last, hs = torch.zeros(1, 2, 4), (torch.zeros(1, 2, 4),)
    out = T5TextOutput(last_hidden_state=last)
    assert out.last_hidden_state is last and out[0] is last and out["last_hidden_state"] is last and out.hidden_states is None
    assert len(out.to_tuple()) == 1
    out["hidden_states"] = hs
    assert out.hidden_states is hs and out[1] is hs
    with pytest.raises(AttributeError):
        out.no_such_field


def test_pipeline_from_pretrained_picks_the_class_from_model_type(tmp_path):
    """native_text_encoder=True reads `model_type` from text_encoder/config.json: "t5" -> muse.T5TextEncoder (loading needs no device);
    the default stays the transformers class"""
    import inspect
    import muse
    import t5_tiny
    import weights as W
    assert inspect.signature(muse.PipelineMuse.from_pretrained).parameters["native_text_encoder"].default is False
    hf, tok, tcfg = t5_tiny.pipeline_parts()
    root = str(tmp_path / "ckpt")
    muse.PipelineMuse(vae=muse.MaskGitVQGAN(**W.VQGAN_TINY), transformer=muse.MaskGitTransformer(**tcfg), text_encoder=hf,
                      tokenizer=tok).save_pretrained(root)
    pipe = muse.PipelineMuse.from_pretrained(root, native_text_encoder=True)
    assert isinstance(pipe.text_encoder, muse.T5TextEncoder) and _same(pipe.text_encoder.state_dict(), hf.state_dict())
    assert pipe.tokenizer("a red fox").input_ids == tok("a red fox").input_ids
