"""muse.CLIPImageEncoder / CLIPScorer / clip_scores without a device: names, parameter layout, checkpoint round trips against
transformers' own classes, the refusals, and the absence of a CPU compute path."""
import inspect
import json
import os

import pytest
import torch

import clip_vision_cpu as CV

TINY = (64, 2, 28, 14)


def _same(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


def test_the_names_are_exported():
    import muse
    import muse.modeling_clip_vision as M
    assert muse.CLIPImageEncoder is M.CLIPImageEncoder and muse.CLIPScorer is M.CLIPScorer and muse.clip_scores is M.clip_scores
    for name in ("CLIPImageEncoder", "CLIPScorer", "clip_scores"):
        assert name in muse.__all__
    assert list(inspect.signature(muse.clip_scores).parameters) == ["image_embeds", "text_embeds", "logit_scale"]
    assert list(inspect.signature(muse.CLIPScorer.__init__).parameters)[1:] == ["image_encoder", "text_encoder", "tokenizer"]
    assert list(inspect.signature(muse.CLIPScorer.__call__).parameters)[1:] == ["images", "text", "input_ids", "text_embeds", "pixel_values"]
    from muse import _hip, ops
    for sym, fn in (("muse_resize_bicubic_norm_f32", ops.resize_bicubic_norm), ("muse_clip_patch_rows", ops.clip_patch_rows),
                    ("muse_clip_vision_embed_ln", ops.clip_vision_embed_ln), ("muse_l2_normalize_rows", ops.l2_normalize_rows)):
        assert sym in _hip.SIGNATURES and callable(fn)


def test_state_dict_is_upstreams_plus_logit_scale():
    import muse
    hf, _ = CV.tower(*TINY)
    enc = muse.CLIPImageEncoder.from_transformers(hf)
    want = {k: v for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    got = enc.state_dict()
    assert set(got) == set(want) | {"logit_scale"}
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == torch.float32 and torch.equal(got[k], v), k
    assert got["logit_scale"].shape == () and abs(float(got["logit_scale"]) - 2.6592600) < 1e-6          # ln(1 / 0.07)
    assert "vision_model.pre_layrnorm.weight" in got and "vision_model.embeddings.class_embedding" in got
    assert not any(p.requires_grad for p in enc.parameters()) and not enc.training
    assert enc.tokens == 5 and enc.image_mean == pytest.approx(CV.MEAN) and enc.image_std == pytest.approx(CV.STD)


def test_casts_select_the_compute_mode_and_masters_stay_f32():
    import muse
    enc = muse.CLIPImageEncoder.from_transformers(CV.tower(*TINY)[0])
    assert enc.compute_dtype == torch.float32
    for dtype in (torch.bfloat16, torch.float16):
        assert enc.to(dtype=dtype).compute_dtype == torch.bfloat16
        assert all(p.dtype == torch.float32 for p in enc.parameters())
        assert enc.to(dtype=torch.float32).compute_dtype == torch.float32


def test_round_trip_through_a_directory_is_bit_exact(tmp_path):
    import muse
    from transformers import CLIPVisionModelWithProjection
    hf, _ = CV.tower(*TINY)
    enc = muse.CLIPImageEncoder.from_transformers(hf)
    enc.logit_scale.data.fill_(3.25)
    d = str(tmp_path / "vision")
    enc.save_pretrained(d)
    assert sorted(os.listdir(d)) == ["config.json", "model.safetensors", "preprocessor_config.json"]
    back = muse.CLIPImageEncoder.from_pretrained(d)
    assert _same(back.state_dict(), enc.state_dict()) and float(back.logit_scale) == 3.25
    for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size", "projection_dim",
              "hidden_act", "layer_norm_eps"):
        assert back.config[k] == enc.config[k] == getattr(hf.config, k), k
    again = CLIPVisionModelWithProjection.from_pretrained(d)            # upstream reads the directory too
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in hf.state_dict().items())
    # a preprocessor_config.json next to the checkpoint overrides the normalisation constants
    pre = json.load(open(os.path.join(d, "preprocessor_config.json")))
    pre.update(image_mean=[0.5, 0.5, 0.5], image_std=[0.25, 0.5, 1.0])
    json.dump(pre, open(os.path.join(d, "preprocessor_config.json"), "w"))
    other = muse.CLIPImageEncoder.from_pretrained(d)
    assert other.image_mean == (0.5, 0.5, 0.5) and other.image_std == (0.25, 0.5, 1.0)
    # pytorch_model.bin is read as well; a sharded checkpoint is refused
    b = str(tmp_path / "bin")
    os.makedirs(b)
    json.dump(dict(enc.config), open(os.path.join(b, "config.json"), "w"))
    torch.save({k: v.clone() for k, v in hf.state_dict().items()}, os.path.join(b, "pytorch_model.bin"))
    from_bin = muse.CLIPImageEncoder.from_pretrained(b)
    assert all(torch.equal(v, from_bin.state_dict()[k]) for k, v in hf.state_dict().items())
    assert abs(float(from_bin.logit_scale) - 2.6592600) < 1e-6          # the checkpoint has none
    open(os.path.join(b, "model.safetensors.index.json"), "w").write("{}")
    with pytest.raises(NotImplementedError, match="sharded checkpoint.*outside the MI355X hot-path build"):
        muse.CLIPImageEncoder.from_pretrained(b)


def test_a_full_clip_model_checkpoint_loads_the_same_tower(tmp_path):
    import muse
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(11)
    vcfg = CV.vision_config(*TINY).to_dict()
    clip = CLIPModel(CLIPConfig(text_config=dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                 num_attention_heads=2, max_position_embeddings=16, bos_token_id=98, eos_token_id=99,
                                                 pad_token_id=99),
                                vision_config=vcfg, projection_dim=CV.PROJ)).eval()
    clip.logit_scale.data.fill_(4.0)
    live = muse.CLIPImageEncoder.from_transformers(clip)
    sd = clip.state_dict()
    for k, v in live.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert float(live.logit_scale) == 4.0 and not any(k.startswith("text_") for k in live.state_dict())
    d = str(tmp_path / "clip")
    clip.save_pretrained(d)
    assert "vision_config" in json.load(open(os.path.join(d, "config.json")))
    assert _same(muse.CLIPImageEncoder.from_pretrained(d).state_dict(), live.state_dict())


@pytest.mark.parametrize("kw,words", [
    (dict(hidden_size=160, num_attention_heads=2), "head_dim 80"),
    (dict(hidden_size=64, num_attention_heads=4), "head_dim 16"),
    (dict(hidden_act="relu"), "hidden_act 'relu'"),
    (dict(attention_dropout=0.1), "attention_dropout"),
    (dict(image_size=30, patch_size=14), "image_size 30"),
    (dict(image_size=350, patch_size=14), "626 tokens"),
])
def test_refusals(kw, words):
    import muse
    cfg = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14, projection_dim=16)
    muse.CLIPImageEncoder({**cfg})
    with pytest.raises(NotImplementedError, match="outside the MI355X hot-path build") as e:
        muse.CLIPImageEncoder({**cfg, **kw})
    assert words in str(e.value)


def test_forward_refusals_and_no_cpu_path():
    import muse
    from muse._hip import MuseHipError
    enc = muse.CLIPImageEncoder.from_transformers(CV.tower(*TINY)[0])
    px = torch.zeros(2, 3, 28, 28)
    with pytest.raises(NotImplementedError, match="interpolate_pos_encoding=True is outside the MI355X hot-path build"):
        enc(px, interpolate_pos_encoding=True)
    for bad in (torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 28, 42)):
        with pytest.raises(ValueError, match="doesn't match model"):
            enc(bad)
    with pytest.raises(ValueError):
        enc(None)
    with pytest.raises(MuseHipError, match="no CPU compute path"):
        enc(px)
    with pytest.raises(MuseHipError, match="no CPU compute path"):
        muse.clip_scores(torch.zeros(2, 8), torch.zeros(3, 8))
    scorer = muse.CLIPScorer(enc)
    with pytest.raises(MuseHipError, match="no CPU compute path"):
        scorer(torch.zeros(2, 3, 16, 16), text_embeds=torch.zeros(2, CV.PROJ))
    with pytest.raises(ValueError):
        scorer(torch.zeros(2, 3, 16, 16), pixel_values=px, text_embeds=torch.zeros(2, CV.PROJ))
    assert list(inspect.signature(enc.forward).parameters)[:1] == ["pixel_values"]
    for name in ("output_hidden_states", "return_dict"):
        assert inspect.signature(enc.forward).parameters[name].default is None
