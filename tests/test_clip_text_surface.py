"""muse.CLIPTextEncoder without a device: construction, the transformers parameter names, loading and saving transformers
directories, copying a live module, and every refusal.  (Numerics: tests/test_gpu_clip_text.py.)

Parameter names: the published checkpoints and CLIPTextModelWithProjection name the tower `text_model.*`.  Newer transformers'
CLIPTextModel IS the bare tower - its state dict drops that prefix and its checkpoints carry it as `base_model_prefix` - so both
classes' keys are compared with the prefix in place (`_with_prefix`)."""
import os

import pytest
import torch

CFG = dict(vocab_size=600, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=77, projection_dim=48, bos_token_id=598, eos_token_id=599, pad_token_id=599)


def _with_prefix(sd):
    return {(k if k.startswith(("text_model.", "text_projection.")) else "text_model." + k): v for k, v in sd.items()}


def _towers():
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(11)
    cfg = CLIPTextConfig(**CFG)
    return [(CLIPTextModelWithProjection, CLIPTextModelWithProjection(cfg).eval()), (CLIPTextModel, CLIPTextModel(cfg).eval())]


def test_state_dict_names_and_shapes_are_those_of_transformers():
    import muse
    assert "CLIPTextEncoder" in muse.__all__
    for klass, hf in _towers():
        want = _with_prefix(hf.state_dict())
        own = muse.CLIPTextEncoder(CFG, with_projection=klass.__name__ == "CLIPTextModelWithProjection").state_dict()
        assert set(own) == set(want), set(own) ^ set(want)
        assert all(tuple(own[k].shape) == tuple(want[k].shape) and own[k].dtype == torch.float32 for k in want)
        assert ("text_projection.weight" in own) == (klass.__name__ == "CLIPTextModelWithProjection")
    by_kwargs = muse.CLIPTextEncoder(**CFG)
    assert by_kwargs.config.hidden_size == 64 and by_kwargs.with_projection and not by_kwargs.training
    assert not any(p.requires_grad for p in by_kwargs.parameters())


def test_a_transformers_directory_loads_bit_equal(tmp_path):
    import muse
    for klass, hf in _towers():
        for safe in (True, False):      # model.safetensors and pytorch_model.bin
            d = str(tmp_path / f"{klass.__name__}_{safe}")
            hf.save_pretrained(d, safe_serialization=safe)
            if not safe and not os.path.isfile(os.path.join(d, "pytorch_model.bin")):    # a transformers that only writes safetensors
                os.remove(os.path.join(d, "model.safetensors"))
                torch.save(_with_prefix(hf.state_dict()), os.path.join(d, "pytorch_model.bin"))
            enc = muse.CLIPTextEncoder.from_pretrained(d, projection_dim=CFG["projection_dim"])
            want, own = _with_prefix(hf.state_dict()), enc.state_dict()
            assert set(own) == set(want) and all(torch.equal(own[k], want[k]) for k in want)
            assert enc.config.eos_token_id == 599 and enc.compute_dtype == torch.float32
    # the subfolder form PipelineMuse uses
    root = str(tmp_path / "ckpt")
    _towers()[0][1].save_pretrained(os.path.join(root, "text_encoder"))
    assert muse.CLIPTextEncoder.from_pretrained(root, subfolder="text_encoder").with_projection


def test_save_pretrained_writes_what_transformers_loads(tmp_path):
    import muse
    for klass, hf in _towers():
        enc = muse.CLIPTextEncoder.from_transformers(hf)
        d = str(tmp_path / klass.__name__)
        enc.save_pretrained(d)
        back, info = klass.from_pretrained(d, output_loading_info=True)
        assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
        want, got = hf.state_dict(), back.state_dict()
        assert set(want) == set(got) and all(torch.equal(want[k], got[k]) for k in want)
        assert back.config.hidden_act == "quick_gelu" and back.config.eos_token_id == 599


def test_from_transformers_copies_the_weights():
    import muse
    for klass, hf in _towers():
        enc = muse.CLIPTextEncoder.from_transformers(hf)
        want, own = _with_prefix(hf.state_dict()), enc.state_dict()
        assert set(own) == set(want) and all(torch.equal(own[k], want[k]) for k in want)
        assert all(own[k].data_ptr() != want[k].data_ptr() for k in want)       # a copy, not a view
        assert enc.with_projection == (klass.__name__ == "CLIPTextModelWithProjection")


def test_casts_select_the_compute_mode_and_masters_stay_f32():
    import muse
    enc = muse.CLIPTextEncoder(CFG)
    assert enc.compute_dtype == torch.float32
    for cast, want in ((lambda m: m.half(), torch.bfloat16), (lambda m: m.to(torch.float32), torch.float32),
                       (lambda m: m.to(dtype=torch.bfloat16), torch.bfloat16), (lambda m: m.float(), torch.float32),
                       (lambda m: m.set_compute_dtype(torch.bfloat16), torch.bfloat16)):
        assert cast(enc) is enc and enc.compute_dtype == want
        assert all(p.dtype == torch.float32 for p in enc.parameters())
    assert enc.requires_grad_(False) is enc and enc.eval() is enc and enc.to("cpu") is enc
    with pytest.raises(ValueError):
        enc.set_compute_dtype("bf16x3")


@pytest.mark.parametrize("override", [dict(num_attention_heads=4), dict(hidden_size=96, num_attention_heads=2), dict(max_position_embeddings=129),
                                      dict(hidden_act="gelu_new"), dict(attention_dropout=0.1)])
def test_constructor_refusals(override):
    import muse
    with pytest.raises(NotImplementedError, match="outside the MI355X hot-path build"):
        muse.CLIPTextEncoder({**CFG, **override})


def test_forward_refusals_and_the_contradicting_override(tmp_path):
    import muse
    enc = muse.CLIPTextEncoder(CFG)
    ids = torch.zeros((1, 5), dtype=torch.long)
    with pytest.raises(NotImplementedError):
        enc(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(NotImplementedError):
        enc(ids, position_ids=torch.arange(5)[None])
    from muse._hip import MuseHipError
    with pytest.raises(MuseHipError):       # no CPU compute path
        enc(ids)
    d = str(tmp_path / "tower")
    _towers()[0][1].save_pretrained(d)
    with pytest.raises(ValueError, match="contradicts"):
        muse.CLIPTextEncoder.from_pretrained(d, projection_dim=CFG["projection_dim"] + 16)
    # without a stored projection the override has nothing to contradict
    d2 = str(tmp_path / "bare")
    _towers()[1][1].save_pretrained(d2)
    assert not muse.CLIPTextEncoder.from_pretrained(d2, projection_dim=768).with_projection


def test_pipeline_from_pretrained_keeps_the_transformers_tower_by_default():
    """the opt-in switch exists and defaults to off (the default class is pinned by the existing pipeline tests)"""
    import inspect
    import muse
    p = inspect.signature(muse.PipelineMuse.from_pretrained).parameters["native_text_encoder"]
    assert p.default is False


def test_output_fields_that_were_not_set_read_as_none():
    """as transformers' ModelOutput: `out.hidden_states is None` when they were not asked for; an unknown name still raises"""
    from muse.modeling_clip_text import CLIPTextOutput
    out = CLIPTextOutput(last_hidden_state=torch.zeros(1, 2, 4), pooler_output=torch.zeros(1, 4))
    assert out.hidden_states is None and out.text_embeds is None and out.attentions is None
    assert out.last_hidden_state is out[0] and out.pooler_output is out[1] and len(out.to_tuple()) == 2
    with pytest.raises(AttributeError):
        out.no_such_field


def test_load_state_dict_assign_adopts_the_tensors():
    import muse
    src, enc = muse.CLIPTextEncoder(CFG), muse.CLIPTextEncoder(CFG)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    enc.load_state_dict(sd, assign=True)
    own = enc.state_dict()
    assert all(own[k].data_ptr() == sd[k].data_ptr() for k in sd)            # adopted, not copied
    assert not any(p.requires_grad for p in enc.parameters())
    enc.load_state_dict(src.state_dict())                                       # the default still copies
    assert all(enc.state_dict()[k].data_ptr() != src.state_dict()[k].data_ptr() for k in sd)


def test_save_pretrained_writes_one_dtype_key(tmp_path):
    """a source config's `torch_dtype` (older transformers' spelling of `dtype`) is not carried beside the float32 `dtype`"""
    import json
    import muse
    enc = muse.CLIPTextEncoder(dict(CFG, torch_dtype="float16"))
    enc.save_pretrained(str(tmp_path))
    cfg = json.load(open(os.path.join(str(tmp_path), "config.json")))
    assert cfg["dtype"] == "float32" and "torch_dtype" not in cfg
