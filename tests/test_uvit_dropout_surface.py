"""muse.MaskGiTUViT with hidden_dropout / attention_dropout > 0, without a device: construction, the config round trip, the
state dict (dropout has no parameters), the numbering of the dropout sites and the refusals.  (Numerics: tests/test_gpu_uvit_dropout.py.)"""
import pytest
import torch

NARROW = dict(vocab_size=264, codebook_size=256, hidden_size=128, in_channels=64, block_out_channels=(128,), encoder_hidden_size=64,
              cond_embed_dim=32, micro_cond_encode_dim=8, micro_cond_embed_dim=40, num_hidden_layers=2, num_attention_heads=2,
              intermediate_size=256, block_num_heads=2, num_res_blocks=1)


def test_constructs_with_dropout_and_has_no_new_parameters():
    import muse
    plain = muse.MaskGiTUViT(**NARROW)
    model = muse.MaskGiTUViT(**NARROW, hidden_dropout=0.1, attention_dropout=0.2)
    assert model.config.hidden_dropout == 0.1 and model.config.attention_dropout == 0.2
    a, b = plain.state_dict(), model.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    for p in (0.0, 0.999):
        muse.MaskGiTUViT(**NARROW, hidden_dropout=p, attention_dropout=p)


def test_config_round_trip(tmp_path):
    import muse
    model = muse.MaskGiTUViT(**NARROW, hidden_dropout=0.1, attention_dropout=0.2)
    model.save_pretrained(str(tmp_path))
    cfg = muse.MaskGiTUViT.load_config(str(tmp_path))
    assert cfg["hidden_dropout"] == 0.1 and cfg["attention_dropout"] == 0.2
    again = muse.MaskGiTUViT.from_pretrained(str(tmp_path))
    assert again.config.hidden_dropout == 0.1 and again.config.attention_dropout == 0.2
    own, back = model.state_dict(), again.state_dict()
    assert list(own) == list(back) and all(torch.equal(own[k], back[k]) for k in own)


@pytest.mark.parametrize("extra", [dict(), dict(num_res_blocks=3, num_hidden_layers=5)])
def test_dropout_sites_are_numbered_once_in_forward_order(extra):
    import muse
    cfg = dict(NARROW, **extra)
    model = muse.MaskGiTUViT(**cfg, hidden_dropout=0.1, attention_dropout=0.2)
    B, S, L = 2, 256, 77
    sites = model.dropout_sites(B, S, L)
    nrb, nl = cfg["num_res_blocks"], cfg["num_hidden_layers"]
    assert len(sites) == 2 * 3 * nrb + 3 * nl
    offsets = [s[2] for s in sites]
    assert offsets == [(k + 1) << 40 for k in range(len(sites))] and all(a < b for a, b in zip(offsets, offsets[1:]))
    names = [s[0] for s in sites]
    assert len(set(names)) == len(names)
    assert names[:3] == ["down_blocks.0.res_blocks.0.channelwise.3", "down_blocks.0.attention_blocks.0.attention.dropout",
                         "down_blocks.0.attention_blocks.0.crossattention.dropout"]
    assert names[3 * nrb:3 * nrb + 3] == ["transformer_layers.0.attention.dropout", "transformer_layers.0.crossattention.dropout",
                                          "transformer_layers.0.ffn.dropout"]
    assert names[3 * nrb + 3 * nl] == "up_blocks.0.res_blocks.0.channelwise.3"
    by_name = {s[0]: s for s in sites}
    C = cfg["block_out_channels"][0]
    assert by_name["down_blocks.0.res_blocks.0.channelwise.3"][1:] == ("hidden", 1 << 40, (B * S, 4 * C))
    assert by_name["transformer_layers.0.ffn.dropout"][1] == "hidden"
    assert by_name["transformer_layers.0.ffn.dropout"][3] == (B * S, cfg["intermediate_size"])
    assert by_name["transformer_layers.1.attention.dropout"][3] == (B * cfg["num_attention_heads"], S, 256)
    assert by_name["transformer_layers.1.crossattention.dropout"][3] == (B * cfg["num_attention_heads"], S, 80)      # round_up(77, 8)
    assert sites[-1][:3] == (f"up_blocks.0.attention_blocks.{nrb - 1}.crossattention.dropout", "attention", len(sites) << 40)
    # (both attentions of a conv-stage block read the text states: reference :821-826)
    assert by_name["up_blocks.0.attention_blocks.0.attention.dropout"][3] == (B * cfg["block_num_heads"], S, 80)
    assert by_name["down_blocks.0.attention_blocks.0.crossattention.dropout"][3] == (B * cfg["block_num_heads"], S, 80)


@pytest.mark.parametrize("key", ["hidden_dropout", "attention_dropout"])
@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_probabilities_outside_the_half_open_unit_interval_are_refused(key, p):
    import muse
    with pytest.raises(ValueError, match=key):
        muse.MaskGiTUViT(**NARROW, **{key: p})


def test_the_other_refusals_keep_their_text():
    import muse
    for extra in (dict(use_bias=True), dict(use_fused_mlp=True)):
        with pytest.raises(NotImplementedError, match="only the bias-free GLU family is built"):
            muse.MaskGiTUViT(**NARROW, hidden_dropout=0.1, **extra)


def test_hip_graph_decoding_refuses_a_training_mode_model_with_dropout():
    """a captured forward would bake one dropout seed into its launches: refused before anything is captured (eval() decodes as before)"""
    import muse
    from muse._hip import MuseHipError
    model = muse.MaskGiTUViT(**NARROW, hidden_dropout=0.1).train()
    enc, cond, micro = torch.zeros(1, 77, 64), torch.zeros(1, 32), torch.tensor([[256.0, 256.0, 0.0, 0.0, 6.0]])
    with pytest.raises(MuseHipError, match="hip_graph=True.*training mode with dropout"):
        model.generate2(enc, cond, micro, enc, cond, timesteps=2, hip_graph=True)
