"""The MoVQ tokenizer's surface without a GPU: module path, constructor and state-dict template, checkpoint round trip, compute modes,
the no-CPU-path rule and the other refusals, how the class is bound (the top-level name stays the stub; a pipeline takes it through
`vae=`), and the CPU restatement (tests/movq_cpu.py) against the real reference's goldens."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import movq_cpu as P  # noqa: E402
import movq_weights as MW  # noqa: E402

FIXTURES = sorted(MW.FIXTURES)


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _plain(cfg):
    return json.loads(json.dumps(cfg))      # tuples as lists, the way config.json and the goldens store them


def test_module_path_constructor_and_state_dict_template(golden_dir):
    from muse.modeling_movq import MOVQ
    sig = inspect.signature(MOVQ.__init__)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(
        resolution=256, num_channels=3, out_channels=3, hidden_channels=128, channel_mult=(1, 2, 2, 4), num_res_blocks=2,
        attn_resolutions=(32,), z_channels=4, double_z=False, num_embeddings=16384, quantized_embed_dim=4, dropout=0.0,
        resample_with_conv=True, commitment_cost=0.25)
    assert not hasattr(MOVQ, "get_soft_code")
    for name in FIXTURES:
        g = _golden(golden_dir, name)
        cfg = json.loads(str(g["config"]))
        assert cfg == _plain(MW.FIXTURES[name])
        want = {k: tuple(v) for k, v in json.loads(str(g["shapes"])).items()}       # recorded from the reference's own state dict
        model = MOVQ(**MW.FIXTURES[name])
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want
        assert {k: tuple(v) for k, v in MW.movq_shapes(cfg).items()} == want
        model.load_state_dict(MW.fill_movq(MW.movq_shapes(cfg), int(g["seed"])), strict=True)
        assert model.config.num_resolutions == len(cfg["channel_mult"])
        assert model.config.reduction_factor == 2 ** (len(cfg["channel_mult"]) - 1)
        assert model.config.latent_size == cfg["resolution"] // model.config.reduction_factor
    assert sum(v.numel() for v in MOVQ(**MW.MOVQ_TINY).state_dict().values()) == 937103
    with torch.device("meta"):
        shipped = MOVQ()
    assert {k: tuple(v.shape) for k, v in shipped.state_dict().items()} == MW.movq_shapes(MW.MOVQ_SHIPPED)
    assert tuple(shipped.state_dict()["decoder.up.0.block.0.norm2.conv_y.weight"].shape) == (128, 4, 1, 1)
    assert tuple(shipped.state_dict()["decoder.mid.attn_1.q.weight"].shape) == (512, 512)


def test_save_and_load_round_trip(tmp_path):
    from muse.modeling_movq import MOVQ
    cfg = MW.MOVQ_TINY
    model = MOVQ(**cfg)
    model.load_state_dict(MW.fill_movq(MW.movq_shapes(cfg), 3), strict=True)
    model.save_pretrained(str(tmp_path))
    stored = json.load(open(os.path.join(str(tmp_path), "config.json")))
    assert stored["_class_name"] == "MOVQ"
    assert {k: stored[k] for k in cfg} == _plain(cfg)
    back = MOVQ.from_pretrained(str(tmp_path))
    assert dict(back.config)["hidden_channels"] == 32 and back.compute_dtype == torch.float32
    want, got = model.state_dict(), back.state_dict()
    assert set(want) == set(got) and all(torch.equal(want[k], got[k]) for k in want)
    model.load_state_dict(back.state_dict(), strict=True)      # and the other way


def test_compute_modes():
    from muse.modeling_movq import MOVQ
    model = MOVQ(**MW.MOVQ_TINY)
    assert model.compute_dtype == torch.float32
    assert model.half().compute_dtype == "bf16x3" and all(p.dtype == torch.float32 for p in model.parameters())
    assert model.float().compute_dtype == torch.float32
    assert model.to(dtype=torch.bfloat16).compute_dtype == "bf16x3" and next(model.parameters()).dtype == torch.float32
    with pytest.raises(ValueError):
        model.set_compute_dtype(torch.bfloat16)
    assert model.set_compute_dtype(torch.float32) is model


def test_packed_weights_are_dropped_on_apply_and_load():
    from muse.modeling_movq import MOVQ
    model = MOVQ(**MW.MOVQ_TINY)
    norm = model.decoder.norm_out
    gamma, beta, wy, by, wb, bb = model._sn_weights(norm)
    assert tuple(wy.shape) == (32, 4) and tuple(wb.shape) == (32, 4) and wy.is_contiguous()
    assert torch.equal(wy, norm.conv_y.weight.data.view(32, 4)) and torch.equal(bb, norm.conv_b.bias.data)
    att = model.decoder.mid.attn_1
    assert tuple(model._qkv(att).weight.shape) == (192, 64, 1, 1) and torch.equal(model._qkv(att).weight[64:128, :, 0, 0], att.k.weight.data)
    assert model._packed
    model.load_state_dict(model.state_dict())
    assert not model._packed
    model._sn_weights(norm)
    model.cpu()                                      # any nn.Module._apply
    assert not model._packed


def test_refusals():
    from muse._hip import MuseHipError
    from muse.modeling_movq import MOVQ
    model = MOVQ(**MW.MOVQ_TINY)
    px = MW.movq_images(1, 32, 32, 1)
    with pytest.raises(MuseHipError):
        model.get_code(px)
    with pytest.raises(MuseHipError):
        model.encode(px)
    with pytest.raises(MuseHipError):
        model.decode_code(torch.zeros((1, 256), dtype=torch.int64))
    with pytest.raises(MuseHipError):
        model.decode(torch.zeros((1, 4, 16, 16)))
    with pytest.raises(ValueError):
        MOVQ(**MW.MOVQ_TINY3).get_code(MW.movq_images(1, 30, 32, 1))        # 30 is no multiple of the reduction factor 4
    with pytest.raises(NotImplementedError):
        MOVQ(**dict(MW.MOVQ_TINY, dropout=0.1))
    with pytest.raises(NotImplementedError, match="beta"):
        model.encode(px, return_loss=True)
    with pytest.raises(NotImplementedError, match="beta"):
        model(px, return_loss=True)


def test_the_top_level_name_is_still_the_stub():
    import muse
    import muse.modeling_movq
    assert muse.MOVQ is not muse.modeling_movq.MOVQ
    with pytest.raises(NotImplementedError, match="not part of the MI355X hot-path build") as e:
        muse.MOVQ()
    assert "muse.modeling_movq" in str(e.value)             # ... and says where the built class lives


def test_a_pipeline_takes_it_through_the_vae_argument():
    import muse
    import weights as W
    from muse.modeling_movq import MOVQ
    vae = MOVQ(**MW.MOVQ_TINY)
    pipe = muse.PipelineMuse(vae=vae, transformer=muse.MaskGitTransformer(**W.TRANSFORMER_TINY), is_class_conditioned=True)
    assert pipe.vae is vae


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_restatement_reproduces_the_reference_goldens(golden_dir, name):
    g = _golden(golden_dir, name)
    cfg = MW.FIXTURES[name]
    seed, side = int(g["seed"]), cfg["resolution"]
    assert float(g["margin"]) >= 1e-3
    sd = MW.fill_movq(MW.movq_shapes(cfg), seed)
    px = MW.movq_images(int(g["batch"]), side, side, seed + 1)
    tol = dict(rtol=1e-5, atol=1e-5)         # what tests/test_oracle_golden.py holds the taming restatement to
    with torch.no_grad():
        z, z_q, idx = P.encode(sd, cfg, px)
        np.testing.assert_allclose(z.numpy(), g["z"], **tol)
        assert np.array_equal(idx.numpy(), g["indices"])
        np.testing.assert_allclose(z_q.numpy(), g["z_q"], rtol=0, atol=0)
        np.testing.assert_allclose(P.decode_code(sd, cfg, idx).numpy(), g["rec"], **tol)
        np.testing.assert_allclose(P.decode(sd, cfg, z_q).numpy(), g["rec_decode"], **tol)
        ns = P.get_code(sd, cfg, MW.movq_images(1, *MW.NONSQUARE, seed + 2))
        assert np.array_equal(ns.numpy(), g["code_nonsquare"])
        assert np.array_equal(P.get_code(sd, cfg, px, torch.float64).numpy(), g["indices"])


def test_restated_nearest_is_interpolate_nearest():
    """the index map the kernel implements (oy // (H / zh), ox // (W / zw)) is F.interpolate(mode="nearest") for integer factors,
    independent per axis"""
    import torch.nn.functional as F
    zq = torch.randn((2, 4, 3, 5), generator=torch.Generator().manual_seed(1))
    for fy, fx in ((1, 1), (2, 2), (4, 2), (1, 8), (3, 2)):
        H, W = 3 * fy, 5 * fx
        iy, ix = torch.arange(H) // fy, torch.arange(W) // fx
        want = zq[:, :, iy][:, :, :, ix]
        assert torch.equal(F.interpolate(zq, size=(H, W), mode="nearest"), want) and torch.equal(P.nearest(zq, H, W), want)
        # the shifted maps of the index test: one source pixel off along each axis (clamped at the border)
        assert torch.equal(P.nearest(zq, H, W, (1, 0)), zq[:, :, (iy + 1).clamp(max=2)][:, :, :, ix])
        assert torch.equal(P.nearest(zq, H, W, (0, -1)), zq[:, :, iy][:, :, :, (ix - 1).clamp(min=0)])
