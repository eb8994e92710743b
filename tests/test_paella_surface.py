"""The Paella VQ tokenizer's surface without a GPU: module path and state-dict template, checkpoint round trip, the no-CPU-path rule,
PipelineMuse's loader, the CPU restatement (tests/paella_cpu.py) against the real reference's goldens, and the gather layout /
transposed-convolution tap table / unshuffle channel order the HIP kernels are built on."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paella_cpu as P  # noqa: E402
import paella_weights as PW  # noqa: E402

FIXTURES = sorted(PW.FIXTURES)


def maxrel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def test_module_path_constructor_and_state_dict_template(golden_dir):
    from muse.modeling_paella_vq import PaellaVQModel
    sig = inspect.signature(PaellaVQModel.__init__)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(
        levels=2, bottleneck_blocks=12, c_hidden=384, c_latent=4, codebook_size=8192, scale_factor=0.3764)
    assert not hasattr(PaellaVQModel, "get_soft_code")
    for name in FIXTURES:
        g = _golden(golden_dir, name)
        cfg = json.loads(str(g["config"]))
        assert cfg == PW.FIXTURES[name][0]
        want = {k: tuple(v) for k, v in json.loads(str(g["shapes"])).items()}
        model = PaellaVQModel(**cfg)
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want
        assert PW.paella_shapes(cfg).keys() == want.keys()
        model.load_state_dict(PW.fill_paella(PW.paella_shapes(cfg), int(g["seed"])), strict=True)
    default = dict(PW.PAELLA_TINY, bottleneck_blocks=12, c_hidden=384, codebook_size=8192)
    assert {k: tuple(v.shape) for k, v in PaellaVQModel().state_dict().items()} == PW.paella_shapes(default)


def test_save_and_load_round_trip(tmp_path):
    from muse.modeling_paella_vq import PaellaVQModel
    cfg = PW.PAELLA_TINY
    model = PaellaVQModel(**cfg)
    model.load_state_dict(PW.fill_paella(PW.paella_shapes(cfg), 3), strict=True)
    model.save_pretrained(str(tmp_path))
    stored = json.load(open(os.path.join(str(tmp_path), "config.json")))
    assert stored["_class_name"] == "PaellaVQModel"
    assert {k: stored[k] for k in cfg} == cfg
    back = PaellaVQModel.from_pretrained(str(tmp_path))
    assert dict(back.config)["levels"] == 2 and back.compute_dtype == torch.float32
    want, got = model.state_dict(), back.state_dict()
    assert set(want) == set(got) and all(torch.equal(want[k], got[k]) for k in want)
    assert back.half().compute_dtype == "bf16x3" and next(back.parameters()).dtype == torch.float32
    assert back.float().compute_dtype == torch.float32
    with pytest.raises(ValueError):
        back.set_compute_dtype(torch.bfloat16)


def test_there_is_no_cpu_path():
    from muse._hip import MuseHipError
    from muse.modeling_paella_vq import PaellaVQModel
    model = PaellaVQModel(**PW.PAELLA_TINY)
    px = PW.paella_images(1, 32, 32, 1)
    with pytest.raises(MuseHipError):
        model.get_code(px)
    with pytest.raises(MuseHipError):
        model.decode_code(torch.zeros((1, 64), dtype=torch.int64))
    with pytest.raises(ValueError):
        model.get_code(PW.paella_images(1, 30, 32, 1))       # not a multiple of 2 ** levels


def test_pipeline_loader_dispatches_on_the_class_name(tmp_path):
    import muse
    import weights as W
    from muse.modeling_paella_vq import PaellaVQModel
    cfg = PW.PAELLA_TINY
    model = PaellaVQModel(**cfg)
    model.load_state_dict(PW.fill_paella(PW.paella_shapes(cfg), 4), strict=True)
    model.save_pretrained(os.path.join(str(tmp_path), "vae"))
    pipe = muse.PipelineMuse.from_pretrained(str(tmp_path), transformer=muse.MaskGitTransformer(**W.TRANSFORMER_TINY), is_class_conditioned=True)
    assert type(pipe.vae) is PaellaVQModel and dict(pipe.vae.config)["c_hidden"] == 48
    assert torch.equal(pipe.vae.state_dict()["vquantizer.codebook.weight"], model.state_dict()["vquantizer.codebook.weight"])
    # a class the build does not have is still refused by name
    cfg_path = os.path.join(str(tmp_path), "vae", "config.json")
    stored = json.load(open(cfg_path))
    json.dump(dict(stored, _class_name="MOVQ"), open(cfg_path, "w"))
    with pytest.raises(ValueError, match="Unknown VAE class"):
        muse.PipelineMuse.from_pretrained(str(tmp_path), transformer=pipe.transformer, is_class_conditioned=True)


def test_the_top_level_name_is_still_the_stub():
    import muse
    with pytest.raises(NotImplementedError):
        muse.PaellaVQModel()


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_restatement_reproduces_the_reference_goldens(golden_dir, name):
    g = _golden(golden_dir, name)
    cfg, side = PW.FIXTURES[name]
    seed = int(g["seed"])
    assert float(g["margin"]) >= 1e-3
    sd = PW.fill_paella(PW.paella_shapes(cfg), seed)
    px = PW.paella_images(int(g["batch"]), side, side, seed + 1)
    tol = dict(rtol=1e-5, atol=1e-5)         # what tests/test_oracle_golden.py holds the taming restatement to
    with torch.no_grad():
        z, z_q, idx = P.encode(sd, cfg, px)
        np.testing.assert_allclose(z.numpy(), g["z"], **tol)
        assert np.array_equal(idx.numpy(), g["indices"])
        np.testing.assert_allclose(z_q.numpy(), g["z_q"], rtol=0, atol=0)
        np.testing.assert_allclose(P.decode_code(sd, cfg, idx).numpy(), g["rec"], **tol)
        np.testing.assert_allclose(P.decode(sd, cfg, z_q).numpy(), g["rec_decode"], **tol)
        ns = P.get_code(sd, cfg, PW.paella_images(1, *PW.NONSQUARE, seed + 2))
        assert np.array_equal(ns.numpy(), g["code_nonsquare"])
        assert np.array_equal(P.get_code(sd, cfg, px, torch.float64).numpy(), g["indices"])


def test_gather_layout_tap_table_and_unshuffle_order():
    gen = torch.Generator().manual_seed(11)
    assert P.UP_TAPS == {(0, 0): 3, (0, 1): 1, (1, 0): 2, (1, 1): 0}
    for B, H, W, cin, cout in ((1, 2, 2, 8, 12), (2, 6, 10, 8, 12), (1, 5, 3, 4, 8)):
        x = torch.randn((B, H, W, cin), generator=gen, dtype=torch.float64)
        bias = torch.randn(cout, generator=gen, dtype=torch.float64)
        if H % 2 == 0 and W % 2 == 0:
            w = torch.randn((cout, cin, 4, 4), generator=gen, dtype=torch.float64)
            want = F.conv2d(x.permute(0, 3, 1, 2), w, bias, stride=2, padding=1).permute(0, 2, 3, 1)
            assert maxrel(P.conv_down_by_rows(x, w, bias), want) < 1e-6
        wt = torch.randn((cin, cout, 4, 4), generator=gen, dtype=torch.float64)
        want = F.conv_transpose2d(x.permute(0, 3, 1, 2), wt, bias, stride=2, padding=1).permute(0, 2, 3, 1)
        assert maxrel(P.conv_up_by_rows(x, wt, bias), want) < 1e-6
    # the model's own packing of the two weights is the one pinned above
    from muse.modeling_paella_vq import PaellaVQModel
    conv, convt = torch.nn.Conv2d(8, 12, 4, 2, 1), torch.nn.ConvTranspose2d(8, 12, 4, 2, 1)
    assert torch.equal(PaellaVQModel._w_down(conv)[0], P.down_weight_rows(conv.weight.data).contiguous())
    phases = PaellaVQModel._w_up(convt)[0]
    assert all(torch.equal(phases[2 * a + b], P.up_weight_rows(convt.weight.data, a, b).contiguous()) for a in (0, 1) for b in (0, 1))
    # PixelUnshuffle(2): channel c * 4 + dy * 2 + dx - not space_to_depth2's (dy, dx, c)
    img = torch.randn((2, 3, 6, 4), generator=gen)
    assert torch.equal(P.unshuffle2(img), F.pixel_unshuffle(img, 2))
    assert torch.equal(P.shuffle2(P.unshuffle2(img)), img) and torch.equal(P.shuffle2(P.unshuffle2(img)), F.pixel_shuffle(F.pixel_unshuffle(img, 2), 2))
    u = P.unshuffle2(img)
    for c in range(3):
        for dy in (0, 1):
            for dx in (0, 1):
                assert torch.equal(u[:, c * 4 + dy * 2 + dx], img[:, c, dy::2, dx::2])
    # the BatchNorm fold of the last encoder stage is the eval-mode BatchNorm
    stage = torch.nn.ModuleList([torch.nn.Conv2d(8, 4, 1, bias=False), torch.nn.BatchNorm2d(4)])
    stage[1].running_mean.normal_(generator=gen)
    stage[1].running_var.uniform_(0.5, 1.5, generator=gen)
    stage[1].weight.data.normal_(generator=gen)
    stage[1].bias.data.normal_(generator=gen)
    stage.eval()
    t = torch.randn((2, 8, 3, 3), generator=gen)
    wl, bl = PaellaVQModel._w_latent(stage)
    with torch.no_grad():
        assert maxrel(F.conv2d(t, wl[:, :, None, None], bl), stage[1](stage[0](t))) < 1e-6
