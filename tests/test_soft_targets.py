"""CPU: the surface of soft-target training (config.training.use_soft_code_target) and the self-consistency of its golden
(tests/golden/soft_target_tiny.npz, made by tests/golden/make_golden_soft.py from the real reference)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import weights as W


def test_soft_target_cross_entropy_is_importable_and_private_to_training():
    import muse
    from muse.training import soft_target_cross_entropy
    assert callable(soft_target_cross_entropy)
    # the reference defines it in the training script, not in the package namespace
    assert "soft_target_cross_entropy" not in muse.__all__
    assert list(inspect.signature(soft_target_cross_entropy).parameters) == ["logits", "labels", "soft_targets"]


def test_soft_target_kwargs_are_accepted_with_unchanged_defaults():
    import muse
    sig = inspect.signature(muse.prepare_inputs_and_labels).parameters
    assert (sig["use_soft_code_target"].default, sig["soft_code_temp"].default, sig["use_stochastic_code"].default) == (False, 1.0, False)
    sig = inspect.signature(muse.TrainStep).parameters
    assert (sig["use_soft_code_target"].default, sig["soft_code_temp"].default, sig["use_stochastic_code"].default) == (False, 1.0, False)
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    step = muse.TrainStep(None, m, muse.FusedAdamW(m.parameters()), use_soft_code_target=True, soft_code_temp=0.5,
                          use_stochastic_code=True)
    assert (step.use_soft_code_target, step.soft_code_temp, step.use_stochastic_code) == (True, 0.5, True)
    with pytest.raises(ValueError, match="image_tokens"):   # pre-encoded tokens carry no soft codes
        step(None, torch.zeros(2, dtype=torch.int64), image_tokens=torch.zeros(2, 16, dtype=torch.int64))


def test_soft_target_cross_entropy_refuses_cpu_tensors():
    from muse._hip import MuseHipError
    from muse.training import soft_target_cross_entropy
    logits = torch.randn(2, 5, 12, requires_grad=True)
    labels = torch.full((2, 5), -100, dtype=torch.int64)
    soft = torch.softmax(torch.randn(2, 4, 8), -1)
    with pytest.raises(MuseHipError):
        soft_target_cross_entropy(logits, labels, soft)


def test_prepare_inputs_refuses_soft_codes_for_pre_encoded_tokens():
    import muse
    tokens = torch.zeros(2, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="soft"):
        muse.prepare_inputs_and_labels(None, None, torch.zeros(2, dtype=torch.int64), 47, image_tokens=tokens, codebook_size=32,
                                       use_soft_code_target=True)


def _soft_ce_f64(logits, labels, soft):
    """the reference's soft_target_cross_entropy restated in float64 numpy"""
    x = logits[:, 1:, :soft.shape[-1]].astype(np.float64)
    m = x.max(-1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    rows = -(soft.astype(np.float64) * logp).sum(-1)
    pad = labels[:, 1:] == -100
    rows[pad] = 0.0
    return rows.sum() / (pad.size - pad.sum())


def test_soft_target_golden_is_self_consistent(golden_dir):
    g = np.load(os.path.join(golden_dir, "soft_target_tiny.npz"))
    assert list(g["cases"]) == ["tiny", "a_width"]
    B = int(g["batch"])
    for c in g["cases"]:
        cfg = json.loads(str(g[c + ".config"]))
        S, K, V = cfg["num_vq_tokens"], cfg["codebook_size"], cfg["vocab_size"]
        soft, tokens, labels, ids = g[c + ".soft_targets"], g[c + ".tokens"], g[c + ".labels"], g[c + ".input_ids"]
        assert soft.shape == (B, S, K) and tokens.shape == (B, S) and ids.shape == labels.shape == (B, S + 1)
        assert g[c + ".logits"].shape == (B, S + 1, V)
        np.testing.assert_allclose(soft.sum(-1), 1.0, rtol=1e-5)
        # the recorded mask: masked positions carry the mask id as input and the token as label, the rest -100
        mask = g[c + ".mask"]
        assert mask.any(1).all() and not mask.all()
        assert (ids[:, 1:][mask] == V - 1).all() and (labels[:, 1:][mask] == tokens[mask]).all()
        assert (labels[:, 1:][~mask] == -100).all() and (labels[:, 0] == -100).all()
        assert (ids[:, 0] == g[c + ".class_ids"] + K).all()
        want = _soft_ce_f64(g[c + ".logits"], labels, soft)
        assert abs(want - float(g[c + ".loss"])) <= 1e-6 * abs(want), (c, want, float(g[c + ".loss"]))
    assert float(g["tiny.temp"]) == np.float32(0.7) and float(g["a_width.temp"]) == 1.0
