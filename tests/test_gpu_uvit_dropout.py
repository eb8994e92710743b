"""muse.MaskGiTUViT training with hidden_dropout / attention_dropout > 0, on the GPU, in all four compute modes.

The golden (tests/golden/uvit_dropout.npz, make_golden_uvit_dropout.py) is the REAL reference with every nn.Dropout replaced by the
Philox mask this package draws at that site for the stored seed: with `_next_dropout_seed` pinned to it both compute the same function,
so loss, logits and every gradient are held to the per-mode tolerances of test_gpu_uvit.test_uvit_config4_vs_reference_golden:

    mode          logits   loss    gradients
    f32, bf16x3   1e-3     1e-4    2e-3
    f16           2e-3     1e-4    6e-3
    bf16          5e-2     2e-3    1.5e-1

(the masks add exact zeros and one f32 multiplication per kept element before the same roundings; the unmasked run sits 0.60 of the
largest logit away).  Model: the narrowest U-ViT that reaches every kernel family (2 heads of 64, 256 tokens, 77 text states, batch 2)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [torch.float32, "bf16x3", "f16", torch.bfloat16]
from uvit_routes_cpu import TOL      # noqa: E402  (the per-mode table above; tests/test_gpu_uvit_routes.py holds its cases to the same one)


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "uvit_dropout.npz"))
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_dropout.json")))
    return g, cfg


def _model(cfg, seed, mode, **over):
    import muse
    import weights as W
    model = muse.MaskGiTUViT(**dict(cfg, **over))
    model.load_state_dict(W.fill_by_shapes({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed), strict=True)
    return model.to(DEV).train().set_compute_dtype(mode)


def _inputs(g, cfg, seq=None, batch=None):
    import weights as W
    return tuple(t.to(DEV) for t in W.uvit_inputs(int(g["batch"]) if batch is None else batch, int(g["seq"]) if seq is None else seq,
                                                  int(g["text_len"]), int(g["seed"]) + 1, cfg["vocab_size"], cfg["codebook_size"],
                                                  cfg["encoder_hidden_size"], cfg["cond_embed_dim"]))


class _Counts:
    """counts the calls of ops functions that carry a dropout argument (and the ones that must not run)"""

    def __init__(self, ops):
        self.ops, self.n, self.saved = ops, {}, {}

    def __enter__(self):
        ops = self.ops

        def wrap(name, dropped):
            inner = self.saved[name] = getattr(ops, name)

            def f(*a, **k):
                key = name + ("+drop" if dropped(a, k) else "")
                self.n[key] = self.n.get(key, 0) + 1
                return inner(*a, **k)
            setattr(ops, name, f)
        for name in ("glu_fwd", "glu_bwd", "grn_fwd", "grn_bwd", "attention_fwd_ex", "attention_bwd_ex", "attention_x3_fwd", "attention_x3_bwd"):
            wrap(name, lambda a, k: k.get("drop") is not None)
        wrap("dropout", lambda a, k: False)
        return self

    def __exit__(self, *exc):
        for name, inner in self.saved.items():
            setattr(self.ops, name, inner)
        return False

    def __getitem__(self, key):
        return self.n.get(key, 0)


@pytest.mark.parametrize("mode", MODES, ids=str)
def test_uvit_dropout_vs_reference_golden_with_the_same_masks(golden_dir, mode):
    import weights as W
    from muse import ops
    g, cfg = _golden(golden_dir)
    model = _model(cfg, int(g["seed"]), mode)
    ids, enc, cond, micro, labels = _inputs(g, cfg)
    sites = model.dropout_sites(int(g["batch"]), int(g["seq"]), int(g["text_len"]))
    n_hidden_res = sum(1 for s in sites if s[1] == "hidden" and ".channelwise." in s[0])
    n_hidden_ffn = sum(1 for s in sites if s[1] == "hidden" and ".ffn." in s[0])
    n_att = sum(1 for s in sites if s[1] == "attention")
    model._next_dropout_seed = int(g["dropout_seed"])
    with _Counts(ops) as n:
        logits, loss = model(ids, enc, cond, micro, labels=labels)
        loss.backward()
    assert model._last_dropout == (int(g["dropout_seed"]), cfg["hidden_dropout"], cfg["attention_dropout"])
    assert not hasattr(model, "_next_dropout_seed")                     # the hook is consumed by the forward it pinned
    # the hidden sites ran inside the row kernels in every mode: no stand-alone pass over a hidden activation
    assert n["glu_fwd+drop"] == n["glu_bwd+drop"] == n_hidden_ffn and n["glu_fwd"] == n["glu_bwd"] == 0
    assert n["grn_fwd+drop"] == n["grn_bwd+drop"] == n_hidden_res and n["grn_fwd"] == n["grn_bwd"] == 0
    if mode == torch.bfloat16:        # the fused kernels of csrc/attention.hip draw the masks themselves
        assert n["attention_fwd_ex+drop"] == n["attention_bwd_ex+drop"] == n_att and n["attention_fwd_ex"] == 0 and n["dropout"] == 0
    elif mode == torch.float32:       # parity mode, the reference's algorithm: one muse_dropout over P, one over dP per attention site
        assert n["dropout"] == 2 * n_att and n["attention_x3_fwd"] == n["attention_x3_fwd+drop"] == 0 and n["attention_fwd_ex+drop"] == 0
    else:                             # bf16x3 / f16: the DROP kernels of csrc/attention3.hip, no materialised probabilities
        assert n["attention_x3_fwd+drop"] == n["attention_x3_bwd+drop"] == n_att and n["attention_x3_fwd"] == n["attention_x3_bwd"] == 0
        assert n["dropout"] == 0
    tl, tloss, tg = TOL[mode]
    assert tuple(logits.shape) == tuple(g["logits_shape"])
    el = float(np.abs(W.subsample(logits.detach().float(), 16384).cpu().numpy() - g["logits"]).max()) / float(g["logits_absmax"])
    lrel = abs(float(loss) - float(g["loss"])) / float(g["loss"])
    errs, nerrs = {}, {}
    for k, p in model.named_parameters():
        gr = p.grad.detach().float()
        errs[k] = float(np.abs(W.subsample(gr, 1024).cpu().numpy() - g["grad." + k]).max()) / float(g["absmax." + k])
        nerrs[k] = abs(float(gr.double().norm()) - float(g["norm." + k])) / float(g["norm." + k])
    worst = max(errs, key=errs.get)
    print(mode, "dropout golden: logits", f"{el:.2e}", "loss", f"{lrel:.1e}", "worst grad", f"{errs[worst]:.1e}", f"({worst})",
          "worst grad norm", f"{max(nerrs.values()):.1e}", "| unmasked run:", f"{float(g['unmasked_gap']):.2e}")
    assert el < tl, (mode, el)
    assert lrel < tloss, (mode, lrel)
    assert errs[worst] < tg, (mode, worst, errs[worst])


def test_a_fresh_seed_per_forward_and_the_hook_pins_it(golden_dir):
    g, cfg = _golden(golden_dir)
    model = _model(cfg, int(g["seed"]), torch.float32)
    ids, enc, cond, micro, labels = _inputs(g, cfg)
    with torch.no_grad():
        a = model(ids, enc, cond, micro)                    # active in train mode with or without labels, like nn.Dropout
        sa = model._last_dropout
        b = model(ids, enc, cond, micro)
        sb = model._last_dropout
        assert sa[0] != sb[0] and 0 <= sa[0] < 2 ** 62 and sa[1:] == sb[1:] == (cfg["hidden_dropout"], cfg["attention_dropout"])
        assert not torch.equal(a, b)
        model._next_dropout_seed = sa[0]
        c = model(ids, enc, cond, micro)
        assert model._last_dropout == sa and torch.equal(a, c)


@pytest.mark.parametrize("mode", MODES, ids=str)
def test_eval_is_dropout_free_and_p0_calls_what_it_called(golden_dir, mode):
    """eval(): the logits of the same weights with p = 0 in the config, bit for bit - no dropped entry point runs.  A p = 0 model in
    train mode launches the same entry points in the same order (none of them a dropout one)."""
    from muse import ops
    g, cfg = _golden(golden_dir)
    ids, enc, cond, micro, labels = _inputs(g, cfg)
    real = ops.lib()

    class Recorder:
        def __init__(self):
            self.names = []

        def __getattr__(self, name):
            self.names.append(name)
            return getattr(real, name)

    def recorded(fn):
        rec, inner = Recorder(), ops.lib
        ops.lib = lambda: rec
        try:
            out = fn()
        finally:
            ops.lib = inner
        return out, rec.names
    dropped = _model(cfg, int(g["seed"]), mode).eval()
    plain = _model(cfg, int(g["seed"]), mode, hidden_dropout=0.0, attention_dropout=0.0)
    with torch.no_grad():
        le, names_e = recorded(lambda: dropped(ids, enc, cond, micro))
        assert dropped._last_dropout == (0, 0.0, 0.0)
        lp, names_p = recorded(lambda: plain(ids, enc, cond, micro))           # train mode, p = 0
    assert torch.equal(le, lp)
    import weights as W
    e0 = float(np.abs(W.subsample(le.float(), 16384).cpu().numpy() - g["eval_logits"]).max()) / float(g["eval_logits_absmax"])
    print(mode, "eval logits vs the reference in eval mode:", f"{e0:.2e}")
    assert e0 < TOL[mode][0], (mode, e0)
    assert names_e == names_p and not any("drop" in n for n in names_p)

    def step(m):
        m.mark_weights_changed()                 # (both models start their step without cached weight copies: the same casts)
        m.zero_grad(set_to_none=True)
        _, loss = m(ids, enc, cond, micro, labels=labels)
        loss.backward()
        return loss
    (_, names_t) = recorded(lambda: step(plain))
    (_, names_d) = recorded(lambda: step(dropped.train()))
    assert not any("drop" in n for n in names_t) and any("drop" in n for n in names_d)
    strip = lambda names: [n.replace("_drop", "") for n in names if n != "muse_dropout"]      # noqa: E731
    if mode == torch.bfloat16:       # the same launches, each dropout site in its kernel's dropped form
        assert strip(names_d) == names_t


def test_fused_and_materialised_attention_dropout_agree_at_1024_tokens(golden_dir, monkeypatch):
    """32 x 32 grid (1024 tokens, batch 1, the narrow widths), bf16x3: the block-by-block DROP route (1024 x 77 per query block, 1024 x
    1024 as block pairs with global q0 / k0) against MUSE_X3_ATTN_DROPOUT_FUSED=0 (materialised) with the same seed, held to the bf16x3
    tolerances above"""
    from muse import ops
    g, cfg = _golden(golden_dir)
    model = _model(cfg, int(g["seed"]), "bf16x3")
    ids, enc, cond, micro, labels = _inputs(g, cfg, seq=1024, batch=1)
    runs = []
    for env in ("1", "0"):
        monkeypatch.setenv("MUSE_X3_ATTN_DROPOUT_FUSED", env)
        model.zero_grad(set_to_none=True)
        model._next_dropout_seed = 4242
        with _Counts(ops) as n:
            logits, loss = model(ids, enc, cond, micro, labels=labels)
            loss.backward()
        assert (n["attention_x3_fwd+drop"] > 0) == (env == "1") and (n["dropout"] > 0) == (env == "0")
        runs.append((logits.detach().double(), float(loss.detach()), {k: p.grad.detach().double() for k, p in model.named_parameters()}))
    (la, sa, ga), (lb, sb, gb) = runs
    tl, tloss, tg = TOL["bf16x3"]
    el = float((la - lb).abs().max() / lb.abs().max())
    eg = max(float((ga[k] - gb[k]).abs().max() / (gb[k].abs().max() + 1e-30)) for k in ga)
    print("1024 tokens, fused vs materialised: logits", f"{el:.2e}", "loss", f"{abs(sa - sb) / abs(sb):.1e}", "worst grad", f"{eg:.1e}")
    assert el < tl and abs(sa - sb) < tloss * abs(sb) and eg < tg
