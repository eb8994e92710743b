"""Golden vectors of the REAL reference (/root/reference, importable only in the build container) TRAINING WITH DROPOUT, for
tests/test_gpu_uvit_dropout.py: the reference's MaskGiTUViT_v2 with hidden_dropout = 0.1 and attention_dropout = 0.2 in train mode, every
nn.Dropout.forward replaced by a multiplication with the Philox keep mask this package draws at that site - tests/philox_cpu.py restates
muse_dropout's stream, the sites' Philox offsets and mask shapes come from the package's own `MaskGiTUViT.dropout_sites` (not re-derived
here), the seed is stored in the file.  With the same masks the two implementations compute the same function, so loss, logits and
gradients are comparable at the tolerances of the p = 0 goldens.

Model: the narrowest U-ViT that reaches every kernel family of the package (head_dim 64, 256 tokens on a 16 x 16 grid, 77 text states,
batch 2).  Output: tests/golden/uvit_dropout.npz + config_uvit_dropout.json.  Re-run:

    python tests/golden/make_golden_uvit_dropout.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import philox_cpu as PH  # noqa: E402
import weights as W  # noqa: E402

torch.set_num_threads(int(os.environ.get("THREADS", "8")))

CONFIG = dict(vocab_size=264, codebook_size=256, hidden_size=128, in_channels=64, block_out_channels=[128], encoder_hidden_size=64,
              cond_embed_dim=32, micro_cond_encode_dim=8, micro_cond_embed_dim=40, num_hidden_layers=2, num_attention_heads=2,
              intermediate_size=256, block_num_heads=2, num_res_blocks=1, hidden_dropout=0.1, attention_dropout=0.2)
BATCH, SEQ, TEXT_LEN, SEED, DROPOUT_SEED = 2, 256, 77, 4100, (0x2BADC0DE << 29) + 12345       # (a 62-bit dropout seed)


def np_(t):
    return t.detach().cpu().numpy()


def package_sites():
    """the package's own numbering of the dropout sites; the package and the reference are both called `muse`, so the package is
    imported first and forgotten again before the reference is"""
    sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
    import muse
    sites = muse.MaskGiTUViT(**CONFIG).dropout_sites(BATCH, SEQ, TEXT_LEN)
    sys.path.remove(os.path.join(ROOT, "open-muse_amd"))
    for name in [n for n in sys.modules if n == "muse" or n.startswith("muse.")]:
        del sys.modules[name]
    return sites


def masked_forward(p, offset, shape):
    """nn.Dropout.forward of one site: x * keep / (1 - p) with the package's mask.  An attention site's mask has the row pitch
    round_up(S_kv, 8); the probabilities it multiplies are [B, heads, S_q, S_kv]."""
    keep = PH.dropout_keep(int(np.prod(shape)), p, DROPOUT_SEED, offset).reshape(shape)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))

    def forward(x):
        k = keep if len(shape) == 2 else keep[:, :, :x.shape[-1]]
        m = torch.from_numpy(np.where(k, scale, np.float32(0.0)).astype(np.float32)).reshape(x.shape)
        return x * m
    return forward


def main():
    sites = package_sites()
    sys.path.insert(0, "/root/reference")
    from muse.modeling_transformer_v2 import MaskGiTUViT_v2
    model = MaskGiTUViT_v2(**CONFIG)
    model.load_state_dict(W.fill_by_shapes({k: tuple(v.shape) for k, v in model.state_dict().items()}, SEED), strict=True)
    ids, enc, cond, micro, labels = W.uvit_inputs(BATCH, SEQ, TEXT_LEN, SEED + 1, CONFIG["vocab_size"], CONFIG["codebook_size"],
                                                  CONFIG["encoder_hidden_size"], CONFIG["cond_embed_dim"])
    model.eval()
    with torch.no_grad():
        plain = model(ids, enc, cond, micro)
    model.train()
    modules = dict(model.named_modules())
    dropouts = [n for n, m in modules.items() if isinstance(m, torch.nn.Dropout)]
    assert sorted(dropouts) == sorted(s[0] for s in sites), (dropouts, [s[0] for s in sites])      # every nn.Dropout is a numbered site
    for name, kind, offset, shape in sites:
        modules[name].forward = masked_forward(CONFIG["hidden_dropout"] if kind == "hidden" else CONFIG["attention_dropout"], offset, shape)
    logits, loss = model(ids, enc, cond, micro, labels=labels)
    loss.backward()
    gap = float((logits.detach() - plain).abs().max() / plain.abs().max())
    assert gap > 5e-2, gap            # the masks matter: a run that ignored them would not pass at the goldens' tolerances
    out = dict(loss=np_(loss), batch=np.int64(BATCH), seq=np.int64(SEQ), text_len=np.int64(TEXT_LEN), seed=np.int64(SEED),
               dropout_seed=np.int64(DROPOUT_SEED), logits=np_(W.subsample(logits, 16384)), logits_absmax=np_(logits.abs().max()),
               logits_norm=np_(logits.double().norm()), logits_shape=np.array(logits.shape, dtype=np.int64), unmasked_gap=np.float64(gap),
               eval_logits=np_(W.subsample(plain, 16384)), eval_logits_absmax=np_(plain.abs().max()))
    for k, p in model.named_parameters():
        g = p.grad.float()
        out["grad." + k] = np_(W.subsample(g, 1024))
        out["absmax." + k] = np_(g.abs().max())
        out["norm." + k] = np_(g.double().norm())
    np.savez_compressed(os.path.join(HERE, "uvit_dropout.npz"), **out)
    with open(os.path.join(HERE, "config_uvit_dropout.json"), "w") as f:
        json.dump(CONFIG, f, indent=1)
    print("uvit_dropout: loss", float(loss), "| masked vs unmasked logits", f"{gap:.2e}", "|", len(sites), "sites,",
          os.path.getsize(os.path.join(HERE, "uvit_dropout.npz")), "bytes")


if __name__ == "__main__":
    main()
