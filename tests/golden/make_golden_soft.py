"""Golden vectors of the soft-target training step (config.training.use_soft_code_target) from the REAL reference, importable
only in the build container:

    python tests/golden/make_golden_soft.py

For each case: the reference's `MaskGitVQGAN.get_soft_code(pixels, temp)` (soft targets and argmin tokens), the cosine-schedule mask
drawn from recorded uniforms (oracle.prepare_inputs_and_labels, pinned against the reference by mask_*.npz), `logits =
model(input_ids=input_ids)` of the reference's MaskGitTransformer and the training script's own `soft_target_cross_entropy`
(compiled from training/train_maskgit_imagenet.py at generation time) followed by `backward()`.  Output:
tests/golden/soft_target_tiny.npz (committed).
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the reference package on sys.path)
import weights as W  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root, for `oracle`
from oracle import maskgit_oracle as O  # noqa: E402

TRAIN_SCRIPT = "/root/reference/training/train_maskgit_imagenet.py"

# the tiny transformer at config A's width (hidden 512, 8 heads of 64, FFN 2048): its gradients are kept as every k-th element
TRANSFORMER_TINY_A_WIDTH = dict(W.TRANSFORMER_TINY, hidden_size=512, num_attention_heads=8, intermediate_size=2048)

CASES = {   # name: (transformer config, temp, seed, keep whole gradients)
    "tiny": (W.TRANSFORMER_TINY, 0.7, 910, True),
    "a_width": (TRANSFORMER_TINY_A_WIDTH, 1.0, 930, False),
}
BATCH = 4


def soft_target_cross_entropy():
    ns = MG._reference_function(TRAIN_SCRIPT, "soft_target_cross_entropy")
    ns["F"] = F
    return ns["soft_target_cross_entropy"]


def golden_case(out, prefix, tcfg, temp, seed, full_grads, loss_fn):
    vcfg = W.VQGAN_TINY
    vq = MG.ref_muse.MaskGitVQGAN(**vcfg)
    vq.load_state_dict(W.fill_state_dict(W.vqgan_shapes(vcfg), seed, "vqgan"), strict=True)
    vq.eval()
    px = W.images(BATCH, vcfg["resolution"], seed + 1)
    with torch.no_grad():
        soft, tokens = vq.get_soft_code(px, temp=temp, stochastic=False)
    S = tokens.shape[1]
    cls = torch.from_numpy(np.random.default_rng(seed + 2).integers(0, tcfg["num_classes"], size=BATCH))
    t, nz = W.uniforms((BATCH,), seed + 3), W.uniforms((BATCH, S), seed + 4)
    ids, labels, _ = O.prepare_inputs_and_labels(tokens, cls, t, nz, mask_id=tcfg["vocab_size"] - 1,
                                                 codebook_size=vcfg["num_embeddings"])
    model = MG.ref_muse.MaskGitTransformer(**tcfg)
    model.load_state_dict(W.fill_state_dict(W.transformer_shapes(tcfg), seed + 5, "transformer"), strict=True)
    model.train()
    logits = model(input_ids=ids)
    loss = loss_fn(logits, labels, soft)
    loss.backward()
    p = prefix + "."
    out.update({p + "config": np.array(json.dumps(tcfg)), p + "seed": np.int64(seed), p + "temp": np.float32(temp),
                p + "pixel_values": MG.np_(px), p + "soft_targets": MG.np_(soft),
                p + "tokens": MG.np_(tokens), p + "class_ids": MG.np_(cls), p + "timesteps": MG.np_(t), p + "noise": MG.np_(nz),
                p + "mask": MG.np_(ids[:, 1:] == tcfg["vocab_size"] - 1), p + "input_ids": MG.np_(ids), p + "labels": MG.np_(labels),
                p + "logits": MG.np_(logits), p + "loss": MG.np_(loss), p + "full_grads": np.bool_(full_grads)})
    for k, prm in model.named_parameters():
        g = prm.grad.float()
        out[p + "grad." + k] = MG.np_(g if full_grads else W.subsample(g, 1024))
        out[p + "absmax." + k] = MG.np_(g.abs().max())
    print(prefix, "temp", temp, "loss", float(loss.detach()), "masked per image", (ids[:, 1:] == tcfg["vocab_size"] - 1).sum(-1).tolist())


def main():
    torch.set_num_threads(1)
    fn = soft_target_cross_entropy()
    out = dict(batch=np.int64(BATCH), cases=np.array(list(CASES)))
    for name, (tcfg, temp, seed, full) in CASES.items():
        golden_case(out, name, tcfg, temp, seed, full, fn)
    path = os.path.join(HERE, "soft_target_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
