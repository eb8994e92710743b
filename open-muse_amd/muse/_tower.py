"""What the frozen encoder towers (CLIPTextEncoder, T5TextEncoder, CLIPImageEncoder) share: the compute-mode switch and packed-operand
cache, the materialised attention route, and the reader / writer of a local transformers checkpoint directory."""
from __future__ import annotations

import json
import os

import torch

from . import ops


class TowerMixin:
    """in front of ModelMixin in a tower's bases; the tower sets `compute_dtype` and `_packed = {}` in its constructor"""

    def set_compute_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{type(self).__name__} computes in torch.float32 (exact) or torch.bfloat16; there is no bf16x3 / f16 mode")
        self.compute_dtype = dtype
        self._packed.clear()
        return self

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._packed.clear()
        for p in self.parameters():
            if p.dtype != torch.float32:
                raise ops._hip.MuseHipError("master parameters stay float32 (compute precision is selected with set_compute_dtype)")
        return out

    def _w(self, key, make):
        """operand of a product in the compute dtype, built once (dropped when weights are loaded / moved or the mode changes)"""
        hit = self._packed.get(key)
        if hit is None:
            t = make()
            hit = self._packed[key] = ops.cast_to_bf16(t.contiguous()) if self.compute_dtype == torch.bfloat16 else t.contiguous()
        return hit

    def _qkv(self, i, att):
        """q | k | v projections as ONE packed [3H, H] operand and [3H] bias"""
        w = self._w((i, "qkv"), lambda: torch.cat([att.q_proj.weight.data, att.k_proj.weight.data, att.v_proj.weight.data], 0))
        b = self._packed.get((i, "qkv_b"))
        if b is None:
            b = self._packed[(i, "qkv_b")] = torch.cat([att.q_proj.bias.data, att.k_proj.bias.data, att.v_proj.bias.data], 0)
        return w, b


def materialised_attention(qkv, B, S, nh, hd, *, alpha, ld, softmax, ctx_dtype):
    """attention of packed q | k | v rows [B S, 3 nh hd] as q k^T -> softmax -> p v on materialised f32 [B nh, S, ld] score matrices.
    `ld` >= S pads a k-contiguous operand's rows to 16 bytes; `softmax(scores)` returns the probabilities the second product reads
    (the scores in place, or a copy in another dtype) with the pad columns written as 0."""
    H = nh * hd
    scores = torch.empty((B * nh, S, ld), dtype=torch.float32, device=qkv.device)
    ops.gemm(qkv, qkv, scores, S, S, hd, la=0, lb=0, lda=3 * H, ldb=3 * H, ldc=ld, b_off=H, alpha=alpha, batch=B * nh, zdiv=nh,
             sA=(S * 3 * H, hd), sB=(S * 3 * H, hd), sC=(nh * S * ld, S * ld))
    probs = softmax(scores)
    ctx = torch.empty((B * S, H), dtype=ctx_dtype, device=qkv.device)
    ops.gemm(probs, qkv, ctx, S, hd, S, la=0, lb=1, lda=ld, ldb=3 * H, ldc=H, b_off=2 * H, batch=B * nh, zdiv=nh,
             sA=(nh * S * ld, S * ld), sB=(S * 3 * H, hd), sC=(S * H, hd))
    return ctx


def read_checkpoint(pretrained_model_name_or_path, subfolder, refuse_sharded=None):
    """(path, config dict, state dict) of a LOCAL transformers directory: config.json + model.safetensors or pytorch_model.bin.
    `refuse_sharded`: the class name of a tower that refuses a directory with a shard index."""
    path = str(pretrained_model_name_or_path)
    if subfolder:
        path = os.path.join(path, subfolder)
    if not os.path.isfile(os.path.join(path, "config.json")):
        raise EnvironmentError(f"Error no file named config.json found in directory {path}.")
    with open(os.path.join(path, "config.json"), "r", encoding="utf-8") as f:
        cfg = json.load(f)
    if refuse_sharded:
        sharded = [n for n in ("model.safetensors.index.json", "pytorch_model.bin.index.json") if os.path.isfile(os.path.join(path, n))]
        if sharded:
            raise NotImplementedError(f"{refuse_sharded}: {path} holds a sharded checkpoint ({sharded[0]}), which is outside the MI355X "
                                      "hot-path build: save the encoder as one model.safetensors")
    if os.path.isfile(os.path.join(path, "model.safetensors")):
        from safetensors.torch import load_file
        sd = load_file(os.path.join(path, "model.safetensors"))
    elif os.path.isfile(os.path.join(path, "pytorch_model.bin")):
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    else:
        raise EnvironmentError(f"Error no file named model.safetensors or pytorch_model.bin found in directory {path}.")
    return path, cfg, sd


def write_checkpoint(save_directory, config, state_dict):
    """config.json + model.safetensors as transformers writes them"""
    from safetensors.torch import save_file
    os.makedirs(save_directory, exist_ok=True)
    cfg = {k: v for k, v in config.items() if not k.startswith("_") and k != "torch_dtype"}    # the source config's spelling of `dtype`
    cfg["dtype"] = "float32"
    with open(os.path.join(save_directory, "config.json"), "w", encoding="utf-8") as f:
        f.write(json.dumps(cfg, indent=2, sort_keys=True) + "\n")
    save_file({k: v.detach().to("cpu").contiguous().clone() for k, v in state_dict.items()},
              os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
