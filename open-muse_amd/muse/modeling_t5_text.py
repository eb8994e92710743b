"""muse.T5TextEncoder - the T5 v1.1 encoder on the HIP kernels (drop-in for `transformers.T5EncoderModel`, the `type: "t5"` text
encoder of the reference's configs: training/train_muse.py:341-343 loads it, :651 calls it every step as `text_encoder(ids)[0]`;
muse/pipeline_muse.py:133,154 reads `.last_hidden_state`).

Frozen and inference-only: there is NO backward, NO CPU compute path (constructing, loading and saving work without a device; `forward`
needs the GPU) and no bf16x3 / f16 compute mode.  Parameter names and shapes are exactly those of `transformers`, masters are float32;
`shared.weight` and `encoder.embed_tokens.weight` are one tensor under two names.

T5's attention has no 1 / sqrt(d) scale and no mask; its scores get a relative-position bias that layer 0 owns and every layer adds:
`relative_attention_bias.weight[bucket(j - i)][head]`, bucket = T5's bidirectional bucketing of the signed distance (`rel_buckets`).
The bias depends on the sequence length and the weights only: it is built once per length as an f32 [heads, 2 S - 1] tensor (one value
per head and signed distance, never an S x S matrix) and kept with the packed operands.

Compute modes (selected like the other classes': `.half()` / `.to(dtype=...)` / `set_compute_dtype`):
  float32  (default)  exact-f32 GEMMs, attention as q k^T -> bias + row softmax -> p v on materialised f32 score matrices
  bfloat16            bf16 operands, f32 accumulation; S <= 128: the fused bias attention kernel (no score matrix in memory);
                      128 < S <= 512: bf16 products around the same bias + softmax kernel
Outputs are float32 in both.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch import nn

from . import ops
from ._tower import TowerMixin, materialised_attention, read_checkpoint, write_checkpoint
from .modeling_utils import FrozenDict, ModelMixin

_DEFAULTS = dict(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_heads=8, relative_attention_num_buckets=32,
                 relative_attention_max_distance=128, dropout_rate=0.1, layer_norm_epsilon=1e-6, initializer_factor=1.0,
                 feed_forward_proj="gated-gelu", pad_token_id=0, eos_token_id=1)
MAX_SEQ = 512         # the T5 tokenizer's model_max_length, which PipelineMuse pads to
FUSED_MAX_SEQ = 128   # the fused attention kernel keeps the sequence in one tile


def rel_buckets(seq, num_buckets, max_distance):
    """int64 [2 seq - 1]: the bucket of every signed distance d = j - i (key minus query) in -(seq - 1) .. seq - 1, T5's bidirectional
    bucketing.  Half of the buckets go to each sign (d > 0: the upper half); within a half the first half are the exact distances
    |d| < max_exact, the rest grow logarithmically up to max_distance (everything beyond shares the last bucket).  float32 arithmetic,
    on the host."""
    d = torch.arange(-(seq - 1), seq, dtype=torch.int64)
    half = num_buckets // 2
    max_exact = half // 2
    n = d.abs()
    log_pos = torch.log(n.clamp(min=1).to(torch.float32) / max_exact) / math.log(max_distance / max_exact) * (half - max_exact)
    large = torch.clamp(max_exact + log_pos.to(torch.int64), max=half - 1)
    return (d > 0).to(torch.int64) * half + torch.where(n < max_exact, n, large)


class T5TextOutput(OrderedDict):
    """`transformers`' BaseModelOutput in small: the fields that are set, by attribute, by key and by position
    (last_hidden_state[, hidden_states]); a field that was not set reads as None by attribute, as ModelOutput's does."""
    _FIELDS = ("last_hidden_state", "hidden_states", "attentions")

    def __getitem__(self, k):
        return self.to_tuple()[k] if isinstance(k, (int, slice)) else super().__getitem__(k)

    def __getattr__(self, name):
        try:
            return super().__getitem__(name)
        except KeyError:
            if name in self._FIELDS:
                return None
            raise AttributeError(name) from None

    def to_tuple(self):
        return tuple(self.values())


class _Weight(nn.Module):
    """a `weight` holder under the transformers module path"""

    def __init__(self, shape):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(shape, dtype=torch.float32))


class _SelfAttention(nn.Module):
    def __init__(self, d_model, inner, rel_shape):
        super().__init__()
        self.q, self.k, self.v, self.o = _Weight((inner, d_model)), _Weight((inner, d_model)), _Weight((inner, d_model)), _Weight((d_model, inner))
        if rel_shape is not None:
            self.relative_attention_bias = _Weight(rel_shape)


class _AttnLayer(nn.Module):
    def __init__(self, d_model, inner, rel_shape):
        super().__init__()
        self.SelfAttention = _SelfAttention(d_model, inner, rel_shape)
        self.layer_norm = _Weight((d_model,))


class _Dense(nn.Module):
    def __init__(self, d_model, d_ff):
        super().__init__()
        self.wi_0, self.wi_1, self.wo = _Weight((d_ff, d_model)), _Weight((d_ff, d_model)), _Weight((d_model, d_ff))


class _FFLayer(nn.Module):
    def __init__(self, d_model, d_ff):
        super().__init__()
        self.DenseReluDense = _Dense(d_model, d_ff)
        self.layer_norm = _Weight((d_model,))


class _Block(nn.Module):
    def __init__(self, d_model, inner, d_ff, rel_shape):
        super().__init__()
        self.layer = nn.ModuleList([_AttnLayer(d_model, inner, rel_shape), _FFLayer(d_model, d_ff)])


class _Stack(nn.Module):
    def __init__(self, cfg, shared):
        super().__init__()
        d_model, nh = cfg["d_model"], cfg["num_heads"]
        self.embed_tokens = shared
        self.block = nn.ModuleList([_Block(d_model, nh * cfg["d_kv"], cfg["d_ff"], (cfg["relative_attention_num_buckets"], nh) if i == 0 else None)
                                    for i in range(cfg["num_layers"])])
        self.final_layer_norm = _Weight((d_model,))


_EMBED_KEYS = ("shared.weight", "encoder.embed_tokens.weight")


class T5TextEncoder(TowerMixin, ModelMixin):
    _cast_selects_compute_mode = True

    def __init__(self, config=None, **kwargs):
        """`config`: a dict (the `config.json` of a transformers T5 model) and / or the same keys as keyword arguments"""
        super().__init__()
        cfg = dict(config.to_dict() if hasattr(config, "to_dict") else (config or {}))
        cfg.update(kwargs)
        cfg = {**_DEFAULTS, **cfg}
        for k in ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets", "relative_attention_max_distance"):
            cfg[k] = int(cfg[k])
        if cfg["feed_forward_proj"] != "gated-gelu":
            raise NotImplementedError(f"T5TextEncoder: feed_forward_proj {cfg['feed_forward_proj']!r} is outside the MI355X hot-path build "
                                      "(T5 v1.1's gated-gelu has a kernel; the original T5's relu does not)")
        if cfg["d_kv"] not in (32, 64):
            raise NotImplementedError(f"T5TextEncoder: d_kv {cfg['d_kv']} is outside the MI355X hot-path build (the bias attention kernel "
                                      "takes head_dim 32 or 64)")
        if cfg["d_model"] % 8 or cfg["d_ff"] % 8:
            raise NotImplementedError(f"T5TextEncoder: d_model {cfg['d_model']} / d_ff {cfg['d_ff']} are outside the MI355X hot-path build "
                                      "(GEMM operand rows are multiples of 16 bytes)")
        if cfg["relative_attention_num_buckets"] < 4 or cfg["relative_attention_num_buckets"] % 2:
            raise NotImplementedError("T5TextEncoder: relative_attention_num_buckets must be even and >= 4")
        cfg["architectures"] = ["T5EncoderModel"]
        cfg["model_type"] = "t5"
        self.config = FrozenDict(cfg)
        self.shared = _Weight((cfg["vocab_size"], cfg["d_model"]))
        self.encoder = _Stack(cfg, self.shared)
        self.compute_dtype = torch.float32
        self._packed = {}
        self._init_weights()
        self.requires_grad_(False)
        self.eval()

    def _init_weights(self):
        f, d_model = float(self.config.initializer_factor), int(self.config.d_model)
        for name, p in self.named_parameters():
            if p.dim() == 1:
                p.data.fill_(f)
            elif name.endswith((".q.weight",)):
                nn.init.normal_(p.data, std=f * (d_model * int(self.config.d_kv)) ** -0.5)
            elif name == "shared.weight":
                nn.init.normal_(p.data, std=f)
            else:
                nn.init.normal_(p.data, std=f * p.shape[1] ** -0.5)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """the token embedding under either of its two names or both; tensors become float32 masters (`assign=True` adopts a float32
        tensor itself instead of copying it, as nn.Module's does)"""
        sd = {k: v.to(torch.float32) for k, v in state_dict.items()}
        have = [k for k in _EMBED_KEYS if k in sd]
        if len(have) == 2 and not torch.equal(sd[have[0]], sd[have[1]]):
            raise ValueError("shared.weight and encoder.embed_tokens.weight are one tensor in T5; the state dict holds two different ones")
        for k in _EMBED_KEYS:
            if have and k not in sd:
                sd[k] = sd[have[0]]
        if len(have) == 2:
            sd[have[1]] = sd[have[0]]
        out = super().load_state_dict(sd, strict=strict, assign=assign)
        self._packed.clear()
        return out

    def _rel(self, S):
        """f32 [heads, 2 S - 1]: the bias of every head at every signed distance, gathered on the device from layer 0's table"""
        hit = self._packed.get(("rel", S))
        if hit is None:
            cfg = self.config
            table = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.data
            bucket = rel_buckets(S, int(cfg.relative_attention_num_buckets), int(cfg.relative_attention_max_distance)).to(table.device)
            hit = self._packed[("rel", S)] = ops.rel_bias_gather(table.contiguous(), bucket)
        return hit

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _attention(self, qkv, rel, B, S, nh, hd):
        H = nh * hd
        bf16 = qkv.dtype == torch.bfloat16
        if bf16 and S <= FUSED_MAX_SEQ:
            return ops.bias_attention_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], rel, B, S, nh, hd)
        # a k-contiguous operand's rows are padded to 16 bytes; the softmax writes the pad columns as 0
        ld = (S + 7) & ~7 if bf16 else (S + 3) & ~3
        return materialised_attention(qkv, B, S, nh, hd, alpha=1.0, ld=ld, ctx_dtype=qkv.dtype,
                                      softmax=lambda scores: ops.bias_softmax_(scores, rel, B * nh, nh, S, ld, bf16_copy=bf16))

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, return_dict=None, output_hidden_states=None):
        if attention_mask is not None:
            raise NotImplementedError("T5TextEncoder: attention_mask is outside the MI355X hot-path build (the reference passes none: "
                                      "training/train_muse.py:651, muse/pipeline_muse.py:133)")
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        cfg, enc, cd = self.config, self.encoder, self.compute_dtype
        ids = input_ids.reshape(-1, input_ids.shape[-1]).to(torch.int64).contiguous()
        B, S = ids.shape
        if S > MAX_SEQ:
            raise ValueError(f"sequence length {S} exceeds {MAX_SEQ}, the longest the T5 text encoder of this build takes")
        ops.require_gpu(ids, enc.final_layer_norm.weight)
        D, nh, hd, eps = int(cfg.d_model), int(cfg.num_heads), int(cfg.d_kv), float(cfg.layer_norm_epsilon)
        rel = self._rel(S)
        x = ops.gather_rows(self.shared.weight.data, ids.view(-1), torch.float32)
        hidden = []
        for i, blk in enumerate(enc.block):
            hidden.append(x)
            att, ff = blk.layer[0].SelfAttention, blk.layer[1].DenseReluDense
            h = ops.rmsnorm_fwd(x, blk.layer[0].layer_norm.weight.data, eps, cd)
            wqkv = self._w((i, "qkv"), lambda: torch.cat([att.q.weight.data, att.k.weight.data, att.v.weight.data], 0))
            ctx = self._attention(ops.linear(h, wqkv), rel, B, S, nh, hd)
            x = ops.linear(ctx, self._w((i, "o"), lambda: att.o.weight.data), out_dtype=torch.float32, residual=x)
            h = ops.rmsnorm_fwd(x, blk.layer[1].layer_norm.weight.data, eps, cd)
            g = ops.gated_gelu_tanh(ops.linear(h, self._w((i, "wi"), lambda: torch.cat([ff.wi_0.weight.data, ff.wi_1.weight.data], 0))))
            x = ops.linear(g, self._w((i, "wo"), lambda: ff.wo.weight.data), out_dtype=torch.float32, residual=x)
        last = ops.rmsnorm_fwd(x, enc.final_layer_norm.weight.data, eps, torch.float32).view(B, S, D)
        out = T5TextOutput(last_hidden_state=last)
        if output_hidden_states:
            out["hidden_states"] = tuple(t.view(B, S, D) for t in hidden) + (last,)
        return out if (return_dict is None or return_dict) else out.to_tuple()

    # ---- transformers checkpoints -----------------------------------------------------------------------------------------------------
    @classmethod
    def from_transformers(cls, module):
        """a live transformers T5EncoderModel -> T5TextEncoder with a copy of its weights"""
        sd = {k: v.detach().to("cpu", torch.float32).clone() for k, v in module.state_dict().items()}
        model = cls({k: v for k, v in module.config.to_dict().items() if k != "architectures"})
        model.load_state_dict(sd, strict=True)
        return model

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, torch_dtype=None, **config_overrides):
        """a LOCAL transformers directory: config.json + model.safetensors or pytorch_model.bin (one file: sharded checkpoints are
        refused).  A full T5 checkpoint's decoder and lm_head are dropped.  Keyword arguments override config entries."""
        _, cfg, sd = read_checkpoint(pretrained_model_name_or_path, subfolder, refuse_sharded=cls.__name__)
        sd = {k: v for k, v in sd.items() if k.startswith("encoder.") or k == "shared.weight"}
        cfg.update(config_overrides)
        cfg.pop("architectures", None)
        model = cls(cfg)
        model.load_state_dict(sd, strict=True)
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        return model

    def save_pretrained(self, save_directory, **kwargs):
        """config.json + model.safetensors as transformers writes them: `T5EncoderModel.from_pretrained` loads the directory"""
        # one tensor under two names: safetensors stores it once, under the name transformers keeps (`shared.weight`)
        write_checkpoint(save_directory, self.config, {k: v for k, v in self.state_dict().items() if k != "encoder.embed_tokens.weight"})
