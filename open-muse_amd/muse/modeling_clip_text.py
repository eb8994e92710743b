"""muse.CLIPTextEncoder - the CLIP text tower on the HIP kernels (drop-in for `transformers.CLIPTextModel` /
`CLIPTextModelWithProjection`, the `type: "clip"` text encoder of the reference's configs: training/train_muse.py:331-338 loads it,
:647-649 calls it every step as `text_encoder(ids, return_dict=True, output_hidden_states=True)` and reads `hidden_states[-2]` and
`outputs[0]`).

Frozen and inference-only: there is NO backward, NO CPU compute path (constructing, loading and saving work without a device; `forward`
needs the GPU) and no bf16x3 / f16 compute mode.  Parameter names and shapes are exactly those of `transformers`, masters are float32.

Compute modes (selected like the other classes': `.half()` / `.to(dtype=...)` / `set_compute_dtype`):
  float32  (default)  exact-f32 GEMMs, attention as q k^T -> causal row softmax -> p v on materialised f32 score matrices
  bfloat16            bf16 operands, f32 accumulation, the fused causal attention kernel (no score matrix in memory)
Outputs are float32 in both.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
from torch import nn

from . import ops
from ._tower import TowerMixin, materialised_attention, read_checkpoint, write_checkpoint
from .modeling_utils import FrozenDict, ModelMixin

_DEFAULTS = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12, num_attention_heads=8,
                 max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0, initializer_range=0.02,
                 initializer_factor=1.0, pad_token_id=1, bos_token_id=49406, eos_token_id=49407)


def _key(k):
    """parameter names always carry the `text_model.` prefix of the published checkpoints; newer transformers' CLIPTextModel IS the
    bare tower (its state dict drops the prefix, its checkpoints keep it as `base_model_prefix`): those keys get it back"""
    return k if k.startswith(("text_model.", "text_projection.")) else "text_model." + k


class CLIPTextOutput(OrderedDict):
    """`transformers`' ModelOutput in small: the fields that are set, by attribute, by key and by position.  With a projection the
    order is (text_embeds, last_hidden_state[, hidden_states]) - CLIPTextModelOutput; without (last_hidden_state, pooler_output[,
    hidden_states]) - BaseModelOutputWithPooling.  `pooler_output` is an attribute in both; a field of either class that was not set
    reads as None by attribute, as ModelOutput's does (`out.hidden_states is None` when they were not asked for)."""
    _FIELDS = ("text_embeds", "last_hidden_state", "pooler_output", "hidden_states", "attentions")

    def __getitem__(self, k):
        return self.to_tuple()[k] if isinstance(k, (int, slice)) else super().__getitem__(k)

    def __getattr__(self, name):
        if name == "pooler_output" and "_pooler_output" in self.__dict__:
            return self.__dict__["_pooler_output"]
        try:
            return super().__getitem__(name)
        except KeyError:
            if name in self._FIELDS:
                return None
            raise AttributeError(name) from None

    def to_tuple(self):
        return tuple(self.values())


class _Weight(nn.Module):
    """a `weight` (and `bias`) holder under the transformers module path"""

    def __init__(self, shape, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(shape, dtype=torch.float32))
        if bias:
            self.bias = nn.Parameter(torch.zeros(shape[0], dtype=torch.float32))


class _Attn(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (_Weight((H, H), True) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, H, inter):
        super().__init__()
        self.fc1, self.fc2 = _Weight((inter, H), True), _Weight((H, inter), True)


class _Layer(nn.Module):
    def __init__(self, H, inter):
        super().__init__()
        self.self_attn = _Attn(H)
        self.layer_norm1 = _Weight((H,), True)
        self.mlp = _MLP(H, inter)
        self.layer_norm2 = _Weight((H,), True)


class _Embeddings(nn.Module):
    def __init__(self, vocab, positions, H):
        super().__init__()
        self.token_embedding, self.position_embedding = _Weight((vocab, H), False), _Weight((positions, H), False)


class _Encoder(nn.Module):
    def __init__(self, n, H, inter):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(H, inter) for _ in range(n)])


class _TextModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg["vocab_size"], cfg["max_position_embeddings"], cfg["hidden_size"])
        self.encoder = _Encoder(cfg["num_hidden_layers"], cfg["hidden_size"], cfg["intermediate_size"])
        self.final_layer_norm = _Weight((cfg["hidden_size"],), True)


class CLIPTextEncoder(TowerMixin, ModelMixin):
    _cast_selects_compute_mode = True

    def __init__(self, config=None, **kwargs):
        """`config`: a dict (the `config.json` of a transformers CLIP text model) and / or the same keys as keyword arguments.
        `with_projection` (default: what `architectures` names, else True): carry `text_projection` and return `text_embeds`."""
        super().__init__()
        cfg = dict(config.to_dict() if hasattr(config, "to_dict") else (config or {}))
        cfg.update(kwargs)
        arch = cfg.get("architectures") or []
        with_projection = bool(cfg.pop("with_projection", "CLIPTextModel" not in arch))
        cfg = {**_DEFAULTS, **cfg}
        H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
        if H % nh or H // nh not in (32, 64):
            raise NotImplementedError(f"CLIPTextEncoder: head_dim {H / nh:g} is outside the MI355X hot-path build (the causal attention "
                                      "kernel takes head_dim 32 or 64)")
        if int(cfg["max_position_embeddings"]) > 128:
            raise NotImplementedError(f"CLIPTextEncoder: max_position_embeddings {cfg['max_position_embeddings']} > 128 is outside the "
                                      "MI355X hot-path build (the causal attention kernel keeps the sequence in one tile)")
        if cfg["hidden_act"] not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"CLIPTextEncoder: hidden_act {cfg['hidden_act']!r} is outside the MI355X hot-path build "
                                      "(quick_gelu and gelu have kernels)")
        if float(cfg["attention_dropout"]) != 0.0:
            raise NotImplementedError("CLIPTextEncoder: attention_dropout > 0 is outside the MI355X hot-path build (frozen text encoder)")
        cfg["architectures"] = ["CLIPTextModelWithProjection" if with_projection else "CLIPTextModel"]
        cfg["model_type"] = "clip_text_model"
        self.config = FrozenDict(cfg)
        self.text_model = _TextModel(cfg)
        if with_projection:
            self.text_projection = _Weight((int(cfg["projection_dim"]), H), False)
        self.compute_dtype = torch.float32
        self._packed = {}
        self._init_weights()
        self.requires_grad_(False)
        self.eval()

    def _init_weights(self):
        std = float(self.config.initializer_range)
        for name, p in self.named_parameters():
            if name.endswith("bias"):
                p.data.zero_()
            elif p.dim() == 1:
                p.data.fill_(1.0)
            else:
                nn.init.normal_(p.data, std=std)

    @property
    def with_projection(self):
        return hasattr(self, "text_projection")

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """keys with or without the `text_model.` prefix; tensors become float32 masters (`assign=True` adopts a float32 tensor itself
        instead of copying it, as nn.Module's does)"""
        out = super().load_state_dict({_key(k): v.to(torch.float32) for k, v in state_dict.items()}, strict=strict, assign=assign)
        self._packed.clear()
        return out

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _attention(self, qkv, B, S, nh, hd):
        H = nh * hd
        alpha = float(hd) ** -0.5
        if qkv.dtype == torch.bfloat16:
            return ops.causal_attention_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, S, nh, hd, alpha)
        ld = (S + 3) & ~3       # a k-contiguous f32 operand's rows are padded to 16 bytes; the softmax writes the pad columns as 0
        return materialised_attention(qkv, B, S, nh, hd, alpha=alpha, ld=ld, softmax=lambda scores: ops.causal_softmax_(scores, B * nh, S, ld),
                                      ctx_dtype=torch.float32)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, return_dict=None, output_hidden_states=None):
        if attention_mask is not None or position_ids is not None:
            raise NotImplementedError("CLIPTextEncoder: attention_mask / position_ids are outside the MI355X hot-path build (the reference "
                                      "passes neither: training/train_muse.py:647-649)")
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        cfg, tm, cd = self.config, self.text_model, self.compute_dtype
        ids = input_ids.reshape(-1, input_ids.shape[-1]).to(torch.int64).contiguous()
        ops.require_gpu(ids, tm.final_layer_norm.weight)
        B, S = ids.shape
        H, nh = int(cfg.hidden_size), int(cfg.num_attention_heads)
        hd, eps = H // nh, float(cfg.layer_norm_eps)
        if S > int(cfg.max_position_embeddings):
            raise ValueError(f"sequence length {S} exceeds max_position_embeddings {cfg.max_position_embeddings}")
        quick = cfg.hidden_act == "quick_gelu"
        x = ops.embed_fwd(ids, tm.embeddings.token_embedding.weight.data, tm.embeddings.position_embedding.weight.data)
        hidden = [x]
        for i, lyr in enumerate(tm.encoder.layers):
            att, mlp = lyr.self_attn, lyr.mlp
            h = ops.layernorm_bias_fwd(x, lyr.layer_norm1.weight.data, lyr.layer_norm1.bias.data, eps, cd)
            wqkv, bqkv = self._qkv(i, att)
            ctx = self._attention(ops.linear(h, wqkv, bias=bqkv), B, S, nh, hd)
            x = ops.linear(ctx, self._w((i, "o"), lambda: att.out_proj.weight.data), out_dtype=torch.float32, residual=x,
                           bias=att.out_proj.bias.data)
            h = ops.layernorm_bias_fwd(x, lyr.layer_norm2.weight.data, lyr.layer_norm2.bias.data, eps, cd)
            w1 = self._w((i, "fc1"), lambda: mlp.fc1.weight.data)
            if quick:
                h = ops.bias_quick_gelu_(ops.linear(h, w1), mlp.fc1.bias.data)
            else:
                h = ops.linear(h, w1, bias=mlp.fc1.bias.data, act=1)
            x = ops.linear(h, self._w((i, "fc2"), lambda: mlp.fc2.weight.data), out_dtype=torch.float32, residual=x, bias=mlp.fc2.bias.data)
            hidden.append(x)
        last = ops.layernorm_bias_fwd(x, tm.final_layer_norm.weight.data, tm.final_layer_norm.bias.data, eps, torch.float32)
        _, flat = ops.eos_index(ids, int(cfg.eos_token_id))
        pooled = ops.gather_rows(last, flat, torch.float32)
        out = CLIPTextOutput()
        if self.with_projection:
            wp = self._w("proj", lambda: self.text_projection.weight.data)
            out["text_embeds"] = ops.linear(pooled if cd == torch.float32 else ops.cast_to_bf16(pooled), wp, out_dtype=torch.float32)
            out["last_hidden_state"] = last.view(B, S, H)
            out.__dict__["_pooler_output"] = pooled
        else:
            out["last_hidden_state"] = last.view(B, S, H)
            out["pooler_output"] = pooled
        if output_hidden_states:
            out["hidden_states"] = tuple(t.view(B, S, H) for t in hidden)
        return out if (return_dict is None or return_dict) else out.to_tuple()

    # ---- transformers checkpoints -----------------------------------------------------------------------------------------------------
    @classmethod
    def from_transformers(cls, module):
        """a live transformers CLIPTextModel / CLIPTextModelWithProjection -> CLIPTextEncoder with a copy of its weights"""
        sd = {k: v.detach().to("cpu", torch.float32).clone() for k, v in module.state_dict().items()}
        cfg = {k: v for k, v in module.config.to_dict().items() if k != "architectures"}
        model = cls(cfg, with_projection="text_projection.weight" in sd)
        model.load_state_dict(sd, strict=True)
        return model

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, **config_overrides):
        """a LOCAL transformers directory: config.json + model.safetensors or pytorch_model.bin.  Keyword arguments override config
        entries (`projection_dim=768`, training/train_muse.py:337); one that contradicts the stored `text_projection` raises.  The tower
        carries a projection iff the checkpoint stores one (`with_projection=False` drops it: the reference's CLIPTextModel branch)."""
        torch_dtype = config_overrides.pop("torch_dtype", None)
        want_projection = config_overrides.pop("with_projection", None)     # False = CLIPTextModel of a checkpoint that stores a projection
        path, cfg, sd = read_checkpoint(pretrained_model_name_or_path, subfolder)
        if "text_config" in cfg and "hidden_size" not in cfg:       # a full CLIPModel config: the text tower's part
            cfg = dict(cfg["text_config"], projection_dim=cfg.get("projection_dim", cfg["text_config"].get("projection_dim")))
        if not any(k.startswith(("vision_model.", "visual_projection.", "logit_scale")) for k in sd):
            sd = {_key(k): v for k, v in sd.items()}
        sd = {k: v for k, v in sd.items() if k.startswith("text_model.") and not k.endswith("position_ids") or k == "text_projection.weight"}
        cfg.update(config_overrides)
        if want_projection is False:
            sd.pop("text_projection.weight", None)
        stored = sd.get("text_projection.weight")
        if want_projection and stored is None:
            raise ValueError(f"{path} stores no text_projection.weight")
        if stored is not None and "projection_dim" in config_overrides and int(config_overrides["projection_dim"]) != stored.shape[0]:
            raise ValueError(f"projection_dim={config_overrides['projection_dim']} contradicts the checkpoint's text_projection.weight "
                             f"{tuple(stored.shape)}")
        cfg.pop("architectures", None)
        model = cls(cfg, with_projection=stored is not None)
        model.load_state_dict(sd, strict=True)
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        return model

    def save_pretrained(self, save_directory, **kwargs):
        """config.json + model.safetensors as transformers writes them: `CLIPTextModel[WithProjection].from_pretrained` loads the directory"""
        write_checkpoint(save_directory, self.config, self.state_dict())
