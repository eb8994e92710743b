"""muse.CLIPImageEncoder / muse.CLIPScorer / muse.clip_scores - the CLIP image tower and the image / text similarity on the HIP kernels
(drop-in for `transformers.CLIPVisionModelWithProjection` and for `CLIPModel(...).logits_per_image`: the reference scores every generated
image against its caption with it, scripts/gen_sdxl_synthetic_dataset.py:34-36,98-105, and reports "CLIP Score" as its quality metric,
benchmark/model_quality.py:32-111).

Frozen and inference-only: there is NO backward and NO CPU compute path (constructing, loading and saving work without a device; `forward`
needs the GPU).  Parameter names and shapes are exactly those of `transformers` (`pre_layrnorm` is upstream's spelling), plus the scalar
`logit_scale` of CLIPModel (ln(1 / 0.07) when a checkpoint has none); masters are float32.

Compute modes (selected like the other classes': `.to(dtype=...)` / `set_compute_dtype`):
  float32  (default)  exact-f32 GEMMs, attention as q k^T -> row softmax -> p v on materialised f32 score matrices
  bfloat16            bf16 operands, f32 accumulation, the fused attention kernel once per layer (no score matrix in memory); residual
                      stream, LayerNorm statistics and the embeddings stay f32
Outputs are float32 in both.

Preprocessing.  `CLIPScorer` takes [B, 3, R, R] f32 images in [0, 1] and resizes them ON THE GPU in f32: antialiased bicubic after ATen's
definition (`F.interpolate(mode="bicubic", antialias=True)`), unclamped, normalised in the same pass.  Upstream's `CLIPImageProcessor`
resizes with PIL on uint8 and rounds to 8 bits between the two passes and after them, so the two pipelines differ by about one quantisation
step per pixel; what that does to `logits_per_image` is measured in DESIGN.md (section 5h).  PIL's 8-bit bicubic is not reproduced.
"""
from __future__ import annotations

import json
import math
import os

import torch
from torch import nn

from . import ops
from ._tower import TowerMixin, materialised_attention, read_checkpoint, write_checkpoint
from .modeling_clip_text import CLIPTextOutput, _Encoder, _Weight
from .modeling_utils import FrozenDict, ModelMixin

_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=12, num_attention_heads=12, num_channels=3,
                 image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0, initializer_range=0.02,
                 initializer_factor=1.0)
CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_TOKENS = 577        # ViT-L/14@336: the longest published tower with head_dim 64
_OWN = ("vision_model.", "visual_projection.", "logit_scale")


def _key(k):
    """parameter names always carry the `vision_model.` prefix of the published checkpoints; a bare tower's keys get it back"""
    return k if k.startswith(_OWN) else "vision_model." + k


class CLIPVisionOutput(CLIPTextOutput):
    """`transformers`' CLIPVisionModelOutput in small: (image_embeds, last_hidden_state[, hidden_states]) by attribute, key and position;
    `pooler_output` is an attribute; a field that was not set reads as None"""
    _FIELDS = ("image_embeds", "last_hidden_state", "pooler_output", "hidden_states", "attentions")


class _VisionEmbeddings(nn.Module):
    def __init__(self, H, P, positions):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.empty(H, dtype=torch.float32))
        self.patch_embedding = _Weight((H, 3, P, P), False)
        self.position_embedding = _Weight((positions, H), False)


class _VisionModel(nn.Module):
    def __init__(self, cfg, positions):
        super().__init__()
        H = cfg["hidden_size"]
        self.embeddings = _VisionEmbeddings(H, cfg["patch_size"], positions)
        self.pre_layrnorm = _Weight((H,), True)
        self.encoder = _Encoder(cfg["num_hidden_layers"], H, cfg["intermediate_size"])
        self.post_layernorm = _Weight((H,), True)


class CLIPImageEncoder(TowerMixin, ModelMixin):
    _cast_selects_compute_mode = True

    def __init__(self, config=None, **kwargs):
        """`config`: a dict (the `config.json` of a transformers CLIP vision model, or a CLIPVisionConfig) and / or the same keys as
        keyword arguments.  `image_mean` / `image_std` (three floats each; default CLIP's) are what `CLIPScorer` normalises with."""
        super().__init__()
        cfg = dict(config.to_dict() if hasattr(config, "to_dict") else (config or {}))
        cfg.update(kwargs)
        self.image_mean = tuple(float(v) for v in cfg.pop("image_mean", None) or CLIP_IMAGE_MEAN)
        self.image_std = tuple(float(v) for v in cfg.pop("image_std", None) or CLIP_IMAGE_STD)
        cfg = {**_DEFAULTS, **cfg}
        H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
        I, P = int(cfg["image_size"]), int(cfg["patch_size"])
        if H % nh or H // nh not in (32, 64):
            raise NotImplementedError(f"CLIPImageEncoder: head_dim {H / nh:g} is outside the MI355X hot-path build (the towers built here "
                                      "have head_dim 32 or 64; ViT-H / bigG are not)")
        if H > 2048:
            raise NotImplementedError(f"CLIPImageEncoder: hidden_size {H} > 2048 is outside the MI355X hot-path build (the embedding kernel "
                                      "keeps a row in registers)")
        if cfg["hidden_act"] not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"CLIPImageEncoder: hidden_act {cfg['hidden_act']!r} is outside the MI355X hot-path build "
                                      "(quick_gelu and gelu have kernels)")
        if float(cfg["attention_dropout"]) != 0.0:
            raise NotImplementedError("CLIPImageEncoder: attention_dropout > 0 is outside the MI355X hot-path build (frozen image encoder)")
        if int(cfg["num_channels"]) != 3:
            raise NotImplementedError(f"CLIPImageEncoder: num_channels {cfg['num_channels']} is outside the MI355X hot-path build (RGB images)")
        if P < 1 or I < P or I % P:
            raise NotImplementedError(f"CLIPImageEncoder: image_size {I} is no multiple of patch_size {P}, which is outside the MI355X "
                                      "hot-path build (upstream's convolution would drop the border)")
        tokens = (I // P) ** 2 + 1
        if tokens > MAX_TOKENS:
            raise NotImplementedError(f"CLIPImageEncoder: {tokens} tokens > {MAX_TOKENS} is outside the MI355X hot-path build (the exact-f32 "
                                      "mode materialises tokens x tokens score matrices)")
        cfg["architectures"] = ["CLIPVisionModelWithProjection"]
        cfg["model_type"] = "clip_vision_model"
        self.config = FrozenDict(cfg)
        self.vision_model = _VisionModel(cfg, tokens)
        self.visual_projection = _Weight((int(cfg["projection_dim"]), H), False)
        self.logit_scale = nn.Parameter(torch.tensor(math.log(1.0 / 0.07), dtype=torch.float32))
        self.compute_dtype = torch.float32
        self._packed = {}
        self._init_weights()
        self.requires_grad_(False)
        self.eval()

    def _init_weights(self):
        std = float(self.config.initializer_range)
        for name, p in self.named_parameters():
            if name == "logit_scale":
                continue
            if name.endswith("bias"):
                p.data.zero_()
            elif p.dim() == 1 and not name.endswith("class_embedding"):
                p.data.fill_(1.0)
            else:
                nn.init.normal_(p.data, std=std)

    @property
    def tokens(self):
        return (int(self.config.image_size) // int(self.config.patch_size)) ** 2 + 1

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """keys with or without the `vision_model.` prefix; a missing `logit_scale` keeps ln(1 / 0.07); tensors become float32 masters"""
        sd = {_key(k): v.to(torch.float32) for k, v in state_dict.items() if not k.endswith("position_ids")}
        if "logit_scale" not in sd:
            sd["logit_scale"] = self.logit_scale.data.clone()
        out = super().load_state_dict(sd, strict=strict, assign=assign)
        self._packed.clear()
        return out

    def _patch_weight(self):
        """Conv2d(3, H, P, stride=P).weight flattened to [H, 3 P P] and zero-padded to the operand width of ops.clip_patch_rows"""
        def make():
            w = self.vision_model.embeddings.patch_embedding.weight.data
            flat = w.reshape(w.shape[0], -1)
            Kp = (flat.shape[1] + 7) & ~7
            return torch.nn.functional.pad(flat, (0, Kp - flat.shape[1]))
        return self._w("patch", make)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _attention(self, qkv, B, S, nh, hd):
        H = nh * hd
        alpha = float(hd) ** -0.5
        if qkv.dtype == torch.bfloat16:
            return ops.attention_fwd_ex(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, S, S, nh, hd, alpha)[0]
        ld = (S + 3) & ~3       # a k-contiguous f32 operand's rows are padded to 16 bytes; the softmax writes the pad columns as 0
        return materialised_attention(qkv, B, S, nh, hd, alpha=alpha, ld=ld, softmax=lambda scores: ops.softmax_(scores, B * nh * S, S, ld),
                                      ctx_dtype=torch.float32)

    @torch.no_grad()
    def forward(self, pixel_values=None, output_attentions=None, output_hidden_states=None, return_dict=None, interpolate_pos_encoding=False):
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        if interpolate_pos_encoding:
            raise NotImplementedError("CLIPImageEncoder: interpolate_pos_encoding=True is outside the MI355X hot-path build (resize the "
                                      "image to the tower's image_size instead: muse.CLIPScorer does)")
        if output_attentions:
            raise NotImplementedError("CLIPImageEncoder: output_attentions is outside the MI355X hot-path build (the fused attention kernel "
                                      "keeps no probabilities)")
        cfg, vm, cd = self.config, self.vision_model, self.compute_dtype
        I, P = int(cfg.image_size), int(cfg.patch_size)
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
            raise ValueError(f"pixel_values is [batch, 3, {I}, {I}], got {tuple(pixel_values.shape)}")
        if pixel_values.shape[2] != I or pixel_values.shape[3] != I:
            raise ValueError(f"Input image size ({pixel_values.shape[2]}*{pixel_values.shape[3]}) doesn't match model ({I}*{I}).")
        ops.require_gpu(pixel_values, vm.post_layernorm.weight)
        px = pixel_values.to(torch.float32).contiguous()
        B, S = int(px.shape[0]), self.tokens
        H, nh = int(cfg.hidden_size), int(cfg.num_attention_heads)
        hd, eps = H // nh, float(cfg.layer_norm_eps)
        quick = cfg.hidden_act == "quick_gelu"
        emb = vm.embeddings
        patches = ops.linear(ops.clip_patch_rows(px, P, cd), self._patch_weight(), out_dtype=torch.float32)
        x = ops.clip_vision_embed_ln(patches, emb.class_embedding.data, emb.position_embedding.weight.data, vm.pre_layrnorm.weight.data,
                                     vm.pre_layrnorm.bias.data, eps, B)
        hidden = [x]
        for i, lyr in enumerate(vm.encoder.layers):
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
        # upstream: last_hidden_state is the encoder's output as it is; only the class token goes through post_layernorm
        first = torch.arange(B, device=x.device, dtype=torch.int64) * S
        pooled = ops.layernorm_bias_fwd(ops.gather_rows(x, first, torch.float32), vm.post_layernorm.weight.data, vm.post_layernorm.bias.data,
                                        eps, torch.float32)
        wp = self._w("proj", lambda: self.visual_projection.weight.data)
        out = CLIPVisionOutput()
        out["image_embeds"] = ops.linear(pooled if cd == torch.float32 else ops.cast_to_bf16(pooled), wp, out_dtype=torch.float32)
        out["last_hidden_state"] = x.view(B, S, H)
        out.__dict__["_pooler_output"] = pooled
        if output_hidden_states:
            out["hidden_states"] = tuple(t.view(B, S, H) for t in hidden)
        return out if (return_dict is None or return_dict) else out.to_tuple()

    # ---- transformers checkpoints -----------------------------------------------------------------------------------------------------
    @classmethod
    def from_transformers(cls, module):
        """a live transformers CLIPVisionModelWithProjection, or a CLIPModel (its vision_model, visual_projection and logit_scale) ->
        CLIPImageEncoder with a copy of the weights"""
        sd = {k: v.detach().to("cpu", torch.float32).clone() for k, v in module.state_dict().items()
              if not k.startswith(("text_model.", "text_projection."))}
        config = module.config
        cfg = config.vision_config.to_dict() if hasattr(config, "vision_config") else config.to_dict()
        cfg = {k: v for k, v in cfg.items() if k != "architectures"}
        if hasattr(config, "vision_config"):
            cfg["projection_dim"] = config.projection_dim
        model = cls(cfg)
        model.load_state_dict(sd, strict=True)
        return model

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, torch_dtype=None, **config_overrides):
        """a LOCAL transformers directory: config.json + model.safetensors or pytorch_model.bin (one file: sharded checkpoints are
        refused) - a vision-only checkpoint or a full CLIPModel one (`vision_config`, prefixed keys; its text tower is dropped).  A
        preprocessor_config.json next to it supplies `image_mean` / `image_std`.  Keyword arguments override config entries."""
        path, cfg, sd = read_checkpoint(pretrained_model_name_or_path, subfolder, refuse_sharded=cls.__name__)
        if "vision_config" in cfg and "hidden_size" not in cfg:       # a full CLIPModel config: the image tower's part
            cfg = dict(cfg["vision_config"], projection_dim=cfg.get("projection_dim", cfg["vision_config"].get("projection_dim")))
        if any(k.startswith(("text_model.", "text_projection.")) for k in sd):
            sd = {k: v for k, v in sd.items() if k.startswith(_OWN)}
        pre = os.path.join(path, "preprocessor_config.json")
        if os.path.isfile(pre):
            with open(pre, "r", encoding="utf-8") as f:
                pc = json.load(f)
            for k in ("image_mean", "image_std"):
                if pc.get(k) is not None:
                    cfg.setdefault(k, pc[k])
        cfg.update(config_overrides)
        cfg.pop("architectures", None)
        model = cls(cfg)
        model.load_state_dict(sd, strict=True)
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        return model

    def save_pretrained(self, save_directory, **kwargs):
        """config.json + model.safetensors in the vision-only layout (`CLIPVisionModelWithProjection.from_pretrained` loads the directory;
        it ignores the extra `logit_scale`), and the preprocessor_config.json that carries image_mean / image_std"""
        write_checkpoint(save_directory, self.config, self.state_dict())
        size = int(self.config.image_size)
        pre = dict(image_processor_type="CLIPImageProcessor", do_resize=True, size={"shortest_edge": size}, resample=3, do_center_crop=True,
                   crop_size={"height": size, "width": size}, do_rescale=True, rescale_factor=1.0 / 255.0, do_normalize=True,
                   image_mean=list(self.image_mean), image_std=list(self.image_std), do_convert_rgb=True)
        with open(os.path.join(save_directory, "preprocessor_config.json"), "w", encoding="utf-8") as f:
            f.write(json.dumps(pre, indent=2, sort_keys=True) + "\n")

# ---- the score ----------------------------------------------------------------------------------------------------------------------
def clip_scores(image_embeds, text_embeds, logit_scale=None):
    """(cosine [Bi, Bt], logits_per_image [Bi, Bt]) of image_embeds [Bi, D] and text_embeds [Bt, D] (f32, on the GPU), un-normalised as
    the towers return them.  `logit_scale` is CLIPModel's parameter, i.e. the LOGARITHM of the multiplier (a one-element tensor or a
    float; None: ln(1 / 0.07)); logits_per_image = exp(logit_scale) * cosine, what `CLIPModel.forward(...).logits_per_image` holds.
    Each side is normalised in one pass (no epsilon: a zero embedding gives NaN in its row / column, as upstream's x / x.norm()), the
    multiplier rides on the image rows, and both matrices are exact-f32 products."""
    ops.require_gpu(image_embeds, text_embeds)
    if image_embeds.dim() != 2 or text_embeds.dim() != 2 or image_embeds.shape[1] != text_embeds.shape[1]:
        raise ValueError(f"clip_scores: image_embeds [Bi, D] and text_embeds [Bt, D], got {tuple(image_embeds.shape)} and {tuple(text_embeds.shape)}")
    img, txt = image_embeds.to(torch.float32).contiguous(), text_embeds.to(torch.float32).contiguous()
    (Bi, D), Bt = img.shape, txt.shape[0]
    if D % 4:
        raise ops._hip.MuseHipError(f"clip_scores: the embedding width {D} is a multiple of 4 (an f32 GEMM operand row is whole 16-byte chunks)")
    if logit_scale is None:
        logit_scale = math.log(1.0 / 0.07)
    if not torch.is_tensor(logit_scale):
        logit_scale = torch.tensor(float(logit_scale), dtype=torch.float32)
    ls = logit_scale.detach().to(device=img.device, dtype=torch.float32).reshape(1)
    nt = ops.l2_normalize_rows(txt)
    ldc = (Bt + 3) & ~3

    def product(rows):
        c = torch.empty((Bi, ldc), dtype=torch.float32, device=img.device)
        ops.gemm(rows, nt, c, Bi, Bt, D, la=0, lb=0, lda=D, ldb=D, ldc=ldc)
        return c[:, :Bt]

    return product(ops.l2_normalize_rows(img)), product(ops.l2_normalize_rows(img, log_mult=ls))


class CLIPScores:
    """what `CLIPScorer.__call__` returns: `cosine` and `logits_per_image` [Bi, Bt] (f32, on the device), the embeddings they were
    made of, and `pairwise()` - the diagonal of `cosine` (image i against caption i) when Bi == Bt"""

    def __init__(self, cosine, logits_per_image, image_embeds, text_embeds):
        self.cosine, self.logits_per_image, self.image_embeds, self.text_embeds = cosine, logits_per_image, image_embeds, text_embeds

    def pairwise(self):
        if self.cosine.shape[0] != self.cosine.shape[1]:
            raise ValueError(f"pairwise() needs as many captions as images, got a {tuple(self.cosine.shape)} matrix")
        return torch.diagonal(self.cosine)


class CLIPScorer:
    """CLIP scores of generated images against their prompts, on the device:

        scorer = muse.CLIPScorer(muse.CLIPImageEncoder.from_pretrained(path), muse.CLIPTextEncoder.from_pretrained(path), tokenizer)
        scores = scorer(pipe(text=prompts, output_type="pt"), text=prompts)      # .cosine, .logits_per_image, .pairwise()

    `images`: [B, 3, R, R] f32 in [0, 1] on the GPU (what `PipelineMuse(..., output_type="pt")` returns), resized to the tower's
    `image_size` and normalised with its `image_mean` / `image_std` in one launch (antialiased bicubic in f32, ATen's definition - NOT
    PIL's 8-bit resize of upstream's CLIPImageProcessor: see the module docstring); or `pixel_values` [B, 3, image_size, image_size],
    already preprocessed, which bypasses that stage.  Text: `text` (strings, needs `tokenizer` and `text_encoder`), `input_ids` (needs
    `text_encoder`: a muse.CLIPTextEncoder with its projection, or any callable whose result has - or is - `text_embeds`), or
    pre-computed `text_embeds` [Bt, D]."""

    def __init__(self, image_encoder, text_encoder=None, tokenizer=None):
        self.image_encoder, self.text_encoder, self.tokenizer = image_encoder, text_encoder, tokenizer

    def preprocess(self, images):
        enc = self.image_encoder
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
            raise ValueError(f"CLIPScorer: images is [B, 3, R, R] (square: crop first), got {tuple(images.shape)}")
        return ops.resize_bicubic_norm(images.to(torch.float32).contiguous(), int(enc.config.image_size), enc.image_mean, enc.image_std)

    def _text_embeds(self, text, input_ids, device):
        if input_ids is None:
            if text is None:
                raise ValueError("CLIPScorer: pass text=, input_ids= or text_embeds=")
            if self.tokenizer is None:
                raise ValueError("CLIPScorer: text= needs the tokenizer handed to the constructor")
            tok = self.tokenizer
            text = [text] if isinstance(text, str) else list(text)
            input_ids = tok(text, return_tensors="pt", padding="max_length", truncation=True, max_length=tok.model_max_length).input_ids
        if self.text_encoder is None:
            raise ValueError("CLIPScorer: text= / input_ids= need the text_encoder handed to the constructor")
        out = self.text_encoder(input_ids.to(device))
        if torch.is_tensor(out):
            return out
        embeds = out.get("text_embeds") if isinstance(out, dict) else getattr(out, "text_embeds", None)
        if embeds is None:
            raise ValueError("CLIPScorer: the text encoder returned no text_embeds (a CLIP text tower WITH its projection is needed)")
        return embeds

    @torch.no_grad()
    def image_embeds(self, images=None, pixel_values=None):
        """the image half of `__call__` on its own: [B, projection_dim] f32 on the device, un-normalised as the tower returns them - the
        features `accumulate` feeds to a muse.FeatureStats"""
        if (images is None) == (pixel_values is None):
            raise ValueError("CLIPScorer: pass exactly one of images= and pixel_values=")
        if pixel_values is None:
            pixel_values = self.preprocess(images)
        return self.image_encoder(pixel_values).image_embeds

    def accumulate(self, stats, images=None, pixel_values=None):
        """embed a batch and add it to `stats` (a muse.FeatureStats of the tower's projection_dim, on the same device) for a Frechet
        distance on CLIP image embeds (muse/frechet.py), or a muse.FeatureBank for the MMD / CMMD on them (muse/mmd.py): the embeds go
        straight into `stats.update`, nothing visits the host"""
        return stats.update(self.image_embeds(images=images, pixel_values=pixel_values))

    @torch.no_grad()
    def __call__(self, images=None, text=None, input_ids=None, text_embeds=None, pixel_values=None):
        image_embeds = self.image_embeds(images=images, pixel_values=pixel_values)
        if text_embeds is None:
            text_embeds = self._text_embeds(text, input_ids, image_embeds.device)
        cosine, logits = clip_scores(image_embeds, text_embeds, self.image_encoder.logit_scale.data)
        return CLIPScores(cosine, logits, image_embeds, text_embeds)
