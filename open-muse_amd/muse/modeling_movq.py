"""muse.modeling_movq.MOVQ (the MoVQ tokenizer of the `vq_model.type: "movq"` configs: cc12m_movq.yaml, imagenet_movq.yaml,
imagenet_text2image_movq_conv.yaml - openMUSE/movq-lion-high-res-f8-16384) for MI355X.

Reference: muse/modeling_movq.py:555-619 - same constructor arguments, config keys, state_dict names / shapes and methods (`encode`,
`decode`, `decode_code`, `get_code`, `forward`; the reference class has no `get_soft_code`).

It runs on the engine of the other two convolutional tokenizers (modeling_maskgit_vqgan._ConvEngine: NHWC activations, implicit-GEMM
MFMA convolutions with bias / residual in the epilogue, GroupNorm statistics from the producing kernel) and shares the taming model's
encoder flow (modeling_taming_vqgan.VQGANModel: biased 3x3 convolutions, zero-pad stride-2 Downsample, single-head pixel attention, a
level's attention blocks run only when the level holds more than one, :260,:299).  What this architecture adds:

  * q / k / v / proj_out of an AttnBlock are nn.Linear weights [C, C] (:168-171), not 1x1 convolutions;
  * every normalisation of the DECODER is a SpatialNorm (:21-49): GroupNorm(f) * conv_y(nearest(zq)) + conv_b(nearest(zq)) with zq the
    quantised latent itself (before post_quant_conv, at latent resolution).  One kernel (ops.spatial_norm): no up-sampled copy of zq,
    no modulation tensors.  In "bf16x3" mode a norm that feeds a 3x3 convolution of the LDS-DMA kernel is written as that
    convolution's (hi, lo) operand planes; every other norm as the f32 tensor;
  * the quantizer is 4 wide: ops.vq_nearest_small (direct distances and argmin in one kernel).  The reference takes the argmin of
    torch.cdist, the un-squared distance: the same winner;
  * the 4-channel layers around the quantizer (encoder.conv_out's consumer quant_conv, post_quant_conv, decoder.conv_in) stay exact f32
    in "bf16x3" mode: four input channels are no whole bf16 operand vector.

Compute modes (`set_compute_dtype`): torch.float32 (default) and "bf16x3"; a cast to half / bfloat16 selects "bf16x3" with f32
parameters.  Frozen tokenizer: forward only, no CPU path.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .modeling_maskgit_vqgan import _Conv, _ConvEngine, _Norm, _Quantizer
from .modeling_taming_vqgan import VQGANModel, _Res, _Resample
from .modeling_utils import ConfigMixin, ModelMixin, register_to_config


class _Linear(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c, c))
        self.bias = nn.Parameter(torch.empty(c))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))   # nn.Linear default init
        nn.init.uniform_(self.bias, -1.0 / math.sqrt(c), 1.0 / math.sqrt(c))


class _SpatialNorm(nn.Module):
    """parameter holder of SpatialNorm (:21-49): `norm_layer`, `conv_y`, `conv_b`"""

    def __init__(self, c, zq_ch):
        super().__init__()
        self.norm_layer = _Norm(c)
        self.conv_y = _Conv(zq_ch, c, 1, True)
        self.conv_b = _Conv(zq_ch, c, 1, True)


class _SRes(nn.Module):
    def __init__(self, cin, cout, zq_ch):
        super().__init__()
        self.norm1 = _SpatialNorm(cin, zq_ch)
        self.conv1 = _Conv(cin, cout, 3, True)
        self.norm2 = _SpatialNorm(cout, zq_ch)
        self.conv2 = _Conv(cout, cout, 3, True)
        if cin != cout:
            self.nin_shortcut = _Conv(cin, cout, 1, True)


class _Attn(nn.Module):
    def __init__(self, c, zq_ch=None):
        super().__init__()
        self.norm = _SpatialNorm(c, zq_ch) if zq_ch else _Norm(c)
        self.q, self.k, self.v, self.proj_out = (_Linear(c) for _ in range(4))


class _Level(nn.Module):
    def __init__(self, cin, cout, nblocks, attn, resample_name, with_conv, zq_ch=None):
        super().__init__()
        self.block = nn.ModuleList([(_SRes(cin if i == 0 else cout, cout, zq_ch) if zq_ch else _Res(cin if i == 0 else cout, cout))
                                    for i in range(nblocks)])
        self.attn = nn.ModuleList([_Attn(cout, zq_ch) for _ in range(nblocks)] if attn else [])
        if resample_name:
            setattr(self, resample_name, _Resample(cout, with_conv))


class _Mid(nn.Module):
    def __init__(self, c, zq_ch=None):
        super().__init__()
        self.block_1 = _SRes(c, c, zq_ch) if zq_ch else _Res(c, c)
        self.attn_1 = _Attn(c, zq_ch)
        self.block_2 = _SRes(c, c, zq_ch) if zq_ch else _Res(c, c)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        hc, mult, nb = cfg.hidden_channels, tuple(cfg.channel_mult), cfg.num_res_blocks
        nres, attn_res = len(mult), tuple(cfg.attn_resolutions)
        self.conv_in = _Conv(cfg.num_channels, hc, 3, True)
        in_mult, cur, levels = (1,) + mult, cfg.resolution, []
        for i in range(nres):
            last = i == nres - 1
            levels.append(_Level(hc * in_mult[i], hc * mult[i], nb, cur in attn_res, None if last else "downsample", cfg.resample_with_conv))
            if not last:
                cur //= 2
        self.down = nn.ModuleList(levels)
        mid = hc * mult[-1]
        self.mid = _Mid(mid)
        self.norm_out = _Norm(mid)
        self.conv_out = _Conv(mid, cfg.z_channels, 3, True)


class _Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        hc, mult, nb, zq_ch = cfg.hidden_channels, tuple(cfg.channel_mult), cfg.num_res_blocks, cfg.quantized_embed_dim
        nres, attn_res = len(mult), tuple(cfg.attn_resolutions)
        mid = hc * mult[-1]
        self.conv_in = _Conv(cfg.z_channels, mid, 3, True)
        self.mid = _Mid(mid, zq_ch)
        cur, levels = cfg.resolution // 2 ** (nres - 1), [None] * nres
        for i in reversed(range(nres)):
            cin = mid if i == nres - 1 else hc * mult[i + 1]
            levels[i] = _Level(cin, hc * mult[i], nb + 1, cur in attn_res, "upsample" if i != 0 else None, cfg.resample_with_conv, zq_ch)
            if i != 0:
                cur *= 2
        self.up = nn.ModuleList(levels)
        self.norm_out = _SpatialNorm(hc * mult[0], zq_ch)
        self.conv_out = _Conv(hc * mult[0], cfg.num_channels, 3, True)


class MOVQ(_ConvEngine, ModelMixin, ConfigMixin):
    _cast_selects_compute_mode = True

    def _compute_mode_for(self, dtype):
        """a cast to half / bfloat16 selects the f32-class "bf16x3" mode (the parameters stay f32), a cast to f32 / f64 exact f32 -
        the rule of VQGANModel._compute_mode_for"""
        if dtype is None or not dtype.is_floating_point:
            return False
        self.set_compute_dtype("bf16x3" if dtype in (torch.float16, torch.bfloat16) else torch.float32)
        return True

    @register_to_config
    def __init__(
        self,
        resolution: int = 256,
        num_channels=3,
        out_channels=3,
        hidden_channels=128,
        channel_mult=(1, 2, 2, 4),
        num_res_blocks=2,
        attn_resolutions=(32,),
        z_channels=4,
        double_z=False,
        num_embeddings=16384,
        quantized_embed_dim=4,
        dropout=0.0,
        resample_with_conv: bool = True,
        commitment_cost: float = 0.25,
    ):
        super().__init__()
        if dropout != 0.0:
            raise NotImplementedError("dropout > 0 in MOVQ is outside the MI355X hot-path build (frozen tokenizer)")
        if z_channels % 4 or quantized_embed_dim not in (4, 8):
            raise ValueError("MOVQ (MI355X build): z_channels is a multiple of 4 and quantized_embed_dim is 4 or 8 (the spatial-norm "
                             "kernel takes a latent of at most 8 channels)")
        self.config.num_resolutions = len(channel_mult)
        self.config.reduction_factor = 2 ** (self.config.num_resolutions - 1)
        self.config.latent_size = resolution // self.config.reduction_factor
        self.encoder = _Encoder(self.config)
        self.decoder = _Decoder(self.config)
        self.quantize = _Quantizer(num_embeddings, quantized_embed_dim)
        self.quant_conv = _Conv(z_channels, quantized_embed_dim, 1, True)
        self.post_quant_conv = _Conv(quantized_embed_dim, z_channels, 1, True)
        self._init_engine()

    def set_compute_dtype(self, dtype):
        """torch.float32: exact-f32 MFMA convolutions; "bf16x3": f32 activations, convolutions as three bf16 MFMA products (f32-class)"""
        if dtype not in (torch.float32, "bf16x3"):
            raise ValueError('compute dtype must be torch.float32 or "bf16x3"')
        self.compute_dtype = dtype
        return self

    # ---- engine ---------------------------------------------------------------------------------------------------------------
    def _conv(self, x, conv, B, H, W, cd, **kw):
        """the engine's convolution; in "bf16x3" mode a layer whose input is a plain tensor of 4 (mod 8) channels - the 4-wide latent
        around the quantizer - runs on the exact-f32 kernel: the bf16 operand vectors hold 8 channels"""
        if cd == "bf16x3" and torch.is_tensor(x):
            cin = conv.weight.shape[1]
            if x.shape[-1] == self._cpad(cin, torch.float32) != self._cpad(cin, cd):
                cd = torch.float32
        return super()._conv(x, conv, B, H, W, cd, **kw)

    # the encoder is the taming encoder: its flow and blocks are VQGANModel's own functions (they reach the attention through self._attn,
    # which here reads the nn.Linear-shaped weights)
    _res = VQGANModel._res
    _level = VQGANModel._level
    _mid = VQGANModel._mid

    def _encode_nhwc(self, pixel_values):
        """NCHW f32 pixels -> quant_conv(encoder(x)) as [B*h*w, quantized_embed_dim] f32 rows and (B, h, w)"""
        if (pixel_values.shape[-2] | pixel_values.shape[-1]) % self.config.reduction_factor:
            raise ValueError("image height / width must be multiples of the reduction factor")
        return VQGANModel._encode_nhwc(self, pixel_values)

    def _as_conv(self, key, make):
        """a stand-in with the two attributes _w reads, kept with the packed weights (and dropped with them)"""
        hit = self._packed.get(key)
        if hit is None:
            w, b = make()
            hit = self._packed[key] = SimpleNamespace(weight=w, bias=b)
        return hit

    def _qkv(self, att: _Attn):
        """q | k | v as ONE stacked [3C, C, 1, 1] weight"""
        return self._as_conv((id(att), "qkv"), lambda: (torch.cat([att.q.weight.data, att.k.weight.data, att.v.weight.data], 0)[:, :, None, None],
                                                         torch.cat([att.q.bias.data, att.k.bias.data, att.v.bias.data], 0)))

    def _sn_weights(self, norm: _SpatialNorm):
        def make():
            c, z = norm.conv_y.weight.shape[:2]
            return tuple(t.data.float().contiguous() for t in (norm.norm_layer.weight, norm.norm_layer.bias, norm.conv_y.weight.view(c, z),
                                                               norm.conv_y.bias, norm.conv_b.weight.view(c, z), norm.conv_b.bias))
        key = (id(norm), "sn")
        hit = self._packed.get(key)
        if hit is None:
            hit = self._packed[key] = make()
        return hit

    def _sn(self, x, norm: _SpatialNorm, zq, B, H, W, silu=True, split=False):
        """SpatialNorm(x, zq) (+ SiLU); zq = (tensor [B, zh, zw, Z] f32, zh, zw); the producer's statistics are used when x carries them"""
        gamma, beta, wy, by, wb, bb = self._sn_weights(norm)
        return ops.spatial_norm(x, zq[0], gamma, beta, wy, by, wb, bb, B, H, W, gamma.shape[0], zq[1], zq[2], groups=32, eps=1e-6, silu=silu,
                                stats=getattr(x, "_gn_stats", None), split=split)

    def _sn_for(self, x, norm: _SpatialNorm, conv: _Conv, zq, B, H, W, cd):
        """SpatialNorm + SiLU feeding `conv`: the (hi, lo) operand planes when the LDS-DMA kernel takes the layer, else the f32 tensor"""
        cout, cin, k, _ = conv.weight.shape
        split = cd == "bf16x3" and self.dma_conv and ops.conv_split2_ok(B, H, W, cin, cout, k)
        return self._sn(x, norm, zq, B, H, W, silu=True, split=split)

    # ---- blocks ---------------------------------------------------------------------------------------------------------------
    def _sres(self, x, blk: _SRes, zq, B, H, W, cd):
        """decoder ResnetBlock (:132-156): both convolutions leave the next norm's statistics; the shortcut rides conv2's epilogue"""
        h = self._conv(self._sn_for(x, blk.norm1, blk.conv1, zq, B, H, W, cd), blk.conv1, B, H, W, cd, gn_next=True)
        sc = self._conv(x, blk.nin_shortcut, B, H, W, cd) if hasattr(blk, "nin_shortcut") else x
        return self._conv(self._sn_for(h, blk.norm2, blk.conv2, zq, B, H, W, cd), blk.conv2, B, H, W, cd, residual=sc, gn_next=True)

    def _attn(self, x, att: _Attn, B, H, W, cd, zq=None):
        """AttnBlock (:184-224) on the NHWC rows [B*HW, C]: softmax(q k^T / sqrt(C)) v per image, then proj_out + x; the norm (no SiLU)
        is a GroupNorm in the encoder and a SpatialNorm in the decoder"""
        C, HW = att.q.weight.shape[0], H * W
        if zq is None:
            h = self._gn(x, att.norm, B, HW, C, silu=False)
        else:
            h = self._sn(x, att.norm, zq, B, H, W, silu=False)
        qkv = self._conv(h, self._qkv(att), B, H, W, cd).view(B * HW, 3 * C)
        scores = torch.empty((B, HW, HW), dtype=torch.float32, device=x.device)
        ops.gemm(qkv, qkv, scores, HW, HW, C, la=0, lb=0, lda=3 * C, ldb=3 * C, ldc=HW, b_off=C, alpha=float(int(C) ** -0.5),
                 batch=B, sA=(HW * 3 * C, 0), sB=(HW * 3 * C, 0), sC=(HW * HW, 0))
        ops.softmax_(scores, B * HW, HW, HW)
        ctx = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
        ops.gemm(scores, qkv, ctx, HW, C, HW, la=0, lb=1, lda=HW, ldb=3 * C, ldc=C, b_off=2 * C, batch=B,
                 sA=(HW * HW, 0), sB=(HW * 3 * C, 0), sC=(HW * C, 0))
        proj = self._as_conv((id(att), "proj"), lambda: (att.proj_out.weight.data[:, :, None, None], att.proj_out.bias.data))
        return self._conv(ctx, proj, B, H, W, cd, residual=x, gn_next=True)

    # ---- decoder (:436-452) -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _decode_nhwc(self, zq_t, B, H, W):
        """zq_t: the quantised latent [B, H, W, quantized_embed_dim] f32 -> NCHW f32 image"""
        cd, dec = self.compute_dtype, self.decoder
        zq_t = zq_t.contiguous()
        zq = (zq_t, H, W)
        h = self._conv(zq_t, self.post_quant_conv, B, H, W, cd)
        h = self._conv(h, dec.conv_in, B, H, W, cd, gn_next=True)
        h = self._sres(h, dec.mid.block_1, zq, B, H, W, cd)
        h = self._attn(h, dec.mid.attn_1, B, H, W, cd, zq)
        h = self._sres(h, dec.mid.block_2, zq, B, H, W, cd)
        for lvl in reversed(dec.up):
            run_attn = len(lvl.attn) > 1   # the reference's condition (:260): a lone attention block is never applied
            for i, blk in enumerate(lvl.block):
                h = self._sres(h, blk, zq, B, H, W, cd)
                if run_attn:
                    h = self._attn(h, lvl.attn[i], B, H, W, cd, zq)
            if hasattr(lvl, "upsample"):
                H, W = H * 2, W * 2
                if hasattr(lvl.upsample, "conv"):
                    h = self._upsample_conv(h, lvl.upsample.conv, B, H, W, cd)
                elif h.shape[-1] % 4 == 0:   # plain nearest x2 (resample_with_conv = False)
                    h = ops.upsample2x(h.contiguous(), B, H // 2, W // 2, h.shape[-1])
                else:   # (channel counts that are not whole 16-byte vectors: no shipped configuration)
                    h = F.interpolate(h.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1).contiguous()
        h = self._conv(self._sn_for(h, dec.norm_out, dec.conv_out, zq, B, H, W, cd), dec.conv_out, B, H, W, cd)
        return ops.nhwc_to_nchw(h, self.config.num_channels)

    def _codebook(self):
        return self.quantize.embedding.weight.data

    def _nearest(self, z):
        cb = self._codebook()
        return ops.vq_nearest_small(z, cb) if cb.shape[1] <= 8 else ops.vq_nearest(z, cb)

    # ---- public surface (reference :586-619) ------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, pixel_values, return_loss=False):
        if return_loss:
            # VectorQuantizer.forward (:500-508) reads self.beta, which its constructor never sets (it stores commitment_cost): the
            # reference raises AttributeError on this path, so there is no loss value to reproduce
            raise NotImplementedError("MOVQ.encode(return_loss=True): the reference's VectorQuantizer.forward reads `self.beta`, which is "
                                      "never set (modeling_movq.py:502-507) and raises AttributeError; there is no loss to reproduce")
        z, (B, H, W) = self._encode_nhwc(pixel_values)
        idx = self._nearest(z)
        zq_rows = ops.gather_rows(self._codebook(), idx, torch.float32)        # == one-hot @ codebook (:489-493)
        return ops.nhwc_to_nchw(zq_rows.view(B, H, W, -1), zq_rows.shape[1]), idx.view(B, H * W)

    @torch.no_grad()
    def decode(self, quant):
        self._check(quant)
        B, C, H, W = quant.shape
        return self._decode_nhwc(ops.nchw_to_nhwc(quant.float(), torch.float32, C), B, H, W)

    @torch.no_grad()
    def decode_code(self, codebook_indices):
        self._check(codebook_indices)
        B, T = codebook_indices.shape
        side = int(math.sqrt(T))
        zq = ops.gather_rows(self._codebook(), codebook_indices.contiguous().view(-1), torch.float32)
        return self._decode_nhwc(zq.view(B, side, side, -1), B, side, side)

    @torch.no_grad()
    def get_code(self, pixel_values):
        z, (B, H, W) = self._encode_nhwc(pixel_values)
        return self._nearest(z).view(B, H * W)

    def forward(self, pixel_values, return_loss=False):
        z_q, idx = self.encode(pixel_values, return_loss)
        return self.decode(z_q), idx
