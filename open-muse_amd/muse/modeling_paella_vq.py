"""muse.modeling_paella_vq.PaellaVQModel (the Paella tokenizer of the `vq_model.type: "paella_vq"` configs) for MI355X.

Reference: muse/modeling_paella_vq.py:148-225 - same constructor arguments, config keys, state_dict names / shapes and methods
(`encode`, `decode`, `decode_code`, `get_code`, `forward`; the reference class has no `get_soft_code`).

Activations are f32 channels-last rows [B*H*W, C] from the first kernel to the last:

  * in_block (PixelUnshuffle(2) + 1x1 convolution, :159) and out_block (1x1 convolution + PixelShuffle(2), :190-193) are direct
    kernels that read / write the NCHW image (ops.paella_in_block / paella_out_block);
  * ResBlock (:139-145): its first half - LayerNorm, the gamma modulation, the replicate-padded depthwise 3x3 and the residual - is
    ONE op (ops.paella_mix_fwd); its second half is ops.layernorm_bias_fwd with the constant vectors (1 + g3, g4) and two products
    (bias + erf-GELU in the first epilogue, gammas[5] folded into the second weight and bias, the residual in its epilogue);
  * Conv2d(4, 2, 1) (:163) = one patch gather (ops.patch_rows) + one product with K = 16 Cin;  ConvTranspose2d(4, 2, 1) (:185-187) =
    four output phases, each a 2x2 patch gather + one product against its four taps, interleaved by ops.depth_to_space2;
  * the last encoder stage (bias-free 1x1 convolution + BatchNorm2d, :167-170) is one product: the BatchNorm (running statistics,
    eps 1e-5 - the tokenizer is frozen) is folded into the weight and a bias when the weights are packed;
  * the quantizer is ops.vq_nearest_small: direct distances to the 4-wide codebook rows and the argmin in one kernel.

Compute modes (`set_compute_dtype`): torch.float32 (default; exact-f32 products) and "bf16x3" (products as three bf16 MFMA products,
ops.f32_gemms_as_bf16x3; products the bf16 kernels do not take stay exact f32).  A cast to half / bfloat16 selects "bf16x3".
Frozen tokenizer: forward only, no CPU path.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import ops
from ._hip import MuseHipError
from .modeling_utils import ConfigMixin, ModelMixin, register_to_config

# a batch is encoded / decoded in chunks whose largest tensor (a block's 4C-wide hidden rows, or a resampling patch matrix) stays
# below this many bytes: the GEMM operand loaders address one operand with 32-bit byte offsets through a buffer descriptor and
# muse_gemm refuses an operand of 4 GiB or more (csrc/gemm.hip, fill_params: the `>= (1LL << 32)` check -> MUSE_ERR_UNSUPPORTED); half
# of that keeps the f32 output, which the epilogue addresses from the same row indices, inside 32 bits as well
_CHUNK_BYTES = (1 << 31) - 1


class _ResBlock(nn.Module):
    """parameter holder of one ResBlock (:112-134): `gammas`, `depthwise.1`, `channelwise.0`, `channelwise.2`"""

    def __init__(self, c):
        super().__init__()
        self.depthwise = nn.ModuleList([nn.Identity(), nn.Conv2d(c, c, kernel_size=3, groups=c)])
        self.channelwise = nn.ModuleList([nn.Linear(c, 4 * c), nn.Identity(), nn.Linear(4 * c, c)])
        self.gammas = nn.Parameter(torch.zeros(6))
        for m in (self.depthwise[1], self.channelwise[0], self.channelwise[2]):
            nn.init.xavier_uniform_(m.weight)
            nn.init.zeros_(m.bias)


class _Quantizer(nn.Module):
    def __init__(self, n, d):
        super().__init__()
        self.codebook = nn.Embedding(n, d)
        self.codebook.weight.data.uniform_(-1.0 / n, 1.0 / n)


class PaellaVQModel(ModelMixin, ConfigMixin):
    _cast_selects_compute_mode = True

    def _compute_mode_for(self, dtype):
        """a cast to half / bfloat16 selects the f32-class "bf16x3" mode (the parameters stay f32), a cast to f32 / f64 exact f32 -
        the rule of VQGANModel._compute_mode_for"""
        if dtype is None or not dtype.is_floating_point:
            return False
        self.set_compute_dtype("bf16x3" if dtype in (torch.float16, torch.bfloat16) else torch.float32)
        return True

    @register_to_config
    def __init__(self, levels=2, bottleneck_blocks=12, c_hidden=384, c_latent=4, codebook_size=8192, scale_factor=0.3764):
        super().__init__()
        self.c_latent = c_latent
        self.scale_factor = scale_factor
        self.codebook_size = codebook_size
        c_levels = [c_hidden // (2 ** i) for i in reversed(range(levels))]
        if any(c % 4 for c in c_levels) or c_latent > 8:
            raise ValueError("PaellaVQModel (MI355X build): every level's channel count is a multiple of 4 and c_latent <= 8")
        self.in_block = nn.ModuleList([nn.Identity(), nn.Conv2d(12, c_levels[0], kernel_size=1)])
        down = []
        for i in range(levels):
            if i > 0:
                down.append(nn.Conv2d(c_levels[i - 1], c_levels[i], kernel_size=4, stride=2, padding=1))
            down.append(_ResBlock(c_levels[i]))
        down.append(nn.ModuleList([nn.Conv2d(c_levels[-1], c_latent, kernel_size=1, bias=False), nn.BatchNorm2d(c_latent)]))
        self.down_blocks = nn.ModuleList(down)
        self.vquantizer = _Quantizer(codebook_size, c_latent)
        up = [nn.ModuleList([nn.Conv2d(c_latent, c_levels[-1], kernel_size=1)])]
        for i in range(levels):
            c = c_levels[levels - 1 - i]
            up.extend(_ResBlock(c) for _ in range(bottleneck_blocks if i == 0 else 1))
            if i < levels - 1:
                up.append(nn.ConvTranspose2d(c, c_levels[levels - 2 - i], kernel_size=4, stride=2, padding=1))
        self.up_blocks = nn.ModuleList(up)
        self.out_block = nn.ModuleList([nn.Conv2d(c_levels[0], 12, kernel_size=1)])
        self.compute_dtype = torch.float32
        self._packed = {}
        self.eval()

    # ---- engine ---------------------------------------------------------------------------------------------------------------
    def set_compute_dtype(self, dtype):
        """torch.float32: exact-f32 products; "bf16x3": every product the bf16 kernels take as three bf16 MFMA products (f32-class)"""
        if dtype not in (torch.float32, "bf16x3"):
            raise ValueError('compute dtype must be torch.float32 or "bf16x3"')
        self.compute_dtype = dtype
        return self

    def _apply(self, fn, recurse=True):
        self._packed = {}
        return super()._apply(fn, recurse)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        self._packed = {}
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _check(self, t):
        if not t.is_cuda:
            raise MuseHipError(f"{type(self).__name__} (MI355X build) has no CPU path: move the model and inputs to the GPU")

    def _pack(self, key, make):
        hit = self._packed.get(key)
        if hit is None:
            hit = self._packed[key] = make()
        return hit

    def _gemms(self):
        return ops.f32_gemms_as_bf16x3(self.compute_dtype == "bf16x3")

    # ---- packed weights -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _w_res(blk: _ResBlock):
        g = blk.gammas.data.float()
        c = blk.depthwise[1].weight.shape[0]
        one = torch.ones(c, dtype=torch.float32, device=g.device)
        return dict(
            g=g.contiguous(),
            w9=blk.depthwise[1].weight.data.float().reshape(c, 9).t().contiguous(),          # tap-major [9, C]
            b9=blk.depthwise[1].bias.data.float().contiguous(),
            ln_w=(one * (1.0 + g[3])).contiguous(), ln_b=(one * g[4]).contiguous(),
            w1=blk.channelwise[0].weight.data.float().contiguous(), b1=blk.channelwise[0].bias.data.float().contiguous(),
            w2=(blk.channelwise[2].weight.data.float() * g[5]).contiguous(), b2=(blk.channelwise[2].bias.data.float() * g[5]).contiguous())

    @staticmethod
    def _w_down(conv):      # Conv2d(4, 2, 1): [Cout, Cin, 4, 4] -> [Cout, (ky, kx, cin)]
        w = conv.weight.data.float()
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous(), conv.bias.data.float().contiguous()

    @staticmethod
    def _w_up(conv):        # ConvTranspose2d(4, 2, 1): [Cin, Cout, 4, 4] -> four phases [Cout, (j, i, cin)] with taps (3 - a - 2j, 3 - b - 2i)
        w = conv.weight.data.float()
        phases = []
        for a in (0, 1):
            for b in (0, 1):
                taps = w[:, :, [3 - a, 1 - a]][:, :, :, [3 - b, 1 - b]]               # [Cin, Cout, j, i]
                phases.append(taps.permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous())
        return phases, conv.bias.data.float().contiguous()

    @staticmethod
    def _w_latent(stage):   # bias-free 1x1 convolution + BatchNorm2d (eval) as one weight and bias
        conv, bn = stage[0], stage[1]
        s = bn.weight.data.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = conv.weight.data.double().reshape(conv.weight.shape[0], -1) * s[:, None]
        return w.float().contiguous(), (bn.bias.data.double() - bn.running_mean.double() * s).float().contiguous()

    # ---- blocks -----------------------------------------------------------------------------------------------------------------------
    def _res(self, x, blk: _ResBlock, B, H, W):
        p = self._pack((id(blk), "res"), lambda: self._w_res(blk))
        x = self._mix(x, p, B, H, W)
        h = ops.layernorm_bias_fwd(x, p["ln_w"], p["ln_b"], 1e-6, torch.float32)
        with self._gemms():
            if self.compute_dtype == "bf16x3":     # (the bf16x3 product has no activation epilogue: the GELU is its own pass)
                h = ops.gelu_fwd(ops.linear(h, p["w1"], bias=p["b1"]))
            else:
                h = ops.linear(h, p["w1"], bias=p["b1"], act=1)
            return ops.linear(h, p["w2"], bias=p["b2"], residual=x)

    def _mix(self, x, p, B, H, W):
        """first half of a block in one op (scripts/exp/paella_encode.py swaps the unfused composition in here to time it)"""
        return ops.paella_mix_fwd(x, p["w9"], p["b9"], p["g"], B, H, W)

    def _down(self, x, conv, B, H, W):
        w, b = self._pack((id(conv), "down"), lambda: self._w_down(conv))
        patches = ops.patch_rows(x, B, H, W, x.shape[1], 4, 2, 1, 1, H // 2, W // 2)
        with self._gemms():
            return ops.linear(patches, w, bias=b)

    def _up(self, x, conv, B, H, W):
        phases, b = self._pack((id(conv), "up"), lambda: self._w_up(conv))
        cout = b.shape[0]
        packed = torch.empty((B * H * W, 4 * cout), dtype=torch.float32, device=x.device)
        with self._gemms():
            for a in (0, 1):
                for c in (0, 1):
                    ph = 2 * a + c
                    patches = ops.patch_rows(x, B, H, W, x.shape[1], 2, 1, 1 - a, 1 - c, H, W)
                    ops.linear(patches, phases[ph], out=packed[:, ph * cout:(ph + 1) * cout], bias=b)
        return ops.depth_to_space2(packed, B, 2 * H, 2 * W, cout)

    def _chunks(self, B, rows_per_image, widest):
        per = max(1, _CHUNK_BYTES // max(1, rows_per_image * widest * 4))
        return [(s, min(B, s + per)) for s in range(0, B, per)]

    # ---- encoder / decoder --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _encode_rows(self, pixel_values):
        """NCHW pixels -> encoder output before quantisation as rows [B*h*w, c_latent] f32, and (B, h, w)"""
        B, C, H, W = pixel_values.shape
        levels = self.config.levels
        if C != 3:
            raise ValueError("PaellaVQModel encodes 3-channel images")
        if (H | W) % (1 << levels):
            raise ValueError("image height / width must be multiples of 2 ** levels")
        self._check(pixel_values)
        px = pixel_values.float().contiguous()
        c0 = self.in_block[1].weight.shape[0]     # (a level's 4C hidden rows and its 16 Cin patch rows are the same size; level 0 is the largest)
        out = [self._encode_chunk(px[s:e]) for s, e in self._chunks(B, (H // 2) * (W // 2), 4 * c0)]
        return (out[0] if len(out) == 1 else torch.cat(out, 0)), (B, H >> levels, W >> levels)

    def _encode_chunk(self, px):
        B, _, H, W = px.shape
        conv = self.in_block[1]
        w12, b12 = self._pack((id(conv), "in"), lambda: (conv.weight.data.float().reshape(conv.weight.shape[0], 12).t().contiguous(),
                                                        conv.bias.data.float().contiguous()))
        x = ops.paella_in_block(px, w12, b12)
        H, W = H // 2, W // 2
        for blk in self.down_blocks[:-1]:
            if isinstance(blk, _ResBlock):
                x = self._res(x, blk, B, H, W)
            else:
                x = self._down(x, blk, B, H, W)
                H, W = H // 2, W // 2
        stage = self.down_blocks[-1]
        wl, bl = self._pack((id(stage), "latent"), lambda: self._w_latent(stage))
        with self._gemms():
            return ops.linear(x, wl, bias=bl)

    @torch.no_grad()
    def _decode_rows(self, zq, B, H, W):
        """zq rows [B*H*W, c_latent] f32 -> NCHW f32 image [B, 3, H * 2 ** levels, W * 2 ** levels]"""
        c_top = self.up_blocks[0][0].weight.shape[0]
        scale = 1 << (self.config.levels - 1)
        c0 = self.out_block[0].weight.shape[1]
        widest = max(4 * c_top, 4 * c0 * scale * scale)
        zq = zq.view(B, H * W, -1)
        out = [self._decode_chunk(zq[s:e].reshape((e - s) * H * W, -1), e - s, H, W) for s, e in self._chunks(B, H * W, widest)]
        return out[0] if len(out) == 1 else torch.cat(out, 0)

    def _decode_chunk(self, x, B, H, W):
        conv = self.up_blocks[0][0]
        w, b = self._pack((id(conv), "up0"), lambda: (conv.weight.data.float().reshape(conv.weight.shape[0], -1).contiguous(),
                                                     conv.bias.data.float().contiguous()))
        with self._gemms():
            x = ops.linear(x.contiguous(), w, bias=b)
        for blk in self.up_blocks[1:]:
            if isinstance(blk, _ResBlock):
                x = self._res(x, blk, B, H, W)
            else:
                x = self._up(x, blk, B, H, W)
                H, W = 2 * H, 2 * W
        conv = self.out_block[0]
        w12, b12 = self._pack((id(conv), "out"), lambda: (conv.weight.data.float().reshape(12, -1).contiguous(), conv.bias.data.float().contiguous()))
        return ops.paella_out_block(x, w12, b12, B, 2 * H, 2 * W)

    def _codebook(self):
        return self.vquantizer.codebook.weight.data

    def _scaled_codebook(self):
        """codebook / scale_factor with the reference's rounding: one correctly rounded f32 division by the f32 scale (the quotient of
        two f32 numbers taken in f64 and rounded once more is that division: 53 >= 2 * 24 + 2 bits), computed once per weight load"""
        def make():
            s32 = float(torch.tensor(self.scale_factor, dtype=torch.float32))
            return (self._codebook().double() / s32).float().contiguous()
        return self._pack(("codebook", "scaled"), make)

    def _nearest(self, z):
        return ops.vq_nearest_small(z, self._codebook())

    # ---- public surface (reference :195-225) ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x):
        z, (B, H, W) = self._encode_rows(x)
        idx = self._nearest(z)
        zq_rows = ops.gather_rows(self._scaled_codebook(), idx, torch.float32)    # == (one-hot @ codebook) / scale_factor (:51-55, :201)
        return ops.nhwc_to_nchw(zq_rows.view(B, H, W, -1), zq_rows.shape[1]), idx.view(B, H * W), None

    @torch.no_grad()
    def decode(self, x):
        self._check(x)
        B, C, H, W = x.shape
        rows = ops.nchw_to_nhwc((x.float() * self.scale_factor).contiguous(), torch.float32, C)
        return self._decode_rows(rows.view(B * H * W, C), B, H, W)

    @torch.no_grad()
    def decode_code(self, codebook_indices):
        """(no scale_factor here: the reference's decode_code does not apply it, :211-215)"""
        self._check(codebook_indices)
        B, T = codebook_indices.shape
        side = int(math.sqrt(T))
        zq = ops.gather_rows(self._codebook(), codebook_indices.contiguous().view(-1), torch.float32)
        return self._decode_rows(zq, B, side, side)

    @torch.no_grad()
    def get_code(self, pixel_values):
        z, (B, H, W) = self._encode_rows(pixel_values)
        return self._nearest(z).view(B, H * W)

    def forward(self, x, quantize=False):
        return self.decode(self.encode(x)[0])
