"""The row kernels that apply nn.Dropout to their own result (include/muse_hip.h: muse_glu_drop_fwd / _bwd / _fwd_x3 / _bwd_x3,
muse_grn_drop_fwd_ex / muse_grn_drop_bwd) restated on the CPU: the oracle of tests/test_gpu_rowdrop.py.

Contract: the keep bit of flat element e of the row-major [rows, cols] result is muse_dropout(seed, offset)'s (philox_cpu.dropout_keep),
the scale 1 / (1 - p) is formed in float32; the forward multiplies the kernel's f32 result once, the backward multiplies the incoming
gradient (one f32 rounding) before anything else reads it.  References are float64; the gradient the backward reads is the float32
product, as in the kernels."""
import numpy as np
import torch

import philox_cpu as PH


def scale_of(p):
    """1 / (1 - p) as the launchers form it: float32 arithmetic"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(rows, cols, p, seed, offset):
    """bool [rows, cols]"""
    return PH.dropout_keep(rows * cols, p, seed, offset).reshape(rows, cols)


def mult(rows, cols, p, seed, offset):
    """float32 [rows, cols]: scale where kept, 0 where dropped"""
    return np.where(keep_mask(rows, cols, p, seed, offset), scale_of(p), np.float32(0.0)).astype(np.float32)


def dropped_gradient(dh, m):
    """what the backward kernels read: float32(dh * m), dh float32 [rows, cols] (a bf16 gradient: its float32 value)"""
    return (np.asarray(dh, dtype=np.float32) * m).astype(np.float32)


def _gelu(a):
    t = torch.from_numpy(np.asarray(a, dtype=np.float64))
    cdf = 0.5 * (1.0 + torch.erf(t / np.sqrt(2.0)))
    pdf = torch.exp(-0.5 * t * t) / np.sqrt(2.0 * np.pi)
    return (t * cdf).numpy(), (cdf + t * pdf).numpy()


def glu_drop_fwd(ab, m):
    """h = keep * s * (gelu_erf(a) * b): ab [rows, 2 * inter] (a first), m = mult(rows, inter, ...) -> float64 [rows, inter]"""
    inter = ab.shape[1] // 2
    a, b = np.asarray(ab[:, :inter], dtype=np.float64), np.asarray(ab[:, inter:], dtype=np.float64)
    return _gelu(a)[0] * b * m.astype(np.float64)


def glu_drop_bwd(ab, dh, m):
    """d(ab) [rows, 2 * inter] float64 from the dropped gradient float32(dh * m)"""
    inter = ab.shape[1] // 2
    a, b = np.asarray(ab[:, :inter], dtype=np.float64), np.asarray(ab[:, inter:], dtype=np.float64)
    de = dropped_gradient(dh, m).astype(np.float64)
    g, dg = _gelu(a)
    return np.concatenate([de * b * dg, de * g], axis=1)


def grn_drop_fwd(y, m):
    """GlobalResponseNorm's result y [B, S, C] (float64, e.g. spatial_cpu.ref_grn: the statistics see the undropped input) times the mask
    m = mult(B * S, C, ...)"""
    return np.asarray(y, dtype=np.float64) * m.reshape(y.shape).astype(np.float64)
