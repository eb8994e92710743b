"""Maximum mean discrepancy between two sets of CLIP image embeds, and CMMD: the metric Jayasumana et al. ("Rethinking FID: Towards a
Better Evaluation Metric for Image Generation", CVPR 2024) define on this feature space.

    bank = muse.FeatureBank(encoder.config.projection_dim, "cuda")
    for batch in images:                                   # [B, 3, R, R] f32 in [0, 1] on the GPU
        scorer.accumulate(bank, batch)                     # resize -> tower -> one row copy; nothing visits the host
    value = muse.cmmd_distance(bank, muse.FeatureBank.load("real_embeds.npz", device="cuda"))

Where the Frechet distance of muse/frechet.py assumes Gaussian features and needs a d x d covariance (rank-deficient below d images), the
MMD assumes nothing about the distribution and needs only the rows: it is already stable at the few hundred to few thousand images of a
periodic evaluation inside a training run.  What it needs is every PAIR of rows: three sums of n^2, m^2 and n m Gaussian kernel values.
Those are one fused HIP launch each (csrc/mmd.hip: f64 MFMA dot products from exact products, exp and the reduction in the same kernel,
the n x m matrix never written); the three mean kernel values are all close to 1 and their combination is 1e-4 .. 1e-3 of that, which
is why everything is f64.  The combination itself is host f64, from one copy of six numbers."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class FeatureBank:
    """f32 feature rows kept on `device`: what the MMD needs where the Frechet distance needs FeatureStats.  `update` has FeatureStats'
    signature, so `CLIPScorer.accumulate(bank, images)` fills it.  The buffer grows by doubling; `features()` is the [n, dim] view of it
    (valid until the next growth)."""

    def __init__(self, dim, device="cuda"):
        self.dim = int(dim)
        if self.dim < 1 or self.dim % 4:
            raise ValueError(f"FeatureBank: the feature width is a positive multiple of 4 (muse_rbf_pair_sums_f64), got {dim}")
        self.n = 0
        self._buf = torch.empty((0, self.dim), dtype=torch.float32, device=device)

    def _reserve(self, rows):
        if rows > self._buf.shape[0]:
            cap = max(self._buf.shape[0], 64)
            while cap < rows:
                cap *= 2
            buf = torch.empty((cap, self.dim), dtype=torch.float32, device=self._buf.device)
            buf[:self.n].copy_(self._buf[:self.n])
            self._buf = buf

    @torch.no_grad()
    def update(self, features):
        """features: f32 [B, dim] on the bank's device, any B (0 included), any strides.  One device copy; no host synchronisation."""
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"FeatureBank.update: features is [B, {self.dim}], got {tuple(getattr(features, 'shape', ()))}")
        if features.dtype != torch.float32 or features.device != self._buf.device:
            raise ValueError(f"FeatureBank.update: features is f32 on {self._buf.device}, got {features.dtype} on {features.device}")
        b = int(features.shape[0])
        self._reserve(self.n + b)
        self._buf[self.n:self.n + b].copy_(features)
        self.n += b
        return self

    def features(self):
        """-> f32 [n, dim], a view of the bank's buffer"""
        return self._buf[:self.n]

    def merge(self, other):
        """append another bank's rows (another shard's or another rank's)"""
        if not isinstance(other, FeatureBank) or other.dim != self.dim:
            raise ValueError(f"FeatureBank.merge: other is a FeatureBank of width {self.dim}")
        return self.update(other.features().to(self._buf.device))

    def to(self, device):
        self._buf = self._buf.to(device)
        return self

    def save(self, path):
        """one .npz: `features`, f32 [n, dim]"""
        with open(path, "wb") as f:
            np.savez(f, features=self.features().cpu().numpy())

    @classmethod
    def load(cls, path, device="cpu"):
        """a file written by `save` (an .npz with `features`), or a plain [n, d] .npy array - the form precomputed reference embeddings
        are commonly distributed in; any real dtype, converted to f32.  Needs no GPU."""
        z = np.load(path)
        if isinstance(z, np.ndarray):
            x = z
        else:
            with z:
                if "features" not in z.files:
                    raise ValueError(f"FeatureBank.load: {path} has no 'features': not a file written by FeatureBank.save")
                x = z["features"]
        if x.ndim != 2 or x.dtype.kind not in "fiu":
            raise ValueError(f"FeatureBank.load: {path}: a real [n, d] array expected, got {x.dtype} {x.shape}")
        bank = cls(x.shape[1], "cpu")
        bank._buf = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).copy())
        bank.n = int(x.shape[0])
        return bank.to(device)


def _rows(x, which):
    """a FeatureBank, tensor or array -> f32 [n, d] tensor whose rows ops.rbf_pair_sums_f64 takes as they are"""
    if isinstance(x, FeatureBank):
        x = x.features()
    elif not torch.is_tensor(x):
        try:
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        except (TypeError, ValueError):
            raise ValueError(f"mmd_distance: {which} is a FeatureBank or an [n, d] tensor or array") from None
    if x.dim() != 2:
        raise ValueError(f"mmd_distance: {which} is [n, d], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"mmd_distance: {which} holds f32 features, got {x.dtype}")
    return x


def _aligned(x):
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) % 4) or x.data_ptr() % 16:
        return x.contiguous()
    return x


def mmd_distance(a, b, sigma=10.0, scale=1000.0, normalize=True, unbiased=False) -> float:
    """scale * MMD^2 of two feature sets under the Gaussian kernel k(x, y) = exp(-|x - y|^2 / (2 sigma^2)); `a`, `b`: a FeatureBank or
    an f32 [n, d] / [m, d] tensor or array, on the GPU (there is no CPU path).  `normalize`: rows are divided by their L2 norm first
    (inside the kernel, by f64 factors; a zero row gives NaN).

        biased (V-statistic, the default):  scale * (sum_ij k(a_i, a_j) / n^2 + sum_ij k(b_i, b_j) / m^2 - 2 sum_ij k(a_i, b_j) / (n m))
        unbiased=True (U-statistic)      :  scale * (sum_{i != j} k(a_i, a_j) / (n (n - 1)) + the same for b - 2 sum_ij k(a_i, b_j) / (n m))

    Two row-norm launches (with `normalize`) and three pair-sum launches, ONE copy of six f64 numbers to the host, the combination there
    in f64.  The RAW value is returned, as muse.frechet_distance does: for equal inputs it may come out a few ulps of the terms below
    zero, and the unbiased estimate is legitimately negative for close distributions."""
    x, y = _rows(a, "a"), _rows(b, "b")
    n, m = int(x.shape[0]), int(y.shape[0])
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"mmd_distance: the two feature widths differ: {x.shape[1]} and {y.shape[1]}")
    if n < 1 or m < 1:
        raise ValueError(f"mmd_distance: both sets need at least one row, got {n} and {m}")
    if unbiased and (n < 2 or m < 2):
        raise ValueError(f"mmd_distance: the unbiased estimate needs at least two rows in each set, got {n} and {m}")
    if not sigma > 0:
        raise ValueError(f"mmd_distance: sigma is positive, got {sigma}")
    ops.require_gpu(x, y)
    x, y = _aligned(x), _aligned(y)
    gamma = 1.0 / (2.0 * float(sigma) ** 2)
    rx = ops.row_norms_f64(x)[1] if normalize else None
    ry = ops.row_norms_f64(y)[1] if normalize else None
    sums = torch.cat([ops.rbf_pair_sums_f64(x, None, gamma, rx), ops.rbf_pair_sums_f64(y, None, gamma, ry),
                      ops.rbf_pair_sums_f64(x, y, gamma, rx, ry)]).cpu().numpy()
    xx_upper, xx_diag, yy_upper, yy_diag, xy = (float(v) for v in sums[:5])
    if unbiased:
        value = 2.0 * xx_upper / (n * (n - 1.0)) + 2.0 * yy_upper / (m * (m - 1.0)) - 2.0 * xy / (float(n) * m)
    else:
        value = (2.0 * xx_upper + xx_diag) / (float(n) * n) + (2.0 * yy_upper + yy_diag) / (float(m) * m) - 2.0 * xy / (float(n) * m)
    return float(scale) * value


def cmmd_distance(a, b) -> float:
    """CMMD (Jayasumana et al., CVPR 2024): 1000 * MMD^2 of the L2-normalised CLIP image embeds under the Gaussian kernel with
    sigma = 10, as the V-statistic -

        1000 * (1 / n^2 sum_ij k(x_i, x_j) + 1 / m^2 sum_ij k(y_i, y_j) - 2 / (n m) sum_ij k(x_i, y_j)),  k(x, y) = exp(-|x - y|^2 / 200),
        x_i = a_i / |a_i|, y_j = b_j / |b_j|

    = mmd_distance(a, b, sigma=10.0, scale=1000.0, normalize=True, unbiased=False).

    The same caveat as muse/frechet.py makes: the tower input here is ATen's antialiased bicubic resize in f32 (the CLIPScorer
    docstring), not the 8-bit image resize of other tools.  Values are therefore comparable with published CMMD numbers by definition,
    but not by preprocessing, and how large that gap is has not been measured here.  For values meant to be read next to published
    ones use the ViT-L/14@336 tower, the one the paper defines the metric on."""
    return mmd_distance(a, b, sigma=10.0, scale=1000.0, normalize=True, unbiased=False)


__all__ = ["FeatureBank", "mmd_distance", "cmmd_distance"]
