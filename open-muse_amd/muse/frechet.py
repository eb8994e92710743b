"""Frechet distance between two sets of CLIP image embeds: the distribution half of the reference's evaluation
(scripts/calculate_fid.py:215-220 calls cleanfid's `fid.compute_fid`; benchmark/model_quality.py tabulates it next to the CLIP score).

    stats = muse.FeatureStats(encoder.config.projection_dim, "cuda")
    for batch in images:                                   # [B, 3, R, R] f32 in [0, 1] on the GPU
        scorer.accumulate(stats, batch)                    # resize -> tower -> muse_moments_f64; nothing visits the host
    distance = muse.frechet_distance(stats, muse.FeatureStats.load("real_stats.npz"))

This is NOT "FID".  The features are the un-normalised `image_embeds` of muse.CLIPImageEncoder, not the pool3 layer of an Inception
network: the values are not comparable with Inception FID numbers (the 38.57 of BASELINE.md among them).  The extractor is the one
clean-fid offers as its CLIP mode, but our preprocessing is ATen's antialiased bicubic resize in f32 (the CLIPScorer docstring), not
clean-fid's PIL resize of 8-bit images, so the values differ from clean-fid's CLIP mode too.  Compare only numbers made by this module
with the same tower.

The accumulation is one HIP launch per batch (csrc/moments.hip: the column sums and the upper triangle of x^T x, in f64 from exact
products); mean, covariance and the distance are host f64 (numpy), once per evaluation."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class FeatureStats:
    """Streaming first and second moments of f32 feature rows: `n` (a Python int), `sum` f64 [d] and `outer` f64 [d, d] on `device`.
    `outer` holds sum_n x_n x_n^T on its upper triangle and diagonal only; its strict lower triangle is never read or written by
    `update` (it stays as allocated: zeros)."""

    def __init__(self, dim, device="cuda"):
        self.dim = int(dim)
        if self.dim < 1 or self.dim % 4:
            raise ValueError(f"FeatureStats: the feature width is a positive multiple of 4 (muse_moments_f64), got {dim}")
        self.n = 0
        self.sum = torch.zeros(self.dim, dtype=torch.float64, device=device)
        self.outer = torch.zeros((self.dim, self.dim), dtype=torch.float64, device=device)
        self._given = None              # from_moments: the (mu, sigma) handed in, returned as they are

    # ---- accumulation ---------------------------------------------------------------------------------------------------------------
    def _refuse_given(self, what):
        if self._given is not None:
            raise ValueError(f"FeatureStats.{what}: these statistics were built by from_moments(n, mean, cov); the sums they came from "
                             "are gone (n mean and (n - 1) cov + n mean mean^T are rounded), so they cannot be updated or merged into")

    @torch.no_grad()
    def update(self, features):
        """features: f32 [B, d] on the GPU, any B (0 included), a row-strided view allowed.  One launch; no host synchronisation."""
        self._refuse_given("update")
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"FeatureStats.update: features is [B, {self.dim}], got {tuple(getattr(features, 'shape', ()))}")
        ops.moments_f64_(features, self.sum, self.outer)
        self.n += int(features.shape[0])
        return self

    def merge(self, other):
        """add another accumulator of the same width (another shard's or another rank's): the three sums add"""
        self._refuse_given("merge")
        if not isinstance(other, FeatureStats) or other.dim != self.dim:
            raise ValueError(f"FeatureStats.merge: other is a FeatureStats of width {self.dim}")
        other._refuse_given("merge")
        self.sum += other.sum.to(self.sum.device)
        self.outer += other.outer.to(self.outer.device)
        self.n += other.n
        return self

    def tensors(self):
        """(sum, outer): what a collective has to add across ranks, next to `n` (INTEGRATION.md has the three lines)"""
        self._refuse_given("tensors")
        return self.sum, self.outer

    def to(self, device):
        if self._given is None:
            self.sum, self.outer = self.sum.to(device), self.outer.to(device)
        return self

    # ---- host values ----------------------------------------------------------------------------------------------------------------
    def _host(self):
        s, o = self.sum.cpu().numpy(), self.outer.cpu().numpy()
        return s, np.triu(o) + np.triu(o, 1).T                     # the lower triangle mirrored from the upper one

    def mean(self):
        """-> numpy f64 [d]"""
        if self._given is not None:
            return self._given[0].copy()
        if self.n < 1:
            raise ValueError("FeatureStats.mean: no features yet")
        return self.sum.cpu().numpy() / self.n

    def cov(self):
        """-> numpy f64 [d, d]: (outer_sym - n mu mu^T) / (n - 1), np.cov(features, rowvar=False)'s definition (one-pass centring: the
        cancellation is bounded in DESIGN.md section 5l)"""
        if self._given is not None:
            return self._given[1].copy()
        if self.n < 2:
            raise ValueError(f"FeatureStats.cov: the covariance needs at least two feature rows, got n = {self.n}")
        s, o = self._host()
        mu = s / self.n
        return (o - self.n * np.outer(mu, mu)) / (self.n - 1)

    # ---- files ----------------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """one .npz: `n`, `sum`, `outer` (the accumulators as they are: lossless, mergeable) and `mu`, `sigma` (the key names other
        Frechet-distance tools use for precomputed statistics; sigma only when n >= 2)"""
        self._refuse_given("save")
        arrays = dict(n=np.int64(self.n), sum=self.sum.cpu().numpy(), outer=self.outer.cpu().numpy())
        if self.n >= 1:
            arrays["mu"] = self.mean()
        if self.n >= 2:
            arrays["sigma"] = self.cov()
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device="cpu"):
        """a file written by `save`, from its `n`, `sum` and `outer`; needs no GPU (`device="cuda"` to go on updating)"""
        with np.load(path) as z:
            missing = [k for k in ("n", "sum", "outer") if k not in z.files]
            if missing:
                raise ValueError(f"FeatureStats.load: {path} has no {missing}: not a file written by FeatureStats.save")
            n, s, o = int(z["n"]), z["sum"], z["outer"]
        if s.dtype != np.float64 or o.dtype != np.float64 or s.ndim != 1 or o.shape != (s.shape[0], s.shape[0]) or n < 0:
            raise ValueError(f"FeatureStats.load: {path}: sum f64 [d] and outer f64 [d, d] expected, got {s.dtype} {s.shape} and {o.dtype} {o.shape}")
        st = cls(s.shape[0], "cpu")
        st.n, st.sum, st.outer = n, torch.from_numpy(s.copy()), torch.from_numpy(o.copy())
        return st.to(device)

    @classmethod
    def from_moments(cls, n, mean, cov):
        """statistics given as (n, mean [d], cov [d, d]) - someone else's precomputed `mu` / `sigma`.  `mean()` and `cov()` return them as
        given; they cannot be updated or merged into.  Needs no GPU."""
        mu, sigma = _as_f64(mean), _as_f64(cov)
        if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
            raise ValueError(f"FeatureStats.from_moments: mean [d] and cov [d, d], got {mu.shape} and {sigma.shape}")
        st = cls.__new__(cls)
        st.dim, st.n, st.sum, st.outer, st._given = int(mu.shape[0]), int(n), None, None, (mu.copy(), sigma.copy())
        return st


def _as_f64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _moments(x, which):
    if isinstance(x, FeatureStats):
        return x.mean(), x.cov()
    try:
        mu, sigma = x
    except (TypeError, ValueError):
        raise ValueError(f"frechet_distance: {which} is a FeatureStats or a (mu, sigma) pair") from None
    mu, sigma = _as_f64(mu), _as_f64(sigma)
    if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"frechet_distance: {which} is (mu [d], sigma [d, d]), got {mu.shape} and {sigma.shape}")
    return mu, sigma


def frechet_distance(a, b) -> float:
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr sqrt(S_a S_b) of two FeatureStats or (mu, sigma) pairs, on the host in f64.

    The last term goes the symmetric way: A = sqrt(S_a) through `eigh` (negative eigenvalues set to 0), then tr sqrt(S_a S_b) = the sum
    of the square roots of the eigenvalues of the symmetric A S_b A (`eigvalsh`, negative ones set to 0): S_a S_b and A S_b A have the
    same spectrum.  No epsilon on the diagonal for singular covariances (n < d) and nothing ever goes complex.  A S_b A is formed in
    the eigenbasis V of S_a with the eigenvalues descending, V^T (A S_b A) V = L^1/2 (V^T S_b V) L^1/2 (an orthogonal similarity: the
    same eigenvalues): the null directions of S_a are then rows and columns that are (nearly) zero at the END of a graded matrix, and
    `eigvalsh` resolves the small eigenvalues to their own size, not to eps |A S_b A| - whose square root, 1e-8 of the largest
    eigenvalue per null direction, the dense form would add to the distance of rank-deficient statistics.

    The RAW value is returned: for equal inputs it may come out a few ulps of the traces below zero.  It is not clamped - a caller who
    wants max(d, 0) writes it, and a distinctly negative value shows broken statistics instead of hiding them."""
    (mua, sa), (mub, sb) = _moments(a, "a"), _moments(b, "b")
    if mua.shape != mub.shape:
        raise ValueError(f"frechet_distance: the two feature widths differ: {mua.shape[0]} and {mub.shape[0]}")
    w, v = np.linalg.eigh(sa)
    w, v = w[::-1], v[:, ::-1]
    root = np.sqrt(np.clip(w, 0.0, None))
    ev = np.linalg.eigvalsh((v.T @ sb @ v) * root[:, None] * root[None, :])
    cross = np.sqrt(np.clip(ev, 0.0, None)).sum()
    diff = mua - mub
    return float(diff @ diff + np.trace(sa) + np.trace(sb) - 2.0 * cross)


__all__ = ["FeatureStats", "frechet_distance"]
