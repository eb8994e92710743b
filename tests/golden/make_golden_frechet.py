"""Golden values for muse.frechet_distance and muse.FeatureStats, from numpy and scipy alone (scipy 1.15):

    python tests/golden/make_golden_frechet.py

Per case (D, N): two sets of N correlated-Gaussian feature rows in f32 (different means, different mixing matrices), the f64 mean and
covariance of each from np.mean / np.cov(rowvar=False) on the rows converted to f64, and the Frechet distance by the published formula
(Heusel et al. 2017, as the common FID tools compute it):

    d = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2)

with scipy.linalg.sqrtm, the tools' fallback of adding 1e-6 to both diagonals when the root comes out non-finite, and the real part of a
complex root.  Cases: three of full rank, (16, 64), (48, 192), (80, 320), and one rank-deficient, (48, 30): N - 1 = 29 < D.

To keep the file small the features are multiples of 1/8 (still f32, still correlated Gaussians up to that rounding: it adds 1/768 to
every variance), which deflate packs well, and each covariance is stored as its upper triangle in row-major order (`sigma*_triu`,
np.triu_indices(D)); np.cov's result is exactly symmetric, which is asserted here.  Output: tests/golden/frechet_golden.npz."""
import os

import numpy as np
from scipy import linalg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((16, 64), (48, 192), (80, 320), (48, 30))          # (D, N)
SEED = 20251


def features(rng, d, n, shift):
    mix = rng.standard_normal((d, d)) / np.sqrt(d) + 0.5 * np.eye(d)
    x = rng.standard_normal((n, d)) @ mix + shift * rng.standard_normal(d)
    return (np.round(x * 8.0) / 8.0).astype(np.float32)


def published(mu1, s1, mu2, s2, eps=1e-6):
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(s1.shape[0]) * eps
        covmean = linalg.sqrtm((s1 + offset).dot(s2 + offset))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(covmean))


def main():
    rng = np.random.default_rng(SEED)
    out = dict(cases=np.asarray(CASES, dtype=np.int64))
    for d, n in CASES:
        key = f"d{d}_n{n}"
        stats = []
        for which, shift in (("a", 0.25), ("b", 0.5)):
            x = features(rng, d, n, shift)
            x64 = x.astype(np.float64)
            mu, sigma = np.mean(x64, axis=0), np.cov(x64, rowvar=False)
            assert np.array_equal(sigma, sigma.T)
            out[f"{key}_x{which}"], out[f"{key}_mu{which}"], out[f"{key}_sigma{which}_triu"] = x, mu, sigma[np.triu_indices(d)]
            stats += [mu, sigma]
        out[f"{key}_distance"] = np.float64(published(*stats))
        print(key, "distance", out[f"{key}_distance"], "traces", np.trace(stats[1]), np.trace(stats[3]))
    path = os.path.join(HERE, "frechet_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
