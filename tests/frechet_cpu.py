"""CPU side of the Frechet-distance tests (tests/test_frechet_cpu.py, tests/test_gpu_frechet.py): the golden cases of
tests/golden/frechet_golden.npz (written by tests/golden/make_golden_frechet.py with scipy.linalg.sqrtm and the published formula), a
second oracle in numpy, the tolerances with their reasons, and the float64 / int64 references of muse_moments_f64.
Everything returned from a cached function is shared between tests and never modified."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frechet_golden.npz")
FULL_RANK = [(16, 64), (48, 192), (80, 320)]                  # (D, N)
RANK_DEFICIENT = [(48, 30)]                                   # N - 1 < D: 19 null directions
CASES = FULL_RANK + RANK_DEFICIENT
EPS = 2.0 ** -53                                              # unit roundoff of f64

# Full rank: scipy's sqrtm route, the eigvals route and the symmetric route agree to 3e-14 .. 1.6e-13 relative on these shapes (1.6e-12 at
# (512, 2048)); 1e-10 is about 500 x that spread, leaves room for the kernel's summation order in the GPU variant, and is still six orders
# tighter than any indexing or centring mistake.
RTOL_FULL = 1e-10
# Rank deficient: the two REFERENCES differ from each other by 2e-9 .. 7e-9 relative here - an eigenvalue that should be 0 comes out as
# +-eps |S_a S_b|, and its square root is 1e-8 of the largest eigenvalue, once per null direction.
RTOL_DEFICIENT = 1e-6


def rtol(d, n):
    return RTOL_FULL if n - 1 >= d else RTOL_DEFICIENT


def unpack_triu(t, d):
    s = np.zeros((d, d), dtype=np.float64)
    s[np.triu_indices(d)] = t
    return s + np.triu(s, 1).T


@functools.lru_cache(maxsize=None)
def golden(d, n):
    """-> dict(xa, xb f32 [n, d]; mua, mub f64 [d]; sa, sb f64 [d, d]; distance float)"""
    with np.load(GOLDEN) as z:
        k = f"d{d}_n{n}"
        out = dict(xa=z[k + "_xa"], xb=z[k + "_xb"], mua=z[k + "_mua"], mub=z[k + "_mub"], sa=unpack_triu(z[k + "_sigmaa_triu"], d),
                   sb=unpack_triu(z[k + "_sigmab_triu"], d), distance=float(z[k + "_distance"]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_distance(mua, sa, mub, sb):
    """the second oracle: tr sqrt(Sa Sb) = sum sqrt(clip(eigvals(Sa Sb).real, 0))"""
    ev = np.linalg.eigvals(sa @ sb).real
    diff = mua - mub
    return float(diff @ diff + np.trace(sa) + np.trace(sb) - 2.0 * np.sqrt(np.clip(ev, 0.0, None)).sum())


def identity_bound(sa):
    """|d(a, a)| <= 1e-9 (tr Sa + tr Sa)"""
    return 1e-9 * 2.0 * float(np.trace(sa))


def close(got, want, tol):
    return abs(got - want) <= tol * abs(want)


# ---- muse_moments_f64 -----------------------------------------------------------------------------------------------------------------
def int_features(n, d, seed):
    """integers in [-3, 3] as f32: every sum of products is an integer far below 2^53, exact in any order"""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, d)).astype(np.float32)


def int_moments(x):
    """-> (sum f64 [d], outer f64 [d, d]) through int64: the exact values"""
    xi = x.astype(np.int64)
    assert np.array_equal(xi.astype(np.float32), x)
    return xi.sum(0).astype(np.float64), (xi.T @ xi).astype(np.float64)


def f64_moments(x):
    """-> (sum, outer, sum of |x|, sum of |x_i| |x_j|) in numpy f64 on the converted inputs"""
    x = x.astype(np.float64)
    a = np.abs(x)
    return x.sum(0), x.T @ x, a.sum(0), a.T @ a


def moments_bound(n_total, calls, abs_outer):
    """elementwise bound of the kernel's error against the f64 reference: the products are exact, so the value is a sum of n_total exact
    terms onto the accumulator's initial 0 - at most n_total roundings in the kernel (one per addition, whatever the MFMA's order inside
    a group of four), `calls` more where a call's partial result is added onto the previous one, and numpy's own pairwise sum adds its
    few; (n_total + calls + 4) 2^-53 sum_n |x_ni| |x_nj| covers both to first order (the issue's bound, derived, not measured)"""
    return (n_total + calls + 4) * EPS * abs_outer


def cov_bound(x):
    """bound of |cov - np.cov| for the one-pass (outer - n mu mu^T) / (n - 1): both terms of the difference are O(sum_n x_ni^2) and each
    carries O(n) roundings of 2^-53 relative, so the cancellation leaves at most 64 n 2^-53 max_i sum_n x_ni^2 / (n - 1); the same
    quantity / n bounds the mean's error with room to spare"""
    x = x.astype(np.float64)
    n = x.shape[0]
    return 64.0 * n * EPS * float((x * x).sum(0).max()) / (n - 1)
