"""Writes tests/golden/mmd_golden.npz: small f32 feature sets and the sums of the Gaussian kernel over their L2-normalised rows at CMMD's
constants (sigma = 10), computed by EXPLICIT DIFFERENCES in np.longdouble - sum_k (x^_ik - y^_jk)^2, no dot-product expansion - an
independent route to what csrc/mmd.hip and the numpy oracle of tests/mmd_cpu.py get from (a + b) - 2 c.

    python tests/golden/make_golden_mmd.py
"""
import os

import numpy as np

CASES = [(16, 40, 56), (48, 96, 64), (768, 24, 17)]           # (d, n, m)
SIGMA, SCALE = 10.0, 1000.0
LD = np.longdouble


def features(d, n, m, seed):
    """two sets with a common direction and different spreads, so that the distance is well away from zero"""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(d)
    xa = (centre + 0.7 * rng.standard_normal((n, d))).astype(np.float32)
    xb = (centre + 0.4 * rng.standard_normal(d) + 1.1 * rng.standard_normal((m, d))).astype(np.float32)
    return xa, xb


def kernel_matrix(x, y):
    """K[i][j] = exp(-|x_i / |x_i| - y_j / |y_j||^2 / (2 sigma^2)) in longdouble, from the differences"""
    x, y = x.astype(LD), y.astype(LD)
    x = x / np.sqrt((x * x).sum(1))[:, None]
    y = y / np.sqrt((y * y).sum(1))[:, None]
    diff = x[:, None, :] - y[None, :, :]
    return np.exp(-(diff * diff).sum(2) / (LD(2) * LD(SIGMA) ** 2))


def main():
    assert np.finfo(LD).nmant > 60, "np.longdouble is not wider than f64 here"
    out = {}
    for d, n, m in CASES:
        xa, xb = features(d, n, m, 1000 * d + n)
        kxx, kyy, kxy = kernel_matrix(xa, xa), kernel_matrix(xb, xb), kernel_matrix(xa, xb)
        sxx, syy, sxy = kxx.sum(), kyy.sum(), kxy.sum()
        sxx_off, syy_off = sxx - np.trace(kxx), syy - np.trace(kyy)
        n_, m_ = LD(n), LD(m)
        v = LD(SCALE) * (sxx / (n_ * n_) + syy / (m_ * m_) - 2 * sxy / (n_ * m_))
        u = LD(SCALE) * (sxx_off / (n_ * (n_ - 1)) + syy_off / (m_ * (m_ - 1)) - 2 * sxy / (n_ * m_))
        k = f"d{d}_n{n}_m{m}_"
        out[k + "xa"], out[k + "xb"] = xa, xb
        for name, value in (("sxx", sxx), ("syy", syy), ("sxx_off", sxx_off), ("syy_off", syy_off), ("sxy", sxy), ("distance", v),
                            ("distance_unbiased", u)):
            out[k + name] = np.float64(value)
        print(f"d {d} n {n} m {m}: sxx / n^2 {float(sxx / (n_ * n_)):.6f} distance {float(v):.6f} unbiased {float(u):.6f}")
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mmd_golden.npz"), **out)


if __name__ == "__main__":
    main()
