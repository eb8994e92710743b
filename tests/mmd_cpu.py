"""CPU side of the MMD tests (tests/test_mmd_cpu.py, tests/test_gpu_mmd.py): the golden cases of tests/golden/mmd_golden.npz (written by
tests/golden/make_golden_mmd.py from explicit differences in np.longdouble), the numpy f64 oracle in the expansion form the kernel
computes, and the error bound with its derivation.  Everything returned from a cached function is shared between tests and never modified."""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mmd_golden.npz")
CASES = [(16, 40, 56), (48, 96, 64), (768, 24, 17)]           # (d, n, m)
SIGMA, SCALE = 10.0, 1000.0                                   # CMMD's constants: the golden sums are made with them, on normalised rows
GAMMA = 1.0 / (2.0 * SIGMA ** 2)
U = 2.0 ** -53                                                # unit roundoff of f64
TILE, FIN = 64, 1024                                          # csrc/mmd.hip: pairs per tile side, threads of the finalize workgroup


@functools.lru_cache(maxsize=None)
def golden(d, n, m):
    """-> dict(xa f32 [n, d], xb f32 [m, d]; sxx, syy (all pairs, diagonal included), sxx_off, syy_off (i != j), sxy; distance (the
    V-statistic x 1000), distance_unbiased) - sums of exp(-|x^ - y^|^2 / 200) over L2-normalised rows, longdouble rounded to f64"""
    with np.load(GOLDEN) as z:
        k = f"d{d}_n{n}_m{m}_"
        out = {name: z[k + name] for name in ("xa", "xb")}
        out.update({name: float(z[k + name]) for name in ("sxx", "syy", "sxx_off", "syy_off", "sxy", "distance", "distance_unbiased")})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def rinv(x):
    """1 / sqrt(sum_k x_ik^2) in f64"""
    x = x.astype(np.float64)
    return 1.0 / np.sqrt((x * x).sum(1))


def sqdist(x, y, rx=None, ry=None):
    """-> (T, W): T[i][j] = (a_i + b_j) - 2 c_ij, the squared distance in the expansion form the kernel computes, in numpy f64, and
    W[i][j] = a_i + b_j + 2 rx_i ry_j sum_k |x_ik| |y_jk|, the magnitude its roundings are relative to"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    rx = np.ones(len(x)) if rx is None else rx
    ry = np.ones(len(y)) if ry is None else ry
    a, b = (rx * rx) * (x * x).sum(1), (ry * ry) * (y * y).sum(1)
    scale = rx[:, None] * ry[None, :]
    return (a[:, None] + b[None, :]) - 2.0 * (scale * (x @ y.T)), a[:, None] + b[None, :] + 2.0 * scale * (np.abs(x) @ np.abs(y).T)


def oracle(x, y, gamma, rx=None, ry=None):
    """the numpy f64 oracle: -> (K, W) with K[i][j] = exp(-gamma T[i][j]) and W of `sqdist`"""
    t, w = sqdist(x, y, rx, ry)
    return np.exp(-gamma * t), w


def exact_sum(values):
    """the correctly rounded sum (math.fsum): the reference side adds ONE rounding, whatever the number of terms"""
    return math.fsum(np.asarray(values, dtype=np.float64).ravel().tolist())


def tiles(n, m, symmetric):
    tn, tm = -(-n // TILE), -(-(n if symmetric else m) // TILE)
    return tn * (tn + 1) // 2 if symmetric else tn * tm


def chain(n, m, symmetric):
    """A, the longest chain of additions a kernel value goes through in csrc/mmd.hip, read off its reduction: a lane adds its 16 values
    (16), a wave's butterfly (6), the finalize thread adds ceil(P / 1024) partials for P = 4 * tiles, and the LDS tree (10); + 1 for the
    one rounding of the reference's math.fsum"""
    return 16 + 6 + -(-4 * tiles(n, m, symmetric) // FIN) + 10 + 1


def bound(k, w, gamma, d, a_chain, where=None):
    """|S - S_ref| <= sum_ij k_ij (2 gamma (d + 5) u w_ij + 4 u) + A u S over the pairs `where` selects (all by default).
    The products inside a dot product are exact and its terms enter by one rounding each: the dot product, the two squared norms and the
    few scalings and additions that form the squared distance are off by at most (d + 5) u relative to w_ij = a_i + b_j + 2 |c|_ij on
    each side, and d exp(-gamma t) = -gamma exp(-gamma t) dt; 4 u: two ulps each for the device's exp and libm's; all k_ij are positive,
    so the A additions of the reduction cost at most A u S to first order."""
    k, w = (k, w) if where is None else (k[where], w[where])
    return float((k * (2.0 * gamma * (d + 5) * U * w + 4.0 * U)).sum() + a_chain * U * k.sum())


def distance_bound(scale, n, m, txx, tyy, txy, unbiased=False):
    """scale (tol(Sxx) / n^2 + tol(Syy) / m^2 + 2 tol(Sxy) / (n m)); the unbiased form divides by n (n - 1) and m (m - 1)"""
    return scale * (txx / (n * (n - 1.0) if unbiased else float(n) * n) + tyy / (m * (m - 1.0) if unbiased else float(m) * m) + 2.0 * txy / (float(n) * m))


def case_bounds(d, n, m):
    """-> (tol(Sxx), tol(Syy), tol(Sxy)) of a golden case at CMMD's constants, for the FULL symmetric sums (2 upper + diagonal: twice the
    upper triangle's bound plus the diagonal's is the bound over all pairs)"""
    g = golden(d, n, m)
    ra, rb = rinv(g["xa"]), rinv(g["xb"])
    out = []
    for x, y, rx, ry, sym in ((g["xa"], g["xa"], ra, ra, True), (g["xb"], g["xb"], rb, rb, True), (g["xa"], g["xb"], ra, rb, False)):
        k, w = oracle(x, y, GAMMA, rx, ry)
        out.append(bound(k, w, GAMMA, d, chain(len(x), len(y), sym)))
    return tuple(out)
