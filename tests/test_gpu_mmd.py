"""GPU (MI355X): muse_row_norms_f64 and muse_rbf_pair_sums_f64 (csrc/mmd.hip) through the raw C-ABI - exact pair counts and group
probes at every edge of the 64 x 64 tile, the 16-row wave strip and the 16-feature step, general values within the derived bound - then
muse.mmd_distance / muse.cmmd_distance on kernel-built sums against the longdouble golden, and muse.FeatureBank with the CLIPScorer surface
that feeds it.  tests/mmd_cpu.py holds the golden cases, the numpy oracle and the bound with its derivation.

Every kernel case: the features sit inside a larger allocation with NaN before and after them and in every ld > d gap (a read outside the
rows' first d columns poisons the sums); the f64 outputs and the workspace sit in one allocation pre-filled with a NaN bit pattern no
result has, with guard bands on both sides and between them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import clip_vision_cpu as CV
import mmd_cpu as MC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FF85EA71E5EA7ED                                     # a quiet NaN with a payload no computation produces
GUARD = 32
ERR_BAD_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3
SIZES = [1, 15, 16, 17, 63, 64, 65, 129]
PAIRS = [(1, 1), (1, 129), (65, 63), (129, 129), (15, 17), (17, 15), (16, 64), (64, 16), (63, 65), (129, 1), (64, 64)]


def _lib():
    from muse import _hip
    return _hip.lib()


def _stream():
    from muse import _hip
    return _hip.stream()


class X:
    """f32 [n, d] rows at stride ld inside a NaN-filled allocation; .ptr is 16-byte aligned"""

    def __init__(self, x, ld=None):
        n, d = x.shape
        self.n, self.d, self.ld = n, d, d if ld is None else ld
        size = max(n - 1, 0) * self.ld + d
        host = torch.full((GUARD + size + GUARD,), float("nan"), dtype=torch.float32)
        if n:
            host[GUARD:GUARD + size].as_strided((n, d), (self.ld, 1)).copy_(torch.from_numpy(np.ascontiguousarray(x)))
        self.t = host.to(DEV)
        self.ptr = self.t.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0


class F64:
    """f64 segments of the given lengths in one sentinel-filled allocation: guard | seg 0 | guard | seg 1 | guard ..."""

    def __init__(self, *lengths):
        self.at, pos = [], GUARD
        for n in lengths:
            self.at.append((pos, n))
            pos += n + GUARD
        self.t = torch.full((pos,), SENT, dtype=torch.int64).to(DEV)

    def ptr(self, i):
        return self.t.data_ptr() + 8 * self.at[i][0]

    def read(self, what):
        """-> the segments as numpy f64, after checking the guard bands"""
        host, pos, out = self.t.cpu(), 0, []
        for lo, n in self.at:
            assert bool((host[pos:lo] == SENT).all()), f"{what}: a guard band was written"
            out.append(host[lo:lo + n].view(torch.float64).numpy().copy())
            pos = lo + n
        assert bool((host[pos:] == SENT).all()), f"{what}: the last guard band was written"
        return out

    def untouched(self, what):
        assert bool((self.t.cpu() == SENT).all()), f"{what}: a refused call wrote to its outputs"


def dev_f64(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV)


def pair_sums(x, y, gamma, rx=None, ry=None, ldx=None, ldy=None, what=""):
    """one muse_rbf_pair_sums_f64 call on numpy inputs (y None: the symmetric form) -> out as numpy f64 [2]"""
    xs, ys = X(x, ldx), (None if y is None else X(y, ldy))
    n, m = xs.n, (0 if ys is None else ys.n)
    count = _lib().muse_rbf_pair_sums_workspace(n, m, 1 if ys is None else 0)
    assert count == (8 if ys is None else 4) * MC.tiles(n, m, ys is None)
    buf = F64(2, count)
    rxd, ryd, g = dev_f64(rx), dev_f64(ry), ctypes.c_double(gamma)
    rc = _lib().muse_rbf_pair_sums_f64(xs.ptr, n, xs.ld, None if rxd is None else rxd.data_ptr(), None if ys is None else ys.ptr, m,
                                       0 if ys is None else ys.ld, None if ryd is None else ryd.data_ptr(), xs.d, ctypes.addressof(g),
                                       buf.ptr(1), buf.ptr(0), _stream())
    assert rc == 0, f"{what}: the entry returned {rc}"
    torch.cuda.synchronize()
    out, ws = buf.read(what)
    assert not np.isnan(ws).any() or np.isnan(out).any(), f"{what}: a workspace slot was never written"
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).tolist()


def normal(n, d, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(np.float32)


# ---- muse_row_norms_f64 ---------------------------------------------------------------------------------------------------------------
def row_norms(x, ld=None, want_rinv=True, what=""):
    xs = X(x, ld)
    buf = F64(xs.n, xs.n)
    rc = _lib().muse_row_norms_f64(xs.ptr, xs.n, xs.d, xs.ld, buf.ptr(0), buf.ptr(1) if want_rinv else None, _stream())
    assert rc == 0, f"{what}: the entry returned {rc}"
    torch.cuda.synchronize()
    if not want_rinv:
        sumsq = buf.read(what)[0]
        assert bool((buf.t.cpu()[buf.at[1][0]:] == SENT).all()), f"{what}: rinv was written without being asked for"
        return sumsq, None
    return tuple(buf.read(what))


@pytest.mark.parametrize("d", [4, 60, 64, 68, 256, 260, 768])
def test_row_norms_are_exact_on_integers_and_within_the_bound(d):
    """integers in [-3, 3]: the sum of squares is an integer, exact in any order (d around the 16-feature group, and around the 256
    features one pass of a wave covers); N(0, 1): a lane adds at most 4 ceil(d / 256) squares, the butterfly 6 more, numpy's pairwise sum
    its few: |err| <= (4 ceil(d / 256) + 6 + 8) u sumsq.  rinv against numpy's 1 / sqrt of the SAME sumsq: at most one ulp (2 u) each for the
    device's sqrt and quotient, half an ulp (u) each for numpy's - 6 u relative."""
    for n in (1, 3, 4, 5, 67):
        xi = np.random.default_rng(100 * d + n).integers(-3, 4, size=(n, d)).astype(np.float32)
        want = (xi.astype(np.int64) ** 2).sum(1).astype(np.float64)
        for ld in (d, d + 4):
            sumsq, none = row_norms(xi, ld, want_rinv=False, what=f"integers n {n} d {d} ld {ld}")
            assert none is None and bits(sumsq) == bits(want), (n, d, ld)
        x = normal(n, d, 7 * d + n)
        sumsq, rinv = row_norms(x, d + 8, what=f"normal n {n} d {d}")
        ref = (x.astype(np.float64) ** 2).sum(1)
        assert (np.abs(sumsq - ref) <= (4 * -(-d // 256) + 14) * MC.U * ref).all()
        with np.errstate(divide="ignore"):
            assert (np.abs(rinv - 1.0 / np.sqrt(sumsq)) <= 6 * MC.U / np.sqrt(sumsq)).all()
    zero = normal(3, d, 1)
    zero[1] = 0.0
    sumsq, rinv = row_norms(zero, what="a zero row")
    assert sumsq[1] == 0.0 and np.isposinf(rinv[1]) and np.isfinite(rinv[[0, 2]]).all()    # inf, as documented: not guarded


# ---- 1. pair counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 60, 64, 68])
def test_pair_counts_are_exact(d):
    """gamma = 0: every k_ij = exp(-0 t) = 1 for finite t, so the sums COUNT the pairs - n m, n (n - 1) / 2 and n, integers, compared on
    their bits.  A padded row or column counted as a pair, or a real one dropped, changes the count."""
    for n, m in PAIRS:
        x, y = normal(n, d, n * 131 + d), normal(m, d, m * 137 + d + 1)
        for ldx, ldy in ((d, d), (d + 4, d + 8)):
            out = pair_sums(x, y, 0.0, ldx=ldx, ldy=ldy, what=f"count n {n} m {m} d {d}")
            assert bits(out) == bits([float(n * m), 0.0]), (n, m, d, out)
    for n in SIZES:
        x = normal(n, d, n * 139 + d)
        out = pair_sums(x, None, 0.0, ldx=d + 4, what=f"symmetric count n {n} d {d}")
        assert bits(out) == bits([n * (n - 1) / 2.0, float(n)]), (n, d, out)
        assert bits(pair_sums(x, x, 0.0, what="y = x")) == bits([float(n * n), 0.0])       # 4.: 2 upper + diagonal = the rectangle


# ---- 2. group probes ------------------------------------------------------------------------------------------------------------------
def one_hot(groups, d, shift=None):
    """rows 64 e_g (divided by 2^shift_i, exactly)"""
    x = np.zeros((len(groups), d), dtype=np.float32)
    x[np.arange(len(groups)), groups] = 64.0 if shift is None else 64.0 / 2.0 ** shift
    return x


@pytest.mark.parametrize("scaled", [False, True])
def test_group_probes_are_exact(scaled):
    """x_i = 64 e_g(i), y_j = 64 e_h(j), gamma = 1: a pair of one group has squared distance exactly 0 and k = 1, any other 8192 and
    k = exp(-8192) = 0.0 exactly - the sums count the same-group pairs.  A pair taken from the wrong row, column or k position changes
    the count.  `scaled`: rx, ry are powers of two and the features are divided by them - the same integers."""
    n, m, d = 65, 129, 68
    g, h = np.arange(n) % d, (7 * np.arange(m) + 3) % d
    sx, sy = (np.arange(n) % 5 - 2, np.arange(m) % 7 - 3) if scaled else (None, None)
    rx, ry = (2.0 ** sx, 2.0 ** sy) if scaled else (None, None)
    want = float(sum(int((g == k).sum()) * int((h == k).sum()) for k in range(d)))
    out = pair_sums(one_hot(g, d, sx), one_hot(h, d, sy), 1.0, rx, ry, ldx=d + 4, what="groups, rectangular")
    assert want > 0 and bits(out) == bits([want, 0.0]), (out, want)
    n = 129
    g = np.arange(n) % d
    sx = np.arange(n) % 5 - 2 if scaled else None
    rx = 2.0 ** sx if scaled else None
    same = g[:, None] == g[None, :]
    want = float(np.triu(same, 1).sum())
    x = one_hot(g, d, sx)
    out = pair_sums(x, None, 1.0, rx, what="groups, symmetric")
    assert want == 61 and bits(out) == bits([want, float(n)]), (out, want)
    assert bits(pair_sums(x, x, 1.0, rx, rx, what="groups, y = x")) == bits([2 * want + n, 0.0])      # 4.


# ---- 3. general values ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case(n, m, d, scale, normalize):
    """-> (x, y, rx, ry, gamma, T, W): N(0, 1) * scale features (y None when m == 0: symmetric), gamma such that gamma T spans 0 .. 20"""
    x = normal(n, d, n + 3 * m + d, scale)
    y = normal(m, d, n + 3 * m + d + 1, scale) if m else None
    rx, ry = (MC.rinv(x), None if y is None else MC.rinv(y)) if normalize else (None, None)
    t, w = MC.sqdist(x, x if y is None else y, rx, rx if y is None else ry)
    return x, y, rx, ry, 20.0 / float(t.max()), t, w


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("scale", [1e-2, 1.0, 1e2])
@pytest.mark.parametrize("n,m,d", [(67, 130, 68), (5, 3, 768), (129, 0, 132)])
def test_general_values_within_the_derived_bound(n, m, d, scale, normalize):
    """against the numpy f64 oracle (summed by math.fsum), within mmd_cpu.bound - computed from the inputs, with A read off the kernel's
    reduction (mmd_cpu.chain).  m = 0 stands for the symmetric form of the n rows; there the upper triangle and the diagonal are held
    to their own bounds, and 2 upper + diagonal to the rectangular call with y = x (4.)."""
    x, y, rx, ry, gamma, t, w = general_case(n, m, d, scale, normalize)
    k = np.exp(-gamma * t)
    what = f"general n {n} m {m} d {d} scale {scale:g} normalize {normalize}"
    if y is not None:
        out = pair_sums(x, y, gamma, rx, ry, ldx=d + 4, what=what)
        ref, tol = MC.exact_sum(k), MC.bound(k, w, gamma, d, MC.chain(n, m, False))
        print(f"{what}: got {out[0]!r} oracle {ref!r} err / bound {abs(out[0] - ref) / tol:.4f}")
        assert abs(out[0] - ref) <= tol and out[1] == 0.0
        return
    out = pair_sums(x, None, gamma, rx, ldx=d + 4, what=what)
    a = MC.chain(n, n, True)
    upper, diag = np.triu(np.ones((n, n), dtype=bool), 1), np.eye(n, dtype=bool)
    tol_u, tol_d = MC.bound(k, w, gamma, d, a, upper), MC.bound(k, w, gamma, d, a, diag)
    ref_u, ref_d = MC.exact_sum(k[upper]), MC.exact_sum(k[diag])
    print(f"{what}: upper err / bound {abs(out[0] - ref_u) / tol_u:.4f}, diagonal err / bound {abs(out[1] - ref_d) / tol_d:.4f}")
    assert abs(out[0] - ref_u) <= tol_u and abs(out[1] - ref_d) <= tol_d
    rect = pair_sums(x, x, gamma, rx, rx, what=what + " y = x")
    tol_r = MC.bound(k, w, gamma, d, MC.chain(n, n, False))
    assert abs(rect[0] - MC.exact_sum(k)) <= tol_r
    assert abs((2.0 * out[0] + out[1]) - rect[0]) <= 2.0 * tol_u + tol_d + tol_r


# ---- 5. equal calls, equal bits -------------------------------------------------------------------------------------------------------
def test_equal_calls_give_equal_bits():
    n, m, d = 67, 130, 68
    x, y = normal(n, d, 1), normal(m, d, 2)
    rx, ry = MC.rinv(x), MC.rinv(y)
    first = pair_sums(x, y, 3.0, rx, ry, what="first")
    assert bits(pair_sums(x, y, 3.0, rx, ry, what="second")) == bits(first)
    assert bits(pair_sums(x, y, 3.0, rx, ry, ldx=d + 4, ldy=d + 12, what="strided")) == bits(first)
    sym = pair_sums(y, None, 3.0, ry, what="symmetric")
    assert bits(pair_sums(y, None, 3.0, ry, ldx=d + 8, what="symmetric, strided")) == bits(sym)
    gamma = 0.05
    plain = pair_sums(x, y, gamma, what="NULL scales")
    assert bits(pair_sums(x, y, gamma, np.ones(n), np.ones(m), what="ones")) == bits(plain)
    assert bits(pair_sums(x, y, gamma, None, np.ones(m), what="ones for y")) == bits(plain)
    assert bits(pair_sums(x, None, gamma, np.ones(n), what="ones, symmetric")) == bits(pair_sums(x, None, gamma, what="NULL, symmetric"))
    assert 0.0 < plain[0] < n * m


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    n, m, d = 5, 7, 68
    xv, yv = normal(n, d, 3), normal(m, d, 4)
    x, y, odd = X(xv), X(yv), X(xv, d + 4)
    r = dev_f64(np.ones(16))
    g = ctypes.c_double(0.5)
    fresh = pair_sums(xv, yv, 0.5, what="fresh")
    base = dict(x=x.ptr, n=n, ldx=d, rx=None, y=y.ptr, m=m, ldy=d, ry=None, d=d, gamma=ctypes.addressof(g))
    big = 64 * 46341                                            # 46341^2 tiles > 2^31 - 1
    cases = [("d = 0", ERR_BAD_ARG, dict(d=0)), ("d < 0", ERR_BAD_ARG, dict(d=-4)), ("d % 4", ERR_BAD_ARG, dict(d=66, ldx=68, ldy=68)),
             ("n < 0", ERR_BAD_ARG, dict(n=-1)), ("m < 0", ERR_BAD_ARG, dict(m=-1)), ("ldx < d", ERR_BAD_ARG, dict(ldx=d - 4)),
             ("ldy < d", ERR_BAD_ARG, dict(ldy=d - 4)), ("x NULL", ERR_BAD_ARG, dict(x=None)), ("gamma NULL", ERR_BAD_ARG, dict(gamma=None)),
             ("workspace NULL", ERR_BAD_ARG, dict(ws=None)), ("out NULL", ERR_BAD_ARG, dict(out=None)),
             ("x 4 bytes off", ERR_ALIGN, dict(x=x.ptr + 4)), ("x 8 bytes off", ERR_ALIGN, dict(x=x.ptr + 8)),
             ("y 4 bytes off", ERR_ALIGN, dict(y=y.ptr + 4)), ("ldx % 4", ERR_ALIGN, dict(ldx=d + 2)), ("ldy % 4", ERR_ALIGN, dict(ldy=d + 1)),
             ("rx 4 bytes off", ERR_ALIGN, dict(rx=r.data_ptr() + 4)), ("ry 4 bytes off", ERR_ALIGN, dict(ry=r.data_ptr() + 4)),
             ("workspace 4 bytes off", ERR_ALIGN, dict(ws="+4")), ("out 4 bytes off", ERR_ALIGN, dict(out="+4")),
             ("too many tiles", ERR_UNSUPPORTED, dict(n=big, m=big)), ("too many tiles, symmetric", ERR_UNSUPPORTED, dict(n=2 * big, y=None))]
    kept = []                                                   # outputs of refused calls stay alive until the device is idle
    count = _lib().muse_rbf_pair_sums_workspace(n, m, 0)
    for what, code, kw in cases:
        buf = F64(2, 2 * count)
        kept.append(buf)
        a = dict(base, ws=buf.ptr(1), out=buf.ptr(0))
        a.update({k: (a[k] + 4 if v == "+4" else v) for k, v in kw.items()})
        rc = _lib().muse_rbf_pair_sums_f64(a["x"], a["n"], a["ldx"], a["rx"], a["y"], a["m"], a["ldy"], a["ry"], a["d"], a["gamma"], a["ws"],
                                           a["out"], _stream())
        assert rc == code, f"{what}: the entry returned {rc}, not {code}"
    norms = F64(n, n)
    for what, code, kw in [("d = 0", ERR_BAD_ARG, dict(d=0)), ("d % 4", ERR_BAD_ARG, dict(d=66)), ("n < 0", ERR_BAD_ARG, dict(n=-1)),
                           ("ld < d", ERR_BAD_ARG, dict(ld=d - 4)), ("x NULL", ERR_BAD_ARG, dict(x=None)), ("sumsq NULL", ERR_BAD_ARG, dict(sumsq=None)),
                           ("x 4 bytes off", ERR_ALIGN, dict(x=x.ptr + 4)), ("ld % 4", ERR_ALIGN, dict(ld=d + 2)),
                           ("sumsq 4 bytes off", ERR_ALIGN, dict(sumsq=norms.ptr(0) + 4)), ("rinv 4 bytes off", ERR_ALIGN, dict(rinv=norms.ptr(1) + 4)),
                           ("too many rows", ERR_UNSUPPORTED, dict(n=2 ** 33))]:
        a = dict(x=x.ptr, n=n, d=d, ld=d, sumsq=norms.ptr(0), rinv=norms.ptr(1))
        a.update(kw)
        rc = _lib().muse_row_norms_f64(a["x"], a["n"], a["d"], a["ld"], a["sumsq"], a["rinv"], _stream())
        assert rc == code, f"row norms, {what}: the entry returned {rc}, not {code}"
    assert _lib().muse_row_norms_f64(x.ptr, 0, d, d, norms.ptr(0), norms.ptr(1), _stream()) == 0       # n == 0: success, nothing launched
    # n == 0 or m == 0: out = {0, 0}, the workspace untouched
    empties = []
    for kw in (dict(n=0), dict(m=0), dict(n=0, y=None)):
        buf = F64(2, 8)
        a = dict(base, ws=buf.ptr(1), out=buf.ptr(0))
        a.update(kw)
        assert _lib().muse_rbf_pair_sums_f64(a["x"], a["n"], a["ldx"], a["rx"], a["y"], a["m"], a["ldy"], a["ry"], a["d"], a["gamma"], a["ws"],
                                             a["out"], _stream()) == 0
        empties.append(buf)
    torch.cuda.synchronize()
    for (what, _, _), buf in zip(cases, kept):
        buf.untouched(what)
    norms.untouched("row norms")
    for buf in empties:
        out, ws = buf.read("an empty set")
        assert bits(out) == bits([0.0, 0.0]) and bool((ws.view(np.int64) == SENT).all())
    assert bits(pair_sums(xv, yv, 0.5, what="after the refusals")) == bits(fresh)
    assert odd.ld == d + 4                                      # (a stride that IS a multiple of 4 is taken: test_equal_calls_give_equal_bits)


def test_ops_wrappers_check_their_arguments():
    from muse import ops
    from muse._hip import MuseHipError
    good, other = torch.ones(3, 8, device=DEV), torch.ones(5, 8, device=DEV)
    wide = torch.ones(3, 10, device=DEV)
    r3 = torch.ones(3, dtype=torch.float64, device=DEV)
    for bad in (lambda: ops.row_norms_f64(good.double()), lambda: ops.row_norms_f64(good.t().contiguous().t()), lambda: ops.row_norms_f64(good.cpu()),
                lambda: ops.row_norms_f64(torch.ones(3, 6, device=DEV)), lambda: ops.row_norms_f64(wide[:, :8]), lambda: ops.row_norms_f64(good[0]),
                lambda: ops.rbf_pair_sums_f64(good.half(), other), lambda: ops.rbf_pair_sums_f64(good, other.double()),
                lambda: ops.rbf_pair_sums_f64(good, torch.ones(5, 12, device=DEV)), lambda: ops.rbf_pair_sums_f64(good, other.cpu()),
                lambda: ops.rbf_pair_sums_f64(wide[:, 1:9], other), lambda: ops.rbf_pair_sums_f64(good, other, rx=r3.float()),
                lambda: ops.rbf_pair_sums_f64(good, other, ry=r3), lambda: ops.rbf_pair_sums_f64(good, other, rx=r3.cpu()),
                lambda: ops.rbf_pair_sums_f64(good, None, ry=r3)):
        with pytest.raises(MuseHipError):
            bad()
    sumsq, rinv = ops.row_norms_f64(good)
    assert torch.equal(sumsq.cpu(), torch.full((3,), 8.0, dtype=torch.float64)) and bits(rinv.cpu().numpy()) == bits([1.0 / np.sqrt(8.0)] * 3)
    assert ops.row_norms_f64(good, want_rinv=False)[1] is None and ops.row_norms_f64(good[:0])[0].numel() == 0
    out = ops.rbf_pair_sums_f64(good, other, gamma=0.0, rx=r3)
    assert out.dtype == torch.float64 and out.is_cuda and out.tolist() == [15.0, 0.0]
    assert ops.rbf_pair_sums_f64(good, gamma=2.0).tolist() == [3.0, 3.0]                  # equal rows: squared distance exactly 0
    assert ops.rbf_pair_sums_f64(good[:0], other).tolist() == [0.0, 0.0]
    pad = torch.ones(3, 12, device=DEV)
    assert ops.rbf_pair_sums_f64(pad[:, 4:], other, gamma=0.0).tolist() == [15.0, 0.0]   # a view 16 bytes into a 48-byte row is fine


# ---- 7. no n x m allocation -----------------------------------------------------------------------------------------------------------
def test_the_distance_allocates_no_pair_matrix():
    """a condition, not a measurement: across one mmd_distance at n = m = 4096, d = 64, features resident, the peak of the allocator
    rises by less than 1 MiB - the partials of one call are 4 * 64^2 f64 = 128 KiB, the row norms 4 * 32 KiB; ONE materialised f64 term
    would be 128 MiB"""
    import muse
    gen = torch.Generator(device=DEV).manual_seed(0)
    a, b = torch.randn(4096, 64, device=DEV, generator=gen), torch.randn(4096, 64, device=DEV, generator=gen) + 0.1
    muse.mmd_distance(a[:8], b[:8])                             # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    value = muse.mmd_distance(a, b)
    rise = torch.cuda.max_memory_allocated() - before
    print(f"mmd_distance n = m = 4096 d = 64: {value!r}, allocator peak + {rise} bytes")
    assert rise < 2 ** 20 and value > 0.0


# ---- 8. distance level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,m", MC.CASES)
def test_distance_of_kernel_built_sums_meets_the_golden(d, n, m):
    import muse
    g = MC.golden(d, n, m)
    txx, tyy, txy = MC.case_bounds(d, n, m)
    tol, tol_u = MC.distance_bound(MC.SCALE, n, m, txx, tyy, txy), MC.distance_bound(MC.SCALE, n, m, txx, tyy, txy, unbiased=True)
    a, b = torch.from_numpy(g["xa"].copy()).to(DEV), torch.from_numpy(g["xb"].copy()).to(DEV)
    bank = muse.FeatureBank(d, DEV).update(a[:n // 2]).update(a[n // 2:])
    got, named, banked, unbiased = muse.mmd_distance(a, b), muse.cmmd_distance(a, b), muse.cmmd_distance(bank, b), muse.mmd_distance(a, b, unbiased=True)
    print(f"d {d} n {n} m {m}: got {got!r} golden {g['distance']!r} err / bound {abs(got - g['distance']) / tol:.4f}; unbiased {unbiased!r} "
          f"golden {g['distance_unbiased']!r} err / bound {abs(unbiased - g['distance_unbiased']) / tol_u:.4f}")
    assert isinstance(got, float) and named == got and banked == got
    assert abs(got - g["distance"]) <= tol and abs(unbiased - g["distance_unbiased"]) <= tol_u
    assert abs(muse.mmd_distance(b, a) - got) <= tol
    # d(a, a): the three sums are the same pairs, by two kernels
    ra = MC.rinv(g["xa"])
    k, w = MC.oracle(g["xa"], g["xa"], MC.GAMMA, ra, ra)
    same = muse.cmmd_distance(a, a)
    print(f"d {d} n {n}: d(a, a) = {same:.3e}")
    assert abs(same) <= MC.distance_bound(MC.SCALE, n, n, txx, txx, MC.bound(k, w, MC.GAMMA, d, MC.chain(n, n, False)))
    # other constants go through: sigma, scale, no normalisation - against the oracle
    t, w = MC.sqdist(g["xa"], g["xb"])
    sigma = float(np.sqrt(t.max() / 8.0))                       # gamma T spans 0 .. 4
    gamma = 1.0 / (2.0 * sigma ** 2)
    sums, tols = [], []
    for x, y, sym in ((g["xa"], g["xa"], True), (g["xb"], g["xb"], True), (g["xa"], g["xb"], False)):
        k, w = MC.oracle(x, y, gamma)
        sums.append(MC.exact_sum(k))
        tols.append(MC.bound(k, w, gamma, d, MC.chain(len(x), len(y), sym)))
    want = 7.0 * (sums[0] / n ** 2 + sums[1] / m ** 2 - 2.0 * sums[2] / (n * m))
    assert abs(muse.mmd_distance(a, b, sigma=sigma, scale=7.0, normalize=False) - want) <= MC.distance_bound(7.0, n, m, *tols)
    bad = a.clone()
    bad[n // 2, d // 2] = float("nan")
    assert np.isnan(muse.cmmd_distance(bad, b)) and np.isnan(muse.mmd_distance(b, bad, normalize=False))


# ---- 9. plumbing ----------------------------------------------------------------------------------------------------------------------
def test_feature_bank_on_the_device(tmp_path):
    import muse
    d = 68
    rows = torch.from_numpy(normal(300, d, 5)).to(DEV)
    bank = muse.FeatureBank(d, DEV)
    cuts = [0, 60, 60, 130, 300]                                # an empty batch; two doublings of the capacity (64 -> 256 -> 512)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        bank.update(rows[lo:hi])
        assert bank.n == hi and bank.features().is_cuda and torch.equal(bank.features(), rows[:hi])
    wide = torch.full((9, d + 12), float("nan"), device=DEV)
    wide[:, 5:5 + d] = rows[:9]
    other = muse.FeatureBank(d, DEV).update(wide[:, 5:5 + d])    # a row-strided view that is not 16-byte aligned: the bank copies it
    assert bank.merge(other).n == 309 and torch.equal(bank.features()[300:], rows[:9])
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    back = muse.FeatureBank.load(path, device=DEV)
    assert back.n == 309 and back.features().is_cuda and torch.equal(back.features().view(torch.int32), bank.features().view(torch.int32))
    assert muse.cmmd_distance(back, other) == muse.cmmd_distance(bank.features(), rows[:9])
    assert muse.cmmd_distance(wide[:, 5:5 + d], bank) == muse.cmmd_distance(rows[:9], bank)          # an unaligned view is copied, same bits
    with pytest.raises(ValueError, match="features is f32 on"):
        bank.update(rows[:2].cpu())


def test_scorer_fills_a_feature_bank():
    import muse
    enc = muse.CLIPImageEncoder.from_transformers(CV.tower(64, 2, 28, 14, "quick_gelu")[0]).to(DEV)
    scorer = muse.CLIPScorer(enc)
    images, others = CV.smooth_images(32, 40).to(DEV), CV.smooth_images(32, 40, seed=1).to(DEV)
    embeds, other_embeds = scorer.image_embeds(images), scorer.image_embeds(others)
    bank, other_bank = muse.FeatureBank(CV.PROJ, DEV), muse.FeatureBank(CV.PROJ, DEV)
    assert scorer.accumulate(bank, images) is bank and scorer.accumulate(other_bank, others) is other_bank
    assert bank.n == 32 and torch.equal(bank.features(), embeds) and torch.equal(other_bank.features(), other_embeds)
    value = muse.cmmd_distance(bank, other_bank)
    print(f"scorer: cmmd(a, b) = {value!r}, cmmd(a, a) = {muse.cmmd_distance(bank, bank)!r}")
    assert value == muse.cmmd_distance(embeds, other_embeds) and np.isfinite(value) and value > abs(muse.cmmd_distance(bank, bank))
