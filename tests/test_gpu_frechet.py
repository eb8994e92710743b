"""GPU (MI355X): muse_moments_f64 (csrc/moments.hip) exactly and per element, muse.FeatureStats / muse.frechet_distance on the statistics
the kernel builds, and the CLIPScorer surface that feeds it.  tests/frechet_cpu.py holds the golden cases, the references and the bounds
with their derivations.

Every kernel case: x sits inside a larger allocation with NaN before and after it and in every ldx > d gap (a read outside the n rows'
first d columns poisons the result); `sum` and `outer` sit in one allocation pre-filled with a NaN bit pattern no result has, guard bands
on both sides and between them, and the strict lower triangle of `outer` keeps that pattern: it must come back bit for bit."""
import functools

import numpy as np
import pytest
import torch

import clip_vision_cpu as CV
import frechet_cpu as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FF85EA71E5EA7ED                                     # a quiet NaN with a payload no computation produces
GUARD = 32
ERR_BAD_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3


def _lib():
    from muse import _hip
    return _hip.lib()


def _stream():
    from muse import _hip
    return _hip.stream()


class X:
    """f32 [n, d] rows at stride ldx inside a NaN-filled allocation; .ptr is 16-byte aligned"""

    def __init__(self, x, ldx=None):
        n, d = x.shape
        self.n, self.d, self.ldx = n, d, d if ldx is None else ldx
        size = max(n - 1, 0) * self.ldx + d
        host = torch.full((GUARD + size + GUARD,), float("nan"), dtype=torch.float32)
        if n:
            host[GUARD:GUARD + size].as_strided((n, d), (self.ldx, 1)).copy_(torch.from_numpy(np.ascontiguousarray(x)))
        self.t = host.to(DEV)
        self.ptr = self.t.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0


class Acc:
    """sum f64 [d] and outer f64 [d, d] in one sentinel-filled allocation: guard | sum | guard | outer | guard.  init = (sum, outer) puts
    values into sum and the upper triangle + diagonal of outer; init = None leaves every byte a sentinel (for refused calls)."""

    def __init__(self, d, init="zeros"):
        self.d = d
        host = torch.full((3 * GUARD + d + d * d,), SENT, dtype=torch.int64)
        self.lo, self.mid = GUARD, 2 * GUARD + d
        if init is not None:
            s, o = (np.zeros(d), np.zeros((d, d))) if isinstance(init, str) else init
            host[self.lo:self.lo + d] = torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).view(torch.int64)
            block = host[self.mid:self.mid + d * d].view(d, d)
            upper = torch.triu(torch.ones(d, d, dtype=torch.bool))
            block[upper] = torch.from_numpy(np.ascontiguousarray(o, dtype=np.float64)).view(torch.int64)[upper]
        self.t = host.to(DEV)
        self.sum_ptr, self.outer_ptr = self.t.data_ptr() + 8 * self.lo, self.t.data_ptr() + 8 * self.mid

    def read(self, what):
        """-> (sum, outer) as numpy f64 after checking the guards and the strict lower triangle"""
        d, host = self.d, self.t.cpu()
        for name, band in (("front", host[:self.lo]), ("middle", host[self.lo + d:self.mid]), ("back", host[self.mid + d * d:])):
            assert bool((band == SENT).all()), f"{what}: the {name} guard band was written"
        outer = host[self.mid:self.mid + d * d].view(d, d)
        lower = torch.tril(torch.ones(d, d, dtype=torch.bool), -1)
        assert bool((outer[lower] == SENT).all()), f"{what}: the strict lower triangle of outer was written"
        return host[self.lo:self.lo + d].view(torch.float64).numpy().copy(), outer.view(torch.float64).numpy().copy()

    def untouched(self, what):
        assert bool((self.t.cpu() == SENT).all()), f"{what}: a refused call wrote to its outputs"


def launch(x, acc, n=None, d=None, ldx=None, xptr=None, sum_ptr=None, outer_ptr=None):
    return _lib().muse_moments_f64(x.ptr if xptr is None else xptr, x.n if n is None else n, x.d if d is None else d,
                                   x.ldx if ldx is None else ldx, acc.sum_ptr if sum_ptr is None else sum_ptr,
                                   acc.outer_ptr if outer_ptr is None else outer_ptr, _stream())


def run(chunks, d, init="zeros", ldx=None, what=""):
    """one launch per chunk onto one accumulator -> (sum, outer) numpy"""
    acc = Acc(d, init)
    xs = [X(c, ldx) for c in chunks]
    for x in xs:
        rc = launch(x, acc)
        assert rc == 0, f"{what}: the entry returned {rc}"
    torch.cuda.synchronize()
    return acc.read(what)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_exact(got, want, what):
    """sum and the upper triangle + diagonal of outer equal the exact values bit for bit"""
    (gs, go), (ws, wo) = got, want
    iu = np.triu_indices(len(ws))
    assert same_bits(gs, ws), f"{what}: sum differs at {np.flatnonzero(gs != ws)[:8]}"
    if not same_bits(go[iu], wo[iu]):
        bad = np.argwhere(np.triu(go != wo))
        raise AssertionError(f"{what}: outer differs at {len(bad)} places, first (i, j) = {bad[:6].tolist()}: "
                             f"got {[go[i, j] for i, j in bad[:6]]} want {[wo[i, j] for i, j in bad[:6]]}")


# ---- exact legs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 16, 60, 64, 68, 132])
def test_integer_probes_are_exact(d):
    """integers in [-3, 3]: one tile, ragged tiles in both directions, three tile columns (diagonal and off-diagonal tiles each with a
    ragged edge); n around the group of four and the 16-row step, with and without a row gap"""
    for n in (1, 3, 4, 5, 67, 260):
        x = FC.int_features(n, d, 1000 * d + n)
        want = FC.int_moments(x)
        for ldx in (d, d + 4):
            what = f"integers d {d} n {n} ldx {ldx}"
            check_exact(run([x], d, ldx=ldx, what=what), want, what)


@pytest.mark.parametrize("d", [16, 68, 132])
def test_index_probes(d):
    """values that name their position: a transposed or mis-mapped f64 fragment shows up as the wrong product at a named (i, j)"""
    ramp = np.zeros((7, d), dtype=np.float32)
    ramp[5] = np.arange(1, d + 1)                                                    # one non-zero row, x[5][c] = c + 1
    idx = np.arange(1, d + 1, dtype=np.float64)
    check_exact(run([ramp], d, what=f"ramp d {d}"), (idx, np.outer(idx, idx)), f"ramp row d {d}: outer[i][j] = (i + 1)(j + 1)")
    primes = np.array([p for p in range(2, 800) if all(p % q for q in range(2, int(p ** 0.5) + 1))][:d], dtype=np.float64)
    col = np.random.default_rng(d).permutation(d)                                    # row r is prime_r at column col[r]
    hot = np.zeros((d, d), dtype=np.float32)
    hot[np.arange(d), col] = primes
    want_sum, want_outer = np.zeros(d), np.zeros((d, d))
    want_sum[col] = primes
    want_outer[col, col] = primes ** 2
    check_exact(run([hot], d, what=f"one-hot d {d}"), (want_sum, want_outer), f"one-hot rows d {d}: a diagonal of squares")


@pytest.mark.parametrize("n1,n2", [(5, 67), (64, 64), (1, 3)])
def test_accumulation_is_in_place_and_exact(n1, n2):
    for d in (68, 132):
        rng = np.random.default_rng(n1 * 1000 + n2 + d)
        init = (rng.integers(-50, 51, size=d).astype(np.float64), rng.integers(-50, 51, size=(d, d)).astype(np.float64))
        x = FC.int_features(n1 + n2, d, 77 * d + n1)
        ws, wo = FC.int_moments(x)                                                   # one shot over the concatenation
        what = f"two calls ({n1}, {n2}) d {d}"
        check_exact(run([x[:n1], x[n1:]], d, init=init, what=what), (init[0] + ws, init[1] + wo), what)


def test_equal_call_sequences_give_equal_bits():
    rng = np.random.default_rng(5)
    chunks = [rng.standard_normal((n, 132)).astype(np.float32) for n in (67, 1, 260)]
    (s1, o1), (s2, o2) = run(chunks, 132, what="sequence, first"), run(chunks, 132, what="sequence, second")
    iu = np.triu_indices(132)
    assert same_bits(s1, s2) and same_bits(o1[iu], o2[iu])


# ---- rounding leg ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("n,d,cuts", [(67, 68, (20, 24)), (260, 132, (100, 101))])
def test_general_values_within_the_derived_bound(n, d, cuts, scale):
    """N(0, 1) * scale in one, two and three calls against numpy f64 on the converted inputs:
    |err| <= (n_total + calls + 4) 2^-53 sum_n |x_ni| |x_nj| elementwise (frechet_cpu.moments_bound: exact products, one rounding per
    addition)"""
    x = (np.random.default_rng(n + d).standard_normal((n, d)) * scale).astype(np.float32)
    ws, wo, abs_sum, abs_outer = FC.f64_moments(x)
    iu = np.triu_indices(d)
    for chunks in ([x], [x[:cuts[0]], x[cuts[0]:]], [x[:cuts[0]], x[cuts[0]:cuts[1]], x[cuts[1]:]]):
        calls = len(chunks)
        gs, go = run(chunks, d, ldx=d + 4, what=f"general n {n} d {d} scale {scale} calls {calls}")
        es, eo = np.abs(gs - ws), np.abs(go - wo)[iu]
        bs, bo = FC.moments_bound(n, calls, abs_sum), FC.moments_bound(n, calls, abs_outer)[iu]
        print(f"n {n} d {d} scale {scale:g} calls {calls}: worst err / bound: sum {float((es / bs).max()):.3f}, outer {float((eo / bo).max()):.3f}")
        assert (es <= bs).all() and (eo <= bo).all()


@pytest.mark.parametrize("first,second", [(np.inf, np.nan), (np.nan, -np.inf)])
def test_special_values_propagate_as_in_numpy(first, second):
    """one special value at an interior position, one in the ragged last group of rows (rows 64 .. 66 of 67): the NaN / inf pattern and
    the finite entries equal numpy's f64 x^T x.  Padding the last group with a clamped address instead of zeros would add row 66 twice."""
    n, d = 67, 68
    x = np.random.default_rng(9).standard_normal((n, d)).astype(np.float32)
    x[21, 37], x[65, 5] = first, second
    with np.errstate(invalid="ignore", over="ignore"):
        ws, wo, abs_sum, abs_outer = FC.f64_moments(x)
    gs, go = run([x], d, what=f"specials {first} {second}")
    iu = np.triu_indices(d)
    for got, want, bound, name in ((gs, ws, FC.moments_bound(n, 1, abs_sum), "sum"), (go[iu], wo[iu], FC.moments_bound(n, 1, abs_outer)[iu], "outer")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: the NaN pattern differs"
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{name}: the inf pattern differs"
        fin = np.isfinite(want)
        assert fin.sum() > 0.9 * fin.size and (np.abs(got[fin] - want[fin]) <= bound[fin]).all(), f"{name}: finite entries"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    d, n = 68, 5
    xv = FC.int_features(n, d, 3)
    x, wide = X(xv), X(xv, d + 4)
    fresh = run([xv], d, what="fresh")
    cases = [("d = 0", ERR_BAD_ARG, dict(d=0)), ("d < 0", ERR_BAD_ARG, dict(d=-4)), ("d % 4", ERR_BAD_ARG, dict(d=66, ldx=66)),
             ("n < 0", ERR_BAD_ARG, dict(n=-1)), ("ldx < d", ERR_BAD_ARG, dict(ldx=d - 4)),
             ("x 4 bytes off", ERR_ALIGN, dict(xptr=x.ptr + 4)), ("x 8 bytes off", ERR_ALIGN, dict(xptr=x.ptr + 8)),
             ("sum 4 bytes off", ERR_ALIGN, dict(sum_ptr="+4")), ("outer 4 bytes off", ERR_ALIGN, dict(outer_ptr="+4")),
             ("grid overflow", ERR_UNSUPPORTED, dict(d=4194244, ldx=4194244, n=1))]        # 65536 tile columns: 2^31 + 32768 tiles
    kept = []                                                   # operands and outputs of refused calls stay alive until the device is idle
    for what, code, kw in cases:
        acc = Acc(d, init=None)
        kept.append(acc)
        if kw.get("sum_ptr") == "+4":
            kw["sum_ptr"] = acc.sum_ptr + 4
        if kw.get("outer_ptr") == "+4":
            kw["outer_ptr"] = acc.outer_ptr + 4
        for operand in (x, wide):
            rc = launch(operand, acc, **kw)
            assert rc == code, f"{what}: the entry returned {rc}, not {code}"
    empty = Acc(d, init=None)
    assert launch(x, empty, n=0) == 0                           # n == 0: success, nothing launched
    torch.cuda.synchronize()
    for (what, _, _), acc in zip(cases, kept):
        acc.untouched(what)
    empty.untouched("n == 0")
    again = run([xv], d, what="after the refusals")
    iu = np.triu_indices(d)
    assert same_bits(again[0], fresh[0]) and same_bits(again[1][iu], fresh[1][iu])
    check_exact(again, FC.int_moments(xv), "after the refusals")


def test_ops_wrapper_checks_its_arguments():
    from muse import ops
    from muse._hip import MuseHipError
    s, o = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    good = torch.ones(3, 8, device=DEV)
    for bad in (lambda: ops.moments_f64_(good.double(), s, o), lambda: ops.moments_f64_(good.t().contiguous().t(), s, o),
                lambda: ops.moments_f64_(torch.ones(3, 6, device=DEV), s[:6], o[:6, :6].contiguous()), lambda: ops.moments_f64_(good, s.float(), o),
                lambda: ops.moments_f64_(good, s, o[:, :4]), lambda: ops.moments_f64_(good.cpu(), s, o)):
        with pytest.raises(MuseHipError):
            bad()
    torch.cuda.synchronize()
    assert not s.any() and not o.any()
    assert ops.moments_f64_(good, s, o) is o
    assert torch.equal(s.cpu(), torch.full((8,), 3.0, dtype=torch.float64)) and torch.equal(o.cpu(), torch.triu(torch.full((8, 8), 3.0, dtype=torch.float64)))


# ---- FeatureStats ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_stats(d, n, which, batch):
    """muse.FeatureStats of a golden feature set, fed `batch` rows at a time (0: in one batch); shared, never modified"""
    import muse
    x = torch.from_numpy(FC.golden(d, n)["x" + which].copy()).to(DEV)
    st = muse.FeatureStats(d, DEV)
    for lo in range(0, n, batch or n):
        st.update(x[lo:lo + (batch or n)])
    return st


@pytest.mark.parametrize("d,n", FC.CASES)
def test_feature_stats_meet_the_golden_mean_and_covariance(d, n):
    """mean() and cov() of the kernel-built statistics against np.mean / np.cov of the golden file, within
    64 n 2^-53 max_i sum_n x_ni^2 / (n - 1) - the cancellation of the one-pass centring (frechet_cpu.cov_bound)"""
    g = FC.golden(d, n)
    for which in "ab":
        bound = FC.cov_bound(g["x" + which])
        for batch in (64, 0):
            st = golden_stats(d, n, which, batch)
            assert st.n == n and st.sum.device.type == "cuda" and st.outer.dtype == torch.float64
            mean_err, cov_err = np.abs(st.mean() - g["mu" + which]).max(), np.abs(st.cov() - g["s" + which]).max()
            print(f"D {d} N {n} set {which} batch {batch}: mean err {mean_err:.3e}, cov err {cov_err:.3e}, bound {bound:.3e}")
            assert mean_err <= bound and cov_err <= bound
            assert np.array_equal(st.cov(), st.cov().T)


@pytest.mark.parametrize("d,n", FC.CASES)
def test_distance_of_kernel_built_statistics_meets_the_golden(d, n):
    import muse
    g = FC.golden(d, n)
    tol = FC.rtol(d, n)
    for batch in (64, 0):
        a, b = golden_stats(d, n, "a", batch), golden_stats(d, n, "b", batch)
        got = muse.frechet_distance(a, b)
        print(f"D {d} N {n} batch {batch}: got {got!r} golden {g['distance']!r} rel {abs(got - g['distance']) / g['distance']:.2e} tolerance {tol:g}")
        assert FC.close(got, g["distance"], tol)
        assert FC.close(muse.frechet_distance(a, (g["mub"], g["sb"])), g["distance"], tol)
        assert abs(muse.frechet_distance(a, a)) <= FC.identity_bound(g["sa"])


def test_merge_save_and_strided_views(tmp_path):
    import muse
    d, n = 68, 90
    x = FC.int_features(n, d, 11)
    wide = torch.full((n, d + 12), float("nan"), device=DEV)
    wide[:, 4:4 + d] = torch.from_numpy(x)
    one = muse.FeatureStats(d, DEV).update(wide[:, 4:4 + d])                     # a row-strided view, 16 bytes into the row
    first, second = muse.FeatureStats(d, DEV).update(wide[:41, 4:4 + d]), muse.FeatureStats(d, DEV).update(wide[41:, 4:4 + d])
    assert first.merge(second) is first and first.n == n == one.n
    ws, wo = FC.int_moments(x)
    for st in (one, first):                                                      # integers: the merge equals one pass exactly
        assert same_bits(st.sum.cpu().numpy(), ws) and same_bits(st.outer.cpu().numpy(), np.triu(wo))
    path = str(tmp_path / "stats.npz")
    one.save(path)
    back = muse.FeatureStats.load(path, device=DEV)
    assert back.n == n and torch.equal(back.sum, one.sum) and torch.equal(back.outer, one.outer)
    back.update(wide[:3, 4:4 + d])                                               # loaded statistics go on accumulating
    ws3, wo3 = FC.int_moments(np.concatenate([x, x[:3]]))
    assert back.n == n + 3 and same_bits(back.sum.cpu().numpy(), ws3) and same_bits(back.outer.cpu().numpy(), np.triu(wo3))
    assert muse.FeatureStats(d, DEV).update(wide[:0, 4:4 + d]).n == 0            # an empty batch is a no-op


# ---- the scorer -----------------------------------------------------------------------------------------------------------------------
def test_scorer_accumulates_what_it_embeds():
    import muse
    enc = muse.CLIPImageEncoder.from_transformers(CV.tower(64, 2, 28, 14, "quick_gelu")[0]).to(DEV)
    scorer = muse.CLIPScorer(enc)
    images, others = CV.smooth_images(32, 40).to(DEV), CV.smooth_images(32, 40, seed=1).to(DEV)
    text_embeds = torch.randn(5, CV.PROJ, generator=torch.Generator().manual_seed(3)).to(DEV)

    embeds = scorer.image_embeds(images)
    assert embeds.shape == (32, CV.PROJ) and embeds.dtype == torch.float32 and embeds.is_cuda
    assert torch.equal(scorer.image_embeds(pixel_values=scorer.preprocess(images)), embeds)
    with pytest.raises(ValueError, match="exactly one of images= and pixel_values="):
        scorer.image_embeds()
    # __call__ is unchanged: its embeds are the method's, and its matrices are clip_scores of them, bit for bit
    scores = scorer(images, text_embeds=text_embeds)
    cosine, logits = muse.clip_scores(embeds, text_embeds, enc.logit_scale.data)
    assert torch.equal(scores.image_embeds, embeds) and torch.equal(scores.cosine, cosine) and torch.equal(scores.logits_per_image, logits)

    def stats(imgs, through):
        st = muse.FeatureStats(CV.PROJ, DEV)
        for lo in (0, 16):
            if through == "accumulate":
                assert scorer.accumulate(st, imgs[lo:lo + 16]) is st
            else:
                st.update(scorer.image_embeds(imgs[lo:lo + 16]))
        return st

    a, again, b = stats(images, "accumulate"), stats(images, "update"), stats(others, "accumulate")
    assert a.n == again.n == 32 and torch.equal(a.sum, again.sum) and torch.equal(a.outer, again.outer)
    assert bool(torch.isfinite(a.sum).all()) and float(a.outer.diagonal().min()) > 0
    same, different = muse.frechet_distance(a, again), muse.frechet_distance(a, b)
    print(f"scorer: d(a, a) = {same:.3e} (bound {FC.identity_bound(a.cov()):.3e}), d(a, b) = {different:.6g}")
    assert abs(same) <= FC.identity_bound(a.cov())                               # 32 rows of width 48: rank deficient, and still inside
    assert different > 0
