"""muse.frechet_distance and muse.FeatureStats without a device: the distance against the scipy golden and a numpy oracle, the identity,
the statistics file, and the refusals.  The accumulation itself (csrc/moments.hip) is tested on the GPU, tests/test_gpu_frechet.py."""
import inspect

import numpy as np
import pytest
import torch

import frechet_cpu as FC


def test_the_names_are_exported():
    import muse
    import muse.frechet as M
    from muse import _hip, ops
    assert muse.FeatureStats is M.FeatureStats and muse.frechet_distance is M.frechet_distance
    assert "FeatureStats" in muse.__all__ and "frechet_distance" in muse.__all__
    assert "muse_moments_f64" in _hip.SIGNATURES and callable(ops.moments_f64_)
    assert list(inspect.signature(muse.CLIPScorer.image_embeds).parameters)[1:] == ["images", "pixel_values"]
    assert list(inspect.signature(muse.CLIPScorer.accumulate).parameters)[1:] == ["stats", "images", "pixel_values"]
    assert not any("fid" in name.lower() for name in dir(M))                      # it is not FID, and is not called so


@pytest.mark.parametrize("d,n", FC.CASES)
def test_distance_meets_the_golden_and_the_numpy_oracle(d, n):
    import muse
    g = FC.golden(d, n)
    got = muse.frechet_distance((g["mua"], g["sa"]), (g["mub"], g["sb"]))
    oracle = FC.oracle_distance(g["mua"], g["sa"], g["mub"], g["sb"])
    tol = FC.rtol(d, n)
    print(f"D {d} N {n}: got {got!r} golden {g['distance']!r} (rel {abs(got - g['distance']) / g['distance']:.2e}) "
          f"oracle {oracle!r} (rel {abs(got - oracle) / oracle:.2e}) tolerance {tol:g}")
    assert isinstance(got, float) and got > 0
    assert FC.close(got, g["distance"], tol) and FC.close(got, oracle, tol)
    # symmetric in its arguments to the same tolerance, and the golden's own mean / covariance are what the features give
    assert FC.close(muse.frechet_distance((g["mub"], g["sb"]), (g["mua"], g["sa"])), got, tol)
    x = g["xa"].astype(np.float64)
    assert np.array_equal(np.mean(x, axis=0), g["mua"]) and np.array_equal(np.cov(x, rowvar=False), g["sa"])


@pytest.mark.parametrize("d,n", FC.CASES)
def test_identity(d, n):
    """|d(a, a)| <= 1e-9 (tr Sa + tr Sa), the rank-deficient case included; the raw value is returned, so it may be negative"""
    import muse
    g = FC.golden(d, n)
    for mu, s in ((g["mua"], g["sa"]), (g["mub"], g["sb"])):
        self_distance = muse.frechet_distance((mu, s), (mu, s))
        print(f"D {d} N {n}: d(a, a) = {self_distance:.3e}, bound {FC.identity_bound(s):.3e}")
        assert abs(self_distance) <= FC.identity_bound(s)


def test_arguments_may_be_stats_pairs_tensors_or_lists():
    import muse
    g = FC.golden(16, 64)
    want = muse.frechet_distance((g["mua"], g["sa"]), (g["mub"], g["sb"]))
    a = muse.FeatureStats.from_moments(64, g["mua"], g["sa"])
    b = muse.FeatureStats.from_moments(64, torch.from_numpy(g["mub"].copy()), torch.from_numpy(g["sb"].copy()))
    assert a.n == 64 and a.dim == 16 and np.array_equal(a.mean(), g["mua"]) and np.array_equal(a.cov(), g["sa"])
    assert muse.frechet_distance(a, b) == want
    assert muse.frechet_distance(a, (g["mub"].tolist(), g["sb"].tolist())) == want
    assert muse.frechet_distance((torch.from_numpy(g["mua"].copy()), torch.from_numpy(g["sa"].copy())), b) == want


def _filled(d, n, seed):
    """a FeatureStats on the CPU whose accumulators were filled by numpy (upper triangle only, as the kernel leaves them)"""
    import muse
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x64 = x.astype(np.float64)
    st = muse.FeatureStats(d, "cpu")
    st.n = n
    st.sum.copy_(torch.from_numpy(x64.sum(0)))
    st.outer.copy_(torch.from_numpy(np.triu(x64.T @ x64)))
    return st, x


def test_mean_and_cov_are_numpys_definition():
    st, x = _filled(12, 40, 1)
    x64 = x.astype(np.float64)
    assert st.mean().dtype == np.float64 and st.cov().dtype == np.float64
    assert np.abs(st.mean() - x64.mean(0)).max() <= FC.cov_bound(x) / 40
    c = st.cov()
    assert np.array_equal(c, c.T) and np.abs(c - np.cov(x64, rowvar=False)).max() <= FC.cov_bound(x)
    # the lower triangle of `outer` is not read: garbage there changes nothing
    st.outer += torch.tril(torch.full((12, 12), 1e30, dtype=torch.float64), -1)
    assert np.array_equal(st.cov(), c)


def test_save_load_round_trip_is_bit_identical(tmp_path):
    import muse
    st, _ = _filled(8, 21, 2)
    path = str(tmp_path / "stats.npz")
    st.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["mu", "n", "outer", "sigma", "sum"]
        assert int(z["n"]) == 21 and np.array_equal(z["mu"], st.mean()) and np.array_equal(z["sigma"], st.cov())
    back = muse.FeatureStats.load(path)
    assert back.n == st.n and back.dim == 8 and back.sum.device.type == "cpu"
    for a, b in zip(back.tensors(), st.tensors()):
        assert a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert np.array_equal(back.cov(), st.cov()) and muse.frechet_distance(back, st) == muse.frechet_distance(st, st)
    # merge adds the three accumulators
    other, _ = _filled(8, 5, 3)
    n0, s0, o0 = back.n, back.sum.clone(), back.outer.clone()
    assert back.merge(other) is back
    assert back.n == n0 + 5 and torch.equal(back.sum, s0 + other.sum) and torch.equal(back.outer, o0 + other.outer)
    # an empty accumulator saves and loads too; a foreign file is refused by name
    empty = str(tmp_path / "empty.npz")
    muse.FeatureStats(4, "cpu").save(empty)
    assert muse.FeatureStats.load(empty).n == 0
    np.savez(str(tmp_path / "foreign.npz"), mu=np.zeros(4), sigma=np.eye(4))
    with pytest.raises(ValueError, match="not a file written by FeatureStats.save"):
        muse.FeatureStats.load(str(tmp_path / "foreign.npz"))


def test_refusals():
    import muse
    from muse._hip import MuseHipError
    g = FC.golden(16, 64)
    given = muse.FeatureStats.from_moments(64, g["mua"], g["sa"])
    for call in (lambda: given.update(torch.zeros(2, 16)), lambda: given.merge(muse.FeatureStats(16, "cpu")),
                 lambda: muse.FeatureStats(16, "cpu").merge(given)):
        with pytest.raises(ValueError, match="from_moments.*cannot be updated"):
            call()
    st = muse.FeatureStats(16, "cpu")
    with pytest.raises(ValueError, match="at least two feature rows"):
        st.cov()
    st.n = 1
    with pytest.raises(ValueError, match="at least two feature rows, got n = 1"):
        st.cov()
    with pytest.raises(MuseHipError, match="no CPU compute path"):          # as everywhere else in the package
        st.update(torch.zeros(3, 16))
    with pytest.raises(ValueError, match=r"features is \[B, 16\]"):
        st.update(torch.zeros(3, 12))
    with pytest.raises(ValueError, match="multiple of 4"):
        muse.FeatureStats(10, "cpu")
    other = FC.golden(48, 192)
    with pytest.raises(ValueError, match="feature widths differ: 16 and 48"):
        muse.frechet_distance((g["mua"], g["sa"]), (other["mua"], other["sa"]))
    with pytest.raises(ValueError, match="widths differ"):
        muse.frechet_distance(given, muse.FeatureStats.from_moments(192, other["mua"], other["sa"]))
    with pytest.raises(ValueError, match=r"\(mu \[d\], sigma \[d, d\]\)"):
        muse.frechet_distance((g["mua"], g["sa"][:, :8]), (g["mub"], g["sb"]))
    with pytest.raises(ValueError, match="FeatureStats or a"):
        muse.frechet_distance(3.0, given)
