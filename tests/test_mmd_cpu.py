"""muse.FeatureBank, muse.mmd_distance and muse.cmmd_distance without a device: the exported surface, the numpy oracle of tests/mmd_cpu.py
against the longdouble golden, the bank on the CPU, and the refusals.  The sums themselves (csrc/mmd.hip) are tested on the GPU,
tests/test_gpu_mmd.py."""
import inspect

import numpy as np
import pytest
import torch

import mmd_cpu as MC


def test_the_names_are_exported():
    import muse
    import muse.mmd as M
    from muse import _hip, ops
    assert muse.FeatureBank is M.FeatureBank and muse.mmd_distance is M.mmd_distance and muse.cmmd_distance is M.cmmd_distance
    assert all(name in muse.__all__ for name in ("FeatureBank", "mmd_distance", "cmmd_distance"))
    for symbol in ("muse_row_norms_f64", "muse_rbf_pair_sums_f64", "muse_rbf_pair_sums_workspace"):
        assert symbol in _hip.SIGNATURES
    assert list(inspect.signature(ops.row_norms_f64).parameters) == ["x", "want_rinv"]
    assert list(inspect.signature(ops.rbf_pair_sums_f64).parameters) == ["x", "y", "gamma", "rx", "ry"]
    p = inspect.signature(muse.mmd_distance).parameters
    assert list(p) == ["a", "b", "sigma", "scale", "normalize", "unbiased"]
    assert (p["sigma"].default, p["scale"].default, p["normalize"].default, p["unbiased"].default) == (10.0, 1000.0, True, False)
    assert list(inspect.signature(muse.cmmd_distance).parameters) == ["a", "b"]
    # the bank goes where the statistics go: CLIPScorer.accumulate calls .update(features) on either
    assert list(inspect.signature(muse.FeatureBank.update).parameters) == list(inspect.signature(muse.FeatureStats.update).parameters)
    for method in ("features", "merge", "to", "save", "load"):
        assert callable(getattr(muse.FeatureBank, method))
    assert "ATen's antialiased bicubic resize" in muse.cmmd_distance.__doc__ and "ViT-L/14@336" in muse.cmmd_distance.__doc__


def test_workspace_count_is_what_the_bound_reads_off():
    """muse_rbf_pair_sums_workspace (a host function: no device needed) = 4 partials per tile, twice that when symmetric"""
    from muse import _hip
    count = _hip.lib().muse_rbf_pair_sums_workspace
    for n, m in ((1, 1), (64, 65), (129, 63), (4096, 4096), (32768, 32768)):
        assert count(n, m, 0) == 4 * MC.tiles(n, m, False) and count(n, m, 1) == 8 * MC.tiles(n, n, True)
    assert count(0, 5, 0) == 0 and count(-1, 5, 0) == -1 and count(5, -1, 0) == -1 and count(5, -1, 1) == 8
    assert count(64 * 46341, 64 * 46341, 0) == -3 and count(64 * 46340, 64 * 46340, 0) == 4 * 46340 ** 2      # 2^31 - 1 tiles at the most


@pytest.mark.parametrize("d,n,m", MC.CASES)
def test_the_f64_oracle_meets_the_longdouble_golden(d, n, m):
    """the expansion form (a + b) - 2 c in f64 - what the kernel computes - against explicit differences in longdouble, within the bound
    the GPU tests hold the kernel to (tests/mmd_cpu.py: bound), with the reference's own chain of one rounding"""
    g = MC.golden(d, n, m)
    ra, rb = MC.rinv(g["xa"]), MC.rinv(g["xb"])
    sums = {}
    for name, x, y, rx, ry in (("sxx", g["xa"], g["xa"], ra, ra), ("syy", g["xb"], g["xb"], rb, rb), ("sxy", g["xa"], g["xb"], ra, rb)):
        k, w = MC.oracle(x, y, MC.GAMMA, rx, ry)
        got, tol = MC.exact_sum(k), MC.bound(k, w, MC.GAMMA, d, 1)
        print(f"d {d} n {n} m {m} {name}: oracle {got!r} golden {g[name]!r} err / bound {abs(got - g[name]) / tol:.3f}")
        assert abs(got - g[name]) <= tol
        sums[name] = got
        if name != "sxy":
            off = ~np.eye(len(x), dtype=bool)
            assert abs(MC.exact_sum(k[off]) - g[name + "_off"]) <= MC.bound(k, w, MC.GAMMA, d, 1, off)
    value = MC.SCALE * (sums["sxx"] / n ** 2 + sums["syy"] / m ** 2 - 2.0 * sums["sxy"] / (n * m))
    assert abs(value - g["distance"]) <= MC.distance_bound(MC.SCALE, n, m, *MC.case_bounds(d, n, m))
    assert 0.5 < g["distance"] < 2.0 and g["distance_unbiased"] < g["distance"]


def test_feature_bank_on_the_cpu(tmp_path):
    import muse
    rng = np.random.default_rng(0)
    rows = torch.from_numpy(rng.standard_normal((300, 12)).astype(np.float32))
    bank = muse.FeatureBank(12, "cpu")
    assert bank.n == 0 and tuple(bank.features().shape) == (0, 12)
    cuts = [0, 3, 3, 70, 71, 300]                              # an empty batch; growth past 64 and past 128 and 256
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        assert bank.update(rows[lo:hi]) is bank
        assert bank.n == hi and torch.equal(bank.features(), rows[:hi])          # earlier rows survive every growth
    wide = torch.full((5, 20), float("nan"))
    wide[:, 3:15] = rows[:5]
    other = muse.FeatureBank(12, "cpu").update(wide[:, 3:15])                       # a row-strided, unaligned view
    assert bank.merge(other) is bank and bank.n == 305 and torch.equal(bank.features()[300:], rows[:5])
    # save / load: bit-identical
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    with np.load(path) as z:
        assert z.files == ["features"] and z["features"].dtype == np.float32 and z["features"].shape == (305, 12)
    back = muse.FeatureBank.load(path)
    assert back.n == 305 and back.dim == 12 and back.features().device.type == "cpu"
    assert torch.equal(back.features().view(torch.int32), bank.features().view(torch.int32))
    back.update(rows[:2])                                                           # a loaded bank goes on growing
    assert back.n == 307 and torch.equal(back.features()[:305], bank.features())
    # a plain [n, d] .npy array loads too (f64 is converted)
    np.save(str(tmp_path / "plain.npy"), rows[:9].numpy())
    np.save(str(tmp_path / "double.npy"), rows[:9].numpy().astype(np.float64))
    for name in ("plain.npy", "double.npy"):
        plain = muse.FeatureBank.load(str(tmp_path / name))
        assert plain.n == 9 and plain.dim == 12 and torch.equal(plain.features(), rows[:9])
    empty = str(tmp_path / "empty.npz")
    muse.FeatureBank(8, "cpu").save(empty)
    assert muse.FeatureBank.load(empty).n == 0 and muse.FeatureBank.load(empty).dim == 8


def test_refusals(tmp_path):
    import muse
    from muse import ops
    from muse._hip import MuseHipError
    with pytest.raises(ValueError, match="multiple of 4"):
        muse.FeatureBank(10, "cpu")
    bank = muse.FeatureBank(16, "cpu")
    with pytest.raises(ValueError, match=r"features is \[B, 16\]"):
        bank.update(torch.zeros(3, 12))
    with pytest.raises(ValueError, match="features is f32"):
        bank.update(torch.zeros(3, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="FeatureBank of width 16"):
        bank.merge(muse.FeatureBank(8, "cpu"))
    np.savez(str(tmp_path / "foreign.npz"), mu=np.zeros(4))
    with pytest.raises(ValueError, match="not a file written by FeatureBank.save"):
        muse.FeatureBank.load(str(tmp_path / "foreign.npz"))
    np.save(str(tmp_path / "flat.npy"), np.zeros(7, dtype=np.float32))
    with pytest.raises(ValueError, match=r"\[n, d\] array expected"):
        muse.FeatureBank.load(str(tmp_path / "flat.npy"))
    a, b = torch.zeros(5, 16), torch.ones(3, 16)
    with pytest.raises(ValueError, match="at least one row"):
        muse.mmd_distance(bank, a)
    with pytest.raises(ValueError, match="at least one row"):
        muse.cmmd_distance(a, a[:0])
    with pytest.raises(ValueError, match="feature widths differ: 16 and 12"):
        muse.mmd_distance(a, torch.zeros(3, 12))
    with pytest.raises(ValueError, match="unbiased estimate needs at least two rows"):
        muse.mmd_distance(a, b[:1], unbiased=True)
    with pytest.raises(ValueError, match="holds f32 features"):
        muse.mmd_distance(a.double(), b)
    with pytest.raises(ValueError, match=r"is \[n, d\]"):
        muse.mmd_distance(a[0], b)
    with pytest.raises(ValueError, match="sigma is positive"):
        muse.mmd_distance(a, b, sigma=0.0)
    for call in (lambda: muse.mmd_distance(a, b), lambda: muse.cmmd_distance(a.numpy(), b.numpy()), lambda: ops.row_norms_f64(a),
                 lambda: ops.rbf_pair_sums_f64(a, b, gamma=1.0)):
        with pytest.raises(MuseHipError, match="no CPU compute path"):              # as everywhere else in the package
            call()
