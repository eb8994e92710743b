"""CPU: the convolution edge tests' own tools (tests/conv_cpu.py) are sound - ref_conv is the convolution torch computes, the clean contract
model passes every check on the shapes of tests/test_gpu_conv_edges.py, each seeded defect fails at least one check, and assert_exact
rejects operands that would let rounding in.  `python tests/test_conv_cpu.py` prints the defect counts of profiles/conv_edges.md."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cpu as Cv  # noqa: E402
from conv_cpu import BF, F32, F64  # noqa: E402


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


# ---- ref_conv is the convolution --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KS,ups", [(1, 0), (3, 0), (1, 1), (3, 1), (3, 2)])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 4, 6), (3, 5, 7), (1, 2, 16)])
def test_ref_conv_is_torch_conv2d(B, H, W, KS, ups):
    if ups == 1 and (H | W) & 1:
        H, W = 2 * H, 2 * W
    Hin, Win = Cv.in_dims(H, W, ups)
    Cin, Cout = 5, 7
    x, w = rnd((B, Hin, Win, Cin), 1), rnd((Cout, KS, KS, Cin), 2)
    bias, res = rnd((Cout,), 3), rnd((B, H, W, Cout), 4)
    xn = x.permute(0, 3, 1, 2)
    if ups == 1:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    if ups == 2:
        ref = F.conv2d(F.pad(xn, (0, 1, 0, 1)), w.permute(0, 3, 1, 2), bias, stride=2)
    else:
        ref = F.conv2d(xn, w.permute(0, 3, 1, 2), bias, padding=(KS - 1) // 2)
    ref = ref.permute(0, 2, 3, 1) + res
    got = Cv.ref_conv(x, w, H, W, KS, ups, bias=bias, residual=res)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_ref_conv_activation_and_pool_are_torch():
    B, H, W, Cin, Cout = 2, 4, 6, 5, 3
    x, w = rnd((B, H, W, Cin), 5), rnd((Cout, 3, 3, Cin), 6)
    sc, sh = 1 + 0.5 * rnd((B, Cin), 7), rnd((B, Cin), 8)
    act = F.silu(x * sc[:, None, None, :] + sh[:, None, None, :])
    ref = F.conv2d(act.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1)          # zero padding AFTER the activation
    got = Cv.ref_conv(x, w, H, W, 3, scale=sc, shift=sh)
    assert float((got - ref.permute(0, 2, 3, 1)).abs().max()) <= 1e-12
    pooled = Cv.ref_conv(x, w, H, W, 3, scale=sc, shift=sh, pool=True)
    assert float((pooled - F.avg_pool2d(ref, 2, 2).permute(0, 2, 3, 1)).abs().max()) <= 1e-12


def test_probe_generators():
    for kind, dt in (("bf16", BF), ("x3", F32), ("f32", F32)):
        v = Cv.coord_ids((2, 5, 7, 12), kind, 3)
        assert int(v.min()) >= 1 and int(v.max()) < Cv.COORD_MOD[kind]
        assert torch.equal(v.to(dt).double(), v.double())
        # neighbours along every axis differ (a one-pixel / one-channel / one-image slip changes the value)
        for d in range(4):
            assert float((v.narrow(d, 0, v.shape[d] - 1) != v.narrow(d, 1, v.shape[d] - 1)).double().mean()) > 0.98
    hi, lo = Cv.split_hi_lo(Cv.coord_ids((4096,), "x3", 1).float())
    assert torch.equal(hi.double() + lo.double(), Cv.coord_ids((4096,), "x3", 1).double())
    for Cin, Cout in ((8, 5), (64, 20), (320, 128)):
        w, tap, ci = Cv.onehot_weights(Cout, 3, Cin, 9)
        assert torch.equal(w.flatten(1).sum(1), torch.ones(Cout, dtype=torch.int64))
        n = min(Cout, 9 * ((Cin + 31) // 32))
        seen = {(int(t), int(c) // 32) for t, c in zip(tap[:n], ci[:n])}
        assert len(seen) == n and (n < 9 or {t for t, _ in seen} == set(range(9)))


# ---- the clean model passes on the shapes of the GPU file ------------------------------------------------------------------------------
LOADER_CASES = [  # path, B, H, W, Cin, Cout, KS, ups, bias, res
    ("f32", 1, 1, 1, 4, 1, 3, 0, False, False), ("f32", 1, 1, 7, 8, 3, 3, 0, True, False), ("f32", 7, 1, 1, 12, 4, 1, 0, False, True),
    ("f32", 3, 5, 7, 20, 5, 3, 0, True, True), ("f32", 1, 8, 16, 64, 127, 3, 0, False, False), ("f32", 1, 3, 43, 68, 129, 3, 0, True, False),
    ("f32", 2, 9, 13, 4, 132, 3, 0, False, True), ("f32", 2, 4, 6, 12, 5, 3, 1, True, True), ("f32", 2, 5, 7, 8, 4, 3, 2, True, True),
    ("bf16", 3, 5, 7, 24, 5, 3, 0, True, True), ("bf16", 1, 3, 43, 72, 129, 3, 0, True, False), ("bf16", 2, 1, 5, 8, 3, 3, 2, False, True),
    ("split", 3, 5, 7, 40, 5, 3, 0, True, True), ("split", 1, 127, 1, 8, 128, 3, 0, False, False), ("split", 2, 2, 2, 16, 132, 1, 1, True, True),
    ("split2", 1, 15, 17, 32, 4, 3, 0, True, True), ("split2", 3, 9, 19, 96, 132, 3, 0, False, True),
]


@pytest.mark.parametrize("case", LOADER_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("probe", ["coord", "dense"])
def test_clean_model_passes(case, probe):
    path, B, H, W, Cin, Cout, KS, ups, bias, res = case
    c = Cv.build_case(path, probe, B, H, W, Cin, Cout, KS, ups, bias, res, seed=11)
    st, _ = Cv.model_case(c)
    Cv.check_out(st, c["expected"].numel(), c["expected"], f"model {case} {probe}")


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 16, 16, 64, 4), (2, 16, 32, 128, 132), (2, 32, 16, 192, 64), (1, 48, 48, 64, 128)])
def test_clean_slab_model_passes_with_partials(B, H, W, Cin, Cout):
    for probe in ("coord", "dense"):
        c = Cv.build_case("split2", probe, B, H, W, Cin, Cout, 3, 0, True, True, seed=12)
        gn = ("slab", 32) if Cout % 128 == 0 else None
        st, part = Cv.model_case(c, order="slab", gn=gn)
        Cv.check_out(st, c["expected"].numel(), c["expected"], "slab model")
        if gn:
            Cv.check_partials(part, Cv.partials_ref(c["expected"], "slab", 32), "slab model partials")


def test_clean_model_passes_on_every_exact_case_of_the_gpu_file():
    """the case lists of tests/test_gpu_conv_edges.py themselves (loader paths, tap-major, slab; slab shapes in both K orders)"""
    import test_gpu_conv_edges as G
    n = 0
    for path, B, H, W, Cin, Cout, KS, ups, bias, res in G.loader_cases():
        for probe in ("coord", "dense"):
            c = Cv.build_case(path, probe, B, H, W, Cin, Cout, KS, ups, bias, res, seed=n)
            Cv.check_out(Cv.model_case(c)[0], c["expected"].numel(), c["expected"], f"model {path} {probe}")
            n += 1
    for i, (B, H, W) in enumerate(G.TAP_BHW):
        c = Cv.build_case("split2", "coord", B, H, W, (32, 96, 160)[i % 3], G.TAP_COUT[i], 3, 0, True, True, seed=n)
        Cv.check_out(Cv.model_case(c)[0], c["expected"].numel(), c["expected"], "model tap-major")
        n += 1
    for B, H, W, Cin, Cout, bias, res in G.slab_cases():
        if (H, W) == (48, 48) and Cin == 320:
            continue                                             # (the nine-patch image once is enough for the model)
        c = Cv.build_case("split2", "coord", B, H, W, Cin, Cout, 3, 0, bias, res, seed=n)
        for order in ("slab", "tap"):
            Cv.check_out(Cv.model_case(c, order=order)[0], c["expected"].numel(), c["expected"], f"model slab shapes, {order} order")
        n += 1
    assert n > 200


def test_partial_maps_differ_and_sum_to_the_same_totals():
    o = Cv.ints((2, 32, 32, 128), 100, 5).double()
    maps = {p: Cv.partials_ref(o, p, 32) for p in ("split", "tap", "slab", "row")}
    tot = o.view(2, 1024, 32, 4).sum((1, 3))
    for p, v in maps.items():
        assert torch.equal(v[..., 0].sum(1), tot), p
    assert maps["split"].shape[1] == 8 and maps["tap"].shape[1] == 4 and maps["slab"].shape[1] == 4 and maps["row"].shape[1] == 32
    assert not torch.equal(maps["tap"], maps["slab"])            # a 256-pixel run is not a 16 x 16 patch when W > 16
    pooled = Cv.pool2(o)
    assert torch.equal(Cv.partials_ref(pooled, "pool", 32)[..., 0].sum(1), pooled.view(2, 256, 32, 4).sum((1, 3)))


# ---- every seeded defect fails a check --------------------------------------------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _act_case(pool=False):
    B, H, W, Cin, Cout = 2, 16, 16, 64, 8
    x = rnd((B, H, W, Cin), 21).float()
    sc, sh = (1 + 0.3 * rnd((B, Cin), 22)).float(), (0.5 * rnd((B, Cin), 23)).float()
    w, _, _ = Cv.onehot_weights(Cout, 3, Cin, 24)
    exp = Cv.ref_conv(x, w, H, W, 3, scale=sc, shift=sh, pool=pool)

    def run(defect):
        st, _ = Cv.model_conv([Cv.place(x, F32)], [Cv.place_weights(w, F32)], H, W, 3, 0, Cin, Cout, order="slab", scale=sc, shift=sh,
                              pool=pool, defect=defect, out_dtype=F64)
        Cv.check_out(st, exp.numel(), exp, "act model", exact=False, bound=torch.full_like(exp, 1e-12))
    return run


def defect_runs(defect):
    """(name, callable that raises AssertionError when a check fails) for every case a defect can show on"""
    runs = []
    for case in LOADER_CASES:
        for probe in ("coord", "dense"):
            path, B, H, W, Cin, Cout, KS, ups, bias, res = case
            order = "tap"

            def run(case=case, probe=probe, order=order):
                path, B, H, W, Cin, Cout, KS, ups, bias, res = case
                c = Cv.build_case(path, probe, B, H, W, Cin, Cout, KS, ups, bias, res, seed=11)
                st, _ = Cv.model_case(c, order=order, defect=defect)
                Cv.check_out(st, c["expected"].numel(), c["expected"], "model")
            runs.append((f"{case}-{probe}", run))
    for B, H, W, Cin, Cout in [(2, 16, 32, 128, 128), (1, 48, 48, 64, 132)]:
        for probe in ("coord", "dense"):
            def run(B=B, H=H, W=W, Cin=Cin, Cout=Cout, probe=probe, pool=False):
                c = Cv.build_case("split2", probe, B, H, W, Cin, Cout, 3, 0, True, True, seed=12)
                gn = ((("pool" if pool else "slab"), 32) if Cout % 128 == 0 else None)
                st, part = Cv.model_conv(c["planes"], c["w_st"], H, W, 3, 0, Cin, Cout, order="slab", bias=c["bias"], residual=c["res"],
                                         pool=pool, gn=gn, defect=defect)
                exp = Cv.pool2(c["expected"]) if pool else c["expected"]
                Cv.check_out(st, exp.numel(), exp, "slab model")
                if gn:
                    Cv.check_partials(part, Cv.partials_ref(exp, gn[0], 32), "slab partials")
            runs.append((f"slab-{B}x{H}x{W}x{Cin}x{Cout}-{probe}", run))
            runs.append((f"pool-{B}x{H}x{W}x{Cin}x{Cout}-{probe}", lambda run=run: run(pool=True)))
    act, actp = _act_case(), _act_case(pool=True)
    runs.append(("act", lambda: act(defect)))
    runs.append(("act-pool", lambda: actp(defect)))
    return runs


def defect_counts(defect):
    runs = defect_runs(defect)
    return sum(_fails(fn) for _, fn in runs), len(runs)


def test_no_defect_no_failure():
    failed, n = defect_counts(None)
    assert failed == 0 and n > 40


@pytest.mark.parametrize("defect", Cv.DEFECTS)
def test_each_seeded_defect_fails_a_check(defect):
    failed, n = defect_counts(defect)
    print(f"[conv_cpu] defect {defect}: {failed} of {n} model runs fail a check")
    assert failed >= 1, f"no check notices the defect {defect}"


# ---- assert_exact ----------------------------------------------------------------------------------------------------------------------
def test_assert_exact_rejects_what_would_round():
    x, w = Cv.ints((1, 4, 4, 8), 1023, 1), Cv.ints((4, 3, 3, 8), 7, 2)
    Cv.assert_exact([(x, w)])
    with pytest.raises(AssertionError):
        Cv.assert_exact([(x * 40000, w)])                       # a partial sum may pass 2^24
    with pytest.raises(AssertionError):
        Cv.assert_exact([(x.double() + 0.5, w)])                # not integers
    with pytest.raises(AssertionError):
        Cv.assert_exact([(x, w)], out_dtype=BF)                 # a bf16 result above 256 need not be representable
    with pytest.raises(AssertionError):
        Cv.assert_exact([(Cv.ints((1, 4, 4, 8), 3, 1), Cv.sparse_pm1(4, 72, 64, 2))], residual=torch.full((1,), 200), out_dtype=BF)
    Cv.assert_exact([(Cv.ints((1, 4, 4, 8), 3, 1), Cv.sparse_pm1(4, 72, 64, 2))], residual=torch.full((1,), 3), out_dtype=BF)
    with pytest.raises(AssertionError):
        Cv.exact_in(torch.tensor([257.0]), BF)


def test_split_residual_bound_is_2_to_minus_17():
    """hi + lo carries x to 2^-17 |x|: attained (x = 1 + 2^-8 + 2^-17 leaves 2^-17, so 2^-18 is no bound) and never exceeded"""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -17], dtype=F32)
    hi, lo = Cv.split_hi_lo(x)
    r = float((x.double() - hi.double() - lo.double()).abs())
    assert r == 2.0 ** -17 and 2.0 ** -18 * float(x) < r <= Cv.SPLIT_RES * float(x)
    g = torch.Generator().manual_seed(51)
    y = torch.cat([rnd((1 << 18,), 51).float(), torch.randint(1 << 23, 1 << 24, (1 << 18,), generator=g).float(),   # every 24-bit pattern kind
                   (1.0 + 2.0 ** -8 + torch.arange(-64, 65) * 2.0 ** -23).float()])
    hi, lo = Cv.split_hi_lo(y)
    assert bool(((y.double() - hi.double() - lo.double()).abs() <= Cv.SPLIT_RES * y.double().abs()).all())
    assert bool((lo.double().abs() <= 2.0 ** -8 * y.double().abs()).all())


# ---- the derived bounds hold for a CPU evaluation in the path's own arithmetic ---------------------------------------------------------
def _im2col(x, H, W, KS, ups):
    cols = []
    for ky in range(KS):
        for kx in range(KS):
            iy, ix, oky, okx = Cv.tap_source(H, W, KS, ups, ky, kx)
            g = x[:, iy.clamp(0, x.shape[1] - 1)][:, :, ix.clamp(0, x.shape[2] - 1)]
            cols.append(g * (oky[:, None] & okx[None, :]).to(x.dtype)[None, :, :, None])
    return torch.cat(cols, -1)


def contract_eval(path, x, w, H, W, KS, ups, bias, res):
    """the path's arithmetic on the CPU: f32 products and sums; bf16 operands with f32 sums and a bf16 result; the three bf16x3 products"""
    f = lambda t: t.float()
    if path == "f32":
        return f(_im2col(f(x), H, W, KS, ups)) @ f(w).flatten(1).T + f(bias) + f(res)
    if path == "bf16":
        return ((_im2col(f(x), H, W, KS, ups) @ f(w).flatten(1).T + f(bias)).to(BF).float() + f(res)).to(BF)
    xh, xl = Cv.split_hi_lo(f(x))
    wh, wl = Cv.split_hi_lo(f(w))
    a_h, a_l = _im2col(xh.float(), H, W, KS, ups), _im2col(xl.float(), H, W, KS, ups)
    return a_l @ wh.float().flatten(1).T + a_h @ wl.float().flatten(1).T + a_h @ wh.float().flatten(1).T + f(bias) + f(res)


ROUNDING = {"f32": Cv.bound_f32, "bf16": Cv.bound_bf16, "x3": Cv.bound_x3}


def rounding_figures(verbose=False):
    out = {}
    for path in ("f32", "bf16", "x3"):
        B, H, W, Cin, Cout, KS = 2, 9, 13, 72, 20, 3
        dt = BF if path == "bf16" else F32
        x, w = rnd((B, H, W, Cin), 31).to(dt), (rnd((Cout, KS, KS, Cin), 32) / 25).to(dt)
        bias, res = rnd((Cout,), 33).float(), rnd((B, H, W, Cout), 34).to(dt)
        ref = Cv.ref_conv(x, w, H, W, KS, 0, bias=bias, residual=res)
        S = Cv.abs_terms(x, w, H, W, KS, 0, bias=bias, residual=res)
        got = contract_eval(path, x, w, H, W, KS, 0, bias, res)
        out[path] = float(((got.double() - ref).abs() / ROUNDING[path](S, KS * KS * Cin)).max())
    return out


def test_derived_bounds_hold_for_the_cpu_contract_evaluation():
    for path, worst in rounding_figures().items():
        print(f"[conv_cpu] {path}: CPU contract evaluation reaches {worst:.3f} of its derived bound")
        assert worst <= 0.5, (path, worst)                       # with margin: the bound is a worst case, the evaluation one sample


def test_activation_bound_holds_for_the_f32_cpu_evaluation():
    x, sc, sh = rnd((2, 16, 16, 64), 41, 2.0).float(), (1 + 0.5 * rnd((2, 64), 42)).float(), rnd((2, 64), 43).float()
    t = x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    err = (Cv.silu32(x, sc, sh).double() - Cv.silu64(t)).abs()
    worst = float((err / Cv.bound_act(t)).max())
    print(f"[conv_cpu] activation: f32 CPU evaluation reaches {worst:.3f} of the derived bound (E_ref {float(err.max()):.3e})")
    assert worst <= 0.5
    hi, lo = Cv.split_hi_lo(Cv.silu32(x, sc, sh))
    # read back as planes: the split's 2^-17 is attained, so this part of the bound has no margin to show - it must simply hold
    assert float(((hi.double() + lo.double() - Cv.silu64(t)).abs() / Cv.bound_act(t, planes=True)).max()) <= 1.0


if __name__ == "__main__":
    for d in Cv.DEFECTS:
        failed, n = defect_counts(d)
        print(f"{d:16s} fails {failed:3d} of {n} model runs")
    print(rounding_figures())
