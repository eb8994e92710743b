"""CPU: the spatial / layout / VQ edge tests' own machinery (tests/spatial_cpu.py).  The float64 references agree with torch.nn.functional;
the clean contract models pass every check the GPU test applies; each of the thirteen seeded defects fails at least one of them."""
import math

import pytest
import torch
import torch.nn.functional as F

import spatial_cpu as S
from spatial_cpu import BF, F32, F64, GUARD


def close(a, b, tol=1e-12):
    return float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


# ---- the references against torch.nn.functional, float64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 3), (2, 3, 5, 10), (3, 1, 7, 4), (2, 6, 1, 5)])
def test_dwconv_reference(B, H, W, C):
    x, dy, w = S.randn((B, H, W, C), 1).double(), S.randn((B, H, W, C), 2).double(), S.randn((C, 3, 3), 3).double()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr.permute(0, 3, 1, 2), wr.view(C, 1, 3, 3), padding=1, groups=C).permute(0, 2, 3, 1)
    y.backward(dy)
    assert close(S.ref_dwconv(x, w), y.detach())
    assert close(S.ref_dwconv_dx(dy, w), xr.grad)
    assert close(S.ref_dwconv_dw(dy, x).sum(0).view(C, 3, 3), wr.grad)
    assert S.ref_dwconv_dw(dy, x).shape == (S.dw_nchunk(B * H * W), C, 9)


def test_movement_references():
    x = S.randn((2, 4, 6, 8), 4).double()
    nchw = x.permute(0, 3, 1, 2)
    assert torch.equal(S.ref_upsample2x(x), F.interpolate(nchw, scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    assert close(S.ref_avgpool(x), F.avg_pool2d(nchw, 2, 2).permute(0, 2, 3, 1))
    pu = F.pixel_unshuffle(nchw, 2).view(2, 8, 2, 2, 2, 3).permute(0, 4, 5, 2, 3, 1).reshape(2, 2, 3, 32)      # (c, di, dj) -> (di, dj, c)
    assert torch.equal(S.ref_space_to_depth(x), pu)
    assert torch.equal(S.ref_space_to_depth(S.ref_space_to_depth(x), True), x)
    t = S.randn((2, 3, 7), 5)
    assert torch.equal(S.ref_nhwc_to_nchw(S.ref_nchw_to_nhwc(t, 8), 3), t)
    assert torch.equal(S.ref_nchw_to_nhwc(t, 4)[:, :, :3], t.permute(0, 2, 1)) and not bool(S.bits(S.ref_nchw_to_nhwc(t, 4)[:, :, 3]).any())
    hi, lo = S.ref_split(t)
    assert float((t.double() - hi.double() - lo.double()).abs().max()) <= 2.0 ** -17 * float(t.abs().max())


@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_reference(silu):
    x, gamma, beta = S.randn((2, 37, 64), 6, 3.0).double(), S.randn((64,), 7).double(), S.randn((64,), 8).double()
    y, t, scale = S.ref_groupnorm(x, gamma, beta, 32, 1e-6, silu)
    ref = F.group_norm(x.transpose(1, 2), 32, gamma, beta, 1e-6).transpose(1, 2)
    assert close(y, F.silu(ref) if silu else ref, 1e-10)
    assert bool((scale >= t.abs() - 1e-9).all())
    p = S.ref_gn_partials(x, 32)
    assert close(p[..., 0].sum(1), x.view(2, 37, 32, 2).sum((1, 3))) and close(p[..., 1].sum(1), (x * x).view(2, 37, 32, 2).sum((1, 3)))


def test_grn_reference():
    x, dy, gamma, beta = S.randn((2, 9, 10), 9).double(), S.randn((2, 9, 10), 10).double(), S.randn((10,), 11).double(), S.randn((10,), 12).double()
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    Gx = torch.norm(xr, p=2, dim=1, keepdim=True)
    y = gr * (xr * (Gx / (Gx.mean(dim=-1, keepdim=True) + 1e-6))) + br + xr
    y.backward(dy)
    ref, G, N = S.ref_grn(x, gamma, beta)
    assert close(ref, y.detach())
    rb = S.ref_grn_bwd(dy, x, gamma, G, N)
    assert close(rb["dx"], xr.grad, 1e-10) and close(rb["NS1"].sum(0), gr.grad, 1e-10) and close(rb["S0"].sum(0), br.grad, 1e-10)
    for k, b in S.bound_grn(x, gamma, beta).items():
        assert bool((b > 0).all()), k
    for k, b in S.bound_grn_bwd(dy, x, gamma, G, N).items():
        assert bool((b > 0).all()), k


def test_small_references():
    x, dy = S.randn((200,), 13).double(), S.randn((200,), 14).double()
    xr = x.clone().requires_grad_(True)
    F.silu(xr).backward(dy)
    dx, scale = S.ref_silu_bwd(x, dy)
    assert close(dx, xr.grad) and bool((scale >= dx.abs() - 1e-12).all())
    assert close(S.silu64(x), F.silu(x))
    B, R, C = 2, 5, 4
    g, v, ss = S.randn((B * R, C), 15).double(), S.randn((B * R, C), 16).double(), S.randn((B, 2 * C), 17).double()
    vr, sr = v.clone().requires_grad_(True), ss.clone().requires_grad_(True)
    (vr.view(B, R, C) * (1.0 + sr[:, None, :C]) + sr[:, None, C:]).backward(g.view(B, R, C))
    edx, edss = S.ref_adaln_bwd(g, v, ss, B, R, C)
    assert close(edx.reshape(B * R, C), vr.grad) and close(edss, sr.grad)
    out, scale = S.ref_sinusoid(torch.tensor([0.0, 1.0, 500.0]), 5, 10000.0)
    assert out.shape == (3, 5) and torch.equal(out[:, 4], torch.zeros(3, dtype=F64)) and torch.equal(out[0, :2], torch.ones(2, dtype=F64))
    assert close(out[2, 3], torch.tensor(math.sin(500.0 * 10000.0 ** -0.5), dtype=F64))


def test_argmin_reference():
    """finite rows and rows of +inf: torch.argmin; NaN: the documented difference"""
    for n in (1, 2, 64, 129):
        for seed in (0, 5):
            d = S.argmin_rows_case(n, 5, seed)
            ref = S.ref_argmin(d)
            assert bool(((ref >= 0) & (ref < n)).all())
            plain = ~d.isnan().any(1)
            assert torch.equal(ref[plain], d.argmin(1)[plain])
    nan, inf = S.NAN, math.inf
    d = torch.tensor([[nan, nan, nan], [nan, inf, inf], [inf, inf, inf], [nan, 2.0, 1.0], [0.0, -0.0, 1.0], [-inf, nan, -inf]])
    assert S.ref_argmin(d).tolist() == [0, 1, 0, 2, 0, 0]
    assert d.argmin(1).tolist()[:2] == [0, 0] and d.argmin(1).tolist()[3] == 0       # torch: the first NaN wins


# ---- the contract models: clean passes every check, a defect fails at least one ---------------------------------------------------------
def storage_of(t, dtype):
    st = S.alloc_out(t.numel(), dtype)
    st[GUARD:GUARD + t.numel()] = t.flatten().to(dtype)
    return st


GN_MODEL_CASES = [(255, 128, 32, 0.0), (1025, 1024, 64, 0.0), (255, 64, 32, 1e3), (2049, 128, 32, 1e3)]      # (HW, C, groups, shift of x)


def checks(defect):
    """every (name, thunk) the GPU test's checks make of a model with `defect`; a thunk raises AssertionError where the check fails"""
    out = []
    for probe in ("coord", "pick", "dense"):
        for B, H, W, C in [(2, 3, 5, 12), (2, 1, 4, 12), (3, 5, 7, 4)]:
            c = S.dwconv_case(probe, B, H, W, C, 40 + C)
            n = c["y"].numel()
            a_st, g_st = S.place(c["a"], F32), S.place(c["g"], F32)
            out.append((f"dwconv y {probe} {B}x{H}x{W}x{C}", lambda c=c, a_st=a_st, n=n: S.check_out(
                S.model_dwconv(a_st, c["w"], c["B"], c["H"], c["W"], c["C"], False, defect), n, c["y"], "y")))
            out.append((f"dwconv dx {probe} {B}x{H}x{W}x{C}", lambda c=c, g_st=g_st, n=n: S.check_out(
                S.model_dwconv(g_st, c["w"], c["B"], c["H"], c["W"], c["C"], True, defect), n, c["dx"], "dx")))
            if c["exact"]["dw"]:
                out.append((f"dwconv dw {probe} {B}x{H}x{W}x{C}", lambda c=c: S.check_out(
                    S.model_dwconv_dw(c["g"], c["a"], defect), c["dw"].numel(), c["dw"], "dw")))
    for n in (1, 2, 63, 64, 65, 129):
        for seed in (0, 5):
            d = S.argmin_rows_case(n, 5, seed)

            def argmin_check(d=d, n=n):
                got = S.model_argmin(S.place_ld(d, F32, n + 5), 5, n, n + 5, defect)
                assert torch.equal(got, S.ref_argmin(d)), (got.tolist(), S.ref_argmin(d).tolist())
            out.append((f"argmin n{n} seed{seed}", argmin_check))
    x = S.coord_ids((2, 3, 37), "bf16", 3).float()
    for dtype in (F32, BF):
        out.append((f"nchw_to_nhwc {dtype}", lambda dtype=dtype: S.check_zero_sign(
            S.check_out(S.model_nchw_to_nhwc(x, 4, dtype, defect), 2 * 37 * 4, S.ref_nchw_to_nhwc(x, 4), "layout"), S.ref_nchw_to_nhwc(x, 4), "layout")))
    full = S.coord_ids((2, 4, 6, 4), "f32", 4).float()
    for inverse in (False, True):
        src = S.ref_space_to_depth(full) if inverse else full
        exp = full if inverse else S.ref_space_to_depth(full)
        out.append((f"space_to_depth inverse{inverse}", lambda src=src, exp=exp, inverse=inverse: S.check_out(
            storage_of(S.ref_space_to_depth(src, inverse, defect), F32), exp.numel(), exp, "s2d")))
    t = S.randn((9, 65), 5)
    out.append(("gather bf16", lambda: S.check_out(storage_of(S.to_bf16(t, defect), BF), t.numel(), S.to_bf16(t), "gather")))
    hi, lo = S.ref_split(t, defect)
    out.append(("split lo", lambda: S.check_out(storage_of(lo, BF), t.numel(), S.ref_split(t)[1], "split")))
    gx, gamma, beta = S.randn((2, 5, 4), 6), S.randn((4,), 7), S.randn((4,), 8)
    y, G, N = S.ref_grn(gx, gamma, beta, defect)
    bd = S.bound_grn(gx, gamma, beta)
    out.append(("grn y", lambda: S.check_out(storage_of(y, F32), y.numel(), S.ref_grn(gx, gamma, beta)[0], "grn", exact=False, bound=bd["y"])))
    out.append(("grn N", lambda: S.check_out(storage_of(N, F32), N.numel(), S.ref_grn(gx, gamma, beta)[2], "grn N", exact=False, bound=bd["N"])))
    for HW, C, G, shift in GN_MODEL_CASES:
        vx, vg, vb = S.randn((2, HW, C), 20 + HW, shift), S.randn((C,), 21), S.randn((C,), 22)
        out.append((f"groupnorm HW{HW} C{C} G{G} shift{int(shift)}", lambda vx=vx, vg=vg, vb=vb, G=G: S.check_out(
            storage_of(S.model_groupnorm(vx, vg, vb, G, 1e-6, defect), F32), vx.numel(), S.ref_groupnorm(vx, vg, vb, G, 1e-6, 0)[0], "groupnorm",
            exact=False, bound=S.bound_groupnorm(vx, vg, vb, G, 1e-6, 0, False))))
    return out


def failures(defect):
    bad = []
    for name, thunk in checks(defect):
        try:
            thunk()
        except AssertionError:
            bad.append(name)
    return bad


def test_clean_models_pass_every_check():
    assert failures(None) == []


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_seeded_defect_is_caught(defect):
    bad = failures(defect)
    print(f"[spatial_cpu] {defect}: {len(bad)} checks fail: {bad[:4]}")
    assert bad, f"no check notices the defect {defect}"


def test_groupnorm_bound_sees_a_wrong_eps():
    """eps ten times too large in the float64 reference itself (no rounding at all) at HW = 255, C = 128, G = 32, N(0, 1): rstd moves by a
    relative 4.5e-6, the derived bound allows about 4 * 2^-24 - with and without the SiLU, f32 and bf16 input"""
    for dtype, silu in ((F32, 0), (F32, 1), (BF, 0)):
        x, gamma, beta = S.randn((2, 255, 128), 30).to(dtype).float(), S.randn((128,), 31), S.randn((128,), 32)
        y = S.ref_groupnorm(x, gamma, beta, 32, 1e-6, silu)[0]
        bad = S.ref_groupnorm(x, gamma, beta, 32, 1e-5, silu)[0]
        w = S.worst_ratio(bad, y, S.bound_groupnorm(x, gamma, beta, 32, 1e-6, silu, False))
        print(f"[spatial_cpu] groupnorm eps x 10, {dtype} silu{silu}: {w:.1f} x bound")
        assert w > 4.0
        assert S.worst_ratio(y, y, S.bound_groupnorm(x, gamma, beta, 32, 1e-6, silu, False)) == 0.0


def test_worst_ratio_never_passes_a_nan():
    ref, bound = torch.ones(4, dtype=F64), torch.ones(4, dtype=F64)
    assert S.worst_ratio(ref + 0.5, ref, bound) == 0.5
    for bad in (S.NAN, math.inf):
        got = ref.clone()
        got[2] = bad
        assert S.worst_ratio(got, ref, bound) == math.inf
    assert S.worst_ratio(ref[:0], ref[:0], bound[:0]) == 0.0


def test_defect_list():
    assert len(S.DEFECTS) >= 10 and len(set(S.DEFECTS)) == len(S.DEFECTS)


# ---- the checks themselves ---------------------------------------------------------------------------------------------------------------
def test_check_index_sees_gap_writes_and_missing_slots():
    idx = S.ld_index(3, 4, 6, batch=2, stride=20)
    exp = torch.arange(24.0)
    st = S.alloc_out(40, F32)
    st[GUARD + idx] = exp
    S.check_index(st, idx, exp, "ok")
    for pos, val in ((GUARD + 4, 0.0), (GUARD - 1, 1.0), (GUARD + 39, 2.0)):            # an ld gap, the front guard, the batch gap at the end
        bad = st.clone()
        bad[pos] = val
        with pytest.raises(AssertionError):
            S.check_index(bad, idx, exp, "stray")
    missing = S.alloc_out(40, F32)
    missing[GUARD + idx[1:]] = exp[1:]
    with pytest.raises(AssertionError):
        S.check_index(missing, idx, exp, "missing")
    with pytest.raises(AssertionError):
        S.check_untouched(st, "written")
    S.check_untouched(S.alloc_out(8, F64), "clean")
    with pytest.raises(AssertionError):
        S.check_zero_sign(torch.tensor([-0.0, 1.0]), torch.tensor([0.0, 1.0]), "minus zero")


def test_storage_builders():
    t = torch.arange(1.0, 7.0).view(2, 3)
    st = S.place_ld(t, F32, 5)
    assert bool(st[:S.LEAD].isnan().all()) and bool(st[S.LEAD + 3:S.LEAD + 5].isnan().all()) and torch.equal(st[S.LEAD + 5:S.LEAD + 8], t[1])
    sh = S.place_shifted(t, F32, 1)
    assert bool(sh[:S.LEAD + 1].isnan().all()) and torch.equal(sh[S.LEAD + 1:S.LEAD + 7], t.flatten()) and bool(sh[S.LEAD + 7:].isnan().all())
    dy = S.pick_dy(3, 5, 7, 4, 9)
    assert torch.equal(dy.view(105, 4)[:64].sum(0), torch.ones(4)) and torch.equal(dy.view(105, 4)[64:].sum(0), torch.ones(4))
    assert torch.equal(S.onehot_taps(12, 5).view(12, 9).sum(1), torch.ones(12)) and len(set(S.onehot_taps(12, 5).view(12, 9).argmax(1).tolist())) == 9
