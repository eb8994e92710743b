"""CPU: the tokenizer edge tests' own machinery (tests/tokenizer_cpu.py).  The float64 references agree with paella_cpu.py, movq_cpu.py
and torch.nn.functional; the clean contract models pass every check the GPU test applies; each of the seventeen seeded defects fails at
least one of them; the derived SpatialNorm bound rejects an eps ten times off, exchanged convolutions and a source pixel one off."""
import math

import pytest
import torch
import torch.nn.functional as F

import movq_cpu
import paella_cpu
import spatial_cpu as S
import test_gpu_tokenizer_edges as G
import tokenizer_cpu as T
from spatial_cpu import F32, F64, LEAD

EPS = 1e-6


def close(a, b, tol=1e-12):
    return float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


# ---- the references against paella_cpu / movq_cpu / torch, float64 -----------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 3, 5, 12), (3, 1, 4, 8), (2, 5, 1, 24)])
def test_mix_reference(B, H, W, C):
    x, w9, bias, g = T.mix_inputs(B, H, W, C, 3)
    y, stats, scale = T.ref_mix(x, w9, bias, g)
    want = paella_cpu.mix(x.double().permute(0, 3, 1, 2), w9.double().t().reshape(C, 1, 3, 3), bias.double(), g.double()).permute(0, 2, 3, 1)
    assert close(y, want)
    assert bool((scale >= (y - x.double()).abs() - 1e-12).all())
    assert close(stats[:, 0], x.double().view(-1, C).mean(1)) and close(stats[:, 1], 1.0 / (x.double().view(-1, C).var(1, unbiased=False) + 1e-6).sqrt())


def test_patch_rows_reference():
    for KS, stride, pt, pl in [(4, 2, 1, 1), (2, 1, 1, 0), (2, 2, 0, 0), (4, 1, 0, 1)]:
        x = T.patch_ramp(2, 5, 6, 8, KS)
        Ho, Wo = (5 - 1 + pt) // stride + 2, (6 - 1 + pl) // stride + 2
        want = paella_cpu.patch_rows(x, KS, stride, pt, pl, Ho, Wo)
        got = T.ref_patch_rows(x, KS, stride, pt, pl, Ho, Wo)
        assert torch.equal(got, want.view_as(got))
        assert bool((S.bits(x.flatten()) == S.bits(torch.tensor([-0.0]))[0]).any()), "the ramp carries -0.0"


def test_block_references():
    c = T.block_case("randn", 2, 6, 10, 12, 5)
    y, sy = T.ref_in_block(c["img"], c["w_in"], c["b_in"])
    want = F.conv2d(F.pixel_unshuffle(c["img"].double(), 2), c["w_in"].double().t().reshape(12, 12, 1, 1), c["b_in"].double()).permute(0, 2, 3, 1)
    assert close(y, want) and bool((sy >= y.abs() - 1e-12).all())
    assert torch.equal(T.unshuffle_rows(c["img"]).permute(0, 3, 1, 2), paella_cpu.unshuffle2(c["img"]))
    img, si = T.ref_out_block(c["x"], c["w_out"], c["b_out"])
    want = F.pixel_shuffle(F.conv2d(c["x"].double().permute(0, 3, 1, 2), c["w_out"].double().reshape(12, 12, 1, 1), c["b_out"].double()), 2)
    assert close(img, want) and bool((si >= img.abs() - 1e-12).all())
    for probe in ("int", "coord"):                                  # the exact probes: the f32 model equals the float64 reference
        c = T.block_case(probe, 2, 4, 6, 8, 6)
        S.check_out(T.model_in_block(c["img"], c["w_in"], c["b_in"]), 2 * 2 * 3 * 8, T.ref_in_block(c["img"], c["w_in"], c["b_in"])[0], probe)
        S.check_out(T.model_out_block(c["x"], c["w_out"], c["b_out"]), 2 * 3 * 4 * 6, T.ref_out_block(c["x"], c["w_out"], c["b_out"])[0], probe)


def test_vq_reference():
    z, cb = S.randn((40, 5), 1), S.randn((300, 5), 2)
    idx, best, d = T.ref_vq(z, cb)
    assert close(d, paella_cpu.sqdist(z.double(), cb.double())) and torch.equal(idx, d.argmin(1)) and torch.equal(best, d.min(1).values)
    z[3], z[4] = S.NAN, 3e38
    idx, best, _ = T.ref_vq(z, cb)
    assert idx[3] == 0 and idx[4] == 0 and best[3] == math.inf and best[4] == math.inf
    assert T.vq_quarter_edges(5, 3) == [0, 1, 2, 3, 4] and T.vq_quarter_edges(2049, 4) == [0, 511, 512, 1023, 1024, 1535, 1536, 2047, 2048]
    assert T.vq_chunk(4) == 2048 and T.vq_chunk(5) == 1024
    assert T.vq_tie_pairs(8192, 4) == [(510, 513), (2046, 2049), (1537, 2050)] and T.vq_tie_pairs(8192, 4, True) == [(511, 512), (2047, 2048), (1537, 2049)]
    assert T.vq_tie_pairs(5, 3) == [] and T.vq_tie_pairs(2, 3, True) == [(0, 1)]
    for Kc, D in ((8192, 4), (2049, 4), (1025, 8), (16384, 5), (5, 3)):       # without edge ties every quarter edge keeps a winner of its own
        z, cb = T.vq_exact_case(129, D, Kc, 7)
        idx, _, d = T.ref_vq(z, cb)
        for e in T.vq_quarter_edges(Kc, D):
            rows = (idx == e).nonzero().flatten()
            assert any(int((d[r] == d[r, e]).sum()) == 1 for r in rows), (Kc, D, e)
        for a, b in T.vq_tie_pairs(Kc, D):
            assert bool(((idx == a) & (d[:, a] == d[:, b])).any()), (Kc, D, a, b)


@pytest.mark.parametrize("silu", [0, 1])
def test_spatial_norm_reference(silu):
    B, H, W, C, zh, zw, Z = 2, 6, 12, 64, 2, 4, 3
    t = T.sn_inputs(B, H, W, C, zh, zw, Z, 9)
    r = T.ref_spatial_norm(t, H, W, 32, EPS, silu)
    d = {k: v.double() for k, v in t.items()}
    want = movq_cpu.spatial_norm(d["x"].transpose(1, 2).reshape(B, C, H, W), d["zq"].permute(0, 3, 1, 2), d["gamma"], d["beta"], d["wy"], d["by"],
                                 d["wb"], d["bb"], groups=32, eps=EPS, silu=bool(silu))
    assert close(r["y"], want.reshape(B, C, H * W).transpose(1, 2), 1e-10)
    assert bool((r["Sm"] >= r["m"].abs() - 1e-12).all()) and bool((r["Sa"] >= r["a"].abs() - 1e-12).all())
    assert close(T.ref_sn_partials(t["x"], 32), S.ref_gn_partials(t["x"], 32))
    part, longest = T.sn_producer_partials(t["x"], 32, [5, 6, 40])
    assert longest == 34 and close(part.sum(1), T.ref_sn_partials(t["x"], 32).sum(1))


def test_apply_chunk_rule():
    """four cases that reach four different apply chunks, at any CU count a device of this family has"""
    for cus in (64, 256, 304):
        cases = G.sn_apix_cases(cus)
        assert sorted(cases) == sorted(G.APIX_CASES)
        for (apix, label), v in cases.items():
            assert all(T.sn_apix(B, HW, cus) == apix for B, HW in v)
            assert label == "small" or [HW for _, HW in v] == [{"2apix-1": 2 * apix - 1, "2apix": 2 * apix, "2apix+1": 2 * apix + 1}[label]]
    assert T.sn_apix(1, 1 << 20, 256) == 1024 and T.sn_apix(8, 128 * 128, 256) == 256 and T.sn_apix(4, 128 * 128, 256) == 128 and T.sn_apix(1, 100, 0) == 128
    assert [T.mix_lanes(C) for C in (4, 8, 12, 24, 252, 256, 260, 1024)] == [1, 2, 4, 8, 64, 64, 64, 64]
    assert G.SN_FACTORS and all(W % fx == 0 for _, fx, W in G.SN_FACTORS)


# ---- the contract models: clean passes every check, a defect fails at least one ---------------------------------------------------------
def checks(defect):
    """every (name, thunk) the GPU test's checks make of a model with `defect`; a thunk raises AssertionError where the check fails"""
    out = []
    E = G.E_REF
    # mix: the neighbour probe and the rounding leg, with the stats buffer
    for (B, H, W, C), oh in [((3, 2, 3, 8), True), ((3, 3, 3, 40), True), ((3, 1, 5, 24), True), ((3, 5, 1, 24), True), ((3, 2, 3, 12), False), ((2, 3, 5, 260), False)]:
        x, w9, bias, g = G.mix_case(B, H, W, C, onehot=oh)
        ref, sref, scale = T.ref_mix(x, w9, bias, g)

        def mix_check(x=x, w9=w9, bias=bias, g=g, ref=ref, sref=sref, scale=scale):
            y, st = T.model_mix(x, w9, bias, g, defect)
            T.check_rounding(y, x.numel(), ref, 4.0 * E["mix"] * scale + S.TINY, "mix")
            sb = S.check_out(st, sref.numel(), sref, "stats", values=False).view(-1, 2)
            assert S.worst_ratio(sb[:, 0], sref[:, 0], 4.0 * E["ln_mean"] * x.double().abs().view(-1, x.shape[-1]).mean(1) + S.TINY) <= 1.0, "mean"
            assert S.worst_ratio(sb[:, 1], sref[:, 1], 4.0 * E["ln_rstd"] * sref[:, 1] + S.TINY) <= 1.0, "rstd"
        out.append((f"mix {B}x{H}x{W}x{C} onehot{oh}", mix_check))
    # vq: the exact leg at the chunk and quarter edges
    for D, Kc, N, edge_ties in [(3, 5, 63, True), (4, 2049, 64, True), (2, 2047, 65, True), (5, 1025, 129, True), (8, 1023, 63, True), (1, 3, 64, True),
                                (4, 2051, 64, False), (5, 2049, 129, False), (3, 8192, 63, False)]:
        z, cb = G.vq_exact_inputs(N, D, Kc, edge_ties)

        def vq_check(z=z, cb=cb, D=D, Kc=Kc, N=N):
            body = torch.full((N, D + 1), S.NAN)
            body[:, :D] = z
            idx, dist = T.model_vq(S.place(body.flatten()[:(N - 1) * (D + 1) + D], F32, tail=0, exact=False), LEAD, D + 1, cb, N, D, Kc, defect)
            T.check_vq_exact(idx, dist, z, cb, "vq")
        out.append((f"vq exact D{D} Kc{Kc} N{N} edge_ties{int(edge_ties)}", vq_check))
    z, cb = G.vq_seeded_inputs(129, 4, 2049)
    out.append(("vq seeded", lambda: T.check_vq_seeded(*T.model_vq(S.place(z, F32, tail=0), LEAD, 4, cb, 129, 4, 2049, defect), z, cb, "vq seeded")))
    # in_block / out_block
    for probe in ("int", "coord", "randn"):
        c = T.block_case(probe, 2, 4, 6, 12, 7)
        ry, sy = T.ref_in_block(c["img"], c["w_in"], c["b_in"])
        ri, si = T.ref_out_block(c["x"], c["w_out"], c["b_out"])
        out.append((f"in_block {probe}", lambda c=c, ry=ry, sy=sy: S.check_out(
            T.model_in_block(c["img"], c["w_in"], c["b_in"], defect), ry.numel(), ry, "in_block", exact=c["exact"], bound=4.0 * E["in_block"] * sy + S.TINY)))
        out.append((f"out_block {probe}", lambda c=c, ri=ri, si=si: S.check_out(
            T.model_out_block(c["x"], c["w_out"], c["b_out"], defect), ri.numel(), ri, "out_block", exact=c["exact"], bound=4.0 * E["out_block"] * si + S.TINY)))
    # spatial norm: channels and groups, factor 3 with a coordinate-coded zq, a ragged apply chunk, offset inputs
    for (B, H, W, C, zh, zw, Z, Gr), kw in [((2, 4, 6, 32, 2, 3, 4, 32), {}), ((2, 4, 6, 128, 2, 3, 3, 64), {}), ((2, 6, 12, 32, 2, 4, 4, 32), dict(coord_zq=True)),
                                            ((2, 2, 6, 32, 2, 2, 5, 32), dict(coord_zq=True)), ((1, 1, 257, 32, 1, 1, 4, 32), {}),
                                            ((2, 8, 12, 64, 8, 3, 4, 32), dict(kind="1e3"))]:
        t = T.sn_inputs(B, H, W, C, zh, zw, Z, 11 + C, **kw)
        for silu in (0, 1):
            r = T.ref_spatial_norm(t, H, W, Gr, EPS, silu)
            bound = T.bound_spatial_norm(t, r, Gr, EPS, silu)
            out.append((f"spatial_norm {B}x{H}x{W}x{C} Z{Z} G{Gr} silu{silu} {kw}", lambda t=t, H=H, W=W, Gr=Gr, silu=silu, r=r, bound=bound: T.check_rounding(
                T.model_spatial_norm(t, H, W, Gr, EPS, silu, T.sn_apix(t["x"].shape[0], H * W, 256), defect), t["x"].numel(), r["y"], bound, "spatial_norm")))
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


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_seeded_defect_is_caught(defect):
    bad = failures(defect)
    print(f"[tokenizer_cpu] {defect}: {len(bad)} checks fail: {bad[:4]}")
    assert bad, f"no check notices the defect {defect}"


def test_defect_list():
    assert len(T.DEFECTS) >= 12 and len(set(T.DEFECTS)) == len(T.DEFECTS)
    assert all(v > 0 for v in G.E_REF.values())


def test_spatial_norm_bound_rejects_what_it_must():
    """in the float64 reference itself (no rounding at all): an eps ten times off, conv_y and conv_b exchanged, a zq source pixel one off -
    each is more than twice outside the derived bound (the planes behind a SiLU are the widest: 3.6 times for the eps), with and without the SiLU; the reference itself is inside"""
    B, H, W, C, zh, zw, Z = 2, 6, 12, 128, 2, 4, 4
    t = T.sn_inputs(B, H, W, C, zh, zw, Z, 30, coord_zq=True)
    swapped = dict(t, wy=t["wb"], by=t["bb"], wb=t["wy"], bb=t["by"])
    for silu in (0, 1):
        r = T.ref_spatial_norm(t, H, W, 32, EPS, silu)
        for planes in (False, True):
            bound = T.bound_spatial_norm(t, r, 32, EPS, silu, planes)
            assert S.worst_ratio(r["y"], r["y"], bound) == 0.0
            wrong = {"eps x 10": T.ref_spatial_norm(t, H, W, 32, 10 * EPS, silu)["y"], "conv_y / conv_b": T.ref_spatial_norm(swapped, H, W, 32, EPS, silu)["y"],
                     "source pixel": T.ref_spatial_norm(t, H, W, 32, EPS, silu, src=T.sn_source(H, W, zh, zw, "sn_src_off_f3"))["y"]}
            for what, y in wrong.items():
                w = S.worst_ratio(y, r["y"], bound)
                print(f"[tokenizer_cpu] spatial_norm {what}, silu{silu} planes{planes}: {w:.1f} x bound")
                assert w > 2.0, what
    # a producer's statistics widen the bound by the f64 allowance of their longest part only
    r = T.ref_spatial_norm(t, H, W, 32, EPS, 0)
    a, b = T.bound_spatial_norm(t, r, 32, EPS, 0), T.bound_spatial_norm(t, r, 32, EPS, 0, stat_len=H * W, stat_parts=9)
    assert bool((b >= a).all()) and float((b / a).max()) < 1.01


def test_worst_ratio_never_passes_a_nan():
    ref, bound = torch.ones(4, dtype=F64), torch.ones(4, dtype=F64)
    for bad in (S.NAN, math.inf):
        got = ref.clone()
        got[2] = bad
        assert S.worst_ratio(got, ref, bound) == math.inf
        with pytest.raises(AssertionError):
            T.check_rounding(T.storage_of(got.float()), 4, ref, bound, "nan")
    T.check_rounding(T.storage_of(ref.float()), 4, ref, bound, "clean")
    idx, dist = torch.zeros(3, dtype=torch.int64), torch.tensor([S.NAN, 0.0, 0.0])
    z = torch.tensor([[1.0], [2.0], [3.0]])
    with pytest.raises(AssertionError):
        T.check_vq_exact(idx, dist, z, z.clone(), "nan distance")


def test_vq_seeds_stay_under_the_cap():
    """the seeded leg may leave out at most 1 % of the rows (float64 gap under the f32 margin): checked here for every case of the GPU file,
    with the reference's own indices standing in for the kernel's"""
    for D in range(1, 9):
        for Kc, N, ldz in G.vq_cases(D):
            z, cb = G.vq_seeded_inputs(N, D, Kc)
            idx, best, _ = T.ref_vq(z, cb)
            T.check_vq_seeded(idx, best.float(), z, cb, f"D{D} Kc{Kc} N{N}")
