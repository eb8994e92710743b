"""CPU: the exact model of the optimizer kernels (tests/optim_cpu.py) checks itself - fmaf against rational arithmetic, the update against
torch.optim.AdamW in float64, the image roundings at their ties - and proves that the case lists the GPU module walks
(tests/test_gpu_optim_edges.py) see every seeded defect of optim_cpu.DEFECTS.  Nothing here needs a GPU."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import optim_cpu as O

F = np.float32


# ---- fmaf -----------------------------------------------------------------------------------------------------------------------------------
def f32_of_fraction(q):
    """round a rational to f32, nearest even, subnormals and overflow to inf"""
    if q == 0:
        return 0.0
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    k, rem = divmod(q, quantum)
    k = int(k)
    if rem * 2 > quantum or (rem * 2 == quantum and k & 1):
        k += 1
    val = k * quantum
    return sign * (float("inf") if val >= Fraction(2) ** 128 else float(val))


def _hard_family():
    """c = +-(1 + k 2^-23), a = 1 + 2^-23, b = +-(1 - 2^-23) 2^-24: a b is just below half an ulp of c, and c + a b in float64 rounds ONTO the
    f32 midpoint, which the second rounding then resolves by the tie rule instead of by the product's true size"""
    k = np.arange(1000)
    c = (1.0 + k * 2.0 ** -23).astype(F)
    a = np.full(1000, 1.0 + 2.0 ** -23, F)
    b = np.full(1000, (1.0 - 2.0 ** -23) * 2.0 ** -24, F)
    return (np.concatenate([a, a, a, a]), np.concatenate([b, -b, b, -b]), np.concatenate([c, c, -c, -c]))


def _random_family(n, seed):
    r = np.random.default_rng(seed)

    def draw(lo, hi):
        return ((r.random(n) + 1.0) * np.where(r.random(n) < 0.5, -1, 1) * np.exp2(r.integers(lo, hi, n).astype(np.float64))).astype(F)
    a, b = draw(-20, 20), draw(-20, 20)
    c = draw(-45, 45)
    near = r.random(n) < 0.5                     # half of them: c cancels most of the product
    c[near] = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + r.integers(-3, 4, n) * 2.0 ** -22)).astype(F)[near]
    return a, b, c


def _fraction_check(a, b, c):
    got = O.fmaf(a, b, c)
    bad = 0
    for x, y, z, w in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        bad += f32_of_fraction(Fraction(x) * Fraction(y) + Fraction(z)) != w
    return bad


def test_fmaf_against_fraction_on_the_double_rounding_family():
    a, b, c = _hard_family()
    assert _fraction_check(a, b, c) == 0
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    wrong = int((naive != O.fmaf(a, b, c)).sum())
    print("float32(a * b + c) in float64 is wrong on", wrong, "of", len(a))
    assert wrong >= 400                          # the family has teeth: the plain float64 expression fails on a large part of it


def test_fmaf_against_fraction_random_subnormal_and_overflow():
    assert _fraction_check(*_random_family(12000, 0)) == 0
    r = np.random.default_rng(9)
    tiny = ((r.random(4000) + 1.0) * np.exp2(r.integers(-80, -60, 4000).astype(np.float64))).astype(F)          # products in the subnormal range
    assert _fraction_check(tiny, tiny[::-1].copy(), (tiny * F(2.0 ** -70)).astype(F) * F(-1)) == 0
    big = ((r.random(4000) + 1.0) * np.exp2(r.integers(60, 64, 4000).astype(np.float64))).astype(F)             # around FLT_MAX
    assert _fraction_check(big, big[::-1].copy(), -big) == 0


def test_bf16_and_half_roundings_against_torch():
    x = O.rounding_patterns()
    t = torch.from_numpy(x.copy())
    assert np.array_equal(O.bf16_bits(x), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(O.half_bits(x), t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    hi = O.bf16_f32(O.bf16_bits(x))
    with np.errstate(all="ignore"):
        lo = x - hi
    fin = np.isfinite(lo)
    ties = ((lo[fin].view(np.uint32) & 0xFFFF) == 0x8000).sum()
    assert ties >= 20, ties                       # the lo plane is rounded at true ties, under even and odd upper halves
    assert ((x.view(np.uint32) & 0xFFFF) == 0x8000).sum() >= 8


# ---- the update against torch.optim.AdamW in float64 ----------------------------------------------------------------------------------------
def _torch_adamw64(p, g, m, v, hyper, step):
    lr, b1, b2, eps, wd = (float(F(x)) for x in hyper)
    P = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    P.grad = torch.from_numpy(g.astype(np.float64))
    opt = torch.optim.AdamW([P], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                        exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
    opt.step()
    st = opt.state[P]
    return P.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("dev", [False, True])
def test_model_update_against_torch_adamw_float64(dev):
    """A few f32 ulp per step.  Each of the model's roundings errs by 2^-24 of its own result; the bounds below carry that through the
    expressions: m' is a sum of terms up to |m| + |g s|, v' is a sum of positive terms, and p' = decay p - t with t = step_size m' / denom
    inherits m's absolute error divided by denom."""
    u, tiny = 2.0 ** -24, 2.0 ** -149
    worst = 0.0
    for case in O.FLAT_CASES:
        if case["n"] > 1025 or case["dev"] != dev:
            continue
        c = O.build_flat(case)
        rec = c["recs"][0]
        for step in O.STEPS:
            p, g, m, v = (x.copy() for x in O._views(c["A"], rec))
            h = O.adam_hyper(*O.HYPER, step)
            p1, m1, v1 = O.update1(p, g, m, v, h, case["factor"], dev)
            gs = g.astype(np.float64) * float(F(case["factor"]))
            rp, rm, rv = _torch_adamw64(p, gs, m, v, O.HYPER, step)
            em = 4 * u * (np.abs(m) + np.abs(gs)) + tiny
            assert np.all(np.abs(m1 - rm) <= em)
            assert np.all(np.abs(v1 - rv) <= 4 * u * rv + 4 * tiny)
            denom = np.sqrt(rv) / float(h["bc2_sqrt"]) + float(h["eps"])
            t = float(h["step_size"]) * (np.abs(m) + np.abs(gs)) / denom
            ep = 8 * u * (np.abs(p) + t) + tiny
            assert np.all(np.abs(p1 - rp) <= ep), case["name"]
            worst = max(worst, float(np.max(np.abs(p1 - rp) / ep)))
            O.model_flat(c["A"], c["I"], rec, O.HYPER, step, case["factor"], dev)
    print("worst error / bound", worst)


def test_model_groups_against_torch_adamw_float64():
    """the eight hyper-parameter sets of the grouped cases (beta1 = 0, weight_decay = 1, eps = 1e-3 among them), bounds as above"""
    u, tiny = 2.0 ** -24, 2.0 ** -149
    case = next(c for c in O.MULTI_CASES if c["name"] == "multi7-sizes-8groups")
    c = O.build_multi(case)
    for step in O.STEPS:
        H = O.fill_groups(case["groups"], step)
        for rec in c["recs"]:
            p, g, m, v = (x.copy() for x in O._views(c["A"], rec))
            G = case["groups"][rec["group"]]
            hyper = (G["lr"], G["betas"][0], G["betas"][1], G["eps"], G["weight_decay"])
            h = H[rec["group"]]
            p1, m1, v1 = O.update1(p, g, m, v, h, case["factor"], False)
            gs = g.astype(np.float64) * float(F(case["factor"]))
            rp, rm, rv = _torch_adamw64(p, gs, m, v, hyper, step)
            assert np.all(np.abs(m1 - rm) <= 4 * u * (np.abs(m) + np.abs(gs)) + tiny)
            assert np.all(np.abs(v1 - rv) <= 4 * u * rv + 4 * tiny)
            denom = np.sqrt(rv) / float(h["bc2_sqrt"]) + float(h["eps"])
            t = float(h["step_size"]) * (np.abs(m) + np.abs(gs)) / denom
            assert np.all(np.abs(p1 - rp) <= 8 * u * (np.abs(p) + t) + tiny), (rec["n"], rec["group"], step)


def test_hyper_rows_and_col6():
    H = O.fill_groups(O.GROUPS8[1:4], 7)
    assert len(H) == 8 and all(H[k] is H[0] for k in range(3, 8)) and H[1]["b2"] == F(0.99)
    rec = dict(img=O.Img(0, 0, True), group=5)
    c6 = O.col6(rec)
    assert c6 < 0 and (c6 & 7) == 5 and (c6 >> 8) < 0
    assert O.col6(dict(img=O.Img(0, 1029), group=7)) == (1029 << 8) | 7 and O.col6(dict(img=None, group=2)) == 2
    assert O.adam_hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, 100000)["step_size"] == F(1e-3)     # beta1^100000 underflows to zero


def test_rounding_cases_leave_the_parameter_unchanged():
    """lr = 0, weight_decay = 0, g = 0: p' = fma(1, p, -0) = p bit for bit, -0 included, so the image is the rounding of a chosen pattern"""
    for case in O.ROUNDING_CASES:
        c = O.build_rounding(case)
        before = c["A"].copy()
        rec = c["recs"][0]
        (A, I), = O.run_rounding(case)
        assert np.array_equal(A[rec["p"]:rec["p"] + rec["n"]], before[rec["p"]:rec["p"] + rec["n"]])
        p = O.f32view(A, rec["p"], rec["n"])
        assert (p.view(np.uint32) == 0x80000000).any() and (p.view(np.uint32) == 0).any()
        want = O.half_bits(p) if case["image"] == "half" else O.bf16_bits(p)
        assert np.array_equal(I[rec["img"].pb:rec["img"].pb + rec["n"]], want)
        vec = O._aligned([rec[k] for k in "pgmv"], rec["img"])
        assert vec == (case["path"] == "quad") and rec["n"] % 4 == 0


# ---- dispatch models --------------------------------------------------------------------------------------------------------------------------
def test_cover_models_partition_their_range():
    for n in (1, 3, 4, 5, 1023, 1025, O.BIG):
        q, t = O.flat_cover(n)
        assert (q.start, q.stop, t.start, t.stop) == (0, n & ~3, n & ~3, n)
    assert O.ew_grid((O.BIG + 3) // 4) == 4096 and (O.BIG >> 2) > 4096 * 256           # the big case needs a second sweep
    for lo, hi in ((0, 1), (0, 4096), (4096, 4097), (4096, 8191), (8192, 8193)):
        for vec in (False, True):
            a, b = O.span_cover(lo, hi, vec)
            assert np.array_equal(np.sort(np.concatenate([a, b])), np.arange(lo, hi))
    ends = [100, 100, 5000, 5000, 5000, 8195]
    assert [O.seg_of(ends, p) for p in (0, 99, 100, 4999, 5000, 8194, 9000)] == [0, 0, 2, 2, 5, 5, 5]
    cf = O.chunk_first([0, 4097, 0, 0, 5, 4096, 0])
    assert [O.tensor_of_chunk(cf, 0, 7, c) for c in range(cf[-1])] == [1, 1, 4, 5]


# ---- every defect is seen by a named case of the GPU case lists ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _good(name):
    return O.run_case(name)


def _differs(a, b):
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


def test_catch_table_names_every_defect():
    assert set(O.CATCH) == set(O.DEFECTS) and len(set(O.DEFECTS)) == len(O.DEFECTS) >= 28
    assert all(len(v) >= 1 for v in O.CATCH.values())


@pytest.mark.parametrize("defect", O.DEFECTS)
def test_defect_is_caught_by_its_cases(defect):
    for name in O.CATCH[defect]:
        assert _differs(_good(name), O.run_case(name, defect)), (defect, name)


def test_model_without_defect_is_deterministic():
    for name in ("multi7-sizes-8groups", "groups-slices", "gradnorm-flat"):
        assert not _differs(_good(name), O.run_case(name))


# ---- gradient norm ------------------------------------------------------------------------------------------------------------------------------
def test_gradnorm_model_order_shows():
    """on the chosen values the tree of chunk_sumsq is NOT a plain sequential float64 sum: a kernel that summed in another order would differ
    (all tensors of 1023 elements and more but the one that holds FLT_MAX, whose three largest squares swamp every order)"""
    c = O.build_gradnorm_multi()
    shown = 0
    for r in c["recs"][:-3] + c["recs"][-2:]:
        x = O.f32view(c["A"], r["g"], r["n"]).astype(np.float64)
        slab = O.tensor_slab(x.astype(F))
        seq = np.array([np.add.accumulate(x[k:k + O.CHUNK] ** 2)[-1] for k in range(0, r["n"], O.CHUNK)])
        assert np.all(np.abs(slab - seq) <= 1e-12 * seq)
        if r["n"] >= 1023:
            assert slab[0] != seq[0], r
            shown += 1
    assert shown >= 30
    f = O.build_gradnorm_flat()
    assert np.array_equal(O.model_gradnorm_flat(f), O.model_gradnorm_flat(O.build_gradnorm_flat(0.0)))      # padding belongs to nobody
    assert all(o % 2 == 1 or o % 4 for o in f["offs"][:2])


def test_finalize_model_fold_and_norm_sets():
    multi = total = 0
    for c in O.finalize_cases():
        r = O.model_finalize(c["slab"], c["cf"], c["grad_scale"], 1e9)
        sets = r["per"] + [r["norm"]]
        total += len(sets)
        multi += sum(len(s) > 1 for s in sets)
        if c["name"] == "fin-chunks":
            for t in (5, 6, 7, 8):               # the order of the fold shows: numpy's pairwise sum differs from the sequential one
                seg = c["slab"][c["cf"][t]:c["cf"][t + 1]]
                assert r["psum"][t] != np.sum(seg) or r["psum"][t] != np.sum(seg[::-1])
    print("norm sets with more than one member:", multi, "of", total)
    assert multi == 0 and total > 4000          # on the chosen slabs the float64 root's last bit never reaches the f32 rounding
    assert O.coef_scale(F(0), 1.0, 0.5) == (F(1), F(1))
    coef, scale = O.coef_scale(F(np.inf), 1.0, np.inf)
    assert np.isnan(coef) and np.isnan(scale)
    assert O.coef_scale(F(np.inf), 0.5, 1e9) == (F(0), F(0))
    assert O.coef_scale(F(3.0), 0.25, 0.5)[0] == F(0.5) / (F(3.0) + F(1e-6))
