"""CPU side of the Lion tests (tests/test_lion_cpu.py, tests/test_gpu_lion.py): the exact numpy model of the Lion instantiations of
csrc/optim.hip, with switchable seeded defects, the case lists both test modules walk and the builders of their inputs.

The kernels are AdamW's with the update rule swapped, and so is this model: who updates which element, the image stores and the skip
guard are tests/optim_cpu.py's `model_flat`, `model_flat_groups` and `model_multi`, run under `lion_rule()` - which puts Lion's constants
and Lion's update of one element in the place of AdamW's for the duration of a call.  Nothing of the dispatch is restated here, and the
dispatch and image defects of optim_cpu.DEFECTS apply to the Lion instantiations under their own names.

The pinned update of one element (lion_update1 of csrc/optim.hip; s = the gradient factor, host or device - the same statements):
    gr = round(g * s)
    p1 = round(p * decay)
    u  = round(round(m * b1) + round(gr * omb1))
    p' = round(p1 + nlr * sign(u))        sign: +1, -1, +0 for u == +-0, NaN for NaN
    m' = fma(omb2, gr, round(m * b2))
with decay = f32(1 - lr wd), b1 = f32(beta1), omb1 = f32(1 - beta1), b2 = f32(beta2), omb2 = f32(1 - beta2), nlr = f32(-lr), each computed
in double from the Python floats and rounded once.  There is no second moment: the `v` of a record is a region the kernels must leave alone.
"""
import contextlib
import functools

import numpy as np

import optim_cpu as O
from optim_cpu import CHUNK, F, SENT32, Arena, chunk_first, col6, f32view, fmaf   # noqa: F401  (the GPU module takes them from here)

UPDATE_DEFECTS = ("momentum_not_fused", "update_from_new_m", "reuses_m_b1", "decay_not_rounded", "decay_after_step", "sign_zero_as_plus",
                  "sign_nan_as_zero", "minus_zero_lost", "factor_not_rounded", "v_touched")
# what the Lion instantiations of the shared dispatch could get wrong on their own (the names and the seeded code are optim_cpu's)
DISPATCH_DEFECTS = ("flat_tail_dropped", "span_last_quad_dropped", "span_tail_from_hi", "boundary_chunk_first_group", "base_ignored",
                    "seg_of_off_by_one", "group_wrong_row", "lo_from_p", "lo_wrong_distance", "half_through_bf16", "image_on_skip",
                    "skip_vector_only")
DEFECTS = UPDATE_DEFECTS + DISPATCH_DEFECTS


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
def lion_hyper(lr, beta1, beta2, weight_decay, step=None):
    """the host's constants (lion_hyper of csrc/optim.hip): double arithmetic on the Python floats, each constant rounded once"""
    lr, beta1, beta2, weight_decay = float(lr), float(beta1), float(beta2), float(weight_decay)
    return dict(decay=F(1.0 - lr * weight_decay), b1=F(beta1), omb1=F(1.0 - beta1), b2=F(beta2), omb2=F(1.0 - beta2), nlr=F(-lr))


def fill_groups(groups, step=None):
    H = [lion_hyper(g["lr"], g["betas"][0], g["betas"][1], g["weight_decay"]) for g in groups]
    return H + [H[0]] * (8 - len(H))


def update1(p, g, m, h, s, defect=None):
    """one Lion update of float32 arrays -> (p', m')"""
    s = F(s)
    p, g, m = (np.asarray(x, F) for x in (p, g, m))
    with np.errstate(all="ignore"):
        gr = g * s
        if defect == "factor_not_rounded":                 # g * s kept unrounded into both of its uses
            gs = g.astype(np.float64) * np.float64(s)
            b = (gs * np.float64(h["omb1"])).astype(F)
        else:
            b = gr * h["omb1"]
        mb = m * (h["b1"] if defect == "reuses_m_b1" else h["b2"])
        if defect == "factor_not_rounded":
            m1 = (np.float64(h["omb2"]) * gs + mb.astype(np.float64)).astype(F)
        elif defect == "momentum_not_fused":
            m1 = (h["omb2"] * gr + mb).astype(F)
        else:
            m1 = fmaf(h["omb2"], gr, mb)
        u = ((m1 if defect == "update_from_new_m" else m) * h["b1"] + b).astype(F)
        zero = F(1.0) if defect == "sign_zero_as_plus" else F(0.0)
        sg = np.where(u > 0, F(1.0), np.where(u < 0, F(-1.0), np.where(u == 0, zero, F(0.0) if defect == "sign_nan_as_zero" else u))).astype(F)
        t = (h["nlr"] * sg).astype(F)
        if defect == "minus_zero_lost":
            t = np.where(u == 0, F(0.0), t).astype(F)      # +0 added in place of nlr * 0 = -0: -0.0 + 0.0 = +0.0
        if defect == "decay_after_step":
            p1 = ((p + t) * h["decay"]).astype(F)
        elif defect == "decay_not_rounded":
            p1 = fmaf(p, h["decay"], t)
        else:
            p1 = (p * h["decay"] + t).astype(F)
    return p1.astype(F), m1.astype(F)


def _update1_in_adams_place(p, g, m, v, h, s, dev, defect=None):
    p1, m1 = update1(p, g, m, h, s, defect)
    if defect == "v_touched":                              # a store of the second moment the rule does not have
        return p1, m1, np.zeros_like(p1)
    return p1, m1, v


@contextlib.contextmanager
def lion_rule():
    """optim_cpu's dispatch models with Lion's rule in the place of AdamW's: `hyper` tuples are (lr, beta1, beta2, weight_decay), groups
    carry no eps, and the step number the models pass along is ignored"""
    saved = O.adam_hyper, O.fill_groups, O.update1
    O.adam_hyper, O.fill_groups, O.update1 = lion_hyper, fill_groups, _update1_in_adams_place
    try:
        yield
    finally:
        O.adam_hyper, O.fill_groups, O.update1 = saved


# ---- which NaN: IEEE 754 leaves sign and payload of a NaN result open, and the host and the GPU choose differently; the comparisons of both
# test modules therefore map every NaN a kernel may produce to one pattern first (the sentinels, NaNs with a payload of their own, stay exact)
def canon32(a):
    """uint32 arena with every NaN but the sentinel mapped to one pattern"""
    a = a.copy()
    a[np.isnan(a.view(F)) & (a != SENT32)] = 0x7FC00000
    return a


def canon_images(I, recs):
    """uint16 arena with every NaN inside an image (bf16 planes or a half copy) mapped to one pattern"""
    I = I.copy()
    for r in recs:
        im = r["img"]
        if im is None or r["n"] == 0:
            continue
        for start in (im.pb,) + ((im.pb + im.plo,) if im.plo else ()):
            w = I[start:start + r["n"]]
            nan = ((w & 0x7C00) == 0x7C00) & ((w & 0x03FF) != 0) if im.half else ((w & 0x7F80) == 0x7F80) & ((w & 0x007F) != 0)
            w[nan] = 0x7E00 if im.half else 0x7FC0
    return I


# ---- values -------------------------------------------------------------------------------------------------------------------------------
HYPER = (1e-2, 0.9, 0.99, 0.1)                          # lr, beta1, beta2, weight_decay
GROUPS3 = [dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.1), dict(lr=3e-3, betas=(0.95, 0.98), weight_decay=0.0),
           dict(lr=1e-4, betas=(0.5, 0.9), weight_decay=0.3)]
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3)
STEPS = 2                                               # launches per case: the second one runs on the first one's m
SENTF = np.array([SENT32], np.uint32).view(F)[0]


def _plants(betas):
    """(p, g, m) of the special elements: u == 0 with g = 0 and m = 0; p = -0.0 with g = 0; m b1 against g omb1 at 0, 1, 2 ulp for each
    of `betas`; a NaN gradient; +-inf in g, p and m; f32 denormals in p, g and m"""
    sub = F(2.0 ** -140)
    out = [(F(0.75), F(0), F(0)), (F(-0.0), F(0), F(0)), (F(-0.0), F(0), F(-0.0)), (F(1.5), F(np.nan), F(0.25)), (F(1.5), F(np.inf), F(0.25)),
           (F(1.5), F(-np.inf), F(-0.25)), (F(np.inf), F(0.5), F(0.25)), (F(2.0), F(0.5), F(-np.inf)), (sub, F(0.5), F(0.25)), (F(-3.0) * sub, F(0), F(0)),
           (F(0.5), sub, F(0)), (F(0.5), F(-5.0) * sub, F(3.0) * sub), (F(0.5), F(0), F(7.0) * sub), (F(0), F(0), F(0))]
    for b1 in betas:
        for k, m in enumerate((F(0.37), F(-1.21e-3), F(5.5))):
            with np.errstate(all="ignore"):
                g = F(-F(m * F(b1)) / F(1.0 - b1))
            for _ in range(k):
                g = np.nextafter(g, F(0))
            out.append((F(-0.6), g, m))
            out.append((F(0.6), np.nextafter(g, F(np.sign(g) * np.inf)), m))
    return out


@functools.lru_cache(maxsize=None)
def values(n, seed):
    """p, g, m of one tensor (v: the sentinel, a region no Lion kernel may touch).  Tensors of 64 elements and more carry every plant,
    from element 1 on; smaller ones as many as fit, beginning at a plant that depends on the seed."""
    r = np.random.default_rng(seed)
    p = (r.standard_normal(n) * np.exp2(r.integers(-6, 5, n))).astype(F)
    g = ((r.random(n) + 1.0) * np.where(r.random(n) < 0.5, -1, 1) * np.exp2(r.integers(-30, 20, n).astype(np.float64))).astype(F)
    m = ((r.random(n) + 0.25) * np.where(r.random(n) < 0.5, -1, 1) * np.exp2(r.integers(-30, 20, n).astype(np.float64))).astype(F)
    g[r.random(n) < 0.05] = 0.0
    m[r.random(n) < 0.05] = 0.0
    plants = _plants(sorted({HYPER[1]} | {G["betas"][0] for G in GROUPS3}))
    if n >= 64:
        assert len(plants) < 63
        where = [(1 + k, k) for k in range(len(plants))]
    else:
        where = [(i, (seed + i) % len(plants)) for i in range(n)]
    for i, k in where:
        p[i], g[i], m[i] = plants[k]
    return p, g, m, np.full(n, SENTF, F)


def _rec(A32, A16, n, seed, image="none", mis=None, plo_extra=0, group=0):
    rec = O._place_tensor(A32, A16, n, seed, image, mis, 0, plo_extra, group)
    rec["values"] = values(n, seed)
    return rec


# ---- regimes: every form runs under each ---------------------------------------------------------------------------------------------------
THIRD = float(F(1.0) / F(3.0))
REGIMES = {                       # name: (factor, device factor, skip counter or None)
    "host_half": (0.5, False, None), "host_third": (THIRD, False, None), "dev_third": (THIRD, True, None),
    "skip_zero": (THIRD, False, 0), "skip_set": (THIRD, False, 3),
}


# ---- cases: dict(name, form, ...) ; build(case) -> dict with A, I, recs ; run(case, regime, defect) -> [(A, I) after each launch] ------------
def _flat_case(n, image, cuts):
    return dict(name=f"flat-n{n}-{'bf16' if image else 'none'}-{'x'.join(map(str, cuts)) or 'one'}", form="flat", n=n, image=image,
                ranges=list(zip((0,) + cuts, cuts + (n,))))


FLAT_CASES = [_flat_case(n, image, ()) for n in SIZES for image in (False, True)]
FLAT_CASES += [_flat_case(n, image, cuts) for n, cuts in ((4097, (4, 4092)), (2 * 4096 + 3, (1028, 4096))) for image in (False, True)]

# three groups, boundaries inside a chunk and off a multiple of 4; whole, in three ranges, and a slice with base != 0
_SEG = dict(seg_end=[1001, 4099, 6001, 2 * 4096 + 3], seg_group=[0, 1, 2, 0])
GROUP_CASES = [dict(name=f"groups-{tag}", form="flat_groups", total=2 * 4096 + 3, slices=sl, image=image, **_SEG)
               for tag, sl, image in (("whole", [(0, 2 * 4096 + 3)], True), ("whole-none", [(0, 2 * 4096 + 3)], False),
                                      ("ranges", [(0, 1000), (1000, 3100), (4100, 4095)], True), ("base", [(996, 4104)], True))]
GROUP_CASES += [dict(name=f"groups-n{n}", form="flat_groups", total=n, slices=[(0, n)], image=True, seg_end=[max(1, n // 2), n], seg_group=[2, 1])
                for n in (1, 3, 4, 5, 4095, 4096, 4097)]

IMAGES7 = ("none", "bf16", "x3", "x3odd", "half")


def _multi_case(name, ncol, tensors, v="region"):
    return dict(name=name, form="multi", ncol=ncol, tensors=tensors, v=v)


def _tensors(ncol, rot):
    ts = []
    for i, n in enumerate(SIZES + (2 * 4096 + 1, 7)):
        image = IMAGES7[(i + rot) % 5] if ncol == 7 else ("none", "bf16")[(i + rot) % 2]
        ts.append(dict(n=n, image=image, group=i % 3 if ncol == 7 else 0, mis={"p": 4, "g": 4, "m": 4} if i == 6 else None))
    return ts


MULTI_CASES = [_multi_case(f"multi{ncol}-rot{rot}", ncol, _tensors(ncol, rot)) for ncol, rots in ((6, 2), (7, 5)) for rot in range(rots)]
MULTI_CASES += [_multi_case(f"multi{ncol}-v-null", ncol, _tensors(ncol, 1), v="null") for ncol in (6, 7)]
MULTI_CASES += [_multi_case("multi7-one-role-off", 7, [dict(n=4097, image=IMAGES7[1 + j], group=j % 3, mis={k: 4}) for j, k in enumerate("pgm")])]
CASES = FLAT_CASES + GROUP_CASES + MULTI_CASES


def build(case):
    A32, A16 = Arena(4), Arena(2)
    if case["form"] == "flat":
        recs = [_rec(A32, A16, case["n"], 9100 + case["n"] % 977, "bf16" if case["image"] else "none")]
    elif case["form"] == "flat_groups":
        recs = [_rec(A32, A16, case["total"], 9300 + case["total"] % 907, "bf16" if case["image"] else "none")]
    else:
        recs = [_rec(A32, A16, t["n"], 9500 + 31 * i + t["n"] % 911, "x3" if t["image"] == "x3odd" else t["image"], t["mis"],
                     1 if t["image"] == "x3odd" else 0, t["group"]) for i, t in enumerate(case["tensors"])]
    return O._finish(dict(case), A32, A16, recs)


def groups_of(case):
    return GROUPS3 if case["form"] == "flat_groups" or case.get("ncol") == 7 else GROUPS3[:1]


def run(case, regime, defect=None, steps=STEPS):
    """the model's arenas after each of `steps` launches of the case under the regime -> [(A, I), ...]"""
    factor, dev, skip = REGIMES[regime]
    c = build(case)
    out = []
    with lion_rule():
        for step in range(steps):
            if case["form"] == "flat":
                rec = c["recs"][0]
                for b, e in case["ranges"]:             # a range of the single-set form is a call on the slices
                    sub = dict(rec, n=e - b, img=None if rec["img"] is None else O.Img(rec["img"].pb + b), **{k: rec[k] + b for k in "pgmv"})
                    O.model_flat(c["A"], c["I"], sub, HYPER, step, factor, dev, skip, defect)
            elif case["form"] == "flat_groups":
                for base, n in case["slices"]:
                    O.model_flat_groups(c["A"], c["I"], c["recs"][0], base, n, case["seg_end"], case["seg_group"], GROUPS3, step, factor, dev, skip,
                                        defect)
            else:
                O.model_multi(c["A"], c["I"], c["recs"], case["ncol"], groups_of(case), step, factor, dev, skip, defect)
            out.append((c["A"].copy(), c["I"].copy()))
    return out
