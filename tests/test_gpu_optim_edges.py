"""GPU (MI355X): the optimizer, EMA and gradient-norm kernels (csrc/optim.hip, csrc/gradnorm.hip) bit for bit against the exact CPU model of
tests/optim_cpu.py, over that module's case lists.  Every comparison is kernel against model - never one kernel form against another - and
covers the WHOLE arena a case's tensors live in, sentinel guards included.  tests/test_optim_cpu.py proves without a GPU that these cases
see every seeded defect of optim_cpu.DEFECTS.  The one exception to "bit for bit" is the float64 square root of the finalize kernel, whose
result must lie in the set the root and its two float64 neighbours round to (on the chosen slabs that set has one member)."""
import numpy as np
import pytest
import torch

import optim_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _ops():
    from muse import ops
    return ops


def up(a):
    """numpy uint32 / uint16 / float64 / int arena -> device tensor of the same bits"""
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(DEV)


def down(t, like):
    return t.cpu().numpy().view(like.dtype)


def same(got, want, what):
    if got.tobytes() != want.tobytes():
        g, w = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
        bad = np.flatnonzero((g != w).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} elements differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def factor_args(case, skip=None):
    """grad_scale / scale_dev / skip keyword arguments of an ops.adamw_* call"""
    kw = dict(skip=skip)
    if case["dev"]:
        kw["scale_dev"] = torch.tensor([case["factor"]], dtype=torch.float32, device=DEV)
    else:
        kw["grad_scale"] = case["factor"]
    return kw


class Dev:
    """a built case on the device: the f32 arena (as float32 views of the same bits) and the 16-bit arena"""

    def __init__(self, c):
        self.c, self.A, self.I = c, up(c["A"]), up(c["I"])
        self.Af = self.A.view(torch.float32)

    def t(self, rec, k, base=0, n=None):
        return self.Af[rec[k] + base:rec[k] + base + (rec["n"] - base if n is None else n)]

    def image(self, rec, base=0):
        return None if rec["img"] is None else self.I[rec["img"].pb + base:]

    def table(self, ncol):
        rows = []
        for r in self.c["recs"]:
            row = [self.A.data_ptr() + 4 * r[k] for k in "pgmv"] + [0 if r["img"] is None else self.I.data_ptr() + 2 * r["img"].pb, r["n"]]
            rows.append(row + [O.col6(r)] if ncol == 7 else row)
        cf = O.chunk_first([r["n"] for r in self.c["recs"]])
        return (torch.tensor(rows, dtype=torch.int64, device=DEV), torch.tensor(cf, dtype=torch.int32, device=DEV), len(rows), cf[-1])

    def check(self, want, what):
        torch.cuda.synchronize()
        same(down(self.A, self.c["A"]), want[0], what + " (f32 arena: p, g, m, v and their guards)")
        same(down(self.I, self.c["I"]), want[1], what + " (16-bit arena: images and their guards)")


# ---- adamw_flat -------------------------------------------------------------------------------------------------------------------------------
def _run_flat(d, case, step, skip=None):
    rec = d.c["recs"][0]
    _ops().adamw_flat(d.t(rec, "p"), d.t(rec, "g"), d.t(rec, "m"), d.t(rec, "v"), d.image(rec), *O.HYPER, step, **factor_args(case, skip))


def test_adamw_flat_small_sizes_factors_and_copy():
    for case in O.FLAT_CASES:
        if case["n"] == O.BIG:
            continue
        d = Dev(O.build_flat(case))
        for step, want in zip(case["steps"], O.run_flat(case)):
            _run_flat(d, case, step)
            d.check(want, f"{case['name']} step {step}")


@pytest.mark.parametrize("name", [c["name"] for c in O.FLAT_CASES if c["n"] == O.BIG])
def test_adamw_flat_second_sweep_and_tail(name):
    """n = 4 * 256 * 4096 + 7: the first blocks sweep twice, block 0 takes the tail"""
    case = next(c for c in O.FLAT_CASES if c["name"] == name)
    d = Dev(O.build_flat(case))
    for step, want in zip(case["steps"], O.run_flat(case)):
        _run_flat(d, case, step)
        d.check(want, f"{name} step {step}")


def test_adamw_flat_refuses_a_misaligned_bf16_copy():
    from muse._hip import MuseHipError
    case = O.SKIP_FLAT
    for dev in (False, True):
        c = O.build_flat(dict(case, dev=dev))
        d, rec = Dev(c), c["recs"][0]
        for off in (1, 2, 3):                          # 2, 4, 6 bytes off 8-byte alignment
            with pytest.raises(MuseHipError, match="alignment"):
                _ops().adamw_flat(d.t(rec, "p"), d.t(rec, "g"), d.t(rec, "m"), d.t(rec, "v"), d.I[rec["img"].pb + off:], *O.HYPER, 1,
                                  **factor_args(dict(case, dev=dev)))
        d.check((c["A"], c["I"]), "refused call")      # nothing was launched


# ---- adam_span through the multi-tensor forms -------------------------------------------------------------------------------------------------
def _run_multi(d, case, step, skip=None):
    table, cf, nt, nchunks = d.table(case["ncol"])
    if case["ncol"] == 6:
        g = case["groups"][0]
        _ops().adamw_multi(table, cf, nt, nchunks, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], step, **factor_args(case, skip))
    else:
        _ops().adamw_multi_groups(table, cf, nt, nchunks, case["groups"], step, **factor_args(case, skip))
    torch.cuda.synchronize()                           # (the table lives until the kernel has read it)


@pytest.mark.parametrize("name", [c["name"] for c in O.MULTI_CASES])
def test_adamw_multi_spans_images_groups(name):
    case = next(c for c in O.MULTI_CASES if c["name"] == name)
    d = Dev(O.build_multi(case))
    for step, want in zip(case["steps"], O.run_multi(case)):
        _run_multi(d, case, step)
        d.check(want, f"{name} step {step}")


@pytest.mark.parametrize("name", [c["name"] for c in O.ROUNDING_CASES])
def test_image_rounding_alone(name):
    """lr = 0, weight_decay = 0, g = 0: p is unchanged (the model confirms it) and the image is the rounding of chosen bit patterns"""
    case = next(c for c in O.ROUNDING_CASES if c["name"] == name)
    c = O.build_rounding(case)
    d = Dev(c)
    _run_multi(d, c, 1)
    d.check(O.run_rounding(case)[0], name)


# ---- adamw_flat_groups ----------------------------------------------------------------------------------------------------------------------
def _run_groups(d, case, step, skip=None):
    rec = d.c["recs"][0]
    ends = torch.tensor(case["seg_end"], dtype=torch.int64, device=DEV)
    grp = torch.tensor(case["seg_group"], dtype=torch.int32, device=DEV)
    for base, n in case["slices"]:
        _ops().adamw_flat_groups(d.t(rec, "p", base, n), d.t(rec, "g", base, n), d.t(rec, "m", base, n), d.t(rec, "v", base, n), d.image(rec, base),
                                 base, ends, grp, case["groups"], step, **factor_args(case, skip))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", [c["name"] for c in O.GROUP_CASES])
def test_adamw_flat_groups_segments_and_slices(name):
    case = next(c for c in O.GROUP_CASES if c["name"] == name)
    d = Dev(O.build_groups(case))
    for step, want in zip(case["steps"], O.run_groups(case)):
        _run_groups(d, case, step)
        d.check(want, f"{name} step {step}")


# ---- the skip guard ---------------------------------------------------------------------------------------------------------------------------
FORMS = {"flat": (O.SKIP_FLAT, O.build_flat, _run_flat, O.run_flat),
         "flat_groups": (O.SKIP_GROUPS, O.build_groups, _run_groups, O.run_groups),
         "multi": (O.SKIP_MULTI6, O.build_multi, _run_multi, O.run_multi),
         "multi_groups": (O.SKIP_MULTI, O.build_multi, _run_multi, O.run_multi)}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("form", list(FORMS))
def test_skip_guard(form, dev):
    """*skip != 0 leaves p, m, v and every image untouched; *skip == 0 is skip = NULL.  (The multi-tensor cases hold aligned and misaligned
    tensors; the flat forms refuse misaligned ones.)"""
    case, build, run, model = FORMS[form]
    case = dict(case, dev=dev)
    c = build(case)
    for value in O.SKIP_VALUES:
        d = Dev(c)
        run(d, case, 1, torch.tensor([value], dtype=torch.int32, device=DEV))
        d.check((c["A"], c["I"]), f"{form} skip = {value}")
    d = Dev(c)
    run(d, case, 1, torch.tensor([0], dtype=torch.int32, device=DEV))
    d.check(model(case)[0], f"{form} skip = 0")


# ---- ema_multi ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in O.EMA_CASES])
def test_ema_multi(name):
    case = next(c for c in O.EMA_CASES if c["name"] == name)
    c = O.build_ema(case)
    A = up(c["A"])
    rows = [[A.data_ptr() + 4 * r["s"], A.data_ptr() + 4 * r["p"], r["n"], int(r["copy"])] for r in c["recs"]]
    cf = O.chunk_first([r["n"] for r in c["recs"]])
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    _ops().ema_multi(table, torch.tensor(cf, dtype=torch.int32, device=DEV), len(rows), cf[-1], case["omd"])
    torch.cuda.synchronize()
    same(down(A, c["A"]), O.run_ema(case)[0][0], name)


# ---- gradient norm ------------------------------------------------------------------------------------------------------------------------------
def _slab(n):
    return torch.full((n + 8,), float("nan"), dtype=torch.float64, device=DEV)


def test_gradnorm_multi_slab():
    c = O.build_gradnorm_multi()
    A = up(c["A"])
    rows = [[0, A.data_ptr() + 4 * r["g"], 0, 0, 0, r["n"]] for r in c["recs"]]
    cf = c["cf"]
    slab = _slab(cf[-1])
    _ops().gradnorm_multi(torch.tensor(rows, dtype=torch.int64, device=DEV), torch.tensor(cf, dtype=torch.int32, device=DEV), len(rows), cf[-1], slab)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    same(got[:cf[-1]], O.model_gradnorm_multi(c), "slab")
    assert np.isnan(got[cf[-1]:]).all()
    same(down(A, c["A"]), c["A"], "gradients are read only")


def test_gradnorm_flat_slab_ranges_and_padding():
    c = O.build_gradnorm_flat()
    want = O.model_gradnorm_flat(c)
    g = torch.from_numpy(c["g"]).to(DEV)
    ptab_host = torch.tensor([[o, n] for o, n in zip(c["offs"], O.GN_FLAT_SIZES)], dtype=torch.int64)
    cf_host = torch.tensor(c["cf"], dtype=torch.int32)
    ptab, cf = ptab_host.to(DEV), cf_host.to(DEV)
    nt, nchunks = len(O.GN_FLAT_SIZES), c["cf"][-1]
    for ranges in O.GN_FLAT_RANGES:
        slab = _slab(nchunks)
        for t0, t1 in ranges:
            b = c["offs"][t0]
            e = c["offs"][t1] if t1 < nt else c["end"]
            _ops().gradnorm_flat(g, b, e - b, ptab_host, cf_host, ptab, cf, slab)
        torch.cuda.synchronize()
        got = slab.cpu().numpy()
        same(got[:nchunks], want, f"slab of ranges {ranges}")
        assert np.isnan(got[nchunks:]).all()
    # one range alone writes its own chunks only
    slab = _slab(nchunks)
    _ops().gradnorm_flat(g, c["offs"][3], c["offs"][6] - c["offs"][3], ptab_host, cf_host, ptab, cf, slab)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    same(got[c["cf"][3]:c["cf"][6]], want[c["cf"][3]:c["cf"][6]], "middle range")
    assert np.isnan(got[:c["cf"][3]]).all() and np.isnan(got[c["cf"][6]:]).all()


def _finalize(case, max_norm):
    """two launches on the same scratch -> (out of the first, out of the second, psum with the ticket)"""
    nt = len(case["cf"]) - 1
    slab = torch.from_numpy(np.concatenate([case["slab"], [np.nan] * 4])).to(DEV)
    cf = torch.tensor(case["cf"], dtype=torch.int32, device=DEV)
    psum = torch.zeros(nt + 1, dtype=torch.float64, device=DEV)
    outs = []
    for _ in range(2):
        out = up(np.full(3 + nt + 4, O.SENT32, np.uint32)).view(torch.float32)
        _ops().gradnorm_finalize(slab, cf, nt, psum, case["grad_scale"], max_norm, out)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    return outs[0], outs[1], psum.cpu().numpy()


def _check_finalize(case, max_norm):
    nt = len(case["cf"]) - 1
    out, again, psum = _finalize(case, max_norm)
    want = O.model_finalize(case["slab"], case["cf"], case["grad_scale"], max_norm)
    what = f"{case['name']} max_norm {max_norm}"
    same(out.view(np.uint32), again.view(np.uint32), what + ": the second launch on the same scratch")
    same(psum[:nt], want["psum"], what + ": per-parameter sums")
    assert psum[nt:].view(np.uint64)[0] == 0, what + ": the ticket is left at zero"
    same(out[3 + nt:].view(np.uint32), np.full(4, O.SENT32, np.uint32), what + ": guard behind out")
    if np.isnan(want["total"]):
        assert np.isnan(out[:3]).all(), what
    else:
        assert out[0].tobytes() in want["norm"], (what, out[0])
        coef, scale = O.coef_scale(out[0], case["grad_scale"], max_norm)
        if np.isnan(coef):
            assert np.isnan(out[1]) and np.isnan(out[2]), what
        else:
            same(out[1:3], np.array([coef, scale], F), what + ": coef, scale")
    for t in range(nt):
        if np.isnan(want["psum"][t]):
            assert np.isnan(out[3 + t])
        else:
            assert out[3 + t].tobytes() in want["per"][t], (what, t, out[3 + t])


def test_gradnorm_finalize_fold_tiles_and_ticket():
    for case in O.finalize_cases():
        if not case["name"].split("-")[1] in O.FIN_SPECIAL:
            _check_finalize(case, 1e9 if case["name"] != "fin-chunks" else 0.5)


def test_gradnorm_finalize_coefficient_edges():
    """norm 0, an infinite norm (an inf entry; a finite total whose root overflows f32), a NaN entry, each with max_norm 0.5, 1e9 and inf
    (inf / inf included)"""
    for case in O.finalize_cases():
        if case["name"].split("-")[1] in O.FIN_SPECIAL:
            for max_norm in O.FIN_MAX_NORMS:
                _check_finalize(case, max_norm)


# ---- grad_scale ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", O.GS_FACTORS)
def test_grad_scale_flat_and_multi(factor):
    c = O.build_grad_scale()
    want = O.model_grad_scale(c, factor)
    scale = torch.tensor([factor], dtype=torch.float32, device=DEV)
    A = up(c["A"])
    Af = A.view(torch.float32)
    for r in c["recs"]:
        if r["n"]:
            _ops().grad_scale_flat_(Af[r["g"]:r["g"] + r["n"]], scale)
    torch.cuda.synchronize()
    same(down(A, c["A"]), want, f"grad_scale_flat_ x {factor}")
    A = up(c["A"])
    rows = [[0, A.data_ptr() + 4 * r["g"], 0, 0, 0, r["n"]] for r in c["recs"]]
    _ops().grad_scale_multi_(torch.tensor(rows, dtype=torch.int64, device=DEV), torch.tensor(c["cf"], dtype=torch.int32, device=DEV), len(rows),
                             c["cf"][-1], scale)
    torch.cuda.synchronize()
    same(down(A, c["A"]), want, f"grad_scale_multi_ x {factor}")
