"""GPU (MI355X): the Lion instantiations of csrc/optim.hip and muse.FusedLion bit for bit against the exact CPU model of tests/lion_cpu.py.
Kernel level: every case of lion_cpu.CASES under every regime (host factor 0.5 and 1/3, device factor 1/3, `skip` at a zero and at a non-zero
counter), the WHOLE arenas compared, sentinel guards and the never-touched `v` regions included; tests/test_lion_cpu.py proves without a GPU
that these runs see every seeded defect.  The reference's recorded steps (tests/golden/lion_steps.npz) replayed through muse.FusedLion.  Model
level: muse.FusedLion on a flat-engine MaskGitTransformer and on a MaskGiTUViT with ordinary parameters, stepped in lockstep with the model on
the host from the device's own gradient bytes.

One thing is not compared bit for bit: WHICH NaN.  IEEE 754 leaves sign and payload of a NaN result to the implementation, the host the model
runs on and the GPU choose differently (inf - inf, a NaN through a multiply), and the inputs hold NaN and inf on purpose.  So every NaN a kernel
may produce - a NaN that is not the arena's sentinel - is compared as "a NaN here" (lion_cpu.canon32 / canon_images, which the CPU proof that
these runs see every defect applies too), and everything else, sentinels included, to the bit."""
import json
import os

import numpy as np
import pytest
import torch

import lion_cpu as L
import optim_cpu as O
import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _ops():
    from muse import ops
    return ops


def up(a):
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(DEV)


def same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} elements differ, first at {bad[0]}: got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


class Dev:
    """a built case on the device: the f32 arena (as float32 views of the same bits) and the 16-bit arena"""

    def __init__(self, c):
        self.c, self.A, self.I = c, up(c["A"]), up(c["I"])
        self.Af = self.A.view(torch.float32)

    def t(self, rec, k, b=0, e=None):
        return self.Af[rec[k] + b:rec[k] + (rec["n"] if e is None else e)]

    def image(self, rec, b=0):
        return None if rec["img"] is None else self.I[rec["img"].pb + b:]

    def table(self, ncol, v):
        rows = []
        for r in self.c["recs"]:
            row = [self.A.data_ptr() + 4 * r[k] for k in "pgm"] + [self.A.data_ptr() + 4 * r["v"] if v == "region" else 0,
                                                                  0 if r["img"] is None else self.I.data_ptr() + 2 * r["img"].pb, r["n"]]
            rows.append(row + [L.col6(r)] if ncol == 7 else row)
        cf = L.chunk_first([r["n"] for r in self.c["recs"]])
        return torch.tensor(rows, dtype=torch.int64, device=DEV), torch.tensor(cf, dtype=torch.int32, device=DEV), len(rows), cf[-1]

    def check(self, want, what):
        torch.cuda.synchronize()
        recs = self.c["recs"]
        same(L.canon32(self.A.cpu().numpy().view(np.uint32)), L.canon32(want[0]), what + " (f32 arena: p, g, m, the untouched v regions and the guards)")
        same(L.canon_images(self.I.cpu().numpy().view(np.uint16), recs), L.canon_images(want[1], recs), what + " (16-bit arena: images and their guards)")


def launch(d, case, regime):
    """one launch (the flat form in ranges: one per range) of the case under the regime"""
    ops = _ops()
    factor, dev, skip = L.REGIMES[regime]
    kw = dict(skip=None if skip is None else torch.tensor([skip], dtype=torch.int32, device=DEV))
    if dev:
        kw["scale_dev"] = torch.tensor([factor], dtype=torch.float32, device=DEV)
    else:
        kw["grad_scale"] = factor
    rec = d.c["recs"][0]
    if case["form"] == "flat":
        for b, e in case["ranges"]:
            ops.lion_flat(d.t(rec, "p", b, e), d.t(rec, "g", b, e), d.t(rec, "m", b, e), d.image(rec, b), *L.HYPER, **kw)
    elif case["form"] == "flat_groups":
        ends = torch.tensor(case["seg_end"], dtype=torch.int64, device=DEV)
        grp = torch.tensor(case["seg_group"], dtype=torch.int32, device=DEV)
        for base, n in case["slices"]:
            ops.lion_flat_groups(d.t(rec, "p", base, base + n), d.t(rec, "g", base, base + n), d.t(rec, "m", base, base + n), d.image(rec, base),
                                 base, ends, grp, L.GROUPS3, **kw)
    else:
        table, cf, nt, nchunks = d.table(case["ncol"], case["v"])
        if case["ncol"] == 6:
            ops.lion_multi(table, cf, nt, nchunks, *L.HYPER, **kw)
        else:
            ops.lion_multi_groups(table, cf, nt, nchunks, L.GROUPS3, **kw)
    torch.cuda.synchronize()                           # (tables and factors live until the kernel has read them)


@pytest.mark.parametrize("regime", list(L.REGIMES))
@pytest.mark.parametrize("form", ["flat", "flat_groups", "multi"])
def test_lion_kernels_against_the_model(form, regime):
    """every case of the form: sizes 1 .. 2 * 4096 + 3, with and without images, ranges / segments / slices / tables, special values"""
    for case in L.CASES:
        if case["form"] != form:
            continue
        c = L.build(case)
        d = Dev(c)
        for step, want in enumerate(L.run(case, regime)):
            launch(d, case, regime)
            if regime == "skip_set":
                want = (c["A"], c["I"])                # a non-zero counter: every buffer and image unchanged to the byte
            d.check(want, f"{case['name']} {regime} launch {step + 1}")


def test_lion_claims_one_group_and_device_factor():
    """the header's two claims, kernel against kernel: a one-group grouped call is the single-set call; a *_dev call is muse_grad_scale_*
    followed by the host-factor call with factor 1"""
    ops = _ops()
    one = [dict(lr=L.HYPER[0], betas=L.HYPER[1:3], weight_decay=L.HYPER[3])]
    flat = next(c for c in L.FLAT_CASES if c["name"] == "flat-n8195-bf16-one")
    n = flat["n"]
    a, b = Dev(L.build(flat)), Dev(L.build(flat))
    ra, rb = a.c["recs"][0], b.c["recs"][0]
    ops.lion_flat(a.t(ra, "p"), a.t(ra, "g"), a.t(ra, "m"), a.image(ra), *L.HYPER, grad_scale=L.THIRD)
    ops.lion_flat_groups(b.t(rb, "p"), b.t(rb, "g"), b.t(rb, "m"), b.image(rb), 0, torch.tensor([n], dtype=torch.int64, device=DEV),
                         torch.tensor([0], dtype=torch.int32, device=DEV), one, grad_scale=L.THIRD)
    torch.cuda.synchronize()
    assert torch.equal(a.A, b.A) and torch.equal(a.I, b.I)
    scale = torch.tensor([L.THIRD], dtype=torch.float32, device=DEV)
    b = Dev(L.build(flat))
    g_before = b.t(rb, "g").clone()
    ops.grad_scale_flat_(b.t(rb, "g"), scale)
    ops.lion_flat(b.t(rb, "p"), b.t(rb, "g"), b.t(rb, "m"), b.image(rb), *L.HYPER, grad_scale=1.0)
    b.t(rb, "g").copy_(g_before)
    a = Dev(L.build(flat))
    ops.lion_flat(a.t(ra, "p"), a.t(ra, "g"), a.t(ra, "m"), a.image(ra), *L.HYPER, scale_dev=scale)
    torch.cuda.synchronize()
    assert torch.equal(a.A, b.A) and torch.equal(a.I, b.I)
    multi = next(c for c in L.MULTI_CASES if c["name"] == "multi6-rot1")
    a, b = Dev(L.build(multi)), Dev(L.build(multi))
    ta, tb = a.table(6, "null"), b.table(7, "null")        # (column 6 of a 6-column case: group 0, plain bf16 copies)
    ops.lion_multi(*ta, *L.HYPER, scale_dev=scale)
    ops.grad_scale_multi_(*tb, scale)
    ops.lion_multi_groups(*tb, one, grad_scale=1.0)
    torch.cuda.synchronize()
    for r in b.c["recs"]:
        b.t(r, "g").copy_(a.t(r, "g"))
    assert torch.equal(a.A, b.A) and torch.equal(a.I, b.I)


def test_lion_entry_points_refuse_what_adamw_refuses():
    from muse._hip import MuseHipError
    ops = _ops()
    case = next(c for c in L.FLAT_CASES if c["name"] == "flat-n4097-bf16-one")
    c = L.build(case)
    d, rec = Dev(c), c["recs"][0]
    scale = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    for kw in (dict(), dict(scale_dev=scale)):
        with pytest.raises(MuseHipError, match="alignment"):
            ops.lion_flat(d.t(rec, "p"), d.t(rec, "g"), d.t(rec, "m"), d.I[rec["img"].pb + 1:], *L.HYPER, **kw)
        with pytest.raises(MuseHipError, match="alignment"):
            ops.lion_flat(d.t(rec, "p", 1), d.t(rec, "g", 1), d.t(rec, "m", 1), None, *L.HYPER, **kw)
        with pytest.raises(MuseHipError, match="alignment"):
            ops.lion_flat_groups(d.t(rec, "p"), d.t(rec, "g", 1, 4097), d.t(rec, "m"), None, 0, torch.tensor([4097], dtype=torch.int64, device=DEV),
                                 torch.tensor([0], dtype=torch.int32, device=DEV), L.GROUPS3, **kw)
        with pytest.raises(MuseHipError, match="bad argument"):
            ops.lion_flat_groups(d.t(rec, "p"), d.t(rec, "g"), d.t(rec, "m"), None, 0, torch.zeros(0, dtype=torch.int64, device=DEV),
                                 torch.zeros(0, dtype=torch.int32, device=DEV), L.GROUPS3, **kw)
    with pytest.raises(MuseHipError, match="1..8 parameter groups"):
        ops.lion_multi_groups(*d.table(7, "null"), L.GROUPS3 * 3)
    d.check((c["A"], c["I"]), "refused calls")            # nothing was launched


# ---- the reference's recorded steps through muse.FusedLion --------------------------------------------------------------------------------------
def test_golden_steps_through_fused_lion(golden_dir):
    import muse
    g = np.load(os.path.join(golden_dir, "lion_steps.npz"))
    lay = json.loads(str(g["layout"]))
    params = [torch.nn.Parameter(torch.from_numpy(g[f"p0_{t}"].copy()).to(DEV)) for t in range(len(lay["sizes"]))]
    groups = [dict(params=[params[t] for t in lay["order"] if lay["group_of"][t] == k], lr=G["lr"], betas=tuple(G["betas"]),
                   weight_decay=G["weight_decay"]) for k, G in enumerate(lay["param_groups"])]
    opt = muse.FusedLion(groups)
    for s in range(1, lay["steps"] + 1):
        for t, p in enumerate(params):
            p.grad = torch.from_numpy(g[f"g{s}_{t}"].copy()).to(DEV)
        opt.step()
        torch.cuda.synchronize()
        for t, p in enumerate(params):
            same(p.detach().cpu().numpy().view(np.uint32), g[f"p{s}_{t}"].view(np.uint32), f"parameter {t} after step {s}")
            same(opt._m[id(p)].cpu().numpy().view(np.uint32), g[f"m{s}_{t}"].view(np.uint32), f"exp_avg {t} after step {s}")
    sd = opt.state_dict()
    assert {str(i): sorted(st) for i, st in sd["state"].items()} == lay["state_keys"]
    assert [sorted(G) for G in sd["param_groups"]] == [sorted(G) for G in lay["param_groups"]]


# ---- model level: lockstep with the model on the host ------------------------------------------------------------------------------------------
def host(t):
    return t.detach().cpu().contiguous().view(-1).numpy().copy()


def bits16(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.int16).numpy().view(np.uint16)


def hyper_of(group):
    return L.lion_hyper(group["lr"], group["betas"][0], group["betas"][1], group["weight_decay"])


def image_of(p_new, kind):
    return O.half_bits(p_new) if kind == "half" else O.bf16_bits(p_new)


def flat_host_step(model, opt, p, m, g, factor):
    """one step of the whole flat buffer on the host, segment by segment -> (p', m')"""
    seg_end, seg_group = (t.tolist() for t in opt._segments(model)) if len(opt.param_groups) > 1 else ([p.size], [0])
    p1, m1, lo = p.copy(), m.copy(), 0
    for e, k in zip(seg_end, seg_group):
        p1[lo:e], m1[lo:e] = L.update1(p[lo:e], g[lo:e], m[lo:e], hyper_of(opt.param_groups[k]), factor)
        lo = e
    return p1, m1


def transformer(cd, seed=5):
    import muse
    cfg = dict(W.TRANSFORMER_TINY)
    m = muse.MaskGitTransformer(**cfg)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), seed, "transformer"))
    m.to(DEV).train().set_compute_dtype(cd)
    ids, labels = (t.to(DEV) for t in W.transformer_inputs(cfg, 4, seed + 1))
    return m, (lambda: m(input_ids=ids, labels=labels)[1])


@pytest.mark.parametrize("variant", ["plain", "in_backward", "max_grad_norm"])
def test_flat_engine_three_steps_against_the_host_model(variant):
    """a 2-layer class-conditional MaskGitTransformer in bf16, two groups from muse.grouped_parameters: parameters, exp_avg and the bf16
    compute copy after every step, against the host model stepped from the device's gradient bytes"""
    import muse
    model, loss = transformer(torch.bfloat16)
    opt = muse.FusedLion(muse.grouped_parameters(model, 0.1), lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1,
                         max_grad_norm=1e-3 if variant == "max_grad_norm" else None)
    n = model.flat_params().numel()
    for step in range(3):
        model.zero_grad(set_to_none=True)
        out = loss()
        p0 = host(model.flat_params())
        m0 = host(opt._m) if opt._m is not None else np.zeros(n, F)
        if variant == "in_backward":
            assert opt.begin_step_in_backward(model)
            try:
                out.backward()
            finally:
                opt.end_step_in_backward(model)
            assert opt._ranges_done is not None and len(opt._ranges_done[1]) > 0          # the update really ran inside backward
        else:
            out.backward()
        torch.cuda.synchronize()
        g = host(model.flat_grads())
        opt.step()
        torch.cuda.synchronize()
        factor = 1.0
        if variant == "max_grad_norm":
            factor = float(opt.last_clip_coef)
            norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
            assert factor < 0.5 and abs(float(opt.last_grad_norm) - norm) <= 1e-5 * norm and abs(factor - 1e-3 / (norm + 1e-6)) <= 1e-5 * factor
        p1, m1 = flat_host_step(model, opt, p0, m0, g, factor)
        same(host(model.flat_params()).view(np.uint32), p1.view(np.uint32), f"{variant}: parameters after step {step + 1}")
        same(host(opt._m).view(np.uint32), m1.view(np.uint32), f"{variant}: exp_avg after step {step + 1}")
        assert model._flat_c is not None and model._flat_c.dtype == torch.bfloat16
        same(bits16(model._flat_c), O.bf16_bits(p1), f"{variant}: bf16 compute copy after step {step + 1}")
    assert opt._v is None and not np.array_equal(p1, p0)


UVIT = dict(vocab_size=520, hidden_size=256, in_channels=128, block_out_channels=(128,), encoder_hidden_size=128, cond_embed_dim=128,
            micro_cond_encode_dim=32, micro_cond_embed_dim=160, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
            block_num_heads=2, num_res_blocks=1, codebook_size=512, mask_token_id=519)


def uvit(mode):
    import muse
    B, S = 2, 256
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 512, (B, S), generator=gen).to(DEV)
    labels = torch.where(torch.rand(B, S, generator=gen) < 0.5, torch.randint(0, 512, (B, S), generator=gen), torch.full((B, S), -100)).to(DEV)
    enc, cond = torch.randn(B, 77, 128, generator=gen).to(DEV), torch.randn(B, 128, generator=gen).to(DEV)
    micro = torch.tensor([[256.0, 256.0, 0.0, 0.0, 6.0]]).repeat(B, 1).to(DEV)
    torch.manual_seed(11)
    model = muse.MaskGiTUViT(**UVIT)
    model.to(DEV).train().set_compute_dtype(mode)
    return model, (lambda: model(ids, enc, cond, micro, labels=labels)[1])


def images_of(p):
    """the image(s) FusedLion's table names for p -> (kind, hi / copy tensor, lo tensor or None), the selection of _step_per_tensor"""
    shadow = getattr(p, "_muse_shadow", None)
    if shadow is not None and (shadow.numel() != p.numel() or shadow.device != p.device or not shadow.is_contiguous()):
        shadow = None
    if shadow is not None:
        return ("half" if shadow.dtype == torch.float16 else "bf16"), shadow, None
    planes = getattr(p, "_muse_planes", None)
    if planes is not None and planes[0].numel() == p.numel() and planes[0].is_contiguous() and planes[1] > 0:
        hi = planes[0]
        lo = torch.empty(0, dtype=hi.dtype, device=hi.device).set_(hi.untyped_storage(), hi.storage_offset() + int(planes[1]), (p.numel(),), (1,))
        return "x3", hi, lo
    return None, None, None


def uvit_step_and_check(model, opt, loss, what, plant_overflow=False):
    """backward, one optimizer step, and the same step on the host from the device's bytes -> the image kinds that were compared"""
    model.zero_grad(set_to_none=True)
    loss().backward()
    torch.cuda.synchronize()
    ps = [(p, k) for k, grp in enumerate(opt.param_groups) for p in grp["params"] if p.grad is not None]
    before = [(host(p), host(p.grad), host(opt._m[id(p)]) if opt._m is not None and id(p) in opt._m else np.zeros(p.numel(), F)) for p, _ in ps]
    images_before = [tuple(None if t is None else bits16(t).copy() for t in images_of(p)[1:]) for p, _ in ps]
    overflowed = False
    if model.__dict__.get("_f32_f16", False):
        stats = model.__dict__["_f16_images"]._stats
        if plant_overflow:
            stats[0] += 1
        overflowed = int(stats[0]) != 0
    assert overflowed == plant_overflow, "the gradient scale of this set-up is chosen so that nothing overflows by itself"
    opt.step()
    torch.cuda.synchronize()
    kinds = set()
    for (p, k), (p0, g, m0), (hi0, lo0) in zip(ps, before, images_before):
        p1, m1 = (p0, m0) if overflowed else L.update1(p0, g, m0, hyper_of(opt.param_groups[k]), float(opt.grad_scale))
        same(host(p).view(np.uint32), p1.view(np.uint32), f"{what}: a parameter of {p.numel()} elements")
        same(host(opt._m[id(p)]).view(np.uint32), m1.view(np.uint32), f"{what}: exp_avg of a parameter of {p.numel()} elements")
        kind, hi, lo = images_of(p)
        kinds.add(kind)
        if kind is None:
            continue
        if overflowed:
            want_hi, want_lo = hi0, lo0
        else:
            want_hi = image_of(p1, kind)
            with np.errstate(all="ignore"):
                want_lo = None if lo is None else O.bf16_bits(p1 - O.bf16_f32(want_hi))
        same(bits16(hi), want_hi, f"{what}: the {kind} image of a parameter of {p.numel()} elements")
        if lo is not None:
            same(bits16(lo), want_lo, f"{what}: the lo plane of a parameter of {p.numel()} elements")
    return kinds, overflowed


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
def test_per_tensor_engine_three_steps_against_the_host_model(mode):
    """a MaskGiTUViT with ordinary parameters, two groups, in the bf16x3 mode (operand planes refreshed through the table's plane column)
    and in the f16 mode (half images; then one more step with a planted overflow counter, which must leave everything untouched)"""
    import muse
    model, loss = uvit(mode)
    if mode == "f16":
        model.f16_grad_scale = 2.0 ** 12
    opt = muse.FusedLion(muse.grouped_parameters(model, 0.01), lr=1e-4, betas=(0.9, 0.99), weight_decay=0.01)
    seen = set()
    for step in range(3):
        kinds, _ = uvit_step_and_check(model, opt, loss, f"{mode} step {step + 1}")
        seen |= kinds
    assert ("x3" if mode == "bf16x3" else "half") in seen, seen
    assert opt._v is None and all(set(st) == {"exp_avg"} for st in opt.state_dict()["state"].values())
    if mode == "f16":
        _, overflowed = uvit_step_and_check(model, opt, loss, "f16 planted overflow", plant_overflow=True)
        assert overflowed
