"""GPU (MI355X): gradient clipping by global L2 norm - the norm / finalize / scale kernels of csrc/gradnorm.hip, the AdamW entry points
that read the gradient factor from device memory (muse_adamw_*_dev), and their use by muse.FusedAdamW(max_grad_norm=...),
muse.TrainStep(max_grad_norm=...), muse.clip_grad_norm_, muse.grad_norms and muse.training_utils.log_grad_norm.

Bounds: norms against float64 of the same bytes 2^-22 relative (squares of f32 are exact in f64; an f64 sum of n <= 2^30 terms errs by
less than n * 2^-53 ~ 1e-7 of the sum, half of that after the root; one rounding to f32 adds 2^-24; 2^-22 leaves a factor of two);
against torch's own f32 norm 2^-20; parameters against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW 2e-6, the bound
test_adamw_flat_groups_matches_torch_and_flat holds the same comparison to without clipping.  Every clipping case asserts coef < 0.5 and
every pass-through case coef == 1 on the returned coefficient."""
import json
import os

import numpy as np
import pytest
import torch

import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [5000, 768, 4096, 3, 10001, 8, 4100, 12288]
BIG = (1 << 24) + 5
CHUNK = 4096


def _ops():
    from muse import ops
    return ops


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale)


class FlatLayout:
    """parameters of `sizes` in one flat buffer, `pads[i]` elements of padding behind parameter i (offsets aligned to nothing)"""

    def __init__(self, sizes, pads, seed, pad_value):
        self.sizes, self.offs, o = sizes, [], 0
        for sz, pd in zip(sizes, pads):
            self.offs.append(o)
            o += sz + pd
        self.n = o
        host = torch.full((self.n,), pad_value, dtype=torch.float32)
        for i, (sz, off) in enumerate(zip(sizes, self.offs)):
            host[off:off + sz] = rnd((sz,), seed + i, 0.1 * (i + 1))
        self.host, self.g = host, host.to(DEV)
        first = [0]
        for sz in sizes:
            first.append(first[-1] + (sz + CHUNK - 1) // CHUNK)
        self.nt, self.nchunks = len(sizes), first[-1]
        self.ptab_host = torch.tensor([[a, b] for a, b in zip(self.offs, sizes)], dtype=torch.int64)
        self.first_host = torch.tensor(first, dtype=torch.int32)
        self.ptab, self.first = self.ptab_host.to(DEV), self.first_host.to(DEV)

    def slab(self):
        slab = torch.full((self.nchunks + self.nt + 1,), float("nan"), dtype=torch.float64, device=DEV)   # (stale partials must never count)
        slab[self.nchunks:] = 0                                 # the finalize launch's scratch: per-parameter sums and the zeroed ticket
        return slab

    def accumulate(self, slab, t0, t1):
        """parameters [t0, t1): the range from t0's offset to t1's offset (or the end of the buffer)"""
        b = self.offs[t0]
        e = self.offs[t1] if t1 < self.nt else self.n
        _ops().gradnorm_flat(self.g, b, e - b, self.ptab_host, self.first_host, self.ptab, self.first, slab)

    def finalize(self, slab, grad_scale, max_norm):
        out = torch.empty(3 + self.nt, dtype=torch.float32, device=DEV)
        _ops().gradnorm_finalize(slab, self.first, self.nt, slab[self.nchunks:], grad_scale, max_norm, out)
        return out

    def want(self):
        per = [float(self.host[o:o + s].double().pow(2).sum().sqrt()) for o, s in zip(self.offs, self.sizes)]
        total = float(torch.cat([self.host[o:o + s] for o, s in zip(self.offs, self.sizes)]).double().pow(2).sum().sqrt())
        return per, total


PADS = [0, 0, 0, 5, 0, 0, 60, 0, 3]


def _torch_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s own f32 statements on an f32 norm"""
    c = max_norm / (norm.cpu() + 1e-6)
    return torch.clamp(c, max=1.0)


def _within_one_ulp(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(np.float64(a) - np.float64(b)) <= np.spacing(np.abs(b))


def test_flat_norm_against_float64_padding_cuts_and_formula():
    lay = FlatLayout(SIZES + [BIG], PADS, 40, 3.0e30)           # padding filled with a large finite value
    zero = FlatLayout(SIZES + [BIG], PADS, 40, 0.0)
    slab = lay.slab()
    lay.accumulate(slab, 0, lay.nt)
    out = lay.finalize(slab, 1.0, 1e9)
    torch.cuda.synchronize()
    per, total = lay.want()
    got = out.cpu().double()
    print("total norm", float(got[0]), "float64", total, "rel", abs(float(got[0]) - total) / total)
    assert abs(float(got[0]) - total) <= 2.0 ** -22 * total
    for t, w in enumerate(per):
        assert abs(float(got[3 + t]) - w) <= 2.0 ** -22 * w, (t, float(got[3 + t]), w)
    assert float(out[1]) == 1.0 and float(out[2]) == 1.0       # pass-through
    # padding is part of no norm: the slab of the buffer whose padding is zero is the same bits
    slab0 = zero.slab()
    zero.accumulate(slab0, 0, zero.nt)
    assert torch.equal(slab0[:lay.nchunks], slab[:lay.nchunks])
    # the same call again; any cut into parameter-aligned ranges, in any order: the same slab, norm and coefficient bit for bit
    again = lay.slab()
    lay.accumulate(again, 0, lay.nt)
    assert torch.equal(again[:lay.nchunks], slab[:lay.nchunks])
    for order in ([(8, 9), (5, 8), (0, 5)], [(3, 4), (0, 3), (4, 9)], [(t, t + 1) for t in (4, 8, 0, 2, 7, 1, 6, 3, 5)]):
        cut = lay.slab()
        for t0, t1 in order:
            lay.accumulate(cut, t0, t1)
        assert torch.equal(cut[:lay.nchunks], slab[:lay.nchunks]), order
        assert torch.equal(lay.finalize(cut, 1.0, 1e9), out), order
    # a range that cuts a parameter, or does not begin at one, is refused
    from muse._hip import MuseHipError
    ops = _ops()
    for b, e in ((lay.offs[1] + 1, lay.offs[3]), (lay.offs[1], lay.offs[2] + 7), (lay.offs[4], lay.offs[4] + 10000)):
        with pytest.raises(MuseHipError):
            ops.gradnorm_flat(lay.g, b, e - b, lay.ptab_host, lay.first_host, lay.ptab, lay.first, slab)
    # coefficient and scale against torch's own f32 formula on the returned norm (clipping and pass-through, with a host factor)
    for grad_scale, max_norm in ((1.0, 1.0), (0.25, 0.5), (1.0, 1e9), (0.5, float("inf"))):
        o = lay.finalize(slab, grad_scale, max_norm).cpu()
        norm, coef, scale = o[0], o[1], o[2]
        assert _within_one_ulp(float(norm), np.float32(grad_scale) * np.float32(float(out[0])))
        want = _torch_coef(norm, max_norm)
        assert _within_one_ulp(float(coef), float(want)), (float(coef), float(want))
        assert _within_one_ulp(float(scale), np.float32(grad_scale) * np.float32(float(want)))
        assert (float(coef) < 0.5) if max_norm <= 1.0 else (float(coef) == 1.0)


def _multi_table(ps, gs, ms, vs, shadows, gid=None):
    rows, first = [], [0]
    for i, (p, g, m, v, s) in enumerate(zip(ps, gs, ms, vs, shadows)):
        r = (p.data_ptr() if p is not None else 0, g.data_ptr(), m.data_ptr() if m is not None else 0,
             v.data_ptr() if v is not None else 0, s.data_ptr() if s is not None else 0, g.numel())
        rows.append(r + (gid[i],) if gid is not None else r)
        first.append(first[-1] + (g.numel() + CHUNK - 1) // CHUNK)
    return torch.tensor(rows, dtype=torch.int64).to(DEV), torch.tensor(first, dtype=torch.int32).to(DEV), first[-1]


def test_multi_tensor_norm_scale_and_agreement_with_flat():
    """the multi-tensor form over a pointer table: float64 bound, two runs bit for bit, the same slab as the flat form of the same
    values (a partial is a function of the values only, aligned or not), in-place scale == torch's multiply bit for bit"""
    ops = _ops()
    lay = FlatLayout(SIZES + [BIG], PADS, 40, 3.0e30)
    none = [None] * lay.nt
    # ordinary tensors, and views at odd element offsets of one allocation (heads that are not 16-byte aligned)
    separate = [lay.host[o:o + s].clone().to(DEV) for o, s in zip(lay.offs, lay.sizes)]
    odd = [lay.g[o:o + s] for o, s in zip(lay.offs, lay.sizes)]
    assert any(t.data_ptr() % 16 for t in odd)
    flat_slab = lay.slab()
    lay.accumulate(flat_slab, 0, lay.nt)
    per, total = lay.want()
    for grads in (separate, odd):
        table, first, nchunks = _multi_table(none, grads, none, none, none)
        assert nchunks == lay.nchunks
        slabs = []
        for _ in range(2):
            slab = lay.slab()
            ops.gradnorm_multi(table, first, lay.nt, nchunks, slab)
            slabs.append(slab)
        assert torch.equal(slabs[0][:nchunks], slabs[1][:nchunks]) and torch.equal(slabs[0][:nchunks], flat_slab[:nchunks])
        out = torch.empty(3 + lay.nt, dtype=torch.float32, device=DEV)
        ops.gradnorm_finalize(slabs[0], first, lay.nt, slabs[0][nchunks:], 1.0, 0.01, out)
        got = out.cpu().double()
        assert abs(float(got[0]) - total) <= 2.0 ** -22 * total and float(got[1]) < 0.5
        for t, w in enumerate(per):
            assert abs(float(got[3 + t]) - w) <= 2.0 ** -22 * w, t
    # in-place scale by the coefficient: torch's multiply, bit for bit; the flat form too (a whole buffer, unaligned head)
    coef = out[1:2]
    want = [g * coef for g in separate]
    table, first, nchunks = _multi_table(none, separate, none, none, none)
    ops.grad_scale_multi_(table, first, lay.nt, nchunks, coef)
    for a, b in zip(separate, want):
        assert torch.equal(a, b)
    buf = lay.g[3:3 + 70001].clone()
    view = buf[1:]                                            # 4-byte aligned only
    wantv = view * coef
    ops.grad_scale_flat_(view, coef)
    assert torch.equal(view, wantv)


def _adamw_case(kind, scale_value=None, grad_scale=1.0, g_mul=None):
    """three steps of one of the four AdamW forms over SIZES; scale_value: through the *_dev entry point reading it from the device;
    else the existing entry point with the host's grad_scale.  g_mul: the gradient is multiplied by it (torch) beforehand."""
    ops = _ops()
    n = sum(SIZES)
    npad = (n + 3) // 4 * 4
    p0, g0 = rnd((npad,), 90), rnd((npad,), 91, 0.1)
    gid = [0, 1, 0, 2, 0, 1, 1, 0]
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05), dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
              dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)]
    extra = {"grad_scale": grad_scale} if scale_value is None else {"scale_dev": torch.tensor([scale_value], dtype=torch.float32, device=DEV)}
    p, g, m, v = p0.to(DEV).clone(), g0.to(DEV).clone(), torch.zeros(npad, device=DEV), torch.zeros(npad, device=DEV)
    sh = torch.zeros(npad, dtype=torch.bfloat16, device=DEV)
    if g_mul is not None:
        g = g * torch.tensor(g_mul, dtype=torch.float32, device=DEV)
    if kind in ("flat", "flat_groups"):
        ends, gids, o = [], [], 0
        for sz, k in zip(SIZES, gid):
            o += sz
            if gids and gids[-1] == k:
                ends[-1] = o
            else:
                ends.append(o); gids.append(k)
        ends[-1] = npad
        seg_end = torch.tensor(ends, dtype=torch.int64, device=DEV)
        seg_group = torch.tensor(gids, dtype=torch.int32, device=DEV)
        for step in (1, 2, 3):
            if kind == "flat":
                ops.adamw_flat(p, g, m, v, sh, 1e-3, 0.9, 0.999, 1e-8, 0.05, step, **extra)
            else:
                ops.adamw_flat_groups(p, g, m, v, sh, 0, seg_end, seg_group, groups, step, **extra)
        return p, m, v, sh
    cut = lambda t: [t[o:o + s] for o, s in zip(np.cumsum([0] + SIZES[:-1]).tolist(), SIZES)]   # noqa: E731  (odd offsets: scalar chunks too)
    table, first, nchunks = _multi_table(cut(p), cut(g), cut(m), cut(v), cut(sh), gid if kind == "multi_groups" else None)
    for step in (1, 2, 3):
        if kind == "multi":
            ops.adamw_multi(table, first, len(SIZES), nchunks, 1e-3, 0.9, 0.999, 1e-8, 0.05, step, **extra)
        else:
            ops.adamw_multi_groups(table, first, len(SIZES), nchunks, groups, step, **extra)
    return p, m, v, sh


@pytest.mark.parametrize("kind", ["flat", "flat_groups", "multi", "multi_groups"])
def test_adamw_with_device_side_factor(kind):
    """pointing at 1.0 / 0.5 the *_dev entry point equals the existing one with grad_scale 1.0 / 0.5 bit for bit (p, m, v, bf16 shadow;
    powers of two: for other factors the existing kernels contract the product into an fma); pointing at 0.3 it equals the existing
    entry point with grad_scale 1.0 on a gradient torch has multiplied by 0.3 - scale inside the kernel == scale the buffer, then step"""
    for s in (1.0, 0.5):
        for a, b in zip(_adamw_case(kind, scale_value=s), _adamw_case(kind, grad_scale=s)):
            assert torch.equal(bits(a), bits(b)), (kind, s)
    got, want = _adamw_case(kind, scale_value=0.3), _adamw_case(kind, grad_scale=1.0, g_mul=0.3)
    for a, b in zip(got, want):
        assert torch.equal(bits(a), bits(b)), kind
    assert not torch.equal(got[0], _adamw_case(kind, grad_scale=1.0)[0])


# ---- optimizer / model level ----------------------------------------------------------------------------------------------------------
def _transformer(cd, seed=5):
    import muse
    cfg = dict(W.TRANSFORMER_TINY)
    m = muse.MaskGitTransformer(**cfg)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), seed, "transformer"))
    m.to(DEV).train().set_compute_dtype(cd)
    ids, labels = W.transformer_inputs(cfg, 4, seed + 1)
    ids, labels = ids.to(DEV), labels.to(DEV)
    return m, (lambda: m(input_ids=ids, labels=labels)[1])


def _uvit(cd, golden_dir):
    import muse
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json")))
    g = np.load(os.path.join(golden_dir, "uvit_tiny.npz"))
    m = muse.MaskGiTUViT(**cfg)
    m.load_state_dict({k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}, strict=True)
    m.to(DEV).train().set_compute_dtype(cd)
    args = [torch.from_numpy(g[k]).to(DEV) for k in ("input_ids", "encoder_hidden_states", "cond_embeds", "micro_conds")]
    labels = torch.from_numpy(g["labels"]).to(DEV)
    return m, (lambda: m(*args, labels=labels)[1])


def _build(kind, cd, golden_dir):
    return _transformer(cd) if kind == "transformer" else _uvit(cd, golden_dir)


def _state(model, opt):
    """parameters, moments and the bf16 compute copies, as lists of tensors to compare bit for bit"""
    ps = list(model.parameters())
    if opt._model is not None:
        out = [model.flat_params(), opt._m, opt._v]
        if getattr(model, "_flat_c", None) is not None:
            out.append(model._flat_c)
        return out
    out = [p.data for p in ps] + [opt._m[id(p)] for p in ps if id(p) in opt._m] + [opt._v[id(p)] for p in ps if id(p) in opt._v]
    return out + [p._muse_shadow for p in ps if getattr(p, "_muse_shadow", None) is not None]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def _copy_grads(src, dst):
    """lockstep runs: the second model steps on the first one's gradient BYTES (what is compared is the optimizer, not backward)"""
    for a, b in zip(src.parameters(), dst.parameters()):
        assert (a.grad is None) == (b.grad is None)
        if a.grad is not None:
            b.grad.copy_(a.grad)


HYPER = dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.05, eps=1e-8)
CLIP = 1e-3


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["transformer", "uvit"])
def test_pass_through_is_bit_identical_to_no_clipping(kind, cd, golden_dir):
    import muse
    (ma, la), (mb, lb) = _build(kind, cd, golden_dir), _build(kind, cd, golden_dir)
    oa = muse.FusedAdamW(ma.parameters(), max_grad_norm=1e9, **HYPER)
    ob = muse.FusedAdamW(mb.parameters(), **HYPER)
    for step in range(3):
        la().backward()
        lb().backward()
        _copy_grads(ma, mb)
        oa.step()
        ob.step()
        assert float(oa.last_clip_coef) == 1.0 and float(oa.last_grad_norm) > 0
        oa.zero_grad(set_to_none=True)
        ob.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert ob.last_grad_norm is None and _same(_state(ma, oa), _state(mb, ob))


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["transformer", "uvit"])
def test_clipped_step_equals_clip_then_step_and_torch(kind, cd, golden_dir):
    """FusedAdamW(max_grad_norm=x).step() == muse.clip_grad_norm_(model, x) + plain step, bit for bit, three steps; p.grad after
    muse.clip_grad_norm_ == grad * coef by torch, bit for bit.  f32 mode: against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on
    CPU twins with the same gradients (2e-6; norm 2^-20)."""
    import muse
    (ma, la), (mb, lb) = _build(kind, cd, golden_dir), _build(kind, cd, golden_dir)
    oa = muse.FusedAdamW(ma.parameters(), max_grad_norm=CLIP, **HYPER)
    ob = muse.FusedAdamW(mb.parameters(), **HYPER)
    names = [n for n, _ in ma.named_parameters()]
    twins = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ma.parameters()]
    ref = torch.optim.AdamW(twins, **HYPER)
    for step in range(3):
        la().backward()
        lb().backward()
        _copy_grads(ma, mb)
        raw = [None if p.grad is None else p.grad.clone() for p in mb.parameters()]
        for t, p in zip(twins, ma.parameters()):
            t.grad = None if p.grad is None else p.grad.detach().cpu().clone()
        oa.step()
        norm, coef = muse.clip_grad_norm_(mb if step != 1 else list(mb.parameters()), CLIP, return_coef=True)
        for p, r in zip(mb.parameters(), raw):
            assert r is None or torch.equal(p.grad, r * coef)
        ob.step()
        assert float(oa.last_clip_coef) < 0.5 and float(coef) < 0.5
        assert torch.equal(oa.last_grad_norm, norm) and torch.equal(oa.last_clip_coef, coef)
        for p, r in zip(ma.parameters(), raw):
            assert r is None or torch.equal(p.grad, r)        # the clipped step leaves p.grad unscaled
        tn = torch.nn.utils.clip_grad_norm_(twins, CLIP)
        ref.step()
        assert abs(float(norm) - float(tn)) <= 2.0 ** -20 * float(tn), (float(norm), float(tn))
        oa.zero_grad(set_to_none=True)
        ob.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert _same(_state(ma, oa), _state(mb, ob))
    if cd == torch.float32:
        for n, p, t in zip(names, ma.parameters(), twins):
            assert float((p.detach().cpu() - t.detach()).abs().max()) < 2e-6, n
    # checkpoints keep torch.optim.AdamW's layout
    sd, sd0 = oa.state_dict(), ob.state_dict()
    assert sd.keys() == sd0.keys() and [g.keys() for g in sd["param_groups"]] == [g.keys() for g in sd0["param_groups"]]
    assert all(sd["state"][i].keys() == sd0["state"][i].keys() for i in sd["state"]) and sd["state"].keys() == sd0["state"].keys()
    ref2 = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in ma.parameters()], **HYPER)
    ref2.load_state_dict(sd)
    assert int(ref2.state_dict()["state"][0]["step"]) == 3


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16])
def test_train_step_accumulates_the_norm_inside_backward(cd):
    """muse.TrainStep(max_grad_norm=x): the sums of squares run range by range from inside backward, step() finalizes and updates;
    bit-identical to the plain loop with FusedAdamW(max_grad_norm=x), three steps (losses, parameters, moments, bf16 copy)"""
    import muse
    ops = _ops()
    cfg = dict(W.TRANSFORMER_TINY)
    sd = W.fill_state_dict(W.transformer_shapes(cfg), 701, "transformer")
    B, S = 4, cfg["num_vq_tokens"]
    rng = np.random.default_rng(11)
    tokens = torch.from_numpy(rng.integers(0, cfg["codebook_size"], size=(B, S))).to(DEV)
    cls = torch.from_numpy(rng.integers(0, cfg["num_classes"], size=B)).to(DEV)

    def model():
        m = muse.MaskGitTransformer(**cfg)
        m.load_state_dict(sd)
        m.to(DEV).train().set_compute_dtype(cd)
        return m
    ma, mb = model(), model()
    oa = muse.FusedAdamW(ma.parameters(), **HYPER)
    ob = muse.FusedAdamW(mb.parameters(), max_grad_norm=CLIP, **HYPER)
    ts = muse.TrainStep(None, ma, oa, max_grad_norm=CLIP)
    assert oa.max_grad_norm == CLIP
    calls, inner = [], ops.gradnorm_flat
    ops.gradnorm_flat = lambda g, base, n, *a: (calls.append((base, base + n)), inner(g, base, n, *a))[1]
    try:
        for step in range(3):
            t, nz = W.uniforms((B,), 20 + step).to(DEV), W.uniforms((B, S), 30 + step).to(DEV)
            calls.clear()
            loss_a, _ = ts(None, cls, t, nz, image_tokens=tokens)
            n = ma.flat_params().numel()
            assert len(calls) > 1 and sum(e - b for b, e in calls) == n, calls     # several ranges that tile the buffer once
            assert sorted(calls)[0][0] == 0 and all(a[1] == b[0] for a, b in zip(sorted(calls), sorted(calls)[1:]))
            ids, labels, _, _ = muse.prepare_inputs_and_labels(None, None, cls, mb.config.mask_token_id, 0.0, t, nz, image_tokens=tokens, codebook_size=mb.config.codebook_size)
            calls.clear()
            _, loss_b = mb(input_ids=ids, labels=labels, label_smoothing=0.0)
            loss_b.backward()
            ob.step()
            assert calls == [(0, n)]
            ob.zero_grad(set_to_none=True)
            assert float(oa.last_clip_coef) < 0.5
            assert torch.equal(loss_a, loss_b.detach()) and torch.equal(oa.last_grad_norm, ob.last_grad_norm)
            assert torch.equal(oa.last_clip_coef, ob.last_clip_coef)
    finally:
        ops.gradnorm_flat = inner
    torch.cuda.synchronize()
    assert _same(_state(ma, oa), _state(mb, ob))


@pytest.mark.parametrize("kind", ["transformer", "uvit"])
def test_log_grad_norm_one_copy(kind, golden_dir, monkeypatch):
    """muse.training_utils.log_grad_norm against the reference's formula (train_muse.py:1313) in float64, with exactly ONE device-to-
    host copy; muse.grad_norms returns the same norms on the device"""
    import muse
    from muse import training_utils as TU
    m, loss = _build(kind, torch.float32, golden_dir)
    loss().backward()
    torch.cuda.synchronize()
    want = {"grad_norm/" + n: float(p.grad.detach().double().norm().cpu()) / p.grad.numel() for n, p in m.named_parameters() if p.grad is not None}
    count = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                count["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    got = TU.log_grad_norm(m)
    assert count["n"] == 1, count
    norms = muse.grad_norms(m)
    assert count["n"] == 1 and norms.is_cuda and norms.dtype == torch.float32 and norms.numel() == len(want)
    monkeypatch.undo()
    assert got.keys() == want.keys() and len(got) > 10
    for k, w in want.items():
        assert abs(got[k] - w) <= 2.0 ** -22 * w, (k, got[k], w)
    per = sorted(float(x) for x in norms.cpu())
    full = sorted(w * p.numel() for (n, p), w in ((np_, want["grad_norm/" + np_[0]]) for np_ in m.named_parameters() if np_[1].grad is not None))
    assert len(per) == len(full) and all(abs(a - b) <= 2.0 ** -22 * b for a, b in zip(per, full))


def test_f16_mode_skipped_step_and_first_applied_step():
    """the "f16" compute mode (set-up of test_flat_engine_f16_overflow_guard) with max_grad_norm: a step whose backward overflowed
    leaves parameters and moments bit-identical (the norm is simply non-finite); the first applied step clips, bit-identical to
    muse.clip_grad_norm_ + a plain step from the same state"""
    import muse
    cfg = dict(W.TRANSFORMER_B, num_hidden_layers=2)
    m = muse.MaskGitTransformer(**cfg)
    m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), 5, "transformer"))
    m.to(DEV).train().set_compute_dtype("f16")
    m.f16_grad_scale = 2.0 ** 30
    ids, labels = (t.to(DEV) for t in W.transformer_inputs(cfg, 2, 6))
    opt = muse.FusedAdamW(m.parameters(), max_grad_norm=CLIP, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.05, eps=1e-8)
    skipped, applied = 0, False
    for it in range(12):
        m.zero_grad(set_to_none=True)
        _, loss = m(input_ids=ids, labels=labels)
        loss.backward()
        torch.cuda.synchronize()
        ov = int(m.__dict__["_f16_images"]._stats[0])
        p0, g = m.flat_params().clone(), m.flat_grads().clone()
        m0 = opt._m.clone() if opt._m is not None else torch.zeros_like(p0)
        v0 = opt._v.clone() if opt._v is not None else torch.zeros_like(p0)
        opt.step()
        torch.cuda.synchronize()
        if ov:
            skipped += 1
            assert torch.equal(m.flat_params(), p0) and torch.equal(opt._m, m0) and torch.equal(opt._v, v0), it
            assert not bool(torch.isfinite(opt.last_grad_norm))
            continue
        assert bool(torch.isfinite(g).all()) and float(opt.last_clip_coef) < 0.5
        p1, m1, v1, coef = m.flat_params().clone(), opt._m.clone(), opt._v.clone(), opt.last_clip_coef.clone()
        assert not torch.equal(p1, p0)
        m.flat_params().copy_(p0); opt._m.copy_(m0); opt._v.copy_(v0)
        opt._step -= 1
        opt.max_grad_norm = None
        _, c2 = muse.clip_grad_norm_(m, CLIP, return_coef=True)
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(c2, coef) and torch.equal(m.flat_params(), p1) and torch.equal(opt._m, m1) and torch.equal(opt._v, v1)
        applied = True
        break
    assert applied and skipped >= 1
