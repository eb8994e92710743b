"""Attention dropout inside the fused attention kernels (muse_attention_drop_fwd_ex / _bwd_ex, csrc/attention.hip) on the GPU.

  (a) exact mask read-back: every keep bit of every (image, head, query, key) as the forward, the dQ and the dK,dV kernels drew it, against
      philox_cpu.dropout_keep on the flat [B * nh, Sq, round_up(Skv, 8)] layout (tests/attention_dropout_cpu.py: the one-hot probes);
  (b) seeded N(0, 1) parity of ctx, lse, dq, dk, dv with float64 under the CPU mask: 4 * E_REF_DROP (+ one bf16 rounding), the rule of
      tests/test_gpu_attention_edges.py; lse also inside that file's bound for attention without dropout - dropout must not move it;
  (c) p = 0 through the new entry points is attention_fwd_ex / attention_bwd_ex bit for bit; bad arguments are refused;
  (d) model level, bf16 train(): the fused route against the materialised one (MUSE_ATTN_DROPOUT_FUSED=0) with the same dropout seed, flat
      engine and text-conditioned tape engine, held to twice the gap the two routes show WITHOUT dropout.

Shapes, p and offsets: attention_dropout_cpu.SHAPES / PS / OFFSETS.  B = 2 images, 2 heads.
"""
import ctypes as C
import gc
import warnings

import pytest
import torch

import attention_cpu as A
import attention_dropout_cpu as D
import test_gpu_attention_edges as EDGES
import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
B, NH = D.B, D.NH


def _ops():
    from muse import ops
    return ops


def runner(p, offset, ld_mask=None):
    """(fwd, bwd) on the entry points under test, as attention_dropout_cpu.run_probes wants them: q rows with stride H + 8, k | v packed,
    dk | dv written into the halves of one packed gradient (the layout of test_gpu_attention_edges.run_ex)"""
    ops = _ops()

    def operands(c):
        H = NH * c["hd"]
        qp = torch.cat([c["q"], torch.full((B * c["Sq"], 8), 3.0)], 1).to(BF).to(DEV)
        kv = torch.cat([c["k"], c["v"]], 1).to(BF).to(DEV)
        ld = D.row_pitch(c["Skv"]) if ld_mask is None else ld_mask
        return qp[:, :H], kv[:, :H], kv[:, H:], (B, c["Sq"], c["Skv"], NH, c["hd"], c["alpha"], p, D.SEED, offset, ld)

    def fwd(c):
        q, k, v, args = operands(c)
        ctx, lse = ops.attention_drop_fwd_ex(q, k, v, *args)
        return dict(ctx=ctx, lse=lse)

    def bwd(c, ctx, lse):
        q, k, v, args = operands(c)
        H = NH * c["hd"]
        dkv = torch.full((B * c["Skv"], 2 * H), 7.0, dtype=BF, device=DEV)
        dq, _, _ = ops.attention_drop_bwd_ex(q, k, v, ctx, c["do"].to(BF).to(DEV), lse, *args, dk=dkv[:, :H], dv=dkv[:, H:])
        return dict(dq=dq, dk=dkv[:, :H], dv=dkv[:, H:])
    return fwd, bwd


def run_all(c, fwd, bwd):
    f = fwd(c)
    out = dict(ctx=f["ctx"], lse=f["lse"][:, :c["Sq"]], **bwd(c, f["ctx"], f["lse"]))
    return {n: t.cpu() for n, t in out.items()}


# =====================================================================================================================================
# (a) every keep bit, all three kernels
# =====================================================================================================================================
@pytest.mark.parametrize("offset", D.OFFSETS)
@pytest.mark.parametrize("p", D.PS)
@pytest.mark.parametrize("Sq,Skv,hd", D.SHAPES)
def test_mask_readback(Sq, Skv, hd, p, offset):
    c = D.random_case(Sq, Skv, hd)
    keep = D.case_keep(Sq, Skv, p, offset)
    assert 0.0 < float(keep.float().mean()) < 1.0
    D.run_probes(c, keep, *runner(p, offset), tag=f"{Sq}x{Skv} hd{hd} p={p} offset={offset:#x}")


def test_mask_follows_ld_mask():
    """ld_mask is the layout's row pitch, not a constant: a caller that passes Skv rounded up to 4 gets that layout's bits"""
    Sq, Skv, hd = 33, 77, 64
    keep = D.keep_mask(B, NH, Sq, Skv, 0.5, D.SEED, 7, ld_mask=84)
    D.run_probes(D.random_case(Sq, Skv, hd), keep, *runner(0.5, 7, ld_mask=84), tag="ld_mask 84")


# =====================================================================================================================================
# (b) parity with float64 under the CPU mask
# =====================================================================================================================================
@pytest.mark.parametrize("offset", D.OFFSETS)
@pytest.mark.parametrize("p", D.PS)
@pytest.mark.parametrize("Sq,Skv,hd", D.SHAPES)
def test_parity_with_float64(Sq, Skv, hd, p, offset):
    c = D.random_case(Sq, Skv, hd)
    ref = D.case_reference(Sq, Skv, hd, p, offset)
    out = run_all(c, *runner(p, offset))
    tag = f"dropout {Sq}x{Skv} hd{hd} p={p} offset={offset:#x}"
    A.check_random(c, out, ref, D.e_ref_for(Sq, Skv), tag=tag)
    A.check_random(c, dict(lse=out["lse"]), ref, EDGES.e_ref_for(Sq, Skv), tag=tag + " (bound of attention without dropout)")


# =====================================================================================================================================
# (c) p = 0, bad arguments
# =====================================================================================================================================
@pytest.mark.parametrize("Sq,Skv,hd", D.SHAPES)
def test_p0_is_the_existing_entry_points(Sq, Skv, hd):
    ops = _ops()
    c = D.random_case(Sq, Skv, hd)
    got = run_all(c, *runner(0.0, 3 << 40))
    H, al = NH * hd, c["alpha"]
    q, kv = c["q"].to(BF).to(DEV), torch.cat([c["k"], c["v"]], 1).to(BF).to(DEV)
    ctx, lse = ops.attention_fwd_ex(q, kv[:, :H], kv[:, H:], B, Sq, Skv, NH, hd, al)
    dq, dk, dv = ops.attention_bwd_ex(q, kv[:, :H], kv[:, H:], ctx, c["do"].to(BF).to(DEV), lse, B, Sq, Skv, NH, hd, al)
    for n, t in dict(ctx=ctx, lse=lse[:, :Sq], dq=dq, dk=dk, dv=dv).items():
        assert torch.equal(got[n], t.cpu()), n


def test_bad_arguments_are_refused():
    from muse import _hip
    ops = _ops()
    Sq, Skv, hd = 17, 17, 16
    c = D.random_case(Sq, Skv, hd)
    q, k, v, do = (c[n].to(BF).to(DEV) for n in ("q", "k", "v", "do"))
    good = (0.5, 1, 2, 24)
    ctx, lse = ops.attention_drop_fwd_ex(q, k, v, B, Sq, Skv, NH, hd, c["alpha"], *good)
    for bad in ((-0.1, 1, 2, 24), (1.0, 1, 2, 24), (float("nan"), 1, 2, 24), (0.5, 1, 2, 18), (0.5, 1, 2, 16), (0.0, 1, 2, 16), (0.0, 1, 2, 18)):
        with pytest.raises(_hip.MuseHipError):
            ops.attention_drop_fwd_ex(q, k, v, B, Sq, Skv, NH, hd, c["alpha"], *bad)
        with pytest.raises(_hip.MuseHipError):
            ops.attention_drop_bwd_ex(q, k, v, ctx, do, lse, B, Sq, Skv, NH, hd, c["alpha"], *bad)
    d = ops._attn_desc(q, k, v, ctx, B, Sq, Skv, NH, hd, c["alpha"])
    assert ops.lib().muse_attention_drop_fwd_ex(C.byref(d), lse.data_ptr(), 1.5, 1, 2, 24, ops.stream()) == ops.lib().muse_attention_drop_fwd_ex(
        C.byref(d), lse.data_ptr(), 0.5, 1, 2, 22, ops.stream()) != 0


# =====================================================================================================================================
# (d) model level
# =====================================================================================================================================
def _maxrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _saved_prob_tensors(shapes):
    gc.collect()
    with warnings.catch_warnings():           # (isinstance wakes deprecated module attributes among the collector's objects)
        warnings.simplefilter("ignore")
        return [o for o in gc.get_objects() if isinstance(o, torch.Tensor) and o.is_cuda and tuple(o.shape) in shapes]


N_LOSS = 8      # input sets behind the loss figure (below)


def _step(make, call, prob_shapes, backward=True, inp=0):
    """one seeded forward (+ backward) of a fresh model on input set `inp` -> (logits, loss, {name: grad}, number of live
    probability-shaped tensors after the forward)"""
    m = make()
    torch.manual_seed(4321 + inp)             # the dropout seed is drawn from torch's CPU generator per forward
    logits, loss = call(m, inp)
    n_prob = len(_saved_prob_tensors(prob_shapes)) if backward else 0
    grads = {}
    if backward:
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    torch.cuda.synchronize()
    return logits.detach().clone(), loss.detach().clone(), grads, n_prob


def _gaps(a, b, loss_pairs, tag):
    """the figures the two routes are compared by: logits and every gradient by their largest difference over the tensor's largest entry
    (input set 0).  The loss is ONE signed number per run - a mean of per-token errors of either sign - so the size of a single run's gap
    is one draw of a zero-mean variable: two such draws differ by more than 2 x in three of ten trials whatever the code does
    (P(|X| > 2 |Y|) = (2 / pi) atan(1 / 2) = 0.295 for two equal Gaussians).  Its figure is therefore the root mean square of the relative
    gap over N_LOSS input sets, which the same argument puts within 2 x of another such figure at about four standard deviations."""
    out = {"logits": _maxrel(a[0], b[0]),
           "loss": (sum((abs(float(x) - float(y)) / abs(float(y))) ** 2 for x, y in loss_pairs) / len(loss_pairs)) ** 0.5}
    assert a[2].keys() == b[2].keys() and a[2]
    for k in b[2]:
        out["grad " + k] = _maxrel(a[2][k], b[2][k])
    worst = max(out, key=out.get)
    print(f"[attention_dropout] {tag}: logits {out['logits']:.3e} loss (rms of {len(loss_pairs)}) {out['loss']:.3e} worst gradient "
          f"{max(v for k, v in out.items() if k.startswith('grad ')):.3e}; worst figure {out[worst]:.3e} ({worst})")
    return out


def _held_to_twice(drop, yard, tag):
    """every figure of the dropout comparison <= 2 x the yardstick's worst figure of its kind (logits | loss | gradients).  The dropped
    operand adds one bf16 rounding per probability and nothing else."""
    kind = lambda k: k.split(" ")[0]   # noqa: E731
    bound = {}
    for k, v in yard.items():
        bound[kind(k)] = max(bound.get(kind(k), 0.0), 2.0 * v)
    fails = [f"{k}: {v:.3e} > 2 x {bound[kind(k)] / 2:.3e}" for k, v in drop.items() if v > bound[kind(k)]]
    assert not fails, f"{tag}: " + "; ".join(fails)


def _model_level(monkeypatch, make, call, prob_shapes, unfuse, tag):
    """make(p_attn) -> model; call(model, i) -> (logits, loss) on input set i; unfuse(model, monkeypatch): the materialised route at
    attention_dropout = 0 (the yardstick's other side)"""
    def both(pa, other, backward, inp):
        """(fused, other route) on one input set; other(mp) -> make for the second run, under a monkeypatch context of its own"""
        monkeypatch.delenv("MUSE_ATTN_DROPOUT_FUSED", raising=False)
        f = _step(lambda: make(pa), call, prob_shapes, backward, inp)
        with monkeypatch.context() as mp:
            o = _step(other(mp), call, prob_shapes, backward, inp)
        return f, o

    def materialised(mp):
        mp.setenv("MUSE_ATTN_DROPOUT_FUSED", "0")
        return lambda: make(0.2)
    fused, mat = both(0.2, materialised, True, 0)
    assert fused[3] == 0, f"the fused route kept {fused[3]} probability-shaped tensors {sorted(prob_shapes)} for its backward"
    assert mat[3] > 0                          # (the materialised route does: the scan can see them)
    y_fused, y_mat = both(0.0, lambda mp: (lambda: unfuse(make(0.0), mp)), True, 0)
    assert y_mat[3] > 0 and y_fused[3] == 0
    assert _maxrel(fused[0], y_fused[0]) > 1e-2  # the masks really changed the result
    drop_losses, yard_losses = [(fused[1], mat[1])], [(y_fused[1], y_mat[1])]
    for i in range(1, N_LOSS):
        f, o = both(0.2, materialised, False, i)
        drop_losses.append((f[1], o[1]))
        f, o = both(0.0, lambda mp: (lambda: unfuse(make(0.0), mp)), False, i)
        yard_losses.append((f[1], o[1]))
    yard = _gaps(y_fused, y_mat, yard_losses, tag + " yardstick (no dropout, fused vs materialised)")
    drop = _gaps(fused, mat, drop_losses, tag + " attention_dropout 0.2, fused vs materialised")
    _held_to_twice(drop, yard, tag)


def test_flat_engine_fused_matches_materialised(monkeypatch):
    """MaskGitTransformer (flat engine), hidden_dropout 0, attention_dropout 0.2, bf16, train(): fused dropout against the materialised
    route with the same masks; the fused run keeps no [B * nh, S, Sp] tensor.
    Measured on an MI355X, logits | loss (rms of 8) | worst gradient: yardstick (no dropout, fused_attention True vs False; the parent
    commit gives the same figures) 2.034e-02 | 3.956e-04 | 3.769e-02; attention_dropout 0.2, fused vs materialised 1.508e-02 | 4.133e-04 |
    2.810e-02."""
    import muse
    cfg0 = W.TRANSFORMER_TINY
    inputs = [W.transformer_inputs(cfg0, 4, 77 + i) for i in range(N_LOSS)]
    nb, S = inputs[0][0].shape
    nh = cfg0["num_attention_heads"]

    def make(pa):
        cfg = dict(cfg0, hidden_dropout=0.0, attention_dropout=pa)
        m = muse.MaskGitTransformer(**cfg)
        m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), 78, "transformer"))
        m.to(DEV).train().set_compute_dtype(BF)
        return m

    def unfuse(m, mp):
        m.fused_attention = False
        return m
    call = lambda m, i: m(input_ids=inputs[i][0].to(DEV), labels=inputs[i][1].to(DEV))   # noqa: E731
    _model_level(monkeypatch, make, call, {(nb * nh, S, (S + 7) // 8 * 8)}, unfuse, "flat engine")


def test_tape_engine_fused_matches_materialised(monkeypatch):
    """the text-conditioned MaskGitTransformer (tape engine): self-attention and cross-attention against 7 text states, both with dropout.
    The tape engine has no fused_attention switch: the yardstick's materialised side is the same model with ops.attention_supported
    answering False.  Measured on an MI355X, logits | loss (rms of 8) | worst gradient: yardstick (the parent commit gives the same
    figures) 9.389e-03 | 2.691e-04 | 3.406e-02; attention_dropout 0.2, fused vs materialised 7.610e-03 | 2.969e-04 | 2.043e-02."""
    import muse
    from muse import ops
    cfg0 = W.TRANSFORMER_TEXT_TINY
    inputs = [W.transformer_text_inputs(cfg0, 3, 7, 801 + i) for i in range(N_LOSS)]
    nb, S = inputs[0][0].shape
    nh = cfg0["num_attention_heads"]

    def make(pa):
        cfg = dict(cfg0, hidden_dropout=0.0, attention_dropout=pa)
        m = muse.MaskGitTransformer(**cfg)
        m.load_state_dict(W.fill_state_dict(W.transformer_shapes(cfg), 800, "transformer"))
        m.to(DEV).train().set_compute_dtype(BF)
        return m

    def unfuse(m, mp):
        mp.setattr(ops, "attention_supported", lambda *a, **k: False)
        return m
    shapes = {(nb * nh, S, (S + 7) // 8 * 8), (nb * nh, S, 8)}
    call = lambda m, i: m(input_ids=inputs[i][0].to(DEV), encoder_hidden_states=inputs[i][2].to(DEV), labels=inputs[i][1].to(DEV))   # noqa: E731
    _model_level(monkeypatch, make, call, shapes, unfuse, "tape engine")
