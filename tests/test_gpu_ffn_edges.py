"""GPU (-m gpu): the fused NormFormer row kernels of csrc/rowops.hip - ln_pair_fwd / ln_pair_bwd (the two back-to-back LayerNorms of a
layer in one pass per direction) and ffn_mid_fwd / ffn_mid_bwd with their two-waves-per-row bf16 routes (GLU + mid LayerNorm) - per
element / per row at every dispatch edge, against float64 torch on the same rounded inputs.  The helpers, the way a bound is made
(4 x E_ref of torch's own float32 CPU composite, + one bf16 ulp for a bf16 output) and the reasons are those of
tests/test_gpu_row_edges.py; profiles/row_edges.md has the table.  `python tests/test_gpu_ffn_edges.py` prints E_REF (no GPU).

What is particular to these kernels:
  * inputs.  Row 0 has b = 0, so h = gelu(a) b is exactly 0: hm and the row's term of dw must be exactly 0.  Rows 1 and 2 have
    a = 1e3 + N(0, 1) (gelu(a) = a) and b = +-1, so h = +-1e3 + N(0, 1): a one-pass variance loses them.  The others are 2 N(0, 1).
    ln_pair gets the same three kinds in `ao` (test_gpu_row_edges.norm_input);
  * f32 ffn_mid is judged against the float64 composite LayerNorm(gelu(a) b) and its autograd.  h is judged per element against |a| |b|,
    dab per element against the magnitudes that do not cancel: |dh| |b| (1 + |a|) resp. |dh| |a| for the GLU's own arithmetic plus the
    row's largest |dh| times |b gelu'(a)| resp. |gelu(a)| for the LayerNorm backward, which is a row operation;
  * bf16 ffn_mid is judged in stages, each with an exact input: the stored h against float64 within the bf16 GELU bound of
    test_gpu_row_edges (times |b|); hm, mean and rstd against the float64 LayerNorm of the kernel's OWN stored h (the source promises
    that LayerNorm sees the rounded h); dab and dw against the float64 backward built from that same h.  A dab element may err by
    4 E_ref[ffn_mid_dh] (row's largest |dh|) |b gelu'(a)| + |dh| |b| E (1 + |a|) + one bf16 ulp (the b half: |gelu(a)|, 0.5 E |a|);
  * keep_h=False must give the bits of keep_h=True: hm, mean, rstd from the forward, dab and dw from the RECOMP backward.  The
    two-waves-per-row backward kernel (MUSE_FFN_MID_WIDE bit 1) sums a row in another order than the generic one (measured: dw equal in
    bits, dab at 12 of 16 cases), so where it is on, it is judged against float64 like any other and the RECOMP backward, always
    the generic kernel, is compared with the generic kernel with h given, reached through an h that is not 16-byte aligned.
    (This comparison found one dab element in 9 x 1024 a bf16 ulp apart: see ffn_glu_bwd_bf16 in csrc/rowops.hip.)
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import test_gpu_row_edges as R
from test_gpu_row_edges import (BF, DEV, F32, GELU_E, TINY, bf16_ulp, check, colsum_scale, elem_scale, gelu_ref, measure, norm_input,
                                randn, rounded, row_scale)

pytestmark = pytest.mark.gpu
F64 = torch.float64
FFN_EPS, LNP_EPS = 1e-6, 1e-5
FFN_BLOCK, LNP_FWD_BLOCK, LNP_BWD_BLOCK = 8, 4, 16      # rows per block (muse_ffn_mid_rows_per_block, ln_pair_fwd, LN_BWD_ROWS)
SENT = 7.0                                             # what an output row that must stay untouched is filled with
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -3

# Worst normalised error of torch's float32 CPU composite against float64 over the case lists below, as printed by
# `python tests/test_gpu_ffn_edges.py`.  bound = 4 * E_ref (+ one bf16 ulp for a bf16 output).
E_REF = {                            # bound = 4 * E_ref; what sets E_ref (f32 / bf16: the storage type of the case)
    "ffn_mid_h": 3.495e-07,          # 1.4e-06  per element over |a| |b| (17 x 4092 f32)
    "ffn_mid_hm": 5.607e-05,         # 2.2e-04  the h = 1e3 + N(0, 1) row of the 8 x 4 f32 input: an f32 mean near 1e3 against std 1
    "ffn_mid_mean": 1.204e-06,       # 4.8e-06  |mean error| over the row's largest |h|: a 4-column f32 row whose h = gelu(a) b is far below |a| |b|
    "ffn_mid_rstd": 2.243e-06,       # 9.0e-06  relative: the same row of the 17 x 4 layout probe (|mean| = 11 std)
    "ffn_mid_dh": 1.094e-03,         # 4.4e-03  the LayerNorm backward alone, per row: the -1e3 row in bf16 (996 / 1000 / 1004), 4 columns
    "ffn_mid_dab": 7.210e-04,        # 2.9e-03  the 1e3 row in bf16, 4 columns, over the sum normaliser of the header
    "ffn_mid_dw": 4.593e-04,         # 1.8e-03  the same rows; over the largest column sum of |dhm|
    "ln_pair_x1": 1.765e-05,         # 7.1e-05  the 1e3 + N(0, 1) row of ao (18 x 260)
    "ln_pair_ln2": 6.025e-06,        # 2.4e-05  the same row: x1's f32 rounding carried through the second LayerNorm
    "ln_pair_mean_post": 2.245e-08,  # 9.0e-08  bf16 ao: the 1e3 rows sum exactly in f32, an ordinary row sets it
    "ln_pair_rstd_post": 9.699e-08,  # 3.9e-07  relative
    "ln_pair_mean_pre": 1.251e-05,   # 5.0e-05  over the row's largest |x1|: x1 itself is 1.8e-5 off in f32 on the 1e3 row
    "ln_pair_rstd_pre": 3.109e-06,   # 1.2e-05  the same row
    "ln_pair_dx1": 2.895e-06,        # 1.2e-05  the same row
    "ln_pair_dao": 3.670e-05,        # 1.5e-04  the 1e3 row of the 33 x 4 input
    "ln_pair_dw_pre": 2.613e-06,     # 1.0e-05  over the largest column sum of |dln2|
    "ln_pair_dw_post": 3.532e-04,    # 1.4e-03  the 1e3 row of 18 x 4; over the largest column sum of |dx1|
}
R.E_REF.update(E_REF)                # `check` looks its constant up there


def _ops():
    from muse import ops
    return ops


def _hip():
    from muse import _hip as H
    return H


def check_bound(name, got, ref, bound, e_txt):
    """`check` for a bound that is not 4 E_ref x one normaliser: |got - ref| <= bound, element by element"""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite output"
    d = (got.double() - ref).abs()
    ratio = torch.where(d > 0, d / bound.clamp(min=1e-300), torch.zeros_like(d))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[row_edges] {name} {str(got.dtype)[6:]} shape={tuple(got.shape)} {e_txt} err/bound={worst:.3f}")
    assert worst <= 1.0, f"{name}: error {worst:.3f} x its bound ({e_txt})"


def same_bits(x, y):
    if x is None or y is None:
        return x is None and y is None
    x, y = x.detach().cpu().contiguous(), y.detach().cpu().contiguous()
    v = torch.int16 if x.dtype == BF else torch.int32
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(v), y.view(v))


def rowmax(t):
    return t.abs().amax(-1).clamp(min=TINY)


# =====================================================================================================================================
# ffn_mid: cases, the float64 / float32 composite, the checkers
# =====================================================================================================================================
FFN_GENERIC_INTER = {F32: [4, 1020, 1024, 1028, 2044, 2052, 3076, 4092, 4096], BF: [4, 1020, 1028, 2044, 2052, 3076, 4092]}
FFN_GENERIC_ROWS = [1, 8, 9, 17]                       # a block is 8 rows
FFN_WIDE_INTER = [1024, 2048, 3072, 4096]
FFN_WIDE_ROWS = [1, 9, 16, 25]                         # a block is 2 pairs x 8 rows: pair 1 dead / one live row / full / second block ragged
FFN_GENERIC_CASES = [(rows, inter, t) for t in (F32, BF) for inter in FFN_GENERIC_INTER[t] for rows in FFN_GENERIC_ROWS]
FFN_WIDE_CASES = [(rows, inter, BF) for inter in FFN_WIDE_INTER for rows in FFN_WIDE_ROWS]


def ffn_case(rows, inter, t, seed):
    n = max(rows, 4)
    a, b = randn((n, inter), seed, 2.0), randn((n, inter), seed + 1, 2.0)
    b[0] = 0.0
    a[1] = 1e3 + randn((inter,), seed + 2)
    b[1] = 1.0
    a[2] = 1e3 + randn((inter,), seed + 3)
    b[2] = -1.0
    pick = slice((0, 1, 3)[seed % 3], (0, 1, 3)[seed % 3] + 1) if rows == 1 else slice(0, rows)      # one row: zero, 1e3 or ordinary
    return dict(a=rounded(a[pick].clone(), t), b=rounded(b[pick].clone(), t), w=1.0 + 0.1 * randn((inter,), 41),
                dhm=rounded(randn((n, inter), seed + 4)[pick].clone(), t), t=t, rows=rows, inter=inter)


def ffn_seed(cases, case):
    return 2000 + 7 * cases.index(case) + (1000 if cases is FFN_WIDE_CASES else 0)


def ffn_ref(c, dt, h_stored=None):
    """LayerNorm(gelu(a) b) w and its gradients in `dt` arithmetic: float64 is the reference (erfc-based GELU), float32 torch's own
    kernels (E_ref).  h_stored: the LayerNorm and everything after it start from this h instead (bf16: the kernel's stored h)"""
    a, b = c["a"].to(dt), c["b"].to(dt)
    g, gp = gelu_ref(c["a"].clone(), dt)
    g, gp = g.detach(), gp.detach()
    h = g * b
    hin = (h if h_stored is None else h_stored.detach().cpu().to(dt)).clone().requires_grad_(True)
    w = c["w"].to(dt).clone().requires_grad_(True)
    hm = F.layer_norm(hin, (c["inter"],), w, None, FFN_EPS)
    hm.backward(c["dhm"].to(dt))
    dh = hin.grad
    x = hin.detach()
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + FFN_EPS)
    return dict(h=h, hin=x, hm=hm.detach(), mean=mean, rstd=rstd, xhat=(x - mean[:, None]) * rstd[:, None], dh=dh,
                dab=torch.cat([dh * b * gp, dh * g], 1), dw=w.grad, g=g, gp=gp)


def ffn_scales(c, r):
    """normalisers from the float64 reference `r` (see the header)"""
    a, b = c["a"].double().abs(), c["b"].double().abs()
    dh, rm = r["dh"].abs(), rowmax(r["dh"])[:, None]
    ln_a, ln_b = rm * (b * r["gp"].abs()), rm * r["g"].abs()                  # what an error of dh, a row quantity, does to dab
    return dict(h=a * b + TINY, mean=rowmax(r["hin"]), ln=torch.cat([ln_a, ln_b], 1),
                glu=torch.cat([dh * b * (1.0 + a), dh * a], 1), a=a, b=b, dh=dh)


def ffn_check(c, out):
    """out: h (or None), hm, mean, rstd, dab, dw of one forward + backward, from the kernels or from an emulation of them"""
    bf = c["t"] == BF
    if bf and out["h"] is None:
        raise AssertionError("the bf16 stages start from the stored h: pass the h of the keep_h=True run")
    r = ffn_ref(c, F64, out["h"] if bf else None)
    s = ffn_scales(c, r)
    if bf:
        exact = ffn_ref(c, F64)
        check_bound("ffn_mid_h", out["h"], exact["h"], bf16_ulp(exact["h"]) + 0.5 * GELU_E * s["h"], f"E={GELU_E:.1e}")
    elif out["h"] is not None:
        check("ffn_mid_h", out["h"], r["h"], s["h"])
    check("ffn_mid_hm", out["hm"], r["hm"], row_scale(r["hm"]))
    check("ffn_mid_mean", out["mean"], r["mean"], s["mean"])
    check("ffn_mid_rstd", out["rstd"], r["rstd"], elem_scale(r["rstd"]))
    if bf:
        glu = torch.cat([s["dh"] * s["b"] * GELU_E * (1.0 + s["a"]), s["dh"] * 0.5 * GELU_E * s["a"]], 1)
        bound = 4.0 * R.E_REF["ffn_mid_dh"] * s["ln"] + glu + bf16_ulp(r["dab"])
        check_bound("ffn_mid_dab", out["dab"], r["dab"], bound, f"E_ref={R.E_REF['ffn_mid_dh']:.3e} E={GELU_E:.1e}")
    else:
        check("ffn_mid_dab", out["dab"], r["dab"], s["ln"] + s["glu"] + TINY)
    check("ffn_mid_dw", out["dw"], r["dw"], colsum_scale(c["dhm"], r["dw"]))
    zero = (c["b"].float() == 0).all(-1)                                       # the h = 0 rows: exactly 0, not merely small
    if bool(zero.any()):
        assert bool((out["hm"].detach().cpu().float()[zero] == 0).all()), "hm of an h = 0 row is not exactly 0"
        assert bool((out["mean"].detach().cpu()[zero] == 0).all()), "mean of an h = 0 row is not exactly 0"
        if out["h"] is not None:
            assert bool((out["h"].detach().cpu().float()[zero] == 0).all())
        if bool(zero.all()):
            assert bool((out["dw"].detach().cpu() == 0).all()), "an h = 0 row adds something to dw"


def ffn_emulate(c, mutant=None):
    """the kernels' arithmetic in float32 torch.  mutant 'divisor': mean and variance over inter rounded up to a multiple of 1024;
    'unrounded': (bf16) LayerNorm reads h before it is rounded to the storage type"""
    t, inter = c["t"], c["inter"]
    a, b, w, dhm = c["a"].float(), c["b"].float(), c["w"], c["dhm"].float()
    g, gp = gelu_ref(c["a"].clone(), F32)
    g, gp = g.detach(), gp.detach()
    h32 = g * b
    h = h32.to(t)
    x = h32 if mutant == "unrounded" else h.float()
    n = float(-(-inter // 1024) * 1024 if mutant == "divisor" else inter)
    mean = x.sum(-1) / n
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).sum(-1) / n + FFN_EPS)
    xhat = (x - mean[:, None]) * rstd[:, None]
    gk = dhm * w
    c1, c2 = gk.sum(-1, keepdim=True) / n, (gk * xhat).sum(-1, keepdim=True) / n
    dh = rstd[:, None] * (gk - c1 - xhat * c2)
    return dict(h=h, hm=(xhat * w).to(t), mean=mean, rstd=rstd, dab=torch.cat([dh * b * gp, dh * g], 1).to(t), dw=(dhm * xhat).sum(0),
                xhat=xhat)


def ffn_run(c, keep_h=True, h=None):
    """forward (+ backward with the forward's h, with `h`, or recomputing it) through muse.ops"""
    ops = _ops()
    ab = torch.cat([c["a"], c["b"]], 1).contiguous().to(DEV)
    w, dhm = c["w"].to(DEV), c["dhm"].to(DEV)
    hk, hm, mean, rstd = ops.ffn_mid_fwd(ab, w, FFN_EPS, keep_h=keep_h)
    assert (hk is None) == (not keep_h)
    dw = torch.full((c["inter"],), SENT, device=DEV)
    dab = ops.ffn_mid_bwd(dhm, hk if h is None else h, ab, w, mean, rstd, dw, False)
    return dict(h=hk, hm=hm, mean=mean, rstd=rstd, dab=dab, dw=dw)


FFN_OUT = ("h", "hm", "mean", "rstd", "dab", "dw")


def shifted(t):
    """the tensor at an address that is 8 but not 16 bytes aligned (bf16 only: the generic kernels read those 8 bytes at a time)"""
    assert t.dtype == BF
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[4:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def wide_bits():
    return int(os.environ.get("MUSE_FFN_MID_WIDE", "1"))


def ffn_case_check(rows, inter, t, seed):
    c = ffn_case(rows, inter, t, seed)
    out = ffn_run(c)
    ffn_check(c, out)
    again = ffn_run(c)
    for k in FFN_OUT:
        assert same_bits(out[k], again[k]), f"{k}: a second run gives other bits"
    rec = ffn_run(c, keep_h=False)                                             # h not written; the backward recomputes it
    if t == F32:                                                              # (f32: without the store the compiler contracts differently)
        ffn_check(c, rec)
        return
    ffn_check(c, dict(rec, h=out["h"]))
    gen = out
    if inter % 1024 == 0 and wide_bits() & 2:                                  # `out` came from the two-wave backward: the generic kernel
        gen = dict(out, **{k: v for k, v in ffn_run(c, h=shifted(out["h"])).items() if k in ("dab", "dw")})      # with h given, for the bits
        ffn_check(c, gen)
        print(f"[row_edges] two-wave backward {rows}x{inter}: dab bit-equal to the generic kernel {same_bits(out['dab'], gen['dab'])}, "
              f"dw {same_bits(out['dw'], gen['dw'])}")
    for k in ("hm", "mean", "rstd", "dab", "dw"):
        assert same_bits(rec[k], gen[k]), f"{k}: keep_h=False / RECOMP differs from keep_h=True"


@pytest.mark.parametrize("inter,t", [(inter, t) for t in (F32, BF) for inter in FFN_GENERIC_INTER[t]], ids=lambda v: str(v).replace("torch.", ""))
def test_ffn_mid_generic_every_width(inter, t):
    """ffn_mid_fwd_kernel<T, 1..4> and ffn_mid_bwd_kernel<T, 1..4, RECOMP>, both types, with h and recomputing it: on either side of
    every NV threshold (f32 also on it: bf16 goes the wide way there), 1 row, a full block, a block + 1 row and two blocks + 1"""
    for case in FFN_GENERIC_CASES:
        if case[1:] == (inter, t):
            ffn_case_check(case[0], inter, t, ffn_seed(FFN_GENERIC_CASES, case))


@pytest.mark.parametrize("inter", FFN_WIDE_INTER)
def test_ffn_mid_wide_every_width(inter):
    """bf16 at the multiples of 1024: ffn_mid_fwd2_kernel<1..4> with and without h by default, the generic forward with
    MUSE_FFN_MID_WIDE=0, ffn_mid_bwd2_kernel<1..4> with MUSE_FFN_MID_WIDE=3 (test_switch_in_a_child_interpreter); the backward with h
    and recomputing it.  Rows: pair 1 dead, pair 1 with one live row, a full block, a ragged second block"""
    for case in FFN_WIDE_CASES:
        if case[1] == inter:
            ffn_case_check(case[0], inter, BF, ffn_seed(FFN_WIDE_CASES, case))


# ---- the C entries with caller-owned buffers: alignment fallback, layout of the partial sums, stray writes ----------------------------
def ffn_buffers(c, extra=1, part_extra=2):
    """every output with `extra` trailing rows of SENT, the partial sums NaN with `part_extra` rows more than there are blocks"""
    rows, inter, t = c["rows"], c["inter"], c["t"]
    nblk = -(-rows // FFN_BLOCK)
    full = lambda shape, v, dtype: torch.full(shape, v, dtype=dtype)
    return dict(h=full((rows + extra, inter), SENT, t), hm=full((rows + extra, inter), SENT, t), mean=full((rows + extra,), SENT, F32),
                rstd=full((rows + extra,), SENT, F32), dab=full((rows + extra, 2 * inter), SENT, t),
                part=full((nblk + part_extra, inter), float("nan"), F32))


def ffn_run_c(c, bufs, shift=None, recomp=False, want=0):
    """muse_ffn_mid_fwd + muse_ffn_mid_bwd on `bufs` (moved to the GPU, `shift`: that one bf16 tensor at an address % 16 == 8)"""
    H, ops = _hip(), _ops()
    lib = H.lib()
    d = {k: v.to(DEV) for k, v in bufs.items()}
    d.update(ab=torch.cat([c["a"], c["b"]], 1).contiguous().to(DEV), dhm=c["dhm"].to(DEV))
    w = c["w"].to(DEV)
    if shift:
        d[shift] = shifted(d[shift])
    assert w.data_ptr() % 16 == 0 and d["part"].data_ptr() % 16 == 0
    rows, inter, code = c["rows"], c["inter"], ops.dt(d["ab"])
    rc = lib.muse_ffn_mid_fwd(d["ab"].data_ptr(), w.data_ptr(), d["h"].data_ptr(), d["hm"].data_ptr(), d["mean"].data_ptr(),
                              d["rstd"].data_ptr(), code, rows, inter, FFN_EPS, H.stream())
    assert rc == want, rc
    rc = lib.muse_ffn_mid_bwd(d["dhm"].data_ptr(), None if recomp else d["h"].data_ptr(), d["ab"].data_ptr(), w.data_ptr(),
                              d["mean"].data_ptr(), d["rstd"].data_ptr(), d["dab"].data_ptr(), d["part"].data_ptr(), code, rows, inter,
                              H.stream())
    assert rc == want, rc
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in bufs}


def ffn_layout_case(rows, inter, t, seed):
    """dhm is nonzero in one row of each block only (another place in each block; the last live row of a ragged block)"""
    c = ffn_case(rows, inter, t, seed)
    keep = torch.zeros(rows, dtype=torch.bool)
    for i in range(-(-rows // FFN_BLOCK)):
        keep[min(FFN_BLOCK * i + (3 * i + 2) % FFN_BLOCK, rows - 1)] = True
    c["dhm"] = c["dhm"] * keep[:, None].to(c["dhm"].dtype)
    return c


def rows_untouched(name, buf, rows):
    tail = buf[rows:].float()
    assert tail.numel() and bool((tail == SENT).all()), f"{name}: written past row {rows - 1}"


def ffn_layout_check(c, got):
    """got: the buffers of ffn_buffers after a forward + backward.  Partial row i = the float64 sum over rows [8 i, 8 i + 8) only,
    exactly ceil(rows / 8) partial rows written, nothing written past the last row of any output"""
    rows, inter = c["rows"], c["inter"]
    nblk = -(-rows // FFN_BLOCK)
    for k in ("h", "hm", "mean", "rstd", "dab"):
        rows_untouched("ffn_mid " + k, got[k], rows)
    assert bool(torch.isnan(got["part"][nblk:]).all()), "more than ceil(rows / 8) partial rows written"
    assert bool(torch.isfinite(got["part"][:nblk]).all()), "a partial row of a live block was not written"
    live = {k: got[k][:rows] for k in ("h", "hm", "mean", "rstd", "dab")}
    ffn_check(c, dict(live, dw=got["part"][:nblk].sum(0)))
    r = ffn_ref(c, F64, live["h"] if c["t"] == BF else None)
    for i in range(nblk):
        blk = slice(FFN_BLOCK * i, min(FFN_BLOCK * (i + 1), rows))
        ref = (c["dhm"][blk].double() * r["xhat"][blk]).sum(0)
        check("ffn_mid_dw", got["part"][i], ref, colsum_scale(c["dhm"][blk], ref))


def ffn_layout_emulate(c, mutant=None):
    """ffn_emulate into the buffers of ffn_buffers.  mutant 'next_block': partial row i holds the rows of block i + 1 (the last one
    those of block 0); 'dead_row': the row after the last live one is written with the last live row's results"""
    rows = c["rows"]
    nblk = -(-rows // FFN_BLOCK)
    e, got = ffn_emulate(c), ffn_buffers(c)
    for k in ("h", "hm", "mean", "rstd", "dab"):
        got[k][:rows] = e[k]
        if mutant == "dead_row":
            got[k][rows] = e[k][rows - 1]
    for i in range(nblk):
        j = (i + 1) % nblk if mutant == "next_block" else i
        blk = slice(FFN_BLOCK * j, min(FFN_BLOCK * (j + 1), rows))
        got["part"][i] = (c["dhm"][blk].float() * e["xhat"][blk]).sum(0)
    return got


FFN_LAYOUT_GENERIC = [(17, 4, F32), (9, 1028, F32), (17, 2052, BF), (25, 4092, BF)]


@pytest.mark.parametrize("rows,inter,t", FFN_LAYOUT_GENERIC, ids=lambda v: str(v).replace("torch.", ""))
def test_ffn_mid_generic_layout_and_stray_writes(rows, inter, t):
    for recomp in (False, True):
        c = ffn_layout_case(rows, inter, t, 3100 + rows + inter)
        got = ffn_run_c(c, ffn_buffers(c), recomp=recomp)
        ffn_layout_check(c, got)


@pytest.mark.parametrize("inter", FFN_WIDE_INTER)
def test_ffn_mid_wide_layout_and_stray_writes(inter):
    """the two-wave kernels walk 8 rows per pair: partial row i is still rows [8 i, 8 i + 8); a dead pair writes no partial row, a
    dead row (it is computed on the clamped row rows - 1) nothing at all"""
    for rows in FFN_WIDE_ROWS:
        for recomp in (False, True):
            c = ffn_layout_case(rows, inter, BF, 3300 + rows + inter)
            got = ffn_run_c(c, ffn_buffers(c), recomp=recomp)
            ffn_layout_check(c, got)


FFN_UNALIGNED_INTER, FFN_UNALIGNED_ROWS = [1024, 4096], 9


@pytest.mark.parametrize("which", ["ab", "h", "hm", "dhm", "dab"])
@pytest.mark.parametrize("inter", FFN_UNALIGNED_INTER)
def test_ffn_mid_wide_unaligned_takes_the_generic_kernel(inter, which):
    """one bf16 tensor at an address % 16 == 8 cannot take the 16-byte accesses of the two-wave kernels: the generic kernel runs, on
    that side, and is held to the same reference, layout and stray-write checks (w and the partial sums stay 16-byte aligned)"""
    rows = FFN_UNALIGNED_ROWS
    c = ffn_layout_case(rows, inter, BF, 3500 + inter)
    got = ffn_run_c(c, ffn_buffers(c), shift=which)
    ffn_layout_check(c, got)
    ref = ffn_run_c(c, ffn_buffers(c))
    print(f"[row_edges] ffn_mid {rows}x{inter} with {which} shifted: bit-equal to the aligned call "
          + " ".join(f"{k}={same_bits(got[k][:rows], ref[k][:rows])}" for k in ("h", "hm", "mean", "rstd", "dab")))


CHILD_SUBSET = "ffn_mid_wide"                                                   # (never matches the test below: a child starts no children)
CHILD_PASSES = len(FFN_WIDE_INTER) * 2 + 2 * 5


@pytest.mark.parametrize("bits", ["0", "3"])
def test_switch_in_a_child_interpreter(bits):
    """the wide-width tests of this file under the two other values of MUSE_FFN_MID_WIDE, which the library reads once per process:
    "0" puts the generic bf16 kernels on the multiples of 1024, "3" is the only way ffn_mid_bwd2_kernel<1..4> runs.  One child at a time."""
    e = dict(os.environ, MUSE_FFN_MID_WIDE=bits)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                            "-k", CHILD_SUBSET], capture_output=True, text=True, timeout=240, env=e)
    except subprocess.TimeoutExpired:
        pytest.exit(f"the child interpreter with MUSE_FFN_MID_WIDE={bits} hung: stopping", returncode=3)
    if r.returncode in (134, 139, -6, -11, 3):
        pytest.exit(f"the child interpreter with MUSE_FFN_MID_WIDE={bits} ended with {r.returncode}: stopping\n" + r.stdout[-1500:] + r.stderr[-1500:],
                    returncode=3)
    print("\n".join(ln for ln in r.stdout.splitlines() if "two-wave" in ln or "shifted" in ln))
    worst = [float(ln.rsplit("err/bound=", 1)[1].split()[0]) for ln in r.stdout.splitlines() if ln.startswith("[row_edges]") and "err/bound=" in ln]
    print(f"[row_edges] MUSE_FFN_MID_WIDE={bits}: worst err/bound of {len(worst)} checks in the child = {max(worst, default=0.0):.3f}")
    assert r.returncode == 0 and f"{CHILD_PASSES} passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


# =====================================================================================================================================
# ln_pair
# =====================================================================================================================================
LNP_COLS = [4, 256, 260, 512, 516, 768, 772, 1024]      # on and one vector past every NIT threshold
LNP_ROWS = [1, 18, 33]                                  # forward: 4 rows a block; backward: 16 (18: wave 0 of the last block holds two rows)
LNP_CASES = [(rows, cols, dres) for cols in LNP_COLS for rows in LNP_ROWS for dres in (False, True)]
LNP_OUT = ("x1", "ln2", "mean_post", "rstd_post", "mean_pre", "rstd_pre", "dx1", "dao", "dw_pre", "dw_post")


def lnp_case(rows, cols, dres, seed):
    return dict(ao=rounded(norm_input(rows, cols, seed), BF), x=randn((rows, cols), seed + 10), w_post=1.0 + 0.1 * randn((cols,), 51),
                w_pre=1.0 + 0.1 * randn((cols,), 52), dln2=rounded(randn((rows, cols), seed + 11), BF),
                dres=randn((rows, cols), seed + 12) if dres else None, rows=rows, cols=cols)


def lnp_seed(case):
    return 5000 + 3 * LNP_CASES.index(case)


def lnp_ref(c, dt):
    """x1 = x + LN(ao) w_post ; ln2 = LN(x1) w_pre ; dx1 = LN_pre'(dln2) + dres ; dao = LN_post'(dx1), by autograd in `dt`"""
    cols = c["cols"]
    ao = c["ao"].to(dt).requires_grad_(True)
    w_post, w_pre = c["w_post"].to(dt).clone().requires_grad_(True), c["w_pre"].to(dt).clone().requires_grad_(True)
    x1 = c["x"].to(dt) + F.layer_norm(ao, (cols,), w_post, None, LNP_EPS)
    x1.retain_grad()
    ln2 = F.layer_norm(x1, (cols,), w_pre, None, LNP_EPS)
    if c["dres"] is None:
        ln2.backward(c["dln2"].to(dt))
    else:
        torch.autograd.backward([ln2, x1], [c["dln2"].to(dt), c["dres"].to(dt)])
    a, v = ao.detach(), x1.detach()
    stat = lambda t: (t.mean(-1), 1.0 / torch.sqrt(t.var(-1, unbiased=False) + LNP_EPS))
    (mean_post, rstd_post), (mean_pre, rstd_pre) = stat(a), stat(v)
    return dict(x1=v, ln2=ln2.detach(), mean_post=mean_post, rstd_post=rstd_post, mean_pre=mean_pre, rstd_pre=rstd_pre, dx1=x1.grad,
                dao=ao.grad, dw_pre=w_pre.grad, dw_post=w_post.grad, xhat_post=(a - mean_post[:, None]) * rstd_post[:, None],
                xhat_pre=(v - mean_pre[:, None]) * rstd_pre[:, None])


def lnp_scales(c, r):
    return dict(x1=row_scale(r["x1"]), ln2=row_scale(r["ln2"]), mean_post=rowmax(c["ao"].double()), mean_pre=rowmax(r["x1"]),
                rstd_post=elem_scale(r["rstd_post"]), rstd_pre=elem_scale(r["rstd_pre"]), dx1=row_scale(r["dx1"]), dao=row_scale(r["dao"]),
                dw_pre=colsum_scale(c["dln2"], r["dw_pre"]), dw_post=colsum_scale(r["dx1"], r["dw_post"]))


def lnp_key(k):
    return "ln_pair_" + k


def lnp_check(c, out, only=LNP_OUT):
    r = lnp_ref(c, F64)
    s = lnp_scales(c, r)
    for k in only:
        check(lnp_key(k), out[k], r[k], s[k])
    const = c["ao"].float().std(-1, unbiased=False) == 0 if c["cols"] > 1 else None
    if "x1" in only and bool(const.any()):                                     # LN of a constant row is exactly 0: x1 = x there
        assert torch.equal(out["x1"].detach().cpu()[const], c["x"][const]), "x1 of a constant ao row is not x"


def lnp_emulate(c, mutant=None):
    """the pair's arithmetic in float32 torch.  mutant 'dres_first': dres is added to dln2's gradient path BEFORE the first LayerNorm
    backward instead of to its result"""
    n = float(c["cols"])
    ao, x, wp, wq, dln2 = c["ao"].float(), c["x"], c["w_post"], c["w_pre"], c["dln2"].float()

    def stats(t):
        mean = t.sum(-1) / n
        rstd = 1.0 / torch.sqrt(((t - mean[:, None]) ** 2).sum(-1) / n + LNP_EPS)
        return mean, rstd, (t - mean[:, None]) * rstd[:, None]

    def bwd(dy, xhat, rstd, w):
        g = dy * w
        c1, c2 = g.sum(-1, keepdim=True) / n, (g * xhat).sum(-1, keepdim=True) / n
        return rstd[:, None] * (g - c1 - xhat * c2), (dy * xhat).sum(0)

    mean_post, rstd_post, xh_post = stats(ao)
    x1 = x + xh_post * wp
    mean_pre, rstd_pre, xh_pre = stats(x1)
    dres = c["dres"] if c["dres"] is not None else torch.zeros_like(x)
    if mutant == "dres_first":
        dx1, dw_pre = bwd(dln2 + dres, xh_pre, rstd_pre, wq)
    else:
        dx1, dw_pre = bwd(dln2, xh_pre, rstd_pre, wq)
        dx1 = dx1 + dres
    dao, dw_post = bwd(dx1, xh_post, rstd_post, wp)
    return dict(x1=x1, ln2=(xh_pre * wq).to(BF), mean_post=mean_post, rstd_post=rstd_post, mean_pre=mean_pre, rstd_pre=rstd_pre, dx1=dx1,
                dao=dao.to(BF), dw_pre=dw_pre, dw_post=dw_post, xhat_pre=xh_pre, xhat_post=xh_post)


def lnp_run(c):
    ops = _ops()
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    x1, mp, rp, ln2, m2, r2 = ops.layernorm_pair_fwd(d["ao"], d["x"], d["w_post"], d["w_pre"], LNP_EPS)
    dw_pre, dw_post = torch.full((c["cols"],), SENT, device=DEV), torch.full((c["cols"],), SENT, device=DEV)
    dx1, dao = ops.layernorm_pair_bwd(d["dln2"], x1, d["w_pre"], m2, r2, d["dres"], d["ao"], d["w_post"], mp, rp, dw_pre, False, dw_post, False)
    return dict(x1=x1, ln2=ln2, mean_post=mp, rstd_post=rp, mean_pre=m2, rstd_pre=r2, dx1=dx1, dao=dao, dw_pre=dw_pre, dw_post=dw_post)


def lnp_two_calls(c):
    """the two muse_layernorm_fwd / _bwd calls that the pair replaces"""
    ops = _ops()
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    x1, mp, rp = ops.layernorm_fwd(d["ao"], d["w_post"], LNP_EPS, F32, residual=d["x"])
    ln2, m2, r2 = ops.layernorm_fwd(x1, d["w_pre"], LNP_EPS, BF)
    dw_pre, dw_post = torch.full((c["cols"],), SENT, device=DEV), torch.full((c["cols"],), SENT, device=DEV)
    dx1 = ops.layernorm_bwd(d["dln2"], x1, d["w_pre"], m2, r2, F32, dw_pre, False, dres=d["dres"])
    dao = ops.layernorm_bwd(dx1, d["ao"], d["w_post"], mp, rp, BF, dw_post, False)
    return dict(x1=x1, ln2=ln2, mean_post=mp, rstd_post=rp, mean_pre=m2, rstd_pre=r2, dx1=dx1, dao=dao, dw_pre=dw_pre, dw_post=dw_post)


LNP_BIT_EQUAL = ("mean_post", "rstd_post")               # what the pair shares with the two calls bit for bit at every case below


@pytest.mark.parametrize("cols", LNP_COLS)
def test_ln_pair_every_width(cols):
    """ln_pair_fwd_kernel<1..4> and ln_pair_bwd_kernel<1..4> (<4>, cols 772 .. 1024, through ops.layernorm_pair_bwd, which does not
    gate on the width) per row against the float64 composite, with and without dres; then bit for bit against the two calls"""
    equal = {k: True for k in LNP_OUT}
    for case in LNP_CASES:
        if case[1] != cols:
            continue
        c = lnp_case(*case, lnp_seed(case))
        out = lnp_run(c)
        lnp_check(c, out)
        again, two = lnp_run(c), lnp_two_calls(c)
        for k in LNP_OUT:
            assert same_bits(out[k], again[k]), f"{k}: a second run gives other bits"
            equal[k] = equal[k] and same_bits(out[k], two[k])
    print(f"[row_edges] ln_pair cols={cols}: bit-equal to the two calls " + " ".join(f"{k}={v}" for k, v in equal.items()))
    for k in LNP_BIT_EQUAL:
        assert equal[k], f"{k}: the pair and the two calls differ"


def lnp_buffers(c, extra=1, part_extra=2):
    rows, cols = c["rows"], c["cols"]
    nblk = -(-rows // LNP_BWD_BLOCK)
    full = lambda shape, v, dtype: torch.full(shape, v, dtype=dtype)
    d = {k: full((rows + extra,), SENT, F32) for k in ("mean_post", "rstd_post", "mean_pre", "rstd_pre")}
    d.update(x1=full((rows + extra, cols), SENT, F32), ln2=full((rows + extra, cols), SENT, BF), dx1=full((rows + extra, cols), SENT, F32),
             dao=full((rows + extra, cols), SENT, BF), part_pre=full((nblk + part_extra, cols), float("nan"), F32),
             part_post=full((nblk + part_extra, cols), float("nan"), F32))
    return d


def lnp_run_c(c, bufs, cols=None, nblk=None, want=0):
    """muse_layernorm_pair_fwd + _bwd on `bufs`; cols / nblk: what the entries are told instead of the truth (refusals)"""
    H = _hip()
    lib = H.lib()
    d = {k: v.to(DEV) for k, v in bufs.items()}
    i = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    rows = c["rows"]
    cols = c["cols"] if cols is None else cols
    if nblk is None:
        rc = lib.muse_layernorm_pair_fwd(i["ao"].data_ptr(), i["x"].data_ptr(), i["w_post"].data_ptr(), i["w_pre"].data_ptr(), d["x1"].data_ptr(),
                                         d["ln2"].data_ptr(), d["mean_post"].data_ptr(), d["rstd_post"].data_ptr(), d["mean_pre"].data_ptr(),
                                         d["rstd_pre"].data_ptr(), rows, cols, LNP_EPS, H.stream())
        assert rc == want, rc
    src = d if want == 0 else {k: torch.ones_like(v) for k, v in d.items()}      # (a refused forward leaves no x1 / statistics to read)
    rc = lib.muse_layernorm_pair_bwd(i["dln2"].data_ptr(), src["x1"].data_ptr(), i["w_pre"].data_ptr(), src["mean_pre"].data_ptr(),
                                     src["rstd_pre"].data_ptr(), i["dres"].data_ptr() if "dres" in i else None, i["ao"].data_ptr(),
                                     i["w_post"].data_ptr(), src["mean_post"].data_ptr(), src["rstd_post"].data_ptr(), d["dx1"].data_ptr(),
                                     d["dao"].data_ptr(), d["part_pre"].data_ptr(), d["part_post"].data_ptr(),
                                     -(-rows // LNP_BWD_BLOCK) if nblk is None else nblk, rows, cols, H.stream())
    assert rc == want, rc
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in bufs}


def lnp_layout_case(rows, cols, seed):
    """dln2 nonzero in one row of each 16-row block and no dres: dx1 is then nonzero in that row only, a sharp probe for both partials"""
    c = lnp_case(rows, cols, False, seed)
    keep = torch.zeros(rows, dtype=torch.bool)
    for i in range(-(-rows // LNP_BWD_BLOCK)):
        keep[min(LNP_BWD_BLOCK * i + (5 * i + 3) % LNP_BWD_BLOCK, rows - 1)] = True
    c["dln2"] = c["dln2"] * keep[:, None].to(BF)
    return c


def lnp_layout_check(c, got):
    rows = c["rows"]
    nblk = -(-rows // LNP_BWD_BLOCK)
    for k in LNP_OUT[:8]:
        rows_untouched("ln_pair " + k, got[k], rows)
    for k in ("part_pre", "part_post"):
        assert bool(torch.isnan(got[k][nblk:]).all()), f"{k}: more than ceil(rows / 16) partial rows written"
        assert bool(torch.isfinite(got[k][:nblk]).all()), f"{k}: a partial row of a live block was not written"
    live = {k: got[k][:rows] for k in LNP_OUT[:8]}
    lnp_check(c, dict(live, dw_pre=got["part_pre"][:nblk].sum(0), dw_post=got["part_post"][:nblk].sum(0)))
    r = lnp_ref(c, F64)
    for i in range(nblk):
        blk = slice(LNP_BWD_BLOCK * i, min(LNP_BWD_BLOCK * (i + 1), rows))
        ref = (c["dln2"][blk].double() * r["xhat_pre"][blk]).sum(0)
        check("ln_pair_dw_pre", got["part_pre"][i], ref, colsum_scale(c["dln2"][blk], ref))
        ref = (r["dx1"][blk] * r["xhat_post"][blk]).sum(0)
        check("ln_pair_dw_post", got["part_post"][i], ref, colsum_scale(r["dx1"][blk], ref))


def lnp_layout_emulate(c, mutant=None):
    rows = c["rows"]
    nblk = -(-rows // LNP_BWD_BLOCK)
    e, got = lnp_emulate(c), lnp_buffers(c)
    for k in LNP_OUT[:8]:
        got[k][:rows] = e[k]
        if mutant == "dead_row":
            got[k][rows] = e[k][rows - 1]
    for i in range(nblk):
        j = (i + 1) % nblk if mutant == "next_block" else i
        blk = slice(LNP_BWD_BLOCK * j, min(LNP_BWD_BLOCK * (j + 1), rows))
        got["part_pre"][i] = (c["dln2"][blk].float() * e["xhat_pre"][blk]).sum(0)
        got["part_post"][i] = (e["dx1"][blk] * e["xhat_post"][blk]).sum(0)
    return got


LNP_LAYOUT = [(18, 4), (33, 260), (18, 768), (33, 1024)]


@pytest.mark.parametrize("rows,cols", LNP_LAYOUT)
def test_ln_pair_layout_and_stray_writes(rows, cols):
    """partial row i of both weight gradients = rows [16 i, 16 i + 16) only (idle waves of a ragged last block add zeros), exactly
    ceil(rows / 16) partial rows, nothing past the last row of any output of either direction"""
    c = lnp_layout_case(rows, cols, 5500 + rows + cols)
    lnp_layout_check(c, lnp_run_c(c, lnp_buffers(c)))


# =====================================================================================================================================
# refusals: the entry answers before it launches anything
# =====================================================================================================================================
def all_untouched(got):
    for k, v in got.items():
        ok = torch.isnan(v).all() if k.startswith("part") else (v.float() == SENT).all()
        assert bool(ok), f"{k}: written by a refused call"


@pytest.mark.parametrize("t", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("inter", [4098, 4100])
def test_ffn_mid_refuses_and_writes_nothing(inter, t):
    """inter % 4 != 0 and inter > 4096 have no kernel: MUSE_ERR_UNSUPPORTED from both directions, every output as it was"""
    c = ffn_case(3, inter, t, 6000 + inter)
    all_untouched(ffn_run_c(c, ffn_buffers(c), want=ERR_UNSUPPORTED))
    ops, H = _ops(), _hip()
    ab = torch.cat([c["a"], c["b"]], 1).contiguous().to(DEV)
    with pytest.raises(H.MuseHipError, match="unsupported"):
        ops.ffn_mid_fwd(ab, c["w"].to(DEV), FFN_EPS)


@pytest.mark.parametrize("cols", [1026, 1028])
def test_ln_pair_refuses_and_writes_nothing(cols):
    c = lnp_case(3, cols, True, 6100 + cols)
    all_untouched(lnp_run_c(c, lnp_buffers(c), want=ERR_UNSUPPORTED))


@pytest.mark.parametrize("nblk", [1, 3])
def test_ln_pair_bwd_refuses_a_wrong_block_count(nblk):
    """18 rows are 2 blocks of 16: any other count of partial rows is MUSE_ERR_BAD_ARG, nothing launched"""
    c = lnp_case(18, 260, True, 6200)
    all_untouched(lnp_run_c(c, lnp_buffers(c), nblk=nblk, want=ERR_BAD_ARG))


# =====================================================================================================================================
# E_ref: torch's float32 CPU composite against float64 over the same cases (python tests/test_gpu_ffn_edges.py; no GPU)
# =====================================================================================================================================
def ffn_all_cases():
    """every input a test of this file gives the ffn_mid kernels"""
    for cases in (FFN_GENERIC_CASES, FFN_WIDE_CASES):
        for case in cases:
            yield ffn_case(*case, ffn_seed(cases, case))
    for rows, inter, t in FFN_LAYOUT_GENERIC:
        yield ffn_layout_case(rows, inter, t, 3100 + rows + inter)
    for inter in FFN_WIDE_INTER:
        for rows in FFN_WIDE_ROWS:
            yield ffn_layout_case(rows, inter, BF, 3300 + rows + inter)
    for inter in FFN_UNALIGNED_INTER:
        yield ffn_layout_case(FFN_UNALIGNED_ROWS, inter, BF, 3500 + inter)


def lnp_all_cases():
    for case in LNP_CASES:
        yield lnp_case(*case, lnp_seed(case))
    for rows, cols in LNP_LAYOUT:
        yield lnp_layout_case(rows, cols, 5500 + rows + cols)


def measure_e_ref():
    E = {}

    def put(name, got, ref, scale):
        E[name] = max(E.get(name, 0.0), measure(got, ref, scale))

    for c in ffn_all_cases():
        stored = ffn_ref(c, F64)["h"].to(BF) if c["t"] == BF else None           # bf16: both arithmetics start from one stored h
        r64, r32 = ffn_ref(c, F64, stored), ffn_ref(c, F32, stored)
        s = ffn_scales(c, r64)
        put("ffn_mid_h", r32["h"], r64["h"], s["h"])
        put("ffn_mid_hm", r32["hm"], r64["hm"], row_scale(r64["hm"]))
        put("ffn_mid_mean", r32["mean"], r64["mean"], s["mean"])
        put("ffn_mid_rstd", r32["rstd"], r64["rstd"], elem_scale(r64["rstd"]))
        put("ffn_mid_dh", r32["dh"], r64["dh"], row_scale(r64["dh"]))
        put("ffn_mid_dab", r32["dab"], r64["dab"], s["ln"] + s["glu"] + TINY)
        put("ffn_mid_dw", r32["dw"], r64["dw"], colsum_scale(c["dhm"], r64["dw"]))
    for c in lnp_all_cases():
        r64, r32 = lnp_ref(c, F64), lnp_ref(c, F32)
        s = lnp_scales(c, r64)
        for k in LNP_OUT:
            put(lnp_key(k), r32[k], r64[k], s[k])
    return E


if __name__ == "__main__":
    torch.set_num_threads(8)
    for k, v in measure_e_ref().items():
        print(f'    "{k}": {v:.3e},')
