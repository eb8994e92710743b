"""GPU (-m gpu): the kernels that make a training step's inputs and its soft-target loss - muse_soft_ce_fwd / muse_soft_ce_bwd and
muse_mask_sample (csrc/rowops.hip), muse_mask_tokens and muse_cond_dropout (csrc/sampling.hip) - at every branch of their launchers.
tests/objective_cpu.py holds the case lists, the references and the checkers; tests/test_objective_cpu.py proves on the CPU that each
checker fails on a wrong model.  profiles/objective_edges.md has the table.

Soft-target cross entropy.  The reference is float64 torch on the documented contract.  The bound of a quantity is 4 * E_REF[kind],
plus one bf16 ulp of the reference for a bf16 gradient.  E_REF is the worst normalised error, over the same case lists, of torch
float32 evaluating the kernel's documented form - psum * lse - sum(p * l) and g / n * (exp(l - lse) * psum - p), not the better
conditioned -(p * log_softmax).sum() - against float64; `python tests/test_gpu_objective_edges.py` prints it (no GPU needed).
Normalisers: loss and psum relative; lse over max(1, |lse|); the row loss over psum |lse| + sum(p |l|) and the gradient, per element, over
|g| / n * (softmax * psum + p) - the two terms each subtracts - all with the 2^-102 floor of tests/test_gpu_row_edges.py.  Every |logit|
is at most 32.

Operands sit inside larger allocations with NaN in front of them, behind them and in every ld > K gap; by default the logits of inactive
rows and the soft rows of label -100 positions are NaN as well (the kernels promise not to read them).  Outputs sit inside buffers filled
with a sentinel that must come back unchanged outside the documented extent.

Mask sampling and conditioning dropout are integer / bit comparisons against oracle/maskgit_oracle.py on the CPU (for tied noise, where
the oracle's argsort is not stable, against the stable restatement of objective_cpu.py).
"""
import math

import pytest
import torch

import objective_cpu as C
from oracle import maskgit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
PAD = 64                      # elements of sentinel / NaN in front of and behind every buffer (64 f32 = 256 bytes: alignment is kept)
BAD_ARG, UNSUPPORTED = -1, -3

# Worst normalised error of the float32 torch model of the kernels' documented form against float64 over soft_ce_all_cases(), as
# printed by `python tests/test_gpu_objective_edges.py`.  The bound of a kind is 4 * E_REF[kind] (+ one bf16 ulp for a bf16 gradient).
E_REF = {                           # bound = 4 * E_ref
    "soft_ce_loss": 1.164e-07,      # 4.7e-07  relative
    "soft_ce_lse": 8.071e-08,       # 3.2e-07  over max(1, |lse|)
    "soft_ce_psum": 1.645e-07,      # 6.6e-07  relative
    "soft_ce_row_loss": 1.369e-07,  # 5.5e-07  over psum |lse| + sum(p |l|)
    "soft_ce_grad": 3.951e-06,      # 1.6e-05  per element over |g| / n (softmax psum + p): a spread-60 row (l - lse down to -60 in the exponent)
}

WORST = {}                          # kind -> worst err / bound seen in this process (printed by the last soft-CE test)


def _lib():
    from muse import _hip
    return _hip.lib(), _hip.stream()


def _ops():
    from muse import ops
    return ops


class Buf:
    """a region of n elements inside a device allocation with PAD (+ off) guard elements in front and PAD behind"""

    def __init__(self, n, dtype, fill, off=0, body=None):
        self.n, self.lo = n, PAD + off
        host = torch.full((self.lo + n + PAD,), fill, dtype=dtype)
        if body is not None:
            host[self.lo:self.lo + n] = body.reshape(-1).to(dtype)
        self.host = host.clone()
        self.t = host.to(DEV)
        self.ptr = self.t.data_ptr() + self.lo * self.t.element_size()

    def get(self):
        return self.t[self.lo:self.lo + self.n].cpu()

    def guards_intact(self):
        got = self.t.cpu()
        return (torch.equal(C.bits(got[:self.lo]), C.bits(self.host[:self.lo]))
                and torch.equal(C.bits(got[self.lo + self.n:]), C.bits(self.host[self.lo + self.n:])))

    def untouched(self):
        return torch.equal(C.bits(self.t.cpu()), C.bits(self.host))


def run_soft_ce(c, poison=True):
    """both kernels on one case through the C entry points -> the outputs on the CPU (objective_cpu.soft_ce_check's format)"""
    lib, stream = _lib()
    B, S1, K, ld, ldo = c["B"], c["S1"], c["K"], c["ld"], c["ldo"]
    rows = B * S1
    active, _ = C.soft_ce_rows(B, S1, c["labels"])
    body = torch.full((rows, ld), NAN if poison else 0.5)
    body[:, :K] = c["x"]
    soft = c["soft"].clone()
    if poison:
        body[~active] = NAN
        dead = (c["labels"].view(B, S1)[:, 1:] == -100).reshape(-1)
        soft[dead] = NAN
    logits = Buf(rows * ld, F32, NAN, off=c["in_off"], body=body)
    softb = Buf(soft.numel(), F32, NAN, body=soft)
    labels = Buf(rows, torch.int64, 12345, body=c["labels"])
    row_loss, lse, psum = (Buf(rows, F32, C.SENTINEL) for _ in range(3))
    loss_out = Buf(2, F32, C.SENTINEL)
    gout = Buf(1, F32, NAN, body=torch.tensor([c["g"]]))
    dl = Buf(rows * ldo, c["out"], C.SENTINEL, off=c["out_off"])
    # the alignment the case is about
    assert logits.ptr % 16 == (c["in_off"] * 4) % 16 and softb.ptr % 16 == 0
    assert dl.ptr % 16 == (c["out_off"] * dl.t.element_size()) % 16
    code = lib.muse_soft_ce_fwd(logits.ptr, labels.ptr, softb.ptr, row_loss.ptr, lse.ptr, psum.ptr, loss_out.ptr, rows, S1, K, ld, stream)
    assert code == 0, code
    code = lib.muse_soft_ce_bwd(logits.ptr, labels.ptr, softb.ptr, lse.ptr, psum.ptr, loss_out.ptr, gout.ptr, dl.ptr,
                                0 if c["out"] == F32 else 1, rows, S1, K, ld, ldo, stream)
    assert code == 0, code
    torch.cuda.synchronize()
    for name, b in (("row_loss", row_loss), ("lse", lse), ("psum", psum), ("loss_out", loss_out), ("dlogits", dl)):
        assert b.guards_intact(), f"{c['name']}: a write outside {name}"
    for name, b in (("logits", logits), ("soft", softb), ("labels", labels), ("grad_out", gout)):
        assert b.untouched(), f"{c['name']}: the input {name} was written"
    return dict(loss_out=loss_out.get(), lse=lse.get(), psum=psum.get(), row_loss=row_loss.get(), dl=dl.get().view(rows, ldo))


def check_soft_ce(c, out=None):
    out = run_soft_ce(c) if out is None else out
    ratios = C.soft_ce_check(c, out, E_REF)
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"[objective_edges] {c['name']:28s} rows={c['B'] * c['S1']:5d} K={c['K']:5d} ld={c['ld']:5d} ldo={c['ldo']:5d} "
          f"branch={C.soft_ce_branch(c):13s} " + " ".join(f"{k[8:]}={v:.3f}" for k, v in ratios.items()))
    return out


def same_bits(a, b):
    return all(torch.equal(C.bits(a[k]), C.bits(b[k])) for k in ("loss_out", "lse", "psum", "row_loss", "dl"))


# =====================================================================================================================================
# A1. soft-target cross entropy
# =====================================================================================================================================
def test_soft_ce_every_launcher_branch():
    """K = 1024 / 512 / 256 aligned (register-resident vector kernels), K = 1024 with an odd ld and with the base one float off (register
    scalar kernel), K = 512 / 256 with an odd ld and eight other K (generic two-pass kernel), f32 and bf16 gradient each; the routes that
    differ only by alignment must both meet the bound.  Two runs of a case give the same bits."""
    seen = set()
    for c in C.soft_ce_branch_cases():
        out = check_soft_ce(c)
        assert same_bits(out, run_soft_ce(c)), f"{c['name']}: two runs differ in bits"
        seen.add(C.soft_ce_branch(c))
    assert seen == {"K1024 vector", "K1024 scalar", "K512 vector", "K256 vector", "generic"}


def test_soft_ce_row_tails():
    """2, 9, 5 and 65 rows: a last block of 2, 1, 1 and 1 waves, on a vector and on the generic kernel"""
    for c in C.soft_ce_tail_cases():
        check_soft_ce(c)


def test_soft_ce_reduce_below_at_and_over_one_block():
    """1023, 1024, 1025 and 1285 rows at K = 64 through the single 1024-thread reduce: n_active exact, the loss within its bound"""
    for c in C.soft_ce_reduce_cases():
        check_soft_ce(c)


def test_soft_ce_output_widths_and_alignments():
    """ldo = K, K + 4, K + 260, K + 1, K + 3, ldo on either side of ld; bf16 gradients at an 8- and at a 2-byte aligned pointer, an f32
    one at a 4-byte aligned pointer: every element outside the active [rows, :K] block an exact +0, nothing behind rows * ldo"""
    for c in C.soft_ce_width_cases():
        check_soft_ce(c)


def test_soft_ce_no_active_row():
    """every label -100 or at position 0: loss NaN, count 0, the gradient all exact +0 without a NaN"""
    for c in C.soft_ce_label_cases():
        out = check_soft_ce(c)
        assert math.isnan(float(out["loss_out"][0])) and float(out["loss_out"][1]) == 0.0
        assert not bool(C.bits(out["dl"]).any())


def test_soft_ce_reads_nothing_it_promises_not_to():
    """NaN in the logits of inactive rows, in columns [K, ld) and in the soft rows of label -100 positions: the bits of a clean run"""
    cases = [c for c in C.soft_ce_branch_cases() if "generic" not in c["name"] or c["K"] in (65, 1000)] + C.soft_ce_tail_cases()
    for c in cases:
        assert same_bits(run_soft_ce(c, poison=True), run_soft_ce(c, poison=False)), c["name"]


def test_soft_ce_refusals_write_nothing():
    """seq1 < 2, rows % seq1 != 0, K > ld, K > ldo: MUSE_ERR_BAD_ARG; a third gradient dtype: MUSE_ERR_UNSUPPORTED; no output touched"""
    lib, stream = _lib()
    rows, S1, K, ld = 6, 3, 64, 64
    x = Buf(rows * ld, F32, NAN, body=torch.zeros(rows, ld))
    soft = Buf(4 * K, F32, NAN, body=torch.full((4, K), 1.0 / K))
    labels = Buf(rows, torch.int64, 12345, body=torch.ones(rows, dtype=torch.int64))
    outs = [Buf(rows, F32, C.SENTINEL) for _ in range(3)] + [Buf(2, F32, C.SENTINEL), Buf(rows * ld, F32, C.SENTINEL)]
    rl, lse, ps, lo, dl = outs
    gout = Buf(1, F32, NAN, body=torch.ones(1))
    fwd = lambda rows_, s1, k, ld_: lib.muse_soft_ce_fwd(x.ptr, labels.ptr, soft.ptr, rl.ptr, lse.ptr, ps.ptr, lo.ptr, rows_, s1, k, ld_, stream)  # noqa: E731
    bwd = lambda dt, rows_, s1, k, ld_, ldo: lib.muse_soft_ce_bwd(x.ptr, labels.ptr, soft.ptr, lse.ptr, ps.ptr, lo.ptr, gout.ptr, dl.ptr, dt,  # noqa: E731
                                                                  rows_, s1, k, ld_, ldo, stream)
    assert fwd(rows, 1, K, ld) == BAD_ARG and bwd(0, rows, 1, K, ld, ld) == BAD_ARG                  # seq1 < 2
    assert fwd(rows, 4, K, ld) == BAD_ARG and bwd(0, rows, 4, K, ld, ld) == BAD_ARG                  # rows % seq1 != 0
    assert fwd(rows, S1, K, K - 1) == BAD_ARG and bwd(0, rows, S1, K, K - 1, ld) == BAD_ARG          # K > ld
    assert bwd(0, rows, S1, K, ld, K - 1) == BAD_ARG and bwd(1, rows, S1, K, ld, K - 1) == BAD_ARG   # K > ldo
    assert bwd(2, rows, S1, K, ld, ld) == UNSUPPORTED                                                # a third gradient dtype
    torch.cuda.synchronize()
    assert all(b.untouched() for b in outs)
    assert fwd(rows, S1, K, ld) == 0 and bwd(0, rows, S1, K, ld, ld) == 0                            # the same buffers, accepted
    torch.cuda.synchronize()
    assert not lo.untouched() and not dl.untouched()


def test_soft_ce_wrapper_matches_the_entry_points():
    """ops.soft_ce_fwd / soft_ce_bwd (the route training takes: ldo = width, 16-byte aligned tensors) give the bits of the direct call"""
    ops = _ops()
    for name in ("K1024-aligned", "K256-aligned-bf16", "K65-generic"):
        c = next(x for x in C.soft_ce_branch_cases() if x["name"] == name)
        rows = c["B"] * c["S1"]
        buf = torch.full((rows, c["ld"]), 0.5)
        buf[:, :c["K"]] = c["x"]
        logits = buf.to(DEV)[:, :c["K"] + (c["ld"] - c["K"]) // 2]
        labels, soft = c["labels"].to(DEV), c["soft"].to(DEV)
        loss_out, lse, psum = ops.soft_ce_fwd(logits, labels, soft, c["S1"])
        dl = ops.soft_ce_bwd(logits, labels, soft, c["S1"], lse, psum, loss_out, torch.tensor([c["g"]], device=DEV), out_dtype=c["out"],
                             width=c["ldo"])
        ref = run_soft_ce(c, poison=False)
        assert torch.equal(C.bits(loss_out.cpu()), C.bits(ref["loss_out"])) and torch.equal(C.bits(lse.cpu()), C.bits(ref["lse"]))
        assert torch.equal(C.bits(psum.cpu()), C.bits(ref["psum"])) and torch.equal(C.bits(dl.cpu()), C.bits(ref["dl"]))


def test_soft_ce_report():
    """prints the worst err / bound per kind over the soft-CE tests of this process (profiles/objective_edges.md records a run)"""
    for k, v in sorted(WORST.items()):
        print(f"[objective_edges] worst err / bound  {k}: {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())


# =====================================================================================================================================
# A2. mask sampling
# =====================================================================================================================================
def run_mask_sample(c, expect=0):
    lib, stream = _lib()
    B, S = c["tokens"].shape
    tok = Buf(B * S, torch.int64, -7, body=c["tokens"])
    cls = Buf(B, torch.int64, -7, body=c["class_ids"])
    t = Buf(B, F32, NAN, body=c["timesteps"])
    nz = Buf(B * S, F32, NAN, body=c["noise"])
    ids, labels = Buf(B * (S + 1), torch.int64, -7), Buf(B * (S + 1), torch.int64, -7)
    prob = Buf(B, F32, C.SENTINEL)
    code = lib.muse_mask_sample(tok.ptr, cls.ptr, t.ptr, nz.ptr, ids.ptr, labels.ptr, prob.ptr, B, S, c["mask_id"], c["codebook"],
                                c["min_rate"], stream)
    torch.cuda.synchronize()
    assert code == expect, code
    outs = (ids, labels, prob)
    if expect != 0:
        assert all(b.untouched() for b in outs), "a refused call wrote to its outputs"
        return None
    assert all(b.guards_intact() for b in outs) and all(b.untouched() for b in (tok, cls, t, nz))
    return ids.get().view(B, S + 1), labels.get().view(B, S + 1), prob.get()


@pytest.mark.parametrize("S", C.MASK_SAMPLE_S)
def test_mask_sample_every_length(S):
    """S on both sides of the block size and at the limit: seeded timesteps (whose S * p is asserted to be 1e-3 away from any half),
    t = 0 (k = S), t = 1 (the clamp to 1), tied noise - all equal, four values, one pair - against the stable restatement and, without
    ties, the oracle"""
    for c in C.mask_sample_cases([S]):
        assert C.margin_ok(c), f"{c['name']}: S * p within 1e-3 of a half-integer"
        C.mask_sample_check(c, run_mask_sample(c))


def test_mask_sample_round_half_to_even():
    """t = 1 clipped to min_masking_rate 0.25 at S = 2, 6, 10, 14: S * p = 0.5, 1.5, 2.5, 3.5 -> k = 1, 2, 2, 4"""
    cases = [c for c in C.mask_sample_cases([]) if "half-even" in c["name"]]
    assert len(cases) == 8
    for c in cases:
        C.mask_sample_check(c, run_mask_sample(c))


def test_mask_sample_refuses_1025():
    c = C.mask_sample_cases([2])[0]
    c = dict(c, tokens=C._tokens(3, 1025, C.CODEBOOK, 5), noise=C.tie_free(3, 1025, 5))
    run_mask_sample(c, expect=UNSUPPORTED)


def run_mask_tokens(c, expect=0, drop=()):
    """drop: operands handed over as NULL although the case has them"""
    lib, stream = _lib()
    kw = c["kw"]
    B, S = c["tokens"].shape
    tok = Buf(B * S, torch.int64, -7, body=c["tokens"])
    opt = lambda k, dt, fill: None if kw.get(k) is None or k in drop else Buf(kw[k].numel(), dt, fill, body=kw[k])   # noqa: E731
    t, mp, nz, rects = opt("timesteps", F32, NAN), opt("mask_prob", F32, NAN), opt("noise", F32, NAN), opt("rects", torch.int32, 9999)
    ids, labels = Buf(B * S, torch.int64, -7), Buf(B * S, torch.int64, -7)
    lw = Buf(B * S, F32, C.SENTINEL) if kw["all_labels"] else None
    prob = Buf(B, F32, C.SENTINEL)
    p = lambda b: None if b is None else b.ptr   # noqa: E731
    code = lib.muse_mask_tokens(tok.ptr, p(t), p(mp), p(nz), p(rects), ids.ptr, labels.ptr, p(lw), prob.ptr, B, S, c["mask_id"],
                                kw["min_rate"], 1 if kw["all_labels"] else 0, 0.3, stream)
    torch.cuda.synchronize()
    assert code == expect, code
    outs = [b for b in (ids, labels, lw, prob) if b is not None]
    if expect != 0:
        assert all(b.untouched() for b in outs), "a refused call wrote to its outputs"
        return None
    assert all(b.guards_intact() for b in outs) and all(b.untouched() for b in (tok, t, mp, nz, rects) if b is not None)
    return ids.get().view(B, S), labels.get().view(B, S), None if lw is None else lw.get().view(B, S), prob.get()


@pytest.mark.parametrize("S", C.MASK_TOKENS_S)
def test_mask_tokens_every_length(S):
    """as test_mask_sample_every_length up to S = 4096, with the exact halves through mask_prob, the eval branch (mask_prob given: not
    clipped by min_masking_rate) and all_labels with its loss weight"""
    for c in C.mask_tokens_cases([S]):
        assert C.margin_ok(c), f"{c['name']}: S * p within 1e-3 of a half-integer"
        C.mask_tokens_check(c, run_mask_tokens(c))


def test_mask_tokens_rectangles():
    """sides 1, 2, 16, 64: the whole grid, h = 0, one cell per corner, rectangles overhanging the right and bottom border"""
    for c in C.rect_cases():
        C.mask_tokens_check(c, run_mask_tokens(c))


def test_mask_tokens_wrapper_and_all_labels_without_weight():
    """ops.mask_tokens: all_labels with and without the loss weight"""
    ops = _ops()
    c = next(x for x in C.mask_tokens_cases([257]) if x["name"] == "S257-seeded-all-labels")
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c["kw"].items()}
    min_rate = kw.pop("min_rate")
    for want_weight in (True, False):
        got = ops.mask_tokens(c["tokens"].to(DEV), c["mask_id"], min_masking_rate=min_rate, want_weight=want_weight, **kw)
        got = tuple(None if g is None else g.cpu() for g in got)
        assert (got[2] is not None) == want_weight
        want = C.mask_tokens_ref(c["tokens"], c["mask_id"], **c["kw"])
        C.mask_check(c["name"], got, want if want_weight else (want[0], want[1], None, want[3]))


def test_mask_tokens_refusals_write_nothing():
    cs = {c["name"]: c for c in C.mask_tokens_cases([4])}
    base = cs["S4-seeded"]
    big = dict(base, tokens=C._tokens(3, 4097, C.CODEBOOK, 3), kw=dict(base["kw"], noise=C.tie_free(3, 4097, 3)))
    run_mask_tokens(big, expect=UNSUPPORTED)                                           # S = 4097
    rect = C.rect_cases()[2]                                                           # side 2
    nb = rect["tokens"].shape[0]
    run_mask_tokens(dict(rect, tokens=C._tokens(nb, 5, C.CODEBOOK, 3)), expect=BAD_ARG)  # rectangles on a non-square S
    run_mask_tokens(base, expect=BAD_ARG, drop=("timesteps",))                         # neither timesteps nor mask_prob
    run_mask_tokens(base, expect=BAD_ARG, drop=("noise",))                             # neither noise nor rects


# =====================================================================================================================================
# A3. conditioning dropout
# =====================================================================================================================================
def test_cond_dropout_bit_for_bit():
    """per_image 1 / 255 / 257, B 1 / 3 / 12 and 524289 elements (the grid-stride path, one past 2048 blocks); u == p, the f32 below
    p, p = 0, p = 1; 0.0, -0.0, NaN, inf, a subnormal and an ordinary value in kept and dropped images - bits of the oracle"""
    lib, stream = _lib()
    for c in C.cond_dropout_cases():
        B, per = c["x"].shape
        x, e, u = Buf(B * per, F32, NAN, body=c["x"]), Buf(per, F32, NAN, body=c["empty"]), Buf(B, F32, NAN, body=c["u"])
        out = Buf(B * per, F32, C.SENTINEL)
        code = lib.muse_cond_dropout(x.ptr, e.ptr, u.ptr, out.ptr, B, per, c["p"], stream)
        torch.cuda.synchronize()
        assert code == 0, code
        assert out.guards_intact() and x.untouched() and e.untouched() and u.untouched()
        C.cond_dropout_check(c, out.get().view(B, per))
        got = _ops().cond_dropout(c["x"].to(DEV), c["empty"].to(DEV), c["u"].to(DEV), c["p"]).cpu()
        C.cond_dropout_check(c, got)


def test_cond_dropout_what_the_oracle_does_with_special_values():
    """pins the oracle's corners themselves: a kept image keeps everything but the two zeros, which take the empty value; a dropped one
    takes the empty value except at NaN and inf"""
    x = torch.tensor([C.SPECIALS, C.SPECIALS])
    empty = torch.arange(6.0) + 10.0
    u = torch.tensor([0.0, 0.9])
    got = _ops().cond_dropout(x.to(DEV), empty.to(DEV), u.to(DEV), 0.5).cpu()
    want_kept = torch.tensor([10.0, 11.0, NAN, math.inf, 1e-42, 1.5])
    want_drop = torch.tensor([10.0, 11.0, NAN, math.inf, 14.0, 15.0])
    assert torch.equal(C.bits(got), C.bits(torch.stack([want_kept, want_drop])))
    assert torch.equal(C.bits(O.cond_dropout(x, empty, u, 0.5)), C.bits(got))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for k, v in C.measure_soft_ce_e_ref().items():
        print(f'    "{k}": {v:.3e},')
