"""tests/attention_dropout_cpu.py checked on the CPU: the float64 reference against autograd, the contract model inside its own bound, and -
the point of this file - the GPU test's checks FAIL for the four defects a fused-dropout kernel can have: a mask shifted by one key, a
mask built with ld_mask = Skv instead of the row pitch, an offset whose high 32 bits are ignored, a missing 1 / (1 - p).  contract_model
with the defective mask stands in for the kernel."""
import pytest
import torch

import attention_cpu as A
import attention_dropout_cpu as D

SHAPE = (33, 77, 64)            # cross-attention, row pitch 80 != Skv
SMALL = (17, 17, 16)
P, OFFSET = 0.5, 3 << 40


def test_mask_is_the_dropout_stream_on_the_padded_layout():
    import philox_cpu as PH
    Sq, Skv = 5, 13
    keep = D.keep_mask(2, 3, Sq, Skv, 0.3, 99, 2 ** 32 - 5)
    flat = PH.dropout_keep(2 * 3 * Sq * 16, 0.3, 99, 2 ** 32 - 5)
    for bh, q, k in ((0, 0, 0), (1, 4, 12), (5, 2, 7), (3, 0, 3)):
        assert bool(keep[bh // 3, bh % 3, q, k]) == bool(flat[(bh * Sq + q) * 16 + k])
    assert D.row_pitch(77) == 80 and D.row_pitch(257) == 264 and D.row_pitch(80) == 80


def test_reference_gradients_are_autograd_gradients():
    """the float64 formulas (dS = P (keep s dP - dsum), dV = (P keep s)^T dO) against torch.autograd on softmax -> mask -> matmul"""
    Sq, Skv, hd = SMALL
    c = D.random_case(Sq, Skv, hd)
    keep = D.case_keep(Sq, Skv, P, OFFSET)
    ref = D.reference(c, keep, P)
    q, k, v, do = (t.clone().requires_grad_(True) for t in A._operands(c, torch.float64))
    pr = torch.softmax((q @ k.transpose(-1, -2)) * float(c["alpha"]), -1)
    o = (pr * keep * D.drop_scale(P)) @ v
    o.backward(do.detach())
    assert torch.allclose(A.to_rows(o.detach()), ref["ctx"], rtol=1e-12, atol=1e-14)
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        assert torch.allclose(A.to_rows(t.grad), ref[n], rtol=1e-10, atol=1e-13), n


@pytest.mark.parametrize("shape", [SMALL, SHAPE])
def test_contract_model_passes_every_check(shape):
    Sq, Skv, hd = shape
    c = D.random_case(Sq, Skv, hd)
    keep = D.case_keep(Sq, Skv, P, OFFSET)
    fwd, bwd = D.model_runner(keep, P)
    D.run_probes(c, keep, fwd, bwd, "model")
    f = fwd(c)
    out = dict(f, **bwd(c, f["ctx"], f["lse"]))
    A.check_random(c, out, D.case_reference(Sq, Skv, hd, P, OFFSET), D.e_ref_for(Sq, Skv), tag="model")
    for n, e in D.model_errors(c, keep, P, D.case_reference(Sq, Skv, hd, P, OFFSET)).items():
        assert e <= 1.001 * D.e_ref_for(Sq, Skv)[n], n   # (E_REF_DROP, four digits of it, is the worst over the list this shape is in)


def _defective_masks():
    Sq, Skv, _ = SHAPE
    good = D.case_keep(Sq, Skv, P, OFFSET)
    return good, {
        "shifted by one key": torch.roll(good, 1, -1),
        "ld_mask = Skv": D.keep_mask(D.B, D.NH, Sq, Skv, P, D.SEED, OFFSET, ld_mask=Skv),
        "high offset word ignored": D.keep_mask(D.B, D.NH, Sq, Skv, P, D.SEED, OFFSET & 0xFFFFFFFF),
    }


@pytest.mark.parametrize("defect", ["shifted by one key", "ld_mask = Skv", "high offset word ignored"])
@pytest.mark.parametrize("kernel", ["forward", "dQ", "dK", "dV"])
def test_probes_catch_a_wrong_mask(defect, kernel):
    """each probe alone: the kernel under it draws the defective mask, the other two the right one"""
    Sq, Skv, hd = SHAPE
    c = D.random_case(Sq, Skv, hd)
    good, bad = _defective_masks()
    gf, gb = D.model_runner(good, P)
    bf_, bb = D.model_runner(bad[defect], P)

    def bwd(case, ctx, lse):
        out, wrong = gb(case, ctx, lse), bb(case, ctx, lse)
        if kernel != "forward":
            n = {"dQ": "dq", "dK": "dk", "dV": "dv"}[kernel]
            out[n] = wrong[n]
        return out
    with pytest.raises(AssertionError, match=kernel + " .* window"):
        D.run_probes(c, good, bf_ if kernel == "forward" else gf, bwd, "defect")


def test_parity_catches_a_missing_scale():
    """keep bits right, 1 / (1 - p) missing: the probes cannot see it (non-zero stays non-zero), the float64 comparison must - at p = 0.1
    too, where the factor is only 1.11"""
    Sq, Skv, hd = SHAPE
    c = D.random_case(Sq, Skv, hd)
    for p in D.PS:
        keep = D.case_keep(Sq, Skv, p, OFFSET)
        fwd, bwd = D.model_runner(keep, p, scale=1.0)
        D.run_probes(c, keep, fwd, bwd, "unscaled")
        f = fwd(c)
        for n, t in dict(f, **bwd(c, f["ctx"], f["lse"])).items():
            if n == "lse":
                continue
            with pytest.raises(AssertionError, match="x its bound"):
                A.check_random(c, {n: t}, D.case_reference(Sq, Skv, hd, p, OFFSET), D.e_ref_for(Sq, Skv), tag=f"unscaled {n}")
