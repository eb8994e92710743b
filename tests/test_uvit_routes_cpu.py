"""The checks of tests/test_gpu_uvit_routes.py have teeth (no GPU): every seeded routing defect of tests/uvit_routes_cpu.py, put into the
float64 oracle, lands at least 4 times above the f32, bf16x3 and f16 bounds of every case it applies to (2 times above the bf16 bound), in
the logits or in the worst gradient; the oracle itself is well conditioned on every case (its own float32 run within 1e-5 of float64)."""
import math

import pytest
import torch

import uvit_routes_cpu as R

# (case, defect) pairs whose distance stays below 2 x the bf16 bound, with (logits distance / bound, worst gradient distance / bound): the
# bf16 leg of such a case carries no evidence against that defect.  None today; an f32, bf16x3 or f16 entry is never allowed.
NO_TEETH_BF16 = {}

PAIRS = [(c, d) for c in R.CASES for d in R.DEFECTS if R.applies(c, d)]


def test_the_case_table_has_a_case_for_every_named_route():
    names = {c.name for c in R.CASES}
    assert {"s16_L77_B2", "s32_L77_B1", "s32_L77_B2", "s32_L77_B1_pairs", "s16_L512_B2", "s32_L512_B1", "s16_L256_B2", "s32_L256_B1", "s16_L64",
            "s16_L96", "s16_L97", "s16_L224", "s16_L225", "s16_L1", "s15_L77_B1", "s17_L77_B3", "s8_L77_B2", "h4_s16", "h1_w64_s16", "c96_s16",
            "ln_s16", "noaffine_s16", "down_s32", "down_s64", "h1_w64_s32_B1"} <= names
    for c in R.CASES:
        assert c.side * c.side <= 4096 and c.B <= 3
    for d in R.DEFECTS:                     # every defect is exercised, and on more than one route
        assert sum(1 for c in R.CASES if R.applies(c, d)) >= 2, d
    cfg = R.config(R.BY_NAME["c96_s16"])
    assert cfg["block_out_channels"][0] // cfg["block_num_heads"] == 48 and R.inner_tokens(R.BY_NAME["down_s64"]) == 1024


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_the_reference_is_finite_and_well_conditioned(case):
    logits, loss, grads = R.reference(case)
    assert torch.isfinite(logits).all() and math.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    # every parameter takes part - but, over ONE text state (a constant softmax), the queries and keys of the attentions over the text and
    # what feeds those queries alone: the conv-stage blocks' two norms, the layers' cross-attention norm and its AdaLN mapper
    text = [k for k in grads if ".crossattention." in k or ".attention_blocks." in k or ".crossattn_layer_norm." in k or ".cross_attn_adaLN" in k]
    single = [k for k in text if not k.endswith((".value.weight", ".out.weight"))]
    assert R.zero_gradients(case) == (sorted(single) if case.L == 1 else [])
    el, es, eg = R.distance(R.reference_f32(case), R.reference(case))
    k, e = R.worst(eg)
    print(case.name, "oracle f32 against f64: logits", f"{el:.1e}", "loss", f"{es:.1e}", "worst gradient", f"{e:.1e}", f"({k})")
    assert el < 1e-5 and es < 1e-5 and e < 1e-5
    bl, bs, bg = R.bounds(case, torch.float32)
    assert (bl, bg) == (R.M_F32 * el, R.M_F32 * e) and R.M_F32 * max(es, 2.0 ** -24) <= bs < R.M_F32 * 1e-6 and R.M_F32 <= 64


@pytest.mark.parametrize("case,defect", PAIRS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_bound_sits_below_every_seeded_defect(case, defect):
    dl, ds, dg = R.distance(R.defective(case, defect), R.reference(case))
    dgw = R.worst(dg)[1]
    for mode in (torch.float32, "bf16x3", "f16"):
        bl, _, bg = R.bounds(case, mode)
        print(case.name, defect, mode, "logits", f"{dl:.1e} / {bl:.1e}", "worst gradient", f"{dgw:.1e} / {bg:.1e}")
        assert dl > 4 * bl or dgw > 4 * bg, (case.name, defect, mode, dl, bl, dgw, bg)
    bl, _, bg = R.bounds(case, torch.bfloat16)
    print(case.name, defect, "bf16", "logits", f"{dl:.1e} / {bl:.1e}", "worst gradient", f"{dgw:.1e} / {bg:.1e}")
    assert (dl > 2 * bl or dgw > 2 * bg) == ((case.name, defect) not in NO_TEETH_BF16), (case.name, defect, dl / bl, dgw / bg)


def test_the_bf16_bound_follows_the_autocast_rule():
    case = R.BY_NAME["s16_L77_B2"]
    el, es, eg = R.distance(R.reference_autocast(case), R.reference(case))
    bl, bs, bg = R.bounds(case, torch.bfloat16)
    assert (bl, bg) == (min(5e-2, 2 * el), min(1.5e-1, 2 * R.worst(eg)[1])) and 2 * es <= bs == min(2e-3, 2 * R.loss_gap(True))
    assert 1e-3 < el < 5e-2                  # autocast really ran in bf16
    assert R.bounds(case, "bf16x3") == (1e-3, 1e-4, 2e-3) and R.bounds(case, "f16") == (2e-3, 1e-4, 6e-3)


def test_no_teeth_entries_name_real_pairs():
    assert set(NO_TEETH_BF16) <= {(c.name, d) for c, d in PAIRS}
