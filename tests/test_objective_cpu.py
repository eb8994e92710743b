"""CPU: the proof that the assertions of tests/test_gpu_objective_edges.py can fail, and that its references are the right ones.

  * soft-target cross entropy: the float32 torch model of the kernels' documented form passes soft_ce_check at every case with the
    E_REF the GPU file carries, the float64 reference passes, and six classic defects seeded into the model each fail;
  * mask sampling: the stable restatements equal oracle/maskgit_oracle.py on every tie-free case and reproduce the committed goldens
    mask_b64 / mask_small / mask_muse; five defects each fail the checkers on the case lists;
  * conditioning dropout: the kernel's statement equals the oracle bit for bit on every case; two defects each fail.
"""
import os

import numpy as np
import pytest
import torch

import objective_cpu as C
import test_gpu_objective_edges as G
from oracle import maskgit_oracle as O


def failing(cases, run):
    """names of the cases whose check raises"""
    bad = []
    for c in cases:
        try:
            run(c)
        except AssertionError:
            bad.append(c["name"])
    return bad


# ---- soft-target cross entropy --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soft_cases():
    cases = C.soft_ce_all_cases()
    return cases, [C.soft_ce_reference(c) for c in cases]


def test_soft_ce_case_lists_reach_what_they_claim(soft_cases):
    cases, refs = soft_cases
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    assert {C.soft_ce_branch(c) for c in cases} == {"K1024 vector", "K1024 scalar", "K512 vector", "K256 vector", "generic"}
    by = {c["name"]: c for c in cases}
    assert C.soft_ce_branch(by["K512-odd-ld"]) == "generic" and C.soft_ce_branch(by["K256-odd-ld"]) == "generic"
    assert C.soft_ce_branch(by["K1024-base-off-1"]) == "K1024 scalar" and C.soft_ce_branch(by["K1024-odd-ld"]) == "K1024 scalar"
    assert C.soft_ce_branch(by["K1024-bf16-out-8B"]) == "K1024 vector" and C.soft_ce_branch(by["K1024-bf16-out-2B"]) == "K1024 scalar"
    assert C.soft_ce_branch(by["K256-f32-out-4B"]) == "generic" and C.soft_ce_branch(by["K256-ldo+260"]) == "K256 vector"
    assert sorted({c["B"] * c["S1"] for c in cases}) == [2, 5, 9, 15, 65, 1023, 1024, 1025, 1285]
    assert all(float(c["x"].abs().max()) <= 32.0 for c in cases)
    c = by["K256-aligned"]                     # 60 soft rows: every soft kind under every logit kind, among the active rows too
    lab = c["labels"].view(c["B"], c["S1"])
    assert bool((lab[1::2, 0] != -100).all()) and bool((lab[1, 1:] == -100).all()) and int((lab[2, 1:] != -100).sum()) == 1
    ps = c["soft"].sum(-1)
    for want in (1.0, 0.5, 2.0, 0.0):
        assert bool(((ps - want).abs() < 1e-5).any())
    assert all(r["n"] > 0 for c, r in zip(cases, refs) if not c["name"].startswith("none-active"))
    assert all(r["n"] == 0 for c, r in zip(cases, refs) if c["name"].startswith("none-active"))


def test_soft_ce_e_ref_is_what_the_gpu_file_carries(soft_cases):
    """E_REF is a measurement of torch's float32 kernels; another CPU may sum in another order, so the committed figures are held to a
    factor of two of what this machine measures"""
    cases, _ = soft_cases
    E = C.measure_soft_ce_e_ref(cases)
    assert set(E) == set(G.E_REF)
    for k, v in E.items():
        assert 0.5 * G.E_REF[k] <= v <= 2.0 * G.E_REF[k], (k, v, G.E_REF[k])


def test_soft_ce_model_and_reference_pass_every_check(soft_cases):
    cases, refs = soft_cases
    for c, ref in zip(cases, refs):
        C.soft_ce_check(c, C.soft_ce_model(c), G.E_REF, ref)
        rows = c["B"] * c["S1"]
        dl = torch.zeros(rows, c["ldo"], dtype=torch.float64)
        dl[:, :c["K"]] = ref["grad"]
        exact = dict(loss_out=torch.tensor([ref["loss"], float(ref["n"])]), lse=ref["lse"], psum=ref["psum"], row_loss=ref["row_loss"],
                     dl=dl.to(c["out"]))
        C.soft_ce_check(c, exact, G.E_REF, ref)


@pytest.mark.parametrize("fault", C.SOFT_CE_FAULTS)
def test_soft_ce_seeded_defect_fails(soft_cases, fault):
    cases, refs = soft_cases
    ref_of = {c["name"]: r for c, r in zip(cases, refs)}
    bad = failing(cases, lambda c: C.soft_ce_check(c, C.soft_ce_model(c, fault), G.E_REF, ref_of[c["name"]]))
    print(f"{fault}: {len(bad)} of {len(cases)} cases fail")
    assert bad, f"no case notices {fault}"
    if fault == "tail_unwritten":            # exactly the cases that have a tail
        assert set(bad) == {c["name"] for c in cases if c["ldo"] > c["K"]}


# ---- mask sampling ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample_cases():
    return C.mask_sample_cases()


@pytest.fixture(scope="module")
def token_cases():
    return C.mask_tokens_cases() + C.rect_cases()


def test_seeded_timesteps_keep_their_margin(sample_cases, token_cases):
    """S * p of every seeded image is at least 1e-3 from a half-integer in f32 and in float64: no case's count hangs on a cosine's ulp"""
    assert all(C.margin_ok(c) for c in sample_cases + token_cases)
    for S in (255, 256, 257, 1023, 1024):
        assert float(C.half_margin(S, torch.rand(64, generator=C.gen(0)), 0.0).min()) >= 6.5e-3


def test_restatements_equal_the_oracle_and_pass_their_checks(sample_cases, token_cases):
    """mask_sample_check / mask_tokens_check compare with the oracle itself wherever the noise has no ties"""
    assert sum(not c["ties"] for c in sample_cases) >= 25 and sum(not c["ties"] for c in token_cases) >= 40
    for c in sample_cases:
        if not c["ties"]:
            assert all(len(torch.unique(row)) == row.numel() for row in c["noise"]), c["name"]
        C.mask_sample_check(c, C.mask_sample_ref(*C.mask_sample_args(c)))
    for c in token_cases:
        C.mask_tokens_check(c, C.mask_tokens_ref(c["tokens"], c["mask_id"], **c["kw"]))


def test_half_even_cases_are_exact_halves(sample_cases, token_cases):
    for c in sample_cases:
        if "half-even" in c["name"]:
            S = c["tokens"].shape[1]
            x = S * O.cosine_schedule(c["timesteps"]).clip(c["min_rate"])
            assert bool((x == S * 0.25).all()) and float(x[0]) % 1.0 == 0.5
    n = 0
    for c in token_cases:
        if "half-even" in c["name"]:
            x = c["tokens"].shape[1] * c["kw"]["mask_prob"]
            assert x.tolist() == [0.5, 1.5, 2.5, 3.5]
            n += 1
    assert n == 8          # S = 4, 256, 1024, 4096, random and all-equal noise


@pytest.mark.parametrize("name", ["mask_b64", "mask_small"])
def test_mask_sample_restatement_reproduces_the_golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    t = lambda k: torch.from_numpy(g[k])   # noqa: E731
    got = C.mask_sample_ref(t("image_tokens"), t("class_ids"), t("timesteps"), t("noise"), int(g["mask_id"]), int(g["codebook_size"]),
                            float(g["min_rate"]))
    assert np.array_equal(got[0].numpy(), g["input_ids"]) and np.array_equal(got[1].numpy(), g["labels"])
    np.testing.assert_array_equal(got[2].numpy(), g["mask_prob"])


@pytest.mark.parametrize("case", ["default", "predict_all", "random_replace", "region", "eval_ratios"])
def test_mask_tokens_restatement_reproduces_the_golden(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "mask_muse.npz"))
    t = lambda k: torch.from_numpy(g[k])   # noqa: E731
    kw = dict(all_labels=case in ("predict_all", "random_replace"))
    if case == "region":
        kw.update(timesteps=t(case + ".timesteps"), rects=t("region.rects"))
    elif case == "eval_ratios":
        kw.update(mask_prob=t(case + ".mask_prob"), noise=t(case + ".noise"))
    else:
        kw.update(timesteps=t(case + ".timesteps"), noise=t(case + ".noise"))
    ids, labels, lw, mp = C.mask_tokens_ref(t("tokens"), int(g["mask_id"]), float(g[case + ".min_rate"]), **kw)
    assert np.array_equal(ids.numpy(), g[case + ".input_ids"]) and np.array_equal(labels.numpy(), g[case + ".labels"])
    np.testing.assert_array_equal(mp.numpy(), g[case + ".mask_prob"])
    if kw["all_labels"]:
        np.testing.assert_array_equal(lw.numpy(), g[case + ".loss_weight"])
    else:
        assert lw is None


@pytest.mark.parametrize("fault", C.MASK_FAULTS)
def test_mask_seeded_defect_fails(sample_cases, token_cases, fault):
    bad_t = failing(token_cases, lambda c: C.mask_tokens_check(c, C.mask_tokens_ref(c["tokens"], c["mask_id"], fault=fault, **c["kw"])))
    print(f"{fault}: mask_tokens {len(bad_t)} of {len(token_cases)} cases fail")
    assert bad_t, f"no mask_tokens case notices {fault}"
    if fault == "eval_clipped":
        assert all("eval-not-clipped" in n for n in bad_t)
        return                                 # mask_sample has no eval branch
    bad_s = failing(sample_cases, lambda c: C.mask_sample_check(c, C.mask_sample_ref(*C.mask_sample_args(c), fault=fault)))
    print(f"{fault}: mask_sample {len(bad_s)} of {len(sample_cases)} cases fail")
    assert bad_s, f"no mask_sample case notices {fault}"
    if fault == "round_half_up":
        assert all("half-even" in n for n in bad_s + bad_t)
    if fault == "no_clamp":                    # only where round(S * p) = 0
        assert all("clamp" in n or "half-even" in n or "S1-" in n or n == "S4-eval-not-clipped" for n in bad_s + bad_t)
    if fault == "reverse_ties":
        assert all("ties" in n or "equal" in n for n in bad_s + bad_t)


# ---- conditioning dropout ---------------------------------------------------------------------------------------------------------
def test_cond_dropout_statement_equals_the_oracle():
    cases = C.cond_dropout_cases()
    assert max(c["x"].numel() for c in cases) == 524289
    for c in cases:
        C.cond_dropout_check(c, C.cond_dropout_model(c["x"], c["empty"], c["u"], c["p"]))
    c = next(x for x in cases if x["name"] == "per257-B3-p0.625")
    assert (c["u"] < c["p"]).tolist() == [True, True, False]
    got = O.cond_dropout(c["x"], c["empty"], c["u"], c["p"])
    n = len(C.SPECIALS)
    for b in range(3):
        assert all(any(C.bits(c["x"][b, :n])[j] == C.bits(torch.tensor([s]))[0] for j in range(n)) for s in C.SPECIALS)
    assert float(got[0, C.SPECIALS.index(1e-42)]) == float(torch.tensor(1e-42)) != 0.0     # image 0 is kept: its subnormal survives


@pytest.mark.parametrize("fault", C.DROPOUT_FAULTS)
def test_cond_dropout_seeded_defect_fails(fault):
    cases = C.cond_dropout_cases()
    bad = failing(cases, lambda c: C.cond_dropout_check(c, C.cond_dropout_model(c["x"], c["empty"], c["u"], c["p"], fault)))
    print(f"{fault}: {len(bad)} of {len(cases)} cases fail")
    assert bad, f"no case notices {fault}"
