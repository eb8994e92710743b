"""tests/attention_x3_dropout_cpu.py on its own, without a GPU: the mask contract with global q0 / k0, the models of the DROP kernels of
csrc/attention3.hip against float64 with the same mask at their E_REF tables, and the seeded defects - each must FAIL the check the GPU
test applies (attention_cpu.check_random at 4 * E_REF), the clean model must pass it."""
import pytest
import torch

import attention_cpu as A
import attention_dropout_cpu as D
import attention_x3_dropout_cpu as X
import philox_cpu as PH


def test_tables_are_what_the_models_measure():
    """E_REF_X3_DROP / E_REF_H16_DROP are the figures `python tests/attention_x3_dropout_cpu.py` prints (here: over the shapes that hold a
    worst case, printed per length class)"""
    worst, where = X.measure_e_ref()
    for mode, name in (("x3", "E_REF_X3_DROP"), ("h16", "E_REF_H16_DROP")):
        for n in A.KINDS:
            print(name, n, " ".join(f"{v:.3e}" for v in worst[mode][n]), "at", [where.get((mode, n, i)) for i in range(3)])
            for w, e in zip(worst[mode][n], X.TABLES[mode][n]):
                assert w <= e * 1.001 + 1e-12 and w >= e * 0.5, (mode, n, w, e)      # (libm differences move the last digits, not the class)


@pytest.mark.parametrize("Sq,Skv", [(256, 77), (512, 77), (512, 512), (256, 768)])
def test_launch_masks_with_global_q0_k0_assemble_the_full_sequence_mask(Sq, Skv):
    """what each one-tile launch draws from (ld_mask, q0, k0, sq_total) is its slice of the materialised route's [B * nh, Sq, round_up(Skv, 8)]
    mask (philox_cpu.dropout_keep over the whole tensor)"""
    p, off = X.DROPS[1]
    ld = D.row_pitch(Skv)
    full = torch.from_numpy(PH.dropout_keep(X.B * X.NH * Sq * ld, p, X.SEED, off).reshape(X.B, X.NH, Sq, ld)[..., :Skv].copy())
    assert torch.equal(X.keep_mask(Sq, Skv, p, off), full)
    for q0, k0, keys in X.launches(Sq, Skv):
        assert torch.equal(X.launch_mask(Sq, Skv, p, off, q0, k0, keys), full[:, :, q0:q0 + 256, k0:k0 + keys]), (q0, k0)
    if Sq > 256:
        assert not torch.equal(X.keep_mask(Sq, Skv, p, off, defect="local_q"), full)
    if Skv % 8:
        assert not torch.equal(X.keep_mask(Sq, Skv, p, off, defect="ld_skv"), full)


# the shape at which each defect shows: more than one query block | S_kv no multiple of 8 | any | any
DEFECT_SHAPES = {"local_q": (512, 77), "ld_skv": (256, 77), "no_scale": (256, 96), "lse_dropped": (256, 256)}


@pytest.mark.parametrize("mode", ["x3", "h16"])
@pytest.mark.parametrize("defect", X.DEFECTS)
def test_every_seeded_defect_fails_the_gpu_check(mode, defect):
    Sq, Skv = DEFECT_SHAPES[defect]
    c = X.random_case(Sq, Skv, mode)
    for p, off in X.DROPS:
        keep = X.keep_mask(Sq, Skv, p, off)
        ref = D.reference(c, keep, p)
        e_ref = X.e_ref_for(mode, Sq, Skv)
        A.check_random(c, X.MODELS[mode](c, keep, p), ref, e_ref, tag=f"clean {mode} {Sq}x{Skv} p={p}")
        bad_keep = X.keep_mask(Sq, Skv, p, off, defect=defect) if defect in ("local_q", "ld_skv") else keep
        out = X.MODELS[mode](c, bad_keep, p, defect=defect)
        with pytest.raises(AssertionError):
            A.check_random(c, out, ref, e_ref, tag=f"{defect} {mode} {Sq}x{Skv} p={p}")
        if defect == "lse_dropped":      # ... and the lse alone gives it away
            with pytest.raises(AssertionError):
                A.check_random(c, dict(lse=out["lse"]), ref, e_ref, tag=f"{defect} lse only")
