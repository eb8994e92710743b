"""CPU: the checkers of tests/test_gpu_ffn_edges.py bite.  Each one is run on a float32 torch emulation of the kernel it judges on the
GPU (ffn_emulate, ffn_layout_emulate, lnp_emulate, lnp_layout_emulate), which must pass at every case of the GPU tests' lists, and on
seeded wrong versions of that emulation, each of which must fail: were one to pass, the same mistake in a kernel would pass too.  The
committed E_REF constants are re-measured as well."""
import pytest
import torch

import test_gpu_ffn_edges as E
from test_gpu_row_edges import BF, F32

ALL_FFN = [(E.FFN_GENERIC_CASES, c) for c in E.FFN_GENERIC_CASES] + [(E.FFN_WIDE_CASES, c) for c in E.FFN_WIDE_CASES]


def ffn_c(cases, case):
    return E.ffn_case(*case, E.ffn_seed(cases, case))


def fails(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_e_ref_constants_are_the_measured_ones():
    for k, v in E.measure_e_ref().items():
        assert float(f"{v:.3e}") == E.E_REF[k], (k, v, E.E_REF[k])
    assert all(E.R.E_REF[k] == v for k, v in E.E_REF.items())


@pytest.mark.parametrize("t", [F32, BF], ids=["f32", "bf16"])
def test_ffn_mid_emulation_passes_every_case(t):
    for cases, case in ALL_FFN:
        if case[2] == t:
            c = ffn_c(cases, case)
            E.ffn_check(c, E.ffn_emulate(c))


@pytest.mark.parametrize("t", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("inter", [1020, 1028, 2044, 3076, 4092])
def test_ffn_mid_wrong_divisor_fails(inter, t):
    """mean and variance over the width rounded up to a multiple of 1024 (what a kernel templated on NV * 1024 columns would do), at
    every row count of that width - the 0.4 % of 1020 / 1024 and of 4092 / 4096 included"""
    for cases, case in ALL_FFN:
        if case[1:] == (inter, t):
            c = ffn_c(cases, case)
            if bool((c["b"].float() == 0).all()):
                continue                                                        # the lone h = 0 row: 0 / n is 0 for every n
            fails(E.ffn_check, c, E.ffn_emulate(c, "divisor"))


def test_ffn_mid_bf16_layernorm_of_the_unrounded_h_fails():
    """bf16: LayerNorm must read the stored, rounded h.  Every case with a row of ordinary values shows it (an h = 0 row or one whose h
    is a itself, 996 / 1000 / 1004, rounds to itself and cannot)"""
    n = 0
    for cases, case in ALL_FFN:
        if case[2] != BF:
            continue
        c = ffn_c(cases, case)
        e = E.ffn_emulate(c, "unrounded")
        if case[0] == 1 and E.same_bits(e["hm"], E.ffn_emulate(c)["hm"]):
            continue
        fails(E.ffn_check, c, e)
        n += 1
    assert n >= sum(1 for _, case in ALL_FFN if case[2] == BF and case[0] > 1)  # every case of more than one row, at the least


LAYOUT_FFN = [(r, i, t) for (r, i, t) in E.FFN_LAYOUT_GENERIC] + [(r, i, BF) for i in E.FFN_WIDE_INTER for r in E.FFN_WIDE_ROWS]


@pytest.mark.parametrize("mutant", [None, "next_block", "dead_row"])
def test_ffn_mid_layout_checker(mutant):
    """partial row i holding the rows of block i + 1, and a dead row of the ragged last block written with the last live row's result"""
    for rows, inter, t in LAYOUT_FFN:
        c = E.ffn_layout_case(rows, inter, t, 3100 + rows + inter)
        got = E.ffn_layout_emulate(c, mutant)
        if mutant is None:
            E.ffn_layout_check(c, got)
        elif mutant == "next_block" and rows <= E.FFN_BLOCK:
            continue                                                            # one block: nothing to swap
        else:
            fails(E.ffn_layout_check, c, got)


def test_ln_pair_emulation_passes_every_case():
    for case in E.LNP_CASES:
        c = E.lnp_case(*case, E.lnp_seed(case))
        E.lnp_check(c, E.lnp_emulate(c))


def test_ln_pair_dres_before_the_layernorm_backward_fails():
    for case in E.LNP_CASES:
        if case[2]:
            c = E.lnp_case(*case, E.lnp_seed(case))
            fails(E.lnp_check, c, E.lnp_emulate(c, "dres_first"))


@pytest.mark.parametrize("mutant", [None, "next_block", "dead_row"])
def test_ln_pair_layout_checker(mutant):
    for rows, cols in E.LNP_LAYOUT:
        c = E.lnp_layout_case(rows, cols, 5500 + rows + cols)
        got = E.lnp_layout_emulate(c, mutant)
        if mutant is None:
            E.lnp_layout_check(c, got)
        else:
            fails(E.lnp_layout_check, c, got)


def test_a_written_buffer_fails_the_refusal_check():
    c = E.ffn_case(3, 4100, BF, 1)
    bufs = E.ffn_buffers(c)
    E.all_untouched(bufs)
    for k in bufs:
        b = {n: v.clone() for n, v in bufs.items()}
        b[k].view(-1)[-1] = 0.0
        fails(E.all_untouched, b)
