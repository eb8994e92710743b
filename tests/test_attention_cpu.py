"""CPU: the proof that the assertions of tests/test_gpu_attention_edges.py can fail.  tests/attention_cpu.py's probes are exact on its
contract model at the edge shapes, its float64 reference passes every check the GPU tests apply, and three classic defects seeded into
the model - a dropped last key, a leaked zero pad key, a causal mask off by one in either direction - each fail them."""
import math

import pytest
import torch

import attention_cpu as A
import test_gpu_attention_edges as G

B, NH = G.B, G.NH
EDGES = [(257, 257, 16), (257, 257, 48), (1025, 1025, 16), (256, 77, 64), (50, 7, 64), (385, 289, 32)]       # Sq, Skv, hd
CAUSAL = [(17, 32), (77, 64), (128, 64)]                                                                       # S, hd


def model_out(c, defect=None, kinds=A.KINDS):
    out = A.rounded_outputs(A.contract_model(c, defect))
    return {n: out[n] for n in kinds}


def ref_out(ref, kinds=A.KINDS):
    return {n: (ref[n].float() if n == "lse" else ref[n].to(A.BF)) for n in kinds}


def first_address_case(Sq, Skv, hd):
    return next(iter(G.address_cases(Sq, Skv, hd)))


def test_probe_values_and_maps():
    """every probe value is exact in bf16 (the builders assert it), the scores are exactly -alpha c' (digit distance)^2, and the maps of
    every GPU case select every key, the last key from the first and from the last query tile (address_maps asserts it)"""
    for Sq, Skv, hd in set(G.BF16_SHAPES) | {(sq, skv, 64) for sq in G.X3_SQ for skv in G.X3_SKV}:
        calls = A.address_maps(Sq, Skv, B * NH)
        for maps in calls:
            assert maps.shape == (B * NH, Sq)
            step = (maps[:, 1:] - maps[:, :-1]) % Skv if Sq > 1 else maps[:, :0]
            assert bool((step == step[:, :1]).all()) and all(math.gcd(int(p), Skv) == 1 for p in step[:, :1].flatten())
    c = first_address_case(50, 289, 48)
    q, k = A.to_heads(c["q"], B, 50, NH, 48).double(), A.to_heads(c["k"], B, 289, NH, 48).double()
    s = q @ k.transpose(-1, -2)
    t = c["targets"]
    j = torch.arange(289)
    d2 = sum((x[..., None] - y) ** 2 for x, y in zip(A._digits(t), A._digits(j)))
    assert torch.equal(s, -A.address_scale(c["alpha"]) * d2.double())
    assert c["alpha"] * A.address_scale(c["alpha"]) >= 32 and float(s.amax(-1).abs().max()) == 0.0
    v = A.to_heads(c["v"], B, 289, NH, 48)
    assert bool((v != 0).all()) and bool((v[:, :, 1:] != v[:, :, :-1]).all())


@pytest.mark.parametrize("Sq,Skv,hd", EDGES)
def test_probes_exact_on_contract_model(Sq, Skv, hd):
    for c in G.address_cases(Sq, Skv, hd):
        out = A.contract_model(c)
        ctx_e, dv_e = A.address_expected(c)
        assert torch.equal(out["ctx"], ctx_e) and not bool(out["lse"].any()), "the address probe is not bit-exact on the contract model"
        A.check_address(c, A.rounded_outputs(out))
    c, ref = G.uniform_case(Sq, Skv, hd)
    A.check_uniform(c, model_out(c), ref, G.e_ref_for(Sq, Skv)["uniform_dq"])


@pytest.mark.parametrize("Sq,Skv,hd", EDGES)
def test_reference_passes_every_check(Sq, Skv, hd):
    c = first_address_case(Sq, Skv, hd)
    A.check_address(c, ref_out(A.reference(c)))
    c, ref = G.uniform_case(Sq, Skv, hd)
    A.check_uniform(c, ref_out(ref), ref, G.e_ref_for(Sq, Skv)["uniform_dq"])
    c, ref = G.random_case(Sq, Skv, hd)
    A.check_random(c, ref_out(ref), ref, G.e_ref_for(Sq, Skv))
    A.check_random(c, model_out(c), ref, G.e_ref_for(Sq, Skv))          # and so does the contract model, by a factor of about 4


@pytest.mark.parametrize("defect", ["drop_last", "leak_pad"])
@pytest.mark.parametrize("Sq,Skv,hd", EDGES)
def test_dropped_and_leaked_keys_fail_the_probes(Sq, Skv, hd, defect):
    """forward and backward separately: the context, the log-sum-exp and dV of the address probe each fail on their own, and so does
    the uniform probe's log-sum-exp"""
    c = first_address_case(Sq, Skv, hd)
    out = model_out(c, defect)
    for kind in ("ctx", "lse", "dv"):
        if defect == "drop_last" and kind == "lse":
            continue                                        # (a dropped key leaves the other rows' lse at 0; its own rows move to <= -32)
        with pytest.raises(AssertionError):
            A.check_address(c, {kind: out[kind]})
    ctx_e, _ = A.address_expected(c)
    bad = (out["ctx"].float() != ctx_e).any(-1)
    if defect == "leak_pad":                                # every row halves
        assert bool(bad.all()) and float((out["lse"] - math.log(2)).abs().max()) < 1e-6
    else:                                                   # exactly the rows aimed at the last key
        aimed = (c["targets"] == Skv - 1).permute(0, 2, 1).any(-1).reshape(-1)
        assert torch.equal(bad, aimed) and bool(bad.any())
    c, ref = G.uniform_case(Sq, Skv, hd)
    with pytest.raises(AssertionError):
        A.check_uniform(c, {"lse": model_out(c, defect)["lse"]}, ref, G.e_ref_for(Sq, Skv)["uniform_dq"])


def test_dropped_key_at_1025_fails_the_per_element_bound():
    """S = 1025, head dim 16: the dropped last key passes the old bars on dq (2.6e-2 of max against 3e-2) and on lse; over the terms
    it is 2.1e-2 against a bound of 7.3e-3 on dq"""
    Sq = Skv = 1025
    c, ref = G.random_case(Sq, Skv, 16)
    out = model_out(c, "drop_last")
    for kind in ("ctx", "dq", "dv"):
        with pytest.raises(AssertionError):
            A.check_random(c, {kind: out[kind]}, ref, G.e_ref_for(Sq, Skv))
    e = A.measure(out["dq"], ref["dq"], ref["t_dq"])
    assert e > 2 * 4 * G.e_ref_for(Sq, Skv)["dq"], e


@pytest.mark.parametrize("S,hd", CAUSAL)
def test_causal_mask_off_by_one_fails(S, hd):
    m = A.causal_maps(S)
    seen = torch.stack([m[("diagonal", "first", "tile")[i % 3]] for i in range(B * NH)]).reshape(B, NH, S)
    cs = A.address_probe(B, S, S, NH, hd, seen, causal=True)
    ch = A.address_probe(B, S, S, NH, hd, m["masked"].expand(B, NH, S).contiguous(), causal=True)
    for c in (cs, ch):
        A.check_address(c, model_out(c, None, ("ctx",)))
        A.check_address(c, ref_out(A.reference(c), ("ctx",)))
    with pytest.raises(AssertionError):                     # the diagonal excluded: the queries aimed at it get a neighbour's row
        A.check_address(cs, model_out(cs, "causal_minus", ("ctx",)))
    with pytest.raises(AssertionError):                     # key i + 1 visible: the hidden target answers
        A.check_address(ch, model_out(ch, "causal_plus", ("ctx",)))
    c, ref = G.random_case(S, S, hd, True)
    A.check_random(c, model_out(c, None, ("ctx",)), ref, dict(ctx=G.E_REF["causal_ctx"][0]))
    for defect in ("causal_plus", "causal_minus"):
        with pytest.raises(AssertionError):
            A.check_random(c, model_out(c, defect, ("ctx",)), ref, dict(ctx=G.E_REF["causal_ctx"][0]))


# =====================================================================================================================================
# the H16 and bf16x3 cores of attention3.hip (tests/test_gpu_attention_x3_edges.py): models, probes in half, scale invariance, defects
# =====================================================================================================================================
import test_gpu_attention_x3_edges as X      # noqa: E402

X_EDGES = [(256, 77), (256, 240), (512, 512), (768, 768)]         # Sq, Skv (head dim 64)


def h16_out(c, S=1.0, defect=None, exact_ctx=True):
    return A.model_h16(c, S, defect, A.address_expected(c)[0] if exact_ctx and c.get("probe") == "address" else None)


def test_h16_probe_values_are_exact_in_half():
    """every value of every address probe of the H16 cases survives .half().float(), the largest magnitude is 57600, and every key beside
    the target has p <= e^-32, which is 0 as a half; the uniform probe's k is exact in bf16 and half"""
    top = 0.0
    for Sq, Skv in X.SHAPES:
        for c in G.address_cases(Sq, Skv, 64):
            A.assert_half_exact(q=c["q"], k=c["k"], v=c["v"], do=c["do"], do_scaled=c["do"] * X.S_PROBE[1])
            top = max(top, *(float(c[n].abs().max()) for n in ("q", "k", "v", "do")))
        k = X.uniform_case_h16(Sq, Skv)[0]["k"]
        A.assert_half_exact(k=k)
        A.assert_bf16_exact(k=k)
    assert top == 57600.0
    assert float(torch.tensor(math.exp(-32.0) * (1 + 2.0 ** -20)).half()) == 0.0


@pytest.mark.parametrize("Sq,Skv", X_EDGES)
def test_h16_probes_exact_on_model(Sq, Skv):
    """on the H16 model the address probe gives ctx == v[target], lse == 0 and dv == the scatter-sum bit for bit at S = 1 and S = 2^13, and
    the model passes the checks the GPU applies (one-tile strictness: no ctx_slack)"""
    for c in G.address_cases(Sq, Skv, 64):
        ctx_e, dv_e = A.address_expected(c)
        for S in X.S_PROBE:
            out = h16_out(c, S)
            assert torch.equal(out["ctx"], ctx_e) and torch.equal(out["dv"], dv_e) and not bool(out["lse"].any())
            A.check_address(c, out, bf16_out=False, h16=S)
    c, ref = X.uniform_case_h16(Sq, Skv)
    A.check_uniform(c, A.model_h16(c), ref, X.e_ref_for(X.E_REF_H16, Sq, Skv)["uniform_dq"], bf16_out=False, h16=True)
    A.check_uniform(c, {n: ref[n].float() for n in A.KINDS}, ref, X.e_ref_for(X.E_REF_H16, Sq, Skv)["uniform_dq"], bf16_out=False, h16=True)


@pytest.mark.parametrize("Sq,Skv", X_EDGES)
def test_core3_models_and_reference_pass_the_random_bound(Sq, Skv):
    for mode, model, table in (("h16", A.model_h16, X.E_REF_H16), ("x3", A.model_x3, X.E_REF_X3)):
        c, ref = X.random_case(Sq, Skv, mode)
        A.check_random(c, model(c), ref, X.e_ref_for(table, Sq, Skv))
        A.check_random(c, {n: ref[n].float() for n in A.KINDS}, ref, X.e_ref_for(table, Sq, Skv))


@pytest.mark.parametrize("Sq,Skv", [(256, 77), (512, 512)])
def test_h16_scale_invariance_on_model(Sq, Skv):
    """(dO 2^-20, S = 2^20) == 2^-20 x (dO, S = 1) bit for bit: S dO is the same half, dsum, alpha / S and 1 / S are powers of two"""
    c, _ = X.random_case(Sq, Skv, "h16")
    one = A.model_h16(c, 1.0)
    two = A.model_h16(dict(c, do=c["do"] * 2.0 ** -20), 2.0 ** 20)
    for n in ("ctx", "lse"):
        assert torch.equal(one[n], two[n])
    for n in ("dq", "dk", "dv"):
        assert torch.equal(two[n], one[n] * 2.0 ** -20), n


@pytest.mark.parametrize("defect", ["drop_last", "leak_pad"])
@pytest.mark.parametrize("Sq,Skv", [(256, 77), (256, 240), (768, 768)])
def test_h16_dropped_and_leaked_keys_fail_the_probes(Sq, Skv, defect):
    """the H16 model with a dropped last key / a leaked zero pad key: check_address fails on ctx, on dv and (leak) on lse, each alone, and
    check_uniform fails on lse"""
    c = first_address_case(Sq, Skv, 64)
    out = h16_out(c, 1.0, defect)
    for kind in ("ctx", "lse", "dv"):
        if defect == "drop_last" and kind == "lse":
            continue
        with pytest.raises(AssertionError):
            A.check_address(c, {kind: out[kind]}, bf16_out=False, h16=1.0, ctx_slack=True)         # (even with the streamed form's slack)
    c, ref = X.uniform_case_h16(Sq, Skv)
    with pytest.raises(AssertionError):
        A.check_uniform(c, {"lse": A.model_h16(c, 1.0, defect)["lse"]}, ref, 0.0, bf16_out=False, h16=True)


def test_h16_missing_unscale_fails_the_scaled_address_probe():
    """no 1 / S on dq, dk, dv: invisible at S = 1, at S = 2^13 check_address fails on dv (2^13 x the scatter-sum); the scale-invariance
    identity fails on all three"""
    c = first_address_case(256, 240, 64)
    A.check_address(c, h16_out(c, 1.0, "no_unscale"), bf16_out=False, h16=1.0)
    S = X.S_PROBE[1]
    with pytest.raises(AssertionError):
        A.check_address(c, {"dv": h16_out(c, S, "no_unscale")["dv"]}, bf16_out=False, h16=S)
    c, _ = X.random_case(256, 77, "h16")
    one, two = A.model_h16(c, 1.0, "no_unscale"), A.model_h16(dict(c, do=c["do"] * 2.0 ** -20), 2.0 ** 20, "no_unscale")
    for n in ("dq", "dk", "dv"):
        assert not torch.equal(two[n], one[n] * 2.0 ** -20)


def test_h16_unscaled_dsum_fails_the_scaled_address_probe():
    """S on dO but not on dsum: the target's dS = p (S dP - dsum) is no longer 0 - check_address fails on dq and on dk at S = 2^13 (at S = 1
    the defect is the identity)"""
    c = first_address_case(256, 240, 64)
    S = X.S_PROBE[1]
    out = h16_out(c, S, "dsum_unscaled")
    for kind in ("dq", "dk"):
        with pytest.raises(AssertionError):
            A.check_address(c, {kind: out[kind]}, bf16_out=False, h16=S)
    c, ref = X.random_case(256, 240, "h16")
    assert torch.equal(A.model_h16(c, 1.0, "dsum_unscaled")["dq"], A.model_h16(c, 1.0)["dq"])


@pytest.mark.parametrize("mode", ["h16", "x3"])
def test_skipped_middle_block_of_768_keys_fails(mode):
    """keys 256 .. 511 skipped: the address probe's ctx and dv fail (the queries aimed into the block), and the seeded case fails the
    per-element bound on every result"""
    Sq = Skv = 768
    c = first_address_case(Sq, Skv, 64)
    kw = dict(bf16_out=False, h16=1.0, ctx_slack=True) if mode == "h16" else dict(bf16_out=False)
    model = A.model_h16 if mode == "h16" else A.model_x3
    good, bad = ((model(c, 1.0, d, A.address_expected(c)[0]) if mode == "h16" else model(c, d, A.address_expected(c)[0])) for d in (None, "skip_middle"))
    A.check_address(c, good, **kw)
    for kind in ("ctx", "dv"):
        with pytest.raises(AssertionError):
            A.check_address(c, {kind: bad[kind]}, **kw)
    c, ref = X.random_case(Sq, Skv, mode)
    out = model(c, 1.0, "skip_middle") if mode == "h16" else model(c, "skip_middle")
    for kind in A.KINDS:
        with pytest.raises(AssertionError):
            A.check_random(c, {kind: out[kind]}, ref, X.e_ref_for(X.E_REF_H16 if mode == "h16" else X.E_REF_X3, Sq, Skv))
