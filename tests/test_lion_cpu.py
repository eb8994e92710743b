"""CPU: the exact model of the Lion kernels (tests/lion_cpu.py) reproduces the reference class's recorded steps bit for bit
(tests/golden/lion_steps.npz), the case list the GPU module walks (tests/test_gpu_lion.py) sees every seeded defect of lion_cpu.DEFECTS, and
the host side of muse.FusedLion - argument checks, group segments, the reference's state-dict layout - works without a GPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import lion_cpu as L
import optim_cpu as O
import weights as W

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lion_steps.npz")


@functools.lru_cache(maxsize=1)
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["layout"]))


def golden_groups(lay):
    return [dict(lr=g["lr"], betas=tuple(g["betas"]), weight_decay=g["weight_decay"]) for g in lay["param_groups"]]


# ---- (a) the model against the reference class ------------------------------------------------------------------------------------------------
def test_model_reproduces_the_reference_class_bit_for_bit():
    g, lay = golden()
    H = L.fill_groups(golden_groups(lay))
    bits = 0
    for t, n in enumerate(lay["sizes"]):
        p, m = g[f"p0_{t}"].copy(), np.zeros(n, F)
        for s in range(1, lay["steps"] + 1):
            p, m = L.update1(p, g[f"g{s}_{t}"], m, H[lay["group_of"][t]], 1.0)
            assert p.tobytes() == g[f"p{s}_{t}"].tobytes(), (t, s, int((p.view(np.uint32) != g[f"p{s}_{t}"].view(np.uint32)).sum()))
            assert m.tobytes() == g[f"m{s}_{t}"].tobytes(), (t, s, int((m.view(np.uint32) != g[f"m{s}_{t}"].view(np.uint32)).sum()))
            bits += 64 * n
    assert bits == 64 * 6 * (1 + 8 + 1003 + 4097)


def test_golden_holds_its_plants():
    g, lay = golden()
    H = L.fill_groups(golden_groups(lay))
    assert lay["sizes"] == [1, 8, 1003, 4097] and lay["steps"] == 6 and len(lay["param_groups"]) == 2
    assert sorted(gr["weight_decay"] for gr in lay["param_groups"]) == [0.0, 0.1] and lay["param_groups"][0]["lr"] != lay["param_groups"][1]["lr"]
    for t, i in lay["plant_zero"]:
        assert all(g[f"g{s}_{t}"][i] == 0 and g[f"m{s}_{t}"][i] == 0 for s in range(1, 7))
    for t, i in lay["plant_minus_zero"]:
        assert lay["param_groups"][lay["group_of"][t]]["weight_decay"] == 0.0
        assert all(g[f"p{s}_{t}"].view(np.uint32)[i] == 0x80000000 for s in range(7))
    near = 0
    for t, i in lay["plant_cancel"]:
        h = H[lay["group_of"][t]]
        for s in range(2, 7):
            a, b = g[f"m{s - 1}_{t}"][i] * h["b1"], g[f"g{s}_{t}"][i] * h["omb1"]
            assert a * b <= 0 and abs(F(a + b)) <= 4 * np.spacing(abs(a)), (t, i, s, a, b)
            near += 1
    assert near == 30


# ---- (b) every seeded defect is seen by a case of the GPU module's list --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _good(name, regime):
    return L.run(next(c for c in L.CASES if c["name"] == name), regime)


def _differs(a, b, recs):
    """under the comparison the GPU module applies: NaNs a kernel may produce count as one pattern"""
    return any(L.canon32(xa).tobytes() != L.canon32(ya).tobytes() or L.canon_images(xi, recs).tobytes() != L.canon_images(yi, recs).tobytes()
               for (xa, xi), (ya, yi) in zip(a, b))


def test_defect_list_is_complete():
    assert len(set(L.DEFECTS)) == len(L.DEFECTS) and set(L.DISPATCH_DEFECTS) <= set(O.DEFECTS)
    for name in ("momentum_not_fused", "update_from_new_m", "reuses_m_b1", "decay_not_rounded", "decay_after_step", "sign_zero_as_plus",
                 "sign_nan_as_zero", "minus_zero_lost", "factor_not_rounded", "v_touched", "image_on_skip"):
        assert name in L.DEFECTS
    assert len({c["name"] for c in L.CASES}) == len(L.CASES)


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_defect_is_caught_by_a_gpu_case(defect):
    caught = [(c["name"], r) for c in L.CASES for r in L.REGIMES if _differs(_good(c["name"], r), L.run(c, r, defect), L.build(c)["recs"])]
    print(defect, "caught by", len(caught), "of", len(L.CASES) * len(L.REGIMES), "runs, e.g.", caught[:3])
    assert caught, defect
    forms = {next(c for c in L.CASES if c["name"] == n)["form"] for n, _ in caught}
    if defect in L.UPDATE_DEFECTS:
        assert forms == {"flat", "flat_groups", "multi"}, (defect, forms)      # the update is seen through every form


def test_model_is_deterministic_and_skip_leaves_everything():
    for c in (L.FLAT_CASES[-1], L.GROUP_CASES[2], L.MULTI_CASES[3]):
        b = L.build(c)
        assert not _differs(_good(c["name"], "host_third"), L.run(c, "host_third"), b["recs"])
        for A, I in L.run(c, "skip_set"):
            assert A.tobytes() == b["A"].tobytes() and I.tobytes() == b["I"].tobytes()
        assert not _differs(_good(c["name"], "skip_zero"), _good(c["name"], "host_third"), b["recs"])
        assert _differs(_good(c["name"], "dev_third"), [(b["A"], b["I"])] * L.STEPS, b["recs"])


def test_lion_rule_is_put_back():
    before = (O.adam_hyper, O.fill_groups, O.update1)
    L.run(L.FLAT_CASES[0], "host_half")
    with pytest.raises(ZeroDivisionError):
        with L.lion_rule():
            1 / 0
    assert (O.adam_hyper, O.fill_groups, O.update1) == before
    case = next(c for c in O.FLAT_CASES if c["name"] == "flat-n5-none-host1.0")
    assert O.run_flat(case)[0][0].tobytes() == O.run_flat(case)[0][0].tobytes()


def test_cases_cover_what_the_gpu_module_promises():
    assert {c["n"] for c in L.FLAT_CASES} == set(L.SIZES) == {1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3}
    assert any(len(c["ranges"]) == 3 for c in L.FLAT_CASES) and {c["image"] for c in L.FLAT_CASES} == {False, True}
    whole = next(c for c in L.GROUP_CASES if c["name"] == "groups-whole")
    assert len(set(whole["seg_group"])) == 3 and any(e % 4 and e % 4096 for e in whole["seg_end"][:-1])
    assert any(b for c in L.GROUP_CASES for b, _ in c["slices"])
    for ncol in (6, 7):
        cs = [c for c in L.MULTI_CASES if c["ncol"] == ncol]
        assert {c["v"] for c in cs} == {"region", "null"}
        built = L.build(cs[0])
        assert any(r["p"] % 4 for r in built["recs"]) and any(r["n"] % 4096 for r in built["recs"])
    kinds = {(r["img"] is None, getattr(r["img"], "half", None), getattr(r["img"], "plo", 0) % 4 == 0 if r["img"] is not None and r["img"].plo else None)
             for c in L.MULTI_CASES if c["ncol"] == 7 for r in L.build(c)["recs"]}
    assert len(kinds) == 5, kinds                                              # none, bf16, planes % 4 == 0, planes % 4 != 0, half
    p, g, m, v = L.values(4097, 1)
    assert np.isnan(g).any() and np.isinf(g).any() and np.isinf(p).any() and np.isinf(m).any()
    tiny = np.finfo(F).tiny
    assert all(((x != 0) & (np.abs(x) < tiny)).any() for x in (p, g, m)) and (p.view(np.uint32) == 0x80000000).any()
    assert (v.view(np.uint32) == O.SENT32).all()


# ---- (c) muse.FusedLion's host side -----------------------------------------------------------------------------------------------------------
def test_fused_lion_argument_checks_and_defaults():
    import muse
    w = [torch.nn.Parameter(torch.zeros(3))]
    opt = muse.FusedLion(w)
    assert opt.defaults == dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0) and opt.max_grad_norm is None
    assert muse.FusedLion(w, lr=1e-3, eps=1e-8, foreach=None, anything=3).param_groups[0]["lr"] == 1e-3      # **kwargs accepted and ignored
    assert muse.FusedLion(w, max_grad_norm=0.5).max_grad_norm == 0.5
    for kw, msg in ((dict(lr=-1e-4), "Invalid learning rate: -0.0001"), (dict(betas=(1.0, 0.99)), "Invalid beta parameter at index 0: 1.0"),
                    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1")):
        with pytest.raises(ValueError, match=msg):
            muse.FusedLion(w, **kw)
    with pytest.raises(muse._hip.MuseHipError, match="FusedLion: at most 8 parameter groups"):
        muse.FusedLion([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(9)])
    assert not isinstance(opt, muse.FusedAdamW) and type(opt).__mro__[1] is type(muse.FusedAdamW(w)).__mro__[1]
    assert opt.step() is None                                                   # no gradient yet: nothing to do, nothing launched


def test_fused_lion_flat_host_logic_state_dict_and_round_trip(monkeypatch):
    """the flat engine without a GPU: the segment table, range-wise application, the state dict in the golden's layout and a round trip;
    ops.lion_flat_groups is replaced by the numpy model per segment"""
    import muse
    from muse import ops
    _, lay = golden()
    calls = []

    def groups_cpu(p, g, m, p_bf16, base, seg_end, seg_group, groups, grad_scale=1.0):
        assert p_bf16 is None and grad_scale == 1.0
        calls.append((base, base + p.numel()))
        lo = 0
        for e, k in zip(seg_end.tolist(), seg_group.tolist()):
            a, b = max(lo, base), min(e, base + p.numel())
            if a < b:
                sl = slice(a - base, b - base)
                h = L.lion_hyper(groups[k]["lr"], *groups[k]["betas"], groups[k]["weight_decay"])
                p1, m1 = L.update1(p[sl].numpy(), g[sl].numpy(), m[sl].numpy(), h, grad_scale)
                p[sl], m[sl] = torch.from_numpy(p1), torch.from_numpy(m1)
            lo = e
    monkeypatch.setattr(ops, "lion_flat_groups", groups_cpu)
    monkeypatch.setattr(ops, "lion_flat", lambda *a, **k: (_ for _ in ()).throw(AssertionError("single-set kernel on a grouped optimizer")))
    torch.manual_seed(5)
    model = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    model.set_compute_dtype(torch.float32)
    groups = muse.grouped_parameters(model, 0.1)
    with pytest.raises(muse._hip.MuseHipError, match="FusedLion steps the model's whole flat parameter buffer"):
        muse.FusedLion(groups[0]["params"])
    opt = muse.FusedLion(groups, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.1)
    seg_end, seg_group = opt._segments(model)
    assert int(seg_end[-1]) == model.flat_params().numel() and bool((seg_end[1:] > seg_end[:-1]).all()) and bool((seg_group[1:] != seg_group[:-1]).all())
    gid_of = {id(p): k for k, g in enumerate(groups) for p in g["params"]}
    for p, o in zip(model._param_order(), model._offsets):
        s = int((seg_end > o).nonzero()[0])
        assert int(seg_group[s]) == gid_of[id(p)] and o + p.numel() <= int(seg_end[s])
    assert opt.state_dict()["state"] == {}
    names = {id(p): n for n, p in model.named_parameters()}
    twins = {n: p.detach().numpy().copy() for n, p in model.named_parameters()}
    moms = {n: np.zeros_like(v) for n, v in twins.items()}
    n = model.flat_params().numel()
    for step in range(3):
        model.flat_grads().copy_(torch.sin(torch.arange(n, dtype=torch.float32) * 0.01 * (step + 1)))
        for p, gv in zip(model._param_order(), model._grad_views):
            p.grad = gv
            h = L.lion_hyper(1e-2, 0.9, 0.99, groups[gid_of[id(p)]]["weight_decay"])
            k = names[id(p)]
            p1, m1 = L.update1(twins[k].ravel(), gv.numpy().ravel(), moms[k].ravel(), h, 1.0)
            twins[k], moms[k] = p1.reshape(twins[k].shape), m1.reshape(moms[k].shape)
        if step == 1:     # range-wise, as backward reports: the tail first, step() covers the rest
            opt._ensure_flat_state(model.flat_params())
            opt._ranges_done_live = (opt._step + 1, [])
            cut = model._offsets[len(model._offsets) // 2] + 8
            opt._apply(model, cut, n, None)
            opt._ranges_done_live[1].append((cut, n))
            opt._ranges_done, opt._ranges_done_live = opt._ranges_done_live, None
        opt.step()
    assert (0, n) in calls and any(b > 0 for b, _ in calls) and opt._v is None
    for k, p in model.named_parameters():
        assert p.detach().numpy().tobytes() == twins[k].tobytes(), k
    sd = opt.state_dict()
    ps = [p for g in groups for p in g["params"]]
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(len(ps)))
    assert {tuple(sorted(st)) for st in sd["state"].values()} == {tuple(ks) for ks in lay["state_keys"].values()} == {("exp_avg",)}
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in lay["param_groups"]]       # lr, betas, weight_decay, params
    assert [g["params"] for g in sd["param_groups"]] == [list(range(len(groups[0]["params"]))), list(range(len(groups[0]["params"]), len(ps)))]
    for i, p in enumerate(ps):
        assert sd["state"][i]["exp_avg"].numpy().tobytes() == moms[names[id(p)]].tobytes() and sd["state"][i]["exp_avg"].shape == p.shape
    opt2 = muse.FusedLion(muse.grouped_parameters(model, 0.1), lr=5.0)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["lr"] == 1e-2 and opt2._m.shape == opt._m.shape and opt2._v is None      # (alignment padding carries no state)
    sd2 = opt2.state_dict()
    assert all(torch.equal(sd2["state"][i]["exp_avg"], sd["state"][i]["exp_avg"]) for i in sd["state"])
    with pytest.raises(muse._hip.MuseHipError, match="FusedLion.load_state_dict expects"):
        opt2.load_state_dict({"state": {}})
    with pytest.raises(ValueError, match="FusedLion.load_state_dict: exp_avg of parameter 0 has shape"):
        opt2.load_state_dict({"state": {i: {"exp_avg": torch.zeros(1, 1, 1)} for i in sd["state"]}, "param_groups": sd["param_groups"]})


def test_fused_lion_checkpoints_go_both_ways_with_a_torch_optimizer_of_the_same_layout():
    """per-tensor mode: a checkpoint in the reference class's layout ({'exp_avg'} per parameter, groups of lr / betas / weight_decay) loads,
    and FusedLion's own state_dict() loads into a torch.optim.Optimizer with the reference class's defaults (its load_state_dict is the
    base class's)"""
    import muse
    g, lay = golden()
    sizes, order = lay["sizes"], lay["order"]
    params = [torch.nn.Parameter(torch.from_numpy(g[f"p6_{t}"].copy())) for t in range(len(sizes))]
    by_group = [[params[t] for t in order if lay["group_of"][t] == k] for k in range(2)]
    opt = muse.FusedLion([dict(params=by_group[k]) for k in range(2)])
    ref_sd = {"state": {i: {"exp_avg": torch.from_numpy(g[f"m6_{t}"].copy())} for i, t in enumerate(order)}, "param_groups": lay["param_groups"]}
    opt.load_state_dict(ref_sd)
    assert [gr["lr"] for gr in opt.param_groups] == [gr["lr"] for gr in lay["param_groups"]]
    assert [tuple(gr["betas"]) for gr in opt.param_groups] == [tuple(gr["betas"]) for gr in lay["param_groups"]]
    sd = opt.state_dict()
    assert {str(i): sorted(st) for i, st in sd["state"].items()} == lay["state_keys"]
    for i, t in enumerate(order):
        assert sd["state"][i]["exp_avg"].numpy().tobytes() == g[f"m6_{t}"].tobytes()

    class SameLayout(torch.optim.Optimizer):
        def __init__(self, params):
            super().__init__(params, dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0))
    other = SameLayout([dict(params=by_group[k]) for k in range(2)])
    other.load_state_dict(sd)
    assert all(torch.equal(other.state[p]["exp_avg"], sd["state"][i]["exp_avg"]) for i, p in enumerate(by_group[0] + by_group[1]))
    assert [gr["weight_decay"] for gr in other.param_groups] == [gr["weight_decay"] for gr in lay["param_groups"]]
