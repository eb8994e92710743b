"""GPU (-m gpu): every attention and norm + AdaLN route of muse.MaskGiTUViT at MODEL level against the float64 oracle, in all four compute
modes.  tests/uvit_routes_cpu.py holds the case table (one case per route of TapeOps._attention / _attention_bwd_x3, ops.attention_x3_*,
_attention_x3_fwd_blocks / _bwd_blocks and _norm_adaln), the references, the distance and the bounds; tests/test_uvit_routes_cpu.py shows on
a CPU that six seeded routing defects land at least 4 times above every f32 / bf16x3 / f16 bound.  profiles/uvit_routes.md has the routes
and the MI355X's figures.

Per (case, mode): one training step - logits, loss and EVERY parameter gradient (whole tensors) within bounds(case, mode) of the float64
reference, all finite, a gradient for every parameter; the no-tape forward under no_grad within the same logits bound; the C entry points
the step called, counted by a recorder around ops.lib, equal to what ROUTES says the (case, mode) takes.  ROUTES is written from reading
tape_ops.py / ops.py, not computed from their gates:

    per attention site   M   materialised (muse_softmax_fwd / _bwd around batched GEMMs)
                         B   csrc/attention.hip's bf16 kernels (muse_attention_fwd_ex / _bwd_ex)
                         T   one tile (muse_attention_x3_fwd / _bwd, one launch each); Tp: the gradients as operand planes only
                         Qn  n query blocks against one key tile: n launches each way, dk / dv folded by muse_sum_parts_strided (n > 1)
                         S   streamed (muse_attention_x3_fwd_stream / _bwd_stream); Sp: the gradients as operand planes only
                         Pnk n x k block pairs + muse_attention_x3_merge; dq / dk / dv folded by muse_sum_parts_strided
    norm + AdaLN         fused (one muse_norm_adaln_* launch per site and direction) or the two-kernel route (none of them)
The model has 2 layers (one self- and one cross-attention each) and 2 conv-stage attention blocks (two attentions over the text each).

A gradient whose exact value is identically zero (s16_L1: a softmax over one key is constant) is measured against the largest gradient of
its enclosing module (uvit_routes_cpu.distance).  Every streamed case of the base widths hands its gradients on as operand planes only;
h1_w64_s32_B1 is there for the stream kernels' f32 gradients + planes form."""
import math

import pytest
import torch

import uvit_routes_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = "x3"          # the bf16x3 and f16 modes share every gate of the attention route
N_LAYERS, N_BLOCKS = 2, 2

# case -> (layer self-attention, layer cross-attention, block attentions) in the bf16x3 / f16 modes, norm + AdaLN fused?
ROUTES = {
    "s16_L77_B2": ("Tp", "T", "T", True),              # (2 x 77 text rows are no multiple of 8: f32 gradients + planes for k | v)
    "s32_L77_B1": ("Sp", "Q4", "Q4", True),
    "s32_L77_B2": ("Sp", "Q4", "Q4", True),
    "s32_L77_B1_pairs": ("P44", "Q4", "Q4", True),
    "s16_L512_B2": ("Tp", "Sp", "Sp", True),
    "s32_L512_B1": ("Sp", "Sp", "Sp", True),
    "s16_L256_B2": ("Tp", "Tp", "Tp", True),
    "s32_L256_B1": ("Sp", "Q4", "Q4", True),
    "s16_L64": ("Tp", "M", "M", True),
    "s16_L96": ("Tp", "Tp", "Tp", True),
    "s16_L97": ("Tp", "M", "M", True),
    "s16_L224": ("Tp", "M", "M", True),
    "s16_L225": ("Tp", "T", "T", True),                # (450 text rows)
    "s16_L1": ("Tp", "M", "M", True),
    "s15_L77_B1": ("M", "M", "M", False),
    "s17_L77_B3": ("M", "M", "M", False),
    "s8_L77_B2": ("M", "M", "M", True),                # (64 tokens: a multiple of 16, the norm + AdaLN kernel takes them)
    "h4_s16": ("M", "M", "M", True),
    "h1_w64_s16": ("T", "T", "T", True),
    "h1_w64_s32_B1": ("S", "Q4", "Q4", True),
    "c96_s16": ("Tp", "T", "M", True),
    "ln_s16": ("Tp", "T", "T", True),
    "noaffine_s16": ("Tp", "T", "T", True),
    "down_s32": ("Tp", "T", "T", True),
    "down_s64": ("Sp", "Q4", "Q4", True),
}
ATTENTION = ["muse_softmax_fwd", "muse_softmax_bwd", "muse_attention_fwd_ex", "muse_attention_bwd_ex", "muse_attention_x3_fwd",
             "muse_attention_x3_bwd", "muse_attention_x3_bwd+planes_only", "muse_attention_x3_fwd_stream", "muse_attention_x3_bwd_stream",
             "muse_attention_x3_bwd_stream+planes_only", "muse_attention_x3_merge", "muse_sum_parts_strided"]
NORM = ["muse_norm_adaln_fwd", "muse_norm_adaln_bwd", "muse_norm_adaln_fwd_x3", "muse_norm_adaln_fwd_x3+planes_only", "muse_norm_adaln_bwd_x3",
        "muse_adaln_fwd_ex"]
TRACKED = ATTENTION + NORM


def _site(route):
    """entry point -> launches of ONE attention site's forward and backward"""
    po = "+planes_only" if route.endswith("p") else ""
    route = route.rstrip("p")
    if route == "M":
        return {"muse_softmax_fwd": 1, "muse_softmax_bwd": 1}
    if route == "B":
        return {"muse_attention_fwd_ex": 1, "muse_attention_bwd_ex": 1}
    if route == "T":
        return {"muse_attention_x3_fwd": 1, "muse_attention_x3_bwd" + po: 1}
    if route == "S":
        return {"muse_attention_x3_fwd_stream": 1, "muse_attention_x3_bwd_stream" + po: 1}
    if route[0] == "Q":
        nq = int(route[1:])
        return {"muse_attention_x3_fwd": nq, "muse_attention_x3_bwd": nq, "muse_sum_parts_strided": 2 if nq > 1 else 0}
    nq, nk = int(route[1]), int(route[2])
    assert route[0] == "P" and nk > 1
    return {"muse_attention_x3_fwd": nq * nk, "muse_attention_x3_merge": 1, "muse_attention_x3_bwd": nq * nk,
            "muse_sum_parts_strided": 1 + (2 if nq > 1 else 0)}


def expected(case, mode):
    """{tracked entry point: launches in one training step} of a (case, mode)"""
    self_, cross, block, fused = ROUTES[case.name]
    family = X3 if mode in ("bf16x3", "f16") else mode
    if family == torch.float32:
        self_ = cross = block = "M"
    elif family == torch.bfloat16:
        self_ = cross = block = "B"
    n = dict.fromkeys(TRACKED, 0)
    for route, sites in ((self_, N_LAYERS), (cross, N_LAYERS), (block, 2 * N_BLOCKS)):
        for k, v in _site(route).items():
            n[k] += v * sites
    n["muse_adaln_fwd_ex"] = N_BLOCKS + (0 if fused else 3 * N_LAYERS)         # the res blocks' AdaLN, + the layers' on the two-kernel route
    if fused:
        cfg, rows = R.config(case), case.B * R.inner_tokens(case)
        if family == X3:
            # m1 / m2 / m3 as operand planes only where the weight GEMMs take them (>= 128 wide, whole 16-byte rows)
            po = cfg["hidden_size"] >= 128 and rows >= 128 and rows % 8 == 0
            n["muse_norm_adaln_fwd_x3" + ("+planes_only" if po else "")] = 3 * N_LAYERS
            n["muse_norm_adaln_bwd_x3"] = 3 * N_LAYERS
        else:
            n["muse_norm_adaln_fwd"] = n["muse_norm_adaln_bwd"] = 3 * N_LAYERS
    return n


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """a launch that faulted leaves the device unusable for the rest of the process: end the session there rather than start more work"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU error after a U-ViT route test, stopping: {e}", returncode=3)


class _Recorder:
    """stands in for the loaded library: counts every entry point called; the attention backward and the fused norm + AdaLN forward are
    tagged +planes_only when their f32 result pointer is NULL (the gradients / m exist as GEMM operand planes only)"""
    F32_RESULT = {"muse_attention_x3_bwd": 5, "muse_attention_x3_bwd_stream": 6, "muse_norm_adaln_fwd_x3": 5}

    def __init__(self, real):
        self.real, self.n = real, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        at = self.F32_RESULT.get(name)

        def call(*a):
            key = name + ("+planes_only" if at is not None and a[at] is None else "")
            self.n[key] = self.n.get(key, 0) + 1
            return fn(*a)
        return call


def recorded(fn):
    from muse import ops
    rec, inner = _Recorder(ops.lib()), ops.lib
    ops.lib = lambda: rec
    try:
        out = fn()
    finally:
        ops.lib = inner
    return out, rec.n


_MODELS = {}
SEEN = {}           # (case name, mode) -> recorded counts of the tests that ran in this session


def _model(case, mode):
    """one model per configuration, reused across cases and modes (set_compute_dtype drops every cached weight copy)"""
    import muse
    if case.over not in _MODELS:
        model = muse.MaskGiTUViT(**R.config(case))
        model.load_state_dict(R.state_dict(case), strict=True)
        _MODELS[case.over] = model.to(DEV).train()
    return _MODELS[case.over].set_compute_dtype(mode)


def _apply(case, monkeypatch):
    from muse import ops
    for name, value in case.attrs:
        assert hasattr(ops, name)
        monkeypatch.setattr(ops, name, value)


def _step(model, inp):
    ids, enc, cond, micro, labels = inp
    model.mark_weights_changed()                 # (every step starts without cached weight copies: the same casts)
    model.zero_grad(set_to_none=True)
    logits, loss = model(ids, enc, cond, micro, labels=labels)
    loss.backward()
    torch.cuda.synchronize()
    missing = [k for k, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    return logits.detach(), float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("mode", R.MODES, ids=str)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_uvit_route_vs_float64_oracle(case, mode, monkeypatch):
    _apply(case, monkeypatch)
    model = _model(case, mode)
    inp = tuple(t.to(DEV) for t in R.inputs(case))
    (logits, loss, grads), names = recorded(lambda: _step(model, inp))
    with torch.no_grad():
        plain = model(*inp[:4])
    assert torch.isfinite(logits).all() and math.isfinite(loss) and torch.isfinite(plain).all()
    assert all(torch.isfinite(g).all() for g in grads.values())
    ref = R.reference(case)
    el, es, eg = R.distance((logits, loss, grads), ref)
    ei = R.distance((plain, loss, grads), ref)[0]
    bl, bs, bg = R.bounds(case, mode)
    k, e = R.worst(eg)
    line = f"{case.name} {mode}: logits {el:.2e} / {bl:.2e}  no-tape logits {ei:.2e}  loss {es:.1e} / {bs:.1e}  worst gradient {e:.2e} / {bg:.2e} ({k})"
    if mode == torch.float32:
        line += f"  | x the oracle's f32 gap: logits {el * R.M_F32 / bl:.1f} loss {es * R.M_F32 / bs:.1f} gradient {e * R.M_F32 / bg:.1f}"
    print(line)
    got = {k: names.get(k, 0) for k in TRACKED}
    print(case.name, mode, "launches:", {k: v for k, v in got.items() if v})
    SEEN[(case.name, str(mode))] = got
    assert got == expected(case, mode), {k: (got[k], v) for k, v in expected(case, mode).items() if got[k] != v}
    assert names.get("muse_norm_res_fwd", 0) > 0
    assert el < bl, (case.name, mode, el, bl)
    assert ei < bl, (case.name, mode, ei, bl)
    assert es < bs, (case.name, mode, es, bs)
    assert e < bg, (case.name, mode, k, e, bg)




@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("name", ["s32_L77_B1", "s16_L77_B2"])
def test_two_identical_steps_give_identical_bits(name, mode):
    """the cached operand planes and the stream-ordered side work of one step do not leak into the next"""
    case = R.BY_NAME[name]
    model = _model(case, mode)
    inp = tuple(t.to(DEV) for t in R.inputs(case))
    la, sa, ga = _step(model, inp)
    lb, sb, gb = _step(model, inp)
    assert torch.equal(la, lb) and sa == sb
    differ = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not differ, differ


def test_every_route_has_a_case():
    """the union over the table holds every tracked attention, merge and norm + AdaLN entry point, so a later change of a gate cannot leave
    a route without a case unnoticed: the per-case test holds each (case, mode) to its row.  When the whole file has run, the launches the
    device recorded are held to the same union."""
    union = set()
    for case in R.CASES:
        for mode in R.MODES:
            union |= {k for k, v in expected(case, mode).items() if v}
    assert union == set(TRACKED), set(TRACKED) - union
    assert set(ROUTES) == {c.name for c in R.CASES}
    if len(SEEN) == len(R.CASES) * len(R.MODES):
        ran = {k for n in SEEN.values() for k, v in n.items() if v}
        assert ran == set(TRACKED), set(TRACKED) ^ ran
