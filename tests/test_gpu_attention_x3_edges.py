"""GPU (-m gpu): the two TF32-class attention cores of csrc/attention3.hip - bf16x3 (three bf16 products of hi / lo planes) and H16 (the "f16"
compute mode: one IEEE-half product, gradient operands times the pass's power-of-two scale S) - at every edge of attn3::check, check_stream,
ops.attention_x3_blocked and attention_x3_streamed, B = 2 images x 3 heads, head dim 64, no sequence longer than 768.  The regime is that of
tests/test_gpu_attention_edges.py: exact probes, seeded cases judged per element over the terms with the bound 4 * E_ref (no output
rounding term: the results are f32), poisoned surroundings, and - new here - the operand images the kernels write next to their f32
results (bit for bit the cast / split of the result), half's overflow counter, the merge and sum kernels on their own, and the refusals.
tests/attention_cpu.py holds the models (core3_model: model_h16, model_x3), tests/test_attention_cpu.py seeds their defects.
`python tests/test_gpu_attention_x3_edges.py` prints E_REF_H16 / E_REF_X3 on a CPU.  profiles/attention_edges.md has the MI355X's figures.

The bf16x3 random bound: the documented class is 2^-16 per product (X3_TOL's reasoning: an operand keeps 16 bits, lo * lo is dropped).  ctx
and dv chain two products, dq and dk three (scores -> dS -> gradient), so a result is within about 2 .. 3 x 2^-16 of its terms; E_REF_X3 is that
figure as model_x3 measures it on the very cases (4.8e-6 .. 1.6e-5 = 0.3 .. 1.0 x 2^-16 of the terms), and the GPU bound is 4 x E_REF_X3.  The inputs of the
bf16x3 random cases are plain f32 N(0, 1) - with bf16-exact inputs every lo plane would be zero.  The inputs of every H16 case are exact in
bf16 AND in half (attention_cpu.bf_half; the probes' integers are; asserted in core3_model).

Which case reaches which instantiation (Sq x Skv; every case in both modes - "H16 = true" in the f16 mode, "false" in bf16x3):
  fwd_kernel<3>, bwd_kernel<3>                          256 x 65, 77 (last key block masked: mask16, fill_two's row < valid), 256 x 96 (full);
                                                        per query block: 512 x 77
  fwd_kernel<8>, bwd_kernel<8>                          256 x 225, 240 (masked), 256 x 256 (full); per query block: 512 x 240, 768 x 256;
                                                        per block pair (X3_STREAM off): 512 x 512, 768 x 768, 256 x 768
  fwd_stream_kernel, bwd_dq_stream_kernel,              (X3_STREAM on) 512 x 512 (first and last key block only), 768 x 768 and 256 x 768 (a
  bwd_dkv_stream_kernel                                 middle block, neither first nor last), 256 x 768 (one query block, nqb = 1)
  merge_kernel (+ its planes / half image)              (X3_STREAM off) 512 x 512 (nk = 2), 768 x 768, 256 x 768 (nk = 3); alone: nk 1, 2, 3, 8
  sum_parts_kernel                                      (X3_STREAM off) dq over key blocks, dk / dv over query blocks of the same; alone
  store_image4 (half image, counter | hi / lo planes)   every case: forward context; gradients of the one-tile and streamed routes (the block
                                                        pairs write f32 only: their half images are muse_cast_f32_to_f16's)

Scale invariance (H16): dO 2^-20 with S = 2^20 gives 2^-20 times the results of dO with S = 1 BIT FOR BIT (every step between is identical -
S dO is the same half - or a multiplication by a power of two: dsum, alpha / S, 1 / S), first on the CPU model (test_attention_cpu.py).
"""
import ctypes as C
import functools
import time

import pytest
import torch

import attention_cpu as A
import test_gpu_attention_edges as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
B, NH, HD = G.B, G.NH, 64
H = NH * HD

ONE_TILE = [(256, 65), (256, 77), (256, 96), (256, 225), (256, 240), (256, 256)]
MULTI_Q = [(512, 77), (512, 240)]
LONG = [(512, 512), (768, 768), (256, 768), (768, 256)]
SHAPES = ONE_TILE + MULTI_Q + LONG
# (Sq, Skv, X3_STREAM): the switch only matters for several key blocks, the issue's list runs every LONG shape both ways
CASES = [(sq, skv, True) for sq, skv in ONE_TILE + MULTI_Q] + [(sq, skv, st) for sq, skv in LONG for st in (True, False)]
IDS = [f"{sq}x{skv}-{'stream' if st else 'pairs'}" for sq, skv, st in CASES]
S_PROBE = (1.0, 2.0 ** 13)          # gradient scales of the address probe: max|dO| 2^13 = 40960 stays inside half

# Worst error of attention_cpu.model_h16 / model_x3 against float64 over SHAPES, per element over the terms (lse: absolute), as printed by
# `python tests/test_gpu_attention_x3_edges.py`; one figure per class of the summed length (test_gpu_attention_edges.E_REF), the classes being
# these kernels' own: three key blocks, one tile, several blocks.  The bound is 4 * E_ref.
LEN_CLASSES = (96, 256)             # n <= 96 | 97 .. 256 | >= 257
E_REF_H16 = {                   # n <= 96, 97 .. 256, >= 257       (bound = 4 * E_ref; dk / dv: by the queries, never <= 96)
    "ctx": (1.812e-04, 1.272e-04, 9.116e-05),           # worst at Sq, Skv = (512,77) (512,240) (512,512)
    "lse": (5.314e-07, 5.225e-07, 5.996e-07),           # worst at Sq, Skv = (256,65) (256,240) (768,768)
    "dq": (2.824e-04, 2.067e-04, 1.486e-04),            # worst at Sq, Skv = (512,77) (512,240) (512,512)
    "dk": (0.000e+00, 1.974e-04, 1.371e-04),            # worst at Sq, Skv = None (256,768) (512,512)
    "dv": (0.000e+00, 1.607e-04, 1.046e-04),            # worst at Sq, Skv = None (256,256) (512,512)
    "uniform_dq": (1.036e-04, 5.490e-05, 3.117e-05),    # worst at Sq, Skv = (256,96) (256,256) (512,512)
}
E_REF_X3 = {
    "ctx": (1.002e-05, 1.469e-05, 4.796e-06),           # worst at Sq, Skv = (256,77) (256,225) (512,512)
    "lse": (5.529e-06, 7.668e-06, 3.268e-06),           # worst at Sq, Skv = (256,65) (256,225) (256,768)
    "dq": (1.580e-05, 1.436e-05, 8.500e-06),            # worst at Sq, Skv = (512,77) (768,256) (512,512)
    "dk": (0.000e+00, 1.271e-05, 7.203e-06),            # worst at Sq, Skv = None (256,768) (512,512)
    "dv": (0.000e+00, 9.776e-06, 4.751e-06),            # worst at Sq, Skv = None (256,225) (512,512)
}


def len_class(n):
    return sum(n > t for t in LEN_CLASSES)


def e_ref_for(table, Sq, Skv):
    kc, qc = len_class(Skv), len_class(Sq)
    return {n: v[qc if n in ("dk", "dv") else kc] for n, v in table.items()}


def _ops():
    from muse import ops
    return ops


@functools.lru_cache(maxsize=None)
def random_case(Sq, Skv, mode):
    """one seeded case and its float64 reference per shape and mode (never modified): H16 inputs exact in bf16 and half, bf16x3 inputs f32"""
    c = A.random_case(B, Sq, Skv, NH, HD, G._seed(Sq, Skv, HD) + 7, rnd=A.bf_half if mode == "h16" else None)
    return c, A.reference(c)


@functools.lru_cache(maxsize=None)
def uniform_case_h16(Sq, Skv):
    c = A.uniform_probe(B, Sq, Skv, NH, HD, G._seed(Sq, Skv, HD) + 1, rnd=A.bf_half)
    return c, A.reference(c)


def pairs_route(Sq, Skv):
    """the backward runs per block pair and writes f32 gradients only (no operand images)"""
    ops = _ops()
    return ops.attention_x3_blocked(Sq, Skv) and not ops.attention_x3_streamed(Sq, Skv)


# =====================================================================================================================================
# the entry points, inside their compute mode, with the operand images checked on every run
# =====================================================================================================================================
def _device_operands(c):
    Sq, Skv = c["Sq"], c["Skv"]
    if Sq == Skv:
        qkv = torch.cat([c["q"], c["k"], c["v"]], 1).to(DEV)
        return qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    q, kv = c["q"].to(DEV), torch.cat([c["k"], c["v"]], 1).to(DEV)
    return q, kv[:, :H], kv[:, H:]


def overflow_groups(t, scale):
    """what store_image4 adds to the counter for an f32 result: the groups of four consecutive columns with an element whose half(x * scale)
    is inf or NaN"""
    return int((~torch.isfinite((t.cpu() * scale).to(F16))).reshape(t.shape[0], t.shape[1] // 4, 4).any(-1).sum())


def run_core(c, mode, S=1.0, ctx_bwd=None, planes_only=False):
    """attention_x3_fwd / attention_x3_bwd inside ops.f32_gemms_as_f16 (mode "h16", gradient scale S) or ops.f32_gemms_as_bf16x3 (mode "x3").
    Asserted on EVERY run: the image the forward registers for the context (the merge kernel's on the block-pair route) and the images the
    backward writes for dq, dk, dv (one-tile and streamed routes) are bit for bit muse_cast_f32_to_f16(result, scale) / muse_split_f32_to_bf16x2
    (result), and half's overflow counter holds EXACTLY the number of 4-column groups of those results that leave half's range, computed
    here from the f32 results: 0 in every case but the address probes at S = 2^13 whose keys collect several queries (Sq > Skv: |dv| reaches
    8 = 65536 / 2^13) - a bare "== 0" cannot hold there.  planes_only: a second backward without f32 gradients writes the same images.  -> CPU tensors ctx, lse, dq, dk, dv, "img" (name -> image) and "stats" (forward count, backward count)."""
    ops = _ops()
    Sq, Skv, al = c["Sq"], c["Skv"], c["alpha"]
    h16 = mode == "h16"
    q, k, v = _device_operands(c)
    do = c["do"].to(DEV)
    assert ops.attention_x3_supported(Sq, Skv, HD)
    im = ops.F16Images() if h16 else ops.X3Images()
    scope = (lambda: ops.f32_gemms_as_f16(True, im)) if h16 else (lambda: ops.f32_gemms_as_bf16x3(True, im))
    expect = (lambda t, s: ops.cast_to_f16(t, s)) if h16 else (lambda t, s: ops._split_planes_now(t))
    img, stats = {}, [0, 0]
    with scope():
        ctx, lse = ops.attention_x3_fwd(q, k, v, B, Sq, Skv, NH, HD, al)
        misses = im.misses
        got = im.image(ctx, 1.0) if h16 else ops.split_planes(ctx)
        assert im.misses == misses and im.produced == 1, "the forward did not hand in the context's operand image"
        assert torch.equal(got.reshape(-1, B * Sq, H), expect(ctx, 1.0).reshape(-1, B * Sq, H)), "ctx image differs from the cast / split of the f32 context"
        img["ctx"] = got.cpu()
    if h16:
        stats[0] = im.stats()[0]
        assert stats[0] == overflow_groups(ctx, 1.0) == 0, f"forward: overflow counter {stats[0]}"
        im.backward = True
        im.set_grad_scale(S)
    else:
        assert S == 1.0
    ctxb = ctx if ctx_bwd is None else ctx_bwd.to(DEV)
    expected = 0
    with scope():
        if pairs_route(Sq, Skv):
            dq, dk, dv = ops.attention_x3_bwd(q, k, v, ctxb, do, lse, B, Sq, Skv, NH, HD, al)
        else:
            g = [torch.empty((B * n, H), dtype=F32, device=DEV) for n in (Sq, Skv, Skv)]
            pl = [ops.planes_alloc(t.shape, DEV) for t in g]
            ent = tuple((p[0], p[0].numel()) for p in pl)
            dq, dk, dv = ops.attention_x3_bwd(q, k, v, ctxb, do, lse, B, Sq, Skv, NH, HD, al, dq=g[0], dk=g[1], dv=g[2], planes=ent)
            for n, t, p in zip(("dq", "dk", "dv"), g, pl):
                assert torch.equal(p, expect(t, S).reshape(p.shape)), f"{n} image differs from the cast / split of the f32 {n}"
                img[n] = p.cpu()
                expected += overflow_groups(t, S) if h16 else 0
            if planes_only:
                pl2 = [ops.planes_alloc(t.shape, DEV) for t in g]
                ops.attention_x3_bwd(q, k, v, ctxb, do, lse, B, Sq, Skv, NH, HD, al, planes=tuple((p[0], p[0].numel()) for p in pl2), planes_only=True)
                for n, p, p2 in zip(("dq", "dk", "dv"), pl, pl2):
                    assert torch.equal(p, p2), f"planes_only {n} image differs from the one written next to the f32 {n}"
    if h16:
        stats[1] = im.stats()[0]
        assert stats[1] == expected * (2 if planes_only and not pairs_route(Sq, Skv) else 1), f"backward: overflow counter {stats[1]}, expected {expected}"
    if lse.dim() == 3:                                    # [query block, B * nh, 256]
        lse = lse.permute(1, 0, 2).reshape(B * NH, Sq)
    return dict(ctx=ctx.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu(), img=img, stats=tuple(stats))


def results(out):
    return {n: out[n] for n in A.KINDS}


REPORT = {}     # mode / route -> kind -> [(error over terms, error / bound)]


# =====================================================================================================================================
# (a) H16: probes, every element of every tensor judged
# =====================================================================================================================================
@pytest.mark.parametrize("Sq,Skv,stream", CASES, ids=IDS)
def test_probes_h16(Sq, Skv, stream, monkeypatch):
    """address probe at S = 1 and S = 2^13: ctx == v[target] and dv == the scatter-sum of dO BIT FOR BIT (the other keys' P is 0 as a half;
    the streamed forward: within attention_cpu.mfma_slack, see check_address), lse 0, dq / dk within address_leak_bounds_h16; uniform
    probe (k exact in half too): lse = log Skv, dk == 0, ctx / dv / dq per element"""
    ops = _ops()
    monkeypatch.setattr(ops, "X3_STREAM", stream)
    tag = f"h16 {Sq}x{Skv}"
    slack = ops.attention_x3_streamed(Sq, Skv)
    for n, c in enumerate(G.address_cases(Sq, Skv, HD)):
        for S in S_PROBE:
            out = run_core(c, "h16", S=S, ctx_bwd=A.address_expected(c)[0])
            A.check_address(c, results(out), tag=f"address {tag} call {n} S={S:g}", bf16_out=False, h16=S, ctx_slack=slack)
    c, ref = uniform_case_h16(Sq, Skv)
    A.check_uniform(c, results(run_core(c, "h16")), ref, e_ref_for(E_REF_H16, Sq, Skv)["uniform_dq"], bf16_out=False, tag=f"uniform {tag}", h16=True)


# =====================================================================================================================================
# (b) H16: seeded N(0, 1) per element, scale invariance bit for bit, planes_only images
# =====================================================================================================================================
@pytest.mark.parametrize("Sq,Skv,stream", CASES, ids=IDS)
def test_random_h16(Sq, Skv, stream, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "X3_STREAM", stream)
    c, ref = random_case(Sq, Skv, "h16")
    out = run_core(c, "h16", planes_only=True)
    route = "h16 " + ("pairs" if Skv > 256 and not stream else "stream" if Skv > 256 else "one tile")
    A.check_random(c, results(out), ref, e_ref_for(E_REF_H16, Sq, Skv), tag=f"random h16 {Sq}x{Skv}", report=REPORT.setdefault(route, {}))
    small = dict(c, do=c["do"] * 2.0 ** -20)
    out2 = run_core(small, "h16", S=2.0 ** 20)
    for n in ("ctx", "lse"):
        assert torch.equal(out2[n], out[n]), f"{n} depends on the gradient scale"
    for n in ("dq", "dk", "dv"):
        assert torch.equal(out2[n], out[n] * 2.0 ** -20), f"{n}: (dO 2^-20, S = 2^20) is not 2^-20 x (dO, S = 1) bit for bit"


# =====================================================================================================================================
# (c) H16: overflow is counted, exactly; a non-finite value made inside the core is counted before the optimizer looks
# =====================================================================================================================================
@pytest.mark.parametrize("Sq,Skv,stream", [(256, 256, True), (256, 77, True), (512, 512, True)], ids=["256x256", "256x77", "512x512-stream"])
def test_overflow_counted_h16(Sq, Skv, stream, monkeypatch):
    """every query of a head aimed at ONE key (key 5 + head index): dv of that key is the sum of all Sq dO rows, up to Sq * 5 in magnitude.
    With S = 2^13 the f32 dv is finite and exact, half(dv * S) is inf wherever |dv| >= 8 (65520 and up round to inf): the dv image holds inf
    exactly there and the counter holds the number of 4-column groups (store_image4 counts groups, not elements) with one, computed here
    from the f32 result; dq and dk (leakage only) and the context's image add nothing."""
    ops = _ops()
    monkeypatch.setattr(ops, "X3_STREAM", stream)
    S = 2.0 ** 13
    targets = (5 + torch.arange(B * NH)).reshape(B, NH, 1).expand(B, NH, Sq).contiguous()
    c = A.address_probe(B, Sq, Skv, NH, HD, targets)
    out = run_core(c, "h16", S=S, ctx_bwd=A.address_expected(c)[0])
    A.check_address(c, results(out), tag=f"overflow {Sq}x{Skv}", bf16_out=False, h16=S, ctx_slack=ops.attention_x3_streamed(Sq, Skv))
    want = (out["dv"] * S).to(F16)
    groups = overflow_groups(out["dv"], S)
    assert groups == 16 * B * NH and overflow_groups(out["dq"], S) == overflow_groups(out["dk"], S) == 0      # (every group of the six target rows)
    assert groups > 0 and float(out["dv"].abs().max()) > 100.0
    got = out["img"]["dv"][0]
    assert torch.equal(got.isinf(), want.isinf()) and torch.equal(got.view(torch.int16), want.view(torch.int16)), "dv image: inf in other elements than half(dv * S)"
    print(f"[attention_x3_edges] overflow {Sq}x{Skv}: expected {groups} groups, counted {out['stats'][1]}; forward counted {out['stats'][0]}")
    assert out["stats"] == (0, groups), f"counted {out['stats']}, expected (0, {groups})"


@pytest.mark.parametrize("Sq,Skv,stream", [(256, 256, True), (512, 512, True), (512, 512, False)], ids=["256x256", "512x512-stream", "512x512-pairs"])
def test_nonfinite_inside_the_core_is_counted_h16(Sq, Skv, stream, monkeypatch):
    """dO * S above 65504: half(dO * S) is inf, the f32 gradients are non-finite by design.  Where the kernel writes images the counter is
    > 0 straight away; on the block-pair route (f32 gradients only) it is > 0 once the gradient's image has been taken, because
    muse_cast_f32_to_f16 counts any all-ones exponent"""
    ops = _ops()
    monkeypatch.setattr(ops, "X3_STREAM", stream)
    c, _ = random_case(Sq, Skv, "h16")
    S = 2.0 ** 20
    assert float((c["do"].abs() * S).max()) > 65504
    q, k, v = _device_operands(c)
    im = ops.F16Images()
    with ops.f32_gemms_as_f16(True, im):
        ctx, lse = ops.attention_x3_fwd(q, k, v, B, Sq, Skv, NH, HD, c["alpha"])
    assert im.stats()[0] == 0
    im.backward = True
    im.set_grad_scale(S)
    with ops.f32_gemms_as_f16(True, im):
        if pairs_route(Sq, Skv):
            dq, dk, dv = ops.attention_x3_bwd(q, k, v, ctx, c["do"].to(DEV), lse, B, Sq, Skv, NH, HD, c["alpha"])
            assert not bool(torch.isfinite(dq).all())
            im.image(dq, S)
        else:
            g = [torch.empty((B * n, H), dtype=F32, device=DEV) for n in (Sq, Skv, Skv)]
            pl = [ops.planes_alloc(t.shape, DEV) for t in g]
            ops.attention_x3_bwd(q, k, v, ctx, c["do"].to(DEV), lse, B, Sq, Skv, NH, HD, c["alpha"], dq=g[0], dk=g[1], dv=g[2],
                                 planes=tuple((p[0], p[0].numel()) for p in pl))
            assert not bool(torch.isfinite(g[0]).all())
    n = im.stats()[0]
    print(f"[attention_x3_edges] non-finite gradients {Sq}x{Skv} {'stream' if stream else 'pairs'}: counted {n}")
    assert n > 0, "non-finite gradients of the H16 core reached no overflow counter"


# =====================================================================================================================================
# (d) bf16x3: seeded f32 N(0, 1) per element, planes bit for bit (the probes, 768 included, are test_gpu_attention_edges.test_probes_x3)
# =====================================================================================================================================
@pytest.mark.parametrize("Sq,Skv,stream", CASES, ids=IDS)
def test_random_x3(Sq, Skv, stream, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "X3_STREAM", stream)
    c, ref = random_case(Sq, Skv, "x3")
    out = run_core(c, "x3", planes_only=True)
    route = "x3 " + ("pairs" if Skv > 256 and not stream else "stream" if Skv > 256 else "one tile")
    A.check_random(c, results(out), ref, e_ref_for(E_REF_X3, Sq, Skv), tag=f"random x3 {Sq}x{Skv}", report=REPORT.setdefault(route, {}))


# =====================================================================================================================================
# (e) both modes: poisoned surroundings
# =====================================================================================================================================
GAP, PADC, SENTINEL = G.GAP, G.PADC, G.SENTINEL
LD = H + PADC


def _gapped(rows, S, fill, dtype=F32, planes=None):
    """[B * S, H] -> [GAP + B (S + GAP), H + PADC] device buffer (planes: that many stacked) filled with `fill`, the images' rows S + GAP
    apart and GAP rows in: nothing the kernels address lies outside the allocation"""
    shape = (GAP + B * (S + GAP), LD)
    buf = torch.full(shape if planes is None else (planes,) + shape, fill, dtype=dtype)
    if rows is not None:
        buf[GAP:].view(B, S + GAP, LD)[:, :S, :H] = rows.view(B, S, H)
    return buf.to(DEV)


def _data(buf, S):
    """the images' own S x H blocks of a (stack of) gapped buffer(s) -> [.., B * S, H]"""
    return buf[..., GAP:, :].reshape(buf.shape[:-2] + (B, S + GAP, LD))[..., :S, :H].reshape(buf.shape[:-2] + (B * S, H))


@pytest.mark.parametrize("mode", ["h16", "x3"])
@pytest.mark.parametrize("Sq,Skv", [(256, 65), (256, 77), (256, 225), (256, 240), (512, 512)])
def test_poisoned_surroundings_x3(Sq, Skv, mode, monkeypatch):
    """f32 q, k, v, dO with NaN in the rows between (and before) the images and in the feature columns behind H - at Skv 65 .. 240 the rows
    >= Skv that fill_two must not read are gap rows -, ctx / dq / dk / dv and their operand images with the same gaps prefilled with a
    sentinel; 512 x 512: the streaming entry points (block offsets on top of the batch strides).  Results, lse and images equal the
    gap-free run bit for bit and no sentinel is touched."""
    ops = _ops()
    monkeypatch.setattr(ops, "X3_STREAM", True)
    h16, streamed = mode == "h16", Skv > 256
    S = 4.0 if h16 else 1.0
    c, _ = random_case(Sq, Skv, mode)
    clean = run_core(c, mode, S=S)
    nan = float("nan")
    q, do = _gapped(c["q"], Sq, nan), _gapped(c["do"], Sq, nan)
    k, v = _gapped(c["k"], Skv, nan), _gapped(c["v"], Skv, nan)
    lens = dict(ctx=Sq, dq=Sq, dk=Skv, dv=Skv)
    res = {n: _gapped(None, s, SENTINEL) for n, s in lens.items()}
    img = {n: _gapped(None, s, SENTINEL, F16 if h16 else BF, 1 if h16 else 2) for n, s in lens.items()}
    lse = torch.empty((Sq // 256, B * NH, 256), dtype=F32, device=DEV)
    dsum = torch.empty_like(lse)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    view = lambda t: t[GAP:, :H]
    ip = lambda n: (view(img[n][0]).data_ptr(), img[n][0].numel())
    d = ops._attn_desc(view(q), view(k), view(v), view(res["ctx"]), B, Sq, Skv, NH, HD, c["alpha"])
    bq, bk = (Sq + GAP) * LD, (Skv + GAP) * LD
    d.bsq, d.bsk, d.bsv, d.bso = bq, bk, bk, bq
    half = 1 if h16 else 0
    lib = ops.lib()
    grads = (view(res["dq"]).data_ptr(), LD, bq, view(res["dk"]).data_ptr(), LD, bk, view(res["dv"]).data_ptr(), LD, bk, *ip("dq"), *ip("dk"), *ip("dv"),
             half, S, stats.data_ptr(), ops.stream())
    if streamed:
        ops.check(lib.muse_attention_x3_fwd_stream(C.byref(d), lse.data_ptr(), *ip("ctx"), half, 1.0, stats.data_ptr(), ops.stream()), "muse_attention_x3_fwd_stream")
        ops.check(lib.muse_attention_x3_bwd_stream(C.byref(d), view(do).data_ptr(), LD, bq, lse.data_ptr(), dsum.data_ptr(), *grads), "muse_attention_x3_bwd_stream")
    else:
        ops.check(lib.muse_attention_x3_fwd(C.byref(d), lse.data_ptr(), *ip("ctx"), half, 1.0, stats.data_ptr(), ops.stream()), "muse_attention_x3_fwd")
        ops.check(lib.muse_attention_x3_bwd(C.byref(d), view(do).data_ptr(), LD, bq, lse.data_ptr(), *grads), "muse_attention_x3_bwd")
    lse = lse.permute(1, 0, 2).reshape(B * NH, Sq)
    torch.cuda.synchronize()
    assert torch.equal(lse.cpu(), clean["lse"]), "lse differs from the gap-free run"
    assert stats.tolist() == [0, 0]
    for n, s in lens.items():
        for what, buf, want in ((n, res[n].cpu(), clean[n]), (n + " image", img[n].cpu(), clean["img"][n])):
            got = _data(buf, s)
            assert torch.equal(got.reshape(want.shape), want), f"{what} differs from the gap-free run ({int((got.reshape(want.shape) != want).sum())} elements)"
            buf[..., GAP:, :].view(buf.shape[:-2] + (B, s + GAP, LD))[..., :s, :H] = SENTINEL
            assert bool((buf == SENTINEL).all()), f"{what}: {int((buf != SENTINEL).sum())} sentinel elements outside the images were overwritten"


# =====================================================================================================================================
# (f) muse_attention_x3_merge and muse_sum_parts_strided on their own
# =====================================================================================================================================
@pytest.mark.parametrize("heads", [3, 17])
@pytest.mark.parametrize("seq", [256, 768])
@pytest.mark.parametrize("nk", [1, 2, 3, 8])
def test_merge_alone(nk, seq, heads):
    """synthetic partials: lp multiples of 2^-10 in [-4, 4] (every l_j - m is exact), the LAST key block's 80 below (its weight e^-80 .. e^-88
    vanishes against the others; out and lse stay finite and within the bound), 17 heads: H = 1088 > 1024, the column loop's second step.
    Against float64.  Bound from the operation count, one unit of f32's last place (2^-23) per expf / logf, half of one per product or sum:
      lse = m + logf(sum_j expf(l_j - m)): nk expf and nk sums on a value in [1, nk], logf, one sum: (nk + 4) 2^-23 max(1, |lse|)
      out = sum_j expf(l_j - lse) part_j: the weights carry lse's error and the rounding of l_j - lse (< 16 2^-24 for a weight above e^-16),
            one expf, one product and one sum each: ((nk + 4) max(1, |lse|) + nk / 2 + 10) 2^-23 of the terms sum_j w_j |part_j|
    Planes (bf16x3) and half image (f16 mode, counter 0) of out bit for bit its split / cast."""
    ops = _ops()
    Hh, nq = heads * 64, seq // 256
    g = torch.Generator().manual_seed(9000 + 100 * nk + seq + heads)
    part = torch.randn((nk, B * seq, Hh), generator=g)
    lp = torch.randint(-4096, 4097, (nk, nq, B * heads, 256), generator=g).float() / 1024
    if nk > 1:
        lp[nk - 1] -= 80.0
    l64 = lp.double()
    lse_ref = torch.logsumexp(l64, 0)
    w = torch.exp(l64 - lse_ref)                                             # [nk, nq, B * heads, 256]
    rows = lambda t: t.reshape(-1, nq, B, heads, 256).permute(0, 2, 1, 4, 3).reshape(-1, B * seq, heads).repeat_interleave(64, -1)
    out_ref = (rows(w) * part.double()).sum(0)
    terms = (rows(w) * part.double().abs()).sum(0).clamp(min=A.TINY)
    pd, lpd = part.to(DEV), lp.to(DEV)
    outs = {}
    for half in (0, 1):
        out = torch.full((B * seq, Hh), SENTINEL, dtype=F32, device=DEV)
        lse = torch.full((nq, B * heads, 256), SENTINEL, dtype=F32, device=DEV)
        planes = torch.empty((1 if half else 2, B * seq, Hh), dtype=F16 if half else BF, device=DEV)
        stats = torch.zeros(2, dtype=torch.int32, device=DEV)
        ops.check(ops.lib().muse_attention_x3_merge(pd.data_ptr(), pd[0].numel(), lpd.data_ptr(), lpd[0].numel(), nk, out.data_ptr(), lse.data_ptr(),
                                                    planes.data_ptr(), out.numel(), B, seq, heads, half, 1.0, stats.data_ptr(), ops.stream()),
                  "muse_attention_x3_merge")
        want = ops.cast_to_f16(out).reshape(planes.shape) if half else ops._split_planes_now(out)
        assert torch.equal(planes, want), f"half={half}: image differs from the cast / split of out"
        assert stats.tolist() == [0, 0]
        outs[half] = (out.cpu(), lse.cpu())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    out, lse = outs[0]
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    lb = (nk + 4) * 2.0 ** -23 * lse_ref.abs().clamp(min=1.0)
    wl = A._worst((lse.double() - lse_ref).abs(), lb)
    ob = (rows(lb[None])[0] + (nk / 2 + 10) * 2.0 ** -23) * terms
    wo = A._worst((out.double() - out_ref).abs(), ob)
    print(f"[attention_x3_edges] merge nk={nk} seq={seq} heads={heads}: lse err/bound={wl:.3f} out err/bound={wo:.3f}")
    REPORT.setdefault("merge", {}).setdefault("lse", []).append((float((lse.double() - lse_ref).abs().max()), wl))
    REPORT.setdefault("merge", {}).setdefault("out", []).append((A.measure(out, out_ref, terms), wo))
    assert wl <= 1.0 and wo <= 1.0, (wl, wo)


def test_merge_refuses_nine_blocks():
    ops = _ops()
    part = torch.zeros((9, B * 256, H), device=DEV)
    lp = torch.zeros((9, 1, B * NH, 256), device=DEV)
    out = torch.full((B * 256, H), SENTINEL, device=DEV)
    lse = torch.full((1, B * NH, 256), SENTINEL, device=DEV)
    for nk in (9, 0):
        rc = ops.lib().muse_attention_x3_merge(part.data_ptr(), part[0].numel(), lp.data_ptr(), lp[0].numel(), nk, out.data_ptr(), lse.data_ptr(), None, 0,
                                               B, 256, NH, 0, 1.0, None, ops.stream())
        assert rc == -3, (nk, rc)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((lse == SENTINEL).all())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n,rows,cols", [(1, 300, 192), (2, 300, 192), (5, 300, 192), (2, 15424, 1088)],
                         ids=["n1", "n2", "n5", "n2-two-sweeps"])
def test_sum_parts_alone(n, rows, cols, accumulate):
    """out rows of pitch cols + 8 with a guarded pad; 15424 x 1088 / 4 = 4195328 vectors > 16384 x 256: the grid-stride loop sweeps twice.
    Exact against the same f32 additions in the order j = 0, 1, ... (then the old contents when accumulating)"""
    ops = _ops()
    g = torch.Generator().manual_seed(7000 + n + rows)
    parts = torch.randn((n, rows, cols), generator=g)
    old = torch.randn((rows, cols), generator=g)
    assert rows * cols // 4 > 16384 * 256 or rows == 300
    want = parts[0].clone()
    for j in range(1, n):
        want += parts[j]
    if accumulate:
        want += old
    out = torch.full((rows, cols + 8), SENTINEL)
    out[:, :cols] = old
    out, pd = out.to(DEV), parts.to(DEV)
    ops.check(ops.lib().muse_sum_parts_strided(pd.data_ptr(), pd[0].numel(), n, rows, cols, out.data_ptr(), cols + 8, accumulate, ops.stream()),
              "muse_sum_parts_strided")
    out = out.cpu()
    assert torch.equal(out[:, :cols], want), f"{int((out[:, :cols] != want).sum())} elements differ from the ordered f32 sum"
    assert bool((out[:, cols:] == SENTINEL).all()), "the pad columns were written"


# =====================================================================================================================================
# (g) refusals, with nothing launched
# =====================================================================================================================================
BAD_ARG, ALIGN, UNSUPPORTED = -1, -2, -3
REFUSALS = [("Skv 64", dict(seq_kv=64), UNSUPPORTED), ("Skv 97", dict(seq_kv=97), UNSUPPORTED), ("Skv 224", dict(seq_kv=224), UNSUPPORTED),
            ("Skv 257", dict(seq_kv=257), UNSUPPORTED), ("Sq 255", dict(seq_q=255), UNSUPPORTED), ("head dim 48", dict(head_dim=48), UNSUPPORTED),
            ("stride 194", dict(ldq=H + 2), ALIGN), ("scale 3", dict(scale=3.0), BAD_ARG), ("scale 0", dict(scale=0.0), BAD_ARG),
            ("half 2", dict(half=2), BAD_ARG)]


@pytest.mark.parametrize("half", [0, 1], ids=["x3", "h16"])
@pytest.mark.parametrize("what,change,code", REFUSALS, ids=[r[0].replace(" ", "") for r in REFUSALS])
def test_refusals(what, change, code, half):
    """one thing wrong per call, on buffers that a launch would be free to write (2 x 257 rows): the one-tile and the streaming entry points,
    forward and backward, return the code attn3::check / check_stream / image_format document - UNSUPPORTED for a shape, ALIGN for a stride
    that breaks the 16-byte vectors, BAD_ARG for a scale that is no positive power of two or half = 2 - and write nothing"""
    ops = _ops()
    n = B * 257
    q, k, v, do = (torch.zeros((n, H + 4), device=DEV) for _ in range(4))
    outs = [torch.full((n, H + 4), SENTINEL, device=DEV) for _ in range(4)]
    lse = torch.full((B * NH, 512), SENTINEL, device=DEV)
    dsum = torch.full((B * NH, 512), SENTINEL, device=DEV)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    d = ops._attn_desc(q[:, :H], k[:, :H], v[:, :H], outs[0][:, :H], B, 256, 256, NH, HD, 0.125)
    args = dict(half=half, scale=1.0)
    for name, val in change.items():
        if name in args:
            args[name] = val
        else:
            setattr(d, name, val)
    img = (args["half"], args["scale"], stats.data_ptr(), ops.stream())
    ld, bs = H + 4, 256 * (H + 4)
    grads = (outs[1].data_ptr(), ld, bs, outs[2].data_ptr(), ld, bs, outs[3].data_ptr(), ld, bs, None, 0, None, 0, None, 0)
    lib = ops.lib()
    rcs = dict(fwd=lib.muse_attention_x3_fwd(C.byref(d), lse.data_ptr(), None, 0, *img),
               bwd=lib.muse_attention_x3_bwd(C.byref(d), do.data_ptr(), ld, bs, lse.data_ptr(), *grads, *img))
    rcs.update(fwd_stream=lib.muse_attention_x3_fwd_stream(C.byref(d), lse.data_ptr(), None, 0, *img),       # (check_stream refuses each of these too)
               bwd_stream=lib.muse_attention_x3_bwd_stream(C.byref(d), do.data_ptr(), ld, bs, lse.data_ptr(), dsum.data_ptr(), *grads, *img))
    torch.cuda.synchronize()
    assert all(rc == code for rc in rcs.values()), f"{what}: {rcs}, expected {code}"
    for t in outs + [lse, dsum]:
        assert bool((t == SENTINEL).all()), f"{what}: a refused call wrote"
    assert stats.tolist() == [0, 0]


def test_report():
    """(last in the file) the worst figures of this run per mode / route and output kind, for profiles/attention_edges.md"""
    for ep, kinds in REPORT.items():
        for n, vals in kinds.items():
            print(f"[attention_x3_edges] worst {ep} {n}: err={max(v[0] for v in vals):.3e} err/bound={max(v[1] for v in vals):.3f} over {len(vals)} cases")


# =====================================================================================================================================
# `python tests/test_gpu_attention_x3_edges.py`: E_REF_H16 and E_REF_X3 on a CPU, over SHAPES
# =====================================================================================================================================
def measure_e_ref():
    worst = {"E_REF_H16": {n: [0.0] * 3 for n in E_REF_H16}, "E_REF_X3": {n: [0.0] * 3 for n in E_REF_X3}}
    where = {}

    def take(tab, key, cls, val, shape):
        if val > worst[tab][key][cls]:
            worst[tab][key][cls], where[tab, key, cls] = val, shape
    for Sq, Skv in SHAPES:
        kc, qc = len_class(Skv), len_class(Sq)
        for tab, mode, model in (("E_REF_H16", "h16", A.model_h16), ("E_REF_X3", "x3", A.model_x3)):
            c, ref = random_case(Sq, Skv, mode)
            for n, e in A.model_errors(c, ref, model=model).items():
                take(tab, n, qc if n in ("dk", "dv") else kc, e, (Sq, Skv))
        c, ref = uniform_case_h16(Sq, Skv)
        take("E_REF_H16", "uniform_dq", kc, A.model_errors(c, ref, ("dq",), model=A.model_h16)["dq"], (Sq, Skv))
        random_case.cache_clear()
        uniform_case_h16.cache_clear()
    return worst, where


if __name__ == "__main__":
    t0 = time.time()
    worst, where = measure_e_ref()
    same = True
    for tab, table in (("E_REF_H16", E_REF_H16), ("E_REF_X3", E_REF_X3)):
        print(tab + " = {")
        for n in table:
            vals = "(" + ", ".join(f"{v:.3e}" for v in worst[tab][n]) + ")"
            print(f'    "{n}": {vals},'.ljust(56) + "# worst at Sq, Skv = " + " ".join(str(where.get((tab, n, i))).replace(" ", "") for i in range(3)))
        print("}")
        same = same and all(f"{w:.3e}" == f"{e:.3e}" for n in table for w, e in zip(worst[tab][n], table[n]))
    print(f"{'matches' if same else 'DIFFERS FROM'} the tables in this file ({time.time() - t0:.0f} s)")
