"""GPU (-m gpu): the fused attention kernels (csrc/attention.hip, attention2.hip, attention3.hip and the causal policy of attention_enc.hip)
with exact key probes and per-element bounds at every edge of their dispatch, B = 2 images x 3 heads, no sequence longer than 1025.
tests/attention_cpu.py holds the float64 reference, the contract model, the probe builders and the checks; tests/test_attention_cpu.py
proves on the CPU that those checks fail for a dropped key, a leaked pad key and a causal mask off by one.  profiles/attention_edges.md
has the table of bounds and the MI355X's observed values.

Why probes: out-of-range K / V rows come back from the buffer descriptor as zeros, so a leaked pad key has score 0 and value 0 and moves a
random-input context by less than the bf16 rounding of P; max|a - b| / max|b| bars of 1.5e-2 / 1e-3 / 3e-2 cannot see it, nor a dropped last
key at S = 1025.  The address probe (ctx = v[target] bit for bit, lse = 0) and the uniform probe (lse = log Skv) turn either into an error
of order one; the seeded N(0, 1) cases are judged per element over the terms each result adds up (attention_cpu.py), with the bound
4 * E_REF[kind] (+ one bf16 rounding of the reference), E_REF being the contract model's own worst error against float64 over the same case
lists, printed by `python tests/test_gpu_attention_edges.py` on a CPU.

Which case meets which branch (Sq x Skv; "self" = the SELF_LENS at all four head dims, "cross" = CROSS at head dims 64 and 48):
  attn_fwd_launch, one K/V tile (Skv <= 288):
    2 | 4 | 6 key tiles                      Skv 1, 16, 17, 32 | 33, 64 | 65, 80, 96 (self; cross 50 x 7, 16 x 33, 80 x 64, 256 x 77)
    every-tile-masked 16-tile form           Skv 97, 129, 224 (self; cross 96 x 97)
    16 | 18 key tiles, last pair masked      Skv 225, 256 | 257, 288 (self - at head dim 48 only with MUSE_ATTN2=0, the ATTN2 list)
    4 | 8 waves (Sq <= 96 | >= 97)           self 96 | 97; cross 80 x 257 (4 q-tiles' worth of waves on the 8-wave 18-tile kernel)
    shared leftover tile, 4 waves            self 80 (5 q-tiles), cross 80 x 64; not taken at 80 x 257 (the 8-wave kernels with <= 6 q-tiles)
    shared leftover tile, 8 waves            self 129 (9 q-tiles), 257 (17), cross 257 x 1, 129 x 77 ; not taken at 128 / 256 (self)
                                             with key pairs that are all mask (the every-tile-masked form, 97 <= Skv <= 224): self 129, cross
                                             257 x 130 - NaN at head dims 16, 48, 64 before the shared loop skipped those pairs
    whole head | 256-query chunks            cross 384 x 77, 384 x 288 | 385 x 77, 385 x 288, 512 x 77
  attn_fwd_launch, streamed K/V (Skv >= 289), 128-query chunks:
    masked | unmasked last tile              Skv 289 (tail 33), 480 (224), 513 (1), 1025 (1) | 481 (225), 512 (256) (self; cross 17 x 289,
                                             128 / 129 x 480 / 481, 130 x 513, 1 x 289)
    one | two query chunks                   cross 128 x 480, 128 x 481 | 129 x 480, 129 x 481, 130 x 513
  make_plan (dQ: stationary Sq, streamed Skv; dK / dV: stationary Skv, streamed Sq):
    streamed side one tile | 256-row tiles   288 | 289 on either side: self 288 | 289, cross 384 x 288 | 17 x 289 (keys), 257 x 1 | 385 x 77 (queries)
    whole head (<= 24 tiles) | 256 chunks    dQ: cross 384 x 77 | 385 x 77; dK / dV: cross 97 x 384 | 97 x 385, 129 x 480, 130 x 513
    4 | 8 waves, shared tile                 as the forward on the stationary side: self 96 | 97, 80, 129, 257; dK / dV shared at Skv 80, 129, 257
    128-row chunks (both sides long)         self 289 .. 1025
  attention2.hip shape_ok (head dim 48, self, 225 <= S <= 260): ATTN2_LENS 224 | 225, 256 | 257 (8 | 9 key blocks), 260 | 261, each with
    MUSE_ATTN2=1 and =0 (at 224 and 261 both settings must reach the general kernels)
  attention3.hip: 3 | 8 key blocks (Skv 65, 77, 96 | 225, 240, 256), one | several 256-query blocks (Sq 256 | 512, 768), several key blocks
    (Skv 512; 768: a middle block, neither first nor last) streamed (X3_STREAM) or as block pairs + merge.  Here: the probes on the bf16x3
    instantiations; tests/test_gpu_attention_x3_edges.py has their seeded cases and planes and everything on the H16 ("f16" mode) ones
  attention_enc.hip, causal policy: S 1, 15, 16, 17, 32, 33, 77, 127, 128 (1 .. 8 waves; an odd number of key tiles; the S = 128 limit)
"""
import ctypes as C
import functools
import time

import pytest
import torch

import attention_cpu as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
B, NH = 2, 3

# Worst error of attention_cpu.contract_model against float64 over the case lists below, before the model's output rounding, as printed by
# `python tests/test_gpu_attention_edges.py`: per element over the terms (lse: absolute).  The bound is 4 * E_REF (+ one bf16 rounding).
# One figure per class of the length n a result is summed over (the keys for ctx, lse and dq, the queries for dk and dv): the bf16 roundings
# of P and dS are independent, so their sum shrinks against the terms as n grows - a single worst figure would be set by 50 x 7 and 1 x 289
# and would let the dropped key at S = 1025 (2.1e-2 of the dq terms) pass.  The classes are the kernels' own: two key tiles, one K/V tile,
# streamed.  The causal kernel's rows hold 1 .. S keys each: one figure.
LEN_CLASSES = (32, 288)         # n <= 32 | 33 .. 288 | >= 289
E_REF = {                       # n <= 32, 33 .. 288, >= 289      (bound = 4 * E_ref)
    "ctx": (2.697e-03, 1.695e-03, 9.020e-04),           # worst at Sq, Skv, hd = (50,7,48) (33,33,32) (385,385,32)
    "lse": (1.451e-03, 1.111e-03, 6.166e-04),           # worst at Sq, Skv, hd = (50,7,48) (33,33,16) (289,289,16)
    "dq": (1.670e-02, 3.637e-03, 1.837e-03),            # worst at Sq, Skv, hd = (50,7,64) (80,80,16) (289,289,64)
    "dk": (1.377e-02, 2.413e-03, 1.535e-03),            # worst at Sq, Skv, hd = (1,289,48) (224,224,48) (512,512,48)
    "dv": (4.151e-03, 2.610e-03, 1.492e-03),            # worst at Sq, Skv, hd = (1,289,48) (33,33,16) (384,288,64)
    "uniform_dq": (2.399e-03, 1.127e-03, 5.719e-04),    # worst at Sq, Skv, hd = (50,7,64) (33,33,32) (289,289,16)
    "causal_ctx": (2.566e-03,),                         # worst at Sq, Skv, hd = (32,32,64)
}


def len_class(n):
    return sum(n > t for t in LEN_CLASSES)


def e_ref_for(Sq, Skv):
    """kind -> E_ref of a case: by the keys for ctx, lse, dq (and the uniform probe's dq), by the queries for dk, dv"""
    kc, qc = len_class(Skv), len_class(Sq)
    return dict(ctx=E_REF["ctx"][kc], lse=E_REF["lse"][kc], dq=E_REF["dq"][kc], dk=E_REF["dk"][qc], dv=E_REF["dv"][qc],
                uniform_dq=E_REF["uniform_dq"][kc])


HDS = (16, 32, 48, 64)
SELF_LENS = [1, 16, 17, 32, 33, 64, 65, 80, 96, 97, 128, 129, 224, 225, 256, 257, 288, 289, 384, 385, 480, 481, 512, 513, 1025]
CROSS_HDS = (64, 48)
CROSS = [(256, 77), (384, 77), (385, 77), (512, 77), (129, 77), (17, 289), (1, 289), (128, 480), (129, 480), (128, 481), (129, 481), (1, 257),
         (257, 1), (384, 288), (385, 288), (130, 513), (97, 384), (97, 385), (80, 257), (80, 64), (96, 97), (16, 33), (50, 7), (257, 130)]
ATTN2_LENS = [224, 225, 256, 257, 260, 261]
CAUSAL_LENS = [1, 15, 16, 17, 32, 33, 77, 127, 128]
CAUSAL_HDS = (32, 64)
X3_SQ, X3_SKV = (256, 512, 768), (65, 77, 96, 225, 240, 256, 512, 768)
POISON = [(17, 64, None), (77, 64, None), (257, 64, None), (257, 48, "1"), (257, 48, "0"), (289, 64, None), (513, 64, None)]

BF16_SHAPES = ([(s, s, hd) for hd in HDS for s in SELF_LENS] + [(sq, skv, hd) for hd in CROSS_HDS for sq, skv in CROSS]
               + [(s, s, 48) for s in ATTN2_LENS if s not in SELF_LENS])


def _ops():
    from muse import ops
    return ops


def _seed(Sq, Skv, hd):
    return 100000 + 131 * Sq + 17 * Skv + hd


@functools.lru_cache(maxsize=None)
def random_case(Sq, Skv, hd, causal=False):
    """one seeded case and its float64 reference per shape, shared by every test that needs them (never modified)"""
    c = A.random_case(B, Sq, Skv, NH, hd, _seed(Sq, Skv, hd), causal=causal)
    return c, A.reference(c)


@functools.lru_cache(maxsize=None)
def uniform_case(Sq, Skv, hd):
    c = A.uniform_probe(B, Sq, Skv, NH, hd, _seed(Sq, Skv, hd) + 1)
    return c, A.reference(c)


def address_cases(Sq, Skv, hd):
    for maps in A.address_maps(Sq, Skv, B * NH):
        yield A.address_probe(B, Sq, Skv, NH, hd, maps.reshape(B, NH, Sq))


# =====================================================================================================================================
# the entry points
# =====================================================================================================================================
def run_packed(c, bwd=True):
    """attention_fwd / attention_bwd on a packed q | k | v projection (self-attention)"""
    ops = _ops()
    S, hd, H, al = c["Sq"], c["hd"], NH * c["hd"], c["alpha"]
    qkv = torch.cat([c["q"], c["k"], c["v"]], 1).to(BF).to(DEV)
    ctx, lse = ops.attention_fwd(qkv, B, S, NH, hd, al)
    out = dict(ctx=ctx.cpu(), lse=lse[:, :S].cpu())
    if bwd:
        d = ops.attention_bwd(qkv, ctx, c["do"].to(BF).to(DEV), lse, B, S, NH, hd, al).cpu()
        out.update(dq=d[:, :H], dk=d[:, H:2 * H], dv=d[:, 2 * H:])
    return out


def run_ex(c, bwd=True):
    """attention_fwd_ex / attention_bwd_ex: q rows with stride H + 8, k | v packed, dk | dv written into the halves of one packed gradient"""
    ops = _ops()
    Sq, Skv, hd, H, al = c["Sq"], c["Skv"], c["hd"], NH * c["hd"], c["alpha"]
    qp = torch.cat([c["q"], torch.full((B * Sq, 8), 3.0)], 1).to(BF).to(DEV)
    kv = torch.cat([c["k"], c["v"]], 1).to(BF).to(DEV)
    ctx, lse = ops.attention_fwd_ex(qp[:, :H], kv[:, :H], kv[:, H:], B, Sq, Skv, NH, hd, al)
    out = dict(ctx=ctx.cpu(), lse=lse[:, :Sq].cpu())
    if bwd:
        dkv = torch.full((B * Skv, 2 * H), 7.0, dtype=BF, device=DEV)
        dq, _, _ = ops.attention_bwd_ex(qp[:, :H], kv[:, :H], kv[:, H:], ctx, c["do"].to(BF).to(DEV), lse, B, Sq, Skv, NH, hd, al,
                                        dk=dkv[:, :H], dv=dkv[:, H:])
        dkv = dkv.cpu()
        out.update(dq=dq.cpu(), dk=dkv[:, :H], dv=dkv[:, H:])
    return out


def run_causal(c):
    ops = _ops()
    S, hd, H = c["Sq"], c["hd"], NH * c["hd"]
    qkv = torch.cat([c["q"], c["k"], c["v"]], 1).to(BF).to(DEV)
    return dict(ctx=ops.causal_attention_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, S, NH, hd, c["alpha"]).cpu())


def run_x3(c, ctx_bwd=None):
    """attention_x3_fwd / attention_x3_bwd on f32 tensors (packed for self-attention, q and k | v otherwise).  ctx_bwd: the context the
    backward reads instead of the forward's own"""
    ops = _ops()
    Sq, Skv, hd, H, al = c["Sq"], c["Skv"], c["hd"], NH * c["hd"], c["alpha"]
    if Sq == Skv:
        qkv = torch.cat([c["q"], c["k"], c["v"]], 1).to(DEV)
        q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    else:
        q, kv = c["q"].to(DEV), torch.cat([c["k"], c["v"]], 1).to(DEV)
        k, v = kv[:, :H], kv[:, H:]
    assert ops.attention_x3_supported(Sq, Skv, hd)
    ctx, lse = ops.attention_x3_fwd(q, k, v, B, Sq, Skv, NH, hd, al)
    dq, dk, dv = ops.attention_x3_bwd(q, k, v, ctx if ctx_bwd is None else ctx_bwd.to(DEV), c["do"].to(DEV), lse, B, Sq, Skv, NH, hd, al)
    if lse.dim() == 3:                                    # [query block, B * nh, 256]
        lse = lse.permute(1, 0, 2).reshape(B * NH, Sq)
    return dict(ctx=ctx.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())


def probes(run, Sq, Skv, hd, bf16_out=True):
    """group (a) / (b) on one shape: every address map of the shape, then the uniform probe"""
    tag = f"{Sq}x{Skv} hd{hd}"
    for n, c in enumerate(address_cases(Sq, Skv, hd)):
        # (an f32 context can sit one unit in the last place off v[target] - attention_cpu.mfma_slack - and dsum = dO . O then no longer
        # cancels dp at the target: the bf16x3 backward reads the exact context, so that its dq and dk stay pure leakage)
        out = run(c) if bf16_out else run(c, ctx_bwd=A.address_expected(c)[0])
        A.check_address(c, out, tag=f"address {tag} call {n}", bf16_out=bf16_out)
    c, ref = uniform_case(Sq, Skv, hd)
    A.check_uniform(c, run(c), ref, e_ref_for(Sq, Skv)["uniform_dq"], bf16_out=bf16_out, tag=f"uniform {tag}")


def randoms(run, Sq, Skv, hd):
    c, ref = random_case(Sq, Skv, hd)
    A.check_random(c, run(c), ref, e_ref_for(Sq, Skv), tag=f"random {Sq}x{Skv} hd{hd}", report=REPORT.setdefault(run.__name__, {}))


REPORT = {}     # entry point -> kind -> [(error over terms, error / bound)]: printed at the end of a `-s` run for profiles/attention_edges.md


# =====================================================================================================================================
# (a) probes on the bf16 entry points
# =====================================================================================================================================
@pytest.mark.parametrize("S", SELF_LENS)
@pytest.mark.parametrize("hd", HDS)
def test_probes_self(hd, S):
    """attention_fwd / attention_bwd, self-attention on the packed projection, at every key and query threshold, all four head dims"""
    probes(run_packed, S, S, hd)


@pytest.mark.parametrize("Sq,Skv", CROSS)
@pytest.mark.parametrize("hd", CROSS_HDS)
def test_probes_cross(hd, Sq, Skv):
    """attention_fwd_ex / attention_bwd_ex on strided views, query and key lengths on different sides of the thresholds"""
    probes(run_ex, Sq, Skv, hd)


@pytest.mark.parametrize("attn2", ["1", "0"])
@pytest.mark.parametrize("S", ATTN2_LENS)
def test_probes_attn2(S, attn2, monkeypatch):
    """head dim 48 at both edges of attention2's shape_ok (224 | 225, 260 | 261) and of its 9th key block (256 | 257 .. 260), with the
    32 x 32-block kernels on and off: the same lengths on the general kernels' 16- and 18-tile forms"""
    monkeypatch.setenv("MUSE_ATTN2", attn2)
    probes(run_ex, S, S, 48)


@pytest.mark.parametrize("S", CAUSAL_LENS)
@pytest.mark.parametrize("hd", CAUSAL_HDS)
def test_probes_causal(hd, S):
    """causal_attention_fwd: the diagonal (the mask edge), key 0 and the first key of the query's own tile bit for bit (the three maps
    alternate over the six heads), then every query aimed at the hidden key i + 1 against the float64 masked reference"""
    m = A.causal_maps(S)
    seen = torch.stack([m[("diagonal", "first", "tile")[i % 3]] for i in range(B * NH)]).reshape(B, NH, S)
    c = A.address_probe(B, S, S, NH, hd, seen, causal=True)
    A.check_address(c, run_causal(c), tag=f"causal address {S} hd{hd}")
    c = A.address_probe(B, S, S, NH, hd, m["masked"].expand(B, NH, S).contiguous(), causal=True)
    A.check_address(c, run_causal(c), tag=f"causal hidden target {S} hd{hd}")


# =====================================================================================================================================
# (b) the same probes on the bf16x3 kernels (f32 tensors: the probe values are their own hi planes, the lo planes are 0)
# =====================================================================================================================================
@pytest.mark.parametrize("stream", [True, False], ids=["stream", "pairs"])
@pytest.mark.parametrize("Skv", X3_SKV)
@pytest.mark.parametrize("Sq", X3_SQ)
def test_probes_x3(Sq, Skv, stream, monkeypatch):
    monkeypatch.setattr(_ops(), "X3_STREAM", stream)
    probes(run_x3, Sq, Skv, 64, bf16_out=False)


# =====================================================================================================================================
# (c) seeded N(0, 1) inputs per element over the terms
# =====================================================================================================================================
@pytest.mark.parametrize("S", SELF_LENS)
@pytest.mark.parametrize("hd", HDS)
def test_random_self(hd, S):
    randoms(run_packed, S, S, hd)


@pytest.mark.parametrize("Sq,Skv", CROSS)
@pytest.mark.parametrize("hd", CROSS_HDS)
def test_random_cross(hd, Sq, Skv):
    randoms(run_ex, Sq, Skv, hd)


@pytest.mark.parametrize("attn2", ["1", "0"])
@pytest.mark.parametrize("S", ATTN2_LENS)
def test_random_attn2(S, attn2, monkeypatch):
    monkeypatch.setenv("MUSE_ATTN2", attn2)
    c, ref = random_case(S, S, 48)
    A.check_random(c, run_ex(c), ref, e_ref_for(S, S), tag=f"random {S}x{S} hd48 MUSE_ATTN2={attn2}", report=REPORT.setdefault("attn2=" + attn2, {}))


@pytest.mark.parametrize("S", CAUSAL_LENS)
@pytest.mark.parametrize("hd", CAUSAL_HDS)
def test_random_causal(hd, S):
    c, ref = random_case(S, S, hd, True)
    A.check_random(c, run_causal(c), ref, dict(ctx=E_REF["causal_ctx"][0]), tag=f"random causal {S} hd{hd}", report=REPORT.setdefault("causal", {}))


# =====================================================================================================================================
# (d) poisoned surroundings
# =====================================================================================================================================
GAP, PADC, SENTINEL = 3, 8, 7.0


def _gapped(rows, S, H, fill):
    """[B * S, H] -> ([GAP + B (S + GAP), H + PADC] bf16 device buffer filled with `fill`, the images' rows S + GAP apart and GAP rows in)"""
    buf = torch.full((GAP + B * (S + GAP), H + PADC), fill, dtype=BF)
    if rows is not None:
        buf[GAP:].view(B, S + GAP, H + PADC)[:, :S, :H] = rows.to(BF).view(B, S, H)
    return buf.to(DEV)


def _data(buf, S, H):
    return buf[GAP:].view(B, S + GAP, H + PADC)[:, :S, :H]


@pytest.mark.parametrize("S,hd,attn2", POISON)
def test_poisoned_surroundings(S, hd, attn2, monkeypatch):
    """q, k, v and dO laid out with NaN in the rows between (and before) the images and in the feature columns behind H, ctx / dq / dk / dv
    views with the same gaps prefilled with a sentinel; the batch strides go on the descriptor of the C entry points.  The results
    equal the gap-free run bit for bit and no sentinel is touched: nothing is read or written outside an image's own S x H block."""
    ops = _ops()
    if attn2 is not None:
        monkeypatch.setenv("MUSE_ATTN2", attn2)
    c, _ = random_case(S, S, hd)
    H, al, ld = NH * hd, c["alpha"], NH * hd + PADC
    clean = run_ex(c)
    nan = float("nan")
    q, k, v, do = (_gapped(c[n], S, H, nan) for n in ("q", "k", "v", "do"))
    ctx, dq, dk, dv = (_gapped(None, S, H, SENTINEL) for _ in range(4))
    lse = torch.empty((B * NH, ops.lib().muse_attention_seq_pad(S)), dtype=F32, device=DEV)
    dsum = torch.empty_like(lse)
    view = lambda t: t[GAP:, :H]
    d = ops._attn_desc(view(q), view(k), view(v), view(ctx), B, S, S, NH, hd, al)
    bs = (S + GAP) * ld
    d.bsq = d.bsk = d.bsv = d.bso = bs
    ops.check(ops.lib().muse_attention_fwd_ex(C.byref(d), lse.data_ptr(), ops.stream()), "muse_attention_fwd_ex")
    ops.check(ops.lib().muse_attention_bwd_ex(C.byref(d), view(do).data_ptr(), ld, bs, lse.data_ptr(), dsum.data_ptr(), view(dq).data_ptr(), ld, bs,
                                              view(dk).data_ptr(), ld, bs, view(dv).data_ptr(), ld, bs, ops.stream()), "muse_attention_bwd_ex")
    torch.cuda.synchronize()
    assert torch.equal(lse[:, :S].cpu(), clean["lse"]), "lse differs from the gap-free run"
    for name, buf in (("ctx", ctx), ("dq", dq), ("dk", dk), ("dv", dv)):
        buf = buf.cpu()
        got = _data(buf, S, H).reshape(B * S, H)
        assert torch.equal(got, clean[name]), f"{name} differs from the gap-free run ({int((got != clean[name]).sum())} elements)"
        _data(buf, S, H).fill_(SENTINEL)
        assert bool((buf == SENTINEL).all()), f"{name}: {int((buf != SENTINEL).sum())} sentinel elements outside the images were overwritten"


def test_report():
    """(last in the file) the worst figures of this run per entry point and output kind, for profiles/attention_edges.md"""
    for ep, kinds in REPORT.items():
        for n, vals in kinds.items():
            print(f"[attention_edges] worst {ep} {n}: err={max(v[0] for v in vals):.3e} err/bound={max(v[1] for v in vals):.3f} over {len(vals)} cases")


# =====================================================================================================================================
# `python tests/test_gpu_attention_edges.py`: E_ref on a CPU, over the same case lists
# =====================================================================================================================================
def measure_e_ref():
    worst = {n: [0.0] * len(v) for n, v in E_REF.items()}
    where = {}

    def take(key, cls, val, shape):
        if val > worst[key][cls]:
            worst[key][cls], where[key, cls] = val, shape
    for Sq, Skv, hd in BF16_SHAPES:
        kc, qc = len_class(Skv), len_class(Sq)
        c, ref = random_case(Sq, Skv, hd)
        for n, e in A.model_errors(c, ref).items():
            take(n, qc if n in ("dk", "dv") else kc, e, (Sq, Skv, hd))
        c, ref = uniform_case(Sq, Skv, hd)
        take("uniform_dq", kc, A.model_errors(c, ref, ("dq",))["dq"], (Sq, Skv, hd))
        random_case.cache_clear()
        uniform_case.cache_clear()
    for hd in CAUSAL_HDS:
        for S in CAUSAL_LENS:
            c, ref = random_case(S, S, hd, True)
            take("causal_ctx", 0, A.model_errors(c, ref, ("ctx",))["ctx"], (S, S, hd))
    return worst, where


if __name__ == "__main__":
    t0 = time.time()
    worst, where = measure_e_ref()
    print("E_REF = {")
    for n in E_REF:
        vals = "(" + ", ".join(f"{v:.3e}" for v in worst[n]) + ("," if len(worst[n]) == 1 else "") + ")"
        print(f'    "{n}": {vals},'.ljust(56) + "# worst at Sq, Skv, hd = " + " ".join(str(where.get((n, i))).replace(" ", "") for i in range(len(worst[n]))))
    print("}")
    same = all(f"{w:.3e}" == f"{e:.3e}" for n in E_REF for w, e in zip(worst[n], E_REF[n]))
    print(f"{'matches' if same else 'DIFFERS FROM'} the table in this file ({time.time() - t0:.0f} s)")
