"""CPU restatement of attention with dropout on the probabilities drawn inside the fused kernels (csrc/attention.hip, the DROP
instantiations behind muse_attention_drop_fwd_ex / _bwd_ex), for tests/test_gpu_attention_dropout.py and
tests/test_attention_dropout_cpu.py.  Imports without a GPU; builds on attention_cpu (layouts, terms, check_random) and philox_cpu (the
dropout stream).

  * `keep_mask`: the mask contract - the keep bit of (bh, q, k) is muse_dropout(seed, offset)'s bit for flat element
    (bh * Sq + q) * ld_mask + k of a [B * nh, Sq, ld_mask] tensor, ld_mask = round_up(Skv, 8) unless given;
  * `reference`: float64 on the rounded inputs with a given keep mask (lse and the softmax from the undropped scores, O = (P keep s) V,
    dS = P (keep s dP - dsum), dV = (P keep s)^T dO; s = 1 / (1 - p) as an f32 number) and attention_cpu's per-element terms, the dropped
    mass in place of P;
  * `contract_model`: the same in float32 at the documented roundings: the row sum over bf16(P), bf16(P keep s) with ONE rounding of the
    f32 product into P V and into dV, dS rounded to bf16 once, the backward reads the bf16 context.  Its error against float64 is
    E_REF_DROP (below).  `o_bwd`, `scale` let the CPU test stand in for a kernel: the probes' zero context, the missing 1 / (1 - p);
  * mask read-back probes.  Softmax probabilities are strictly positive, so with one-hot operands "non-zero" reads one keep bit exactly:
      - `key_window_fwd` (k0): V[k, d] = 1 iff k == k0 + d, K one-hot the same way -> ctx[q, d] != 0 <=> keep(q, k0 + d);
      - `key_window_bwd`: the same Q, K with V[:, 0] = 1, dO = e_0 (dP = 1), context 0 (dsum = 0) -> dQ[q, d] != 0 <=> keep(q, k0 + d);
      - `query_window` (q0): Q[q, d] = 1 iff q == q0 + d, V[:, 0] = 1, dO = e_0, context 0 -> dK[k, d] != 0 <=> keep(q0 + d, k);
      - `query_window_dv`: Q, K random, dO[q, d] = 1 iff q == q0 + d -> dV[k, d] != 0 <=> keep(q0 + d, k);
    `check_key_window` / `check_query_window` compare EVERY (bh, row, column) with the mask and raise AssertionError.

`python tests/attention_dropout_cpu.py` prints E_REF_DROP.
"""
import functools
import time

import numpy as np
import torch

import attention_cpu as A
import philox_cpu as PH

F32, F64 = torch.float32, torch.float64
B, NH = 2, 2                    # two images, two heads: a wrong bh stride shows
PS = (0.5, 0.1)
OFFSETS = (3 << 40, 2 ** 32 - 5)     # the models' site offset of layer 1; the carry into the high counter word after 5 blocks
SEED = 0x1234_5678_9ABC_DEF1
# (Sq, Skv, hd): K = 16 tail | cross-attention with Sp = 80 != Skv | shared leftover tile, 4 waves, K = 32 + 16 | 18 key tiles, shared tile,
# 8 waves | the same at head dim 48 (never attention2.hip) | streamed keys | streamed queries
SHAPES = [(17, 17, 16), (33, 77, 64), (80, 80, 48), (257, 257, 64), (257, 257, 48), (129, 320, 64), (320, 129, 32)]

# Worst error of contract_model against reference over SHAPES x PS x OFFSETS, before the model's output rounding, per element over the
# terms (lse: absolute), per class of the length a result is summed over (tests/test_gpu_attention_edges.py: LEN_CLASSES) - as printed by
# `python tests/attention_dropout_cpu.py`.  The GPU bound is 4 * E_REF_DROP (+ one bf16 rounding).
LEN_CLASSES = (32, 288)         # n <= 32 | 33 .. 288 | >= 289
E_REF_DROP = {                  # n <= 32, 33 .. 288, >= 289
    "ctx": (2.611e-03, 1.906e-03, 1.123e-03),           # worst at Sq, Skv, hd, p = (17,17,16,0.5) (80,80,48,0.5) (129,320,64,0.5)
    "lse": (9.272e-04, 7.559e-04, 4.487e-04),           # worst at Sq, Skv, hd, p = (17,17,16,0.5) (80,80,48,0.5) (129,320,64,0.5)
    "dq": (4.495e-03, 3.152e-03, 1.647e-03),            # worst at Sq, Skv, hd, p = (17,17,16,0.5) (80,80,48,0.5) (129,320,64,0.5)
    "dk": (4.063e-03, 2.732e-03, 1.262e-03),            # worst at Sq, Skv, hd, p = (17,17,16,0.5) (80,80,48,0.5) (320,129,32,0.5)
    "dv": (3.379e-03, 3.267e-03, 1.144e-03),            # worst at Sq, Skv, hd, p = (17,17,16,0.5) (33,77,64,0.5) (320,129,32,0.5)
}


def len_class(n):
    return sum(n > t for t in LEN_CLASSES)


def e_ref_for(Sq, Skv):
    """kind -> E_REF_DROP of a case: by the keys for ctx, lse, dq, by the queries for dk, dv"""
    kc, qc = len_class(Skv), len_class(Sq)
    return dict(ctx=E_REF_DROP["ctx"][kc], lse=E_REF_DROP["lse"][kc], dq=E_REF_DROP["dq"][kc], dk=E_REF_DROP["dk"][qc], dv=E_REF_DROP["dv"][qc])


def row_pitch(Skv):
    """the materialised route's row pitch: what the models pass as ld_mask"""
    return (Skv + 7) // 8 * 8


def drop_scale(p):
    """1 / (1 - p) in f32, as a python float"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(nb, nh, Sq, Skv, p, seed, offset, ld_mask=None):
    """bool [nb, nh, Sq, Skv]"""
    ld = row_pitch(Skv) if ld_mask is None else ld_mask
    assert ld >= Skv
    keep = PH.dropout_keep(nb * nh * Sq * ld, p, seed, offset)
    return torch.from_numpy(keep.reshape(nb, nh, Sq, ld)[..., :Skv].copy())


def _seed(Sq, Skv, hd):
    return 200000 + 131 * Sq + 17 * Skv + hd


@functools.lru_cache(maxsize=None)
def random_case(Sq, Skv, hd):
    """one seeded N(0, 1) case per shape, shared (never modified)"""
    return A.random_case(B, Sq, Skv, NH, hd, _seed(Sq, Skv, hd))


@functools.lru_cache(maxsize=None)
def case_keep(Sq, Skv, p, offset):
    return keep_mask(B, NH, Sq, Skv, p, SEED, offset)


@functools.lru_cache(maxsize=None)
def case_reference(Sq, Skv, hd, p, offset):
    return reference(random_case(Sq, Skv, hd), case_keep(Sq, Skv, p, offset), p)


def reference(c, keep, p):
    """float64 -> dict of row tensors ctx, lse, dq, dk, dv and the normalisers t_ctx, t_dq, t_dk, t_dv (attention_cpu.reference's keys)"""
    q, k, v, do = A._operands(c, F64)
    a, s = float(c["alpha"]), drop_scale(p)
    sc = (q @ k.transpose(-1, -2)) * a
    lse = torch.logsumexp(sc, -1)
    pr = torch.exp(sc - lse[..., None])
    m = keep.to(F64) * s
    pd = pr * m
    ctx = pd @ v
    dpe = m * (do @ v.transpose(-1, -2))
    dsum = (do * ctx).sum(-1, keepdim=True)
    ds = pr * (dpe - dsum)
    w = pr * (dpe.abs() + dsum.abs())
    out = dict(ctx=ctx, dq=a * (ds @ k), dk=a * (ds.transpose(-1, -2) @ q), dv=pd.transpose(-1, -2) @ do,
               t_ctx=pd @ v.abs(), t_dq=a * (w @ k.abs()), t_dk=a * (w.transpose(-1, -2) @ q.abs()), t_dv=pd.transpose(-1, -2) @ do.abs())
    out = {n: A.to_rows(t) for n, t in out.items()}
    for n in ("t_ctx", "t_dq", "t_dk", "t_dv"):
        out[n] = out[n].clamp(min=A.TINY)
    out["lse"] = lse.reshape(c["B"] * c["nh"], c["Sq"])
    return out


def contract_model(c, keep, p, scale=None, o_bwd=None):
    """float32 at the documented roundings (module docstring) -> ctx, lse, dq, dk, dv before the output rounding.  scale: in place of
    1 / (1 - p); o_bwd: the context the backward reads ([B * Sq, H] rows) in place of the forward's own, rounded to bf16."""
    q, k, v, do = A._operands(c, F32)
    A.assert_bf16_exact(q=q, k=k, v=v, do=do)
    a = float(c["alpha"])
    m = keep.to(F32) * np.float32(drop_scale(p) if scale is None else scale)
    sc = (q @ k.transpose(-1, -2)) * a
    mx = sc.amax(-1, keepdim=True)
    pe = torch.exp(sc - mx)
    l = A.bf(pe).sum(-1, keepdim=True)
    ctx = (A.bf(pe * m) @ v) / l
    lse = mx + torch.log(l)
    o = A.bf(ctx) if o_bwd is None else A.to_heads(o_bwd.to(F32), c["B"], c["Sq"], c["nh"], c["hd"])
    pr = torch.exp(sc - lse)
    dv = A.bf(pr * m).transpose(-1, -2) @ do
    dsb = A.bf(pr * (m * (do @ v.transpose(-1, -2)) - (do * o).sum(-1, keepdim=True)))
    out = {n: A.to_rows(t) for n, t in dict(ctx=ctx, dq=a * (dsb @ k), dk=a * (dsb.transpose(-1, -2) @ q), dv=dv).items()}
    out["lse"] = lse.reshape(c["B"] * c["nh"], c["Sq"])
    return out


def model_errors(c, keep, p, ref):
    m = contract_model(c, keep, p)
    return {n: A.measure(m[n], ref[n], 1.0 if n == "lse" else ref["t_" + n]) for n in A.KINDS}


# =====================================================================================================================================
# mask read-back probes
# =====================================================================================================================================
def windows(n, hd):
    return list(range(0, n, hd))


def _onehot_rows(nb, S, nh, hd, w0):
    """[nb * S, nh * hd]: row s of every head holds a 1 in column s - w0 (where that is a column)"""
    t = torch.zeros((nb, nh, S, hd))
    for d in range(min(hd, S - w0)):
        t[:, :, w0 + d, d] = 1.0
    return A.to_rows(t)


def _e0_rows(nb, S, nh, hd):
    """[nb * S, nh * hd]: a 1 in column 0 of every head of every row"""
    t = torch.zeros((nb, nh, S, hd))
    t[..., 0] = 1.0
    return A.to_rows(t)


def key_window_fwd(c, k0):
    """forward probe of key window k0 (its lse also serves key_window_bwd)"""
    Bc, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    oh = _onehot_rows(Bc, Skv, nh, hd, k0)
    return A.make_case(Bc, Sq, Skv, nh, hd, c["q"], oh, oh.clone(), torch.zeros_like(c["q"]), alpha=c["alpha"], window=k0)


def key_window_bwd(c, k0):
    """dQ probe of key window k0: run with the lse of key_window_fwd's forward and an all-zero context"""
    Bc, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    return A.make_case(Bc, Sq, Skv, nh, hd, c["q"], _onehot_rows(Bc, Skv, nh, hd, k0), _e0_rows(Bc, Skv, nh, hd), _e0_rows(Bc, Sq, nh, hd),
                       alpha=c["alpha"], window=k0)


def query_window(c, q0):
    """dK probe of query window q0 (forward for the lse, backward with an all-zero context)"""
    Bc, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    return A.make_case(Bc, Sq, Skv, nh, hd, _onehot_rows(Bc, Sq, nh, hd, q0), c["k"], _e0_rows(Bc, Skv, nh, hd), _e0_rows(Bc, Sq, nh, hd),
                       alpha=c["alpha"], window=q0)


def query_window_dv(c, q0):
    """dV probe of query window q0"""
    Bc, Sq, Skv, nh, hd = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"]
    return A.make_case(Bc, Sq, Skv, nh, hd, c["q"], c["k"], c["v"], _onehot_rows(Bc, Sq, nh, hd, q0), alpha=c["alpha"], window=q0)


def _compare(got, want, tag, what):
    got = got != 0
    bad = got != want
    if bool(bad.any()):
        b, h, r, d = (int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} keep bits differ from the Philox stream; first at image {b} head {h} "
                             f"row {r} column {d}: the kernel {'kept' if bool(got[b, h, r, d]) else 'dropped'} {what(r, d)}")


def check_key_window(c, rows, keep, tag):
    """rows: ctx or dq [B * Sq, H] of a key-window probe: element (q, d) is non-zero iff keep(q, k0 + d) (columns past the last key: zero)"""
    Bc, Sq, Skv, nh, hd, k0 = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"], c["window"]
    want = torch.zeros((Bc, nh, Sq, hd), dtype=torch.bool)
    n = min(hd, Skv - k0)
    want[..., :n] = keep[..., k0:k0 + n]
    _compare(A.to_heads(rows.float().cpu(), Bc, Sq, nh, hd), want, f"{tag} key window {k0}", lambda r, d: f"(query {r}, key {k0 + d})")


def check_query_window(c, rows, keep, tag):
    """rows: dk or dv [B * Skv, H] of a query-window probe: element (k, d) is non-zero iff keep(q0 + d, k)"""
    Bc, Sq, Skv, nh, hd, q0 = c["B"], c["Sq"], c["Skv"], c["nh"], c["hd"], c["window"]
    want = torch.zeros((Bc, nh, Skv, hd), dtype=torch.bool)
    n = min(hd, Sq - q0)
    want[..., :n] = keep[:, :, q0:q0 + n, :].transpose(-1, -2)
    _compare(A.to_heads(rows.float().cpu(), Bc, Skv, nh, hd), want, f"{tag} query window {q0}", lambda r, d: f"(query {q0 + d}, key {r})")


def run_probes(c, keep, fwd, bwd, tag):
    """every keep bit of every (bh, q, k) through all three kernels.  fwd(case) -> dict(ctx, lse) and bwd(case, ctx, lse) -> dict(dq, dk, dv)
    run the code under test; ctx / lse pass through opaquely (the probes hand bwd an all-zero context)"""
    zero = lambda t: torch.zeros_like(t)   # noqa: E731
    for k0 in windows(c["Skv"], c["hd"]):
        cf = key_window_fwd(c, k0)
        f = fwd(cf)
        check_key_window(cf, f["ctx"], keep, tag + " forward")
        cb = key_window_bwd(c, k0)
        check_key_window(cb, bwd(cb, zero(f["ctx"]), f["lse"])["dq"], keep, tag + " dQ")
    for q0 in windows(c["Sq"], c["hd"]):
        cq = query_window(c, q0)
        f = fwd(cq)
        check_query_window(cq, bwd(cq, zero(f["ctx"]), f["lse"])["dk"], keep, tag + " dK")
        cv = query_window_dv(c, q0)
        f = fwd(cv)
        check_query_window(cv, bwd(cv, f["ctx"], f["lse"])["dv"], keep, tag + " dV")


def model_runner(keep, p, scale=None):
    """(fwd, bwd) for run_probes / check_random that stand in for the kernels: contract_model with the mask `keep`"""
    def fwd(c):
        m = contract_model(c, keep, p, scale=scale)
        return dict(ctx=m["ctx"].to(A.BF), lse=m["lse"])

    def bwd(c, ctx, lse):
        m = contract_model(c, keep, p, scale=scale, o_bwd=ctx)
        return {n: m[n].to(A.BF) for n in ("dq", "dk", "dv")}
    return fwd, bwd


# =====================================================================================================================================
# `python tests/attention_dropout_cpu.py`: E_REF_DROP
# =====================================================================================================================================
def measure_e_ref():
    worst = {n: [0.0] * len(v) for n, v in E_REF_DROP.items()}
    where = {}
    for Sq, Skv, hd in SHAPES:
        kc, qc = len_class(Skv), len_class(Sq)
        c = random_case(Sq, Skv, hd)
        for p in PS:
            for off in OFFSETS:
                keep = case_keep(Sq, Skv, p, off)
                for n, e in model_errors(c, keep, p, case_reference(Sq, Skv, hd, p, off)).items():
                    cls = qc if n in ("dk", "dv") else kc
                    if e > worst[n][cls]:
                        worst[n][cls], where[n, cls] = e, (Sq, Skv, hd, p)
    return worst, where


if __name__ == "__main__":
    t0 = time.time()
    worst, where = measure_e_ref()
    print("E_REF_DROP = {")
    for n in E_REF_DROP:
        vals = "(" + ", ".join(f"{v:.3e}" for v in worst[n]) + ")"
        print(f'    "{n}": {vals},'.ljust(56) + "# worst at Sq, Skv, hd, p = " + " ".join(str(where.get((n, i))).replace(" ", "") for i in range(len(worst[n]))))
    print("}")
    same = all(f"{w:.3e}" == f"{e:.3e}" for n in E_REF_DROP for w, e in zip(worst[n], E_REF_DROP[n]))
    print(f"{'matches' if same else 'DIFFERS FROM'} the table in this file ({time.time() - t0:.0f} s)")
