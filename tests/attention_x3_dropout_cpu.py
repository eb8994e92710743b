"""CPU restatement of the DROP instantiations of csrc/attention3.hip (muse_attention_x3_drop_fwd / _bwd: attention dropout inside the
bf16x3 / f16 attention cores), for tests/test_attention_x3_dropout_cpu.py and tests/test_gpu_attention_x3_dropout.py.  Imports without a
GPU; builds on attention_cpu (core3_model's products, layouts, check_random), attention_dropout_cpu (the float64 reference with a mask) and
philox_cpu (the dropout stream).

  * `keep_mask`: the mask contract with GLOBAL indices - the keep bit of (bh, q, k) is muse_dropout(seed, offset)'s bit of flat element
    (bh * S_q + q) * ld_mask + k of the full-sequence [B * nh, S_q, ld_mask] mask, ld_mask = round_up(S_kv, 8); `launches` lists the
    (q0, k0) of the kernel launches a shape takes (256-query blocks; 256-key blocks past 256 keys) and `launch_mask` is the slice a launch
    draws from its q0 / k0 / sq_total arguments;
  * `model_x3` / `model_h16`: attention_cpu.core3_model extended by the mask: row maximum, row sum and lse from the undropped P;
    P keep s in f32, then the product's operand conversion; dsum = S (dO . O) of the dropped context; dS = P (keep s prod(S dO, V^T) - dsum)
    in f32; dV from the dropped P;
  * defects (each must fail check_random at 4 * E_REF; tests/test_attention_x3_dropout_cpu.py):
      "local_q"      the mask drawn with the block-local instead of the global query index (every 256-query block repeats block 0's rows);
      "ld_skv"       ld_mask = S_kv instead of round_up(S_kv, 8);
      "no_scale"     the 1 / (1 - p) is missing;
      "lse_dropped"  row sum and lse taken from the dropped P.

`python tests/attention_x3_dropout_cpu.py` prints E_REF_X3_DROP / E_REF_H16_DROP per length class.
"""
import functools
import time

import numpy as np
import torch

import attention_cpu as A
import attention_dropout_cpu as D
import philox_cpu as PH

F32 = torch.float32
B, NH, HD = 2, 3, 64
SEED = 0x1234_5678_9ABC_DEF1
DROPS = ((0.5, 3 << 40), (0.1, 2 ** 32 - 5))      # (p, offset): the models' site offset of layer 1; the carry into the high counter word
SHAPES = [(256, 65), (256, 77), (256, 96), (256, 225), (256, 256), (512, 77), (512, 512), (256, 768)]
DEFECTS = ("local_q", "ld_skv", "no_scale", "lse_dropped")

# Worst error of model_x3 / model_h16 (with the mask) against float64 with the same mask over SHAPES x DROPS, per element over the terms
# (lse: absolute), per class of the summed length (test_gpu_attention_x3_edges.LEN_CLASSES) - as printed by
# `python tests/attention_x3_dropout_cpu.py`.  The GPU bound is 4 * E_REF.
LEN_CLASSES = (96, 256)             # n <= 96 | 97 .. 256 | >= 257      (dk / dv: by the queries, never <= 96)
E_REF_X3_DROP = {               # n <= 96, 97 .. 256, >= 257
    "ctx": (1.229e-05, 7.636e-06, 9.298e-06),           # worst at Sq, Skv, p = (512,77,0.5) (256,256,0.1) (512,512,0.1)
    "lse": (6.595e-06, 3.158e-06, 3.104e-06),           # worst at Sq, Skv, p = (512,77,0.5) (256,225,0.5) (512,512,0.5)
    "dq": (3.574e-05, 1.241e-05, 1.167e-05),            # worst at Sq, Skv, p = (512,77,0.5) (256,256,0.5) (512,512,0.5)
    "dk": (0.000e+00, 1.431e-05, 1.075e-05),            # worst at Sq, Skv, p = None (256,768,0.5) (512,512,0.5)
    "dv": (0.000e+00, 9.556e-06, 6.306e-06),            # worst at Sq, Skv, p = None (256,256,0.5) (512,512,0.1)
}
E_REF_H16_DROP = {
    "ctx": (2.586e-04, 1.734e-04, 1.278e-04),           # worst at Sq, Skv, p = (256,96,0.5) (256,256,0.5) (512,512,0.5)
    "lse": (4.763e-07, 4.704e-07, 6.097e-07),           # worst at Sq, Skv, p = (512,77,0.5) (256,225,0.5) (256,768,0.5)
    "dq": (3.437e-04, 2.462e-04, 2.266e-04),            # worst at Sq, Skv, p = (256,77,0.5) (256,225,0.5) (512,512,0.5)
    "dk": (0.000e+00, 2.265e-04, 1.730e-04),            # worst at Sq, Skv, p = None (256,768,0.5) (512,512,0.5)
    "dv": (0.000e+00, 2.232e-04, 1.780e-04),            # worst at Sq, Skv, p = None (256,768,0.5) (512,512,0.1)
}
TABLES = {"x3": E_REF_X3_DROP, "h16": E_REF_H16_DROP}


def len_class(n):
    return sum(n > t for t in LEN_CLASSES)


def e_ref_for(mode, Sq, Skv):
    kc, qc = len_class(Skv), len_class(Sq)
    return {n: v[qc if n in ("dk", "dv") else kc] for n, v in TABLES[mode].items()}


def launches(Sq, Skv):
    """[(q0, k0, keys)] of the one-tile launches of a shape: 256-query blocks, key blocks of 256 past 256 keys"""
    kb = [(k0, 256) for k0 in range(0, Skv, 256)] if Skv > 256 else [(0, Skv)]
    return [(q0, k0, n) for q0 in range(0, Sq, 256) for k0, n in kb]


def keep_mask(Sq, Skv, p, offset, defect=None, seed=SEED):
    """bool [B, NH, Sq, Skv]: the full-sequence mask (defects "local_q" / "ld_skv": what a kernel with that mistake would draw)"""
    ld = Skv if defect == "ld_skv" else D.row_pitch(Skv)
    flat = PH.dropout_keep(B * NH * Sq * ld, p, seed, offset)
    qi = np.arange(Sq) % 256 if defect == "local_q" else np.arange(Sq)
    e = ((np.arange(B * NH)[:, None, None] * Sq + qi[None, :, None]) * ld + np.arange(Skv)[None, None, :])
    return torch.from_numpy(flat[e].reshape(B, NH, Sq, Skv))


def launch_mask(Sq, Skv, p, offset, q0, k0, keys, seed=SEED):
    """bool [B, NH, 256, keys]: what the launch (q0, k0) draws from its arguments (ld_mask, q0, k0, sq_total = Sq) - element by element"""
    ld = D.row_pitch(Skv)
    bh, q, k = np.arange(B * NH)[:, None, None], np.arange(256)[None, :, None], np.arange(keys)[None, None, :]
    e = (bh * Sq + q0 + q) * ld + k0 + k
    blocks = np.unique(e >> 2)
    lo = int(blocks.min())
    u = PH.dropout_uniforms(4 * (int(blocks.max()) - lo + 1), seed, offset + lo)
    return torch.from_numpy((u[e - 4 * lo] >= np.float32(p)).reshape(B, NH, 256, keys))


@functools.lru_cache(maxsize=None)
def random_case(Sq, Skv, mode):
    """one seeded case per shape and mode, shared (never modified): plain f32 N(0, 1) for bf16x3 (both planes in use), exact in bf16 and
    half for H16 (core3_model asserts it)"""
    return A.random_case(B, Sq, Skv, NH, HD, 300000 + 131 * Sq + 17 * Skv, rnd=A.bf_half if mode == "h16" else None)


def core3_drop_model(c, prod, keep, p, S=1.0, defect=None, ctx_bwd=None):
    """attention_cpu.core3_model with the keep mask (module docstring).  keep: bool [B, nh, Sq, Skv]"""
    assert defect is None or defect in DEFECTS
    q, k, v, do = A._operands(c, F32)
    if prod is A.prod_h16:
        A.assert_bf16_exact(q=q, k=k, v=v)
        A.assert_half_exact(q=q, k=k, v=v, do_scaled=do * S)
    Bc, Sq, nh, hd = c["B"], c["Sq"], c["nh"], c["hd"]
    a = float(c["alpha"])
    m = keep.to(F32) * np.float32(1.0 if defect == "no_scale" else D.drop_scale(p))
    s = prod(q, k.transpose(-1, -2))
    mx = s.amax(-1, keepdim=True)
    pe = torch.exp((s - mx) * a)
    pd = pe * m
    l = (pd if defect == "lse_dropped" else pe).sum(-1, keepdim=True)
    ctx = prod(pd, v) / l
    lse = mx * a + torch.log(l)
    o = ctx if ctx_bwd is None else A.to_heads(ctx_bwd.to(F32), Bc, Sq, nh, hd)
    dos = do * S
    dsum = (do * o).sum(-1, keepdim=True) * S
    pb = torch.exp(s * a - lse)
    ds = pb * (m * prod(dos, v.transpose(-1, -2)) - dsum)
    dq, dk, dv = prod(ds, k) * (a / S), prod(ds.transpose(-1, -2), q) * (a / S), prod((pb * m).transpose(-1, -2), dos) / S
    out = {n: A.to_rows(t) for n, t in dict(ctx=ctx, dq=dq, dk=dk, dv=dv).items()}
    out["lse"] = lse.reshape(Bc * nh, Sq)
    return out


def model_x3(c, keep, p, defect=None, ctx_bwd=None):
    return core3_drop_model(c, A.prod_x3, keep, p, 1.0, defect, ctx_bwd)


def model_h16(c, keep, p, S=1.0, defect=None, ctx_bwd=None):
    return core3_drop_model(c, A.prod_h16, keep, p, S, defect, ctx_bwd)


MODELS = {"x3": model_x3, "h16": model_h16}


def model_errors(c, keep, p, ref, mode):
    m = MODELS[mode](c, keep, p)
    return {n: A.measure(m[n], ref[n], 1.0 if n == "lse" else ref["t_" + n]) for n in A.KINDS}


def measure_e_ref(shapes=SHAPES):
    worst = {mode: {n: [0.0] * 3 for n in A.KINDS} for mode in TABLES}
    where = {}
    for Sq, Skv in shapes:
        kc, qc = len_class(Skv), len_class(Sq)
        for p, off in DROPS:
            keep = keep_mask(Sq, Skv, p, off)
            for mode in TABLES:
                c = random_case(Sq, Skv, mode)
                for n, e in model_errors(c, keep, p, D.reference(c, keep, p), mode).items():
                    cls = qc if n in ("dk", "dv") else kc
                    if e > worst[mode][n][cls]:
                        worst[mode][n][cls], where[mode, n, cls] = e, (Sq, Skv, p)
    return worst, where


if __name__ == "__main__":
    t0 = time.time()
    worst, where = measure_e_ref()
    same = True
    for mode, name in (("x3", "E_REF_X3_DROP"), ("h16", "E_REF_H16_DROP")):
        print(name + " = {")
        for n in A.KINDS:
            vals = "(" + ", ".join(f"{v:.3e}" for v in worst[mode][n]) + ")"
            print(f'    "{n}": {vals},'.ljust(56) + "# worst at Sq, Skv, p = " + " ".join(str(where.get((mode, n, i))).replace(" ", "") for i in range(3)))
            same = same and all(f"{w:.3e}" == f"{e:.3e}" for w, e in zip(worst[mode][n], TABLES[mode][n]))
        print("}")
    print(f"{'matches' if same else 'DIFFERS FROM'} the tables in this file ({time.time() - t0:.0f} s)")
