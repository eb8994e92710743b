"""CPU side of tests/test_gpu_objective_edges.py: the case lists, float64 references, restatements and checkers for the kernels that make
a training step's inputs and its soft-target loss (muse_soft_ce_fwd / _bwd, muse_mask_sample, muse_mask_tokens, muse_cond_dropout).

Nothing here needs a GPU.  Every checker takes the outputs of *an implementation* - the HIP kernels in the GPU file, a float32 torch model
of the kernels' documented form here - so that tests/test_objective_cpu.py can hand the same checkers deliberately wrong models and
require each to fail (the proof that the GPU assertions can fail).

Soft-target cross entropy (include/muse_hip.h, muse_soft_ce_fwd): logits f32 [B * S1, ld], labels [B * S1], soft [B * S, K] with
S1 = S + 1.  Row (b, s) is active iff s >= 1 and labels != -100; its soft row is b * S + s - 1.  Forward: lse, psum = sum(p),
row_loss = psum * lse - sum(p * l) per active row (0 on inactive ones), loss = sum(row_loss) / n_active.  Backward:
g / n_active * (exp(l - lse) * psum - p) on [active rows, :K], exact +0 on every other element of [rows, ldo].

Mask sampling: position j is masked iff argsort(noise)[j] < k - the argsort ARRAY is thresholded, not the rank - with
k = max(round_half_even(S * p), 1) and ties in the noise broken by position (a stable sort).  oracle/maskgit_oracle.py is the reference;
its argsort is not stable, so the restatements below sort with stable=True and are proven equal to the oracle on tie-free input.
"""
import math
import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:                      # pytest's conftest.py has done this; `python tests/test_gpu_objective_edges.py` has not
    sys.path.insert(0, _ROOT)
from oracle import maskgit_oracle as O         # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TINY = 2.0 ** -102          # absolute floor of every normaliser (tests/test_gpu_row_edges.py)
BF16_SUB = 2.0 ** -133      # spacing of bf16 subnormals
GOUT = 1.75                 # the incoming scalar gradient of every soft-CE case
SENTINEL = 7.0              # what an output buffer holds before a kernel runs
MASK_RTOL = 3e-7            # mask_prob / loss weight: the bar of tests/test_gpu_sampling.py


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf16_ulp(ref):
    return (ref.abs() * 2.0 ** -8).clamp(min=BF16_SUB)


def bits(t):
    """integer view: NaN payloads and the sign of zero take part in torch.equal"""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


# =====================================================================================================================================
# soft-target cross entropy: cases
# =====================================================================================================================================
SOFT_KINDS = ["normalised", "sum_half", "sum_two", "all_zero", "one_hot"]
LOGIT_KINDS = ["n02", "spread60", "constant", "offset30"]


def _soft_row(kind, K, g):
    p = torch.softmax(torch.randn(K, generator=g) * 1.5, -1)
    if kind == "sum_half":
        return p * 0.5
    if kind == "sum_two":
        return p * 2.0
    if kind == "all_zero":
        return torch.zeros(K)
    if kind == "one_hot":
        return torch.nn.functional.one_hot(torch.randint(0, K, (1,), generator=g)[0], K).float()
    return p


def _logit_row(kind, K, g, r):
    if kind == "spread60":          # exp(l - max) reaches e^-60: nothing of the small end is left in the f32 sum
        return torch.linspace(-30.0, 30.0, K)[torch.randperm(K, generator=g)] if K > 1 else torch.tensor([30.0])
    if kind == "constant":
        return torch.full((K,), 1.5)
    if kind == "offset30":
        return ((30.0 if r % 2 == 0 else -30.0) + 0.5 * torch.randn(K, generator=g)).clamp(-32.0, 32.0)
    return (2.0 * torch.randn(K, generator=g)).clamp(-32.0, 32.0)


def soft_ce_case(name, B, S1, K, ld, ldo, *, out=F32, in_off=0, out_off=0, labels="mixed", seed=0):
    """One case.  Soft row q is of kind SOFT_KINDS[q % 5] and the logits row that reads it of kind LOGIT_KINDS[(q // 5) % 4], so 20 soft
    rows hold every combination.  labels "mixed": about 40 % of the positions -100; position 0 carries -100 in even images and a real
    label (7) in odd ones - inactive either way; from three images on, image 1 has no active row and image 2 exactly one; (0, 1) is
    always active.  in_off / out_off: floats / output elements by which the logits / dlogits base is moved off its 16-byte boundary."""
    g = gen(1000 + seed)
    S, rows = S1 - 1, B * S1
    soft = torch.stack([_soft_row(SOFT_KINDS[q % 5], K, g) for q in range(B * S)])
    x = torch.zeros(rows, K)
    for r in range(rows):
        b, s = divmod(r, S1)
        q = max(b * S + s - 1, 0)
        x[r] = _logit_row(LOGIT_KINDS[(q // 5) % 4], K, g, r)
    assert float(x.abs().max()) <= 32.0
    lab = torch.randint(0, K, (B, S1), generator=g)
    if labels == "none_active":
        lab[:, 1:] = -100
        lab[:, 0] = 3
    else:
        lab[torch.rand(B, S1, generator=g) < 0.4] = -100
        lab[0::2, 0] = -100
        lab[1::2, 0] = 7
        lab[0, 1] = 1 % K
        if B >= 3:
            lab[1, 1:] = -100
            lab[2, 1:] = -100
            lab[2, S1 - 1] = 0
    return dict(name=name, B=B, S1=S1, K=K, ld=ld, ldo=ldo, out=out, in_off=in_off, out_off=out_off, x=x, soft=soft,
                labels=lab.reshape(-1).contiguous(), g=GOUT)


def soft_ce_branch(c):
    """the kernel instance muse_soft_ce_bwd's launcher picks for this case (the forward's is the same without the output terms): buffers
    are carved out of 16-byte aligned allocations, so only in_off / out_off / ld / ldo decide"""
    out_align = 16 if c["out"] == F32 else 8
    esz = 4 if c["out"] == F32 else 2
    vec = c["ld"] % 4 == 0 and c["ldo"] % 4 == 0 and c["in_off"] % 4 == 0 and (c["out_off"] * esz) % out_align == 0
    K = c["K"]
    if K == 1024:
        return "K1024 vector" if vec else "K1024 scalar"
    if K in (512, 256) and vec:
        return f"K{K} vector"
    return "generic"


def _both(cases):
    """every case with an f32 and with a bf16 gradient"""
    out = []
    for c in cases:
        out.append(c)
        d = dict(c)
        d.update(out=BF, name=c["name"] + "-bf16")
        out.append(d)
    return out


def soft_ce_branch_cases():
    cs, seed = [], 0
    for K in (1024, 512, 256):
        cs.append(soft_ce_case(f"K{K}-aligned", 5, 13, K, K + 8, K + 4, seed=seed)); seed += 1
    cs.append(soft_ce_case("K1024-odd-ld", 5, 13, 1024, 1027, 1027, seed=seed)); seed += 1
    cs.append(soft_ce_case("K1024-base-off-1", 5, 13, 1024, 1032, 1028, in_off=1, seed=seed)); seed += 1
    for K in (512, 256):
        cs.append(soft_ce_case(f"K{K}-odd-ld", 5, 13, K, K + 3, K + 4, seed=seed)); seed += 1
    for K in (1, 3, 63, 64, 65, 255, 257, 1000):
        cs.append(soft_ce_case(f"K{K}-generic", 5, 13, K, K + 3, K, seed=seed)); seed += 1
    return _both(cs)


ROW_TAILS = [(1, 2), (3, 3), (1, 5), (5, 13)]           # 2, 9, 5, 65 rows: a last block of 2, 1, 1, 1 waves
REDUCE_SHAPES = [(3, 341), (4, 256), (5, 205), (5, 257)]  # 1023, 1024, 1025, 1285 rows: the one-block reduce below, at and over 1024


def soft_ce_tail_cases():
    cs, seed = [], 40
    for B, S1 in ROW_TAILS:
        cs.append(soft_ce_case(f"rows{B * S1}-K256", B, S1, 256, 264, 260, seed=seed)); seed += 1
        cs.append(soft_ce_case(f"rows{B * S1}-K65", B, S1, 65, 67, 66, seed=seed)); seed += 1
    return _both(cs)


def soft_ce_reduce_cases():
    return [soft_ce_case(f"reduce-rows{B * S1}", B, S1, 64, 64, 64, seed=60 + i) for i, (B, S1) in enumerate(REDUCE_SHAPES)]


def soft_ce_width_cases():
    """ldo = K (no tail), K + 4, K + 260 (a second trip of the vector zero-fill), K + 1 / K + 3 (scalar route), ldo < ld and ldo > ld,
    and output pointers 8- / 2-byte (bf16) and 4-byte (f32) aligned"""
    cs, seed = [], 70
    for K in (1024, 512, 256, 64):
        for extra in (0, 4, 260, 1, 3):
            cs.append(soft_ce_case(f"K{K}-ldo+{extra}", 3, 3, K, K + 8, K + extra, seed=seed)); seed += 1
        cs.append(soft_ce_case(f"K{K}-ldo>ld", 3, 3, K, K, K + 260, seed=seed)); seed += 1
    cs = _both(cs)
    for K in (1024, 256):
        cs.append(soft_ce_case(f"K{K}-bf16-out-8B", 3, 3, K, K + 8, K + 4, out=BF, out_off=4, seed=seed)); seed += 1
        cs.append(soft_ce_case(f"K{K}-bf16-out-2B", 3, 3, K, K + 8, K + 4, out=BF, out_off=1, seed=seed)); seed += 1
        cs.append(soft_ce_case(f"K{K}-f32-out-4B", 3, 3, K, K + 8, K + 4, out=F32, out_off=1, seed=seed)); seed += 1
    return cs


def soft_ce_label_cases():
    return _both([soft_ce_case("none-active-K256", 3, 5, 256, 264, 260, labels="none_active", seed=90),
                  soft_ce_case("none-active-K65", 3, 5, 65, 67, 66, labels="none_active", seed=91)])


def soft_ce_all_cases():
    return soft_ce_branch_cases() + soft_ce_tail_cases() + soft_ce_reduce_cases() + soft_ce_width_cases() + soft_ce_label_cases()


# =====================================================================================================================================
# soft-target cross entropy: reference, model, checker
# =====================================================================================================================================
def soft_ce_rows(B, S1, labels):
    """-> active [rows] bool, srow [rows] (clamped to 0 where the row has none)"""
    r = torch.arange(B * S1)
    b, s = r // S1, r % S1
    return (s >= 1) & (labels != -100), (b * (S1 - 1) + s - 1).clamp(min=0)


def f64_reference(logits, labels, soft, S1, K, g):
    """float64 torch on the documented contract -> dict(loss, n, lse, psum, row_loss, row_mag [rows], grad, mag [rows, K], active).
    mag is the gradient's normaliser |g| / n * (softmax * psum + p) and row_mag the row loss's, psum |lse| + sum(p |l|): in both the
    two terms the kernel subtracts.  Works on any device."""
    rows = logits.shape[0]
    dev = logits.device
    x = logits[:, :K].double()
    r = torch.arange(rows, device=dev)
    s, b = r % S1, r // S1
    active = (s >= 1) & (labels != -100)
    srow = (b * (S1 - 1) + s - 1).clamp(min=0)
    p = soft.double()[srow]
    logp = torch.log_softmax(x, dim=-1)
    lse = torch.logsumexp(x, dim=-1)
    psum = p.sum(-1)
    row = -(p * logp).sum(-1)
    n = int(active.sum())
    z = torch.zeros((), dtype=F64, device=dev)
    loss = float(row[active].sum()) / n if n else float("nan")
    scale = g / n if n else 0.0
    grad = scale * (torch.exp(logp) * psum[:, None] - p)
    mag = abs(scale) * (torch.exp(logp) * psum[:, None] + p)
    grad[~active] = 0.0
    mag[~active] = 0.0
    row_mag = psum * lse.abs() + (p * x.abs()).sum(-1)
    return dict(loss=loss, n=n, lse=torch.where(active, lse, z), psum=torch.where(active, psum, z), row_loss=torch.where(active, row, z),
                row_mag=torch.where(active, row_mag, z), grad=grad, mag=mag, active=active)


def soft_ce_reference(c):
    return f64_reference(c["x"], c["labels"], c["soft"], c["S1"], c["K"], c["g"])


SOFT_CE_FAULTS = ["drop_last_column", "soft_row_off_by_one", "position0_active", "psum_one", "tail_unwritten", "divide_by_rows"]


def soft_ce_model(c, fault=None):
    """torch float32 evaluating the kernels' documented form, psum * lse - sum(p * l) and g / n * (exp(l - lse) * psum - p) - the
    baseline that defines E_REF - in the output layout of the kernels: dl is the whole [rows, ldo] block of a SENTINEL-filled buffer.
    `fault` seeds one classic defect (SOFT_CE_FAULTS)."""
    B, S1, K, ldo = c["B"], c["S1"], c["K"], c["ldo"]
    rows = B * S1
    x, lab = c["x"].float(), c["labels"]
    r = torch.arange(rows)
    b, s = r // S1, r % S1
    active = (lab != -100) if fault == "position0_active" else (s >= 1) & (lab != -100)
    srow = b * (S1 - 1) + s - (0 if fault == "soft_row_off_by_one" else 1)
    p = c["soft"].float()[srow.clamp(0, B * (S1 - 1) - 1)]
    if fault == "drop_last_column":
        x, p = x[:, :K - 1], p[:, :K - 1]
    lse = torch.logsumexp(x, -1) if x.shape[1] else torch.full((rows,), -math.inf)
    psum = torch.ones(rows) if fault == "psum_one" else p.sum(-1)
    row = psum * lse - (p * x).sum(-1)
    zero = torch.zeros(rows)
    n = int(active.sum())
    total = row[active].sum()
    loss = total / (rows if fault == "divide_by_rows" else n) if n else torch.tensor(float("nan"))
    dl = torch.full((rows, ldo), SENTINEL)
    if fault != "tail_unwritten":
        dl[:] = 0.0
    if n:
        gr = (c["g"] / n) * (torch.exp(x - lse[:, None]) * psum[:, None] - p)
        dl[:, :gr.shape[1]] = torch.where(active[:, None], gr, torch.zeros_like(gr))
        if fault == "drop_last_column":
            dl[:, K - 1] = 0.0
    return dict(loss_out=torch.stack([loss.float(), torch.tensor(float(n))]), lse=torch.where(active, lse, zero),
                psum=torch.where(active, psum, zero), row_loss=torch.where(active, row, zero), dl=dl.to(c["out"]))


def soft_ce_errors(c, out, ref=None):
    """normalised errors of one implementation's outputs, per kind (what E_REF is the maximum of, over the case lists)"""
    ref = soft_ce_reference(c) if ref is None else ref
    a = ref["active"]
    K = c["K"]
    E = {}
    if ref["n"]:
        E["soft_ce_loss"] = abs(float(out["loss_out"][0]) - ref["loss"]) / max(abs(ref["loss"]), TINY)
    d = lambda k: (out[k].double() - ref[k]).abs()   # noqa: E731
    E["soft_ce_lse"] = float((d("lse") / ref["lse"].abs().clamp(min=1.0)).max())
    E["soft_ce_psum"] = float((d("psum") / ref["psum"].abs().clamp(min=TINY)).max())
    E["soft_ce_row_loss"] = float((d("row_loss") / ref["row_mag"].clamp(min=TINY)).max())
    if out["dl"].dtype == F32 and bool(a.any()):
        E["soft_ce_grad"] = float(((out["dl"][:, :K].double() - ref["grad"]).abs() / (ref["mag"] + TINY))[a].max())
    return E


def soft_ce_check(c, out, e_ref, ref=None):
    """every assertion the GPU test makes on one case's outputs -> {kind: err / bound}.  out: loss_out [2], lse / psum / row_loss [rows],
    dl [rows, ldo] in the case's gradient dtype."""
    ref = soft_ce_reference(c) if ref is None else ref
    K, rows = c["K"], c["B"] * c["S1"]
    a = ref["active"]
    ratios = {}
    lo = out["loss_out"].double()
    assert float(lo[1]) == ref["n"], f"{c['name']}: n_active {float(lo[1])} != {ref['n']}"
    if ref["n"] == 0:
        assert math.isnan(float(lo[0])), f"{c['name']}: the loss of no active row is {float(lo[0])}, not NaN"
    for k in ("lse", "psum", "row_loss"):
        assert out[k].shape == (rows,)
        assert not bool(bits(out[k].float())[~a].any()), f"{c['name']}: {k} of an inactive row is not +0"
    for kind, err in soft_ce_errors(c, out, ref).items():
        if kind == "soft_ce_grad":
            continue
        ratios[kind] = err / (4.0 * e_ref[kind])
    dl = out["dl"]
    assert dl.dtype == c["out"] and dl.shape == (rows, c["ldo"])
    assert bool(torch.isfinite(dl.float()).all()), f"{c['name']}: NaN / inf in the gradient"
    inside = torch.zeros((rows, c["ldo"]), dtype=torch.bool)
    inside[:, :K] = a[:, None]
    assert not bool(bits(dl)[~inside].any()), f"{c['name']}: an element outside the active [rows, :K] block is not an exact +0"
    if bool(a.any()):
        dd = (dl[:, :K].double() - ref["grad"]).abs()
        bound = 4.0 * e_ref["soft_ce_grad"] * (ref["mag"] + TINY)
        if dl.dtype == BF:
            bound = bound + bf16_ulp(ref["grad"])
        ratios["soft_ce_grad" + ("_bf16" if dl.dtype == BF else "")] = float((dd / bound)[a].max())
    for kind, v in ratios.items():
        assert v <= 1.0, f"{c['name']}: {kind} is {v:.3f} x its bound"
    return ratios


def measure_soft_ce_e_ref(cases=None):
    E = {}
    for c in (soft_ce_all_cases() if cases is None else cases):
        for k, v in soft_ce_errors(c, soft_ce_model(dict(c, out=F32))).items():
            E[k] = max(E.get(k, 0.0), v)
    return E


# =====================================================================================================================================
# mask sampling: restatements, cases, checker
# =====================================================================================================================================
MASK_FAULTS = ["rank_threshold", "reverse_ties", "round_half_up", "no_clamp", "eval_clipped"]


def mask_count(S, prob, fault=None):
    x = S * prob
    k = torch.floor(x + 0.5) if fault == "round_half_up" else x.round()
    return k if fault == "no_clamp" else k.clamp(min=1)


def noise_mask(noise, k, fault=None):
    """mask[b, j] = argsort(noise[b], stable)[j] < k[b]"""
    if fault == "reverse_ties":
        S = noise.shape[-1]
        perm = S - 1 - noise.flip(-1).argsort(dim=-1, stable=True)
    else:
        perm = noise.argsort(dim=-1, stable=True)
    if fault == "rank_threshold":
        perm = perm.argsort(dim=-1, stable=True)
    return perm < k.unsqueeze(-1)


def mask_sample_ref(tokens, class_ids, timesteps, noise, mask_id, codebook, min_rate=0.0, fault=None):
    """oracle.prepare_inputs_and_labels with a stable argsort -> (input_ids [B, S + 1], labels [B, S + 1], mask_prob [B])"""
    S = tokens.shape[1]
    prob = O.cosine_schedule(timesteps).clip(min_rate)
    mask = noise_mask(noise, mask_count(S, prob, fault), fault)
    cls = (class_ids + codebook).unsqueeze(-1)
    ids = torch.cat([cls, torch.where(mask, mask_id, tokens)], -1)
    labels = torch.cat([torch.full_like(cls, -100), torch.where(mask, tokens, -100)], -1)
    return ids, labels, prob


def mask_tokens_ref(tokens, mask_id, min_rate, *, timesteps=None, mask_prob=None, noise=None, rects=None, all_labels=False, fault=None):
    """oracle.mask_or_random_replace_tokens with a stable argsort; a rectangle masks what the Python slice [y0:y0 + h, x0:x0 + w] does
    for non-negative origins (it may overhang the right and bottom border) -> (input_ids, labels, loss_weight or None, mask_prob)"""
    B, S = tokens.shape
    if mask_prob is None:
        mask_prob = O.cosine_schedule(timesteps).clip(min_rate)
    elif fault == "eval_clipped":
        mask_prob = mask_prob.clip(min_rate)
    if rects is None:
        mask = noise_mask(noise, mask_count(S, mask_prob, fault), fault)
    else:
        side = math.isqrt(S)
        y, x = torch.arange(S) // side, torch.arange(S) % side
        r = rects.long()
        mask = ((y >= r[:, 0:1]) & (y < r[:, 0:1] + r[:, 2:3]) & (x >= r[:, 1:2]) & (x < r[:, 1:2] + r[:, 3:4]))
    ids = torch.where(mask, mask_id, tokens)
    if all_labels:
        return ids, tokens, 1 - (1 - mask.long()) * ((1 - mask_prob) * (1 - 0.3))[:, None], mask_prob
    return ids, torch.where(mask, tokens, -100), None, mask_prob


def half_margin(S, timesteps, min_rate):
    """distance of S * p from the nearest half-integer, the smaller of the f32 and the float64 evaluation, per image"""
    m = []
    for dt in (F32, F64):
        x = (S * O.cosine_schedule(timesteps.to(dt)).clip(min_rate)).double()
        m.append(((x - 0.5) - (x - 0.5).round()).abs())
    return torch.minimum(*m)


def seeded_timesteps(B):
    return torch.rand(64, generator=gen(0))[:B]


def tie_free(B, S, seed):
    """uniform noise without ties: torch.rand has 24 bits, so 4096 draws collide about every other time; these are S distinct values in
    a random order per image"""
    order = torch.rand(B, S, generator=gen(seed), dtype=F64).argsort(-1)
    return ((order.double() + 0.25) / S).float()


def tie_noise(kind, B, S, k):
    """noise with ties: "equal" (mask = j < k), "four" distinct values, "pair" - a tie-free row whose k-th and (k + 1)-th smallest values
    are made equal, a duplicated pair straddling the threshold"""
    if kind == "equal":
        return torch.full((B, S), 0.25)
    if kind == "four":
        return torch.randint(0, 4, (B, S), generator=gen(S)).float() * 0.25
    nz = tie_free(B, S, S + 1)
    if S >= 2:
        order = nz.argsort(-1)
        for b in range(B):
            kk = min(max(int(k[b]), 1), S - 1)
            nz[b, order[b, kk]] = nz[b, order[b, kk - 1]]
    return nz


def _tokens(B, S, codebook, seed):
    return torch.randint(0, codebook, (B, S), generator=gen(seed))


MASK_SAMPLE_S = [1, 2, 255, 256, 257, 1023, 1024]
MASK_TOKENS_S = [1, 4, 255, 256, 257, 1024, 4095, 4096]
HALF_EVEN_S = [2, 6, 10, 14]        # t = 1 is clipped to min_masking_rate 0.25: S * 0.25 = 0.5, 1.5, 2.5, 3.5 -> k = 1, 2, 2, 4
HALF_EVEN_K = [1, 2, 2, 4]
CODEBOOK, MASK_ID = 1024, 2047


def mask_sample_cases(S_list=MASK_SAMPLE_S, B=3):
    """dicts of keyword arguments for mask_sample_ref / ops.mask_sample, with `ties` telling whether the oracle itself may be asked"""
    cs = []

    def add(name, S, t, noise, min_rate=0.0, ties=False, k=None):
        cs.append(dict(name=name, tokens=_tokens(t.numel(), S, CODEBOOK, S), class_ids=torch.arange(t.numel()) * 7 % 1000, timesteps=t,
                       noise=noise, mask_id=MASK_ID, codebook=CODEBOOK, min_rate=min_rate, ties=ties, k=k))

    for S in S_list:
        rnd = tie_free(B, S, S + 7)
        t = seeded_timesteps(B)
        add(f"S{S}-seeded", S, t, rnd)
        add(f"S{S}-t0", S, torch.zeros(B), rnd, k=[S] * B)                            # every position masked
        add(f"S{S}-t1-clamp", S, torch.ones(B), rnd, k=[1] * B)                       # cos = -4.4e-8 -> clip 0 -> k = 0 -> clamp 1
        k = mask_count(S, O.cosine_schedule(t))
        for kind in ("equal", "four", "pair"):
            add(f"S{S}-ties-{kind}", S, t, tie_noise(kind, B, S, k), ties=True)
    for S, k in zip(HALF_EVEN_S, HALF_EVEN_K):
        add(f"S{S}-half-even", S, torch.ones(B), tie_free(B, S, S + 9), min_rate=0.25, k=[k] * B)
        add(f"S{S}-half-even-equal", S, torch.ones(B), tie_noise("equal", B, S, None), min_rate=0.25, ties=True, k=[k] * B)
    return cs


def mask_tokens_cases(S_list=MASK_TOKENS_S, B=3):
    cs = []

    def add(name, S, ties=False, k=None, nb=B, **kw):
        kw.setdefault("min_rate", 0.0)
        kw.setdefault("all_labels", False)
        cs.append(dict(name=name, tokens=_tokens(nb, S, CODEBOOK, S + 1), mask_id=MASK_ID, ties=ties, k=k, kw=kw))

    for S in S_list:
        rnd = tie_free(B, S, S + 11)
        t = seeded_timesteps(B)
        add(f"S{S}-seeded", S, timesteps=t, noise=rnd)
        add(f"S{S}-seeded-all-labels", S, timesteps=t, noise=rnd, all_labels=True)
        add(f"S{S}-t0", S, timesteps=torch.zeros(B), noise=rnd, k=[S] * B)
        add(f"S{S}-t1-clamp", S, timesteps=torch.ones(B), noise=rnd, k=[1] * B)
        k = mask_count(S, O.cosine_schedule(t))
        for kind in ("equal", "four", "pair"):
            add(f"S{S}-ties-{kind}", S, ties=True, timesteps=t, noise=tie_noise(kind, B, S, k))
        if S >= 4:
            # exact halves through mask_prob: S * p = 0.5, 1.5, 2.5, 3.5 -> 0 (clamped to 1), 2, 2, 4; S a power of two or p * S exact
            halves = torch.tensor([0.5, 1.5, 2.5, 3.5])
            p = (halves.double() / S).float()
            if bool((p.double() * S == halves.double()).all()) and bool(((S * p) == halves).all()):
                add(f"S{S}-half-even", S, nb=4, k=[1, 2, 2, 4], mask_prob=p, noise=tie_free(4, S, S + 13))
                add(f"S{S}-half-even-equal", S, nb=4, ties=True, k=[1, 2, 2, 4], mask_prob=p, noise=tie_noise("equal", 4, S, None))
        # the eval branch is not clipped: p = 1 / 8 with min_masking_rate 0.5
        add(f"S{S}-eval-not-clipped", S, min_rate=0.5, mask_prob=torch.full((B,), 0.125), noise=rnd, all_labels=S % 2 == 0)
    return cs


def rect_cases():
    """side 1, 2, 16, 64: the whole grid, h = 0, one cell in each corner, an overhang over the right and bottom border; no negative
    origin (the oracle's slices wrap there, which is not the contract)"""
    cs = []
    for side in (1, 2, 16, 64):
        e = side - 1
        rects = torch.tensor([[0, 0, side, side], [0, 0, 0, side], [0, 0, 1, 1], [0, e, 1, 1], [e, 0, 1, 1], [e, e, 1, 1],
                              [side // 2, side // 2, side, side], [e, 0, 5, side + 3], [0, e, side + 1, 2]], dtype=torch.int32)
        nb = rects.shape[0]
        for all_labels in (False, True):
            cs.append(dict(name=f"rect-side{side}" + ("-all-labels" if all_labels else ""), tokens=_tokens(nb, side * side, CODEBOOK, side),
                           mask_id=MASK_ID, ties=False, k=None,
                           kw=dict(min_rate=0.1, timesteps=torch.rand(nb, generator=gen(side)), rects=rects, all_labels=all_labels)))
    return cs


def mask_check(name, got, want):
    """ids and labels equal; mask_prob and the loss weight within MASK_RTOL.  got / want: (ids, labels, [weight or None,] mask_prob)"""
    assert torch.equal(got[0], want[0]), f"{name}: input_ids differ at {int((got[0] != want[0]).sum())} positions"
    assert torch.equal(got[1], want[1]), f"{name}: labels differ at {int((got[1] != want[1]).sum())} positions"
    torch.testing.assert_close(got[-1].float(), want[-1].float(), rtol=MASK_RTOL, atol=0.0, msg=f"{name}: mask_prob")
    if len(want) == 4:
        assert (got[2] is None) == (want[2] is None), f"{name}: loss weight present / absent"
        if want[2] is not None:
            torch.testing.assert_close(got[2].float(), want[2].float(), rtol=MASK_RTOL, atol=0.0, msg=f"{name}: loss weight")


def mask_sample_args(c):
    return (c["tokens"], c["class_ids"], c["timesteps"], c["noise"], c["mask_id"], c["codebook"], c["min_rate"])


def mask_sample_check(c, got):
    """against the stable restatement and, where the noise has no ties, against the oracle itself; the count where the case names it;
    the class id at position 0"""
    mask_check(c["name"], got, mask_sample_ref(*mask_sample_args(c)))
    if not c["ties"]:
        mask_check(c["name"] + " (oracle)", got, O.prepare_inputs_and_labels(*mask_sample_args(c)))
    ids, labels = got[0], got[1]
    assert torch.equal(ids[:, 0], c["class_ids"] + c["codebook"]) and bool((labels[:, 0] == -100).all())
    masked = ids[:, 1:] == c["mask_id"]
    assert torch.equal(labels[:, 1:], torch.where(masked, c["tokens"], -100))
    if c["k"] is not None:
        assert masked.sum(-1).tolist() == list(c["k"]), (c["name"], masked.sum(-1).tolist(), c["k"])


def mask_tokens_check(c, got):
    kw = c["kw"]
    mask_check(c["name"], got, mask_tokens_ref(c["tokens"], c["mask_id"], **kw))
    if not c["ties"]:
        okw = dict(kw)
        mask_check(c["name"] + " (oracle)", got, O.mask_or_random_replace_tokens(c["tokens"], c["mask_id"], okw.pop("min_rate"), **okw))
    masked = got[0] == c["mask_id"]
    if c["k"] is not None:
        assert masked.sum(-1).tolist() == list(c["k"]), (c["name"], masked.sum(-1).tolist(), c["k"])


def margin_ok(c):
    """the condition on seeded timesteps: S * p is at least 1e-3 from a half-integer in f32 and in float64, for every image"""
    t = c["timesteps"] if "timesteps" in c else c["kw"].get("timesteps")
    if t is None or (c.get("kw") or {}).get("rects") is not None:
        return True
    min_rate = c["min_rate"] if "min_rate" in c else c["kw"]["min_rate"]
    S = c["tokens"].shape[1]
    exact = bool(((t == 0) | (t == 1)).all())            # t = 0 / 1 do not depend on the cosine's last ulp: 1 and the clip
    return exact or float(half_margin(S, t, min_rate).min()) >= 1e-3


# =====================================================================================================================================
# conditioning dropout
# =====================================================================================================================================
DROPOUT_FAULTS = ["u_le_p", "kept_zero_keeps_value"]
SPECIALS = [0.0, -0.0, float("nan"), float("inf"), 1e-42, 1.5]         # 1e-42 is an f32 subnormal: a flushed one would show
DROP_P = 0.625


def cond_dropout_model(x, empty, u, p, fault=None):
    """the kernel's statement: keep = u < p per image; out = (x * keep != 0) ? x : empty"""
    B = x.shape[0]
    keep = ((u <= p) if fault == "u_le_p" else (u < p)).reshape(B, *([1] * (x.dim() - 1))).float()
    nz = (x * keep) != 0
    if fault == "kept_zero_keeps_value":
        nz = nz | (keep.bool() & (x == 0))
    return torch.where(nz, x, empty.expand_as(x))


def cond_dropout_cases():
    """per_image 1 / 255 / 257 x B 1 / 3, twelve one-element images (every special kept and dropped), and 3 x 174763 = 524289 elements,
    one past the 2048-block grid.  Uniforms: u == p (dropped: the test is a strict <), the f32 just below p (kept), 0 and just under 1;
    plus p = 0 (all dropped) and p = 1 (all kept)."""
    p32 = torch.tensor(DROP_P)
    below = torch.nextafter(p32, torch.tensor(0.0))
    edge_u = torch.stack([p32, below, torch.tensor(0.0), torch.tensor(0.99999994), p32, below])
    cs = []
    for per, B in [(1, 1), (1, 3), (255, 1), (255, 3), (257, 1), (257, 3), (1, 12), (174763, 3)]:
        g = gen(per + B)
        x = torch.randn(B, per, generator=g)
        for b in range(B):
            for j in range(min(len(SPECIALS), per)):
                x[b, j] = SPECIALS[(j + b // 2) % len(SPECIALS)]
        empty = torch.randn(per, generator=g) + 3.0
        u = torch.stack([edge_u[(b + 1) % 6] for b in range(B)])      # image 0 kept (below p), image 1 u = 0 kept, image 3 dropped ...
        if B == 12:
            u = torch.stack([below if b % 2 == 0 else p32 for b in range(B)])
        for p in (DROP_P, 0.0, 1.0):
            cs.append(dict(name=f"per{per}-B{B}-p{p}", x=x, empty=empty, u=u, p=p))
        if B == 1:
            cs.append(dict(name=f"per{per}-B1-u==p", x=x, empty=empty, u=p32.reshape(1), p=DROP_P))
    return cs


def cond_dropout_check(c, got):
    want = O.cond_dropout(c["x"], c["empty"], c["u"], c["p"])
    assert got.shape == want.shape and got.dtype == F32
    assert torch.equal(bits(got), bits(want)), f"{c['name']}: {int((bits(got) != bits(want)).sum())} elements differ in bits"
