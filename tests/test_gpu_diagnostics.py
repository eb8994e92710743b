"""GPU (-m gpu): the masked-token logging diagnostics of muse.training_utils on their kernel path (csrc/diag.hip: muse_token_stats,
muse_masked_row_mean, muse_masked_mean_probs; the per-token cross-entropy is muse_cross_entropy_fwd's row_loss).

Expected values come from three sources, none of them the code under test: the reference module's own results in
tests/golden/training_utils.npz, this module's unchanged CPU path (tests/test_surface.py shows it equals the reference bit for bit), and
a float64 numpy restatement below (`f64_diagnostics`).

The bound.  For each case and each diagnostic the kernel path's [10] vector is compared with the float64 result; g is the CPU path's
(the reference's f32 formulation's) largest gap to the same float64 result over the ten buckets, and the kernel path may err by 4 g -
the bar DESIGN.md uses for muse_resize_bicubic_norm_f32.  g must be non-zero.  The seeds: g is the error of ONE float32 number per
bucket, so by chance it can be a small fraction of the result's unit in the last place (the first seeds tried had g down to 1/40 ulp),
and 4 g is then finer than float32 itself - a correctly rounded result, half an ulp off, would miss it.  Each case therefore uses
the first seed (own number + 100 n) at which g is at least half an ulp of the largest float64 entry for every diagnostic and the
frame, found on the CPU from the reference formulation alone: `python tests/test_gpu_diagnostics.py` prints every g and g / ulp
without a GPU.  bf16 logits: the float64 result and the CPU path are those of the upcast input.

Which shape reaches which edge (f32 groups are 4 columns, bf16 groups 8; a wave folds 64 groups per step, two steps per loop trip):
  golden 12 x 20 x 16     fewer columns than lanes; all ten buckets; the reference's own numbers
  V = 63 / 64 / 65        a partial last group / whole groups / one column in the last group
  V = 255 / 257           64 groups: every lane exactly one / 65 groups: lane 0 enters the two-group loop trip
  V = 513, 1025           a third and a fifth group for lane 0 (f32: 129 / 257 groups; bf16: 65 / 129 groups); 1025 f32 = 257 groups is
                          also the first shape with two column blocks in muse_masked_mean_probs
  V = 2025, ld = 2025     config A: B x S = 8 x 9 puts the always-masked token 0 of image b at row 9 b, i.e. at all four (f32) / eight
                          (bf16) offsets from 16-byte alignment - the funnel-shifted vector pairs, the peeled head group and tail
  V = 8192, 16384         the coyo_f8 and MoVQ codebooks (B * S = 3 x 4 for the latter: with B = 2 every masked share of S = 4 tokens
                          names a bucket >= B, for which the reference's frame raises)
  ld > V slices           V = 125 in ld = 131 (odd ld: unaligned rows AND pad columns), V = 2025 in ld = 2048 (aligned rows, partial tail)
  S = 1, S = 257          one token per image (B = 10: share 1 is bucket 9, which the frame looks up as image 9); 25 / 51 / 77 masked
                          rows: whole unrolled steps of eight plus a remainder
  S = 2049                one row more than a segment of muse_masked_mean_probs' masked-row list (2048)
  B * S = 15 and 21       one row below / above a whole number of four-row workgroups
  bf16                    V = 65, 513, 1025 and 2025 (ld = 2025)
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
LS = 0.1          # label smoothing of the cross-entropy diagnostic (the golden's)

#        name            B   S     V      ld     dtype seed
CASES = [
    ("v63",              6,  10,   63,    63,    F32,  201),
    ("v64",              6,  10,   64,    64,    F32,  302),
    ("v65",              6,  10,   65,    65,    F32,  303),
    ("v255",             5,  6,    255,   255,   F32,  104),
    ("v257",             5,  6,    257,   257,   F32,  105),
    ("v513",             4,  6,    513,   513,   F32,  6),
    ("v1025",            3,  5,    1025,  1025,  F32,  7),
    ("v2025",            8,  9,    2025,  2025,  F32,  208),
    ("v8192",            3,  8,    8192,  8192,  F32,  9),
    ("v16384",           3,  4,    16384, 16384, F32,  210),
    ("slice125",         5,  7,    125,   131,   F32,  211),
    ("slice2025",        3,  6,    2025,  2048,  F32,  912),
    ("s1",               10, 1,    65,    65,    F32,  13),
    ("s257",             3,  257,  33,    33,    F32,  314),
    ("s2049",            2,  2049, 5,     5,     F32,  115),
    ("rows15",           3,  5,    40,    40,    F32,  2516),
    ("rows21",           3,  7,    40,    40,    F32,  617),
    ("v65_bf16",         6,  10,   65,    65,    BF,   18),
    ("v513_bf16",        4,  6,    513,   513,   BF,   819),
    ("v1025_bf16",       3,  5,    1025,  1025,  BF,   20),
    ("v2025_bf16",       8,  9,    2025,  2025,  BF,   221),
]
CASE_NAMES = [c[0] for c in CASES]


def make_case(name):
    """-> dict(logits [B, S, V] (a view into [B, S, ld]), ids, labels, mask_id), all on the CPU.  Every image has its token 0 masked (the
    cross-entropy diagnostic averages the first B token losses: it sees a masked token) plus others up to a share of (b + 1) / 10 for
    image b, so image b's bucket number is at most b: the reference's frame looks bucket k up as IMAGE k and raises for k >= B"""
    _, B, S, V, ld, dtype, seed = next(c for c in CASES if c[0] == name)
    g = torch.Generator().manual_seed(1000 + seed)
    mask_id = V - 1
    tokens = torch.randint(0, V - 1, (B, S), generator=g)
    ids = tokens.clone()
    for b in range(B):
        n = max(1, int(S * (min(b, 9) + 1) / 10 + 1e-9))
        pos = torch.cat([torch.zeros(1, dtype=torch.long), 1 + torch.randperm(S - 1, generator=g)[:n - 1]])
        ids[b, pos] = mask_id
    labels = torch.where(ids == mask_id, tokens, torch.full_like(tokens, -100))
    buf = (torch.randn(B, S, ld, generator=g) * 2).to(dtype)
    return dict(buf=buf, logits=buf[..., :V], ids=ids, labels=labels, mask_id=mask_id)


def golden_case(golden_dir):
    g = np.load(os.path.join(golden_dir, "training_utils.npz"))
    ids, labels, logits = (torch.from_numpy(g[k]) for k in ("input_ids", "labels", "logits"))
    return dict(buf=logits, logits=logits, ids=ids, labels=labels, mask_id=int(g["mask_id"])), g


def _avg64(values, buckets):
    """average_by_buckets in float64: only the leading len(buckets) values take part"""
    total = np.zeros(10)
    np.add.at(total, buckets, values[:len(buckets)])
    return total / np.maximum(np.bincount(buckets, minlength=10), 1)


def f64_diagnostics(logits, ids, labels, mask_id, ls=LS):
    """the four diagnostics restated in float64 numpy -> dict(pixel [10], image [10], ce [10], dist (buckets, probs))"""
    from muse import training_utils as TU
    x = logits.double().numpy()
    m = (ids == mask_id).numpy()
    lab = labels.numpy()
    buckets = TU.input_ids_to_masked_buckets(ids, mask_id).numpy()          # [B] integers: left in torch by the feature too
    with np.errstate(all="ignore"):
        z = x - x.max(-1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(-1, keepdims=True))
        p = np.exp(logp)
        ent = np.where(m, -(p * logp).sum(-1), 0.0)
        pixel_img = ent.sum(-1) / m.sum(-1)
        mean = (p * m[..., None]).sum(1) / m.sum(-1, keepdims=True)
        image_img = -(mean * np.log(mean)).sum(-1)
        valid = lab >= 0
        nll = -np.take_along_axis(logp, np.where(valid, lab, 0)[..., None], -1)[..., 0]
        ce = np.where(valid, (1 - ls) * nll + ls * -logp.mean(-1), 0.0).reshape(-1)
    db, dp = [], []
    for b in range(10):
        if (buckets == b).any() and b < len(buckets) and m[b].any():
            db += [b] * x.shape[-1]
            dp += list(p[b][m[b]][0])
    return dict(pixel=_avg64(pixel_img, buckets), image=_avg64(image_img, buckets), ce=_avg64(ce, buckets), dist=(np.array(db), np.array(dp)),
                pixel_img=pixel_img, image_img=image_img)


def cpu_diagnostics(logits, ids, labels, mask_id, ls=LS, dist=True):
    """the module's CPU path (the reference's f32 formulation) on the upcast logits"""
    from muse import training_utils as TU
    x = logits.float()
    out = dict(pixel=TU.pixel_entropy_per_percent_masked_bucket(x.clone(), ids, mask_id).double().numpy(),
               image=TU.image_entropy_per_percent_masked_bucket(x.clone(), ids, mask_id).double().numpy(),
               ce=TU.cross_entropy_per_percent_masked_bucket(x.clone(), labels, ids, mask_id, x.shape[-1], ls).double().numpy())
    if dist:
        df = TU.token_probability_distributions_per_percent_masked_bucket(x.clone(), ids, mask_id)
        out["dist"] = (df["bucket"].to_numpy(), df["masked_pixel_prob"].to_numpy().astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, float64 results, CPU-path results), computed once per case and shared"""
    c = make_case(name)
    return c, f64_diagnostics(c["logits"], c["ids"], c["labels"], c["mask_id"]), cpu_diagnostics(c["logits"], c["ids"], c["labels"], c["mask_id"])


def gap(a, ref):
    """largest |a - ref| over the entries where ref is a number; the NaN entries must coincide"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), (a, ref)
    ok = ~np.isnan(ref)
    return float(np.abs(a[ok] - ref[ok]).max()) if ok.any() else 0.0


def check_bound(what, kernel, cpu, f64, also=None):
    g, e = gap(cpu, f64), gap(kernel, f64)
    print(f"{what}: kernel error {e:.3e}  g {g:.3e}  ratio {e / g if g else float(e > 0):.2f}")
    # the golden batch has no seed to choose: its cross-entropy entries are the first 12 token losses, all of unmasked tokens, i.e. exact
    # zeros on every path (g = 0, and the bound then asks for an error of 0)
    assert g > 0 or also is not None, f"{what}: the CPU path equals float64 here, choose another seed"
    assert e <= 4 * g, f"{what}: kernel error {e:.3e} > 4 x {g:.3e}"
    if also is not None:
        e2 = gap(kernel, also)
        print(f"{what}: against the golden {e2:.3e}  ratio {e2 / g if g else float(e2 > 0):.2f}")
        assert e2 <= 4 * g, f"{what}: {e2:.3e} from the golden > 4 x {g:.3e}"


def on_gpu(c):
    """the case's tensors on the GPU, the logits still the [..., :V] view of the [B, S, ld] buffer"""
    buf = c["buf"].to(DEV)
    return buf[..., :c["logits"].shape[-1]], c["ids"].to(DEV), c["labels"].to(DEV), c["mask_id"]


def kernel_diagnostics(logits, ids, labels, mask_id, ls=LS):
    from muse import training_utils as TU
    df = TU.token_probability_distributions_per_percent_masked_bucket(logits, ids, mask_id)
    return dict(pixel=TU.pixel_entropy_per_percent_masked_bucket(logits, ids, mask_id).double().cpu().numpy(),
                image=TU.image_entropy_per_percent_masked_bucket(logits, ids, mask_id).double().cpu().numpy(),
                ce=TU.cross_entropy_per_percent_masked_bucket(logits, labels, ids, mask_id, logits.shape[-1], ls).double().cpu().numpy(),
                dist=(df["bucket"].to_numpy(), df["masked_pixel_prob"].to_numpy().astype(np.float64)))


def bits(t):
    """a float tensor's bit patterns (NaN-safe equality)"""
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).clone()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
def _check_values(name, c, f64, cpu, golden=None):
    from muse import training_utils as TU
    logits, ids, labels, mask_id = on_gpu(c)
    assert logits.stride(-1) == 1 and logits.stride(-2) == c["buf"].shape[-1]      # the slice goes in as a view
    k = kernel_diagnostics(logits, ids, labels, mask_id)
    for d, key in (("pixel", "pixel_entropy"), ("image", "image_entropy"), ("ce", "cross_entropy")):
        check_bound(f"{name} {d}", k[d], cpu[d], f64[d], None if golden is None else golden[key].astype(np.float64))
    assert k["dist"][0].dtype == cpu["dist"][0].dtype and np.array_equal(k["dist"][0], cpu["dist"][0]) and np.array_equal(k["dist"][0], f64["dist"][0])
    check_bound(f"{name} dist", k["dist"][1], cpu["dist"][1], f64["dist"][1], None if golden is None else golden["dist.prob"].astype(np.float64))
    # masked_token_diagnostics: the same launches, so the same bits as the three functions
    r = TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)
    assert torch.equal(r.buckets.cpu(), TU.input_ids_to_masked_buckets(c["ids"], mask_id))
    for d, v in (("pixel", r.pixel_entropy), ("image", r.image_entropy), ("ce", r.cross_entropy)):
        assert np.array_equal(v.double().cpu().numpy(), k[d], equal_nan=True), d
    assert r.token_cross_entropy.shape == (ids.numel(),) and r.pixel_entropy_per_image.shape == r.image_entropy_per_image.shape == (ids.shape[0],)
    check_bound(f"{name} pixel per image", r.pixel_entropy_per_image.double().cpu().numpy(), *_per_image_cpu(c, "pixel"), f64["pixel_img"])
    check_bound(f"{name} image per image", r.image_entropy_per_image.double().cpu().numpy(), *_per_image_cpu(c, "image"), f64["image_img"])
    no_ce = TU.masked_token_diagnostics(logits, None, ids, mask_id)
    assert no_ce.token_cross_entropy is None and no_ce.cross_entropy is None and same_bits(no_ce.pixel_entropy, r.pixel_entropy)


def _per_image_cpu(c, which):
    """the CPU path's per-image value: the bucket function on each image alone has it in the image's bucket"""
    from muse import training_utils as TU
    fn = TU.pixel_entropy_per_percent_masked_bucket if which == "pixel" else TU.image_entropy_per_percent_masked_bucket
    out = []
    for b in range(c["ids"].shape[0]):
        one = c["ids"][b:b + 1]
        out.append(float(fn(c["logits"][b:b + 1].float().clone(), one, c["mask_id"])[int(TU.input_ids_to_masked_buckets(one, c["mask_id"]))]))
    return (np.array(out),)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_values_within_four_times_the_cpu_paths_gap(name):
    c, f64, cpu = expected(name)
    _check_values(name, c, f64, cpu)


def test_values_on_the_reference_golden_batch(golden_dir):
    """V = 16 (fewer columns than lanes), all ten buckets: against float64 AND the reference module's own recorded results"""
    c, g = golden_case(golden_dir)
    f64, cpu = f64_diagnostics(c["logits"], c["ids"], c["labels"], c["mask_id"]), cpu_diagnostics(c["logits"], c["ids"], c["labels"], c["mask_id"])
    assert np.array_equal(cpu["pixel"], g["pixel_entropy"].astype(np.float64))          # the CPU path IS the reference (test_surface.py)
    _check_values("golden", c, f64, cpu, golden=g)


# ---- 2. structure: exact --------------------------------------------------------------------------------------------------------------
POISON = (float("nan"), float("inf"), float("-inf"), 1e30)


def _poison_(t, where):
    """write NaN, +inf, -inf, 1e30 in turn into t[where]"""
    n = int(where.sum())
    t[where] = torch.tensor(POISON, dtype=t.dtype, device=t.device).repeat(n // 4 + 1)[:n]


@pytest.mark.parametrize("name", ["slice125", "slice2025", "v2025_bf16"])
def test_poison_in_unmasked_rows_and_pad_columns_changes_no_bit(name):
    """(a) rows that are not masked are not loaded and pad columns are never read: NaN / inf / 1e30 there leave the entropies bit-identical;
    for the cross-entropy the poison goes only into rows whose label is -100 (their loss is 0 whatever they hold)"""
    from muse import training_utils as TU
    c = make_case(name)
    logits, ids, labels, mask_id = on_gpu(c)
    V = logits.shape[-1]
    clean = TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)
    clean_fn = (TU.pixel_entropy_per_percent_masked_bucket(logits, ids, mask_id), TU.image_entropy_per_percent_masked_bucket(logits, ids, mask_id))
    buf = c["buf"].to(DEV)
    unmasked = (ids != mask_id)[..., None].expand_as(buf)
    rows_only = buf.clone()
    _poison_(rows_only, unmasked & (torch.arange(buf.shape[-1], device=DEV) < V))
    ce = TU.masked_token_diagnostics(rows_only[..., :V], labels, ids, mask_id, label_smoothing=LS)
    assert same_bits(ce.token_cross_entropy, clean.token_cross_entropy) and same_bits(ce.cross_entropy, clean.cross_entropy)
    assert same_bits(TU.cross_entropy_per_percent_masked_bucket(rows_only[..., :V], labels, ids, mask_id, V, LS), clean.cross_entropy)
    pad = (torch.arange(buf.shape[-1], device=DEV) >= V).expand_as(buf)
    _poison_(buf, unmasked | pad)
    assert bool(torch.isnan(buf).any()) and (buf.shape[-1] == V or bool(torch.isnan(buf[..., V:]).any()))
    got = TU.masked_token_diagnostics(buf[..., :V], None, ids, mask_id)
    for f in ("pixel_entropy_per_image", "image_entropy_per_image", "pixel_entropy", "image_entropy"):
        assert same_bits(getattr(got, f), getattr(clean, f)), f
        assert not bool(torch.isnan(getattr(got, f)[:ids.shape[0]] if "per_image" in f else getattr(got, f)).any()), f
    assert same_bits(TU.pixel_entropy_per_percent_masked_bucket(buf[..., :V], ids, mask_id), clean_fn[0])
    assert same_bits(TU.image_entropy_per_percent_masked_bucket(buf[..., :V], ids, mask_id), clean_fn[1])


@pytest.mark.parametrize("name", ["v2025", "v2025_bf16", "slice125", "s257"])
def test_each_image_alone_gives_the_bits_it_gives_in_the_batch(name):
    """(b) an image's entropies do not depend on the other images - nor on where its rows lie: the B = 1 call gets a fresh copy, so with
    ld = 2025 its rows sit at other offsets from 16-byte alignment than in the batch"""
    from muse import training_utils as TU
    c = make_case(name)
    logits, ids, labels, mask_id = on_gpu(c)
    batch = TU.masked_token_diagnostics(logits, None, ids, mask_id)
    for b in range(ids.shape[0]):
        for shift in (0, 1):                                              # the copy at an aligned base and one element behind it
            flat = torch.empty(logits[b].numel() + 1, dtype=logits.dtype, device=DEV)
            one = flat[shift:shift + logits[b].numel()].view(1, *logits[b].shape).copy_(logits[b:b + 1])
            alone = TU.masked_token_diagnostics(one, None, ids[b:b + 1], mask_id)
            assert same_bits(alone.pixel_entropy_per_image, batch.pixel_entropy_per_image[b:b + 1]), (b, shift)
            assert same_bits(alone.image_entropy_per_image, batch.image_entropy_per_image[b:b + 1]), (b, shift)


@pytest.mark.parametrize("name", ["v8192", "v2025_bf16"])
def test_two_calls_give_identical_bits(name):
    """(c)"""
    from muse import training_utils as TU
    c = make_case(name)
    logits, ids, labels, mask_id = on_gpu(c)
    a = TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)
    b = TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)
    for x, y in zip(a, b):
        assert same_bits(x, y) if x.is_floating_point() else torch.equal(x, y)
    da, db = (TU.token_probability_distributions_per_percent_masked_bucket(logits, ids, mask_id) for _ in range(2))
    assert da.equals(db)


def _all_functions(TU, logits, labels, ids, mask_id):
    V = logits.shape[-1]
    return [lambda: TU.pixel_entropy_per_percent_masked_bucket(logits, ids, mask_id),
            lambda: TU.image_entropy_per_percent_masked_bucket(logits, ids, mask_id),
            lambda: TU.cross_entropy_per_percent_masked_bucket(logits, labels, ids, mask_id, V, LS),
            lambda: TU.token_probability_distributions_per_percent_masked_bucket(logits, ids, mask_id),
            lambda: TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)]


@pytest.mark.parametrize("name", ["slice125", "v65_bf16"])
def test_logits_are_bitwise_unchanged_after_every_function(name):
    """(d) also for logits that require grad and hang on a graph (what the training script passes): no function writes them, bumps their
    version or disturbs the backward pass"""
    from muse import training_utils as TU
    c = make_case(name)
    logits, ids, labels, mask_id = on_gpu(c)
    buf = logits._base if logits._base is not None else logits
    before = bits(buf)
    for fn in _all_functions(TU, logits, labels, ids, mask_id):
        fn()
        assert torch.equal(bits(buf), before)
    leaf = logits.float().clone().requires_grad_(True)
    attached = leaf * 1.0
    before, version = bits(attached.detach()), attached._version
    for fn in _all_functions(TU, attached, labels, ids, mask_id):
        out = fn()
        assert torch.equal(bits(attached.detach()), before) and attached._version == version
        assert not any(getattr(t, "requires_grad", False) for t in (out if isinstance(out, tuple) else (out,)))
    attached.sum().backward()
    assert torch.equal(leaf.grad, torch.ones_like(leaf))


# ---- 3. the reference's edge semantics --------------------------------------------------------------------------------------------------
def test_an_image_without_masked_tokens_gives_nan_where_the_cpu_path_does():
    from muse import training_utils as TU
    c = make_case("v257")
    ids = c["ids"].clone()
    ids[1] = torch.where(ids[1] == c["mask_id"], torch.zeros_like(ids[1]), ids[1])        # image 1: nothing masked -> bucket 0
    c = dict(c, ids=ids, labels=torch.where(ids == c["mask_id"], c["labels"], torch.full_like(ids, -100)))
    f64, cpu = f64_diagnostics(c["logits"], ids, c["labels"], c["mask_id"]), cpu_diagnostics(c["logits"], ids, c["labels"], c["mask_id"], dist=False)
    assert np.isnan(cpu["pixel"]).sum() == 1 and np.isnan(cpu["image"]).sum() == 1
    logits, ids_d, labels, mask_id = on_gpu(c)
    for d, fn in (("pixel", TU.pixel_entropy_per_percent_masked_bucket), ("image", TU.image_entropy_per_percent_masked_bucket)):
        check_bound(f"nothing masked {d}", fn(logits, ids_d, mask_id).double().cpu().numpy(), cpu[d], f64[d])    # gap() compares the NaN entries
    r = TU.masked_token_diagnostics(logits, labels, ids_d, mask_id, label_smoothing=LS)
    assert torch.isnan(r.pixel_entropy_per_image).tolist() == torch.isnan(r.image_entropy_per_image).tolist() == [b == 1 for b in range(ids.shape[0])]


def test_a_code_of_exactly_zero_mean_probability_gives_nan_image_entropy():
    """a logit gap above 110 underflows exp in f32: the mean probability of the other codes is exactly 0 and 0 * log(0) is NaN, on the CPU
    path and on the kernel path; the per-token entropy of such a row is a number on both"""
    from muse import training_utils as TU
    c = make_case("v65")
    logits = c["logits"].clone()
    logits[2][c["ids"][2] == c["mask_id"]] = 0.0
    logits[2, :, 7][c["ids"][2] == c["mask_id"]] = 120.0
    cpu_image = TU.image_entropy_per_percent_masked_bucket(logits.clone(), c["ids"], c["mask_id"])
    cpu_pixel = TU.pixel_entropy_per_percent_masked_bucket(logits.clone(), c["ids"], c["mask_id"])
    assert int(torch.isnan(cpu_image).sum()) == 1 and not bool(torch.isnan(cpu_pixel).any())
    dev = logits.to(DEV)
    ids = c["ids"].to(DEV)
    assert torch.isnan(TU.image_entropy_per_percent_masked_bucket(dev, ids, c["mask_id"])).cpu().tolist() == torch.isnan(cpu_image).tolist()
    assert not bool(torch.isnan(TU.pixel_entropy_per_percent_masked_bucket(dev, ids, c["mask_id"])).any())
    r = TU.masked_token_diagnostics(dev, None, ids, c["mask_id"])
    assert torch.isnan(r.image_entropy_per_image).tolist() == [b == 2 for b in range(ids.shape[0])] and float(r.pixel_entropy_per_image[2]) == 0.0


@pytest.mark.parametrize("device", ["cpu", DEV])
def test_token_distribution_frame_raises_the_references_index_errors(device):
    """the frame indexes the batch with the bucket's own number: a bucket number >= B, and a bucket whose image b has no masked token, raise
    IndexError on the CPU path and on the kernel path alike"""
    from muse import training_utils as TU
    mask_id, V = 9, 10
    logits = torch.randn(3, 10, V, generator=torch.Generator().manual_seed(5)).to(device)
    ids = torch.zeros(3, 10, dtype=torch.long)
    ids[0, :1], ids[1, :2], ids[2, :8] = mask_id, mask_id, mask_id                 # buckets 0, 1, 7: bucket 7 >= B = 3
    with pytest.raises(IndexError, match="index 7 is out of bounds for dimension 0 with size 3"):
        TU.token_probability_distributions_per_percent_masked_bucket(logits, ids.to(device), mask_id)
    ids = torch.zeros(3, 10, dtype=torch.long)
    ids[0, :2], ids[2, :3] = mask_id, mask_id                                       # buckets 1, 0, 2: bucket 1 occurs, image 1 has no masked token
    with pytest.raises(IndexError, match="index 0 is out of bounds for dimension 0 with size 0"):
        TU.token_probability_distributions_per_percent_masked_bucket(logits, ids.to(device), mask_id)
    ids[1, 4:6] = mask_id                                                           # buckets 1, 1, 2: rows of images 1 and 2, first masked tokens 4 and 0
    df = TU.token_probability_distributions_per_percent_masked_bucket(logits, ids.to(device), mask_id)
    assert df["bucket"].tolist() == [1] * V + [2] * V
    want = torch.softmax(logits.cpu().double(), -1)
    assert np.allclose(df["masked_pixel_prob"].to_numpy().astype(np.float64), torch.cat([want[1, 4], want[2, 0]]).numpy(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("S", [10, 20, 256, 1000])
def test_buckets_of_gpu_ids_fall_as_on_the_cpu(S):
    """every masked count 0 ... S, bucket edges included (18 of 20 is bucket 8 in the reference's golden): ids on the GPU get the buckets
    the CPU code gives them"""
    from muse import training_utils as TU
    ids = (torch.arange(S)[None, :] < torch.arange(S + 1)[:, None]).long()          # row n: n tokens equal to mask id 1
    cpu = TU.input_ids_to_masked_buckets(ids, 1)
    assert cpu[0] == 0 and cpu[-1] == 9 and sorted(set(cpu.tolist())) == list(range(10))
    got = TU.input_ids_to_masked_buckets(ids.to(DEV), 1)
    assert got.dtype == torch.long and got.is_cuda and torch.equal(got.cpu(), cpu)


# ---- 4. memory: the feature's contract ------------------------------------------------------------------------------------------------
def test_no_call_allocates_anything_of_the_logits_size():
    """B = 8, S = 64, V = 2048 f32 (4 MiB of logits): each bucket function and masked_token_diagnostics stays below HALF the logits' bytes
    of peak allocation above the level before the call (the workspaces are O(B S + B V), about 70 KiB).  The torch formulation allocates
    three logits-sized temporaries."""
    from muse import training_utils as TU
    B, S, V, mask_id = 8, 64, 2048, 2047
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(B, S, V, generator=g).to(DEV)
    ids = torch.randint(0, V - 1, (B, S), generator=g)
    ids[torch.rand(B, S, generator=g) < torch.linspace(0.05, 0.95, B)[:, None]] = mask_id
    ids[:, 0] = mask_id
    labels = torch.where(ids == mask_id, torch.randint(0, V - 1, (B, S), generator=g), torch.full_like(ids, -100)).to(DEV)
    ids = ids.to(DEV)
    calls = {"pixel": lambda: TU.pixel_entropy_per_percent_masked_bucket(logits, ids, mask_id),
             "image": lambda: TU.image_entropy_per_percent_masked_bucket(logits, ids, mask_id),
             "cross_entropy": lambda: TU.cross_entropy_per_percent_masked_bucket(logits, labels, ids, mask_id, V, LS),
             "all": lambda: TU.masked_token_diagnostics(logits, labels, ids, mask_id, label_smoothing=LS)}
    limit = logits.numel() * logits.element_size() // 2
    for name, fn in calls.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        print(f"{name}: peak {peak} bytes above the level before the call (limit {limit})")
        assert peak < limit, (name, peak, limit)
        del out


# ---- 5. the wrappers refuse what the kernels do not take --------------------------------------------------------------------------------
def test_the_ops_wrappers_refuse_instead_of_computing_something_else():
    from muse import ops
    from muse._hip import MuseHipError
    assert hasattr(ops.lib(), "muse_token_stats") and hasattr(ops.lib(), "muse_masked_mean_probs")
    rows, cols = 8, 32
    x = torch.randn(rows, cols, device=DEV)
    ids = torch.zeros(2, 4, dtype=torch.long, device=DEV)
    lse = torch.ones(rows, device=DEV)
    bad = {"cpu tensors": x.cpu(), "float16": x.half(), "float64": x.double(), "last stride 2": torch.randn(rows, 2 * cols, device=DEV)[:, ::2]}
    for why, t in bad.items():
        with pytest.raises(MuseHipError):
            ops.token_stats(t)
        with pytest.raises(MuseHipError):
            ops.masked_mean_probs(t, ids.cpu() if why == "cpu tensors" else ids, *([lse.cpu() if why == "cpu tensors" else lse] * 2), 0)
    for vocab in (cols + 1, 0):                                                       # vocab > ld, and no column at all
        with pytest.raises(MuseHipError):
            ops.token_stats(x, vocab=vocab)
        with pytest.raises(MuseHipError):
            ops.masked_mean_probs(x, ids, lse, lse, 0, vocab=vocab)
    with pytest.raises(MuseHipError):
        ops.token_stats(torch.randn(rows * cols, device=DEV).as_strided((rows, cols), (cols // 2, 1)), vocab=cols)   # overlapping rows: vocab > ld
    with pytest.raises(MuseHipError):
        ops.masked_mean_probs(x, ids[:, :3].contiguous(), lse, lse, 0)                    # ids that do not match the rows
    with pytest.raises(MuseHipError):
        ops.token_stats(x, row_mask=torch.ones(rows - 1, dtype=torch.bool, device=DEV))
    for values, id_ in ((lse.view(2, 4).cpu(), ids.cpu()), (lse.view(2, 4).double(), ids), (lse.view(4, 2), ids), (lse.view(2, 4), ids.int())):
        with pytest.raises(MuseHipError):
            ops.masked_row_mean(values, id_, 0)
    assert ops.masked_row_mean(lse.view(2, 4), ids, 0).tolist() == [1.0, 1.0]          # four ones over four masked tokens (ids are all 0)
    lse_ok, ent = ops.token_stats(x, vocab=cols - 3)                                  # and what they do take still runs
    want = torch.logsumexp(x[:, :cols - 3].double(), -1)
    assert float((lse_ok.double() - want).abs().max()) < 1e-5 and ent.shape == (rows,)


if __name__ == "__main__":
    # no GPU needed: every case's g (the CPU path's gap to float64) - the tests require each to be non-zero
    sys_path = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import sys
    sys.path[:0] = [os.path.join(sys_path, "open-muse_amd")]
    for case_name in CASE_NAMES:
        _, f64_, cpu_ = expected(case_name)
        f64_["dist_p"], cpu_["dist_p"] = f64_["dist"][1], cpu_["dist"][1]
        print(case_name, {d: f"g {gap(cpu_[d], f64_[d]):.3e} = {gap(cpu_[d], f64_[d]) / np.spacing(np.float32(np.nanmax(np.abs(f64_[d])))):.2f} ulp"
                          for d in ("pixel", "image", "ce", "dist_p")})
