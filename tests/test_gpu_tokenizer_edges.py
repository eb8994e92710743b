"""GPU (-m gpu): the six tokenizer entry points of csrc/paella.hip and csrc/movq.hip at each edge of their dispatch: exact probes, a
per-element rounding leg, the special values and the host-side refusals.  tests/tokenizer_cpu.py holds the float64 references, the probes,
the checks, the derived bounds and a contract model; tests/test_tokenizer_cpu.py proves on a CPU that the checks fail for seventeen seeded
defects.  profiles/tokenizer_edges.md has the edge table and the MI355X's figures; DESIGN.md ("Tokenizer kernel contract") the contract.

Every case: operands sit inside larger allocations with NaN in front of them and in every ld > cols gap; the activation (x, z, the image)
ends its allocation, every other operand has NaN behind it too; outputs and the `stats` / `partial` buffers are pre-filled with a NaN bit
pattern no result has, guard bands on both sides - the guards come back bit for bit and every slot is written; the case is launched
twice from the same initial state and the two results are bit-identical (the SpatialNorm f64 partials, which accumulate through LDS
atomicAdd, agree within the rounding of an f64 sum of their length instead).

Exact legs (equal to the float64 reference whatever the order): muse_patch_rows_nhwc on a coordinate ramp with -0.0 elements, bit for bit;
muse_vq_nearest_small on small integers (idx = the float64 argmin, lowest index on ties, dist bit-exact); in_block / out_block on integers
and on one-hot coordinate probes.  Rounding legs: seeded N(0, 1) (and 1e3 + N(0, 1)) per element against float64, bound = 4 * E_REF[leg]
* the sum of the absolute terms, E_REF = torch's own float32 CPU computation against float64 over the same cases (`python
tests/test_gpu_tokenizer_edges.py` reprints it, no GPU needed).  SpatialNorm's bound is derived (tokenizer_cpu.bound_spatial_norm on top
of spatial_cpu.bound_groupnorm): its f64 statistics make it far smaller than 4 * E_REF of torch's f32 GroupNorm.  The codebook search is
judged against the derived margin (D + 2) * 2^-23 (tokenizer_cpu.vq_margin).

Edges (thresholds as the code has them) and the case that meets each:
  muse_spatial_norm_nhwc
    apply chunk apix 128 / 256 / 512 / 1024 (halved until batch * chunks >= 2 CUs): test_spatial_norm_apply_chunk[apix-label], batch chosen
      by tokenizer_cpu.sn_batch_for from the device's CU count, HW {apix k - 1, apix k, apix k + 1}, k = 2, tensor and planes; at 128 also HW
      {1, 127, 128, 129, 257}
    UN = 4 tail, every residue of UN * ppi: test_spatial_norm_un_tail (C 1024, ppi 1: HW 1 .. 5; C 256, ppi 4: HW 15, 16, 17)
    template instances Z 1 .. 8: test_spatial_norm_z[1 .. 8]; Z 4, 8 with zq 4 bytes off refused (MUSE_ERR_ALIGN), every other Z (3 and 5
      among them) 4 bytes off gives the aligned bits with NaN directly behind the last zq row (the 12- and 20-byte rows are read float by
      float); both sides of that comparison take one producer partial, so no atomicAdd stands between them
    sn_div shift / division for W, H / zh, W / zw, factor 3 included: test_spatial_norm_factors (factors (1, 1), (2, 2), (3, 1), (1, 3),
      (3, 2), (8, 8) x W {2, 6, 8, 12}, coordinate-coded zq)
    channels: test_spatial_norm_channels (C 32 .. 1024: vpp 8 .. 256; 1056, 2048: the vpp > 256 loop; G = 64 at C 64, 256, 2048), planes too
    statistics chunks of 1024 pixels: test_spatial_norm_stats_chunks (HW 1023, 1024, 1025, 2049)
    producer statistics: test_spatial_norm_producer_stats (stats_nchunk 1, 7, 8, 9 at G = 32 (tpg 8); 3, 4, 5 at G = 64 (tpg 4))
    inputs N(0, 1), 1e3 + N(0, 1), constant image: test_spatial_norm_inputs; NaN confinement: test_spatial_norm_nan_confinement
    batch 65535 served, 65536 refused: test_spatial_norm_batch_limit; refusals by return code (C 96, 2080, 48; groups 16; Z 0, 9;
      H % zh; batch 65536): test_spatial_norm_refusals
  muse_paella_mix_fwd
    statistics lanes G = 1 .. 64 and one to four vectors per lane: test_mix_channels (C 4, 8, 12, 24, 252, 256, 260, 512, 516, 768, 772,
      1024); rows {1, 256 / G - 1, 256 / G, 256 / G + 1} per G: test_mix_row_counts
    replicate border, image boundary (row0), ky / kx: test_mix_neighbour_probe (one-hot taps, (H, W) in (1, 1) .. (3, 3), B = 3)
    rounding N(0, 1) and 1e3 + N(0, 1), the stats buffer: test_mix_rounding; g2 = 0 returns x: test_mix_g2_zero_returns_x (C 4, 1024)
    refusals C 1028, C 6, x == y, x / y / stats 4 bytes off: test_mix_refusals
  muse_patch_rows_nhwc: test_patch_rows (KS {2, 4} x stride {1, 2} x pads {0, 1}^2 x C {4, 8, 384}, B = 2, Hout / Wout one larger than the
    image supports); refusals KS 3, C 6, misaligned: test_patch_rows_refusals
  muse_vq_nearest_small: test_vq_exact / test_vq_seeded[D 1 .. 8]: Kc {1, 2, 3, 4, 5, CH - 1, CH, CH + 1, 2 CH + 1, 8192, 16384} (CH 2048
    for D <= 4, else 1024; Kc < 4: waves with an empty quarter), N {1, 63, 64, 65, 129}, ldz {D, D + 1, 16}; planted winners on the first and
    last code of every quarter of the first and last chunk; planted ties across a quarter, across a chunk and between chunks, once on codes
    that are no quarter edge (every edge keeps its unique winner; Kc >= CH + 3 for the chunk pairs) and once directly at the boundaries
    (tokenizer_cpu.vq_tie_pairs); a NaN row and an all-inf row return 0; test_vq_rows_and_strides crosses N x ldz
  muse_paella_in_block / out_block: test_blocks[int | coord | randn] ((H, W) {(2, 2), (2, 6), (6, 2), (4, 4), (6, 10)} x C {4, 8, 12, 384},
    B = 2; the image pointer 4 bytes off gives the aligned bits); refusals odd H / W, C 6, misaligned w12 / x / y: test_blocks_refusals
  grid-stride cap of 32768 blocks (grid_for): test_cap_mix, test_cap_patch_rows, test_cap_in_block, test_cap_out_block at C = 4: the whole
    batch in one launch against the same input image by image, bit for bit
"""
import sys
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

import spatial_cpu as S
import tokenizer_cpu as T
from spatial_cpu import BF, F32, F64, GUARD, LEAD

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_BAD_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3
EPS = 1e-6

# Worst normalised error of torch's float32 CPU computation against float64 over the case lists below, as printed by
# `python tests/test_gpu_tokenizer_edges.py`.  bound = 4 * E_REF[leg] * scale.
E_REF = {
    "mix": 2.841e-07,        # over |x| + |g2| (|bias| + sum |w| (|LN| |1 + g0| + |g1|))
    "mix_1e3": 3.478e-07,    # the same, 1e3 + N(0, 1) rows
    "ln_mean": 1.239e-07,    # over mean |x|
    "ln_rstd": 1.213e-07,    # over rstd; torch.rsqrt(torch.var(x, unbiased=False) + eps)
    "ln_mean_1e3": 1.326e-07,
    "ln_rstd_1e3": 1.070e-07,
    "in_block": 2.153e-07,   # over |bias| + sum |u| |w|, 12 terms
    "out_block": 1.409e-07,  # over |bias| + sum |x| |w|, C terms
    # printed for the profile; SpatialNorm is judged by tokenizer_cpu.bound_spatial_norm.  Over |n| Sm + Sa, n = GroupNorm(x): torch's f32
    # statistics set the first, and on 1e3 + N(0, 1) inputs they lose the variance altogether
    "spatial_norm": 1.588e-06,
    "spatial_norm_1e3": 6.814e-01,
}


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """a launch that faulted leaves the device unusable for the rest of the process: end the session there rather than start more work"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU error after a tokenizer edge test, stopping: {e}", returncode=3)


def _lib():
    from muse._hip import lib
    return lib()


def _stream():
    from muse.ops import stream
    return stream()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


class Op:
    """a storage on the device and the address of the operand / result `lead` elements into it"""

    def __init__(self, st, lead):
        self.t = st.to(DEV)
        self.lead = lead
        self.ptr = self.t.data_ptr() + lead * st.element_size()


def op_in(t, dtype=F32, shift=0, tail=LEAD):
    """an input inside NaN; shift = 1 (f32): 4 bytes off its 16-byte alignment; tail = 0: the operand ends its allocation"""
    body = torch.cat([torch.full((shift,), S.NAN, dtype=dtype), t.to(dtype).flatten()]) if shift else t
    o = Op(S.place(body, dtype, tail=tail, exact=False), LEAD + shift)
    assert (o.ptr % 16 == 0) == (shift == 0)
    return o


def op_out(n, dtype=F32, shift=0):
    return Op(S.alloc_out(n + shift, dtype), GUARD + shift)


def twice(what, spec, launch):
    """launch(*outputs) -> return code, run twice on fresh sentinel outputs of spec = [(n, dtype[, shift])]; the two runs' storages are
    bit-identical.  Returns the first run's storages (CPU)."""
    runs = []
    for _ in range(2):
        outs = [op_out(*s) for s in spec]
        rc = launch(*outs)
        assert rc == 0, f"{what}: the entry returned {rc}"
        runs.append([o.t.cpu() for o in outs])
    for i, (a, b) in enumerate(zip(*runs)):
        S.check_same_bits(a, b, f"{what} output {i}")
    return runs[0]


def refused(what, code, spec, launch):
    """launch(*outputs) must return `code` and launch nothing: every output storage keeps its sentinels"""
    outs = [op_out(*s) for s in spec]
    rc = launch(*outs)
    assert rc == code, f"{what}: the entry returned {rc}, not {code}"
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        S.check_untouched(o.t.cpu(), f"{what} output {i}")


WORST = {}


def note(leg, what, w):
    WORST[leg] = max(WORST.get(leg, 0.0), w)
    print(f"[tokenizer_edges] {leg} {what}: err/bound={w:.3f} (worst so far {WORST[leg]:.3f})")
    assert w <= 1.0, f"{what}: error {w:.3f} x its bound"


def judge(leg, what, st, n, ref, bound, guard=GUARD):
    """storage checks, then |got - ref| <= bound per element (on ref's device); prints the worst figure first"""
    body = S.check_out(st, n, ref.new_zeros(1), what, guard=guard, values=False)
    note(leg, what, S.worst_ratio(body.to(ref.device), ref, bound))
    return body


# =========================================================================================================================================
# a. muse_spatial_norm_nhwc
# =========================================================================================================================================
def sn_call(L, x, y, hi, lo, prm, part, snc, B, H, W, C, zh, zw, Z, G, silu, zq=None):
    return L.muse_spatial_norm_nhwc(x, y, hi, lo, prm["gamma"].ptr, prm["beta"].ptr, (zq or prm["zq"]).ptr, prm["wy"].ptr, prm["by"].ptr,
                                    prm["wb"].ptr, prm["bb"].ptr, part, snc, B, H, W, C, zh, zw, Z, G, EPS, silu, _stream())


def run_sn(t, H, W, G, what, leg="spatial_norm", planes=False, zq_shift=0, cuts=None, silus=(0, 1), nan_mask=None):
    """t: tokenizer_cpu.sn_inputs.  Launches the tensor (and with planes the (hi, lo)) form twice for every SiLU setting and judges each
    against the derived bound; cuts: a producer's statistics over that partition of the pixels.  Returns {silu: the f32 result body}."""
    L = _lib()
    B, HW, C = t["x"].shape
    _, zh, zw, Z = t["zq"].shape
    n = t["x"].numel()
    nch = L.muse_groupnorm_nchunk(HW)
    assert nch == (HW + T.SN_PIX - 1) // T.SN_PIX
    prm = {k: op_in(t[k]) for k in ("gamma", "beta", "wy", "by", "wb", "bb")}
    prm["zq"] = op_in(t["zq"], shift=zq_shift)
    xi = op_in(t["x"], tail=0)
    big = n > (1 << 21)
    td = {k: v.to(DEV) for k, v in t.items()} if big else t
    if nan_mask is not None:                                       # the reference of the clean input; the NaN elements are compared apart
        td = dict(td, x=torch.where(nan_mask, torch.zeros_like(t["x"]), t["x"]))
    stat_len, pin, snc = None, None, 0
    if cuts is not None:
        part, stat_len = T.sn_producer_partials(t["x"], G, cuts)
        pin, snc = op_in(part, F64), len(cuts) + 1
    npart = B * nch * G * 2
    if pin is None:                                                # (with a NaN input: the clean input's sums, the NaN slots compared apart)
        clean = t["x"] if nan_mask is None else td["x"]
        pref = T.ref_sn_partials(clean, G)
        pbound = min(HW, T.SN_PIX) * (C // G) * 2.0 ** -53 * T.ref_sn_partials(clean, G, terms=True) + S.TINY
        pnan = T.ref_sn_partials(t["x"], G).isnan().flatten()
    out = {}
    for silu in silus:
        r = T.ref_spatial_norm(td, H, W, G, EPS, silu)
        forms = [False, True] if planes else [False]
        for pl in forms:
            w_ = f"{what} silu{silu}{' planes' if pl else ''}"
            runs = []
            for _ in range(2):
                outs = [op_out(n, BF), op_out(n, BF)] if pl else [op_out(n, F32)]
                po = pin if pin is not None else op_out(npart, F64)
                rc = sn_call(L, xi.ptr, None if pl else outs[0].ptr, outs[0].ptr if pl else None, outs[1].ptr if pl else None, prm, po.ptr, snc,
                             B, H, W, C, zh, zw, Z, G, silu)
                assert rc == 0, f"{w_}: the entry returned {rc}"
                runs.append([o.t.cpu() for o in outs] + ([] if pin is not None else [po.t.cpu()]))
            same_partials = pin is not None or torch.equal(S.bits(runs[0][-1]), S.bits(runs[1][-1]))
            if pin is None and nan_mask is not None:              # guards, every slot written, NaN in the NaN group's slots only
                for run in runs:
                    pb_, s_ = S.bits(run[-1]), S.bits(S.sentinel(1, F64))[0]
                    assert bool((pb_[:GUARD] == s_).all()) and bool((pb_[GUARD + npart:] == s_).all()), f"{w_}: a guard band of the partials was written"
                    assert not bool((pb_[GUARD:GUARD + npart] == s_).any()), f"{w_}: a partial slot was never written"
                    pg = run[-1][GUARD:GUARD + npart]
                    assert torch.equal(pg.isnan(), pnan), f"{w_}: NaN outside its (image, group) in the partials, or a finite sum of NaN"
                    assert S.worst_ratio(pg[~pnan], pref.flatten()[~pnan], pbound.flatten()[~pnan]) <= 1.0, f"{w_}: partials"
            if pin is None and nan_mask is None:
                p0 = S.check_out(runs[0][-1], npart, pref, w_ + " partials", exact=False, bound=pbound)
                p1 = S.check_out(runs[1][-1], npart, pref, w_ + " partials (second launch)", exact=False, bound=pbound)
                assert S.worst_ratio(p0, p1, pbound) <= 1.0, f"{w_}: the two launches' partials differ by more than the rounding of their sums"
            if same_partials:
                for a, b in zip(runs[0], runs[1]):
                    S.check_same_bits(a, b, w_ + ": two launches with bit-equal partials")
            bound = T.bound_spatial_norm(td, r, G, EPS, silu, planes=pl, stat_len=stat_len, stat_parts=snc)
            for run in runs:
                if nan_mask is not None:
                    sb, s_ = S.bits(run[0]), S.bits(S.sentinel(1, F32))[0]
                    assert bool((sb[:GUARD] == s_).all()) and bool((sb[GUARD + n:] == s_).all()), f"{w_}: a guard band was written"
                    assert not bool((sb[GUARD:GUARD + n] == s_).any()), f"{w_}: a slot was never written"
                    got = run[0][GUARD:GUARD + n].view(B, HW, C)
                    assert torch.equal(got.isnan(), nan_mask), f"{w_}: NaN outside its (image, group), or a finite value inside"
                    note(leg, w_, S.worst_ratio(got[~nan_mask], r["y"][~nan_mask], bound[~nan_mask]))
                    out[silu] = got
                elif pl:
                    hi = S.check_out(run[0], n, r["y"].new_zeros(1), w_ + " hi", values=False)
                    lo = S.check_out(run[1], n, r["y"].new_zeros(1), w_ + " lo", values=False)
                    ref = r["y"]
                    note(leg + "_planes", w_ + " hi + lo", S.worst_ratio((hi.double() + lo.double()).to(ref.device), ref, bound))
                    note(leg + "_planes", w_ + " hi", S.worst_ratio(hi.to(ref.device), ref, bound + T.UBF * ref.abs()))
                else:
                    out[silu] = judge(leg, w_, run[0], n, r["y"], bound)
    return out


SN_CHANNELS = [(32, 32), (64, 32), (128, 32), (256, 32), (512, 32), (1024, 32), (1056, 32), (2048, 32), (64, 64), (256, 64), (2048, 64)]   # (C, G)


def sn_t(B, H, W, C, zh, zw, Z, key, **kw):
    return T.sn_inputs(B, H, W, C, zh, zw, Z, seed_of("sn", key, B, H, W, C, zh, zw, Z), **kw)


@pytest.mark.parametrize("C,G", SN_CHANNELS)
def test_spatial_norm_channels(C, G):
    run_sn(sn_t(2, 4, 6, C, 2, 3, 4, "ch"), 4, 6, G, f"spatial_norm C{C} G{G}", planes=True)


@pytest.mark.parametrize("Z", range(1, 9))
def test_spatial_norm_z(Z):
    """every template instance; Z % 4 == 0 wants a 16-byte zq (refused 4 bytes off), the others read float by float: the same bits 4 bytes
    off, with NaN directly behind the last zq row"""
    L = _lib()
    B, H, W, C, zh, zw = 2, 4, 6, 32, 2, 3
    t = sn_t(B, H, W, C, zh, zw, Z, "z")
    a = run_sn(t, H, W, 32, f"spatial_norm Z{Z}")
    if Z % 4:       # (both sides from one producer partial: no atomicAdd in the chain, so the bits are comparable across calls)
        a = run_sn(t, H, W, 32, f"spatial_norm Z{Z} producer statistics", cuts=[])
        b = run_sn(t, H, W, 32, f"spatial_norm Z{Z} zq 4 bytes off", zq_shift=1, cuts=[])
        for silu in (0, 1):
            S.check_same_bits(a[silu], b[silu], f"spatial_norm Z{Z}: aligned against 4 bytes off")
    else:
        prm = {k: op_in(t[k]) for k in ("gamma", "beta", "wy", "by", "wb", "bb")}
        xi, zs = op_in(t["x"], tail=0), op_in(t["zq"], shift=1)
        refused(f"spatial_norm Z{Z} zq 4 bytes off", ERR_ALIGN, [(t["x"].numel(), F32), (B * 32 * 2, F64)],
                lambda o, p: sn_call(L, xi.ptr, o.ptr, None, None, prm, p.ptr, 0, B, H, W, C, zh, zw, Z, 32, 1, zq=zs))


SN_FACTORS = [(fy, fx, W) for fy, fx in ((1, 1), (2, 2), (3, 1), (1, 3), (3, 2), (8, 8)) for W in (2, 6, 8, 12) if W % fx == 0]


def test_spatial_norm_factors():
    """zq is a coordinate code: a map one source pixel off moves whole rows by O(1), far outside the rounding bound"""
    for fy, fx, W in SN_FACTORS:
        zh, zw = 2, W // fx
        H = zh * fy
        run_sn(sn_t(2, H, W, 32, zh, zw, 4, "factor", coord_zq=True), H, W, 32, f"spatial_norm factor {fy}x{fx} W{W}")


APIX_CASES = [(apix, label) for apix in (128, 256, 512, 1024) for label in ("2apix-1", "2apix", "2apix+1")] + [(128, "small")]


def sn_apix_cases(cus):
    """{(apix, label): [(B, HW)]} for APIX_CASES: the smallest batch that reaches each apply chunk at HW = 2 apix - 1, 2 apix, 2 apix + 1
    under the host's rule, and the small images at 128"""
    out = {(128, "small"): [(1, HW) for HW in (1, 127, 128, 129, 257)]}
    for apix in (128, 256, 512, 1024):
        for label, HW in (("2apix-1", 2 * apix - 1), ("2apix", 2 * apix), ("2apix+1", 2 * apix + 1)):
            B = T.sn_batch_for(apix, HW, cus)
            assert B is not None, (apix, HW, cus)
            out[(apix, label)] = [(B, HW)]
    return out


@pytest.mark.parametrize("apix,label", APIX_CASES)
def test_spatial_norm_apply_chunk(apix, label):
    """the chunk sizes are reached under the host's rule as restated in tokenizer_cpu.sn_apix (the kernel's own apix is not observable)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = sn_apix_cases(cus)
    assert {T.sn_apix(B, HW, cus) for k, v in cases.items() if k[1] == "2apix" for B, HW in v} == {128, 256, 512, 1024}
    for B, HW in cases[(apix, label)]:
        assert T.sn_apix(B, HW, cus) == apix
        run_sn(sn_t(B, 1, HW, 32, 1, 1, 4, "apix"), 1, HW, 32, f"spatial_norm apix{apix} B{B} HW{HW}", planes=True)


def test_spatial_norm_un_tail():
    for C, HWs in ((1024, (1, 2, 3, 4, 5)), (256, (15, 16, 17))):
        for HW in HWs:
            run_sn(sn_t(2, 1, HW, C, 1, 1, 4, "un"), 1, HW, 32, f"spatial_norm UN tail C{C} HW{HW}")


@pytest.mark.parametrize("HW", [1023, 1024, 1025, 2049])
def test_spatial_norm_stats_chunks(HW):
    run_sn(sn_t(2, 1, HW, 32, 1, 1, 4, "stats"), 1, HW, 32, f"spatial_norm HW{HW}")


SN_PRODUCER = [(32, 64, k) for k in (1, 7, 8, 9)] + [(64, 128, k) for k in (3, 4, 5)]      # (G, C, stats_nchunk)


def producer_cuts(HW, k, seed):
    """k - 1 distinct sorted cut points in (0, HW): an arbitrary partition"""
    return sorted((torch.randperm(HW - 1, generator=S.gen(seed))[:k - 1] + 1).tolist())


@pytest.mark.parametrize("kind", ["randn", "1e3"])
def test_spatial_norm_producer_stats(kind):
    """float64 partial sums over an arbitrary partition: the same per-element bound as with self-computed statistics (+ the f64 allowance
    of the partition's longest part)"""
    H, W = 12, 25
    for G, C, k in SN_PRODUCER:
        t = sn_t(2, H, W, C, 4, 5, 4, ("prod", kind), kind=kind)
        run_sn(t, H, W, G, f"spatial_norm producer G{G} nchunk{k} {kind}", leg="spatial_norm" + ("_1e3" if kind == "1e3" else ""),
               cuts=producer_cuts(H * W, k, seed_of("cuts", G, k)), planes=(k == 9 or k == 5))


@pytest.mark.parametrize("kind", ["randn", "1e3", "const"])
def test_spatial_norm_inputs(kind):
    for B, H, W, C, G in ((2, 8, 12, 64, 32), (2, 33, 40, 128, 64)):
        out = run_sn(sn_t(B, H, W, C, H // 1, W // 4, 4, ("in", kind), kind=kind), H, W, G, f"spatial_norm {kind} {H}x{W} C{C} G{G}",
                     leg="spatial_norm" + {"randn": "", "1e3": "_1e3", "const": "_const"}[kind], planes=True)
        assert all(bool(torch.isfinite(o).all()) for o in out.values())


def test_spatial_norm_nan_confinement():
    """NaN in one group of one image reaches no other group and no other image"""
    B, H, W, C, G = 3, 5, 6, 64, 32
    t = sn_t(B, H, W, C, 5, 3, 4, "nan")
    mask = torch.zeros(B, H * W, C, dtype=torch.bool)
    mask[1, :, 6:8] = True                                          # group 3 of image 1
    t["x"][1, 17, 7] = S.NAN
    run_sn(t, H, W, G, "spatial_norm NaN in one group", nan_mask=mask)


def test_spatial_norm_batch_limit():
    """gridDim.y = 65535 is served; 65536 is refused by test_spatial_norm_refusals"""
    run_sn(sn_t(65535, 1, 1, 32, 1, 1, 4, "batch"), 1, 1, 32, "spatial_norm B65535")


def test_spatial_norm_refusals():
    """by return code, nothing launched: the outputs keep their sentinels and a following valid call gives the same bits as before"""
    L = _lib()
    B, H, W, zh, zw = 1, 4, 6, 2, 3
    t = sn_t(B, H, W, 2080, zh, zw, 4, "refuse")
    t9 = dict(t, wy=S.randn((2080, 9), 1), wb=S.randn((2080, 9), 2), zq=S.randn((B, zh, zw, 9), 3))
    prm, prm9 = ({k: op_in(d[k]) for k in ("gamma", "beta", "wy", "by", "wb", "bb", "zq")} for d in (t, t9))
    xi = op_in(t["x"], tail=0)
    spec = [(t["x"].numel(), F32), (128, F64)]
    pin = op_in(T.sn_producer_partials(t["x"].flatten()[:H * W * 64].view(1, H * W, 64), 32, [])[0], F64)

    def valid():       # (a producer's statistics: no atomicAdd in the chain, so the bits are reproducible)
        return twice("spatial_norm valid", spec[:1], lambda o: sn_call(L, xi.ptr, o.ptr, None, None, prm, pin.ptr, 1, B, H, W, 64, zh, zw, 4, 32, 1))[0]
    before = valid()
    for what, code, a in [("C 96", ERR_UNSUPPORTED, dict(C=96)), ("C 2080", ERR_UNSUPPORTED, dict(C=2080)), ("C 48", ERR_UNSUPPORTED, dict(C=48)),
                          ("groups 16", ERR_UNSUPPORTED, dict(G=16)), ("Z 0", ERR_UNSUPPORTED, dict(Z=0)), ("Z 9", ERR_UNSUPPORTED, dict(Z=9)),
                          ("H % zh", ERR_BAD_ARG, dict(H=5)), ("batch 65536", ERR_UNSUPPORTED, dict(B=65536))]:
        k = dict(B=B, H=H, C=64, Z=4, G=32)
        k.update(a)
        refused("spatial_norm " + what, code, spec, lambda o, p: sn_call(L, xi.ptr, o.ptr, None, None, prm9 if k["Z"] == 9 else prm, p.ptr, 0, k["B"],
                                                                      k["H"], W, k["C"], zh, zw, k["Z"], k["G"], 1))
    S.check_same_bits(before, valid(), "spatial_norm: a valid call after the refusals")


# =========================================================================================================================================
# b. muse_paella_mix_fwd
# =========================================================================================================================================
MIX_C = [4, 8, 12, 24, 252, 256, 260, 512, 516, 768, 772, 1024]
MIX_HW = [(1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (2, 3), (3, 3)]
MIX_G_C = [(1, 4), (2, 8), (4, 12), (8, 32), (16, 64), (32, 128), (64, 256)]           # a width C for every lane count G


def mix_row_shapes():
    out = []
    for G, C in MIX_G_C:
        assert T.mix_lanes(C) == G
        per = 256 // G
        for rows in sorted({1, per - 1, per, per + 1} - {0}):
            out.append((1, 1, rows, C))
    return out


def run_mix(x, w9, bias, g, what, tag=""):
    L = _lib()
    B, H, W, C = x.shape
    rows, n = B * H * W, x.numel()
    xi, wi, bi, gi = op_in(x, tail=0), op_in(w9), op_in(bias), op_in(g)
    st, y = twice(what, [(2 * rows, F32), (n, F32)],
                  lambda s, o: L.muse_paella_mix_fwd(xi.ptr, wi.ptr, bi.ptr, gi.ptr, s.ptr, o.ptr, B, H, W, C, _stream()))
    ref, sref, scale = T.ref_mix(x, w9, bias, g)
    body = judge("mix" + tag, what, y, n, ref, 4.0 * E_REF["mix" + tag] * scale + S.TINY)
    sb = S.check_out(st, 2 * rows, sref, what + " stats", values=False).view(rows, 2)
    ax = x.double().abs().view(rows, C).mean(1)
    note("ln_mean" + tag, what + " mean", S.worst_ratio(sb[:, 0], sref[:, 0], 4.0 * E_REF["ln_mean" + tag] * ax + S.TINY))
    note("ln_rstd" + tag, what + " rstd", S.worst_ratio(sb[:, 1], sref[:, 1], 4.0 * E_REF["ln_rstd" + tag] * sref[:, 1] + S.TINY))
    return body


def mix_case(B, H, W, C, tag="", onehot=False):
    return T.mix_inputs(B, H, W, C, seed_of("mix", B, H, W, C, tag, onehot), 1e3 if tag else 0.0, onehot)


@pytest.mark.parametrize("C", MIX_C)
def test_mix_channels(C):
    run_mix(*mix_case(3, 2, 3, C), f"mix C{C}")
    run_mix(*mix_case(3, 2, 3, C, onehot=True), f"mix C{C} one-hot taps")


def test_mix_row_counts():
    for B, H, W, C in mix_row_shapes():
        run_mix(*mix_case(B, H, W, C), f"mix rows{W} C{C}")


@pytest.mark.parametrize("H,W", MIX_HW)
def test_mix_neighbour_probe(H, W):
    """one-hot taps, a different tap per channel group: y - x is g2 times ONE neighbour's modulated value, so y is judged against x + that;
    zero padding, wrap-around, a clamp into the neighbouring image and swapped ky / kx each miss it by O(1) (tests/test_tokenizer_cpu.py)"""
    for C in (4, 24, 40):
        run_mix(*mix_case(3, H, W, C, onehot=True), f"mix probe {H}x{W} C{C}")
        run_mix(*mix_case(3, H, W, C), f"mix {H}x{W} C{C}")


MIX_ROUNDING = [(3, 2, 3, 4), (2, 7, 9, 96), (3, 5, 4, 260), (2, 3, 5, 772), (1, 3, 2, 1024)]


@pytest.mark.parametrize("tag", ["", "_1e3"])
def test_mix_rounding(tag):
    for B, H, W, C in MIX_ROUNDING:
        run_mix(*mix_case(B, H, W, C, tag), f"mix rounding{tag} B{B} {H}x{W} C{C}", tag)


@pytest.mark.parametrize("C", [4, 1024])
def test_mix_g2_zero_returns_x(C):
    x, w9, bias, g = mix_case(3, 3, 3, C)
    g[2] = 0.0
    L = _lib()
    xi, wi, bi, gi = op_in(x, tail=0), op_in(w9), op_in(bias), op_in(g)
    _, y = twice(f"mix g2 = 0 C{C}", [(2 * 27, F32), (x.numel(), F32)],
                 lambda s, o: L.muse_paella_mix_fwd(xi.ptr, wi.ptr, bi.ptr, gi.ptr, s.ptr, o.ptr, 3, 3, 3, C, _stream()))
    body = S.check_out(y, x.numel(), x, f"mix g2 = 0 C{C}")
    assert torch.equal(S.bits(body), S.bits(x.flatten())), "g2 = 0: y is x bit for bit"


def test_mix_refusals():
    L = _lib()
    x, w9, bias, g = mix_case(1, 2, 3, 1028)
    xi, xs, wi, bi, gi = op_in(x), op_in(x, shift=1), op_in(w9), op_in(bias), op_in(g)
    spec = [(2 * 6 + 1, F32), (x.numel() + 1, F32)]
    call = lambda xp, s, o, C=8: L.muse_paella_mix_fwd(xp, wi.ptr, bi.ptr, gi.ptr, s, o, 1, 2, 3, C, _stream())   # noqa: E731
    refused("mix C 1028", ERR_UNSUPPORTED, spec, lambda s, o: call(xi.ptr, s.ptr, o.ptr, 1028))
    refused("mix C 6", ERR_UNSUPPORTED, spec, lambda s, o: call(xi.ptr, s.ptr, o.ptr, 6))
    refused("mix x == y", ERR_BAD_ARG, spec, lambda s, o: call(xi.ptr, s.ptr, xi.ptr))
    refused("mix x 4 bytes off", ERR_ALIGN, spec, lambda s, o: call(xs.ptr, s.ptr, o.ptr))
    refused("mix y 4 bytes off", ERR_ALIGN, spec, lambda s, o: call(xi.ptr, s.ptr, o.ptr + 4))
    refused("mix stats 4 bytes off", ERR_ALIGN, spec, lambda s, o: call(xi.ptr, s.ptr + 4, o.ptr))
    assert bool(xi.t.cpu()[LEAD:LEAD + 48].eq(x.flatten()[:48]).all()), "x == y refused: x is unchanged"


# =========================================================================================================================================
# c. muse_patch_rows_nhwc
# =========================================================================================================================================
@pytest.mark.parametrize("KS,stride", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_patch_rows(KS, stride):
    """bit for bit on a coordinate ramp (the sign of -0.0 kept, padding +0); Hout / Wout one past what the image supports"""
    L = _lib()
    B, H, W = 2, 5, 6
    for pt in (0, 1):
        for pl in (0, 1):
            for C in (4, 8, 384):
                Ho, Wo = (H - 1 + pt) // stride + 2, (W - 1 + pl) // stride + 2
                assert (Ho - 1) * stride - pt >= H and (Wo - 1) * stride - pl >= W
                x = T.patch_ramp(B, H, W, C, seed_of("patch", KS, stride, pt, pl, C))
                exp = T.ref_patch_rows(x, KS, stride, pt, pl, Ho, Wo)
                xi = op_in(x, tail=0)
                what = f"patch_rows KS{KS} s{stride} pad{pt}{pl} C{C}"
                (y,) = twice(what, [(exp.numel(), F32)], lambda o: L.muse_patch_rows_nhwc(xi.ptr, o.ptr, B, H, W, C, KS, stride, pt, pl, Ho, Wo, _stream()))
                body = S.check_out(y, exp.numel(), exp, what)
                assert torch.equal(S.bits(body), S.bits(exp.flatten())), f"{what}: a sign of zero differs"
                assert bool((exp.view(B, Ho, Wo, -1)[:, -1] == 0).all()) and bool((exp.view(B, Ho, Wo, -1)[:, :, -1] == 0).all())


def test_patch_rows_refusals():
    L = _lib()
    x = T.patch_ramp(1, 4, 4, 8, 1)
    xi, xs = op_in(x), op_in(x, shift=1)
    spec = [(4 * 4 * 16 * 8 + 1, F32)]
    call = lambda xp, o, C=8, KS=2: L.muse_patch_rows_nhwc(xp, o, 1, 4, 4, C, KS, 1, 0, 0, 4, 4, _stream())   # noqa: E731
    refused("patch_rows KS 3", ERR_UNSUPPORTED, spec, lambda o: call(xi.ptr, o.ptr, KS=3))
    refused("patch_rows C 6", ERR_UNSUPPORTED, spec, lambda o: call(xi.ptr, o.ptr, C=6))
    refused("patch_rows x 4 bytes off", ERR_ALIGN, spec, lambda o: call(xs.ptr, o.ptr))
    refused("patch_rows y 4 bytes off", ERR_ALIGN, spec, lambda o: call(xi.ptr, o.ptr + 4))


# =========================================================================================================================================
# d. muse_vq_nearest_small
# =========================================================================================================================================
VQ_N = [1, 63, 64, 65, 129]


def vq_kcs(D):
    CH = T.vq_chunk(D)
    return [1, 2, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 1, 8192, 16384]


def vq_cases(D):
    """(Kc, N, ldz): every Kc, with N and ldz cycling so that each of them meets each D"""
    return [(Kc, VQ_N[(i + D) % 5], (D, D + 1, 16)[(i + D) % 3]) for i, Kc in enumerate(vq_kcs(D))]


def vq_launch(z, cb, ldz, what):
    """z [N, D] as a column slice of row stride ldz whose last row ends its allocation (NaN in the gaps and in front).  Returns (idx, dist)"""
    L = _lib()
    N, D = z.shape
    Kc = cb.shape[0]
    body = torch.full((N, ldz), S.NAN)
    body[:, :D] = z
    zi, ci = op_in(body.flatten()[:(N - 1) * ldz + D], tail=0), op_in(cb)
    ist, dst = twice(what, [(N, F64), (N, F32)], lambda i, d: L.muse_vq_nearest_small(zi.ptr, ldz, ci.ptr, i.ptr, d.ptr, N, D, Kc, _stream()))
    s = S.bits(S.sentinel(1, F64))[0]
    b = S.bits(ist)
    assert bool((b[:GUARD] == s).all()) and bool((b[GUARD + N:] == s).all()), f"{what}: wrote outside the index tensor"
    idx = b[GUARD:GUARD + N]
    assert not bool((idx == s).any()), f"{what}: an index was never written"
    sd = S.bits(S.sentinel(1, F32))[0]
    bd = S.bits(dst)
    assert bool((bd[:GUARD] == sd).all()) and bool((bd[GUARD + N:] == sd).all()), f"{what}: wrote outside the distance tensor"
    assert not bool((bd[GUARD:GUARD + N] == sd).any()), f"{what}: a distance was never written"
    return idx, dst[GUARD:GUARD + N]


def vq_exact_inputs(N, D, Kc, edge_ties=False):
    z, cb = T.vq_exact_case(N, D, Kc, seed_of("vqx", N, D, Kc), edge_ties)
    if N >= 63:
        z[1], z[2] = S.NAN, 3e38                                   # a NaN row; a row whose every distance overflows to +inf
    return z, cb


@pytest.mark.parametrize("D", range(1, 9))
def test_vq_exact(D):
    for Kc, N, ldz in vq_cases(D):
        for edge_ties in (False, True):
            z, cb = vq_exact_inputs(N, D, Kc, edge_ties)
            what = f"vq exact D{D} Kc{Kc} N{N} ldz{ldz} edge_ties{int(edge_ties)}"
            idx, dist = vq_launch(z, cb, ldz, what)
            T.check_vq_exact(idx, dist, z, cb, what)
            if N >= 63:
                assert idx[1] == 0 and idx[2] == 0, f"{what}: a NaN row and an all-inf row return 0"


def vq_seeded_inputs(N, D, Kc):
    sd = seed_of("vqs", N, D, Kc)
    return S.randn((N, D), sd), S.randn((Kc, D), sd + 1)


@pytest.mark.parametrize("D", range(1, 9))
def test_vq_seeded(D):
    for Kc, N, ldz in vq_cases(D):
        z, cb = vq_seeded_inputs(N, D, Kc)
        what = f"vq seeded D{D} Kc{Kc} N{N} ldz{ldz}"
        idx, dist = vq_launch(z, cb, ldz, what)
        w = T.check_vq_seeded(idx, dist, z, cb, what)
        WORST["vq_dist"] = max(WORST.get("vq_dist", 0.0), w)
        print(f"[tokenizer_edges] vq_dist {what}: err/margin={w:.3f} (worst so far {WORST['vq_dist']:.3f})")


@pytest.mark.parametrize("D", [3, 8])
def test_vq_rows_and_strides(D):
    CH = T.vq_chunk(D)
    for N in VQ_N:
        for ldz in (D, D + 1, 16):
            z, cb = vq_exact_inputs(N, D, CH + 1)
            what = f"vq rows D{D} N{N} ldz{ldz}"
            idx, dist = vq_launch(z, cb, ldz, what)
            T.check_vq_exact(idx, dist, z, cb, what)


# =========================================================================================================================================
# e. muse_paella_in_block / muse_paella_out_block
# =========================================================================================================================================
BLOCK_HW = [(2, 2), (2, 6), (6, 2), (4, 4), (6, 10)]
BLOCK_C = [4, 8, 12, 384]


def block_cases(probe):
    return [T.block_case(probe, 2, H, W, C, seed_of("block", probe, H, W, C)) for H, W in BLOCK_HW for C in BLOCK_C]


def run_blocks(c, shift=0):
    """both kernels on one case; shift = 1: the image pointer 4 bytes off (allowed).  Returns the two result bodies"""
    L = _lib()
    B, _, H, W = c["img"].shape
    C = c["w_in"].shape[1]
    ny, ni = B * (H // 2) * (W // 2) * C, c["img"].numel()
    what = f"{c['probe']} B{B} {H}x{W} C{C} shift{shift}"
    ii, wi, bi = op_in(c["img"], shift=shift, tail=0), op_in(c["w_in"]), op_in(c["b_in"])
    (y,) = twice("in_block " + what, [(ny, F32)], lambda o: L.muse_paella_in_block(ii.ptr, wi.ptr, bi.ptr, o.ptr, B, H, W, C, _stream()))
    xi, wo, bo = op_in(c["x"], tail=0), op_in(c["w_out"]), op_in(c["b_out"])
    (img,) = twice("out_block " + what, [(ni, F32, shift)], lambda o: L.muse_paella_out_block(xi.ptr, wo.ptr, bo.ptr, o.ptr, B, H, W, C, _stream()))
    ry, sy = T.ref_in_block(c["img"], c["w_in"], c["b_in"])
    ri, si = T.ref_out_block(c["x"], c["w_out"], c["b_out"])
    if c["exact"]:
        return S.check_out(y, ny, ry, "in_block " + what), S.check_out(img, ni, ri, "out_block " + what, guard=GUARD + shift)
    return (judge("in_block", "in_block " + what, y, ny, ry, 4.0 * E_REF["in_block"] * sy + S.TINY),
            judge("out_block", "out_block " + what, img, ni, ri, 4.0 * E_REF["out_block"] * si + S.TINY, guard=GUARD + shift))


@pytest.mark.parametrize("probe", ["int", "coord", "randn"])
def test_blocks(probe):
    for c in block_cases(probe):
        a, b = run_blocks(c), run_blocks(c, shift=1)
        S.check_same_bits(a[0], b[0], "in_block: image aligned against 4 bytes off")
        S.check_same_bits(a[1], b[1], "out_block: image aligned against 4 bytes off")


def test_blocks_refusals():
    L = _lib()
    c = T.block_case("int", 1, 4, 4, 8, 3)
    ii, wi, bi, ws = op_in(c["img"]), op_in(c["w_in"]), op_in(c["b_in"]), op_in(c["w_in"], shift=1)
    xi, xs, wo, bo = op_in(c["x"]), op_in(c["x"], shift=1), op_in(c["w_out"]), op_in(c["b_out"])
    spec = [(64, F32)]
    inb = lambda o, w=wi.ptr, H=4, W=4, C=8: L.muse_paella_in_block(ii.ptr, w, bi.ptr, o, 1, H, W, C, _stream())   # noqa: E731
    outb = lambda o, x=xi.ptr, w=wo.ptr, H=4, W=4, C=8: L.muse_paella_out_block(x, w, bo.ptr, o, 1, H, W, C, _stream())   # noqa: E731
    refused("in_block odd H", ERR_UNSUPPORTED, spec, lambda o: inb(o.ptr, H=3))
    refused("in_block odd W", ERR_UNSUPPORTED, spec, lambda o: inb(o.ptr, W=3))
    refused("in_block C 6", ERR_UNSUPPORTED, spec, lambda o: inb(o.ptr, C=6))
    refused("in_block w12 4 bytes off", ERR_ALIGN, spec, lambda o: inb(o.ptr, w=ws.ptr))
    refused("in_block y 4 bytes off", ERR_ALIGN, spec, lambda o: inb(o.ptr + 4))
    refused("out_block odd H", ERR_UNSUPPORTED, spec, lambda o: outb(o.ptr, H=3))
    refused("out_block odd W", ERR_UNSUPPORTED, spec, lambda o: outb(o.ptr, W=3))
    refused("out_block C 6", ERR_UNSUPPORTED, spec, lambda o: outb(o.ptr, C=6))
    refused("out_block x 4 bytes off", ERR_ALIGN, spec, lambda o: outb(o.ptr, x=xs.ptr))
    refused("out_block w12 4 bytes off", ERR_ALIGN, spec, lambda o: outb(o.ptr, w=ws.ptr))


# =========================================================================================================================================
# f. the 32768-block grid-stride cap of the four Paella kernels, C = 4
# =========================================================================================================================================
CAP = T.CAP_BLOCKS * 256


def dev_in(n, seed):
    """N(0, 1) made on the device, NaN in front and behind; returns (storage, pointer of the operand)"""
    st = torch.randn(n + 2 * LEAD, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    st[:LEAD] = S.NAN
    st[LEAD + n:] = S.NAN
    return st, st.data_ptr() + 4 * LEAD


def dev_out(n):
    st = S.alloc_out(n, F32).to(DEV)
    return st, st.data_ptr() + 4 * GUARD


def cap_compare(what, whole, parts, n):
    """the one-launch storage against the image-by-image one, bit for bit (guards included); guards intact, every slot written"""
    s = int(S.bits(S.sentinel(1, F32))[0])
    a, b = whole.view(torch.int32), parts.view(torch.int32)
    assert bool((a[:GUARD] == s).all()) and bool((a[GUARD + n:] == s).all()), f"{what}: a guard band was written"
    assert not bool((a[GUARD:GUARD + n] == s).any()), f"{what}: a slot was never written"
    assert torch.equal(a, b), f"{what}: the launch past the cap differs from the image-by-image launches"


def test_cap_mix():
    L = _lib()
    B, H, W, C = 3, 3, 932068, 4
    rows = H * W
    assert B * rows > CAP >= rows
    (xs, xp), w9, bias, g = dev_in(B * rows * C, 1), op_in(S.randn((9, C), 2) / 3), op_in(S.randn((C,), 3)), op_in(0.5 * S.randn((6,), 4))
    (ya, yap), (sa, sap), (yb, ybp), (sb, sbp) = dev_out(B * rows * C), dev_out(B * rows * 2), dev_out(B * rows * C), dev_out(B * rows * 2)
    assert L.muse_paella_mix_fwd(xp, w9.ptr, bias.ptr, g.ptr, sap, yap, B, H, W, C, _stream()) == 0
    for b in range(B):
        assert L.muse_paella_mix_fwd(xp + 4 * b * rows * C, w9.ptr, bias.ptr, g.ptr, sbp + 4 * b * rows * 2, ybp + 4 * b * rows * C, 1, H, W, C, _stream()) == 0
    torch.cuda.synchronize()
    cap_compare("mix y", ya, yb, B * rows * C)
    cap_compare("mix stats", sa, sb, B * rows * 2)


def test_cap_patch_rows():
    L = _lib()
    B, H, W, C, KS = 3, 1674, 1674, 4, 2
    Ho = Wo = H // 2
    per = Ho * Wo * KS * KS * C
    assert B * per // 4 > CAP >= per // 4
    xs, xp = dev_in(B * H * W * C, 5)
    (ya, yap), (yb, ybp) = dev_out(B * per), dev_out(B * per)
    assert L.muse_patch_rows_nhwc(xp, yap, B, H, W, C, KS, 2, 0, 0, Ho, Wo, _stream()) == 0
    for b in range(B):
        assert L.muse_patch_rows_nhwc(xp + 4 * b * H * W * C, ybp + 4 * b * per, 1, H, W, C, KS, 2, 0, 0, Ho, Wo, _stream()) == 0
    torch.cuda.synchronize()
    cap_compare("patch_rows", ya, yb, B * per)


def test_cap_in_block():
    L = _lib()
    B, H, W, C = 3, 4, 2 * 1398102, 4
    pix = (H // 2) * (W // 2)
    assert B * pix > CAP >= pix
    (xs, xp), w, bias = dev_in(B * 3 * H * W, 6), op_in(S.randn((12, C), 7)), op_in(S.randn((C,), 8))
    (ya, yap), (yb, ybp) = dev_out(B * pix * C), dev_out(B * pix * C)
    assert L.muse_paella_in_block(xp, w.ptr, bias.ptr, yap, B, H, W, C, _stream()) == 0
    for b in range(B):
        assert L.muse_paella_in_block(xp + 4 * b * 3 * H * W, w.ptr, bias.ptr, ybp + 4 * b * pix * C, 1, H, W, C, _stream()) == 0
    torch.cuda.synchronize()
    cap_compare("in_block", ya, yb, B * pix * C)


def test_cap_out_block():
    L = _lib()
    B, H, W, C = 3, 2, 2 * 466034, 4
    pix = (H // 2) * (W // 2)
    assert B * 3 * H * (W // 2) > CAP >= 3 * H * (W // 2)
    (xs, xp), w, bias = dev_in(B * pix * C, 9), op_in(S.randn((12, C), 10)), op_in(S.randn((12,), 11))
    (ya, yap), (yb, ybp) = dev_out(B * 3 * H * W), dev_out(B * 3 * H * W)
    assert L.muse_paella_out_block(xp, w.ptr, bias.ptr, yap, B, H, W, C, _stream()) == 0
    for b in range(B):
        assert L.muse_paella_out_block(xp + 4 * b * pix * C, w.ptr, bias.ptr, ybp + 4 * b * 3 * H * W, 1, H, W, C, _stream()) == 0
    torch.cuda.synchronize()
    cap_compare("out_block", ya, yb, B * 3 * H * W)


# =========================================================================================================================================
# E_ref: torch's float32 CPU computation against float64 over the same cases (python tests/test_gpu_tokenizer_edges.py; no GPU)
# =========================================================================================================================================
def mix_e_ref_cases():
    cases = [((3, 2, 3, C), "", oh) for C in MIX_C for oh in (False, True)] + [(s, "", False) for s in mix_row_shapes()]
    cases += [((3, H, W, C), "", oh) for H, W in MIX_HW for C in (4, 24, 40) for oh in (False, True)]
    return cases + [(s, tag, False) for tag in ("", "_1e3") for s in MIX_ROUNDING]


def measure_e_ref(cus=256):
    E = {}

    def put(name, got, ref, scale):
        E[name] = max(E.get(name, 0.0), S.measure(got, ref, scale))

    for (B, H, W, C), tag, oh in mix_e_ref_cases():
        x, w9, bias, g = mix_case(B, H, W, C, tag, oh)
        ref, sref, scale = T.ref_mix(x, w9, bias, g)
        ln = F.layer_norm(x, (C,), eps=T.LN_EPS) * (1 + g[0]) + g[1]
        pad = F.pad(ln.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate")
        got = x + g[2] * F.conv2d(pad, w9.t().reshape(C, 1, 3, 3), bias, groups=C).permute(0, 2, 3, 1)
        put("mix" + tag, got, ref, scale)
        rows = x.view(-1, C)
        put("ln_mean" + tag, rows.mean(1), sref[:, 0], rows.double().abs().mean(1))
        put("ln_rstd" + tag, torch.rsqrt(rows.var(1, unbiased=False) + T.LN_EPS), sref[:, 1], sref[:, 1])     # torch.var (biased), torch.rsqrt
    for c in block_cases("randn"):
        ry, sy = T.ref_in_block(c["img"], c["w_in"], c["b_in"])
        C = c["w_in"].shape[1]
        got = F.conv2d(F.pixel_unshuffle(c["img"], 2), c["w_in"].t().reshape(C, 12, 1, 1), c["b_in"]).permute(0, 2, 3, 1)
        put("in_block", got, ry, sy)
        ri, si = T.ref_out_block(c["x"], c["w_out"], c["b_out"])
        got = F.pixel_shuffle(F.conv2d(c["x"].permute(0, 3, 1, 2), c["w_out"].reshape(12, C, 1, 1), c["b_out"]), 2)
        put("out_block", got, ri, si)
    sn = [(sn_t(2, 4, 6, C, 2, 3, 4, "ch"), 4, 6, G, "") for C, G in SN_CHANNELS]
    sn += [(sn_t(2, 1, HW, 32, 1, 1, 4, "stats"), 1, HW, 32, "") for HW in (1023, 1024, 1025, 2049)]
    sn += [(sn_t(B, 1, HW, 32, 1, 1, 4, "apix"), 1, HW, 32, "") for v in sn_apix_cases(cus).values() for B, HW in v]
    sn += [(sn_t(B, H, W, C, H, W // 4, 4, ("in", kind), kind=kind), H, W, G, "_1e3" if kind == "1e3" else "")
           for kind in ("randn", "1e3") for B, H, W, C, G in ((2, 8, 12, 64, 32), (2, 33, 40, 128, 64))]
    for t, H, W, G, tag in sn:
        B, HW, C = t["x"].shape
        if HW * (C // G) == 1:                                     # one value per group: torch's group_norm refuses the shape
            continue
        r = T.ref_spatial_norm(t, H, W, G, EPS, 0)
        up = F.interpolate(t["zq"].permute(0, 3, 1, 2), size=(H, W), mode="nearest")
        m, a = F.conv2d(up, t["wy"][:, :, None, None], t["by"]), F.conv2d(up, t["wb"][:, :, None, None], t["bb"])
        got = F.group_norm(t["x"].transpose(1, 2).reshape(B, C, H, W), G, t["gamma"], t["beta"], EPS) * m + a
        put("spatial_norm" + tag, got.reshape(B, C, HW).transpose(1, 2), r["t"], r["n"].abs() * r["Sm"] + r["Sa"])
    return E


if __name__ == "__main__":
    torch.set_num_threads(8)
    t0 = time.time()
    for k, v in measure_e_ref().items():
        print(f'    "{k}": {v:.3e},')
    print(f"({time.time() - t0:.1f} s)", file=sys.stderr)
