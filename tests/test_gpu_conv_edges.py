"""GPU (-m gpu): the convolution family of csrc/ (gemm_core.h ConvLoader, conv_split.hip, conv_dma.hip, the direct kernels of vqgan.hip)
with EXACT probes at each edge of its dispatch, plus a per-element rounding leg and the host-side refusals.  tests/conv_cpu.py holds the
reference, the probes, the storage builders, the checks and a contract model; tests/test_conv_cpu.py proves on a CPU that the checks fail
for eleven seeded defects.  profiles/conv_edges.md has the edge table and the MI355X's figures; DESIGN.md ("Convolution contract") the
contract.

Every exact case (run_exact):
  * coordinate probe: input element (b, y, x, c) holds a seeded id its operand type carries exactly, the weights are one-hot per output
    channel - every output is ONE input element (or 0 in the padding) + integer bias + integer residual; dense probe: seeded small
    integers with every partial sum below 2^24 (conv_cpu.assert_exact).  The reference is float64 on the CPU (conv_cpu.ref_conv, written
    over the taps) and the result must equal it exactly in every accumulation order;
  * every operand sits inside a larger allocation with NaN in front of its offset and behind its end, the weight images continue with NaN
    rows past Cout, conv_in_direct's x has NaN in channels Cin .. Cpad - 1: a tap taken from the neighbouring row or image is a wrong id,
    a read outside the operand a NaN;
  * the output and the f64 GroupNorm partials are pre-filled with a NaN bit pattern no result has, guard bands on both sides: the guards
    must come back bit for bit and every slot must be written;
  * the case is launched twice from the same initial output: bit-identical;
  * GroupNorm partials are compared per (image, chunk, group) SLOT with the path's own chunk map (conv_cpu.partials_ref), not after summing.

Edges (thresholds as the code has them; file: function):
  muse_conv2d_nhwc f32 / bf16, muse_conv2d_nhwc_split (gemm_core.h: ConvLoader, gemm_kernel; conv_split.hip: conv_split_kernel) - 128 x 128
  x 64 tile
    (B, H, W): (1,1,1) (1,1,7) (7,1,1): W = 1 / H = 1; (3,5,7): one tile over three images; (1,8,16): M = 128; (1,3,43): M = 129;
      (1,127,1): M = 127; (2,9,13): two tiles, image change inside the second
    Cin {4, 8, 12, 20, 64, 68} f32, {8, 16, 24, 40, 64, 72} bf16 / split: ConvLoader::load shift (power of two) against division; K tails
      (K = 9 * 8 = 72 = 64 + 8; KS = 1: K = Cin < 64)
    Cout {1, 3, 4, 5, 127, 128, 129, 132}: Cout % 4 != 0 takes the scalar epilogue; 1 / 2 column tiles, ragged
    KS {1, 3} x upsample {0, 1, 2}: 1 = nearest x2 in the index math (even H, W); 2 = stride 2, output (1,1) (1,5) (5,7)
    muse_conv2d_nhwc_split gn_partial: cpg {4, 8, 16, 32}, H * W in {128, 256}; refused outside (cpg 2 / 64, H * W = 192)
  muse_conv2d_nhwc_split2 tap-major (conv_dma.hip: conv_dma_kernel) - 256 x 128 x 32 tile, taken when H or W % 16 != 0 or Cin % 64 != 0
    Cin {32, 96, 160}: 9 / 27 / 45 K-tiles (the loop is padded to a multiple of 6); M around 256 / 512: (1,15,17) = 255, (1,257,1),
    (1,1,257), (2,16,17) = 544, (3,9,19) = 513; Cout {4, 124, 128, 132, 260}; partials where (H * W) % 256 == 0: (1,16,48), (2,32,8)
  slab kernels (conv_dma.hip: conv_slab_kernel<GN, POOL>; muse_conv2d_nhwc_split2 on H, W % 16 == 0 and Cin % 64 == 0,
  muse_conv2d_nhwc_gn_split2, muse_conv2d_nhwc_gn_split2_pool)
    (B, H, W): (1,16,16): every halo row is padding; (2,16,32) (2,32,16): image change; (1,48,48): an interior patch with eight neighbours
    Cin {64, 128, 192, 256, 320}: 2 .. 10 channel chunks (double-buffer parity), P_GSS_MAX_CIN = 256 against 320
    Cout {4, 64, 124, 128, 132, 256}; partials: groups 32 / 64, cpg {4, 8, 16, 32, 64, 128}
  persistent kernels (conv_dma.hip: conv_slab_persist_kernel<GN, POOL>, conv_gn_split2_launch)
    default route in process: tiles in {2 CUs - 1, 2 CUs, 2 CUs + 1} (taken when tiles >= 2 x CUs), Cin 64, Cout 8
    child interpreters (the library reads the switches once): MUSE_CONV_PERSIST_GRID = 3 | 8, MUSE_CONV_PERSIST_TILES = 2 with
    MUSE_CONV_PERSIST_MIN = 0, MUSE_CONV_SLAB = 0 (tap-major kernel on slab shapes), MUSE_CONV_SLAB = 2 (conv_slab_persist_kernel<false>,
    grid = min(tiles, CUs): more tiles than CUs - 2 CUs + 1 in one column tile, two images x two column tiles - make it walk)
  muse_conv_in_direct / _nchw (vqgan.hip: conv_in_direct_kernel): Cin 1 .. 4, Cpad {4, 8}, Cout {4, 8, 32, 128, 256, 1024} (qpp 1 .. 256),
    W {1, 2, pstep - 1, pstep, pstep + 1, 257, 1022} with pstep = 256 / qpp, refused at 1023; H {1, 2, 3}; B = 2; partials per image row
  muse_conv_out_direct (vqgan.hip: conv_out_direct_kernel): C {32, 64, 96}, Cout 1 .. 4, (H, W) {(16,16), (16,32), (48,48)}, B = 2
"""
import ctypes as C
import os
import subprocess
import sys
import zlib

import pytest
import torch

import conv_cpu as Cv
from conv_cpu import BF, F32, F64, GUARD, LEAD

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_BAD_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3
SLAB_ENV = int(os.environ.get("MUSE_CONV_SLAB", "1") or 1)       # what the library reads once per process


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """a launch that faulted leaves the device unusable for the rest of the process: end the session there rather than start more work"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU error after a convolution edge test, stopping: {e}", returncode=3)


def _ops():
    from muse import ops
    return ops


def _lib():
    from muse._hip import lib
    return lib()


def _stream():
    from muse.ops import stream
    return stream()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed & 0x7FFFFFFF), dtype=F64) * scale).float()


class Op:
    """an operand storage of conv_cpu.place on the device and the address of the operand inside it"""

    def __init__(self, st, lead=LEAD):
        self.t = st.to(DEV)
        self.ptr = self.t.data_ptr() + lead * st.element_size()
        assert self.ptr % 16 == 0


def op(st):
    return Op(st) if st is not None else None


def p_(o):
    return o.ptr if o is not None else None


def fresh_out(n, dtype):
    return Op(Cv.alloc_out(n, dtype), GUARD)


def slab_shape(H, W, Cin):
    return H % 16 == 0 and W % 16 == 0 and Cin % 64 == 0


def split2_map(H, W, Cin):
    """the chunk map of muse_conv2d_nhwc_split2's partials: the kernel that runs decides"""
    return "slab" if slab_shape(H, W, Cin) and SLAB_ENV != 0 else "tap"


# =========================================================================================================================================
# the exact runner
# =========================================================================================================================================
def launch_case(c, d, out, part, groups):
    L, B, H, W, Cin, Cout, KS, ups = _lib(), c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["KS"], c["ups"]
    if c["path"] in ("f32", "bf16"):
        assert part is None
        return L.muse_conv2d_nhwc(d["x"].ptr, d["w"][0].ptr, p_(d["bias"]), p_(d["res"]), out.ptr, 1 if c["path"] == "bf16" else 0, B, H, W,
                                  Cin, Cout, KS, ups, _stream())
    if c["path"] == "split":
        return L.muse_conv2d_nhwc_split(d["x"].ptr, d["w"][0].ptr, d["w"][1].ptr, p_(d["bias"]), p_(d["res"]), out.ptr, p_(part), groups, B, H, W,
                                        Cin, Cout, KS, ups, _stream())
    assert c["path"] == "split2" and ups == 0
    return L.muse_conv2d_nhwc_split2(d["p"][0].ptr, d["p"][1].ptr, d["w"][0].ptr, d["w"][1].ptr, p_(d["bias"]), p_(d["res"]), out.ptr, p_(part),
                                     groups, B, H, W, Cin, Cout, KS, _stream())


def to_dev(c):
    d = dict(w=[Op(w) for w in c["w_st"]], res=op(c["res_st"]), bias=None, p=None, x=None)
    if c["bias_t"] is not None:
        d["bias"] = Op(Cv.place(c["bias_t"], F32))
    if c["path"] == "split2":
        d["p"] = [Op(p) for p in c["planes"]]
    else:
        d["x"] = Op(c["x_st"] if c["path"] == "split" else c["planes"][0])
    return d


def run_exact(c, gn=None, what=""):
    """gn = (map, groups): also the partials, compared per slot"""
    d = to_dev(c)
    exp = c["expected"]
    n = exp.numel()
    pexp = Cv.partials_ref(exp, gn[0], gn[1]) if gn else None
    if gn:
        assert float(pexp.abs().max()) < 2.0 ** 53, "the probe's squares do not stay exact in f64"
    got = []
    for _ in range(2):
        out = fresh_out(n, c["out_dtype"])
        part = fresh_out(pexp.numel(), F64) if gn else None
        rc = launch_case(c, d, out, part, gn[1] if gn else 0)
        assert rc == 0, f"{what}: the entry returned {rc}"
        got.append((out.t.cpu(), part.t.cpu() if gn else None))
    Cv.check_same_bits(got[0][0], got[1][0], what)
    Cv.check_out(got[0][0], n, exp, what)
    if gn:
        Cv.check_same_bits(got[0][1], got[1][1], what + " partials")
        Cv.check_partials(got[0][1], pexp, what)


def both_probes(path, B, H, W, Cin, Cout, KS=3, ups=0, bias=False, res=False, gn=None):
    for probe in ("coord", "dense"):
        what = f"{path} {probe} B{B} {H}x{W} Cin{Cin} Cout{Cout} KS{KS} ups{ups} bias{int(bias)} res{int(res)} gn{gn}"
        c = Cv.build_case(path, probe, B, H, W, Cin, Cout, KS, ups, bias, res, seed=seed_of(what))
        run_exact(c, gn, what)


# =========================================================================================================================================
# a. ConvLoader paths: muse_conv2d_nhwc (f32, bf16) and muse_conv2d_nhwc_split
# =========================================================================================================================================
BHW = [(1, 1, 1), (1, 1, 7), (7, 1, 1), (3, 5, 7), (1, 8, 16), (1, 3, 43), (1, 127, 1), (2, 9, 13)]
CIN = {"f32": [4, 8, 12, 20, 64, 68], "bf16": [8, 16, 24, 40, 64, 72], "split": [8, 16, 24, 40, 64, 72]}
COUT = [1, 3, 4, 5, 127, 128, 129, 132]


def loader_cases():
    """a pruned cross product: every (B, H, W) with every Cin and every Cout at least once per path, bias / residual cycling through their
    four combinations; then every KS x upsample mode"""
    cases = []
    for path in ("f32", "bf16", "split"):
        i = 0
        for s, bhw in enumerate(BHW):
            for j in range(2):                                   # two (Cin, Cout) pairs per shape: 16 per path, each value at least twice
                cin, cout = CIN[path][(2 * s + j) % 6], COUT[(3 * s + 5 * j + i) % 8]
                cases.append((path, *bhw, cin, cout, 3, 0, bool(i & 1), bool(i & 2)))
                i += 1
        # Cout values the walk above may have left out at 3 x 3, on the two-tile shape
        for k, cout in enumerate(COUT):
            cases.append((path, 2, 9, 13, CIN[path][k % 6], cout, 3, 0, bool(k & 2), bool(k & 1)))
        # KS = 1 and the upsample modes: 1 needs even output dims; 2 the output sizes (1,1), (1,5), (5,7)
        cases += [(path, 3, 5, 7, CIN[path][3], 5, 1, 0, True, True), (path, 1, 3, 43, CIN[path][5], 129, 1, 0, False, True),
                  (path, 2, 2, 2, CIN[path][0], 4, 1, 1, True, False), (path, 1, 6, 14, CIN[path][2], 132, 1, 1, False, True),
                  (path, 2, 4, 6, CIN[path][1], 5, 3, 1, True, True), (path, 1, 10, 26, CIN[path][5], 129, 3, 1, False, True),
                  (path, 3, 2, 2, CIN[path][4], 3, 3, 1, True, False),
                  (path, 2, 1, 1, CIN[path][0], 4, 3, 2, True, True), (path, 3, 1, 5, CIN[path][3], 5, 3, 2, False, True),
                  (path, 4, 5, 7, CIN[path][5], 129, 3, 2, True, False)]
    return cases


@pytest.mark.parametrize("case", loader_cases(), ids=lambda c: "-".join(str(int(v)) if not isinstance(v, str) else v for v in c))
def test_loader_paths_exact(case):
    """gemm_core.h ConvLoader under gemm_kernel (f32, bf16) and conv_split_kernel: both probes at every shape / channel / mode edge"""
    path, B, H, W, Cin, Cout, KS, ups, bias, res = case
    both_probes(path, B, H, W, Cin, Cout, KS, ups, bias, res)


@pytest.mark.parametrize("cpg", [4, 8, 16, 32])
@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (3, 16, 16)], ids=["hw128", "hw256"])
def test_split_partials_per_chunk(B, H, W, cpg):
    """conv_split_kernel's GroupNorm partials: per (image, 128-pixel chunk, group) slot, exact; Cout = 32 cpg (128 .. 1024: 1 .. 8 column tiles)"""
    both_probes("split", B, H, W, 8, 32 * cpg, 3, 0, True, True, gn=("split", 32))


def test_split_partials_refusals():
    """outside cpg {4, 8, 16, 32} or H * W % 128 == 0 the entry refuses before it launches"""
    L = _lib()
    buf = torch.zeros(4096, device=DEV)
    a = buf.data_ptr()
    for groups, H, W, Cout in [(32, 8, 16, 64), (32, 8, 16, 2048), (32, 8, 24, 128), (0, 8, 16, 128), (32, 8, 16, 132)]:
        assert L.muse_conv2d_nhwc_split(a, a, a, None, None, a, a, groups, 1, H, W, 8, Cout, 3, 0, _stream()) == ERR_UNSUPPORTED
    ops = _ops()
    x = torch.zeros(1, 8, 24, 8, device=DEV)
    wh = torch.zeros(128, 3, 3, 8, dtype=BF, device=DEV)
    assert not hasattr(ops.conv2d_nhwc_split(x, wh, wh, 1, 8, 24, 8, 128, 3, gn_groups=32), "_gn_stats")


# =========================================================================================================================================
# b. muse_conv2d_nhwc_split2, tap-major kernel
# =========================================================================================================================================
TAP_BHW = [(1, 15, 17), (1, 257, 1), (1, 1, 257), (2, 16, 17), (3, 9, 19)]
TAP_COUT = [4, 124, 128, 132, 260]


@pytest.mark.parametrize("B,H,W", TAP_BHW, ids=lambda v: str(v))
@pytest.mark.parametrize("Cin", [32, 96, 160])
def test_tap_major_exact(Cin, B, H, W):
    """conv_dma_kernel: 9 / 27 / 45 K-tiles against the loop's multiple of 6, M around one and two 256-pixel tiles, every Cout edge"""
    i = TAP_BHW.index((B, H, W)) + [32, 96, 160].index(Cin)
    both_probes("split2", B, H, W, Cin, TAP_COUT[i % 5], 3, 0, bool(i & 1), bool(i & 2))
    if Cin == 96:
        both_probes("split2", B, H, W, 32, TAP_COUT[(i + 2) % 5], 3, 0, True, True)


@pytest.mark.parametrize("B,H,W,Cin,Cout,groups", [(1, 16, 48, 32, 128, 32), (2, 32, 8, 96, 256, 64), (2, 8, 32, 32, 256, 64)])
def test_tap_major_partials_per_chunk(B, H, W, Cin, Cout, groups):
    """the 256-pixel tile is the chunk: (H * W) % 256 == 0 with W no multiple of 16, or Cin % 64 != 0 (slab shapes excluded)"""
    assert not slab_shape(H, W, Cin)
    both_probes("split2", B, H, W, Cin, Cout, 3, 0, True, True, gn=("tap", groups))


# =========================================================================================================================================
# c. slab kernels
# =========================================================================================================================================
SLAB_BHW = [(1, 16, 16), (2, 16, 32), (2, 32, 16), (1, 48, 48)]
SLAB_CIN = [64, 128, 192, 256, 320]
SLAB_COUT = [4, 64, 124, 128, 132, 256]


SLAB_PARTIALS = [(g, c) for c in (4, 8, 16, 32, 64, 128) for g in (32, 64)]


def slab_cases():
    cases = []
    for s, bhw in enumerate(SLAB_BHW):
        for j, cin in enumerate(SLAB_CIN):
            if bhw == (1, 48, 48) and cin not in (64, 320):      # the nine-patch image at the smallest and the largest chunk count
                continue
            k = s + j
            cases.append((*bhw, cin, SLAB_COUT[k % 6], bool(k & 1), bool(k & 2)))
    return cases


@pytest.mark.parametrize("B,H,W,Cin,Cout,bias,res", slab_cases(), ids=lambda v: str(int(v)))
def test_slab_split2_exact(B, H, W, Cin, Cout, bias, res):
    """muse_conv2d_nhwc_split2 on slab shapes (conv_slab_kernel<false>; MUSE_CONV_SLAB=0: conv_dma_kernel, =2: conv_slab_persist_kernel<false>)"""
    both_probes("split2", B, H, W, Cin, Cout, 3, 0, bias, res)


@pytest.mark.parametrize("groups,cpg", SLAB_PARTIALS)
def test_slab_partials_per_chunk(groups, cpg):
    """the 16 x 16 patch img * tpi + prem is the chunk; Cin = 64, H * W = 256 per patch, two images of two patches"""
    B, H, W = 2, 16, 32
    both_probes("split2", B, H, W, 64, groups * cpg, 3, 0, True, True, gn=(split2_map(H, W, 64), groups))


def patch_grid(p):
    """(th, tw) with th * tw == p, as square as p's factors allow"""
    th = max(d for d in range(1, int(p ** 0.5) + 1) if p % d == 0)
    return th, p // th


def persist_walk_changes(ntm, ntn, grid, tpi):
    """conv_slab_persist_kernel's walk (conv_dma.hip: geo_of; workgroup g takes v = g, g + grid, ...; v -> tile by the XCD-aware map of
    the launch-per-tile kernels): does some workgroup change its column tile / its image (tpi patches each) between two consecutive tiles?"""
    ntiles = ntm * ntn
    bq, br = ntiles >> 3, ntiles & 7

    def tile(v):
        xcd, bi = v & 7, v >> 3
        return (xcd * (bq + 1) if xcd < br else br * (bq + 1) + (xcd - br) * bq) + bi
    ncross = mcross = False
    for g in range(min(grid, ntiles)):
        t = [tile(v) for v in range(g, ntiles, grid)]
        for a, b in zip(t, t[1:]):
            ncross |= a % ntn != b % ntn
            mcross |= a // ntn // tpi != b // ntn // tpi
    return ncross, mcross


@pytest.mark.parametrize("which", ["one-column-tile", "three-column-tiles", "partials"])
def test_slab_split2_more_tiles_than_cus(which):
    """muse_conv2d_nhwc_split2 with more tiles than the device has CUs, both probes.  Under MUSE_CONV_SLAB=2 the grid of
    conv_slab_persist_kernel<false> is min(tiles, CUs) (MUSE_CONV_PERSIST_GRID / _TILES do not reach it), so only here does a workgroup of
    that kernel walk on to a second and third tile: its look-ahead into the next tile (issue_slab / issue_b with chunk == nchunks,
    slab_off_n / voffB_n) and the staging epilogue against the next tile's DMAs run.  2 CUs + 1 tiles in one column tile of one image; two
    images of ceil((CUs + 1) / 2) patches in THREE column tiles (Cout 260, Cin 128: 4 chunks): a workgroup's next tile is CUs / 8 tiles
    on in the walk, which two column tiles would divide on every CU count that is a multiple of 16 - with three the column tile (voffB_n,
    the epilogue's n0) changes at every step, and the walk crosses the image change; persist_walk_changes asserts both for the device at
    hand.  CUs + 1 tiles with the GroupNorm partials, per patch slot"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if which == "one-column-tile":
        B, H, W = tiles_shape(2 * ncu + 1)
        Cin, Cout, tiles = 64, 8, 2 * ncu + 1
    elif which == "three-column-tiles":
        th, tw = patch_grid((ncu + 2) // 2)
        B, H, W, Cin, Cout = 2, 16 * th, 16 * tw, 128, 260
        tiles = 2 * th * tw * 3
        ncross, mcross = persist_walk_changes(2 * th * tw, 3, ncu, th * tw)
        assert ncross and mcross, f"on {ncu} CUs no workgroup of this case changes its column tile / its image between two tiles"
    else:
        B, H, W = tiles_shape(ncu + 1)
        Cin, Cout, tiles = 64, 128, ncu + 1
    assert tiles > ncu and slab_shape(H, W, Cin)
    both_probes("split2", B, H, W, Cin, Cout, 3, 0, True, True, gn=(split2_map(H, W, Cin), 32) if which == "partials" else None)


def gn_planes_ok(Cin):
    """channel counts muse_groupnorm_silu_nhwc_split takes (vqgan.hip: 256 % (C / 4) == 0): 64, 128, 256 of the slab list, not 192 / 320"""
    return 256 % (Cin // 4) == 0


def gn_inputs(B, H, W, Cin, seed):
    """x, the planes muse_groupnorm_silu_nhwc_split writes from it, and the (scale, shift) of the same statistics.  Where that kernel
    does not take Cin there are no planes and (scale, shift) are seeded: the fused convolution takes any"""
    ops, L = _ops(), _lib()
    from muse.ops import check
    x = Op(Cv.place(rnd((B, H, W, Cin), seed, 1.5), F32))
    n = B * H * W * Cin
    body = lambda o: o.t[LEAD:LEAD + n].view(B, H, W, Cin).cpu()
    g = dict(x=x, x_c=body(x), hi=None)
    if gn_planes_ok(Cin):
        gamma, beta = (1.0 + 0.2 * rnd((Cin,), seed + 1)).to(DEV), (0.3 * rnd((Cin,), seed + 2)).to(DEV)
        nchunk = L.muse_groupnorm_nchunk(H * W)
        part = torch.empty(B * nchunk * 32 * 2, dtype=F64, device=DEV)
        hi, lo = Op(Cv.place(torch.zeros(n), BF)), Op(Cv.place(torch.zeros(n), BF))
        check(L.muse_groupnorm_silu_nhwc_split(x.ptr, hi.ptr, lo.ptr, gamma.data_ptr(), beta.data_ptr(), part.data_ptr(), 0, B, H * W, Cin, 32,
                                               1e-6, 1, _stream()), "muse_groupnorm_silu_nhwc_split")
        sc, sh = ops.groupnorm_scale_shift((part, nchunk), gamma, beta, B, H * W, Cin)
        g.update(hi=hi, lo=lo, hi_c=body(hi), lo_c=body(lo))
    else:
        sc, sh = (1.0 + 0.3 * rnd((B, Cin), seed + 1)).to(DEV), (0.5 * rnd((B, Cin), seed + 2)).to(DEV)
    # the tables the convolution reads sit between NaN like every other operand (the persistent kernel copies the current AND the next
    # image's rows into LDS: a row past the last image would be NaN)
    g.update(sc=Op(Cv.place(sc.cpu(), F32)), sh=Op(Cv.place(sh.cpu(), F32)), sc_c=sc.cpu(), sh_c=sh.cpu())
    return g


def launch_gn(g, w, bias, res, out, part, groups, B, H, W, Cin, Cout, pool, persistent=1):
    fn = _lib().muse_conv2d_nhwc_gn_split2_pool if pool else _lib().muse_conv2d_nhwc_gn_split2
    rc = fn(g["x"].ptr, g["sc"].ptr, g["sh"].ptr, w[0].ptr, w[1].ptr, p_(bias), p_(res), out.ptr, p_(part), groups, B, H, W, Cin,
            Cout, 3, persistent, _stream())
    assert rc == 0, rc


def gn_coordinate_check(g, B, H, W, Cin, Cout, what, pool_too=True):
    """one-hot weights: every output is hi + lo of ONE activation (exact in f32) or 0 in the padding - bit for bit against the planes
    muse_groupnorm_silu_nhwc_split wrote, and per element against float64 silu(x * scale + shift) within conv_cpu.bound_act"""
    w1, _, _ = Cv.onehot_weights(Cout, 3, Cin, seed_of(what))
    w = [Op(Cv.place_weights(w1, BF)), Op(Cv.place_weights(torch.zeros_like(w1), BF))]
    n = B * H * W * Cout
    outs = []
    for _ in range(2):
        out = fresh_out(n, F32)
        launch_gn(g, w, None, None, out, None, 0, B, H, W, Cin, Cout, False)
        outs.append(out.t.cpu())
    Cv.check_same_bits(outs[0], outs[1], what)
    t = g["x_c"].double() * g["sc_c"].double()[:, None, None, :] + g["sh_c"].double()[:, None, None, :]
    ref = Cv.ref_conv(g["x_c"], w1, H, W, 3, scale=g["sc_c"], shift=g["sh_c"])
    bound = Cv.ref_conv(Cv.bound_act(t, planes=True), w1, H, W, 3) + 1e-30
    body = Cv.check_out(outs[0], n, ref, what + " against float64", values=False)      # guards, written, no NaN
    if g["hi"] is not None:
        Cv.check_out(outs[0], n, Cv.ref_conv(g["hi_c"].double() + g["lo_c"].double(), w1, H, W, 3), what + " against the planes")
    assert bool((body.view_as(ref)[ref == 0] == 0).all()), f"{what}: a padding tap is not zero"
    err = float(((body.double().view_as(ref) - ref).abs() / bound).max())
    print(f"[conv_edges] {what}: activation error / bound = {err:.3f}")
    assert err <= 1.0, f"{what}: the fused activation is {err:.3f} x its derived bound away from float64"
    if pool_too:
        pout = fresh_out(n // 4, F32)
        launch_gn(g, w, None, None, pout, None, 0, B, H, W, Cin, Cout, True)
        Cv.check_out(pout.t.cpu(), n // 4, Cv.pool2(body.view(B, H, W, Cout)), what + " pooled")


def gn_cases():
    cases = []
    for s, bhw in enumerate(SLAB_BHW):
        for j, cin in enumerate(SLAB_CIN):
            if (s + j) % 2 and bhw != (1, 16, 16):               # every shape with 2 - 3 chunk counts; (1,16,16) with all five
                continue
            cases.append((*bhw, cin, SLAB_COUT[(s + 2 * j + 1) % 6]))
    return cases


@pytest.mark.parametrize("B,H,W,Cin,Cout", gn_cases(), ids=lambda v: str(v))
def test_slab_gn_forms(B, H, W, Cin, Cout):
    """conv_slab_kernel<true> / <true, true> (children: conv_slab_persist_kernel<true, POOL>): the coordinate probe against the planes and
    float64; dense: bit-identity with muse_conv2d_nhwc_split2 on those planes (which the integer probes judge independently), partials
    included; pooled: the f32 expression (((v0 + v1) + v2) + v3) * 0.25 of the un-pooled GPU output, evaluated on the CPU"""
    what = f"gn_split2 B{B} {H}x{W} Cin{Cin} Cout{Cout}"
    sd = seed_of(what)
    assert _ops().conv_gn_split2_ok(B, H, W, Cin, Cout, 3)
    g = gn_inputs(B, H, W, Cin, sd)
    gn_coordinate_check(g, B, H, W, Cin, Cout, what)
    # dense
    wf = rnd((Cout, 3, 3, Cin), sd + 5, 1.0 / (3.0 * Cin ** 0.5))
    wh, wl = Cv.split_hi_lo(wf)
    w = [Op(Cv.place_weights(wh, BF)), Op(Cv.place_weights(wl, BF))]
    bias, res = Op(Cv.place(rnd((Cout,), sd + 6, 0.1), F32)), Op(Cv.place(rnd((B, H, W, Cout), sd + 7), F32))
    groups = 32 if Cout % 128 == 0 else 0
    n = B * H * W * Cout
    pn = B * (H * W // 256) * groups * 2
    o_gn, o_pool = fresh_out(n, F32), fresh_out(n // 4, F32)
    p_gn, p_pool = (fresh_out(pn, F64), fresh_out(pn, F64)) if groups else (None, None)
    launch_gn(g, w, bias, res, o_gn, p_gn, groups, B, H, W, Cin, Cout, False)
    launch_gn(g, w, bias, res, o_pool, p_pool, groups, B, H, W, Cin, Cout, True)
    gn_c, pool_c = o_gn.t.cpu(), o_pool.t.cpu()
    bias_c, res_c = bias.t[LEAD:LEAD + Cout].cpu(), res.t[LEAD:LEAD + n].view(B, H, W, Cout).cpu()
    t = g["x_c"].double() * g["sc_c"].double()[:, None, None, :] + g["sh_c"].double()[:, None, None, :]
    ref = Cv.ref_conv(g["x_c"], wf, H, W, 3, bias=bias_c, residual=res_c, scale=g["sc_c"], shift=g["sh_c"])
    bound = Cv.bound_x3(Cv.abs_terms(Cv.silu64(t), wf, H, W, 3, 0, bias_c, res_c), 9 * Cin) + Cv.ref_conv(Cv.bound_act(t), wf.abs(), H, W, 3)
    body = Cv.check_out(gn_c, n, ref, what + " dense against float64", exact=False, bound=bound)
    p_ref = None
    if g["hi"] is not None:
        # split2 on the planes: bit-identical, partials included, when it runs a slab kernel (same K order: chunk, tap, channel); the
        # tap-major kernel (MUSE_CONV_SLAB=0) sums the same products in (tap, channel) order and is judged against float64 alone
        o_ref, p_ref = fresh_out(n, F32), fresh_out(pn, F64) if groups else None
        rc = _lib().muse_conv2d_nhwc_split2(g["hi"].ptr, g["lo"].ptr, w[0].ptr, w[1].ptr, bias.ptr, res.ptr, o_ref.ptr, p_(p_ref), groups, B, H, W,
                                            Cin, Cout, 3, _stream())
        assert rc == 0
        ref_body = Cv.check_out(o_ref.t.cpu(), n, ref, what + " split2 on the planes", exact=False, bound=bound)
        if split2_map(H, W, Cin) == "slab":
            Cv.check_out(gn_c, n, ref_body, what + " dense against split2")
    Cv.check_out(pool_c, n // 4, Cv.pool2(body.view(B, H, W, Cout)), what + " dense pooled")
    if groups:
        pg, pp = p_gn.t.cpu(), p_pool.t.cpu()
        if p_ref is not None and split2_map(H, W, Cin) == "slab":
            Cv.check_partials(pg, p_ref.t.cpu()[GUARD:GUARD + pn].view(B, -1, groups, 2), what + " partials against split2")
        for st, o, m in ((pg, body.view(B, H, W, Cout), "slab"), (pp, Cv.pool2(body.view(B, H, W, Cout)), "pool")):
            e = Cv.partials_ref(o, m, groups)                       # f64 sums of f32 values: the order shows at 1e-16, a wrong slot at 1
            Cv.check_out(st, pn, e, what + " " + m + " partials", exact=False, bound=1e-12 * e.abs() + 1e-12)


@pytest.mark.parametrize("B,H,W,Cout,groups", [(2, 16, 32, 128, 32), (1, 48, 48, 256, 64), (2, 32, 16, 128, 0)])
def test_pooled_partials_per_chunk(B, H, W, Cout, groups):
    """the pooled epilogue alone with integers: zero weights, integer bias and residual - every pooled output is a multiple of 1 / 4,
    exact in any order, and each (image, patch, group) slot holds the sums of the patch's 64 pooled pixels"""
    what = f"pooled integers B{B} {H}x{W} Cout{Cout} g{groups}"
    sd = seed_of(what)
    Cin = 64
    g = gn_inputs(B, H, W, Cin, sd)
    z = torch.zeros(Cout, 3, 3, Cin)
    w = [Op(Cv.place_weights(z, BF)), Op(Cv.place_weights(z, BF))]
    bvec, rten = Cv.ints((Cout,), 50, sd + 1), Cv.ints((B, H, W, Cout), 1000, sd + 2)
    bias, res = Op(Cv.place(bvec, F32)), Op(Cv.place(rten, F32))
    exp = Cv.pool2((rten + bvec).double())
    n = exp.numel()
    pexp = Cv.partials_ref(exp, "pool", groups) if groups else None
    outs = []
    for _ in range(2):
        out, part = fresh_out(n, F32), fresh_out(pexp.numel(), F64) if groups else None
        launch_gn(g, w, bias, res, out, part, groups, B, H, W, Cin, Cout, True)
        outs.append((out.t.cpu(), part.t.cpu() if groups else None))
    Cv.check_same_bits(outs[0][0], outs[1][0], what)
    Cv.check_out(outs[0][0], n, exp, what)
    if groups:
        Cv.check_same_bits(outs[0][1], outs[1][1], what)
        Cv.check_partials(outs[0][1], pexp, what)


# =========================================================================================================================================
# d. persistent kernels
# =========================================================================================================================================
def tiles_shape(T):
    """(B, H, W) with B * (H / 16) * (W / 16) == T and the image as square as T's factors allow"""
    best = None
    for b in range(1, 9):
        if T % b:
            continue
        r = T // b
        th = max(d for d in range(1, int(r ** 0.5) + 1) if r % d == 0)
        cand = (r // th - th, b, th, r // th)
        best = cand if best is None or cand < best else best
    _, b, th, tw = best
    return b, 16 * th, 16 * tw


@pytest.mark.parametrize("which", ["2cu-1", "2cu", "2cu+1"])
def test_persistent_default_route(which):
    """grid = CU count, taken at tiles >= 2 x CUs (conv_gn_split2_launch): one tile below (launch per tile), at and one above the
    threshold, Cin 64 -> Cout 8, coordinate probe, un-pooled and pooled - the production route of the tokenizer.  The route is chosen by
    the entry's `persistent` argument (launch_gn passes 1; ops.conv_persistent only sets that argument for the ops wrappers) and by the tile
    count; the library has no query for the route that ran, so the three tile counts are what places the cases on either side"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    T = 2 * ncu + {"2cu-1": -1, "2cu": 0, "2cu+1": 1}[which]
    B, H, W = tiles_shape(T)
    what = f"persistent default route, {T} tiles = B{B} {H}x{W}"
    g = gn_inputs(B, H, W, 64, seed_of(what))
    gn_coordinate_check(g, B, H, W, 64, 8, what)


CHILD_LEGS = {"grid3": dict(MUSE_CONV_PERSIST_GRID="3", MUSE_CONV_PERSIST_MIN="0"), "grid8": dict(MUSE_CONV_PERSIST_GRID="8", MUSE_CONV_PERSIST_MIN="0"),
              "tiles2": dict(MUSE_CONV_PERSIST_TILES="2", MUSE_CONV_PERSIST_MIN="0"), "slab0": dict(MUSE_CONV_SLAB="0"),
              "slab2": dict(MUSE_CONV_SLAB="2")}
CHILD_SUBSET = "test_slab_split2_exact or test_slab_gn_forms or test_slab_partials_per_chunk or test_pooled_partials_per_chunk"
MANY_TILES = "test_slab_split2_more_tiles_than_cus"             # the MUSE_CONV_SLAB=2 leg only: no other switch changes how split2 walks tiles


@pytest.mark.parametrize("leg", list(CHILD_LEGS))
def test_switches_in_a_child_interpreter(leg):
    """the slab tests of this file under each switch the library reads once per process: the persistent fused kernel walking several tiles
    per workgroup across image and N-tile changes (grid 3), about one tile each (grid 8), two-tile workgroups; the tap-major kernel on slab
    shapes (MUSE_CONV_SLAB=0); conv_slab_persist_kernel<false> (MUSE_CONV_SLAB=2), which walks several tiles per workgroup only in
    test_slab_split2_more_tiles_than_cus.  One child at a time."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("MUSE_CONV_")}
    e.update(CHILD_LEGS[leg], MUSE_CONV_PERSIST="1")
    many = leg == "slab2"
    subset = CHILD_SUBSET + (" or " + MANY_TILES if many else "")            # (never matches this test: a child starts no children)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                            subset], capture_output=True, text=True, timeout=240, env=e)
    except subprocess.TimeoutExpired:
        pytest.exit(f"the child interpreter of leg {leg} hung: stopping", returncode=3)
    if r.returncode in (134, 139, -6, -11, 3):
        pytest.exit(f"the child interpreter of leg {leg} ended with {r.returncode}: stopping\n" + r.stdout[-1500:] + r.stderr[-1500:], returncode=3)
    want = len(slab_cases()) + len(gn_cases()) + len(SLAB_PARTIALS) + 3 + (3 if many else 0)      # (3: test_pooled_partials_per_chunk)
    assert r.returncode == 0 and f"{want} passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


# =========================================================================================================================================
# e. the direct kernels
# =========================================================================================================================================
def conv_in_cases():
    cases, i = [], 0
    for cout in [4, 8, 32, 128, 256, 1024]:
        pstep = 256 // (cout // 4)
        ws = sorted({1, 2, max(pstep - 1, 1), pstep, pstep + 1, 257} | ({1022} if cout in (4, 32) else set()))
        for w in ws:
            cases.append((2, 1 + i % 3, w, 1 + i % 4, 4 + 4 * ((i // 2) % 2), cout))
            i += 1
    return cases


@pytest.mark.parametrize("B,H,W,Cin,Cpad,Cout", conv_in_cases(), ids=lambda v: str(v))
def test_conv_in_direct_exact(B, H, W, Cin, Cpad, Cout):
    """conv_in_direct_kernel<CIN> and <CIN, true>: W below, at and above the pixel step 256 / (Cout / 4), at 257 and at the 1022 of the LDS
    limit; H 1 .. 3 with B = 2 (top / bottom masks at the image change); x channels Cin .. Cpad - 1 are NaN; partials per image row"""
    L = _lib()
    for probe in ("coord", "dense"):
        what = f"conv_in {probe} B{B} {H}x{W} Cin{Cin} Cpad{Cpad} Cout{Cout}"
        sd = seed_of(what)
        if probe == "coord":
            x = Cv.coord_ids((B, H, W, Cin), "x3", sd)
            w, _, _ = Cv.onehot_weights(Cout, 3, Cin, sd + 1)
        else:
            x, w = Cv.ints((B, H, W, Cin), 1023, sd), Cv.ints((Cout, 3, 3, Cin), 7, sd + 1)
        bvec = Cv.ints((Cout,), 50, sd + 2)
        Cv.assert_exact([(x, w)], bvec)
        exp = Cv.ref_conv(x, w, H, W, 3, bias=bvec)
        xp = torch.full((B, H, W, Cpad), float("nan"), dtype=F64)
        xp[..., :Cin] = x.double()
        w4 = torch.zeros(Cout, 9, 4, dtype=F64)
        w4[:, :, :Cin] = w.view(Cout, 9, Cin).double()
        groups = Cout // 4
        pexp = Cv.partials_ref(exp, "row", groups)
        assert float(pexp.abs().max()) < 2.0 ** 53
        xd = Op(Cv.place(xp, F32, exact=False))
        xn = Op(Cv.place(x.permute(0, 3, 1, 2).contiguous(), F32))
        wd, bd = Op(Cv.place_weights(w4, F32)), Op(Cv.place(bvec, F32))
        n = exp.numel()
        got = []
        for nchw in (False, False, True):
            out, part = fresh_out(n, F32), fresh_out(pexp.numel(), F64)
            if nchw:
                rc = L.muse_conv_in_direct_nchw(xn.ptr, wd.ptr, bd.ptr, out.ptr, part.ptr, groups, B, H, W, Cin, Cout, _stream())
            else:
                rc = L.muse_conv_in_direct(xd.ptr, wd.ptr, bd.ptr, out.ptr, part.ptr, groups, B, H, W, Cin, Cpad, Cout, _stream())
            assert rc == 0, (what, rc)
            got.append((out.t.cpu(), part.t.cpu()))
        for k in (1, 2):
            Cv.check_same_bits(got[0][0], got[k][0], what + (" nchw" if k == 2 else ""))
            Cv.check_same_bits(got[0][1], got[k][1], what + (" nchw" if k == 2 else "") + " partials")
        Cv.check_out(got[0][0], n, exp, what)
        Cv.check_partials(got[0][1], pexp, what)


CONV_OUT_CASES = [(32, 1, 16, 16), (64, 2, 16, 32), (96, 3, 48, 48), (32, 4, 48, 48), (64, 3, 16, 16), (96, 4, 16, 32), (32, 2, 16, 32), (64, 1, 48, 48),
                  (96, 1, 16, 16)]


@pytest.mark.parametrize("C_,Cout,H,W", CONV_OUT_CASES, ids=lambda v: str(v))
def test_conv_out_direct_coordinate(C_, Cout, H, W):
    """conv_out_direct_kernel<COUT>: one-hot weights - each output is the f32 activation at ONE input element or 0 in the padding (zero
    padding AFTER the activation), judged per element against float64 silu(x * scale + shift) within conv_cpu.bound_act; twice, same bits"""
    B = 2
    what = f"conv_out C{C_} Cout{Cout} {H}x{W}"
    sd = seed_of(what)
    x, sc, sh = rnd((B, H, W, C_), sd, 1.5), 1.0 + 0.5 * rnd((B, C_), sd + 1), 0.5 * rnd((B, C_), sd + 2)
    w, _, _ = Cv.onehot_weights(Cout, 3, C_, sd + 3)
    xd, scd, shd, wd = Op(Cv.place(x, F32)), Op(Cv.place(sc, F32)), Op(Cv.place(sh, F32)), Op(Cv.place_weights(w.view(Cout, 9 * C_), F32))
    n = B * H * W * Cout
    outs = []
    for _ in range(2):
        out = fresh_out(n, F32)
        assert _lib().muse_conv_out_direct(xd.ptr, scd.ptr, shd.ptr, wd.ptr, None, out.ptr, B, H, W, C_, Cout, _stream()) == 0
        outs.append(out.t.cpu())
    Cv.check_same_bits(outs[0], outs[1], what)
    t = x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    ref = Cv.ref_conv(x, w, H, W, 3, scale=sc, shift=sh)
    bound = Cv.ref_conv(Cv.bound_act(t), w, H, W, 3) + 1e-30
    body = Cv.check_out(outs[0], n, ref, what, exact=False, bound=bound)
    assert bool((body.view_as(ref)[ref == 0] == 0).all()), f"{what}: a padding tap is not zero"
    e32 = float(((Cv.ref_conv(Cv.silu32(x, sc, sh), w, H, W, 3) - ref).abs() / bound).max())
    print(f"[conv_edges] {what}: err/bound = {float(((body.double().view_as(ref) - ref).abs() / bound).max()):.3f}, f32 CPU evaluation {e32:.3f}")


# =========================================================================================================================================
# f. rounding leg: N(0,1) data, judged per element over the terms each output sums
# =========================================================================================================================================
ROUNDING_CASES = [("f32", 3, 5, 7, 20, 5, 3, 0), ("f32", 1, 10, 26, 68, 129, 3, 1), ("bf16", 2, 9, 13, 72, 132, 3, 0), ("bf16", 4, 5, 7, 24, 129, 3, 2),
                  ("split", 2, 9, 13, 72, 128, 3, 0), ("split", 1, 3, 43, 40, 5, 1, 0), ("split2", 3, 9, 19, 160, 132, 3, 0),
                  ("split2", 2, 16, 32, 320, 128, 3, 0), ("gn", 2, 32, 16, 192, 132, 3, 0), ("pool", 1, 48, 48, 64, 64, 3, 0),
                  ("conv_in", 2, 3, 257, 3, 128, 3, 0), ("conv_out", 2, 16, 32, 96, 3, 3, 0)]


@pytest.mark.parametrize("case", ROUNDING_CASES, ids=lambda c: "-".join(map(str, c)))
def test_rounding_per_element(case):
    """|got - float64| <= bound(S), S = sum |x_i| |w_i| + |bias| + |res| per output element; the bounds are derived in conv_cpu (bound_f32,
    bound_bf16, bound_x3, bound_act) and confirmed by the CPU evaluation of tests/test_conv_cpu.py"""
    path, B, H, W, Cin, Cout, KS, ups = case
    L = _lib()
    sd = seed_of("rounding", case)
    Hin, Win = Cv.in_dims(H, W, ups)
    K = KS * KS * Cin
    dt = BF if path == "bf16" else F32
    x = rnd((B, Hin, Win, Cin), sd, 1.0).to(dt)
    w = rnd((Cout, KS, KS, Cin), sd + 1, 1.0 / K ** 0.5).to(dt)
    bias = rnd((Cout,), sd + 2, 0.5)
    res = rnd((B, H, W, Cout), sd + 3).to(dt)
    n = B * H * W * Cout
    out = fresh_out(n // 4 if path == "pool" else n, dt)
    bd, rd = Op(Cv.place(bias, F32)), Op(Cv.place(res, dt))
    if path in ("f32", "bf16"):
        xd, wd = Op(Cv.place(x, dt)), Op(Cv.place_weights(w, dt))
        rc = L.muse_conv2d_nhwc(xd.ptr, wd.ptr, bd.ptr, rd.ptr, out.ptr, 1 if dt == BF else 0, B, H, W, Cin, Cout, KS, ups, _stream())
        ref = Cv.ref_conv(x, w, H, W, KS, ups, bias=bias, residual=res)
        bound = (Cv.bound_f32 if dt == F32 else Cv.bound_bf16)(Cv.abs_terms(x, w, H, W, KS, ups, bias, res), K)
    elif path in ("split", "split2"):
        wh, wl = Cv.split_hi_lo(w)
        whd, wld = Op(Cv.place_weights(wh, BF)), Op(Cv.place_weights(wl, BF))
        if path == "split":
            xd = Op(Cv.place(x, F32))
            rc = L.muse_conv2d_nhwc_split(xd.ptr, whd.ptr, wld.ptr, bd.ptr, rd.ptr, out.ptr, None, 0, B, H, W, Cin, Cout, KS, ups, _stream())
        else:
            xh, xl = Cv.split_hi_lo(x)
            xhd, xld = Op(Cv.place(xh, BF)), Op(Cv.place(xl, BF))
            rc = L.muse_conv2d_nhwc_split2(xhd.ptr, xld.ptr, whd.ptr, wld.ptr, bd.ptr, rd.ptr, out.ptr, None, 0, B, H, W, Cin, Cout, KS, _stream())
        ref = Cv.ref_conv(x, w, H, W, KS, ups, bias=bias, residual=res)
        bound = Cv.bound_x3(Cv.abs_terms(x, w, H, W, KS, ups, bias, res), K)
    elif path in ("gn", "pool"):
        g = gn_inputs(B, H, W, Cin, sd)
        wh, wl = Cv.split_hi_lo(w)
        launch_gn(g, [Op(Cv.place_weights(wh, BF)), Op(Cv.place_weights(wl, BF))], bd, rd, out, None, 0, B, H, W, Cin, Cout, path == "pool")
        rc = 0
        t = g["x_c"].double() * g["sc_c"].double()[:, None, None, :] + g["sh_c"].double()[:, None, None, :]
        ref = Cv.ref_conv(g["x_c"], w, H, W, 3, bias=bias, residual=res, scale=g["sc_c"], shift=g["sh_c"])
        # the activation's own error reaches the output through |w|; then the bf16x3 sum of the activated values
        bound = Cv.bound_x3(Cv.abs_terms(Cv.silu64(t), w, H, W, 3, 0, bias, res), K) + Cv.ref_conv(Cv.bound_act(t), w.abs(), H, W, 3)
        if path == "pool":                                        # three f32 additions of values <= the window's largest bound sum
            ref, bound = Cv.pool2(ref), Cv.pool2(bound) + 3 * Cv.U32 * Cv.pool2(ref.abs() + bound)
    elif path == "conv_in":
        xd = Op(Cv.place(torch.cat([x, torch.full((B, H, W, 4 - Cin), float("nan"))], -1), F32, exact=False))
        w4 = torch.zeros(Cout, 9, 4)
        w4[:, :, :Cin] = w.view(Cout, 9, Cin)
        wd = Op(Cv.place_weights(w4, F32))
        rc = L.muse_conv_in_direct(xd.ptr, wd.ptr, bd.ptr, out.ptr, None, 0, B, H, W, Cin, 4, Cout, _stream())
        ref = Cv.ref_conv(x, w, H, W, 3, bias=bias)
        bound = Cv.bound_f32(Cv.abs_terms(x, w, H, W, 3, 0, bias), K)
    else:
        sc, sh = 1.0 + 0.5 * rnd((B, Cin), sd + 4), 0.5 * rnd((B, Cin), sd + 5)
        xd, scd, shd, wd = Op(Cv.place(x, F32)), Op(Cv.place(sc, F32)), Op(Cv.place(sh, F32)), Op(Cv.place_weights(w.view(Cout, K), F32))
        rc = L.muse_conv_out_direct(xd.ptr, scd.ptr, shd.ptr, wd.ptr, bd.ptr, out.ptr, B, H, W, Cin, Cout, _stream())
        t = x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
        ref = Cv.ref_conv(x, w, H, W, 3, bias=bias, scale=sc, shift=sh)
        bound = Cv.bound_f32(Cv.abs_terms(Cv.silu64(t), w, H, W, 3, 0, bias), K) + Cv.ref_conv(Cv.bound_act(t), w.abs(), H, W, 3)
    assert rc == 0, rc
    body = Cv.check_out(out.t.cpu(), ref.numel(), ref, f"rounding {case}", values=False)   # guards, written, no NaN
    ratio = (body.double().view_as(ref) - ref).abs() / bound
    print(f"[conv_edges] rounding {path} {case[1:]}: worst |err| / bound = {float(ratio.max()):.4f}, worst |err| / S-free scale = "
          f"{float((body.double().view_as(ref) - ref).abs().max() / ref.abs().max()):.3e}")
    assert float(ratio.max()) <= 1.0, f"rounding {case}: {float(ratio.max()):.3f} x the derived bound at {int(ratio.argmax())}"


# =========================================================================================================================================
# g. host-side refusals: the entry returns before any launch (the pointers are one small real allocation)
# =========================================================================================================================================
def test_refusals_of_the_loader_entries():
    L = _lib()
    a = torch.zeros(4096, device=DEV).data_ptr()
    s = _stream()

    def nhwc(dtype=0, ptr=a, wptr=a, B=1, H=4, W=4, Cin=8, Cout=8, KS=3, ups=0):
        return L.muse_conv2d_nhwc(ptr, wptr, None, None, a, dtype, B, H, W, Cin, Cout, KS, ups, s)

    def split(ptr=a, wptr=a, lptr=a, B=1, H=4, W=4, Cin=8, Cout=8, KS=3, ups=0):
        return L.muse_conv2d_nhwc_split(ptr, wptr, lptr, None, None, a, None, 0, B, H, W, Cin, Cout, KS, ups, s)

    for fn in (nhwc, split):
        assert fn(KS=2) == ERR_UNSUPPORTED and fn(KS=5) == ERR_UNSUPPORTED
        assert fn(ups=3) == ERR_BAD_ARG and fn(ups=-1) == ERR_BAD_ARG
        assert fn(ups=1, H=5) == ERR_BAD_ARG and fn(ups=1, W=3) == ERR_BAD_ARG
        assert fn(ups=2, KS=1) == ERR_BAD_ARG
        assert fn(ptr=a + 4) == ERR_ALIGN and fn(wptr=a + 8) == ERR_ALIGN
    assert split(lptr=a + 2) == ERR_ALIGN
    assert nhwc(dtype=0, Cin=6) == ERR_ALIGN and nhwc(dtype=1, Cin=12) == ERR_ALIGN and split(Cin=12) == ERR_ALIGN
    # span limits (include/muse_hip.h): input of 4 GiB - 64 or more in its real extent per upsample mode, weight image, batch * H * W
    for fn, esz in ((nhwc, 4), (lambda **k: nhwc(dtype=1, **k), 2), (split, 4)):
        big = 128 * 4 // esz
        assert fn(B=big, H=256, W=256, Cin=128) == ERR_UNSUPPORTED                     # exactly 4 GiB
        assert fn(B=big // 4, H=256, W=256, Cin=128, ups=2) == ERR_UNSUPPORTED         # [B, 512, 512, 128]: 4 GiB, output a quarter
        assert fn(B=4 * big, H=256, W=256, Cin=128, ups=1) == ERR_UNSUPPORTED          # [B, 128, 128, 128]: 4 GiB
        assert fn(B=1, H=1, W=1, Cin=512, Cout=(1 << 32) // (9 * 512 * esz) + 1) == ERR_UNSUPPORTED     # weight image >= 4 GiB
        assert fn(B=1 << 15, H=256, W=256, Cin=8, KS=1) == ERR_UNSUPPORTED              # batch * H * W = 2^31
        assert fn(B=1, H=46341, W=46341, Cin=8, KS=1) == ERR_UNSUPPORTED                # H * W alone overflows an int


def test_refusals_of_split2_and_the_ok_predicates():
    L, ops = _lib(), _ops()
    a = torch.zeros(4096, device=DEV).data_ptr()
    s = _stream()

    def split2(xh=a, xl=a, wh=a, wl=a, out=a, res=None, B=1, H=16, W=16, Cin=64, Cout=8, KS=3):
        return L.muse_conv2d_nhwc_split2(xh, xl, wh, wl, None, res, out, None, 0, B, H, W, Cin, Cout, KS, s)

    assert split2(KS=1) == ERR_UNSUPPORTED
    assert split2(Cin=48) == ERR_ALIGN and split2(Cout=6) == ERR_ALIGN
    for k in ("xh", "xl", "wh", "wl", "out", "res"):
        assert split2(**{k: a + 8}) == ERR_ALIGN, k
    # ops.conv_split2_ok against the entry, refusing side of every threshold (the accepting side launches: the exact tests above)
    for kw in (dict(KS=1), dict(Cin=48), dict(Cout=6), dict(B=1 << 10, H=256, W=256, Cin=32),          # plane = 4 GiB
               dict(Cin=8192, Cout=29128), dict(B=1 << 15, H=256, W=256, Cin=32)):          # weight image >= 4 GiB - 64; M = 2^31
        full = dict(B=1, H=16, W=16, Cin=64, Cout=8, KS=3)
        full.update(kw)
        assert not ops.conv_split2_ok(**full) and split2(**kw) < 0, kw
    assert ops.conv_split2_ok(1 << 10, 256, 256 - 1, 32, 8, 3) and ops.conv_split2_ok(1, 16, 16, 8192, 29124, 3)
    # accepting side: the weight-span constant is shared with the pure C predicate of gn_split2 - both sides of it at Cin 2048 (the plane
    # and M terms of split2 have no C form that does not launch; their accepting side stays the Python expression)
    for cout, want in ((116508, True), (116512, False)):
        assert ops.conv_split2_ok(1, 16, 16, 2048, cout, 3) == want and bool(L.muse_conv2d_nhwc_gn_split2_ok(1, 16, 16, 2048, cout, 3)) == want
    # gn_split2: the C predicate is the entry's own check; ops wraps it
    ok = L.muse_conv2d_nhwc_gn_split2_ok
    for args, want in (((1, 16, 16, 64, 8, 3), 1), ((1, 16, 24, 64, 8, 3), 0), ((1, 8, 16, 64, 8, 3), 0), ((1, 16, 16, 32, 8, 3), 0),
                       ((1, 16, 16, 2048, 8, 3), 1), ((1, 16, 16, 2112, 8, 3), 0), ((1, 16, 16, 64, 6, 3), 0), ((1, 16, 16, 64, 8, 1), 0),
                       ((1 << 8, 256, 256, 64, 8, 3), 0), ((1 << 8, 256, 240, 64, 8, 3), 1)):
        assert ok(*args) == want and ops.conv_gn_split2_ok(*args) == bool(want), args
        if not want:
            for fn in (L.muse_conv2d_nhwc_gn_split2, L.muse_conv2d_nhwc_gn_split2_pool):
                assert fn(a, a, a, a, a, None, None, a, None, 0, *args, 1, s) == ERR_UNSUPPORTED, args
    # partial statistics: ops.conv_gn_stats_ok against both entries
    for groups, Cout, want in ((32, 128, True), (32, 64, False), (64, 64 * 128, True), (32, 32 * 256, False), (32, 96 * 32, False), (16, 128, False)):
        assert ops.conv_gn_stats_ok(16, 16, Cout, groups) == want
        if not want and groups in (32, 64):
            assert L.muse_conv2d_nhwc_split2(a, a, a, a, None, None, a, a, groups, 1, 16, 16, 64, Cout, 3, s) == ERR_UNSUPPORTED
            assert L.muse_conv2d_nhwc_gn_split2(a, a, a, a, a, None, None, a, a, groups, 1, 16, 16, 64, Cout, 3, 1, s) == ERR_UNSUPPORTED
    assert not ops.conv_gn_stats_ok(16, 24, 128, 32)
    assert L.muse_conv2d_nhwc_split2(a, a, a, a, None, None, a, a, 32, 1, 16, 24, 32, 128, 3, s) == ERR_UNSUPPORTED
    # ops.conv_gn_split2_pool_ok = the shape predicate and, with statistics, the partial's condition: the pooled entry refuses what it refuses
    pool = L.muse_conv2d_nhwc_gn_split2_pool
    for args, groups, want in (((1, 16, 16, 64, 128, 3), 0, True), ((1, 16, 16, 64, 128, 3), 32, True), ((1, 16, 24, 64, 128, 3), 0, False),
                               ((1, 16, 16, 32, 128, 3), 32, False), ((1, 16, 16, 64, 64, 3), 32, False), ((1, 16, 16, 64, 32 * 256, 3), 32, False),
                               ((1, 16, 16, 64, 64, 3), 0, True)):
        assert ops.conv_gn_split2_pool_ok(*args, gn_groups=groups) == want, (args, groups)
        if not want:
            assert pool(a, a, a, a, a, None, None, a, a if groups else None, groups, *args, 1, s) == ERR_UNSUPPORTED, (args, groups)
    # ops.conv_slab_ok names the kernel muse_conv2d_nhwc_split2 runs (H, W % 16, Cin % 64, MUSE_CONV_SLAB): each side of each threshold.
    # That the entry agrees is what the partial tests show: test_slab_partials_per_chunk / test_tap_major_partials_per_chunk pass only
    # with the chunk map of the kernel that ran (16 x 16 patches against 256 consecutive pixels).
    for H, W, Cin in ((16, 16, 64), (16, 32, 128), (16, 24, 64), (8, 16, 64), (16, 16, 32), (16, 16, 96), (48, 48, 320)):
        assert ops.conv_slab_ok(H, W, Cin) == (split2_map(H, W, Cin) == "slab"), (H, W, Cin)


def test_refusals_of_the_direct_entries():
    L, ops = _lib(), _ops()
    a = torch.zeros(4096, device=DEV).data_ptr()
    s = _stream()

    def cin(W=16, Cin=3, Cpad=4, Cout=128, x=a, groups=0, part=None):
        return L.muse_conv_in_direct(x, a, None, a, part, groups, 1, 4, W, Cin, Cpad, Cout, s)

    for kw, ok_args in ((dict(W=1023), (3, 128, 3, 4, 1023)), (dict(Cin=5), (5, 128, 3, 4)), (dict(Cpad=6), (3, 128, 3, 6)), (dict(Cout=6), (3, 6, 3, 4)),
                        (dict(Cout=96), (3, 96, 3, 4)), (dict(Cout=2048), (3, 2048, 3, 4))):
        assert cin(**kw) == ERR_UNSUPPORTED and not ops.conv_in_direct_ok(*ok_args), kw
    assert ops.conv_in_direct_ok(3, 128, 3, 4, 1022) and ops.conv_in_direct_ok(4, 1024, 3, 8)
    assert cin(x=a + 4) == ERR_ALIGN and cin(groups=16, part=a) == ERR_UNSUPPORTED
    assert L.muse_conv_in_direct_nchw(a, a, None, a, None, 0, 1, 4, 1023, 3, 128, s) == ERR_UNSUPPORTED
    assert L.muse_conv_in_direct_nchw(a + 2, a, None, a, None, 0, 1, 4, 16, 3, 128, s) == ERR_ALIGN

    def cout(H=16, W=16, C_=32, Cout=3, x=a):
        return L.muse_conv_out_direct(x, a, a, a, None, a, 1, H, W, C_, Cout, s)

    for kw, ok_args in ((dict(H=17), (17, 16, 32, 3, 3)), (dict(W=8), (16, 8, 32, 3, 3)), (dict(C_=48), (16, 16, 48, 3, 3)), (dict(Cout=5), (16, 16, 32, 5, 3))):
        assert cout(**kw) == ERR_UNSUPPORTED and not ops.conv_out_direct_ok(*ok_args), kw
    assert not ops.conv_out_direct_ok(16, 16, 32, 3, 1) and ops.conv_out_direct_ok(16, 16, 32, 4, 3)
    assert cout(x=a + 4) == ERR_ALIGN
