"""GPU (-m gpu): the spatial, layout and VQ entry points of csrc/uvit.hip and csrc/vqgan.hip, EXACTLY at each edge of their dispatch, plus a
per-element rounding leg, the special values and the host-side refusals.  tests/spatial_cpu.py holds the float64 references, the probes,
the storage builders, the checks, the derived bounds and a contract model; tests/test_spatial_cpu.py proves on a CPU that the checks fail
for thirteen seeded defects.  profiles/spatial_edges.md has the edge table and the MI355X's figures; DESIGN.md ("Spatial / layout / VQ
contract") the contract.

Every case: operands sit inside larger allocations with NaN before and after them and in every ld > cols gap; outputs and partial buffers
are pre-filled with a NaN bit pattern no result has, guard bands on both sides - the guards come back bit for bit and every slot is
written; the case is launched twice from the same initial state and the two results are bit-identical (the GroupNorm f64 partials, which
accumulate through LDS atomicAdd, agree within the rounding of an f64 sum of their length instead).

Exact legs (equal to the float64 reference whatever the order): coordinate probes for the data movement (space-to-depth, upsample, layout,
gather, transpose) and for the depthwise convolution with one-hot taps; integer probes with every partial sum below 2^24 for the depthwise
convolution (y, dx, the dw partials per (chunk, channel, tap) slot), the pools, and the small reductions; muse_argmin_rows against its
contract.  Rounding legs: seeded N(0, 1) (and 1e3 + N(0, 1) for both norms, GRN forward / backward and the GroupNorm) per element against
float64; bound = 4 * E_REF (+ one bf16 rounding), E_REF = torch's own float32 CPU computation against float64 normalised by the sum of
the absolute terms (`python tests/test_gpu_spatial_edges.py` reprints it, no GPU needed); GRN's and the dw partials' bounds are derived
from the summed length (spatial_cpu.bound_grn, bound_grn_bwd, bound_dw).  The GroupNorm's bound is derived too (spatial_cpu.
bound_groupnorm: f64 statistics, one f32 rounding each of mean, rstd, sc, sh and the fma; + the activation's own error behind a SiLU): the
kernel's f64 statistics make it SMALLER than 4 * E_REF of the same class of input (about 130 times on N(0, 1), where torch's f32
statistics of 16k-element groups set E_REF; about 3 times on 1e3 + N(0, 1)), and a bound as wide as 4 * E_REF passes an eps ten times off
(tests/test_spatial_cpu.py shows the derived one does not).

Edges (thresholds as the code has them):
  dwconv forward / dx (uvit.hip launch_dwconv_v4: v4 needs C % 4 == 0, vpp = C / 4 >= 256 or 256 % vpp == 0, 16-byte pointers, B * H <= 65535)
    C {4, 8, 64, 1024, 1028} v4 (vpp 1, 2, 16, 256, 257: 1028 leaves a second column block with one live lane); C {6, 10, 12, 24, 96, 1020}
    scalar (1020: vpp = 255 does not divide 256); B * H {1, 7, 8, 9, 15, 17}: the XCD row remap of gridDim.x == 1 with a remainder;
    B * H {65535, 65536} at W = 1, C = 4: v4 against the scalar fallback; W {1, 2, 3, xs - 1, xs, xs + 1} with xs = 256 / vpp (C = 64: 15, 16,
    17) and W = 83 (a tail of the unroll-4 loop); H = 1; B >= 2; the same values 4 bytes off alignment take the scalar kernels: same bits
  dwconv dw (DW_PIX = 64): pixels {1, 63, 64, 65, 129}; (3, 5, 7): chunks straddle images; C {4, 256, 260} v4, {10, 66} scalar;
    pixels = 4,194,241 at C = 4 (nchunk = 65536 > gridDim.y) is refused before the dx launch; muse_transpose at rows = 32 * 65535 + 1 too
  GRN: C {4, 10, 60, 64, 68, 256, 260, 1024} (64-channel column blocks, the 256-lane stride of the scale kernel, apply4 against the scalar
    apply); S {1, 2, 3, 4, 5, 257} (waves with no rows); S * C / 4 = 262,400 > 262,144 (the grid-stride loop under the 1024-block cap); bf16
    output refused for C % 4 != 0 and for a misaligned x, before anything is launched; every case again with x 4 bytes off alignment;
    1e3 + N(0, 1) inputs at C {4, 10, 64, 68, 260} and S {5, 257}, aligned and 4 bytes off
  muse_groupnorm_silu_nhwc: groups {32, 64}; f32 C {64, 128, 1024, 1280, 2048} (1280, 2048: vpp > 256), bf16 C {64, 256, 2048}; HW {1, 255,
    1023, 1024, 1025, 2049} (1024-pixel chunks, the UN = 4 tail); refused by return code: C 2112, C 96, groups 16
  avgpool / upsample / space-to-depth / layout: (H, W) {(2, 2), (2, 6), (6, 2), larger}; C at vec and 3 vec; stats variant: HW / 4 {1023,
    1024, 1025}, C {32, 64, 1024}; muse_nchw_to_nhwc C = 3, Cpad {3, 4, 8}, f32 and bf16
  muse_transpose: rows, cols in {1, 31, 32, 33, 65}^2, ld gaps, batch 3 with strides
  muse_argmin_rows: n {1, 2, 63, 64, 65, 127, 128, 129, 1024, 8192}, rows {1, 3, 4, 5}, ld > n
  grid-stride caps: silu forward / backward and adaln_bwd's dx at 16384 blocks of 256 (4-element vectors for adaln), space_to_depth at 16384
    blocks: one case just past each
"""
import math
import sys
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

import spatial_cpu as S
from spatial_cpu import BF, F32, F64, GUARD, LEAD

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_BAD_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3
DT = {F32: 0, BF: 1}

# Worst normalised error of torch's float32 CPU computation against float64 over the case lists below, as printed by
# `python tests/test_gpu_spatial_edges.py`.  bound = 4 * E_REF[leg] * scale (+ one bf16 rounding).
E_REF = {
    "silu_fwd": 1.286e-07,   # over |silu(x)|
    "silu_bwd": 1.853e-07,   # over |dy| s (1 + |x| (1 - s))
    "sinusoid": 2.996e-07,   # over 1 + |angle|: the f32 product k * (-ln(maxpos) / half) moves the frequency by up to 9.2 * 2^-24
    "adaln_bwd_dx": 1.183e-07,   # over |dy| (1 + |scale|): two roundings
    "dwconv": 1.877e-07,   # over sum |x| |w| of the nine taps
    # printed for the profile; these legs are judged by the derived bounds of spatial_cpu
    "groupnorm": 4.236e-06,   # over |x sc| + |sh|, N(0, 1) inputs: torch's f32 statistics of 16k-element groups (HW 1025, C 1024, G 64)
    "groupnorm_1e3": 7.724e-08,  # the same, 1e3 + N(0, 1) inputs (the normaliser is about 1e3 times larger)
    "grn_fwd": 5.308e-07,
    "grn_bwd_dx": 6.213e-06,
    "grn_fwd_1e3": 2.438e-07,     # 1e3 + N(0, 1) inputs
    "grn_bwd_dx_1e3": 2.256e-06,
}


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """a launch that faulted leaves the device unusable for the rest of the process: end the session there rather than start more work"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU error after a spatial edge test, stopping: {e}", returncode=3)


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


class Op:
    """a storage on the device and the address of the operand / result `lead` elements into it"""

    def __init__(self, st, lead):
        self.t = st.to(DEV)
        self.lead = lead
        self.ptr = self.t.data_ptr() + lead * st.element_size()


def op_in(t, dtype=F32, shift=0):
    """an input inside NaN; shift = 1 (f32): 4 bytes off its 16-byte alignment"""
    o = Op(S.place_shifted(t, dtype, shift) if shift else S.place(t, dtype), LEAD + shift)
    assert (o.ptr % 16 == 0) == (shift == 0)
    return o


def op_raw(st, lead=LEAD):
    return Op(st, lead)


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
    """launch(*outputs) must return `code` and launch nothing: every output storage keeps its sentinels.  The outputs (and, in the caller,
    the operands) stay alive in locals until the device has been waited for."""
    outs = [op_out(*s) for s in spec]
    rc = launch(*outs)
    assert rc == code, f"{what}: the entry returned {rc}, not {code}"
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        S.check_untouched(o.t.cpu(), f"{what} output {i}")


WORST = {}


def judge(leg, what, st, n, ref, bound, guard=GUARD):
    """storage checks, then |got - ref| <= bound per element; prints the worst figure first"""
    body = S.check_out(st, n, ref, what, guard=guard, values=False)
    w = S.worst_ratio(body, ref, bound)
    WORST[leg] = max(WORST.get(leg, 0.0), w)
    print(f"[spatial_edges] {leg} {what}: err/bound={w:.3f} (worst so far {WORST[leg]:.3f})")
    assert w <= 1.0, f"{what}: error {w:.3f} x its bound"
    return body


# =========================================================================================================================================
# a. pure data movement
# =========================================================================================================================================
S2D_SHAPES = [(2, 2, 2, 4), (1, 2, 6, 12), (3, 6, 2, 4), (2, 6, 10, 12)]


@pytest.mark.parametrize("B,H,W,C", S2D_SHAPES + [(1, 1026, 1024, 16)])          # the last: n4 = 4,202,496 > 16384 * 256 (grid-stride)
def test_space_to_depth(B, H, W, C):
    L = _lib()
    x = S.coord_ids((B, H, W, C), "f32", seed_of("s2d", B, H, W, C)).float()
    for inverse in ((0,) if H > 100 else (0, 1)):
        src = S.ref_space_to_depth(x, False) if inverse else x          # inverse: packed -> full
        exp = x if inverse else S.ref_space_to_depth(x, False)
        assert torch.equal(S.ref_space_to_depth(S.ref_space_to_depth(x), True), x)
        xi = op_in(src)
        what = f"space_to_depth B{B} {H}x{W} C{C} inverse{inverse}"
        (y,) = twice(what, [(x.numel(), F32)], lambda o: L.muse_space_to_depth2_nhwc(xi.ptr, o.ptr, B, H, W, C, inverse, _stream()))
        S.check_out(y, x.numel(), exp, what)
    xs, xi = op_in(x, shift=1), op_in(x)
    refused("space_to_depth misaligned", ERR_UNSUPPORTED, [(x.numel(), F32)], lambda o: L.muse_space_to_depth2_nhwc(xs.ptr, o.ptr, B, H, W, C, 0, _stream()))
    refused("space_to_depth odd H", ERR_UNSUPPORTED, [(x.numel(), F32)], lambda o: L.muse_space_to_depth2_nhwc(xi.ptr, o.ptr, B, H + 1, W, C, 0, _stream()))


def spatial_shapes(vec):
    return [(2, 2, 2, vec), (1, 2, 6, 3 * vec), (3, 6, 2, vec), (2, 10, 14, 3 * vec)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_upsample2x(dtype):
    L = _lib()
    vec = 4 if dtype == F32 else 8
    for B, H, W, C in spatial_shapes(vec) + [(2, 1, 1, vec), (1, 3, 5, vec)]:
        x = S.coord_ids((B, H, W, C), "f32" if dtype == F32 else "bf16", seed_of("ups", B, H, W, C)).float()
        xi = op_in(x, dtype)
        what = f"upsample2x {dtype} B{B} {H}x{W} C{C}"
        (y,) = twice(what, [(4 * x.numel(), dtype)], lambda o: L.muse_upsample2x_nhwc(xi.ptr, o.ptr, DT[dtype], B, H, W, C, _stream()))
        S.check_out(y, 4 * x.numel(), S.ref_upsample2x(x), what)
    refused("upsample2x C % vec", ERR_UNSUPPORTED, [(4 * (vec + 1), dtype)], lambda o: L.muse_upsample2x_nhwc(xi.ptr, o.ptr, DT[dtype], 1, 1, 1, vec + 1, _stream()))
    refused("upsample2x misaligned", ERR_ALIGN, [(4 * vec, dtype)], lambda o: L.muse_upsample2x_nhwc(xi.ptr + 4, o.ptr, DT[dtype], 1, 1, 1, vec, _stream()))


def test_upsample2x_split():
    """the (hi, lo) planes equal bf16(x) and bf16(x - hi) of the source pixel"""
    L = _lib()
    for B, H, W, C in spatial_shapes(8) + [(2, 1, 1, 8)]:
        x = S.randn((B, H, W, C), seed_of("upsplit", B, H, W, C))
        hi, lo = S.ref_split(S.ref_upsample2x(x))
        xi = op_in(x)
        n = 4 * x.numel()
        what = f"upsample2x_split B{B} {H}x{W} C{C}"
        yh, yl = twice(what, [(n, BF), (n, BF)], lambda a, b: L.muse_upsample2x_split_nhwc(xi.ptr, a.ptr, b.ptr, B, H, W, C, _stream()))
        S.check_out(yh, n, hi, what + " hi")
        S.check_out(yl, n, lo, what + " lo")
    refused("upsample2x_split C % 8", ERR_UNSUPPORTED, [(48, BF), (48, BF)], lambda a, b: L.muse_upsample2x_split_nhwc(xi.ptr, a.ptr, b.ptr, 1, 1, 1, 12, _stream()))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_layout(dtype):
    """muse_nchw_to_nhwc (zero padding is +0) and muse_nhwc_to_nchw (the padding channels, NaN here, are never read)"""
    L = _lib()
    kind = "f32" if dtype == F32 else "bf16"
    for B, C, HW, Cpad in [(2, 3, 1, 3), (2, 3, 37, 4), (2, 3, 300, 8), (3, 3, 300, 3), (1, 8, 257, 8), (2, 3, 4500, 4)]:
        x = S.coord_ids((B, C, HW), kind, seed_of("layout", B, C, HW, Cpad)).float()
        xi = op_in(x)
        n = B * HW * Cpad
        what = f"nchw_to_nhwc {kind} B{B} C{C} HW{HW} Cpad{Cpad}"
        (y,) = twice(what, [(n, dtype)], lambda o: L.muse_nchw_to_nhwc(xi.ptr, o.ptr, DT[dtype], B, C, HW, Cpad, _stream()))
        exp = S.ref_nchw_to_nhwc(x, Cpad)
        S.check_zero_sign(S.check_out(y, n, exp, what), exp, what)
        padded = torch.full((B, HW, Cpad), S.NAN)
        padded[:, :, :C] = x.transpose(1, 2)
        pi = op_raw(S.place(padded, dtype, exact=False))
        what = f"nhwc_to_nchw {kind} B{B} C{C} HW{HW} Cpad{Cpad}"
        (z,) = twice(what, [(x.numel(), F32)], lambda o: L.muse_nhwc_to_nchw(pi.ptr, DT[dtype], o.ptr, B, C, HW, Cpad, _stream()))
        S.check_out(z, x.numel(), x, what)


@pytest.mark.parametrize("out_dtype", [F32, BF], ids=["f32", "bf16"])
def test_gather_rows(out_dtype):
    """f32: every output is one table element; bf16: the float32 -> bfloat16 rounding of the selected row"""
    L = _lib()
    for rows, cols, Kc in [(1, 1, 1), (5, 63, 7), (3, 64, 2), (4, 65, 9), (300, 256, 33), (2, 129, 1024)]:
        sd = seed_of("gather", rows, cols, Kc)
        table = S.coord_ids((Kc, cols), "f32", sd).float() if out_dtype == F32 else S.randn((Kc, cols), sd)
        idx = torch.randint(0, Kc, (rows,), generator=S.gen(sd))
        idx[0], idx[-1] = Kc - 1, 0
        ti, ii = op_in(table), idx.to(DEV)
        what = f"gather_rows {out_dtype} rows{rows} cols{cols} Kc{Kc}"
        (y,) = twice(what, [(rows * cols, out_dtype)], lambda o: L.muse_gather_rows(ti.ptr, ii.data_ptr(), o.ptr, DT[out_dtype], rows, cols, _stream()))
        S.check_out(y, rows * cols, table[idx] if out_dtype == F32 else S.to_bf16(table[idx]), what)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_transpose(dtype):
    L = _lib()
    kind = "f32" if dtype == F32 else "bf16"
    sizes = [1, 31, 32, 33, 65]
    for rows in sizes:
        for cols in sizes:
            gap = (rows + cols) % 2 == 0                     # every second pair: ld gaps and three strided matrices
            batch = 3 if gap else 1
            ldi, ldo = cols + (3 if gap else 0), rows + (5 if gap else 0)
            si, so = rows * ldi + (7 if gap else 0), cols * ldo + (11 if gap else 0)
            x = S.coord_ids((batch, rows, cols), kind, seed_of("tr", rows, cols)).float()
            body = torch.full((batch * si,), S.NAN)
            body[S.ld_index(rows, cols, ldi, batch, si)] = x.flatten()
            xi = op_raw(S.place(body, dtype, exact=False))
            what = f"transpose {kind} {rows}x{cols} ld {ldi}/{ldo} batch{batch}"
            (y,) = twice(what, [(batch * so, dtype)],
                         lambda o: L.muse_transpose(xi.ptr, o.ptr, DT[dtype], rows, cols, ldi, ldo, batch, si, so, _stream()))
            S.check_index(y, S.ld_index(cols, rows, ldo, batch, so), x.transpose(1, 2), what)


def test_transpose_refuses_a_grid_overflow():
    """rows = 32 * 65535 + 1 needs gridDim.y = 65536: MUSE_ERR_UNSUPPORTED from the host check, nothing launched"""
    L = _lib()
    rows = 32 * 65535 + 1
    xi, out = op_in(torch.ones(rows)), op_out(rows)
    assert L.muse_transpose(xi.ptr, out.ptr, 0, rows, 1, 1, rows, 1, 0, 0, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    S.check_untouched(out.t.cpu(), "transpose rows = 32 * 65535 + 1")
    assert L.muse_transpose(xi.ptr, out.ptr, 0, 1, 1, 1, 1, 65536, 0, 0, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    S.check_untouched(out.t.cpu(), "transpose batch = 65536")
    rows -= 1                                                  # gridDim.y = 65535 is served
    x = S.coord_ids((rows, 1), "f32", 5).float()
    xi = op_in(x)
    (y,) = twice("transpose rows = 32 * 65535", [(rows, F32)], lambda o: L.muse_transpose(xi.ptr, o.ptr, 0, rows, 1, 1, rows, 1, 0, 0, _stream()))
    S.check_out(y, rows, x, "transpose rows = 32 * 65535")


# =========================================================================================================================================
# b. depthwise 3 x 3: forward, dx, dw partials
# =========================================================================================================================================
def run_dwconv(c, shift=0):
    """forward on a, backward on (g, a): storage checks on all three outputs, exact where the probe is, else within the bound.  Returns the
    three result bodies (the same-bits comparison of the two routes reads them)."""
    L = _lib()
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    n, nch = B * H * W * C, S.dw_nchunk(B * H * W)
    assert L.muse_dwconv3x3_bwd_nchunk(B * H * W) == nch
    a, g, w = op_in(c["a"], shift=shift), op_in(c["g"], shift=shift), op_in(c["w"])
    what = f"dwconv {c['probe']} B{B} {H}x{W} C{C} shift{shift}"
    (y,) = twice(what + " y", [(n, F32, shift)], lambda o: L.muse_dwconv3x3_nhwc(a.ptr, w.ptr, o.ptr, B, H, W, C, _stream()))
    dx, dw = twice(what + " bwd", [(n, F32, shift), (nch * C * 9, F32)],
                   lambda o, p: L.muse_dwconv3x3_bwd(g.ptr, a.ptr, w.ptr, o.ptr, p.ptr, B, H, W, C, _stream()))
    res = {}
    for key, st, m, guard in (("y", y, n, GUARD + shift), ("dx", dx, n, GUARD + shift), ("dw", dw, nch * C * 9, GUARD)):
        if c["exact"][key]:
            res[key] = S.check_out(st, m, c[key], f"{what} {key}", guard=guard)
            if key != "dw":
                S.check_zero_sign(res[key], c[key], f"{what} {key}")
        elif key == "dw":
            res[key] = judge("dwconv_dw", f"{what} dw", st, m, c["dw"], S.bound_dw(c["g"], c["a"]), guard)
        else:
            src = c["a"] if key == "y" else c["g"]
            scale = S.ref_dwconv(src.abs(), c["w"].abs()) if key == "y" else S.ref_dwconv_dx(src.abs(), c["w"].abs())
            res[key] = judge("dwconv", f"{what} {key}", st, m, c[key], 4.0 * E_REF["dwconv"] * scale + S.TINY, guard)
    return res


DW_C = [4, 8, 64, 1020, 1024, 1028, 6, 10, 12, 24, 96]
DW_ROWS = [(1, 1), (1, 7), (2, 4), (3, 3), (3, 5), (1, 17)]                       # B * H in {1, 7, 8, 9, 15, 17}
DW_PIXELS = [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (3, 1, 43), (3, 5, 7)]  # 1, 63, 64, 65, 129 pixels; chunks straddling three images


def dw_shapes():
    s = [(2, 3, 5, C) for C in DW_C]
    s += [(B, H, 3, 8) for B, H in DW_ROWS]
    s += [(2, 3, W, 64) for W in (1, 2, 3, 15, 16, 17, 83)] + [(2, 1, 16, 64)]
    s += [(2, 2, W, 1024) for W in (1, 2, 5)]
    s += [(B, H, W, C) for B, H, W in DW_PIXELS for C in (4, 10)]
    s += [(3, 5, 7, C) for C in (256, 260, 66)]
    return s


@pytest.mark.parametrize("probe", ["coord", "pick", "dense"])
def test_dwconv_exact(probe):
    for B, H, W, C in dw_shapes():
        run_dwconv(S.dwconv_case(probe, B, H, W, C, seed_of("dw", probe, B, H, W, C)))


@pytest.mark.parametrize("B,H", [(1, 65535), (2, 32768)], ids=["rows65535_v4", "rows65536_scalar"])
def test_dwconv_tall(B, H):
    """B * H = 65535 is the last row count the v4 kernels take (gridDim.y); 65536 falls back to the scalar kernels"""
    run_dwconv(S.dwconv_case("coord", B, H, 1, 4, seed_of("tall", B, H)))
    run_dwconv(S.dwconv_case("dense", B, H, 1, 4, seed_of("tall", B, H)))


def test_dwconv_rounding_and_route_bits():
    """N(0, 1): per element against float64; and the same values 4 bytes off alignment (the scalar kernels) give the v4 kernels' bits, as the
    comments at dwconv3x3_v4_kernel and dwconv3x3_bwd_dw_v4_kernel promise"""
    for B, H, W, C in [(2, 5, 7, 64), (3, 5, 7, 260), (2, 3, 5, 1024), (2, 9, 17, 8), (2, 5, 7, 10)]:
        c = S.dwconv_case("randn", B, H, W, C, seed_of("dwr", B, H, W, C))
        v4, sc = run_dwconv(c), run_dwconv(c, shift=1)
        for key in ("y", "dx", "dw"):
            S.check_same_bits(v4[key], sc[key], f"dwconv B{B} {H}x{W} C{C} {key}: aligned against 4 bytes off")


def test_dwconv_bwd_refuses_a_grid_overflow():
    """pixels = 4,194,241 needs 65536 dw chunks in gridDim.y: MUSE_ERR_UNSUPPORTED before the dx kernel is launched, dx keeps its sentinels"""
    L = _lib()
    B, H, W, C = 1, 4194241, 1, 4
    n = B * H * W * C
    z = torch.zeros(n + 2 * LEAD)
    g, a, w = Op(z, LEAD), Op(z, LEAD), op_in(torch.ones(C, 9))
    dx, dw = op_out(n), op_out(S.dw_nchunk(B * H * W) * C * 9)
    assert L.muse_dwconv3x3_bwd(g.ptr, a.ptr, w.ptr, dx.ptr, dw.ptr, B, H, W, C, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    S.check_untouched(dx.t.cpu(), "dwconv3x3_bwd at 4,194,241 pixels: dx")
    S.check_untouched(dw.t.cpu(), "dwconv3x3_bwd at 4,194,241 pixels: dw partials")


# =========================================================================================================================================
# c. pools
# =========================================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_avgpool(dtype):
    L = _lib()
    vec = 4 if dtype == F32 else 8
    for B, H, W, C in spatial_shapes(vec) + [(2, 66, 62, 3 * vec)]:
        x = 4.0 * S.ints((B, H, W, C), 255 if dtype == F32 else 31, seed_of("pool", B, H, W, C)).float()      # bf16: |x| <= 124, results <= 124
        xi = op_in(x, dtype)
        n = x.numel() // 4
        what = f"avgpool {dtype} B{B} {H}x{W} C{C}"
        (y,) = twice(what, [(n, dtype)], lambda o: L.muse_avgpool2x2_nhwc(xi.ptr, o.ptr, DT[dtype], B, H, W, C, _stream()))
        S.check_out(y, n, S.ref_avgpool(x.double()), what)
    refused("avgpool odd H", ERR_BAD_ARG, [(2 * vec, dtype)], lambda o: L.muse_avgpool2x2_nhwc(xi.ptr, o.ptr, DT[dtype], 1, 3, 2, vec, _stream()))


@pytest.mark.parametrize("H,W,C,G", [(66, 62, 32, 32), (64, 64, 32, 32), (82, 50, 32, 32), (66, 62, 64, 64), (64, 64, 64, 32), (82, 50, 64, 64),
                                     (82, 50, 1024, 32), (2, 2, 1024, 64)])
def test_avgpool_stats(H, W, C, G):
    """pooled pixels 1023 / 1024 / 1025 (and 1): the pooled values carry the plain kernel's bits, the f64 partials are exact per slot"""
    L = _lib()
    B = 2
    x = 4.0 * S.ints((B, H, W, C), 255, seed_of("poolstats", H, W, C, G)).float()
    xi = op_in(x)
    n, HWo = x.numel() // 4, (H // 2) * (W // 2)
    exp = S.ref_avgpool(x.double())
    pexp = S.ref_gn_partials(exp.view(B, HWo, C), G)
    assert float(pexp.abs().max()) < 2.0 ** 53
    what = f"avgpool_stats {H}x{W} C{C} G{G}"
    y, part = twice(what, [(n, F32), (pexp.numel(), F64)], lambda o, p: L.muse_avgpool2x2_nhwc_stats(xi.ptr, o.ptr, p.ptr, G, B, H, W, C, _stream()))
    (plain,) = twice(what + " plain", [(n, F32)], lambda o: L.muse_avgpool2x2_nhwc(xi.ptr, o.ptr, 0, B, H, W, C, _stream()))
    S.check_out(y, n, exp, what)
    S.check_same_bits(y, plain, what + ": the stats kernel's pooled values against the plain kernel's")
    S.check_out(part, pexp.numel(), pexp, what + " partials")
    refused(what + " groups 16", ERR_UNSUPPORTED, [(n, F32), (pexp.numel(), F64)],
            lambda o, p: L.muse_avgpool2x2_nhwc_stats(xi.ptr, o.ptr, p.ptr, 16, B, H, W, C, _stream()))


# =========================================================================================================================================
# d. small reductions and element-wise kernels, integer probes
# =========================================================================================================================================
@pytest.mark.parametrize("B,R,C,lim", [(2, 1, 4, 7), (3, 5, 68, 7), (2, 257, 64, 7), (1, 3, 260, 7), (1, 16400, 1024, 3)])
def test_adaln_bwd_exact(B, R, C, lim):
    """integer probe: dx and both column sums exact.  The last case: n / 4 = 4,198,400 > 16384 * 256, the dx kernel's grid-stride loop"""
    L = _lib()
    sd = seed_of("adaln", B, R, C)
    dy, x, ss = S.ints((B * R, C), lim, sd).float(), S.ints((B * R, C), 255, sd + 1).float(), S.ints((B, 2 * C), 3, sd + 2).float()
    assert R * lim * 255 < 2 ** 24
    dyi, xi, si = op_in(dy), op_in(x), op_in(ss)
    what = f"adaln_bwd B{B} R{R} C{C}"
    dx, dss = twice(what, [(dy.numel(), F32), (2 * B * C, F32)], lambda o, p: L.muse_adaln_bwd(dyi.ptr, xi.ptr, si.ptr, o.ptr, p.ptr, B, R, C, _stream()))
    edx, edss = S.ref_adaln_bwd(dy, x, ss, B, R, C)
    S.check_out(dx, dy.numel(), edx, what + " dx")
    S.check_out(dss, 2 * B * C, edss, what + " dss")
    refused("adaln_bwd C % 4", ERR_UNSUPPORTED, [(6, F32), (12, F32)], lambda o, p: L.muse_adaln_bwd(dyi.ptr, xi.ptr, si.ptr, o.ptr, p.ptr, 1, 1, 6, _stream()))


def test_colsum_segments():
    L = _lib()
    for nseg, seg, cols in [(1, 1, 1), (3, 5, 255), (2, 16, 256), (4, 7, 257), (2, 33, 1024)]:
        p = S.ints((nseg * seg, cols), 1023, seed_of("colseg", nseg, seg, cols)).float()
        pi = op_in(p)
        what = f"colsum_segments {nseg}x{seg}x{cols}"
        (y,) = twice(what, [(nseg * cols, F32)], lambda o: L.muse_colsum_segments(pi.ptr, o.ptr, nseg, seg, cols, _stream()))
        S.check_out(y, nseg * cols, p.double().view(nseg, seg, cols).sum(1), what)
    big = op_in(torch.ones(65536))
    refused("colsum_segments nseg 65536", ERR_UNSUPPORTED, [(65536, F32)], lambda o: L.muse_colsum_segments(big.ptr, o.ptr, 65536, 1, 1, _stream()))


def test_row_sumsq():
    L = _lib()
    for rows in (1, 3, 4, 5):
        for cols in (1, 63, 64, 65, 256, 1024):
            x = S.ints((rows, cols), 63, seed_of("sumsq", rows, cols)).float()
            xi = op_raw(S.place_ld(x, F32, cols + 3))
            what = f"row_sumsq {rows}x{cols}"
            (y,) = twice(what, [(rows, F32)], lambda o: L.muse_row_sumsq(xi.ptr, o.ptr, rows, cols, cols + 3, _stream()))
            S.check_out(y, rows, (x.double() ** 2).sum(1), what)


def test_weighted_mean():
    """float32(a / b) with a = sum v w and b = sum w exact in float64, as the kernel computes it"""
    L = _lib()
    for n in (1, 63, 64, 1023, 1024, 1025, 5000):
        v, w = S.ints((n,), 100, seed_of("wm", n)).float(), (S.ints((n,), 3, seed_of("wmw", n)).float() + 5.0)
        vi, wi = op_in(v), op_in(w)
        (y,) = twice(f"weighted_mean n{n}", [(1, F32)], lambda o: L.muse_weighted_mean(vi.ptr, wi.ptr, o.ptr, n, _stream()))
        exp = ((v.double() * w.double()).sum() / w.double().sum()).float()
        S.check_out(y, 1, exp.view(1), f"weighted_mean n{n}")
    refused("weighted_mean n 0", ERR_BAD_ARG, [(1, F32)], lambda o: L.muse_weighted_mean(vi.ptr, wi.ptr, o.ptr, 0, _stream()))


def test_scale_rows():
    """power-of-two weights: exact; the ld > cols gap (and the NaN around the tensor) comes back bit for bit"""
    L = _lib()
    for rows, cols, ld in [(1, 1, 4), (5, 63, 70), (3, 256, 256), (7, 257, 300), (300, 65, 67)]:
        sd = seed_of("scale", rows, cols)
        x = S.ints((rows, cols), 1023, sd).float()
        w = 2.0 ** torch.randint(-3, 4, (rows,), generator=S.gen(sd)).float()
        st = S.place_ld(x, F32, ld)
        wi, num, den = op_in(w), op_in(torch.tensor([8.0])), op_in(torch.tensor([2.0]))
        runs = []
        for _ in range(2):
            xi = op_raw(st.clone())
            assert L.muse_scale_rows(xi.ptr, wi.ptr, num.ptr, den.ptr, rows, cols, ld, _stream()) == 0
            runs.append(xi.t.cpu())
        what = f"scale_rows {rows}x{cols} ld{ld}"
        S.check_same_bits(runs[0], runs[1], what)
        exp = S.place_ld(x * w[:, None] * 4.0, F32, ld)
        assert torch.equal(S.bits(runs[0]), S.bits(exp)), f"{what}: values differ, or the gap / the surroundings were written"


def test_silu_past_the_grid_cap():
    """n = 16384 * 256 + 257: the grid-stride loop (257 threads take a second element).  Exact probe: for x >= 32, exp(-x) < 2^-24 vanishes
    beside 1, so silu(x) = x and the backward's factor s (1 + x (1 - s)) = 1: y = x and dx = dy, both seeded ids - the reference is index
    arithmetic.  Then N(0, 1) at the same n, per element against float64: the compiler is free to build the loop's first and later trips
    differently (it does for silu_bwd: the last bit of an element can depend on its thread's trip count), every trip is within the bound"""
    L = _lib()
    n = 16384 * 256 + 257
    x, dy = S.coord_ids((n,), "f32", 77).float() + 32.0, S.coord_ids((n,), "f32", 78).float()
    xi, dyi = op_in(x), op_in(dy)
    (y,) = twice("silu past the cap", [(n, F32)], lambda o: L.muse_silu_fwd(xi.ptr, o.ptr, n, _stream()))
    (dx,) = twice("silu_bwd past the cap", [(n, F32)], lambda o: L.muse_silu_bwd(xi.ptr, dyi.ptr, o.ptr, n, _stream()))
    S.check_out(y, n, x, "silu past the cap")
    S.check_out(dx, n, dy, "silu_bwd past the cap")
    x, dy = S.randn((n,), 79), S.randn((n,), 80)
    xi, dyi = op_in(x), op_in(dy)
    (y,) = twice("silu past the cap, N(0, 1)", [(n, F32)], lambda o: L.muse_silu_fwd(xi.ptr, o.ptr, n, _stream()))
    (dx,) = twice("silu_bwd past the cap, N(0, 1)", [(n, F32)], lambda o: L.muse_silu_bwd(xi.ptr, dyi.ptr, o.ptr, n, _stream()))
    ref = S.silu64(x)
    judge("silu_fwd", "silu past the cap", y, n, ref, 4.0 * E_REF["silu_fwd"] * ref.abs() + S.TINY)
    rb, sb = S.ref_silu_bwd(x, dy)
    judge("silu_bwd", "silu_bwd past the cap", dx, n, rb, 4.0 * E_REF["silu_bwd"] * sb + S.TINY)


# =========================================================================================================================================
# e. muse_argmin_rows
# =========================================================================================================================================
ARGMIN_N = [1, 2, 63, 64, 65, 127, 128, 129, 1024, 8192]


def argmin_launch(d, ld, what):
    L = _lib()
    rows, n = d.shape
    di = op_raw(S.place_ld(d, F32, ld))
    (st,) = twice(what, [(rows, F64)], lambda o: L.muse_argmin_rows(di.ptr, o.ptr, rows, n, ld, _stream()))
    s = S.bits(S.sentinel(1, F64))[0]
    b = S.bits(st)
    assert bool((b[:GUARD] == s).all()) and bool((b[GUARD + rows:] == s).all()), f"{what}: wrote outside the index tensor"
    idx = b[GUARD:GUARD + rows]
    assert not bool((idx == s).any()), f"{what}: an index was never written"
    return idx


@pytest.mark.parametrize("n", ARGMIN_N)
def test_argmin_rows(n):
    """the index tensor alone is inspected (never gathered with): always in [0, n), the lowest index of the smallest non-NaN value, 0 for a
    row of +inf and for a row of NaN"""
    for rows, seed in [(5, 0), (5, 5), (1, 6), (1, 7), (3, 1), (4, 2), (4, 8), (3, 9)]:
        d = S.argmin_rows_case(n, rows, seed)
        for ld in (n, n + 5):
            what = f"argmin_rows n{n} rows{rows} seed{seed} ld{ld}"
            idx = argmin_launch(d, ld, what)
            assert bool(((idx >= 0) & (idx < n)).all()), f"{what}: index out of [0, {n}): {idx.tolist()}"
            exp = S.ref_argmin(d)
            assert torch.equal(idx, exp), f"{what}: rows {(idx != exp).nonzero().flatten().tolist()} got {idx.tolist()} expected {exp.tolist()}"
    finite = torch.isfinite(d).all(1)
    assert torch.equal(S.ref_argmin(d)[finite], d.argmin(1)[finite])          # on finite rows the contract is torch.argmin's
    ones = op_in(torch.ones(8))
    refused("argmin_rows ncodes 0", ERR_BAD_ARG, [(8, F64)], lambda o: _lib().muse_argmin_rows(ones.ptr, o.ptr, 1, 0, 1, _stream()))


@pytest.mark.parametrize("N,Kc,D", [(1, 63, 16), (3, 64, 16), (4, 65, 32), (5, 1024, 16), (130, 129, 64)])
def test_vq_nearest_index_contract(N, Kc, D):
    """through ops.vq_nearest(return_dist=True): the index is the contract's argmin of the distance rows the kernel ran over - with exact
    ties (duplicated codes), and with rows that overflow to +inf / NaN (an encoder output of 3e38)"""
    ops = _ops()
    sd = seed_of("vq", N, Kc, D)
    z, cb = S.randn((N, D), sd), S.randn((Kc, D), sd + 1)
    cb[Kc // 2] = cb[0]                                       # two identical codes: equal distances
    z[0] = cb[0]
    if N > 1:
        z[-1] = 3e38                                          # |z|^2 = +inf: the row is +inf and NaN
    idx, dist = ops.vq_nearest(z.to(DEV), cb.to(DEV), return_dist=True)
    idx, dist = idx.cpu(), dist.cpu()
    assert bool(((idx >= 0) & (idx < Kc)).all()), idx.tolist()
    assert torch.equal(idx, S.ref_argmin(dist))
    assert int(idx[0]) == 0, "identical codes: the lower index"
    if N > 1:
        assert not bool(torch.isfinite(dist[-1]).any())


# =========================================================================================================================================
# f. rounding legs
# =========================================================================================================================================
def silu32(x):
    return x / (1.0 + torch.exp(-x))


def silu_bwd32(x, dy):
    s = 1.0 / (1.0 + torch.exp(-x))
    return dy * s * (1.0 + x * (1.0 - s))


def silu_inputs():
    return S.randn((3001,), 11), S.randn((3001,), 12)


def test_silu_rounding():
    L = _lib()
    x, dy = silu_inputs()
    n = x.numel()
    xi, dyi = op_in(x), op_in(dy)
    (y,) = twice("silu", [(n, F32)], lambda o: L.muse_silu_fwd(xi.ptr, o.ptr, n, _stream()))
    (dx,) = twice("silu_bwd", [(n, F32)], lambda o: L.muse_silu_bwd(xi.ptr, dyi.ptr, o.ptr, n, _stream()))
    ref = S.silu64(x)
    judge("silu_fwd", "silu", y, n, ref, 4.0 * E_REF["silu_fwd"] * ref.abs() + S.TINY)
    rb, sb = S.ref_silu_bwd(x, dy)
    judge("silu_bwd", "silu_bwd", dx, n, rb, 4.0 * E_REF["silu_bwd"] * sb + S.TINY)


SINUSOID = [(1, 2, 0.0), (7, 3, 0.0), (33, 256, 0.0), (33, 256, 1e3), (5, 257, 1e3), (300, 64, 0.0)]      # (n, dim, shift of the features)


def test_sinusoid_rounding():
    L = _lib()
    for n, dim, shift in SINUSOID:
        f = S.randn((n,), seed_of("sin", n, dim), shift)
        fi = op_in(f)
        what = f"sinusoid n{n} dim{dim} shift{shift}"
        (y,) = twice(what, [(n * dim, F32)], lambda o: L.muse_sinusoidal_encode(fi.ptr, o.ptr, n, dim, 10000.0, _stream()))
        ref, scale = S.ref_sinusoid(f, dim, 10000.0)
        body = judge("sinusoid", what, y, n * dim, ref, 4.0 * E_REF["sinusoid"] * scale)
        if dim % 2:
            assert not bool(S.bits(body.view(n, dim)[:, -1]).any()), "the padding column of an odd dim is +0"
    refused("sinusoid dim 1", ERR_BAD_ARG, [(8, F32)], lambda o: L.muse_sinusoidal_encode(fi.ptr, o.ptr, 1, 1, 10000.0, _stream()))


ADALN_R = [(2, 5, 68), (3, 257, 64)]


def test_adaln_bwd_dx_rounding():
    L = _lib()
    for B, R, C in ADALN_R:
        sd = seed_of("adalnr", B, R, C)
        dy, x, ss = S.randn((B * R, C), sd), S.randn((B * R, C), sd + 1), S.randn((B, 2 * C), sd + 2)
        dyi, xi, si = op_in(dy), op_in(x), op_in(ss)
        what = f"adaln_bwd randn B{B} R{R} C{C}"
        dx, dss = twice(what, [(dy.numel(), F32), (2 * B * C, F32)], lambda o, p: L.muse_adaln_bwd(dyi.ptr, xi.ptr, si.ptr, o.ptr, p.ptr, B, R, C, _stream()))
        edx, edss = S.ref_adaln_bwd(dy, x, ss, B, R, C)
        scale = dy.double().view(B, R, C).abs() * (1.0 + ss.double()[:, None, :C].abs())
        judge("adaln_bwd_dx", what, dx, dy.numel(), edx, 4.0 * E_REF["adaln_bwd_dx"] * scale + S.TINY)
        # the sums: exact in test_adaln_bwd_exact; here ceil(R / 4) + 2 roundings of partial sums <= sum |terms|
        t = torch.cat([(dy.double() * x.double()).view(B, R, C).abs().sum(1), dy.double().view(B, R, C).abs().sum(1)], 1)
        judge("adaln_bwd_dss", what + " dss", dss, 2 * B * C, edss, 1.01 * (math.ceil(R / 4) + 2) * S.U32 * t + S.TINY)


# ---- GlobalResponseNorm ----------------------------------------------------------------------------------------------------------------
GRN_CASES = [(2, 5, C) for C in (4, 10, 60, 64, 68, 256, 260, 1024)] + [(2, S_, 68) for S_ in (1, 2, 3, 4, 257)] + [(2, 257, 10), (1, 1025, 1024)]
# x = 1e3 + N(0, 1): G is about 1e3 sqrt(S) and N about 1 in every channel, y and x K about 1e3.  C on both sides of apply4 / scalar
# (C % 4), of the 64-channel column block and of the 256-lane stride; S = 5 and 257
GRN_OFFSET_CASES = [(2, 5, C) for C in (4, 10, 64, 68, 260)] + [(2, 257, 68), (2, 257, 10)]


def grn_inputs(B, S_, C, special=None, offset=0.0):
    sd = seed_of("grn", B, S_, C, offset) if offset else seed_of("grn", B, S_, C)
    x, dy, gamma, beta = S.randn((B, S_, C), sd, offset), S.randn((B, S_, C), sd + 1), S.randn((C,), sd + 2), S.randn((C,), sd + 3)
    if special == "zero_channel":
        x[:, :, C // 2] = 0.0
    if special == "zero_image":
        x[0] = 0.0
    return x, dy, gamma, beta


def run_grn(B, S_, C, shift=0, special=None, offset=0.0):
    L = _lib()
    x, dy, gamma, beta = grn_inputs(B, S_, C, special, offset)
    n = x.numel()
    xi, gi, bi = op_in(x, shift=shift), op_in(gamma), op_in(beta)
    what = f"grn B{B} S{S_} C{C} shift{shift} {special or ''}{' 1e3 + N(0, 1)' if offset else ''}"
    tag = "_1e3" if offset else ""
    y, stats = twice(what, [(n, F32), (2 * B * C, F32)], lambda o, s: L.muse_grn_fwd_ex(xi.ptr, gi.ptr, bi.ptr, o.ptr, None, s.ptr, B, S_, C, _stream()))
    ref, G, N = S.ref_grn(x, gamma, beta)
    bd = S.bound_grn(x, gamma, beta)
    judge("grn_stats" + tag, what + " [G | N]", stats, 2 * B * C, torch.cat([G.flatten(), N.flatten()]), torch.cat([bd["G"].flatten(), bd["N"].flatten()]))
    yb = judge("grn_fwd" + tag, what + " y", y, n, ref, bd["y"])
    if special == "zero_channel":
        c = C // 2
        assert torch.equal(yb.view(B, S_, C)[:, :, c], beta[c].expand(B, S_)), "an all-zero channel: y = beta exactly"
        assert not bool(stats[GUARD:GUARD + 2 * B * C].view(2, B, C)[:, :, c].any()), "an all-zero channel: G = N = 0"
    if C % 4 == 0 and shift == 0:
        yb16, st2 = twice(what + " bf16", [(n, BF), (2 * B * C, F32)], lambda o, s: L.muse_grn_fwd_ex(xi.ptr, gi.ptr, bi.ptr, None, o.ptr, s.ptr, B, S_, C, _stream()))
        S.check_same_bits(stats, st2, what + ": the statistics of the bf16-output call")
        b16 = S.check_out(yb16, n, ref, what + " bf16", values=False)
        assert torch.equal(S.bits(b16), S.bits(S.to_bf16(yb))), f"{what}: the bf16 output is not the rounding of the f32 output"
    else:                                                      # no kernel writes bf16 here: refused before the statistics are launched
        o, s = op_out(n, BF), op_out(2 * B * C)
        assert L.muse_grn_fwd_ex(xi.ptr, gi.ptr, bi.ptr, None, o.ptr, s.ptr, B, S_, C, _stream()) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        S.check_untouched(s.t.cpu(), what + " refused bf16: statistics")
    # backward from the statistics the forward saved
    Gs, Ns = stats[GUARD:GUARD + B * C].view(B, C), stats[GUARD + B * C:GUARD + 2 * B * C].view(B, C)
    dyi, si = op_in(dy, shift=shift), op_in(torch.cat([Gs.flatten(), Ns.flatten()]))
    dx, work = twice(what + " bwd", [(n, F32, shift), (4 * B * C, F32)],
                     lambda o, wk: L.muse_grn_bwd(dyi.ptr, xi.ptr, gi.ptr, si.ptr, o.ptr, wk.ptr, B, S_, C, _stream()))
    rb, bb = S.ref_grn_bwd(dy, x, gamma, Gs, Ns), S.bound_grn_bwd(dy, x, gamma, Gs, Ns)
    dxb = judge("grn_bwd_dx" + tag, what + " dx", dx, n, rb["dx"], bb["dx"], guard=GUARD + shift)
    bc = B * C
    s = S.bits(S.sentinel(1, F32))[0]
    wb = S.bits(work)
    assert bool((wb[:GUARD] == s).all()) and bool((wb[GUARD + 3 * bc:] == s).all()), f"{what}: the work buffer's guards / unused quarter were written"
    assert not bool((wb[GUARD:GUARD + 3 * bc] == s).any()), f"{what}: a work slot was never written"
    for k, key in enumerate(("S0", "NS1", "K")):               # S0 / N S1: the image's dbeta / dgamma terms
        got = work[GUARD + k * bc:GUARD + (k + 1) * bc]
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite {key}"
        w = S.worst_ratio(got, rb[key], bb[key])
        leg = "grn_bwd_" + key + tag
        WORST[leg] = max(WORST.get(leg, 0.0), w)
        print(f"[spatial_edges] {leg} {what}: err/bound={w:.3f} (worst so far {WORST[leg]:.3f})")
        assert w <= 1.0, f"{what} {key}: error {w:.3f} x its bound"
    if special == "zero_channel":
        assert not bool(work[GUARD + 2 * bc:GUARD + 3 * bc].view(B, C)[:, C // 2].any()), "an all-zero channel: K = 0"
    return dxb


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "misaligned"])
def test_grn(shift):
    for B, S_, C in GRN_CASES:
        run_grn(B, S_, C, shift)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "misaligned"])
def test_grn_offset_inputs(shift):
    """1e3 + N(0, 1): forward, statistics and backward against the same derived bounds"""
    for B, S_, C in GRN_OFFSET_CASES:
        dx = run_grn(B, S_, C, shift, offset=1e3)
        assert bool(torch.isfinite(dx).all())


def test_grn_special_values():
    for special in ("zero_channel", "zero_image"):
        for B, S_, C in [(2, 5, 68), (2, 7, 10)]:
            dx = run_grn(B, S_, C, 0, special)
            assert bool(torch.isfinite(dx).all())


def test_grn_dgamma_dbeta():
    """ops.grn_bwd folds the per-image terms over the batch (muse_colsum): B more additions"""
    ops = _ops()
    B, S_, C = 3, 37, 68
    x, dy, gamma, beta = grn_inputs(B, S_, C)
    _, stats = ops.grn_fwd(x.view(B * S_, C).to(DEV), gamma.to(DEV), beta.to(DEV), B, S_, want_stats=True)
    dx, dgamma, dbeta = ops.grn_bwd(dy.view(B * S_, C).to(DEV), x.view(B * S_, C).to(DEV), gamma.to(DEV), stats, B, S_)
    st = stats.cpu()
    Gs, Ns = st[:B * C].view(B, C), st[B * C:].view(B, C)
    rb, bb = S.ref_grn_bwd(dy, x, gamma, Gs, Ns), S.bound_grn_bwd(dy, x, gamma, Gs, Ns)
    for got, key in ((dgamma, "NS1"), (dbeta, "S0")):
        bound = bb[key].sum(0) + B * S.U32 * rb[key].abs().sum(0)
        assert got.shape == (C,) and bool(torch.isfinite(got).all()), f"{key}: shape {tuple(got.shape)} or a non-finite value"
        assert S.worst_ratio(got.cpu(), rb[key].sum(0), bound) <= 1.0, key
    assert dx.numel() == x.numel() and bool(torch.isfinite(dx).all()), "dx: a non-finite value"
    assert S.worst_ratio(dx.cpu(), rb["dx"], bb["dx"]) <= 1.0


# ---- GroupNorm (+ SiLU) ----------------------------------------------------------------------------------------------------------------
def gn_cases():
    """(dtype, B, HW, C, groups, silu, shift of the input)"""
    cases, k = [], 0
    for dtype, Cs in ((F32, (64, 128, 1024, 1280, 2048)), (BF, (64, 256, 2048))):
        for C in Cs:
            for HW, G in ((255, 32), (1025, 64)):
                cases.append((dtype, 2, HW, C, G, k % 2, 1e3 if k % 3 == 0 else 0.0))
                k += 1
        for HW in (1, 1023, 1024, 2049):
            cases.append((dtype, 2, HW, 128 if dtype == F32 else 64, 32, k % 2, 1e3 if k % 3 == 0 else 0.0))
            k += 1
    return cases


def gn_inputs(dtype, B, HW, C, shift):
    sd = seed_of("gn", B, HW, C, shift)
    return S.randn((B, HW, C), sd, shift).to(dtype).float(), S.randn((C,), sd + 1), S.randn((C,), sd + 2)


def run_gn(dtype, B, HW, C, G, silu, x, gamma, beta, what, eps=1e-6, finite_only=False, leg="groupnorm"):
    L = _lib()
    nch = L.muse_groupnorm_nchunk(HW)
    assert nch == (HW + S.GN_PIX - 1) // S.GN_PIX
    xi, gi, bi = op_in(x, dtype), op_in(gamma), op_in(beta)
    n, npart = x.numel(), B * nch * G * 2
    runs = []
    for _ in range(2):
        o, p = op_out(n, dtype), op_out(npart, F64)
        assert L.muse_groupnorm_silu_nhwc(xi.ptr, o.ptr, DT[dtype], gi.ptr, bi.ptr, p.ptr, B, HW, C, G, eps, silu, _stream()) == 0
        runs.append((o.t.cpu(), p.t.cpu()))
    # f64 partials through LDS atomicAdd: per slot within the rounding of an f64 sum of that length, in both runs and between them
    pref, pabs = S.ref_gn_partials(x, G), S.ref_gn_partials(x, G, terms=True)
    pbound = min(HW, S.GN_PIX) * (C // G) * 2.0 ** -53 * pabs + S.TINY
    p0 = S.check_out(runs[0][1], npart, pref, what + " partials", exact=False, bound=pbound)
    p1 = S.check_out(runs[1][1], npart, pref, what + " partials (second launch)", exact=False, bound=pbound)
    assert S.worst_ratio(p0, p1, pbound) <= 1.0, f"{what}: the two launches' partials differ by more than the rounding of their sums"
    y = S.ref_groupnorm(x, gamma, beta, G, eps, silu)[0]
    if torch.equal(S.bits(runs[0][1]), S.bits(runs[1][1])):      # the apply pass read the same partials: the same bits out
        S.check_same_bits(runs[0][0], runs[1][0], what + ": two launches with bit-equal partials")
    if finite_only:
        body = S.check_out(runs[0][0], n, y, what, values=False)
        assert bool(torch.isfinite(body.float()).all()), f"{what}: non-finite output"
        return body
    # where the partials differ in their last f64 bits between the launches so may y: both are judged
    bound = S.bound_groupnorm(x, gamma, beta, G, eps, silu, dtype == BF, fused=C // (8 if dtype == BF else 4) <= 256)
    for o, _ in runs:
        body = judge(leg, what, o, n, y, bound)
    return body


@pytest.mark.parametrize("case", gn_cases(), ids=lambda c: f"{'f32' if c[0] == F32 else 'bf16'}-HW{c[2]}-C{c[3]}-G{c[4]}-silu{c[5]}-shift{int(c[6])}")
def test_groupnorm_silu(case):
    dtype, B, HW, C, G, silu, shift = case
    x, gamma, beta = gn_inputs(dtype, B, HW, C, shift)
    run_gn(dtype, B, HW, C, G, silu, x, gamma, beta, f"groupnorm {dtype} B{B} HW{HW} C{C} G{G} silu{silu} shift{shift}",
           leg="groupnorm" + ("_bf16" if dtype == BF else "") + ("_1e3" if shift else ""))


def test_groupnorm_constant_group():
    """a constant group: the variance clamps to 0 (never negative under the root), outputs finite"""
    for dtype, C in ((F32, 128), (BF, 64)):
        x, gamma, beta = gn_inputs(dtype, 2, 300, C, 0.0)
        x[:, :, :C // 32] = 1000.0
        x[1, :, C // 32:2 * (C // 32)] = -0.1 if dtype == F32 else -0.5
        run_gn(dtype, 2, 300, C, 32, 1, x, gamma, beta, f"groupnorm constant group {dtype}", finite_only=True)


def test_groupnorm_refusals():
    """by return code, nothing launched: C > 2048, a vpp that does not divide 256, groups other than 32 / 64"""
    L = _lib()
    x = op_in(torch.zeros(2112))
    for dt_, C, G in [(0, 2112, 32), (0, 96, 32), (0, 64, 16), (1, 2112, 32), (1, 96, 32), (1, 68, 32)]:
        o, p = op_out(2112, F32 if dt_ == 0 else BF), op_out(128, F64)
        assert L.muse_groupnorm_silu_nhwc(x.ptr, o.ptr, dt_, x.ptr, x.ptr, p.ptr, 1, 1, C, G, 1e-6, 1, _stream()) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        S.check_untouched(o.t.cpu(), f"groupnorm refused C{C} G{G}")
        S.check_untouched(p.t.cpu(), f"groupnorm refused C{C} G{G} partials")


# =========================================================================================================================================
# E_ref: torch's float32 CPU computation against float64 over the same cases (python tests/test_gpu_spatial_edges.py; no GPU)
# =========================================================================================================================================
def measure_e_ref():
    E = {}

    def put(name, got, ref, scale):
        E[name] = max(E.get(name, 0.0), S.measure(got, ref, scale))

    x, dy = silu_inputs()
    put("silu_fwd", silu32(x), S.silu64(x), S.silu64(x).abs())
    rb, sb = S.ref_silu_bwd(x, dy)
    put("silu_bwd", silu_bwd32(x, dy), rb, sb)
    for n, dim, shift in SINUSOID:
        f = S.randn((n,), seed_of("sin", n, dim), shift)
        half = dim // 2
        ang = f[:, None] * torch.exp(-math.log(10000.0) / half * torch.arange(half, dtype=F32))[None, :]
        got = torch.zeros(n, dim)
        got[:, :half], got[:, half:2 * half] = ang.cos(), ang.sin()
        ref, scale = S.ref_sinusoid(f, dim, 10000.0)
        put("sinusoid", got, ref, scale)
    for B, R, C in ADALN_R:
        sd = seed_of("adalnr", B, R, C)
        dy_, ss = S.randn((B * R, C), sd), S.randn((B, 2 * C), sd + 2)
        edx, _ = S.ref_adaln_bwd(dy_, dy_, ss, B, R, C)
        put("adaln_bwd_dx", dy_.view(B, R, C) * (1.0 + ss[:, None, :C]), edx, dy_.double().view(B, R, C).abs() * (1.0 + ss.double()[:, None, :C].abs()))
    for B, H, W, C in [(2, 5, 7, 64), (3, 5, 7, 260), (2, 3, 5, 1024), (2, 9, 17, 8), (2, 5, 7, 10)]:
        c = S.dwconv_case("randn", B, H, W, C, seed_of("dwr", B, H, W, C))
        got = F.conv2d(c["a"].permute(0, 3, 1, 2), c["w"].view(C, 1, 3, 3), padding=1, groups=C).permute(0, 2, 3, 1)
        put("dwconv", got, c["y"], S.ref_dwconv(c["a"].abs(), c["w"].abs()))
    for dtype, B, HW, C, G, silu, shift in gn_cases():
        x, gamma, beta = gn_inputs(dtype, B, HW, C, shift)
        got = F.group_norm(x.transpose(1, 2), G, gamma, beta, 1e-6).transpose(1, 2)
        _, t, scale = S.ref_groupnorm(x, gamma, beta, G, 1e-6, 0)
        put("groupnorm_1e3" if shift else "groupnorm", got, t, scale)
    for B, S_, C, offset in [c + (0.0,) for c in GRN_CASES] + [c + (1e3,) for c in GRN_OFFSET_CASES]:
        tag = "_1e3" if offset else ""
        x, dy_, gamma, beta = grn_inputs(B, S_, C, offset=offset)
        xr = x.clone().requires_grad_(True)
        Gx = torch.norm(xr, p=2, dim=1, keepdim=True)
        y32 = gamma * (xr * (Gx / (Gx.mean(dim=-1, keepdim=True) + 1e-6))) + beta + xr
        y32.backward(dy_)
        ref, G64, N64 = S.ref_grn(x, gamma, beta)
        put("grn_fwd" + tag, y32.detach(), ref, (gamma.double() * (x.double() * N64[:, None])).abs() + beta.double().abs() + x.double().abs())
        rb = S.ref_grn_bwd(dy_, x, gamma, G64, N64)
        put("grn_bwd_dx" + tag, xr.grad, rb["dx"], dy_.double().abs() * ((gamma.double() * N64).abs() + 1.0)[:, None] + (x.double() * rb["K"][:, None]).abs())
    return E


if __name__ == "__main__":
    torch.set_num_threads(8)
    t0 = time.time()
    for k, v in measure_e_ref().items():
        print(f'    "{k}": {v:.3e},')
    print(f"({time.time() - t0:.1f} s)", file=sys.stderr)
