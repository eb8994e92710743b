"""GPU (-m gpu): every GEMM path of csrc/ (gemm_core.h, gemm256.h, gemm256_host.h, gemm256p.h, gemm_p.h, gemm_p.hip, gemm.hip) and the slice reducers of rowops.hip
with EXACT integer probes at each edge of their dispatch, plus a small per-element rounding leg.  tests/gemm_cpu.py holds the reference,
the storage builders, the checks and a tiled contract model; tests/test_gemm_cpu.py proves on a CPU that the checks fail for nine seeded
bookkeeping defects.  profiles/gemm_edges.md has the edge table and the MI355X's figures; DESIGN.md ("GEMM output contract") the contract.

Every exact case (run_case):
  * operands are seeded integers with K max|a| max|b| < 2^24 (gemm_cpu.assert_exact), the reference is float64 on the CPU: an f32 output
    must be torch.equal to it, a bf16 output bit-equal to its round-to-nearest-even - or, with a residual / an old C, to the once- or
    twice-rounded value DESIGN.md lists for the path (contract_rounding);
  * operand storage contract (include/muse_hip.h "Requirements", PlainLoader::load of gemm_core.h, Dma<L, BK>::init / issue of gemm256.h): the
    loaders fetch 16-byte chunks and mask a chunk by its first element, so a k-contiguous operand is read on rows r < R and columns
    k < roundup(K, chunk) - columns K .. roundup(K, chunk) must hold zeros and do -, a k-major one on k rows < K and columns
    r < roundup(R, chunk).  Everything else (rows past M / N / K, columns up to ld, the bytes in front of the operand's offset, the gap
    between batch groups) is NaN: one stray read turns a row or a column of C into NaN;
  * C is allocated with ldc > N, extra rows behind M and, in batches, gaps between the slices, all filled with a NaN bit pattern no result
    has (0x7FC0DEAD / 0x7FC1): it must come back bit for bit;
  * the case is launched twice from the same initial C: bit-identical.

Edges (thresholds as the code has them; file: function):
  128^2 kernel, MUSE_GEMM256=0 (gemm_core.h: gemm_kernel, PlainLoader; gemm.hip: dispatch_bm)
    M, N in {1, 15, 16, 17, 127, 128, 129, 257}: row / column masks inside a 16-row fragment, a 64-row wave, a 128 tile; 1 .. 3 tiles
    K in {1, 7, 8, 9, 63, 64, 65, 128, 129, 192, 200}: chunk masks (8 bf16 / 4 f32), 1 .. 4 K-tiles of 64 - an odd count meets the even
      round-up nk2 of the two-stage loop (launch_gemm: gemm_stages = 2 on every bf16 layout but (0, 0)), (0, 0) and f32 the one-stage loop
    epilogue: fast (C through LDS) iff N % EPC == 0, ldc % EPC == 0, C 16-byte aligned, residual absent or (ldr % EPC == 0 and aligned),
      EPC = 4 f32 / 8 bf16 (gemm_kernel: `fast`); each condition flipped alone (EPILOGUE_FLIPS)
    atomic split-K: split_k in {2, 3, 7} at nk = 4 and 9 (per = ceil(nk / split_k): nk = 4, split 3 leaves slice 2 empty; nk = 9,
      split 7 leaves slices 5, 6 empty); workspace split-K: the same, into NaN
  256^2 launch-per-tile kernel, MUSE_GEMM256=1 MUSE_G256P=0 (gemm256.h: tile_body, Pipe / Pipe32; gemm_p.h: gemm256_ok; gemm.hip: takes_gemm256)
    M in {8, 64, 248, 256, 264, 520}, N in {8, 256, 264}, K in {8, 56, 64, 72, 120, 128, 136, 200} (kt_last even round-up: nk = 1, 3),
    MUSE_G256_BK = 64 | 32 (gemm256_host.h: launch_gemm256_l), act = 1 -> 128 (gemm256_ok)
  persistent kernel, MUSE_G256P=1 (gemm_p.hip: eligible, launch; gemm256p.h): K <= 128 -> 256; M < 256 has ntm_full = 0 (strip only);
    N = 256 t at M = 256, t = 1 .. 9: nfull % 8 = 1 .. 7, 0, 1 (sc.q, sc.r: the per-XCD queue lengths); > 256 tiles -> a.dyn
  muse_gemm_x3 (gemm.hip; gemm256.h: PipeX3): M, N >= 128, K >= 64, batch 1, no act, a_lo / b_lo positive multiples of 8
  half operands (gemm.hip: takes_gemm256): M, N >= 128, K >= 64, else MUSE_ERR_UNSUPPORTED
  grouped dW (gemm.hip: group_fill; gemm256.h: kernel_group): 1 .. 8 products, M, N >= 256, K >= 128, layout (1, 1)
  skinny split-K (ops.gemm: SKINNY): sk = ceil(nk / ceil(nk / sk)): M = 256, K = 2816: 16 -> 15
"""
import contextlib
import ctypes as C
import os
import time
import zlib

import pytest
import torch

import gemm_cpu as G
from gemm_cpu import BF, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_BAD_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """a launch that faulted leaves the device unusable for the rest of the process: end the session there rather than start more work"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU error after a GEMM edge test, stopping: {e}", returncode=3)


def _ops():
    from muse import ops
    return ops


def _lib():
    from muse._hip import lib
    return lib()


@contextlib.contextmanager
def env(**kv):
    """set (value) or unset (None) environment switches the library reads per call"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


ENV128 = dict(MUSE_GEMM256="0", MUSE_G256P="1", MUSE_G256_BK=None)
ENV256 = dict(MUSE_GEMM256="1", MUSE_G256P="0", MUSE_G256_BK=None)
ENV256_BK32 = dict(MUSE_GEMM256="1", MUSE_G256P="0", MUSE_G256_BK="32")
ENVP = dict(MUSE_GEMM256="1", MUSE_G256P="1", MUSE_G256_BK=None)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def make_desc(A, B, Cp, M, N, K, *, dtype, out_dtype, la=0, lb=0, lda, ldb, ldc, ldr=0, alpha=1.0, bias=0, rowvec=0, residual=0, batch=1,
              zdiv=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), accumulate=0, act=0, split_k=1, split_stride=0):
    """a muse_gemm_desc from raw addresses (host-only queries take aligned fake pointers: they never launch and never dereference)"""
    from muse._hip import GemmDesc
    code = {F32: 0, BF: 1, F16: 2}
    d = GemmDesc()
    d.A, d.B, d.C = A, B, Cp
    d.bias, d.rowvec, d.residual = bias or None, rowvec or None, residual or None
    d.dtype, d.out_dtype, d.layout_a, d.layout_b = code[dtype], code[out_dtype], la, lb
    d.M, d.N, d.K, d.batch, d.zdiv = M, N, K, batch, zdiv
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.sA0, d.sA1 = sA
    d.sB0, d.sB1 = sB
    d.sC0, d.sC1 = sC
    d.alpha, d.accumulate, d.act, d.split_k, d.split_stride = alpha, int(accumulate), act, split_k, split_stride
    return d


def gemm_path(d):
    return _lib().muse_gemm_path(C.byref(d))


def gemm_tile(d):
    return _lib().muse_gemm_tile(C.byref(d))


def contract_rounding(path, odt, N, ldc, c_off, residual, accumulate, ldr, r_off):
    """DESIGN.md, GEMM output contract: how often a bf16 output with a residual / an old C is rounded on the path that runs.
    128^2 (gemm_core.h gemm_kernel): the fast epilogue stages the bf16 tile in LDS and adds behind it - twice; the direct epilogue adds in
    registers - once.  256^2 (gemm256.h tile_body): bf16 residual / accumulate are added in the store loop behind the staged bf16 tile -
    twice.  The persistent kernel refuses them (gemm_p.hip eligible)."""
    if odt != BF or not (residual or accumulate):
        return "once"
    if path == 256:
        return "twice"
    assert path == 128
    fast = N % 8 == 0 and ldc % 8 == 0 and c_off % 8 == 0 and (not residual or (ldr % 8 == 0 and r_off % 8 == 0))
    return "twice" if fast else "once"


def build_case(dt, odt, la, lb, M, N, K, *, alpha=1.0, bias=False, rowvec=False, residual=False, accumulate=False, batch=1, zdiv=1,
               split_k=1, split=None, ldc=None, c_off=0, ldr=None, r_off=0, wide="a", x3=False, scale=None, lead=0, res_lim=None, bias_lim=50):
    """the probe, its storage and its exact pre-activation.  wide: the operand that carries the 11-bit integers (f32 / half operands)"""
    key = (str(dt), str(odt), la, lb, M, N, K, alpha, bias, rowvec, residual, accumulate, batch, zdiv, split_k, split, ldc, c_off, ldr, r_off,
           wide, x3)
    sd = seed_of(*key)
    ch = G.CHUNK[dt]
    if dt == BF:
        amax = bmax = 7
    else:
        amax, bmax = (1023, 7) if wide == "a" else (7, 1023)
    res_lim = res_lim if res_lim is not None else (1000 if odt == F32 else 9)
    extra = (bias_lim if bias else 0) + (50 if rowvec else 0) + (res_lim if residual else 0) + (res_lim if accumulate or split == "atomic" else 0)
    G.assert_exact(K, amax, bmax, terms=3 if x3 else 1, extra=extra)
    c = dict(dt=dt, odt=odt, la=la, lb=lb, M=M, N=N, K=K, alpha=alpha, batch=batch, zdiv=zdiv, split_k=split_k, split=split, c_off=c_off,
             r_off=r_off, x3=x3)
    Z = batch
    A = G.ints((Z, M, K), amax, sd + 1)
    B = G.ints((Z, N, K), bmax, sd + 2)
    if x3:
        assert Z == 1
        Al, Bl = G.ints((Z, M, K), 7, sd + 3), G.ints((Z, N, K), 7, sd + 4)
        acc = G.product_x3(A, Al, B, Bl)
        ah, lda = G.place(A[0], la, dt, lead=lead)
        al, _ = G.place(Al[0], la, dt, lead=lead)
        bh, ldb = G.place(B[0], lb, dt)
        bl, _ = G.place(Bl[0], lb, dt)
        c["A"], c["B"], c["x3_lo"] = torch.cat([ah, al]), torch.cat([bh, bl]), (ah.numel(), bh.numel())
        c["sA"] = c["sB"] = (0, 0)
    else:
        acc = G.product(A, B)
        if Z == 1:
            c["A"], lda = G.place(A[0], la, dt, lead=lead)
            c["B"], ldb = G.place(B[0], lb, dt)
            c["sA"] = c["sB"] = (0, 0)
        else:
            c["A"], lda, c["sA"] = G.place_batched(A, la, dt, zdiv, lead=lead)
            c["B"], ldb, c["sB"] = G.place_batched(B, lb, dt, zdiv)
    c["lda"], c["ldb"], c["a_off"] = lda, ldb, lead
    if scale is not None:                                   # a half image that carries a power-of-two scale: the values are value * scale
        c["A"] = c["A"] * scale
        c["a_scale"] = scale
    c["bias_v"] = G.ints((N,), bias_lim, sd + 5) if bias else None
    c["rowvec_v"] = G.ints((M,), 50, sd + 6) if rowvec else None
    c["res_v"] = G.ints((M, N), res_lim, sd + 7) if residual else None
    c["old_v"] = G.ints((Z, M, N), res_lim, sd + 8) if (accumulate or split == "atomic") else None
    c["accumulate"] = accumulate
    c["pre"] = G.pre_activation(acc, alpha, c["bias_v"], c["rowvec_v"])
    epc = 16 // (4 if odt == F32 else 2)
    if split == "ws":
        c["ldc"], c["sC"] = N, (0, 0)
        c["split_stride"] = M * N
        c["C0"] = torch.full((split_k * M * N + 8,), float("nan"), dtype=F32)
        c["idx"] = None
    else:
        c["ldc"] = ldc if ldc is not None else G.rup(N, epc) + epc
        block = G.rup((M + 2) * c["ldc"], 8)
        c["sC"] = (zdiv * block + 8, block) if Z > 1 else (0, 0)
        c["split_stride"] = 0
        c["C0"], c["idx"] = G.alloc_c(M, N, odt, c["ldc"], c_off, batch=Z, zdiv=zdiv, sC=c["sC"], old=c["old_v"])
    c["ldr"] = (ldr if ldr is not None else G.rup(N, epc) + 2 * epc) if residual else 0
    c["R"] = G.residual_storage(c["res_v"], odt, c["ldr"], r_off) if residual else None
    c["bias"] = G.vec(c["bias_v"]) if bias else None
    c["rowvec"] = G.vec(c["rowvec_v"]) if rowvec else None
    return c


def fresh(C0):
    """a new device copy of a case's initial C (sentinel padding, old values)"""
    return C0.to(DEV, copy=True)


def to_dev(c):
    d = {}
    for k in ("A", "B", "R", "bias", "rowvec"):
        d[k] = c[k].to(DEV) if c[k] is not None else None
    if c.get("a_scale") is not None:
        d["A"]._muse_scale = c["a_scale"]
    return d


def case_desc(c, d, Cd, act=0):
    esz = lambda t: t.element_size()
    return make_desc(d["A"].data_ptr() + c["a_off"] * esz(d["A"]), d["B"].data_ptr(), Cd.data_ptr() + c["c_off"] * esz(Cd), c["M"], c["N"], c["K"],
                     dtype=c["dt"], out_dtype=c["odt"], la=c["la"], lb=c["lb"], lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], ldr=c["ldr"],
                     alpha=c["alpha"], bias=d["bias"].data_ptr() if d["bias"] is not None else 0,
                     rowvec=d["rowvec"].data_ptr() if d["rowvec"] is not None else 0,
                     residual=(d["R"].data_ptr() + c["r_off"] * esz(d["R"])) if d["R"] is not None else 0, batch=c["batch"], zdiv=c["zdiv"],
                     sA=c["sA"], sB=c["sB"], sC=c["sC"], accumulate=c["accumulate"], act=act, split_k=c["split_k"],
                     split_stride=c["split_stride"])


def launch(c, d, Cd, act=0):
    ops = _ops()
    R = d["R"][c["r_off"]:] if d["R"] is not None else None
    out = ops.gemm(d["A"], d["B"], Cd, c["M"], c["N"], c["K"], la=c["la"], lb=c["lb"], lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"],
                   a_off=c["a_off"], c_off=c["c_off"], alpha=c["alpha"], bias=d["bias"], rowvec=d["rowvec"], residual=R, ldr=c["ldr"],
                   batch=c["batch"], zdiv=c["zdiv"], sA=c["sA"], sB=c["sB"], sC=c["sC"], accumulate=c["accumulate"], act=act,
                   split_k=c["split_k"], split_stride=c["split_stride"], x3_lo=c.get("x3_lo"))
    assert out is not None, "the four-plane kernel refused a product it documents to take"
    return Cd


def run_case(c, path=None, rounding=None, what=""):
    """launch twice, check against the exact reference, the guards and the second launch.  path: the answer muse_gemm_path must give
    (None: x3, which has no path query)."""
    d = to_dev(c)
    outs = []
    for _ in range(2):
        Cd = fresh(c["C0"])
        if path is not None:
            got = gemm_path(case_desc(c, d, Cd))
            assert got == path, f"{what}: muse_gemm_path says {got}, this case is meant for {path}"
        launch(c, d, Cd)
        outs.append(Cd.cpu())
    torch.cuda.synchronize()
    G.check_same_bits(outs[0], outs[1], what)
    if c["split"] == "ws":
        M, N, sk = c["M"], c["N"], c["split_k"]
        ws = outs[0][:sk * M * N].view(sk, M, N)
        G.check_workspace(ws, sk, G.used_slices(c["K"], sk), G.expected(c["pre"][0], F32), what)
        assert bool(outs[0][sk * M * N:].isnan().all()), f"{what}: the workspace was written behind its last slice"
        return outs[0]
    if rounding is None:
        rounding = contract_rounding(path if path in (128, 256) else 256, c["odt"], c["N"], c["ldc"], c["c_off"], c["res_v"] is not None,
                                     c["accumulate"], c["ldr"], c["r_off"])
    exp = G.expected(c["pre"], c["odt"], c["res_v"], c["old_v"], rounding)
    G.check_c(outs[0], c["C0"], c["idx"], exp, what)
    return outs[0]


LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
TYPES = [(F32, F32), (BF, F32), (BF, BF)]
TID = {(F32, F32): "f32", (BF, F32): "bf16-f32", (BF, BF): "bf16-bf16"}


def tname(t):
    return TID[t]


# =========================================================================================================================================
# 1a. the 128^2 kernel
# =========================================================================================================================================
MN128 = [1, 15, 16, 17, 127, 128, 129, 257]
K128 = [1, 7, 8, 9, 63, 64, 65, 128, 129, 192, 200]
SHAPES128 = ([(m, 136, 72) for m in MN128] + [(129, n, 200) for n in MN128] + [(17, 129, k) for k in K128] +
             [(257, 257, 200), (1, 1, 1), (128, 128, 64)])


@pytest.mark.parametrize("M,N,K", SHAPES128, ids=lambda v: str(v))
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("types", TYPES, ids=tname)
def test_128_shapes(types, la, lb, M, N, K):
    """gemm_core.h gemm_kernel / PlainLoader: every M, N, K edge on every layout and type; f32 cases alternate the wide operand"""
    with env(**ENV128):
        c = build_case(types[0], types[1], la, lb, M, N, K, wide="ab"[(M + N + K) & 1])
        run_case(c, path=128, what=f"128^2 {tname(types)} ({la},{lb}) {M}x{N}x{K}")


# the fast epilogue's four conditions, each flipped alone from a shape that meets all of them (gemm_kernel: `fast`); EPC = 4 (f32) / 8 (bf16)
def epilogue_flips(odt):
    e = 4 if odt == F32 else 8
    N = 136
    return {
        "fast": dict(N=N, ldc=N + e, c_off=0, ldr=N + 2 * e, r_off=0),
        "N%EPC": dict(N=N + 1, ldc=N + 1 + (e - 1) + e, c_off=0, ldr=N + 1 + (e - 1) + 2 * e, r_off=0),
        "ldc%EPC": dict(N=N, ldc=N + e + 1, c_off=0, ldr=N + 2 * e, r_off=0),
        "c_off": dict(N=N, ldc=N + e, c_off=1, ldr=N + 2 * e, r_off=0),
        "ldr%EPC": dict(N=N, ldc=N + e, c_off=0, ldr=N + 2 * e + 1, r_off=0),
        "res_off": dict(N=N, ldc=N + e, c_off=0, ldr=N + 2 * e, r_off=1),
    }


FLIPS = ["fast", "N%EPC", "ldc%EPC", "c_off", "ldr%EPC", "res_off"]


@pytest.mark.parametrize("flip", FLIPS)
@pytest.mark.parametrize("la,lb", [(0, 0), (1, 1)])
@pytest.mark.parametrize("types", TYPES, ids=tname)
def test_128_epilogue_flips(types, la, lb, flip):
    """residual + accumulate on each side of each condition of the fast epilogue.  For bf16 outputs the two epilogues round differently
    (contract_rounding) and the probe makes that visible: the once- and the twice-rounded references differ on a known share of elements"""
    f = epilogue_flips(types[1])[flip]
    with env(**ENV128):
        c = build_case(types[0], types[1], la, lb, 129, f["N"], 200, residual=True, accumulate=True, ldc=f["ldc"], c_off=f["c_off"],
                       ldr=f["ldr"], r_off=f["r_off"])
        if types[1] == BF:
            share = G.once_twice_share(c["pre"], c["res_v"], c["old_v"])
            assert share > 0.05, share           # (sums of K = 200 products of [-7, 7] pass 256 for most elements: bf16 steps of 2 and 4)
            want = "twice" if flip == "fast" else "once"
            assert contract_rounding(128, BF, f["N"], f["ldc"], f["c_off"], True, True, f["ldr"], f["r_off"]) == want
        run_case(c, path=128, what=f"128^2 epilogue {flip} {tname(types)} ({la},{lb})")


COMBOS = [(b, r, s, a) for b in (0, 1) for r in (0, 1) for s in (0, 1) for a in (0, 1) if b or r or s or a]


@pytest.mark.parametrize("bias,rowvec,residual,accumulate", COMBOS)
@pytest.mark.parametrize("N", [136, 131], ids=["fast", "direct"])
@pytest.mark.parametrize("types", TYPES, ids=tname)
def test_128_epilogue_combos(types, N, bias, rowvec, residual, accumulate):
    alpha = (1.0, 0.5, 0.25)[(bias + 2 * rowvec + 4 * residual + 8 * accumulate) % 3]
    la, lb = LAYOUTS[(bias + 2 * rowvec + residual + accumulate) % 4]
    with env(**ENV128):
        c = build_case(types[0], types[1], la, lb, 129, N, 200, alpha=alpha, bias=bool(bias), rowvec=bool(rowvec), residual=bool(residual),
                       accumulate=bool(accumulate))
        run_case(c, path=128, what=f"128^2 combo {tname(types)} N={N} b{bias} r{rowvec} s{residual} a{accumulate} alpha={alpha}")


@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("types", TYPES, ids=tname)
def test_128_strided_batch(types, la, lb):
    """batch 6 as (2 groups x zdiv 3) with distinct group / inner strides on A, B and C, as the attention core's (image, head) products"""
    with env(**ENV128):
        c = build_case(types[0], types[1], la, lb, 65, 72, 72, batch=6, zdiv=3, bias=True, accumulate=True, alpha=0.5, lead=G.CHUNK[types[0]])
        assert c["sA"][0] != 3 * c["sA"][1] and c["sC"][0] != 3 * c["sC"][1]
        run_case(c, path=128, what=f"128^2 batch {tname(types)} ({la},{lb})")


@pytest.mark.parametrize("K", [200, 520], ids=["nk4", "nk9"])
@pytest.mark.parametrize("split_k", [2, 3, 7])
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["atomic", "ws"])
def test_128_split_k(mode, dt, la, lb, split_k, K):
    """atomic slices add onto a preset integer C (order-independent for integers: exact); workspace slices go into NaN - exactly
    ceil(nk / ceil(nk / split_k)) slices are written and sum to the reference"""
    with env(**ENV128):
        c = build_case(dt, F32, la, lb, 129, 72, K, split_k=split_k, split=mode, alpha=0.5 if mode == "atomic" else 1.0)
        run_case(c, path=128, what=f"128^2 split {mode} {dt} ({la},{lb}) split_k={split_k} K={K}")


# =========================================================================================================================================
# 1b. the 256^2 launch-per-tile kernel
# =========================================================================================================================================
M256, N256, K256 = [8, 64, 248, 256, 264, 520], [8, 256, 264], [8, 56, 64, 72, 120, 128, 136, 200]
SHAPES256 = [(m, 264, 136) for m in M256] + [(264, n, 72) for n in N256] + [(264, 8, k) for k in K256] + [(8, 8, 8), (520, 264, 200)]
TYPES256 = [(BF, BF), (BF, F32)]


@pytest.mark.parametrize("M,N,K", SHAPES256, ids=lambda v: str(v))
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("types", TYPES256, ids=tname)
@pytest.mark.parametrize("bk", [64, 32])
def test_256_shapes(bk, types, la, lb, M, N, K):
    """gemm256.h tile_body with Pipe (BK = 64, two stages) and Pipe32 (BK = 32, five stages)"""
    with env(**(ENV256 if bk == 64 else ENV256_BK32)):
        c = build_case(types[0], types[1], la, lb, M, N, K)
        run_case(c, path=256, what=f"256^2 bk{bk} {tname(types)} ({la},{lb}) {M}x{N}x{K}")


@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("types", TYPES256, ids=tname)
def test_256_strided_batch(types, la, lb):
    with env(**ENV256):
        c = build_case(types[0], types[1], la, lb, 72, 264, 72, batch=3, zdiv=3, rowvec=True, accumulate=True, lead=8)
        run_case(c, path=256, what=f"256^2 batch {tname(types)} ({la},{lb})")


@pytest.mark.parametrize("bias,rowvec,residual,accumulate", COMBOS)
@pytest.mark.parametrize("types", TYPES256, ids=tname)
def test_256_epilogue_combos(types, bias, rowvec, residual, accumulate):
    """the 256^2 epilogue stages the bf16 tile and adds a bf16 residual / old C behind it: twice rounded (f32 outputs add in fragment
    layout before the staging: exact)"""
    alpha = (1.0, 0.5, 0.25)[(bias + 2 * rowvec + 4 * residual + 8 * accumulate) % 3]
    la, lb = LAYOUTS[(bias + 2 * rowvec + residual + accumulate) % 4]
    with env(**ENV256):
        c = build_case(types[0], types[1], la, lb, 264, 264, 200, alpha=alpha, bias=bool(bias), rowvec=bool(rowvec), residual=bool(residual),
                       accumulate=bool(accumulate))
        if types[1] == BF and (residual or accumulate) and alpha == 1.0:
            assert G.once_twice_share(c["pre"], c["res_v"], c["old_v"]) > 0.05
        run_case(c, path=256, what=f"256^2 combo {tname(types)} b{bias} r{rowvec} s{residual} a{accumulate} alpha={alpha}")


@pytest.mark.parametrize("split_k", [2, 3, 5])
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("bk", [64, 32])
def test_256_split_k_workspace(bk, la, lb, split_k):
    """slices are cut on 64-wide boundaries for either pipeline (tile_body: nk64); K = 520 = 9 tiles: 2 -> 5 + 4, 3 -> 3 x 3, 5 -> 2 each,
    the fifth holds one; K = 264 = 5 tiles with 3 slices: 2 + 2 + 1"""
    with env(**(ENV256 if bk == 64 else ENV256_BK32)):
        for K in (520, 264):
            c = build_case(BF, F32, la, lb, 264, 72, K, split_k=split_k, split="ws")
            run_case(c, path=256, what=f"256^2 split ws bk{bk} ({la},{lb}) split_k={split_k} K={K}")


def test_256_activation_stays_on_128():
    """gemm256_ok refuses an activation: the same environment reports 128"""
    with env(**ENV256):
        d = make_desc(4096, 8192, 16384, 264, 264, 136, dtype=BF, out_dtype=BF, lda=136, ldb=136, ldc=264)
        assert gemm_path(d) == 256
        d.act = 1
        assert gemm_path(d) == 128 and gemm_tile(d) == 128


# =========================================================================================================================================
# 1c. the persistent kernel
# =========================================================================================================================================
FORMS_P = [(BF, BF, 0), (BF, BF, 1), (BF, F32, 0)]                      # operand, output, lb (la = 0)
SHAPES_P = ([(264, 264, k) for k in (136, 192, 200, 264)] + [(m, 264, 136) for m in (64, 248, 256, 264, 520)] +
            [(256, 256 * t, 136) for t in range(1, 10)] + [(520, 520, 136)])


@pytest.mark.parametrize("M,N,K", SHAPES_P, ids=lambda v: str(v))
@pytest.mark.parametrize("form", FORMS_P, ids=["bf16-lb0", "bf16-lb1", "f32-lb0"])
def test_persistent_shapes(form, M, N, K):
    """gemm_p.hip launch: ntm_full = M / 256 (0 at M = 64, 248: strip only), nfull % 8 through 1 .. 7, 0, 1 at N = 256 t"""
    dt, odt, lb = form
    with env(**ENVP):
        c = build_case(dt, odt, 0, lb, M, N, K)
        run_case(c, path=257, what=f"persistent {form} {M}x{N}x{K}")


def test_persistent_k128_is_launch_per_tile():
    with env(**ENVP):
        c = build_case(BF, BF, 0, 0, 264, 264, 128)
        run_case(c, path=256, what="persistent K=128")


def test_persistent_dynamic_queues():
    """more than 256 tiles: 17 x 17 full tiles + a 17-tile strip, a.dyn set (queues longer than an XCD's 32 workgroups).  The f32 matmul
    of the CPU is exact for these integers (136 * 49 < 2^24) and takes about a second."""
    M, N, K = 4360, 4104, 136
    G.assert_exact(K, 7, 7)
    A, B = G.ints((M, K), 7, 11), G.ints((N, K), 7, 12)
    t0 = time.perf_counter()
    ref = A.float() @ B.float().t()
    print(f"CPU f32 reference {M}x{N}x{K}: {time.perf_counter() - t0:.2f} s")
    exp = ref.to(BF)
    a, lda = G.place(A, 0, BF)
    b, ldb = G.place(B, 0, BF)
    ldc = N + 8
    C0, idx = G.alloc_c(M, N, BF, ldc)
    ad, bd = a.to(DEV), b.to(DEV)
    with env(**ENVP):
        outs = []
        for _ in range(2):
            Cd = fresh(C0)
            assert gemm_path(make_desc(ad.data_ptr(), bd.data_ptr(), Cd.data_ptr(), M, N, K, dtype=BF, out_dtype=BF, lda=lda, ldb=ldb, ldc=ldc)) == 257
            _ops().gemm(ad, bd, Cd, M, N, K, lda=lda, ldb=ldb, ldc=ldc)
            outs.append(Cd)
        assert torch.equal(G.bits(outs[0]), G.bits(outs[1]))
    G.check_c(outs[0].cpu(), C0, idx, exp[None], "persistent dyn 4360x4104x136")


@pytest.mark.parametrize("which", ["residual", "accumulate"])
@pytest.mark.parametrize("M", [264, 248])
def test_persistent_f32_start_values(which, M):
    """f32 outputs start the accumulators from the residual / the old C (alpha = 1): exact for integers"""
    with env(**ENVP):
        c = build_case(BF, F32, 0, 0, M, 264, 200, residual=which == "residual", accumulate=which == "accumulate")
        run_case(c, path=257, what=f"persistent f32 {which} M={M}")


REFUSED_P = {
    "f32 residual+accumulate": dict(odt=F32, residual=True, accumulate=True),
    "f32 residual alpha": dict(odt=F32, residual=True, alpha=0.5),
    "f32 accumulate alpha": dict(odt=F32, accumulate=True, alpha=0.25),
    "bf16 residual": dict(odt=BF, residual=True),
    "bf16 accumulate": dict(odt=BF, accumulate=True),
    "bias": dict(odt=BF, bias=True),
    "rowvec": dict(odt=F32, rowvec=True),
    "la=1": dict(odt=BF, la=1),
    "f32 lb=1": dict(odt=F32, lb=1),
}


@pytest.mark.parametrize("name", list(REFUSED_P))
def test_persistent_refusals_fall_back_exactly(name):
    """gemm_p.hip eligible: each refused combination reports the launch-per-tile kernel and is still exact"""
    kw = dict(REFUSED_P[name])
    odt, la, lb = kw.pop("odt"), kw.pop("la", 0), kw.pop("lb", 0)
    with env(**ENVP):
        c = build_case(BF, odt, la, lb, 264, 264, 200, **kw)
        run_case(c, path=256, what=f"persistent refusal {name}")


# =========================================================================================================================================
# 1d. muse_gemm_x3: four hand-made integer planes, no lo x lo term
# =========================================================================================================================================
SHAPES_X3 = [(128, 264, 136), (136, 136, 136), (264, 128, 136)] + [(136, 264, k) for k in (64, 72, 136, 200)]


@pytest.mark.parametrize("M,N,K", SHAPES_X3, ids=lambda v: str(v))
@pytest.mark.parametrize("la,lb", LAYOUTS)
def test_x3_planes(la, lb, M, N, K):
    """A_hi, A_lo, B_hi, B_lo unrelated integers in [-7, 7]: the lo planes carry full weight, so a dropped, swapped or misplaced plane, or an
    A_lo B_lo term, changes almost every element"""
    c = build_case(BF, F32, la, lb, M, N, K, x3=True)
    run_case(c, what=f"x3 ({la},{lb}) {M}x{N}x{K}")


@pytest.mark.parametrize("split_k", [2, 3])
@pytest.mark.parametrize("la,lb", LAYOUTS)
def test_x3_split_k_workspace(la, lb, split_k):
    c = build_case(BF, F32, la, lb, 136, 264, 264, x3=True, split_k=split_k, split="ws")
    run_case(c, what=f"x3 split ({la},{lb}) {split_k}")


@pytest.mark.parametrize("bias,residual,accumulate", [(b, s, a) for b in (0, 1) for s in (0, 1) for a in (0, 1) if b or s or a])
def test_x3_epilogue(bias, residual, accumulate):
    la, lb = LAYOUTS[(bias + 2 * residual + accumulate) % 4]
    c = build_case(BF, F32, la, lb, 264, 136, 200, x3=True, bias=bool(bias), residual=bool(residual), accumulate=bool(accumulate),
                   alpha=(1.0, 0.5)[bias])
    run_case(c, what=f"x3 epilogue b{bias} s{residual} a{accumulate}")


def test_x3_refusals():
    """gemm.hip muse_gemm_x3: host-side answers, nothing is launched"""
    x3 = lambda d, a_lo=1 << 16, b_lo=1 << 16: _lib().muse_gemm_x3(C.byref(d), a_lo, b_lo, None)
    mk = lambda M=136, K=136, **kw: make_desc(4096, 1 << 20, 1 << 22, M, 136, K, dtype=BF, out_dtype=F32, lda=136, ldb=136, ldc=136, **kw)
    assert x3(mk(M=120)) == ERR_UNSUPPORTED
    assert x3(mk(K=56)) == ERR_UNSUPPORTED
    assert x3(mk(batch=2)) == ERR_UNSUPPORTED
    assert x3(mk(act=1)) == ERR_UNSUPPORTED
    assert x3(mk(), a_lo=(1 << 16) + 4) == ERR_ALIGN and x3(mk(), b_lo=(1 << 16) + 4) == ERR_ALIGN
    assert x3(mk(), a_lo=0) == ERR_ALIGN and x3(mk(), a_lo=-8) == ERR_ALIGN and x3(mk(), b_lo=0) == ERR_ALIGN


# =========================================================================================================================================
# 1e. half operands
# =========================================================================================================================================
@pytest.mark.parametrize("M,N,K", [(136, 264, 72), (264, 136, 200)], ids=lambda v: str(v))
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("pers", [0, 1])
def test_half_operands(pers, la, lb, M, N, K):
    """IEEE half holds the 11-bit integers bf16 cannot.  (0, 0) with K > 128 takes the persistent form when MUSE_G256P allows it, every
    other layout and K = 72 the launch-per-tile form"""
    with env(MUSE_GEMM256=None, MUSE_G256P=str(pers), MUSE_G256_BK=None):
        c = build_case(F16, F32, la, lb, M, N, K, wide="ab"[(la + M) & 1], bias=True)
        run_case(c, path=256, what=f"half ({la},{lb}) {M}x{N}x{K}")
        c = build_case(F16, F32, la, lb, M, N, K, wide="ab"[(lb + M) & 1], accumulate=True)
        run_case(c, path=257 if (pers and (la, lb) == (0, 0) and K > 128) else 256, what=f"half ({la},{lb}) {M}x{N}x{K} accumulate")


@pytest.mark.parametrize("scale", [0.25, 8.0])
def test_half_scaled_image(scale):
    """an operand image that carries a power-of-two `_muse_scale`: ops.gemm divides alpha by it, the result is still exact"""
    with env(MUSE_GEMM256=None, MUSE_G256P="1", MUSE_G256_BK=None):
        c = build_case(F16, F32, 0, 0, 136, 136, 200, wide="b", scale=scale)
        d = to_dev(c)
        Cd = fresh(c["C0"])
        launch(c, d, Cd)
        G.check_c(Cd.cpu(), c["C0"], c["idx"], G.expected(c["pre"], F32), f"half scale {scale}")


def test_half_refusals():
    mk = lambda M=136, K=136, **kw: make_desc(4096, 1 << 20, 1 << 22, M, 136, K, dtype=F16, out_dtype=F32, lda=136, ldb=136, ldc=136, **kw)
    with env(MUSE_GEMM256=None, MUSE_G256P="1"):
        assert gemm_tile(mk()) == 256
        for d in (mk(M=120), mk(K=56), mk(act=1)):
            assert gemm_tile(d) == ERR_UNSUPPORTED and gemm_path(d) == ERR_UNSUPPORTED
            assert _lib().muse_gemm(C.byref(d), None) == ERR_UNSUPPORTED        # refused before any launch
        d = mk()
        d.out_dtype = 1
        assert gemm_tile(d) == ERR_UNSUPPORTED


# =========================================================================================================================================
# 1f. grouped dW
# =========================================================================================================================================
GROUP_SIZES = [(256, 256), (264, 520), (520, 256), (256, 264), (512, 256), (264, 264), (256, 520), (272, 256)]      # (N_i, K_i) of dw_i


def group_items(n, dt, T, accumulate_some):
    """n products dw_i [N_i, K_i] = dy_i^T x_i over T tokens: k-major operands inside NaN-guarded storage, dw behind a sentinel tail"""
    items, checks = [], []
    for i in range(n):
        Ni, Ki = GROUP_SIZES[i]
        amax, bmax = (7, 7) if dt == BF else ((1023, 7) if i & 1 else (7, 1023))
        G.assert_exact(T, amax, bmax, extra=1000)
        dy, x = G.ints((Ni, T), amax, 100 + i), G.ints((Ki, T), bmax, 200 + i)       # logical [rows, k]
        a, lda = G.place(dy, 1, dt)
        b, ldb = G.place(x, 1, dt)
        ad, bd = a.to(DEV), b.to(DEV)
        dy_d = ad.view(-1, lda)[:T, :Ni]
        x_d = bd.view(-1, ldb)[:T, :Ki]
        acc = bool(accumulate_some and i % 2 == 0)
        old = G.ints((1, Ni, Ki), 1000, 300 + i) if acc else None
        C0, idx = G.alloc_c(Ni, Ki, F32, Ki, old=old)
        Cd = fresh(C0)
        dw = Cd[:Ni * Ki].view(Ni, Ki)
        items.append((dy_d, x_d, dw, acc, None, None))
        checks.append((Cd, C0, idx, G.expected(G.product(dy, x)[None], F32, old=old), (ad, bd)))
    return items, checks


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "half"])
def test_group_wgrad(monkeypatch, dt, n, split):
    """ops.linear_wgrad_group -> muse_gemm_group + muse_sum_multi.  Tile counts 1, 6, 3, 2, 2, 4, 3, 2: uneven tile_start steps and a
    product of exactly one tile; T = 200 is 4 K-tiles: split 3 cuts 2 + 2 and leaves the third slice of the (uninitialised) workspace
    unwritten.  The per-product path is closed, so only the grouped launch can have produced the result."""
    ops = _ops()

    def closed(*a, **k):
        raise AssertionError("the grouped launch refused the list: muse_gemm_group_ok != 0")
    monkeypatch.setattr(ops, "linear_wgrad", closed)
    monkeypatch.setattr(torch, "empty", nan_empty(torch.empty))
    items, checks = group_items(n, dt, 200, accumulate_some=True)
    ops.linear_wgrad_group(items, split=split)
    torch.cuda.synchronize()
    for i, (Cd, C0, idx, exp, _) in enumerate(checks):
        G.check_c(Cd.cpu(), C0, idx, exp, f"group n={n} split={split} product {i}")


def nan_empty(real_empty):
    """torch.empty that hands out NaN-filled float tensors: a workspace slice that is summed although no block wrote it shows"""
    def f(*a, **k):
        t = real_empty(*a, **k)
        if t.is_floating_point():
            t.fill_(float("nan"))
        return t
    return f


def test_group_refusals():
    """gemm.hip group_fill, host only"""
    from muse._hip import GemmDesc
    ok = lambda ds, split=1: _lib().muse_gemm_group_ok((GemmDesc * len(ds))(*ds) if ds else None, len(ds), split)
    mk = lambda M=256, N=256, K=128, dt=BF, la=1, lb=1, **kw: make_desc(4096, 1 << 20, 1 << 22, M, N, K, dtype=dt, out_dtype=F32, la=la, lb=lb,
                                                                          lda=M, ldb=N, ldc=N, **kw)
    assert ok([mk()]) == 0 and ok([mk()] * 8) == 0
    assert ok([mk()], split=2) == ERR_BAD_ARG                                   # split > 1 with stride 0
    assert ok([mk(split_stride=256 * 256)], split=2) == 0
    assert ok([]) == ERR_BAD_ARG and ok([mk()] * 9) == ERR_BAD_ARG
    assert ok([mk(M=248)]) == ERR_UNSUPPORTED and ok([mk(K=120)]) == ERR_UNSUPPORTED
    assert ok([mk(), mk(dt=F16)]) == ERR_UNSUPPORTED
    assert ok([mk(la=0, M=256)]) == ERR_UNSUPPORTED and ok([mk(lb=0)]) == ERR_UNSUPPORTED
    assert ok([mk(split_stride=256 * 256, accumulate=1)], split=2) == ERR_BAD_ARG


# =========================================================================================================================================
# 1g. slice reducers
# =========================================================================================================================================
def hand_slices(ns, extra, n, stride, seed):
    """ns integer slices of n elements `stride` apart, `extra` NaN slices behind them, NaN in the gaps"""
    ws = torch.full(((ns + extra) * stride + 4,), float("nan"), dtype=F32)
    vals = G.ints((ns, n), 100000, seed)
    for s in range(ns):
        ws[s * stride:s * stride + n] = vals[s].float()
    return ws, vals


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ns,n", [(1, 4), (3, 4100), (15, 8196)])
def test_sum_slices(ns, n, accumulate):
    ws, vals = hand_slices(ns, 2, n, n + 4, ns * 7 + n)
    old = G.ints((1, 1, n), 1000, 5)
    C0, idx = G.alloc_c(1, n, F32, n + 4, old=old)
    Cd, wd = fresh(C0), ws.to(DEV)
    rc = _lib().muse_sum_slices(wd.data_ptr(), Cd.data_ptr(), ns, n, n + 4, accumulate, None)
    assert rc == 0
    torch.cuda.synchronize()
    exp = (vals.double().sum(0) + (old.double().flatten() if accumulate else 0)).float().view(1, 1, n)
    G.check_c(Cd.cpu(), C0, idx, exp, f"sum_slices ns={ns} n={n}")


def test_sum_multi_slice_jobs():
    """three kind-0 jobs of different sizes in one launch (item boundaries at 4096 outputs), NaN slices behind the used ones"""
    jobs, checks, keep = [], [], []
    for j, (ns, n, acc) in enumerate([(2, 4096, 0), (3, 4100, 1), (5, 12, 0)]):
        ws, vals = hand_slices(ns, 1, n, n + 8, 40 + j)
        old = G.ints((1, 1, n), 1000, 50 + j)
        C0, idx = G.alloc_c(1, n, F32, n + 4, old=old)
        Cd, wd = fresh(C0), ws.to(DEV)
        keep.append(wd)
        jobs.append((0, wd, Cd, ns, n, n + 8, acc))
        checks.append((Cd, C0, idx, (vals.double().sum(0) + (old.double().flatten() if acc else 0)).float().view(1, 1, n)))
    _ops().sum_multi(jobs)
    torch.cuda.synchronize()
    for j, (Cd, C0, idx, exp) in enumerate(checks):
        G.check_c(Cd.cpu(), C0, idx, exp, f"sum_multi job {j}")


@pytest.mark.parametrize("odt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("bias,residual", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_sum_slices_epilogue_direct(odt, bias, residual):
    """hand-made slices whose sums pass 256: the bf16 output is ONE rounding of sum + bias + residual (the kernel adds in f32)"""
    rows, cols, ns = 5, 12, 3
    n = rows * cols
    ws, vals = hand_slices(ns, 2, n, n + 4, 77)
    ws = torch.where(ws.isnan(), ws, (ws / 400).round())                 # sums of about +-400: exact, above bf16's integer range
    pre = ws[: (ns) * (n + 4)].view(ns, n + 4)[:, :n].double().sum(0).view(rows, cols)
    b = G.ints((cols,), 50, 78) if bias else None
    r = G.ints((rows, cols), 9 if odt == BF else 1000, 79) if residual else None
    pre = G.pre_activation(pre, 1.0, b, None)
    ldr, ldc = cols + 4, cols + 8
    C0, idx = G.alloc_c(rows, cols, odt, ldc)
    Cd, wd = fresh(C0), ws.to(DEV)
    bd = G.vec(b).to(DEV) if bias else None
    rd = G.residual_storage(r, odt, ldr).to(DEV) if residual else None
    rc = _lib().muse_sum_slices_epilogue(wd.data_ptr(), ns, n + 4, bd.data_ptr() if bias else None, rd.data_ptr() if residual else None, ldr,
                                         Cd.data_ptr(), 1 if odt == BF else 0, ldc, rows, cols, None)
    assert rc == 0
    torch.cuda.synchronize()
    G.check_c(Cd.cpu(), C0, idx, G.expected(pre, odt, r, None, "once")[None], f"sum_slices_epilogue {odt} b{bias} s{residual}")


@pytest.mark.parametrize("odt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K,bias,residual", [(256, 128, 2816, 1, 1), (129, 136, 520, 0, 1), (64, 72, 1032, 1, 0), (17, 132, 512, 0, 0)])
def test_skinny_split_k(monkeypatch, odt, M, N, K, bias, residual):
    """ops.gemm with SKINNY = 2: split-K into an (here NaN-filled) workspace + muse_sum_slices_epilogue.  M = 256, K = 2816: 16 requested
    slices become 15 (44 K-tiles, 3 per slice); a 16th summed slice would be NaN.  bf16 output with a residual: rounded once."""
    ops = _ops()
    monkeypatch.setattr(ops, "SKINNY", 2)
    monkeypatch.setattr(torch, "empty", nan_empty(torch.empty))
    if (M, K) == (256, 2816):
        assert min(256 // 2, K // 128, 16) == 16 and G.used_slices(K, 16) == 15
    with env(MUSE_GEMM256=None, MUSE_G256P=None, MUSE_G256_BK=None):
        c = build_case(BF, odt, 0, 0, M, N, K, bias=bool(bias), residual=bool(residual), ldc=N + 8, ldr=N + 4)
        d = to_dev(c)
        outs = []
        for _ in range(2):
            Cd = fresh(c["C0"])
            launch(c, d, Cd)
            outs.append(Cd.cpu())
    G.check_same_bits(outs[0], outs[1])
    G.check_c(outs[0], c["C0"], c["idx"], G.expected(c["pre"], odt, c["res_v"], None, "once"), f"skinny {M}x{N}x{K} {odt}")


# =========================================================================================================================================
# 1h. callers
# =========================================================================================================================================
def _pair(dt, shape_a, shape_b, seed):
    if dt == BF:
        return G.ints(shape_a, 7, seed), G.ints(shape_b, 7, seed + 1)
    return G.ints(shape_a, 1023, seed), G.ints(shape_b, 7, seed + 1)


@pytest.mark.parametrize("dt", [F32, BF, F16], ids=["f32", "bf16", "half"])
def test_callers_linear_dgrad_wgrad(dt):
    """ops.linear / linear_dgrad / linear_wgrad at one ragged shape per dtype (half: the smallest the half kernels take), the weight-gradient
    plan recomputed"""
    ops = _ops()
    ops._WGRAD_PLAN.clear()
    T, N, K = (129, 72, 200) if dt != F16 else (136, 136, 200)
    with env(MUSE_GEMM256=None, MUSE_G256P=None, MUSE_G256_BK=None):
        x, w = _pair(dt, (T, K), (N, K), 1)
        G.assert_exact(K, 1023, 7)
        y = ops.linear(G.to_dtype_exact(x, dt).to(DEV), G.to_dtype_exact(w, dt).to(DEV), out=torch.empty((T, N), dtype=F32, device=DEV))
        assert torch.equal(y.cpu(), G.expected(G.product(x, w), F32)), "ops.linear"
        dy, w2 = _pair(dt, (T, N), (N, K), 3)
        G.assert_exact(N, 1023, 7)
        dx = ops.linear_dgrad(G.to_dtype_exact(dy, dt).to(DEV), G.to_dtype_exact(w2, dt).to(DEV), out=torch.empty((T, K), dtype=F32, device=DEV))
        assert torch.equal(dx.cpu(), G.expected(dy.double() @ w2.double(), F32)), "ops.linear_dgrad"
        T2 = 520
        dy2, x2 = _pair(dt, (T2, N), (T2, K), 5)
        G.assert_exact(T2, 1023, 7, extra=1000)
        old = G.ints((N, K), 1000, 7)
        for acc in (False, True):
            dw = old.float().to(DEV)
            ops.linear_wgrad(G.to_dtype_exact(dy2, dt).to(DEV), G.to_dtype_exact(x2, dt).to(DEV), dw, acc)
            exp = dy2.double().t() @ x2.double() + (old.double() if acc else 0)
            assert torch.equal(dw.cpu(), G.expected(exp, F32)), f"ops.linear_wgrad accumulate={acc}"
    ops._WGRAD_PLAN.clear()


@pytest.mark.parametrize("la,lb", [(0, 1), (1, 0), (1, 1)])
def test_caller_gemm_via_transpose(monkeypatch, la, lb):
    """MUSE_GEMM_TR=0's route: k-major operands through muse_transpose into zero-padded k-contiguous copies"""
    ops = _ops()
    monkeypatch.setattr(ops, "USE_TR", False)
    with env(**ENV128):
        c = build_case(BF, F32, la, lb, 65, 72, 100, bias=True, batch=2, zdiv=1)
        d = to_dev(c)
        Cd = fresh(c["C0"])
        launch(c, d, Cd)
        G.check_c(Cd.cpu(), c["C0"], c["idx"], G.expected(c["pre"], F32), f"via transpose ({la},{lb})")


@pytest.mark.parametrize("route", ["native", "cat3", "three"])
@pytest.mark.parametrize("la,lb", [(0, 0), (0, 1), (1, 1)])
def test_caller_bf16x3_routes(monkeypatch, route, la, lb):
    """ops._gemm_bf16x3 on integer f32 operands (11-bit against [-7, 7]); the reference is the three-term sum of the CPU's own hi / lo
    split (bf16 RNE, then bf16 of the remainder), without lo x lo"""
    ops = _ops()
    monkeypatch.setattr(ops, "X3_NATIVE", route == "native")
    monkeypatch.setattr(ops, "X3_CAT", route != "three")
    M, N, K = 136, 264, 200
    A, B = G.ints((M, K), 1023, 31), G.ints((N, K), 7, 32)
    (ah, al), (bh, bl) = G.split_hi_lo(A), G.split_hi_lo(B)
    G.assert_exact(K, 1024, 7, terms=3)
    exp = G.expected(G.product_x3(ah.double(), al.double(), bh.double(), bl.double()), F32)
    assert bool((al != 0).any())
    At = (A if la == 0 else A.t()).float().contiguous().to(DEV)
    Bt = (B if lb == 0 else B.t()).float().contiguous().to(DEV)
    C0, idx = G.alloc_c(M, N, F32, N + 4)
    Cd = fresh(C0)
    with env(MUSE_GEMM256=None, MUSE_G256P=None, MUSE_G256_BK=None), ops.f32_gemms_as_bf16x3(True):
        ops.gemm(At, Bt, Cd, M, N, K, la=la, lb=lb, lda=At.stride(0), ldb=Bt.stride(0), ldc=N + 4)
    G.check_c(Cd.cpu(), C0, idx, exp[None], f"bf16x3 {route} ({la},{lb})")


# =========================================================================================================================================
# host-only answers of muse_gemm_tile / muse_gemm_path: no launch, no dereference - aligned fake pointers
# =========================================================================================================================================
PA, PB, PC = 1 << 20, 1 << 24, 1 << 28


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_host_alignment_refusals(dt):
    """every MUSE_ERR_ALIGN condition of gemm.hip fill_params, one at a time"""
    ch = G.CHUNK[dt]
    base = dict(dtype=dt, out_dtype=F32, lda=64, ldb=64, ldc=64)
    with env(**ENV128):
        assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 64, **base)) == 128
        for k in ("lda", "ldb"):
            assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 64, **dict(base, **{k: 64 + ch // 2}))) == ERR_ALIGN, k
        assert gemm_tile(make_desc(PA + 8, PB, PC, 64, 64, 64, **base)) == ERR_ALIGN
        assert gemm_tile(make_desc(PA, PB + 8, PC, 64, 64, 64, **base)) == ERR_ALIGN
        for k in ("sA", "sB"):
            for pos in (0, 1):
                s = [4096, 4096]
                s[pos] += ch // 2
                assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 64, batch=4, zdiv=2, **dict(base, **{k: tuple(s)}))) == ERR_ALIGN, (k, pos)
        assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 64, batch=4, zdiv=2, sA=(4096, 4096 + ch), sB=(ch, 0), **base)) == 128
        assert gemm_tile(make_desc(0, PB, PC, 64, 64, 64, **base)) == ERR_BAD_ARG


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_host_4gib_span(dt, layout, operand):
    """fill_params: a batch slice of ((rows - 1) ld + cols + chunk) * esz >= 2^32 bytes is refused; the last accepted and the first refused
    row count, rows = M / N (layout 0) or K (layout 1)"""
    esz, ch = (2, 8) if dt == BF else (4, 4)
    ld, cols = 1 << 20, 64

    def span(rows):
        return ((rows - 1) * ld + cols + ch) * esz

    last = (1 << 32) // (ld * esz)
    assert span(last) < (1 << 32) <= span(last + 1)
    with env(**ENV128):
        for rows, want in ((last, 128), (last + 1, ERR_UNSUPPORTED)):
            M, N, K = 64, 64, 64
            kw = dict(dtype=dt, out_dtype=F32, lda=64, ldb=64, ldc=64)
            if operand == "A":
                kw.update(la=layout, lda=ld)
                if layout == 0:
                    M = rows
                else:
                    K = rows
            else:
                kw.update(lb=layout, ldb=ld)
                if layout == 0:
                    N = rows
                else:
                    K = rows
            # the other operand is k-contiguous [64, K]: when K is the long dimension give it a row stride that fits K but stays below 4 GiB
            other = "ldb" if operand == "A" else "lda"
            kw[other] = G.rup(K, ch)
            assert gemm_tile(make_desc(PA, PB, PC, M, N, K, **kw)) == want, (rows, want)


def test_host_split_k_excludes_epilogue():
    base = dict(dtype=BF, out_dtype=F32, lda=256, ldb=256, ldc=64, split_k=2, split_stride=64 * 64)
    with env(**ENV128):
        assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 256, **base)) == 128
        assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 256, **dict(base, split_stride=0))) == 128          # atomic slices
        for extra in (dict(bias=PC), dict(rowvec=PC), dict(residual=PC, ldr=64), dict(act=1), dict(out_dtype=BF)):
            assert gemm_tile(make_desc(PA, PB, PC, 64, 64, 256, **dict(base, **extra))) == ERR_BAD_ARG, extra
            assert gemm_path(make_desc(PA, PB, PC, 64, 64, 256, **dict(base, **extra))) == ERR_BAD_ARG, extra


def test_host_default_mode_floor():
    """gemm256_preferred with MUSE_GEMM256 unset: K < 128, M < 256 or N < 256 never take the 256^2 kernels, whatever the cost estimate"""
    mk = lambda M=4096, N=4096, K=1024: make_desc(PA, PB, PC, M, N, K, dtype=BF, out_dtype=BF, lda=K, ldb=K, ldc=N)
    with env(MUSE_GEMM256=None, MUSE_G256P=None):
        assert gemm_tile(mk()) == 256 and gemm_path(mk()) == 257
        assert gemm_tile(mk(K=120)) == 128 and gemm_tile(mk(M=248)) == 128 and gemm_tile(mk(N=248)) == 128
        assert gemm_path(mk(K=120)) == 128 and gemm_path(mk(M=248)) == 128 and gemm_path(mk(N=248)) == 128
    with env(MUSE_GEMM256=None, MUSE_G256P="0"):
        assert gemm_path(mk()) in (128, 256)          # (without the persistent form the estimate decides; either answer is a tile kernel)


# =========================================================================================================================================
# 2. the rounding leg: seeded N(0, 1) operands, K ~ 700, judged per element against float64 with a derived bound
# =========================================================================================================================================
RATIOS = {}


def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _rounding_case(name):
    ops = _ops()
    M, N, K = 264, 136, 696
    A64, B64 = normal((M, K), 1), normal((N, K), 2)
    extra, ctx, odt, envv, path = 0.0, contextlib.nullcontext(), F32, ENV128, 128
    if name == "128-f32":
        A, B = A64.float(), B64.float()
        M, N = 129, 72
        A, B = A[:M].contiguous(), B[:N].contiguous()
    elif name.split("+")[0] in ("128-bf16", "256", "persistent"):
        A, B = A64.to(BF), B64.to(BF)
        odt = F32 if name.endswith("+f32out") else BF          # (f32 output: the accumulation error alone, no output rounding on top)
        name0 = name.split("+")[0]
        envv, path = {"128-bf16": (ENV128, 128), "256": (ENV256, 256), "persistent": (ENVP, 257)}[name0]
        if name0 == "128-bf16":
            M, N = 129, 72
            A, B = A[:M].contiguous(), B[:N].contiguous()
    elif name == "x3":
        A, B = A64.float(), B64.float()
        extra, ctx, envv, path = 2.0 ** -16, ops.f32_gemms_as_bf16x3(True), dict(MUSE_GEMM256=None, MUSE_G256P=None, MUSE_G256_BK=None), None
    else:
        assert name == "half"
        A, B = A64.float(), B64.float()
        extra, ctx, envv, path = 2.0 ** -10, ops.f32_gemms_as_f16(True), dict(MUSE_GEMM256=None, MUSE_G256P=None, MUSE_G256_BK=None), None
    ref = A.double() @ B.double().t()                    # the operands as the kernel receives them (x3 / half: the f32 tensors)
    terms = G.abs_terms(A, B)
    bound = G.rounding_bound(K, terms, ref, out_bf16=odt == BF, extra=extra)
    Ad, Bd = A.to(DEV), B.to(DEV)
    Cd = torch.full((M, N), float("nan"), dtype=odt, device=DEV)
    with env(**envv), ctx:
        if path is not None:
            assert gemm_path(make_desc(Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), M, N, K, dtype=A.dtype, out_dtype=odt, lda=K, ldb=K, ldc=N)) == path
        ops.gemm(Ad, Bd, Cd, M, N, K, lda=K, ldb=K, ldc=N)
    ratio = G.worst_ratio(Cd.cpu(), ref, bound)
    RATIOS[name] = ratio
    print(f"rounding leg {name}: worst error / bound = {ratio:.4f}  ({M}x{N}x{K})")
    return ratio


@pytest.mark.parametrize("name", ["128-f32", "128-bf16", "256", "persistent", "128-bf16+f32out", "256+f32out", "persistent+f32out", "x3", "half"])
def test_rounding_leg(name):
    """bound per element: (K + 2) 2^-23 sum|a b| (a truncating f32 accumulator in any order), + 2^-8 |ref| for a bf16 output,
    + 2^-16 sum|a b| for bf16x3 (dropped lo x lo, lo-plane rounding), + 2^-10 sum|a b| for the two half roundings of the f16 mode"""
    assert _rounding_case(name) <= 1.0


GELU_SHAPE = (129, 136, 200)


def gelu_bound(c):
    pre = c["pre"]
    e_ref = G.gelu_e_ref(pre)
    ref = G.gelu64(pre)
    bound = torch.full_like(ref, 4.0 * e_ref)
    if c["odt"] == BF:
        bound = bound + 2.0 ** -8 * (ref.abs() + 4.0 * e_ref)
    return e_ref, ref, bound


@pytest.mark.parametrize("odt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [136, 131], ids=["fast", "direct"])
def test_gelu_epilogue(odt, N):
    """act = 1 on both 128^2 epilogues: the pre-activation is exact, the result is judged per element against float64 gelu with
    4 x E_ref (+ one bf16 rounding), E_ref = the error of torch's own f32 CPU gelu on the same pre-activations"""
    M, _, K = GELU_SHAPE
    with env(**ENV128):
        c = build_case(BF, odt, 0, 1, M, N, K, alpha=2.0 ** -6, bias=True, bias_lim=2)
        e_ref, ref, bound = gelu_bound(c)
        d = to_dev(c)
        Cd = fresh(c["C0"])
        assert gemm_path(case_desc(c, d, Cd, act=1)) == 128
        launch(c, d, Cd, act=1)
        out = Cd.cpu()
    got = out[c["idx"].flatten()].view(ref.shape)
    err = (got.double() - ref).abs()
    print(f"gelu epilogue {odt} N={N}: E_ref {e_ref:.3e}, bound(f32 part) {4 * e_ref:.3e}, worst error {float(err.max()):.3e}, "
          f"worst error / bound {float((err / bound).max()):.3f}")
    assert not bool(got.isnan().any()) and bool((err <= bound).all())
    keep = torch.ones(out.numel(), dtype=torch.bool)
    keep[c["idx"].flatten()] = False
    assert torch.equal(G.bits(out)[keep], G.bits(c["C0"])[keep]), "C padding written"


if __name__ == "__main__":       # on a CPU: reprint E_ref of the GELU cases
    for odt in (F32, BF):
        for N in (136, 131):
            M, _, K = GELU_SHAPE
            c = build_case(BF, odt, 0, 1, M, N, K, alpha=2.0 ** -6, bias=True, bias_lim=2)
            e_ref, ref, bound = gelu_bound(c)
            print(f"gelu {odt} N={N}: E_ref = {e_ref:.3e}, bound = 4 E_ref = {4 * e_ref:.3e} (+ 2^-8 |ref| for bf16), "
                  f"max |pre| = {float(c['pre'].abs().max()):.2f}")
