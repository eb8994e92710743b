"""CPU side of the GEMM edge tests (tests/test_gpu_gemm_edges.py, tests/test_gemm_cpu.py): integer probes, the exact reference, the
storage builders with their NaN / sentinel guards, the check functions, and a plain tiled contract model of the GEMM kernels' bookkeeping
with switchable defects.

Why integers: with |a|, |b| integers and K max|a| max|b| < 2^24 every product and every partial sum is an integer that f32 holds exactly,
so the f32 result does not depend on the accumulation order, the tile shape, the K split or the pipeline depth - every path must return
the reference bit for bit, and a bf16 output must be the bf16 rounding of it.  `assert_exact` guards that bound for every case.

Storage contract of an operand (include/muse_hip.h, PlainLoader of csrc/gemm_core.h, Dma<L, BK> of csrc/gemm256.h): the loaders fetch
16-byte chunks along the contiguous dimension and mask a chunk by its FIRST element, so they may read
  k-contiguous X(r, k) at r * ld + k:  rows r < R, columns k < roundup(K, chunk) - the columns K .. roundup(K, chunk) must hold zeros;
  k-major      X(r, k) at k * ld + r:  rows k < K exactly, columns r < roundup(R, chunk) - those extra columns only feed output rows /
                                       columns past M / N, which are never stored; `place` keeps them zero all the same.
Everything else - rows past the matrix, columns past the chunk-rounded extent up to ld, the bytes before the operand's offset and behind its
last row - is filled with NaN by `place`: one element read from there turns a whole output row or column into NaN.
"""
import math

import torch

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CHUNK = {BF: 8, F16: 8, F32: 4}                      # elements per 16-byte chunk
_INT = {BF: torch.int16, F16: torch.int16, F32: torch.int32, torch.float64: torch.int64}
SENTINEL = {BF: 0x7FC1, F32: 0x7FC0DEAD}             # quiet NaNs with a payload: no GEMM result has these bits
LIMIT = 1 << 24


def rup(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


def bits(t):
    return t.contiguous().view(_INT[t.dtype])


def ints(shape, lim, seed):
    """seeded integers in [-lim, lim], int64"""
    g = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFF)
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g, dtype=torch.int64)


def assert_exact(K, amax, bmax, terms=1, extra=0):
    """every partial sum of the probe stays an integer below 2^24 (terms: products summed per k - 3 for bf16x3; extra: |epilogue addends|)"""
    assert terms * K * amax * bmax + extra < LIMIT, (K, amax, bmax, terms, extra)


def to_dtype_exact(x, dtype):
    y = x.to(dtype)
    assert torch.equal(y.double(), x.double()), f"probe values are not exact in {dtype}"
    return y


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def product(A, B):
    """A [.., M, K], B [.., N, K] integers -> exact A B^T in float64"""
    return A.double() @ B.double().transpose(-1, -2)


def product_x3(Ah, Al, Bh, Bl):
    """the three-term bf16x3 sum hi hi + hi lo + lo hi - no lo lo term"""
    return product(Ah, Bh) + product(Ah, Bl) + product(Al, Bh)


def pre_activation(acc, alpha=1.0, bias=None, rowvec=None):
    pre = alpha * acc
    if rowvec is not None:
        pre = pre + rowvec.double()[..., :, None]
    if bias is not None:
        pre = pre + bias.double()[..., None, :]
    return pre


def _f32_exact(x):
    y = x.float()
    assert torch.equal(y.double(), x), "the reference is not exact in f32: the probe is too large"
    assert float(x.abs().max()) < LIMIT
    return y


def expected(pre, out_dtype, residual=None, old=None, rounding="once"):
    """the output the contract asks for.  f32: exact.  bf16: round-to-nearest-even of the exact value - with a residual / an old C
    either ONCE (add in f32, then round) or TWICE (round the product to bf16, add in f32, round again), as DESIGN.md lists per path."""
    add = torch.zeros_like(pre)
    for t in (residual, old):
        if t is not None:
            add = add + t.double()
    if out_dtype == F32:
        return _f32_exact(pre + add)
    assert out_dtype == BF
    if rounding == "once":
        return _f32_exact(pre + add).to(BF)
    assert rounding == "twice"
    staged = _f32_exact(pre).to(BF)
    return _f32_exact(staged.double() + add).to(BF)


def split_hi_lo(x):
    """the CPU's own bf16x3 split of f32 values: hi = bf16(x) (RNE), lo = bf16(x - hi)"""
    x = x.float()
    hi = x.to(BF)
    lo = (x - hi.float()).to(BF)
    return hi, lo


# ---- storage ---------------------------------------------------------------------------------------------------------------------------
def place(X, layout, dtype, pad=1, extra_rows=2, lead=0, ld=None):
    """integer matrix X [R, K] -> (flat storage, ld): the operand at element offset `lead`, zeros where the loaders may read beyond the
    matrix, NaN everywhere else (see the module docstring).  pad: chunks of NaN columns between the chunk-rounded extent and ld."""
    R, K = X.shape
    ch = CHUNK[dtype]
    rows, cols = (R, K) if layout == 0 else (K, R)
    cr = rup(cols, ch)
    ld = cr + pad * ch if ld is None else ld
    assert ld % ch == 0 and ld >= cr and lead % ch == 0
    st = torch.full((lead + (rows + extra_rows) * ld,), float("nan"), dtype=dtype)
    body = st[lead:].view(rows + extra_rows, ld)
    body[:rows, :cr] = 0
    body[:rows, :cols] = to_dtype_exact(X if layout == 0 else X.t(), dtype)
    return st, ld


def place_batched(Xz, layout, dtype, zdiv, pad=1, lead=0):
    """Xz [Z, R, K] -> (flat, ld, (s0, s1)): slice z at (z // zdiv) * s0 + (z % zdiv) * s1, s0 != zdiv * s1 (a NaN gap between groups)"""
    Z = Xz.shape[0]
    parts = [place(Xz[z], layout, dtype, pad=pad, lead=0) for z in range(Z)]
    ld, S = parts[0][1], parts[0][0].numel()
    ch = CHUNK[dtype]
    s1, s0 = S, zdiv * S + 2 * ch
    total = lead + (cdiv(Z, zdiv) - 1) * s0 + zdiv * s1
    flat = torch.full((total,), float("nan"), dtype=dtype)
    for z in range(Z):
        o = lead + (z // zdiv) * s0 + (z % zdiv) * s1
        flat[o:o + S] = parts[z][0]
    return flat, ld, (s0, s1)


def vec(x, dtype=F32, tail=4):
    """a bias / row vector with a NaN tail behind its last element"""
    st = torch.full((x.numel() + tail,), float("nan"), dtype=dtype)
    st[:x.numel()] = to_dtype_exact(x, dtype)
    return st


def sentinel(n, dtype):
    return torch.full((n,), SENTINEL[dtype], dtype=_INT[dtype]).view(dtype)


def c_index(M, N, ldc, c_off=0, batch=1, zdiv=1, sC=(0, 0)):
    """flat element indices of C[z, m, n] -> int64 [batch, M, N]"""
    z = torch.arange(batch)
    base = c_off + (z // zdiv) * sC[0] + (z % zdiv) * sC[1]
    return base[:, None, None] + torch.arange(M)[None, :, None] * ldc + torch.arange(N)[None, None, :]


def alloc_c(M, N, dtype, ldc, c_off=0, extra_rows=2, batch=1, zdiv=1, sC=(0, 0), old=None):
    """flat C storage: the sentinel everywhere (ldc - N pad columns, extra rows, the bytes before c_off), `old` [batch, M, N] in place"""
    idx = c_index(M, N, ldc, c_off, batch, zdiv, sC)
    span = int(idx.max()) + 1 + (ldc - N) + extra_rows * ldc
    flat = sentinel(rup(span, 8) + 8, dtype)
    if old is not None:
        flat[idx.flatten()] = to_dtype_exact(old, dtype).flatten()
    return flat, idx


def residual_storage(res, dtype, ldr, r_off=0, extra_rows=1):
    """flat residual [M, ldr] at element offset r_off, NaN outside the M x N values"""
    M, N = res.shape
    st = torch.full((r_off + (M + extra_rows) * ldr + 8,), float("nan"), dtype=dtype)
    idx = r_off + torch.arange(M)[:, None] * ldr + torch.arange(N)[None, :]
    st[idx.flatten()] = to_dtype_exact(res, dtype).flatten()
    return st


# ---- checks (shared by the GPU tests and the CPU proof that they bite) -------------------------------------------------------------------
def check_c(out_flat, init_flat, idx, exp, what=""):
    """the M x N region of every batch equals `exp` (values; no NaN can pass), every other element still has its initial bits"""
    out_flat, init_flat = out_flat.cpu(), init_flat.cpu()
    assert out_flat.dtype == exp.dtype == init_flat.dtype, (out_flat.dtype, exp.dtype)
    got = out_flat[idx.flatten()].view(exp.shape)
    if not torch.equal(got, exp):
        bad = (got != exp) | got.isnan()
        where = bad.nonzero()
        first = tuple(int(v) for v in where[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {exp.numel()} elements differ from the exact reference; first at {first}: "
                             f"got {float(got[first])}, want {float(exp[first])}; rows {sorted(set(where[:, -2].tolist()))[:6]} "
                             f"cols {sorted(set(where[:, -1].tolist()))[:6]}")
    keep = torch.ones(out_flat.numel(), dtype=torch.bool)
    keep[idx.flatten()] = False
    ob, ib = bits(out_flat)[keep], bits(init_flat)[keep]
    if not torch.equal(ob, ib):
        pos = keep.nonzero().flatten()[(ob != ib).nonzero().flatten()]
        raise AssertionError(f"{what}: {int((ob != ib).sum())} elements of C's padding were written; first flat offsets {pos[:8].tolist()}")


def check_same_bits(a, b, what=""):
    assert torch.equal(bits(a.cpu()), bits(b.cpu())), f"{what}: a second launch of the same case is not bit-identical"


def used_slices(K, split_k, bk=64):
    """the slices a split-K launch really writes: the kernels cut per = ceil(nk / split_k) K-tiles per slice, a slice that starts at or
    beyond nk returns without storing (gemm_kernel of csrc/gemm_core.h, tile_body of csrc/gemm256.h)"""
    nk = cdiv(K, bk)
    return cdiv(nk, cdiv(nk, split_k))


def check_workspace(ws, split_k, used, exp, what=""):
    """ws [split_k, M, N] f32, NaN-filled before the launch: exactly the first `used` slices are written, they sum to the exact reference"""
    ws = ws.cpu()
    assert 1 <= used <= split_k
    for s in range(split_k):
        nan = ws[s].isnan()
        if s < used:
            assert not bool(nan.any()), f"{what}: slice {s} of {used} used slices still holds {int(nan.sum())} NaN: not (fully) written"
        else:
            assert bool(nan.all()), f"{what}: slice {s} lies beyond the {used} slices the kernel cuts and was written"
    total = ws[:used].double().sum(0)
    assert torch.equal(total, exp.double()), f"{what}: the {used} written slices do not sum to the exact reference " \
                                             f"({int((total != exp.double()).sum())} elements differ)"


def once_twice_share(pre, residual=None, old=None):
    """share of elements on which the once- and the twice-rounded bf16 result differ"""
    a, b = expected(pre, BF, residual, old, "once"), expected(pre, BF, residual, old, "twice")
    return float((a != b).float().mean())


# ---- per-element bounds of the rounding leg ------------------------------------------------------------------------------------------------
def abs_terms(A, B):
    """sum_k |a_k b_k| per output element, float64"""
    return A.double().abs() @ B.double().abs().transpose(-1, -2)


def rounding_bound(K, terms, ref, out_bf16=False, extra=0.0):
    """(K + 2) 2^-23 sum|a b| (an f32 accumulator that may truncate, in any order) + extra * sum|a b| (the path's operand roundings)
    + one bf16 rounding of the result for bf16 outputs"""
    b = ((K + 2) * 2.0 ** -23 + extra) * terms
    if out_bf16:
        b = b + 2.0 ** -8 * (ref.abs() + b)
    return b


def worst_ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    assert not bool(got.double().isnan().any())
    return float((err / bound.clamp_min(1e-300)).max())


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_e_ref(pre):
    """E_ref: the worst error of torch's own f32 CPU gelu against float64 on the same (exact) pre-activations"""
    return float((torch.nn.functional.gelu(pre.float()).double() - gelu64(pre)).abs().max())


# ---- the contract model: a plain tiled GEMM that keeps the kernels' bookkeeping ----------------------------------------------------------
DEFECTS = ("drop_last_k_chunk", "leak_pad_column", "n_mask_off_by_one", "skip_last_row_tile", "one_slice_more", "tile_start_off_by_one",
           "lo_planes_swapped", "lo_lo_included", "round_twice")


def _load_tile(st, layout, ld, R, K, kend, r0, k0, BR, BK, ch, defect):
    """one BR x BK operand tile as the loaders see it: a chunk is fetched when its first element lies inside the matrix (row < R, k < kend),
    an offset beyond the buffer descriptor's range ((rows - 1) * ld + roundup(cols, chunk)) reads zero"""
    r = r0 + torch.arange(BR)[:, None]
    k = k0 + torch.arange(BK)[None, :]
    klim = kend
    if defect == "drop_last_k_chunk":
        klim = kend - ch                                  # the k mask one chunk short
    if layout == 0:
        kfirst = (k - k0) // ch * ch + k0
        ok = (r < R) & (kfirst < klim)
        if defect == "leak_pad_column":
            ok = (r < R) & (k < rup(kend, BK))            # the mask at tile granularity: pad columns up to ld come in
        idx = r * ld + k
        size = (R - 1) * ld + rup(K, ch)
        if defect == "leak_pad_column":
            size = R * ld
    else:
        rfirst = (r - r0) // ch * ch + r0
        ok = (rfirst < R) & (k < klim)
        if defect == "leak_pad_column":
            ok = (rfirst < R) & (k < rup(kend, BK))       # k rows past K come in
        idx = k * ld + r
        size = (K - 1) * ld + rup(R, ch)
        if defect == "leak_pad_column":
            size = st.numel()
    ok = ok & (idx < size) & (idx < st.numel())
    vals = st[idx.clamp(max=st.numel() - 1)].double()
    return torch.where(ok, vals, torch.zeros((), dtype=torch.float64))


def model_tile(p, tid, y, defect=None):
    """one output tile (or one K slice of it) of the product described by dict p, written into p['C'] (flat, typed).  Keys: A, B (flat
    storage), C, dtype, out_dtype, la, lb, M, N, K, lda, ldb, ldc, and optionally a_off, b_off, c_off, alpha, bias, rowvec, residual,
    ldr, r_off, accumulate, split_k, split_stride, BM, BN, BK, GM, two_stage, rounding, a_lo, b_lo (bf16x3 planes)."""
    g = p.get
    M, N, K, BM, BN, BK = p["M"], p["N"], p["K"], g("BM", 128), g("BN", 128), g("BK", 64)
    ch = CHUNK[p["dtype"]]
    ntm, ntn = cdiv(M, BM), cdiv(N, BN)
    GM = g("GM", 1024 // BM)
    grp, first_m = tid // (GM * ntn), tid // (GM * ntn) * GM             # grouped raster: GM row tiles x all column tiles, M fastest
    gm = min(ntm - first_m, GM)
    in_grp = tid - grp * (GM * ntn)
    m0, n0 = (first_m + in_grp % gm) * BM, (in_grp // gm) * BN
    split_k, stride = g("split_k", 1), g("split_stride", 0)
    nk, kt0 = cdiv(K, BK), 0
    if split_k > 1:
        per = cdiv(nk, split_k)                                          # the slice cut
        kt0 = y * per
        nk = min(nk, kt0 + per)
        if kt0 >= nk:
            return                                                       # an empty slice stores nothing
    kend = min(K, nk * BK)
    last = kt0 + rup(nk - kt0, 2) if g("two_stage", False) else nk       # even round-up of the K-tile count: the extra tile is all masked
    A, B = p["A"][g("a_off", 0):], p["B"][g("b_off", 0):]
    acc = torch.zeros((BM, BN), dtype=torch.float64)
    for kt in range(kt0, last):
        ld_ = lambda st, lay, ld, R, r0, BR: _load_tile(st, lay, ld, R, K, kend, r0, kt * BK, BR, BK, ch, defect)
        a = ld_(A, p["la"], p["lda"], M, m0, BM)
        b = ld_(B, p["lb"], p["ldb"], N, n0, BN)
        if g("a_lo") is None:
            acc += a @ b.t()
        else:
            al = ld_(A[p["a_lo"]:], p["la"], p["lda"], M, m0, BM)
            bl = ld_(B[p["b_lo"]:], p["lb"], p["ldb"], N, n0, BN)
            if defect == "lo_planes_swapped":
                b, bl = bl, b
            acc += a @ bl.t() + al @ b.t() + a @ b.t()
            if defect == "lo_lo_included":
                acc += al @ bl.t()
    m = m0 + torch.arange(BM)
    n = n0 + torch.arange(BN)
    nlim = N + 1 if defect == "n_mask_off_by_one" else N
    mm, nn = m[m < M], n[n < nlim]
    if mm.numel() == 0 or nn.numel() == 0:
        return
    acc = acc[:mm.numel(), :nn.numel()]
    pre = g("alpha", 1.0) * acc
    if g("rowvec") is not None:
        pre = pre + p["rowvec"][mm].double()[:, None]
    if g("bias") is not None:
        pre = pre + p["bias"][nn.clamp(max=N - 1)].double()[None, :]
    C = p["C"]
    cidx = (g("c_off", 0) + (y * stride if split_k > 1 else 0) + mm[:, None] * p["ldc"] + nn[None, :]).flatten()
    add = torch.zeros_like(pre)
    if g("residual") is not None:
        add = add + p["residual"][(g("r_off", 0) + mm[:, None] * p["ldr"] + nn[None, :]).flatten()].double().view(pre.shape)
    if g("accumulate") or (split_k > 1 and stride == 0):                 # atomic slices add onto the preset C
        add = add + C[cidx].double().view(pre.shape)
    rounding = g("rounding", "once")
    if defect == "round_twice":
        rounding = "twice"
    if p["out_dtype"] == BF and rounding == "twice":
        pre = pre.float().to(BF).double()
    C[cidx] = (pre + add).float().to(p["out_dtype"]).flatten()


def model_gemm(p, defect=None):
    ntm, ntn = cdiv(p["M"], p.get("BM", 128)), cdiv(p["N"], p.get("BN", 128))
    BM = p.get("BM", 128)
    for y in range(max(1, p.get("split_k", 1))):
        for tid in range(ntm * ntn):
            if defect == "skip_last_row_tile" and ntm > 1:
                GM = p.get("GM", 1024 // BM)                              # (the raster decides which tile ids form the last row tile)
                grp = tid // (GM * ntn)
                gm = min(ntm - grp * GM, GM)
                if grp * GM + (tid - grp * GM * ntn) % gm == ntm - 1:
                    continue
            model_tile(p, tid, y, defect)
    return p["C"]


def model_group(ps, split_k, defect=None):
    """the grouped launch: the concatenated tile lists of the products, each global tile looked up in tile_start (kernel_group)"""
    start = [0]
    for p in ps:
        start.append(start[-1] + cdiv(p["M"], 256) * cdiv(p["N"], 256))
    for y in range(split_k):
        for gt in range(start[-1]):
            if defect == "tile_start_off_by_one":
                pi = sum(1 for k in range(1, len(ps)) if gt > start[k])
            else:
                pi = sum(1 for k in range(1, len(ps)) if gt >= start[k])
            p = dict(ps[pi], BM=256, BN=256, GM=4, two_stage=True, split_k=split_k)
            tid = gt - start[pi]
            if tid >= cdiv(p["M"], 256) * cdiv(p["N"], 256):
                continue                                                 # (a tile index past the product: rows beyond M, nothing stored)
            model_tile(p, tid, y, defect)


def model_sum_slices(ws, out, nslices, n, stride, accumulate, defect=None):
    """out[i] (+)= sum over the first nslices slices of ws (flat f32, `stride` apart)"""
    ns = nslices + 1 if defect == "one_slice_more" else nslices
    tot = out[:n].double() if accumulate else torch.zeros(n, dtype=torch.float64)
    for s in range(ns):
        tot = tot + ws[s * stride:s * stride + n].double()
    out[:n] = tot.float()
    return out
