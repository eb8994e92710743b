"""CPU: the proof that the assertions of tests/test_gpu_gemm_edges.py can fail.  tests/gemm_cpu.py's tiled contract model - the tile
raster, the chunk-granular M / N / K masks, the even round-up of the K-tile count, the slice cut and the used-slice count, the group
tile_start search, the once- or twice-rounded bf16 epilogue - passes the very check functions the GPU tests apply, on the very cases they
build, and each of nine seeded defects fails them.  Also here: the slice counts the callers sum are fixed points of the kernels' cut."""
import pytest
import torch

import gemm_cpu as G
import test_gpu_gemm_edges as T
from gemm_cpu import BF, F16, F32

KERNEL = {128: dict(BM=128, BN=128, GM=8), 256: dict(BM=256, BN=256, GM=4, two_stage=True)}


def model_run(c, tile=128, two_stage=None, rounding="once", defect=None):
    """run the contract model on a case of the GPU file (build_case) -> flat C as the GPU would leave it"""
    Cf = c["C0"].clone()
    kern = dict(KERNEL[tile])
    if two_stage is not None:
        kern["two_stage"] = two_stage
    for z in range(c["batch"]):
        zq, zr = divmod(z, c["zdiv"])
        p = dict(A=c["A"], B=c["B"], C=Cf, dtype=c["dt"], out_dtype=c["odt"], la=c["la"], lb=c["lb"], M=c["M"], N=c["N"], K=c["K"],
                 lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], a_off=c["a_off"] + zq * c["sA"][0] + zr * c["sA"][1],
                 b_off=zq * c["sB"][0] + zr * c["sB"][1], c_off=c["c_off"] + zq * c["sC"][0] + zr * c["sC"][1], alpha=c["alpha"],
                 bias=c["bias"], rowvec=c["rowvec"], residual=c["R"], ldr=c["ldr"], r_off=c["r_off"], accumulate=c["accumulate"],
                 split_k=c["split_k"], split_stride=c["split_stride"], rounding=rounding, **kern)
        if c["x3"]:
            p["a_lo"], p["b_lo"] = c["x3_lo"]
        G.model_gemm(p, defect)
    return Cf


def judge(c, out, rounding="once"):
    """exactly what run_case asserts about a launch's result"""
    if c["split"] == "ws":
        M, N, sk = c["M"], c["N"], c["split_k"]
        G.check_workspace(out[:sk * M * N].view(sk, M, N), sk, G.used_slices(c["K"], sk), G.expected(c["pre"][0], F32))
        assert bool(out[sk * M * N:].isnan().all())
        return
    G.check_c(out, c["C0"], c["idx"], G.expected(c["pre"], c["odt"], c["res_v"], c["old_v"], rounding))


CLEAN = [
    # tile, two_stage, rounding, build_case arguments
    (128, False, "once", (F32, F32, 0, 0, 129, 131, 200), dict(wide="b", bias=True, rowvec=True, alpha=0.5)),
    (128, True, "once", (BF, F32, 1, 1, 257, 17, 129), dict(accumulate=True)),
    (128, True, "twice", (BF, BF, 0, 1, 129, 136, 200), dict(residual=True, accumulate=True)),
    (128, True, "once", (BF, BF, 1, 0, 129, 131, 200), dict(residual=True, accumulate=True)),
    (128, False, "once", (F32, F32, 1, 0, 65, 72, 72), dict(batch=6, zdiv=3, bias=True, accumulate=True, lead=4)),
    (128, True, "once", (BF, F32, 0, 1, 129, 72, 200), dict(split_k=3, split="atomic", alpha=0.5)),
    (128, True, "once", (BF, F32, 1, 1, 129, 72, 520), dict(split_k=7, split="ws")),
    (256, True, "twice", (BF, BF, 0, 0, 264, 264, 200), dict(bias=True, residual=True)),
    (256, True, "once", (BF, F32, 1, 1, 520, 264, 136), dict(rowvec=True)),
    (256, True, "once", (BF, F32, 0, 1, 264, 72, 264), dict(split_k=3, split="ws")),
    (256, True, "once", (BF, F32, 1, 0, 136, 264, 72), dict(x3=True, accumulate=True)),
    (256, True, "once", (F16, F32, 0, 0, 136, 264, 72), dict(wide="b", bias=True)),
]


@pytest.mark.parametrize("tile,two_stage,rounding,args,kw", CLEAN, ids=[str(i) for i in range(len(CLEAN))])
def test_clean_model_passes_the_gpu_checks(tile, two_stage, rounding, args, kw):
    c = T.build_case(*args, **kw)
    judge(c, model_run(c, tile, two_stage, rounding), rounding)


def test_contract_rounding_distinguishes():
    """the bf16 residual probe: the once- and the twice-rounded references differ on a known share of the elements, so asserting one of
    them bit-exactly tells the two epilogues apart"""
    c = T.build_case(BF, BF, 0, 0, 129, 136, 200, residual=True, accumulate=True)
    share = G.once_twice_share(c["pre"], c["res_v"], c["old_v"])
    assert 0.05 < share < 0.95, share
    once = model_run(c, 128, False, "once")
    with pytest.raises(AssertionError):
        judge(c, once, "twice")
    judge(c, once, "once")


# defect -> (tile, build_case arguments, keyword arguments): a case of the GPU file on which the defect must show
DEFECT_CASES = {
    "drop_last_k_chunk": [(128, (BF, F32, 0, 0, 17, 129, 200), {}), (128, (F32, F32, 1, 1, 17, 129, 65), {}), (256, (BF, BF, 0, 1, 264, 8, 72), {})],
    "leak_pad_column": [(128, (BF, F32, 0, 0, 17, 129, 200), {}), (128, (F32, F32, 0, 1, 129, 15, 200), {}), (256, (BF, F32, 1, 1, 264, 264, 136), {})],
    "n_mask_off_by_one": [(128, (BF, BF, 0, 0, 129, 131, 200), {}), (128, (F32, F32, 0, 0, 129, 136, 72), {})],
    "skip_last_row_tile": [(128, (BF, F32, 0, 0, 129, 136, 72), {}), (256, (BF, BF, 0, 0, 520, 264, 136), {}), (128, (BF, F32, 0, 0, 257, 257, 200), {})],
    "lo_planes_swapped": [(256, (BF, F32, 0, 0, 136, 136, 136), dict(x3=True))],
    "lo_lo_included": [(256, (BF, F32, 1, 1, 136, 264, 64), dict(x3=True))],
    "round_twice": [(128, (BF, BF, 0, 0, 129, 131, 200), dict(residual=True, accumulate=True))],
}


@pytest.mark.parametrize("defect", list(DEFECT_CASES))
def test_each_kernel_defect_fails_the_gpu_checks(defect):
    for tile, args, kw in DEFECT_CASES[defect]:
        c = T.build_case(*args, **kw)
        judge(c, model_run(c, tile), "once")                         # the clean model passes ...
        with pytest.raises(AssertionError):                          # ... the seeded one does not
            judge(c, model_run(c, tile, defect=defect), "once")


def test_one_slice_too_many_fails():
    """a reducer that sums one slice more than the kernel wrote adds the NaN of the untouched workspace: muse_sum_slices' check"""
    ns, n = 3, 4100
    ws, vals = T.hand_slices(ns, 2, n, n + 4, 9)
    C0, idx = G.alloc_c(1, n, F32, n + 4)
    exp = vals.double().sum(0).float().view(1, 1, n)
    G.check_c(G.model_sum_slices(ws, C0.clone(), ns, n, n + 4, False), C0, idx, exp)
    with pytest.raises(AssertionError):
        G.check_c(G.model_sum_slices(ws, C0.clone(), ns, n, n + 4, False, defect="one_slice_more"), C0, idx, exp)
    # and through the split-K workspace rule: K = 200 is 4 K-tiles, split 3 cuts 2 + 2 - the third slice stays NaN
    c = T.build_case(BF, F32, 1, 1, 129, 72, 200, split_k=3, split="ws")
    out = model_run(c, 128, True)
    judge(c, out)
    assert G.used_slices(200, 3) == 2
    tot = G.model_sum_slices(out, torch.zeros(129 * 72), 2, 129 * 72, 129 * 72, False)
    assert torch.equal(tot.view(129, 72), G.expected(c["pre"][0], F32))
    bad = G.model_sum_slices(out, torch.zeros(129 * 72), 2, 129 * 72, 129 * 72, False, defect="one_slice_more")
    assert bool(bad.isnan().all())


def _group_model(n, split, defect=None):
    ps, checks = [], []
    T_ = 200
    for i in range(n):
        Ni, Ki = T.GROUP_SIZES[i]
        dy, x = G.ints((Ni, T_), 7, 100 + i), G.ints((Ki, T_), 7, 200 + i)
        a, lda = G.place(dy, 1, BF)
        b, ldb = G.place(x, 1, BF)
        if split > 1:
            Cf = torch.full((split * Ni * Ki + 8,), float("nan"), dtype=F32)
        else:
            Cf, idx = G.alloc_c(Ni, Ki, F32, Ki)
        ps.append(dict(A=a, B=b, C=Cf, dtype=BF, out_dtype=F32, la=1, lb=1, M=Ni, N=Ki, K=T_, lda=lda, ldb=ldb, ldc=Ki,
                       split_stride=Ni * Ki if split > 1 else 0))
        checks.append((Cf, G.expected(G.product(dy, x), F32)))
    G.model_group(ps, split, defect)
    for i, (Cf, exp) in enumerate(checks):
        Ni, Ki = T.GROUP_SIZES[i]
        if split > 1:
            G.check_workspace(Cf[:split * Ni * Ki].view(split, Ni, Ki), split, G.used_slices(T_, split), exp, f"product {i}")
        else:
            C0, idx = G.alloc_c(Ni, Ki, F32, Ki)
            G.check_c(Cf, C0, idx, exp[None], f"product {i}")


@pytest.mark.parametrize("n,split", [(1, 1), (2, 3), (8, 1), (8, 2)])
def test_group_model(n, split):
    _group_model(n, split)
    if n > 1:
        with pytest.raises(AssertionError):
            _group_model(n, split, defect="tile_start_off_by_one")


def test_every_defect_is_covered():
    covered = set(DEFECT_CASES) | {"one_slice_more", "tile_start_off_by_one"}
    assert covered == set(G.DEFECTS)


def test_slice_counts_are_fixed_points_of_the_kernel_cut():
    """the callers sum exactly `sk` slices of an uninitialised workspace, the kernels write slice y only while y * ceil(nk / sk) < nk: for
    every nk = 1 .. 1100 and every requested count s = 1 .. 64 the count the callers derive (ops.wgrad_splits' s_eff, the skinny path's and
    linear_wgrad_group's recomputation) must reproduce itself under the kernel's cut, ceil(nk / ceil(nk / s_eff)) == s_eff"""
    for nk in range(1, 1101):
        for s in range(1, 65):
            per = G.cdiv(nk, s)
            s_eff = G.cdiv(nk, per)
            assert G.cdiv(nk, G.cdiv(nk, s_eff)) == s_eff, (nk, s, s_eff)
            assert (s_eff - 1) * G.cdiv(nk, s_eff) < nk          # the last summed slice owns at least one K-tile
            assert G.used_slices(nk * 64, s) == s_eff


def test_wgrad_splits_returns_fixed_points():
    """ops.wgrad_splits itself (host arithmetic only), both cost models, over token counts with every K-tile remainder"""
    from muse import ops
    for tile, slots in ((128, 512), (256, 256)):
        for K in list(range(64, 4200, 72)) + [16448, 65536, 70000]:
            for M, N in ((768, 768), (3072, 768), (256, 256), (1024, 4096)):
                sk = ops.wgrad_splits(M, N, K, torch.bfloat16, slots=slots, tile=tile)
                assert sk >= 1 and G.used_slices(K, sk) == sk, (tile, M, N, K, sk)


def test_probe_bounds_and_storage():
    """assert_exact refuses an inexact probe; place() keeps the loader contract: zeros up to the chunk, NaN beyond"""
    with pytest.raises(AssertionError):
        G.assert_exact(2343, 1023, 7)
    G.assert_exact(2342, 1023, 7)
    with pytest.raises(AssertionError):
        G.to_dtype_exact(torch.tensor([1023]), BF)
    X = G.ints((5, 13), 7, 1)
    st, ld = G.place(X, 0, BF, lead=8)
    body = st[8:].view(7, ld)
    assert ld == 24 and bool(st[:8].isnan().all()) and bool(body[5:].isnan().all()) and bool(body[:5, 16:].isnan().all())
    assert bool((body[:5, 13:16] == 0).all()) and torch.equal(body[:5, :13].double(), X.double())
    st, ld = G.place(X, 1, F32)
    body = st.view(15, ld)
    assert ld == 12 and torch.equal(body[:13, :5].double(), X.t().double()) and bool((body[:13, 5:8] == 0).all())
    assert bool(body[:13, 8:].isnan().all()) and bool(body[13:].isnan().all())
    assert G.used_slices(2816, 16) == 15 and G.used_slices(200, 3) == 2 and G.used_slices(520, 7) == 5
