"""The Paella VQ tokenizer on the GPU: the kernels of csrc/paella.hip one by one against the float64 CPU restatement
(tests/paella_cpu.py), and muse.modeling_paella_vq.PaellaVQModel against the real reference's goldens (tests/golden/paella_*.npz,
make_golden_paella.py) in both compute modes, plus one full-width geometry against the restatement in float64."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paella_cpu as P  # noqa: E402
import paella_weights as PW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def rows(x_nchw):
    """NCHW (CPU) -> channels-last rows [B*H*W, C] f32 on the device"""
    return x_nchw.permute(0, 2, 3, 1).reshape(-1, x_nchw.shape[1]).float().contiguous().to(DEV)


def nchw(r, B, H, W):
    return r.view(B, H, W, -1).permute(0, 3, 1, 2)


# ---- kernel: mix_fwd -----------------------------------------------------------------------------------------------------------------
def _mix_inputs(B, H, W, C, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C, H, W), generator=gen)
    w = torch.randn((C, 1, 3, 3), generator=gen) / 3
    b = 0.1 * torch.randn(C, generator=gen)
    g = 0.5 * torch.randn(6, generator=gen)
    return x, w, b, g


def _mix_gpu(x, w, b, g):
    from muse import ops
    B, C, H, W = x.shape
    w9 = w.reshape(C, 9).t().contiguous().to(DEV)
    return nchw(ops.paella_mix_fwd(rows(x), w9, b.to(DEV), g.to(DEV), B, H, W), B, H, W)


# (the last two: the widths at which a lane of the statistics pass holds three and four 16-byte vectors - 1024 is the entry point's cap)
MIX_SHAPES = [(1, 1, 1, 24), (1, 1, 5, 24), (1, 5, 1, 48), (2, 2, 3, 24), (2, 7, 9, 96), (1, 8, 8, 192), (1, 8, 8, 384), (1, 33, 17, 48),
              (1, 2, 3, 520), (1, 3, 2, 1024)]


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_fwd_against_float64(shape):
    """f32 chain per element: one normalisation, nine fmas, two more operations -> 2e-6 of the output's largest value"""
    x, w, b, g = _mix_inputs(*shape, seed=sum(shape))
    want = P.mix(x.double(), w.double(), b.double(), g.double())
    err = maxrel(_mix_gpu(x, w, b, g), want)
    print("mix_fwd", shape, "maxrel %.3e" % err)
    assert err < 2e-6


def test_mix_fwd_replicates_the_border():
    """a constant interior inside a strongly different border: zero padding instead of replication is off by far more than the bar"""
    B, H, W, C = 1, 6, 7, 24
    x, w, b, g = _mix_inputs(B, H, W, C, seed=5)
    x[:, :, 1:-1, 1:-1] = x[:, :, 2:3, 2:3].clone()
    x[:, :, 0] *= 25.0
    x[:, :, -1] *= -25.0
    x[:, :, :, 0] += 40.0 * torch.sign(x[:, :, :, 0])
    g[2] = 1.5
    want = P.mix(x.double(), w.double(), b.double(), g.double())
    t = P._ln(x.double()) * (1 + g[0].double()) + g[1].double()
    zero_padded = x.double() + g[2].double() * F.conv2d(t, w.double(), b.double(), padding=1, groups=C)
    assert maxrel(zero_padded, want) > 1e-2
    err = maxrel(_mix_gpu(x, w, b, g), want)
    print("mix_fwd border maxrel %.3e" % err)
    assert err < 2e-6


def test_mix_fwd_with_g2_zero_returns_x():
    x, w, b, g = _mix_inputs(2, 7, 9, 96, seed=8)
    g[2] = 0.0
    assert torch.equal(_mix_gpu(x, w, b, g).cpu(), x)


# ---- kernel: patch rows, and the two resampling convolutions as gather + product ---------------------------------------------------------
def _engine():
    from muse.modeling_paella_vq import PaellaVQModel
    return PaellaVQModel(**PW.PAELLA_TINY).to(DEV)


@pytest.mark.parametrize("geom", [(4, 2, 1, 1), (2, 1, 1, 1), (2, 1, 0, 1), (2, 1, 1, 0), (2, 1, 0, 0)], ids=str)
def test_patch_rows_is_the_gather(geom):
    from muse import ops
    KS, stride, pt, pl = geom
    B, H, W, C = 2, 6, 10, 24
    x = torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(3))
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    got = ops.patch_rows(x.reshape(-1, C).to(DEV), B, H, W, C, KS, stride, pt, pl, Ho, Wo)
    assert torch.equal(got.cpu(), P.patch_rows(x, KS, stride, pt, pl, Ho, Wo))


RESAMPLE = [(1, 2, 2, 24, 48), (2, 6, 10, 24, 48), (1, 8, 8, 192, 384)]


@pytest.mark.parametrize("B,H,W,cin,cout", RESAMPLE)
def test_conv_down_as_gather_and_product(B, H, W, cin, cout):
    gen = torch.Generator().manual_seed(cin + H)
    conv = torch.nn.Conv2d(cin, cout, 4, 2, 1)
    conv.weight.data = torch.randn(conv.weight.shape, generator=gen) / (16 * cin) ** 0.5
    conv.bias.data = 0.1 * torch.randn(cout, generator=gen)
    x = torch.randn((B, cin, H, W), generator=gen)
    want = F.conv2d(x.double(), conv.weight.data.double(), conv.bias.data.double(), stride=2, padding=1)
    got = nchw(_engine()._down(rows(x), conv.to(DEV), B, H, W), B, H // 2, W // 2)
    err = maxrel(got, want)
    print("conv down", (B, H, W, cin, cout), "maxrel %.3e" % err)
    assert err < 2e-5


@pytest.mark.parametrize("B,H,W,cout,cin", RESAMPLE)
def test_conv_transpose_as_gather_and_product(B, H, W, cout, cin):
    gen = torch.Generator().manual_seed(cin + W)
    conv = torch.nn.ConvTranspose2d(cin, cout, 4, 2, 1)
    conv.weight.data = torch.randn(conv.weight.shape, generator=gen) / (4 * cin) ** 0.5
    conv.bias.data = 0.1 * torch.randn(cout, generator=gen)
    x = torch.randn((B, cin, H, W), generator=gen)
    want = F.conv_transpose2d(x.double(), conv.weight.data.double(), conv.bias.data.double(), stride=2, padding=1)
    got = nchw(_engine()._up(rows(x), conv.to(DEV), B, H, W), B, 2 * H, 2 * W)
    err = maxrel(got, want)
    print("conv transpose", (B, H, W, cin, cout), "maxrel %.3e" % err)
    assert err < 2e-5


def test_in_block_and_out_block_against_float64():
    from muse import ops
    gen = torch.Generator().manual_seed(21)
    for B, H, W, C in ((1, 2, 2, 24), (2, 6, 10, 48), (1, 10, 6, 96)):
        img = torch.rand((B, 3, H, W), generator=gen)
        w_in, b_in = torch.randn((C, 12, 1, 1), generator=gen) / 12 ** 0.5, 0.1 * torch.randn(C, generator=gen)
        want = F.conv2d(F.pixel_unshuffle(img.double(), 2), w_in.double(), b_in.double())
        got = ops.paella_in_block(img.to(DEV), w_in.reshape(C, 12).t().contiguous().to(DEV), b_in.to(DEV))
        assert maxrel(nchw(got, B, H // 2, W // 2), want) < 2e-5      # (the exact-f32 bar of the products: these are 12- and C-term dots)
        x = torch.randn((B, C, H // 2, W // 2), generator=gen)
        w_out, b_out = torch.randn((12, C, 1, 1), generator=gen) / C ** 0.5, 0.1 * torch.randn(12, generator=gen)
        want = F.pixel_shuffle(F.conv2d(x.double(), w_out.double(), b_out.double()), 2)
        got = ops.paella_out_block(rows(x), w_out.reshape(12, C).contiguous().to(DEV), b_out.to(DEV), B, H, W)
        assert maxrel(got, want) < 2e-5


# ---- kernel: vq_nearest_small ------------------------------------------------------------------------------------------------------------
def _vq_inputs(N, Kc, D, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)), torch.from_numpy(rng.standard_normal((Kc, D)).astype(np.float32))


def _vq_check(z, cb, require_no_disagreement):
    """indices against the float64 argmin: a disagreement is acceptable only where the float64 relative gap between the two squared
    distances is <= 2^-20 (16 units of f32 round-off: seven roundings per four-term direct sum, two sums); the returned squared
    distance is within 2^-20 relative of float64"""
    from muse import ops
    idx, dist = ops.vq_nearest_small(z.to(DEV), cb.to(DEV), return_dist=True)
    idx, dist = idx.cpu(), dist.cpu().double()
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (z.shape[0],)
    d64 = P.sqdist(z.double(), cb.double())
    want = d64.argmin(1)
    ar = torch.arange(z.shape[0])
    best, got = d64[ar, want], d64[ar, idx]
    bad = idx != want
    assert bool(((got - best)[bad] <= 2.0 ** -20 * got[bad]).all())
    if require_no_disagreement:
        assert int(bad.sum()) == 0
    assert bool(((dist - got).abs() <= 2.0 ** -20 * got).all())
    return idx


def test_vq_nearest_small_8192_codes():
    """seed 0: the float64 answer has no relative squared-distance gap below 1.7e-3 over these 300 rows (checked on the CPU), so the
    indices equal the float64 argmin exactly - and the expanded-form ops.vq_nearest on the same input"""
    from muse import ops
    z, cb = _vq_inputs(300, 8192, 4, 0)
    two = torch.topk(P.sqdist(z.double(), cb.double()), 2, dim=1, largest=False).values
    assert float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()) > 1e-3
    idx = _vq_check(z, cb, True)
    assert torch.equal(ops.vq_nearest(z.to(DEV), cb.to(DEV)).cpu(), idx)


@pytest.mark.parametrize("N,Kc,D", [(1, 100, 4), (300, 8192, 8), (130, 2049, 3), (70, 5000, 5)])
def test_vq_nearest_small_other_shapes(N, Kc, D):
    _vq_check(*_vq_inputs(N, Kc, D, 0), (N, Kc, D) in ((1, 100, 4), (300, 8192, 8)))


def test_vq_nearest_small_lowest_index_wins_a_tie():
    from muse import ops
    z, cb = _vq_inputs(64, 100, 4, 2)
    cb[70] = cb[5].clone()
    z[:] = cb[5]
    idx, dist = ops.vq_nearest_small(z.to(DEV), cb.to(DEV), return_dist=True)
    assert bool((idx.cpu() == 5).all()) and bool((dist.cpu() == 0).all())
    # ... also across the four code quarters a workgroup scans in parallel, and across LDS chunks
    z, cb = _vq_inputs(3, 8192, 4, 3)
    cb[[40, 700, 1500, 2047, 2048, 6000]] = cb[1100].clone()
    z[:] = cb[1100]
    assert ops.vq_nearest_small(z.to(DEV), cb.to(DEV)).cpu().tolist() == [40, 40, 40]


# ---- the model against the reference goldens ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg, side = PW.FIXTURES[name]
    seed = int(g["seed"])
    return g, cfg, PW.fill_paella(PW.paella_shapes(cfg), seed), PW.paella_images(int(g["batch"]), side, side, seed + 1), \
        PW.paella_images(1, *PW.NONSQUARE, seed + 2)


@pytest.mark.parametrize("cd", [torch.float32, "bf16x3"], ids=str)
@pytest.mark.parametrize("name", sorted(PW.FIXTURES))
def test_paella_vs_reference_golden(golden_dir, name, cd):
    from muse.modeling_paella_vq import PaellaVQModel
    g, cfg, sd, px, px_ns = _fixture(golden_dir, name)
    v = PaellaVQModel(**cfg)
    v.load_state_dict(sd, strict=True)
    v.to(DEV).eval().set_compute_dtype(cd)
    px = px.to(DEV)
    z_rows, (B, H, W) = v._encode_rows(px)
    err_z = maxrel(nchw(z_rows, B, H, W), torch.from_numpy(g["z"]))
    z_q, idx, loss = v.encode(px)
    tol = 1e-4 if cd == torch.float32 else 2e-4
    rec, rec_decode = v.decode_code(idx), v.decode(z_q)
    err_rec, err_dec = maxrel(rec, torch.from_numpy(g["rec"])), maxrel(rec_decode, torch.from_numpy(g["rec_decode"]))
    print(name, cd, "z %.3e rec %.3e rec_decode %.3e" % (err_z, err_rec, err_dec))
    assert err_z < (2e-5 if cd == torch.float32 else 1e-4)
    assert loss is None and idx.dtype == torch.int64 and tuple(idx.shape) == g["indices"].shape
    assert np.array_equal(idx.cpu().numpy(), g["indices"])              # bit-exact token indices (margin recorded in the fixture)
    assert np.array_equal(z_q.cpu().numpy(), g["z_q"])
    assert err_rec < tol and err_dec < tol
    assert torch.equal(v.get_code(px), idx)
    assert torch.equal(v(px), rec_decode)
    assert np.array_equal(v.get_code(px_ns.to(DEV)).cpu().numpy(), g["code_nonsquare"])
    assert torch.equal(v.decode_code(idx), rec)


@pytest.mark.parametrize("cd", [torch.float32, "bf16x3"], ids=str)
def test_batch_chunks_reproduce_the_whole_batch(golden_dir, monkeypatch, cd):
    """a batch whose largest activation passes the chunk limit is encoded / decoded image group by image group: with the limit set to
    one image's worth (3 chunks) and to two images' worth (2 chunks) of a 3-image batch, the exact-f32 mode gives bit-identical outputs
    (a row's product does not depend on how many rows share the launch); in the bf16x3 mode the row count decides which of the
    three-product forms a GEMM takes (ops._gemm_bf16x3), each 2^-16 relative per product: the indices are equal (fixture margin 2.7e-3)
    and the images agree within the mode's golden bar"""
    import muse.modeling_paella_vq as M
    g, cfg, sd, px, _ = _fixture(golden_dir, "paella_tiny")
    v = M.PaellaVQModel(**cfg)
    v.load_state_dict(sd, strict=True)
    v.to(DEV).eval().set_compute_dtype(cd)
    px = torch.cat([px, px[:1]], 0).to(DEV)                                # 3 images, all inside the fixture's index margin
    z_q, idx, _ = v.encode(px)
    rec, rec_decode = v.decode_code(idx), v.decode(z_q)
    B, _, H, W = px.shape
    per_image = (H // 2) * (W // 2) * 4 * 24 * 4                            # bytes of level 0's hidden rows, the encoder's widest tensor
    assert len(v._chunks(B, (H // 2) * (W // 2), 4 * 24)) == 1
    for limit, want_chunks in ((per_image, 3), (2 * per_image + 7, 2)):
        monkeypatch.setattr(M, "_CHUNK_BYTES", limit)
        assert len(v._chunks(B, (H // 2) * (W // 2), 4 * 24)) == want_chunks
        z_q2, idx2, _ = v.encode(px)
        assert torch.equal(idx2, idx) and torch.equal(z_q2, z_q) and torch.equal(v.get_code(px), idx)
        if cd == torch.float32:
            assert torch.equal(v.decode_code(idx), rec) and torch.equal(v.decode(z_q), rec_decode)
        else:
            assert maxrel(v.decode_code(idx), rec) < 2e-4 and maxrel(v.decode(z_q), rec_decode) < 2e-4


def test_paella_full_width_bf16x3_against_float64():
    """levels 3, c_hidden 384, 8192 codes on one 64 x 64 image (2 bottleneck blocks: depth adds no kernel path): the channel counts
    and the codebook of the f8 configurations.  Seed 1400: the f32 restatement picks the float64 indices everywhere (smallest float64
    relative gap 2.3e-2, checked on the CPU)."""
    from muse.modeling_paella_vq import PaellaVQModel
    cfg = dict(levels=3, bottleneck_blocks=2, c_hidden=384, c_latent=4, codebook_size=8192, scale_factor=0.3764)
    sd = PW.fill_paella(PW.paella_shapes(cfg), 1400)
    px = PW.paella_images(1, 64, 64, 1401)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count()))
    try:
        with torch.no_grad():
            z64 = P.encoder(sd, cfg, px, torch.float64)
            idx64, d64 = P.nearest(z64, sd["vquantizer.codebook.weight"])
            rec64 = P.decode_code(sd, cfg, idx64, torch.float64)
            assert torch.equal(P.get_code(sd, cfg, px, torch.float32), idx64)
    finally:
        torch.set_num_threads(threads)
    v = PaellaVQModel(**cfg)
    v.load_state_dict(sd, strict=True)
    v.to(DEV).eval().half()
    assert v.compute_dtype == "bf16x3"
    z_rows, (B, H, W) = v._encode_rows(px.to(DEV))
    idx = v.get_code(px.to(DEV)).cpu()
    rec = v.decode_code(idx64.to(DEV))
    err_z, err_rec = maxrel(nchw(z_rows, B, H, W), z64), maxrel(rec, rec64)
    bad = (idx != idx64).view(-1)
    print("full width bf16x3: z %.3e rec %.3e index disagreements %d" % (err_z, err_rec, int(bad.sum())))
    assert err_z < 1e-4 and err_rec < 3e-4
    ar = torch.arange(idx64.numel())
    best, got = d64[ar, idx64.view(-1)], d64[ar, idx.view(-1)]
    assert bool(((got - best)[bad] < 1e-3 * got[bad]).all()) and int(bad.sum()) <= 2
