"""CPU: class surface / file formats of the drop-in boundary, C-ABI symbol export, host logic."""
import ctypes
import os
import re
import tempfile

import numpy as np

import pytest
import torch

import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transformer_surface_and_roundtrip(golden_dir):
    import muse
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    shapes = W.transformer_shapes(W.TRANSFORMER_TINY)
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in sd)
    assert m.config.mask_token_id == W.TRANSFORMER_TINY["vocab_size"] - 1
    assert m.output_size == W.TRANSFORMER_TINY["vocab_size"]
    # config.json byte-identical to what the reference writes for the same kwargs
    assert m.to_json_string() == open(os.path.join(golden_dir, "config_transformer_tiny.json")).read()
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        assert sorted(os.listdir(d)) == ["config.json", "pytorch_model.bin"]
        m2 = muse.MaskGitTransformer.from_pretrained(d)
        assert not m2.training and m2.config._name_or_path == d
        for a, b in zip(sd.values(), m2.state_dict().values()):
            assert torch.equal(a, b)
        bad = {k: v for k, v in sd.items() if k != "encoder_layer_norm.weight"}
        torch.save(bad, os.path.join(d, "pytorch_model.bin"))
        with pytest.raises(ValueError):
            muse.MaskGitTransformer.from_pretrained(d)
    with pytest.raises(EnvironmentError):
        muse.MaskGitTransformer.from_pretrained("/nonexistent/dir/for/sure")
    m.enable_xformers_memory_efficient_attention()  # accepted no-op (train script calls it)
    assert m.num_parameters() == sum(int(torch.tensor(s).prod()) for s in shapes.values())


def test_flat_parameter_storage():
    import muse
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    assert m._flat_ok()
    l0 = m.transformer_layers[0]
    q, k, v = l0.attention.query.weight, l0.attention.key.weight, l0.attention.value.weight
    assert k.data_ptr() == q.data_ptr() + q.numel() * 4 and v.data_ptr() == k.data_ptr() + k.numel() * 4
    assert l0.ffn.wi_1.weight.data_ptr() == l0.ffn.wi_0.weight.data_ptr() + l0.ffn.wi_0.weight.numel() * 4
    sd = W.fill_state_dict(W.transformer_shapes(W.TRANSFORMER_TINY), 7, "transformer")
    m.load_state_dict(sd)
    assert m._flat_ok() and torch.equal(m.state_dict()["mlm_layer.to_logits.weight"], sd["mlm_layer.to_logits.weight"])
    m.double if False else None
    g = m.flat_grads()
    assert g.numel() == m.flat_params().numel()


def test_fused_adamw_parameter_groups_host_logic(monkeypatch):
    """training/train_muse.py:425-445 hands the optimizer TWO parameter groups (no weight decay on bias / LayerNorm / embedding
    weights).  Host side of muse.FusedAdamW for them, without a GPU: the segment table of the flat buffer (neighbouring parameters of a
    group merged, padding kept with its parameter), range-wise application against the shared table, torch.optim.AdamW's state-dict
    numbering.  The HIP kernel is replaced by its CPU restatement (oracle.adamw_step per segment) - the kernel itself is tested on the
    GPU (test_adamw_flat_groups_matches_torch_and_flat)."""
    import muse
    from muse import ops
    from oracle import maskgit_oracle as O
    calls = []

    def groups_cpu(p, g, m, v, p_bf16, base, seg_end, seg_group, groups, step, grad_scale=1.0):
        assert p_bf16 is None and grad_scale == 1.0
        calls.append((base, base + p.numel()))
        lo = 0
        for e, k in zip(seg_end.tolist(), seg_group.tolist()):
            a, b = max(lo, base), min(e, base + p.numel())
            if a < b:
                h = groups[k]
                sl = slice(a - base, b - base)
                O.adamw_step(p[sl], g[sl], m[sl], v[sl], int(step), h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"])
            lo = e
    monkeypatch.setattr(ops, "adamw_flat_groups", groups_cpu)
    monkeypatch.setattr(ops, "adamw_flat", lambda *a, **k: (_ for _ in ()).throw(AssertionError("single-group kernel on a grouped optimizer")))
    torch.manual_seed(5)
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    m.set_compute_dtype(torch.float32)
    wd = 0.3
    groups = muse.grouped_parameters(m, wd)
    names = {id(p): n for n, p in m.named_parameters()}
    assert sorted(names[id(p)] for p in groups[1]["params"] if "layers" not in names[id(p)]) == [
        "embed.position_embeddings.weight", "embed.word_embeddings.weight", "encoder_layer_norm.weight", "mlm_layer.mlm_ln.weight"]
    opt = muse.FusedAdamW(groups, lr=1e-2, betas=(0.9, 0.99), weight_decay=wd, eps=1e-8)
    seg_end, seg_group = opt._segments(m)
    assert int(seg_end[-1]) == m.flat_params().numel() and bool((seg_end[1:] > seg_end[:-1]).all())
    assert bool((seg_group[1:] != seg_group[:-1]).all())                  # neighbouring segments of one group are merged
    gid_of = {id(p): k for k, g in enumerate(groups) for p in g["params"]}
    for p, o in zip(m._param_order(), m._offsets):                        # every parameter lies inside a segment of its own group
        s = int((seg_end > o).nonzero()[0])
        assert int(seg_group[s]) == gid_of[id(p)] and o + p.numel() <= int(seg_end[s])
    twins = {n: torch.nn.Parameter(p.detach().clone()) for n, p in m.named_parameters()}
    nd = ("bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight")
    ref = torch.optim.AdamW([{"params": [p for n, p in twins.items() if not any(x in n for x in nd)], "weight_decay": wd},
                             {"params": [p for n, p in twins.items() if any(x in n for x in nd)], "weight_decay": 0.0}],
                            lr=1e-2, betas=(0.9, 0.99), weight_decay=wd, eps=1e-8)
    n = m.flat_params().numel()
    for step in range(3):
        g = m.flat_grads()
        g.copy_(torch.sin(torch.arange(n, dtype=torch.float32) * 0.01 * (step + 1)))
        for p, gv in zip(m._param_order(), m._grad_views):
            p.grad = gv
            twins[names[id(p)]].grad = gv.detach().clone()
        if step == 1:     # range-wise, as backward reports: the tail first, then the rest (what begin_step_in_backward's hook does)
            opt._ensure_flat_state(m.flat_params())
            opt._ranges_done_live = (opt._step + 1, [])
            cut = m._offsets[len(m._offsets) // 2] + 8
            opt._apply(m, cut, n, None); opt._ranges_done_live[1].append((cut, n))
            opt._ranges_done, opt._ranges_done_live = opt._ranges_done_live, None
        opt.step()
        ref.step()
    assert (0, n) in calls and any(b > 0 for b, _ in calls)
    for k, p in m.named_parameters():
        assert float((p.detach() - twins[k].detach()).abs().max()) < 1e-6, k
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in rsd["param_groups"]]
    for i, st in rsd["state"].items():
        assert torch.allclose(sd["state"][i]["exp_avg_sq"], st["exp_avg_sq"], rtol=1e-5, atol=1e-10), i
    opt2 = muse.FusedAdamW(muse.grouped_parameters(m, wd), lr=1e-2, betas=(0.9, 0.99), weight_decay=wd, eps=1e-8)
    opt2.load_state_dict(rsd)
    assert opt2._step == 3 and [g["weight_decay"] for g in opt2.param_groups] == [wd, 0.0]
    with pytest.raises(muse._hip.MuseHipError):
        muse.FusedAdamW([{"params": [p]} for p in list(m.parameters())[:9]], lr=1e-3)     # nine groups / a subset of the buffer


def test_vqgan_surface(golden_dir):
    import muse
    v = muse.MaskGitVQGAN(**W.VQGAN_TINY)
    shapes = W.vqgan_shapes(W.VQGAN_TINY)
    sd = v.state_dict()
    assert set(sd.keys()) == set(shapes.keys())
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in sd)
    assert v.num_embeddings == W.VQGAN_TINY["num_embeddings"]
    assert v.to_json_string() == open(os.path.join(golden_dir, "config_vqgan_tiny.json")).read()
    full = muse.MaskGitVQGAN()
    assert full.num_parameters() == 54515587
    assert len(full.state_dict()) == 168


@pytest.mark.parametrize("name,cfg", [("taming_tiny", W.TAMING_TINY), ("taming_tiny_pool", W.TAMING_TINY_POOL)])
def test_taming_vqgan_surface(golden_dir, name, cfg):
    """row f4: muse.VQGANModel keeps the reference's state-dict template (muse/modeling_taming_vqgan.py), writes the same
    config.json, round-trips through save_pretrained / from_pretrained, and has no CPU path"""
    import muse
    from muse._hip import MuseHipError
    v = muse.VQGANModel(**cfg)
    sd = v.state_dict()
    assert {k: tuple(t.shape) for k, t in sd.items()} == W.taming_shapes(cfg)
    assert v.num_embeddings == cfg["num_embeddings"] and v.config.latent_size == cfg["resolution"] // 2 ** (len(cfg["channel_mult"]) - 1)
    assert v.to_json_string() == open(os.path.join(golden_dir, f"config_{name}.json")).read()
    with tempfile.TemporaryDirectory() as d:
        v.save_pretrained(d)
        v2 = muse.VQGANModel.from_pretrained(d)
        assert not v2.training
        for a, b in zip(sd.values(), v2.state_dict().values()):
            assert torch.equal(a, b)
    with pytest.raises(MuseHipError):
        v.encode(torch.zeros(1, 3, cfg["resolution"], cfg["resolution"]))
    with pytest.raises(NotImplementedError):
        muse.VQGANModel(**{**cfg, "dropout": 0.1})


def test_taming_vqgan_full_size_template():
    import muse
    full = muse.VQGANModel(num_embeddings=8192)   # openMUSE/vqgan-f16-8192-laion geometry (configs/cc12m_uvit_clip.yaml:19-21)
    assert len(full.state_dict()) == 343 and full.num_parameters() == 73976707   # the reference's counts


def test_no_cpu_fallback():
    import muse
    from muse._hip import MuseHipError
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TINY)
    with pytest.raises(MuseHipError):
        m(torch.zeros(2, 17, dtype=torch.long))
    v = muse.MaskGitVQGAN(**W.VQGAN_TINY)
    with pytest.raises(MuseHipError):
        v.encode(torch.zeros(1, 3, 16, 16))


def test_unsupported_configs_fail_loudly():
    import muse
    with pytest.raises(NotImplementedError):
        muse.MaskGitTransformer(vocab_size=48, hidden_size=32, num_attention_heads=2, use_conv_in_out=True)
    with pytest.raises(ValueError):
        muse.MaskGitTransformer(vocab_size=48, hidden_size=30, num_attention_heads=4)
    m = muse.MaskGitTransformer(**W.TRANSFORMER_TEXT_TINY)
    with pytest.raises(ValueError):                       # reference :1234-1235
        m(torch.zeros(2, 16, dtype=torch.long))


@pytest.mark.parametrize("name,cfg", [("transformer_text_tiny", W.TRANSFORMER_TEXT_TINY),
                                      ("transformer_text_proj_tiny", W.TRANSFORMER_TEXT_PROJ_TINY),
                                      ("transformer_plain_tiny", W.TRANSFORMER_PLAIN_TINY),
                                      ("transformer_text_bias_tiny", W.TRANSFORMER_TEXT_BIAS_TINY),
                                      ("transformer_rms_bias_tiny", W.TRANSFORMER_RMS_BIAS_TINY),
                                      ("transformer_cc12m_2l", W.TRANSFORMER_CC12M_2L)])
def test_general_transformer_surface_and_roundtrip(golden_dir, tmp_path, name, cfg):
    """the general form of muse.MaskGitTransformer (text conditioning / RMSNorm / plain pre-LN layers): parameter names and shapes
    are the REAL reference's (the goldens list its named_parameters), a state dict loads strictly, save_pretrained ->
    from_pretrained round-trips config and weights"""
    import muse
    import numpy as np
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    m = muse.MaskGitTransformer(**cfg)
    shapes = W.transformer_shapes(cfg)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    ref_names = set(f[5:] for f in g.files if f.startswith("grad."))
    if name != "transformer_cc12m_2l":                    # (the width-1024 golden keeps a subset of the gradients)
        assert ref_names == set(shapes)
    else:
        assert ref_names <= set(shapes)
    sd = W.fill_state_dict(shapes, 5, "transformer")
    m.load_state_dict(sd, strict=True)
    m.save_pretrained(str(tmp_path))
    m2 = muse.MaskGitTransformer.from_pretrained(str(tmp_path))
    assert m2.config.norm_type == cfg["norm_type"] and m2.config.mask_token_id == cfg["vocab_size"] - 1
    assert m2.output_size == (cfg["codebook_size"] if cfg.get("use_codebook_size_for_output") else cfg["vocab_size"])
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert not m2.training and m._general and m2._general


def test_library_exports_every_declared_symbol():
    """the C-ABI library loads and exports every symbol include/muse_hip.h declares (no compute calls on CPU)"""
    hdr = open(os.path.join(ROOT, "include", "muse_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(muse_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 30
    from muse import _hip
    assert declared == set(_hip.SIGNATURES), declared ^ set(_hip.SIGNATURES)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert _hip.lib().muse_version() == 1
    assert _hip.lib().muse_layernorm_bwd_nblk(16448) == 1028


def test_ctypes_signatures_match_the_header():
    """every prototype of include/muse_hip.h against _hip.SIGNATURES, argument by argument: the same arity and the same kind per
    position (a ctypes list one entry short shifts every later argument - a pointer arrives as an int), and the same return type"""
    from muse import _hip
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", "muse_hip.h")).read(), flags=re.S)
    protos = re.findall(r"^\s*(int|int64_t)\s+(muse_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    assert len(protos) == len(set(_hip.SIGNATURES)), sorted({p[1] for p in protos} ^ set(_hip.SIGNATURES))

    def c_kind(param):
        words = param.replace("*", " * ").split()
        if "*" in words:
            return "ptr"
        return {"int32_t": "i32", "int": "i32", "int64_t": "i64", "float": "f32", "uint32_t": "u32", "uint64_t": "u64"}[words[0]]

    def ctypes_kind(t):
        if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
            return "ptr"
        return {ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_uint32: "u32", ctypes.c_uint64: "u64"}[t]

    bad = []
    for ret, name, params in protos:
        params = [p.strip() for p in params.split(",")]
        want = [] if params == ["void"] else [c_kind(p) for p in params]
        got = [ctypes_kind(t) for t in _hip.SIGNATURES[name]]
        ret_got = _hip._RESTYPES.get(name, ctypes.c_int32)
        if want != got or ret_got is not {"int": ctypes.c_int32, "int64_t": ctypes.c_int64}[ret]:
            bad.append((name, ret, want, got))
    assert not bad, bad


def test_sampling_schedules():
    from muse.sampling import cosine_schedule, get_mask_chedule
    t = torch.tensor([0.0, 0.5, 1.0])
    assert torch.allclose(cosine_schedule(t), torch.tensor([1.0, 0.70710678, 0.0]), atol=1e-6)
    assert get_mask_chedule("cosine") is cosine_schedule
    with pytest.raises(ValueError):
        get_mask_chedule("nope")


def test_host_side_plans():
    """pure host logic around the C-ABI: split-K plan of the weight-gradient GEMMs and the eligibility predicates of the
    LDS-DMA convolution / its fused GroupNorm statistics (no GPU, no library call)"""
    from muse import ops
    # config B, bs 64: T = 16448 tokens -> 257 K-tiles of 64.  256x256 tiles, 256 slots: few tiles -> many slices, but never
    # more workspace traffic than the rounds it saves
    plan = {(m, n): ops.wgrad_splits(m, n, 16448, torch.bfloat16, slots=256, tile=256)
            for (m, n) in [(2304, 768), (768, 768), (6144, 768), (768, 3072)]}
    assert plan == {(2304, 768): 9, (768, 768): 26, (6144, 768): 3, (768, 3072): 7}
    for (m, n), s in plan.items():
        tiles = -(-m // 256) * -(-n // 256)
        per = -(-257 // s)
        assert -(-257 // per) == s            # every slice owns at least one K-tile (no empty workspace slice)
        assert tiles * s <= 2 * 256           # at most two rounds of resident blocks
    # 128x128 kernel: efficiency rule, at least 4 K-tiles per slice
    s128 = ops.wgrad_splits(6144, 768, 16448, torch.bfloat16)
    assert 1 <= s128 <= 257 // 4
    assert ops.wgrad_splits(6144, 768, 64, torch.bfloat16) == 1   # a single K-tile cannot be split
    # LDS-DMA convolution: 3x3, Cin % 32 == 0, 32-bit buffer offsets
    assert ops.conv_split2_ok(64, 256, 256, 128, 128, 3)
    assert not ops.conv_split2_ok(64, 256, 256, 128, 128, 1)        # 1x1 layers stay on the register-staged kernel
    assert not ops.conv_split2_ok(64, 256, 256, 8, 128, 3)          # RGB stem (padded to 8 channels)
    assert not ops.conv_split2_ok(256, 256, 256, 128, 128, 3)       # plane of 4 GiB: offsets would not fit 32 bits
    # fused GroupNorm statistics: whole 256-pixel tiles per image, 4 * 2^k channels per group
    assert ops.conv_gn_stats_ok(256, 256, 128, 32) and ops.conv_gn_stats_ok(16, 16, 512, 32)
    assert not ops.conv_gn_stats_ok(20, 24, 128, 32)                # 480 pixels per image
    assert not ops.conv_gn_stats_ok(16, 16, 96, 32)                 # 3 channels per group
    assert not ops.conv_gn_stats_ok(16, 16, 64, 32)                 # 2 channels per group: below one 4-channel chunk


def test_uvit_surface_and_roundtrip(golden_dir):
    """row a12: muse.MaskGiTUViT keeps the reference's state-dict template, config handling and init (CPU side only)"""
    import json
    import numpy as np
    import muse
    from muse._hip import MuseHipError
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json")))
    g = np.load(os.path.join(golden_dir, "uvit_tiny.npz"))
    ref_shapes = {k[len("param."):]: tuple(g[k].shape) for k in g.files if k.startswith("param.")}
    torch.manual_seed(0)
    m = muse.MaskGiTUViT(**cfg, some_unknown_legacy_key=123, block_num_heads_unused=None)   # unknown kwargs are dropped (:140-142)
    assert muse.MaskGiTUViT is muse.MaskGiTUViT_v2
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref_shapes                  # the reference's 120-tensor template
    assert m.config.mask_token_id == cfg["vocab_size"] - 1 and m.output_size == cfg["codebook_size"]
    assert "some_unknown_legacy_key" not in m.config
    # degenerate-at-init structure of the reference (:209-223)
    assert float(sd["mlm_layer.conv1.weight"].abs().max()) == 0.0
    assert all(float(v.abs().max()) == 0.0 for k, v in sd.items() if "adaLN_modulation.mapper" in k or k.endswith("adaLN_modulation.mapper.weight"))
    assert torch.equal(sd["mlm_layer.conv2.weight"][:, :, 0, 0], sd["embed.embeddings.weight"][: cfg["codebook_size"]])
    assert all(float((v - 1).abs().max()) == 0.0 for k, v in sd.items() if k.endswith("norm.weight"))
    m.load_state_dict({k: torch.from_numpy(g["param." + k]) for k in ref_shapes}, strict=True)
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        m2 = muse.MaskGiTUViT.from_pretrained(d)
        assert dict(m2.config)["block_out_channels"] == [24] and not m2.training
        for a, b in zip(m.state_dict().values(), m2.state_dict().values()):
            assert torch.equal(a, b)
    with pytest.raises(MuseHipError):                                                # no CPU path
        m(torch.zeros(1, 16, dtype=torch.long), torch.zeros(1, 7, 24), torch.zeros(1, 16), torch.zeros(1, 5))
    with pytest.raises(NotImplementedError):                                         # outside the built family: refused loudly
        muse.MaskGiTUViT(**{**cfg, "use_fused_mlp": True})
    assert muse.MaskGiTUViT(**{**cfg, "norm_type": "layernorm"})._default_norm_mode == 1   # (built since round 4: tests/golden/uvit_tiny_layernorm.npz)
    with pytest.raises(AssertionError):
        m.generate()


def test_pre_encoded_token_shards_roundtrip(tmp_path):
    """token shards in the layout of scripts/pre_encode.py:54-56,225-241 / training/data.py:561-573:
    a POSIX tar of `<key>.<checkpoint with '/' -> '.'>.pth` (torch.save) members + `<key>.json`"""
    import tarfile
    from muse import pre_encode as PE
    vae, txt = "openMUSE/vqgan-f16-8192-laion", "openMUSE/CLIP-ViT-L-14-DataComp.XL-s13B-b90K-penultimate"
    toks = torch.randint(0, 8192, (5, 256))
    enc = torch.randn(5, 77, 8)
    keys = [f"{i:09d}" for i in range(5)]
    path = str(tmp_path / "00000.tar")
    PE.write_token_shard(path, keys, toks, vae, encoder_hidden_states=enc, text_encoder_checkpoint=txt, metadata=[{"i": i} for i in range(5)])
    names = tarfile.open(path).getnames()
    assert names[:3] == ["000000000.openmuse.vqgan-f16-8192-laion.pth",
                         "000000000.openmuse.clip-vit-l-14-datacomp.xl-s13b-b90k-penultimate.pth", "000000000.json"]
    got = list(PE.read_token_shard(path, vae, txt))
    assert [s["__key__"] for s in got] == keys
    assert all(torch.equal(s["image_input_ids"], toks[i]) and torch.equal(s["encoder_hidden_states"], enc[i]) for i, s in enumerate(got))
    batches = list(PE.token_batches([path], vae, 2, device="cpu"))
    assert len(batches) == 2 and torch.equal(batches[1], toks[2:4])            # ragged tail dropped
    # a shard as the REFERENCE writes it (scripts/pre_encode.py:54-56: mixed-case member names, here inside a directory and with a
    # dot in the directory name): webdataset lower-cases the extension on read and keys on the base name
    import io
    ref_path = str(tmp_path / "ref.tar")
    with tarfile.open(ref_path, "w") as tar:
        for i, key in enumerate(keys[:2]):
            for ext, t in ((".openMUSE.vqgan-f16-8192-laion.pth", toks[i]), (".json", None)):
                payload = io.BytesIO()
                if t is None:
                    payload.write(b"{}")
                else:
                    torch.save(t.clone(), payload)
                info = tarfile.TarInfo(f"./shard.0/{key}{ext}")
                info.size = payload.tell()
                payload.seek(0)
                tar.addfile(info, payload)
    got = list(PE.read_token_shard(ref_path, vae))
    assert [os.path.basename(s["__key__"]) for s in got] == keys[:2]
    assert all(torch.equal(s["image_input_ids"], toks[i]) for i, s in enumerate(got))


def test_bench_config4_is_the_baseline_geometry():
    """bench.py's config-4 legs must build the geometry BASELINE.md's row U counts its 275.10 / 1137.05 GFLOP on
    (configs/cc12m_uvit_clip.yaml + block_num_heads=16: 728 725 504 parameters), the same one the full-size golden was generated with"""
    import importlib.util
    import weights as W
    import muse
    from muse import modeling_transformer_v2 as M
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.UVIT_CC12M == W.UVIT_CC12M
    init = M.MaskGiTUViT_v2._init_weights
    M.MaskGiTUViT_v2._init_weights = lambda self: None
    try:
        model = muse.MaskGiTUViT(**bench.UVIT_CC12M)
    finally:
        M.MaskGiTUViT_v2._init_weights = init
    assert sum(p.numel() for p in model.parameters()) == 728725504


def test_uvit_forced_down_up_sample_surface(golden_dir):
    """force_down_up_sample=True (configs/research_run_512_with_downsample*.yaml): state-dict keys IN ORDER, shapes and the parameter
    list equal the real reference's (downsample registered before the blocks, upsample after them; the transposed conv keeps torch's
    default init because the reference's _init_weights only matches nn.Conv2d / nn.Linear, :225-231)"""
    import json
    import muse
    g = np.load(os.path.join(golden_dir, "uvit_tiny_downup.npz"))
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny_downup.json")))
    ref = {k[len("param."):]: tuple(g[k].shape) for k in g.files if k.startswith("param.")}
    torch.manual_seed(0)
    m = muse.MaskGiTUViT(**cfg)
    assert list(m.state_dict().keys()) == list(ref.keys()) and {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref
    assert [n for n, _ in m.named_parameters()] == list(ref.keys())
    for k in ("down_blocks.0.downsample.0.norm.weight", "down_blocks.0.downsample.1.weight", "up_blocks.0.upsample.0.norm.weight",
              "up_blocks.0.upsample.1.weight"):
        assert k in ref
    C = cfg["block_out_channels"][0]
    wu = m.up_blocks[0].upsample["1"].weight.detach()
    assert float(wu.abs().max()) <= 1.0 / (4 * C) ** 0.5 and float(wu.abs().max()) > 0.05      # kaiming_uniform(a = sqrt 5): +-1/sqrt(fan_in)
    assert abs(float(m.down_blocks[0].downsample["1"].weight.detach().std()) - 0.02) < 0.002        # trunc_normal(std 0.02) like every conv
    m.load_state_dict({k: torch.from_numpy(g["param." + k]) for k in ref}, strict=True)
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        m2 = muse.MaskGiTUViT.from_pretrained(d)
        assert m2.config.force_down_up_sample and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_uvit_without_norm_gains_surface(golden_dir):
    """ln_elementwise_affine=False: the state dict and the parameter list of muse.MaskGiTUViT equal the real reference's (no norm
    weights; the gains are non-persistent constant buffers here), save / load round-trips"""
    import json
    import muse
    g = np.load(os.path.join(golden_dir, "uvit_tiny_noaffine.npz"))
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny_noaffine.json")))
    ref_keys = [k[len("param."):] for k in g.files if k.startswith("param.")]
    m = muse.MaskGiTUViT(**cfg)
    assert list(m.state_dict().keys()) == ref_keys and not any(k.endswith("norm.weight") for k in ref_keys)
    assert [n for n, _ in m.named_parameters()] == [k for k in ref_keys if "grad." + k in g.files]
    m.load_state_dict({k: torch.from_numpy(g["param." + k]) for k in ref_keys}, strict=True)
    m2 = muse.MaskGiTUViT(**dict(cfg, ln_elementwise_affine=True))           # the flag does not leak into the next model built
    assert any(k.endswith("norm.weight") for k in m2.state_dict())


def test_ema_model_host_logic(golden_dir):
    """muse.EMAModel (CPU side): the reference's decay schedule (against the decays the real class used, tests/golden/ema_tiny.npz),
    state-dict keys and validation errors, store / copy_to / restore (parameter version counters move: the models' cached bf16 weights
    are keyed on them), the call counters of skipped steps, and a loud refusal to update on the CPU"""
    import muse
    import weights as W
    from muse._hip import MuseHipError
    from muse.modeling_ema import EMAModel as SameClass
    assert SameClass is muse.EMAModel
    g = np.load(os.path.join(golden_dir, "ema_tiny.npz"))
    seed, steps = int(g["seed"]), int(g["steps"])
    for si, kw in enumerate(W.EMA_SCHEDULES):
        ema = muse.EMAModel([torch.nn.Parameter(t) for t in W.ema_params(seed, 0)], **kw)
        for step in range(1, steps + 1):
            want = float(g[f"s{si}.decay{step}"])
            if want >= 0:
                assert ema.get_decay(step) == want
    params = [torch.nn.Parameter(t) for t in W.ema_params(seed, 0)]
    ema = muse.EMAModel(params, decay=0.99, update_every=3)
    assert list(ema.state_dict().keys()) == ["decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma",
                                             "power", "shadow_params"]                       # reference :163-177
    assert all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() for s, p in zip(ema.shadow_params, params))
    with pytest.raises(MuseHipError):
        ema.step(params)                                                                     # call 1 updates: no CPU path
    assert ema.optimization_step == 1
    ema.step(params)                                                                         # calls 2, 3 are skipped (update_every 3): counters only
    ema.step(params)
    assert ema.optimization_step == 3 and ema.cur_decay_value == 0.0
    # swap in / out
    v0 = [p._version for p in params]
    ema.shadow_params = [s + 1 for s in ema.shadow_params]
    with pytest.raises(RuntimeError):
        ema.restore(params)
    ema.store(params)
    ema.copy_to(params)
    assert all(torch.equal(p, s) for p, s in zip(params, ema.shadow_params)) and all(p._version > v for p, v in zip(params, v0))
    ema.restore(params)
    assert all(torch.equal(p.detach(), t) for p, t in zip(params, W.ema_params(seed, 0))) and ema.temp_stored_params is None
    # state dict round trip + the reference's validation
    sd = ema.state_dict()
    other = muse.EMAModel(params)
    other.load_state_dict(sd)
    assert other.decay == 0.99 and other.optimization_step == 3 and all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    assert other.shadow_params[0].data_ptr() != ema.shadow_params[0].data_ptr()            # deep copy, like the reference
    for bad, msg in ((dict(decay=1.5), "Decay must be between 0 and 1"), (dict(min_decay=1), "Invalid min_decay"),
                     (dict(optimization_step=1.0), "Invalid optimization_step"), (dict(use_ema_warmup=1), "Invalid use_ema_warmup"),
                     (dict(power="x"), "Invalid power"), (dict(shadow_params=(1,)), "shadow_params must be a list"),
                     (dict(shadow_params=[1]), "shadow_params must all be Tensors")):
        with pytest.raises(ValueError, match=msg):
            muse.EMAModel(params).load_state_dict(bad)
    with pytest.raises(ValueError, match="model_cls"):
        ema.save_pretrained("/nonexistent")


def test_ema_model_save_and_from_pretrained(golden_dir):
    """EMAModel.save_pretrained / from_pretrained (reference :64-88): the average is written as the model's weights and the EMA scalars
    into its config.json.  Like the reference (observed on the real class: decay 0.97 / step 42 saved, 0.9999 / 0 after from_pretrained),
    from_pretrained restores the AVERAGE but not the scalars: `load_config(return_unused_kwargs=True)` hands back the unused *call*
    kwargs, which are empty - kept as is, a drop-in does not change what a resumed run does"""
    import json
    import muse
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json")))
    torch.manual_seed(1)
    m = muse.MaskGiTUViT(**cfg)
    ema = muse.EMAModel(m.parameters(), decay=0.97, update_after_step=5, model_cls=muse.MaskGiTUViT, model_config=m.config)
    ema.shadow_params = [s * 0.5 for s in ema.shadow_params]
    ema.optimization_step = 42
    with tempfile.TemporaryDirectory() as d:
        ema.save_pretrained(d)
        saved = json.load(open(os.path.join(d, "config.json")))
        assert saved["decay"] == 0.97 and saved["update_after_step"] == 5 and saved["optimization_step"] == 42 and "shadow_params" not in saved
        back = muse.EMAModel.from_pretrained(d, muse.MaskGiTUViT)
        assert back.decay == 0.9999 and back.update_after_step == 0 and back.optimization_step == 0      # (the reference's behaviour)
        assert back.model_cls is muse.MaskGiTUViT and back.model_config is not None
        assert all(torch.equal(a, b) for a, b in zip(back.shadow_params, ema.shadow_params))
        assert all(torch.equal(p.detach() * 0.5, s) for p, s in zip(m.parameters(), back.shadow_params))


def test_inpainting_pipeline_surface_and_image_preparation():
    """muse.PipelineMuseInpainting exists with the reference's call signature (:374-395); its image preparation = Resize(shorter side,
    bilinear) -> CenterCrop -> ToTensor of the reference (:399-405) restated on PIL alone (no torchvision in this image)"""
    import inspect
    import muse
    from PIL import Image
    from muse.pipeline_muse import _center_square
    assert issubclass(muse.PipelineMuseInpainting, muse.PipelineMuse)
    names = list(inspect.signature(muse.PipelineMuseInpainting.__call__).parameters)
    assert names[:21] == ["self", "image", "mask", "text", "negative_text", "class_ids", "timesteps", "guidance_scale", "guidance_schedule",
                          "temperature", "topk_filter_thres", "num_images_per_prompt", "use_maskgit_generate", "generator", "use_fp16",
                          "image_size", "orig_size", "crop_coords", "aesthetic_score", "prompt_embeds", "pooled_embeds"]
    d = inspect.signature(muse.PipelineMuseInpainting.__call__).parameters
    assert d["timesteps"].default == 8 and d["guidance_scale"].default == 8.0 and d["image_size"].default == 256 and d["temperature"].default == 1.0
    # a 64 x 32 picture whose left half is black and right half white, to 16 x 16: shorter side 32 -> 16 (so 32 x 16), centre 16 columns
    arr = np.zeros((32, 64, 3), np.uint8)
    arr[:, 32:] = 255
    t = _center_square(Image.fromarray(arr), 16)
    assert t.shape == (3, 16, 16) and t.dtype == torch.float32
    assert float(t[:, :, :7].max()) == 0.0 and float(t[:, :, 9:].min()) == 1.0              # the edge sits in the middle of the crop
    # already square at the target size: untouched, exactly uint8 / 255
    rng = np.random.default_rng(1)
    a = (rng.random((16, 16, 3)) * 255).astype(np.uint8)
    assert torch.equal(_center_square(Image.fromarray(a), 16), torch.from_numpy(a).permute(2, 0, 1).float() / 255.0)
    # tall picture: the crop is vertical
    tall = np.zeros((48, 16, 3), np.uint8)
    tall[16:32] = 200
    assert float(_center_square(Image.fromarray(tall), 16).min()) == float(torch.tensor(200.0) / 255.0)
    with pytest.raises(NotImplementedError):
        muse.PipelineMuse(vae=None, transformer=None)._encode_text("a", None)                  # no text encoder: loud


def test_every_reference_configuration_constructs_or_fails_like_the_reference(golden_dir):
    """tests/golden/reference_configs.json: the `model.transformer` section of every configs/*.yaml the reference's classes can be asked
    to build, with what the REAL class answered (make_golden.py::reference_configs).  Ours answers the same: builds where it builds
    (same parameter count as the state-dict template implies), raises the same ValueError text where it does not (1024 channels on 12
    block heads) and builds with the D3 override BASELINE.json's config 4 uses"""
    import json
    import muse
    cfgs = json.load(open(os.path.join(golden_dir, "reference_configs.json")))
    assert len(cfgs) == 16 and sum(v["reference_error"] is None for v in cfgs.values()) == 8
    for name, entry in cfgs.items():
        cls = muse.MaskGiTUViT if entry["architecture"] == "uvit" else muse.MaskGitTransformer
        t = dict(entry["transformer"])
        with torch.device("meta"):
            if entry["reference_error"] is None:
                m = cls(**t)
            else:
                with pytest.raises(ValueError) as e:
                    cls(**t)
                assert entry["reference_error"] == f"ValueError: {e.value}", name
                m = cls(**dict(t, block_num_heads=16))
        assert sum(p.numel() for p in m.parameters()) > 1e8, name
        assert m.config.mask_token_id == t["vocab_size"] - 1
        # the state-dict template of the real class at this configuration: same tensors, same names in the same order, same shapes
        import hashlib
        items = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        tmpl = entry["state_dict_template"]
        assert (len(items), sum(p.numel() for p in m.parameters())) == (tmpl["tensors"], tmpl["parameters"]), name
        assert hashlib.sha1(repr(items).encode()).hexdigest() == tmpl["sha1"], name


def test_pipeline_save_and_from_pretrained_with_a_text_encoder(golden_dir, tmp_path):
    """PipelineMuse.save_pretrained / from_pretrained as the reference lays a text-to-image pipeline out (:254-369): `text_encoder/`
    (a real, tiny transformers CLIPTextModelWithProjection + CLIPTokenizer built offline), `vae/`, `transformer/`; the classes are
    picked from the checkpoints' config.json; a local checkpoint without `text_encoder/` loads as a pipeline for pre-computed text
    states; the separate-paths form needs all three paths"""
    import json
    import muse
    import weights as W
    cfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json")))
    enc, tok = W.tiny_clip(str(tmp_path / "clip_src"), hidden=cfg["encoder_hidden_size"], pooled=cfg["cond_embed_dim"])
    torch.manual_seed(3)
    pipe = muse.PipelineMuse(vae=muse.VQGANModel(**W.TAMING_TINY), transformer=muse.MaskGiTUViT(**cfg), text_encoder=enc, tokenizer=tok)
    d = str(tmp_path / "pipe")
    pipe.save_pretrained(d)
    assert sorted(os.listdir(d)) == ["text_encoder", "transformer", "vae"]
    back = muse.PipelineMuse.from_pretrained(d)
    assert type(back.vae).__name__ == "VQGANModel" and type(back.transformer).__name__ == "MaskGiTUViT_v2" and not back.is_class_conditioned
    assert type(back.text_encoder).__name__ == "CLIPTextModelWithProjection" and back.tokenizer.model_max_length == 7
    for a, b in zip(enc.state_dict().values(), back.text_encoder.state_dict().values()):
        assert torch.equal(a, b)
    for a, b in zip(pipe.transformer.state_dict().values(), back.transformer.state_dict().values()):
        assert torch.equal(a, b)
    ids = lambda t: t(["a red fox"], return_tensors="pt", padding="max_length", truncation=True, max_length=t.model_max_length).input_ids   # noqa: E731
    assert torch.equal(ids(tok), ids(back.tokenizer))
    # the same checkpoint as a class-conditional pipeline: no text encoder is touched
    assert muse.PipelineMuse.from_pretrained(d, is_class_conditioned=True).text_encoder is None
    # separate paths (:270-286), and the reference's complaint when one is missing
    sep = muse.PipelineMuse.from_pretrained(text_encoder_path=os.path.join(d, "text_encoder"), vae_path=os.path.join(d, "vae"),
                                            transformer_path=os.path.join(d, "transformer"))
    assert type(sep.text_encoder).__name__ == "CLIPTextModelWithProjection" and sep.tokenizer is not None
    with pytest.raises(ValueError, match="text_encoder_path, vae_path, and transformer_path must be"):
        muse.PipelineMuse.from_pretrained(vae_path=os.path.join(d, "vae"), transformer_path=os.path.join(d, "transformer"))
    # a local checkpoint without text_encoder/: a pipeline for pre-computed text states
    import shutil
    shutil.rmtree(os.path.join(d, "text_encoder"))
    bare = muse.PipelineMuse.from_pretrained(d)
    assert bare.text_encoder is None and bare.tokenizer is None


def test_tokenizers_keep_their_derived_config_values_through_from_pretrained():
    """the VQGANs hang derived values on their config as plain attributes (num_resolutions, reduction_factor, latent_size - reference
    modeling_maskgit_vqgan.py:370-372, not part of config.json); from_pretrained registers `_name_or_path` afterwards, which rebuilds
    the config object: the derived values must still be there (the encode / decode engines read them), and still not be saved"""
    import json
    import muse
    import weights as W
    for cls, cfg in ((muse.MaskGitVQGAN, W.VQGAN_TINY), (muse.VQGANModel, W.TAMING_TINY)):
        v = cls(**cfg)
        with tempfile.TemporaryDirectory() as d:
            v.save_pretrained(d)
            saved = json.load(open(os.path.join(d, "config.json")))
            assert "num_resolutions" not in saved and "latent_size" not in saved
            b = cls.from_pretrained(d)
        assert b.config.num_resolutions == len(cfg["channel_mult"]) and b.config.reduction_factor == 2 ** (len(cfg["channel_mult"]) - 1)
        assert b.config.latent_size == cfg["resolution"] // b.config.reduction_factor and "_name_or_path" in b.config
        assert "num_resolutions" not in dict(b.config)


def test_models_and_configs_survive_deepcopy_and_pickle(golden_dir):
    """copy.deepcopy(model) - what the reference's training_utils.EMA does with the model it tracks (:61-80) - and pickling of the
    config: the frozen config rebuilds from its items and keeps its derived attributes, stays frozen; the copy owns its own storage"""
    import copy
    import json
    import pickle
    import muse
    import weights as W
    ucfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json")))
    for m in (muse.MaskGitTransformer(**W.TRANSFORMER_TINY), muse.MaskGitTransformer(**W.TRANSFORMER_TEXT_TINY), muse.MaskGiTUViT(**ucfg),
              muse.MaskGitVQGAN(**W.VQGAN_TINY), muse.VQGANModel(**W.TAMING_TINY)):
        c = copy.deepcopy(m)
        assert dict(c.config) == dict(m.config) and c.config is not m.config
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(m.state_dict().values(), c.state_dict().values()))
        with torch.no_grad():
            next(c.parameters()).add_(1.0)
        assert not torch.equal(next(c.parameters()), next(m.parameters()))
        cfg2 = pickle.loads(pickle.dumps(m.config))
        assert cfg2 == m.config and type(cfg2) is type(m.config)
        for k in ("num_resolutions", "latent_size"):
            if hasattr(m.config, k):
                assert getattr(cfg2, k) == getattr(m.config, k) and getattr(c.config, k) == getattr(m.config, k) and k not in dict(cfg2)
        with pytest.raises(Exception, match="cannot mutate"):
            cfg2["x"] = 1


_CKPT = [("transformer_tiny", "MaskGitTransformer"), ("transformer_text_tiny", "MaskGitTransformer"), ("uvit_tiny", "MaskGiTUViT"),
         ("vqgan_tiny", "MaskGitVQGAN"), ("taming_tiny", "VQGANModel")]


def _ckpt_expected(golden_dir, name):
    import json
    import weights as W
    if name == "uvit_tiny":
        g = np.load(os.path.join(golden_dir, "uvit_tiny.npz"))
        return {k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    shapes, seed, kind = {"transformer_tiny": (W.transformer_shapes(W.TRANSFORMER_TINY), 100, "transformer"),
                          "transformer_text_tiny": (W.transformer_shapes(W.TRANSFORMER_TEXT_TINY), 800, "transformer"),
                          "vqgan_tiny": (W.vqgan_shapes(W.VQGAN_CKPT), 300, "vqgan"),
                          "taming_tiny": (W.taming_shapes(W.TAMING_CKPT), 310, "vqgan")}[name]
    return W.fill_state_dict(shapes, seed, kind)


@pytest.mark.parametrize("name,cls_name", _CKPT)
def test_checkpoints_written_by_the_reference_load_here(golden_dir, name, cls_name):
    """tests/golden/ckpt/<name>: config.json + pytorch_model.bin written by the REAL reference's save_pretrained
    (make_golden.py::golden_checkpoints).  This package's from_pretrained reads them: same parameters under the same names, eval mode,
    `_name_or_path` registered, every config key of the file present with its value; and what it saves back is, file for file, what the
    reference wrote (same config.json content, same tensors under the same keys in pytorch_model.bin)"""
    import json
    import muse
    d = os.path.join(golden_dir, "ckpt", name)
    cls = getattr(muse, cls_name)
    m, info = cls.from_pretrained(d, output_loading_info=True)
    assert info["missing_keys"] == [] and info["unexpected_keys"] == [] and info["mismatched_keys"] == []
    want = _ckpt_expected(golden_dir, name)
    sd = m.state_dict()
    written = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(written.keys()) and set(sd.keys()) == set(want.keys())       # the reference's names, in its order
    assert all(torch.equal(sd[k], want[k]) for k in want) and not m.training and m.config._name_or_path == d
    ref_cfg = json.load(open(os.path.join(d, "config.json")))
    for k, v in ref_cfg.items():
        if not k.startswith("_"):
            got = m.config[k]
            assert (list(got) if isinstance(got, (tuple, list)) else got) == v, k
    with tempfile.TemporaryDirectory() as out:
        m.save_pretrained(out)
        assert sorted(os.listdir(out)) == ["config.json", "pytorch_model.bin"]
        mine = json.load(open(os.path.join(out, "config.json")))
        skip = ("_name_or_path",)
        assert {k: v for k, v in mine.items() if k not in skip} == {k: v for k, v in ref_cfg.items() if k not in skip}
        a = torch.load(os.path.join(out, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        b = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        assert list(a.keys()) == list(b.keys()) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name,cls_name", _CKPT)
def test_checkpoints_written_here_load_in_the_reference(golden_dir, name, cls_name, tmp_path):
    """the other direction: a checkpoint written by THIS package's save_pretrained, held against what the real reference's
    from_pretrained needs to load it strictly.  The reference's own save_pretrained output (tests/golden/ckpt/<name>) is its
    model's state dict and every constructor argument of its class: so the file written here must carry the same class name and
    constructor arguments (the reference builds the same model from it) and a state dict with exactly its keys, in its order, with
    its shapes and dtypes (no missing, unexpected or size-mismatched key), holding this package's parameters bit-identically"""
    import json
    import muse
    ref_dir = os.path.join(golden_dir, "ckpt", name)
    cls = getattr(muse, cls_name)
    m = cls.from_pretrained(ref_dir)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.25)                                   # not the bytes the reference wrote
    if hasattr(m, "mark_weights_changed"):
        m.mark_weights_changed()
    d = str(tmp_path / "mine")
    m.save_pretrained(d)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    ref_cfg = json.load(open(os.path.join(ref_dir, "config.json")))
    mine_cfg = json.load(open(os.path.join(d, "config.json")))
    assert mine_cfg["_class_name"] == ref_cfg["_class_name"]
    assert {k: mine_cfg.get(k, "<missing>") for k in ref_cfg if not k.startswith("_")} == {k: v for k, v in ref_cfg.items() if not k.startswith("_")}
    ref_sd = torch.load(os.path.join(ref_dir, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    sd = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(ref_sd.keys()), (list(sd.keys())[:3], list(ref_sd.keys())[:3])
    assert all(sd[k].shape == ref_sd[k].shape and sd[k].dtype == ref_sd[k].dtype for k in ref_sd)
    assert list(want.keys()) == list(sd.keys()) and all(torch.equal(sd[k], want[k]) for k in want)
    assert not all(torch.equal(sd[k], ref_sd[k]) for k in ref_sd)         # (the scaled parameters, not the fixture, were written)


def test_precision_casts_select_the_compute_mode_and_keep_f32_masters(golden_dir):
    """`model.half()` (scripts/benchmark_models.py:33-34), `.to(device, dtype=...)` (pipeline_muse.py:55-64) and
    `from_pretrained(torch_dtype=...)` of the reference cast the parameters; here the masters stay float32 and the cast picks the
    transformers' compute mode (fp16 / bf16 -> bf16 MFMA path, fp32 -> exact f32); the tokenizers ignore it ("keep vae in fp32")"""
    import json
    import muse
    import weights as W
    ucfg = json.load(open(os.path.join(golden_dir, "config_uvit_tiny.json")))
    flat, text, uvit = muse.MaskGitTransformer(**W.TRANSFORMER_TINY), muse.MaskGitTransformer(**W.TRANSFORMER_TEXT_TINY), muse.MaskGiTUViT(**ucfg)
    mode = lambda m: m._resolve_cd() if hasattr(m, "_resolve_cd") else m.compute_dtype      # noqa: E731  ("auto" resolves to f32 outside autocast)
    for m in (flat, text, uvit):
        assert m.half() is m and mode(m) == torch.bfloat16 and all(p.dtype == torch.float32 for p in m.parameters())
        assert m.float() is m and mode(m) == torch.float32
        assert m.bfloat16() is m and mode(m) == torch.bfloat16
        assert m.to(torch.float32) is m and mode(m) == torch.float32
        assert m.to("cpu", dtype=torch.float16) is m and mode(m) == torch.bfloat16
        assert m.to("cpu") is m and mode(m) == torch.bfloat16 and m.dtype == torch.float32        # a pure device move changes nothing
        with tempfile.TemporaryDirectory() as d:
            m.save_pretrained(d)
            assert all(v.dtype == torch.float32 for v in torch.load(os.path.join(d, "pytorch_model.bin"), weights_only=True).values())
            b = type(m).from_pretrained(d, torch_dtype=torch.float16)
            assert mode(b) == torch.bfloat16 and all(p.dtype == torch.float32 for p in b.parameters())
            assert mode(type(m).from_pretrained(d)) == torch.float32
    for v in (muse.MaskGitVQGAN(**W.VQGAN_TINY), muse.VQGANModel(**W.TAMING_TINY)):     # tokenizers: half -> the f32-class "bf16x3" mode
        assert v.half() is v and v.compute_dtype == "bf16x3" and all(p.dtype == torch.float32 for p in v.parameters())
        assert v.float() is v and v.compute_dtype == torch.float32
        assert v.to(dtype=torch.bfloat16) is v and v.compute_dtype == "bf16x3" and all(p.dtype == torch.float32 for p in v.parameters())
        assert v.to("cpu") is v and v.compute_dtype == "bf16x3"


def test_sampling_helpers_vs_reference_golden(golden_dir):
    """muse.sampling's import-surface helpers against the REAL reference module on seeded inputs (tests/golden/sampling_helpers.npz,
    make_golden.py::golden_sampling_helpers): every schedule get_mask_chedule knows (and its keyword form), log with its clamp, top_k,
    gumbel_sample and mask_by_random_topk under seeded CPU generators - exact"""
    from muse import sampling as S
    g = np.load(os.path.join(golden_dir, "sampling_helpers.npz"))
    seed, t = int(g["seed"]), torch.from_numpy(g["t"])
    for method in ("cosine", "linear", "pow0.5", "pow2", "pow3.5", "sigmoid"):
        got, want = S.get_mask_chedule(method)(t), torch.from_numpy(g["schedule." + method])
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-7), method
    assert torch.allclose(S.get_mask_chedule("sigmoid", start=-2, end=4, tau=0.7)(t), torch.from_numpy(g["schedule.sigmoid_kw"]), rtol=1e-6, atol=1e-7)
    assert torch.equal(S.log(torch.from_numpy(g["log.in"])), torch.from_numpy(g["log.out"]))
    logits = torch.from_numpy(g["top_k.in"])
    for thres in (0.9, 0.5, 0.97):
        assert torch.equal(S.top_k(logits, thres), torch.from_numpy(g[f"top_k.{thres}"]))
    assert torch.equal(S.gumbel_sample(logits, temperature=1.0, generator=torch.Generator().manual_seed(seed + 1)), torch.from_numpy(g["gumbel_sample.t1"]))
    assert torch.equal(S.gumbel_sample(logits, temperature=0.0, generator=torch.Generator().manual_seed(seed + 2)), torch.from_numpy(g["gumbel_sample.t0"]))
    got = S.mask_by_random_topk(torch.from_numpy(g["mask.len"]), torch.from_numpy(g["mask.probs"]), temperature=2.0,
                                generator=torch.Generator().manual_seed(seed + 3))
    assert torch.equal(got, torch.from_numpy(g["mask.out"])) and got.sum(-1).tolist() == [1, 7, 15]


def test_lr_schedules_vs_reference_golden(golden_dir):
    """`from muse.lr_schedulers import get_scheduler` (training/train_muse.py:61,512-517): every schedule name of the reference over a
    whole run and past its end, two parameter groups, on muse.FusedAdamW's param_groups - the learning rates the REAL module produced
    (tests/golden/lr_schedules.npz) to the last bit of float64 arithmetic that is order-independent (1e-15 relative); argument errors as
    the reference raises them"""
    import weights as W
    import muse
    from muse.lr_schedulers import SchedulerType, get_scheduler
    g = np.load(os.path.join(golden_dir, "lr_schedules.npz"))
    steps = int(g["steps"])
    for ci, (kind, kw) in enumerate(W.LR_CASES):
        w = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
        opt = muse.FusedAdamW([{"params": [w[0]]}, {"params": [w[1]], "lr": 2.5e-4}], lr=1e-3)
        sched = get_scheduler(kind, opt, **kw)
        got = []
        for _ in range(steps):
            got.append([grp["lr"] for grp in opt.param_groups])
            sched.step()                      # (the optimizer itself has no CPU path: only the schedule is under test here)
        np.testing.assert_allclose(np.asarray(got), g[f"case{ci}"], rtol=1e-15, atol=0, err_msg=kind)
    opt = muse.FusedAdamW([torch.nn.Parameter(torch.zeros(2))], lr=1e-3)
    assert SchedulerType("cosine") is SchedulerType.COSINE
    with pytest.raises(ValueError, match="requires `num_warmup_steps`"):
        get_scheduler("linear", opt)
    with pytest.raises(ValueError, match="requires `num_training_steps`"):
        get_scheduler("cosine", opt, num_warmup_steps=3)
    with pytest.raises(ValueError):
        get_scheduler("not_a_schedule", opt)
    with pytest.raises(ValueError, match="must be be smaller than initial lr"):
        get_scheduler("polynomial", muse.FusedAdamW([torch.nn.Parameter(torch.zeros(2))], lr=1e-8), num_warmup_steps=1, num_training_steps=5)


def test_training_utils_diagnostics_vs_reference_golden(golden_dir):
    """`muse.training_utils` as training/train_muse.py uses it (:50, :1319-1375): the masked-share buckets and the four logging
    diagnostics on the batch of tests/golden/training_utils.npz equal what the REAL reference module returned (bit for bit: the same
    torch reductions on the CPU), including the data frame of token distributions; set_seed seeds `random`, numpy and torch"""
    import random
    from muse import training_utils as TU
    import muse.training_utils                                  # noqa: F401  (the script's import form)
    g = np.load(os.path.join(golden_dir, "training_utils.npz"))
    ids, labels, logits = (torch.from_numpy(g[k]) for k in ("input_ids", "labels", "logits"))
    mask_id = int(g["mask_id"])
    buckets = TU.input_ids_to_masked_buckets(ids, mask_id)
    assert buckets.dtype == torch.long and torch.equal(buckets, torch.from_numpy(g["buckets"])) and sorted(set(buckets.tolist())) == list(range(10))
    assert torch.equal(TU.pixel_entropy_per_percent_masked_bucket(logits.clone(), ids, mask_id), torch.from_numpy(g["pixel_entropy"]))
    assert torch.equal(TU.image_entropy_per_percent_masked_bucket(logits.clone(), ids, mask_id), torch.from_numpy(g["image_entropy"]))
    assert torch.equal(TU.cross_entropy_per_percent_masked_bucket(logits.clone(), labels, ids, mask_id, logits.shape[-1], 0.1),
                       torch.from_numpy(g["cross_entropy"]))
    df = TU.token_probability_distributions_per_percent_masked_bucket(logits.clone(), ids, mask_id)
    assert list(df.columns) == ["bucket", "masked_pixel_prob"]
    assert np.array_equal(df["bucket"].to_numpy(), g["dist.bucket"]) and np.array_equal(df["masked_pixel_prob"].to_numpy().astype(np.float32), g["dist.prob"])
    empty = TU.average_by_buckets(torch.tensor([2.0, 4.0]), torch.tensor([3, 3]), 10)
    assert empty.tolist() == [0, 0, 0, 3.0, 0, 0, 0, 0, 0, 0]
    TU.set_seed(5)
    a = (random.random(), float(np.random.rand()), float(torch.rand(())))
    TU.set_seed(5)
    assert a == (random.random(), float(np.random.rand()), float(torch.rand(())))


def test_the_training_scripts_import_block_resolves():
    """the import statements of training/train_muse.py:49-61 and training/train_maskgit_imagenet.py:37-40, verbatim: every name exists;
    the two tokenizers outside the build refuse to construct instead of being absent at import time"""
    import muse
    import muse.training_utils                                                        # noqa: F401
    from muse import (                                                                # noqa: F401
        MOVQ,
        EMAModel,
        MaskGitTransformer,
        MaskGiTUViT,
        MaskGitVQGAN,
        PaellaVQModel,
        VQGANModel,
        get_mask_chedule,
    )
    from muse.lr_schedulers import get_scheduler                                      # noqa: F401
    from muse.sampling import cosine_schedule                                         # noqa: F401
    from muse import PipelineMuse, PipelineMuseInpainting                             # noqa: F401  (scripts/*.py)
    for cls in (MOVQ, PaellaVQModel):
        with pytest.raises(NotImplementedError, match="not part of the MI355X hot-path build"):
            cls()
        with pytest.raises(NotImplementedError):
            cls.from_pretrained("anything")
    assert muse.__version__ == "0.0.1"

