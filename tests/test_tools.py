"""CPU: the profile-analysis tooling (scripts/overlap_report.py) on a hand-made kernel trace with known overlaps."""
import importlib.util
import io
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("overlap_report", os.path.join(ROOT, "scripts", "overlap_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_overlap_report_interval_arithmetic(tmp_path):
    t = _tool()
    ms = 1_000_000
    # queue 1 / stream 1: two GEMMs [0,4) [5,9); queue 2 / stream 2: a conv [2,7); queue 2 / stream 3: AdamW [8,10); idle nowhere but [4,5) on q1
    rows = [("g256::kernel<a>", 1, 1, 0, 4), ("g256::kernel<b>", 1, 1, 5, 9), ("cslab::conv_slab_kernel(x)", 2, 2, 2, 7),
            ("adamw_kernel(y)", 2, 3, 8, 10)]
    p = tmp_path / "t_kernel_trace.csv"
    with open(p, "w") as f:
        f.write('"Kind","Agent_Id","Queue_Id","Stream_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n')
        for name, q, st, s, e in rows:
            f.write(f'"KERNEL_DISPATCH","Agent 2",{q},{st},"{name}",{s * ms},{e * ms}\n')
    out = io.StringIO()
    r = t.report(t.load(str(p)), out=out)
    assert abs(r["span_ms"] - 10.0) < 1e-9 and r["idle_ms"] == 0.0
    fam = r["families"]
    assert abs(fam["gemm"]["kernel_ms"] - 8.0) < 1e-9 and abs(fam["gemm"]["wall_ms"] - 8.0) < 1e-9
    assert abs(fam["gemm"]["overlapped_ms"] - 5.0) < 1e-9      # conv over [2,4) and [5,7), AdamW over [8,9)
    assert abs(fam["conv"]["overlapped_ms"] - 4.0) < 1e-9 and abs(fam["adamw"]["overlapped_ms"] - 1.0) < 1e-9
    assert r["shared_queues"] == {"2": ["2", "3"]}             # two streams multiplexed onto hardware queue 2
    hist = t.depth_histogram(t.load(str(p)))
    assert hist[1] == 5 * ms and hist[2] == 5 * ms and hist[0] == 0
    assert t.family("void ffn_mid_bwd_kernel<unsigned short, 3, true>") == "rows" and t.family("ncclDevKernel_AllReduce") == "collective"
    # --last-ms keeps only the tail of the trace
    assert len(t.load(str(p), last_ms=2.5)) == 1


def test_attention2_lane_arithmetic_on_cpu():
    """scripts/exp/attn2_emulate.py restates the address formulas of csrc/attention2.hip lane by lane (the row permutation pi, both LDS
    read patterns, the C/D register <-> row map of the 32 x 32 x 16 MFMA, the v_permlane32_swap store packing, the lse / dsum hand-over
    order) on the documented instruction semantics and checks forward and fused backward of one head against float64 attention - and
    that both read patterns are bank-conflict free under the guide's LDS model.  S = 257 (one real row in the 9th block) and 240 (keys
    masked inside the 8th block); the GPU tests (test_one_tile_attention_blocks32) are the parity tests proper."""
    import subprocess
    import sys
    for S in ("257", "240"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "exp", "attn2_emulate.py"), S], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-1500:]
        assert "OK" in out.stdout and "worst multiplicity of a 16-byte slot inside a service group = 1" in out.stdout
        assert "worst multiplicity of a bank inside a 32-lane group = 1" in out.stdout


def test_bf16x3_operand_image_cache_host_logic(monkeypatch):
    """CPU: ops.X3Images (one operand image per tensor and training step) and ops.Planes (a planes-only operand) without a GPU - the split
    is replaced by a counting stand-in.  A tensor is split once however many products read it; a rewritten tensor (version bump) is
    split again; producer-written planes are found without a split; backward-made images live in a short LRU; clear() forgets all;
    outside a step nothing is cached and planes-only results are refused."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
    from muse import ops
    calls = []

    def fake_split(t):
        calls.append(t)
        return torch.zeros((2,) + tuple(t.shape), dtype=torch.bfloat16)
    monkeypatch.setattr(ops, "_split_planes_now", fake_split)
    monkeypatch.setattr(ops, "require_gpu", lambda *a: None)
    a, b = torch.zeros(8, 16), torch.zeros(8, 16)
    ops.split_planes(a); ops.split_planes(a)
    assert len(calls) == 2                                        # no step running: every product splits its own operands
    im = ops.X3Images(recent=2)
    with ops.f32_gemms_as_bf16x3(True, im):
        p1 = ops.split_planes(a)
        assert ops.split_planes(a) is p1 and len(calls) == 3 and (im.hits, im.misses) == (1, 1)
        assert ops.split_planes(b) is not p1 and len(calls) == 4  # same shape, other storage: its own image
        ops._touched(a)                                           # a kernel rewrote a in place
        assert ops.split_planes(a) is not p1 and len(calls) == 5
        made = torch.ones((2, 8, 16), dtype=torch.bfloat16)
        c = torch.zeros(8, 16)
        im.put_planes(c, made)                                    # a producer kernel wrote c's planes itself
        assert ops.split_planes(c) is made and len(calls) == 5 and im.produced == 1
        with ops.f32_gemms_as_bf16x3(False):                      # (the products' own inner scope keeps the step's cache visible)
            assert ops.split_planes(c) is made
        im.backward = True
        g = [torch.zeros(8, 16) for _ in range(3)]
        for t in g:
            ops.split_planes(t)
        assert len(calls) == 8 and len(im.lru) == 2               # the oldest backward image was evicted ...
        ops.split_planes(g[0])
        assert len(calls) == 9                                    # ... and is split again when asked for
        assert ops.split_planes(c) is made                        # forward images stay until the step ends
        im.clear()
        assert not im.persist and not im.lru
    assert ops._PASS.kind is None and ops._PASS.images is None and not ops.planes_only_ok(512, 512)      # no pass is running
    pl = ops.Planes(torch.zeros((2, 256, 128), dtype=torch.bfloat16))
    assert tuple(pl.shape) == (256, 128) and pl.dtype == torch.float32 and pl.stride() == (128, 1) and pl.stride(0) == 128
    assert pl.dim() == 2 and pl.numel() == 256 * 128 and pl.is_contiguous() and ops.split_planes(pl) is pl.planes and len(calls) == 9


def test_f16_mode_host_logic(monkeypatch):
    """CPU: the host side of the "f16" compute mode without a GPU - the cast is a counting stand-in.  One half image per tensor, scale and
    step; a gradient scale must be a power of two (it is undone exactly in alpha); backward images live in a short LRU, and so do a
    tape-less forward's (keep = False: no activation outlives its consumers); a producer's image is found without a cast and carries
    the pass's scale; the default gradient scale is 2^10 x the loss's token rows rounded up to a power of two; the dynamic policy halves
    on overflow (skip the step) and doubles after `growth_interval` good steps."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
    from muse import ops, tape_ops
    from muse._hip import MuseHipError
    casts = []

    def fake_cast(t, scale=1.0, stats=None):
        casts.append((t, scale))
        out = torch.zeros(t.shape, dtype=torch.float16)
        out._muse_scale = float(scale)
        return out
    monkeypatch.setattr(ops, "cast_to_f16", fake_cast)
    monkeypatch.setattr(ops.F16Images, "_ensure_stats", lambda self, device=None: None)
    im = ops.F16Images(recent=2)
    with pytest.raises(MuseHipError):
        im.set_grad_scale(3.0)
    with pytest.raises(MuseHipError):
        im.set_grad_scale(0.0)
    im.set_grad_scale(2.0 ** 19)
    a, b = torch.zeros(8, 16), torch.zeros(8, 16)
    i1 = im.image(a, 1.0)
    assert im.image(a, 1.0) is i1 and len(casts) == 1 and (im.hits, im.misses) == (1, 1)
    assert im.image(a, 2.0 ** 19) is not i1 and len(casts) == 2          # the same tensor as a gradient operand: another image
    assert im.image(b, 1.0) is not i1 and len(casts) == 3
    ops._touched(a)
    assert im.image(a, 1.0) is not i1 and len(casts) == 4                 # rewritten in place: converted again
    w16 = torch.zeros(8, 16, dtype=torch.float16)
    assert im.image(w16, 1.0) is w16 and len(casts) == 4                  # a weight's cached half copy is its own image
    im.backward = True
    made = torch.zeros((1, 8, 16), dtype=torch.float16)
    c = torch.zeros(8, 16)
    im.put_planes(c, made)                                                # a backward producer wrote c's image with the pass's scale
    got = im.image(c, im.grad_scale)
    assert got._muse_scale == 2.0 ** 19 and got.data_ptr() == made.data_ptr() and len(casts) == 4
    for t in [torch.zeros(8, 16) for _ in range(3)]:
        im.image(t, im.grad_scale)
    assert len(im.lru) == 2 and len(im.persist) == 4
    im.clear()
    im.backward, im.keep = False, False                                   # inference forward: nothing persists
    im.image(a, 1.0)
    assert not im.persist and len(im.lru) == 1
    # a planes-only half operand is given its scale: the one the running pass hands its producer kernels
    im.backward = True
    with ops.f32_gemms_as_f16(True, im):
        pl = ops.operand_only(torch.zeros((1, 256, 128), dtype=torch.float16), True)
        assert isinstance(pl, ops.HalfImage) and ops.operand_only(pl.planes, False).scale == 1.0
        assert pl.scale == 2.0 ** 19 and tuple(pl.shape) == (256, 128) and pl.half_image()._muse_scale == 2.0 ** 19
        assert im.image(pl, 1.0).data_ptr() == pl.planes.data_ptr()
        with pytest.raises(MuseHipError):
            im.image(ops.Planes(torch.zeros((2, 256, 128), dtype=torch.bfloat16)), 1.0)
    assert ops._PASS.kind is None and im in ops._F16_GUARDS                # (a backward pass leaves its overflow guard behind)
    ops._F16_GUARDS.discard(im)

    class Host(tape_ops.TapeOps):
        pass
    h = Host()
    assert h.f16_grad_scale_for(16384) == 2.0 ** 24 and h.f16_grad_scale_for(16385) == 2.0 ** 25 and h.f16_grad_scale_for(1) == 1024.0
    h.__dict__["_loss_rows"] = 512
    stats = [(3, 0), (0, 7), (0, 0), (0, 0)]
    monkeypatch.setattr(Host, "f16_stats", lambda self, reset=True: stats.pop(0))
    assert h.f16_update_grad_scale(growth_interval=2) is False and h.f16_grad_scale == 2.0 ** 18      # overflow: halve, skip the step
    assert h.f16_update_grad_scale(growth_interval=2) is True and h.f16_grad_scale == 2.0 ** 18
    assert h.f16_update_grad_scale(growth_interval=2) is True and h.f16_grad_scale == 2.0 ** 19       # two good steps: double
    assert h.f16_update_grad_scale(growth_interval=2) is True and h.f16_grad_scale == 2.0 ** 19


def _ops():
    import sys
    if os.path.join(ROOT, "open-muse_amd") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
    from muse import ops
    return ops


def test_gemm_prologue_and_plain_body_stay_in_step(monkeypatch):
    """CPU: ops.gemm forwards to ops._gemm_plain positionally, so the two parameter lists must be the same names in the same order with
    the same defaults (the leading dimensions, which gemm requires, aside); and a weight gradient of a mixed-dtype pair still goes through
    gemm's prologue, which refuses it - only a bf16 / half pair may skip it."""
    import inspect
    import torch
    ops = _ops()
    from muse._hip import MuseHipError
    pg, pp = inspect.signature(ops.gemm).parameters, inspect.signature(ops._gemm_plain).parameters
    assert list(pg) == list(pp)
    for name in pg:
        if name not in ("lda", "ldb", "ldc"):
            assert pg[name].default == pp[name].default, name
    monkeypatch.setattr(ops, "require_gpu", lambda *a: None)
    monkeypatch.setattr(ops, "_gemm_plain", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a mixed pair reached the launch")))
    dw = torch.zeros(9, 7)                                   # (9 * 7 is no multiple of 4: one product, no split-K plan)
    for dy_dt, x_dt in ((torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16), (torch.float16, torch.bfloat16)):
        with pytest.raises(MuseHipError, match="share a dtype"):
            ops.linear_wgrad(torch.zeros(16, 9, dtype=dy_dt), torch.zeros(16, 7, dtype=x_dt), dw, False)
    with ops.f32_gemms_as_f16(True):                         # (half, f32) in an f16 pass is the prologue's to route or refuse, too
        with pytest.raises(MuseHipError, match="share a dtype"):
            ops.linear_wgrad(torch.zeros(16, 9, dtype=torch.float16), torch.zeros(16, 7), dw, False)


def test_compute_pass_scopes_restore_the_previous_pass():
    """CPU: ops.f32_gemms_as_bf16x3 / f32_gemms_as_f16 set the ONE running pass (ops._PASS) and put the previous one back - also when the
    body raises; on=False of the running mode stops the routing (the step's split cache stays readable), on=False of the other mode
    leaves the running pass alone."""
    ops = _ops()

    def state():
        return ops._PASS.kind, ops._PASS.images
    assert state() == (None, None)
    im = ops.X3Images()
    with ops.f32_gemms_as_bf16x3(True, im):
        assert state() == ("bf16x3", im) and ops._PASS.x3 is im
        with ops.f32_gemms_as_bf16x3(False):
            assert state() == (None, im) and ops._PASS.x3 is im
        assert state() == ("bf16x3", im)
        with ops.f32_gemms_as_f16(False):                      # the other mode's "off" does not touch a running pass
            assert state() == ("bf16x3", im)
        with ops.f32_gemms_as_bf16x3(True):                    # route, do not cache
            assert state() == ("bf16x3", None)
        assert state() == ("bf16x3", im)
    assert state() == (None, None)
    with pytest.raises(KeyError):
        with ops.f32_gemms_as_bf16x3(True, im):
            raise KeyError("inside")
    assert state() == (None, None)
    f16 = ops.F16Images()
    with ops.f32_gemms_as_f16(True, f16):
        assert state() == ("f16", f16) and ops._PASS.x3 is None
        with ops.f32_gemms_as_bf16x3(False):
            assert state() == ("f16", f16)
        with ops.f32_gemms_as_f16(False):
            assert state() == (None, None)
        assert state() == ("f16", f16)
    assert state() == (None, None) and f16 not in ops._F16_GUARDS          # (a forward pass leaves no overflow guard)
    with ops.f32_gemms_as_f16() as scope:                                  # no images given: a private F16Images
        assert isinstance(scope.images, ops.F16Images) and ops._PASS.images is scope.images
    assert state() == (None, None)


def test_operand_only_classes_refuse_the_other_format_and_keep_their_scale():
    """CPU: ops.Planes holds bf16 (hi, lo) planes only, ops.HalfImage one half image and the scale it was GIVEN - also when it is built
    after the pass that wrote it has exited; split_planes refuses a half image."""
    import torch
    ops = _ops()
    from muse._hip import MuseHipError
    half, planes = torch.zeros((1, 256, 128), dtype=torch.float16), torch.zeros((2, 256, 128), dtype=torch.bfloat16)
    with pytest.raises(MuseHipError):
        ops.HalfImage(planes, 1.0)
    with pytest.raises(MuseHipError):
        ops.Planes(half)
    with pytest.raises(MuseHipError):
        ops.split_planes(ops.HalfImage(half, 1.0))
    im = ops.F16Images(grad_scale=2.0 ** 19)
    im.backward = True
    with ops.f32_gemms_as_f16(True, im):
        scale = ops._PASS.scale(True)                          # what _image_args hands the producer kernel
    ops._F16_GUARDS.discard(im)
    hi = ops.HalfImage(half, scale)                            # wrapped after the pass: the scale is the one passed in, not ambient state
    assert ops._PASS.kind is None and hi.scale == 2.0 ** 19 and hi.half_image()._muse_scale == 2.0 ** 19
    assert isinstance(hi, ops.OperandOnly) and isinstance(ops.Planes(planes), ops.OperandOnly) and hi.dtype == torch.float32
    assert tuple(hi.shape) == (256, 128) and hi.stride() == (128, 1) and hi.dim() == 2 and hi.numel() == 256 * 128 and hi.is_contiguous()
    assert isinstance(ops.operand_only(planes, True), ops.Planes)          # no f16 pass running: bf16 planes


def test_image_caches_share_one_store_policy(monkeypatch):
    """CPU: X3Images and F16Images over the same scripted sequence (recent = 2): forward images are kept for the step, backward images -
    a producer's included - go to the short LRU and the oldest is evicted at `recent`, a forward image nobody keeps (F16Images.keep =
    False) goes to the LRU too.  The (persist, lru) sizes and the hit / miss / produced counts are what the two separate classes gave
    before they shared a base."""
    import torch
    ops = _ops()
    monkeypatch.setattr(ops, "_split_planes_now", lambda t: torch.zeros((2,) + tuple(t.shape), dtype=torch.bfloat16))

    def fake_cast(t, scale=1.0, stats=None):
        out = torch.zeros(t.shape, dtype=torch.float16)
        out._muse_scale = float(scale)
        return out
    monkeypatch.setattr(ops, "cast_to_f16", fake_cast)
    monkeypatch.setattr(ops.F16Images, "_ensure_stats", lambda self, device=None: None)

    def script(im, make, made):
        ts = [torch.zeros(8, 16) for _ in range(8)]
        sizes = []
        for t in ts[:3]:
            make(im, t)
        sizes.append((len(im.persist), len(im.lru)))
        im.backward = True
        for t in ts[3:6]:
            make(im, t)
        sizes.append((len(im.persist), len(im.lru)))
        im.put_planes(ts[6], made)
        sizes.append((len(im.persist), len(im.lru)))
        make(im, ts[0])
        make(im, ts[6])
        im.backward = False
        if isinstance(im, ops.F16Images):
            im.keep = False
            make(im, ts[7])
            sizes.append((len(im.persist), len(im.lru)))
        return sizes, (im.hits, im.misses, im.produced)
    assert script(ops.X3Images(recent=2), lambda im, t: im.planes(t), torch.zeros((2, 8, 16), dtype=torch.bfloat16)) \
        == ([(3, 0), (3, 2), (3, 2)], (2, 6, 1))
    assert script(ops.F16Images(recent=2), lambda im, t: im.image(t, im.grad_scale if im.backward else 1.0),
                  torch.zeros((1, 8, 16), dtype=torch.float16)) == ([(3, 0), (3, 2), (3, 2), (3, 2)], (2, 7, 1))


def test_bf16x3_attention_shape_logic_and_step_timeline_on_cpu(tmp_path):
    """host logic added in round 6: which sequence shapes the bf16x3 attention takes in one tile / block by block / not at all
    (ops.attention_x3_supported / attention_x3_blocked), and scripts/step_timeline.py on a synthetic kernel trace (two steps of three
    streams: the per-bin busy shares add up)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))
    from muse import ops
    for sq, skv, ok, blocked in [(256, 256, True, False), (256, 77, True, False), (256, 96, True, False), (256, 128, False, False),
                                 (1024, 1024, True, True), (1024, 77, True, True), (512, 512, True, True), (512, 300, False, True),
                                 (384, 384, False, True), (128, 128, False, False)]:
        assert ops.attention_x3_supported(sq, skv, 64) == ok, (sq, skv)
        assert ops.attention_x3_blocked(sq, skv) == blocked, (sq, skv)
    assert not ops.attention_x3_supported(1024, 1024, 48)
    # a synthetic trace: steps start with mask_sample_kernel on stream 1 every 10 ms; stream 2 busy the first half of each step
    rows = ["Kind,Start_Timestamp,End_Timestamp,Kernel_Name,Queue_Id,Stream_Id"]
    for st in range(4):
        t0 = st * 10_000_000
        rows.append(f'KERNEL_DISPATCH,{t0},{t0 + 50_000},"mask_sample_kernel(long)",1,1')
        rows.append(f'KERNEL_DISPATCH,{t0 + 100_000},{t0 + 9_900_000},"void g256p::kernel<unsigned short, 0, 0>(g256p::PArgs)",1,1')
        rows.append(f'KERNEL_DISPATCH,{t0},{t0 + 5_000_000},"void cslab::conv_slab_kernel<true>(cdma::Params)",2,2')
    trace = tmp_path / "t_kernel_trace.csv"
    trace.write_text("\n".join(rows) + "\n")
    spec = importlib.util.spec_from_file_location("step_timeline", os.path.join(ROOT, "scripts", "step_timeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old_argv, old_out = sys.argv, sys.stdout
    sys.argv, sys.stdout = ["step_timeline.py", str(trace), "--dump", str(tmp_path / "step.csv")], io.StringIO()
    try:
        mod.main()
        out = sys.stdout.getvalue()
    finally:
        sys.argv, sys.stdout = old_argv, old_out
    assert "step of 10.00 ms" in out and "gemmNN" in out and "conv" in out
    lines = [l for l in out.splitlines() if " ms | " in l]
    assert len(lines) >= 10 and lines[2].split("|")[2].strip().startswith("1.00") and lines[7].split("|")[2].strip().startswith("0.00")
    assert (tmp_path / "step.csv").read_text().count("\n") >= 3


def test_kernel_digest_parser_on_a_synthetic_listing():
    """scripts/kernel_digest.py: kernels only (.amdhsa_kernel), instructions counted without labels / directives / comments, figures from the
    '; Kernel info' block, and a digest that ignores comments and the function number of local labels but not an instruction or its order;
    the body digest starts at the first local label, so it ignores the set-up code before it, and is the whole digest without a label"""
    spec = importlib.util.spec_from_file_location("kernel_digest", os.path.join(ROOT, "scripts", "kernel_digest.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)

    def listing(fn, body):
        return f"""\t.text
\t.globl\t_Z1kv
_Z1kv:                                  ; @_Z1kv
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0       ; a comment
{body}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z1kv
\t\t.amdhsa_next_free_vgpr 7
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\t_Z1kv, .Lfunc_end{fn}-_Z1kv
; Kernel info:
; codeLenInByte = 40
; TotalNumSgprs: 12
; NumVgprs: 7
; ScratchSize: 16
; Occupancy: 8
_Z6helperv:
\tv_mov_b32_e32 v0, 0
\ts_setpc_b64 s[30:31]
.Lfunc_end{fn + 1}:
; NumVgprs: 99
"""
    loop = lambda fn, a, b: f"\ts_cmp_lt_i32 s0, 1\n\ts_cbranch_scc1 .LBB{fn}_2\n.LBB{fn}_1:   ; loop\n\t{a}\n\t{b}\n.LBB{fn}_2:"
    k, = kd.parse(listing(0, loop(0, "v_add_u32_e32 v1, v0, v0", "v_mul_lo_u32 v2, v1, v1")))
    assert k["name"] == "_Z1kv" and k["insts"] == 6                      # (the device function is no kernel; labels are no instructions)
    assert (k["vgprs"], k["sgprs"], k["scratch"], k["occupancy"]) == (7, 12, 16, 8)
    same, = kd.parse(listing(3, loop(3, "v_add_u32_e32   v1, v0, v0 ; other comment", "v_mul_lo_u32 v2, v1, v1")))
    assert same["digest"] == k["digest"]                                 # another function number, spacing, comments
    swapped, = kd.parse(listing(0, loop(0, "v_mul_lo_u32 v2, v1, v1", "v_add_u32_e32 v1, v0, v0")))
    renamed, = kd.parse(listing(0, loop(0, "v_add_u32_e32 v1, v0, v0", "v_mul_lo_u32 v3, v1, v1")))
    assert swapped["insts"] == 6 and len({k["digest"], swapped["digest"], renamed["digest"]}) == 3
    assert len({k["body"], swapped["body"], renamed["body"]}) == 3 and k["body"] != k["digest"] and same["body"] == k["body"]
    setup = lambda fn, a, b: f"\t{a}\n\t{b}\n" + loop(fn, "v_add_u32_e32 v1, v0, v0", "v_mul_lo_u32 v2, v1, v1")
    one, = kd.parse(listing(0, setup(0, "s_mov_b32 s1, 0", "s_mov_b32 s2, 1")))
    two, = kd.parse(listing(5, setup(5, "s_mov_b32 s2, 1", "s_mov_b32 s1, 0")))
    assert one["body"] == two["body"] == k["body"] and one["digest"] != two["digest"]   # they differ only before the first label
    flat, = kd.parse(listing(0, "\tv_add_u32_e32 v1, v0, v0"))
    assert flat["insts"] == 3 and flat["body"] == flat["digest"]                          # no label: one digest
