"""Thin Python wrappers over the libmuse_hip C-ABI (one function per kernel entry point, no autograd here).

Tensors are allocated by PyTorch; every wrapper enqueues on torch's current HIP stream.  All of them raise
MuseHipError if the tensors are not on the GPU or the native library is missing: there is no eager fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import weakref

import torch

from . import _hip
from ._hip import BF16, F16, F32, GemmDesc, check, dt, lib, ptr, require_gpu, stream

# MUSE_GEMM_TR=0 routes k-major GEMM operands through an explicit transpose + the k-contiguous path instead of the
# ds_read_b64_tr_b16 path (debug / bring-up switch; both run on the GPU through libmuse_hip).
USE_TR = os.environ.get("MUSE_GEMM_TR", "1") != "0"


def _esz(t):
    return t.element_size()


# ---- optional per-launch timing of the MFMA kernels (bench.py's roofline leg): HIP events on the launch stream ----------
_PROF = None


PROF_BYTES = {}   # kernel family -> algorithmic HBM bytes of the instrumented launches (each operand read / written once)


def profile_start():
    global _PROF
    _PROF = []
    PROF_BYTES.clear()


def profile_stop(with_kind=False):
    """-> list of (kernel name, algorithmic work, milliseconds) per launch; work = flops for the MFMA kernels.  with_kind adds
    the HBM-bound kernels (work = algorithmic bytes: every operand read or written once) and a 4th field "flop" | "byte"."""
    global _PROF
    rec, _PROF = _PROF, None
    torch.cuda.synchronize()
    out = [(n, f, e0.elapsed_time(e1), k) for n, f, e0, e1, k in rec]
    return out if with_kind else [(n, f, t) for n, f, t, k in out if k == "flop"]


def _prof_begin():
    if _PROF is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _prof_end(e0, name, work, kind="flop"):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        _PROF.append((name, work, e0, e1, kind))


def _touched(t):
    """a HIP kernel of this package just rewrote t through its raw pointer: bump autograd's version counter, the way a torch in-place
    op would - X3Images keys a tensor's cached operand planes by (storage, shape, version), so a rewritten tensor never finds the planes
    of its previous contents"""
    torch.autograd.graph.increment_version(t)
    return t


def _nbytes(*tensors):
    return float(sum(t.numel() * t.element_size() for t in tensors if t is not None))


def capture_graph(fn):
    """Run fn() once eagerly (one-time packing / first-use work stays out of the graph), then capture a second run into a
    HIP graph: every libmuse_hip launch inside goes to torch's capture stream (`stream()` is torch's current stream) and the
    tensors fn allocates come from the graph's private pool.  -> (graph, fn's captured return value); graph.replay() re-runs
    it on the inputs' current contents."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


SKINNY = int(os.environ.get("MUSE_GEMM_SKINNY", "1"))   # split-K + fused reduction for forward products of <= 2048 rows: 1 = inside graph capture


def gemm(A, B, C_, M, N, K, *, la=0, lb=0, lda, ldb, ldc, a_off=0, b_off=0, c_off=0, alpha=1.0, bias=None, rowvec=None,
         residual=None, ldr=0, batch=1, zdiv=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), accumulate=False, act=0, split_k=1,
         split_stride=0, x3_lo=None):
    """C[z] = epilogue(alpha * A[z] @ B[z]^T).  A/B/C_ are tensors, *_off element offsets of the (0,0) entry.

    la/lb = 0: operand(r,k) at base + r*ld + k;  1: at base + k*ld + r (see include/muse_hip.h).
    x3_lo = (a_lo, b_lo): A / B are the bf16 hi planes of a bf16x3 product, their lo planes that many elements behind them
    (muse_gemm_x3); returns None when that kernel does not take the product.

    Here: the mode prologue - an f32 product of a running "f16" / "bf16x3" pass (GemmPass) goes to that mode's route; the rest is _gemm_plain.
    """
    require_gpu(A, B, C_)
    kind = _PASS.kind
    if (kind == "f16" and C_.dtype == torch.float32 and (A.dtype, B.dtype) in _F16_MODE_PAIRS and act == 0 and split_k == 1 and batch == 1
            and _gemm_f16(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, c_off, alpha, bias, rowvec, residual, ldr, accumulate, a_off, b_off)):
        return C_
    if A.dtype != B.dtype:
        raise _hip.MuseHipError("gemm operands must share a dtype")
    if (kind == "bf16x3" and A.dtype == torch.float32 and C_.dtype == torch.float32 and act == 0 and split_k == 1
            and _gemm_bf16x3(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, a_off, b_off, c_off, alpha, bias, rowvec, residual, ldr, batch, zdiv,
                             sA, sB, sC, accumulate)):
        return C_
    if isinstance(A, OperandOnly) or isinstance(B, OperandOnly):
        # an operand-only object has no f32 bytes behind data_ptr(): every path below would read its image as something else
        raise _hip.MuseHipError("a planes-only operand reached a product the four-plane kernel does not take")
    return _gemm_plain(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, a_off, b_off, c_off, alpha, bias, rowvec, residual, ldr, batch, zdiv, sA, sB, sC,
                       accumulate, act, split_k, split_stride, x3_lo)      # (positional: this hop is on every product's host path)


def _gemm_plain(A, B, C_, M, N, K, la=0, lb=0, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c_off=0, alpha=1.0, bias=None, rowvec=None,
                residual=None, ldr=0, batch=1, zdiv=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), accumulate=False, act=0, split_k=1,
                split_stride=0, x3_lo=None):
    """gemm() on the operands as they are, whatever pass is running: the skinny split-K of a captured forward, the bring-up transpose
    route, or one muse_gemm / muse_gemm_x3 launch"""
    if (SKINNY and x3_lo is None and A.dtype == torch.bfloat16 and batch == 1 and la == 0 and lb == 0 and act == 0 and rowvec is None and not accumulate
            and split_k == 1 and M <= 2048 and K >= 512 and N % 4 == 0 and ldc % 4 == 0 and (residual is None or ldr % 4 == 0)
            and (SKINNY == 2 or torch.cuda.is_current_stream_capturing())):
        # small-batch decoding: a forward Linear of a few hundred rows has too few 128^2 tiles for 256 CUs ([512 x 1024] x [1024 x 1024]^T:
        # 32 tiles, 36 us of a 16-K-tile loop on an eighth of the chip; 77 % of a 512-row U-ViT forward was such launches,
        # profiles/r04_decode_kernel_stats_before.csv).  K is cut so that tiles x slices fill the chip (>= 2 K-tiles per slice), the
        # slices go to an f32 workspace and ONE row kernel sums them in fixed order and applies the Linear's epilogue (bias, residual,
        # output dtype).  Only while the forward is being CAPTURED into a HIP graph (generate2(hip_graph=True), PipelineMuse): the path
        # trades kernel time for launches (+36 % launches), and an eager small-batch forward is bound by per-launch host time - measured
        # on MI355X, PipelineMuse at batch 1 (profiles/r04_latency_ab.txt): eager 123.5 ms, eager + split-K 152.3, graph 112.2,
        # graph + split-K 98.9.  (MUSE_GEMM_SKINNY=2 forces it everywhere, 0 turns it off.)
        t128 = ((M + 127) // 128) * ((N + 127) // 128)
        sk = min(256 // t128, K // 128, 16) if t128 <= 96 else 1
        if sk >= 2:
            # the kernels cut K on 64-wide tile boundaries, ceil(nk / sk) tiles per slice: a slice that starts at or beyond nk returns
            # without writing its part of the workspace, so only the slices that hold work may be summed (M=256, K=2816: 16 -> 15)
            nk = (K + 63) // 64
            per = (nk + sk - 1) // sk
            sk = (nk + per - 1) // per
        if sk >= 2:
            ws = torch.empty((sk, M, N), dtype=torch.float32, device=A.device)
            _gemm_plain(A, B, ws, M, N, K, la=0, lb=0, lda=lda, ldb=ldb, ldc=N, a_off=a_off, b_off=b_off, alpha=alpha, split_k=sk, split_stride=M * N)
            check(lib().muse_sum_slices_epilogue(ws.data_ptr(), sk, M * N, ptr(bias), ptr(residual), ldr, C_.data_ptr() + c_off * _esz(C_),
                                                 dt(C_), ldc, M, N, stream()), "muse_sum_slices_epilogue")
            return _touched(C_)
    # (Measured and dropped, round 5: the ragged last row tile of M = 16448 as a launch of its own wherever it saves a round of the
    #  256-CU chip - N = 6144 / 3072 / 2048: the step came out 0.45 ms SLOWER, 53.08 against 52.64 ms same box, transformer alone 33.34
    #  against 32.85: the extra launches cost more than the rounds, and in the step other streams fill the tail anyway.)
    if not USE_TR and A.dtype == torch.bfloat16 and (la == 1 or lb == 1):
        if x3_lo is not None:
            return None        # (the bring-up transpose route would drop the lo planes: the caller falls back to its three-product form)
        return _gemm_via_transpose(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, a_off, b_off, c_off, alpha, bias, rowvec,
                                   residual, ldr, batch, zdiv, sA, sB, sC, accumulate, act)
    d = GemmDesc()
    d.A = A.data_ptr() + a_off * _esz(A)
    d.B = B.data_ptr() + b_off * _esz(B)
    d.C = C_.data_ptr() + c_off * _esz(C_)
    d.bias = ptr(bias)
    d.rowvec = ptr(rowvec)
    d.residual = ptr(residual)
    d.dtype = F16 if A.dtype == torch.float16 else dt(A)
    d.out_dtype = dt(C_)
    d.layout_a, d.layout_b = la, lb
    d.M, d.N, d.K = M, N, K
    d.batch, d.zdiv = batch, zdiv
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.sA0, d.sA1 = sA
    d.sB0, d.sB1 = sB
    d.sC0, d.sC1 = sC
    # (half operand images carry the power of two they were scaled by: the product is handed back unscaled)
    d.alpha = alpha / (getattr(A, "_muse_scale", 1.0) * getattr(B, "_muse_scale", 1.0)) if d.dtype == F16 else alpha
    d.accumulate = 1 if accumulate else 0
    d.act = act
    d.split_k = split_k
    d.split_stride = split_stride
    e0 = _prof_begin()
    if x3_lo is not None:
        rc = lib().muse_gemm_x3(C.byref(d), int(x3_lo[0]), int(x3_lo[1]), stream())
        if rc == -3:         # MUSE_ERR_UNSUPPORTED: a shape the four-plane kernel does not take
            return None
        check(rc, "muse_gemm_x3")
        _prof_end(e0, f"gemm_bf16x3_{'NT'[la]}{'NT'[lb]}", 2.0 * M * N * K * batch)
        return _touched(C_)
    check(lib().muse_gemm(C.byref(d), stream()), "muse_gemm")
    _prof_end(e0, f"gemm_{ {BF16: 'bf16', F16: 'f16'}.get(d.dtype, 'f32')}_{'NT'[la]}{'NT'[lb]}", 2.0 * M * N * K * batch)
    return _touched(C_)


# ---- the compute pass: how the f32 products of the forward / backward pass that is running are computed --------------------------------
# Exact f32 (no pass), "bf16x3" or "f16" (the two sections below).  _PASS is the ONE place that knows: gemm() / linear_wgrad() ask it for
# the route, the producer kernels' wrappers for the operand-image format, scale and cache, split_planes / split_cat3 for the split cache.
class GemmPass:
    """kind: None | "bf16x3" | "f16"; images: the operand-image cache of the step - an X3Images or None ("bf16x3": None = route, do not
    cache), an F16Images ("f16": always one)"""

    def __init__(self, kind=None, images=None):
        self.kind, self.images = kind, images
        self.x3 = None if kind == "f16" else images        # the split cache split_planes / split_cat3 go through
        # the operand-image tensor a producer kernel writes (planes_alloc): ONE IEEE-half image [1, r, c], or (hi, lo) bf16 planes [2, r, c]
        self.image_planes, self.image_dtype = (1, torch.float16) if kind == "f16" else (2, torch.bfloat16)

    def scale(self, gradient):
        """the power of two a producer kernel applies to its image: the pass's gradient scale for a backward result of an "f16" pass"""
        return self.images.grad_scale if (gradient and self.kind == "f16") else 1.0

    def producing(self):
        """the cache a producer kernel's operand image goes to, None when it should write none"""
        return self.images if (F16_PRODUCERS if self.kind == "f16" else X3_NATIVE and X3_PRODUCERS) else None


_PASS = GemmPass()


class _PassScope:
    """makes a GemmPass the running one for a `with` body; the previous pass is back on exit (also when the body raises).  There is one
    slot: an inner scope wins, so an on=True scope of one mode inside a pass of the other REPLACES that pass for its body (no caller
    nests them).  on=False switches this mode's routing off - a bf16x3 step's split cache stays readable - and leaves a pass of the
    other mode alone."""

    def __init__(self, kind, on, images):
        self.kind, self.on, self.images = kind, bool(on), images

    def __enter__(self):
        global _PASS
        self.prev = _PASS
        if self.on:
            _PASS = GemmPass(self.kind, self.images)
        elif _PASS.kind == self.kind:
            _PASS = GemmPass(None, _PASS.x3)
        return self

    def __exit__(self, *exc):
        global _PASS
        _PASS = self.prev
        if self.on and self.kind == "f16" and self.images.backward:
            _F16_GUARDS.add(self.images)         # (the owner's optimizer step that follows skips its update if this pass overflowed)
        return False


def f32_gemms_as_bf16x3(on=True, images=None):
    """`images`: an X3Images to share operand images between the products of a step (None: every product splits its operands)"""
    return _PassScope("bf16x3", on, images)


def f32_gemms_as_f16(on=True, images=None):
    """`images`: the F16Images of the step (None: a private one - every product converts its operands)"""
    return _PassScope("f16", on, images if images is not None else (F16Images() if on else None))


class _ImageCache:
    """What the two modes' operand-image caches share: entries keyed by (storage address, shape, strides, autograd version, form) that
    hold their source tensor - so an address cannot come back with other contents while the entry exists, and the wrappers of kernels
    that rewrite a tensor in place bump its version (`_touched`) - in `persist` until the owner's clear(), or in a short LRU of `recent`
    entries: the images a backward pass makes are dead two products later, and so are those of a forward nobody keeps (`keep`)."""
    keep = True

    def __init__(self, recent=12):
        self.persist, self.lru, self.recent, self.backward = {}, {}, int(recent), False
        self.hits = self.misses = self.produced = 0

    def clear(self):
        self.persist.clear()
        self.lru.clear()

    @staticmethod
    def _key(t, *form):
        return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version) + form

    def _find(self, key):
        hit = self.persist.get(key)
        if hit is None:
            hit = self.lru.get(key)
        if hit is None:
            self.misses += 1
        else:
            self.hits += 1
        return hit

    def _store(self, key, entry, short=False):
        if short or self.backward or not self.keep:
            self.lru[key] = entry
            while len(self.lru) > self.recent:
                self.lru.pop(next(iter(self.lru)))
        else:
            self.persist[key] = entry


class OperandOnly:
    """An f32-class GEMM operand that exists ONLY as the operand image a producer kernel wrote - the result of a kernel that nothing but
    weight GEMMs reads (the GLU output and its input gradient inside an MLP, planes_only=True): the f32 tensor is never written.
    Quacks like the contiguous f32 [rows, cols] tensor it stands for as far as the GEMM entry points look (shape, dtype, strides); the
    products that take it are its mode's (Planes: muse_gemm_x3, HalfImage: the half kernels) - anything else raises instead of reading
    bytes that are not there."""
    dtype = torch.float32
    is_cuda = True
    _version = 0

    def __init__(self, planes):
        if planes.dtype != self.image_dtype:
            raise _hip.MuseHipError(f"{type(self).__name__} holds {self.image_dtype} images, got {planes.dtype}")
        self.planes = planes
        self.shape = torch.Size(planes.shape[1:])
        self.device = planes.device

    def dim(self):
        return 2

    def numel(self):
        return self.shape[0] * self.shape[1]

    def stride(self, i=None):
        st = (self.shape[1], 1)
        return st if i is None else st[i]

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.planes.data_ptr()      # (only ever probed for alignment)

    def record_stream(self, s):
        self.planes.record_stream(s)


class Planes(OperandOnly):
    """"bf16x3" mode: the (hi, lo) bf16 planes [2, rows, cols]"""
    image_dtype = torch.bfloat16


class HalfImage(OperandOnly):
    """"f16" mode: ONE IEEE-half image [1, rows, cols] = half(x * scale), `scale` the power of two the producer kernel was GIVEN
    (_image_args: the pass's gradient scale for a backward result, 1 for a forward one) - handed in by whoever launched it"""
    image_dtype = torch.float16

    def __init__(self, planes, scale):
        super().__init__(planes)
        self.scale = float(scale)

    def half_image(self):
        t = self.planes[0]
        t._muse_scale = self.scale
        return t


def operand_only(planes, gradient):
    """the operand-only result of a producer kernel of the running pass: `planes` is the tensor it has just written (planes_alloc) with
    the (half, scale) of _image_args(gradient, planes)"""
    return HalfImage(planes, _PASS.scale(gradient)) if _PASS.kind == "f16" else Planes(planes)


# ---- "f16": every f32 weight GEMM as ONE product of IEEE-half operand images ----------------------------------------------------------
# configs/cc12m_uvit_clip.yaml:102-103 trains f32 tensors with `enable_tf32`: the products round their operands to TF32 (10-bit mantissa,
# 8-bit exponent) and accumulate in f32.  gfx950 has no xf32 MFMA; IEEE half has the SAME 10-bit mantissa, and its MFMA
# (v_mfma_f32_16x16x32_f16, f32 accumulation) runs at the bf16 rate - a third of the "bf16x3" mode's cost for the operand precision the
# YAML asks for.  What half lacks is TF32's exponent range, which is the host's job here: an operand image is half(x * s) with s a power
# of two (exact) and the product's alpha carries 1 / (s_a s_b).  Forward operands (normalised activations, weights) use s = 1; every
# GRADIENT operand of a backward pass uses the pass's `grad_scale` (per-token loss gradients are ~1 / tokens: far below half's normal
# range unscaled).  A finite element beyond +-65504 / s becomes inf - the product and the step's gradients turn NaN rather than silently
# wrong - and is counted (F16Images.stats()[0]): the cast kernel counts every ELEMENT whose half is inf or NaN (an input that already was
# one included), the producer kernels (common.h store_image4) every 4-element GROUP that holds one; the cast kernel also counts the
# finite non-zero elements it rounds to +-0 ([1]).  The fp16-training recipe applies on top: TapeOps.f16_update_grad_scale() halves the
# scale and has the caller skip the step, or muse.FusedAdamW skips it on the device.  Products the 256^2 half kernels refuse stay in exact f32.
# Scoped by f32_gemms_as_f16 (a GemmPass of kind "f16" whose images are the step's F16Images).
# the F16Images of f16 BACKWARD passes whose overflow counter no optimizer step has consumed yet: muse.FusedAdamW guards its update
# with the counter of a pass of the model whose parameters it steps (F16Images.owner) - never with another model's
_F16_GUARDS = weakref.WeakSet()
# operand dtypes of a product the mode converts: f32 tensors, or an f32 tensor against an operand that already IS a half image (a
# weight's copy kept across steps: tape_ops._wb)
_F16_MODE_PAIRS = {(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float16, torch.float32)}


class F16Images(_ImageCache):
    """The half operand images of ONE training step (the role X3Images plays for the bf16x3 mode): a tensor is converted once per step and
    scale, whichever products read it (the key's form is the scale).  `backward`: the pass running is a backward pass - the A operand of
    its products and the dy of its weight gradients are gradients and take `grad_scale`.  `keep` (forward passes): the backward pass reads
    the images again; a forward that records no tape (inference) sets it False, so no activation outlives its consumers."""

    def __init__(self, grad_scale=1.0, recent=12):
        super().__init__(recent)
        self.grad_scale = float(grad_scale)
        self._stats = None
        self._snaps, self._free, self.totals = [], [], [0, 0]      # counter copies in flight (pinned buffer, event), free ones, running totals
        self.owner = None      # weakref to the model whose passes these are (the optimizer steps that honour its overflow guard)

    def set_grad_scale(self, s):
        if s <= 0 or math.frexp(float(s))[0] != 0.5:
            raise _hip.MuseHipError(f"f16 mode: the gradient scale must be a power of two, got {s}")
        self.grad_scale = float(s)

    def _ensure_stats(self, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        if self._stats is None or self._stats.device != device:
            self._stats = torch.zeros(2, dtype=torch.int32, device=device)
        return self._stats

    def stats(self, reset=True):
        """(operand images with an inf / NaN half - elements of a cast, 4-element groups of a producer kernel -, finite non-zero
        elements a cast rounded to +-0) since the last reset - one device read (plus what optimizer steps have already taken off the
        device counters: after_optimizer_step)"""
        self.consume_snapshots(block=True)
        v = [0, 0] if self._stats is None else self._stats.tolist()
        out = (int(v[0]) + self.totals[0], int(v[1]) + self.totals[1])
        if reset:
            if self._stats is not None:
                self._stats.zero_()
            self.totals = [0, 0]
        return out

    def after_optimizer_step(self):
        """muse.FusedAdamW has launched its update guarded by this pass's overflow counter: take the counters off the device - copied
        to pinned memory behind the update, zeroed behind the copy (all stream-ordered, no host wait) - for the next backward pass,
        which reads the copies that have arrived (consume_snapshots) to move the gradient scale"""
        if self._stats is None:
            return
        buf, ev = self._free.pop() if self._free else (torch.zeros(2, dtype=torch.int32).pin_memory(), torch.cuda.Event())
        buf.copy_(self._stats, non_blocking=True)
        ev.record(torch.cuda.current_stream(self._stats.device))
        self._stats.zero_()
        self._snaps.append((buf, ev))

    def consume_snapshots(self, block=False):
        """-> [(overflowed, rounded to zero), ...] of the guarded optimizer steps whose counter copies have ARRIVED, oldest first.  Never
        waits unless `block`: the host enqueues a step or more ahead of the GPU, and waiting here for the previous step's copy would
        cost that run-ahead (measured: 648 -> 596 images/s on the config-4 leg) - a copy still in flight is read by a later pass."""
        out = []
        while self._snaps:
            buf, ev = self._snaps[0]
            if block:
                ev.synchronize()
            elif not ev.query():
                break
            self._snaps.pop(0)
            v = buf.tolist()
            self._free.append((buf, ev))
            self.totals[0] += int(v[0])
            self.totals[1] += int(v[1])
            out.append((int(v[0]), int(v[1])))
        return out

    def image(self, t, scale):
        if isinstance(t, OperandOnly):     # a producer's result that exists as its half image only
            if not isinstance(t, HalfImage):
                raise _hip.MuseHipError("a bf16x3 planes-only operand reached a half product")
            return t.half_image()
        if t.dtype == torch.float16:       # already an image (a weight's half copy): its own scale rides on it
            return t
        key = self._key(t, float(scale))
        hit = self._find(key)
        if hit is not None:
            return hit[1]
        out = cast_to_f16(t, scale, self._ensure_stats(t.device))
        self._store(key, (t, out))
        return out

    def put_planes(self, t, planes):
        """a producer kernel wrote t's half image itself ([1, *t.shape], the bits muse_cast_f32_to_f16 makes of t with the scale the
        kernel was given: the pass's gradient scale in a backward pass, 1 in a forward one): no cast pass when a product reads t"""
        scale = self.grad_scale if self.backward else 1.0
        img = planes[0]
        img._muse_scale = scale
        self.produced += 1
        self._store(self._key(t, float(scale)), (t, img))


def _image_args(gradient, *planes):
    """(half, scale, stats) of a producer entry point (*_x3) in the running pass: half = 1 in an "f16" pass (the kernel writes ONE IEEE-half
    image, and the x3 attention kernels compute in half), scale = the pass's gradient scale for a backward result (`gradient`), 1 for a
    forward one, stats = the pass's overflow counter.  A plane tensor given must have the mode's dtype (half: float16, else bfloat16)."""
    half = _PASS.kind == "f16"
    for p in planes:
        if p is not None and p.dtype != _PASS.image_dtype:
            raise _hip.MuseHipError(f"operand image of dtype {p.dtype} in a{'n f16' if half else ' bf16x3'} pass")
    return (1, _PASS.scale(gradient), _PASS.images._ensure_stats().data_ptr()) if half else (0, 1.0, None)


def cast_to_f16(t, scale=1.0, stats=None):
    """half(t * scale) of a contiguous f32 tensor (muse_cast_f32_to_f16); the image remembers its scale (`_muse_scale`: gemm divides alpha
    by it)"""
    require_gpu(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _hip.MuseHipError("cast_to_f16: contiguous f32 tensor")
    out = torch.empty(t.shape, dtype=torch.float16, device=t.device)
    check(lib().muse_cast_f32_to_f16(t.data_ptr(), out.data_ptr(), t.numel(), float(scale), ptr(stats), stream()), "muse_cast_f32_to_f16")
    out._muse_scale = float(scale)
    return out


def _f16_operands_ok(A, B, M, N, K, la, lb, lda, ldb):
    """whole contiguous 2-D f32 tensors read as [rows, K] / [K, rows] operands with 16-byte half rows (what an image can stand for)"""
    return (A.dim() == 2 and B.dim() == 2 and A.is_contiguous() and B.is_contiguous() and K % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0
            and A.stride(0) == lda and B.stride(0) == ldb and A.shape[1 if la == 0 else 0] == K and B.shape[1 if lb == 0 else 0] == K
            and A.shape[0 if la == 0 else 1] >= M and B.shape[0 if lb == 0 else 1] >= N and M >= 128 and N >= 128 and K >= 64
            and A.numel() * 2 < (1 << 31) and B.numel() * 2 < (1 << 31))


def _f16_kernel_takes(A, B, c_ptr, M, N, K, la, lb, lda, ldb, ldc, residual=None, ldr=0):
    d = GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), c_ptr           # (the f32 tensors' addresses stand in for their images': alignment probe)
    d.dtype, d.out_dtype, d.layout_a, d.layout_b = F16, F32, la, lb
    d.M, d.N, d.K, d.batch, d.zdiv = M, N, K, 1, 1
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.residual = ptr(residual)
    d.alpha = 1.0
    return lib().muse_gemm_tile(C.byref(d)) == 256


def _gemm_f16(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, c_off, alpha, bias, rowvec, residual, ldr, accumulate, a_off, b_off):
    """-> True when the product ran on half operand images, False when the half kernels do not take it (it then runs in exact f32)"""
    if a_off or b_off or not _f16_operands_ok(A, B, M, N, K, la, lb, lda, ldb):
        return False
    if not _f16_kernel_takes(A, B, C_.data_ptr() + c_off * 4, M, N, K, la, lb, lda, ldb, ldc, residual, ldr):
        return False
    im = _PASS.images
    a16 = im.image(A, im.grad_scale if im.backward else 1.0)
    b16 = im.image(B, 1.0)
    _gemm_plain(a16, b16, C_, M, N, K, la=la, lb=lb, lda=lda, ldb=ldb, ldc=ldc, c_off=c_off, alpha=alpha, bias=bias, rowvec=rowvec,
                residual=residual, ldr=ldr, accumulate=accumulate)
    return True


def f16_wgrad_operands(dy, x, M=None, lda=None):
    """the half images (dy with the pass's gradient scale, x unscaled) of a weight-gradient product dy^T x the half kernels take, through
    the running step's image cache - or None (no f16 step running / a shape they refuse: the caller keeps the f32 tensors)"""
    if not (_PASS.kind == "f16" and dy.dtype == torch.float32 and x.dtype == torch.float32 and dy.dim() == 2 and x.dim() == 2
            and (lda is None or lda == dy.stride(0)) and dy.shape[0] == x.shape[0]):
        return None
    N = M if M is not None else dy.shape[1]
    if not (_f16_operands_ok(dy, x, N, x.shape[1], dy.shape[0], 1, 1, dy.stride(0), x.stride(0))
            and _f16_kernel_takes(dy, x, dy.data_ptr(), N, x.shape[1], dy.shape[0], 1, 1, dy.stride(0), x.stride(0), x.shape[1])):
        return None
    im = _PASS.images
    return im.image(dy, im.grad_scale), im.image(x, 1.0)


# ---- "bf16x3": every f32 GEMM as three bf16 MFMA products ---------------------------------------------------------------------------
# The exact-f32 parity mode of the tape engines (MaskGiTUViT, text-conditioned MaskGitTransformer) runs its GEMMs on the f32-input MFMA
# (157 TFLOP/s peak).  configs/cc12m_uvit_clip.yaml:102-103 trains in f32 tensors with TF32 products (10-bit mantissa); gfx950 has no
# xf32 MFMA, the CDNA4 counterpart at or above that precision is the three-product scheme the tokenizer already uses: operands split
# into hi = bf16(x), lo = bf16(x - hi), C = hi*hi + hi*lo + lo*hi with f32 accumulation (the dropped lo*lo term is 2^-16 relative) on
# the bf16 kernels at 1/3 of their rate.  Scoped by f32_gemms_as_bf16x3, which the models enter for "bf16x3" compute (a GemmPass of that
# kind; its images are the step's X3Images, or None); a product the bf16 kernels cannot take (operand rows that are not whole 16-byte
# chunks in bf16) silently stays on the exact-f32 kernel.
class X3Images(_ImageCache):
    """The bf16x3 operand images of ONE training step, so that a tensor is split once per step instead of once per product.  An
    activation x is the A operand of its Linear's forward product and the B operand of the weight-gradient product; a gradient dY is
    the A operand of the dX product and the A operand of dW; a weight is the B operand of the forward and of the dX product.
    Two image forms:
      * planes [2, rows, cols] (hi, lo) for the four-plane kernel (muse_gemm_x3): ONE image per tensor whatever the product reads it as;
        a producer kernel may hand them in itself (put_planes);
      * K-concatenated images for the plain kernel (shapes muse_gemm_x3 refuses): with the patterns chosen in `_gemm_bf16x3` /
        `linear_wgrad` the row-concatenated image [T, 3K] of the forward / dX product, viewed as [3T, K], IS the token-stacked image of
        the dW product (token t's three thirds are rows 3t .. 3t+2 - a contraction does not care about the order of its slots).
    The form is (layout, lo position), or (9, 0) for the planes.  The owner clears the cache at the start of a forward and at the end of
    a backward."""

    def get(self, t, layout, K, lo_pos, last_use=False):
        key = self._key(t, layout, lo_pos)
        hit = self._find(key)
        if hit is not None:
            if last_use and self.persist.pop(key, None) is not None:
                self._store(key, hit, short=True)      # (dW is an activation's last reader - bar siblings that share it, q / k / v)
            return hit[1], hit[2]
        out, ld = _split_cat3_now(t, layout, K, lo_pos)
        self._store(key, (t, out, ld), short=last_use)
        return out, ld

    def planes(self, t):
        """(hi, lo) planes [2, *t.shape] of a contiguous f32 tensor (the operand form of muse_gemm_x3): ONE image per tensor whatever
        the product reads it as (forward A, dX A, dW A / B, a weight in the forward and in dX)"""
        key = self._key(t, 9, 0)
        hit = self._find(key)
        if hit is not None:
            return hit[1]
        out = _split_planes_now(t)
        self._store(key, (t, out, 0))
        return out

    def put_planes(self, t, planes):
        """a producer kernel wrote t's planes itself (same bits as the split of t): no split pass when a product reads t"""
        self.produced += 1
        self._store(self._key(t, 9, 0), (t, planes, 0))


def split_f32(t):
    """f32 tensor -> (hi, lo) bf16 tensors of the same shape AND strides (a GEMM's offsets / leading dimensions / batch strides
    stay valid); contiguous storage goes through muse_split_f32_to_bf16x2"""
    require_gpu(t)
    if t.is_contiguous():
        hi = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
        lo = torch.empty_like(hi)
        check(lib().muse_split_f32_to_bf16x2(t.data_ptr(), hi.data_ptr(), lo.data_ptr(), t.numel(), stream()), "muse_split_f32_to_bf16x2")
        return hi, lo
    hi = torch.empty_strided(t.shape, t.stride(), dtype=torch.bfloat16, device=t.device)
    lo = torch.empty_strided(t.shape, t.stride(), dtype=torch.bfloat16, device=t.device)
    hi.copy_(t)
    lo.copy_(t - hi.float())
    return hi, lo


X3_NATIVE = os.environ.get("MUSE_X3_NATIVE", "1") != "0"   # bf16x3 GEMM mode: the four-plane kernel (muse_gemm_x3) where it takes the product
X3_CAT = os.environ.get("MUSE_X3_CAT", "1") != "0"    # bf16x3 GEMM mode: one launch over a 3K-long concatenated operand pair (0: three launches)


def _split_planes_now(t):
    out = torch.empty((2,) + tuple(t.shape), dtype=torch.bfloat16, device=t.device)
    check(lib().muse_split_f32_to_bf16x2(t.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), t.numel(), stream()), "muse_split_f32_to_bf16x2")
    return out


def split_planes(t):
    """[2, *t.shape] bf16: hi = bf16(t), lo = bf16(t - hi), through the running step's image cache when there is one"""
    if isinstance(t, OperandOnly):
        if not isinstance(t, Planes):
            raise _hip.MuseHipError("a half image reached a bf16x3 product")
        return t.planes
    require_gpu(t)
    im = _PASS.x3
    return _split_planes_now(t) if im is None else im.planes(t)


def split_cat3(t, layout, K, lo_pos, last_use=False):
    """_split_cat3_now through the running step's image cache (X3Images), when there is one"""
    im = _PASS.x3
    if im is None:
        return _split_cat3_now(t, layout, K, lo_pos)
    return im.get(t, layout, K, lo_pos, last_use)


def _split_cat3_now(t, layout, K, lo_pos):
    """the bf16x3 operand of a 2-D contiguous f32 tensor for a product over its K dimension: layout 0 (k-contiguous [R, K]) ->
    ([R, 3K], ld 3K), layout 1 (k-major [K, R]) -> ([3K, R], ld R); thirds (hi | hi | lo) for lo_pos 2, (hi | lo | hi) for lo_pos 1"""
    require_gpu(t)
    rows, cols = t.shape
    if layout == 0:
        out = torch.empty((rows, 3 * cols), dtype=torch.bfloat16, device=t.device)
        ld_out = 3 * cols
    else:
        out = torch.empty((3 * rows, cols), dtype=torch.bfloat16, device=t.device)
        ld_out = cols
    check(lib().muse_split_f32_to_bf16_cat3(t.data_ptr(), out.data_ptr(), rows, cols, t.stride(0), ld_out, layout, lo_pos, stream()),
          "muse_split_f32_to_bf16_cat3")
    return out, ld_out


def _gemm_bf16x3(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, a_off, b_off, c_off, alpha, bias, rowvec, residual, ldr, batch, zdiv,
                 sA, sB, sC, accumulate):
    """-> True when the product ran as three bf16 GEMMs accumulating into the f32 output, False when the bf16 kernels cannot take it"""
    d = GemmDesc()
    d.A, d.B, d.C = A.data_ptr() + a_off * 2, B.data_ptr() + b_off * 2, C_.data_ptr() + c_off * 4     # (alignment probe: bf16 offsets)
    d.dtype, d.out_dtype, d.layout_a, d.layout_b = BF16, F32, la, lb
    d.M, d.N, d.K, d.batch, d.zdiv = M, N, K, batch, zdiv
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.sA0, d.sA1 = sA
    d.sB0, d.sB1 = sB
    d.sC0, d.sC1 = sC
    d.alpha = alpha
    if batch > 1:
        # the batched products of the materialised attention core (per-head Q K^T, P V and their gradients: K = head_dim or the
        # sequence length, a few hundred at most) stay on the exact-f32 MFMA: they are ~4 % of a layer's flops, and three launches of
        # the 128^2 bf16 kernel plus the operand splits cost MORE than one exact product at these sizes (rocprof of the config-4
        # bf16x3 leg, profiles/r04_config4_bf16x3_kernel_stats_before.csv: 4452 + 4464 launches of ~45 us)
        return False
    if (a_off % 8) or (b_off % 8) or lib().muse_gemm_tile(C.byref(d)) < 0:
        return False
    full2d = (a_off == 0 and b_off == 0 and A.dim() == 2 and B.dim() == 2 and A.is_contiguous() and B.is_contiguous() and K % 8 == 0
              and A.stride(0) == lda and B.stride(0) == ldb and A.shape[1 if la == 0 else 0] == K and B.shape[1 if lb == 0 else 0] == K
              and A.shape[0 if la == 0 else 1] >= M and B.shape[0 if lb == 0 else 1] >= N and A.numel() * 2 < (1 << 31) and B.numel() * 2 < (1 << 31))
    if X3_NATIVE and full2d and lda % 8 == 0 and ldb % 8 == 0 and A.numel() % 8 == 0 and B.numel() % 8 == 0:
        # ONE kernel on the four planes (hi, lo of each operand; csrc/gemm256.h PipeX3): every plane goes through the LDS-DMA path once
        # per K-tile and feeds three MFMA products; one image per tensor serves every product that reads it
        a2, b2 = split_planes(A), split_planes(B)
        if _gemm_plain(a2[0], b2[0], C_, M, N, K, la=la, lb=lb, lda=lda, ldb=ldb, ldc=ldc, c_off=c_off, alpha=alpha, bias=bias, rowvec=rowvec,
                       residual=residual, ldr=ldr, accumulate=accumulate, x3_lo=(A.numel(), B.numel())) is not None:
            return True
    if isinstance(A, OperandOnly) or isinstance(B, OperandOnly):
        raise _hip.MuseHipError("a planes-only operand reached a product the four-plane kernel does not take")
    if X3_CAT and full2d and 3 * A.numel() * 2 < (1 << 31) and 3 * B.numel() * 2 < (1 << 31):
        # ONE launch: A' = (hi | hi | lo), B' = (hi | lo | hi) along a three times longer K (muse_split_f32_to_bf16_cat3) - one epilogue,
        # no read-modify-write of C between the terms, the persistent kernel where the plain product would take it
        # which operand carries (hi | hi | lo) and which (hi | lo | hi) is free as long as the two differ; chosen so that the images of
        # a Linear's forward (x W^T: lb = 0) and dX (dY W: lb = 1) products are the ones its dW product wants (X3Images)
        pa, pb = (2, 1) if lb == 0 else (1, 2)
        a3, lda3 = split_cat3(A, la, K, pa)
        b3, ldb3 = split_cat3(B, lb, K, pb)
        _gemm_plain(a3, b3, C_, M, N, 3 * K, la=la, lb=lb, lda=lda3, ldb=ldb3, ldc=ldc, c_off=c_off, alpha=alpha, bias=bias, rowvec=rowvec,
                    residual=residual, ldr=ldr, accumulate=accumulate)
        return True
    ah, al = split_f32(A)
    bh, bl = split_f32(B)
    kw = dict(la=la, lb=lb, lda=lda, ldb=ldb, ldc=ldc, a_off=a_off, b_off=b_off, c_off=c_off, alpha=alpha, batch=batch, zdiv=zdiv,
              sA=sA, sB=sB, sC=sC)
    _gemm_plain(ah, bh, C_, M, N, K, bias=bias, rowvec=rowvec, residual=residual, ldr=ldr, accumulate=accumulate, **kw)
    _gemm_plain(ah, bl, C_, M, N, K, accumulate=True, **kw)
    _gemm_plain(al, bh, C_, M, N, K, accumulate=True, **kw)
    return True


def _gemm_via_transpose(A, B, C_, M, N, K, la, lb, lda, ldb, ldc, a_off, b_off, c_off, alpha, bias, rowvec, residual,
                        ldr, batch, zdiv, sA, sB, sC, accumulate, act):
    """Bring-up fallback: materialise k-contiguous copies of k-major operands with muse_transpose."""
    Kp = (K + 7) // 8 * 8

    def fix(X, layout, R, ld, off, s):
        if layout == 0:
            return X, ld, off, s
        # X(r,k) at off + k*ld + r  ->  T[z][r][k], zero padded to Kp
        T = torch.zeros((batch, R, Kp), dtype=X.dtype, device=X.device)
        for z in range(batch):  # batches are few in this debug path
            zo = off + (z // zdiv) * s[0] + (z % zdiv) * s[1]
            check(lib().muse_transpose(X.data_ptr() + zo * _esz(X), T[z].data_ptr(), dt(X), K, R, ld, Kp, 1, 0, 0,
                                       stream()), "muse_transpose")
        return T, Kp, 0, (zdiv * R * Kp, R * Kp)

    A2, lda2, a_off2, sA2 = fix(A, la, M, lda, a_off, sA)
    B2, ldb2, b_off2, sB2 = fix(B, lb, N, ldb, b_off, sB)
    return _gemm_plain(A2, B2, C_, M, N, K, la=0, lb=0, lda=lda2, ldb=ldb2, ldc=ldc, a_off=a_off2, b_off=b_off2, c_off=c_off,
                       alpha=alpha, bias=bias, rowvec=rowvec, residual=residual, ldr=ldr, batch=batch, zdiv=zdiv, sA=sA2,
                       sB=sB2, sC=sC, accumulate=accumulate, act=act)


def linear(x, w, out=None, *, out_dtype=None, residual=None, act=0, bias=None):
    """y[T,N] = x[T,K] @ w[N,K]^T (+bias) (gelu) (+residual)   — nn.Linear forward."""
    T_, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((T_, N), dtype=out_dtype or x.dtype, device=x.device)
    return gemm(x, w, out, T_, N, K, la=0, lb=0, lda=x.stride(0), ldb=w.stride(0), ldc=out.stride(0), residual=residual,
                ldr=residual.stride(0) if residual is not None else 0, act=act, bias=bias)


def linear_dgrad(dy, w, out=None):
    """dx[T,K] = dy[T,N] @ w[N,K]    (w consumed as a k-major operand)."""
    T_, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty((T_, K), dtype=dy.dtype, device=dy.device)
    return gemm(dy, w, out, T_, K, N, la=0, lb=1, lda=dy.stride(0), ldb=w.stride(0), ldc=out.stride(0))


SPLIT_K = os.environ.get("MUSE_SPLIT_K", "1") != "0"   # MUSE_SPLIT_K=0: deterministic (no f32 atomics) weight gradients


def wgrad_splits(M, N, K, dtype, slots=512, tile=128, ktile_us=1.8):
    """K slices for a weight-gradient GEMM.  The [N_out, K_in] output has few tiles while K = tokens is long, so the K
    loop is cut.  128^2 kernel (2 blocks per CU = 512 slots): the slice count that fills whole rounds of resident blocks
    best, with at least 4 K-tiles per slice.  256^2 LDS-DMA kernel (1 block per CU = 256 slots): the slice count with the
    smallest modelled time = rounds x (K-tiles per slice x 1.8 us + 6 us) + workspace traffic of the slice reduction
    ((slices + 1) x 4 M N bytes at ~4 TB/s)."""
    if not SPLIT_K:
        return 1
    tiles = ((M + tile - 1) // tile) * ((N + tile - 1) // tile)
    nk = (K + 63) // 64
    best, best_eff, best_cost = 1, 0.0, float("inf")
    for s in range(1, max(1, min(nk // 4, 64)) + 1):
        per = (nk + s - 1) // s
        s_eff = (nk + per - 1) // per          # every slice must own at least one K-tile
        blocks = tiles * s_eff
        if tile == 256:
            cost = ((blocks + slots - 1) // slots) * (per * ktile_us + 6.0) + ((s_eff + 1) * 4.0 * M * N / 4e6 if s_eff > 1 else 0.0)
            if cost < best_cost - 1e-9:
                best, best_cost = s_eff, cost
        else:
            eff = blocks / (((blocks + slots - 1) // slots) * slots)
            if eff > best_eff + 0.02:
                best, best_eff = s_eff, eff
    return best


_WGRAD_PLAN = {}


def _wgrad_plan(dy, x, N, K, T_, lda, ldb):
    """(split_k) for dw[N,K] = dy^T x: sized for the 256^2 kernel when muse_gemm would take it (muse_gemm_tile), else for
    the 128^2 one."""
    key = (N, K, T_, dy.dtype, lda, ldb)
    plan = _WGRAD_PLAN.get(key)
    if plan is None:
        plan = wgrad_splits(N, K, T_, dy.dtype, slots=512, tile=128)
        if dy.dtype in (torch.bfloat16, torch.float16):
            sk = wgrad_splits(N, K, T_, dy.dtype, slots=256, tile=256)
            d = GemmDesc()
            d.A, d.B, d.C = dy.data_ptr(), x.data_ptr(), dy.data_ptr()   # (pointers only checked for alignment)
            d.dtype, d.out_dtype, d.layout_a, d.layout_b = (F16 if dy.dtype == torch.float16 else BF16), F32, 1, 1
            d.M, d.N, d.K, d.batch, d.zdiv = N, K, T_, 1, 1
            d.lda, d.ldb, d.ldc = lda, ldb, K
            d.alpha = 1.0
            d.split_k, d.split_stride = sk, (N * K if sk > 1 else 0)
            if lib().muse_gemm_tile(C.byref(d)) == 256:
                plan = sk
        _WGRAD_PLAN[key] = plan
    return plan


_WGRAD_X3_PLAN = {}
X3_WGRAD_KTILE_US = float(os.environ.get("MUSE_X3_WGRAD_KTILE_US", "4.7"))   # cost-model time of a 64-wide K chunk of kernel_x3 (plain kernel: 1.8)


def _wgrad_x3_native(dy, x, dw, accumulate, M):
    """dw (+)= dy^T x as the four-plane bf16x3 product (muse_gemm_x3, both operands k-major) with the K split of the 256-tile kernel;
    False when that kernel does not take the shape"""
    T_, ncols = dy.shape
    N = M if M is not None else ncols
    K = x.shape[1]
    if N < 128 or K < 128 or T_ < 64 or dy.numel() % 8 or x.numel() % 8 or dy.numel() * 2 >= (1 << 31) or x.numel() * 2 >= (1 << 31):
        return False
    dy2, x2 = split_planes(dy), split_planes(x)
    lo = (dy.numel(), x.numel())
    splittable = dw.dtype == torch.float32 and dw.is_contiguous() and (N * K) % 4 == 0
    sk = 1
    if splittable:
        sk = _WGRAD_X3_PLAN.get((N, K, T_))
        if sk is None:      # a 64-wide K-tile of this kernel is three products: ~2.6 x the plain kernel's time per tile
            sk = _WGRAD_X3_PLAN[(N, K, T_)] = wgrad_splits(N, K, T_, torch.bfloat16, slots=256, tile=256, ktile_us=X3_WGRAD_KTILE_US)
    if sk <= 1:
        return _gemm_plain(dy2[0], x2[0], dw, N, K, T_, la=1, lb=1, lda=ncols, ldb=K, ldc=dw.stride(0), accumulate=accumulate, x3_lo=lo) is not None
    ws = torch.empty((sk, N, K), dtype=torch.float32, device=dw.device)
    if _gemm_plain(dy2[0], x2[0], ws, N, K, T_, la=1, lb=1, lda=ncols, ldb=K, ldc=K, split_k=sk, split_stride=N * K, x3_lo=lo) is None:
        return False
    check(lib().muse_sum_slices(ws.data_ptr(), dw.data_ptr(), sk, N * K, N * K, 1 if accumulate else 0, stream()), "muse_sum_slices")
    return True


def planes_only_ok(rows, cols):
    """may a producer hand its [rows, cols] result to the weight GEMMs as its operand image only?  (a step of either mode is running, its
    producers are on and its kernels take products with this operand: >= 128 rows / columns, whole 16-byte rows)"""
    return (X3_PLANES_ONLY and _PASS.kind is not None and _PASS.producing() is not None and rows >= 128 and cols >= 128
            and rows % 8 == 0 and cols % 8 == 0 and rows * cols * 2 < (1 << 31))


def linear_wgrad(dy, x, dw, accumulate, M=None, lda=None):
    """dw[N,K] (+)= dy[T,N]^T @ x[T,K]   (both operands k-major, f32 output into the flat grad buffer).
    Split-K slices write partial tiles to a workspace that muse_sum_slices folds into dw in a fixed order."""
    kind = _PASS.kind
    if kind == "f16" and dw.dtype == torch.float32 and dw.is_contiguous() and dw.data_ptr() % 16 == 0:
        pair = f16_wgrad_operands(dy, x, M, lda)      # half operand images: dy is a gradient (the pass's scale), x a saved activation
        if pair is not None:
            return _linear_wgrad_plain(pair[0], pair[1], dw, accumulate, M, lda)
    x3 = kind == "bf16x3" and dy.dtype == torch.float32 and x.dtype == torch.float32 and dw.dtype == torch.float32 \
        and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0 and x.shape[1] % 8 == 0 and (M if M is not None else dy.shape[1]) % 8 == 0
    if not x3:
        if isinstance(dy, OperandOnly) or isinstance(x, OperandOnly):
            raise _hip.MuseHipError("a planes-only operand reached a weight-gradient product outside the bf16x3 mode's preconditions")
        return _linear_wgrad_plain(dy, x, dw, accumulate, M, lda)
    whole = dy.dim() == x.dim() == 2 and dy.is_contiguous() and x.is_contiguous() and (lda is None or lda == dy.stride(0)) and dy.shape[0] == x.shape[0]
    if X3_NATIVE and whole and _wgrad_x3_native(dy, x, dw, accumulate, M):
        return dw
    if isinstance(dy, OperandOnly) or isinstance(x, OperandOnly):
        raise _hip.MuseHipError("a planes-only operand reached a weight-gradient product the four-plane kernel does not take")
    if X3_CAT and whole and 3 * dy.numel() * 2 < (1 << 32) - 64 and 3 * x.numel() * 2 < (1 << 32) - 64:
        # one product over 3 T slots: the ROW-concatenated images dY' [T, 3N] = (hi | lo | hi), X' [T, 3K] = (hi | hi | lo) - the ones
        # the dX product of dY and the forward product of x made (X3Images) - read as [3T, N] / [3T, K]: slot 3t + s holds third s
        # of token t in both, so the contraction over slots is sum_t hi hi + lo hi + hi lo
        T_ = dy.shape[0]
        dy3, _ = split_cat3(dy, 0, dy.shape[1], 1)
        xc3, _ = split_cat3(x, 0, x.shape[1], 2, last_use=True)
        _linear_wgrad_plain(dy3.view(3 * T_, dy.shape[1]), xc3.view(3 * T_, x.shape[1]), dw, accumulate, M, lda)
    else:                             # three bf16 products through the bf16 split-K machinery, accumulated in a fixed order
        dyh, dyl = split_f32(dy)
        xh, xl = split_f32(x)
        _linear_wgrad_plain(dyh, xh, dw, accumulate, M, lda)
        _linear_wgrad_plain(dyh, xl, dw, True, M, lda)
        _linear_wgrad_plain(dyl, xh, dw, True, M, lda)
    return dw


def _linear_wgrad_plain(dy, x, dw, accumulate, M, lda):
    """linear_wgrad on the operands as they are: one product, or split-K slices and their fixed-order sum"""
    T_, N = dy.shape
    if M is not None:
        N = M
    K = x.shape[1]
    lda = lda or dy.stride(0)
    splittable = dw.dtype == torch.float32 and dw.is_contiguous() and (N * K) % 4 == 0
    sk = _wgrad_plan(dy, x, N, K, T_, lda, x.stride(0)) if splittable else 1
    # (a bf16 / half pair: nothing for the mode prologue to route; anything else - f32, a mixed pair it routes or refuses - goes through it)
    mm = _gemm_plain if dy.dtype == x.dtype != torch.float32 else gemm
    if sk <= 1:
        return mm(dy, x, dw, N, K, T_, la=1, lb=1, lda=lda, ldb=x.stride(0), ldc=dw.stride(0), accumulate=accumulate)
    ws = torch.empty((sk, N, K), dtype=torch.float32, device=dw.device)
    mm(dy, x, ws, N, K, T_, la=1, lb=1, lda=lda, ldb=x.stride(0), ldc=K, split_k=sk, split_stride=N * K)
    check(lib().muse_sum_slices(ws.data_ptr(), dw.data_ptr(), sk, N * K, N * K, 1 if accumulate else 0, stream()),
          "muse_sum_slices")
    return dw


# ---- grouped weight gradients -------------------------------------------------------------------------------------------------------
# MUSE_WGRAD_GROUP = K slices per product of a grouped dW launch when it runs BESIDE the backward chain on the weight-gradient stream
# (0: off - one split-K launch + slice sum per weight, the round-3 path).  Default 1: 144 blocks of 257 K-tiles at config B - no
# workspace, no slice sum, one f32 epilogue per tile; the launch fills 144 of 256 CUs and the concurrent dX / row kernels take the
# rest.  Same box, default bench loop (profiles/r04_wgrad_group_ab.txt): off 1155 images/s, 1 slice 1190, 2: 1185, 3: 1182, 5: 1172, 7: 1163.
# MUSE_WGRAD_GROUP_SERIAL = the slice count when nothing runs beside it (weight gradients on the main stream: wgrad_stream off, the
# instrumented serial step of bench.py): 5 slices = 720 blocks = 2.8 rounds of the chip (1114 TFLOP/s alone; 1 slice: 798).
WGRAD_GROUP = int(os.environ.get("MUSE_WGRAD_GROUP", "1"))
WGRAD_GROUP_SERIAL = int(os.environ.get("MUSE_WGRAD_GROUP_SERIAL", "5"))
WGRAD_SEQ_SLICES = int(os.environ.get("MUSE_WGRAD_SEQ_SLICES", "1"))   # (experiment: see linear_wgrad_group)


def sum_multi(jobs):
    """jobs: list of (kind, ws, out, nslices, n, stride, accumulate) with kind 0 = slice sum (muse_sum_slices), 1 = column sum
    (muse_colsum) - ONE launch, each job bit-identical to its single-job kernel"""
    for i in range(0, len(jobs), 16):
        part = jobs[i:i + 16]
        n = len(part)
        vp, i32, i64 = C.c_void_p * n, C.c_int32 * n, C.c_int64 * n
        check(lib().muse_sum_multi(vp(*[j[1].data_ptr() for j in part]), vp(*[j[2].data_ptr() for j in part]),
                                   i32(*[int(j[3]) for j in part]), i64(*[int(j[4]) for j in part]), i64(*[int(j[5]) for j in part]),
                                   i32(*[1 if j[6] else 0 for j in part]), i32(*[int(j[0]) for j in part]), n, stream()), "muse_sum_multi")


def linear_wgrad_group(items, colsums=None, split=None):
    """The weight gradients of one transformer layer in ONE launch + one reduction launch.
    items: list of (dy, x, dw, accumulate, M, lda) as linear_wgrad takes them (M / lda may be None); colsums: a queue of pending
    column sums (see _colsum_or_defer) folded into the same reduction launch.  Falls back to linear_wgrad per item whenever the
    256^2 kernel does not take every product (f32 mode, tiny shapes)."""
    split = WGRAD_GROUP if split is None else split
    descs, meta = [], []
    dt16 = items[0][0].dtype if items else None
    ok = split >= 1 and 1 <= len(items) <= 8 and dt16 in (torch.bfloat16, torch.float16) and all(it[0].dtype == dt16 and it[1].dtype == dt16 for it in items)
    if ok:
        arr = (GemmDesc * len(items))()
        for d, (dy, x, dw, accumulate, M, lda) in zip(arr, items):
            T_, N = dy.shape
            N = M if M is not None else N
            K = x.shape[1]
            ok = ok and dw.dtype == torch.float32 and dw.is_contiguous() and (N * K) % 4 == 0
            ok = ok and (split == 1 or dw.data_ptr() % 16 == 0)   # muse_sum_multi's slice sums store 16 bytes at a time
            d.A, d.B = dy.data_ptr(), x.data_ptr()
            d.dtype, d.out_dtype, d.layout_a, d.layout_b = (F16 if dt16 == torch.float16 else BF16), F32, 1, 1
            d.M, d.N, d.K, d.batch, d.zdiv = N, K, T_, 1, 1
            d.lda, d.ldb, d.ldc = (lda or dy.stride(0)), x.stride(0), K
            d.alpha = 1.0 / (getattr(dy, "_muse_scale", 1.0) * getattr(x, "_muse_scale", 1.0))      # (half images carry their power-of-two scale)
            meta.append((N, K, T_))
        if ok:
            ws = []
            for d, (dy, x, dw, accumulate, M, lda), (N, K, T_) in zip(arr, items, meta):
                if split > 1:
                    w = torch.empty((split, N, K), dtype=torch.float32, device=dw.device)
                    ws.append(w)
                    d.C, d.split_k, d.split_stride, d.accumulate = w.data_ptr(), split, N * K, 0
                else:
                    d.C, d.split_k, d.split_stride, d.accumulate = dw.data_ptr(), 1, 0, (1 if accumulate else 0)
            ok = lib().muse_gemm_group_ok(arr, len(items), split) == 0
    if not ok:
        for dy, x, dw, accumulate, M, lda in items:
            linear_wgrad(dy, x, dw, accumulate, M=M, lda=lda)
        if colsums:
            flush_colsums(colsums)
        return
    e0 = _prof_begin()
    seq = WGRAD_SEQ_SLICES if split == 1 else 1
    if seq > 1:
        # experiment (round 6, MUSE_WGRAD_SEQ_SLICES): the token dimension cut into `seq` launches that accumulate into dw one after the other -
        # no workspace, no reduction, the same tiles, but a workgroup of the dW stream holds its CU a `seq`-th as long (the step's
        # critical path is the main stream's latency: profiles/r06_ceiling.md)
        base = [(d.A, d.B, d.K, d.accumulate) for d in arr]
        for i in range(seq):
            for d, (a0, b0, T_, acc0) in zip(arr, base):
                nk = (T_ + 63) // 64
                k0 = (nk * i // seq) * 64
                k1 = min(T_, (nk * (i + 1) // seq) * 64) if i + 1 < seq else T_
                d.A, d.B, d.K = a0 + k0 * d.lda * 2, b0 + k0 * d.ldb * 2, k1 - k0
                d.accumulate = acc0 if i == 0 else 1
            check(lib().muse_gemm_group(arr, len(items), 1, stream()), "muse_gemm_group")
    else:
        check(lib().muse_gemm_group(arr, len(items), split, stream()), "muse_gemm_group")
    _prof_end(e0, "gemm_f16_TT" if dt16 == torch.float16 else "gemm_bf16_TT", sum(2.0 * N * K * T_ for N, K, T_ in meta))
    jobs = []
    if split > 1:
        # (the slice count the kernel really cuts: ceil(nk / ceil(nk / split)) slices are non-empty; the others leave their workspace
        #  slice untouched, so only the written ones are summed)
        for w, (dy, x, dw, accumulate, M, lda), (N, K, T_) in zip(ws, items, meta):
            nk = (T_ + 63) // 64
            per = (nk + split - 1) // split
            jobs.append((0, w, dw, (nk + per - 1) // per, N * K, N * K, accumulate))
    if colsums:
        cur = torch.cuda.current_stream(colsums[0][0].device)
        for part, dw, nblk, cols, accumulate in colsums:
            jobs.append((1, part, dw, nblk, cols, cols, accumulate))
            part.record_stream(cur)
        colsums.clear()
    if jobs:
        sum_multi(jobs)


def transpose(src, dst):
    """dst[c, r] = src[r, c] for contiguous 2-D tensors of the same dtype"""
    require_gpu(src, dst)
    r, c = src.shape
    check(lib().muse_transpose(src.data_ptr(), dst.data_ptr(), dt(src), r, c, src.stride(0), dst.stride(0), 1, 0, 0, stream()),
          "muse_transpose")
    return dst


def layernorm_fwd(x, w, eps, out_dtype, residual=None):
    require_gpu(x, w)
    rows, cols = x.shape
    y = torch.empty((rows, cols), dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_layernorm_fwd(x.data_ptr(), dt(x), w.data_ptr(), ptr(residual), y.data_ptr(), dt(y), mean.data_ptr(),
                                   rstd.data_ptr(), rows, cols, eps, stream()), "muse_layernorm_fwd")
    _prof_end(e0, "layernorm_fwd", _nbytes(x, residual, y), "byte")
    return y, mean, rstd


# The column sums that finish a LayerNorm weight gradient (per-block partials -> dw) are leaves of the backward graph.  A caller that
# runs weight gradients on a second stream passes `colsum_queue` (a list it owns): the sum is queued instead of launched, and
# flush_colsums(queue) launches the queue on whatever stream is current - the weight-gradient stream, off the dX chain.
def _colsum_or_defer(part, dw, nblk, cols, accumulate, queue):
    if queue is not None:
        queue.append((part, dw, nblk, cols, accumulate))
    else:
        check(lib().muse_colsum(part.data_ptr(), dw.data_ptr(), nblk, cols, 1 if accumulate else 0, stream()), "muse_colsum")


def flush_colsums(queue):
    """launch the queued column sums on the current stream (the caller has ordered it behind the kernels that wrote the partials)"""
    if not queue:
        return
    cur = torch.cuda.current_stream(queue[0][0].device)
    for part, dw, nblk, cols, accumulate in queue:
        check(lib().muse_colsum(part.data_ptr(), dw.data_ptr(), nblk, cols, 1 if accumulate else 0, stream()), "muse_colsum")
        part.record_stream(cur)
    queue.clear()


def layernorm_bwd(dy, x, w, mean, rstd, dx_dtype, dw, accumulate, dres=None, also_bf16=False, colsum_queue=None):
    """returns dx (= LN'(dy) + dres); dw (+)= column sums of dy * xhat.  also_bf16: returns (dx, bf16 copy of dx) written in the
    same pass."""
    require_gpu(dy, x, w)
    rows, cols = x.shape
    dx = torch.empty((rows, cols), dtype=dx_dtype, device=x.device)
    dx2 = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device) if also_bf16 else None
    nblk = lib().muse_layernorm_bwd_nblk(rows)
    part = torch.empty((nblk, cols), dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_layernorm_bwd(dy.data_ptr(), dt(dy), x.data_ptr(), dt(x), w.data_ptr(), mean.data_ptr(),
                                   rstd.data_ptr(), ptr(dres), dx.data_ptr(), dt(dx), ptr(dx2), part.data_ptr(), nblk, rows, cols,
                                   stream()), "muse_layernorm_bwd")
    _colsum_or_defer(part, dw, nblk, cols, accumulate, colsum_queue)
    _prof_end(e0, "layernorm_bwd", _nbytes(dy, x, dres, dx, dx2), "byte")
    return (dx, dx2) if also_bf16 else dx


# bit 0: fused forward pair (ln_fwd 1.74 -> 1.30 ms per step), bit 1: fused backward pair (measured SLOWER: 128 VGPRs / 4 waves per
# SIMD against 78 / 6 of ln_bwd_kernel - 2.96 -> 3.41 ms; kept for experiments, off by default)
LN_PAIR = int(os.environ.get("MUSE_LN_PAIR", "1"))


def layernorm_pair_ok(ao, x, cd, direction):
    return bool(LN_PAIR & direction) and cd == torch.bfloat16 and ao.dtype == torch.bfloat16 and x.dtype == torch.float32 and \
        x.shape[1] % 4 == 0 and x.shape[1] <= (1024 if direction == 1 else 768)


def layernorm_pair_fwd(ao, x, w_post, w_pre, eps):
    """x1 = x + LN(ao) * w_post ; ln2 = LN(x1) * w_pre  ->  (x1 f32, mean_post, rstd_post, ln2 bf16, mean_pre, rstd_pre)"""
    require_gpu(ao, x, w_post, w_pre)
    rows, cols = x.shape
    x1 = torch.empty_like(x)
    ln2 = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    st = torch.empty((4, rows), dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_layernorm_pair_fwd(ao.data_ptr(), x.data_ptr(), w_post.data_ptr(), w_pre.data_ptr(), x1.data_ptr(), ln2.data_ptr(),
                                        st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), rows, cols, eps, stream()),
          "muse_layernorm_pair_fwd")
    _prof_end(e0, "layernorm_fwd", _nbytes(ao, x, x1, ln2), "byte")
    return x1, st[0], st[1], ln2, st[2], st[3]


def layernorm_pair_bwd(dln2, x1, w_pre, mean_pre, rstd_pre, dres, ao, w_post, mean_post, rstd_post, dw_pre, acc_pre, dw_post, acc_post,
                       colsum_queue=None):
    """dx1 = LN_pre'(dln2) + dres ; dao = LN_post'(dx1)  ->  (dx1 f32, dao bf16); dw_pre / dw_post (+)= their weight gradients"""
    require_gpu(dln2, x1, ao)
    rows, cols = x1.shape
    dx1 = torch.empty_like(x1)
    dao = torch.empty((rows, cols), dtype=torch.bfloat16, device=x1.device)
    nblk = lib().muse_layernorm_bwd_nblk(rows)
    part = torch.empty((2, nblk, cols), dtype=torch.float32, device=x1.device)
    e0 = _prof_begin()
    check(lib().muse_layernorm_pair_bwd(dln2.data_ptr(), x1.data_ptr(), w_pre.data_ptr(), mean_pre.data_ptr(), rstd_pre.data_ptr(), ptr(dres),
                                        ao.data_ptr(), w_post.data_ptr(), mean_post.data_ptr(), rstd_post.data_ptr(), dx1.data_ptr(),
                                        dao.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), nblk, rows, cols, stream()),
          "muse_layernorm_pair_bwd")
    _colsum_or_defer(part[0], dw_pre, nblk, cols, acc_pre, colsum_queue)
    _colsum_or_defer(part[1], dw_post, nblk, cols, acc_post, colsum_queue)
    _prof_end(e0, "layernorm_bwd", _nbytes(dln2, x1, dres, ao, dx1, dao), "byte")
    return dx1, dao


def softmax_(x, rows, cols, ld):
    require_gpu(x)
    check(lib().muse_softmax_fwd(x.data_ptr(), x.data_ptr(), dt(x), rows, cols, ld, stream()), "muse_softmax_fwd")
    return _touched(x)


def softmax_bwd_(p, dp, rows, cols, ld):
    """in place on dp: ds = p * (dp - sum(p*dp))"""
    require_gpu(p, dp)
    check(lib().muse_softmax_bwd(p.data_ptr(), dp.data_ptr(), dp.data_ptr(), dt(p), rows, cols, ld, stream()), "muse_softmax_bwd")
    return _touched(dp)


def attention_supported(dtype, seq, head_dim, seq_kv=None):
    """the fused attention kernels take bf16, head_dim 16/32/48/64 and any query / key length"""
    return dtype == torch.bfloat16 and seq > 0 and (seq_kv is None or seq_kv > 0) and head_dim in (16, 32, 48, 64)


def _row_view(t, heads_dim):
    """(base tensor pointer, elements between tokens) of a [tokens, >= heads_dim] view with unit column stride"""
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < heads_dim:
        raise _hip.MuseHipError("attention operands are [tokens, features] views with contiguous features")
    return t.data_ptr(), t.stride(0)


def _attn_desc(q, k, v, o, B, Sq, Skv, nh, hd, alpha):
    d = _hip.AttnDesc()
    H = nh * hd
    (d.q, d.ldq), (d.k, d.ldk), (d.v, d.ldv), (d.o, d.ldo) = _row_view(q, H), _row_view(k, H), _row_view(v, H), _row_view(o, H)
    d.bsq, d.bsk, d.bsv, d.bso = Sq * d.ldq, Skv * d.ldk, Skv * d.ldv, Sq * d.ldo
    d.batch, d.heads, d.head_dim, d.seq_q, d.seq_kv, d.alpha = B, nh, hd, Sq, Skv, alpha
    return d


def _drop_args(drop):
    p, seed, offset, ld_mask = drop
    return float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(ld_mask)


def attention_fwd_ex(q, k, v, B, Sq, Skv, nh, hd, alpha, out=None, drop=None):
    """fused softmax(alpha q k^T) v for separate q [B*Sq, H], k / v [B*Skv, H] views (row strides free: slices of a packed
    projection are fine); -> (ctx [B*Sq, H] bf16, lse [B*nh, seq_pad(Sq)] f32).  Self- and cross-attention."""
    require_gpu(q, k, v)
    H = nh * hd
    ctx = out if out is not None else torch.empty((B * Sq, H), dtype=q.dtype, device=q.device)
    lse = torch.empty((B * nh, lib().muse_attention_seq_pad(Sq)), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha)
    e0 = _prof_begin()
    if drop is None:
        check(lib().muse_attention_fwd_ex(C.byref(d), lse.data_ptr(), stream()), "muse_attention_fwd_ex")
    else:   # (attention_drop_fwd_ex)
        check(lib().muse_attention_drop_fwd_ex(C.byref(d), lse.data_ptr(), *_drop_args(drop), stream()), "muse_attention_drop_fwd_ex")
    _prof_end(e0, "attn_fwd_bf16", 4.0 * B * nh * Sq * Skv * hd)
    return ctx, lse


def attention_bwd_ex(q, k, v, ctx, dctx, lse, B, Sq, Skv, nh, hd, alpha, dq=None, dk=None, dv=None, drop=None):
    """-> (dq [B*Sq, H], dk, dv [B*Skv, H]) bf16; dq / dk / dv may be views (e.g. the three column blocks of a packed gradient)"""
    require_gpu(q, k, v, ctx, dctx, lse)
    H = nh * hd
    dq = dq if dq is not None else torch.empty((B * Sq, H), dtype=q.dtype, device=q.device)
    dk = dk if dk is not None else torch.empty((B * Skv, H), dtype=q.dtype, device=q.device)
    dv = dv if dv is not None else torch.empty((B * Skv, H), dtype=q.dtype, device=q.device)
    dsum = torch.empty_like(lse)
    d = _attn_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha)
    (pdo, lddo), (pdq, lddq), (pdk, lddk), (pdv, lddv) = _row_view(dctx, H), _row_view(dq, H), _row_view(dk, H), _row_view(dv, H)
    e0 = _prof_begin()
    if drop is None:
        check(lib().muse_attention_bwd_ex(C.byref(d), pdo, lddo, Sq * lddo, lse.data_ptr(), dsum.data_ptr(), pdq, lddq, Sq * lddq,
                                          pdk, lddk, Skv * lddk, pdv, lddv, Skv * lddv, stream()), "muse_attention_bwd_ex")
    else:   # (attention_drop_bwd_ex)
        check(lib().muse_attention_drop_bwd_ex(C.byref(d), pdo, lddo, Sq * lddo, lse.data_ptr(), dsum.data_ptr(), pdq, lddq, Sq * lddq,
                                               pdk, lddk, Skv * lddk, pdv, lddv, Skv * lddv, *_drop_args(drop), stream()),
              "muse_attention_drop_bwd_ex")
    _prof_end(e0, "attn_bwd_bf16", 10.0 * B * nh * Sq * Skv * hd)
    return dq, dk, dv


def attention_dropout_fused():
    """MUSE_ATTN_DROPOUT_FUSED=0 (read per call, like MUSE_ATTN2): attention dropout on the materialised route (scores, softmax_,
    dropout, P V as four launches with P and the dropped P kept for the backward) instead of inside the fused kernels"""
    return os.environ.get("MUSE_ATTN_DROPOUT_FUSED", "1") != "0"


def attention_drop_fwd_ex(q, k, v, B, Sq, Skv, nh, hd, alpha, p, seed, offset, ld_mask, out=None):
    """attention_fwd_ex with nn.Dropout(p) on the probabilities inside the kernel: element (bh, q, k) is kept iff muse_dropout(seed, offset)
    keeps flat element (bh * Sq + q) * ld_mask + k (ld_mask: multiple of 4, >= Skv; the materialised route's row pitch round_up(Skv, 8)
    reproduces its masks).  lse is that of the undropped softmax.  -> (ctx, lse)"""
    return attention_fwd_ex(q, k, v, B, Sq, Skv, nh, hd, alpha, out=out, drop=(p, seed, offset, ld_mask))


def attention_drop_bwd_ex(q, k, v, ctx, dctx, lse, B, Sq, Skv, nh, hd, alpha, p, seed, offset, ld_mask, dq=None, dk=None, dv=None):
    """backward of attention_drop_fwd_ex (same p, seed, offset, ld_mask: the masks are drawn again) -> (dq, dk, dv) as attention_bwd_ex"""
    return attention_bwd_ex(q, k, v, ctx, dctx, lse, B, Sq, Skv, nh, hd, alpha, dq=dq, dk=dk, dv=dv, drop=(p, seed, offset, ld_mask))


X3_STREAM = os.environ.get("MUSE_X3_STREAM", "1") != "0"   # sequences of several 256-key blocks: the streaming kernels (0: block pairs + merge)


def _x3_one_tile_keys(Skv):
    return 224 < Skv <= 256 or 64 < Skv <= 96


def attention_x3_blocked(Sq, Skv):
    """longer sequences (round 6: BASELINE config 4's 1024 tokens) run attention3.hip's one-tile kernels block by block: q rows in
    blocks of 256, keys in blocks of 256 (or one block of <= 96 text states), the key blocks' partial results merged by their log-sum-exps"""
    return Sq > 256 or Skv > 256


def attention_x3_streamed(Sq, Skv, dropout=False):
    """whole 256-row blocks on both sides and more than one key block: the streaming kernels (online-softmax forward, dQ and dK / dV
    passes; csrc/attention3.hip) - one writer per result, so operand images / planes-only gradients work as in the one-tile form.
    dropout: the streaming kernels have no dropout form - those steps take the block-pair route, whose one-tile kernels draw
    the full-sequence mask through their q0 / k0 arguments"""
    return X3_STREAM and not dropout and Sq % 256 == 0 and Skv % 256 == 0 and Skv > 256


def attention_x3_dropout_fused():
    """MUSE_X3_ATTN_DROPOUT_FUSED=0 (read per call, like MUSE_ATTN_DROPOUT_FUSED): attention dropout of the bf16x3 / f16 modes on the
    materialised route instead of inside the kernels of csrc/attention3.hip"""
    return os.environ.get("MUSE_X3_ATTN_DROPOUT_FUSED", "1") != "0"


def _x3_drop(drop, q0, k0, Sq):
    """drop = (p, seed, offset, ld_mask) -> the dropout arguments of muse_attention_x3_drop_fwd / _bwd for the launch whose first query /
    key is (q0, k0) of a sequence of Sq queries"""
    p, seed, offset, ld_mask = _drop_args(drop)
    return p, seed, offset, ld_mask, int(q0), int(k0), int(Sq)


def attention_x3_supported(Sq, Skv, hd):
    """shapes of the fused bf16x3 attention (csrc/attention3.hip): config 4's 16 x 16 grid against itself or its 77 text states in one tile
    per head, and whole multiples of 256 query rows / 256 keys block by block (attention_x3_blocked)"""
    return hd == 64 and Sq >= 256 and Sq % 256 == 0 and (_x3_one_tile_keys(Skv) or (Skv >= 256 and Skv % 256 == 0))


def _x3_block_desc(q, k, v, o, B, Sq, Skv, nh, hd, alpha, qi, kj, kb):
    """descriptor of query block qi (256 rows) against key block kj (kb keys) of every image: full-sequence batch strides, block pointers"""
    d = _attn_desc(q, k, v, o, B, Sq, Skv, nh, hd, alpha)
    d.q += qi * 256 * d.ldq * 4
    d.o += qi * 256 * d.ldo * 4
    d.k += kj * 256 * d.ldk * 4
    d.v += kj * 256 * d.ldv * 4
    d.seq_q, d.seq_kv = 256, kb
    return d


def _attention_x3_fwd_blocks(q, k, v, B, Sq, Skv, nh, hd, alpha, drop=None):
    """-> (ctx [B*Sq, H] f32, lse [Sq // 256, B*nh, 256] f32).  softmax over all keys = the key blocks' softmaxes re-weighted by
    exp(lse_block - lse): exact in exact arithmetic, f32 here (the products inside each block are the kernels' bf16x3 ones)."""
    H = nh * hd
    nq = Sq // 256
    nk, kb = (Skv // 256, 256) if Skv > 256 else (1, Skv)
    dev = q.device
    ctx = torch.empty((B * Sq, H), dtype=torch.float32, device=dev)
    lse = torch.empty((nq, B * nh, 256), dtype=torch.float32, device=dev)
    e0 = _prof_begin()
    if nk > 1 and X3_STREAM and drop is None:
        # whole 256-row blocks on both sides: a workgroup keeps its 256 queries and streams the key blocks through LDS with an online
        # softmax (csrc/attention3.hip fwd_stream_kernel) - q read once, the context and its log-sum-exp written once, no partials
        planes = x3_new_planes(ctx)
        d = _attn_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha)
        check(lib().muse_attention_x3_fwd_stream(C.byref(d), lse.data_ptr(), ptr(planes), ctx.numel() if planes is not None else 0,
                                                 *_image_args(False, planes), stream()), "muse_attention_x3_fwd_stream")
        x3_put_planes(ctx, planes)
    elif nk == 1:
        planes = x3_new_planes(ctx)          # ctx feeds the output projection: every block writes its rows of the operand planes too
        img = _image_args(False, planes)
        for qi in range(nq):
            d = _x3_block_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha, qi, 0, kb)
            pp = None if planes is None else planes.data_ptr() + qi * 256 * H * 2
            if drop is not None:
                check(lib().muse_attention_x3_drop_fwd(C.byref(d), lse[qi].data_ptr(), pp, ctx.numel() if planes is not None else 0,
                                                       *_x3_drop(drop, qi * 256, 0, Sq), *img, stream()), "muse_attention_x3_drop_fwd")
                continue
            check(lib().muse_attention_x3_fwd(C.byref(d), lse[qi].data_ptr(), pp, ctx.numel() if planes is not None else 0, *img, stream()),
                  "muse_attention_x3_fwd")
        x3_put_planes(ctx, planes)
    else:
        part = torch.empty((nk, B * Sq, H), dtype=torch.float32, device=dev)
        lp = torch.empty((nk, nq, B * nh, 256), dtype=torch.float32, device=dev)
        img = _image_args(False)
        for kj in range(nk):
            for qi in range(nq):
                d = _x3_block_desc(q, k, v, part[kj], B, Sq, Skv, nh, hd, alpha, qi, kj, kb)
                if drop is not None:     # (dropout commutes with the log-sum-exp merge: a block's partial context is linear in its dropped P)
                    check(lib().muse_attention_x3_drop_fwd(C.byref(d), lp[kj, qi].data_ptr(), None, 0, *_x3_drop(drop, qi * 256, kj * 256, Sq),
                                                           *img, stream()), "muse_attention_x3_drop_fwd")
                    continue
                check(lib().muse_attention_x3_fwd(C.byref(d), lp[kj, qi].data_ptr(), None, 0, *img, stream()), "muse_attention_x3_fwd")
        planes = x3_new_planes(ctx)          # ctx feeds the output projection: its operand planes come out of the merge kernel
        check(lib().muse_attention_x3_merge(part.data_ptr(), part[0].numel(), lp.data_ptr(), lp[0].numel(), nk, ctx.data_ptr(), lse.data_ptr(),
                                            ptr(planes), ctx.numel(), B, Sq, nh, *_image_args(False, planes), stream()), "muse_attention_x3_merge")
        x3_put_planes(ctx, planes)
    _prof_end(e0, "attn_fwd_bf16x3", 4.0 * B * nh * Sq * Skv * hd)
    return ctx, lse


def _attention_x3_bwd_blocks(q, k, v, ctx, dctx, lse, B, Sq, Skv, nh, hd, alpha, dq, dk, dv, drop=None):
    """block-pair backward: every (query block, key block) pair with the query block's GLOBAL log-sum-exp and the final context (so the
    probabilities and the row sums dO.O are the full-sequence ones); dq summed over key blocks, dk / dv over query blocks"""
    H = nh * hd
    nq = Sq // 256
    nk, kb = (Skv // 256, 256) if Skv > 256 else (1, Skv)
    dev = q.device
    pdo, lddo = _row_view(dctx, H)
    # partial gradients: dq of key block kj, dk / dv of query block qi - one contiguous stack each, folded by ONE row kernel into the
    # caller's (possibly strided) views; a single block writes the view directly
    dqs = None if nk == 1 else torch.empty((nk, B * Sq, H), dtype=torch.float32, device=dev)
    dks = None if nq == 1 else torch.empty((nq, B * Skv, H), dtype=torch.float32, device=dev)
    dvs = None if nq == 1 else torch.empty((nq, B * Skv, H), dtype=torch.float32, device=dev)
    dqp = [dq] if dqs is None else list(dqs)
    dkp = [dk] if dks is None else list(dks)
    dvp = [dv] if dvs is None else list(dvs)
    img = _image_args(True)
    e0 = _prof_begin()
    for qi in range(nq):
        for kj in range(nk):
            d = _x3_block_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha, qi, kj, kb)
            (pq, ldq_), (pk, ldk_), (pv, ldv_) = _row_view(dqp[kj], H), _row_view(dkp[qi], H), _row_view(dvp[qi], H)
            fn, extra = ((lib().muse_attention_x3_bwd, ()) if drop is None
                         else (lib().muse_attention_x3_drop_bwd, _x3_drop(drop, qi * 256, kj * 256, Sq)))
            check(fn(C.byref(d), pdo + qi * 256 * lddo * 4, lddo, Sq * lddo, lse[qi].data_ptr(),
                     pq + qi * 256 * ldq_ * 4, ldq_, Sq * ldq_, pk + kj * 256 * ldk_ * 4, ldk_, Skv * ldk_,
                     pv + kj * 256 * ldv_ * 4, ldv_, Skv * ldv_, None, 0, None, 0, None, 0, *extra, *img, stream()),
                  "muse_attention_x3_bwd" if drop is None else "muse_attention_x3_drop_bwd")
    for stack, g, rows in ((dqs, dq, B * Sq), (dks, dk, B * Skv), (dvs, dv, B * Skv)):
        if stack is not None:
            pg, ldg = _row_view(g, H)
            check(lib().muse_sum_parts_strided(stack.data_ptr(), stack[0].numel(), stack.shape[0], rows, H, pg, ldg, 0, stream()), "muse_sum_parts_strided")
    for t in (dq, dk, dv):
        _touched(t)            # (written through raw pointers: cached operand planes of their previous contents must not be found)
    _prof_end(e0, "attn_bwd_bf16x3", 10.0 * B * nh * Sq * Skv * hd)
    return dq, dk, dv


def attention_x3_fwd(q, k, v, B, Sq, Skv, nh, hd, alpha, drop=None):
    """fused softmax(alpha q k^T) v on f32 tensors with bf16x3 products (TF32-class: <= 2^-16 relative per product); q [B*Sq, H],
    k / v [B*Skv, H] f32 views (slices of a packed projection are fine) -> (ctx [B*Sq, H] f32, lse [B*nh, 256] f32).
    drop = (p, seed, offset, ld_mask): nn.Dropout on the probabilities inside the kernels, attention_drop_fwd_ex's mask contract (lse is
    the undropped softmax's); longer sequences run block by block (never the streaming kernels) and draw the full-sequence mask"""
    require_gpu(q, k, v)
    if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32:
        raise _hip.MuseHipError("attention_x3: f32 operands")
    if not attention_x3_supported(Sq, Skv, hd):
        raise _hip.MuseHipError(f"attention_x3: shape ({Sq} x {Skv}, head_dim {hd}) outside attention_x3_supported")
    if attention_x3_blocked(Sq, Skv):
        return _attention_x3_fwd_blocks(q, k, v, B, Sq, Skv, nh, hd, alpha, drop=drop)
    ctx = torch.empty((B * Sq, nh * hd), dtype=torch.float32, device=q.device)
    lse = torch.empty((B * nh, Sq), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha)
    planes = x3_new_planes(ctx)          # ctx feeds the output projection: its operand planes come out of the kernel
    e0 = _prof_begin()
    if drop is None:
        check(lib().muse_attention_x3_fwd(C.byref(d), lse.data_ptr(), ptr(planes), ctx.numel(), *_image_args(False, planes), stream()), "muse_attention_x3_fwd")
    else:
        check(lib().muse_attention_x3_drop_fwd(C.byref(d), lse.data_ptr(), ptr(planes), ctx.numel(), *_x3_drop(drop, 0, 0, Sq),
                                               *_image_args(False, planes), stream()), "muse_attention_x3_drop_fwd")
    _prof_end(e0, "attn_fwd_bf16x3", 4.0 * B * nh * Sq * Skv * hd)
    x3_put_planes(ctx, planes)
    return ctx, lse


def attention_x3_bwd(q, k, v, ctx, dctx, lse, B, Sq, Skv, nh, hd, alpha, dq=None, dk=None, dv=None, planes=None, planes_only=False, drop=None):
    """-> (dq [B*Sq, H], dk, dv [B*Skv, H]) f32; dq / dk / dv may be views (the column blocks of a packed gradient).
    planes = ((dq_hi, dq_lo_off), (dk_hi, ..), (dv_hi, ..)): hi-plane views shaped / strided like dq / dk / dv and the element distance
    to their lo planes (entries may be None) - the gradients also come out as operand planes (x3_new_planes of the packed tensor).
    planes_only: no f32 gradients at all (dq / dk / dv stay None; the caller wraps the plane tensors: operand_only).
    drop: attention_x3_fwd's - the same masks, drawn again"""
    require_gpu(q, k, v, ctx, dctx, lse)
    H = nh * hd
    planes = planes or (None, None, None)
    if not planes_only:
        dq = dq if dq is not None else torch.empty((B * Sq, H), dtype=torch.float32, device=q.device)
        dk = dk if dk is not None else torch.empty((B * Skv, H), dtype=torch.float32, device=q.device)
        dv = dv if dv is not None else torch.empty((B * Skv, H), dtype=torch.float32, device=q.device)
    elif dq is not None or dk is not None or dv is not None or any(e is None or e[0] is None for e in planes):
        raise _hip.MuseHipError("attention_x3_bwd(planes_only=True): three plane views and no f32 gradient tensors")
    for t in (ctx, dctx, dq, dk, dv):
        if t is not None and t.dtype != torch.float32:
            raise _hip.MuseHipError("attention_x3: f32 operands")
    streamed = attention_x3_streamed(Sq, Skv, drop is not None)
    if attention_x3_blocked(Sq, Skv) and not streamed:
        if planes_only or any(e is not None and e[0] is not None for e in planes):
            raise _hip.MuseHipError("attention_x3_bwd: the block-by-block form (more than 256 query rows or keys) writes f32 gradients, no operand planes")
        return _attention_x3_bwd_blocks(q, k, v, ctx, dctx, lse, B, Sq, Skv, nh, hd, alpha, dq, dk, dv, drop=drop)
    d = _attn_desc(q, k, v, ctx, B, Sq, Skv, nh, hd, alpha)
    pdo, lddo = _row_view(dctx, H)
    e0 = _prof_begin()
    args = []
    pl = []
    for ent, g, rows in zip(planes, (dq, dk, dv), (Sq, Skv, Skv)):
        ref = g if g is not None else ent[0]               # (strides: the f32 view's, or - planes only - the hi-plane view's own)
        pg, ldg = _row_view(ref, H)
        args += [pg if g is not None else None, ldg, rows * ldg]
        if ent is None or ent[0] is None:
            pl += [None, 0]
        else:
            if ent[0].stride() != ref.stride() or ent[0].shape != ref.shape:
                raise _hip.MuseHipError("attention_x3_bwd: a hi-plane view must mirror its gradient view")
            pl += [ent[0].data_ptr(), int(ent[1])]
    img = _image_args(True, *(e[0] for e in planes if e is not None))
    if streamed:
        # dQ per query block over the streamed key blocks (it also leaves dO . O per query in dsum), then dK / dV per key block over the
        # streamed query blocks: every gradient written once (bwd_dq_stream_kernel / bwd_dkv_stream_kernel)
        dsum = torch.empty_like(lse)
        check(lib().muse_attention_x3_bwd_stream(C.byref(d), pdo, lddo, Sq * lddo, lse.data_ptr(), dsum.data_ptr(), *args, *pl, *img, stream()),
              "muse_attention_x3_bwd_stream")
        for t in (dq, dk, dv):
            if t is not None:
                _touched(t)
    elif drop is not None:
        check(lib().muse_attention_x3_drop_bwd(C.byref(d), pdo, lddo, Sq * lddo, lse.data_ptr(), *args, *pl, *_x3_drop(drop, 0, 0, Sq), *img, stream()),
              "muse_attention_x3_drop_bwd")
    else:
        check(lib().muse_attention_x3_bwd(C.byref(d), pdo, lddo, Sq * lddo, lse.data_ptr(), *args, *pl, *img, stream()), "muse_attention_x3_bwd")
    _prof_end(e0, "attn_bwd_bf16x3", 10.0 * B * nh * Sq * Skv * hd)
    return dq, dk, dv


def attention_fwd(qkv, B, S, nh, hd, alpha):
    """fused softmax(alpha q k^T) v; qkv [B*S, 3H] bf16 -> (ctx [B*S, H] bf16, lse [B*nh, seq_pad] f32)"""
    require_gpu(qkv)
    H = nh * hd
    ctx = torch.empty((B * S, H), dtype=qkv.dtype, device=qkv.device)
    sp = lib().muse_attention_seq_pad(S)
    lse = torch.empty((B * nh, sp), dtype=torch.float32, device=qkv.device)
    e0 = _prof_begin()
    check(lib().muse_attention_fwd(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, S, nh, hd, alpha, stream()), "muse_attention_fwd")
    _prof_end(e0, "attn_fwd_bf16", 4.0 * B * nh * S * S * hd)
    return ctx, lse


def attention_bwd(qkv, ctx, dctx, lse, B, S, nh, hd, alpha):
    """-> dqkv [B*S, 3H] bf16"""
    require_gpu(qkv, ctx, dctx, lse)
    dqkv = torch.empty_like(qkv)
    dsum = torch.empty_like(lse)
    e0 = _prof_begin()
    check(lib().muse_attention_bwd(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), dsum.data_ptr(),
                                   dqkv.data_ptr(), B, S, nh, hd, alpha, stream()), "muse_attention_bwd")
    _prof_end(e0, "attn_bwd_bf16", 10.0 * B * nh * S * S * hd)
    return dqkv


X3_PLANES_ONLY = os.environ.get("MUSE_X3_PLANES_ONLY", "1") != "0"   # ... and skip the f32 result where only weight GEMMs read it (ops.OperandOnly)
X3_PRODUCERS = os.environ.get("MUSE_X3_PRODUCERS", "1") != "0"   # bf16x3 mode: kernels whose f32 result feeds a product write its operand planes too
F16_PRODUCERS = os.environ.get("MUSE_F16_PRODUCERS", "1") != "0"  # f16 mode: ... write its half image too (0: every operand through muse_cast_f32_to_f16)


def _x3_producing(t):
    """the running step's image cache when a producer of `t`-like f32 results should write operand planes next to them"""
    return _PASS.producing() if (t.dtype == torch.float32 and t.is_contiguous()) else None


def x3_new_planes(t):
    """[2, *t.shape] bf16 for a producer that writes t's operand planes next to t - None when nothing would read them (no bf16x3 step
    running, the four-plane kernel off, or t no contiguous f32 tensor with whole 16-byte bf16 rows)"""
    im = _x3_producing(t)
    if im is None or t.dim() != 2 or t.shape[1] % 8:
        return None
    return planes_alloc(tuple(t.shape), t.device)


def planes_alloc(shape, device):
    """the operand-image tensor a producer kernel of the running step writes for a [rows, cols] result: [2, rows, cols] bf16 (hi, lo
    planes, "bf16x3" mode) or [1, rows, cols] IEEE half ("f16" mode: _image_args tells the kernels which)"""
    return torch.empty((_PASS.image_planes,) + tuple(shape), dtype=_PASS.image_dtype, device=device)


def x3_put_planes(t, planes):
    if planes is not None:
        _PASS.images.put_planes(t, planes)


def _row_drop(drop):
    """(p, seed, offset) of a dropped row kernel as its C arguments"""
    p, seed, offset = drop
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), but got {p}")
    return float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)


def row_drop_ok(cols):
    """the dropped GLU / GRN kernels take the width: a thread's four consecutive columns are one Philox block"""
    return cols % 4 == 0


def grn_drop_ok(B, S, C_):
    """muse_grn_drop_fwd_ex / _bwd take the shape (their four-channel kernels index an image with 32 bits and walk images in gridDim.y)"""
    return row_drop_ok(C_) and S * (C_ >> 2) < (1 << 31) and B <= 65535


def glu_fwd(ab, planes_only=False, drop=None):
    """planes_only (see planes_only_ok): -> OperandOnly, the result as the running pass's GEMM operand image without its f32 tensor.
    drop = (p, seed, offset): nn.Dropout on the result, drawn inside the kernel (the keep bits of ops.dropout on the [rows, inter] result)"""
    require_gpu(ab)
    rows, two_i = ab.shape
    inter = two_i // 2
    d = () if drop is None else _row_drop(drop)
    if d and not row_drop_ok(inter):          # a width the dropped kernels refuse: the plain kernel, then ops.dropout
        if planes_only:
            raise _hip.MuseHipError("glu_fwd(planes_only=True, drop=) needs inter % 4 == 0")
        h = glu_fwd(ab)
        return dropout(h, *d, out=h)          # (no operand image of the undropped h is registered: inter % 8 != 0 writes none)
    fn = "muse_glu_drop_fwd" if d else "muse_glu_fwd"
    if planes_only:
        if not (planes_only_ok(rows, inter) and ab.dtype == torch.float32 and ab.is_contiguous()):
            raise _hip.MuseHipError("glu_fwd(planes_only=True) outside planes_only_ok")
        h = im = None
    else:
        h = torch.empty((rows, inter), dtype=ab.dtype, device=ab.device)
        im = _x3_producing(ab)
    if planes_only or (im is not None and inter % 8 == 0):
        planes = planes_alloc((rows, inter), ab.device)
        check(getattr(lib(), fn + "_x3")(ab.data_ptr(), ptr(h), planes.data_ptr(), rows, inter, *d, *_image_args(False, planes), stream()), fn + "_x3")
        if planes_only:
            return operand_only(planes, False)
        im.put_planes(h, planes)
        return h
    check(getattr(lib(), fn)(ab.data_ptr(), h.data_ptr(), dt(ab), rows, inter, *d, stream()), fn)
    return h


def glu_bwd(ab, dh, planes_only=False, drop=None):
    """drop = glu_fwd's: the same keep mask, redrawn, multiplies dh before anything else"""
    require_gpu(ab, dh)
    rows, two_i = ab.shape
    inter = two_i // 2
    d = () if drop is None else _row_drop(drop)
    if d and not row_drop_ok(inter):
        return glu_bwd(ab, dropout(dh.contiguous(), *d), planes_only=planes_only)
    fn = "muse_glu_drop_bwd" if d else "muse_glu_bwd"
    if planes_only:
        if not (planes_only_ok(rows, two_i) and ab.dtype == torch.float32 and dh.dtype == torch.float32 and ab.is_contiguous() and dh.is_contiguous()):
            raise _hip.MuseHipError("glu_bwd(planes_only=True) outside planes_only_ok")
        dab = im = None
    else:
        # (only the dropped route refuses these; without drop a non-contiguous dh merely keeps the call off the operand-image kernel)
        if d and (dh.dtype != ab.dtype or not dh.is_contiguous() or not ab.is_contiguous()):
            raise _hip.MuseHipError("glu_bwd(drop=) expects contiguous ab and dh of one dtype")
        dab = torch.empty_like(ab)
        im = _x3_producing(ab)
    if planes_only or (im is not None and dh.dtype == torch.float32 and dh.is_contiguous() and two_i % 16 == 0):
        planes = planes_alloc((rows, two_i), ab.device)
        check(getattr(lib(), fn + "_x3")(ab.data_ptr(), dh.data_ptr(), ptr(dab), planes.data_ptr(), rows, inter, *d, *_image_args(True, planes), stream()),
              fn + "_x3")
        if planes_only:
            return operand_only(planes, True)
        im.put_planes(dab, planes)
        return dab
    check(getattr(lib(), fn)(ab.data_ptr(), dh.data_ptr(), dab.data_ptr(), dt(ab), rows, inter, *d, stream()), fn)
    return dab


def ffn_mid_fwd(ab, w, eps, keep_h=True):
    """fused GLU + mid LayerNorm: ab [rows, 2I] -> (h, hm, mean, rstd).  keep_h=False: h = gelu(a) * b is not written (h is None);
    ffn_mid_bwd then recomputes it from ab, bit for bit."""
    require_gpu(ab, w)
    rows, two_i = ab.shape
    inter = two_i // 2
    h = torch.empty((rows, inter), dtype=ab.dtype, device=ab.device) if keep_h else None
    hm = torch.empty((rows, inter), dtype=ab.dtype, device=ab.device)
    mean = torch.empty(rows, dtype=torch.float32, device=ab.device)
    rstd = torch.empty_like(mean)
    e0 = _prof_begin()
    check(lib().muse_ffn_mid_fwd(ab.data_ptr(), w.data_ptr(), ptr(h), hm.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 dt(ab), rows, inter, eps, stream()), "muse_ffn_mid_fwd")
    _prof_end(e0, "ffn_mid_fwd", _nbytes(ab, h, hm), "byte")
    return h, hm, mean, rstd


def ffn_mid_bwd(dhm, h, ab, w, mean, rstd, dw, accumulate, colsum_queue=None):
    """fused mid-LayerNorm backward + GLU backward: -> dab [rows, 2I]; dw (+)= column sums of dhm * xhat.  h may be None (see
    ffn_mid_fwd keep_h=False): it is then recomputed from ab."""
    require_gpu(dhm, ab, w)
    rows, inter = dhm.shape
    dab = torch.empty_like(ab)
    rpb = lib().muse_ffn_mid_rows_per_block()
    nblk = (rows + rpb - 1) // rpb
    part = torch.empty((nblk, inter), dtype=torch.float32, device=dhm.device)
    e0 = _prof_begin()
    check(lib().muse_ffn_mid_bwd(dhm.data_ptr(), ptr(h), ab.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 dab.data_ptr(), part.data_ptr(), dt(dhm), rows, inter, stream()), "muse_ffn_mid_bwd")
    _colsum_or_defer(part, dw, nblk, inter, accumulate, colsum_queue)
    _prof_end(e0, "ffn_mid_bwd", _nbytes(dhm, h, ab, dab), "byte")
    return dab


def gelu_fwd(x):
    require_gpu(x)
    y = torch.empty_like(x)
    check(lib().muse_gelu_fwd(x.data_ptr(), y.data_ptr(), dt(x), x.numel(), stream()), "muse_gelu_fwd")
    return y


def gelu_bwd(x, dy, out_dtype=None):
    """out_dtype=torch.bfloat16 with f32 x / dy: the result written directly as the bf16 operand of the next weight GEMMs"""
    require_gpu(x, dy)
    if out_dtype == torch.bfloat16 and x.dtype == torch.float32 and dy.dtype == torch.float32:
        dx = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        check(lib().muse_gelu_bwd_f32_bf16(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), stream()), "muse_gelu_bwd_f32_bf16")
        return dx
    dx = torch.empty_like(x)
    check(lib().muse_gelu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), dt(x), x.numel(), stream()), "muse_gelu_bwd")
    return dx


def embed_fwd(ids, word, pos):
    require_gpu(ids, word, pos)
    B, S = ids.shape
    V, H = word.shape
    out = torch.empty((B * S, H), dtype=torch.float32, device=ids.device)
    check(lib().muse_embed_fwd(ids.data_ptr(), word.data_ptr(), pos.data_ptr(), out.data_ptr(), B, S, H, V, stream()), "muse_embed_fwd")
    return out


EMBED_BWD_SORT = os.environ.get("MUSE_EMBED_BWD_SORT", "1") != "0"   # 0: the scan-per-row kernel (muse_embed_bwd)


def embed_bwd(ids, dout, dword, dpos, accumulate):
    """dword[v] (+)= sum of dout rows whose token id is v (position order), dpos[s] (+)= sum over the batch"""
    require_gpu(ids, dout, dword, dpos)
    B, S = ids.shape
    V, H = dword.shape
    if EMBED_BWD_SORT:
        nb = lib().muse_embed_bwd2_scratch_bytes(B, S, H, V)
        if nb < 0:
            raise _hip.MuseHipError("muse_embed_bwd2_scratch_bytes failed")
        scratch = torch.empty(nb, dtype=torch.uint8, device=ids.device)   # (the caching allocator hands out 512-byte aligned blocks)
        check(lib().muse_embed_bwd2(ids.data_ptr(), dout.data_ptr(), dword.data_ptr(), dpos.data_ptr(), scratch.data_ptr(), nb, B, S, H,
                                    V, 1 if accumulate else 0, stream()), "muse_embed_bwd2")
        return
    n = lib().muse_embed_bwd_scratch_floats(H, V)
    scratch = torch.empty(n, dtype=torch.float32, device=ids.device)
    check(lib().muse_embed_bwd(ids.data_ptr(), dout.data_ptr(), dword.data_ptr(), dpos.data_ptr(), scratch.data_ptr(), B, S, H,
                               V, 1 if accumulate else 0, stream()), "muse_embed_bwd")


def cross_entropy_fwd(logits, labels, label_smoothing, vocab=None, want_rows=False):
    """logits [rows, ld] with the first `vocab` columns valid; returns (loss_out[2] = (mean loss, n_valid), lse[rows])"""
    require_gpu(logits, labels)
    rows = logits.shape[0]
    V = vocab or logits.shape[1]
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    loss_out = torch.empty(2, dtype=torch.float32, device=logits.device)
    check(lib().muse_cross_entropy_fwd(logits.data_ptr(), dt(logits), labels.data_ptr(), row_loss.data_ptr(), lse.data_ptr(),
                                       loss_out.data_ptr(), rows, V, logits.stride(0), label_smoothing, stream()),
          "muse_cross_entropy_fwd")
    if want_rows:
        return loss_out, lse, row_loss   # row_loss[r] = 0 for ignored rows (reduction="none" semantics)
    return loss_out, lse


def _logit_rows(what, logits, vocab):
    """(rows, V, ld) of a [rows, cols] logits tensor the diagnostics kernels read in place: unit last stride, V <= cols, V <= ld"""
    require_gpu(logits)
    dt(logits)
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise _hip.MuseHipError(f"{what}: logits must be [rows, cols] with rows, cols >= 1, got {tuple(logits.shape)}")
    if logits.stride(1) != 1:
        raise _hip.MuseHipError(f"{what}: the last stride of logits must be 1, got {logits.stride(1)}")
    rows, cols = logits.shape
    V = cols if vocab is None else int(vocab)
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), cols)
    if not 1 <= V <= cols or V > ld:
        raise _hip.MuseHipError(f"{what}: vocab {V} does not fit rows of {cols} columns with row stride {ld}")
    return rows, V, ld


def token_stats(logits, vocab=None, row_mask=None, want_max_sum=False):
    """logits [rows, cols] (f32 / bf16, last stride 1, any row stride: a sliced view goes in as it is), first `vocab` columns valid ->
    (lse [rows], entropy [rows]) f32 from one read of each row, and with want_max_sum also (row_max [rows], sum_exp [rows]) - the row
    maximum m and sum of exp(x - m) that lse = m + log(sum) is made of, which masked_mean_probs takes.  row_mask (bool / uint8
    [rows]): rows whose entry is 0 are not loaded, their entropy is 0 and their other results unspecified.  Nothing is written but
    the results."""
    rows, V, ld = _logit_rows("token_stats", logits, vocab)
    if row_mask is not None:
        require_gpu(row_mask)
        if row_mask.dtype not in (torch.bool, torch.uint8) or row_mask.numel() != rows or not row_mask.is_contiguous():
            raise _hip.MuseHipError("token_stats: row_mask must be a contiguous bool / uint8 tensor with one entry per row")
    out = torch.empty((4 if want_max_sum else 2, rows), dtype=torch.float32, device=logits.device)
    e0 = _prof_begin()
    check(lib().muse_token_stats(logits.data_ptr(), dt(logits), ptr(row_mask), out[0].data_ptr(), out[1].data_ptr(),
                                 out[2].data_ptr() if want_max_sum else None, out[3].data_ptr() if want_max_sum else None, rows, V, ld,
                                 stream()), "muse_token_stats")
    _prof_end(e0, "token_stats", float(rows) * V * _esz(logits) + _nbytes(out), "byte")   # an upper bound under a row_mask
    return tuple(out.unbind(0))


def masked_row_mean(values, input_ids, mask_id):
    """values f32 [B, S] contiguous (token_stats' entropies: exact zeros where not masked), input_ids int64 [B, S] -> f32 [B]: the row
    sums over the images' masked counts, in a fixed order per image (the same bits in any batch); NaN for an image without a masked token"""
    require_gpu(values, input_ids)
    if (values.dtype != torch.float32 or input_ids.dtype != torch.long or input_ids.dim() != 2 or values.shape != input_ids.shape
            or not values.is_contiguous() or not input_ids.is_contiguous()):
        raise _hip.MuseHipError("masked_row_mean: values f32 and input_ids int64 must be contiguous [B, S] tensors of one shape")
    B, S = input_ids.shape
    out = torch.empty(B, dtype=torch.float32, device=values.device)
    check(lib().muse_masked_row_mean(values.data_ptr(), input_ids.data_ptr(), out.data_ptr(), B, S, int(mask_id), stream()),
          "muse_masked_row_mean")
    return out


def masked_mean_probs(logits, input_ids, row_max, sum_exp, mask_id, vocab=None, want_entropy=True):
    """logits [B * S, cols] as for token_stats, input_ids int64 [B, S], (row_max, sum_exp) f32 [B * S] from token_stats(...,
    want_max_sum=True), valid for at least the masked rows -> (mean_probs f32 [B, vocab], entropy f32 [B] or None): per image the mean
    of softmax(logits) over its masked tokens (rows added in ascending order, unmasked rows not loaded) and -sum(mean_probs *
    log(mean_probs)); NaN for an image with no masked token and for a mean probability of exactly 0, as the reference's expression"""
    rows, V, ld = _logit_rows("masked_mean_probs", logits, vocab)
    require_gpu(input_ids, row_max, sum_exp)
    if input_ids.dim() != 2 or input_ids.dtype != torch.long or not input_ids.is_contiguous() or input_ids.numel() != rows:
        raise _hip.MuseHipError("masked_mean_probs: input_ids must be a contiguous int64 [B, S] with B * S = the logits' rows")
    for t in (row_max, sum_exp):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != rows:
            raise _hip.MuseHipError("masked_mean_probs: row_max and sum_exp must be contiguous f32 tensors with one entry per row")
    B, S = input_ids.shape
    mean = torch.empty((B, V), dtype=torch.float32, device=logits.device)
    ent = torch.empty(B, dtype=torch.float32, device=logits.device) if want_entropy else None
    e0 = _prof_begin()
    check(lib().muse_masked_mean_probs(logits.data_ptr(), dt(logits), input_ids.data_ptr(), row_max.data_ptr(), sum_exp.data_ptr(),
                                       mean.data_ptr(), ptr(ent), B, S, V, ld, int(mask_id), stream()), "muse_masked_mean_probs")
    _prof_end(e0, "masked_mean_probs", float(rows) * V * _esz(logits) + 8.0 * B * V, "byte")   # an upper bound: masked rows only
    return mean, ent


def cross_entropy_bwd(logits, labels, lse, loss_out, grad_out, label_smoothing, out_dtype, vocab=None):
    """dlogits has the same (padded) row stride as logits; pad columns are written as zeros."""
    require_gpu(logits, labels, grad_out)
    rows = logits.shape[0]
    V = vocab or logits.shape[1]
    dl = torch.empty((rows, logits.shape[1]), dtype=out_dtype, device=logits.device)
    check(lib().muse_cross_entropy_bwd(logits.data_ptr(), dt(logits), labels.data_ptr(), lse.data_ptr(), loss_out.data_ptr(),
                                       grad_out.data_ptr(), dl.data_ptr(), dt(dl), rows, V, logits.stride(0), label_smoothing,
                                       stream()), "muse_cross_entropy_bwd")
    return dl


def _soft_ce_check(logits, labels, soft, seq1):
    require_gpu(logits, labels, soft)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype != torch.float32:
        raise _hip.MuseHipError("soft_ce: logits must be f32 [rows, ld] with unit column stride")
    rows, K = logits.shape[0], soft.shape[-1]
    if (labels.dtype != torch.int64 or not labels.is_contiguous() or labels.numel() != rows or soft.dtype != torch.float32
            or not soft.is_contiguous() or seq1 < 2 or rows % seq1 or soft.numel() != rows // seq1 * (seq1 - 1) * K
            or K > logits.shape[1]):
        raise _hip.MuseHipError(f"soft_ce: labels int64 [{rows}] and soft f32 [B*S, K <= {logits.shape[1]}] expected, got "
                           f"{labels.dtype} {tuple(labels.shape)} / {soft.dtype} {tuple(soft.shape)} with S + 1 = {seq1}")
    return rows, K


def soft_ce_fwd(logits, labels, soft, seq1):
    """soft-target cross entropy over the first K = soft.shape[-1] columns of logits [B*seq1, ld] (row stride ld; position 0 of every
    sequence and label -100 rows are left out) -> (loss_out[2] = (mean loss, n_active), lse[rows], psum[rows])"""
    rows, K = _soft_ce_check(logits, labels, soft, seq1)
    dev = logits.device
    row_loss = torch.empty(rows, dtype=torch.float32, device=dev)
    lse = torch.empty(rows, dtype=torch.float32, device=dev)
    psum = torch.empty(rows, dtype=torch.float32, device=dev)
    loss_out = torch.empty(2, dtype=torch.float32, device=dev)
    check(lib().muse_soft_ce_fwd(logits.data_ptr(), labels.data_ptr(), soft.data_ptr(), row_loss.data_ptr(), lse.data_ptr(),
                                 psum.data_ptr(), loss_out.data_ptr(), rows, seq1, K, logits.stride(0), stream()), "muse_soft_ce_fwd")
    return loss_out, lse, psum


def soft_ce_bwd(logits, labels, soft, seq1, lse, psum, loss_out, grad_out, out_dtype=torch.float32, width=None):
    """d(loss)/d(logits) of soft_ce_fwd as a new [rows, width] tensor (width defaults to logits' column count): the gradient on the
    first K columns of active rows, exact zeros everywhere else.  grad_out: the incoming scalar gradient, on the device."""
    rows, K = _soft_ce_check(logits, labels, soft, seq1)
    require_gpu(lse, psum, loss_out, grad_out)
    width = logits.shape[1] if width is None else int(width)
    if width < K:
        raise _hip.MuseHipError(f"soft_ce_bwd: output width {width} < K = {K}")
    dl = torch.empty((rows, width), dtype=out_dtype, device=logits.device)
    check(lib().muse_soft_ce_bwd(logits.data_ptr(), labels.data_ptr(), soft.data_ptr(), lse.data_ptr(), psum.data_ptr(),
                                 loss_out.data_ptr(), grad_out.data_ptr(), dl.data_ptr(), dt(dl), rows, seq1, K, logits.stride(0),
                                 width, stream()), "muse_soft_ce_bwd")
    return dl


# skip (every adamw_*): None, or the device int32 overflow counter of an "f16" backward pass - the kernel leaves parameters and moments
# untouched when it is non-zero (training.FusedAdamW's guard)
# scale_dev (every adamw_*): None, or a device f32 (gradnorm_finalize's `scale`) the kernel multiplies the gradient by INSTEAD of
# grad_scale (the muse_adamw_*_dev entry points: gradient clipping without a host round trip)
def _adamw_call(name, args, grad_scale, skip, scale_dev, prof=None):
    """muse_<name> (the host's grad_scale) or muse_<name>_dev (scale_dev), AdamW and Lion alike; prof: the parameter tensor and its bf16
    copy, to report to the profiler (28 B per element of state traffic for adamw_*, 20 B for lion_*)"""
    what, per = ("lion", 20.0) if name.startswith("lion") else ("adamw", 28.0)
    name = "muse_" + name + ("_dev" if scale_dev is not None else "")
    e0 = _prof_begin() if prof else None
    check(getattr(lib(), name)(*args, float(grad_scale) if scale_dev is None else scale_dev.data_ptr(), ptr(skip), stream()), name)
    if prof:
        _prof_end(e0, what, per * prof[0].numel() + (2.0 * prof[0].numel() if prof[1] is not None else 0.0), "byte")


def adamw_flat(p, g, m, v, p_bf16, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, skip=None, scale_dev=None):
    require_gpu(p, g, m, v, scale_dev)
    _adamw_call("adamw_flat", (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(p_bf16), p.numel(), lr, beta1, beta2, eps,
                               weight_decay, step), grad_scale, skip, scale_dev, prof=(p, p_bf16))


def adamw_multi(table, chunk_first, num_tensors, num_chunks, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, skip=None,
                scale_dev=None):
    """one AdamW launch over a device-side table of tensors (muse_adamw_multi; training.FusedAdamW builds the table)"""
    require_gpu(table, chunk_first, scale_dev)
    _adamw_call("adamw_multi", (table.data_ptr(), chunk_first.data_ptr(), int(num_tensors), int(num_chunks), lr, beta1, beta2, eps,
                                weight_decay, step), grad_scale, skip, scale_dev)


def ema_multi(table, chunk_first, num_tensors, num_chunks, one_minus_decay):
    """shadow -= (1 - decay) * (shadow - param) over a device-side table of tensors in one launch (muse_ema_multi; muse.EMAModel builds
    the table)"""
    require_gpu(table, chunk_first)
    check(lib().muse_ema_multi(table.data_ptr(), chunk_first.data_ptr(), int(num_tensors), int(num_chunks), float(one_minus_decay), stream()),
          "muse_ema_multi")


def _group_hyper(groups):
    """host array of {lr, beta1, beta2, eps, weight_decay} rows for muse_adamw_*_groups (kept alive by the caller for the call)"""
    import ctypes
    if not 1 <= len(groups) <= 8:
        raise _hip.MuseHipError(f"FusedAdamW: 1..8 parameter groups are supported, got {len(groups)}")
    flat = []
    for g in groups:
        flat += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])]
    return (ctypes.c_float * len(flat))(*flat)


def adamw_flat_groups(p, g, m, v, p_bf16, base, seg_end, seg_group, groups, step, grad_scale=1.0, skip=None, scale_dev=None):
    """AdamW on elements [base, base + p.numel()) of a flat buffer whose segments belong to different parameter groups
    (muse_adamw_flat_groups); p, g, m, v, p_bf16 are the slices starting at `base`; `groups`: torch param_groups-like dicts"""
    require_gpu(p, g, m, v, seg_end, seg_group, scale_dev)
    import ctypes
    hy = _group_hyper(groups)
    _adamw_call("adamw_flat_groups", (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(p_bf16), p.numel(), int(base),
                                      seg_end.data_ptr(), seg_group.data_ptr(), int(seg_end.numel()), ctypes.cast(hy, ctypes.c_void_p),
                                      len(groups), int(step)), grad_scale, skip, scale_dev, prof=(p, p_bf16))


def adamw_multi_groups(table, chunk_first, num_tensors, num_chunks, groups, step, grad_scale=1.0, skip=None, scale_dev=None):
    """muse_adamw_multi with a group column in the table (7 x int64 per tensor)"""
    require_gpu(table, chunk_first, scale_dev)
    import ctypes
    hy = _group_hyper(groups)
    _adamw_call("adamw_multi_groups", (table.data_ptr(), chunk_first.data_ptr(), int(num_tensors), int(num_chunks),
                                       ctypes.cast(hy, ctypes.c_void_p), len(groups), int(step)), grad_scale, skip, scale_dev)


# Lion (training/optimizer.py of the reference; muse_lion_*): the adamw_* forms without eps, step and v.  grad_scale, skip and scale_dev as
# above.  The hyper-parameters go down as DOUBLE rows {lr, beta1, beta2, weight_decay}: the kernel's constants are rounded once, from the
# Python floats (f32(1 - lr * wd) is not computable from an f32 lr).
def _lion_hyper(groups):
    """host array of {lr, beta1, beta2, weight_decay} double rows for muse_lion_* (kept alive by the caller for the call)"""
    import ctypes
    if not 1 <= len(groups) <= 8:
        raise _hip.MuseHipError(f"FusedLion: 1..8 parameter groups are supported, got {len(groups)}")
    flat = []
    for g in groups:
        flat += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["weight_decay"])]
    return (ctypes.c_double * len(flat))(*flat)


def _lion_row(lr, beta1, beta2, weight_decay):
    return _lion_hyper([dict(lr=lr, betas=(beta1, beta2), weight_decay=weight_decay)])


def lion_flat(p, g, m, p_bf16, lr, beta1, beta2, weight_decay, grad_scale=1.0, skip=None, scale_dev=None):
    require_gpu(p, g, m, scale_dev)
    import ctypes
    hy = _lion_row(lr, beta1, beta2, weight_decay)
    _adamw_call("lion_flat", (p.data_ptr(), g.data_ptr(), m.data_ptr(), ptr(p_bf16), p.numel(), ctypes.cast(hy, ctypes.c_void_p)),
                grad_scale, skip, scale_dev, prof=(p, p_bf16))


def lion_multi(table, chunk_first, num_tensors, num_chunks, lr, beta1, beta2, weight_decay, grad_scale=1.0, skip=None, scale_dev=None):
    """one Lion launch over a device-side table of tensors (muse_lion_multi: adamw_multi's 6-column table, column 3 ignored)"""
    require_gpu(table, chunk_first, scale_dev)
    import ctypes
    hy = _lion_row(lr, beta1, beta2, weight_decay)
    _adamw_call("lion_multi", (table.data_ptr(), chunk_first.data_ptr(), int(num_tensors), int(num_chunks), ctypes.cast(hy, ctypes.c_void_p)),
                grad_scale, skip, scale_dev)


def lion_flat_groups(p, g, m, p_bf16, base, seg_end, seg_group, groups, grad_scale=1.0, skip=None, scale_dev=None):
    """Lion on elements [base, base + p.numel()) of a flat buffer cut into parameter-group segments (muse_lion_flat_groups; arguments as for
    adamw_flat_groups)"""
    require_gpu(p, g, m, seg_end, seg_group, scale_dev)
    import ctypes
    hy = _lion_hyper(groups)
    _adamw_call("lion_flat_groups", (p.data_ptr(), g.data_ptr(), m.data_ptr(), ptr(p_bf16), p.numel(), int(base), seg_end.data_ptr(),
                                     seg_group.data_ptr(), int(seg_end.numel()), ctypes.cast(hy, ctypes.c_void_p), len(groups)),
                grad_scale, skip, scale_dev, prof=(p, p_bf16))


def lion_multi_groups(table, chunk_first, num_tensors, num_chunks, groups, grad_scale=1.0, skip=None, scale_dev=None):
    """muse_lion_multi with a group column in the table (7 x int64 per tensor, as for adamw_multi_groups)"""
    require_gpu(table, chunk_first, scale_dev)
    import ctypes
    hy = _lion_hyper(groups)
    _adamw_call("lion_multi_groups", (table.data_ptr(), chunk_first.data_ptr(), int(num_tensors), int(num_chunks),
                                      ctypes.cast(hy, ctypes.c_void_p), len(groups)), grad_scale, skip, scale_dev)


# ---- gradient clipping by global L2 norm / per-parameter gradient norms (csrc/gradnorm.hip; training.GradNorm drives these) -------------
GRADNORM_CHUNK = 4096     # elements per f64 partial, counted from each parameter's own start (GN_CHUNK of csrc/gradnorm.hip, the AdamW chunk)


def chunk_first(sizes):
    """the chunk tables of the chunked multi-tensor kernels (AdamW, EMA, gradient norm): exclusive prefix sum of ceil(n / GRADNORM_CHUNK)
    over the tensors' element counts -> (list of len(sizes) + 1 entries, total number of chunks)"""
    first = [0]
    for n in sizes:
        first.append(first[-1] + (n + GRADNORM_CHUNK - 1) // GRADNORM_CHUNK)
    return first, first[-1]


def gradnorm_flat(g_flat, base, n, ptab_host, chunk_first_host, ptab, chunk_first, slab):
    """sums of squares of the parameters inside [base, base + n) of the flat f32 gradient buffer `g_flat` (the WHOLE buffer) -> their
    chunks of `slab` (f64).  ptab {offset, n} int64 rows and chunk_first int32, on the device and (`*_host`) on the host.  A range that
    does not begin at a parameter or cuts one raises (MUSE_ERR_BAD_ARG)."""
    require_gpu(g_flat, ptab, chunk_first, slab)
    if ptab_host.is_cuda or chunk_first_host.is_cuda:
        raise _hip.MuseHipError("gradnorm_flat: ptab_host / chunk_first_host are host tensors")
    e0 = _prof_begin()
    check(lib().muse_gradnorm_flat(g_flat.data_ptr(), int(base), int(n), ptab_host.data_ptr(), chunk_first_host.data_ptr(), ptab.data_ptr(),
                                   chunk_first.data_ptr(), int(ptab_host.shape[0]), slab.data_ptr(), stream()), "muse_gradnorm_flat")
    _prof_end(e0, "gradnorm", 4.0 * n, "byte")


def gradnorm_multi(table, chunk_first, num_tensors, num_chunks, slab):
    """the same over FusedAdamW's device pointer table ({p, g, m, v, shadow, n[, group]} rows): every tensor in one launch"""
    require_gpu(table, chunk_first, slab)
    check(lib().muse_gradnorm_multi(table.data_ptr(), int(table.shape[1]), chunk_first.data_ptr(), int(num_tensors), int(num_chunks),
                                    slab.data_ptr(), stream()), "muse_gradnorm_multi")


def gradnorm_finalize(slab, chunk_first, num_tensors, psum, grad_scale, max_norm, out):
    """slab -> out (f32 [3 + num_tensors]): norm, coef = min(1, max_norm / (norm + 1e-6)), scale = grad_scale * coef, per-parameter norms"""
    require_gpu(slab, chunk_first, psum, out)
    check(lib().muse_gradnorm_finalize(slab.data_ptr(), chunk_first.data_ptr(), int(num_tensors), psum.data_ptr(), float(grad_scale),
                                       float(max_norm), out.data_ptr(), stream()), "muse_gradnorm_finalize")


def grad_scale_flat_(g, scale):
    """g *= scale (a device f32) in place"""
    require_gpu(g, scale)
    check(lib().muse_grad_scale_flat(g.data_ptr(), g.numel(), scale.data_ptr(), stream()), "muse_grad_scale_flat")


def grad_scale_multi_(table, chunk_first, num_tensors, num_chunks, scale):
    """every gradient of the pointer table *= scale (a device f32) in place, one launch"""
    require_gpu(table, chunk_first, scale)
    check(lib().muse_grad_scale_multi(table.data_ptr(), int(table.shape[1]), chunk_first.data_ptr(), int(num_tensors), int(num_chunks),
                                      scale.data_ptr(), stream()), "muse_grad_scale_multi")


def cast_to_bf16(src, dst=None):
    require_gpu(src)
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    check(lib().muse_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), stream()), "muse_cast_f32_to_bf16")
    return dst


def cast_to_f32(src, dst=None):
    require_gpu(src)
    given = dst is not None
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    check(lib().muse_cast_bf16_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream()), "muse_cast_bf16_to_f32")
    return _touched(dst) if given else dst


def mask_sample(tokens, class_ids, timesteps, noise, mask_id, codebook_size, min_masking_rate=0.0):
    require_gpu(tokens, class_ids, timesteps, noise)
    B, S = tokens.shape
    input_ids = torch.empty((B, S + 1), dtype=torch.int64, device=tokens.device)
    labels = torch.empty((B, S + 1), dtype=torch.int64, device=tokens.device)
    mask_prob = torch.empty(B, dtype=torch.float32, device=tokens.device)
    check(lib().muse_mask_sample(tokens.data_ptr(), class_ids.data_ptr(), timesteps.data_ptr(), noise.data_ptr(),
                                 input_ids.data_ptr(), labels.data_ptr(), mask_prob.data_ptr(), B, S, mask_id, codebook_size,
                                 min_masking_rate, stream()), "muse_mask_sample")
    return input_ids, labels, mask_prob


def sample_step(cond_logits, input_ids, mask_id, vocab, temperature, sched_mask_len, *, uncond_logits=None, guidance_scale=0.0,
                noise_exp=None, noise_u=None, seed=0, step=0, want_raw=False, top_k=None, top_p=None, want_cutoff=False):
    """one MaskGit decoding iteration (muse_sample_step): cond_logits [B, S, >= vocab] f32 view (last dim contiguous; a slice
    that skips the class-token row is fine) -> (sampled [B,S], next_input_ids [B,S], raw samples or None)

    Truncated sampling (muse_sample_step_filtered, taken when top_k or top_p is not None; vocab <= 16384), with l_j the logit of
    code j < vocab after the guidance mix, rounded exactly as the plain step rounds it:
      top_k (integer, 1 <= top_k): keep j iff l_j >= v_k, v_k the k-th largest value of the row; all ties at v_k are kept;
        top_k >= vocab means off.
      top_p (float, 0 < top_p <= 1): with p_j = softmax(l)_j over the codes that survive top_k, keep j iff the mass strictly above
        it, M_gt(j) = sum over {i : l_i > l_j} of p_i, is < top_p; a group of tied logits is kept or dropped as a whole; the largest
        logit is always kept; top_p == 1 means off.
      Both given: top_k first, then the nucleus over the distribution renormalised on the top-k set.
      Filtered codes behave exactly as if their logit were -inf before the step.
    Both filters reduce to one per-row cutoff tau, the kept set being {j : l_j >= tau}; want_cutoff appends tau [B, S] f32 (-inf for
    a row with both filters off) to the returned tuple."""
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1):
        raise ValueError(f"sample_step: top_k must be an integer >= 1, got {top_k!r}")
    if top_p is not None and not (isinstance(top_p, (int, float)) and not isinstance(top_p, bool) and 0.0 < top_p <= 1.0):
        raise ValueError(f"sample_step: top_p must lie in (0, 1], got {top_p!r}")
    filtered = top_k is not None or top_p is not None
    if want_cutoff and not filtered:
        raise ValueError("sample_step: want_cutoff needs top_k or top_p (top_k=vocab / top_p=1.0 turn a filter off)")
    require_gpu(cond_logits, input_ids)
    B, S = input_ids.shape

    def layout(t):
        if t.dim() != 3 or t.shape[0] != B or t.shape[1] != S or t.stride(2) != 1 or t.dtype != torch.float32 or t.shape[2] < vocab:
            raise _hip.MuseHipError("sample_step: logits must be a float32 [B, S, >= vocab] view with a contiguous last dim")
        return t.stride(0), t.stride(1)

    lay = layout(cond_logits)
    if uncond_logits is not None and layout(uncond_logits) != lay:
        raise _hip.MuseHipError("sample_step: cond / uncond logits must share a layout")
    ids = input_ids.contiguous()
    sampled, nxt = torch.empty_like(ids), torch.empty_like(ids)
    raw = torch.empty_like(ids) if want_raw else None
    conf = torch.empty(B * S, dtype=torch.float32, device=ids.device)
    if noise_exp is not None:
        noise_exp = noise_exp.reshape(B * S, vocab).to(device=ids.device, dtype=torch.float32).contiguous()
    if noise_u is not None:
        noise_u = noise_u.reshape(B * S).to(device=ids.device, dtype=torch.float32).contiguous()
    args = (cond_logits.data_ptr(), ptr(uncond_logits), float(guidance_scale), lay[0], lay[1], int(vocab), ids.data_ptr(), int(mask_id),
            ptr(noise_exp), ptr(noise_u), int(seed) & (2 ** 64 - 1), int(step), float(temperature), int(sched_mask_len), B, S, ptr(raw),
            sampled.data_ptr(), nxt.data_ptr(), conf.data_ptr())
    if not filtered:
        check(lib().muse_sample_step(*args, stream()), "muse_sample_step")
        return sampled, nxt, raw
    cutoff = torch.empty((B, S), dtype=torch.float32, device=ids.device) if want_cutoff else None
    k = 2 ** 31 - 1 if top_k is None else min(top_k, 2 ** 31 - 1)
    check(lib().muse_sample_step_filtered(*args, k, 1.0 if top_p is None else float(top_p), ptr(cutoff), stream()),
          "muse_sample_step_filtered")
    return (sampled, nxt, raw, cutoff) if want_cutoff else (sampled, nxt, raw)


def mask_tokens(tokens, mask_id, *, timesteps=None, mask_prob=None, noise=None, rects=None, min_masking_rate=0.0, all_labels=False,
                want_weight=False, weight_min=0.3):
    """training/train_muse.py:149-226 on the device -> (input_ids, labels, loss_weight or None, mask_prob)"""
    require_gpu(tokens)
    B, S = tokens.shape
    dev = tokens.device
    tokens = tokens.contiguous()
    input_ids, labels = torch.empty_like(tokens), torch.empty_like(tokens)
    lw = torch.empty((B, S), dtype=torch.float32, device=dev) if want_weight else None
    mp = torch.empty(B, dtype=torch.float32, device=dev)
    f = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()   # noqa: E731
    timesteps, mask_prob, noise = f(timesteps), f(mask_prob), f(noise)
    if rects is not None:
        rects = rects.to(device=dev, dtype=torch.int32).contiguous()
    check(lib().muse_mask_tokens(tokens.data_ptr(), ptr(timesteps), ptr(mask_prob), ptr(noise), ptr(rects), input_ids.data_ptr(),
                                 labels.data_ptr(), ptr(lw), mp.data_ptr(), B, S, int(mask_id), float(min_masking_rate),
                                 1 if all_labels else 0, float(weight_min), stream()), "muse_mask_tokens")
    return input_ids, labels, lw, mp


def dropout(x, p, seed, offset, out=None):
    """y = x * keep / (1 - p) with the Philox keep-mask of (seed, offset); the same call on a gradient is the backward.
    `out` may be x (in place)."""
    require_gpu(x)
    if not x.is_contiguous():
        raise _hip.MuseHipError("dropout expects a contiguous tensor")
    y = out if out is not None else torch.empty_like(x)
    check(lib().muse_dropout(x.data_ptr(), y.data_ptr(), dt(x), x.numel(), float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                             stream()), "muse_dropout")
    return _touched(y) if out is not None else y


def cond_dropout(x, empty, uniforms, prob):
    """training/train_muse.py:715-731: x [B, ...] f32, empty [...] (one image's worth), uniforms [B]"""
    require_gpu(x, empty, uniforms)
    B = x.shape[0]
    xc = x.float().contiguous()
    per = xc.numel() // B
    e = empty.float().contiguous()
    if e.numel() != per:
        raise _hip.MuseHipError("cond_dropout: the empty embedding must have the shape of one batch element")
    out = torch.empty_like(xc)
    check(lib().muse_cond_dropout(xc.data_ptr(), e.data_ptr(), uniforms.float().contiguous().data_ptr(), out.data_ptr(), B, per,
                                  float(prob), stream()), "muse_cond_dropout")
    return out


# ---- VQGAN (NHWC) ----------------------------------------------------------------------------------------------
def conv2d_nhwc(x, w, B, H, W, Cin, Cout, KS, bias=None, residual=None, upsample=False):
    """x: [B, Hin, Win, Cin], w: [Cout, KS, KS, Cin]; returns [B, H, W, Cout].  upsample: False / 0 = stride 1 (Hin = H);
    True / 1 = nearest x2 upsample folded in (Hin = H/2);  2 = stride-2 3x3 over the bottom/right zero-padded input (Hin = 2H)."""
    require_gpu(x, w)
    out = torch.empty((B, H, W, Cout), dtype=x.dtype, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_conv2d_nhwc(x.data_ptr(), w.data_ptr(), ptr(bias), ptr(residual), out.data_ptr(), dt(x), B, H, W, Cin,
                                 Cout, KS, int(upsample), stream()), "muse_conv2d_nhwc")
    _prof_end(e0, f"conv_{'bf16' if x.dtype == torch.bfloat16 else 'f32'}", 2.0 * B * H * W * Cout * KS * KS * Cin)
    return out


def split_bf16(w):
    """f32 -> (hi, lo) bf16 with w ~= hi + lo (weights of the bf16x3 convolution; one-time packing)"""
    hi = cast_to_bf16(w.contiguous())
    lo = cast_to_bf16((w - cast_to_f32(hi)).contiguous())
    return hi, lo


def conv2d_nhwc_split(x, w_hi, w_lo, B, H, W, Cin, Cout, KS, bias=None, residual=None, upsample=False, gn_groups=0):
    """f32 NHWC convolution as 3 bf16 MFMAs per product (see muse_conv2d_nhwc_split).  gn_groups > 0: the epilogue also
    leaves the GroupNorm statistics of the output on the returned tensor (`out._gn_stats = (partial, nchunk)`)."""
    require_gpu(x, w_hi, w_lo)
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    part, nchunk = None, 0
    cpg = Cout // gn_groups if gn_groups else 0
    if gn_groups and Cout % gn_groups == 0 and cpg in (4, 8, 16, 32) and (H * W) % 128 == 0:
        nchunk = (H * W) // 128
        part = torch.empty(B * nchunk * gn_groups * 2, dtype=torch.float64, device=out.device)
    e0 = _prof_begin()
    check(lib().muse_conv2d_nhwc_split(x.data_ptr(), w_hi.data_ptr(), w_lo.data_ptr(), ptr(bias), ptr(residual), out.data_ptr(),
                                       ptr(part), gn_groups if part is not None else 0, B, H, W, Cin, Cout, KS,
                                       int(upsample), stream()), "muse_conv2d_nhwc_split")
    _prof_end(e0, "conv_bf16x3", 2.0 * B * H * W * Cout * KS * KS * Cin)
    if part is not None:
        out._gn_stats = (part, nchunk)
    return out


def conv2d_nhwc_split2(x_hi, x_lo, w_hi, w_lo, B, H, W, Cin, Cout, bias=None, residual=None, gn_groups=0):
    """3x3 bf16x3 convolution on pre-split activation planes, operands by LDS-DMA (see muse_conv2d_nhwc_split2).
    gn_groups > 0: the epilogue also produces the GroupNorm statistics of the output; they ride on the returned tensor as
    `out._gn_stats = (partial, nchunk)` for groupnorm_silu_nhwc_split."""
    require_gpu(x_hi, x_lo, w_hi, w_lo)
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x_hi.device)
    part, nchunk = None, 0
    if gn_groups and conv_gn_stats_ok(H, W, Cout, gn_groups):
        nchunk = (H * W) // 256
        part = torch.empty(B * nchunk * gn_groups * 2, dtype=torch.float64, device=out.device)
    e0 = _prof_begin()
    check(lib().muse_conv2d_nhwc_split2(x_hi.data_ptr(), x_lo.data_ptr(), w_hi.data_ptr(), w_lo.data_ptr(), ptr(bias),
                                        ptr(residual), out.data_ptr(), ptr(part), gn_groups if part is not None else 0,
                                        B, H, W, Cin, Cout, 3, stream()), "muse_conv2d_nhwc_split2")
    _prof_end(e0, "conv_bf16x3_dma", 2.0 * B * H * W * Cout * 9 * Cin)
    if e0 is not None:
        PROF_BYTES["conv_bf16x3_dma"] = PROF_BYTES.get("conv_bf16x3_dma", 0.0) + _nbytes(x_hi, x_lo, w_hi, w_lo, residual, out)
    if part is not None:
        out._gn_stats = (part, nchunk)
    return out


def conv_in_direct_ok(Cin, Cout, KS, Cpad, W=256):
    """shapes muse_conv_in_direct takes: the image-to-features 3x3 convolution of an encoder (image rows of up to 1022 pixels: three
    of them are staged in LDS)"""
    return (KS == 3 and Cin <= 4 and Cpad % 4 == 0 and Cpad >= 4 and Cout % 4 == 0 and Cout // 4 <= 256 and 256 % (Cout // 4) == 0
            and W <= 1022)


def conv_in_direct(x, w4, B, H, W, Cin, Cpad, Cout, bias=None, gn_groups=0):
    """conv_in as a direct exact-f32 convolution (muse_conv_in_direct): x [B, H, W, Cpad] f32, w4 [Cout, 9, 4] f32.
    gn_groups * 4 == Cout: the GroupNorm statistics of the output ride on it (`out._gn_stats = (partial, H)`)."""
    require_gpu(x, w4)
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    part = None
    if gn_groups and gn_groups * 4 == Cout:
        part = torch.empty(B * H * gn_groups * 2, dtype=torch.float64, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_conv_in_direct(x.data_ptr(), w4.data_ptr(), ptr(bias), out.data_ptr(), ptr(part), gn_groups if part is not None else 0,
                                    B, H, W, Cin, Cpad, Cout, stream()), "muse_conv_in_direct")
    _prof_end(e0, "conv_in_direct", _nbytes(x, out), "byte")
    if part is not None:
        out._gn_stats = (part, H)
    return out


def conv_in_direct_nchw(x, w4, B, H, W, Cin, Cout, bias=None, gn_groups=0):
    """conv_in_direct reading the image as it arrives (muse_conv_in_direct_nchw): x [B, Cin, H, W] f32 contiguous; no padded NHWC copy.
    Same bits as nchw_to_nhwc + conv_in_direct."""
    require_gpu(x, w4)
    if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != (B, Cin, H, W):
        raise ValueError("conv_in_direct_nchw: x must be a contiguous f32 [B, Cin, H, W] tensor")
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    part = None
    if gn_groups and gn_groups * 4 == Cout:
        part = torch.empty(B * H * gn_groups * 2, dtype=torch.float64, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_conv_in_direct_nchw(x.data_ptr(), w4.data_ptr(), ptr(bias), out.data_ptr(), ptr(part), gn_groups if part is not None else 0,
                                         B, H, W, Cin, Cout, stream()), "muse_conv_in_direct_nchw")
    _prof_end(e0, "conv_in_direct", _nbytes(x, out), "byte")
    if part is not None:
        out._gn_stats = (part, H)
    return out


def conv_out_direct_ok(H, W, Cin, Cout, KS):
    """shapes muse_conv_out_direct takes: the features-to-image 3x3 convolution of a decoder"""
    return KS == 3 and Cout <= 4 and Cin % 32 == 0 and Cin >= 32 and H % 16 == 0 and W % 16 == 0


def conv_out_direct(x, scale, shift, w, bias, B, H, W, Cin, Cout):
    """norm_out -> swish -> conv_out as one direct exact-f32 convolution (muse_conv_out_direct): x [B, H, W, Cin] f32, scale / shift
    [B, Cin] (groupnorm_scale_shift), w [Cout, 9, Cin] f32 -> [B, H, W, Cout] f32"""
    require_gpu(x, scale, shift, w)
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_conv_out_direct(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), w.data_ptr(), ptr(bias), out.data_ptr(),
                                     B, H, W, Cin, Cout, stream()), "muse_conv_out_direct")
    _prof_end(e0, "conv_out_direct", _nbytes(x, out), "byte")
    return out


def upsample2x(x, B, H, W, C):
    """nearest x2 of an NHWC tensor [B, H, W, C] (f32 / bf16) -> [B, 2H, 2W, C] (muse_upsample2x_nhwc)"""
    require_gpu(x)
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=x.dtype, device=x.device)
    check(lib().muse_upsample2x_nhwc(x.data_ptr(), y.data_ptr(), dt(x), B, H, W, C, stream()), "muse_upsample2x_nhwc")
    return y


def upsample2x_split(x, B, H, W, C):
    """nearest x2 of x [B, H, W, C] f32 as the (hi, lo) bf16 operand planes [B, 2H, 2W, C] of conv2d_nhwc_split2"""
    require_gpu(x)
    hi = torch.empty((B, 2 * H, 2 * W, C), dtype=torch.bfloat16, device=x.device)
    lo = torch.empty_like(hi)
    e0 = _prof_begin()
    check(lib().muse_upsample2x_split_nhwc(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), B, H, W, C, stream()), "muse_upsample2x_split_nhwc")
    _prof_end(e0, "upsample2x_split", _nbytes(x, hi, lo), "byte")
    return hi, lo


# the fused GroupNorm convolution may take its persistent kernel (one workgroup per CU walks the tiles: 6-8 % faster when the convolution
# has the chip to itself - a tokenizer or decoder pass on its own).  Default MUSE_CONV_PERSIST, else on; conv_persistent scopes it.
_CONV_PERSISTENT = [os.environ.get("MUSE_CONV_PERSIST", "1") != "0"]


class conv_persistent:
    """with ops.conv_persistent(False): ... - the fused convolutions launched inside run on the launch-per-tile kernel: what a tokenizer
    pass enqueued BESIDE a train step wants (muse.TrainStep); restored on exit"""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _CONV_PERSISTENT[0]
        _CONV_PERSISTENT[0] = self.on
        return self

    def __exit__(self, *exc):
        _CONV_PERSISTENT[0] = self.prev
        return False


def conv_gn_split2_ok(B, H, W, Cin, Cout, KS):
    """shapes muse_conv2d_nhwc_gn_split2 takes (GroupNorm + SiLU + split fused into the patch-slab convolution)"""
    return bool(lib().muse_conv2d_nhwc_gn_split2_ok(B, H, W, Cin, Cout, KS))


def groupnorm_scale_shift(stats, gamma, beta, B, HW, C, groups=32, eps=1e-6):
    """(scale, shift) [B, C] f32 with GroupNorm(x)[b, :, c] = x * scale[b, c] + shift[b, c], from a producer's partial sums
    `stats` = (partial, nchunk)"""
    part, nchunk = stats
    require_gpu(part, gamma, beta)
    sc = torch.empty((B, C), dtype=torch.float32, device=part.device)
    sh = torch.empty((B, C), dtype=torch.float32, device=part.device)
    check(lib().muse_groupnorm_scale_shift(part.data_ptr(), nchunk, gamma.data_ptr(), beta.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                           B, HW, C, groups, eps, stream()), "muse_groupnorm_scale_shift")
    return sc, sh


def conv2d_nhwc_gn_split2(x, scale, shift, w_hi, w_lo, B, H, W, Cin, Cout, bias=None, residual=None, gn_groups=0):
    """conv3x3(silu(GroupNorm(x))) in one kernel: x f32 NHWC, scale / shift from groupnorm_scale_shift (see
    muse_conv2d_nhwc_gn_split2); otherwise as conv2d_nhwc_split2"""
    require_gpu(x, scale, shift, w_hi, w_lo)
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    part, nchunk = None, 0
    if gn_groups and conv_gn_stats_ok(H, W, Cout, gn_groups):
        nchunk = (H * W) // 256
        part = torch.empty(B * nchunk * gn_groups * 2, dtype=torch.float64, device=out.device)
    e0 = _prof_begin()
    check(lib().muse_conv2d_nhwc_gn_split2(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), w_hi.data_ptr(), w_lo.data_ptr(), ptr(bias),
                                           ptr(residual), out.data_ptr(), ptr(part), gn_groups if part is not None else 0,
                                           B, H, W, Cin, Cout, 3, int(_CONV_PERSISTENT[0]), stream()), "muse_conv2d_nhwc_gn_split2")
    _prof_end(e0, "conv_bf16x3_dma", 2.0 * B * H * W * Cout * 9 * Cin)
    if e0 is not None:
        PROF_BYTES["conv_bf16x3_dma"] = PROF_BYTES.get("conv_bf16x3_dma", 0.0) + _nbytes(x, w_hi, w_lo, residual, out)
    if part is not None:
        out._gn_stats = (part, nchunk)
    return out


def conv_gn_split2_pool_ok(B, H, W, Cin, Cout, KS, gn_groups=0):
    """layers muse_conv2d_nhwc_gn_split2_pool takes: the shapes of conv2d_nhwc_gn_split2 (H, W multiples of 16: every 2 x 2 window lies
    inside one convolution tile) and, when the pooled tensor's GroupNorm statistics are wanted, the epilogue's channel condition"""
    return conv_gn_split2_ok(B, H, W, Cin, Cout, KS) and (not gn_groups or conv_gn_stats_ok(H, W, Cout, gn_groups))


def conv2d_nhwc_gn_split2_pool(x, scale, shift, w_hi, w_lo, B, H, W, Cin, Cout, bias=None, residual=None, gn_groups=0):
    """avg_pool2d(conv3x3(silu(GroupNorm(x))) + residual, 2, 2) in one kernel (muse_conv2d_nhwc_gn_split2_pool): the 2 x 2 average is taken
    in the convolution's epilogue -> [B, H/2, W/2, Cout] f32, the bits of conv2d_nhwc_gn_split2 + avgpool2x2_nhwc.  gn_groups > 0: the
    GroupNorm statistics of the POOLED tensor ride on it (`out._gn_stats = (partial, H * W / 256)`: one chunk per convolution tile)."""
    require_gpu(x, scale, shift, w_hi, w_lo)
    out = torch.empty((B, H // 2, W // 2, Cout), dtype=torch.float32, device=x.device)
    part, nchunk = None, 0
    if gn_groups and conv_gn_stats_ok(H, W, Cout, gn_groups):
        nchunk = (H * W) // 256
        part = torch.empty(B * nchunk * gn_groups * 2, dtype=torch.float64, device=out.device)
    e0 = _prof_begin()
    check(lib().muse_conv2d_nhwc_gn_split2_pool(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), w_hi.data_ptr(), w_lo.data_ptr(), ptr(bias),
                                                ptr(residual), out.data_ptr(), ptr(part), gn_groups if part is not None else 0,
                                                B, H, W, Cin, Cout, 3, int(_CONV_PERSISTENT[0]), stream()), "muse_conv2d_nhwc_gn_split2_pool")
    _prof_end(e0, "conv_bf16x3_dma", 2.0 * B * H * W * Cout * 9 * Cin)
    if e0 is not None:
        PROF_BYTES["conv_bf16x3_dma"] = PROF_BYTES.get("conv_bf16x3_dma", 0.0) + _nbytes(x, w_hi, w_lo, residual, out)
    if part is not None:
        out._gn_stats = (part, nchunk)
    return out


def conv_split2_ok(B, H, W, Cin, Cout, KS):
    """shapes muse_conv2d_nhwc_split2 takes (the rest stay on muse_conv2d_nhwc_split)"""
    M = B * H * W
    return (KS == 3 and Cin % 32 == 0 and Cout % 4 == 0 and M * Cin * 2 < (1 << 32) - 64 and Cout * 9 * Cin * 2 < (1 << 32) - 64
            and M < (1 << 31) - 256)


def conv_slab_ok(H, W, Cin):
    """shapes muse_conv2d_nhwc_split2 runs on its patch-slab kernel (16 x 16 pixel patches, K order chunk / tap / channel) unless
    MUSE_CONV_SLAB=0; the others run on the tap-major kernel"""
    import os
    return H % 16 == 0 and W % 16 == 0 and Cin % 64 == 0 and os.environ.get("MUSE_CONV_SLAB", "1") != "0"


def conv_gn_stats_ok(H, W, Cout, groups):
    cpg = Cout // groups if groups else 0
    return groups in (32, 64) and Cout % groups == 0 and (H * W) % 256 == 0 and 4 <= cpg <= 128 and (cpg & (cpg - 1)) == 0


def groupnorm_silu_nhwc_split(x, gamma, beta, B, HW, C, groups=32, eps=1e-6, silu=True, stats=None):
    """GroupNorm + SiLU of an f32 NHWC tensor, returned as the (hi, lo) bf16 planes of the result.
    stats = (partial, nchunk) from the producing convolution's epilogue skips the statistics pass."""
    require_gpu(x, gamma, beta)
    hi = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    lo = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if stats is not None:
        part, snc = stats
    else:
        nchunk = lib().muse_groupnorm_nchunk(HW)
        part, snc = torch.empty(B * nchunk * groups * 2, dtype=torch.float64, device=x.device), 0
    e0 = _prof_begin()
    check(lib().muse_groupnorm_silu_nhwc_split(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                               part.data_ptr(), snc, B, HW, C, groups, eps, 1 if silu else 0, stream()),
          "muse_groupnorm_silu_nhwc_split")
    _prof_end(e0, "groupnorm_silu", _nbytes(x, hi, lo), "byte")
    return hi, lo


def groupnorm_silu_nhwc(x, gamma, beta, B, HW, C, groups=32, eps=1e-6, silu=True):
    require_gpu(x, gamma, beta)
    y = torch.empty_like(x)
    nchunk = lib().muse_groupnorm_nchunk(HW)
    part = torch.empty(B * nchunk * groups * 2, dtype=torch.float64, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_groupnorm_silu_nhwc(x.data_ptr(), y.data_ptr(), dt(x), gamma.data_ptr(), beta.data_ptr(), part.data_ptr(),
                                         B, HW, C, groups, eps, 1 if silu else 0, stream()), "muse_groupnorm_silu_nhwc")
    _prof_end(e0, "groupnorm_silu", _nbytes(x, y), "byte")
    return y


def avgpool2x2_nhwc(x, B, H, W, C_, gn_groups=0):
    """F.avg_pool2d(2, 2) on NHWC.  gn_groups > 0 (f32): the same pass also leaves the GroupNorm statistics of the pooled
    tensor on it (`y._gn_stats`), so the next level's first norm does not re-read it."""
    require_gpu(x)
    y = torch.empty((B, H // 2, W // 2, C_), dtype=x.dtype, device=x.device)
    e0 = _prof_begin()
    vpp = C_ // 4
    if gn_groups and x.dtype == torch.float32 and C_ % 4 == 0 and C_ % gn_groups == 0 and vpp <= 256 and 256 % vpp == 0:
        nchunk = lib().muse_groupnorm_nchunk((H // 2) * (W // 2))
        part = torch.empty(B * nchunk * gn_groups * 2, dtype=torch.float64, device=x.device)
        check(lib().muse_avgpool2x2_nhwc_stats(x.data_ptr(), y.data_ptr(), part.data_ptr(), gn_groups, B, H, W, C_, stream()),
              "muse_avgpool2x2_nhwc_stats")
        y._gn_stats = (part, nchunk)
    else:
        check(lib().muse_avgpool2x2_nhwc(x.data_ptr(), y.data_ptr(), dt(x), B, H, W, C_, stream()), "muse_avgpool2x2_nhwc")
    _prof_end(e0, "avgpool2x2", _nbytes(x, y), "byte")
    return y


def nchw_to_nhwc(x, out_dtype, cpad):
    require_gpu(x)
    B, C_, H, W = x.shape
    x = x.contiguous()
    out = torch.empty((B, H, W, cpad), dtype=out_dtype, device=x.device)
    check(lib().muse_nchw_to_nhwc(x.data_ptr(), out.data_ptr(), dt(out), B, C_, H * W, cpad, stream()), "muse_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, C_):
    require_gpu(x)
    B, H, W, cpad = x.shape
    out = torch.empty((B, C_, H, W), dtype=torch.float32, device=x.device)
    check(lib().muse_nhwc_to_nchw(x.data_ptr(), dt(x), out.data_ptr(), B, C_, H * W, cpad, stream()), "muse_nhwc_to_nchw")
    return out


def vq_nearest(z_flat, codebook, en=None, return_dist=False):
    """argmin_j |z - e_j|^2 computed as the reference does: addmm(|z|^2 + |e|^2, z, e^T, alpha=-2) then argmin.

    z_flat [N, D] f32, codebook [Kc, D] f32 -> int64 [N] (with return_dist also the f32 distance rows [N, Kc] the argmin ran over:
    the parity tests' near-tie accounting reads them)."""
    require_gpu(z_flat, codebook)
    N, D = z_flat.shape
    Kc = codebook.shape[0]
    zn = torch.empty(N, dtype=torch.float32, device=z_flat.device)
    check(lib().muse_row_sumsq(z_flat.data_ptr(), zn.data_ptr(), N, D, z_flat.stride(0), stream()), "muse_row_sumsq")
    if en is None:
        en = torch.empty(Kc, dtype=torch.float32, device=z_flat.device)
        check(lib().muse_row_sumsq(codebook.data_ptr(), en.data_ptr(), Kc, D, codebook.stride(0), stream()), "muse_row_sumsq")
    dist = torch.empty((N, Kc), dtype=torch.float32, device=z_flat.device)
    gemm(z_flat, codebook, dist, N, Kc, D, la=0, lb=0, lda=z_flat.stride(0), ldb=codebook.stride(0), ldc=Kc, alpha=-2.0,
         bias=en, rowvec=zn)
    idx = torch.empty(N, dtype=torch.int64, device=z_flat.device)
    check(lib().muse_argmin_rows(dist.data_ptr(), idx.data_ptr(), N, Kc, Kc, stream()), "muse_argmin_rows")
    return (idx, dist) if return_dist else idx


def vq_neg_distances_scaled(z_flat, codebook, inv_temp):
    """-(|z|^2 + |e|^2 - 2 z.e) * inv_temp as one GEMM with its row / column vectors pre-scaled: the logits of
    VectorQuantizer.get_soft_code (muse/modeling_maskgit_vqgan.py:327-331) -> f32 [N, Kc]"""
    require_gpu(z_flat, codebook)
    N, D = z_flat.shape
    Kc = codebook.shape[0]
    zn = torch.empty(N, dtype=torch.float32, device=z_flat.device)
    en = torch.empty(Kc, dtype=torch.float32, device=z_flat.device)
    check(lib().muse_row_sumsq(z_flat.data_ptr(), zn.data_ptr(), N, D, z_flat.stride(0), stream()), "muse_row_sumsq")
    check(lib().muse_row_sumsq(codebook.data_ptr(), en.data_ptr(), Kc, D, codebook.stride(0), stream()), "muse_row_sumsq")
    out = torch.empty((N, Kc), dtype=torch.float32, device=z_flat.device)
    gemm(z_flat, codebook, out, N, Kc, D, la=0, lb=0, lda=z_flat.stride(0), ldb=codebook.stride(0), ldc=Kc, alpha=2.0 * inv_temp,
         bias=en.mul_(-inv_temp), rowvec=zn.mul_(-inv_temp))
    return out


def gather_rows(table, idx, out_dtype):
    require_gpu(table, idx)
    rows = idx.numel()
    cols = table.shape[1]
    out = torch.empty((rows, cols), dtype=out_dtype, device=table.device)
    check(lib().muse_gather_rows(table.data_ptr(), idx.data_ptr(), out.data_ptr(), dt(out), rows, cols, stream()), "muse_gather_rows")
    return out


# ---- MaskGiTUViT_v2 : f32 forward ops --------------------------------------------------------
def norm_res_fwd(x, w, eps, mode, residual=None, want_pre=False):
    """v = x (+ residual); y = RMSNorm(v) * w (mode 0) / LayerNorm(v) * w (mode 1); returns (y, v or None)"""
    require_gpu(x)
    rows, cols = x.shape
    y = torch.empty_like(x)
    pre = torch.empty_like(x) if want_pre else None
    check(lib().muse_norm_res_fwd(x.data_ptr(), ptr(residual), ptr(w), y.data_ptr(), ptr(pre), rows, cols, eps, mode, stream()),
          "muse_norm_res_fwd")
    return y, pre


def adaln_fwd(x, ss, batch, out_dtype=torch.float32):
    """AdaLN modulation; out_dtype=torch.bfloat16 writes the result directly as the bf16 GEMM operand (no f32 copy)"""
    require_gpu(x, ss)
    rows, C_ = x.shape
    y = torch.empty((rows, C_), dtype=out_dtype, device=x.device)
    f32 = out_dtype == torch.float32
    check(lib().muse_adaln_fwd_ex(x.data_ptr(), ss.data_ptr(), y.data_ptr() if f32 else None, None if f32 else y.data_ptr(), batch,
                                  rows // batch, C_, stream()), "muse_adaln_fwd_ex")
    return y


def silu_fwd(x):
    require_gpu(x)
    y = torch.empty_like(x)
    check(lib().muse_silu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), stream()), "muse_silu_fwd")
    return y


def dwconv3x3_nhwc(x, w, B, H, W, C_):
    """x [B*H*W, C] (NHWC rows), w [C, 1, 3, 3] contiguous"""
    require_gpu(x, w)
    y = torch.empty_like(x)
    check(lib().muse_dwconv3x3_nhwc(x.data_ptr(), w.data_ptr(), y.data_ptr(), B, H, W, C_, stream()), "muse_dwconv3x3_nhwc")
    return y


def space_to_depth2(x, B, H, W, C_):
    """x [B*H*W, C] f32 (NHWC rows) -> [B*(H/2)*(W/2), 4C], channel order (di, dj, c): the operand of the stride-2 2x2 convolution as
    a product (DownsampleBlock, reference modeling_transformer_v2.py:510-514); also the backward of depth_to_space2"""
    require_gpu(x)
    y = torch.empty((B * (H // 2) * (W // 2), 4 * C_), dtype=torch.float32, device=x.device)
    check(lib().muse_space_to_depth2_nhwc(x.data_ptr(), y.data_ptr(), B, H, W, C_, 0, stream()), "muse_space_to_depth2_nhwc")
    return y


def depth_to_space2(x, B, H, W, C_):
    """x [B*(H/2)*(W/2), 4C] f32, channel order (di, dj, c) -> [B*H*W, C]: the stride-2 2x2 transposed convolution's output placement
    (UpsampleBlock, reference :558-562); H, W are the full-resolution sides"""
    require_gpu(x)
    y = torch.empty((B * H * W, C_), dtype=torch.float32, device=x.device)
    check(lib().muse_space_to_depth2_nhwc(x.data_ptr(), y.data_ptr(), B, H, W, C_, 1, stream()), "muse_space_to_depth2_nhwc")
    return y


def grn_fwd(x, gamma, beta, B, S, want_stats=False, out_dtype=torch.float32, drop=None):
    """GlobalResponseNorm over the S pixels of each image; x [B*S, C] f32.  out_dtype=torch.bfloat16: the result is written
    only as the bf16 GEMM operand of the bf16 compute mode (no f32 copy, no cast pass).
    drop = (p, seed, offset): nn.Dropout on the result inside the apply kernel (the keep bits of ops.dropout on the [B*S, C] result); a
    width the dropped kernel refuses (C % 4 != 0) gets the plain kernels and an ops.dropout pass over the f32 result"""
    require_gpu(x, gamma, beta)
    C_ = x.shape[1]
    bf = out_dtype == torch.bfloat16 and C_ % 4 == 0
    y = torch.empty(x.shape, dtype=torch.bfloat16 if bf else torch.float32, device=x.device)
    stats = torch.empty(2 * B * C_, dtype=torch.float32, device=x.device)   # [G | N], kept for grn_bwd
    if drop is not None and grn_drop_ok(B, S, C_):
        check(lib().muse_grn_drop_fwd_ex(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None if bf else y.data_ptr(), y.data_ptr() if bf else None,
                                         stats.data_ptr(), B, S, C_, *_row_drop(drop), stream()), "muse_grn_drop_fwd_ex")
        return (y, stats) if want_stats else y
    check(lib().muse_grn_fwd_ex(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None if bf else y.data_ptr(), y.data_ptr() if bf else None,
                                stats.data_ptr(), B, S, C_, stream()), "muse_grn_fwd_ex")
    if drop is not None:
        dropout(y, *_row_drop(drop), out=y)
    return (y, stats) if want_stats else y


def sinusoidal_encode(features, dim, max_positions=10000.0):
    require_gpu(features)
    f = features.reshape(-1).float().contiguous()
    out = torch.empty((f.numel(), dim), dtype=torch.float32, device=f.device)
    check(lib().muse_sinusoidal_encode(f.data_ptr(), out.data_ptr(), f.numel(), dim, max_positions, stream()), "muse_sinusoidal_encode")
    return out


def weighted_mean(v, w):
    require_gpu(v, w)
    out = torch.empty(1, dtype=torch.float32, device=v.device)
    check(lib().muse_weighted_mean(v.data_ptr(), w.data_ptr(), out.data_ptr(), v.numel(), stream()), "muse_weighted_mean")
    return out


def colsum(part, out, accumulate=False):
    """out[c] (+)= sum_r part[r, c]  (fixed order)"""
    require_gpu(part, out)
    rows, cols = part.shape
    check(lib().muse_colsum(part.data_ptr(), out.data_ptr(), rows, cols, 1 if accumulate else 0, stream()), "muse_colsum")
    return out


def add_rowvec_(x, b):
    """x[r, :] += b, f32 in place (LayerNorm bias of a use_bias model)"""
    require_gpu(x, b)
    if x.dtype != torch.float32 or b.dtype != torch.float32 or not x.is_contiguous():
        raise _hip.MuseHipError("add_rowvec_: contiguous f32 rows and an f32 vector")
    check(lib().muse_add_rowvec(x.data_ptr(), b.data_ptr(), x.numel() // x.shape[-1], x.shape[-1], stream()), "muse_add_rowvec")
    return _touched(x)


def bias_grad(dy, cols=None):
    """d(bias)[c] = sum_r dy[r, c] for the first `cols` columns of dy [rows, >= cols] (f32 or bf16, any row stride): two fixed-order
    stages (per-chunk partial rows, then muse_colsum)"""
    require_gpu(dy)
    rows = dy.shape[0]
    cols = dy.shape[1] if cols is None else cols
    if dy.stride(1) != 1:
        raise _hip.MuseHipError("bias_grad: unit column stride")
    R = lib().muse_bias_grad_rows_per_block()
    part = torch.empty(((rows + R - 1) // R, cols), dtype=torch.float32, device=dy.device)
    check(lib().muse_bias_grad_partial(dy.data_ptr(), dt(dy), part.data_ptr(), rows, cols, dy.stride(0), stream()), "muse_bias_grad_partial")
    return colsum(part, torch.empty(cols, dtype=torch.float32, device=dy.device))


def norm_res_bwd(dy, v, w, eps, mode, dpre=None, want_dw=True, also_bf16=False):
    """backward of norm_res_fwd: returns (dv = dx = dres, dw or None[, bf16 copy of dv]).  v = the forward's pre-norm sum."""
    require_gpu(dy, v)
    rows, cols = v.shape
    dv = torch.empty_like(v)
    dvb = torch.empty(v.shape, dtype=torch.bfloat16, device=v.device) if also_bf16 else None
    nblk = lib().muse_norm_res_bwd_nblk(rows)
    part = torch.empty((nblk, cols), dtype=torch.float32, device=v.device)
    check(lib().muse_norm_res_bwd_ex(dy.data_ptr(), ptr(dpre), v.data_ptr(), ptr(w), dv.data_ptr(), ptr(dvb), part.data_ptr(), rows,
                                     cols, eps, mode, stream()), "muse_norm_res_bwd_ex")
    dw = colsum(part, torch.empty(cols, dtype=torch.float32, device=v.device)) if want_dw else None
    return (dv, dw, dvb) if also_bf16 else (dv, dw)


def norm_adaln_ok(rows, cols, batch):
    """shapes the fused norm + AdaLN kernels take (muse_norm_adaln_fwd / _bwd)"""
    return cols % 4 == 0 and cols <= 1024 and rows % batch == 0 and (rows // batch) % 16 == 0


def norm_adaln_fwd(x, w, ss, batch, eps, mode, residual=None, out_dtype=torch.float32, planes_only=False):
    """v = x (+ residual); m = Norm(v) * w * (1 + scale) + shift with (scale | shift) = ss [batch, 2C]  ->  (m in out_dtype, v).
    planes_only (planes_only_ok): m comes back as OperandOnly - the running pass's operand image without the f32 tensor"""
    require_gpu(x, ss)
    rows, cols = x.shape
    pre = torch.empty_like(x)
    if planes_only:
        if not (planes_only_ok(rows, cols) and x.dtype == torch.float32 and x.is_contiguous()):
            raise _hip.MuseHipError("norm_adaln_fwd(planes_only=True) outside planes_only_ok")
        planes = planes_alloc((rows, cols), x.device)
        check(lib().muse_norm_adaln_fwd_x3(x.data_ptr(), ptr(residual), ptr(w), ss.data_ptr(), pre.data_ptr(), None, planes.data_ptr(),
                                           batch, rows // batch, cols, eps, mode, *_image_args(False, planes), stream()), "muse_norm_adaln_fwd_x3")
        return operand_only(planes, False), pre
    m = torch.empty((rows, cols), dtype=out_dtype, device=x.device)
    f32 = out_dtype == torch.float32
    im = _x3_producing(x) if f32 else None
    if im is not None and cols % 8 == 0:        # "bf16x3" mode: m feeds weight GEMMs - its operand planes come out of this kernel
        planes = planes_alloc((rows, cols), x.device)
        check(lib().muse_norm_adaln_fwd_x3(x.data_ptr(), ptr(residual), ptr(w), ss.data_ptr(), pre.data_ptr(), m.data_ptr(), planes.data_ptr(),
                                           batch, rows // batch, cols, eps, mode, *_image_args(False, planes), stream()), "muse_norm_adaln_fwd_x3")
        im.put_planes(m, planes)
        return m, pre
    check(lib().muse_norm_adaln_fwd(x.data_ptr(), ptr(residual), ptr(w), ss.data_ptr(), pre.data_ptr(), m.data_ptr() if f32 else None,
                                    None if f32 else m.data_ptr(), batch, rows // batch, cols, eps, mode, stream()), "muse_norm_adaln_fwd")
    return m, pre


def norm_adaln_bwd(dm, v, w, ss, batch, eps, mode, dpre=None, also_bf16=False, dss_out=None):
    """backward of norm_adaln_fwd -> (dv = dx = dres, dw, dss [batch, 2C][, bf16 copy of dv])"""
    require_gpu(dm, v, ss)
    rows, cols = v.shape
    dv = torch.empty_like(v)
    dvb = torch.empty(v.shape, dtype=torch.bfloat16, device=v.device) if also_bf16 else None
    nblk = lib().muse_norm_res_bwd_nblk(rows)
    part = torch.empty((nblk, cols), dtype=torch.float32, device=v.device)
    spart = torch.empty((nblk, 2 * cols), dtype=torch.float32, device=v.device)
    im = _x3_producing(v) if not also_bf16 else None
    if im is not None and cols % 8 == 0:        # "bf16x3" mode: dv is the dY of the weight GEMMs below - planes from this kernel
        planes = planes_alloc((rows, cols), v.device)
        check(lib().muse_norm_adaln_bwd_x3(dm.data_ptr(), ptr(dpre), v.data_ptr(), ptr(w), ss.data_ptr(), dv.data_ptr(), planes.data_ptr(),
                                           part.data_ptr(), spart.data_ptr(), batch, rows // batch, cols, eps, mode, *_image_args(True, planes),
                                           stream()), "muse_norm_adaln_bwd_x3")
        im.put_planes(dv, planes)
    else:
        check(lib().muse_norm_adaln_bwd(dm.data_ptr(), ptr(dpre), v.data_ptr(), ptr(w), ss.data_ptr(), dv.data_ptr(), ptr(dvb), part.data_ptr(),
                                        spart.data_ptr(), batch, rows // batch, cols, eps, mode, stream()), "muse_norm_adaln_bwd")
    dw = colsum(part, torch.empty(cols, dtype=torch.float32, device=v.device))
    dss = dss_out if dss_out is not None else torch.empty((batch, 2 * cols), dtype=torch.float32, device=v.device)
    check(lib().muse_colsum_segments(spart.data_ptr(), dss.data_ptr(), batch, nblk // batch, 2 * cols, stream()), "muse_colsum_segments")
    return (dv, dw, dss, dvb) if also_bf16 else (dv, dw, dss)


def adaln_bwd(dy, x, ss, batch, dss_out=None):
    """-> (dx, dss [batch, 2C]); dss_out: a contiguous [batch, 2C] f32 buffer to write dss into"""
    require_gpu(dy, x, ss)
    rows, C_ = x.shape
    dx = torch.empty_like(x)
    dss = dss_out if dss_out is not None else torch.empty(ss.shape, dtype=torch.float32, device=ss.device)
    check(lib().muse_adaln_bwd(dy.data_ptr(), x.data_ptr(), ss.data_ptr(), dx.data_ptr(), dss.data_ptr(), batch, rows // batch, C_,
                               stream()), "muse_adaln_bwd")
    return dx, dss


def silu_bwd(x, dy):
    require_gpu(x, dy)
    dx = torch.empty_like(x)
    check(lib().muse_silu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), stream()), "muse_silu_bwd")
    return dx


def dwconv3x3_bwd(dy, x, w, B, H, W, C_):
    """-> (dx, dw [C, 1, 3, 3])"""
    require_gpu(dy, x, w)
    dx = torch.empty_like(x)
    nchunk = lib().muse_dwconv3x3_bwd_nchunk(B * H * W)
    part = torch.empty((nchunk, C_ * 9), dtype=torch.float32, device=x.device)
    check(lib().muse_dwconv3x3_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr(), part.data_ptr(), B, H, W, C_, stream()),
          "muse_dwconv3x3_bwd")
    dw = colsum(part, torch.empty(C_ * 9, dtype=torch.float32, device=x.device)).view(C_, 1, 3, 3)
    return dx, dw


def grn_bwd(dy, x, gamma, stats, B, S, drop=None):
    """-> (dx, dgamma [C], dbeta [C]).  drop = grn_fwd's: the same keep mask, redrawn, multiplies dy before everything else"""
    require_gpu(dy, x, gamma, stats)
    C_ = x.shape[1]
    dx = torch.empty_like(x)
    work = torch.empty(4 * B * C_, dtype=torch.float32, device=x.device)
    if drop is not None and grn_drop_ok(B, S, C_):
        if dy.dtype != torch.float32 or not dy.is_contiguous():
            raise _hip.MuseHipError("grn_bwd(drop=) expects a contiguous f32 gradient")
        check(lib().muse_grn_drop_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), stats.data_ptr(), dx.data_ptr(), work.data_ptr(), B, S, C_,
                                      *_row_drop(drop), stream()), "muse_grn_drop_bwd")
        dbeta = colsum(work[: B * C_].view(B, C_), torch.empty(C_, dtype=torch.float32, device=x.device))
        dgamma = colsum(work[B * C_: 2 * B * C_].view(B, C_), torch.empty(C_, dtype=torch.float32, device=x.device))
        return dx, dgamma, dbeta
    if drop is not None:
        dy = dropout(dy.contiguous(), *_row_drop(drop))
    check(lib().muse_grn_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), stats.data_ptr(), dx.data_ptr(), work.data_ptr(), B, S, C_,
                             stream()), "muse_grn_bwd")
    dbeta = colsum(work[: B * C_].view(B, C_), torch.empty(C_, dtype=torch.float32, device=x.device))
    dgamma = colsum(work[B * C_: 2 * B * C_].view(B, C_), torch.empty(C_, dtype=torch.float32, device=x.device))
    return dx, dgamma, dbeta


def scale_rows_(x, w, num, den, cols):
    """x[r, :cols] *= w[r] * num[0] / den[0]  (in place; num / den are 1-element device tensors)"""
    require_gpu(x, w, num, den)
    check(lib().muse_scale_rows(x.data_ptr(), w.data_ptr(), num.data_ptr(), den.data_ptr(), x.shape[0], cols, x.stride(0), stream()),
          "muse_scale_rows")
    return _touched(x)


def probe_tr16(addr):
    require_gpu(addr)
    out = torch.empty(256, dtype=torch.int32, device=addr.device)
    check(lib().muse_probe_tr16(addr.data_ptr(), out.data_ptr(), stream()), "muse_probe_tr16")
    return out


# ---- CLIP text tower (csrc/clip_text.hip, its fused attention csrc/attention_enc.hip; muse.CLIPTextEncoder): forward only ---------------
def causal_attention_fwd(q, k, v, B, S, nh, hd, alpha, out=None):
    """fused causal softmax(alpha q k^T) v for q / k / v [B*S, H] bf16 views (row strides free: slices of one packed q | k | v
    projection; rows >= S of an image are never read) -> ctx [B*S, H] bf16.  No score matrix in memory."""
    require_gpu(q, k, v)
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
        raise _hip.MuseHipError("the fused causal attention kernel takes bf16 operands")
    ctx = out if out is not None else torch.empty((B * S, nh * hd), dtype=torch.bfloat16, device=q.device)
    d = _attn_desc(q, k, v, ctx, B, S, S, nh, hd, alpha)
    e0 = _prof_begin()
    check(lib().muse_causal_attention_fwd(C.byref(d), stream()), "muse_causal_attention_fwd")
    _prof_end(e0, "attn_causal_fwd_bf16", 4.0 * B * nh * S * S * hd)
    return _touched(ctx)


def causal_softmax_(x, mats, seq, ld):
    """in place on [mats, seq, ld] score matrices: row i = softmax over its columns 0..i, every other column of [0, ld) = 0"""
    require_gpu(x)
    e0 = _prof_begin()
    check(lib().muse_causal_softmax_fwd(x.data_ptr(), x.data_ptr(), dt(x), mats, seq, ld, stream()), "muse_causal_softmax_fwd")
    _prof_end(e0, "causal_softmax_fwd", 2.0 * _nbytes(x), "byte")
    return _touched(x)


def bias_quick_gelu_(x, bias):
    """in place on x [rows, cols] (f32 / bf16): v = x + bias[col]; x = v * sigmoid(1.702 v)"""
    require_gpu(x, bias)
    rows, cols = x.shape
    if not x.is_contiguous() or bias.dtype != torch.float32 or bias.numel() != cols:
        raise _hip.MuseHipError("bias_quick_gelu_: x contiguous [rows, cols], bias f32 [cols]")
    check(lib().muse_bias_quick_gelu(x.data_ptr(), bias.data_ptr(), x.data_ptr(), dt(x), rows, cols, stream()), "muse_bias_quick_gelu")
    return _touched(x)


def layernorm_bias_fwd(x, w, b, eps, out_dtype):
    """LayerNorm(x) * w + b in one pass: x f32 [rows, cols] -> f32 or bf16"""
    require_gpu(x, w, b)
    rows, cols = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise _hip.MuseHipError("layernorm_bias_fwd: x is a contiguous f32 [rows, cols] tensor")
    for name, t in (("w", w), ("b", b)):
        if t.dtype != torch.float32 or tuple(t.shape) != (cols,) or not t.is_contiguous():
            raise _hip.MuseHipError(f"layernorm_bias_fwd: {name} is a contiguous f32 [{cols}] tensor, got {t.dtype} {tuple(t.shape)}")
    y = torch.empty((rows, cols), dtype=out_dtype, device=x.device)
    check(lib().muse_layernorm_bias_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), dt(y), rows, cols, eps, stream()),
          "muse_layernorm_bias_fwd")
    return y


def eos_index(ids, eos_token_id):
    """ids int64 [B, S] -> (idx [B], flat [B] = b * S + idx[b]) int64: the pooled position of every row (first eos_token_id; with
    eos_token_id == 2 the first position of the row maximum; 0 when nothing matches) - no host read of the ids"""
    require_gpu(ids)
    if ids.dtype != torch.int64 or ids.dim() != 2 or not ids.is_contiguous():
        raise _hip.MuseHipError("eos_index: ids is a contiguous int64 [batch, seq] tensor")
    B, S = ids.shape
    idx = torch.empty(B, dtype=torch.int64, device=ids.device)
    flat = torch.empty(B, dtype=torch.int64, device=ids.device)
    check(lib().muse_eos_index(ids.data_ptr(), idx.data_ptr(), flat.data_ptr(), B, S, int(eos_token_id), stream()), "muse_eos_index")
    return idx, flat


# ---- T5 text encoder (csrc/t5_text.hip, its fused attention csrc/attention_enc.hip; muse.T5TextEncoder): forward only -------------------
def _rel_check(what, rel, nh, S):
    if rel.dtype != torch.float32 or not rel.is_contiguous() or tuple(rel.shape) != (nh, 2 * S - 1):
        raise _hip.MuseHipError(f"{what}: rel is a contiguous f32 [heads, 2 S - 1] = {(nh, 2 * S - 1)} tensor, got {rel.dtype} {tuple(rel.shape)}")


def bias_attention_fwd(q, k, v, rel, B, S, nh, hd, out=None):
    """fused bidirectional softmax(q k^T + bias) v, bias(query i, key j) = rel[head][j - i + S - 1], no score scale: q / k / v [B*S, H]
    bf16 views (row strides free: slices of one packed q | k | v projection; rows >= S of an image are never read), rel f32
    [heads, 2 S - 1] -> ctx [B*S, H] bf16.  No score matrix in memory."""
    require_gpu(q, k, v, rel)
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
        raise _hip.MuseHipError("the fused bias attention kernel takes bf16 operands")
    _rel_check("bias_attention_fwd", rel, nh, S)
    ctx = out if out is not None else torch.empty((B * S, nh * hd), dtype=torch.bfloat16, device=q.device)
    d = _attn_desc(q, k, v, ctx, B, S, S, nh, hd, 1.0)
    e0 = _prof_begin()
    check(lib().muse_bias_attention_fwd(C.byref(d), rel.data_ptr(), stream()), "muse_bias_attention_fwd")
    _prof_end(e0, "attn_bias_fwd_bf16", 4.0 * B * nh * S * S * hd)
    return _touched(ctx)


def bias_softmax_(x, rel, mats, nh, seq, ld, bf16_copy=False):
    """[mats, seq, ld] f32 score matrices: row i of matrix z = softmax over j < seq of x[i][j] + rel[z % nh][j - i + seq - 1], every
    column of [seq, ld) = 0.  In place -> x; bf16_copy: x is left as it is and the result comes back as a bf16 tensor of the same shape"""
    require_gpu(x, rel)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != mats * seq * ld:
        raise _hip.MuseHipError("bias_softmax_: x is a contiguous f32 [mats, seq, ld] tensor")
    _rel_check("bias_softmax_", rel, nh, seq)
    yb = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if bf16_copy else None
    e0 = _prof_begin()
    check(lib().muse_bias_softmax_fwd(x.data_ptr(), None if bf16_copy else x.data_ptr(), ptr(yb), rel.data_ptr(), mats, nh, seq, ld, stream()),
          "muse_bias_softmax_fwd")
    _prof_end(e0, "bias_softmax_fwd", _nbytes(x) + _nbytes(yb if bf16_copy else x), "byte")
    return yb if bf16_copy else _touched(x)


def gated_gelu_tanh(ab):
    """ab [rows, 2 F] (f32 / bf16, the packed wi_0 | wi_1 product) -> gelu_new(ab[:, :F]) * ab[:, F:] in the same dtype"""
    require_gpu(ab)
    rows, two_f = ab.shape
    if not ab.is_contiguous() or two_f % 2:
        raise _hip.MuseHipError("gated_gelu_tanh: ab is a contiguous [rows, 2 F] tensor")
    y = torch.empty((rows, two_f // 2), dtype=ab.dtype, device=ab.device)
    check(lib().muse_gated_gelu_tanh(ab.data_ptr(), y.data_ptr(), dt(ab), rows, two_f // 2, stream()), "muse_gated_gelu_tanh")
    return y


def rmsnorm_fwd(x, w, eps, out_dtype):
    """x * rsqrt(mean(x^2) + eps) * w (T5LayerNorm: no mean subtraction, no bias): x f32 [rows, cols] -> f32 (muse_norm_res_fwd mode 0,
    cols % 4 == 0) or bf16"""
    require_gpu(x, w)
    rows, cols = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or w.dtype != torch.float32 or w.numel() != cols:
        raise _hip.MuseHipError("rmsnorm_fwd: x is a contiguous f32 [rows, cols] tensor, w f32 [cols]")
    if out_dtype == torch.float32:
        return norm_res_fwd(x, w, eps, 0)[0]
    y = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    check(lib().muse_rmsnorm_bf16_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, cols, eps, stream()), "muse_rmsnorm_bf16_fwd")
    return y


def rel_bias_gather(table, bucket):
    """table f32 [buckets, heads] (relative_attention_bias.weight), bucket int64 [n] -> rel f32 [heads, n], rel[h][t] = table[bucket[t]][h]"""
    require_gpu(table, bucket)
    if table.dtype != torch.float32 or not table.is_contiguous() or table.dim() != 2 or bucket.dtype != torch.int64 or not bucket.is_contiguous():
        raise _hip.MuseHipError("rel_bias_gather: table is a contiguous f32 [buckets, heads] tensor, bucket a contiguous int64 vector")
    nb, nh = table.shape
    rel = torch.empty((nh, bucket.numel()), dtype=torch.float32, device=table.device)
    check(lib().muse_rel_bias_gather(table.data_ptr(), bucket.data_ptr(), rel.data_ptr(), nh, bucket.numel(), nb, stream()), "muse_rel_bias_gather")
    return rel


# ---- Paella VQ tokenizer (csrc/paella.hip) : f32 forward ops on channels-last rows ---------------------------------------------
def _f32_operand(what, t, shape):
    """the kernels read their weights through raw pointers: a transposed, strided or non-f32 operand would be read in the wrong order"""
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise _hip.MuseHipError(f"{what} must be a contiguous f32 tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)} "
                                f"(contiguous: {t.is_contiguous()})")


def paella_mix_fwd(x, w9, bias, gammas, B, H, W):
    """y = x + g2 * (dwconv3x3_replicate(LN(x) * (1 + g0) + g1) + bias): x [B*H*W, C] f32, w9 [9, C] (tap-major), gammas = the block's
    six floats ON THE DEVICE (read by the kernel)"""
    require_gpu(x, w9, bias, gammas)
    rows, C_ = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or rows != B * H * W or gammas.numel() < 3:
        raise _hip.MuseHipError("paella_mix_fwd: x is a contiguous f32 [B*H*W, C] tensor, gammas holds g0, g1, g2")
    _f32_operand("paella_mix_fwd: w9", w9, (9, C_))
    _f32_operand("paella_mix_fwd: bias", bias, (C_,))
    if gammas.dtype != torch.float32 or not gammas.is_contiguous():
        raise _hip.MuseHipError("paella_mix_fwd: gammas is a contiguous f32 tensor")
    y = torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_paella_mix_fwd(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), gammas.data_ptr(), stats.data_ptr(), y.data_ptr(), B, H, W,
                                    C_, stream()), "muse_paella_mix_fwd")
    _prof_end(e0, "paella_mix", _nbytes(x, x, y, stats, stats), "byte")
    return y


def patch_rows(x, B, H, W, C_, KS, stride, pad_top, pad_left, Hout, Wout):
    """zero-padded KS x KS patches of x [B*H*W, C] f32 -> [B*Hout*Wout, KS*KS*C], patch element order (ky, kx, c)"""
    require_gpu(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != B * H * W * C_:
        raise _hip.MuseHipError("patch_rows: x is a contiguous f32 [B*H*W, C] tensor")
    y = torch.empty((B * Hout * Wout, KS * KS * C_), dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_patch_rows_nhwc(x.data_ptr(), y.data_ptr(), B, H, W, C_, KS, stride, pad_top, pad_left, Hout, Wout, stream()),
          "muse_patch_rows_nhwc")
    _prof_end(e0, "patch_rows", _nbytes(x, y), "byte")
    return y


def vq_nearest_small(z_flat, codebook, return_dist=False):
    """argmin_j sum_k (z_k - e_jk)^2 for codebook width D <= 8, distance and argmin in one kernel (no [N, Kc] matrix).
    z_flat [N, D] f32 (row stride free), codebook [Kc, D] f32 -> int64 [N] (with return_dist also the winning squared distances)"""
    require_gpu(z_flat, codebook)
    N, D = z_flat.shape
    if z_flat.dtype != torch.float32 or codebook.dtype != torch.float32 or codebook.shape[1] != D or z_flat.stride(1) != 1:
        raise _hip.MuseHipError("vq_nearest_small: z [N, D] and codebook [Kc, D] are f32 with unit column stride")
    _f32_operand("vq_nearest_small: codebook", codebook, (codebook.shape[0], D))
    idx = torch.empty(N, dtype=torch.int64, device=z_flat.device)
    dist = torch.empty(N, dtype=torch.float32, device=z_flat.device) if return_dist else None
    e0 = _prof_begin()
    check(lib().muse_vq_nearest_small(z_flat.data_ptr(), z_flat.stride(0), codebook.data_ptr(), idx.data_ptr(), ptr(dist), N, D,
                                      codebook.shape[0], stream()), "muse_vq_nearest_small")
    _prof_end(e0, "vq_nearest_small", _nbytes(z_flat, codebook, idx), "byte")
    return (idx, dist) if return_dist else idx


def paella_in_block(pixel_values, w12, bias):
    """PixelUnshuffle(2) + 1x1 convolution 12 -> C of an NCHW f32 image batch [B, 3, H, W] -> rows [B*(H/2)*(W/2), C]; w12 [12, C]"""
    require_gpu(pixel_values, w12, bias)
    B, Ci, H, W = pixel_values.shape
    if Ci != 3 or pixel_values.dtype != torch.float32 or not pixel_values.is_contiguous():
        raise _hip.MuseHipError("paella_in_block: pixel_values is a contiguous f32 [B, 3, H, W] tensor")
    C_ = w12.shape[-1]
    _f32_operand("paella_in_block: w12", w12, (12, C_))
    _f32_operand("paella_in_block: bias", bias, (C_,))
    y = torch.empty((B * (H // 2) * (W // 2), C_), dtype=torch.float32, device=pixel_values.device)
    e0 = _prof_begin()
    check(lib().muse_paella_in_block(pixel_values.data_ptr(), w12.data_ptr(), bias.data_ptr(), y.data_ptr(), B, H, W, C_, stream()),
          "muse_paella_in_block")
    _prof_end(e0, "paella_in_block", _nbytes(pixel_values, y), "byte")
    return y


def paella_out_block(x, w12, bias, B, H, W):
    """1x1 convolution C -> 12 + PixelShuffle(2): rows x [B*(H/2)*(W/2), C] f32 -> NCHW f32 image [B, 3, H, W]; w12 [12, C]"""
    require_gpu(x, w12, bias)
    rows, C_ = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or rows != B * (H // 2) * (W // 2):
        raise _hip.MuseHipError("paella_out_block: x is a contiguous f32 [B*(H/2)*(W/2), C] tensor")
    _f32_operand("paella_out_block: w12", w12, (12, C_))
    _f32_operand("paella_out_block: bias", bias, (12,))
    img = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    e0 = _prof_begin()
    check(lib().muse_paella_out_block(x.data_ptr(), w12.data_ptr(), bias.data_ptr(), img.data_ptr(), B, H, W, C_, stream()),
          "muse_paella_out_block")
    _prof_end(e0, "paella_out_block", _nbytes(x, img), "byte")
    return img


# ---- MoVQ tokenizer (csrc/movq.hip) ----------------------------------------------------------------------------------------------
def spatial_norm(x, zq, gamma, beta, wy, by, wb, bb, B, H, W, C, zh, zw, groups=32, eps=1e-6, silu=True, stats=None, split=False):
    """SpatialNorm (+ SiLU) of an f32 NHWC tensor in one apply pass (muse_spatial_norm_nhwc):
    GroupNorm(x) * conv_y(nearest(zq)) + conv_b(nearest(zq)), x [B, H, W, C], zq [B, zh, zw, Z] (Z <= 8; H % zh == W % zw == 0),
    wy / wb [C, Z] and by / bb [C] the two 1x1 convolutions.  -> y f32 like x, or with split=True the (hi, lo) bf16 operand planes of
    conv2d_nhwc_split2.  stats = (partial, nchunk) from the producing kernel's epilogue skips the statistics pass."""
    require_gpu(x, zq, gamma, beta, wy, by, wb, bb)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != B * H * W * C:
        raise _hip.MuseHipError(f"spatial_norm: x is a contiguous f32 [B, H, W, C] tensor, got {x.dtype} {tuple(x.shape)}")
    if zq.dim() != 4:
        raise _hip.MuseHipError("spatial_norm: zq is a contiguous f32 [B, zh, zw, Z] tensor")
    Z = zq.shape[-1]
    _f32_operand("spatial_norm: zq", zq, (B, zh, zw, Z))
    for what, t, shape in (("gamma", gamma, (C,)), ("beta", beta, (C,)), ("wy", wy, (C, Z)), ("by", by, (C,)), ("wb", wb, (C, Z)),
                           ("bb", bb, (C,))):
        _f32_operand("spatial_norm: " + what, t, shape)
    if stats is not None:
        part, snc = stats
        require_gpu(part)
        if part.dtype != torch.float64 or not part.is_contiguous() or snc <= 0 or part.numel() != B * snc * groups * 2:
            raise _hip.MuseHipError("spatial_norm: stats = (partial f64 [B, nchunk, groups, 2], nchunk)")
    else:
        part, snc = torch.empty(B * lib().muse_groupnorm_nchunk(H * W) * groups * 2, dtype=torch.float64, device=x.device), 0
    if split:
        out = (torch.empty(x.shape, dtype=torch.bfloat16, device=x.device), torch.empty(x.shape, dtype=torch.bfloat16, device=x.device))
        y_ptr, hi_ptr, lo_ptr = None, out[0].data_ptr(), out[1].data_ptr()
    else:
        out = torch.empty_like(x)
        y_ptr, hi_ptr, lo_ptr = out.data_ptr(), None, None
    e0 = _prof_begin()
    check(lib().muse_spatial_norm_nhwc(x.data_ptr(), y_ptr, hi_ptr, lo_ptr, gamma.data_ptr(), beta.data_ptr(), zq.data_ptr(), wy.data_ptr(),
                                       by.data_ptr(), wb.data_ptr(), bb.data_ptr(), part.data_ptr(), snc, B, H, W, C, zh, zw, Z, groups, eps,
                                       1 if silu else 0, stream()), "muse_spatial_norm_nhwc")
    _prof_end(e0, "spatial_norm", _nbytes(x, zq, gamma, beta, wy, by, wb, bb, *(out if split else (out,))), "byte")
    return out


# ---- pre-encode image stage (csrc/resize.hip) ------------------------------------------------------------------------------------
def resize_crop_u8(packed, table, B, R, out=None, host_table=None):
    """Antialiased bilinear resize + crop (+ flip) of B packed uint8 HWC images into [B, 3, R, R] f32 NCHW in one launch
    (muse_resize_crop_u8; the value is spelled out in include/muse_hip.h).  packed: uint8 device bytes; table: int64 device [B, 8] =
    (offset, H, W, oh, ow, top, left, flip) per image.  The kernel trusts the table, so every row is checked here on the host:
    against `host_table` (the CPU tensor the device table was copied from) when the caller still has it, else against a read-back."""
    require_gpu(packed, table, out)
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise _hip.MuseHipError(f"resize_crop_u8: packed is a contiguous 1-D uint8 tensor, got {packed.dtype} {tuple(packed.shape)}")
    if table.dtype != torch.int64 or tuple(table.shape) != (B, 8) or not table.is_contiguous():
        raise _hip.MuseHipError(f"resize_crop_u8: table is a contiguous int64 [B, 8] tensor, got {table.dtype} {tuple(table.shape)}")
    if B < 1 or R < 1:
        raise _hip.MuseHipError(f"resize_crop_u8: B and R are at least 1, got B {B}, R {R}")
    rows = (table if host_table is None else host_table).cpu()
    if rows.dtype != torch.int64 or tuple(rows.shape) != (B, 8):
        raise _hip.MuseHipError("resize_crop_u8: host_table is the int64 [B, 8] CPU copy of table")
    for b, (off, H, W, oh, ow, top, left, flip) in enumerate(rows.tolist()):
        if H < 1 or W < 1 or off < 0 or off + 3 * H * W > packed.numel():
            raise _hip.MuseHipError(f"resize_crop_u8: image {b} ({H} x {W} at byte {off}) does not lie inside packed ({packed.numel()} bytes)")
        if oh < R or ow < R or not (0 <= top <= oh - R) or not (0 <= left <= ow - R) or flip not in (0, 1):
            raise _hip.MuseHipError(f"resize_crop_u8: image {b}: window ({top}, {left}) + {R} outside the resized image {oh} x {ow}, or "
                                    f"flip {flip} not 0 / 1")
        if max(H, W, oh, ow) >= 1 << 24 or 3 * H * W >= 1 << 31:
            raise _hip.MuseHipError(f"resize_crop_u8: image {b}: sides are below 2^24 (exact in f32) and an image below 2 GiB")
    if out is None:
        out = torch.empty((B, 3, R, R), dtype=torch.float32, device=packed.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, R, R) or not out.is_contiguous():
        raise _hip.MuseHipError(f"resize_crop_u8: out is a contiguous f32 [B, 3, R, R] tensor, got {out.dtype} {tuple(out.shape)}")
    e0 = _prof_begin()
    check(lib().muse_resize_crop_u8(packed.data_ptr(), table.data_ptr(), out.data_ptr(), B, R, stream()), "muse_resize_crop_u8")
    _prof_end(e0, "resize_crop_u8", _nbytes(packed, out), "byte")
    return out


# ---- CLIP image tower (csrc/clip_vision.hip; muse.CLIPImageEncoder / muse.CLIPScorer): forward only -----------------------------------
def resize_bicubic_norm(images, size, mean, std, out=None):
    """images f32 [B, 3, R, R] -> f32 [B, 3, size, size] = (F.interpolate(images, (size, size), mode="bicubic", antialias=True) -
    mean[c]) / std[c] in one launch, nothing clamped (muse_resize_bicubic_norm_f32; the value is spelled out in include/muse_hip.h).
    mean / std: three Python floats each."""
    require_gpu(images, out)
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3] or not images.is_contiguous():
        raise _hip.MuseHipError(f"resize_bicubic_norm: images is a contiguous f32 [B, 3, R, R] tensor, got {images.dtype} {tuple(images.shape)}")
    B, R, size = int(images.shape[0]), int(images.shape[2]), int(size)
    if B < 1 or R < 1 or size < 1 or len(mean) != 3 or len(std) != 3:
        raise _hip.MuseHipError(f"resize_bicubic_norm: B, R and size are at least 1 and mean / std hold three floats, got B {B}, R {R}, size {size}")
    if out is None:
        out = torch.empty((B, 3, size, size), dtype=torch.float32, device=images.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, size, size) or not out.is_contiguous():
        raise _hip.MuseHipError(f"resize_bicubic_norm: out is a contiguous f32 [B, 3, size, size] tensor, got {out.dtype} {tuple(out.shape)}")
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    e0 = _prof_begin()
    check(lib().muse_resize_bicubic_norm_f32(images.data_ptr(), out.data_ptr(), B, R, size, m3, s3, stream()), "muse_resize_bicubic_norm_f32")
    _prof_end(e0, "resize_bicubic_norm", _nbytes(images, out), "byte")
    return _touched(out)


def clip_patch_rows(pixel_values, patch, out_dtype=torch.float32, out=None):
    """pixel_values f32 [B, 3, I, I] -> [B * G * G, Kp] (f32 or bf16), G = I / patch, Kp = 3 patch^2 rounded up to a multiple of 8:
    row (b, gy, gx), column (c, ky, kx) - the flattening of Conv2d(3, H, patch, stride=patch).weight; columns >= 3 patch^2 are zeros"""
    require_gpu(pixel_values, out)
    if (pixel_values.dtype != torch.float32 or pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or pixel_values.shape[2] != pixel_values.shape[3]
            or not pixel_values.is_contiguous()):
        raise _hip.MuseHipError(f"clip_patch_rows: pixel_values is a contiguous f32 [B, 3, I, I] tensor, got {pixel_values.dtype} {tuple(pixel_values.shape)}")
    B, I, P = int(pixel_values.shape[0]), int(pixel_values.shape[2]), int(patch)
    if B < 1 or P < 1 or I % P:
        raise _hip.MuseHipError(f"clip_patch_rows: the image side {I} is a multiple of the patch side {P}, and the batch is not empty")
    G, Kp = I // P, (3 * P * P + 7) & ~7
    if out is None:
        out = torch.empty((B * G * G, Kp), dtype=out_dtype, device=pixel_values.device)
    elif out.dtype not in (torch.float32, torch.bfloat16) or tuple(out.shape) != (B * G * G, Kp) or not out.is_contiguous():
        raise _hip.MuseHipError(f"clip_patch_rows: out is a contiguous f32 / bf16 [{B * G * G}, {Kp}] tensor, got {out.dtype} {tuple(out.shape)}")
    e0 = _prof_begin()
    check(lib().muse_clip_patch_rows(pixel_values.data_ptr(), out.data_ptr(), dt(out), B, I, P, Kp, stream()), "muse_clip_patch_rows")
    _prof_end(e0, "clip_patch_rows", _nbytes(pixel_values, out), "byte")
    return _touched(out)


def clip_vision_embed_ln(patch, class_embedding, position_embedding, w, b, eps, batch):
    """patch f32 [batch * (T - 1), H], class_embedding [H], position_embedding [T, H], w / b [H] -> f32 [batch * T, H]:
    row (b, 0) = LN(class + pos[0]), row (b, t) = LN(patch[b, t - 1] + pos[t]), each * w + b, in one pass"""
    require_gpu(patch, class_embedding, position_embedding, w, b)
    T, H = position_embedding.shape
    for name, t, shape in (("patch", patch, (batch * (T - 1), H)), ("class_embedding", class_embedding, (H,)),
                           ("position_embedding", position_embedding, (T, H)), ("w", w, (H,)), ("b", b, (H,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _hip.MuseHipError(f"clip_vision_embed_ln: {name} is a contiguous f32 {shape} tensor, got {t.dtype} {tuple(t.shape)}")
    y = torch.empty((batch * T, H), dtype=torch.float32, device=patch.device)
    e0 = _prof_begin()
    check(lib().muse_clip_vision_embed_ln(patch.data_ptr(), class_embedding.data_ptr(), position_embedding.data_ptr(), w.data_ptr(),
                                          b.data_ptr(), y.data_ptr(), batch, T, H, eps, stream()), "muse_clip_vision_embed_ln")
    _prof_end(e0, "clip_vision_embed_ln", _nbytes(patch, position_embedding, y), "byte")
    return y


def l2_normalize_rows(x, mult=None, log_mult=None, out=None):
    """x f32 [N, D] -> x / ||x||_2 per row (* mult, a Python float) (* exp(log_mult), a one-element f32 DEVICE tensor: no host read).
    No epsilon: a zero row becomes NaN, as x / x.norm(dim=-1, keepdim=True)."""
    require_gpu(x, log_mult, out)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise _hip.MuseHipError(f"l2_normalize_rows: x is a contiguous f32 [rows, cols] tensor, got {x.dtype} {tuple(x.shape)}")
    if log_mult is not None and (log_mult.dtype != torch.float32 or log_mult.numel() != 1):
        raise _hip.MuseHipError("l2_normalize_rows: log_mult is a one-element f32 tensor")
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous():
        raise _hip.MuseHipError("l2_normalize_rows: out is a contiguous f32 tensor of x's shape")
    N, D = x.shape
    e0 = _prof_begin()
    check(lib().muse_l2_normalize_rows(x.data_ptr(), out.data_ptr(), N, D, 1.0 if mult is None else float(mult), 0 if mult is None else 1,
                                       ptr(log_mult), stream()), "muse_l2_normalize_rows")
    _prof_end(e0, "l2_normalize_rows", _nbytes(x, out), "byte")
    return _touched(out)


# ---- feature statistics (csrc/moments.hip; muse.FeatureStats): the accumulation behind the Frechet distance on CLIP image embeds ---------
def moments_f64_(x, sum, outer):
    """sum f64 [d] += column sums of x, outer f64 [d, d] += x^T x on its upper triangle and diagonal (the strict lower triangle is
    neither read nor written), both IN PLACE, in f64 from exact products, in one launch (muse_moments_f64).  x: f32 [n, d], unit stride
    along a row and any row stride >= d (a column slice of a wider matrix is fine), d a multiple of 4, 16-byte aligned; n = 0 is a
    no-op.  Equal call sequences give equal bits."""
    require_gpu(x, sum, outer)
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _hip.MuseHipError(f"moments_f64_: x is an f32 [n, d] tensor with contiguous rows, got {x.dtype} {tuple(x.shape)} strides {tuple(x.stride())}")
    n, d = int(x.shape[0]), int(x.shape[1])
    ldx = int(x.stride(0)) if n > 1 else d
    if d < 1 or d % 4 or ldx < d:
        raise _hip.MuseHipError(f"moments_f64_: the width {d} is a positive multiple of 4 and the row stride {ldx} is at least the width")
    if sum.dtype != torch.float64 or tuple(sum.shape) != (d,) or not sum.is_contiguous():
        raise _hip.MuseHipError(f"moments_f64_: sum is a contiguous f64 [{d}] tensor, got {sum.dtype} {tuple(sum.shape)}")
    if outer.dtype != torch.float64 or tuple(outer.shape) != (d, d) or not outer.is_contiguous():
        raise _hip.MuseHipError(f"moments_f64_: outer is a contiguous f64 [{d}, {d}] tensor, got {outer.dtype} {tuple(outer.shape)}")
    if n == 0:                  # an empty tensor has no storage to point at
        return outer
    e0 = _prof_begin()
    check(lib().muse_moments_f64(x.data_ptr(), n, d, ldx, sum.data_ptr(), outer.data_ptr(), stream()), "muse_moments_f64")
    _prof_end(e0, "moments_f64", float(n) * d * (d + 1), "flop")
    _touched(sum)
    return _touched(outer)


# ---- Gaussian-kernel pair sums (csrc/mmd.hip; muse.mmd_distance): the sums behind the maximum mean discrepancy on CLIP image embeds --------
def _mmd_rows(name, what, x):
    """x: f32 [n, d], unit stride along a row, d a positive multiple of 4, every row 16-byte aligned -> (n, d, ld)"""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _hip.MuseHipError(f"{name}: {what} is an f32 [n, d] tensor with contiguous rows, got {getattr(x, 'dtype', type(x))} "
                                f"{tuple(getattr(x, 'shape', ()))} strides {tuple(x.stride()) if torch.is_tensor(x) else ()}")
    n, d = int(x.shape[0]), int(x.shape[1])
    ld = int(x.stride(0)) if n > 1 else d
    if d < 1 or d % 4 or ld < d:
        raise _hip.MuseHipError(f"{name}: {what}: the width {d} is a positive multiple of 4 and the row stride {ld} is at least the width")
    if n and (ld % 4 or x.data_ptr() % 16):
        raise _hip.MuseHipError(f"{name}: {what}: every row starts 16-byte aligned (a lane loads a float4): row stride {ld} elements, "
                                f"address % 16 = {x.data_ptr() % 16}")
    return n, d, ld


def _mmd_scales(name, what, r, n, like):
    if r is None:
        return
    require_gpu(r)
    if r.dtype != torch.float64 or tuple(r.shape) != (n,) or not r.is_contiguous() or r.device != like.device:
        raise _hip.MuseHipError(f"{name}: {what} is a contiguous f64 [{n}] tensor on {like.device}, got {r.dtype} {tuple(r.shape)} "
                                f"strides {tuple(r.stride())} on {r.device}")


def row_norms_f64(x, want_rinv=True):
    """x f32 [n, d] -> (sumsq, rinv): sumsq[i] = sum_k x_ik^2 in f64 from exact squares, rinv[i] = 1 / sqrt(sumsq[i]) (None unless
    want_rinv); one launch (muse_row_norms_f64), no host synchronisation.  A zero row gives rinv = inf (and NaN downstream): not
    guarded.  Rows as in rbf_pair_sums_f64."""
    require_gpu(x)
    n, d, ldx = _mmd_rows("row_norms_f64", "x", x)
    sumsq = torch.empty(n, dtype=torch.float64, device=x.device)
    rinv = torch.empty(n, dtype=torch.float64, device=x.device) if want_rinv else None
    if n == 0:                  # an empty tensor has no storage to point at
        return sumsq, rinv
    e0 = _prof_begin()
    check(lib().muse_row_norms_f64(x.data_ptr(), n, d, ldx, sumsq.data_ptr(), ptr(rinv), stream()), "muse_row_norms_f64")
    _prof_end(e0, "row_norms_f64", _nbytes(x, sumsq) + (0 if rinv is None else _nbytes(rinv)), "byte")
    return sumsq, rinv


def rbf_pair_sums_f64(x, y=None, gamma=1.0, rx=None, ry=None):
    """sums of k_ij = exp(-gamma |rx_i x_i - ry_j y_j|^2) over pairs of rows, in f64, without the n x m matrix (muse_rbf_pair_sums_f64:
    the squared distance is (a_i + b_j) - 2 c_ij from exact products, not clamped at 0).  -> f64 [2] on the device, no host
    synchronisation:
        y given: [sum over all i < n, j < m, 0]
        y None : [sum over i < j, sum over i == j] of x against itself; the full sum is 2 * out[0] + out[1]
    x, y: f32 [n, d] / [m, d], unit stride along a row, any row stride >= d that is a multiple of 4, d a multiple of 4, 16-byte aligned.
    rx, ry: None (a factor of 1) or contiguous f64 [n] / [m] (row_norms_f64's rinv for L2-normalised rows).  Equal calls give equal bits."""
    require_gpu(x, y, rx, ry)
    n, d, ldx = _mmd_rows("rbf_pair_sums_f64", "x", x)
    _mmd_scales("rbf_pair_sums_f64", "rx", rx, n, x)
    if y is None:
        if ry is not None:
            raise _hip.MuseHipError("rbf_pair_sums_f64: ry without y (the symmetric form scales both sides by rx)")
        m, ldy = n, ldx
    else:
        m, dy, ldy = _mmd_rows("rbf_pair_sums_f64", "y", y)
        if dy != d or y.device != x.device:
            raise _hip.MuseHipError(f"rbf_pair_sums_f64: x and y have one width and one device, got {d} on {x.device} and {dy} on {y.device}")
        _mmd_scales("rbf_pair_sums_f64", "ry", ry, m, x)
    out = torch.zeros(2, dtype=torch.float64, device=x.device)
    if n == 0 or m == 0:        # an empty tensor has no storage to point at
        return out
    count = int(lib().muse_rbf_pair_sums_workspace(n, m, 1 if y is None else 0))
    if count < 0:
        check(count, "muse_rbf_pair_sums_workspace")
    workspace = torch.empty(count, dtype=torch.float64, device=x.device)
    g = C.c_double(float(gamma))
    e0 = _prof_begin()
    check(lib().muse_rbf_pair_sums_f64(x.data_ptr(), n, ldx, ptr(rx), ptr(y), m, ldy, ptr(ry), d, C.addressof(g), workspace.data_ptr(),
                                       out.data_ptr(), stream()), "muse_rbf_pair_sums_f64")
    pairs = float(n) * (n + 1) / 2 if y is None else float(n) * m
    _prof_end(e0, "rbf_pair_sums_f64", 2.0 * pairs * d, "flop")
    return out
