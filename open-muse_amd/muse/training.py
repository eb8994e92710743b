"""Train-step pieces of the hot path that live in the reference's *training script* rather than in its package:

  * prepare_inputs_and_labels  — training/train_maskgit_imagenet.py:357-394 (VQ encode + cosine-schedule mask sampling)
  * FusedAdamW                 — the `fused_adamw` optimizer choice (:242-261, apex FusedAdam adam_w_mode), one HIP
                                 launch over the model's flat parameter buffer
  * FusedLion                  — the `lion` optimizer choice (training/train_muse.py:405-424, training/optimizer.py): the same
                                 machinery and kernels with Lion's update rule
  * GradReducer                — replaces accelerate/DDP (:152-158, :305, :433): bucketed all-reduce of the flat
                                 gradient buffer over RCCL (xGMI) on a side stream, overlapped with backward
  * TrainStep                  — the loop body (:405-452) strung together for benchmarks / smoke tests
"""
from __future__ import annotations

import os
import weakref
import warnings
from typing import Optional

import torch
import torch.distributed as dist

from . import ops
from ._hip import MuseHipError


@torch.no_grad()
def prepare_inputs_and_labels(vq_model, pixel_values, class_ids, mask_id, min_masking_rate: float = 0.0, timesteps=None,
                              noise=None, generator=None, image_tokens=None, codebook_size=None, use_soft_code_target=False,
                              soft_code_temp=1.0, use_stochastic_code=False):
    """-> (input_ids [B,S+1], labels [B,S+1], soft_targets, mask_prob [B]).

    `timesteps` [B] and `noise` [B,S] are the two torch.rand draws of the reference (:375, :381); pass them in for
    bit-reproducible masks (parity tests), otherwise they are drawn on the GPU.  With pre-encoded `image_tokens` the
    tokenizer is not touched: `vq_model` may be None when `codebook_size` (the class-token offset, :388) is given.

    `use_soft_code_target` (config.training.use_soft_code_target, :364-367): tokens and soft_targets [B, S, codebook] come from
    `vq_model.get_soft_code(pixel_values, soft_code_temp, use_stochastic_code)`; otherwise soft_targets is None."""
    if use_soft_code_target and image_tokens is not None:
        raise ValueError("prepare_inputs_and_labels: use_soft_code_target needs the images - pre-encoded image_tokens carry no soft codes")
    if codebook_size is None:
        if vq_model is None:
            raise ValueError("prepare_inputs_and_labels: without a vq_model pass codebook_size (the class-token offset)")
        codebook_size = vq_model.num_embeddings
    soft_targets = None
    if use_soft_code_target:
        soft_targets, image_tokens = vq_model.get_soft_code(pixel_values, temp=soft_code_temp, stochastic=use_stochastic_code)
    elif image_tokens is None:
        image_tokens = vq_model.get_code(pixel_values)      # == vq_model.encode(pixel_values)[1] (:369) without the unused z_q
    B, S = image_tokens.shape
    dev = image_tokens.device
    if timesteps is None:
        timesteps = torch.rand(B, device=dev, generator=generator)
    if noise is None:
        noise = torch.rand(B, S, device=dev, generator=generator)
    input_ids, labels, mask_prob = ops.mask_sample(image_tokens.contiguous(), class_ids.contiguous(),
                                                   timesteps.float().contiguous(), noise.float().contiguous(), int(mask_id),
                                                   int(codebook_size), float(min_masking_rate))
    return input_ids, labels, soft_targets, mask_prob


class _SoftTargetCE(torch.autograd.Function):
    """muse_soft_ce_fwd / muse_soft_ce_bwd on logits [B, S+1, V]: the loss and, in backward, g_logits shaped like logits"""

    @staticmethod
    def forward(ctx, logits, labels, soft_targets):
        B, S1, V = logits.shape
        x = logits.reshape(B * S1, V)
        lab = labels.contiguous().view(-1)
        soft = soft_targets.contiguous()
        loss_out, lse, psum = ops.soft_ce_fwd(x, lab, soft, S1)
        ctx.save_for_backward(x, lab, soft, lse, psum, loss_out)
        ctx.shape = (B, S1, V)
        return loss_out[0]

    @staticmethod
    def backward(ctx, g):
        x, lab, soft, lse, psum, loss_out = ctx.saved_tensors
        dl = ops.soft_ce_bwd(x, lab, soft, ctx.shape[1], lse, psum, loss_out, g.reshape(1).to(torch.float32).contiguous())
        return dl.view(ctx.shape), None, None


def soft_target_cross_entropy(logits, labels, soft_targets):
    """soft_target_cross_entropy of training/train_maskgit_imagenet.py:101-117 (the class-conditional MaskGitTransformer's
    loss under config.training.use_soft_code_target): position 0 (the class token) of logits [B, S+1, V] and labels [B, S+1] is
    dropped, logits are cut to their first K = soft_targets.shape[-1] columns, and sum(-soft_targets * log_softmax) over the rows
    whose label is not -100, divided by the number of those rows (0 rows: nan, like the reference).  Two HIP kernels; backward
    returns d(loss)/d(logits) shaped like logits, zero outside the first K columns of counted rows.  f32 logits / targets only."""
    ops.require_gpu(logits, labels, soft_targets)
    if logits.dtype != torch.float32 or soft_targets.dtype != torch.float32:
        raise MuseHipError(f"soft_target_cross_entropy: f32 logits and soft_targets only (got {logits.dtype} / {soft_targets.dtype})")
    if labels.dtype != torch.int64:
        raise ValueError(f"soft_target_cross_entropy: labels must be int64 (got {labels.dtype})")
    if (logits.dim() != 3 or labels.dim() != 2 or soft_targets.dim() != 3 or tuple(labels.shape) != tuple(logits.shape[:2])
            or logits.shape[1] < 2 or tuple(soft_targets.shape[:2]) != (logits.shape[0], logits.shape[1] - 1)
            or not 0 < soft_targets.shape[2] <= logits.shape[2]):
        raise ValueError(f"soft_target_cross_entropy: expected logits [B, S+1, V], labels [B, S+1] and soft_targets [B, S, K <= V]; got "
                         f"{tuple(logits.shape)}, {tuple(labels.shape)} and {tuple(soft_targets.shape)}")
    # "f16" compute mode: the gradient operand scale is bounded by the loss's row count (tape_ops.f16_grad_scale_for) - the same bound
    # the engine records for its own cross entropy, set here for the model whose logits these are
    model = getattr(logits.grad_fn, "model", None)
    if model is not None and hasattr(model, "f16_grad_scale_for"):
        model.__dict__["_loss_rows"] = logits.shape[0] * logits.shape[1]
    return _SoftTargetCE.apply(logits, labels, soft_targets)


def mask_or_random_replace_tokens(image_tokens, mask_id, config, mask_schedule=None, is_train=True, *, timesteps=None, noise=None,
                                  rects=None, generator=None):
    """training/train_muse.py:149-226 on the device (muse_mask_tokens), same signature and return value
    `(input_ids, labels, loss_weight, mask_prob)`; `config` is read like the reference reads its OmegaConf node
    (`config.training.get(...)`, `config.training.min_masking_rate`).

    Host-side randomness follows the reference: `random.choices` for eval_mask_ratios, `random.random()` /
    `random.randint` for the contiguous-region coin and rectangle (which costs the reference - and this function - one
    device read of the per-image mask counts); the two device draws (`timesteps` [B], `noise` [B, S]) can be passed in for
    bit-reproducible masks.  The reference's `noise_type` test (:202) is always true, so "random_replace" also writes the mask
    id; that is kept."""
    import math
    import random
    tr = config.training
    B, S = image_tokens.shape
    dev = image_tokens.device
    mask_prob_in = None
    if not is_train and tr.get("eval_mask_ratios", None):
        mask_prob_in = torch.tensor(random.choices(tr.eval_mask_ratios, k=B), device=dev)
    elif timesteps is None:
        timesteps = torch.rand(B, device=dev, generator=generator)
    if mask_prob_in is None and mask_schedule is not None:
        from .sampling import cosine_schedule
        if mask_schedule is not cosine_schedule:       # any other schedule: evaluate it like the reference does (:160-161)
            mask_prob_in = mask_schedule(timesteps.float()).clip(tr.min_masking_rate)
    region_p = tr.get("mask_contiguous_region_prob", None)
    region = region_p is not None and random.random() < region_p
    if region and rects is None:
        # ONE mask_prob for the rectangle sizes and for the kernel (which otherwise evaluates its own double-precision cosine: the two
        # could disagree at a .5 rounding boundary): the f32 cosine of the reference (:160-161) is handed to muse_mask_tokens
        mp = mask_prob_in if mask_prob_in is not None else torch.cos(timesteps.float() * (math.pi * 0.5)).clip(tr.min_masking_rate)
        mask_prob_in = mp
        counts = (S * mp).round().clamp(min=1).tolist()
        res = int(S ** 0.5)
        boxes = []
        for n in counts:                                # :186-199, the reference's "a bit handwavy" rectangle
            n = int(n)
            h = min(random.randint(math.ceil(n / res), min(res, n)), res)
            w = min(math.ceil(n / h), res)
            boxes.append([random.randint(0, res - h), random.randint(0, res - w), h, w])
        rects = torch.tensor(boxes, dtype=torch.int32)
    if not region:
        rects = None
        if noise is None:
            noise = torch.rand(B, S, device=dev, generator=generator)
    all_labels = bool(tr.get("predict_all_tokens", False)) or tr.get("noise_type", "mask") == "random_replace"
    input_ids, labels, loss_weight, mask_prob = ops.mask_tokens(
        image_tokens, int(mask_id), timesteps=None if mask_prob_in is not None else timesteps, mask_prob=mask_prob_in, noise=noise,
        rects=rects, min_masking_rate=float(tr.min_masking_rate), all_labels=all_labels, want_weight=all_labels)
    return input_ids, labels, loss_weight, mask_prob


def cond_dropout(encoder_hidden_states, clip_embeds, empty_embeds, empty_clip_embeds, cond_dropout_prob, uniforms=None,
                 generator=None):
    """training/train_muse.py:715-731: one uniform per image decides, for the text states and the pooled embedding alike,
    whether the conditioning is kept (u < p) or replaced by the empty-prompt embedding -> (encoder_hidden_states, cond_embeds)"""
    B = encoder_hidden_states.shape[0]
    if uniforms is None:
        uniforms = torch.rand(B, device=encoder_hidden_states.device, generator=generator)
    enc = ops.cond_dropout(encoder_hidden_states, empty_embeds, uniforms, cond_dropout_prob).view(encoder_hidden_states.shape)
    cond = ops.cond_dropout(clip_embeds, empty_clip_embeds, uniforms, cond_dropout_prob).view(clip_embeds.shape)
    # (the kernel works in f32; torch.where in the reference keeps the inputs' dtype)
    return enc.to(encoder_hidden_states.dtype), cond.to(clip_embeds.dtype)


def _owner_of(params, who="FusedAdamW"):
    """the muse.MaskGitTransformer that owns all `params` in its flat buffer, or None when the parameters are ordinary tensors
    (muse.MaskGiTUViT): those are stepped one launch per tensor with the same kernel"""
    owner = None
    if all(getattr(p, "_muse_owner", None) is None for p in params):
        return None
    for p in params:
        ref = getattr(p, "_muse_owner", None)
        m = ref() if ref is not None else None
        if m is None:
            raise MuseHipError(f"{who}: either all or none of the parameters may live in a flat parameter buffer")
        if owner is None:
            owner = m
        elif owner is not m:
            raise MuseHipError(f"{who}: parameters of several models in one optimizer are not supported")
    return owner


def _flat_grad_checked(model, params, who="FusedAdamW"):
    """the flat gradient buffer, after making sure it really holds this step's gradients: every p.grad must be the
    parameter's view of it (what backward writes with model.direct_grad); a gradient that lives elsewhere (autograd-
    returned with direct_grad=False, or assigned by the user) is copied in."""
    g = model.flat_grads()
    for p, gv in zip(params, model._grad_views):
        if not p.requires_grad:
            raise MuseHipError(f"{who} steps the whole flat buffer: a frozen parameter (requires_grad=False) is not supported")
        if p.grad.data_ptr() != gv.data_ptr():
            if p.grad.shape != gv.shape:
                raise MuseHipError(f"{who}: gradient shape differs from its parameter")
            gv.copy_(p.grad)
            p.grad = gv
    return g


class _FlatNormState:
    """what the gradient-norm kernels need for a model with a flat gradient buffer, built once: the {offset, n} table of its
    parameters and the chunk prefix sums (on the host for muse_gradnorm_flat's range check, on the device for the kernels) and the
    slab of f64 partials - one per (parameter, 4096-element chunk), then the finalize kernel's scratch (one per parameter and its
    zeroed ticket)."""

    def __init__(self, model):
        flat = model.flat_params()
        order = model._param_order()
        sizes = [p.numel() for p in order]
        first, self.nchunks = ops.chunk_first(sizes)
        self.key = (flat.device, tuple(model._offsets), tuple(sizes))
        self.ptab_host = torch.tensor([[o, n] for o, n in zip(model._offsets, sizes)], dtype=torch.int64)
        self.first_host = torch.tensor(first, dtype=torch.int32)
        self.ptab, self.first = self.ptab_host.to(flat.device), self.first_host.to(flat.device)
        self.nt = len(sizes)
        self.slab = torch.zeros(self.nchunks + self.nt + 1, dtype=torch.float64, device=flat.device)

    @staticmethod
    def of(model):
        st = model.__dict__.get("_muse_gradnorm")
        flat = model.flat_params()
        if st is None or st.key != (flat.device, tuple(model._offsets), tuple(p.numel() for p in model._param_order())):
            st = model.__dict__["_muse_gradnorm"] = _FlatNormState(model)
        return st

    def accumulate(self, g, begin, end):
        """the parameters inside [begin, end) of the flat gradient buffer g -> their chunks of the slab (current stream)"""
        ops.gradnorm_flat(g, begin, end - begin, self.ptab_host, self.first_host, self.ptab, self.first, self.slab)

    def finish(self, g, covered, grad_scale, max_norm):
        """cover what `covered` ([(begin, end), ...], accumulated earlier) left out, then the finalize launch -> out (f32 [3 + nt]:
        norm, coef, scale, per-parameter norms)"""
        pos = 0
        for b, e in sorted(covered):
            if b > pos:
                self.accumulate(g, pos, b)
            pos = max(pos, e)
        if pos < g.numel():
            self.accumulate(g, pos, g.numel())
        out = torch.empty(3 + self.nt, dtype=torch.float32, device=g.device)
        ops.gradnorm_finalize(self.slab, self.first, self.nt, self.slab[self.nchunks:], grad_scale, max_norm, out)
        return out


def _multi_norm(table, chunk_first, nt, nchunks, slab, grad_scale, max_norm):
    """the multi-tensor form: sums of squares over a FusedAdamW-style pointer table, then the finalize launch -> out"""
    if slab is None or slab.numel() != nchunks + nt + 1 or slab.device != table.device:
        slab = torch.zeros(nchunks + nt + 1, dtype=torch.float64, device=table.device)   # (partials, per-parameter sums, the zeroed ticket)
    ops.gradnorm_multi(table, chunk_first, nt, nchunks, slab)
    out = torch.empty(3 + nt, dtype=torch.float32, device=table.device)
    ops.gradnorm_finalize(slab, chunk_first, nt, slab[nchunks:], grad_scale, max_norm, out)
    return out, slab


def _grad_table(grads):
    """device pointer table in muse_adamw_multi's layout (only the gradient pointer and n filled) for a list of gradient tensors
    -> (table, chunk_first, nchunks).  One (pageable) host -> device copy: the optimizer's own path keeps its pinned staging."""
    rows = []
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise MuseHipError("muse.clip_grad_norm_ / grad_norms: gradients must be contiguous float32 tensors")
        rows.append((0, g.data_ptr(), 0, 0, 0, g.numel()))
    first, nchunks = ops.chunk_first(g.numel() for g in grads)
    dev = grads[0].device
    return torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(first, dtype=torch.int32).to(dev), nchunks


def _norm_target(parameters_or_model):
    """-> (flat-buffer model or None, the parameters that have a gradient, in the order of the norms)"""
    if isinstance(parameters_or_model, torch.Tensor):
        parameters_or_model = [parameters_or_model]
    model = parameters_or_model if hasattr(parameters_or_model, "parameters") else None
    params = list(model.parameters() if model is not None else parameters_or_model)
    owner = _owner_of(params) if params else None
    if owner is not None:
        theirs = owner._param_order()
        if len(params) == len(theirs) and {id(q) for q in params} == {id(q) for q in theirs} and owner._flat_ok() \
                and all(q.grad is not None for q in theirs):
            return owner, theirs
    return None, [q for q in params if q.grad is not None]


def _run_norm(parameters_or_model, max_norm, scale_in_place):
    """-> (out of the finalize launch or None when there is no gradient, the parameters the per-parameter norms belong to)"""
    owner, params = _norm_target(parameters_or_model)
    if not params:
        return None, params
    if owner is not None:
        g = _flat_grad_checked(owner, params, "muse.clip_grad_norm_")
        out = _FlatNormState.of(owner).finish(g, [], 1.0, max_norm)
        if scale_in_place:
            ops.grad_scale_flat_(g, out[1:2])
            ops._touched(g)
        return out, params
    grads = [q.grad for q in params]
    ops.require_gpu(*grads)
    table, first, nchunks = _grad_table(grads)
    out, _ = _multi_norm(table, first, len(grads), nchunks, None, 1.0, max_norm)
    if scale_in_place:
        ops.grad_scale_multi_(table, first, len(grads), nchunks, out[1:2])
        for g in grads:
            ops._touched(g)
    return out, params


@torch.no_grad()
def clip_grad_norm_(parameters_or_model, max_norm, return_coef=False):
    """Drop-in for `accelerator.clip_grad_norm_(model.parameters(), max_norm)` / `torch.nn.utils.clip_grad_norm_` (norm_type 2;
    training/train_muse.py:758-759) for loops that keep the reference's statement order or another optimizer: the global L2 norm of
    the gradients by the HIP norm kernels (f64 sums, deterministic), then `grad *= min(1, max_norm / (norm + 1e-6))` in place by one
    more launch (applied also when the coefficient is 1, as torch does).  No device-to-host copy.  Takes a model or its parameters:
    a muse.MaskGitTransformer's flat gradient buffer in one piece, ordinary tensors (muse.MaskGiTUViT) through one pointer table.
    -> the norm before clipping, a 0-dim device tensor (with `return_coef`: (norm, coefficient)).  With muse.FusedAdamW prefer
    `FusedAdamW(max_grad_norm=...)`: same result bit for bit, without the write pass over the gradient."""
    out, params = _run_norm(parameters_or_model, float(max_norm), True)
    if out is None:
        z = torch.zeros((), dtype=torch.float32)
        return (z, torch.ones_like(z)) if return_coef else z
    return (out[0], out[1]) if return_coef else out[0]


@torch.no_grad()
def grad_norms(model_or_parameters):
    """L2 norm of every gradient -> f32 device tensor [number of parameters that have a gradient] (order: the model's flat-buffer
    order for a flat-buffer model with all gradients present - see named_grad_norms -, else the order given): one launch chain, no
    device-to-host copy."""
    out, params = _run_norm(model_or_parameters, float("inf"), False)
    if out is None:
        return torch.zeros(0, dtype=torch.float32)
    return out[3:]


@torch.no_grad()
def named_grad_norms(model):
    """-> ([names], f32 device tensor of their gradients' L2 norms), for the parameters that have a gradient"""
    out, params = _run_norm(model, float("inf"), False)
    names = {id(p): n for n, p in model.named_parameters()}
    if out is None:
        return [], torch.zeros(0, dtype=torch.float32)
    return [names[id(p)] for p in params], out[3:]


class _FusedOptimizer(torch.optim.Optimizer):
    """What muse.FusedAdamW and muse.FusedLion share - everything but the update rule: ownership of a model's flat buffers and its
    parameter-group segments, the per-tensor pointer table, stepping inside backward / behind the reducer's buckets, clipping by the
    global norm read on the device, the "f16" overflow guard and the refresh of the weights' operand images.  A rule supplies its
    constructor (param_groups defaults, then `_init_fused`), `_who` (its name in messages), the state tensors (`_tensor_state`,
    `_ensure_flat_state`), the launches (`_launch_flat`, `_launch_multi`) and `state_dict` / `load_state_dict`."""
    _who = "FusedOptimizer"
    _rule = "the update"
    _subset_hint = "torch.optim.AdamW"     # what the "whole flat buffer" message recommends for a subset of the parameters

    def _init_fused(self, max_grad_norm):
        # Parameter groups: `params` may be the list of dicts training/train_muse.py:425-445 builds (weight decay on the matrices,
        # none on bias / LayerNorm / embedding weights) - torch.optim semantics, every group its own lr / betas / eps / weight_decay.
        # One group runs the single-set kernels (muse_adamw_flat / _multi); several run the *_groups kernels, still ONE launch.
        if len(self.param_groups) > 8:
            raise MuseHipError(f"{self._who}: at most 8 parameter groups (got {len(self.param_groups)})")
        every = self._all_params()
        owner = _owner_of(every, self._who)
        self._model = weakref.ref(owner) if owner is not None else None
        self._flat_gid = self._seg_dev = None
        if owner is not None:
            theirs = owner._param_order()
            if len(every) != len(theirs) or {id(q) for q in every} != {id(q) for q in theirs}:
                raise MuseHipError(f"{self._who} steps the model's whole flat parameter buffer: pass model.parameters() "
                                   f"(all of them, as one list or split into groups); for a subset use {self._subset_hint}")
            gid = {id(q): k for k, grp in enumerate(self.param_groups) for q in grp["params"]}
            self._flat_gid = [gid[id(q)] for q in theirs]           # group of each parameter, in the flat buffer's order
        self._m = self._v = None
        self._step = 0
        self._table = self._chunk_first = self._table_key = self._stage = None   # per-tensor mode: device table of muse_adamw_multi
        self._ranges_done = self._ranges_done_live = None                        # (step, [(begin, end), ...]) applied inside backward
        self._upd_stream, self._upd_used = None, False                           # stream of the per-bucket update (begin_step_in_reducer)
        self.grad_scale = 1.0   # multiplied into the gradient inside the kernel (GradReducer sets 1/world for SUM reductions)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = self.last_clip_coef = None
        self._norm_done = self._norm_live = None     # (step, [(begin, end), ...]) whose sums of squares backward already delivered
        self._norm_slab = None                       # per-tensor mode: the slab of f64 partials

    def _all_params(self):
        """every parameter, in torch.optim's state-dict order (group by group)"""
        return [q for grp in self.param_groups for q in grp["params"]]

    def _segments(self, model):
        """device tables of the flat buffer's parameter-group segments: (seg_end int64 - absolute element offsets -, seg_group int32).
        Neighbouring parameters of one group form one segment; a parameter's alignment padding stays with it."""
        flat = model.flat_params()
        if self._seg_dev is not None and self._seg_dev[0].device == flat.device and self._seg_dev[2] == tuple(model._offsets):
            return self._seg_dev[0], self._seg_dev[1]
        ends, gids = [], []
        offs = list(model._offsets) + [flat.numel()]
        for i, k in enumerate(self._flat_gid):
            if gids and gids[-1] == k:
                ends[-1] = offs[i + 1]
            else:
                ends.append(offs[i + 1])
                gids.append(k)
        self._seg_dev = (torch.tensor(ends, dtype=torch.int64, device=flat.device),
                         torch.tensor(gids, dtype=torch.int32, device=flat.device), tuple(model._offsets))
        return self._seg_dev[0], self._seg_dev[1]

    @torch.no_grad()
    def step(self, closure=None):
        self._check_not_partial()
        loss = closure() if closure is not None else None
        if self._model is None:
            return self._step_per_tensor(loss)
        model = self._model()
        if model is None:
            raise MuseHipError(f"{self._who}: the model that owned these parameters is gone")
        if not model._flat_ok():
            raise MuseHipError(f"{self._who}: the model's flat parameter buffer was rebuilt (model.to(...) / load after the "
                               "optimizer was created is fine, replacing p.data is not)")
        flat = model.flat_params()
        order = model._param_order()
        if any(p.grad is None for p in order):
            if all(p.grad is None for p in order):
                return loss  # nothing to do before the first backward (torch skips None grads)
            raise MuseHipError(f"{self._who}: some parameters have no gradient; the flat step needs all of them")
        g = _flat_grad_checked(model, order, self._who)
        self._ensure_flat_state(flat)
        self._step += 1
        shadow = model._flat_c if model._flat_c is not None and model._flat_c.device == flat.device else None
        done = self._ranges_done
        self._ranges_done = None
        normed, self._norm_done = self._norm_done, None
        guards, skip = self._f16_guard_on(flat.device)     # ("f16" mode: as in _step_per_tensor - the update is skipped on the device on overflow)
        try:
            if self.max_grad_norm is not None:
                # clipping: sums of squares of what backward has not delivered, the finalize launch, ONE update that reads the scale
                # from the device (on an "f16" step that overflowed the norm is simply non-finite and the guard skips the update)
                covered = normed[1] if normed is not None and normed[0] == self._step else []
                out = _FlatNormState.of(model).finish(g, covered, float(self.grad_scale), float(self.max_grad_norm))
                self.last_grad_norm, self.last_clip_coef = out[0], out[1]
                self._apply(model, 0, flat.numel(), shadow, skip, scale_dev=out[2:3])
            elif done is not None and done[0] == self._step:
                # backward already applied this step's update range by range (begin_step_in_backward); cover what it did not report
                covered = sorted(done[1])
                pos = 0
                for b, e in covered:
                    if b > pos:
                        self._apply(model, pos, b, shadow, skip)
                    pos = max(pos, e)
                if pos < flat.numel():
                    self._apply(model, pos, flat.numel(), shadow, skip)
            else:
                self._apply(model, 0, flat.numel(), shadow, skip)
        finally:
            self._f16_guard_off(guards)
        model._note_shadow_refreshed(shadow is not None)
        return loss

    def _apply(self, model, b, e, shadow, skip=None, scale_dev=None):
        # (the guard only when there is one: an unguarded update stays the call it always was, so a stand-in for ops.adamw_flat /
        #  adamw_flat_groups written without the keyword - a host-logic test, a CPU restatement of the kernel - keeps working; the
        #  same for the device-side gradient factor of a clipped step)
        guard = {} if skip is None else {"skip": skip}
        if scale_dev is not None:
            guard["scale_dev"] = scale_dev
        self._launch_flat(model, b, e, shadow, guard)

    @property
    def _step_for_apply(self):
        d = self._ranges_done_live
        return d[0] if d is not None else self._step

    def begin_step_in_backward(self, model):
        """Arm the optimizer to apply THIS step's update inside backward: every time backward reports a finished range of the flat
        gradient buffer (model.grad_ready_hook) the AdamW kernel runs on that slice, on the stream the report comes from (the
        weight-gradient stream) - the HBM-bound update hides behind the MFMA-bound dX chain of the earlier layers instead of
        following backward.  Element-wise identical to one launch over the whole buffer.  The following step() only advances the
        step count and covers ranges backward did not report.  Valid when nothing sits between backward and step(): no gradient
        clipping, no gradient accumulation, no all-reduce (muse.TrainStep checks this and arms it).  Never for a model in the "f16"
        compute mode: its update waits for the whole backward pass's overflow guard (step())."""
        self._check_not_partial()
        if model.__dict__.get("_f32_f16", False) or self.max_grad_norm is not None:
            return False                      # (clipping: no update before the last gradient exists - begin_norm_in_backward)
        flat = model.flat_params()
        self._ensure_flat_state(flat)
        if any((o * 4) % 16 for o in model._offsets):
            return False                      # (slices must keep the kernel's 16-byte alignment)
        self._ranges_done_live = (self._step + 1, [])
        self._direct_grad_before = model.direct_grad
        shadow = model.compute_weights(torch.bfloat16) if model._resolve_cd() == torch.bfloat16 else None

        def hook(begin, end):
            live = self._ranges_done_live
            if live is None or end <= begin:
                return
            self._apply(model, begin, end, model._flat_c if shadow is not None else None)
            live[1].append((begin, end))
        model.direct_grad = True
        model.grad_ready_hook = hook
        return True

    def end_step_in_backward(self, model, failed=False):
        """`failed`: backward raised.  Ranges it had already reported carry this step's update (weights changed, moments advanced)
        while the step count has not: the step can be neither retried nor skipped, and every later call says so."""
        model.grad_ready_hook = None
        model.direct_grad = getattr(self, "_direct_grad_before", model.direct_grad)
        self._ranges_done, self._ranges_done_live = self._ranges_done_live, None
        if failed and self._ranges_done is not None and self._ranges_done[1]:
            self._partial_step = True

    def _check_not_partial(self):
        if getattr(self, "_partial_step", False):
            raise MuseHipError(f"{self._who}: an earlier step failed inside backward after {self._rule} had already been applied to part of "
                               "the parameters (in-backward / behind-the-all-reduce update); the optimizer state is inconsistent - "
                               "restore parameters and optimizer from a checkpoint (or set MUSE_OPT_IN_BACKWARD=0 / "
                               "MUSE_OPT_IN_REDUCER=0 to keep the update out of backward)")

    def begin_step_in_reducer(self, model, reducer):
        """The data-parallel form of begin_step_in_backward: the AdamW kernel runs on each gradient bucket right after its all-reduce
        (GradReducer.post_reduce), while backward is still computing the earlier layers and the next bucket is being filled - instead
        of one pass over all parameters after the last all-reduce.  The kernel runs on the reducer's (high-priority) stream, behind
        the bucket's collective.  MUSE_OPT_REDUCER_STREAM=own puts it on a normal-priority stream of its own instead (same results
        bit for bit, but measured much slower at one rank: 69.6 vs 61.5 ms per step, profiles/r02_ab_dp1_updstream_*.json - the
        low-priority update is starved until the end of the step and then serialises).  Same validity conditions as
        begin_step_in_backward; call end_step_in_reducer after reducer.finish()."""
        if model.__dict__.get("_f32_f16", False) or self.max_grad_norm is not None:
            return False
        flat = model.flat_params()
        self._ensure_flat_state(flat)
        if any((o * 4) % 16 for o in model._offsets):
            return False
        self._ranges_done_live = (self._step + 1, [])
        has_shadow = model._resolve_cd() == torch.bfloat16
        if has_shadow:
            model.compute_weights(torch.bfloat16)
        # where the per-bucket update runs: "comm" (default) = the reducer's high-priority stream right behind the collective;
        # "side" = the model's weight-gradient stream, in order with the dW GEMMs still to come (the placement of the single-GPU
        # in-backward update); "own" = a normal-priority stream of its own.  One-rank launch line on MI355X, per step
        # (profiles/r03_dp1_update_placement.txt): comm 60.7 ms / side 62.2 ms with the default 4 hardware queues, 66.7 / 65.8 ms
        # with GPU_MAX_HW_QUEUES=8 (plain single-GPU step on that box: 59.9 ms) - the 8-queue penalty is not the update's placement.
        where = os.environ.get("MUSE_OPT_REDUCER_STREAM", "comm")
        own = flat.is_cuda and where in ("own", "side")
        if own and where == "side" and hasattr(model, "_wgrad_side_stream"):
            self._upd_stream = model._wgrad_side_stream(flat.device)
        elif own and (self._upd_stream is None or self._upd_stream.device != flat.device or
                      self._upd_stream is getattr(model, "_side_stream", None)):
            self._upd_stream = torch.cuda.Stream(device=flat.device)
        self._upd_used = False

        def hook(begin, end):
            live = self._ranges_done_live
            if live is None or end <= begin:
                return
            if own:
                self._upd_stream.wait_stream(torch.cuda.current_stream(flat.device))   # (the reducer's stream, behind the collective)
                with torch.cuda.stream(self._upd_stream):
                    self._apply(model, begin, end, model._flat_c if has_shadow else None)
                self._upd_used = True
            else:
                self._apply(model, begin, end, model._flat_c if has_shadow else None)
            live[1].append((begin, end))
        reducer.post_reduce = hook
        return True

    def end_step_in_reducer(self, reducer, failed=False):
        reducer.post_reduce = None
        if self._upd_used:   # the caller's stream continues behind the last bucket's update
            torch.cuda.current_stream(self._upd_stream.device).wait_stream(self._upd_stream)
            self._upd_used = False
        self._ranges_done, self._ranges_done_live = self._ranges_done_live, None
        if failed and self._ranges_done is not None and self._ranges_done[1]:
            self._partial_step = True

    # ---- clipping: the sums of squares overlapped with backward ---------------------------------------------------------------------
    def begin_norm_in_backward(self, model):
        """With `max_grad_norm` set the update cannot start before the last gradient exists, but the norm can be accumulated where the
        update runs otherwise: every time backward reports a finished range of the flat gradient buffer (model.grad_ready_hook, on the
        weight-gradient stream) the sum-of-squares kernel runs on that range, and step() is left with the ranges that were never
        reported, the finalize launch and the update.  Ranges are whole parameters, partials go to fixed slots of a slab: the norm is
        bit-identical to the one step() alone computes.  Arm it around the LAST backward before step() (gradient accumulation: the
        earlier micro-batches' backward runs unarmed); pair with end_norm_in_backward.  Nothing is applied inside backward, so a
        backward that raises leaves the step retryable - unlike begin_step_in_backward."""
        self._check_not_partial()
        if self.max_grad_norm is None or self._model is None or self._model() is not model or model.__dict__.get("_f32_f16", False):
            return False                      # ("f16" compute mode: as for the update, everything waits for the whole backward pass)
        st = _FlatNormState.of(model)
        self._norm_live = (self._step + 1, [])
        self._direct_grad_before = model.direct_grad

        def hook(begin, end):
            live = self._norm_live
            if live is None or end <= begin:
                return
            st.accumulate(model.flat_grads(), begin, end)
            live[1].append((begin, end))
        model.direct_grad = True
        model.grad_ready_hook = hook
        return True

    def end_norm_in_backward(self, model, failed=False):
        """`failed`: backward raised - what it had accumulated is dropped, step() takes the whole norm itself"""
        model.grad_ready_hook = None
        model.direct_grad = getattr(self, "_direct_grad_before", model.direct_grad)
        self._norm_done, self._norm_live = (None if failed else self._norm_live), None

    def begin_norm_in_reducer(self, model, reducer):
        """The data-parallel form: the sum-of-squares kernel runs on each bucket right behind its all-reduce (GradReducer.post_reduce),
        on the reducer's stream, so the norm is that of the averaged gradient - the same bytes on every rank, hence the same norm and
        coefficient bit for bit without another collective.  Under reducer.no_sync() no bucket is reduced and nothing is accumulated;
        the synchronising backward reports the accumulated gradient.  Call end_norm_in_reducer after reducer.finish()."""
        self._check_not_partial()
        if self.max_grad_norm is None or self._model is None or self._model() is not model or model.__dict__.get("_f32_f16", False):
            return False
        st = _FlatNormState.of(model)
        self._norm_live = (self._step + 1, [])

        def hook(begin, end):
            live = self._norm_live
            if live is None or end <= begin:
                return
            st.accumulate(model.flat_grads(), begin, end)
            live[1].append((begin, end))
        reducer.post_reduce = hook
        return True

    def end_norm_in_reducer(self, reducer, failed=False):
        reducer.post_reduce = None
        self._norm_done, self._norm_live = (None if failed else self._norm_live), None

    def _step_per_tensor(self, loss):
        """parameters that are ordinary (contiguous f32) tensors: one muse_adamw_multi launch over all of them.  torch.optim.AdamW
        semantics: a parameter without a gradient is skipped and keeps its own state; the step count is shared (all
        parameters of these models receive a gradient every step).  With several parameter groups the table carries each
        tensor's group and the launch is muse_adamw_multi_groups."""
        params = [(p, k) for k, grp in enumerate(self.param_groups) for p in grp["params"] if p.grad is not None]
        # (operand planes of the bf16x3 mode ride in the group column of the grouped table: a one-group model with planes takes that kernel too)
        multi = len(self.param_groups) > 1 or any(getattr(p, "_muse_planes", None) is not None
                                                  or getattr(getattr(p, "_muse_shadow", None), "dtype", None) == torch.float16 for p, _ in params)
        if not params:
            return loss
        self._step += 1
        rows = []
        for p, gk in params:
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                raise MuseHipError(f"{self._who}: parameters and gradients must be contiguous float32 tensors")
            state_ptrs = self._tensor_state(p)          # (m, v) pointers of the rule's state for p, created / moved to p's device
            shadow = getattr(p, "_muse_shadow", None)   # the model's cached bf16 compute copy of this weight (MaskGiTUViT bf16 mode)
            if shadow is not None and (shadow.numel() != p.numel() or shadow.device != p.device or not shadow.is_contiguous()):
                shadow = None
            # ... or (bf16x3 mode, tape_ops._wp) its (hi, lo) operand planes: hi-plane rows + the element distance to the lo plane, which
            # rides in the group column above bit 8
            lo = -1 if (shadow is not None and shadow.dtype == torch.float16) else 0     # ("f16" mode: the copy is IEEE half)
            planes = getattr(p, "_muse_planes", None)
            if planes is not None and shadow is None and planes[0].numel() == p.numel() and planes[0].device == p.device \
                    and planes[0].is_contiguous() and planes[1] > 0:
                shadow, lo = planes[0], int(planes[1])
            row = (p.data.data_ptr(), p.grad.data_ptr()) + state_ptrs + (shadow.data_ptr() if shadow is not None else 0, p.numel())
            rows.append(row + (gk | (lo << 8),) if multi else row)
        # one launch for all tensors.  Gradients are fresh allocations every step, so the pointer table is rebuilt every step: ~500
        # rows staged through two alternating PINNED host buffers and copied asynchronously (a pageable copy would make the host
        # wait for the stream and lose its run-ahead into the next step)
        dev = params[0][0].device
        ncol = 7 if multi else 6
        key = tuple(rows)
        if self._table_key != key:
            nt = len(rows)
            if self._table is None or self._table.shape[0] < nt or self._table.shape[1] != ncol or self._table.device != dev:
                self._table = torch.empty((nt, ncol), dtype=torch.int64, device=dev)
                self._chunk_first = torch.empty(nt + 1, dtype=torch.int32, device=dev)
                self._stage = [(torch.empty((nt, ncol), dtype=torch.int64).pin_memory(), torch.empty(nt + 1, dtype=torch.int32).pin_memory(),
                                torch.cuda.Event()) for _ in range(2)]
                self._stage_i = 0
            ht, hf, ev = self._stage[self._stage_i]
            self._stage_i ^= 1
            ev.synchronize()      # the copy issued from this staging buffer two rebuilds ago has run
            first, nchunks = ops.chunk_first(r[5] for r in rows)
            ht[:nt].copy_(torch.tensor(rows, dtype=torch.int64))
            hf[:nt + 1].copy_(torch.tensor(first, dtype=torch.int32))
            self._table[:nt].copy_(ht[:nt], non_blocking=True)
            self._chunk_first[:nt + 1].copy_(hf[:nt + 1], non_blocking=True)
            ev.record(torch.cuda.current_stream(dev))
            self._table_key, self._nchunks = key, nchunks
        # "f16" compute mode: the update is guarded ON THE DEVICE by the overflow counter of the backward pass that made these gradients
        # (an operand beyond half's range turns them NaN): the kernel leaves parameters and moments untouched when it is non-zero, the
        # model's next backward pass halves the gradient scale (tape_ops._gemm_mode) - GradScaler's policy without a host round trip
        # (the host does not know about the skip when it happens: self._step advances anyway, so the bias corrections of the following
        #  updates are those of one step later - a factor that tends to 1)
        guards, skip = self._f16_guard_on(dev)
        clip = {}
        if self.max_grad_norm is not None:      # the norm over the same pointer table, then the update reads the scale from the device
            out, self._norm_slab = _multi_norm(self._table, self._chunk_first, len(rows), self._nchunks, self._norm_slab,
                                               float(self.grad_scale), float(self.max_grad_norm))
            self.last_grad_norm, self.last_clip_coef = out[0], out[1]
            clip = {"scale_dev": out[2:3]}
        try:
            self._launch_multi(multi, len(rows), dict(grad_scale=float(self.grad_scale), skip=skip, **clip))
        finally:
            self._f16_guard_off(guards)
        return loss

    def _f16_guard_on(self, dev):
        """"f16" compute mode: the device-side skip of the update that follows is the overflow counter of the backward pass(es) that
        made these gradients - passes of a model whose parameters this optimizer steps (F16Images.owner); a pass of any other model gates
        nothing here.  -> (the guards to hand to _f16_guard_off once the update is enqueued, the counter the update's kernel reads or None)"""
        if not ops._F16_GUARDS:
            return [], None
        mine, guards = None, []
        for images in list(ops._F16_GUARDS):
            model = images.owner() if images.owner is not None else None
            if model is None or images._stats is None or images._stats.device != dev:
                continue
            if mine is None:
                mine = {id(q) for q in self._all_params()}
            if any(id(q) in mine for q in model.parameters()):
                guards.append(images)
        if not guards:
            return [], None
        for images in guards:
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(images._stats)        # every rank skips together (GradScaler's found_inf all-reduce)
        # (one counter the kernel reads; two models stepped by one optimizer: their sum, stream-ordered like the update)
        skip = guards[0]._stats if len(guards) == 1 else torch.stack([g._stats for g in guards]).sum(0, dtype=torch.int32)
        return guards, skip

    def _f16_guard_off(self, guards):
        """the guarded update is enqueued: take each pass's counters off the device for its model's scale policy"""
        for images in guards:
            images.after_optimizer_step()
            ops._F16_GUARDS.discard(images)

    # ---- the rule's state: `_MOMENTS` names its tensors ((state-dict key, attribute), the first one `_m`), `_HAS_STEP` whether its
    # checkpoints carry a step count.  Flat mode: one buffer per moment, shaped like the model's flat parameter buffer; per-tensor mode:
    # one dict per moment, keyed by id(parameter)
    _MOMENTS = ()
    _HAS_STEP = True

    def _ensure_flat_state(self, flat):
        attrs = [a for _, a in self._MOMENTS]
        if self._m is None:
            for a in attrs:
                setattr(self, a, torch.zeros_like(flat))
        elif self._m.device != flat.device:       # the model moved after the state was created / loaded: follow it
            for a in attrs:
                setattr(self, a, getattr(self, a).to(flat.device))
        if self._m.shape != flat.shape:
            raise MuseHipError(f"{self._who}: optimizer state does not match the model's flat parameter buffer")

    def _tensor_state(self, p):
        """per-tensor mode: p's state tensors, created as zeros / moved to p's device -> the table's (m, v) pointer columns (0 where the
        rule has no such moment)"""
        if self._m is None:
            for _, a in self._MOMENTS:
                setattr(self, a, {})
        k, ptrs = id(p), []
        for _, a in self._MOMENTS:
            store = getattr(self, a)
            if k not in store:
                store[k] = torch.zeros_like(p)
            elif store[k].device != p.device:
                store[k] = store[k].to(p.device)
            ptrs.append(store[k].data_ptr())
        return tuple(ptrs) + (0,) * (2 - len(ptrs))

    # ---- checkpointing in the layout of the torch.optim class the rule stands in for ----------------------------------
    def _flat_offsets(self, model):
        return {id(q): o for q, o in zip(model._param_order(), model._offsets)}

    def state_dict(self):
        ps = self._all_params()
        groups, n0 = [], 0
        for grp in self.param_groups:                      # torch.optim's packing: parameters numbered group by group
            g = {k: v for k, v in grp.items() if k != "params"}
            g["params"] = list(range(n0, n0 + len(grp["params"])))
            n0 += len(grp["params"])
            groups.append(g)
        state = {}
        if (self._step > 0 or not self._HAS_STEP) and self._m is not None:
            stepv = torch.tensor(float(self._step))
            head = (lambda: {"step": stepv.clone()}) if self._HAS_STEP else dict
            if self._model is None:
                for i, p in enumerate(ps):
                    if id(p) in self._m:
                        state[i] = dict(head(), **{name: getattr(self, a)[id(p)] for name, a in self._MOMENTS})
            else:
                offs = self._flat_offsets(self._model())
                for i, p in enumerate(ps):
                    o, n = offs[id(p)], p.numel()
                    state[i] = dict(head(), **{name: getattr(self, a)[o:o + n].view(p.shape) for name, a in self._MOMENTS})
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        if "state" not in sd or "param_groups" not in sd:
            raise MuseHipError(f"{self._who}.load_state_dict expects torch.optim's layout {{'state', 'param_groups'}}")
        ps = self._all_params()
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        ids = []
        for mine, grp in zip(self.param_groups, sd["param_groups"]):
            gi = list(grp.get("params", range(len(ids), len(ids) + len(mine["params"]))))
            if len(gi) != len(mine["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            ids += gi
            mine.update({k: v for k, v in grp.items() if k != "params"})
        state = {ids.index(k) if k in ids else k: v for k, v in sd["state"].items()}
        if self._HAS_STEP:
            steps = {int(float(v["step"])) for v in state.values()}
            if len(steps) > 1:
                raise MuseHipError(f"{self._who} keeps one step count for all parameters; the checkpoint has several")
            self._step = steps.pop() if steps else 0
        attrs = [a for _, a in self._MOMENTS]
        if not state:
            for a in attrs:
                setattr(self, a, None)
            return
        model = self._model() if self._model is not None else None
        if model is None:
            for a in attrs:
                setattr(self, a, {})
            for i, st in state.items():
                p = ps[i]
                for name, a in self._MOMENTS:
                    t = st[name]
                    if tuple(t.shape) != tuple(p.shape):
                        raise ValueError(f"{self._who}.load_state_dict: {name} of parameter {i} has shape {tuple(t.shape)}, "
                                         f"expected {tuple(p.shape)}")
                    getattr(self, a)[id(p)] = t.detach().to(device=p.device, dtype=torch.float32).contiguous().clone()
            return
        if len(state) != len(ps):
            raise MuseHipError(f"{self._who} (flat): the checkpoint must carry state for every parameter")
        flat = model.flat_params()
        offs = self._flat_offsets(model)
        for a in attrs:
            setattr(self, a, torch.zeros_like(flat))
        for i, p in enumerate(ps):
            o, n = offs[id(p)], p.numel()
            for name, a in self._MOMENTS:
                t = state[i][name]
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"{self._who}.load_state_dict: {name} of parameter {i} has shape {tuple(t.shape)}, "
                                     f"expected {tuple(p.shape)}")
                getattr(self, a)[o:o + n].view(p.shape).copy_(t.detach().to(device=flat.device, dtype=torch.float32))


class FusedAdamW(_FusedOptimizer):
    """AdamW (decoupled weight decay, torch.optim.AdamW numerics) as ONE kernel launch over the model's flat f32
    parameter / gradient buffers; also refreshes the bf16 compute copy of the weights in the same pass.

    Drop-in for `optimizer_cls(model.parameters(), lr=..., betas=..., weight_decay=..., eps=...)`.  `state_dict()` /
    `load_state_dict()` use torch.optim.AdamW's layout ({"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups"}),
    so optimizer checkpoints written by the reference's `adamw` choice load here and vice versa.

    `max_grad_norm` (also an attribute; None = off): clip the gradient by its global L2 norm inside the step - the semantics of
    `accelerator.clip_grad_norm_(model.parameters(), max_grad_norm)` right before `optimizer.step()` (training/train_muse.py:758-761):
    step() = norm kernels (for whatever begin_norm_in_backward / begin_norm_in_reducer have not already delivered) -> one finalize
    launch -> ONE AdamW launch that reads `grad_scale * min(1, max_grad_norm / (norm + 1e-6))` from device memory.  No device-to-host
    copy, no stream synchronisation.  `p.grad` is left UNSCALED (that write pass is what is saved): code that reads the gradients
    after step() sees the unclipped ones - use muse.clip_grad_norm_ where the clipped gradient itself is needed.  After the step
    `last_grad_norm` (the norm before clipping, of the gradient times `grad_scale`) and `last_clip_coef` are 0-dim device tensors.
    It is not a param_groups default and does not enter state_dict(): checkpoints keep torch.optim.AdamW's layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._init_fused(max_grad_norm)

    _who = "FusedAdamW"
    _rule = "AdamW"
    _MOMENTS = (("exp_avg", "_m"), ("exp_avg_sq", "_v"))

    def _launch_flat(self, model, b, e, shadow, guard):
        flat, g = model.flat_params(), model.flat_grads()
        if len(self.param_groups) > 1:
            seg_end, seg_group = self._segments(model)
            ops.adamw_flat_groups(flat[b:e], g[b:e], self._m[b:e], self._v[b:e], None if shadow is None else shadow[b:e], b,
                                  seg_end, seg_group, self.param_groups, self._step_for_apply, grad_scale=float(self.grad_scale), **guard)
            return
        grp = self.param_groups[0]
        ops.adamw_flat(flat[b:e], g[b:e], self._m[b:e], self._v[b:e], None if shadow is None else shadow[b:e], float(grp["lr"]),
                       grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], self._step_for_apply,
                       grad_scale=float(self.grad_scale), **guard)

    def _launch_multi(self, multi, nrows, kw):
        if multi:
            ops.adamw_multi_groups(self._table, self._chunk_first, nrows, self._nchunks, self.param_groups, self._step, **kw)
        else:
            grp = self.param_groups[0]
            ops.adamw_multi(self._table, self._chunk_first, nrows, self._nchunks, float(grp["lr"]), grp["betas"][0], grp["betas"][1],
                            grp["eps"], grp["weight_decay"], self._step, **kw)


class FusedLion(_FusedOptimizer):
    """Lion (the reference's `lion` optimizer choice, training/optimizer.py) on muse.FusedAdamW's machinery with the update rule
    swapped: ONE launch over the model's flat buffers (or over the pointer table of a model with ordinary parameters), the weights'
    bf16 / bf16x3 / half images refreshed in the same pass, parameter groups, `max_grad_norm`, the "f16" overflow guard, stepping
    inside backward and behind the reducer's buckets - see muse.FusedAdamW.  The arithmetic is the reference class's, rounding by
    rounding (lion_update1 of csrc/optim.hip): p = p * (1 - lr * wd) - lr * sign(beta1 * m + (1 - beta1) * g), then
    m = beta2 * m + (1 - beta2) * g.  The state is `exp_avg` alone: 4 bytes per parameter against AdamW's 8.

    Drop-in for `Lion(params, lr=..., betas=..., weight_decay=...)` with the reference's defaults and argument checks; further keyword
    arguments are accepted and ignored, as there.  `state_dict()` / `load_state_dict()` use the reference class's layout ({"state":
    {i: {"exp_avg"}}, "param_groups": [{lr, betas, weight_decay, params}]}: no step count, no exp_avg_sq), so a checkpoint written
    by the reference's `lion` choice loads here and vice versa."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, max_grad_norm=None, **kwargs):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        super().__init__(list(params), dict(lr=lr, betas=betas, weight_decay=weight_decay))
        self._init_fused(max_grad_norm)

    _who = "FusedLion"
    _rule = "Lion"
    _subset_hint = "the reference's Lion class"
    _MOMENTS = (("exp_avg", "_m"),)
    _HAS_STEP = False

    def _launch_flat(self, model, b, e, shadow, guard):
        flat, g = model.flat_params(), model.flat_grads()
        if len(self.param_groups) > 1:
            seg_end, seg_group = self._segments(model)
            ops.lion_flat_groups(flat[b:e], g[b:e], self._m[b:e], None if shadow is None else shadow[b:e], b, seg_end, seg_group,
                                 self.param_groups, grad_scale=float(self.grad_scale), **guard)
            return
        grp = self.param_groups[0]
        ops.lion_flat(flat[b:e], g[b:e], self._m[b:e], None if shadow is None else shadow[b:e], float(grp["lr"]), grp["betas"][0],
                      grp["betas"][1], grp["weight_decay"], grad_scale=float(self.grad_scale), **guard)

    def _launch_multi(self, multi, nrows, kw):
        if multi:
            ops.lion_multi_groups(self._table, self._chunk_first, nrows, self._nchunks, self.param_groups, **kw)
        else:
            grp = self.param_groups[0]
            ops.lion_multi(self._table, self._chunk_first, nrows, self._nchunks, float(grp["lr"]), grp["betas"][0], grp["betas"][1],
                           grp["weight_decay"], **kw)


def grouped_parameters(model, weight_decay, no_decay=("bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight")):
    """The two parameter groups of training/train_muse.py:425-437 - weight decay on everything whose name carries none of the
    `no_decay` fragments, 0.0 on the rest - ready for `muse.FusedAdamW(grouped_parameters(model, wd), lr=..., weight_decay=wd)`."""
    named = list(model.named_parameters())
    return [
        {"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": weight_decay},
        {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0},
    ]


class GradReducer:
    """Data-parallel gradient averaging.  muse.MaskGitTransformer: the flat gradient buffer is all-reduced in large
    contiguous buckets (default 64 MiB; xGMI rings are per-link bound, so few large messages) as soon as backward has
    finished writing them, on a side stream, while backward keeps computing earlier layers.

    The mean is taken by the collective itself (`ReduceOp.AVG`, one pass) on RCCL; on gloo (CPU tests), which has no
    AVG, the bucket is pre-scaled.  `grad_dtype=torch.bfloat16` sends each bucket as bf16 (half the xGMI bytes:
    SURVEY.md section 5 sizes config B at 1.5 ms instead of 3.0 ms per step) and expands the reduced bucket back to f32.

    torch.distributed's "nccl" backend is RCCL on ROCm; on CPU tensors (gloo) the same logic runs synchronously, which
    is how the world_size-2 tests cover it."""

    def __init__(self, model, process_group=None, bucket_bytes: int = 64 << 20, broadcast_params: bool = True,
                 grad_dtype=torch.float32):
        if not dist.is_initialized():
            raise MuseHipError("GradReducer needs an initialised torch.distributed process group")
        if grad_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("grad_dtype must be torch.float32 or torch.bfloat16")
        self.model = model
        self.pg = process_group
        self.world = dist.get_world_size(process_group)
        # gloo has no ReduceOp.AVG: pre-scale and SUM (also for GPU tensors: protocol tests of the N > 1 path run two gloo ranks on one GPU)
        self._has_avg = dist.get_backend(process_group) != "gloo"
        self.bucket_elems = max(1, bucket_bytes // 4)
        self.grad_dtype = grad_dtype
        self._hi = self._lo = None
        self._handles = []
        self._stream = None
        self.post_reduce = None   # callable(lo, hi): runs on the reduction stream right after bucket [lo, hi) has been averaged
        self.stats = {"buckets": 0, "bytes": 0}
        # bench.py's `comm` block: a list here makes every flat-buffer bucket leave (start event, end event, payload bytes) on the
        # communication stream and finish() an event at the point where backward's last kernel has been enqueued on the compute
        # stream - per bucket, the share of its all-reduce that ran before that point is what backward hid (bucket_overlap())
        self.trace = None
        self._bwd_end = None
        self._sync = True         # False inside no_sync(): gradient accumulation, no collective
        self._deferred = False    # tape engines: this backward adds to existing gradients -> the SUM is reduced in finish()
        # Models with a flat gradient buffer (MaskGitTransformer) report finished ranges during backward.  Models whose
        # parameters are ordinary tensors (MaskGiTUViT: one autograd node hands every gradient back at once) are reduced in
        # finish(): gradients packed, in reverse parameter order, into the same large buckets.
        self._flat_mode = hasattr(model, "flat_grads") and hasattr(model, "grad_ready_hook")
        if self._flat_mode:
            model.direct_grad = True
            model.grad_ready_hook = self._on_ready
            if broadcast_params:
                dist.broadcast(model.flat_params(), src=0, group=process_group)  # DDP's constructor sync (:305)
                model.mark_weights_changed()
        else:
            self._params = [p for p in model.parameters() if p.requires_grad]
            # the tape engines (MaskGiTUViT, text-conditioned MaskGitTransformer) report finished gradients from inside their
            # hand-written backward: buckets are packed and all-reduced on the communication stream while backward computes the
            # earlier blocks (DDP's overlap, training/train_muse.py:753-759); finish() then has nothing left to do.  Models without
            # the hook are reduced after backward.
            self._pending, self._pending_n, self._in_backward_done = [], 0, False
            if hasattr(model, "grad_tensors_hook"):
                model.grad_tensors_hook = self._on_tensors
            if broadcast_params:
                with torch.no_grad():
                    for bucket in self._buckets([p.data for p in self._params]):
                        flat = torch.cat([t.reshape(-1) for t in bucket])
                        dist.broadcast(flat, src=0, group=process_group)
                        o = 0
                        for t in bucket:
                            t.copy_(flat[o:o + t.numel()].view_as(t))
                            o += t.numel()
                if hasattr(model, "mark_weights_changed"):
                    model.mark_weights_changed()

    def no_sync(self):
        """Gradient accumulation: backward inside this context keeps the gradients local (no collective, no per-bucket callback), like
        `DistributedDataParallel.no_sync()` - what `accelerator.accumulate(model)` enters on all but the last micro-batch of
        `gradient_accumulation_steps` (training/train_muse.py:734; 2 in ten of the reference's configurations, cc12m_uvit_clip.yaml among
        them).  The first synchronising backward after it averages the ACCUMULATED gradients: the flat buffer already holds the sum when
        its ranges are reported; the tape engines hand over only that micro-batch's gradients, so their in-backward buckets are skipped
        for this step and finish() reduces the `.grad` tensors autograd has summed into.

            for i, batch in enumerate(micro_batches):
                with (reducer.no_sync() if i + 1 < len(micro_batches) else contextlib.nullcontext()):
                    loss(batch).backward()
            reducer.finish(); optimizer.step(); optimizer.zero_grad(set_to_none=True)"""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            prev, self._sync = self._sync, False
            try:
                yield self
            finally:
                self._sync = prev
        return ctx()

    def _buckets(self, tensors):
        """consecutive tensors grouped into buckets of >= bucket_elems elements (the last one may be smaller)"""
        out, cur, n = [], [], 0
        for t in tensors:
            cur.append(t)
            n += t.numel()
            if n >= self.bucket_elems:
                out.append(cur)
                cur, n = [], 0
        if cur:
            out.append(cur)
        return out

    def _on_tensors(self, tensors, final, side_stream=None):
        """called from inside backward (TapeOps._report_grads) with gradient tensors that are complete on the model's compute stream
        (and its weight-gradient stream `side_stream`).  They are collected into buckets of >= bucket_elems elements; a full bucket is
        packed, all-reduced and unpacked IN PLACE on the communication stream, behind both compute streams.  `final`: flush the
        rest and make the compute stream wait for every bucket - autograd receives averaged gradients."""
        if not self._sync:
            return                                   # no_sync(): this micro-batch's gradients stay local (autograd accumulates them)
        if not self._pending and not self._deferred and any(p.grad is not None for p in self._params):
            self._deferred = True                    # gradients of earlier micro-batches exist: reduce the sums after backward (finish)
            # ... also when the earlier backward of this step was itself reduced in-backward (two synchronising backwards before one
            # finish()): its averaged gradients are identical on every rank, so averaging the sums again yields avg(g1) + avg(g2),
            # what DDP's per-backward all-reduce produces.  Without this, finish() took the "already reduced" early return and every
            # rank kept avg(g1) + its LOCAL g2.
            self._in_backward_done = False
        if self._deferred:
            return
        for t in tensors:
            self._pending.append(t)
            self._pending_n += t.numel()
        if self._pending and (self._pending_n >= self.bucket_elems or final):
            self._reduce_list(self._pending, side_stream)
            self._pending, self._pending_n = [], 0
        if final:
            for h in self._handles:
                h.wait()
            self._handles = []
            if self._stream is not None and self._live:
                torch.cuda.current_stream().wait_stream(self._stream)
                self._live = False
            self._in_backward_done = True

    _live = False

    def _reduce_list(self, bucket, side_stream=None):
        on_gpu = bucket[0].is_cuda
        self.stats["buckets"] += 1
        self.stats["bytes"] += sum(t.numel() for t in bucket) * (2 if self.grad_dtype == torch.bfloat16 else 4)
        if not on_gpu:
            flat = torch.cat([g.reshape(-1) for g in bucket])
            self._reduce(flat, False)
            o = 0
            for g in bucket:
                g.copy_(flat[o:o + g.numel()].view_as(g))
                o += g.numel()
            return
        if self._stream is None:
            self._stream = torch.cuda.Stream(priority=-1)
        cur = torch.cuda.current_stream()
        self._stream.wait_stream(cur)
        if side_stream is not None:
            self._stream.wait_stream(side_stream)
        with torch.cuda.stream(self._stream):
            flat = torch.cat([g.reshape(-1) for g in bucket])        # pack on the communication stream: no work on the compute streams
            h = self._reduce(flat, True)
            if h is not None:
                h.wait()                                             # stream-side: the unpack below follows the collective
            o = 0
            for g in bucket:
                g.copy_(flat[o:o + g.numel()].view_as(g))
                o += g.numel()
        for g in bucket:
            g.record_stream(self._stream)
        self._live = True

    def _finish_tensor_list(self):
        self._deferred = False
        if not self._sync:
            return
        if self._in_backward_done:           # every gradient was reduced from inside backward (_on_tensors)
            self._in_backward_done = False
            return
        grads = [p.grad for p in reversed(self._params) if p.grad is not None]
        if not grads:
            return
        on_gpu = grads[0].is_cuda
        if on_gpu and self._stream is None:
            self._stream = torch.cuda.Stream(priority=-1)
        packed = []
        for bucket in self._buckets(grads):
            flat = torch.cat([g.reshape(-1) for g in bucket])        # pack (one pass); the collective then moves one large message
            self.stats["buckets"] += 1
            self.stats["bytes"] += flat.numel() * (2 if self.grad_dtype == torch.bfloat16 else 4)
            if on_gpu:
                self._stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._stream):
                    h = self._reduce(flat, True)
                    if h is not None:
                        self._handles.append(h)
                flat.record_stream(self._stream)
            else:
                self._reduce(flat, False)
            packed.append((bucket, flat))
        for h in self._handles:
            h.wait()
        self._handles = []
        if on_gpu:
            torch.cuda.current_stream().wait_stream(self._stream)
        for bucket, flat in packed:                                   # unpack into the .grad tensors the optimizer reads
            o = 0
            for g in bucket:
                g.copy_(flat[o:o + g.numel()].view_as(g))
                o += g.numel()

    def _reduce(self, g, on_gpu):
        """mean over ranks of one bucket (in place)"""
        if self.grad_dtype == torch.bfloat16:
            c = ops.cast_to_bf16(g) if on_gpu else g.to(torch.bfloat16)
            if on_gpu and self._has_avg:
                dist.all_reduce(c, op=dist.ReduceOp.AVG, group=self.pg)
                ops.cast_to_f32(c, g)
            else:   # gloo: no AVG and no bf16 arithmetic guarantee: reduce the bf16-rounded values in f32
                c = c.to(torch.float32).mul_(1.0 / self.world)
                dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.pg)
                g.copy_(c)
            return None
        if on_gpu and self._has_avg:
            return dist.all_reduce(g, op=dist.ReduceOp.AVG, group=self.pg, async_op=True)
        g.mul_(1.0 / self.world)
        dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.pg)
        return None

    def _launch(self, lo, hi):
        g = self.model.flat_grads()[lo:hi]
        self.stats["buckets"] += 1                     # (bench.py's `comm` block: buckets and payload bytes per step)
        self.stats["bytes"] += (hi - lo) * (2 if self.grad_dtype == torch.bfloat16 else 4)
        if g.is_cuda:
            if self._stream is None:
                self._stream = torch.cuda.Stream(priority=-1)
            self._stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._stream):
                ev = None
                if self.trace is not None:
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record()
                h = self._reduce(g, True)
                if ev is not None:
                    if h is not None:
                        h.wait()
                        h = None
                    ev[1].record()
                    self.trace.append((ev[0], ev[1], (hi - lo) * (2 if self.grad_dtype == torch.bfloat16 else 4)))
                if self.post_reduce is not None:
                    if h is not None:
                        h.wait()          # (a stream-side wait: the reduction stream continues behind the collective; the host does not block)
                    self.post_reduce(lo, hi)
                elif h is not None:
                    self._handles.append(h)
        else:
            self._reduce(g, False)
            if self.post_reduce is not None:
                self.post_reduce(lo, hi)

    def _on_ready(self, begin: int, end: int):
        """backward reports finished [begin, end) ranges of the flat grad buffer, from the end of the buffer downward"""
        if not self._sync:
            return                                   # no_sync(): the buffer keeps accumulating, nothing is sent
        if self._hi is None:
            self._hi, self._lo = end, begin
        elif end == self._lo:
            self._lo = begin
        else:  # non-contiguous report: flush what we have and start a new run
            self._launch(self._lo, self._hi)
            self._hi, self._lo = end, begin
        if (self._hi - self._lo) >= self.bucket_elems:
            self._launch(self._lo, self._hi)
            self._hi = self._lo = None

    def finish(self):
        """flush the last bucket and make the compute stream wait for every outstanding all-reduce"""
        if not self._flat_mode:
            return self._finish_tensor_list()
        if not self._sync:
            return
        if self.trace is not None and self.model.flat_grads().is_cuda:
            self._bwd_end = torch.cuda.Event(enable_timing=True)
            self._bwd_end.record()                   # backward's last kernel is on the compute stream; what follows is exposed
        if self._hi is not None:
            self._launch(self._lo, self._hi)
            self._hi = self._lo = None
        for h in self._handles:
            h.wait()
        self._handles = []
        if self._stream is not None:
            torch.cuda.current_stream().wait_stream(self._stream)

    def bucket_overlap(self):
        """after a traced step and a device synchronisation: per bucket {bytes, ms, hidden_fraction} - the share of the bucket's
        all-reduce (as timed on the communication stream) that ran before backward's last kernel was enqueued.  A bucket launched
        in finish() itself (the last, ragged one) is exposed by construction."""
        out = []
        if not self.trace or self._bwd_end is None:
            return out
        for e0, e1, nbytes in self.trace:
            ms = e0.elapsed_time(e1)
            before = e0.elapsed_time(self._bwd_end)          # > 0: the bucket started that long before the end of backward
            hidden = 0.0 if ms <= 0 else max(0.0, min(1.0, before / ms))
            out.append({"bytes": int(nbytes), "ms": round(ms, 3), "hidden_fraction": round(hidden, 3)})
        return out

    def reduce_metrics(self, loss, mask_prob):
        """The two logged scalars of the reference's loop (`accelerator.gather(loss.repeat(bs)).mean()` and
        `accelerator.gather(mask_prob.repeat(bs)).mean()`, train_maskgit_imagenet.py:430-431) as ONE 2-float all-reduce
        instead of two all-gathers of bs and bs^2 floats.  -> (mean loss, mean mask rate) over all ranks."""
        v = torch.stack([loss.detach().float().reshape(()), mask_prob.detach().float().mean()])
        if v.is_cuda and self._has_avg:
            dist.all_reduce(v, op=dist.ReduceOp.AVG, group=self.pg)
        else:
            v.mul_(1.0 / self.world)
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=self.pg)
        return v[0], v[1]


class TrainStep:
    """One optimisation step exactly as the reference's loop body strings it together (:405-452):
    VQ-encode -> mask -> forward(loss) -> backward (+ overlapped gradient all-reduce) -> AdamW -> zero_grad.

    `next_pixel_values`: the following batch's images.  The tokenizer is frozen (`vq_model.requires_grad_(False)`, :283), so its
    token ids do not depend on the optimizer state and the NEXT batch can be encoded while this one trains: the encode is
    enqueued on a second HIP stream before this step's forward (the software analogue of the reference's dataloader workers
    running ahead of the loop; the token ids are bit-identical to encoding inline).  The convolution blocks and the
    transformer's GEMM / HBM-bound kernels then share the chip: each fills the CUs and memory cycles the other leaves idle
    (tile seams, short grids).  The next call picks the tokens up when it is given the same tensor as `pixel_values`.

    `use_soft_code_target` / `soft_code_temp` / `use_stochastic_code` (config.training, :364-367, :421-424): the tokens and the soft
    targets come from `vq_model.get_soft_code`, and the step is `logits = model(input_ids)`, `soft_target_cross_entropy(logits,
    labels, soft_targets)`, backward, AdamW (class-conditional MaskGitTransformer only).  The prefetch then carries both.

    `max_grad_norm` (config.training.max_grad_norm, training/train_maskgit_imagenet.py:435-436): clip the gradient by its global L2
    norm before the update (muse.FusedAdamW's / muse.FusedLion's `max_grad_norm`, which this sets).  The sums of squares are then accumulated where the
    update runs otherwise - inside backward, or behind each bucket's all-reduce - and step() finalizes and updates; the update itself
    cannot overlap backward any more (it needs the last gradient's norm)."""

    def __init__(self, vq_model, model, optimizer, reducer: Optional[GradReducer] = None, label_smoothing: float = 0.0,
                 min_masking_rate: float = 0.0, use_soft_code_target: bool = False, soft_code_temp: float = 1.0,
                 use_stochastic_code: bool = False, max_grad_norm: Optional[float] = None):
        if max_grad_norm is not None:
            if not isinstance(optimizer, _FusedOptimizer):
                raise MuseHipError("TrainStep(max_grad_norm=...) clips inside muse.FusedAdamW's / muse.FusedLion's step; with another optimizer call "
                                   "muse.clip_grad_norm_ between backward and step in a loop of your own")
            optimizer.max_grad_norm = float(max_grad_norm)
        self.vq_model, self.model, self.optimizer, self.reducer = vq_model, model, optimizer, reducer
        self.label_smoothing, self.min_masking_rate = label_smoothing, min_masking_rate
        self.use_soft_code_target, self.soft_code_temp = bool(use_soft_code_target), float(soft_code_temp)
        self.use_stochastic_code = bool(use_stochastic_code)
        self._pf = None          # (pixel tensor, tokens or (soft targets, tokens), ready event) of the prefetched batch
        self._pf_stream = None
        self.compute_priority = -1   # stream priority of the step while a prefetch is in flight (None: stay on the caller's stream)
        self.optimizer_in_backward = os.environ.get("MUSE_OPT_IN_BACKWARD", "1") != "0"
        self.optimizer_in_reducer = os.environ.get("MUSE_OPT_IN_REDUCER", "1") != "0"
        self._hp_stream, self._in_hp = None, False

    @torch.no_grad()
    def _encode(self, pixel_values):
        """tokens, or (soft targets, tokens) in the soft-target mode"""
        if self.use_soft_code_target:
            return self.vq_model.get_soft_code(pixel_values, temp=self.soft_code_temp, stochastic=self.use_stochastic_code)
        return self.vq_model.get_code(pixel_values)

    @torch.no_grad()
    def _prefetch(self, pixel_values):
        if not pixel_values.is_cuda:
            raise MuseHipError("TrainStep: next_pixel_values must be on the GPU")
        main = torch.cuda.current_stream(pixel_values.device)
        if self._pf_stream is None or self._pf_stream.device != pixel_values.device:
            # MUSE_PF_PRIORITY: stream priority of the tokenizer's prefetch stream (default 0 = normal; 1 = low where the runtime offers it)
            self._pf_stream = torch.cuda.Stream(device=pixel_values.device, priority=int(os.environ.get("MUSE_PF_PRIORITY", "0")))
        side = self._pf_stream
        side.wait_stream(main)                      # the images (and the previous use of the tokenizer's buffers) are ready
        with torch.cuda.stream(side), ops.conv_persistent(False):
            # (beside the step the launch-per-tile convolution: a persistent workgroup would hold its CU against the step's stream)
            codes = self._encode(pixel_values)
            ev = torch.cuda.Event()
            ev.record(side)
        pixel_values.record_stream(side)
        self._pf = (pixel_values, codes, ev)

    def __call__(self, pixel_values, class_ids, timesteps=None, noise=None, image_tokens=None, next_pixel_values=None):
        """image_tokens [B, S] int64: pre-encoded VQ tokens (muse.pre_encode; the reference's scripts/pre_encode.py regime) -
        the tokenizer is then skipped and pixel_values may be None"""
        # With a tokenizer pass of the next batch in flight, the train step itself runs on a HIGH-priority stream: the hardware
        # then serves its (latency-critical, serially dependent) kernels first and fits the tokenizer's blocks into what is left
        # (62.3 -> 61.1 ms per step on MI355X; the reverse, a high-priority tokenizer stream, costs 1.5 ms).  The caller's stream is
        # joined on entry and on return, so nothing changes for code around the step.
        if next_pixel_values is not None and self.compute_priority is not None and class_ids.is_cuda and not self._in_hp:
            dev = class_ids.device
            if self._hp_stream is None or self._hp_stream.device != dev:
                self._hp_stream = torch.cuda.Stream(device=dev, priority=self.compute_priority)
            cur = torch.cuda.current_stream(dev)
            self._hp_stream.wait_stream(cur)
            self._in_hp = True
            try:
                with torch.cuda.stream(self._hp_stream):
                    loss, mask_prob = self.__call__(pixel_values, class_ids, timesteps, noise, image_tokens, next_pixel_values)
            finally:
                self._in_hp = False
            cur.wait_stream(self._hp_stream)
            loss.record_stream(cur)
            mask_prob.record_stream(cur)
            return loss, mask_prob
        if self.use_soft_code_target and image_tokens is not None:
            raise ValueError("TrainStep: use_soft_code_target needs the images - pre-encoded image_tokens carry no soft codes")
        soft = None
        if image_tokens is None and self._pf is not None and self._pf[0] is pixel_values:
            _, codes, ev = self._pf
            soft, image_tokens = codes if self.use_soft_code_target else (None, codes)
            main = torch.cuda.current_stream(image_tokens.device)
            main.wait_event(ev)
            image_tokens.record_stream(main)
            if soft is not None:
                soft.record_stream(main)
        elif self._pf is not None and image_tokens is None:
            # the prefetch is keyed by tensor IDENTITY: a different tensor object here means this batch is tokenised a second time
            warnings.warn("TrainStep: the prefetched batch is discarded - `pixel_values` is not the tensor object that was passed as "
                          "`next_pixel_values` to the previous call; this step encodes its images again", RuntimeWarning, stacklevel=2)
        self._pf = None
        if next_pixel_values is not None:
            if image_tokens is None:   # first step of a run: this batch inline, then the next one on the side stream
                codes = self._encode(pixel_values)
                soft, image_tokens = codes if self.use_soft_code_target else (None, codes)
            self._prefetch(next_pixel_values)
        inline_soft = self.use_soft_code_target and image_tokens is None      # encode (soft codes and tokens) right here
        input_ids, labels, soft_inline, mask_prob = prepare_inputs_and_labels(
            self.vq_model, pixel_values, class_ids, self.model.config.mask_token_id, self.min_masking_rate, timesteps, noise,
            image_tokens=image_tokens,
            codebook_size=None if self.vq_model is not None else self.model.config.codebook_size,
            use_soft_code_target=inline_soft, soft_code_temp=self.soft_code_temp, use_stochastic_code=self.use_stochastic_code)
        if soft_inline is not None:
            soft = soft_inline
        if self.use_soft_code_target:
            logits = self.model(input_ids=input_ids)
            loss = soft_target_cross_entropy(logits, labels, soft)
        else:
            _, loss = self.model(input_ids=input_ids, labels=labels, label_smoothing=self.label_smoothing)
        # clipping (FusedAdamW / FusedLion .max_grad_norm): the sums of squares are accumulated where the update would run - the update waits for step()
        clip = isinstance(self.optimizer, _FusedOptimizer) and self.optimizer.max_grad_norm is not None
        flat_model = hasattr(self.model, "grad_ready_hook") and hasattr(self.model, "flat_grads")
        normed = (clip and self.optimizer_in_backward and self.reducer is None and flat_model
                  and self.optimizer.begin_norm_in_backward(self.model))
        normed_r = (clip and not normed and self.optimizer_in_reducer and self.reducer is not None
                    and getattr(self.reducer, "_flat_mode", False) and self.reducer.model is self.model
                    and self.optimizer.begin_norm_in_reducer(self.model, self.reducer))
        # the update inside backward (FusedAdamW / FusedLion .begin_step_in_backward): only when nothing sits between the two - no reducer here
        armed = (not clip and self.optimizer_in_backward and self.reducer is None and isinstance(self.optimizer, _FusedOptimizer)
                 and getattr(self.model, "wgrad_stream", False) and hasattr(self.model, "grad_ready_hook")
                 and self.model._resolve_cd() == torch.bfloat16 and self.optimizer.begin_step_in_backward(self.model))
        # ... and with a reducer: the update on each bucket right behind its all-reduce, on the reducer's stream
        armed_r = (not clip and not armed and self.optimizer_in_reducer and self.reducer is not None and getattr(self.reducer, "_flat_mode", False)
                   and self.reducer.model is self.model and isinstance(self.optimizer, _FusedOptimizer) and loss.is_cuda
                   and self.model._resolve_cd() == torch.bfloat16 and self.optimizer.begin_step_in_reducer(self.model, self.reducer))
        failed = True
        try:
            loss.backward()
            if self.reducer is not None:
                self.reducer.finish()
            failed = False
        finally:
            if armed:
                self.optimizer.end_step_in_backward(self.model, failed=failed)
            if armed_r:
                self.optimizer.end_step_in_reducer(self.reducer, failed=failed)
            if normed:
                self.optimizer.end_norm_in_backward(self.model, failed=failed)
            if normed_r:
                self.optimizer.end_norm_in_reducer(self.reducer, failed=failed)
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        return loss.detach(), mask_prob
