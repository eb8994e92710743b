"""muse.training_utils - what training/train_muse.py reaches for in `muse.training_utils` (`import muse.training_utils`, :50): seeding
helpers and the four logging diagnostics it computes from a step's logits every `log_*_every` steps (:1319-1375; reference
muse/training_utils.py:27-58, :299-455).  Diagnostics over logits the step already produced, bucketed by the share of masked tokens
per image: with CPU tensors the reference's own torch reductions, which return exactly what the reference's return for the same
tensors - including where the reference's indexing is not what its comments describe (noted inline) - pinned by
tests/golden/training_utils.npz; with logits on the GPU one pass of the row kernels of csrc/diag.hip over the masked rows (see "the
kernel path" below), and `masked_token_diagnostics` for a loop that logs all of them at one step.
The deep-copy `EMA` class of that file is superseded by `muse.EMAModel`, which is what the training script uses (:367-373).
"""
from __future__ import annotations

import collections
import functools
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

_EDGES = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)
_BUCKETS = 10


def set_seed(seed: int):
    """`random`, numpy and torch (all devices) from one seed"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def enable_full_determinism(seed: int):
    """seed everything and ask torch for deterministic algorithms (the environment switches the reference sets are kept: harmless on ROCm)"""
    set_seed(seed)
    os.environ["CUDA_LAUNCH_BLOCKING"] = "1"
    os.environ["CUBLAS_WORKSPACE_CONFIG"] = ":16:8"
    torch.use_deterministic_algorithms(True)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


def input_ids_to_masked_buckets(input_ids, mask_id, total_buckets=10):
    """per image: which tenth its share of masked tokens falls into - (0, 0.1] -> 0, ..., (0.9, 1] -> 9; an image with nothing masked
    also lands in 0.  For ids on the GPU the bucket of every possible masked COUNT 0 ... S is worked out by the same float32 code on
    the CPU, once per S, and looked up by the image's count: a share on a bucket edge must fall as it does in the reference's recorded
    numbers (18 of 20 tokens masked is bucket 8 there), and the same expressions evaluated on the GPU put it into bucket 9"""
    assert total_buckets == _BUCKETS
    count = (input_ids == mask_id).sum(-1)
    if input_ids.is_cuda:
        return _bucket_of_count(input_ids.shape[-1], str(input_ids.device))[count]
    return _buckets_of_counts(count, input_ids.shape[-1])


def _buckets_of_counts(count, seq):
    share = count / seq
    bucket = torch.zeros(share.shape, dtype=torch.long, device=share.device)
    for k in range(1, _BUCKETS):
        bucket += ((_EDGES[k] < share) & (share <= _EDGES[k + 1])) * k
    return bucket


@functools.lru_cache(maxsize=16)
def _bucket_of_count(seq, device):
    return _buckets_of_counts(torch.arange(seq + 1), seq).to(device)


def average_by_buckets(values, masked_buckets, total_buckets):
    """mean of `values` per bucket (0 for an empty bucket).  `values` may be longer than `masked_buckets`: like the reference's
    scatter_add_, only its leading len(masked_buckets) entries take part"""
    total = torch.zeros(total_buckets, device=values.device).scatter_add_(0, masked_buckets, values)
    count = torch.bincount(masked_buckets, minlength=total_buckets).clamp(min=1)
    return total / count


def _pixel_entropy_torch(logits, input_ids, mask_id):
    """entropy of each masked token's predicted distribution, averaged per image over its masked tokens, then per bucket"""
    masked = input_ids == mask_id
    logp = F.log_softmax(logits, dim=-1)
    entropy = -(F.softmax(logits, dim=-1) * logp).sum(-1)
    entropy[~masked] = 0
    per_image = entropy.sum(-1) / masked.sum(-1)
    return average_by_buckets(per_image, input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS), _BUCKETS)


def _image_entropy_torch(logits, input_ids, mask_id):
    """entropy of the image's AVERAGE predicted distribution over its masked tokens, then per bucket"""
    masked = input_ids == mask_id
    probs = F.softmax(logits, dim=-1)
    probs[~masked] = 0
    mean_probs = probs.sum(-2) / masked.sum(-1, keepdim=True)
    per_image = -(mean_probs * mean_probs.log()).sum(-1)
    return average_by_buckets(per_image, input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS), _BUCKETS)


def _cross_entropy_torch(logits, labels, input_ids, mask_id, output_size, label_smoothing):
    """per-token cross-entropy handed to the bucket average.  (The reference passes one value per TOKEN with one bucket index per IMAGE,
    so the average runs over the first batch-size token losses - kept, see average_by_buckets.)"""
    per_token = F.cross_entropy(logits.view(-1, output_size), labels.view(-1), ignore_index=-100, label_smoothing=label_smoothing,
                                reduction="none")
    return average_by_buckets(per_token, input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS), _BUCKETS)


def _token_probability_distributions_torch(logits, input_ids, mask_id):
    """pandas frame {bucket, masked_pixel_prob}: for every bucket that occurs, the predicted distribution of the first masked token of
    ONE image.  (The reference indexes the batch with the bucket's own number - `masked_buckets[masked_buckets == b][0]` is b - kept.)"""
    import pandas as pd
    probs = F.softmax(logits, dim=-1)
    buckets = input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS)
    rows = []
    for b in range(_BUCKETS):
        if not bool((buckets == b).any()):
            continue
        first_masked = probs[b][input_ids[b] == mask_id][0]
        rows += [{"bucket": b, "masked_pixel_prob": p} for p in first_masked.cpu().numpy()]
    return pd.DataFrame(rows)


# ---- the kernel path: logits on the GPU ---------------------------------------------------------------------------------------------
# The four `_*_torch` functions above are the reference's formulation, kept as it was: they are what runs for CPU tensors (pinned bit
# for bit against the reference module by tests/test_surface.py) and what scripts/diag_timing.py times the kernels against.  With
# CUDA logits the public functions below go through muse_token_stats / muse_masked_mean_probs (csrc/diag.hip) and the training loss's
# own muse_cross_entropy_fwd instead: each logits row is read once (masked rows only), and nothing of the logits' size is allocated -
# the temporaries are [B * S] and [B, V].  `input_ids_to_masked_buckets` and `average_by_buckets` stay in torch ON PURPOSE: they work
# on [B]-sized tensors (and [B, S] ids), where a kernel of this library would save nothing.
#
# Logits handling: always detached (the script hands over the training logits, graph attached) and never written.  A tensor or view
# with unit last stride whose leading dimensions collapse to one row stride - a contiguous [B, S, V], or `logits[..., :codebook_size]`
# of a wider one (ld > V) - goes to the kernels as it is; any other layout is made contiguous first (one copy of the logits).  f32 and
# bf16 only, as the models here return; anything else raises MuseHipError.

MaskedTokenDiagnostics = collections.namedtuple("MaskedTokenDiagnostics", [
    "buckets",                      # [B] long: input_ids_to_masked_buckets
    "pixel_entropy_per_image",      # [B]: mean entropy of the masked tokens' predicted distributions (NaN: no masked token)
    "image_entropy_per_image",      # [B]: entropy of the mean predicted distribution over the masked tokens
    "token_cross_entropy",          # [B * S]: F.cross_entropy(..., reduction="none"); None without labels
    "pixel_entropy",                # [10]: pixel_entropy_per_percent_masked_bucket
    "image_entropy",                # [10]: image_entropy_per_percent_masked_bucket
    "cross_entropy",                # [10]: cross_entropy_per_percent_masked_bucket; None without labels
])


def _logit_rows(logits, vocab=None):
    """the detached logits as the [rows, V] strided view the kernels read (see "Logits handling" above)"""
    x = logits.detach()
    if vocab is not None and x.shape[-1] != vocab:                      # the reference's logits.view(-1, output_size) regrouping
        return x.contiguous().view(-1, vocab)
    V = x.shape[-1]
    lead = [(n, st) for n, st in zip(x.shape[:-1], x.stride()[:-1]) if n != 1]
    ld = lead[-1][1] if lead else V
    if not ((x.stride(-1) == 1 or V == 1) and ld >= V and all(lead[i][1] == lead[i + 1][0] * lead[i + 1][1] for i in range(len(lead) - 1))):
        x, ld = x.contiguous(), V
    return x.as_strided((x.numel() // V, V), (ld, 1))


def _ids_2d(input_ids):
    return input_ids.reshape(-1, input_ids.shape[-1]).long().contiguous()


def _entropies(x, ids, mask_id, pixel=True, image=True):
    """-> (pixel entropy per image [B] or None, image entropy per image [B] or None): one muse_token_stats launch over the masked
    rows (entropy, row maximum and sum of exponentials from one read) and the [B, S] entropies' mean per image, then one
    muse_masked_mean_probs launch over the same rows and its [B, V] entropy"""
    from . import ops
    masked = ids == mask_id
    _, ent, row_max, sum_exp = ops.token_stats(x, row_mask=masked.view(-1), want_max_sum=True)
    # unselected rows are exact zeros, as entropy[~masked] = 0; the sum over S in the library's fixed order: torch's depends on B
    per_pixel = ops.masked_row_mean(ent.view(ids.shape), ids, mask_id) if pixel else None
    per_image = ops.masked_mean_probs(x, ids, row_max, sum_exp, mask_id)[1] if image else None
    return per_pixel, per_image


def _token_cross_entropy(logits, labels, output_size, label_smoothing):
    from . import ops
    return ops.cross_entropy_fwd(_logit_rows(logits, output_size), labels.reshape(-1).long().contiguous(), float(label_smoothing),
                                 want_rows=True)[2]


def pixel_entropy_per_percent_masked_bucket(logits, input_ids, mask_id):
    """entropy of each masked token's predicted distribution, averaged per image over its masked tokens, then per bucket"""
    if not logits.is_cuda:
        return _pixel_entropy_torch(logits, input_ids, mask_id)
    per_image, _ = _entropies(_logit_rows(logits), _ids_2d(input_ids), mask_id, image=False)
    return average_by_buckets(per_image, input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS), _BUCKETS)


def image_entropy_per_percent_masked_bucket(logits, input_ids, mask_id):
    """entropy of the image's AVERAGE predicted distribution over its masked tokens, then per bucket"""
    if not logits.is_cuda:
        return _image_entropy_torch(logits, input_ids, mask_id)
    _, per_image = _entropies(_logit_rows(logits), _ids_2d(input_ids), mask_id, pixel=False)
    return average_by_buckets(per_image, input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS), _BUCKETS)


def cross_entropy_per_percent_masked_bucket(logits, labels, input_ids, mask_id, output_size, label_smoothing):
    """per-token cross-entropy handed to the bucket average.  (The reference passes one value per TOKEN with one bucket index per IMAGE,
    so the average runs over the first batch-size token losses - kept, see average_by_buckets.)"""
    if not logits.is_cuda:
        return _cross_entropy_torch(logits, labels, input_ids, mask_id, output_size, label_smoothing)
    per_token = _token_cross_entropy(logits, labels, output_size, label_smoothing)
    return average_by_buckets(per_token, input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS), _BUCKETS)


def token_probability_distributions_per_percent_masked_bucket(logits, input_ids, mask_id):
    """pandas frame {bucket, masked_pixel_prob}: for every bucket that occurs, the predicted distribution of the first masked token of
    ONE image.  (The reference indexes the batch with the bucket's own number - `masked_buckets[masked_buckets == b][0]` is b - kept,
    with its IndexError for a bucket number >= B and for an image b without a masked token.)  On the GPU the ten candidate rows are
    gathered first and only they are softmaxed (muse_softmax_fwd); one device-to-host copy brings them and the flags over."""
    if not logits.is_cuda:
        return _token_probability_distributions_torch(logits, input_ids, mask_id)
    import pandas as pd
    from . import ops
    x, ids = _logit_rows(logits), _ids_2d(input_ids)
    (B, S), V = ids.shape, x.shape[1]
    masked = ids == mask_id
    occurs = torch.bincount(input_ids_to_masked_buckets(ids, mask_id, _BUCKETS), minlength=_BUCKETS) > 0
    image = torch.arange(_BUCKETS, device=x.device).clamp(max=B - 1)               # bucket number -> the image it indexes (clamped: b >= B raises below)
    first = masked.int().argmax(-1)[image]                                         # its first masked token (0 if it has none: raises below)
    probs = x.index_select(0, image * S + first).float()
    ops.softmax_(probs, _BUCKETS, V, V)
    host = torch.cat([occurs.float()[:, None], masked.any(-1)[image].float()[:, None], probs], dim=1).cpu()   # the one device-to-host copy
    rows = []
    for b in range(_BUCKETS):
        if not host[b, 0]:
            continue
        if b >= B:
            raise IndexError(f"index {b} is out of bounds for dimension 0 with size {B}")
        if not host[b, 1]:
            raise IndexError("index 0 is out of bounds for dimension 0 with size 0")
        rows += [{"bucket": b, "masked_pixel_prob": p} for p in host[b, 2:].numpy()]
    return pd.DataFrame(rows)


def masked_token_diagnostics(logits, labels, input_ids, mask_id, label_smoothing=0.0):
    """Everything the three bucket functions compute, for a loop that logs them at the same step: one muse_token_stats launch, one
    muse_masked_mean_probs launch plus its entropy, and one cross-entropy forward (`labels=None` skips it) over logits [B, S, V] on the
    GPU -> MaskedTokenDiagnostics.  The [10] entries equal the three functions' results bit for bit (the same launches)."""
    from ._hip import require_gpu
    require_gpu(logits, input_ids, labels)
    x, ids = _logit_rows(logits), _ids_2d(input_ids)
    buckets = input_ids_to_masked_buckets(input_ids, mask_id, _BUCKETS)
    pixel, image = _entropies(x, ids, mask_id)
    per_token = None if labels is None else _token_cross_entropy(logits, labels, logits.shape[-1], label_smoothing)
    return MaskedTokenDiagnostics(buckets, pixel, image, per_token, average_by_buckets(pixel, buckets, _BUCKETS),
                                  average_by_buckets(image, buckets, _BUCKETS),
                                  None if labels is None else average_by_buckets(per_token, buckets, _BUCKETS))


@torch.no_grad()
def log_grad_norm(model):
    """training/train_muse.py:1309-1314 (`log_grad_norm`, every `experiment.log_grad_norm_every` steps) without its one norm and one
    `.item()` per parameter: -> {"grad_norm/" + name: ||grad||_2 / grad.numel()} for every parameter that has a gradient - the
    reference's formula (:1313) -, all norms from one launch chain of the HIP norm kernels and ONE device-to-host copy.  Hand the
    dictionary to `accelerator.log(..., step=global_step)`.  Call it where the reference does, between backward and
    `optimizer.zero_grad()`."""
    from .training import named_grad_norms
    names, norms = named_grad_norms(model)
    if not names:
        return {}
    numel = {n: p.numel() for n, p in model.named_parameters()}
    values = norms.tolist()                       # the one device-to-host copy
    return {"grad_norm/" + n: v / numel[n] for n, v in zip(names, values)}
