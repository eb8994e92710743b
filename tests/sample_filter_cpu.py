"""The top-k / nucleus (top-p) filter of muse_sample_step_filtered restated on the CPU in float64: the oracle of
tests/test_gpu_sample_filter.py (semantics: include/muse_hip.h at muse_sample_step_filtered, ops.sample_step).

  top_k: keep j iff l_j >= v_k, the k-th largest value of the row (all ties at v_k kept); top_k >= vocab: off.
  top_p: with p = softmax(l) over the codes that survive top_k, keep j iff M_gt(j) = sum over {i : l_i > l_j} of p_i is < top_p
         (a tie group is kept or dropped whole, the largest logit always stays); top_p == 1: off.
"""
import torch


def kept_mask(logits, top_k=None, top_p=None):
    """logits [..., V] (the f32 values the kernel sees, i.e. after the guidance mix) -> (kept [..., V] bool, M_gt [..., V] float64).
    M_gt is taken over the distribution renormalised on the top-k set; a code outside that set has probability 0 there and carries
    the mass of everything above it like any other code."""
    l = logits.double()
    V = l.shape[-1]
    kept = torch.ones_like(l, dtype=torch.bool)
    if top_k is not None and top_k < V:
        kept = l >= torch.sort(l, dim=-1, descending=True).values[..., top_k - 1:top_k]
    p = torch.where(kept, l, torch.full_like(l, float("-inf"))).softmax(dim=-1)
    srt, idx = torch.sort(l, dim=-1, descending=True, stable=True)
    ps = p.gather(-1, idx)
    before = ps.cumsum(-1) - ps                                   # mass at earlier sorted positions
    first = torch.ones_like(srt, dtype=torch.bool)                # the first position of each group of equal logits
    first[..., 1:] = srt[..., 1:] != srt[..., :-1]
    # every member of a tie group takes the group's first entry (`before` never decreases, so a running maximum carries it along)
    m_sorted = torch.where(first, before, torch.full_like(before, -1.0)).cummax(-1).values
    m_gt = torch.empty_like(l).scatter_(-1, idx, m_sorted)
    if top_p is not None and top_p < 1.0:
        kept = kept & (m_gt < top_p)
    return kept, m_gt


def filtered_logits(logits, kept):
    """the logits a filtered step samples from: -inf where the code is dropped"""
    return torch.where(kept, logits, torch.full_like(logits, float("-inf")))
