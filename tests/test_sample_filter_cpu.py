"""CPU: tests/sample_filter_cpu.py (the float64 statement of top-k / nucleus filtering the GPU tests hold muse_sample_step_filtered to)
against the usual statements of both filters, its tie rule, and the argument validation of ops.sample_step."""
import pytest
import torch

import sample_filter_cpu as F


def _logits(seed, rows=24, V=32):
    return torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * 2.0


def _brute_m_gt(l, kept):
    """M_gt by its definition, one pair of codes at a time (float64)"""
    l = l.double()
    p = torch.where(kept, l, torch.full_like(l, float("-inf"))).softmax(-1)
    return ((l[..., None, :] > l[..., :, None]) * p[..., None, :]).sum(-1)


@pytest.mark.parametrize("top_p", [0.3, 0.5, 0.9, 0.999])
def test_nucleus_equals_the_sorted_cumsum_statement(top_p):
    """tie-free rows: sort descending, cumsum, drop where the mass before the token is >= top_p"""
    l = _logits(1)
    assert all(len(set(r.tolist())) == l.shape[1] for r in l)
    kept, m_gt = F.kept_mask(l, top_p=top_p)
    srt, idx = torch.sort(l.double(), dim=-1, descending=True)
    probs = srt.softmax(-1)
    drop_sorted = (probs.cumsum(-1) - probs) >= top_p
    want = torch.empty_like(kept).scatter_(-1, idx, ~drop_sorted)
    assert torch.equal(kept, want)
    assert torch.allclose(m_gt, _brute_m_gt(l, torch.ones_like(kept)), rtol=0, atol=1e-14)
    assert bool(kept.gather(-1, l.argmax(-1, keepdim=True)).all())


@pytest.mark.parametrize("k", [1, 2, 5, 31, 32, 100])
def test_top_k_equals_the_topk_statement(k):
    l = _logits(2)
    kept, _ = F.kept_mask(l, top_k=k)
    want = ~(l < torch.topk(l, min(k, l.shape[1]), dim=-1).values[..., -1:])
    assert torch.equal(kept, want)
    assert torch.equal(kept.sum(-1), torch.full((l.shape[0],), min(k, l.shape[1])))


def test_top_k_one_keeps_exactly_the_row_maxima():
    l = _logits(3)
    l[0, 7] = l[0, 9] = l[0].max() + 1.0          # a row with two maxima keeps both
    kept, _ = F.kept_mask(l, top_k=1)
    assert torch.equal(kept, l == l.max(-1, keepdim=True).values)
    assert int(kept[0].sum()) == 2 and int(kept[1:].sum()) == l.shape[0] - 1


def test_a_tie_group_is_kept_or_dropped_whole():
    l = torch.round(_logits(4) * 4) / 4          # multiples of 0.25: plenty of ties
    assert any(len(set(r.tolist())) < l.shape[1] for r in l)
    for top_k, top_p in ((4, None), (None, 0.6), (8, 0.9), (None, 0.05)):
        kept, m_gt = F.kept_mask(l, top_k=top_k, top_p=top_p)
        for r in range(l.shape[0]):
            for v in set(l[r].tolist()):
                grp = l[r] == v
                assert bool(kept[r][grp].all()) or not bool(kept[r][grp].any()), (top_k, top_p, r, v)
                assert float(m_gt[r][grp].max() - m_gt[r][grp].min()) == 0.0
        assert bool(kept.gather(-1, l.argmax(-1, keepdim=True)).all())
        k_set = F.kept_mask(l, top_k=top_k)[0]
        assert torch.allclose(m_gt, _brute_m_gt(l, k_set), rtol=0, atol=1e-14)
        if top_k is not None:       # ties at the k-th value are all kept: never fewer than k codes before the nucleus
            assert int(k_set.sum(-1).min()) >= top_k and bool((k_set.sum(-1) > top_k).any())


def test_combined_takes_the_nucleus_over_the_renormalised_top_k_set():
    l = _logits(5)
    both, _ = F.kept_mask(l, top_k=8, top_p=0.9)
    k_set, _ = F.kept_mask(l, top_k=8)
    inner, _ = F.kept_mask(F.filtered_logits(l, k_set), top_p=0.9)
    assert torch.equal(both, inner & k_set)
    assert not torch.equal(both, k_set & F.kept_mask(l, top_p=0.9)[0])     # not the intersection of the two separate filters


def test_off_values():
    l = _logits(6)
    assert bool(F.kept_mask(l, top_k=32, top_p=1.0)[0].all()) and bool(F.kept_mask(l)[0].all())


@pytest.mark.parametrize("kw", [dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-3), dict(top_p=float("nan")), dict(top_k=2.5)])
def test_sample_step_refuses_bad_filter_arguments(kw):
    from muse import ops
    logits = torch.zeros(1, 2, 4)
    ids = torch.full((1, 2), 9)
    with pytest.raises(ValueError) as e:
        ops.sample_step(logits, ids, 9, 4, 1.0, 1, **kw)
    bad = next(iter(kw.values()))
    assert repr(bad) in str(e.value)
