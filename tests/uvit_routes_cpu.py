"""U-ViT model-level route cases (no GPU needed): the case table of tests/test_gpu_uvit_routes.py, the float64 reference of every case
(oracle/uvit_oracle.py on float64 weights and inputs), the distance the U-ViT parity tests use, six seeded routing defects and the bounds.

The kernels have exact per-element tests at every edge of their own dispatch; this suite owns what lies between them - which kernel
`TapeOps._attention` / `_attention_bwd_x3`, `ops.attention_x3_*`, `_attention_x3_fwd_blocks` / `_bwd_blocks` and `_norm_adaln` launch, on
which views, with which saved tensors.  A case exists for a ROUTE (the last column of CASES); the GPU test asserts that route ran.

Model: tests/golden/config_uvit_dropout.json with both dropouts 0 - hidden 128, channels 128, 2 heads of 64, 2 block heads, 2 layers, 1 res
block, encoder_hidden_size 64 - weights.fill_by_shapes(template, seed) unscaled, inputs weights.uvit_inputs.

Bounds (bounds(case, mode) -> (logits, loss, gradients), distances as in distance()):
    f32      M_F32 x the case's OWN float32-oracle-against-float64 gap (worst gradient tensor's figure for every gradient).  M_F32 = 8: GPU
             products add K in other orders and splits than the CPU's (profiles/uvit_routes.md: the MI355X reached 0.9 to 1.9 x the gap)
    bf16x3   (1e-3, 1e-4, 2e-3)   } TOL: the bar of test_uvit_config4_vs_reference_golden
    f16      (2e-3, 1e-4, 6e-3)   }
    bf16     min(TOL's (5e-2, 2e-3, 1.5e-1), 2 x the oracle's own torch.autocast(bfloat16) gap on the case): the CLIP / T5 towers' rule
    the loss figure of both gap rules is the largest loss gap over the case table, not the case's own (loss_gap: one scalar's gap is one draw)
tests/test_uvit_routes_cpu.py shows every f32 / bf16x3 / f16 bound at least 4 times below every seeded defect that applies to the case."""
import functools
import json
import os
from collections import namedtuple

import torch

TOL = {torch.float32: (1e-3, 1e-4, 2e-3), "bf16x3": (1e-3, 1e-4, 2e-3), "f16": (2e-3, 1e-4, 6e-3), torch.bfloat16: (5e-2, 2e-3, 1.5e-1)}
MODES = [torch.float32, "bf16x3", "f16", torch.bfloat16]
M_F32 = 8
SEED = 5200
THREADS = 8          # of the oracle runs

Case = namedtuple("Case", "name over side L B attrs route")


def _case(name, side, L, B, over=(), attrs=(), route=""):
    return Case(name, tuple(sorted(dict(over).items())), side, L, B, tuple(attrs), route)


_H4 = dict(num_attention_heads=4, block_num_heads=4)
_W64 = dict(hidden_size=64, block_out_channels=(64,), num_attention_heads=1, block_num_heads=1, intermediate_size=64)
_C96 = dict(block_out_channels=(96,), block_num_heads=2, hidden_size=128)
_LN = dict(norm_type="layernorm", ln_elementwise_affine=True)
_NOAFF = dict(norm_type="rmsnorm", ln_elementwise_affine=False)
_DOWN = dict(force_down_up_sample=True)

CASES = [
    _case("s16_L77_B2", 16, 77, 2, route="one-tile self + one-tile cross; planes-only gradients (the base route)"),
    _case("s32_L77_B1", 32, 77, 1, route="streamed 1024 x 1024 self; cross 1024 x 77 one query block at a time"),
    _case("s32_L77_B2", 32, 77, 2, route="the same with the batch strides of the block descriptors"),
    _case("s32_L77_B1_pairs", 32, 77, 1, attrs=(("X3_STREAM", False),),
          route="X3_STREAM off: block pairs + log-sum-exp merge, muse_sum_parts_strided in the backward"),
    _case("s16_L512_B2", 16, 512, 2, route="T5's padded length: cross-attention streamed, 1 query block"),
    _case("s32_L512_B1", 32, 512, 1, route="cross-attention streamed, 4 query blocks"),
    _case("s16_L256_B2", 16, 256, 2, route="Skv = 256: one key tile, not blocked"),
    _case("s32_L256_B1", 32, 256, 1, route="Skv = 256: blocked by queries only"),
    _case("s16_L64", 16, 64, 2, route="_x3_one_tile_keys edge: cross materialised beside a fused self"),
    _case("s16_L96", 16, 96, 2, route="_x3_one_tile_keys edge: cross fused (96 keys)"),
    _case("s16_L97", 16, 97, 2, route="_x3_one_tile_keys edge: cross materialised"),
    _case("s16_L224", 16, 224, 2, route="_x3_one_tile_keys edge: cross materialised"),
    _case("s16_L225", 16, 225, 2, route="_x3_one_tile_keys edge: cross fused (225 keys)"),
    _case("s16_L1", 16, 1, 2, route="one text state: cross materialised"),
    _case("s15_L77_B1", 15, 77, 1, route="225 tokens: two-kernel norm + AdaLN, materialised core in x3 / f16, rows % 8 != 0"),
    _case("s17_L77_B3", 17, 77, 3, route="289 tokens x 3: the same, more than 256 rows per image"),
    _case("s8_L77_B2", 8, 77, 2, route="64 tokens: below every fused gate of the x3 / f16 modes"),
    _case("h4_s16", 16, 77, 2, over=_H4, route="head dim 32: bf16 fused, bf16x3 / f16 materialised"),
    _case("h1_w64_s16", 16, 77, 2, over=_W64, route="every min(w.shape) >= 128 / go gate false: f32 gradients + planes"),
    _case("h1_w64_s32_B1", 32, 77, 1, over=_W64, route="the same gates false on the streamed route: f32 gradients + planes out of the stream kernels"),
    _case("c96_s16", 16, 77, 2, over=_C96, route="C != H (senc, kv_mapper); block attention (head dim 48) off the x3 route"),
    _case("ln_s16", 16, 77, 2, over=_LN, route="norm_type layernorm on the fused routes"),
    _case("noaffine_s16", 16, 77, 2, over=_NOAFF, route="norms without gains on the fused routes"),
    _case("down_s32", 32, 77, 2, over=_DOWN, route="down / up sampling around 256 inner tokens"),
    _case("down_s64", 64, 77, 1, over=_DOWN, route="down / up sampling around 1024 inner tokens: streamed"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

DEFECTS = ["last_key_block_dropped", "key_blocks_rolled_for_query_block_1", "heads_rolled", "text_of_next_image", "text_keys_past_64_dropped",
           "query_blocks_0_1_swapped"]


def config(case):
    """the model configuration of a case: the narrow dropout configuration with both dropouts 0, plus the case's overrides"""
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = json.load(open(os.path.join(here, "golden", "config_uvit_dropout.json")))
    cfg.update(hidden_dropout=0.0, attention_dropout=0.0)
    cfg.update(norm_type="rmsnorm", layer_norm_eps=1e-6, ln_elementwise_affine=True, use_bias=False, force_down_up_sample=False)   # the defaults, spelled out
    cfg.update(dict(case.over))
    return cfg


def inner_tokens(case):
    """the sequence length the blocks and the transformer layers see"""
    return case.side * case.side // (4 if dict(case.over).get("force_down_up_sample") else 1)


def _key(case):
    return (case.over, case.side, case.L, case.B)


@functools.lru_cache(maxsize=None)
def _weights(over):
    import muse
    import weights as W
    cfg = config(_case("", 0, 0, 0, over=over))
    model = muse.MaskGiTUViT(**cfg)
    return W.fill_by_shapes({k: tuple(v.shape) for k, v in model.state_dict().items()}, SEED)


def state_dict(case):
    """seeded f32 weights in the reference's names (a fresh dict of the shared, never modified tensors)"""
    return dict(_weights(case.over))


@functools.lru_cache(maxsize=None)
def _inputs(key):
    import weights as W
    over, side, L, B = key
    cfg = config(_case("", 0, 0, 0, over=over))
    return W.uvit_inputs(B, side * side, L, SEED + 1, cfg["vocab_size"], cfg["codebook_size"], cfg["encoder_hidden_size"], cfg["cond_embed_dim"])


def inputs(case):
    """(input_ids, encoder_hidden_states, cond_embeds, micro_conds, labels) on the CPU"""
    return _inputs(_key(case))


def _oracle(key, dtype, autocast=False):
    from oracle import uvit_oracle as O
    over, side, L, B = key
    case = _case("", side, L, B, over=over)
    sd = {k: v.to(dtype) for k, v in state_dict(case).items()}
    ids, enc, cond, micro, labels = inputs(case)
    # a fixed thread count: the float32 and autocast runs' own gaps (the bounds) depend on how torch splits its CPU reductions, and other
    # test modules leave the process at one thread
    threads = torch.get_num_threads()
    torch.set_num_threads(min(THREADS, os.cpu_count()))
    try:
        with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
            logits, loss, grads = O.uvit_loss_and_grads(sd, config(case), ids, enc.to(dtype), cond.to(dtype), micro.to(dtype), labels)
    finally:
        torch.set_num_threads(threads)
    return logits.double(), float(loss), {k: g.double() for k, g in grads.items()}


@functools.lru_cache(maxsize=None)
def _reference(key):
    return _oracle(key, torch.float64)


@functools.lru_cache(maxsize=None)
def _reference_f32(key):
    return _oracle(key, torch.float32)


@functools.lru_cache(maxsize=None)
def _reference_autocast(key):
    return _oracle(key, torch.float32, autocast=True)


def reference(case):
    """(logits, loss, {name: gradient}) of the float64 oracle - shared by every test of the case, never modified"""
    return _reference(_key(case))


def reference_f32(case):
    return _reference_f32(_key(case))


def reference_autocast(case):
    return _reference_autocast(_key(case))


def distance(got, ref):
    """(logits: max|d| / max|ref|, loss: relative, {name: max|d| / max|ref tensor|}) - test_uvit_config4_vs_reference_golden's measure"""
    (gl, gs, gg), (rl, rs, rg) = got, ref
    assert tuple(gl.shape) == tuple(rl.shape) and set(gg) == set(rg), (gl.shape, rl.shape, set(gg) ^ set(rg))
    el = float((gl.double().cpu() - rl).abs().max() / rl.abs().max())
    es = abs(float(gs) - float(rs)) / abs(float(rs))
    scale = {k: float(r.abs().max()) for k, r in rg.items()}
    nonzero = {k: v for k, v in scale.items() if v > 0.0}
    for k in set(scale) - set(nonzero):
        # a tensor whose exact gradient is identically zero (one text state: the softmax over a single key is constant, so nothing reaches
        # the queries and keys of that attention, nor the norm and AdaLN that feed its queries alone) is measured against the largest
        # gradient of the smallest enclosing module that has one
        parts = k.split(".")
        for n in range(len(parts) - 2, -1, -1):
            inside = [v for j, v in nonzero.items() if j.startswith(".".join(parts[:n]) + "." if n else "")]
            if inside:
                scale[k] = max(inside)
                break
    eg = {k: float((gg[k].double().cpu().reshape(rg[k].shape) - rg[k]).abs().max()) / scale[k] for k in rg}
    return el, es, eg


def zero_gradients(case):
    """names of the parameters whose exact gradient is identically zero on the case"""
    return sorted(k for k, g in reference(case)[2].items() if float(g.abs().max()) == 0.0)


def worst(eg):
    k = max(eg, key=eg.get)
    return k, eg[k]


def applies(case, defect):
    cfg, S = config(case), inner_tokens(case)
    return {"last_key_block_dropped": S >= 512, "key_blocks_rolled_for_query_block_1": S >= 512, "query_blocks_0_1_swapped": S >= 512,
            "heads_rolled": cfg["num_attention_heads"] >= 2 or cfg["block_num_heads"] >= 2, "text_of_next_image": case.B >= 2,
            "text_keys_past_64_dropped": case.L > 64}[defect]


def _defective_attention(defect):
    """oracle.uvit_oracle.attention with one routing defect of the block-by-block host code seeded into it"""
    def attention(x, context, sd, prefix, num_heads):
        from oracle.uvit_oracle import linear
        self_attn = context is x
        B, Sq, H = x.shape
        if defect == "text_of_next_image" and not self_attn and B >= 2:            # a wrong batch stride / base of the k | v views
            context = context.roll(-1, 0)
        if defect == "text_keys_past_64_dropped" and not self_attn and context.shape[1] > 64:     # seq_kv of the one-tile descriptor
            context = context[:, :64]
        Skv = context.shape[1]
        hd = H // num_heads
        q = linear(x, sd, prefix + "query.").view(B, Sq, num_heads, hd).transpose(1, 2)
        k = linear(context, sd, prefix + "key.").view(B, Skv, num_heads, hd).transpose(1, 2)
        v = linear(context, sd, prefix + "value.").view(B, Skv, num_heads, hd).transpose(1, 2)
        alpha = 1.0 / float(torch.sqrt(torch.tensor(hd, dtype=torch.float32)))
        scores = torch.matmul(q, k.transpose(-1, -2)) * alpha
        if defect == "last_key_block_dropped" and self_attn and Skv >= 512:         # nk one short: the merge / the stream ends early
            scores = scores[..., :Skv - 256]
            v = v[:, :, :Skv - 256]
        probs = torch.softmax(scores, dim=-1)
        ctx = torch.matmul(probs, v)
        if defect == "key_blocks_rolled_for_query_block_1" and Sq >= 512 and Skv >= 512:      # k and v block pointers one block apart
            ctx = torch.cat([ctx[:, :, :256], torch.matmul(probs[:, :, 256:512], v.roll(256, 2)), ctx[:, :, 512:]], dim=2)
        if defect == "heads_rolled" and num_heads >= 2:                              # head h's context in head h + 1's columns
            ctx = ctx.roll(1, 1)
        if defect == "query_blocks_0_1_swapped" and Sq >= 512:                       # d.o += qi * 256 * ldo with the wrong qi
            ctx = torch.cat([ctx[:, :, 256:512], ctx[:, :, :256], ctx[:, :, 512:]], dim=2)
        return linear(ctx.transpose(1, 2).reshape(B, Sq, H), sd, prefix + "out.")
    return attention


def defective(case, defect):
    """the float64 oracle with uvit_oracle.attention replaced by the defective one for the duration of the call"""
    from oracle import uvit_oracle as O
    assert defect in DEFECTS and applies(case, defect), (case.name, defect)
    real = O.attention
    O.attention = _defective_attention(defect)
    try:
        return _oracle(_key(case), torch.float64)
    finally:
        O.attention = real


@functools.lru_cache(maxsize=None)
def own_gap(key, autocast):
    """the oracle's own float32 (or float32 under torch.autocast(bfloat16)) run against its float64 run: (logits, loss, worst gradient)"""
    el, es, eg = distance((_reference_autocast if autocast else _reference_f32)(key), _reference(key))
    return el, es, worst(eg)[1]


@functools.lru_cache(maxsize=None)
def loss_gap(autocast):
    """the largest loss gap of own_gap over the case table.  The logits and gradient figures are maxima over thousands of elements and
    move by less than 2 x from case to case; the loss is ONE number, and its gap on one case is one draw of a rounding error - measured
    8e-9 to 1.8e-7 in float32 (below float32's unit roundoff of 6e-8 on four cases: no f32 result can be held to a multiple of that) and
    7.7e-7 to 4.7e-4 under autocast beside logits gaps of 1.0e-2 to 2.0e-2.  The scale of that error is what the draws reach together."""
    return max(own_gap(_key(c), autocast)[1] for c in CASES)


def bounds(case, mode):
    """-> (logits, loss, gradients), see the module docstring"""
    if mode == torch.float32:
        el, _, eg = own_gap(_key(case), False)
        return M_F32 * el, M_F32 * loss_gap(False), M_F32 * eg
    if mode == torch.bfloat16:
        el, _, eg = own_gap(_key(case), True)
        return tuple(min(t, 2.0 * e) for t, e in zip(TOL[mode], (el, loss_gap(True), eg)))
    return TOL[mode]
