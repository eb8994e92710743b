"""Tiny T5 encoders and a T5-style tokenizer built offline, shared by tests/test_t5_text_surface.py and tests/test_gpu_t5_text.py."""
import copy
import functools
import string

import torch

VOCAB, LAYERS, BATCH = 600, 3, 3
GEOMETRIES = [128, 96]        # d_model with 2 heads of d_kv 64: num_heads * d_kv == d_model and != d_model


@functools.lru_cache(maxsize=None)
def tower(d_model, seed=3):
    """-> (transformers T5EncoderModel on the CPU in f32, its f64 copy), shared and never modified.  Made to behave like a trained
    encoder: relative_attention_bias.weight ~ N(0, 2), every other non-embedding 2-D weight x 2, norm weights 1 + 0.2 N(0, 1) - the
    softmax is not flat and the bias moves the output by about max |x| (zeroing the table changes last_hidden_state by 1.0 .. 1.1 of
    max |x|), so a bias that is dropped, transposed or mis-signed cannot pass."""
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=VOCAB, d_model=d_model, d_kv=64, d_ff=320, num_layers=LAYERS, num_heads=2, feed_forward_proj="gated-gelu",
                   dropout_rate=0.0)
    m = T5EncoderModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "relative_attention_bias" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 2.0)
            elif p.dim() == 2 and "shared" not in name and "embed_tokens" not in name:
                p.mul_(2.0)
            elif p.dim() == 1:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
    return m, copy.deepcopy(m).double()


def make_ids(S, seed=0, batch=BATCH):
    return torch.randint(2, VOCAB, (batch, S), generator=torch.Generator().manual_seed(100 + S + seed))


def tokenizer(max_len=12):
    """a T5-style tokenizer without a download: a `tokenizers` Unigram model over a handful of pieces (metaspace pre-tokenizer, `</s>`
    = 1 appended, `<pad>` = 0: T5's conventions; 55 entries), wrapped as transformers' fast tokenizer.  AutoTokenizer reloads what its
    save_pretrained writes."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    pieces = [("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0), ("▁", -2.0)] + [(c, -3.0) for c in string.ascii_lowercase + string.digits + ".,!?'"]
    pieces += [("▁" + w, -1.0) for w in ("a", "the", "red", "fox", "two", "cats", "on", "sofa", "blue", "whale")]
    tk = Tokenizer(models.Unigram(pieces, unk_id=2, byte_fallback=False))
    tk.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
    tk.decoder = decoders.Metaspace(replacement="▁", prepend_scheme="always")
    tk.post_processor = processors.TemplateProcessing(single="$A </s>", special_tokens=[("</s>", 1)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, pad_token="<pad>", eos_token="</s>", unk_token="<unk>", model_max_length=max_len)


def pipeline_parts(seed=7):
    """(transformers T5EncoderModel with d_model 64, tokenizer, text-conditioned MaskGitTransformer config taking 64 text features)"""
    import weights as W
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=64, d_model=64, d_kv=64, d_ff=128, num_layers=2, num_heads=1, feed_forward_proj="gated-gelu", dropout_rate=0.0)
    return T5EncoderModel(cfg).eval(), tokenizer(), dict(W.TRANSFORMER_TEXT_TINY, encoder_hidden_size=64)
