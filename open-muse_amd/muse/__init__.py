"""muse — MI355X-native drop-in for the hot path of huggingface/open-muse.

Same import surface as the reference package for the classes on the path (reference muse/__init__.py:18-25):
MaskGitTransformer, MaskGiTUViT, MaskGitVQGAN, VQGANModel (the taming tokenizer of the text-to-image configs),
PipelineMuse, PipelineMuseInpainting, EMAModel (the weight average train_muse.py advances behind every optimizer step), get_mask_chedule; plus
CLIPTextEncoder and T5TextEncoder, the CLIP text tower and the T5 v1.1 encoder of the text-to-image configs on the same kernels (opt-in), and CLIPImageEncoder / CLIPScorer / clip_scores, the CLIP image tower and the
CLIP score of generated images (opt-in), and FeatureStats / frechet_distance, the Frechet distance on CLIP image embeds that closes the
reference's sample -> score loop (opt-in; not comparable with Inception FID numbers, muse/frechet.py), and FeatureBank / mmd_distance /
cmmd_distance, the maximum mean discrepancy on the same embeds (CMMD, muse/mmd.py); everything computes
through libmuse_hip.so (hand-written HIP kernels for gfx950).
The Paella and MoVQ tokenizers are built on the same kernels under the reference's module paths, `muse.modeling_paella_vq.PaellaVQModel` and
`muse.modeling_movq.MOVQ` (bind them from there); the top-level names `muse.MOVQ` / `muse.PaellaVQModel` are still the stubs of
muse/unbuilt.py: they import (the training scripts import them unconditionally) and refuse to construct, saying where the built class lives.
`muse.lr_schedulers` / `muse.training_utils` carry the host-side helpers those scripts import.
"""
__version__ = "0.0.1"

from .ema import EMAModel
from .frechet import FeatureStats, frechet_distance
from .mmd import FeatureBank, cmmd_distance, mmd_distance
from .modeling_clip_text import CLIPTextEncoder
from .modeling_clip_vision import CLIPImageEncoder, CLIPScorer, clip_scores
from .modeling_maskgit_vqgan import MaskGitVQGAN
from .modeling_t5_text import T5TextEncoder
from .modeling_taming_vqgan import VQGANModel
from .modeling_transformer import MaskGitTransformer
from .modeling_transformer_v2 import MaskGiTUViT, MaskGiTUViT_v2
from . import pre_encode
from .pipeline_muse import PipelineMuse, PipelineMuseInpainting
from .sampling import get_mask_chedule
from .unbuilt import MOVQ, PaellaVQModel
from . import lr_schedulers, training_utils
from .training import (FusedAdamW, FusedLion, GradReducer, TrainStep, clip_grad_norm_, cond_dropout, grad_norms, grouped_parameters,
                       mask_or_random_replace_tokens, prepare_inputs_and_labels)

__all__ = ["MOVQ", "PaellaVQModel", "EMAModel", "CLIPTextEncoder", "CLIPImageEncoder", "CLIPScorer", "clip_scores", "FeatureStats", "frechet_distance", "FeatureBank", "mmd_distance", "cmmd_distance", "T5TextEncoder", "MaskGitVQGAN", "VQGANModel", "MaskGitTransformer", "MaskGiTUViT", "MaskGiTUViT_v2", "PipelineMuse", "PipelineMuseInpainting", "get_mask_chedule", "FusedAdamW", "FusedLion", "GradReducer", "clip_grad_norm_", "grad_norms",
           "TrainStep", "prepare_inputs_and_labels", "mask_or_random_replace_tokens", "cond_dropout", "grouped_parameters"]
