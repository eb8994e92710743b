"""Top-level names the reference's training scripts import from `muse` that this module answers with refusing stubs: `MOVQ` and
`PaellaVQModel`.  The scripts import both unconditionally (training/train_muse.py:51-60, training/train_maskgit_imagenet.py:38) and pick
one by the config's `model.vq_model.type`.  Every tokenizer of the reference is built on the HIP kernels: `maskgit_vqgan`
(muse.MaskGitVQGAN), `vqgan` (muse.VQGANModel), `paella_vq` (muse.modeling_paella_vq.PaellaVQModel) and `movq`
(muse.modeling_movq.MOVQ).  The last two are bound from their modules while the top-level names here stay the stubs:
importing them works; building one says where the built class lives instead of computing something else."""
from __future__ import annotations

from ._hip import MuseHipError


class _NotBuilt:
    _what = "this model"
    _built = "none"

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"muse.{type(self).__name__} ({self._what}) is not part of the MI355X hot-path build under this name: "
                                  f"the class built on the HIP kernels is {self._built} (bind it from there, INTEGRATION.md); the other "
                                  "tokenizers are muse.MaskGitVQGAN (`maskgit_vqgan`) and muse.VQGANModel (`vqgan`)")

    @classmethod
    def from_pretrained(cls, *args, **kwargs):
        cls()

    @classmethod
    def from_config(cls, *args, **kwargs):
        cls()


class MOVQ(_NotBuilt):
    _what = "the MoVQ tokenizer, reference muse/modeling_movq.py"
    _built = "muse.modeling_movq.MOVQ"


class PaellaVQModel(_NotBuilt):
    _what = "the Paella VQ tokenizer, reference muse/modeling_paella_vq.py"
    _built = "muse.modeling_paella_vq.PaellaVQModel"


__all__ = ["MOVQ", "PaellaVQModel", "MuseHipError"]
