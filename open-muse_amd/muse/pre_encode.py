"""Pre-encoded token shards — SURVEY.md section 8(f) row 4: take the VQ tokenizer out of the train step.

The reference's text-to-image configs never run the VQGAN inside the loop: scripts/pre_encode.py:440-511 encodes every image once
(`vae.get_code(image)`) and writes webdataset shards whose samples carry `<key>.<vae checkpoint>.pth` (the token ids) and
`<key>.<text encoder checkpoint>.pth` (the text states) next to a `<key>.json`; training/data.py:561-573 reads them back as
`image_input_ids` / `encoder_hidden_states` (the TODO at training/train_maskgit_imagenet.py:404 asks for the same for ImageNet).

This module produces and consumes that layout with the tokenizer on the HIP kernels (`MaskGitVQGAN.get_code`) and plain `tarfile`
(webdataset itself is not needed to write or read a POSIX tar of `<key>.<ext>` members): shards written here are readable by the
reference's pipeline and vice versa (member extensions are matched case-insensitively, as webdataset does).  `muse.TrainStep(...)(pixel_values=None, class_ids, image_tokens=tokens)` is the step that
consumes the tokens.

The image stage in front of `get_code` (scripts/pre_encode.py:449-489: per image to(cuda), permute, div(255), antialiased bilinear
TF.resize, TF.center_crop, then stack) is `resize_center_crop`: a ragged batch of decoded uint8 images -> `pixel_values` in one host-to-
device copy and one launch (csrc/resize.hip).  `image_batches` feeds `pre_encode` with it; `random_crop_offsets` draws the windows of
training/data.py:136-145.
"""
from __future__ import annotations

import io
import json
import os
import tarfile
from typing import Dict, Iterable, Iterator, Optional, Sequence

import torch

from . import _hip


def checkpoint_ext(checkpoint: str) -> str:
    """member extension of a checkpoint name: scripts/pre_encode.py:54-56 joins the path parts with '.', training/data.py:562-563
    lower-cases it and replaces '/' by '.' before matching"""
    return checkpoint.lower().replace("/", ".") + ".pth"


def _add(tar: tarfile.TarFile, name: str, payload: bytes):
    info = tarfile.TarInfo(name)
    info.size = len(payload)
    tar.addfile(info, io.BytesIO(payload))


def _pth(t: torch.Tensor) -> bytes:
    buf = io.BytesIO()
    torch.save(t.detach().cpu().clone(), buf)      # what webdataset's `pth` handler (torch_dumps) writes
    return buf.getvalue()


def write_token_shard(path: str, keys: Sequence[str], image_tokens: torch.Tensor, vae_checkpoint: str,
                      encoder_hidden_states: Optional[torch.Tensor] = None, text_encoder_checkpoint: Optional[str] = None,
                      metadata: Optional[Sequence[dict]] = None) -> None:
    """one tar shard: per sample `<key>.<vae>.pth` = int64 [num_vq_tokens] (+ `<key>.<text encoder>.pth`, `<key>.json`)"""
    if len(keys) != image_tokens.shape[0]:
        raise ValueError("one key per row of image_tokens")
    with tarfile.open(path, "w") as tar:
        for i, key in enumerate(keys):
            _add(tar, f"{key}.{checkpoint_ext(vae_checkpoint)}", _pth(image_tokens[i].to(torch.int64)))
            if encoder_hidden_states is not None:
                _add(tar, f"{key}.{checkpoint_ext(text_encoder_checkpoint)}", _pth(encoder_hidden_states[i]))
            _add(tar, f"{key}.json", json.dumps(dict(metadata[i]) if metadata is not None else {}).encode())


def read_token_shard(path: str, vae_checkpoint: str, text_encoder_checkpoint: Optional[str] = None) -> Iterator[Dict[str, object]]:
    """samples of a shard as training/data.py:561-573 presents them: {"__key__", "image_input_ids"[, "encoder_hidden_states"]}"""
    want = {checkpoint_ext(vae_checkpoint): "image_input_ids"}
    if text_encoder_checkpoint is not None:
        want[checkpoint_ext(text_encoder_checkpoint)] = "encoder_hidden_states"
    cur_key, cur = None, {}
    with tarfile.open(path, "r") as tar:
        for m in tar:
            if not m.isfile():
                continue
            # webdataset (base_plus_ext): the key is the directory part plus everything before the first dot of the BASE name, and
            # the extension is lower-cased on read - the reference writes mixed-case members (`<key>.openMUSE.vqgan-....pth`)
            dirname, base = os.path.split(m.name)
            stem, _, ext = base.partition(".")
            key, ext = (os.path.join(dirname, stem) if dirname else stem), ext.lower()
            if key != cur_key:
                if cur_key is not None and "image_input_ids" in cur:
                    yield cur
                cur_key, cur = key, {"__key__": key}
            if ext in want:
                cur[want[ext]] = torch.load(io.BytesIO(tar.extractfile(m).read()), map_location="cpu")
    if cur_key is not None and "image_input_ids" in cur:
        yield cur


@torch.no_grad()
def pre_encode(vq_model, batches: Iterable, shard_pattern: str, vae_checkpoint: str, samples_per_shard: int = 10000) -> int:
    """encode batches of (keys, pixel_values [B,3,H,W] in [0,1] on the GPU) with `vq_model.get_code` (scripts/pre_encode.py:497-498)
    and write them as shards `shard_pattern % n`; returns the number of samples written"""
    n_written, shard, keys, toks = 0, 0, [], []

    def flush():
        nonlocal shard, keys, toks
        if keys:
            write_token_shard(shard_pattern % shard, keys, torch.cat(toks), vae_checkpoint)
            shard, keys, toks = shard + 1, [], []
    for bkeys, pixel_values in batches:
        codes = vq_model.get_code(pixel_values).cpu()
        keys += list(bkeys)
        toks.append(codes)
        n_written += len(bkeys)
        if len(keys) >= samples_per_shard:
            flush()
    flush()
    return n_written


def token_batches(shards: Sequence[str], vae_checkpoint: str, batch_size: int, device="cuda") -> Iterator[torch.Tensor]:
    """[batch_size, num_vq_tokens] int64 batches on `device` from pre-encoded shards (drops the ragged tail like the reference's
    `.batched(batch_size, partial=False)`)"""
    buf = []
    for path in shards:
        for s in read_token_shard(path, vae_checkpoint):
            buf.append(s["image_input_ids"].reshape(-1))
            if len(buf) == batch_size:
                yield torch.stack(buf).to(device, non_blocking=True)
                buf = []


# ---- the image stage in front of get_code (scripts/pre_encode.py:449-489) on the GPU, one copy + one launch per batch ----------------
def _resized_size(H: int, W: int, R: int):
    """torchvision's _compute_resized_output_size for an int size: the shorter side becomes R, the longer int(R * long / short)"""
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def _center_offsets(oh: int, ow: int, R: int):
    """torchvision's center_crop: Python's round (half to even) of half the excess"""
    return int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))


def _as_u8_hwc(i: int, image):
    """image -> uint8 [H, W, 3] torch tensor (CPU or GPU, any strides); ValueError naming what arrived otherwise"""
    if isinstance(image, torch.Tensor):
        t = image
    elif hasattr(image, "mode") and hasattr(image, "getbands"):            # a PIL image
        if image.mode != "RGB":
            raise ValueError(f"resize_center_crop: image {i} is a PIL image of mode {image.mode!r}; only 'RGB' is taken (convert it first)")
        import numpy as np
        t = torch.from_numpy(np.array(image, dtype=np.uint8))
    elif hasattr(image, "__array_interface__"):
        import numpy as np
        a = np.asarray(image)
        if a.dtype != np.uint8:
            raise ValueError(f"resize_center_crop: image {i} has dtype {a.dtype}; uint8 is required")
        t = torch.from_numpy(a if a.flags.writeable else a.copy())
    else:
        raise ValueError(f"resize_center_crop: image {i} is a {type(image).__name__}; a uint8 [H, W, 3] tensor, numpy array or RGB PIL image is required")
    if t.dtype != torch.uint8:
        raise ValueError(f"resize_center_crop: image {i} has dtype {t.dtype}; uint8 is required")
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"resize_center_crop: image {i} has shape {tuple(t.shape)}; [H, W, 3] (RGB, channels last) is required")
    return t


_staging = {"buf": None, "event": None}      # the pinned host buffer of the last call and the event behind its copy


def _pinned(nbytes: int) -> torch.Tensor:
    """a pinned uint8 buffer of at least nbytes, reused between calls (pinning is the expensive part); the previous call's copy out of
    it is waited for before it is overwritten"""
    if _staging["event"] is not None:
        _staging["event"].synchronize()
        _staging["event"] = None
    if _staging["buf"] is None or _staging["buf"].numel() < nbytes:
        _staging["buf"] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    return _staging["buf"]


@torch.no_grad()
def resize_center_crop(images: Sequence, resolution: int, *, crop_offsets=None, flip=None, return_meta: bool = False):
    """A ragged batch of uint8 [H, W, 3] images -> pixel_values [B, 3, R, R] f32 in [0, 1] on the GPU, as scripts/pre_encode.py:449-489
    computes them per image (permute, div(255), TF.resize(size=R, BILINEAR, antialias=True), TF.center_crop, stack), in ONE host-to-
    device copy and ONE kernel launch (ops.resize_crop_u8).

    images: torch tensors on the CPU or the GPU, numpy arrays, or PIL images of mode RGB.  CPU images and the size table are packed
    into one pinned buffer and cross in one copy; GPU images are concatenated behind it on the device.
    crop_offsets [B, 2] (top, left in the RESIZED image, e.g. from random_crop_offsets) replaces the centred window; flip [B] mirrors
    the cropped window horizontally (crop first, then flip: training/data.py:119-125).
    return_meta=True -> (pixel_values, orig_size [B, 2] = (width, height) as training/data.py:96-97 orders it, crop_coords [B, 2] =
    (top, left) as training/data.py:140-144), both int64 on the CPU."""
    from . import ops
    R = int(resolution)
    if R < 1:
        raise ValueError(f"resize_center_crop: resolution is at least 1, got {resolution}")
    imgs = [_as_u8_hwc(i, im) for i, im in enumerate(images)]
    B = len(imgs)
    if B == 0:
        raise ValueError("resize_center_crop: no images")
    if crop_offsets is not None:
        crop_offsets = torch.as_tensor(crop_offsets).cpu().to(torch.int64)
        if tuple(crop_offsets.shape) != (B, 2):
            raise ValueError(f"resize_center_crop: crop_offsets has shape {tuple(crop_offsets.shape)}; [{B}, 2] is required")
        crop_offsets = crop_offsets.tolist()
    if flip is not None:
        flip = torch.as_tensor(flip).cpu().reshape(-1).to(torch.bool).tolist()
        if len(flip) != B:
            raise ValueError(f"resize_center_crop: flip has {len(flip)} entries for {B} images")
    rows = []
    for b, t in enumerate(imgs):
        H, W = int(t.shape[0]), int(t.shape[1])
        oh, ow = _resized_size(H, W, R)
        if crop_offsets is None:
            top, left = _center_offsets(oh, ow, R)
        else:
            top, left = crop_offsets[b]
            if not (0 <= top <= oh - R and 0 <= left <= ow - R):
                raise ValueError(f"resize_center_crop: crop_offsets[{b}] = ({top}, {left}) outside [0, {oh - R}] x [0, {ow - R}] "
                                 f"(image {H} x {W} resized to {oh} x {ow})")
        rows.append([0, H, W, oh, ow, top, left, int(bool(flip[b])) if flip is not None else 0])
    # layout of the device buffer: [table 64 B bytes][CPU images, back to back][GPU images, back to back]
    off = 64 * B
    for on_gpu in (False, True):
        for b, t in enumerate(imgs):
            if t.is_cuda == on_gpu:
                rows[b][0] = off
                off += 3 * rows[b][1] * rows[b][2]
    n_host = 64 * B + sum(3 * r[1] * r[2] for r, t in zip(rows, imgs) if not t.is_cuda)
    table = torch.tensor(rows, dtype=torch.int64)
    gpu_imgs = [t for t in imgs if t.is_cuda]
    if not torch.cuda.is_available():
        raise _hip.MuseHipError("resize_center_crop: the resize runs on the GPU; there is no CPU compute path")
    device = gpu_imgs[0].device if gpu_imgs else torch.device("cuda")
    host = _pinned(n_host)[:n_host]
    host[:64 * B].view(torch.int64).view(B, 8).copy_(table)
    for r, t in zip(rows, imgs):
        if not t.is_cuda:
            host[r[0]:r[0] + 3 * r[1] * r[2]].view(r[1], r[2], 3).copy_(t)
    packed = host.to(device, non_blocking=True)
    _staging["event"] = torch.cuda.Event()
    _staging["event"].record()
    if gpu_imgs:
        packed = torch.cat([packed] + [t.reshape(-1) for t in gpu_imgs])
    px = ops.resize_crop_u8(packed, packed[:64 * B].view(torch.int64).view(B, 8), B, R, host_table=table)
    if not return_meta:
        return px
    return px, torch.tensor([[r[2], r[1]] for r in rows], dtype=torch.int64), torch.tensor([[r[5], r[6]] for r in rows], dtype=torch.int64)


def random_crop_offsets(sizes, resolution: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """torchvision's RandomCrop.get_params for every image of `sizes` [B, 2] = (H, W) of the ORIGINAL images, applied to their resized
    sizes: per image i = randint(0, oh - R + 1) then j = randint(0, ow - R + 1), one torch.randint(.., (1,)) each on the host, and no
    draw at all when the resized image is already R x R.  -> int64 [B, 2] (top, left) for resize_center_crop(crop_offsets=)."""
    R = int(resolution)
    out = []
    for H, W in torch.as_tensor(sizes).reshape(-1, 2).tolist():
        oh, ow = _resized_size(int(H), int(W), R)
        if oh == R and ow == R:
            out.append([0, 0])
            continue
        i = int(torch.randint(0, oh - R + 1, (1,), generator=generator))
        j = int(torch.randint(0, ow - R + 1, (1,), generator=generator))
        out.append([i, j])
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 2)


def image_batches(samples: Iterable, resolution: int, batch_size: int, drop_last: bool = False) -> Iterator:
    """(key, image) pairs -> (keys, pixel_values [b, 3, R, R]) batches through resize_center_crop: what pre_encode(vq_model, batches, ..)
    consumes, so images -> token shards is pre_encode(vq, image_batches(samples, R, bs), pattern, checkpoint)"""
    keys, imgs = [], []
    for key, image in samples:
        keys.append(key)
        imgs.append(image)
        if len(keys) == batch_size:
            yield keys, resize_center_crop(imgs, resolution)
            keys, imgs = [], []
    if keys and not drop_last:
        yield keys, resize_center_crop(imgs, resolution)
