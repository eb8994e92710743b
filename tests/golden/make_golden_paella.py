"""Golden vectors of the Paella VQ tokenizer from the REAL reference (muse/modeling_paella_vq.py), importable only in the build
container:

    python tests/golden/make_golden_paella.py

For each fixture of paella_weights.FIXTURES (batch 2): the encoder output before quantisation (`z`), `encode`'s indices and z_q,
`decode_code(indices)`, `decode(z_q)`, `get_code` of one non-square 24 x 40 image, and the state-dict name -> shape list as JSON.

Bit-exact index comparison needs a margin.  Over all tokens of a fixture (the batch and the non-square image) the generator takes
the reference's smallest relative gap between its best and second-best distance and searches seeds until
  * that gap is >= 1e-3 (ten times the 1e-4 latent tolerance the bf16x3 mode is held to), and
  * the reference run in float64 picks the same indices.
The achieved margin and the seed are written into the .npz.  Output: tests/golden/paella_tiny.npz, paella_tiny3.npz (committed).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the reference package on sys.path)
import paella_weights as PW  # noqa: E402

MIN_MARGIN = 1e-3
FIRST_SEED = {"paella_tiny": 1200, "paella_tiny3": 1300}


def _margin(model, z):
    """smallest relative gap (second - best) / best of the reference's own distances (compute_distances: torch.cdist) over the tokens"""
    d = model.vquantizer.compute_distances(z.permute(0, 2, 3, 1).contiguous())
    two = torch.topk(d, 2, dim=1, largest=False).values
    return float(((two[:, 1] - two[:, 0]) / two[:, 0]).min())


def _latent(model, x):
    return model.down_blocks(model.in_block(x))


def try_seed(name, cfg, side, seed):
    from muse.modeling_paella_vq import PaellaVQModel
    shapes = PW.paella_shapes(cfg)
    model = PaellaVQModel(**cfg)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    model.load_state_dict(PW.fill_paella(shapes, seed), strict=True)
    model.eval()
    px = PW.paella_images(PW.BATCH, side, side, seed + 1)
    px_ns = PW.paella_images(1, *PW.NONSQUARE, seed + 2)
    with torch.no_grad():
        z, z_ns = _latent(model, px), _latent(model, px_ns)
        margin = min(_margin(model, z), _margin(model, z_ns))
        if margin < MIN_MARGIN:
            return None, margin
        z_q, idx, loss = model.encode(px)
        assert loss is None
        code_ns = model.get_code(px_ns)
        m64 = PaellaVQModel(**cfg).double()
        m64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in model.state_dict().items()}, strict=True)
        m64.eval()
        if not (torch.equal(m64.get_code(px.double()), idx) and torch.equal(m64.get_code(px_ns.double()), code_ns)):
            return None, margin
        assert torch.equal(model.get_code(px), idx)
        rec, rec_decode = model.decode_code(idx), model.decode(z_q)
        assert torch.equal(model(px), rec_decode)
    out = dict(config=np.array(json.dumps(cfg)), seed=np.int64(seed), batch=np.int64(PW.BATCH), side=np.int64(side), margin=np.float64(margin),
               shapes=np.array(json.dumps({k: list(v) for k, v in shapes.items()})), z=MG.np_(z), indices=MG.np_(idx), z_q=MG.np_(z_q),
               rec=MG.np_(rec), rec_decode=MG.np_(rec_decode), code_nonsquare=MG.np_(code_ns))
    return out, margin


def main():
    torch.set_num_threads(1)
    for name, (cfg, side) in PW.FIXTURES.items():
        seed = FIRST_SEED[name]
        while True:
            out, margin = try_seed(name, cfg, side, seed)
            if out is not None:
                break
            seed += 1
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "seed", seed, "margin %.3e" % margin, "tokens", out["indices"].shape, path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
