"""Golden vectors of the `lion` optimizer choice from the REAL reference class (training/optimizer.py: Lion), importable only in the
build container:

    python tests/golden/make_golden_lion.py

Two parameter groups with different lr, betas and weight_decay (one with weight_decay = 0), tensors of 1, 8, 1003 and 4097 elements, six
steps on the CPU with seeded gradients, fresh each step.  Stored: the initial parameters, every step's gradients, parameters and exp_avg
after every step, and the layout of the class's state_dict() (state keys, group keys and values) as JSON.  Planted in the inputs:
  * PLANT_ZERO: elements whose gradient is 0 from step 1 on - exp_avg stays 0, so u == 0 and sign(u) == 0 on every step;
  * PLANT_MINUS_ZERO: p = -0.0 with g = 0 in the weight_decay = 0 group - p must keep the bits of -0.0;
  * PLANT_CANCEL: from step 2 on g is chosen so that exp_avg * beta1 and g * (1 - beta1) have opposite signs and magnitudes one or two
    ulp apart (or equal): the sign of u hangs on the roundings of the two products and of their sum.
Output: tests/golden/lion_steps.npz (committed; data the class wrote, none of its text).
"""
import importlib.util
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_OPTIMIZER = "/root/reference/training/optimizer.py"

SIZES = (1, 8, 1003, 4097)
GROUP_OF = (1, 0, 1, 0)                                  # tensor -> parameter group
GROUPS = (dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.1), dict(lr=3e-3, betas=(0.95, 0.98), weight_decay=0.0))
STEPS = 6
SEED = 20240
PLANT_ZERO = ((2, 5), (3, 7), (1, 3))                    # (tensor, element)
PLANT_MINUS_ZERO = ((2, 6),)
PLANT_CANCEL = ((3, 9), (3, 10), (3, 11), (2, 12), (2, 13), (1, 4))


def reference_lion():
    spec = importlib.util.spec_from_file_location("reference_training_optimizer", REFERENCE_OPTIMIZER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Lion


def main():
    Lion = reference_lion()
    gen = torch.Generator().manual_seed(SEED)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen) * 2.0 ** float(torch.randint(-3, 3, (1,), generator=gen))) for n in SIZES]
    with torch.no_grad():
        for t, i in PLANT_MINUS_ZERO:
            params[t][i] = -0.0
    opt = Lion([dict(params=[p for p, k in zip(params, GROUP_OF) if k == gi], **g) for gi, g in enumerate(GROUPS)])
    order = [p for grp in opt.param_groups for p in grp["params"]]          # the state_dict numbering
    out = {f"p0_{t}": p.detach().numpy().copy() for t, p in enumerate(params)}
    f32 = np.float32
    for step in range(1, STEPS + 1):
        for t, p in enumerate(params):
            p.grad = torch.randn(p.numel(), generator=gen) * 2.0 ** float(torch.randint(-8, 2, (1,), generator=gen))
        for t, i in PLANT_ZERO + PLANT_MINUS_ZERO:
            params[t].grad[i] = 0.0
        if step >= 2:
            for k, (t, i) in enumerate(PLANT_CANCEL):
                b1 = GROUPS[GROUP_OF[t]]["betas"][0]
                m = opt.state[params[t]]["exp_avg"][i].numpy().astype(f32)
                a = f32(m * f32(b1))                                         # round(m * b1)
                g = f32(-a / f32(1.0 - b1))
                for _ in range((k + step) % 3):                              # 0, 1 or 2 ulp away from the cancelling gradient
                    g = np.nextafter(g, f32(0) if (k + step) % 2 else f32(np.sign(g) * np.inf))
                params[t].grad[i] = float(g)
        for t, p in enumerate(params):
            out[f"g{step}_{t}"] = p.grad.numpy().copy()
        opt.step()
        for t, p in enumerate(params):
            out[f"p{step}_{t}"] = p.detach().numpy().copy()
            out[f"m{step}_{t}"] = opt.state[p]["exp_avg"].numpy().copy()
    sd = opt.state_dict()
    layout = dict(state_keys={str(i): sorted(st) for i, st in sd["state"].items()},
                  param_groups=[{k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in g.items()} for g in sd["param_groups"]],
                  order=[next(t for t, q in enumerate(params) if q is p) for p in order],
                  sizes=list(SIZES), group_of=list(GROUP_OF), steps=STEPS,
                  plant_zero=PLANT_ZERO, plant_minus_zero=PLANT_MINUS_ZERO, plant_cancel=PLANT_CANCEL)
    out["layout"] = np.array(json.dumps(layout))
    # the plants did what they are there for
    for t, i in PLANT_ZERO + PLANT_MINUS_ZERO:
        assert all(out[f"m{s}_{t}"][i] == 0 for s in range(1, STEPS + 1))
    for t, i in PLANT_MINUS_ZERO:
        assert all(out[f"p{s}_{t}"][i:i + 1].view(np.uint32)[0] == 0x80000000 for s in range(STEPS + 1)), "the -0.0 was lost"
    path = os.path.join(HERE, "lion_steps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
