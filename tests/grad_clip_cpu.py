"""CPU restatements of the gradient-norm / clipping entry points (csrc/gradnorm.hip, the muse_adamw_*_dev kernels) for the host-logic
tests of test_grad_clip.py and test_grad_clip_gloo.py: same arguments as the wrappers in muse.ops, same slab layout (one f64 partial
per parameter and 4096-element chunk, folded in chunk order, parameters in parameter order), same refusal of a range that cuts a
parameter.  The kernels themselves are tested on the GPU (test_gpu_grad_clip.py)."""
import torch

CHUNK = 4096


class Recorder:
    """install(ops) replaces the entry points; `norm_calls` / `adamw_calls` / `scale_calls` record what the host logic asked for"""

    def __init__(self, adamw_step):
        self.adamw_step = adamw_step        # oracle.maskgit_oracle.adamw_step
        self.norm_calls, self.adamw_calls, self.scale_calls, self.finalize_calls = [], [], [], 0

    def gradnorm_flat(self, g_flat, base, n, ptab_host, first_host, ptab, first, slab):
        from muse._hip import MuseHipError
        offs, sizes = ptab_host[:, 0].tolist(), ptab_host[:, 1].tolist()
        if base not in offs:
            raise MuseHipError("muse_gradnorm_flat failed with code -1 (bad argument)")
        t = offs.index(base)
        self.norm_calls.append((base, base + n))
        while t < len(offs) and offs[t] < base + n:
            if offs[t] + sizes[t] > base + n:
                raise MuseHipError("muse_gradnorm_flat failed with code -1 (bad argument)")
            x = g_flat[offs[t]:offs[t] + sizes[t]].double()
            for c in range((sizes[t] + CHUNK - 1) // CHUNK):
                slab[int(first_host[t]) + c] = (x[c * CHUNK:(c + 1) * CHUNK] ** 2).sum()
            t += 1

    def gradnorm_finalize(self, slab, first, nt, psum, grad_scale, max_norm, out):
        self.finalize_calls += 1
        f = first.tolist()
        total = torch.zeros((), dtype=torch.float64)
        for t in range(nt):
            s = torch.zeros((), dtype=torch.float64)
            for c in range(f[t], f[t + 1]):
                s = s + slab[c]
            psum[t] = s
            out[3 + t] = (grad_scale * s.sqrt()).float()
            total = total + s
        norm = (grad_scale * total.sqrt()).float()
        c = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
        coef = torch.where(c > 1, torch.ones_like(c), c)
        out[0], out[1], out[2] = norm, coef, torch.tensor(grad_scale, dtype=torch.float32) * coef

    def grad_scale_flat_(self, g, scale):
        self.scale_calls.append(g.numel())
        g.mul_(scale.reshape(()))

    def adamw_flat(self, p, g, m, v, p_bf16, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, scale_dev=None):
        assert p_bf16 is None
        self.adamw_calls.append((p.numel(), scale_dev is not None))
        gr = g * (scale_dev.reshape(()) if scale_dev is not None else grad_scale)     # (one f32 rounding, as the *_dev kernels)
        self.adamw_step(p, gr, m, v, int(step), lr, beta1, beta2, eps, weight_decay)

    def install(self, ops, setattr_=setattr):
        for name in ("gradnorm_flat", "gradnorm_finalize", "grad_scale_flat_", "adamw_flat"):
            setattr_(ops, name, getattr(self, name))
        return self
