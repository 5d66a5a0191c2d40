"""References for the Adam kernels (csrc/mmad_ops_adam.hip): the update of
include/mmad.h (mmad_adam) as a plain float64 formula, and torch.optim.Adam's
CPU single-tensor step from a given state.  tests/test_adam_reference.py pins
the two against each other in float64, so the GPU tests compare the kernels
with a reference that is itself checked on a machine without a GPU."""
import math

import torch


def adam_consts(lr, betas, step):
    """(step_size, bc2_sqrt) = (lr / (1 - b1^t), sqrt(1 - b2^t)), formed in
    double: the two scalars mmad_adam takes."""
    b1, b2 = betas
    return lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)


def adam_step_f64(p, g, m, v, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, step=1):
    """One Adam step (amsgrad=False, weight_decay=0) in float64 from the state
    (p, m, v) after step - 1 steps: m = lerp(m, g, 1 - b1), v = v b2 +
    (1 - b2) g g, p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps).
    Returns new (p, m, v), float64; the arguments are left alone."""
    b1, b2 = betas
    step_size, bc2_sqrt = adam_consts(lr, betas, step)
    p, g, m, v = (t.detach().double() for t in (p, g, m, v))
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    p = p + (-step_size * m) / (v.sqrt() / bc2_sqrt + eps)
    return p, m, v


def torch_cpu_adam(p, g, m, v, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, step=1):
    """torch.optim.Adam(foreach=False) (_single_tensor_adam) on the CPU, in the
    tensors' own dtype, from the state (p, m, v, step - 1).  Returns new
    (p, m, v); the arguments are left alone."""
    prm = torch.nn.Parameter(p.detach().cpu().clone())
    opt = torch.optim.Adam([prm], lr=lr, betas=betas, eps=eps, foreach=False)
    opt.state[prm] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().cpu().clone(),
                      "exp_avg_sq": v.detach().cpu().clone()}
    prm.grad = g.detach().cpu().clone()
    opt.step()
    st = opt.state[prm]
    return prm.detach(), st["exp_avg"], st["exp_avg_sq"]
