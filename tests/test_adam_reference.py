"""tests/adam_ref.py against itself (no GPU): the float64 formula of
include/mmad.h's mmad_adam and torch.optim.Adam's CPU single-tensor step, run
in float64 from the same state, agree to 1e-12 relative (max-norm) at steps 1,
2 and 1000 and for the betas tests/test_gpu_adam_ops.py uses."""
import pytest
import torch

from tests import adam_ref as A

BETAS = [((0.9, 0.999), 1e-3), ((0.8, 0.95), 3e-4)]   # test_gpu_adam_ops.CONFIGS' hyper-parameters


def _state(n, step, seed):
    g_ = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g_, dtype=torch.float64) * 0.05
    g = torch.randn(n, generator=g_, dtype=torch.float64) * 1e-2
    m = torch.randn(n, generator=g_, dtype=torch.float64) * 1e-3 if step > 1 else torch.zeros(n, dtype=torch.float64)
    v = torch.rand(n, generator=g_, dtype=torch.float64) * 1e-5 if step > 1 else torch.zeros(n, dtype=torch.float64)
    return p, g, m, v


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("betas,lr", BETAS)
def test_float64_formula_is_torch_cpu_adam(betas, lr, step):
    p, g, m, v = _state(4099, step, seed=step)
    keep = [t.clone() for t in (p, g, m, v)]
    want = A.torch_cpu_adam(p, g, m, v, lr=lr, betas=betas, eps=1e-8, step=step)
    got = A.adam_step_f64(p, g, m, v, lr=lr, betas=betas, eps=1e-8, step=step)
    for name, a, b in zip("pmv", got, want):
        assert a.dtype == torch.float64 and b.dtype == torch.float64
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f"betas {betas} step {step} {name}: {err:.2e}")
        assert err <= 1e-12, (name, err)
    # both helpers leave their arguments alone
    for t, k in zip((p, g, m, v), keep):
        assert torch.equal(t, k)
    # and the step moved something
    assert not torch.equal(got[0], p)


def test_consts_are_the_bias_corrections():
    s, b = A.adam_consts(1e-3, (0.9, 0.999), 1)
    assert abs(s - 1e-2) <= 1e-15 * 1e-2 and abs(b - 0.001 ** 0.5) <= 1e-12 * b
    s, b = A.adam_consts(3e-4, (0.8, 0.95), 2)
    assert abs(s - 3e-4 / 0.36) <= 1e-12 * s and abs(b - 0.0975 ** 0.5) <= 1e-12 * b
