"""The BN-backward apply kernel (bn_bwd_apply_k, csrc/mmad_ops_bn_bwd.hip) on its own,
against a float64 torch restatement of the formula it evaluates -- the
backward of layers/fc_layer.py:39-45's BatchNorm1d(act(Linear)) as autograd
forms it:

    dbeta = sum dy,  dgamma = sum dy * xhat,  xhat = (a - mean) * rstd
    dz    = act'(a) * gamma * rstd / M * (M dy - dbeta - xhat * dgamma)

fed with the bwd-data epilogue's per-64-row fp64 column partials of (sum dy,
sum dy*xhat).  Every activation (the LeakyReLU-specialised kernel and the
generic one), bf16 and fp32, a ragged batch (rows past M give dz = 0), and
both partial-merge widths (64 partials per column at 4096 padded rows, 16 at
1024).  bf16: dz within 2^-7 of the column's largest |dz| (one bf16 rounding
of an fp32 bracket); fp32 (fp64 bracket): 1e-5."""
import ctypes

import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import ptr, stream_ptr

pytestmark = pytest.mark.gpu

_ACT = {"leakyrelu": 1, "relu": 2, "sigmoid": 3, "tanh": 4}
SLOPE = 0.2


def _fn():
    lib = _native.load()
    fn = lib._Z21mmad_bn_act_bwd_applyiifiiiiPKvS0_PKfS2_S2_PKdiPvPfS6_S6_S5_
    fn.restype = ctypes.c_int
    P = ctypes.c_void_p
    fn.argtypes = ([ctypes.c_int, ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 4 + [P] * 6 +
                   [ctypes.c_int] + [P] * 5)
    return fn


def _act_grad(a, act):
    if act == "leakyrelu":
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    if act == "relu":
        return (a > 0).to(a.dtype)
    if act == "sigmoid":
        return a * (1 - a)
    return 1 - a * a


@pytest.mark.parametrize("act", list(_ACT))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("M,N,Mp,Np", [(4000, 1000, 4096, 1024), (1024, 300, 1024, 384)])
def test_bn_bwd_apply_matches_float64(act, dtype, M, N, Mp, Np):
    torch.manual_seed(M + N + _ACT[act])
    dev = torch.device("cuda", 0)
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    # the activation output a (BN input) in the activation's range; dy
    dy = torch.zeros(Mp, Np, device=dev, dtype=td)
    a = torch.zeros(Mp, Np, device=dev, dtype=td)
    dy[:M, :N] = torch.randn(M, N, device=dev).to(td)
    if act == "sigmoid":
        a[:M, :N] = torch.rand(M, N, device=dev).to(td)
    elif act == "tanh":
        a[:M, :N] = (torch.rand(M, N, device=dev) * 2 - 1).to(td)
    else:
        a[:M, :N] = (torch.randn(M, N, device=dev) + 0.3).to(td)
    a64, dy64 = a[:M, :N].double(), dy[:M, :N].double()
    mean = torch.zeros(Np, device=dev)
    rstd = torch.zeros(Np, device=dev)
    mean[:N] = a64.mean(0).float()
    rstd[:N] = (1.0 / torch.sqrt(a64.var(0, unbiased=False) + 1e-5)).float()
    gamma = torch.zeros(Np, device=dev)
    gamma[:N] = torch.rand(N, device=dev) + 0.5
    xh = (a64 - mean[:N].double()) * rstd[:N].double()
    # the bwd-data epilogue's partials: [Mp/64][2][Np] fp64, chunk i = rows 64i..64i+63
    nparts = Mp // 64
    part = torch.zeros(nparts, 2, Np, device=dev, dtype=torch.float64)
    dyp = torch.zeros(Mp, N, device=dev, dtype=torch.float64)
    dxp = torch.zeros(Mp, N, device=dev, dtype=torch.float64)
    dyp[:M] = dy64
    dxp[:M] = dy64 * xh
    part[:, 0, :N] = dyp.view(nparts, 64, N).sum(1)
    part[:, 1, :N] = dxp.view(nparts, 64, N).sum(1)
    dz = torch.full((Mp, Np), float("nan"), device=dev).to(td)
    dg = torch.zeros(Np, device=dev)
    db = torch.zeros(Np, device=dev)
    dbp = torch.zeros(Mp // 128, Np, device=dev)
    rc = _fn()(1 if dtype == "bf16" else 0, _ACT[act], SLOPE, M, N, Mp, Np, ptr(dy), ptr(a), ptr(mean),
               ptr(rstd), ptr(gamma), ptr(part), nparts, ptr(dz), ptr(dg), ptr(db), ptr(dbp), stream_ptr())
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    sdy, sdx = dy64.sum(0), (dy64 * xh).sum(0)
    cf = gamma[:N].double() * rstd[:N].double() / M
    ref = _act_grad(a64, act) * cf * (M * dy64 - sdy - xh * sdx)
    assert torch.allclose(db[:N].double(), sdy, rtol=1e-5, atol=1e-4)
    assert torch.allclose(dg[:N].double(), sdx, rtol=1e-5, atol=1e-4)
    out = dz.double()
    assert torch.isfinite(out).all()
    assert (out[M:] == 0).all() and (out[:, N:] == 0).all()
    tol = 2.0 ** -7 if dtype == "bf16" else 1e-5
    scale = ref.abs().amax(0).clamp_min(1e-30)
    assert float(((out[:M, :N] - ref).abs() / scale).max()) < tol
    # db partials: per 128-row slab, the column sum of the dz this kernel wrote
    want = out[:, :N].view(Mp // 128, 128, N).sum(1)
    assert torch.allclose(dbp[:, :N].double(), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))
