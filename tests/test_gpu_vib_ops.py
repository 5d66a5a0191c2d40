"""The VIB waist as operators: mmad_vib_reparam_fwd / mmad_vib_reparam_bwd
(vib_fwd_k, vib_bwd_k, philox_normal, csrc/mmad_ops_vib.hip; the colsum pass,
csrc/mmad_ops_reduce.hip)
through the public C-ABI, against float64 of the values the kernels read.

* the generated noise (eps = NULL) against the numpy Philox4x32-10 +
  Box-Muller restatement of tests/philox_ref.py, high seed / offset words
  included;
* the forward with injected eps, the zero padding of the packed z buffer, the
  deterministic form;
* the KL partials, sized by the count include/mmad.h documents, with guard
  floats behind them;
* the backward with beta_kl in {0, 1, 0.25} and its column-sum partials.

mu ~ N(0,1), logvar uniform in [-6, 4], both rounded to the operand type
first; every buffer is allocated at its full padded size, with NaN wherever
the kernels must not read and must (or must not) write.  Bounds come from the
number formats (see each test); the worst observed error / bound goes to
$MMAD_RECORD_DIR/vib_ops.json (default test_records/), the run quoted in
DESIGN.md is kept as profiles/vib_ops_tests.md."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, pad, ptr, stream_ptr
from tests import philox_ref

pytestmark = pytest.mark.gpu

# (B, btl, k, ld_enc, ld_z): one element; a batch inside a slab with k = 3; a
# full 128-row slab; one row past it with a 256-wide encoder output; the
# unpadded FCLayer form (ld_enc = 2 btl, ld_z = btl)
SHAPES = [(1, 1, 1, 128, 128), (37, 5, 3, 128, 128), (128, 64, 1, 128, 128), (129, 100, 2, 256, 128),
          (200, 16, 2, 32, 16)]
DTYPES = {"f32": (_native.F32, torch.float32), "bf16": (_native.BF16, torch.bfloat16)}
SEEDS = [(0, 0), (7, 3), (2 ** 40 + 5, 2 ** 33 + 1)]
SENTINEL = -1234.5
GUARD = 64
NAN = float("nan")

_REC = {}


def _record(key, value):
    """Keep the worst value seen per key and rewrite the record file."""
    value = float(value)
    if value > _REC.get(key, -1.0):
        _REC[key] = value
        out_dir = os.environ.get("MMAD_RECORD_DIR", "test_records")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "vib_ops.json"), "w") as f:
            json.dump(_REC, f, indent=1, sort_keys=True)


def _worst(err, tol):
    """max err / tol over the elements (an element with tol = 0 must have err = 0)."""
    err, tol = err.reshape(-1), tol.reshape(-1)
    if err.numel() == 0:
        return 0.0
    zero = tol == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0


def _kl_parts(B, k, ld_z):
    """The kl_partial count include/mmad.h documents."""
    return (pad(k * B) * ld_z + 255) // 256


@functools.lru_cache(maxsize=None)
def _case(B, btl, k, ld_enc, ld_z, dtype):
    """Inputs of one (shape, dtype) and their float64 values, built once."""
    td = DTYPES[dtype][1]
    g = torch.Generator().manual_seed(1000 * B + 10 * btl + k)
    mu = torch.randn(B, btl, generator=g).to(td)
    lv = (torch.rand(B, btl, generator=g) * 10 - 6).to(td)
    eps = torch.randn(k, B, btl, generator=g)
    dz = torch.randn(k * B, btl, generator=g).to(td)
    enc = torch.full((pad(B), ld_enc), NAN, dtype=td)
    enc[:B, :btl] = mu
    enc[:B, btl:2 * btl] = lv
    dzp = torch.full((pad(k * B), ld_z), NAN, dtype=td)
    dzp[:k * B, :btl] = dz
    return dict(B=B, btl=btl, k=k, ld_enc=ld_enc, ld_z=ld_z, dt=DTYPES[dtype][0], td=td, dtype=dtype,
                enc=enc.cuda(), eps=eps.cuda(), dz=dzp.cuda(), mu64=mu.double(), lv64=lv.double(),
                eps64=eps.double(), dz64=dz.double().view(k, B, btl))


def _fwd(c, eps=None, eps_out=None, seed=0, offset=0, det=0, kl=None, k=None):
    k = c["k"] if k is None else k
    z = torch.full((pad(k * c["B"]), c["ld_z"]), NAN, dtype=c["td"], device="cuda")
    call("mmad_vib_reparam_fwd", c["dt"], c["B"], c["btl"], k, ptr(c["enc"]), c["ld_enc"], ptr(eps),
         ptr(eps_out), seed, offset, det, ptr(z), c["ld_z"], ptr(kl), stream_ptr())
    torch.cuda.synchronize()
    return z.cpu()


def _fwd_tol(c, eps64):
    """|z - ref| bound: fp32 1e-5 (|mu| + |eps| sigma) -- the fast exp over
    [-3, 2] is within about 2e-7 relative, so about 50x -- plus one RNE output
    rounding, 2^-8 |ref|, in bf16.  Returns (ref, tol), [k][B][btl] float64."""
    sig = torch.exp(0.5 * c["lv64"])
    ref = eps64 * sig + c["mu64"]
    tol = 1e-5 * (c["mu64"].abs() + eps64.abs() * sig)
    if c["dtype"] == "bf16":
        tol = tol + 2.0 ** -8 * ref.abs()
    return ref, tol


def _check_z(c, z, eps64, what):
    B, btl, k = c["B"], c["btl"], c["k"]
    ref, tol = _fwd_tol(c, eps64)
    got = z[:k * B, :btl].double().view(k, B, btl)
    err = (got - ref).abs()
    w = _worst(err, tol)
    print(f"{what} {c['dtype']} B={B} btl={btl} k={k}: worst err / bound {w:.4f}")
    _record(f"{what}_{c['dtype']}", w)
    assert (err <= tol).all(), w
    # padding of the packed z buffer: exactly 0
    assert (z[k * B:] == 0).all() and (z[:, btl:] == 0).all()


# ------------------------------------------------------------ 1. generated noise
@pytest.mark.parametrize("seed,offset", SEEDS)
@pytest.mark.parametrize("B,btl,k,ld_enc,ld_z", SHAPES)
def test_generated_noise_matches_philox_reference(B, btl, k, ld_enc, ld_z, seed, offset):
    """eps = NULL: eps_out is the draw of tests/philox_ref.py, within
    1e-4 (1 + |ref|) where u1 <= 0.99 and 5e-3 absolute elsewhere (near
    u1 -> 1 an absolute error d of the fast log gives up to sqrt(2 d) in the
    draw, 1.4e-3 for d = 1e-6); a wrong generator is off by O(1)."""
    ref, u1 = philox_ref.vib_eps(seed, offset, k, B, btl)
    ref, u1 = torch.from_numpy(ref), torch.from_numpy(u1)
    n = k * B * btl
    outs = {}
    for dtype in DTYPES:
        c = _case(B, btl, k, ld_enc, ld_z, dtype)
        eo = torch.full((n + GUARD,), SENTINEL, device="cuda")
        z = _fwd(c, eps_out=eo, seed=seed, offset=offset)
        eo2 = torch.full((n + GUARD,), SENTINEL, device="cuda")
        z2 = _fwd(c, eps_out=eo2, seed=seed, offset=offset)
        # the same seed and offset give the same bits
        assert torch.equal(eo, eo2) and torch.equal(z.view(torch.uint8), z2.view(torch.uint8))
        eo = eo.cpu()
        assert (eo[n:] == SENTINEL).all()
        got = eo[:n].view(k, B, btl)
        assert torch.isfinite(got).all()
        err = (got.double() - ref).abs()
        body = u1 <= 0.99
        rel = float((err[body] / (1 + ref[body].abs())).max()) if body.any() else 0.0
        tail = float(err[~body].max()) if (~body).any() else 0.0
        print(f"noise {dtype} B={B} btl={btl} k={k} seed={seed} offset={offset}: "
              f"u1<=0.99 err/(1+|ref|) {rel:.3e}, u1>0.99 abs err {tail:.3e}")
        _record("noise_rel_u1_le_0.99", rel)
        _record("noise_abs_u1_gt_0.99", tail)
        assert rel <= 1e-4
        assert tail <= 5e-3
        # z is built from that draw
        _check_z(c, z, got.double(), "z_generated")
        outs[dtype] = got
    # the draw does not depend on the operand type
    assert torch.equal(outs["f32"], outs["bf16"])
    # the k samples of one window differ (iid draws collide with probability ~2^-24 each)
    for kk in range(1, k):
        assert float((outs["f32"][kk] != outs["f32"][0]).double().mean()) > 0.99
    # another offset or seed gives another draw
    c = _case(B, btl, k, ld_enc, ld_z, "f32")
    for s2, o2 in ((seed, offset + 1), (seed + 1, offset)):
        eo = torch.full((n + GUARD,), SENTINEL, device="cuda")
        _fwd(c, eps_out=eo, seed=s2, offset=o2)
        assert not torch.equal(eo.cpu()[:n].view(k, B, btl), outs["f32"])


# ------------------------------------------------------ 2. forward, injected eps
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,btl,k,ld_enc,ld_z", SHAPES)
def test_forward_injected_eps(B, btl, k, ld_enc, ld_z, dtype):
    c = _case(B, btl, k, ld_enc, ld_z, dtype)
    n = k * B * btl
    eo = torch.full((n + GUARD,), SENTINEL, device="cuda")
    z = _fwd(c, eps=c["eps"], eps_out=eo)
    _check_z(c, z, c["eps64"], "z_injected")
    # the noise used is handed back unchanged
    eo = eo.cpu()
    assert torch.equal(eo[:n], c["eps"].cpu().reshape(-1)) and (eo[n:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,btl,k,ld_enc,ld_z", SHAPES)
def test_forward_deterministic_is_mu(B, btl, k, ld_enc, ld_z, dtype):
    """deterministic = 1: z == mu bit for bit in every one of the k copies,
    zero padding, eps_out untouched."""
    c = _case(B, btl, k, ld_enc, ld_z, dtype)
    n = k * B * btl
    eo = torch.full((n + GUARD,), SENTINEL, device="cuda")
    z = _fwd(c, eps=c["eps"], eps_out=eo, det=1)
    mu = c["enc"].cpu()[:B, :btl].contiguous()
    for kk in range(k):
        got = z[kk * B:(kk + 1) * B, :btl].contiguous()
        assert torch.equal(got.view(torch.uint8), mu.view(torch.uint8))
    assert (z[k * B:] == 0).all() and (z[:, btl:] == 0).all()
    assert (eo.cpu() == SENTINEL).all()


# ------------------------------------------------------------------ 3. KL partials
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,btl,k,ld_enc,ld_z", SHAPES)
def test_kl_partials(B, btl, k, ld_enc, ld_z, dtype):
    """The float64 sum of the partials against -1/2 sum(1 + lv - mu^2 - e^lv)
    over the B windows, within 2e-5 A, A = 1/2 sum(1 + |lv| + mu^2 + e^lv)
    (fp32 terms and partial sums, the fast exp); the buffer holds exactly the
    documented count, the floats behind it stay; the kk > 0 copies add nothing."""
    c = _case(B, btl, k, ld_enc, ld_z, dtype)
    mu, lv = c["mu64"], c["lv64"]
    want = float((-0.5 * (1 + lv - mu * mu - torch.exp(lv))).sum())
    A = float((0.5 * (1 + lv.abs() + mu * mu + torch.exp(lv))).sum())
    sums = {}
    for kk in (k, 3 if k == 1 else 1):
        parts = _kl_parts(B, kk, ld_z)
        kl = torch.full((parts + GUARD,), SENTINEL, device="cuda")
        _fwd(c, eps=c["eps"] if kk == k else None, kl=kl, k=kk, seed=5, offset=1)
        kl = kl.cpu()
        assert (kl[parts:] == SENTINEL).all()
        assert torch.isfinite(kl[:parts]).all() and (kl[:parts] != SENTINEL).all()
        sums[kk] = float(kl[:parts].double().sum())
    w = abs(sums[k] - want) / (2e-5 * A)
    print(f"kl {dtype} B={B} btl={btl} k={k}: {sums[k]:.9e} want {want:.9e}, err / bound {w:.4f}")
    _record(f"kl_{dtype}", w)
    assert abs(sums[k] - want) <= 2e-5 * A
    # the windows' blocks hold the same terms whatever k is; the others hold 0
    assert len(set(sums.values())) == 1, sums


# --------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.25])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,btl,k,ld_enc,ld_z", SHAPES)
def test_backward(B, btl, k, ld_enc, ld_z, dtype, beta):
    """dmu = sum_k dz + beta mu, dlv = 1/2 sigma sum_k dz eps + 1/2 beta (e^lv - 1),
    within 1e-5 S (S the sum of the terms' magnitudes) plus, in bf16, one output
    rounding 2^-8 |ref|; zero padding; colsum partials = float64 column sums of
    the d_enc_out written, per 128-row slab, within 1e-5 sum |.|."""
    c = _case(B, btl, k, ld_enc, ld_z, dtype)
    td = c["td"]
    ld_denc, Mpe = ld_enc, pad(B)
    denc = torch.full((Mpe, ld_denc), NAN, dtype=td, device="cuda")
    with_colsum = ld_denc % 64 == 0
    cs = torch.full((Mpe // 128 * ld_denc + GUARD,), SENTINEL, device="cuda") if with_colsum else None
    call("mmad_vib_reparam_bwd", c["dt"], B, btl, k, ptr(c["enc"]), ld_enc, ptr(c["eps"]), ptr(c["dz"]),
         ld_z, beta, ptr(denc), ld_denc, ptr(cs), stream_ptr())
    torch.cuda.synchronize()
    out = denc.cpu().double()
    mu, lv, dz, eps = c["mu64"], c["lv64"], c["dz64"], c["eps64"]
    sig = torch.exp(0.5 * lv)
    ref_mu = dz.sum(0) + beta * mu
    s_mu = dz.abs().sum(0) + beta * mu.abs()
    ref_lv = 0.5 * sig * (dz * eps).sum(0) + 0.5 * beta * (torch.exp(lv) - 1)
    s_lv = 0.5 * sig * (dz * eps).abs().sum(0) + 0.5 * beta * (torch.exp(lv) + 1)
    for name, got, ref, s in (("dmu", out[:B, :btl], ref_mu, s_mu), ("dlv", out[:B, btl:2 * btl], ref_lv, s_lv)):
        tol = 1e-5 * s + (2.0 ** -8 * ref.abs() if dtype == "bf16" else 0.0)
        err = (got - ref).abs()
        w = _worst(err, tol)
        print(f"{name} {dtype} B={B} btl={btl} k={k} beta={beta}: worst err / bound {w:.4f}")
        _record(f"{name}_{dtype}", w)
        assert (err <= tol).all(), (name, w)
    assert (out[B:] == 0).all() and (out[:, 2 * btl:] == 0).all()
    if with_colsum:
        cs = cs.cpu()
        n = Mpe // 128 * ld_denc
        assert (cs[n:] == SENTINEL).all()
        got = cs[:n].double().view(Mpe // 128, ld_denc)
        slabs = out.view(Mpe // 128, 128, ld_denc)
        want, mag = slabs.sum(1), slabs.abs().sum(1)
        err = (got - want).abs()
        w = _worst(err, 1e-5 * mag)
        print(f"colsum {dtype} B={B} btl={btl} k={k} beta={beta}: worst err / bound {w:.4f}")
        _record(f"colsum_{dtype}", w)
        assert (err <= 1e-5 * mag).all(), w
