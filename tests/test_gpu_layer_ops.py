"""The layer operators between the GEMMs (csrc/mmad_ops_*.hip), fp32 and bf16,
through the public C-ABI at the edges where the 64-column x 128-row slab
kernels index differently: a batch that ends inside a 32-row statistics
chunk, inside / at / one past a 128-row slab, widths at 63 / 64 / 65 of a
column slab.

    mmad_pack_input, mmad_unpack_output        bit-exact against torch (also the split-bf16 planes)
    mmad_bn_train_apply, mmad_bn_eval_affine   float64 from the input itself
    mmad_bn_act_bwd (reduce + apply)           float64, bounds of test_gpu_bn_apply.py
    mmad_act_bwd, mmad_colsum                  exact dz, float64 column sums

Buffers have their full padded size.  Padding columns of packed operands are
zero (the packed layout); padding rows hold a finite sentinel, so a kernel
that let them into a sum or a statistic would show; outputs start as NaN.
The worst observed error / bound goes to $MMAD_RECORD_DIR/layer_ops.json
(default test_records/); the run quoted in DESIGN.md is in
profiles/vib_ops_tests.md."""
import json
import os

import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, pad, ptr, stream_ptr

pytestmark = pytest.mark.gpu

# every M of {2, 31, 32, 33, 127, 128, 129, 200} and every N of
# {1, 63, 64, 65, 128, 130} at least once
PAIRS = [(2, 1), (31, 63), (32, 64), (33, 65), (127, 128), (128, 130), (129, 1), (200, 65), (128, 64),
         (33, 130)]
DTYPES = {"f32": (_native.F32, torch.float32), "bf16": (_native.BF16, torch.bfloat16)}
# pack / unpack also have a split-bf16 form: two bf16 planes [2][Mp][Kp], hi = RNE(x), lo = RNE(x - hi)
PACK_DTYPES = list(DTYPES) + ["x3"]
ACTS = ["leakyrelu", "relu", "sigmoid", "tanh"]
SLOPE = 0.2
ROW_SENTINEL = 3.0
SENTINEL = -1234.5
GUARD = 64
NAN = float("nan")

_REC = {}


def _record(key, value):
    value = float(value)
    if value > _REC.get(key, -1.0):
        _REC[key] = value
        out_dir = os.environ.get("MMAD_RECORD_DIR", "test_records")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "layer_ops.json"), "w") as f:
            json.dump(_REC, f, indent=1, sort_keys=True)


def _worst(err, tol):
    """max err / tol (an element with tol = 0 must have err = 0)."""
    err, tol = err.reshape(-1), tol.expand_as(err).reshape(-1)
    if err.numel() == 0:
        return 0.0
    zero = tol == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * p for k, p in zip(key, (1009, 31, 7, 3))))


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _packed(M, N, vals, td, row_fill=ROW_SENTINEL):
    """[Mp][Np] operand: vals in [M][N], zero padding columns, row_fill in rows >= M."""
    out = torch.zeros(pad(M), pad(N), dtype=td)
    out[M:, :] = row_fill
    out[:M, :N] = vals.to(td)
    return out


# ------------------------------------------------------------ 1. pack / unpack
def _pack_sources(M, K):
    """(name, ld_x, offset in floats): the aligned vector path; ld_x > K; an
    ld_x that is no multiple of 4 and a source one float off 16-byte alignment
    (both the scalar path)."""
    r4 = (K + 3) // 4 * 4
    odd = K + 1 if (K + 1) % 4 else K + 2
    return [("vector", r4, 0), ("ld_x>K", r4 + 8, 0), ("ld_x%4", odd, 0), ("offset", r4 + 4, 1)]


def _planes_of(x):
    hi = x.bfloat16()
    return torch.stack((hi, (x - hi.float()).bfloat16()))


@pytest.mark.parametrize("dtype", PACK_DTYPES)
@pytest.mark.parametrize("M,K", PAIRS)
def test_pack_input_is_torch_rounding(M, K, dtype):
    """out[:M, :K] is x.to(dtype) bit for bit (RNE for bf16, a copy for fp32),
    everything else of [Mp][Kp] is 0.  x3: both planes of [2][Mp][Kp]."""
    if dtype == "x3":
        return _pack_planes_case(M, K)
    dt, td = DTYPES[dtype]
    Mp, Kp = pad(M), pad(K)
    for name, ld_x, off in _pack_sources(M, K):
        g = _gen(M, K, ld_x, off)
        flat = torch.randn(off + M * ld_x + GUARD, generator=g) * 3
        # bf16 rounding ties (to even: down, up), the largest finite bf16 step, tiny values
        ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -130, -0.0, 65280.0])
        flat[off:off + min(6, M * ld_x)] = ties[:min(6, M * ld_x)]
        x = flat[off:off + M * ld_x].view(M, ld_x)
        dflat = flat.cuda()
        src = dflat[off:]
        assert (src.data_ptr() % 16 == 0) == (off == 0)
        out = torch.full((Mp, Kp), NAN, dtype=td, device="cuda")
        call("mmad_pack_input", dt, M, K, Mp, Kp, ptr(src), ld_x, ptr(out), stream_ptr())
        torch.cuda.synchronize()
        out = out.cpu()
        want = torch.zeros(Mp, Kp, dtype=td)
        want[:M, :K] = x[:, :K].to(td)
        assert torch.equal(_bits(out[:M, :K]), _bits(want[:M, :K])), name
        assert (out[M:] == 0).all() and (out[:, K:] == 0).all(), name


def _pack_planes_case(M, K):
    """the x3 form on the sources and special values of the test above"""
    Mp, Kp = pad(M), pad(K)
    for name, ld_x, off in _pack_sources(M, K):
        g = _gen(M, K, ld_x, off)
        flat = torch.randn(off + M * ld_x + GUARD, generator=g) * 3
        ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -130, -0.0, 65280.0])
        flat[off:off + min(6, M * ld_x)] = ties[:min(6, M * ld_x)]
        x = flat[off:off + M * ld_x].view(M, ld_x)
        dflat = flat.cuda()
        src = dflat[off:]
        assert (src.data_ptr() % 16 == 0) == (off == 0)
        out = torch.full((2, Mp, Kp), NAN, dtype=torch.bfloat16, device="cuda")
        call("mmad_pack_input", _native.BF16X3, M, K, Mp, Kp, ptr(src), ld_x, ptr(out), stream_ptr())
        torch.cuda.synchronize()
        out = out.cpu()
        want = _planes_of(x[:, :K].contiguous())
        assert torch.equal(_bits(out[0, :M, :K]), _bits(want[0])), name
        assert torch.equal(_bits(out[1, :M, :K]), _bits(want[1])), name
        assert (out[:, M:] == 0).all() and (out[:, :, K:] == 0).all(), name


@pytest.mark.parametrize("dtype", PACK_DTYPES)
@pytest.mark.parametrize("M,N", PAIRS)
def test_unpack_output_writes_only_the_valid_region(M, N, dtype):
    """x3: out = float(hi) + float(lo) bit for bit, the lo plane at
    roundup(M, 128) * Np elements."""
    if dtype == "x3":
        return _unpack_planes_case(M, N)
    dt, td = DTYPES[dtype]
    Mp, Np, ld_out = pad(M), pad(N), N + 3
    y = torch.full((Mp, Np), NAN, dtype=td)
    y[:M, :N] = (torch.randn(M, N, generator=_gen(M, N)) * 3).to(td)
    out = torch.full((M * ld_out + GUARD,), SENTINEL, device="cuda")
    yd = y.cuda()
    call("mmad_unpack_output", dt, M, N, Np, ptr(yd), ptr(out), ld_out, stream_ptr())
    torch.cuda.synchronize()
    out = out.cpu()
    body = out[:M * ld_out].view(M, ld_out)
    assert torch.equal(_bits(body[:, :N]), _bits(y[:M, :N].float()))
    assert (body[:, N:] == SENTINEL).all() and (out[M * ld_out:] == SENTINEL).all()


def _unpack_planes_case(M, N):
    Mp, Np, ld_out = pad(M), pad(N), N + 3
    y = torch.full((2, Mp, Np), NAN, dtype=torch.bfloat16)
    y[:, :M, :N] = _planes_of(torch.randn(M, N, generator=_gen(M, N)) * 3)
    assert (y[1, :M, :N] != 0).any()
    out = torch.full((M * ld_out + GUARD,), SENTINEL, device="cuda")
    yd = y.cuda()
    call("mmad_unpack_output", _native.BF16X3, M, N, Np, ptr(yd), ptr(out), ld_out, stream_ptr())
    torch.cuda.synchronize()
    out = out.cpu()
    body = out[:M * ld_out].view(M, ld_out)
    assert torch.equal(_bits(body[:, :N]), _bits(y[0, :M, :N].float() + y[1, :M, :N].float()))
    assert (body[:, N:] == SENTINEL).all() and (out[M * ld_out:] == SENTINEL).all()


# ------------------------------------------------------------ 2. BN train / eval
def _bn_input(M, N, td, g):
    """a [M][N] in the dtype: distinct column means in [-3, 3], column std >= 0.5."""
    means = torch.linspace(-3.0, 3.0, N)[torch.randperm(N, generator=g)] if N > 1 else torch.tensor([1.5])
    a = (means + (0.75 + torch.rand(N, generator=g)) * torch.randn(M, N, generator=g)).to(td)
    low = a.double().std(0, unbiased=False) < 0.5
    if low.any():   # few rows: push the rows apart
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).view(M, 1)
        a = torch.where(low, (a.float() + sign).to(td), a)
    assert (a.double().std(0, unbiased=False) >= 0.5).all()
    return a


def _chunk_stats(a64, M, N, Mp, Np):
    """The forward GEMM's Welford partials [Mp/32][2][Np]: (mean, M2) of each
    32-row chunk's valid rows, float64 rounded to fp32; a large sentinel in the
    chunks that hold no valid row."""
    nparts = Mp // 32
    st = torch.zeros(nparts, 2, Np)
    for i in range(nparts):
        rows = a64[32 * i:min(M, 32 * i + 32)]
        if rows.shape[0] == 0:
            st[i, :, :N] = 1e30
            continue
        m = rows.mean(0)
        st[i, 0, :N] = m.float()
        st[i, 1, :N] = ((rows - m) ** 2).sum(0).float()
    return st


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("M,N", PAIRS)
def test_bn_train_apply_matches_float64(M, N, dtype):
    """y, save_mean, save_rstd and the running statistics against float64
    BatchNorm1d of a itself.  save_mean within 1e-6 (|mean| + std) (fp32
    chunk means merged in fp64), rstd and the running stats 1e-5 relative, y
    within 1e-5 of the column's largest |y| (fp32 a * scale + shift), plus one
    output rounding 2^-8 |ref| in bf16."""
    dt, td = DTYPES[dtype]
    Mp, Np, eps = pad(M), pad(N), 1e-5
    g = _gen(M, N, 5)
    a = _bn_input(M, N, td, g)
    a64 = a.double()
    mean, var = a64.mean(0), a64.var(0, unbiased=False)
    std, rstd = var.sqrt(), 1.0 / torch.sqrt(var + eps)
    gamma = torch.full((Np,), NAN)
    beta = torch.full((Np,), NAN)
    gamma[:N] = 0.5 + torch.rand(N, generator=g)
    beta[:N] = 0.5 * torch.randn(N, generator=g)
    ref_y = (a64 - mean) * rstd * gamma[:N].double() + beta[:N].double()
    # running stats start away from zero, on the side of the batch mean (no cancellation in the update)
    rm0 = torch.full((Np,), SENTINEL)
    rv0 = torch.full((Np,), SENTINEL)
    rm0[:N] = torch.where(mean >= 0, 1.0, -1.0).float() * (0.5 + torch.rand(N, generator=g))
    rv0[:N] = 0.5 + torch.rand(N, generator=g)
    ad = _packed(M, N, a, td).cuda()
    stats = _chunk_stats(a64, M, N, Mp, Np).cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    for momentum in (0.1, 1.0):
        rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
        sm = torch.full((Np,), NAN, device="cuda")
        sr = torch.full((Np,), NAN, device="cuda")
        y = torch.full((Mp, Np), NAN, dtype=td, device="cuda")
        call("mmad_bn_train_apply", dt, M, N, Mp, Np, ptr(ad), ptr(stats), ptr(gd), ptr(bd), ptr(rm), ptr(rv),
             momentum, eps, ptr(sm), ptr(sr), ptr(y), stream_ptr())
        torch.cuda.synchronize()
        rm, rv, sm, sr, y = (t.cpu().double() for t in (rm, rv, sm, sr, y))
        unb = var * M / (M - 1)
        ref_rm = (1 - momentum) * rm0[:N].double() + momentum * mean
        ref_rv = (1 - momentum) * rv0[:N].double() + momentum * unb
        colmax = ref_y.abs().amax(0)
        ytol = 1e-5 * colmax + (2.0 ** -8 * ref_y.abs() if dtype == "bf16" else 0.0)
        checks = [("save_mean", sm[:N], mean, 1e-6 * (mean.abs() + std)),
                  ("save_rstd", sr[:N], rstd, 1e-5 * rstd),
                  ("running_mean", rm[:N], ref_rm, 1e-5 * ref_rm.abs()),
                  ("running_var", rv[:N], ref_rv, 1e-5 * ref_rv.abs()),
                  ("y", y[:M, :N], ref_y, ytol)]
        for name, got, ref, tol in checks:
            err = (got - ref).abs()
            w = _worst(err, tol)
            print(f"bn_train_apply {dtype} M={M} N={N} momentum={momentum} {name}: err / bound {w:.4f}")
            _record(f"bn_train_{name}_{dtype}", w)
            assert (err <= tol).all(), (name, w)
        assert (y[M:] == 0).all() and (y[:, N:] == 0).all()
        assert (sm[N:] == 0).all() and (sr[N:] == 0).all()
        assert (rm[N:] == SENTINEL).all() and (rv[N:] == SENTINEL).all()


@pytest.mark.parametrize("N", [1, 65, 130])
def test_bn_eval_affine_matches_float64(N):
    """scale = gamma / sqrt(rv + eps) 1e-5 relative; shift = beta - rm scale
    within 1e-5 (|beta| + |rm scale|) (one fp32 product and difference);
    padded columns 0."""
    Np, eps = pad(N), 1e-5
    g = _gen(N, 11)
    gamma, beta, rm, rv = (torch.full((Np,), NAN) for _ in range(4))
    gamma[:N] = 0.5 + torch.rand(N, generator=g)
    beta[:N] = torch.randn(N, generator=g)
    rm[:N] = 2 * torch.randn(N, generator=g)
    rv[:N] = torch.rand(N, generator=g) * 4 + 1e-3
    scale = torch.full((Np,), NAN, device="cuda")
    shift = torch.full((Np,), NAN, device="cuda")
    dev = [t.cuda() for t in (gamma, beta, rm, rv)]
    call("mmad_bn_eval_affine", N, Np, *(ptr(t) for t in dev), eps, ptr(scale), ptr(shift), stream_ptr())
    torch.cuda.synchronize()
    scale, shift = scale.cpu().double(), shift.cpu().double()
    ref_sc = gamma[:N].double() / torch.sqrt(rv[:N].double() + eps)
    ref_sh = beta[:N].double() - rm[:N].double() * ref_sc
    for name, got, ref, tol in (("scale", scale[:N], ref_sc, 1e-5 * ref_sc.abs()),
                                ("shift", shift[:N], ref_sh,
                                 1e-5 * (beta[:N].double().abs() + (rm[:N].double() * ref_sc).abs()))):
        err = (got - ref).abs()
        w = _worst(err, tol)
        print(f"bn_eval_affine N={N} {name}: err / bound {w:.4f}")
        _record(f"bn_eval_{name}", w)
        assert (err <= tol).all(), (name, w)
    assert (scale[N:] == 0).all() and (shift[N:] == 0).all()


# ------------------------------------------------------- 3. BN + activation backward
def _act_out(act, M, N, g):
    """Activation outputs (the BN input) in the activation's range, fp32."""
    if act == "sigmoid":
        return torch.rand(M, N, generator=g)
    if act == "tanh":
        return torch.rand(M, N, generator=g) * 2 - 1
    return torch.randn(M, N, generator=g) + 0.3


def _act_grad64(a, act):
    if act == "leakyrelu":
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    if act == "relu":
        return (a > 0).to(a.dtype)
    if act == "sigmoid":
        return a * (1 - a)
    return 1 - a * a


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("M,N", PAIRS)
def test_bn_act_bwd_matches_float64(M, N, dtype, act):
    """mmad_bn_act_bwd (bn_bwd_reduce_k + bn_bwd_apply_k) against the float64
    formula of tests/test_gpu_bn_apply.py at its bounds: dz within 2^-7 (bf16)
    or 1e-5 (fp32) of the column's largest |dz|, dgamma / dbeta rtol 1e-5 atol
    1e-4, db partials = per-slab column sums of the dz written."""
    dt, td = DTYPES[dtype]
    Mp, Np = pad(M), pad(N)
    g = _gen(M, N, _native.ACT[act], 13)
    a = _act_out(act, M, N, g).to(td)
    dy = torch.randn(M, N, generator=g).to(td)
    a64, dy64 = a.double(), dy.double()
    mean, rstd, gamma = torch.zeros(Np), torch.zeros(Np), torch.zeros(Np)
    mean[:N] = a64.mean(0).float()
    rstd[:N] = (1.0 / torch.sqrt(a64.var(0, unbiased=False) + 1e-5)).float()
    gamma[:N] = torch.rand(N, generator=g) + 0.5
    xh = (a64 - mean[:N].double()) * rstd[:N].double()
    sdy, sdx = dy64.sum(0), (dy64 * xh).sum(0)
    cf = gamma[:N].double() * rstd[:N].double() / M
    ref = _act_grad64(a64, act) * cf * (M * dy64 - sdy - xh * sdx)
    ws_bytes = int(_native.load().mmad_bn_act_bwd_ws(Mp, Np))
    assert ws_bytes % 8 == 0
    ws = torch.full((ws_bytes // 8 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    dz = torch.full((Mp, Np), NAN, dtype=td, device="cuda")
    dg = torch.full((Np,), NAN, device="cuda")
    db = torch.full((Np,), NAN, device="cuda")
    dbp = torch.full((Mp // 128 * Np + GUARD,), SENTINEL, device="cuda")
    dev = [t.cuda() for t in (_packed(M, N, dy, td), _packed(M, N, a, td), mean, rstd, gamma)]
    call("mmad_bn_act_bwd", dt, _native.ACT[act], SLOPE, M, N, Mp, Np, *(ptr(t) for t in dev), ptr(dz), ptr(dg),
         ptr(db), ptr(dbp), ptr(ws), stream_ptr())
    torch.cuda.synchronize()
    out, dg, db, dbp, ws = dz.cpu().double(), dg.cpu().double(), db.cpu().double(), dbp.cpu(), ws.cpu()
    assert (ws[ws_bytes // 8:] == SENTINEL).all() and (dbp[Mp // 128 * Np:] == SENTINEL).all()
    assert torch.allclose(db[:N], sdy, rtol=1e-5, atol=1e-4)
    assert torch.allclose(dg[:N], sdx, rtol=1e-5, atol=1e-4)
    assert (db[N:] == 0).all() and (dg[N:] == 0).all()
    assert torch.isfinite(out).all()
    assert (out[M:] == 0).all() and (out[:, N:] == 0).all()
    tol = 2.0 ** -7 if dtype == "bf16" else 1e-5
    scale = ref.abs().amax(0).clamp_min(1e-30)
    w = float(((out[:M, :N] - ref).abs() / scale).max()) / tol
    print(f"bn_act_bwd {dtype} {act} M={M} N={N}: dz err / bound {w:.4f}, "
          f"dbeta {float((db[:N] - sdy).abs().max()):.2e} dgamma {float((dg[:N] - sdx).abs().max()):.2e}")
    _record(f"bn_act_bwd_dz_{dtype}", w)
    assert w < 1.0
    want = out.view(Mp // 128, 128, Np).sum(1)
    got = dbp[:Mp // 128 * Np].double().view(Mp // 128, Np)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))


# ------------------------------------------------------- 4. activation backward + colsum
def _act_bwd_exact(dy, a, act):
    """dz as the kernel forms it: act'(a) and the product in fp32, one rounding
    to the dtype.  Returns the admissible results: tanh's 1 - a*a may be one
    fused multiply-add (one rounding) or two operations; they differ only
    where a*a is inexact in fp32 (fp32 operands)."""
    dy, a = dy.float(), a.float()
    if act in ("leakyrelu", "relu"):   # a product: dy * 0 keeps dy's sign on its zero
        lo = torch.tensor(SLOPE if act == "leakyrelu" else 0.0, dtype=torch.float32)
        return [dy * torch.where(a > 0, torch.ones_like(a), lo)]
    if act == "sigmoid":
        return [dy * (a * (1 - a))]
    return [dy * (1 - a * a), dy * (1 - a.double() * a.double()).float()]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("M,N", PAIRS + [(0, 65)])
def test_act_bwd_and_colsum(M, N, dtype, act):
    """dz = dy * act'(a) exactly, rows >= M zero (M = 0 included); the db
    partials and mmad_colsum(scale = 0.5) of them against float64 column sums
    of the dz written, within 1e-5 sum |dz|; colsum columns >= N are 0."""
    dt, td = DTYPES[dtype]
    Mp, Np = max(pad(M), 128), pad(N)
    g = _gen(M, N, _native.ACT[act], 17)
    # all Np columns carry data: the operator has no N
    a = _act_out(act, M, Np, g).to(td)
    dy = torch.randn(M, Np, generator=g).to(td)
    ap = torch.full((Mp, Np), ROW_SENTINEL, dtype=td)
    dyp = torch.full((Mp, Np), ROW_SENTINEL, dtype=td)
    ap[:M], dyp[:M] = a, dy
    dz = torch.full((Mp, Np), NAN, dtype=td, device="cuda")
    dbp = torch.full((Mp // 128 * Np + GUARD,), SENTINEL, device="cuda")
    cs = torch.full((Np + GUARD,), SENTINEL, device="cuda")
    dyd, adv = dyp.cuda(), ap.cuda()
    call("mmad_act_bwd", dt, _native.ACT[act], SLOPE, M, Mp, Np, ptr(dyd), ptr(adv), ptr(dz), ptr(dbp),
         stream_ptr())
    call("mmad_colsum", Mp // 128, N, Np, ptr(dbp), Np, 0.5, ptr(cs), stream_ptr())
    torch.cuda.synchronize()
    out, dbp, cs = dz.cpu(), dbp.cpu(), cs.cpu()
    ok = torch.zeros(M, Np, dtype=torch.bool)
    es = out.element_size()
    for cand in _act_bwd_exact(dy, a, act):
        ok |= _bits(out[:M]).view(M, Np, es).eq(_bits(cand.to(td)).view(M, Np, es)).all(-1)
    assert ok.all(), int((~ok).sum())
    assert (out[M:] == 0).all()
    n = Mp // 128 * Np
    assert (dbp[n:] == SENTINEL).all() and (cs[Np:] == SENTINEL).all()
    slabs = out.double().view(Mp // 128, 128, Np)
    want, mag = slabs.sum(1), slabs.abs().sum(1)
    err = (dbp[:n].double().view(Mp // 128, Np) - want).abs()
    w = _worst(err, 1e-5 * mag)
    _record(f"act_bwd_partials_{dtype}", w)
    assert (err <= 1e-5 * mag).all(), w
    err = (cs[:N].double() - 0.5 * want.sum(0)[:N]).abs()
    tol = 1e-5 * 0.5 * mag.sum(0)[:N]
    w2 = _worst(err, tol)
    print(f"act_bwd {dtype} {act} M={M} N={N}: partials err / bound {w:.4f}, colsum {w2:.4f}")
    _record(f"colsum_{dtype}", w2)
    assert (err <= tol).all(), w2
    assert (cs[N:Np] == 0).all()
