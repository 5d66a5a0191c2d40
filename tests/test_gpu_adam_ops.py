"""The flat Adam kernel (csrc/mmad_ops_adam.hip, adam_k) and the executor's
range form (mmad_ae_adam_range) through the public C-ABI, at the sizes where
adam_k changes path: the float4 body, the scalar tail of a buffer whose length
is no multiple of 4, and a bf16 shadow that is absent, empty, whole, ends on a
quad boundary or ends inside a quad.

    mmad_adam            m / v bit-equal to torch's CPU single-tensor step, p to the
                         bounds of test_public_adam_matches_torch_cpu_adam, all within
                         1e-6 of tests/adam_ref.py's float64 step; the shadow is
                         bf16(p) up to n_shadow and untouched from there on
    mmad_ae_adam_range   the ranges of a partition give mmad_ae_adam's bits
                         (include/mmad.h), in any order, on an fp32 and a bf16 handle

Every buffer carries guard elements in front of and behind the n the kernel
is given; they hold a sentinel and must keep it."""
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr
from tests import adam_ref as A

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
# (betas, step, lr) of test_public_adam_matches_torch_cpu_adam; tests/test_adam_reference.py runs the same betas
CONFIGS = [((0.9, 0.999), 1, 1e-3), ((0.9, 0.999), 3, 1e-3), ((0.8, 0.95), 2, 3e-4)]
EPS = 1e-8
GUARD = 8            # elements in front of and behind every buffer (32 bytes fp32, 16 bytes bf16)
SENTINEL = -1234.5
SHADOW_FILL = 7.0    # exact in bf16; no bf16(p) of these tests comes near it


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _guarded(vals, fill=SENTINEL, dtype=torch.float32):
    """[GUARD | vals | GUARD] on the device; the body's address keeps the
    allocation's 16-byte alignment."""
    n = vals.numel()
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype)
    buf[GUARD:GUARD + n] = vals.to(dtype)
    dev = buf.cuda()
    assert dev[GUARD:].data_ptr() % 16 == 0
    return dev


def _shadow_cases(n):
    """None = a null shadow pointer; 0; n; the largest multiple of 4 below n;
    and, from n = 5 on, the three lengths that end inside the last quad that
    lies wholly below n (adam_k's third branch)."""
    cases = [None, 0, n, (n - 1) // 4 * 4]
    if n >= 5:
        base = (n // 4 - 1) * 4
        assert base + 4 <= n
        cases += [base + 1, base + 2, base + 3]
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


def _state(n, step, seed):
    g_ = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g_) * 0.05
    g = torch.randn(n, generator=g_) * 1e-2
    m0 = torch.randn(n, generator=g_) * 1e-3 if step > 1 else torch.zeros(n)
    v0 = torch.rand(n, generator=g_) * 1e-5 if step > 1 else torch.zeros(n)
    return p0, g, m0, v0


def _run_adam(state, betas, step, lr, n_shadow):
    """mmad_adam on guarded copies of the state; returns the host copies of the
    whole buffers (p, g, m, v, shadow)."""
    n = state[0].numel()
    step_size, bc2_sqrt = A.adam_consts(lr, betas, step)
    dp, dg, dm, dv = (_guarded(t) for t in state)
    sh = _guarded(torch.full((n,), SHADOW_FILL), fill=SHADOW_FILL, dtype=torch.bfloat16)
    body = lambda t: t[GUARD:]   # noqa: E731
    call("mmad_adam", n, ptr(body(dp)), ptr(body(dg)), ptr(body(dm)), ptr(body(dv)), betas[0], betas[1], EPS,
         step_size, bc2_sqrt, ptr(body(sh)) if n_shadow is not None else None,
         n_shadow if n_shadow is not None else 0, stream_ptr())
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (dp, dg, dm, dv, sh))


def _check_against_references(state, betas, step, lr, got, share):
    """m / v bit-equal to torch's CPU step, p within 2^-21 max(|p0|, |p|) of it
    (and bit-equal on >= 95 % of the elements where `share`), p / m / v within
    1e-6 relative (max-norm) of the float64 step."""
    p0, g, m0, v0 = state
    pt, mt, vt = A.torch_cpu_adam(p0, g, m0, v0, lr=lr, betas=betas, eps=EPS, step=step)
    pd, md, vd = A.adam_step_f64(p0, g, m0, v0, lr=lr, betas=betas, eps=EPS, step=step)
    p, m, v = got
    assert torch.equal(_bits(m), _bits(mt))
    assert torch.equal(_bits(v), _bits(vt))
    pg, pt = p.double(), pt.double()
    scale = torch.maximum(p0.double().abs(), pt.abs())
    assert bool(((pg - pt).abs() <= scale * 2.0 ** -21).all())
    if share:
        assert float((pg == pt).double().mean()) >= 0.95
    for name, a, ref in (("p", p, pd), ("m", m, md), ("v", v, vd)):
        err, mag = float((a.double() - ref).abs().max()), float(ref.abs().max())
        assert err <= 1e-6 * mag, (name, err, mag)


@pytest.mark.parametrize("betas,step,lr", CONFIGS)
@pytest.mark.parametrize("n", SIZES)
def test_adam_sizes_and_shadow_lengths(n, betas, step, lr):
    state = _state(n, step, seed=1000 * step + n)
    ref_bits = None
    for n_shadow in _shadow_cases(n):
        what = f"n={n} n_shadow={n_shadow}"
        p, g, m, v, sh = _run_adam(state, betas, step, lr, n_shadow)
        body = slice(GUARD, GUARD + n)
        for name, t, src in (("p", p, None), ("g", g, state[1]), ("m", m, None), ("v", v, None)):
            assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + n:] == SENTINEL).all(), (what, name)
            if src is not None:
                assert torch.equal(_bits(t[body]), _bits(src)), (what, name)
        got = (p[body], m[body], v[body])
        if ref_bits is None:
            _check_against_references(state, betas, step, lr, got, share=n >= 1023)
            ref_bits = [_bits(t).clone() for t in got]
        else:   # the shadow's length changes nothing in p / m / v
            for t, r in zip(got, ref_bits):
                assert torch.equal(_bits(t), r), what
        ns = n_shadow or 0
        shb = sh[body]
        assert torch.equal(_bits(shb[:ns]), _bits(got[0][:ns].bfloat16())), what
        assert (shb[ns:] == SHADOW_FILL).all(), what
        assert (sh[:GUARD] == SHADOW_FILL).all() and (sh[GUARD + n:] == SHADOW_FILL).all(), what


def test_adam_edge_values():
    """n = 1025, step 2: blocks (inside the float4 body, and the scalar tail
    element) with g = 0 and v0 = 0 (the denominator is eps alone), g = 1e-30
    (g^2 underflows), |g| = 1e3 from m0 = 0, and p0 = 0."""
    n, (betas, step, lr) = 1025, CONFIGS[2]
    p0, g, m0, v0 = _state(n, step, seed=77)
    g[0:64] = 0.0
    v0[0:64] = 0.0
    m0[32:64] = 0.0                                     # ... and with m0 = 0: the update is 0 / eps
    g[64:128] = 1e-30
    g[128:192] = torch.where(torch.arange(64) % 2 == 0, 1e3, -1e3)
    m0[128:192] = 0.0
    p0[192:256] = 0.0
    g[1021:1025], v0[1021:1025] = 0.0, 0.0              # the last quad's 3 elements and the tail element
    g[1017:1021] = 1e-30
    p0[1015:1025] = 0.0
    assert float(torch.tensor(1e-30) * torch.tensor(1e-30)) == 0.0
    state = (p0, g, m0, v0)
    p, g_out, m, v, sh = _run_adam(state, betas, step, lr, n)
    body = slice(GUARD, GUARD + n)
    got = (p[body], m[body], v[body])
    for t in got:
        assert torch.isfinite(t).all()
    _check_against_references(state, betas, step, lr, got, share=True)
    assert torch.equal(_bits(g_out[body]), _bits(g))
    assert torch.equal(_bits(sh[body]), _bits(got[0].bfloat16()))
    for t in (p, g_out, m, v):
        assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + n:] == SENTINEL).all()


def test_adam_refusals_leave_the_buffers_alone():
    """n_shadow > n, n < 0 and a p that is 4 bytes off 16-byte alignment return
    MMAD_EINVAL; n = 0 returns MMAD_OK; none of them writes anything."""
    n = 64
    lib = _native.load()
    state = _state(n, 2, seed=5)
    dp, dg, dm, dv = (_guarded(t) for t in state)
    sh = _guarded(torch.full((n,), SHADOW_FILL), fill=SHADOW_FILL, dtype=torch.bfloat16)
    before = [_bits(t.cpu()).clone() for t in (dp, dg, dm, dv, sh)]
    step_size, bc2_sqrt = A.adam_consts(1e-3, (0.9, 0.999), 2)

    def run(n_arg, n_shadow, p_off=0):
        st = lib.mmad_adam(n_arg, ptr(dp[GUARD + p_off:]), ptr(dg[GUARD:]), ptr(dm[GUARD:]), ptr(dv[GUARD:]),
                           0.9, 0.999, EPS, step_size, bc2_sqrt, ptr(sh[GUARD:]), n_shadow, stream_ptr())
        torch.cuda.synchronize()
        for t, b in zip((dp, dg, dm, dv, sh), before):
            assert torch.equal(_bits(t.cpu()), b)
        return st

    assert run(n, n + 1) == _native.MMAD_EINVAL
    assert run(-1, 0) == _native.MMAD_EINVAL
    assert run(n - 4, 0, p_off=1) == _native.MMAD_EINVAL
    assert run(0, 0) == _native.MMAD_OK


# ------------------------------------------------------------ mmad_ae_adam_range
ENC, DEC = [70, 33, 9], [9, 33, 70]
STEP, LR, BETAS = 3, 1e-3, (0.9, 0.999)
STATE = ("params", "grads", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module", params=["f32", "bf16"])
def handle(request):
    """A 70 -> 33 -> 9 -> 33 -> 70 executor handle with random parameters,
    gradients and moments over the whole flat buffers (Adam is elementwise: it
    does not know the padding), the shadow filled with a sentinel, and the
    one-shot mmad_ae_adam(step 3) result from that state."""
    from icra2021_multimodal_ad_amd.engine import NativeAE
    nat = NativeAE(ENC, DEC, dtype=request.param, device="cuda:0")
    assert nat.n_weight % 4 == 0 and 0 < nat.n_weight < nat.n_params
    g_ = torch.Generator().manual_seed(31)
    n = nat.n_params
    init = {"params": torch.randn(n, generator=g_) * 0.05, "grads": torch.randn(n, generator=g_) * 1e-2,
            "exp_avg": torch.randn(n, generator=g_) * 1e-3, "exp_avg_sq": torch.rand(n, generator=g_) * 1e-5}
    if nat._shadow_buf is not None:
        init["_shadow_buf"] = torch.full((nat._shadow_buf.numel(),), SHADOW_FILL, dtype=torch.bfloat16)
    _restore(nat, init)
    nat.adam(lr=LR, betas=BETAS, eps=EPS, step=STEP)
    torch.cuda.synchronize()
    one_shot = _snapshot(nat)
    assert not torch.equal(one_shot["params"], init["params"])
    return nat, init, one_shot


def _snapshot(nat):
    torch.cuda.synchronize()
    return {k: getattr(nat, k).cpu().clone() for k in STATE + ("_shadow_buf",) if getattr(nat, k) is not None}


def _restore(nat, snap):
    for k, t in snap.items():
        getattr(nat, k).copy_(t)
    torch.cuda.synchronize()


def _shadow_base(nat):
    """offset in _shadow_buf of the shadow the handle writes (the first of a pair, or the second)"""
    return (nat.shadow.data_ptr() - nat._shadow_buf.data_ptr()) // 2


def _partitions(nat):
    nw, n = nat.n_weight, nat.n_params
    # (a) dist.py's exchange: the dW buckets, then [n_weight, n_params)
    plan = [(off, ln) for off, ln, _ in nat.dw_plan()] + [(nw, n - nw)]
    # (b) cuts at multiples of 4; [nw - 8, nw + 36) straddles the end of the weights
    cuts = [0, 4, 1004, 40000, nw - 8, nw + 36, nw + 40, n - 4, n]
    assert all(c % 4 == 0 for c in cuts) and cuts == sorted(cuts)
    arbitrary = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
    # (c) backwards, a zero-length range among them
    cuts = [0, 20000, nw - 128, nw + 256, n]
    backwards = [(a, b - a) for a, b in zip(cuts, cuts[1:])][::-1]
    backwards.insert(2, (40000, 0))
    return {"dw_plan": plan, "arbitrary": arbitrary, "backwards": backwards}


@pytest.mark.parametrize("which", ["dw_plan", "arbitrary", "backwards"])
def test_adam_range_partition_gives_adam_bits(handle, which):
    nat, init, one_shot = handle
    ranges = _partitions(nat)[which]
    covered = torch.zeros(nat.n_params, dtype=torch.int32)
    for off, ln in ranges:
        covered[off:off + ln] += 1
    assert (covered == 1).all(), "not a partition"
    _restore(nat, init)
    for off, ln in ranges:
        nat.adam_range(off, ln, lr=LR, betas=BETAS, eps=EPS, step=STEP)
    got = _snapshot(nat)
    for k in STATE:
        assert torch.equal(_bits(got[k]), _bits(one_shot[k])), k
    if nat.dtype_name == "bf16":
        assert torch.equal(_bits(got["_shadow_buf"]), _bits(one_shot["_shadow_buf"]))
        b, nw = _shadow_base(nat), nat.n_weight
        assert torch.equal(_bits(got["_shadow_buf"][b:b + nw]), _bits(got["params"][:nw].bfloat16()))


def test_adam_range_writes_only_its_range(handle):
    """One range that straddles n_weight: p / m / v change inside it only, the
    gradients nowhere, the shadow only in [off, n_weight)."""
    nat, init, one_shot = handle
    nw = nat.n_weight
    for off, ln in [(nw - 8, 44), (1004, 36), (nw, 12)]:
        _restore(nat, init)
        nat.adam_range(off, ln, lr=LR, betas=BETAS, eps=EPS, step=STEP)
        got = _snapshot(nat)
        assert torch.equal(_bits(got["grads"]), _bits(init["grads"]))
        for k in ("params", "exp_avg", "exp_avg_sq"):
            want = init[k].clone()
            want[off:off + ln] = one_shot[k][off:off + ln]
            assert torch.equal(_bits(got[k]), _bits(want)), (k, off, ln)
        if nat.dtype_name == "bf16":
            b = _shadow_base(nat)
            want = init["_shadow_buf"].clone()
            hi = min(off + ln, nw)
            if hi > off:
                want[b + off:b + hi] = one_shot["params"][off:hi].bfloat16()
            assert torch.equal(_bits(got["_shadow_buf"]), _bits(want)), (off, ln)


def test_adam_range_refusals_leave_the_state_alone(handle):
    nat, init, _ = handle
    _restore(nat, init)
    lib = _native.load()
    n = nat.n_params
    for step, off, ln in [(STEP, 2, 8), (STEP, n - 4, 8), (0, 0, 8)]:
        st = lib.mmad_ae_adam_range(nat._h, LR, BETAS[0], BETAS[1], EPS, step, off, ln, stream_ptr())
        assert st == _native.MMAD_EINVAL, (step, off, ln)
    got = _snapshot(nat)
    for k, t in init.items():
        assert torch.equal(_bits(got[k]), _bits(t)), k
