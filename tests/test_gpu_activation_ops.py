"""The standalone activations (csrc/mmad_ops_act.hip) through
mmad_activation_fwd / mmad_activation_bwd, all eight (none, relu, leakyrelu
0.2, sigmoid, tanh, logsigmoid, softmax, logsoftmax), against float64 torch at
rtol 1e-5, atol 1e-6 (test_standalone_activation_matches_torch's), where the
kernels index differently or leave the middle of their range:

    rows M of 1 / 3 / 4 / 5 (softmax puts four rows in a block, a wave per row),
    widths N of 1 / 63 / 64 / 65 / 129 / 1000 (one lane of a wave, a wave less
    one, a whole wave, a wave and one more, ...);
    ld = N, ld = N + 3 everywhere, and a different ld on every operand: the
    gap columns hold a sentinel and keep it;
    y aliasing x, dx aliasing dy: the out-of-place bits;
    |x| up to 1e4: sigmoid / tanh / logsigmoid where they saturate, softmax of
    shifted, dominated and constant rows."""
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu

SLOPE = 0.2
ACT = {"none": 0, "leakyrelu": 1, "relu": 2, "sigmoid": 3, "tanh": 4, "logsigmoid": 5, "softmax": 6,
       "logsoftmax": 7}   # MMAD_ACT_* (include/mmad.h)
ELEMENTWISE = ["none", "relu", "leakyrelu", "sigmoid", "tanh", "logsigmoid"]
ROWWISE = ["softmax", "logsoftmax"]
ROWS = [1, 3, 4, 5]
WIDTHS = [1, 63, 64, 65, 129, 1000]
RTOL, ATOL = 1e-5, 1e-6
SENTINEL = -1234.5
GUARD = 8


def _ref(act, x):
    """the activation on a float64 tensor"""
    F = torch.nn.functional
    return {"none": lambda t: t * 1.0, "relu": torch.relu, "leakyrelu": lambda t: F.leaky_relu(t, SLOPE),
            "sigmoid": torch.sigmoid, "tanh": torch.tanh, "logsigmoid": F.logsigmoid,
            "softmax": lambda t: torch.softmax(t, -1), "logsoftmax": lambda t: torch.log_softmax(t, -1)}[act](x)


def _ref_fwd_bwd(act, x, dy):
    """float64 forward and autograd backward"""
    xr = x.double().requires_grad_(True)
    yr = _ref(act, xr)
    yr.backward(dy.double())
    return yr.detach(), xr.grad


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _strided(vals, ld):
    """vals [M][N] in a sentinel-filled [M * ld + GUARD] device buffer with row stride ld"""
    M, N = vals.shape
    buf = torch.full((M * ld + GUARD,), SENTINEL)
    buf[:M * ld].view(M, ld)[:, :N] = vals
    return buf.cuda()


def _body(buf, M, N, ld):
    """(the [M][N] values, True if every other element of the buffer kept the sentinel)"""
    buf = buf.cpu()
    mat = buf[:M * ld].view(M, ld)
    return mat[:, :N].clone(), bool((mat[:, N:] == SENTINEL).all() and (buf[M * ld:] == SENTINEL).all())


def _fwd(act, x, ldx, ldy, in_place=False):
    M, N = x.shape
    xd = _strided(x, ldx)
    yd = xd if in_place else _strided(torch.full((M, N), float("nan")), ldy)
    call("mmad_activation_fwd", ACT[act], SLOPE, M, N, ptr(xd), ldx, ptr(yd), ldx if in_place else ldy,
         stream_ptr())
    torch.cuda.synchronize()
    y, clean = _body(yd, M, N, ldx if in_place else ldy)
    assert clean, "forward wrote outside [M][N]"
    if not in_place:   # the input is read only
        x_after, clean = _body(xd, M, N, ldx)
        assert clean and torch.equal(_bits(x_after), _bits(x))
    return y


def _bwd(act, y, dy, ldy, lddy, lddx, in_place=False):
    M, N = y.shape
    yd, dyd = _strided(y, ldy), _strided(dy, lddy)
    dxd = dyd if in_place else _strided(torch.full((M, N), float("nan")), lddx)
    call("mmad_activation_bwd", ACT[act], SLOPE, M, N, ptr(yd), ldy, ptr(dyd), lddy, ptr(dxd),
         lddy if in_place else lddx, stream_ptr())
    torch.cuda.synchronize()
    dx, clean = _body(dxd, M, N, lddy if in_place else lddx)
    assert clean, "backward wrote outside [M][N]"
    y_after, clean = _body(yd, M, N, ldy)
    assert clean and torch.equal(_bits(y_after), _bits(y))
    return dx


def _close(got, ref):
    return torch.allclose(got.double(), ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("act", list(ACT))
def test_activation_shapes_strides_and_aliasing(act, N):
    for M in ROWS:
        g = torch.Generator().manual_seed(1000 * ACT[act] + 10 * N + M)
        x = torch.randn(M, N, generator=g) * 4.0
        dy = torch.randn(M, N, generator=g)
        y_ref, dx_ref = _ref_fwd_bwd(act, x, dy)
        # (ldx, ldy of the forward = ldy of the backward, lddy, lddx)
        lds = [(N, N, N, N), (N + 3, N + 3, N + 3, N + 3), (N + 3, N + 5, N + 1, N + 2)]
        ys, dxs = [], []
        for ldx, ldy, lddy, lddx in lds:
            what = (M, N, ldx, ldy, lddy, lddx)
            y = _fwd(act, x, ldx, ldy)
            assert _close(y, y_ref), what
            dx = _bwd(act, y, dy, ldy, lddy, lddx)
            assert _close(dx, dx_ref), what
            ys.append(y)
            dxs.append(dx)
        # the strides change no bit, and neither does running in place
        for y, dx in zip(ys[1:], dxs[1:]):
            assert torch.equal(_bits(y), _bits(ys[0])) and torch.equal(_bits(dx), _bits(dxs[0]))
        for ld in (N, N + 3):
            assert torch.equal(_bits(_fwd(act, x, ld, ld, in_place=True)), _bits(ys[0])), (M, N, ld)
            assert torch.equal(_bits(_bwd(act, ys[0], dy, ld, ld, ld, in_place=True)), _bits(dxs[0])), (M, N, ld)
        if act == "softmax":
            assert ((ys[0].double().sum(-1) - 1.0).abs() <= N * 2.0 ** -23).all()


@pytest.mark.parametrize("act", ELEMENTWISE)
def test_elementwise_saturation(act):
    """+-0, +-1e-30, +-30, +-90, +-1e4: finite, within tolerance of float64
    (forward, and backward with dy = 1 and a random dy); logsigmoid(-1e4) =
    -1e4 and logsigmoid(1e4) = 0 exactly; sigmoid in [0, 1], tanh in [-1, 1]."""
    vals = [0.0, 1e-30, 30.0, 90.0, 1e4]
    x = torch.tensor([[s * v for v in vals for s in (1.0, -1.0)]], dtype=torch.float32)
    N = x.shape[1]
    y = _fwd(act, x, N, N)
    assert torch.isfinite(y).all()
    for dy in (torch.ones(1, N), torch.randn(1, N, generator=torch.Generator().manual_seed(3))):
        y_ref, dx_ref = _ref_fwd_bwd(act, x, dy)
        assert _close(y, y_ref), (y, y_ref)
        dx = _bwd(act, y, dy, N, N, N)
        assert torch.isfinite(dx).all()
        assert _close(dx, dx_ref), (dx, dx_ref)
    at = {float(v): float(o) for v, o in zip(x[0], y[0])}
    if act == "logsigmoid":
        assert at[-1e4] == -1e4 and at[1e4] == 0.0
    if act == "sigmoid":
        assert ((y >= 0.0) & (y <= 1.0)).all() and at[1e4] == 1.0 and at[-1e4] == 0.0
    if act == "tanh":
        assert ((y >= -1.0) & (y <= 1.0)).all() and at[1e4] == 1.0 and at[-1e4] == -1.0


@pytest.mark.parametrize("N", [1, 63, 65, 1000])
@pytest.mark.parametrize("act", ROWWISE)
def test_softmax_stability(act, N):
    """Rows of multiples of 2^-8 in [-16, 16) (so that row + 1e4 is exact in
    fp32): the row shifted by 1e4 gives the unshifted row's output; a row with
    one entry 200 above the rest gives softmax exactly 1 there (0 elsewhere)
    and a finite logsoftmax; a constant row gives 1 / N in every entry."""
    g = torch.Generator().manual_seed(N)
    base = torch.randint(-4096, 4096, (1, N), generator=g).float() / 256.0
    shifted = base + 1e4
    assert torch.equal((shifted.double() - 1e4).float(), base)
    peak = base.clone()
    j = N // 2
    peak[0, j] = float(base.max()) + 200.0
    const = torch.full((1, N), 2.75)
    x = torch.cat([base, shifted, peak, const, -1e4 + const])
    y = _fwd(act, x, N + 3, N + 1)
    assert torch.isfinite(y).all()
    assert _close(y, _ref(act, x.double()))
    assert _close(y[1], y[0].double())
    if act == "softmax":
        assert float(y[2, j]) == 1.0 and float(y[2].sum()) == 1.0
        for r in (3, 4):
            assert _close(y[r], torch.full((N,), 1.0 / N, dtype=torch.float64))
    else:
        assert float(y[2, j]) == 0.0
        for r in (3, 4):
            assert _close(y[r], -torch.log(torch.full((N,), float(N), dtype=torch.float64)))
    for r in (3, 4):   # every lane of the wave holds the same sum
        assert (y[r] == y[r, 0]).all()
    assert ((torch.softmax(x.double(), -1).sum(-1) - 1.0).abs() < 1e-12).all()
    if act == "softmax":
        assert ((y.double().sum(-1) - 1.0).abs() <= N * 2.0 ** -23).all()


def test_degenerate_sizes_and_refusals():
    """M = 0 or N = 0 with null pointers is MMAD_OK; ld < N and an act outside
    the enum are MMAD_EINVAL and write nothing."""
    lib = _native.load()
    s = stream_ptr()
    for M, N in ((0, 5), (5, 0), (0, 0)):
        for act in (ACT["tanh"], ACT["softmax"]):
            assert lib.mmad_activation_fwd(act, SLOPE, M, N, None, N, None, N, s) == _native.MMAD_OK
            assert lib.mmad_activation_bwd(act, SLOPE, M, N, None, N, None, N, None, N, s) == _native.MMAD_OK
    M, N = 3, 8
    x = torch.randn(M, N, generator=torch.Generator().manual_seed(1))
    bufs = [_strided(x, N) for _ in range(3)]
    before = [_bits(b.cpu()).clone() for b in bufs]
    a, b, c = (ptr(t) for t in bufs)
    E = _native.MMAD_EINVAL
    for act in (ACT["relu"], ACT["logsoftmax"]):
        assert lib.mmad_activation_fwd(act, SLOPE, M, N, a, N - 1, b, N, s) == E
        assert lib.mmad_activation_fwd(act, SLOPE, M, N, a, N, b, N - 1, s) == E
        assert lib.mmad_activation_bwd(act, SLOPE, M, N, a, N - 1, b, N, c, N, s) == E
        assert lib.mmad_activation_bwd(act, SLOPE, M, N, a, N, b, N - 1, c, N, s) == E
        assert lib.mmad_activation_bwd(act, SLOPE, M, N, a, N, b, N, c, N - 1, s) == E
    for act in (-1, 8):
        assert lib.mmad_activation_fwd(act, SLOPE, M, N, a, N, b, N, s) == E
        assert lib.mmad_activation_bwd(act, SLOPE, M, N, a, N, b, N, c, N, s) == E
    torch.cuda.synchronize()
    for t, bits in zip(bufs, before):
        assert torch.equal(_bits(t.cpu()), bits)
