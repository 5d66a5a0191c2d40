"""mmad_group_sq on the GPU: the mean square of arbitrary column groups of an
fp32 matrix (NativeAE.group_sq), against float64 numpy, for bitwise
independence of a (row, group) from everything but the group's two bounds, for
the strict flag rule and for its refusals."""
import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native

pytestmark = pytest.mark.gpu

LDD, ROWS = 1760, 130
BOUNDS = {
    "fused": [0, 1024, 1536, 1600, 1728],                       # the fused HSR row
    "odd": [0, 1, 17, 64, 100, 1727],                           # width 1, unaligned, last column left out
    "head": [3, 1728],                                          # a misaligned start: the scalar head
    "g8": [5, 6, 70, 333, 334, 900, 1281, 1700, 1759],          # G = 8, groups inside one quad
}
SENTINEL = -3.0


@pytest.fixture(scope="module")
def nat():
    from icra2021_multimodal_ad_amd.engine import NativeAE
    return NativeAE([192, 64, 16], [16, 64, 192], dtype="f32", device="cuda:0")


@pytest.fixture(scope="module")
def data():
    """d [130][1760] fp32 on the device and, per bounds set, the float64
    reference [G][130] on the same fp32 values (computed once)."""
    rng = np.random.default_rng(20241)
    d = (rng.standard_normal((ROWS, LDD)) * rng.uniform(0.01, 3.0, (ROWS, 1))).astype(np.float32)
    sq = d.astype(np.float64) ** 2
    ref = {k: np.stack([sq[:, b[g]:b[g + 1]].sum(1) / (b[g + 1] - b[g]) for g in range(len(b) - 1)])
           for k, b in BOUNDS.items()}
    return torch.from_numpy(d).cuda(), ref


@pytest.mark.parametrize("name", list(BOUNDS))
@pytest.mark.parametrize("N", [1, 15, 16, 17, 64, 130])
def test_group_sq_against_float64(nat, data, N, name):
    """Every term is non-negative, so any fixed-order fp32 sum of w terms plus
    the squares and the division is within (w + 2) 2^-24 relative of the exact
    value: rtol = (w_g + 2) 2^-24 per group, atol = 0.  The output sits in a
    sentinel frame: one row and three columns more than the call may write."""
    d, ref = data
    b = BOUNDS[name]
    G = len(b) - 1
    out = torch.full((G + 1, N + 3), SENTINEL, device="cuda")
    got = nat.group_sq(d[:N], b, out=out)
    torch.cuda.synchronize()
    assert got is out
    assert (out[G] == SENTINEL).all() and (out[:, N:] == SENTINEL).all()
    got = out[:G, :N].double().cpu().numpy()
    want = ref[name][:, :N]
    for g in range(G):
        rtol = (b[g + 1] - b[g] + 2) * 2.0 ** -24
        err = np.abs(got[g] - want[g]) / want[g]
        print(f"{name} N={N} group {g} [{b[g]}, {b[g + 1]}): max rel err {err.max():.3e} (bound {rtol:.3e})")
        assert (np.abs(got[g] - want[g]) <= rtol * want[g]).all(), (g, err.max(), rtol)


@pytest.mark.parametrize("name", list(BOUNDS))
def test_a_row_and_group_depend_on_the_bounds_alone(nat, data, name):
    """Row i of the N = 130 call, the same row alone, the same row at other
    leading dimensions (1764: rows still 16-byte aligned; 1761 and 1763: rows
    at every 4-byte phase, the scalar-load path) and each group asked for alone
    (G = 1) are the same bits."""
    d, _ = data
    b = BOUNDS[name]
    G = len(b) - 1
    full = nat.group_sq(d, b)
    for i in (0, 1, 2, 77, 129):
        assert torch.equal(nat.group_sq(d[i:i + 1], b)[:, 0], full[:, i]), i
    for ldd in (1764, 1761, 1763):
        wide = torch.full((ROWS, ldd), 9.0, device="cuda")
        wide[:, :LDD] = d
        assert wide.stride(0) == ldd
        assert torch.equal(nat.group_sq(wide, b), full), ldd
    for g in range(G):
        assert torch.equal(nat.group_sq(d, b[g:g + 2])[0], full[g]), g
    assert torch.equal(nat.group_sq(d[3:20], b), full[:, 3:20])


def test_flags_follow_the_strict_rule(nat, data):
    d, _ = data
    b = BOUNDS["fused"]
    G, N = len(b) - 1, 64
    out = nat.group_sq(d[:N], b)
    # a threshold that IS a produced score (the bits read back): no flag there
    thr = out[:, 7].clone()
    flags = torch.full((G, N), 9, device="cuda", dtype=torch.uint8)
    out2 = nat.group_sq(d[:N], b, thresholds=thr, flags=flags)
    assert torch.equal(out2, out)
    assert (flags[:, 7] == 0).all()
    assert torch.equal(flags.bool(), out > thr[:, None]) and 0 < int(flags.sum()) < G * N
    # one ulp below: flagged
    below = torch.nextafter(thr, torch.zeros_like(thr))
    nat.group_sq(d[:N], b, thresholds=below, flags=flags)
    assert (flags[:, 7] == 1).all() and torch.equal(flags.bool(), out > below[:, None])
    # NaN flags nothing; no thresholds flag nothing
    nan = thr.clone()
    nan[1] = float("nan")
    nat.group_sq(d[:N], b, thresholds=nan, flags=flags)
    assert (flags[1] == 0).all() and torch.equal(flags.bool(), out > nan[:, None])
    flags.fill_(9)
    nat.group_sq(d[:N], b, flags=flags)
    assert (flags == 0).all()
    # flags=None writes no flag anywhere: the buffer of the calls above keeps its fill
    flags.fill_(9)
    assert torch.equal(nat.group_sq(d[:N], b, thresholds=thr), out)
    torch.cuda.synchronize()
    assert (flags == 9).all()


@pytest.mark.parametrize("bounds,word", [
    ([0, 1024, 512, 1728], "bounds not strictly ascending"),
    ([0, 1024, 1024, 1728], "bounds not strictly ascending"),
    ([0], "G=0 outside 1..8"),
    (list(range(0, 1000, 100)), "G=9 outside 1..8"),
    ([0, 1024, LDD + 1], "exceeds ldd"),
], ids=["descending", "equal", "G0", "G9", "past-ldd"])
def test_refusals_launch_nothing(nat, data, bounds, word):
    d, _ = data
    out = torch.full((9, 16), SENTINEL, device="cuda")
    with pytest.raises(_native.NativeError, match=word):
        nat.group_sq(d[:16], bounds, out=out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
