"""The references the split-bf16 GEMM matrix compares with (tests/x3_ref.py),
checked against each other on the CPU, on the exact operands of
tests/test_gpu_x3_matrix.py: the plane pair represents its fp32 value to
2^-17, the three-product reference P3 lies within 3 * 2^-18 D of the true
product T for every activation and affine (so a kernel that computes P3 to the
fp32 bar can meet the T bar), and the single-plane bf16 product does not."""
import pytest
import torch

from tests import x3_ref as R

ACTS = [R.ACT_NONE, R.ACT_LEAKY, R.ACT_RELU, R.ACT_SIGMOID, R.ACT_TANH]
PROBLEMS = {"main": R.MAIN, "mini": R.MINI}


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_planes_represent_the_operand(name):
    """hi + lo is within 2^-17 |v| of v, zero stays zero in both planes, and
    the operands are normal fp32 numbers (no denormal residual is needed)."""
    p = R.problem(**PROBLEMS[name])
    M, N, K = p.dims[:3]
    for v, pl, rows in ((p.x, p.xp, M), (p.w, p.wp, N)):
        back = pl[0].double() + pl[1].double()
        assert ((back - v.double()).abs() <= R.PLANE_REL * v.double().abs()).all()
        assert (pl[:, rows:, :] == 0).all() and (pl[:, :, K:] == 0).all()
        valid = v[:rows, :K]
        assert (valid.abs() >= torch.finfo(torch.float32).tiny).all()
        assert torch.equal(pl[0], v.bfloat16())


@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("act", ACTS, ids=[R.ACT_NAME[a] for a in ACTS])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_three_products_meet_the_true_product_bar(name, act, affine):
    """|P3 - T| <= 3 * 2^-18 D elementwise, D carried through the affine."""
    p = R.problem(**PROBLEMS[name])
    err = (p.y("p3", act, affine) - p.y("t", act, affine)).abs()
    bound = R.T_REL * p.dy(affine)
    ratio = float((err / bound).max())
    print(f"x3 reference {name} {R.ACT_NAME[act]} affine={affine}: |P3 - T| / (3 2^-18 D) = {ratio:.3f}")
    assert (err <= bound).all(), ratio


@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("act", ACTS, ids=[R.ACT_NAME[a] for a in ACTS])
def test_single_plane_product_misses_the_bar(act, affine):
    """Ah.Bh^T alone (what the bf16 path computes) exceeds the whole T bar,
    fp32 term included: the bar tells the three products from one."""
    p = R.problem(**R.MAIN)
    ref = p.y("t", act, affine)
    err = (p.y("hh", act, affine) - ref).abs()
    ratio = float((err / R.t_bound(ref, p.dy(affine), stored=True)).max())
    print(f"x3 reference main {R.ACT_NAME[act]} affine={affine}: single plane error / bar = {ratio:.1f}")
    assert ratio > 1.0
