"""mmad_fc_rows_group against mmad_fc_rows16 / mmad_fc_rows64, member by
member and bit for bit: y, diff and rowsq with their canary frames (so the
zeroed rows >= M / columns >= N and everything left untouched compare too).
Every case runs at both row capacities; no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import FcRowsDesc, pad, ptr, stream_ptr

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
EINVAL, EUNSUPPORTED = -1, -2


class Member:
    """Operands of one member and two canary-framed output sets (single, group).
    score: the full score epilogue (ref + rowsq + diff + colw); plain: y only."""

    def __init__(self, rows, dtype, M, N, K, score=False, act=1, affine=True, seed=0):
        g = torch.Generator().manual_seed(1000 * N + 10 * K + M + seed)
        tdt = torch.float32 if dtype == F32 else torch.bfloat16
        self.rows, self.dtype, self.M, self.N, self.K = rows, dtype, M, N, K
        self.Kp, self.Np = pad(K), pad(N, 16)
        self.score, self.act = score, act
        rnd = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
        x = torch.zeros(rows, self.Kp)
        x[:M, :K] = rnd(M, K)
        w = torch.zeros(self.Np, self.Kp)
        w[:N, :K] = rnd(N, K) / K ** 0.5
        self.x, self.w = x.to(tdt).cuda(), w.to(tdt).cuda()
        vec = lambda v: torch.cat([v, torch.zeros(self.Np - N)]).cuda()    # noqa: E731
        self.bias = vec(0.1 * rnd(N))
        self.sc = vec(0.5 + torch.rand(N, generator=g)) if affine else None
        self.sh = vec(0.1 * rnd(N)) if affine else None
        self.ref = self.cw = None
        if score:
            self.ref = rnd(rows, self.Np).to(tdt).cuda()
            self.cw = vec(0.5 + torch.rand(N, generator=g))
        self.ld, self.c0 = N + 7, 3
        self.outs = [self._outputs(tdt), self._outputs(tdt)]

    def _outputs(self, tdt):
        return dict(y=torch.full((self.rows + 1, self.Np), 5.0, device="cuda", dtype=tdt),
                    diff=torch.full((self.rows + 2, self.ld), 77.0, device="cuda"),
                    rowsq=torch.full((self.Np // 16 + 1, self.rows), 55.0, device="cuda"))

    def args(self, which):
        """The arguments of mmad_fc_rows16 without the stream == the descriptor's fields."""
        o = self.outs[which]
        return [self.dtype, self.M, self.N, self.K, self.Np, self.Kp, ptr(self.x), ptr(self.w), ptr(self.bias),
                self.act, 0.2, ptr(self.sc), ptr(self.sh), ptr(o["y"]), ptr(self.ref), self.dtype, self.Np,
                ptr(o["diff"][0, self.c0:]) if self.score else None, self.ld, ptr(self.cw),
                ptr(o["rowsq"]) if self.score else None]

    def desc(self, d, **over):
        for (name, _), v in zip(FcRowsDesc._fields_, self.args(1)):
            setattr(d, name, v.value if isinstance(v, ctypes.c_void_p) else v)
        for k, v in over.items():
            setattr(d, k, v)

    def single(self):
        _native.call(f"mmad_fc_rows{self.rows}", *self.args(0), stream_ptr())

    def same(self):
        for k in ("y", "diff", "rowsq"):
            assert torch.equal(self.outs[0][k], self.outs[1][k]), (k, self.N, self.K, self.M)
        y = self.outs[1]["y"]
        assert (y[self.M:self.rows] == 0).all() and (y[:self.rows, self.N:] == 0).all() and (y[self.rows] == 5).all()
        assert (y[:self.M, :self.N] != 5).any()

    def untouched(self):
        o = self.outs[1]
        return bool((o["y"] == 5).all() and (o["diff"] == 77).all() and (o["rowsq"] == 55).all())


def group(rows, members, n=None, **over):
    """One mmad_fc_rows_group call over ``members`` (None: an empty member); returns its status."""
    d = (FcRowsDesc * max(len(members), 1))()
    for m, di in zip(members, d):
        if m is not None:
            m.desc(di)
    for k, v in over.items():
        setattr(d[0], k, v)
    rc = _native.load().mmad_fc_rows_group(rows, len(members) if n is None else n, d, stream_ptr())
    torch.cuda.synchronize()
    return rc


def check(rows, members):
    for m in members:
        if m is not None:
            m.single()
    assert group(rows, members) == 0, _native.last_error()
    for m in members:
        if m is not None:
            m.same()


ROWS = [16, 64]


@pytest.mark.parametrize("rows", ROWS)
def test_one_member(rows):
    check(rows, [Member(rows, F32, min(10, rows), 100, 200, score=True)])
    check(rows, [Member(rows, BF16, rows, 40, 130)])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_three_members_one_tile_beside_many(rows, dtype):
    """N = 16 / 100 / 1402 (1 / 7 / 88 tiles) with Kp = 128 / 256 / 1792: the
    first and last block of every member sit on a prefix-table edge."""
    B = 10 if rows == 16 else 37
    ms = [Member(rows, dtype, B, 16, 128), Member(rows, dtype, B, 100, 250, score=True),
          Member(rows, dtype, B, 1402, 1700)]
    assert [m.Kp for m in ms] == [128, 256, 1792] and [m.Np // 16 for m in ms] == [1, 7, 88]
    check(rows, ms)
    check(rows, ms[::-1])


@pytest.mark.parametrize("rows", ROWS)
def test_member_without_tiles(rows):
    """N == 0: the member owns no blocks -- first, in the middle and last."""
    a, b = Member(rows, F32, 5, 100, 128, score=True), Member(rows, F32, 5, 16, 300)
    check(rows, [None, a, None, b, None])


@pytest.mark.parametrize("rows", ROWS)
def test_mixed_element_types(rows):
    B = rows - 3
    check(rows, [Member(rows, F32, B, 100, 128, score=True), Member(rows, BF16, B, 52, 256, score=True),
                 Member(rows, F32, B, 16, 140), Member(rows, BF16, B, 200, 128)])


@pytest.mark.parametrize("rows", ROWS)
def test_score_epilogue_beside_plain(rows):
    check(rows, [Member(rows, F32, 9, 121, 156, score=True, act=0, affine=False), Member(rows, F32, 9, 121, 156)])


@pytest.mark.parametrize("rows", ROWS)
def test_row_edges(rows):
    """M = 1 and M = rows, alone and side by side (the launch rides the larger M's row tiles)."""
    for dtype in (F32, BF16):
        check(rows, [Member(rows, dtype, 1, 100, 128, score=True)])
        check(rows, [Member(rows, dtype, rows, 100, 128, score=True)])
        check(rows, [Member(rows, dtype, 1, 52, 256, score=True), Member(rows, dtype, rows, 100, 128, score=True),
                     Member(rows, dtype, min(17, rows), 16, 128)])


@pytest.mark.parametrize("rows", ROWS)
def test_all_eight_members(rows):
    assert _native.MAX_BANK == 8
    ms = [Member(rows, (F32, BF16)[i % 2], 1 + (5 * i) % rows, 16 + 23 * i, 100 + 60 * i, score=i % 3 == 0, seed=i)
          for i in range(8)]
    check(rows, ms)


@pytest.mark.parametrize("rows", ROWS)
def test_refusals_launch_nothing(rows):
    """n outside 1..8, rows other than 16 / 64, and every refusal of
    mmad_fc_rows16 / 64 on one member: MMAD_EINVAL (an activation without an
    epilogue: MMAD_EUNSUPPORTED, as the single form), every member's outputs
    untouched -- the good member beside the refused one too."""
    lib = _native.load()
    good = Member(rows, F32, 5, 100, 128, score=True)
    bad = Member(rows, F32, 5, 52, 200, score=True)
    plain = Member(rows, F32, 5, 52, 200)
    for n in (0, 9, -3):
        assert group(rows, [good], n=n) == EINVAL
    for r in (0, 8, 32, 128):
        assert group(r, [good]) == EINVAL
    cases = {
        "M = 0": dict(M=0), "M > rows": dict(M=rows + 1), "N > Np": dict(N=bad.Np + 1), "N negative": dict(N=-1),
        "Np not a multiple of 16": dict(Np=bad.Np + 8), "Kp not a multiple of 128": dict(Kp=bad.Kp + 64),
        "Kp = 0": dict(Kp=0, K=0), "K = 0": dict(K=0), "K > Kp": dict(K=bad.Kp + 1), "null x": dict(x=None),
        "null w": dict(w=None), "misaligned x": dict(x=bad.x.data_ptr() + 4), "misaligned w": dict(w=bad.w.data_ptr() + 8),
        "bn_scale alone": dict(bn_shift=None), "ref of another type": dict(ref_dtype=BF16),
        "ldref < N": dict(ldref=bad.N - 1), "lddiff < N": dict(lddiff=bad.N - 1), "dtype 2": dict(dtype=2),
        "dtype 7": dict(dtype=7), "ref without rowsq": dict(rowsq=None, diff=None, colw=None),
        "neither y nor rowsq": dict(y=None, rowsq=None, ref=None, diff=None, colw=None),
    }
    for what, over in cases.items():
        d = (FcRowsDesc * 2)()
        good.desc(d[0])
        bad.desc(d[1], **over)
        assert lib.mmad_fc_rows_group(rows, 2, d, stream_ptr()) == EINVAL, what
        assert len(_native.last_error()) > 0
        # the single form refuses the same member
        a = bad.args(1)
        for k, v in over.items():
            a[[f for f, _ in FcRowsDesc._fields_].index(k)] = v
        assert getattr(lib, f"mmad_fc_rows{rows}")(*a, stream_ptr()) == EINVAL, what
    d = (FcRowsDesc * 2)()
    good.desc(d[0])
    plain.desc(d[1], act=5)
    assert lib.mmad_fc_rows_group(rows, 2, d, stream_ptr()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert good.untouched() and bad.untouched() and plain.untouched()
    check(rows, [good, bad, plain])                    # and the same members are fine as they are
