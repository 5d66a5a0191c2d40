"""The split-bf16 ("x3", MMAD_BF16X3) GEMM of csrc/mmad_gemm_x3.hip and the x3
form of the VIB waist, through the public C-ABI, against the float64
references of tests/x3_ref.py (bars and their derivation there; none comes
from the kernel).  tests/test_gpu_gemm_matrix.py walks tile x epilogue for
fp32 and bf16; this is the same walk for the one kernel it does not reach.

  1. the matrix at one masked problem (512^3 padded, M = 400, N = 300,
     K = 489) and at the smallest one (one tile, two K stages, M = 1, N = 3,
     K = 1): FWD with every activation x affine against both references;
     SCORE with the fp32 reference's padding NaN, the diff at ld_diff = N + 5
     inside a sentinel frame, rowsq per 128-column group (also against
     float64 sums of the returned diff: the reduction alone); the stored
     planes bit for bit hi = RNE(v), lo = RNE(v - hi) of the epilogue's fp32
     value; the NAP form; every call twice with equal bits;
  2. the tile order (x_tile: XCD interleave, groups of group_m row tiles with
     a shorter last group) on the smallest grids with more than 8 tiles, a
     tile count that is no multiple of 8 and tiles_m % group_m != 0, outputs
     pre-filled with NaN so that a tile left out shows, and the same bits for
     every group_m;
  3. M, N, K at and around the tile and K-stage sizes;
  4. mmad_vib_reparam_fwd(MMAD_BF16X3, deterministic): a copy of mu on both
     planes, the lo plane at roundup(B, 128) * ld_enc.

Operands are packed by torch on the host (tests/x3_ref.py: planes_of), so the
kernel reads exactly the planes the references are formed from.  The worst
error / bound per check goes to $MMAD_RECORD_DIR/x3_matrix.json (default
test_records/); the run quoted in DESIGN.md is in profiles/x3_matrix_tests.md."""
import json
import os

import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr
from tests import x3_ref as R

pytestmark = pytest.mark.gpu

X3 = _native.BF16X3
SLOPE = R.SLOPE
SENTINEL = 12345.0
NAN = float("nan")
ACTS = [R.ACT_NONE, R.ACT_LEAKY, R.ACT_RELU, R.ACT_SIGMOID, R.ACT_TANH]
ACT_IDS = [R.ACT_NAME[a] for a in ACTS]

_REC = {}


def worse(a, b):
    """the larger of two error / bound ratios; a NaN wins and stays"""
    return a if a != a or a >= b else b


def _record(key, value):
    new = worse(_REC.get(key, 0.0), float(value))
    if key not in _REC or new != _REC[key]:
        _REC[key] = new
        out_dir = os.environ.get("MMAD_RECORD_DIR", "test_records")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "x3_matrix.json"), "w") as f:
            json.dump(_REC, f, indent=1, sort_keys=True)


class Checker:
    """error / bound ratios of one test (<= 1 passes, NaN fails); `where`
    names the case a ratio belongs to."""

    def __init__(self, section):
        self.section, self.where, self.bad = section, "", []

    def _note(self, name, ratio):
        ratio = float(ratio)
        if not ratio <= 1.0:
            self.bad.append((self.where, name, ratio))
        print(f"x3 {self.section} [{self.where}] {name}: error / bound {ratio:.3g}")
        _record(f"{self.section}: {name}", ratio)

    def ratio(self, name, got, ref, bound):
        self._note(name, ((got.double() - ref).abs() / bound).max() if ref.numel() else 0.0)

    def fp32(self, name, got, ref):
        """|got - ref| <= 2e-5 max|ref|"""
        self.ratio(name, got, ref, R.p3_bound(ref, stored=False))

    def exact(self, name, cond):
        self._note(name, 0.0 if bool(cond) else float("inf"))


# ---------------------------------------------------------------------------
# operands on the device (built once per problem, read only)
# ---------------------------------------------------------------------------
class Dev:
    def __init__(self, p):
        self.p = p
        for name in ("xp", "wp", "b", "sc", "sh", "colw", "ref"):
            setattr(self, name, getattr(p, name).cuda())
        self._zero_ref = None

    @property
    def zero_ref(self):
        if self._zero_ref is None:
            z = self.ref.clone()                 # NaN padding kept
            M, N = self.p.dims[:2]
            z[:M, :N] = 0.0
            self._zero_ref = z
        return self._zero_ref


@pytest.fixture(scope="module")
def devs():
    cache = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = Dev(R.problem(**kw))
        return cache[key]
    return get


def _bits_equal(a, b):
    return all(torch.equal(s.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8))
               for s, t in zip(a, b))


def twice(ck, fn):
    """run a call twice; the outputs (CPU tensors) of the first, and the
    repeat-run identity noted"""
    first, again = fn(), fn()
    ck.exact("repeat run bit-identical", _bits_equal(first, again))
    return first


# ---------------------------------------------------------------------------
# the calls: every output pre-filled (NaN, or a sentinel where the kernel
# writes only the valid region), returned on the CPU
# ---------------------------------------------------------------------------
def call_fwd(d, act, affine):
    M, N, K, Mp, Np, Kp = d.p.dims
    y = torch.full((2, Mp, Np), NAN, dtype=torch.bfloat16, device="cuda")
    call("mmad_fc_fwd", X3, M, N, K, Mp, Np, Kp, ptr(d.xp), ptr(d.wp), ptr(d.b), act, SLOPE,
         ptr(d.sc) if affine else None, ptr(d.sh) if affine else None, ptr(y), None, stream_ptr())
    torch.cuda.synchronize()
    return (y.cpu(),)


def call_score(d, act, affine, with_diff, ref=None):
    M, N, K, Mp, Np, Kp = d.p.dims
    ld_diff = N + 5
    y = torch.full((2, Mp, Np), NAN, dtype=torch.bfloat16, device="cuda")
    rows = torch.full((Np // 128, Mp), NAN, device="cuda")
    diff = torch.full((M + 2, ld_diff), SENTINEL, device="cuda") if with_diff else None
    call("mmad_fc_fwd_score", X3, M, N, K, Mp, Np, Kp, ptr(d.xp), ptr(d.wp), ptr(d.b), act, SLOPE,
         ptr(d.sc) if affine else None, ptr(d.sh) if affine else None, ptr(y),
         ptr(d.ref if ref is None else ref), ptr(rows), ptr(diff), ld_diff, stream_ptr())
    torch.cuda.synchronize()
    return (y.cpu(), rows.cpu()) + ((diff.cpu(),) if with_diff else ())


def call_nap(d):
    M, N, K, Mp, Np, Kp = d.p.dims            # R = N columns of vt = w
    rows = torch.full((Np // 128, Mp), NAN, device="cuda")
    score = torch.full((M + 1,), SENTINEL, device="cuda")
    call("mmad_nap_score", X3, M, K, N, Mp, Kp, Np, ptr(d.xp), ptr(d.wp), ptr(d.b), ptr(d.colw),
         ptr(rows), ptr(score), stream_ptr())
    torch.cuda.synchronize()
    return rows.cpu(), score.cpu()


# ---------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------
def check_y(ck, p, y, act, affine, with_t):
    M, N = p.dims[:2]
    got = y[0, :M, :N].double() + y[1, :M, :N].double()
    ref = p.y("p3", act, affine)
    ck.ratio("y (planes) vs P3", got, ref, R.p3_bound(ref, stored=True))
    if with_t:
        ref = p.y("t", act, affine)
        ck.ratio("y (planes) vs T", got, ref, R.t_bound(ref, p.dy(affine), stored=True))
    ck.exact("y planes == 0 for rows >= M and cols >= N",
             (y[:, M:, :] == 0).all() and (y[:, :, N:] == 0).all())


def check_score(ck, p, outs, act, affine, ref32=None):
    M, N, K, Mp, Np, Kp = p.dims
    y, rows = outs[0], outs[1]
    check_y(ck, p, y, act, affine, with_t=False)
    rf = (p.ref if ref32 is None else ref32)[:M, :N].double()
    d = p.y("p3", act, affine) - rf
    diff = outs[2][:M, :N] if len(outs) > 2 else None
    ck.exact("rowsq finite", torch.isfinite(rows).all())
    ck.exact("rowsq[:, M:Mp] == 0", (rows[:, M:] == 0).all())
    for t in range(Np // 128):
        cols = slice(128 * t, min(N, 128 * t + 128))
        if cols.start >= N:
            ck.exact("rowsq of a fully masked column group == 0", (rows[t] == 0).all())
            continue
        ck.fp32("rowsq vs P3", rows[t, :M], (d[:, cols] ** 2).sum(1))
        if diff is not None:
            ck.fp32("rowsq vs the returned diff", rows[t, :M], (diff[:, cols].double() ** 2).sum(1))
    if diff is not None:
        ck.fp32("diff vs P3", diff, d)
        full = outs[2]
        ck.exact("diff sentinels past row M and column N untouched",
                 (full[M:, :] == SENTINEL).all() and (full[:, N:] == SENTINEL).all())


def done(ck):
    assert not ck.bad, (len(ck.bad), ck.bad[:12])


# ---------------------------------------------------------------------------
# 1. the matrix at one masked problem
# ---------------------------------------------------------------------------
PROBLEMS = {"main": R.MAIN, "mini": R.MINI}


@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("act", ACTS, ids=ACT_IDS)
def test_fwd_epilogue(devs, act, affine):
    """y read back from the planes against P3 and against the true product,
    both planes exactly 0 on padding, equal bits on a second run."""
    ck = Checker("fwd")
    for name, kw in PROBLEMS.items():
        d = devs(**kw)
        ck.where = f"{name} {R.ACT_NAME[act]} affine={affine}"
        (y,) = twice(ck, lambda: call_fwd(d, act, affine))
        check_y(ck, d.p, y, act, affine, with_t=True)
    done(ck)


@pytest.mark.parametrize("with_diff", [0, 1], ids=["nodiff", "diff"])
@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_LEAKY, R.ACT_SIGMOID], ids=["none", "leaky", "sigmoid"])
def test_score_epilogue(devs, act, affine, with_diff):
    """mmad_fc_fwd_score(MMAD_BF16X3): fp32 ref at ldref = Np with NaN
    padding, diff at ld_diff = N + 5 in a sentinel frame, rowsq per column
    group (rows >= M and the fully masked group exactly 0)."""
    ck = Checker("score")
    for name, kw in PROBLEMS.items():
        d = devs(**kw)
        ck.where = f"{name} {R.ACT_NAME[act]} affine={affine} diff={with_diff}"
        outs = twice(ck, lambda: call_score(d, act, affine, with_diff))
        check_score(ck, d.p, outs, act, affine)
    done(ck)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_stored_planes_are_the_split_of_the_fp32_value(devs, name):
    """With ref == 0 the diff is the epilogue's fp32 value v bit for bit, so
    the planes must be hi = RNE_bf16(v), lo = RNE_bf16(v - hi) exactly."""
    ck = Checker("planes")
    d = devs(**PROBLEMS[name])
    M, N = d.p.dims[:2]
    ck.where = f"{name} leaky affine=1"
    y, rows, diff = twice(ck, lambda: call_score(d, R.ACT_LEAKY, 1, 1, ref=d.zero_ref))
    check_score(ck, d.p, (y, rows, diff), R.ACT_LEAKY, 1, ref32=torch.zeros_like(d.p.ref))
    v = diff[:M, :N].contiguous()
    hi, lo = R.planes_of(v)
    ck.exact("y_hi == bf16(diff) bitwise", torch.equal(y[0, :M, :N].contiguous().view(torch.int16),
                                                      hi.view(torch.int16)))
    ck.exact("y_lo == bf16(diff - hi) bitwise", torch.equal(y[1, :M, :N].contiguous().view(torch.int16),
                                                           lo.view(torch.int16)))
    ck.exact("the value is not all zero", (v != 0).any())
    done(ck)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_nap_form(devs, name):
    """mmad_nap_score(MMAD_BF16X3): score[m] = sum_j w_j z_mj^2 / R at the
    fp32 bar (w in [0.5, 1.5], 0 on padding; no reference), nothing written
    behind score[M - 1]."""
    ck = Checker("nap")
    d = devs(**PROBLEMS[name])
    p = d.p
    M, N = p.dims[:2]
    ck.where = name
    rows, score = twice(ck, lambda: call_nap(d))
    ref = (p.colw[:N].double() * p.z_p3 * p.z_p3).sum(1) / N
    ck.fp32("nap score vs P3", score[:M], ref)
    ck.exact("sentinel behind score[M - 1] untouched", score[M] == SENTINEL)
    ck.exact("rowsq finite", torch.isfinite(rows).all())
    done(ck)


# ---------------------------------------------------------------------------
# 2. tile order
# ---------------------------------------------------------------------------
GRIDS = [(9, 1), (1, 9), (3, 5), (5, 5), (2, 4)]      # tiles_m x tiles_n
GRID_IDS = [f"{a}x{b}" for a, b in GRIDS]


def grid_problem(tm, tn):
    """K = Kp = 128 (two stages), M and N one less than padded"""
    return dict(M=128 * tm - 1, N=128 * tn - 1, K=128, Mp=128 * tm, Np=128 * tn, Kp=128,
                seed=100 + 10 * tm + tn)


@pytest.mark.parametrize("tm,tn", GRIDS, ids=GRID_IDS)
def test_tile_order_covers_every_tile_once(devs, tm, tn):
    """Grids with more than 8 tiles, ntiles % 8 != 0 and a short last row
    group: every valid element finite and at the bar (a tile the map leaves
    out keeps its NaN), all padding zero.  SCORE with diff on 9x1 and 1x9."""
    ck = Checker("tile order")
    d = devs(**grid_problem(tm, tn))
    ck.where = f"grid {tm}x{tn} fwd"
    (y,) = twice(ck, lambda: call_fwd(d, R.ACT_LEAKY, 1))
    ck.exact("every valid element finite", torch.isfinite(y[:, :d.p.dims[0], :d.p.dims[1]].float()).all())
    check_y(ck, d.p, y, R.ACT_LEAKY, 1, with_t=False)
    if (tm, tn) in GRIDS[:2]:
        ck.where = f"grid {tm}x{tn} score"
        outs = twice(ck, lambda: call_score(d, R.ACT_LEAKY, 1, 1))
        check_score(ck, d.p, outs, R.ACT_LEAKY, 1)
    done(ck)


@pytest.mark.parametrize("tm,tn", [(5, 5), (3, 5)], ids=["5x5", "3x5"])
def test_group_m_changes_no_bit(devs, tm, tn):
    """The K order is fixed, so the tile order cannot change a bit: the
    default group height against group_m = 1, 2, 3 (a shorter last group), 5
    and 7 (above tiles_m: clamped), FWD and SCORE with diff."""
    ck = Checker("group_m")
    d = devs(**grid_problem(tm, tn))

    def both():
        return call_fwd(d, R.ACT_LEAKY, 1) + call_score(d, R.ACT_LEAKY, 1, 1)
    ck.where = f"grid {tm}x{tn} default"
    base = both()
    check_y(ck, d.p, base[0], R.ACT_LEAKY, 1, with_t=False)
    check_score(ck, d.p, base[1:], R.ACT_LEAKY, 1)
    for g in (1, 2, 3, 5, 7):
        ck.where = f"grid {tm}x{tn} group_m={g}"
        with _native.tune(group_m=g):
            got = both()
        ck.exact("bits equal to the default order", _bits_equal(base, got))
    done(ck)


# ---------------------------------------------------------------------------
# 3. edges of M, N, K
# ---------------------------------------------------------------------------
# every M of {1, 127, 128, 129}, N of {1, 3, 127, 128, 129} and K of
# {1, 63, 64, 65, 128, 129} at least once; one or two tiles each way
EDGES = [(1, 1, 1), (127, 3, 63), (128, 127, 64), (129, 128, 65), (1, 129, 128), (127, 129, 129),
         (129, 129, 129)]


@pytest.mark.parametrize("M,N,K", EDGES)
def test_edges_of_m_n_k(devs, M, N, K):
    ck = Checker("edges")
    d = devs(M=M, N=N, K=K, seed=1000 + 100 * M + 10 * N + K)
    ck.where = f"M={M} N={N} K={K} fwd"
    (y,) = twice(ck, lambda: call_fwd(d, R.ACT_NONE, 0))
    check_y(ck, d.p, y, R.ACT_NONE, 0, with_t=False)
    ck.where = f"M={M} N={N} K={K} score"
    outs = twice(ck, lambda: call_score(d, R.ACT_LEAKY, 1, 1))
    check_score(ck, d.p, outs, R.ACT_LEAKY, 1)
    done(ck)


# ---------------------------------------------------------------------------
# 4. the x3 VIB waist: z = mu on both planes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("B", [1, 127, 128, 129])
def test_vib_deterministic_copies_both_planes(B, k):
    """z[kk B + b, :btl] of each plane is that plane of enc[b, :btl] bit for
    bit (the lo plane of enc at roundup(B, 128) * ld_enc), everything else of
    [roundup(k B, 128)][ld_z] is 0 in both planes: the logvar columns and the
    padding rows of enc (all non-zero here) never reach the output."""
    btl, ld_enc, ld_z = 5, 128, 128
    Mpe, Mpz = R.pad(B), R.pad(k * B)
    g = torch.Generator().manual_seed(31 * B + k)
    v = torch.randn(Mpe, ld_enc, generator=g) + 3.0          # no zero anywhere in enc
    enc = torch.stack(R.planes_of(v))
    assert (enc[0] != 0).all()
    enc_d = enc.cuda()
    z = torch.full((2, Mpz, ld_z), NAN, dtype=torch.bfloat16, device="cuda")
    ck = Checker("vib")
    ck.where = f"B={B} k={k}"

    def run():
        z.fill_(NAN)
        call("mmad_vib_reparam_fwd", X3, B, btl, k, ptr(enc_d), ld_enc, None, None, 0, 0, 1, ptr(z), ld_z,
             None, stream_ptr())
        torch.cuda.synchronize()
        return (z.cpu(),)
    (out,) = twice(ck, run)
    want = torch.zeros(2, Mpz, ld_z, dtype=torch.bfloat16)
    for kk in range(k):
        want[:, kk * B:(kk + 1) * B, :btl] = enc[:, :B, :btl]
    ck.exact("z == mu on both planes, 0 elsewhere, bitwise",
             torch.equal(out.view(torch.int16), want.view(torch.int16)))
    ck.exact("lo plane is not all zero", (out[1] != 0).any())
    done(ck)
