"""Every MFMA GEMM kernel the layer operators can reach -- tile x epilogue x
operand type x split factor -- against a float64 reference.

Which tile runs for a shape is normally the autotuner's choice, so a parity
test at one shape exercises one tile.  Here every tile the rule allows
(mmad_gemm_tile_for) is forced through the tune table (knob 0; knob 5 for the
Adam-fused dW) on ONE small problem whose edges are all masked, and every
output -- the matrix, the per-chunk partials, the score rows, the diff, the
Adam state -- is compared with torch float64 evaluated on exactly the operand
values the kernel read (bf16 operands widened to float64).

The problem: every padded dimension 512 (each tile shape, 64x64 to 256x256,
divides it and gives a grid of at least 2x2 tiles), valid extents
  M = 400  the last 256-row tile partial; 32-row chunk 12 half valid (16
           rows), chunks 13-15 empty;
  N = 300  column 300 inside a 16-column fragment, the 128-column group
           256..383 partial, 384..511 fully masked;
  K = 489  the last K stage partially zero padding; 8 bf16 / 16 fp32 stages,
           more than any tile's ring depth.
The split rule (K / S >= 4 K-stages of 64 bf16 / 32 fp32 elements) admits
S = 2 for both operand types and S = 4 for fp32 only at K = 512.

Bars, from the number formats (none from the kernels' results):
  fp32 outputs (fp32 operands; dW; partials; score rows, diffs, scores)
      |got - ref| <= 2e-5 max|ref|   (test_gpu_gemm.py's fp32 bar; for
      partials max over the per-chunk references of that quantity);
  bf16-stored outputs (y, dz, dx of the bf16 path), per element
      |got - ref| <= 2^-8 |ref| + 2e-5 max|ref|   (bf16 keeps 8 significand
      bits, so round-to-nearest moves a value by at most half an ulp = 2^-8
      of it, reached at the bottom of a binade -- measured 0.99 of the bar;
      truncation would reach 2^-7 and fail; the second term is the fp32 bar
      on the value that is rounded);
  the bf16 score epilogue forms d = y - ref from the STORED bf16 y (it reads
      the staged bf16 tile back: to_f32(pv[e]) - to_f32(pr[e]) in both store
      paths of gemm_body, and the register-direct tiles are bit-identical), so
      a diff element may be off by y's rounding, 2^-8 |y|, and a score row by
      sum_j colw_j 2 |d_j| 2^-8 |y_j|, each plus the fp32 term.  Where y is
      stored the same quantities are also checked at the fp32 bar against
      float64 formed from the stored y: that pins the reduction itself.
Zero padding, untouched sentinels, shadow == bf16(p), bit-equal dw, zero
split-K control words and repeat-run identity are exact conditions."""
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr, F32, BF16

FWD, MSE, BWD_DATA, BWD_WEIGHT, SCORE = range(5)
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID, ACT_TANH = range(5)
M, N, K, P = 400, 300, 489, 512
CHUNK = 32
NCH = P // CHUNK
CNT = [max(0, min(CHUNK, M - c * CHUNK)) for c in range(NCH)]     # 12 x 32, 16, 3 x 0
SLOPE = 0.2
LD_T, LD_D = N + 7, N + 5
SENTINEL = 12345.0
FP32_BAR = 2e-5
BF16_REL = 2.0 ** -8

EPILOGUES = ("fwd", "mse", "score", "bwd_data", "bwd_weight", "adam")
EPI_OF = {"fwd": FWD, "mse": MSE, "score": SCORE, "bwd_data": BWD_DATA, "bwd_weight": BWD_WEIGHT,
          "adam": BWD_WEIGHT}
SPLITS = (1, 2, 4)

# Runnable tiles per (operand type, epilogue) at 512 x 512, written out by hand
# from the rule: tiles 0-5 serve everything; the 256x256 tile 6 the bf16
# forward-type epilogues (FWD, MSE, SCORE); the register-direct tiles 7, 8, 9
# bf16 FWD and SCORE; SCORE needs a tile at least 128 columns wide (not the
# 64x64 tile 3); tiles 6-9 combine no split-K slices.  The Adam-fused dW is
# the dW kernel with another epilogue branch: the same tiles.
TILE_COUNT = {
    1: {F32: {"fwd": 6, "mse": 6, "bwd_data": 6, "bwd_weight": 6, "adam": 6, "score": 5},
        BF16: {"fwd": 10, "mse": 7, "bwd_data": 6, "bwd_weight": 6, "adam": 6, "score": 9}},
    2: {F32: {"fwd": 6, "mse": 6, "bwd_data": 6, "bwd_weight": 6, "adam": 6, "score": 5},
        BF16: {"fwd": 6, "mse": 6, "bwd_data": 6, "bwd_weight": 6, "adam": 6, "score": 5}},
    # K / 4 = 128 is four fp32 K stages but only two bf16 ones: bf16 does not split by 4
    4: {F32: {"fwd": 6, "mse": 6, "bwd_data": 6, "bwd_weight": 6, "adam": 6, "score": 5},
        BF16: {"fwd": 0, "mse": 0, "bwd_data": 0, "bwd_weight": 0, "adam": 0, "score": 0}},
}
SPLIT_TAKEN = {F32: (1, 2, 4), BF16: (1, 2)}
BASE = {7: 6, 8: 6, 9: 1}            # the row-quad tile a register-direct tile falls back to


def options(epi):
    """The option sets of one epilogue: dicts with at least `partials` and
    `act`, the two things the tile query looks at besides the shape."""
    if epi == "fwd":
        return [dict(act=a, affine=af, stats=st, partials=st)
                for a in (ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID, ACT_TANH)
                for af in (0, 1) for st in (0, 1)]
    if epi == "mse":
        return [dict(act=ACT_NONE, partials=1, gscale=g) for g in (2.0, 0.5)]
    if epi == "score":
        o = [dict(act=a, affine=af, diff=d, partials=0, nap=0)
             for a in (ACT_NONE, ACT_LEAKY) for af in (0, 1) for d in (0, 1)]
        return o + [dict(act=ACT_NONE, affine=0, diff=0, partials=0, nap=1)]
    if epi == "bwd_data":
        return [dict(act=ACT_NONE, partials=c, colsum=c) for c in (0, 1)]
    if epi == "bwd_weight":
        return [dict(act=ACT_NONE, partials=0)]
    return [dict(act=ACT_NONE, partials=0, dw=d, step=s) for d in (0, 1) for s in (1, 3)]


def expected_run_tile(cfg, opt):
    if cfg in BASE and (opt["partials"] or opt["act"] not in (ACT_NONE, ACT_LEAKY, ACT_RELU)):
        return BASE[cfg]
    return cfg


def combos(lib, dt, epi, split):
    """(tile, option set, the tile the query says runs) for every runnable
    combination; [] when the split rule does not take `split` here.  Call with
    knob 4 (splitk) set to `split`."""
    if lib.mmad_gemm_splitk_for(P, P, P, dt, EPI_OF[epi]) != split:
        return []
    out = []
    for cfg in range(10):
        for opt in options(epi):
            run = lib.mmad_gemm_tile_for(cfg, dt, EPI_OF[epi], P, P, split, 0, opt["partials"], opt["act"])
            if run >= 0:
                out.append((cfg, opt, run))
    return out


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("epi", EPILOGUES)
def test_matrix_size_is_pinned(dt, epi, split):
    """The matrix cannot shrink silently: the number of runnable tiles per
    (operand type, epilogue, split) equals the hand-written table, every
    option set of an epilogue sees the same tiles, and the tile the query
    reports is the forced one or the documented fallback.  Pure queries."""
    lib = _native.load()
    with _native.tune(splitk=split):
        got = combos(lib, dt, epi, split)
        assert (lib.mmad_gemm_splitk_for(P, P, P, dt, EPI_OF[epi]) == split) == (split in SPLIT_TAKEN[dt])
    n_opt = len(options(epi))
    tiles = sorted({c for c, _, _ in got})
    assert len(tiles) == TILE_COUNT[split][dt][epi], (tiles, epi, dt, split)
    assert len(got) == len(tiles) * n_opt
    for cfg, opt, run in got:
        assert run == expected_run_tile(cfg, opt), (cfg, opt, run)
    if split > 1:
        assert not set(tiles) & {6, 7, 8, 9}


# ---------------------------------------------------------------------------
# operands and float64 references (built once, read only)
# ---------------------------------------------------------------------------
class Ops:
    def __init__(self, dt):
        dev = torch.device("cuda", 0)
        self.dt = dt
        self.tdt = tdt = torch.bfloat16 if dt == BF16 else torch.float32
        g = torch.Generator(device="cuda").manual_seed(20261 + dt)

        def packed(rows, cols, scale=1.0, dtype=tdt):
            t = torch.zeros(P, P, device=dev, dtype=dtype)
            t[:rows, :cols] = (torch.randn(rows, cols, device=dev, generator=g) * scale).to(dtype)
            return t

        def vec(n, scale, shift=0.0):
            t = torch.zeros(P, device=dev)
            t[:n] = torch.randn(n, device=dev, generator=g) * scale + shift
            return t
        self.x = packed(M, K)                      # [Mp][Kp]
        self.w = packed(N, K, 0.05)                # [Np][Kp]
        self.b = vec(N, 0.1)
        self.sc = vec(N, 0.1, 1.0)                 # eval-BN affine, 0 on padding
        self.sh = vec(N, 0.1)
        self.ref = packed(M, N)                    # score reference, independent of y
        self.tgt = torch.randn(M, LD_T, device=dev, generator=g)     # MSE target, ld > N
        self.colw = torch.zeros(P, device=dev)
        self.colw[:N] = torch.rand(N, device=dev, generator=g) + 0.5
        self.dz = packed(M, N)                     # [Mp][Np]; rows >= M zero (the dW ABI)
        # Adam state, zero on padding; m / v at the gradient's scale (dW entries
        # are sums of 400 products of N(0,1) values: ~20)
        self.p0 = packed(N, K, 0.05, torch.float32)
        self.m0 = packed(N, K, 2.0, torch.float32)
        self.v0 = torch.zeros(P, P, device=dev)
        self.v0[:N, :K] = (torch.rand(N, K, device=dev, generator=g) + 0.5) * 400.0
        # float64 references
        xd, wd = self.x[:M, :K].double(), self.w[:N, :K].double()
        self.z = xd @ wd.t() + self.b[:N].double()                   # pre-activation [M][N]
        self.dx = self.dz[:M, :N].double() @ wd                       # [M][K]
        self.dw = self.dz.double().t() @ self.x.double()              # [Np][Kp], zero padding
        self._y = {}

    def y(self, act, affine):
        key = (act, affine)
        if key not in self._y:
            z = self.z
            slope = float(torch.tensor(SLOPE, dtype=torch.float32))   # the float the kernel gets
            a = {ACT_NONE: lambda: z, ACT_LEAKY: lambda: torch.where(z > 0, z, z * slope),
                 ACT_RELU: lambda: z.clamp_min(0.0), ACT_SIGMOID: lambda: torch.sigmoid(z),
                 ACT_TANH: lambda: torch.tanh(z)}[act]()
            if affine:
                a = a * self.sc[:N].double() + self.sh[:N].double()
            self._y[key] = a
        return self._y[key]


@pytest.fixture(scope="module")
def ops():
    cache = {}

    def get(dt):
        if dt not in cache:
            cache[dt] = Ops(dt)
        return cache[dt]
    return get


@pytest.fixture(scope="module")
def ws():
    w = _native.enable_gemm_workspace(torch.device("cuda", 0))
    yield w
    call("mmad_gemm_set_workspace", None, 0)


def _ctl_zero(ws):
    lib = _native.load()
    n = int(lib.mmad_gemm_ws_bytes())
    ctl = (8191 + 1) * 4                     # MMAD_SK_ERR_WORD + 1 words (csrc/mmad_gemm.h)
    slab = 832 * 128 * 128 * 4               # MMAD_SK_SLAB_TILES 128x128 fp32 tiles
    assert n == slab + ctl
    return int(ws[slab:n].view(torch.int32).abs().sum().item()) == 0


# ---------------------------------------------------------------------------
# checks: each returns error / bound (<= 1 passes; NaN fails)
# ---------------------------------------------------------------------------
def worse(a, b):
    """the larger of two error / bound ratios; a NaN wins and stays"""
    return a if a != a or a >= b else b


class Checker:
    def __init__(self, dt):
        self.bf16 = dt == BF16
        self.ratios = {}
        self.bad = []

    def note(self, name, ratio):
        ratio = float(ratio)
        if not ratio <= 1.0:
            self.bad.append((name, ratio))
        self.ratios[name] = worse(self.ratios.get(name, 0.0), ratio)

    def fp32(self, name, got, ref):
        """|got - ref| <= 2e-5 max|ref|"""
        ref = ref.double()
        bound = FP32_BAR * ref.abs().max() + 1e-300
        self.note(name, ((got.double() - ref).abs() / bound).max())

    def stored(self, name, got, ref):
        """an output in the operand type: the bf16 per-element bar, or fp32's"""
        if not self.bf16:
            return self.fp32(name, got, ref)
        bound = BF16_REL * ref.abs() + FP32_BAR * ref.abs().max()
        self.note(name, ((got.double() - ref).abs() / bound).max())

    def slack(self, name, got, ref, slack):
        """|got - ref| <= slack + 2e-5 max|ref| (slack: elementwise, from the reference)"""
        bound = slack + FP32_BAR * ref.abs().max() + 1e-300
        self.note(name, ((got.double() - ref).abs() / bound).max())

    def exact(self, name, cond):
        self.note(name, 0.0 if bool(cond) else float("inf"))


def chunk_sums(a):
    """[M][cols] float64 -> [NCH][cols]: sums over each 32-row chunk's valid rows"""
    full = torch.zeros(NCH * CHUNK, a.shape[1], device=a.device, dtype=torch.float64)
    full[:M] = a
    return full.view(NCH, CHUNK, -1).sum(1)


def nan_like(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), device="cuda", dtype=dtype)


def zero_padding(t, rows, cols):
    return bool((t[rows:, :] == 0).all()) and bool((t[:, cols:] == 0).all())


def run_fwd(o, opt, ck):
    y = nan_like(P, P, o.tdt)
    st = torch.full((NCH, 2, P), float("nan"), device="cuda") if opt["stats"] else None
    call("mmad_fc_fwd", o.dt, M, N, K, P, P, P, ptr(o.x), ptr(o.w), ptr(o.b), opt["act"], SLOPE,
         ptr(o.sc) if opt["affine"] else None, ptr(o.sh) if opt["affine"] else None, ptr(y), ptr(st),
         stream_ptr())
    ref = o.y(opt["act"], opt["affine"])
    ck.stored("y", y[:M, :N], ref)
    ck.exact("y padding == 0", zero_padding(y, M, N))
    if st is not None:
        cnt = torch.tensor(CNT, device="cuda", dtype=torch.float64).view(NCH, 1)
        mean_ref = chunk_sums(ref) / cnt.clamp_min(1.0)
        full = torch.zeros(NCH * CHUNK, N, device="cuda", dtype=torch.float64)
        full[:M] = ref
        dev = full.view(NCH, CHUNK, N) - mean_ref.view(NCH, 1, N)
        rows = torch.arange(NCH * CHUNK, device="cuda").view(NCH, CHUNK, 1) < M
        m2_ref = (dev * dev * rows).sum(1)
        mean, m2 = st[:, 0, :N].double(), st[:, 1, :N].double()
        ck.fp32("welford mean", mean, mean_ref)          # chunk 12: the mean of 16 rows, not 32
        ck.fp32("welford M2", m2, m2_ref)
        ck.exact("empty chunks == (0, 0)", (st[13:, :, :N] == 0).all())
        # Chan's merge of the chunks, in float64
        n, bm, bq = 0.0, torch.zeros(N, device="cuda", dtype=torch.float64), 0.0
        for c in range(NCH):
            if CNT[c] == 0:
                continue
            tot = n + CNT[c]
            d = mean[c] - bm
            bm = bm + d * (CNT[c] / tot)
            bq = bq + m2[c] + d * d * (n * CNT[c] / tot)
            n = tot
        ck.fp32("batch mean", bm, ref.mean(0))
        ck.fp32("batch var", bq / M, ref.var(0, unbiased=False))
    return (y, st) if st is not None else (y,)


def run_mse(o, opt, ck):
    dz = nan_like(P, P, o.tdt)
    part = torch.full((NCH, 2, P), float("nan"), device="cuda")
    call("mmad_fc_fwd_mse", o.dt, M, N, K, P, P, P, ptr(o.x), ptr(o.w), ptr(o.b), ptr(o.tgt), LD_T,
         opt["gscale"], ptr(dz), ptr(part), stream_ptr())
    d = o.z - o.tgt[:, :N].double()
    ref = opt["gscale"] * d
    ck.stored("dz", dz[:M, :N], ref)
    ck.exact("dz padding == 0", zero_padding(dz, M, N))
    # the partials are summed from the fp32 values, before dz is rounded
    ck.fp32("partial sum dz", part[:, 0, :N], chunk_sums(ref))
    ck.fp32("partial sum d^2", part[:, 1, :N], chunk_sums(d * d))
    ck.fp32("sum-MSE", part[:, 1, :N].double().sum().view(1), (d * d).sum().view(1))
    return dz, part


def run_score(o, opt, ck):
    rows = torch.full((P // 128, P), float("nan"), device="cuda")
    if opt["nap"]:
        # score[m] = (1/R) sum_j colw[j] (x . vt[j] + bias[j])^2, R = N, vt = w
        score = torch.full((M + 1,), SENTINEL, device="cuda")
        call("mmad_nap_score", o.dt, M, K, N, P, P, P, ptr(o.x), ptr(o.w), ptr(o.b), ptr(o.colw),
             ptr(rows), ptr(score), stream_ptr())
        cw = o.colw[:N].double()
        ref = (cw * o.z * o.z).sum(1) / N
        slack = (cw * 2.0 * o.z.abs() * BF16_REL * o.z.abs()).sum(1) / N if ck.bf16 else 0.0
        ck.slack("nap score", score[:M], ref, slack)
        ck.exact("nap guard row untouched", score[M] == SENTINEL)
        return rows, score
    y = nan_like(P, P, o.tdt)
    diff = torch.full((M + 2, LD_D), SENTINEL, device="cuda") if opt["diff"] else None
    call("mmad_fc_fwd_score", o.dt, M, N, K, P, P, P, ptr(o.x), ptr(o.w), ptr(o.b), opt["act"], SLOPE,
         ptr(o.sc) if opt["affine"] else None, ptr(o.sh) if opt["affine"] else None, ptr(y), ptr(o.ref),
         ptr(rows), ptr(diff), LD_D, stream_ptr())
    yr = o.y(opt["act"], opt["affine"])
    rf = o.ref[:M, :N].double()
    d = yr - rf
    ck.stored("y", y[:M, :N], yr)
    ck.exact("y padding == 0", zero_padding(y, M, N))
    got_rows = rows[:, :M].double().sum(0)
    # bf16: d is formed from the stored (rounded) y -- see the module docstring
    ck.slack("rowsq", got_rows, (d * d).sum(1),
             (2.0 * d.abs() * BF16_REL * yr.abs()).sum(1) if ck.bf16 else 0.0)
    ds = y[:M, :N].double() - rf                    # what the epilogue subtracts, in float64
    ck.fp32("rowsq (stored y)", got_rows, (ds * ds).sum(1))
    if diff is not None:
        ck.slack("diff", diff[:M, :N], d, BF16_REL * yr.abs() if ck.bf16 else 0.0)
        ck.fp32("diff (stored y)", diff[:M, :N], ds)
        ck.exact("diff outside [M, N] untouched",
                 (diff[M:, :] == SENTINEL).all() and (diff[:, N:] == SENTINEL).all())
        return y, rows, diff
    return y, rows


def run_bwd_data(o, opt, ck):
    dx = nan_like(P, P, o.tdt)
    cs = torch.full((NCH, 2, P), float("nan"), device="cuda") if opt["colsum"] else None
    call("mmad_fc_bwd_data", o.dt, M, N, K, P, P, P, ptr(o.dz), ptr(o.w), ptr(dx), ptr(cs), stream_ptr())
    ck.stored("dx", dx[:M, :K], o.dx)
    ck.exact("dx padding == 0", zero_padding(dx, M, K))
    if cs is not None:
        ck.fp32("colsum", cs[:, 0, :K], chunk_sums(o.dx))
        return dx, cs
    return (dx,)


def run_bwd_weight(o, opt, ck):
    dw = nan_like(P, P, torch.float32)
    call("mmad_fc_bwd_weight", o.dt, P, P, P, ptr(o.dz), ptr(o.x), ptr(dw), stream_ptr())
    if ck is not None:
        ck.fp32("dW", dw, o.dw)
    return (dw,)


def adam_ref(g, p0, m0, v0, b1, b2, eps, step_size, bc2_sqrt):
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * g * g
    return p0 - step_size * m / (v.sqrt() / bc2_sqrt + eps), m, v


def run_adam(o, opt, ck):
    b1, b2, eps, lr, step = 0.9, 0.999, 1e-8, 1e-3, opt["step"]
    step_size, bc2_sqrt = lr / (1.0 - b1 ** step), (1.0 - b2 ** step) ** 0.5
    first = step == 1
    p = o.p0.clone()
    m = torch.zeros_like(o.m0) if first else o.m0.clone()
    v = torch.zeros_like(o.v0) if first else o.v0.clone()
    shadow = nan_like(P, P, torch.bfloat16) if ck.bf16 else None
    dw = nan_like(P, P, torch.float32) if opt["dw"] else None
    call("mmad_fc_bwd_weight_adam", o.dt, P, P, P, ptr(o.dz), ptr(o.x), ptr(p), ptr(m), ptr(v), ptr(shadow),
         ptr(dw), b1, b2, eps, step_size, bc2_sqrt, stream_ptr())
    m0 = torch.zeros_like(o.dw) if first else o.m0.double()
    v0 = torch.zeros_like(o.dw) if first else o.v0.double()
    args = (o.p0.double(), m0, v0, b1, b2, eps, step_size, bc2_sqrt)
    pr, mr, vr = adam_ref(o.dw, *args)
    ck.fp32("adam m", m, mr)
    ck.fp32("adam v", v, vr)
    # p: the update m / (sqrt(v) / bc2 + eps) is not Lipschitz in the gradient
    # where v comes from that gradient alone (step 1: lr g / (|g| + eps'), a
    # step function of an entry that is zero to rounding), so the fp32 bar on
    # dW, dg = 2e-5 max|dW|, is carried through the update: the reference is
    # evaluated at g - dg and g + dg (step 1: the update is monotone in g, so
    # the ends bound it; step 3: v >= b2 v0 > 0 makes it smooth over dg).
    # Padding (g exactly 0) gets no such allowance: it is checked exactly.
    dg = FP32_BAR * o.dw.abs().max()
    lo, hi = adam_ref(o.dw - dg, *args)[0], adam_ref(o.dw + dg, *args)[0]
    slack = torch.maximum((lo - pr).abs(), (hi - pr).abs())
    slack[N:, :] = 0.0
    slack[:, K:] = 0.0
    ck.slack("adam p", p, pr, slack)
    for name, t in (("p", p), ("m", m), ("v", v)):
        ck.exact(f"adam {name} padding == 0", zero_padding(t, N, K))
    if shadow is not None:
        ck.exact("shadow == bf16(p)", torch.equal(shadow, p.bfloat16()))
    if dw is not None:
        ck.fp32("dW", dw, o.dw)
        with _native.tune(tile=_native.tune_get("tile_adam")):
            plain = run_bwd_weight(o, opt, None)[0]
        ck.exact("dw bit-equal to mmad_fc_bwd_weight", torch.equal(dw, plain))
        return p, m, v, dw
    return p, m, v


RUN = {"fwd": run_fwd, "mse": run_mse, "score": run_score, "bwd_data": run_bwd_data,
       "bwd_weight": run_bwd_weight, "adam": run_adam}


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("epi", EPILOGUES)
def test_every_kernel_against_fp64(ws, ops, dt, epi, split):
    """Every runnable (tile, option set) of one (epilogue, operand type,
    split factor) at the ragged 512^3 problem, each output at its bar; with a
    split, twice (bit-identical) and the control words left zero.  Prints the
    worst error / bound per checked quantity."""
    lib = _native.load()
    o = ops(dt)
    knob = "tile_adam" if epi == "adam" else "tile"
    bad, worst, ran = [], {}, 0
    with _native.tune(splitk=split):
        todo = combos(lib, dt, epi, split)
        for cfg, opt, run_tile in todo:
            # the query's answer first: the forced tile, or its documented fallback
            assert run_tile == expected_run_tile(cfg, opt), (cfg, opt, run_tile)
            ck = Checker(dt)
            with _native.tune(**{knob: cfg}):
                outs = RUN[epi](o, opt, ck)
                if split > 1:
                    again = RUN[epi](o, opt, Checker(dt))
                    ck.exact("repeat run bit-identical",
                             all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                 for a, b in zip(outs, again)))
            ck.exact("split-K control words zero", _ctl_zero(ws))
            ran += 1
            bad += [(cfg, opt, name, r) for name, r in ck.bad]
            for name, r in ck.ratios.items():
                worst[name] = worse(worst.get(name, 0.0), r)
    for name in sorted(worst):
        print(f"matrix {'bf16' if dt == BF16 else 'f32'} {epi} split {split}: {name}: "
              f"worst error/bound {worst[name]:.3g}")
    assert ran == TILE_COUNT[split][dt][epi] * len(options(epi)), ran
    assert not bad, (len(bad), bad[:12])
