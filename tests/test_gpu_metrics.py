"""The device metrics (csrc/mmad_metrics.hip) through the public entries
mmad_rank_metrics / mmad_threshold_metrics with explicit, exactly sized
workspaces inside sentinel-filled buffers, and through metric.py where the
wrapper is the subject, against tests/metrics_ref.py (numpy float64 and integer
counts; held to sklearn by tests/test_metrics_reference.py without a GPU).

Size classes of the installed rocPRIM (device_radix_sort.hpp,
detail/device_config_helper.hpp, device_merge_sort.hpp, device_scan.hpp,
detail/config/*.hpp; only the onesweep kernel shapes carry a gfx950 table, the
rest take the generic defaults):

  radix sort, (uint32 key, uint8 value) and (float key, no value): item scale 4,
  so the single-block sort is 256 threads x 4 items
      n <= 1024                one block (radix_sort_block_sort)
      1025 .. 1,048,576        merge sort (merge_sort_limit = 1024 * 1024, keys
                               wider than 2 bytes): 1024-item block sorts, then
                               block merges, odd-even up to n = (1 << 17) + 70000
                               = 201,072 and merge-path above it
      n > 1,048,576            onesweep
  inclusive scan, uint8 in, uint32 accumulator (plus<uint32_t>): 256 threads x
  16 items
      n <= 4096                one block (single_scan)
      n > 4096                 decoupled look-back over 4096-item blocks
  (the gfx942 table's 256 x 21 = 5376 would be the limit if a later rocPRIM
  mapped gfx950 onto it; 5376 / 5377 are in the sizes at no cost)

and the kernels' own: launches of 256 (n = 255, 256, 257), rank_final_k's
strided sum from 257 blocks (n > 65,536).  RANK_SIZES has a case on each side of
every limit above.

Bars
  n_pos, n_neg   exact
  AUROC          bit-equal: every term of U is a multiple of 1/2 and
                 U < n^2 < 2^52, so every partial sum is exact in fp64 in any
                 order; P N is exact; the division is correctly rounded on
                 both sides.  NaN exactly when P N = 0.
  AUPR           |got - ref| <= k 2^-53 ref, all terms >= 0, k the roundings on
                 the longest path of the kernel's tree:
                   7   inside one term: four quotients (tp / cnt, tp / P, and
                       the previous run's two), one difference, one sum, one
                       product (the factor 0.5 is exact)
                   10  block_sum_d in rank_contrib_k: 6 shuffle steps and the
                       4 wave partials added by thread 0
                   c   rank_final_k's strided adds, c = ceil(blocks / 256)
                   10  its block_sum_d
                   1   the reference's own rounding (math.fsum rounds once)
                 k = 28 + ceil(ceil(n / 256) / 256): 29 up to n = 65,536, 45 at
                 n = 1,100,003.  Without positives the sum is 0.5 + zeros: 0.5
                 exactly.  With positives only the reference is 1.0 exactly
                 and the kernel is held to the same k 2^-53.
  threshold      within one fp32 ulp of float32(np.quantile(float64(valid), q))
                 (a contraction of a + (b - a) g into an fma moves the float64
                 by an ulp, the fp32 rounding only next to a tie); cases that
                 are not bit-equal are printed (none expected)
  counts         tp / fp / fn / tn and the F1 counts at the threshold the
                 kernel returned, exact; p, r, precision, recall the float64
                 quotients of those integers, exact; F1 within 2 fp64 ulps of
                 p r 2 / (p + r); NaN exactly where the float64 formulas give it

Lines starting with "metrics:" carry the measured figures (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native, metric
from icra2021_multimodal_ad_amd._native import ptr, stream_ptr
from tests import metrics_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
FILL = 0xA5                     # workspace sentinel byte
PAD = 512                       # sentinel bytes kept before and behind a workspace
GUARD = 4                       # NaN doubles before and behind `out`
NAN_BITS = 0x7ff8000000000000
U53 = 2.0 ** -53

RANK_SIZES = [1, 2, 255, 256, 257, 513, 1024, 1025, 4096, 4097, 5376, 5377, 65536, 65537, 201072, 201073,
              300001, 1048576, 1048577, 1100003]
PATTERNS = ["distinct", "equal", "split256", "run200_600", "top_bottom", "round1"]
LABELS = ["rand30", "none", "all", "one_best", "one_worst", "one_in_run", "many_in_run"]


@pytest.fixture(scope="module")
def lib():
    _native.require_gpu()
    return _native.load()


# ------------------------------------------------------------------ plumbing
class _Ws:
    """`nbytes` of workspace at a 256-byte aligned address inside a
    buffer of FILL bytes, PAD or more of them on either side."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * PAD + 512,), FILL, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.start = (base + PAD + 255) // 256 * 256 - base
        self.ptr = ctypes.c_void_p(base + self.start)

    def guards_intact(self):
        a, b = self.buf[:self.start], self.buf[self.start + self.nbytes:]
        assert a.numel() >= PAD and b.numel() >= PAD
        return bool((a == FILL).all()) and bool((b == FILL).all())

    def untouched(self):
        return bool((self.buf == FILL).all())


class _Out:
    """`n` doubles inside a frame of NaN, NaN themselves before the call."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        assert int(self.buf.view(torch.int64)[0]) == NAN_BITS
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 8 * GUARD)

    def read(self):
        bits = self.buf.view(torch.int64).cpu().numpy()
        frame = np.concatenate((bits[:GUARD], bits[GUARD + self.n:]))
        assert (frame == NAN_BITS).all(), "a slot outside out[] was written"
        return self.buf[GUARD:GUARD + self.n].cpu().numpy()

    def untouched(self):
        return bool((self.buf.view(torch.int64) == NAN_BITS).all())


def _rank(lib, score, label, ws=None):
    """One mmad_rank_metrics call on host arrays: out[4] as float64 numpy."""
    s = torch.from_numpy(np.ascontiguousarray(score, np.float32)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).cuda()
    n = s.numel()
    ws = ws or _Ws(lib.mmad_rank_metrics_ws_bytes(n))
    assert ws.nbytes > 0
    out = _Out(4)
    _native.call("mmad_rank_metrics", n, ptr(s), ptr(lab), out.ptr, ws.ptr, ws.nbytes, stream_ptr())
    torch.cuda.synchronize()
    assert ws.guards_intact(), "mmad_rank_metrics wrote outside its workspace"
    return out.read()


def _threshold(lib, valid, test, label, q):
    v = torch.from_numpy(np.ascontiguousarray(valid, np.float32)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(test, np.float32)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).cuda()
    ws = _Ws(lib.mmad_threshold_metrics_ws_bytes(v.numel()))
    assert ws.nbytes > 0
    out = _Out(10)
    _native.call("mmad_threshold_metrics", v.numel(), ptr(v), t.numel(), ptr(t), ptr(lab), float(q), out.ptr,
                 ws.ptr, ws.nbytes, stream_ptr())
    torch.cuda.synchronize()
    assert ws.guards_intact(), "mmad_threshold_metrics wrote outside its workspace"
    assert (v.cpu().numpy().view(np.uint32) == np.ascontiguousarray(valid, np.float32).view(np.uint32)).all()
    return out.read()


def _same(a, b):
    """Equal as float64 bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a, b, equal_nan=True)


def _ulps64(a, b):
    if math.isnan(a) or math.isnan(b):
        return 0 if math.isnan(a) and math.isnan(b) else math.inf
    ia, ib = (int(np.float64(x).view(np.int64)) for x in (a, b))
    return abs(ia - ib)


def _aupr_k(n):
    return 28 + math.ceil(math.ceil(n / 256) / 256)


def _check_rank(got, ref, n, what):
    """The rank bars of the module docstring; returns AUPR error / bound."""
    assert got[2] == ref["P"] and got[3] == ref["N"], (what, got, ref["P"], ref["N"])
    if ref["P"] and ref["N"]:
        assert got[0] == ref["auroc"], (what, "AUROC not bit-equal", got[0], ref["auroc"])
    else:
        assert math.isnan(got[0]), (what, got[0])
    bound = _aupr_k(n) * U53 * ref["aupr"]
    err = abs(got[1] - ref["aupr"])
    assert math.isfinite(got[1]) and err <= bound, (what, got[1], ref["aupr"], err, bound)
    if ref["P"] == 0:
        assert ref["aupr"] == 0.5 and got[1] == 0.5, (what, got[1])
    if ref["N"] == 0:
        assert ref["aupr"] == 1.0, (what, ref["aupr"])
    return err / bound


# ------------------------------------------------------------- rank: inputs
def _pattern(name, n, rng):
    """fp32 scores of the pattern, shuffled (n >= _MIN_N[name]).  Positions are
    those of the kernel's descending order."""
    rank = np.arange(n)                                   # 0 = best score
    if name == "distinct":
        v = (n // 2 - rank) * 0.25                        # n < 2^24: all distinct in fp32
    elif name == "equal":
        v = np.full(n, 0.75)
    elif name == "split256":                              # two values, the cut at sorted index 256
        v = np.where(rank < 256, 2.0, -1.0)
    elif name == "run200_600":                            # one run over sorted elements 200 .. 600
        v = -rank.astype(np.float64)
        v[200:601] = -200.0
    elif name == "top_bottom":                            # a run from index 0 and one up to n - 1
        t = max(1, min(300, n // 3))
        v = -rank.astype(np.float64)
        v[:t] = 1.0
        v[n - t:] = -float(n)
    elif name == "round1":
        v = np.round(rng.normal(size=n), 1)
    v = v.astype(np.float32)
    rng.shuffle(v)
    return v


def _largest_run(score):
    vals, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    j = int(cnt.argmax())
    return np.flatnonzero(inv.reshape(-1) == j), int(cnt[j])


def _labels(name, score, rng, run=None):
    """uint8 labels of the kind, or None where the scores have no room for it."""
    n = score.size
    lab = np.zeros(n, np.uint8)
    if name == "rand30":
        lab = (rng.random(n) < 0.3).astype(np.uint8)
    elif name == "all":
        lab[:] = 1
    elif name == "one_best":
        lab[int(score.argmax())] = 1
    elif name == "one_worst":
        lab[int(score.argmin())] = 1
    elif name in ("one_in_run", "many_in_run"):
        idx, length = run
        if name == "one_in_run":
            if length < 2:
                return None
            lab[idx[length // 2]] = 1
        else:                                             # > 255 positives inside one run, negatives beside them
            if length < 258:
                return None
            lab = (rng.random(n) < 0.1).astype(np.uint8)
            lab[idx] = 0
            lab[idx[:max(256, length - length // 4)]] = 1
            assert lab[idx].sum() > 255 and lab[idx].sum() < length
    return lab


def _label_kinds(n, pattern):
    """Every kind up to 65,537 elements; above, where one reference costs tens
    of milliseconds, every kind on the round(., 1) ties (up to 300,001) and on
    the distinct scores the kinds that do not need a run."""
    if n <= 65537:
        return LABELS
    if pattern == "round1":
        return LABELS if n <= 300001 else ["rand30", "many_in_run"]
    if pattern == "distinct":
        return ["rand30", "none", "all", "one_best", "one_worst"] if n <= 300001 else ["rand30", "all"]
    return ["rand30"]


_MIN_N = {"split256": 257, "run200_600": 602, "top_bottom": 3}
RANK_CASES = [(n, p) for n in RANK_SIZES for p in PATTERNS if n >= _MIN_N.get(p, 1)]


@pytest.mark.parametrize("n,pattern", RANK_CASES)
def test_rank_metrics_match_the_float64_rank_reference(lib, n, pattern):
    """Every size x score pattern (where it fits) x label kind (where the
    scores have a run for it), each call with an exactly sized workspace in a
    sentinel frame and out[4] in a NaN frame, twice for the same bits."""
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n % 997)
    score = _pattern(pattern, n, rng)
    kinds = _label_kinds(n, pattern)
    run = _largest_run(score) if any(k.endswith("in_run") for k in kinds) else None
    worst, ran = 0.0, 0
    for kind in kinds:
        lab = _labels(kind, score, rng, run)
        if lab is None:
            continue
        ref = R.rank_ref(score, lab)
        got = _rank(lib, score, lab)
        again = _rank(lib, score, lab)
        assert got.tobytes() == again.tobytes(), (kind, got, again)
        worst = max(worst, _check_rank(got, ref, n, (n, pattern, kind)))
        ran += 1
    assert ran >= 1
    print(f"metrics: rank n={n} {pattern}: {ran} label kinds, AUROC bit-equal, "
          f"AUPR worst error / bound {worst:.4f} (k = {_aupr_k(n)})")


def _special_values():
    fi = np.finfo(np.float32)
    den = np.float32(1e-45)                               # the smallest denormal
    s = np.array([-0.0, 0.0, 0.0, -0.0, -den, den, -fi.tiny, fi.tiny, -fi.max, fi.max, -np.inf, np.inf,
                  -1.5, 2.5, -3e-39, 3e-39, np.inf, -np.inf, fi.max, -fi.max, 1e-30, -1e-30], np.float32)
    # both -0.0 are positive and both +0.0 negative: tied, the four pairs add 4 x 1/2 to
    # U; ordered by their bits they add 0 (and 4 with the labels exchanged).  Every
    # other negative value's positive twin is labelled the other way, so a key order
    # that misplaces a sign class, the denormals or the infinities changes U; each
    # infinity appears with both labels
    lab = np.array([1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1,
                    1, 0, 0, 1, 0, 1, 1, 0, 0, 1], np.uint8)
    return s, lab


def test_rank_metrics_special_values(lib):
    """-0.0 beside +0.0 with opposite labels, +-denormal, +-FLT_MIN, +-FLT_MAX,
    +-inf and normals of both signs in one vector, alone (one block) and among
    3000 normal scores (the merge sort); the reference is rank_ref (sklearn
    refuses inf).  Exchanging the labels of the two zero signs must not move
    either metric, since the zeros are one run."""
    s, lab = _special_values()
    rng = np.random.default_rng(7)
    big_s = np.concatenate((s, rng.normal(size=3000).astype(np.float32)))
    big_l = np.concatenate((lab, (rng.random(3000) < 0.3).astype(np.uint8)))
    perm = rng.permutation(big_s.size)
    for score, label in ((s, lab), (big_s[perm], big_l[perm])):
        ref = R.rank_ref(score, label)
        got = _rank(lib, score, label)
        _check_rank(got, ref, score.size, ("special", score.size))
        neg0 = np.flatnonzero((score == 0) & np.signbit(score))
        pos0 = np.flatnonzero((score == 0) & ~np.signbit(score))
        assert neg0.size == 2 and pos0.size == 2
        swapped = label.copy()
        swapped[neg0], swapped[pos0] = label[pos0], label[neg0]
        assert (swapped != label).sum() == 4
        assert _rank(lib, score, swapped).tobytes() == got.tobytes()
    print("metrics: rank special values: AUROC bit-equal, signed zeros tie")


def test_rank_metrics_cached_workspace_large_small_large():
    """metric.rank_metrics keeps one workspace per device and grows it: sizes in
    the order large, small, larger, small reuse it both ways."""
    rng = np.random.default_rng(21)
    metric._ws.clear()
    for n in (300001, 257, 1100003, 1, 4097):
        score = np.round(rng.normal(size=n), 2).astype(np.float32)
        lab = (rng.random(n) < 0.3).astype(np.uint8)
        lab[0] = 1
        got = np.array(metric.rank_metrics(score, lab))
        _check_rank(got, R.rank_ref(score, lab), n, ("cached", n))
    (w,) = [v for k, v in metric._ws.items() if k[0] == "rank"]
    assert w.numel() >= _native.load().mmad_rank_metrics_ws_bytes(1100003)
    with pytest.raises(ValueError, match="length mismatch"):
        metric.rank_metrics(np.zeros(3, np.float32), np.zeros(4, np.uint8))


# ---------------------------------------------------------------- thresholds
# 1024 / 1025: the single-block sort's limit; 300,001: merge-path merges;
# 1,048,577: onesweep (keys only, the same limits as the pair sort)
VALID_SIZES = [1, 2, 3, 10, 11, 257, 1024, 1025, 4097, 100003, 300001, 1048577]
QS = [0.0, 0.1, 0.5, 0.9, 0.99, 1.0]


def _virtual(n, q):
    """(lo, hi, g) of threshold_k: float64 q (n - 1), floor, clamp."""
    vi = q * (n - 1)
    lo = min(max(int(math.floor(vi)), 0), n - 1)
    return lo, min(lo + 1, n - 1), vi - lo


def test_threshold_grid_takes_both_lerp_branches():
    gs = {(n, q): _virtual(n, q)[2] for n in VALID_SIZES for q in QS}
    assert any(0 < g < 0.5 for g in gs.values()) and any(g >= 0.5 for g in gs.values())
    assert any(g == 0 and 0 < q < 1 and n > 1 for (n, q), g in gs.items())


def _valid_sets(n, q, rng):
    """(name, fp32 valid scores): unsorted; tied neighbours around the quantile
    index; -0.0 and +0.0 at the quantile index."""
    lo, hi, _ = _virtual(n, q)
    base = rng.normal(size=n).astype(np.float32)
    out = [("unsorted", base)]
    srt = np.sort(base)
    tied = srt.copy()
    tied[max(lo - 1, 0):hi + 2] = srt[lo]
    out.append(("tied", rng.permutation(tied)))
    z = (srt - srt[lo]).astype(np.float32)                # monotone; z[lo] = +0.0
    z[lo], z[hi] = -0.0, 0.0
    assert (np.diff(z) >= 0).all()
    out.append(("zeros", rng.permutation(z)))
    return out


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("n_valid", VALID_SIZES)
def test_threshold_is_the_float64_quantile_rounded_once(lib, n_valid, q):
    rng = np.random.default_rng(7919 * n_valid + int(q * 100))
    test = np.array([-0.5, 0.0, 0.25, 3.0, -2.0], np.float32)
    label = np.array([0, 1, 1, 0, 1], np.uint8)
    off = 0
    for name, valid in _valid_sets(n_valid, q, rng):
        got = _threshold(lib, valid, test, label, q)
        ref = R.threshold_ref(valid, q)
        thr = np.float32(got[0])
        assert float(thr) == got[0], "the threshold is an fp32 value"
        d = R.ulps32(thr, ref)
        assert d <= 1, (n_valid, q, name, thr, ref, d)
        if d:
            off += 1
            print(f"metrics: threshold NOT bit-equal n_valid={n_valid} q={q} {name}: {thr!r} vs {ref!r}")
        want = R.counts_ref(test, label, thr)
        assert _same(got[[0, 2, 3, 4, 5, 6, 7, 8, 9]], np.array(want)[[0, 2, 3, 4, 5, 6, 7, 8, 9]]), (got, want)
        assert _ulps64(got[1], want[1]) <= 2, (got[1], want[1])
    print(f"metrics: threshold n_valid={n_valid} q={q}: 3 inputs, {off} not bit-equal")


TEST_SIZES = [1, 255, 256, 257, 5000]
KINDS = ["equal", "above_all", "below_all", "no_positive"]


@pytest.fixture(scope="module")
def kernel_threshold(lib):
    """A threshold the kernel returned (257 valid scores, q = 0.9), and its inputs."""
    valid = np.random.default_rng(3).normal(size=257).astype(np.float32)
    got = _threshold(lib, valid, np.zeros(1, np.float32), np.zeros(1, np.uint8), 0.9)
    thr = np.float32(got[0])
    assert R.ulps32(thr, R.threshold_ref(valid, 0.9)) <= 1
    return valid, thr


def _test_vector(kind, n, thr, rng):
    s = (thr + rng.normal(size=n)).astype(np.float32)
    lab = (rng.random(n) < 0.3).astype(np.uint8)
    if kind in ("equal", "no_positive"):
        s[::4] = thr                                      # elements 0, 4, 8, ... sit on the threshold
        lab[::8], lab[4::8] = 1, 0                        # with both labels
    if kind == "above_all":                               # the threshold above every score
        s = (thr - 1 - np.abs(s - thr)).astype(np.float32)
    if kind == "below_all":
        s = (thr + 1 + np.abs(s - thr)).astype(np.float32)
    if kind == "no_positive":
        lab[:] = 0
    elif n > 1:
        lab[1] = 1
    return s, lab


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_test", TEST_SIZES)
def test_threshold_counts_at_the_returned_threshold(lib, kernel_threshold, n_test, kind):
    """The ten outputs from integer counts at the kernel's own threshold.  On
    the `equal` vectors test > thr and test >= thr count differently and the
    elements on the threshold carry both labels (one label each way at
    n_test = 1); NaN comes out exactly where a denominator is 0: p, f1 and
    precision with the threshold above every score, r, f1 and recall without
    positives."""
    valid, thr = kernel_threshold
    rng = np.random.default_rng(n_test * 10 + KINDS.index(kind))
    score, lab = _test_vector(kind, n_test, thr, rng)
    variants = [lab] if n_test > 1 else [np.ones(1, np.uint8), np.zeros(1, np.uint8)]
    if kind == "no_positive":
        variants = [lab]
    for label in variants:
        got = _threshold(lib, valid, score, label, 0.9)
        assert np.float32(got[0]) == thr
        want = np.array(R.counts_ref(score, label, thr))
        exact = [0, 2, 3, 4, 5, 6, 7, 8, 9]
        assert _same(got[exact], want[exact]), (kind, n_test, got, want)
        assert _ulps64(got[1], want[1]) <= 2, (got[1], want[1])
        n_gt, n_ge = int((score > thr).sum()), int((score >= thr).sum())
        assert got[6] + got[7] == n_ge and got[6] + got[7] + got[8] + got[9] == n_test
        if kind in ("equal", "no_positive"):
            assert n_ge > n_gt                            # the two rules differ on this vector
            if n_test > 4 and kind == "equal":
                on = score == thr
                assert label[on].min() == 0 and label[on].max() == 1
        if kind == "above_all":
            assert n_ge == 0 and all(math.isnan(got[i]) for i in (1, 2, 4))
            assert got[5] == 0.0 or math.isnan(got[5])
        if kind == "below_all":
            assert n_gt == n_test and got[9] == 0 and got[8] == 0
        if kind == "no_positive":
            assert all(math.isnan(got[i]) for i in (1, 3, 5)) and got[6] == 0 and got[8] == 0


def test_confusion_matrix_takes_the_float64_threshold():
    """metric.get_confusion_matrix counts score >= threshold with the caller's
    float64 threshold, as numpy does on fp32 scores: a threshold strictly
    between two adjacent fp32 values a < b, on scores holding both, counts b and
    not a whichever way the threshold rounds to fp32.  (Rounded to nearest, a
    threshold in the lower half becomes a and a is counted: the defect this
    case found; metric.py rounds up.)  +-1e39 lie outside fp32."""
    a = np.float32(0.3)
    b = np.nextafter(a, np.float32(1))
    rng = np.random.default_rng(4)
    score = np.concatenate(([a, a, b, b, a, b], (a + rng.normal(size=40) * 0.2).astype(np.float32)))
    score = score.astype(np.float32)
    label = np.concatenate(([1, 0, 1, 0, 1, 1], rng.random(40) < 0.4)).astype(bool)
    lo, hi = float(a), float(b)
    thresholds = [lo + 0.25 * (hi - lo), lo + 0.75 * (hi - lo), lo + 0.5 * (hi - lo), lo, hi,
                  np.nextafter(lo, 1.0), np.nextafter(hi, 0.0), 1e39, -1e39, float(score.min()), -0.0]
    assert np.float32(thresholds[0]) == a and np.float32(thresholds[1]) == b
    for t in thresholds:
        pred = score.astype(np.float64) >= t
        tp, fp, fn = int((pred & label).sum()), int((pred & ~label).sum()), int((~pred & label).sum())
        want = (tp / (tp + fp) if tp + fp else math.nan, tp / (tp + fn) if tp + fn else math.nan)
        got = metric.get_confusion_matrix(score, label, t)
        assert _same(got, want), (t, got, want)


def test_f1_score_returns_the_kernels_threshold(lib):
    rng = np.random.default_rng(8)
    valid = rng.normal(size=1003).astype(np.float32)
    score = rng.normal(size=500).astype(np.float32)
    label = rng.random(500) < 0.3
    raw = _threshold(lib, valid, score, label, metric.F1_QUANTILE)
    f1, thr = metric.get_f1_score(valid, score, label)
    assert thr == raw[0] and float(np.float32(thr)) == thr and _same(f1, raw[1])
    assert _same(metric.threshold_metrics(valid, score, label), raw)
    # the argument the reference ignores (utils/metric.py:120) is ignored here too
    assert metric.get_f1_score(valid, score, label, f1_quantiles=(.5,)) == (f1, thr)
    # cached workspace: large, small, large
    metric._ws.clear()
    for n in (100003, 3, 300001, 1):
        v = rng.normal(size=n).astype(np.float32)
        got = metric.threshold_metrics(v, score, label, 0.9)
        assert R.ulps32(np.float32(got[0]), R.threshold_ref(v, 0.9)) <= 1
        assert _same(got[2:], R.counts_ref(score, label, got[0])[2:])


# ------------------------------------------------------ workspace and refusals
@pytest.mark.parametrize("n", [3, 256, 1100003])
def test_workspace_and_out_frames(lib, n):
    """Exactly mmad_*_ws_bytes(n) bytes at a 256-byte aligned address inside a
    sentinel-filled buffer: the bytes before and behind it, and the NaN doubles
    around out[4] / out[10], are unchanged, and every out slot is written."""
    rng = np.random.default_rng(n)
    score = rng.normal(size=n).astype(np.float32)
    lab = (rng.random(n) < 0.3).astype(np.uint8)
    lab[0] = 1
    lab[-1] = 0 if n > 1 else 1
    need = lib.mmad_rank_metrics_ws_bytes(n)
    assert need > 0 and need % 256 == 0
    ws = _Ws(need)
    assert ws.ptr.value % 256 == 0
    got = _rank(lib, score, lab, ws)                      # asserts both frames
    assert not np.isnan(got).any()
    assert not ws.untouched()
    got = _threshold(lib, score, score[:5000], lab[:5000], 0.9)
    assert not np.isnan(got[[0, 6, 7, 8, 9]]).any()
    assert lib.mmad_threshold_metrics_ws_bytes(n) % 256 == 0


def _refused(lib, rc, entry, out, ws):
    torch.cuda.synchronize()
    msg = lib.mmad_last_error_string()
    assert rc == EINVAL, (rc, msg)
    assert entry.encode() in msg, msg
    assert out.untouched() and ws.untouched(), msg
    return msg


def test_rank_refusals_launch_nothing(lib):
    n = 1000
    s = torch.zeros(n, device="cuda")
    lab = torch.zeros(n, dtype=torch.uint8, device="cuda")
    need = lib.mmad_rank_metrics_ws_bytes(n)
    out, ws, st = _Out(4), _Ws(need + 256), stream_ptr()
    f = lib.mmad_rank_metrics
    args = [n, ptr(s), ptr(lab), out.ptr, ws.ptr, need, st]
    for i, v in ((0, 0), (0, 1 << 31), (1, None), (2, None), (3, None), (4, None)):
        bad = list(args)
        bad[i] = v
        assert b"bad arguments" in _refused(lib, f(*bad), "rank_metrics", out, ws)
    bad = list(args)
    bad[5] = need - 1                                     # one byte short
    assert b"workspace" in _refused(lib, f(*bad), "rank_metrics", out, ws)
    bad = list(args)
    bad[4] = ctypes.c_void_p(ws.ptr.value + 64)           # off alignment, long enough
    assert b"aligned" in _refused(lib, f(*bad), "rank_metrics", out, ws)
    assert f(*args) == 0                                  # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert out.read()[3] == n


def test_threshold_refusals_launch_nothing(lib):
    nv, nt = 1000, 100
    v = torch.zeros(nv, device="cuda")
    t = torch.zeros(nt, device="cuda")
    lab = torch.zeros(nt, dtype=torch.uint8, device="cuda")
    need = lib.mmad_threshold_metrics_ws_bytes(nv)
    out, ws, st = _Out(10), _Ws(need), stream_ptr()
    f = lib.mmad_threshold_metrics
    args = [nv, ptr(v), nt, ptr(t), ptr(lab), 0.9, out.ptr, ws.ptr, need, st]
    for i, val in ((0, 0), (0, 1 << 31), (2, 0), (1, None), (3, None), (4, None), (6, None), (7, None),
                   (5, -0.1), (5, 1.1), (5, float("nan"))):
        bad = list(args)
        bad[i] = val
        assert b"bad arguments" in _refused(lib, f(*bad), "threshold_metrics", out, ws)
    bad = list(args)
    bad[8] = need - 1
    assert b"workspace" in _refused(lib, f(*bad), "threshold_metrics", out, ws)
    assert f(*args) == 0
    torch.cuda.synchronize()
    assert out.read()[7] == nt                            # every 0 >= the threshold 0, none labelled: all fp


# ------------------------------------------------------------------ wrappers
def _wrapper_data():
    rng = np.random.default_rng(17)
    widths = (7, 130, 64)
    mk = lambda rows, scale: [(rng.normal(size=(rows, w)) * scale).astype(np.float32) for w in widths]
    train, valid, test = mk(50, 1.0), mk(50, 1.0), mk(50, 1.5)
    label = rng.random(50) < 0.4
    return train, valid, test, label


def _ms64(ds):
    return (np.concatenate([d.astype(np.float64) for d in ds], axis=1) ** 2).mean(axis=1)


def _check_summary(lib, valid_score, loss, label, auroc, aupr, f1, prec, rec):
    """The five metrics are those of the returned fp32 scores."""
    ref = R.rank_ref(loss, label)
    assert auroc == ref["auroc"]
    assert abs(aupr - ref["aupr"]) <= _aupr_k(loss.size) * U53 * ref["aupr"]
    raw = _threshold(lib, valid_score, loss, label, metric.F1_QUANTILE)
    assert R.ulps32(np.float32(raw[0]), R.threshold_ref(valid_score, metric.F1_QUANTILE)) <= 1
    want = R.counts_ref(loss, label, raw[0])
    assert _ulps64(f1, want[1]) <= 2 and _same((prec, rec), (want[4], want[5]))


def test_recon_and_d_loss_wrappers(lib):
    """get_recon_loss (BASE), get_d_loss (SAP) with _clamp's three branches,
    and _mean_sq of a list against the concatenated matrix: scores within 1e-6
    relative of the float64 mean squares (fp32 row sums of at most 201 terms),
    metrics equal to the references' on the returned scores."""
    train, valid, test, label = _wrapper_data()
    cat = np.concatenate(test, axis=1)
    for got in (metric._mean_sq(test), metric._mean_sq(cat), metric._mean_sq(tuple(test))):
        np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), _ms64(test), rtol=1e-6, atol=0)
    # BASE: the last layer's diff matrix
    loss, *m = metric.get_recon_loss(valid[2], test[2], label)
    assert loss.dtype == np.float32 and loss.shape == (50,)
    np.testing.assert_allclose(loss.astype(np.float64), _ms64(test[2:]), rtol=1e-6, atol=0)
    _check_summary(lib, metric._mean_sq(valid[2]).cpu().numpy(), loss, label, *m)
    # SAP: (start, end) -> the layers _clamp keeps (utils/metric.py:155-162)
    assert metric._clamp(3, 0, None) == (0, 4) and metric._clamp(3, 5, None) == (2, 4)
    assert metric._clamp(3, 1, 1) == (1, 2) and metric._clamp(3, 2, 0) == (2, 3) and metric._clamp(3, 0, 2) == (0, 2)
    for (start, end), keep in (((0, None), slice(0, 3)), ((5, None), slice(2, 3)), ((1, 1), slice(1, 2)),
                               ((0, 2), slice(0, 2))):
        loss, *m = metric.get_d_loss(train, valid, test, label, start_layer_index=start, end_layer_index=end)
        np.testing.assert_allclose(loss.astype(np.float64), _ms64(test[keep]), rtol=1e-6, atol=0)
        _check_summary(lib, metric._mean_sq(list(valid[keep])).cpu().numpy(), loss, label, *m)
