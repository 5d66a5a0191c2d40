"""tests/metrics_ref.py against sklearn and numpy (no GPU), wherever those are
defined: the GPU tests (tests/test_gpu_metrics.py) compare the kernels with a
reference that is itself checked here, and then take it where sklearn does
not go (infinite scores)."""
import math
import warnings

import numpy as np
import pytest
from sklearn import metrics as skm

from tests import metrics_ref as R


def _cases():
    rng = np.random.default_rng(11)
    out = []
    for n in (2, 37, 257, 1000, 5000):
        s = rng.normal(size=n).astype(np.float32)
        lab = rng.random(n) < 0.3
        lab[0], lab[1] = True, False
        out.append((f"distinct{n}", s, lab))
        out.append((f"ties{n}", np.round(s, 1).astype(np.float32), lab))
    s = rng.normal(size=300).astype(np.float32)
    out.append(("no_positive", s, np.zeros(300, bool)))
    out.append(("all_positive", s, np.ones(300, bool)))
    out.append(("no_positive_ties", np.round(s, 1).astype(np.float32), np.zeros(300, bool)))
    out.append(("all_positive_ties", np.round(s, 1).astype(np.float32), np.ones(300, bool)))
    out.append(("all_tied", np.full(64, 0.25, np.float32), rng.random(64) < 0.5))
    out.append(("all_tied_no_positive", np.full(9, -3.0, np.float32), np.zeros(9, bool)))
    out.append(("all_tied_all_positive", np.full(9, -3.0, np.float32), np.ones(9, bool)))
    z = np.array([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0], np.float32)
    out.append(("signed_zeros", z, np.array([1, 0, 0, 1, 1, 0], bool)))
    return out


@pytest.mark.parametrize("name,score,label", _cases(), ids=[c[0] for c in _cases()])
def test_rank_ref_matches_sklearn(name, score, label):
    """AUROC = auc(roc_curve) and AUPR = auc(precision_recall_curve) to
    1e-12; with one class sklearn's AUROC is NaN (it warns) and so is ours;
    AUPR is 0.5 without positives and 1.0 with positives only."""
    r = R.rank_ref(score, label)
    assert r["P"] == int(label.sum()) and r["N"] == int((~label).sum())
    assert r["U"] * 2 == int(r["U"] * 2) and (r["terms"] >= 0).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, _ = skm.roc_curve(label, score)
        pr, rc, _ = skm.precision_recall_curve(label, score)
        sk_auroc, sk_aupr = skm.auc(fpr, tpr), skm.auc(rc, pr)
    if r["P"] and r["N"]:
        assert abs(r["auroc"] - sk_auroc) <= 1e-12, (r["auroc"], sk_auroc)
    else:
        assert math.isnan(r["auroc"]) and math.isnan(sk_auroc)
    assert abs(r["aupr"] - sk_aupr) <= 1e-12, (r["aupr"], sk_aupr)
    if r["P"] == 0:
        assert r["aupr"] == 0.5
    if r["N"] == 0:
        assert r["aupr"] == 1.0


def test_rank_ref_brute_force_on_special_values():
    """Where sklearn refuses (inf): U against the O(n^2) definition, on a
    vector with both zeros, denormals, FLT_MIN, FLT_MAX and the infinities."""
    fi = np.finfo(np.float32)
    s = np.array([-np.inf, -fi.max, -2.5, -fi.tiny, -1e-45, -0.0, 0.0, 1e-45, fi.tiny, 2.5, fi.max, np.inf,
                  0.0, -0.0, 2.5, -np.inf], np.float32)
    lab = np.array([1, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0], bool)
    r = R.rank_ref(s, lab)
    d = s.astype(np.float64)
    u = sum((d[j] < d[i]) + 0.5 * (d[j] == d[i]) for i in np.flatnonzero(lab) for j in np.flatnonzero(~lab))
    assert r["U"] == u and r["auroc"] == u / (r["P"] * r["N"])
    with pytest.raises(ValueError):
        R.rank_ref(np.array([1.0, np.nan], np.float32), [0, 1])


def test_counts_ref_matches_sklearn_confusion_matrix():
    rng = np.random.default_rng(5)
    for n in (1, 37, 1000):
        s = np.round(rng.normal(size=n), 1).astype(np.float32)
        lab = rng.random(n) < 0.4
        for thr in (np.float32(0.1), np.float32(-0.5), s[0], np.float32(9.0), np.float32(-9.0)):
            out = R.counts_ref(s, lab, thr)
            tn, fp, fn, tp = skm.confusion_matrix(lab, s >= thr, labels=[False, True]).ravel()
            assert out[6:] == (tp, fp, fn, tn)
            assert out[0] == float(thr)
            pred = s > thr
            hit = int((pred & lab).sum())
            for got, num, den in ((out[2], hit, int(pred.sum())), (out[3], hit, int(lab.sum())),
                                  (out[4], tp, tp + fp), (out[5], tp, tp + fn)):
                assert (math.isnan(got) and den == 0) or got == num / den
            if not math.isnan(out[2]) and not math.isnan(out[3]) and out[2] + out[3] > 0:
                assert out[1] == out[2] * out[3] * 2 / (out[2] + out[3])
            else:
                assert math.isnan(out[1])


def test_threshold_ref_is_the_float64_rule_and_numpy_fp32_path_differs():
    """threshold_ref equals the kernel's rule restated in numpy float64
    (virtual index q (n - 1), numpy's _lerp with its switch at g = 0.5, one
    rounding to fp32) in every case; numpy's own fp32 path (np.quantile of a
    float32 array) is another rule: the count and the largest distance are
    printed, not bounded."""
    rng = np.random.default_rng(0)
    qs = (0.0, 0.5, 0.9, 0.99, 1.0)
    differ, worst, cases = 0, 0, 0
    for n in range(1, 400):
        v = rng.normal(size=n).astype(np.float32)
        srt = np.sort(v).astype(np.float64)
        for q in qs:
            ref = R.threshold_ref(v, q)
            vi = q * (n - 1)
            lo = min(max(int(math.floor(vi)), 0), n - 1)
            hi = min(lo + 1, n - 1)
            g = vi - lo
            a, b = srt[lo], srt[hi]
            rule = np.float32(b - (b - a) * (1.0 - g) if g >= 0.5 else a + (b - a) * g)
            assert rule == ref, (n, q, rule, ref)
            d = R.ulps32(np.quantile(v, q), ref)
            differ += d != 0
            worst = max(worst, d)
            cases += 1
    print(f"numpy fp32 quantile path differs from threshold_ref in {differ} of {cases} cases, "
          f"by up to {worst} fp32 ulps")
    assert cases == 1995


def test_ulps32():
    one = np.float32(1.0)
    assert R.ulps32(one, np.nextafter(one, np.float32(2))) == 1
    assert R.ulps32(np.float32(-0.0), np.float32(0.0)) == 0
    assert R.ulps32(np.float32(-1e-45), np.float32(1e-45)) == 2
