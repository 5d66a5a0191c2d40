"""References for the device metrics (csrc/mmad_metrics.hip: mmad_rank_metrics,
mmad_threshold_metrics) in plain numpy float64 and integer counts, without
sklearn, so that they are defined where sklearn refuses the input (infinite
scores) and exact where the kernels are exact.  tests/test_metrics_reference.py
holds them to sklearn on a machine without a GPU wherever sklearn is defined.

Scores are fp32 values; -0.0 is +0.0 (one tie run); equal scores form one run
(np.unique).  NaN scores are outside these references, as they are outside
the reference implementation's sklearn."""
import math

import numpy as np


def _scores(score):
    s = np.asarray(score, dtype=np.float32).reshape(-1).astype(np.float64)
    if np.isnan(s).any():
        raise ValueError("NaN scores have no defined rank")
    return s + 0.0           # -0.0 + 0.0 = +0.0


def _labels(label):
    return np.asarray(label).reshape(-1) != 0


def rank_ref(score, label):
    """dict(U, auroc, terms, aupr, P, N):
      U      sum over positives of (#negatives strictly below + 1/2 #negatives
             tied): a Python float holding an exact integer or half-integer
             (2 U is formed in int64)
      auroc  U / (P N), NaN when P N = 0
      terms  (R_j - R_{j-1}) (P_j + P_{j-1}) / 2 per distinct score in
             descending order, (R, P)_{-1} = (0, 1), R = 1 without positives;
             each term is formed in float64 from the integer counts by
             precision = tp / count, recall = tp / P
      aupr   math.fsum(terms)
      P, N   the numbers of positive and negative labels (ints)."""
    s, lab = _scores(score), _labels(label)
    if s.size != lab.size or s.size == 0:
        raise ValueError("score and label need the same positive length")
    _, inv = np.unique(s, return_inverse=True)
    inv = inv.reshape(-1)
    runs = int(inv.max()) + 1
    pos = np.bincount(inv[lab], minlength=runs).astype(np.int64)      # ascending score order
    neg = np.bincount(inv[~lab], minlength=runs).astype(np.int64)
    P, N = int(pos.sum()), int(neg.sum())
    neg_below = np.cumsum(neg) - neg
    U = int((pos * (2 * neg_below + neg)).sum()) / 2.0                 # < n^2 < 2^52: exact
    auroc = U / (float(P) * float(N)) if P > 0 and N > 0 else math.nan
    tp = np.cumsum(pos[::-1]).astype(np.float64)                       # descending thresholds
    cnt = np.cumsum((pos + neg)[::-1]).astype(np.float64)
    prec = tp / cnt
    rec = tp / float(P) if P > 0 else np.ones_like(tp)
    prec_p = np.concatenate(([1.0], prec[:-1]))
    rec_p = np.concatenate(([0.0], rec[:-1]))
    terms = (rec - rec_p) * (prec + prec_p) * 0.5
    return dict(U=U, auroc=auroc, terms=terms, aupr=math.fsum(terms.tolist()), P=P, N=N)


def threshold_ref(valid, q):
    """numpy's linear quantile taken in float64, rounded once to fp32."""
    v = np.asarray(valid, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.float32(np.quantile(v, float(q)))


def _ratio(a, b):
    return a / b if b > 0 else math.nan


def counts_ref(test, label, thr):
    """The ten outputs of threshold_k at the fp32 threshold `thr`, from
    integer counts: (thr, f1, p, r, precision, recall, tp, fp, fn, tn) with
    p, r from test > thr, the confusion matrix from test >= thr, and NaN where
    a denominator is 0 (f1 = p r 2 / (p + r) is NaN with either, and 0 / 0)."""
    t = np.asarray(test, dtype=np.float32).reshape(-1)
    lab = _labels(label)
    thr = np.float32(thr)
    gt, ge = t > thr, t >= thr
    n_gt, gt_pos, n_ge, ge_pos, pos = (int(x.sum()) for x in (gt, gt & lab, ge, ge & lab, lab))
    p, r = _ratio(gt_pos, n_gt), _ratio(gt_pos, pos)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = float(np.float64(p) * np.float64(r) * 2.0 / (np.float64(p) + np.float64(r)))
    tp, fp, fn = ge_pos, n_ge - ge_pos, pos - ge_pos
    tn = t.size - n_ge - fn
    return (float(thr), f1, p, r, _ratio(tp, tp + fp), _ratio(tp, tp + fn), float(tp), float(fp),
            float(fn), float(tn))


def ulps32(a, b):
    """Distance in fp32 steps between two finite fp32 values (+-0 coincide)."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))
