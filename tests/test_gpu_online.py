"""Online scoring on the GPU: the 16-row weight-streaming operator
(mmad_fc_rows16), the whole pass (mmad_ae_online_score) and the Python surface
(online.OnlineScorer, NoveltyDetecter.online_scorer).

Models, fit and buffers are those of tests/online_fixture.py (the mm192 golden,
widths [192, 156, 121, 86, 51, 16]).  Figures go to
$MMAD_RECORD_DIR/online.json (default test_records/)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd.data import synth_windows
from tests.online_fixture import (BF16, F32, VARIANTS, X3, _fit, _graphs, _model, _Rig, _sd,
                                  check_fc_rows_against_fp64)

pytestmark = pytest.mark.gpu

_REC = {}


def _record():
    out_dir = os.environ.get("MMAD_RECORD_DIR", "test_records")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "online.json"), "w") as f:
        json.dump(_REC, f, indent=1, default=float)


# ------------------------------------------------- 1. the operator vs fp64 numpy
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "act%d-bn%d-score%d-ref%d-colw%d" % tuple(map(int, v)))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (10, 130, 70), (16, 128, 2048), (7, 100, 6442)])
def test_fc_rows16_against_fp64(M, N, K, dtype, variant):
    """The bars of tests/online_fixture.py::check_fc_rows_against_fp64 on
    mmad_fc_rows16; the figures go to online.json under fc_rows16/..."""
    def record(key, figures):
        _REC[key] = figures
        _record()

    check_fc_rows_against_fp64(16, M, N, K, dtype, variant, record)


# ----------------------------------------------- 2. whole pass vs the fp64 oracle
def _oracle(m, x):
    from oracle import ae_oracle as O
    from oracle.model_io import model_from_state_dict
    om = model_from_state_dict({k: v.cpu().numpy() for k, v in m.state_dict().items()})
    diffs = O.get_diffs(x, om)
    return O.layer_sq_sums(diffs), O.base_score(diffs), O.sap_score(diffs)


@pytest.mark.parametrize("B", [1, 10, 16])
def test_online_pass_against_oracle_f32(golden, B):
    m = _model(golden)
    nat, n = m._native, m._native.n_enc
    x = synth_windows(B, nat.enc_widths[0], seed=61 + B)
    lsq, base, sap = _oracle(m, x)
    rig = _Rig(m)
    xd = torch.from_numpy(x).cuda()
    out, _ = rig.run(xd)
    got = out.double().cpu().numpy()
    assert np.allclose(got[:n + 1, :B], lsq, rtol=1e-4, atol=0)
    assert np.allclose(got[n + 1, :B], base, rtol=1e-4, atol=0)
    assert np.allclose(got[n + 2, :B], sap, rtol=1e-4, atol=0)
    batch = nat.score(xd)[0].double().cpu().numpy()
    assert np.allclose(got[:n + 1, :B], batch, rtol=1e-4, atol=0)
    assert (out[:, B:] == rig.canary).all() and (out[n + 3] == rig.canary).all()   # no fit: NAP untouched
    # a strict SAP sub-range, and the reference's clamping of a degenerate one
    from oracle import ae_oracle as O
    from oracle.model_io import model_from_state_dict
    diffs = O.get_diffs(x, model_from_state_dict({k: v.cpu().numpy() for k, v in m.state_dict().items()}))
    for s_, e_ in ((1, 4), (9, 2)):
        o2, _ = rig.run(xd, start=s_, end=e_)
        assert np.allclose(o2[n + 2, :B].double().cpu().numpy(), O.sap_score(diffs, s_, e_), rtol=1e-4, atol=0)


def test_online_pass_bf16_band(golden):
    """Per layer, the relative Frobenius error of the per-window sums against
    the fp64 oracle < 3e-2: the band of tests/test_gpu_score_c5.py."""
    m = _model(golden, dtype="bf16")
    nat = m._native
    x = synth_windows(16, nat.enc_widths[0], seed=71)
    lsq, _, _ = _oracle(m, x)
    out, _ = _Rig(m).run(torch.from_numpy(x).cuda())
    got = out[:nat.n_enc + 1].double().cpu().numpy()
    for l in range(lsq.shape[0]):
        rel = np.linalg.norm(got[l] - lsq[l]) / np.linalg.norm(lsq[l])
        _REC[f"bf16_layer{l}_rel"] = rel
        assert rel < 3e-2, (l, rel)
    _record()


def test_online_pass_vib(golden):
    torch.manual_seed(5)
    m = _model(golden, models="vib_ae")
    nat = m._native
    assert nat.vib
    xd = torch.from_numpy(synth_windows(10, nat.enc_widths[0], seed=81)).cuda()
    out, _ = _Rig(m).run(xd)
    batch = nat.score(xd)[0]
    assert torch.allclose(out[:nat.n_enc + 1, :10], batch, rtol=1e-4, atol=0)


# --------------------------------------- 3. NAP on the reference-trained weights
def test_online_nap_parity_on_reference_weights(golden):
    """nap_wc golden, seed 0, three well-conditioned ranges -- (1, 5), the widest
    the fixture holds (the full range [0, 6) is not among its well-conditioned
    ones), its strict sub-range (2, 4), and (0, 1), the range fed by pass 1's
    score launch -- through NoveltyDetecter.online_scorer, 16 windows a call.
    Scores of the first 256 test windows within 1e-3 relative of the
    reference's (the bar of tests/test_gpu_nap_wc.py).  Those 256 windows are
    all normal, so an AUROC needs a second class: the first 256 anomalous test
    windows are scored too and the AUROC over the 512 is within 0.002 of the
    AUROC of the reference's scores on the same windows."""
    from icra2021_multimodal_ad_amd import metric
    from icra2021_multimodal_ad_amd.data_loaders import get_loaders
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.novelty_detection import NoveltyDetecter
    g = golden("nap_wc")
    skip = ("meta/torch", "meta/seeds", "meta/min_var_ratio", "meta/members")
    seed, p = 0, "s0/"
    cfg = types.SimpleNamespace(**{k[len("meta/"):]: g[k].item() for k in g.files
                                   if k.startswith("meta/") and k not in skip})
    cfg.gpu_id, cfg.dtype = 0, "f32"
    cfg.data_seed, cfg.sampler_seed, cfg.model_seed = 500 + seed, 600 + seed, 700 + seed
    model = get_model(cfg)
    keys = [str(k) for k in g[p + "state_dict_keys"]]
    model.load_state_dict({k: torch.from_numpy(np.asarray(g[p + f"sd/{k}"])) for k in keys})
    dset, tr, va, te = get_loaders(cfg)
    with torch.no_grad():
        train_x, _ = dset.get_transformed_data(tr)
        valid_x, _ = dset.get_transformed_data(va)
        test_x, _ = dset.get_transformed_data(te)
    label = np.asarray(g[p + "test_label"]).astype(bool)
    rows = np.r_[0:256, np.flatnonzero(label)[:256]]
    assert len(rows) == 512 and not label[:256].any()
    ranges = [tuple(int(v) for v in r) for r in np.asarray(g[p + "ranges"]).reshape(-1, 2)]
    xs = torch.as_tensor(test_x)[torch.from_numpy(rows)].float().cuda()
    rec, bad = {}, []
    for s, e in ((1, 5), (2, 4), (0, 1)):
        assert (s, e) in ranges
        c = types.SimpleNamespace(**vars(cfg))
        c.start_layer_index, c.end_layer_index = s, c.n_layers + 1 - e
        scorer = NoveltyDetecter(c).online_scorer(model, train_x, valid_x)
        ours = torch.cat([scorer.score(xs[i:i + 16])["nap"].clone() for i in range(0, 512, 16)])
        scorer.close()
        ours = ours.double().cpu().numpy()
        ref = np.asarray(g[p + f"nap_{s}_{e}/score"], np.float64)[rows]
        err = float(np.abs(ours[:256] - ref[:256]).max() / np.abs(ref[:256]).max())
        a_ours = metric.rank_metrics(ours, label[rows])[0]
        a_ref = metric.rank_metrics(ref, label[rows])[0]
        rec[f"nap[{s},{e})"] = {"score_rel_err": err, "auroc": a_ours, "auroc_reference_scores": a_ref}
        print(f"\nonline NAP [{s},{e}): score rel err {err:.1e} auroc {a_ours:.5f} vs {a_ref:.5f}")
        if err > 1e-3 or abs(a_ours - a_ref) > 0.002:
            bad.append((s, e, err, a_ours, a_ref))
    _REC["nap_wc"] = rec
    _record()
    assert not bad, bad


# ---------------------------- 4. rows are independent, and the padding is clean
@pytest.fixture(scope="module")
def fitted(golden):
    m = _model(golden)
    sc = _fit(m)
    sc.attach(m, precision="f32", layers=(0, 6))
    yield m, sc
    sc.detach()


def test_rows_are_independent_bitwise(fitted):
    m, _ = fitted
    nat = m._native
    rig = _Rig(m)
    x = torch.from_numpy(synth_windows(16, nat.enc_widths[0], seed=91)).cuda()
    rig.thr.copy_(torch.tensor([0.05, 0.05, 1.0]))
    out16, fl16 = rig.run(x)
    assert torch.isfinite(out16).all()
    for i in range(16):
        o1, f1 = rig.run(x[i:i + 1])
        assert torch.equal(o1[:, 0], out16[:, i]), i
        assert torch.equal(f1[:, 0], fl16[:, i]), i


def test_padding_is_clean_after_a_larger_call(fitted):
    m, _ = fitted
    nat = m._native
    rig = _Rig(m)
    x = torch.from_numpy(synth_windows(16, nat.enc_widths[0], seed=92)).cuda()
    rig.run(x * 1e18)                                   # inf / NaN everywhere a row >= 10 could leak from
    out_a, fl_a = rig.run(x[:10])
    out_b, fl_b = rig.run(x[:10], fresh=True)
    assert torch.isfinite(out_a[:, :10]).all()
    assert torch.equal(out_a, out_b) and torch.equal(fl_a, fl_b)
    assert (out_a[:, 10:] == rig.canary).all() and (fl_a[:, 10:] == 9).all()


# ------------------------------------------------------------------- 5. graph
def test_graph_replay_and_lifecycle(golden):
    m = _model(golden)
    nat = m._native
    sc = _fit(m)
    assert _graphs(nat) == 0
    sc.attach(m, precision="f32", layers=(0, 6))
    rig = _Rig(m)
    x = torch.from_numpy(synth_windows(10, nat.enc_widths[0], seed=93)).cuda()
    eager = rig.run(x)
    assert _graphs(nat) == 0
    first = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    replay = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    for a, b in ((eager, first), (eager, replay)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # other weights and running statistics: a replay reads them when it runs
    g = golden("mm192")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _sd(g, "after0/").items()})
    r2 = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    assert not torch.equal(r2[0], replay[0])
    assert torch.equal(r2[0], rig.run(x)[0])
    m.train()
    m.train_step_async(torch.from_numpy(synth_windows(64, nat.enc_widths[0], seed=94)).cuda())
    m.eval()
    r3 = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    assert not torch.equal(r3[0], r2[0])
    assert torch.equal(r3[0], rig.run(x)[0])
    # the thresholds are read at replay time: only the flags move
    n = nat.n_enc
    rig.thr.copy_(torch.stack([r3[0][n + 1, :10].median(), r3[0][n + 2, :10].median(),
                               r3[0][n + 3, :10].median()]))
    r4 = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    assert torch.equal(r4[0], r3[0]) and not torch.equal(r4[1], r3[1])
    assert (r3[1][:, :10] == 0).all() and 0 < int(r4[1][:, :10].sum()) < 30
    # detach and attach drop the cached online graphs
    sc.detach()
    assert _graphs(nat) == 0
    rig2 = _Rig(m)
    rig2.run(x, graph=True)
    assert _graphs(nat) == 1
    sc.attach(m, precision="f32", layers=(0, 6))
    assert _graphs(nat) == 0
    sc.detach()


def test_online_graph_cache_is_bounded_and_drops_the_oldest(golden):
    """The online graph cache holds 8 passes.  Nine B = 10 passes that differ
    only in the out buffer: 8 cached after the 8th and after the 9th.  The
    first buffer again (dropped: run eagerly and captured anew) leaves 8 and
    equals the use_graph=0 result bit for bit; the 9th buffer again leaves 8,
    so the 9th was cached and the oldest was the one dropped."""
    m = _model(golden)
    nat = m._native
    rig = _Rig(m)
    x = torch.from_numpy(synth_windows(10, nat.enc_widths[0], seed=97)).cuda()
    ref = rig.run(x)[0]
    outs = [torch.full_like(rig.out, rig.canary) for _ in range(9)]

    def run(o):
        o.fill_(rig.canary)
        nat.online_score(rig.x, 10, o, rig.state, flags=rig.flags, thresholds=rig.thr, graph=True)

    assert _graphs(nat) == 0
    for i, o in enumerate(outs):
        run(o)
        assert _graphs(nat) == min(i + 1, 8)
    run(outs[0])
    assert _graphs(nat) == 8
    assert torch.equal(outs[0], ref)
    run(outs[8])
    assert _graphs(nat) == 8
    for o in outs:
        assert torch.equal(o, ref)


# ------------------------------------------------------------------- 6. flags
def test_flags_follow_the_strict_rule(fitted):
    m, _ = fitted
    nat, n = m._native, m._native.n_enc
    rig = _Rig(m)
    x = torch.from_numpy(synth_windows(16, nat.enc_widths[0], seed=95)).cuda()
    out, fl = rig.run(x)
    assert (fl == 0).all()                                             # NaN thresholds: no flag
    base, sap, nap = out[n + 1], out[n + 2], out[n + 3]
    rig.thr.copy_(torch.stack([base[3], torch.tensor(float("nan"), device="cuda"), nap.median()]))
    out2, fl2 = rig.run(x)
    assert torch.equal(out2, out)
    want = torch.stack([base > base[3], torch.zeros_like(sap, dtype=torch.bool), nap > nap.median()])
    assert torch.equal(fl2.bool(), want)
    assert fl2[0, 3] == 0 and fl2[0].sum() > 0 and fl2[2].sum() > 0     # equal to its threshold: no flag


# ---------------------------------------------------- 7. refusals launch nothing
def test_refusals_launch_nothing(golden):
    m = _model(golden, score_dtype="bf16x3")
    nat = m._native
    lib, h, err = nat._lib, nat._h, nat._lib.mmad_last_error_string
    assert nat.score_dtype == X3
    rig = _Rig(m)
    x = torch.from_numpy(synth_windows(10, nat.enc_widths[0], seed=96)).cuda()
    with pytest.raises(_native.NativeError, match="not supported on the online path"):
        rig.run(x)
    # an x3 fit left attached after its score planes went away
    sc = _fit(m)
    sc.attach(m, precision="bf16x3", layers=(0, 6))
    rig = _Rig(m)                                                      # a state sized with the fit
    assert lib.mmad_ae_set_score_planes(h, None) == 0
    assert nat.score_dtype == F32
    with pytest.raises(_native.NativeError, match="MMAD_BF16X3"):
        rig.run(x)
    assert b"fit" in err()
    torch.cuda.synchronize()
    assert (rig.out == rig.canary).all() and (rig.flags == 9).all()
    assert _graphs(nat) == 0
    sc.detach()


# ------------------------------------------- 8. NoveltyDetecter.online_scorer
def test_novelty_detecter_online_scorer(golden):
    """On the mm192 golden's synthetic split.  BASE / SAP of 16 test windows
    equal NoveltyDetecter.scores' at rtol 1e-4.  The full NAP range of this
    model is not one the nap_wc golden calls well-conditioned (that fixture is
    another model), and a rank-deficient fit multiplies fp32 rounding by
    1 / var, so NAP is checked for finiteness and run-to-run bit-equality
    only.  The thresholds are metric.threshold_metrics' on the same
    validation scores."""
    from icra2021_multimodal_ad_amd import metric
    from icra2021_multimodal_ad_amd.novelty_detection import NoveltyDetecter
    g = golden("mm192")
    m = _model(golden)
    cfg = types.SimpleNamespace(n_layers=int(g["meta_n_layers"]), batch_size=int(g["meta_batch"]),
                                start_layer_index=0, end_layer_index=-1, dtype="f32")
    train_x, valid_x = torch.from_numpy(g["score/train_x"]), torch.from_numpy(g["score/valid_x"])
    test_x = torch.from_numpy(g["score/test_x"])[:16]
    det = NoveltyDetecter(cfg)
    scorer = det.online_scorer(m, train_x, valid_x)
    got = {k: (v.clone() if v is not None else None) for k, v in scorer.score(test_x).items()}
    again = scorer.score(test_x)
    thr = scorer.thresholds.cpu().numpy()
    scorer.close()
    ref = det.scores(m, train_x, valid_x, test_x)
    for k in ("base", "sap"):
        assert torch.allclose(got[k], ref[k][1], rtol=1e-4, atol=0), k
    assert torch.isfinite(got["nap"]).all() and torch.equal(got["nap"], again["nap"])
    for i, k in enumerate(("base", "sap", "nap")):
        want = np.float32(metric.threshold_metrics(ref[k][0], ref[k][0][:1], np.zeros(1, np.uint8))[0])
        assert thr[i] == want, (k, thr[i], want)
    assert torch.equal(got["flags"].bool(), torch.stack([got[k] > float(thr[i])
                                                         for i, k in enumerate(("base", "sap", "nap"))]))
    with pytest.raises(ValueError, match="score_windows"):
        scorer.score(torch.zeros(17, test_x.shape[1]))
