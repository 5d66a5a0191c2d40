"""Per-modality scores from the online pass (mmad_ae_online_score_groups,
OnlineScorer(groups=...)) and the batch route (group_scores) on the GPU.

Models are the mm192 golden of tests/online_fixture.py (widths [192, 156, 121,
86, 51, 16]); its input row is cut into four groups at columns no multiple of
4, and into two groups that leave both ends of the row out."""
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd.data import synth_windows
from icra2021_multimodal_ad_amd.online import OnlineScorer
from icra2021_multimodal_ad_amd.reconstruction_aggregation import group_scores
from tests.online_fixture import _fit, _graphs, _model

pytestmark = pytest.mark.gpu

GROUPS = {"a": (0, 101), "b": (101, 107), "c": (107, 171), "d": (171, 192)}   # covers the row
BOUNDS = [0, 101, 107, 171, 192]
INNER = [(3, 64), (64, 190)]
THR = {"base": 0.05, "sap": 0.05, "nap": 1.0, "groups": {"a": 0.05, "b": 0.01, "c": -1.0}}   # d: NaN


@pytest.fixture(scope="module")
def models(golden):
    return {"f32": _model(golden), "bf16": _model(golden, dtype="bf16")}


@pytest.fixture(scope="module")
def fits(models):
    """fits of the fp32 model's diffs: over every diff layer, and from layer 1 up"""
    return {"full": _fit(models["f32"], (0, 6)), "from1": _fit(models["f32"], (1, 6))}


@pytest.fixture(scope="module")
def windows(models):
    return torch.from_numpy(synth_windows(64, models["f32"]._native.enc_widths[0], seed=301)).cuda()


def _scorer(m, fits, route, rows, groups=None, thresholds=THR):
    """route: 'nofit' (d0 into the groups buffer), 'full' (d0 in the fit's
    operand), 'from1' (a fit whose range starts above layer 0: the buffer)."""
    thr = dict(thresholds)
    if groups is None:
        thr.pop("groups", None)
    nap = None if route == "nofit" else fits[route]
    return OnlineScorer(m, nap, start_layer_index=1 if route == "from1" else 0, thresholds=thr, rows=rows,
                        groups=groups)


def _keep(res):
    return {k: v.clone() for k, v in res.items() if v is not None}


# ------------------------------------------------------ 5. nothing existing moves
@pytest.mark.parametrize("route", ["nofit", "full", "from1"])
@pytest.mark.parametrize("rows", [16, 64])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_pass_leaves_the_ungrouped_outputs_bitwise(models, fits, windows, dtype, rows, route):
    """out and flags of a grouped pass equal those of an ungrouped pass on a
    fresh scorer, for each of the three places d0 can come from; then the two
    scorers take turns on the one handle for three calls each, through the
    shared graph cache, and each keeps its own results."""
    m = models[dtype]
    B = 10 if rows == 16 else 40
    x = windows[:B]
    plain = _scorer(m, fits, route, rows)
    want = _keep(plain.score(x))
    plain.close()
    assert "groups" not in want and "group_flags" not in want
    grouped = _scorer(m, fits, route, rows, groups=GROUPS)
    got = _keep(grouped.score(x))
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert got["groups"].shape == (4, B) and got["group_flags"].shape == (4, B)
    assert torch.isfinite(got["groups"]).all() and (got["groups"] > 0).all()
    plain = _scorer(m, fits, route, rows)
    m._native._lib.mmad_ae_clear_graphs(m._native._h)
    for turn in range(3):
        a = _keep(plain.score(x))
        b = _keep(grouped.score(x))
        assert 1 <= _graphs(m._native) <= 2
        for k in want:
            assert torch.equal(a[k], want[k]) and torch.equal(b[k], want[k]), (turn, k)
        assert torch.equal(b["groups"], got["groups"]) and torch.equal(b["group_flags"], got["group_flags"])
    assert _graphs(m._native) == 2
    plain.close()
    grouped.close()


def test_grouped_and_ungrouped_passes_never_share_a_graph(models, windows):
    """The same x, out, flags, thresholds and state through the raw entry
    points: an ungrouped replay must not write the group outputs, a grouped
    one must, and other bounds on the same buffers are another pass."""
    nat = models["f32"]._native
    x = windows[:16].contiguous()
    out = torch.zeros((nat.n_enc + 4, 16), device="cuda")
    state, gstate = nat.online_state(16), nat.online_groups_state(16)
    gout = torch.zeros((4, 16), device="cuda")
    nat._lib.mmad_ae_clear_graphs(nat._h)
    seen = {}
    for turn in range(3):
        for name, bounds in (("plain", None), ("grouped", BOUNDS), ("shifted", [1, 100, 108, 170, 191])):
            gout.fill_(-5.0)
            nat.online_score(x, 10, out, state, groups=bounds, group_out=gout, groups_state=gstate)
            torch.cuda.synchronize()
            if bounds is None:
                assert (gout == -5.0).all(), turn
            else:
                assert (gout[:, :10] > 0).all() and (gout[:, 10:] == 0).all(), (turn, name)
                assert torch.equal(seen.setdefault(name, gout.clone()), gout), (turn, name)
    assert not torch.equal(seen["grouped"], seen["shifted"])
    assert _graphs(nat) == 3
    nat._lib.mmad_ae_clear_graphs(nat._h)


# --------------------------------------------------- 6. the group scores are right
def _check_cover(res, D):
    """sum_g w_g groups[g] against layer_sq[0] of the same pass: two fixed-order
    fp32 sums of the same D non-negative terms, each within (D + 2) 2^-24."""
    w = torch.tensor([c1 - c0 for c0, c1 in GROUPS.values()], dtype=torch.float64)
    total = (res["groups"].double().cpu() * w[:, None]).sum(0)
    lsq0 = res["layer_sq"][0].double().cpu()
    assert torch.allclose(total, lsq0, rtol=2 * (D + 2) * 2.0 ** -24, atol=0)


@pytest.mark.parametrize("case", ["f32", "vib"])
def test_online_groups_against_the_batch_route_f32(golden, models, windows, case):
    """B = 10: online 'groups' against group_scores at the bar
    tests/test_gpu_online.py holds the online layer_sq to the batch route's
    (rtol 1e-4, atol 0); the VIB golden model is one case."""
    if case == "vib":
        torch.manual_seed(5)
        m = _model(golden, models="vib_ae")
        assert m._native.vib
    else:
        m = models["f32"]
    x = windows[:10]
    sc = OnlineScorer(m, groups=GROUPS)
    res = _keep(sc.score(x))
    batch = group_scores(x, m, GROUPS)
    assert batch.shape == (4, 10)
    assert torch.allclose(res["groups"], batch, rtol=1e-4, atol=0)
    assert torch.equal(group_scores(x, m, BOUNDS), batch)
    assert torch.allclose(group_scores(x, m, BOUNDS, batch_size=4), batch, rtol=1e-4, atol=0)   # 4, 4, 2
    _check_cover(res, 192)
    # groups that leave both ends of the row out
    inner = _keep(OnlineScorer(m, groups=INNER).score(x))
    assert torch.allclose(inner["groups"], group_scores(x, m, INNER), rtol=1e-4, atol=0)


def test_online_groups_bf16_band(models, windows):
    """The bf16 handle: per group, the relative Frobenius error of the online
    scores against the batch route's < 3e-2 (the bf16 band of
    tests/test_gpu_online.py); the cover identity is dtype-blind (d0 is fp32)."""
    m = models["bf16"]
    x = windows[:10]
    res = _keep(OnlineScorer(m, groups=GROUPS).score(x))
    batch = group_scores(x, m, GROUPS).double().cpu().numpy()
    got = res["groups"].double().cpu().numpy()
    for g in range(4):
        rel = np.linalg.norm(got[g] - batch[g]) / np.linalg.norm(batch[g])
        print(f"bf16 group {g}: rel {rel:.3e}")
        assert rel < 3e-2, (g, rel)
    _check_cover(res, 192)


# ------------------------------------------------------- 7. bitwise across routes
def test_group_scores_are_bitwise_across_routes(models, fits, windows):
    m = models["f32"]
    sc16 = _scorer(m, fits, "nofit", 16, groups=GROUPS)
    sc64 = _scorer(m, fits, "nofit", 64, groups=GROUPS)
    assert sc16.group_names == ("a", "b", "c", "d") and sc16.groups == BOUNDS
    # thresholds that bite: the medians of groups a and b; c negative, d NaN
    med = sc16.score(windows[:16])["groups"].median(dim=1).values.cpu()
    thr = {"groups": {"a": float(med[0]), "b": float(med[1]), "c": -1.0}}
    sc16.set_thresholds(thr)
    sc64.set_thresholds(thr)
    r16 = _keep(sc16.score(windows[:16]))
    assert 0 < int(r16["group_flags"][:2].sum()) < 32                 # the thresholds bite
    assert (r16["group_flags"][2] == 1).all() and (r16["group_flags"][3] == 0).all()   # -1.0 and NaN
    for B in (17, 64):
        r64 = _keep(sc64.score(windows[:B]))
        assert torch.equal(r64["groups"][:, :16], r16["groups"])
        assert torch.equal(r64["group_flags"][:, :16], r16["group_flags"])
    for i in (0, 9, 15):
        r1 = sc16.score(windows[i:i + 1])
        assert torch.equal(r1["groups"][:, 0], r16["groups"][:, i]), i
        assert torch.equal(r1["group_flags"][:, 0], r16["group_flags"][:, i]), i
    for i in (16, 40, 63):
        r1 = sc16.score(windows[i:i + 1])
        assert torch.equal(r1["groups"][:, 0], r64["groups"][:, i]), i
    # the batch route forms d0 in another GEMM: the bar of test 6, not bits
    assert torch.allclose(group_scores(windows, m, GROUPS), r64["groups"], rtol=1e-4, atol=0)
    # with the fit's operand as the source of d0 (another leading dimension)
    scf = _scorer(m, fits, "full", 64, groups=GROUPS)
    scf.set_thresholds(thr)
    rf = scf.score(windows)
    assert torch.equal(rf["groups"], r64["groups"]) and torch.equal(rf["group_flags"], r64["group_flags"])
    scf.close()
    # padding: after B = 64, a B = 3 call leaves rows 3..63 zero (scores and
    # flags, whatever the threshold: group c's is negative)
    sc64.score(windows)
    sc64.score(windows[:3])
    torch.cuda.synchronize()
    assert (sc64.group_out[:, 3:] == 0).all() and (sc64.group_flags[:, 3:] == 0).all()
    assert (sc64.group_out[:, :3] > 0).all() and (sc64.group_flags[2, :3] == 1).all()


# ------------------------------------------------------------ 8. score_frames
def test_score_frames_with_the_modality_columns(tmp_path):
    """HSR_Net on the recordings of tests/hsr_fixture.py, 40 frames, a 1728-wide
    model: four named groups whose widths sum to 1728, equal to score() on the
    fused rows, and covering layer_sq[0]."""
    from icra2021_multimodal_ad_amd import hsr_dataset as H
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from tests.hsr_fixture import CASES, SHUFFLE_SEED, write_recordings
    folder, img = write_recordings(str(tmp_path))
    cfg = types.SimpleNamespace(data_folder_name=folder, image_root=img, gpu_id=0, data_seed=SHUFFLE_SEED,
                                **CASES["All"])
    torch.manual_seed(7)
    net = HSR_Net(False, cfg).cuda()
    ins = H.TabularDataset(cfg, hsr_net=net).inputs
    r, d, t, mm = ins["r"], ins["d"], ins["t"], ins["m"]
    torch.manual_seed(8)
    model = get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                            models="ae"))
    cols = net.modality_columns()
    sc = OnlineScorer(model, rows=64, groups=cols)
    assert sc.group_names == ("r", "d", "t", "m")
    assert sum(c1 - c0 for c0, c1 in cols.values()) == 1728 and sc.groups == [0, 1024, 1536, 1600, 1728]
    a = _keep(sc.score_frames(net, r, d, t, mm))
    b = sc.score(net.forward(r, d, None, t, mm).reshape(40, -1))
    assert a["groups"].shape == (4, 40) and torch.isfinite(a["groups"]).all() and (a["groups"] > 0).all()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    w = torch.tensor([c1 - c0 for c0, c1 in cols.values()], dtype=torch.float64)
    total = (a["groups"].double().cpu() * w[:, None]).sum(0)
    assert torch.allclose(total, a["layer_sq"][0].double().cpu(), rtol=2 * (1728 + 2) * 2.0 ** -24, atol=0)


# --------------------------------------------------------------- 9. calibrate
def test_calibrate_with_a_groups_entry(models, windows):
    from icra2021_multimodal_ad_amd import metric
    m = models["f32"]
    sc = OnlineScorer(m, groups=GROUPS)
    assert torch.isnan(sc.group_thresholds).all()
    first = _keep(sc.score(windows[:16]))
    assert (first["group_flags"] == 0).all()                          # NaN thresholds: no flag
    valid = group_scores(windows, m, GROUPS).cpu().numpy()            # [4, 64]
    q = 0.7
    thr = sc.calibrate({"base": first["base"], "groups": {n: valid[i] for i, n in enumerate("abcd") if n != "d"}},
                       q=q)
    got = sc.group_thresholds.cpu().numpy()
    for i, n in enumerate("abc"):
        want = np.float32(np.quantile(valid[i].astype(np.float64), q))
        assert got[i] == want and np.float32(thr["groups"][n]) == want, (n, got[i], want)
    assert np.isnan(got[3])
    res = sc.score(windows[:16])                                      # the replayed graph reads them
    assert torch.equal(res["groups"], first["groups"])
    assert torch.equal(res["group_flags"].bool(), res["groups"] > sc.group_thresholds[:, None])
    assert 0 < int(res["group_flags"][:3].sum()) < 48 and (res["group_flags"][3] == 0).all()
    # the default quantile is metric.threshold_metrics'
    sc.calibrate({"groups": {"a": valid[0]}})
    want = np.float32(metric.threshold_metrics(torch.from_numpy(valid[0]), torch.from_numpy(valid[0][:1]),
                                               np.zeros(1, np.uint8))[0])
    assert sc.group_thresholds.cpu().numpy()[0] == want


# ---------------------------------------------------- refusals launch nothing
def test_grouped_refusals_launch_nothing(models, windows):
    nat = models["f32"]._native
    x = windows[:32]                                                  # rows enough for the B = 17 refusal
    out = torch.full((nat.n_enc + 4, 16), -7.0, device="cuda")
    gout = torch.full((4, 16), -7.0, device="cuda")
    state, gstate = nat.online_state(16), nat.online_groups_state(16)
    graphs = _graphs(nat)

    def run(bounds, word, go=gout, gs=gstate, B=10):
        g = torch.full((len(bounds) - 1, 16), -7.0, device="cuda") if go is gout and len(bounds) != 5 else go
        with pytest.raises(_native.NativeError, match=word):
            nat.online_score(x, B, out, state, groups=bounds, group_out=g, groups_state=gs)

    run([0], "G=0 outside 1..8")
    run(list(range(0, 100, 10)), "G=9 outside 1..8")
    run([0, 100, 50, 192, 192], "bounds not strictly ascending")
    run([0, 101, 107, 171, 193], r"bounds\[G\]=193 exceeds the input width D=192")
    run(BOUNDS, "null group_out", go=None)
    run(BOUNDS, "gstate null or too small", gs=None)
    run(BOUNDS, "gstate null or too small", gs=gstate[:1024])
    run(BOUNDS, "outside 1..16", B=17)
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (gout == -7.0).all() and _graphs(nat) == graphs


# ------------------------------------------- NoveltyDetecter.online_scorer
def test_novelty_detecter_passes_the_modality_columns_on():
    """config.online_groups on a 1728-wide model: four modality groups, their
    thresholds the quantile of the batch route's group scores of valid_x;
    absent (the default) or on another input width: no groups."""
    from icra2021_multimodal_ad_amd import metric
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.novelty_detection import NoveltyDetecter
    torch.manual_seed(8)
    model = get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                            models="ae"))
    model.eval()
    # NAP and SAP over the last diff layer alone (16 columns): a small fit
    cfg = types.SimpleNamespace(n_layers=3, batch_size=64, start_layer_index=3, end_layer_index=-1, dtype="f32",
                                online_groups=True)
    train_x = torch.from_numpy(synth_windows(96, 1728, seed=401))
    valid_x = torch.from_numpy(synth_windows(48, 1728, seed=402))
    scorer = NoveltyDetecter(cfg).online_scorer(model, train_x, valid_x)
    assert scorer.group_names == ("r", "d", "t", "m") and scorer.groups == [0, 1024, 1536, 1600, 1728]
    valid = group_scores(valid_x.cuda(), model, scorer.groups)
    got = scorer.group_thresholds.cpu().numpy()
    for g in range(4):
        want = np.float32(metric.threshold_metrics(valid[g], valid[g][:1], np.zeros(1, np.uint8))[0])
        assert got[g] == want, (g, got[g], want)
    res = scorer.score(valid_x[:10])
    assert torch.equal(res["group_flags"].bool(), res["groups"] > scorer.group_thresholds[:, None])
    assert torch.allclose(res["groups"], valid[:, :10], rtol=1e-4, atol=0)
    scorer.close()
    cfg.online_groups = False
    plain = NoveltyDetecter(cfg).online_scorer(model, train_x, valid_x)
    assert plain.groups is None and "groups" not in plain.score(valid_x[:10])
    plain.close()
    small = _cfg_model_192()
    cfg192 = types.SimpleNamespace(n_layers=5, batch_size=64, start_layer_index=5, end_layer_index=-1, dtype="f32",
                                   online_groups=True)
    x192 = torch.from_numpy(synth_windows(96, 192, seed=403))
    sc = NoveltyDetecter(cfg192).online_scorer(small, x192, x192[:48])
    assert sc.groups is None                                          # not the fused width: off
    sc.close()


def _cfg_model_192():
    from icra2021_multimodal_ad_amd.model_builder import get_model
    torch.manual_seed(9)
    m = get_model(types.SimpleNamespace(input_size=192, btl_size=16, n_layers=5, gpu_id=0, dtype="f32", models="ae"))
    m.eval()
    return m
