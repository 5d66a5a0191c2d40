"""64-row online scoring on the GPU: the multi-row-tile weight-streaming
operator (mmad_fc_rows64), the whole pass (mmad_ae_online_score64) and the
Python surface (OnlineScorer(rows=64), NoveltyDetecter.online_scorer).

The design constraint is bit equality with the 16-row path: a row's
accumulator sees the same products in the same order, so every comparison
against mmad_fc_rows16 / mmad_ae_online_score below is torch.equal.  Models,
the fitted NAP and the buffers are those of tests/online_fixture.py (the
mm192 golden)."""
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, pad, ptr, stream_ptr
from icra2021_multimodal_ad_amd.data import synth_windows
from tests.online_fixture import (BF16, F32, VARIANTS, X3, _fit, _graphs, _model, _Rig, _vec,
                                  check_fc_rows_against_fp64)

pytestmark = pytest.mark.gpu


# ------------------------------------ 1. the operator's rows vs the 16-row kernel
# (act, BN affine, score epilogue, fp32 ref + colw + diff at a column offset)
ROW_VARIANTS = {"fwd": (0, False, False, False), "leaky-bn": (1, True, False, False),
                "score-ref": (1, True, True, False), "score-f32ref-colw-diff": (1, False, True, True)}


def _operands(N, K, dtype, wide, seed):
    """64 rows of operands, packed; ref in the operand dtype (ldref = Np) or, for
    the `wide` variant, fp32 at an odd row stride."""
    rng = np.random.default_rng(seed)
    tdt = torch.float32 if dtype == F32 else torch.bfloat16
    Kp, Np = pad(K), pad(N)
    s = stream_ptr()
    o = types.SimpleNamespace(tdt=tdt, Kp=Kp, Np=Np)
    o.x = torch.from_numpy(rng.standard_normal((64, K)).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)).cuda()
    o.wp = torch.empty((Np, Kp), device="cuda", dtype=tdt)
    call("mmad_pack_input", dtype, N, K, Np, Kp, ptr(w), K, ptr(o.wp), s)
    o.bias = _vec(torch.from_numpy((0.1 * rng.standard_normal(N)).astype(np.float32)).cuda(), Np)
    o.scale = _vec(torch.from_numpy(rng.uniform(0.5, 1.5, N).astype(np.float32)).cuda(), Np)
    o.shift = _vec(torch.from_numpy((0.1 * rng.standard_normal(N)).astype(np.float32)).cuda(), Np)
    o.colw = _vec(torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).cuda(), Np)
    rf = torch.from_numpy(rng.standard_normal((64, N)).astype(np.float32)).cuda()
    o.ldref = N + 5 if wide else Np
    o.ref = torch.zeros((64, o.ldref), device="cuda", dtype=torch.float32 if wide else tdt)
    o.ref[:, :N] = rf.to(o.ref.dtype)
    o.ref_dtype = F32 if wide else dtype
    return o


def _rows_call(fn, rows, dtype, M, N, K, o, x, variant, row0, canary_rows):
    """One mmad_fc_rows16 / mmad_fc_rows64 call on packed x [rows][Kp]; the
    reference rows start at row0.  Outputs sit in canary frames."""
    act, affine, score, wide = variant
    c0 = 3 if wide else 0
    ld = o.Np + 7
    y = torch.full((rows + canary_rows, o.Np), 5.0, device="cuda", dtype=o.tdt)
    diff = torch.full((rows + canary_rows, ld), 77.0, device="cuda")
    rowsq = torch.full((o.Np // 16 + 1, rows), 55.0, device="cuda")
    call(fn, dtype, M, N, K, o.Np, o.Kp, ptr(x), ptr(o.wp), ptr(o.bias), act, 0.2,
         ptr(o.scale) if affine else None, ptr(o.shift) if affine else None, ptr(y),
         ptr(o.ref[row0:]) if score else None, o.ref_dtype, o.ldref,
         ptr(diff[0, c0:]) if wide else None, ld, ptr(o.colw) if wide else None,
         ptr(rowsq) if score else None, stream_ptr())
    return y, diff, rowsq


@pytest.mark.parametrize("variant", list(ROW_VARIANTS), ids=list(ROW_VARIANTS))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 48, 64])
@pytest.mark.parametrize("N,K", [(1, 1), (130, 70), (100, 896), (16, 2048)])
def test_fc_rows64_rows_equal_fc_rows16_bitwise(N, K, M, dtype, variant):
    """Row tile t of a 64-row call equals mmad_fc_rows16 on rows 16t..16t+15
    with M_t = min(16, M - 16t) valid rows, bit for bit, in y, diff and rowsq;
    rows [M, 64) of y and diff are zero; nothing past row 63 is written.
    Shapes: one K chunk (three waves idle), a column tail inside a 16-column
    tile, chunk counts not divisible by the 4 waves."""
    v = ROW_VARIANTS[variant]
    _, _, score, wide = v
    o = _operands(N, K, dtype, wide, seed=10000 * N + 10 * K + dtype)
    x64 = torch.empty((64, o.Kp), device="cuda", dtype=o.tdt)
    call("mmad_pack_input", dtype, M, K, 64, o.Kp, ptr(o.x), K, ptr(x64), stream_ptr())
    y, diff, rowsq = _rows_call("mmad_fc_rows64", 64, dtype, M, N, K, o, x64, v, 0, 2)
    torch.cuda.synchronize()
    c0 = 3 if wide else 0
    for t in range(4):
        Mt = min(16, M - 16 * t)
        r = slice(16 * t, 16 * t + 16)
        if Mt < 1:                               # a tile that is not computed: written as zero
            assert (y[r] == 0).all()
            if score:
                assert (rowsq[:-1, r] == 0).all()
            if wide:
                assert (diff[r, c0:c0 + N] == 0).all()
            continue
        y16, d16, rs16 = _rows_call("mmad_fc_rows16", 16, dtype, Mt, N, K, o, x64[r], v, 16 * t, 0)
        torch.cuda.synchronize()
        assert torch.equal(y[r], y16), t
        assert torch.equal(diff[r], d16), t
        assert torch.equal(rowsq[:, r], rs16), t
    assert (y[M:64] == 0).all() and (y[:64, N:] == 0).all()
    assert (y[64:] == 5.0).all() and (diff[64:] == 77.0).all() and (rowsq[-1] == 55.0).all()
    if wide:
        assert (diff[M:64, c0:c0 + N] == 0).all()
        assert (diff[:, :c0] == 77.0).all() and (diff[:, c0 + N:] == 77.0).all()
    else:
        assert (diff == 77.0).all()
    if not score:
        assert (rowsq == 55.0).all()
    else:
        assert (rowsq[:-1, M:] == 0).all() and torch.isfinite(rowsq).all()


# ------------------------------------------- 2. the operator on its own vs fp64
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "act%d-bn%d-score%d-ref%d-colw%d" % tuple(map(int, v)))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(40, 130, 70), (64, 100, 896)])
def test_fc_rows64_against_fp64(M, N, K, dtype, variant):
    """The bars of tests/test_gpu_online.py::test_fc_rows16_against_fp64
    (tests/online_fixture.py::check_fc_rows_against_fp64) on the 64-row layouts."""
    check_fc_rows_against_fp64(64, M, N, K, dtype, variant)


# ------------------------------------- 3. the whole pass vs the 16-row pass, bits
def _by_groups_of_16(rig16, x, **kw):
    """The 16-row pass over x's windows in groups of 16: (out [n+4, B], flags [3, B])."""
    outs, fls = [], []
    for i in range(0, x.shape[0], 16):
        g = x[i:i + 16]
        o, f = rig16.run(g, **kw)
        outs.append(o[:, :g.shape[0]])
        fls.append(f[:, :g.shape[0]])
    return torch.cat(outs, 1), torch.cat(fls, 1)


@pytest.fixture(scope="module")
def nap_fit(golden):
    """The fit of tests/test_gpu_online.py::fitted (full range of the fp32 golden
    model), unattached: its numbers also serve the bf16 handle."""
    return _fit(_model(golden))


HANDLES = {"f32-nap": dict(dtype="f32", fit=True), "f32-nofit": dict(dtype="f32", fit=False),
           "f32-nap-sap1to4": dict(dtype="f32", fit=True, start=1, end=4),
           "bf16-nap": dict(dtype="bf16", fit=True), "vib": dict(dtype="f32", fit=False, models="vib_ae")}


@pytest.mark.parametrize("handle", list(HANDLES), ids=list(HANDLES))
def test_online_pass64_equals_the_16_row_pass_bitwise(golden, nap_fit, handle):
    """B in {1, 16, 17, 40, 64}: every window's layer_sq, BASE, SAP, NAP and
    flags from mmad_ae_online_score64 equal the same window's from
    mmad_ae_online_score on its 16-window group; columns >= B of out and flags
    keep their fill."""
    spec = HANDLES[handle]
    torch.manual_seed(5)
    m = _model(golden, dtype=spec["dtype"], models=spec.get("models", "ae"))
    nat, n = m._native, m._native.n_enc
    if spec["fit"]:
        nap_fit.attach(m, precision="f32", layers=(0, 6))
    try:
        r16, r64 = _Rig(m, 16), _Rig(m, 64)
        kw = dict(start=spec.get("start", 0), end=spec.get("end"))
        xs = torch.from_numpy(synth_windows(64, nat.enc_widths[0], seed=191)).cuda()
        # thresholds that split the windows: the medians of the first 16 (NAP: with a fit)
        o16 = r16.run(xs[:16], **kw)[0]
        thr = torch.stack([o16[n + 1].median(), o16[n + 2].median(),
                           o16[n + 3].median() if spec["fit"] else o16[n + 1].median()])
        r16.thr.copy_(thr)
        r64.thr.copy_(thr)
        for B in (1, 16, 17, 40, 64):
            want_o, want_f = _by_groups_of_16(r16, xs[:B], **kw)
            out, fl = r64.run(xs[:B], **kw)
            assert torch.isfinite(out[:n + 3, :B]).all(), B
            assert torch.equal(out[:, :B], want_o), B
            assert torch.equal(fl[:, :B], want_f), B
            assert (out[:, B:] == r64.canary).all() and (fl[:, B:] == 9).all(), B
            if not spec["fit"]:
                assert (out[n + 3] == r64.canary).all()           # no fit: NAP untouched
        assert 0 < int(fl[0].sum()) < 64                          # the thresholds split the windows
    finally:
        nap_fit.detach()


# -------------------------------------------------------------- 4. lifecycle
@pytest.fixture()
def fitted(golden, nap_fit):
    m = _model(golden)
    nap_fit.attach(m, precision="f32", layers=(0, 6))
    yield m
    nap_fit.detach()


def test_padding_is_clean_after_a_64_window_call(fitted):
    rig = _Rig(fitted, 64)
    x = torch.from_numpy(synth_windows(64, rig.nat.enc_widths[0], seed=192)).cuda()
    rig.run(x * 1e18)                                   # inf / NaN everywhere a row >= 3 could leak from
    out_a, fl_a = rig.run(x[:3])
    out_b, fl_b = rig.run(x[:3], fresh=True)
    assert torch.isfinite(out_a[:, :3]).all()
    assert torch.equal(out_a, out_b) and torch.equal(fl_a, fl_b)
    assert (out_a[:, 3:] == rig.canary).all() and (fl_a[:, 3:] == 9).all()


def test_graph_replay_equals_eager(fitted):
    nat = fitted._native
    rig = _Rig(fitted, 64)
    x = torch.from_numpy(synth_windows(40, nat.enc_widths[0], seed=193)).cuda()
    assert _graphs(nat) == 0
    eager = rig.run(x)
    assert _graphs(nat) == 0
    first = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    replay = rig.run(x, graph=True)
    assert _graphs(nat) == 1
    for a, b in ((eager, first), (eager, replay)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_16_and_64_row_scorers_alternate_on_one_handle(fitted):
    """Two states on one handle, taking turns through the shared graph cache:
    each call equals its own eager result, whatever ran before it; more call
    signatures than the cache holds (8) never push the count past the bound."""
    nat = fitted._native
    r16, r64 = _Rig(fitted, 16), _Rig(fitted, 64)
    x = torch.from_numpy(synth_windows(64, nat.enc_widths[0], seed=194)).cuda()
    sizes16, sizes64 = (10, 16, 3, 7, 12), (10, 16, 40, 64, 17)       # B = 10 and 16 on both
    ref16 = {B: r16.run(x[:B]) for B in sizes16}
    ref64 = {B: r64.run(x[:B]) for B in sizes64}
    assert _graphs(nat) == 0
    for rnd in range(2):                                              # capture, then replay or re-capture
        for B16, B64 in zip(sizes16, sizes64):
            o, f = r16.run(x[:B16], graph=True)
            assert torch.equal(o, ref16[B16][0]) and torch.equal(f, ref16[B16][1]), (rnd, B16)
            assert 1 <= _graphs(nat) <= 8
            o, f = r64.run(x[:B64], graph=True)
            assert torch.equal(o, ref64[B64][0]) and torch.equal(f, ref64[B64][1]), (rnd, B64)
            assert 1 <= _graphs(nat) <= 8
    assert _graphs(nat) == 8
    # the same windows through both: the 64-row scores are the 16-row bits
    assert torch.equal(ref64[10][0][:, :10], ref16[10][0][:, :10])


def test_refusals_launch_nothing(golden, nap_fit):
    m = _model(golden, score_dtype="bf16x3")
    nat = m._native
    lib, h, err = nat._lib, nat._h, nat._lib.mmad_last_error_string
    assert nat.score_dtype == X3
    rig = _Rig(m, 64)
    x = torch.from_numpy(synth_windows(40, nat.enc_widths[0], seed=195)).cuda()
    with pytest.raises(_native.NativeError, match="not supported on the online path"):
        rig.run(x)
    # an x3 fit left attached after its score planes went away
    nap_fit.attach(m, precision="bf16x3", layers=(0, 6))
    try:
        rig = _Rig(m, 64)                                              # a state sized with the fit
        assert lib.mmad_ae_set_score_planes(h, None) == 0
        assert nat.score_dtype == F32
        with pytest.raises(_native.NativeError, match="MMAD_BF16X3"):
            rig.run(x)
        assert b"fit" in err()
        with pytest.raises(_native.NativeError, match="outside 1..64"):
            nat.online_score(torch.zeros((65, nat.enc_widths[0]), device="cuda"), 65, rig.out, rig.state,
                             rows=64)
        torch.cuda.synchronize()
        assert (rig.out == rig.canary).all() and (rig.flags == 9).all()
        assert _graphs(nat) == 0
    finally:
        nap_fit.detach()


# ------------------------------------------------------------------ 5. Python
def test_online_scorer_rows64_equals_three_16_row_calls(golden, nap_fit):
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    m = _model(golden)
    x = torch.from_numpy(synth_windows(40, m._native.enc_widths[0], seed=196))
    thr = {"base": 0.05, "sap": 0.05, "nap": 1.0}
    keys = ("layer_sq", "base", "sap", "nap", "flags")
    sc16 = OnlineScorer(m, nap_fit, thresholds=thr)
    parts = []
    for i in (0, 16, 32):
        parts.append({k: v.clone() for k, v in sc16.score(x[i:i + 16]).items()})
    sc16.close()
    want = {k: torch.cat([p[k] for p in parts], dim=-1) for k in keys}
    sc64 = OnlineScorer(m, nap_fit, thresholds=thr, rows=64)
    got = sc64.score(x)
    again = {k: v.clone() for k, v in got.items()}
    for k in keys:
        assert got[k].shape[-1] == 40 and torch.equal(got[k], want[k]), k
    got = sc64.score(x.cuda())                                        # the replayed graph
    for k in keys:
        assert torch.equal(got[k], again[k]), k
    with pytest.raises(ValueError, match="score_windows"):
        sc64.score(torch.zeros(65, x.shape[1]))
    sc64.close()


def test_score_frames_of_40_frames(golden, tmp_path):
    """HSR_Net(slicing_size = 40) on the recordings of tests/hsr_fixture.py:
    score_frames fuses straight into the scorer's input buffer and equals
    score(hsr_net.forward(...))."""
    from icra2021_multimodal_ad_amd import hsr_dataset as H
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    from tests.hsr_fixture import CASES, SHUFFLE_SEED, write_recordings
    folder, img = write_recordings(str(tmp_path))
    cfg = types.SimpleNamespace(data_folder_name=folder, image_root=img, gpu_id=0, data_seed=SHUFFLE_SEED,
                                **CASES["All"])
    assert cfg.slicing_size == 40
    torch.manual_seed(7)
    net = HSR_Net(False, cfg).cuda()
    ins = H.TabularDataset(cfg, hsr_net=net).inputs
    r, d, t, mm = ins["r"], ins["d"], ins["t"], ins["m"]
    torch.manual_seed(8)
    model = get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                            models="ae"))
    sc = OnlineScorer(model, rows=64)
    a = {k: v.clone() for k, v in sc.score_frames(net, r, d, t, mm).items() if v is not None}
    b = sc.score(net.forward(r, d, None, t, mm).reshape(40, -1))
    assert a["base"].shape == (40,) and torch.isfinite(a["base"]).all() and (a["base"] > 0).all()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="score_windows"):
        OnlineScorer(model).score_frames(net, r, d, t, mm)            # 40 frames > the default 16 rows


def test_novelty_detecter_picks_64_rows_for_40_windows(golden):
    """slicing_size = 40 -> a 64-row scorer; BASE / SAP of 40 test windows equal
    NoveltyDetecter.scores' at rtol 1e-4 and NAP is finite and repeatable (the
    bars of tests/test_gpu_online.py::test_novelty_detecter_online_scorer, for
    its reasons)."""
    from icra2021_multimodal_ad_amd.novelty_detection import NoveltyDetecter
    g = golden("mm192")
    m = _model(golden)
    cfg = types.SimpleNamespace(n_layers=int(g["meta_n_layers"]), batch_size=int(g["meta_batch"]),
                                start_layer_index=0, end_layer_index=-1, dtype="f32", slicing_size=40)
    train_x, valid_x = torch.from_numpy(g["score/train_x"]), torch.from_numpy(g["score/valid_x"])
    test_x = torch.from_numpy(g["score/test_x"])[:40]
    assert test_x.shape[0] == 40
    det = NoveltyDetecter(cfg)
    scorer = det.online_scorer(m, train_x, valid_x)
    assert scorer.rows == 64
    got = {k: (v.clone() if v is not None else None) for k, v in scorer.score(test_x).items()}
    again = scorer.score(test_x)
    thr = scorer.thresholds.cpu().numpy()
    scorer.close()
    ref = det.scores(m, train_x, valid_x, test_x)
    for k in ("base", "sap"):
        assert torch.allclose(got[k], ref[k][1], rtol=1e-4, atol=0), k
    assert torch.isfinite(got["nap"]).all() and torch.equal(got["nap"], again["nap"])
    assert torch.equal(got["flags"].bool(), torch.stack([got[k] > float(thr[i])
                                                         for i, k in enumerate(("base", "sap", "nap"))]))
    with pytest.raises(ValueError, match="score_windows"):
        scorer.score(torch.zeros(65, test_x.shape[1]))
