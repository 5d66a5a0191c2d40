"""Online scoring on the GPU: the 16-row weight-streaming operator
(mmad_fc_rows16), the whole pass (mmad_ae_online_score) and the Python surface
(online.OnlineScorer, NoveltyDetecter.online_scorer).

Models follow tests/test_gpu_nap_stream.py::_model: the mm192 golden, widths
[192, 156, 121, 86, 51, 16] -- no layer width is a multiple of 16 and the diff
columns of the NAP operand start at odd offsets.  Figures go to
$MMAD_RECORD_DIR/online.json (default test_records/)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import call, pad, ptr, stream_ptr
from icra2021_multimodal_ad_amd.data import synth_windows

pytestmark = pytest.mark.gpu

F32, BF16, X3 = 0, 1, 2
_REC = {}


def _record():
    out_dir = os.environ.get("MMAD_RECORD_DIR", "test_records")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "online.json"), "w") as f:
        json.dump(_REC, f, indent=1, default=float)


def _sd(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def _model(golden, dtype="f32", score_dtype=None, step=None, models="ae"):
    from icra2021_multimodal_ad_amd.model_builder import get_model
    g = golden("mm192")
    cfg = types.SimpleNamespace(input_size=int(g["meta_d"]), btl_size=int(g["meta_btl"]),
                                n_layers=int(g["meta_n_layers"]), gpu_id=0, dtype=dtype, models=models)
    if score_dtype is not None:
        cfg.score_dtype = score_dtype
    m = get_model(cfg)
    if models == "ae":
        step = int(g["meta_steps"]) - 1 if step is None else step
        sd = _sd(g, f"after{step}/")
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m.eval()
    return m


def _fit(m, rng_=(0, 6), n_train=300, seed=11):
    """A NapScorer fitted on the model's own train diffs of the layer range."""
    from icra2021_multimodal_ad_amd.reconstruction_aggregation import NapScorer
    nat = m._native
    cuts = np.cumsum([0] + nat.diff_widths())
    c0, c1 = int(cuts[rng_[0]]), int(cuts[rng_[1]])
    xt = torch.from_numpy(synth_windows(n_train, nat.enc_widths[0], seed=seed)).cuda()
    train = nat.score(xt, want_diffs=True)[1][:, c0:c1].contiguous()
    return NapScorer.standalone(c1 - c0, device=nat.device).fit(train_diffs=train)


class _Rig:
    """Fixed buffers for raw mmad_ae_online_score calls on one model."""

    def __init__(self, m, canary=-7.0):
        self.nat = nat = m._native
        self.canary = canary
        self.x = torch.zeros((16, nat.enc_widths[0]), device="cuda")
        self.out = torch.full((nat.n_enc + 4, 16), canary, device="cuda")
        self.flags = torch.full((3, 16), 9, device="cuda", dtype=torch.uint8)
        self.thr = torch.full((3,), float("nan"), device="cuda")
        self.state = nat.online_state()

    def run(self, x, graph=False, start=0, end=None, fresh=False):
        B = x.shape[0]
        self.x[:B].copy_(x)
        self.out.fill_(self.canary)
        self.flags.fill_(9)
        if fresh:
            self.state = self.nat.online_state()
        self.nat.online_score(self.x, B, self.out, self.state, flags=self.flags, thresholds=self.thr,
                              start=start, end=end, graph=graph)
        torch.cuda.synchronize()
        return self.out.clone(), self.flags.clone()


def _graphs(nat):
    return nat._lib.mmad_ae_graph_count(nat._h)


# ------------------------------------------------- 1. the operator vs fp64 numpy
def _vec(v, Np):
    if v is None:
        return None
    p = torch.zeros(Np, device="cuda")
    p[:v.numel()] = v
    return p


# (act, BN affine, score epilogue, ref, colw)
VARIANTS = [(0, False, False, False, False), (1, True, False, False, False), (1, True, True, True, False),
            (0, False, True, False, True), (1, False, True, True, True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "act%d-bn%d-score%d-ref%d-colw%d" % tuple(map(int, v)))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (10, 130, 70), (16, 128, 2048), (7, 100, 6442)])
def test_fc_rows16_against_fp64(M, N, K, dtype, variant):
    """max |err| / (sum_k |a||b| + |bias|) (carried through the BN affine, the
    measure of tests/test_gpu_x3.py) of mmad_fc_rows16 at most twice the same
    figure of the parent's mmad_fc_fwd / mmad_fc_fwd_score on the same
    operands: both are fp32 accumulations that differ only in association.
    With the score epilogue the figure is taken on the diff output.  Exact:
    rows >= M of y are zero, rows >= M / columns >= N are absent from rowsq,
    the canaries around diff's written region are intact; rowsq itself equals
    the fp64 sum of colw d^2 over each tile's columns of the kernel's own diff
    within 8 * 2^-24 relative (two products per term and a 4-level tree of
    non-negative fp32 adds)."""
    act, affine, score, use_ref, use_colw = variant
    rng = np.random.default_rng(1000 * M + 10 * N + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, N).astype(np.float32) if affine else None
    sh = (0.1 * rng.standard_normal(N)).astype(np.float32) if affine else None
    rf = rng.standard_normal((M, N)).astype(np.float32) if use_ref else None
    cw = rng.uniform(0.5, 2.0, N).astype(np.float32) if use_colw else None
    tdt = torch.float32 if dtype == F32 else torch.bfloat16
    if rf is not None:
        rf = torch.from_numpy(rf).to(tdt).float().numpy()          # representable in the operand dtype
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    z = x64 @ w64.T + b
    ref = np.where(z > 0, z, 0.2 * z) if act == 1 else z
    den = np.abs(x64) @ np.abs(w64).T + np.abs(b)
    if affine:
        ref = ref * sc + sh
        den = den * np.abs(sc) + np.abs(sh)
    if use_ref:
        ref = ref - rf
    Mp, Kp, Np = pad(M), pad(K), pad(N)
    s = stream_ptr()
    dx, dw = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    x16 = torch.empty((16, Kp), device="cuda", dtype=tdt)
    xin = torch.empty((Mp, Kp), device="cuda", dtype=tdt)
    wp = torch.empty((Np, Kp), device="cuda", dtype=tdt)
    call("mmad_pack_input", dtype, M, K, 16, Kp, ptr(dx), K, ptr(x16), s)
    call("mmad_pack_input", dtype, M, K, Mp, Kp, ptr(dx), K, ptr(xin), s)
    call("mmad_pack_input", dtype, N, K, Np, Kp, ptr(dw), K, ptr(wp), s)
    bp, scp, shp, cwp = (_vec(None if v is None else torch.from_numpy(v).cuda(), Np) for v in (b, sc, sh, cw))
    refp = None
    if use_ref:
        refp = torch.zeros((Mp, Np), device="cuda", dtype=tdt)
        refp[:M, :N] = torch.from_numpy(rf).cuda().to(tdt)
    # the parent's kernel on the same operands
    yp = torch.empty((Mp, Np), device="cuda", dtype=tdt)
    if use_ref:
        rsq = torch.empty((Np // 128, Mp), device="cuda")
        dparent = torch.zeros((M, N), device="cuda")
        call("mmad_fc_fwd_score", dtype, M, N, K, Mp, Np, Kp, ptr(xin), ptr(wp), ptr(bp), act, 0.2, ptr(scp),
             ptr(shp), ptr(yp), ptr(refp), ptr(rsq), ptr(dparent), N, s)
        parent = dparent.double().cpu().numpy()
    else:
        call("mmad_fc_fwd", dtype, M, N, K, Mp, Np, Kp, ptr(xin), ptr(wp), ptr(bp), act, 0.2, ptr(scp),
             ptr(shp), ptr(yp), None, s)
        parent = yp[:M, :N].double().cpu().numpy()
    # the 16-row operator; diff sits inside a canary frame at an odd column
    y = torch.full((17, Np), 5.0, device="cuda", dtype=tdt)
    ld, c0 = N + 7, 3
    diff = torch.full((18, ld), 77.0, device="cuda")
    rowsq = torch.full((Np // 16 + 1, 16), 55.0, device="cuda")
    call("mmad_fc_rows16", dtype, M, N, K, Np, Kp, ptr(x16), ptr(wp), ptr(bp), act, 0.2, ptr(scp), ptr(shp),
         ptr(y), ptr(refp), dtype, Np, ptr(diff[0, c0:]) if score else None, ld, ptr(cwp),
         ptr(rowsq) if score else None, s)
    torch.cuda.synchronize()
    got = (diff[:M, c0:c0 + N] if score else y[:M, :N]).double().cpu().numpy()
    e_new = float((np.abs(got - ref) / den).max())
    e_old = float((np.abs(parent - ref) / den).max())
    key = f"fc_rows16/{'bf16' if dtype == BF16 else 'f32'}/{M}x{N}x{K}/" + "".join(str(int(v)) for v in variant)
    _REC[key] = {"rows16": e_new, "parent": e_old}
    _record()
    print(f"\n{key}: rows16 {e_new:.3e} parent {e_old:.3e}")
    assert (y[M:16] == 0).all() and (y[:16, N:] == 0).all() and (y[16] == 5.0).all()
    if score:
        assert (diff[M:16, c0:c0 + N] == 0).all()                     # rows >= M: written as zero
        assert (diff[:, :c0] == 77.0).all() and (diff[:, c0 + N:] == 77.0).all() and (diff[16:] == 77.0).all()
        assert (rowsq[-1] == 55.0).all()
        rs = rowsq[:-1].double().cpu().numpy()                        # [tiles][16]
        assert (rs[:, M:] == 0).all()
        d = np.zeros((16, Np))
        d[:M, :N] = got
        wgt = np.ones(Np) if cw is None else np.r_[cw.astype(np.float64), np.zeros(Np - N)]
        want = ((d * d * wgt).reshape(16, Np // 16, 16).sum(-1)).T    # columns >= N: d = 0
        assert (rs[N // 16 + 1:] == 0).all()
        assert np.all(np.abs(rs - want) <= 8 * 2.0 ** -24 * want + 1e-300)
    else:
        assert (rowsq == 55.0).all() and (diff == 77.0).all()
    assert e_new <= 2 * e_old


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
