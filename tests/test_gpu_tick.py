"""The sensor tick on the GPU: mmad_hsr_fuse_raw against mmad_hsr_fuse on
torch-normalised inputs, and OnlineScorer.tick (one copy + one replayed graph,
mmad_ae_online_tick) against score_sensors, bit for bit.

Shapes are those of test_gpu_mfcc's score_sensors test: the fused HSR_Net
(seed 7), the 1728-wide 3-layer fp32 autoencoder (seed 8), the "deploy" PCM
case (11 frames) for B = 10 and the same signal recipe at 19 frames for
B = 17."""
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from tests.test_mfcc_abi import CASES, case_pcm, signal

pytestmark = pytest.mark.gpu

keep = lambda res: {k: v.clone() for k, v in res.items() if v is not None}   # noqa: E731


def norm_vec_torch(v, lo, hi):
    """data_loaders.norm_vec to [-1, 1], the expression normalised_sensors evaluates."""
    return (2 * (v - lo) / (hi - lo)) + -1


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def model():
    from icra2021_multimodal_ad_amd.model_builder import get_model
    torch.manual_seed(8)
    return get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                           models="ae"))


@pytest.fixture
def graphs(model):
    """() -> the handle's cached graph count; the cache starts empty (it holds
    8 passes and drops the oldest: a count taken on a full one cannot rise)."""
    lib, h = _native.load(), model._native._h
    assert lib.mmad_ae_clear_graphs(h) == 0
    return lambda: int(lib.mmad_ae_graph_count(h))


def make_net(B):
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    torch.manual_seed(7)
    return HSR_Net(False, types.SimpleNamespace(slicing_size=B, batch_size=B, gpu_id=0)).cuda()


@pytest.fixture(scope="module")
def pcm():
    """B -> int16 samples: "deploy" (11 frames) for B <= 11, else its recipe at 19 frames."""
    long = signal(**dict(CASES["deploy"][3], L=18 * 4410))
    return lambda B: case_pcm("deploy") if B <= 11 else long


def queues(B, seed, y, roll=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    hand_q = rng.integers(0, 256, size=(B, 32 * 32 * 3)).astype(np.uint8)
    depth_q = rng.integers(0, 256, size=(B, 32 * 32)).astype(np.uint8)
    force_q = rng.uniform(0, 400, size=B)
    y = np.roll(y, roll)
    mic_q = [y[i:i + 4096].tobytes() for i in range(0, len(y), 4096)]
    return force_q, hand_q, depth_q, mic_q


# ---- 1: the kernel against mmad_hsr_fuse on normalised inputs ------------------
@pytest.fixture(scope="module")
def raw_case():
    """n = 3 windows holding 0, 255, a pixel outside the range (fp32 only) and
    forces 0, 400, 512; the packed weights; m in [-1, 1]."""
    n = 3
    rng = np.random.Generator(np.random.PCG64(5))
    r = rng.integers(0, 256, size=(n, 3072)).astype(np.uint8)
    d = rng.integers(0, 256, size=(n, 1024)).astype(np.uint8)
    r[0, :2], r[2, -2:], d[1, :2], d[2, -2:] = (0, 255), (255, 0), (255, 0), (0, 255)
    t = np.array([0.0, 400.0, 512.0], dtype=np.float32)
    m = rng.uniform(-1, 1, size=(n, 13)).astype(np.float32)
    m[0, 0], m[1, 12] = -1.0, 1.0
    return dict(n=n, r=r, d=d, t=t, m=torch.from_numpy(m).cuda(), w=make_net(n).packed_weights())


def division_is_correctly_rounded(samples):
    """Whether torch's device quotient by a Python scalar is the IEEE quotient
    (torch on the host divides; a device kernel may multiply by 1 / b)."""
    for v, b in samples:
        if not torch.equal((v.cuda() / b).cpu(), v / b):
            return False
    return True


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_fuse_raw_is_fuse_on_normalised_inputs(raw_case, kind):
    """Measured on the MI355X with torch 2.10: see DESIGN.md §4 "Sensor tick in
    one graph" for which reference the device's division selected."""
    c, n = raw_case, raw_case["n"]
    if kind == "u8":
        r_h, d_h, code = torch.from_numpy(c["r"]), torch.from_numpy(c["d"]), _native.SRC_U8
    else:
        r_h, d_h, code = torch.from_numpy(c["r"]).float(), torch.from_numpy(c["d"]).float(), _native.SRC_F32
        r_h[1, 7], d_h[0, 9] = 300.5, 300.5                      # outside [0, 255]
    t_h = torch.from_numpy(c["t"])
    r_f, d_f = r_h.float(), d_h.float()
    # the reference: norm_vec in torch on the device, then mmad_hsr_fuse; where the
    # device's division by a scalar is not the correctly rounded quotient, the same
    # expression evaluated by torch on the host and uploaded
    on_device = division_is_correctly_rounded([(2 * r_f, 255), (2 * d_f, 255), (2 * t_h, 400)])
    print(f"fuse_raw {kind}: torch's device division is {'the' if on_device else 'NOT the'} correctly rounded quotient")
    up = (lambda v: v.cuda()) if on_device else (lambda v: v)
    rn = norm_vec_torch(up(r_f), 0, 255).cuda()
    dn = norm_vec_torch(up(d_f), 0, 255).cuda()
    tn = norm_vec_torch(up(t_h), 0, 400).cuda()
    assert float(rn.min()) == -1.0 and float(tn[1]) == 1.0 and float(tn[2]) > 1.0
    if kind == "f32":
        assert float(rn.max()) > 1.0
    r_d, d_d, t_d = r_h.cuda(), d_h.cuda(), t_h.cuda()
    ptr, SENT = _native.ptr, -777.0
    sel = {"fused": (0, "rdtm", 1728), "r": (1, "r", 1024), "d": (1, "d", 512), "t": (1, "t", 64), "m": (1, "m", 128)}
    for name, (unimodal, has, width) in sel.items():
        for pad in (0, 5):
            pick = lambda k, v: v if k in has else None   # noqa: E731
            ref = torch.full((n, width + pad), SENT, device="cuda")
            got = torch.full((n, width + pad), SENT, device="cuda")
            _native.call("mmad_hsr_fuse", n, ptr(pick("r", rn)), ptr(pick("d", dn)), ptr(pick("t", tn)),
                         ptr(pick("m", c["m"])), ptr(c["w"]), unimodal, ptr(ref), width + pad, _native.stream_ptr())
            _native.call("mmad_hsr_fuse_raw", n, ptr(pick("r", r_d)), code, ptr(pick("d", d_d)), code,
                         ptr(pick("t", t_d)), ptr(pick("m", c["m"])), 0.0, 255.0, 0.0, 255.0, 0.0, 400.0, ptr(c["w"]),
                         unimodal, ptr(got), width + pad, _native.stream_ptr())
            diff = int((ref != got).sum())
            print(f"  {name:5s} ld_out = width + {pad}: {diff} of {ref.numel()} values differ")
            assert torch.equal(ref, got), (kind, name, pad)
            assert (got[:, width:] == SENT).all() and (got[:, :width] != SENT).all()


# ---- 2: tick against score_sensors ----------------------------------------------
CASES_TICK = {"b10_rows16_groups": (10, 16, True), "b17_rows64": (17, 64, False)}


def scorer(model, net, rows, grouped):
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    return OnlineScorer(model, rows=rows, groups=net.modality_columns() if grouped else None)


@pytest.mark.parametrize("case", list(CASES_TICK))
def test_tick_is_score_sensors(model, graphs, pcm, case):
    """score_sensors normalises with torch on the device, whose division by a
    Python scalar is (MI355X, torch 2.10) a product with the rounded reciprocal;
    bind_sensors probes that and has the tick form the quotient the same way
    (OnlineScorer.norm_division).  With the IEEE quotient instead, 4903 of 17280
    fused values differ in the last place at B = 10 and 8529 of 29376 at B = 17
    (DESIGN.md §4 "Sensor tick in one graph")."""
    B, rows, grouped = CASES_TICK[case]
    net, y = make_net(B), pcm(B)
    q = queues(B, 81, y)
    sc = scorer(model, net, rows, grouped)
    want = keep(sc.score_sensors(net, *q))
    row = sc.x[:B].clone()
    sc.x.zero_()
    sc.bind_sensors(net, len(y))
    got = keep(sc.tick(*q))
    bad = int((row != sc.x[:B]).sum())
    print(f"tick {case}: {bad} of {row.numel()} fused values differ from score_sensors' row; "
          f"base max |diff| {float((got['base'] - want['base']).abs().max()):.3e}")
    assert {"base", "sap", "layer_sq", "flags"} <= set(got) and ("groups" in got) == grouped
    assert torch.equal(row, sc.x[:B])
    same(got, want)


def ieee_frames(force_q, hand_q, depth_q, mic_q, B):
    """score_frames' inputs with norm_vec evaluated by torch on the host (a true
    fp32 division) and uploaded; m from the front end."""
    from icra2021_multimodal_ad_amd.mfcc import MfccFrontEnd
    f32 = lambda q: torch.from_numpy(np.asarray(q, dtype=np.float32))   # noqa: E731
    r = norm_vec_torch(f32(hand_q).view(-1, 1, 3, 32, 32), 0, 255).cuda()
    d = norm_vec_torch(f32(depth_q).view(-1, 1, 1, 32, 32), 0, 255).cuda()
    t = norm_vec_torch(f32(force_q), 0, 400).cuda()
    return r, d, t, MfccFrontEnd().latest(mic_q, B)[1]


@pytest.mark.parametrize("case", list(CASES_TICK))
def test_tick_is_score_frames_on_host_normalised_streams(model, graphs, pcm, case):
    """norm_division = "ieee": the tick against the same pass fed by hand with IEEE-normalised streams:
    every key and the fused row bit for bit, on a first call, on a replay with
    other queue contents and after refresh_sensors -- one graph throughout."""
    B, rows, grouped = CASES_TICK[case]
    net, y = make_net(B), pcm(B)
    sc = scorer(model, net, rows, grouped)
    sc.norm_division = "ieee"
    sc.bind_sensors(net, len(y))
    assert sc._tick["args"].norm_rcp == 0
    ref = scorer(model, net, rows, grouped)
    for step, (seed, roll) in enumerate(((81, 0), (82, 1000), (81, 0), (82, 1000))):
        if step == 2:
            with torch.no_grad():
                net.conv1r.bias.add_(0.25)
            sc.refresh_sensors()
        q = queues(B, seed, y, roll)
        n0 = graphs()
        got = keep(sc.tick(*q))
        assert graphs() == n0 + (1 if step == 0 else 0)
        want = keep(ref.score_frames(net, *ieee_frames(*q, B)))
        same(got, want)
        assert torch.equal(sc.x[:B], ref.x[:B])


# ---- 3: a replay reads the buffers ----------------------------------------------
def test_replay_reads_the_buffers(model, graphs, pcm):
    B = 10
    net, y = make_net(B), pcm(B)
    sc = scorer(model, net, 16, True).bind_sensors(net, len(y))
    q1, q2 = queues(B, 81, y), queues(B, 82, y, roll=1000)
    n0 = graphs()
    a1 = keep(sc.tick(*q1))
    assert graphs() == n0 + 1
    a2 = keep(sc.tick(*q2))
    assert graphs() == n0 + 1
    assert not torch.equal(a1["base"], a2["base"])
    a3 = keep(sc.tick(*q1))
    assert graphs() == n0 + 1
    same(a3, a1)
    other = scorer(model, net, 16, True)
    same(a2, keep(other.score_sensors(net, *q2)))
    # new weights in the same buffer: no new capture
    with torch.no_grad():
        net.conv1r.bias.add_(0.25)
    n1 = graphs()
    stale = keep(sc.tick(*q2))
    same(stale, a2)                                      # the graph reads the packed copy
    sc.refresh_sensors()
    b2 = keep(sc.tick(*q2))
    assert graphs() == n1
    assert not torch.equal(b2["base"], a2["base"])
    same(b2, keep(other.score_sensors(net, *q2)))


# ---- 4: the routes take turns -----------------------------------------------------
def test_routes_take_turns(model, graphs, pcm):
    B = 10
    net, y = make_net(B), pcm(B)
    q = queues(B, 81, y)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).normal(size=(B, 1728)).astype(np.float32)).cuda()
    sc = scorer(model, net, 16, True).bind_sensors(net, len(y))
    s1 = keep(sc.score(x))
    tk = keep(sc.tick(*q))
    s2 = keep(sc.score(x))
    same(s1, s2)
    fresh = scorer(model, net, 16, True).bind_sensors(net, len(y))
    same(tk, keep(fresh.tick(*q)))


# ---- 5: refusals --------------------------------------------------------------------
def test_refusals_touch_nothing(model, graphs, pcm):
    B = 10
    net, y = make_net(B), pcm(B)
    force_q, hand_q, depth_q, mic_q = queues(B, 81, y)
    sc = scorer(model, net, 16, False)
    n0 = graphs()
    with pytest.raises(ValueError, match="bind_sensors"):
        sc.tick(force_q, hand_q, depth_q, mic_q)
    with pytest.raises(ValueError, match="bind_sensors"):
        sc.refresh_sensors()
    with pytest.raises(ValueError, match="> 16"):
        sc.bind_sensors(make_net(17), 18 * 4410)
    assert sc._tick is None
    sc.bind_sensors(net, len(y))
    out = sc.out.clone()
    with pytest.raises(ValueError, match="score_sensors"):
        sc.tick(force_q, hand_q, depth_q, mic_q[:-1])
    with pytest.raises(ValueError, match="score_sensors"):
        sc.tick(force_q, hand_q, depth_q, np.zeros(len(y) + 1, np.int16))
    with pytest.raises(ValueError, match="hand queue of 9 frames"):
        sc.tick(force_q, hand_q[:B - 1], depth_q, mic_q)
    with pytest.raises(ValueError, match="force queue of 9 frames"):
        sc.tick(force_q[:B - 1], hand_q, depth_q, mic_q)
    assert graphs() == n0 and torch.equal(out, sc.out)
    # the native entry refuses before its first launch too: a workspace one byte short
    a = sc._tick["args"]
    a.mfcc_ws_bytes -= 1
    with pytest.raises(_native.NativeError, match="mfcc: workspace"):
        sc.tick(force_q, hand_q, depth_q, mic_q)
    a.mfcc_ws_bytes += 1
    a.range_in[5] = 0.0                                   # the force range (0, 0)
    with pytest.raises(_native.NativeError, match="hsr_fuse_raw: range_in of t"):
        sc.tick(force_q, hand_q, depth_q, mic_q)
    a.range_in[5] = 400.0
    torch.cuda.synchronize()
    assert graphs() == n0 and torch.equal(out, sc.out)
    assert torch.isfinite(sc.tick(force_q, hand_q, depth_q, mic_q)["base"]).all() and graphs() == n0 + 1


# ---- 6: the same inputs, the same bits ------------------------------------------------
def test_two_scorers_same_bits(model, graphs, pcm):
    B = 17
    net, y = make_net(B), pcm(B)
    q = queues(B, 83, y)
    a = scorer(model, net, 64, False).bind_sensors(net, len(y), hand_dtype=np.float32)
    b = scorer(model, net, 64, False).bind_sensors(net, len(y))
    ra, rb = keep(a.tick(*q)), keep(b.tick(*q))
    same(ra, rb)                                          # fp32 and uint8 staging of the same frames
    assert torch.equal(a.x[:B], b.x[:B])
    same(keep(a.tick(*q)), ra)
