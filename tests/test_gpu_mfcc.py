"""Microphone front end on the GPU (mmad_mfcc, MfccFrontEnd, score_sensors).

Every case is compared with the float64 restatement stored in
tests/golden/mfcc_cases.npz (tests/golden/gen_mfcc_golden.py; the recipe is
tests/test_mfcc_abi.mfcc_ref); the bar is max abs error <= 2 x the case's
``err32``, the error of the same restatement run in float32 end to end (the
reference's own arithmetic).  The inputs come from test_mfcc_abi.signal."""
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from tests.test_mfcc_abi import CASES, case_pcm, norm_vec_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ends():
    """The two plans the cases need, built once."""
    from icra2021_multimodal_ad_amd.mfcc import MfccFrontEnd
    return {(44100, 4410): MfccFrontEnd(), (22050, 2205): MfccFrontEnd(sr=22050)}


@pytest.fixture(scope="module")
def pcm():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = case_pcm(name)
        return cache[name]
    return get


def _check(name, got, golden):
    g = golden("mfcc_cases")
    ref, err32 = g[name + "/mfcc"], float(g[name + "/err32"])
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max()
    print(f"mfcc {name}: max abs err {err:.3e}  (err32 {err32:.3e}, bar {2 * err32:.3e}, max|mfcc| {np.abs(ref).max():.1f})")
    assert err <= 2 * err32
    return ref, err32


# 1, 2, 5: the deployment shape, odd n_fft with a ragged tail, the 64-row scorer's 65 frames
@pytest.mark.parametrize("name", ["deploy", "odd", "rows64"])
def test_mfcc_against_float64(name, ends, pcm, golden):
    kind, sr, n_fft, _ = CASES[name]
    fe = ends[(sr, n_fft)]
    y = pcm(name)
    assert y.dtype == (np.int16 if kind == "i16" else np.float32)
    out = fe.mfcc(y)
    assert out.shape[0] == fe.frames(len(y)) == {"deploy": 11, "odd": 6, "rows64": 65}[name]
    _check(name, out, golden)


# 3: one frame, reflected at both ends; nothing outside out / norm_out is written
def test_single_frame_and_sentinels(ends, pcm, golden):
    fe = ends[(44100, 4410)]
    y = torch.from_numpy(pcm("one")).cuda()
    assert y.numel() == 2206 and fe.frames(y.numel()) == 1
    buf = torch.full((3, 13), -12345.0, device="cuda")
    nbuf = torch.full((3, 13), -54321.0, device="cuda")
    ws = torch.empty(int(_native.load().mmad_mfcc_ws_bytes(1, 128)), dtype=torch.uint8, device="cuda")
    _native.call("mmad_mfcc", _native.ptr(y), _native.PCM_I16, y.numel(), *fe.params, _native.ptr(fe.plan),
                 fe.plan.numel(), _native.ptr(buf[1]), 1, -1.0, 1.0, _native.ptr(nbuf[1]), _native.ptr(ws),
                 ws.numel(), _native.stream_ptr())
    torch.cuda.synchronize()
    assert (buf[0] == -12345.0).all() and (buf[2] == -12345.0).all()
    assert (nbuf[0] == -54321.0).all() and (nbuf[2] == -54321.0).all()
    ref, err32 = _check("one", buf[1:2], golden)
    nref = norm_vec_ref(ref)
    assert np.abs(nbuf[1].double().cpu().numpy() - nref[0]).max() <= 2 * err32 * 2 / (ref.max() - ref.min())


# 4: three frames of exact silence, then a loud tone: the silent frames sit on the -80 dB floor
def test_silent_frames_sit_on_the_floor(ends, pcm, golden):
    from tests.test_mfcc_abi import dct_basis, mel_db
    y = pcm("silence")
    assert (y[:3 * 4410] == 0).all() and np.abs(y[3 * 4410:]).max() >= 29999
    db, share = mel_db(y, 44100, 4410, 128)
    assert 0 < share < 1                                                # the clamp is exercised, not everything clamped
    out = ends[(44100, 4410)].mfcc(y)
    ref, err32 = _check("silence", out, golden)
    floor = (dct_basis(128, 13) @ np.full(128, -80.0))                  # a frame wholly on the floor
    got = out.double().cpu().numpy()
    assert np.abs(got[:3] - floor).max() <= 2 * err32
    assert (got[0] == got[1]).all() and (got[1] == got[2]).all()


# 6: norm_out over the last 10 of 11 frames
def test_norm_out_of_the_kept_frames(ends, pcm, golden):
    fe = ends[(44100, 4410)]
    raw, norm = fe.latest(pcm("deploy"), 10)
    g = golden("mfcc_cases")
    ref, err32 = g["deploy/mfcc"][1:], float(g["deploy/err32"])
    assert raw.shape == norm.shape == (10, 13)
    assert np.abs(raw.double().cpu().numpy() - ref).max() <= 2 * err32
    nref = norm_vec_ref(ref)
    err = np.abs(norm.double().cpu().numpy() - nref).max()
    bar = 2 * err32 * 2 / (ref.max() - ref.min())
    print(f"norm_out: max abs err {err:.3e}  (bar {bar:.3e})")
    assert err <= bar
    assert float(norm.min()) == -1.0 and float(norm.max()) == 1.0
    assert int(norm.argmax()) == int(nref.argmax()) and int(norm.argmin()) == int(nref.argmin())
    # another range, and the raw rows are the tail of mfcc()
    _, n01 = fe.latest(pcm("deploy"), 10, out_range=(0, 1))
    assert float(n01.min()) == 0.0 and float(n01.max()) == 1.0
    assert np.abs(n01.double().cpu().numpy() - norm_vec_ref(ref, 0.0, 1.0)).max() <= bar / 2
    assert torch.equal(raw, fe.mfcc(pcm("deploy"))[1:])


# 7: a call's bits repeat; int16 samples and their fp32 copies give the same bits
def test_bits_repeat(ends, pcm):
    fe = ends[(44100, 4410)]
    y = pcm("deploy")
    a_raw, a_norm = fe.latest(y, 10)
    b_raw, b_norm = fe.latest(torch.from_numpy(y).cuda(), 10)
    c_raw, c_norm = fe.latest(y.astype(np.float32), 10)
    d_raw, d_norm = fe.latest([y[:10000].tobytes(), y[10000:].tobytes()], 10)     # the reference's mic_q
    for raw, norm in ((b_raw, b_norm), (c_raw, c_norm), (d_raw, d_norm)):
        assert torch.equal(a_raw, raw) and torch.equal(a_norm, norm)
    big = pcm("rows64")
    assert torch.equal(fe.mfcc(big), fe.mfcc(big))


# 8: score_sensors on a fused-row model, B = 10
def test_score_sensors_is_score_frames_on_the_normalised_streams(pcm):
    from icra2021_multimodal_ad_amd import data_loaders
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.mfcc import MfccFrontEnd
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    B = 10
    cfg = types.SimpleNamespace(slicing_size=B, batch_size=B, gpu_id=0)
    torch.manual_seed(7)
    net = HSR_Net(False, cfg).cuda()
    torch.manual_seed(8)
    model = get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                            models="ae"))
    rng = np.random.Generator(np.random.PCG64(81))
    hand_q = rng.integers(0, 256, size=(B, 32 * 32 * 3)).astype(np.uint8)
    depth_q = rng.integers(0, 256, size=(B, 32 * 32)).astype(np.uint8)
    force_q = rng.uniform(0, 400, size=B)
    y = pcm("deploy")
    mic_q = [y[i:i + 4096].tobytes() for i in range(0, len(y), 4096)]
    sc = OnlineScorer(model, rows=16, groups=net.modality_columns())
    keep = lambda res: {k: v.clone() for k, v in res.items() if v is not None}   # noqa: E731
    a = keep(sc.score_sensors(net, force_q, hand_q, depth_q, mic_q))
    row = sc.x[:B].clone()
    # the same pass fed by hand: r, d, t normalised in torch, m from the front end
    f32 = lambda q: torch.from_numpy(np.asarray(q, dtype=np.float32)).cuda()   # noqa: E731
    r = 2 * (f32(hand_q).view(-1, 1, 3, 32, 32) - 0) / 255 + -1
    d = 2 * (f32(depth_q).view(-1, 1, 1, 32, 32) - 0) / 255 + -1
    t = 2 * (f32(force_q) - 0) / 400 + -1
    m = MfccFrontEnd().latest(mic_q, B)[1]
    b = keep(sc.score_frames(net, r, d, t, m))
    assert set(a) == set(b) and {"base", "sap", "layer_sq", "flags", "groups"} <= set(a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["base"]).all() and (a["groups"] > 0).all()
    assert torch.equal(row, sc.x[:B])
    # the drop-in loader returns the row score_sensors scored
    fused = data_loaders.get_realtime_dataloader(cfg, force_q, hand_q, depth_q, mic_q, hsr_net=net)
    assert fused.shape == (B, 1728) and torch.equal(fused, row)
    # and the reference-named MFCC stage the raw rows
    raw = data_loaders.save_mfcc_from_wav(mic_q, cfg, length=1.0)
    assert raw.shape == (B, 13) and raw.dtype == np.float32
    assert np.array_equal(raw, MfccFrontEnd().latest(mic_q, B)[0].cpu().numpy())
