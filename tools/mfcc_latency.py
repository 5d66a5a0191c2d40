"""What the microphone front end costs -> profiles/mfcc_latency.json.

  (1) GPU time of mmad_mfcc (three launches, by events) and host wall including
      one stream synchronise, for 10, 16 and 64 kept windows at n_fft 4410: an
      int16 buffer of keep + 1 frames already on the device (the deployment's
      shape: the kept windows plus the dropped first frame), norm_out on.
  (2) OnlineScorer.score_sensors against score_frames at 10 windows on a
      1728-wide fp32 model, alternated in one process; their difference is
      the front end's cost inside a tick (score_sensors also normalises the
      camera, depth and force/torque queues in torch and uploads the PCM;
      score_frames is handed device tensors that are already normalised).
  (3) beside each, the host time of the recipe's float32 numpy / scipy
      restatement (tests/test_mfcc_abi.mfcc_ref with scipy.fft, on the
      threads the process is given): the stand-in for the reference's CPU
      stage (librosa is not installed).

After 50 warm-up calls, median and 10th / 90th percentile of 300 calls.

  python tools/mfcc_latency.py [--out profiles/mfcc_latency.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icra2021_multimodal_ad_amd import _native  # noqa: E402
from icra2021_multimodal_ad_amd._native import ptr, stream_ptr  # noqa: E402

WARMUP, CALLS = 50, 300
N_FFT = 4410


def stats(v):
    p = np.percentile(np.asarray(v), [50, 10, 90])
    return {"median_us": float(p[0]), "p10_us": float(p[1]), "p90_us": float(p[2])}


def measure(fns):
    """fns: {name: callable enqueueing one call on the current stream}, alternated."""
    st = torch.cuda.current_stream()
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in fns}
    gpu, wall = {k: [] for k in fns}, {k: [] for k in fns}
    for it in range(WARMUP + CALLS):
        for k, fn in fns.items():
            a, b = ev[k]
            t0 = time.perf_counter()
            a.record(st)
            fn()
            b.record(st)
            st.synchronize()
            t1 = time.perf_counter()
            if it >= WARMUP:
                gpu[k].append(a.elapsed_time(b) * 1e3)
                wall[k].append((t1 - t0) * 1e6)
    return {k: {"gpu": stats(gpu[k]), "wall": stats(wall[k])} for k in fns}


def host_time(fn, calls=20):
    fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return stats(t)


def restatement():
    """The float32 CPU recipe: (callable y -> mfcc, what it ran on)."""
    from tests.test_mfcc_abi import mfcc_ref
    try:
        import scipy.fft
        rfft, dct, name = scipy.fft.rfft, (lambda db: scipy.fft.dct(db, axis=0, type=2, norm="ortho")), "scipy.fft"
    except ImportError:
        rfft, dct, name = np.fft.rfft, None, "numpy.fft"
    return (lambda y: mfcc_ref(y, 44100, N_FFT, dtype=np.float32, rfft=rfft, dct=dct)), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mfcc_latency.json")
    a = ap.parse_args()
    _native.require_gpu()
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.mfcc import MfccFrontEnd
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    from tests.test_mfcc_abi import TONES, signal
    lib = _native.load()
    fe = MfccFrontEnd()
    cpu, cpu_name = restatement()
    y_all = signal(65 * N_FFT, TONES, 300, 9)
    doc = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "n_fft": N_FFT,
           "cpu_restatement": cpu_name, "cpu_threads": os.environ.get("OMP_NUM_THREADS"), "mmad_mfcc": {}}

    for keep in (10, 16, 64):
        y = y_all[:(keep + 1) * N_FFT - N_FFT // 2]          # keep + 1 frames
        F = fe.frames(len(y))
        assert F == keep + 1, (F, keep)
        yd = torch.from_numpy(y).cuda()
        out = torch.empty((F, 13), device="cuda")
        norm = torch.empty((keep, 13), device="cuda")
        ws = torch.empty(int(lib.mmad_mfcc_ws_bytes(F, 128)), dtype=torch.uint8, device="cuda")
        args = (ptr(yd), _native.PCM_I16, yd.numel(), *fe.params, ptr(fe.plan), fe.plan.numel(), ptr(out), keep,
                -1.0, 1.0, ptr(norm), ptr(ws), ws.numel(), stream_ptr())
        res = measure({"mmad_mfcc": lambda: _native.check(lib.mmad_mfcc(*args), "mmad_mfcc")})["mmad_mfcc"]
        ref = cpu(y)
        res["max_abs_diff_vs_cpu_f32"] = float(np.abs(out.cpu().numpy() - ref).max())
        res["cpu_f32_restatement"] = host_time(lambda: cpu(y))
        res["frames"] = F
        doc["mmad_mfcc"][f"keep{keep}"] = res
        print(f"keep {keep}: gpu {res['gpu']['median_us']:.1f} us, wall {res['wall']['median_us']:.1f} us, "
              f"cpu f32 {res['cpu_f32_restatement']['median_us']:.0f} us", flush=True)

    # (2) a tick from the raw queues against a tick from normalised device tensors
    B = 10
    cfg = types.SimpleNamespace(slicing_size=B, batch_size=B, gpu_id=0)
    torch.manual_seed(7)
    net = HSR_Net(False, cfg).cuda()
    torch.manual_seed(8)
    model = get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                            models="ae"))
    sc = OnlineScorer(model, rows=16)
    rng = np.random.Generator(np.random.PCG64(81))
    hand_q = rng.integers(0, 256, size=(B, 3072)).astype(np.float32)
    depth_q = rng.integers(0, 256, size=(B, 1024)).astype(np.float32)
    force_q = rng.uniform(0, 400, size=B).astype(np.float32)
    y = y_all[:11 * N_FFT - N_FFT // 2]
    from icra2021_multimodal_ad_amd.data_loaders import normalised_sensors
    r, d, t = normalised_sensors(force_q, hand_q, depth_q, "cuda")
    m = fe.latest(y, B)[1]
    yd = torch.from_numpy(y).cuda()
    res = measure({"score_frames": lambda: sc.score_frames(net, r, d, t, m),
                   "score_sensors_host_queues": lambda: sc.score_sensors(net, force_q, hand_q, depth_q, y),
                   "score_frames_plus_latest_device_pcm":
                       lambda: sc.score_frames(net, r, d, t, fe.latest(yd, B)[1])})
    for k in ("score_sensors_host_queues", "score_frames_plus_latest_device_pcm"):
        res[k + "_minus_score_frames"] = {w: res[k][w]["median_us"] - res["score_frames"][w]["median_us"]
                                          for w in ("gpu", "wall")}
    res["cpu_f32_restatement"] = host_time(lambda: cpu(y))
    doc["tick_B10"] = res
    print({k: (round(v["gpu"]["median_us"], 1), round(v["wall"]["median_us"], 1)) for k, v in res.items()
           if isinstance(v, dict) and "gpu" in v and isinstance(v["gpu"], dict)}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
