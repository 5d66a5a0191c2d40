#!/usr/bin/env python
"""Scoring throughput of the three precisions at the C5 shape (D = 2048,
1,048,576 windows resident in HBM, 65,536-row batches, one hipGraph replay per
pass): an fp32 model on the exact path (`f32`), the same fp32 model scoring on
split-bf16 planes (`f32 + bf16x3`, config.score_dtype = "bf16x3") and a bf16
model (`bf16`).  Prints one JSON line: ms per 1 M windows (median of 3 passes)
for each mode, the x3 / f32 ratio, and the per-launch time of the last decoder
layer's forward GEMM (65,536 x 2048 x ~2048) from the executor's kernel probe
(kind 2: events attached to the launch itself) in fp32-equivalent TFLOP/s.

The measurement runs in a child process under a time limit; the three modes
share that one process so they see the same device state.

    python tools/score_x3_bench.py [--windows N] [--batch B] [--dim D] [--timeout S]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def measure_mode(name, dtype, score_dtype, x, batch, passes, probe_iters):
    import ctypes
    import types
    import torch
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.data import synth_windows_device
    from icra2021_multimodal_ad_amd import reconstruction_aggregation as ra
    N, dim = x.shape
    dev = x.device
    cfg = types.SimpleNamespace(input_size=dim, btl_size=100, n_layers=5, gpu_id=0, dtype=dtype)
    if score_dtype:
        cfg.score_dtype = score_dtype
    torch.manual_seed(0)
    model = get_model(cfg)
    for i in range(20):                                # real BN statistics
        model.train_step_async(synth_windows_device(1024, dim, dev, seed=500 + i))
    model.eval()
    nat = model._native
    nat.sync_shadow(force=True)
    widths = nat.diff_widths()
    layer_sq = torch.empty((nat.n_enc + 1, N), device=dev)

    def one_pass():
        ra.score_windows(x, model, batch, out=layer_sq, graph=True)
        return ra.base_from_layer_sq(layer_sq, widths), ra.sap_from_layer_sq(layer_sq, widths)

    for _ in range(2):                                 # tile tuning, capture, first replay
        base, sap = one_pass()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        t0 = time.perf_counter()
        base, sap = one_pass()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    nat.check_status()
    # the last decoder layer's forward GEMM inside the eval forward
    last = nat.n_enc + nat.n_dec - 1
    L = nat.layers[last]
    lib = nat._lib
    xb = x[:batch]
    nat.forward(xb, want_xhat=False)
    assert lib.mmad_ae_probe(nat._h, 2, last, probe_iters) == 0
    for _ in range(probe_iters):
        nat.forward(xb, want_xhat=False)
    buf = (ctypes.c_float * probe_iters)()
    n = lib.mmad_ae_probe_read(nat._h, buf, probe_iters)
    lib.mmad_ae_probe(nat._h, 2, -1, 0)
    gemm_ms = statistics.median(buf[:n]) if n > 0 else float("nan")
    fl = 2.0 * xb.shape[0] * L["K"] * L["N"]
    res = {"mode": name, "score_dtype": int(nat.score_dtype),
           "ms_per_pass": [round(v, 3) for v in ms],
           "ms_per_1M_windows": round(statistics.median(ms) * (1 << 20) / N, 3),
           "gemm_shape": [int(xb.shape[0]), L["N"], L["K"]], "gemm_us": round(gemm_ms * 1e3, 2),
           "gemm_fp32_equiv_tflops": round(fl / (gemm_ms * 1e-3) / 1e12, 2),
           "checksum": {"base_mean": float(base.mean()), "sap_mean": float(sap.mean())}}
    del model, nat, layer_sq
    torch.cuda.empty_cache()
    return res


def child(args):
    import torch
    from icra2021_multimodal_ad_amd.data import synth_windows_device
    dev = torch.device("cuda", 0)
    N, dim = args.windows, args.dim
    x = torch.empty((N, dim), device=dev)
    for s0 in range(0, N, 65536):
        n = min(65536, N - s0)
        x[s0:s0 + n] = synth_windows_device(n, dim, dev, seed=7 + s0)
    modes = [("f32", "f32", None), ("f32+bf16x3", "f32", "bf16x3"), ("bf16", "bf16", None)]
    out = {"tool": "score_x3_bench", "dim": dim, "windows": N, "batch": args.batch,
           "passes": args.passes, "device": torch.cuda.get_device_name(0), "modes": {}}
    for name, dtype, sdt in modes:
        out["modes"][name] = measure_mode(name, dtype, sdt, x, args.batch, args.passes, args.probe_iters)
    m = out["modes"]
    out["x3_over_f32_time"] = round(m["f32+bf16x3"]["ms_per_1M_windows"] / m["f32"]["ms_per_1M_windows"], 4)
    out["f32_over_x3_speedup"] = round(m["f32"]["ms_per_1M_windows"] / m["f32+bf16x3"]["ms_per_1M_windows"], 3)
    out["x3_over_bf16_time"] = round(m["f32+bf16x3"]["ms_per_1M_windows"] / m["bf16"]["ms_per_1M_windows"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--probe-iters", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the measuring child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows),
           "--batch", str(args.batch), "--dim", str(args.dim), "--passes", str(args.passes),
           "--probe-iters", str(args.probe_iters)]
    try:
        r = subprocess.run(cmd, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(json.dumps({"tool": "score_x3_bench", "error": f"timed out after {args.timeout} s"}))
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
