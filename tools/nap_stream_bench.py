#!/usr/bin/env python
"""NAP scoring throughput at the C5 shape (D = 2048, fp32 model, 65,536-row
batches, the full layer range: 6442 concatenated diff columns), one process,
median of 3 passes, ms per 1,048,576 windows:

  (a) materialised  score(want_diffs) + NapScorer.score per batch (the route
                    without streamed NAP), over --parent-windows windows and
                    scaled to 1,048,576 (marked "scaled")
  (b) f32/f32       streamed NAP: fp32 scoring, fp32 NAP GEMM (one hipGraph)
  (c) x3/f32        split-bf16 scoring, fp32 NAP GEMM
  (d) x3/x3         split-bf16 scoring, split-bf16 NAP GEMM

and the NAP GEMM alone (mmad_nap_score on a packed 65,536-row operand, events
around the call, median of 5) in fp32 and in x3.  The fit is synthetic (random
V^T, unit weights): timing does not depend on its values.  Writes the JSON to
--out (default profiles/nap_stream_bench.json) and prints it on one line.

    python tools/nap_stream_bench.py [--windows N] [--batch B] [--dim D] [--timeout S]
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


def timed(fn, passes, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def gemm_alone(sc, precision, batch, iters=5):
    """mmad_nap_score alone on a packed [batch][Kp] operand of this precision."""
    import torch
    from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr, pad, F32, BF16X3
    W, R, Kp, Rp, vt, bias, w = sc._dev
    dev = vt.device
    Mp = pad(batch)
    s = stream_ptr()
    dt = BF16X3 if precision == "bf16x3" else F32
    src = torch.randn((batch, W), device=dev) * 0.1
    xp = torch.empty((Mp, Kp), device=dev)
    call("mmad_pack_input", dt, batch, W, Mp, Kp, ptr(src), W, ptr(xp), s)
    del src
    op = vt
    if dt == BF16X3:
        n = Rp * Kp
        op = torch.empty(2 * n, device=dev, dtype=torch.bfloat16)
        call("mmad_split_planes", n, ptr(vt), ptr(op), ptr(op[n:]), s)
    rowsq = torch.empty((Rp // 128, Mp), device=dev)
    out = torch.empty(batch, device=dev)

    def run():
        call("mmad_nap_score", dt, batch, W, R, Mp, Kp, Rp, ptr(xp), ptr(op), ptr(bias), ptr(w),
             ptr(rowsq), ptr(out), s)

    run()                                              # tile choice
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return {"shape": [batch, R, W], "ms": round(med, 3),
            "fp32_equiv_tflops": round(2.0 * batch * R * W / (med * 1e-3) / 1e12, 2)}


def child(args):
    import types
    import torch
    from icra2021_multimodal_ad_amd.data import synth_windows_device
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd import reconstruction_aggregation as ra
    dev = torch.device("cuda", 0)
    N, dim, batch = args.windows, args.dim, args.batch
    x = torch.empty((N, dim), device=dev)
    for s0 in range(0, N, 65536):
        n = min(65536, N - s0)
        x[s0:s0 + n] = synth_windows_device(n, dim, dev, seed=7 + s0)
    cfg = types.SimpleNamespace(input_size=dim, btl_size=100, n_layers=5, gpu_id=0, dtype="f32")
    torch.manual_seed(0)
    model = get_model(cfg)
    for i in range(20):                                # real BN statistics
        model.train_step_async(synth_windows_device(1024, dim, dev, seed=500 + i))
    model.eval()
    nat = model._native
    W = nat.diff_width()
    R = W
    g = torch.Generator(device=dev).manual_seed(1)
    fit = {"mu_r": torch.zeros(W, device=dev),
           "v": torch.randn((W, R), device=dev, generator=g) / W ** 0.5,
           "mu_s": torch.zeros(R, device=dev), "var": torch.ones(R, device=dev)}
    sc = ra.NapScorer.standalone(W, device=dev).fit(fit_state=fit)
    del fit
    layer_sq = torch.empty((nat.n_enc + 1, N), device=dev)
    nap = torch.empty(N, device=dev)
    out = {"tool": "nap_stream_bench", "dim": dim, "windows": N, "batch": batch, "nap_columns": W,
           "nap_rank": R, "fit": "synthetic", "passes": args.passes,
           "device": torch.cuda.get_device_name(0), "modes": {}}

    def scale(ms, n):
        return round(statistics.median(ms) * (1 << 20) / n, 3)

    # (a) the materialised route
    Na = min(args.parent_windows, N)

    def parent():
        for s0 in range(0, Na, batch):
            _, d = nat.score(x[s0:s0 + batch], want_diffs=True)
            nap[s0:s0 + batch] = sc.score(d)

    ms = timed(parent, args.passes, 1)
    out["modes"]["a_materialised"] = {"windows": Na, "scaled": Na != (1 << 20),
                                      "ms_per_pass": [round(v, 3) for v in ms],
                                      "ms_per_1M_windows": scale(ms, Na)}
    ref_nap = nap[:Na].clone()

    def streamed():
        ra.score_windows(x, model, batch, out=layer_sq, graph=True, nap=sc, nap_out=nap)

    for key, score_prec, nap_prec in (("b_stream_f32_f32", None, "f32"), ("c_stream_x3_f32", "bf16x3", "f32"),
                                      ("d_stream_x3_x3", "bf16x3", "bf16x3")):
        nat.set_score_precision(score_prec)
        sc.attach(model, precision=nap_prec, layers=(0, nat.n_enc + 1))
        ms = timed(streamed, args.passes, 2)           # tile tuning + capture, first replay
        nat.check_status()
        row = {"ms_per_pass": [round(v, 3) for v in ms], "ms_per_1M_windows": scale(ms, N),
               "nap_mean": float(nap.mean())}
        if key == "b_stream_f32_f32":
            row["bit_equal_to_materialised"] = bool(torch.equal(nap[:Na], ref_nap))
        else:
            row["max_rel_dev_from_materialised"] = float(((nap[:Na] - ref_nap).abs() / ref_nap.abs().max()).max())
        out["modes"][key] = row
        sc.detach()
    nat.set_score_precision(None)
    del layer_sq, x
    torch.cuda.empty_cache()
    out["nap_gemm_alone"] = {"f32": gemm_alone(sc, "f32", batch), "bf16x3": gemm_alone(sc, "bf16x3", batch)}
    m = out["modes"]
    out["b_over_a_time"] = round(m["b_stream_f32_f32"]["ms_per_1M_windows"] / m["a_materialised"]["ms_per_1M_windows"], 4)
    out["d_over_b_time"] = round(m["d_stream_x3_x3"]["ms_per_1M_windows"] / m["b_stream_f32_f32"]["ms_per_1M_windows"], 4)
    out["nap_gemm_f32_over_x3"] = round(out["nap_gemm_alone"]["f32"]["ms"] / out["nap_gemm_alone"]["bf16x3"]["ms"], 3)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=1 << 20)
    ap.add_argument("--parent-windows", type=int, default=1 << 18)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nap_stream_bench.json"))
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the measuring child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows),
           "--parent-windows", str(args.parent_windows), "--batch", str(args.batch), "--dim", str(args.dim),
           "--passes", str(args.passes), "--out", args.out]
    try:
        r = subprocess.run(cmd, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(json.dumps({"tool": "nap_stream_bench", "error": f"timed out after {args.timeout} s"}))
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
