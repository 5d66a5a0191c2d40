"""NAP fit at the c5 model (D=2048, W=6442): the materialised fit (mmad_nap_fit
on the concatenated train diffs) against the streamed fit
(mmad_ae_nap_fit_stream), alternated on one box.

Per alternation: the parent's route (materialise the diffs, mmad_nap_fit; its
nap_gram_k time from the profiler's kernel records), then the streamed route
end to end, then the streamed phases one by one through the operand-level
entry points on the same rows (sums, centre + Gram, solve, rotated moments) and
one plain scoring pass (the streamed fit runs three).  Gram TFLOP/s counts the
upper triangle's N W (W + 1) flop.  --big adds one streamed fit over 1,048,576
windows and records its peak device memory.

    python tools/nap_fit_bench.py [--windows 65536] [--batch 8192] [--reps 3] [--big]
        [--out profiles/nap_fit_stream_bench.json]"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--big-windows", type=int, default=1048576)
    ap.add_argument("--out", default="profiles/nap_fit_stream_bench.json")
    a = ap.parse_args()
    import torch
    from icra2021_multimodal_ad_amd import _native
    from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr
    from icra2021_multimodal_ad_amd.data import synth_windows_device
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.novelty_detection import _device_diffs
    from icra2021_multimodal_ad_amd.reconstruction_aggregation import nap_fit, score_windows
    dev = torch.device("cuda", 0)
    cfg = types.SimpleNamespace(input_size=a.dim, btl_size=100, n_layers=5, gpu_id=0, dtype="f32")
    torch.manual_seed(0)
    model = get_model(cfg)
    for i in range(20):                                   # real BN statistics
        model.train_step_async(synth_windows_device(1024, a.dim, dev, seed=500 + i))
    model.eval()
    nat = model._native
    W = nat.diff_width()
    N, B = a.windows, a.batch

    def windows(n):
        x = torch.empty((n, a.dim), device=dev)
        for s0 in range(0, n, 65536):
            m = min(65536, n - s0)
            x[s0:s0 + m] = synth_windows_device(m, a.dim, dev, seed=7 + s0)
        return x

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    x = windows(N)
    score_windows(x[:B], model, B, graph=False)           # warm / tile choices
    lib = _native.load()
    sb = int(lib.mmad_nap_fit_state_bytes(W))
    rows = []
    for rep in range(a.reps):
        row = {}
        # ---- the parent's route
        diffs, row["parent_materialise_s"] = timed(lambda: _device_diffs(model, x, B))
        row["materialised_diffs_bytes"] = diffs.numel() * 4
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                ref, row["parent_nap_fit_s"] = timed(lambda: nap_fit(diffs))
            gram = [e for e in prof.events() if "nap_gram_k" in e.name]
            row["parent_nap_gram_k_s"] = sum(e.device_time_total for e in gram) / 1e6 if gram else None
            rot = [e for e in prof.events() if "nap_rotstats_k" in e.name]
            row["parent_nap_rotstats_k_s"] = sum(e.device_time_total for e in rot) / 1e6 if rot else None
        except Exception as exc:                           # no kernel records on this box
            row["profiler_error"] = repr(exc)
            ref, row["parent_nap_fit_s"] = timed(lambda: nap_fit(diffs))
        # ---- the streamed route, end to end
        (got, _), row["stream_fit_total_s"] = timed(lambda: nat.nap_fit_stream(x, B))
        _, row["one_score_pass_s"] = timed(lambda: score_windows(x, model, B, graph=False))
        row["mu_r_max_abs_diff"] = float((got["mu_r"] - ref["mu_r"]).abs().max())
        row["var_max_rel_diff"] = float(((got["var"] - ref["var"]).abs().max() / ref["var"].max()))
        del got
        # ---- its phases on the same rows, through the operand-level entry points
        state = torch.empty(sb + 256, dtype=torch.uint8, device=dev)
        sp = ctypes.c_void_p((state.data_ptr() + 255) // 256 * 256)
        s = stream_ptr()
        mu_r, v = torch.empty(W, device=dev), torch.empty((W, min(N, W)), device=dev)
        mu_s, var = torch.empty(min(N, W), device=dev), torch.empty(min(N, W), device=dev)
        cuts = list(range(0, N, B))
        call("mmad_nap_fit_begin", W, sp, sb, s)

        def sums():
            for c in cuts:
                d = diffs[c:c + B]
                call("mmad_nap_fit_accumulate_sums", W, d.shape[0], ptr(d), W, sp, sb, s)
            call("mmad_nap_fit_finish_mean", W, N, sp, sb, ptr(mu_r), s)

        def gram():
            for c in cuts:                                 # in place: the copy is pass 3's input
                d = work[c:c + B]
                call("mmad_nap_fit_accumulate_gram", W, d.shape[0], ptr(d), W, ptr(mu_r), sp, sb, s)

        def rot():
            for c in cuts:
                d = diffs[c:c + B]
                call("mmad_nap_fit_accumulate_rot", W, N, d.shape[0], ptr(d), W, ptr(mu_r), sp, sb, s)
            call("mmad_nap_fit_finish", W, N, sp, sb, ptr(mu_s), ptr(var), s)

        _, row["stream_sums_s"] = timed(sums)
        work = diffs.clone()
        _, row["stream_centre_gram_s"] = timed(gram)
        del work
        _, row["stream_solve_s"] = timed(lambda: call("mmad_nap_fit_solve", W, N, sp, sb, ptr(v), s))
        _, row["stream_rot_s"] = timed(rot)
        row["stream_gram_fp64_tflops"] = N * W * (W + 1) / row["stream_centre_gram_s"] / 1e12
        del diffs, ref, state
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"model": f"D={a.dim} btl=100 n_layers=5 fp32", "W": W, "windows": N, "batch": B,
           "fit_state_bytes": sb, "alternations": rows}
    if a.big:
        del x
        torch.cuda.empty_cache()
        xb = windows(a.big_windows)
        torch.cuda.reset_peak_memory_stats()
        _, t = timed(lambda: nat.nap_fit_stream(xb, 65536))
        out["big"] = {"windows": a.big_windows, "batch": 65536, "stream_fit_total_s": t,
                      "peak_device_bytes": int(torch.cuda.max_memory_allocated()),
                      "input_windows_bytes": xb.numel() * 4,
                      "materialised_diffs_would_be_bytes": a.big_windows * W * 4}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "alternations"}))


if __name__ == "__main__":
    main()
