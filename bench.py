"""Benchmark: sensor-windows/sec of the AE train step (fwd + sum-MSE + bwd +
Adam) on synthetic 4-modal windows, 1..8 MI355X (BASELINE.json metric).

Workloads (``--config``; ``auto`` = c3 on one GPU -- the largest single-GPU
configuration, C4's per-GPU shard -- with c2 measured after it in the same line
as the ``c2`` sub-object and c3 on the exact-fp32 parity path as ``c3_f32``; c4
on several):
  c2  BASELINE configs[1]: FC-AE, D=2048, 1024 windows, bf16, 1 GPU
  c3  BASELINE configs[2]: VIB-AE (k=1, beta_kl=1), D=2048, 4096 windows, bf16
  c4  BASELINE configs[3]: the c3 model, 4096 windows PER GPU (global 4096*N),
      one process per GPU, RCCL reduce-scatter / sharded Adam / all-gather of the
      weight gradients in buckets of consecutive layers over xGMI, overlapped with
      the backward (weak scaling)
  c5  BASELINE configs[4]: RaPP scoring (get_diffs + BASE + SAP) over 1,048,576
      windows resident in HBM, D=2048, one hipGraph-captured pass per step
      (bench_score.run_c5; metric: scored windows/s)
``--model/--dim/--batch`` override the chosen config's fields.

A plain run (``bench.py --gpus 1 --steps K --warmup W``) sets up, warms up,
times the K steps of the headline workload and prints the result line:
``metric`` / ``value`` / ``unit`` / ``higher_is_better`` / ``dtype`` /
``ms_per_step`` (milliseconds per timed step) and the workload description.
``--full`` adds everything else described below (per-step spread, kernel probes
and rooflines, the CPU baseline, the c2 / c3_f32 sub-objects, the N>1
same-workload run); each of those takes runs of its own after the timed region.

``--dump-outputs DIR`` (one GPU) writes what the last timed step handed back as
``DIR/<name>.npy`` (float32): the step's loss, the BatchNorm running statistics
and a fixed seeded sample (DUMP_SAMPLE elements, the same indices for all three)
of the fp32 master parameters and the two Adam moments; c5 writes the BASE and
SAP score of every window.  The timed steps always start from the model state
the W warm-up steps left (the time-sized soak's updates are rolled back before
the timed region), on the same seeded batches, so two runs with the same
arguments feed every timed step the same inputs.

``python bench.py --gpus N`` without torchrun env vars spawns the N ranks itself
(torch.multiprocessing, before any GPU call); under torchrun it reads
RANK/WORLD_SIZE/LOCAL_RANK.  W untimed steps, then K timed steps between
barrier + synchronize pairs, the max over ranks; rank 0 prints ONE JSON line.
With ``--full`` the line also holds:

* the timed steps are eager executor steps (mmad_ae_train_step: one host
  call enqueues the whole step on the main + side streams, no host sync);
  ``train_step`` says which schedule ran.  ``step_spread`` = per-step GPU
  times from HIP events between consecutive steps of a separate run of the
  same length right after the timed region (median / p10 / p90 / max).
* ``roofline``: the kernel that dominates the step -- the dW GEMM with the
  fused Adam epilogue of the largest layer, HBM-bound (26 B of Adam state per
  parameter + its two bf16 operands).  Its duration comes from the executor's
  probe inside the timed steps (mmad_ae_probe kind 3: start / stop events
  attached to that one launch by hipExtLaunchKernel, no marker packet, no
  wait for the side stream -- the launch as it runs beside the side stream's
  work, what rocprofv3's kernel records of the same command show);
  ``avg_us_isolated`` = the same launch alone, in eager steps right after the
  timed region (kind 1);  ``traffic`` =
  PMC HBM bytes per launch from the newest matching profiles/*_pmc_dw.json.
* ``roofline_encoder_gemm``: the encoder's first forward GEMM (the north-star
  MFMA target), launched back to back between one event pair.
* ``cpu_baseline`` (rank 0, N=1): the torch-CPU fp32 restatement of the
  reference's modules (oracle/torch_ref.py) timed on this host's cores on a
  bounded sample of the same workload.
* N>1: ``n1_same_workload`` = the same ranks' windows/s per GPU with the
  exchange switched off (same process, after the timed region), so scaling
  can be read against the same workload.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

BF16_PEAK_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
F32_PEAK_TFLOPS = 157.3     # f32 MFMA = vector rate
HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md)

CONFIGS = {
    "c2": dict(model="ae", dim=2048, batch=1024, name="BASELINE configs[1]"),
    "c3": dict(model="vib_ae", dim=2048, batch=4096, name="BASELINE configs[2]"),
    "c4": dict(model="vib_ae", dim=2048, batch=4096, name="BASELINE configs[3]"),
    "c5": dict(model="ae", dim=2048, batch=65536, name="BASELINE configs[4]"),
}


def ae_flops_per_window(widths_enc, widths_dec):
    macs = sum(a * b for a, b in zip(widths_enc[:-1], widths_enc[1:]))
    macs += sum(a * b for a, b in zip(widths_dec[:-1], widths_dec[1:]))
    return 6.0 * macs, macs   # fwd 2*MAC + bwd-data 2*MAC + bwd-weight 2*MAC


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cores():
    """The host cores this process may actually use: the CPU affinity mask,
    capped by the cgroup CPU quota (cgroup v2 cpu.max / v1 cfs quota).  On the
    GPU box the affinity mask lists the whole machine (256 CPUs) while the
    lease's quota is 16; torch with 256 threads on a 16-CPU quota runs ~300x
    slower than with 16."""
    n = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    used = n if quota is None else max(1, min(n, int(quota)))
    return used, n, quota


def cpu_baseline(d, batch, vib, budget_s=12.0):
    """The reference's modules in torch-CPU fp32 (oracle/torch_ref.py): whole
    train steps (fwd + loss + bwd + Adam) at the same D and batch, timed on
    this host's cores for a bounded sample."""
    import torch
    from oracle import torch_ref
    from icra2021_multimodal_ad_amd.common_utils import init_state_dict, ae_widths
    from icra2021_multimodal_ad_amd.data import synth_windows
    # every host core this process may run on (affinity capped by the cgroup quota)
    threads, n_aff, quota = host_cores()
    torch.set_num_threads(threads)
    enc_out = 200 if vib else None
    enc, dec = ae_widths(d, 100, 5, enc_out=enc_out)
    sd = init_state_dict(d, 100, 5, seed=0, enc_out=enc_out)
    m = torch_ref.build(sd, enc, dec, vib=vib)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x = torch.from_numpy(synth_windows(batch, d, seed=1))
    torch_ref.train_step(m, opt, x)            # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        torch_ref.train_step(m, opt, x)
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s or n >= 200:
            break
    return {"value": round(n * batch / el, 1), "unit": "sensor-windows/sec", "cores": threads,
            "kind": "port", "cpu": cpu_model(),
            "sample": f"{n} train steps of the reference's modules in torch-CPU fp32 "
                      f"(nn.Linear/LeakyReLU/BatchNorm1d, MSELoss(sum), optim.Adam; "
                      f"oracle/torch_ref.py{', VIB-AE' if vib else ''}) at D={d}, batch={batch}, "
                      f"{el:.1f} s, torch threads={threads} (affinity {n_aff} CPUs, cgroup quota "
                      f"{quota if quota is not None else 'none'})"}


def dw_adam_bytes(N, K, B, es=2):
    """Algorithmic HBM bytes of one dW GEMM with the fused Adam epilogue:
    fp32 p/m/v read + written (24 B/param) + the bf16 weight shadow written
    (2 B/param, bf16 models only) + the two operands dz [B x N] and a [B x K]
    read once (es bytes per element)."""
    return (26 if es == 2 else 24) * N * K + es * B * (N + K)


def pick_dominant_layer(nat, batch):
    """Largest parameter count among the layers (every dW GEMM carries the
    fused Adam epilogue; ties: the first, encoder layer 1, on the main stream
    at the end of the chain)."""
    return max(range(len(nat.layers)), key=lambda l: (nat.layers[l]["N"] * nat.layers[l]["K"], -l))


CSRC = os.path.join(REPO, "icra2021_multimodal_ad_amd", "csrc")


def src_sha16(kind):
    """Hash of the kernel sources a PMC summary of `kind` measured: the GEMM
    template (+ the executor's dW tile rule for `dw`).  A summary whose hash
    differs from this tree's was taken on other code: bench reports it as
    `traffic_prior_profile`, not as `traffic`."""
    import glob
    import hashlib
    files = sorted(glob.glob(os.path.join(CSRC, "mmad_gemm*")) + [os.path.join(CSRC, "mmad_common.h")])
    if kind == "dw":
        files.append(os.path.join(CSRC, "mmad_ae.hip"))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _pmc_file(kind, workload):
    """Newest profiles/*_pmc_<kind>.json for this workload: (summary, path,
    matches-this-build)."""
    import glob
    cur = src_sha16(kind)
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", f"*_pmc_{kind}.json")))[::-1]:
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        if d.get("workload") == workload:
            return d, os.path.relpath(f, REPO), d.get("src_sha16") == cur
    return None, None, False


def pmc_fields(kind, workload):
    """roofline `traffic` (+ provenance) from the matching PMC summary; a
    summary taken on other kernel sources is reported as prior, never as
    this build's traffic."""
    pmc, src, current = _pmc_file(kind, workload)
    out = {"traffic": None}
    if pmc is None:
        return out, None
    if current:
        out["traffic"] = pmc.get("traffic_bytes_per_launch")
    else:
        out["traffic_prior_profile"] = pmc.get("traffic_bytes_per_launch")
    out["traffic_source"] = src
    out["traffic_source_matches_build"] = current
    return out, (pmc if current else None)


def gemm_roofline(model, batch, iters=50):
    """Average duration of the encoder's first-layer forward GEMM from HIP
    events on the launch stream (back-to-back launches between one pair)."""
    import torch
    from icra2021_multimodal_ad_amd import _native
    from icra2021_multimodal_ad_amd._native import call, ptr, stream_ptr
    nat = model._native
    L = nat.layers[0]
    Mp = _native.pad(batch)
    dt = nat.dt
    tdt = torch.bfloat16 if dt == _native.BF16 else torch.float32
    dev = nat.device
    xin = torch.randn((Mp, L["Kp"]), device=dev).to(tdt)
    out = torch.empty((Mp, L["Np"]), device=dev, dtype=tdt)
    stats = torch.empty((Mp // 32, 2, L["Np"]), device=dev)
    w = nat.shadow[L["w_off"]:] if nat.shadow is not None else nat.params[L["w_off"]:]
    b = nat.params[L["b_off"]:]
    s = stream_ptr()

    def launch():
        call("mmad_fc_fwd", dt, batch, L["N"], L["K"], Mp, L["Np"], L["Kp"], ptr(xin), ptr(w), ptr(b),
             1, 0.2, None, None, ptr(out), ptr(stats), s)
    import statistics
    for _ in range(5):
        launch()
    # 5 groups of iters/5 back-to-back launches, each between its own event
    # pair; the median group (one slow group -- a clock dip -- does not move it)
    groups, per = 5, max(iters // 5, 1)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(groups)]
    for e0, e1 in ev:
        e0.record()
        for _ in range(per):
            launch()
        e1.record()
    torch.cuda.synchronize()
    avg_s = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) / 1e3 / per
    iters = groups * per
    flops = 2.0 * batch * L["K"] * L["N"]
    peak = BF16_PEAK_TFLOPS if dt == _native.BF16 else F32_PEAK_TFLOPS
    ach = flops / avg_s / 1e12
    wl = {"dim": L["K"], "batch": batch, "dtype": nat.dtype_name}
    tf, pmc = pmc_fields("traffic", wl)
    res = {"kernel": f"mmad_gemm fwd (encoder layer 1: {batch}x{L['K']} . {L['N']}x{L['K']}^T,"
                     f" bias+LeakyReLU+BN-stat epilogue)",
           "bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
           "frac": round(ach / peak, 4), **tf,
           "avg_us": round(avg_s * 1e6, 2), "flops_per_launch": flops,
           "timing": f"{iters} launches: the median of 5 groups of back-to-back launches, each "
                     f"group between one HIP event pair"}
    if pmc is not None and pmc.get("SQ_VALU_MFMA_BUSY_CYCLES"):
        # rocprofv3 counters of the same kernel and shape (tools/pmc_gemm.py)
        res["mfma_counters"] = {k: pmc.get(k) for k in (
            "SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE", "mfma_busy_over_issued",
            "mfma_busy_frac_grbm", "mfma_busy_frac_at_2p4ghz", "effective_clock_ghz_grbm",
            "kernel_trace_median_us", "l2_hit_rate")}
    return res


def dw_roofline(nat, layer, durations_ms, batch, steps_timed, fused_adam=True, layers=None,
                in_timed=False, isolated_ms=None):
    """roofline of the dominant dW GEMM launch from the in-situ probe durations.
    layers: the layers that launch covered (mmad_ae_probe_layers).  in_timed:
    the durations are the timed steps' own launches (kernel-attached events);
    isolated_ms: the same launch timed alone after the timed region."""
    import statistics
    layers = sorted(layers or [layer], reverse=True)
    rows = batch                      # k = 1: decoder rows = encoder rows
    es = 2 if nat.dtype_name == "bf16" else 4
    nbytes, flops = 0, 0.0
    for l in layers:
        L = nat.layers[l]
        if fused_adam:
            nbytes += dw_adam_bytes(L["N"], L["K"], rows, es)
        else:
            nbytes += 4 * L["N"] * L["K"] + es * rows * (L["N"] + L["K"])
        flops += 2.0 * rows * L["N"] * L["K"]
    if fused_adam:
        what = "bwd-weight + fused Adam"
        body = ("p/m/v fp32 + bf16 shadow updated in the epilogue" if es == 2 else
                "p/m/v fp32 updated in the epilogue")
    else:
        what = "bwd-weight"
        body = "fp32 dW written for the all-reduce; Adam runs after the exchange"
    avg_s = statistics.fmean(durations_ms) / 1e3
    wl = {"dim": nat.enc_widths[0], "batch": batch, "dtype": nat.dtype_name,
          "model": "vib_ae" if nat.vib else "ae", "layer": layer}
    if len(layers) > 1:
        wl["layers"] = layers
    tf, _ = pmc_fields("dw", wl)
    shapes = ", ".join(f"layer {l}: dW[{nat.layers[l]['N']}x{nat.layers[l]['K']}]" for l in layers)
    kern = "mmad_gemm"
    # the bound is whichever resource the launch needs longer at its peak: HBM
    # for the bf16 launch (26 B/param of Adam state against bf16 MFMA), the
    # f32-input MFMA for the exact-fp32 one (1/16 of the bf16 rate)
    mpeak = BF16_PEAK_TFLOPS if es == 2 else F32_PEAK_TFLOPS
    hbm_bound = nbytes / (HBM_PEAK_GBS * 1e9) >= flops / (mpeak * 1e12)
    if hbm_bound:
        bound, ach, peak, unit = "hbm", nbytes / avg_s / 1e9, HBM_PEAK_GBS, "GB/s"
        other = {"mfma_tflops": round(flops / avg_s / 1e12, 2), "mfma_frac": round(flops / avg_s / 1e12 / mpeak, 4)}
    else:
        bound, ach, peak, unit = "mfma", flops / avg_s / 1e12, mpeak, "TFLOP/s"
        other = {"hbm_gbs": round(nbytes / avg_s / 1e9, 1), "hbm_frac": round(nbytes / avg_s / 1e9 / HBM_PEAK_GBS, 4)}
    return {"kernel": f"{kern} {what} ({shapes} = dz^T a over {rows} windows"
                      f"{'; both layers in one launch' if len(layers) > 1 else ''}; {body})",
            "bound": bound, "achieved": round(ach, 2), "peak": peak, "unit": unit,
            "frac": round(ach / peak, 4), **tf, **other,
            "avg_us": round(avg_s * 1e6, 2), "launches_timed": len(durations_ms),
            "algorithmic_bytes_per_launch": nbytes,
            "flops_per_launch": flops,
            **({"avg_us_isolated": round(statistics.fmean(isolated_ms) * 1e3, 2),
                "frac_isolated": round((nbytes if hbm_bound else flops / 1e3) /
                                       (statistics.fmean(isolated_ms) / 1e3) / 1e9 / peak, 4)}
               if in_timed and isolated_ms else {}),
            "timing": (f"executor probe inside the timed region: events attached to this launch "
                       f"(hipExtLaunchKernel start / stop) in each of the {steps_timed} timed steps, as "
                       f"it runs beside the side stream's work"
                       + ("; avg_us_isolated: the same launch alone (started once the side stream's "
                          "earlier work is done), in eager steps right after the timed region"
                          if isolated_ms else "")
                       if in_timed else
                       f"executor probe: HIP event pair around this launch on its stream, in "
                       f"{steps_timed} eager steps right after the timed region")}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="auto", choices=["auto"] + sorted(CONFIGS))
    ap.add_argument("--model", choices=["ae", "vib_ae"])
    ap.add_argument("--dim", type=int)
    ap.add_argument("--batch", type=int, help="windows per GPU per step")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: per-step spread, kernel "
                         "probes / rooflines, CPU baseline, c2 and c3_f32 sub-objects, N>1 same-workload run")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy (one GPU)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=12.0)
    ap.add_argument("--no-probe", action="store_true", help="skip the in-situ kernel probe")
    ap.add_argument("--soak-s", type=float, default=2.0,
                    help="untimed steps for about this many seconds after the warmup (0 = none)")
    ap.add_argument("--no-c2", action="store_true",
                    help="auto at N=1: skip the c2 sub-object (BASELINE configs[1]) in the same line")
    ap.add_argument("--no-f32", action="store_true",
                    help="auto at N=1: skip the c3_f32 sub-object (the exact-fp32 parity path at c3)")
    ap.add_argument("--stream", choices=["default", "own"], default="default",
                    help="own: run every step on a created non-blocking stream instead of the "
                         "caller's default stream (schedule studies, e.g. --tune side_cu_held=N)")
    ap.add_argument("--tune", action="append", default=[], metavar="KNOB=VALUE",
                    help="set a tune-table knob for the whole run (A/B of schedules; "
                         "icra2021_multimodal_ad_amd._native.KNOB names)")
    return ap.parse_args(argv)


def _spawn_entry(rank, world, port, argv):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    run(parse_args(argv))


def run(args):
    import torch
    from icra2021_multimodal_ad_amd import dist as mdist
    from icra2021_multimodal_ad_amd import _native

    # MMAD_BENCH_SHARED_GPU=1 (harness test only): every rank on cuda:0 over
    # gloo, so the N>1 launch / rendezvous / max-over-ranks / report path can be
    # exercised on a one-GPU box (RCCL refuses two ranks on one device)
    shared = os.environ.get("MMAD_BENCH_SHARED_GPU", "0") == "1"
    torch.cuda.set_device(0 if shared else int(os.environ.get("LOCAL_RANK", "0")))
    rank, world, local = mdist.init_from_env(backend="gloo" if shared else None)
    if shared:
        local = 0
    # auto: the largest single-GPU configuration on one GPU (c3 = BASELINE
    # configs[2], which is also C4's per-GPU shard, where the 1/2/4/8 curve
    # starts); c4 on several
    cname = args.config if args.config != "auto" else ("c3" if world == 1 else "c4")
    if args.dump_outputs and world > 1:
        raise SystemExit("--dump-outputs is a one-GPU option")
    for kv in args.tune:
        k, v = kv.split("=", 1)
        _native.tune_set(k, int(v))
    if args.stream == "own":
        torch.cuda.set_stream(torch.cuda.Stream())
    if cname == "c5":
        import bench_score
        if world > 1:
            raise SystemExit("c5 (scoring) is a one-GPU configuration")
        bench_score.run_c5(args)
        return
    cfgd = dict(CONFIGS[cname])
    for k in ("model", "dim", "batch"):
        if getattr(args, k) is not None:
            cfgd[k] = getattr(args, k)
    res, model = train_workload(args, cname, cfgd, rank, world, local, with_cpu=True, dump=True)
    if (args.full and rank == 0 and world == 1 and args.config == "auto" and not args.no_c2
            and all(getattr(args, k) is None for k in ("model", "dim", "batch"))):
        # the smaller BASELINE configs[1] in the same line, so the c2 series of
        # earlier rounds stays comparable (same steps / warmup, its own probes)
        del model
        model = None
        torch.cuda.synchronize()
        sub, _ = train_workload(args, "c2", dict(CONFIGS["c2"]), rank, world, local, with_cpu=False)
        keep = ("value", "unit", "ms_per_step", "steps", "warmup", "soak_steps", "config", "model_tflops",
                "host_enqueue_ms_per_step", "final_loss", "step_spread", "train_step", "roofline",
                "roofline_encoder_gemm")
        res["c2"] = {k: sub[k] for k in keep if k in sub}
        if not args.no_f32:
            # the same c3 workload on the exact-fp32 path (fp32 storage, f32-input
            # MFMA, apply-mode BatchNorm): the path the parity tests pin at 1e-4
            # (tests/test_gpu_vib_full.py), with its own rooflines against the
            # f32 MFMA peak
            torch.cuda.synchronize()
            a32 = argparse.Namespace(**vars(args))
            a32.dtype = "f32"
            sub, _ = train_workload(a32, "c3", dict(CONFIGS["c3"]), rank, world, local, with_cpu=False)
            res["c3_f32"] = {k: sub[k] for k in keep + ("dtype",) if k in sub}
            res["c3_f32"]["note"] = ("c3 on the exact-fp32 path (the one pinned within 1e-4 of the fp64 "
                                     "oracle); value / ms_per_step measured like the headline's")
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        if model.dist is not None and model.dist.native:
            model._native.set_comm(None)
            model.dist.close()
        dist.destroy_process_group()


DUMP_SAMPLE = 1 << 21     # elements of each large buffer --dump-outputs writes
DUMP_SEED = 20210530


def snapshot_state(model):
    """Everything a train step updates: the fp32 master parameters, the Adam
    moments and step count, the BatchNorm running statistics, the noise
    offset.  (The bf16 weight shadow is rebuilt from the master on restore.)"""
    nat = model._native
    return ([t.clone() for t in (nat.params, nat.exp_avg, nat.exp_avg_sq, nat.running)],
            nat.adam_step_count, model._rng_offset)


def restore_state(model, state):
    nat = model._native
    bufs, nat.adam_step_count, model._rng_offset = state
    for t, s in zip((nat.params, nat.exp_avg, nat.exp_avg_sq, nat.running), bufs):
        t.copy_(s)
    nat.sync_shadow(force=True)


def save_outputs(out_dir, arrays):
    """DIR/<name>.npy, float32 (numpy or device arrays)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if hasattr(a, "detach"):
            a = a.detach().float().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def dump_train_outputs(out_dir, nat, loss):
    """What the last timed train step handed back: its loss and the updated
    model / optimizer state.  The three n_params-sized buffers are sampled at
    the same DUMP_SAMPLE fixed, seeded positions (the whole buffer when it is
    smaller)."""
    import numpy as np
    import torch
    n = nat.n_params
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=DUMP_SAMPLE, replace=False))
        idx = torch.from_numpy(idx).to(nat.device)
        pick = lambda t: t[idx]   # noqa: E731
    else:
        pick = lambda t: t        # noqa: E731
    save_outputs(out_dir, {"loss": loss, "params": pick(nat.params), "adam_exp_avg": pick(nat.exp_avg),
                           "adam_exp_avg_sq": pick(nat.exp_avg_sq), "bn_running": nat.running})


def train_workload(args, cname, cfgd, rank, world, local, with_cpu, dump=False):
    """W untimed + K timed train steps of one workload; returns (result dict,
    model).  With --full the probes and the CPU baseline run after the timed
    region.  dump: this is the workload --dump-outputs writes."""
    import types
    import torch
    import torch.distributed as dist
    from icra2021_multimodal_ad_amd import dist as mdist
    from icra2021_multimodal_ad_amd import _native
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.data import synth_windows_device

    model_name, dim, batch = cfgd["model"], cfgd["dim"], cfgd["batch"]
    vib = model_name == "vib_ae"
    torch.cuda.set_device(local)
    cfg = types.SimpleNamespace(input_size=dim, btl_size=100, n_layers=5, gpu_id=local,
                                dtype=args.dtype, models=model_name, vib_k=1, beta_kl=1.0)
    torch.manual_seed(0)
    model = get_model(cfg)
    mdist.attach_data_parallel(model)
    if model.dist is not None and os.environ.get("MMAD_BENCH_DP_OVERLAP") in ("0", "1"):
        # A/B of the torch exchange (default: serial, dist.DataParallel.overlap)
        model.dist.overlap = os.environ["MMAD_BENCH_DP_OVERLAP"] == "1"
    model._native.sync_shadow(force=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    dev = torch.device("cuda", local)
    nat = model._native
    # a pool of distinct synthetic batches resident in HBM before timing
    pool = [synth_windows_device(batch, dim, dev, seed=1000 * rank + i) for i in range(8)]

    for i in range(args.warmup):
        model.train_step_async(pool[i % len(pool)], opt)
    torch.cuda.synchronize()
    # one GPU: the state the W warm-up steps left, put back before the timed
    # region -- the soak below is sized by time, so the number of updates it
    # applies differs from run to run
    state0 = snapshot_state(model) if world == 1 else None
    tw = time.perf_counter()                     # step time for the soak's length
    for i in range(10):
        model.train_step_async(pool[i % len(pool)], opt)
    torch.cuda.synchronize()
    # untimed soak: about args.soak_s seconds of the same steps before the
    # timed region, so it runs at the clock the chip holds under sustained
    # load (MI355X_MICROARCH.md 'DVFS give-back') and a sampling observer sees
    # the GPU busy; the same step count on every rank (DP steps exchange)
    per = (time.perf_counter() - tw) / 10
    soak = int(min(args.soak_s / max(per, 1e-5), 20000)) if args.soak_s > 0 else 0
    if world > 1:
        t = torch.tensor([soak], device=dev, dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        soak = int(t.item())
    for i in range(soak):
        model.train_step_async(pool[i % len(pool)], opt)
    torch.cuda.synchronize()
    if state0 is not None:
        restore_state(model, state0)
        del state0
        torch.cuda.synchronize()
    probe_layer = pick_dominant_layer(nat, batch)
    lib = _native.load()
    # the dominant dW launch timed inside the timed steps themselves: events
    # attached to that one launch (hipExtLaunchKernel start / stop, no marker
    # packet, no wait for the side stream; mmad_ae_probe kind 3), read after
    # the timed region
    probe_timed = args.full and not args.no_probe and rank == 0 and not nat.use_graph and args.steps > 0
    n_cap = min(args.steps, 4096)              # the executor's probe capacity limit: the first 4096 steps
    if probe_timed:
        _native.check(lib.mmad_ae_probe(nat._h, 3, probe_layer, n_cap), "mmad_ae_probe")
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = model.train_step_async(pool[i % len(pool)], opt)
    t_host = time.perf_counter() - t0           # enqueue time (no sync inside the loop)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # a fused-BN barrier or split-K combine that timed out leaves its launch's
    # outputs unwritten (sticky error word): such steps are not a measurement.
    # Every rank checks; the flag is all-reduced so all ranks stop together.
    bad = 0
    try:
        nat.check_status()
    except Exception as e:   # noqa: BLE001 -- reported below, on every rank
        print(f"[bench] rank {rank}: {e}", file=sys.stderr, flush=True)
        bad = 1
    if world > 1:
        t = torch.tensor([el, float(bad)], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el, bad = float(t[0].item()), int(t[1].item())
    if bad:
        raise SystemExit("bench: a kernel barrier timed out in the timed steps; no valid measurement")
    loss_v = float(loss.item())
    if args.dump_outputs and dump:
        dump_train_outputs(args.dump_outputs, nat, loss)
    durs_timed, layers_timed = [], None
    if probe_timed:
        import ctypes
        tbuf = (ctypes.c_float * n_cap)()
        nt = lib.mmad_ae_probe_read(nat._h, tbuf, n_cap)
        if nt < 0:
            _native.check(nt, "mmad_ae_probe_read")
        durs_timed = list(tbuf[:nt])
        tmask = lib.mmad_ae_probe_layers(nat._h)
        layers_timed = [l for l in range(len(nat.layers)) if tmask > 0 and (tmask >> l) & 1] or [probe_layer]
        _native.check(lib.mmad_ae_probe(nat._h, 1, -1, 0), "mmad_ae_probe")

    fpw, _ = ae_flops_per_window(nat.enc_widths, nat.dec_widths)
    windows = args.steps * batch * world
    value = windows / el
    exchange = ("native RCCL buckets (reduce-scatter" +
                (" of bf16 gradients" if getattr(nat, "_grad_bf16", None) is not None else "") +
                ", sharded Adam, all-gather) overlapped with backward"
                if model.dist is not None and model.dist.native else
                (("torch.distributed per-bucket all-reduce + Adam overlapped with backward"
                  if model.dist.overlapped else "torch.distributed flat all-reduce") if world > 1 else "none"))
    res = {
        "metric": "sensor-windows/sec (train fwd+bwd)",
        "value": round(value, 1),
        "unit": "sensor-windows/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "soak_steps": soak,
        "ms_per_step": round(el / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic (seeded 4-modal window generator, random-init weights)",
        "config": {"workload": f"{cname} ({cfgd['name']}): "
                               f"{'VIB-AE (k=1, beta_kl=1)' if vib else 'FC-AE'} train step "
                               f"(fwd+sum-MSE{'+KL' if vib else ''}+bwd+Adam), D={dim}, btl=100, "
                               f"n_layers=5, {batch} windows/GPU",
                   "global_batch": batch * world, "input_dim": dim,
                   "parallelism": f"dp{world}", "exchange": exchange},
        "model_tflops": round(value * fpw / 1e12, 2),
        "host_enqueue_ms_per_step": round(t_host / args.steps * 1e3, 4),
        "final_loss": loss_v,
    }
    if args.tune:
        res["tune"] = args.tune
    if args.full:
        # per-step spread: the same number of steps again, a HIP event after each
        # (on the caller's stream, which joins the side streams at every step end)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        evs[0].record()
        for i in range(args.steps):
            model.train_step_async(pool[i % len(pool)], opt)
            evs[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
        q = lambda f: per[min(len(per) - 1, int(f * len(per)))]   # noqa: E731
        res["step_spread"] = {"median_ms": round(q(0.5), 4), "p10_ms": round(q(0.1), 4),
                              "p90_ms": round(q(0.9), 4), "max_ms": round(per[-1], 4),
                              "steps": args.steps,
                              "how": "HIP event after every step, separate run right after the timed one"}
    if args.full and world > 1:
        # same workload without the exchange, same ranks (read scaling against it)
        mdl_dist = model.dist
        model.dist = None
        if mdl_dist is not None and mdl_dist.native:
            nat.set_comm(None)
        for i in range(5):
            model.train_step_async(pool[i % len(pool)], opt)
        torch.cuda.synchronize()
        n1 = max(10, args.steps // 2)
        t1 = time.perf_counter()
        for i in range(n1):
            model.train_step_async(pool[i % len(pool)], opt)
        torch.cuda.synchronize()
        e1 = time.perf_counter() - t1
        t = torch.tensor([e1], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        e1 = float(t.item())
        res["n1_same_workload"] = {"value": round(n1 * batch / e1, 1), "unit": "sensor-windows/sec per GPU",
                                   "ms_per_step": round(e1 / n1 * 1e3, 4), "steps": n1,
                                   "how": "same ranks, exchange off, after the timed region (max over ranks)"}
        model.dist = mdl_dist
    durs, n_probe, probe_layers, fwd_in_step = [], 0, None, []
    if args.full and not args.no_probe and rank == 0:
        # the same launch once more, isolated: eager steps of the same state
        # and inputs right after the timed region, each probed launch started
        # only once the side stream's earlier work is done (a HIP event pair
        # around it on its stream) -- the kernel alone, beside the in-step
        # figure above
        import ctypes
        n_probe = min(4096, max(20, args.steps // 4))
        graph_mode = nat.use_graph
        nat.use_graph = False
        _native.check(lib.mmad_ae_probe(nat._h, 1, probe_layer, n_probe), "mmad_ae_probe")
        # rank 0 alone: single-process fused steps (no collective the other
        # ranks would have to join; at N > 1 the exchange is already detached
        # from the executor by the n1_same_workload run above)
        probe_dist = model.dist
        model.dist = None
        with mdist.rank_local():      # a step that still carried the exchange raises here
            for i in range(n_probe):
                model.train_step_async(pool[i % len(pool)], opt)
        torch.cuda.synchronize()
        buf = (ctypes.c_float * n_probe)()
        n = lib.mmad_ae_probe_read(nat._h, buf, n_probe)
        if n < 0:
            _native.check(n, "mmad_ae_probe_read")
        durs = list(buf[:n])
        mask = lib.mmad_ae_probe_layers(nat._h)
        probe_layers = [l for l in range(len(nat.layers)) if mask > 0 and (mask >> l) & 1] or [probe_layer]
        # the encoder's first forward GEMM as it runs inside the step (train
        # mode: its epilogue also finishes the layer's BatchNorm -- column
        # barrier + y store -- when the fused schedule applies)
        _native.check(lib.mmad_ae_probe(nat._h, 0, 0, n_probe), "mmad_ae_probe")
        with mdist.rank_local():
            for i in range(n_probe):
                model.train_step_async(pool[i % len(pool)], opt)
        model.dist = probe_dist
        torch.cuda.synchronize()
        fbuf = (ctypes.c_float * n_probe)()
        nf = lib.mmad_ae_probe_read(nat._h, fbuf, n_probe)
        if nf < 0:
            _native.check(nf, "mmad_ae_probe_read")
        fwd_in_step = list(fbuf[:nf])
        _native.check(lib.mmad_ae_probe(nat._h, 1, -1, 0), "mmad_ae_probe")
        nat.use_graph = graph_mode
        nat.check_status()
    res["train_step"] = ("one captured hipGraph replay per step (mmad_ae_train_step_graph)"
                         if nat.use_graph and (model.dist is None or not model.dist.native)
                         else "eager executor step (mmad_ae_train_step)")
    if args.full and rank == 0:
        if durs_timed or durs:
            # fused steps (Adam in the dW epilogue): the timed steps' own
            # launches when they were probed, else the isolated probe steps
            res["roofline"] = dw_roofline(nat, probe_layer, durs_timed or durs, batch,
                                          len(durs_timed) or n_probe, fused_adam=True,
                                          layers=(layers_timed if durs_timed else probe_layers),
                                          in_timed=bool(durs_timed), isolated_ms=durs)
        res["roofline_encoder_gemm"] = gemm_roofline(model, batch)
        if fwd_in_step:
            import statistics
            r = res["roofline_encoder_gemm"]
            us = statistics.fmean(fwd_in_step) * 1e3
            r["in_step_us"] = round(us, 2)
            r["in_step_frac"] = round(r["flops_per_launch"] / (us * 1e-6) / 1e12 / r["peak"], 4)
            r["in_step_timing"] = (f"executor probe: HIP event pair around the layer-0 forward GEMM inside "
                                   f"{len(fwd_in_step)} eager train steps (its epilogue also finishes the "
                                   f"layer's train-mode BatchNorm in the fused schedule)")
        if with_cpu and not args.no_cpu_baseline and world == 1:   # host baseline: rank 0 at N=1 only
            res["cpu_baseline"] = cpu_baseline(dim, batch, vib, budget_s=args.cpu_budget)
    return res, model


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # spawn the ranks here (no GPU has been touched in this process)
        import socket
        import torch.multiprocessing as mp
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        mp.start_processes(_spawn_entry, args=(args.gpus, port, sys.argv[1:]), nprocs=args.gpus,
                           join=True, start_method="spawn")
        return
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}; "
              f"using WORLD_SIZE", file=sys.stderr)
    run(args)


if __name__ == "__main__":
    main()
