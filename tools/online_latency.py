"""Latency of scoring a few windows now: the batch path's entry points against
the online path (mmad_ae_online_score) -> profiles/online_latency.json.

Workload: the D = 2048, btl 100, 5-layer autoencoder, fp32 and bf16 handles,
B = 10 and 16 windows, a full-range fp32 NAP fit attached (W = R = 6442; the
fit's values are random but finite -- only the time matters here).  After 50
warm-up calls, median and 10th / 90th percentile of 300 calls, alternated in
one process, each as GPU time between two events and as host wall including
one stream synchronise:
  (a) mmad_ae_score_nap, eager
  (b) mmad_ae_score_nap_stream with N = batch = B, use_graph = 1
  (c) mmad_ae_online_score, replayed
  (c0) the same without a fit (no NAP launch)
Beside them the weight-stream lower bound: the bytes every pass has to read
once (AE weights + the encoder again + V^T) / 8 TB/s.

  python tools/online_latency.py [--out profiles/online_latency.json]
  python tools/online_latency.py --variant TAG --out FILE   # (c) / (c0) only, merged
      into FILE under "variants": a library built with other compile-time
      constants (MMAD_LIB=...: -DMMAD_SKINNY_NT=1, -DMMAD_SKINNY_WAVES=8)
  python tools/online_latency.py --rows64 [--out profiles/online_rows64_latency.json]
      the 64-row route (mmad_ae_online_score64): B = 10, 16, 17, 32, 64 on both
      handles, with the fit and without, each B's routes alternated in one
      process with the same warm-up and call counts:
        (b)   mmad_ae_score_nap_stream (without a fit: mmad_ae_score_stream),
              N = batch = B, graph-replayed
        (c16) mmad_ae_online_score, replayed, where B <= 16
        (c64) mmad_ae_online_score64, replayed
      and the two comparisons the documents rest on: c64 / b at every B, c64 /
      c16 at B <= 16 (a route is the faster one beyond the 3 % spread).
  python tools/online_latency.py --groups [--out profiles/online_groups_latency.json]
      per-modality scores (mmad_ae_online_score_groups): the grouped and the
      ungrouped pass alternated in one process at B = 10, 16 (16 rows) and 64
      (64 rows), both handles, with the fit (d0 read from the NAP operand) and
      without (d0 into the groups buffer); groups = the fused row's modality
      columns scaled to the model's D.  The grouped pass is one dependent
      launch more; a difference inside the 3 % spread decides nothing.
  python tools/online_latency.py --tick [--out profiles/online_tick_latency.json]
      the sensor tick in one graph (OnlineScorer.tick: one host-to-device copy
      and one replay of mmad_ae_online_tick) against score_sensors on the same
      scorer and the same raw queues, alternated call by call in one process:
      10 windows on 16 rows and 32 windows on 64 rows, the 1728-wide 3-layer
      fp32 model with the modality groups.  The baseline is the score_sensors
      of the same run; a GPU-time ratio inside 1 +- 3 % is no gain.
  python tools/online_latency.py --bank [--out profiles/online_bank_latency.json]
      the sensor bank (SensorBank.tick: one copy and one replay of
      mmad_online_bank_tick for all members) against the members' own calls one
      after another (the fused scorer's tick, then each unimodal scorer's score
      on its columns of the fused row), and a one-member bank against
      OnlineScorer.tick; 10 windows on 16 rows and 32 windows on 64 rows; five
      fp32 members of D = 1728 / 1024 / 512 / 64 / 128, btl 100, 5 layers, a
      full-range fp32 fit on the fused one.  Pairs alternate call by call in one
      process; a GPU-time ratio inside 1 +- 3 % decides nothing."""
import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icra2021_multimodal_ad_amd import _native  # noqa: E402
from icra2021_multimodal_ad_amd._native import pad, ptr, stream_ptr  # noqa: E402

WARMUP, CALLS = 50, 300
HBM_BYTES_PER_S = 8e12


def build(dtype):
    from icra2021_multimodal_ad_amd.model_builder import get_model
    cfg = types.SimpleNamespace(input_size=2048, btl_size=100, n_layers=5, gpu_id=0, dtype=dtype, models="ae")
    torch.manual_seed(3)
    m = get_model(cfg)
    m.eval()
    return m


def random_fit(nat):
    W = nat.diff_width()
    R, Kp, Rp = W, pad(W), pad(W)
    g = torch.Generator(device="cuda").manual_seed(7)
    vt = torch.zeros((Rp, Kp), device="cuda")
    vt[:R, :W] = torch.randn((R, W), device="cuda", generator=g) / W ** 0.5
    bias = torch.zeros(Rp, device="cuda")
    bias[:R] = 0.1 * torch.randn(R, device="cuda", generator=g)
    w = torch.zeros(Rp, device="cuda")
    w[:R] = torch.rand(R, device="cuda", generator=g) + 0.5
    return R, vt, bias, w


def stream_bytes(nat, with_nap):
    e = 2 if nat.dtype_name == "bf16" else 4
    ae = sum(L["Np"] * L["Kp"] for L in nat.layers) * e
    enc = sum(L["Np"] * L["Kp"] for L in nat.layers[:nat.n_enc]) * e
    vt = pad(nat.diff_width()) ** 2 * 4 if with_nap else 0
    return ae + enc + vt


def measure(fns):
    """fns: {name: callable enqueueing one call on the current stream}."""
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

    def stats(v):
        p = np.percentile(np.asarray(v), [50, 10, 90])
        return {"median_us": float(p[0]), "p10_us": float(p[1]), "p90_us": float(p[2])}
    return {k: {"gpu": stats(gpu[k]), "wall": stats(wall[k])} for k in fns}


def run_case(dtype, B, variant):
    lib = _native.load()
    m = build(dtype)
    nat = m._native
    h, s = nat._h, stream_ptr()
    D, n = nat.enc_widths[0], nat.n_enc
    x = torch.randn((16, D), device="cuda")
    out = torch.zeros((n + 4, 16), device="cuda")
    flags = torch.zeros((3, 16), device="cuda", dtype=torch.uint8)
    thr = torch.ones(3, device="cuda")
    nat.sync_shadow()

    def online(state):
        base = state.data_ptr()
        al = (base + 255) // 256 * 256
        args = (h, ptr(x), D, B, 0, n + 2, ptr(thr), ptr(out), ptr(flags), ctypes.c_void_p(al),
                state.numel() - (al - base), 1, s)

        def fn():
            _native.check(lib.mmad_ae_online_score(*args), "mmad_ae_online_score")
        return fn

    res = {}
    state0 = nat.online_state()
    res.update(measure({"c0_online_no_nap": online(state0)}))
    fit = random_fit(nat)
    nat.set_nap(fit)
    state1 = nat.online_state()
    fns = {"c_online": online(state1)}
    if not variant:
        ws, nb = nat.workspace(B, 1)
        lsq = torch.zeros((n + 1, B), device="cuda")
        nap = torch.zeros(B, device="cuda")
        a_args = (h, ptr(x), D, B, ptr(lsq), ptr(nap), ws, nb, s)
        b_args = (h, ptr(x), D, B, B, ptr(lsq), B, ptr(nap), ws, nb, 1, s)
        fns = {"a_score_nap_eager": lambda: _native.check(lib.mmad_ae_score_nap(*a_args), "a"),
               "b_score_nap_stream_graph": lambda: _native.check(lib.mmad_ae_score_nap_stream(*b_args), "b"),
               "c_online": fns["c_online"]}
    res.update(measure(fns))
    assert torch.isfinite(out[:, :B]).all()
    res["weight_stream_bound_us"] = {"with_nap": stream_bytes(nat, True) / HBM_BYTES_PER_S * 1e6,
                                     "no_nap": stream_bytes(nat, False) / HBM_BYTES_PER_S * 1e6}
    nat.set_nap(None)
    return res


ROWS64_B = (10, 16, 17, 32, 64)
SPREAD = 0.03   # box-to-box spread: a ratio inside 1 +- SPREAD decides nothing


def run_rows64(dtype):
    lib = _native.load()
    m = build(dtype)
    nat = m._native
    h, s = nat._h, stream_ptr()
    D, n = nat.enc_widths[0], nat.n_enc
    x = torch.randn((64, D), device="cuda")
    thr = torch.ones(3, device="cuda")
    outs = {r: torch.zeros((n + 4, r), device="cuda") for r in (16, 64)}
    flags = {r: torch.zeros((3, r), device="cuda", dtype=torch.uint8) for r in (16, 64)}
    nat.sync_shadow()

    def online(rows, B, state):
        base = state.data_ptr()
        al = (base + 255) // 256 * 256
        name = "mmad_ae_online_score" + ("" if rows == 16 else "64")
        fn_, args = getattr(lib, name), (h, ptr(x), D, B, 0, n + 2, ptr(thr), ptr(outs[rows]), ptr(flags[rows]),
                                         ctypes.c_void_p(al), state.numel() - (al - base), 1, s)
        return lambda: _native.check(fn_(*args), name)

    cases = {}
    for with_nap in (False, True):
        if with_nap:
            fit = random_fit(nat)
            nat.set_nap(fit)
        states = {r: nat.online_state(r) for r in (16, 64)}   # sized for the handle as it stands
        for B in ROWS64_B:
            ws, nb = nat.workspace(B, 1)
            lsq = torch.zeros((n + 1, B), device="cuda")
            nap = torch.zeros(B, device="cuda")
            if with_nap:
                b_args = (h, ptr(x), D, B, B, ptr(lsq), B, ptr(nap), ws, nb, 1, s)
                b_fn = lambda a_=b_args: _native.check(lib.mmad_ae_score_nap_stream(*a_), "b")
            else:
                b_args = (h, ptr(x), D, B, B, ptr(lsq), B, ws, nb, 1, s)
                b_fn = lambda a_=b_args: _native.check(lib.mmad_ae_score_stream(*a_), "b")
            fns = {"b_batch_stream_graph": b_fn}
            if B <= 16:
                fns["c16_online"] = online(16, B, states[16])
            fns["c64_online"] = online(64, B, states[64])
            res = measure(fns)
            assert torch.isfinite(outs[64][:n + 3, :B]).all() and torch.isfinite(lsq).all()
            # the two routes' layer sums agree (fp32: another summation order; bf16: its rounding)
            rel = float(((outs[64][:n + 1, :B] - lsq).abs().max() / lsq.abs().max()).item())
            assert rel < (1e-3 if dtype == "f32" else 1e-1), rel
            if B <= 16:
                assert torch.equal(outs[64][:n + 3, :B], outs[16][:n + 3, :B])
            med = {k: v["gpu"]["median_us"] for k, v in res.items()}
            res["c64_vs_b_gpu"] = med["c64_online"] / med["b_batch_stream_graph"]
            if B <= 16:
                res["c64_vs_c16_gpu"] = med["c64_online"] / med["c16_online"]
            res["layer_sq_max_rel_diff_c64_vs_b"] = rel
            res["weight_stream_bound_us"] = stream_bytes(nat, with_nap) / HBM_BYTES_PER_S * 1e6
            cases[f"{dtype}_{'nap' if with_nap else 'nonap'}_B{B}"] = res
            print(f"{dtype} nap={int(with_nap)} B={B}", {k: round(v, 1) for k, v in med.items()}, flush=True)
    nat.set_nap(None)
    return cases


GROUPS_B = (10, 16, 64)
FUSED_BOUNDS = (0, 1024, 1536, 1600, 1728)


def run_groups(dtype):
    lib = _native.load()
    m = build(dtype)
    nat = m._native
    h, s = nat._h, stream_ptr()
    D, n = nat.enc_widths[0], nat.n_enc
    bounds = [round(c * D / FUSED_BOUNDS[-1]) for c in FUSED_BOUNDS]
    G = len(bounds) - 1
    cb = (ctypes.c_int * len(bounds))(*bounds)
    x = torch.randn((64, D), device="cuda")
    thr, gthr = torch.ones(3, device="cuda"), torch.ones(G, device="cuda")
    nat.sync_shadow()
    cases = {}
    for with_nap in (False, True):
        if with_nap:
            fit = random_fit(nat)
            nat.set_nap(fit)
        for B in GROUPS_B:
            rows = 16 if B <= 16 else 64
            # each pass its own outputs and state: neither replays into the other's buffers
            bufs = {}
            for tag in ("plain", "grouped"):
                state = nat.online_state(rows)
                al = (state.data_ptr() + 255) // 256 * 256
                bufs[tag] = (torch.zeros((n + 4, rows), device="cuda"),
                             torch.zeros((3, rows), device="cuda", dtype=torch.uint8), state,
                             (ctypes.c_void_p(al), state.numel() - (al - state.data_ptr())))
            gstate = nat.online_groups_state(rows)
            gal = (gstate.data_ptr() + 255) // 256 * 256
            gout = torch.zeros((G, rows), device="cuda")
            gflags = torch.zeros((G, rows), device="cuda", dtype=torch.uint8)
            o, f, _, (sp, sb) = bufs["plain"]
            p_fn = getattr(lib, "mmad_ae_online_score" + ("" if rows == 16 else "64"))
            p_args = (h, ptr(x), D, B, 0, n + 2, ptr(thr), ptr(o), ptr(f), sp, sb, 1, s)
            o2, f2, _, (sp2, sb2) = bufs["grouped"]
            g_args = (h, ptr(x), D, B, 0, n + 2, ptr(thr), ptr(o2), ptr(f2), sp2, sb2, 1, s, rows, cb, G,
                      ptr(gthr), ptr(gout), ptr(gflags), ctypes.c_void_p(gal),
                      gstate.numel() - (gal - gstate.data_ptr()))
            res = measure({"ungrouped": lambda: _native.check(p_fn(*p_args), "ungrouped"),
                           "grouped": lambda: _native.check(lib.mmad_ae_online_score_groups(*g_args), "grouped")})
            assert torch.equal(o[:n + 3, :B], o2[:n + 3, :B]) and torch.isfinite(gout).all()
            assert (gout[:, :B] > 0).all() and (gout[:, B:] == 0).all()
            med = {k: v["gpu"]["median_us"] for k, v in res.items()}
            res["grouped_minus_ungrouped_gpu_us"] = med["grouped"] - med["ungrouped"]
            res["grouped_vs_ungrouped_gpu"] = med["grouped"] / med["ungrouped"]
            res["rows"] = rows
            cases[f"{dtype}_{'nap' if with_nap else 'nonap'}_B{B}"] = res
            print(f"{dtype} nap={int(with_nap)} B={B}", {k: round(v, 1) for k, v in med.items()}, flush=True)
    nat.set_nap(None)
    return bounds, cases


TICK_CASES = ((10, 16), (32, 64))   # (windows a tick, row capacity)


def run_tick(B, rows):
    """OnlineScorer.tick (one copy + one graph launch, mmad_ae_online_tick)
    against score_sensors on the same scorer and queues, call by call."""
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    torch.manual_seed(7)
    net = HSR_Net(False, types.SimpleNamespace(slicing_size=B, batch_size=B, gpu_id=0)).cuda()
    torch.manual_seed(8)
    model = get_model(types.SimpleNamespace(input_size=1728, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                            models="ae"))
    rng = np.random.Generator(np.random.PCG64(81))
    hand_q = rng.integers(0, 256, size=(B, 32 * 32 * 3)).astype(np.uint8)
    depth_q = rng.integers(0, 256, size=(B, 32 * 32)).astype(np.uint8)
    force_q = rng.uniform(0, 400, size=B)
    pcm = rng.integers(-8000, 8000, size=(B + 1) * 4410 - 2205).astype(np.int16)   # B + 1 frames
    sc = OnlineScorer(model, rows=rows, groups=net.modality_columns())
    sc.bind_sensors(net, len(pcm))
    q = (force_q, hand_q, depth_q, pcm)
    keep = lambda r: {k: v.clone() for k, v in r.items() if v is not None}   # noqa: E731
    a, b = keep(sc.tick(*q)), keep(sc.score_sensors(net, *q))
    same_bits = all(torch.equal(a[k], b[k]) for k in a)
    rel = float(((a["base"] - b["base"]).abs().max() / b["base"].abs().max()).item())
    res = measure({"score_sensors": lambda: sc.score_sensors(net, *q), "tick": lambda: sc.tick(*q)})
    for kind in ("gpu", "wall"):
        s, t = res["score_sensors"][kind], res["tick"][kind]
        res[f"tick_minus_score_sensors_{kind}_us"] = t["median_us"] - s["median_us"]
        res[f"tick_vs_score_sensors_{kind}"] = t["median_us"] / s["median_us"]
    res.update(B=B, rows=rows, pcm_samples=len(pcm), tick_equals_score_sensors_bits=same_bits,
               base_max_rel_diff=rel, tick_host_calls="1 copy_ + 1 hipGraphLaunch")
    print(f"tick B={B} rows={rows}", {k: (round(v["gpu"]["median_us"], 1), round(v["wall"]["median_us"], 1))
                                     for k, v in res.items() if isinstance(v, dict) and "gpu" in v},
          f"bits equal: {same_bits}", flush=True)
    return res


BANK_WIDTHS = {"All": 1728, "hand_camera": 1024, "head_depth": 512, "force_torque": 64, "mic": 128}


def bank_members(rows, names):
    """name -> OnlineScorer over a btl-100, 5-layer fp32 model of that sensor's
    width (a full-range fp32 fit with random values on the fused member)."""
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    out = {}
    for i, name in enumerate(names):
        torch.manual_seed(20 + i)
        m = get_model(types.SimpleNamespace(input_size=BANK_WIDTHS[name], btl_size=100, n_layers=5, gpu_id=0,
                                            dtype="f32", models="ae"))
        m.eval()
        if name == "All":
            fit = random_fit(m._native)
            m._native.set_nap(fit)
            m._fit = fit                     # the handle reads these buffers: keep them alive
        out[name] = OnlineScorer(m, rows=rows)
    return out


def run_bank(B, rows):
    """SensorBank.tick against the members' own calls one after another (what
    the deployment loop had to do before the bank: the fused scorer's tick,
    then every unimodal scorer's ``score`` on its columns of the fused row the
    tick left on the device), and a one-member bank against OnlineScorer.tick.
    Each pair alternates call by call in one process; the two sides of a pair
    run on their own model copies (the same seeds), so neither re-zeroes the
    other's NAP operand."""
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.online import SensorBank
    torch.manual_seed(7)
    net = HSR_Net(False, types.SimpleNamespace(slicing_size=B, batch_size=B, gpu_id=0)).cuda()
    rng = np.random.Generator(np.random.PCG64(81))
    hand_q = rng.integers(0, 256, size=(B, 32 * 32 * 3)).astype(np.uint8)
    depth_q = rng.integers(0, 256, size=(B, 32 * 32)).astype(np.uint8)
    force_q = rng.uniform(0, 400, size=B)
    pcm = rng.integers(-8000, 8000, size=(B + 1) * 4410 - 2205).astype(np.int16)   # B + 1 frames
    q = (force_q, hand_q, depth_q, pcm)
    keep = lambda r: {k: v.clone() for k, v in r.items() if v is not None}   # noqa: E731
    names = tuple(BANK_WIDTHS)
    res = {"B": B, "rows": rows, "pcm_samples": len(pcm)}

    # ---- five members: the bank against the members in sequence
    bank = SensorBank.for_sensors(net, bank_members(rows, names)).bind_sensors(net, len(pcm))
    seq = bank_members(rows, names)
    seq["All"].bind_sensors(net, len(pcm))
    cols = bank.columns

    def sequence():
        out = {"All": seq["All"].tick(*q)}
        row = seq["All"].x
        for n in names[1:]:
            c0, c1 = cols[n]
            out[n] = seq[n].score(row[:B, c0:c1])
        return out
    a, b = bank.tick(*q), sequence()
    res["five_members_bits_equal"] = all(torch.equal(a[n][k], b[n][k]) for n in names for k in keep(a[n]))
    m5 = measure({"members_in_sequence": sequence, "bank_tick": lambda: bank.tick(*q)})
    res["five_members"] = m5
    res["five_members"]["graph_nodes"] = bank.graph_nodes()
    # ---- one member: the bank against OnlineScorer.tick
    bank1 = SensorBank.for_sensors(net, bank_members(rows, ("All",))).bind_sensors(net, len(pcm))
    single = bank_members(rows, ("All",))["All"].bind_sensors(net, len(pcm))
    a, b = keep(bank1.tick(*q)["All"]), keep(single.tick(*q))
    res["one_member_bits_equal"] = all(torch.equal(a[k], b[k]) for k in a)
    m1 = measure({"scorer_tick": lambda: single.tick(*q), "bank_tick": lambda: bank1.tick(*q)})
    res["one_member"] = m1
    res["one_member"]["graph_nodes"] = bank1.graph_nodes()
    for kind in ("gpu", "wall"):
        res[f"bank5_vs_sequence_{kind}"] = (m5["bank_tick"][kind]["median_us"]
                                            / m5["members_in_sequence"][kind]["median_us"])
        res[f"bank1_vs_scorer_tick_{kind}"] = m1["bank_tick"][kind]["median_us"] / m1["scorer_tick"][kind]["median_us"]
    print(f"bank B={B} rows={rows}",
          {k: (round(v["gpu"]["median_us"], 1), round(v["wall"]["median_us"], 1)) for k, v in m5.items()
           if isinstance(v, dict)},
          {k: (round(v["gpu"]["median_us"], 1), round(v["wall"]["median_us"], 1)) for k, v in m1.items()
           if isinstance(v, dict)},
          f"bits equal: {res['five_members_bits_equal']} {res['one_member_bits_equal']}", flush=True)
    bank.close()
    bank1.close()
    return res


def main_bank(out):
    cases = {f"f32_B{B}_rows{rows}": run_bank(B, rows) for B, rows in TICK_CASES}
    doc = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "spread": SPREAD,
           "members": {n: f"input {d}, btl 100, 5 layers, fp32" + (", full-range fp32 fit" if n == "All" else "")
                       for n, d in BANK_WIDTHS.items()},
           "cases": cases,
           "bank5_faster_than_sequence_outside_spread": {k: c["bank5_vs_sequence_gpu"] for k, c in cases.items()
                                                         if c["bank5_vs_sequence_gpu"] < 1 - SPREAD},
           "bank1_slower_than_scorer_tick_outside_spread": {k: c["bank1_vs_scorer_tick_gpu"]
                                                            for k, c in cases.items()
                                                            if c["bank1_vs_scorer_tick_gpu"] > 1 + SPREAD}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


def main_tick(out):
    cases = {f"f32_B{B}_rows{rows}": run_tick(B, rows) for B, rows in TICK_CASES}
    doc = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "spread": SPREAD,
           "model": "input 1728, btl 16, 3 layers, fp32, groups = the fused row's modality columns",
           "cases": cases,
           "gpu_gain_outside_spread": {k: c["tick_vs_score_sensors_gpu"] for k, c in cases.items()
                                       if c["tick_vs_score_sensors_gpu"] < 1 - SPREAD}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


def main_groups(out):
    cases = {}
    for dt in ("f32", "bf16"):
        bounds, c = run_groups(dt)
        cases.update(c)
    doc = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "spread": SPREAD,
           "bounds": bounds, "cases": cases,
           "outside_spread": {k: c["grouped_vs_ungrouped_gpu"] for k, c in cases.items()
                              if abs(c["grouped_vs_ungrouped_gpu"] - 1) > SPREAD}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


def main_rows64(out):
    cases = {}
    for dt in ("f32", "bf16"):
        cases.update(run_rows64(dt))
    faster_than_b = {}
    for dt in ("f32", "bf16"):
        for tag in ("nap", "nonap"):
            faster_than_b[f"{dt}_{tag}"] = [B for B in ROWS64_B
                                            if cases[f"{dt}_{tag}_B{B}"]["c64_vs_b_gpu"] < 1 - SPREAD]
    doc = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "spread": SPREAD, "cases": cases,
           "c64_faster_than_b_at_B": faster_than_b,
           "c64_slower_than_c16_at_B": {k: c["c64_vs_c16_gpu"] for k, c in cases.items()
                                        if c.get("c64_vs_c16_gpu", 0) > 1 + SPREAD}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", default=None)
    ap.add_argument("--rows64", action="store_true")
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--tick", action="store_true")
    ap.add_argument("--bank", action="store_true")
    a = ap.parse_args()
    _native.require_gpu()
    if a.bank:
        return main_bank(a.out or "profiles/online_bank_latency.json")
    if a.tick:
        return main_tick(a.out or "profiles/online_tick_latency.json")
    if a.rows64:
        return main_rows64(a.out or "profiles/online_rows64_latency.json")
    if a.groups:
        return main_groups(a.out or "profiles/online_groups_latency.json")
    a.out = a.out or "profiles/online_latency.json"
    cases = {f"{dt}_B{B}": run_case(dt, B, a.variant) for dt in ("f32", "bf16") for B in (10, 16)}
    if a.variant:
        doc = json.load(open(a.out))
        doc.setdefault("variants", {})[a.variant] = {"lib": os.path.basename(os.environ.get("MMAD_LIB", "")), "cases": cases}
    else:
        doc = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS,
               "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": cases}
        for k, c in cases.items():
            b, cc = c["b_score_nap_stream_graph"]["gpu"]["median_us"], c["c_online"]["gpu"]["median_us"]
            c["online_vs_b_gpu"] = cc / b
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    for k, c in cases.items():
        print(k, {n_: (round(v["gpu"]["median_us"], 1), round(v["wall"]["median_us"], 1))
                  for n_, v in c.items() if isinstance(v, dict) and "gpu" in v})


if __name__ == "__main__":
    main()
