"""Grouped dW launches of the ping-pong step (mmad_ae_set_dw_group,
mmad_gemm_dispatch_group): consecutive narrow layers' dW + Adam GEMMs issued
as one launch give the separate launches' bits -- parameters, both Adam
moments, the bf16 shadow, the BN running statistics and the losses -- whatever
the block budget and member cap, and a group the plan or the dispatcher turns
down runs as separate launches."""
import ctypes
import functools
import types

import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd.data import synth_windows

pytestmark = pytest.mark.gpu

STATE = ("params", "exp_avg", "exp_avg_sq", "running")


def _run(model, d, dtype, rows, knobs, probe_layer=-1, step_knobs=(), steps=3):
    """`steps` fused train steps of a fresh model from one seed under `knobs`
    (set while the model is built; `step_knobs` then and while it steps: a
    handle takes the split-K slabs only if a split knob is set when it is
    created).  Returns (state tensors on the host, losses, probe layer mask of
    the last step)."""
    from icra2021_multimodal_ad_amd.model_builder import get_model
    lib = _native.load()
    knobs, step_knobs = dict(knobs), dict(step_knobs)
    cfg = types.SimpleNamespace(input_size=d, btl_size=16, n_layers=5, gpu_id=0, dtype=dtype, models=model)
    torch.manual_seed(8)
    with _native.tune(**knobs, **step_knobs):
        m = get_model(cfg)
    nat = m._native
    nat.sync_shadow(force=True)
    if probe_layer >= 0:
        assert lib.mmad_ae_probe(nat._h, 3, probe_layer, steps) == 0
    losses = []
    with _native.tune(**step_knobs):
        for s in range(steps):
            x = torch.from_numpy(synth_windows(rows, d, seed=40 + s)).cuda()
            losses.append(float(nat.train_step_fused(x, beta_kl=1.0)))
    torch.cuda.synchronize()
    nat.check_status()
    mask = lib.mmad_ae_probe_layers(nat._h) if probe_layer >= 0 else 0
    if probe_layer >= 0:
        buf = (ctypes.c_float * steps)()
        assert lib.mmad_ae_probe_read(nat._h, buf, steps) == steps
        assert lib.mmad_ae_probe(nat._h, 1, -1, 0) == 0
    out = {n: getattr(nat, n).cpu() for n in STATE}
    out["shadow"] = nat.shadow.cpu() if nat.shadow is not None else None
    return out, losses, mask, nat.layers


@functools.lru_cache(maxsize=None)
def _separate(model, d, dtype, rows, extra=()):
    """The reference: every dW its own launch (budget 0), computed once."""
    return _run(model, d, dtype, rows, dict(extra, pair_rows=0, dw_group=0))[:2]


def _assert_same(got, want):
    (a, la), (b, lb) = got, want
    assert la == lb, (la, lb)
    for n in STATE:
        assert torch.equal(a[n], b[n]), n
    if b["shadow"] is not None:
        assert torch.equal(a["shadow"], b["shadow"])


def _plan_mask(layers, rows, budget, members, probe_layer, dw_main=1):
    """Layer mask of the launch holding `probe_layer` under the grouping rule."""
    lib = _native.load()
    n = len(layers)
    arr = ctypes.c_int * n
    g = arr()
    lib.mmad_dw_group_plan(n, arr(*[L["Np"] for L in layers]), arr(*[L["Kp"] for L in layers]),
                           arr(*[_native.pad(rows)] * n), dw_main, n, budget, members, g)
    if g[probe_layer] < 0:
        return 1 << probe_layer
    return sum(1 << l for l in range(n) if g[l] == g[probe_layer])


def _popcount(v):
    return bin(v).count("1")


SETTINGS = {"all_fit": dict(dw_group=-1), "pairs": dict(dw_group=-1, dw_group_members=2),
            "budget32": dict(dw_group=32)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("rows", [256, 200])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_grouped_dw_matches_separate_launches(dtype, rows, setting):
    """VIB-AE D=256, btl=16, 5+5 layers (every dW on the 64x64 tile), full and
    ragged rows: one resident round, groups of two and a 32-block budget all
    give the bits of budget 0.  bf16 (ping-pong with pair_rows=0) really
    groups: the probe of layer 3's dW names the members the rule gives; fp32
    has no ping-pong schedule and keeps one launch per layer."""
    knobs = dict(SETTINGS[setting], pair_rows=0)
    out, losses, mask, layers = _run("vib_ae", 256, dtype, rows, knobs, probe_layer=3)
    _assert_same((out, losses), _separate("vib_ae", 256, dtype, rows))
    if dtype == "bf16":
        budget = 512 if knobs["dw_group"] < 0 else knobs["dw_group"]
        want = _plan_mask(layers, rows, budget, knobs.get("dw_group_members", 4), 3)
        assert _popcount(want) >= 2 and mask == want, (mask, want)
        if setting == "pairs":
            assert _popcount(mask) == 2
    else:
        assert mask == 1 << 3


@pytest.mark.parametrize("bn_mode", [1, -1])
def test_unequal_members(bn_mode):
    """D=640 at 512 rows: the top group's members have 100, 80, 48 and 24 tiles
    (100 is padded to 104 blocks, and first_block is searched over unequal
    ranges); the lower group holds the VIB layer (4; its bias partials come
    from the reparametrisation backward) beside layers behind a train-mode BN
    producer -- with bn_mode 1 (fold) their dW is fixed up in the epilogue
    (b_scale / b_shift, bias partials from gb_src)."""
    extra = (("bn_mode", bn_mode),)
    knobs = dict(extra, pair_rows=0, dw_group=-1)
    out, losses, mask, layers = _run("vib_ae", 640, "bf16", 512, knobs, probe_layer=4)
    _assert_same((out, losses), _separate("vib_ae", 640, "bf16", 512, extra))
    tiles = [(L["Np"] // 64) * (L["Kp"] // 64) for L in layers]
    assert tiles[9] % 8 != 0 and len({tiles[l] for l in (6, 7, 8, 9)}) == 4
    assert mask == _plan_mask(layers, 512, 512, 4, 4)
    assert (mask >> 4) & 1 and (mask >> 3) & 1 and _popcount(mask) >= 3
    _, _, top, _ = _run("vib_ae", 640, "bf16", 512, knobs, probe_layer=9, steps=1)
    assert top == sum(1 << l for l in (6, 7, 8, 9))


@pytest.mark.parametrize("case", ["budget", "tile", "splitk"])
def test_refused_group_runs_separately(case):
    """No group, one launch per layer (the probe's mask names one layer), a
    clean status and the separate launches' bits when (budget) no two members
    fit the block budget, (tile) knob 5 sends every dW to the 128x128 tile, or
    (splitk) the plan forms groups but the dispatcher refuses them because
    knob 9 splits every dW GEMM over K."""
    knobs, step_knobs, extra = dict(pair_rows=0, dw_group=-1), {}, ()
    if case == "budget":
        knobs["dw_group"] = 8
    elif case == "tile":
        step_knobs = {"tile_adam": 0}
    else:
        step_knobs = {"splitk_dw": 2}
    out, losses, mask, _ = _run("vib_ae", 256, "bf16", 512, knobs, probe_layer=3, step_knobs=step_knobs)
    assert mask == 1 << 3
    ref = _run("vib_ae", 256, "bf16", 512, dict(pair_rows=0, dw_group=0), step_knobs=step_knobs)[:2]
    _assert_same((out, losses), ref)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_group_kernel_matches_single_launches(dtype):
    """The grouped kernel itself, both instantiations, through the layer
    operator mmad_fc_bwd_weight_group: three plain dW GEMMs (12, 100 and 8
    tiles of 64x64, 192 valid rows of 256) in one launch equal
    mmad_fc_bwd_weight's outputs on the same tile bit for bit."""
    lib = _native.load()
    dt = _native.BF16 if dtype == "bf16" else _native.F32
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    shapes = [(64 * 5, 64), (640, 640), (128, 256)]   # (N, K): dW is [Np][Kp]
    Mp, M = 256, 192
    g = torch.Generator().manual_seed(3)
    dys, xs, want, got = [], [], [], []
    for n, k in shapes:
        n_p, k_p = _native.pad(n), _native.pad(k)
        dy = torch.zeros(Mp, n_p)
        dy[:M, :n] = torch.randn(M, n, generator=g)
        x = torch.zeros(Mp, k_p)
        x[:M, :k] = torch.randn(M, k, generator=g)
        dys.append(dy.to(tdt).cuda())
        xs.append(x.to(tdt).cuda())
        want.append(torch.zeros(n_p, k_p, device="cuda"))
        got.append(torch.full((n_p, k_p), 7.0, device="cuda"))
        with _native.tune(tile=3):
            _native.call("mmad_fc_bwd_weight", dt, Mp, n_p, k_p, _native.ptr(dys[-1]), _native.ptr(xs[-1]),
                         _native.ptr(want[-1]), _native.stream_ptr())
    n = len(shapes)
    ia, pa = ctypes.c_int * n, ctypes.c_void_p * n
    rc = lib.mmad_fc_bwd_weight_group(dt, n, Mp, ia(*[t.shape[0] for t in want]),
                                      ia(*[t.shape[1] for t in want]), pa(*[t.data_ptr() for t in dys]),
                                      pa(*[t.data_ptr() for t in xs]), pa(*[t.data_ptr() for t in got]),
                                      _native.stream_ptr())
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
        assert float(b.abs().max()) > 0
