"""The sensor bank against its scorers on the GPU: SensorBank.score equals, key
by key and bit for bit, every member scorer's own score on its columns of the
shared row -- first call, replays, both row capacities; the captured pass has
the launch count the design promises; the refusals launch nothing.

Members (tests/online_fixture.py's models and fit):
  ae   fp32 AE   D = 192, 5 layers, full-range NAP fit, groups   columns   0..192
  bf   bf16 AE   D = 64,  5 layers, btl 100 (widths expand)      columns 128..192
  vib  fp32 VIB  D = 128, 3 layers (shallower)                   columns  64..192"""
import types

import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd.data import synth_windows
from icra2021_multimodal_ad_amd.online import OnlineScorer, SensorBank
from tests.online_fixture import _fit, _model

pytestmark = pytest.mark.gpu

COLS = {"ae": 0, "bf": 128, "vib": 64}
GROUPS = {"a": (0, 101), "b": (101, 107), "c": (107, 192)}
THR = {"base": 0.05, "sap": 0.05, "nap": 1.0, "groups": {"a": 0.05, "c": -1.0}}
KEYS = ("base", "sap", "nap", "layer_sq", "flags", "groups", "group_flags")


def small(d, btl, n_layers, dtype, models, seed):
    from icra2021_multimodal_ad_amd.model_builder import get_model
    torch.manual_seed(seed)
    m = get_model(types.SimpleNamespace(input_size=d, btl_size=btl, n_layers=n_layers, gpu_id=0, dtype=dtype,
                                        models=models))
    m.eval()
    return m


@pytest.fixture(scope="module")
def models(golden):
    ae = _model(golden)
    return {"ae": ae, "bf": small(64, 100, 5, "bf16", "ae", 21), "vib": small(128, 16, 3, "f32", "vib_ae", 22),
            "fit": _fit(ae, (0, 6))}


@pytest.fixture(scope="module")
def windows():
    return torch.from_numpy(synth_windows(64, 192, seed=401)).cuda()


def scorers(models, rows):
    assert models["vib"]._native.vib and models["bf"]._native.enc_widths[1] > 64
    return {"ae": OnlineScorer(models["ae"], models["fit"], thresholds=THR, rows=rows, groups=GROUPS),
            "bf": OnlineScorer(models["bf"], thresholds={"base": 0.5, "sap": 0.5}, rows=rows),
            "vib": OnlineScorer(models["vib"], rows=rows)}


def keep(res):
    return {k: v.clone() for k, v in res.items() if v is not None}


def poison(sc):
    """Canaries into a scorer's outputs, so that equality shows the next call wrote them."""
    sc.out.fill_(-7.0)
    sc.flags.fill_(9)
    if sc.groups is not None:
        sc.group_out.fill_(-7.0)
        sc.group_flags.fill_(9)


def compare(bank, x):
    """bank.score(x) against every member's own score on its columns."""
    want = {}
    for name, sc in bank.scorers.items():
        c0, c1 = bank.columns[name]
        want[name] = keep(sc.score(x[:, c0:c1]))
        poison(sc)
    got = bank.score(x)
    torch.cuda.synchronize()
    assert set(got) == set(bank.scorers)
    for name in got:
        g = keep(got[name])
        assert set(g) == set(want[name]) and set(g) <= set(KEYS), name
        for k in g:
            assert torch.equal(g[k], want[name][k]), (name, k)
    if "ae" in got:
        assert {"groups", "group_flags", "nap"} <= set(got["ae"]) and got["bf"]["nap"] is None
    return got


@pytest.mark.parametrize("rows,Bs", [(16, (1, 10, 16)), (64, (17, 64))])
def test_bank_equals_its_scorers(models, windows, rows, Bs):
    scs = scorers(models, rows)
    bank = SensorBank(scs, COLS)
    assert bank.x.shape == (rows, 192) and bank.columns == {"ae": (0, 192), "bf": (128, 192), "vib": (64, 192)}
    for B in Bs:
        n0 = bank.graph_count()
        compare(bank, windows[:B])
        assert bank.graph_count() == n0 + 1                  # one capture per B
        # replays: new rows in the same buffers, no new capture
        compare(bank, windows[64 - B:])
        compare(bank, windows[:B].flip(0))
        assert bank.graph_count() == n0 + 1
    # bank and single calls take turns on the scorers' states
    sc = scs["ae"]
    a = keep(sc.score(windows[:Bs[0]]))
    b = keep(bank.score(windows[:Bs[0]])["ae"])
    assert all(torch.equal(a[k], b[k]) for k in a)
    bank.close()


def chain(widths, vib, seed):
    """An fp32 autoencoder whose encoder runs through ``widths`` (the decoder back again)."""
    from icra2021_multimodal_ad_amd.auto_encoder import AutoEncoder
    from icra2021_multimodal_ad_amd.fc_module import FCModule, Loss
    torch.manual_seed(seed)
    d, btl, hidden = widths[0], widths[-1], list(widths[1:-1])
    fc = dict(use_batch_norm=True, act="leakyrelu", last_act=None)
    m = AutoEncoder(encoder=FCModule(input_size=d, output_size=2 * btl if vib else btl, hidden_sizes=hidden, **fc),
                    decoder=FCModule(input_size=btl, output_size=d, hidden_sizes=hidden[::-1], **fc),
                    recon_loss=Loss("mse", reduction="sum"), vib=vib).cuda(0)
    m.eval()
    return m


def buffers(sc):
    """A scorer's whole output buffers (the canaries a call leaves included)."""
    bufs = {"out": sc.out, "flags": sc.flags}
    if sc.groups is not None:
        bufs.update(group_out=sc.group_out, group_flags=sc.group_flags)
    return {k: v.clone() for k, v in bufs.items()}


@pytest.mark.parametrize("rows,B", [(16, 3), (64, 17)])
@pytest.mark.parametrize("widths", [((128, 64), (128, 64, 32), (128, 64, 32, 16)),
                                    ((128, 16), (128, 32, 64), (128, 16, 64, 32))], ids=["halving", "mixed"])
def test_members_run_out_of_steps_at_different_points(windows, widths, rows, B):
    """Three fp32 members of 1, 2 and 3 encoder layers on one 128-column row:
    pass 1 has 2 / 4 / 6 steps and pass 2 has 1 / 2 / 3, so every step from the
    third on is absent for a neighbour, and the VIB launch of the middle member
    lands between two grouped steps.  The shallow member has two groups, the
    deep one an fp32 NAP fit.  Eagerly, on the capturing call and replayed,
    every member's out, flags, group_out and group_flags are, bit for bit,
    what its own scorer's ``score`` leaves there."""
    one, two, three = (chain(w, vib=i == 1, seed=40 + i) for i, w in enumerate(widths))
    scs = {"one": OnlineScorer(one, rows=rows, groups=[(0, 64), (64, 128)],
                               thresholds={"base": 0.05, "sap": 0.05, "groups": {0: 0.05, 1: -1.0}}),
           "two": OnlineScorer(two, rows=rows),
           "three": OnlineScorer(three, _fit(three, (0, 4)), rows=rows,
                                 thresholds={"base": 0.05, "sap": 0.05, "nap": 1.0})}
    assert [sc.nat.n_enc for sc in scs.values()] == [1, 2, 3] and scs["two"].nat.vib
    assert scs["one"].groups == [0, 64, 128] and scs["three"].nap is not None
    bank = SensorBank(scs)                                   # every member reads columns 0..128
    assert bank.x.shape == (rows, 128)
    x = windows[:B, :128]
    want = {}
    for name, sc in scs.items():
        poison(sc)
        sc.score(x)
        want[name] = buffers(sc)
    for graph in (False, True, True):                        # eager, the capturing call, a replay
        for sc in scs.values():
            poison(sc)
        bank.x[:B].copy_(x)
        bank._run(B, graph=graph)
        torch.cuda.synchronize()
        for name, sc in scs.items():
            got = buffers(sc)
            assert set(got) == set(want[name])
            for k in got:
                assert torch.equal(got[k], want[name][k]), (name, k, graph)
    assert bank.graph_count() == 1
    bank.close()


def launches(nat, groups=False):
    """The single pass's launch list: pack, fold, one per layer, one per
    encoder layer again, (VIB, group_sq, NAP), finish."""
    return 2 + len(nat.layers) + nat.n_enc + 1 + int(bool(nat.vib)) + int(groups)


def test_graph_shape(models, windows, golden):
    """Three same-depth, same-dtype, fit-less, non-VIB members: the node count
    of ONE such member's pass.  The mixed bank: at most the deepest member's,
    plus one per step that holds both element types, plus the per-member VIB /
    group launches (and the NAP launch of the member with a fit)."""
    x = windows[:10]
    trio = [small(192, 16, 5, "f32", "ae", s) for s in (31, 32, 33)]
    one = SensorBank([OnlineScorer(trio[0])])
    one.score(x)
    n_one = one.graph_nodes()
    assert n_one == launches(trio[0]._native) == 18
    bank = SensorBank([OnlineScorer(m) for m in trio])
    compare(bank, x)
    assert bank.graph_nodes() == n_one
    scs = scorers(models, 16)
    mixed = SensorBank(scs, COLS)
    compare(mixed, x)
    deepest = launches(models["ae"]._native)                 # pack, fold, 10 + 5 layer steps, finish
    bf_steps = len(models["bf"]._native.layers) + models["bf"]._native.n_enc   # steps that also hold bf16
    extra = 1 + 1 + 1                                        # VIB (vib), group_sq (ae), NAP (ae)
    print(f"graph nodes: one {n_one}, trio {bank.graph_nodes()}, mixed {mixed.graph_nodes()} "
          f"(bound {deepest + bf_steps + extra})")
    assert deepest <= mixed.graph_nodes() <= deepest + bf_steps + extra
    for b in (one, bank, mixed):
        b.close()


def test_refusals(models, windows, golden):
    lib = _native.load()
    scs = scorers(models, 16)
    # mixed rows: refused before anything native exists
    with pytest.raises(ValueError, match="mixed rows"):
        SensorBank({"ae": scs["ae"], "bf": OnlineScorer(models["bf"], rows=64)}, COLS)
    with pytest.raises(ValueError, match="9 scorers"):
        SensorBank([scs["bf"]] * 9)
    # misaligned col0: 130 is no multiple of 4 (the grouped pack reads 16-byte quads)
    bad = SensorBank({"ae": scs["ae"], "bf": scs["bf"]}, {"ae": 0, "bf": 130}, width=196)
    for sc in scs.values():
        poison(sc)
    with pytest.raises(_native.NativeError, match="16-byte aligned"):
        bad.score(torch.zeros(10, 196))
    assert bad.graph_count() == 0
    # col0 + D > ld_x: the native entry on a row narrower than the member's columns
    bank = SensorBank(scs, COLS)
    narrow = torch.zeros(16, 188, device="cuda")
    rc = lib.mmad_online_bank_score(bank._h, narrow.data_ptr(), narrow.stride(0), 10, bank._members, 1,
                                    _native.stream_ptr())
    assert rc == -1 and "ld_x=188" in _native.last_error()
    # B outside 1..rows, a state one byte short: the members' own refusals
    rc = lib.mmad_online_bank_score(bank._h, bank.x.data_ptr(), bank.x.stride(0), 17, bank._members, 1,
                                    _native.stream_ptr())
    assert rc == -1 and "B=17 outside 1..16" in _native.last_error()
    bank._members[2].state_bytes -= 512
    with pytest.raises(_native.NativeError, match="online state null or too small"):
        bank.score(windows[:10])
    bank._members[2].state_bytes += 512
    # a member with score planes attached (split-bf16 is not supported on the online path)
    x3 = _model(golden, score_dtype="bf16x3")
    assert x3._native.score_dtype == 2
    planes = SensorBank({"bf": scs["bf"], "x3": OnlineScorer(x3)}, {"bf": 128, "x3": 0})
    with pytest.raises(_native.NativeError, match="score planes attached"):
        planes.score(windows[:10])
    torch.cuda.synchronize()
    assert bank.graph_count() == 0 and planes.graph_count() == 0
    for sc in scs.values():
        assert (sc.out == -7.0).all() and (sc.flags == 9).all()
    compare(bank, windows[:10])                              # and the bank is fine afterwards
    for b in (bad, bank, planes):
        b.close()
