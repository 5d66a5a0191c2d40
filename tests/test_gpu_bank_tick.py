"""The bank's sensor tick on the GPU (SensorBank.bind_sensors / tick,
mmad_online_bank_tick): the fused member against OnlineScorer.tick, every
unimodal member against its own scorer on its columns of the fused row, a
mic-only bank, and refresh_sensors without a new capture -- all bit for bit.

The queues, the fused HSR_Net (seed 7) and the PCM cases are those of
tests/test_gpu_tick.py; the models are 1728 / 1024 / 512 / 64 / 128 wide,
3 layers at btl 16."""
import types

import pytest
import torch

from icra2021_multimodal_ad_amd.online import OnlineScorer, SensorBank
from tests.test_gpu_tick import keep, make_net, pcm, queues, same   # noqa: F401  (pcm: a fixture)

pytestmark = pytest.mark.gpu

WIDTHS = {"All": 1728, "hand_camera": 1024, "head_depth": 512, "force_torque": 64, "mic": 128}


@pytest.fixture(scope="module")
def models():
    from icra2021_multimodal_ad_amd.model_builder import get_model
    out = {}
    for i, (name, d) in enumerate(WIDTHS.items()):
        torch.manual_seed(8 + i)
        out[name] = get_model(types.SimpleNamespace(input_size=d, btl_size=16, n_layers=3, gpu_id=0, dtype="f32",
                                                    models="ae"))
        out[name].eval()
    return out


def bank_of(models, net, rows, names=tuple(WIDTHS)):
    scs = {n: OnlineScorer(models[n], rows=rows, groups=net.modality_columns() if n == "All" else None)
           for n in names}
    return SensorBank.for_sensors(net, scs)


@pytest.mark.parametrize("B,rows", [(10, 16), (17, 64)])
def test_tick_equals_the_members_own_calls(models, pcm, B, rows):
    net, y = make_net(B), pcm(B)
    q = queues(B, 81, y)
    bank = bank_of(models, net, rows).bind_sensors(net, len(y))
    cols = net.modality_columns()
    assert bank.x.shape == (rows, 1728)
    assert bank.columns == {"All": (0, 1728), "hand_camera": cols["r"], "head_depth": cols["d"],
                            "force_torque": cols["t"], "mic": cols["m"]}
    got = {n: keep(r) for n, r in bank.tick(*q).items()}
    # the fused member: OnlineScorer.tick on the same queues
    ref = OnlineScorer(models["All"], rows=rows, groups=cols).bind_sensors(net, len(y))
    same(got["All"], keep(ref.tick(*q)))
    assert torch.equal(bank.x[:B], ref.x[:B])
    # the unimodal members: their scorer's own score on their columns of the row score_sensors forms
    former = OnlineScorer(models["All"], rows=rows)
    former.score_sensors(net, *q)
    row = former.x[:B].clone()
    assert torch.equal(row, bank.x[:B])
    for name in list(WIDTHS)[1:]:
        c0, c1 = bank.columns[name]
        assert c1 - c0 == WIDTHS[name]
        alone = OnlineScorer(models[name], rows=rows)
        same(got[name], keep(alone.score(row[:, c0:c1])))
    # a replay with other queues, and the bank's other routes on the same queues
    q2 = queues(B, 82, y, roll=1000)
    n0 = bank.graph_count()
    got2 = {n: keep(r) for n, r in bank.tick(*q2).items()}
    assert bank.graph_count() == n0 == 1
    same(got2["All"], keep(ref.tick(*q2)))
    assert not torch.equal(got2["mic"]["base"], got["mic"]["base"])
    via_sensors = {n: keep(r) for n, r in bank.score_sensors(net, *q2).items()}
    for n in WIDTHS:
        same(via_sensors[n], got2[n])
    bank.close()


def test_mic_only_bank(models, pcm):
    """No fused member at all: the unimodal tick."""
    B = 10
    net, y = make_net(B), pcm(B)
    q = queues(B, 83, y)
    bank = bank_of(models, net, 16, names=("mic",)).bind_sensors(net, len(y))
    assert bank.x.shape == (16, 1728) and bank.columns == {"mic": (1600, 1728)}
    got = keep(bank.tick(*q)["mic"])
    former = OnlineScorer(models["All"])
    former.score_sensors(net, *q)
    same(got, keep(OnlineScorer(models["mic"]).score(former.x[:B, 1600:1728])))
    assert torch.isfinite(got["base"]).all() and (got["base"] > 0).all()
    bank.close()


def test_refresh_sensors_needs_no_capture(models, pcm):
    B = 10
    net, y = make_net(B), pcm(B)
    q = queues(B, 81, y)
    bank = bank_of(models, net, 16, names=("All", "hand_camera", "mic")).bind_sensors(net, len(y))
    with pytest.raises(ValueError, match="bind_sensors"):
        bank_of(models, net, 16, names=("mic",)).tick(*q)
    a = {n: keep(r) for n, r in bank.tick(*q).items()}
    n0 = bank.graph_count()
    assert n0 == 1
    with torch.no_grad():
        net.conv1r.bias.add_(0.25)
    stale = {n: keep(r) for n, r in bank.tick(*q).items()}
    for n in a:
        same(stale[n], a[n])                               # the graph reads the packed copy
    bank.refresh_sensors()
    b = {n: keep(r) for n, r in bank.tick(*q).items()}
    assert bank.graph_count() == n0
    assert not torch.equal(b["All"]["base"], a["All"]["base"])
    assert not torch.equal(b["hand_camera"]["base"], a["hand_camera"]["base"])
    same(b["mic"], a["mic"])                               # conv1r feeds the camera block only
    ref = OnlineScorer(models["All"], groups=net.modality_columns()).bind_sensors(net, len(y))
    same(b["All"], keep(ref.tick(*q)))
    bank.close()
