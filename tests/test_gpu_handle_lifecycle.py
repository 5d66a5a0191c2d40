"""The executor handle through its whole life: eager and graph-replayed train
steps and a graph-replayed score pass, a rebind onto fresh buffers (the model
moved to the CPU and back), the same calls again, then destruction."""
import gc
import types

import numpy as np
import pytest
import torch

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd.common_utils import init_state_dict
from icra2021_multimodal_ad_amd.data import synth_windows

pytestmark = pytest.mark.gpu

D, BTL, NL, B = 256, 16, 3, 128


def _model(sd, graph):
    from icra2021_multimodal_ad_amd.model_builder import get_model
    cfg = types.SimpleNamespace(input_size=D, btl_size=BTL, n_layers=NL, gpu_id=0, dtype="bf16")
    with _native.tune(train_graph=graph):
        m = get_model(cfg)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return m


def _calls(m, x):
    """Two train steps and one graph-replayed score pass; (losses, scores)."""
    nat = m._native
    losses = [float(nat.train_step_fused(x)) for _ in range(2)]
    out = torch.full((nat.n_enc + 1, B), float("nan"), device="cuda")
    nat.score_stream(x, 64, out, graph=True)
    return losses, out


def _state(m):
    nat = m._native
    return (nat.params.clone(), nat.exp_avg.clone(), nat.exp_avg_sq.clone(), nat.running.clone(),
            nat.shadow.clone())


@pytest.mark.parametrize("graph", [False, True])
def test_rebind_after_captured_paths_then_destroy(graph):
    """bf16, D = 256, bottleneck 16, 3 layers, 128 rows.  Two train steps (eager,
    or replayed from the captured step under train_graph) and a graph-replayed
    score pass; the model to the CPU and back (fresh buffers, mmad_ae_bind
    again): no captured train step survives the rebind (the eager case holds
    none to begin with; only the graph case exercises the clear).  The two
    cases run on a handle each, not one after the other.  The same calls again
    leave parameters, Adam moments, running statistics, shadow, losses and
    scores equal, bit for bit, to those of a fresh model loaded with the rebound
    model's state and run through the same calls.  Deleting every model and
    synchronising leaves the device without an error."""
    x = torch.from_numpy(synth_windows(B, D, seed=32)).cuda()
    m = _model(init_state_dict(D, BTL, NL, seed=31), graph)
    nat = m._native
    assert nat.use_graph == graph
    _calls(m, x)
    assert nat._lib.mmad_ae_train_graph_count(nat._h) == (1 if graph else 0)
    assert nat._lib.mmad_ae_graph_count(nat._h) == 1
    m.cpu()
    m.cuda()
    assert nat._lib.mmad_ae_train_graph_count(nat._h) == 0

    fresh = _model({k: v.cpu().numpy() for k, v in m.state_dict().items()}, graph)
    fnat = fresh._native
    fnat.exp_avg.copy_(nat.exp_avg)
    fnat.exp_avg_sq.copy_(nat.exp_avg_sq)
    fnat.adam_step_count = nat.adam_step_count
    for a, b in zip(_state(m)[:4], _state(fresh)[:4]):
        assert torch.equal(a, b)

    la, sa = _calls(m, x)
    lb, sb = _calls(fresh, x)
    assert nat._lib.mmad_ae_train_graph_count(nat._h) == (1 if graph else 0)
    assert la == lb and all(np.isfinite(la))
    assert torch.equal(sa, sb) and bool(torch.isfinite(sa).all())
    for a, b in zip(_state(m), _state(fresh)):
        assert torch.equal(a, b)

    del m, nat, fresh, fnat
    gc.collect()
    torch.cuda.synchronize()
    assert float(torch.ones(4, device="cuda").sum()) == 4.0
