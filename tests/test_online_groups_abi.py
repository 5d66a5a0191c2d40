"""CPU-side checks of the per-modality scoring surface (no GPU): the new C-ABI
symbols and their ctypes signatures, MMAD_MAX_GROUPS, the groups buffer size
query, the host-side refusals of mmad_group_sq and mmad_ae_online_score_groups
(checked before any launch), HSR_Net.modality_columns and OnlineScorer's
attribute set with and without groups."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.conftest import REPO

NEW = ("mmad_group_sq", "mmad_ae_online_groups_bytes", "mmad_ae_online_score_groups")
WIDTHS = [192, 156, 121, 86, 51, 16]            # the mm192 golden's encoder
UNGROUPED_ATTRS = {"rows", "model", "nat", "nap", "start", "end", "x", "out", "flags", "thresholds", "state"}


@pytest.fixture(scope="module")
def lib():
    from icra2021_multimodal_ad_amd import _native
    return _native.load()


def _nat(dtype="f32"):
    from icra2021_multimodal_ad_amd.engine import NativeAE
    return NativeAE(WIDTHS, WIDTHS[::-1], dtype=dtype, device="cpu")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mmad.h")).read(), flags=re.S)


def test_new_symbols_exported_with_the_headers_argument_count(lib):
    from icra2021_multimodal_ad_amd._native import SIGNATURES
    src = _header()
    for name, n_args in zip(NEW, (11, 2, 21)):
        m = re.search(r"\b%s\s*\(([^;]*?)\);" % name, src, re.S)
        assert m, name
        assert hasattr(lib, name), name
        assert name in SIGNATURES
        assert len(SIGNATURES[name][1]) == m.group(1).count(",") + 1 == n_args, name
    assert SIGNATURES["mmad_ae_online_groups_bytes"][0] is ctypes.c_int64


def test_max_groups_constant():
    from icra2021_multimodal_ad_amd import _native
    m = re.search(r"#define\s+MMAD_MAX_GROUPS\s+(\d+)", _header())
    assert m and int(m.group(1)) == _native.MAX_GROUPS == 8


def test_online_groups_bytes(lib):
    nat = _nat()
    # [rows][Kp0] fp32, Kp0 = 192 padded to 256
    assert lib.mmad_ae_online_groups_bytes(nat._h, 16) == 16 * 256 * 4
    assert lib.mmad_ae_online_groups_bytes(nat._h, 64) == 64 * 256 * 4
    assert lib.mmad_ae_online_groups_bytes(_nat("bf16")._h, 16) == 16 * 256 * 4      # d0 is fp32
    assert lib.mmad_ae_online_groups_bytes(nat._h, 32) == -1
    assert lib.mmad_ae_online_groups_bytes(None, 16) == -1


def _bounds(*b):
    return (ctypes.c_int * len(b))(*b)


def test_group_sq_refusals_on_the_host(lib):
    err = lib.mmad_last_error_string
    d = np.zeros((4, 64), np.float32)
    out = np.zeros((8, 4), np.float32)
    pd, po = ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(out.ctypes.data)

    def run(b, N=4, ldd=64, d=pd, o=po, ldo=4):
        return lib.mmad_group_sq(N, d, ldd, _bounds(*b), len(b) - 1, None, o, ldo, None, 0, None)

    assert run([0]) == -1 and b"G=0 outside 1..8" in err()
    assert run(list(range(10))) == -1 and b"G=9 outside 1..8" in err()
    assert run([0, 32, 16, 64]) == -1 and b"bounds not strictly ascending" in err()
    assert run([0, 32, 32, 64]) == -1 and b"bounds not strictly ascending" in err()
    assert run([-1, 32]) == -1 and b"bounds[0]" in err()
    assert run([0, 65]) == -1 and b"exceeds ldd" in err()
    assert run([0, 64], N=0) == -1 and b"N=0" in err()
    assert run([0, 64], d=None) == -1 and b"d null" in err()
    assert run([0, 64], o=None) == -1 and b"null out" in err()
    assert run([0, 64], ldo=3) == -1 and b"ld_out" in err()
    assert lib.mmad_group_sq(4, pd, 64, None, 1, None, po, 4, None, 0, None) == -1 and b"null bounds" in err()
    assert not out.any()


def test_online_score_groups_refusals_on_the_host(lib):
    nat = _nat()
    h, err = nat._h, lib.mmad_last_error_string
    need, gneed = lib.mmad_ae_online_state_bytes(h), lib.mmad_ae_online_groups_bytes(h, 16)
    buf, gbuf = np.zeros(need + 256, np.uint8), np.zeros(gneed + 512, np.uint8)
    state = ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)
    g0 = (gbuf.ctypes.data + 255) // 256 * 256
    gstate = ctypes.c_void_p(g0)
    x = np.zeros((17, 192), np.float32)
    out, gout = np.zeros((9, 16), np.float32), np.zeros((4, 16), np.float32)
    px, po, pg = (ctypes.c_void_p(a.ctypes.data) for a in (x, out, gout))
    good = [0, 101, 107, 171, 192]

    def run(b=good, B=10, rows=16, go=pg, gs=gstate, gb=gneed, hh=h):
        return lib.mmad_ae_online_score_groups(hh, px, 192, B, 0, 7, None, po, None, state, need, 0, None, rows,
                                               _bounds(*b), len(b) - 1, None, go, None, gs, gb)

    assert run(rows=32) == -1 and b"rows=32" in err()
    assert run(b=[0]) == -1 and b"G=0 outside 1..8" in err()
    assert run(b=list(range(10))) == -1 and b"G=9 outside 1..8" in err()
    assert run(b=[0, 101, 101, 192]) == -1 and b"bounds not strictly ascending" in err()
    assert run(b=[0, 101, 50, 192]) == -1 and b"bounds not strictly ascending" in err()
    assert run(b=[0, 101, 193]) == -1 and b"bounds[G]=193 exceeds the input width D=192" in err()
    assert run(go=None) == -1 and b"null group_out" in err()
    assert run(gs=None) == -1 and b"gstate null or too small" in err()
    assert run(gb=gneed - 1) == -1 and b"gstate null or too small" in err()
    assert run(gs=ctypes.c_void_p(g0 + 16)) == -1 and b"gstate must be 256-byte aligned" in err()
    assert run(hh=None) == -1 and b"null handle" in err()
    # the ungrouped entry point's refusals
    assert run(B=0) == -1 and b"outside 1..16" in err()
    assert run(B=17) == -1 and b"outside 1..16" in err()
    assert run(B=40, rows=64) == -1 and b"gstate null or too small" in err()   # 16-row buffers under rows = 64
    # a well-formed call on a handle that was never bound to device buffers
    assert run() == -1 and b"unbound" in err()
    assert not out.any() and not gout.any()


def test_modality_columns():
    from icra2021_multimodal_ad_amd import hsr_net
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    table = {"r": (0, 1024), "d": (1024, 1536), "t": (1536, 1600), "m": (1600, 1728)}
    fused = HSR_Net(False, types.SimpleNamespace(slicing_size=4, sensor="All")).modality_columns()
    assert fused == table and list(fused) == ["r", "d", "t", "m"]
    assert HSR_Net(False, types.SimpleNamespace(slicing_size=4)).modality_columns() == table
    assert hsr_net.FUSED_WIDTH == 1728
    for sensor, key, channels in (("hand_camera", "r", 16), ("head_depth", "d", 8), ("force_torque", "t", 1),
                                  ("mic", "m", 2)):
        cols = HSR_Net(True, types.SimpleNamespace(slicing_size=4, sensor=sensor)).modality_columns()
        assert cols == {key: (0, 64 * channels)}, sensor
        assert hsr_net._BLOCK[key] == channels
    with pytest.raises(ValueError, match="sensor"):
        HSR_Net(True, types.SimpleNamespace(slicing_size=4)).modality_columns()


def _cpu_model():
    from icra2021_multimodal_ad_amd.model_builder import get_model
    return get_model(types.SimpleNamespace(input_size=192, btl_size=16, n_layers=5, gpu_id=-1, dtype="f32",
                                           models="ae"))


def test_online_scorer_attributes_with_and_without_groups():
    from icra2021_multimodal_ad_amd.online import OnlineScorer, group_bounds
    m = _cpu_model()
    plain = OnlineScorer(m)
    assert set(vars(plain)) == UNGROUPED_ATTRS
    assert plain.groups is None and plain.group_names == ()
    with pytest.raises(ValueError, match="without groups"):
        plain.set_thresholds({"groups": {"a": 1.0}})
    sc = OnlineScorer(m, rows=64, groups={"late": (100, 192), "early": (0, 100)},
                      thresholds={"base": 1.0, "groups": {"late": 2.5}})
    assert set(vars(sc)) == UNGROUPED_ATTRS | {"groups", "group_names", "group_out", "group_flags",
                                               "group_thresholds", "groups_state"}
    assert sc.group_names == ("early", "late") and sc.groups == [0, 100, 192]
    assert sc.group_out.shape == (2, 64) and sc.group_flags.shape == (2, 64)
    assert sc.group_flags.dtype == torch.uint8
    thr = sc.group_thresholds.numpy()
    assert np.isnan(thr[0]) and thr[1] == 2.5
    sc.set_thresholds({"base": 2.0})                                  # no 'groups' entry: left as they are
    assert sc.group_thresholds.numpy()[1] == 2.5
    # a list of pairs is named by position; the contract is contiguous groups
    assert group_bounds([(64, 128), (0, 64)], 192) == ((1, 0), [0, 64, 128])
    with pytest.raises(ValueError, match="contiguous"):
        group_bounds({"a": (0, 64), "b": (70, 128)}, 192)
    with pytest.raises(ValueError, match="contiguous"):
        group_bounds({"a": (0, 64), "b": (60, 128)}, 192)
    with pytest.raises(ValueError, match="outside"):
        group_bounds({"a": (0, 193)}, 192)
    with pytest.raises(ValueError, match="empty"):
        group_bounds({"a": (5, 5)}, 192)
    with pytest.raises(ValueError, match="groups"):
        group_bounds([(i, i + 1) for i in range(9)], 192)
