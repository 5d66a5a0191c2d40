"""CPU-side checks of the online scoring surface (no GPU): the new C-ABI
symbols and their ctypes signatures, the state size query, the host-side
refusals of mmad_ae_online_score (checked before any launch) and
OnlineScorer's row limit."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.conftest import REPO

NEW = ("mmad_fc_rows16", "mmad_ae_online_state_bytes", "mmad_ae_online_score")
WIDTHS = [192, 156, 121, 86, 51, 16]            # the mm192 golden's encoder


@pytest.fixture(scope="module")
def lib():
    from icra2021_multimodal_ad_amd import _native
    return _native.load()


def _nat(dtype="f32"):
    from icra2021_multimodal_ad_amd.engine import NativeAE
    return NativeAE(WIDTHS, WIDTHS[::-1], dtype=dtype, device="cpu")


def test_new_symbols_exported_with_the_headers_argument_count(lib):
    from icra2021_multimodal_ad_amd._native import SIGNATURES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mmad.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\);" % name, src, re.S)
        assert m, name
        assert hasattr(lib, name), name
        assert name in SIGNATURES
        assert len(SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert SIGNATURES["mmad_ae_online_state_bytes"][0] is ctypes.c_int64


def test_online_state_bytes(lib):
    nat = _nat()
    n0 = lib.mmad_ae_online_state_bytes(nat._h)
    assert n0 > 0
    assert lib.mmad_ae_online_state_bytes(None) == -1
    # at least the packed input and every layer's 16-row output
    floor = 16 * 4 * (256 + sum(256 if w > 128 else 128 for w in WIDTHS[1:] + WIDTHS[::-1][1:]))
    assert n0 >= floor
    assert lib.mmad_ae_online_state_bytes(_nat("bf16")._h) < n0
    # a fit's dimensions attached: an MMAD_F32 attachment stores the pointers
    # and launches nothing, so host buffers stand in (never dereferenced here)
    W, R = sum(WIDTHS), 300
    Kp, Rp = 640, 384
    vt, bias, w = np.zeros((Rp, Kp), np.float32), np.zeros(Rp, np.float32), np.zeros(Rp, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.mmad_ae_set_nap(nat._h, 0, 6, R, p(vt), p(bias), p(w), 0, None, None) == 0
    n1 = lib.mmad_ae_online_state_bytes(nat._h)
    assert n1 >= n0 + 16 * Kp * 4 + Rp * 4
    assert lib.mmad_ae_set_nap(nat._h, 0, 0, 0, None, None, None, 0, None, None) == 0
    assert lib.mmad_ae_online_state_bytes(nat._h) == n0
    assert W == 622


def test_online_score_refusals_on_the_host(lib):
    nat = _nat()
    h, err = nat._h, lib.mmad_last_error_string
    need = lib.mmad_ae_online_state_bytes(h)
    buf = np.zeros(need + 256, np.uint8)
    state = ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)
    x = np.zeros((17, 192), np.float32)
    out = np.zeros((9, 16), np.float32)
    px, po = ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(out.ctypes.data)

    def run(B, st, nb):
        return lib.mmad_ae_online_score(h, px, 192, B, 0, 7, None, po, None, st, nb, 0, None)

    assert run(0, state, need) == -1 and b"outside 1..16" in err()
    assert run(17, state, need) == -1 and b"outside 1..16" in err()
    assert run(10, None, need) == -1 and b"state" in err()
    assert run(10, state, need - 1) == -1 and b"too small" in err()
    assert lib.mmad_ae_online_score(None, px, 192, 10, 0, 7, None, po, None, state, need, 0, None) == -1
    assert b"null handle" in err()
    # a well-formed call on a handle that was never bound to device buffers
    assert run(10, state, need) == -1 and b"unbound" in err()
    assert not out.any()


def test_fc_rows16_refusals_on_the_host(lib):
    a = np.zeros(16 * 128, np.float32)
    p = ctypes.c_void_p((a.ctypes.data + 15) // 16 * 16)
    run = lambda M, N, Np, Kp: lib.mmad_fc_rows16(0, M, N, 1, Np, Kp, p, p, None, 0, 0.2, None, None, p,
                                                  None, 0, 0, None, 0, None, None, None)
    assert run(0, 1, 128, 128) == -1 and b"outside 1..16" in lib.mmad_last_error_string()
    assert run(17, 1, 128, 128) == -1
    assert run(1, 1, 120, 128) == -1 and b"bad sizes" in lib.mmad_last_error_string()
    assert run(1, 1, 128, 64) == -1


def test_online_scorer_refuses_17_rows():
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    cfg = types.SimpleNamespace(input_size=192, btl_size=16, n_layers=5, gpu_id=-1, dtype="f32", models="ae")
    sc = OnlineScorer(get_model(cfg))
    with pytest.raises(ValueError, match="score_windows"):
        sc.score(torch.zeros(17, 192))
    with pytest.raises(ValueError):
        sc.score(torch.zeros(4, 191))
