"""CPU-side checks of the 64-row online scoring surface (no GPU): the three new
C-ABI symbols and their ctypes signatures, the 64-row state size query, the
host-side refusals of mmad_ae_online_score64 / mmad_fc_rows64 (checked before
any launch) and OnlineScorer's ``rows`` argument.  Modelled on
tests/test_online_abi.py, same encoder widths."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.conftest import REPO

NEW = ("mmad_fc_rows64", "mmad_ae_online_state_bytes64", "mmad_ae_online_score64")
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
    assert SIGNATURES["mmad_ae_online_state_bytes64"][0] is ctypes.c_int64
    assert SIGNATURES["mmad_fc_rows64"] == SIGNATURES["mmad_fc_rows16"]
    assert SIGNATURES["mmad_ae_online_score64"] == SIGNATURES["mmad_ae_online_score"]
    assert lib.mmad_abi_version() == 1


def test_online_state_bytes64(lib):
    nat = _nat()
    n16 = lib.mmad_ae_online_state_bytes(nat._h)
    n0 = lib.mmad_ae_online_state_bytes64(nat._h)
    assert lib.mmad_ae_online_state_bytes64(None) == -1
    # at least the packed input and every layer's 64-row output
    floor = 64 * 4 * (256 + sum(256 if w > 128 else 128 for w in WIDTHS[1:] + WIDTHS[::-1][1:]))
    assert n0 >= floor
    assert n0 > n16 > 0
    assert lib.mmad_ae_online_state_bytes64(_nat("bf16")._h) < n0
    # a fit's dimensions attached (host buffers stand in: an MMAD_F32
    # attachment stores the pointers and launches nothing)
    R, Kp, Rp = 300, 640, 384
    vt, bias, w = np.zeros((Rp, Kp), np.float32), np.zeros(Rp, np.float32), np.zeros(Rp, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.mmad_ae_set_nap(nat._h, 0, 6, R, p(vt), p(bias), p(w), 0, None, None) == 0
    n1 = lib.mmad_ae_online_state_bytes64(nat._h)
    assert n1 >= n0 + 64 * Kp * 4 + Rp * 4
    assert lib.mmad_ae_set_nap(nat._h, 0, 0, 0, None, None, None, 0, None, None) == 0
    assert lib.mmad_ae_online_state_bytes64(nat._h) == n0
    assert lib.mmad_ae_online_state_bytes(nat._h) == n16            # the 16-row query: as before


def test_online_score64_refusals_on_the_host(lib):
    nat = _nat()
    h, err = nat._h, lib.mmad_last_error_string
    need = lib.mmad_ae_online_state_bytes64(h)
    buf = np.zeros(need + 256, np.uint8)
    state = ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)
    x = np.zeros((65, 192), np.float32)
    out = np.zeros((9, 64), np.float32)
    px, po = ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(out.ctypes.data)

    def run(B, st, nb):
        return lib.mmad_ae_online_score64(h, px, 192, B, 0, 7, None, po, None, st, nb, 0, None)

    assert run(0, state, need) == -1 and b"outside 1..64" in err()
    assert run(65, state, need) == -1 and b"outside 1..64" in err()
    assert run(40, None, need) == -1 and b"state" in err()
    assert run(40, state, need - 1) == -1 and b"too small" in err()
    # a state sized by the 16-row query is too small for the 64-row pass
    assert run(40, state, lib.mmad_ae_online_state_bytes(h)) == -1 and b"too small" in err()
    assert lib.mmad_ae_online_score64(None, px, 192, 40, 0, 7, None, po, None, state, need, 0, None) == -1
    assert b"null handle" in err()
    # a well-formed call on a handle that was never bound to device buffers
    assert run(40, state, need) == -1 and b"unbound" in err()
    assert not out.any()


def test_fc_rows64_refusals_on_the_host(lib):
    a = np.zeros(64 * 128, np.float32)
    p = ctypes.c_void_p((a.ctypes.data + 15) // 16 * 16)
    err = lib.mmad_last_error_string

    def run(M, N, Np, Kp, act=0, rowsq=None, diff=None):
        return lib.mmad_fc_rows64(0, M, N, 1, Np, Kp, p, p, None, act, 0.2, None, None, p,
                                  None, 0, 0, diff, 128, None, rowsq, None)

    assert run(0, 1, 128, 128) == -1 and b"outside 1..64" in err()
    assert run(65, 1, 128, 128) == -1 and b"outside 1..64" in err()
    assert run(1, 1, 120, 128) == -1 and b"bad sizes" in err()
    assert run(1, 1, 128, 64) == -1
    assert run(1, 1, 128, 128, diff=p) == -1 and b"need rowsq" in err()
    assert run(1, 1, 128, 128, act=99) == -2 and b"per-element epilogue" in err()
    # misaligned and null operands
    q = ctypes.c_void_p(p.value + 4)
    assert lib.mmad_fc_rows64(0, 1, 1, 1, 128, 128, q, p, None, 0, 0.2, None, None, p, None, 0, 0, None, 0,
                              None, None, None) == -1 and b"16-byte aligned" in err()
    assert lib.mmad_fc_rows64(0, 1, 1, 1, 128, 128, p, None, None, 0, 0.2, None, None, p, None, 0, 0, None, 0,
                              None, None, None) == -1
    assert not a.any()


def test_online_scorer_rows_argument():
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    cfg = types.SimpleNamespace(input_size=192, btl_size=16, n_layers=5, gpu_id=-1, dtype="f32", models="ae")
    model = get_model(cfg)
    sc = OnlineScorer(model, rows=64)
    assert tuple(sc.x.shape) == (64, 192) and tuple(sc.out.shape) == (9, 64) and tuple(sc.flags.shape) == (3, 64)
    assert sc.state.numel() >= model._native._lib.mmad_ae_online_state_bytes64(model._native._h)
    with pytest.raises(ValueError, match="score_windows"):
        sc.score(torch.zeros(65, 192))
    with pytest.raises(ValueError):
        sc.score(torch.zeros(40, 191))
    with pytest.raises(ValueError):
        OnlineScorer(model, rows=48)
    from icra2021_multimodal_ad_amd.online import rows_for
    assert [rows_for(n) for n in (None, 1, 10, 16, 17, 40, 64, 65)] == [16, 16, 16, 16, 64, 64, 64, 16]
    # the default is the 16-row scorer, refusing a 17th window as before
    sc16 = OnlineScorer(model)
    assert sc16.rows == 16 and tuple(sc16.x.shape) == (16, 192)
    with pytest.raises(ValueError, match="score_windows"):
        sc16.score(torch.zeros(17, 192))
