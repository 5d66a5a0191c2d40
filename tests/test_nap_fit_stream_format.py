"""Streaming NAP fit on the CPU: the header / ctypes surface declares the new
entry points, the size queries behave, the host-side refusals refuse, and the
config flag is plumbed through NoveltyDetecter.scores (which needs a GPU to go
any further and says so)."""
import ctypes
import re
import os
import types

import pytest
import torch

from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "mmad.h")
NEW = {"mmad_nap_fit_state_bytes": 1, "mmad_nap_fit_state_layout": 2, "mmad_nap_fit_begin": 4,
       "mmad_nap_fit_accumulate_sums": 7, "mmad_nap_fit_finish_mean": 6, "mmad_nap_fit_accumulate_gram": 8,
       "mmad_nap_fit_solve": 6, "mmad_nap_fit_accumulate_rot": 9, "mmad_nap_fit_finish": 7,
       "mmad_ae_nap_fit_workspace_bytes": 4, "mmad_ae_nap_fit_stream": 16}


def _header_args():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"(?:int64_t|int)\s+(mmad_\w+)\s*\(([^;]*?)\);", src, re.S)}


def _ctype_of(arg):
    if "*" in arg:
        return "P"
    return {"int": "i", "int64_t": "q"}[arg.split()[0]]


def test_header_and_ctypes_declare_the_streaming_fit():
    from icra2021_multimodal_ad_amd import _native
    lib = _native.load()
    args = _header_args()
    code = {ctypes.c_int: "i", ctypes.c_int64: "q", ctypes.c_void_p: "P", ctypes.POINTER(ctypes.c_int64): "P"}
    for fn, nargs in NEW.items():
        assert fn in args and len(args[fn]) == nargs, fn
        assert hasattr(lib, fn), fn
        res, sig = _native.SIGNATURES[fn]
        assert [code[t] for t in sig] == [_ctype_of(a) for a in args[fn]], fn
        assert res is (ctypes.c_int64 if fn.endswith("_bytes") else ctypes.c_int), fn
    assert lib.mmad_abi_version() == 1          # additive: the version rule of mmad.h


def test_state_size_and_layout():
    from icra2021_multimodal_ad_amd import _native
    lib = _native.load()
    info = (ctypes.c_int64 * 3)()
    prev = 0
    for W in (1, 48, 127, 128, 129, 700, 6442):
        b = lib.mmad_nap_fit_state_bytes(W)
        assert b > prev                                         # grows with W
        prev = b
        assert lib.mmad_nap_fit_state_layout(W, info) == 0
        s_off, g_off, total = list(info)
        assert total == b and s_off % 256 == 0 and g_off % 256 == 0
        assert g_off >= s_off + 8 * W and total >= g_off + 2 * 8 * W * W      # sums, G and its mirror
    # constant in the number of windows: under 1.1 GB at the c5 width, where
    # 65,536 windows of materialised diffs alone are 1.7 GB
    assert lib.mmad_nap_fit_state_bytes(6442) < 1.1e9
    for W in (0, -3, 46341):
        assert lib.mmad_nap_fit_state_bytes(W) == -1
        assert lib.mmad_nap_fit_state_layout(W, info) == -1
    assert lib.mmad_nap_fit_state_layout(48, None) == -1


def test_workspace_query_and_refusals_on_the_host():
    from icra2021_multimodal_ad_amd import _native
    lib = _native.load()
    h = ctypes.c_void_p()
    enc = (ctypes.c_int * 3)(64, 32, 8)
    dec = (ctypes.c_int * 3)(8, 32, 64)
    assert lib.mmad_ae_create(ctypes.byref(h), 0, 2, enc, 2, dec, 0, 0.2, 1e-5, 0.1) == 0
    err = lib.mmad_last_error_string
    p = ctypes.c_void_p(4096)
    try:
        q = lib.mmad_ae_nap_fit_workspace_bytes
        for B in (1, 100, 128, 129, 1000):
            base = lib.mmad_ae_workspace_bytes(h, B, 1)
            Mp = (B + 127) // 128 * 128
            # the scoring workspace, then the operand [Mp][Kp] and the layer sums [3][Mp]
            assert q(h, B, 0, 3) == (base + 255) // 256 * 256 + Mp * 128 * 4 + 3 * Mp * 4      # W = 104
            assert q(h, B, 1, 3) == (base + 255) // 256 * 256 + Mp * 128 * 4 + 3 * Mp * 4      # W = 40
            assert lib.mmad_ae_workspace_bytes(h, B, 1) == base                                # untouched
        sizes = [q(h, B, 0, 3) for B in (1, 129, 257, 1000, 4096)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)                       # grows with the batch
        big = ctypes.c_void_p()
        enc2 = (ctypes.c_int * 3)(640, 320, 8)
        dec2 = (ctypes.c_int * 3)(8, 320, 640)
        assert lib.mmad_ae_create(ctypes.byref(big), 0, 2, enc2, 2, dec2, 0, 0.2, 1e-5, 0.1) == 0
        try:
            # ... and with W: [1, 2) is 320 wide, [0, 2) 960, [0, 3) 968 (Kp 384, 1024, 1024)
            a, b, c = (q(big, 256, s, e) for s, e in ((1, 2), (0, 2), (0, 3)))
            assert a < b == c
        finally:
            lib.mmad_ae_destroy(big)
        for s, e in ((2, 1), (1, 1), (-1, 2), (0, 4)):
            assert q(h, 100, s, e) == -1
        assert q(h, 0, 0, 3) == -1 and q(None, 100, 0, 3) == -1
        # the unbound handle refuses before anything else is looked at
        assert lib.mmad_ae_nap_fit_stream(h, 0, 3, p, 64, 100, 10, p, p, p, p, p, 1 << 40, p, 1 << 40, None) == -1
        assert b"unbound" in err()
        # operand level: argument checks only
        sb = lib.mmad_nap_fit_state_bytes(40)
        assert lib.mmad_nap_fit_begin(40, None, sb, None) == -1 and b"aligned" in err()
        assert lib.mmad_nap_fit_begin(40, ctypes.c_void_p(4100), sb, None) == -1
        assert lib.mmad_nap_fit_begin(40, p, sb - 1, None) == -1 and b"fit state" in err()
        assert lib.mmad_nap_fit_accumulate_sums(40, 0, p, 40, p, sb, None) == -1 and b"bad batch" in err()
        assert lib.mmad_nap_fit_accumulate_gram(40, 8, p, 39, p, p, sb, None) == -1
        assert lib.mmad_nap_fit_accumulate_rot(40, 1, 8, p, 40, p, p, sb, None) == -1 and b"< 2" in err()
        assert lib.mmad_nap_fit_finish_mean(40, 1, p, sb, p, None) == -1
        assert lib.mmad_nap_fit_solve(40, 100, p, sb, None, None) == -1
        assert lib.mmad_nap_fit_finish(40, 100, p, sb, p, None, None) == -1
    finally:
        lib.mmad_ae_destroy(h)


def test_config_flag_plumbing_without_a_gpu():
    from icra2021_multimodal_ad_amd._native import NativeUnavailable
    from icra2021_multimodal_ad_amd.model_builder import get_model
    from icra2021_multimodal_ad_amd.novelty_detection import NoveltyDetecter
    from icra2021_multimodal_ad_amd.reconstruction_aggregation import NapScorer
    cfg = types.SimpleNamespace(input_size=64, btl_size=8, n_layers=2, gpu_id=-1, batch_size=16,
                                nap_fit_stream=True)
    m = get_model(cfg)
    x = torch.zeros(40, 64)
    cfg.train_diffs = "train_diffs.pt"
    with pytest.raises(ValueError, match="train_diffs"):
        NoveltyDetecter(cfg).scores(m, x, x, x)
    cfg.train_diffs = None
    m.dist = types.SimpleNamespace(world=2)
    with pytest.raises(ValueError, match="data-parallel"):
        NoveltyDetecter(cfg).scores(m, x, x, x)
    m.dist = None
    if not torch.cuda.is_available():
        with pytest.raises(NativeUnavailable):
            NoveltyDetecter(cfg).scores(m, x, x, x)
        with pytest.raises(NativeUnavailable):
            NapScorer(m).fit_stream(m, x, 16)
        with pytest.raises(NativeUnavailable):
            m._native.nap_fit_stream(x, 16)
    with pytest.raises(ValueError, match="scorer width"):
        NapScorer.standalone(7, device="cpu").fit_stream(m, x, 16, layers=(0, 2))
