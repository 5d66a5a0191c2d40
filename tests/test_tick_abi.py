"""The sensor tick, host side (no GPU): mmad_hsr_fuse_raw and
mmad_ae_online_tick are declared and exported, every refusal of
mmad_hsr_fuse_raw comes back as MMAD_EINVAL with a message before any launch
(as tests/test_mfcc_abi.py checks for mmad_mfcc), and OnlineScorer has the
bind_sensors / tick / refresh_sensors surface."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from tests.conftest import REPO

EINVAL = -1
U8, F32 = 1, 4      # MMAD_SRC_U8, MMAD_SRC_F32


@pytest.fixture(scope="module")
def lib():
    from icra2021_multimodal_ad_amd import _native
    return _native.load()


def test_symbols_declared_and_exported(lib):
    from icra2021_multimodal_ad_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(REPO + "/include/mmad.h").read(), flags=re.S)
    for name, n in {"mmad_hsr_fuse_raw": 18, "mmad_ae_online_tick": 4}.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\);", src, re.S)
        assert m is not None, name
        assert m.group(1).count(",") + 1 == n == len(_native.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+MMAD_SRC_U8\s+1\b", src) and re.search(r"#define\s+MMAD_SRC_F32\s+4\b", src)
    assert (_native.SRC_U8, _native.SRC_F32) == (U8, F32)
    # the argument struct mirrors the header's, name for name and in order
    body = re.search(r"typedef\s+struct\s+mmad_tick_args\s*\{(.*?)\}\s*mmad_tick_args\s*;", src, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.search(r"(\w+)\s*(?:\[\d+\])?$", first.strip()).group(1))
        names += [re.search(r"(\w+)", r).group(1) for r in rest]
    assert names == [f[0] for f in _native.TickArgs._fields_]
    # additive entries leave the ABI version where it was
    assert lib.mmad_abi_version() == 1


def _fake(addr):
    """A device-looking pointer that is never dereferenced."""
    return ctypes.c_void_p(addr)


def test_every_refusal_of_hsr_fuse_raw_comes_before_a_launch(lib):
    good = dict(n=3, r=_fake(0x10000), r_type=U8, d=_fake(0x20000), d_type=U8, t=_fake(0x30000), m=_fake(0x40000),
                ranges=(0.0, 255.0, 0.0, 255.0, 0.0, 400.0), w=_fake(0x50000), unimodal=0, out=_fake(0x60000),
                ld_out=1728)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mmad_hsr_fuse_raw(a["n"], a["r"], a["r_type"], a["d"], a["d_type"], a["t"], a["m"], *a["ranges"],
                                     a["w"], a["unimodal"], a["out"], a["ld_out"], None)

    bad = {
        # mmad_hsr_fuse's own
        "negative n": dict(n=-1), "null weights": dict(w=None), "null out": dict(out=None),
        "fused without r": dict(r=None), "fused without d": dict(d=None), "fused without t": dict(t=None),
        "fused without m": dict(m=None),
        "unimodal without a modality": dict(unimodal=1, r=None, d=None, t=None, m=None),
        "ld_out below the fused width": dict(ld_out=1727),
        "ld_out below the unimodal width": dict(unimodal=1, d=None, t=None, m=None, ld_out=1023),
        # the raw entry's
        "r of uint16": dict(r_type=2), "r of float64": dict(r_type=0), "d of int32": dict(d_type=3),
        "d of an unknown type": dict(d_type=9), "r type negative": dict(r_type=-1),
        "r range empty": dict(ranges=(7.0, 7.0, 0.0, 255.0, 0.0, 400.0)),
        "d range empty": dict(ranges=(0.0, 255.0, 255.0, 255.0, 0.0, 400.0)),
        "t range empty": dict(ranges=(0.0, 255.0, 0.0, 255.0, 400.0, 400.0)),
        "unimodal d, its range empty": dict(unimodal=1, t=None, m=None, ranges=(0.0, 255.0, 1.0, 1.0, 0.0, 400.0)),
        "unimodal r, its type unknown": dict(unimodal=1, d=None, t=None, m=None, r_type=7),
        "u8 r on an odd address": dict(r=_fake(0x10001)),
        "fp32 d off a 4-byte boundary": dict(d_type=F32, d=_fake(0x20002)),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        msg = lib.mmad_last_error_string()
        assert msg.startswith(b"hsr_fuse_raw:") and len(msg) > len(b"hsr_fuse_raw: "), (what, msg)
    # n == 0 is an empty call, as for mmad_hsr_fuse: accepted, nothing to launch
    assert call(n=0) == 0
    # a modality the call does not read is not checked: unimodal mic ignores r's type and range
    assert call(n=0, unimodal=1, r_type=9, ranges=(1.0, 1.0, 0.0, 255.0, 0.0, 400.0)) == 0


def test_tick_refuses_a_null_handle_or_struct(lib):
    from icra2021_multimodal_ad_amd._native import TickArgs
    assert lib.mmad_ae_online_tick(None, ctypes.byref(TickArgs()), 1, None) == EINVAL
    assert lib.mmad_last_error_string().startswith(b"ae_online_tick:")


def test_scorer_surface():
    from icra2021_multimodal_ad_amd.hsr_net import HSR_Net
    from icra2021_multimodal_ad_amd.online import OnlineScorer
    p = inspect.signature(OnlineScorer.bind_sensors).parameters
    assert list(p) == ["self", "hsr_net", "mic_samples", "hand_dtype", "depth_dtype", "front_end"]
    assert p["hand_dtype"].default is np.uint8 and p["depth_dtype"].default is np.uint8
    assert p["front_end"].default is None
    assert list(inspect.signature(OnlineScorer.tick).parameters) == ["self", "force_q", "hand_q", "depth_q", "mic_q"]
    assert list(inspect.signature(OnlineScorer.refresh_sensors).parameters) == ["self"]
    out = inspect.signature(HSR_Net.packed_weights).parameters["out"]
    assert out.default is None
    from icra2021_multimodal_ad_amd.engine import NativeAE
    assert callable(NativeAE.online_tick)
