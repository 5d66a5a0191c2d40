"""The split-bf16 ("x3", MMAD_BF16X3) storage format on the CPU: a numpy
emulation of the eval / score data flow shows that two bf16 planes per operand
and three products per pair meet the project's fp32 bars on the goldens, and
the header / ctypes surface declares the format and its entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "mmad.h")
CASES = ["c1_ft64", "mm192"]
SLOPE, BN_EPS = 0.2, 1e-5


def _rel(a, r):
    a = np.asarray(a, np.float64)
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-30))


def split(x):
    """hi = RNE_bf16(x), lo = RNE_bf16(x - hi), both returned as float32."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.numpy(), lo.numpy()


def x3_matmul(a_planes, w_planes):
    """hi.hi + (hi.lo + lo.hi), products and sums in float64, result float32."""
    ah, al = (p.astype(np.float64) for p in a_planes)
    wh, wl = (p.astype(np.float64) for p in w_planes)
    return ((ah @ wl.T + al @ wh.T) + ah @ wh.T).astype(np.float32)


def _layers(g, prefix, side):
    out = []
    i = 0
    while f"{prefix}{side}.net.{i}.layer.weight" in g.files:
        p = f"{prefix}{side}.net.{i}."
        L = dict(W=split(g[p + "layer.weight"]), b=g[p + "layer.bias"].astype(np.float32), bn=None)
        if p + "bn.weight" in g.files:
            rstd = (1.0 / np.sqrt(g[p + "bn.running_var"].astype(np.float64) + BN_EPS))
            scale = (g[p + "bn.weight"] * rstd).astype(np.float32)
            shift = (g[p + "bn.bias"] - g[p + "bn.running_mean"] * scale).astype(np.float32)
            L["bn"] = (scale, shift)
        out.append(L)
        i += 1
    return out


def fc_eval(planes, L):
    """One eval FCLayer on operand planes: fp32 y = bn_affine(act(acc + bias))."""
    z = x3_matmul(planes, L["W"]) + L["b"]
    if L["bn"] is None:
        return z.astype(np.float32)
    a = np.where(z > 0, z, z * np.float32(SLOPE)).astype(np.float32)
    return (a * L["bn"][0] + L["bn"][1]).astype(np.float32)


def emulate(g, x):
    """(x_hat, diffs) as the x3 executor forms them: activations travel as
    planes, every reference of a diff stays fp32."""
    steps = int(g["meta_steps"])
    pre = f"after{steps - 1}/"
    enc, dec = _layers(g, pre, "encoder"), _layers(g, pre, "decoder")
    x = x.astype(np.float32)
    h = split(x)
    refs = []
    for L in enc:
        y = fc_eval(h, L)
        refs.append(y)
        h = split(y)
    for L in dec:
        y = fc_eval(h, L)
        h = split(y)
    xh = y
    diffs = [xh - x]
    for L, r in zip(enc, refs):
        y = fc_eval(h, L)
        diffs.append(y - r)
        h = split(y)
    return xh, diffs


@pytest.mark.parametrize("name", CASES)
def test_x3_emulation_meets_fp32_bars(golden, name):
    g = golden(name)
    xh, _ = emulate(g, g["x/0"])
    assert _rel(xh, g["eval/x_hat"]) < 1e-4
    _, diffs = emulate(g, g["score/test_x"])
    for i, dd in enumerate(diffs):
        ref = g[f"score/test_diff{i}"]
        assert dd.shape == ref.shape
        assert np.abs(dd - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), i
    base = (diffs[0].astype(np.float64) ** 2).mean(axis=1)
    sap = (np.concatenate(diffs, axis=-1).astype(np.float64) ** 2).mean(axis=1)
    assert _rel(base, g["score/base"]) < 1e-4
    assert _rel(sap, g["score/sap"]) < 1e-4


def test_split_is_exact_to_two_planes():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))).astype(np.float32)
    hi, lo = split(x)
    err = np.abs((hi.astype(np.float64) + lo) - x) / np.abs(x)
    assert err.max() <= 2.0 ** -17        # 8 + 8 mantissa bits and the two signs


def test_header_declares_the_format():
    src = open(HEADER).read()
    m = re.search(r"enum\s*\{[^}]*MMAD_BF16X3\s*=\s*(\d+)[^}]*\}", src)
    assert m and int(m.group(1)) == 2
    for fn in ("mmad_split_planes", "mmad_ae_set_score_planes", "mmad_ae_score_dtype"):
        assert re.search(r"^int\s+" + fn + r"\s*\(", src, re.M), fn


def test_ctypes_surface_declares_the_format():
    from icra2021_multimodal_ad_amd import _native
    assert _native.BF16X3 == 2
    for fn in ("mmad_split_planes", "mmad_ae_set_score_planes", "mmad_ae_score_dtype"):
        assert fn in _native.SIGNATURES, fn
    assert len(_native.SIGNATURES["mmad_split_planes"][1]) == 5
    lib = _native.load()
    for fn in ("mmad_split_planes", "mmad_ae_set_score_planes", "mmad_ae_score_dtype"):
        assert hasattr(lib, fn), fn


def test_x3_refusals_on_the_host():
    """Argument checks that need no GPU: a score-only handle cannot be created,
    planes attach to fp32 handles only, the training operators refuse dtype 2."""
    import ctypes
    from icra2021_multimodal_ad_amd import _native
    lib = _native.load()
    h = ctypes.c_void_p()
    enc = (ctypes.c_int * 3)(64, 32, 8)
    dec = (ctypes.c_int * 3)(8, 32, 64)
    assert lib.mmad_ae_create(ctypes.byref(h), 2, 2, enc, 2, dec, 0, 0.2, 1e-5, 0.1) == -1
    assert lib.mmad_last_error_string()
    assert lib.mmad_ae_create(ctypes.byref(h), 1, 2, enc, 2, dec, 0, 0.2, 1e-5, 0.1) == 0
    try:
        assert lib.mmad_ae_score_dtype(h) == 1
        assert lib.mmad_ae_set_score_planes(h, ctypes.c_void_p(4096)) == -1
        assert b"fp32 handles only" in lib.mmad_last_error_string()
    finally:
        lib.mmad_ae_destroy(h)
    assert lib.mmad_fc_bwd_weight(2, 128, 128, 128, None, None, None, None) == -2
    assert b"MMAD_BF16X3" in lib.mmad_last_error_string()
