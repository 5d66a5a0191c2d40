"""Microphone front end, host side (no GPU): the exported mmad_mfcc_* symbols,
the frame count, the mel filterbank against a float64 restatement, every
refusal of mmad_mfcc / mmad_mfcc_plan_init (none reaches a launch: they pass
on a machine with no GPU) and the Python front end's argument check.

This module also holds the yardstick of tests/test_gpu_mfcc.py and
tests/golden/gen_mfcc_golden.py: ``mfcc_ref``, librosa 0.8's recipe
(melspectrogram -> power_to_db(ref=np.max) -> DCT-II ortho) restated in numpy,
and the closed integer formula of the test signals."""
import ctypes
import re

import numpy as np
import pytest

from tests.conftest import REPO

EINVAL = -1

# ----------------------------------------------------------------- the yardstick


def mel_filterbank(sr, n_fft, n_mels):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin=0, fmax=sr/2, htk=False,
    norm='slaney'), float64 [n_mels, n_fft//2 + 1]."""
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz_to_mel(f):
        return min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    mels = np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2)
    mel_f = np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)), f_sp * mels)
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def dct_basis(n_mels, n_mfcc, dtype=np.float64):
    """Rows 0..n_mfcc-1 of the orthonormal DCT-II (scipy.fftpack.dct(type=2, norm='ortho'))."""
    m = np.arange(n_mels)
    b = np.sqrt(2.0 / n_mels) * np.cos(np.pi * (2 * m[None, :] + 1) * np.arange(n_mfcc)[:, None] / (2.0 * n_mels))
    b[0] = np.sqrt(1.0 / n_mels)
    return b.astype(dtype)


def mel_db(y, sr, n_fft, n_mels, dtype=np.float64, rfft=np.fft.rfft):
    """power_to_db(melspectrogram(y, sr, n_fft, hop_length=n_fft, n_mels), ref=np.max) in
    ``dtype``: (dB [n_mels, n_frames], the share of entries on the -80 dB floor)."""
    y = np.asarray(y).astype(dtype)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    F = 1 + (len(yp) - n_fft) // n_fft
    n = np.arange(n_fft)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)).astype(dtype)
    frames = yp[:F * n_fft].reshape(F, n_fft) * win                       # hop == n_fft
    spec = rfft(frames, axis=1)
    power = (np.abs(spec) ** 2).astype(dtype)                             # [F, bins]
    S = mel_filterbank(sr, n_fft, n_mels).astype(dtype) @ power.T         # [n_mels, F]
    amin = dtype(1e-10)
    db = dtype(10.0) * np.log10(np.maximum(amin, S)) - dtype(10.0) * np.log10(np.maximum(amin, S.max()))
    floor = db.max() - dtype(80.0)
    return np.maximum(db, floor).astype(dtype), float((db < floor).mean())


def mfcc_ref(y, sr, n_fft, n_mels=128, n_mfcc=13, dtype=np.float64, rfft=np.fft.rfft, dct=None):
    """[n_frames, n_mfcc] in ``dtype``; dct: None (the explicit cosine matrix) or a
    callable dB [n_mels, F] -> [n_mels, F] (scipy's, in gen_mfcc_golden.py)."""
    db, _ = mel_db(y, sr, n_fft, n_mels, dtype, rfft)
    if dct is None:
        return (dct_basis(n_mels, n_mfcc, dtype) @ db).T
    return np.asarray(dct(db))[:n_mfcc].T


def norm_vec_ref(v, lo=-1.0, hi=1.0):
    v = np.asarray(v, dtype=np.float64)
    return (hi - lo) * (v - v.min()) / (v.max() - v.min()) + lo


def signal(L, tones, noise, seed, silent=0):
    """int16 [L]: the sum of ``tones`` (amplitude, cycles per 44100 samples,
    phase in 1/360 turns) rounded to the nearest integer, plus ``noise`` *
    uniform [-1, 1) steps of a 31-bit linear congruential generator; the
    first ``silent`` samples exactly 0."""
    n = np.arange(L, dtype=np.int64)
    y = np.zeros(L)
    for amp, cyc, ph in tones:
        turns = ((n * cyc) % 44100) / 44100.0 + ph / 360.0                  # exact phase reduction
        y += amp * np.sin(2 * np.pi * turns)
    y = np.rint(y).astype(np.int64)
    if noise:
        state, draws = seed, np.empty(L, dtype=np.int64)
        for i in range(L):
            state = (1103515245 * state + 12345) % (1 << 31)
            draws[i] = state
        y += ((draws >> 8) % (2 * noise)) - noise
    y[:silent] = 0
    assert np.abs(y).max() < 32768
    return y.astype(np.int16)


TONES = [(9000, 440, 0), (4000, 3520, 90), (1500, 9001, 45)]
# name -> (pcm_type, sr, n_fft, signal arguments); the cases of the issue's GPU list
CASES = {
    "deploy": ("i16", 44100, 4410, dict(L=44100, tones=TONES, noise=300, seed=1)),
    "odd": ("f32", 22050, 2205, dict(L=5 * 2205 + 777, tones=TONES, noise=300, seed=2)),
    "one": ("i16", 44100, 4410, dict(L=4410 // 2 + 1, tones=TONES, noise=300, seed=3)),
    "silence": ("i16", 44100, 4410, dict(L=44100, tones=[(30000, 1000, 0)], noise=0, seed=4, silent=3 * 4410)),
    "rows64": ("i16", 44100, 4410, dict(L=64 * 4410, tones=TONES, noise=300, seed=5)),
}


def case_pcm(name):
    """The case's samples as the kernel takes them: int16, or their fp32 / 32768."""
    kind, _, _, args = CASES[name]
    y = signal(**args)
    return y if kind == "i16" else (y.astype(np.float32) / np.float32(32768.0))


# --------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def lib():
    from icra2021_multimodal_ad_amd import _native
    return _native.load()


def test_symbols_exported_with_the_headers_argument_counts(lib):
    from icra2021_multimodal_ad_amd._native import SIGNATURES
    src = re.sub(r"/\*.*?\*/", "", open(REPO + "/include/mmad.h").read(), flags=re.S)
    want = {"mmad_mfcc_frames": 2, "mmad_mfcc_filterbank": 4, "mmad_mfcc_plan_bytes": 4, "mmad_mfcc_plan_init": 7,
            "mmad_mfcc_ws_bytes": 2, "mmad_mfcc": 17}
    for name, n in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\);", src, re.S)
        assert m is not None, name
        assert m.group(1).count(",") + 1 == n == len(SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+MMAD_PCM_I16\s+0\b", src) and re.search(r"#define\s+MMAD_PCM_F32\s+1\b", src)


@pytest.mark.parametrize("L,n_fft,want", [(44100, 4410, 11), (11025 + 777, 2205, 6), (2206, 4410, 1),
                                          (2205, 4410, -1)])
def test_frame_count(lib, L, n_fft, want):
    assert lib.mmad_mfcc_frames(L, n_fft) == want
    if want > 0:
        assert want == 1 + (len(np.pad(np.zeros(L), n_fft // 2, mode="reflect")) - n_fft) // n_fft


@pytest.mark.parametrize("sr,n_fft,n_mels", [(44100, 4410, 128), (22050, 2205, 128), (44100, 126, 128)])
def test_filterbank_against_float64(lib, sr, n_fft, n_mels):
    ref = mel_filterbank(sr, n_fft, n_mels)
    got = np.full(ref.shape, np.nan)
    assert lib.mmad_mfcc_filterbank(sr, n_fft, n_mels, got.ctypes.data_as(ctypes.c_void_p)) == 0
    err = np.abs(got - ref).max()
    print(f"filterbank {sr}/{n_fft}/{n_mels}: max abs err {err:.3e}, largest weight {ref.max():.3e}")
    assert err <= 1e-10 * ref.max()
    empty = ~ref.any(axis=1)
    assert (got[empty] == 0).all()
    if n_fft == 126:
        assert int(empty.sum()) == 55
    # a bin lies inside at most two triangles: what the plan's weight capacity rests on
    assert int((got != 0).sum()) <= 2 * ref.shape[1]


def test_filterbank_refusals(lib):
    fb = np.zeros((128, 2206))
    p = fb.ctypes.data_as(ctypes.c_void_p)
    for args in [(44100, 4411, 128, p), (44100, 15, 128, p), (44100, 4410, 129, p), (44100, 4410, 0, p),
                 (0, 4410, 128, p), (44100, 4410, 128, None)]:
        assert lib.mmad_mfcc_filterbank(*args) == EINVAL, args
    assert (fb == 0).all()


def _fake(addr):
    """A device-looking pointer that is never dereferenced: every call below
    is refused on the host before any launch or copy."""
    return ctypes.c_void_p(addr)


def test_every_refusal_of_mmad_mfcc_comes_before_a_launch(lib):
    P = (44100, 4410, 128, 13)
    L, F = 44100, 11
    pb, wb = lib.mmad_mfcc_plan_bytes(*P), lib.mmad_mfcc_ws_bytes(F, 128)
    assert pb > 0 and wb > 0 and pb % 256 == 0 and wb % 256 == 0
    good = dict(pcm=_fake(0x10000), pcm_type=0, L=L, P=P, plan=_fake(0x20000), plan_bytes=pb, out=_fake(0x30000),
                keep=10, norm_out=_fake(0x40000), ws=_fake(0x50000), ws_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mmad_mfcc(a["pcm"], a["pcm_type"], a["L"], *a["P"], a["plan"], a["plan_bytes"], a["out"],
                             a["keep"], -1.0, 1.0, a["norm_out"], a["ws"], a["ws_bytes"], None)

    bad = {
        "null pcm": dict(pcm=None), "null plan": dict(plan=None), "null out": dict(out=None),
        "null ws": dict(ws=None),
        "plan too small": dict(plan_bytes=pb - 1), "plan misaligned": dict(plan=_fake(0x20080)),
        "ws too small": dict(ws_bytes=wb - 1), "ws misaligned": dict(ws=_fake(0x50010)),
        "L too short": dict(L=2205), "L zero": dict(L=0),
        "keep zero": dict(keep=0), "keep past the frames": dict(keep=F + 1), "keep negative": dict(keep=-3),
        "pcm_type": dict(pcm_type=2), "pcm_type negative": dict(pcm_type=-1),
        "n_fft high": dict(P=(44100, 4411, 128, 13)), "n_fft low": dict(P=(44100, 15, 128, 13)),
        "n_mels high": dict(P=(44100, 4410, 129, 13)), "n_mels zero": dict(P=(44100, 4410, 0, 13)),
        "n_mfcc high": dict(P=(44100, 4410, 64, 65)), "n_mfcc zero": dict(P=(44100, 4410, 128, 0)),
        "sr zero": dict(P=(0, 4410, 128, 13)),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        assert lib.mmad_last_error_string().startswith(b"mfcc:"), what


def test_every_refusal_of_plan_init_comes_before_the_copy(lib):
    P = (44100, 4410, 128, 13)
    pb = lib.mmad_mfcc_plan_bytes(*P)
    for what, args in {
        "null plan": (None, pb, *P), "misaligned": (_fake(0x20040), pb, *P), "too small": (_fake(0x20000), pb - 1, *P),
        "n_fft high": (_fake(0x20000), pb, 44100, 4411, 128, 13), "n_fft low": (_fake(0x20000), pb, 44100, 15, 128, 13),
        "n_mels": (_fake(0x20000), pb, 44100, 4410, 129, 13), "n_mfcc": (_fake(0x20000), pb, 44100, 4410, 13, 14),
        "sr": (_fake(0x20000), pb, -1, 4410, 128, 13),
    }.items():
        assert lib.mmad_mfcc_plan_init(*args, None) == EINVAL, what
        assert lib.mmad_last_error_string().startswith(b"mfcc_plan_init:"), what
    for P_bad in [(44100, 4411, 128, 13), (44100, 4410, 129, 13), (44100, 4410, 128, 129), (0, 4410, 128, 13)]:
        assert lib.mmad_mfcc_plan_bytes(*P_bad) == -1
    assert lib.mmad_mfcc_ws_bytes(0, 128) == -1 and lib.mmad_mfcc_ws_bytes(4, 129) == -1


def test_plan_and_workspace_sizes_grow_monotonically(lib):
    ffts = [16, 17, 126, 1024, 2205, 4409, 4410]
    sizes = [lib.mmad_mfcc_plan_bytes(44100, n, 128, 13) for n in ffts]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]
    by_mels = [lib.mmad_mfcc_plan_bytes(44100, 4410, m, min(m, 13)) for m in (1, 13, 40, 128)]
    by_mfcc = [lib.mmad_mfcc_plan_bytes(44100, 4410, 128, c) for c in (1, 13, 64, 128)]
    assert by_mels == sorted(by_mels) and by_mfcc == sorted(by_mfcc) and by_mfcc[-1] > by_mfcc[0]
    # the plan holds at least the tables the header names
    assert sizes[-1] >= 8 * (3 * 4410 + 13 * 128)
    ws = [lib.mmad_mfcc_ws_bytes(f, 128) for f in (1, 2, 11, 65, 1000)]
    assert all(b > a for a, b in zip(ws, ws[1:]))
    assert all(lib.mmad_mfcc_ws_bytes(11, a) <= lib.mmad_mfcc_ws_bytes(11, b) for a, b in [(1, 40), (40, 128)])
    assert lib.mmad_mfcc_ws_bytes(11, 128) >= 8 * 11 * (128 + 1)


def test_front_end_refuses_window_size_other_than_stride():
    from icra2021_multimodal_ad_amd.mfcc import MfccFrontEnd
    with pytest.raises(ValueError, match="window_size"):
        MfccFrontEnd(window_size=0.1, stride=0.05)
    from icra2021_multimodal_ad_amd import data_loaders
    import types
    with pytest.raises(ValueError, match="window_size"):
        data_loaders.save_mfcc_from_wav([b"\0\0"], types.SimpleNamespace(batch_size=1, gpu_id=0), 0.1,
                                        window_size=0.2, stride=0.1)


def test_restatement_properties():
    """The yardstick itself: the DCT basis is orthonormal, the silent-prefix
    case exercises the -80 dB clamp without being all clamp."""
    b = dct_basis(128, 128)
    assert np.abs(b @ b.T - np.eye(128)).max() < 1e-13
    _, sr, n_fft, args = CASES["silence"]
    db, share = mel_db(signal(**args), sr, n_fft, 128)
    assert 0 < share < 1
    assert (db[:, :3] == db.max() - 80).all()
