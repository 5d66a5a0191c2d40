"""Microphone front end: MFCCs from raw PCM on the device.

The reference's deployment loop turns the raw microphone queue into MFCCs with
librosa on the CPU every tick (``save_mfcc_from_wav``,
utils/data_loaders.py:676-701: int16 PCM at 44.1 kHz, ``melspectrogram`` with
``n_fft = hop = 4410`` and 128 mels, ``power_to_db(ref=np.max)``, 13
coefficients, the last ``batch_size`` frames) and min-max normalises them
(``norm_vec``, :703-712).  ``MfccFrontEnd`` is that stage as one native call
(``mmad_mfcc``, include/mmad.h; kernels ``csrc/mmad_mfcc.hip``): it owns the
plan (window, twiddles, filterbank, DCT basis) and a growable workspace.  No
CPU fallback: without the library or a GPU it raises ``NativeUnavailable``.
"""
import numpy as np
import torch

from . import _native


def n_fft_of(sr, window_size, stride):
    """(n_fft, hop) of save_mfcc_from_wav (:691-692); the two must agree."""
    if window_size != stride:
        raise ValueError(f"MfccFrontEnd: window_size={window_size!r} != stride={stride!r}: the front end frames "
                         "with hop == n_fft, as every call of the reference does")
    return int(round(sr * window_size))


class MfccFrontEnd:
    def __init__(self, sr=44100, window_size=0.1, stride=0.1, n_mels=128, n_mfcc=13, device=None):
        self.sr, self.n_mels, self.n_mfcc = int(sr), int(n_mels), int(n_mfcc)
        self.n_fft = n_fft_of(sr, window_size, stride)
        _native.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        lib = _native.load()
        self.params = (self.sr, self.n_fft, self.n_mels, self.n_mfcc)
        nbytes = int(lib.mmad_mfcc_plan_bytes(*self.params))
        if nbytes < 0:
            raise ValueError(f"MfccFrontEnd: sr, n_fft, n_mels, n_mfcc = {self.params} out of range "
                             "(n_fft 16..4410, n_mels 1..128, n_mfcc 1..n_mels)")
        self.plan = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _native.call("mmad_mfcc_plan_init", _native.ptr(self.plan), nbytes, *self.params, _native.stream_ptr())
        self.ws = None

    def frames(self, n_samples):
        """librosa's centred frame count of ``n_samples`` (-1: too short)."""
        return int(_native.load().mmad_mfcc_frames(int(n_samples), self.n_fft))

    def _pcm(self, pcm):
        """A contiguous int16 or fp32 device vector of: a list of ``bytes``
        chunks (the reference's mic_q), an ndarray, or a tensor."""
        if isinstance(pcm, (list, tuple)) and (not pcm or isinstance(pcm[0], (bytes, bytearray, memoryview))):
            pcm = np.frombuffer(b"".join(pcm), dtype=np.int16)
        elif isinstance(pcm, (bytes, bytearray, memoryview)):
            pcm = np.frombuffer(pcm, dtype=np.int16)
        if not torch.is_tensor(pcm):
            a = np.ascontiguousarray(pcm)
            if a.dtype not in (np.int16, np.float32):
                raise TypeError(f"MfccFrontEnd: PCM of dtype {a.dtype} (int16 or float32)")
            pcm = torch.from_numpy(a.copy() if not a.flags.writeable else a)
        if pcm.dtype not in (torch.int16, torch.float32):
            raise TypeError(f"MfccFrontEnd: PCM of dtype {pcm.dtype} (int16 or float32)")
        return pcm.reshape(-1).to(self.device).contiguous()

    def run(self, pcm, keep=None, out_range=(-1, 1)):
        """(mfcc [n_frames, n_mfcc], norm [keep, n_mfcc] or None) on the device,
        enqueued on the current stream (no host synchronisation)."""
        y = self._pcm(pcm)
        F = self.frames(y.numel())
        if F < 1:
            raise ValueError(f"MfccFrontEnd: {y.numel()} samples < n_fft/2 + 1 = {self.n_fft // 2 + 1}")
        if keep is not None and not 1 <= int(keep) <= F:
            raise ValueError(f"MfccFrontEnd: the last {keep} of {F} frames")
        need = int(_native.load().mmad_mfcc_ws_bytes(F, self.n_mels))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty((F, self.n_mfcc), dtype=torch.float32, device=self.device)
        norm = None if keep is None else torch.empty((int(keep), self.n_mfcc), dtype=torch.float32,
                                                     device=self.device)
        with torch.cuda.device(self.device):
            _native.call("mmad_mfcc", _native.ptr(y), _native.PCM_I16 if y.dtype == torch.int16 else _native.PCM_F32,
                         y.numel(), *self.params, _native.ptr(self.plan), self.plan.numel(), _native.ptr(out),
                         1 if keep is None else int(keep), float(out_range[0]), float(out_range[1]),
                         _native.ptr(norm), _native.ptr(self.ws), self.ws.numel(), _native.stream_ptr())
        return out, norm

    def mfcc(self, pcm):
        """[n_frames, n_mfcc] fp32 on the device: every frame of ``pcm``."""
        return self.run(pcm)[0]

    def latest(self, pcm, B, out_range=(-1, 1)):
        """(raw, normalised) [B, n_mfcc]: the last ``B`` frames (:699) and
        their norm_vec into ``out_range`` (min and max over all B * n_mfcc)."""
        out, norm = self.run(pcm, keep=B, out_range=out_range)
        return out[out.shape[0] - int(B):], norm
