"""Writes tests/golden/mfcc_cases.npz: per case of tests/test_mfcc_abi.CASES
the float64 MFCCs of the numpy restatement (``<case>/mfcc``) and ``<case>/err32``,
the max abs error against them of the same restatement run in float32 end to
end (scipy.fft.rfft and scipy.fft.dct on float32: the reference's own
arithmetic, librosa computing in float32).  The bar of tests/test_gpu_mfcc.py
is twice that error.  The inputs are not stored: the tests regenerate them
from the closed formula (test_mfcc_abi.signal).

Run from the repository root (needs scipy):  python tests/golden/gen_mfcc_golden.py
"""
import os
import sys

import numpy as np
import scipy.fft

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_mfcc_abi import CASES, case_pcm, mfcc_ref  # noqa: E402


def main():
    out = {}
    for name, (_, sr, n_fft, _) in CASES.items():
        y = case_pcm(name)
        ref = mfcc_ref(y, sr, n_fft)
        f32 = mfcc_ref(y, sr, n_fft, dtype=np.float32, rfft=scipy.fft.rfft,
                       dct=lambda db: scipy.fft.dct(db, axis=0, type=2, norm="ortho"))
        assert f32.dtype == np.float32 and ref.dtype == np.float64
        err = float(np.abs(f32.astype(np.float64) - ref).max())
        out[name + "/mfcc"] = ref
        out[name + "/err32"] = np.float64(err)
        print(f"{name:8s} frames {ref.shape[0]:3d}  max|mfcc| {np.abs(ref).max():8.3f}  err32 {err:.3e}")
    np.savez_compressed(os.path.join(HERE, "mfcc_cases.npz"), **out)


if __name__ == "__main__":
    main()
