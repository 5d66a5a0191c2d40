"""Numpy restatement of the VIB noise draw (philox_normal, csrc/mmad_ops_vib.hip):
Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
SC'11) keyed by the 64-bit seed, counter = (element index, offset), the first
two output words turned into one N(0,1) value by Box-Muller in float64.

    counter = (idx_lo, idx_hi, offset_lo, offset_hi),  key = (seed_lo, seed_hi)
    u1 = ((c0 >> 8) + 1) / 16777217  in (0, 1),  u2 = (c1 >> 8) / 16777216  in [0, 1)
    e  = sqrt(-2 ln u1) * cos(2 pi u2)
    idx = (kk * B + b) * btl + c      (sample kk, window b, bottleneck column c)

Shared by tests/test_vib_noise_ref.py (known answers, statistics; no GPU) and
tests/test_gpu_vib_ops.py (the kernel's eps_out against this draw)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 words.  Returns the
    4 output words as uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]        # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> _S32, p0 & _MASK
        hi1, lo1 = p1 >> _S32, p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def uniforms(seed, offset, idx):
    """(u1, u2) in float64 of the elements idx (any integer array)."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed, offset = int(seed), int(offset)
    c = philox4x32((idx & _MASK, idx >> _S32, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                   (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = ((c[0] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777217.0
    u2 = (c[1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    return u1, u2


def normal(seed, offset, idx):
    u1, u2 = uniforms(seed, offset, idx)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def vib_eps(seed, offset, k, B, btl):
    """The draw of one VIB forward: float64 [k][B][btl] and its u1."""
    idx = np.arange(k * B * btl, dtype=np.uint64)
    u1, u2 = uniforms(seed, offset, idx)
    e = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return e.reshape(k, B, btl), u1.reshape(k, B, btl)
