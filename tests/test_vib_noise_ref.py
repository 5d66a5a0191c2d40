"""The reference generator the GPU noise test compares with (tests/philox_ref.py)
is itself pinned here, without a GPU: its integer core against the published
Philox4x32-10 known-answer vectors (Random123's kat_vectors), and its N(0,1)
output by the moments and correlations of 2^20 draws.

The statistical bounds are 5 sigma for n = 2^20 iid N(0,1) values: the mean
has sd 1/sqrt(n) = 9.8e-4, the variance sqrt(2/n) = 1.4e-3, the fourth moment
sqrt(96/n) = 9.6e-3, a sample correlation 1/sqrt(n) = 9.8e-4."""
import numpy as np
import pytest

from tests import philox_ref as P

N = 1 << 20

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox4x32_10_known_answers(counter, key, want):
    got = tuple(int(w[0]) for w in P.philox4x32(counter, key))
    assert got == want, [hex(g) for g in got]


def test_counter_and_key_words():
    """uniforms() puts idx in counter words 0-1, offset in 2-3, seed in the key,
    low word first, and vectorises: element i of an array call is the scalar call."""
    seed, offset = (0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e
    idx = (0x85a308d3 << 32) | 0x243f6a88
    u1, u2 = P.uniforms(seed, offset, np.array([idx], dtype=np.uint64))
    assert u1[0] == ((0xd16cfe09 >> 8) + 1) / 16777217.0
    assert u2[0] == (0x94fdcceb >> 8) / 16777216.0
    many = P.normal(7, 3, np.arange(1000))
    for i in (0, 1, 255, 999):
        assert many[i] == P.normal(7, 3, np.array([i]))[0]
    e, u = P.vib_eps(7, 3, 2, 5, 4)
    assert e.shape == (2, 5, 4) and np.array_equal(e.ravel(), many[:40])
    assert (u > 0).all() and (u < 1).all()


@pytest.fixture(scope="module")
def draws():
    idx = np.arange(N)
    return P.normal(7, 3, idx), P.normal(7, 4, idx), P.normal(8, 3, idx)


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def test_reference_draws_are_standard_normal(draws):
    e = draws[0]
    assert np.isfinite(e).all()
    mean, var, m4 = float(e.mean()), float(e.var()), float((e ** 4).mean())
    print(f"mean {mean:.3e} var {var:.6f} m4 {m4:.5f}")
    assert abs(mean) <= 5e-3
    assert abs(var - 1.0) <= 7e-3
    assert abs(m4 - 3.0) <= 0.05


def test_reference_draws_are_uncorrelated(draws):
    e, e_off, e_seed = draws
    lag1, off, seed = _corr(e[:-1], e[1:]), _corr(e, e_off), _corr(e, e_seed)
    print(f"lag1 {lag1:.3e} offset {off:.3e} seed {seed:.3e}")
    assert abs(lag1) <= 5e-3
    assert abs(off) <= 5e-3
    assert abs(seed) <= 5e-3
