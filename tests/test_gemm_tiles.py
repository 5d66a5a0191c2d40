"""The GEMM dispatcher's tile rule (mmad_gemm_tile_for: which tile's kernel
runs when a tile is forced through knob 0, or -1 when it may not be chosen),
checked over the whole grid of tiles x problems against the rules written out
here by hand.  The query is a pure function, so this needs no GPU.

The expectation below is the rule as the dispatcher applied it before it was
folded into one table (the fit check, the dispatcher's filter for splits and
fused BN, and the launcher's register-direct fallback); it deliberately
shares nothing with the library's table."""
import itertools

import pytest

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd._native import F32, BF16

FWD, MSE, BWD_DATA, BWD_WEIGHT, SCORE = range(5)
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
# tile -> (rows, columns) of its block
SHAPE = {0: (128, 128), 1: (256, 128), 2: (128, 256), 3: (64, 64), 4: (64, 128), 5: (128, 128),
         6: (256, 256), 7: (256, 256), 8: (256, 256), 9: (256, 128)}
PROBLEMS = [(128, 128), (256, 128), (128, 256), (256, 256), (4096, 1664), (4096, 2048)]


def expected_tile(cfg, dtype, epi, Mp, Np, splitk, fused_bn, has_partials, act):
    bm, bn = SHAPE[cfg]
    if Mp % bm or Np % bn:
        return -1
    if cfg in (6, 7, 8) and not (dtype == BF16 and epi in (FWD, MSE, SCORE)):
        return -1
    if cfg in (7, 8, 9) and not (dtype == BF16 and epi in (FWD, SCORE)):
        return -1
    if epi == SCORE and bn < 128:
        return -1
    if cfg in (6, 7, 8, 9) and (splitk > 1 or fused_bn):
        return -1
    if fused_bn and epi not in (FWD, BWD_DATA):
        return -1
    if cfg in (7, 8, 9) and (has_partials or act not in (ACT_NONE, ACT_LEAKY, ACT_RELU)):
        return 6 if cfg in (7, 8) else 1
    return cfg


def test_tile_rule_over_the_whole_grid():
    lib = _native.load()
    bad = []
    n = 0
    for cfg, dtype, epi, (Mp, Np), splitk, bnf, part, act in itertools.product(
            range(10), (F32, BF16), range(5), PROBLEMS, (1, 2), (0, 1), (0, 1),
            (ACT_NONE, ACT_LEAKY, ACT_SIGMOID)):
        got = lib.mmad_gemm_tile_for(cfg, dtype, epi, Mp, Np, splitk, bnf, part, act)
        want = expected_tile(cfg, dtype, epi, Mp, Np, splitk, bnf, part, act)
        n += 1
        if got != want:
            bad.append(((cfg, dtype, epi, Mp, Np, splitk, bnf, part, act), got, want))
    assert n == 10 * 2 * 5 * 6 * 2 * 2 * 2 * 3
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("cfg", [-1, 10, 99])
def test_no_such_tile_is_never_chosen(cfg):
    assert _native.load().mmad_gemm_tile_for(cfg, BF16, FWD, 4096, 2048, 1, 0, 0, ACT_NONE) == -1
