"""The grouping rule of the ping-pong step's grouped dW launches
(mmad_dw_group_plan, a pure host function): which side-stream layers share a
launch for the bench configurations' widths."""
import ctypes

import pytest

from icra2021_multimodal_ad_amd import _native
from icra2021_multimodal_ad_amd.common_utils import ae_widths


def plan(d, btl, vib, rows, budget, members, dw_main=1, late=0):
    lib = _native.load()
    enc, dec = ae_widths(d, btl, 5, enc_out=2 * btl if vib else None)
    ws = list(zip(enc[:-1], enc[1:])) + list(zip(dec[:-1], dec[1:]))
    n = len(ws)
    arr = ctypes.c_int * n
    g = arr()
    k = lib.mmad_dw_group_plan(n, arr(*[_native.pad(b) for _, b in ws]), arr(*[_native.pad(a) for a, _ in ws]),
                               arr(*[_native.pad(rows)] * n), dw_main, n - late, budget, members, g)
    return k, list(g)


def test_c3_groups():
    """c3 (VIB-AE D=2048, 4096 rows), one resident round of 512 blocks: the
    four narrow layers 6, 5, 4, 3 (112 + 16 + 40 + 160 blocks) form the one
    group.  Layers 7 (280 blocks) and 2 (352) exceed half a round and layers
    9, 8, 1 take the 128x128 tile: launches of their own."""
    assert plan(2048, 100, True, 4096, 512, 4) == (1, [-1, -1, -1, 0, 0, 0, 0, -1, -1, -1])
    # capped at two members: {6, 5} and {4, 3}
    assert plan(2048, 100, True, 4096, 512, 2) == (2, [-1, -1, -1, 1, 1, 0, 0, -1, -1, -1])
    # a budget the four do not fit: {6, 5, 4} (168 blocks), layer 3 alone
    assert plan(2048, 100, True, 4096, 320, 4) == (1, [-1, -1, -1, -1, 0, 0, 0, -1, -1, -1])
    # off
    assert plan(2048, 100, True, 4096, 0, 4) == (0, [-1] * 10)
    assert plan(2048, 100, True, 4096, 512, 1) == (0, [-1] * 10)
    # the top layers held back (knob 33) stay out
    assert plan(2048, 100, True, 4096, 512, 4, late=4) == (1, [-1, -1, -1, 0, 0, 0, -1, -1, -1, -1])


def test_c2_groups():
    """c2's widths (AE D=2048, 1024 rows: every dW on the 64x64 tile) give the
    same four narrow layers (112 + 16 + 16 + 112 blocks); its step has no
    ping-pong schedule at 1024 rows, so the executor never applies the rule
    there."""
    assert plan(2048, 100, False, 1024, 512, 4, dw_main=2) == (1, [-1, -1, -1, 0, 0, 0, 0, -1, -1, -1])


def test_tile_rule_decides_membership():
    """A member is a layer knob 5's rule puts on the 64x64 tile."""
    with _native.tune(tile_adam=0):
        assert plan(2048, 100, True, 4096, 512, 4) == (0, [-1] * 10)
    with _native.tune(tile_adam=3):
        # every layer on the tile: only the size rule and the budget are left
        k, g = plan(2048, 100, True, 4096, 512, 4)
        assert k == 1 and g == [-1, -1, -1, 0, 0, 0, 0, -1, -1, -1]
