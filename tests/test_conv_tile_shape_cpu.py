"""The convolution dispatcher's rule (``conv_tile_shape`` in ``csrc/conv.hip``) through its host query ``ophip_conv_tile_shape``; no GPU.

The wave tile follows from a wave count of the (2, 2) shape, ``w22 = ceil(Wout/32) * ceil(Hout/2) * B * ceil(cout_pad/128) * 2``, with
thresholds at 1000 and 2000.  Every row below names its sizes, the ``w22`` they give and the band that value lies in, all written out by
hand; ``EXPECT`` is the rule's table, written out as well.  Nothing here computes ``w22`` or a shape.
"""
import ctypes

import pytest

from onepose_st_amd import hip

# (ks, stride) -> band -> (th, nt, wave_rows);  "hi": w22 >= 2000, "mid": 1000 <= w22 < 2000, "lo": w22 < 1000
EXPECT = {
    (3, 1): {"hi": (2, 2, 2), "mid": (2, 1, 1), "lo": (1, 1, 1)},
    (3, 2): {"hi": (2, 2, 1), "mid": (1, 2, 1), "lo": (1, 1, 1)},
    (1, 1): {"hi": (2, 2, 1), "mid": (1, 2, 1), "lo": (1, 2, 1)},
    (1, 2): {"hi": (2, 2, 1), "mid": (1, 2, 1), "lo": (1, 2, 1)},
}

ROWS = [
    # B, Hout, Wout, cout_pad, w22, band
    # Wout = 37 (2 tile columns), B = 2, cout_pad = 224 (2 channel groups): w22 = 16 * ceil(Hout / 2) -- the reachable values around 1000 ...
    (2, 123, 37, 224, 992, "lo"),
    (2, 124, 37, 224, 992, "lo"),
    (2, 125, 37, 224, 1008, "mid"),
    (2, 126, 37, 224, 1008, "mid"),
    # ... and around 2000, which is reached exactly
    (2, 247, 37, 224, 1984, "mid"),
    (2, 248, 37, 224, 1984, "mid"),
    (2, 249, 37, 224, 2000, "hi"),
    (2, 250, 37, 224, 2000, "hi"),
    (2, 251, 37, 224, 2016, "hi"),
    # B = 1, cout_pad = 128: w22 = 4 * ceil(Hout / 2) reaches 1000 exactly, with 996 / 1004 and 1996 / 2004 beside the thresholds
    (1, 498, 37, 128, 996, "lo"),
    (1, 499, 37, 128, 1000, "mid"),
    (1, 500, 37, 128, 1000, "mid"),
    (1, 501, 37, 128, 1004, "mid"),
    (1, 998, 37, 128, 1996, "mid"),
    (1, 999, 37, 128, 2000, "hi"),
    (1, 1001, 37, 128, 2004, "hi"),
    # every factor counts: from (2, 250, 37, 224) = 2000, one factor changed at a time
    (1, 250, 37, 224, 1000, "mid"),       # B
    (3, 250, 37, 128, 1500, "mid"),
    (4, 250, 37, 128, 2000, "hi"),
    (2, 250, 37, 128, 1000, "mid"),       # channel groups: 128 -> 1, 160 .. 256 -> 2, 288 -> 3
    (2, 250, 37, 160, 2000, "hi"),
    (2, 250, 37, 256, 2000, "hi"),
    (1, 250, 37, 288, 1500, "mid"),
    (2, 250, 32, 224, 1000, "mid"),       # tile columns: 32 -> 1, 33 -> 2, 65 -> 3
    (2, 250, 33, 224, 2000, "hi"),
    (2, 82, 65, 224, 984, "lo"),
    (2, 84, 65, 224, 1008, "mid"),
    (1, 2, 1, 32, 2, "lo"),
]


def query(B, Hin, Win, cout_pad, ks, stride):
    th, nt, wr = ctypes.c_int(-7), ctypes.c_int(-8), ctypes.c_int(-9)
    rc = hip.load().ophip_conv_tile_shape(B, Hin, Win, cout_pad, ks, stride, ctypes.byref(th), ctypes.byref(nt), ctypes.byref(wr))
    return rc, (th.value, nt.value, wr.value)


@pytest.mark.parametrize("ks,stride", sorted(EXPECT))
def test_tile_shape_on_both_sides_of_each_threshold(ks, stride):
    for B, Hout, Wout, cout_pad, w22, band in ROWS:
        # input sizes that give this output size: stride 1 keeps it (padding ks / 2); stride 2 maps 2 n - 1 and 2 n to n
        sizes = [(Hout, Wout)] if stride == 1 else [(2 * Hout - 1, 2 * Wout - 1), (2 * Hout, 2 * Wout)]
        for Hin, Win in sizes:
            rc, shape = query(B, Hin, Win, cout_pad, ks, stride)
            assert rc == 0
            assert shape == EXPECT[(ks, stride)][band], f"B {B}, {Hin} x {Win} -> {Hout} x {Wout}, cout_pad {cout_pad}: w22 = {w22}"


@pytest.mark.parametrize("bad", [dict(ks=5), dict(stride=3), dict(cout_pad=48), dict(B=0), dict(ks=2), dict(stride=0), dict(cout_pad=0),
                                 dict(Hin=0), dict(Win=0)])
def test_bad_arguments_leave_the_outputs_untouched(bad):
    args = dict(B=2, Hin=251, Win=37, cout_pad=224, ks=3, stride=1)
    assert query(**args) == (0, (2, 2, 2))
    args.update(bad)
    assert query(**args) == (-1, (-7, -8, -9))
    with pytest.raises(ValueError):
        hip.call("ophip_conv_tile_shape", *args.values(), *(ctypes.byref(ctypes.c_int(0)) for _ in range(3)))


def test_null_outputs_are_refused():
    th = ctypes.c_int(-7)
    assert hip.load().ophip_conv_tile_shape(2, 251, 37, 224, 3, 1, ctypes.byref(th), None, None) == -1 and th.value == -7
