"""Cases of tests/test_net_f16x3_groups_gpu.py and tests/test_net_f16x3_groups_emu.py: the split-f16 trunk kernel
(csrc/raz_net_f16x3.hip k_conv3x3_f16x3) at the edges of a wave's tile.  A workgroup takes 8 positions; a wave computes one board-row
half of FOUR of them (positions 0-3 or 4-7 of the workgroup), so whether a lane computes, stores and raises the range flag is
decided per lane by its own position, and a wave leaves early only when none of its four positions is live.
tests/net_f16x3_bits_cases.py covers the edges of the 8-position workgroup (1, 7, 8, 9, 63, 64, 65 rows, rows 0 and n - 1 masked);
these are the edges of the 4-position group inside it.

Nets and versions: net_f16x3_bits_cases.NETS and VERSIONS.  Rows: 3, 4, 5 (a group partly filled, exactly filled, one row into the
second group) and 11, 12, 13 (the same in a second workgroup).  Masks:
  rows_1_2_off   two lanes' positions inside a group dead, their neighbours live
  group_off      one whole 4-position group dead: the second group of the first workgroup when there are more than 8 rows (its
                 waves leave early beside live ones), else the first group (3 and 4 rows: nothing is live at all; 5 rows: row 4 alone)
  alternate_off  every odd row dead: two live positions in every group, at the places where the LDS image alternates

An answer is a function of the row's position alone, so the expected bits are rows of ONE table per (net, version): on the GPU the
recording tests/golden/f16x3_bits.npz (table pv_<net>_<ver>, the first 65 of net_f16x3_bits_cases.positions()), on the emulator
the plain forward of those 65 rows.

The range case: a net whose stem stays inside the f16 range on every board and whose FIRST RESIDUAL CONVOLUTION leaves it on a
crowded board - the flag the trunk kernel itself raises, per position.  One crowded board stands at each of the four places of a
group in turn among sparse boards."""
import numpy as np

COUNTS = (3, 4, 5, 11, 12, 13)
MASKS = ("rows_1_2_off", "group_off", "alternate_off")
RANGE_SHAPE = (128, 1, 16)
RANGE_ROWS = 8
RANGE_PLACES = (0, 1, 2, 3)


def mask(name, n):
    a = np.ones(n, np.uint8)
    if name == "rows_1_2_off":
        a[1:3] = 0
    elif name == "group_off":
        if n > 8:
            a[4:8] = 0
        else:
            a[0:4] = 0
    elif name == "alternate_off":
        a[1::2] = 0
    else:
        raise ValueError(name)
    return a


def net_that_overflows_in_the_trunk(F, V):
    """Stem weights all 1 and bias 0: a stem activation is the number of discs in the square's 3x3 neighbourhood, at most 9.  First
    residual convolution: all weights w = 1.2e5 / (81 F), bias 0, so an output is w x F x (the stem activations in ITS 3x3
    neighbourhood).  On a full board an inner square sums 9 x 9: 1.2e5, beyond 60000.  A disc adds 1 to the stem activation of at most 9
    squares, so a board of two discs stays below 18 F w = 2.7e4.  The second convolution is scaled down (x 1e-7), so the block's
    output is the stem's again."""
    import torch
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    net = ReversiNet(F, 1, V).keras_init_(6)
    with torch.no_grad():
        net.stem.conv.weight.fill_(1.0)
        net.stem.conv.bias.zero_()
        net.res[0][0].conv.weight.fill_(1.2e5 / (81.0 * F))
        net.res[0][0].conv.bias.zero_()
        net.res[0][1].conv.weight.mul_(1.0e-7)
    return net.to_blob()


def range_boards(place):
    """(own, enemy, index of the crowded row): RANGE_ROWS - 1 boards of two discs and one full board at row `place`."""
    rng = np.random.default_rng(11)
    own = np.array([1 << int(rng.integers(0, 64)) for _ in range(RANGE_ROWS)], dtype=np.uint64)
    enemy = np.array([(1 << int(rng.integers(0, 64))) & ~int(o) for o in own], dtype=np.uint64)
    full = rng.integers(0, 2**64, dtype=np.uint64)
    own[place], enemy[place] = full, ~full
    return own, enemy, place
