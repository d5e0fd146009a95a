"""GPU: raznet-forward-v2 and v3 at the edges of the trunk kernel's 4-position groups (tests/net_f16x3_groups_cases.py has the cases
and their reasons), against the SAME recording as tests/test_net_f16x3_bits_gpu.py (tests/golden/f16x3_bits.npz): an answer depends
on the row's position alone, so rows 0 .. n - 1 of the table pv_<net>_<ver> are the expected bits at every count and mask.  And the
trunk's own range flag: a position that leaves the f16 range inside the first residual convolution is repaired alone, whichever
place of a wave's group it stands at."""
import os

import numpy as np
import pytest

import net_f16x3_bits_cases as C
import net_f16x3_groups_cases as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16x3_bits.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files if k.startswith("pv_")}


@pytest.fixture(scope="module")
def boards():
    return C.positions()


_NETS = {}


def _net(shape, kernel):
    from reversi_alpha_zero_amd.engine import DeviceNet
    if (shape, kernel) not in _NETS:
        _NETS[shape, kernel] = DeviceNet(C.blob(shape), C.DEV, kernel=kernel)
    return _NETS[shape, kernel]


def _pv(dn, own, enemy, active=None):
    p, v = C.forward(dn, own, enemy, active)
    return np.concatenate([p, v[:, None]], axis=1)


def _differing(got, want):
    return np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)).tolist()


@pytest.mark.parametrize("n", G.COUNTS)
@pytest.mark.parametrize("ver", list(C.VERSIONS))
@pytest.mark.parametrize("shape", C.NETS, ids=C.key)
def test_rows_keep_their_bits_at_the_edges_of_a_group(gold, boards, shape, ver, n):
    own, enemy = boards
    want = gold[f"pv_{C.key(shape)}_{ver}"][:n]
    dn = _net(shape, C.VERSIONS[ver])
    got = _pv(dn, own[:n], enemy[:n])
    assert np.array_equal(got, want), f"plain: rows {_differing(got, want)[:8]} differ from the recording"
    for name in G.MASKS:
        a = G.mask(name, n)
        got = _pv(dn, own[:n], enemy[:n], a)
        on = a != 0
        assert np.array_equal(got[on], want[on]), f"{name}: rows {np.flatnonzero(on)[_differing(got[on], want[on])][:8].tolist()} differ"
        assert not got[~on].any(), f"{name}: a row the mask switched off was written"
    assert dn.range_ok()


@pytest.mark.parametrize("place", G.RANGE_PLACES)
@pytest.mark.parametrize("ver", list(C.VERSIONS))
def test_a_row_that_leaves_the_range_inside_the_trunk_is_repaired_alone(ver, place):
    from reversi_alpha_zero_amd.engine import DeviceNet
    F, _, V = G.RANGE_SHAPE
    blob = G.net_that_overflows_in_the_trunk(F, V)
    own, enemy, crowded = G.range_boards(place)
    others = np.arange(len(own)) != crowded
    dn = DeviceNet(blob, C.DEV, kernel=C.VERSIONS[ver])
    alone = _pv(dn, own[others], enemy[others])
    assert dn.range_stats() == (True, 0), "the sparse boards alone left the range: the case does not isolate the crowded row"
    got = _pv(dn, own, enemy)
    exact = _pv(DeviceNet(blob, C.DEV, kernel="f32"), own[crowded:crowded + 1], enemy[crowded:crowded + 1])
    assert np.array_equal(got[crowded], exact[0]), "the crowded row is not raznet-forward-v1's"
    assert np.array_equal(got[others], alone), f"rows {np.flatnonzero(others)[_differing(got[others], alone)].tolist()} changed beside the crowded row"
    assert dn.range_stats() == (True, 1)
