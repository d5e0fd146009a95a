"""GPU: the bits of raznet-forward-v2 (split-f16 trunk) and v3 (plain f16), pinned to a recording (tests/golden/f16x3_bits.npz,
written by tests/golden/make_golden_f16x3_bits.py on an MI355X at the commit before the trunk's epilogue, the first-layer kernel and
the leaf cache's resolve kernel were rewritten for speed).  Those rewrites move data differently - a lane of the trunk kernel owns
the 8 channels of one square instead of 4 channels of two, the first layer computes two rows per lane, the compact list is built by
workgroups - and must not move a bit: every output element still goes through the same operations in the same order.  The cases and
their reasons are in tests/net_f16x3_bits_cases.py.  A split `fma`, a contracted multiply-add or another rounding of a conversion
changes low bits of most rows, and the equalities below fail: checked once with a library whose trunk file was compiled with
contraction allowed (the product build forbids it, so the epilogue's multiply-add is two operations) - all 42 cases failed
(profiles/r8/pytest_bits_test_on_a_contracted_trunk_library.log).  In the compacted cases the evaluated rows stay below the rows the
games asked for (8 steps of 63 games: 127 evaluated of 504) except with a single game, whose 8 leaves are all new positions."""
import os

import numpy as np
import pytest

import net_f16x3_bits_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16x3_bits.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def boards():
    return C.positions()


_NETS = {}


def _net(shape, kernel):
    from reversi_alpha_zero_amd.engine import DeviceNet
    if (shape, kernel) not in _NETS:
        _NETS[shape, kernel] = DeviceNet(C.blob(shape), C.DEV, kernel=kernel)
    return _NETS[shape, kernel]


def _differing(got, want):
    return np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)).tolist()


@pytest.mark.parametrize("n", C.COUNTS)
@pytest.mark.parametrize("ver", list(C.VERSIONS))
@pytest.mark.parametrize("shape", C.NETS, ids=C.key)
def test_rows_keep_their_bits_plain_and_masked(gold, boards, shape, ver, n):
    own, enemy = boards
    want = gold[f"pv_{C.key(shape)}_{ver}"][:n]
    dn = _net(shape, C.VERSIONS[ver])
    p, v = C.forward(dn, own[:n], enemy[:n])
    got = np.concatenate([p, v[:, None]], axis=1)
    assert np.array_equal(got, want), f"plain: rows {_differing(got, want)[:8]} differ from the recording"
    a = C.mask(n)
    p, v = C.forward(dn, own[:n], enemy[:n], a)
    got = np.concatenate([p, v[:, None]], axis=1)
    on = a != 0
    assert np.array_equal(got[on], want[on]), f"masked: rows {np.flatnonzero(on)[_differing(got[on], want[on])][:8].tolist()} differ"
    assert not got[~on].any(), "a row the mask switched off was written"
    assert dn.range_ok()


@pytest.mark.parametrize("n", C.COUNTS)
@pytest.mark.parametrize("shape", C.NETS, ids=C.key)
def test_rows_keep_their_bits_through_the_compacted_forward(gold, shape, n):
    want = gold[f"compact_{C.key(shape)}_{n}"]
    dn = _net(shape, "f16x3")
    got, st = C.compacted(dn, n)
    total = st["hits"] + st["in_batch_duplicates"] + st["evaluated"]
    assert n == 1 or st["evaluated"] < total, st   # the device-side count was below the games' rows: surplus workgroups exited
    for t in range(C.STEPS):
        assert np.array_equal(got[t, :, :2], want[t, :, :2]), f"step {t}: the games asked for other positions than in the recording"
        assert np.array_equal(got[t, :, 2:], want[t, :, 2:]), f"step {t}: rows {_differing(got[t, :, 2:], want[t, :, 2:])[:8]} hold other answers"
    assert dn.range_ok()
