"""CPU: the evaluation cache's claim / resolve / fill kernels (csrc/raz_leaf_cache.hip) row by row on the wave emulator
(tests/native/libraz_emu.so), through raz_leaf_cache_probe on host arrays.  Cases and assertions: tests/leaf_cache_cases.py, the
same that tests/test_leaf_cache_gpu.py runs on the device - tag collisions with different keys, full and wrapping probe windows, the
disc threshold, slice shapes around the kernels' block sizes, unfinished claims, owners in another slice, a re-attached table, the
entry's refusals.  Every comparison is of bits or integers."""
import pytest

import emu_util
import leaf_cache_cases as C


@pytest.fixture(scope="module")
def emu():
    return emu_util.load()


@pytest.fixture(scope="module")
def run(emu):
    def run(rig, calls, **ov):
        ptr = {"cache": rig.buf.ctypes.data, "own": rig.own.ctypes.data, "enemy": rig.enemy.ctypes.data, "active": rig.active.ctypes.data,
               "policy": rig.policy.ctypes.data, "value": rig.value.ctypes.data}
        return [emu.raz_leaf_cache_probe(*C.call_args(rig, ptr, call, ov), None) for call in calls]
    return run


def test_the_restated_layout_is_the_tables(emu):
    C.check_layout(emu.raz_leaf_cache_bytes)


def test_builders_find_what_they_look_for():
    (ao, ae), (bo, be) = C.collisions()
    assert len(ao) >= 8
    assert (C.leaf_tag(ao, ae) == C.leaf_tag(bo, be)).all() and not (bo & be).any()
    for h in (0, 100, 1016, 1020, 1023):
        o, e = C.at_home(h, 12)
        assert (C.home_slot(C.leaf_tag(o, e), 10) == h).all() and len(set(zip(o.tolist(), e.tolist()))) == 12
    w = C.net(ao, ae)
    assert w.shape == (len(ao), 65) and len(set(w.ravel().tolist())) == w.size       # no number twice
    assert (((w >> 23) & 0xff) != 0xff).all() and (((w >> 23) & 0xff) != 0).all()      # finite


@pytest.mark.parametrize("case", list(C.CASES))
def test_leaf_cache_rows(run, case):
    C.CASES[case](run)
