"""CPU: the scenario of tests/test_leaf_resolve_blocks_gpu.py on the wave emulator (tests/native/libraz_emu.so): k_leaf_resolve's
ballots, its prefix over four waves and its two barriers, on slices around the 256-row workgroup."""
import pytest

import emu_util
import leaf_cache_cases as C
import leaf_resolve_blocks_cases as B


@pytest.fixture(scope="module")
def run():
    emu = emu_util.load()

    def run(rig, calls, **ov):
        ptr = {"cache": rig.buf.ctypes.data, "own": rig.own.ctypes.data, "enemy": rig.enemy.ctypes.data, "active": rig.active.ctypes.data,
               "policy": rig.policy.ctypes.data, "value": rig.value.ctypes.data}
        return [emu.raz_leaf_cache_probe(*C.call_args(rig, ptr, call, ov), None) for call in calls]
    return run


@pytest.mark.parametrize("p0", B.P0S)
@pytest.mark.parametrize("pn", B.PNS)
def test_resolve_by_workgroups(run, pn, p0):
    B.scenario(run, pn, p0)
