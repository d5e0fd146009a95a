"""GPU: k_leaf_resolve in 256-row workgroups (csrc/raz_leaf_cache.hip) - one reservation of the compact list per workgroup instead of
one per row - on slices around its block size with rows of every role; two parts share one table.  The scenario and what is asserted
are in tests/leaf_resolve_blocks_cases.py; the rig and its assertions are those of tests/test_leaf_cache_gpu.py."""
import numpy as np
import pytest

import leaf_cache_cases as C
import leaf_resolve_blocks_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


@pytest.fixture(scope="module")
def run():
    import torch
    from reversi_alpha_zero_amd import _native as N
    names = {"cache": "buf", "own": "own", "enemy": "enemy", "active": "active", "policy": "policy", "value": "value"}

    def run(rig, calls, **ov):
        t = {k: _dev(getattr(rig, a)) for k, a in names.items()}
        ptr = {k: v.data_ptr() for k, v in t.items()}
        assert ptr["cache"] % 256 == 0 and ptr["own"] % 8 == 0 and ptr["enemy"] % 8 == 0
        stream = N.current_stream_ptr()
        rcs = [N.lib.raz_leaf_cache_probe(*C.call_args(rig, ptr, call, ov), stream) for call in calls]
        torch.cuda.synchronize()
        for k, a in names.items():
            np.copyto(getattr(rig, a).view(np.uint8).reshape(-1), t[k].cpu().numpy())
        return rcs
    return run


@pytest.mark.parametrize("p0", B.P0S)
@pytest.mark.parametrize("pn", B.PNS)
def test_resolve_by_workgroups(run, pn, p0):
    B.scenario(run, pn, p0)
