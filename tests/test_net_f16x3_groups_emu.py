"""CPU: the cases of tests/net_f16x3_groups_cases.py on EMULATED matrix cores (tests/native/wave_emu, the net library of
tests/test_net_emu.py).  The GPU recording does not apply here - the emulation fixes its own summation order inside a matrix
instruction - so the rule is: a row's bits at any count and mask equal that row's bits in the plain forward of all 65 rows.  Both
sides are the code under test: this proves that a row's answer does not depend on its group, its neighbours or the mask, and that
dead rows stay unwritten; that the answers are RIGHT is tests/test_net_emu.py's tolerance against the oracle.  The range case holds
bit for bit here as well: the exact-f32 chains (raznet-forward-v1) are exact on the emulator.

Cost: the emulation runs a workgroup of the trunk kernel in about a second per layer and output-channel tile, so the 65-row table
of the (256, 2, 16) net alone takes 1.5 min for v2 (0.5 min for v3), and a case of four forwards up to 1.5 min; the (128, 1, 16)
cases take seconds.  All cases together: about 25 min (measured once, in one process: 1,458 s)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import net_f16x3_bits_cases as C
import net_f16x3_groups_cases as G
from conftest import ROOT, _locked

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_net.so")
RESERVED = {"v2": 4, "v3": 8, "v1": 0}   # raz_net.reserved of each version (include/raz.h)


@pytest.fixture(scope="module")
def lib():
    with _locked("emu"):
        r = subprocess.run(["make", "-C", EMU_DIR, "../libraz_emu_net.so"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from reversi_alpha_zero_amd import _native as N
    lib = ctypes.CDLL(LIB)
    lib.raz_last_error.restype = ctypes.c_char_p
    for name in ("raz_net_weight_bytes", "raz_net_scratch_bytes", "raz_net_load", "raz_net_forward", "raz_net_range_stats"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    return lib


class EmuNet:
    def __init__(self, lib, blob, reserved):
        from reversi_alpha_zero_amd import _native as N
        self.lib = lib
        _, _, self.F, self.R, self.V = struct.unpack_from("<5i", blob, 0)
        self.w = np.zeros(lib.raz_net_weight_bytes(self.F, self.R, self.V), dtype=np.uint8)
        self.net = N.RazNet()
        self.net.reserved = reserved
        assert lib.raz_net_load(ctypes.byref(self.net), blob, len(blob), self.w.ctypes.data, self.w.size, None) == 0, lib.raz_last_error()

    def forward(self, own, enemy, active=None):
        """uint32 [n, 65]: the bits of a row's policy and value; rows the forward does not write read as zeros."""
        n = len(own)
        own, enemy = np.ascontiguousarray(own), np.ascontiguousarray(enemy)
        need = self.lib.raz_net_scratch_bytes(self.F, self.V, n)
        scratch = np.full(max(need, 8), 0xFF, dtype=np.uint8)   # NaN halfs: nothing may be read that was not written
        pol, val = np.zeros((n, 64), np.float32), np.zeros(n, np.float32)
        rc = self.lib.raz_net_forward(ctypes.byref(self.net), own.ctypes.data, enemy.ctypes.data, active.ctypes.data if active is not None else None,
                                      pol.ctypes.data, val.ctypes.data, n, scratch.ctypes.data if need else None, need, None)
        assert rc == 0, self.lib.raz_last_error()
        return np.concatenate([pol.view(np.uint32), val.view(np.uint32)[:, None]], axis=1)

    def range_stats(self):
        over, rows = ctypes.c_int(0), ctypes.c_ulonglong(0)
        assert self.lib.raz_net_range_stats(ctypes.byref(self.net), ctypes.byref(over), ctypes.byref(rows), None) == 0, self.lib.raz_last_error()
        return not over.value, int(rows.value)


@pytest.fixture(scope="module")
def boards():
    return C.positions()


_TABLES = {}


def _table(lib, boards, shape, ver):
    """(the loaded net, its plain forward of all 65 rows), computed once per (net, version)."""
    if (shape, ver) not in _TABLES:
        net = EmuNet(lib, C.blob(shape), RESERVED[ver])
        _TABLES[shape, ver] = net, net.forward(*boards)
    return _TABLES[shape, ver]


def _differing(got, want):
    return np.flatnonzero((got != want).any(axis=1)).tolist()


@pytest.mark.parametrize("n", G.COUNTS)
@pytest.mark.parametrize("ver", list(C.VERSIONS))
@pytest.mark.parametrize("shape", C.NETS, ids=C.key)
def test_emulated_rows_keep_their_bits_at_the_edges_of_a_group(lib, boards, shape, ver, n):
    own, enemy = boards
    net, table = _table(lib, boards, shape, ver)
    assert table.any(axis=1).all()
    want = table[:n]
    got = net.forward(own[:n], enemy[:n])
    assert np.array_equal(got, want), f"plain: rows {_differing(got, want)[:8]} differ from the 65-row forward"
    for name in G.MASKS:
        a = G.mask(name, n)
        got = net.forward(own[:n], enemy[:n], a)
        on = a != 0
        assert np.array_equal(got[on], want[on]), f"{name}: rows {np.flatnonzero(on)[_differing(got[on], want[on])][:8].tolist()} differ"
        assert not got[~on].any(), f"{name}: a row the mask switched off was written"
    assert net.range_stats() == (True, 0)


@pytest.mark.parametrize("place", G.RANGE_PLACES)
@pytest.mark.parametrize("ver", list(C.VERSIONS))
def test_emulated_row_that_leaves_the_range_inside_the_trunk_is_repaired_alone(lib, ver, place):
    F, _, V = G.RANGE_SHAPE
    blob = G.net_that_overflows_in_the_trunk(F, V)
    own, enemy, crowded = G.range_boards(place)
    others = np.arange(len(own)) != crowded
    net = EmuNet(lib, blob, RESERVED[ver])
    alone = net.forward(own[others], enemy[others])
    assert net.range_stats() == (True, 0), "the sparse boards alone left the range: the case does not isolate the crowded row"
    got = net.forward(own, enemy)
    exact = EmuNet(lib, blob, RESERVED["v1"]).forward(own[crowded:crowded + 1], enemy[crowded:crowded + 1])
    assert np.array_equal(got[crowded], exact[0]), "the crowded row is not raznet-forward-v1's"
    assert np.array_equal(got[others], alone), f"rows {np.flatnonzero(others)[_differing(got[others], alone)].tolist()} changed beside the crowded row"
    assert net.range_stats() == (True, 1)
