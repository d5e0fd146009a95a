"""CPU: raznet-forward-v3, the plain-f16 trunk (raz_net.reserved = 8; csrc/raz_net_f16x3.hip with SPLIT = false), on EMULATED matrix
cores (tests/native/wave_emu, the net library of tests/test_net_emu.py), and its host side: raz_net_form, DeviceNet's mapping, the
worker's replay rule.  The cases and their reasoning are in tests/net_f16_cases.py; tests/test_net_f16_gpu.py is the test of
record.  On the integer nets the emulation's own summation order inside a matrix instruction does not matter (integer sums are
exact in any order), so here too the comparison is bit for bit."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import net_cases as C
import net_f16_cases as K
import oracle as O
from conftest import ROOT, _locked

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_net.so")


@pytest.fixture(scope="module")
def lib():
    with _locked("emu"):
        r = subprocess.run(["make", "-C", EMU_DIR, "../libraz_emu_net.so"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from reversi_alpha_zero_amd import _native as N
    lib = ctypes.CDLL(LIB)
    lib.raz_last_error.restype = ctypes.c_char_p
    for name in ("raz_net_weight_bytes", "raz_net_scratch_bytes", "raz_net_load", "raz_net_forward", "raz_net_range_stats", "raz_net_form"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    return lib


class EmuNet:
    """A loaded net on the emulator library; the scratch arrives filled with NaN halfs (0xFF bytes), as uninitialised as memory
    gets: v3 may read none of the lo planes it never writes."""

    def __init__(self, lib, blob, reserved=K.RESERVED):
        from reversi_alpha_zero_amd import _native as N
        self.lib = lib
        _, _, self.F, self.R, self.V = struct.unpack_from("<5i", blob, 0)
        self.w = np.zeros(lib.raz_net_weight_bytes(self.F, self.R, self.V), dtype=np.uint8)
        self.net = N.RazNet()
        self.net.reserved = reserved
        assert lib.raz_net_load(ctypes.byref(self.net), blob, len(blob), self.w.ctypes.data, self.w.size, None) == 0, lib.raz_last_error()

    def forward(self, own, enemy, active=None):
        n = len(own)
        own, enemy = np.ascontiguousarray(own), np.ascontiguousarray(enemy)
        need = self.lib.raz_net_scratch_bytes(self.F, self.V, n)
        scratch = np.full(max(need, 8), 0xFF, dtype=np.uint8)
        pol, val = np.full((n, 64), 7.0, np.float32), np.full(n, 7.0, np.float32)
        rc = self.lib.raz_net_forward(ctypes.byref(self.net), own.ctypes.data, enemy.ctypes.data, active.ctypes.data if active is not None else None,
                                      pol.ctypes.data, val.ctypes.data, n, scratch.ctypes.data if need else None, need, None)
        assert rc == 0, self.lib.raz_last_error()
        return pol, val

    def range_stats(self):
        over, rows = ctypes.c_int(0), ctypes.c_ulonglong(0)
        assert self.lib.raz_net_range_stats(ctypes.byref(self.net), ctypes.byref(over), ctypes.byref(rows), None) == 0, self.lib.raz_last_error()
        return not over.value, int(rows.value)


def _oracle(blob, own, enemy):
    o = O.load_ext()
    pol, val = np.zeros((len(own), 64), np.float32), np.zeros(len(own), np.float32)
    for i in range(len(own)):
        v = np.zeros(1, np.float32)
        assert o.orc_net_forward(blob, len(blob), int(own[i]), int(enemy[i]), pol[i].ctypes.data, v.ctypes.data) == 0
        val[i] = v[0]
    return pol, val


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape,n", [((128, 2, 64), 3), ((128, 2, 64), 11), ((256, 1, 16), 3)], ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_emulated_plain_f16_trunk_equals_the_oracle_bit_for_bit_on_integer_nets(lib, shape, n):
    """The test that carries the kernel (net_f16_cases.integer_net: nothing in v3 rounds on such a net): k_conv0_split<false> +
    k_conv3x3_f16x3<false> (12 of a stage's 24 weight pieces and the two hi planes by LDS-DMA, one matrix instruction per tile,
    the skip's and the output's hi plane alone) + k_heads_split<false> == the C oracle on every active row, policy and value, on a
    partly filled position group (3), a second group (11) and two output-channel tiles per group (F = 256); rows the `active` mask
    skips stay untouched, the range flag stays clear, and a row alone equals the row inside the batch."""
    blob, maxima = K.integer_net(*shape)
    print(f"{shape}: layer maxima {maxima}")
    own, enemy = K.positions(n)
    active = (np.arange(n) % 5 != 1).astype(np.uint8)
    net = EmuNet(lib, blob)
    assert lib.raz_net_form(ctypes.byref(net.net), n) == 8
    pol, val = net.forward(own, enemy, active)
    on = active.astype(bool)
    rp, rv = _oracle(blob, own[on], enemy[on])
    assert np.array_equal(_bits(pol[on]), _bits(rp)) and np.array_equal(_bits(val[on]), _bits(rv))
    assert (pol[~on] == 7.0).all() and (val[~on] == 7.0).all()
    i = n - 1
    pa, va = net.forward(own[i:i + 1], enemy[i:i + 1])
    assert np.array_equal(_bits(pa[0]), _bits(pol[i])) and _bits(va)[0] == _bits(val)[i]
    assert net.range_stats() == (True, 0)


def _sharp_rows():
    own, enemy, names = C.inputs(n_random=3)
    rows = [0, 1, 2, names.index("empty"), names.index("full"), names.index("own@0"), names.index("enemy@63"),
            names.index("own@7"), names.index("overlap all"), len(names) - 1]
    return own[rows], enemy[rows]


def test_emulated_plain_f16_trunk_error_is_the_quantisations_and_no_more(lib):
    """On a sharp float net (128, 1, 64) over the edge boards tests/test_net_emu.py runs: the kernel's distance E_k from the f64
    graph against E_q, the distance of the f64 restatement of v3's specification from the same graph
    (net_f16_cases.quantised_reference): E_k <= (4, 2.5) x E_q on (max, mean), and E_k[mean] > 1e-5 - single products, not v2."""
    F, R, V = 128, 1, 64
    own, enemy = _sharp_rows()
    net = C.sharp_net(F, R, V, F + R, own, enemy)
    rp, rv = C.reference(net, own, enemy)
    C.assert_sharp(rp, rv, "128x1")
    e_q = C.errors(*K.quantised_reference(net, own, enemy), rp, rv)
    en = EmuNet(lib, net.to_blob())
    pol, val = en.forward(own, enemy)
    e_k = C.errors(pol, val, rp, rv)
    print(f"(128, 1, 64) emulated v3: E_k max {e_k[0]:.3g} mean {e_k[1]:.3g}; E_q max {e_q[0]:.3g} mean {e_q[1]:.3g}")
    assert np.isfinite(pol).all() and np.isfinite(val).all()
    assert K.within_quantisation_rule(e_k, e_q), (e_k, e_q)
    assert e_k[1] > K.MIN_MEAN_ERROR, e_k
    assert en.range_stats() == (True, 0)


def test_emulated_plain_f16_rows_out_of_range_are_repaired_or_flagged(lib):
    """tests/test_engine_gpu.py test_net_f16x3_range_flag's construction (the stem x 1e6: every row leaves the f16 range) with
    reserved 8: 8 rows are all evaluated by the exact-f32 chains inside the forward - the oracle, bit for bit, range_stats ==
    (True, 8); 40 rows in one forward raise the sticky flag (and are still answered exactly)."""
    blob = K.net_that_overflows(128, 1, 64)
    for n, in_range in ((8, True), (40, False)):
        own, enemy = K.harvested_positions(n, 2)
        net = EmuNet(lib, blob)
        assert net.range_stats() == (True, 0)
        pol, val = net.forward(own, enemy)
        rp, rv = _oracle(blob, own, enemy)
        assert np.array_equal(_bits(pol), _bits(rp)) and np.array_equal(_bits(val), _bits(rv))
        assert net.range_stats() == (in_range, n)


# ---- host side: no device work -------------------------------------------------------------------------------------------------

def test_net_form_over_reserved_8():
    """raz_net_form's table for raznet-forward-v3 (include/raz.h): the f16x3 shapes, split by the in-forward repair as for reserved 4;
    a shape k_net_mfma takes answers as for 4; any other filters is refused; 3 and 16 stay refused and the text names 8."""
    from reversi_alpha_zero_amd import _native as N

    def form(F, V, reserved):
        net = N.RazNet(filters=F, res_layers=1, value_fc=V, reserved=reserved)
        return N.lib.raz_net_form(ctypes.byref(net), 1)
    assert [form(F, V, 8) for (F, V), _ in K.FORM_TABLE] == [f for _, f in K.FORM_TABLE]
    assert form(192, 7, 8) == -1 and "128" in N.last_error()
    for r in (3, 16):
        assert form(128, 64, r) == -1 and "0, 1, 2, 4 or 8" in N.last_error()
    assert [form(128, 64, 4), form(384, 1, 4), form(128, 64, 0)] == [6, 7, 5]   # the other forms keep their answers


def test_device_net_maps_f16_to_reserved_8(monkeypatch):
    """DeviceNet(kernel="f16") -> raz_net.reserved 8, FORMS names 8 / 9, a kernel_name bench.py does not take for the 1e-5 form, and
    "auto" still the split-f16 trunk.  (raz_net_load is stubbed: the mapping is host code.)"""
    import contextlib
    import torch
    from reversi_alpha_zero_amd import engine as E
    from reversi_alpha_zero_amd.agent.model import blob_float_count

    def load(netref, blob, nbytes, dptr, dbytes, stream):
        _, _, netref._obj.filters, netref._obj.res_layers, netref._obj.value_fc = struct.unpack_from("<5i", blob, 0)
        return 0
    monkeypatch.setattr(E.lib, "raz_net_load", load)
    monkeypatch.setattr(E, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    assert E.FORMS[8] == "f16_repair" and E.FORMS[9] == "f16_no_repair"
    for (F, V), want in (((128, 64), "f16_repair"), ((384, 16), "f16_no_repair")):
        blob = struct.pack("<8i", 0x4E5A4152, 1, F, 1, V, 3, 0, 0) + bytes(4 * blob_float_count(F, 1, V))
        dn = E.DeviceNet(blob, "cpu", kernel="f16")
        assert dn.c.reserved == 8 and dn.form(1) == want
        assert "f16x3" not in dn.kernel_name and "raznet-forward-v3" in dn.kernel_name
        auto = E.DeviceNet(blob, "cpu", kernel="auto")
        assert auto.c.reserved == 4 and "f16x3" in auto.kernel_name


def test_worker_may_replay_a_block_played_on_the_plain_f16_trunk():
    """worker/self_play.py: net_kernel="f16" passes through, and a block whose forward raised the sticky range flag is replayed on
    the exact-f32 kernels as for "f16x3" (_may_replay_block)."""
    from reversi_alpha_zero_amd.agent.model import blob_float_count
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.worker.self_play import BatchedSelfPlayWorker
    wide = struct.pack("<8i", 0x4E5A4152, 1, 256, 1, 16, 3, 0, 0)
    narrow = struct.pack("<8i", 0x4E5A4152, 1, 16, 1, 16, 3, 0, 0)
    w = BatchedSelfPlayWorker(Config(), wide, games_in_flight=8, net_kernel="f16")
    assert w.net_kernel == "f16" and w._may_replay_block()
    assert not BatchedSelfPlayWorker(Config(), narrow, games_in_flight=8, net_kernel="f16")._may_replay_block()
    assert not BatchedSelfPlayWorker(Config(), wide, games_in_flight=8, net_kernel="f32")._may_replay_block()
    w._f32_fallback = True
    assert not w._may_replay_block()
