"""CPU: the loops of the batched sweep kernels (csrc/raz_sweep.hip, raz_sweep_sliced.h) taking several trips, on the wave emulator -
the cases of tests/sweep_cases.py, which tests/test_sweep_loops_gpu.py runs on the device.  In this process the seven entries run at
the default grid on the edge sizes and on N_LOOP = 5 * 2048 + 307 boards against references of their own (one trip per loop: plain
size checks); the test at the end runs the file again in five children, one per configuration of sweep_cases.CONFIGS, where
RAZ_SWEEP_MAXGRID caps the grids at 2 or 1 workgroups and every kernel's loop takes at least three trips - which each child proves
from raz_sweep_max_grid and raz_sweep_forms before it compares anything.  (A child takes some seconds here, all of N_LOOP boards.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_cases as C
from emu_util import EMU_LIB, load

CONFIG = os.environ.get("RAZ_SWEEP_LOOPS_CHILD") or None


def _library_of_its_own():
    """The emulator library (built by emu_util.load) loaded once more from a copy: the sweep entries read their variables once per
    LIBRARY, and emu_util's instance is shared with tests/test_sweep_emu.py, which may run in this process before or after this
    file with variables of its own - what is fixed here must not reach it, nor the other way round."""
    import shutil
    import tempfile
    from reversi_alpha_zero_amd import _native as N
    load()
    with tempfile.TemporaryDirectory() as d:
        lib = ctypes.CDLL(shutil.copy(EMU_LIB, os.path.join(d, "libraz_emu_sweep_loops.so")))
    lib.raz_last_error.restype = ctypes.c_char_p
    for name in ("raz_legal_moves_batch", "raz_calc_flip_batch", "raz_step_batch", "raz_score_batch", "raz_d4_batch", "raz_planes_batch",
                 "raz_pick_kth_legal_batch", "raz_sweep_forms", "raz_sweep_max_grid"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    return lib


class EmuDriver:
    """sweep_cases' driver on the emulator's C ABI: host arrays, stream NULL."""
    allocates = ()

    def __init__(self):
        self.lib = _library_of_its_own()

    @staticmethod
    def _put(a, off=0, fill=None):
        """A copy of `a` (or, with fill, an array like it full of that byte) `off` bytes behind a 256-byte boundary."""
        a = np.ascontiguousarray(a)
        buf = np.zeros(a.nbytes + 512, dtype=np.uint8)
        start = (-buf.ctypes.data) % 256 + off
        v = buf[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
        if fill is None:
            v[...] = a
        else:
            v.view(np.uint8)[...] = fill
        assert a.size == 0 or v.ctypes.data % 256 == off    # (an empty view's address is anybody's)
        return v

    def _blank(self, dtype, shape, off=0):
        return self._put(np.zeros(shape, dtype=dtype), off, fill=C.SENTINEL)

    def _run(self, name, args, n, outputs):
        rc = getattr(self.lib, name)(*[a.ctypes.data for a in args], n, None)
        if rc != 0:
            raise C.Refused(rc, (self.lib.raz_last_error() or b"").decode(), outputs)
        return tuple(outputs.values())

    def legal_moves(self, own, enemy, offsets={}):
        o, e, l = self._put(own, offsets.get("own", 0)), self._put(enemy, offsets.get("enemy", 0)), self._blank(np.uint64, len(own), offsets.get("legal", 0))
        return self._run("raz_legal_moves_batch", (o, e, l), len(own), {"legal": l})

    def calc_flip(self, pos, own, enemy, offsets={}):
        p, o, e = self._put(pos, offsets.get("pos", 0)), self._put(own, offsets.get("own", 0)), self._put(enemy, offsets.get("enemy", 0))
        f = self._blank(np.uint64, len(own), offsets.get("flipped", 0))
        return self._run("raz_calc_flip_batch", (p, o, e, f), len(own), {"flipped": f})

    def step(self, black, white, player, status, action, offsets={}):
        b, w, p, s = (self._put(a, offsets.get(k, 0)) for k, a in (("black", black), ("white", white), ("player", player), ("status", status)))
        l, a = self._blank(np.uint64, len(black), offsets.get("legal", 0)), self._put(action, offsets.get("action", 0))
        return self._run("raz_step_batch", (b, w, p, s, l, a), len(black), {"black": b, "white": w, "player": p, "status": s, "legal": l})

    def score(self, black, white, offsets={}):
        b, w = self._put(black, offsets.get("black", 0)), self._put(white, offsets.get("white", 0))
        win, d = self._blank(np.uint8, len(black), offsets.get("winner", 0)), self._blank(np.int8, len(black), offsets.get("diff", 0))
        return self._run("raz_score_batch", (b, w, win, d), len(black), {"winner": win, "diff": d})

    def d4(self, x, sym, offsets={}):
        i, o, s = self._put(x, offsets.get("x", 0)), self._blank(np.uint64, len(x), offsets.get("out", 0)), self._put(sym, offsets.get("sym", 0))
        return self._run("raz_d4_batch", (i, o, s), len(x), {"out": o})

    def planes(self, own, enemy, offsets={}):
        o, e, p = self._put(own), self._put(enemy), self._blank(np.float32, (len(own), 128))
        return self._run("raz_planes_batch", (o, e, p), len(own), {"planes": p})

    def pick_kth(self, legal, rnd, offsets={}):
        l, r, a = self._put(legal), self._put(rnd), self._blank(np.uint8, len(legal))
        return self._run("raz_pick_kth_legal_batch", (l, r, a), len(legal), {"action": a})

    def forms(self, n):
        lf, sf = ctypes.c_int(-1), ctypes.c_int(-1)
        assert self.lib.raz_sweep_forms(n, ctypes.addressof(lf), ctypes.addressof(sf)) == 0
        return lf.value, sf.value

    def max_grid(self):
        return int(self.lib.raz_sweep_max_grid())


@pytest.fixture(scope="module")
def drv():
    return EmuDriver()


def test_emulated_configuration_is_in_force_and_the_loops_iterate(drv):
    """First in the file: what a child runs before anything else."""
    C.check_configuration(drv, CONFIG)
    t = C.check_iterations(drv, CONFIG)
    print(f"\ntrips[{CONFIG}] " + " ".join(f"{k}={v[0]}/{v[1]}" for k, v in sorted(t.items())))


def test_the_cases_check_themselves():
    C.self_check()


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("entry", C.ENTRIES)
def test_emulated_entry_equals_its_reference(drv, entry, n):
    C.check_entry(drv, entry, n, CONFIG)


def test_emulated_misaligned_arrays_are_refused_and_nothing_is_written(drv):
    assert C.check_refusals(drv) == len(C.REFUSALS)


def test_emulated_step_with_byte_arrays_4_bytes_off_equals_the_aligned_call(drv):
    """(In configurations c and e: the hybrid form's demotion to k_step, whose pipeline then walks all 41 blocks.)"""
    C.check_step_with_bytes_4_off(drv)


@pytest.mark.parametrize("config", sorted(C.CONFIGS))
def test_emulated_loops_iterate_in_a_process_of_their_own(config):
    """The file again in a child with the configuration's variables (read once per process) and no other RAZ_SWEEP_* variable."""
    if CONFIG:
        pytest.skip("a child of this test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RAZ_SWEEP_")}
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-p", "no:cacheprovider", "-p", "no:xdist",
                        "-k", "not in_a_process_of_their_own"],
                       env={**env, **C.CONFIGS[config]["env"], "RAZ_SWEEP_LOOPS_CHILD": config}, capture_output=True, text=True, timeout=900,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and f"trips[{config}]" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
