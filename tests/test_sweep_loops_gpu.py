"""GPU: the loops of the batched sweep kernels (csrc/raz_sweep.hip, raz_sweep_sliced.h) taking several trips - the cases of
tests/sweep_cases.py through lib/bitboard.py's wrappers, as tests/test_sweep_loops_emu.py runs them on the wave emulator.  In this
process the seven entries run at the default grid on the edge sizes and on N_LOOP = 5 * 2048 + 307 boards against references of their
own - the direct device check of k_score, k_pick_kth, k_planes, k_d4 and k_calc_flip (pos up to 255, masks of 0 and 64 bits, rnd >=
2^31) at odd sizes; the test at the end runs the file again in five children, one per configuration of sweep_cases.CONFIGS, where
RAZ_SWEEP_MAXGRID caps the grids at 2 or 1 workgroups: k_legal_moves' and k_step's prefetch pipeline, the superblock loops of the
three sliced kernels (k_step_sliced's overlap fall-back followed by another superblock) and the grid-stride loops of the other five
kernels then take three trips and more, which each child proves from raz_sweep_max_grid and raz_sweep_forms before it compares
anything.  No test here hands an entry arrays of different lengths: lib/bitboard.py refuses those on the host
(tests/test_bitboard_wrappers_host.py), and such a call must never reach a device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIG = os.environ.get("RAZ_SWEEP_LOOPS_CHILD") or None
_TORCH_VIEW = {np.dtype(np.uint64): torch.int64, np.dtype(np.uint32): torch.int32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int8): torch.int8}
_NUMPY_VIEW = {torch.int64: np.uint64, torch.int32: np.uint32}


class DeviceDriver:
    """sweep_cases' driver on the device: numpy arrays go up into tensors placed `off` bytes behind a 256-byte boundary, the calls go
    through lib/bitboard.py, the results come back as numpy arrays.  winner / diff are allocated by score_batch itself."""
    allocates = ("winner", "diff")

    def __init__(self):
        from reversi_alpha_zero_amd.lib import bitboard
        self.bb = bitboard

    @staticmethod
    def _put(a, off=0, fill=None):
        a = np.array(a, order="C")                     # (a copy: the cases' arrays are read-only, which torch.from_numpy warns about)
        buf = torch.full((a.nbytes + 256,), C.SENTINEL, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 256 == 0
        t = buf[off:off + a.nbytes].view(_TORCH_VIEW[a.dtype])
        if fill is None:
            t.copy_(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a))
        assert a.size == 0 or t.data_ptr() % 256 == off
        return t

    def _blank(self, dtype, n, off=0):
        return self._put(np.zeros(n, dtype=dtype), off, fill=C.SENTINEL)

    @staticmethod
    def _get(t):
        a = t.cpu().numpy()
        return a.view(_NUMPY_VIEW[t.dtype]) if t.dtype in _NUMPY_VIEW else a

    def _run(self, fn, outputs):
        """outputs: {name: tensor}, or a function of fn's result that gives it."""
        try:
            res = fn()
        except RuntimeError as e:
            torch.cuda.synchronize()
            raise C.Refused(None, str(e), {k: self._get(t) for k, t in outputs.items()} if isinstance(outputs, dict) else {})
        torch.cuda.synchronize()
        outputs = outputs if isinstance(outputs, dict) else outputs(res)
        return tuple(self._get(t) for t in outputs.values())

    def legal_moves(self, own, enemy, offsets={}):
        o, e, l = self._put(own, offsets.get("own", 0)), self._put(enemy, offsets.get("enemy", 0)), self._blank(np.uint64, len(own), offsets.get("legal", 0))
        return self._run(lambda: self.bb.legal_moves_batch(o, e, out=l), {"legal": l})

    def calc_flip(self, pos, own, enemy, offsets={}):
        p, o, e = self._put(pos, offsets.get("pos", 0)), self._put(own, offsets.get("own", 0)), self._put(enemy, offsets.get("enemy", 0))
        f = self._blank(np.uint64, len(own), offsets.get("flipped", 0))
        return self._run(lambda: self.bb.calc_flip_batch(p, o, e, out=f), {"flipped": f})

    def step(self, black, white, player, status, action, offsets={}):
        b, w, p, s = (self._put(a, offsets.get(k, 0)) for k, a in (("black", black), ("white", white), ("player", player), ("status", status)))
        l, a = self._blank(np.uint64, len(black), offsets.get("legal", 0)), self._put(action, offsets.get("action", 0))
        return self._run(lambda: self.bb.step_batch(b, w, p, s, l, a), {"black": b, "white": w, "player": p, "status": s, "legal": l})

    def score(self, black, white, offsets={}):
        b, w = self._put(black, offsets.get("black", 0)), self._put(white, offsets.get("white", 0))
        return self._run(lambda: self.bb.score_batch(b, w), lambda res: {"winner": res[0], "diff": res[1]})

    def d4(self, x, sym, offsets={}):
        i, o, s = self._put(x, offsets.get("x", 0)), self._blank(np.uint64, len(x), offsets.get("out", 0)), self._put(sym, offsets.get("sym", 0))
        return self._run(lambda: self.bb.d4_batch(i, s, out=o), {"out": o})

    def planes(self, own, enemy, offsets={}):
        o, e = self._put(own), self._put(enemy)
        return self._run(lambda: self.bb.planes_batch(o, e), lambda res: {"planes": res.reshape(len(own), 128)})

    def pick_kth(self, legal, rnd, offsets={}):
        l, r = self._put(legal), self._put(rnd)
        return self._run(lambda: self.bb.pick_kth_legal_batch(l, r), lambda res: {"action": res})

    def forms(self, n):
        return self.bb.sweep_forms(n)

    def max_grid(self):
        return self.bb.sweep_max_grid()


@pytest.fixture(scope="module")
def drv():
    return DeviceDriver()


def test_configuration_is_in_force_and_the_loops_iterate(drv):
    """First in the file: what a child runs before anything else.  (A run with RAZ_SWEEP_* variables set from outside and not by the
    test below has a configuration this file knows nothing about: the comparisons still hold, this one has nothing to say.)"""
    if CONFIG is None and any(k.startswith("RAZ_SWEEP_") for k in os.environ):
        return
    C.check_configuration(drv, CONFIG)
    if CONFIG is None:
        assert drv.forms(C.N_LOOP) == (0, 0)
    t = C.check_iterations(drv, CONFIG)
    print(f"\ntrips[{CONFIG}] " + " ".join(f"{k}={v[0]}/{v[1]}" for k, v in sorted(t.items())))


def test_the_cases_check_themselves():
    C.self_check()


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("entry", C.ENTRIES)
def test_entry_equals_its_reference(drv, entry, n):
    C.check_entry(drv, entry, n, CONFIG)


def test_misaligned_arrays_are_refused_and_nothing_is_written(drv):
    """(raz_*_batch compare the pointers on the host, in RAZ_REQUIRE, before the first launch: no kernel sees such an array.)"""
    assert C.check_refusals(drv) == len(C.REFUSALS) - 2          # (winner, diff: score_batch's own tensors)


def test_step_with_byte_arrays_4_bytes_off_equals_the_aligned_call(drv):
    """(In configurations c and e: the hybrid form's demotion to k_step, whose pipeline then walks all 41 blocks.)"""
    C.check_step_with_bytes_4_off(drv)


@pytest.mark.parametrize("config", sorted(C.CONFIGS))
def test_loops_iterate_in_a_process_of_their_own(config):
    """The file again in a child with the configuration's variables (read once per process) and no other RAZ_SWEEP_* variable; one
    child at a time."""
    if CONFIG:
        pytest.skip("a child of this test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RAZ_SWEEP_")}
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not in_a_process_of_their_own"],
                       env={**env, **C.CONFIGS[config]["env"], "RAZ_SWEEP_LOOPS_CHILD": config}, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and f"trips[{config}]" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
