"""CPU: raz_spec_probe on the wave emulator (tests/native/libraz_emu.so) - the device source of raz-math-v1, raz-rng-v1 and of the tree
kernels' wave reductions, compiled for the host, against the oracle (bit for bit) and numpy.  Same cases and same assertions as
tests/test_spec_probe_gpu.py (tests/spec_cases.py); the large random blocks are thinned to 2^18, the float32 sweep to every
61 * 64-th bit pattern, the wave selectors' random rows to 2048 and the root-noise rows to 64 events per (alpha, k) instead of 256 (each row is a wave of 64 fibers here)
so that the file runs in tens of seconds; every structured edge and every coverage condition is kept."""
import numpy as np
import pytest

import oracle as O
import emu_util
import spec_cases as S

N_ELEMENTWISE = 1 << 18   # (element-wise kernels run at native speed here; the wave selectors are the slow ones)


@pytest.fixture(scope="module")
def lib():
    return O.load_ext()


@pytest.fixture(scope="module")
def probe():
    emu = emu_util.backend()

    def run(what, in0, in1, out_dtype, out_shape):
        in0 = np.ascontiguousarray(in0)
        in1 = None if in1 is None else np.ascontiguousarray(in1)
        out = np.zeros(out_shape, dtype=out_dtype)
        n = len(in0)
        emu.call("raz_spec_probe", what, in0.ctypes.data, None if in1 is None else in1.ctypes.data, out.ctypes.data, n, None)
        return out
    return run


def test_probe_rejects_bad_arguments(probe):
    emu = emu_util.load()
    x = np.zeros(64)
    assert emu.raz_spec_probe(99, x.ctypes.data, None, x.ctypes.data, 1, None) < 0
    assert emu.raz_spec_probe(S.POW, x.ctypes.data, None, x.ctypes.data, 1, None) < 0
    assert emu.raz_spec_probe(S.LOG, None, None, x.ctypes.data, 1, None) < 0
    assert emu.raz_spec_probe(S.MAX_F64, x.ctypes.data, None, x.ctypes.data, 1 << 24, None) < 0
    assert emu.raz_spec_probe(S.LOG, None, None, None, 0, None) == 0
    # rows the sampler has no exit for are answered with zeros: k outside 1..64, alpha not a positive finite number
    alpha = np.array([0.3, 0.3, 0.0, -1.0, np.nan, np.inf])
    keys = np.array([[0, 1, 2, 3], [65, 1, 2, 3], [4, 1, 2, 3], [4, 1, 2, 3], [4, 1, 2, 3], [4, 1, 2, 3]], dtype=np.uint32)
    raw = probe(S.ROOT_GAMMAS, alpha, keys, np.uint8, (6 * 1028,))
    assert not raw.any()


def test_elementwise_functions_equal_the_oracle_bit_for_bit(probe, lib):
    S.check_elementwise(probe, lib, N_ELEMENTWISE, 61 * 64)


def test_gamma_half_pair_equals_the_oracle(probe, lib):
    S.check_gamma_half_pair(probe, lib, 1 << 12)


def test_gamma_attempts_equal_the_oracle_sampler(probe, lib):
    S.check_gamma_attempt(probe, lib)


def test_root_gammas_every_k_and_every_attempts_per_round_class(probe, lib):
    S.check_root_gammas(probe, lib, n_events=64)


def test_wave_reductions_equal_numpy(probe):
    S.check_wave_reductions(probe, 2048)


def test_choice_equals_numpy_searchsorted(probe):
    S.check_choice(probe)
