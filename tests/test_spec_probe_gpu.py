"""GPU: raz_spec_probe on the device - raz-math-v1, raz-rng-v1 and the tree kernels' wave reductions as gfx950 executes them, against
the oracle (bit for bit, no tolerance) and numpy.  Cases and assertions: tests/spec_cases.py, at full size (2^20 random values per
function, every 61st float32 bit pattern).  This is the test of the premise that gfx950 rounds + - * / sqrt and the int/float
conversions exactly like x86-64 in these translation units, with the flags libraz is built with."""
import numpy as np
import pytest

import oracle as O
import spec_cases as S

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return O.load_ext()


@pytest.fixture(scope="module")
def probe():
    import torch
    from reversi_alpha_zero_amd import _native as N

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def run(what, in0, in1, out_dtype, out_shape):
        n = len(in0)
        d0, d1 = dev(in0), None if in1 is None else dev(in1)
        nbytes = int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        N.check(N.lib.raz_spec_probe(what, d0.data_ptr(), None if d1 is None else d1.data_ptr(), out.data_ptr(), n, N.current_stream_ptr()),
                "raz_spec_probe")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(out_dtype).reshape(out_shape)
    return run


def test_probe_rejects_bad_arguments(probe):
    import torch
    from reversi_alpha_zero_amd import _native as N
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert N.lib.raz_spec_probe(99, x.data_ptr(), None, x.data_ptr(), 1, None) < 0
    assert N.lib.raz_spec_probe(S.POW, x.data_ptr(), None, x.data_ptr(), 1, None) < 0
    assert N.lib.raz_spec_probe(S.LOG, None, None, x.data_ptr(), 1, None) < 0
    assert N.lib.raz_spec_probe(S.MAX_F64, x.data_ptr(), None, x.data_ptr(), 1 << 24, None) < 0
    assert N.lib.raz_spec_probe(S.LOG, None, None, None, 0, None) == 0
    alpha = np.array([0.3, 0.3, 0.0, -1.0, np.nan, np.inf])
    keys = np.array([[0, 1, 2, 3], [65, 1, 2, 3], [4, 1, 2, 3], [4, 1, 2, 3], [4, 1, 2, 3], [4, 1, 2, 3]], dtype=np.uint32)
    raw = probe(S.ROOT_GAMMAS, alpha, keys, np.uint8, (6 * 1028,))
    assert not raw.any()


def test_elementwise_functions_equal_the_oracle_bit_for_bit(probe, lib):
    S.check_elementwise(probe, lib, N_RANDOM, 61)


def test_gamma_half_pair_equals_the_oracle(probe, lib):
    S.check_gamma_half_pair(probe, lib, 1 << 16)


def test_gamma_attempts_equal_the_oracle_sampler(probe, lib):
    S.check_gamma_attempt(probe, lib)


def test_root_gammas_every_k_and_every_attempts_per_round_class(probe, lib):
    S.check_root_gammas(probe, lib)


def test_wave_reductions_equal_numpy(probe):
    S.check_wave_reductions(probe, 4096)


def test_choice_equals_numpy_searchsorted(probe):
    S.check_choice(probe)
