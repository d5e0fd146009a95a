"""CPU, no kernels: what raznet-train-v2 refuses, and the arithmetic fact its tolerance rests on - a dot product of split-f16
operands (three terms, f32 accumulation, one exact un-scale) is an f32-class result, the hi halves alone are not."""
import ctypes
import types

import numpy as np
import pytest


def test_device_trainer_refuses_an_unknown_precision():
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer, precision_code
    assert precision_code("f32") == 0 and precision_code("f16x3") == 1
    for bad in ("f16", "F16X3", "", None, 1):
        with pytest.raises(ValueError, match="precision"):
            DeviceTrainer(ReversiNet(16, 1, 16), max_batch=4, precision=bad)   # refused before any device call


def test_worker_refuses_precision_with_the_torch_backend_and_unknown_ones():
    from reversi_alpha_zero_amd.worker import optimize
    cfg = types.SimpleNamespace()
    with pytest.raises(ValueError, match="precision"):
        optimize.OptimizeWorker(cfg, backend="torch", precision="f16x3")
    with pytest.raises(ValueError, match="precision"):
        optimize.OptimizeWorker(cfg, backend="torch", precision="f32")
    with pytest.raises(ValueError, match="precision"):
        optimize.OptimizeWorker(cfg, backend="hip", precision="bf16", device="cuda:0")
    assert optimize.DEFAULT_BACKEND == "torch"
    assert optimize.OptimizeWorker(cfg, backend="hip", device="cuda:0").precision == "f32"
    assert optimize.OptimizeWorker(cfg, backend="hip", precision="f16x3", device="cuda:0").precision == "f16x3"
    assert optimize.OptimizeWorker(cfg, backend="torch", device="cpu").precision == "f32"
    with pytest.raises(ValueError, match="precision"):
        optimize.start(cfg, backend="torch", precision="f16x3")


def test_the_c_entries_refuse_precision_2():
    import emu_util
    lib = emu_util.load_train()
    lib.raz_last_error.restype = ctypes.c_char_p
    assert lib.raz_trainer_bytes2(16, 1, 16, 8, 2) == 0
    assert b"precision" in lib.raz_last_error()
    assert lib.raz_trainer_bytes2(16, 1, 16, 8, -1) == 0
    need = lib.raz_trainer_bytes2(16, 1, 16, 8, 1)
    assert need > lib.raz_trainer_bytes2(16, 1, 16, 8, 0) == lib.raz_trainer_bytes(16, 1, 16, 8) > 0
    keep, base = emu_util.aligned(need)
    h = ctypes.c_void_p()
    assert lib.raz_trainer_create2(16, 1, 16, 8, 2, base, need, ctypes.byref(h), None) == -1 and not h.value
    assert b"precision" in lib.raz_last_error()
    assert lib.raz_trainer_create2(16, 1, 16, 8, 1, base, need - 1, ctypes.byref(h), None) == -1 and not h.value   # one byte short
    assert lib.raz_trainer_create2(24, 1, 16, 8, 1, base, need, ctypes.byref(h), None) == -1 and not h.value       # F % 16 != 0
    assert b"raz_trainer_create2" in lib.raz_last_error() and b"raznet-train-v2" in lib.raz_last_error()   # the entry and precision used
    assert lib.raz_trainer_create(24, 1, 16, 8, base, need, ctypes.byref(h), None) == -1 and not h.value
    assert lib.raz_last_error().startswith(b"raz_trainer_create: raznet-train-v1 takes")
    assert lib.raz_trainer_precision(None) == -1
    assert lib.raz_trainer_create2(16, 1, 16, 8, 1, base, need, ctypes.byref(h), None) == 0 and h.value
    assert lib.raz_trainer_precision(h) == 1
    lib.raz_trainer_destroy(h)


# ---- the split, restated in numpy ---------------------------------------------------------------------------------------------
def scale_of(x):
    """The power of two S with max |x| S in [2^14, 2^15); 1 for zeros (k_scale_f16x3)."""
    mx = float(np.abs(x).max())
    if mx == 0.0:
        return np.float32(1.0)
    _, e = np.frexp(np.float32(mx))
    return np.float32(np.ldexp(1.0, 15 - int(e)))


def split(x, S):
    v = (x.astype(np.float32) * S).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_dot(pairs, Sa, Sb):
    """The given (operand, operand) terms into ONE f32 accumulator, as the kernels issue them: per 16 consecutive k one matrix
    instruction per term, in the order given; a product of two halfs is exact in f32, an instruction's 16 products are added in f32
    (k ascending, as the wave emulator does; the device's order inside an instruction is not documented) and their sum is added to
    the accumulator in f32; then the two exact un-scales."""
    acc = np.float32(0.0)
    n = len(pairs[0][0])
    for i in range(0, n, 16):
        for x, y in pairs:
            group = np.float32(0.0)
            for p in x[i:i + 16].astype(np.float32) * y[i:i + 16].astype(np.float32):
                group = np.float32(group + p)
            acc = np.float32(acc + group)
    return float(np.float32(np.float32(acc * (np.float32(1.0) / Sa)) * (np.float32(1.0) / Sb)))


def vectors():
    """Eight pairs of random f32 vectors of length 2304 (a 3x3 product over 256 channels), seeds 0 to 7, none passed over:
    activations ~ 0.1 N(0, 1), gradients ~ N(0, 1) with their 1 / B."""
    out = []
    for seed in range(8):
        rng = np.random.default_rng(seed)
        a = (0.1 * rng.standard_normal(2304)).astype(np.float32)
        b = (0.05 / 33 * rng.standard_normal(2304)).astype(np.float32)
        out.append((a, b, float(np.dot(a.astype(np.float64), b.astype(np.float64)))))
    return out


def test_three_term_split_dot_product_is_f32_class_and_hi_alone_is_not():
    """Relative to the f64 dot product: the three terms are within 2^-19 on EVERY pair.  The hi halves alone are not within 2^-13:
    an operand rounded to 11 bits leaves an error that is a random number of that size per pair - 2^-9.1 to 2^-17.5 here - so the
    bound 2^-13 fails on most pairs (asserted: on at least half of them), and cannot be asked to fail on each."""
    three, hi_only = [], []
    for a, b, exact in vectors():
        Sa, Sb = scale_of(a), scale_of(b)
        assert 2.0 ** 14 <= float(np.abs(a).max()) * float(Sa) < 2.0 ** 15 and 2.0 ** 14 <= float(np.abs(b).max()) * float(Sb) < 2.0 ** 15
        (ah, al), (bh, bl) = split(a, Sa), split(b, Sb)
        assert np.isfinite(ah.astype(np.float32)).all() and np.isfinite(bh.astype(np.float32)).all()
        three.append(abs(split_dot([(al, bh), (ah, bl), (ah, bh)], Sa, Sb) - exact) / abs(exact))
        hi_only.append(abs(split_dot([(ah, bh)], Sa, Sb) - exact) / abs(exact))
        print(f"three terms {three[-1]:.3g} (2^{np.log2(max(three[-1], 1e-300)):.1f}), hi alone {hi_only[-1]:.3g} (2^{np.log2(hi_only[-1]):.1f}) relative to f64")
    assert all(e <= 2.0 ** -19 for e in three)
    assert 2 * sum(e > 2.0 ** -13 for e in hi_only) >= len(hi_only)


def test_scale_rule_edges():
    assert scale_of(np.zeros(4, np.float32)) == 1.0
    for mx in (1.0, 0.99999994, 2.0 ** -30, 3e-5 / 256, 1234.5):
        S = float(scale_of(np.array([mx, -mx / 3], np.float32)))
        assert 2.0 ** 14 <= mx * S < 2.0 ** 15 and np.log2(S) == int(np.log2(S))
