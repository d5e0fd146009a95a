"""Inputs and assertions shared by the tests of raz_spec_probe (tests/test_spec_probe_gpu.py on the GPU, tests/test_spec_probe_emu.py
on the wave emulator) and by the oracle-against-mathematics test (tests/test_oracle_mcts.py).

raz_spec_probe (include/raz.h) runs the device forms of raz-math-v1 / raz-rng-v1 (csrc/raz_detmath.h) and the wave-level reductions of
the tree kernels (csrc/raz_engine_core.h) on caller-supplied buffers.  The builders below return deterministic inputs at the places
where such code goes wrong - range ends, subnormals, reduction split points, ties, exact cdf steps - plus large random blocks (`n_random`;
the emulator tests pass a smaller number, the structured values are always all there).  The `check_*` functions hold the assertions;
they take `probe(what, in0, in1, out_dtype, out_shape) -> numpy array`, which is all that differs between the two test files.

References: the C oracle (oracle/orc_rng.c), bit for bit, for everything that is specified by raz-math-v1 / raz-rng-v1; numpy for the
wave reductions (the reference project's arithmetic is numpy's)."""
import ctypes

import numpy as np

# include/raz.h RAZ_PROBE_*
PHILOX, RNG_PAIR, LOG, EXP, COS2, POW, EXPF, TANHF, GAMMA_HALF_PAIR, GAMMA_ATTEMPT = range(10)
NP_SUM_F32, ARGMAX_F64, ARGMAX_NONNEG_F64, MAX_F64, SUM_U32, ROOT_GAMMAS, CHOICE = range(10, 17)

ALPHAS = (0.03, 0.3, 0.75, 1.0, 1.01, 1.7, 3.0, 12.5)   # every branch of the Gamma sampler: numpy's shape < 1 scheme, exponential, Marsaglia-Tsang
SQRT2_SPLIT = float.fromhex("0x1.6a09e667f3bcdp+0")    # raz_det_log's mantissa split (sqrt 2 rounded)
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
DBL_MAX = float.fromhex("0x1.fffffffffffffp+1023")
U53_TOP = 1.0 - 2.0 ** -53                              # the largest value of raz_u53


def _rng(tag):
    return np.random.default_rng([20240917, tag])


def f64_of_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def bits_of(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def around(x, k, dtype=np.float64):
    """x and its k neighbours on either side in `dtype` (finite x != 0: the bit pattern +- j)."""
    it = {np.float64: np.int64, np.float32: np.int32}[dtype]
    b = np.asarray([x], dtype=dtype).view(it)[0]
    return (b + np.arange(-k, k + 1, dtype=it)).view(dtype)


# ---------------------------------------------------------------------------------------------------------------- element-wise inputs
def log_cases(n_random=1 << 20, n_sampler=1 << 16):
    r = _rng(1)
    parts = [
        f64_of_bits([1, 0x000fffffffffffff, 0x0010000000000000]),          # 5e-324, the largest subnormal, the smallest normal
        np.ldexp(1.0, np.arange(-1074, 1024)),                              # every power of two
        around(1.0, 1), around(2.0 ** 0.5, 3), around(0.5 ** 0.5, 3), around(SQRT2_SPLIT, 3),
        around(SQRT2_SPLIT, 3) * 2.0 ** -1022, around(SQRT2_SPLIT, 3) * 2.0 ** 1000, around(SQRT2_SPLIT, 3) * 2.0 ** -1060,
        np.array([DBL_MAX, np.inf]),
        np.array([0.0, -0.0, -1.0, np.nan, -np.inf, -5e-324]),              # not > 0: all -1e308
        1.0 - np.arange(0, 4097) * 2.0 ** -53,                              # 1 - u53: what the samplers feed it
        1.0 - r.integers(0, 1 << 53, n_sampler).astype(np.float64) * 2.0 ** -53,
        f64_of_bits(r.integers(1, 0x7ff0000000000000, n_random, dtype=np.uint64)),   # any positive finite number
    ]
    return np.concatenate(parts)


def exp_cases(n_random=1 << 20):
    """NaN is left out: raz_det_exp converts its argument with (long long), which C leaves undefined for a NaN - outside its contract."""
    r = _rng(2)
    k = np.arange(-1075, 1025, dtype=np.float64)
    steps = (k + 0.5) * LN2                                                 # where the reduction's k = floor(x / ln2 + 1/2) changes
    steps = (bits_of(steps).view(np.int64)[:, None] + np.arange(-3, 4)).view(np.float64).ravel()
    parts = [
        around(-745.0, 1), around(709.78, 1), np.array([np.inf, DBL_MAX, -np.inf, -DBL_MAX]),
        np.array([0.0, -0.0, 5e-324, -5e-324]),
        around(LN2 / 2, 3), around(-LN2 / 2, 3), steps,
        np.array([-746.0, 710.0, -744.5, -708.5, -708.0, 709.0, 709.5]),    # both scaled-result branches (ki < -1021, ki > 1023) and their edges
        r.uniform(-746.0, 710.0, n_random),
    ]
    return np.concatenate(parts)


def cos2_cases(n_random=1 << 20):
    """u in [0, 1).  j/8 and both neighbours; 0 has no lower neighbour in the domain (its place is taken by the largest u, 1 - 2^-53)."""
    r = _rng(3)
    parts = [np.array([0.0, 5e-324, 2.0 ** -53, U53_TOP])]
    parts += [around(j / 8.0, 1) for j in range(1, 8)]
    parts += [np.arange(0, 1 << 12) * 2.0 ** -12]
    parts += [r.integers(0, 1 << 53, n_random).astype(np.float64) * 2.0 ** -53]
    return np.concatenate(parts)


def pow_cases(n_random=1 << 16):
    """(x, y) as the shape < 1 Gamma sampler calls raz_det_pow: (U, 1/alpha) on its first branch, (1 - alpha + alpha Y, 1/alpha) with
    Y = -log((1 - U) / alpha) on its second; also U = 2^-53 and values of U small enough for the result to underflow, and x <= 0."""
    r = _rng(4)
    xs, ys = [], []
    for a in (0.03, 0.3, 0.75):
        u = r.integers(1, 1 << 53, n_random).astype(np.float64) * 2.0 ** -53
        edge = np.array([2.0 ** -53, 2.0 ** -52, 1e-250, 2.0 ** -1000, 5e-324, U53_TOP, 1.0 - a, 1.0, 0.0, -0.0, -1.0])
        u2 = 1.0 - a + a * r.random(n_random)                               # U > 1 - alpha
        arg = 1.0 - a + a * -np.log((1.0 - u2) / a)
        x = np.concatenate([u, edge, arg])
        xs.append(x)
        ys.append(np.full(len(x), 1.0 / a))
    return np.concatenate(xs), np.concatenate(ys)


def f32_cases(stride=61):
    """Every float32 bit pattern that is 0 mod `stride` (61 in the full test), NaNs removed, plus the edges of raz_det_expf / raz_det_tanhf:
    +-4096 ulp around -87, 88, +-10 and 0; +-0, +-inf, FLT_MAX, subnormals."""
    sweep = np.arange(0, 1 << 32, stride, dtype=np.uint64).astype(np.uint32).view(np.float32)
    sweep = sweep[~np.isnan(sweep)]
    z = np.arange(0, 4097, dtype=np.uint32)
    parts = [sweep, around(-87.0, 4096, np.float32), around(88.0, 4096, np.float32), around(10.0, 4096, np.float32),
             around(-10.0, 4096, np.float32), z.view(np.float32), (z | np.uint32(0x80000000)).view(np.float32),
             np.array([0.0, -0.0, np.inf, -np.inf, 3.4028234663852886e38, -3.4028234663852886e38], dtype=np.float32),
             np.array([0x00000001, 0x007fffff, 0x00800000, 0x80000001, 0x807fffff, 0x80800000], dtype=np.uint32).view(np.float32)]
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------------------------- Philox
PHILOX_KATS = [   # Random123 kat_vectors, philox4x32-10: (counter, key, output)
    ([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xffffffff


def philox_inverse(out, key):
    """The counter that Philox4x32-10 maps to `out` under `key` (a round is a bijection: c2 = lo(M1 c2) / M1 mod 2^32, ...)."""
    i0, i1 = pow(_M0, -1, 1 << 32), pow(_M1, -1, 1 << 32)
    c0, c1, c2, c3 = out
    for r in range(9, -1, -1):
        k0, k1 = (key[0] + r * _W0) & _MASK, (key[1] + r * _W1) & _MASK
        p2, p0 = (c1 * i1) & _MASK, (c3 * i0) & _MASK                       # the round's input c2 and c0
        c0, c1, c2, c3 = p0, c0 ^ ((_M1 * p2) >> 32) ^ k0, p2, c2 ^ ((_M0 * p0) >> 32) ^ k1
    return [c0, c1, c2, c3]


def u53_edge_tuples():
    """(seed, game, purpose, event, sub, idx) whose Philox block is all zeros / all ones / mixed: raz_u53 = 0 and 1 - 2^-53, found by
    running the cipher backwards (raz_rng_pair's counter is (idx, sub, event, purpose), its key (seed, game))."""
    rows = []
    for out in ([0, 0, 0, 0], [_MASK] * 4, [0, 0, _MASK, _MASK], [_MASK, _MASK, 0, 0], [31, 63, _MASK & ~31, _MASK & ~63]):
        for key in ([0, 0], [7, 12345], [_MASK, 1]):
            idx, sub, event, purpose = philox_inverse(out, key)
            rows.append([key[0], key[1], purpose, event, sub, idx])
    return np.array(rows, dtype=np.uint32)


def philox_cases(n_random=1 << 20):
    r = _rng(5)
    kat = np.array([c + k for c, k, _ in PHILOX_KATS], dtype=np.uint32)
    small = np.array([[i, j, e, p, 1, g] for i in range(3) for j in range(3) for e in range(3) for p in range(4) for g in range(3)], dtype=np.uint32)
    return np.concatenate([kat, small, r.integers(0, 1 << 32, (n_random, 6), dtype=np.uint64).astype(np.uint32)])


def rng_pair_cases(n_random=1 << 20):
    r = _rng(6)
    return np.concatenate([u53_edge_tuples(), philox_cases(0), r.integers(0, 1 << 32, (n_random, 6), dtype=np.uint64).astype(np.uint32)])


# ---------------------------------------------------------------------------------------------------------------- Gamma sampler
def gamma_half_pair_cases(n=1 << 16):
    r = _rng(7)
    small = np.array([[s, g, e, m] for s in (0, 11) for g in range(4) for e in range(8) for m in range(32)], dtype=np.uint32)
    return np.concatenate([small, r.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)])


def gamma_attempt_cases(n_pairs=4096, n_t=16):
    """alpha[n], (seed, game, event, sub, t)[n]: per alpha n_pairs (event, sub) pairs x attempts t = 0 .. n_t - 1, t fastest."""
    al, keys = [], []
    for i, a in enumerate(ALPHAS):
        ev, sub, t = np.meshgrid(np.arange(n_pairs // 32), np.arange(32), np.arange(n_t), indexing="ij")
        k = np.stack([np.full(ev.size, 11), np.full(ev.size, 5 + i), ev.ravel() * 7 + i, sub.ravel(), t.ravel()], axis=1)
        keys.append(k.astype(np.uint32))
        al.append(np.full(ev.size, a))
    return np.concatenate(al), np.concatenate(keys)


# Rows (alpha, k, seed, game, event) of root_noise in which some sample needs a SECOND round of the wave loop, one per
# attempts-per-round class A = min(8, 64 // k): found on the CPU with orc_gamma_sample_t (t_accepted >= A), see test_*_root_gammas.
# (at A = 8 eight attempts in a row must fail: about one sample in 3e7 at alpha = 0.3, the alpha that rejects most often.)
SECOND_ROUND_ROWS = [
    (0.3, 8, 21, 4, 3967665),    # A = 8: t_accepted = 8
    (0.75, 9, 21, 4, 7793792),   # A = 7 (lanes 63.. idle): t_accepted = 7
    (0.75, 10, 21, 4, 1403128),  # A = 6: 6
    (0.75, 12, 21, 4, 404413),   # A = 5: 5
    (0.75, 16, 21, 4, 2035),     # A = 4: 4
    (0.75, 21, 21, 4, 178),      # A = 3: 3
    (0.75, 30, 21, 4, 8),        # A = 2: 3
    (0.75, 47, 21, 4, 0),        # A = 1: 1
]


def root_gammas_cases(n_events=256):
    """alpha[n], (k, seed, game, event)[n]: every k in 1..64 (every attempts-per-round class A = 8 .. 1, lanes beyond A k idle as at k = 9)
    at every alpha of ALPHAS and at 0.5 (the pair path), n_events events each, and the SECOND_ROUND_ROWS."""
    al, keys = [], []
    for i, a in enumerate(ALPHAS + (0.5,)):
        k, ev = np.meshgrid(np.arange(1, 65), np.arange(n_events), indexing="ij")
        keys.append(np.stack([k.ravel(), np.full(k.size, 3 + i), k.ravel() % 5, ev.ravel() + 1000 * i], axis=1).astype(np.uint32))
        al.append(np.full(k.size, a))
    al.append(np.array([r[0] for r in SECOND_ROUND_ROWS], dtype=np.float64))
    keys.append(np.array([r[1:] for r in SECOND_ROUND_ROWS], dtype=np.uint32).reshape(-1, 4))
    return np.concatenate(al), np.concatenate(keys)


# ---------------------------------------------------------------------------------------------------------------- wave reductions
def np_sum_cases(n_random=4096):
    """float32[n][64]; the first n_random rows are the wide-range ones (1e-8 .. 1e8, both signs: cancellation)."""
    r = _rng(8)
    wide = (10.0 ** r.uniform(-8, 8, (n_random, 64)) * r.choice([-1.0, 1.0], (n_random, 64))).astype(np.float32)
    logits = r.normal(0, 3, (n_random, 64))
    soft = np.exp(logits - logits.max(1, keepdims=True))
    soft = (soft / soft.sum(1, keepdims=True)).astype(np.float32) * (r.random((n_random, 64)) < r.random((n_random, 1))).astype(np.float32)
    single = np.zeros((128, 64), dtype=np.float32)
    single[np.arange(64), np.arange(64)] = 0.1
    single[64 + np.arange(64), np.arange(64)] = np.float32(1e-40)          # a subnormal
    return np.concatenate([wide, soft, np.zeros((1, 64), dtype=np.float32), single]), n_random


def _tie_lanes():
    """Lane sets that hold the maximum: 2, 3 and 64 lanes in every alignment class of the reduction (inside a quad, across quads of a
    row of 16, across the 16 / 32 / 48 row boundaries)."""
    sets = [list(range(64))]
    for a in range(64):
        for d in (1, 2, 3, 4, 8, 12, 15, 16, 17, 31, 32, 33, 47, 48, 63):
            if a + d < 64:
                sets.append([a, a + d])
    for a, b, c in [(0, 1, 2), (1, 2, 3), (3, 4, 5), (2, 7, 9), (14, 15, 16), (15, 16, 17), (15, 31, 47), (16, 32, 48), (31, 32, 33),
                    (47, 48, 63), (5, 37, 62), (0, 16, 63), (13, 29, 45), (62, 63, 0)]:
        sets.append(sorted({a, b, c}))
    return sets


def argmax_cases(nonneg, n_random=4096):
    """float64[n][64].  nonneg: inputs of wave_argmax_nonneg_f64, whose contract is FINITE values >= +0 (it orders IEEE bit patterns as
    unsigned integers: -0 and NaN would order wrongly, and the PUCT scores it serves are never either) - so no -0, no NaN, no negatives
    here; the general wave_argmax_f64 also gets negatives and +-0 mixed."""
    r = _rng(9 + int(nonneg))
    rows = [r.random((n_random, 64)), 1000.0 + r.random((n_random, 64)) * 1e-9]
    if not nonneg:
        rows += [r.normal(0, 1, (n_random, 64)), -r.random((n_random, 64))]
    ties = _tie_lanes()
    base = r.random((len(ties), 64)) * 0.5
    for vals in ((0.75,), (1000.0 + 2.0 ** -40,)) if nonneg else ((0.75,), (-0.0,), (1000.0 + 2.0 ** -40,)):
        t = base.copy() if vals[0] > 0 else -1.0 - base
        for i, lanes in enumerate(ties):
            t[i, lanes] = vals[0]
        rows.append(t)
    # top values that share the high word and differ in the low word only (1000 + tiny: the PUCT scores' own shape)
    hi = np.uint64(np.float64(1000.0).view(np.uint64) & np.uint64(0xffffffff00000000))
    low = r.integers(0, 1 << 32, (n_random, 64), dtype=np.uint64)
    rows.append((hi | low).view(np.float64))
    low2 = low.copy()
    low2[:, 1::2] = low2[:, ::2]                                            # and with low-word ties among them
    rows.append((hi | low2).view(np.float64))
    sub = r.integers(0, 1 << 20, (256, 64), dtype=np.uint64).view(np.float64)   # subnormals and +0
    sub[:, ::5] = 0.0
    rows.append(sub)
    rows.append(np.zeros((1, 64)))
    if not nonneg:
        z = np.where(r.random((256, 64)) < 0.5, 0.0, -0.0)                  # +-0 mixed: equal, so the first lane wins
        rows += [z, np.where(r.random((256, 64)) < 0.2, z[:256], -1.0 - r.random((256, 64)))]
    return np.concatenate(rows)


def sum_u32_cases(n_random=4096):
    r = _rng(12)
    return np.concatenate([r.integers(0, 1000, (n_random, 64), dtype=np.uint64).astype(np.uint32),
                           r.integers(0, 1 << 32, (n_random, 64), dtype=np.uint64).astype(np.uint32),      # wraps around
                           np.full((1, 64), 0xffffffff, dtype=np.uint32), np.zeros((1, 64), dtype=np.uint32),
                           np.eye(64, dtype=np.uint32) * np.uint32(0x80000001)])


def np_cdf(p):
    c = np.cumsum(p, axis=-1)
    return c / c[..., -1:]


def choice_cases(n_random=512):
    """policy float64[n][64], uniform float64[n]: policies from visit counts (N / sum N), one-hot at every lane, leading and trailing
    zero runs; uniforms 0, 1 - 2^-53, random, and every cdf step with both neighbours."""
    r = _rng(13)
    pol = []
    for _ in range(n_random):
        n = r.integers(0, 50, 64).astype(np.float64) * (r.random(64) < r.random())
        if n.sum() == 0:
            n[r.integers(64)] = 1.0
        pol.append(n / n.sum())
    pol += list(np.eye(64))
    for lead, trail in ((1, 0), (0, 1), (10, 10), (31, 32), (62, 0), (0, 62), (20, 43)):
        n = np.zeros(64)
        n[lead:64 - trail] = r.integers(1, 30, 64 - lead - trail)
        pol.append(n / n.sum())
    P, U = [], []
    for p in pol:
        steps = np.unique(np_cdf(p))
        steps = steps[(steps > 0) & (steps < 1)]
        if len(steps) > 12:
            steps = np.concatenate([steps[:4], steps[-4:], r.choice(steps[4:-4], 4, replace=False)])
        us = [0.0, U53_TOP, r.random(), r.random()]
        for s in steps:
            us += list(around(s, 1))
        us = [u for u in us if 0.0 <= u < 1.0]
        P += [p] * len(us)
        U += us
    return np.array(P), np.array(U)


# ---------------------------------------------------------------------------------------------------------------- the oracle, in batches
def orc_map(lib, what, in0, in1, out_dtype, per=1):
    in0 = np.ascontiguousarray(in0)
    n = len(in0)
    out = np.zeros((n, per) if per > 1 else n, dtype=out_dtype)
    rc = lib.orc_spec_map(what, in0.ctypes.data, None if in1 is None else np.ascontiguousarray(in1).ctypes.data, out.ctypes.data, n)
    assert rc == 0
    return out


def orc_gamma_t(lib, alpha, key4):
    alpha, key4 = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(key4, dtype=np.uint32)
    x, t = np.zeros(len(alpha)), np.zeros(len(alpha), dtype=np.uint32)
    lib.orc_gamma_sample_t_n(alpha.ctypes.data, key4.ctypes.data, x.ctypes.data, t.ctypes.data, len(alpha))
    return x, t


def same_bits(got, want, what, inputs=None):
    g, w = bits_of(got).ravel(), bits_of(want).ravel()
    bad = np.flatnonzero(g != w)
    if len(bad):
        i = bad[0]
        per = g.size // len(got)
        where = "" if inputs is None else f" input {inputs[i // per]!r}"
        raise AssertionError(f"{what}: {len(bad)} of {g.size} differ; first at {i}:{where} got {got.ravel()[i]!r} ({g[i]:#x}) want {want.ravel()[i]!r} ({w[i]:#x})")


# ---------------------------------------------------------------------------------------------------------------- assertions
def check_elementwise(probe, lib, n_random, f32_stride):
    """Device == oracle, bit for bit: philox, rng_pair, log, exp, cos2, pow, expf, tanhf."""
    x = philox_cases(n_random)
    got = probe(PHILOX, x, None, np.uint32, (len(x), 4))
    same_bits(got, orc_map(lib, PHILOX, x, None, np.uint32, 4), "philox", x)
    for c, k, out in PHILOX_KATS:
        i = [j for j in range(3) if list(x[j]) == c + k][0]
        assert list(got[i]) == out
    x = rng_pair_cases(n_random)
    got = probe(RNG_PAIR, x, None, np.float64, (len(x), 2))
    same_bits(got, orc_map(lib, RNG_PAIR, x, None, np.float64, 2), "rng_pair", x)
    e = got[: len(u53_edge_tuples())].reshape(5, 3, 2)
    assert (e[0] == 0.0).all() and (e[1] == U53_TOP).all() and (e[2] == [0.0, U53_TOP]).all() and (e[3] == [U53_TOP, 0.0]).all()
    assert (e[4] == [0.0, U53_TOP]).all()                                   # the bits raz_u53 drops (a & 31, b & 63) do not matter
    assert got.min() >= 0.0 and got.max() < 1.0
    for what, name, x in ((LOG, "log", log_cases(n_random, max(n_random >> 4, 1 << 12))), (EXP, "exp", exp_cases(n_random)),
                          (COS2, "cos2", cos2_cases(n_random))):
        got = probe(what, x, None, np.float64, (len(x),))
        same_bits(got, orc_map(lib, what, x, None, np.float64), name, x)
        if what == LOG:
            assert (got[~(x > 0)] == -1.0e308).all() and (~(x > 0)).sum() >= 6
        if what == EXP:
            assert (got[x < -745.0] == 0.0).all() and (got[x > 709.78] == DBL_MAX).all() and (x < -745.0).sum() > 2 and (x > 709.78).sum() > 2
    x, y = pow_cases(max(n_random >> 4, 1 << 12))
    got = probe(POW, x, y, np.float64, (len(x),))
    same_bits(got, orc_map(lib, POW, x, y, np.float64), "pow", x)
    assert (got[~(x > 0)] == 0.0).all() and ((got == 0.0) & (x > 0)).any()   # underflow is reached
    x = f32_cases(f32_stride)
    for what, name in ((EXPF, "expf"), (TANHF, "tanhf")):
        got = probe(what, x, None, np.float32, (len(x),))
        same_bits(got, orc_map(lib, what, x, None, np.float32), name, x)


def check_gamma_half_pair(probe, lib, n):
    x = gamma_half_pair_cases(n)
    got = probe(GAMMA_HALF_PAIR, x, None, np.float64, (len(x), 2))
    want = np.zeros((len(x), 2))
    g = (ctypes.c_double * 64)()
    for i, (seed, game, event, m) in enumerate(x.tolist()):
        if m < 32:
            lib.orc_dirichlet_gammas(0.5, 2 * m + 2, seed, game, event, g)
            want[i] = g[2 * m], g[2 * m + 1]
        else:                                                               # (pair m >= 32 is beyond a board's 64 moves: from its two functions)
            d = orc_map(lib, RNG_PAIR, np.array([[seed, game, 2, event, m, 0]], dtype=np.uint32), None, np.float64, 2)[0]
            E = -orc_map(lib, LOG, np.array([1.0 - d[0]]), None, np.float64)[0]
            c2 = orc_map(lib, COS2, np.array([d[1]]), None, np.float64)[0]
            want[i] = E * c2, E * (1.0 - c2)
    same_bits(got, want, "gamma_half_pair", x)


def check_gamma_attempt(probe, lib, n_pairs=4096, n_t=16):
    """For every (alpha, event, sub): the X of the first accepted attempt t == orc_gamma_sample_t's sample and its t.  Coverage, from the
    oracle: every alpha != 1 rejects some attempt 0; alpha = 1.01 and 1.7 meet V <= 0 (at 3.0 that needs a normal below -4.9, p = 5e-7,
    at 12.5 below -10.5: neither occurs in the 65 536 attempts per alpha here, nor should one be contrived)."""
    alpha, keys = gamma_attempt_cases(n_pairs, n_t)
    got = probe(GAMMA_ATTEMPT, alpha, keys, np.float64, (len(alpha), 2)).reshape(-1, n_t, 2)
    a1, k1 = alpha[::n_t], keys[::n_t, :4]
    x, t = orc_gamma_t(lib, a1, k1)
    acc = got[:, :, 1]
    assert np.isin(acc, (0.0, 1.0)).all()
    first = np.where(acc.any(1), acc.argmax(1), n_t)
    want_first = np.minimum(t, n_t)
    assert (first == want_first).all(), "first accepted attempt"
    ok = first < n_t
    assert ok.mean() > 0.99
    same_bits(got[ok, first[ok], 0], x[ok], "gamma_attempt X of the first accepted attempt")
    for a in ALPHAS:
        m = a1 == a
        assert (t[m] == 0).all() if a == 1.0 else (t[m] > 0).any(), a
    # V <= 0: from the oracle's own functions, V = 1 + c Z with Z of block 2t (Box-Muller) and its sign of block 2t + 1
    for a, expect in ((1.01, True), (1.7, True)):
        m = alpha == a
        kk = keys[m]
        blk = lambda idx: np.stack([kk[:, 0], kk[:, 1], np.full(len(kk), 2), kk[:, 2], kk[:, 3], idx], axis=1).astype(np.uint32)
        d = orc_map(lib, RNG_PAIR, blk(2 * kk[:, 4]), None, np.float64, 2)
        e = orc_map(lib, RNG_PAIR, blk(2 * kk[:, 4] + 1), None, np.float64, 2)
        E = -orc_map(lib, LOG, 1.0 - d[:, 0], None, np.float64)
        z2 = 2.0 * (E * orc_map(lib, COS2, d[:, 1].copy(), None, np.float64))
        Z = np.where(e[:, 0] < 0.5, -np.sqrt(z2), np.sqrt(z2))
        V = 1.0 + (1.0 / np.sqrt(9.0 * (a - float.fromhex("0x1.5555555555555p-2")))) * Z
        neg = V <= 0.0
        assert neg.any() == expect, a
        g = got.reshape(-1, 2)[m][neg]
        assert (g == 0.0).all(), "a V <= 0 attempt is rejected with X = 0"


def a_of_k(k):
    return np.minimum(8, 64 // k)


def check_root_gammas(probe, lib, n_events=256):
    """gammas, noise == orc_dirichlet_gammas / orc_dirichlet_noise_of_mask on a mask with k bits, for every row; the rounds the device
    reports == max_j(t_accepted_j // A) + 1 with t_accepted from orc_gamma_sample_t; and, from the oracle alone, every A in 1..8 has a
    row whose rounds are >= 2 (some sample's first A attempts all fail)."""
    alpha, keys = root_gammas_cases(n_events)
    n = len(alpha)
    raw = probe(ROOT_GAMMAS, alpha, keys, np.uint8, (n * 1028,))
    gam = raw[: n * 512].view(np.float64).reshape(n, 64)
    noise = raw[n * 512: n * 1024].view(np.float64).reshape(n, 64)
    rounds = raw[n * 1024:].view(np.uint32)
    want_g, want_n = np.zeros((n, 64)), np.zeros((n, 64))
    out = (ctypes.c_double * 64)()
    masks = {}
    r = _rng(14)
    for i in range(n):
        k, seed, game, event = keys[i].tolist()
        a = float(alpha[i])
        lib.orc_dirichlet_gammas(a, k, seed, game, event, want_g[i].ctypes.data)
        if (k, event & 3) not in masks:
            masks[(k, event & 3)] = sorted(r.choice(64, k, replace=False).tolist())
        sq = masks[(k, event & 3)]
        lib.orc_dirichlet_noise_of_mask(sum(1 << s for s in sq), a, seed, game, event, ctypes.byref(out))
        v = np.array(out[:])
        assert (v != 0).sum() <= k and (np.delete(v, sq) == 0).all()
        want_n[i, :k] = v[sq]                                               # by rank = ascending square
    same_bits(gam, want_g, "root gammas", keys)
    same_bits(noise, want_n, "root noise", keys)
    # rounds
    k = keys[:, 0].astype(np.int64)
    rej = alpha != 0.5
    rows = np.flatnonzero(rej)
    rep = np.repeat(rows, k[rows])
    sub = np.concatenate([np.arange(kk) for kk in k[rows]])
    key4 = np.stack([keys[rep, 1], keys[rep, 2], keys[rep, 3], sub], axis=1).astype(np.uint32)
    _, t = orc_gamma_t(lib, alpha[rep], key4)
    worst = np.zeros(n, dtype=np.int64)
    np.maximum.at(worst, rep, t.astype(np.int64) // a_of_k(k[rep]))
    want_rounds = np.where(rej, worst + 1, 0)
    assert (rounds == want_rounds).all(), f"rounds differ at rows {np.flatnonzero(rounds != want_rounds)[:8]}"
    A = a_of_k(k)
    for a in range(1, 9):
        assert (want_rounds[rej & (A == a)] >= 2).any(), f"no row with a second round at A = {a}"
    lit = np.arange(n - len(SECOND_ROUND_ROWS), n)
    assert (want_rounds[lit] >= 2).all() and sorted(set(A[lit].tolist())) == list(range(1, 9))


def check_wave_reductions(probe, n_random):
    """== numpy."""
    x, n_wide = np_sum_cases(n_random)
    got = probe(NP_SUM_F32, x, None, np.float32, (len(x),))
    want = np.array([np.sum(row) for row in x], dtype=np.float32)
    assert want.dtype == np.float32
    same_bits(got, want, "np_sum_f32")
    seq = np.zeros(len(x), dtype=np.float32)
    for j in range(64):
        seq = (seq + x[:, j]).astype(np.float32)
    assert (bits_of(seq[:n_wide]) != bits_of(want[:n_wide])).mean() > 0.5     # the order matters on these rows: a wrong one would show
    for what, nonneg in ((ARGMAX_F64, False), (ARGMAX_NONNEG_F64, True)):
        x = argmax_cases(nonneg, n_random)
        if nonneg:
            assert np.isfinite(x).all() and not np.signbit(x).any()
        got = probe(what, x, None, np.int32, (len(x),))
        want = np.argmax(x, axis=1)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"argmax (nonneg={nonneg}): {len(bad)} rows differ, first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    x = argmax_cases(False, n_random)
    got = probe(MAX_F64, x, None, np.float64, (len(x),))
    want = x.max(axis=1)
    assert (got == want).all()
    nz = want != 0
    same_bits(got[nz], want[nz], "max_f64")                                  # (+0 and -0 are one maximum: either may be returned)
    x = sum_u32_cases(n_random)
    got = probe(SUM_U32, x, None, np.uint32, (len(x),))
    assert (got == x.sum(axis=1, dtype=np.uint32)).all()
    assert (x.sum(axis=1, dtype=np.uint64) >> 32).any()


def check_choice(probe, n_random=512):
    p, u = choice_cases(n_random)
    got = probe(CHOICE, p, u, np.int32, (len(p),))
    cdf = np_cdf(p)
    want = np.array([min(63, int(np.searchsorted(cdf[i], u[i], side="right"))) for i in range(len(p))])
    on_step = (cdf == u[:, None]).any(1)
    assert on_step.sum() > 500                                               # uniforms that fall exactly on a cdf step are there
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"choice: {len(bad)} rows differ, first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    assert want.min() == 0 and want.max() == 63
