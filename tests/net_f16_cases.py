"""Nets, references and rules shared by the tests of raznet-forward-v3, the plain-f16 trunk (raz_net.reserved = 8, DeviceNet(kernel="f16");
tests/test_net_f16_emu.py on the wave emulator, tests/test_net_f16_gpu.py on the device).

v3 (include/raz.h raz_net_range_check): stem = the exact-f32 chains, then a = h(relu(.)); trunk layer l: out = h(relu(acc / S_l + bias
[+ skip])) with acc the f32 matrix-core accumulation of h(w * S_l) * a; heads = the exact-f32 chains on the f16 trunk output; h() =
round-to-nearest-even to f16.

Two kinds of net:
  - `integer_net`: every trunk activation is an f16 number and every sum an integer below 2^24, so NOTHING in v3 rounds - the
    quantisation is the identity, integer sums are exact in any order (matrix core or fmaf chain), the scale 2^14 and its inverse are
    exact, the heads are the same f32 chains in every form - and v3 must equal the exact-f32 kernels and the C oracle bit for bit;
  - net_cases.sharp_net float nets, where `quantised_reference` restates the specification in f64 and the kernel's distance from
    the true graph is held to a multiple of that restatement's own (`within_quantisation_rule`)."""
import numpy as np
import torch

import net_cases as C

RESERVED = 8                                   # include/raz.h: raz_net.reserved of raznet-forward-v3
INTEGER_CASES = [(128, 2, 64), (256, 1, 16)]   # one oc tile + two residual blocks (ping-pong, skip); two oc tiles per position group
DENSITY = {128: 0.1, 256: 0.05}                # share of non-zero (+-1) trunk weights
POOL = 67                                      # positions the integer nets are built on (the largest batch of the tests)


def positions(n=POOL, seed=1):
    """The first n of POOL random positions (own, enemy: uint64 numpy)."""
    rng = np.random.default_rng(seed)
    own = rng.integers(0, 2**64, size=POOL, dtype=np.uint64)
    enemy = rng.integers(0, 2**64, size=POOL, dtype=np.uint64) & ~own
    return own[:n], enemy[:n]


def _conv_int(a, w):
    """3x3 'same' cross-correlation of integer activations a (n, C, 8, 8) with integer weights w (O, C, 3, 3), as int64.  The
    products run through float64 BLAS: every operand and every partial sum is an integer far below 2^53, so each is exact."""
    n, c = a.shape[:2]
    ap = np.zeros((n, c, 10, 10), np.float64)
    ap[:, :, 1:9, 1:9] = a
    cols = np.stack([ap[:, :, ky:ky + 8, kx:kx + 8] for ky in range(3) for kx in range(3)], axis=2)   # (n, C, 9, 8, 8)
    out = np.tensordot(w.reshape(w.shape[0], -1).astype(np.float64), cols.reshape(n, c * 9, 64), axes=([1], [1]))   # (O, n, 64)
    assert np.array_equal(out, np.rint(out)) and np.abs(out).max() < 2.0**53
    return out.transpose(1, 0, 2).reshape(n, -1, 8, 8).astype(np.int64)


def integer_trunk(F, R, seed, own, enemy):
    """Integer conv parameters [(w (O, C, 3, 3) int64, b (O,) int64)] for the stem and the 2R trunk layers, and the int64 restatement's
    per-layer maxima over (own, enemy).  Stem: weights uniform in {-1, 0, +1}, bias 0.  Trunk: weights +-1 with density DENSITY[F],
    per-channel bias = minus the 0.9-quantile (the largest value not above it) of that layer's pre-activations - the convolution, plus
    the skip for a block's second layer - over (own, enemy), so that about a tenth of a layer's outputs stay above 0.
    Asserts the preconditions of the bit-exact test on the restatement alone: every activation is an f16 number, every |pre-sum|
    (bias and skip included, and every partial sum with them: all are bounded by the sum of the |terms|) is below 2^24."""
    rng = np.random.default_rng(seed)
    x = C.planes(own, enemy).numpy().astype(np.int64)
    params, maxima = [], []
    w0 = rng.integers(-1, 2, size=(F, 2, 3, 3)).astype(np.int64)
    params.append((w0, np.zeros(F, np.int64)))
    a = np.maximum(_conv_int(x, w0), 0)
    maxima.append(int(a.max()))
    for r in range(R):
        skip = a
        for half in range(2):
            w = (rng.random((F, F, 3, 3)) < DENSITY[F]).astype(np.int64) * rng.choice(np.array([-1, 1], np.int64), size=(F, F, 3, 3))
            pre = _conv_int(a, w) + (skip if half == 1 else 0)
            bound = _conv_int(a, np.abs(w)) + (skip if half == 1 else 0)   # sum of the |terms|: bounds every partial sum
            b = -np.quantile(pre.transpose(1, 0, 2, 3).reshape(F, -1), 0.9, axis=1, method="lower").astype(np.int64)
            assert (bound + np.abs(b)[None, :, None, None]).max() < 2**24, "a pre-sum reaches 2^24: pick another seed"
            a = np.maximum(pre + b[None, :, None, None], 0)
            params.append((w, b))
            maxima.append(int(a.max()))
    return params, maxima, a


def assert_f16_exact(a, what=""):
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a), f"{what}: an activation is not an f16 number: pick another seed"


_INTEGER = {}


def integer_net(F, R, V, seed=1):
    """(blob, layer maxima) of the integer net of shape (F, R, V) on positions(): integer_trunk's parameters under an identity
    BatchNorm (net_cases._prefold_), float heads scaled as net_cases.sharp_net scales them.  Built once per shape."""
    key = (F, R, V, seed)
    if key not in _INTEGER:
        own, enemy = positions()
        params, maxima, out = integer_trunk(F, R, seed, own, enemy)
        # every layer's activations are checked, not only the last one's: the restatement again, layer by layer
        x = C.planes(own, enemy).numpy().astype(np.int64)
        a = np.maximum(_conv_int(x, params[0][0]), 0)
        assert_f16_exact(a, "stem")
        for r in range(R):
            (w1, b1), (w2, b2) = params[1 + 2 * r], params[2 + 2 * r]
            y = np.maximum(_conv_int(a, w1) + b1[None, :, None, None], 0)
            assert_f16_exact(y, f"block {r} layer 1")
            a = np.maximum(_conv_int(y, w2) + b2[None, :, None, None] + a, 0)
            assert_f16_exact(a, f"block {r} layer 2")
        assert np.array_equal(a, out)

        def edit(net):
            convs = [net.stem] + [c for blk in net.res for c in blk]
            for cb, (w, b) in zip(convs, params):
                cb.conv.weight.copy_(torch.from_numpy(w).float())
                cb.conv.bias.copy_(torch.from_numpy(b).float())
        net = C.sharp_net(F, R, V, seed + 100, own, enemy, edit=edit)
        # the f64 graph of the module is the restatement (the blob holds exactly these parameters)
        t = C.trunk(C.graph(net), C.planes(own, enemy).double()).numpy()
        assert np.array_equal(t, a.astype(np.float64))
        C.assert_sharp(*C.reference(net, own, enemy), f"integer net {key}")   # (the runners repeat it on the outputs they compare against)
        _INTEGER[key] = (net.to_blob(), maxima)
    return _INTEGER[key]


def h(x):
    """Round-to-nearest-even to f16, carried on in the tensor's own dtype."""
    return x.to(torch.float16).to(x.dtype)


def layer_scale(w):
    """S_l of raz_net_build_f16x3: the power of two with max |w| * S in [2^14, 2^15) (w: the layer's float32 weights)."""
    mx = float(w.detach().abs().max())
    if mx == 0.0:
        return 2.0**15
    _, e = np.frexp(np.float32(mx))
    return 2.0 ** (15 - int(e))


def quantised_reference(net, own, enemy, device="cpu"):
    """(policy, value) of the SPECIFICATION of v3 in f64: h() after the stem's and every trunk layer's relu, trunk weights h(w S) / S,
    the skip operand the stored (quantised) activation, heads in f64.  `net`: a net_cases.sharp_net (BatchNorm folded)."""
    m = C.graph(net, torch.float64, device)
    with torch.no_grad():
        src_convs = [c for blk in net.res for c in blk]
        for cb, src in zip([c for blk in m.res for c in blk], src_convs):
            S = layer_scale(src.conv.weight)
            cb.conv.weight.copy_(h(src.conv.weight.detach().double().to(device) * S) / S)
        x = C.planes(own, enemy).double().to(device)
        x = h(torch.relu(m.stem(x)))
        for c1, c2 in m.res:
            x = h(torch.relu(c2(h(torch.relu(c1(x)))) + x))
        p = torch.relu(m.policy_conv(x)).flatten(1)
        p = torch.softmax(m.policy_fc(p), dim=1)
        v = torch.relu(m.value_conv(x)).flatten(1)
        v = torch.tanh(m.value_fc2(torch.relu(m.value_fc1(v))))
    return p.cpu().numpy(), v[:, 0].cpu().numpy()


# The kernel and the f64 restatement compute the same quantised graph, but the kernel accumulates in f32: a pre-activation that lies
# within an f32 rounding of the midpoint of two halfs rounds the other way, one f16 ulp instead of none.  Two f32 evaluations of one
# quantised 128x2 graph in different summation orders lay 1.0e-5 mean / 8e-4 max from its f64 evaluation, where the quantisation
# itself costs 3.7e-5 mean / 2.2e-3 max against the true graph: the kernel's distance from the true graph may pass the
# restatement's by that bounded share, and is held to the project's pair for a matrix-core accumulation (net_cases.F16X3_FACTOR:
# 4 x on the maximum, 2.5 x on the mean) with within_fp32_rule's floors.  An operand or indexing bug costs 1e-1.
def within_quantisation_rule(e_kernel, e_quant):
    return C.within_fp32_rule(e_kernel, e_quant, C.F16X3_FACTOR)


# v2 is within 1e-5 of the graph at its worst output; a mean distance above that shows single products, not v2 under another name
MIN_MEAN_ERROR = 1e-5


def net_that_overflows(F=128, R=1, V=64):
    """tests/test_engine_gpu.py test_net_f16x3_range_flag's net: Keras initialisers with the stem x 1e6, so that every row's stem
    activations leave the f16 range."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    net = ReversiNet(F, R, V).keras_init_(5)
    with torch.no_grad():
        net.stem.conv.weight.mul_(1.0e6)
    return net.to_blob()


def harvested_positions(n, seed):
    """tests/test_engine_gpu.py _harvested_positions: random playouts from the start, stopped at a random ply (oracle env = test
    infrastructure), from the mover's view."""
    import oracle as O
    rng = np.random.default_rng(seed)
    own, enemy = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    orc = O.load()
    for i in range(n):
        env = O.OrcEnv()
        orc.orc_env_reset(env)
        for _ in range(int(rng.integers(0, 58))):
            if env.done:
                break
            o, e = (env.black, env.white) if env.next_player == 1 else (env.white, env.black)
            legal = orc.orc_find_correct_moves(o, e)
            moves = [s for s in range(64) if legal >> s & 1]
            prev = (env.black, env.white, env.next_player)
            orc.orc_env_step(env, int(moves[rng.integers(0, len(moves))]))
            if env.done:   # keep the last live position
                orc.orc_env_update(env, prev[0], prev[1], prev[2])
                break
        own[i], enemy[i] = (env.black, env.white) if env.next_player == 1 else (env.white, env.black)
    return own, enemy


# include/raz.h raz_net_form over reserved 8: (filters, value_fc) -> form (negative: refused)
FORM_TABLE = [((128, 16192), 8), ((256, 8000), 8), ((256, 8001), 9), ((384, 1), 9), ((192, 7), -1), ((16, 16), 1)]
