"""Shapes, nets, inputs and the f64 reference shared by the net-kernel tests (tests/test_net_shapes_gpu.py, tests/test_net_emu.py).

raz_net_forward picks one of five kernel families from (filters F, value_fc V, raz_net.reserved) - include/raz.h raz_net_form.
SHAPES reaches every form and every edge of that choice; `sharp_net` builds a net whose f64 evaluation is not degenerate (a live
value head, a policy far from uniform), so that a tolerance against it measures the kernels and not the net; `inputs` adds the
boards where convolution indexing goes wrong (every square's off-board taps, empty, full, own/enemy overlap) to random positions."""
import numpy as np
import torch

# (F, R, V): every F in {16 .. 512}, R in {0, 1, 2} (10 at F = 256), V in {1, 7, 64, 1024, 1025, 4096} and the edges of the dispatch:
# V = 1024 / 1025 (k_net_mfma's cut-over), 3*64*F + 192 + V floats around 64 KB (k_net_wave in LDS or in scratch), F % 64 (wide),
# F % 128 (f16x3), 2*64*F + 192 + V floats around 160 KB (f16x3 with or without the in-forward repair)
SHAPES = [
    (16, 0, 1), (16, 1, 1025), (32, 2, 7), (48, 1, 64), (64, 1, 1024), (64, 0, 1025), (80, 2, 7), (80, 1, 1025),
    (96, 1, 64), (112, 0, 1), (128, 1, 64), (128, 0, 4096), (144, 1, 7), (192, 1, 1025), (256, 10, 64), (256, 1, 8192),
    (320, 1, 7), (384, 1, 32), (512, 2, 4096),
]
MAX_V = 16192   # include/raz.h RAZ_NET_MAX_VALUE_FC


def reserved_for(F):
    """The raz_net.reserved values that select a form of their own for F: 0 (by shape), 1 (k_net_wave), 2 (the matrix-core test
    variant: only where k_net_mfma runs), 4 (split-f16 trunk: F % 128 == 0)."""
    out = [0, 1]
    if F in (16, 32, 64):
        out.append(2)
    if F >= 128 and F % 128 == 0:
        out.append(4)
    return out


def _prefold_(net):
    """BatchNorm folded into the convolutions in place (the float32 rounding agent/model.py to_blob does), BN left as an exact
    identity (eps 0: to_blob's fold then multiplies by exactly 1) - the blob holds exactly the module's conv parameters."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    with torch.no_grad():
        for cb in [net.stem] + [c for blk in net.res for c in blk] + [net.policy_conv, net.value_conv]:
            w, b = ReversiNet._fold(cb)
            cb.conv.weight.copy_(w)
            cb.conv.bias.copy_(b)
            cb.bn.weight.fill_(1.0)
            cb.bn.bias.zero_()
            cb.bn.running_mean.zero_()
            cb.bn.running_var.fill_(1.0)
            cb.bn.eps = 0.0
    return net


def planes(own, enemy):
    """(n, 2, 8, 8) planes of (own, enemy) bitboards (uint64 numpy), bit i = square i: each plane from its own bits."""
    o = torch.from_numpy(np.asarray(own, np.uint64).view(np.int64))
    e = torch.from_numpy(np.asarray(enemy, np.uint64).view(np.int64))
    sh = torch.arange(64, dtype=torch.int64)
    return torch.stack([(o[:, None] >> sh) & 1, (e[:, None] >> sh) & 1], dim=1).reshape(-1, 2, 8, 8)


def graph(net, dtype=torch.float64, device="cpu"):
    """A copy of a _prefold_-ed net without its (identity) BatchNorm layers, in `dtype` on `device`: the graph of exactly the
    weights the kernels receive, evaluated in any precision."""
    import copy
    m = copy.deepcopy(net)
    for cb in [m.stem] + [c for blk in m.res for c in blk] + [m.policy_conv, m.value_conv]:
        cb.bn = torch.nn.Identity()
    return m.to(dtype).to(device).eval()


def trunk(net, x):
    with torch.no_grad():
        x = torch.relu(net.stem(x))
        for c1, c2 in net.res:
            x = torch.relu(c2(torch.relu(c1(x))) + x)
    return x


def sharp_net(F, R, V, seed, own, enemy, device="cpu", edit=None):
    """ReversiNet(F, R, V): Keras initialisers plus BatchNorm statistics, folded (_prefold_), then the heads scaled on the f64 trunk
    output of (own, enemy) so that the reference is not degenerate: the 1x1 head convolutions' biases put 70 % of their outputs
    above 0 and the value head's hidden units 95 % of theirs, the policy dense layer is scaled to a median per-row logit range of 6 (max / min probability ~400), the value output
    layer so that 95 % of the pre-tanh values lie in [-1.6, 1.6] around 0.  Every parameter stays a float32 the kernels receive as it is."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    net = _prefold_(ReversiNet(F, R, V).keras_init_(seed).randomize_bn_(seed + 1))
    if edit is not None:   # a change to the trunk's (folded) parameters before the heads are scaled
        with torch.no_grad():
            edit(net)
    a = trunk(graph(net, device=device), planes(own, enemy).double().to(device))
    with torch.no_grad():
        for cb in (net.policy_conv, net.value_conv):
            w = cb.conv.weight.double().to(device)
            pre = torch.einsum("nchw,oc->nohw", a, w[:, :, 0, 0])
            q = torch.quantile(pre.transpose(0, 1).reshape(w.shape[0], -1), 0.3, dim=1)
            cb.conv.bias.copy_((-q).float().cpu())
        ph = torch.relu(torch.einsum("nchw,oc->nohw", a, net.policy_conv.conv.weight.double().to(device)[:, :, 0, 0])
                        + net.policy_conv.conv.bias.double().to(device)[None, :, None, None]).flatten(1)
        logits = ph @ net.policy_fc.weight.double().to(device).t()
        spread = float((logits.max(1).values - logits.min(1).values).median())
        if spread > 0:
            net.policy_fc.weight.mul_(6.0 / spread)
        vh = torch.relu(torch.einsum("nchw,oc->nohw", a, net.value_conv.conv.weight.double().to(device)[:, :, 0, 0])
                        + net.value_conv.conv.bias.double().to(device)[None, :, None, None]).flatten(1)
        pre1 = vh @ net.value_fc1.weight.double().to(device).t()
        net.value_fc1.bias.copy_((-torch.quantile(pre1, 0.05, dim=0)).float().cpu())
        h1 = torch.relu(pre1 + net.value_fc1.bias.double().to(device))
        z = h1 @ net.value_fc2.weight.double().to(device)[0]
        med = float(z.median())
        q95 = float(torch.quantile((z - med).abs(), 0.95))
        if q95 > 0:
            k = 1.6 / q95
            net.value_fc2.weight.mul_(k)
            net.value_fc2.bias.fill_(-k * med)
    return net


def reference(net, own, enemy, device="cpu", dtype=torch.float64):
    """(policy (n, 64), value (n,)) of `net` - a ReversiNet whose BN is folded (sharp_net) - in `dtype`, as float64 numpy."""
    m = graph(net, dtype, device)
    with torch.no_grad():
        p, v = m(planes(own, enemy).to(dtype).to(device))
    return p.double().cpu().numpy(), v[:, 0].double().cpu().numpy()


def assert_sharp(policy, value, what=""):
    """The guard every comparison starts with: the f64 reference is not degenerate."""
    v = np.asarray(value)
    assert v.std() >= 0.2, f"{what}: value std {v.std():.3g}"
    assert (v == 0).mean() <= 0.1, f"{what}: {(v == 0).mean():.0%} of values exactly 0"
    assert (np.abs(v) > 0.97).mean() <= 0.1, f"{what}: {(np.abs(v) > 0.97).mean():.0%} of values saturated"
    p = np.asarray(policy)
    ratio = float(np.median(p.max(1) / np.maximum(p.min(1), 1e-300)))
    assert ratio >= 50, f"{what}: median policy max/min {ratio:.3g}"


def inputs(n_random=48, seed=0):
    """(own, enemy, names) uint64 arrays: random positions of random density, the empty board, a full board, the 64 single-disc
    boards of each colour (every square's off-board taps), and rows whose own and enemy overlap (the kernels form each plane from
    its own bits; the graph defines those rows too)."""
    rng = np.random.default_rng(seed)
    bits = lambda p, k: (rng.random((k, 64)) < p).astype(np.uint64) @ (np.uint64(1) << np.arange(64, dtype=np.uint64))
    own, enemy, names = [], [], []
    for i in range(n_random):
        fill = bits(rng.uniform(0.1, 1.0), 1)[0]
        o = fill & rng.integers(0, 2**64, dtype=np.uint64)
        own.append(o); enemy.append(fill & ~o); names.append("random")
    own.append(np.uint64(0)); enemy.append(np.uint64(0)); names.append("empty")
    full = rng.integers(0, 2**64, dtype=np.uint64)
    own.append(full); enemy.append(~full); names.append("full")
    for sq in range(64):
        own.append(np.uint64(1) << np.uint64(sq)); enemy.append(np.uint64(0)); names.append(f"own@{sq}")
    for sq in range(64):
        own.append(np.uint64(0)); enemy.append(np.uint64(1) << np.uint64(sq)); names.append(f"enemy@{sq}")
    for k in range(6):
        o, e = rng.integers(0, 2**64, size=2, dtype=np.uint64)
        own.append(o); enemy.append(e | (o & rng.integers(0, 2**64, dtype=np.uint64))); names.append("overlap")
    ones = ~np.uint64(0)
    own.append(ones); enemy.append(ones); names.append("overlap all")
    own.append(ones); enemy.append(np.uint64(1) << np.uint64(63)); names.append("overlap corner")
    return np.array(own, np.uint64), np.array(enemy, np.uint64), names


def oracle_rows(names):
    """At most 3 rows per shape for the C oracle (a few seconds a row at the widest shapes): first, last, a corner single-disc board."""
    return [0, len(names) - 1, names.index("own@7")]


def errors(policy, value, ref_policy, ref_value):
    """(max, mean) |difference| over every output (64 probabilities + the value) of every row."""
    d = np.concatenate([np.abs(np.asarray(policy, np.float64) - ref_policy).ravel(), np.abs(np.asarray(value, np.float64) - ref_value)])
    return float(d.max()), float(d.mean())


# The exact-f32 forms compute raznet-forward-v1's chains: ONE sequential fmaf chain per output (9 F terms for a convolution, V for
# the value output).  fp32 torch sums in blocks, so its error grows more slowly with F: measured on an MI355X against f64 on the
# sharp nets here, the exact forms (all of them bit-identical to each other and to the C oracle) are 1-2 x torch's error up to
# F = 112, 3 x at F = 128 .. 384 and 5.9 x (max) / 7 x (mean) at F = 512 - a property of the chain order the contract fixes, not
# of a kernel.  Those forms are held to 10 x.  The split-f16 trunk accumulates each output in one matrix-core accumulator over
# all 9 F products too: 1.5-2 x torch's error, 2.9 x on the maximum at F = 384; it is held to 2.5 x (mean) and 4 x (max).  Every
# indexing or operand bug these tests look for costs 1e-3 or more (a dropped lo x hi product: 3e-3).
EXACT_FACTOR = (10.0, 10.0)
F16X3_FACTOR = (4.0, 2.5)


def within_fp32_rule(err, err32, factor=(2.5, 2.5)):
    """tests/test_engine_gpu.py test_net_f16x3_accuracy_on_4096_positions_of_three_nets' rule, per case: max and mean |difference|
    against f64 at most factor (2.5, 2.5) x fp32 torch's own, plus 1e-7 (max) / 2e-8 (mean)."""
    return err[0] <= factor[0] * err32[0] + 1e-7 and err[1] <= factor[1] * err32[1] + 2e-8
