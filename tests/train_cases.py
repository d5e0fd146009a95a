"""Shapes, batches, data and the f64 yardsticks shared by the training tests (tests/test_train_gpu.py, tests/test_train_host.py).

raznet-train-v1 is restated by agent/trainer.py's TorchTrainer over autograd; in f64 it is the reference, in
fp32 on the CPU it is the measure of what fp32 arithmetic costs on the same case.  An implementation X is compared

  * forward: per tensor, max and mean |X - f64| <= k x fp32 torch's own + the floors of net_cases.within_fp32_rule;
  * gradients: against the f64 graph in which every ReLU passes exactly where X's OWN forward output was positive (one ReLU whose
    input changes sign between precisions moves a gradient tensor by 2e-4 relative, a thousand times the rounding error), per
    tensor ||g_X - g_64|| / ||g_64|| <= k x fp32 torch's (against ITS masked f64 graph) + 1e-7;
  * conv biases ahead of BatchNorm (true gradient 0, fp32 residue 1e-8): ||g_X|| <= 10 x fp32 torch's residue norm.

SCALARS.  A tensor of ONE element (at these shapes: the value head's batch mean and variance, its BatchNorm's gamma and beta
gradients, value_out's bias gradient, the two losses) is one number, and fp32 torch's own error on it is a single sample: on an
MI355X it fell to 4e-9 on a loss of 1.0 and to 3e-9 relative on a gradient whose neighbours sit at 1e-6, a few times in 64 cases -
below the resolution of float32 arithmetic on that quantity - and the device, carrying ordinary fp32 error, then showed "ratios" of
12 to 85.  For such a tensor alone, fp32 torch's error is floored - before the factor k is applied - at ONE ULP OF FLOAT32 AT THE
MAGNITUDE OF THE TERMS THE QUANTITY IS SUMMED FROM, computed from the f64 graph alone, per tensor:
  batch mean      terms y_i:            ulp32(sqrt(var + mean^2))      (the RMS of y bounds the mean of |y_i| from above)
  batch variance  terms (y_i - m)^2:    ulp32(var)
  policy loss     terms the row losses: ulp32(loss)
  value loss      terms (v - z)^2 with v a float32 below 1: one ulp of v (2^-24) moves a row by 2 |v - z|: 2 sqrt(loss) 2^-24
  gradient sums   bn.beta = sum g, bn.gamma = sum g xhat, value_out.bias = sum d loss / d pre-tanh:
                  ulp32(sum |term|) / |sum term|   (relative, as the rule is)
A float32 sum cannot be expected closer to the exact one than one ulp of what it adds up; every tensor of two elements and more
is held to the rule as it stands.  The tests print the un-floored ratio beside the floored one and record both."""
import functools

import numpy as np
import torch

import net_cases

# the mini net, R > 1, the narrowest "wide" shape, F % 64 == 0 but F % 128 != 0
SHAPES = [(16, 1, 16), (32, 2, 7), (128, 1, 64), (192, 1, 32)]
# the edges of k_tconv's 4-position tile, of k_twgrad's 32 position splits and of a 64-row block
BATCHES = [1, 3, 4, 5, 31, 32, 33, 67]
L2 = 1e-4
# Measured on an MI355X (profiles/r7/train_step_accuracy.json): the worst ratio of the device's error to fp32 torch's own over
# every tensor of every case, rounded up to the next of {2, 4, 10}.
K_FORWARD = 10.0
K_GRAD = 10.0


def make_net(F, R, V):
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    return ReversiNet(F, R, V).keras_init_(3).randomize_bn_(4)


@functools.lru_cache(maxsize=None)
def data():
    """(own u64[N], enemy u64[N], policy f32[N,64], z i8[N]): net_cases.inputs() rows with sparse policies summing to 1 and z in {-1,0,1}."""
    own, enemy, _ = net_cases.inputs()
    rng = np.random.default_rng(11)
    n = len(own)
    policy = np.zeros((n, 64), np.float64)
    for i in range(n):
        k = int(rng.integers(1, 5))
        sq = rng.choice(64, size=k, replace=False)
        w = rng.random(k) + 0.1
        policy[i, sq] = w / w.sum()
    z = (np.arange(n) % 3 - 1).astype(np.int8)[rng.permutation(n)]
    return own, enemy, policy.astype(np.float32), z


def batch_rows(B, salt=0):
    """Row numbers of a batch: B distinct rows of data(), a pure function of (B, salt); the first row is one with z != 0, so that
    the value loss of the smallest batches is not that of a draw against an untrained value head (about 0)."""
    perm = np.random.default_rng((B, salt)).permutation(len(data()[0]))
    first = int(np.flatnonzero(data()[3][perm] != 0)[0])
    perm[[0, first]] = perm[[first, 0]]
    return perm[:B].astype(np.int64)


def torch_backward(net, idx, dtype, masks=None):
    """One backward of a TorchTrainer on the CPU: dict of everything the tests compare."""
    from reversi_alpha_zero_amd.agent.trainer import TorchTrainer
    t = TorchTrainer(net, dtype=dtype, l2=L2)
    t.relu_masks = masks
    losses = t.backward(*data(), idx)
    return {"acts": [a.double() for a in t.activations()], "mean": [m.double().cpu() for m in t.batch_mean],
            "var": [v.double().cpu() for v in t.batch_var], "losses": losses, "grads": {k: g.double() for k, g in t.gradients().items()},
            "abs_sums": t.abs_sums}


def masks_of(acts):
    return [a > 0 for a in acts]


def _f64(x):
    """A flat float64 tensor (a list of Python floats keeps its 53 bits)."""
    return (x.detach().double() if torch.is_tensor(x) else torch.tensor(np.asarray(x, dtype=np.float64))).reshape(-1)


def err(x, ref):
    d = (_f64(x) - _f64(ref)).abs()
    return float(d.max()), float(d.mean())


def is_scalar(ref):
    return _f64(ref).numel() == 1


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def forward_floor(kind, ref, mean=None, var=None):
    """The floor of fp32 torch's absolute error on a ONE-element forward tensor (module docstring); 0 for every other tensor."""
    if not is_scalar(ref):
        return 0.0
    r = float(_f64(ref)[0])
    if kind == "mean":
        return ulp32(np.sqrt(float(var) + float(mean) ** 2))
    if kind in ("var", "policy loss"):
        return ulp32(r)
    if kind == "value loss":
        return 2.0 * np.sqrt(r) * 2.0 ** -24
    return 0.0


def grad_floor(name, ref, abs_sums):
    """The floor of fp32 torch's relative error on a ONE-element gradient that is a plain sum over the batch; 0 otherwise."""
    if not is_scalar(ref) or name not in abs_sums:
        return 0.0
    return ulp32(float(abs_sums[name].reshape(-1)[0])) / abs(float(_f64(ref)[0]))


def floored(e32, floor):
    return (max(e32[0], floor), max(e32[1], floor))


def forward_ok(e, e32, k):
    return e[0] <= k * e32[0] + 1e-7 and e[1] <= k * e32[1] + 2e-8


def ratio(e, e32):
    """The k a tensor needs (0 when the floors alone cover it)."""
    need = lambda a, b, floor: 0.0 if a <= floor else (a - floor) / b if b > 0 else float("inf")
    return max(need(e[0], e32[0], 1e-7), need(e[1], e32[1], 2e-8))


def sharp_batch(net, B):
    """(row numbers, the f64 backward on them) of the first batch_rows(B, salt) whose f64 evaluation is not degenerate: every ReLU
    layer between 10 % and 90 % active, both losses above 0.05.  Chosen on the reference alone."""
    for salt in range(16):
        idx = batch_rows(B, salt)
        ref = torch_backward(net, idx, torch.float64)
        if min(ref["losses"]) > 0.05 and all(0.1 <= float((a > 0).double().mean()) <= 0.9 for a in ref["acts"]):
            break
    return idx, ref


def rel_l2(g, ref):
    return float((g.double() - ref).norm() / ref.norm())


def is_conv_bias(name):
    return name.startswith("conv") and name.endswith(".bias")


def layer_names(R):
    return [f"conv{i}" for i in range(2 * R + 3)] + ["dense_1"]
