"""Shapes, batches, data, the f64 yardsticks and the SCENARIOS shared by the training tests: tests/test_train_gpu.py runs them on the
device (agent/trainer.py's DeviceTrainer), tests/test_train_emu.py on the wave-emulator build of the same, unchanged
csrc/raz_train.hip (tests/emu_util.py's EmuTrainer); tests/test_train_host.py uses the data and the rules.  A scenario takes a
trainer factory `make(net, max_batch)` - with `make.driver`, the name the records carry, and `make.raw`, the raw C entries and
memory of that driver (lib, stream(), last_error(), alloc(nbytes) / put(array) -> an object with .ptr, sync()) - and knows nothing of
where the kernels execute.  The emulator's double exp / log / tanh / sqrt are libm's, not the device library's: neither driver's
bits are pinned to the other's, both are held to the same rules against f64.

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
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import net_cases

# the mini net, R > 1, the narrowest "wide" shape, F % 64 == 0 but F % 128 != 0
SHAPES = [(16, 1, 16), (32, 2, 7), (128, 1, 64), (192, 1, 32)]
# the edges of k_tconv's 4-position tile, of k_twgrad's 32 position splits and of a 64-row block
BATCHES = [1, 3, 4, 5, 31, 32, 33, 67]
# Edges the shapes above do not reach: F % 64 = 48 (three working waves of k_twgrad's four), F = 80 (a second, partly filled group
# of 64 output channels: blockIdx.x = 1, one working wave), the shipped value_fc_size 256 (value_out's bias gradient is thread 0 of a
# second workgroup of k_dense_wgrad) - at batches inside and across k_tconv's 4-position tile and the 32 splits.
EDGE_SHAPES = [(48, 1, 16), (80, 1, 7), (16, 1, 256)]
EDGE_BATCHES = [3, 5, 33]
# B > 256: the strided loop of k_loss_sum, more than eight positions per split of k_twgrad
LONG_BATCHES = [256, 257]
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


def long_batch_rows(B):
    """Row numbers of a batch of B > len(data()) rows: every row once, then B - len(data()) of them a second time (repeated rows are
    legitimate input: the `opt` worker draws its batches from a data set that may hold a position many times)."""
    n = len(data()[0])
    assert B > n
    return np.concatenate([batch_rows(n, 0), batch_rows(B - n, 1)])


def torch_backward(net, idx, dtype, masks=None):
    """One backward of a TorchTrainer on the CPU: dict of everything the tests compare."""
    from reversi_alpha_zero_amd.agent.trainer import TorchTrainer
    t = TorchTrainer(net, dtype=dtype, l2=L2)
    t.relu_masks = masks
    losses = t.backward(*data(), idx)
    return {"acts": [a.double() for a in t.activations()], "mean": [m.double().cpu() for m in t.batch_mean],
            "var": [v.double().cpu() for v in t.batch_var], "losses": losses, "grads": {k: g.double() for k, g in t.gradients().items()},
            "abs_sums": t.abs_sums, "policy": t.policy.double().cpu(), "value": t.value.double().cpu()}


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


# ---------------------------------------------------------------------------------------------------------------------- scenarios
RAZ_EINVAL, RAZ_ESTATE = -1, -4
READ_GRADS, READ_ACT, READ_MEAN, READ_VAR, READ_HIDDEN, READ_POLICY, READ_VALUE = range(7)


class Buf:
    """Memory of a driver: .ptr for the C entries, .host() -> its bytes now as a numpy array, .keep whatever owns it."""

    def __init__(self, ptr, keep, host):
        self.ptr, self.keep, self.host = ptr, keep, host


def record(driver, kind, case, worst, unfloored):
    path = os.environ.get("RAZ_TRAIN_ACCURACY_JSON")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"driver": driver, "kind": kind, "case": list(case), "worst_ratio": worst[0], "tensor": worst[1],
                                "scalars_unfloored": unfloored}) + "\n")


def degenerate_net():
    """The mini net with what a trained net meets and make_net never does: an output channel of the stem whose kernel is 0 (constant
    over the batch: variance exactly 0), a channel whose ReLU never passes (beta -50), and heads 40 times as sharp (a saturated softmax,
    where p + 1e-7 is the constant's; tanh at +-1 in float32)."""
    net = make_net(16, 1, 16)
    t = dict(net.train_tensors())
    with torch.no_grad():
        t["conv0.kernel"][3].zero_()
        t["bn1.beta"][5] = -50.0
        t["policy_out.kernel"].mul_(40.0)
        t["value_out.kernel"].mul_(40.0)
    return net


_cases = {}


def case(make, F, R, V, B, rows="sharp"):
    """One backward of the driver's trainer, of fp32 torch and of the three f64 graphs (plain, masked as the driver, masked as fp32
    torch), computed once per process.  rows: "sharp" (sharp_batch), "long" (long_batch_rows), "degenerate" (degenerate_net)."""
    key = (make.driver, F, R, V, B, rows)
    if key not in _cases:
        net = degenerate_net() if rows == "degenerate" else make_net(F, R, V)
        if rows == "sharp":
            idx, f64 = sharp_batch(net, B)
        else:
            idx = long_batch_rows(B) if rows == "long" else batch_rows(B)
            f64 = torch_backward(net, idx, torch.float64)
        dev = make(net, B)
        before = dev.get_blob()
        losses = dev.backward(*data(), idx)
        mean, var = dev.batch_stats()
        d = {"acts": dev.activations(), "mean": mean, "var": var, "losses": losses, "grads": dev.gradients(),
             "untouched": bool(np.array_equal(before.view(np.uint32), dev.get_blob().view(np.uint32)))}
        dev.close()
        t32 = torch_backward(net, idx, torch.float32)
        _cases[key] = {"net": net, "dev": d, "t32": t32, "f64": f64,
                       "f64_as_dev": torch_backward(net, idx, torch.float64, masks_of(d["acts"])),
                       "f64_as_t32": torch_backward(net, idx, torch.float64, masks_of(t32["acts"]))}
    return _cases[key]


def forward_rule(make, c, case_id, guards=True):
    dev, t32, ref = c["dev"], c["t32"], c["f64"]
    assert dev["untouched"], "raz_trainer_backward changed the state"
    names = layer_names(case_id[1])
    if guards:   # a comparison of dead or saturated layers shows nothing
        for name, a in zip(names, ref["acts"]):
            on = float((a > 0).double().mean())
            assert 0.1 <= on <= 0.9, f"{name}: {on:.0%} of its ReLUs active in f64"
        assert min(ref["losses"]) > 0.05, ref["losses"]
    bad, worst = [], (0.0, "")
    items = [(f"{n} relu", "relu", x, y, r, None, None) for n, x, y, r in zip(names, dev["acts"], t32["acts"], ref["acts"])]
    items += [(f"{n} batch mean", "mean", x, y, r, r, v) for n, x, y, r, v in zip(names, dev["mean"], t32["mean"], ref["mean"], ref["var"])]
    items += [(f"{n} batch variance", "var", x, y, r, None, None) for n, x, y, r in zip(names, dev["var"], t32["var"], ref["var"])]
    items += [(f"{n} loss", f"{n} loss", [dev["losses"][i]], [t32["losses"][i]], [ref["losses"][i]], None, None)
              for i, n in enumerate(("policy", "value"))]
    unfloored = {}
    for name, kind, x, y, r, m, v in items:
        e, raw = err(x, r), err(y, r)
        floor = forward_floor(kind, r, m, v)   # 0 unless the tensor is ONE number (module docstring, SCALARS)
        e32 = floored(raw, floor)
        k = ratio(e, e32)
        note = ""
        if is_scalar(r):
            unfloored[name] = ratio(e, raw)
            note = f"   (scalar: fp32 torch's own {raw[0]:.3g}, un-floored ratio {unfloored[name]:.2f})"
        print(f"{name:28s} {make.driver} max {e[0]:.3g} mean {e[1]:.3g}   fp32 torch max {e32[0]:.3g} mean {e32[1]:.3g}   ratio {k:.2f}{note}")
        worst = max(worst, (k, name))
        if not forward_ok(e, e32, K_FORWARD):
            bad.append((name, e, e32))
    record(make.driver, "forward", case_id, worst, unfloored)
    assert not bad, bad


def gradient_rule(make, c, case_id):
    bad, worst = [], (0.0, "")
    unfloored = {}
    for name, ref in c["f64_as_dev"]["grads"].items():
        g, g32, ref32 = c["dev"]["grads"][name], c["t32"]["grads"][name], c["f64_as_t32"]["grads"][name]
        assert tuple(g.shape) == tuple(ref.shape), name
        if is_conv_bias(name):   # true gradient 0: absolute, against fp32 torch's residue
            n, n32 = float(g.double().norm()), float(g32.norm())
            print(f"{name:28s} |g| {make.driver} {n:.3g}   fp32 torch {n32:.3g}")
            if not n <= 10 * n32:
                bad.append((name, n, n32))
            continue
        assert float(ref.norm()) > 1e-6, f"{name}: the f64 gradient is (nearly) zero, the case shows nothing"
        r, r32 = rel_l2(g, ref), rel_l2(g32, ref32)
        ratio_to = lambda own: max(0.0, (r - 1e-7) / own) if own > 0 else (0.0 if r <= 1e-7 else float("inf"))
        note = ""
        if is_scalar(ref):   # ONE number: fp32 torch's error floored at one ulp of what the sum adds up (module docstring, SCALARS)
            unfloored[name] = ratio_to(r32)
            note = f"   (scalar: fp32 torch's own {r32:.3g}, un-floored ratio {unfloored[name]:.2f})"
            r32 = max(r32, grad_floor(name, ref, c["f64_as_dev"]["abs_sums"]))
        k = ratio_to(r32)
        print(f"{name:28s} relative L2 {make.driver} {r:.3g}   fp32 torch {r32:.3g}   ratio {k:.2f}{note}")
        worst = max(worst, (k, name))
        if not r <= K_GRAD * r32 + 1e-7:
            bad.append((name, r, r32))
    record(make.driver, "gradients", case_id, worst, unfloored)
    assert not bad, bad


def degenerate_guards_and_exact_values(make, c):
    """What tests/test_train_*.py assert on the degenerate case beside the two rules (which run on it with their constants unchanged,
    the usual guards replaced by these, on the f64 graph alone)."""
    ref, dev, net = c["f64"], c["dev"], c["net"]
    sharp = float(ref["policy"].max(1).values.mean())
    flat = int((ref["value"].abs() > 0.999).sum())
    print(f"f64: mean max_a p {sharp:.3f}, {flat} of {len(ref['value'])} rows with |v| > 0.999, variance of conv0[3] "
          f"{float(ref['var'][0][3]):.3g}, conv1[5] active {int((ref['acts'][1][:, 5] > 0).sum())} times")
    assert sharp >= 0.9 and 4 * flat >= len(ref["value"])
    assert float(ref["var"][0][3]) < 1e-20 and not bool((ref["acts"][1][:, 5] > 0).any())
    t = dict(net.train_tensors())
    # a channel that is constant over the batch: its f64 sums are exact, so the variance is 0 and the output the ReLU of beta
    assert float(dev["var"][0][3]) == 0.0
    beta = np.float32(t["bn0.beta"][3].item())
    assert np.array_equal(dev["acts"][0][:, 3].numpy(), np.full((33, 8, 8), max(beta, np.float32(0)), np.float32))
    # a channel whose ReLU never passes: no gradient reaches its BatchNorm, its kernel's is the regulariser's alone
    g = dev["grads"]
    assert float(g["bn1.gamma"][5]) == 0.0 and float(g["bn1.beta"][5]) == 0.0
    want = (np.float32(2.0) * np.float32(L2)) * t["conv1.kernel"][5].detach().numpy().astype(np.float32)   # k_twgrad_fold: 0 + (2.0f * l2) * w
    assert want.dtype == np.float32 and np.array_equal(g["conv1.kernel"][5].numpy().view(np.uint32), want.view(np.uint32))
    assert all(np.isfinite(x) for x in dev["losses"]), dev["losses"]


def _updates(state, ref, init):
    """{tensor: ||w - w_64|| / ||w_64 - w_init||}, conv biases ahead of BatchNorm as max |w - w_64| under 'abs'."""
    rel, absd = {}, {}
    for name, w64 in ref.items():
        base = name[len("momentum."):] if name.startswith("momentum.") else name
        d = (state[name].double() - w64.double())
        if is_conv_bias(base):
            absd[name] = float(d.abs().max())
        else:
            moved = float((w64.double() - init[name].double()).norm())
            assert moved > 0, f"{name} did not move in f64: the case shows nothing"
            rel[name] = float(d.norm()) / moved
    return rel, absd


def eight_steps_track_the_f64_trainer(make, F, R, V, B):
    """Eight steps at lr 1e-2 with momentum, the same batches as an f64 TorchTrainer: every tensor of the state (moving statistics
    and momentum buffers included) stays within 1e-2 of ITS OWN UPDATE of the f64 trainer's, conv biases ahead of BatchNorm within
    1e-5 absolutely.  fp32 torch on the CPU stays within 3e-4 and 5e-7; a wrong momentum, update order or BatchNorm momentum moves
    a tensor by tens of percent of its update."""
    from reversi_alpha_zero_amd.agent.trainer import TorchTrainer
    net = make_net(F, R, V)
    trainers = {"f64": TorchTrainer(net, dtype=torch.float64, l2=L2), "fp32 torch": TorchTrainer(net, dtype=torch.float32, l2=L2),
                make.driver: make(net, B)}
    init = {k: v.clone() for k, v in trainers["f64"].state().items()}
    for step in range(8):
        idx = batch_rows(B, salt=step)
        for t in trainers.values():
            t.step(*data(), idx, 1e-2)
    ref = trainers["f64"].state()
    for who in ("fp32 torch", make.driver):
        rel, absd = _updates(trainers[who].state(), ref, init)
        w, a = max(rel, key=rel.get), max(absd, key=absd.get)
        print(f"{who:10s} worst relative {rel[w]:.3g} ({w})   worst conv-bias |difference| {absd[a]:.3g} ({a})")
        if who == make.driver:
            assert not {k: v for k, v in rel.items() if not v <= 1e-2}
            assert not {k: v for k, v in absd.items() if not v <= 1e-5}
    trainers[make.driver].close()


def two_trainers_hold_the_same_bytes(make, F, R, V, B=67):
    net = make_net(F, R, V)
    blobs = []
    for _ in range(2):
        t = make(net, B)
        for step in range(3):
            t.step(*data(), batch_rows(B, salt=step), 1e-2)
        blobs.append(t.get_blob())
        t.close()
    assert not np.array_equal(blobs[0], net.to_train_blob()), "three steps changed nothing"
    assert np.array_equal(blobs[0].view(np.uint32), blobs[1].view(np.uint32))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def the_batch_size_alone_fixes_the_bytes(make, F, R, V):
    """the order of every sum depends on (shape, batch size) alone.  One trainer with room for 67 rows steps through
    batches of changing size - as the `opt` worker does at the end of every epoch - with the rows of larger batches left behind in
    its saved tensors, gradient buffers, partial sums and per-row losses, and S = min(B, 32) moving; before each step its state goes
    to a fresh trainer with max_batch = B, which takes the same step.  The two states are the same bits after every step, and so
    are the gradients and losses of a backward at B = 5 after a step at B = 67."""
    net = make_net(F, R, V)
    big = make(net, 67)
    for k, B in enumerate((67, 5, 33, 1, 32, 4, 67)):
        idx = batch_rows(B, salt=k)
        blob = big.get_blob()
        fresh = make(net, B)
        fresh.set_blob(blob)
        if k == 1:
            losses = [t.backward(*data(), idx) for t in (big, fresh)]
            assert _same_bits(np.float32(losses[0]), np.float32(losses[1])), losses
            ga, gb = big.gradients(), fresh.gradients()
            assert not [n for n in ga if not _same_bits(ga[n].numpy(), gb[n].numpy())]
            assert any(float(g.abs().max()) > 0 for g in ga.values())
        losses = [t.step(*data(), idx, 1e-2) for t in (big, fresh)]
        a, b = big.get_blob(), fresh.get_blob()
        fresh.close()
        assert not _same_bits(a, blob), f"step {k} (B = {B}) changed nothing"
        assert _same_bits(np.float32(losses[0]), np.float32(losses[1])), (k, B, losses)
        assert _same_bits(a, b), f"step {k}: B = {B} in a trainer of max_batch 67 and in one of max_batch {B} differ in {int((a.view(np.uint32) != b.view(np.uint32)).sum())} words"
    big.close()


def abi_guards_refuse_and_leave_the_state_untouched(make):
    raw = make.raw
    lib, s = raw.lib, raw.stream()
    assert lib.raz_trainer_bytes(24, 1, 16, 8) == 0 and lib.raz_trainer_state_bytes(24, 1, 16) == 0
    need = lib.raz_trainer_bytes(16, 1, 16, 8)
    ws = raw.alloc(need + 256)
    h = ctypes.c_void_p()
    assert lib.raz_trainer_create(24, 1, 16, 8, ws.ptr, need, ctypes.byref(h), s) == -1 and not h.value      # F % 16 != 0
    assert lib.raz_trainer_create(16, 1, 16, 8, ws.ptr, need - 1, ctypes.byref(h), s) == -1 and not h.value  # one byte short
    assert lib.raz_trainer_create(16, 1, 16, 8, ws.ptr + 4, need, ctypes.byref(h), s) == -1 and not h.value  # misaligned
    assert lib.raz_trainer_create(16, 1, 16, 8, None, need, ctypes.byref(h), s) == -1 and not h.value
    assert "raz_trainer_create" in raw.last_error()
    t = make(make_net(16, 1, 16), 8)
    own, enemy, policy, z = (raw.put(a) for a in data())
    idx = raw.put(np.arange(9, dtype=np.int32))
    losses, before = raw.put(np.zeros(2, np.float32)), t.get_blob()
    a = [own.ptr, enemy.ptr, policy.ptr, z.ptr, idx.ptr]

    def step(args, B, out=losses.ptr):
        return lib.raz_trainer_step(t.handle, *args, B, 1e-2, L2, out, s)
    assert step(a, 0) == -1 and step(a, 9) == -1                       # B = 0, B > max_batch
    for i in range(5):                                                 # a NULL array
        assert step(a[:i] + [None] + a[i + 1:], 4) == -1
    assert step(a, 4, None) == -1
    assert step([a[0] + 4] + a[1:], 4) == -1 and step([a[0], a[1] + 4] + a[2:], 4) == -1   # misaligned bitboards
    assert step(a[:2] + [a[2] + 2] + a[3:], 4) == -1 and step(a[:4] + [a[4] + 2], 4) == -1  # misaligned policy / idx
    assert lib.raz_trainer_backward(t.handle, *a, 9, L2, losses.ptr, s) == -1
    assert lib.raz_trainer_set_state(t.handle, ws.ptr, before.nbytes - 4, s) == -1
    assert lib.raz_trainer_read(t.handle, 99, 0, ws.ptr, 4, s) == -1
    raw.sync()
    assert np.array_equal(before.view(np.uint32), t.get_blob().view(np.uint32)), "a refused call changed the state"
    assert step(a, 4) == 0
    raw.sync()
    assert not np.array_equal(before.view(np.uint32), t.get_blob().view(np.uint32))
    t.close()
    with pytest.raises(ValueError):
        make(make_net(24, 1, 16), 8)


def reads_are_refused_before_a_step_and_at_a_wrong_size(make):
    """raz_trainer_read: what depends on the last batch (an activation, dense_1's output, the policy, the value) is RAZ_ESTATE before
    any step, whatever the size given; a byte count one float off the tensor's is RAZ_EINVAL; neither writes a byte of the output
    or of the state."""
    raw = make.raw
    lib, s = raw.lib, raw.stream()
    F, R, V, MB, B = 16, 1, 16, 8, 5
    t = make(make_net(F, R, V), MB)
    before = t.get_blob()
    np_floats = (before.size - sum(x.numel() for _, x in make_net(F, R, V).stat_tensors())) // 2
    room = MB * F * 64 + np_floats + 1
    mark = np.full(room, 7.0, np.float32)
    out = raw.put(mark)
    read = lambda which, layer, floats: lib.raz_trainer_read(t.handle, which, layer, out.ptr, 4 * floats, s)
    batch_sized = lambda b: [(READ_ACT, 0, b * F * 64), (READ_ACT, 2 * R + 1, b * 2 * 64), (READ_ACT, 2 * R + 2, b * 64),
                             (READ_HIDDEN, 0, b * V), (READ_POLICY, 0, b * 64), (READ_VALUE, 0, b)]
    for b in (0, 1, MB):
        for which, layer, n in batch_sized(b):
            assert read(which, layer, n) == RAZ_ESTATE, (which, layer, n)
    assert "no step has run" in raw.last_error()
    fixed = [(READ_GRADS, 0, np_floats), (READ_MEAN, 0, F), (READ_VAR, 2 * R + 1, 2), (READ_MEAN, 2 * R + 2, 1)]
    for which, layer, n in fixed:
        assert read(which, layer, n - 1) == RAZ_EINVAL and read(which, layer, n + 1) == RAZ_EINVAL, (which, layer, n)
    raw.sync()
    assert np.array_equal(out.host().view(np.uint32), mark.view(np.uint32)), "a refused read wrote its output"
    assert _same_bits(before, t.get_blob()), "a refused read changed the state"
    t.step(*data(), batch_rows(B), 1e-2)
    after = t.get_blob()
    for which, layer, n in batch_sized(B) + fixed:
        assert read(which, layer, n - 1) == RAZ_EINVAL and read(which, layer, n + 1) == RAZ_EINVAL, (which, layer, n)
    assert "size does not match" in raw.last_error()
    raw.sync()
    assert np.array_equal(out.host().view(np.uint32), mark.view(np.uint32)), "a refused read wrote its output"
    for which, layer, n in batch_sized(B) + fixed:
        assert read(which, layer, n) == 0, (which, layer, n)
    raw.sync()
    assert _same_bits(after, t.get_blob()), "a read changed the state"
    t.close()
