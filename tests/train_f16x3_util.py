"""Trainer factories of raznet-train-v2 (precision "f16x3": csrc/raz_train_f16x3.h) for the scenarios of tests/train_cases.py: on the
wave emulator (EmuTrainerF16x3: DeviceTrainer(precision="f16x3") on the emulator's backend) and on the device
(DeviceTrainer(precision="f16x3")).  The records they write carry the drivers "emu-f16x3" / "gpu-f16x3"."""
import ctypes

import numpy as np

import emu_util
import train_cases as tc

RAZ_TRAIN_F32, RAZ_TRAIN_F16X3 = 0, 1


class EmuTrainerF16x3(emu_util.EmuTrainer):
    """emu_util.EmuTrainer at precision "f16x3": DeviceTrainer's own constructor, raz_trainer_bytes2 / raz_trainer_create2."""

    def __init__(self, net, max_batch, l2=1e-4):
        super().__init__(net, max_batch, l2=l2, precision="f16x3")


EmuTrainerF32Via2 = emu_util.EmuTrainer   # precision 0 through the `...2` entries (what raz_trainer_create makes)


class EmuTrainerV1Entry(emu_util.EmuTrainer):
    """The trainer made again in its workspace by raz_trainer_create, the entry without a precision; every other entry is the same."""

    def __init__(self, net, max_batch, l2=1e-4):
        super().__init__(net, max_batch, l2=l2)
        self.close()
        self.handle = ctypes.c_void_p()
        assert self.workspace.numel() == self.lib.raz_trainer_bytes(self.F, self.R, self.V, self.max_batch)
        self._launch("raz_trainer_create", self.F, self.R, self.V, self.max_batch, self.workspace.data_ptr(), self.workspace.numel(),
                     ctypes.byref(self.handle))
        self.from_net(net)


class _EmuRaw:
    stream = staticmethod(lambda: None)
    sync = staticmethod(lambda: None)

    @property
    def lib(self):
        return emu_util.load_train()

    def last_error(self):
        return (self.lib.raz_last_error() or b"").decode()

    def alloc(self, nbytes):
        keep, ptr = emu_util.aligned(nbytes)
        return tc.Buf(ptr, keep, lambda: keep.copy())

    def put(self, a):
        a = np.array(a, copy=True, order="C")
        return tc.Buf(a.ctypes.data, a, lambda: a.copy())


def make_emu(net, max_batch):
    return EmuTrainerF16x3(net, max_batch, l2=tc.L2)


make_emu.driver = "emu-f16x3"
make_emu.raw = _EmuRaw()

DEV = "cuda:0"


def make_gpu(net, max_batch):
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
    return DeviceTrainer(net, max_batch=max_batch, device=DEV, l2=tc.L2, precision="f16x3")


make_gpu.driver = "gpu-f16x3"


# Worst ratio of v2's error to fp32 torch's own over every tensor of every case of tests/test_train_f16x3_gpu.py, measured on an
# MI355X (profiles/r10/train_f16x3_accuracy_gpu.json) and rounded up to the next of {10, 20, 40, 100}.  The ceiling is derived, not
# measured: a split operand keeps 22 bits, a product's relative error is at most 3 x 2^-22 = 12 x an f32 rounding, and exact f32 (v1)
# sits at 6.4 - a worst ratio above 100 is a bug, never a constant.
K_FORWARD = 10.0   # measured 7.6 (conv3 batch variance, 80x1x7 at 33 rows)
K_GRAD = 20.0      # measured 11.8 (dense_1.bias, 128x1x64 at ONE row, where fp32 torch's own error fell to 3e-8); 7.7 the next case


def use_v2_constants(monkeypatch):
    monkeypatch.setattr(tc, "K_FORWARD", K_FORWARD)
    monkeypatch.setattr(tc, "K_GRAD", K_GRAD)


def trunk_differs_and_precisions_read_back(make_v2, make_v1, precision_of):
    """A v2 and a v1 trainer with the same state and batch: raz_trainer_precision 1 / 0, the stem's activations (v1's own kernels in
    both) are the same bits and at least one activation of every trunk layer differs."""
    net = tc.make_net(16, 1, 16)
    idx = tc.batch_rows(5)
    acts = []
    for make, want in ((make_v2, RAZ_TRAIN_F16X3), (make_v1, RAZ_TRAIN_F32)):
        t = make(net, 5)
        assert precision_of(t) == want
        t.backward(*tc.data(), idx)
        acts.append([a.numpy().copy() for a in t.activations()])
        t.close()
    same = [bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))) for a, b in zip(*acts)]
    assert same[0], "the stem is v1's kernel in both precisions"
    assert not same[1] and not same[2], same
    for a, b in zip(*acts):
        assert float(np.abs(a - b).max()) < 1e-4


# ---- a batch whose output gradients one row dominates ---------------------------------------------------------------------------


def _skewed(hot_i):
    """The mini net with a value head 300 times flatter (flatter still, and the f64 gradients of the value head's BatchNorm fall below the 1e-6 that
    tc.gradient_rule asks of a case), and tc.data() with the targets of the batch's rows replaced: every row
    but one is given the net's own f64 policy and z = 0 (its gradient at the logits vanishes, at the value 2 v / B with |v| of a few 1e-4),
    row hot_i the whole policy target on the square the net likes least and z = -1 (gradients of order 1 / B)."""
    import torch
    from reversi_alpha_zero_amd.agent.trainer import TorchTrainer
    net = tc.make_net(16, 1, 16)
    t = dict(net.train_tensors())
    with torch.no_grad():
        t["value_out.kernel"].mul_(3e-3)
        t["value_out.bias"].mul_(3e-3)
    idx = tc.batch_rows(len(tc.data()[0]))   # every row of the data set: the more rows, the less one row's gradient leaks into the others through BatchNorm
    own, enemy, policy, z = (a.copy() for a in tc.data())
    tr = TorchTrainer(net, dtype=torch.float64, l2=tc.L2)
    tr.backward(own, enemy, policy, z, idx)
    p = tr.policy.cpu().numpy()
    policy[idx] = p.astype(np.float32)
    z[idx] = 0
    hot = idx[hot_i]
    policy[hot] = 0
    policy[hot, int(np.argmin(p[hot_i]))] = 1.0
    z[hot] = -1
    return net, (own, enemy, policy, z), idx


def _row_maxima(net, data, idx):
    """Per trunk layer: max |d loss / d conv output| of every row of the batch, on the f64 graph."""
    import torch
    from reversi_alpha_zero_amd.agent.trainer import TorchTrainer
    tr = TorchTrainer(net, dtype=torch.float64, l2=tc.L2)
    ys = []
    hooks = [cb.conv.register_forward_hook(lambda m, i, o: ys.append(o)) for cb in tr.net.conv_bns()]
    total = tr._objective(*data, idx)[2]
    g = torch.autograd.grad(total, ys)
    for h in hooks:
        h.remove()
    return [x.abs().flatten(1).max(1).values for x in g[1:1 + 2 * net.res_layers]]


def skewed_gradients_meet_the_rule(make, monkeypatch):
    """The scale rule where it is strained: a split tensor's scale comes from its maximum, and here the maximum of every trunk layer's
    output gradient is one row's, at least 2^10 times the median row's - those rows keep 2^-10 of the f16 range and lose lo bits.
    The dominating row is the one of the batch's first eight with the largest such ratio on the f64 graph (chosen on the reference
    alone); the ratio is asserted, then tc.gradient_rule holds as everywhere."""
    best = None
    for hot_i in range(8):
        net, data, idx = _skewed(hot_i)
        r = min(float(m.max() / m.median()) for m in _row_maxima(net, data, idx))
        if best is None or r > best[0]:
            best = (r, net, data, idx)
    r, net, data, idx = best
    print(f"output gradients of the trunk layers: the largest row's maximum is at least {r:.0f} times the median row's")
    assert r >= 2.0 ** 10
    monkeypatch.setattr(tc, "data", lambda: data)
    monkeypatch.setattr(tc, "make_net", lambda F, R, V: net)
    monkeypatch.setattr(tc, "batch_rows", lambda B, salt=0: idx)
    B = len(idx)
    c = tc.case(make, 16, 1, 16, B, rows="one row dominates")   # (a tag of this test's own: computed under the patches above)
    tc.gradient_rule(make, c, (16, 1, 16, B, "one row dominates"))
