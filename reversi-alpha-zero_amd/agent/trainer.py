"""raznet-train-v1: the training step of the reference's `opt` worker (worker/optimize.py:73-86 over the
graph and losses of agent/model.py:28-72,104-110), twice:

  * DeviceTrainer - the HIP kernels of csrc/raz_train.hip behind include/raz.h's raz_trainer_* entries.  State, saved tensors and
    the data set live on the device; a step launches kernels only.
  * TorchTrainer  - the same step restated over ReversiNet in training mode and autograd, in fp32 or f64, on CPU or GPU: the
    yardstick of the tests, the backend of the CPU tests and the baseline of tools/bench_train.py.

Both take the PACKED data set (lib/data_helper.pack_game_data: own u64[N], enemy u64[N], policy f32[N,64], z i8[N]) and the row
indices of the batch:  step(own, enemy, policy, z, idx, lr) -> (policy_loss, value_loss).

The step: BatchNorm normalises with the batch mean and the biased batch variance and moves its statistics with momentum 0.99
(the moving variance takes the unbiased batch variance: torch.nn.BatchNorm2d(momentum=0.01)); the objective is
mean_b sum_a -pi log(p + 1e-7) + mean_b (v - z)^2 + l2 sum w^2 over the Conv2D / Dense KERNELS only (Keras kernel_regularizer:
gradient term 2 l2 w; biases and BatchNorm parameters are not regularised); the update is Keras SGD(momentum=0.9):
m <- 0.9 m - lr g, w <- w + m.
"""
import copy
import ctypes

import numpy as np
import torch

from .model import ReversiNet

MOMENTUM = 0.9
BN_MOMENTUM_TORCH = 0.01   # Keras momentum 0.99


def check_trainable(net):
    if net.filter_size != 3 or net.filters % 16 or net.filters < 16:
        raise ValueError(f"raznet-train-v1 takes cnn_filter_size 3 and cnn_filter_num % 16 == 0 (got size {net.filter_size}, "
                         f"{net.filters} filters)")


def _tensor(x, device, dtype=None):
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint64:
            x = x.view(np.int64)
        elif x.dtype == np.uint32:
            x = x.astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not torch.is_tensor(x):
        x = torch.as_tensor(x)
    x = x.to(device)
    return x if dtype is None or x.dtype == dtype else x.to(dtype)


def named_state(net, momentum):
    """{name: tensor} of a whole training state: parameters, moving statistics, momentum buffers ("momentum.<name>")."""
    out = {n: t.detach().cpu() for n, t in net.train_tensors() + net.stat_tensors()}
    out.update({"momentum." + n: m.detach().cpu() for (n, _), m in zip(net.train_tensors(), momentum)})
    return out


class TorchTrainer:
    """raznet-train-v1 over autograd.  `relu_masks` (a list of boolean tensors, one per ReLU in graph order: stem, the 2 R trunk
    layers, policy conv, value conv, dense_1) replaces every ReLU by a multiplication with the given mask - the f64 yardstick
    of an implementation whose own ReLUs passed exactly there."""

    def __init__(self, net, max_batch=None, device="cpu", dtype=torch.float32, l2=1e-4):
        check_trainable(net)
        self.device, self.dtype, self.l2, self.max_batch = torch.device(device), dtype, float(l2), max_batch
        self.relu_masks = None
        self.from_net(net)

    # -- state ---------------------------------------------------------------------------------------------------------------
    def from_net(self, net, momentum=None):
        self.net = copy.deepcopy(net).to(device=self.device, dtype=self.dtype)
        for m in self.net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = BN_MOMENTUM_TORCH
        self.net.train()
        self.params = [t for _, t in self.net.train_tensors()]
        self.kernels = [t for n, t in self.net.train_tensors() if n.endswith(".kernel")]
        self.momentum = [torch.zeros_like(p) for p in self.params] if momentum is None else \
            [m.to(device=self.device, dtype=self.dtype).clone() for m in momentum]
        self._grads = None
        return self

    def to_net(self):
        net = copy.deepcopy(self.net).to(device="cpu", dtype=torch.float32)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 0.1
        return net.eval()

    def state(self):
        return named_state(self.net, self.momentum)

    # -- the graph -----------------------------------------------------------------------------------------------------------
    def _relu(self, t):
        i = len(self.acts)
        out = torch.relu(t) if self.relu_masks is None else t * self.relu_masks[i].to(device=t.device, dtype=t.dtype)
        self.acts.append(out.detach())
        return out

    def _forward(self, planes):
        net, self.acts, self.batch_mean, self.batch_var, self._bn_outs = self.net, [], [], [], []

        def bn(cb, x):
            y = cb.conv(x)
            self.batch_mean.append(y.detach().mean((0, 2, 3)))
            self.batch_var.append(y.detach().var((0, 2, 3), unbiased=False))
            out = cb.bn(y)
            self._bn_outs.append(out)
            return out
        x = self._relu(bn(net.stem, planes))
        for c1, c2 in net.res:
            h = self._relu(bn(c1, x))
            x = self._relu(bn(c2, h) + x)
        p = self._relu(bn(net.policy_conv, x)).flatten(1)
        p = torch.softmax(net.policy_fc(p), dim=1)
        v = self._relu(bn(net.value_conv, x)).flatten(1)
        self._vpre = net.value_fc2(self._relu(net.value_fc1(v)))
        v = torch.tanh(self._vpre)
        self.policy, self.value = p.detach(), v.detach()[:, 0]
        return p, v

    def _regulariser(self):
        return self.l2 * sum((w * w).sum() for w in self.kernels)

    def _objective(self, own, enemy, policy, z, idx):
        dev = self.device
        idx = _tensor(idx, dev, torch.int64)
        o, e = _tensor(own, dev)[idx], _tensor(enemy, dev)[idx]
        sh = torch.arange(64, device=dev, dtype=torch.int64)
        planes = torch.stack([(o[:, None] >> sh) & 1, (e[:, None] >> sh) & 1], dim=1).to(self.dtype).view(-1, 2, 8, 8)
        pi = _tensor(policy, dev)[idx].to(self.dtype)
        zz = _tensor(z, dev)[idx].to(self.dtype)
        p, v = self._forward(planes)
        pl = (-(pi * torch.log(p + 1e-7)).sum(1)).mean()
        vl = ((v[:, 0] - zz) ** 2).mean()
        return pl, vl, pl + vl + self._regulariser()

    def backward(self, own, enemy, policy, z, idx):
        """Gradients of the full objective without any update (moving statistics included): see gradients()."""
        saved = [t.detach().clone() for _, t in self.net.stat_tensors()]
        counts = [(m, m.num_batches_tracked.clone()) for m in self.net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        pl, vl, total = self._objective(own, enemy, policy, z, idx)
        grads = torch.autograd.grad(total, self.params + self._bn_outs + [self._vpre])
        self._grads = grads[:len(self.params)]
        # sum |term| of the gradients that are plain sums over the batch: BatchNorm's beta (terms g) and gamma (terms g xhat) per
        # channel, value_out's bias (terms d loss / d pre-tanh) - what a float32 sum's rounding is proportional to (tests)
        self.abs_sums = {}
        with torch.no_grad():
            for i, (cb, out, g) in enumerate(zip(self.net.conv_bns(), self._bn_outs, grads[len(self.params):-1])):
                xhat = (out - cb.bn.bias.view(1, -1, 1, 1)) / cb.bn.weight.view(1, -1, 1, 1)
                self.abs_sums[f"bn{i}.beta"] = g.abs().sum((0, 2, 3)).double().cpu()
                self.abs_sums[f"bn{i}.gamma"] = (g * xhat).abs().sum((0, 2, 3)).double().cpu()
            self.abs_sums["value_out.bias"] = grads[-1].abs().sum(0).double().cpu()
        with torch.no_grad():
            for (_, t), s in zip(self.net.stat_tensors(), saved):
                t.copy_(s)
            for m, c in counts:
                m.num_batches_tracked.copy_(c)
        return float(pl.detach()), float(vl.detach())

    def step(self, own, enemy, policy, z, idx, lr, sync=True):
        """sync=False returns the two losses as tensors on the trainer's device instead of waiting for them."""
        pl, vl, total = self._objective(own, enemy, policy, z, idx)
        self._grads = torch.autograd.grad(total, self.params)
        with torch.no_grad():
            for w, m, g in zip(self.params, self.momentum, self._grads):
                m.mul_(MOMENTUM).sub_(g, alpha=lr)
                w.add_(m)
        return (float(pl.detach()), float(vl.detach())) if sync else (pl.detach(), vl.detach())

    def gradients(self):
        return {n: g.detach().cpu() for (n, _), g in zip(self.net.train_tensors(), self._grads)}

    def activations(self):
        """Post-ReLU outputs of the last forward, graph order (the last one is dense_1's)."""
        return [a.cpu() for a in self.acts]


PRECISIONS = {"f32": 0, "f16x3": 1}   # include/raz.h RAZ_TRAIN_F32 (raznet-train-v1), RAZ_TRAIN_F16X3 (raznet-train-v2)


def precision_code(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision={precision!r}: 'f32' (raznet-train-v1) or 'f16x3' (raznet-train-v2)")
    return PRECISIONS[precision]


class DeviceTrainer:
    """The HIP trainer.  All arrays given to step / backward are moved to the trainer's device if they are not there already;
    keep the data set resident (torch tensors on the device) to launch kernels only.  precision="f32" is raznet-train-v1;
    "f16x3" is raznet-train-v2: the trunk's 3x3 products on the f16 matrix cores over split operands -
    as reproducible as v1, not v1's bytes."""

    READ_GRADS, READ_ACT, READ_MEAN, READ_VAR, READ_HIDDEN, READ_POLICY, READ_VALUE = range(7)

    def __init__(self, net, max_batch, device="cuda:0", l2=1e-4, precision="f32", *, backend=None):
        """backend: the build of the C ABI to run on (None: _native.HIP, the only one the product makes)."""
        code = precision_code(precision)
        if backend is None:
            from .. import _native as N   # (here, not at the top: TorchTrainer needs no library)
            backend = N.HIP
        check_trainable(net)
        self.precision = precision
        self.backend, self.lib, self.device, self.l2, self.max_batch = backend, backend.lib, torch.device(device), float(l2), int(max_batch)
        self.F, self.R, self.V = net.filters, net.res_layers, net.value_fc
        self.handle = ctypes.c_void_p()
        nbytes = self.lib.raz_trainer_bytes2(self.F, self.R, self.V, self.max_batch, code)   # (precision 0: raz_trainer_bytes / _create to the byte)
        if not nbytes:
            raise ValueError(f"raz_trainer_bytes2 refuses {self.F}x{self.R}x{self.V}, max_batch {self.max_batch}, precision {precision!r}")
        self.state_floats = self.lib.raz_trainer_state_bytes(self.F, self.R, self.V) // 4
        self.workspace = self.backend.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._launch("raz_trainer_create2", self.F, self.R, self.V, self.max_batch, code, self.workspace.data_ptr(), nbytes, ctypes.byref(self.handle))
        self.losses = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._shape_net = ReversiNet(self.F, self.R, self.V)
        self.last_batch = 0
        self.from_net(net)

    def _launch(self, name, *args):
        """lib.<name>(*args, stream) with the trainer's device current (_native.Wrapper's helper; see the import above)."""
        b = self.backend
        with b.on(self.device):
            b.call(name, *args, b.stream(self.device))

    def close(self):
        if getattr(self, "handle", None):
            self.backend.synchronize(self.device)
            self.lib.raz_trainer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ---------------------------------------------------------------------------------------------------------------
    def set_blob(self, blob):
        t = _tensor(np.ascontiguousarray(blob, dtype=np.float32), self.device)
        self._launch("raz_trainer_set_state", self.handle, t.data_ptr(), t.numel() * 4)
        self.backend.synchronize(self.device)

    def get_blob(self):
        t = torch.empty(self.state_floats, dtype=torch.float32, device=self.device)
        self._launch("raz_trainer_get_state", self.handle, t.data_ptr(), t.numel() * 4)
        return t.cpu().numpy()

    def from_net(self, net, momentum=None):
        if (net.filters, net.res_layers, net.value_fc) != (self.F, self.R, self.V):
            raise ValueError("the net's shape differs from the trainer's")
        self.set_blob(net.to_train_blob(momentum))
        return self

    def to_net(self):
        net = ReversiNet(self.F, self.R, self.V)
        self._momentum = net.load_train_blob(self.get_blob())
        return net.eval()

    def state(self):
        net = self.to_net()
        return named_state(net, self._momentum)

    # -- the step ------------------------------------------------------------------------------------------------------------
    def _args(self, own, enemy, policy, z, idx):
        d = self.device
        own, enemy = _tensor(own, d, torch.int64).contiguous(), _tensor(enemy, d, torch.int64).contiguous()
        policy, z = _tensor(policy, d, torch.float32).contiguous(), _tensor(z, d, torch.int8).contiguous()
        idx = _tensor(idx, d, torch.int32).contiguous()   # (row numbers below 2^31: the bits of the u32 the entry reads)
        if not (own.numel() == enemy.numel() == z.numel() and policy.numel() == 64 * own.numel()):
            raise ValueError("own, enemy, policy [N,64] and z must describe the same N rows")
        return own, enemy, policy, z, idx

    def backward(self, own, enemy, policy, z, idx):
        own, enemy, policy, z, idx = self._args(own, enemy, policy, z, idx)
        self._launch("raz_trainer_backward", self.handle, own.data_ptr(), enemy.data_ptr(), policy.data_ptr(), z.data_ptr(),
                     idx.data_ptr(), idx.numel(), self.l2, self.losses.data_ptr())
        self.last_batch = idx.numel()
        return tuple(self.losses.tolist())

    def step(self, own, enemy, policy, z, idx, lr, sync=True):
        """sync=False returns the device tensor of the two losses instead of waiting for them."""
        own, enemy, policy, z, idx = self._args(own, enemy, policy, z, idx)
        self._launch("raz_trainer_step", self.handle, own.data_ptr(), enemy.data_ptr(), policy.data_ptr(), z.data_ptr(),
                     idx.data_ptr(), idx.numel(), float(lr), self.l2, self.losses.data_ptr())
        self.last_batch = idx.numel()
        return tuple(self.losses.tolist()) if sync else self.losses

    # -- what the last step left ---------------------------------------------------------------------------------------------
    def read(self, which, layer, shape):
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._launch("raz_trainer_read", self.handle, which, layer, out.data_ptr(), out.numel() * 4)
        return out.cpu()

    def _channels(self, layer):
        return self.F if layer <= 2 * self.R else 2 if layer == 2 * self.R + 1 else 1

    def activations(self):
        """Post-ReLU outputs of the last step, graph order: the 2 R + 3 conv layers, then dense_1's."""
        B = self.last_batch
        acts = [self.read(self.READ_ACT, i, (B, self._channels(i), 8, 8)) for i in range(2 * self.R + 3)]
        return acts + [self.read(self.READ_HIDDEN, 0, (B, self.V))]

    def batch_stats(self):
        n = 2 * self.R + 3
        return ([self.read(self.READ_MEAN, i, (self._channels(i),)) for i in range(n)],
                [self.read(self.READ_VAR, i, (self._channels(i),)) for i in range(n)])

    def outputs(self):
        return self.read(self.READ_POLICY, 0, (self.last_batch, 64)), self.read(self.READ_VALUE, 0, (self.last_batch,))

    def gradients(self):
        flat = self.read(self.READ_GRADS, 0, ((self.state_floats - self._n_stats()) // 2,))
        out, o = {}, 0
        for name, t in self._shape_net.train_tensors():
            v = flat[o:o + t.numel()]
            o += t.numel()
            out[name] = (v.view(t.shape[1], t.shape[0]).t() if name.endswith(".kernel") and t.dim() == 2 else v.view(t.shape)).clone()
        return out

    def _n_stats(self):
        return sum(t.numel() for _, t in self._shape_net.stat_tensors())
