"""raznet-train-v1 on the device (csrc/raz_train.hip through agent/trainer.py's DeviceTrainer) against the f64 restatement, tensor by
tensor - the rules are in tests/train_cases.py.  RAZ_TRAIN_ACCURACY_JSON=<path> appends the measured ratios of every case."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import train_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(F, R, V, B) for (F, R, V) in tc.SHAPES for B in tc.BATCHES]


def _record(kind, case, worst, unfloored):
    path = os.environ.get("RAZ_TRAIN_ACCURACY_JSON")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": list(case), "worst_ratio": worst[0], "tensor": worst[1],
                                "scalars_unfloored": unfloored}) + "\n")


@functools.lru_cache(maxsize=None)
def _case(F, R, V, B):
    """One backward of the device, of fp32 torch and of the three f64 graphs (plain, masked as the device, masked as fp32 torch)."""
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
    net = tc.make_net(F, R, V)
    idx, f64 = tc.sharp_batch(net, B)
    dev = DeviceTrainer(net, max_batch=B, device=DEV, l2=tc.L2)
    before = dev.get_blob()
    losses = dev.backward(*tc.data(), idx)
    mean, var = dev.batch_stats()
    d = {"acts": dev.activations(), "mean": mean, "var": var, "losses": losses, "grads": dev.gradients(),
         "untouched": bool(np.array_equal(before.view(np.uint32), dev.get_blob().view(np.uint32)))}
    dev.close()
    t32 = tc.torch_backward(net, idx, torch.float32)
    return {"dev": d, "t32": t32, "f64": f64,
            "f64_as_dev": tc.torch_backward(net, idx, torch.float64, tc.masks_of(d["acts"])),
            "f64_as_t32": tc.torch_backward(net, idx, torch.float64, tc.masks_of(t32["acts"]))}


@pytest.mark.parametrize("F,R,V,B", CASES)
def test_forward_in_training_mode(F, R, V, B):
    c = _case(F, R, V, B)
    dev, t32, ref = c["dev"], c["t32"], c["f64"]
    assert dev["untouched"], "raz_trainer_backward changed the state"
    names = tc.layer_names(R)
    for name, a in zip(names, ref["acts"]):   # the guards: a comparison of dead or saturated layers shows nothing
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
        e, raw = tc.err(x, r), tc.err(y, r)
        floor = tc.forward_floor(kind, r, m, v)   # 0 unless the tensor is ONE number (tests/train_cases.py, SCALARS)
        e32 = tc.floored(raw, floor)
        k = tc.ratio(e, e32)
        note = ""
        if tc.is_scalar(r):
            unfloored[name] = tc.ratio(e, raw)
            note = f"   (scalar: fp32 torch's own {raw[0]:.3g}, un-floored ratio {unfloored[name]:.2f})"
        print(f"{name:28s} device max {e[0]:.3g} mean {e[1]:.3g}   fp32 torch max {e32[0]:.3g} mean {e32[1]:.3g}   ratio {k:.2f}{note}")
        worst = max(worst, (k, name))
        if not tc.forward_ok(e, e32, tc.K_FORWARD):
            bad.append((name, e, e32))
    _record("forward", (F, R, V, B), worst, unfloored)
    assert not bad, bad


@pytest.mark.parametrize("F,R,V,B", CASES)
def test_gradients_tensor_by_tensor(F, R, V, B):
    c = _case(F, R, V, B)
    bad, worst = [], (0.0, "")
    unfloored = {}
    for name, ref in c["f64_as_dev"]["grads"].items():
        g, g32, ref32 = c["dev"]["grads"][name], c["t32"]["grads"][name], c["f64_as_t32"]["grads"][name]
        assert tuple(g.shape) == tuple(ref.shape), name
        if tc.is_conv_bias(name):   # true gradient 0: absolute, against fp32 torch's residue
            n, n32 = float(g.double().norm()), float(g32.norm())
            print(f"{name:28s} |g| device {n:.3g}   fp32 torch {n32:.3g}")
            if not n <= 10 * n32:
                bad.append((name, n, n32))
            continue
        assert float(ref.norm()) > 1e-6, f"{name}: the f64 gradient is (nearly) zero, the case shows nothing"
        r, r32 = tc.rel_l2(g, ref), tc.rel_l2(g32, ref32)
        ratio = lambda own: max(0.0, (r - 1e-7) / own) if own > 0 else (0.0 if r <= 1e-7 else float("inf"))
        note = ""
        if tc.is_scalar(ref):   # ONE number: fp32 torch's error floored at one ulp of what the sum adds up (tests/train_cases.py, SCALARS)
            unfloored[name] = ratio(r32)
            note = f"   (scalar: fp32 torch's own {r32:.3g}, un-floored ratio {unfloored[name]:.2f})"
            r32 = max(r32, tc.grad_floor(name, ref, c["f64_as_dev"]["abs_sums"]))
        k = ratio(r32)
        print(f"{name:28s} relative L2 device {r:.3g}   fp32 torch {r32:.3g}   ratio {k:.2f}{note}")
        worst = max(worst, (k, name))
        if not r <= tc.K_GRAD * r32 + 1e-7:
            bad.append((name, r, r32))
    _record("gradients", (F, R, V, B), worst, unfloored)
    assert not bad, bad


def _updates(state, ref, init):
    """{tensor: ||w - w_64|| / ||w_64 - w_init||}, conv biases ahead of BatchNorm as max |w - w_64| under 'abs'."""
    rel, absd = {}, {}
    for name, w64 in ref.items():
        base = name[len("momentum."):] if name.startswith("momentum.") else name
        d = (state[name].double() - w64.double())
        if tc.is_conv_bias(base):
            absd[name] = float(d.abs().max())
        else:
            moved = float((w64.double() - init[name].double()).norm())
            assert moved > 0, f"{name} did not move in f64: the case shows nothing"
            rel[name] = float(d.norm()) / moved
    return rel, absd


@pytest.mark.parametrize("F,R,V,B", [(16, 1, 16, 5), (16, 1, 16, 67), (128, 1, 64, 5), (128, 1, 64, 67)])
def test_eight_steps_track_the_f64_trainer(F, R, V, B):
    """Eight steps at lr 1e-2 with momentum, the same batches as an f64 TorchTrainer: every tensor of the state (moving statistics
    and momentum buffers included) stays within 1e-2 of ITS OWN UPDATE of the f64 trainer's, conv biases ahead of BatchNorm within
    1e-5 absolutely.  fp32 torch on the CPU stays within 3e-4 and 5e-7; a wrong momentum, update order or BatchNorm momentum moves
    a tensor by tens of percent of its update."""
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer, TorchTrainer
    net = tc.make_net(F, R, V)
    trainers = {"f64": TorchTrainer(net, dtype=torch.float64, l2=tc.L2), "fp32 torch": TorchTrainer(net, dtype=torch.float32, l2=tc.L2),
                "device": DeviceTrainer(net, max_batch=B, device=DEV, l2=tc.L2)}
    init = {k: v.clone() for k, v in trainers["f64"].state().items()}
    for step in range(8):
        idx = tc.batch_rows(B, salt=step)
        for t in trainers.values():
            t.step(*tc.data(), idx, 1e-2)
    ref = trainers["f64"].state()
    for who in ("fp32 torch", "device"):
        rel, absd = _updates(trainers[who].state(), ref, init)
        w, a = max(rel, key=rel.get), max(absd, key=absd.get)
        print(f"{who:10s} worst relative {rel[w]:.3g} ({w})   worst conv-bias |difference| {absd[a]:.3g} ({a})")
        if who == "device":
            assert not {k: v for k, v in rel.items() if not v <= 1e-2}
            assert not {k: v for k, v in absd.items() if not v <= 1e-5}
    trainers["device"].close()


def test_two_trainers_hold_the_same_bytes():
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
    net = tc.make_net(128, 1, 64)
    blobs = []
    for _ in range(2):
        t = DeviceTrainer(net, max_batch=67, device=DEV, l2=tc.L2)
        for step in range(3):
            t.step(*tc.data(), tc.batch_rows(67, salt=step), 1e-2)
        blobs.append(t.get_blob())
        t.close()
    assert not np.array_equal(blobs[0], net.to_train_blob()), "three steps changed nothing"
    assert np.array_equal(blobs[0].view(np.uint32), blobs[1].view(np.uint32))


def test_abi_guards_refuse_and_leave_the_state_untouched():
    from reversi_alpha_zero_amd import _native as N
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer, _tensor
    lib, s = N.lib, N.current_stream_ptr()
    assert lib.raz_trainer_bytes(24, 1, 16, 8) == 0 and lib.raz_trainer_state_bytes(24, 1, 16) == 0
    need = lib.raz_trainer_bytes(16, 1, 16, 8)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    h = ctypes.c_void_p()
    assert lib.raz_trainer_create(24, 1, 16, 8, ws.data_ptr(), need, ctypes.byref(h), s) == -1 and not h.value      # F % 16 != 0
    assert lib.raz_trainer_create(16, 1, 16, 8, ws.data_ptr(), need - 1, ctypes.byref(h), s) == -1 and not h.value  # one byte short
    assert lib.raz_trainer_create(16, 1, 16, 8, ws.data_ptr() + 4, need, ctypes.byref(h), s) == -1 and not h.value  # misaligned
    assert lib.raz_trainer_create(16, 1, 16, 8, None, need, ctypes.byref(h), s) == -1 and not h.value
    assert "raz_trainer_create" in N.last_error()
    t = DeviceTrainer(tc.make_net(16, 1, 16), max_batch=8, device=DEV, l2=tc.L2)
    own, enemy, policy, z = (_tensor(a, torch.device(DEV)) for a in tc.data())
    idx = torch.arange(9, dtype=torch.int32, device=DEV)
    losses, before = torch.zeros(2, device=DEV), t.get_blob()
    a = [own.data_ptr(), enemy.data_ptr(), policy.data_ptr(), z.data_ptr(), idx.data_ptr()]

    def step(args, B, out=losses.data_ptr()):
        return lib.raz_trainer_step(t.handle, *args, B, 1e-2, tc.L2, out, s)
    assert step(a, 0) == -1 and step(a, 9) == -1                       # B = 0, B > max_batch
    for i in range(5):                                                 # a NULL array
        assert step(a[:i] + [None] + a[i + 1:], 4) == -1
    assert step(a, 4, None) == -1
    assert step([a[0] + 4] + a[1:], 4) == -1 and step([a[0], a[1] + 4] + a[2:], 4) == -1   # misaligned bitboards
    assert step(a[:2] + [a[2] + 2] + a[3:], 4) == -1 and step(a[:4] + [a[4] + 2], 4) == -1  # misaligned policy / idx
    assert lib.raz_trainer_backward(t.handle, *a, 9, tc.L2, losses.data_ptr(), s) == -1
    assert lib.raz_trainer_set_state(t.handle, ws.data_ptr(), before.nbytes - 4, s) == -1
    assert lib.raz_trainer_read(t.handle, 99, 0, ws.data_ptr(), 4, s) == -1
    torch.cuda.synchronize()
    assert np.array_equal(before.view(np.uint32), t.get_blob().view(np.uint32)), "a refused call changed the state"
    assert step(a, 4) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(before.view(np.uint32), t.get_blob().view(np.uint32))
    t.close()
    with pytest.raises(ValueError):
        DeviceTrainer(tc.make_net(24, 1, 16), max_batch=8, device=DEV)
