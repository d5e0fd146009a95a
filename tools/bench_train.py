"""Time one raznet-train-v1 step on the HIP kernels and on fp32 torch, alternating in one process.

  python tools/bench_train.py [--shape 256,10,256 --shape 16,1,16] [--batch 256] [--steps 50] [--warmup 5] [--precision f16x3] [--out file.json]

The data set (random positions, sparse policies) is resident on the device; every timed step is bracketed by device events on
the synchronised stream; the backends take turns step by step so that clocks and neighbours affect both alike.  Reported per
backend: ms per step (median and mean), the algorithmic FLOP of the three 3x3 products (3 x macs_per_position x 2 x batch; the
heads' and the element-wise terms are listed separately and not counted) and the share of the 157.3 TF/s f32 matrix peak.
--precision f16x3 adds raznet-train-v2 ("hip-f16x3": the trunk products on the f16 matrix cores over split operands) as a third
contestant in the same alternating loop - with --backend hip it runs alone - and reports the share of the 2.5 PF/s f16 matrix peak
its trunk products EXECUTE: three matrix instructions per algorithmic product."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MATRIX_PEAK = 157.3e12
F16_MATRIX_PEAK = 2.5e15


def dataset(n, seed=0):
    rng = np.random.default_rng(seed)
    fill = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    own = fill & rng.integers(0, 2**64, size=n, dtype=np.uint64)
    policy = np.zeros((n, 64), np.float32)
    for i in range(n):
        sq = rng.choice(64, size=4, replace=False)
        w = rng.random(4) + 0.1
        policy[i, sq] = w / w.sum()
    return own, fill & ~own, policy, rng.integers(-1, 2, size=n).astype(np.int8)


def bench(F, R, V, B, steps, warmup, dev, backends=("hip", "torch")):
    from reversi_alpha_zero_amd.agent.model import ReversiNet, macs_per_position
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer, TorchTrainer, _tensor
    net = ReversiNet(F, R, V).keras_init_(0)
    n = 16 * B
    data = tuple(_tensor(a, torch.device(dev)) for a in dataset(n))
    make = {"hip": lambda: DeviceTrainer(net, max_batch=B, device=dev), "torch": lambda: TorchTrainer(net, max_batch=B, device=dev),
            "hip-f16x3": lambda: DeviceTrainer(net, max_batch=B, device=dev, precision="f16x3")}
    trainers = {k: make[k]() for k in backends}
    times = {k: [] for k in trainers}
    rng = np.random.default_rng(1)
    for it in range(warmup + steps):
        idx = torch.from_numpy(rng.permutation(n)[:B]).to(dev)
        for name, t in trainers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t.step(*data, idx, 1e-2)
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    for name in ("hip", "hip-f16x3"):
        if name in trainers:
            trainers[name].close()
    macs = macs_per_position(F, R, V)
    trunk = 64 * R * 2 * F * F * 9
    flop = 3 * macs * 2 * B
    out = {"shape": [F, R, V], "batch": B, "steps": steps, "warmup": warmup,
           "flop_per_step_products": flop, "flop_per_step_3x3_trunk_only": 3 * trunk * 2 * B,
           "not_counted": "BatchNorm, ReLU, losses, L2 and the update: O(batch x F x 64) element-wise terms per layer",
           "floor_ms_at_f32_matrix_peak": flop / F32_MATRIX_PEAK * 1e3}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"ms_per_step_median": med, "ms_per_step_mean": statistics.fmean(ts), "ms_min": min(ts), "ms_max": max(ts),
                     "tflops": flop / med / 1e9, "share_of_f32_matrix_peak": flop / (med * 1e-3) / F32_MATRIX_PEAK}
    if "hip" in times and "torch" in times:
        out["hip_over_torch"] = out["hip"]["ms_per_step_median"] / out["torch"]["ms_per_step_median"]
    if "hip-f16x3" in times:
        v2 = out["hip-f16x3"]
        v2["share_of_f16_matrix_peak_executed_trunk_only"] = 3 * out["flop_per_step_3x3_trunk_only"] / (v2["ms_per_step_median"] * 1e-3) / F16_MATRIX_PEAK
        for other in ("hip", "torch"):
            if other in times:
                out[f"hip-f16x3_over_{other}"] = v2["ms_per_step_median"] / out[other]["ms_per_step_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="F,R,V (default: 256,10,256 and 16,1,16)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--backend", default="both", choices=("both", "hip", "torch"),
                    help="one backend alone: the run to put under `rocprofv3 --kernel-trace --stats -- python tools/bench_train.py ...`")
    ap.add_argument("--precision", default="f32", choices=("f32", "f16x3"),
                    help="f16x3: raznet-train-v2 as well (with --backend hip: instead of v1)")
    ap.add_argument("--out")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in (a.shape or ["256,10,256", "16,1,16"])]
    if a.precision == "f16x3":
        backends = {"both": ("hip", "hip-f16x3", "torch"), "hip": ("hip-f16x3",), "torch": ("torch",)}[a.backend]
    else:
        backends = ("hip", "torch") if a.backend == "both" else (a.backend,)
    results = [bench(F, R, V, a.batch, a.steps, a.warmup, a.device, backends) for F, R, V in shapes]
    doc = {"device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
