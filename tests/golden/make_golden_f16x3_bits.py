#!/usr/bin/env python
"""Record tests/golden/f16x3_bits.npz: policy and value of raznet-forward-v2 and v3 as THIS checkout computes them on an MI355X, for
the cases of tests/net_f16x3_bits_cases.py:
    python tests/golden/make_golden_f16x3_bits.py
Run once, at the commit whose bits are to be kept, before a change to the trunk's epilogue, the first-layer kernel or the compacted
forward that must not move a bit; tests/test_net_f16x3_bits_gpu.py then holds every later build to the recording.

Contents: "pv_<F>x<R>x<V>_<version>" uint32 [65, 65] - per position of the pool 64 policy words and the value word (the plain and the
masked cases of every row count are checked against it here: a row's answer does not depend on the batch around it);
"compact_<F>x<R>x<V>_<n>" uint64 [steps, n, 4] - the compacted form, see net_f16x3_bits_cases.compacted."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import __graft_entry__ as g  # noqa: E402
import net_f16x3_bits_cases as C  # noqa: E402


def main():
    g.build()
    from reversi_alpha_zero_amd.engine import DeviceNet
    own, enemy = C.positions()
    out = {}
    for shape in C.NETS:
        blob = C.blob(shape)
        for ver, kernel in C.VERSIONS.items():
            dn = DeviceNet(blob, C.DEV, kernel=kernel)
            p, v = C.forward(dn, own, enemy)
            table = np.concatenate([p, v[:, None]], axis=1)
            for n in C.COUNTS:   # batch invariance, as the fixture relies on it
                pn, vn = C.forward(dn, own[:n], enemy[:n])
                assert np.array_equal(pn, p[:n]) and np.array_equal(vn, v[:n]), (shape, ver, n)
                a = C.mask(n)
                pm, vm = C.forward(dn, own[:n], enemy[:n], a)
                on = a != 0
                assert np.array_equal(pm[on], p[:n][on]) and np.array_equal(vm[on], v[:n][on]), (shape, ver, n, "masked")
                assert not pm[~on].any() and not vm[~on].any()
            assert dn.range_ok()
            out[f"pv_{C.key(shape)}_{ver}"] = table
            print(shape, ver, "distinct value words:", len(np.unique(v)))
        dn = DeviceNet(blob, C.DEV, kernel="f16x3")
        for n in C.COUNTS:
            rows, st = C.compacted(dn, n)
            total = st["hits"] + st["in_batch_duplicates"] + st["evaluated"]
            print(shape, "compacted", n, st)
            assert n == 1 or st["evaluated"] < total, "the compacted case never had fewer rows than games"
            out[f"compact_{C.key(shape)}_{n}"] = rows
        assert dn.range_ok()
    path = os.path.join(HERE, "f16x3_bits.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
