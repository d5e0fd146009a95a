"""GPU: every kernel form of the policy/value net (include/raz.h raz_net_form) against the f64 evaluation of the same graph, at the
shapes and batch sizes where the forms' indexing and dispatch have edges (tests/net_cases.py).

  - exact-f32 forms (raz_net.reserved 0 / 1 / 2): equal to each other bit for bit on every row, equal to the C oracle bit for bit
    on three rows per shape, and - per case, over all rows - max and mean |error| against f64 within a multiple of fp32 torch's
    own (+1e-7 / +2e-8; net_cases.EXACT_FACTOR: the contract's sequential chains);
  - the split-f16 trunk (reserved 4): the same rule (net_cases.F16X3_FACTOR), a row alone == the row in the batch;
  - batch edges of every form: rows past n and inactive rows come back bit-unchanged;
  - the f16x3 weight image at the edges of its per-layer scale, the shapes without in-forward repair, the widest value head."""
import ctypes

import numpy as np
import pytest
import torch

import net_cases as C
import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = {0: "f32", 1: "valu", 2: "mfma_wave", 4: "f16x3"}
NAN = 0x7FC0DEAD   # the guard rows' bit pattern (a quiet NaN no kernel writes)


def expected_form(F, V, reserved):
    """The table of include/raz.h raz_net_form, restated: what each case means to exercise."""
    if F in (16, 32, 64) and V <= 1024 and reserved != 1:
        return "mfma_wave" if reserved == 2 else "mfma"
    if reserved == 4:
        return "f16x3_repair" if (2 * 64 * F + 192 + V) * 4 <= 160 * 1024 else "f16x3_no_repair"
    if F >= 128 and F % 64 == 0 and reserved != 1:
        return "wide"
    return "wave_lds" if (3 * 64 * F + 192 + V) * 4 <= 64 * 1024 else "wave_scratch"


_INPUTS = {}


def _inputs():
    if not _INPUTS:
        own, enemy, names = C.inputs()
        _INPUTS.update(own=own, enemy=enemy, names=names, own_t=torch.from_numpy(own.view(np.int64)).to(DEV),
                       enemy_t=torch.from_numpy(enemy.view(np.int64)).to(DEV))
    return _INPUTS


def _net(shape, seed, edit=None):
    """(blob, f64 reference, fp32 torch's error against it) of a sharp net on the shared inputs; the guard runs first."""
    F, R, V = shape
    x = _inputs()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = C.sharp_net(F, R, V, seed, x["own"], x["enemy"], device=DEV, edit=edit)
    rp, rv = C.reference(net, x["own"], x["enemy"], device=DEV)
    C.assert_sharp(rp, rv, str(shape))
    tp, tv = C.reference(net, x["own"], x["enemy"], device=DEV, dtype=torch.float32)
    return net.to_blob(), (rp, rv), C.errors(tp, tv, rp, rv)


def _forward(blob, reserved, own_t, enemy_t):
    dn = DeviceNet_(blob, reserved)
    p, v = dn.predict_bitboards(own_t, enemy_t)
    torch.cuda.synchronize()
    return dn, p.cpu().numpy(), v.cpu().numpy()


def DeviceNet_(blob, reserved):
    from reversi_alpha_zero_amd.engine import DeviceNet
    return DeviceNet(blob, DEV, kernel=KERNEL[reserved])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_form_of_a_shape_against_f64(shape):
    F, R, V = shape
    x = _inputs()
    n = len(x["names"])
    blob, (rp, rv), e32 = _net(shape, seed=F + R)
    exact = {}
    for r in C.reserved_for(F):
        dn, p, v = _forward(blob, r, x["own_t"], x["enemy_t"])
        form = dn.form(n)
        assert form == expected_form(F, V, r), (shape, r, form)
        e = C.errors(p, v, rp, rv)
        print(f"{shape} reserved {r} {form}: max {e[0]:.3g} mean {e[1]:.3g} vs f64; fp32 torch max {e32[0]:.3g} mean {e32[1]:.3g}")
        assert np.isfinite(p).all() and np.isfinite(v).all()
        assert C.within_fp32_rule(e, e32, C.F16X3_FACTOR if r == 4 else C.EXACT_FACTOR), (shape, form, e, e32)
        if r == 4:
            for i in C.oracle_rows(x["names"]):   # a row alone == the same row inside the batch
                pa, va = dn.predict_bitboards(x["own_t"][i:i + 1], x["enemy_t"][i:i + 1])
                assert np.array_equal(_bits(pa.cpu().numpy()[0]), _bits(p[i])) and _bits(va.cpu().numpy())[0] == _bits(v)[i], (shape, i)
            assert dn.range_stats() == (True, 0)
        else:
            exact[r] = (p, v)
        del dn
    first = exact[0]
    for r, (p, v) in exact.items():   # raznet-forward-v1: every exact-f32 form computes the same chains
        assert np.array_equal(_bits(p), _bits(first[0])) and np.array_equal(_bits(v), _bits(first[1])), (shape, r)
    o = O.load_ext()
    for i in C.oracle_rows(x["names"]):
        op, ov = np.zeros(64, np.float32), np.zeros(1, np.float32)
        assert o.orc_net_forward(blob, len(blob), int(x["own"][i]), int(x["enemy"][i]), op.ctypes.data, ov.ctypes.data) == 0
        assert np.array_equal(_bits(first[0][i]), _bits(op)) and _bits(first[1])[i] == _bits(ov)[0], (shape, x["names"][i])


# One net per form, small enough that only the batch shapes matter
EDGE_FORMS = [("mfma", (16, 1, 16), 0), ("mfma_wave", (16, 1, 16), 2), ("wave_lds", (48, 1, 16), 0), ("wave_scratch", (96, 1, 16), 0),
              ("wide", (128, 1, 16), 0), ("f16x3_repair", (128, 1, 16), 4), ("f16x3_no_repair", (384, 1, 16), 4)]
EDGE_N = [1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513]
GUARD = 9


def _raw_forward(dn, own_t, enemy_t, n, active=None):
    """raz_net_forward through ctypes into output buffers of n + GUARD rows, all of them filled with NAN first."""
    from reversi_alpha_zero_amd._native import lib, check
    pol = torch.full(((n + GUARD) * 64,), NAN, dtype=torch.int32, device=DEV)
    val = torch.full((n + GUARD,), NAN, dtype=torch.int32, device=DEV)
    sp, sb = dn.scratch(n)
    check(lib.raz_net_forward(ctypes.byref(dn.c), own_t.data_ptr(), enemy_t.data_ptr(), active.data_ptr() if active is not None else None,
                              pol.data_ptr(), val.data_ptr(), n, sp, sb, torch.cuda.current_stream().cuda_stream), "raz_net_forward")
    torch.cuda.synchronize()
    return pol.cpu().numpy().view(np.uint32).reshape(n + GUARD, 64), val.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("form,shape,reserved", EDGE_FORMS, ids=[f[0] for f in EDGE_FORMS])
def test_batch_edges_leave_guard_and_inactive_rows_untouched(form, shape, reserved):
    """Batches of n in EDGE_N (the position groups: 4 per workgroup wide, 8 per workgroup and 8 workgroups per run f16x3, min(n, 256)
    repair blocks) with and without an active mask, an all-inactive mask, only the last row active: every row < n that is active
    equals the same row of a 513-row forward bit for bit, every other row of the buffer (inactive, or past n) keeps its NaN."""
    F, R, V = shape
    rng = np.random.default_rng(F + reserved)
    N = max(EDGE_N)
    own = rng.integers(0, 2**64, size=N, dtype=np.uint64)
    enemy = rng.integers(0, 2**64, size=N, dtype=np.uint64) & ~own
    own_t, enemy_t = torch.from_numpy(own.view(np.int64)).to(DEV), torch.from_numpy(enemy.view(np.int64)).to(DEV)
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    dn = DeviceNet_(ReversiNet(F, R, V).keras_init_(F).randomize_bn_(R).to_blob(), reserved)
    assert dn.form(N) == form == expected_form(F, V, reserved)
    ref_p, ref_v = _raw_forward(dn, own_t, enemy_t, N)
    assert not (ref_p[:N] == NAN).any() and not (ref_v[:N] == NAN).any()
    masks = {n: torch.from_numpy((np.arange(n) % 3 != 1).astype(np.uint8)).to(DEV) for n in EDGE_N}
    cases = [(n, None) for n in EDGE_N] + [(n, masks[n]) for n in EDGE_N]
    cases += [(65, torch.zeros(65, dtype=torch.uint8, device=DEV)), (257, torch.zeros(257, dtype=torch.uint8, device=DEV))]
    cases += [(n, torch.from_numpy((np.arange(n) == n - 1).astype(np.uint8)).to(DEV)) for n in (9, 65, 513)]
    for n, active in cases:
        p, v = _raw_forward(dn, own_t, enemy_t, n, active)
        on = np.zeros(n + GUARD, bool)
        on[:n] = True if active is None else active.cpu().numpy().astype(bool)
        what = (form, n, None if active is None else int(active.sum()))
        assert np.array_equal(p[on], ref_p[:n + GUARD][on]) and np.array_equal(v[on], ref_v[:n + GUARD][on]), what
        assert (p[~on] == NAN).all() and (v[~on] == NAN).all(), what
    if reserved == 4:
        assert dn.range_stats() == (True, 0)


def _zero_layer(net):
    net.res[0][1].conv.weight.zero_()                                # raz_net_build_f16x3's mx == 0 branch


def _tiny_layer(net):
    w = net.res[0][0].conv.weight
    w.mul_(1e-20 / float(w.abs().max()))                             # max |w| ~ 1e-20: S = 2^81, its outputs are its biases


def _huge_layer(net):
    """max |w| ~ 1e6 in the first residual conv, its inputs compensate: stem activations k x 2^-20 (k < 64, exact halfs)."""
    g = torch.Generator().manual_seed(3)
    net.stem.conv.weight.copy_(torch.randint(1, 4, net.stem.conv.weight.shape, generator=g).float() * 2.0 ** -20)
    net.stem.conv.bias.zero_()
    w = net.res[0][0].conv.weight
    w.mul_(1e6 / float(w.abs().max()))
    net.res[0][1].conv.weight.mul_(1e-3)


def _dominant_weight(net):
    w = net.res[0][0].conv.weight
    i = int(w.abs().argmax())
    keep = float(w.view(-1)[i])
    w.mul_(2.0 ** -30)                                               # one weight, the rest 2^-30 smaller
    w.view(-1)[i] = keep


@pytest.mark.parametrize("edit", [_zero_layer, _tiny_layer, _huge_layer, _dominant_weight], ids=lambda f: f.__name__.strip("_"))
def test_f16x3_weight_scales_at_their_edges(edit):
    """raz_net_build_f16x3's per-layer power-of-two scale at the edges of a layer's weights, on a 128x2 net: the split-f16 forward
    against f64 by the same rule as every f16x3 case; no row leaves the f16 range."""
    shape = (128, 2, 16)
    x = _inputs()
    blob, (rp, rv), e32 = _net(shape, seed=41, edit=edit)
    dn, p, v = _forward(blob, 4, x["own_t"], x["enemy_t"])
    assert dn.form(len(p)) == "f16x3_repair"
    e = C.errors(p, v, rp, rv)
    print(f"f16x3 {edit.__name__}: max {e[0]:.3g} mean {e[1]:.3g} vs f64; fp32 torch max {e32[0]:.3g} mean {e32[1]:.3g}")
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert C.within_fp32_rule(e, e32, C.F16X3_FACTOR), (e, e32)
    assert dn.range_stats() == (True, 0)


def _overflowing_blob(F, V):
    """Stem weights all 1e4: a stem activation is 1e4 x the discs of both colours around the square - in range on boards of at most
    one disc per colour, beyond 60000 on a full board.  The residual convs are scaled down so that the trunk stays the stem's."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    net = ReversiNet(F, 1, V).keras_init_(6)
    with torch.no_grad():
        net.stem.conv.weight.fill_(1.0e4)
        net.stem.conv.bias.zero_()
        for cb in net.res[0]:
            cb.conv.weight.mul_(1.0e-7)
    return net.to_blob()


@pytest.mark.parametrize("shape", [(384, 1, 16), (256, 1, 8192)], ids=lambda s: "x".join(map(str, s)))
def test_f16x3_without_repair_raises_the_sticky_flag_on_one_row(shape):
    """The shapes whose rows do not fit a CU's LDS (include/raz.h raz_net_range_check): one row out of the f16 range in a batch
    raises the sticky flag at once and nothing is repaired; the rows in range are what a forward of them alone computes, and
    within 1e-5 of the exact-f32 kernels."""
    F, R, V = shape
    blob = _overflowing_blob(F, V)
    rng = np.random.default_rng(5)
    n = 20
    own = np.array([1 << int(s) for s in rng.integers(0, 64, n)], dtype=np.uint64)
    enemy = np.array([(1 << int(s)) & ~int(o) for s, o in zip(rng.integers(0, 64, n), own)], dtype=np.uint64)
    bad = 13
    own[bad] = rng.integers(0, 2**64, dtype=np.uint64)
    enemy[bad] = ~own[bad]
    own_t, enemy_t = torch.from_numpy(own.view(np.int64)).to(DEV), torch.from_numpy(enemy.view(np.int64)).to(DEV)
    ok = np.arange(n) != bad
    alone, pa, va = _forward(blob, 4, own_t[torch.from_numpy(ok).to(DEV)], enemy_t[torch.from_numpy(ok).to(DEV)])
    assert alone.form(n) == "f16x3_no_repair" and alone.range_stats() == (True, 0)
    dn, p, v = _forward(blob, 4, own_t, enemy_t)
    assert dn.range_stats() == (False, 0) and not dn.range_ok()
    assert np.array_equal(_bits(p[ok]), _bits(pa)) and np.array_equal(_bits(v[ok]), _bits(va))
    _, p1, v1 = _forward(blob, 0, own_t, enemy_t)
    assert np.abs(p[ok] - p1[ok]).max() <= 1e-5 and np.abs(v[ok] - v1[ok]).max() <= 1e-5


@pytest.mark.parametrize("F,reserved", [(16, 0), (128, 0), (128, 4)])
def test_widest_value_head_against_f64(F, reserved):
    """value_fc = RAZ_NET_MAX_VALUE_FC: the heads' (192 + V) floats of LDS are exactly the default 64 KB (k_net_wave in scratch,
    k_heads_wide, k_heads_split); one unit more is refused on the host (tests/test_native_host.py)."""
    from reversi_alpha_zero_amd._native import lib
    shape = (F, 1, C.MAX_V)
    assert lib.raz_net_weight_bytes(F, 1, C.MAX_V + 1) == 0 and lib.raz_net_weight_bytes(*shape) > 0
    x = _inputs()
    blob, (rp, rv), e32 = _net(shape, seed=F + 7)
    dn, p, v = _forward(blob, reserved, x["own_t"], x["enemy_t"])
    assert dn.form(len(p)) == expected_form(F, C.MAX_V, reserved)
    e = C.errors(p, v, rp, rv)
    print(f"{shape} reserved {reserved} {dn.form()}: max {e[0]:.3g} mean {e[1]:.3g} vs f64; fp32 torch max {e32[0]:.3g} mean {e32[1]:.3g}")
    assert C.within_fp32_rule(e, e32, C.F16X3_FACTOR if reserved == 4 else C.EXACT_FACTOR), (e, e32)
