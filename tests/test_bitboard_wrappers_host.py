"""CPU: what lib/bitboard.py's `*_batch` wrappers refuse before they take a pointer.  The entries of include/raz.h get one length and
bare pointers, so a shorter `enemy` would be read past its end on the device and an int64 `action` would be read as bytes and give
wrong boards without an error: the wrappers compare element types, lengths and devices first - and before they ask for device tensors,
so that all of it is checked here with CPU tensors and no such call ever reaches a GPU.  No kernel is launched."""
import pytest
import torch

from reversi_alpha_zero_amd.lib import bitboard as bb

N = 6


def _args():
    u64 = lambda: torch.zeros(N, dtype=torch.int64)
    u8 = lambda: torch.zeros(N, dtype=torch.uint8)
    return {
        "legal_moves_batch": dict(own=u64(), enemy=u64(), out=u64()),
        "calc_flip_batch": dict(pos=u8(), own=u64(), enemy=u64(), out=u64()),
        "step_batch": dict(black=u64(), white=u64(), player=u8(), status=u8(), legal=u64(), action=u8()),
        "score_batch": dict(black=u64(), white=u64()),
        "d4_batch": dict(x=u64(), sym=u8(), out=u64()),
        "planes_batch": dict(own=u64(), enemy=u64()),
        "pick_kth_legal_batch": dict(legal=u64(), rnd=torch.zeros(N, dtype=torch.int32)),
    }


CALLS = [(fn, arg) for fn, kw in _args().items() for arg in kw]
FIRST = {fn: ("own" if fn == "calc_flip_batch" else next(iter(kw))) for fn, kw in _args().items()}   # the tensor that gives the length


@pytest.mark.parametrize("fn", sorted(_args()))
def test_a_well_formed_cpu_call_is_still_refused_as_device_only(fn):
    with pytest.raises(ValueError, match="device-only"):
        getattr(bb, fn)(**_args()[fn])
    kw = {k: v for k, v in _args()[fn].items() if k != "out"}
    with pytest.raises(ValueError, match="device-only"):
        getattr(bb, fn)(**kw)
    if fn == "pick_kth_legal_batch" and hasattr(torch, "uint32"):
        with pytest.raises(ValueError, match="device-only"):
            bb.pick_kth_legal_batch(kw["legal"], torch.zeros(N, dtype=torch.uint32))


@pytest.mark.parametrize("fn,arg", CALLS)
def test_a_tensor_of_another_length_is_a_value_error_that_names_it(fn, arg):
    for n in (N - 1, N + 1, 0):
        kw = _args()[fn]
        kw[arg] = kw[arg][:n] if n < N else torch.cat([kw[arg], kw[arg][:1]])
        other = FIRST[fn] if arg != FIRST[fn] else next(k for k in kw if k != arg)
        with pytest.raises(ValueError, match="elements") as e:
            getattr(bb, fn)(**kw)
        assert fn in str(e.value) and (arg in str(e.value).split() or other in str(e.value).split()), str(e.value)
        assert "device-only" not in str(e.value)


@pytest.mark.parametrize("fn,arg", CALLS)
def test_a_tensor_of_another_element_type_is_a_type_error_that_names_it(fn, arg):
    good = _args()[fn][arg].dtype
    wrong = {torch.int64: (torch.int32, torch.float64, torch.uint8), torch.uint8: (torch.int64, torch.int8, torch.bool, torch.int32),
             torch.int32: (torch.int64, torch.float32, torch.int16, torch.uint8)}[good]
    for dt in wrong:
        kw = _args()[fn]
        kw[arg] = kw[arg].to(dt)
        with pytest.raises(TypeError) as e:
            getattr(bb, fn)(**kw)
        assert fn in str(e.value) and arg in str(e.value).split(), str(e.value)
    kw = _args()[fn]
    kw[arg] = kw[arg].numpy()
    with pytest.raises(TypeError):
        getattr(bb, fn)(**kw)


@pytest.mark.parametrize("fn,arg", [(f, a) for f, a in CALLS if a != FIRST[f]])
def test_a_tensor_on_another_device_is_a_value_error_that_names_it(fn, arg):
    kw = _args()[fn]
    kw[arg] = kw[arg].to("meta")            # (a device that needs no hardware: nothing is read from it)
    with pytest.raises(ValueError, match=" is on ") as e:
        getattr(bb, fn)(**kw)
    assert fn in str(e.value) and arg in str(e.value).split(), str(e.value)


def test_sweep_max_grid_is_the_default_without_the_variable():
    import os
    if "RAZ_SWEEP_MAXGRID" not in os.environ:
        assert bb.sweep_max_grid() == 65536
