"""CPU: the memory-contract helper (tests/memcheck.py) catches each class of violation it exists for, on CPU tensors with a
fake "kernel" - what keeps the net of tests/test_hip_memory_contract.py from silently going slack - and the GPU module's
declared coverage equals the kernel-launching entry points of include/tdc_hip.h."""
import re

import pytest
import torch

import memcheck as mc

ROWS, COLS, LD, BAND = 5, 6, 8, 4


def _kernel(x, y, rows, cols, ldx, ldy, bug=None):
    """y[r, c] = 2 * x[r, c] on flat storage, the way a device kernel addresses its operands (row * ld + col from the base
    pointer - a negative or too large index lands in the arena around the view, never outside it)."""
    xs, ys = x._base_flat, y._base_flat
    for r in range(rows):
        for c in range(cols):
            ys[y._base_off + r * ldy + c] = 2 * xs[x._base_off + r * ldx + c]
    if bug == "row_past_end":
        ys[y._base_off + rows * ldy + 1] = 1.0
    elif bug == "pad_column":
        ys[y._base_off + 2 * ldy + cols] = 1.0
    elif bug == "front_band":
        ys[y._base_off - 3] = 1.0
    elif bug == "reads_poison":                                  # an unmasked clamped load: row `rows` of x joins row 0 of y
        ys[y._base_off] = ys[y._base_off] + 0 * xs[x._base_off + rows * ldx]


def _flat(view, arena):
    """attach the arena's flat typed storage + the view's element offset (what a raw pointer is to a kernel)"""
    view._base_flat = arena.buf.view(arena.dtype)
    view._base_off = arena.front // arena.item
    return view


def _run(fill, bug=None, dtype=torch.float32):
    data = (torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS) / 7 - 2).to(dtype)
    x, xa = mc.poisoned(data, BAND, BAND, ld=LD, fill=fill)
    y, ya = mc.guarded((ROWS, COLS), dtype, "cpu", BAND, BAND, ld=LD, fill=fill)
    _kernel(_flat(x, xa), _flat(y, ya), ROWS, COLS, LD, LD, bug)
    return data, y, ya


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_a_correct_kernel_passes(dtype):
    outs = []
    for fill in mc.PATTERNS:
        data, y, ya = _run(fill, dtype=dtype)
        mc.assert_untouched(ya)
        assert torch.equal(y, 2 * data)
        outs.append(y.clone())
    assert mc.same_bits(outs[0], outs[1]) and mc.all_finite(outs[1])


@pytest.mark.parametrize("bug,where", [("row_past_end", (ROWS, 1)), ("pad_column", (2, COLS)), ("front_band", (-1, LD - 3))])
@pytest.mark.parametrize("fill", mc.PATTERNS)
def test_a_stray_store_is_caught_and_located(bug, where, fill):
    _, _, ya = _run(fill, bug)
    with pytest.raises(AssertionError) as e:
        mc.assert_untouched(ya)
    assert "(%d, %d)" % where in str(e.value), str(e.value)


def test_a_poisoned_read_is_caught():
    outs = []
    for fill in mc.PATTERNS:
        _, y, ya = _run(fill, "reads_poison")
        mc.assert_untouched(ya)                                  # the write set is honoured: only the read set is not
        outs.append(y.clone())
    assert not mc.same_bits(outs[0], outs[1])
    assert mc.all_finite(outs[0]) and not mc.all_finite(outs[1])
    bad = torch.nonzero(~torch.isfinite(outs[1]))
    assert bad.tolist() == [[0, 0]]                              # ... and the position is named


def test_the_nan_pattern_is_nan_in_every_type_of_the_path():
    raw = torch.full((8,), mc.NAN_FF, dtype=torch.uint8)
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float8_e4m3fn):
        assert bool(torch.isnan(raw.view(dt).float()).all()), dt
    assert raw.view(torch.int32).tolist() == [-1, -1]


def test_write_masks_rows_elements_and_pad_columns():
    y, ya = mc.guarded((4, 3), torch.float16, "cpu", 2, 2, ld=8)
    assert y.shape == (4, 3) and y.stride() == (8, 1) and (y.data_ptr() - ya.buf.data_ptr()) % 256 == 0
    assert bool(torch.isnan(y.float()).all())                    # the view's previous contents are the sentinel too
    y[1] = 1.0
    mc.assert_untouched(ya, torch.tensor([False, True, False, False]))
    with pytest.raises(AssertionError, match=r"\(1, 0\)"):
        mc.assert_untouched(ya, torch.tensor([True, False, True, True]))
    ya.full[1, 3:5] = 0                                          # pad columns: legal only under an [rows, ld] element mask
    with pytest.raises(AssertionError, match=r"\(1, 3\)"):
        mc.assert_untouched(ya, torch.tensor([False, True, False, False]))
    m = torch.zeros(4, 8, dtype=torch.bool)
    m[1, :5] = True
    mc.assert_untouched(ya, m)
    v, va = mc.guarded((7,), torch.float32, "cpu", 16, 16)       # 1-D: n rows of one element
    v[:] = 0
    mc.assert_untouched(va)
    va.buf[va.front + 7 * 4] = 0
    with pytest.raises(AssertionError, match=r"\(7, 0\)"):
        mc.assert_untouched(va)


def test_poisoned_row_gaps_and_pad_columns():
    data = torch.ones(3, 4, dtype=torch.bfloat16)
    x, xa = mc.poisoned(data, 1, 1, ld=8, rows=[0, 2, 5], total_rows=6)
    f = xa.full.float()
    assert torch.equal(f[[0, 2, 5], :4], torch.ones(3, 4)) and torch.count_nonzero(f[[0, 2, 5], 4:]) == 0
    assert bool(torch.isnan(f[[1, 3, 4]]).all())
    x2, xa2 = mc.poisoned(data, 1, 1, ld=8, fill=mc.ZERO, pad="poison")
    assert torch.count_nonzero(xa2.buf.view(torch.bfloat16).float()) == 12
    _, xa3 = mc.poisoned(data, 1, 1, ld=8, pad="poison")
    assert bool(torch.isnan(xa3.full[:, 4:].float()).all())


def test_poison_empty_patches_only_the_package_and_is_undone(monkeypatch):
    import types
    import sys
    mod = types.ModuleType("fakepkg_memcheck.sub")
    mod.torch = torch
    mod.make = lambda: (mod.torch.empty(3, 5, dtype=torch.float16), mod.torch.empty_like(torch.zeros(2, 2)),
                        mod.torch.empty((4,), dtype=torch.int32), mod.torch.zeros(2))
    monkeypatch.setitem(sys.modules, "fakepkg_memcheck.sub", mod)
    with monkeypatch.context() as mp:
        mc.poison_empty(mp, mc.NAN_FF, prefix="fakepkg_memcheck")
        a, b, c, z = mod.make()
        assert bool(torch.isnan(a.float()).all()) and bool(torch.isnan(b).all()) and c.tolist() == [-1] * 4
        assert a.shape == (3, 5) and b.shape == (2, 2) and torch.count_nonzero(z) == 0
        assert mod.torch.float16 is torch.float16
    assert mod.torch is torch
    with monkeypatch.context() as mp:
        arenas = mc.poison_empty(mp, mc.ZERO, guard_bytes=64, prefix="fakepkg_memcheck")
        a, b, c, _ = mod.make()
        assert len(arenas) == 3 and torch.count_nonzero(a.float()) == 0
        a.fill_(1.0)
        c.fill_(7)
        for ar in arenas:
            mc.assert_untouched(ar)
        arenas[2].buf[arenas[2].front - 1] = 9                     # one byte in front of the int32 vector
        with pytest.raises(AssertionError, match=r"\(-1, 0\)"):
            mc.assert_untouched(arenas[2])


def test_every_kernel_launching_entry_point_is_in_the_memory_contract_module():
    """the symbol list of the C ABI minus the entry points that launch nothing == what the GPU module declares it covers,
    and the source of every test that declares a name holds the symbol or the ops / engine call that wraps it"""
    import os
    import test_hip_memory_contract as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tdc_hip.h")).read()
    declared = set(re.findall(r"\b(tdc_[a-z0-9_]+)\s*\(", hdr))
    assert T.NON_LAUNCHING <= declared, T.NON_LAUNCHING - declared
    assert declared - T.NON_LAUNCHING == set(T.COVERED), (declared - T.NON_LAUNCHING) ^ set(T.COVERED)
    import inspect
    for name, tests in T.COVERED.items():                       # the symbol, or the wrapper that calls it, is in the test's source
        for fn in tests:
            body = inspect.getsource(getattr(T, fn)).split("def " + fn, 1)[1]        # without the @covers line above it
            assert name in body or T.WRAPPERS.get(name, "\0") in body, (name, fn)
