"""K4's block order (csrc/rls_step_plan.h), asked through rls_maxcut_step_block of the C ABI -- the function the kernels call, on the
host, without a device.  Order 1 (xcd-fwd) must send the workgroups of a grid to every block exactly once for ANY grid size: a block
hit twice would have two workgroups write one run, a block left out a run that is never written."""
import ctypes as C

import numpy as np
import pytest

from rlsolver_amd import _abi

RLS_OK, RLS_EINVAL = 0, -1


def block_map(order, nb):
    fn = _abi.lib().rls_maxcut_step_block
    fn.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
    fn.restype = C.c_int
    out = C.c_int64(-1)
    ref = C.byref(out)
    vb = np.empty(nb, dtype=np.int64)
    for b in range(nb):
        assert fn(order, b, nb, ref) == RLS_OK
        vb[b] = out.value
    return vb


SIZES = list(range(1, 4101)) + [2 ** 14 - 1, 2 ** 14, 2 ** 14 + 1]


def test_xcd_fwd_is_a_bijection_for_every_grid_size():
    for nb in SIZES:
        vb = block_map(1, nb)
        assert np.array_equal(np.sort(vb), np.arange(nb)), nb


def test_forward_is_the_identity():
    for nb in (1, 2, 7, 8, 9, 63, 64, 65, 4096, 4099, 2 ** 14 + 1):
        assert np.array_equal(block_map(0, nb), np.arange(nb)), nb


@pytest.mark.parametrize("nb", [8, 16, 64, 4096, 2 ** 14])
def test_one_contiguous_range_per_class_of_eight(nb):
    """nb % 8 == 0: the blocks with equal b % 8 (one XCD under round-robin placement) take [x nb / 8, (x + 1) nb / 8), in order."""
    vb = block_map(1, nb)
    for x in range(8):
        assert np.array_equal(vb[x::8], np.arange(x * nb // 8, (x + 1) * nb // 8)), x


@pytest.mark.parametrize("nb", [1, 5, 9, 13, 4099])
def test_classes_stay_contiguous_and_ordered_on_ragged_grids(nb):
    """nb % 8 != 0: still one ascending contiguous range per class, the ranges following each other in the order of the classes."""
    vb = block_map(1, nb)
    start = 0
    for x in range(min(8, nb)):
        mine = vb[x::8]
        assert np.array_equal(mine, np.arange(start, start + len(mine))), x
        start += len(mine)
    assert start == nb


def test_refusals():
    fn = _abi.lib().rls_maxcut_step_block
    fn.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
    fn.restype = C.c_int
    out = C.c_int64(0)
    for order, b, nb, ref in [(2, 0, 8, C.byref(out)), (-1, 0, 8, C.byref(out)), (1, 8, 8, C.byref(out)), (1, -1, 8, C.byref(out)),
                              (1, 0, 0, C.byref(out)), (1, 0, 8, None)]:
        assert fn(order, b, nb, ref) == RLS_EINVAL, (order, b, nb)


def test_the_knob_is_registered():
    assert "RLS_STEP_ORDER" in _abi.tuning_names()
