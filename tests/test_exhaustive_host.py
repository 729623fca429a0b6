"""Exhaustive enumeration, the parts that need no GPU: the numpy restatement against the reference's own `_calc_over_range`
(tests/golden/spin_exhaustive.npz, tools/gen_golden_exhaustive.py), the range split, the key layout, and the new entries at every
layer (header, ctypes table, op list, env classes)."""
import os
import re

import numpy as np
import pytest

from tests import exhaustive_oracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rls_spin_exhaustive_pack", "rls_spin_exhaustive")


def test_oracle_reproduces_the_reference(golden):
    z = golden("spin_exhaustive")
    sizes = set()
    for tag in z["cases"]:
        W, ranges = z[f"{tag}/W"], z[f"{tag}/ranges"]
        sizes.add(W.shape[0])
        assert np.array_equal(W, W.T) and set(np.unique(W[~np.eye(len(W), dtype=bool)])) <= {-1.0, 0.0, 1.0}
        for k, (i0, i1) in enumerate(ranges):
            e, i, s = xo.calc_over_range(W, int(i0), int(i1))
            assert e == z[f"{tag}/energy"][k], (tag, k)
            assert np.array_equal(s, z[f"{tag}/spins"][k]), (tag, k)
            assert xo.index_of(s) == i and i0 <= i < i1
            assert e == xo.e_off(W, s) - np.trace(W) / 2                       # the trace term is real with a diagonal
            assert xo.cut(W, s) == (np.triu(W, 1).sum() + xo.e_off(W, s)) / 2   # the cut identity
        assert tuple(ranges[0]) == (0, 1 << W.shape[0]) and z[f"{tag}/spins"][0][0] == -1.0    # global flip: the first of the pair wins
    assert sizes == {5, 11, 12, 16}
    assert any(np.trace(z[f"{tag}/W"]) != 0 for tag in z["cases"])


def test_the_reference_s_own_calculate_best_energy_raises(golden):
    """The claim of the envs' docstrings, as data: at n_spins <= 10 an undefined method, above a float count given to np.linspace."""
    z = golden("spin_exhaustive")
    assert str(z["calculate_best_energy/n5"]).startswith("AttributeError")
    assert str(z["calculate_best_energy/n12"]).startswith("TypeError")
    assert float(z["reference_states_per_second"]) > 0


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("total", [0, 1, 5, 1 << 13, (1 << 13) - 8, (1 << 48) - 3])
def test_split_range_covers_the_range_without_gap_or_overlap(world, total):
    from rlsolver_amd.ops import split_range
    parts = [split_range(total, r, world) for r in range(world)]
    assert parts == [xo.split_range(total, r, world) for r in range(world)]
    assert parts[0][0] == 0 and parts[-1][1] == total
    for (a, b), (c, d) in zip(parts, parts[1:]):
        assert b == c
    lens = [b - a for a, b in parts]
    assert min(lens) >= 0 and max(lens) - min(lens) <= 1 and sum(lens) == total
    for bad in ((total, world, world), (total, -1, world), (total, 0, 0), (-1, 0, 1)):
        with pytest.raises(ValueError):
            split_range(*bad)


def test_key_round_trips_at_the_extremes():
    from rlsolver_amd import ops
    top = (1 << 48) - 1
    for e in (-2256, -1128, -1, 0, 1, 1128, 2256):
        for i in (0, 1, 1 << 31, 1 << 32, top):
            k = ops.exhaustive_key_encode(e, i)
            assert k == xo.key_encode(e, i) and 0 <= k < ops.EXHAUSTIVE_KEY_EMPTY
            assert ops.exhaustive_key_decode(k) == (e, i) == xo.key_decode(k)
    # the order of the keys is the order of (energy, index)
    assert ops.exhaustive_key_encode(-3, top) < ops.exhaustive_key_encode(-2, 0) < ops.exhaustive_key_encode(-2, 1)
    import torch
    k = torch.tensor([xo.key_encode(-2256, top), xo.key_encode(2256, 0)], dtype=torch.int64)
    e, i = ops.exhaustive_key_decode(k)
    assert e.tolist() == [-2256, 2256] and i.tolist() == [top, 0]
    assert ops.EXHAUSTIVE_KEY_BIAS == xo.KEY_BIAS and ops.EXHAUSTIVE_KEY_EMPTY == xo.KEY_EMPTY == (1 << 63) - 1


def test_header_declares_both_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rlsolver_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
    assert "#define RLS_ABI_VERSION 12" in src


def test_ctypes_table_and_op_list_hold_both():
    from rlsolver_amd import _abi, build, torch_ops
    for name in ENTRIES:
        assert name in _abi.SIGNATURES, name
        assert name[len("rls_"):] in torch_ops.DEVICE_ENTRY_POINTS, name
    assert "rls_exhaustive.hip" in build.SOURCES


def test_the_c_entries_refuse_bad_sizes_before_any_device_work():
    from rlsolver_amd import _abi
    for args in ((None, None, 1, 49, 0, 1, None, None), (None, None, 1, 0, 0, 1, None, None), (None, None, 1, 5, 3, 3, None, None),
                 (None, None, 1, 5, 0, 33, None, None), (None, None, 1, 5, -1, 4, None, None), (None, None, 1, 5, 0, 32, None, None)):
        with pytest.raises(_abi.RlsError) as e:
            _abi.call("rls_spin_exhaustive", *args)
        assert e.value.code == -1
    for args in ((None, 4, 1, 49, None, None, None, None), (None, 2, 1, 5, None, None, None, None), (None, 8, 1, 5, None, None, None, None)):
        with pytest.raises(_abi.RlsError):
            _abi.call("rls_spin_exhaustive_pack", *args)


def test_env_classes_expose_the_three_methods():
    from rlsolver_amd.envs.spinsystem import SpinSystem, SpinSystemUnbiased
    for cls in (SpinSystem, SpinSystemUnbiased):
        for name in ("_calc_over_range", "calculate_best_energy", "calculate_best"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
        assert "reference raises" in cls.calculate_best_energy.__doc__
