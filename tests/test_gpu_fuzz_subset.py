"""A seeded 5-second slice of tools/fuzz/fuzz_subset.py (sub_set_sampling against its numpy restatement) from another seed than
the one tests/test_gpu_fuzzers.py gives every fuzzer, so that the two slices cover different configurations."""
import os
import runpy
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_subset_slice(capsys, monkeypatch):
    path = os.path.join(ROOT, "tools", "fuzz", "fuzz_subset.py")
    monkeypatch.chdir(ROOT)
    monkeypatch.setattr(sys, "argv", [path, os.environ.get("RLS_FUZZ_SECONDS", "5"), "20261020"])
    runpy.run_path(path, run_name="__main__")                 # an AssertionError names the failing configuration
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last.startswith("fuzz_subset: ") and last.endswith("random configurations, no mismatch") and int(last.split()[1]) >= 1, last
