"""The MaxSAT sampler kernel (rls_maxsat_local_search) on every case of tests/maxsat_cases.py: each counter width at its edges
with the counters full, weighted carry ripples, ties at every width, stream lengths and clause ends at the block edges, levels of
more groups than waves, clause counts at the score loop's trip edges -- chains and ``expected`` against the numpy oracle
(tests/maxsat_oracle.py), bit for bit.  There is no tolerance anywhere: every compared quantity is 0 | 1 or an integer below
2^24 held in a float32.

Uniforms are two-valued (maxsat_cases.two_valued): the reference's float32 rule and the kernel's coin then agree up to a listed
weight of 2^22, and at the weight limit while |old| stays small; check_kernel asserts the agreement on the oracle's side for every
run.  tests/test_maxsat_cases.py holds each case to its plane counts on the host; here the table is decoded once more on the
device's copy, so a case cannot reach the kernel on another form than the one it is named for."""
import functools

import numpy as np
import pytest
import torch

import maxsat_cases as mc
import maxsat_oracle as orc
from test_gpu_maxsat import check_kernel, dev, ms, packed

pytestmark = pytest.mark.gpu

LAYOUT_CASES = ("company_5", "weighted_three_widths")


@functools.lru_cache(maxsize=None)
def built(name):
    case = mc.get(name)
    data = ms().make_data(case.nvar, case.clauses, case.weights, case.top, None, dev(), sorted_nodes=case.order)
    planes = mc.decode_planes(data.schedule()[0].cpu().numpy())
    assert set(planes) == set(case.planes) and len(planes) == case.groups, (name, planes)
    return data, orc.Instance(case.nvar, case.clauses, case.weights, case.top), case.order


def saturating_start(nvar):
    """128 chains: all variables 0 (every [x] makes) and all variables 1 (every [-x] makes), alternating within the first word
    and as two halves of the second."""
    cols = np.array([0, 1] * 32 + [0] * 32 + [1] * 32, dtype=np.float32)
    return np.tile(cols, (nvar, 1))


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_against_the_oracle(name):
    data, inst, order = built(name)
    for num_ls in (0, 2):
        check_kernel(data, inst, order, 64, num_ls, seed=10 + num_ls, draw=mc.two_valued)


@pytest.mark.parametrize("name", mc.WIDTH_CASES)
def test_width_case_from_the_saturating_starts(name):
    data, inst, order = built(name)
    check_kernel(data, inst, order, 128, 2, seed=3, draw=mc.two_valued, start=saturating_start(inst.nvar))


def bits_past(xs, C):
    """The bits of the packed words at and past chain C (the layout's rule: zero)."""
    w = xs.words.cpu().numpy().view(np.uint64)
    assert w.shape[0] == (C + 63) // 64
    return w[-1] & ~np.uint64((1 << (C % 64)) - 1) if C % 64 else np.zeros(1, dtype=np.uint64)


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layouts(name):
    data, inst, order = built(name)
    for C in (1, 63, 65, 200):                                                    # packed output, a ragged last tile
        xs, _ = check_kernel(data, inst, order, C, 2, seed=C, draw=mc.two_valued)
        assert not bits_past(xs, C).any(), C
    for c_in, C in ((64, 200), (128, 320)):                                       # a broadcast start meets a ragged C
        xs, _ = check_kernel(data, inst, order, C, 2, seed=C + c_in, c_in=c_in, draw=mc.two_valued)
        assert not bits_past(xs, C).any(), (c_in, C)
    xs, _ = check_kernel(data, inst, order, 200, 2, seed=7, draw=mc.two_valued, in_place=True)
    assert not bits_past(xs, 200).any()
    for C in (1, 63):                                                             # the f32 surface below one tile
        check_kernel(data, inst, order, C, 2, seed=100 + C, draw=mc.two_valued, packed_out=False)


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_shards_of_a_broadcast_launch(name):
    """Two ranks that each own 64 of 128 kept chains x 2 repeats draw what the one 256-chain launch draws (production coins)."""
    data, inst, _ = built(name)
    rng = np.random.RandomState(17)
    start = packed().pack(torch.from_numpy((rng.rand(inst.nvar, 64) < 0.5).astype(np.float32)).to(dev()))
    whole, e_whole = data.local_search(start, 2, seed=4321, out=packed().empty(inst.nvar, 256, dev()), num_chains=256)
    w = whole.unpack()
    for half in (0, 1):
        cols = torch.cat([torch.arange(r * 128 + half * 64, r * 128 + half * 64 + 64) for r in range(2)]).to(dev())
        xs, e = data.local_search(start, 2, seed=4321, out=packed().empty(inst.nvar, 128, dev()), num_chains=128, chain_ids=(half * 64, 64, 64))
        assert torch.equal(xs.unpack(), w[:, cols]) and torch.equal(e, e_whole[cols]), half
    # the whole launch itself: the score of its own chains, in Python ints
    total, sat = mc.satisfied_weight(inst.nvar, inst.clauses, inst.weights, w.cpu().numpy().T)
    assert [int(v) for v in e_whole.cpu().numpy()] == [total - 2 * k for k in sat]


@pytest.mark.parametrize("name", ["width_13", "w24_limit", "company_12"])
def test_production_draws_decide_only_ties(name):
    """With the kernel's own coins (seed) every decision that is not a tie equals the oracle's.  One pass: a variable is decided
    once, so where new == old -- computed here, exactly -- the kernel's own bit is taken over and every other decision, and with
    it the whole tile, must follow.  (A case whose decisions are mostly ties would check nothing.)"""
    data, inst, order = built(name)
    C = 128
    rng = np.random.RandomState(13)
    start = (rng.rand(inst.nvar, C) < 0.5).astype(np.float32)
    xs, expected = data.local_search(packed().pack(torch.from_numpy(start).to(dev())), 1, seed=2026, out=packed().empty(inst.nvar, C, dev()))
    got = (xs.unpack().cpu().numpy().T * 2 - 1).astype(np.float32)
    s = (start.T * 2 - 1).astype(np.float32)
    ties = [0]

    def decide(cnt, pos, i, old, new):
        tie = new.astype(np.float64) == old.astype(np.float64)
        ties[0] += int(tie.sum())
        return np.where(tie, got[:, i] == s[:, i], new > old)              # (s[:, i] holds the flipped value here)
    orc.visit(inst, s, order, 1, decide)
    assert 2 * ties[0] <= inst.nvar * C, ties
    assert np.array_equal(got, s)
    assert np.array_equal(expected.cpu().numpy(), -orc.score(inst, s))
