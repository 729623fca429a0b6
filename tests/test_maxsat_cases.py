"""The MaxSAT form cases (tests/maxsat_cases.py) on the host, no GPU: every case's table holds the plane counts its construction
names, the two-valued uniforms keep the reference's float32 rule and the coin in agreement, the table replayed in plain Python
(maxsat_oracle.replay_schedule) is the sequential sweep of the oracle, and the oracle's score is a plain integer count.  What
tests/test_gpu_maxsat_forms.py then compares the kernel with is held to the construction here first."""
import numpy as np
import pytest

import maxsat_cases as mc
import maxsat_oracle as orc

C, NUM_LS = 64, 2


def ms():
    from rlsolver_amd.methods import MCPG_maxsat
    return MCPG_maxsat


def table(case):
    data = ms().make_data(case.nvar, case.clauses, case.weights, case.top, None, "cpu", sorted_nodes=case.order)
    lvp, lvd = data.schedule()
    return data, lvp.numpy(), lvd.numpy()


def words(x01):
    """0|1 [nvar, 64] -> one python int per variable."""
    return [int(sum(int(b) << c for c, b in enumerate(row))) for row in x01]


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_on_the_host(name):
    case = mc.get(name)
    inst = orc.Instance(case.nvar, case.clauses, case.weights, case.top)
    data, lvp, lvd = table(case)
    planes = mc.decode_planes(lvp)
    listed = mc.listed_weights(case.nvar, case.clauses, case.weights)
    assert set(planes) == set(case.planes), (name, sorted(set(planes)))
    assert max(planes) == max(1, max(listed)).bit_length()                       # exactly the width the widest variable needs
    assert set(planes) <= {max(1, w).bit_length() for w in listed}               # and every group's count is some variable's need
    assert len(planes) == case.groups, (name, len(planes))
    assert bool((int(np.asarray(lvp).view(np.uint32)[0]) >> 30) & 1) == (case.weights is not None)
    rng = np.random.RandomState(len(name) + case.nvar)
    start = (rng.rand(case.nvar, C) < 0.5).astype(np.float32)
    uni = mc.two_valued(rng, (NUM_LS, case.nvar, C))
    s = (start.T * 2 - 1).astype(np.float32)
    assert orc.coin_rule_agrees(inst, s, case.order, NUM_LS, uni)
    orc.sweep(inst, s, case.order, NUM_LS, uni)
    want = (s.T + 1) / 2
    coins = [[words([uni[cnt, pos] < 0.5])[0] for pos in range(case.nvar)] for cnt in range(NUM_LS)]
    got = orc.replay_schedule(lvp, lvd, case.nvar, words(start), NUM_LS, coins)
    assert got == words(want)
    # the score in Python ints: S = (satisfied) - (unsatisfied) = 2 satisfied - all, over the non-empty clauses
    total, sat = mc.satisfied_weight(case.nvar, case.clauses, case.weights, want.T)
    assert total < (1 << 24) and [int(v) for v in orc.score(inst, s)] == [2 * k - total for k in sat]
    assert data.num_edges == len(case.clauses)                                   # no clause of a case is hard


def test_saturating_starts_fill_the_counters():
    """From all-zero chains every [x] of a width hub makes and every [-x] breaks (and the reverse from all-one chains): the
    counts the kernel holds are K and K - 1 themselves, in every chain."""
    for p in mc.WIDTHS:
        case, K = mc.get(f"width_{p}"), 1 << (p - 1)
        npos = sum(1 for cl in case.clauses if cl == [1])
        nneg = sum(1 for cl in case.clauses if cl == [-1])
        assert (npos, nneg) == (K, K - 1) and K.bit_length() == p and (K - 1).bit_length() == p - 1 and K - 1 == (1 << (p - 1)) - 1
        inst = orc.Instance(case.nvar, case.clauses)
        for v0 in (0.0, 1.0):
            s = np.full((1, 2), v0 * 2 - 1, dtype=np.float32)
            orc.sweep(inst, s, case.order, 1, np.full((1, 2, 1), 0.75, dtype=np.float32))
            assert ((s[0] + 1) / 2).tolist() == [1.0, 0.0]                       # x goes where K clauses want it, y likewise


def test_every_kernel_form_is_reached_at_both_edges():
    """Each instantiation of ms_group is reached by a case at the lower and one at the upper edge of its plane range -- but for
    the unweighted 24-plane form, whose two cases both sit at its first plane count, 13 (maxsat_cases.FORM_EDGES says why)."""
    lower = {(3, False): 1, (5, False): 4, (8, False): 6, (12, False): 9, (24, False): 13, (8, True): 1, (14, True): 9, (24, True): 15}
    upper = {(3, False): 3, (5, False): 5, (8, False): 8, (12, False): 12, (24, False): 13, (8, True): 8, (14, True): 14, (24, True): 24}
    assert set(mc.FORM_EDGES) == set(lower)
    for form, (lo, hi) in mc.FORM_EDGES.items():
        for name, want in ((lo, lower[form]), (hi, upper[form])):
            case = mc.get(name)
            assert (case.weights is not None) == form[1] and want in case.planes, (form, name)
    # and the cases named here are all in the list the tests run
    assert all(n in mc.NAMES for pair in mc.FORM_EDGES.values() for n in pair) and set(mc.WIDTH_CASES) <= set(mc.NAMES)
