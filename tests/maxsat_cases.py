"""Shared inputs of the MaxSAT form tests (tests/test_maxsat_cases.py on the host, tests/test_gpu_maxsat_forms.py on the GPU):
named formulas that put the sampler's bit-sliced make / break counters (csrc/rls_maxsat.hip: ms_add, ms_group) at the edges
random 3-SAT never reaches.  No GPU; nothing of the product beyond MCPG_maxsat.make_data.

Why these inputs.  The kernel picks a counter width per GROUP of 64 variables from the `planes` the host writes into the table
(unweighted: <= 3 | 5 | 8 | 12 | else 24; weighted: <= 8 | 14 | else 24), planes = bit length of the largest weight one variable
of the group lists.  A hub with K = 2^(p-1) unit clauses [x] and K - 1 clauses [-x] lists 2^p - 1: the host must say exactly p, a
make count of K lives in the top plane alone, a break count of K - 1 fills every plane below it, and every listed clause is
critical in every chain (a unit clause has no other literal): the counters are FULL.  A carry lost in the top plane, a compare
that starts one plane low, a dispatch that sends a width to the narrower form or a host `planes` one short all turn the hub's
decision.  K against K is the tie only the coin decides (p + 1 planes).  The weighted cases do the same with single weights whose
sums ripple through the full-adder chain.  The stream, level and score cases build on purpose what a random formula leaves to
chance: stream lengths of 4k, 4k + 1 and 4k + 3 entries, clauses that end on the last entry of a block or straddle blocks, one long
stream beside 63 short ones, more groups in a level than the workgroup has waves, clause counts at the score loop's trip edges.

Every case names the SET of plane counts its table must hold and the number of its groups -- written down from the construction
where a case is built by hand, recorded per seed where its formula or order is drawn: tests/test_maxsat_cases.py holds the host
library to both, so a later change of the table cannot move a case off its kernel form unnoticed.

Uniforms.  The reference's float32 accept rule and the kernel's coin "u < 1/2" agree everywhere but in a band of width ulp(|old|) / 2
below 1/2.  Draws from {0.25, 0.75} stay out of that band up to |old| < 2^22, far past the 2^13 the recorded-draw tests allow;
`two_valued` is that generator and every test asserts the agreement on the oracle's side (maxsat_oracle.coin_rule_agrees).
"""
from __future__ import annotations

import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name nvar clauses weights top order planes groups")
# planes: the exact set of plane counts in lv_ptr, groups: the number of group records.  For the hand-built cases both follow from
# the construction; for the seeded random ones (the score cases, the visiting order of stream_block_edges) they are RECORDED from
# the host table of that seed -- a pin, so that a table change shows -- and tests/test_maxsat_cases.py holds every set to the bit
# lengths of the listed weights besides

TOP = 1 << 24                     # the hard weight of the weighted cases: above every weight used, so no clause is hard


def two_valued(rng, shape):
    """Uniforms from {0.25, 0.75}: u < 1/2 is a fair coin and no draw sits where the float32 rule and the coin differ."""
    return np.where(rng.rand(*shape) < 0.5, np.float32(0.25), np.float32(0.75)).astype(np.float32)


def decode_planes(lv_ptr):
    """The plane count of every group record of lv_ptr (include/rlsolver_hip.h: bits 24..28), as a list."""
    lp = np.asarray(lv_ptr).view(np.uint32)[:-1]
    return ((lp >> 24) & 31).astype(int).tolist()


def listed_weights(nvar, clauses, weights=None):
    """Per variable, the weight of the clauses listed for it -- once per OCCURRENCE of the variable -- in Python ints."""
    out = [0] * nvar
    for c, cl in enumerate(clauses):
        for l in cl:
            out[abs(l) - 1] += 1 if weights is None else int(weights[c])
    return out


def satisfied_weight(nvar, clauses, weights, x01):
    """Plain integer score per chain: (weight of the non-empty clauses, [weight of the satisfied clauses per chain]).  x01: rows of
    0 | 1 per chain.  Python ints only; equal clauses are counted once and multiplied."""
    mult = collections.Counter((tuple(cl), 1 if weights is None else int(weights[c])) for c, cl in enumerate(clauses) if cl)
    total = sum(w * n for (_, w), n in mult.items())
    sat = []
    for row in x01:
        bits = [int(b) for b in row]
        sat.append(sum(w * n for (cl, w), n in mult.items() if any(bits[abs(l) - 1] == (1 if l > 0 else 0) for l in cl)))
    return total, sat


def _case(name, nvar, clauses, weights=None, order=None, planes=(), groups=None):
    assert planes and groups
    order = np.arange(nvar) if order is None else np.asarray(order)
    assert sorted(order.tolist()) == list(range(nvar))
    return Case(name, nvar, clauses, weights, None if weights is None else TOP, order, frozenset(planes), groups)


def _sign(rng, v):
    return int(v) * (1 if rng.rand() < 0.5 else -1)


# ----------------------------------------------------------------------------- unweighted width edges
WIDTHS = (2, 3, 4, 5, 6, 8, 9, 12, 13)
TIES = (2, 3, 4, 5, 6, 8, 9, 12)          # K against K: p + 1 planes, so 3 -> 4, 5 -> 6, 8 -> 9 and 12 -> 13 cross a dispatch edge
COMPANY = (3, 5, 8, 12)


def hub(x, npos, nneg):
    """npos clauses [x] and nneg clauses [-x], interleaved while both last (the counters grow together)."""
    both = min(npos, nneg)
    return [[x], [-x]] * both + [[x]] * (npos - both) + [[-x]] * (nneg - both)


def width(p):
    """x: K [x] against K - 1 [-x]; y: the mirror image.  Both list 2^p - 1 in one group: exactly p planes."""
    K = 1 << (p - 1)
    return _case(f"width_{p}", 2, hub(1, K, K - 1) + hub(2, K - 1, K), planes={p}, groups=1)


def tie(p):
    """K [x] against K [-x]: make == break in every chain, the coin decides; the listed 2^p needs p + 1 planes."""
    K = 1 << (p - 1)
    return _case(f"tie_{p}", 1, hub(1, K, K), planes={p + 1}, groups=1)


def company(p, m=6):
    """The width-p hub, every clause of it with one more literal of one of m variables visited BEFORE the hub: the hub sits in
    level 2, a clause is critical only in the chains where its companion literal is false, so make / break differ per chain and
    per plane.  Companion c is in the clauses j = c (mod m): it lists ceil((2K - 1 - c) / m) of them, the most for c = 0."""
    K = 1 << (p - 1)
    x = m + 1
    clauses = [[x if j < K else -x, (j % m + 1) * (1 if (j // m) % 3 else -1)] for j in range(2 * K - 1)]
    most = -(-(2 * K - 1) // m)
    return _case(f"company_{p}", m + 1, clauses, planes={p, most.bit_length()}, groups=2)


# ----------------------------------------------------------------------------- weighted width edges
WEIGHTED = {                       # name: ((a, b), planes): [x]:a against [-x]:b
    "w8": ((127, 128), 8),                               # <8, true> at its edge
    "w9": ((255, 256), 9),                               # first of <14, true>
    "w14": ((0x2AAA, 0x1555), 14),                       # last of <14, true>
    "w15": ((0x4000, 0x3FFF), 15),                       # first of <24, true>
    "w22_tie": ((0x1FFFFF, 0x1FFFFF), 22),               # a tie
    "w24_limit": (((1 << 23), (1 << 23) - 1), 24),       # the weight limit: the formula's total is 2^24 - 1
}
RIPPLES = {                        # name: (weights of [x] clauses, weights of [-x] clauses, planes)
    "ripple_tie": ((0x0FFF, 1), (0x1000,), 14),          # 0x0FFF + 1 ripples through 12 planes into a tie
    "ripple_win": ((0x0FFF, 1), (0x0FFF,), 13),          # the same, make wins by 1
    "ripple_5555": ((0x5555, 0x2AAA), (0x7FFF,), 16),    # alternating planes add up to all ones: a tie
}


def weighted_pair(name):
    """[x]:a against [-x]:b and, where the formula's total stays within 2^24 - 1, the mirror image on y."""
    (a, b), planes = WEIGHTED[name]
    clauses, weights = [[1], [-1]], [a, b]
    if 2 * (a + b) <= (1 << 24) - 1:
        clauses, weights = clauses + [[2], [-2]], weights + [b, a]
    assert (a + b).bit_length() == planes
    return _case(name, len(clauses) // 2, clauses, weights, planes={planes}, groups=1)


def ripple(name):
    pos, neg, planes = RIPPLES[name]
    assert (sum(pos) + sum(neg)).bit_length() == planes
    clauses = [[1]] * len(pos) + [[-1]] * len(neg) + [[-2]] * len(pos) + [[2]] * len(neg)
    return _case(name, 2, clauses, list(pos + neg) * 2, planes={planes}, groups=1)


def weighted_three_widths():
    """Three weighted widths in three levels (a - b and b - c share a clause): 1, 9 and 16 planes, one kernel form each."""
    clauses = [[1, 2], [2], [-2], [2, 3], [3], [-3]]
    weights = [1, 300, 200, 1, 0x4000, 0x4001]
    return _case("weighted_three_widths", 3, clauses, weights, planes={1, (1 + 300 + 200 + 1).bit_length(), (1 + 0x8001).bit_length()}, groups=3)


# ----------------------------------------------------------------------------- stream geometry
def stream_lengths():
    """Five variables in a chain of binary clauses (so: five levels, five groups) whose streams have 4, 5, 7, 8 and 9 entries:
    a link is one entry at either end, the rest are unit clauses of alternating sign."""
    units = (3, 3, 5, 6, 8)                                # + 1, 2, 2, 2, 1 links
    clauses = [[i + 1, -(i + 2)] for i in range(4)]
    for i, n in enumerate(units):
        clauses += [[(i + 1) * (1 if k % 2 == 0 else -1)] for k in range(n)]
    return _case("stream_lengths", 5, clauses, planes={3, 4}, groups=5)        # listed 4, 5, 7 | 8, 9


def stream_block_edges():
    """g: entries [g a] [-g b] [g c d] fill block 0 -- the two-other-literal clause ends on entry 3 -- and the unit clause [-g]
    opens block 1.  h: [h o o] (entries 0-1), a 6-literal clause (entries 2-6) and a 40-literal clause (entries 7-45) straddle
    the blocks, a unit clause ends the stream.  The others are 39 variables visited in a shuffled order around g and h."""
    g, h, first = 40, 41, list(range(1, 40))
    clauses = [[g, 1], [-g, -2], [g, 3, -4], [-g],
               [h, 5, -6], [h, -7, 8, 9, -10, 11], [-h] + [v * (1 if v % 3 else -1) for v in first], [h]]
    rng = np.random.RandomState(41)
    # listed: g 4, h 4; others <= 3 (variables 5 .. 11 are in two of h's clauses, 1 .. 4 in one of g's and the long one); the 39
    # others and h share the long clause -- 40 levels of one variable -- and g, whose level is 1 + that of a neighbour, joins one
    return _case("stream_block_edges", 41, clauses, order=rng.permutation(41), planes={1, 2, 3}, groups=40)


def hub_beside_63():
    """One group: the p = 12 hub in lane 0 (4095 entries) beside 63 variables with one entry each."""
    rng = np.random.RandomState(63)
    clauses = hub(1, 2048, 2047) + [[_sign(rng, v)] for v in range(2, 65)]
    return _case("hub_beside_63", 64, clauses, planes={12}, groups=1)


# ----------------------------------------------------------------------------- level geometry
def units(n):
    """n variables with one unit clause each: one level of ceil(n / 64) groups."""
    rng = np.random.RandomState(n)
    return _case(f"units_{n}", n, [[_sign(rng, v + 1)] for v in range(n)], order=rng.permutation(n), planes={1}, groups=-(-n // 64))


def level_of_600():
    """600 unit-clause variables in one level -- 10 groups on 8 waves (group k goes to wave k % 8), so two waves take two groups of
    the level and six take one -- then a last
    variable whose 40 clauses each name a different one of them.  Those 40 list two clauses (2 planes), the last one 40 (6)."""
    rng = np.random.RandomState(600)
    z = 601
    clauses = [[_sign(rng, v + 1)] for v in range(600)] + [[_sign(rng, z), _sign(rng, 15 * j + 1)] for j in range(40)]
    order = np.concatenate([rng.permutation(600), [600]])
    return _case("level_of_600", 601, clauses, order=order, planes={1, 2, 6}, groups=11)


def chain_70_hub():
    """A chain of 70 variables, 70 levels; the last one is also the p = 8 hub: 128 [x], 126 [-x] and the link, which holds -x."""
    rng = np.random.RandomState(70)
    x = 70
    clauses = [[_sign(rng, i + 1), _sign(rng, i + 2)] for i in range(68)] + [[_sign(rng, 69), -x]] + hub(x, 128, 126)
    return _case("chain_70_hub", 70, clauses, planes={1, 2, 8}, groups=70)


# ----------------------------------------------------------------------------- score
SCORE_M = (511, 512, 513, 1025)           # the score loop takes 8 waves x 64 clauses per trip
SCORE_TABLE = {                           # (M, holes): (plane set, groups) of the seeded formula, recorded from the host table
    (511, False): ({6, 7}, 29), (511, True): ({6}, 29), (512, False): ({6}, 29), (512, True): ({5, 6}, 29),
    (513, False): ({6, 7}, 29), (513, True): ({5, 6}, 28), (1025, False): ({7}, 30), (1025, True): ({6, 7}, 30),
}


def _three_sat(rng, nvar, n):
    return [[_sign(rng, v + 1) for v in rng.choice(nvar, 3, replace=False)] for _ in range(n)]


def score(M, holes=False):
    """M random 3-SAT clauses over 30 variables; with `holes`, every fifth clause is empty."""
    rng = np.random.RandomState(M)
    clauses = _three_sat(rng, 30, M)
    if holes:
        clauses = [[] if c % 5 == 4 else cl for c, cl in enumerate(clauses)]
    planes, groups = SCORE_TABLE[M, holes]
    return _case(f"score_{M}{'_holes' if holes else ''}", 30, clauses, order=rng.permutation(30), planes=planes, groups=groups)


def score_weight_limit():
    """A weighted formula whose weights total exactly 2^24 - 1 while no variable lists more than 2^22."""
    rng = np.random.RandomState(24)
    nvar, M = 24, 96
    clauses = [[_sign(rng, v + 1) for v in rng.choice(nvar, int(rng.randint(1, 4)), replace=False)] for _ in range(M)]
    weights = [int(rng.choice([1, (1 << k) - 1, 1 << k])) for k in rng.randint(14, 20, M - 8)]
    rest = (1 << 24) - 1 - sum(weights)                    # the last 8 clauses share what is left to the limit
    weights += [rest // 8] * 7 + [rest - 7 * (rest // 8)]
    listed = listed_weights(nvar, clauses, weights)
    assert sum(weights) == (1 << 24) - 1 and min(weights) >= 1 and max(listed) <= (1 << 22), (weights[-1], max(listed))
    return _case("score_weight_limit", nvar, clauses, weights, order=rng.permutation(nvar), planes={19, 20, 21, 22}, groups=11)   # recorded


# ----------------------------------------------------------------------------- the list
BUILDERS = collections.OrderedDict()
for _p in WIDTHS:
    BUILDERS[f"width_{_p}"] = functools.partial(width, _p)
for _p in TIES:
    BUILDERS[f"tie_{_p}"] = functools.partial(tie, _p)
for _p in COMPANY:
    BUILDERS[f"company_{_p}"] = functools.partial(company, _p)
for _n in WEIGHTED:
    BUILDERS[_n] = functools.partial(weighted_pair, _n)
for _n in RIPPLES:
    BUILDERS[_n] = functools.partial(ripple, _n)
BUILDERS["weighted_three_widths"] = weighted_three_widths
BUILDERS["stream_lengths"] = stream_lengths
BUILDERS["stream_block_edges"] = stream_block_edges
BUILDERS["hub_beside_63"] = hub_beside_63
for _n in (64, 65, 128):
    BUILDERS[f"units_{_n}"] = functools.partial(units, _n)
BUILDERS["level_of_600"] = level_of_600
BUILDERS["chain_70_hub"] = chain_70_hub
for _m in SCORE_M:
    BUILDERS[f"score_{_m}"] = functools.partial(score, _m)
    BUILDERS[f"score_{_m}_holes"] = functools.partial(score, _m, True)
BUILDERS["score_weight_limit"] = score_weight_limit
NAMES = list(BUILDERS)

# the cases whose point is a counter width: they also run from the saturating starts (all variables 0 / all variables 1)
WIDTH_CASES = [n for n in NAMES if n.split("_")[0] in ("width", "tie", "company", "ripple") or n in WEIGHTED] + ["weighted_three_widths"]

# (form, weighted) -> the cases that reach it at the lower and at the upper edge of its plane range.  The unweighted 24-plane form
# is the exception: both of its cases sit at 13 planes, its FIRST -- 14 planes would take 16 383 unit clauses, 24 would take 2^23 --
# so its planes 13 .. 23 never hold a bit here; the weighted 24-plane form runs the same adder's upper planes up to 24.
FORM_EDGES = {
    (3, False): ("units_64", "width_3"), (5, False): ("width_4", "width_5"), (8, False): ("width_6", "width_8"),
    (12, False): ("width_9", "width_12"), (24, False): ("width_13", "tie_12"),
    (8, True): ("weighted_three_widths", "w8"), (14, True): ("w9", "w14"), (24, True): ("w15", "w24_limit"),
}


@functools.lru_cache(maxsize=None)
def get(name) -> Case:
    return BUILDERS[name]()
