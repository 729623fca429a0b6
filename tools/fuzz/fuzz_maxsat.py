"""Fuzz of the MaxSAT sampler kernel (rls_maxsat_local_search on the schedule of rls_maxsat_visit_levels) against the numpy
oracle of tests/maxsat_oracle.py with recorded draws: random formulas (uniform k-SAT with k in 1..5, hubs, chains, clauses with
duplicate literals, tautologies, empty and unit clauses, variables in no clause), unweighted or with weights 1 / 3 / top,
saturation hubs (K unit clauses [x] against K - 1 or K of [-x], K a power of two up to 2048: the counters full, with or without a
second literal), weights from {1, 2^k - 1, 2^k} with k up to 22 under the total of 2^24 - 1, up to 700 variables; random visiting
orders, ragged and full tiles, a broadcast start (C_in < C), packed or float32 output, num_ls in 0..3.  Chains after the sweep
and ``expected`` must match bit for bit; draws inside the band where the reference's float32 rule and the coin differ
("MaxSAT") are moved out of it first -- from a listed weight of 2^13 on, where that band is wider than the move
covers, the draws are two-valued (0.25 | 0.75; no variable lists more than 2^22) -- and the agreement of the two rules is asserted
on the oracle's side.
`python tools/fuzz/fuzz_maxsat.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from tests import maxsat_oracle as orc
from rlsolver_amd.methods import MCPG_maxsat as ms
from rlsolver_amd.ops_mcpg_tsp import PackedChains

DEV = torch.device("cuda:0")
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
it = 0
while time.time() < t_end:
    kind = rng.choice(["ksat", "hub", "chain", "odd", "saturate", "pow2", "wide"])
    nvar = int(rng.choice([1, 2, rng.randint(3, 40), rng.randint(40, 130)])) if kind != "wide" else int(rng.randint(130, 701))
    lit = lambda v: int(v + 1) * (1 if rng.rand() < 0.5 else -1)      # noqa: E731
    clauses = []
    if kind == "ksat":
        for _ in range(int(rng.randint(0, 5 * nvar + 1))):
            clauses.append([lit(v) for v in rng.randint(0, nvar, int(rng.randint(1, 6)))])          # (repeats of a variable allowed)
    elif kind == "hub":
        hub = int(rng.randint(0, nvar))
        for _ in range(int(rng.choice([40, 300, 700]))):
            clauses.append([lit(hub)] + [lit(v) for v in rng.randint(0, nvar, int(rng.randint(0, 3)))])
    elif kind == "chain":
        clauses = [[lit(i), lit(i + 1)] for i in range(nvar - 1)]
    elif kind == "saturate":
        hub, K = int(rng.randint(0, nvar)), 1 << int(rng.randint(1, 12))
        tail = [[], [lit(rng.randint(0, nvar))]][int(rng.randint(0, 2))]             # every hub clause bare, or with one fixed second literal
        clauses = [[hub + 1] + tail] * K + [[-(hub + 1)] + tail] * (K - int(rng.randint(0, 2)))
        clauses += [[lit(v) for v in rng.randint(0, nvar, int(rng.randint(1, 4)))] for _ in range(int(rng.randint(0, nvar + 1)))]
    elif kind in ("pow2", "wide"):
        for _ in range(int(rng.randint(1, 3 * nvar + 2))):
            clauses.append([lit(v) for v in rng.randint(0, nvar, int(rng.randint(1, 4)))])
    else:
        for _ in range(int(rng.randint(1, 3 * nvar + 2))):
            v = int(rng.randint(0, nvar))
            clauses.append([[], [v + 1], [v + 1, v + 1], [v + 1, -(v + 1)], [v + 1, -(v + 1), lit(rng.randint(0, nvar))],
                            [lit(u) for u in rng.randint(0, nvar, 12)]][int(rng.randint(0, 6))])
    weighted = bool(rng.rand() < 0.35) and kind != "saturate" or kind == "pow2"
    top = int(rng.choice([5, 20, 200]))
    weights = [int(rng.choice([1, 3, top])) for _ in clauses] if weighted else None
    if kind == "pow2":
        # {1, 2^k - 1, 2^k}, each cut to what the total (2^24 - 1, one unit kept for every later clause) and the 2^22 a variable may
        # list still allow
        top, left, listed = 1 << 24, (1 << 24) - 1 - len(clauses), [0] * nvar
        for c, cl in enumerate(clauses):
            k = int(rng.randint(1, 23))
            room = min([left + 1] + [((1 << 22) - listed[abs(l) - 1]) // sum(1 for m in cl if abs(m) == abs(l)) for l in cl])
            weights[c] = max(1, min(int(rng.choice([1, (1 << k) - 1, 1 << k])), room))
            left -= weights[c] - 1
            for l in cl:
                listed[abs(l) - 1] += weights[c]
        if max(listed) > (1 << 22):                                                   # (too many clauses on one variable for any weights)
            continue
    order = rng.permutation(nvar)
    data = ms.make_data(nvar, clauses, weights, top if weighted else None, len(clauses) + int(rng.randint(0, 3)), DEV, sorted_nodes=order)
    inst = orc.Instance(nvar, clauses, weights, top if weighted else None, data.pdata[1])
    C = int(rng.choice([1, 63, 64, 65, 128, 200]))
    c_in = 64 if (C == 128 and rng.rand() < 0.5) else C
    num_ls = int(rng.randint(0, 4))
    packed_out = bool(rng.rand() < 0.5)
    tag = f"it={it} kind={kind} nvar={nvar} M={len(clauses)} weighted={weighted} C={C} C_in={c_in} num_ls={num_ls} packed_out={packed_out}"
    if "-v" in sys.argv:
        print(tag, flush=True)
    start = (rng.rand(nvar, c_in) < 0.5).astype(np.float32)
    full = np.tile(start, (1, C // c_in))
    uni = rng.rand(max(num_ls, 1), nvar, C).astype(np.float32)[:num_ls]
    heavy = max(np.bincount(inst.vi, weights=np.abs(inst.neg), minlength=nvar)) >= (1 << 13)      # the largest listed weight
    uni = np.where(uni < 0.5, np.float32(0.25), np.float32(0.75)) if heavy else orc.prepare_uniforms(uni)
    s = (full.T * 2 - 1).astype(np.float32)
    assert orc.coin_rule_agrees(inst, s, order, num_ls, uni), "coin rule " + tag
    orc.sweep(inst, s, order, num_ls, uni)
    coins = ms.maxsat_tie_coins_from_uniforms(torch.from_numpy(uni).to(DEV)) if num_ls else None
    xin = PackedChains.pack(torch.from_numpy(start).to(DEV))
    out = PackedChains.empty(nvar, C, DEV) if packed_out else None
    xs, expected = data.local_search(xin, num_ls, coins=coins, out=out, num_chains=C)
    got = (xs.unpack() if packed_out else xs).cpu().numpy()
    assert np.array_equal(got, (s.T + 1) / 2), "chains " + tag
    assert np.array_equal(expected.cpu().numpy(), -orc.score(inst, s)), "expected " + tag
    it += 1
print(f"fuzz_maxsat: {it} random configurations, no mismatch")
