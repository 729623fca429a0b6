"""Differential fuzz of the MCPG metro walk (rls_mcpg_metro_rounds, every kernel form) against tests/metro_oracle.py, bit for bit:
N from every band of the launcher (small, around 6144 / 10240 / 13652 / 16384 / 20480), node-major f32 / uint8 or bit-packed with
the draw windows in LDS or in scratch, 1..200 rounds, a round offset, a device-side round limit (below 0 and past T included),
1..7 accept rows, ragged chain counts up to 130, a broadcast start state, recorded draws (half of them metro_oracle.pattern_draws:
the node revisits the packed walker's look-ahead has to repair) or the production hash with 64-bit seeds and chain ids.  Each
configuration checks the state, the accept counts row by row and, for a dry pass, that the state is untouched.
`python tools/fuzz/fuzz_metro.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from tests import metro_oracle as mo
from rlsolver_amd import _abi
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.ops_mcpg_tsp import PackedChains

DEV = torch.device("cuda:0")
LDS = 160 * 1024
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def to_form(form, x):
    if form == "f32":
        return dev(x.astype(np.float32))
    if form == "u8":
        return dev(x.astype(np.uint8))
    return PackedChains(dev(mo.pack(x)), x.shape[1])


def read(form, obj):
    return obj.words.cpu().numpy().view(np.uint64) if form.startswith("packed") else obj.cpu().numpy() != 0


BANDS = [(1, 12), (12, 400), (6100, 6200), (10200, 10280), (13600, 13700), (16350, 16420), (20440, 20481)]
t_end = time.time() + budget
it = 0
while time.time() < t_end:
    lo, hi = BANDS[rng.randint(len(BANDS))]
    N = int(rng.randint(lo, hi))
    form = str(rng.choice(["f32", "u8", "packed_lds", "packed_scratch"]))
    C = int(rng.choice([1, 63, 64, 65, 128, rng.randint(1, 131)]))
    T = int(rng.choice([rng.randint(1, 201), rng.choice([1, 8, 63, 64, 65, 128, 129])]))
    t_offset = int(rng.choice([0, 0, 64, rng.randint(0, 200)]))
    rows = int(rng.randint(1, 8))
    with_acc = rng.rand() < 0.7
    # the form this N can take: the launcher's own limits (include/rlsolver_hip.h), so that nothing here is refused
    need = int(_abi.lib().rls_mcpg_metro_scratch_bytes(N, C))
    if form == "packed_scratch" and need == 0:
        form = "packed_lds"
    if form == "packed_lds" and ((N + 1) & ~1) * 8 + 32768 > LDS:
        form = "packed_scratch"
    if form in ("f32", "u8"):
        room = LDS - 8 * N - 16
        if room < 0:
            form = "packed_scratch"
        elif with_acc and room < 4 * T:
            if room >= 4:
                T = int(rng.randint(1, room // 4 + 1))
            else:
                with_acc = False
    packed = form.startswith("packed")
    bcast = packed and C % 64 == 0 and C > 64 and rng.rand() < 0.5
    c_in = 64 if bcast else C
    dry = with_acc and not bcast and rng.rand() < 0.3
    in_place = dry or (not bcast and rng.rand() < 0.5)
    tl = None if rng.rand() < 0.3 else int(rng.choice([-3, 0, 1, T - 1, T, T + 5, rng.randint(0, T + 1)]))
    given = rng.rand() < 0.5
    seed = [0, 77, 2 ** 32 + 5, 2 ** 63 + 1, int(rng.randint(1 << 30))][rng.randint(5)]
    chain_ids = None
    if not given and rng.rand() < 0.5:
        chain_ids = (int(rng.choice([3, 2 ** 32 + 64])), 64, int(64 * rng.randint(1, 5))) if C % 64 == 0 and rng.rand() < 0.5 \
            else (int(rng.choice([3, 2 ** 32 + 64])), 0, 0)
    tag = (f"it={it} N={N} form={form} C={C} C_in={c_in} T={T} t_offset={t_offset} rows={rows if with_acc else None} t_limit={tl} "
           f"dry={dry} in_place={in_place} draws={'recorded' if given else 'hash'} seed={seed} chain_ids={chain_ids}")
    if "-v" in sys.argv:
        print(tag, flush=True)
    probs = (rng.rand(N) * 0.6 + 0.2).astype(np.float32)
    start = rng.randint(0, 2, size=(N, c_in)).astype(bool)
    if given:
        if rng.rand() < 0.5:                                           # node revisits, on a few nodes at both ends of the state
            n = int(min(N, rng.randint(1, 11)))
            index, u, _ = mo.pattern_draws(n, t_offset + T, C, int(rng.randint(1 << 30)))
            index = np.where(index < (n + 1) // 2, index, N - n + index)
        else:
            index, u = rng.randint(0, N, size=(t_offset + T, C)).astype(np.int64), rng.rand(t_offset + T, C).astype(np.float32)
        ix, uu = index[t_offset:], u[t_offset:]
        d_index, d_u = dev(index), dev(u)
    else:
        ix, uu = mo.production_draws(seed, mo.global_ids(C, chain_ids), t_offset, T, N)
        d_index = d_u = None
    x0 = start[:, np.arange(C) % c_in]
    rounds = T if tl is None else min(T, max(tl, 0))
    wk = mo.Walker(x0, probs)
    acc = np.zeros((T, C), np.int64)
    for t in range(rounds):
        acc[t] = wk.step(ix[t], uu[t])
    tiles = (C + 63) // 64
    pad = np.zeros((T, tiles * 64), np.int64)
    pad[:, :C] = acc
    per_tile = pad.reshape(T, tiles, 64).sum(axis=2)
    want_acc = np.zeros((rows, T), np.int64)
    for k in range(tiles):
        want_acc[k % rows] += per_tile[:, k]
    fill = rng.randint(0, 1000, size=(rows, T)).astype(np.int64)
    d_acc = dev(fill) if with_acc else None
    d_start = to_form(form, start)
    out = d_start if in_place else to_form(form, ~x0)
    d_tl = None if tl is None else torch.tensor([tl], dtype=torch.int64, device=DEV)
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV) if packed and need > 0 else None
    if form == "packed_lds":
        _abi.tuning_set("RLS_METRO_QG", 0)
    try:
        mops.mcpg_metro_rounds(out, dev(probs), T, d_index, d_u, seed, d_tl, not dry, d_acc, t_offset=t_offset,
                               samples_in=None if in_place else d_start, chain_ids=chain_ids, scratch=scratch)
    finally:
        _abi.tuning_unset("RLS_METRO_QG")
    final = mo.pack(x0) if dry and packed else x0 if dry else wk.words if packed else wk.x
    assert np.array_equal(read(form, out), final), "state " + tag
    if not in_place:
        assert np.array_equal(read(form, d_start), mo.pack(start) if packed else start), "start state " + tag
    if with_acc:
        assert np.array_equal(d_acc.cpu().numpy() - fill, want_acc), "accept counts " + tag
    it += 1
print(f"fuzz_metro: {it} random configurations, no mismatch")
