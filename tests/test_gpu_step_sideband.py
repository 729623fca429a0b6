"""K4's headline form (MODE 2, 1-byte rows, write-through stores) where its per-env outputs and its trip after landing can go wrong.
The wave reads all 2 x EPW bytes of the gain from its LDS stage before one wait -- none under a branch, so an invalid action, an env
past a short run's end and a lane past a CSR row's end read too and must change nothing -- and flips the action's byte with one LDS
write of the byte it has read.  A call with full runs, no cur / done and max_degree <= 64 runs k_maxcut_step_lean, every other call
k_maxcut_step: both are driven (B a multiple of EPW or not, cur / done NULL or given, largest degree 64 or more).  Cases: workgroups
whose last wave(s) have no run or a short one, every EPW the launcher picks with a partial last workgroup, invalid actions mixed into a workgroup, filling a wave and filling a whole workgroup, degrees 64 / 65 / a hub /
an isolated last node / no edges, cur and done given or NULL, slots that start anywhere in a line, the persistent grid, plain and
write-through stores, a captured chain over a 3-slot ring, a 50-step chain.  Everything against oracle_np.PPOEnvOracle bit for bit
after every step (the helpers of test_gpu_step_overlap.py); each case takes a fraction of a second."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import ops
from tests.gpu_util import DEV, device_graph
from tests.test_gpu_step_overlap import (D64, D65, HUB, edge_graph, forced_actions, run_ring, slot_views, spins, trajectory)
from tests.test_gpu_step_store import knobs

pytestmark = pytest.mark.gpu

BAD = np.array([-1, 0, (1 << 31) + 5, (1 << 32) + 1, -(1 << 40)], dtype=np.int64)     # entry 1 is replaced by n


def bad_values(n):
    v = BAD.copy()
    v[1] = n
    return v


def capped_graph(n, maxdeg):
    """Node 0 -- 1..maxdeg and a ring over the other nodes: the largest degree is exactly `maxdeg` (node 0's)."""
    e = [(0, v) for v in range(1, maxdeg + 1)] + [(v, v + 1) for v in range(maxdeg + 1, n - 1)]
    g = np.asarray([(u, v, 1) for u, v in e], dtype=np.int64)
    deg = np.bincount(g[:, :2].ravel(), minlength=n)
    assert deg.max() == maxdeg == deg[0]
    return g


# ---------------------------------------------------------------------------------------------------------------- workgroup edges
@pytest.mark.parametrize("with_cur_done", [True, False])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 15, 16, 17, 31, 33])
def test_workgroup_edges(B, with_cur_done):
    """N = 2000: runs of 4 rows, 4 waves = 16 envs per workgroup.  One to four waves present in the last workgroup, a short last run."""
    n = 2000
    graph = edge_graph(n, 3 * n)
    acts = forced_actions(n, max(B, 8), 6, seed=B + 1)
    acts = [a[:B].copy() for a in acts]
    for t, a in enumerate(acts):
        a[B - 1] = (HUB, n - 1, D64, D65, n - 2, 7)[t]
    run_ring(("sb-edge", B), graph, n, spins(B, n, 21), acts, "u8", {}, with_cur_done=with_cur_done)


@pytest.mark.parametrize("with_cur_done", [True, False])
@pytest.mark.parametrize("n,B", [(1024, 75),      # EPW 8: 32 envs per workgroup; the last has runs of 8 and 3
                                 (2000, 37),      # EPW 4: 16 envs per workgroup; the last has runs of 4 and 1
                                 (4000, 19),      # EPW 2: 8 envs per workgroup; the last has runs of 2 and 1
                                 (8000, 7),       # EPW 1: 4 envs per workgroup; the last has 3 waves
                                 (3000, 5)])      # EPW 2; the last run is one row of 3000 bytes = 187 vectors + 8 bytes
def test_every_epw_with_a_partial_last_workgroup(n, B, with_cur_done):
    graph = edge_graph(n, 2 * n)
    acts = forced_actions(n, max(B, 8), 6, seed=n + B)
    acts = [a[:B].copy() for a in acts]
    for t, a in enumerate(acts):                    # the last env picks the special nodes and the row's last bytes
        a[B - 1] = (n - 1, HUB, n - 2, D65, D64, n - 1)[t]
    run_ring(("sb-epw", n, B), graph, n, spins(B, n, 22), acts, "u8", {}, with_cur_done=with_cur_done)


# ---------------------------------------------------------------------------------------------------------------- invalid actions
@pytest.mark.parametrize("n,B", [(2000, 33), (1024, 75), (8000, 7)])
def test_invalid_actions_in_a_workgroup(n, B):
    """Step 1: -1, n and values past 2^31 beside valid actions in every wave.  Step 2: one wave with nothing valid beside valid waves.
    Step 3: the whole first workgroup invalid (reward NaN, obj and state as they were), the rest valid.  Step 4: every env invalid."""
    graph = edge_graph(n, 2 * n)
    acts = forced_actions(n, max(B, 8), 6, seed=n + 5)
    acts = [a[:B].copy() for a in acts]
    bad = bad_values(n)
    epw = {2000: 4, 1024: 8, 8000: 1}[n]
    idx = np.arange(1, B, 3)
    acts[1][idx] = bad[idx % len(bad)]
    acts[2][epw:min(2 * epw, B)] = bad[np.arange(min(2 * epw, B) - epw) % len(bad)]
    wg = min(4 * epw, B)
    acts[3][:wg] = bad[np.arange(wg) % len(bad)]
    acts[4][:] = bad[np.arange(B) % len(bad)]
    _, traj = trajectory(("sb-bad", n, B), graph, n, spins(B, n, 23), acts)
    assert np.isnan(traj[3][1][:wg]).all() and np.isnan(traj[4][1]).all()
    assert np.array_equal(traj[4][0], traj[3][0])                                   # nothing moved in the all-invalid step
    run_ring(("sb-bad", n, B), graph, n, spins(B, n, 23), acts, "u8", {})


# ---------------------------------------------------------------------------------------------------------------- graphs
@pytest.mark.parametrize("with_cur_done", [True, False])
@pytest.mark.parametrize("maxdeg", [64, 65])
def test_max_degree_64_and_65(maxdeg, with_cur_done):
    """A graph whose largest degree is exactly 64 (every gain is one ballot) and one where it is 65 (node 0 takes the loop)."""
    n, B = 2000, 32
    graph = capped_graph(n, maxdeg)
    rng = np.random.RandomState(maxdeg)
    acts = [rng.randint(0, n, size=B).astype(np.int64) for _ in range(6)]
    for t, a in enumerate(acts):
        a[t % B] = 0
        a[(t + 4) % B] = 0
        a[B - 1] = (0, n - 1, 1, maxdeg, maxdeg + 1, 0)[t]
    run_ring(("sb-cap", maxdeg), graph, n, spins(B, n, 24), acts, "u8", {}, with_cur_done=with_cur_done)


@pytest.mark.parametrize("with_cur_done", [True, False])
@pytest.mark.parametrize("n,B", [(2000, 24), (2000, 21), (8000, 8)])
def test_edgeless_graph(n, B, with_cur_done):
    graph = np.zeros((0, 3), dtype=np.int64)
    rng = np.random.RandomState(B)
    acts = [rng.randint(0, n, size=B).astype(np.int64) for _ in range(5)]
    acts[2][1::2] = -1
    run_ring(("sb-edgeless", n, B), graph, n, spins(B, n, 25), acts, "u8", {}, with_cur_done=with_cur_done)


# ---------------------------------------------------------------------------------------------------------------- the lean kernel
def capped_actions(n, B, steps, epw, seed):
    """Random actions on capped_graph(n, 64) with node 0 (degree 64), its last neighbour, a ring node and the last node in every step;
    step 1: invalid values in every wave; step 2: the second wave all invalid; step 3: the first workgroup all invalid."""
    rng = np.random.RandomState(seed)
    bad = bad_values(n)
    acts = []
    for t in range(steps):
        a = rng.randint(0, n, size=B).astype(np.int64)
        a[t % B], a[(t + 1) % B], a[(t + 2) % B], a[B - 1] = 0, 64, 65 + t, (n - 1, 0, n - 2)[t % 3]
        if t == 1:
            idx = np.arange(1, B, 3)
            a[idx] = bad[idx % len(bad)]
        if t == 2:
            a[epw:2 * epw] = bad[np.arange(len(a[epw:2 * epw])) % len(bad)]
        if t == 3:
            wg = min(4 * epw, B)
            a[:wg] = bad[np.arange(wg) % len(bad)]
        acts.append(a)
    return acts


@pytest.mark.parametrize("offsets", [None, [16, 16, 48, 112, 112, 48, 16, 112]])
@pytest.mark.parametrize("n,B,epw", [(1024, 72, 8), (2000, 36, 4), (4000, 18, 2), (8000, 7, 1), (2000, 4, 4), (2000, 16, 4)])
def test_lean_kernel_every_epw(n, B, epw, offsets):
    """Full runs, cur = done = NULL, largest degree 64: k_maxcut_step_lean, each EPW with a last workgroup of one wave (or a single
    wave, or exactly one workgroup), invalid actions included, slots aligned or anywhere in a line."""
    graph = capped_graph(n, 64)
    acts = capped_actions(n, B, 6, epw, seed=n + B)
    run_ring(("sb-lean", n, B), graph, n, spins(B, n, 30), acts, "u8", {}, with_cur_done=False, offsets=offsets)


# ---------------------------------------------------------------------------------------------------------------- slots and knobs
@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("n,B", [(2000, 17), (1024, 35)])
def test_misaligned_slots_plain_and_write_through(n, B, wt):
    """Slots starting 16, 48 and 112 bytes into a line; RLS_STEP_WT = 0 runs the plain-store body, 1 the headline's."""
    graph = edge_graph(n, 2 * n)
    acts = forced_actions(n, B, 8, seed=n + 6)
    run_ring(("sb-misal", n, B), graph, n, spins(B, n, 26), acts, "u8", {"RLS_STEP_WT": wt}, offsets=[16, 16, 48, 112, 112, 48, 16, 112])


@pytest.mark.parametrize("persist", [0, 1])
def test_persistent_grid_and_one_shot(persist):
    """RLS_STEP_PERSIST = 1 with one wave per workgroup: every wave makes three trips and some a fourth, short one, refilling the stage
    whose flipped byte and gather reads the last trip left; 0: the one-shot grid on the same batch."""
    n = 144
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    B = 8 * 3 * (8 * cus) + 5
    graph = edge_graph(n, 2 * n)
    acts = forced_actions(n, B, 5, seed=12)
    acts[3][40:48] = -1
    run_ring(("sb-persist", B), graph, n, spins(B, n, 27), acts, "u8", {"RLS_STEP_PERSIST": persist, "RLS_STEP_WPB": 1, "RLS_STEP_WT": 1})


# ---------------------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("lean", [False, True])
def test_captured_chain_over_three_slots_replayed_twice(lean):
    """8 steps over a 3-slot ring in one captured graph.  The chain ends in slot 2; it is copied to slot 0 and the graph replayed: 16
    steps of the oracle.  lean: full runs, no cur, largest degree 64 (k_maxcut_step_lean); else a hub, a short last run and cur."""
    n, B = 2000, 36 if lean else 37
    graph = capped_graph(n, 64) if lean else edge_graph(n, 2 * n)
    acts8 = capped_actions(n, B, 8, 4, seed=31) if lean else forced_actions(n, B, 8, seed=31)
    xs = spins(B, n, 28)
    obj0, traj = trajectory(("sb-graph", B), graph, n, xs, acts8 + acts8)
    g = device_graph(graph, n, 0)
    slots = [torch.empty((B, n), dtype=torch.bool, device=DEV) for _ in range(3)]
    slots[0].copy_(torch.from_numpy(xs).to(DEV).to(torch.bool))
    obj = torch.from_numpy(obj0.astype(np.int32)).to(DEV)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    cur = None if lean else torch.empty(B, dtype=torch.float32, device=DEV)
    acts_dev = [torch.from_numpy(a).to(DEV) for a in acts8]
    ops.maxcut_step(g, slots[0], slots[1], acts_dev[0], obj.clone(), reward, cur=cur)   # (loads the kernel before the capture)
    launchers = [ops.maxcut_step_launcher(g, slots[t % 3], slots[(t + 1) % 3], acts_dev[t], obj, reward, cur=cur) for t in range(8)]
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for launch in launchers:
            launch()
    for rep in range(2):
        gr.replay()
        torch.cuda.synchronize()
        x_ref, r_ref, c_ref, _ = traj[8 * rep + 7]
        assert np.array_equal(slots[8 % 3].float().cpu().numpy(), x_ref), rep
        assert np.array_equal(reward.cpu().numpy(), r_ref, equal_nan=True), rep
        assert lean or np.array_equal(cur.cpu().numpy(), c_ref), rep
        assert np.array_equal(obj.cpu().numpy().astype(np.float32), c_ref), rep
        slots[0].copy_(slots[8 % 3])
    assert torch.equal(ops.maxcut_obj(g, slots[0]), obj.long())


@pytest.mark.parametrize("lean", [False, True])
def test_fifty_step_chain_keeps_obj_equal_to_the_cut(lean):
    n, B = 2000, 64
    graph = capped_graph(n, 64) if lean else edge_graph(n, 3 * n)
    acts = capped_actions(n, B, 50, 4, seed=41) if lean else forced_actions(n, B, 50, seed=41)
    g, x, obj = run_ring(("sb-50", B, lean), graph, n, spins(B, n, 29), acts, "u8", {}, with_cur_done=False)
    assert torch.equal(ops.maxcut_obj(g, x), obj.long())
