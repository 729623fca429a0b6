"""K4's block order (RLS_STEP_ORDER: -1 automatic, 0 forward, 1 xcd-fwd; csrc/rls_step_plan.h) on the write-through MODE 2 form of 1-byte
rows: workgroup b of a one-shot grid works on block step_block(order, b, grid) of runs.  A wrong map shows as two workgroups on one
run or as a run left unwritten, so every case is compared bit for bit with oracle_np.PPOEnvOracle after every step of an 8-step
chain over a 3-slot ring, under every value of the knob and with the knob unset.  Shapes: N = 2000 (runs of 4 rows, 16 envs per
workgroup) with grids of 1, 2, 3, 5, 7, 9, 10 and 17 workgroups, a last workgroup with one wave, full runs and largest degree 64
(k_maxcut_step_lean); B = 33 and N = 3000 with B = 7 (k_maxcut_step: a short last run and its element tail); N = 144 (runs of 8
rows); invalid actions in one lane, a whole wave and a whole workgroup; nodes of degree 64 and 65, an isolated last node, a graph
without edges; slots that start 16 and 112 bytes into a line; the chain captured in a graph and replayed twice.  The oracle's
trajectory is computed once per case and shared by the knob's values; each case takes a fraction of a second."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import ops
from tests.gpu_util import DEV, device_graph
from tests.test_gpu_step_overlap import DONE_EVERY, D64, D65, HUB, edge_graph, forced_actions, spins, trajectory
from tests.test_gpu_step_sideband import bad_values, capped_actions, capped_graph
from tests.test_gpu_step_store import knobs

pytestmark = pytest.mark.gpu

ORDERS = [None, -1, 0, 1]          # None: the knob unset


def order_knob(order):
    return {} if order is None else {"RLS_STEP_ORDER": order}


def slots3(B, n, offsets):
    """3 ring slots; slot i starts offsets[i] bytes into a 128-byte line (None: wherever the allocator puts it)."""
    keep, slots = [], []
    for i in range(3):
        if offsets is None:
            slots.append(torch.empty((B, n), dtype=torch.bool, device=DEV))
            continue
        buf = torch.empty(B * n + 256, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 128 == 0
        v = buf[offsets[i]:offsets[i] + B * n].view(torch.bool).view(B, n)
        assert v.data_ptr() % 128 == offsets[i]
        keep.append(buf)
        slots.append(v)
    return slots, keep


def run_chain(key, graph, n, xs, acts, order, with_cur_done=False, offsets=None):
    """`acts` (8 steps) over a 3-slot ring, everything compared with the oracle after every step."""
    assert len(acts) == 8
    obj0, traj = trajectory(("policy",) + tuple(key), graph, n, xs, acts)
    g = device_graph(graph, n, 0)
    B = xs.shape[0]
    slots, _keep = slots3(B, n, offsets)
    slots[0].copy_(torch.from_numpy(xs).to(DEV).to(torch.bool))
    obj = torch.from_numpy(obj0.astype(np.int32)).to(DEV)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    cur = torch.empty(B, dtype=torch.float32, device=DEV) if with_cur_done else None
    done = torch.empty(B, dtype=torch.float32, device=DEV) if with_cur_done else None
    with knobs(**order_knob(order)):
        for t, a in enumerate(acts):
            dst = slots[(t + 1) % 3]
            dv = 1.0 if (t + 1) % DONE_EVERY == 0 else 0.0
            ops.maxcut_step(g, slots[t % 3], dst, torch.from_numpy(a).to(DEV), obj, reward, cur=cur, done=done, done_value=dv)
            x_ref, r_ref, c_ref, d_ref = traj[t]
            assert np.array_equal(dst.float().cpu().numpy(), x_ref), t
            assert np.array_equal(reward.cpu().numpy(), r_ref, equal_nan=True), t
            assert np.array_equal(obj.cpu().numpy().astype(np.float32), c_ref), t
            if with_cur_done:
                assert np.array_equal(cur.cpu().numpy(), c_ref), t
                assert np.array_equal(done.cpu().numpy(), d_ref), t
    assert np.array_equal(obj.cpu().numpy().astype(np.int64), onp.maxcut_obj(traj[7][0] > 0, graph, False))


def lean_graph(n):
    """Node 0 -- 1..64 (the largest degree, exactly a wave), a ring over 65 .. n - 2, and node n - 1 without an edge (its CSR row starts
    at nnz): every row fits a wave, so full runs without cur / done run k_maxcut_step_lean."""
    e = [(0, v) for v in range(1, 65)] + [(v, v + 1) for v in range(65, n - 2)]
    g = np.asarray([(u, v, 1) for u, v in e], dtype=np.int64)
    deg = np.bincount(g[:, :2].ravel(), minlength=n)
    assert deg.max() == 64 == deg[0] and deg[n - 1] == 0
    return g


# ---------------------------------------------------------------------------------------------------------------- the lean kernel
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B", [4, 28, 36, 68, 112, 132, 4 * 4 * 9 + 4, 272])
def test_lean_kernel_grids(B, order):
    """N = 2000: 1, 2, 3, 5, 7, 9, 10 and 17 workgroups; 28, 36, 68, 132 and 148 envs end in a workgroup with fewer than 4 waves.  The
    actions hold the degree-64 node, the isolated last node, invalid values in single lanes (step 1), in the whole second wave
    (step 2) and in the whole first workgroup (step 3)."""
    n = 2000
    graph = lean_graph(n)
    acts = capped_actions(n, B, 8, 4, seed=B)
    for t, a in enumerate(acts):
        if t != 3:
            a[B - 1] = (n - 1, 0, 64)[t % 3]
    run_chain(("lean", B), graph, n, spins(B, n, 50 + B % 7), acts, order)


@pytest.mark.parametrize("order", ORDERS)
def test_rows_of_144_bytes(order):
    """N = 144: runs of 8 rows, 32 envs per workgroup; 9 workgroups and a last one with a single wave."""
    n, B = 144, 8 * 4 * 9 + 8
    graph = lean_graph(n)
    run_chain(("n144", B), graph, n, spins(B, n, 58), capped_actions(n, B, 8, 8, seed=58), order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B", [36, 132])
def test_graph_without_edges(B, order):
    n = 2000
    graph = np.zeros((0, 3), dtype=np.int64)
    rng = np.random.RandomState(B)
    acts = [rng.randint(0, n, size=B).astype(np.int64) for _ in range(8)]
    acts[2][1::2] = -1
    acts[5][B - 1] = n - 1
    run_chain(("edgeless", B), graph, n, spins(B, n, 59), acts, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B", [36, 132])
def test_slots_16_and_112_bytes_into_a_line(B, order):
    n = 2000
    graph = lean_graph(n)
    run_chain(("misal", B), graph, n, spins(B, n, 60), capped_actions(n, B, 8, 4, seed=60 + B), order, offsets=[16, 112, 16])


# ---------------------------------------------------------------------------------------------------------------- the general kernel
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("with_cur_done", [True, False])
@pytest.mark.parametrize("n,B", [(2000, 33),       # 3 workgroups; the last has one run of a single row
                                 (3000, 7)])       # runs of 2 rows; the last run is one row of 3000 bytes = 187 vectors + 8 bytes
def test_general_kernel_short_last_run(n, B, with_cur_done, order):
    """A hub of degree 130, nodes of degree 64 and 65 and an isolated last node side by side in one wave; step 1 holds invalid actions
    in single lanes, step 3 in the whole first workgroup (or the whole batch where it is smaller)."""
    graph = edge_graph(n, 2 * n)
    acts = forced_actions(n, max(B, 8), 8, seed=n + B)
    acts = [a[:B].copy() for a in acts]
    bad = bad_values(n)
    idx = np.arange(1, B, 3)
    acts[1][idx] = bad[idx % len(bad)]
    wg = min(16, B)
    acts[3][:wg] = bad[np.arange(wg) % len(bad)]
    for t, a in enumerate(acts):
        if t not in (1, 3):
            a[B - 1] = (HUB, n - 1, D64, D65)[t % 4]
    run_chain(("general", n, B), graph, n, spins(B, n, 61), acts, order, with_cur_done=with_cur_done,
              offsets=[16, 112, 16] if with_cur_done else None)


# ---------------------------------------------------------------------------------------------------------------- captured
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("lean", [True, False])
def test_captured_chain_over_three_slots_replayed_twice(lean, order):
    """8 steps over the 3-slot ring in one captured graph.  The chain ends in slot 2; it is copied to slot 0 and the graph replayed: 16
    steps of the oracle.  lean: 132 envs, full runs, no cur; else 33 envs, a hub, a short last run and cur."""
    n, B = 2000, 132 if lean else 33
    graph = lean_graph(n) if lean else edge_graph(n, 2 * n)
    acts8 = capped_actions(n, B, 8, 4, seed=62) if lean else forced_actions(n, B, 8, seed=62)
    xs = spins(B, n, 62)
    obj0, traj = trajectory(("policy", "graph", B), graph, n, xs, acts8 + acts8)
    g = device_graph(graph, n, 0)
    slots, _keep = slots3(B, n, None)
    slots[0].copy_(torch.from_numpy(xs).to(DEV).to(torch.bool))
    obj = torch.from_numpy(obj0.astype(np.int32)).to(DEV)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    cur = None if lean else torch.empty(B, dtype=torch.float32, device=DEV)
    acts_dev = [torch.from_numpy(a).to(DEV) for a in acts8]
    with knobs(**order_knob(order)):
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
