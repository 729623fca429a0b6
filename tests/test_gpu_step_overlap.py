"""K4's staged forms at the edges where the order of their memory operations matters.  MODE 2 on 1-byte rows with write-through
stores requests every operand of the gain (obj, the CSR row bounds, the neighbour ids) beside the run instead of after it; the other
staged forms (MODE 3, plain / nontemporal stores, f32 rows) run through the same cases.  No form may differ from the oracle by a bit:
at the degree limits of the one-instruction gather (64 / 65 neighbours, a hub, an isolated last node whose row starts at nnz), on a
graph without edges, for out-of-range actions, on short last runs and ragged grids, in the persistent loop (where a trip's LDS-DMA
follows the last trip's reads of the same stage), on runs that start anywhere in a cache line, and inside a captured graph.  Every
case chains 6 - 10 steps over an 8-slot ring (the captured chain: 8 steps replayed twice) and compares next state, reward, obj and cur
with oracle_np.PPOEnvOracle after every step; graphs are explicit edge lists."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import ops
from tests.gpu_util import DEV, device_graph
from tests.test_gpu_step_store import FORMS, knobs

pytestmark = pytest.mark.gpu

HUB, D64, D65 = 0, 131, 132      # degrees 130, 64, 65; node n - 1 is isolated
DONE_EVERY = 3


def edge_graph(n, extra):
    """Hub 0 -- 1..130; node 131 -- 1..64 (degree 64); node 132 -- 1..65 (degree 65); `extra` distinct random edges among the nodes
    133 .. n - 2 (none touches a special node); node n - 1 has no edge, so rowptr[n - 1] == nnz."""
    assert n >= 144
    e = [(HUB, v) for v in range(1, 131)] + [(D64, v) for v in range(1, 65)] + [(D65, v) for v in range(1, 66)]
    rng = np.random.RandomState(n)
    extra = min(extra, (n - 134) * (n - 135) // 4)      # at most half of the pairs there are
    seen = set()
    while len(seen) < extra:
        u, v = (int(t) for t in rng.randint(133, n - 1, size=2))
        if u != v:
            seen.add((min(u, v), max(u, v)))
    e += sorted(seen)
    g = np.asarray([(u, v, 1) for u, v in e], dtype=np.int64).reshape(-1, 3)
    deg = np.bincount(g[:, :2].ravel(), minlength=n)
    assert deg[HUB] == 130 and deg[D64] == 64 and deg[D65] == 65 and deg[n - 1] == 0
    return g


def forced_actions(n, B, steps, seed, group=8):
    """Random actions with, in every step, envs that pick the hub, the degree-64 node, the degree-65 node and the isolated last node
    side by side (one wave holds them all) and scattered over the batch; in step 2, whole waves whose envs all pick one node."""
    rng = np.random.RandomState(seed)
    special = np.array([HUB, D64, D65, n - 1])
    acts = []
    for t in range(steps):
        a = rng.randint(0, n, size=B)
        a[:4] = np.roll(special, t)
        idx = np.arange(5, B, 7)
        a[idx] = special[(idx + t) % 4]
        if t == 2:
            for w, node in enumerate((HUB, 77, n - 1, D65)):
                a[(w + 1) * group:(w + 2) * group] = node
        acts.append(a.astype(np.int64))
    return acts


_TRAJ = {}


def trajectory(key, graph, n, xs, acts):
    """The oracle's (state, reward, cur, done) after every step, computed once per key.  An action outside [0, n) leaves its env and
    its obj as they were and reports NaN."""
    if key not in _TRAJ:
        env = onp.PPOEnvOracle(graph, n, DONE_EVERY, False)
        env.reset_to(xs)
        obj0 = env.last.copy()
        out = []
        for a in acts:
            bad = (a < 0) | (a >= n)
            xs_before, last_before = env.xs.copy(), env.last.copy()
            _, r, d, c = env.step(np.where(bad, 0, a))
            r, c = r.copy(), c.copy()
            if bad.any():
                env.xs[bad] = xs_before[bad]
                env.last[bad] = last_before[bad]
                r[bad] = np.nan
                c[bad] = last_before[bad]
            out.append((env.xs.copy(), r, c, d.copy()))
        _TRAJ[key] = (obj0, out)
    return _TRAJ[key]


def slot_views(B, n, tdt, offsets):
    """8 ring slots; slot i starts offsets[i % len] bytes into a 128-byte line (None: wherever the allocator puts it)."""
    sb = 4 if tdt == torch.float32 else 1
    keep, slots = [], []
    for i in range(8):
        if offsets is None:
            slots.append(torch.empty((B, n), dtype=tdt, device=DEV))
            continue
        off = offsets[i % len(offsets)]
        buf = torch.empty(B * n * sb + 256, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 128 == 0
        v = buf[off:off + B * n * sb].view(tdt).view(B, n)
        assert v.data_ptr() % 128 == off
        keep.append(buf)
        slots.append(v)
    return slots, keep


def run_ring(key, graph, n, xs, acts, dt, extra, with_cur_done=True, offsets=None):
    obj0, traj = trajectory(key, graph, n, xs, acts)
    g = device_graph(graph, n, 0)
    B = xs.shape[0]
    tdt = torch.bool if dt == "u8" else torch.float32
    slots, _keep = slot_views(B, n, tdt, offsets)
    slots[0].copy_(torch.from_numpy(xs).to(DEV).to(tdt))
    obj = torch.from_numpy(obj0.astype(np.int32)).to(DEV)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    cur = torch.empty(B, dtype=torch.float32, device=DEV) if with_cur_done else None
    done = torch.empty(B, dtype=torch.float32, device=DEV) if with_cur_done else None
    with knobs(**extra):
        for t, a in enumerate(acts):
            dst = slots[(t + 1) % 8]
            dv = 1.0 if (t + 1) % DONE_EVERY == 0 else 0.0
            ops.maxcut_step(g, slots[t % 8], dst, torch.from_numpy(a).to(DEV), obj, reward, cur=cur, done=done, done_value=dv)
            x_ref, r_ref, c_ref, d_ref = traj[t]
            assert np.array_equal(dst.float().cpu().numpy(), x_ref), t
            assert np.array_equal(reward.cpu().numpy(), r_ref, equal_nan=True), t
            assert np.array_equal(obj.cpu().numpy().astype(np.float32), c_ref), t
            if with_cur_done:
                assert np.array_equal(cur.cpu().numpy(), c_ref), t
                assert np.array_equal(done.cpu().numpy(), d_ref), t
    final = traj[len(acts) - 1][0]
    assert np.array_equal(obj.cpu().numpy().astype(np.int64), onp.maxcut_obj(final > 0, graph, False))
    return g, dst, obj


def spins(B, n, seed):
    return np.random.RandomState(seed).randint(0, 2, size=(B, n)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- degree edges
@pytest.mark.parametrize("n,dt,B,chase", [(144, "u8", 203, -1),      # runs of 8 rows
                                          (2000, "u8", 203, -1),     # runs of 4 rows (the headline's form)
                                          (144, "f32", 203, -1),     # the chase form (MODE 3) by the launcher's rule
                                          (144, "u8", 203, 1),       # the chase form on 1-byte rows
                                          (144, "f32", 203, 0)])     # MODE 2 on f32 rows
def test_degree_edges(n, dt, B, chase):
    graph = edge_graph(n, 3 * n)
    group = 8 if n == 144 else 4
    acts = forced_actions(n, B, 8, seed=n + 1, group=group)
    extra = {} if chase < 0 else {"RLS_STEP_CHASE": chase}
    run_ring(("deg", n, B), graph, n, spins(B, n, 3), acts, dt, extra)


# ---------------------------------------------------------------------------------------------------------------- no edges at all
@pytest.mark.parametrize("dt,chase", [("u8", 0), ("u8", 1), ("f32", 1)])
def test_edgeless_graph(dt, chase):
    """nnz == 0 (col may be NULL): every action is valid, every reward 0, the state flipped."""
    n, B = 144, 67
    graph = np.zeros((0, 3), dtype=np.int64)
    rng = np.random.RandomState(9)
    acts = [rng.randint(0, n, size=B).astype(np.int64) for _ in range(6)]
    _, traj = trajectory(("edgeless", B), graph, n, spins(B, n, 4), acts)
    assert all(not r.any() for _, r, _, _ in traj)
    run_ring(("edgeless", B), graph, n, spins(B, n, 4), acts, dt, {"RLS_STEP_CHASE": chase})


# ---------------------------------------------------------------------------------------------------------------- invalid actions
@pytest.mark.parametrize("n,dt,chase", [(2000, "u8", 0), (144, "u8", 0), (144, "f32", 1)])
def test_out_of_range_actions(n, dt, chase):
    """-1, n, values past 2^31 (one of them a valid node once truncated to 32 bits) mixed into waves with valid actions, and one whole
    wave (8 envs at n = 144, 4 at n = 2000: envs 16..23 cover either) with nothing valid."""
    B = 131
    graph = edge_graph(n, 3 * n)
    acts = forced_actions(n, B, 7, seed=n + 2)
    badv = np.array([-1, n, (1 << 31) + 5, (1 << 32) + 1, -(1 << 40)], dtype=np.int64)
    for t in (1, 2, 4):
        a = acts[t]
        idx = np.arange(1 + t, B, 3)
        a[idx] = badv[(idx + t) % len(badv)]
        a[16:24] = badv[np.arange(8) % len(badv)]
        a[0] = HUB                                   # valid hub next to invalid neighbours in the same wave
    run_ring(("bad", n, B), graph, n, spins(B, n, 5), acts, dt, {"RLS_STEP_CHASE": chase})


# ---------------------------------------------------------------------------------------------------------------- short runs, ragged grids
@pytest.mark.parametrize("with_cur_done", [True, False])
@pytest.mark.parametrize("n,B", [(2000, 201), (2000, 203),      # B = 4k + 1, 4k + 3: a last run of 1 and of 3 rows
                                 (1000, 203)])                  # runs of 8 rows; the last has 3 = 3000 bytes: 187 vectors + 8 bytes
def test_short_last_run(n, B, with_cur_done):
    graph = edge_graph(n, 3 * n)
    acts = forced_actions(n, B, 6, seed=B + n)
    for t, a in enumerate(acts):                    # the short run's envs pick the special nodes and its last bytes
        a[B - 1] = (HUB, n - 1, n - 2, D65, D64, n - 1)[t]
    run_ring(("short", n, B), graph, n, spins(B, n, 6), acts, "u8", {}, with_cur_done=with_cur_done)


@pytest.mark.parametrize("chase", [0, 1])
def test_short_last_run_f32(chase):
    """f32 rows of 1000 nodes: runs of 2 rows, the last of one."""
    n, B = 1000, 67
    graph = edge_graph(n, 3 * n)
    acts = forced_actions(n, B, 6, seed=B + n)
    run_ring(("short32", n, B), graph, n, spins(B, n, 6), acts, "f32", {"RLS_STEP_CHASE": chase})


# ---------------------------------------------------------------------------------------------------------------- persistent grid
@pytest.mark.parametrize("form", ["plain", "wt", "nt"])
@pytest.mark.parametrize("chase", [0, 1])
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_persistent_grid_three_trips(dt, chase, form):
    """RLS_STEP_PERSIST=1 with one wave per workgroup: 8 workgroups = 8 waves are resident per CU, so with 8 * 3 * (8 * CUs) + 5 envs of
    144 nodes (runs of 8 rows) every wave makes at least three trips and some a fourth, short one."""
    n = 144
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    B = 8 * 3 * (8 * cus) + 5
    graph = edge_graph(n, 2 * n)
    acts = forced_actions(n, B, 6, seed=11)
    acts[3][40:48] = n + 3                          # a wave with nothing valid, mid-loop
    extra = dict(FORMS[form], RLS_STEP_PERSIST=1, RLS_STEP_WPB=1, RLS_STEP_CHASE=chase)
    run_ring(("persist", B), graph, n, spins(B, n, 7), acts, dt, extra)


# ---------------------------------------------------------------------------------------------------------------- misaligned runs
@pytest.mark.parametrize("align", [1, 0])
@pytest.mark.parametrize("n,dt,chase", [(2000, "u8", 0), (144, "u8", 0), (144, "f32", 1), (144, "u8", 1)])
def test_misaligned_slots(n, dt, chase, align):
    """Slots that start 16, 48 and 112 bytes into a line; steps 0 -> 1 and 3 -> 4 have equal offsets on both sides, the others differ."""
    B = 67
    graph = edge_graph(n, 3 * n)
    acts = forced_actions(n, B, 8, seed=n + 3)
    run_ring(("misal", n, B), graph, n, spins(B, n, 8), acts, dt, {"RLS_STEP_CHASE": chase, "RLS_STEP_ALIGN": align},
             offsets=[16, 16, 48, 112, 112, 48, 16, 112])


# ---------------------------------------------------------------------------------------------------------------- captured graph
@pytest.mark.parametrize("n,dt", [(2000, "u8"), (144, "f32")])
def test_captured_chain_replayed_twice(n, dt):
    """8 steps round the whole ring in one captured graph, replayed twice (the second replay starts from the state the first one left
    in slot 0): equal to 16 eager steps and to the oracle."""
    B = 203
    graph = edge_graph(n, 3 * n)
    acts8 = forced_actions(n, B, 8, seed=n + 4)
    acts = acts8 + acts8
    xs = spins(B, n, 9)
    obj0, traj = trajectory(("graph", n, B), graph, n, xs, acts)
    g, x_eager, obj_eager = run_ring(("graph", n, B), graph, n, xs, acts, dt, {})

    tdt = torch.bool if dt == "u8" else torch.float32
    slots, _ = slot_views(B, n, tdt, None)
    slots[0].copy_(torch.from_numpy(xs).to(DEV).to(tdt))
    obj = torch.from_numpy(obj0.astype(np.int32)).to(DEV)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    cur = torch.empty(B, dtype=torch.float32, device=DEV)
    acts_dev = [torch.from_numpy(a).to(DEV) for a in acts8]
    launchers = [ops.maxcut_step_launcher(g, slots[t], slots[(t + 1) % 8], acts_dev[t], obj, reward, cur=cur) for t in range(8)]
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for launch in launchers:
            launch()
    for rep in range(2):
        gr.replay()
        torch.cuda.synchronize()
        x_ref, r_ref, c_ref, _ = traj[8 * rep + 7]
        assert np.array_equal(slots[0].float().cpu().numpy(), x_ref), rep
        assert np.array_equal(reward.cpu().numpy(), r_ref), rep
        assert np.array_equal(cur.cpu().numpy(), c_ref), rep
    assert torch.equal(slots[0], x_eager) and torch.equal(obj, obj_eager)
    assert torch.equal(ops.maxcut_obj(g, slots[0]), obj.long())
