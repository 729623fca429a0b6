"""K4's store policies (csrc/rls_step.hip, st_vec): plain, nontemporal and write-through (sc1) stores of the emitted next state.
Every form, forced through rls_tuning_set or chosen by the launcher, must give the bits of the oracle: next state, reward and obj,
on a chained 8-slot rollout ring, on non-chained calls, on ragged batches, short last runs, f32 rows (the chase form), the persistent
grid, out-of-range actions and inside a captured hipGraph."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import _abi, ops
from tests.gpu_util import DEV, device_graph, gnm_arr, to_dev_bool

pytestmark = pytest.mark.gpu

# knob settings of one store form; "auto" leaves the launcher's rule in charge (write-through at these sizes)
FORMS = {"auto": {}, "plain": {"RLS_STEP_WT": 0, "RLS_STEP_NTS": 0}, "wt": {"RLS_STEP_WT": 1, "RLS_STEP_NTS": 0},
         "nt": {"RLS_STEP_NTS": 1}}


@contextlib.contextmanager
def knobs(**kv):
    for k, v in kv.items():
        _abi.tuning_set(k, v)
    try:
        yield
    finally:
        for k in kv:
            _abi.tuning_unset(k)


def _ring_vs_oracle(n, m, B, dt, steps, extra, chained=True, bad_at=None):
    graph = gnm_arr(n, m, seed=n % 89)
    g = device_graph(graph, n, 0)
    rng = np.random.RandomState(B + n)
    xs = rng.randint(0, 2, size=(B, n)).astype(np.uint8)
    env = onp.PPOEnvOracle(graph, n, 10 ** 9, False)
    env.reset_to(xs)
    tdt = torch.bool if dt == "u8" else torch.float32
    x0 = to_dev_bool(xs) if dt == "u8" else to_dev_bool(xs).float()
    slots = [torch.empty_like(x0) for _ in range(8)]
    slots[0].copy_(x0)
    obj = ops.maxcut_obj(g, x0).to(torch.int32)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    cur = torch.empty(B, dtype=torch.float32, device=DEV)
    state = env.xs.copy()
    with knobs(**extra):
        for t in range(steps):
            a = rng.randint(0, n, size=B)
            src = slots[t % 8]
            if not chained and t % 2:        # a non-chained call: the input is a copy, not the slot the last call wrote
                src = src.clone()
            dst = slots[(t + 1) % 8]
            act = torch.from_numpy(a).to(DEV)
            bad = np.zeros(B, dtype=bool)
            if bad_at is not None and t == bad_at:
                bad[::5] = True
                act[torch.from_numpy(bad).to(DEV)] = torch.tensor([n, -1, n + 7], device=DEV).repeat(B)[: int(bad.sum())]
            obj_before = obj.clone()
            ops.maxcut_step(g, src, dst, act, obj, reward, cur=cur)
            r_dev, o_dev, x_dev = reward.cpu().numpy(), obj.cpu().numpy(), dst.float().cpu().numpy()
            if bad.any():
                # out-of-range actions: reward NaN, env and obj untouched; the others step as the oracle does
                assert bool(np.isnan(r_dev[bad]).all()) and np.array_equal(o_dev[bad], obj_before.cpu().numpy()[bad]), t
                assert np.array_equal(x_dev[bad], state[bad]), t
                ok = ~bad
                sub = onp.PPOEnvOracle(graph, n, 10 ** 9, False)
                sub.reset_to(state[ok].astype(np.uint8))
                _, r, _, c = sub.step(a[ok])
                assert np.array_equal(r_dev[ok], r) and np.array_equal(o_dev[ok].astype(np.float32), c), t
                state[ok] = sub.xs
                env.reset_to(state.astype(np.uint8))
            else:
                _, r, _, c = env.step(a)
                assert np.array_equal(r_dev, r) and np.array_equal(o_dev.astype(np.float32), c), t
                assert np.array_equal(cur.cpu().numpy(), c), t
                state = env.xs.copy()
            assert np.array_equal(x_dev, state), t
    assert dst.dtype == tdt
    assert np.array_equal(ops.maxcut_obj(g, dst).cpu().numpy(), obj.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n,m,B", [(2000, 19990, 203),    # G22 rows; 203 envs: not a multiple of EPW x waves x 8 (remainder blocks)
                                   (1000, 5000, 203),     # runs of 8 rows = 8000 bytes, a short last run of 3 rows (element tail)
                                   (2000, 19990, 512)])   # whole workgroups only
def test_ring_u8_every_store_form(form, n, m, B):
    _ring_vs_oracle(n, m, B, "u8", 10, FORMS[form])


@pytest.mark.parametrize("form", list(FORMS))
def test_non_chained_calls(form):
    _ring_vs_oracle(2000, 19990, 131, "u8", 6, FORMS[form], chained=False)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("chase", [1, 0])
def test_f32_rows_chase_and_staged_forms(form, chase):
    """f32 rows run MODE 3 (the stores chase the loads) by default; write-through there only when forced."""
    _ring_vs_oracle(2000, 19990, 67, "f32", 6, dict(FORMS[form], RLS_STEP_CHASE=chase))


def _ring_bits(g, x0, acts, extra):
    """The ring's next states, rewards and objs on the GPU under one set of knobs."""
    slots = [torch.empty_like(x0) for _ in range(8)]
    slots[0].copy_(x0)
    obj = ops.maxcut_obj(g, x0).to(torch.int32)
    reward = torch.empty(x0.shape[0], dtype=torch.float32, device=DEV)
    out = []
    with knobs(**extra):
        for t, a in enumerate(acts):
            ops.maxcut_step(g, slots[t % 8], slots[(t + 1) % 8], a, obj, reward)
            out.append((slots[(t + 1) % 8].clone(), reward.clone(), obj.clone()))
    return out


@pytest.mark.parametrize("form", ["auto", "wt", "plain"])
def test_persistent_grid(form):
    """RLS_STEP_PERSIST=1: 2^15 + 37 envs of 2000 nodes are 8202 runs, more than the 5120 waves resident at once, so the waves loop.  Bits
    against the one-shot grid with plain stores (the form before write-through); obj against a from-scratch evaluation."""
    n, B = 2000, 2 * 16384 + 37
    g = device_graph(gnm_arr(n, 19990, seed=5), n, 0)
    x0 = ops.rand_spins(B, n, 3, DEV)
    acts = [ops.rand_actions(B, n, 7, s, DEV) for s in range(4)]
    acts[2][::9] = n + 1                                                   # and some out-of-range actions
    ref = _ring_bits(g, x0, acts, {"RLS_STEP_PERSIST": 0, "RLS_STEP_WT": 0, "RLS_STEP_NTS": 0})
    got = _ring_bits(g, x0, acts, dict(FORMS[form], RLS_STEP_PERSIST=1))
    for t, ((xr, rr, orf), (xg, rg, og)) in enumerate(zip(ref, got)):
        assert torch.equal(xr, xg) and torch.equal(orf, og), t
        assert torch.equal(torch.isnan(rr), torch.isnan(rg)) and torch.equal(rr.nan_to_num(), rg.nan_to_num()), t
    assert torch.equal(ops.maxcut_obj(g, got[-1][0]), got[-1][2].long())


@pytest.mark.parametrize("form", list(FORMS))
def test_out_of_range_actions(form):
    _ring_vs_oracle(2000, 19990, 203, "u8", 5, FORMS[form], bad_at=2)


@pytest.mark.parametrize("form", ["auto", "wt"])
def test_captured_graph_with_an_odd_number_of_steps(form):
    """Steps 1..5 of the ring captured into one hipGraph (step 0 eager: it loads the kernel), replayed once."""
    n, m, B = 2000, 19990, 203
    graph = gnm_arr(n, m, seed=11)
    g = device_graph(graph, n, 0)
    rng = np.random.RandomState(12)
    xs = rng.randint(0, 2, size=(B, n)).astype(np.uint8)
    env = onp.PPOEnvOracle(graph, n, 10 ** 9, False)
    env.reset_to(xs)
    slots = [torch.empty((B, n), dtype=torch.bool, device=DEV) for _ in range(8)]
    slots[0].copy_(to_dev_bool(xs))
    obj = ops.maxcut_obj(g, slots[0]).to(torch.int32)
    reward = torch.empty(B, dtype=torch.float32, device=DEV)
    acts = [rng.randint(0, n, size=B) for _ in range(6)]
    acts_dev = [torch.from_numpy(a).to(DEV) for a in acts]
    with knobs(**FORMS[form]):
        launchers = [ops.maxcut_step_launcher(g, slots[t], slots[t + 1], acts_dev[t], obj, reward) for t in range(6)]
        launchers[0]()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for t in range(1, 6):
                launchers[t]()
        gr.replay()
        torch.cuda.synchronize()
    for t in range(6):
        _, r, _, c = env.step(acts[t])
    assert np.array_equal(reward.cpu().numpy(), r) and np.array_equal(obj.cpu().numpy().astype(np.float32), c)
    assert np.array_equal(slots[6].float().cpu().numpy(), env.xs)
