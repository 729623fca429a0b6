"""sub_set_sampling (rls_sub_set_sampling) and the L2A search step on the GPU: the reference's recorded runs bit for bit, every
shape at which the kernel takes another turn against the numpy restatement (tests/subset_oracle.py), the lower-index tie rule,
the production draws (reproducible, shard-invariant, Bernoulli(det)), and search_step against the same body composed by hand."""
import math

import numpy as np
import pytest
import torch

import subset_oracle as orc
from test_subset_oracle import CASES, golden_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_op(probs, start, R, top_k, uniforms=None, seed=0, env_offset=0, want_probs=True):
    """Straight through torch.ops.rlsolver_hip.sub_set_sampling -> (xs, probs_out) as numpy; checks that the inputs are unchanged."""
    from rlsolver_amd.torch_ops import ops as T
    S, N = probs.shape
    d_probs, d_start = dev(probs), dev(start)
    d_uni = None if uniforms is None else dev(uniforms)
    xs = torch.empty((R * S, N), dtype=torch.bool, device=DEV)
    pr = torch.full((S, N), -7.0, dtype=torch.float32, device=DEV) if want_probs else None
    T.sub_set_sampling(d_probs, d_start, R, top_k, d_uni, seed, env_offset, xs, pr)
    assert np.array_equal(d_probs.cpu().numpy().view(np.uint32), probs.view(np.uint32)) and np.array_equal(d_start.cpu().numpy(), start)
    return xs.cpu().numpy(), (pr.cpu().numpy() if want_probs else None)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("tag", CASES)
def test_golden_parity(golden, tag):
    probs, start, R, top_k, uniforms, xs, probs_out = golden_case(golden("sub_set_sampling"), tag)
    got_xs, got_probs = run_op(probs, start, R, top_k, uniforms)
    assert np.array_equal(got_xs, xs)
    assert same_bits(got_probs, probs_out)


def shape_settings(N):
    ks = sorted({0, 1, N // 4, N - 1, N, N + 5})
    return [(k, R, S) for k in ks for R in (1, 2, 33) for S in (1, 3, 64)]


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 1000, 2000, 4099])
def test_shapes_against_the_restatement(N):
    """Rows of every alignment (odd N: each row starts at another byte), one and many sims, fewer and more repeats than one
    workgroup writes (the planner gives a workgroup 4 repeats where the sims alone do not fill the chip: 33 is cut into 9 chunks,
    the last one shorter), every edge of top_k."""
    rng = np.random.RandomState(1000 + N)
    for top_k, R, S in shape_settings(N):
        probs = rng.rand(S, N).astype(np.float32)
        start = rng.rand(S, N) < 0.5
        uniforms = (rng.rand(R * S, N) * 0.5).astype(np.float32)         # det <= 0.5: half of the draws land on either side
        want_xs, want_probs = orc.sub_set_sampling(probs, start, R, top_k, uniforms)
        got_xs, got_probs = run_op(probs, start, R, top_k, uniforms)
        assert np.array_equal(got_xs, want_xs), (N, top_k, R, S)
        assert same_bits(got_probs, want_probs), (N, top_k, R, S)


def test_output_at_any_byte_and_the_wrapper():
    """ops.sub_set_sampling into an `out` view that starts at every byte offset of a 16-byte line, N a multiple of 16 and not."""
    from rlsolver_amd import ops
    rng = np.random.RandomState(5)
    for N in (48, 50):
        S, R, top_k = 3, 5, 13
        probs, start = rng.rand(S, N).astype(np.float32), rng.rand(S, N) < 0.5
        uniforms = (rng.rand(R * S, N) * 0.5).astype(np.float32)
        want_xs, want_probs = orc.sub_set_sampling(probs, start, R, top_k, uniforms)
        for shift in range(16):
            buf = torch.zeros(R * S * N + 32, dtype=torch.bool, device=DEV)
            out = buf[shift:shift + R * S * N].view(R * S, N)
            xs, pr = ops.sub_set_sampling(dev(probs), dev(start), R, top_k, uniforms=dev(uniforms), out=out)
            assert xs.data_ptr() == out.data_ptr() and np.array_equal(xs.cpu().numpy(), want_xs), (N, shift)
            assert same_bits(pr.cpu().numpy(), want_probs)
            assert not buf[:shift].any() and not buf[shift + R * S * N:].any(), "bytes outside the output were written"


def test_output_overlapping_an_input_is_an_error():
    """Workgroups re-read the start row and the probs while others write xs: an output that shares bytes with an input is refused."""
    from rlsolver_amd import ops
    S, N, R = 4, 32, 2
    probs = torch.rand((S, N), device=DEV)
    big = torch.zeros(R * S * N + S * N, dtype=torch.bool, device=DEV)
    start_inside, out = big[:S * N].view(S, N), big[:R * S * N].view(R * S, N)
    with pytest.raises(RuntimeError, match="xs_out overlaps start_xs"):
        ops.sub_set_sampling(probs, start_inside, R, 5, out=out)
    as_bytes = torch.zeros(S * N * 4 + R * S * N, dtype=torch.uint8, device=DEV)
    probs_inside = as_bytes[:S * N * 4].view(torch.float32).view(S, N)
    with pytest.raises(RuntimeError, match="xs_out overlaps probs"):
        ops.sub_set_sampling(probs_inside, torch.zeros((S, N), dtype=torch.uint8, device=DEV), R, 5,
                             out=as_bytes[S * N * 4 - 1:S * N * 4 - 1 + R * S * N].view(R * S, N))
    xs, _ = ops.sub_set_sampling(probs, big[R * S * N:].view(S, N), R, 5, out=out)         # adjacent, not overlapping: fine
    assert xs.data_ptr() == out.data_ptr()


def test_node_limit_last_supported_and_first_refused():
    from rlsolver_amd import _abi, ops
    from rlsolver_amd.torch_ops import ops as T
    limit = ops.SUB_SET_SAMPLING_MAX_NODES
    rng = np.random.RandomState(9)
    for N in (limit, limit + 1):
        S, R, top_k = 2, 3, N // 4
        probs, start = rng.rand(S, N).astype(np.float32), rng.rand(S, N) < 0.5
        uniforms = (rng.rand(R * S, N) * 0.5).astype(np.float32)
        want_xs, want_probs = orc.sub_set_sampling(probs, start, R, top_k, uniforms)
        assert ops.sub_set_sampling_supported(S, N, R, top_k) == (N == limit)
        if N == limit:
            got_xs, got_probs = run_op(probs, start, R, top_k, uniforms)
        else:
            xs = torch.empty((R * S, N), dtype=torch.bool, device=DEV)
            with pytest.raises(RuntimeError, match=r"rls_sub_set_sampling failed \(-2\)"):          # RLS_EUNSUPPORTED, nothing launched
                T.sub_set_sampling(dev(probs), dev(start), R, top_k, dev(uniforms), 0, 0, xs, None)
            with pytest.raises(_abi.RlsError) as e:
                _abi.call("rls_sub_set_sampling", None, None, S, N, R, top_k, None, 0, 0, None, None, None)
            assert e.value.code == -2
            xs, pr = ops.sub_set_sampling(dev(probs), dev(start), R, top_k, uniforms=dev(uniforms))   # the wrapper's torch path
            got_xs, got_probs = xs.cpu().numpy(), pr.cpu().numpy()
        assert np.array_equal(got_xs, want_xs), N
        assert same_bits(got_probs, want_probs), N


def test_ties_go_to_the_lower_node_index():
    N, R, top_k = 70, 3, 20
    d = np.float32(0.125)
    probs = np.empty((3, N), dtype=np.float32)
    probs[0] = 0.5                                                                       # every det equal (0)
    probs[1] = np.where(np.arange(N) % 3 == 0, 0.3, 0.9)                                 # two distinct values: 24 nodes hold the smaller det
    probs[2] = np.where(np.arange(N) % 2 == 0, 0.5 + d, 0.5 - d)                         # p / 1 - p pairs: one det, the boundary inside them
    probs[2, 60:] = 0.5 + np.float32(0.375)
    rng = np.random.RandomState(2)
    start = rng.rand(3, N) < 0.5
    uniforms = (rng.rand(R * 3, N) * 0.25).astype(np.float32)
    assert not orc.boundary_is_distinct(probs, top_k)
    want_xs, want_probs = orc.sub_set_sampling(probs, start, R, top_k, uniforms)
    got_xs, got_probs = run_op(probs, start, R, top_k, uniforms)
    assert np.array_equal(got_xs, want_xs) and same_bits(got_probs, want_probs)
    sel = orc.selected_mask(probs, top_k)
    assert np.array_equal(sel[0], np.arange(N) < top_k) and np.array_equal(sel[2], np.arange(N) < top_k)
    assert not got_xs.reshape(R, 3, N)[:, 0, :top_k].any(), "det = 0: no uniform is below it, every selected bit is 0"
    # exactly min(top_k, N) nodes per sim can differ from the start row: uniforms of 0 and of 1 set every selected bit both ways
    for k in (top_k, N + 3):
        ones, _ = run_op(probs[1:], start[1:], 1, k, np.zeros((2, N), np.float32), want_probs=False)
        zeros, _ = run_op(probs[1:], start[1:], 1, k, np.ones((2, N), np.float32), want_probs=False)
        assert np.array_equal((ones != zeros).sum(axis=1), [min(k, N)] * 2)
        assert np.array_equal(ones != zeros, orc.selected_mask(probs[1:], k))


def test_production_draws_reproducible_sharded_and_restated():
    from rlsolver_amd import ops
    S, N, R, top_k = 6, 203, 9, 50
    rng = np.random.RandomState(11)
    probs, start = rng.rand(S, N).astype(np.float32), rng.rand(S, N) < 0.5
    seed, off = 0x1234_5678_9ABC_DEF0, 2 ** 32 + 40
    a, pa = run_op(probs, start, R, top_k, None, ops._s64(seed), off)
    b, _ = run_op(probs, start, R, top_k, None, ops._s64(seed), off)
    c, _ = run_op(probs, start, R, top_k, None, ops._s64(seed + 1), off)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    sel = orc.selected_mask(probs, top_k)
    assert np.array_equal(a.reshape(R, S, N)[:, ~sel], np.broadcast_to(start[~sel], (R, (~sel).sum()))), "an unselected entry moved"
    # two shards of the sims, env_offset = off and off + S / 2, hold the whole batch's rows (r, s)
    h = S // 2
    lo, _ = run_op(probs[:h], start[:h], R, top_k, None, ops._s64(seed), off)
    hi, _ = run_op(probs[h:], start[h:], R, top_k, None, ops._s64(seed), off + h)
    whole = a.reshape(R, S, N)
    assert np.array_equal(lo.reshape(R, h, N), whole[:, :h]) and np.array_equal(hi.reshape(R, S - h, N), whole[:, h:])
    # the torch path past the node limit draws the same uniforms: the kernel's result bit for bit
    xs, pr = ops.sub_set_sampling_torch(dev(probs), dev(start), R, top_k, None, seed, off)
    assert np.array_equal(xs.cpu().numpy(), a) and same_bits(pr.cpu().numpy(), pa)


def test_production_draws_are_bernoulli_of_the_determinism():
    """Per selected (sim, node) the mean over R repeats lies within 5 binomial standard deviations of min(det, 1); of the 2048 cells
    at most max(1, ceil(2048 P(|z| > 5))) = 1 may lie outside."""
    S, N, top_k, R = 16, 512, 128, 4096
    g = torch.Generator().manual_seed(77)
    probs = torch.rand((S, N), generator=g, dtype=torch.float32)
    start = torch.rand((S, N), generator=g) < 0.5
    xs = torch.empty((R * S, N), dtype=torch.bool, device=DEV)
    from rlsolver_amd.torch_ops import ops as T
    T.sub_set_sampling(probs.to(DEV), start.to(DEV), R, top_k, None, 20261020, 0, xs, None)
    mean = (xs.view(R, S, N).sum(dim=0, dtype=torch.int64).double() / R).cpu().numpy()
    sel = orc.selected_mask(probs.numpy(), top_k)
    assert sel.sum() == S * top_k == 2048
    p = np.minimum(orc.determinism(probs.numpy())[0].astype(np.float64), 1.0)[sel]
    sd = np.sqrt(p * (1.0 - p) / R)
    outside = int((np.abs(mean[sel] - p) > 5.0 * sd).sum())
    allowed = max(1, math.ceil(2048 * math.erfc(5.0 / math.sqrt(2.0))))
    print(f"cells outside 5 sd: {outside} of 2048 (allowed {allowed}); largest |z| {np.max(np.abs(mean[sel] - p) / np.maximum(sd, 1e-300)):.2f}")
    assert outside <= allowed
    assert np.array_equal(xs.view(R, S, N)[:, torch.from_numpy(~sel).to(DEV)].cpu().numpy(),
                          np.broadcast_to(start.numpy()[~sel], (R, (~sel).sum())))


def _graphs(golden):
    from tests.gpu_util import gnm_arr
    ba = golden("maxcut_obj")["BA_100_ID0/graph"]
    return {"BA_100_ID0": (ba, 100), "gnm_300": (gnm_arr(300, 1200, 21), 300)}


@pytest.mark.parametrize("name", ["BA_100_ID0", "gnm_300"])
def test_search_step_equals_the_body_composed_by_hand(golden, name, tmp_path):
    from rlsolver_amd import ops
    from rlsolver_amd.envs.env_L2A import EnvMaxcut
    from rlsolver_amd.methods import L2A
    from rlsolver_amd.methods.util_evaluator import Evaluator
    from rlsolver_amd.methods.util_read_data import pick_xs_by_vs, update_xs_by_vs
    garr, n = _graphs(golden)[name]
    graph = [tuple(int(v) for v in r) for r in garr]
    S, R, top_k, searchers, iters = 8, 4, n // 4, 2, 8
    sim = EnvMaxcut(mygraph=graph, device=DEV, if_bidirectional=True, num_nodes=n, seed=5)
    best_xs = sim.generate_xs_randomly(S)
    best_vs = sim.calculate_obj_values(best_xs)
    evaluator = Evaluator(save_dir=str(tmp_path), num_bits=n, if_maximize=True, x=best_xs[0], v=best_vs[0])
    hand_xs, hand_vs = best_xs.clone(), best_vs.clone()
    g = torch.Generator().manual_seed(3)
    for t in range(3):
        probs = (L2A.convert_solution_to_prob(best_xs)[:, :, 0].T.float() * 0.3 + 0.5
                 + torch.randn((S, n), generator=g).to(DEV) * 0.05)                       # stand-in policy: spins pulled toward 0.5
        uniforms = torch.rand((R * S, n), generator=g).to(DEV)
        noise = torch.randn((searchers, iters + 1, R * S, n), generator=g).to(DEV)
        before_xs, before_vs = best_xs.clone(), best_vs.clone()
        curr_xs, curr_vs, rewards = L2A.search_step(sim, probs, best_xs, best_vs, R, top_k, searchers, evaluator=evaluator, iter_i=t,
                                                    uniforms=uniforms, noise=noise)
        assert torch.equal(curr_xs, before_xs) and torch.equal(curr_vs, before_vs)
        assert (best_vs >= before_vs).all()
        assert torch.equal(rewards, best_vs - curr_vs)
        assert torch.equal(best_vs, sim.calculate_obj_values(best_xs))
        # the same body from the existing ops
        full_xs, _ = ops.sub_set_sampling(probs.contiguous(), hand_xs, R, top_k, uniforms=uniforms)
        full_vs = None
        for k in range(searchers):
            full_xs, full_vs = sim.local_search_inplace(full_xs, torch.empty(()), noise=noise[k])
        good_xs, good_vs = pick_xs_by_vs(full_xs, full_vs, R, True)
        update_xs_by_vs(hand_xs, hand_vs, good_xs, good_vs, True)
        assert torch.equal(hand_xs, best_xs) and torch.equal(hand_vs, best_vs)
    assert evaluator.best_v == int(best_vs.max())
    assert int(best_vs.sum()) > int(sim.calculate_obj_values(sim.generate_xs_randomly(S)).sum())     # the search did search


def test_search_step_with_its_own_draws_is_reproducible(golden):
    from rlsolver_amd.envs.env_L2A import EnvMaxcut
    from rlsolver_amd.methods import L2A
    garr, n = _graphs(golden)["BA_100_ID0"]
    graph = [tuple(int(v) for v in r) for r in garr]
    runs = []
    for _ in range(2):
        sim = EnvMaxcut(mygraph=graph, device=DEV, if_bidirectional=True, num_nodes=n, seed=8)
        best_xs = sim.generate_xs_randomly(8)
        best_vs = sim.calculate_obj_values(best_xs)
        probs = torch.rand((8, n), generator=torch.Generator().manual_seed(1)).to(DEV)
        for t in range(2):
            L2A.search_step(sim, probs, best_xs, best_vs, 4, n // 4, 2)
        runs.append((best_xs.clone(), best_vs.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    with pytest.raises(ValueError):
        L2A.search_step(sim, probs, best_xs, best_vs, 4, n // 4, 0)
