"""S2V_PPO env: hip-event time of one step and one reset of VecEnvMaxcut (rls_s2vppo_step / rls_s2vppo_reset), beside the same step
written as batched torch ops on the same GPU in two forms of the delta update -- "gather": the action rows gathered through rowptr,
padded to the batch's longest row, O(B max deg); "list": one masked index_add_ over the whole edge list, O(E), more work than a step
needs but no padding to a hub's row -- with scatter sums for column 4,
the history test on Zobrist hashes; the basin table is left out of it, which only makes it cheaper).  Shapes: the reference's own
config (8 envs of 200 nodes, train_ddp.py), 4096 envs of 200 nodes, 64 envs of 10^4 nodes; BA-like graphs of mean degree 8.
Per shape: warm-up, then 7 interleaved groups of launches per variant, medians (min, max).
    python tools/timing/s2v_ppo_step.py [--quick] > profiles/s2v_ppo_kernels.txt"""
import os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd.envs.env_S2V_PPO import VecEnvMaxcut
dev = torch.device("cuda:0")


def t(f, reps):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def groups(fs, reps):
    for f in fs.values():
        t(f, 3)
    rows = {k: [] for k in fs}
    for _ in range(7):
        for k, f in fs.items():
            rows[k].append(t(f, reps))
    return rows


def ba_graph(rng, n, m=4):
    """preferential attachment, m lines per new node, both directions listed"""
    targets, repeated, e = list(range(m)), [], []
    for v in range(m, n):
        e += [(v, u) for u in targets]
        repeated += targets + [v] * m
        targets = list({repeated[i] for i in rng.randint(0, len(repeated), size=3 * m)})[:m]
    e = np.array(e, dtype=np.int64).T
    return {"edge_index": torch.from_numpy(np.concatenate([e, e[::-1]], axis=1)), "edge_weight": torch.ones(2 * e.shape[1]), "num_nodes": n}


class TorchStep:
    """the step of env.py:140-206 for the whole batch as torch ops on the concatenated layout (no host read)"""

    def __init__(self, env, gather):
        self.e, self.gather = env, gather
        self.src, self.dst, self.ew = env.edge_index[0], env.edge_index[1], env.edge_weight
        self.ebatch = env.batch[self.src]
        B, T = env.num_envs, env.z.numel()
        self.rowptr, self.col, self.w = env._rowptr, env._col.long(), env._w
        self.lanes = torch.arange(int((self.rowptr[1:] - self.rowptr[:-1]).max()), device=dev)[None, :]     # the longest row of the batch
        self.z, self.delta = env.z.float().clone(), env.delta_cache.clone()
        self.cut, self.best = env.current_cut.clone(), env.best_cut.clone()
        self.last_flip = torch.zeros(T, device=dev)
        self.keys = torch.randint(-2 ** 62, 2 ** 62, (T,), device=dev)
        self.hash = torch.zeros(B, dtype=torch.int64, device=dev)
        self.hist = torch.zeros((B, 50), dtype=torch.int64, device=dev)
        self.tabu = torch.zeros((B, env.tabu_tenure), dtype=torch.int64, device=dev)
        self.x = torch.zeros((T, 5), device=dev)
        self.mask = torch.ones(T, dtype=torch.bool, device=dev)
        self.n = env.num_nodes.float()
        self.steps = 0

    def __call__(self, actions):
        e = self.e
        ga = e.ptr[:-1] + actions
        d = self.delta[ga]
        self.z[ga] = -self.z[ga]
        self.cut += d.double()
        if self.gather:
            at = self.rowptr[ga][:, None] + self.lanes                   # [B, max deg]: the rows of the action nodes, padded
            live = at < self.rowptr[ga + 1][:, None]
            at = torch.where(live, at, 0)
            dst = self.col[at]
            self.delta.index_add_(0, dst.reshape(-1), torch.where(live, 2 * self.z[dst] * self.z[ga][:, None] * self.w[at], 0.0).reshape(-1))
        else:
            sel = self.src == ga[self.ebatch]
            self.delta.index_add_(0, self.dst, torch.where(sel, 2 * self.z[self.dst] * self.z[self.src] * self.ew, 0.0))
        self.delta[ga] = -self.delta[ga]
        self.steps += 1
        self.tabu[:, self.steps % e.tabu_tenure] = ga
        self.last_flip[ga] = self.steps
        self.hash ^= self.keys[ga]
        new = ~(self.hist == self.hash[:, None]).any(dim=1)
        gain = self.cut - self.best
        reward = torch.where(gain > 0, gain / (gain + 0.1), 0.0) - torch.where(new, 0.0, e.stag_punishment)
        self.best = torch.maximum(self.best, self.cut)
        npos = torch.zeros(e.num_envs, device=dev).index_add_(0, e.batch, (self.delta > 0).float())
        reward = reward + torch.where(npos == 0, 0.01, 0.0)
        self.hist[:, self.steps % 50] = self.hash
        self.x[:, 0] = self.z
        self.x[:, 1] = self.delta / e._wtot[:, 1][e.batch]
        self.x[:, 2] = 0
        self.x[self.tabu.reshape(-1), 2] = 1
        self.x[:, 3] = (self.steps - self.last_flip) / e.max_steps.float()[e.batch]
        self.x[:, 4] = (npos / self.n)[e.batch]
        self.mask.fill_(True)
        tb = self.tabu.reshape(-1)
        self.mask[tb[self.delta[tb] <= 0]] = False
        return reward


quick = "--quick" in sys.argv[1:]
fmt = lambda r: f"{np.median(r):9.1f} ({min(r):.1f}, {max(r):.1f})"           # noqa: E731
print("# python tools/timing/s2v_ppo_step.py  -- MI355X, medians of 7 interleaved groups (min, max), microseconds")
print("B N entries (longest row) form | step kernel us (ns per env-step) | reset kernel us, random | reset us, greedy | torch-op step us, rows gathered | torch-op step us, whole list (the faster of the two: x kernel)")
cfg = types.SimpleNamespace(device=dev, node_feature_dim=5, episode_length_multiplier=2, tabu_tenure=10, stag_punishment=0.01)
for B, N in ((8, 200), (512, 200)) if quick else ((8, 200), (4096, 200), (64, 10_000)):
    rng = np.random.RandomState(B + N)
    protos = [ba_graph(rng, N) for _ in range(min(B, 8))]
    env = VecEnvMaxcut([protos[i % len(protos)] for i in range(B)], cfg, seed=1)      # (a reset comes before any env ends)
    acts = [torch.from_numpy(rng.randint(0, N, size=B)).to(dev) for _ in range(16)]
    ref, ref_list = TorchStep(env, True), TorchStep(env, False)
    k = [0]

    def step():
        k[0] += 1
        env.step(acts[k[0] & 15])

    def tstep():
        k[0] += 1
        ref(acts[k[0] & 15])

    def lstep():
        k[0] += 1
        ref_list(acts[k[0] & 15])

    rnd, grd = torch.zeros(B, dtype=torch.bool, device=dev), torch.ones(B, dtype=torch.bool, device=dev)
    fs = {"step": step, "reset": lambda: env.reset(greedy=rnd), "greedy": lambda: env.reset(greedy=grd), "torch": tstep, "list": lstep}
    rows = groups(fs, 20 if B * N < 500_000 else 5)
    med = {key: float(np.median(v)) for key, v in rows.items()}
    plan = env.launch_plan()
    best = min(med["torch"], med["list"])
    note = "" if best > med["step"] else "   <-- the kernel is NOT faster than the torch-op forms here"
    print(f"{B} {N} {env.edge_index.shape[1]} ({ref.lanes.numel()}) {plan['form']}/{plan['block']} | {fmt(rows['step'])} ({1e3 * med['step'] / B:.1f}) | "
          f"{fmt(rows['reset'])} | {fmt(rows['greedy'])} | {fmt(rows['torch'])} | {fmt(rows['list'])} (x{best / med['step']:.1f}){note}", flush=True)
