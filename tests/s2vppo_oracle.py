"""numpy restatement of the S2V_PPO MaxCut env (rlsolver/methods/S2V_PPO/env.py), what rls_s2vppo_step / rls_s2vppo_reset are
compared with.  float64 deltas and cut; history and basins compare WHOLE states (the kernel compares 64-bit hashes); the feature
columns are formed in float32 exactly as the reference forms them; column 3 comes from the step number of a node's last flip
(the reference adds 1.0 to every node each step: the same float32 for counts below 2^24).  With integer-valued weights every
quantity is exact, so the kernel, the reference and this file agree bit for bit (tests/golden/s2v_ppo.npz)."""
from collections import deque

import numpy as np

HISTORY = 50


class OracleEnv:
    def __init__(self, edge_index, edge_weight, num_nodes, multiplier=2, tenure=10, stag=0.01):
        ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
        self.src, self.dst = ei[0], ei[1]
        self.w32 = np.asarray(edge_weight, dtype=np.float32).reshape(-1)
        self.w = self.w32.astype(np.float64)
        self.n = int(num_nodes)
        self.max_steps = int(multiplier) * self.n
        self.tenure, self.stag = int(tenure), float(stag)
        self.total_weight = np.float32(self.w32.sum(dtype=np.float32) / np.float32(2))
        self.wden = np.float32(self.total_weight + np.float32(1e-8))
        order = np.argsort(self.src, kind="stable")         # rows[i]: the entries with src == i, in list order
        self.rows = np.split(order, np.cumsum(np.bincount(self.src, minlength=self.n))[:-1]) if self.n else []

    # ---- reset ------------------------------------------------------------------------------------------------------
    def all_deltas(self, z):
        nb = np.zeros(self.n)
        np.add.at(nb, self.src, self.w * z[self.dst])
        return z * nb

    def greedy_start(self):
        """env.py:51-57 -> (z, flips made)"""
        z = np.ones(self.n)
        flips = 0
        for _ in range(self.n // 2):
            gains = self.all_deltas(z)
            best = int(np.argmax(gains))                 # the first of equal maxima, as torch's argmax on CPU
            if gains[best] <= 0:
                break
            z[best] = -z[best]
            flips += 1
        return z, flips

    def reset(self, z0):
        self.z = np.asarray(z0, dtype=np.float64).copy()
        self.delta = self.all_deltas(self.z)
        self.cut = float(self.total_weight) / 2 - float(self.delta.sum()) / 4
        self.best_cut, self.best_z = self.cut, self.z.copy()
        self.steps = 0
        self.last_flip = np.zeros(self.n, dtype=np.int64)
        self.tabu = deque(maxlen=self.tenure)
        self.history = deque(maxlen=HISTORY)
        self.basins = set()
        return self.state()

    # ---- what a step returns ----------------------------------------------------------------------------------------
    def state(self):
        x = np.zeros((self.n, 5), dtype=np.float32)
        d32 = self.delta.astype(np.float32)
        x[:, 0] = self.z
        x[:, 1] = d32 / self.wden
        mask = np.ones(self.n, dtype=bool)
        if self.tenure > 0 and self.tabu:
            t = np.array(self.tabu, dtype=np.int64)
            x[t, 2] = 1.0
            mask[t[self.delta[t] <= 0]] = False
        if self.n:
            x[:, 3] = (self.steps - self.last_flip).astype(np.float32) / np.float32(self.max_steps)
            x[:, 4] = np.float32((self.delta > 0).sum()) / np.float32(self.n)
        return x, mask

    def step(self, a):
        a = int(a)
        self.cut += float(self.delta[a])
        self.z[a] = -self.z[a]
        rows = self.rows[a]
        np.add.at(self.delta, self.dst[rows], 2.0 * self.z[self.dst[rows]] * self.z[a] * self.w[rows])
        self.delta[a] = -self.delta[a]                  # after the row: a loop (a, a) has added to it
        self.steps += 1
        if self.tenure > 0:
            self.tabu.append(a)
        self.last_flip[a] = self.steps
        key = self.z.astype(np.int8).tobytes()
        new = key not in self.history
        r = 0.0
        if self.cut > self.best_cut:
            r = (self.cut - self.best_cut) / (self.cut - self.best_cut + 0.1)
            self.best_cut, self.best_z = self.cut, self.z.copy()
        if not new:
            r -= self.stag
        if (self.delta <= 0).all() and key not in self.basins:
            r += 0.01
            self.basins.add(key)
        self.history.append(key)
        x, mask = self.state()
        return dict(x=x, mask=mask, reward=r, done=self.steps >= self.max_steps, cut=self.cut, best=self.best_cut)


def random_graph(rng, n, m, weights="unit"):
    """m distinct lines on n nodes, both directions listed as the reference's loader does -> (edge_index [2, 2m], w f32 [2m])"""
    pairs = set()
    limit = n * (n - 1) // 2
    m = min(m, limit)
    while len(pairs) < m:
        u, v = int(rng.randint(0, n)), int(rng.randint(0, n))
        if u != v:
            pairs.add((min(u, v), max(u, v)))
    e = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    if weights == "unit":
        w = np.ones(len(e), dtype=np.float32)
    elif weights == "pm1":
        w = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=len(e))
    else:
        w = rng.uniform(0.1, 1.0, size=len(e)).astype(np.float32)
    return np.concatenate([e.T, e.T[::-1]], axis=1), np.concatenate([w, w])


def golden_case(z, name):
    """one trace of tests/golden/s2v_ppo.npz, unpacked: row 0 of x / mask / cut / best is the reset state"""
    p = name + "/"
    n, tenure, multiplier, greedy = (int(v) for v in z[p + "meta"])
    c = dict(name=name, n=n, tenure=tenure, multiplier=multiplier, greedy=bool(greedy), edge_index=z[p + "edge_index"].astype(np.int64),
             edge_weight=z[p + "edge_weight"], z0=z[p + "z0"], actions=z[p + "actions"].astype(np.int64), reward=z[p + "reward"],
             cut=z[p + "cut"], best=z[p + "best"], best_z=z[p + "best_z"])
    steps = len(c["actions"])
    c["done"] = np.unpackbits(z[p + "done"])[:steps].astype(bool)
    if p + "delta" in z.files:
        c["delta"] = z[p + "delta"]
        return c
    x = np.zeros((steps + 1, n, 5), dtype=np.float32)
    x[:, :, 0], x[:, :, 1], x[:, :, 3] = z[p + "x0"], z[p + "x1"], z[p + "x3"]
    x[:, :, 2] = np.unpackbits(z[p + "x2"], axis=1)[:, :n]
    x[:, :, 4] = z[p + "x4"][:, None]
    c["x"] = x
    c["mask"] = np.unpackbits(z[p + "mask"], axis=1)[:, :n].astype(bool)
    return c


def oracle_for(c, stag=0.01):
    return OracleEnv(c["edge_index"], c["edge_weight"], c["n"], c["multiplier"], c["tenure"], stag)
