"""The MaxCut env of S2V_PPO -- drop-in for rlsolver/methods/S2V_PPO/env.py, and the batch of them that train_ddp.py:85-163 steps in
a Python loop as ONE kernel per step (rls_s2vppo_step) and per reset (rls_s2vppo_reset).

``VecEnvMaxcut(graph_datas, config)`` holds B envs on B DIFFERENT graphs, laid out like ``Batch.from_data_list``: ``ptr`` [B + 1],
``batch`` [sum N], ``edge_index`` with the node offsets added, and every per-node array (``x`` [sum N, 5], ``valid_actions_mask``, ``z``,
``delta_cache``, ``best_z``) concatenated in env order.  ``x`` and the mask are persistent buffers rewritten in place by every step,
as the reference's are (train_ddp.py clones what it keeps).  ``reward`` / ``done`` / ``cut_value`` / ``best_cut`` come back as device
tensors [B] (float64 / bool): nothing is read back to the host.  The edge list counts AS GIVEN, like the reference's row reads
(env.py:199): a line listed twice adds twice, a loop (u, u) is an ordinary entry, a one-directional line stays one-directional.

What differs from the reference, all of it stated:

* a state's identity (the last-50 history, the visited basins) is a 64-bit Zobrist hash kept on the device; the reference compares
  Python hashes of the spin bytes.  Two different states of one episode collide with probability about 2^-64 per pair: at most
  max_steps * 50 history pairs and max_steps^2 / 2 basin pairs per episode, below 10^-11 for a 10^4-node graph;
* ``step()`` on an env that is already done raises ``ValueError("... reset it first")`` (a host mirror of the step count, no device
  read): the basin table holds one episode.  The mirror counts calls, so it never lags the device on eager steps: an out-of-range
  action (reward NaN, env untouched, as rls_maxcut_step) counts although the device does not move, and the guard may then fire
  early; ``sync_steps()`` reads the device's counts back (one host read).  A captured graph that is replayed advances the device
  only: ``count_steps(k)`` or ``sync_steps()`` tells the mirror.  Where the mirror does lag, the kernel itself leaves a done env
  untouched and reports reward NaN, done True;
* ``z`` / ``best_z`` are int8 (the reference: int64), ``current_cut`` / ``best_cut`` of the batch are float64 tensors;
* production ``reset()`` draws its coin and spins from the counter-based generator of the ISCO steps, keyed by (seed, env_offset + env,
  the env's episode counter): shards of a batch reproduce the whole batch (rlsolver_amd/seeding.py).

``EnvMaxcut(graph_data, config)`` is the single env with the reference's attribute names; its ``step(int)`` returns Python scalars
(one device read, what Inference.py:53-88 needs).  The reference's host-side bookkeeping (``tabu_list``, ``state_history``,
``visited_basins``, ``time_since_flip``, ``no_improve_count``) lives on the device in another form and has no attribute here.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..seeding import Sharded
from ..torch_ops import ops as _t

NODE_FEATURE_DIM = 5
HISTORY = 50


def _np(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def build_batch_csr(graph_datas: Sequence[dict]) -> dict:
    """The host side of a batch (numpy; plumbing): graph_datas[i] = {'edge_index': [2, E_i], 'edge_weight': [E_i], 'num_nodes': N_i}.

    -> ptr int64 [B + 1]; rowptr int64 [sum N + 1], col int32 / w f32 [sum E]: one CSR by source over the concatenated nodes, every
    entry kept in its multiplicity (loops too), a row sorted by destination with equal destinations in list order; edge_index int64
    [2, sum E] / edge_weight f32: the lists concatenated in the given order with ptr[i] added (Batch.from_data_list); num_nodes int64
    [B]; wtot f32 [B, 3] = (W, W + 1e-8, symmetric) with W = sum(w) / 2 in float32 (env.py:19, :119) and symmetric = 1 when the list equals
    its transpose, weights included (the greedy reset then follows a flip through the node's own row); degrees f32 [sum N] (env.py:23-28)."""
    B = len(graph_datas)
    ns = np.array([int(g["num_nodes"]) for g in graph_datas], dtype=np.int64).reshape(B)
    if (ns < 0).any():
        raise ValueError("num_nodes must be >= 0")
    ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(ns, out=ptr[1:])
    total = int(ptr[-1])
    eis, ws, cols, wsorted, counts = [], [], [], [], [np.zeros(0, dtype=np.int64)]
    wtot = np.zeros((B, 3), dtype=np.float32)
    degrees = np.zeros(total, dtype=np.float32)
    for i, g in enumerate(graph_datas):
        ei = _np(g["edge_index"], np.int64).reshape(2, -1)
        w = _np(g["edge_weight"], np.float32).reshape(-1)
        n = int(ns[i])
        if ei.shape[1] != w.shape[0]:
            raise ValueError(f"graph {i}: edge_index has {ei.shape[1]} entries, edge_weight {w.shape[0]}")
        if ei.size and (ei.min() < 0 or ei.max() >= n):
            raise ValueError(f"graph {i}: edge_index outside [0, {n})")
        order = np.lexsort((ei[1], ei[0]))                    # by source, then destination; stable: equal pairs keep list order
        cols.append((ei[1][order] + ptr[i]).astype(np.int32))
        wsorted.append(w[order])
        counts.append(np.bincount(ei[0], minlength=n).astype(np.int64))
        eis.append(ei + ptr[i])
        ws.append(w)
        tw = torch.from_numpy(w).sum() / 2                    # float32, as the reference forms it
        wtot[i, 0], wtot[i, 1] = float(tw), float(tw + 1e-8)
        back = np.lexsort((w, ei[0], ei[1]))                  # the transposed list in the order `order` gives the list itself
        fwd = np.lexsort((w, ei[1], ei[0]))
        wtot[i, 2] = float(np.array_equal(ei[0][fwd], ei[1][back]) and np.array_equal(ei[1][fwd], ei[0][back]) and np.array_equal(w[fwd], w[back]))
        np.add.at(degrees, ei[0] + ptr[i], w)
    rowptr = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(np.concatenate(counts), out=rowptr[1:])
    cat = lambda parts, dt, shape: np.concatenate(parts, axis=-1) if parts else np.zeros(shape, dtype=dt)   # noqa: E731
    return dict(ptr=ptr, rowptr=rowptr, col=cat(cols, np.int32, 0), w=cat(wsorted, np.float32, 0), edge_index=cat(eis, np.int64, (2, 0)),
                edge_weight=cat(ws, np.float32, 0), num_nodes=ns, wtot=wtot, degrees=degrees)


def launch_plan(num_envs: int, max_nodes: int) -> dict:
    """What rls_s2vppo_step / _reset launch for this batch (csrc/rls_s2vppo_plan.h; a host query, no device needed)."""
    import ctypes as C
    from .. import _abi
    out = (C.c_int64 * 4)()
    _abi.call("rls_s2vppo_launch_plan", int(num_envs), int(max_nodes), C.cast(out, C.c_void_p))
    return dict(form=("wave", "workgroup")[out[0]], block=int(out[1]), envs_per_workgroup=int(out[2]), grid=int(out[3]))


class VecEnvMaxcut(Sharded):
    def __init__(self, graph_datas: Sequence[dict], config, env_offset: int = 0, seed: Optional[int] = None):
        """``config``: device, node_feature_dim (5), episode_length_multiplier, tabu_tenure, stag_punishment (S2V_PPO/config.py).
        ``env_offset`` / ``seed``: rlsolver_amd/seeding.py -- the batch is this rank's share of the envs."""
        self._init_shard(env_offset, seed)
        self.config = config
        self.device = torch.device(config.device)
        if self.device.type != "cuda":
            raise TypeError(f"rlsolver_amd.VecEnvMaxcut needs a HIP device (got {self.device}); there is no CPU path")
        if int(getattr(config, "node_feature_dim", NODE_FEATURE_DIM)) != NODE_FEATURE_DIM:
            raise ValueError(f"node_feature_dim must be {NODE_FEATURE_DIM}")
        self.tabu_tenure = int(config.tabu_tenure)
        self.episode_length_multiplier = int(config.episode_length_multiplier)
        self.stag_punishment = float(config.stag_punishment)
        if self.tabu_tenure < 0 or self.episode_length_multiplier < 1:
            raise ValueError("tabu_tenure must be >= 0 and episode_length_multiplier >= 1")
        self._graphs = list(graph_datas)
        if any(int(g["num_nodes"]) < 1 for g in self._graphs):
            raise ValueError("every graph needs at least one node")
        self.num_envs = len(self._graphs)
        self._draw_seed = self._next_seed()           # one seed for the object's life: an env's draws move with its episode counter
        B = self.num_envs
        dev = self.device
        self._counters = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.current_cut = torch.zeros(B, dtype=torch.float64, device=dev)
        self.best_cut = torch.zeros(B, dtype=torch.float64, device=dev)
        self._tabu = torch.zeros((B, max(self.tabu_tenure, 1)), dtype=torch.int32, device=dev)
        self._hash = torch.zeros((B, HISTORY + 1), dtype=torch.int64, device=dev)
        self.reward = torch.zeros(B, dtype=torch.float64, device=dev)
        self.done = torch.zeros(B, dtype=torch.bool, device=dev)
        self._steps = np.zeros(B, dtype=np.int64)     # host mirror of step_count
        self._upload(None)
        self.reset()

    # ---- the batch and its per-node state -------------------------------------------------------------------------------
    def _upload(self, node_map):
        """(re)build the batch CSR from self._graphs and upload it; per-node state is new (node_map None) or gathered from the old
        arrays by one index map (new node -> old node)."""
        h = build_batch_csr(self._graphs)
        dev, m = self.device, self.episode_length_multiplier
        up = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
        self.ptr, self._rowptr, self._col, self._w = up(h["ptr"]), up(h["rowptr"]), up(h["col"]), up(h["w"])
        self._wtot, self.edge_index, self.edge_weight = up(h["wtot"]), up(h["edge_index"]), up(h["edge_weight"])
        self.degrees, self.num_nodes = up(h["degrees"]), up(h["num_nodes"])
        self.total_weight = self._wtot[:, 0]
        self.max_steps = self.num_nodes * m
        self._num_nodes_host, self._max_steps_host = h["num_nodes"], h["num_nodes"] * m
        self._ptr_host = h["ptr"]
        self._max_nodes = int(h["num_nodes"].max()) if self.num_envs else 0
        total = int(h["ptr"][-1])
        self.batch = torch.repeat_interleave(torch.arange(self.num_envs, device=dev), self.num_nodes)
        if node_map is None:
            self.z = torch.ones(total, dtype=torch.int8, device=dev)
            self.delta_cache = torch.zeros(total, dtype=torch.float32, device=dev)
            self._last_flip = torch.zeros(total, dtype=torch.int32, device=dev)
            self.best_z = torch.ones(total, dtype=torch.int8, device=dev)
            self._basins = torch.zeros(m * total, dtype=torch.int64, device=dev)
            self.x = torch.zeros((total, NODE_FEATURE_DIM), dtype=torch.float32, device=dev)
            self.valid_mask = torch.ones(total, dtype=torch.bool, device=dev)
        else:
            idx = up(node_map)
            self.z, self.delta_cache, self._last_flip, self.best_z = self.z[idx], self.delta_cache[idx], self._last_flip[idx], self.best_z[idx]
            self.x, self.valid_mask = self.x[idx], self.valid_mask[idx]
            self._basins = self._basins[(idx[:, None] * m + torch.arange(m, device=dev)[None, :]).reshape(-1)]

    def _args(self):
        return (self.ptr, self._rowptr, self._col, self._w, self._wtot, self.z, self.delta_cache, self._last_flip, self.best_z,
                self._counters, self.current_cut, self.best_cut, self._tabu, self._hash, self._basins, self.x, self.valid_mask,
                self._max_nodes, self.tabu_tenure, self.episode_length_multiplier)

    @property
    def step_count(self):
        return self._counters[:, 0]

    @property
    def start_branch(self):
        """where each env's last reset took its spins from: 0 recorded z0, 1 random, 2 greedy from all-ones"""
        return self._counters[:, 3]

    def launch_plan(self):
        return launch_plan(self.num_envs, self._max_nodes)

    def _state(self):
        return {"x": self.x, "edge_index": self.edge_index, "valid_actions_mask": self.valid_mask, "batch": self.batch, "ptr": self.ptr}

    def get_valid_actions_mask(self):
        return self.valid_mask

    def _ids(self, ids):
        if ids is None:
            return None, None
        host = np.unique(_np(ids, np.int64).reshape(-1))
        if host.size and (host[0] < 0 or host[-1] >= self.num_envs):
            raise ValueError(f"ids outside [0, {self.num_envs})")
        return host, torch.from_numpy(host).to(self.device)

    # ---- env.py:46-74 ---------------------------------------------------------------------------------------------------
    def reset(self, ids=None, z0=None, greedy=None):
        """Reset the envs ``ids`` (all when None) in one launch -> state.  ``z0`` (test hook): recorded start spins, +-1 [sum N] (or a
        list with one array per env of the batch); ``greedy`` bool [B] (hook): True = greedy from all-ones, False = random spins;
        neither: a coin per env."""
        host, dev_ids = self._ids(ids)
        if z0 is not None:
            if isinstance(z0, (list, tuple)):
                z0 = np.concatenate([_np(a, np.int8).reshape(-1) for a in z0])
            z0 = torch.as_tensor(_np(z0, np.int8) if not isinstance(z0, torch.Tensor) else z0).to(self.device, torch.int8).contiguous()
        if greedy is not None:
            greedy = torch.as_tensor(greedy).to(self.device, torch.bool).reshape(self.num_envs).contiguous()
        _t.s2vppo_reset(*self._args(), dev_ids, z0, greedy, self._draw_seed, self.env_offset)
        if host is None:
            self._steps[:] = 0
        else:
            self._steps[host] = 0
        return self._state()

    # ---- env.py:140-195 -------------------------------------------------------------------------------------------------
    def step(self, actions):
        """actions int64 [B] on the device, LOCAL node ids -> (state, reward f64 [B], done bool [B], {'cut_value', 'best_cut'} f64 [B]):
        persistent tensors rewritten by every step."""
        if (self._steps >= self._max_steps_host).any():
            raise ValueError(f"envs {np.flatnonzero(self._steps >= self._max_steps_host).tolist()} are done: reset it first "
                             "(reset(ids) or set_graphs(ids, graphs))")
        if not (isinstance(actions, torch.Tensor) and actions.dtype == torch.int64 and actions.device == self.device):
            actions = torch.as_tensor(actions).to(self.device, torch.int64)
        _t.s2vppo_step(*self._args(), actions.reshape(self.num_envs), self.stag_punishment, self.reward, self.done)
        self._steps += 1
        return self._state(), self.reward, self.done, {"cut_value": self.current_cut, "best_cut": self.best_cut}

    def sync_steps(self):
        """Set the host mirror to the device's step counts (one host read): after replayed graphs or out-of-range actions."""
        self._steps[:] = self._counters[:, 0].cpu().numpy()
        return self._steps.copy()

    def count_steps(self, k: int):
        """Tell the host mirror that a replayed graph has made k more steps of every env."""
        self._steps += int(k)

    # ---- train_ddp.py:154-160: a done env gets a new graph ---------------------------------------------------------------
    def set_graphs(self, ids, graph_datas: Sequence[dict]):
        """Replace the graphs of the envs ``ids`` (any sizes) and reset those envs; every other env keeps its state.  The batch CSR,
        ``ptr``, ``batch`` and ``edge_index`` are rebuilt, per-node arrays re-laid by one index map (they are NEW tensors)."""
        ids = [int(i) for i in _np(ids, np.int64).reshape(-1)]
        if len(ids) != len(graph_datas) or len(set(ids)) != len(ids):
            raise ValueError("ids must be distinct and as many as graph_datas")
        if any(i < 0 or i >= self.num_envs for i in ids) or any(int(g["num_nodes"]) < 1 for g in graph_datas):
            raise ValueError(f"ids outside [0, {self.num_envs}) or a graph without nodes")
        old_ptr = self._ptr_host
        for i, g in zip(ids, graph_datas):
            self._graphs[i] = g
        parts = [np.zeros(int(self._graphs[i]["num_nodes"]), dtype=np.int64) if i in ids else np.arange(old_ptr[i], old_ptr[i + 1])
                 for i in range(self.num_envs)]
        self._upload(np.concatenate(parts))
        return self.reset(ids)


class EnvMaxcut:
    """The single env with the reference's names (S2V_PPO/env.py:8-206): a B = 1 view of VecEnvMaxcut.  The constructor resets;
    ``step(int)`` returns Python scalars (it reads the device once)."""

    def __init__(self, graph_data, config, env_offset: int = 0, seed: Optional[int] = None):
        self._vec = VecEnvMaxcut([graph_data], config, env_offset=env_offset, seed=seed)
        v = self._vec
        self.config, self.device = config, v.device
        self.num_nodes = int(graph_data["num_nodes"])
        self.max_steps = v.episode_length_multiplier * self.num_nodes
        self.tabu_tenure = v.tabu_tenure
        self.edge_index, self.edge_weight = v.edge_index, v.edge_weight
        self.total_weight = v.total_weight[0]
        self.max_possible_cut = self.total_weight
        self.degrees = v.degrees

    z = property(lambda self: self._vec.z)
    delta_cache = property(lambda self: self._vec.delta_cache)
    best_z = property(lambda self: self._vec.best_z)
    features_tensor = property(lambda self: self._vec.x)
    valid_mask = property(lambda self: self._vec.valid_mask)
    current_cut = property(lambda self: float(self._vec.current_cut[0]))
    best_cut = property(lambda self: float(self._vec.best_cut[0]))
    step_count = property(lambda self: int(self._vec._steps[0]))

    def _state(self):
        v = self._vec
        return {"x": v.x, "edge_index": v.edge_index, "valid_actions_mask": v.valid_mask}

    def reset(self, z0=None, greedy=None):
        self._vec.reset(z0=z0, greedy=None if greedy is None else [bool(greedy)])
        return self._state()

    def get_valid_actions_mask(self):
        return self._vec.valid_mask

    def step(self, action):
        v = self._vec
        if not 0 <= int(action) < self.num_nodes:
            raise IndexError(f"action {int(action)} outside [0, {self.num_nodes})")
        _, reward, done, info = v.step(torch.tensor([int(action)], dtype=torch.int64, device=v.device))
        out = torch.stack([reward[0], info["cut_value"][0], info["best_cut"][0], done[0].double()]).tolist()       # the one device read
        return self._state(), out[0], bool(out[3]), {"cut_value": out[1], "best_cut": out[2]}
