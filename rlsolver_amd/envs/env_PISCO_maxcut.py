"""PISCO_maxcut -- drop-in for rlsolver/envs/env_ISCO.py:365-448 (the dense, weighted MaxCut ISCO sampler; driver
methods/ISCO/main_PISCO_maxcut.py, loader methods/ISCO/util_maxcut.py).

The graph is an f16 adjacency matrix A [Np, Np] with the weights in it, symmetric, zero-padded from n to Np = ceil(n / 8) * 8
nodes.  With delta = 2x - 1 and r = delta . A (ONE product on the f16 matrix cores, rls_pisco_product):
    energy_x[b]          = -0.25 * sum_k r_k delta_k / T          (= (cut(x_b) - sum(A) / 4) / T)
    score_change_x[b, k] = (1 - 2 x_k) * dE/dx_k / 2 = delta_k r_k / (2T)
    log_prob             = log_softmax(score) over all Np columns: a padded column scores 0 and can be selected and flipped
``step`` is that product plus ONE kernel (rls_pisco_step): the proposal's row of r comes from a rank-L update with the selected
rows of A, not from a second product.  Samples keep the reference's dtype / shape (float16 0/1, [B, Np]).

``half_rounding=True`` is the reference's arithmetic: r and sum_k r_k delta_k are each rounded to f16 once (energies are
quantised in steps of 8 from |sum| = 8192 on).  ``False`` keeps everything in f32.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops
from ..ops import _check
from ..seeding import Sharded


def load_data(filename, device=None):
    """methods/ISCO/util_maxcut.py:7-46 without networkx -> {num_nodes, num_edges, edge_from, edge_to, adj_matrix}.

    What the reference's nx.Graph does with the file is read off util_maxcut.py:17-35 (networkx is not a dependency here):
    lines with ``//`` are comments; node ids are 1-based; weights are ``int``; ``Graph.add_edge`` overwrites, so a repeated or
    reversed line REPLACES the weight of its edge; a loop (u, u) sets A[u][u]; the matrix is symmetric, float16, zero-padded to
    a multiple of 8; ``edge_from`` / ``edge_to`` (int64) hold the distinct edges in first-seen order in arrays of the header's
    ``num_edges`` entries, zero-filled past them."""
    with open(filename, 'r') as f:
        lines = [[int(t) for t in ln.split()] for ln in f if '//' not in ln and ln.strip()]
    num_nodes, num_edges = lines[0][0], lines[0][1]
    weight = {}                                                  # (min, max) -> the LAST weight given for that edge
    # nx.Graph.edges() walks the nodes in the order they entered the graph (all are added up front, in id order) and, for each,
    # its neighbours in the order their edge was FIRST added, listing an edge under the endpoint it reaches first
    order = {}
    for item in lines[1:]:
        u, v = item[0] - 1, item[1] - 1
        weight[(min(u, v), max(u, v))] = item[2]
        order.setdefault(u, {}).setdefault(v, None)
        order.setdefault(v, {}).setdefault(u, None)
    A = np.zeros((num_nodes, num_nodes), np.float64)
    for (u, v), w in weight.items():
        A[u, v] = A[v, u] = w
    padded = (num_nodes + 7) // 8 * 8
    Ap = np.zeros((padded, padded), np.float16)
    Ap[:num_nodes, :num_nodes] = A.astype(np.float16)
    edge_from, edge_to = [0] * num_edges, [0] * num_edges
    i, seen = 0, set()
    for u in range(num_nodes):                                   # Graph.edges(): node by node, each undirected edge once
        for v in order.get(u, {}):
            if (v, u) in seen:
                continue
            seen.add((u, v))
            if i < num_edges:
                edge_from[i], edge_to[i] = u, v
            else:
                raise IndexError("list assignment index out of range")      # as the reference: more edges than the header says
            i += 1
    dev = torch.device(device) if device is not None else None
    return {'num_nodes': num_nodes, 'num_edges': num_edges,
            'edge_from': torch.tensor(edge_from, dtype=torch.int64, device=dev),
            'edge_to': torch.tensor(edge_to, dtype=torch.int64, device=dev),
            'adj_matrix': torch.from_numpy(Ap).to(dev) if dev is not None else torch.from_numpy(Ap)}


def record(pre_obj, pre_sample, new_obj, new_sample):
    """util_maxcut.py:48-53 without the host branch: the best energy so far and its sample stay on the device.

    The reference ASSIGNS the better row, so the driver may start from ``best_sample = zeros(num_nodes)`` (main_PISCO_maxcut.py:28)
    while the samples have Np = ceil(n / 8) * 8 columns.  Here the result always has the samples' width: a ``pre_sample`` of
    another length is zero-padded or cut to it first (the padded columns of a kept sample are part of it, as there)."""
    max_value, max_index = torch.max(new_obj, dim=0)
    width = new_sample.shape[-1]
    if pre_sample.shape[-1] < width:
        pre_sample = torch.nn.functional.pad(pre_sample, (0, width - pre_sample.shape[-1]))
    elif pre_sample.shape[-1] > width:
        pre_sample = pre_sample[..., :width]
    better = max_value > pre_obj
    return (torch.where(better, max_value.to(pre_obj.dtype), pre_obj),
            torch.where(better, new_sample[max_index], pre_sample.to(new_sample.dtype)))


class PISCO_maxcut(Sharded):
    def __init__(self, params_dict, batch_size: int = 1, device=None, chain_length: int = 200, init_temperature: float = 1.0,
                 final_temperature: float = 0.0, env_offset: int = 0, seed: Optional[int] = None, half_rounding: bool = True):
        """``params_dict``: the reference's (adj_matrix f16 [Np, Np], num_nodes, num_edges, edge_from, edge_to).
        ``env_offset`` / ``seed``: rlsolver_amd/seeding.py."""
        self._init_shard(env_offset, seed)
        A = params_dict['adj_matrix']
        self.device = torch.device(device) if device is not None else A.device
        if self.device.type != 'cuda':
            raise TypeError(f"rlsolver_amd.PISCO_maxcut needs a HIP device (got {self.device}); there is no CPU path")
        if A.dtype != torch.float16:
            raise TypeError(f"adj_matrix has dtype {A.dtype}, expected torch.float16")
        if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] == 0 or A.shape[0] % 8:
            raise ValueError(f"adj_matrix must be [Np, Np] with Np a positive multiple of 8, got {tuple(A.shape)}")
        if not torch.equal(A, A.t()):
            raise ValueError("adj_matrix must be symmetric (the closed-form gradient and the rank-L update assume it)")
        self.batch_size = batch_size
        self.chain_length = chain_length
        self.init_temperature = torch.tensor(init_temperature, device=self.device)
        self.final_temperature = torch.tensor(final_temperature, device=self.device)
        self.max_num_nodes = params_dict['num_nodes']
        self.num_edges = params_dict['num_edges']
        self.edge_from = params_dict['edge_from']
        self.edge_to = params_dict['edge_to']
        self.adj_matrix = A.to(self.device).contiguous()
        self.padded_num_nodes = int(A.shape[0])
        if not 0 < self.max_num_nodes <= self.padded_num_nodes:
            raise ValueError(f"num_nodes={self.max_num_nodes} does not fit adj_matrix {tuple(A.shape)}")
        self.sum_A = torch.sum(self.adj_matrix)                                # env_ISCO.py:377 (f16, as the reference keeps it)
        self.half_rounding = bool(half_rounding)
        self._scratch = None

    def random_gen_init_sample(self):
        """env_ISCO.py:379-382: Bernoulli(1/2) samples as float16 [B, n] (Philox kernel seeded from torch); the caller pads to
        Np columns, as main_PISCO_maxcut.py:23-24 does."""
        n = self.max_num_nodes
        bits = ops.rand_spins(self.batch_size, max(n, 2), self._next_seed(), self.device, env_offset=self.env_offset)[:, :n]
        bits = bits.clone()
        # no gauge fixing here: node 0 is a coin like the others (bit 1 of a second keyed draw)
        bits[:, 0] = ops.rand_spins(self.batch_size, 2, self._next_seed(), self.device, env_offset=self.env_offset)[:, 1]
        return bits.to(torch.float16)

    def _step_scratch(self, B: int):
        need = max(ops.pisco_scratch_bytes(self.padded_num_nodes, B), 16)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch

    def launch_plan(self, B: int) -> dict:
        """What ``step`` launches after the product for B samples on this device under the tuning knobs as they stand
        (rls_isco_launch_plan, dense: the launcher's own planner, csrc/rls_isco_plan.h)."""
        from .env_ISCO_maxcut import isco_launch_plan
        return isco_launch_plan(self.padded_num_nodes, B, torch.cuda.get_device_properties(self.device).multi_processor_count, True)

    def _sample(self, x, name="x"):
        x = _check(x.contiguous(), name, (torch.float16,), self.device)
        if x.dim() != 2 or x.shape[1] != self.padded_num_nodes:
            raise ValueError(f"{name} must be [B, {self.padded_num_nodes}] (padded to a multiple of 8 columns), got {tuple(x.shape)}")
        return x

    def step(self, x, path_length, temperature, draws: Optional[dict] = None, want_terms: bool = False):
        """env_ISCO.py:384-392 -> (y f16 [B, Np], ll_y * temperature f32 [B], acceptance probability f32 [B]).

        ``draws`` (test hook) = {"u_gumbel": f32 [B, Np], "u_accept": f32 [B]}, the reference's two torch.rand draws.
        ``want_terms`` additionally returns (terms f32 [B, 5] = ll_x, ll_x2y, ll_y, ll_y2x, log_acc; mask bool [B, Np])."""
        x = self._sample(x)
        B, Np = x.shape
        pl = torch.as_tensor(path_length, device=self.device).to(torch.int64).expand(B).contiguous()
        ug = ua = None
        if draws is not None:
            ug = _check(draws["u_gumbel"].to(self.device).contiguous(), "u_gumbel", (torch.float32,), self.device, (B, Np))
            ua = _check(draws["u_accept"].to(self.device).contiguous(), "u_accept", (torch.float32,), self.device, (B,))
        return ops.pisco_step(self.adj_matrix, x, pl, float(temperature), self.half_rounding, ug, ua,
                              0 if draws is not None else self._next_seed(), self.env_offset, want_terms, self._step_scratch(B))

    def _product(self, sample):
        r = ops.pisco_product(self.adj_matrix, self._sample(sample, "sample"))
        return r.to(torch.float16).to(torch.float32) if self.half_rounding else r

    def tensor_core_energy(self, sample, temperature):
        """env_ISCO.py:436-444 -> (energy f32 [B], grad f32 [B, Np]): -0.25 sum_k r_k delta_k / T and its gradient -r / T."""
        r = self._product(sample)
        # a device tensor: dividing by a host scalar multiplies by its reciprocal on the GPU, one ulp off the reference's division
        t = torch.as_tensor(temperature, dtype=torch.float32).to(self.device)
        delta = (sample > 0).to(torch.float32) * 2 - 1
        s = (r * delta).sum(dim=1)
        if self.half_rounding:
            s = s.to(torch.float16).to(torch.float32)
        return (-0.25 * s) / t, -r / t

    def get_local_dist(self, sample, temperature):
        """env_ISCO.py:407-416 -> (energy f32 [B], log_prob f32 [B, Np])."""
        energy_x, grad_x = self.tensor_core_energy(sample, temperature)
        delta_x = 1 - (sample > 0).to(torch.float32) * 2
        return energy_x, torch.log_softmax((delta_x * grad_x) / 2, dim=-1)

    def check_tensor(self, tensor):
        """env_ISCO.py:446-448"""
        if torch.isinf(tensor).any():
            raise ValueError(" contains inf values!")

    # ---- the pieces of a step as the reference exposes them.  ``step`` does not call them: they are composed from
    # get_local_dist (the product kernel) and torch ops, with torch's generator for the two draws -- a second implementation
    # beside the fused kernel, for callers that drive the pieces themselves.
    def proposal(self, x, path_length, temperature):
        """env_ISCO.py:394-405 -> (ll_x, y, trajectory)."""
        ll_x, log_prob = self.get_local_dist(x, temperature)
        perturbed = log_prob - torch.log(-torch.log(torch.rand(log_prob.shape, device=log_prob.device)))
        Np = log_prob.shape[-1]
        pl = torch.as_tensor(path_length, device=log_prob.device).to(torch.int64).expand(log_prob.shape[0])
        threshold = torch.gather(torch.sort(perturbed).values, 1, (Np - pl).unsqueeze(1))
        mask = (perturbed >= threshold).int()
        order = torch.argsort(-perturbed, dim=-1)
        ll_sorted = _renormalize(torch.gather(log_prob, -1, order))
        ll_selected = torch.zeros_like(ll_sorted).scatter_(1, order, ll_sorted) * mask
        y = x * (1 - mask) + mask * (1 - x)
        return ll_x, y, {'ll_x2y': ll_selected.sum(dim=-1), 'selected_idx': {'selected_mask': mask, 'perturbed_ll': perturbed}}

    def ll_y2x(self, forward_trajectory, y, temperature):
        """env_ISCO.py:418-430 -> (ll_y, ll_y2x)."""
        ll_y, log_prob = self.get_local_dist(y, temperature)
        mask = forward_trajectory['selected_idx']['selected_mask']
        back = torch.argsort(forward_trajectory['selected_idx']['perturbed_ll'], dim=-1)
        log_prob = torch.where(mask.bool(), log_prob, torch.full_like(log_prob, -1e18))
        ll_back = _renormalize(torch.gather(log_prob, -1, back))
        back_mask = torch.gather(mask, -1, back).bool()
        return ll_y, torch.where(back_mask, ll_back, torch.zeros_like(ll_back)).sum(dim=-1)

    def select_sample(self, log_acc, x, y):
        """env_ISCO.py:432-434 (mh_step, methods/ISCO/util.py:62-75)."""
        use = torch.log(torch.rand(log_acc.shape, device=log_acc.device) + 1e-24) < log_acc
        return torch.where(use.unsqueeze(-1), y, x)


def _renormalize(ll):
    """noreplacement_sampling_renormalize, methods/ISCO/util.py:7-17."""
    base = ll.max(dim=-1, keepdim=True).values
    p = torch.exp(ll - base)
    t = -torch.abs(torch.log(torch.cumsum(p, dim=-1) - p) + base)
    log1mexp = torch.where(t > -0.693, torch.log(-torch.expm1(t)), torch.log1p(-torch.exp(t)))
    return torch.clamp(ll - log1mexp, max=0.0)
