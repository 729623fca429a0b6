"""ISCO_MIS -- drop-in for rlsolver/envs/env_ISCO.py:93-174 (the maximum-independent-set ISCO sampler).

``step`` is ONE kernel (rls_isco_mis_step): ISCO_maxcut's step with the energy of env_ISCO.py:162-170,
    energy_x[b]          = (sum_i x_i - lam * pairs(x_b)) / T,   pairs = edge-list entries with both ends in the set
    score_change_x[b, i] = (1 - 2 x_i) * dE/dx_i / 2 = (1 - 2 x_i) (1 - lam * cnt_i) / (2T),   cnt_i = set neighbours of i
in closed form (the reference gets them from ``vmap(model)`` + ``autograd.grad``, :134-146).  The edge list counts as given:
a duplicated line twice, a loop (u, u) once in ``pairs`` and twice in ``cnt_u``.  Samples keep the reference's dtype / shape
(float32 0/1, [B, N]).  ``get_local_dist`` and ``model`` are composed from the MaxCut ops -- a second implementation beside
the fused kernel:  with gain_i = same - differing row entries (K3) and deg_i the row length,
    cnt_i = (deg_i + gain_i) / 2 if x_i else (deg_i - gain_i) / 2.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops
from ..graph import build_csr
from ..ops import _check, _s64, _t
from ..seeding import Sharded
from .env_ISCO_maxcut import ISCO_maxcut


class ISCO_MIS(Sharded):
    def __init__(self, params_dict, batch_size: int = 1, device=None, chain_length: int = 20000,
                 init_temperature: float = 1.0, final_temperature: float = 0.0, lam: float = 1.001, env_offset: int = 0,
                 seed: Optional[int] = None):
        """``lam``: the reference's LAMADA (methods/ISCO/config_MIS.py).  ``env_offset`` / ``seed``: rlsolver_amd/seeding.py."""
        self._init_shard(env_offset, seed)
        self.edge_from = params_dict['edge_from']
        self.edge_to = params_dict['edge_to']
        self.device = torch.device(device) if device is not None else self.edge_from.device
        if self.device.type != 'cuda':
            raise TypeError(f"rlsolver_amd.ISCO_MIS needs a HIP device (got {self.device}); there is no CPU path")
        self.batch_size = batch_size
        self.chain_length = chain_length
        self.init_temperature = torch.tensor(init_temperature, device=self.device)
        self.final_temperature = torch.tensor(final_temperature, device=self.device)
        self.max_num_nodes = params_dict['num_nodes']
        self.num_edges = params_dict['num_edges']
        self.lam = float(lam)
        eu = self.edge_from.detach().cpu().numpy().astype(np.int64)
        ev = self.edge_to.detach().cpu().numpy().astype(np.int64)
        # rows as ISCO_maxcut builds them: one entry per end of every line, a loop listed twice in its row
        csr = build_csr((eu, ev, np.ones_like(eu)), num_nodes=self.max_num_nodes, if_bidirectional=False, keep_loops=True)
        self.graph = ops.DeviceGraph(csr, self.device)
        self._deg = torch.from_numpy(np.diff(csr.rowptr).astype(np.int32)).to(self.device)

    # env_ISCO.py:106-109 and the scratch of rows past the LDS: the same samples, the same rows (rls_isco_maxcut_scratch_bytes)
    random_gen_init_sample = ISCO_maxcut.random_gen_init_sample
    _step_scratch = ISCO_maxcut._step_scratch
    launch_plan = ISCO_maxcut.launch_plan

    def step(self, x, path_length, temperature, draws: Optional[dict] = None, want_terms: bool = False):
        """env_ISCO.py:111-119 -> (y f32 [B, N], ll_y * temperature f32 [B], acceptance probability f32 [B]).

        ``draws`` / ``want_terms``: the hooks of ISCO_maxcut.step (the two torch.rand draws; terms f32 [B, 5] = ll_x, ll_x2y,
        ll_y, ll_y2x, log_acc and mask bool [B, N])."""
        x = _check(x.contiguous(), "x", (torch.float32,), self.device)
        B, N = x.shape
        if N != self.max_num_nodes:
            raise ValueError(f"x must be [B, {self.max_num_nodes}]")
        pl = torch.as_tensor(path_length, device=self.device).to(torch.int64).expand(B).contiguous()
        y = torch.empty_like(x)
        energy = torch.empty(B, dtype=torch.float32, device=self.device)
        acc = torch.empty(B, dtype=torch.float32, device=self.device)
        terms = torch.empty((B, 5), dtype=torch.float32, device=self.device) if want_terms else None
        mask = torch.empty((B, N), dtype=torch.bool, device=self.device) if want_terms else None
        ug = ua = None
        if draws is not None:
            ug = _check(draws["u_gumbel"].to(self.device).contiguous(), "u_gumbel", (torch.float32,), self.device, (B, N))
            ua = _check(draws["u_accept"].to(self.device).contiguous(), "u_accept", (torch.float32,), self.device, (B,))
        _t.isco_mis_step(self.graph.handle, x, y, pl, float(temperature), self.lam, ug, ua,
                         _s64(0 if draws is not None else self._next_seed()), self.env_offset, energy, acc, terms, mask,
                         self._step_scratch(B))
        if want_terms:
            return y, energy, acc, terms, mask
        return y, energy, acc

    def _set_neighbours(self, xb):
        """cnt int32 [B, N]: row entries of node i whose other end is in the set (a loop: two entries)."""
        gain = ops.maxcut_delta_all(self.graph, xb)
        return torch.where(xb, self._deg + gain, self._deg - gain) // 2

    def get_local_dist(self, sample, temperature):
        """env_ISCO.py:134-146 -> (energy f32 [B], log_prob f32 [B, N])."""
        xb = (sample > 0).contiguous()
        t = float(temperature)
        cnt = self._set_neighbours(xb)
        sign = 1.0 - 2.0 * xb.to(torch.float32)
        score_change_x = sign * (1.0 - self.lam * cnt.to(torch.float32)) / (2.0 * t)
        return self._energy(xb, cnt, t), torch.log_softmax(score_change_x, dim=-1)

    def _energy(self, xb, cnt, t):
        ones = xb.sum(dim=-1)
        pairs = (cnt * xb).sum(dim=-1) // 2
        return (ones.to(torch.float32) - self.lam * pairs.to(torch.float32)) / t

    def model(self, x, temperature):
        """energy of a batch (the reference vmaps a per-sample version, env_ISCO.py:162-170)."""
        xb = (x > 0).contiguous()
        if xb.dim() == 1:
            xb = xb[None, :]
        return self._energy(xb, self._set_neighbours(xb), float(temperature))
