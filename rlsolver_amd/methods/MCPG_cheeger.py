"""Cheeger-cut family of the upstream MCPG package -- drop-in for rlsolver/methods/MCPG/sampling.py:181-250
(mcpg_sampling_rcheegercut, mcpg_sampling_ncheegercut) and :7-20 (sample_initializer), on HIP tensors.  The data are those of the
weighted MaxCut loader (dataloader.py:53-103: the family shares maxcut_dataloader).

    metro_sampling -> cut = (W - sum_e s_u s_v) / 2 (the edge sum UNWEIGHTED, as the reference has it), size = sum_v x_v,
    h = cut / min(size, N - size)  |  cut (1 / size + 1 / (N - size))
    -> num_ls node-sequential passes: flip a node unless h < h' or the smaller side would be empty -> best of the repeats.

The walk is the package's metro walk (methods/MCPG.py); everything after it is ONE kernel (include/rlsolver_hip.h:
rls_cheeger_local_search), lane = chain, on a flat visit stream in visiting order; best of repeats, merge and get_return are
the kernels the MaxCut family uses, with ``expected := 2 h`` and ``num_edges := 0`` (rls_mcpg_pick_best's (0 - 2 h) / 2 is -h
exactly).  MCPGRound / run_mcpg accept the data object as they accept a MaxCut graph -- unsharded: the values are fractions.

The rule draws nothing.  h holds NaN only where nothing has been swept (num_ls = 0, an empty side: 0 / 0); with n >= 2 the first
visit of such a chain always flips.  rls_mcpg_pick_best keeps the first strict minimum of the repeats, which is torch.argmin
for every value but NaN.  On signed weights +-inf can survive a sweep (-inf < h' keeps it), as in the reference.

Shapes follow the reference: chains node-major f32 [N, C] holding 0|1; a sampler returns
(-h[best] f32 [M], best 0|1 f32 [N, M], raw samples f32 [N, C], h - mean(h) f32 [C])."""
from __future__ import annotations

import ctypes as C
import types
from typing import Optional

import numpy as np
import torch
from torch.distributions.bernoulli import Bernoulli

from .. import _abi, ops_mcpg_tsp as mops
from ..graph import read_edge_arrays
from ..ops_mcpg_tsp import PackedChains
from . import MCPG_maxcut
from .MCPG import build_cheeger_stream, metro_sampling

TEN = torch.Tensor
CHEEGER_PROBLEMS = ("rcheegercut", "ncheegercut")


def supported_limit() -> int:
    """Largest node count the sampler covers (rls_cheeger_local_search_supported: the 64-chain tile in LDS)."""
    n = C.c_int64(0)
    _abi.lib().rls_cheeger_local_search_supported(1, 0, 0, C.byref(n))
    return int(n.value)


class Data_Cheeger(types.SimpleNamespace):
    """What MCPG_maxcut.make_data builds (edge_index, edge_attr, edge_weight_sum, weighted_degree, sorted_degree_nodes, graph: the
    neighbour rows with multiplicity) + ``device``, ``normalized`` (which of the two cuts the round hooks compute) and the visit
    stream, built on first use and again when ``sorted_degree_nodes`` has been replaced.

    For MCPGRound / run_mcpg the object stands where a MaxCut graph stands: ``round_local_search`` hands back expected = 2 h,
    ``num_edges`` is 0 (the edge count is ``num_graph_edges``) and ``value_scale`` 0.5, so that the round's best-of-repeats
    value (num_edges - expected) / 2 is -h and its value h - mean(h), both exactly (doubling commutes with float32 rounding)."""

    value_scale = 0.5
    fractional_values = True      # MCPGRound: no integer MAXLOC key exists for these values, a sharded round is refused

    def stream(self) -> TEN:
        """The visit stream on the device for the current ``sorted_degree_nodes``."""
        order = np.ascontiguousarray(torch.as_tensor(self.sorted_degree_nodes).cpu().numpy(), dtype=np.int64)
        if self._stream is None or not np.array_equal(self._stream[0], order):
            self._stream = (order, torch.from_numpy(build_cheeger_stream(self.graph.csr, order)).to(self.device))
        return self._stream[1]

    def local_search(self, xs: PackedChains, num_ls: int, normalized: Optional[bool] = None, out=None, num_chains: Optional[int] = None,
                     want_cut_size: bool = True):
        """Sweep + score on bit-packed chains: (chains after the sweep, h f32 [C], cut f32 [C], size f32 [C])."""
        nrm = self.normalized if normalized is None else normalized
        return mops.mcpg_cheeger_local_search(self.graph, xs, self.stream(), nrm, num_ls, self.edge_weight_sum, out=out,
                                              num_chains=num_chains, want_cut_size=want_cut_size)

    def round_local_search(self, samples: PackedChains, num_ls: int, seed: int, out: PackedChains, chain_ids):
        """What MCPGRound calls in place of the MaxCut kernel: (chains, 2 h).  Nothing is drawn: seed and chain_ids are unused."""
        xs, h, _, _ = self.local_search(samples, num_ls, out=out, want_cut_size=False)
        return xs, h * 2

    def result(self, xs) -> TEN:
        """-h f32 [C] of chains (f32 [N, C] or PackedChains) -- the incumbents' values run_mcpg starts from.  NaN where a side is
        empty (nothing is swept here)."""
        packed = xs if isinstance(xs, PackedChains) else PackedChains.pack(xs.to(self.device, torch.float32).contiguous())
        _, h, _, _ = self.local_search(packed, 0, out=PackedChains.empty(packed.num_nodes, packed.num_chains, self.device),
                                       want_cut_size=False)
        return -h


def make_data(num_nodes: int, eu, ev, w, device, sorted_degree_nodes=None, normalized: bool = False) -> Data_Cheeger:
    """The data object of a graph given as edge arrays (0-based endpoints, integer weights), on MCPG_maxcut.make_data: the same
    neighbour rows, weighted_degree, edge_weight_sum and sorted_degree_nodes.  Raises ValueError naming the limit for a graph
    outside the kernel's range (rls_cheeger_local_search_supported)."""
    num_nodes = int(num_nodes)
    wabs = int(np.abs(np.asarray(w).astype(np.int64)).sum()) if len(w) else 0
    E = int(np.asarray(eu).shape[0])
    max_n = C.c_int64(0)
    if not _abi.lib().rls_cheeger_local_search_supported(num_nodes, E, wabs, C.byref(max_n)):
        raise ValueError(f"the Cheeger sampler covers 1 <= num_nodes <= {int(max_n.value)} (the 64-chain tile in LDS) and "
                         f"|weights| sum + 2 E < 2^24 (exact float32); got num_nodes={num_nodes}, E={E}, |weights| sum={wabs}")
    base = MCPG_maxcut.make_data(num_nodes, eu, ev, w, device, sorted_degree_nodes)
    data = Data_Cheeger(**vars(base))
    data.device = torch.device(device)
    data.num_graph_edges, data.num_edges = base.num_edges, 0
    data.normalized = bool(normalized)
    data._stream = None
    data.stream()
    return data


def cheeger_dataloader(path, device, normalized: bool = False):
    """dataloader.py:53-103 for the two Cheeger problems: returns (Data_Cheeger, num_nodes)."""
    num_nodes, eu, ev, w = read_edge_arrays(path)
    return make_data(num_nodes, eu, ev, w, device, normalized=normalized), num_nodes


def _is_cheeger(problem) -> bool:
    return getattr(problem, "value", problem) in CHEEGER_PROBLEMS


def sample_initializer(problem, probs: TEN, config, device=None, data=None) -> TEN:
    """sampling.py:7-20 -> start chains f32 [N, total_mcmc_num * repeat_times].  The two Cheeger problems start from one-hot
    chains: chain i < min(M, N) holds the single node sorted_degree_nodes[-M:][i] (the M nodes of smallest degree; with M > N
    the chains past N stay empty), repeated repeat_times.  Every other problem draws Bernoulli(probs) (torch's generator).
    ``problem``: a Problem-like enum (matched by .value) or the plain string."""
    if device is None:
        device = data.device if data is not None and hasattr(data, "device") else probs.device
    M, R = int(config.total_mcmc_num), int(config.repeat_times)
    if _is_cheeger(problem):
        samples = torch.zeros(M, data.num_nodes)
        index = torch.as_tensor(data.sorted_degree_nodes).cpu()[-M:]
        k = min(len(index), M)
        samples[torch.arange(k), index[:k].long()] = 1
        return samples.repeat(R, 1).t().contiguous().to(device)
    samples = Bernoulli(probs).sample([M * R])
    return samples.detach().to(device).t()


def cheeger_value(h: TEN) -> TEN:
    """h - mean(h) as the reference forms it (sampling.py:214, :250): its tensors live on the CPU, so the mean is torch's CPU
    reduction, and h is not made of integers -- a device reduction adds in another order and lands an ulp away.  The C values
    cross to the host and back; the round (MCPGRound) keeps its own mean on the device."""
    hc = h.detach().cpu()
    return (hc - torch.mean(hc)).to(h.device)


def sampler_cheeger_packed(data: Data_Cheeger, xs: PackedChains, num_ls: int, total_mcmc_num: int, repeat_times: int,
                           normalized: Optional[bool] = None, num_chains: Optional[int] = None, in_place: bool = True):
    """Sweep, score and best of repeats on bit-packed chains.  Returns (-h[best] f32 [M], best PackedChains of M chains, value
    f32 [C] = h - mean(h), chains after the sweep)."""
    Cc = xs.num_chains if num_chains is None else num_chains
    out = xs if (in_place and xs.num_chains == Cc) else PackedChains.empty(xs.num_nodes, Cc, xs.device)
    xs_loc, h, _, _ = data.local_search(xs, num_ls, normalized, out=out, num_chains=Cc, want_cut_size=False)
    _, best_val, best = mops.mcpg_pick_best(h * 2, xs_loc, total_mcmc_num, repeat_times, 0)
    return best_val, best, cheeger_value(h), xs_loc


def _sampling(data, normalized, start_result, probs, num_ls, change_times, total_mcmc_num, device, index, u):
    device = data.device if device is None else torch.device(device)
    raw = metro_sampling(probs, start_result.to(device), change_times, device, index=index, u=u)
    Cc = raw.shape[1]
    xs_loc, h, _, _ = data.local_search(PackedChains.pack(raw), num_ls, normalized, want_cut_size=False)
    _, best_val, best = mops.mcpg_pick_best(h * 2, xs_loc, total_mcmc_num, Cc // total_mcmc_num, 0)
    return best_val, best, raw, cheeger_value(h)


def mcpg_sampling_rcheegercut(data: Data_Cheeger, start_result: TEN, probs: TEN, num_ls: int, change_times: int, total_mcmc_num: int,
                              device=None, index: Optional[TEN] = None, u: Optional[TEN] = None):
    """sampling.py:181-214, the ratio cut h = cut / min(size, N - size).  ``index`` / ``u`` replace the walk's torch.randint /
    torch.rand draws (test hooks).  NaN in h exists only with num_ls = 0; the best of the repeats is then the first strict
    minimum, where torch.argmin would pick the NaN."""
    return _sampling(data, False, start_result, probs, num_ls, change_times, total_mcmc_num, device, index, u)


def mcpg_sampling_ncheegercut(data: Data_Cheeger, start_result: TEN, probs: TEN, num_ls: int, change_times: int, total_mcmc_num: int,
                              device=None, index: Optional[TEN] = None, u: Optional[TEN] = None):
    """sampling.py:217-250, the normalised cut h = cut (1 / size + 1 / (N - size)); otherwise as mcpg_sampling_rcheegercut."""
    return _sampling(data, True, start_result, probs, num_ls, change_times, total_mcmc_num, device, index, u)
