"""Edge-flip MaxCut sampler of the upstream MCPG package -- drop-in for rlsolver/methods/MCPG/sampling.py:130-178
(mcpg_sampling_maxcut_edge) and the edge part of its loader rlsolver/methods/MCPG/dataloader.py:87-101 (the ``add`` table and the
edge order) and :125-153 (the per-edge neighbour rows), on HIP tensors.

    metro_sampling -> gauge fix (every chain XORed with its value at the node of largest |weighted degree|, :142-145)
    -> num_ls edge-sequential passes: at edge (r, c), with t_r / t_c the weighted sums over the other neighbours of r / c,
       a = t_r + U0 / 10 + add0,  b = t_c + U1 / 10 + add1,  z = a + b + U2 / 10 - add2;  (x_r, x_c) <- the first maximum of
       (z, a, b, 0) as two bits (:152-168; a node holds -0.5 | 1.5 until its first write)
    -> sum_e w_e (2 x_u - 1)(2 x_v - 1), best of the repeats per kept chain.

The walk is the package's metro walk (methods/MCPG.py); everything after it is ONE kernel (include/rlsolver_hip.h:
rls_maxcut_edge_local_search), lane = chain, on a flat visit stream in visiting order (methods/MCPG.py: build_edge_stream); best of
repeats, merge and get_return are the kernels the MaxCut family uses, with ``num_edges := edge_weight_sum`` (rls_mcpg_pick_best's
(num_edges - expected) / 2 is then the cut).  MCPGRound / run_mcpg accept the data object as they accept a MaxCut graph, sharded
or not: the values are integers or half-integers and every draw is keyed by the chain's global id.

Integer edge weights.  The reference's edge order comes from an unstable argsort; here it is the stable one (descending in
|w_e| (A_r + A_c), A = sum of |w| at a node) unless the caller brings an order, as for the nodes.  The reference runs one pass
with num_ls = 0 (its loop tests after the body); the reference-shaped sampler here does the same, the kernel and the round take
num_ls as the number of passes.

Shapes follow the reference: chains node-major f32 [N, C]; a sampler returns ((edge_weight_sum - expected[best]) / 2 f32 [M], best
f32 [N, M] holding 0 | 1 -- and -0.5 | 1.5 at a node no edge touches --, raw samples f32 [N, C], expected - mean f32 [C])."""
from __future__ import annotations

import ctypes as C
import types
from typing import Optional

import numpy as np
import torch

from .. import _abi, ops_mcpg_tsp as mops
from ..graph import read_edge_arrays
from ..ops_mcpg_tsp import PackedChains
from . import MCPG_maxcut
from .MCPG import _seed_from_torch, build_edge_stream, metro_sampling

TEN = torch.Tensor


def supported_limit() -> int:
    """Largest node count the sampler covers (rls_maxcut_edge_local_search_supported: the 64-chain tile and its bitmap in LDS)."""
    n = C.c_int64(0)
    _abi.lib().rls_maxcut_edge_local_search_supported(1, 0, 0, 0, 0, C.byref(n))
    return int(n.value)


def edge_tables(num_nodes: int, eu, ev, w, sorted_degree_edges=None):
    """The loader's edge tables in numpy (dataloader.py:87-101): (add f32 [3, E], sorted_degree_edges int64 [E], key int64 [E],
    max_abs_degree, weight_abs_sum).
        add[0][e] = (-Wdeg_r / 2 + w_e) - 0.05f,  add[1][e] = (-Wdeg_c / 2 + w_e) - 0.05f,  add[2][e] = w_e + 0.05f   (float32)
        key[e] = |w_e| (A_r + A_c), A = sum of |w| at a node; the order is its stable descending argsort unless given."""
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    w = np.asarray(w)
    if np.any(w != np.round(w)):
        raise ValueError("the edge-flip MaxCut sampler takes integer edge weights")
    wi = w.astype(np.int64)
    E = int(eu.shape[0])
    wdeg = np.zeros(num_nodes, np.int64)
    adeg = np.zeros(num_nodes, np.int64)
    for ends in (eu, ev):
        np.add.at(wdeg, ends, wi)
        np.add.at(adeg, ends, np.abs(wi))
    wf = wi.astype(np.float32)
    c05 = np.float32(0.05)
    add = np.stack([((-wdeg[eu] / 2).astype(np.float32) + wf) - c05, ((-wdeg[ev] / 2).astype(np.float32) + wf) - c05, wf + c05]) \
        if E else np.zeros((3, 0), np.float32)
    key = np.abs(wi) * (adeg[eu] + adeg[ev])
    if sorted_degree_edges is None:   # torch.argsort(descending=True) is not stable; any tie order is a valid reference outcome
        order = torch.argsort(torch.from_numpy(key), descending=True, stable=True).numpy()
    else:
        order = np.asarray(torch.as_tensor(sorted_degree_edges).cpu().numpy(), dtype=np.int64)
    return add.astype(np.float32), order, key, int(adeg.max()) if num_nodes else 0, int(np.abs(wi).sum())


def check_limits(num_nodes: int, E: int, max_abs_degree: int, weight_abs_sum: int, stream_len: int) -> None:
    """ValueError naming the limit for a graph outside the kernel's range (rls_maxcut_edge_local_search_supported)."""
    max_n = C.c_int64(0)
    if not _abi.lib().rls_maxcut_edge_local_search_supported(int(num_nodes), int(E), int(max_abs_degree), int(weight_abs_sum),
                                                             int(stream_len), C.byref(max_n)):
        raise ValueError(f"the edge-flip MaxCut sampler covers 1 <= num_nodes <= {int(max_n.value)} (the 64-chain tile and its bitmap in "
                         f"LDS), 3 max |weighted degree| < 2^24 and |weights| sum < 2^24 (exact float32) and a visit stream below 2^31 "
                         f"words; got num_nodes={num_nodes}, E={E}, max |weighted degree|={max_abs_degree}, |weights| sum={weight_abs_sum}, "
                         f"stream of {stream_len} words")


def stream_words(num_nodes: int, eu, ev) -> int:
    """Length of the visit stream: 7 words per edge and two per entry of both rows less the removed ones."""
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    deg = np.bincount(np.concatenate([eu, ev]), minlength=num_nodes)
    return int(7 * eu.shape[0] + 2 * (deg[eu] + deg[ev] - 2).sum())


class Data_MaxCutEdge(types.SimpleNamespace):
    """What MCPG_maxcut.make_data builds (edge_index, edge_attr, edge_weight_sum, weighted_degree, sorted_degree_nodes, graph) +
    ``device``, ``add`` f32 [3, E], ``sorted_degree_edges`` and the visit stream, built on first use and again when either order
    has been replaced.

    For MCPGRound / run_mcpg the object stands where a MaxCut graph stands: ``round_local_search`` hands back (chains, expected),
    ``num_edges`` is int(edge_weight_sum) (the edge count is ``num_graph_edges``), so the round's best-of-repeats value
    (num_edges - expected) / 2 is the cut."""

    def stream(self) -> TEN:
        """The visit stream on the device for the current ``sorted_degree_edges``."""
        order = np.ascontiguousarray(torch.as_tensor(self.sorted_degree_edges).cpu().numpy(), dtype=np.int64)
        if self._stream is None or not np.array_equal(self._stream[0], order):
            eu, ev = self._edges
            self._stream = (order, torch.from_numpy(build_edge_stream(self.num_nodes, eu, ev, self._weights, order, self._add_np)).to(self.device))
        return self._stream[1]

    def hub(self) -> int:
        """The gauge node: sorted_degree_nodes[0] as it stands now."""
        return int(torch.as_tensor(self.sorted_degree_nodes)[0])

    def local_search(self, xs: PackedChains, num_ls: int, uniforms: Optional[TEN] = None, seed: int = 0, out=None,
                     num_chains: Optional[int] = None, chain_ids=None, gauge: bool = True):
        """Gauge fix + sweep + score on bit-packed chains: (chains after the sweep, expected f32 [C])."""
        return mops.mcpg_maxcut_edge_local_search(self.graph, self._edge_w, xs, self.stream(), self.max_abs_degree, self.weight_abs_sum,
                                                  num_ls, self.hub() if gauge else -1, uniforms, seed, out=out, num_chains=num_chains,
                                                  chain_ids=chain_ids)

    def round_local_search(self, samples: PackedChains, num_ls: int, seed: int, out: PackedChains, chain_ids):
        """What MCPGRound calls in place of the MaxCut kernel: (chains, expected)."""
        return self.local_search(samples, num_ls, None, seed, out=out, chain_ids=chain_ids)

    def result(self, xs) -> TEN:
        """Cut value f32 [C] of chains (f32 [N, C] or PackedChains) -- the incumbents' values run_mcpg starts from."""
        packed = xs if isinstance(xs, PackedChains) else PackedChains.pack(xs.to(self.device, torch.float32).contiguous())
        _, expected = self.local_search(packed, 0, out=PackedChains.empty(packed.num_nodes, packed.num_chains, self.device), gauge=False)
        return (self.edge_weight_sum - expected) / 2


def make_data(num_nodes: int, eu, ev, w, device, sorted_degree_nodes=None, sorted_degree_edges=None) -> Data_MaxCutEdge:
    """The data object of a graph given as edge arrays (0-based endpoints, integer weights), on MCPG_maxcut.make_data: the same
    neighbour rows, weighted_degree, edge_weight_sum and sorted_degree_nodes, + the loader's ``add`` table, its edge order (stable;
    or the caller's) and the visit stream.  Raises ValueError naming the limit for a graph outside the kernel's range."""
    num_nodes = int(num_nodes)
    add, order, _, max_abs_degree, weight_abs_sum = edge_tables(num_nodes, eu, ev, w, sorted_degree_edges)
    E = int(np.asarray(eu).shape[0])
    check_limits(num_nodes, E, max_abs_degree, weight_abs_sum, stream_words(num_nodes, eu, ev))
    base = MCPG_maxcut.make_data(num_nodes, eu, ev, w, device, sorted_degree_nodes)
    data = Data_MaxCutEdge(**vars(base))
    data.device = torch.device(device)
    data.num_graph_edges, data.num_edges = base.num_edges, int(base.edge_weight_sum)
    data.max_abs_degree, data.weight_abs_sum = max_abs_degree, weight_abs_sum
    data._edges = (np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64))
    data._weights = np.asarray(w).astype(np.int64)
    data._add_np = add
    data.add = torch.from_numpy(add).to(data.device)
    data.sorted_degree_edges = torch.from_numpy(order.copy()).to(torch.int64)
    data._stream = None
    data.stream()
    return data


def maxcut_edge_dataloader(path, device):
    """dataloader.py:53-160 for Problem.maxcut_edge: returns (Data_MaxCutEdge, num_nodes)."""
    num_nodes, eu, ev, w = read_edge_arrays(path)
    return make_data(num_nodes, eu, ev, w, device), num_nodes


def value_of(expected: TEN) -> TEN:
    """expected - mean(expected) as the reference forms it (sampling.py:178: the exact sum of the integers divided by the count,
    rounded once).  A float32 device mean multiplies by a rounded 1 / C and lands an ulp away where C is no power of two; the
    quotient is taken in float64 instead, whose error is far below the distance of sum / C from any float32 rounding boundary
    (|sum| < 2^24: sum / C is either a float32 itself or at least 2^-28 of its size away from a midpoint)."""
    return expected - (expected.sum(dtype=torch.float64) / expected.shape[0]).to(torch.float32)


def sampler_maxcut_edge_packed(data: Data_MaxCutEdge, xs: PackedChains, num_ls: int, total_mcmc_num: int, repeat_times: int,
                               seed: int = 0, uniforms: Optional[TEN] = None, num_chains: Optional[int] = None, in_place: bool = True,
                               chain_ids=None):
    """Gauge fix, sweep, score and best of repeats on bit-packed chains.  Returns (cut of the best repeats f32 [M], best
    PackedChains of M chains, value f32 [C] = expected - mean, chains after the sweep)."""
    Cc = xs.num_chains if num_chains is None else num_chains
    out = xs if (in_place and xs.num_chains == Cc) else PackedChains.empty(xs.num_nodes, Cc, xs.device)
    xs_loc, expected = data.local_search(xs, num_ls, uniforms, seed, out=out, num_chains=Cc, chain_ids=chain_ids)
    _, best_val, best = mops.mcpg_pick_best(expected, xs_loc, total_mcmc_num, repeat_times, data.num_edges)
    return best_val, best, value_of(expected), xs_loc


def mcpg_sampling_maxcut_edge(data: Data_MaxCutEdge, start_result: TEN, probs: TEN, num_ls: int, change_times: int, total_mcmc_num: int,
                              device=None, index: Optional[TEN] = None, u: Optional[TEN] = None, uniforms: Optional[TEN] = None):
    """sampling.py:130-178 -> ((edge_weight_sum - best expected) / 2 f32 [M], chains of the best repeats f32 [N, M], the metro
    output f32 [N, C], expected - mean f32 [C]).  ``index`` / ``u`` / ``uniforms`` replace the torch draws of the walk and of the
    sweep (test hooks; uniforms f32 [passes, E, 3, C]).  The reference's loop tests num_ls after the body: num_ls = 0 runs one pass."""
    device = data.device if device is None else torch.device(device)
    raw = metro_sampling(probs, start_result.to(device), change_times, device, index=index, u=u)
    Cc = raw.shape[1]
    passes = max(1, int(num_ls))
    xs_loc, expected = data.local_search(PackedChains.pack(raw), passes, uniforms, 0 if uniforms is not None else _seed_from_torch())
    best_index, _, _ = mops.mcpg_pick_best(expected, PackedChains.pack(xs_loc), total_mcmc_num, Cc // total_mcmc_num, data.num_edges)
    res = (data.edge_weight_sum - expected[best_index]) / 2
    return res, xs_loc[:, best_index], raw, value_of(expected)
