"""MaxSAT family of the upstream MCPG package -- drop-in for rlsolver/methods/MCPG/dataloader.py:163-275 (Data_MaxSAT,
maxsat_dataloader, sort_node) and sampling.py:253-285 (mcpg_sampling_maxsat), on HIP tensors.

The walk is the package's metro walk (methods/MCPG.py), the sweep and the score are ONE kernel
(include/rlsolver_hip.h: rls_maxsat_local_search) on a level schedule built by the host library from the clause list and
the visiting order; best of repeats, merge and get_return are the kernels the MaxCut family uses, with
``expected := -S`` and ``num_edges := K``.  MCPGRound / run_mcpg accept the data object as they accept a MaxCut graph.

Shapes follow the reference: chains node-major f32 [nvar, C] holding 0|1; the sampler returns
(max_res f32 [M], best 0|1 f32 [nvar, M], raw samples f32 [nvar, C], -(res - mean(res)) f32 [C])."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from .. import _abi, ops_mcpg_tsp as mops
from ..ops_mcpg_tsp import PackedChains
from ..seeding import seed_from_torch as _seed_from_torch
from .MCPG import metro_sampling

TEN = torch.Tensor


def supported_limits():
    """(largest nvar, largest sum of clause weights) the sampler covers (rls_maxsat_local_search_supported)."""
    nv, ws = C.c_int64(0), C.c_int64(0)
    _abi.lib().rls_maxsat_local_search_supported(1, 0, C.byref(nv), C.byref(ws))
    return int(nv.value), int(ws.value)


class Data_MaxSAT(object):
    """The reference's data object (dataloader.py:163-166): ``pdata`` = [nvar, nclause, variable_index, clause_index, neg_index]
    (+ [top, nhard] for .wcnf), ``ndata`` = [nvi, nci, nneg, sorted, degree].  make_data adds what the HIP path reads:
    ``num_nodes`` = nvar, ``num_edges`` = K (res = (S + K) / 2), ``device``, the clause CSR and -- built on first use, and
    again when ``ndata[3]`` has been replaced -- the level schedule of the sweep."""

    value_scale = 0.5          # MCPGRound: the round's value in units of res, not of expected = -S

    def __init__(self, pdata=None, ndata=None):
        self.pdata = pdata
        self.ndata = ndata
        self._schedule = None

    def schedule(self):
        """(lv_ptr, lv_data) on the device for the current visiting order ndata[3]."""
        order = np.ascontiguousarray(torch.as_tensor(self.ndata[3]).cpu().numpy(), dtype=np.int32)
        if self._schedule is None or not np.array_equal(self._schedule[0], order):
            lvp, lvd = build_visit_levels(self._clause_ptr_np, self._lit_np, self._weight_np, self.num_nodes, order)
            self._schedule = (order, torch.from_numpy(lvp).to(self.device), torch.from_numpy(lvd).to(self.device))
        return self._schedule[1], self._schedule[2]

    def local_search(self, xs: PackedChains, num_ls: int, seed: int = 0, coins: Optional[TEN] = None, out=None,
                     num_chains: Optional[int] = None, chain_ids=None):
        """Sweep + score on bit-packed chains: (chains after the sweep, expected = -S f32 [C])."""
        lv_ptr, lv_data = self.schedule()
        return mops.mcpg_maxsat_local_search(xs, lv_ptr, lv_data, self._clause_ptr, self._lit, self._weight, num_ls, seed, coins=coins,
                                             out=out, num_chains=num_chains, chain_ids=chain_ids)

    def round_local_search(self, samples: PackedChains, num_ls: int, seed: int, out: PackedChains, chain_ids):
        """What MCPGRound calls in place of the MaxCut kernel."""
        return self.local_search(samples, num_ls, seed, out=out, chain_ids=chain_ids)

    def result(self, xs) -> TEN:
        """res = (S + K) / 2 f32 [C] of chains (f32 [nvar, C] or PackedChains) -- the incumbents' values run_mcpg starts from."""
        packed = xs if isinstance(xs, PackedChains) else PackedChains.pack(xs.to(self.device, torch.float32).contiguous())
        _, expected = self.local_search(packed, 0, out=PackedChains.empty(packed.num_nodes, packed.num_chains, self.device))
        return (self.num_edges - expected) / 2


def build_visit_levels(clause_ptr: np.ndarray, lit: np.ndarray, weight: Optional[np.ndarray], nvar: int, order: np.ndarray):
    """Level schedule of the sweep (include/rlsolver_hip.h: rls_maxsat_visit_levels) as two int32 arrays.  Raises RlsError
    naming the limit for a formula outside the kernel's range, and for a literal 0 or past nvar."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    args = (p(clause_ptr), p(lit), p(weight), int(nvar), int(clause_ptr.size - 1), p(order))
    ng, tot = C.c_int64(0), C.c_int64(0)
    _abi.call("rls_maxsat_visit_levels", *args, None, 0, None, 0, C.byref(ng), C.byref(tot))
    lvp = np.empty(int(ng.value) + 1, dtype=np.int32)
    lvd = np.empty(int(tot.value), dtype=np.int32)
    _abi.call("rls_maxsat_visit_levels", *args, p(lvp), lvp.size, p(lvd), lvd.size, C.byref(ng), C.byref(tot))
    return lvp, lvd


def sort_node(ndata):
    """dataloader.py:269-275: variables by degree + (rand - 0.5) / 2, descending (one torch.rand draw)."""
    degree = ndata[4]
    temp = degree + (torch.rand(degree.shape[0], device=degree.device) - 0.5) / 2
    ndata[3] = torch.argsort(temp, descending=True).to("cpu")
    return ndata


def make_data(nvar: int, clauses, weights=None, top: Optional[int] = None, nclause: Optional[int] = None, device="cuda",
              sorted_nodes=None) -> Data_MaxSAT:
    """The data object of a formula given as lists: ``clauses`` = lists of signed literals +-(v + 1); ``weights`` (with the hard
    weight ``top``) makes it the partial form of a .wcnf; ``nclause`` = the header's clause count where it differs from
    len(clauses); ``sorted_nodes`` replaces sort_node's random tie-break."""
    device = torch.device(device)
    nvar = int(nvar)
    clauses = [[int(l) for l in cl] for cl in clauses]
    if weights is not None and (top is None or len(weights) != len(clauses)):
        raise ValueError("weights need the hard weight `top` and one entry per clause")
    for c, cl in enumerate(clauses):
        for l in cl:
            if l == 0 or abs(l) > nvar:
                raise ValueError(f"clause {c}: literal {l} is outside +-[1, {nvar}]")
    w = [1] * len(clauses) if weights is None else [int(x) for x in weights]
    sizes = np.array([len(cl) for cl in clauses], dtype=np.int64)
    clause_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    lit = np.array([l for cl in clauses for l in cl], dtype=np.int32)
    var = np.abs(lit).astype(np.int64) - 1
    ci = np.repeat(np.arange(len(clauses), dtype=np.int64), sizes)
    neg = np.sign(lit).astype(np.int64) * np.repeat(np.asarray(w, dtype=np.int64), sizes)
    # per variable, once per occurrence: the whole clause of the occurrence, with a fresh local clause id (dataloader.py:240-247)
    occ = np.argsort(var, kind="stable")                      # occurrences grouped by variable, in file order
    occ_clause = ci[occ]
    rep = sizes[occ_clause]
    src = np.repeat(clause_ptr[occ_clause].astype(np.int64) - (np.cumsum(rep) - rep), rep) + np.arange(int(rep.sum()))
    counts = np.bincount(var, minlength=nvar)
    per_var = np.bincount(var, weights=sizes[ci], minlength=nvar).astype(np.int64).tolist()     # literals listed per variable
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    local = np.repeat(np.arange(rep.size) - np.repeat(first, counts), rep)
    nvi = list(torch.split(torch.from_numpy(var[src]).to(device), per_var))
    nci = list(torch.split(torch.from_numpy(local).to(device), per_var))
    nneg = list(torch.split(torch.from_numpy(neg[src]).to(device), per_var))
    degree = torch.from_numpy(counts.astype(np.float32)).to(device)
    ndata = [nvi, nci, nneg, torch.argsort(degree, descending=True).to("cpu"), degree]
    ndata = sort_node(ndata) if sorted_nodes is None else ndata[:3] + [torch.as_tensor(sorted_nodes, dtype=torch.int64).cpu(), degree]
    ncl = len(clauses) if nclause is None else int(nclause)
    pdata = [nvar, ncl, var.tolist(), torch.from_numpy(ci).to(device), torch.from_numpy(neg).to(device)]
    K = ncl
    if weights is not None:
        nhard = sum(1 for x in w if x == int(top))
        pdata += [int(top), nhard]
        K = ncl - nhard + int(top) * nhard
    data = Data_MaxSAT(pdata=pdata, ndata=ndata)
    data.num_nodes, data.num_edges, data.device = nvar, K, device
    data._clause_ptr_np, data._lit_np = clause_ptr, lit
    data._weight_np = None if weights is None else np.asarray(w, dtype=np.int32)
    # (a formula without a literal -- no clause, or empty clauses only -- still hands the kernel a valid lit pointer: one unused entry)
    data._clause_ptr, data._lit = torch.from_numpy(clause_ptr).to(device), torch.from_numpy(lit if lit.size else np.zeros(1, dtype=np.int32)).to(device)
    data._weight = None if weights is None else torch.from_numpy(data._weight_np).to(device)
    if data._weight_np is not None and (data._weight_np.astype(np.int64) != np.asarray(w, dtype=np.int64)).any():
        raise ValueError("clause weights must fit int32")
    # the host builder validates the range now (nvar, weight sums), not at the first round
    build_visit_levels(clause_ptr, lit, data._weight_np, nvar, np.ascontiguousarray(ndata[3].numpy(), dtype=np.int32))
    return data


def read_formula(path):
    """(nvar, nclause, clauses, weights | None, top | None) of a .cnf / .wcnf file as the reference reads it: one clause per line;
    .cnf drops every token "0", .wcnf takes a line's first token as its weight and drops its last one (dataloader.py:192-239)."""
    ext = os.path.splitext(path)[-1]
    if ext not in (".cnf", ".wcnf"):
        raise Exception("Unrecognized file type {}".format(path))
    partial = ext == ".wcnf"
    nvar = nclause = top = None
    clauses, weights = [], []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0] == "c":
                continue
            if t[0] == "p":
                nvar, nclause = int(t[2]), int(t[3])
                top = int(t[4]) if partial else None
                continue
            if partial:
                weights.append(int(t[0]))
                clauses.append([int(x) for x in t[1:-1]])
            else:
                clauses.append([int(x) for x in t if x != "0"])
    return nvar, nclause, clauses, (weights if partial else None), top


def maxsat_dataloader(path, device="cuda", sorted_nodes=None):
    """dataloader.py:169-266: returns (Data_MaxSAT, nvar)."""
    nvar, nclause, clauses, weights, top = read_formula(path)
    return make_data(nvar, clauses, weights, top, nclause, device, sorted_nodes), nvar


def maxsat_tie_coins_from_uniforms(uniforms: TEN) -> TEN:
    """Recorded torch.rand draws f32 [num_ls, nvar (visiting position), C] on the device -> the kernel's tie coins "u < 1/2",
    int64 words [num_ls * nvar, ceil(C / 64)].  new - old is an even integer, so the draw of sampling.py:270 only decides
    d == 0, where the float32 expression is u < 1/2 except for 0 < 1/2 - u <= ulp(|old|) / 2 ("MaxSAT")."""
    num_ls, n, Cc = uniforms.shape
    coin = uniforms.to(torch.float32) < 0.5
    return PackedChains.pack(coin.reshape(num_ls * n, Cc).contiguous()).words.t().contiguous()


def sampler_maxsat_packed(data: Data_MaxSAT, xs: PackedChains, num_ls: int, total_mcmc_num: int, repeat_times: int,
                          num_chains: Optional[int] = None, in_place: bool = True, seed: Optional[int] = None, chain_ids=None):
    """Sweep, score and best of repeats on bit-packed chains, production draws.  Returns (max_res f32 [M], best PackedChains of M
    chains, value f32 [C] = -(res - mean(res)), chains after the sweep)."""
    Cc = xs.num_chains if num_chains is None else num_chains
    out = xs if (in_place and xs.num_chains == Cc) else PackedChains.empty(xs.num_nodes, Cc, xs.device)
    xs_loc, expected = data.local_search(xs, num_ls, _seed_from_torch() if seed is None else seed, out=out, num_chains=Cc,
                                         chain_ids=chain_ids)
    _, max_res, best = mops.mcpg_pick_best(expected, xs_loc, total_mcmc_num, repeat_times, data.num_edges)
    return max_res, best, (expected - expected.mean()) * data.value_scale, xs_loc


def mcpg_sampling_maxsat(data: Data_MaxSAT, start_result: TEN, probs: TEN, num_ls: int, change_times: int, total_mcmc_num: int,
                         device=None, index: Optional[TEN] = None, u: Optional[TEN] = None, uniforms: Optional[TEN] = None):
    """sampling.py:253-285.  ``index`` / ``u`` replace the walk's torch.randint / torch.rand draws, ``uniforms`` f32
    [num_ls, nvar, C] the sweep's (test hooks)."""
    device = data.device if device is None else torch.device(device)
    raw = metro_sampling(probs, start_result.to(device), change_times, device, index=index, u=u)
    Cc = raw.shape[1]
    coins = None if uniforms is None else maxsat_tie_coins_from_uniforms(uniforms.to(device))
    xs_loc, expected = data.local_search(PackedChains.pack(raw), num_ls, 0 if uniforms is not None else _seed_from_torch(), coins=coins)
    _, max_res, best = mops.mcpg_pick_best(expected, xs_loc, total_mcmc_num, Cc // total_mcmc_num, data.num_edges)
    res = (data.num_edges - expected) / 2
    return max_res, best, raw, -(res - res.sum() / Cc)
