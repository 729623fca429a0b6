"""Tensor-level wrappers for the MCPG and TSP entry points (same conventions as ops.py: outputs allocated here, the work
goes through ``torch.ops.rlsolver_hip.*``)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _abi
from .ops import DeviceGraph, _check, _ptr, _s64, _stream, _t  # noqa: F401  (_ptr / _stream: raw C-ABI calls in tests)

TEN = torch.Tensor
_NM_DTYPES = (torch.float32, torch.uint8, torch.bool)


# ------------------------------------------------------------------------------ MCPG
class PackedChains:
    """C chains over N nodes, bit-packed tile-major: ``words`` int64 [ceil(C / 64), N] (the uint64 bit patterns; word
    (t, n) bit e = node n of chain 64 t + e).  include/rlsolver_hip.h, "Layouts of a batch of C chains"."""

    __slots__ = ("words", "num_chains")

    def __init__(self, words: TEN, num_chains: int):
        _check(words, "words", (torch.int64,))
        if words.dim() != 2 or words.shape[0] != (num_chains + 63) // 64:
            raise ValueError(f"words must be [ceil({num_chains} / 64), N]")
        self.words, self.num_chains = words, num_chains

    @property
    def num_nodes(self) -> int:
        return self.words.shape[1]

    @property
    def device(self):
        return self.words.device

    @classmethod
    def empty(cls, num_nodes: int, num_chains: int, device):
        return cls(torch.empty(((num_chains + 63) // 64, num_nodes), dtype=torch.int64, device=device), num_chains)

    @classmethod
    def pack(cls, xs: TEN):
        """node-major [N, C] float32 / uint8 / bool -> PackedChains (one kernel)."""
        _check(xs, "xs", _NM_DTYPES)
        N, Cc = xs.shape
        out = cls.empty(N, Cc, xs.device)
        _t.mcpg_pack_chains(xs, out.words)
        return out

    def unpack(self) -> TEN:
        """-> node-major float32 [N, C] holding 0.0 | 1.0 (the reference's surface)."""
        xs = torch.empty((self.num_nodes, self.num_chains), dtype=torch.float32, device=self.device)
        _t.mcpg_unpack_chains(self.words, self.num_chains, xs)
        return xs

    def clone(self):
        return PackedChains(self.words.clone(), self.num_chains)


def _chains(x, name):
    """(pointer tensor, spin_bytes, N, C) of a node-major tensor or a PackedChains."""
    if isinstance(x, PackedChains):
        return x.words, 0, x.num_nodes, x.num_chains
    _check(x, name, _NM_DTYPES)
    if x.dim() != 2:
        raise ValueError(f"{name} must be [N, C]")
    return x, (4 if x.dtype == torch.float32 else 1), x.shape[0], x.shape[1]


def _chain_ids(chain_ids) -> tuple:
    """(offset, period, skip) of include/rlsolver_hip.h: rls_chain_ids; None = the single-process numbering."""
    if chain_ids is None:
        return (0, 0, 0)
    off, per, skip = (int(v) for v in chain_ids)
    return (off, per, skip)


def mcpg_metro_rounds(samples, probs: TEN, T: int, index: Optional[TEN] = None, u: Optional[TEN] = None,
                      seed: int = 0, t_limit: Optional[TEN] = None, write_back: bool = True,
                      accepts: Optional[TEN] = None, t_offset: int = 0, samples_in=None, chain_ids=None, scratch: Optional[TEN] = None) -> None:
    """K9 (see include/rlsolver_hip.h).  samples [N, C] f32/uint8 or PackedChains, in place, or read from
    ``samples_in`` (same layout; a PackedChains with fewer chains -- a multiple of 64 -- is broadcast) and written to
    ``samples``.  ``chain_ids`` = (offset, period, skip): the global ids of a shard's chains (rls_chain_ids)."""
    st, sb, N, Cc = _chains(samples, "samples")
    dev = st.device
    _check(probs, "probs", (torch.float32,), dev, (N,))
    if (index is None) != (u is None):
        raise ValueError("index and u must be given together")
    if index is not None:
        _check(index, "index", (torch.int64,), dev)
        _check(u, "u", (torch.float32,), dev)
        if index.shape[0] < t_offset + T or u.shape[0] < t_offset + T or index.shape[1:] != (Cc,) or u.shape[1:] != (Cc,):
            raise ValueError("index/u must be [>= t_offset + T, C]")
    if t_limit is not None:
        _check(t_limit, "t_limit", (torch.int64,), dev)
    accept_rows = 1
    if accepts is not None:     # [T] or [rows, T]: workgroups spread their adds over the rows, a round's count = its column sum
        _check(accepts, "accepts", (torch.int64,), dev)
        if accepts.dim() == 2:
            accept_rows = accepts.shape[0]
        if accepts.dim() not in (1, 2) or accepts.shape[-1] != T:
            raise ValueError("accepts must be [T] or [rows, T]")
    sin, c_in = None, Cc
    if samples_in is not None:
        sin, sb_in, n_in, c_in = _chains(samples_in, "samples_in")
        if sb_in != sb or n_in != N or (sb != 0 and (c_in != Cc or sin.dtype != st.dtype)) or sin.device != dev:
            raise ValueError("samples_in must have the layout and node count of samples")
        if not write_back:
            raise ValueError("samples_in needs write_back")
    if scratch is None and sb == 0:     # the packed walk's draw windows (include/rlsolver_hip.h: rls_mcpg_metro_scratch_bytes)
        scratch = metro_scratch(N, Cc, dev)
    _t.mcpg_metro_rounds(st, sin, c_in, Cc, probs, T, t_offset, index, u, _s64(seed), t_limit, bool(write_back), accepts,
                         *_chain_ids(chain_ids), scratch)


def metro_scratch(N: int, C: int, device) -> Optional[TEN]:
    """The scratch the bit-packed walk wants at this size (None: it keeps its draw windows in LDS).  A caller that walks in chunks
    allocates it once and passes it to every mcpg_metro_rounds call."""
    from . import _abi
    need = int(_abi.lib().rls_mcpg_metro_scratch_bytes(int(N), int(C)))
    return torch.empty(need, dtype=torch.uint8, device=device) if need > 0 else None


def mcpg_metro_max_rounds(N: int, spin_bytes: int) -> int:
    """Rounds one mcpg_metro_rounds launch can take with accept counts in this layout (0: N does not fit at all)."""
    from . import _abi
    return int(_abi.lib().rls_mcpg_metro_max_rounds(int(N), int(spin_bytes)))


def mcpg_metro_stop(accepts: TEN, target: int, first: int, next_T: int, ctl: TEN, apply_limit: Optional[TEN] = None) -> None:
    """The stop rule between two chunks of metro rounds (include/rlsolver_hip.h: rls_mcpg_metro_stop).  accepts int64 [rows, T],
    ctl int64 [3] = {accepts so far, live, limit of the next dry pass} (in / out), apply_limit int64 [1] (out).  first: 1 the
    call's first chunk, 2 a later chunk applied directly (inside the first T rounds), 0 a dry pass."""
    dev = accepts.device
    _check(accepts, "accepts", (torch.int64,), dev)
    _check(ctl, "ctl", (torch.int64,), dev, (3,))
    if apply_limit is not None:
        _check(apply_limit, "apply_limit", (torch.int64,), dev, (1,))
    _t.mcpg_metro_stop(accepts, int(target), int(first), int(next_T), ctl, apply_limit)


def mcpg_local_search(g: DeviceGraph, xs_in: TEN, order: TEN, num_ls: int, uniforms: Optional[TEN] = None,
                      seed: int = 0, visit_stream: Optional[TEN] = None, edge_weights: Optional[TEN] = None,
                      gauge_node: int = -1, chain_ids=None):
    """K7 + expected cut.  Returns (xs_out f32 [N, C], expected f32 [C]).  ``edge_weights`` int32 [E'] (in the order of
    the graph's stored edges) + a weighted visit stream select the weighted sampler; ``gauge_node`` >= 0 XORs every
    chain with its value at that node first (rlsolver/methods/MCPG/sampling.py:101-104)."""
    _check(xs_in, "xs_in", _NM_DTYPES, g.device)
    if xs_in.dim() != 2 or xs_in.shape[0] != g.num_nodes:
        raise ValueError(f"xs_in must be [{g.num_nodes}, C]")
    Cc = xs_in.shape[1]
    _check(order, "order", (torch.int32,), g.device, (g.num_nodes,))
    if uniforms is not None:
        _check(uniforms, "uniforms", (torch.float32,), g.device, (num_ls, g.num_nodes, Cc))
    xs_out = torch.empty((g.num_nodes, Cc), dtype=torch.float32, device=g.device)
    expected = torch.empty(Cc, dtype=torch.float32, device=g.device)
    if visit_stream is not None:
        _check(visit_stream, "visit_stream", (torch.int32,), g.device)
    if edge_weights is not None:
        _check(edge_weights, "edge_weights", (torch.int32,), g.device, (g.num_stored_edges,))
    _t.mcpg_local_search(g.handle, xs_in, xs_out, order, visit_stream, num_ls, uniforms, _s64(seed), edge_weights, int(gauge_node), expected,
                         *_chain_ids(chain_ids))
    return xs_out, expected


def mcpg_local_search_levels(g: DeviceGraph, xs_in, lv_ptr: TEN, lv_data: TEN, num_ls: int, seed: int = 0,
                             coins: Optional[TEN] = None, out=None, num_chains: Optional[int] = None, chain_ids=None):
    """K7 + expected cut on the level-parallel schedule (rls_mcpg_visit_levels).  ``xs_in``: node-major [N, C] or
    PackedChains (which may hold fewer chains than ``num_chains``, a multiple of 64: broadcast).  ``coins`` int64 (bit
    pattern of uint64) [num_ls * N, ceil(C / 64)]: the tie coins "u < 1/2" -- test hook; None = counter hash keyed by
    seed.  ``out``: a PackedChains to write (may be xs_in itself) or None = node-major f32.
    Returns (xs_out, expected f32 [C])."""
    st, sb, N, c_in = _chains(xs_in, "xs_in")
    if st.device != g.device or N != g.num_nodes:
        raise ValueError(f"xs_in must hold {g.num_nodes} nodes on {g.device}")
    Cc = c_in if num_chains is None else num_chains
    _check(lv_ptr, "lv_ptr", (torch.int32,), g.device)
    _check(lv_data, "lv_data", (torch.int32,), g.device)
    if coins is not None:
        _check(coins, "coins", (torch.int64,), g.device, (num_ls * g.num_nodes, (Cc + 63) // 64))
    if out is None:
        xs_out = torch.empty((g.num_nodes, Cc), dtype=torch.float32, device=g.device)
        ot, osb = xs_out, 4
    else:
        if not isinstance(out, PackedChains) or out.num_chains != Cc or out.num_nodes != N or out.device != g.device:
            raise ValueError("out must be a PackedChains of num_chains chains")
        xs_out, ot, osb = out, out.words, 0
    expected = torch.empty(Cc, dtype=torch.float32, device=g.device)
    _t.mcpg_local_search_levels(g.handle, st, c_in, ot, Cc, lv_ptr, lv_data, num_ls, coins, _s64(seed), expected,
                                *_chain_ids(chain_ids))
    return xs_out, expected


def mcpg_maxsat_local_search(xs_in: PackedChains, lv_ptr: TEN, lv_data: TEN, clause_ptr: TEN, lit: TEN, weight: Optional[TEN],
                             num_ls: int, seed: int = 0, coins: Optional[TEN] = None, out=None, num_chains: Optional[int] = None,
                             chain_ids=None):
    """The sweep and the score of the MaxSAT sampler (include/rlsolver_hip.h: rls_maxsat_local_search) on the schedule of
    rls_maxsat_visit_levels.  ``xs_in``: PackedChains over the variables (may hold fewer chains than ``num_chains``, a multiple of
    64: broadcast); ``clause_ptr`` / ``lit`` / ``weight``: the formula as a clause CSR, int32 on the device; ``coins`` int64
    [num_ls * nvar, ceil(C / 64)]: the tie coins "u < 1/2" -- test hook; None = counter hash keyed by seed.  ``out``: a PackedChains
    to write (may be xs_in itself) or None = node-major f32.  ``num_ls = 0`` only scores.
    Returns (xs_out, expected f32 [C]) with expected = -sum_clauses max_lit(s_v neg)."""
    if not isinstance(xs_in, PackedChains):
        raise TypeError("xs_in must be a PackedChains")
    dev, N = xs_in.device, xs_in.num_nodes
    Cc = xs_in.num_chains if num_chains is None else num_chains
    for t, name in ((lv_ptr, "lv_ptr"), (lv_data, "lv_data"), (clause_ptr, "clause_ptr"), (lit, "lit")):
        _check(t, name, (torch.int32,), dev)
    if weight is not None:
        _check(weight, "weight", (torch.int32,), dev, (clause_ptr.numel() - 1,))
    if coins is not None:
        _check(coins, "coins", (torch.int64,), dev, (num_ls * N, (Cc + 63) // 64))
    if out is None:
        xs_out = ot = torch.empty((N, Cc), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, PackedChains) or out.num_chains != Cc or out.num_nodes != N or out.device != dev:
            raise ValueError("out must be a PackedChains of num_chains chains")
        xs_out, ot = out, out.words
    expected = torch.empty(Cc, dtype=torch.float32, device=dev)
    _t.maxsat_local_search(xs_in.words, xs_in.num_chains, ot, Cc, lv_ptr, lv_data, int(num_ls), coins, _s64(seed), clause_ptr, lit, weight,
                           expected, *_chain_ids(chain_ids))
    return xs_out, expected


def mcpg_cheeger_local_search(g: DeviceGraph, xs_in: PackedChains, visit_stream: TEN, normalized: bool, num_ls: int, edge_weight_sum: float,
                              out=None, num_chains: Optional[int] = None, want_cut_size: bool = True):
    """The sweep and the score of the two Cheeger-cut samplers (include/rlsolver_hip.h: rls_cheeger_local_search).  ``xs_in``:
    PackedChains over the nodes (may hold fewer chains than ``num_chains``, a multiple of 64: broadcast); ``visit_stream`` int32
    [3 N + nnz]: the records of methods/MCPG_cheeger.py: build_cheeger_stream in visiting order; ``normalized``: the normalised cut
    (ncheegercut) instead of the ratio cut.  ``out``: a PackedChains to write (may be xs_in itself) or None = node-major f32.
    ``num_ls = 0`` only scores (the one case where h can hold NaN: an empty side, 0 / 0).
    Returns (xs_out, h f32 [C], cut f32 [C], size f32 [C]); cut and size are None with ``want_cut_size=False``."""
    if not isinstance(xs_in, PackedChains):
        raise TypeError("xs_in must be a PackedChains")
    dev, N = xs_in.device, xs_in.num_nodes
    if dev != g.device or N != g.num_nodes:
        raise ValueError(f"xs_in must hold {g.num_nodes} nodes on {g.device}")
    Cc = xs_in.num_chains if num_chains is None else num_chains
    _check(visit_stream, "visit_stream", (torch.int32,), dev, (3 * N + g.nnz,))
    if out is None:
        xs_out = ot = torch.empty((N, Cc), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, PackedChains) or out.num_chains != Cc or out.num_nodes != N or out.device != dev:
            raise ValueError("out must be a PackedChains of num_chains chains")
        xs_out, ot = out, out.words
    h = torch.empty(Cc, dtype=torch.float32, device=dev)
    cut = torch.empty(Cc, dtype=torch.float32, device=dev) if want_cut_size else None
    size = torch.empty(Cc, dtype=torch.float32, device=dev) if want_cut_size else None
    _t.cheeger_local_search(g.handle, xs_in.words, xs_in.num_chains, ot, Cc, visit_stream, int(bool(normalized)), int(num_ls),
                            float(edge_weight_sum), h, cut, size)
    return xs_out, h, cut, size


def mcpg_maxcut_edge_local_search(g: DeviceGraph, edge_weights: TEN, xs_in: PackedChains, visit_stream: TEN, max_abs_degree: int,
                                  weight_abs_sum: int, num_ls: int, gauge_node: int = -1, uniforms: Optional[TEN] = None, seed: int = 0,
                                  out=None, num_chains: Optional[int] = None, chain_ids=None):
    """Gauge fix, sweep and score of the edge-flip MaxCut sampler (include/rlsolver_hip.h: rls_maxcut_edge_local_search).
    ``xs_in``: PackedChains over the nodes (may hold fewer chains than ``num_chains``, a multiple of 64: broadcast);
    ``edge_weights`` int32 [E'] in the order of the graph's stored edges; ``visit_stream`` int32: the records of
    methods/MCPG.py: build_edge_stream; ``max_abs_degree`` / ``weight_abs_sum``: the largest sum of |weights| at a node and the
    sum over the edges (the exactness limits are checked on them); ``gauge_node``: the hub every chain is XORed with, -1 = none.
    ``uniforms`` f32 [num_ls, E', 3, C]: the three draws per (pass, position) -- test hook; None = counter hash keyed by seed and
    the global chain id (``chain_ids``).  ``out``: a PackedChains to write (may be xs_in itself) or None = node-major f32, where a
    node no position writes holds -0.5 | 1.5.  ``num_ls = 0`` applies the gauge and scores.
    Returns (xs_out, expected f32 [C])."""
    if not isinstance(xs_in, PackedChains):
        raise TypeError("xs_in must be a PackedChains")
    dev, N = xs_in.device, xs_in.num_nodes
    if dev != g.device or N != g.num_nodes:
        raise ValueError(f"xs_in must hold {g.num_nodes} nodes on {g.device}")
    Cc = xs_in.num_chains if num_chains is None else num_chains
    _check(edge_weights, "edge_weights", (torch.int32,), dev, (g.num_stored_edges,))
    _check(visit_stream, "visit_stream", (torch.int32,), dev)
    if uniforms is not None:
        _check(uniforms, "uniforms", (torch.float32,), dev, (num_ls, g.num_stored_edges, 3, Cc))
    if out is None:
        xs_out = ot = torch.empty((N, Cc), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, PackedChains) or out.num_chains != Cc or out.num_nodes != N or out.device != dev:
            raise ValueError("out must be a PackedChains of num_chains chains")
        xs_out, ot = out, out.words
    expected = torch.empty(Cc, dtype=torch.float32, device=dev)
    _t.maxcut_edge_local_search(g.handle, edge_weights, xs_in.words, xs_in.num_chains, ot, Cc, visit_stream, int(max_abs_degree),
                                int(weight_abs_sum), int(gauge_node), int(num_ls), uniforms, _s64(seed), expected, *_chain_ids(chain_ids))
    return xs_out, expected


def mimo_launch_form(n: int, num_chains: int):
    """(supported, form) of rls_mimo_local_search_supported: whether n variables fit the kernel's LDS budget at this many chains and
    which launch form the shape gets (0: 32-chain workgroups of 8 waves, 1: of 4 waves, 2: 64-chain workgroups).  A host query."""
    import ctypes
    from . import _abi
    form = ctypes.c_int32(-1)
    ok = _abi.lib().rls_mimo_local_search_supported(int(n), int(num_chains), ctypes.byref(form))
    return bool(ok), int(form.value)


def mcpg_mimo_local_search(Sigma: TEN, Diag: TEN, xs_in: PackedChains, num_ls: int, out=None, num_chains: Optional[int] = None,
                           _score_only: bool = False):
    """The coordinate search and the value of the MIMO detection sampler (include/rlsolver_hip.h: rls_mimo_local_search).
    ``Sigma`` f32 [n, n], ``Diag`` f32 [n]; ``xs_in``: PackedChains over the variables (bit 1 = +; may hold fewer chains than
    ``num_chains``, a multiple of 64: broadcast).  ``out``: a PackedChains to write (may be xs_in itself) or None = node-major f32
    holding 0|1 (the packed result through the unpack kernel).  ``num_ls`` >= 1: every variable counts +-2 until its first visit.
    Returns (xs_out, expected f32 [C]) with expected = info^T Sigma info + Diag . info, the quantity the sampler minimises."""
    if not isinstance(xs_in, PackedChains):
        raise TypeError("xs_in must be a PackedChains")
    _check(Sigma, "Sigma", (torch.float32,))
    dev = Sigma.device
    if Sigma.dim() != 2 or Sigma.shape[0] != Sigma.shape[1] or Sigma.shape[0] < 1:
        raise ValueError(f"Sigma must be square [n, n], got {tuple(Sigma.shape)}")
    n = Sigma.shape[0]
    _check(Diag, "Diag", (torch.float32,), dev, (n,))
    if xs_in.device != dev or xs_in.num_nodes != n:
        raise ValueError(f"xs_in must hold {n} variables on {dev}")
    Cc = xs_in.num_chains if num_chains is None else int(num_chains)
    if not _score_only and int(num_ls) < 1:
        raise ValueError(f"num_ls must be >= 1 (a sweep-less call would leave +-2 entries), got {num_ls}")
    if Cc != xs_in.num_chains and (xs_in.num_chains % 64 != 0 or xs_in.num_chains > Cc):
        raise ValueError("a broadcast input needs a multiple of 64 chains, fewer than num_chains")
    ok, _ = mimo_launch_form(n, Cc)
    if not ok:
        raise ValueError(f"n={n} is beyond the LDS limit of the MIMO kernel at {Cc} chains (rls_mimo_local_search_supported)")
    expected = torch.empty(Cc, dtype=torch.float32, device=dev)
    if _score_only:                      # Data_MIMO.result: the value of +-1 chains, no sweep, nothing written
        _t.mimo_local_search(Sigma, Diag, xs_in.words, xs_in.num_chains, None, Cc, 0, expected)
        return xs_in, expected
    if out is None:
        packed = PackedChains.empty(n, Cc, dev)
    else:
        if not isinstance(out, PackedChains) or out.num_chains != Cc or out.num_nodes != n or out.device != dev:
            raise ValueError("out must be a PackedChains of num_chains chains")
        if out.words.data_ptr() == xs_in.words.data_ptr() and xs_in.num_chains != Cc:
            raise ValueError("in-place needs xs_in to hold num_chains chains")
        packed = out
    _t.mimo_local_search(Sigma, Diag, xs_in.words, xs_in.num_chains, packed.words, Cc, int(num_ls), expected)
    return (packed.unpack() if out is None else packed), expected


def mcpg_pick_best(expected: TEN, xs, total_mcmc_num: int, repeat_times: int, num_edges: int):
    """K8 second half.  Returns (best_index int64 [M], vs_good f32 [M], xs_good: f32 [N, M] or PackedChains of M chains)."""
    st, sb, N, Cc = _chains(xs, "xs")
    if sb == 1:
        raise TypeError("xs must be float32 node-major or PackedChains")
    dev = st.device
    if Cc != total_mcmc_num * repeat_times:
        raise ValueError("xs must hold total_mcmc_num * repeat_times chains")
    _check(expected, "expected", (torch.float32,), dev, (Cc,))
    idx = torch.empty(total_mcmc_num, dtype=torch.int64, device=dev)
    vs = torch.empty(total_mcmc_num, dtype=torch.float32, device=dev)
    if sb == 0:
        xg = PackedChains.empty(N, total_mcmc_num, dev)
        xgt = xg.words
    else:
        xg = xgt = torch.empty((N, total_mcmc_num), dtype=torch.float32, device=dev)
    _t.mcpg_pick_best(expected, st, N, total_mcmc_num, repeat_times, num_edges, idx, vs, xgt)
    return idx, vs, xg


def mcpg_merge_best(temp_max: TEN, temp_info: PackedChains, now_max_res: TEN, now_info: PackedChains, replace_worst: bool = True):
    """The best-merge of methods/MCPG.py:376-391 in place on the device.  Returns (best value f32 [1], its chain int64 [1]);
    with ``replace_worst=False`` (a shard of the kept chains) only the per-chain merge is applied and the results are
    [2] = {max, min} of now_max_res and their first chains."""
    M, N, dev = temp_info.num_chains, temp_info.num_nodes, temp_info.device
    _check(temp_max, "temp_max", (torch.float32,), dev, (M,))
    _check(now_max_res, "now_max_res", (torch.float32,), dev, (M,))
    if now_info.num_chains != M or now_info.num_nodes != N:
        raise ValueError("now_info must match temp_info")
    mask = torch.empty((M + 63) // 64, dtype=torch.int64, device=dev)
    bv = torch.empty(1 if replace_worst else 2, dtype=torch.float32, device=dev)
    bi = torch.empty(1 if replace_worst else 2, dtype=torch.int64, device=dev)
    _t.mcpg_merge_best(temp_max, temp_info.words, now_max_res, now_info.words, M, mask, bv, bi, bool(replace_worst))
    return bv, bi


def mcpg_value_bit_sums(samples: PackedChains, value: TEN) -> TEN:
    """A[n] = sum_c value[c] * s[n, c]  (f32 [N]); see rls_mcpg_value_bit_sums."""
    _check(value, "value", (torch.float32,), samples.device, (samples.num_chains,))
    A = torch.zeros(samples.num_nodes, dtype=torch.float32, device=samples.device)
    _t.mcpg_value_bit_sums(samples.words, samples.num_chains, value, A)
    return A


# ------------------------------------------------------------------------------ TSP
def _perm(p: TEN, name="perm"):
    _check(p, name, (torch.int64,))
    if p.dim() != 2:
        raise ValueError(f"{name} must be [B, N]")
    return p.shape


def tsp_tour_length(dist: TEN, perm: TEN) -> TEN:
    B, N = _perm(perm)
    _check(dist, "dist", (torch.float32,), perm.device, (N, N))
    out = torch.empty(B, dtype=torch.float32, device=perm.device)
    _t.tsp_tour_length(dist, perm, out)
    return out


def tsp_tables8(nearest: TEN, random: TEN) -> Optional[TEN]:
    """The two neighbour tables of ISCO_TSP as the byte block K13 keeps in LDS (include/rlsolver_hip.h: rls_tsp_tables8_bytes):
    uint8 [N, K] then the first N - K - 1 columns of ``random`` as uint8, each zero-padded to 16 bytes; None when N > 256."""
    from . import _abi
    N, K = int(nearest.shape[0]), int(nearest.shape[1])
    nb = int(_abi.lib().rls_tsp_tables8_bytes(N, K))
    if nb == 0:
        return None
    out = torch.zeros(nb, dtype=torch.uint8, device=nearest.device)
    a = (N * K + 15) // 16 * 16
    out[:N * K] = nearest.reshape(-1).to(torch.uint8)
    out[a:a + N * (N - K - 1)] = random[:, :N - K - 1].reshape(-1).to(torch.uint8)
    return out


def tsp_swap_delta_all(dist: TEN, perm: TEN, selected: Optional[TEN], temperature: float, nearest: Optional[TEN] = None,
                       random: Optional[TEN] = None, near_threshold: float = 0.0, seed: int = 0, env_offset: int = 0,
                       return_selected: bool = False, tables8: Optional[TEN] = None):
    """K13, ISCO_TSP.opt_2 (env_ISCO.py:238-335) -> (logratio f32, indices int64, ban bool), all [B, N].
    ``selected`` int64 [B, N]: the partner cities, given (the recorded-draw hook of the golden tests); None (production): drawn
    in the kernel from (seed, env_offset + b, position) through ``nearest`` int32 [N, K] / ``random`` int32 [N, >= N - K - 1]
    with ``near_threshold`` = K / (K + 1) -- ``return_selected`` appends the drawn cities (int64 [B, N]); ``tables8`` =
    ``tsp_tables8(nearest, random)``, built once by the caller, lets the kernel keep both tables in LDS (N <= 256)."""
    B, N = _perm(perm)
    dev = perm.device
    _check(dist, "dist", (torch.float32,), dev, (N, N))
    sel_out = None
    if selected is not None:
        _check(selected, "selected", (torch.int64,), dev, (B, N))
        if return_selected:
            raise ValueError("return_selected records the in-kernel draw: it needs selected=None")
    else:
        if nearest is None or random is None:
            raise ValueError("selected=None draws the partners in the kernel: nearest / random tables must be given")
        _check(nearest, "nearest", (torch.int32,), dev)
        _check(random, "random", (torch.int32,), dev)
        if return_selected:
            sel_out = torch.empty((B, N), dtype=torch.int64, device=dev)
    logratio = torch.empty((B, N), dtype=torch.float32, device=dev)
    indices = torch.empty((B, N), dtype=torch.int64, device=dev)
    ban = torch.empty((B, N), dtype=torch.bool, device=dev)
    _t.tsp_swap_delta_all(dist, perm, selected, nearest, random, tables8, float(near_threshold), _s64(seed), int(env_offset), sel_out,
                          float(temperature), logratio, indices, ban)
    return (logratio, indices, ban, sel_out) if return_selected else (logratio, indices, ban)


def tsp_apply_swap(perm: TEN, pos: TEN, indices: TEN) -> None:
    B, N = _perm(perm)
    _check(pos, "pos", (torch.int64,), perm.device, (B,))
    _check(indices, "indices", (torch.int64,), perm.device, (B, N))
    _t.tsp_apply_swap(perm, pos, indices)


def tsp_2opt_delta(dist: TEN, perm: TEN, i: TEN, j: TEN) -> TEN:
    B, N = _perm(perm)
    dev = perm.device
    _check(dist, "dist", (torch.float32,), dev, (N, N))
    _check(i, "i", (torch.int64,), dev, (B,))
    _check(j, "j", (torch.int64,), dev, (B,))
    out = torch.empty(B, dtype=torch.float32, device=dev)
    _t.tsp_2opt_delta(dist, perm, i, j, out)
    return out


def rand_perms(B: int, N: int, seed: int, device, env_offset: int = 0) -> TEN:
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError("rand_perms needs a HIP device")
    out = torch.empty((B, N), dtype=torch.int64, device=device)
    _t.rand_perms(out, _s64(seed), env_offset)
    return out


def tsp_2opt_best(dist64: TEN, perm: TEN, cur_length: Optional[TEN] = None, slices: Optional[int] = None):
    """One best-improvement 2-opt pass per tour (rls_tsp_2opt_best): -> (best_i, best_j int64 [B], best_value f64 [B]).
    ``cur_length`` f64 [B]: candidates ranked by their whole length summed as the reference's distance_calc does (its own
    comparison values); best_value = the best candidate's length, or cur_length and (-1, -1) where none is shorter.
    Without it: ranked by the O(1) reversal delta (symmetric dist); best_value = the most negative delta, or 0.
    ``slices`` workgroups share one tour's candidates (default: enough to put ~2 workgroups on every CU)."""
    dev = perm.device
    _check(dist64, "dist", (torch.float64,), dev)
    _check(perm, "perm", (torch.int64,), dev)
    B, N = perm.shape
    if dist64.shape != (N, N):
        raise ValueError(f"dist must be [{N}, {N}]")
    if cur_length is not None:
        _check(cur_length, "cur_length", (torch.float64,), dev, (B,))
    if slices is None:   # ~512 workgroups in all; a workgroup gets >= 256 candidates (whole-length ranking: O(N) each) or >= 8192 (deltas)
        per_wg = 256 if cur_length is not None else 8192
        slices = max(1, min(512 // max(B, 1), (N * (N - 1) // 2 + per_wg - 1) // per_wg))
    bi = torch.empty(slices * B, dtype=torch.int64, device=dev)
    bj = torch.empty(slices * B, dtype=torch.int64, device=dev)
    bv = torch.empty(slices * B, dtype=torch.float64, device=dev)
    _t.tsp_2opt_best(dist64, perm, cur_length, bi, bj, bv)
    return bi[:B], bj[:B], bv[:B]


def tsp_3opt_default_slices(N: int, B: int, exact: bool) -> int:
    """Workgroups per tour when the caller names none: ~512 in all, and a wave gets at least one item of the kernel's work list
    -- whole-length ranking: a chunk of 64 triples (about C(N, 3) / 64 + N of them: every i ends on a ragged one), O(N) per
    candidate; deltas: an (i, j) pair, N (N - 1) / 2 of them, and at least 8 per wave."""
    items = (N * (N - 1) * (N - 2) // 6 + (N - 1) * (N - 2) // 2) // 64 + N if exact else N * (N - 1) // 2
    per_wg = max(1, _abi.tsp_3opt_launch_form(N, exact).waves) * (1 if exact else 8)
    return max(1, min(512 // max(B, 1), (items + per_wg - 1) // per_wg))


def tsp_3opt_best(dist64: TEN, perm: TEN, cur_length: Optional[TEN] = None, slices: Optional[int] = None):
    """One best-improvement pass of the reference's 3-opt per tour (rls_tsp_3opt_best, opt_3.py:42-105): over all triples
    (i, j, k) of segments_3_opt(N) and the seven in-place reversals of S1 / S2 / C (trial 0..6 = aBC AbC ABc Abc abC aBc abc)
    -> (best_i, best_j, best_k, best_trial int64 [B], best_value f64 [B]), the first strict minimum in (i, j, k, trial) order.
    ``cur_length`` f64 [B]: candidates ranked by their whole length summed as the reference's distance_calc does;
    best_value = the winner's length, or cur_length and -1 indices where none is shorter.  Without it: ranked by the
    junction delta (symmetric dist); best_value = the most negative delta, or 0.
    ``slices`` workgroups share one tour's (i, j) pairs (default: a lone tour spreads over the chip)."""
    dev = perm.device
    _check(dist64, "dist", (torch.float64,), dev)
    _check(perm, "perm", (torch.int64,), dev)
    if perm.dim() != 2:
        raise ValueError("perm must be [B, N]")
    B, N = perm.shape
    if N < 3:
        raise ValueError(f"tsp_3opt_best needs N >= 3 cities, got {N}")
    if dist64.shape != (N, N):
        raise ValueError(f"dist must be [{N}, {N}]")
    if cur_length is not None:
        _check(cur_length, "cur_length", (torch.float64,), dev, (B,))
    slices = tsp_3opt_default_slices(N, B, cur_length is not None) if slices is None else int(slices)
    if not 1 <= slices <= 65535:
        raise ValueError(f"slices = {slices} outside [1, 65535]")
    out = [torch.empty(slices * B, dtype=torch.int64, device=dev) for _ in range(4)]
    bv = torch.empty(slices * B, dtype=torch.float64, device=dev)
    _t.tsp_3opt_best(dist64, perm, cur_length, out[0], out[1], out[2], out[3], bv)
    return out[0][:B], out[1][:B], out[2][:B], out[3][:B], bv[:B]


def tsp_neighbour_chain(dist64: TEN, start: TEN, farthest: bool = False):
    """The order in which the reference's constructors take up cities (rls_tsp_neighbour_chain; nn.py:62-75, ins_f.py:84-96):
    chain[s, 0] = start[s], chain[s, k + 1] = the nearest (``farthest``: farthest) city to chain[s, k] not yet in the chain, the
    lowest index among equals.  -> (chain int64 [S, N], status int32 [S]); status 2 where start[s] lies outside [0, N): that row
    of chain is then zeros."""
    _check(dist64, "dist", (torch.float64,))
    dev = dist64.device
    if dist64.dim() != 2 or dist64.shape[0] != dist64.shape[1] or dist64.shape[0] < 2:
        raise ValueError(f"dist must be square [N, N] with N >= 2, got {tuple(dist64.shape)}")
    _check(start, "start", (torch.int64,), dev)
    if start.dim() != 1:
        raise ValueError("start must be [S]")
    S, N = start.shape[0], dist64.shape[0]
    chain = torch.zeros((S, N), dtype=torch.int64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    _t.tsp_neighbour_chain(dist64, start, int(bool(farthest)), chain, status)
    return chain, status


def tsp_grow_2opt(dist64: TEN, order: TEN, m_seed: int = 2, m_end: Optional[int] = None, first_m: int = 3, max_passes: Optional[int] = None,
                  out=None):
    """Grow-and-converge (rls_tsp_grow_2opt): row s starts as order[s, :m_seed], takes order[s, m - 1] at its end for m = m_seed + 1
    .. m_end, and from m = first_m on is 2-opted (the exact ranking of tsp_2opt_best) until a pass brings nothing, all in one launch.
    -> (tours int64 [S, N], length f64 [S], passes int64 [S], status int32 [S]); status 1: a convergence reached ``max_passes``
    (default N^2, a guard and no tuning value); 2: an entry of the row outside [0, N), its outputs untouched.  ``out``: the four
    output tensors to write into (default: new ones, tours / length / passes zeroed)."""
    _check(dist64, "dist", (torch.float64,))
    dev = dist64.device
    if dist64.dim() != 2 or dist64.shape[0] != dist64.shape[1] or dist64.shape[0] < 2:
        raise ValueError(f"dist must be square [N, N] with N >= 2, got {tuple(dist64.shape)}")
    N = dist64.shape[0]
    _check(order, "order", (torch.int64,), dev)
    if order.dim() != 2 or order.shape[1] != N:
        raise ValueError(f"order must be [S, {N}]")
    S = order.shape[0]
    m_end = N if m_end is None else int(m_end)
    max_passes = N * N if max_passes is None else int(max_passes)
    if not 2 <= int(m_seed) <= m_end <= N:
        raise ValueError(f"need 2 <= m_seed = {m_seed} <= m_end = {m_end} <= N = {N}")
    if max_passes < 1:
        raise ValueError(f"max_passes = {max_passes} must be >= 1")
    if not _abi.tsp_grow_launch_form(N).supported:
        raise ValueError(f"N = {N} is beyond the LDS limit of rls_tsp_grow_2opt (rls_tsp_grow_launch_form)")
    if out is None:
        out = (torch.zeros((S, N), dtype=torch.int64, device=dev), torch.zeros(S, dtype=torch.float64, device=dev),
               torch.zeros(S, dtype=torch.int64, device=dev), torch.empty(S, dtype=torch.int32, device=dev))
    tours, length, passes, status = out
    _t.tsp_grow_2opt(dist64, order, int(m_seed), m_end, int(first_m), max_passes, tours, length, passes, status)
    return tours, length, passes, status
