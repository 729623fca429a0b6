"""The search body of the L2A policy step on HIP tensors -- drop-in for the functions of rlsolver/methods/L2A/transformer.py
that demo_instance.py:141-165 (and demo_distribution.py:160, transformer.py:385) run per step:

    probs -> sub_set_sampling -> num_searchers x local_search_inplace -> pick_xs_by_vs -> update_xs_by_vs -> record2

``sub_set_sampling`` is one kernel (rls_sub_set_sampling) where the reference runs two topk, a gather / scatter, a repeat and a
Python loop over top_k columns; ``search_step`` is that loop body on the kernels of this package, without a host read.
The policy and graph-embedding networks, the buffer and the PPO update stay with the caller.

Differences from the reference, all deliberate: ties of the determinism at the selection boundary go to the LOWER node index
(torch.topk leaves them unspecified); the draws come from the counter-based generator keyed by (seed, repeat, global sim id,
node), so a rank that holds sims [off, off + S_local) and passes ``env_offset = off`` computes exactly its rows of the one-process
result; ``device`` must be a HIP device.
"""
from __future__ import annotations

from typing import Optional

import torch as th

from .. import ops
from ..seeding import seed_from_torch
from .util_read_data import update_xs_by_vs

TEN = th.Tensor


def convert_solution_to_prob(solution_xs: TEN) -> TEN:
    """transformer.py:41-48: bool [num_sims, num_nodes] -> int64 [num_nodes, num_sims, 2]; entry (n, s) holds (+1, -1) where
    the spin is set and (-1, +1) where it is not."""
    spins = solution_xs.t().to(th.int64) * 2 - 1
    return th.stack((spins, -spins), dim=-1)


def sub_set_sampling(probs: TEN, start_xs: TEN, num_repeats: int, top_k: int, *, uniforms: Optional[TEN] = None,
                     seed: Optional[int] = None, env_offset: int = 0, out: Optional[TEN] = None) -> (TEN, TEN):
    """transformer.py:335-353 -> (xs bool [num_repeats * S, N], probs f32 [S, N]); neither input is modified.
    The min(top_k, N) least determined nodes of each sim (smallest |probs - 0.5|, ties to the lower node index) are redrawn in
    every repeat as ``u < |probs - 0.5|`` -- the reference's Bernoulli parameter is the determinism --, every other node keeps
    ``start_xs``; the returned probs keep the input at the redrawn nodes and are ``1.0 if p < 0.5 else 0.0`` elsewhere.
    ``uniforms`` f32 [num_repeats * S, N] replaces the draws (only the redrawn entries are read); ``seed`` None takes one from
    torch's CPU generator; ``out`` receives xs."""
    probs = probs.to(th.float32).contiguous()          # callers pass seq_prob[:, :, 0]
    start_xs = start_xs.contiguous()
    if seed is None:
        seed = 0 if uniforms is not None else seed_from_torch()
    return ops.sub_set_sampling(probs, start_xs, num_repeats, top_k, uniforms=uniforms, seed=seed, env_offset=env_offset, out=out)


def search_step(sim, probs: TEN, best_xs: TEN, best_vs: TEN, num_repeats: int, top_k: int, num_searchers: int, evaluator=None,
                iter_i=0, *, uniforms: Optional[TEN] = None, noise=None):
    """The body of demo_instance.py:148-165 for one t: candidates around ``best_xs`` from ``probs``, ``num_searchers`` local
    searches on them, the best repeat of every sim, then ``best_xs`` / ``best_vs`` updated IN PLACE where a sim improved (ties
    accepted) and ``evaluator.record2(i=iter_i, ...)`` when an evaluator is given.
    -> (curr_xs, curr_vs, rewards): the state before the update and ``best_vs - curr_vs``.
    ``sim`` (envs.env_L2A.EnvMaxcut) supplies the seed stream and ``env_offset``.  Nothing here reads the device back.
    Test hooks: ``uniforms`` for sub_set_sampling, ``noise`` = one local_search_inplace noise tensor per searcher."""
    if num_searchers < 1:
        raise ValueError("search_step needs num_searchers >= 1 (the reference picks by the last searcher's values)")
    maximize = bool(sim.if_maximize)
    draw_seed = 0 if uniforms is not None else sim._next_seed()
    cand_xs, _ = sub_set_sampling(probs, best_xs, num_repeats, top_k, uniforms=uniforms, seed=draw_seed, env_offset=sim.env_offset)
    cand_vs = th.empty(())                                   # 0-dim: "compute the values" for the first searcher
    for k in range(num_searchers):
        cand_xs, cand_vs = sim.local_search_inplace(cand_xs, cand_vs, noise=None if noise is None else noise[k])
    winner_xs, winner_vs = ops.pick_best_of_repeats(cand_xs, cand_vs, num_repeats, maximize)
    before_xs, before_vs = best_xs.clone(), best_vs.clone()
    update_xs_by_vs(best_xs, best_vs, winner_xs, winner_vs, maximize)
    if evaluator is not None:
        evaluator.record2(iter_i, best_vs, best_xs)
    return before_xs, before_vs, best_vs - before_vs
