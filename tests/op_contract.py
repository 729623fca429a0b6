"""One small VALID call per torch.ops.rlsolver_hip op: the table the refusal sweep of tests/test_gpu_op_contract.py mutates.

A row is a function that returns the op's full positional argument list.  Argument names, kinds and which arguments an op
writes come from the op's own schema (``names`` / ``tensor_names`` / ``written``), never from a restatement here.  Most rows
call the package's own Python wrapper and take the arguments at the moment the wrapper hands them to the op (``tap``: the op is
not run, so in / out tensors still hold their inputs); rows of ops without a wrapper give the arguments directly.  Shapes are
small but not degenerate: about 70 nodes (no multiple of 16), 5 or 65 envs / chains.

``outs``: the written arguments a call never reads (results only).  The sweep fills them with a pattern before every call, so a
kernel that runs although it should have been refused always changes them.  ``fix``: the spin-system ops take a handle of a host
struct that holds the address of ``state``; the sweep moves every tensor into guard-banded memory, and ``fix(op, args)`` returns the
arguments with the handle of a copy of the struct that names the moved ``state``.
"""
import contextlib
import ctypes
import functools

import numpy as np
import torch

from rlsolver_amd import torch_ops

DEV = torch.device("cuda:0")
N, B, C = 70, 5, 65            # nodes, envs, chains: no multiple of 16 / of the 64-chain tile


# ---------------------------------------------------------------------------------------------------------------- schema
def schema(op):
    return getattr(torch.ops.rlsolver_hip, op).default._schema


def names(op):
    return [a.name for a in schema(op).arguments]


def kinds(op):
    """name -> 'Tensor' | 'Optional[Tensor]' | 'int' | 'float' | 'bool', as the schema states it"""
    return {a.name: str(a.type) for a in schema(op).arguments}


def tensor_names(op):
    return [n for n, k in kinds(op).items() if k in ("Tensor", "Optional[Tensor]")]


def written(op):
    return [a.name for a in schema(op).arguments if a.alias_info is not None and a.alias_info.is_write]


def bind(op, args, kwargs=None):
    """positional / keyword arguments -> the full positional list, schema defaults filled in"""
    kwargs = dict(kwargs or {})
    out = list(args)
    for a in schema(op).arguments[len(args):]:
        if a.name in kwargs:
            out.append(kwargs.pop(a.name))
        else:
            assert a.has_default_value(), f"{op}: argument {a.name} is missing"
            out.append(a.default_value)
    assert not kwargs and len(out) == len(schema(op).arguments), (op, kwargs)
    return out


def call(op, args):
    return getattr(torch_ops.ops, op)(*args)


# ---------------------------------------------------------------------------------------------------------------- the tap
class _Taken(BaseException):
    pass


@contextlib.contextmanager
def tap(op):
    """Inside the block the package's wrappers reach every op but `op`: its first call is bound to the schema, recorded in the
    yielded dict under "args" and ends the block (the op itself does not run)."""
    rec = torch_ops.ops
    assert hasattr(rec, "_ns"), "RLS_RECORD_OPS=1 must be set before rlsolver_amd is imported (tests/conftest.py does)"
    real, box = rec._ns, {}

    class Namespace:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != op:
                return fn

            def take(*a, **k):
                box["args"] = bind(op, a, k)
                raise _Taken()
            return take

    rec._ns = Namespace()
    try:
        yield box
    except _Taken:
        pass
    finally:
        rec._ns = real
    assert "args" in box, f"the wrapper never called {op}"


def taken(op, fn):
    with tap(op) as box:
        fn()
    return box["args"]


# ---------------------------------------------------------------------------------------------------------------- the table
class Row:
    def __init__(self, op, build, outs, repeatable):
        self.op, self._build, self.outs, self.repeatable = op, build, tuple(outs), repeatable

    def valid_call(self):
        """-> (argument list, names of the written arguments, fix or None)"""
        got = self._build()
        args, fix = got if isinstance(got, tuple) else (got, None)
        assert len(args) == len(names(self.op)), self.op
        assert set(self.outs) <= set(written(self.op)), (self.op, self.outs)
        return list(args), written(self.op), fix


ROWS = {}       # op -> its row
ALL = {}        # "op" and "op#variant" -> row: a variant passes the optional tensors the op's first row leaves out
KEEP = []      # what owns the host structs behind the integer handles of the recorded calls (a graph dies with its sampler)


def row(op, outs=(), repeatable=True, variant=None):
    """repeatable=False: the op also changes state behind a handle, so a second valid call need not repeat the first"""
    def deco(fn):
        key = op if variant is None else f"{op}#{variant}"
        assert key not in ALL and (variant is None or op in ROWS), key
        ALL[key] = Row(op, fn, outs, repeatable)
        if variant is None:
            ROWS[op] = ALL[key]
        return fn
    return deco


def given(op, args, name, tensor):
    """`args` with the optional argument `name`, which the wrapper left out at this size, set to `tensor`"""
    i = names(op).index(name)
    if args[i] is None:
        args[i] = tensor
    return args


def some_scratch(nbytes=4096):
    return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x if dtype is None else x.to(dtype)


def rng(seed):
    return np.random.RandomState(seed)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
def _ops():
    from rlsolver_amd import ops
    return ops


def _mops():
    from rlsolver_amd import ops_mcpg_tsp
    return ops_mcpg_tsp


LS_N = 72                      # the fused local search wants rows of x that start 4-byte aligned: a multiple of 4, still none of 16


@functools.lru_cache(maxsize=None)
def graph_edges(n=N):
    from tests.gpu_util import gnm_arr
    return gnm_arr(n, 230, 3)


@functools.lru_cache(maxsize=None)
def graph(n=N):
    from tests.gpu_util import device_graph
    return device_graph(graph_edges(n), n, 0)


def spins(rows=B, seed=1, n=N):
    return _ops().rand_spins(rows, n, seed, DEV)


def cut_of(xs):
    return _ops().maxcut_obj(graph(xs.shape[1]), xs)


@functools.lru_cache(maxsize=None)
def ls_inputs(n=N):
    """(xs, ws int8 padded, rd_std f32, obj, thresh) of the local-search round kernels, computed by the kernels themselves"""
    o, g = _ops(), graph(n)
    xs = spins(n=n)
    ws, std = o.maxcut_ls_weights(g, xs, 4, dtype=torch.int8, padded=True)
    rd_std = std.to(torch.float32).contiguous()
    thresh = o.maxcut_ls_threshold(g, ws, rd_std, seed=7, num_spin=4)
    return xs, ws, rd_std, cut_of(xs), thresh


# ---------------------------------------------------------------------------------------------------------------- MaxCut
@row("maxcut_obj", outs=("obj",))
def _():
    return taken("maxcut_obj", lambda: _ops().maxcut_obj(graph(), spins()))


@row("maxcut_edge_cut_mask", outs=("mask",))
def _():
    return taken("maxcut_edge_cut_mask", lambda: _ops().maxcut_edge_cut_mask(graph(), spins()))


@row("maxcut_node_cutdeg", outs=("out",))
def _():
    return taken("maxcut_node_cutdeg", lambda: _ops().maxcut_node_cutdeg(graph(), spins()))


@row("maxcut_delta_all", outs=("out",))
def _():
    return taken("maxcut_delta_all", lambda: _ops().maxcut_delta_all(graph(), spins()))


@row("maxcut_step", outs=("reward",))
def _():
    xs = spins()
    z = lambda: torch.zeros(B, dtype=torch.float32, device=DEV)       # noqa: E731
    return taken("maxcut_step", lambda: _ops().maxcut_step(graph(), xs, xs.clone(), _ops().rand_actions(B, N, 5, 0, DEV),
                                                           cut_of(xs).to(torch.int32), z(), z(), z(), 3.0))


@row("maxcut_greedy_sweep")
def _():
    xs = spins()
    return taken("maxcut_greedy_sweep", lambda: _ops().maxcut_greedy_sweep(graph(), xs.clone(), cut_of(xs)))


@row("maxcut_propose_accept")
def _():
    xs = spins()
    mask = torch.rand((B, N), device=DEV) < 0.1
    return taken("maxcut_propose_accept", lambda: _ops().maxcut_propose_accept(graph(), xs.clone(), mask, cut_of(xs)))


@row("maxcut_ls_weights", outs=("ws_minmax",))
def _():
    return taken("maxcut_ls_weights", lambda: _ops().maxcut_ls_weights(graph(), spins(), 4, dtype=torch.int8, padded=True))


@row("maxcut_local_search")
def _():
    xs, ws, rd_std, obj, _ = ls_inputs(LS_N)
    noise = torch.randn((3, B, LS_N), device=DEV)
    return taken("maxcut_local_search", lambda: _ops().maxcut_local_search(graph(LS_N), xs.clone(), ws, rd_std, obj.clone(), 2, 4, noise=noise,
                                                                           seed=7, compute_obj=True))


@row("maxcut_ls_normals", outs=("out",))
def _():
    return taken("maxcut_ls_normals", lambda: _ops().maxcut_ls_normals(B, N, 7, 1, DEV))


@row("maxcut_ls_threshold", outs=("thresh",))
def _():
    xs, ws, rd_std, _, _ = ls_inputs()
    args = taken("maxcut_ls_threshold", lambda: _ops().maxcut_ls_threshold(graph(), ws, rd_std, seed=7, num_spin=4,
                                                                           scratch=_ops().ls_scratch(graph(), B, ws)))
    return given("maxcut_ls_threshold", args, "scratch", some_scratch())


@row("maxcut_ls_propose")
def _():
    xs, ws, rd_std, obj, thresh = ls_inputs()
    args = taken("maxcut_ls_propose", lambda: _ops().maxcut_ls_propose(graph(), xs.clone(), ws, rd_std, thresh, obj.clone(), 7, 0,
                                                                       scratch=_ops().ls_scratch(graph(), B, ws)))
    return given("maxcut_ls_propose", args, "scratch", some_scratch())


@row("maxcut_ls_rounds")
def _():
    xs, ws, rd_std, obj, thresh = ls_inputs()
    args = taken("maxcut_ls_rounds", lambda: _ops().maxcut_ls_rounds(graph(), xs.clone(), ws, rd_std, thresh, obj.clone(), 7, 0, 2,
                                                                     scratch=_ops().ls_scratch(graph(), B, ws, 2)))
    return given("maxcut_ls_rounds", args, "scratch", some_scratch())


# ---------------------------------------------------------------------------------------------------------------- rows and bests
@row("select_better_rows")
def _():
    a, b = spins(seed=1), spins(seed=2)
    return taken("select_better_rows", lambda: _ops().select_better_rows(a.clone(), cut_of(a), b, cut_of(b)))


@row("pick_best_of_repeats", outs=("good_xs", "good_vs"))
def _():
    xs = spins(rows=65)
    return taken("pick_best_of_repeats", lambda: _ops().pick_best_of_repeats(xs, cut_of(xs), 5))


def _copy_rows_args(op):
    xs = spins()
    move = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)       # noqa: E731
    return bind(op, [xs.clone(), cut_of(xs), move([1, 3]), move([0, 4])])


@row("copy_rows")
def _():
    return _copy_rows_args("copy_rows")


@row("copy_rows_bounded")
def _():
    return _copy_rows_args("copy_rows_bounded")


@row("best_update")
def _():
    xs = spins()
    return bind("best_update", [xs, cut_of(xs), True, torch.zeros(N, dtype=torch.bool, device=DEV),
                                torch.full((1,), -1.0, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.uint8, device=DEV),
                                torch.zeros(4, dtype=torch.float64, device=DEV), 3, False])


@row("best_key")
def _():
    z = lambda dt: torch.zeros(1, dtype=dt, device=DEV)       # noqa: E731
    return bind("best_key", [cut_of(spins()), 20, 5, 1 << 40, z(torch.int64), z(torch.int64), z(torch.int32)])


@row("key_unpack")
def _():
    z = lambda dt: torch.zeros(1, dtype=dt, device=DEV)       # noqa: E731
    key = torch.tensor([(37 << 20) | 5], dtype=torch.int64, device=DEV)
    return bind("key_unpack", [key, 20, 8, z(torch.int64), z(torch.int64), -1, z(torch.int32)])


def _winner_message_args():
    key = torch.tensor([(37 << 20) | 5], dtype=torch.int64, device=DEV)
    index = torch.tensor([2], dtype=torch.int64, device=DEV)
    return bind("winner_message", [spins(), index, key, 20, 5, 1 << 33, N, torch.zeros(8 + (N + 7) // 8, dtype=torch.uint8, device=DEV)])


@row("winner_message", outs=("msg",))
def _():
    return _winner_message_args()


@row("winner_unpack", outs=("x_out", "index_out"))
def _():
    a = _winner_message_args()
    call("winner_message", a)
    return bind("winner_unpack", [a[-1], N, torch.zeros(N, dtype=torch.bool, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)])


# ---------------------------------------------------------------------------------------------------------------- generators
@row("rand_spins", outs=("x",))
def _():
    return taken("rand_spins", lambda: spins())


@row("rand_spins_repeats", outs=("x",))
def _():
    return taken("rand_spins_repeats", lambda: _ops().rand_spins_repeats([11, 12, 13], B, N, DEV))


@row("rand_actions", outs=("action",))
def _():
    return taken("rand_actions", lambda: _ops().rand_actions(B, N, 5, 2, DEV))


@row("rand_perms", outs=("perm",))
def _():
    return taken("rand_perms", lambda: _mops().rand_perms(B, N, 5, DEV))


@row("rand_couplings", outs=("matrix",))
def _():
    from rlsolver_amd.envs.util_envs_PECO import RandomERGraphGenerator
    gg = RandomERGraphGenerator(n_spins=N, p_connection=0.2, num_envs=B, device=DEV)
    return taken("rand_couplings", lambda: gg.get(seed=3))


@row("sub_set_sampling", outs=("xs_out", "probs_out"))
def _():
    probs = torch.rand((B, N), device=DEV)
    uni = torch.rand((3 * B, N), device=DEV)
    return taken("sub_set_sampling", lambda: _ops().sub_set_sampling(probs, spins(), 3, 7, uniforms=uni, seed=9))


# ---------------------------------------------------------------------------------------------------------------- S2V_PPO
S2V_SIZES = (9, 30, 70, 17, 65)


def s2v_env(sizes=S2V_SIZES, tenure=3, seed=1):
    from rlsolver_amd.envs.env_S2V_PPO import VecEnvMaxcut
    from tests import s2vppo_oracle as orc
    from tests.s2vppo_checks import cfg, gd
    graphs = [orc.random_graph(rng(100 + n), n, 2 * n, "unit") + (n,) for n in sizes]
    return VecEnvMaxcut([gd(*g) for g in graphs], cfg(tenure), seed=seed)


@row("s2vppo_step", outs=("reward", "done"))
def _():
    env = s2v_env()
    act = torch.tensor([n // 2 for n in S2V_SIZES], dtype=torch.int64, device=DEV)
    return taken("s2vppo_step", lambda: env.step(act))


@row("s2vppo_reset")
def _():
    env = s2v_env()
    z0 = rng(4).choice(np.array([-1, 1], dtype=np.int8), size=sum(S2V_SIZES))
    return taken("s2vppo_reset", lambda: env.reset(ids=[3, 1], z0=z0, greedy=[True, False, True, False, True]))


# ---------------------------------------------------------------------------------------------------------------- spin system
def _spin_fix(env):
    keep = []

    def fix(op, args):
        nm = names(op)
        moved = type(env._env).from_buffer_copy(env._env)
        moved.state = args[nm.index("state")].data_ptr()
        keep.append(moved)
        args = list(args)
        args[nm.index("env")] = ctypes.addressof(moved)
        return args
    fix.keep = (env, keep)
    return fix


def spin_env(dense):
    from rlsolver_amd.envs.spinsystem import SpinSystem
    from rlsolver_amd.graph import generate_gnm
    if dense:
        from rlsolver_amd.envs.util_envs_PECO import RandomERGraphGenerator
        torch.manual_seed(5)
        return SpinSystem(None, None, B, max_steps=10, device=DEV,
                          graph_generator=RandomERGraphGenerator(n_spins=N, p_connection=0.2, num_envs=B, device=DEV))
    torch.manual_seed(5)
    return SpinSystem(generate_gnm(N, 230, 3), N, B, max_steps=10, device=DEV)


def _spin_row(op, dense, act):
    env = spin_env(dense)
    return taken(op, lambda: act(env)), _spin_fix(env)


def _spin_action():
    return torch.arange(B, dtype=torch.int64, device=DEV) * 7 + 1


@row("spin_reset", repeatable=False)
def _():
    return _spin_row("spin_reset", False, lambda env: env.reset())


@row("spin_step", repeatable=False)
def _():
    return _spin_row("spin_step", False, lambda env: env.step(_spin_action()))


@row("spin_observation", outs=("out",), repeatable=False)
def _():
    return _spin_row("spin_observation", False, lambda env: env.get_observation())


def _stale_state(env):
    env.step(_spin_action())
    return env.state


@row("spin_materialize", repeatable=False)
def _():
    return _spin_row("spin_materialize", False, _stale_state)


@row("spin_reset_dense", repeatable=False)
def _():
    return _spin_row("spin_reset_dense", True, lambda env: env.reset())


@row("spin_step_dense", repeatable=False)
def _():
    return _spin_row("spin_step_dense", True, lambda env: env.step(_spin_action()))


# ---------------------------------------------------------------------------------------------------------------- MCPG
@functools.lru_cache(maxsize=None)
def mcpg_data():
    from rlsolver_amd.methods import MCPG
    g = graph_edges()
    return MCPG.make_data(N, g[:, 0].copy(), g[:, 1].copy(), DEV)


def chains(seed=2, c=C, n=N):
    return t((rng(seed).rand(n, c) < 0.5).astype(np.float32))


def packed(seed=2, c=C, n=N):
    return _mops().PackedChains.pack(chains(seed, c, n))


@row("mcpg_metro_rounds")
def _():
    r, T = rng(6), 3
    index, u = t(r.randint(0, N, size=(T, C)).astype(np.int64)), t(r.rand(T, C).astype(np.float32))
    lim = torch.full((1,), T, dtype=torch.int64, device=DEV)
    acc = torch.zeros(T, dtype=torch.int64, device=DEV)
    return taken("mcpg_metro_rounds", lambda: _mops().mcpg_metro_rounds(chains(), t(r.rand(N).astype(np.float32)), T, index, u, t_limit=lim,
                                                                        accepts=acc))


@row("mcpg_metro_rounds", variant="packed")
def _():
    """bit-packed chains read from samples_in, with the scratch of the draw windows"""
    r, T = rng(16), 3
    index, u = t(r.randint(0, N, size=(T, C)).astype(np.int64)), t(r.rand(T, C).astype(np.float32))
    lim = torch.full((1,), T, dtype=torch.int64, device=DEV)
    acc = torch.zeros(T, dtype=torch.int64, device=DEV)
    args = taken("mcpg_metro_rounds", lambda: _mops().mcpg_metro_rounds(packed(5), t(r.rand(N).astype(np.float32)), T, index, u, t_limit=lim,
                                                                        accepts=acc, samples_in=packed(6)))
    return given("mcpg_metro_rounds", args, "scratch", some_scratch())


@row("mcpg_metro_stop")
def _():
    acc = t(rng(7).randint(0, 9, size=(2, 3)).astype(np.int64))
    io = torch.zeros(4, dtype=torch.int64, device=DEV)
    return taken("mcpg_metro_stop", lambda: _mops().mcpg_metro_stop(acc, 11, 1, 3, io[:3].clone(), io[3:].clone()))


@row("mcpg_local_search", outs=("xs_out", "expected"))
def _():
    d = mcpg_data()
    uni = t(rng(8).rand(2, N, C).astype(np.float32))
    return taken("mcpg_local_search", lambda: _mops().mcpg_local_search(d.graph, chains(), d._order_i32, 2, uni, 0, visit_stream=d._visit_stream))


@row("mcpg_local_search", outs=("xs_out", "expected"), variant="weighted")
def _():
    """the weighted sampler: edge_weights, the weighted visit stream and the gauge node"""
    from rlsolver_amd.methods import MCPG_maxcut
    d = MCPG_maxcut.make_data(N, *_weighted_graph(), DEV)
    KEEP.append(d)
    uni = t(rng(8).rand(2, N, C).astype(np.float32))
    return taken("mcpg_local_search", lambda: _mops().mcpg_local_search(d.graph, chains(), d._order_i32, 2, uni, 0, visit_stream=d._visit_stream,
                                                                        edge_weights=d._edge_w, gauge_node=int(d.sorted_degree_nodes[0])))


@row("mcpg_local_search_levels", outs=("xs_out", "expected"))
def _():
    d = mcpg_data()
    coins = t(rng(9).randint(0, 1 << 62, size=(2 * N, (C + 63) // 64)).astype(np.int64))
    return taken("mcpg_local_search_levels", lambda: _mops().mcpg_local_search_levels(d.graph, chains(), d._lv_ptr, d._lv_data, 2, 0, coins=coins))


@row("mcpg_pick_best", outs=("best_index", "vs_good", "xs_good"))
def _():
    M, R = 13, 5
    return taken("mcpg_pick_best", lambda: _mops().mcpg_pick_best(t(rng(10).randn(M * R).astype(np.float32)), chains(c=M * R), M, R, 230))


@row("mcpg_merge_best", outs=("mask_scratch", "best_value", "best_index"))
def _():
    r = rng(11)
    return taken("mcpg_merge_best", lambda: _mops().mcpg_merge_best(t(r.randn(N).astype(np.float32)), packed(3, c=N), t(r.randn(N).astype(np.float32)),
                                                                    packed(4, c=N)))


@row("mcpg_value_bit_sums")
def _():
    return taken("mcpg_value_bit_sums", lambda: _mops().mcpg_value_bit_sums(packed(), t(rng(12).randn(C).astype(np.float32))))


@row("mcpg_pack_chains", outs=("packed",))
def _():
    return taken("mcpg_pack_chains", lambda: packed())


@row("mcpg_unpack_chains", outs=("xs",))
def _():
    p = packed()
    return taken("mcpg_unpack_chains", lambda: p.unpack())


def _qubo():
    r = rng(13)
    Q = (r.randint(-9, 10, size=(N, N)) * (r.rand(N, N) < 0.2)).astype(np.float32)
    return t(np.triu(Q) + np.triu(Q, 1).T)


@row("qubo_local_search_value", outs=("xs_out", "value"))
def _():
    from rlsolver_amd.methods import MCPG_qubo as q
    return taken("qubo_local_search_value", lambda: q.qubo_local_search_value(_qubo(), chains(), 2, False))


@row("qubo_sparse_local_search_value", outs=("xs_out", "value"))
def _():
    from rlsolver_amd.methods import MCPG_qubo as q
    csr = q.qubo_to_csr(_qubo())
    return taken("qubo_sparse_local_search_value", lambda: q.qubo_sparse_local_search_value(csr, chains(), 2, False))


@row("maxsat_local_search", outs=("xs_out", "expected"))
def _():
    from rlsolver_amd.methods import MCPG_maxsat
    r = rng(70)
    clauses = [[int(v + 1) * (1 if r.rand() < 0.5 else -1) for v in r.choice(N, 3, replace=False)] for _ in range(300)]
    data = MCPG_maxsat.make_data(N, clauses, None, None, None, DEV, sorted_nodes=r.permutation(N))
    coins = t(r.randint(0, 1 << 62, size=(N, (C + 63) // 64)).astype(np.int64))
    return taken("maxsat_local_search", lambda: data.local_search(packed(), 1, coins=coins))


@row("maxsat_local_search", outs=("xs_out", "expected"), variant="weighted")
def _():
    from rlsolver_amd.methods import MCPG_maxsat
    r = rng(71)
    clauses = [[int(v + 1) * (1 if r.rand() < 0.5 else -1) for v in r.choice(N, 3, replace=False)] for _ in range(300)]
    data = MCPG_maxsat.make_data(N, clauses, [int(w) for w in r.randint(1, 6, size=300)], 1 << 24, None, DEV, sorted_nodes=r.permutation(N))
    coins = t(r.randint(0, 1 << 62, size=(N, (C + 63) // 64)).astype(np.int64))
    return taken("maxsat_local_search", lambda: data.local_search(packed(), 1, coins=coins))


def _weighted_graph():
    g, r = graph_edges(), rng(14)
    return g[:, 0].copy(), g[:, 1].copy(), r.randint(1, 4, size=len(g)).astype(np.int64)


@row("cheeger_local_search", outs=("xs_out", "h", "cut", "size"))
def _():
    from rlsolver_amd.methods import MCPG_cheeger
    data = MCPG_cheeger.make_data(N, *_weighted_graph(), DEV)
    KEEP.append(data)
    return taken("cheeger_local_search", lambda: data.local_search(packed(), 1))


@row("maxcut_edge_local_search", outs=("xs_out", "expected"))
def _():
    from rlsolver_amd.methods import MCPG_maxcut_edge
    eu, ev, w = _weighted_graph()
    data = MCPG_maxcut_edge.make_data(N, eu, ev, w, DEV)
    KEEP.append(data)
    uni = t(rng(15).rand(1, len(eu), 3, C).astype(np.float32))
    return taken("maxcut_edge_local_search", lambda: data.local_search(packed(), 1, uni))


@row("mimo_local_search", outs=("xs_out", "expected"))
def _():
    from tests import mimo_oracle
    Sigma, Diag, _, x01 = mimo_oracle.integer_case(40, 9, 128)[:4]
    pc = _mops().PackedChains
    return taken("mimo_local_search", lambda: _mops().mcpg_mimo_local_search(t(Sigma, torch.float32), t(Diag, torch.float32),
                                                                             pc.pack(t(x01, torch.float32)), 1, out=pc.empty(40, 128, DEV)))


# ---------------------------------------------------------------------------------------------------------------- TSP
TSP_K = 5


@functools.lru_cache(maxsize=None)
def tsp_env():
    from rlsolver_amd.envs.env_ISCO import ISCO_TSP
    from tests import tsp_cases
    dist, near, rnd = tsp_cases.circle_instance(N, TSP_K)
    return ISCO_TSP({"num_nodes": N, "distance": t(np.array(dist)), "nearest_indices": t(np.array(near)), "random_indices": t(np.array(rnd))},
                    batch_size=B, K=TSP_K, device=DEV)


def far_table():
    """the N - K - 1 columns of `random` the draws use, and not one more: a column less is then a table too narrow"""
    return tsp_env()._rand32[:, :N - TSP_K - 1].contiguous()


def tours(seed=3):
    return t(np.stack([rng(seed + b).permutation(N) for b in range(B)]).astype(np.int64))


@row("tsp_tour_length", outs=("length",))
def _():
    return taken("tsp_tour_length", lambda: _mops().tsp_tour_length(tsp_env().distance, tours()))


def _swap_call():
    s = tsp_env()
    return _mops().tsp_swap_delta_all(s.distance, tours(), None, 0.5, nearest=s._near32, random=far_table(), near_threshold=s._near_thr, seed=4,
                                      return_selected=True, tables8=s._tab8)


@row("tsp_swap_delta_all", outs=("selected_out", "logratio", "indices", "ban"))
def _():
    return taken("tsp_swap_delta_all", _swap_call)


@row("tsp_swap_delta_all", outs=("logratio", "indices", "ban"), variant="selected")
def _():
    """the recorded-draw form: the partner cities given"""
    selected = _swap_call()[3]
    return taken("tsp_swap_delta_all", lambda: _mops().tsp_swap_delta_all(tsp_env().distance, tours(), selected, 0.5))


@row("tsp_apply_swap")
def _():
    _, indices, _, _ = _swap_call()
    pos = t(rng(5).randint(0, N, size=B).astype(np.int64))
    return taken("tsp_apply_swap", lambda: _mops().tsp_apply_swap(tours(), pos, indices))


@row("tsp_2opt_delta", outs=("delta",))
def _():
    i, j = t(np.array([0, 3, 10, 20, 68], dtype=np.int64)), t(np.array([5, 4, 69, 40, 69], dtype=np.int64))
    return taken("tsp_2opt_delta", lambda: _mops().tsp_2opt_delta(tsp_env().distance, tours(), i, j))


@row("tsp_2opt_best", outs=("best_i", "best_value"))      # (of best_j only the first B entries are written when slices > 1)
def _():
    d64 = tsp_env().distance.to(torch.float64)
    p = tours()
    cur = _mops().tsp_tour_length(tsp_env().distance, p).to(torch.float64)
    return taken("tsp_2opt_best", lambda: _mops().tsp_2opt_best(d64, p, cur, slices=2))


@row("isco_tsp_step", outs=("perm_out", "log_acc_out", "acc_out", "cur_out"))
def _():
    from tests import tsp_cases
    draws = {k: torch.from_numpy(v) for k, v in tsp_cases.recorded_draws(rng(6), 2, B, N, TSP_K).items()}
    args = taken("isco_tsp_step", lambda: tsp_env().step(tours(), 2, 0.5, draws=draws, want_terms=True))
    args[names("isco_tsp_step").index("random")] = far_table()
    return args


# ---------------------------------------------------------------------------------------------------------------- ISCO flip steps
def flip_draws(seed, b, n):
    r = rng(seed)
    return {"u_gumbel": torch.from_numpy(r.rand(b, n).astype(np.float32).clip(1e-7, 1 - 1e-7)), "u_accept": torch.from_numpy(r.rand(b).astype(np.float32))}


def graph_params(g, n):
    return {"num_nodes": n, "num_edges": len(g), "edge_from": t(g[:, 0].copy()), "edge_to": t(g[:, 1].copy())}


def _flip_row(op, cls):
    s = cls(graph_params(graph_edges(), N), batch_size=B, device=DEV)
    KEEP.append(s)
    x = t(rng(7).randint(0, 2, size=(B, N)).astype(np.float32))
    pl = t(np.array([1, 7, 35, 3, 70], dtype=np.int64))
    args = taken(op, lambda: s.step(x, pl, 0.7, draws=flip_draws(8, B, N), want_terms=True))
    return given(op, args, "scratch", some_scratch(B * N * 8))       # (the rows fit LDS at this size: the kernel leaves it alone)


@row("isco_maxcut_step", outs=("y_out", "energy_out", "acc_out", "terms_out", "mask_out"))
def _():
    from rlsolver_amd.envs.env_ISCO_maxcut import ISCO_maxcut
    return _flip_row("isco_maxcut_step", ISCO_maxcut)


@row("isco_mis_step", outs=("y_out", "energy_out", "acc_out", "terms_out", "mask_out"))
def _():
    from rlsolver_amd.envs.env_ISCO_MIS import ISCO_MIS
    return _flip_row("isco_mis_step", ISCO_MIS)


@functools.lru_cache(maxsize=None)
def pisco_adj():
    from tests import pisco_oracle as po
    return po.dense_graph(N, 0.1, 2, 21).astype(np.float16)            # [72, 72]: 70 nodes padded to a multiple of 8


def pisco_env(b=B, half=True):
    from rlsolver_amd.envs.env_PISCO_maxcut import PISCO_maxcut
    adj = pisco_adj()
    iu, ju = np.nonzero(np.triu(adj.astype(np.float64)))
    return PISCO_maxcut({"num_nodes": N, "num_edges": len(iu), "edge_from": t(iu), "edge_to": t(ju), "adj_matrix": t(adj)}, batch_size=b,
                        device=DEV, half_rounding=half)


def pisco_x(b=B, seed=9):
    return t((rng(seed).rand(b, pisco_adj().shape[0]) < 0.5).astype(np.float16))


@row("pisco_product", outs=("r_out",))
def _():
    return taken("pisco_product", lambda: _ops().pisco_product(t(pisco_adj()), pisco_x()))


@row("pisco_step", outs=("y_out", "energy_out", "acc_out", "terms_out", "mask_out"))
def _():
    s, Np = pisco_env(), pisco_adj().shape[0]
    pl = t(np.array([1, 7, 36, 3, 72], dtype=np.int64))
    return taken("pisco_step", lambda: s.step(pisco_x(), pl, 0.7, draws=flip_draws(10, B, Np), want_terms=True))
