"""MaxCut consumers on the graph forms a file may hold: self loops (also on a node with no other edge, and repeated),
the same edge repeated in the same and in the opposite orientation, lines with n0 > n1, and shuffled line order.

The reference takes an edge list as it is given (util_read_data.py:144-187, MCPG.py:235-252, the autograd energy of
env_ISCO.py), and so does the oracle; every test here compares a HIP path with it (or with a vectorised numpy restatement
where the oracle's literal re-evaluation is too slow), each form on its own and all of them together, in each kernel form
the dev knobs can force.  Widths: a hub whose loop puts its STORED degree one past the int8 / int16 limit, while its
symmetric degree stays inside it."""
import numpy as np
import pytest
import torch

from oracle import oracle_isco as oi
from oracle import oracle_np as onp
from tests.gpu_util import DEV, to_dev_bool
from tests.test_gpu_isco_steps import _maxcut_sampler

pytestmark = pytest.mark.gpu

KINDS = ("loops", "repeats", "reversed", "all")


def forms_graph(rng, n, m, kind):
    """int64 [E, 3] edge list of ``kind`` on nodes 0..n-1, every id appearing (the reference sizes its env by distinct
    endpoints).  "loops": loops, one of them twice and one on node n - 1, which has no other edge; "repeats": edges
    repeated in the same and in the opposite orientation; "reversed": about half the lines with n0 > n1; "all": all three.
    Line order shuffled."""
    loops, repeats, rev = kind in ("loops", "all"), kind in ("repeats", "all"), kind in ("reversed", "all")
    hi_id = n - 1 if loops else n            # node n - 1 keeps its loop only
    a = rng.randint(0, hi_id, size=m)
    b = rng.randint(0, hi_id, size=m)
    ok = a != b
    e = np.stack([np.minimum(a, b)[ok], np.maximum(a, b)[ok]], axis=1)
    covered = np.zeros(n, bool)
    covered[e.reshape(-1)] = True
    miss = np.flatnonzero(~covered[:hi_id])
    if miss.size:
        e = np.concatenate([e, np.stack([np.minimum(miss, (miss + 1) % hi_id), np.maximum(miss, (miss + 1) % hi_id)], 1)])
    if repeats:
        k = max(2, len(e) // 6)
        dup = e[rng.randint(0, len(e), size=k)].copy()
        dup[: k // 2] = dup[: k // 2, ::-1]                          # half of them in the opposite orientation
        e = np.concatenate([e, dup])
    if rev:
        flip = rng.rand(len(e)) < 0.5
        e[flip] = e[flip, ::-1]
    if loops:
        li = rng.choice(hi_id, size=max(2, n // 8), replace=False)
        e = np.concatenate([e, np.stack([li, li], 1), [[li[0], li[0]], [n - 1, n - 1]]])
    e = e[rng.permutation(len(e))]
    return np.concatenate([e, np.ones((len(e), 1), np.int64)], axis=1).astype(np.int64)


def mygraph(g):
    return [tuple(int(v) for v in r) for r in g]


def stored_cutdeg(xb, g, n, bidir):
    """K2 restated over the stored adjacency, vectorised: int64 [B, N]."""
    u, v = onp.stored_edges(g, bidir)
    d = (xb[:, u] ^ xb[:, v]).astype(np.int64)
    out = np.zeros((xb.shape[0], n), np.int64)
    np.add.at(out.T, u, d.T)
    return out


def flip_gain(xb, g, n):
    """K3 restated: cut(flip_i(x)) - cut(x) from the edge list (a loop never changes), vectorised: int64 [B, N]."""
    u, v = g[:, 0], g[:, 1]
    keep = u != v
    u, v = u[keep], v[keep]
    s = np.where(xb[:, u] == xb[:, v], 1, -1).astype(np.int64)
    out = np.zeros((xb.shape[0], n), np.int64)
    np.add.at(out.T, u, s.T)
    np.add.at(out.T, v, s.T)
    return out


# knob settings: the launcher's own choice, and each tile form forced (test_gpu_tile32.py, test_gpu_full_size.py)
FORMS = {
    "auto": {},
    "tile32": {"RLS_K1_TILE32": 1, "RLS_K5_TILE32": 1, "RLS_K6_TILE32": 1, "RLS_NS_TILE32": 1},
    "narrow16": {"RLS_NARROW_TILE": 2, "RLS_NODE_STATS_MIN_B": 0},
    "narrow8": {"RLS_NARROW_TILE": 3, "RLS_NODE_STATS_MIN_B": 0},
    "tile64": {"RLS_NARROW_TILE": 0, "RLS_K1_TILE32": 0, "RLS_K5_TILE32": 0, "RLS_K6_TILE32": 0, "RLS_NS_TILE32": 0,
               "RLS_NODE_STATS_MIN_B": 0},
    "elem": {"RLS_NODE_STATS_MIN_B": 1 << 40},
}


class forced:
    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        from rlsolver_amd import _abi
        for k, v in self.knobs.items():
            _abi.tuning_set(k, v)

    def __exit__(self, *exc):
        from rlsolver_amd import _abi
        for k in self.knobs:
            _abi.tuning_unset(k)


# ------------------------------------------------------------------------------------------ K1 / K2 / K3 / K6 / K5
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,B", [(63, 65), (64, 1), (65, 130), (129, 63), (1000, 65), (20300, 63)])
@pytest.mark.parametrize("bidir", [False, True])
def test_node_kernels_vs_oracle(form, kind, n, B, bidir):
    """K1 (objective over the stored edges), K2 (stored cut degree, n0_num_n1), K3 (flip gain), the local-search weights
    with their min / max table, K6 (propose / accept) and K5 (greedy sweep; literal oracle on the first rows)."""
    from rlsolver_amd import ops
    from rlsolver_amd.envs.env_L2A import EnvMaxcut
    rng = np.random.RandomState(n * 7 + B + KINDS.index(kind) + 100 * bidir)
    g = forms_graph(rng, n, 2 * n, kind)
    assert onp.num_nodes_distinct(g) == n
    env = EnvMaxcut(mygraph=mygraph(g), device=DEV, if_bidirectional=bidir)     # sized by distinct endpoints, as the reference
    assert env.num_nodes == n
    u, _ = onp.stored_edges(g, bidir)
    deg_st = np.bincount(u, minlength=n)
    assert np.array_equal(env.n0_num_n1.cpu().numpy()[0], deg_st)
    xb = rng.randint(0, 2, size=(B, n)).astype(bool)
    xb[0] = False                                    # every ws at its largest
    xs = to_dev_bool(xb)
    g_ = env.graph
    with forced(FORMS[form]):
        if "RLS_NODE_STATS_MIN_B" in FORMS[form]:       # the forced node-stats family is the one that runs
            for sym in (True, False):
                assert (ops.node_stats_form(g_, B, sym) == "bits") == (form != "elem"), (form, sym)
        obj = env.calculate_obj_values(xs).cpu().numpy()
        cd = ops.maxcut_node_cutdeg(g_, xs).cpu().numpy()
        fl = env.calculate_obj_values_for_loop(xs).cpu().numpy()
        dl = ops.maxcut_delta_all(g_, xs).cpu().numpy()
        ws = {}
        for mult in ((1,) if bidir else (1, 2)):
            w, mm = ops.maxcut_ls_weights(g_, xs, mult, return_minmax=True)
            ws[mult] = (w.cpu().numpy(), mm.cpu().numpy(), w.dtype)
        mask = rng.rand(B, n) < 0.1
        x6 = xs.clone()
        v6 = torch.from_numpy(obj.copy()).to(DEV)
        ops.maxcut_propose_accept(g_, x6, to_dev_bool(mask), v6)
        x5, v5 = x6.clone(), v6.clone()
        ops.maxcut_greedy_sweep(g_, x5, v5)
    want_obj = onp.maxcut_obj(xb, g, bidir)
    assert np.array_equal(obj, want_obj)
    want_cd = stored_cutdeg(xb, g, n, bidir)
    assert np.array_equal(cd, want_cd)
    if n <= 129:
        assert np.array_equal(want_cd, onp.maxcut_node_cutdeg(xb, g, n, bidir))
        np.testing.assert_array_equal(fl, onp.maxcut_obj_for_loop(xb, g, n, bidir))
        assert np.array_equal(dl, onp.maxcut_delta_all(xb, g, n))
    else:
        assert np.array_equal(dl, flip_gain(xb, g, n))
    for mult, (w, mm, dt) in ws.items():
        want = deg_st[None, :] - mult * want_cd
        assert np.array_equal(w.astype(np.int64), want), (mult, dt)
        assert np.array_equal(mm, np.stack([want.min(axis=0), want.max(axis=0)])), mult
        span = int(np.abs(want).max())
        assert torch.iinfo(dt).max >= span, (dt, span)
    prop = xb ^ mask
    pv = onp.maxcut_obj(prop, g, bidir)
    take = pv >= want_obj
    assert np.array_equal(v6.cpu().numpy(), np.where(take, pv, want_obj))
    assert np.array_equal(x6.cpu().numpy(), np.where(take[:, None], prop, xb))
    rows = 2 if n <= 1000 else 0
    if rows:
        wx, wv = x6.cpu().numpy()[:rows].copy(), v6.cpu().numpy()[:rows].copy()
        onp.greedy_sweep(wx, wv, g, bidir)
        assert np.array_equal(x5.cpu().numpy()[:rows], wx) and np.array_equal(v5.cpu().numpy()[:rows], wv)
    assert np.array_equal(v5.cpu().numpy(), onp.maxcut_obj(x5.cpu().numpy(), g, bidir))


# ------------------------------------------------------------------------------------------ the whole local search
LS_FORMS = ("fused", "rounds", "decomposed")


def _ls_env(g, n, bidir, ls_form):
    from rlsolver_amd.envs.env_L2A import EnvMaxcut
    env = EnvMaxcut(mygraph=mygraph(g), device=DEV, if_bidirectional=bidir, num_nodes=n, seed=n + 17)
    env.fused_local_search = ls_form != "decomposed"
    env.force_ls_rounds = ls_form == "rounds"
    env.force_ls_fused = ls_form == "fused"
    return env


def run_ls(monkeypatch, env, xb, mult, num_iters, num_spin, ls_form, rng):
    """The local search in ``ls_form`` (mult 1: local_search_inplace, 2: LocalSearch.random_search) -> (xs, vs, the draws it
    used, f32 [draws, B, N]).  Asserts which path ran.  The fused and decomposed forms take supplied noise; the round kernels
    only exist for the kernels' own draws (env_L2A.py: noise=None), so that form runs seeded, and its draws are regenerated
    from the seed the threshold kernel was given (ops.maxcut_ls_normals: the same counter-based normals)."""
    from rlsolver_amd import ops
    from rlsolver_amd.methods.LocalSearch import LocalSearch
    calls, seeds = [], []
    for name in ("maxcut_local_search", "maxcut_ls_threshold", "maxcut_ls_rounds", "maxcut_propose_accept"):
        def wrap(*a, _orig=getattr(ops, name), _name=name, **k):
            calls.append(_name)
            if _name == "maxcut_ls_threshold":
                seeds.append(a[3])
            return _orig(*a, **k)
        monkeypatch.setattr(ops, name, wrap)
    B, n = xb.shape
    draws = num_iters + (1 if mult == 1 else 0)
    noise = None if ls_form == "rounds" else rng.randn(draws, B, n).astype(np.float32)
    nz = None if noise is None else torch.from_numpy(noise).to(DEV)
    try:
        if mult == 1:
            gx, gv = env.local_search_inplace(to_dev_bool(xb), torch.empty(()), num_iters=num_iters, num_spin=num_spin,
                                              noise_std=0.3, noise=nz)
        else:
            ls = LocalSearch(env, n)
            ls.reset(to_dev_bool(xb))
            gx, gv, _ = ls.random_search(num_iters=num_iters, num_spin=num_spin, noise_std=0.3, noise=nz)
    finally:
        monkeypatch.undo()
    ran = "fused" if "maxcut_local_search" in calls else "rounds" if "maxcut_ls_rounds" in calls else "decomposed"
    assert ran == ls_form, (ls_form, calls)
    if noise is None:
        assert len(seeds) == 1, calls
        noise = torch.stack([ops.maxcut_ls_normals(B, n, seeds[0], t, DEV) for t in range(draws)]).cpu().numpy()
    return gx.cpu().numpy(), gv.cpu().numpy(), noise


@pytest.mark.parametrize("ls_form", LS_FORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,B,num_iters", [(64, 65, 8), (128, 63, 0), (132, 1, 8)])
@pytest.mark.parametrize("bidir", [False, True])
def test_local_search_inplace_vs_oracle(monkeypatch, ls_form, kind, n, B, num_iters, bidir):
    rng = np.random.RandomState(n + B + 31 * KINDS.index(kind) + 7 * bidir)
    g = forms_graph(rng, n, 3 * n, kind)
    env = _ls_env(g, n, bidir, ls_form)
    xb = rng.randint(0, 2, size=(B, n)).astype(bool)
    gx, gv, noise = run_ls(monkeypatch, env, xb, 1, num_iters, 6, ls_form, rng)
    wx, wv = onp.local_search_inplace(xb, g, n, bidir, noise, num_iters=num_iters, num_spin=6)
    assert np.array_equal(gx, wx) and np.array_equal(gv, wv)


@pytest.mark.parametrize("ls_form", LS_FORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,B", [(64, 65), (132, 2)])
def test_random_search_vs_oracle(monkeypatch, ls_form, kind, n, B):
    """LocalSearch.random_search: weights n0_num_n1 - 2 * cut degree (unidirectional env: the reference raises otherwise)."""
    rng = np.random.RandomState(3 * n + B + KINDS.index(kind))
    g = forms_graph(rng, n, 3 * n, kind)
    env = _ls_env(g, n, False, ls_form)
    xb = rng.randint(0, 2, size=(B, n)).astype(bool)
    gx, gv, noise = run_ls(monkeypatch, env, xb, 2, 6, 5, ls_form, rng)
    wx, wv, _ = onp.local_search_class_random_search(xb.copy(), onp.maxcut_obj(xb, g, False), g, n, noise, 6, 5)
    assert np.array_equal(gx, wx) and np.array_equal(gv, wv)


# ------------------------------------------------------------------------------------------ entry widths
def hub_graph(rng, n, k, extra):
    """Node 0 with k neighbours stored as (0, j) plus a loop (0, 0); ``extra`` random edges among the other nodes."""
    e = [(0, j) for j in range(1, k + 1)] + [(0, 0)]
    a, b = rng.randint(1, n, size=extra), rng.randint(1, n, size=extra)
    e += [(int(x), int(y)) for x, y in zip(a, b) if x != y]
    e += [(j, j + 1) for j in range(k + 1, n - 1)]                   # (every id appears)
    e = np.asarray(e, np.int64)
    e = e[rng.permutation(len(e))]
    return np.concatenate([e, np.ones((len(e), 1), np.int64)], axis=1)


def _width_xs(rng, g, B, n):
    xb = rng.randint(0, 2, size=(B, n)).astype(bool)
    xb[0] = False                        # nothing cut: ws of the hub = its stored degree
    xb[1] = True
    xb[1, 0] = False                     # the hub against all its neighbours: ws = deg - mult * k
    return xb


@pytest.mark.parametrize("stored_deg", [126, 127, 128, 129])
@pytest.mark.parametrize("bidir,mult", [(False, 1), (True, 1), (False, 2)])
@pytest.mark.parametrize("ls_form", LS_FORMS)
def test_ls_width_at_the_int8_limit(monkeypatch, stored_deg, bidir, mult, ls_form):
    """A loop counts in the hub's stored degree (once, twice when bidirectional) but not in its symmetric one: the weights'
    entry type must follow the stored degree.  The whole local search against the oracle, in each of its three forms."""
    from rlsolver_amd import ops
    n, B = 160, 5
    rng = np.random.RandomState(stored_deg + 10 * mult + 100 * bidir)
    k = stored_deg - (2 if bidir else 1)
    g = hub_graph(rng, n, k, 120)
    env = _ls_env(g, n, bidir, ls_form)
    u, _ = onp.stored_edges(g, bidir)
    assert np.bincount(u, minlength=n)[0] == stored_deg
    xb = _width_xs(rng, g, B, n)
    ws, mm = ops.maxcut_ls_weights(env.graph, to_dev_bool(xb), mult, return_minmax=True)
    want = np.bincount(u, minlength=n)[None, :] - mult * stored_cutdeg(xb, g, n, bidir)
    assert int(want.max()) == stored_deg
    assert np.array_equal(ws.cpu().numpy().astype(np.int64), want), ws.dtype
    assert np.array_equal(mm.cpu().numpy(), np.stack([want.min(axis=0), want.max(axis=0)]))
    gx, gv, noise = run_ls(monkeypatch, env, xb, mult, 8, 8, ls_form, rng)
    if mult == 1:
        wx, wv = onp.local_search_inplace(xb, g, n, bidir, noise, num_iters=8, num_spin=8)
    else:
        wx, wv, _ = onp.local_search_class_random_search(xb.copy(), onp.maxcut_obj(xb, g, False), g, n, noise, 8, 8)
    assert np.array_equal(gx, wx) and np.array_equal(gv, wv)


@pytest.mark.parametrize("stored_deg", [32767, 32768])
@pytest.mark.parametrize("bidir,mult", [(False, 1), (True, 1), (False, 2)])
def test_ls_weights_width_at_the_int16_limit(stored_deg, bidir, mult):
    """The same at the int16 limit: ws and its min / max table against numpy int64 (the oracle's sweep is too slow here)."""
    from rlsolver_amd import ops
    n, B = stored_deg + 40, 3
    rng = np.random.RandomState(stored_deg + mult + 10 * bidir)
    k = stored_deg - (2 if bidir else 1)
    g = hub_graph(rng, n, k, 200)
    from rlsolver_amd.graph import build_csr
    csr = build_csr((g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()), num_nodes=n, if_bidirectional=bidir)
    dg = ops.DeviceGraph(csr, DEV)
    u, _ = onp.stored_edges(g, bidir)
    assert np.bincount(u, minlength=n)[0] == stored_deg
    xb = _width_xs(rng, g, B, n)
    ws, mm = ops.maxcut_ls_weights(dg, to_dev_bool(xb), mult, return_minmax=True)
    want = np.bincount(u, minlength=n)[None, :] - mult * stored_cutdeg(xb, g, n, bidir)
    assert int(want.max()) == stored_deg
    assert ws.dtype == (torch.int16 if stored_deg <= 32767 else torch.int32)
    assert np.array_equal(ws.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(mm.cpu().numpy(), np.stack([want.min(axis=0), want.max(axis=0)]))


# ------------------------------------------------------------------------------------------ K4
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("bidir", [False, True])
@pytest.mark.parametrize("n,B", [(65, 130), (1000, 63)])
def test_gym_step_vs_oracle(kind, f32, in_place, bidir, n, B):
    """K4, next state emitted or flipped in place, byte and f32 rows; actions include the loop nodes."""
    from rlsolver_amd import ops
    from rlsolver_amd.envs.env_L2A import EnvMaxcut
    rng = np.random.RandomState(n + B + KINDS.index(kind) + 2 * f32 + 4 * in_place + 8 * bidir)
    g = forms_graph(rng, n, 2 * n, kind)
    env = EnvMaxcut(mygraph=mygraph(g), device=DEV, if_bidirectional=bidir, num_nodes=n)
    loop_nodes = np.unique(g[g[:, 0] == g[:, 1], 0])
    xb = rng.randint(0, 2, size=(B, n)).astype(bool)
    obj = onp.maxcut_obj(xb, g, bidir)
    x = torch.from_numpy(xb.astype(np.float32)).to(DEV) if f32 else to_dev_bool(xb)
    o = torch.from_numpy(obj.astype(np.int32)).to(DEV)
    for step in range(4):
        a = rng.randint(0, n, size=B)
        if loop_nodes.size:
            a[: B // 2] = rng.choice(loop_nodes, size=B // 2)
        x_out = x if in_place else torch.empty_like(x)
        r = torch.empty(B, dtype=torch.float32, device=DEV)
        ops.maxcut_step(env.graph, x, x_out, torch.from_numpy(a).to(DEV), o, r)
        xb = xb.copy()
        xb[np.arange(B), a] ^= True
        nobj = onp.maxcut_obj(xb, g, bidir)
        got = x_out.cpu().numpy()
        assert np.array_equal(got > 0 if f32 else got, xb), step
        assert np.array_equal(o.cpu().numpy(), nobj) and np.array_equal(r.cpu().numpy(), (nobj - obj).astype(np.float32))
        obj, x = nobj, x_out


# ------------------------------------------------------------------------------------------ MCPG samplers
def _mcpg_graph(rng, n, kind):
    g = forms_graph(rng, n, 2 * n, kind)
    if n >= 100:                                     # a hub of degree > 128 (hub groups of the levels), with a loop where loops go
        hub = 1
        extra = np.array([(hub, j, 1) if j % 2 or kind not in ("reversed", "all") else (j, hub, 1)
                          for j in rng.choice(np.arange(2, n - 1), size=min(n - 3, 140), replace=False)])
        g = np.concatenate([g, extra] + ([[[hub, hub, 1]]] if kind in ("loops", "all") else []))
    return g


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,C,num_ls", [(17, 65, 2), (64, 1, 1), (130, 130, 3), (300, 63, 2)])
def test_mcpg_sampler_vs_oracle(kind, n, C, num_ls):
    """K7 by levels (tie coins), sequential with and without the visit stream, against the oracle's sequential pass:
    a loop lists the node twice among its own neighbours (append_neighbors), so its own value -- -0.5 | 1.5 in the first
    pass, before its own visit -- enters its sum twice."""
    from rlsolver_amd import ops_mcpg_tsp as mops
    from rlsolver_amd.methods import MCPG as amcpg
    rng = np.random.RandomState(50 * n + C + KINDS.index(kind))
    g = _mcpg_graph(rng, n, kind)
    ei = g[:, :2].T.copy()
    deg = np.bincount(ei.reshape(-1), minlength=n)
    order = np.argsort(-deg, kind="stable")
    data = amcpg.make_data(n, ei[0], ei[1], DEV, sorted_degree_nodes=order)
    xs0 = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    coin = rng.randint(0, 2, size=(num_ls, n, C)).astype(bool)
    uni = np.where(coin, 0.25, 0.75).astype(np.float32)
    _, _, _, x_all, exp_w = onp.sampler_func(ei, n, order, xs0, num_ls, C, 1, uni)
    x0 = torch.from_numpy(xs0).to(DEV)
    assert amcpg._levels_ok(data)
    CB = (C + 63) // 64
    bits = np.zeros((num_ls * n, CB * 64), dtype=np.uint64)
    bits[:, :C] = coin.reshape(num_ls * n, C)
    words = (bits.reshape(num_ls * n, CB, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    xs_l, exp_l = mops.mcpg_local_search_levels(data.graph, x0, data._lv_ptr, data._lv_data, num_ls, 0,
                                                coins=torch.from_numpy(words.view(np.int64)).to(DEV))
    assert np.array_equal(xs_l.cpu().numpy(), x_all) and np.array_equal(exp_l.cpu().numpy(), exp_w)
    for vs in (data._visit_stream, None):
        xs_s, exp_s = mops.mcpg_local_search(data.graph, x0, data._order_i32, num_ls, torch.from_numpy(uni).to(DEV), 0,
                                             visit_stream=vs)
        assert np.array_equal(xs_s.cpu().numpy(), x_all) and np.array_equal(exp_s.cpu().numpy(), exp_w), vs is None
    # the public sampler with recorded uniforms (coins from the reference's float32 rule) against the oracle's whole result
    M, R = (C, 1) if C < 2 else (C // 2, 2) if C % 2 == 0 else (C, 1)
    uni2 = rng.rand(num_ls, n, M * R).astype(np.float32)
    want = onp.sampler_func(ei, n, order, xs0[:, :M * R], num_ls, M, R, uni2)
    vs_g, xg_g, val_g = amcpg.sampler_func(data, x0[:, :M * R].contiguous(), num_ls, M, R, DEV, uniforms=torch.from_numpy(uni2).to(DEV))
    assert np.array_equal(vs_g.cpu().numpy(), want[0]) and np.array_equal(xg_g.cpu().numpy(), want[1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,M,R,num_ls", [(40, 16, 4, 2), (300, 64, 2, 1)])
def test_mcpg_weighted_sampler_vs_oracle(kind, n, M, R, num_ls):
    """The weighted sampler (rlsolver/methods/MCPG/sampling.py:89-127) with weights from {-2, -1, 1, 3} on the same lists."""
    from rlsolver_amd.methods import MCPG_maxcut as wm
    rng = np.random.RandomState(n + M + KINDS.index(kind))
    g = _mcpg_graph(rng, n, kind)
    g[:, 2] = rng.choice([-2, -1, 1, 3], size=len(g))
    C = M * R
    adeg = np.zeros(n)
    np.add.at(adeg, g[:, 0], np.abs(g[:, 2]))
    np.add.at(adeg, g[:, 1], np.abs(g[:, 2]))
    order = np.argsort(-adeg, kind="stable")
    data = wm.make_data(n, g[:, 0], g[:, 1], g[:, 2], DEV, sorted_degree_nodes=order)
    probs = (rng.rand(n) * 0.6 + 0.2).astype(np.float32)
    start = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    T = max(1, n // 10)
    index = rng.randint(0, n, size=(5 * T, C)).astype(np.int64)
    u = rng.rand(5 * T, C).astype(np.float32)
    uni = rng.rand(num_ls, n, C).astype(np.float32)
    w_vs, w_xs, w_start, w_val, _ = onp.mcpg_sampling_maxcut(g, n, order, start, probs, num_ls, T, M, index, u, uni)
    dev = lambda a: torch.from_numpy(a).to(DEV)     # noqa: E731
    vs, xs_good, st, value = wm.mcpg_sampling_maxcut(data, dev(start), dev(probs), num_ls, T, M, DEV, index=dev(index), u=dev(u),
                                                     uniforms=dev(uni))
    assert np.array_equal(st.cpu().numpy(), w_start) and np.array_equal(vs.cpu().numpy(), w_vs)
    assert np.array_equal(xs_good.cpu().numpy(), w_xs)
    np.testing.assert_allclose(value.cpu().numpy(), w_val, rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------ ISCO
def isco_graph(rng, n, kind):
    """``forms_graph``, or for "padded" what ISCO's own loader gives for a file that repeats lines: edge_from / edge_to sized
    by the header's edge count, filled from a deduplicated graph, the rest (0, 0) -- here three such rows."""
    if kind != "padded":
        return forms_graph(rng, n, 2 * n, kind)
    g = forms_graph(rng, n, 2 * n, "reversed")
    return np.concatenate([g, np.tile(np.array([[0, 0, 1]], np.int64), (3, 1))])


def oracle_step(x, g, pl, T, ug, ua):
    """oracle_isco.maxcut_step in float32 (the reference's arithmetic), plus the spread of its path log-probabilities
    against the same chain in float64: the renormalised terms are ill-conditioned in f32 itself (tests/isco_tol.py), and
    where that spread exceeds ll_atol the f32 reference does not fix the value to within it."""
    r = oi.maxcut_step(x, g[:, 0], g[:, 1], pl, T, ug, ua)
    try:
        oi.F = np.float64
        r64 = oi.maxcut_step(x, g[:, 0], g[:, 1], pl, T, ug, ua)
    finally:
        oi.F = np.float32
    spread = {k: np.abs(r[k].astype(np.float64) - r64[k]) for k in ("ll_x2y", "ll_y2x", "log_acc")}
    return r, spread


def check_step(s, x, pl, T, ug, ua, want, spread, what):
    """_check_maxcut of tests/test_gpu_isco_steps.py with the f32 / f64 spread of each term added to its tolerance."""
    from tests.isco_tol import MIN_MASS, RTOL, ll_atol
    y, energy, acc, terms, mask = s.step(torch.from_numpy(x).to(DEV), torch.from_numpy(pl).to(DEV), T,
                                         draws={"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)},
                                         want_terms=True)
    terms = terms.cpu().numpy().astype(np.float64)
    mass = want["remaining_mass"]
    assert np.array_equal(mask.cpu().numpy().astype(np.uint8), want["mask"].astype(np.uint8)), what
    np.testing.assert_allclose(terms[:, 0], want["ll_x"], rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(terms[:, 2], want["ll_y"], rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(energy.cpu().numpy(), want["energy"], rtol=RTOL, atol=1e-5)
    # a tie among the selected nodes' perturbed values leaves their reverse order -- and so ll_y2x -- unspecified in the
    # reference itself (torch.sort is not stable); such envs are compared on their discrete outputs only, like MIN_MASS ones
    _, lp = oi.maxcut_local_dist(x, s.edge_from.cpu().numpy(), s.edge_to.cpu().numpy(), T)
    pert = (lp - np.log(-np.log(ug))).astype(np.float32)
    tie = np.array([np.unique(pert[b, m]).size < int(m.sum()) for b, m in enumerate(want["mask"].astype(bool))])
    ok = (mass >= MIN_MASS) & ~tie
    tol = {}
    for c, k in ((1, "ll_x2y"), (3, "ll_y2x"), (4, "log_acc")):
        tol[k] = ll_atol(mass, pl) + RTOL * np.abs(want[k]) + spread[k]
        err = np.abs(terms[:, c] - want[k])
        bad = ok & ~(err <= tol[k])
        assert not bad.any(), f"{what}/{k}: envs {np.flatnonzero(bad).tolist()} err {err[bad]} tol {tol[k][bad]} mass {mass[bad]}"
    assert bool((np.abs(acc.cpu().numpy() - want["acc"])[ok] <= 2 * tol["log_acc"][ok]).all()), what
    sure = (want["accept_margin"] > 2 * tol["log_acc"]) & ~tie
    yk = y.cpu().numpy()
    assert np.array_equal(yk[sure], want["y"][sure].astype(np.float32)), what
    assert set(np.unique(yk)) <= {0.0, 1.0}
    return int(ok.sum()), int(sure.sum())


@pytest.mark.parametrize("kind", KINDS + ("padded",))
@pytest.mark.parametrize("n,B,ns", [(64, 12, "auto"), (300, 3, "auto"), (2000, 65, "auto"), (2000, 65, "bits"),
                                    (300, 130, "bits")])
def test_isco_local_dist_and_step_vs_oracle(kind, n, B, ns):
    """get_local_dist (K1 + K3 on the loop-keeping CSR; "bits": K3's bit-sliced form forced and checked to run) and two steps
    (their isco_local_dist) against oracle_isco: each loop adds +1/T to its node's score.  Path lengths up to N / 2, as
    tests/test_gpu_isco_steps.py draws them."""
    from rlsolver_amd import ops
    rng = np.random.RandomState(n + B + len(kind))
    g = isco_graph(rng, n, kind)
    s = _maxcut_sampler(g, n, B)
    x = rng.randint(0, 2, size=(B, n)).astype(np.float32)
    knobs = {"RLS_NODE_STATS_MIN_B": 0} if ns == "bits" else {}
    for T in (1.0, 0.4):
        with forced(knobs):
            if ns == "bits":
                assert ops.node_stats_form(s.graph, B, True) == "bits"
            energy, logp = s.get_local_dist(torch.from_numpy(x).to(DEV), T)
        we, wl = oi.maxcut_local_dist(x, g[:, 0], g[:, 1], T)
        np.testing.assert_allclose(energy.cpu().numpy(), we, rtol=1e-6)
        np.testing.assert_allclose(logp.cpu().numpy(), wl, rtol=1e-5, atol=1e-5)
        pl = rng.randint(1, max(2, n // 2), size=B).astype(np.int64)
        pl[0], pl[-1] = 1, min(70, n // 2)
        ug = rng.rand(B, n).astype(np.float32).clip(1e-7, 1 - 1e-7)
        ua = rng.rand(B).astype(np.float32)
        r, spread = oracle_step(x, g, pl, T, ug, ua)
        n_ok, _ = check_step(s, x, pl, T, ug, ua, r, spread, f"{kind} n={n} T={T}")
        assert n_ok >= B // 2, (n_ok, T)
        x = r["y"].astype(np.float32)
