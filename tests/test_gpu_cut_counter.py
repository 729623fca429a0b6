"""The bit-sliced cut counter (csrc/rls_cutcount.h: tile_cut_count<P> on 64-bit words and on the half / narrow tiles' words) under every kernel that
reports an objective with it, at each plane count P, on both sides of each plane limit, at the edges of its 1024-edge blocks, and on
the one state that fills its top plane.

Graphs: tests/cut_graphs.py -- bipartite circulants, whose parity state cuts EVERY stored edge.  With E' = limit - 1 stored edges and one
wave per tile that state puts 2^(P - 6) in 63 of the 64 per-lane counts: the only input that reaches the counter's last plane
(k_mcpg_local_search counts with one wave).  States: row 0 cuts nothing, rows 1 and 2 everything, the rest are random.

Every comparison is of integers, against the plain numpy count over the stored edges (cut_graphs.stored_cut: oracle_np.maxcut_obj's sum,
checked against it in tests/test_cut_graphs.py), computed once per graph and state.  Every test enters the (consumer, form, planes) it ran
into a registry; the last test asserts that each triple the dispatch code can reach on this family was run.

Not reachable on this family, and so not in the registry: k_ls_apply_rounds<24, 4> (rows of 15 500 < N <= 20 224 nodes that are no multiple
of 8) and the weighted MCPG stream kernel (its own weighted sum, no planes to pick)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from tests import cut_graphs as cg
from tests.gpu_util import DEV, to_dev_bool
from tests.test_gpu_graph_forms import FORMS, LS_FORMS, forced, run_ls
from tests.test_maxcut_launch_plan import F32, K1, K5, K6, NARROW8, NARROW16, TILE32, TILE64, Plan

pytestmark = pytest.mark.gpu

B = cg.B
K_FORMS = ("auto", "tile64", "tile32", "narrow16", "narrow8")
FORM_ID = {"tile64": TILE64, "tile32": TILE32, "narrow16": NARROW16, "narrow8": NARROW8}
FORM_NAME = {v: k for k, v in FORM_ID.items()}
ALL = cg.cases()
RAN = set()          # (consumer, form, planes) of every launch the tests below checked
_CASES = {}


class Case:
    """One graph of the family on the device, its states and their oracle counts -- built once per module."""

    def __init__(self, c):
        from rlsolver_amd.envs.env_L2A import EnvMaxcut
        self.size, self.stored, self.bidir = c
        self.N, self.u, self.v, w = cg.case_edges(c)
        self.env = EnvMaxcut(mygraph=(self.u, self.v, w), device=DEV, if_bidirectional=self.bidir, num_nodes=self.N, seed=self.stored)
        self.env.num_edges = len(self.u)
        self.dg = self.env.graph
        assert self.dg.num_stored_edges == self.stored
        self.planes = cg.planes(self.stored)
        self.full = self.stored // 2 if self.bidir else self.stored       # the objective of a state that cuts every edge
        self.xb = cg.states(self.N, self.stored + self.bidir)
        self._memo = {}
        self.obj0 = self.obj(self.xb)
        assert self.obj0[0] == 0 and self.obj0[1] == self.full and self.obj0[2] == self.full
        self.sym_deg = np.bincount(np.concatenate([self.u, self.v]), minlength=self.N)

    def obj(self, xb):
        """The oracle objective of bool rows [B, N] (memoised: the forms of one consumer return the same rows)."""
        xb = np.ascontiguousarray(np.asarray(xb).astype(bool))
        key = hash(xb.tobytes())
        if key not in self._memo:
            self._memo[key] = cg.obj_of(xb, self.u, self.v, self.bidir)
        return self._memo[key]


def case(c):
    if c not in _CASES:
        _CASES[c] = Case(c)
    return _CASES[c]


def num_cus():
    return int(torch.cuda.get_device_properties(DEV).multi_processor_count)


def plan_of(k, what, flags=0):
    from rlsolver_amd import _abi
    p = Plan()
    _abi.call("rls_maxcut_launch_plan", k.dg.ref, what, B, flags, num_cus(), C.byref(p))
    return p


def ran_plan(consumer, k, what, form, flags=0):
    """The plan the launcher takes under the knobs now set: the forced form, with the planes of E'.  Enters it into the registry."""
    p = plan_of(k, what, flags)
    assert p.form in FORM_NAME, (consumer, form, p.form)
    if form != "auto":
        assert p.form == FORM_ID[form], (consumer, form, p.form)
    narrow = p.form in (NARROW16, NARROW8)
    assert p.planes == (16 if narrow and k.planes == 12 else k.planes), (consumer, form, k.stored, p.planes)
    RAN.add((consumer, FORM_NAME[p.form], p.planes))
    return p


# ------------------------------------------------------------------------------------------ K1 / K6 / K5
@pytest.mark.parametrize("c", ALL, ids=cg.case_id)
def test_k1_objective(c):
    from rlsolver_amd import ops
    k = case(c)
    rows = {0: to_dev_bool(k.xb), F32: torch.from_numpy(k.xb.astype(np.float32)).to(DEV)}
    for form in K_FORMS:
        with forced(FORMS[form]):
            for flags, xs in rows.items():
                p = ran_plan("K1", k, K1, form, flags)
                got = ops.maxcut_obj(k.dg, xs).cpu().numpy()
                bad = np.flatnonzero(got != k.obj0)
                assert not bad.size, (form, flags, p.planes, p.waves, bad[:8].tolist(), got[bad[:8]].tolist(), k.obj0[bad[:8]].tolist())


@pytest.mark.parametrize("c", ALL, ids=cg.case_id)
def test_k6_propose_accept(c):
    """A sparse random mask; on row 0 (all zeros) the parity mask: that proposal cuts every edge and must be accepted at the full value."""
    from rlsolver_amd import ops
    k = case(c)
    rng = np.random.RandomState(k.stored + 3)
    mask = rng.rand(B, k.N) < 0.02
    mask[0] = k.xb[1]
    prop = k.xb ^ mask
    pv = k.obj(prop)
    take = pv >= k.obj0
    assert take[0] and pv[0] == k.full
    want_v, want_x = np.where(take, pv, k.obj0), np.where(take[:, None], prop, k.xb)
    md = to_dev_bool(mask)
    for form in K_FORMS:
        with forced(FORMS[form]):
            p = ran_plan("K6", k, K6, form)
            x6, v6 = to_dev_bool(k.xb), torch.from_numpy(k.obj0.copy()).to(DEV)
            ops.maxcut_propose_accept(k.dg, x6, md, v6)
        got = v6.cpu().numpy()
        bad = np.flatnonzero(got != want_v)
        assert not bad.size, (form, p.planes, p.waves, bad[:8].tolist(), got[bad[:8]].tolist(), want_v[bad[:8]].tolist())
        assert np.array_equal(x6.cpu().numpy(), want_x), form


@pytest.mark.parametrize("c", ALL, ids=cg.case_id)
def test_k5_greedy_sweep(c):
    """The returned value is the cut of the returned row and no less than the input's.  A row that cuts every edge keeps every node that
    has an edge (its flip loses them all); a node without one flips once, on the tie the sweep accepts (env_L2A.py:109-116)."""
    from rlsolver_amd import ops
    k = case(c)
    for form in K_FORMS:
        with forced(FORMS[form]):
            p = ran_plan("K5", k, K5, form)
            x5, v5 = to_dev_bool(k.xb), torch.from_numpy(k.obj0.copy()).to(DEV)
            ops.maxcut_greedy_sweep(k.dg, x5, v5)
        gx, gv = x5.cpu().numpy(), v5.cpu().numpy()
        want = k.obj(gx)
        bad = np.flatnonzero(gv != want)
        assert not bad.size, (form, p.planes, p.waves, bad[:8].tolist(), gv[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert np.all(gv >= k.obj0), form
        for r in (1, 2):
            assert gv[r] == k.full and np.array_equal(gx[r], k.xb[r] ^ (k.sym_deg == 0)), (form, r)
        if k.size == "S12":      # the literal oracle (O(N E) per row) on the rows that cut nothing and everything
            g = np.stack([k.u, k.v, np.ones_like(k.u)], axis=1)
            wx, wv = onp.greedy_sweep(k.xb[:2].copy(), k.obj0[:2].copy(), g, k.bidir)
            assert np.array_equal(gx[:2], wx) and np.array_equal(gv[:2], wv), form


# ------------------------------------------------------------------------------------------ the local search
M20 = 1 << 20
LS_CASES = [("S12", 1024, False), ("S12", 4095, False), ("S12", 4096, False), ("S12", 4098, True),
            ("S16", 8 * 1024, False), ("S16", 65535, False), ("S16", 65536, False), ("S16", 65537, False), ("S16", 65534, True), ("S16", 65538, True),
            ("S24", M20 - 1, False), ("S24", M20 + 2, True)]


def check_ls_result(k, gx, gv, what):
    want = k.obj(gx)
    bad = np.flatnonzero(gv != want)
    assert not bad.size, (what, bad[:8].tolist(), gv[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert np.all(gv >= k.obj0), what
    assert gv[1] == k.full and gv[2] == k.full, what          # nothing beats a row that cuts every edge, and no step may lose value


@pytest.mark.parametrize("num_iters", [0, 2])
@pytest.mark.parametrize("ls_form", LS_FORMS)
@pytest.mark.parametrize("c", LS_CASES, ids=cg.case_id)
def test_local_search_forms(monkeypatch, c, ls_form, num_iters):
    """EnvMaxcut.local_search_inplace in each of its three forms (run_ls asserts which one ran).  S24 is past the fused kernel's LDS
    layout: that refusal is asserted, and the forms that do cover it run."""
    from rlsolver_amd import ops
    k = case(c)
    fusable, rounds = ops.local_search_fusable(k.dg, 6, B), ops.ls_rounds_supported(k.dg, 6)
    assert fusable == (k.size != "S24") and rounds, (fusable, rounds)
    if ls_form == "fused" and not fusable:
        with pytest.raises(RuntimeError, match="LDS"):
            xs = to_dev_bool(k.xb)
            ws, mm = ops.maxcut_ls_weights(k.dg, xs, 1, padded=True, return_minmax=True)
            ops.maxcut_local_search(k.dg, xs, ws, (mm[1] - mm[0]).float(), torch.zeros(B, dtype=torch.int64, device=DEV), num_iters, 6, compute_obj=True)
        return
    env = k.env
    env.fused_local_search, env.force_ls_rounds, env.force_ls_fused = ls_form != "decomposed", ls_form == "rounds", ls_form == "fused"
    try:
        gx, gv, _ = run_ls(monkeypatch, env, k.xb, 1, num_iters, 6, ls_form, np.random.RandomState(k.stored + num_iters))
    finally:
        env.fused_local_search, env.force_ls_rounds, env.force_ls_fused = True, False, False
    check_ls_result(k, gx, gv, (ls_form, num_iters))


def ls_inputs(k, dtype=None):
    from rlsolver_amd import ops
    xs = to_dev_bool(k.xb)
    ws, mm = ops.maxcut_ls_weights(k.dg, xs, 1, dtype=dtype, padded=True, return_minmax=True)
    return xs, ws, (mm[1] - mm[0]).to(torch.float32).mul_(0.3)


FUSED_CASES = [("S12", 4095, False), ("S12", 4097, False), ("S12", 2600, True), ("S16", 65535, False), ("S16", 65536, False), ("S16", 65538, True),
               ("S16w", 4096 * 17, False)]


@pytest.mark.parametrize("c", FUSED_CASES, ids=cg.case_id)
def test_fused_local_search_widths_and_waves(c):
    """k_maxcut_local_search<.., WT, P, W>: P = 16 below 2^16 stored edges and 24 from there on, int8 and int16 weights, 4 and 8 waves
    (dev knob RLS_LS_WAVES).  It counts the start value itself (compute_obj), every proposal and the swept rows."""
    from rlsolver_amd import ops
    k = case(c)
    assert ops.local_search_fusable(k.dg, 6, B)
    natural = ops.ls_weight_dtype(k.dg, 1)
    assert natural == (torch.int8 if k.size in ("S12", "S16w") else torch.int16)
    first = None
    for dt in dict.fromkeys((natural, torch.int16)):
        for W in (4, 8):
            xs, ws, rd_std = ls_inputs(k, dt)
            vs = torch.zeros(B, dtype=torch.int64, device=DEV)
            with forced({"RLS_LS_WAVES": W}):
                ops.maxcut_local_search(k.dg, xs, ws, rd_std, vs, 2, 6, seed=k.stored, compute_obj=True)
            gx, gv = xs.cpu().numpy(), vs.cpu().numpy()
            check_ls_result(k, gx, gv, (dt, W))
            RAN.add(("ls_fused", f"{str(dt)[6:]}-w{W}", 16 if k.planes <= 16 else 24))
            if first is None:
                first = (gx, gv)
            assert np.array_equal(gx, first[0]) and np.array_equal(gv, first[1]), (dt, W)      # the same draws: the same search


ROUND_CASES = [("S12", 4095, False), ("S16", 15 * 1024 + 1000, False), ("S16", 65536, False), ("S24", M20 - 1, False), ("S24", M20, False),
               ("S24", M20 + 2, True)]


@pytest.mark.parametrize("c", ROUND_CASES, ids=cg.case_id)
def test_round_kernels(c):
    """The three kernels that apply proposal rounds, all with 24 planes: k_ls_propose (one launch per round, no scratch),
    k_ls_apply_rounds<24, 8> and k_ls_apply_rounds32<24, 8> (all rounds' mask words in the scratch; dev knob RLS_LS_APPLY32 picks)."""
    from rlsolver_amd import ops
    k = case(c)
    assert ops.ls_rounds_supported(k.dg, 6)
    seed, rounds = k.stored + 11, 2
    first = None
    for kern, knob32 in (("ls_propose", None), ("ls_apply_rounds", 0), ("ls_apply_rounds32", 1)):
        xs, ws, rd_std = ls_inputs(k)
        vs = torch.from_numpy(k.obj0.copy()).to(DEV)
        thresh = ops.maxcut_ls_threshold(k.dg, ws, rd_std, seed, 6, draw=0)
        if knob32 is None:
            for r in range(rounds):
                ops.maxcut_ls_propose(k.dg, xs, ws, rd_std, thresh, vs, seed, 1 + r)
        else:
            need = max(ops.ls_scratch_bytes(k.dg, B, ws.dtype, rounds), -(-B // 64) * k.N * 8 * rounds)
            scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
            with forced({"RLS_LS_APPLY32": knob32}):
                ops.maxcut_ls_rounds(k.dg, xs, ws, rd_std, thresh, vs, seed, 1, rounds, scratch=scratch)
        gx, gv = xs.cpu().numpy(), vs.cpu().numpy()
        check_ls_result(k, gx, gv, kern)
        RAN.add((kern, "w8", 24))
        if first is None:
            first = (gx, gv)
        assert np.array_equal(gx, first[0]) and np.array_equal(gv, first[1]), kern


# ------------------------------------------------------------------------------------------ MCPG
MCPG_CASES = [("S12", e, False) for e in (1024, 4095, 4096, 4097)] + [("S16", e, False) for e in (16 * 1024, 65535, 65536, 65537)] + \
             [("S24", e, False) for e in (M20 - 1, M20, M20 + 1)]
_MCPG = {}


def mcpg_tables(k):
    """(order, visit stream, level pointers, level data) of the MCPG samplers for a case's graph (methods/MCPG.py: make_data; the
    graph has no loops, so the DeviceGraph of the case is the one make_data would build)."""
    from rlsolver_amd import _abi
    from rlsolver_amd.methods import MCPG as amcpg
    key = (k.size, k.stored)
    if key not in _MCPG:
        order = np.argsort(-k.sym_deg, kind="stable")
        csr = k.dg.csr
        lv = amcpg.build_visit_levels(csr, order)
        assert lv is not None and _abi.lib().rls_mcpg_local_search_levels_supported(k.dg.ref, lv[0].size - 1)
        # the stream kernel runs only where the launcher's test passes (rls_mcpg_local_search: `fast`); else the call falls to the one-wave one
        assert csr.max_degree + 4 <= 512 and (k.N + 2) * 8 + 4096 * 4 + 16 * 64 * 8 <= 160 * 1024
        _MCPG[key] = (torch.from_numpy(order.astype(np.int32)).to(DEV), torch.from_numpy(amcpg.build_visit_stream(csr, order)).to(DEV),
                      torch.from_numpy(lv[0]).to(DEV), torch.from_numpy(lv[1]).to(DEV))
    return _MCPG[key]


def mcpg_draws(k, num_ls):
    """Tie coins as the sequential kernels' uniforms (0.25 | 0.75) and as the level kernel's packed words."""
    if num_ls == 0:
        return None, None
    coin = np.random.RandomState(k.stored + 5).randint(0, 2, size=(num_ls, k.N, B)).astype(bool)
    CB = (B + 63) // 64
    bits = np.zeros((num_ls * k.N, CB * 64), dtype=np.uint64)
    bits[:, :B] = coin.reshape(num_ls * k.N, B)
    words = (bits.reshape(num_ls * k.N, CB, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    return torch.from_numpy(np.where(coin, 0.25, 0.75).astype(np.float32)).to(DEV), torch.from_numpy(words.view(np.int64)).to(DEV)


def check_mcpg(k, num_ls, xs_out, expected, what):
    """expected = E' - 2 cut, the cut counted by the oracle from the kernel's own output; with no pass the output is the input."""
    got_x = xs_out.cpu().numpy()
    assert set(np.unique(got_x)) <= {0.0, 1.0}, what
    rows = got_x.T > 0
    if num_ls == 0:
        assert np.array_equal(rows, k.xb), what
    want = (k.stored - 2 * k.obj(rows)).astype(np.float32)
    got = expected.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not bad.size, (what, num_ls, k.planes, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("num_ls", [0, 1])
@pytest.mark.parametrize("c", MCPG_CASES, ids=cg.case_id)
def test_mcpg_local_search_one_wave(c, num_ls):
    """k_mcpg_local_search: ONE wave counts every edge -- at E' = limit - 1 the parity chain puts 2^(P - 6) in a lane, the top plane."""
    from rlsolver_amd import ops_mcpg_tsp as mops
    k = case(c)
    order, _, _, _ = mcpg_tables(k)
    uni, _ = mcpg_draws(k, num_ls)
    x0 = torch.from_numpy(np.ascontiguousarray(k.xb.T).astype(np.float32)).to(DEV)
    xs, exp = mops.mcpg_local_search(k.dg, x0, order, num_ls, uni, 0, visit_stream=None)
    check_mcpg(k, num_ls, xs, exp, "one wave")
    RAN.add(("mcpg_plain", "w1", k.planes))


@pytest.mark.parametrize("num_ls", [0, 1])
@pytest.mark.parametrize("c", MCPG_CASES, ids=cg.case_id)
def test_mcpg_local_search_stream(c, num_ls):
    from rlsolver_amd import ops_mcpg_tsp as mops
    k = case(c)
    order, stream, _, _ = mcpg_tables(k)
    uni, _ = mcpg_draws(k, num_ls)
    for x0 in (torch.from_numpy(np.ascontiguousarray(k.xb.T).astype(np.float32)).to(DEV), to_dev_bool(np.ascontiguousarray(k.xb.T))):
        xs, exp = mops.mcpg_local_search(k.dg, x0, order, num_ls, uni, 0, visit_stream=stream)
        check_mcpg(k, num_ls, xs, exp, ("stream", x0.dtype))
    RAN.add(("mcpg_stream", "w16", k.planes))


LEVEL_IO = [(i, o, w) for i in ("bool", "f32", "packed") for o in ("f32", "packed") for w in (0,)] + [("packed", "packed", 4), ("packed", "packed", 16)]


@pytest.mark.parametrize("num_ls", [0, 1])
@pytest.mark.parametrize("c", MCPG_CASES, ids=cg.case_id)
def test_mcpg_local_search_levels(c, num_ls):
    """k_mcpg_local_search_levels<TI, TO, P, W>: bool, float32 and bit-packed chains in, float32 and packed out; packed to packed also with
    4 and 16 waves (dev knob RLS_K7_WAVES; 8 otherwise, 16 for the other layouts)."""
    from rlsolver_amd import ops_mcpg_tsp as mops
    k = case(c)
    _, _, lvp, lvd = mcpg_tables(k)
    _, coins = mcpg_draws(k, num_ls)
    xt = np.ascontiguousarray(k.xb.T)
    f32 = torch.from_numpy(xt.astype(np.float32)).to(DEV)
    first = None
    for i, o, w in LEVEL_IO:
        xin = {"bool": to_dev_bool(xt), "f32": f32, "packed": mops.PackedChains.pack(f32)}[i]
        out = mops.PackedChains.empty(k.N, B, DEV) if o == "packed" else None
        with forced({"RLS_K7_WAVES": w} if w else {}):
            xs, exp = mops.mcpg_local_search_levels(k.dg, xin, lvp, lvd, num_ls, 0, coins=coins, out=out)
        xs = xs.unpack() if o == "packed" else xs
        check_mcpg(k, num_ls, xs, exp, (i, o, w))
        RAN.add(("mcpg_levels", f"{i}->{o}" + (f"-w{w}" if w else ""), k.planes))
        if first is None:
            first = xs.cpu().numpy()
        assert np.array_equal(xs.cpu().numpy(), first), (i, o, w)


# ------------------------------------------------------------------------------------------ the registry
def reachable():
    """Every (consumer, form, planes) the dispatch code reaches on this family: plan_planes / narrow_planes of rls_maxcut_plan.h for K1 /
    K6 / K5, DISPATCH_P of rls_maxcut_local_search ({16, 24}), the round kernels' single width, pick_planes in rls_mcpg.hip."""
    want = set()
    for cons in ("K1", "K6", "K5"):
        want |= {(cons, f, P) for f in ("tile64", "tile32") for P in (12, 16, 20, 24)}
        want |= {(cons, f, P) for f in ("narrow16", "narrow8") for P in (16, 20, 24)}
    want |= {("ls_fused", f"{dt}-w{W}", P) for dt in ("int8", "int16") for W in (4, 8) for P in (16, 24)}
    want |= {(kern, "w8", 24) for kern in ("ls_propose", "ls_apply_rounds", "ls_apply_rounds32")}
    for P in (12, 16, 20, 24):
        want |= {("mcpg_plain", "w1", P), ("mcpg_stream", "w16", P)}
        want |= {("mcpg_levels", f"{i}->{o}" + (f"-w{w}" if w else ""), P) for i, o, w in LEVEL_IO}
    return want


def test_zz_every_reachable_counter_instantiation_was_run(request):
    """Runs last in this file.  Meaningful when the whole file ran; a subset (-k, a node id, --deselect) skips."""
    cfg = request.config
    if cfg.getoption("-k") or cfg.getoption("deselect") or any("::" in str(a) for a in cfg.args):
        pytest.skip("the registry is checked when the whole file ran")
    want = reachable()
    assert len(want) == 3 * 14 + 8 + 3 + 4 * (2 + len(LEVEL_IO))
    missing = sorted(want - RAN)
    assert not missing, f"{len(missing)} of {len(want)} reachable (consumer, form, planes) never ran: {missing}"
    print(f"cut counter: {len(want)} reachable (consumer, form, planes) triples, all run; also run: {sorted(RAN - want)}")
