"""The launch policy of the MaxCut tile entry points (csrc/rls_maxcut_plan.h), queried on the host (rls_maxcut_launch_plan: the
planner the launchers call, nothing is launched): pinned to the launches recorded from the commit before the planner existed, and
checked for the invariants every plan must keep.  No GPU.

tests/golden/maxcut_launch_plans.json holds, for every call of tools/timing/maxcut_launch_trace.py (shapes on both sides of every
LDS limit and num_cus crossover, every policy knob), the kernel name with its template arguments, the grid and the workgroup size
that `rocprofv3 --kernel-trace` reported on an MI355X (256 CUs), and the dynamic LDS bytes of the launch (the trace reports static
LDS only -- 0 for these kernels --, so a build of that commit whose launch macro logs its arguments recorded them: the file's note)."""
import ctypes as C
import json
import os

import pytest

from rlsolver_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maxcut_launch_plans.json")
KLDS = 160 * 1024
RLS_EINVAL, RLS_EUNSUPPORTED = -1, -2      # include/rlsolver_hip.h
K1, K5, K6, K2, K3, WS = range(6)
WHAT = {"K1": K1, "K5": K5, "K6": K6, "K2": K2, "K3": K3, "WS": WS}
F32, BASE_UNALIGNED, MASK_BITS, OUT_UNALIGNED, NO_MINMAX = 1, 2, 4, 8, 16
TILE64, TILE32, NARROW16, NARROW8, ROWS, SW_BATCHED, SW_FAST, SW_GENERIC, NS_TILE, NS_ELEM, UNSUPPORTED = range(11)
WIDTH = {TILE64: 64, TILE32: 32, NARROW16: 16, NARROW8: 8, SW_BATCHED: 64, SW_FAST: 64, SW_GENERIC: 64, NS_TILE: 64}
WORD = {TILE64: 8, TILE32: 4, NARROW16: 2, NARROW8: 1}
DUMMY = 1 << 20      # a non-NULL, 16-byte-aligned "device pointer": the query tests pointers for NULL and alignment only


class Plan(C.Structure):
    _fields_ = [("form", C.c_int32), ("waves", C.c_int32), ("planes", C.c_int32), ("vec", C.c_int32), ("wide", C.c_int32),
                ("stage", C.c_int32), ("grid", C.c_uint32), ("block", C.c_uint32), ("lds", C.c_int64), ("err", C.c_int32)]


def graph(N, E, nnz=None, G=None, max_degree=8, weighted=False, levels=True):
    G = (N + 63) // 64 + 3 if G is None else G
    return _abi.RlsGraph(num_nodes=N, num_stored_edges=E, nnz=2 * E if nnz is None else nnz, if_bidirectional=0, max_degree=max_degree,
                         eu=DUMMY, ev=DUMMY, erowptr=DUMMY, rowptr=DUMMY, col=DUMMY, wgt=DUMMY if weighted else 0, sweep_rowptr=DUMMY,
                         sweep_stream=DUMMY, ell_sym_ptr=DUMMY, ell_sym=DUMMY, ell_st_ptr=DUMMY, ell_st=DUMMY,
                         sweep_lv_ptr=DUMMY if levels else 0, sweep_lv_data=DUMMY if levels else 0, num_sweep_groups=G if levels else 0)


def plan(g, what, B, flags=0, cus=256):
    p = Plan()
    _abi.call("rls_maxcut_launch_plan", C.byref(g), what, B, flags, cus, C.byref(p))
    return p


@pytest.fixture
def knobs():
    """Sets tuning knobs for one test and clears the table afterwards."""
    _abi.tuning_unset()
    yield lambda kv: [_abi.tuning_set(k, v) for k, v in kv.items()]
    _abi.tuning_unset()


def check_invariants(p, what, N, B, G, ctx):
    """What holds for every plan, whatever the policy picked."""
    if p.form == UNSUPPORTED:
        assert p.err == RLS_EUNSUPPORTED, ctx
        return
    assert 0 <= p.lds <= KLDS, ctx
    if p.form == NS_ELEM:
        assert p.block == 256 and p.lds == 0 and p.grid >= 1, ctx
        return
    assert p.block == p.waves * 64 and 1 <= p.waves <= 16, ctx
    if p.form == ROWS:      # one env per wave, a 16-byte-aligned byte row each
        assert p.grid == -(-B // p.waves) and p.lds == p.waves * ((N + 15) // 16 * 16), ctx
        return
    assert p.grid == -(-B // WIDTH[p.form]), ctx
    if p.form in WORD:      # the words of the width the plan names fit, with what the kernel keeps beside them
        pad = 0 if what in (K1, K6) and p.form in (TILE64, TILE32) or what in (K2, K3, WS) and p.form in (TILE64, TILE32) else 2
        scratch = 0 if what in (K2, K3, WS) else p.waves * 512
        table = (4 * (G + 1) + 15) // 16 * 16 if what == K5 else 0
        assert (N + pad) * WORD[p.form] + scratch + table <= p.lds, ctx
    if p.form in (TILE64, TILE32, NARROW16, NARROW8) and what in (K1, K5, K6):
        assert p.planes in ((12, 16, 20, 24) if p.form in (TILE64, TILE32) else (16, 20, 24)), ctx


def row_fits(N):
    return (N + 15) // 16 * 16 <= KLDS


SWEEP_N = sorted({n + d for n in (1536, 3000, 6144, 7680, 8192, 12032, 15872, 16384, 17776, 19808, 19968, 20224, 20480, 32768, 35280, 39936, 40448,
                                  40960, 77432, 79872, 81920, 150312, 159744, 163840) for d in (-16, -8, -5, -4, -2, 0, 1, 2, 4, 8, 16)})
SWEEP_KNOBS = [{}, {"RLS_NARROW_TILE": 0}, {"RLS_NARROW_TILE": 2}, {"RLS_NARROW_TILE": 3},
               {"RLS_K1_TILE32": 0, "RLS_K5_TILE32": 0, "RLS_K6_TILE32": 0, "RLS_NS_TILE32": 0},
               {"RLS_K1_TILE32": 1, "RLS_K5_TILE32": 1, "RLS_K6_TILE32": 1, "RLS_NS_TILE32": 1},
               {"RLS_SWEEP_WAVES": 16, "RLS_NS_WAVES": 4, "RLS_NS_ROWS": 1}, {"RLS_SWEEP_NO_LEVELS": 1, "RLS_NODE_STATS_LANE_ENV": 1},
               {"RLS_K1_LDS_KB": 128, "RLS_NS_PARK": 0, "RLS_SWEEP_WAVES": 2}]


@pytest.mark.parametrize("kn", SWEEP_KNOBS, ids=lambda k: "-".join(f"{a[4:]}={b}" for a, b in k.items()) or "default")
def test_every_plan_around_every_limit_keeps_the_invariants(knobs, kn):
    knobs(kn)
    for N in SWEEP_N:
        for E in (N // 4, 1 << 20):
            for weighted in (False, True):
                g = graph(N, E, weighted=weighted, max_degree=300 if E > N else 8)
                for B in (1, 200, 4112, 1 << 16):
                    for what in range(6):
                        for flags in (0, BASE_UNALIGNED) + ((F32,) if what == K1 else (MASK_BITS,) if what == K6 else (OUT_UNALIGNED,)):
                            p = plan(g, what, B, flags)
                            ctx = (kn, N, E, weighted, B, what, flags, [getattr(p, f) for f, _ in Plan._fields_])
                            check_invariants(p, what, N, B, g.num_sweep_groups, ctx)
                            if p.form == UNSUPPORTED:      # only where not even a row kernel fits (or K6's packed mask meets one)
                                assert what in (K1, K5, K6) and (not row_fits(N) or (what == K6 and flags & MASK_BITS)), ctx
                            if p.form == ROWS:
                                assert N * 8 > KLDS - 2048, ctx      # (past the 64-env tile)


def test_node_stats_form_is_a_view_of_the_plan(knobs):
    for N, E, B, weighted in ((2000, 19990, 64, False), (2000, 19990, 4096, False), (2000, 19990, 64, True), (2000, 19990, 1 << 14, True),
                              (200000, 1000, 1 << 12, False)):
        g = graph(N, E, weighted=weighted)
        for what, sym in ((K2, 0), (K3, 1)):
            form = plan(g, what, B).form
            assert _abi.lib().rls_maxcut_node_stats_form(C.byref(g), B, sym) == (0 if form == NS_ELEM else 2 if form == NS_TILE else 1)


def test_query_rejects_bad_arguments():
    g, p = graph(100, 300), Plan()
    lib = _abi.lib()
    assert lib.rls_maxcut_launch_plan(C.byref(g), 6, 64, 0, 256, C.byref(p)) == RLS_EINVAL
    assert lib.rls_maxcut_launch_plan(C.byref(g), K1, 0, 0, 256, C.byref(p)) == RLS_EINVAL
    assert lib.rls_maxcut_launch_plan(None, K1, 64, 0, 256, C.byref(p)) == RLS_EINVAL
    assert lib.rls_maxcut_launch_plan(C.byref(g), K1, 64, 0, 256, None) == RLS_EINVAL


# ---- the recorded launches ------------------------------------------------------------------------------------------------
CT = {1: "unsigned char", 4: "float"}
BOOL = ("false", "true")
NARROW_WORD = {NARROW16: "unsigned short", NARROW8: "unsigned char", TILE32: "unsigned int"}
WS_TYPE = {1: "signed char", 2: "short", 4: "int"}


def kernel_of(p, row):
    """The kernel (name and template arguments as the trace prints them) a plan stands for."""
    e, v, w, P = row["entry"], BOOL[p.vec], p.waves, p.planes
    bits, wgt = BOOL[row["bits"]], BOOL[row["weighted"]]
    T = CT[4 if row["f32"] else 1]
    if e == "K1":
        return {TILE64: f"k_maxcut_obj<{T}, {v}, {P}, {w}>", TILE32: f"k_maxcut_obj32<{T}, {v}, {P}, {w}>", ROWS: f"k_maxcut_obj_rows<{T}>",
                NARROW16: f"k_maxcut_obj_n<{T}, {v}, {P}, unsigned short>", NARROW8: f"k_maxcut_obj_n<{T}, {v}, {P}, unsigned char>"}[p.form]
    if e == "K6":
        return {TILE64: f"k_maxcut_propose_accept<{v}, {P}, {w}, {bits}>", TILE32: f"k_maxcut_propose_accept32<{v}, {P}, {w}, {bits}>",
                ROWS: "k_maxcut_propose_accept_rows", NARROW16: f"k_maxcut_propose_accept_n<{v}, {P}, unsigned short, {bits}>",
                NARROW8: f"k_maxcut_propose_accept_n<{v}, {P}, unsigned char, {bits}>"}[p.form]
    if e == "K5":
        return {TILE64: f"k_maxcut_greedy_sweep_levels<{v}, {w}, {P}>", TILE32: f"k_maxcut_greedy_sweep_levels32<{v}, {w}, {P}>",
                NARROW16: f"k_maxcut_greedy_sweep_levels_n<{v}, {P}, unsigned short>", NARROW8: f"k_maxcut_greedy_sweep_levels_n<{v}, {P}, unsigned char>",
                SW_BATCHED: f"k_maxcut_greedy_sweep_batched<{v}, {w}>", SW_FAST: f"k_maxcut_greedy_sweep<{v}>",
                SW_GENERIC: f"k_maxcut_greedy_sweep_generic<{v}, {wgt}>", ROWS: f"k_maxcut_greedy_sweep_rows<{wgt}>"}[p.form]
    mode = {"K2": 0, "K3": 1, "WS": 2}[e]
    wt = WS_TYPE[row["ws_bytes"]] if e == "WS" else "int"
    if p.form == NS_ELEM:
        return {"K2": "k_node_cutdeg", "K3": f"k_delta_all<{wgt}>", "WS": f"k_ls_weights_elem<{wt}>"}[e]
    if p.form == NS_TILE:
        return f"k_node_stats_tile<long, false, false, {v}>" if e == "K2" else f"k_node_stats_tile<int, true, {wgt}, {v}>"
    if p.form == TILE64:
        return f"k_node_stats_bits<{mode}, {v}, {BOOL[p.wide]}, {wt}, {w}>"
    return f"k_node_stats_bits32<{mode}, {v}, {BOOL[p.wide]}, {wt}, {NARROW_WORD[p.form]}>"


def test_plans_are_the_recorded_launches(knobs):
    gold = json.load(open(GOLDEN))
    granule = gold["lds_granule"]
    rows = [dict(zip(gold["fields"], r)) for r in gold["rows"]]
    for row in rows:      # (the file names settings and kernels by index)
        row["setting"] = list(gold["settings"])[row["setting"]]
        row["kernel"] = None if row["kernel"] is None else gold["kernels"][row["kernel"]]
    assert len(rows) >= 300
    bad = []
    for row in rows:
        _abi.tuning_unset()
        knobs(gold["settings"][row["setting"]])
        g = graph(row["N"], row["E"], nnz=row["nnz"], G=row["G"], max_degree=row["max_degree"], weighted=row["weighted"], levels=row["G"] > 0)
        p = plan(g, WHAT[row["entry"]], row["B"], (F32 if row["f32"] else 0) | (MASK_BITS if row["bits"] else 0))
        check_invariants(p, WHAT[row["entry"]], row["N"], row["B"], row["G"], row)
        if row["kernel"] is None:
            got = (None, p.form)
            want = (None, UNSUPPORTED)
        else:
            got = (kernel_of(p, row), p.grid, p.block, -(-p.lds // granule) * granule)
            want = (row["kernel"], row["grid"], row["block"], row["lds"])
        if got != want:
            bad.append((row["setting"], row["entry"], row["N"], row["B"], want, got))
    assert not bad, (len(bad), bad[:10])
