"""The launch policy of the local-search entry points (csrc/rls_ls_plan.h), queried on the host (rls_maxcut_ls_launch_plan: the planner
the launchers call, nothing is launched): pinned to the launches recorded from the commit before the planner existed, and checked
for the invariants every plan must keep.  No GPU.

tests/golden/ls_launch_plans.json.gz is the output of tools/ls_launch_record/record.py on that commit: rls_localsearch.hip compiled with
its launch macro turned into a recorder, its four entry points called on dummy pointers (no device: 256 CUs) for N on both sides of
every limit of the policy, crossed with batch sizes, weight widths, edge counts, scratch sizes, alignments, schedules and policy
knobs.  Per case: every launch in order (kernel with template arguments, grid, block, dynamic LDS, every argument -- pointers by the
dummy they point into), or the refusal's code and text, and what the four host queries answered."""
import ctypes as C
import gzip
import json
import os

import pytest

from rlsolver_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ls_launch_plans.json.gz")
KLDS = 160 * 1024
RLS_EINVAL, RLS_EUNSUPPORTED = -1, -2      # include/rlsolver_hip.h
FUSED, THRESHOLD, PROPOSE, ROUNDS = range(4)
X_UNALIGNED, NOISE_UNALIGNED, SCRATCH_UNALIGNED, NO_SCRATCH = 1, 2, 4, 8
K_FUSED, K_THRESHOLD, K_MERGE, K_MASK, K_PROPOSE, K_APPLY, K_APPLY32, K_K6 = range(8)
DUMMY = 1 << 20      # a non-NULL "device pointer": the query tests pointers for NULL only
CAP = 64


class Launch(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("ws_bytes", C.c_int32), ("planes", C.c_int32), ("waves", C.c_int32), ("sd_lds", C.c_int32),
                ("premask", C.c_int32), ("grid", C.c_uint32 * 3), ("block", C.c_uint32), ("lds", C.c_int64), ("batched", C.c_int32),
                ("x_aligned", C.c_int32), ("stage", C.c_int32), ("rounds", C.c_int32), ("first_round", C.c_int32), ("round_words", C.c_int64)]


class Info(C.Structure):
    _fields_ = [("err", C.c_int32), ("num_launches", C.c_int32), ("msg", C.c_char * 288)]


def graph(N, E=40000, schedule=2, weighted=0, max_degree=8):
    lv = DUMMY if schedule >= 2 else 0
    return _abi.RlsGraph(num_nodes=N, num_stored_edges=E, nnz=2 * E, if_bidirectional=1, max_degree=max_degree, eu=DUMMY, ev=DUMMY, erowptr=DUMMY,
                         rowptr=DUMMY, col=DUMMY, wgt=DUMMY if weighted else 0, sweep_rowptr=DUMMY if schedule >= 1 else 0,
                         sweep_stream=DUMMY if schedule >= 1 else 0, ell_sym_ptr=0, ell_sym=0, ell_st_ptr=0, ell_st=0, sweep_lv_ptr=lv, sweep_lv_data=lv,
                         num_sweep_groups=N // 64 + 3 if schedule >= 2 else 0)


def plan(g, what, B, ws_bytes=1, ws_pitch=None, num_spin=5, num_draws=1, flags=0, scratch_bytes=1 << 40, cus=256):
    """(err, msg, launches) of an entry point.  ws_pitch None: N rounded up to 16 entries; the scratch, unless told, is plentiful."""
    out, info = (Launch * CAP)(), Info()
    pitch = (g.num_nodes + 15) // 16 * 16 if ws_pitch is None else ws_pitch
    _abi.call("rls_maxcut_ls_launch_plan", C.byref(g), what, B, ws_bytes, pitch, num_spin, num_draws, flags, scratch_bytes, cus, out, CAP, C.byref(info))
    assert info.num_launches <= CAP and (info.err == 0 or info.num_launches == 0)
    return info.err, info.msg.decode(), list(out[:info.num_launches])


@pytest.fixture
def knobs():
    """Sets tuning knobs for one test and clears the table afterwards."""
    _abi.tuning_unset()
    yield lambda kv: [_abi.tuning_set(k, v) for k, v in kv.items()]
    _abi.tuning_unset()


# ---- the recorded launches ------------------------------------------------------------------------------------------------
WT = {1: "signed char", 2: "short"}
BOOL = ("false", "true")


def kernel_of(l):
    """The kernel (name and template arguments as the recorder demangles them) a launch of the plan stands for."""
    wt, sd = WT.get(l.ws_bytes), BOOL[l.sd_lds]
    return {K_FUSED: f"rls::k_maxcut_local_search<true, {wt}, {l.planes}, {l.waves}>", K_THRESHOLD: f"rls::k_ls_threshold<{wt}, {sd}>",
            K_MERGE: "rls::k_ls_threshold_merge", K_MASK: f"rls::k_ls_mask<{wt}, {sd}>",
            K_PROPOSE: f"rls::k_ls_propose<{wt}, {l.planes}, {sd}, {BOOL[l.premask]}>", K_APPLY: f"rls::k_ls_apply_rounds<{l.planes}, {l.waves}>",
            K_APPLY32: f"rls::k_ls_apply_rounds32<{l.planes}, {l.waves}>", K_K6: "rls_maxcut_propose_accept"}[l.kernel]


def args_of(l, row, call):
    """The arguments the launcher passes with this launch, as the recorder prints them: integers by value, pointers by dummy."""
    at = lambda name, off: f"{name}+{off}" if off else name      # noqa: E731
    N, B, E, spin = row["N"], row["B"], row["E"], row["num_spin"]
    x, noise, pitch, tiles = at("x", row["x_off"]), at("noise", row["noise_off"]), row["ws_pitch"] or N, -(-B // 64)
    scr = "0" if row["scratch_mode"] == 0 else at("scr", row["scratch_off"])
    seed, off, draw = call["seed"], call["env_offset"], call["first_draw"] + l.first_round
    edges = f"{x},{B},{N},eu,ev,{E},{call['halve']}"
    if l.kernel == K_FUSED:
        sweep = {2: f"sweep_lv_ptr,sweep_lv_data,{N // 64 + 3}", 1: f"sweep_rowptr,sweep_stream,{2 * E + N}", 0: f"rowptr,col,{2 * E}"}[l.batched]
        return f"{edges},{sweep},ws,{pitch},sd,{noise},{seed},{off},{call['num_iters']},{spin},{call['first_draw_proposes']},obj,{call['compute_obj']},{l.batched}"
    if l.kernel == K_THRESHOLD:
        return f"ws,{pitch},{B},{N},sd,{seed},{off},{call['first_draw']},{spin},th,{scr}"
    if l.kernel == K_MERGE:
        return f"{scr},{l.rounds},{B},{spin},th"
    if l.kernel == K_MASK:
        return f"ws,{pitch},{B},{N},sd,th,{seed},{off},{draw},{scr},{l.round_words}"
    if l.kernel == K_PROPOSE:
        return f"{edges},ws,{pitch},sd,th,{seed},{off},{draw},obj,{scr},{l.x_aligned}"
    if l.kernel == K_APPLY32:
        return f"{edges},{scr},{tiles},{l.rounds},obj,{l.x_aligned},{l.stage}"
    if l.kernel == K_APPLY:
        return f"{edges},{scr},{l.rounds},obj,{l.x_aligned},{l.stage}"
    return f"g,{x},{B},{at('scr', row['scratch_off'] + (l.first_round % l.rounds) * tiles * N * 8)},1,obj"      # (round k's words of the launch)


def test_plans_are_the_recorded_launches(knobs):
    gold = json.load(gzip.open(GOLDEN))
    rows = [dict(zip(gold["fields"], r)) for r in gold["rows"]]
    assert len(rows) >= 7000 and {r["entry"] for r in rows} == {FUSED, THRESHOLD, PROPOSE, ROUNDS}
    table = gold["launch_table"]
    bad, current = [], None
    for row in rows:      # every row: there is no skip list
        if row["knobs"] != current:
            _abi.tuning_unset()
            knobs({"RLS_" + k: v for k, v in gold["knobs"][row["knobs"]].items()})
            current = row["knobs"]
        g = graph(row["N"], row["E"], row["schedule"], row["weighted"], row["max_degree"])
        flags = ((X_UNALIGNED if row["x_off"] % 16 else 0) | (NOISE_UNALIGNED if row["noise_off"] % 16 else 0) |
                 (SCRATCH_UNALIGNED if row["scratch_off"] % 16 else 0) | (NO_SCRATCH if row["scratch_mode"] == 0 else 0))
        err, msg, ls = plan(g, row["entry"], row["B"], row["ws_bytes"], row["ws_pitch"], row["num_spin"], row["num_draws"], flags, row["scratch_bytes"])
        got = (err, msg, [[kernel_of(l)] + ([0] * 5 if l.kernel == K_K6 else [*l.grid, l.block, l.lds]) + [args_of(l, row, gold["call"])] for l in ls])
        want = (row["rc"], gold["errors"][row["error"]], [[gold["kernels"][table[i][0]]] + table[i][1:] for i in row["launches"]])
        lib = _abi.lib()
        queries = [lib.rls_maxcut_local_search_supported(C.byref(g), row["B"], row["num_spin"]), lib.rls_maxcut_ls_rounds_supported(C.byref(g), row["num_spin"]),
                   lib.rls_maxcut_ls_scratch_bytes(C.byref(g), row["B"], row["ws_bytes"], row["num_draws"]), lib.rls_maxcut_ls_slices(C.byref(g), row["B"], row["ws_bytes"])]
        if got != want or queries != [row["fused_supported"], row["rounds_supported"], row["ls_scratch_bytes"], row["ls_slices"]]:
            bad.append((row, want, got, queries))
    assert not bad, (len(bad), bad[:5])


# ---- invariants around every limit ----------------------------------------------------------------------------------------
LIMITS = (3172, 6348, 7268, 10580, 15872, 20224, 24576, 31744, 39936, 159740)
SWEEP_N = sorted({800, 2000} | {L + d for L in LIMITS for d in range(-17, 18)})
SWEEP_KNOBS = [{}, {"RLS_LS_WAVES": 4}, {"RLS_LS_WAVES": 8}, {"RLS_LS_SLICES": 3}, {"RLS_LS_PER_ROUND": 1}, {"RLS_LS_APPLY32": 0}, {"RLS_LS_APPLY32": 1},
               {"RLS_LS_SD_GLOBAL": 1}, {"RLS_NARROW_TILE": 0}]
# what of the tile the kernel keeps in LDS at the least: bytes per node (the fused kernel: the tile and the proposal tile)
WORDS = {K_FUSED: 16, K_PROPOSE: 8, K_APPLY: 8, K_APPLY32: 4}


def check_launches(ls, N, B, ctx):
    for l in ls:
        if l.kernel == K_K6:
            continue
        assert 0 <= l.lds <= KLDS and l.block == 64 * l.waves and l.waves in (1, 4, 8), ctx
        assert l.grid[0] == -(-B // (32 if l.kernel == K_APPLY32 else 64)) and 1 <= l.grid[1] <= 8 and l.grid[2] >= 1, ctx
        assert l.lds >= N * WORDS.get(l.kernel, 0) + (4 * N if l.kernel in (K_THRESHOLD, K_PROPOSE) and l.sd_lds else 0), ctx
        assert l.lds == 0 if l.kernel in (K_MASK, K_MERGE) else l.lds > 0, ctx
        assert l.kernel not in (K_PROPOSE, K_APPLY, K_APPLY32) or l.planes == 24, ctx


@pytest.mark.parametrize("kn", SWEEP_KNOBS, ids=lambda k: "-".join(f"{a[4:]}={b}" for a, b in k.items()) or "default")
def test_every_plan_around_every_limit_keeps_the_invariants(knobs, kn):
    knobs(kn)
    lib = _abi.lib()
    for N in SWEEP_N:
        g = graph(N)
        for B in (1, 256, 8256, 16448, 65536):
            for wb in (1, 2):
                ctx = (kn, N, B, wb)
                slices = lib.rls_maxcut_ls_slices(C.byref(g), B, wb)
                need1, need4 = (lib.rls_maxcut_ls_scratch_bytes(C.byref(g), B, wb, d) for d in (1, 4))
                err, _, ls = plan(g, FUSED, B, wb)      # the four host queries are views of the plans
                check_launches(ls, N, B, ctx)
                assert lib.rls_maxcut_local_search_supported(C.byref(g), B, 5) == (err == 0), ctx
                err, _, ls = plan(g, THRESHOLD, B, wb, scratch_bytes=need1)
                check_launches(ls, N, B, ctx)
                assert err != 0 or (ls[0].grid[1] == slices and len(ls) == (2 if slices > 1 else 1)), ctx
                one = plan(g, ROUNDS, B, wb, scratch_bytes=need1)
                check_launches(one[2], N, B, ctx)
                assert lib.rls_maxcut_ls_rounds_supported(C.byref(g), 5) == (one[0] == 0), ctx
                pr = plan(g, PROPOSE, B, wb, scratch_bytes=need1)      # rls_maxcut_ls_propose is rls_maxcut_ls_rounds with one draw
                assert (pr[0], pr[1], [bytes(l) for l in pr[2]]) == (one[0], one[1], [bytes(l) for l in one[2]]), ctx
                err, _, ls = plan(g, ROUNDS, B, wb, num_draws=4, scratch_bytes=need4)
                check_launches(ls, N, B, ctx)
                assert (err == 0) == (one[0] == 0), ctx
                masked = one[0] == 0 and one[2][-1].kernel in (K_APPLY, K_APPLY32, K_K6)      # the rounds run through the mask words
                if masked:      # ... and then not without one round's worth of scratch; the mask grid keeps the slices
                    assert plan(g, ROUNDS, B, wb, scratch_bytes=need1 - 1)[0] == RLS_EUNSUPPORTED and one[2][0].grid[1] == slices, ctx
                if err == 0 and not kn.get("RLS_LS_PER_ROUND") and -(-B // 64) * N * 32 <= 1 << 30:      # all four rounds' words at once
                    assert ls[0].kernel == K_MASK and ls[0].grid[2] == 4 and ls[0].rounds == 4 and ls[1].rounds == 4 and need4 >= -(-B // 64) * N * 32, ctx
                    assert len(ls) == (5 if ls[1].kernel == K_K6 else 2), ctx
                    if need4 == -(-B // 64) * N * 32:      # one byte less: a round per launch
                        assert all(l.rounds <= 1 for l in plan(g, ROUNDS, B, wb, num_draws=4, scratch_bytes=need4 - 1)[2]), ctx


def test_query_rejects_bad_arguments():
    g, out, info = graph(100, 300), (Launch * 4)(), Info()
    f = _abi.lib().rls_maxcut_ls_launch_plan
    good = [C.byref(g), ROUNDS, 64, 1, 112, 5, 4, 0, 1 << 20, 256, out, 4, C.byref(info)]
    assert f(*good) == 0 and info.err == 0 and info.num_launches == 2
    for i, v in ((0, None), (1, 4), (1, -1), (2, 0), (3, 3), (4, -16), (6, 0), (10, None), (11, -1), (12, None)):
        assert f(*(good[:i] + [v] + good[i + 1:])) == RLS_EINVAL, (i, v)
    assert f(*(good[:10] + [None, 0, C.byref(info)])) == 0 and info.num_launches == 2      # counting only
