"""The launch policy of the ISCO sampler steps (csrc/rls_isco_plan.h) through its host query rls_isco_launch_plan, against the
documented rule restated here in Python -- on both sides of every boundary, under every knob, and over a sweep.  No device.

The rule, from the header and the kernels' layout comment (csrc/rls_isco.hip):
  a sample's rows   two byte rows, each padded to 8 bytes, and two f32 rows (lp, pert): 2 * pad8(N) + 8 N bytes
  the list          sel_key f32 [P] and sel_idx i32 [P]: 8 P bytes, P a power of two
  a workgroup       adds what its 16 waves share (16 floats, 16 ints, a 256-bin histogram, three words) and 16 bytes
  LDS               160 KB
  capacity          the power of two >= N (the dense step: at least 64), halved while rows + list + shared part do not fit, never
                    below 64.  N = 10^4 -> 4096.  (The header said "N = 15 000: 512"; its own rule gives 1024 there -- 150 000 +
                    8192 + 1180 = 159 372 <= 163 840 -- and 512 from N = 15 447 on; the launchers have always used the rule, so
                    the example in the header is corrected and both sizes are checked here.)
  rows in scratch   (graph steps only) once rows + a 64-entry list + the shared part exceed LDS, or by RLS_ISCO_GLOBAL_ROWS: only
                    the byte rows and a list of at most 4096 entries stay in LDS; refused once those exceed it.  The dense step is
                    refused (RLS_EUNSUPPORTED) where the graph steps move their rows.
  workgroup         per sample when N >= 256 and (B <= 2 cus or N >= 1536); RLS_ISCO_FORCE_WG overrides the second half only
  wave              per sample otherwise: as many samples per workgroup as fit, at most 8 (RLS_ISCO_WAVES); the list is halved
                    while it stays >= 512 entries and the halving gains a resident sample (not under RLS_ISCO_SEL_CAP)
  RLS_ISCO_SEL_CAP  replaces the capacity if it is a power of two >= 2 below it
"""
import itertools

import pytest

from rlsolver_amd import _abi
from rlsolver_amd.envs.env_ISCO_maxcut import isco_launch_plan

LDS = 160 * 1024
SHARED = (16 * 4 + 16 * 4 + 256 * 4 + 3 * 4) + 16
RLS_EUNSUPPORTED = -2
KNOBS = ("RLS_ISCO_SEL_CAP", "RLS_ISCO_FORCE_WG", "RLS_ISCO_GLOBAL_ROWS", "RLS_ISCO_WAVES")


def pad8(n):
    return (n + 7) // 8 * 8


def rows_bytes(N):
    return 2 * pad8(N) + 8 * N


def next_pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def is_pow2(v):
    return v >= 1 and v & (v - 1) == 0


def rule(N, B, cus, dense, cap=None, force_wg=None, global_rows=None, waves=None):
    """The documented rule -> the dictionary of isco_launch_plan."""
    rows = rows_bytes(N)

    def fitted(P, room):          # halved while the list does not fit beside `room` bytes, never below 64; then the forced capacity
        while P > 64 and room + 8 * P + SHARED > LDS:
            P //= 2
        return cap if cap is not None and cap >= 2 and is_pow2(cap) and cap < P else P

    out = dict(form="wave", wg=False, grows=False, P=0, Pw=0, waves=0, lds=0, err=0, need=rows + 64 * 8 + SHARED)
    rows_fit = out["need"] <= LDS
    if not dense and (not rows_fit or global_rows):
        byte_rows = 2 * pad8(N)
        out.update(form="workgroup, rows in scratch", wg=True, grows=True, waves=1, need=byte_rows + 64 * 8 + SHARED)
        if out["need"] > LDS:
            out["err"] = RLS_EUNSUPPORTED
            return out
        P = fitted(min(max(next_pow2(N), 64), 4096), byte_rows)
        out.update(P=P, Pw=P, lds=byte_rows + 8 * P + SHARED)
        return out
    if not rows_fit:
        out["err"] = RLS_EUNSUPPORTED
        return out
    P = fitted(max(next_pow2(N), 64 if dense else 1), rows)
    by_choice = (B <= 2 * cus or N >= 1536) if force_wg is None else force_wg != 0
    wg = by_choice and N >= 256
    max_waves = 8 if waves is None else waves

    def resident(c):
        return min(max_waves, LDS // (rows + 8 * c))

    Pw = P
    if not wg and cap in (None, 0):
        while Pw > 512 and resident(Pw // 2) > resident(Pw):
            Pw //= 2
    w = max(1, resident(Pw))
    out.update(form="workgroup" if wg else "wave", wg=wg, P=P, Pw=Pw, waves=w, lds=rows + 8 * P + SHARED if wg else (rows + 8 * Pw) * w)
    return out


class knobs:
    def __init__(self, cap=None, force_wg=None, global_rows=None, waves=None):
        self.values = dict(zip(KNOBS, (cap, force_wg, global_rows, waves)))

    def __enter__(self):
        for k, v in self.values.items():
            if v is not None:
                _abi.tuning_set(k, v)

    def __exit__(self, *exc):
        for k in KNOBS:
            _abi.tuning_unset(k)


def check(N, B, cus, dense, **kn):
    with knobs(**kn):
        got = isco_launch_plan(N, B, cus, dense)
    want = rule(N, B, cus, dense, **kn)
    if want["err"]:          # a refusal answers the code and the bytes only
        assert got["err"] == want["err"] and got["need"] == want["need"] and got["need"] > LDS, (N, B, cus, dense, kn, got, want)
    else:
        assert got == want, (N, B, cus, dense, kn, got, want)
    return got


def _last_fitting(bytes_of):
    """the largest N with bytes_of(N) <= LDS (bytes_of grows with N, in steps at every multiple of 8)"""
    lo, hi = 1, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if bytes_of(mid) <= LDS else (lo, mid)
    return lo


def test_shared_part_and_row_bytes_are_the_layout_comments():
    """need = rows + the smallest list + the shared part, at sizes whose padding differs"""
    for N in (1, 7, 8, 9, 64, 1001):
        assert isco_launch_plan(N, 1, 256, False)["need"] == 2 * pad8(N) + 8 * N + 512 + SHARED
    assert SHARED == 1180 and rows_bytes(9) == 32 + 72


def test_rows_leave_lds_at_the_documented_size():
    """The last N whose rows fit LDS and the first that does not: the graph steps move the f32 rows to scratch, the dense step
    refuses with the byte count; past the byte rows' own limit the graph steps refuse too."""
    n_fit = _last_fitting(lambda n: rows_bytes(n) + 512 + SHARED)
    assert n_fit == 16_214                                                 # 10 N + 512 + 1180 <= 163 840 (the documents' "~16 000")
    for B in (1, 5000):
        a, b = check(n_fit, B, 256, False), check(n_fit + 1, B, 256, False)
        assert a["form"] == "workgroup" and not a["grows"] and a["P"] == 64 and a["lds"] <= LDS
        assert b["form"] == "workgroup, rows in scratch" and b["grows"] and b["wg"] and b["P"] == 4096 and b["err"] == 0
    d_fit = n_fit // 8 * 8
    a, b = check(d_fit, 3, 256, True), check(d_fit + 8, 3, 256, True)
    assert a["err"] == 0 and a["P"] == 64 and not a["grows"]
    assert b["err"] == RLS_EUNSUPPORTED and b["need"] > LDS and b["need"] == rows_bytes(d_fit + 8) + 512 + SHARED
    g_fit = _last_fitting(lambda n: 2 * pad8(n) + 512 + SHARED)
    assert 81_000 < g_fit < 81_200                                         # "~81 000"
    a, b = check(g_fit, 3, 256, False), check(g_fit + 1, 3, 256, False)
    assert a["grows"] and a["err"] == 0 and a["P"] == 64 and a["lds"] <= LDS
    assert b["err"] == RLS_EUNSUPPORTED and b["need"] == 2 * pad8(g_fit + 1) + 512 + SHARED > LDS
    # rows in scratch: the list is the power of two >= N up to 4096, halved while it does not fit beside the byte rows
    assert check(20_000, 4, 256, False)["P"] == 4096 and check(70_000, 4, 256, False)["P"] == 2048
    assert check(80_000, 4, 256, False)["P"] == 256


def test_list_capacities():
    """The power of two >= N while it fits, then what the rows leave, at least 64; the dense step keeps 64 entries at any Np."""
    for N, P in ((1, 1), (2, 2), (3, 4), (63, 64), (64, 64), (65, 128), (2048, 2048), (2049, 4096), (4096, 4096), (4097, 8192), (8192, 8192),
                 (9712, 8192), (9713, 4096), (10_000, 4096), (15_000, 1024), (15_446, 1024), (15_447, 512), (15_500, 512), (15_856, 512),
                 (15_857, 256), (16_100, 128), (16_200, 64)):
        assert check(N, 3, 256, False)["P"] == P, N
    # 16 384 entries beside the rows of 8193 nodes: 81 944 + 131 072 > LDS, halved once
    assert check(8193, 3, 256, False)["P"] == 8192
    for Np, P in ((8, 64), (64, 64), (72, 128), (2048, 2048), (2056, 4096), (10_000, 4096), (15_000, 1024), (15_496, 512)):
        assert check(Np, 3, 256, True)["P"] == P, Np


def test_wave_or_workgroup_crossovers():
    cus = 256
    for dense in (False, True):
        # N >= 256: a workgroup per sample up to two samples per CU, a wave per sample beyond
        for N in (256, 264, 1024, 1528):
            assert check(N, 2 * cus, cus, dense)["form"] == "workgroup" and check(N, 2 * cus + 1, cus, dense)["form"] == "wave", N
        assert check(248, 1, cus, dense)["form"] == "wave" and check(256, 1, cus, dense)["form"] == "workgroup"
        # N >= 1536: the workgroup kernel at any batch
        assert check(1528, 100_000, cus, dense)["form"] == "wave" and check(1536, 100_000, cus, dense)["form"] == "workgroup"
    assert check(255, 1, cus, False)["form"] == "wave" and check(1535, 100_000, cus, False)["form"] == "wave"
    # the crossover follows the CU count it is given
    assert check(500, 9, 4, False)["form"] == "wave" and check(500, 8, 4, False)["form"] == "workgroup"


def test_wave_form_gives_up_capacity_only_for_a_resident_sample_and_never_below_512():
    cus, B = 256, 100_000
    # G22-sized rows: 2048 entries x 4 samples -> 512 x 6 (the header's example) -- forced, as from 1536 nodes a workgroup runs
    got = check(2000, B, cus, False, force_wg=0)
    assert got["form"] == "wave" and got["P"] == 2048 and got["Pw"] == 512 and got["waves"] == 6
    for N in (600, 1000, 1400):
        got = check(N, B, cus, False)
        rows = rows_bytes(N)
        assert got["Pw"] >= 512 or got["Pw"] == got["P"]
        if got["Pw"] < got["P"]:      # each halving gained a sample; one more would not, or would go below 512
            assert min(8, LDS // (rows + 8 * got["Pw"])) > min(8, LDS // (rows + 16 * got["Pw"]))
            assert got["Pw"] == 512 or min(8, LDS // (rows + 4 * got["Pw"])) == got["waves"]
        assert got["lds"] == (rows + 8 * got["Pw"]) * got["waves"] <= LDS
    # a small row keeps its whole list: eight samples are resident anyway
    got = check(200, B, cus, False)
    assert got["Pw"] == got["P"] == 256 and got["waves"] == 8
    with knobs(force_wg=0):
        big = isco_launch_plan(10_000, B, cus, False)
    assert big["form"] == "wave" and big["Pw"] == big["P"] == 4096 and big["waves"] == 1     # halving gains nothing: kept
    # past 2048 nodes (keys re-read from LDS): 4096 entries -> 512 for 3 -> 6 resident samples
    got = check(2049, B, cus, False, force_wg=0)
    assert got["form"] == "wave" and (got["P"], got["Pw"], got["waves"]) == (4096, 512, 6)


def test_sel_cap_takes_only_powers_of_two_from_2_below_the_capacity():
    for dense, N in ((False, 1000), (True, 1000), (False, 20_000)):
        P = check(N, 3, 256, dense)["P"]
        assert P in (1024, 4096)
        for cap in (2, 16, 64, P // 2):
            assert check(N, 3, 256, dense, cap=cap)["P"] == cap, (N, cap)
        for cap in (0, 1, 3, 17, 24, P, 2 * P):
            assert check(N, 3, 256, dense, cap=cap)["P"] == P, (N, cap)
    # the wave form takes the forced capacity as it is (and does not halve a capacity it was told to keep)
    got = check(1400, 100_000, 256, False, cap=1024)
    assert got["form"] == "wave" and got["P"] == got["Pw"] == 1024
    got = check(64, 9, 256, False, cap=16)
    assert got["form"] == "wave" and got["Pw"] == 16 and got["waves"] == 8 and got["lds"] == 8 * (rows_bytes(64) + 128)


def test_force_wg_cannot_give_a_small_row_to_a_workgroup():
    for dense in (False, True):
        assert check(248, 1, 256, dense, force_wg=1)["form"] == "wave"
        assert check(256, 100_000, 256, dense, force_wg=1)["form"] == "workgroup"
        assert check(256, 1, 256, dense, force_wg=0)["form"] == "wave"
        assert check(2056, 1, 256, dense, force_wg=0)["form"] == "wave"
    assert check(255, 1, 256, False, force_wg=1)["form"] == "wave"


def test_global_rows_knob_moves_the_graph_steps_only():
    for N in (1, 256, 1025, 3000):
        got = check(N, 3, 256, False, global_rows=1)
        assert got["form"] == "workgroup, rows in scratch" and got["P"] == max(64, next_pow2(N)) and got["lds"] == 2 * pad8(N) + 8 * got["P"] + SHARED
    assert check(256, 3, 256, False, global_rows=1, cap=16)["P"] == 16
    assert check(256, 3, 256, False, global_rows=0)["form"] == "workgroup"
    assert check(256, 3, 256, True, global_rows=1) == check(256, 3, 256, True)       # not built for the dense step


def test_waves_knob_bounds_the_samples_of_a_workgroup():
    for wv in (1, 2, 4, 8):
        got = check(64, 1000, 256, False, waves=wv)
        assert got["waves"] == wv and got["lds"] == wv * (rows_bytes(64) + 8 * 64)
    assert check(64, 1000, 256, False)["waves"] == 8
    got = check(1400, 100_000, 256, False, waves=4)       # four resident samples whatever the list: nothing to gain, 2048 kept
    assert got["Pw"] == 2048 and got["waves"] == 4
    assert check(64, 1000, 256, False, waves=0)["waves"] == 1


def test_invariants_over_a_sweep():
    """What tools/host_sanitize.cpp checks over random shapes, here over a grid that brackets every boundary, and the rule itself."""
    sizes = (1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 1535, 1536, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 10_000, 15_000, 15_856,
             15_857, 16_214, 16_215, 20_000, 44_000, 81_000, 82_000, 100_000)
    n = 0
    for cap, fwg, gr, wv in itertools.product((None, 16, 64, 1024), (None, 0, 1), (None, 1), (None, 1, 4, 8)):
        for N, B, cus, dense in itertools.product(sizes, (1, 9, 513, 40_000), (1, 256, 304), (False, True)):
            Nd = pad8(N) if dense else N
            p = check(Nd, B, cus, dense, cap=cap, force_wg=fwg, global_rows=gr, waves=wv)
            n += 1
            if p["err"]:
                continue

            def list_ok(P):
                return is_pow2(P) and (P >= 64 or P == cap or (not dense and P >= Nd))

            assert list_ok(p["P"]) and list_ok(p["Pw"]) and p["Pw"] <= p["P"] and p["lds"] <= LDS and 1 <= p["waves"] <= 8, (Nd, B, cus, p)
            assert (not p["grows"] or (p["wg"] and not dense)) and (not p["wg"] or p["grows"] or Nd >= 256), (Nd, B, cus, p)
            if not p["wg"]:
                assert p["waves"] * (rows_bytes(Nd) + 8 * p["Pw"]) == p["lds"], (Nd, B, cus, p)
    assert n == 4 * 3 * 2 * 4 * len(sizes) * 4 * 3 * 2


def test_query_rejects_bad_arguments_and_is_a_host_entry_point():
    from rlsolver_amd import torch_ops
    assert "isco_launch_plan" in torch_ops.HOST_ENTRY_POINTS
    with pytest.raises(_abi.RlsError, match="out is NULL"):
        _abi.call("rls_isco_launch_plan", 64, 1, 256, 0, None)
    for N, B, cus, dense in ((0, 1, 256, False), (2 ** 31, 1, 256, False), (64, -1, 256, False), (64, 1, 0, False), (12, 1, 256, True)):
        with pytest.raises(_abi.RlsError):
            isco_launch_plan(N, B, cus, dense)
    assert isco_launch_plan(64, 0, 256, False)["form"] == "wave"


def test_env_accessors_exist_without_a_device():
    from rlsolver_amd.envs.env_ISCO_maxcut import ISCO_maxcut
    from rlsolver_amd.envs.env_ISCO_MIS import ISCO_MIS
    from rlsolver_amd.envs.env_PISCO_maxcut import PISCO_maxcut
    assert ISCO_MIS.launch_plan is ISCO_maxcut.launch_plan and callable(PISCO_maxcut.launch_plan)
