"""Every form of the glue that ends an MCPG round -- rls_mcpg_pick_best, rls_mcpg_merge_best, rls_mcpg_value_bit_sums,
rls_mcpg_pack_chains, rls_mcpg_unpack_chains: thirteen kernels -- against tests/glue_oracle.py, bit for bit, and the
all-NaN / all-infinite rule of k_mcpg_merge_minmax and k_best_update.

    bit sums   k_mcpg_value_bit_sums_lut<true>   N <= 12 288 (sums in registers, 1024 resident workgroups)
               k_mcpg_value_bit_sums_lut<false>  12 289 <= N <= 18 368 (sums in LDS, 512 workgroups)
               k_mcpg_value_bit_sums             N >= 18 369 (one atomic per tile and node)
    pack       k_mcpg_pack_f32x4                 f32, C % 4 == 0, 16-byte aligned base, N < 2^21, RLS_MCPG_SHIM & 15 != 0;
                                                 1 / 2 / 4 spans per wave from the knob's bits 4..7
               k_mcpg_pack<float>, <uint8_t>     everything else; refused from N = 2^22
    unpack     k_mcpg_unpack<true, true, 2>      C % 4 == 0 and aligned: two rows per thread, 32 768 rows per grid.y sweep
               k_mcpg_unpack<true>               the same with RLS_MCPG_SHIM = 0
               k_mcpg_unpack<false>              every other C or base
    pick       k_mcpg_pick_argmin, then k_mcpg_pick_gather (f32) or k_mcpg_pick_gather_packed
    merge      k_mcpg_merge_mask, k_mcpg_merge_apply, k_mcpg_merge_minmax (one workgroup of 1024 threads)

The boundaries come from tests/glue_oracle.py (tests/test_glue_oracle.py checks them); every launch writes into guarded
outputs (tests/glue_checks.py).  The only inexact comparison is the bit sums of Gaussian values, held to the worst-case bound
of a float32 sum of C terms in any order."""
import numpy as np
import pytest
import torch

from rlsolver_amd import _abi
from tests import glue_checks as gc
from tests import glue_oracle as go
from tests.glue_checks import DEV, dev, host

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ bit sums
BITSUM_N = [1, 511, 512, 513, 2047, 2048, 2049, go.BITSUM_REG_MAX_N - 1, go.BITSUM_REG_MAX_N,      # 2048: the uniform `break`
            go.BITSUM_LDS_MIN_N, go.BITSUM_LDS_MAX_N, go.BITSUM_ATOMIC_MIN_N]
BITSUM_C = [1, 63, 64, 65, 130]


def planted_words(rng, tiles, N):
    """Random words (garbage past C included) with a few all-zero and all-one nodes."""
    words = gc.random_words(rng, tiles, N)
    for k, n in enumerate(sorted({0, N // 3, N // 2, N - 2 if N > 1 else 0, N - 1})):
        words[:, n] = np.uint64(0) if k % 2 else ~np.uint64(0)
    return words


def int_values(rng, C):
    v = rng.randint(-1024, 1025, size=C).astype(np.float32)
    v[rng.randint(C)] = 1024.0
    return v


def half_values(rng, C):
    return rng.randint(-2048, 2049, size=C).astype(np.float32) * np.float32(0.5)


@pytest.mark.parametrize("C", BITSUM_C)
@pytest.mark.parametrize("N", BITSUM_N)
def test_bit_sums_every_form_and_tile_edge(N, C):
    rng = np.random.RandomState(N * 7 + C)
    values = [int_values(rng, C), half_values(rng, C)]
    if C == 130:
        values.append(rng.randn(C).astype(np.float32))
    gc.check_bit_sums(planted_words(rng, (C + 63) // 64, N), C, values, f"N={N} C={C} {go.bitsum_form(N)}")


@pytest.mark.parametrize("N,C", [(70, go.BITSUM_REG_GRID * 64 + 3 * 64 + 5), (go.BITSUM_LDS_MIN_N, go.BITSUM_LDS_GRID * 64 + 64 + 5)])
def test_bit_sums_tile_loop_runs_past_the_resident_grid(N, C):
    """More tiles than workgroups: tile += gridDim.x takes a second trip in the first workgroups only."""
    tiles = (C + 63) // 64
    assert tiles > go.bitsum_grid(N, C) and go.bitsum_grid(N, C) == (go.BITSUM_REG_GRID if N == 70 else go.BITSUM_LDS_GRID)
    rng = np.random.RandomState(N)
    gc.check_bit_sums(planted_words(rng, tiles, N), C, [int_values(rng, C), half_values(rng, C), rng.randn(C).astype(np.float32)],
                      f"N={N} C={C} tile loop")


@pytest.mark.parametrize("N,C", [(513, 130), (2049, 65), (go.BITSUM_LDS_MIN_N, 130), (go.BITSUM_ATOMIC_MIN_N, 130), (70, go.BITSUM_REG_GRID * 64 + 70)])
def test_bit_sums_of_non_finite_values(N, C):
    """+inf, -inf and NaN in known chains: A is NaN / +-inf exactly where the float64 sum of the selected values is."""
    rng = np.random.RandomState(N + C)
    tiles = (C + 63) // 64
    words = planted_words(rng, tiles, N)
    value = int_values(rng, C)
    spots = {3 % C: np.inf, (C - 1): np.nan, C // 2: -np.inf, (C - 2) % C: np.inf}
    for c, x in spots.items():
        value[c] = x
    # thin the non-finite chains so that a good share of the nodes keeps a finite sum
    for c in spots:
        keep = np.frombuffer(rng.bytes(N), np.uint8) < 48
        words[c >> 6] &= ~(np.uint64(1) << np.uint64(c & 63)) | (keep.astype(np.uint64) << np.uint64(c & 63))
    exact = go.bit_sums_exact(words, C, value)
    assert np.isnan(exact).any() and np.isposinf(exact).any() and np.isneginf(exact).any() and np.isfinite(exact).sum() > N // 4
    gc.check_bit_sums(words, C, [value], f"N={N} C={C} non-finite")


@pytest.mark.parametrize("N", [513, go.BITSUM_LDS_MIN_N, go.BITSUM_ATOMIC_MIN_N])
@pytest.mark.parametrize("C", [1, 65, 130])
def test_bit_sums_ignore_garbage_past_C(N, C):
    rng = np.random.RandomState(N + C)
    tiles = (C + 63) // 64
    clean = go.mask_past(gc.random_words(rng, tiles, N), C)
    dirty = clean.copy()
    dirty[-1] |= ~go.mask_past(np.full((tiles, N), ~np.uint64(0)), C)[-1]
    value = int_values(rng, C)
    a, b = gc.run_bit_sums(dev(clean), C, value), gc.run_bit_sums(dev(dirty), C, value)
    assert np.array_equal(a, b) and np.array_equal(a, go.bit_sums_exact(clean, C, value).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------- pack
PACK_N = [1, 15, 16, 17, 63, 64, 65, 1001]
LINE_C = [4, 60, 64, 68, 252, 256, 260, 1028]
GENERIC_C = [1, 63, 65, 511, 513, 577]


@pytest.mark.parametrize("C", LINE_C)
@pytest.mark.parametrize("knob", [1, 0x21, 0x31])
def test_pack_line_wide_form_at_1_2_and_4_spans(knob, C):
    for N in PACK_N:
        rng = np.random.RandomState(N * 1031 + C)
        gc.check_pack(gc.draw_chains(rng, N, C, "f32"), knob, "k_mcpg_pack_f32x4", f"N={N} C={C} knob={knob:#x}")


@pytest.mark.parametrize("C", GENERIC_C)
@pytest.mark.parametrize("kind", ["f32", "u8", "bool"])
def test_pack_generic_forms(kind, C):
    for N in PACK_N:
        rng = np.random.RandomState(N * 1031 + C)
        form = "k_mcpg_pack<float>" if kind == "f32" else "k_mcpg_pack<uint8_t>"
        gc.check_pack(gc.draw_chains(rng, N, C, kind), None, form, f"N={N} C={C} {kind}")


@pytest.mark.parametrize("C", [4, 64, 260, 1028])
def test_pack_generic_form_with_the_knob_off_and_off_the_line(C):
    for N in PACK_N:
        rng = np.random.RandomState(N * 1031 + C)
        x = gc.draw_chains(rng, N, C, "f32")
        gc.check_pack(x, 0, "k_mcpg_pack<float>", f"N={N} C={C} knob=0")
        gc.check_pack(x, 0x20, "k_mcpg_pack<float>", f"N={N} C={C} knob=0x20")          # bits 0..3 clear: off as well
        gc.check_pack(gc.off_line(x), None, "k_mcpg_pack<float>", f"N={N} C={C} base + 4 bytes")
        gc.check_pack(gc.draw_chains(rng, N, C, "u8"), None, "k_mcpg_pack<uint8_t>", f"N={N} C={C} u8")


@pytest.mark.parametrize("N,form", [(go.PACK_LINE_N_END - 1, "k_mcpg_pack_f32x4"), (go.PACK_LINE_N_END, "k_mcpg_pack<float>")])
def test_pack_at_the_line_wide_forms_node_limit(N, form):
    rng = np.random.RandomState(5)
    gc.check_pack(gc.draw_chains(rng, N, 4, "f32"), None, form, f"N={N} C=4")


def test_pack_refuses_two_to_the_22_nodes():
    x = torch.zeros((go.PACK_N_END, 1), dtype=torch.uint8, device=DEV)
    words = torch.full((1, go.PACK_N_END), 0x5A, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"rls_mcpg_pack_chains failed \(-2\)"):
        gc._t.mcpg_pack_chains(x, words)
    assert _abi.ERROR_NAMES[-2] == "RLS_EUNSUPPORTED" and bool(words.eq(0x5A).all())
    x1 = torch.ones((go.PACK_N_END - 1, 1), dtype=torch.uint8, device=DEV)                # the last N that is taken
    w1 = gc.check_pack(x1, None, "k_mcpg_pack<uint8_t>", "N=2^22-1")
    assert bool(w1.eq(1).all())


# -------------------------------------------------------------------------------------------------------------------- unpack
SWEEP = go.UNPACK_SWEEP_ROWS


@pytest.mark.parametrize("N", [1, 2, 3, 1001, SWEEP, SWEEP + 1, 2 * SWEEP + 1])
def test_unpack_two_row_form_on_odd_counts_and_past_one_sweep(N):
    words = gc.random_words(np.random.RandomState(N), 1, N)
    gc.check_unpack(words, 4, None, 0, "k_mcpg_unpack<true,true,2>", f"N={N} C=4")
    if N in (3, SWEEP + 1):
        gc.check_unpack(words, 4, 0, 0, "k_mcpg_unpack<true>", f"N={N} C=4 knob=0")


@pytest.mark.parametrize("C", [60, 64, 68, 1024, 1028])
def test_unpack_chain_counts_around_a_tile_and_a_block(C):
    for N in (7, 3):
        words = gc.random_words(np.random.RandomState(C), (C + 63) // 64, N)
        gc.check_unpack(words, C, None, 0, "k_mcpg_unpack<true,true,2>", f"N={N} C={C}")
        gc.check_unpack(words, C, 0, 0, "k_mcpg_unpack<true>", f"N={N} C={C} knob=0")
        gc.check_unpack(words, C, None, 4, "k_mcpg_unpack<false>", f"N={N} C={C} base + 4 bytes")


@pytest.mark.parametrize("C", GENERIC_C + [2, 130])
def test_unpack_element_form(C):
    for N in (1, 7, 1001):
        words = gc.random_words(np.random.RandomState(C + N), (C + 63) // 64, N)
        gc.check_unpack(words, C, None, 0, "k_mcpg_unpack<false>", f"N={N} C={C}")


INVERSE_SHAPES = [(PACK_N, c) for c in LINE_C + GENERIC_C] + [((2, 3, SWEEP, SWEEP + 1, 2 * SWEEP + 1), 4), ((7,), 1024)]


@pytest.mark.parametrize("Ns,C", INVERSE_SHAPES)
def test_pack_and_unpack_are_inverses(Ns, C):
    """Every pack and unpack shape of this file: pack(unpack(words)) == words (bits past C cleared), unpack(pack(x)) == x."""
    for N in Ns:
        _inverses(N, C)


def _inverses(N, C):
    rng = np.random.RandomState(N + C)
    words = gc.random_words(rng, (C + 63) // 64, N)
    xs = gc.check_unpack(words, C, None, 0, None, f"N={N} C={C}")
    back = gc.check_pack(xs, None, None, f"N={N} C={C} pack(unpack)")
    assert np.array_equal(host(back), go.mask_past(words, C))
    x = gc.draw_chains(rng, N, C, "f32_01")
    w = gc.check_pack(x, None, None, f"N={N} C={C}")
    assert np.array_equal(host(gc.check_unpack(host(w), C, None, 0, None, f"N={N} C={C} unpack(pack)")), x)


# ---------------------------------------------------------------------------------------------------------------------- pick
PICK_M = [1, 63, 64, 65, 130]
PICK_N = [1, 255, 256, 257, 1001]
PICK_R = [1, 2, 9, 17]
PICK_E = [0, 4999, 20000]          # the Cheeger doubling (vs == -h exactly), an odd count (half-integers), an even one
PICK_CASES = [(M, N, PICK_R[(i + j) % 4], PICK_E[(i + 2 * j) % 3]) for i, M in enumerate(PICK_M) for j, N in enumerate(PICK_N)]


def test_pick_cases_cover_every_axis_value():
    assert {c[2] for c in PICK_CASES} == set(PICK_R) and {c[3] for c in PICK_CASES} == set(PICK_E)
    assert {(c[0], c[1]) for c in PICK_CASES} == {(m, n) for m in PICK_M for n in PICK_N}
    assert max(PICK_R) > 2 * go.PICK_UNROLL and any(go.PICK_UNROLL < r < 2 * go.PICK_UNROLL for r in PICK_R)


@pytest.mark.parametrize("M,N,R,num_edges", PICK_CASES)
def test_pick_best_of_repeats_both_layouts(M, N, R, num_edges):
    """Six shifts of the planted features: every kept chain meets a tie, a NaN first, a NaN later, -inf, +inf and plain values."""
    for shift in range(6):
        rng = np.random.RandomState(M * 1009 + N * 7 + shift)
        bits = rng.randint(0, 2, size=(N, M * R)).astype(bool)
        gc.check_pick(bits, gc.plant_expected(rng, M, R, shift), M, R, num_edges, f"M={M} N={N} R={R} E={num_edges} shift={shift}")


@pytest.mark.parametrize("R", PICK_R)
def test_pick_with_num_edges_zero_returns_minus_h(R):
    """The Cheeger family passes expected = 2 h and num_edges = 0: vs is -h exactly, NaN and +-inf included."""
    M, N = 70, 33
    rng = np.random.RandomState(R)
    h = gc.plant_expected(rng, M, R, 1)
    idx, vs = go.pick(h * np.float32(2), M, R, 0)
    assert gc.same_f32(vs, -h[idx])
    gc.check_pick(rng.randint(0, 2, size=(N, M * R)).astype(bool), h * np.float32(2), M, R, 0, f"R={R} cheeger")


# --------------------------------------------------------------------------------------------------------------------- merge
def merge_case(rng, M, N, best, worst, via_temp):
    """Integer incumbents in 10..40 with ties everywhere; the best (60) at every index of `best`, the worst (1) at every index
    of `worst`.  via_temp: the best arrives through temp_max, so the min / max pass must see the merged values."""
    temp_max = rng.randint(10, 41, M).astype(np.float32)
    now_res = rng.randint(10, 41, M).astype(np.float32)
    for b in best:
        (temp_max if via_temp else now_res)[b] = 60.0
    for w in worst:
        temp_max[w] = now_res[w] = 1.0
        if via_temp:
            temp_max[w] = 0.0
    tiles = (M + 63) // 64
    return temp_max, gc.random_words(rng, tiles, N), now_res, gc.random_words(rng, tiles, N)


T = go.MERGE_THREADS
MERGE_PLANTS = [                                  # (best indices, worst indices): the first of each must win
    ((T + 6,), (T + 7,)),                         # neighbour bits of one word, both in a thread's second trip
    ((T + 7,), (T + 6,)),
    ((T + 6,), (T + 36,)),                        # same tile
    ((T + 6, 5), (T - 1, 200)),                   # a tie between a second-trip index and a first-trip one of another thread
    ((200, T + 6), (T + 6 - 1, 70)),              # ... where the first is in a later wave than the second's thread
    ((T - 1, T), (0, T - 1 - 64)),                # last thread / first thread's second trip; different tiles
    ((3,), (3 + 64,)),
]


@pytest.mark.parametrize("M", [T, T + 1, 2500])
@pytest.mark.parametrize("replace_worst", [True, False])
def test_merge_past_one_trip_of_the_workgroup(M, replace_worst):
    for k, (best, worst) in enumerate(MERGE_PLANTS):
        best, worst = [min(b, M - 1) for b in best], [min(w, M - 2) for w in worst]
        if set(best) & set(worst):
            continue
        for via_temp in (False, True):
            rng = np.random.RandomState(M + k)
            N = 1100 if k == 0 else 70                                      # 1100: the column copy loops as well
            gc.check_merge(*merge_case(rng, M, N, best, worst, via_temp), replace_worst, f"M={M} plant {k} via_temp={via_temp}")


@pytest.mark.parametrize("M", [1, 5, 64, 70, T + 1])
def test_merge_when_every_incumbent_is_equal(M):
    rng = np.random.RandomState(M)
    tiles = (M + 63) // 64
    for rw in (True, False):
        gc.check_merge(np.full(M, 10.0, np.float32), gc.random_words(rng, tiles, 77), np.full(M, 12.0, np.float32),
                       gc.random_words(rng, tiles, 77), rw, f"M={M} all equal")


NAN, INF = np.float32(np.nan), np.float32(np.inf)
NON_FINITE = {
    "all_nan": lambda rng, M: np.full(M, NAN),
    "all_minus_inf": lambda rng, M: np.full(M, -INF),
    "all_plus_inf": lambda rng, M: np.full(M, INF),
    "nan_and_finite": lambda rng, M: np.where(rng.rand(M) < 0.5, NAN, rng.randint(0, 9, M).astype(np.float32)).astype(np.float32),
    "minus_inf_and_nan": lambda rng, M: np.where(rng.rand(M) < 0.5, NAN, -INF).astype(np.float32),
    "nan_then_finite": lambda rng, M: np.concatenate([np.full(M - M // 3, NAN), rng.randint(0, 9, M // 3).astype(np.float32)]),
}


@pytest.mark.parametrize("M", [1, 70, T + 1, 2500])
@pytest.mark.parametrize("kind", sorted(NON_FINITE))
def test_merge_non_finite_incumbents(kind, M):
    """All NaN (a Cheeger run from empty start chains: 0 / 0), all -inf, all +inf: the kernel used to address chain INT64_MAX.
    Best and worst are the first -inf / +inf, index 0 when all is NaN; NaN mixed with numbers is skipped.  temp_max is NaN, equal
    to the incumbent or (second pass) finite and sometimes better, so that chains also move first."""
    rng = np.random.RandomState(M + len(kind))
    tiles = (M + 63) // 64
    now_res = NON_FINITE[kind](rng, M)
    for temp_max in (np.where(rng.rand(M) < 0.5, NAN, now_res).astype(np.float32), rng.randint(-3, 12, M).astype(np.float32)):
        if kind.startswith("all_") and np.isfinite(temp_max).any() and kind != "all_plus_inf":
            temp_max = np.where(rng.rand(M) < 0.9, NAN, temp_max).astype(np.float32)       # mostly stay non-finite
        for rw in (True, False):
            gc.check_merge(temp_max, gc.random_words(rng, tiles, 50), now_res, gc.random_words(rng, tiles, 50), rw, f"{kind} M={M} rw={rw}")
    for rw in (True, False):                        # and with nothing to take at all: the input stays exactly the named kind
        gc.check_merge(np.full(M, NAN), gc.random_words(rng, tiles, 50), now_res, gc.random_words(rng, tiles, 50), rw, f"{kind} M={M} pure")


# --------------------------------------------------------------------------------------------------------------- best_update
@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("fill", ["worst_inf", "nan"])
@pytest.mark.parametrize("B", [1, 70, 1500])
def test_best_update_forced_on_values_that_never_compare_better(B, fill, maximize):
    """k_best_update with force: every value -inf under maximise (+inf under minimise), or every value NaN, copies row 0 and
    reports that value; it used to address row INT64_MAX.  One planted number among NaNs is found."""
    N = 33
    rng = np.random.RandomState(B)
    xs = rng.randint(0, 2, size=(B, N)).astype(np.uint8)
    x = (-np.inf if maximize else np.inf) if fill == "worst_inf" else np.nan
    for dt in (torch.float32, torch.float64):
        for planted in (None, B - 1):
            vs = np.full(B, x)
            if planted is not None and fill == "nan":
                vs[planted] = 3.5
            g = gc.Guard()
            best_x = g.out((N,), torch.uint8)
            best_v = g.out((1,), torch.float64, fill=7.0)
            improved = g.out((1,), torch.uint8)
            log = g.out((2,), torch.float64, fill=0.0)
            gc._t.best_update(dev(xs), torch.from_numpy(vs).to(dt).to(DEV), maximize, best_x, best_v, improved, log, 1, True)
            row = planted if planted is not None and fill == "nan" else 0
            got_x, got_v, got_log = host(best_x), host(best_v), host(log)
            g.check(f"B={B} {fill}")
            assert np.array_equal(got_x, xs[row]) and int(host(improved)[0]) == 1
            assert np.array_equal(got_v, [vs[row]], equal_nan=True) and np.array_equal(got_log, [0.0, vs[row]], equal_nan=True)


@pytest.mark.parametrize("B", [1, 70, 1500])
def test_best_key_of_values_that_never_compare_greater_reports_row_zero(B):
    """k_best_key has the same start (index INT64_MAX, moved on a strict compare with -inf).  All -inf or all NaN is outside the
    key's range and raises the flag, but the flag is read by the host later while rls_winner_message already takes row
    index[0] of xs: the index must name a row that exists.  A number among them is still found."""
    for dt in (torch.float32, torch.float64):
        for x in (-np.inf, np.nan):
            for planted in (None, B - 1):
                vs = np.full(B, x)
                if planted is not None:
                    vs[planted] = 2.5
                g = gc.Guard()
                key, idx = g.out((1,), torch.int64), g.out((1,), torch.int64)
                flag = g.out((1,), torch.int32, fill=0)
                gc._t.best_key(torch.from_numpy(vs).to(dt).to(DEV), 20, 5, 1 << 42, key, idx, flag)
                got = int(host(idx).view(np.int64)[0]), int(host(flag)[0]), int(host(key).view(np.int64)[0])
                g.check(f"B={B} {x}")
                assert got == ((planted, 0, (5 << 20) | 5) if planted is not None else (0, 1, 5)), (got, B, x, planted)
