"""tests/glue_oracle.py against the functions the project already trusts (numpy's argmin / packbits, oracle_np.mcpg_merge_best and
oracle_np.mcpg_get_return) on finite inputs, its non-finite rules on small hand-checked cases, and the dispatch constants that
tests/test_gpu_mcpg_glue.py imports against the numbers the launchers' comments state.  CPU only."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import glue_oracle as go


@pytest.mark.parametrize("N,C", [(1, 1), (7, 63), (5, 64), (9, 65), (33, 130), (3, 577)])
def test_pack_and_unpack_are_inverses_and_match_packbits(N, C):
    rng = np.random.RandomState(N + C)
    x = rng.randint(0, 2, size=(N, C)).astype(np.float32)
    words = go.pack_words(x)
    assert words.dtype == np.uint64 and words.shape == ((C + 63) // 64, N)
    tiles = (C + 63) // 64
    pad = np.zeros((N, tiles * 64), np.uint8)
    pad[:, :C] = x
    want = np.packbits(pad, axis=1, bitorder="little").reshape(N, tiles, 8).copy().view(np.uint64)[:, :, 0].T
    assert np.array_equal(words, want)
    assert np.array_equal(go.unpack_words(words, C), x)
    for dt in (np.uint8, bool):
        assert np.array_equal(go.pack_words(x.astype(dt)), words)
    junk = rng.randint(0, 1 << 62, size=words.shape).astype(np.uint64) | (np.uint64(1) << np.uint64(63))
    assert np.array_equal(go.pack_words(go.unpack_words(junk, C)), go.mask_past(junk, C))


def test_pack_rules_beyond_zero_and_one():
    f = np.array([[-1.0, -0.0, 0.5, 2.0, np.nan, 0.0, 1.0]], np.float32)
    assert int(go.pack_words(f)[0, 0]) == 0b1001100                  # float32: > 0
    u = np.array([[2, 255, 0, 1]], np.uint8)
    assert int(go.pack_words(u)[0, 0]) == 0b1011                     # uint8: != 0


@pytest.mark.parametrize("M,R", [(1, 1), (1, 9), (64, 2), (65, 17), (130, 9)])
@pytest.mark.parametrize("num_edges", [0, 4999, 20000])
def test_pick_is_argmin_over_repeats_on_finite_input(M, R, num_edges):
    rng = np.random.RandomState(M * 31 + R)
    expected = rng.randint(-6, 6, size=M * R).astype(np.float32) * np.float32(0.5)       # many ties
    idx, vs = go.pick(expected, M, R, num_edges)
    br = np.argmin(expected.reshape(R, M), axis=0)                   # numpy keeps the first minimum
    assert np.array_equal(idx, np.arange(M) + br * M)
    assert vs.dtype == np.float32 and np.array_equal(vs, (np.float32(num_edges) - expected[idx]) / np.float32(2))


def test_pick_non_finite_rule():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    #                m = 0     1     2     3     4
    e = np.array([nan,  3.0,  inf, -inf,  1.0,              # repeat 0
                  1.0,  nan, -inf, -inf,  1.0,              # repeat 1
                  0.0,  2.0, -inf,  5.0,  0.5], np.float32)  # repeat 2
    idx, vs = go.pick(e, 5, 3, 0)
    assert idx.tolist() == [0, 11, 7, 3, 14]      # NaN first stays; NaN later skipped; first -inf; -inf tie: first; plain
    assert np.isnan(vs[0]) and vs[1:].tolist() == [-1.0, inf, inf, -0.25]


@pytest.mark.parametrize("M,N", [(1, 5), (5, 77), (64, 3), (70, 50), (130, 9)])
def test_merge_follows_the_trusted_oracle_on_finite_input(M, N):
    rng = np.random.RandomState(M + N)
    for trial in range(4):
        temp_max = rng.randint(0, 8, M).astype(np.float32)            # ties in both vectors
        now_res = rng.randint(0, 8, M).astype(np.float32) if trial else np.full(M, 9.0, np.float32)
        temp_info = rng.randint(0, 2, size=(N, M)).astype(np.float32)
        now_info = rng.randint(0, 2, size=(N, M)).astype(np.float32)
        w_res, w_info, w_temp, w_max, w_idx = onp.mcpg_merge_best(temp_max, temp_info, now_res, now_info)
        res, info, temp, vals, idxs = go.merge(temp_max, go.pack_words(temp_info), now_res, go.pack_words(now_info))
        assert np.array_equal(res, w_res) and np.array_equal(go.unpack_words(info, M), w_info)
        assert np.array_equal(go.unpack_words(temp, M), w_temp) and vals.tolist() == [w_max] and idxs.tolist() == [w_idx]
        res2, info2, temp2, vals2, idxs2 = go.merge(temp_max, go.pack_words(temp_info), now_res, go.pack_words(now_info), False)
        merged = np.maximum(temp_max, now_res)
        assert np.array_equal(res2, merged) and np.array_equal(temp2, go.pack_words(temp_info))
        assert vals2.tolist() == [merged.max(), merged.min()] and idxs2.tolist() == [int(merged.argmax()), int(merged.argmin())]
        taken = temp_max > now_res
        assert np.array_equal(go.unpack_words(info2, M), np.where(taken[None, :], temp_info, now_info))


def test_best_and_worst_rule_on_non_finite_values():
    nan, inf = np.nan, np.inf
    f = lambda v: (go.first_extreme(np.array(v, np.float32), True), go.first_extreme(np.array(v, np.float32), False))
    assert f([nan, nan, nan]) == (0, 0)                          # torch.argmax / argmin of all NaN
    assert f([-inf, -inf]) == (0, 0) and f([inf, inf, inf]) == (0, 0)
    assert f([nan, 2.0, 3.0, nan, 1.0]) == (2, 4)                # NaN is skipped (the reference would pick index 0 twice)
    assert f([nan, -inf, nan, -inf]) == (1, 1)
    assert f([nan, inf, -inf, inf]) == (1, 2)
    assert f([1.0, 2.0, 2.0, 1.0]) == (1, 0)


@pytest.mark.parametrize("N,C,M,R", [(20, 70, 35, 2), (33, 130, 130, 1), (7, 192, 64, 3)])
def test_bit_sums_are_the_gradient_term_of_get_return(N, C, M, R):
    rng = np.random.RandomState(C)
    probs = rng.rand(N) * 0.6 + 0.2
    s = rng.randint(0, 2, size=(C, N)).astype(np.float32)
    value = rng.randn(C).astype(np.float32)
    words = go.pack_words(s.T)
    words[-1] |= ~go.mask_past(np.full_like(words, ~np.uint64(0)), C)[-1]            # garbage past C must not count
    A = go.bit_sums_exact(words, C, value)
    assert np.allclose(A, s.astype(np.float64).T @ value.astype(np.float64), rtol=1e-13, atol=1e-13)
    _, grad = onp.mcpg_get_return(probs, s, value, M, R)
    V = value.astype(np.float64).sum()
    assert np.allclose((A / probs - (V - A) / (1 - probs)) / C, grad, rtol=1e-11, atol=1e-13)
    assert np.allclose(go.bit_sums_abs(words, C, value), s.astype(np.float64).T @ np.abs(value.astype(np.float64)), rtol=1e-13)
    for chunk in (1, 2, 5):
        assert np.allclose(go.bit_sums_many(words, C, value[:, None], chunk=chunk)[:, 0], A, rtol=1e-14, atol=1e-14)


def test_bit_sums_select_non_finite_values():
    value = np.array([1.0, np.inf, -np.inf, np.nan, 2.0], np.float32)
    x = np.array([[1, 0, 0, 0, 1],      # finite: 3
                  [1, 1, 0, 0, 0],      # +inf
                  [0, 0, 1, 0, 1],      # -inf
                  [0, 1, 1, 0, 0],      # inf - inf
                  [1, 0, 0, 1, 0],      # NaN
                  [0, 0, 0, 0, 0]], np.float32)
    A = go.bit_sums_exact(go.pack_words(x), 5, value)
    assert A[0] == 3.0 and A[1] == np.inf and A[2] == -np.inf and np.isnan(A[3]) and np.isnan(A[4]) and A[5] == 0.0


def test_dispatch_constants():
    """The numbers the launchers' comments and the issue of record state, from the restated arithmetic."""
    assert (go.BITSUM_REG_MAX_N, go.BITSUM_LDS_MIN_N) == (12288, 12289)
    assert (go.BITSUM_LDS_MAX_N, go.BITSUM_ATOMIC_MIN_N) == (18368, 18369)
    assert go.BITSUM_FIXED_LDS == 8448 and go.BITSUM_FIXED_LDS + 4 * go.BITSUM_LDS_MAX_N == go.LDS_BYTES // 2
    assert (go.BITSUM_REG_GRID, go.BITSUM_LDS_GRID) == (1024, 512) and go.bitsum_grid(go.BITSUM_LDS_MAX_N, 1 << 30) == 512
    assert go.bitsum_grid(70, 64 * 1024 + 3 * 64 + 5) == 1024 and go.bitsum_grid(12289, 512 * 64 + 64 + 5) == 512
    assert go.bitsum_grid(70, 130) == 3
    assert [go.bitsum_form(n) for n in (1, 12288, 12289, 18368, 18369)] == ["regs", "regs", "lds", "lds", "atomic"]
    assert (go.PACK_LINE_N_END, go.PACK_N_END, go.UNPACK_SWEEP_ROWS) == (1 << 21, 1 << 22, 32768)
    assert go.MERGE_THREADS == 1024 and go.PICK_UNROLL == 8
