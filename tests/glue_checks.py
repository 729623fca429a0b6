"""One guarded launch per MCPG glue entry point, compared with tests/glue_oracle.py.  Shared by tests/test_gpu_mcpg_glue.py and
tools/fuzz/fuzz_mcpg_glue.py.

Every output of a launch is a view into a byte arena with canary bytes in front of it and behind it (Guard); each check_*
function asserts the canaries after the launch, so a store one element outside an output fails the test that made it instead
of corrupting a neighbour.  The ops are called through torch.ops.rlsolver_hip directly, with the outputs given."""
import contextlib

import numpy as np
import torch

from rlsolver_amd import ops_mcpg_tsp as mops
from tests import glue_oracle as go
from tests.test_gpu_step_store import knobs

DEV = torch.device("cuda:0")
_t = mops._t
PAD = 256            # canary bytes on each side; a multiple of 16, so a view keeps the arena's alignment
CANARY = 0x5A
F32_KINDS = np.array([0.0, 1.0, -1.0, -0.0, 0.5, 2.0, np.nan, 1.0, 0.0], np.float32)     # the `> 0` rule: bits 0 1 0 0 1 1 0 1 0
U8_KINDS = np.array([0, 1, 2, 255, 0, 1], np.uint8)                                       # the `!= 0` rule


def shim(value):
    """RLS_MCPG_SHIM for the block; None leaves the default."""
    return contextlib.nullcontext() if value is None else knobs(RLS_MCPG_SHIM=value)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


class Guard:
    """Output tensors carved out of canary-filled arenas."""

    def __init__(self):
        self.arenas = []

    def out(self, shape, dtype, lead=0, fill=None):
        """A contiguous tensor of `shape` that starts PAD + lead bytes into its own arena (lead = 4: off the 16-byte line)."""
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        arena = torch.full((PAD + lead + nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)
        view = arena[PAD + lead:PAD + lead + nbytes].view(dtype).view(*shape)
        assert view.data_ptr() % 16 == lead % 16
        if fill is not None:
            view.copy_(fill) if isinstance(fill, torch.Tensor) else view.fill_(fill)
        self.arenas.append((arena, PAD + lead, nbytes))
        return view

    def check(self, tag=""):
        for k, (arena, start, nbytes) in enumerate(self.arenas):
            assert bool(arena[:start].eq(CANARY).all()), f"bytes in front of output {k} were written {tag}"
            assert bool(arena[start + nbytes:].eq(CANARY).all()), f"bytes behind output {k} were written {tag}"


def off_line(a):
    """`a` on the device, contiguous, starting 4 bytes into a 16-byte line (float32 only)."""
    flat = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    v = flat[1:1 + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 4
    return v


def same_f32(got, want):
    """float32 arrays equal bit for bit, except that any NaN equals any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def random_words(rng, tiles, N):
    return np.frombuffer(rng.bytes(tiles * N * 8), np.uint64).reshape(tiles, N).copy()


def draw_chains(rng, N, C, kind):
    """[N, C] input of a pack: "f32" / "u8" draw from every value class of the rule, "f32_01" / "bool" are 0 | 1."""
    if kind == "f32":
        return F32_KINDS[rng.randint(0, len(F32_KINDS), size=(N, C))]
    if kind == "u8":
        return U8_KINDS[rng.randint(0, len(U8_KINDS), size=(N, C))]
    b = rng.randint(0, 2, size=(N, C))
    return b.astype(np.float32) if kind == "f32_01" else b.astype(bool)


# ---- pack / unpack ----
def pack_form(x, knob):
    """The kernel rls_mcpg_pack_chains takes for the device tensor x under RLS_MCPG_SHIM = knob (None: the default 1)."""
    N, C = x.shape
    k = 1 if knob is None else knob
    if x.dtype != torch.float32:
        return "k_mcpg_pack<uint8_t>"
    if (k & 15) and C % 4 == 0 and x.data_ptr() % 16 == 0 and N < go.PACK_LINE_N_END:
        return "k_mcpg_pack_f32x4"
    return "k_mcpg_pack<float>"


def check_pack(x, knob=None, form=None, tag=""):
    """x: numpy [N, C] or a device tensor (for a chosen alignment).  All words are compared, bits past C included."""
    xd = x if isinstance(x, torch.Tensor) else dev(x)
    N, C = xd.shape
    if form is not None:
        assert pack_form(xd, knob) == form, (pack_form(xd, knob), form, tag)
    g = Guard()
    words = g.out(((C + 63) // 64, N), torch.int64)
    with shim(knob):
        _t.mcpg_pack_chains(xd, words)
    got = host(words)
    g.check(tag)
    want = go.pack_words(host(xd))
    assert np.array_equal(got, want), f"pack {tag}: {int((got != want).sum())} of {want.size} words differ"
    return words


def unpack_form(N, C, lead, knob):
    k = 1 if knob is None else knob
    if C % 4 == 0 and lead % 16 == 0:
        return "k_mcpg_unpack<true,true,2>" if k != 0 else "k_mcpg_unpack<true>"
    return "k_mcpg_unpack<false>"


def check_unpack(words, C, knob=None, lead=0, form=None, tag=""):
    """words: numpy uint64 [tiles, N], garbage past C welcome."""
    tiles, N = words.shape
    if form is not None:
        assert unpack_form(N, C, lead, knob) == form, (unpack_form(N, C, lead, knob), form, tag)
    g = Guard()
    xs = g.out((N, C), torch.float32, lead=lead)
    with shim(knob):
        _t.mcpg_unpack_chains(dev(words), C, xs)
    got = host(xs)
    g.check(tag)
    want = go.unpack_words(words, C)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"unpack {tag}: {int((got != want).sum())} elements differ"
    return xs


# ---- pick ----
def plant_expected(rng, M, R, shift=0):
    """float32 [R M] of fractional values in which kept chain m carries feature (m + shift) % 6: 0 a tie between two repeats at
    the minimum, 1 a NaN in repeat 0, 2 a NaN in a later repeat, 3 -inf (twice where R allows),
    4 +inf in repeat 0 (and everywhere for every other such chain), 5 nothing."""
    e = (rng.randn(R, M) * 3).astype(np.float32)
    for m in range(M):
        f = (m + shift) % 6
        rs = rng.permutation(R)
        if f == 0 and R >= 2:
            e[rs[:2], m] = e[:, m].min() - np.float32(0.75)
        elif f == 1:
            e[0, m] = np.nan
        elif f == 2 and R >= 2:
            e[1 + rng.randint(R - 1), m] = np.nan
        elif f == 3:
            e[rs[:2], m] = -np.inf
        elif f == 4:
            e[0, m] = np.inf
            if (m // 6) % 2:
                e[:, m] = np.inf
    return e.reshape(-1)


def check_pick(bits, expected, M, R, num_edges, tag=""):
    """bits: bool [N, R M].  Both layouts against glue_oracle.pick; the packed result's bits past M are zero."""
    N = bits.shape[0]
    idx, vs = go.pick(expected, M, R, num_edges)
    chains = bits[:, idx]
    d_exp = dev(expected)
    for layout in ("f32", "packed"):
        g = Guard()
        bi = g.out((M,), torch.int64)
        vg = g.out((M,), torch.float32)
        if layout == "f32":
            xs, xg = dev(bits.astype(np.float32)), g.out((N, M), torch.float32)
        else:
            xs, xg = dev(go.pack_words(bits)), g.out(((M + 63) // 64, N), torch.int64)
        _t.mcpg_pick_best(d_exp, xs, N, M, R, num_edges, bi, vg, xg)
        got_idx, got_vs, got_x = host(bi).view(np.int64), host(vg), host(xg)
        g.check(f"{layout} {tag}")
        assert np.array_equal(got_idx, idx), f"best_index {layout} {tag}: {np.nonzero(got_idx != idx)[0][:8]}"
        assert same_f32(got_vs, vs), f"vs_good {layout} {tag}"
        if layout == "f32":
            assert np.array_equal(got_x, chains.astype(np.float32)), f"chains f32 {tag}"
        else:
            assert np.array_equal(got_x, go.pack_words(chains)), f"chains packed {tag}"


# ---- merge ----
def check_merge(temp_max, temp_info, now_res, now_info, replace_worst=True, tag=""):
    """temp_info / now_info: numpy uint64 [ceil(M / 64), N] (bits past M are carried along untouched)."""
    M, N = temp_max.shape[0], temp_info.shape[1]
    tiles = (M + 63) // 64
    w_res, w_info, w_temp, w_vals, w_idx = go.merge(temp_max, temp_info, now_res, now_info, replace_worst)
    g = Guard()
    d_res = g.out((M,), torch.float32, fill=dev(now_res))
    d_info = g.out((tiles, N), torch.int64, fill=dev(now_info))
    d_temp = g.out((tiles, N), torch.int64, fill=dev(temp_info))
    mask = g.out((tiles,), torch.int64)
    k = 1 if replace_worst else 2
    bv, bi = g.out((k,), torch.float32), g.out((k,), torch.int64)
    _t.mcpg_merge_best(dev(temp_max), d_temp, d_res, d_info, M, mask, bv, bi, replace_worst)
    got = host(d_res), host(d_info), host(d_temp), host(bv), host(bi).view(np.int64)
    g.check(tag)
    assert np.array_equal(got[4], w_idx), f"merge index {tag}: {got[4]} != {w_idx}"
    assert same_f32(got[3], w_vals), f"merge value {tag}: {got[3]} != {w_vals}"
    assert same_f32(got[0], w_res), f"merge incumbents {tag}: {np.nonzero(got[0].view(np.uint32) != w_res.view(np.uint32))[0][:8]}"
    assert np.array_equal(got[1], w_info), f"merge now_info {tag}"
    assert np.array_equal(got[2], w_temp), f"merge temp_info {tag}"


# ---- bit sums ----
def run_bit_sums(d_words, C, value, tag=""):
    g = Guard()
    A = g.out((d_words.shape[1],), torch.float32, fill=0.0)
    _t.mcpg_value_bit_sums(d_words, C, dev(np.asarray(value, np.float32)), A)
    got = host(A)
    g.check(tag)
    return got


def assert_bit_sums(got, value, exact, absum, C, tag=""):
    """got float32 [N] against the oracle's float64 sums.  Values that are all integers or halves of magnitude <= 1024: every
    partial sum is an exact float32 in any order, so the result is compared exactly (the sign of zero aside).  Otherwise: the
    worst-case bound of summing C float32 terms in any order, C 2^-24 sum_c |value_c| s_nc.  Non-finite values: NaN exactly
    where the oracle's sum is NaN, +-inf exactly where it is +-inf, and the rule above elsewhere."""
    value = np.asarray(value, np.float32)
    fin = np.isfinite(exact)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), f"bit sums NaN set {tag}"
    assert np.array_equal(got[~fin & ~np.isnan(exact)], exact[~fin & ~np.isnan(exact)].astype(np.float32)), f"bit sums inf set {tag}"
    v = value[np.isfinite(value)]
    if np.array_equal(v * 2, np.rint(v * 2)) and np.abs(v).max(initial=0) <= 1024:
        bad = np.nonzero(got[fin] != exact[fin].astype(np.float32))[0]
        assert bad.size == 0, f"bit sums {tag}: {bad.size} nodes differ, first {bad[:5]}"
    else:
        err = np.abs(got[fin].astype(np.float64) - exact[fin])
        bound = C * 2.0 ** -24 * absum[fin]
        assert np.all(err <= bound), f"bit sums {tag}: error {err.max():.3e} at node {int(err.argmax())} over its bound {bound[err.argmax()]:.3e}"


def check_bit_sums(words, C, values, tag=""):
    """words numpy uint64 [tiles, N]; values: a list of float32 [C] vectors, all held to one pass of the oracle."""
    vals = np.stack([np.asarray(v, np.float32) for v in values], axis=1)
    both = go.bit_sums_many(words, C, np.concatenate([vals.astype(np.float64), np.abs(vals.astype(np.float64))], axis=1))
    d_words = dev(words)
    K = vals.shape[1]
    for k in range(K):
        got = run_bit_sums(d_words, C, vals[:, k], tag)
        assert_bit_sums(got, vals[:, k], both[:, k], both[:, K + k], C, f"{tag} values {k}")
