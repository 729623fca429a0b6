"""Differential fuzz of the glue that ends an MCPG round (rls_mcpg_pick_best, rls_mcpg_merge_best, rls_mcpg_value_bit_sums,
rls_mcpg_pack_chains, rls_mcpg_unpack_chains: thirteen kernels) against tests/glue_oracle.py, bit for bit, through the guarded
launches of tests/glue_checks.py (canary bytes around every output).  Each configuration draws one entry point and then its
axes: node counts at every form boundary +- 1 (bit sums 512 k, 2048, 12 288, 18 368; the unpack's 32 768-row sweep), chain
counts around a tile, a 256-chain span and a block, RLS_MCPG_SHIM off / 1 / 2 / 4 spans, a base 4 bytes off the 16-byte line,
every value class of the pack rules, integer / half / Gaussian / non-finite values, planted ties, NaN and +-inf in the pick and
in the incumbents of the merge.  `python tools/fuzz/fuzz_mcpg_glue.py [seconds] [seed]`."""
import sys, time
import numpy as np
sys.path.insert(0, ".")
from tests import glue_checks as gc
from tests import glue_oracle as go

KNOBS = [None, 0, 1, 0x11, 0x21, 0x31, 0x20]
EDGE_C = [1, 2, 3, 4, 60, 63, 64, 65, 68, 127, 128, 130, 252, 255, 256, 257, 260, 511, 512, 513, 577, 1024, 1028]


def around(rng, edges, lo=1):
    return max(lo, int(rng.choice(edges)) + int(rng.randint(-1, 2)))


def fuzz_bit_sums(rng, tag):
    N = around(rng, [1, 2, 64, 512, 1024, 2048, 4096, go.BITSUM_REG_MAX_N, go.BITSUM_LDS_MAX_N, 19000]) if rng.rand() < 0.7 \
        else int(rng.randint(1, 3000))
    C = int(rng.choice(EDGE_C[:12])) if rng.rand() < 0.8 else int(rng.randint(1, 700))
    if N < 200 and rng.rand() < 0.1:
        C = go.BITSUM_REG_GRID * 64 + int(rng.randint(1, 200))                   # the tile loop of the register form
    words = gc.random_words(rng, (C + 63) // 64, N)
    for n in rng.randint(0, N, size=3):
        words[:, n] = np.uint64(0) if rng.rand() < 0.5 else ~np.uint64(0)
    kind = rng.randint(4)
    value = [rng.randint(-1024, 1025, size=C).astype(np.float32), rng.randint(-2048, 2049, size=C).astype(np.float32) * np.float32(0.5),
             rng.randn(C).astype(np.float32), rng.randint(-9, 10, size=C).astype(np.float32)][kind]
    if kind == 3:
        for x in (np.inf, -np.inf, np.nan):
            if rng.rand() < 0.7:
                c = int(rng.randint(C))
                value[c] = x
                words[c >> 6] &= ~(np.uint64(1) << np.uint64(c & 63)) | ((rng.rand(N) < 0.3).astype(np.uint64) << np.uint64(c & 63))
    gc.check_bit_sums(words, C, [value], f"{tag} bit sums N={N} C={C} values={kind}")


def fuzz_pack(rng, tag):
    N = around(rng, [1, 16, 32, 64, 128, 1001]) if rng.rand() < 0.8 else int(rng.randint(1, 3000))
    C = int(rng.choice(EDGE_C)) if rng.rand() < 0.8 else int(rng.randint(1, 1100))
    kind = str(rng.choice(["f32", "f32", "u8", "bool"]))
    knob = KNOBS[rng.randint(len(KNOBS))]
    x = gc.draw_chains(rng, N, C, kind)
    if kind == "f32" and rng.rand() < 0.25:
        x = gc.off_line(x)
    gc.check_pack(x, knob, None, f"{tag} pack N={N} C={C} {kind} knob={knob}")


def fuzz_unpack(rng, tag):
    N = around(rng, [1, 2, 64, 1001, go.UNPACK_SWEEP_ROWS, 2 * go.UNPACK_SWEEP_ROWS]) if rng.rand() < 0.7 else int(rng.randint(1, 3000))
    C = int(rng.choice([1, 3, 4, 8, 60, 64, 68])) if N > 3000 else int(rng.choice(EDGE_C)) if rng.rand() < 0.8 else int(rng.randint(1, 1100))
    knob = KNOBS[rng.randint(len(KNOBS))]
    lead = 4 if rng.rand() < 0.25 else 0
    words = gc.random_words(rng, (C + 63) // 64, N)
    xs = gc.check_unpack(words, C, knob, lead, None, f"{tag} unpack N={N} C={C} knob={knob} lead={lead}")
    back = gc.check_pack(xs, knob, None, f"{tag} pack(unpack) N={N} C={C} knob={knob} lead={lead}")
    assert np.array_equal(gc.host(back), go.mask_past(words, C)), f"{tag} pack(unpack) is not the identity"


def fuzz_pick(rng, tag):
    M = around(rng, [1, 64, 128, 192]) if rng.rand() < 0.8 else int(rng.randint(1, 300))
    N = around(rng, [1, 256, 512, 1001]) if rng.rand() < 0.8 else int(rng.randint(1, 1500))
    R = int(rng.choice([1, 2, 3, 7, 8, 9, 16, 17, 25]))
    num_edges = int(rng.choice([0, 1, 4999, 20000, 2 ** 24 + 1]))
    expected = gc.plant_expected(rng, M, R, int(rng.randint(6)))
    if rng.rand() < 0.3:
        expected = np.rint(expected)                                             # integer cuts: many ties
    bits = rng.randint(0, 2, size=(N, M * R)).astype(bool)
    gc.check_pick(bits, expected, M, R, num_edges, f"{tag} pick M={M} N={N} R={R} E={num_edges}")


def fuzz_merge(rng, tag):
    M = around(rng, [1, 64, 128, go.MERGE_THREADS, 2 * go.MERGE_THREADS]) if rng.rand() < 0.8 else int(rng.randint(1, 2600))
    N = int(rng.choice([1, 50, 77, 1023, 1024, 1025])) if rng.rand() < 0.8 else int(rng.randint(1, 1200))
    tiles = (M + 63) // 64
    span = int(rng.choice([1, 3, 40]))                                           # 1: every incumbent equal; 3: ties everywhere
    now_res = rng.randint(0, span, M).astype(np.float32)
    temp_max = rng.randint(0, span + 1, M).astype(np.float32)
    kind = rng.randint(6)
    if kind < 4:                                                                 # non-finite incumbents
        x = [np.nan, -np.inf, np.inf, np.nan][kind]
        share = float(rng.choice([1.0, 1.0, 0.5, 0.05]))
        now_res = np.where(rng.rand(M) < share, x, now_res).astype(np.float32)
        if kind == 3:
            now_res = np.where(rng.rand(M) < 0.5, -np.inf, now_res).astype(np.float32)
        temp_max = np.where(rng.rand(M) < 0.7, np.nan, temp_max).astype(np.float32)
    gc.check_merge(temp_max, gc.random_words(rng, tiles, N), now_res, gc.random_words(rng, tiles, N), bool(rng.rand() < 0.6),
                   f"{tag} merge M={M} N={N} span={span} kind={kind}")


WHAT = [fuzz_bit_sums, fuzz_pack, fuzz_unpack, fuzz_pick, fuzz_merge]


def run(seconds, seed):
    rng = np.random.RandomState(seed)
    t_end = time.time() + seconds
    it = 0
    while time.time() < t_end:
        f = WHAT[rng.randint(len(WHAT))]
        tag = f"it={it}"
        if "-v" in sys.argv:
            print(tag, f.__name__, flush=True)
        f(rng, tag)
        it += 1
    print(f"fuzz_mcpg_glue: {it} random configurations, no mismatch")


if __name__ == "__main__":
    run(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
