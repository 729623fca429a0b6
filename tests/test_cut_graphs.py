"""CPU side of tests/test_gpu_cut_counter.py: the bipartite circulant family is what that file takes it for (distinct edges, every
stored edge cut by the parity state, the degrees every consumer's limit is checked against), its fast count is the oracle's, and
the launch planner picks the counter planes the GPU tests expect on both sides of each plane limit.  No GPU."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from rlsolver_amd.graph import build_csr
from tests import cut_graphs as cg
from tests.test_maxcut_launch_plan import (K1, K5, K6, NARROW8, NARROW16, RLS_EUNSUPPORTED, SW_BATCHED, SW_FAST, SW_GENERIC, TILE32, TILE64,
                                           UNSUPPORTED, graph, knobs, plan)  # noqa: F401  (knobs: a fixture)
from tests.test_gpu_graph_forms import FORMS

FORM_OF = {"tile64": TILE64, "tile32": TILE32, "narrow16": NARROW16, "narrow8": NARROW8}


@pytest.mark.parametrize("size", list(cg.SIZES) + list(cg.SIZES_EXTRA))
def test_family_is_bipartite_with_distinct_edges_and_the_listed_degrees(size):
    N, k = {**cg.SIZES, **cg.SIZES_EXTRA}[size]
    assert N % 64 == 0
    u, v, w = cg.bipartite_circulant(N, k, N * k)
    assert len(u) == N * k and u.min() == 0 and max(u.max(), v.max()) == N - 1 and np.all(w == 1)
    assert np.all(np.diff(u) >= 0)                                        # i-major
    assert np.all((u ^ v) & 1)                                            # even -- odd: bipartite
    pairs = np.minimum(u, v) * N + np.maximum(u, v)
    assert np.unique(pairs).size == N * k                                 # distinct as unordered pairs: none repeated, none reversed
    deg = np.bincount(np.concatenate([u, v]), minlength=N)
    assert deg.max() == deg.min() == 2 * k
    if size in cg.MAX_DEGREE:
        assert cg.MAX_DEGREE[size] == 2 * k
    # the consumers' limits: K5's level schedule < 256, the ring forms < 512, the MCPG levels < 1024
    assert 2 * k < 256
    for bidir in (False, True):
        assert build_csr((u, v, w), num_nodes=N, if_bidirectional=bidir).max_degree == 2 * k


def test_a_prefix_is_a_prefix():
    u, v, _ = cg.bipartite_circulant(256, 17, 4352)
    for E in (1, 63, 1025, 4097):
        a, b, _ = cg.bipartite_circulant(256, 17, E)
        assert np.array_equal(a, u[:E]) and np.array_equal(b, v[:E])
    for bad in ((255, 3, 10), (256, 65, 10), (256, 17, 0), (256, 17, 4353)):
        with pytest.raises(ValueError):
            cg.bipartite_circulant(*bad)


@pytest.mark.parametrize("c", cg.cases(), ids=cg.case_id)
def test_stored_edge_counts_and_the_parity_cut(c):
    size, stored, bidir = c
    N, u, v, w = cg.case_edges(c)
    csr = build_csr((u, v, w), num_nodes=N, if_bidirectional=bidir)
    assert csr.num_stored_edges == stored == (2 if bidir else 1) * len(u)
    assert csr.max_degree <= cg.MAX_DEGREE[size]
    xb = cg.states(N, 1, rows=5)
    cut = cg.stored_cut(xb, u, v, bidir)
    assert cut[0] == 0 and cut[1] == stored and cut[2] == stored          # the parity state and its complement cut every stored edge
    assert np.all(cut[3:] < stored) or stored < 8
    if size != "S24":                                                      # the fast count is the oracle's (its fancy index takes seconds at S24)
        g = np.stack([u, v, w], axis=1)
        su, sv = onp.stored_edges(g, bidir)
        assert np.array_equal(cut, (xb[:, su] ^ xb[:, sv]).sum(axis=1))
        assert np.array_equal(cg.obj_of(xb, u, v, bidir), onp.maxcut_obj(xb, g, bidir))


def test_the_edge_counts_sit_on_the_counter_edges():
    for lim, size in zip(cg.LIMITS, ("S12", "S16", "S24")):
        assert {lim - 1, lim, lim + 1} <= set(cg.UNI_STORED[size])
        assert {lim - 2, lim, lim + 2} <= set(cg.BIDIR_STORED[size])
        assert any(e % 1024 not in (0, 1, 2, 1022, 1023) for e in cg.BIDIR_STORED[size])      # one in the middle of a block
        assert all(e % 2 == 0 for e in cg.BIDIR_STORED[size])
    assert [e // 1024 for e in cg.UNI_STORED["S16"][:5]] == [7, 8, 15, 16, 17]                  # the ragged block's owner: nfull % W
    assert [e % 1024 == 0 for e in cg.UNI_STORED["S16"][:5]] == [False, True, False, True, True]
    assert [cg.planes(e) for e in (4095, 4096, 65535, 65536, (1 << 20) - 1, 1 << 20, (1 << 24) - 1, 1 << 24)] == [12, 16, 16, 20, 20, 24, 24, 0]


@pytest.mark.parametrize("form", list(FORM_OF))
@pytest.mark.parametrize("N", [256, 1024, 8448])
def test_planner_picks_the_planes_on_both_sides_of_every_limit(knobs, form, N):
    knobs(FORMS[form])
    narrow = form.startswith("narrow")
    for lim, below in zip(cg.LIMITS, (12, 16, 20)):
        for E, P in ((lim - 1, below), (lim, below + 4), (lim + 1, below + 4)):
            for what in (K1, K6, K5):
                for flags in (0, 1) if what == K1 else (0,):                 # (1: float32 rows)
                    p = plan(graph(N, E, max_degree=250), what, cg.B, flags)
                    assert (p.form, p.planes) == (FORM_OF[form], 16 if narrow and P == 12 else P), (form, N, E, what, flags, p.form, p.planes)
    # 2^24 stored edges and more: no counter takes them.  K1 and K6 refuse; K5 falls back to its stream forms, which add the accepted
    # gains to the caller's value and count nothing
    for E in ((1 << 24) - 1, 1 << 24, (1 << 24) + 1):
        for what in (K1, K6, K5):
            p = plan(graph(N, E, max_degree=250), what, cg.B)
            if E < (1 << 24):
                assert (p.form, p.planes) == (FORM_OF[form], 24), (form, N, E, what)
            elif what == K5:
                assert p.form in (SW_BATCHED, SW_FAST, SW_GENERIC) and p.planes == 0, (form, N, E, p.form)
            else:
                assert p.form == UNSUPPORTED and p.err == RLS_EUNSUPPORTED, (form, N, E, what, p.form)
