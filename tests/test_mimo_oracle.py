"""MIMO detection family, host side (no GPU): the numpy oracle against the fixture recorded from the reference, the loaders against
what the reference's loaders returned, the margin condition under which the GPU comparison may leave chains out, integer exactness
and ties, the reference's signatures, the driver's table and vote."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import mimo_oracle as orc
from oracle import oracle_np as onp

CASES = list(orc.fixture_cases())
GOLD_API = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_surface.npz")


def mm():
    from rlsolver_amd.methods import MCPG_mimo
    return MCPG_mimo


def test_fixture_covers_the_recipe():
    assert sorted(c["case"] for c in CASES) == ["int_24/ls1", "int_24/ls3", "real_24/ls1", "real_24/ls3"]
    for c in CASES:
        assert c["n"] == 24 and c["M"] == 6 and c["R"] == 4 and c["raw"].shape == (24, 24)
        if c["integer"]:
            assert np.array_equal(c["Sigma"], np.round(c["Sigma"])) and np.array_equal(c["Diag"], np.round(c["Diag"]))
            assert c["sca"] == round(c["sca"])


@pytest.mark.parametrize("c", CASES, ids=[c["case"] for c in CASES])
def test_oracle_equals_fixture(c):
    raw = onp.metro_sampling(c["probs"], c["start"], c["change_times"], c["index"], c["u"])
    raw = raw[0] if isinstance(raw, tuple) else raw
    assert np.array_equal(np.asarray(raw).astype(np.uint8), c["raw"])
    o = orc.sampler(c["Sigma"], c["Diag"], c["sca"], c["raw"], c["num_ls"], c["M"])
    assert np.array_equal(o["best"], c["best"])
    C = c["M"] * c["R"]
    tol = 2 * C * 2.0 ** -24 * float(np.abs(o["expected"]).max())       # the two means' and sums' rounding
    if c["integer"]:
        assert o["max_res"].dtype == np.float32 and np.array_equal(o["max_res"].view(np.uint32), c["max_res"].view(np.uint32))
    else:
        assert o["safe"].all()                                            # the generator picked the seed so: the fixture is unambiguous
        assert np.abs(o["max_res"].astype(np.float64) - c["max_res"]).max() <= tol
    assert np.abs(o["value"].astype(np.float64) - c["value"]).max() <= tol


def test_first_sweep_counts_unvisited_variables_twice():
    """num_ls = 1 on the fixture differs from a model whose chains are +-1 from the start: the +-2 rule is pinned."""
    differ = 0
    for c in CASES:
        if c["num_ls"] != 1:
            continue
        two = orc.local_search(c["Sigma"], c["Diag"], c["raw"], 1)
        one = orc.local_search(c["Sigma"], c["Diag"], c["raw"], 1, start_scale=1.0)
        assert np.array_equal(((two["info"] + 1) / 2).astype(np.uint8)[:, orc.first_min(two["expected"].astype(np.float32), c["M"])], c["best"])
        differ += int((two["info"] != one["info"]).any())
    assert differ == 2


# ------------------------------------------------------------------------------ loaders
def _gold():
    return np.load(orc.GOLDEN)


def _inst(z):
    return dict(K=int(z["loader/inst/K"]), SNR=float(z["loader/inst/SNR"]), H=z["loader/inst/H"], X=z["loader/inst/X"], v=z["loader/inst/v"])


def _check_loader(data, z, tag, sigma_rel):
    """Sigma / Diag are float32 here, float64 (mimo5) or a float32 product (mimo3) in the reference: they agree within float32
    rounding of the entries' own products, sum_k |H_ki| |H_kj| (for Diag: of |Y|^T |H|, bounded by the same scale)."""
    S, D = z[f"loader/{tag}/Sigma"].astype(np.float64), z[f"loader/{tag}/Diag"].astype(np.float64)
    H = np.abs(z["loader/inst/H"])
    scale = (H.T @ H).max()
    assert isinstance(data, list) and len(data) == 5 and data[0].dtype == torch.float32 and data[1].dtype == torch.float32
    assert data.num_nodes == S.shape[0] and tuple(data[0].shape) == S.shape
    assert np.abs(data[0].numpy().astype(np.float64) - S).max() <= sigma_rel * scale
    assert (np.diag(data[0].numpy()) == 0).all()
    assert np.abs(data[1].numpy().astype(np.float64) - D).max() <= sigma_rel * np.abs(D).max()
    assert np.array_equal(data[2].numpy(), z[f"loader/{tag}/X"])
    assert abs(float(data[3]) - float(z[f"loader/{tag}/sca"])) <= sigma_rel * abs(float(z[f"loader/{tag}/sca"]))
    assert abs(float(data[4]) - float(z[f"loader/{tag}/noise"])) <= 1e-12 * float(z[f"loader/{tag}/noise"])


def test_read_data_mimo3_equals_the_reference(tmp_path):
    z = _gold()
    p = tmp_path / "inst.txt"
    p.write_text(str(z["loader/text"]))
    rows = z["loader/inst/H"].shape[0]
    # the reference multiplies H in float32 here: rows products of relative error 2^-24 each, + the final cast
    _check_loader(mm().read_data_mimo3(str(p), 10, 0, "cpu"), z, "mimo3", (rows + 2) * 2.0 ** -24)
    p2 = tmp_path / "again.txt"
    mm().write_mimo3(str(p2), _inst(z))
    assert p2.read_text() == str(z["loader/text"])
    _check_loader(mm().read_data_mimo3(str(p2), 10, 0, "cpu"), z, "mimo3", (rows + 2) * 2.0 ** -24)


def test_read_data_mimo5_equals_the_reference(tmp_path):
    z = _gold()
    K, N, SNR, X_num, r_seed = (int(v) for v in z["loader/mimo5_args"])
    d = tmp_path / f"4QAM{N}_{K}"
    d.mkdir()
    mm().write_mimo5(str(d / f"4QAM{K}_{r_seed // X_num + 1}.npz"), _inst(z))
    data = mm().read_data_mimo5(K, N, SNR, X_num, r_seed, "cpu", data_dir=str(tmp_path))
    _check_loader(data, z, "mimo5", 2.0 ** -23)                          # float64 on both sides: only the cast to float32 remains
    # the noise scale comes from the ARGUMENTS: another SNR than the file's changes the noise
    other = mm().read_data_mimo5(K, N, SNR + 4, X_num, r_seed, "cpu", data_dir=str(tmp_path))
    assert abs(other[4] / data[4] - 10 ** (-4 / 20)) < 1e-12


def test_loaders_refuse_malformed_input(tmp_path):
    z = _gold()
    lines = str(z["loader/text"]).split("\n")
    h = lines.index("H")
    short = list(lines)
    short[h + 2] = ", ".join(short[h + 2].split(", ")[:-1])
    for bad, what in ((short, "one length"), ([ln for i, ln in enumerate(lines) if i not in (lines.index("v"), lines.index("v") + 1)], "v missing"),
                      (lines[:h], "missing")):
        p = tmp_path / "bad.txt"
        p.write_text("\n".join(bad))
        with pytest.raises(ValueError, match=what):
            mm().read_data_mimo3(str(p), 10, 0, "cpu")
    S = np.zeros((3, 4))
    with pytest.raises(ValueError, match="square"):
        mm().make_data(S, np.zeros(3), np.ones(3), 0.0, 0.0, "cpu")
    with pytest.raises(ValueError, match="Diag"):
        mm().make_data(np.zeros((3, 3)), np.zeros(4), np.ones(3), 0.0, 0.0, "cpu")
    with pytest.raises(ValueError, match="finite"):
        mm().make_data(np.full((3, 3), np.inf), np.zeros(3), np.ones(3), 0.0, 0.0, "cpu")
    with pytest.raises(ValueError, match="covers 1 <= n <="):
        mm().make_data(np.zeros((40000, 40000), dtype=np.float32), np.zeros(40000), np.ones(40000), 0.0, 0.0, "cpu")


# ------------------------------------------------------------------------------ the margin condition of the GPU comparison
@pytest.mark.parametrize("n,num_ls", orc.REAL_SHAPES)
@pytest.mark.parametrize("snr", orc.REAL_SNRS)
def test_margin_condition_leaves_out_at_most_a_tenth(n, num_ls, snr):
    run = orc.real_run(n, snr, num_ls)
    share = 1.0 - run["safe"].mean()
    print(f"n={n} num_ls={num_ls} SNR={snr}: {100 * share:.2f} % of {orc.REAL_CHAINS} chains have a decision inside the bound")
    assert share <= 0.10


# ------------------------------------------------------------------------------ integer exactness, ties
def test_integer_instance_is_exact_in_float32_and_ties_give_minus_one():
    Sigma, Diag, _, x01 = orc.integer_case(96, 31, 512, even_diag=True)
    assert 2 * np.abs(Sigma).sum(axis=1).max() + np.abs(Diag).max() < 2 ** 24 and np.abs(Sigma).sum() + np.abs(Diag).sum() < 2 ** 24
    a = orc.local_search(Sigma, Diag, x01, 2, np.float64)
    b = orc.local_search(Sigma, Diag, x01, 2, np.float32)
    assert b["info"].dtype == np.float32 and np.array_equal(a["info"], b["info"])
    assert np.array_equal(a["expected"], b["expected"].astype(np.float64))
    assert a["ties"] >= 1 and a["ties"] == b["ties"]
    # a tie resolved: r == thr gives -1 whatever the start (Sigma = 0, Diag = 0: every decision is the tie 0 < 0)
    t = orc.local_search(np.zeros((3, 3)), np.zeros(3), np.array([[0, 1], [1, 0], [1, 1]]), 1)
    assert t["ties"] == 6 and (t["info"] == -1).all()


# ------------------------------------------------------------------------------ the reference's signatures
@pytest.mark.parametrize("file,name", [("sampling.py", "mcpg_sampling_mimo"), ("dataloader.py", "read_data_mimo3"), ("dataloader.py", "read_data_mimo5")])
def test_reference_signature(file, name):
    surface = json.loads(str(np.load(GOLD_API)["surface"]))
    ref = surface["rlsolver/methods/MCPG/" + file][name]
    have = list(inspect.signature(getattr(mm(), name)).parameters)
    want = list(ref["args"])
    assert have[:len(want)] == want
    params = inspect.signature(getattr(mm(), name)).parameters
    assert all(params[p].default is inspect.Parameter.empty for p in want[:ref["required"]])
    assert all(params[p].default is not inspect.Parameter.empty for p in have[ref["required"]:])


# ------------------------------------------------------------------------------ the driver's table and vote
def test_vote_counts_the_best_chain_twice():
    res = torch.tensor([1.0, 5.0, 3.0, -2.0])
    info = torch.tensor([[1, 0, 1, 0],        # best (chain 1) says -, second (2) says +, third (0) says +: - - + + -> 0
                         [0, 1, 0, 0],        # best says +, the other two -: + + - - -> 0
                         [0, 1, 1, 0],        # + + + - -> +
                         [1, 0, 0, 1]], dtype=torch.float32)
    v2 = mm().mimo_vote(res, info, 2)          # best + {best, second}: the best chain's double count decides rows 0 and 1
    assert v2.tolist() == [-1.0, 1.0, 1.0, -1.0]
    v3 = mm().mimo_vote(res, info, 3)
    assert v3.tolist() == [0.0, 0.0, 1.0, -1.0]
    assert mm().mimo_vote(res, info, 150).tolist() == mm().mimo_vote(res, info, 4).tolist()
    assert mm().bit_error_rate(v2, torch.tensor([-1.0, 1.0, -1.0, -1.0])) == 0.25
    assert mm().bit_error_rate(np.array([1.0, 1.0]), np.array([1.0, 1.0])) == 0.0


def test_parameter_table():
    p = mm().mimo_parameters
    assert p(8, 800, 800) == (7, 3, 150) and p(2, 1000, 1000) == (2, 2, 150) and p(8, 1200, 1200) == (6, 4, 100)
    assert p(6, 1200, 1200) == (7, 3, 150) and p(12, 1000, 1000) == (3, 3, 150)
    assert p(8, 180, 180) == (4, 3, 150) and p(7, 800, 800) == (4, 3, 150) and p(8, 800, 1000) == (4, 3, 150)


def test_instances_are_seeded_and_integer_ones_give_integers():
    a, b = mm().mimo_instance(5, 6, 8, 3), mm().mimo_instance(5, 6, 8, 3)
    assert a["H"].shape == (12, 10) and a["X"].shape == (10,) and a["v"].shape == (12,) and set(np.unique(a["X"])) <= {-1.0, 1.0}
    assert all(np.array_equal(a[k], b[k]) for k in ("H", "X", "v")) and not np.array_equal(a["H"], mm().mimo_instance(5, 6, 8, 4)["H"])
    i = mm().mimo_instance(5, 6, 8, 3, integer=True)
    assert np.abs(i["H"]).max() <= 3 and np.abs(i["v"]).max() <= 2
    S, D, X, sca, noise = mm().instance_arrays(i["H"], i["X"], i["v"], i["K"], i["SNR"], 1.0)
    assert np.array_equal(S, np.round(S)) and np.array_equal(D, np.round(D)) and sca == round(sca) and (np.diag(S) == 0).all()
    d = mm().data_from_instance(i, "cpu", 1.0)
    assert d.num_edges == 0 and d.value_scale == 0.5 and d.fractional_values and d.num_nodes == 10
    assert d.objective(3.0) == 3.0 - sca
