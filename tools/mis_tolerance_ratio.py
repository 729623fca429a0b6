#!/usr/bin/env python3
"""How far is tests/mis_oracle.py (numpy f32) from the reference's ISCO_MIS.step (torch f32, CPU) in units of the
tests/isco_tol.py tolerance?  Over the committed traces (tests/golden/isco_mis.npz) and over the shapes of the GPU oracle
tests (tests/mis_oracle.py: EDGE_CASES, the same graphs, samples and draws), with the reference imported like
tools/gen_golden.py does and its two torch.rand draws replaced by the recorded ones.  Prints the largest error / tolerance
of ll_x2y, ll_y2x and log_acc -- MEASURED_RATIO in tests/mis_oracle.py -- and how many envs the mask-exactness rule would
leave out for the oracle alone.

    PYTHONDONTWRITEBYTECODE=1 python tools/mis_tolerance_ratio.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)

import numpy as np
import torch as th

import rlsolver.envs.env_ISCO as E
from tests import mis_oracle as mo
from tests.isco_tol import RTOL, ll_atol

KEYS = ("ll_x2y", "ll_y2x", "log_acc")


def ratios(got, r, pl, decided=True):
    """error / tolerance per env and key, where the oracle says the env carries information"""
    ok = (r["remaining_mass"] >= 1e-6) & decided
    out = []
    for k in KEYS:
        err = np.abs(got[k].astype(np.float64) - r[k])
        tol = ll_atol(r["remaining_mass"], pl) + RTOL * np.abs(r[k])
        out.append(np.where(ok & np.isfinite(err), err / tol, 0.0).max())
    print("   ", " ".join(f"{k} {v:.3f}" for k, v in zip(KEYS, out)))
    return max(out)


def reference_step(s, x, pl, T, ug, ua):
    cap = {}
    o_prop, o_y2x, o_sel = type(s).proposal, type(s).ll_y2x, type(s).select_sample

    def w_prop(x, pl, T):
        r = o_prop(s, x, pl, T)
        cap["ll_x"], cap["ll_x2y"], cap["mask"] = r[0], r[2]["ll_x2y"], r[2]["selected_idx"]["selected_mask"]
        return r

    def w_y2x(tr, y, T):
        r = o_y2x(s, tr, y, T)
        cap["ll_y"], cap["ll_y2x"] = r
        return r

    def w_sel(la, x, y):
        cap["log_acc"] = la
        return o_sel(s, la, x, y)

    s.proposal, s.ll_y2x, s.select_sample = w_prop, w_y2x, w_sel
    seq = [th.from_numpy(ug), th.from_numpy(ua)]
    orig = th.rand
    th.rand = lambda *a, **k: seq.pop(0)
    try:
        y, energy, acc = s.step(th.from_numpy(x), th.from_numpy(pl), th.tensor(T))
    finally:
        th.rand = orig
    assert not seq
    got = {k: v.numpy() for k, v in cap.items()}
    got["y"], got["energy"] = y.numpy(), energy.numpy()
    return got


worst, envs, undecided = 0.0, 0, 0
z = np.load(os.path.join(ROOT, "tests", "golden", "isco_mis.npz"))
lam = float(z["lam"])
for gname in ("BA_100_ID0", "PL_20_ID0", "loader_13"):
    g = z[f"{gname}/graph"]
    for k in range(3):
        t = f"{gname}/step{k}"
        pl, T = z[f"{t}/path_length"], float(z[f"{t}/temperature"])
        r = mo.mis_step(z[f"{t}/x"], g[:, 0], g[:, 1], lam, pl, T, z[f"{t}/rand_gumbel"], z[f"{t}/rand_accept"])
        q = ratios({kk: z[f"{t}/{kk}"] for kk in KEYS}, r, pl)
        print(f"{t}: {q:.3f}")
        worst = max(worst, q)

E.DEVICE = th.device("cpu")
for n, m, B, pl_hi in mo.EDGE_CASES:
    eu, ev, x, draws = mo.edge_case(n, m, B, pl_hi)
    E.BATCH_SIZE = B
    s = E.ISCO_MIS({"num_nodes": n, "num_edges": len(eu), "edge_from": th.from_numpy(eu), "edge_to": th.from_numpy(ev)})
    for T, pl, ug, ua in draws:
        got = reference_step(s, x, pl, T, ug, ua)
        r = mo.mis_step(x, eu, ev, s.lam, pl, T, ug, ua)
        decided = mo.mask_is_decided(x, eu, ev, s.lam, pl, T, ug)
        assert np.array_equal(got["mask"].astype(np.uint8)[decided], r["mask"].astype(np.uint8)[decided])
        assert np.array_equal(got["energy"], r["energy"]), "energies are expected to agree bit for bit"
        sure = r["accept_margin"] > 2 * (ll_atol(r["remaining_mass"], pl) + RTOL * np.abs(r["log_acc"]))
        assert np.array_equal(got["y"][sure & decided], r["y"][sure & decided])
        q = ratios(got, r, pl, decided)
        print(f"n={n} m={m} B={B} T={T}: {q:.3f}   undecided masks {int((~decided).sum())} of {B}")
        worst, envs, undecided = max(worst, q), envs + B, undecided + int((~decided).sum())
        x = r["y"]
print(f"largest error / tolerance: {worst:.2f}   envs whose mask the rule leaves out: {undecided} of {envs}")
