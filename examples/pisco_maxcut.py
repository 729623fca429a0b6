#!/usr/bin/env python3
"""The reference's dense, weighted MaxCut sampler loop -- rlsolver/methods/ISCO/main_PISCO_maxcut.py:19-44 -- on the drop-in
PISCO_maxcut: Poisson path lengths clamped to [1, n], their mean `mu` adapted towards an acceptance of 0.574, a linear
temperature schedule.  The graph is a generated +-1-weighted G(n, m) (a spin-glass instance, which the unit-weight ISCO_maxcut
cannot sample) or a Gset-style file; every step is one f16 matrix-core product plus one kernel (rls_pisco_step).

    python examples/pisco_maxcut.py                        # 100 nodes, 400 edges, 1 chain (the reference's BATCH_SIZE), 2000 steps
    python examples/pisco_maxcut.py --batch-size 4096 --nodes 2000 --edges 19990 --chain-length 500
    python examples/pisco_maxcut.py --file graph.txt --unit-weights

One departure from the reference's loop: it records the energy the step returns, which is the PROPOSAL's, beside the samples
kept; here the kept samples are scored by a second product per step (`tensor_core_energy`), so that the best energy belongs to
the best sample.  `best_sample` starts with `num_nodes` entries as there; `record` returns it at the samples' padded width.

Prints the sampler's own number for the best sample kept (0.25 * sum(A) + best energy; for unit weights the reference's
`0.5 * num_edges + best`) beside the weighted cut of that sample recomputed from the flip gains of the CSR kernels."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--edges", type=int, default=400)
    ap.add_argument("--file", default=None, help="Gset-style file read by load_data (methods/ISCO/util_maxcut.py)")
    ap.add_argument("--unit-weights", action="store_true", help="generated graph with weights 1 instead of +-1")
    ap.add_argument("--chain-length", type=int, default=2000)
    ap.add_argument("--full-precision", action="store_true", help="half_rounding=False: f32 energies instead of the reference's f16")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from rlsolver_amd import ops
    from rlsolver_amd.envs.env_ISCO import PISCO_maxcut
    from rlsolver_amd.envs.env_PISCO_maxcut import load_data, record
    from rlsolver_amd.graph import build_csr, generate_gnm

    dev = torch.device("cuda:0")
    if a.file:
        params_dict = load_data(a.file, dev)
    else:
        g = np.asarray(generate_gnm(a.nodes, a.edges, a.seed), dtype=np.int64)
        w = np.ones(len(g), np.int64) if a.unit_weights else np.random.RandomState(a.seed).choice([-1, 1], size=len(g))
        Np = (a.nodes + 7) // 8 * 8
        A = np.zeros((Np, Np), np.float16)
        A[g[:, 0], g[:, 1]] = A[g[:, 1], g[:, 0]] = w
        params_dict = {"num_nodes": a.nodes, "num_edges": len(g), "edge_from": torch.from_numpy(g[:, 0].copy()).to(dev),
                       "edge_to": torch.from_numpy(g[:, 1].copy()).to(dev), "adj_matrix": torch.from_numpy(A).to(dev)}
    torch.manual_seed(a.seed)
    sampler = PISCO_maxcut(params_dict, batch_size=a.batch_size, device=dev, chain_length=a.chain_length,
                           half_rounding=not a.full_precision)
    n, Np = sampler.max_num_nodes, sampler.padded_num_nodes
    sample = F.pad(sampler.random_gen_init_sample(), (0, Np - n), mode="constant", value=0).contiguous()
    mu = torch.ones(a.batch_size, device=dev, dtype=torch.float) * 10
    best_energy = torch.tensor(-float("inf"), device=dev, dtype=torch.float)
    best_sample = torch.zeros(n, device=dev, dtype=torch.float16)          # main_PISCO_maxcut.py:28
    start_time = time.time()
    for step in range(sampler.chain_length):
        path_length = torch.clamp(torch.poisson(mu), min=1, max=n).long()
        temperature = sampler.init_temperature - step / sampler.chain_length * (sampler.init_temperature - sampler.final_temperature)
        sample, new_energy, acc = sampler.step(sample, path_length, temperature)
        mu = torch.clamp((mu + 0.01 * (acc - 0.574)), min=1.0, max=float(n))
        # new_energy is the energy of the PROPOSALS (as in the reference, which records it beside the kept samples); the samples
        # kept are scored here, so that the best energy belongs to the best sample
        best_energy, best_sample = record(best_energy, best_sample, sampler.tensor_core_energy(sample, 1.0)[0], sample)
    seconds = time.time() - start_time
    Ah = sampler.adj_matrix[:n, :n].cpu().numpy().astype(np.int64)
    iu, ju = np.nonzero(np.triu(Ah))
    csr = build_csr((iu.astype(np.int64), ju.astype(np.int64), Ah[iu, ju]), num_nodes=n, if_bidirectional=False)
    graph = ops.DeviceGraph(csr, dev, use_weights=True)
    assert best_sample.shape[0] == Np
    xb = (best_sample[:n] > 0)[None, :].contiguous()
    total = int(np.triu(Ah).sum())
    cut = (2 * total - int(ops.maxcut_delta_all(graph, xb).sum())) // 4          # sum_i gain_i = delta' A delta
    own = 0.25 * float(sampler.adj_matrix.float().sum()) + float(best_energy)
    line = f"best sample: weighted cut {cut} (recomputed), sampler's own number {own:.1f}"
    if bool((sampler.adj_matrix >= 0).all()) and bool((sampler.adj_matrix <= 1).all()):
        line += f", 0.5 * num_edges + best = {0.5 * len(iu) + float(best_energy):.1f}, cut edges {int(ops.maxcut_obj(graph, xb)[0])}"
    print(f"{line}   ({a.chain_length} steps x {a.batch_size} chains on {n} nodes, {len(iu)} edges: {seconds:.1f} s)")
    # the two numbers agree exactly unless f16 could not hold sum_k r_k delta_k = -4 * energy (half_rounding, from 2048 on)
    exact = not sampler.half_rounding or abs(4.0 * float(best_energy)) < 2048
    return 0 if own == cut or not exact else 1


if __name__ == "__main__":
    sys.exit(main())
