#!/usr/bin/env python3
"""The reference's maximum-independent-set sampler loop -- rlsolver/methods/ISCO/main_ISCO_MIS.py:19-42 -- on the drop-in
ISCO_MIS: Poisson path lengths clamped to [1, N], their mean `mu` adapted towards an acceptance of 0.574, a linear
temperature schedule from init_temperature to final_temperature.  The graph is a generated Barabasi-Albert graph (the
reference's default instance is BA_100_ID0); every step is one kernel (rls_isco_mis_step).

    python examples/isco_mis.py                        # BA-100, 2 chains (the reference's BATCH_SIZE), 20 000 steps
    python examples/isco_mis.py --batch-size 4096 --nodes 1000 --chain-length 5000

Prints the best energy seen and, for the best sample of the last step, the size of the set and the number of violated edges."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--ba-m", type=int, default=4, help="edges per new node of the Barabasi-Albert graph")
    ap.add_argument("--chain-length", type=int, default=20000)
    ap.add_argument("--lam", type=float, default=1.001)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.envs.env_ISCO import ISCO_MIS
    from rlsolver_amd.graph import generate_ba

    dev = torch.device("cuda:0")
    g = np.asarray(generate_ba(a.nodes, a.ba_m, a.seed), dtype=np.int64)
    params_dict = {"num_nodes": a.nodes, "num_edges": len(g), "edge_from": torch.from_numpy(g[:, 0].copy()).to(dev),
                   "edge_to": torch.from_numpy(g[:, 1].copy()).to(dev)}
    torch.manual_seed(a.seed)
    sampler = ISCO_MIS(params_dict, batch_size=a.batch_size, device=dev, chain_length=a.chain_length, lam=a.lam)
    sample = sampler.random_gen_init_sample(params_dict)
    mu = torch.ones(a.batch_size, device=dev, dtype=torch.float) * 10
    energy = torch.tensor(0, device=dev, dtype=torch.float)
    start_time = time.time()
    for step in range(sampler.chain_length):
        path_length = torch.clamp(torch.poisson(mu), min=1, max=sampler.max_num_nodes).long()
        temperature = sampler.init_temperature - step / sampler.chain_length * (sampler.init_temperature - sampler.final_temperature)
        sample, new_energy, acc = sampler.step(sample, path_length, temperature)
        mu = torch.clamp((mu + 0.01 * (acc - 0.574)), min=1.0, max=float(sampler.max_num_nodes))
        energy = torch.max(energy, torch.max(new_energy, dim=0)[0])
    # new_energy is the energy of the last PROPOSALS (as in the reference); the samples kept are scored here
    final = sampler.model(sample, 1.0)
    obj, obj_index = torch.max(final, dim=0)
    result = sample[obj_index]
    violated = int((result[params_dict["edge_from"]] * result[params_dict["edge_to"]]).sum())
    print(f"best energy {float(energy):.3f}   best sample: energy {float(obj):.3f}, set size {int(result.sum())}, "
          f"violated edges {violated}   ({a.chain_length} steps x {a.batch_size} chains on BA-{a.nodes}: "
          f"{time.time() - start_time:.1f} s)")
    return 0 if violated == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
