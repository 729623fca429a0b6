"""rls_pisco_product alone, for a counter pass (tools/sweeps/pmc_passes.sh <outdir> tools/sweeps/pisco_product_one.py [n] [B]):
five launches on a full-density unit-weight matrix; read with pmc_show.py <outdir> k_pisco_product."""
import sys
import numpy as np, torch
from rlsolver_amd import ops
n, B = (int(sys.argv[1]) if len(sys.argv) > 1 else 2000), (int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
dev = torch.device("cuda:0")
rng = np.random.RandomState(n)
U = np.triu(rng.rand(n, n) < 1.0, 1)
A = torch.from_numpy((U | U.T).astype(np.float16)).to(dev)
x = torch.from_numpy((rng.rand(B, n) < 0.5).astype(np.float16)).to(dev)
out = torch.empty((B, n), dtype=torch.float32, device=dev)
for _ in range(5):
    ops.pisco_product(A, x, out)
torch.cuda.synchronize()
