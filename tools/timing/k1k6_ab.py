"""K1 and K6 (byte mask, 1 % proposals) at the judged shapes -- for A/B builds (e.g. RLS_EXTRA_CFLAGS=-DRLS_TILE_CONTIG).
    python tools/timing/k1k6_ab.py [tag]
    python tools/timing/k1k6_ab.py host [tag]     # host cost of a launch: wall us per call of the six MaxCut tile entry points on a
                                                  # launch-bound shape (N = 800, 64 envs), back-to-back calls, one sync at the end"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from rlsolver_amd import _abi, graph, ops

dev = torch.device("cuda:0")
host = len(sys.argv) > 1 and sys.argv[1] == "host"
tag = sys.argv[1 + host] if len(sys.argv) > 1 + host else ""


def t_us(fn, n=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def host_us(fn, n=4000):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    dt = time.perf_counter() - t
    torch.cuda.synchronize()
    return dt / n * 1e6


if host:
    N, B = 800, 64
    dg = ops.DeviceGraph(graph.build_csr(graph.generate_gnm(N, 4694, seed=1), num_nodes=N, if_bidirectional=False), dev)
    xs = ops.rand_spins(B, N, 1, dev)
    obj, mask = ops.maxcut_obj(dg, xs), torch.zeros((B, N), device=dev, dtype=torch.bool)
    cd, dl = torch.empty((B, N), dtype=torch.int64, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev)
    ws, mm = torch.empty((B, N), dtype=torch.int8, device=dev), torch.empty((2, N), dtype=torch.int32, device=dev)
    t = torch.ops.rlsolver_hip      # the ops themselves: no Python wrapper, no allocation in the timed loop
    calls = (("K1", lambda: t.maxcut_obj(dg.handle, xs, obj)), ("K6", lambda: t.maxcut_propose_accept(dg.handle, xs, mask, obj)),
             ("K5", lambda: t.maxcut_greedy_sweep(dg.handle, xs, obj)), ("K2", lambda: t.maxcut_node_cutdeg(dg.handle, xs, cd)),
             ("K3", lambda: t.maxcut_delta_all(dg.handle, xs, dl)), ("weights", lambda: t.maxcut_ls_weights(dg.handle, xs, 2, ws, mm)))
    for rep in range(5):
        print(f"HOST {tag} rep {rep}: " + " ".join(f"{n} {host_us(f):.2f}" for n, f in calls), flush=True)
    sys.exit(0)

for name, N, E, B, gen in (("G22", 2000, 19990, 65536, "gnm"), ("G70", 10000, 9999, 131072, "gnm"), ("ER-2000", 2000, 9995, 65536, "gnm"),
                           ("BA-2000", 2000, 0, 65536, "ba"), ("G14", 800, 4694, 65536, "gnm"), ("N3008", 3008, 30000, 65536, "gnm")):
    g = graph.generate_ba(N, 4, seed=1) if gen == "ba" else graph.generate_gnm(N, E, seed=1)
    dg = ops.DeviceGraph(graph.build_csr(g, num_nodes=N, if_bidirectional=False), dev)
    xs = ops.rand_spins(B, N, 1, dev)
    obj = ops.maxcut_obj(dg, xs)
    k1 = t_us(lambda: ops.maxcut_obj(dg, xs))
    mask = (torch.rand((B, N), device=dev) < 0.004)
    o2 = obj.clone()
    k6 = t_us(lambda: ops.maxcut_propose_accept(dg, xs, mask, o2))
    ok = torch.equal(ops.maxcut_obj(dg, xs), o2)
    print(f"{tag} {name}: K1 {k1:.1f} us {B * (N + 8) / k1 / 8e6:.3f} | K6 byte {k6:.1f} us {B * (2 * N + 16) / k6 / 8e6:.3f} (2N+16){'' if ok else ' K6 PARITY BROKEN'}", flush=True)
