"""Which kernel, grid, workgroup and LDS size every MaxCut tile entry point (K1, K6, K5, K2, K3, the local-search weights)
launches, over shapes on both sides of every launch-policy limit and under every policy knob.

    python tools/timing/maxcut_launch_trace.py run OUTDIR [JOBS] # one `rocprofv3 --kernel-trace` child per knob setting, JOBS at a time
    python tools/timing/maxcut_launch_trace.py parse OUTDIR    # OUTDIR/plans.json: one row per call
    python tools/timing/maxcut_launch_trace.py golden OUTDIR/plans.json tests/golden/maxcut_launch_plans.json [LDS_DIR]
    python tools/timing/maxcut_launch_trace.py diff A/plans.json B/plans.json

The rows of a build are the fixture of tests/test_maxcut_launch_plan.py (tests/golden/maxcut_launch_plans.json): run it on two
builds and `diff` says whether every launch stayed what it was.  A child drives the entry points through torch.ops.rlsolver_hip.*
with the knobs of its setting in RLS_<KNOB> variables (_abi.tuning_from_env), and writes the list of its calls; the kernel trace
of the same process, filtered to the kernels of those entry points, has one row per call that launched."""
import csv, ctypes as C, glob, json, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KLDS = 160 * 1024
ENTRIES = ("K1", "K6", "K5", "K2", "K3", "WS")
KERNELS = re.compile(r"\bk_(maxcut_obj|maxcut_propose_accept|maxcut_greedy_sweep|node_stats_|node_cutdeg|delta_all|ls_weights_elem)")
# knob setting -> (knobs, the entry points they reach).  "default" runs the whole shape list, the others the short one.
SETTINGS = {
    "default": ({}, ENTRIES),
    "tile32_0": ({"RLS_K1_TILE32": 0, "RLS_K5_TILE32": 0, "RLS_K6_TILE32": 0, "RLS_NS_TILE32": 0}, ENTRIES),
    "tile32_1": ({"RLS_K1_TILE32": 1, "RLS_K5_TILE32": 1, "RLS_K6_TILE32": 1, "RLS_NS_TILE32": 1}, ENTRIES),
    "narrow_0": ({"RLS_NARROW_TILE": 0}, ENTRIES),
    "narrow_2": ({"RLS_NARROW_TILE": 2}, ENTRIES),
    "narrow_3": ({"RLS_NARROW_TILE": 3}, ENTRIES),
    "sw2_ns4_pad": ({"RLS_SWEEP_WAVES": 2, "RLS_NS_WAVES": 4, "RLS_K1_LDS_KB": 96}, ("K1", "K5", "K2", "K3", "WS")),
    "sw4_rows0": ({"RLS_SWEEP_WAVES": 4, "RLS_NS_ROWS": 0}, ("K5", "K2", "K3")),
    "sw8_rows1": ({"RLS_SWEEP_WAVES": 8, "RLS_NS_ROWS": 1}, ("K5", "K2", "K3")),
    "sw16_park0": ({"RLS_SWEEP_WAVES": 16, "RLS_NS_PARK": 0}, ("K5", "WS")),
    "nolevels_laneenv": ({"RLS_SWEEP_NO_LEVELS": 1, "RLS_NODE_STATS_LANE_ENV": 1}, ("K5", "K2", "K3", "WS")),
    "unbatched_notile": ({"RLS_SWEEP_NO_LEVELS": 1, "RLS_SWEEP_UNBATCHED": 1, "RLS_NODE_STATS_LANE_ENV": 1, "RLS_NODE_STATS_NO_TILE": 1},
                         ("K5", "K2", "K3", "WS")),
    "sw16_unbatched": ({"RLS_SWEEP_NO_LEVELS": 1, "RLS_SWEEP_WAVES": 16, "RLS_NODE_STATS_MIN_B": 100}, ("K5", "K2", "K3", "WS")),
    "minb_big": ({"RLS_NODE_STATS_MIN_B": 1000000}, ("K2", "K3", "WS")),
}


def _groups(csr):
    """Groups of the level schedule (what DeviceGraph stores as num_sweep_groups), on the host."""
    import numpy as np
    from rlsolver_amd import _abi
    rp, col = np.ascontiguousarray(csr.rowptr, dtype=np.int32), np.ascontiguousarray(csr.col, dtype=np.int32)
    ng, tot = C.c_int64(0), C.c_int64(0)
    _abi.call("rls_graph_sweep_levels", rp.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), csr.num_nodes, None, 0, None, 0,
              C.byref(ng), C.byref(tot))
    return int(ng.value)


def _k5_last_fit(word_bytes, extra, guess):
    """Largest N, a multiple of 8, whose sweep tile -- (N + 2) words, the level table of ITS graph, `extra` bytes -- fits LDS."""
    from rlsolver_amd import graph
    fits = lambda n: ((n + 2) * word_bytes + 15) // 16 * 16 + ((_groups(graph.build_csr(graph.generate_gnm(n, n // 4, seed=1), num_nodes=n)) + 1) * 4 + 15) // 16 * 16 + extra <= KLDS
    lo, hi = guess // 8 - 512, guess // 8 + 512      # (bisection over multiples of 8: fits(8 lo), not fits(8 hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(8 * mid) else (lo, mid)
    n = 8 * lo
    return n


def cases(entries, full):
    """(entry, N, E, B, options): options among f32, bits (K6's mask), weighted, hub (a node of 300 neighbours)."""
    out = []
    add = lambda e, N, E, B, **o: out.append((e, N, E, B, o)) if e in entries else None
    # B around the num_cus crossovers, on rows of 16-byte multiples
    for N in (800, 2000, 3008, 10000) if full else (2000, 10000):
        for B in (64, 256, 4096, 1 << 14, 1 << 16) if full else (256, 1 << 14):
            for e in ENTRIES:
                if e in ("K2", "K3", "WS") and B * N > 1 << 28:
                    continue
                add(e, N, 5 * N, B)
    # rows of 8-byte-only, 4-byte-only and odd length; the other spin / mask forms; weights; a hub; the four plane classes
    for N in (2008, 2004, 2001, 10008) if full else (2001,):
        for e in ENTRIES:
            add(e, N, 4 * N, 4096)
    for N in (2000, 10000, 2001) if full else ():
        add("K1", N, 4 * N, 4096, f32=True)
        add("K6", N, 4 * N, 4096, bits=True)
        for e in ("K5", "K2", "K3", "WS"):
            add(e, N, 4 * N, 4096, weighted=True)
            add(e, N, 4 * N, 4096, hub=True)
    if full:
        for E in (4000, 60000, 1000000, 1100000):
            for e in ("K1", "K6", "K5"):
                add(e, 10000, E, 4096)
                add(e, 50000, E, 512)      # (narrow tiles: 12 planes count as 16)
    # N on both sides of every LDS limit (B past the narrow tiles' batches up to the half tile, small beyond)
    big = lambda N: 4112 if N <= 41000 else 1024
    k1 = (7680, 7688, 15872, 15880, 19968, 19976, 20224, 20232, 39936, 39944, 40448, 40456, 40450, 79864, 79872, 79866, 159736, 159744,
          163840, 163848) if full else (19976, 20232, 40456, 79872, 163848)
    for N in k1:
        add("K1", N, N // 4, big(N))
        add("K6", N, N // 4, big(N))
        if N > 40448:
            add("K6", N, N // 4, big(N), bits=True)
    add("K1", 40456, 10000, 512, f32=True)
    add("K1", 20225, 5000, 512)
    ns = (6144, 6152, 12032, 12040, 15864, 15872, 16384, 16392, 20480, 20488, 32768, 32776, 40960, 40968, 81912, 81920, 163832, 163840,
          163848) if full else (12040, 16392, 20488, 40968, 81920)
    for N in ns:
        for e in ("K2", "K3", "WS"):
            add(e, N, N // 4, 4112 if N <= 41000 else 256)
    for N in (16386, 20490, 40970) if full else ():      # (rows the fast loaders do not take)
        for e in ("K2", "K3", "WS"):
            add(e, N, N // 4, 512)
    if "K5" in entries:
        lim = [_k5_last_fit(8, 8 * 512 + 16384, 17800), _k5_last_fit(8, 8 * 512, 19800), _k5_last_fit(8, 4 * 512, 20060),
               _k5_last_fit(8, 2 * 512, 20190), _k5_last_fit(4, 8 * 512 + 16384, 35200), _k5_last_fit(4, 8 * 512, 39200),
               _k5_last_fit(4, 4 * 512, 39700), _k5_last_fit(4, 2 * 512, 39950), _k5_last_fit(2, 4096, 77000), _k5_last_fit(1, 4096, 153000)]
        for N in lim if full else lim[3::4]:
            for M in (N, N + 8):
                add("K5", M, M // 4, big(M))
                if full:
                    add("K5", M, M // 4, 256)
        add("K5", 163840, 40000, 256)
        add("K5", 163848, 40000, 256)
        add("K5", 163848, 40000, 256, weighted=True)
        add("K5", 20001, 5000, 512)
    return out


def child(name, outdir):
    import numpy as np
    import torch
    from rlsolver_amd import _abi, graph, ops
    knobs, entries = SETTINGS[name]
    assert _abi.tuning_from_env() == {k: v for k, v in knobs.items()}, "the setting's knobs are this process's RLS_* variables"
    dev = torch.device("cuda:0")
    graphs, calls = {}, []
    for entry, N, E, B, o in cases(entries, name == "default"):
        key = (N, E, bool(o.get("weighted")), bool(o.get("hub")))
        if key not in graphs:
            graphs.clear()      # (cases come grouped by graph: one resident at a time)
            g = np.asarray(graph.generate_gnm(N, E, seed=1), dtype=np.int64)
            if o.get("hub"):
                g = np.concatenate([g, np.asarray([(7, j, 1) for j in range(8, 308) if not (((g[:, 0] == 7) & (g[:, 1] == j)) | ((g[:, 1] == 7) & (g[:, 0] == j))).any()],
                                                  dtype=np.int64)])
            if o.get("weighted"):
                g[:, 2] = np.where(np.arange(len(g)) % 3 == 0, -1, 1)
            graphs[key] = ops.DeviceGraph(graph.build_csr(g, num_nodes=N, if_bidirectional=False), dev, use_weights=bool(o.get("weighted")))
        dg = graphs[key]
        xs = torch.randint(0, 2, (B, N), device=dev, dtype=torch.uint8).view(torch.bool)
        row = dict(entry=entry, N=N, B=B, E=dg.num_stored_edges, nnz=dg.nnz, G=dg.num_sweep_groups, max_degree=int(dg.csr.max_degree),
                   weighted=bool(o.get("weighted")), f32=bool(o.get("f32")), bits=bool(o.get("bits")), knobs=knobs, error=None)
        torch.cuda.synchronize()
        try:
            if entry == "K1":
                ops.maxcut_obj(dg, xs.float() if o.get("f32") else xs)
            elif entry == "K6":
                mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
                ops.maxcut_propose_accept(dg, xs, torch.zeros(((B + 63) // 64, N), device=dev, dtype=torch.int64) if o.get("bits") else mask, torch.zeros(B, dtype=torch.int64, device=dev))
            elif entry == "K5":
                ops.maxcut_greedy_sweep(dg, xs, torch.zeros(B, dtype=torch.int64, device=dev))
            elif entry == "K2":
                ops.maxcut_node_cutdeg(dg, xs)
            elif entry == "K3":
                ops.maxcut_delta_all(dg, xs)
            else:
                ops.maxcut_ls_weights(dg, xs, 2)
            torch.cuda.synchronize()
        except RuntimeError as e:      # a refused shape: nothing was launched
            row["error"] = str(e).splitlines()[0][:200]
        calls.append(row)
        del xs
    with open(os.path.join(outdir, "calls.json"), "w") as f:
        json.dump(calls, f)
    print(name, len(calls), "calls", flush=True)


def run(outdir, jobs=5):
    names = list(SETTINGS)
    for i in range(0, len(names), int(jobs)):      # `jobs` children at a time, each a process (and a trace) of its own
        procs = []
        for name in names[i:i + int(jobs)]:
            d = os.path.join(outdir, name)
            os.makedirs(d, exist_ok=True)
            env = {k: v for k, v in os.environ.items() if not k.startswith("RLS_")}
            env.update({k: str(v) for k, v in SETTINGS[name][0].items()})
            cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "trace", "--",
                   sys.executable, os.path.abspath(__file__), "child", name, d]
            procs.append((name, subprocess.Popen(cmd, env=env, stdout=open(os.path.join(d, "child.log"), "w"), stderr=subprocess.STDOUT)))
        failed = [(name, p.returncode) for name, p in procs if p.wait() != 0]
        print("done:", [name for name, _ in procs], flush=True)
        if failed:      # nothing more is started on the GPU after a failure
            sys.exit(f"exit status {failed}: see child.log")


def parse(outdir):
    rows = []
    for name in SETTINGS:
        d = os.path.join(outdir, name)
        calls = json.load(open(os.path.join(d, "calls.json")))
        (path,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        disp = [r for r in csv.DictReader(open(path)) if KERNELS.search(r["Kernel_Name"])]
        disp.sort(key=lambda r: int(r["Start_Timestamp"]))
        it = iter(disp)
        for c in calls:
            if c["error"] is None:
                r = next(it)
                wg = int(r["Workgroup_Size_X"])
                c.update(kernel=re.sub(r"^void |\(.*$| \[clone .*$", "", r["Kernel_Name"]).replace("rls::", ""), grid=int(r["Grid_Size_X"]) // wg, block=wg,
                         lds=int(r["LDS_Block_Size"]))
            c["setting"] = name
            rows.append(c)
        assert next(it, None) is None, f"{name}: more traced kernels than calls"
    with open(os.path.join(outdir, "plans.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print(len(rows), "rows ->", os.path.join(outdir, "plans.json"))


FIELDS = ("setting", "entry", "N", "B", "E", "nnz", "G", "max_degree", "weighted", "f32", "bits", "ws_bytes", "kernel", "grid", "block", "lds")


def golden(plans, out, lds_dir=None):
    """plans.json -> the compact fixture.  The kernel trace reports a kernel's STATIC LDS only (0 for all of these), so the dynamic LDS
    of every launch comes from `lds_dir`: the children run once more, without the profiler, on a build of the same commit whose
    hipLaunchKernelGGL in rls_maxcut.hip first appends "<kernel expression> <grid> <block> <lds>" to $RLS_LAUNCH_LOG
    (lds_dir/<setting>/launch.log); grid and block of the two recordings must agree row for row."""
    rows = json.load(open(plans))
    if lds_dir:
        logs = {n: iter([l.split() for l in open(os.path.join(lds_dir, n, "launch.log")) if not l.startswith("k_fill_minmax")]) for n in SETTINGS}
        for r in rows:
            if r["error"] is None:
                _, grid, block, lds = next(logs[r["setting"]])
                assert (int(grid), int(block)) == (r["grid"], r["block"]), (r, grid, block)
                r["lds"] = int(lds)
        assert all(next(it, None) is None for it in logs.values())
    for r in rows:
        r.setdefault("kernel", None), r.setdefault("grid", None), r.setdefault("block", None), r.setdefault("lds", None)
        r["ws_bytes"] = 1 if r["max_degree"] <= 127 else 2      # (ops.ls_weight_dtype at mult = 2)
    doc = {"note": "Launches of the six MaxCut tile entry points as `rocprofv3 --kernel-trace` reported them on an MI355X (256 CUs) for the "
                   "commit before csrc/rls_maxcut_plan.h existed; recorded with tools/timing/maxcut_launch_trace.py.  kernel = null: the call "
                   "returned RLS_EUNSUPPORTED and launched nothing.  The trace's LDS_Block_Size is the kernels' static LDS, 0 for every row; lds "
                   "is the dynamic LDS argument of the launch, logged by a build of that commit whose launch macro records it (exact bytes: "
                   "lds_granule 1).",
           "lds_granule": 1, "settings": {k: v[0] for k, v in SETTINGS.items()}, "fields": FIELDS,
           "kernels": sorted({r["kernel"] for r in rows if r["kernel"]})}      # (rows name setting and kernel by index; booleans as 0 / 1)
    names = list(SETTINGS)
    cell = lambda r, f: names.index(r[f]) if f == "setting" else (None if r[f] is None else doc["kernels"].index(r[f])) if f == "kernel" else \
        int(r[f]) if isinstance(r[f], bool) else r[f]
    doc["rows"] = [[cell(r, f) for f in FIELDS] for r in rows]
    with open(out, "w") as f:
        f.write(json.dumps({k: v for k, v in doc.items() if k != "rows"})[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in doc["rows"]) + "\n]}\n")
    print(len(rows), "rows,", os.path.getsize(out), "bytes ->", out)


def diff(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    bad = [(x, y) for x, y in zip(ra, rb) if x != y]
    for x, y in bad[:20]:
        print("-", x, "\n+", y)
    print(f"{len(ra)} vs {len(rb)} rows, {len(bad)} differ")
    sys.exit(1 if bad or len(ra) != len(rb) else 0)


if __name__ == "__main__":
    {"run": run, "parse": parse, "golden": golden, "diff": diff, "child": child}[sys.argv[1]](*sys.argv[2:])
