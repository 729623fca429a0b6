"""Record every launch of the local-search entry points (csrc/rls_localsearch.hip) on the CPU: the file is compiled with the build's
flags behind shim.h, which turns hipLaunchKernelGGL into a recorder, and linked with main.cpp, which calls the entry points on dummy
pointers (no device: 256 CUs).  Writes the cases and what each launched or refused as JSON -- tests/golden/ls_launch_plans.json.gz is
this tool's output on the commit before csrc/rls_ls_plan.h existed; the same command on any later tree must reproduce it.

    python tools/ls_launch_record/record.py [--tree ROOT] [--out tests/golden/ls_launch_plans.json.gz]
    python tools/ls_launch_record/record.py --mcpg [--tree ROOT] --out FILE     # the three MCPG local-search launchers (csrc/rls_mcpg.hip):
                                                                                # no planner there, so nothing to pin -- compare two trees' files"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from rlsolver_amd import build as rb  # noqa: E402

# the largest N on the near side of every limit of the policy (256 CUs): two 4-wave fused tiles per CU, 8-wave fused, 4-wave fused,
# k_ls_propose with rd_std in LDS, the propose tile, the bare tile, rd_std in LDS for threshold / mask, the staged half-tile apply,
# the half tile, the narrow tile
LIMITS = (3172, 6348, 7268, 10580, 15872, 20224, 24576, 31744, 39936, 159740)
NS = sorted({800, 2000} | {L + d for L in LIMITS for d in (-8, -4, -2, -1, 0, 1, 2, 4, 8)})
BS = (1, 64, 256, 4096, 8192, 8256, 16384, 16448, 65536)
ES = (3000, 40000, 200000, 2000000, 1 << 24)      # 12 / 16 / 20 / 24 counter planes, none
FUSED, THRESHOLD, PROPOSE, ROUNDS = range(4)
FIELDS = ("entry", "N", "B", "ws_bytes", "E", "ws_pitch", "num_spin", "num_draws", "x_off", "noise_off", "scratch_mode", "scratch_off", "schedule",
          "weighted", "max_degree")


def case(entry, N, B=256, **kw):
    c = dict(entry=entry, N=N, B=B, ws_bytes=1, E=40000, ws_pitch=(N + 15) // 16 * 16, num_spin=5, num_draws=4 if entry == ROUNDS else 1, x_off=0,
             noise_off=0, scratch_mode=2, scratch_off=0, schedule=2, weighted=0, max_degree=8, knobs={})
    bad = set(kw) - set(c)
    assert not bad, bad
    c.update(kw)
    return c


def cases():
    out = []
    for N in NS:
        every = (FUSED, THRESHOLD, PROPOSE, ROUNDS)
        out += [case(e, N, B) for B in BS for e in (FUSED, THRESHOLD, ROUNDS)] + [case(PROPOSE, N, B) for B in (256, 65536)]
        out += [case(e, N, ws_bytes=2) for e in every]
        out += [case(FUSED, N, E=E) for E in ES if E != 40000] + [case(e, N, E=1 << 24) for e in (PROPOSE, ROUNDS)]
        out += [case(e, N, scratch_mode=m, scratch_off=o) for e in (THRESHOLD, PROPOSE, ROUNDS) for m, o in ((0, 0), (3, 0), (2, 8))]
        out += [case(ROUNDS, N, scratch_mode=1), case(ROUNDS, N, num_draws=1)]
        tiles = (1 << 25) // N      # four rounds' mask words of so many 64-env tiles: just under / just over 1 GiB
        out += [case(ROUNDS, N, 64 * tiles), case(ROUNDS, N, 64 * (tiles + 1))]
        out += [case(e, N, x_off=4) for e in (FUSED, PROPOSE, ROUNDS)] + [case(FUSED, N, noise_off=4)]
        out += [case(e, N, ws_pitch=(N + 15) // 16 * 16 + 4) for e in every] + [case(e, N, ws_pitch=0) for e in (FUSED, ROUNDS)]
        out += [case(FUSED, N, schedule=s) for s in (0, 1)]
        out += [case(FUSED, N, B, knobs={"LS_WAVES": w}) for w in (4, 8) for B in (64, 65536)]
        out += [case(e, N, knobs={"LS_SLICES": s}) for e in (THRESHOLD, ROUNDS) for s in (1, 3, 8)]
        out += [case(ROUNDS, N, knobs={"LS_PER_ROUND": 1})] + [case(ROUNDS, N, B, knobs={"LS_APPLY32": v}) for v, B in ((0, 256), (1, 256), (1, 65536))]
        out += [case(PROPOSE, N, 65536, knobs={"LS_SD_GLOBAL": 1}), case(ROUNDS, N, knobs={"NARROW_TILE": 0}), case(FUSED, N, knobs={"SWEEP_NO_LEVELS": 1})]
    out += [case(FUSED, N, **kw) for N in (800, 3172, 7272) for kw in (dict(weighted=1), dict(max_degree=512), dict(max_degree=511))]
    out += [case(e, 800, num_spin=s) for e in (FUSED, THRESHOLD) for s in (15, 16)] + [case(e, 12, num_spin=12) for e in (FUSED, THRESHOLD)]
    return out


def mcpg_cases():
    """entry (4 levels, 5 stream, 6 plain), N, C, spin_bytes, out_spin_bytes, E, weighted, max_degree, gauge_node, knobs: every in / out pair, every plane count,
    every forced wave count, both sides of every LDS limit (levels: N + groups; stream: (N + 2) * 8 + 24 KB; plain: N * 8 + N / 8)."""
    out = []
    for N in (800, 10000, 19440, 19448, 19456, 19464, 20444, 20448, 20452, 20456, 20464, 20480):
        for E in ES:
            out += [(4, N, C, si, so, E, 0, 8, -1, kn) for C in (64, 4096) for si in (0, 1, 4) for so in (0, 4) for kn in ({}, {"K7_WAVES": 4}, {"K7_WAVES": 16})]
            out += [(e, N, 4096, sb, 4, E, w, md, gn, {}) for e in (5, 6) for sb in (1, 4) for w in (0, 1) for md, gn in ((8, -1), (8, 5), (600, -1))]
    return out + [(4, 800, 4096, 0, 0, 40000, 1, 8, -1, {}), (4, 800, 4096, 0, 0, 40000, 0, 1024, -1, {}), (4, 1 << 20, 4096, 0, 0, 40000, 0, 8, -1, {})]


def build(tree, tmp, mcpg=False):
    csrc, inc = os.path.join(tree, "rlsolver_amd", "csrc"), os.path.join(tree, "include")
    obj, mobj, exe = (os.path.join(tmp, n) for n in ("ls.o", "main.o", "ls_record"))
    hipcc = rb._hipcc()
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    subprocess.run([hipcc] + rb._flags() + [f"-I{inc}", f"-I{csrc}", f"-I{HERE}", "-include", "shim.h", "-c", os.path.join(csrc, "rls_mcpg.hip" if mcpg else "rls_localsearch.hip"), "-o", obj],
                   check=True)
    subprocess.run([hipcc, "-O1", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__"] + (["-DRECORD_MCPG"] if mcpg else []) + [ f"-I{rocm_inc}", f"-I{inc}", f"-I{csrc}", f"-I{HERE}", "-c", os.path.join(HERE, "main.cpp"), "-o", mobj], check=True)
    subprocess.run([hipcc, obj, mobj, "-o", exe, "-rdynamic", "-ldl"], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the source tree whose rls_localsearch.hip is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ls_launch_plans.json.gz"),
                    help="a name ending in .gz is written gzipped (no time stamp: the same launches give the same bytes)")
    ap.add_argument("--mcpg", action="store_true", help="record the MCPG local-search launchers (rls_mcpg.hip) instead")
    a = ap.parse_args()
    if a.mcpg:
        cs = mcpg_cases()
        lines = "".join(" ".join(map(str, c[:-1])) + "".join(f" {k}={v}" for k, v in c[-1].items()) + "\n" for c in cs)
        with tempfile.TemporaryDirectory() as tmp:
            res = subprocess.run([build(os.path.abspath(a.tree), tmp, True)], input=lines, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(res) == len(cs), (len(res), len(cs))
        with open(a.out, "w") as f:
            f.write("".join(json.dumps({"case": c, **json.loads(r)}) + "\n" for c, r in zip(cs, res)))
        print(len(cs), "MCPG cases ->", a.out)
        return
    cs = cases()
    lines = "".join(" ".join(str(c[f]) for f in FIELDS) + "".join(f" {k}={v}" for k, v in c["knobs"].items()) + "\n" for c in cs)
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([build(os.path.abspath(a.tree), tmp)], input=lines, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(res) == len(cs), (len(res), len(cs))
    index = lambda table, v: table.setdefault(v, len(table))      # noqa: E731
    kernels, launches, errors, knobs, rows = {}, {}, {"": 0}, {"{}": 0}, []
    for c, r in zip(cs, map(json.loads, res)):
        ls = [index(launches, json.dumps([index(kernels, l[0])] + l[1:], separators=(",", ":"))) for l in r["l"]]
        rows.append([c[f] for f in FIELDS] + [index(knobs, json.dumps(c["knobs"])), r["sb"]] + r["q"] + [r["rc"], index(errors, r["err"]), ls])
    doc = {"note": "tools/ls_launch_record/record.py: every launch and refusal of the local-search entry points, recorded on the CPU (256 CUs)",
           "fields": list(FIELDS) + ["knobs", "scratch_bytes", "fused_supported", "rounds_supported", "ls_scratch_bytes", "ls_slices", "rc", "error", "launches"],
           "launch_fields": ["kernel", "grid_x", "grid_y", "grid_z", "block", "lds", "args"],
           "call": {"seed": 7, "env_offset": 3, "first_draw": 2, "num_iters": 8, "first_draw_proposes": 1, "compute_obj": 1, "halve": 1},      # main.cpp
           "knobs": [json.loads(k) for k in knobs], "kernels": list(kernels), "errors": list(errors)}
    with open(a.out, "wb") as raw, (gzip.GzipFile("", "wb", 9, raw, mtime=0) if a.out.endswith(".gz") else raw) as f:
        f.write((json.dumps(doc, indent=0)[:-2] + ',\n"launch_table": [\n' + ",\n".join(launches) + '\n],\n"rows": [\n' +
                ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n").encode())
    print(len(rows), "cases,", len(launches), "distinct launches,", len(kernels), "kernels,", len(errors) - 1, "refusal texts ->", a.out)


if __name__ == "__main__":
    main()
