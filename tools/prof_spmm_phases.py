#!/usr/bin/env python3
"""Where the config-5 SpMM layer spends its time, phase by phase, and which block order the launch should walk.

The production launch (`spmm_rows_kernel`, d = 64) runs three kinds of work one after the other in grid order: the chunk
blocks of the long item rows (uniform gathers from the 256-MB user table), the user rows (Zipf gathers of item rows, mostly
L2 hits) and the short item rows (uniform gathers again).  Each phase is timed here ALONE as a launch of the production
library on a sub-graph that holds only its rows (the other rows of the sub-graph are empty, so their row blocks only read
rowptr):  chunks = item rows with the short ones emptied, users = the user rows, items_short = item rows with the long ones
emptied.  Next to them: the production launch with its multi-chunk rows finished inside the launch (tickets) and in a
second launch (tickets withheld), and the block orders of `MMREC_SPMM_ORDER` (variant builds of spmm.hip with
profiles/r07_spmm_block_order_rejected.patch applied: `git apply` it, `build`, revert), A/B alternated, every one checked bit
for bit against the production launch (profiles/r07_spmm_phases.log).

    python tools/prof_spmm_phases.py build              # order variants -> tools/probe_libs/ (no GPU needed; patched source)
    python tools/prof_spmm_phases.py time  [rounds]     # HIP-event times of phases, one/two-launch forms and orders
    python tools/prof_spmm_phases.py child              # a few launches of every phase (the workload of the passes below)
    python tools/prof_spmm_phases.py pmc   OUT_PREFIX   # rocprofv3: a --kernel-trace --stats pass, then one --pmc pass per
                                                        # counter set (FETCH_SIZE / WRITE_SIZE / TCC_HIT_sum TCC_MISS_sum)

Phases are told apart in the profiler output by grid size (the `grid` column printed by `child`)."""
import csv
import ctypes
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tools", "probe_libs")
ORDERS = (0, 1, 2, 3)
# one pass per set, as bench.py collects them: FETCH_SIZE with WRITE_SIZE in one pass exceeds what the hardware can collect
# at once (rocprofv3: "Request exceeds the capabilities of the hardware to collect")
COUNTER_SETS = (["FETCH_SIZE"], ["WRITE_SIZE"], ["TCC_HIT_sum", "TCC_MISS_sum"])


def lib_path(order):
    return os.path.join(OUT, "libspmm_order%d.so" % order)


def build():
    os.makedirs(OUT, exist_ok=True)
    csrc = os.path.join(ROOT, "mmrec_amd", "csrc")
    procs = []
    for o in ORDERS:
        procs.append(subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics",
                                       "-I" + os.path.join(ROOT, "include"), "-DMMREC_SPMM_ORDER=%d" % o,
                                       os.path.join(csrc, "spmm.hip"), os.path.join(csrc, "spmm_narrow.hip"), "-o", lib_path(o)]))
    assert all(p.wait() == 0 for p in procs)
    print("built", len(procs), "variants under", OUT)


def c5_graphs(dev):
    """The bench's config-5 graph (same generator, same device CSR build) and the three phase sub-graphs."""
    import numpy as np
    import torch
    from mmrec_amd import hip_ops, synth
    nu, ni, eu, ei = synth.shaped_edges("c5", seed=0)
    r, c, v = synth.sym_norm_coo(eu, ei, nu, ni)
    n = nu + ni
    g = hip_ops.CsrGraph.from_coo_device(torch.from_numpy(r.astype(np.int32)).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev),
                                         torch.from_numpy(v).to(dev), n, n, symmetric=True)
    rp = g.rowptr_host.astype(np.int64)

    def sub(r0, r1, keep_long=None):
        deg = np.diff(rp[r0:r1 + 1])
        keep = np.ones(deg.shape, bool) if keep_long is None else ((deg > g.long_row_threshold) == keep_long)
        nrp = np.concatenate([[0], np.cumsum(np.where(keep, deg, 0))]).astype(np.int32)
        m = torch.from_numpy(np.repeat(keep, deg)).to(dev)
        col = g.colidx[rp[r0]:rp[r1]][m].contiguous()
        val = g.vals[rp[r0]:rp[r1]][m].contiguous()
        return hip_ops.CsrGraph(torch.from_numpy(nrp).to(dev), col, val, r1 - r0, n, long_row_threshold=g.long_row_threshold,
                                rowptr_host=nrp)
    phases = {"chunks": sub(nu, n, True), "users": sub(0, nu), "items_short": sub(nu, n, False)}
    return g, phases


def grid_of(g):
    rpg = 1 if g.n_rows <= (1 << 18) else 4
    return ((g.n_rows + 16 * rpg - 1) // (16 * rpg) + g.n_chunks) * 256


def alg_bytes(g):
    """264 B per nonzero + 260 B per non-empty output row"""
    import numpy as np
    return 264 * g.nnz + 260 * int(np.count_nonzero(np.diff(g.rowptr_host)))


def describe(name, g):
    print("%-12s rows %8d nnz %9d long rows %6d chunks %6d grid %9d alg %.3f GB" %
          (name, g.n_rows, g.nnz, g.n_long, g.n_chunks, grid_of(g), alg_bytes(g) / 1e9), flush=True)


def variant_call(lib, g, x, y, tickets=True):
    from mmrec_amd import hip_ops
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = lib.mmrec_spmm_csr_f32(P(g.rowptr), P(g.colidx), P(g.vals), P(x), P(y), None, None, None, g.n_rows, 64, 1.0, 0.0, 1.0,
                                g.long_row_threshold, P(g.long_rows), P(g.long_chunk_ptr), g.n_long, g.n_chunks,
                                P(g.partials_for(64)), P(g.long_tickets) if tickets else None, hip_ops._stream())
    assert rc == 0, rc


def load_variant(order):
    lib = ctypes.CDLL(lib_path(order))
    lib.mmrec_spmm_csr_f32.restype = ctypes.c_int32
    lib.mmrec_spmm_csr_f32.argtypes = ([ctypes.c_void_p] * 8 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    return lib


def two_launch(g, fn):
    """fn() with the graph's tickets withheld: multi-chunk rows are finished by the second launch"""
    t, g.long_tickets = g.long_tickets, None
    try:
        fn()
    finally:
        g.long_tickets = t


def time_all(rounds):
    import statistics
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    g, phases = c5_graphs(dev)
    describe("full", g)
    for k, p in phases.items():
        describe(k, p)
    x = torch.rand(g.n_rows, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) - 0.5
    y = torch.empty_like(x)
    libs = {o: load_variant(o) for o in ORDERS if os.path.exists(lib_path(o))}
    cases = {"full one-launch": lambda: hip_ops.spmm_raw(g, x, Y=y),
             "full two-launch": lambda: two_launch(g, lambda: hip_ops.spmm_raw(g, x, Y=y))}
    for k, p in phases.items():
        cases["phase " + k] = (lambda p=p: hip_ops.spmm_raw(p, x, Y=y))
    for o, lib in libs.items():
        cases["order %d" % o] = (lambda lib=lib: variant_call(lib, g, x, y))

    # bits: every form and order against the production one-launch form
    hip_ops.spmm_raw(g, x, Y=y)
    ref = y.clone()
    for name in ["full two-launch"] + ["order %d" % o for o in libs]:
        y.fill_(float("nan"))
        cases[name]()
        torch.cuda.synchronize()
        print("bits %-16s %s  tickets zero %s" % (name, "identical" if torch.equal(y, ref) else "DIFFERENT",
                                                  int(g.long_tickets.abs().sum()) == 0), flush=True)

    reps = 10
    times = {k: [] for k in cases}
    for fn in cases.values():       # warm every case
        fn()
    for _ in range(rounds):
        for name, fn in cases.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) / reps)
    print("%-18s %9s %9s %9s   (ms per launch over %d rounds of %d, alternated)" % ("case", "median", "min", "max", rounds, reps))
    for name, ts in times.items():
        gb = alg_bytes(phases[name[6:]]) if name.startswith("phase ") else alg_bytes(g)
        print("%-18s %9.4f %9.4f %9.4f   alg %.2f TB/s" % (name, statistics.median(ts), min(ts), max(ts),
                                                            gb / (statistics.median(ts) * 1e-3) / 1e12), flush=True)


def child():
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    g, phases = c5_graphs(dev)
    x = torch.rand(g.n_rows, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) - 0.5
    y = torch.empty_like(x)
    for name, gg in [("full", g)] + list(phases.items()):
        describe(name, gg)
        for _ in range(3):
            hip_ops.spmm_raw(gg, x, Y=y)
        torch.cuda.synchronize()


def pmc(prefix):
    """One rocprofv3 pass after the other; each pass's own output goes to PREFIX.passN.log as it runs."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="mmrec_phases_")
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    passes = [["--kernel-trace", "--stats"]] + [["--kernel-trace", "--pmc"] + cs for cs in COUNTER_SETS]
    agg = {}   # grid -> {counter: [per-dispatch values]}
    for i, opts in enumerate(passes):
        d = os.path.join(tmp, "pass%d" % i)
        cmd = [exe] + opts + ["--output-format", "csv", "-d", d, "-o", "ph", "--", sys.executable, os.path.abspath(__file__), "child"]
        print("pass %d: %s" % (i, " ".join(opts)), flush=True)
        with open("%s.pass%d.log" % (prefix, i), "w") as log:
            rc = subprocess.run(cmd, cwd=tmp, stdout=log, stderr=subprocess.STDOUT, timeout=240).returncode
        if rc != 0:
            print("pass %d failed (rc %d)" % (i, rc), flush=True)
            break
        if i == 0:
            for row in csv.DictReader(open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0])):
                if "spmm_" not in row["Kernel_Name"]:
                    continue
                grid = int(row.get("Grid_Size") or int(row.get("Grid_Size_X", 1)) * int(row.get("Grid_Size_Y", 1)))
                kind = "reduce" if "long_reduce" in row["Kernel_Name"] else "rows"
                agg.setdefault((kind, grid), {}).setdefault("duration_ns", []).append(
                    float(row["End_Timestamp"]) - float(row["Start_Timestamp"]))
            continue
        per = {}
        for row in csv.DictReader(open(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0])):
            if "spmm_" not in row["Kernel_Name"]:
                continue
            kind = "reduce" if "long_reduce" in row["Kernel_Name"] else "rows"
            key = ((kind, int(row["Grid_Size"])), row["Dispatch_Id"])
            per.setdefault(key, {}).setdefault(row["Counter_Name"], 0.0)
            per[key][row["Counter_Name"]] += float(row["Counter_Value"])
        for (k, _), cs in per.items():
            for c, v in cs.items():
                agg.setdefault(k, {}).setdefault(c, []).append(v)
    shutil.rmtree(tmp, ignore_errors=True)
    lines = ["kernel  grid        dispatches  median_us   FETCH_KiB   WRITE_KiB   line_GB  line_TB/s  L2_hit"]
    for (kind, grid), cs in sorted(agg.items()):
        med = lambda c: sorted(cs[c])[len(cs[c]) // 2] if c in cs else float("nan")
        us = med("duration_ns") / 1e3
        fetch, write = med("FETCH_SIZE"), med("WRITE_SIZE")
        gb = (2 * fetch + write) * 1024 / 1e9          # FETCH_SIZE x 2 on gfx950
        hit, miss = med("TCC_HIT_sum"), med("TCC_MISS_sum")
        lines.append("%-7s %-11d %10d %10.1f %11.0f %11.0f %9.3f %10.2f %7.3f" % (
            kind, grid, len(cs.get("duration_ns", [])), us, fetch, write, gb, gb / (us * 1e-6) / 1e3, hit / (hit + miss)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    open(prefix + ".txt", "w").write(text)
    print(text, end="")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "time"
    if what == "build":
        return build()
    if what == "time":
        return time_all(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    if what == "child":
        return child()
    if what == "pmc":
        if len(sys.argv) < 3:
            raise SystemExit("usage: prof_spmm_phases.py pmc OUT_PREFIX")
        return pmc(sys.argv[2])
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
