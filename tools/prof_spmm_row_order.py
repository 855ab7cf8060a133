#!/usr/bin/env python3
"""The row schedule of the config-5 SpMM layer against the identity row order, in ONE process: two CsrGraphs over the same
device arrays (row_schedule=True / False), HIP events, alternated rounds, a bit comparison of the outputs, the schedule's
build time and bytes (profiles/r09_spmm_row_order_*.log).

The two short-row phases are timed ALONE as in tools/prof_spmm_phases.py: launches on sub-graphs that hold only the user
rows / only the short item rows (each with its own schedule, as a row_block() shard has).

    python tools/prof_spmm_row_order.py time [rounds]          # whole launch + the two short-row phases, both orders
    python tools/prof_spmm_row_order.py sweep [rounds]         # (or --key-deg-max) ceilings 64 / 128 / 256 (MMREC_SPMM_KEY_DEG_MAX)
    python tools/prof_spmm_row_order.py child                  # a few launches of every case (the workload of `pmc`)
    python tools/prof_spmm_row_order.py pmc OUT_PREFIX         # rocprofv3 --kernel-trace --pmc <one set>, one run per set:
                                                               # FETCH_SIZE / WRITE_SIZE / TCC_HIT_sum TCC_MISS_sum
Cases are told apart in the profiler output by the kernel's template flag (scheduled: spmm_rows_kernel<1, false, true>) and
its grid size (printed by `child`)."""
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNTER_SETS = (["FETCH_SIZE"], ["WRITE_SIZE"], ["TCC_HIT_sum", "TCC_MISS_sum"])   # one pass each (what the hardware collects at once)
REPS = 10


def c5_pairs(dev, phases=True):
    """{case: (scheduled graph, identity graph)} over shared arrays: the bench's config-5 graph and its short-row phases"""
    import numpy as np
    import torch
    from mmrec_amd import hip_ops, synth
    nu, ni, eu, ei = synth.shaped_edges("c5", seed=0)
    r, c, v = synth.sym_norm_coo(eu, ei, nu, ni)
    n = nu + ni
    ident = hip_ops.CsrGraph.from_coo_device(torch.from_numpy(r.astype(np.int32)).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev),
                                             torch.from_numpy(v).to(dev), n, n, symmetric=True, row_schedule=False)
    rp = ident.rowptr_host.astype(np.int64)

    def both(rowptr, col, val, n_rows, rph, symmetric=False):
        return tuple(hip_ops.CsrGraph(rowptr, col, val, n_rows, n, symmetric=symmetric, long_row_threshold=ident.long_row_threshold,
                                      rowptr_host=rph, row_schedule=flag) for flag in (True, False))

    def sub(r0, r1, keep_long=None):
        deg = np.diff(rp[r0:r1 + 1])
        keep = np.ones(deg.shape, bool) if keep_long is None else ((deg > ident.long_row_threshold) == keep_long)
        nrp = np.concatenate([[0], np.cumsum(np.where(keep, deg, 0))]).astype(np.int32)
        m = torch.from_numpy(np.repeat(keep, deg)).to(dev)
        return both(torch.from_numpy(nrp).to(dev), ident.colidx[rp[r0]:rp[r1]][m].contiguous(),
                    ident.vals[rp[r0]:rp[r1]][m].contiguous(), r1 - r0, nrp)
    out = {"full": both(ident.rowptr, ident.colidx, ident.vals, n, ident.rowptr_host, symmetric=True)}
    if phases:
        out["users"] = sub(0, nu)
        out["items_short"] = sub(nu, n, False)
    return out


def grid_of(g):
    rpg = 1 if g.n_rows <= (1 << 18) else 4
    rows = g.sched["n_short"] if g.sched is not None else g.n_rows
    return ((rows + 16 * rpg - 1) // (16 * rpg) + g.n_chunks) * 256


def describe(name, g):
    print("%-22s rows %8d nnz %9d long rows %6d chunks %6d grid %9d schedule %.1f MB" %
          (name, g.n_rows, g.nnz, g.n_long, g.n_chunks, grid_of(g), g.schedule_bytes() / 1e6), flush=True)


def x_of(g, dev):
    import torch
    return torch.rand(g.n_cols, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) - 0.5


def build_cost(g):
    """seconds of one more build of g's schedule (key kernel, sort, gather), device-synchronised"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g._plan_schedule()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(cases, rounds):
    """{name: [ms per launch, one per round]}: every round runs every case once (REPS launches between two events)"""
    import torch
    times = {k: [] for k in cases}
    for fn in cases.values():
        fn()
    for _ in range(rounds):
        for name, fn in cases.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(REPS):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) / REPS)
    return times


def report(times, rounds):
    print("%-24s %9s %9s %9s   (ms per launch over %d rounds of %d, alternated)" % ("case", "median", "min", "max", rounds, REPS))
    for name, ts in times.items():
        print("%-24s %9.4f %9.4f %9.4f" % (name, statistics.median(ts), min(ts), max(ts)), flush=True)


def time_all(rounds):
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    pairs = c5_pairs(dev)
    x = x_of(pairs["full"][0], dev)
    cases = {}
    for name, (gs, gi) in pairs.items():
        describe(name + " scheduled", gs)
        describe(name + " identity", gi)
        ys, yi = (torch.full((gs.n_rows, 64), float("nan"), device=dev) for _ in range(2))
        hip_ops.spmm_raw(gs, x, Y=ys)
        hip_ops.spmm_raw(gi, x, Y=yi)
        torch.cuda.synchronize()
        ok = torch.equal(ys, yi) and not bool(torch.isnan(yi).any())
        print("bits %-12s scheduled vs identity: %s" % (name, "identical" if ok else "DIFFERENT"), flush=True)
        y = ys
        del yi
        cases[name + " identity"] = (lambda g=gi, y=y: hip_ops.spmm_raw(g, x, Y=y))
        cases[name + " scheduled"] = (lambda g=gs, y=y: hip_ops.spmm_raw(g, x, Y=y))
    gs = pairs["full"][0]
    secs = sorted(build_cost(gs) for _ in range(3))
    print("schedule of the full graph: %.1f MB (%d short rows, %d short nonzeros), build %.1f ms (median of 3; min %.1f)" % (
        gs.schedule_bytes() / 1e6, gs.sched["n_short"], int(gs.sched["span"][-1, 1]), secs[1] * 1e3, secs[0] * 1e3), flush=True)
    keyed = int((gs.row_key >= 0).sum())
    print("rows with a key: %d of %d short rows; key degree ceiling %d" % (keyed, gs.sched["n_short"], hip_ops.spmm_key_deg_max()))
    times = alternate(cases, rounds)
    report(times, rounds)
    for name in pairs:
        a, b = times[name + " identity"], times[name + " scheduled"]
        print("%-12s scheduled / identity (medians) %.4f   max(scheduled) %s min(identity)" % (
            name, statistics.median(b) / statistics.median(a), "<" if max(b) < min(a) else ">="), flush=True)


def sweep(rounds):
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gs0, gi = c5_pairs(dev, phases=False)["full"]
    x = x_of(gi, dev)
    y = torch.empty(gi.n_rows, 64, device=dev)
    ref = torch.empty_like(y)
    hip_ops.spmm_raw(gi, x, Y=ref)
    cases = {"identity": lambda: hip_ops.spmm_raw(gi, x, Y=y)}
    del gs0
    for k in (64, 128, 256):
        os.environ["MMREC_SPMM_KEY_DEG_MAX"] = str(k)
        g = hip_ops.CsrGraph(gi.rowptr, gi.colidx, gi.vals, gi.n_rows, gi.n_cols, symmetric=True, rowptr_host=gi.rowptr_host,
                             long_row_threshold=gi.long_row_threshold, row_schedule=True)
        y.fill_(float("nan"))
        hip_ops.spmm_raw(g, x, Y=y)
        print("key-deg-max %3d: rows with a key %d, bits %s" % (k, int((g.row_key >= 0).sum()),
                                                                 "identical" if torch.equal(y, ref) else "DIFFERENT"), flush=True)
        cases["key-deg-max %d" % k] = (lambda g=g: hip_ops.spmm_raw(g, x, Y=y))
    os.environ.pop("MMREC_SPMM_KEY_DEG_MAX")
    report(alternate(cases, rounds), rounds)


def child():
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    pairs = c5_pairs(dev)
    x = x_of(pairs["full"][0], dev)
    y = torch.empty(pairs["full"][0].n_rows, 64, device=dev)
    for name, (gs, gi) in pairs.items():
        for form, g in (("scheduled", gs), ("identity", gi)):
            describe(name + " " + form, g)
            for _ in range(3):
                hip_ops.spmm_raw(g, x, Y=y)
            torch.cuda.synchronize()


def pmc(prefix):
    """One rocprofv3 pass after the other (counters never together with anything but the kernel trace)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="mmrec_row_order_")
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    passes = [["--kernel-trace", "--stats"]] + [["--kernel-trace", "--pmc"] + cs for cs in COUNTER_SETS]
    agg, grids = {}, {}
    form = lambda kname: "scheduled" if kname.replace(" ", "").split("spmm_rows_kernel<")[-1].startswith("1,false,true") else "identity"
    for i, opts in enumerate(passes):
        d = os.path.join(tmp, "pass%d" % i)
        cmd = [exe] + opts + ["--output-format", "csv", "-d", d, "-o", "ro", "--", sys.executable, os.path.abspath(__file__), "child"]
        print("pass %d: %s" % (i, " ".join(opts)), flush=True)
        with open("%s.pass%d.log" % (prefix, i), "w") as log:
            rc = subprocess.run(cmd, cwd=tmp, stdout=log, stderr=subprocess.STDOUT, timeout=400).returncode
        if rc != 0:
            print("pass %d failed (rc %d)" % (i, rc), flush=True)
            break
        if i == 0:
            for line in open("%s.pass0.log" % prefix):
                if " grid " in line and " rows " in line:
                    grids[(line.split()[1], int(line.split(" grid ")[1].split()[0]))] = line.split()[0]
            for row in csv.DictReader(open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0])):
                if "spmm_rows_kernel" not in row["Kernel_Name"]:
                    continue
                grid = int(row.get("Grid_Size") or int(row.get("Grid_Size_X", 1)) * int(row.get("Grid_Size_Y", 1)))
                agg.setdefault((form(row["Kernel_Name"]), grid), {}).setdefault("duration_ns", []).append(
                    float(row["End_Timestamp"]) - float(row["Start_Timestamp"]))
            continue
        per = {}
        for row in csv.DictReader(open(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0])):
            if "spmm_rows_kernel" not in row["Kernel_Name"]:
                continue
            key = ((form(row["Kernel_Name"]), int(row["Grid_Size"])), row["Dispatch_Id"])
            per.setdefault(key, {}).setdefault(row["Counter_Name"], 0.0)
            per[key][row["Counter_Name"]] += float(row["Counter_Value"])
        for (k, _), cs in per.items():
            for c, v in cs.items():
                agg.setdefault(k, {}).setdefault(c, []).append(v)
    shutil.rmtree(tmp, ignore_errors=True)
    lines = ["case         form       grid        dispatches  median_us   FETCH_KiB   WRITE_KiB   line_GB  line_TB/s  L2_hit"]
    for (frm, grid), cs in sorted(agg.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        med = lambda c: sorted(cs[c])[len(cs[c]) // 2] if c in cs else float("nan")
        us = med("duration_ns") / 1e3
        fetch, write = med("FETCH_SIZE"), med("WRITE_SIZE")
        gb = (2 * fetch + write) * 1024 / 1e9          # FETCH_SIZE x 2 on gfx950
        hit, miss = med("TCC_HIT_sum"), med("TCC_MISS_sum")
        lines.append("%-12s %-10s %-11d %10d %10.1f %11.0f %11.0f %9.3f %10.2f %7.3f" % (
            grids.get((frm, grid), "?"), frm, grid, len(cs.get("duration_ns", [])), us, fetch, write, gb,
            gb / (us * 1e-6) / 1e3, hit / (hit + miss)))
    text = "\n".join(lines) + "\n"
    open(prefix + ".txt", "w").write(text)
    print(text, end="")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "time"
    what = "sweep" if what == "--key-deg-max" else what
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 and what in ("time", "sweep") else 5
    if what == "time":
        return time_all(rounds)
    if what == "sweep":
        return sweep(rounds)
    if what == "child":
        return child()
    if what == "pmc":
        if len(sys.argv) < 3:
            raise SystemExit("usage: prof_spmm_row_order.py pmc OUT_PREFIX")
        return pmc(sys.argv[2])
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
