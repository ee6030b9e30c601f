"""replace_all on the device (daac_replace_all) against the tuple route it is built on and against a plain copy: one JSON line.

Workloads: the cfg3 dictionary (100 k patterns) over `--gib` GiB of uniform text and of word soup generated on the device, find_iter
on a Standard build and leftmost_find_iter on a LeftmostLongest one.  Per workload, median of `--reps`, GB/s of haystack, measured in
the same run: replace_all(device=True) with one replacement for every match, scan_device(fmt16=True) of the same mode on the same
bytes (the tuple list replace_all starts from) and a device-to-device copy of the haystack (the floor of any splice).  With
--kernels the tool runs itself once more under `rocprofv3 --kernel-trace --stats` (a child process, no counters) and adds the time
per kernel of one replace_all per workload.

    python tools/time_replace.py [--gib 1] [--reps 3] [--kernels] [--out profiles/r13_replace_time.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import daachorse_amd as da  # noqa: E402
from daachorse_amd import ScanMode, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

REPL = b"[redacted]"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def workloads(gib):
    pats = synth.patterns_cfg3(100_000)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    pl, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats, kind=orc.KIND["LeftmostLongest"]).serialize())
    hay = torch.empty(int(gib * (1 << 30)), dtype=torch.uint8, device="cuda")
    for text in ("uniform", "word_soup"):
        if text == "uniform":
            synth.device_uniform(hay, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
        else:
            synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
        for name, pma, mode in (("find", p, ScanMode.Find), ("leftmost", pl, ScanMode.LeftmostFind)):
            yield f"{text}_{name}", pma, mode, hay


def measure(gib, reps):
    res = {}
    for name, pma, mode, hay in workloads(gib):
        n = hay.numel()
        gbs = lambda t: float(f"{n / t / 1e9:.4g}")
        r = {"bytes": n}

        def replace():
            dm = pma.replace_all(hay, REPL, mode=mode, device=True)
            r["matches"], r["out_bytes"] = dm.n_replaced, dm.count
            dm.free()
        t_rep = timed(replace, reps)
        r["route"] = da.last_kernel()
        t_tup = timed(lambda: pma.scan_device(mode, hay, fmt16=True).free(), reps)
        dst = torch.empty_like(hay)
        t_copy = timed(lambda: dst.copy_(hay), reps)
        del dst
        r["replace_gbs"], r["tuples_gbs"], r["copy_gbs"] = gbs(t_rep), gbs(t_tup), gbs(t_copy)
        r["replace_ms"], r["tuples_ms"], r["copy_ms"] = round(t_rep * 1e3, 3), round(t_tup * 1e3, 3), round(t_copy * 1e3, 3)
        r["splice_ms"] = round((t_rep - t_tup) * 1e3, 3)   # everything behind the tuple list: sizing, sums, read-back, allocation, splice
        res[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    return res


def one_pass(gib):
    """what the profiled child runs: one replace_all per workload"""
    for _, pma, mode, hay in workloads(gib):
        pma.replace_all(hay, REPL, mode=mode, device=True).free()
    torch.cuda.synchronize()


def kernel_times(gib):
    """-> {kernel: {calls, total_ms}} of the replace_* and scan kernels of one_pass, from rocprofv3's kernel statistics"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "replace", "--",
               sys.executable, os.path.abspath(__file__), "--one-pass", "--gib", str(gib)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Name"].split("(")[0]
                    e = out.setdefault(name, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(row["Calls"])
                    e["total_ms"] = round(e["total_ms"] + float(row["TotalDurationNs"]) / 1e6, 3)
        return dict(sorted(out.items(), key=lambda kv: -kv[1]["total_ms"])[:24])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--one-pass", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    da.set_option("max_result_bytes", 32 << 30)
    if args.one_pass:
        one_pass(args.gib)
        return
    res = {"tool": "time_replace", "gib": args.gib, "reps": args.reps, "replacement_bytes": len(REPL)}
    res.update(measure(args.gib, args.reps))
    if args.kernels:
        res["kernels_one_pass"] = kernel_times(args.gib)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
