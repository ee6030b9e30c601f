"""tokenize on the device (daac_tokenize) against the tuple route it is built on and against a plain copy: one JSON line.

Workloads: the cfg3 dictionary (100 k patterns) over `--gib` GiB of uniform text and of word soup generated on the device, find_iter
on a Standard build and leftmost_find_iter on a LeftmostLongest one, each with Gap.Unk and Gap.Chars.  Per workload, median of `--reps`,
GB/s of haystack, measured in the same run: tokenize(device=True), scan_device(fmt16=True) of the same mode on the same bytes (the
tuple list tokenize starts from) and a device-to-device copy of the haystack.  Behind the tuple list the passes read the text about
twice, so `passes_ms` is to be read against twice `copy_ms`.  With --kernels the tool adds the time per kernel of one tokenize per
workload from one `rocprofv3 --kernel-trace --stats` run (no counters).

Every GPU step is a child process of its own under `timeout -k 10`; the tool stops at the first step that fails and returns its status.

    python tools/time_tokenize.py [--gib 1] [--reps 3] [--kernels] [--out profiles/r14_tokenize_time.json]
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

TEXTS = ("uniform", "word_soup")
MODES = ("find", "leftmost")
GAPS = ("Unk", "Chars")
STEP_SECONDS = 300


def timed(fn, reps):
    import numpy as np
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def workload(text, mode_name, gib):
    """-> (pma, mode, haystack tensor) of one step"""
    import torch
    import daachorse_amd as da
    from daachorse_amd import ScanMode, synth
    from oracle import oracle as orc
    da.set_option("max_result_bytes", 32 << 30)
    pats = synth.patterns_cfg3(100_000)
    kind = orc.KIND["Standard"] if mode_name == "find" else orc.KIND["LeftmostLongest"]
    pma, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats, kind=kind).serialize())
    hay = torch.empty(int(gib * (1 << 30)), dtype=torch.uint8, device="cuda")
    if text == "uniform":
        synth.device_uniform(hay, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
    else:
        synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    return pma, (ScanMode.Find if mode_name == "find" else ScanMode.LeftmostFind), hay


def step(text, mode_name, gib, reps):
    """one text and mode: both gap rules, the tuple list and the copy, as one JSON line on stdout"""
    import torch
    import daachorse_amd as da
    from daachorse_amd import Gap
    pma, mode, hay = workload(text, mode_name, gib)
    n = hay.numel()
    gbs = lambda t: float(f"{n / t / 1e9:.4g}")
    t_tup = timed(lambda: pma.scan_device(mode, hay, fmt16=True).free(), reps)
    dst = torch.empty_like(hay)
    t_copy = timed(lambda: dst.copy_(hay), reps)
    del dst
    out = {}
    for gap in GAPS:
        r = {"bytes": n}

        def tokenize():
            dm = pma.tokenize(hay, gap=Gap[gap], gap_id=1 << 20, mode=mode, device=True)
            r["matches"], r["tokens"] = dm.n_matches, dm.count
            dm.free()
        t_tok = timed(tokenize, reps)
        r["route"] = da.last_kernel()
        r["tokenize_gbs"], r["tuples_gbs"], r["copy_gbs"] = gbs(t_tok), gbs(t_tup), gbs(t_copy)
        r["tokenize_ms"], r["tuples_ms"], r["copy_ms"] = round(t_tok * 1e3, 3), round(t_tup * 1e3, 3), round(t_copy * 1e3, 3)
        r["passes_ms"] = round((t_tok - t_tup) * 1e3, 3)   # everything behind the tuple list: prep, sums, count, read-back, allocation, write
        out[f"{text}_{mode_name}_{gap.lower()}"] = r
    print(json.dumps(out), flush=True)


def one_pass(gib):
    """what the profiled child runs: one tokenize per workload"""
    import torch
    from daachorse_amd import Gap
    for text in TEXTS:
        for mode_name in MODES:
            pma, mode, hay = workload(text, mode_name, gib)
            for gap in GAPS:
                pma.tokenize(hay, gap=Gap[gap], gap_id=1 << 20, mode=mode, device=True).free()
            del hay
    torch.cuda.synchronize()


def run_step(cmd, seconds):
    """a child under its own time limit -> its stdout; the tool ends with the child's status when that is not 0"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE)
    if p.returncode != 0:
        print(f"step failed with status {p.returncode}: {' '.join(cmd)}", file=sys.stderr)
        sys.exit(p.returncode)
    return p.stdout.decode()


def kernel_times(gib):
    """-> {kernel: {calls, total_ms}} of one_pass, from rocprofv3's kernel statistics"""
    with tempfile.TemporaryDirectory() as d:
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tokenize", "--",
                  sys.executable, os.path.abspath(__file__), "--one-pass", "--gib", str(gib)], 2 * STEP_SECONDS)
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
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # text:mode, run in a child
    ap.add_argument("--one-pass", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one_pass:
        one_pass(args.gib)
        return
    if args.step:
        text, mode_name = args.step.split(":")
        step(text, mode_name, args.gib, args.reps)
        return
    res = {"tool": "time_tokenize", "gib": args.gib, "reps": args.reps}
    for text in TEXTS:
        for mode_name in MODES:
            lines = run_step([sys.executable, os.path.abspath(__file__), "--step", f"{text}:{mode_name}", "--gib", str(args.gib), "--reps",
                              str(args.reps)], STEP_SECONDS).strip().splitlines()
            res.update(json.loads(lines[-1]))
    if args.kernels:
        res["kernels_one_pass"] = kernel_times(args.gib)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
