"""tokenize_wordpiece_docs with and without pack= (daac_tokens_pack): one JSON line.

Workload: `--mib` MiB of cfg3 word soup generated on the device, cut into documents of `--doc-bytes` bytes (the text of
tools/time_tokenize_wordpiece.py and tools/time_special.py), tokenized by tokenize_wordpiece_docs(device=True) over the cfg3
dictionary with the 26 lower-case letters added, every piece in both roles.  The packer is Packer(bert_template(..), max_length=128,
padding="longest", dtype=np.int64).  Configurations:
    plain          pack=None (the keyword is not passed at all, so the step also runs on a commit that does not know it)
    plain_parent   the same step with the package of another checkout, `--parent DIR` (the parent commit, its library built): what
                   `plain` is compared with; left out without --parent
    pack           the same call with pack=: the chain, then the pack call, the token result freed
    pack_call      Packer.pack alone, over a token result that the chain left in device memory before the clock started
Every configuration is a child process of its own under `timeout -k 10`, warmed up once and timed `--reps` times with a host clock
around work that ends in a device synchronise; the configurations alternate over `--rounds` rounds, and per configuration the tool
reports the fastest, the median and the slowest of all its repetitions (`ms_min`, `ms`, `ms_max`).  No rate is required of the call.
`plane_bytes` is what the slot kernel writes to HBM in one call: n * L slots of four int64 planes; `slot_kernel_floor_ms` is that
over `--hbm-gbs` (the HBM rate a streaming write reaches; the default is the device's nominal 8 TB/s, so the floor is a lower bound),
the time against which `pack_slots` below is read.  The kernel reads 4 bytes a token, the 32-byte row headers and the template.

With --kernels the tool runs the `pack` configuration once more under `rocprofv3 --kernel-trace --stats` (a child process, no
counters) and adds the kernels' times: the header kernel (`pack_header`), the slot kernel (`pack_slots`) and everything else
(`chain`: the split, the tokenizer's scan, its passes, the sums and gathers), of one call.

The tool stops at the first step that fails and returns its status.

    python tools/time_pack.py [--mib 256] [--doc-bytes 512] [--reps 5] [--rounds 2] [--parent DIR] [--kernels] [--out FILE]
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

STEP_SECONDS = 300
CLS, SEP = 1 << 21, (1 << 21) + 1
MAX_LENGTH = 128


def workload(name, mib, doc_bytes):
    """-> (run, r): `run()` is one call of the configuration, `r` collects what it saw"""
    import numpy as np
    import torch
    import daachorse_amd as da
    from daachorse_amd import synth
    da.set_option("max_result_bytes", 64 << 30)
    pats = synth.patterns_cfg3(100_000)
    n = int(mib * (1 << 20)) // doc_bytes * doc_bytes
    hay = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    off = torch.arange(0, n + 1, doc_bytes, dtype=torch.int64, device="cuda")
    docs = (hay, off)
    r = {"bytes": n, "docs": off.numel() - 1}
    letters = [bytes([c]) for c in range(ord("a"), ord("z") + 1)]
    pieces = sorted(set(bytes(p) for p in pats) | set(letters))
    ids = np.arange(1, len(pieces) + 1, dtype=np.uint32)   # id 0 is [UNK]
    pma = da.DoubleArrayAhoCorasick.new(pieces)
    if name == "plain":
        def run():
            out = pma.tokenize_wordpiece_docs(docs, ids, ids, 0, device=True)
            r["tokens"], r["matches"] = out[0].count, out[0].n_matches
            for o in out:
                o.free()
        return run, r
    packer = da.Packer(da.bert_template(CLS, SEP), max_length=MAX_LENGTH, padding="longest", dtype=np.int64)

    def seen(out):
        r["rows"], r["row_length"] = out["input_ids"].shape
        r["plane_bytes"] = 4 * 8 * r["rows"] * r["row_length"]
        r["last_kernel"] = da.last_kernel()
        for o in out.values():
            o.free()

    if name == "pack":
        def run():
            seen(pma.tokenize_wordpiece_docs(docs, ids, ids, 0, device=True, pack=packer))
        return run, r
    tokens = pma.tokenize_wordpiece_docs(docs, ids, ids, 0, device=True)   # pack_call: kept for every repetition
    r["tokens"] = tokens[0].count

    def run():
        seen(packer.pack(tuple(tokens), device=True))
    return run, r


def step(name, mib, doc_bytes, reps, package):
    """one configuration, timed: one JSON line on stdout"""
    sys.path.insert(0, package or ROOT)
    import torch
    run, r = workload("plain" if name == "plain_parent" else name, mib, doc_bytes)
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ts.append(round((time.perf_counter() - t) * 1e3, 3))
    r["ms_all"] = ts
    print(json.dumps({name: r}), flush=True)


def one_pass(mib, doc_bytes):
    """the `pack` configuration twice, for the profiler: the first call loads the code objects"""
    sys.path.insert(0, ROOT)
    import torch
    run, _ = workload("pack", mib, doc_bytes)
    run()
    run()
    torch.cuda.synchronize()


def run_step(cmd, seconds):
    """a child under its own time limit -> its stdout; the tool ends with the child's status when that is not 0"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE)
    if p.returncode != 0:
        print(f"step failed with status {p.returncode}: {' '.join(cmd)}", file=sys.stderr)
        sys.exit(p.returncode)
    return p.stdout.decode()


def group_of(kernel):
    if "pack_header_kernel" in kernel:
        return "pack_header"
    if "pack_slots_kernel" in kernel:
        return "pack_slots"
    return "chain"


def kernel_times(mib, doc_bytes):
    """-> ({kernel: {calls, total_ms}}, {group: ms of one call}) of one_pass, from rocprofv3's kernel statistics"""
    with tempfile.TemporaryDirectory() as d:
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pack", "--",
                  sys.executable, os.path.abspath(__file__), "--one-pass", "--mib", str(mib), "--doc-bytes", str(doc_bytes)], 2 * STEP_SECONDS)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Name"].split("(")[0]
                    e = out.setdefault(name, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(row["Calls"])
                    e["total_ms"] = round(e["total_ms"] + float(row["TotalDurationNs"]) / 1e6, 3)
    groups = {"pack_header": 0.0, "pack_slots": 0.0, "chain": 0.0}
    for name, e in out.items():
        groups[group_of(name)] += e["total_ms"] / 2   # two calls in one_pass
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["total_ms"])[:32]), {g + "_ms": round(v, 3) for g, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--doc-bytes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM write rate the slot kernel's floor is computed with")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # one configuration, run in a child
    ap.add_argument("--package", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--one-pass", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one_pass:
        one_pass(args.mib, args.doc_bytes)
        return
    if args.step:
        step(args.step, args.mib, args.doc_bytes, args.reps, args.package)
        return
    res = {"tool": "time_pack", "mib": args.mib, "doc_bytes": args.doc_bytes, "reps": args.reps, "rounds": args.rounds, "max_length": MAX_LENGTH}
    names = (["plain_parent"] if args.parent else []) + ["plain", "pack", "pack_call"]
    for _ in range(args.rounds):
        for name in names:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--mib", str(args.mib), "--doc-bytes", str(args.doc_bytes), "--reps", str(args.reps)]
            if name == "plain_parent":
                cmd += ["--package", os.path.abspath(args.parent)]
            r = json.loads(run_step(cmd, STEP_SECONDS).strip().splitlines()[-1])[name]
            e = res.setdefault(name, r)
            if e is not r:
                e["ms_all"] += r["ms_all"]
    for name in names:
        e = res[name]
        ts = sorted(e["ms_all"])
        e["ms_min"], e["ms"], e["ms_max"] = ts[0], ts[len(ts) // 2], ts[-1]
    # differences of the fastest repetitions: on a shared machine the medians move with the neighbours' work
    res["pack_over_plain_ms"] = round(res["pack"]["ms_min"] - res["plain"]["ms_min"], 3)
    res["plane_bytes"] = res["pack"]["plane_bytes"]
    res["slot_kernel_floor_ms"] = round(res["plane_bytes"] / (args.hbm_gbs * 1e9) * 1e3, 3)
    if args.parent:
        res["plain_over_parent_ms"] = round(res["plain"]["ms_min"] - res["plain_parent"]["ms_min"], 3)
    if args.kernels:
        res["kernels_two_calls"], res["kernel_groups_one_call"] = kernel_times(args.mib, args.doc_bytes)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
