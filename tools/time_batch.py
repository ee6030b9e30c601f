"""Batches (daac_scan_count_batch / daac_scan_batch_device16) against the single-haystack calls on the same bytes: one JSON line.

Workloads: the cfg3 dictionary (100 k patterns) over `--gib` GiB of device documents with lengths uniform in 64-4 096 B, and over a
log-normal mix (1 B to 4 MiB).  Per workload: batch GB/s of count, count + checksum and tuples of find_overlapping_iter; the same bytes as
ONE haystack with the same engine (TIERED and DARRAY); a loop of daac_scan_count over the first 10 000 documents, extrapolated to all; the
chain modes (find_iter, leftmost_find_iter) as batches, how many documents took the lane route and the long route, and the single-haystack
rate of the same bytes.

    python tools/time_batch.py [--gib 1] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import daachorse_amd as da  # noqa: E402
from daachorse_amd import Engine, ScanMode, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402


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


def workload(p, pl, text, lens, reps):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    nbytes = int(off[-1])
    hay = torch.from_numpy(text[:nbytes].copy()).cuda()
    offs = torch.from_numpy(off).cuda()
    n = len(lens)
    c = torch.zeros(n, dtype=torch.int64, device="cuda")
    s = torch.zeros(n, dtype=torch.int64, device="cuda")
    gbs = lambda t: float(f"{nbytes / t / 1e9:.4g}")
    r = {"docs": n, "bytes": nbytes}
    for eng, name in ((Engine.Tiered, "tiered"), (Engine.DArray, "darray")):
        t = timed(lambda: p.count_batch(ScanMode.FindOverlapping, (hay, offs), engine=eng, out=c), reps)
        r[f"batch_count_{name}_gbs"] = gbs(t)
        r[f"batch_kernel_{name}"] = da.last_kernel()
        t = timed(lambda: p.scan_count_batch(ScanMode.FindOverlapping, (hay, offs), engine=eng, out=(c, s)), reps)
        r[f"batch_checksum_{name}_gbs"] = gbs(t)
        t = timed(lambda: p.scan_count(ScanMode.FindOverlapping, hay, engine=eng), reps)
        r[f"single_{name}_gbs"] = gbs(t)
        r[f"batch_vs_single_{name}"] = round(r[f"batch_count_{name}_gbs"] / r[f"single_{name}_gbs"], 3)

    def tuples():
        dm, do = p.scan_batch_device(ScanMode.FindOverlapping, (hay, offs))
        r["tuples"] = dm.count
        dm.free()
        do.free()
    r["batch_tuples_gbs"] = gbs(timed(tuples, reps))
    # a loop of single-haystack calls over the first 10 000 documents, extrapolated
    k = min(n, 10_000)
    out = [0]

    def loop():
        for i in range(k):
            out[0] += p.scan_count(ScanMode.FindOverlapping, hay[off[i]:off[i + 1]], engine=Engine.Tiered)[0]
    t = timed(loop, 1) * n / k
    r["per_doc_loop_gbs"] = gbs(t)
    r["batch_vs_loop"] = round(r["batch_count_tiered_gbs"] / r["per_doc_loop_gbs"], 1)
    # chain modes
    for mode, pma, name in ((ScanMode.Find, p, "find"), (ScanMode.LeftmostFind, pl, "leftmost")):
        t = timed(lambda: pma.count_batch(mode, (hay, offs), out=c), reps)
        r[f"batch_{name}_gbs"] = gbs(t)
        r[f"batch_{name}_route"] = da.last_kernel()
        t = timed(lambda: pma.scan_count(mode, hay, engine=Engine.DArray), reps)
        r[f"single_{name}_darray_gbs"] = gbs(t)
        r[f"batch_vs_single_{name}"] = round(r[f"batch_{name}_gbs"] / r[f"single_{name}_darray_gbs"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    da.set_option("max_result_bytes", 32 << 30)   # word soup: ~9 GB of 16-byte tuples per GiB
    pats = synth.patterns_cfg3(100_000)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    pl, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats, kind=orc.KIND["LeftmostLongest"]).serialize())
    total = int(args.gib * (1 << 30))
    text = synth.wordsoup_haystack(total, synth.SEEDS["cfg3_dense"], pats, 20)
    rng = np.random.default_rng(3)
    uni = rng.integers(64, 4097, size=total // 2000)
    uni = uni[np.cumsum(uni) <= total]
    logn = np.clip(rng.lognormal(mean=5.0, sigma=2.0, size=total // 200), 1, 4 << 20).astype(np.int64)
    logn = logn[np.cumsum(logn) <= total]
    res = {"tool": "time_batch", "gib": args.gib}
    for name, lens in (("uniform_64_4096", uni), ("lognormal", logn)):
        res[name] = workload(p, pl, text, lens, args.reps)
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
