"""Per-document pattern counts of a batch (daac_scan_histogram_batch) against the two calls a caller had before: one JSON line.

Workloads: the cfg3 dictionary (100 k patterns) over `--gib` GiB of word soup generated on the device, cut into documents with lengths
uniform in 64-4 096 B and into a log-normal mix (1 B to 4 MiB) — the two mixes of tools/time_batch.py.  Per mix, median of `--reps`:
GB/s of haystack of histogram_batch_device (find_overlapping_iter; the other three modes on the uniform mix), of scan_batch_device (the
16-byte tuples a caller would have grouped on the host) and of count_batch (the scan's floor), the route split, and with --sweep the
same call under every batch_hist_wave_max / batch_hist_sort_max of the sweep.  The dense route's cost per document comes from the
first `--dense-docs` documents of the uniform mix, all sent through it, against the same documents at the defaults.

    python tools/time_batch_hist.py [--gib 1] [--reps 3] [--sweep] [--out profiles/r12_batch_hist_time.json]
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
from daachorse_amd import ScanMode, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

WAVE_SWEEP = (64, 128, 256, 512, 1024, 2048, 4096)
SORT_SWEEP = (4096, 8192, 16384, 32768)


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


def hist_call(p, mode, batch, info=None):
    def fn():
        dm, do = p.histogram_batch_device(mode, batch)
        if info is not None:
            info["rows"] = dm.count
        dm.free()
        do.free()
    return fn


def workload(p, pl, hay, lens, reps, sweep, chain_modes):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    nbytes = int(off[-1])
    offs = torch.from_numpy(off).cuda()
    batch = (hay, offs)
    gbs = lambda t: float(f"{nbytes / t / 1e9:.4g}")
    r = {"docs": len(lens), "bytes": nbytes}
    c = torch.zeros(len(lens), dtype=torch.int64, device="cuda")
    r["count_batch_gbs"] = gbs(timed(lambda: p.count_batch(ScanMode.FindOverlapping, batch, out=c), reps))

    def tuples():
        dm, do = p.scan_batch_device(ScanMode.FindOverlapping, batch)
        r["tuples"] = dm.count
        dm.free()
        do.free()
    r["batch_tuples_gbs"] = gbs(timed(tuples, reps))
    r["hist_batch_gbs"] = gbs(timed(hist_call(p, ScanMode.FindOverlapping, batch, r), reps))
    r["route"] = da.last_kernel()
    r["hist_vs_tuples"] = round(r["hist_batch_gbs"] / r["batch_tuples_gbs"], 3)
    if chain_modes:
        for mode, pma, name in ((ScanMode.FindOverlappingNoSuffix, p, "no_suffix"), (ScanMode.Find, p, "find"), (ScanMode.LeftmostFind, pl, "leftmost")):
            r[f"hist_batch_{name}_gbs"] = gbs(timed(hist_call(pma, mode, batch), reps))
            dm_t = timed(lambda: [x.free() for x in pma.scan_batch_device(mode, batch)], reps)
            r[f"batch_tuples_{name}_gbs"] = gbs(dm_t)
    if sweep:
        r["sweep_wave_max"], r["sweep_sort_max"] = {}, {}
        for s in SORT_SWEEP:
            p.set_option("batch_hist_sort_max", s)
            r["sweep_sort_max"][str(s)] = gbs(timed(hist_call(p, ScanMode.FindOverlapping, batch), reps))
        p.set_option("batch_hist_sort_max")
        for w in WAVE_SWEEP:
            p.set_option("batch_hist_wave_max", w)
            r["sweep_wave_max"][str(w)] = gbs(timed(hist_call(p, ScanMode.FindOverlapping, batch), reps))
        p.set_option("batch_hist_wave_max")
        r["hist_batch_after_sweep_gbs"] = gbs(timed(hist_call(p, ScanMode.FindOverlapping, batch), reps))
    return r


def dense_cost(p, hay, lens, k, reps):
    off = np.zeros(k + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens[:k])
    batch = (hay, torch.from_numpy(off).cuda())
    base = timed(hist_call(p, ScanMode.FindOverlapping, batch), reps)
    p.set_option("batch_hist_wave_max", 0).set_option("batch_hist_sort_max", 0)
    dense = timed(hist_call(p, ScanMode.FindOverlapping, batch), reps)
    route = da.last_kernel()
    p.set_option("batch_hist_wave_max").set_option("batch_hist_sort_max")
    return {"docs": k, "outputs_len": len(p.outputs()), "default_ms": round(base * 1e3, 3), "all_dense_ms": round(dense * 1e3, 3),
            "dense_us_per_doc": round((dense - base) / k * 1e6, 2), "route": route}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--dense-docs", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    da.set_option("max_result_bytes", 32 << 30)   # word soup: ~9 GB of 16-byte tuples per GiB
    pats = synth.patterns_cfg3(100_000)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    pl, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats, kind=orc.KIND["LeftmostLongest"]).serialize())
    total = int(args.gib * (1 << 30))
    hay = torch.empty(total, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    rng = np.random.default_rng(3)
    uni = rng.integers(64, 4097, size=total // 2000)
    uni = uni[np.cumsum(uni) <= total]
    logn = np.clip(rng.lognormal(mean=5.0, sigma=2.0, size=total // 200), 1, 4 << 20).astype(np.int64)
    logn = logn[np.cumsum(logn) <= total]
    res = {"tool": "time_batch_hist", "gib": args.gib, "reps": args.reps}
    for name, lens, chain in (("uniform_64_4096", uni, True), ("lognormal", logn, False)):
        res[name] = workload(p, pl, hay, lens, args.reps, args.sweep, chain)
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
    res["dense_route"] = dense_cost(p, hay, uni, min(args.dense_docs, len(uni)), args.reps)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
