"""Histograms (daac_scan_histogram) against the same engine's count + checksum scan on the same bytes: one JSON line.

Workloads: the cfg3 dictionary (100 k patterns) over `--gib` GiB of device text, uniform and word soup, on TIERED and DARRAY, and the
cfg5 dictionary on the charwise engine over Zipf text.  Per workload and engine: GB/s of daac_scan_count (count + checksum, forced to
that engine) and of the histogram with option hist_lds_bins swept over 0, a few powers of two and the most LDS the engine leaves
(the library clamps; the bins it ran with are read back from daac_last_kernel()), plus the rate at the library's default.

    python tools/time_hist.py [--gib 1] [--reps 3] [--out profiles/r11_hist_time.json]
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import daachorse_amd as da  # noqa: E402
from daachorse_amd import Engine, ScanMode, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

SWEEP = (0, 256, 1024, 4096, 16384, 1 << 30)


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


def workload(p, hay, engines, reps):
    nbytes = hay.numel()
    gbs = lambda t: float(f"{nbytes / t / 1e9:.4g}")
    out = torch.zeros(len(p.outputs()), dtype=torch.int64, device="cuda")
    mode = ScanMode.FindOverlapping
    r = {"bytes": nbytes}
    for eng, name in engines:
        e = {}
        count, _ = p.scan_count(mode, hay, engine=eng)
        e["count_checksum_gbs"] = gbs(timed(lambda: p.scan_count(mode, hay, engine=eng), reps))
        e["count_checksum_kernel"] = da.last_kernel()
        e["matches_per_byte"] = round(count / nbytes, 3)
        p.set_option("hist_lds_bins")
        e["hist_default_gbs"] = gbs(timed(lambda: p.histogram(mode, hay, engine=eng, out=out), reps))
        e["hist_kernel"] = da.last_kernel()
        assert int(out.sum().item()) == count
        e["heads_only_default_gbs"] = gbs(timed(lambda: p.histogram(ScanMode.FindOverlappingNoSuffix, hay, engine=eng, out=out), reps))
        sweep = {}
        for bins in SWEEP:
            p.set_option("hist_lds_bins", bins)
            t = timed(lambda: p.histogram(mode, hay, engine=eng, out=out), reps)
            ran = int(re.search(r"lds_bins=(\d+)", da.last_kernel()).group(1))
            assert int(out.sum().item()) == count
            sweep[str(ran)] = gbs(t)
        p.set_option("hist_lds_bins")
        e["hist_gbs_by_lds_bins"] = sweep
        e["best_lds_bins"] = int(max(sweep, key=sweep.get))
        e["hist_default_vs_count_checksum"] = round(e["hist_default_gbs"] / e["count_checksum_gbs"], 3)
        r[name] = e
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    total = int(args.gib * (1 << 30))
    res = {"tool": "time_hist", "gib": args.gib, "reps": args.reps}
    pats = synth.patterns_cfg3(100_000)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    hay = torch.empty(total, dtype=torch.uint8, device="cuda")
    both = ((Engine.Tiered, "tiered"), (Engine.DArray, "darray"))
    synth.device_uniform(hay, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
    res["cfg3_uniform"] = workload(p, hay, both, args.reps)
    print("cfg3_uniform", json.dumps(res["cfg3_uniform"]), file=sys.stderr, flush=True)
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    res["cfg3_wordsoup"] = workload(p, hay, both, args.reps)
    print("cfg3_wordsoup", json.dumps(res["cfg3_wordsoup"]), file=sys.stderr, flush=True)
    del p
    cp = synth.patterns_cfg5()
    c, _ = da.CharwiseDoubleArrayAhoCorasick.deserialize(orc.OracleCharwisePma.build(cp).serialize())
    n = total - total % synth.CFG5_SLOT
    synth.device_zipf_text(hay[:n])
    res["cfg5_zipf"] = workload(c, hay[:n], ((Engine.DArray, "charwise"),), args.reps)
    print("cfg5_zipf", json.dumps(res["cfg5_zipf"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
