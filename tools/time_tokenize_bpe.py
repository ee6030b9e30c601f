"""tokenize_bpe on the device (daac_tokenize_bpe_batch) against the tuple list it starts from and against tokenize_unigram: one JSON line.

Workload: the cfg3 dictionary (100 k patterns, ranks = NULL: a pattern's rank is its value) over `--mib` MiB of word soup generated on
the device, cut into documents of 8, 64 and 512 bytes.  Per document size, median of `--reps`, GB/s of text, all from the same run:
tokenize_bpe_batch(device=True), scan_batch_device(FindOverlapping) on the same batch (the list the call starts from) and
tokenize_unigram_batch(device=True) (one random score per pattern).  No rate is required of the call; what matters is `passes_ms`, the
time on top of the tuple list.

Every GPU step is a child process of its own under `timeout -k 10`; the tool stops at the first step that fails and returns its status.

    python tools/time_tokenize_bpe.py [--mib 256] [--reps 3] [--out profiles/r16_tokenize_bpe_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DOC_BYTES = (8, 64, 512)
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


def step(doc_bytes, mib, reps):
    """one document size: the three columns as one JSON line on stdout"""
    import numpy as np
    import torch
    import daachorse_amd as da
    from daachorse_amd import Gap, ScanMode, synth
    from oracle import oracle as orc
    da.set_option("max_result_bytes", 32 << 30)
    pats = synth.patterns_cfg3(100_000)
    pma, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    scores = (-np.random.default_rng(15).gamma(2.0, 3.0, size=len(pats))).astype(np.float32)
    n = int(mib * (1 << 20))
    hay = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    off = torch.arange(0, n + 1, doc_bytes, dtype=torch.int64, device="cuda")
    if int(off[-1]) != n:
        off = torch.cat([off, torch.tensor([n], dtype=torch.int64, device="cuda")])
    docs = (hay, off)
    r = {"bytes": n, "docs": off.numel() - 1, "doc_bytes": doc_bytes}

    def bpe():
        ids, offs = pma.tokenize_bpe_batch(docs, None, gap=Gap.Bytes, gap_id=1 << 20, device=True)
        r["matches"], r["tokens"] = ids.n_matches, ids.count
        ids.free()
        offs.free()

    def tuples():
        dm, do = pma.scan_batch_device(ScanMode.FindOverlapping, docs)
        dm.free()
        do.free()

    def unigram():
        ids, offs = pma.tokenize_unigram_batch(docs, scores, -20.0, gap=Gap.Bytes, gap_id=1 << 20, device=True)
        r["unigram_tokens"] = ids.count
        ids.free()
        offs.free()

    t_bpe = timed(bpe, reps)
    r["route"] = da.last_kernel()
    t_tup = timed(tuples, reps)
    t_uni = timed(unigram, reps)
    gbs = lambda t: float(f"{n / t / 1e9:.4g}")
    r["bpe_gbs"], r["tuples_gbs"], r["unigram_gbs"] = gbs(t_bpe), gbs(t_tup), gbs(t_uni)
    r["bpe_ms"], r["tuples_ms"], r["unigram_ms"] = round(t_bpe * 1e3, 3), round(t_tup * 1e3, 3), round(t_uni * 1e3, 3)
    r["passes_ms"] = round((t_bpe - t_tup) * 1e3, 3)   # everything behind the tuple list: ranks, index + merge, sum, read-back, allocation, write
    print(json.dumps({f"docs_of_{doc_bytes}": r}), flush=True)


def run_step(cmd, seconds):
    """a child under its own time limit -> its stdout; the tool ends with the child's status when that is not 0"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE)
    if p.returncode != 0:
        print(f"step failed with status {p.returncode}: {' '.join(cmd)}", file=sys.stderr)
        sys.exit(p.returncode)
    return p.stdout.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)   # the document size, run in a child
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.mib, args.reps)
        return
    res = {"tool": "time_tokenize_bpe", "mib": args.mib, "reps": args.reps}
    for doc_bytes in DOC_BYTES:
        lines = run_step([sys.executable, os.path.abspath(__file__), "--step", str(doc_bytes), "--mib", str(args.mib), "--reps", str(args.reps)],
                         STEP_SECONDS).strip().splitlines()
        res.update(json.loads(lines[-1]))
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
