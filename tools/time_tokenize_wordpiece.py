"""tokenize_wordpiece_docs on the device against its own split and against tokenize_bpe_docs on the same text: one JSON line.

Workload: `--mib` MiB of cfg3 word soup generated on the device, cut into documents of `--doc-bytes` bytes.  The WordPiece vocabulary is
the cfg3 dictionary with the 26 lower-case letters added, every piece in both roles (an initial and a continuation piece), so a word of
the soup is segmented and noise falls to single letters; [UNK] is what holds a byte outside a-z.  Median of `--reps`, GB/s of text, with
the fastest and the slowest repetition (`*_ms_min`, `*_ms_max`):
    bert_split        split_batch(Split.Bert, device=True)
    wordpiece_docs    tokenize_wordpiece_docs(device=True): split, words_space, the tuple scan, the two passes, rebase and compose
    bpe_docs_gpt2     tokenize_bpe_docs(split=Split.Gpt2, device=True) over the cfg3 dictionary (ranks = NULL), for comparison
No rate is required of the call.

Every GPU step is a child process of its own under `timeout -k 10`.  The tool stops at the first step that fails: it writes what the
steps before it gave, names the failed step and returns its status.

    python tools/time_tokenize_wordpiece.py [--mib 256] [--doc-bytes 512] [--reps 3] [--out profiles/r18_wordpiece_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("bert_split", "wordpiece_docs", "bpe_docs_gpt2")
STEP_SECONDS = 300


def timed_all(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return sorted(ts)


def step(name, mib, doc_bytes, reps):
    """one column as one JSON line on stdout"""
    import numpy as np
    import torch
    import daachorse_amd as da
    from daachorse_amd import Gap, Split, synth
    da.set_option("max_result_bytes", 64 << 30)
    pats = synth.patterns_cfg3(100_000)
    n = int(mib * (1 << 20))
    hay = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    off = torch.arange(0, n + 1, doc_bytes, dtype=torch.int64, device="cuda")
    if int(off[-1]) != n:
        off = torch.cat([off, torch.tensor([n], dtype=torch.int64, device="cuda")])
    docs = (hay, off)
    r = {"bytes": n, "docs": off.numel() - 1}
    if name == "bert_split":
        sp = da.Splitter(Split.Bert, da.bert_char_classes())

        def run():
            wo, dw = sp.split_batch(docs, device=True)
            r["words"] = wo.count - 1
            wo.free()
            dw.free()
    elif name == "wordpiece_docs":
        letters = [bytes([c]) for c in range(ord("a"), ord("z") + 1)]
        pieces = sorted(set(bytes(p) for p in pats) | set(letters))
        ids = np.arange(1, len(pieces) + 1, dtype=np.uint32)   # id 0 is [UNK]
        pma = da.DoubleArrayAhoCorasick.new(pieces)

        def run():
            out = pma.tokenize_wordpiece_docs(docs, ids, ids, 0, device=True)
            r["tokens"], r["matches"] = out[0].count, out[0].n_matches
            for o in out:
                o.free()
    else:
        pma = da.DoubleArrayAhoCorasick.new(sorted(set(bytes(p) for p in pats)))

        def run():
            out = pma.tokenize_bpe_docs(docs, None, split=Split.Gpt2, gap=Gap.Bytes, gap_id=1 << 20, device=True)
            r["tokens"], r["matches"] = out[0].count, out[0].n_matches
            for o in out:
                o.free()
    ts = timed_all(run, reps)
    t = ts[len(ts) // 2] if len(ts) % 2 else (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]) / 2
    r["gbs"], r["ms"], r["ms_min"], r["ms_max"] = float(f"{n / t / 1e9:.4g}"), round(t * 1e3, 3), round(ts[0] * 1e3, 3), round(ts[-1] * 1e3, 3)
    r["route"] = da.last_kernel()
    print(json.dumps({name: r}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--doc-bytes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # one column, run in a child
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step is not None:
        step(args.step, args.mib, args.doc_bytes, args.reps)
        return
    res = {"tool": "time_tokenize_wordpiece", "mib": args.mib, "doc_bytes": args.doc_bytes, "reps": args.reps}
    status = 0
    for name in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--mib", str(args.mib), "--doc-bytes", str(args.doc_bytes), "--reps", str(args.reps)]
        p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS)] + cmd, stdout=subprocess.PIPE)
        status = p.returncode
        if status != 0:
            print(f"step failed with status {status}: {' '.join(cmd)}", file=sys.stderr)
            res["failed_step"] = {"step": name, "status": status}
            break
        res.update(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(status)


if __name__ == "__main__":
    main()
