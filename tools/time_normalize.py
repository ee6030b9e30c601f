"""normalize_batch on the device next to a device-to-device copy and the BERT split of the same text, and tokenize_wordpiece_docs with
and without the normalizer in front of it: one JSON line.

Workload: `--mib` MiB of cfg3 word soup generated on the device, cut into documents of `--doc-bytes` bytes, and the default BERT table
(bert_normalizer()).  The soup is lower-case ASCII, so it takes the table's direct path only and nothing is rewritten: the `accented`
columns run over the same text with a 2-byte accented capital (U+00C9) put behind every 16 bytes, which takes the two-stage lookup and a
replacement from the pool once in 17 units; their documents are 18 / 16 as long, so no document boundary cuts a character.  Median of
`--reps`, GB/s of input text, with the fastest and the slowest repetition (`*_ms_min`, `*_ms_max`):
    d2d_copy                   a device-to-device copy of the text (torch.Tensor.clone): what moving the bytes once costs
    bert_split                 split_batch(Split.Bert, device=True)
    normalize                  normalize_batch(device=True)
    normalize_src              normalize_batch(src=True, device=True)
    normalize_accented         normalize_batch(device=True) over the accented text
    normalize_src_accented     normalize_batch(src=True, device=True) over the accented text
    wordpiece_docs             tokenize_wordpiece_docs(spans=True, device=True), no normalizer
    wordpiece_docs_normalized  tokenize_wordpiece_docs(spans=True, device=True, normalizer=bert_normalizer())
The WordPiece vocabulary is that of tools/time_tokenize_wordpiece.py.  No rate is required of the call.

Every GPU step is a child process of its own under `timeout -k 10`.  The tool stops at the first step that fails: it writes what the
steps before it gave, names the failed step and returns its status.

    python tools/time_normalize.py [--mib 256] [--doc-bytes 512] [--reps 3] [--out profiles/r20_normalize_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("d2d_copy", "bert_split", "normalize", "normalize_src", "normalize_accented", "normalize_src_accented", "wordpiece_docs", "wordpiece_docs_normalized")
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
    from daachorse_amd import Split, synth
    da.set_option("max_result_bytes", 64 << 30)
    pats = synth.patterns_cfg3(100_000)
    n = int(mib * (1 << 20)) // 16 * 16
    hay = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    if name.endswith("_accented"):
        wide = torch.empty((n // 16, 18), dtype=torch.uint8, device="cuda")
        wide[:, :16] = hay.view(-1, 16)
        wide[:, 16], wide[:, 17] = 0xC3, 0x89
        hay, n, doc_bytes = wide.view(-1), n // 16 * 18, doc_bytes // 16 * 18
    off = torch.arange(0, n + 1, doc_bytes, dtype=torch.int64, device="cuda")
    if int(off[-1]) != n:
        off = torch.cat([off, torch.tensor([n], dtype=torch.int64, device="cuda")])
    docs = (hay, off)
    r = {"bytes": n, "docs": off.numel() - 1}
    if name == "d2d_copy":
        def run():
            hay.clone()
    elif name == "bert_split":
        sp = da.Splitter(Split.Bert, da.bert_char_classes())

        def run():
            wo, dw = sp.split_batch(docs, device=True)
            r["words"] = wo.count - 1
            wo.free()
            dw.free()
    elif name.startswith("normalize"):
        nz = da.bert_normalizer()
        r["table_bytes"] = nz.table_bytes
        src = "_src" in name

        def run():
            out = nz.normalize_batch(docs, src=src, device=True)
            r["out_bytes"] = out[0].count
            for o in out:
                o.free()
    else:
        letters = [bytes([c]) for c in range(ord("a"), ord("z") + 1)]
        pieces = sorted(set(bytes(p) for p in pats) | set(letters))
        ids = np.arange(1, len(pieces) + 1, dtype=np.uint32)   # id 0 is [UNK]
        pma = da.DoubleArrayAhoCorasick.new(pieces)
        nz = da.bert_normalizer() if name.endswith("_normalized") else None

        def run():
            out = pma.tokenize_wordpiece_docs(docs, ids, ids, 0, spans=True, device=True, normalizer=nz)
            r["tokens"], r["matches"] = out[0].count, out[0].n_matches
            for o in out:
                o.free()
    ts = timed_all(run, reps)
    t = ts[len(ts) // 2] if len(ts) % 2 else (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]) / 2
    r["gbs"], r["ms"], r["ms_min"], r["ms_max"] = float(f"{n / t / 1e9:.4g}"), round(t * 1e3, 3), round(ts[0] * 1e3, 3), round(ts[-1] * 1e3, 3)
    if name != "d2d_copy":
        r["route"] = da.last_kernel()
    print(json.dumps({name: r}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--doc-bytes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", default=",".join(STEPS), help="the columns to run, in this order")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # one column, run in a child
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step is not None:
        step(args.step, args.mib, args.doc_bytes, args.reps)
        return
    steps = [s for s in args.steps.split(",") if s]
    for s in steps:
        if s not in STEPS:
            ap.error(f"no such step: {s}")
    res = {"tool": "time_normalize", "mib": args.mib, "doc_bytes": args.doc_bytes, "reps": args.reps}
    status = 0
    for name in steps:
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
