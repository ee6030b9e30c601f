"""split_batch on the device (daac_split_batch) against a device-to-device copy of the same text and against tokenize_bpe_batch on the
words it makes: one JSON line.

Workload: `--mib` MiB of cfg3 word soup generated on the device, as one document and cut into documents of 64 and 512 bytes.  Per shape,
median of `--reps`, GB/s of text, all from the same run: split_batch(device=True) under each of `--rules`, a device-to-device copy of the buffer
(the memory-bound yardstick the split is read against) and tokenize_bpe_batch(device=True) over (hay, word_offsets) of the GPT-2 split
(the cfg3 dictionary, ranks = NULL), which shows what share of the pipeline the split is.  No rate is required of the call.  Where the
word batch holds a word above bpe_doc_max the BPE column carries the refusal instead of a figure.  `--no-bpe` leaves that column out.
Every split column also carries the fastest and the slowest of its repetitions (`*_ms_min`, `*_ms_max`): the spread a comparison between
two builds is read against.

`--text mixed` times the rules on a text with what the soup lacks and Split.O200k looks at: made from the soup once on the host, with every
7th word capitalised, U+0301 behind every 17th letter and "/" and a newline behind every 50th word, cut to `--mib` again.  `--shapes`
picks the document sizes (0: one document).

Every GPU step — a shape's split and copy columns, then a shape's BPE column — is a child process of its own under `timeout -k 10`.
The tool stops at the first step that fails: it writes what the steps before it gave, names the failed step and returns its status.

    python tools/time_split.py [--mib 256] [--reps 3] [--rules whitespace,gpt2,cl100k,llama3,o200k] [--text soup|mixed] [--shapes 0,64,512] [--no-bpe]
                               [--out profiles/r17_split_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DOC_BYTES = (0, 64, 512)   # 0: the whole text as one document
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
    return ts


def timed(fn, reps):
    import numpy as np
    return float(np.median(timed_all(fn, reps)))


def mixed_text(soup):
    """the soup (np.uint8) with capitals, marks, slashes and newlines, cut to the soup's length"""
    import numpy as np
    letter = (soup >= 97) & (soup <= 122)
    first = letter.copy()
    first[1:] &= ~letter[:-1]                     # a word's first letter
    last = letter.copy()
    last[:-1] &= ~letter[1:]                      # ... and its last
    word_no = np.cumsum(first, dtype=np.int64)    # the word a letter lies in, from 1
    out = soup.copy()
    out[first & (word_no % 7 == 0)] -= 32
    mark = np.flatnonzero(letter & (np.cumsum(letter, dtype=np.int64) % 17 == 0)) + 1
    trail = np.flatnonzero(last & (word_no % 50 == 0)) + 1
    pos = np.concatenate((mark, mark, trail, trail))
    val = np.concatenate((np.full(mark.size, 0xCC, np.uint8), np.full(mark.size, 0x81, np.uint8), np.full(trail.size, 0x2F, np.uint8), np.full(trail.size, 0x0A, np.uint8)))
    order = np.argsort(pos, kind="stable")
    return np.insert(out, pos[order], val[order])[:soup.size].copy()


def step(doc_bytes, mib, reps, bpe_column, rules, text="soup"):
    """one shape of the batch: the split and copy columns, or the BPE column, as one JSON line on stdout"""
    import torch
    import daachorse_amd as da
    from daachorse_amd import Gap, Split, synth
    from oracle import oracle as orc
    da.set_option("max_result_bytes", 32 << 30)
    pats = synth.patterns_cfg3(100_000)
    pma, _ = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    n = int(mib * (1 << 20))
    hay = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    if text == "mixed":
        hay = torch.from_numpy(mixed_text(hay.cpu().numpy())).cuda()
    if doc_bytes:
        off = torch.arange(0, n + 1, doc_bytes, dtype=torch.int64, device="cuda")
        if int(off[-1]) != n:
            off = torch.cat([off, torch.tensor([n], dtype=torch.int64, device="cuda")])
    else:
        off = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    docs = (hay, off)
    key = f"docs_of_{doc_bytes}" if doc_bytes else "one_document"
    r = {"bytes": n, "docs": off.numel() - 1, "doc_bytes": doc_bytes}
    gbs = lambda t: float(f"{n / t / 1e9:.4g}")
    for name in () if bpe_column else rules:
        rule = next(x for x in Split if x.name.lower() == name)
        sp = da.Splitter(rule)

        def split():
            wo, dw = sp.split_batch(docs, device=True)
            r[name + "_words"] = wo.count - 1
            wo.free()
            dw.free()

        ts = sorted(timed_all(split, reps))
        t = ts[len(ts) // 2] if len(ts) % 2 else (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]) / 2
        r[name + "_gbs"], r[name + "_ms"] = gbs(t), round(t * 1e3, 3)
        r[name + "_ms_min"], r[name + "_ms_max"] = round(ts[0] * 1e3, 3), round(ts[-1] * 1e3, 3)
        r["route"] = da.last_kernel()
    if not bpe_column:
        dst = torch.empty_like(hay)
        t = timed(lambda: dst.copy_(hay), reps)
        r["copy_gbs"], r["copy_ms"] = gbs(t), round(t * 1e3, 3)   # n bytes read and n written
        print(json.dumps({key: r}), flush=True)
        return
    r = {}
    wo, dw = da.Splitter(Split.Gpt2).split_batch(docs, device=True)
    words = (hay, torch.from_numpy(wo.to_numpy().astype("int64")).cuda())
    wo.free()
    dw.free()

    def bpe():
        ids, offs = pma.tokenize_bpe_batch(words, None, gap=Gap.Bytes, gap_id=1 << 20, device=True)
        r["bpe_tokens"] = ids.count
        ids.free()
        offs.free()

    try:
        t = timed(bpe, reps)
        r["bpe_gbs"], r["bpe_ms"] = gbs(t), round(t * 1e3, 3)
    except da.DaachorseError as e:
        if e.code != 6:
            raise
        r["bpe_refused"] = str(e)[:160]
    print(json.dumps({key: r}), flush=True)


def run_step(cmd, seconds):
    """a child under its own time limit -> (its status, its stdout)"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE)
    if p.returncode != 0:
        print(f"step failed with status {p.returncode}: {' '.join(cmd)}", file=sys.stderr)
    return p.returncode, p.stdout.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)   # the document size, run in a child
    ap.add_argument("--bpe", action="store_true", help=argparse.SUPPRESS)       # ... that shape's BPE column
    ap.add_argument("--rules", default="whitespace,gpt2", help="the split columns, by the lower-case names of Split")
    ap.add_argument("--no-bpe", action="store_true", help="leave out the tokenize_bpe_batch column")
    ap.add_argument("--text", default="soup", choices=("soup", "mixed"), help="mixed: the soup with capitals, marks, slashes and newlines")
    ap.add_argument("--shapes", default=",".join(map(str, DOC_BYTES)), help="the document sizes, 0 for one document")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rules = [x for x in args.rules.split(",") if x]
    if args.step is not None:
        step(args.step, args.mib, args.reps, args.bpe, rules, args.text)
        return
    res = {"tool": "time_split", "mib": args.mib, "reps": args.reps, "rules": rules, "text": args.text}
    status = 0
    for bpe_column in (False,) if args.no_bpe else (False, True):
        for doc_bytes in [int(x) for x in args.shapes.split(",") if x]:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", str(doc_bytes), "--mib", str(args.mib), "--reps", str(args.reps), "--rules", args.rules, "--text", args.text] + (["--bpe"] if bpe_column else [])
            status, out = run_step(cmd, STEP_SECONDS)
            if status != 0:
                res["failed_step"] = {"doc_bytes": doc_bytes, "bpe": bpe_column, "status": status}
                break
            for key, cols in json.loads(out.strip().splitlines()[-1]).items():
                res.setdefault(key, {}).update(cols)
        if status != 0:
            break
    for cols in res.values():
        if isinstance(cols, dict) and "gpt2_ms" in cols and "bpe_ms" in cols:
            cols["split_share_of_split_plus_bpe"] = round(cols["gpt2_ms"] / (cols["gpt2_ms"] + cols["bpe_ms"]), 4)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(status)


if __name__ == "__main__":
    main()
