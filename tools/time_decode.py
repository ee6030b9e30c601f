"""Decoder.decode_batch (daac_tokens_decode) beside its two yardsticks: one JSON line.

Workload: `--mib` MiB of cfg3 word soup generated on the device, cut into documents of `--doc-bytes` bytes (the README's standing one:
256 MiB as 524 288 documents of 512 bytes), tokenized once with each of the two fixture vocabularies of tests/golden/: WordPiece
(tokenizer_wordpiece_vocab.json, Split.Bert) and byte-level BPE (tokenizer_bpe_vocab.json, Split.Gpt2).  Per vocabulary, in ONE child
process (one session), each step warmed up once and timed `--reps` times with a host clock around work that ends in a device
synchronise:
    encode        tokenize_wordpiece_docs / tokenize_bpe_docs(device=True) of the batch: the call that decode reverses (yardstick)
    decode_csr    decode_batch(device=True) from that CSR token result
    decode_plane  decode_batch(device=True) from the [n, 128] int64 input_ids plane of pack= (the template's ids and the padding flagged
                  special, max_length 128, rows padded to 128)
    memcpy        a device-to-device hipMemcpyAsync (torch's copy_ of a contiguous uint8 tensor) of as many bytes as decode_csr wrote:
                  the floor of any pass that writes them (yardstick)
Per step the tool reports the fastest, the median and the slowest repetition (`ms_min`, `ms`, `ms_max`).  On a shared machine the
medians move with the neighbours' work, so the ratios are taken over the fastest repetitions only:
    call_over_encode     decode_csr.ms_min / encode.ms_min
    copy_over_memcpy     (out_bytes / copy kernel time) / (out_bytes / memcpy.ms_min), with --kernels
With --kernels the tool runs decode_csr twice more per vocabulary under `rocprofv3 --kernel-trace --stats` (a child process of its own,
no counters) and adds the time of one call's copy kernel (`copy_ms`), sizing pass (`size_ms`) and the rest of the call's kernels.  No
rate is required of the call.  The tool stops at the first step that fails and returns its status.

    python tools/time_decode.py [--mib 256] [--doc-bytes 512] [--reps 10] [--kernels] [--out FILE]
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
GOLDEN = os.path.join(ROOT, "tests", "golden")

STEP_SECONDS = 420
ROW = 128
VOCABS = ("wordpiece", "bpe")


def workload(vocab, mib, doc_bytes):
    """-> (docs, encode, packed, decoder): the batch on the device, encode(pack=None) and the decoder of the vocabulary"""
    import numpy as np
    import torch
    import daachorse_amd as da
    from daachorse_amd import synth
    da.set_option("max_result_bytes", 64 << 30)
    pats = synth.patterns_cfg3(100_000)
    n = int(mib * (1 << 20)) // doc_bytes * doc_bytes
    hay = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(hay, synth.SEEDS["cfg3_dense"], pats, 20)
    docs = (hay, torch.arange(0, n + 1, doc_bytes, dtype=torch.int64, device="cuda"))
    with open(os.path.join(GOLDEN, f"tokenizer_{vocab}_vocab.json"), encoding="utf-8") as f:
        v = json.load(f)
    if vocab == "wordpiece":
        patterns, first, cont = da.wordpiece_tables(v["vocab"], v["prefix"])
        pma = da.DoubleArrayAhoCorasick.new(patterns)
        k = len(v["vocab"])
        spec = da.SpecialTokens({"[CLS]": k, "[SEP]": k + 1, "[PAD]": k + 2})
        dec = da.Decoder.wordpiece(v["vocab"], v["prefix"], special=spec)
        packer = da.Packer(da.bert_template(k, k + 1), max_length=ROW, padding=ROW, pad_id=k + 2, dtype=np.int64)

        def encode(pack=None):
            kw = {} if pack is None else {"pack": pack}
            return pma.tokenize_wordpiece_docs(docs, first, cont, v["unk_id"], v["max_input_chars_per_word"], device=True, **kw)
    else:
        pieces = [bytes.fromhex(h) for h in v["pieces_hex"]]
        pma = da.DoubleArrayAhoCorasick.with_values([(p, i) for i, p in enumerate(pieces)])
        k = len(pieces)
        spec = da.SpecialTokens({"<s>": k, "</s>": k + 1, "<pad>": k + 2})
        dec = da.Decoder.byte_level(pieces, special=spec)
        packer = da.Packer(da.roberta_template(k, k + 1), max_length=ROW, padding=ROW, pad_id=k + 2, dtype=np.int64)

        def encode(pack=None):
            kw = {} if pack is None else {"pack": pack}
            return pma.tokenize_bpe_docs(docs, split=da.Split.Gpt2, gap=da.Gap.Bytes, gap_id=1 << 20, device=True, **kw)
    return docs, encode, packer, dec


def timed(run, reps):
    import torch
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ts.append(round((time.perf_counter() - t) * 1e3, 3))
    s = sorted(ts)
    return {"ms_min": s[0], "ms": s[len(s) // 2], "ms_max": s[-1], "ms_all": ts}


def free(out):
    for o in (out.values() if isinstance(out, dict) else out):
        o.free()


def step(vocab, mib, doc_bytes, reps):
    """one vocabulary's four steps in one session: one JSON line on stdout"""
    sys.path.insert(0, ROOT)
    import torch
    import daachorse_amd as da
    docs, encode, packer, dec = workload(vocab, mib, doc_bytes)
    r = {"bytes": docs[0].numel(), "docs": docs[1].numel() - 1}
    r["encode"] = timed(lambda: free(encode()), reps)
    tokens = encode()
    r["tokens"] = tokens[0].count

    def decode_csr():
        out = dec.decode_batch(tuple(tokens), device=True)
        r["out_bytes"], r["last_kernel"] = out[0].count, da.last_kernel()
        free(out)

    r["decode_csr"] = timed(decode_csr, reps)
    free(tokens)
    planes = encode(packer)
    r["plane_shape"] = list(planes["input_ids"].shape)

    def decode_plane():
        out = dec.decode_batch(planes["input_ids"], device=True)
        r["plane_out_bytes"], r["plane_last_kernel"] = out[0].count, da.last_kernel()
        free(out)

    r["decode_plane"] = timed(decode_plane, reps)
    free(planes)
    src = torch.empty(r["out_bytes"], dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    r["memcpy"] = timed(lambda: dst.copy_(src), reps)
    print(json.dumps({vocab: r}), flush=True)


def one_pass(vocab, mib, doc_bytes):
    """decode_csr twice, for the profiler: the first call loads the code objects"""
    sys.path.insert(0, ROOT)
    import torch
    _, encode, _, dec = workload(vocab, mib, doc_bytes)
    tokens = encode()
    for _ in range(2):
        free(dec.decode_batch(tuple(tokens), device=True))
    torch.cuda.synchronize()


def run_step(cmd, seconds):
    """a child under its own time limit -> its stdout; the tool ends with the child's status when that is not 0"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE)
    if p.returncode != 0:
        print(f"step failed with status {p.returncode}: {' '.join(cmd)}", file=sys.stderr)
        sys.exit(p.returncode)
    return p.stdout.decode()


def kernel_times(vocab, mib, doc_bytes):
    """-> {copy_ms, size_ms, other_decode_ms} of one decode call of one_pass, from rocprofv3's kernel statistics"""
    groups = {"copy_ms": 0.0, "size_ms": 0.0, "other_decode_ms": 0.0}
    with tempfile.TemporaryDirectory() as d:
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "decode", "--",
                  sys.executable, os.path.abspath(__file__), "--one-pass", vocab, "--mib", str(mib), "--doc-bytes", str(doc_bytes)], 2 * STEP_SECONDS)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name, ms = row["Name"].split("(")[0], float(row["TotalDurationNs"]) / 1e6 / 2   # two calls in one_pass
                    if "decode_copy_kernel" in name:
                        groups["copy_ms"] += ms
                    elif "decode_size_kernel" in name:
                        groups["size_ms"] += ms
                    elif "decode_" in name:
                        groups["other_decode_ms"] += ms
    return {k: round(v, 3) for k, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--doc-bytes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # one vocabulary, run in a child
    ap.add_argument("--one-pass", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one_pass:
        one_pass(args.one_pass, args.mib, args.doc_bytes)
        return
    if args.step:
        step(args.step, args.mib, args.doc_bytes, args.reps)
        return
    res = {"tool": "time_decode", "mib": args.mib, "doc_bytes": args.doc_bytes, "reps": args.reps, "row": ROW}
    for vocab in VOCABS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", vocab, "--mib", str(args.mib), "--doc-bytes", str(args.doc_bytes), "--reps", str(args.reps)]
        r = res[vocab] = json.loads(run_step(cmd, STEP_SECONDS).strip().splitlines()[-1])[vocab]
        # ratios of the fastest repetitions: on a shared machine the medians move with the neighbours' work
        r["call_over_encode"] = round(r["decode_csr"]["ms_min"] / r["encode"]["ms_min"], 4)
        r["plane_call_over_encode"] = round(r["decode_plane"]["ms_min"] / r["encode"]["ms_min"], 4)
        r["memcpy_gbs"] = round(r["out_bytes"] / r["memcpy"]["ms_min"] / 1e6, 1)
        if args.kernels:
            r.update(kernel_times(vocab, args.mib, args.doc_bytes))
            if r["copy_ms"] > 0:
                r["copy_gbs"] = round(r["out_bytes"] / r["copy_ms"] / 1e6, 1)
                r["copy_over_memcpy"] = round(r["copy_gbs"] / r["memcpy_gbs"], 4)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
