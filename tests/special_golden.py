"""The special-token fixture of tests/golden/ (written by make_special_golden.py from `tokenizers`) as the host tests and the GPU tests
read it, and the definitions of daac_cut_batch and daac_tokens_splice in pure Python.  A plain helper: no test lives here, and nothing
here reads `tokenizers`."""
import functools
import json
import os

import numpy as np

import wordpiece_golden as wg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXT = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def load():
    with open(os.path.join(GOLDEN, "special_tokens_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def specials(which):
    """which: "bpe" or "wordpiece" -> [(bytes, id)] in the maker's list order"""
    return [(t.encode(), i) for t, i in load()[which + "_specials"]]


def docs():
    return [d.encode() for d in load()["docs"]]


def wordpiece_spans():
    return [wg.unpack_spans(x) for x in load()["wordpiece_spans"]]


def bpe_spans(pieces_len, special_len):
    """the tiling spans of the BPE ids: a piece's length is its bytes, a special's its text"""
    out = []
    for ids in load()["bpe_ids"]:
        pos, spans = 0, []
        for i in ids:
            n = special_len[i] if i in special_len else pieces_len[i]
            spans.append((pos, pos + n))
            pos += n
        out.append(spans)
    return out


# ---------------------------------------------------------------------------------------------------------- the definitions
def leftmost(doc, spec, longest=True):
    """leftmost_find_iter of one document over [(pattern, value)]: at the first position where a pattern starts, the longest one
    (`longest=False`: the first in list order), then on behind it -> [(start, end, value)]"""
    out, p = [], 0
    while p < len(doc):
        here = [(len(t), v) for t, v in spec if doc.startswith(t, p)]
        if not here:
            p += 1
            continue
        n, v = max(here, key=lambda x: x[0]) if longest else here[0]
        out.append((p, p + n, v))
        p += n
    return out


def cut(docs_, scan, base=0):
    """daac_cut_batch: `scan(doc)` -> the document's [(start, end, value)] -> (seg_offsets, doc_segs, seg_values)"""
    seg_offsets, doc_segs, seg_values, at = [], [0], [], base
    for d in docs_:
        pos = 0
        for s, e, v in list(scan(d)) + [(len(d), len(d), None)]:
            if s > pos:
                seg_offsets.append(at + pos)
                seg_values.append(TEXT)
            if v is not None:
                seg_offsets.append(at + s)
                seg_values.append(v)
            pos = e
        at += len(d)
        doc_segs.append(len(seg_values))
    return np.array(seg_offsets + [at], dtype=np.uint64), np.array(doc_segs, dtype=np.uint64), np.array(seg_values, dtype=np.uint32)


def splice(ids, spans, seg_tok, seg_values, seg_offsets, doc_segs, doc_offsets):
    """daac_tokens_splice -> (ids, spans or None, doc_tok)"""
    out_ids, out_spans, doc_tok = [], [], [0]
    for d in range(len(doc_offsets) - 1):
        for s in range(int(doc_segs[d]), int(doc_segs[d + 1])):
            delta = int(seg_offsets[s]) - int(doc_offsets[d])
            if seg_values[s] != TEXT:
                out_ids.append(int(seg_values[s]))
                out_spans.append((delta, delta + int(seg_offsets[s + 1]) - int(seg_offsets[s])))
                continue
            for t in range(int(seg_tok[s]), int(seg_tok[s + 1])):
                out_ids.append(int(ids[t]))
                if spans is not None:
                    out_spans.append((int(spans[t][0]) + delta, int(spans[t][1]) + delta))
        doc_tok.append(len(out_ids))
    return (np.array(out_ids, dtype=np.uint32), None if spans is None else np.array(out_spans, dtype=np.uint64).reshape(-1, 2),
            np.array(doc_tok, dtype=np.uint64))


def tokenize_docs(docs_, scan, tokenize_text):
    """cut, `tokenize_text(bytes)` -> (ids, spans) on every text segment and one garbage token on every special one, splice -> per
    document (ids, spans)"""
    so, ds, sv = cut(docs_, scan)
    hay = b"".join(docs_)
    ids, spans, seg_tok = [], [], [0]
    for s in range(len(sv)):
        if sv[s] == TEXT:
            i, sp = tokenize_text(hay[int(so[s]):int(so[s + 1])])
            ids += list(i)
            spans += list(sp)
        else:
            ids.append(0xDEAD)
            spans.append((0, 1))
        seg_tok.append(len(ids))
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs_])]).astype(np.uint64)
    oi, osp, dt = splice(ids, spans, seg_tok, sv, so, ds, off)
    return [(oi[int(a):int(b)].tolist(), [tuple(x) for x in osp[int(a):int(b)].tolist()]) for a, b in zip(dt, dt[1:])]
