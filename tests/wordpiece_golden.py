"""The WordPiece fixtures of tests/golden/ (written by make_wordpiece_golden.py from `tokenizers`) as the host tests and the GPU tests read
them, and the two definitions in pure Python that the generator checked against `tokenizers` on every document: the sequential
Split.Bert scanner and greedy longest-match-first with roles.  A plain helper: no test lives here, and nothing here reads `tokenizers`."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFFFFFF
O, L, N, S = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def load(name):
    with open(os.path.join(GOLDEN, f"tokenizer_wordpiece_{name}.json"), encoding="utf-8") as f:
        return json.load(f)


def unpack_spans(flat):
    """[gap, length, gap, length, ..] (gap: from the end of the span in front, or from 0) -> [(start, end), ..]"""
    out, pos = [], 0
    for gap, length in zip(flat[0::2], flat[1::2]):
        out.append((pos + gap, pos + gap + length))
        pos += gap + length
    return out


def pack_spans(spans):
    out, pos = [], 0
    for s, e in spans:
        out += [s - pos, e - s]
        pos = e
    return out


@functools.lru_cache(maxsize=None)
def model():
    """-> (vocab {bytes: id}, unk_id, max_chars, prefix)"""
    v = load("vocab")
    return {k.encode(): i for k, i in v["vocab"].items()}, v["unk_id"], v["max_input_chars_per_word"], v["prefix"]


@functools.lru_cache(maxsize=None)
def cases():
    """-> (docs as bytes, per document tokenizers' ids, its token byte spans and BertPreTokenizer's word byte spans)"""
    c = load("cases")
    return ([d.encode() for d in c["docs"]], c["ids"], [unpack_spans(x) for x in c["tok_spans"]], [unpack_spans(x) for x in c["word_spans"]])


# ---------------------------------------------------------------------------------------------------------- the definitions
def class_table(classes):
    """rows {first, last, cls} -> the class of every code point, the fixed ASCII classes included"""
    a = np.zeros(0x110000, dtype=np.uint8)
    for first, last, cls in np.asarray(classes).reshape(-1, 3).tolist():
        a[first:last + 1] = cls
    a[:0x80] = O
    a[ord("A"):ord("Z") + 1] = L
    a[ord("a"):ord("z") + 1] = L
    a[ord("0"):ord("9") + 1] = N
    a[0x09:0x0E] = S
    a[0x20] = S
    return a.tolist()


def units(d, table):
    """a document's units -> (at, cls): per unit its first byte and its class; a well-formed UTF-8 sequence (Unicode Table 3-7) inside the
    document is one unit, every other byte a unit of class O"""
    at, cls, i, n = [], [], 0, len(d)
    while i < n:
        b0 = d[i]
        k = 1
        if b0 < 0x80:
            c = table[b0]
        else:
            try:
                need = 2 if 0xC2 <= b0 <= 0xDF else 3 if 0xE0 <= b0 <= 0xEF else 4 if 0xF0 <= b0 <= 0xF4 else 0
                ch = bytes(d[i:i + need]).decode("utf-8") if need and i + need <= n else ""   # (strict: overlong forms and surrogates raise)
            except UnicodeDecodeError:
                ch = ""
            if len(ch) == 1:
                k, c = need, table[ord(ch)]
            else:
                c = O
        at.append(i)
        cls.append(c)
        i += k
    return at, cls


def bert_scan(doc, table):
    """Split.Bert, sequentially: -> [(start, end, is_space)] of the words of one document — a maximal run of S units, every O unit alone,
    a maximal run of L and N units"""
    d = bytes(doc)
    at, cls = units(d, table)
    at.append(len(d))
    words, i, n = [], 0, len(cls)
    while i < n:
        j = i + 1
        if cls[i] == S:
            while j < n and cls[j] == S:
                j += 1
        elif cls[i] != O:
            while j < n and cls[j] in (L, N):
                j += 1
        words.append((at[i], at[j], cls[i] == S))
        i = j
    return words


def bert_offsets(docs, table, base=0):
    """-> (word_offsets, doc_words, space flags) of a batch under Split.Bert, as daac_split_batch and daac_split_words_space define them"""
    wo, dw, sp, pos = [], [0], [], base
    for d in docs:
        for s, _, is_space in bert_scan(d, table):
            wo.append(pos + s)
            sp.append(int(is_space))
        dw.append(len(wo))
        pos += len(d)
    return np.array(wo + [pos], dtype=np.uint64), np.array(dw, dtype=np.uint64), np.array(sp, dtype=np.uint8)


def wordpiece(word, vocab, unk_id, max_chars, prefix=b"##", roles=True, shortest=False):
    """The definition for one word (bytes): -> [(id, start, end)].  `roles=False` merges the two piece sets, `shortest=True` takes the
    shortest piece first: the two wrong rules the fixtures can tell from the right one."""
    w = bytes(word)
    n = len(w)
    if not n:
        return []
    if sum((b & 0xC0) != 0x80 for b in w) > max_chars:
        return [(unk_id, 0, n)]
    out, p = [], 0
    while p < n:
        ends = range(p + 1, n + 1) if shortest else range(n, p, -1)
        for e in ends:
            piece = w[p:e]
            if roles:
                i = vocab.get(piece if p == 0 else prefix + piece)
            else:
                i = vocab.get(piece, vocab.get(prefix + piece))
            if i is not None:
                out.append((i, p, e))
                p = e
                break
        else:
            return [(unk_id, 0, n)]
    return out


def wordpiece_doc(doc, table, vocab, unk_id, max_chars, prefix=b"##"):
    """split, drop the whitespace words, segment -> (ids, spans relative to the document)"""
    ids, spans = [], []
    for s, e, is_space in bert_scan(doc, table):
        if is_space:
            continue
        for i, a, b in wordpiece(doc[s:e], vocab, unk_id, max_chars, prefix):
            ids.append(i)
            spans.append((s + a, s + b))
    return ids, spans


@functools.lru_cache(maxsize=None)
def distinct_words():
    """-> (the distinct non-whitespace words of the fixture documents, sorted; their ids and spans by the definition, which the generator
    has checked against `tokenizers`)"""
    docs, _, _, word_spans = cases()
    vocab, unk_id, max_chars, prefix = model()
    words = sorted({d[s:e] for d, ws in zip(docs, word_spans) for s, e in ws})
    return words, [wordpiece(w, vocab, unk_id, max_chars, prefix.encode()) for w in words]
