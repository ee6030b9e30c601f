"""Batches of many documents drawn from a small pool, and their expected results without a loop over the documents.  A plain helper: no
test lives here.

A batch call treats every document on its own, so the result of a batch whose documents are pool[idx[0]], pool[idx[1]], .. is the
per-document results of the pool in that order.  `pooled` draws idx and packs the bytes, the `ref_*` functions run the references the
suite already uses (the CPU oracle, the pure-Python definitions of the feature tests and of the *_golden helpers) once per pool document,
and `expand` lays their CSR results out for the whole batch with np.repeat and cumulative sums.  tests/test_batch_scale_host.py holds
`expand` and the packing against the plain per-document loop.  `high_window` puts a batch at a chosen position of a large device buffer
of which nothing else is initialised.  Nothing here calls the library for an expected value."""
import numpy as np

import normalize_golden as ng
import special_golden as sg
import wordpiece_golden as wg
from oracle import oracle as orc
from test_gpu_batch_hist import _Slots
from test_gpu_replace import _splice
from test_gpu_tokenize import _tokens
from test_gpu_tokenize_bpe import _bpe
from test_gpu_tokenize_unigram import _viterbi
from test_split_host import scan_batch as _scan_gpt2_batch
from test_split_o200k_host import scan_o200k_batch as _scan_o200k_batch
from test_split_rules_host import scan_rule_batch as _scan_rule_batch

import daachorse_amd as da
from daachorse_amd import Split

TURN = 4096 * 256   # items of one turn of the helper kernels whose grid is capped at 4096 blocks of 256 lanes
MAX_POOL = 256


def _b(d):
    return d.encode("utf-8") if isinstance(d, str) else bytes(d)


def pack(docs, base=0):
    """the plain packing of a list of documents -> (bytes as np.uint8, np.int64[n + 1] offsets that start at `base`)"""
    blobs = [_b(d) for d in docs]
    off = np.full(len(blobs) + 1, base, dtype=np.int64)
    off[1:] += np.cumsum([len(x) for x in blobs], dtype=np.int64)
    return np.frombuffer(b"".join(blobs), dtype=np.uint8).copy(), off


def expand(per_pool, idx):
    """per_pool = (offsets[P + 1], array, ..): a CSR result of the pool, document p's items are array[offsets[p] : offsets[p + 1]]
    -> (np.uint64[n + 1] offsets, array, ..) of the batch pool[idx[0]], pool[idx[1]], ..; np.repeat and cumulative sums only"""
    off = np.asarray(per_pool[0]).astype(np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    cnt = np.diff(off)[idx]
    new = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(cnt, out=new[1:])
    src = np.repeat(off[:-1][idx] - new[:-1], cnt) + np.arange(int(new[-1]), dtype=np.int64)
    return (new.astype(np.uint64),) + tuple(np.asarray(a)[src] for a in per_pool[1:])


def pack_idx(pool, idx):
    """the packing of the batch pool[idx[0]], pool[idx[1]], .. -> (bytes as np.uint8, np.int64[n + 1] offsets from 0), without a loop over idx"""
    blob, off = pack(pool)
    new, hay = expand((off, blob), idx)
    return hay, new.astype(np.int64)


def marks(n, turns=(TURN,)):
    """the documents a test pins: the first, the last, and those on either side of every turn boundary below n"""
    at = [0, n - 1] + [t + d for t in turns for d in (-1, 0, 1) if 0 <= t + d < n]
    return sorted(set(a for a in at if 0 <= a < n))


def pooled(pool, n, seed, pins=(), turns=(TURN,)):
    """n documents drawn from `pool` (at most 256 distinct documents) -> (idx, the packed bytes as np.uint8, np.int64[n + 1] offsets from
    0).  The documents at marks(n, turns) are the pool entries `pins` in turn (distinct, non-empty, result-bearing entries, the caller's
    choice), so that neighbours at a turn boundary differ in length and in result.  No Python loop over n."""
    assert 0 < len(pool) <= MAX_POOL and len({_b(d) for d in pool}) == len(pool), "a pool is at most 256 distinct documents"
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(pool), n).astype(np.int64)
    if pins and n:
        assert len(set(pins)) == len(pins) >= 3 and all(len(_b(pool[p])) for p in pins)
        at = marks(n, turns)
        idx[at] = np.array([pins[j % len(pins)] for j in range(len(at))], dtype=np.int64)
    return (idx,) + pack_idx(pool, idx)


def high_window(big, docs, base, front=b"\xe4", tail=b"\xe4"):
    """Writes a batch into the preallocated uint8 CUDA tensor `big` so that its first document begins at `base`; `docs` is a list of
    documents or (bytes as np.uint8, offsets from 0).  The 64 bytes in front of the window repeat `front` and the 64 behind it `tail`:
    bytes that would change the result if a kernel read them (a pattern's prefix, a special's prefix, a UTF-8 lead byte).  Nothing else
    of `big` is written.  -> (big, int64 CUDA offsets with offsets[0] = base)"""
    import torch
    hay, off = docs if isinstance(docs, tuple) else pack(docs)
    total = int(off[-1]) - int(off[0])
    assert base >= 64 and base + total + 64 <= big.numel() and len(hay) == total and len(front) and len(tail)
    f = (front * 64)[-64:]
    t = (tail * 64)[:64]
    win = np.concatenate([np.frombuffer(f, dtype=np.uint8), hay, np.frombuffer(t, dtype=np.uint8)])
    big[base - 64:base + total + 64] = torch.from_numpy(win).to(big.device)
    return big, torch.from_numpy(np.asarray(off, dtype=np.int64) - int(off[0]) + base).to(big.device)


# --------------------------------------------------------------------------------------------- the references, once per pool document
API = {da.ScanMode.FindOverlapping: "find_overlapping_iter", da.ScanMode.FindOverlappingNoSuffix: "find_overlapping_no_suffix_iter",
       da.ScanMode.Find: "find_iter", da.ScanMode.LeftmostFind: "leftmost_find_iter"}


def _csr(rows, width, dtype):
    """per document a list of `width`-tuples -> (offsets, one array per column)"""
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    a = np.array([t for r in rows for t in r], dtype=np.uint64).reshape(-1, width)
    return (off,) + tuple(a[:, j].astype(dtype[j]) for j in range(width))


def terminates(o, mode, doc):
    """False where the reference iterator does not terminate on `doc` (leftmost kinds with "" in the set): such a document is in no pool"""
    try:
        getattr(o, API[mode])(doc)
        return True
    except orc.OracleError as e:
        assert e.code == 6
        return False


def ref_scan(o, mode, pool):
    """the oracle's stream per pool document -> (counts u64[P], checksums u64[P], (offsets, start, end, value))"""
    ms = [getattr(o, API[mode])(d) for d in pool]
    counts = np.array([len(m) for m in ms], dtype=np.uint64)
    sums = np.array([orc.matches_checksum(m) for m in ms], dtype=np.uint64)
    rows = [list(zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist())) for m in ms]
    return counts, sums, _csr(rows, 3, (np.uint64, np.uint64, np.uint32))


def ref_hist(o, mode, pool):
    """the oracle's tuples binned by slot -> (offsets, slot u32, count u32)"""
    slots = _Slots(o)
    return _csr([slots.rows(getattr(o, API[mode])(d)) for d in pool], 2, (np.uint32, np.uint32))


def ref_replace(o, mode, pool, table):
    """the ten-line splice over the oracle's tuples -> (offsets, bytes u8)"""
    outs = [_splice(_b(d), getattr(o, API[mode])(d), [_b(r) for r in table]) for d in pool]
    blob, off = pack(outs)
    return off.astype(np.uint64), blob


def ref_matches(o, mode, pool):
    """-> the oracle's match count per pool document (u64[P])"""
    return np.array([len(getattr(o, API[mode])(d)) for d in pool], dtype=np.uint64)


def _tok_csr(toks):
    """per document (ids, spans[T, 2]) -> (offsets, ids u32, spans u64[T, 2])"""
    off = np.cumsum([0] + [len(i) for i, _ in toks]).astype(np.uint64)
    ids = np.concatenate([np.asarray(i, dtype=np.uint32).reshape(-1) for i, _ in toks] + [np.zeros(0, dtype=np.uint32)])
    spans = np.concatenate([np.asarray(s, dtype=np.uint64).reshape(-1, 2) for _, s in toks] + [np.zeros((0, 2), dtype=np.uint64)])
    return off, ids, spans


def _triples(t):
    return [x[0] for x in t], [x[1:] for x in t]


def ref_tokenize(o, mode, pool, gap, gap_id):
    """the restatement of tokenize over the oracle's tuples -> (offsets, ids, spans)"""
    return _tok_csr([_tokens(_b(d), getattr(o, API[mode])(d), gap, gap_id) for d in pool])


def ref_bpe(o, pool, ranks, gap, gap_id):
    """`_bpe` over the oracle's overlapping matches -> (offsets, ids, spans)"""
    return _tok_csr([_triples(_bpe(_b(d), o.find_overlapping_iter(d), ranks, gap, gap_id)) for d in pool])


def ref_unigram(o, pool, scores, unk, gap, gap_id):
    """the float32 lattice walk over the oracle's overlapping matches -> ((offsets, ids, spans), scores f32[P])"""
    scores, unk = np.asarray(scores, dtype=np.float32), np.float32(unk)
    res = [_viterbi(_b(d), o.find_overlapping_iter(d), scores, unk, gap, gap_id) for d in pool]
    return _tok_csr([_triples(t) for t, _ in res]), np.array([s for _, s in res], dtype=np.float32)


def ref_wordpiece(pool, vocab, unk_id, max_chars, skip=None):
    """the WordPiece walk per pool word; a word whose `skip` entry is non-zero yields nothing -> (offsets, ids, spans)"""
    toks = [wg.wordpiece(_b(w), vocab, unk_id, max_chars) for w in pool]
    if skip is not None:
        toks = [[] if s else t for s, t in zip(skip, toks)]
    return _tok_csr([_triples(t) for t in toks])


_CLASSES = {}


def _classes(rule):
    """the default classes of a rule, one object per rule (the scanners cache on the object's identity)"""
    if rule not in _CLASSES:
        _CLASSES[rule] = da.bert_char_classes() if rule == Split.Bert else da.o200k_char_classes() if rule == Split.O200k else da.char_classes()
    return _CLASSES[rule]


def split_scan_batch(docs, rule, base=0):
    """the sequential scanner of `rule` over a list of documents -> (word_offsets, doc_words), as the feature's own tests use it"""
    if rule in (Split.Whitespace, Split.Gpt2):
        return _scan_gpt2_batch(docs, rule, _classes(rule), base)
    if rule == Split.O200k:
        return _scan_o200k_batch(docs, _classes(rule), base)
    if rule == Split.Bert:
        return wg.bert_offsets(docs, wg.class_table(_classes(rule)), base)[:2]
    return _scan_rule_batch(docs, rule, _classes(rule), base)


def ref_split(pool, rule):
    """-> (offsets, word starts relative to the document u64, whitespace flag u8 of words_space): one scanner run per pool document"""
    table = wg.class_table(_classes(rule))
    rows = []
    for d in pool:
        d = _b(d)
        wo, _ = split_scan_batch([d], rule)
        starts = wo[:-1].tolist()
        rows.append([(s, int(wg.units(d[s:], table)[1][0] == wg.S)) for s in starts])
    return _csr(rows, 2, (np.uint64, np.uint8))


def expand_split(per_pool, idx, doc_offsets):
    """-> (word_offsets u64[n_words + 1] absolute in the batch's buffer, doc_words u64[n + 1], space flags u8[n_words])"""
    dw, rel, space = expand(per_pool, idx)
    doc_offsets = np.asarray(doc_offsets).astype(np.uint64)
    wo = np.empty(len(rel) + 1, dtype=np.uint64)
    wo[:-1] = rel + np.repeat(doc_offsets[:-1], np.diff(dw.astype(np.int64)))
    wo[-1] = doc_offsets[-1]
    return wo, dw, space


def ref_cut(pool, spec):
    """special_golden.cut per pool document -> (offsets, segment starts relative to the document u64, seg_values u32)"""
    rows = []
    for d in pool:
        so, _, sv = sg.cut([_b(d)], lambda x: sg.leftmost(x, spec))
        rows.append(list(zip(so[:-1].tolist(), sv.tolist())))
    return _csr(rows, 2, (np.uint64, np.uint32))


def expand_cut(per_pool, idx, doc_offsets):
    """-> (seg_offsets u64[n_segs + 1] absolute, doc_segs u64[n + 1], seg_values u32[n_segs])"""
    ds, rel, sv = expand(per_pool, idx)
    doc_offsets = np.asarray(doc_offsets).astype(np.uint64)
    so = np.empty(len(rel) + 1, dtype=np.uint64)
    so[:-1] = rel + np.repeat(doc_offsets[:-1], np.diff(ds.astype(np.int64)))
    so[-1] = doc_offsets[-1]
    return so, ds, sv


def ref_normalize(pool, image):
    """normalize_golden.scan per pool document -> ((offsets, bytes u8, src u32))"""
    outs = [ng.scan(_b(d), image) for d in pool]
    off = np.cumsum([0] + [len(o) for o, _ in outs]).astype(np.uint64)
    return off, np.frombuffer(b"".join(o for o, _ in outs), dtype=np.uint8), np.array([x for _, s in outs for x in s], dtype=np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the pools
BYTE_PATTERNS = [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", "é".encode(), "世".encode(), "世界".encode()]
CHAR_PATTERNS = ["a", "ab", "全世界", "世界", "に", "世", "é", "bé"]
# the empty document, one without a match, every length from 1 to 8, characters of two and three bytes, ill-formed bytes, all matches
BYTE_HAND = [b"", b"xyz", b"a", b"ab", b"abc", b"abca", b"xabcx", b"abcabc", b"bcabcab", b"abcxabca", "é".encode(), "aé".encode(),
             "世".encode(), "世界".encode(), "a世界b".encode(), b"a\xffb", b"\xe4\xb8", b"\xa9a", "xéy世".encode(), b"zz"]
CHAR_HAND = ["", "xyz", "a", "ab", "abx", "abab", "xabax", "ababab", "é", "aé", "世", "世界", "全世界", "a全世界b",
             "に世", "xéy世", "zz", "界", "abé", "全世"]
BYTE_LETTERS = [b"a", b"b", b"c", b"a", b"b", b"c", b"x", "é".encode(), "世".encode(), "界".encode(), b"\xff", b"\xe4"]
CHAR_LETTERS = ["a", "b", "a", "b", "x", "é", "全", "世", "界", "に"]


def make_pool(hand, letters, size, seed, max_letters=6, keep=None):
    """the hand-written documents, then seeded random ones of up to `max_letters` letters, distinct, `size` in all; `keep(doc)` False
    leaves a document out (one the reference refuses)"""
    rng = np.random.default_rng(seed)
    pool, seen = [], set()
    for d in hand:
        if _b(d) not in seen and (keep is None or keep(d)):
            seen.add(_b(d))
            pool.append(d)
    while len(pool) < size:
        d = type(hand[0])().join(letters[i] for i in rng.integers(0, len(letters), int(rng.integers(1, max_letters + 1))).tolist())
        if _b(d) not in seen and (keep is None or keep(d)):
            seen.add(_b(d))
            pool.append(d)
    assert len(pool) <= MAX_POOL
    return pool


def pins_of(per_pool_counts, pool, k=5):
    """k pool entries that are not empty, bear a result and differ from one another in length or in count, in pool order"""
    out, seen = [], set()
    for p, c in enumerate(np.asarray(per_pool_counts).tolist()):
        key = (len(_b(pool[p])), c)
        if c and len(_b(pool[p])) and key not in seen:
            seen.add(key)
            out.append(p)
        if len(out) == k:
            return out
    raise AssertionError("the pool has too few distinct result-bearing documents")


# words for tokenize_wordpiece_batch over the hand vocabulary of tests/test_gpu_tokenize_wordpiece.py, with max_chars = 6: several
# pieces, one piece, the whole word unknown, more characters than the cap, an ill-formed byte
WORD_HAND = [b"", b"zzz", b"a", b"ab", b"abc", b"abab", b"unabl", b"unable", b"unables", b"abcababs", "é".encode(), "aé".encode(), "、".encode(), b"!",
             b"aaaaaaa", b"a\xffb", "abé".encode(), b"abs", b"s", b"ables", b"abcabs"]
WORD_LETTERS = [b"a", b"b", b"c", b"s", b"un", b"able", b"ab", "é".encode(), "、".encode(), b"!", b"z", b"\xff"]
# documents for the split rules and the chains behind them
TEXT_HAND = [b"", b"   ", b"a", b"it", b"a b", b"it's", b" we'l", b"we'll ", b"123abc ", b"x\n\n y12", "é漢 ٣".encode(), b"!?", b"a\xff b", b"\xe6\xbc", b"unable ab",
             "É　abc".encode(), b" ", b"1234567", b"ab!abc", b"abc  \n"]
TEXT_LETTERS = [b" ", b" ", b"  ", b"\n", b"a", b"B", b"cd", b"'s", b"'ll", b"1", b"23", b"!", "é".encode(), "漢".encode(), "　".encode(), b"\xff", "٣".encode(),
                "É".encode(), b"un", b"able", b"ab", b"abc"]
# documents around the special tokens <|e|>, <|end|> and <|
SPECIAL_HAND = [b"", b"ab", b"a<|e|>b", b"<|e|>", b"<|e|><|e|>", b"<|end|>x", b"<|", b"x<|en", "é<|e|>世".encode(), b"a\xff", b"a", b"abc", b"abca", b"abcab", b"abcabc",
                b"abcabca", b"abcabcab", b"<", b"|>a<", b"a<|e|"]
SPECIAL_LETTERS = [b"a", b"b", b"c", b"<|e|>", b"<|end|>", b"<|", b"<", b"|>", "é".encode(), "世".encode(), b"\xff"]
# documents for BERT's normalizer: lowercased, accents stripped, padded, decomposed, deleted, copied
NORM_HAND = [b"", b"xyz", b"A", b"Ab", "É".encode(), "中".encode(), "\U00020000".encode(), "한".encode(), b"\0", "‍".encode(), b"a\xffB", b"\xe4\xb8", b"AbCd", b"AbCdE",
             "aÉb中".encode(), b"A\tb c d", b"ABCDEFGH", "\0‍".encode(), "ü한".encode(), b"q\0Q", b"AbCdEf"]
NORM_LETTERS = [b"A", b"b", "É".encode(), "中".encode(), "한".encode(), b"\0", b" ", b"\t", b"\xff", b"\xe4", "ü".encode(), b"z"]


# ------------------------------------------------------------------------------------------- the chains, once per pool document
def _per_doc(pool, text, spec):
    """per pool document `text(bytes)` -> (ids, spans); with `spec` ([(bytes, id)]) around the special tokens, by
    special_golden.tokenize_docs (cut, text on every text segment, splice)"""
    if spec is None:
        return [text(_b(d)) for d in pool]
    return [sg.tokenize_docs([_b(d)], lambda x: sg.leftmost(x, spec), text)[0] for d in pool]


def ref_bpe_docs(o, pool, rule, ranks, gap, gap_id, spec=None):
    """tokenize_bpe_docs by its definition: the rule's scanner cuts the text into words, `_bpe` runs on every word, spans count from the
    document -> (offsets, ids, spans)"""
    def text(seg):
        ids, spans = [], []
        wo = split_scan_batch([seg], rule)[0].tolist()
        for s, e in zip(wo, wo[1:]):
            for i, a, b in _bpe(seg[s:e], o.find_overlapping_iter(seg[s:e]), ranks, gap, gap_id):
                ids.append(i)
                spans.append((s + a, s + b))
        return ids, spans
    return _tok_csr(_per_doc(pool, text, spec))


def ref_wordpiece_docs(pool, vocab, unk_id, max_chars, image=None, spec=None):
    """tokenize_wordpiece_docs by its definition: the normalizer's scanner where `image` is given, Split.Bert's scanner, the WordPiece
    walk on every word that is not whitespace, spans back to the raw text -> (offsets, ids, spans)"""
    table = wg.class_table(_classes(Split.Bert))

    def text(seg):
        if image is None:
            return wg.wordpiece_doc(seg, table, vocab, unk_id, max_chars)
        out, src = ng.scan(seg, image)
        ids, spans = wg.wordpiece_doc(out, table, vocab, unk_id, max_chars)
        return ids, ng.spans_to_source(spans, src, seg)
    return _tok_csr(_per_doc(pool, text, spec))
