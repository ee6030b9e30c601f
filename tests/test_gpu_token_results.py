"""What the token calls do with their result (include/daachorse_amd.h: daac_tokenize, daac_tokenize_bpe, daac_tokenize_unigram,
daac_tokenize_wordpiece, each with its _batch, and daac_tokens_splice): the edge of max_result_bytes with and without spans, what a
refused call leaves in the caller's out-arguments, what a call with nothing to return hands out, and the optional outs.

Every tokenizer call goes through the C ABI as its caller would make it (`_invoke`), so that the out-arguments can be preset and read as
they are; the splice goes through SpecialTokens / splice_special and the raw call.  Expected values come from the definitions of the
neighbouring modules (_tokens, _bpe, _viterbi, wordpiece_golden, special_golden), one document at a time, never from a call.

The option also limits the tuple list the calls are made of (24 bytes a tuple for a single haystack, 16 for a batch, another message)
and the splice's doc_tok (8 bytes a document and one more): the texts are mostly gap (one "ab" among bytes the dictionary lacks), and
WordPiece's words are of letters its vocabulary lacks (one unk_id each, no match), so that the token list is the larger by the
definitions' own counts, which every test asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import special_golden as sg
import wordpiece_golden as wg
from oracle import oracle as orc
from test_gpu_batch_front_door import GID, PATS, SCORES, SPECIALS, UNK_SCORE, VOCAB
from test_gpu_streams import _plain, _tok_lists
from test_gpu_tokenize import _tokens
from test_gpu_tokenize_bpe import _bpe
from test_gpu_tokenize_unigram import _viterbi

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap, ScanMode, _ffi
from daachorse_amd.bytewise import SPAN_DTYPE, DeviceMatches, DeviceOffsets

NAMES = ["tokenize", "bpe", "unigram", "wordpiece"]
PLACES = ["host", "device"]
TEXT = b"ab" + b"x" * 60
DOCS = [b"ab" + b"x" * 20, b"", b"y" * 30]
WORD = b"xyz"
WORDS = [b"xx", b"yyy", b"", b"z"]
DEFAULT_MAX = 8 << 30
assert not set(WORD + b"".join(WORDS)) & set(b"".join(VOCAB)), "a word of letters the vocabulary has would match"


class _World:
    def __init__(self):
        self.o = orc.OraclePma.build(PATS)
        self.p, rest = da.DoubleArrayAhoCorasick.deserialize(self.o.serialize())
        assert rest == b""
        patterns, self.first, self.cont = da.wordpiece_tables(VOCAB)
        self.wp = da.DoubleArrayAhoCorasick.new(patterns)
        self.special = da.SpecialTokens(SPECIALS)

    def handle(self, name):
        return self.wp if name == "wordpiece" else self.p


@pytest.fixture(scope="module")
def world():
    return _World()


def _docs(name, batch):
    if name == "wordpiece":
        return WORDS if batch else [WORD]
    return DOCS if batch else [TEXT]


def _want(w, name, docs):
    """-> ([ids, spans, offsets] of the definition, its match count, the documents' scores as bits (unigram) or None)"""
    per_doc, k, scores = [], 0, None
    for d in docs:
        if name == "tokenize":
            m = w.o.find_iter(d)
            ids, sp = _tokens(d, m, Gap.Bytes, GID)
            toks = [(i, a, b) for i, (a, b) in zip(ids.tolist(), sp.tolist())]
        elif name == "bpe":
            m = w.o.find_overlapping_iter(d)
            toks = _bpe(d, m, None, Gap.Bytes, GID)
        elif name == "unigram":
            m = w.o.find_overlapping_iter(d)
            toks, score = _viterbi(d, m, SCORES, np.float32(UNK_SCORE), Gap.Chars, GID)
            scores = (scores or []) + [_plain(np.float32(score))]
        else:
            m = []   # (the module's assertion on WORD and WORDS)
            toks = wg.wordpiece(d, VOCAB, 0, 100)
        per_doc.append([tuple(int(x) for x in t) for t in toks])
        k += len(m)
    return _tok_lists(per_doc), k, scores


def _text(docs, batch, device):
    """-> (the call's text arguments, what keeps them alive)"""
    buf = np.frombuffer(b"".join(docs) or b"\0", dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    if device:
        h, o = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        hp, op = h.data_ptr(), o.data_ptr()
    else:
        h, o = buf, off
        hp, op = buf.ctypes.data, off.ctypes.data
    return ((hp, op, len(docs), int(device)) if batch else (hp, len(docs[0]), int(device))), (h, o)


class _Outs:
    """the out-arguments of a token call; `preset`: non-zero in every one of them"""

    def __init__(self, preset=False):
        p = 0xDEAD0 if preset else None
        self.ids, self.sp, self.offs, self.ds = C.c_void_p(p), C.c_void_p(p), C.c_void_p(p), C.c_void_p(p)
        self.n, self.k, self.score = C.c_uint64(77 if preset else 0), C.c_uint64(77 if preset else 0), C.c_float(1.5 if preset else 0.0)

    def cleared(self, batch, spans, doc_scores=False):
        ptrs = [self.ids] + [self.sp] * bool(spans) + [self.offs] * bool(batch) + [self.ds] * bool(doc_scores)
        return all(not p.value for p in ptrs) and self.n.value == 0 and self.k.value == 0

    def read(self, n_docs, batch, spans):
        """-> [ids, spans?, offsets?] as plain lists; the buffers are freed"""
        out = [DeviceMatches(self.ids.value, self.n.value, np.dtype(np.uint32))]
        if spans:
            out.append(DeviceMatches(self.sp.value, self.n.value, SPAN_DTYPE))
        if batch:
            out.append(DeviceOffsets(self.offs.value, n_docs + 1))
        try:
            return [_plain(x.to_numpy()) for x in out]
        finally:
            for x in out:
                x.free()


def _invoke(w, name, batch, text, spans, o, doc_scores=False, skip=None):
    """the C call -> its status"""
    h = w.handle(name)._h
    fn = getattr(_ffi.lib(), "daac_tokenize" + ("" if name == "tokenize" else "_" + name) + ("_batch" if batch else ""))
    head = (h, int(ScanMode.Find), int(Engine.Auto)) if name == "tokenize" else (h, int(Engine.Auto))
    mid = {"tokenize": (int(Gap.Bytes), GID), "bpe": (None, 0, int(Gap.Bytes), GID),
           "unigram": (SCORES.ctypes.data, SCORES.size, C.c_float(UNK_SCORE), int(Gap.Chars), GID),
           "wordpiece": (w.first.ctypes.data, w.cont.ctypes.data, w.first.size, 0, 100)}[name]
    if name == "wordpiece" and batch:
        mid += (skip,)
    outs = [C.byref(o.ids), C.byref(o.sp) if spans else None]
    if batch:
        outs.append(C.byref(o.offs))
        if name == "unigram":
            outs.append(C.byref(o.ds) if doc_scores else None)
    outs += [C.byref(o.n), C.byref(o.k)]
    if name == "unigram" and not batch:
        outs.append(C.byref(o.score))
    return fn(*head, *text, None, *mid, *outs)


def _error():
    return _ffi.lib().daac_last_error().decode()


def _line(name, n_docs):
    return "tokenize matches=0 tokens=0 " if name == "tokenize" else "%s docs=%d matches=0 tokens=0 " % (name, n_docs)


# ------------------------------------------------------------------- 1, 2, 4. the limit's edge, a refused call's outs, the optional outs
@pytest.mark.parametrize("spans", [False, True])
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_the_edge_of_max_result_bytes_and_the_outs_of_a_refused_call(world, name, batch, place, spans):
    docs = _docs(name, batch)
    want, k, scores = _want(world, name, docs)
    t, per = len(want[0]), 20 if spans else 4
    assert t and 24 * k < 4 * t, "the tuple list would be refused first"
    want = [want[0]] + [want[1]] * spans + [want[2]] * batch
    text, keep = _text(docs, batch, place == "device")
    ds = name == "unigram" and batch
    h = world.handle(name)
    try:
        h.set_option("max_result_bytes", t * per)   # (spans=False: no span counts, 4 bytes a token hold the result)
        o = _Outs()
        assert _invoke(world, name, batch, text, spans, o, doc_scores=ds) == 0, _error()
        assert (o.n.value, o.k.value) == (t, k)
        if ds:
            dm = DeviceMatches(o.ds.value, len(docs), np.dtype(np.float32))
            assert _plain(dm.to_numpy()) == scores
            dm.free()
        elif name == "unigram":
            assert [_plain(np.float32(o.score.value))] == scores
        assert o.read(len(docs), batch, spans) == want
        h.set_option("max_result_bytes", t * per - 1)
        o = _Outs(preset=True)
        assert _invoke(world, name, batch, text, spans, o, doc_scores=ds) == 2
        assert "%d tokens" % t in _error() and "max_result_bytes" in _error(), _error()
        assert o.cleared(batch, spans, ds), "a refused call leaves NULL in every pointer and 0 in both counts"
    finally:
        h.set_option("max_result_bytes")


# ------------------------------------------------------------------------------------------------------- 3. nothing to return
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES + ["wordpiece skipped"])
def test_a_batch_without_a_token(world, name, place):
    """three empty documents, and three words that are skipped: no ids, no spans, n + 1 zeros, and the line of the call"""
    docs, skip = [b"", b"", b""], None
    if name == "wordpiece skipped":
        name, docs, skip = "wordpiece", [b"xx", b"y", b"zz"], torch.ones(3, dtype=torch.uint8, device="cuda")
    text, keep = _text(docs, True, place == "device")
    o = _Outs(preset=True)
    assert _invoke(world, name, True, text, True, o, skip=skip.data_ptr() if skip is not None else None) == 0, _error()
    assert da.last_kernel().startswith(_line(name, 3)), da.last_kernel()
    assert not o.ids.value and not o.sp.value and o.offs.value and (o.n.value, o.k.value) == (0, 0)
    assert o.read(3, True, True) == [[], [], [0, 0, 0, 0]]


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_the_empty_haystack(world, name, place):
    text, keep = _text([b""], False, place == "device")
    o = _Outs(preset=True)
    assert _invoke(world, name, False, text, True, o) == 0, _error()
    assert not o.ids.value and not o.sp.value and (o.n.value, o.k.value) == (0, 0)
    assert da.last_kernel().startswith(_line(name, 1)), da.last_kernel()
    if name == "unigram":
        assert o.score.value == 0.0


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_no_document(world, name, place):
    text, keep = _text([], True, place == "device")
    o = _Outs(preset=True)
    assert _invoke(world, name, True, text, True, o, doc_scores=True) == 0, _error()
    assert da.last_kernel().startswith(_line(name, 0)), da.last_kernel()
    assert not o.ids.value and not o.sp.value and not (name == "unigram" and o.ds.value) and (o.n.value, o.k.value) == (0, 0)
    assert o.read(0, True, True) == [[], [], [0]]


# ------------------------------------------------------------------------------------------------------------- the splice
@pytest.fixture(scope="module")
def spliced(world):
    """DOCS with specials in them, cut, tokenized per segment and left on the device; what the definition splices of them"""
    docs = [b"ab" + b"x" * 30, b"", b"xbca" + b"y" * 20 + b"ab"]
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    batch = (torch.from_numpy(np.frombuffer(b"".join(docs), dtype=np.uint8).copy()).cuda(), torch.from_numpy(off).cuda())

    def text(seg):
        ids, sp = _tokens(seg, world.o.find_iter(seg), Gap.Bytes, GID)
        return ids.tolist(), [tuple(x) for x in sp.tolist()]

    per_doc = sg.tokenize_docs(docs, lambda d: sg.leftmost(d, SPECIALS), text)
    want = _tok_lists([[(i, a, b) for i, (a, b) in zip(ids, sp)] for ids, sp in per_doc])
    cut = world.special.cut_batch(batch, device=True)
    ids, spans, seg_tok = world.p.tokenize_batch((batch[0], cut[0]), gap=Gap.Bytes, gap_id=GID, spans=True, device=True)
    yield dict(n=len(docs), batch=batch, cut=cut, ids=ids, spans=spans, seg_tok=seg_tok, want=want)
    for x in (ids, spans, seg_tok) + tuple(cut):
        x.free()


@pytest.mark.parametrize("with_spans", [False, True])
def test_splice_at_the_edge_of_max_result_bytes(spliced, with_spans):
    s = spliced
    t, per = len(s["want"][0]), 20 if with_spans else 4
    assert t and 8 * (s["n"] + 1) <= 4 * t, "doc_tok would be refused first"
    want = [s["want"][0]] + [s["want"][1]] * with_spans + [s["want"][2]]
    spans = s["spans"] if with_spans else None
    try:
        da.set_option("max_result_bytes", t * per)
        assert _plain(da.splice_special(s["ids"], spans, s["seg_tok"], s["cut"], s["batch"])) == want
        assert da.last_kernel() == "splice docs=%d segs=%d tokens=%d" % (s["n"], s["cut"][2].count, t)
        da.set_option("max_result_bytes", t * per - 1)
        with pytest.raises(da.DaachorseError) as ei:
            da.splice_special(s["ids"], spans, s["seg_tok"], s["cut"], s["batch"])
        assert ei.value.code == 2 and "%d tokens" % t in str(ei.value) and "max_result_bytes" in str(ei.value), str(ei.value)
        o = _Outs(preset=True)
        st = _ffi.lib().daac_tokens_splice(s["ids"].ptr, spans.ptr if with_spans else None, s["seg_tok"].ptr, s["cut"][2].ptr, s["cut"][0].ptr,
                                           s["cut"][1].ptr, s["batch"][1].data_ptr(), s["cut"][2].count, s["n"], None, C.byref(o.ids),
                                           C.byref(o.sp) if with_spans else None, C.byref(o.offs), C.byref(o.n))
        assert st == 2 and "%d tokens" % t in _error(), _error()
        o.k.value = 0   # (the splice has no match count)
        assert o.cleared(True, with_spans)
    finally:
        da.set_option("max_result_bytes", DEFAULT_MAX)
