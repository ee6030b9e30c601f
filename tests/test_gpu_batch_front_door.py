"""The batch calls' common contract, call by call (include/daachorse_amd.h, "batches"): what every call that takes (hay, offsets, n,
hay_is_device) does with no document, with empty documents, with bytes in front of offsets[0], with offsets that decrease and with a
NULL text, for host and for device batches, and that a single haystack is a batch of one document.

Every batch is handed to the C call as the caller of the C ABI would hand it over: `_Raw` stands in for the package's `_Batch`, so a host
batch may start at offsets[0] != 0, decrease or come without a text.  Expected values come from the references of the neighbouring
modules (the CPU oracle, the token / splice / BPE / Viterbi definitions, the sequential split scanner, wordpiece_golden,
normalize_golden, special_golden), applied to one document at a time, never from a batch call.

Asserted elsewhere and not repeated: decreasing device offsets for split_batch and normalize_batch
(test_decreasing_device_offsets_answer_1 in test_gpu_split.py and test_gpu_normalize.py).  Not rebuilt small: the length limits of
unigram and wordpiece, which take a document of 2^32 - 1 bytes (host offsets: test_tokenize_wordpiece_host.py)."""
import numpy as np
import pytest
import torch

import normalize_golden as ng
import special_golden as sg
import wordpiece_golden as wg
from oracle import oracle as orc
from test_gpu_batch_hist import _Slots
from test_gpu_replace import _splice
from test_gpu_streams import _csr, _plain, _sev, _tok_lists
from test_gpu_tokenize import _tokens
from test_gpu_tokenize_bpe import _bpe
from test_gpu_tokenize_unigram import _viterbi
from test_split_host import scan_batch as split_scan_batch

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, ScanMode, Split, bytewise

GID = 0x10000
PATS = [b"ab", b"bc", b"abc", b"ca", b"bb"]
TABLE = [b"<%d>" % i for i in range(len(PATS))]
SCORES = np.array([-(1.0 + 0.37 * i) for i in range(len(PATS))], dtype=np.float32)
UNK_SCORE = -4.25
SPECIALS = [(b"ab", 7), (b"bca", 9)]
VOCAB = {b"[UNK]": 0, b"a": 1, b"##a": 2, b"b": 3, b"##b": 4, b"c": 5, b"##c": 6, b"ab": 7, b"##ab": 8, b"bc": 9, b"##ca": 10, b"cab": 11}
OV = ScanMode.FindOverlapping
# three bytes that belong to no document: "b" in front of a document that begins with "c" or "b" reads bc / bb, continues a word of
# the splitter and of WordPiece, and shifts every position if it were counted
FRONT = b"bbb"
DOCS = [b"cab c", b"bca", b"abcab", b" bc"]
EMPTIES = [b"", b"cab c", b"", b"bcabc", b""]


class _Raw:
    """what the wrappers read of a batch argument"""

    def __init__(self, hay, off, n, is_device, keep):
        self.hay, self.off, self.n, self.is_device, self.keep = hay, off, n, is_device, keep


@pytest.fixture(autouse=True)
def _raw_batches(monkeypatch):
    made = bytewise._Batch
    monkeypatch.setattr(bytewise, "_Batch", lambda docs: docs if isinstance(docs, _Raw) else made(docs))


def _raw(hay, offsets, device, null_hay=False):
    off = np.asarray(offsets, dtype=np.uint64)
    buf = np.frombuffer(hay or b"\0", dtype=np.uint8).copy()
    if device:
        h, o = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        return _Raw(None if null_hay else h.data_ptr(), o.data_ptr(), len(off) - 1, 1, (h, o))
    return _Raw(None if null_hay else buf.ctypes.data, off.ctypes.data, len(off) - 1, 0, (buf, off))


def _batch(docs, device, front=b""):
    off = len(front) + np.cumsum([0] + [len(d) for d in docs])
    return _raw(front + b"".join(docs), off, device)


class _World:
    def __init__(self):
        self.o = orc.OraclePma.build(PATS)
        self.p, rest = da.DoubleArrayAhoCorasick.deserialize(self.o.serialize())
        assert rest == b""
        self.slots = _Slots(self.o)
        patterns, self.first, self.cont = da.wordpiece_tables(VOCAB)
        self.wp = da.DoubleArrayAhoCorasick.new(patterns)
        self.cc = da.char_classes()
        self.splitter = da.Splitter(Split.Gpt2)
        self.nz = da.bert_normalizer()
        self.special = da.SpecialTokens(SPECIALS)


@pytest.fixture(scope="module")
def world():
    return _World()


def _normalize_want(docs):
    res = [ng.bert_scan(d, ng.OPTIONS["default"]) for d in docs]
    return [list(b"".join(o for o, _ in res)), np.cumsum([0] + [len(o) for o, _ in res]).tolist(), [x for _, sr in res for x in sr]]


def _unigram_want(w, docs):
    res = [_viterbi(d, w.o.find_overlapping_iter(d), SCORES, np.float32(UNK_SCORE), Gap.Chars, GID) for d in docs]
    return _tok_lists([t for t, _ in res]) + [[_plain(sc) for _, sc in res]]


def _tokenize_want(w, docs):
    per_doc = []
    for d in docs:
        ids, sp = _tokens(d, w.o.find_iter(d), Gap.Chars, GID)
        per_doc.append([(i, a, b) for i, (a, b) in zip(ids.tolist(), sp.tolist())])
    return _tok_lists(per_doc)


# name -> (call(w, batch) -> plain values, want(w, docs, base) -> the same from one document at a time)
CALLS = {
    "count_batch": (lambda w, b: w.p.count_batch(OV, b).tolist(), lambda w, docs, base: [len(w.o.find_overlapping_iter(d)) for d in docs]),
    "scan_batch": (lambda w, b: _plain(w.p.scan_batch(OV, b)), lambda w, docs, base: list(_csr([_sev(w.o.find_overlapping_iter(d)) for d in docs]))),
    "histogram_batch": (lambda w, b: _plain(w.p.histogram_batch(OV, b)),
                        lambda w, docs, base: list(_csr([w.slots.rows(w.o.find_overlapping_iter(d)) for d in docs]))),
    "tokenize_batch": (lambda w, b: _plain(w.p.tokenize_batch(b, gap=Gap.Chars, gap_id=GID, spans=True)), lambda w, docs, base: _tokenize_want(w, docs)),
    "replace_all_batch": (lambda w, b: w.p.replace_all_batch(b, TABLE), lambda w, docs, base: [_splice(d, w.o.find_iter(d), TABLE) for d in docs]),
    "tokenize_unigram_batch": (lambda w, b: _plain(w.p.tokenize_unigram_batch(b, SCORES, UNK_SCORE, gap=Gap.Chars, gap_id=GID, spans=True, doc_scores=True)),
                               lambda w, docs, base: _unigram_want(w, docs)),
    "tokenize_bpe_batch": (lambda w, b: _plain(w.p.tokenize_bpe_batch(b, gap=Gap.Bytes, gap_id=GID, spans=True)),
                           lambda w, docs, base: _tok_lists([_bpe(d, w.o.find_overlapping_iter(d), None, Gap.Bytes, GID) for d in docs])),
    "tokenize_wordpiece_batch": (lambda w, b: _plain(w.wp.tokenize_wordpiece_batch(b, w.first, w.cont, 0, spans=True)),
                                 lambda w, docs, base: _tok_lists([wg.wordpiece(d, VOCAB, 0, 100) for d in docs])),
    "split_batch": (lambda w, b: _plain(w.splitter.split_batch(b)), lambda w, docs, base: [x.tolist() for x in split_scan_batch(docs, Split.Gpt2, w.cc, base)]),
    "normalize_batch": (lambda w, b: _plain(w.nz.normalize_batch(b, src=True)), lambda w, docs, base: _normalize_want(docs)),
    "cut_batch": (lambda w, b: _plain(w.special.cut_batch(b)), lambda w, docs, base: [x.tolist() for x in sg.cut(docs, lambda d: sg.leftmost(d, SPECIALS), base)]),
}
NAMES = sorted(CALLS)
PLACES = ["host", "device"]
VALIDATED = ("split_batch", "normalize_batch")   # device offsets checked by a kernel of their own: see the module's docstring


def _refused(w, name, b):
    with pytest.raises(da.DaachorseError) as ei:
        CALLS[name][0](w, b)
    return ei.value.code, str(ei.value)


# --------------------------------------------------------------------------------------------------------------- results
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_no_document(world, name, place):
    """n == 0: every list is empty and every offsets array is the one entry 0"""
    call, want = CALLS[name]
    got = call(world, _raw(FRONT, [0], place == "device"))
    assert got == want(world, [], 0)
    assert all(x in ([], [0]) for x in got), got


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_three_empty_documents(world, name, place):
    call, want = CALLS[name]
    assert call(world, _batch([b"", b"", b""], place == "device")) == want(world, [b"", b"", b""], 0)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_bytes_in_front_of_the_first_offset_belong_to_no_document(world, name, place):
    call, want = CALLS[name]
    across = world.o.find_overlapping_iter(FRONT + DOCS[0])
    assert np.any((across["start"] < len(FRONT)) & (across["end"] > len(FRONT))), "the front would match if it were read"
    assert call(world, _batch(DOCS, place == "device", FRONT)) == want(world, DOCS, len(FRONT))
    if name not in ("split_batch", "cut_batch"):   # (their positions are the buffer's): the batch without the front
        assert want(world, DOCS, len(FRONT)) == want(world, DOCS, 0)
        assert call(world, _batch(DOCS, place == "device")) == want(world, DOCS, 0)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_empty_documents_first_last_and_in_between(world, name, place):
    call, want = CALLS[name]
    assert call(world, _batch(EMPTIES, place == "device")) == want(world, EMPTIES, 0)


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_a_decreasing_pair_answers_1(world, name, place):
    if place == "device" and name in VALIDATED:
        return   # test_decreasing_device_offsets_answer_1 of test_gpu_split.py / test_gpu_normalize.py
    code, msg = _refused(world, name, _raw(b"abcab" * 4, [0, 10, 5, 20], place == "device"))
    assert code == 1 and "decrease" in msg, msg
    assert place == "device" or "document 1" in msg, msg


@pytest.mark.parametrize("name", NAMES)
def test_device_offsets_that_end_before_they_begin_answer_1(world, name):
    code, msg = _refused(world, name, _raw(b"abcab" * 4, [10, 12, 5], True))
    assert code == 1 and "decrease" in msg, msg


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", NAMES)
def test_no_text_with_bytes_to_read_answers_1(world, name, place):
    code, msg = _refused(world, name, _raw(b"abca", [0, 4], place == "device", null_hay=True))
    assert code == 1 and "hay is NULL" in msg, msg


@pytest.fixture(scope="module")
def short_bpe():
    """a handle whose bpe_doc_max is 64"""
    p = da.DoubleArrayAhoCorasick.new(PATS)
    p.set_option("bpe_doc_max", 64)
    return p


@pytest.mark.parametrize("place", PLACES)
def test_bpe_document_above_bpe_doc_max_answers_6(short_bpe, place):
    with pytest.raises(da.DaachorseError) as ei:
        short_bpe.tokenize_bpe_batch(_batch([b"ab", b"c", b"abc" * 33 + b"a"], place == "device"))
    assert ei.value.code == 6 and "document 2" in str(ei.value) and "100 bytes" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("place", PLACES)
def test_bpe_decreasing_pair_comes_before_the_long_document(short_bpe, place):
    with pytest.raises(da.DaachorseError) as ei:
        short_bpe.tokenize_bpe_batch(_raw(b"abc" * 35, [0, 10, 5, 105], place == "device"))
    assert ei.value.code == 1 and "decrease" in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------------------- one haystack is a batch of one
def _tok_want(toks):
    return [[t[0] for t in toks], [[t[1], t[2]] for t in toks]]


def _unigram_one(w, d):
    toks, score = _viterbi(d, w.o.find_overlapping_iter(d), SCORES, np.float32(UNK_SCORE), Gap.Chars, GID)
    return _tok_want(toks) + [_plain(score)]


# name -> (one haystack, the batch call's answer cut down to the same values, want(w, document))
SINGLES = {
    "tokenize_bpe": (lambda w, h: _plain(w.p.tokenize_bpe(h, gap=Gap.Bytes, gap_id=GID, spans=True)),
                     lambda w, b: CALLS["tokenize_bpe_batch"][0](w, b)[:2], lambda w, d: _tok_want(_bpe(d, w.o.find_overlapping_iter(d), None, Gap.Bytes, GID))),
    "tokenize_unigram": (lambda w, h: _plain(w.p.tokenize_unigram(h, SCORES, UNK_SCORE, gap=Gap.Chars, gap_id=GID, spans=True)),
                         lambda w, b: (lambda r: r[:2] + [r[3][0]])(CALLS["tokenize_unigram_batch"][0](w, b)), _unigram_one),
    "tokenize_wordpiece": (lambda w, h: _plain(w.wp.tokenize_wordpiece(h, w.first, w.cont, 0, spans=True)),
                           lambda w, b: CALLS["tokenize_wordpiece_batch"][0](w, b)[:2], lambda w, d: _tok_want(wg.wordpiece(d, VOCAB, 0, 100))),
    "split": (lambda w, h: _plain(w.splitter.split(h)), lambda w, b: CALLS["split_batch"][0](w, b)[0],
              lambda w, d: split_scan_batch([d], Split.Gpt2, w.cc, 0)[0].tolist()),
    "normalize": (lambda w, h: _plain(w.nz.normalize(h, src=True)), lambda w, b: (lambda r: [r[0], r[2]])(CALLS["normalize_batch"][0](w, b)),
                  lambda w, d: (lambda r: [r[0], r[2]])(_normalize_want([d]))),
}


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("hay", [b"", b"cab c"])
@pytest.mark.parametrize("name", sorted(SINGLES))
def test_one_haystack_is_a_batch_of_one(world, name, hay, place):
    one, as_batch, want = SINGLES[name]
    h = torch.from_numpy(np.frombuffer(hay, dtype=np.uint8).copy()).cuda() if place == "device" else hay
    w = want(world, hay)
    assert one(world, h) == w
    assert as_batch(world, _batch([hay], place == "device")) == w
