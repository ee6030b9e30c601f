"""Split.Bert and daac_split_words_space on the MI355X.  Expected words come from the pure-Python sequential scanner of
tests/wordpiece_golden.py (`bert_scan`, which the fixture generator checked against `tokenizers`' BertPreTokenizer on every fixture
document) with bert_char_classes(), and from the fixture's own word spans; never from the library.  The rules that existed before are
run on the same inputs against the scanner of tests/test_split_host.py.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from test_split_host import scan_batch
from test_split_rules_host import scan_rule_batch
import wordpiece_golden as wg

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Split

COMMA = "、".encode()   # IDEOGRAPHIC COMMA: punctuation of three bytes
NBSP, WIDE_SPACE = " ".encode(), "　".encode()


@pytest.fixture(scope="module")
def table():
    return wg.class_table(da.bert_char_classes())


@pytest.fixture(scope="module")
def bert():
    return da.Splitter(Split.Bert, da.bert_char_classes())


def _device_batch(docs, front=0, fill=b"\xe3"):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    off = np.full(len(docs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(fill * front + b"".join(docs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _check(bert, table, docs, front=2, what=None):
    """split_batch and words_space on a host batch and on a device batch against the scanner -> the word offsets of the host batch"""
    w_wo, w_dw, w_sp = wg.bert_offsets(docs, table)
    for src in ("host", "device"):
        shift = np.uint64(front if src == "device" else 0)
        b = _device_batch(docs, front) if src == "device" else docs
        wo, dw = bert.split_batch(b)
        assert "rule=bert" in da.last_kernel(), da.last_kernel()
        assert np.array_equal(dw, w_dw) and np.array_equal(wo, w_wo + shift), (what, src)
        # the words' flags, from the device offsets of the same split
        hay = b[0] if src == "device" else b"".join(docs)
        d_wo, d_dw = bert.split_batch(b, device=True)
        try:
            sp = bert.words_space((hay, d_wo))
        finally:
            d_wo.free()
            d_dw.free()
        assert sp.dtype == np.uint8 and np.array_equal(sp, w_sp), (what, src)
    return w_wo


def test_fixture_documents_against_bert_pre_tokenizer(bert, table):
    docs, _, _, word_spans = wg.cases()
    wo = _check(bert, table, docs, what="fixture").tolist()
    _, dw, sp = wg.bert_offsets(docs, table)
    pos, k = 0, 0
    for d, ws in zip(docs, word_spans):   # BertPreTokenizer's spans are the words that are no whitespace, and whitespace lies between them
        mine = [(wo[w] - pos, wo[w + 1] - pos) for w in range(int(dw[k]), int(dw[k + 1])) if not sp[w]]
        assert mine == ws, d
        covered = sorted(ws + [(wo[w] - pos, wo[w + 1] - pos) for w in range(int(dw[k]), int(dw[k + 1])) if sp[w]])
        assert [s for s, _ in covered] == [0] + [e for _, e in covered][:-1] if d else covered == [], d
        pos += len(d)
        k += 1


def test_tile_edges_and_document_edges(bert, table):
    docs = []
    for lead in (1021, 1022, 1023):                       # U+3001 across positions 1023 / 1024, ending at 1024, starting at 1023
        docs.append([b"a" * lead + COMMA + b"b" * 5])
    for at in (1023, 1024, 1025):                          # a word start at 1023, 1024 and 1025
        docs.append([b"a" * (at - 1) + b" " + b"b" * 7])
        docs.append([b"a" * at + b"!" + b"b" * 7])
        docs.append([b"7" * (at - 2) + WIDE_SPACE[:2], WIDE_SPACE[2:] + b"x"])   # a document edge inside a character, near the tile edge
    docs.append([b"ab" + COMMA[:2]])                      # a document that ends inside multi-byte punctuation: its bytes are O words
    docs.append([b"ab" + COMMA[:1], COMMA[1:] + b"cd"])
    docs.append([b"hello", b"world", b"", b"!", b"", b" x"])   # documents with no whitespace between them
    docs.append([b"", b"", b" \t\n", b"...", b"", NBSP + b"a" + WIDE_SPACE + NBSP + b"b\x01c", b""])
    for i, batch in enumerate(docs):
        for front in (0, 3):
            _check(bert, table, batch, front=front, what=i)
    wo, dw = bert.split_batch([b"ab" + COMMA[:2]])
    assert wo.tolist() == [0, 2, 3, 4] and dw.tolist() == [0, 3]
    wo, dw = bert.split_batch([b"hello", b"world"])
    assert wo.tolist() == [0, 5, 10] and dw.tolist() == [0, 1, 2]
    assert np.array_equal(bert.split(b"a" * 1023 + COMMA), np.array([0, 1023, 1026], dtype=np.uint64))


def test_words_space_by_the_first_unit(bert, table):
    """any word list: flags[w] is the class of the word's first unit, taken inside the word"""
    text = b"a " + NBSP + b"b" + WIDE_SPACE + b"\t\tc" + WIDE_SPACE[:2] + b" " + NBSP[1:] + b"\n!" + b"" + WIDE_SPACE
    cuts = [0, 1, 2, 4, 5, 8, 8, 9, 11, 13, 14, 15, 16, 17, len(text)]
    want = []
    for s, e in zip(cuts, cuts[1:]):
        at, cls = wg.units(text[s:e], table)
        want.append(int(bool(cls) and cls[0] == wg.S))
    assert 0 < sum(want) < len(want)
    hay = torch.from_numpy(np.frombuffer(b"\xe3\x80" + text, dtype=np.uint8).copy()).cuda()
    off = torch.tensor(cuts, dtype=torch.int64).cuda()
    assert bert.words_space((hay, off + 2)).tolist() == want
    assert bert.words_space((b"\xe3\x80" + text, off + 2)).tolist() == want          # a host haystack, staged once
    flags = bert.words_space((hay, off + 2), device=True)
    assert flags.count == len(want) and flags.to_numpy().tolist() == want
    flags.free()
    assert bert.words_space((hay, off[:1])).tolist() == []                            # no word
    # the same words under the default classes: U+3000 and U+00A0 are whitespace there too
    assert da.Splitter(Split.Whitespace).words_space((hay, off + 2)).tolist() == want


def test_the_rules_that_existed_give_what_they_gave(table):
    docs, _, _, _ = wg.cases()
    extra = [b"a" * 1021 + COMMA + b"b" * 5, b"a" * 1023 + b" " + b"b" * 7, b"ab" + COMMA[:2], b"hello", b"world", b"", b" \t\n", b"it's 1234 x" + NBSP + b"y"]
    cc = da.char_classes()
    for rule in (Split.Whitespace, Split.Gpt2):
        w_wo, w_dw = scan_batch(docs + extra, rule, cc)
        wo, dw = da.split_batch(docs + extra, rule)
        assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw), rule
    for rule in (Split.Cl100k, Split.Llama3):   # the scanner of the two rules with scans
        w_wo, w_dw = scan_rule_batch(docs + extra, rule, cc)
        wo, dw = da.split_batch(docs + extra, rule)
        assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw), rule
    # Split.Bert's cached default splitter has bert_char_classes()
    wo, dw = da.split_batch(docs, Split.Bert)
    w_wo, w_dw, _ = wg.bert_offsets(docs, table)
    assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw)
