"""Split.O200k on the MI355X.  Expected words come from the pure-Python sequential scanner of tests/test_split_o200k_host.py
(`scan_o200k`, which that file checks against the `regex` module, `tokenizers` and the stored fixture) with o200k_char_classes(), and
from the fixture itself, never from the library.  Every comparison is exact: word_offsets and doc_words.  The shapes are the smallest at
which the scans across tiles of 1024 positions can go wrong: runs of three tiles and a little, begun around a tile edge.  Every case runs
from host lists and from device (hay, offsets) tensors with offsets[0] > 0.  The five rules that existed before run on one mixed batch
against their own scanners."""
import json
import random

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_split_host import scan_batch
from test_split_rules_host import scan_rule_batch
from test_split_o200k_host import FIXTURE, random_bytes_doc, random_text, scan_o200k_batch
import wordpiece_golden as wg

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, Split

CC = da.o200k_char_classes()
TILE = 1024
HAN, MARK = "\u4e2d".encode(), "\u0301".encode()   # a caseless letter of three bytes, a mark of two


@pytest.fixture(scope="module")
def o200k():
    return da.Splitter(Split.O200k)


def _device_batch(docs, front=0, fill=b"\xe4"):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    off = np.full(len(docs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(fill * front + b"".join(docs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _check(sp, docs, front=3, what=None, classes=CC):
    """split_batch(docs) as a host batch and as a device batch with offsets[0] = front against the scanner -> the expected result"""
    w_wo0, w_dw = scan_o200k_batch(docs, classes)
    for src in ("host", "device"):
        w_wo = w_wo0 + np.uint64(front if src == "device" else 0)
        wo, dw = sp.split_batch(_device_batch(docs, front) if src == "device" else docs)
        assert wo.dtype == np.uint64 and dw.dtype == np.uint64, (what, src)
        assert da.last_kernel().startswith("split rule=o200k ") and f"words={len(w_wo) - 1} " in da.last_kernel() + " ", (what, src, da.last_kernel())
        assert np.array_equal(dw, w_dw), (what, src)
        assert np.array_equal(wo, w_wo), (what, src)
    return w_wo0, w_dw


# ----------------------------------------------------------------------------------------------------- the fixture, random batches
def test_the_fixture_as_one_batch(o200k):
    with open(FIXTURE, encoding="utf-8") as fh:
        cases = json.load(fh)["cases"]
    docs = [c["text"].encode("utf-8") for c in cases]
    lens = np.cumsum([0] + [len(d) for d in docs])
    w_wo = np.array([int(lens[i]) + b for i, c in enumerate(cases) for b in c["o200k"][:-1]] + [int(lens[-1])], dtype=np.uint64)
    w_dw = np.cumsum([0] + [len(c["o200k"]) - 1 for c in cases]).astype(np.uint64)
    wo, dw = o200k.split_batch(docs)
    assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw)
    assert "rule=o200k" in da.last_kernel()
    # again with offsets[0] = 5 and an empty document in front of, between and behind the fixture's
    spaced = [b""] + [x for d in docs for x in (d, b"")]
    wo, dw = o200k.split_batch(_device_batch(spaced, 5))
    assert np.array_equal(wo, w_wo + np.uint64(5))
    assert np.array_equal(dw[1::2], w_dw) and np.array_equal(dw[2::2], w_dw[1:])
    _check(o200k, spaced, front=5, what="fixture")


def test_random_documents(o200k):
    rng = random.Random(11)
    docs = [random_text(rng, 64).encode("utf-8") if k % 4 else random_bytes_doc(rng, 64) for k in range(2000)]
    assert sum(1 for d in docs if not d) > 5 and max(map(len, docs)) > 100
    _check(o200k, docs, front=9, what="random")


def test_custom_classes_make_every_letter_caseless():
    """Splitter(Split.O200k, char_classes()): cls 1 is a caseless letter, so only ASCII has case"""
    plain = da.char_classes()
    sp = da.Splitter(Split.O200k, plain)
    docs = ["éÉ中 ÉéÉ".encode(), "aÉB ÉcD".encode(), "x'ſ".encode()] + [random_text(random.Random(k), 40).encode() for k in range(50)]
    want = _check(sp, docs, what="plain", classes=plain)
    assert not np.array_equal(want[0], scan_o200k_batch(docs, CC)[0])
    sp.free()


# ------------------------------------------------------------------------------------------------------------ runs across tiles
RUNS = {
    "lower_caseless_upper": (b"a", HAN, b"B"),          # breaks in front of B: a lower unit lies any number of caseless units back
    "upper_caseless_upper_lower": (b"A", HAN, b"Bc"),   # one word
    "upper_caseless_upper_space": (b"A", HAN, b"B "),   # the back-off break in front of B
    "caseless_uppers_space": (HAN, b"A", b" "),         # the run of uppers reaches a space: breaks behind the caseless unit
    "caseless_uppers_lower": (HAN, b"A", b"b"),         # one word
    "prefix_marks_lower": (b"!", MARK, b"a"),           # one word: ! is the prefix, the marks are word body
    "punctuation_marks_lower": (b"!!", MARK, b"a"),     # the marks are punctuation body
    "punctuation_newlines_slash": (b"!", b"\n", b"/!"), # / belongs to the trailer
    "digits": (b"x", b"1", b"a"),
    "whitespace_newline_at_the_end": (b"x", b" ", b"\n a"),
}


@pytest.mark.parametrize("kind", list(RUNS))
def test_runs_across_tiles(o200k, kind):
    """a run of 3 * 1024 + k positions, begun at position 1020 .. 1028 of the buffer (host batch: offsets[0] = 0)"""
    head, unit, tail = RUNS[kind]
    docs = []
    for start in range(TILE - 4, TILE + 5):
        fill = b"ab " * ((start - len(head)) // 3) + b"xy "[:(start - len(head)) % 3]
        doc = fill + head + unit * ((3 * TILE + start % 4) // len(unit)) + tail + b" x1"
        assert doc[start - len(head):start] == head and doc[start:start + len(unit)] == unit
        docs.append(doc)
    for doc in docs:   # each alone, so that the run starts where it says
        _check(o200k, [doc], front=TILE, what=(kind, len(doc)))
    _check(o200k, docs, front=1, what=kind)


def test_run_words_are_what_the_rule_says(o200k):
    n = 3 * TILE + 1
    assert o200k.split(b"a" + HAN * n + b"B").tolist() == [0, 1 + 3 * n, 2 + 3 * n]
    assert o200k.split(b"A" + HAN * n + b"Bc").tolist() == [0, 3 + 3 * n]
    assert o200k.split(b"A" + HAN * n + b"B ").tolist() == [0, 1 + 3 * n, 2 + 3 * n, 3 + 3 * n]
    assert o200k.split(HAN + b"A" * n + b" ").tolist() == [0, 3, 3 + n, 4 + n]
    assert o200k.split(HAN + b"A" * n + b"b").tolist() == [0, 4 + n]
    assert o200k.split(b"!" + MARK * n + b"a").tolist() == [0, 2 + 2 * n]
    assert o200k.split(b"!!" + MARK * n + b"a").tolist() == [0, 2 + 2 * n, 3 + 2 * n]
    assert o200k.split(b"!" + b"\n" * n + b"/!").tolist() == [0, 2 + n, 3 + n]


def test_a_state_does_not_cross_a_document_boundary(o200k):
    wo, dw = o200k.split_batch([b"a" + HAN * 2, HAN + b"B"])   # as one document: a|B alone; here the second document is caseless|B
    assert wo.tolist() == [0, 7, 10, 11] and dw.tolist() == [0, 1, 3]
    assert o200k.split(b"a" + HAN * 3 + b"B").tolist() == [0, 10, 11]
    wo, dw = o200k.split_batch([b"a" + HAN * 2, HAN + b"Bc"])  # as one document the lower unit far back breaks in front of B
    assert wo.tolist() == [0, 7, 12] and dw.tolist() == [0, 1, 2]
    assert o200k.split(b"a" + HAN * 3 + b"Bc").tolist() == [0, 10, 12]
    wo, dw = o200k.split_batch([b"!\n", b"/!"])               # as one document / is in the trailer
    assert wo.tolist() == [0, 2, 4] and dw.tolist() == [0, 1, 2]
    assert o200k.split(b"!\n/!").tolist() == [0, 3, 4]
    for docs in ([b"a" + HAN * 2, HAN + b"B"], [b"!\n", b"/!"], [b"ab'", b"s"], [b"12", b"3456"], [b"!", MARK + b"a"], [b"A" + HAN, b"B "], [b"A" + HAN + b"B", b" "]):
        _check(o200k, docs, what=docs)
    # the same boundaries at a tile edge and in the middle of long runs
    for at in (TILE - 1, TILE, TILE + 1):
        _check(o200k, [b"a" + HAN * ((at - 1) // 3) + b"!!"[:(at - 1) % 3], HAN * 400 + b"B", b"", b"A" + HAN * 700, b"B ", b"!" + b"\n" * (at - 1), b"/" * 20 + b"!"],
               front=0, what=at)


def test_a_three_byte_unit_across_a_tile_edge(o200k):
    for lead in (TILE - 2, TILE - 1, 2 * TILE - 2, 2 * TILE - 1):
        for unit, tail in ((HAN, b"B"), (HAN, b"B "), ("\u3001".encode(), b"\n/"), ("\u01c5\u2028".encode(), b"a")):
            for first in (b"a", b"A", b"!"):
                doc = b"z" * (lead - 1) + first + unit + tail
                assert np.array_equal(o200k.split(doc), scan_o200k_batch([doc], CC)[0]), (lead, unit, tail, first)
    _check(o200k, [b"z" * (TILE - 2) + b"a" + HAN + b"B", b"z" * (TILE - 3) + HAN * 2 + b"B "], front=0, what="edge")


# --------------------------------------------------------------------------------------- tokenize_bpe_docs, words_space, one haystack
def test_tokenize_bpe_docs_behind_the_o200k_split():
    """equals split_batch + tokenize_bpe_batch + offsets_compose done by hand, spans moved to the document here"""
    pats = [bytes([b]) for b in range(256)]
    pats += [b"th", b"he", b"the", b" t", b" th", b" the", b"Th", b"The", b" The", b"in", b"ing", b"'s", b"'l", b"'ll", b"ll", b"12", b"123", b"Re", b"que", b"st",
             b"HT", b"TP", b"HTTP", b"!!", b"\n\n", b"//", HAN, MARK, b"e" + MARK]
    p, rest = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(pats).serialize())
    assert rest == b""
    ranks = np.random.default_rng(5).permutation(len(pats)).astype(np.uint32)
    rng = random.Random(6)
    pieces = [b"the", b" The", b"HTTP", b"Request", b"it's", b" WE'LL", b" 12345", b"!!", b"  ", b"\n", b" ", b"/", HAN, MARK, b"e" + MARK, b"'", b"x", b"\xff", "É".encode()]
    docs = [b"".join(rng.choice(pieces) for _ in range(rng.randrange(12))) for _ in range(300)] + [b"getHTTPResponse's !\n/x", b"", b"!!\n\n123"]
    hay, off = _device_batch(docs, 6)
    wo, dw = da.split_batch((hay, off), Split.O200k, device=True)
    h_wo, h_dw = wo.to_numpy(), dw.to_numpy()
    assert np.array_equal(h_wo, scan_o200k_batch(docs, CC, 6)[0])
    words = (hay, torch.from_numpy(h_wo.astype(np.int64)).cuda())
    ids, spans, tok = p.tokenize_bpe_batch(words, ranks, gap=Gap.Bytes, gap_id=1000, spans=True, device=True)
    doc_tok = da.offsets_compose(tok, dw)
    h_tok, h_spans = tok.to_numpy().astype(np.int64), spans.to_numpy().astype(np.int64).reshape(-1, 2)
    word_of_token = np.repeat(np.arange(len(h_wo) - 1), np.diff(h_tok))
    doc_of_word = np.searchsorted(h_dw.astype(np.int64), np.arange(len(h_wo) - 1), side="right") - 1
    shift = h_wo.astype(np.int64)[word_of_token] - off.cpu().numpy()[doc_of_word[word_of_token]]
    want = (ids.to_numpy(), (h_spans + shift[:, None]).astype(np.uint64), doc_tok)
    for x in (wo, dw, ids, spans, tok):
        x.free()
    for arg in (docs, (hay, off)):
        g_ids, g_sp, g_off = p.tokenize_bpe_docs(arg, ranks, split=Split.O200k, gap_id=1000, spans=True)
        assert np.array_equal(g_ids, want[0]) and np.array_equal(g_sp.reshape(-1, 2), want[1]) and np.array_equal(g_off, want[2])
    sp = da.Splitter(Split.O200k)
    g_ids, g_off = p.tokenize_bpe_docs(docs, ranks, split=sp, gap_id=1000)
    assert np.array_equal(g_ids, want[0]) and np.array_equal(g_off, want[2])
    assert int(want[2][-1]) == len(want[0]) > 1000


def test_words_space_and_one_haystack(o200k):
    rng = random.Random(8)
    text = "".join(random_text(rng, 14) for _ in range(500)).encode() + b"  \n  "
    assert len(text) > 3 * TILE
    want = scan_o200k_batch([text], CC)[0]
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    assert np.array_equal(o200k.split(text), want) and np.array_equal(o200k.split(dev), want)
    assert "rule=o200k" in da.last_kernel()
    assert np.array_equal(da.split_batch([text], Split.O200k)[0], want) and o200k.split(b"").tolist() == [0]
    # a word is whitespace where its first unit is: U+2028 and U+00A0 are, a mark and a caseless letter are not
    space = {" ", "\n", "\t", "\r", "\u2028", "\u00a0"}
    w_sp = np.array([text[s:e].decode("utf-8")[0] in space for s, e in zip(want.tolist(), want.tolist()[1:])], dtype=np.uint8)
    assert 0 < w_sp.sum() < len(w_sp)
    for hay in (text, dev):
        d_wo = o200k.split(hay, device=True)
        try:
            assert np.array_equal(o200k.words_space((hay, d_wo)), w_sp)
        finally:
            d_wo.free()


# ------------------------------------------------------------------------------------------------------------ the earlier rules
def test_the_earlier_rules_on_one_mixed_batch():
    """Split.Whitespace, Gpt2, Cl100k, Llama3 and Bert still equal their own scanners"""
    rng = random.Random(9)
    docs = [random_text(rng, 40).encode() for _ in range(300)] + [b"ab " * 333 + b"x" + b"1" * (3 * TILE + 1) + b"x", b"!" + b"\n" * 1100 + b" it's", b"",
                                                                 b"ab " * 333 + b"!" + b" " * (TILE + 7) + b"\n" + b" " * (2 * TILE) + b"a"]
    plain = da.char_classes()
    want = {Split.Whitespace: scan_batch(docs, Split.Whitespace, plain), Split.Gpt2: scan_batch(docs, Split.Gpt2, plain),
            Split.Cl100k: scan_rule_batch(docs, Split.Cl100k, plain), Split.Llama3: scan_rule_batch(docs, Split.Llama3, plain),
            Split.Bert: wg.bert_offsets(docs, wg.class_table(da.bert_char_classes()))[:2]}
    for rule, (w_wo, w_dw) in want.items():
        wo, dw = da.split_batch(docs, rule)
        assert da.last_kernel().startswith("split rule=" + rule.name.lower() + " "), rule
        assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw), rule
        wo, dw = da.split_batch(_device_batch(docs, 4), rule)
        assert np.array_equal(wo, w_wo + np.uint64(4)) and np.array_equal(dw, w_dw), rule
