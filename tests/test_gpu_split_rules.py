"""Split.Cl100k and Split.Llama3 on the MI355X.  Expected words come from the pure-Python sequential scanner of
tests/test_split_rules_host.py (`scan_rule`, which that file checks against the `regex` module, `tokenizers` and the stored fixture) with
char_classes(), and from the fixture itself, never from the library.  Every comparison is exact: word_offsets and doc_words.  The shapes
are the smallest at which the scans across tiles of 1024 positions can go wrong: runs of three tiles and a little, begun around a tile
edge.  Every case runs for both rules, from host lists and from device (hay, offsets) tensors with offsets[0] > 0."""
import json
import random
import re

import numpy as np
import pytest
import torch

from test_gpu_split import _device_batch, _mixed_docs, vocab  # noqa: F401  (vocab: the BPE fixture vocabulary)
from test_split_host import scan_batch
from test_split_rules_host import FIXTURE, random_bytes_doc, scan_rule_batch

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, Split

RULES = (Split.Cl100k, Split.Llama3)
CC = da.char_classes()
TILE = 1024
DIGIT2 = "٣".encode()   # U+0663: a digit of two bytes


@pytest.fixture(scope="module")
def splitters():
    return {rule: da.Splitter(rule) for rule in RULES}


def _check(splitters, docs, front=3, what=None, differ=None):
    """split_batch(docs) as a host batch and as a device batch with offsets[0] = front against the scanner; `differ`: whether the two
    rules must give different words"""
    want = {rule: scan_rule_batch(docs, rule, CC) for rule in RULES}
    if differ is not None:
        assert np.array_equal(want[Split.Cl100k][0], want[Split.Llama3][0]) != differ, what
    for rule in RULES:
        w_wo0, w_dw = want[rule]
        for src in ("host", "device"):
            w_wo = w_wo0 + np.uint64(front if src == "device" else 0)
            wo, dw = splitters[rule].split_batch(_device_batch(docs, front) if src == "device" else docs)
            assert wo.dtype == np.uint64 and dw.dtype == np.uint64, (what, rule, src)
            assert da.last_kernel().startswith("split rule=" + rule.name.lower() + " "), (what, rule, src, da.last_kernel())
            assert int(re.search(r"tile=(\d+)", da.last_kernel()).group(1)) == TILE
            assert np.array_equal(dw, w_dw), (what, rule, src)
            assert np.array_equal(wo, w_wo), (what, rule, src)


# ------------------------------------------------------------------------------------------------------------------ digit runs
@pytest.mark.parametrize("digit", [b"1", DIGIT2], ids=["ascii", "two_bytes"])
def test_digit_runs_across_tiles(splitters, digit):
    """runs of 3 * 1024 + k bytes (of as many two-byte digits: a unit then straddles a tile edge), begun at 1022 .. 1025"""
    for start in (TILE - 2, TILE - 1, TILE, TILE + 1):
        for k in (0, 1, 2):
            doc = b"ab " * (start // 3) + b"xy"[:start % 3] + digit * (3 * TILE + k) + b"x1234"
            assert len(doc) > start and doc[start:start + len(digit)] == digit and doc[start - 1:start] not in b"0123456789"
            _check(splitters, [doc], what=(start, k))
    wo = splitters[Split.Llama3].split(b"." * TILE + b"1" * (3 * TILE + 1))
    assert wo.tolist() == [0] + list(range(TILE, 4 * TILE + 1, 3)) + [4 * TILE + 1]


def test_digit_runs_cut_by_a_document_boundary(splitters):
    """in the middle of a tile and exactly at a tile edge: the count starts again with the document"""
    for digit in (b"1", DIGIT2):
        _check(splitters, [digit * 750, digit * 1000], what="mid")          # a boundary at byte 750 or 1500
        _check(splitters, [digit * (TILE // len(digit)), digit * 1030, b"", digit * 999], what="edge")
        _check(splitters, [b"a" + digit * 2047, digit * 5, digit * 4, digit * 3000], what="mixed")
    wo, dw = splitters[Split.Cl100k].split_batch([b"1" * TILE, b"1" * 8])
    assert wo.tolist()[-5:] == [TILE - 1, TILE, TILE + 3, TILE + 6, TILE + 8] and dw.tolist() == [0, 342, 345]


# ------------------------------------------------------------------------------------------------------------- whitespace runs
@pytest.mark.parametrize("newline", ["first", "middle", "last", "none"])
def test_whitespace_run_over_three_tiles(splitters, newline):
    """a whitespace run from position 1000 over three tile edges with its only newline in its first, middle or last tile, or none (F is
    false throughout), followed by a letter, punctuation, a digit and the document's end, where the two rules must differ"""
    n = 3 * TILE + 17
    run = bytearray(b" " * n)
    if newline != "none":
        run[{"first": 11, "middle": TILE + 300, "last": n - 3}[newline]] = 0x0A
    for tail in (b"a", b"!", b"7", b""):
        for head in (b"ab " * 333 + b"x", b"ab " * 333 + b"!"):
            doc = head + bytes(run) + tail
            assert len(head) == 1000
            _check(splitters, [doc], what=(newline, tail, head[-1:]), differ=(tail == b"" and newline != "none") or None)
    # the same with whitespace of two and three bytes, and the run as a document of its own between two others
    wide = (" \u0085 " * (n // 3)).encode()
    _check(splitters, [b"x" * 1001 + wide + b"a", bytes(run), b"a" + bytes(run)], what=(newline, "batch"))


def test_newline_runs_carry_the_unit_in_front_of_them(splitters):
    """more than a tile of newlines behind one O unit (the punctuation alternative takes them: T) and behind a letter (it does not)"""
    for front in (b"ab!", b"aba", "ab中".encode(), "ab。".encode(), b"ab\xff"):
        for at in (0, TILE - 4, TILE - 3):
            docs = [b"c " * (at // 2) + front + b"\n" * (TILE + 90) + b" y", b"\n" * 70 + b"!" + b"\r\n" * 600 + b"\n"]
            _check(splitters, docs, what=(front, at))
    wo = splitters[Split.Llama3].split(b"!" + b"\n" * 2000 + b"a")
    assert wo.tolist() == [0, 2001, 2002]
    wo = splitters[Split.Llama3].split(b"a" + b"\n" * 2000 + b"a")
    assert wo.tolist() == [0, 1, 2001, 2002]


# -------------------------------------------------------------------------------------------------- the fixture, random batches
def test_the_fixture_as_one_batch(splitters):
    with open(FIXTURE, encoding="utf-8") as fh:
        cases = json.load(fh)["cases"]
    docs = [c["text"].encode("utf-8") for c in cases]
    lens = np.cumsum([0] + [len(d) for d in docs])
    for rule in RULES:
        key = rule.name.lower()
        w_wo = np.array([int(lens[i]) + b for i, c in enumerate(cases) for b in c[key][:-1]] + [int(lens[-1])], dtype=np.uint64)
        w_dw = np.cumsum([0] + [len(c[key]) - 1 for c in cases]).astype(np.uint64)
        wo, dw = splitters[rule].split_batch(docs)
        assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw), rule
        wo, dw = splitters[rule].split_batch(_device_batch(docs, 5))
        assert np.array_equal(wo, w_wo + np.uint64(5)) and np.array_equal(dw, w_dw), rule
    _check(splitters, docs, what="fixture")


def test_many_short_documents_with_malformed_utf8(splitters):
    rng = random.Random(7)
    docs = [random_bytes_doc(rng, 40)[:40] for _ in range(4000)]
    assert sum(1 for d in docs if not d) > 20 and max(map(len, docs)) == 40
    _check(splitters, docs, front=9, what="short")


def test_split_of_one_haystack(splitters):
    rng = random.Random(8)
    text = b"".join(random_bytes_doc(rng, 14) for _ in range(400)) + b"  \n  "
    assert len(text) > 3 * TILE
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for rule in RULES:
        want = scan_rule_batch([text], rule, CC)[0]
        assert np.array_equal(splitters[rule].split(text), want), rule
        assert np.array_equal(splitters[rule].split(dev), want), rule
        assert np.array_equal(da.split_batch([text], rule)[0], want), rule
        assert splitters[rule].split(b"").tolist() == [0]
    assert not np.array_equal(splitters[Split.Cl100k].split(text), splitters[Split.Llama3].split(text))


# ----------------------------------------------------------------------------------------------------------- tokenize_bpe_docs
def test_tokenize_bpe_docs_behind_the_llama3_split(vocab):  # noqa: F811
    """equals split_batch + tokenize_bpe_batch + offsets_compose done by hand, spans moved to the document here"""
    p, ranks = vocab
    docs = _mixed_docs(300) + [b"it'S 12345 we'LL\n\n  the cat  ", b"", b"!!\n\n123"]
    hay, off = _device_batch(docs, 6)
    for rule in RULES:
        wo, dw = da.split_batch((hay, off), rule, device=True)
        h_wo, h_dw = wo.to_numpy(), dw.to_numpy()
        assert np.array_equal(h_wo, scan_rule_batch(docs, rule, CC, 6)[0])
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
            g_ids, g_sp, g_off = p.tokenize_bpe_docs(arg, ranks, split=rule, gap_id=1000, spans=True)
            assert np.array_equal(g_ids, want[0]) and np.array_equal(g_sp.reshape(-1, 2), want[1]) and np.array_equal(g_off, want[2]), rule
        sp = da.Splitter(rule)
        g_ids, g_off = p.tokenize_bpe_docs(docs, ranks, split=sp, gap_id=1000)
        assert np.array_equal(g_ids, want[0]) and np.array_equal(g_off, want[2]), rule
    assert int(want[2][-1]) == len(want[0]) > 1000


# ------------------------------------------------------------------------------------------------------- the two earlier rules
def test_the_earlier_rules_on_a_long_run_input():
    """Split.Gpt2 and Split.Whitespace on runs over three tiles still equal the scanner of tests/test_split_host.py"""
    docs = [b"ab " * 333 + b"x" + b"1" * (3 * TILE + 1) + b"x", b"ab " * 333 + b"!" + b" " * (TILE + 7) + b"\n" + b" " * (2 * TILE) + b"a", b"!" + b"\n" * 1100]
    for rule in (Split.Gpt2, Split.Whitespace):
        w_wo, w_dw = scan_batch(docs, rule, CC)
        wo, dw = da.split_batch(docs, rule)
        assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw), rule
        assert da.last_kernel().startswith("split rule=" + rule.name.lower() + " ")
        wo, dw = da.split_batch(_device_batch(docs, 4), rule)
        assert np.array_equal(wo, w_wo + np.uint64(4)) and np.array_equal(dw, w_dw), rule
