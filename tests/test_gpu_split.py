"""split_batch on the MI355X (daac_split_batch / daac_split / daac_offsets_compose, tokenize_bpe_docs).  Expected words come from the
pure-Python sequential scanner of tests/test_split_host.py (`_scan`, which that file checks against the `regex` module) with
char_classes(), never from the library.  Every comparison is exact: word_offsets, doc_words and n_words.  There is no tolerance in this
feature."""
import random
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_split_host import ALPHABET, random_doc, scan_batch

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, Split, _ffi

RULES = (Split.Whitespace, Split.Gpt2)
CC = da.char_classes()
LETTER4 = "\U0001d400".encode()   # a letter of four bytes


@pytest.fixture(scope="module")
def splitters():
    return {rule: da.Splitter(rule) for rule in RULES}


def _device_batch(docs, front=0, fill=b"\xe6"):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    off = np.full(len(docs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(fill * front + b"".join(docs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _words_reported():
    return int(re.search(r"words=(\d+)", da.last_kernel()).group(1))


def _tile():
    """the positions of a workgroup, as the library reports them"""
    return int(re.search(r"tile=(\d+)", da.last_kernel()).group(1))


def _check(splitters, docs, front=3, rules=RULES, want=None, what=None):
    """split_batch(docs) as a host batch and as a device batch against the scanner"""
    for rule in rules:
        w_wo0, w_dw = want[rule] if want else scan_batch(docs, rule, CC)
        for src in ("host", "device"):
            w_wo = w_wo0 + np.uint64(front if src == "device" else 0)
            wo, dw = splitters[rule].split_batch(_device_batch(docs, front) if src == "device" else docs)
            assert wo.dtype == np.uint64 and dw.dtype == np.uint64, (what, rule, src)
            assert _words_reported() == len(w_wo) - 1 and da.last_kernel().startswith("split rule="), (what, rule, src, da.last_kernel())
            assert np.array_equal(dw, w_dw), (what, rule, src)
            assert np.array_equal(wo, w_wo), (what, rule, src)


def _b(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


# ------------------------------------------------------------------------------------------------------------- 1. hand cases
def test_hand_cases(splitters):
    han = "漢".encode()
    docs = [_b(d) for d in (
        "", "", "it's we'll  a\n'd !'s 123abc", "a   ", "  'll", "", "x's't", "'s", "we'l", "l go", "'", "re",
        b"a" + han[:2], han[2:] + b"b", han[:1], han[1:], "", "é漢 ٣²\u0085 　x" + "\U0001d400", b"\xff\xc0\xaf \xed\xa0\x80", " ", "  ", "", "")]
    _check(splitters, docs, what="hand")
    wo, dw = splitters[Split.Gpt2].split_batch(docs[2:3])
    assert [docs[2][s:e] for s, e in zip(wo.tolist(), wo.tolist()[1:])] == [b"it", b"'s", b" we", b"'ll", b" ", b" a", b"\n", b"'d", b" !'", b"s", b" 123", b"abc"]
    assert dw.tolist() == [0, 12]
    for one in docs:   # a batch of one document, and the single-haystack call
        _check(splitters, [one], front=1, what=one)
        for rule in RULES:
            want = scan_batch([one], rule, CC)[0]
            assert np.array_equal(splitters[rule].split(one), want), (one, rule)
            if one:
                assert np.array_equal(splitters[rule].split(torch.from_numpy(np.frombuffer(one, dtype=np.uint8).copy()).cuda()), want), (one, rule)
    # only empty documents, and no document at all
    _check(splitters, [b"", b"", b""], what="empty")
    for rule in RULES:
        wo, dw = splitters[rule].split_batch([])
        assert wo.tolist() == [0] and dw.tolist() == [0] and wo.dtype == np.uint64


def test_front_bytes_are_not_read(splitters):
    """a device batch whose first document begins with continuation bytes, behind `front` bytes E6 that would make them a character"""
    docs = [b"\xbc\xa2x y", b"\xa2 z"]
    for front in (1, 2, 3, 13, 64):
        _check(splitters, docs, front=front, what=front)
    wo, dw = splitters[Split.Gpt2].split_batch(_device_batch(docs, 2))
    assert wo[:3].tolist() == [2, 4, 5] and wo[-1] == 2 + 5 + 3   # BC A2 are two units of class O: x is no letter behind a letter


def test_module_level_split_batch_and_custom_classes():
    docs = [b"it's  so", "éa٣1 x".encode()]
    for rule in RULES:
        wo, dw = da.split_batch(docs, rule)
        w_wo, w_dw = scan_batch(docs, rule, CC)
        assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw)
    mine = np.array([(0xE9, 0xE9, 2), (0x663, 0x663, 1)], dtype=np.uint32)   # é a number, ٣ a letter
    sp = da.Splitter(Split.Gpt2, mine)
    wo, dw = sp.split_batch(docs)
    w_wo, w_dw = scan_batch(docs, Split.Gpt2, mine)
    assert np.array_equal(wo, w_wo) and np.array_equal(dw, w_dw)
    assert not np.array_equal(w_wo, scan_batch(docs, Split.Gpt2, CC)[0])
    none = da.Splitter(Split.Gpt2, [])   # no ranges: every code point from U+0080 on is O
    assert np.array_equal(none.split_batch(docs)[0], scan_batch(docs, Split.Gpt2, np.zeros((0, 3), dtype=np.uint32))[0])


# -------------------------------------------------------------------------------------------------- 2. edges of the launch shape
def test_one_long_text(splitters):
    """about 1 MiB as one document: a thousand workgroup tiles"""
    rng = random.Random(1)
    text = b"".join(rng.choice(ALPHABET) for _ in range(640000))
    assert len(text) > 1000000
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for rule in RULES:   # (rule by rule on one text: the scanner cuts it into units once)
        want = scan_batch([text], rule, CC)[0]
        assert np.array_equal(splitters[rule].split(dev), want), rule
        assert _words_reported() == len(want) - 1
        assert np.array_equal(splitters[rule].split(text), want), rule


def test_many_tiles_take_the_chunked_sum(splitters):
    """more tiles than launch_exclusive_scan sums in one workgroup (8192): 150 copies of one document of 65 521 bytes, whose words the
    scanner finds once (documents are independent)"""
    rng = random.Random(2)
    doc = b"".join(rng.choice(ALPHABET) for _ in range(40000))[:65521]
    copies = 150
    hay, off = _device_batch([doc] * copies, front=7)
    for rule in RULES:
        wo1, _ = scan_batch([doc], rule, CC)
        per = len(wo1) - 1
        want = (wo1[:-1][None, :] + (np.arange(copies, dtype=np.uint64) * np.uint64(len(doc)))[:, None] + np.uint64(7)).reshape(-1)
        wo, dw = splitters[rule].split_batch((hay, off))
        assert len(doc) * copies > 8192 * _tile()
        assert np.array_equal(dw, np.arange(copies + 1, dtype=np.uint64) * np.uint64(per)), rule
        assert np.array_equal(wo[:-1], want) and wo[-1] == 7 + len(doc) * copies, rule


def _sweep_texts(tile):
    """each probe at 64 consecutive byte shifts across the first tile edge and across the first 64-byte edge"""
    probes = (b"'ll", LETTER4, b"  a", b"\n'd")
    texts = []
    for edge in (64, tile):
        for probe in probes:
            for shift in range(64):
                at = edge - 60 + shift   # the probe begins 60 bytes in front of the edge .. 3 bytes behind it
                texts.append((b"ab " * (at // 3 + 1))[:at] + probe + b"cd 'll" + LETTER4 + b"  x\n'd e" * 3)
    return texts


def test_sweep_over_lane_mask_word_and_tile_edges(splitters):
    splitters[Split.Gpt2].split(b"x")
    tile = _tile()
    texts = _sweep_texts(tile)
    assert max(map(len, texts)) > tile + 8
    for rule in RULES:
        for i, t in enumerate(texts):   # one text, one call: the probe lies at a known position of the launch
            want = scan_batch([t], rule, CC)[0]
            assert np.array_equal(splitters[rule].split(t), want), (rule, i)
    # the same texts as the documents of one batch: every probe at yet another phase
    _check(splitters, texts, front=5, what="sweep batch")


def test_sweep_of_a_document_boundary(splitters):
    """a document boundary at each of those shifts, inside a contraction, a character, a whitespace run and behind a newline"""
    splitters[Split.Gpt2].split(b"x")
    tile = _tile()
    body = (b"we'll  a\n'd " + LETTER4 + "漢 ".encode()) * (tile // 16)
    for edge in (64, tile):
        docs = []
        for shift in range(64):
            cut = edge - 60 + shift
            docs += [body[:cut], body[cut:edge + 40]]
            _check(splitters, docs[-2:], front=0, what=(edge, shift))
        _check(splitters, docs, front=11, what=edge)


# ---------------------------------------------------------------------------------------------------- 3. many short documents
def test_many_short_documents(splitters):
    rng = random.Random(3)
    docs = []
    for _ in range(20000):
        d = random_doc(rng, 6)
        docs.append(d[:rng.randrange(13)])
    want = {rule: scan_batch(docs, rule, CC, 0) for rule in RULES}
    _check(splitters, docs, front=9, want=want, what="short")
    for rule in RULES:
        wo, dw = splitters[rule].split_batch(docs)
        assert (np.diff(dw.astype(np.int64)) >= 0).all() and dw[-1] == len(wo) - 1 == _words_reported()
        lens = np.array([len(d) for d in docs])
        assert ((np.diff(dw.astype(np.int64)) == 0) == (lens == 0)).all()   # exactly the empty documents have no word


# ------------------------------------------------------------------------------------------------- 4. offsets_compose, device
def test_offsets_compose():
    rng = np.random.default_rng(4)
    inner = np.cumsum(rng.integers(0, 9, 5000)).astype(np.int64)
    d_in = torch.from_numpy(inner).cuda()
    for n_outer in (1, 2, 777, 100000):
        outer = np.sort(rng.integers(0, len(inner), n_outer)).astype(np.int64)
        got = da.offsets_compose(d_in, torch.from_numpy(outer).cuda())
        assert got.dtype == np.uint64 and np.array_equal(got, inner[outer].astype(np.uint64)), n_outer
    got = da.offsets_compose(d_in, torch.from_numpy(np.array([4999], dtype=np.int64)).cuda(), device=True)
    assert isinstance(got, da.bytewise.DeviceOffsets) and got.count == 1 and got.to_numpy().tolist() == [int(inner[4999])]
    # DeviceOffsets as arguments: a split's own results
    wo, dw = da.split_batch([b"a b", b"", b"c"], device=True)
    assert da.offsets_compose(wo, dw).tolist() == wo.to_numpy()[dw.to_numpy()].tolist() == [0, 3, 3, 4]
    for x in (got, wo, dw):
        x.free()


def test_results_left_on_the_device(splitters):
    docs = [b"it's a test", b"", "é漢 12".encode()]
    for rule in RULES:
        w_wo, w_dw = scan_batch(docs, rule, CC, 4)
        for arg in (docs, _device_batch(docs, 4)):
            wo, dw = splitters[rule].split_batch(arg, device=True)
            base = 4 if isinstance(arg, tuple) else 0
            assert isinstance(wo, da.bytewise.DeviceOffsets) and isinstance(dw, da.bytewise.DeviceOffsets)
            assert wo.count == len(w_wo) and dw.count == len(docs) + 1
            a, b = wo.to_numpy(), dw.to_numpy()
            assert a.dtype == np.uint64 and b.dtype == np.uint64
            assert np.array_equal(a, w_wo - np.uint64(4 - base)) and np.array_equal(b, w_dw)
            assert np.array_equal(wo.to_numpy(), a)   # a second copy is the same
            wo.free()
            dw.free()
            wo.free()
            with pytest.raises(da.DaachorseError):
                wo.to_numpy()
        one = splitters[rule].split(docs[0], device=True)
        assert isinstance(one, da.bytewise.DeviceOffsets) and np.array_equal(one.to_numpy(), scan_batch(docs[:1], rule, CC)[0])
        one.free()
    # (hay, word_offsets) is a batch itself: the words of the words under the whitespace rule are the words
    hay, off = _device_batch(docs, 4)
    wo, dw = splitters[Split.Gpt2].split_batch((hay, off), device=True)
    words = torch.from_numpy(wo.to_numpy().astype(np.int64)).cuda()
    wo2, dw2 = splitters[Split.Gpt2].split_batch((hay, words))
    assert np.array_equal(wo2, wo.to_numpy()) and np.array_equal(dw2, np.arange(wo.count, dtype=np.uint64))


def test_a_word_list_above_max_result_bytes_answers_2(splitters):
    da.set_option("max_result_bytes", 64)
    try:
        with pytest.raises(da.DaachorseError) as ei:
            splitters[Split.Gpt2].split_batch([b"a b c d e f g h i j k l"])
        assert ei.value.code == 2 and "max_result_bytes" in str(ei.value)
        wo, dw = splitters[Split.Gpt2].split_batch([b"a b c"])   # 3 words + 1: fits
        assert wo.tolist() == [0, 1, 3, 5]
    finally:
        da.set_option("max_result_bytes", 8 << 30)


def test_decreasing_device_offsets_answer_1(splitters):
    hay = torch.zeros(64, dtype=torch.uint8).cuda()
    off = torch.tensor([0, 10, 5, 20], dtype=torch.int64).cuda()
    with pytest.raises(da.DaachorseError) as ei:
        splitters[Split.Gpt2].split_batch((hay, off))
    assert ei.value.code == 1 and "document 1" in str(ei.value)


# ------------------------------------------------------------------------------------------------------- 5. tokenize_bpe_docs
@pytest.fixture(scope="module")
def vocab():
    pats = [bytes([b]) for b in range(256) if chr(b).isalnum() or b in b" '!\n"]
    pats += [b"th", b"he", b"the", b" t", b" th", b" the", b"in", b"ing", b" a", b"an", b"and", b" and", b"'s", b"'l", b"'ll", b"ll", b"12", b"123", b" 1",
             b"it", b"we", b" we", b"at", b"cat", b" cat", b" c", "é".encode(), "漢".encode(), b"  ", b"!!"]
    o = orc.OraclePma.build(pats)
    p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    ranks = np.random.default_rng(5).permutation(len(pats)).astype(np.uint32)
    return p, ranks


def _mixed_docs(n):
    rng = random.Random(6)
    pieces = [b"the", b" the", b" cat", b" and", b"it's", b" we'll", b" 123", b"!!", b"  ", b"\n", b" ", "é漢".encode(), b"sing", b"'", b"x", b"\xff", LETTER4]
    return [b"".join(rng.choice(pieces) for _ in range(rng.randrange(12))) for _ in range(n)]


def test_tokenize_bpe_docs(vocab):
    """ids, spans and per-document offsets equal tokenize_bpe run on each word of the reference split, concatenated"""
    p, ranks = vocab
    docs = _mixed_docs(300)
    docs[7] = b""
    for rule in RULES:
        ids, spans, off, memo = [], [], [0], {}
        for d in docs:
            b = scan_batch([d], rule, CC)[0].tolist()
            for s, e in zip(b, b[1:]):
                if d[s:e] not in memo:   # (the same word again is the same call again)
                    memo[d[s:e]] = p.tokenize_bpe(d[s:e], ranks, gap=Gap.Bytes, gap_id=1000, spans=True)
                w_ids, w_sp = memo[d[s:e]]
                ids += w_ids.tolist()
                spans += (w_sp + np.uint64(s)).tolist()
            off.append(len(ids))
        want = (np.array(ids, dtype=np.uint32), np.array(spans, dtype=np.uint64).reshape(-1, 2), np.array(off, dtype=np.uint64))
        for arg in (docs, _device_batch(docs, 6)):
            g_ids, g_sp, g_off = p.tokenize_bpe_docs(arg, ranks, split=rule, gap_id=1000, spans=True)
            assert g_ids.dtype == np.uint32 and g_sp.dtype == np.uint64 and g_off.dtype == np.uint64
            assert np.array_equal(g_off, want[2]) and np.array_equal(g_ids, want[0]) and np.array_equal(g_sp, want[1]), rule
            g_ids, g_off = p.tokenize_bpe_docs(arg, ranks, split=rule, gap_id=1000)
            assert np.array_equal(g_off, want[2]) and np.array_equal(g_ids, want[0]), rule
        dev = p.tokenize_bpe_docs(docs, ranks, split=rule, gap_id=1000, spans=True, device=True)
        assert np.array_equal(dev[0].to_numpy(), want[0]) and np.array_equal(dev[1].to_numpy(), want[1]) and np.array_equal(dev[2].to_numpy(), want[2])
        for x in dev:
            x.free()
    # a splitter of the caller's, no document, only empty documents
    sp = da.Splitter(Split.Gpt2)
    assert np.array_equal(p.tokenize_bpe_docs(docs, ranks, split=sp, gap_id=1000)[0], p.tokenize_bpe_docs(docs, ranks, gap_id=1000)[0])
    ids, off = p.tokenize_bpe_docs([], ranks)
    assert ids.tolist() == [] and off.tolist() == [0]
    ids, sp_, off = p.tokenize_bpe_docs([b"", b""], ranks, spans=True)
    assert ids.tolist() == [] and sp_.shape == (0, 2) and off.tolist() == [0, 0, 0]


def test_tokenize_bpe_docs_passes_a_long_word_through_as_6(vocab):
    p, ranks = vocab
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_bpe_docs([b"a cat", b"so " + b"x" * 5000 + b" long"], ranks)
    assert ei.value.code == 6 and "bpe_doc_max" in str(ei.value)
    ids, off = p.tokenize_bpe_docs([b"a cat", b"so " + b"x" * 4000 + b" long"], ranks)
    assert off[-1] == len(ids) and off[1] >= 2
