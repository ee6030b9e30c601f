"""tests/batch_scale.py on the host: `expand` over the per-pool-document results equals the plain per-document loop over the same
references at n = 3000, for every feature whose batch the GPU tests expand to a million documents, and `pooled` packs what _Batch packs.
No GPU: this keeps the million-document expectations of tests/test_gpu_batch_scale.py from being an unverified piece of numpy."""
import numpy as np
import pytest

import batch_scale as bs
import normalize_golden as ng
import special_golden as sg
from oracle import oracle as orc
from test_gpu_tokenize_bpe import _expect as bpe_expect
from test_gpu_tokenize_unigram import _bits, _expect as unigram_expect
from test_gpu_tokenize_wordpiece import VOCAB

import daachorse_amd as da
from daachorse_amd import Gap, ScanMode, Split
from daachorse_amd.bytewise import _Batch

N = 3000
GID = 0x10000
MODES = (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix, ScanMode.Find, ScanMode.LeftmostFind)


def _oracle(mode, charwise=False, empty=False):
    pats = list(bs.CHAR_PATTERNS if charwise else bs.BYTE_PATTERNS) + ([""] if empty else [])
    kind = 1 if mode == ScanMode.LeftmostFind else 0
    return (orc.OracleCharwisePma if charwise else orc.OraclePma).build(pats, kind=kind)


def _pool(charwise=False, keep=None):
    return bs.make_pool(bs.CHAR_HAND if charwise else bs.BYTE_HAND, bs.CHAR_LETTERS if charwise else bs.BYTE_LETTERS, 64, 3, keep=keep)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g, w)


def test_pooled_packs_what_the_batch_argument_packs():
    pool = _pool()
    pins = [2, 3, 4, 5, 6]
    idx, hay, off = bs.pooled(pool, N, 1, pins=pins, turns=(1000,))
    docs = [pool[i] for i in idx.tolist()]
    b = _Batch(docs)
    assert b.n == N and np.array_equal(b.offsets, off.astype(np.uint64)) and b.buf.tobytes() == hay.tobytes()
    assert off.dtype == np.int64 and hay.dtype == np.uint8 and idx.min() == 0 and idx.max() == len(pool) - 1
    assert [int(idx[a]) for a in bs.marks(N, (1000,))] == pins and bs.marks(N, (1000,)) == [0, 999, 1000, 1001, N - 1]
    assert bs.marks(N) == [0, N - 1]   # the default turn lies beyond this batch
    assert len({(len(pool[p]), pool[p]) for p in pins}) == 5
    hay2, off2 = bs.pack(docs, base=37)
    assert hay2.tobytes() == hay.tobytes() and np.array_equal(off2, off + 37)
    idx0, hay0, off0 = bs.pooled(pool, 0, 1)
    assert len(idx0) == 0 and len(hay0) == 0 and off0.tolist() == [0]


def test_the_pools_hold_what_the_issue_asks():
    for charwise in (False, True):
        pool = _pool(charwise)
        blobs = [bs._b(d) for d in pool]
        assert len(pool) == 64 and len(set(blobs)) == 64 and b"" in blobs
        assert {len(b) for b in blobs} >= set(range(0, 9))
        assert any(0xC2 <= b[0] <= 0xDF for b in blobs if b) and any(0xE0 <= b[0] <= 0xEF for b in blobs if b)
        o = _oracle(ScanMode.FindOverlapping, charwise)
        counts = bs.ref_matches(o, ScanMode.FindOverlapping, pool)
        assert (counts == 0).sum() >= 2 and counts.max() >= 6
        assert len(bs.pins_of(counts, pool)) == 5
    assert any(b"\xff" in bs._b(d) for d in _pool())   # an ill-formed byte


@pytest.mark.parametrize("name", ["WORD", "TEXT", "SPECIAL", "NORM"])
def test_the_feature_pools_hold_what_the_issue_asks(name):
    """the hand-written part alone, without the random fill: the empty document, every length from 1 to 8 bytes, characters of two and
    three bytes, an ill-formed byte, a document without a result and documents with several"""
    hand = [bs._b(d) for d in getattr(bs, name + "_HAND")]
    assert len(set(hand)) == len(hand) and hand[0] == b"" and {len(d) for d in hand} >= set(range(9))

    def valid(d):
        try:
            d.decode("utf-8")
            return True
        except UnicodeDecodeError:
            return False
    text = "".join(d.decode("utf-8") for d in hand if valid(d))
    assert any(0x80 <= ord(c) < 0x800 for c in text) and any(0x800 <= ord(c) < 0x10000 for c in text) and not all(valid(d) for d in hand)
    pool = bs.make_pool(getattr(bs, name + "_HAND"), getattr(bs, name + "_LETTERS"), 64, 1)
    assert pool[:len(hand)] == hand and len(pool) == 64
    if name == "WORD":
        vocab = {k.encode(): i for k, i in VOCAB.items()}
        counts = np.diff(bs.ref_wordpiece(pool, vocab, 0, 6)[0].astype(np.int64))
        unk = [bs.ref_wordpiece([d], vocab, 0, 6)[1].tolist() == [0] for d in hand]
    elif name == "TEXT":
        counts = np.diff(bs.ref_split(pool, Split.Gpt2)[0].astype(np.int64))
        unk = [c == 0 for c in counts[:len(hand)]]
    elif name == "SPECIAL":
        spec = [(b"<|e|>", 7), (b"<|end|>", 9), (b"<|", 11)]
        off, _, sv = bs.ref_cut(pool, spec)
        counts = np.diff(off.astype(np.int64))   # segments
        unk = [(sv[int(a):int(b)] == sg.TEXT).all() for a, b in zip(off, off[1:])][:len(hand)]   # no special
        assert any((sv[int(a):int(b)] != sg.TEXT).all() and b - a >= 2 for a, b in zip(off, off[1:]))   # all specials
    else:
        image = ng.rules_image(*da.bert_normalizer_rules(*ng.OPTIONS["default"]))
        off, out, _ = bs.ref_normalize(pool, image)
        counts = np.diff(off.astype(np.int64))
        unk = [out[int(a):int(b)].tobytes() == d for d, a, b in zip(hand, off, off[1:])]   # unchanged by the normalizer
        assert any(len(d) and a == b for d, a, b in zip(hand, off, off[1:]))                # normalized away
    assert (counts[:len(hand)] == 0).any() and (counts[:len(hand)] >= 3).any() and any(unk) and not all(unk)


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("empty", [False, True])
def test_expand_equals_the_loop_for_the_scans(charwise, empty):
    for mode in MODES:
        o = _oracle(mode, charwise, empty)
        pool = _pool(charwise, keep=lambda d: bs.terminates(o, mode, d))
        counts, sums, tuples = bs.ref_scan(o, mode, pool)
        idx, _, _ = bs.pooled(pool, N, 5, pins=bs.pins_of(counts, pool), turns=(1000,))
        ms = [getattr(o, bs.API[mode])(pool[i]) for i in idx.tolist()]
        assert counts[idx].tolist() == [len(m) for m in ms] and sums[idx].tolist() == [orc.matches_checksum(m) for m in ms]
        off, start, end, value = bs.expand(tuples, idx)
        assert off.tolist() == [0] + np.cumsum([len(m) for m in ms]).tolist()
        whole = np.concatenate(ms)
        _same((start, end, value), (whole["start"], whole["end"], whole["value"]))
        if not empty:
            from test_gpu_batch_hist import _want
            rows = _want(o, bs.API[mode], [pool[i] for i in idx.tolist()])
            off, slot, count = bs.expand(bs.ref_hist(o, mode, pool), idx)
            assert off.tolist() == [0] + np.cumsum([len(r) for r in rows]).tolist()
            assert list(zip(slot.tolist(), count.tolist())) == [rc for r in rows for rc in r]
            assert slot.dtype == np.uint32 and count.dtype == np.uint32


@pytest.mark.parametrize("charwise", [False, True])
def test_expand_equals_the_loop_for_replace_and_tokenize(charwise):
    from test_gpu_replace import _want as replace_want
    from test_gpu_tokenize import _tokens
    for mode in (ScanMode.Find, ScanMode.LeftmostFind):
        o = _oracle(mode, charwise)
        pool = _pool(charwise)
        idx, _, _ = bs.pooled(pool, N, 6)
        docs = [pool[i] for i in idx.tolist()]
        table = [b"<%d>" % i for i in range(len(bs.BYTE_PATTERNS))]
        off, out = bs.expand(bs.ref_replace(o, mode, pool, table), idx)
        want = [replace_want(o, bs.API[mode], d, table) for d in docs]
        assert out.tobytes() == b"".join(want) and off.tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
        for gap in (Gap.Unk, Gap.Chars, Gap.Bytes, Gap.Skip):
            off, ids, spans = bs.expand(bs.ref_tokenize(o, mode, pool, gap, GID), idx)
            per = [_tokens(bs._b(d), getattr(o, bs.API[mode])(d), gap, GID) for d in docs]
            assert off.tolist() == [0] + np.cumsum([len(i) for i, _ in per]).tolist()
            _same((ids, spans), (np.concatenate([i for i, _ in per]), np.concatenate([s for _, s in per])))
            assert ids.dtype == np.uint32 and spans.dtype == np.uint64 and spans.shape == (len(ids), 2)


@pytest.mark.parametrize("charwise", [False, True])
def test_expand_equals_the_loop_for_bpe_and_unigram(charwise):
    o = _oracle(ScanMode.FindOverlapping, charwise)
    pool = _pool(charwise)
    idx, _, _ = bs.pooled(pool, N, 7)
    docs = [pool[i] for i in idx.tolist()]
    ms = [o.find_overlapping_iter(d) for d in docs]
    n_pat = len(bs.BYTE_PATTERNS)
    for ranks in (None, np.random.default_rng(1).permutation(n_pat).astype(np.uint32)):
        for gap in (Gap.Bytes, Gap.Chars):
            _same(bs.expand(bs.ref_bpe(o, pool, ranks, gap, GID), idx), [bpe_expect(docs, ms, ranks, gap)[j] for j in (2, 0, 1)])
    scores = -np.random.default_rng(2).random(n_pat).astype(np.float32) * 3
    for gap in (Gap.Bytes, Gap.Chars):
        toks, sc = bs.ref_unigram(o, pool, scores, -2.5, gap, GID)
        w_ids, w_sp, w_off, w_sc, _ = unigram_expect(o, docs, scores, -2.5, gap)
        _same(bs.expand(toks, idx), (w_off, w_ids, w_sp))
        assert np.array_equal(_bits(sc[idx]), _bits(w_sc))


def test_expand_equals_the_loop_for_wordpiece():
    import wordpiece_golden as wg
    from test_gpu_tokenize_wordpiece import _flat
    vocab = {k.encode(): i for k, i in VOCAB.items()}
    pool = bs.make_pool(bs.WORD_HAND, bs.WORD_LETTERS, 64, 4)
    skip_pool = (np.arange(len(pool)) % 5 == 3).astype(np.uint8)
    idx, _, _ = bs.pooled(pool, N, 8)
    full = [wg.wordpiece(pool[i], vocab, 0, 6) for i in idx.tolist()]
    _same(bs.expand(bs.ref_wordpiece(pool, vocab, 0, 6), idx), [_flat(full)[j] for j in (2, 0, 1)])
    skipped = [[] if skip_pool[i] else t for i, t in zip(idx.tolist(), full)]
    _same(bs.expand(bs.ref_wordpiece(pool, vocab, 0, 6, skip_pool), idx), [_flat(skipped)[j] for j in (2, 0, 1)])
    assert any(t and t[0][0] == 0 for t in full) and any(len(t) > 1 for t in full)


@pytest.mark.parametrize("rule", [Split.Whitespace, Split.Gpt2, Split.Cl100k, Split.Llama3, Split.Bert, Split.O200k])
def test_expand_equals_the_loop_for_split(rule):
    import wordpiece_golden as wg
    pool = bs.make_pool(bs.TEXT_HAND, bs.TEXT_LETTERS, 96, 5, max_letters=8)
    idx, _, off = bs.pooled(pool, N, 9)
    docs = [pool[i] for i in idx.tolist()]
    for base in (0, 37, (1 << 32) + 3):
        wo, dw, space = bs.expand_split(bs.ref_split(pool, rule), idx, off + base)
        w_wo, w_dw = bs.split_scan_batch(docs, rule, base)
        _same((wo, dw), (w_wo, w_dw))
        assert wo.dtype == np.uint64 and dw.dtype == np.uint64 and space.dtype == np.uint8
    if rule == Split.Bert:
        assert np.array_equal(space, wg.bert_offsets(docs, wg.class_table(da.bert_char_classes()))[2])
    assert 0 < space.sum() < len(space)


def test_expand_equals_the_loop_for_cut():
    spec = [(b"<|e|>", 7), (b"<|end|>", 9), (b"<|", 11)]
    pool = bs.make_pool(bs.SPECIAL_HAND, bs.SPECIAL_LETTERS, 64, 6)
    idx, _, off = bs.pooled(pool, N, 10)
    docs = [pool[i] for i in idx.tolist()]
    for base in (0, 5, (1 << 32) - 100):
        got = bs.expand_cut(bs.ref_cut(pool, spec), idx, off + base)
        _same(got, sg.cut(docs, lambda d: sg.leftmost(d, spec), base))
    assert (got[2] != sg.TEXT).sum() > N // 4


def test_expand_equals_the_loop_for_normalize():
    image = ng.rules_image(*da.bert_normalizer_rules(*ng.OPTIONS["default"]))
    pool = bs.make_pool(bs.NORM_HAND, bs.NORM_LETTERS, 64, 7)
    idx, _, _ = bs.pooled(pool, N, 11)
    out, off, src = ng.scan_batch([pool[i] for i in idx.tolist()], image)
    g_off, g_out, g_src = bs.expand(bs.ref_normalize(pool, image), idx)
    assert g_out.tobytes() == out and g_off.tolist() == off and g_src.tolist() == src and g_src.dtype == np.uint32


def test_expand_equals_the_loop_for_the_chains():
    """tokenize_bpe_docs and tokenize_wordpiece_docs, with and without special tokens: the per-pool-document results expanded equal one
    run of special_golden.tokenize_docs over the whole batch (whose cut and splice walk the documents in order)"""
    import wordpiece_golden as wg
    spec = [(b"<|e|>", 7), (b"<|end|>", 9), (b"<|", 11)]
    o = _oracle(ScanMode.FindOverlapping)
    vocab = {k.encode(): i for k, i in VOCAB.items()}
    image = ng.rules_image(*da.bert_normalizer_rules(*ng.OPTIONS["default"]))
    pool = bs.make_pool(bs.SPECIAL_HAND + bs.TEXT_HAND[1:], bs.SPECIAL_LETTERS + bs.TEXT_LETTERS, 96, 12, max_letters=8)
    idx, _, _ = bs.pooled(pool, N, 13)
    docs = [pool[i] for i in idx.tolist()]
    scan = lambda d: sg.leftmost(d, spec)
    for ref in (lambda p, s: bs.ref_bpe_docs(o, p, Split.Gpt2, None, Gap.Bytes, GID, s), lambda p, s: bs.ref_bpe_docs(o, p, Split.Cl100k, None, Gap.Chars, GID, s),
                lambda p, s: bs.ref_wordpiece_docs(p, vocab, 0, 6, None, s), lambda p, s: bs.ref_wordpiece_docs(p, vocab, 0, 6, image, s)):
        for s in (None, spec):
            _same(bs.expand(ref(pool, s), idx), ref(docs, s))
    # with specials, the batch's own cut and splice in one go equal the per-document runs
    table = wg.class_table(da.bert_char_classes())
    per = sg.tokenize_docs(docs, scan, lambda seg: wg.wordpiece_doc(seg, table, vocab, 0, 6))
    off, ids, spans = bs.expand(bs.ref_wordpiece_docs(pool, vocab, 0, 6, None, spec), idx)
    assert off.tolist() == [0] + np.cumsum([len(i) for i, _ in per]).tolist() and ids.tolist() == [x for i, _ in per for x in i]
    assert [tuple(x) for x in spans.tolist()] == [x for _, s in per for x in s]
