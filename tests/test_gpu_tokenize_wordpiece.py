"""tokenize_wordpiece on the MI355X (daac_tokenize_wordpiece / daac_tokenize_wordpiece_batch, tokenize_wordpiece_docs).  Expected tokens
are `tokenizers`' (models.WordPiece behind BertPreTokenizer), as the fixtures of tests/golden/ hold them, and for hand cases the
pure-Python definition of tests/wordpiece_golden.py, which the fixture generator checked against `tokenizers` on every document; never
the library.  Every comparison is exact: ids, spans and offsets.  There is no tolerance in this feature."""
import numpy as np
import pytest
import torch

import tokenizer_golden as tg
import wordpiece_golden as wg

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Split

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def model():
    """-> {charwise: automaton}, first_ids, cont_ids, unk_id, max_chars of the fixture vocabulary"""
    patterns, first, cont = da.wordpiece_tables(wg.load("vocab")["vocab"])
    pmas = {False: da.DoubleArrayAhoCorasick.new(patterns), True: da.CharwiseDoubleArrayAhoCorasick.new([p.decode() for p in patterns])}
    _, unk_id, max_chars, _ = wg.model()
    return pmas, first, cont, unk_id, max_chars


def _flat(tokens_per_doc):
    """[[(id, start, end)]] -> ids, spans, offsets as the batch calls give them"""
    ids = np.array([t[0] for toks in tokens_per_doc for t in toks], dtype=np.uint32)
    spans = np.array([t[1:] for toks in tokens_per_doc for t in toks], dtype=np.uint64).reshape(-1, 2)
    offs = np.cumsum([0] + [len(toks) for toks in tokens_per_doc]).astype(np.uint64)
    return ids, spans, offs


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what


def _device_batch(docs, front=0):
    off = np.full(len(docs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(b"\xe3" * front + b"".join(docs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


# ----------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("charwise", [False, True])
def test_docs_equal_tokenizers_on_every_fixture_document(model, charwise):
    pmas, first, cont, unk_id, max_chars = model
    docs, ids, tok_spans, _ = wg.cases()
    want = _flat([[(i, s, e) for i, (s, e) in zip(a, b)] for a, b in zip(ids, tok_spans)])
    p = pmas[charwise]
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, spans=True), want, "host documents")
    assert da.last_kernel().startswith("wordpiece docs="), da.last_kernel()
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars), (want[0], want[2]), "no spans")
    out = p.tokenize_wordpiece_docs(_device_batch(docs, front=5), first, cont, unk_id, max_chars, spans=True, device=True)
    try:
        _same([o.to_numpy() for o in out], want, "device documents, device results")
    finally:
        for o in out:
            o.free()
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, split=da.Splitter(Split.Bert, da.bert_char_classes()), spans=True), want, "a Splitter")


@pytest.mark.parametrize("charwise", [False, True])
def test_word_batches_at_the_lane_edges(model, charwise):
    pmas, first, cont, unk_id, max_chars = model
    words, tokens = wg.distinct_words()
    assert len(words) >= max(tg.BATCH_SIZES)
    p = pmas[charwise]
    for n in tg.BATCH_SIZES:
        at = (7 * n) % (len(words) - n)
        _same(p.tokenize_wordpiece_batch(words[at:at + n], first, cont, unk_id, max_chars, spans=True), _flat(tokens[at:at + n]), n)
    _same(p.tokenize_wordpiece_batch(_device_batch(words, front=1), first, cont, unk_id, max_chars, spans=True), _flat(tokens), "all words, device")
    for k in range(0, len(words), 97):   # the single-word call equals the batch of one
        ids, spans = p.tokenize_wordpiece(words[k], first, cont, unk_id, max_chars, spans=True)
        b_ids, b_spans, b_off = p.tokenize_wordpiece_batch([words[k]], first, cont, unk_id, max_chars, spans=True)
        _same((ids, spans), (b_ids, b_spans), words[k])
        _same((ids, spans, b_off), _flat([tokens[k]]), words[k])
    w = torch.from_numpy(np.frombuffer(words[0], dtype=np.uint8).copy()).cuda()
    _same((p.tokenize_wordpiece(w, first, cont, unk_id, max_chars),), (_flat([tokens[0]])[0],), "a device word")


# ------------------------------------------------------------------------------------------------------------- edge cases
def _hand(vocab, charwise=False):
    patterns, first, cont = da.wordpiece_tables(vocab)
    new = da.CharwiseDoubleArrayAhoCorasick.new if charwise else da.DoubleArrayAhoCorasick.new
    return new([p.decode() for p in patterns] if charwise else patterns), first, cont, {k.encode(): i for k, i in vocab.items()}


VOCAB = {"[UNK]": 0, "un": 1, "##able": 2, "able": 3, "##s": 4, "a": 5, "##a": 6, "##b": 7, "b": 8, "é": 9, "##é": 10, "!": 11, "、": 12, "ab": 13, "##ab": 14,
         "abc": 15, "##c": 16, "##bc": 17}


@pytest.mark.parametrize("charwise", [False, True])
def test_empty_batches_and_empty_documents(charwise):
    p, first, cont, v = _hand(VOCAB, charwise)
    table = wg.class_table(da.bert_char_classes())
    ids, spans, off = p.tokenize_wordpiece_batch([], first, cont, 0, spans=True)
    assert ids.shape == (0,) and spans.shape == (0, 2) and off.tolist() == [0]
    ids, off = p.tokenize_wordpiece_docs([], first, cont, 0)
    assert ids.shape == (0,) and off.tolist() == [0]
    assert p.tokenize_wordpiece(b"", first, cont, 0).shape == (0,)
    docs = [b"", b"unable", b"", b"", b"abs!", b""]
    want = _flat([wg.wordpiece(d, v, 0, 100) for d in docs])
    assert want[2].tolist() == [0, 0, 2, 2, 2, 3, 3]   # "abs!" is no word: [UNK]
    _same(p.tokenize_wordpiece_batch(docs, first, cont, 0, spans=True), want, "words")
    docs = [b"", b" \t\n", "　 ".encode(), "!!、!".encode(), b"unable  abs!", b"", b"...", b""]
    per_doc = []
    for d in docs:
        i, s = wg.wordpiece_doc(d, table, v, 0, 100)
        per_doc.append([(a, b, c) for a, (b, c) in zip(i, s)])
    want = _flat(per_doc)
    assert want[2].tolist()[:5] == [0, 0, 0, 0, 4]     # only whitespace: no tokens; only punctuation: one token each
    _same(p.tokenize_wordpiece_docs(docs, first, cont, 0, spans=True), want, "documents")
    _same(p.tokenize_wordpiece_docs([b"", b""], first, cont, 0, spans=True), _flat([[], []]), "all empty")
    _same(p.tokenize_wordpiece_docs([b"  ", b"\n"], first, cont, 0, spans=True), _flat([[], []]), "all whitespace")


def test_skip_flags():
    p, first, cont, v = _hand(VOCAB)
    words = [b"unable", b"abs", b"", b"a", b"zzz"]
    full = [wg.wordpiece(w, v, 0, 100) for w in words]
    for skip in ([0, 1, 0, 0, 0], [1, 0, 1, 0, 255], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]):
        want = _flat([[] if s else t for s, t in zip(skip, full)])
        _same(p.tokenize_wordpiece_batch(words, first, cont, 0, skip=np.array(skip, dtype=np.uint8), spans=True), want, skip)
        _same(p.tokenize_wordpiece_batch(words, first, cont, 0, skip=torch.tensor(skip, dtype=torch.uint8).cuda(), spans=True), want, skip)
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_wordpiece_batch(words, first, cont, 0, skip=np.zeros(4, dtype=np.uint8))
    assert ei.value.code == 1 and "skip" in str(ei.value)


@pytest.mark.parametrize("charwise", [False, True])
def test_the_character_cap_counts_characters_not_bytes(charwise):
    p, first, cont, v = _hand(VOCAB, charwise)
    e = "é".encode()
    for max_chars in (1, 3, 4):
        words = [e * max_chars, e * (max_chars + 1), b"a" * max_chars, b"a" * (max_chars + 1), (b"a" + e) * max_chars, e * (max_chars - 1) + b"ab"]
        want = [wg.wordpiece(w, v, 0, max_chars) for w in words]
        assert len(want[0]) == max_chars and len(words[0]) > max_chars       # exactly max_chars characters, more bytes: segmented
        assert want[1] == [(0, 0, 2 * max_chars + 2)] and want[3] == [(0, 0, max_chars + 1)]
        _same(p.tokenize_wordpiece_batch(words, first, cont, 0, max_chars, spans=True), _flat(want), max_chars)
    _same(p.tokenize_wordpiece_batch([b"a" * 300, b"a" * 101], first, cont, 0, 0xFFFFFFFF, spans=True), _flat([[(5, 0, 1)] + [(6, i, i + 1) for i in range(1, 300)],
                                                                                                                 [(5, 0, 1)] + [(6, i, i + 1) for i in range(1, 101)]]), "no cap")
    _same(p.tokenize_wordpiece_batch([b"a" * 100, b"a" * 101], first, cont, 0)[1:], (np.array([0, 100, 101], dtype=np.uint64),), "BERT's 100")


@pytest.mark.parametrize("charwise", [False, True])
def test_whole_word_unk_and_roles(charwise):
    p, first, cont, v = _hand(VOCAB, charwise)
    cases = {b"unablez": [(0, 0, 7)],                 # the only failure is the last character
             b"unable": [(1, 0, 2), (2, 2, 6)],
             b"ableun": [(0, 0, 6)],                  # "un" is no continuation piece
             b"sable": [(0, 0, 5)],                   # "s" is no initial piece
             b"abs": [(13, 0, 2), (4, 2, 3)],
             b"abcab": [(15, 0, 3), (14, 3, 5)],      # the longest piece first, in either role
             b"aabc": [(5, 0, 1), (14, 1, 3), (16, 3, 4)],
             b"z": [(0, 0, 1)]}
    for w, want in cases.items():
        assert wg.wordpiece(w, v, 0, 100) == want, w
    _same(p.tokenize_wordpiece_batch(list(cases), first, cont, 0, spans=True), _flat(list(cases.values())), "hand")
    _same(p.tokenize_wordpiece_batch(list(cases), first, cont, 0xFFFFFFFE)[:1], (np.array([0xFFFFFFFE if i == 0 else i for t in cases.values() for i, _, _ in t],
                                                                                           dtype=np.uint32),), "another unk_id")


@pytest.mark.parametrize("charwise", [False, True])
def test_an_empty_pattern_and_values_with_gaps(charwise):
    """"" among the patterns matches everywhere and is no piece; values far apart leave most of the two tables at NONE"""
    cls = da.CharwiseDoubleArrayAhoCorasick if charwise else da.DoubleArrayAhoCorasick
    pats = ["", "un", "able", "s", "é"]
    vals = [40, 3, 1000, 77, 500]
    p = cls.with_values(list(zip(pats, vals)))
    first, cont = np.full(1001, NONE, dtype=np.uint32), np.full(1001, NONE, dtype=np.uint32)
    first[40], cont[40] = 90, 91           # ids for "": never used
    first[3], first[1000], cont[1000], cont[77], first[500], cont[500] = 1, 3, 2, 4, 9, 10
    v = {b"un": 1, b"able": 3, b"##able": 2, b"##s": 4, "é".encode(): 9, "##é".encode(): 10}
    words = [b"unable", b"ables", b"sable", b"unx", b"", "éés".encode(), b"un"]
    want = [wg.wordpiece(w, v, 0, 100) for w in words]
    assert want[1] == [(3, 0, 4), (4, 4, 5)] and want[3] == [(0, 0, 3)]
    got = p.tokenize_wordpiece_batch(words, first, cont, 0, spans=True)
    _same(got, _flat(want), "gaps")
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_wordpiece_batch(words, first[:1000], cont[:1000], 0)
    assert ei.value.code == 1 and "n_ids" in str(ei.value)
