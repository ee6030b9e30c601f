"""normalize_batch on the MI355X (daac_normalize_batch / daac_normalize / daac_spans_to_source, tokenize_wordpiece_docs(normalizer=..)).
Expected bytes are `tokenizers`' BertNormalizer.normalize_str and expected tokens the full Tokenizer's (BertNormalizer + BertPreTokenizer +
WordPiece), as tests/golden/normalize_cases.json holds them; for shapes, the sequential scanner of tests/normalize_golden.py over the
rules, which the host tests hold against the fixture and `tokenizers`; never the library.  Every comparison is exact: bytes, offsets,
src, ids and spans.  There is no tolerance in this feature."""
import functools

import numpy as np
import pytest
import torch

import normalize_golden as ng
import wordpiece_golden as wg

pytestmark = pytest.mark.gpu

import daachorse_amd as da

TILE = 1024   # kNormTile
E_ACUTE, CJK, WIDE, HANGUL3, HANGUL2 = "\u00c9".encode(), "\u4e2d".encode(), "\U00020000".encode(), "\ud55c".encode(), "\uac00".encode()


@functools.lru_cache(maxsize=None)
def _image(name="default"):
    return ng.rules_image(*da.bert_normalizer_rules(*ng.OPTIONS[name]))


def _nz(name="default"):
    return da.bert_normalizer(*ng.OPTIONS[name])


def _device_batch(docs, front=0):
    off = np.full(len(docs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(b"\xe3" * front + b"".join(docs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _check(docs, what, name="default", front=3):
    """host and device documents, with and without src, against the sequential scanner"""
    nz = _nz(name)
    out, off, src = ng.scan_batch(docs, _image(name))
    want = (np.frombuffer(out, dtype=np.uint8), np.array(off, dtype=np.uint64), np.array(src, dtype=np.uint32))
    for batch, where in ((docs, "host"), (_device_batch(docs, front), "device")):
        got = nz.normalize_batch(batch, src=True)
        assert len(got) == 3
        for g, w, part in zip(got, want, ("out", "out_offsets", "src")):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, where, part)
        got = nz.normalize_batch(batch)
        assert len(got) == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, where, "no src")
    return want


# ----------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", sorted(ng.OPTIONS))
def test_the_fixture_in_one_batch(name):
    docs, want = ng.docs(), ng.expected(name)
    out, off, _ = _check(docs, name, name)
    assert out.tobytes() == b"".join(want) and off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()   # the scanner is tokenizers' bytes
    assert da.last_kernel().startswith("normalize rules="), da.last_kernel()


@pytest.mark.parametrize("name", sorted(ng.OPTIONS))
def test_the_fixture_at_the_batch_sizes(name):
    docs, want = ng.docs(), ng.expected(name)
    nz = _nz(name)
    for n in (63, 64, 65, 257):
        at = (7 * n) % (len(docs) - n)
        w = want[at:at + n]
        for batch in (docs[at:at + n], _device_batch(docs[at:at + n], front=1)):
            out, off = nz.normalize_batch(batch)
            assert out.tobytes() == b"".join(w) and off.tolist() == np.cumsum([0] + [len(x) for x in w]).tolist(), (name, n)


def test_one_haystack_and_device_results():
    nz = _nz()
    docs = ng.docs()
    text = b"".join(docs[:40])
    want_out, _, want_src = ng.scan_batch([text], _image())
    out, src = nz.normalize(text, src=True)
    assert out.tobytes() == want_out and src.tolist() == want_src and src.dtype == np.uint32
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    assert nz.normalize(dev).tobytes() == want_out
    assert nz.normalize(b"").shape == (0,)
    res = nz.normalize_batch(docs[:40], src=True, device=True)
    _, want_off, want_src = ng.scan_batch(docs[:40], _image())   # src counts from each document's start
    try:
        assert res[0].to_numpy().tobytes() == want_out and res[1].to_numpy().tolist() == want_off and res[2].to_numpy().tolist() == want_src
    finally:
        for r in res:
            r.free()


# ------------------------------------------------------------------------------------------- shapes where the passes can go wrong
@pytest.mark.parametrize("unit", [E_ACUTE, CJK, WIDE, HANGUL3], ids=["2 bytes", "3 bytes", "4 bytes", "hangul"])
def test_a_unit_begun_at_the_last_positions_of_a_tile(unit):
    for tile in (0, 1):
        for back in (1, 2, 3):
            at = (tile + 1) * TILE - back
            whole = b"a" * at + unit + b"B" * 5
            _check([whole], (at, "one document"))
            _check([b"x" * 7, whole[7:]], (at, "a document in front"), front=1)
            for cut in range(1, len(unit)):   # a document boundary inside the unit: its bytes are ill-formed on either side and copied
                _check([whole[:at + cut], whole[at + cut:]], (at, cut))


def test_three_tiles_of_hangul():
    docs = [HANGUL3 * TILE]          # 3 tiles of text, every unit triples
    out, off, src = _check(docs, "hangul")
    assert len(out) == 9 * TILE and src[9 * 700] == 3 * 700
    _check([HANGUL3 * 300, HANGUL2 * 341 + b"a", (HANGUL3 + HANGUL2) * 200], "hangul, three documents", front=5)


def test_three_tiles_of_deleted_characters_then_one_kept_byte():
    out, off, src = _check([b"\0" * (3 * TILE) + b"a"], "tile counts of 0")
    assert out.tobytes() == b"a" and src.tolist() == [3 * TILE]
    _check([b"\0" * (3 * TILE)], "nothing is kept")
    _check([b"\0" * TILE, "\u200d".encode() * TILE, b"Q"], "tile counts of 0, three documents")


def test_a_pad_unit_first_and_last_in_a_tile():
    doc = CJK + b"a" * (TILE - 6) + CJK + CJK + b"b" * (TILE - 6) + WIDE[:3]
    _check([doc], "pad at the tile edges")
    _check([doc[:TILE], doc[TILE:]], "pad at the tile edges, a document per tile")


def test_empty_documents_and_documents_that_become_empty():
    gone = "\0\u200d\ufffd\ue000".encode()
    _check([b"", b"", b"Ab", b"", b"", "\u00c9".encode(), b"", b""], "empty documents at the front, in the middle and at the end")
    _check([b"Ab", gone, b"cD"], "a document that normalizes to nothing between two that do not")
    _check([gone, b"", gone], "nothing at all")
    _check([b"", b""], "only empty documents")
    _check([b"a" * (TILE - 1), b"", b"", b"B", b"", b"c" * TILE, b""], "empty documents at a tile edge")


def test_offsets_that_start_at_an_odd_address():
    docs = ng.docs()[:50]
    want_out, want_off, want_src = ng.scan_batch(docs, _image())
    hay, off = _device_batch(docs, front=7)
    view = hay[1:]   # the buffer's address is odd; the offsets count from it
    assert view.data_ptr() % 2 == 1
    out, oo, src = _nz().normalize_batch((view, off - 1), src=True)
    assert out.tobytes() == want_out and oo.tolist() == want_off and src.tolist() == want_src


def test_no_document():
    nz = _nz()
    out, off, src = nz.normalize_batch([], src=True)
    assert out.shape == (0,) and off.tolist() == [0] and src.shape == (0,) and src.dtype == np.uint32
    out, off = nz.normalize_batch((torch.zeros(4, dtype=torch.uint8).cuda(), torch.zeros(1, dtype=torch.int64).cuda()))
    assert out.shape == (0,) and off.tolist() == [0]


def test_positions_beyond_2_to_the_31_and_more_than_2_to_the_20_tiles():
    """2 GiB of deleted characters with four kept ones: 64-bit positions in both passes, the grid's second dimension, a document
    start far into the text, src that counts from it"""
    n, cut = (1 << 31) + 3 * TILE + 5, (1 << 30) + 7
    tail = "Ab\u00c9".encode()
    hay = torch.zeros(n, dtype=torch.uint8, device="cuda")
    hay[cut] = ord("Z")
    hay[n - len(tail):] = torch.tensor(list(tail), dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, cut, n], dtype=torch.int64, device="cuda")
    out, oo, src = _nz().normalize_batch((hay, off), src=True)
    assert out.tobytes() == b"zabe" and oo.tolist() == [0, 0, 4]
    assert src.tolist() == [0, n - 4 - cut, n - 3 - cut, n - 2 - cut]
    out, oo = _nz().normalize_batch((hay, off))
    assert out.tobytes() == b"zabe" and oo.tolist() == [0, 0, 4]


def test_a_document_of_2_to_the_32_minus_1_bytes_with_src_answers_6():
    n = (1 << 32) - 1
    hay = torch.empty(n + 1, dtype=torch.uint8, device="cuda")   # (its content does not matter: the answer is given before the write pass)
    off = torch.tensor([0, 1, n + 1], dtype=torch.int64, device="cuda")
    with pytest.raises(da.DaachorseError) as ei:
        _nz().normalize_batch((hay, off), src=True)
    assert ei.value.code == 6 and "2^32" in str(ei.value)
    del hay
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out, oo, src = _nz().normalize_batch((small, torch.tensor([0, 64], dtype=torch.int64, device="cuda")), src=True)   # the next call is served
    assert out.shape == (0,) and oo.tolist() == [0, 0]


def test_ill_formed_bytes_are_copied():
    docs = [b"A\xc3(\xe4\xb8", b"\x80\xbf\xff", b"\xed\xa0\x80Z", b"\xf4\x90\x80\x80", b"\xc0\xaf", b"\xe4\xb8", b"\xadX"]
    out, _, _ = _check(docs, "ill-formed")
    assert out.tobytes() == b"a\xc3(\xe4\xb8\x80\xbf\xff\xed\xa0\x80z\xf4\x90\x80\x80\xc0\xaf\xe4\xb8\xadx"


def test_a_rule_set_of_ones_own():
    """every kind on ASCII too, an image of the longest length, a range that shares one image"""
    pool = b"z" * 255 + b"-"
    nz = da.Normalizer([(0x30, 0x39, 2, 255, 1), (0x41, 0x41, 1, 0, 0), (0x42, 0x42, 2, 0, 255), (0x43, 0x43, 3, 0, 0), (0x44, 0x44, 2, 0, 0), (0xAC00, 0xD7A3, 4, 0, 0)], pool)
    image = ng.rules_image(nz.rules, nz.pool)
    docs = [b"A1B2C3D4e" * 300, HANGUL2 + b"B" * 9, b"", b"C" * 2000]
    want = ng.scan_batch(docs, image)
    out, off, src = nz.normalize_batch(docs, src=True)
    assert out.tobytes() == want[0] and off.tolist() == want[1] and src.tolist() == want[2]
    nz.free()


def test_an_output_above_max_result_bytes_answers_2():
    nz = _nz()
    da.set_option("max_result_bytes", 64)
    try:
        with pytest.raises(da.DaachorseError) as ei:
            nz.normalize_batch([b"a" * 65])
        assert ei.value.code == 2 and "max_result_bytes" in str(ei.value)
        with pytest.raises(da.DaachorseError) as ei:
            nz.normalize_batch([b"a" * 13], src=True)   # 5 bytes per output byte
        assert ei.value.code == 2
        assert nz.normalize_batch([b"A" * 12], src=True)[0].tobytes() == b"a" * 12
    finally:
        da.set_option("max_result_bytes", 8 << 30)


def test_decreasing_device_offsets_answer_1():
    hay = torch.zeros(64, dtype=torch.uint8).cuda()
    off = torch.tensor([0, 10, 5, 20], dtype=torch.int64).cuda()
    with pytest.raises(da.DaachorseError) as ei:
        _nz().normalize_batch((hay, off))
    assert ei.value.code == 1 and "document 1" in str(ei.value)


# ------------------------------------------------------------------------------------------------------------- spans_to_source
def test_spans_to_source_on_the_device():
    docs = ["\ud55c\u00c9\u4e2dx".encode(), b"", b"A\0b", "\0\u200d".encode(), b"q"]
    nz = _nz()
    spans = [[(0, 3), (3, 6), (6, 9), (9, 10), (11, 14), (15, 16), (0, 0), (10, 10), (16, 16)], [], [(0, 1), (1, 2), (0, 2), (2, 2)], [(0, 0)], [(0, 1)]]
    want = []
    for d, sp in zip(docs, spans):
        _, src = ng.scan(d, _image())
        want += ng.spans_to_source(sp, src, d)
    assert want[:6] == [(0, 3)] * 3 + [(3, 5), (5, 8), (8, 9)] and want[9:13] == [(0, 1), (2, 3), (0, 3), (3, 3)] and want[13] == (4, 4)
    tok_off = torch.tensor(np.cumsum([0] + [len(s) for s in spans]), dtype=torch.int64).cuda()
    for batch in (docs, _device_batch(docs, front=3)):
        out, oo, src = nz.normalize_batch(batch, src=True, device=True)
        try:
            t = torch.tensor([x for sp in spans for s in sp for x in s], dtype=torch.int64).reshape(-1, 2).cuda()
            da.Normalizer.spans_to_source(t, tok_off, oo, src, batch)
            assert t.cpu().tolist() == [list(w) for w in want]
        finally:
            for r in (out, oo, src):
                r.free()


# ------------------------------------------------------------------------------------------------- tokenize_wordpiece_docs
@pytest.fixture(scope="module")
def model():
    patterns, first, cont = da.wordpiece_tables(wg.load("vocab")["vocab"])
    pmas = {False: da.DoubleArrayAhoCorasick.new(patterns), True: da.CharwiseDoubleArrayAhoCorasick.new([p.decode() for p in patterns])}
    _, unk_id, max_chars, _ = wg.model()
    return pmas, first, cont, unk_id, max_chars


def _flat(ids, spans):
    return (np.array([i for a in ids for i in a], dtype=np.uint32), np.array([s for b in spans for s in b], dtype=np.uint64).reshape(-1, 2),
            np.cumsum([0] + [len(a) for a in ids]).astype(np.uint64))


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what


@pytest.mark.parametrize("charwise", [False, True])
def test_wordpiece_docs_with_the_normalizer_equal_tokenizers_from_raw_text(model, charwise):
    pmas, first, cont, unk_id, max_chars = model
    docs = ng.docs()
    want = _flat(*ng.tokens())
    p, nz = pmas[charwise], da.bert_normalizer()
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, spans=True, normalizer=nz), want, "host documents")
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, normalizer=nz), (want[0], want[2]), "no spans")
    out = p.tokenize_wordpiece_docs(_device_batch(docs, front=5), first, cont, unk_id, max_chars, spans=True, device=True, normalizer=nz)
    try:
        _same([o.to_numpy() for o in out], want, "device documents, device results")
    finally:
        for o in out:
            o.free()
    _same(p.tokenize_wordpiece_docs([], first, cont, unk_id, max_chars, spans=True, normalizer=nz), _flat([], []), "no document")
    _same(p.tokenize_wordpiece_docs([b"", b"\0\0", b" \t"], first, cont, unk_id, max_chars, spans=True, normalizer=nz), _flat([[], [], []], [[], [], []]), "no token")
    with pytest.raises(da.DaachorseError):
        p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, normalizer="bert")


def test_the_readme_recipe(model):
    """H\u00e9llo WORLD through an uncased vocabulary: [UNK] [UNK] without the normalizer, pieces with it"""
    vocab = {"[UNK]": 0, "hello": 1, "world": 2, "##s": 3}
    patterns, first, cont = da.wordpiece_tables(vocab)
    p = da.DoubleArrayAhoCorasick.new(patterns)
    text = "H\u00e9llo WORLDS".encode()
    ids, spans, off = p.tokenize_wordpiece_docs([text], first, cont, 0, spans=True)
    assert ids.tolist() == [0, 0]
    ids, spans, off = p.tokenize_wordpiece_docs([text], first, cont, 0, spans=True, normalizer=da.bert_normalizer())
    assert ids.tolist() == [1, 2, 3] and spans.tolist() == [[0, 6], [7, 12], [12, 13]] and off.tolist() == [0, 3]


@pytest.mark.parametrize("charwise", [False, True])
def test_wordpiece_docs_without_a_normalizer_are_unchanged(model, charwise):
    pmas, first, cont, unk_id, max_chars = model
    docs, ids, tok_spans, _ = wg.cases()
    want = _flat(ids, tok_spans)
    _same(pmas[charwise].tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, spans=True, normalizer=None), want, "normalizer=None")
    _same(pmas[charwise].tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, spans=True), want, "no normalizer argument")
    assert da.last_kernel().startswith("wordpiece docs="), da.last_kernel()
