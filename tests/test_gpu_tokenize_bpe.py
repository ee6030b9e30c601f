"""tokenize_bpe on the MI355X (daac_tokenize_bpe / daac_tokenize_bpe_batch): byte-pair merging in rank order.  Expected tokens come from
a pure-Python restatement of the definition (`_bpe`) over the CPU oracle's find_overlapping_iter matches of each document, never from
the library.  Every comparison is exact: ids, spans and tok_offsets.  There is no tolerance in this feature.

The merge loop costs (merges x live parts) on one lane and as much in `_bpe`, so the long documents here (3000 and 4096 bytes) are mostly
bytes the vocabulary lacks, with words scattered through them: a few dozen merges each."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap

GID = 0x10000   # keeps byte ids apart from values
NO = 0xFFFFFFFF


def _pair(patterns, charwise=False, values=None, kind=0):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p


def _b(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def _cuts(doc, gap):
    L = len(doc)
    return [0] + [p for p in range(1, L) if gap == Gap.Bytes or (doc[p] & 0xC0) != 0x80] + ([L] if L else [])


def _pieces(m):
    return {(s, e): v for s, e, v in zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist()) if s < e}


def _bpe(doc, matches, ranks, gap, gap_id):
    """the definition -> tokens [(id, start, end)]; `matches`: the oracle's find_overlapping_iter(doc)"""
    if not len(doc):
        return []
    piece = _pieces(matches)
    rank = (lambda v: v) if ranks is None else (lambda v: int(ranks[v]))
    b = _cuts(doc, gap)
    while True:
        best, at = NO, None
        for i in range(len(b) - 2):
            v = piece.get((b[i], b[i + 2]))
            if v is not None and rank(v) < best:
                best, at = rank(v), i
        if at is None:
            break
        del b[at + 1]
    return [(piece.get((s, e), gap_id + (doc[s] if gap == Gap.Bytes else 0)), s, e) for s, e in zip(b, b[1:])]


def _matches(o, docs):
    return [o.find_overlapping_iter(d) for d in docs]


def _expect(docs, ms, ranks, gap, gap_id=GID):
    """-> (ids uint32[T], spans uint64[T, 2], offsets uint64[n + 1])"""
    toks, off = [], [0]
    for d, m in zip(docs, ms):
        toks += _bpe(_b(d), m, ranks, gap, gap_id)
        off.append(len(toks))
    a = np.array(toks, dtype=np.uint64).reshape(len(toks), 3)
    return a[:, 0].astype(np.uint32), a[:, 1:].copy(), np.array(off, dtype=np.uint64)


def _device_batch(docs, front=0):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    blobs = [_b(d) for d in docs]
    off = np.full(len(blobs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(b) for b in blobs], dtype=np.int64)
    hay = np.frombuffer(b"\xff" * front + b"".join(blobs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _same(got, want, spans, what):
    ids, sp, off = want
    g_ids, g_sp, g_off = got if spans else (got[0], None, got[1])
    assert g_ids.dtype == np.uint32 and np.array_equal(g_ids, ids), what
    if spans:
        assert g_sp.dtype == np.uint64 and g_sp.shape == (len(ids), 2) and np.array_equal(g_sp, sp), what
    assert g_off.dtype == np.uint64 and np.array_equal(g_off, off), what


def _check_batch(o, p, docs, ranks=None, gaps=(Gap.Bytes, Gap.Chars), front=5, engines=(Engine.Auto, Engine.DArray), what=None):
    """tokenize_bpe_batch(docs) against the definition, host and device batches, spans on and off
    -> {gap: ((ids, spans, offsets) wanted, the library's result with spans, the oracle's matches per document)}"""
    ms = _matches(o, docs)
    out = {}
    for gap in gaps:
        want = _expect(docs, ms, ranks, gap)
        for src, with_spans, eng in ((s, w, e) for s in ("host", "device") for w in (True, False) for e in engines):
            arg = _device_batch(docs, front) if src == "device" else docs
            got = p.tokenize_bpe_batch(arg, ranks, gap=gap, gap_id=GID, spans=with_spans, engine=eng)
            assert da.last_kernel().startswith(f"bpe docs={len(docs)} matches={sum(len(m) for m in ms)} tokens={len(want[0])} "), da.last_kernel()
            _same(got, want, with_spans, (what, gap, src, with_spans, eng))
            if with_spans:
                out[gap] = (want, got, ms)
    return out


def _check_single(o, p, hay, ranks, gap, **kw):
    ids, sp, _ = _expect([hay], _matches(o, [hay]), ranks, gap)
    g_ids, g_sp = p.tokenize_bpe(hay, ranks, gap=gap, gap_id=GID, spans=True, **kw)
    assert g_ids.dtype == np.uint32 and g_sp.dtype == np.uint64 and g_sp.shape == (len(ids), 2)
    assert np.array_equal(g_ids, ids) and np.array_equal(g_sp, sp), (hay, gap)
    assert np.array_equal(p.tokenize_bpe(hay, ranks, gap=gap, gap_id=GID, **kw), ids)
    return ids, sp


def _dev(hay):
    return torch.from_numpy(np.frombuffer(hay, dtype=np.uint8).copy()).cuda()


# --------------------------------------------------------------------------------------------------- 1. the worked examples
def test_merge_order_beats_longest_match():
    pats = [b"a", b"b", b"c", b"bc", b"ab", b"d", b"bcd"]   # values 0 .. 6
    o, p = _pair(pats)
    for gap in (Gap.Bytes, Gap.Chars):
        for hay in (b"abcd", _dev(b"abcd")):
            for eng in (Engine.Auto, Engine.DArray):
                ids, sp = p.tokenize_bpe(hay, gap=gap, gap_id=GID, spans=True, engine=eng)
                assert ids.tolist() == [0, 6] and sp.tolist() == [[0, 1], [1, 4]]
                assert p.tokenize_bpe(hay, gap=gap, gap_id=GID, engine=eng).tolist() == [0, 6]
        _check_single(o, p, b"abcd", None, gap)
    # longest-match-first on a leftmost-longest automaton of the same patterns takes ab first
    lo, lp = _pair(pats, kind=1)
    assert lp.tokenize(b"abcd", gap=Gap.Bytes, gap_id=GID).tolist() == [4, 2, 5]
    # a rank table overrides the values: ab merges first
    ranks = [0, 1, 2, 4, 3, 5, 6]
    for gap in (Gap.Bytes, Gap.Chars):
        ids, sp = p.tokenize_bpe(b"abcd", ranks, gap=gap, gap_id=GID, spans=True)
        assert ids.tolist() == [4, 2, 5] and sp.tolist() == [[0, 2], [2, 3], [3, 4]]
        _check_single(o, p, b"abcd", ranks, gap)
    # the same as a batch, host and device, with offsets[0] != 0
    docs = [b"abcd", b"", b"bcd", b"abcd", b"dcba"]
    res = _check_batch(o, p, docs, what="worked")
    (ids, sp, off), _, _ = res[Gap.Bytes]
    assert ids.tolist() == [0, 6, 6, 0, 6, 5, 2, 1, 0] and off.tolist() == [0, 2, 2, 3, 5, 9] and sp[:2].tolist() == [[0, 1], [1, 4]]
    res = _check_batch(o, p, docs, ranks, what="worked, ranks")
    (ids, sp, off), _, _ = res[Gap.Chars]
    assert ids[:3].tolist() == [4, 2, 5] and off.tolist() == [0, 3, 3, 4, 7, 11]


def test_ties_go_left():
    o, p = _pair([b"a", b"aa"])
    for gap in (Gap.Bytes, Gap.Chars):
        for hay in (b"aaaaa", _dev(b"aaaaa")):
            ids, sp = p.tokenize_bpe(hay, gap=gap, gap_id=GID, spans=True)
            assert ids.tolist() == [1, 1, 0] and sp.tolist() == [[0, 2], [2, 4], [4, 5]]
    res = _check_batch(o, p, [b"aaaaa", b"aa", b"a", b"aaaa"], what="a aa")
    (ids, sp, off), _, _ = res[Gap.Bytes]
    assert ids.tolist() == [1, 1, 0, 1, 0, 1, 1]


# -------------------------------------------------------------------------------------------------------------------- 2. ties
def test_ties():
    rng = np.random.default_rng(7)
    pats = sorted({bytes(rng.choice(list(b"ab"), size=int(rng.integers(1, 5))).tolist()) for _ in range(14)})
    o, p = _pair(pats)
    docs = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) for n in rng.integers(0, 41, size=70)]
    # all ranks equal: every choice is a tie and goes to the leftmost pair
    res = _check_batch(o, p, docs, [5] * len(pats), what="equal")
    (ids, sp, off), _, _ = res[Gap.Bytes]
    assert (ids < GID).any() and len(ids) < sum(len(d) for d in docs)
    # three distinct ranks
    _check_batch(o, p, docs, rng.integers(0, 3, size=len(pats)).tolist(), what="three")


# -------------------------------------------------------------------------------------------------------------------- 3. fuzz
def _legal(doc, toks, spans, m, ranks, gap):
    """the properties that do not depend on the tie rule: the tokens tile [0, L), each is a match with its own value or an initial part
    with its gap id, and no two neighbours are a piece that could still be merged"""
    L, at = len(doc), 0
    piece = _pieces(m)
    cuts = _cuts(doc, gap)
    initial = set(zip(cuts, cuts[1:]))
    for i, (s, e) in zip(toks.tolist(), spans.tolist()):
        assert s == at and s < e <= L
        if i >= GID:
            assert (s, e) in initial and (s, e) not in piece and i == GID + (doc[s] if gap == Gap.Bytes else 0)
        else:
            assert piece.get((s, e)) == i
        at = e
    assert at == L
    sp = spans.tolist()
    for (s, _), (_, e) in zip(sp, sp[1:]):
        v = piece.get((s, e))
        assert v is None or (v if ranks is None else int(ranks[v])) == NO


@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("letters", [2, 3])
def test_fuzz(letters, n_docs):
    rng = np.random.default_rng(1000 * letters + n_docs)
    alphabet = list(b"abc"[:letters])
    pats = set()
    want_pats = int(rng.integers(30, 61))
    while len(pats) < want_pats:
        pats.add(bytes(rng.choice(alphabet, size=int(rng.integers(1, 7))).tolist()))
    pats = sorted(pats)
    o, p = _pair(pats)
    lens = rng.integers(0, 71, size=n_docs)
    lens[rng.random(n_docs) < 0.15] = 0
    lens[0] = 70
    if n_docs > 1:
        lens[-1] = 0
    docs = [bytes(rng.choice(alphabet, size=int(n)).tolist()) for n in lens]
    perm = rng.permutation(len(pats)).astype(np.uint32)
    perm[rng.choice(len(pats), size=4, replace=False)] = NO
    for ranks in (None, perm):
        res = _check_batch(o, p, docs, ranks, front=int(rng.integers(1, 40)), what=(letters, n_docs, ranks is None))
        for gap, ((ids, sp, off), got, ms) in res.items():
            g_ids, g_sp, g_off = got
            for d, doc in enumerate(docs):
                a, b = int(g_off[d]), int(g_off[d + 1])
                _legal(doc, g_ids[a:b], g_sp[a:b], ms[d], ranks, gap)


# ------------------------------------------------------------------------------------- 4. a vocabulary that lacks some single bytes
def test_vocabulary_without_some_single_bytes():
    o, p = _pair([b"ab", b"abc", b"c"])   # no a, no b
    docs = [b"abc", b"ba", b"xabcx", b"cabab", b"abcabc", b"", b"aab", b"b"]
    res = _check_batch(o, p, docs, what="no a, no b")
    (ids, sp, off), _, _ = res[Gap.Bytes]
    tok = lambda d: ids[off[d]:off[d + 1]].tolist()
    assert tok(0) == [1]                                          # a, b absent: a+b -> ab, ab+c -> abc
    assert tok(1) == [GID + ord("b"), GID + ord("a")]             # the leftovers: gap_id + byte
    assert tok(2) == [GID + ord("x"), 1, GID + ord("x")]
    assert tok(3) == [2, 0, 0] and tok(4) == [1, 1] and tok(6) == [GID + ord("a"), 0]
    (ids, sp, off), _, _ = res[Gap.Chars]
    assert ids[off[1]:off[2]].tolist() == [GID, GID]
    _check_batch(o, p, docs, [2, 0, 1], what="no a, no b, ranks")
    for d in docs:
        _check_single(o, p, d, None, Gap.Bytes)


# ------------------------------------------------------------------------------------- 5. DAAC_GAP_CHARS on bytes that are no UTF-8
def test_chars_gap_on_bytes_that_are_not_utf8():
    # patterns that end inside a code point: such a piece is never an initial part, and pairs of _CHARS parts seldom add up to one
    pats = [b"a\xc3", b"\xa9b", b"\xe4\xb8", b"\x96", b"\x80\x80", b"a", b"\xa9", b"a\xc3\xa9", b"\xc3\xa9", b"\xc3\xa9b"]
    o, p = _pair(pats)
    docs = [b"\x80\x80\x80ab", b"\xa9ba\xc3\xa9b", b"a\xc3\xa9b\xe4\xb8\x96\xe4\xb8", b"\x80" * 300, b"\x80" * 301, b"\xbf", b"", b"a\xc3", b"\xa9\xa9a\xc3\xa9",
            b"\xe4\xb8\x96a\xc3\xa9b" * 9]
    for ranks in (None, [3, 1, 4, 1, 5, 9, 2, 6, 5, 0]):
        res = _check_batch(o, p, docs, ranks, engines=(Engine.Auto,), what="not utf-8")
        (ids, sp, off), _, _ = res[Gap.Chars]
        # 300 and 301 continuation bytes are one initial part, which the vocabulary lacks
        for d in (3, 4):
            assert ids[off[d]:off[d + 1]].tolist() == [GID] and sp[off[d]:off[d + 1]].tolist() == [[0, len(docs[d])]]
        (ids, sp, off), _, _ = res[Gap.Bytes]
        assert ids[off[3]:off[4]].tolist() == [4] * 150 and off[5] - off[4] == 151
    for d in docs[:5]:
        _check_single(o, p, d, None, Gap.Chars)


# ---------------------------------------------------------------------------------------------------------------- 6. charwise
def test_charwise_automaton():
    pats = ["全世界", "世界", "界", "a", "é世", "𠮷a", "é", "世", "全", "全世"]
    values = np.array([3, 9, 4, 0, 7, 1, 2, 5, 11, 6], dtype=np.uint32)
    o, p = _pair(pats, charwise=True, values=values)
    docs = ["全世界中に世界の世", "", "a", "é世界aé中", "に世", "界全世界の" * 20, "𠮷", "𠮷aé世界"]
    rng = np.random.default_rng(3)
    for ranks in (None, rng.permutation(12).astype(np.uint32)):
        res = _check_batch(o, p, docs, ranks, what="charwise")
        (ids, sp, off), _, _ = res[Gap.Chars]
        assert (ids >= GID).any() and (ids < GID).any()
    ids, sp = _check_single(o, p, "に世界", None, Gap.Chars)
    assert sp.tolist()[0] == [0, 3] and ids[0] == GID   # に: one unknown token of three bytes
    ids, sp = _check_single(o, p, "に世界", None, Gap.Bytes)
    assert ids[:3].tolist() == [GID + c for c in "に".encode()]


# ------------------------------------------------------------------------------------------------------------ 7. "" in the set
def test_empty_pattern_is_no_piece():
    o, p = _pair([b"", b"wor", b"o", b"w", b"wo", b"r"])
    docs = [b"world", b"", b"o", b"xx", b"wow wor"]
    res = _check_batch(o, p, docs, what='""')
    (ids, sp, off), _, ms = res[Gap.Bytes]
    assert sum(len(m) for m in ms) > sum(len(d) for d in docs) and not np.any(ids == 0) and np.all(sp[:, 0] < sp[:, 1])
    assert ids[off[0]:off[1]].tolist() == [1, GID + ord("l"), GID + ord("d")]
    o, p = _pair([b""])
    res = _check_batch(o, p, docs, what='only ""')
    (ids, sp, off), _, _ = res[Gap.Bytes]
    assert len(ids) == sum(len(d) for d in docs) and np.all(ids >= GID) and np.all(sp[:, 1] - sp[:, 0] == 1)


# ---------------------------------------------------------------------------------------------------------------- 8. chunking
def _sparse(rng, n, keep):
    """n bytes, mostly x (in no pattern), letters of abc with probability `keep`: words scattered through noise, so few merges"""
    text = rng.choice(list(b"abc"), size=n)
    text[rng.random(n) >= keep] = ord("x")
    return bytes(text.tolist())


@pytest.mark.parametrize("piece", [None, 64])
def test_long_document_among_short_ones(piece):
    """one document of 3000 bytes: with batch_piece = 64 its tuple list comes from dozens of pieces"""
    rng = np.random.default_rng(20)
    pats = sorted({bytes(rng.choice(list(b"abc"), size=int(rng.integers(1, 6))).tolist()) for _ in range(25)})
    o, p = _pair(pats)
    if piece is not None:
        p.set_option("batch_piece", piece)
    docs = [b"ab", _sparse(rng, 3000, 0.25), b"", b"cabca", bytes(rng.choice(list(b"abc"), size=60).tolist())]
    res = _check_batch(o, p, docs, what=("long", piece))
    (ids, sp, off), _, _ = res[Gap.Chars]
    assert 2000 < off[2] - off[1] < 2990 and np.any(sp[off[1]:off[2], 1] - sp[off[1]:off[2], 0] > 2)


# --------------------------------------------------------------------------------------------------------------------- 9. the cap
@pytest.mark.parametrize("cap", [None, 100])
def test_document_length_cap(cap):
    rng = np.random.default_rng(9)
    o, p = _pair([b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca"])
    if cap is not None:
        p.set_option("bpe_doc_max", cap)
    L = 4096 if cap is None else cap
    full = _sparse(rng, L, 0.12 if cap is None else 0.6)
    docs = [b"abc", full, b"", b"cab"]
    _check_batch(o, p, docs, what=("at the cap", cap))          # exactly bpe_doc_max bytes: served
    _check_single(o, p, full, None, Gap.Bytes)
    _check_single(o, p, _dev(full), None, Gap.Chars)
    over = full + b"a"
    for arg in (docs[:2] + [b"", over], _device_batch(docs[:2] + [b"", over], 3)):
        with pytest.raises(da.DaachorseError) as ei:
            p.tokenize_bpe_batch(arg, gap_id=GID)
        assert ei.value.code == 6 and "document 3" in str(ei.value) and "pre-split" in str(ei.value), str(ei.value)
    for arg in (over, _dev(over)):
        with pytest.raises(da.DaachorseError) as ei:
            p.tokenize_bpe(arg, gap_id=GID)
        assert ei.value.code == 6 and "document 0" in str(ei.value)
    for bad in (0, 65537):
        with pytest.raises(da.DaachorseError) as ei:
            p.set_option("bpe_doc_max", bad)
        assert ei.value.code == 1
    # ... and the handle still serves what fits
    assert p.tokenize_bpe(b"abc", gap_id=GID).tolist() == [5]


# ------------------------------------------------------------------------------------------- 10. limits and degenerate batches
def test_result_above_max_result_bytes_answers_2():
    o, p = _pair([b"ab"])
    hay = b"abx" * 100 + b"xyz" * 900      # 100 matches (1600 bytes of tuples); 200 + 2700 tokens
    p.set_option("max_result_bytes", 20 * 2900 - 1)   # 2900 tokens with spans: 58000 bytes
    ids = p.tokenize_bpe(hay, gap=Gap.Bytes, gap_id=GID)
    assert len(ids) == 2900 and ids[:2].tolist() == [0, GID + ord("x")]
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_bpe(hay, gap=Gap.Bytes, gap_id=GID, spans=True)
    assert ei.value.code == 2 and "max_result_bytes" in str(ei.value)
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_bpe_batch([hay, b"ab"], gap=Gap.Bytes, gap_id=GID, spans=True)
    assert ei.value.code == 2
    ids, off = p.tokenize_bpe_batch([hay, b"ab"], gap=Gap.Bytes, gap_id=GID)
    assert off.tolist() == [0, 2900, 2901]


def test_no_documents_and_empty_documents():
    o, p = _pair([b"ab", b"b"])
    ids, sp, off = p.tokenize_bpe_batch([], spans=True)
    assert ids.dtype == np.uint32 and len(ids) == 0 and sp.dtype == np.uint64 and sp.shape == (0, 2) and off.dtype == np.uint64 and off.tolist() == [0]
    assert da.last_kernel().startswith("bpe docs=0 matches=0 tokens=0 ")
    ids, off = p.tokenize_bpe_batch([], [1, 0])
    assert len(ids) == 0 and off.tolist() == [0]
    for arg in ([b"", b"", b""], _device_batch([b"", b"", b""], 3)):
        ids, sp, off = p.tokenize_bpe_batch(arg, spans=True)
        assert ids.dtype == np.uint32 and len(ids) == 0 and sp.shape == (0, 2) and off.tolist() == [0, 0, 0, 0]
    for hay in (b"", _dev(b"")):
        ids, sp = p.tokenize_bpe(hay, spans=True)
        assert ids.dtype == np.uint32 and len(ids) == 0 and sp.dtype == np.uint64 and sp.shape == (0, 2)
    # device=True: the buffers round-trip and free
    d_ids, d_sp, d_off = p.tokenize_bpe_batch([b"ab", b"", b"xb"], gap_id=GID, spans=True, device=True)
    assert d_ids.to_numpy().tolist() == [0, GID + ord("x"), 1] and d_off.to_numpy().tolist() == [0, 1, 1, 3]
    assert d_sp.to_numpy().tolist() == [[0, 2], [0, 1], [1, 2]] and d_ids.n_matches == 3
    for x in (d_ids, d_sp, d_off):
        x.free()
    d_ids = p.tokenize_bpe(b"abb", gap_id=GID, device=True)
    assert d_ids.to_numpy().tolist() == [0, 1] and d_ids.n_matches == 3
    d_ids.free()


# ------------------------------------------------------------------------------------------------------------ 11. determinism
def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(5)
    pats = sorted({bytes(rng.choice(list(b"ab"), size=int(rng.integers(1, 6))).tolist()) for _ in range(40)})
    o, p = _pair(pats)
    ranks = rng.integers(0, 4, size=len(pats)).astype(np.uint32)
    docs = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) for n in rng.integers(0, 71, size=300)]
    arg = _device_batch(docs, 9)
    a = p.tokenize_bpe_batch(arg, ranks, gap=Gap.Bytes, gap_id=GID, spans=True)
    b = p.tokenize_bpe_batch(arg, ranks, gap=Gap.Bytes, gap_id=GID, spans=True)
    assert len(a[0]) > 300
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
