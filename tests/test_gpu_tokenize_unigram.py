"""tokenize_unigram on the MI355X (daac_tokenize_unigram / daac_tokenize_unigram_batch): the segmentation whose pieces' scores sum
highest.  Expected tokens and scores come from a float32 restatement of the definition (`_viterbi`) over the CPU oracle's
find_overlapping_iter matches of each document, never from the library.  Every comparison is exact: ids, spans, tok_offsets, and the
scores as their uint32 views.  There is no numeric tolerance in this feature."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap

F = np.float32
NINF = F(-np.inf)
GID = 0x10000   # keeps byte ids apart from values


def _pair(patterns, charwise=False, values=None):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p


def _b(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def _cuts(doc, gap):
    L = len(doc)
    return [0] + [p for p in range(1, L) if gap == Gap.Bytes or (doc[p] & 0xC0) != 0x80] + ([L] if L else [])


def _viterbi(doc, m, scores, unk, gap, gap_id):
    """the definition -> (tokens [(id, start, end)], score np.float32); `m`: the oracle's find_overlapping_iter(doc), in its order"""
    L = len(doc)
    best = [NINF] * (L + 1)
    best[0] = F(0.0)
    back = [None] * (L + 1)
    into = {}
    for s, e, v in zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist()):
        if s < e:
            into.setdefault(e, []).append((s, v))
    cuts = _cuts(doc, gap)
    prev = {c1: c0 for c0, c1 in zip(cuts, cuts[1:])}
    for q in range(1, L + 1):
        inc, edge = NINF, None
        for s, v in into.get(q, ()):
            if best[s] == NINF:
                continue
            c = best[s] + scores[v]   # np.float32 + np.float32: one float32 addition
            if c > inc:
                inc, edge = c, (v, s, q)
        if q in prev and best[prev[q]] != NINF:
            c = best[prev[q]] + unk
            if c > inc:
                inc, edge = c, (gap_id + (doc[prev[q]] if gap == Gap.Bytes else 0), prev[q], q)
        assert type(inc) is np.float32
        best[q], back[q] = inc, edge
    toks, q = [], L
    while q > 0:
        toks.append(back[q])
        q = back[q][1]
    return toks[::-1], best[L]


def _bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


def _expect(o, docs, scores, unk, gap, gap_id=GID):
    """-> (ids uint32[T], spans uint64[T, 2], offsets uint64[n + 1], doc scores float32[n], the oracle's matches per document)"""
    scores, unk = np.asarray(scores, dtype=np.float32), F(unk)
    toks, off, sc, ms = [], [0], [], []
    for d in docs:
        m = o.find_overlapping_iter(d)
        t, s = _viterbi(_b(d), m, scores, unk, gap, gap_id)
        toks += t
        off.append(len(toks))
        sc.append(s)
        ms.append(m)
    a = np.array(toks, dtype=np.uint64).reshape(len(toks), 3)
    return a[:, 0].astype(np.uint32), a[:, 1:].copy(), np.array(off, dtype=np.uint64), np.array(sc, dtype=np.float32), ms


def _device_batch(docs, front=0):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    blobs = [_b(d) for d in docs]
    off = np.full(len(blobs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(b) for b in blobs], dtype=np.int64)
    hay = np.frombuffer(b"\xff" * front + b"".join(blobs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _same(got, want, spans, what):
    """a batch result (ids, [spans], offsets, doc_scores) against _expect's"""
    ids, sp, off, sc = want[:4]
    g_ids, g_sp, g_off, g_sc = got if spans else (got[0], None, got[1], got[2])
    assert g_ids.dtype == np.uint32 and np.array_equal(g_ids, ids), what
    if spans:
        assert g_sp.dtype == np.uint64 and g_sp.shape == (len(ids), 2) and np.array_equal(g_sp, sp), what
    assert g_off.dtype == np.uint64 and np.array_equal(g_off, off), what
    assert g_sc.dtype == np.float32 and np.array_equal(_bits(g_sc), _bits(sc)), what


def _check_batch(o, p, docs, scores, unk, gaps=(Gap.Bytes, Gap.Chars), front=5, engines=(Engine.Auto, Engine.DArray), inputs=("host", "device"),
                 spans=(True, False), what=None):
    """tokenize_unigram_batch(docs) against the definition -> {gap: (what _expect returns, the library's result with spans)}"""
    out = {}
    for gap in gaps:
        want = _expect(o, docs, scores, unk, gap)
        for src, with_spans, eng in ((s, w, e) for s in inputs for w in spans for e in engines):
            arg = _device_batch(docs, front) if src == "device" else docs
            got = p.tokenize_unigram_batch(arg, scores, unk, gap=gap, gap_id=GID, spans=with_spans, doc_scores=True, engine=eng)
            assert da.last_kernel().startswith(f"unigram docs={len(docs)} matches={sum(len(m) for m in want[4])} tokens={len(want[0])} "), da.last_kernel()
            _same(got, want, with_spans, (what, gap, src, with_spans, eng))
            if with_spans:
                out[gap] = (want, got)
    return out


def _check_single(o, p, hay, scores, unk, gap, **kw):
    ids, sp, off, sc, _ = _expect(o, [hay], scores, unk, gap)
    g_ids, g_sp, g_sc = p.tokenize_unigram(hay, scores, unk, gap=gap, gap_id=GID, spans=True, **kw)
    assert np.array_equal(g_ids, ids) and np.array_equal(g_sp, sp) and type(g_sc) is np.float32 and _bits(g_sc)[0] == _bits(sc)[0], (hay, gap)
    g2, s2 = p.tokenize_unigram(hay, scores, unk, gap=gap, gap_id=GID, **kw)
    assert np.array_equal(g2, ids) and _bits(s2)[0] == _bits(sc)[0]
    return ids, sp, sc[0]


# ------------------------------------------------------------------------------------------------------------ 1. not greedy
def test_not_greedy():
    """ab|cd beats abc|d, which is what longest-match-first takes"""
    o, p = _pair([b"ab", b"abc", b"cd", b"d"])
    scores = [-1.0, -1.0, -1.0, -3.0]
    for gap in (Gap.Bytes, Gap.Chars):
        ids, sp, sc = _check_single(o, p, b"abcd", scores, -10.0, gap)
        assert ids.tolist() == [0, 2] and sp.tolist() == [[0, 2], [2, 4]] and sc == F(-2.0)
        dev = torch.from_numpy(np.frombuffer(b"abcd", dtype=np.uint8).copy()).cuda()
        _check_single(o, p, dev, scores, -10.0, gap)
    # tokenize's longest-match-first answer on the same patterns (a leftmost-longest automaton, as MaxMatch builds it) is the other one
    lo, lp = _pair_left([b"ab", b"abc", b"cd", b"d"])
    longest = lp.tokenize(b"abcd", gap=Gap.Bytes, gap_id=GID)
    assert longest.tolist() == [1, 3] and longest.tolist() != ids.tolist()
    # with the scores the other way round the same call takes abc|d, which find_iter's tokenize on this automaton does not
    ids, sp, sc = _check_single(o, p, b"abcd", [-3.0, -1.0, -3.0, -1.0], -10.0, Gap.Chars)
    assert ids.tolist() == [1, 3] and p.tokenize(b"abcd", gap=Gap.Bytes, gap_id=GID).tolist() != ids.tolist()
    # an unknown piece where the dictionary has none, and where it is the better one
    ids, sp, sc = _check_single(o, p, b"xabcdx", scores, -0.25, Gap.Bytes)
    assert ids.tolist() == [GID + c for c in b"xabcdx"] and sc == F(-1.5)


def _pair_left(patterns):
    o = orc.OraclePma.build(patterns, kind=1)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    return o, p


# -------------------------------------------------------------------------------------------------------------------- 2. ties
def test_ties():
    rng = np.random.default_rng(7)
    pats = sorted({bytes(rng.choice(list(b"ab"), size=int(rng.integers(1, 5))).tolist()) for _ in range(14)})
    o, p = _pair(pats)
    docs = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) for n in rng.integers(0, 40, size=70)]
    # all scores 0: every path ties; the earliest match of the reference's order wins, and a match wins against the unknown edge
    res = _check_batch(o, p, docs, [0.0] * len(pats), 0.0, what="zeros")
    (ids, sp, off, sc, _), _ = res[Gap.Bytes]
    assert np.all(_bits(sc) == 0) and (ids < GID).any()
    # few distinct scores, exactly representable, and unk_score equal to a pattern's
    for unk in (-0.25, -0.5, -0.75):
        scores = rng.choice(np.array([-0.25, -0.5, -0.75], dtype=np.float32), size=len(pats))
        assert F(unk) in scores
        _check_batch(o, p, docs, scores, unk, engines=(Engine.Auto,), what=("few", unk))


# -------------------------------------------------------------------------------------------------------------------- 3. fuzz
def _legal(doc, toks, spans, m, gap):
    """the properties that do not depend on the tie rule: the tokens tile [0, L), each is a match with its own value or a legal unknown edge"""
    L, at = len(doc), 0
    have = set(zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist()))
    cuts = _cuts(doc, gap)
    edges = set(zip(cuts, cuts[1:]))
    for i, (s, e) in zip(toks.tolist(), spans.tolist()):
        assert s == at and s < e <= L
        if i >= GID:
            assert (s, e) in edges and i == GID + (doc[s] if gap == Gap.Bytes else 0)
        else:
            assert (s, e, i) in have
        at = e
    assert at == L


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
    scores = (-rng.gamma(2.0, 3.0, size=len(pats))).astype(np.float32)
    unk = F(-rng.gamma(2.0, 4.0))
    lens = rng.integers(0, 71, size=n_docs)
    lens[rng.random(n_docs) < 0.15] = 0
    if n_docs > 1:
        lens[-1] = 0
        lens[0] = 70
    docs = [bytes(rng.choice(alphabet, size=int(n)).tolist()) for n in lens]
    res = _check_batch(o, p, docs, scores, unk, front=int(rng.integers(1, 40)), what=(letters, n_docs))
    for gap, ((ids, sp, off, sc, ms), got) in res.items():
        g_ids, g_sp, g_off, g_sc = got
        for d, doc in enumerate(docs):
            a, b = int(g_off[d]), int(g_off[d + 1])
            _legal(doc, g_ids[a:b], g_sp[a:b], ms[d], gap)
            total = F(0.0)
            for i in g_ids[a:b].tolist():
                total = total + (F(unk) if i >= GID else scores[i])
            assert _bits(total)[0] == _bits(g_sc[d])[0], (gap, d)


# ------------------------------------------------------------------------------------- 4. DAAC_GAP_CHARS on bytes that are no UTF-8
def test_chars_gap_on_bytes_that_are_not_utf8():
    # patterns that end inside a code point: the walk reaches a non-cut position and leaves it by a match or not at all
    pats = [b"a\xc3", b"\xa9b", b"\xe4\xb8", b"\x96", b"\x80\x80", b"a", b"\xa9"]
    o, p = _pair(pats)
    docs = [b"\x80\x80\x80ab", b"\xa9ba\xc3\xa9b", b"a\xc3\xa9b\xe4\xb8\x96\xe4\xb8", b"\x80" * 300, b"\x80" * 301, b"\xbf", b"", b"a\xc3", b"\xa9\xa9a\xc3\xa9",
            b"\xe4\xb8\x96a\xc3\xa9b" * 9]
    for scores, unk in (([-1.0, -1.0, -0.5, -0.5, -0.01, -2.0, -0.125], -3.0), ([-5.0, -0.5, -3.0, -0.25, -4.0, -0.5, -6.0], -1.0)):
        res = _check_batch(o, p, docs, scores, unk, engines=(Engine.Auto,), what="not utf-8")
        (ids, sp, off, sc, _), _ = res[Gap.Chars]
        # 301 continuation bytes and a pattern of two: position 301 is reached by the one unknown edge 0 -> 301 alone
        assert ids[off[4]:off[5]].tolist() == [GID] and sp[off[4]:off[5]].tolist() == [[0, 301]]
        assert np.all(ids[off[3]:off[4]] == 4) or ids[off[3]:off[4]].tolist() == [GID]
    for d in docs[:5]:
        _check_single(o, p, d, [-1.0, -1.0, -0.5, -0.5, -0.01, -2.0, -0.125], -3.0, Gap.Chars)


# ---------------------------------------------------------------------------------------------------------------- 5. charwise
def test_charwise_automaton():
    pats = ["全世界", "世界", "界", "a", "é世", "𠮷a", "é", "世"]
    values = np.array([3, 9, 4, 0, 7, 1, 2, 5], dtype=np.uint32)
    o, p = _pair(pats, charwise=True, values=values)
    docs = ["全世界中に世界の世", "", "a", "é世界aé中", "に世", "界全世界の" * 20, "𠮷", "𠮷aé世界"]
    rng = np.random.default_rng(3)
    for _ in range(2):
        scores = (-rng.gamma(2.0, 2.0, size=10)).astype(np.float32)
        res = _check_batch(o, p, docs, scores, -4.5, engines=(Engine.Auto, Engine.DArray), what="charwise")
    (ids, sp, off, sc, _), _ = res[Gap.Chars]
    assert (ids >= GID).any() and (ids < GID).any()
    ids, sp, sc = _check_single(o, p, "に世界", scores, -4.5, Gap.Chars)
    assert sp.tolist()[0] == [0, 3]   # に: one unknown token of three bytes


# ------------------------------------------------------------------------------------------------------------ 6. "" in the set
def test_empty_pattern_is_no_edge():
    o, p = _pair([b"", b"wor", b"o", b"w"])
    docs = [b"world", b"", b"o", b"xx", b"wow wor"]
    res = _check_batch(o, p, docs, [5.0, -1.0, -0.5, -0.75], -2.0, what='""')
    (ids, sp, off, sc, ms), _ = res[Gap.Bytes]
    assert sum(len(m) for m in ms) > sum(len(d) for d in docs) and not np.any(ids == 0) and np.all(sp[:, 0] < sp[:, 1])
    o, p = _pair([b""])
    _check_batch(o, p, docs, [1.0], -2.0, what='only ""')


# ---------------------------------------------------------------------------------------------------------------- 7. chunking
@pytest.mark.parametrize("piece", [None, 64])
def test_long_document_among_short_ones(piece):
    """one document of 20 000 bytes: with batch_piece = 64 its tuple list comes from hundreds of pieces"""
    rng = np.random.default_rng(20)
    pats = sorted({bytes(rng.choice(list(b"abc"), size=int(rng.integers(1, 6))).tolist()) for _ in range(25)})
    o, p = _pair(pats)
    if piece is not None:
        p.set_option("batch_piece", piece)
    scores = (-rng.gamma(2.0, 3.0, size=len(pats))).astype(np.float32)
    docs = [b"ab", bytes(rng.choice(list(b"abcx"), size=20000).tolist()), b"", b"cabca", bytes(rng.choice(list(b"abc"), size=200).tolist())]
    res = _check_batch(o, p, docs, scores, -7.0, gaps=(Gap.Chars,), what=("long", piece))
    (ids, sp, off, sc, _), _ = res[Gap.Chars]
    assert off[2] - off[1] > 4000


# ------------------------------------------------------------------------------------------- 8. limits and degenerate batches
def test_result_above_max_result_bytes_answers_2():
    o, p = _pair([b"ab"])
    hay = b"abx" * 1000
    p.set_option("max_result_bytes", 20 * 3000 - 1)   # 3000 byte tokens with spans: 60000 bytes; the tuple list: 16000
    ids, sc = p.tokenize_unigram(hay, [-9.0], -1.0, gap=Gap.Bytes)
    assert len(ids) == 3000 and sc == F(-3000.0)
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_unigram(hay, [-9.0], -1.0, gap=Gap.Bytes, spans=True)
    assert ei.value.code == 2 and "max_result_bytes" in str(ei.value)
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_unigram_batch([hay, b"ab"], [-9.0], -1.0, gap=Gap.Bytes, spans=True)
    assert ei.value.code == 2
    ids, off = p.tokenize_unigram_batch([hay, b"ab"], [-9.0], -1.0, gap=Gap.Bytes)
    assert off.tolist() == [0, 3000, 3002]   # a|b at -2 beats ab at -9


def test_no_documents_and_empty_documents():
    o, p = _pair([b"ab", b"b"])
    ids, sp, off, sc = p.tokenize_unigram_batch([], [-1.0, -1.0], -2.0, spans=True, doc_scores=True)
    assert ids.dtype == np.uint32 and len(ids) == 0 and sp.shape == (0, 2) and off.tolist() == [0] and sc.dtype == np.float32 and len(sc) == 0
    ids, off = p.tokenize_unigram_batch([], [-1.0, -1.0], -2.0)
    assert len(ids) == 0 and off.tolist() == [0]
    for arg in ([b"", b"", b""], _device_batch([b"", b"", b""], 3)):
        ids, sp, off, sc = p.tokenize_unigram_batch(arg, [-1.0, -1.0], -2.0, spans=True, doc_scores=True)
        assert len(ids) == 0 and sp.shape == (0, 2) and off.tolist() == [0, 0, 0, 0] and _bits(sc).tolist() == [0, 0, 0]
    ids, sp, sc = p.tokenize_unigram(b"", [-1.0, -1.0], -2.0, spans=True)
    assert len(ids) == 0 and sp.shape == (0, 2) and _bits(sc)[0] == 0
    d_ids, d_off, d_sc = p.tokenize_unigram_batch([b"ab", b"", b"xb"], [-1.0, -1.0], -2.0, doc_scores=True, device=True)
    assert d_ids.to_numpy().tolist() == [0, 0, 1] and d_off.to_numpy().tolist() == [0, 1, 1, 3] and d_sc.to_numpy().tolist() == [-1.0, 0.0, -3.0]
    assert d_ids.n_matches == 3
    for x in (d_ids, d_off, d_sc):
        x.free()


# ------------------------------------------------------------------------------------------------------------- 9. determinism
def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(5)
    pats = sorted({bytes(rng.choice(list(b"ab"), size=int(rng.integers(1, 6))).tolist()) for _ in range(40)})
    o, p = _pair(pats)
    scores = rng.choice(np.array([-0.25, -0.5, -0.75, -1.0], dtype=np.float32), size=len(pats))
    docs = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) for n in rng.integers(0, 71, size=300)]
    arg = _device_batch(docs, 9)
    a = p.tokenize_unigram_batch(arg, scores, -0.5, gap=Gap.Bytes, gap_id=GID, spans=True, doc_scores=True)
    b = p.tokenize_unigram_batch(arg, scores, -0.5, gap=Gap.Bytes, gap_id=GID, spans=True, doc_scores=True)
    assert len(a[0]) > 300
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
