"""tokenize on the MI355X (daac_tokenize / daac_tokenize_batch): the values of the matches of find_iter / leftmost_find_iter and the gaps
between them as one id list.  Expected tokens come from a short restatement of the definition over the CPU oracle's tuples (`_tokens`),
never from the library; the 16 MiB text is also held against a vectorised numpy restatement over the library's own scan() tuples, code
the tokenize passes do not touch.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import iter_vector_runs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap, ScanMode, synth

T = 4096   # bytes of text per tile (tokenize.hpp: kTokTile)
API = {0: "find_iter", 1: "leftmost_find_iter", 2: "leftmost_find_iter"}
GAPS = [Gap.Skip, Gap.Unk, Gap.Bytes, Gap.Chars]
GID = 0x10000   # keeps byte ids apart from values


def _pair(patterns, kind=0, charwise=False, values=None):
    kind = orc.KIND.get(kind, kind)
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p, API[kind]


def _b(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def _gap_tokens(hay, a, b, gap, gap_id):
    """tok([a, b)) of the definition"""
    if gap == Gap.Skip or a == b:
        return []
    if gap == Gap.Unk:
        return [(gap_id, a, b)]
    if gap == Gap.Bytes:
        return [(gap_id + hay[p], p, p + 1) for p in range(a, b)]
    cuts = [a] + [p for p in range(a + 1, b) if (hay[p] & 0xC0) != 0x80] + [b]
    return [(gap_id, cuts[j], cuts[j + 1]) for j in range(len(cuts) - 1)]


def _tokens(hay, m, gap, gap_id):
    """the definition: tok(g_0), m_0, tok(g_1), m_1, .., m_{k-1}, tok(g_k) as (ids uint32[T], spans uint64[T, 2])"""
    assert np.all(m["start"][1:] >= m["end"][:-1]), "the oracle's list is not ordered and disjoint"
    out, at = [], 0
    for s, e, v in zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist()):
        out += _gap_tokens(hay, at, s, gap, gap_id)
        out.append((v, s, e))
        at = e
    out += _gap_tokens(hay, at, len(hay), gap, gap_id)
    a = np.array(out, dtype=np.uint64).reshape(len(out), 3)
    return a[:, 0].astype(np.uint32), a[:, 1:].copy()


def _matches(o, api, hay):
    """the oracle's tuples, or None where the reference iterator does not terminate (note D)"""
    try:
        return getattr(o, api)(hay)
    except orc.OracleError as e:
        assert e.code == 6
        return None


def _dev(hay, skew=0):
    """the bytes on the device, `skew` bytes behind a 16-byte boundary"""
    a = np.frombuffer(_b(hay), dtype=np.uint8)
    t = torch.zeros(skew + len(a), dtype=torch.uint8, device="cuda")
    t[skew:] = torch.from_numpy(a.copy())
    t = t[skew:]
    assert skew == 0 or len(a) == 0 or t.data_ptr() % 16 == skew
    return t


def _check(o, p, api, hay, gaps=GAPS, dev=False, spans=(True,), gap_id=GID, what=None, **kw):
    """tokenize(hay) on a host or device haystack against the definition over the oracle's tuples -> the number of calls, or None (note D)"""
    m = _matches(o, api, hay)
    arg = _dev(hay, dev if dev is not True else 0) if dev is not False else hay
    if m is None:
        with pytest.raises(da.DaachorseError) as ei:
            p.tokenize(arg, spans=True, **kw)
        assert ei.value.code == 6, what
        return None
    calls = 0
    for gap in gaps:
        ids, sp = _tokens(_b(hay), m, gap, gap_id)
        for with_spans in spans:
            got = p.tokenize(arg, gap=gap, gap_id=gap_id, spans=with_spans, **kw)
            assert da.last_kernel().startswith(f"tokenize matches={len(m)} tokens={len(ids)} "), da.last_kernel()
            g_ids, g_sp = got if with_spans else (got, None)
            assert g_ids.dtype == np.uint32 and np.array_equal(g_ids, ids), (what, gap, len(g_ids), len(ids))
            if with_spans:
                assert g_sp.dtype == np.uint64 and g_sp.shape == (len(ids), 2) and np.array_equal(g_sp, sp), (what, gap)
            calls += 1
    return calls


# ---------------------------------------------------------------------------------------------------------- 1. golden vectors
@pytest.mark.parametrize("charwise", [False, True])
def test_golden_vectors(vectors, charwise):
    n = noted = 0
    for runner, case in iter_vector_runs(vectors):
        if runner["api"] not in ("find_iter", "leftmost_find_iter"):
            continue
        o, p, api = _pair(case["patterns"], runner.get("kind", "Standard"), charwise)
        assert api == runner["api"]
        hay = case["haystack"] if charwise else case["haystack"].encode("utf-8")
        noted += _check(o, p, api, hay, dev=True if n % 2 == 1 else False, what=(case["name"], api, charwise)) is None
        n += 1
    assert n == 61 + 93 + 91 and noted < n


# ------------------------------------------------------------------------------------------------------------------- 2. fuzz
LENGTHS = [0, 1, 15, 16, 17, 257, 3001, T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_fuzz(kind):
    rng = np.random.default_rng(4100 + kind)
    calls = noted = skew = 0
    for rnd in range(5):
        alphabet = list((b"ab", b"abc", b"ab", b"abc", bytes(range(97, 123)) + b" \xc3\xa9\xe4\xb8\x96")[rnd])   # the last: sparse
        pats = sorted({bytes(rng.choice(alphabet, size=int(rng.integers(1, 6))).tolist()) for _ in range(int(rng.integers(2, 9)))})
        if rnd in (2, 3):
            pats = [b""] + pats
        if kind == 0 and rnd % 2 == 1:
            pats = pats + pats[-2:]   # copies of patterns: two values for one string
        o, p, api = _pair(pats, kind)
        for li, n in enumerate(LENGTHS):
            hay = bytes(rng.choice(alphabet, size=n).tolist())
            eng = (Engine.Auto, Engine.DArray)[(li + rnd) % 2]
            if li % 2:   # device, at every data_ptr() % 16 in turn
                dev, skew = skew % 16, skew + 1
            else:
                dev = False
            got = _check(o, p, api, hay, dev=dev, spans=(True, False), what=(kind, rnd, n), engine=eng)
            noted += got is None
            calls += got or 0
    assert skew >= 16 and noted < 5 * len(LENGTHS) // 2 and calls == 8 * (5 * len(LENGTHS) - noted)


# -------------------------------------------------------------------------------------------------------------- 3. boundaries
def _edge_cases():
    e3, e4 = "世".encode(), "𠮷".encode()   # 3 and 4 bytes
    cases = {
        "across a lane's boundary": ([b"abc"], b"x" * 14 + b"abc" + b"y" * 40),
        "across a tile boundary": ([b"abc"], b"x" * (T - 2) + b"abc" + b"y" * 70),
        "ends on a tile boundary": ([b"abc"], b"x" * (T - 3) + b"abc" + b"y" * 70),
        "begins on a tile boundary": ([b"abc"], b"x" * T + b"abc" + b"y" * 70),
        "adjacent matches": ([b"ab", b"cd"], b"xxabcdababcdyy" * 5 + b"ab" * 2100),
        "only a match": ([b"ab"], b"ab"),
        "a match longer than a tile": ([b"a" * (T + 40), b"b"], b"xb" + b"a" * (T + 40) + b"bx" + b"a" * 50),
        "every byte a match": ([b"a", b"b"], b"ab" * (T // 2 + 9) + b"a"),
        "text ends with a match at a tile's end": ([b"ab"], b"x" * (T - 2) + b"ab"),
        "text ends with a gap at a tile's end": ([b"ab"], b"ab" + b"x" * (T - 2)),
        # continuation bytes as the first bytes of a lane (16 | position) and of a tile
        "3-byte character across a lane": ([b"ab"], b"ab" + b"x" * 12 + e3 + b"yab" + b"x" * 9 + e3[:1] + e3 + b"z"),
        "4-byte character across a lane": ([b"ab"], b"x" * 13 + e4 + b"ab" + b"x" * 12 + e4 + b"x" * 11 + e4),
        "3-byte character across a tile": ([b"ab"], b"x" * (T - 1) + e3 + b"ab" + b"x" * (T - 7) + e3 + b"q"),
        "4-byte character across a tile": ([b"ab"], b"x" * (T - 3) + e4 + b"ab" + b"x" * (T - 4) + e4 + b"x" * (T - 5) + e4),
        "a run of continuation bytes longer than a tile": ([b"ab"], b"ab\xe4" + b"\x80" * (T + 100) + b"ab" + b"\x80" * 40),
        # the automaton matches the lead byte alone: the gap behind it begins with continuation bytes
        "lead byte matched": ([b"\xe4", b"\xf0"], b"x" + e3 + e3 + b"y" * 11 + e3 + e4 + b"zz" + e4),
    }
    return cases


@pytest.mark.parametrize("dev", [False, 0, 5])
def test_boundaries(dev):
    for name, (pats, hay) in _edge_cases().items():
        for kind in (0, 1):
            o, p, api = _pair(pats, kind)
            assert _check(o, p, api, hay, dev=dev, spans=(True, False), what=(name, kind)) == 8, name
    # no match: one unknown token, or none and no buffer
    o, p, api = _pair([b"ab"], 0)
    hay = b"x" * (T + 7)
    arg = hay if dev is False else _dev(hay, dev)
    ids, sp = p.tokenize(arg, gap=Gap.Unk, gap_id=9, spans=True)
    assert ids.tolist() == [9] and sp.tolist() == [[0, T + 7]]
    d_ids, d_sp = p.tokenize(arg, gap=Gap.Skip, spans=True, device=True)
    assert d_ids.count == 0 and d_ids.ptr is None and d_sp.ptr is None and d_ids.n_matches == 0
    assert len(p.tokenize(arg, gap=Gap.Bytes, gap_id=GID)) == T + 7 == len(p.tokenize(arg, gap=Gap.Chars))
    # every byte a match: as many tokens as bytes, whatever the gap rule
    o, p, api = _pair([b"a", b"b"], 0)
    hay = b"ab" * (T // 2 + 9) + b"a"
    for gap in GAPS:
        assert len(p.tokenize(hay if dev is False else _dev(hay, dev), gap=gap)) == len(hay)
    # an empty text
    for gap in GAPS:
        ids, sp = p.tokenize(b"" if dev is False else _dev(b"", dev), gap=gap, spans=True)
        assert ids.shape == (0,) and sp.shape == (0, 2)


def test_empty_pattern():
    """"" among the patterns of a Standard automaton: empty-match tokens at 0 .. len, each between two gaps"""
    for pats in ([b""], [b"", b"wor", b"o"]):
        o, p, api = _pair(pats, 0)
        for hay in (b"", b"h", b"hello world " * 30, ("wo世r" * 7).encode() + b"world " * (T // 6 + 3)):
            assert _check(o, p, api, hay, spans=(True, False), what=(pats, len(hay))) == 8
            assert _check(o, p, api, hay, dev=11, what=(pats, len(hay))) == 4
    o, p, api = _pair([b""], 0)
    ids, sp = p.tokenize(b"abc", gap=Gap.Unk, gap_id=5, spans=True)
    assert len(ids) == 4 + 3 and sp[:, 0].tolist() == [0, 0, 1, 1, 2, 2, 3]


def test_result_above_max_result_bytes_answers_2():
    o, p, api = _pair([b"ab"], 0)
    hay = b"abx" * 1000
    p.set_option("max_result_bytes", 20 * 2000 - 1)   # 2000 tokens with spans: 40000 bytes; the tuple list: 16000
    assert len(p.tokenize(hay)) == 2000
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize(hay, spans=True)
    assert ei.value.code == 2


# -------------------------------------------------------------------------------------------------------------------- 4. batch
def _device_batch(docs, front=0):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    blobs = [_b(d) for d in docs]
    off = np.full(len(blobs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(b) for b in blobs], dtype=np.int64)   # (of no documents: an empty sum, not a float one)
    hay = np.frombuffer(b"ab" * (front // 2 + 1), dtype=np.uint8)[:front].tolist() + list(b"".join(blobs))
    return torch.tensor(hay, dtype=torch.uint8).cuda(), torch.from_numpy(off).cuda()


def _check_batch(o, p, api, docs, gaps=GAPS, what=None, route="", front=0):
    ms = [_matches(o, api, d) for d in docs]
    for batch in (docs, _device_batch(docs, front)):
        if any(m is None for m in ms):
            first = next(i for i, m in enumerate(ms) if m is None)
            with pytest.raises(da.DaachorseError) as ei:
                p.tokenize_batch(batch, spans=True)
            assert ei.value.code == 6 and f"document {first}:" in str(ei.value), (what, str(ei.value))
            continue
        for gap in gaps:
            wants = [_tokens(_b(d), m, gap, GID) for d, m in zip(docs, ms)]
            w_ids = np.concatenate([w[0] for w in wants]) if wants else np.zeros(0, np.uint32)
            w_sp = np.concatenate([w[1] for w in wants]) if wants else np.zeros((0, 2), np.uint64)
            w_off = [0] + np.cumsum([len(w[0]) for w in wants]).tolist()
            ids, sp, off = p.tokenize_batch(batch, gap=gap, gap_id=GID, spans=True)
            assert da.last_kernel().startswith("tokenize matches=") and " batch " in da.last_kernel() and route in da.last_kernel(), da.last_kernel()
            assert off.dtype == np.uint64 and off.tolist() == w_off, (what, gap)
            assert np.array_equal(ids, w_ids) and np.array_equal(sp, w_sp) and sp.shape == (len(w_ids), 2), (what, gap)
            ids2, off2 = p.tokenize_batch(batch, gap=gap, gap_id=GID)
            assert np.array_equal(ids2, w_ids) and off2.tolist() == w_off, (what, gap)
            d_ids, d_off = p.tokenize_batch(batch, gap=gap, gap_id=GID, device=True)
            assert d_ids.count == w_off[-1] == int(d_off.to_numpy()[-1]) and d_off.count == len(docs) + 1, (what, gap)
            assert (d_ids.ptr is None) == (d_ids.count == 0)
            assert d_ids.n_matches == sum(len(m) for m in ms)
            d_ids.free()
            d_off.free()
    return ms


@pytest.mark.parametrize("kind", [0, 1])
def test_batch(kind):
    rng = np.random.default_rng(91 + kind)
    pats = [b"abc", b"bc", b"c", b"cab", b"aa"]
    o, p, api = _pair(pats, kind)
    p.set_option("batch_lane_max", 300)
    long_doc = bytes(rng.choice(list(b"abcx"), size=5000).tolist())   # beyond batch_lane_max: the long-document route
    # "ab" + "c..." and "ca" + "b": a pattern would match across these boundaries and must not; "xx" + "yx": a gap ends one document and
    # begins the next
    docs = [b"", b"", b"a", b"ab", b"cab", b"ca", b"b", b"", b"", b"xx", b"yx", long_doc, b"c", bytes(rng.choice(list(b"abcx"), size=299).tolist()),
            bytes(rng.choice(list(b"abcx"), size=301).tolist()), b"", b"abcabc" * 40, b"x" * T, b"aa" * (T // 2), b"x", b""]
    ms = _check_batch(o, p, api, docs, what=kind, route="long_docs=4", front=0)
    _check_batch(o, p, api, docs, gaps=[Gap.Unk, Gap.Chars], what=kind, front=37)   # offsets[0] != 0, every boundary off the 16s
    # the documents "xx", "yx": two unknown tokens, not one
    ids, sp, off = p.tokenize_batch([b"xx", b"yx"], gap=Gap.Unk, gap_id=GID, spans=True)
    assert ids.tolist() == [GID, GID] and sp.tolist() == [[0, 2], [0, 2]] and off.tolist() == [0, 1, 2]
    # each document equals tokenize of it alone
    for d, m in list(zip(docs, ms))[:14]:
        assert np.array_equal(p.tokenize(d, gap=Gap.Chars, gap_id=GID), _tokens(d, m, Gap.Chars, GID)[0])
    # n = 0: no result, one offset
    for batch in ([], _device_batch([])):
        ids, sp, off = p.tokenize_batch(batch, spans=True)
        assert ids.shape == (0,) and sp.shape == (0, 2) and off.tolist() == [0]
        d_ids, d_off = p.tokenize_batch(batch, device=True)
        assert d_ids.ptr is None and d_ids.count == 0 and d_off.to_numpy().tolist() == [0]
        d_off.free()
    # only empty documents
    _check_batch(o, p, api, [b"", b"", b""])


def test_batch_with_empty_pattern_and_note_d():
    """"" among the patterns: every document gets its empty-match tokens at 0 .. len, empty documents too; a leftmost automaton whose
    document ends inside a longer pattern makes the call answer 6, naming the document"""
    o, p, api = _pair([b"", b"ab"], 0)
    _check_batch(o, p, api, [b"", b"a", b"abab", b"", b"", b"xaby", b""])
    _check_batch(o, p, api, [b"x" * (T - 1), b"", b"ab", b"", b"y" * 20], front=5)
    o, p, api = _pair([b"", b"abc"], 1)
    _check_batch(o, p, api, [b"xx", b"abcx", b""])
    ms = _check_batch(o, p, api, [b"xx", b"abcx", b"zab", b"ab"])
    assert ms[2] is None and ms[0] is not None


def test_batch_charwise():
    pats = ["全世界", "世界", "界", "a", "é世"]
    # "中" ends a document and "に" begins the next: one unknown character each
    docs = ["全世界中に世界の世", "", "a", "é世界aé中", "に世", "界全世界の" * 200, "𠮷"]
    for kind in (0, 1):
        o, p, api = _pair(pats, kind, charwise=True)
        p.set_option("batch_lane_max", 300)
        _check_batch(o, p, api, docs, what=kind)
        ids, sp, off = p.tokenize_batch(["é中", "に世"], gap=Gap.Chars, gap_id=GID, spans=True)
        assert ids.tolist() == [GID] * 4 and sp.tolist() == [[0, 2], [2, 5], [0, 3], [3, 6]] and off.tolist() == [0, 2, 4]


# -------------------------------------------------------------------------------------------------------- 5. one larger text
def _numpy_tokens(hay, m, gap, gap_id):
    """the definition, vectorised, for a list without empty matches: a token begins at every match's start and, outside the matches, at
    a gap's first byte (Unk), at every byte (Bytes) or at a gap's first byte and every byte that is no continuation byte (Chars)"""
    n = len(hay)
    start, end = m["start"].astype(np.int64), m["end"].astype(np.int64)
    assert np.all(end > start) and np.all(start[1:] >= end[:-1])
    d = np.zeros(n + 1, dtype=np.int32)
    d[start] += 1   # (the matches are disjoint and not empty: no start and no end comes twice)
    d[end] -= 1
    cov = np.cumsum(d)[:n] > 0
    mst = np.zeros(n, dtype=bool)
    mst[start] = True
    first = np.zeros(n + 1, dtype=bool)   # a gap's first byte, if the position is not in a match
    first[0] = True
    first[end] = True
    rule = {Gap.Skip: np.zeros(n, dtype=bool), Gap.Unk: first[:n], Gap.Bytes: np.ones(n, dtype=bool), Gap.Chars: first[:n] | ((hay & 0xC0) != 0x80)}[gap]
    at = np.flatnonzero(mst | (~cov & rule))
    is_m = mst[at]
    value = np.zeros(n, dtype=np.uint32)
    value[start] = m["value"]
    m_end = np.zeros(n, dtype=np.int64)
    m_end[start] = end
    ids = np.where(is_m, value[at], np.uint32(gap_id) + (hay[at].astype(np.uint32) if gap == Gap.Bytes else np.uint32(0))).astype(np.uint32)
    nxt = np.append(at[1:], n)   # a gap token ends where the next token begins, or at len
    sp = np.stack([at, np.where(is_m, m_end[at], nxt)], axis=1).astype(np.uint64)
    return ids, sp


@pytest.mark.parametrize("kind", [0, 1])
def test_cfg3_16mib(kind):
    """16 MiB + 5 bytes: 4097 tiles, so the tile bases take more than one level of the exclusive sum"""
    pats = synth.patterns_cfg3(2000)
    o, p, api = _pair(pats, kind)
    mode = ScanMode.Find if kind == 0 else ScanMode.LeftmostFind
    n = (16 << 20) + 5
    buf = torch.empty((16 << 20) + 16, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(buf, synth.SEEDS["cfg3_dense"], pats, 20)
    dev = buf[:n]
    host = dev.cpu().numpy()
    # the first 2T + 1 bytes against the oracle
    assert _check(o, p, api, host[:2 * T + 1].tobytes(), dev=False) == 4
    # the whole against the library's own tuples
    m = p.scan(mode, dev)
    assert len(m) > 1000
    for gap in (Gap.Unk, Gap.Chars) if kind == 0 else (Gap.Bytes, Gap.Skip):
        want_ids, want_sp = _numpy_tokens(host, m, gap, GID)
        d_ids, d_sp = p.tokenize(dev, gap=gap, gap_id=GID, spans=True, device=True)
        assert d_ids.count == len(want_ids) == d_sp.count and d_ids.n_matches == len(m)
        ids, sp = d_ids.to_numpy(), d_sp.to_numpy()
        assert np.array_equal(ids, want_ids) and np.array_equal(sp, want_sp), gap
        # a second call gives the same bits
        e_ids, e_sp = p.tokenize(dev, gap=gap, gap_id=GID, spans=True, device=True)
        assert e_ids.ptr != d_ids.ptr and np.array_equal(e_ids.to_numpy(), ids) and np.array_equal(e_sp.to_numpy(), sp), gap
        for x in (d_ids, d_sp, e_ids, e_sp):
            x.free()


# ------------------------------------------------------------------------------------------------------- 6. device results
def test_device_results_round_trip():
    o, p, api = _pair([b"ab", b"c"], 0, values=np.array([7, 8], dtype=np.uint32))
    hay = b"xxabycab" * 100
    ids, sp = _tokens(hay, o.find_iter(hay), Gap.Unk, 1)
    d_ids, d_sp = p.tokenize(_dev(hay, 3), gap=Gap.Unk, gap_id=1, spans=True, device=True)
    assert da.last_kernel().startswith("tokenize matches=300 tokens=500 "), da.last_kernel()
    assert d_ids.count == d_sp.count == 500 and d_ids.n_matches == 300
    assert np.array_equal(d_ids.to_numpy(), ids) and np.array_equal(d_sp.to_numpy(), sp)
    assert np.array_equal(d_ids.to_numpy(first=10, n=5), ids[10:15]) and np.array_equal(d_sp.to_numpy(first=499), sp[499:])
    only = p.tokenize(hay, gap=Gap.Unk, gap_id=1, device=True)
    assert isinstance(only, da.bytewise.DeviceMatches) and np.array_equal(only.to_numpy(), ids)
    for x in (d_ids, d_sp, only):
        x.free()
        assert x.ptr is None
        with pytest.raises(da.DaachorseError):
            x.to_numpy()
    d_ids, d_sp, d_off = p.tokenize_batch([hay, b"", b"abq"], gap=Gap.Unk, gap_id=1, spans=True, device=True)
    assert isinstance(d_off, da.bytewise.DeviceOffsets) and d_off.to_numpy().tolist() == [0, 500, 500, 502]
    assert d_sp.to_numpy()[-2:].tolist() == [[0, 2], [2, 3]] and d_ids.to_numpy()[-2:].tolist() == [7, 1]
    for x in (d_ids, d_sp, d_off):
        x.free()
        assert x.ptr is None
