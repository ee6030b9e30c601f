"""replace_all on the MI355X (daac_replace_all / daac_replace_all_batch): the text with every match of find_iter / leftmost_find_iter
replaced.  Expected bytes come from a ten-line splice over the CPU oracle's tuples (`_splice`), never from the library; the 16 MiB
texts are also held against a vectorised numpy splice of the library's own scan() tuples, code the splice does not touch."""
import numpy as np
import pytest
import torch

from conftest import iter_vector_runs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

T = 4096   # output bytes per splice tile (replace.hpp: kSpliceTile)
STAGE = 1536   # segments of a tile whose positions LDS takes (kSpliceStage)
API = {0: "find_iter", 1: "leftmost_find_iter", 2: "leftmost_find_iter"}


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


def _splice(hay, m, table):
    """the definition: hay[0:start_0] + r(m_0) + hay[end_0:start_1] + ... + hay[end_{k-1}:]; one replacement serves every match"""
    assert np.all(m["start"][1:] >= m["end"][:-1]), "the oracle's list is not ordered and disjoint"
    out, at = [], 0
    for s, e, v in zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist()):
        out += [hay[at:s], table[0] if len(table) == 1 else table[v]]
        at = e
    return b"".join(out + [hay[at:]])


def _want(o, api, hay, table):
    """the oracle splice, or None where the reference iterator does not terminate (note D)"""
    try:
        m = getattr(o, api)(hay)
    except orc.OracleError as e:
        assert e.code == 6
        return None
    return _splice(_b(hay), m, [_b(r) for r in table])


def _dev(hay, skew=0):
    """the bytes on the device, `skew` bytes behind a 16-byte boundary"""
    a = np.frombuffer(_b(hay), dtype=np.uint8)
    t = torch.zeros(skew + len(a), dtype=torch.uint8, device="cuda")
    t[skew:] = torch.from_numpy(a.copy())
    t = t[skew:]
    assert skew == 0 or len(a) == 0 or t.data_ptr() % 16 == skew
    return t


def _check(o, p, api, hay, table, dev, what=None, **kw):
    """replace_all(hay) on a host or device haystack against the oracle splice; a single table entry goes as one bytes object"""
    want = _want(o, api, hay, table)
    arg = _dev(hay, dev if dev is not True else 0) if dev else hay
    repl = table[0] if len(table) == 1 else table
    if want is None:
        with pytest.raises(da.DaachorseError) as ei:
            p.replace_all(arg, repl, **kw)
        assert ei.value.code == 6, what
        return None
    got = p.replace_all(arg, repl, **kw)
    assert got == want, (what, len(got), len(want))
    assert da.last_kernel().startswith("replace matches="), da.last_kernel()
    return got


def _tables(n):
    return [[b"<%d>" % i for i in range(n)], [b"[x]"], [b""]]


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
        for k, table in enumerate(_tables(max(1, len(case["patterns"])))):
            noted += _check(o, p, api, hay, table, dev=(n + k) % 2 == 1, what=(case["name"], api, charwise, k)) is None
        n += 1
    assert n == 61 + 93 + 91 and noted < n


# ------------------------------------------------------------------------------------------------------------------- 2. fuzz
LENGTHS = [0, 1, 15, 16, 17, 257, 3001, T - 1, T, T + 1, 2 * T + 1]


def _fuzz_table(rng, pats, variant):
    """replacement lengths 0, 1, equal to the match, 3, 40 — per value, so a pattern's copies may differ"""
    if variant == 0:
        return [b""]
    if variant == 1:
        return [b"#"]
    if variant == 2:
        return [bytes(x ^ 0x20 for x in _b(q)) for q in pats]   # as long as the match (upper case)
    if variant == 3:
        return [b"%03d" % (i % 1000) for i in range(len(pats))]
    return [bytes(rng.integers(48, 58, size=(0, 1, 3, 40)[int(rng.integers(0, 4))]).astype(np.uint8)) for _ in pats]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_fuzz(kind):
    rng = np.random.default_rng(2300 + kind)
    calls = noted = 0
    for rnd in range(4):
        alphabet = list(b"ab" if rnd % 2 == 0 else b"abc")
        pats = sorted({bytes(rng.choice(alphabet, size=int(rng.integers(1, 6))).tolist()) for _ in range(int(rng.integers(2, 9)))})
        if rnd >= 2:
            pats = [b""] + pats
        if kind == 0 and rnd % 2 == 1:
            pats = pats + pats[-2:]   # copies of patterns: two values for one string
        o, p, api = _pair(pats, kind)
        for li, n in enumerate(LENGTHS):
            hay = bytes(rng.choice(alphabet, size=n).tolist())
            table = _fuzz_table(rng, pats, (li + rnd) % 5)
            p.set_option("seg_bytes", (None, 16, 64)[(li + rnd) % 3])
            eng = (Engine.Auto, Engine.DArray)[(li + rnd) % 2]
            dev = (0, 3, 0, 13)[li % 4] if li % 2 else False   # host, and device at data_ptr() % 16 = 3 or 13
            noted += _check(o, p, api, hay, table, dev or (li % 4 == 2), what=(kind, rnd, n), engine=eng) is None
            calls += 1
    assert calls == 4 * len(LENGTHS) and noted < calls // 2


# -------------------------------------------------------------------------------------------------------------- 3. tile edges
def _edge_cases():
    big = bytes(i % 251 for i in range(10000))
    return {
        # a replacement that begins in one tile and ends in the next
        "straddle": ([b"ab"], b"x" * (T - 5) + b"ab" + b"y" * 70, [b"0123456789"]),
        # one replacement that spans several tiles
        "long replacement": ([b"ab"], b"x" * 100 + b"ab" + b"y" * 100, [big]),
        # every byte deleted: an empty result
        "all deleted": ([b"a"], b"a" * 20000, [b""]),
        # 2047 segments begin inside a tile: more than LDS staging takes
        "dense": ([b"a"], b"a" * 20000, [b"xy"]),
        # 20 000 matches share output position 0, then text: a tile inside deleted adjacent matches
        "ties": ([b"a"], b"a" * 20000 + b"b" * 100, [b""]),
        "ties then a match": ([b"a", b"bb"], b"b" * 40 + b"a" * 5000 + b"bbb" + b"a" * 3000 + b"c" * 37, [b"", b"<2>"]),
        # no match: a pure copy, 16 | len and not
        "copy 16": ([b"ab"], bytes(97 + (i * 7) % 23 for i in range(2 * T)).replace(b"ab", b"ba"), [b"-"]),
        "copy odd": ([b"ab"], bytes(97 + (i * 7) % 23 for i in range(5007)).replace(b"ab", b"ba"), [b"-"]),
        # "" inserts at 0, between all bytes and at len
        "insertions": ([b""], b"hello world " * 30, [b"-"]),
        "insertions and words": ([b"", b"wor", b"o"], b"hello world " * 400, [b"", b"<1>", b"00"]),
        # a match at position 0 and one that ends at len
        "ends": ([b"ab"], b"ab" + b"x" * 100 + b"ab", [b"<ab>"]),
        "only a match": ([b"ab"], b"ab", [b""]),
        "empty text": ([b"ab"], b"", [b"q"]),
        "empty text, insertion": ([b""], b"", [b"q"]),
    }


@pytest.mark.parametrize("name", sorted(_edge_cases()))
def test_tile_edges(name):
    pats, hay, table = _edge_cases()[name]
    o, p, api = _pair(pats)
    k = len(o.find_iter(hay))
    assert not name.startswith("copy") or k == 0
    if name == "dense":
        assert T // len(table[0]) - 1 > STAGE   # segments that begin inside one tile
    if name.startswith("ties"):
        assert k > 2 * STAGE
    for dev in (False, True, 5):
        got = _check(o, p, api, hay, table, dev, what=name)
        assert name != "all deleted" or got == b""
    # the device form: a buffer of out_len bytes (none when the result is empty), and the number of matches replaced
    dm = p.replace_all(_dev(hay), table[0] if len(table) == 1 else table, device=True)
    assert dm.n_replaced == k and dm.dtype == np.uint8
    assert (dm.ptr is None) == (dm.count == 0)
    assert dm.to_numpy().tobytes() == _want(o, api, hay, table)
    dm.free()


# ---------------------------------------------------------------------------------------------------------------- 4. bad value
def test_a_value_without_replacement_answers_1():
    pats = [b"ab", b"b", b"cd", b"dd", b"e", b"ff", b"gab", b"h", b"ij", b"jj"]
    o = orc.OraclePma.build(pats, values=np.arange(10, dtype=np.uint32))
    p = da.DoubleArrayAhoCorasick.with_values(list(zip(pats, range(10))))
    assert p.serialize() == o.serialize()
    hay = b"xx ab cd e ab ff h ab jj gab " * 300
    m = o.find_iter(hay)
    first = next(x for x in m if x["value"] >= 5)
    for arg in (hay, _dev(hay)):
        with pytest.raises(da.DaachorseError) as ei:
            p.replace_all(arg, [b"<%d>" % i for i in range(5)])
        assert ei.value.code == 1
        assert f"value {int(first['value'])}:" in str(ei.value) and f"start {int(first['start'])})" in str(ei.value), str(ei.value)
    with pytest.raises(da.DaachorseError) as ei:
        p.replace_all_batch([b"ab", hay, b""], [b"<%d>" % i for i in range(5)])
    assert ei.value.code == 1 and f"value {int(first['value'])}:" in str(ei.value)
    # ten replacements serve every value, and one serves them all
    table = [b"<%d>" % i for i in range(10)]
    assert p.replace_all(hay, table) == _splice(hay, m, table)
    assert p.replace_all(hay, b"") == _splice(hay, m, [b""])


# -------------------------------------------------------------------------------------------------------------------- 5. batch
def _device_batch(docs):
    blobs = [_b(d) for d in docs]
    off = np.zeros(len(blobs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    hay = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)[:int(off[-1])].copy()
    return torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()


def _check_batch(o, p, api, docs, table, what=None, route=""):
    wants = [_want(o, api, d, table) for d in docs]
    repl = table[0] if len(table) == 1 else table
    for batch in (docs, _device_batch(docs)):
        if any(w is None for w in wants):
            first = next(i for i, w in enumerate(wants) if w is None)
            with pytest.raises(da.DaachorseError) as ei:
                p.replace_all_batch(batch, repl)
            assert ei.value.code == 6 and f"document {first}:" in str(ei.value), (what, str(ei.value))
            continue
        got = p.replace_all_batch(batch, repl)
        assert got == wants, what
        assert da.last_kernel().startswith("replace matches=") and " batch " in da.last_kernel() and route in da.last_kernel(), da.last_kernel()
        dm, do = p.replace_all_batch(batch, repl, device=True)
        assert do.to_numpy().tolist() == [0] + np.cumsum([len(w) for w in wants]).tolist(), what
        assert dm.to_numpy().tobytes() == b"".join(wants) and dm.count == sum(len(w) for w in wants), what
        assert (dm.ptr is None) == (dm.count == 0)
        dm.free()
        do.free()
    if all(w is not None for w in wants):   # each document equals replace_all of it alone
        for d, w in list(zip(docs, wants))[:12]:
            assert p.replace_all(d, repl) == w, what
    return wants


@pytest.mark.parametrize("kind", [0, 1])
def test_batch(kind):
    rng = np.random.default_rng(77 + kind)
    pats = [b"abc", b"bc", b"c", b"cab", b"aa"]
    o, p, api = _pair(pats, kind)
    p.set_option("batch_lane_max", 300)
    long_doc = bytes(rng.choice(list(b"abc"), size=5000).tolist())   # beyond batch_lane_max: the single-haystack route
    # "ab" + "c..." and "ca" + "b": a pattern would match across these boundaries and must not
    docs = [b"", b"a", b"ab", b"cab", b"ca", b"b", b"", b"", long_doc, b"c", bytes(rng.choice(list(b"abc"), size=299).tolist()),
            bytes(rng.choice(list(b"abc"), size=301).tolist()), b"", b"abcabc" * 40, b"x" * T, b"aa" * (T // 2), b""]
    for table in ([b"<%d>" % i for i in range(len(pats))], [b""], [b"0123456789abcdefXYZ"]):
        wants = _check_batch(o, p, api, docs, table, what=(kind, table[0]), route="long_docs=4")
        assert b"".join(wants) != _want(o, api, b"".join(docs), table)   # the concatenation has matches across boundaries
    # n = 0: no result, one offset
    for batch in ([], _device_batch([])):
        assert p.replace_all_batch(batch, b"x") == []
        dm, do = p.replace_all_batch(batch, b"x", device=True)
        assert dm.ptr is None and dm.count == 0 and do.to_numpy().tolist() == [0]
        do.free()
    # only empty documents
    _check_batch(o, p, api, [b"", b"", b""], [b"x"])


def test_batch_with_insertions_and_note_d():
    """"" among the patterns: every document gets its insertions at 0 .. len; a leftmost automaton whose document ends inside a longer
    pattern makes the call answer 6, naming the document"""
    o, p, api = _pair([b"", b"ab"], 0)
    _check_batch(o, p, api, [b"", b"a", b"abab", b"", b"xaby"], [b"-", b"<1>"])
    o, p, api = _pair([b"", b"abc"], 1)
    _check_batch(o, p, api, [b"xx", b"abcx", b""], [b"-", b"<1>"])
    wants = _check_batch(o, p, api, [b"xx", b"abcx", b"zab", b"ab"], [b"-", b"<1>"])
    assert wants[2] is None and wants[0] is not None


def test_batch_charwise():
    pats = ["全世界", "世界", "界", "a", "é世"]
    docs = ["全世界中に世界の世", "", "a", "é世界aé", "世", "界全世界" * 200]
    for kind in (0, 1):
        o, p, api = _pair(pats, kind, charwise=True)
        p.set_option("batch_lane_max", 300)
        _check_batch(o, p, api, docs, ["〈%d〉" % i for i in range(len(pats))], what=kind)
        _check_batch(o, p, api, docs, ["é"], what=kind)


# -------------------------------------------------------------------------------------------------------- 6. a real dictionary
def _numpy_splice(hay, m, table):
    """the same splice, vectorised: the pieces gap_0, r_0, gap_1, r_1, .. , gap_k gathered from [hay | blob]"""
    blob = np.frombuffer(b"".join(table) or b"\0", dtype=np.uint8)
    roff = np.zeros(len(table) + 1, dtype=np.int64)
    roff[1:] = np.cumsum([len(r) for r in table])
    idx = np.zeros(len(m), dtype=np.int64) if len(table) == 1 else m["value"].astype(np.int64)
    k = len(m)
    start, end = m["start"].astype(np.int64), m["end"].astype(np.int64)
    plen = np.zeros(2 * k + 1, dtype=np.int64)
    psrc = np.zeros(2 * k + 1, dtype=np.int64)
    plen[0::2] = np.concatenate([start, [len(hay)]]) - np.concatenate([[0], end])
    psrc[0::2] = np.concatenate([[0], end])
    plen[1::2] = roff[idx + 1] - roff[idx]
    psrc[1::2] = len(hay) + roff[idx]
    assert plen.min() >= 0
    at = np.cumsum(plen) - plen
    src = np.concatenate([hay, blob])
    return src[np.repeat(psrc - at, plen) + np.arange(int(plen.sum()), dtype=np.int64)]


@pytest.mark.parametrize("kind", [0, 1])
def test_cfg3_16mib(kind):
    pats = synth.patterns_cfg3(2000)
    o, p, api = _pair(pats, kind)
    mode = ScanMode.Find if kind == 0 else ScanMode.LeftmostFind
    table = [b"<%d>" % i for i in range(len(pats))] if kind == 0 else [b"[redacted]"]
    repl = table if kind == 0 else table[0]
    dev = torch.empty(16 << 20, dtype=torch.uint8, device="cuda")
    for text in ("word soup", "uniform"):
        if text == "uniform":
            synth.device_uniform(dev, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
        else:
            synth.device_wordsoup(dev, synth.SEEDS["cfg3_dense"], pats, 20)
        host = dev.cpu().numpy()
        # the first 1 MiB against the oracle splice
        want_1m = _want(o, api, host[:1 << 20].tobytes(), table)
        assert p.replace_all(dev[:1 << 20], repl) == want_1m, text
        # ... and with the selection route forced through windows of 12 KiB + 17: many restarts
        p.set_option("find3_window", 8192 + 4096 + 17).set_option("left3" if kind else "find3", 2)
        assert p.replace_all(dev[:1 << 20], repl) == want_1m, text
        p.set_option("find3_window").set_option("left3" if kind else "find3")
        # the whole against the library's own tuples, spliced by numpy
        m = p.scan(mode, dev)
        assert len(m) > 1000, text
        want = _numpy_splice(host, m, table)
        dm = p.replace_all(dev, repl, device=True)
        sum_l = int((m["end"] - m["start"]).sum())
        sum_r = len(m) * len(table[0]) if kind else int(np.array([len(r) for r in table])[m["value"]].sum())
        assert dm.count == len(host) - sum_l + sum_r == len(want), text
        assert dm.n_replaced == len(m) == p.count(mode, dev), text
        assert np.array_equal(dm.to_numpy(), want), text
        dm.free()


# ------------------------------------------------------------------------------------------------------------------ 7. charwise
@pytest.mark.parametrize("kind", [0, 1])
def test_charwise_cfg5(kind):
    pats = synth.patterns_cfg5(400)
    o, p, api = _pair(pats, kind, charwise=True)
    hay = synth.zipf_text(48 * 4000).tobytes().decode("utf-8")
    assert len(getattr(o, api)(hay)) > 1000
    for table in (["〈%d〉" % i for i in range(len(pats))], ["世"], [""]):
        _check(o, p, api, hay, table, dev=False, what=(kind, table[0]))
        _check(o, p, api, hay, table, dev=7, what=(kind, table[0]))
