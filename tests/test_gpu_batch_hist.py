"""Per-document pattern counts of a batch on the MI355X (daac_scan_histogram_batch): for every document the rows {slot, count} of the
matches the single-haystack iterator reports on it alone, in ascending slot order.  Expected values come from the CPU oracle's tuple
stream of each document on its own, each tuple mapped to its slot by (value, end - start) against the oracle's own outputs(); the
middle-sized runs are held against the library's independent count / checksum / histogram kernels instead."""
import re

import numpy as np
import pytest
import torch

from conftest import iter_vector_runs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

API_MODE = {"find_overlapping_iter": ScanMode.FindOverlapping, "find_overlapping_no_suffix_iter": ScanMode.FindOverlappingNoSuffix,
            "find_iter": ScanMode.Find, "leftmost_find_iter": ScanMode.LeftmostFind}
STANDARD_APIS = ("find_overlapping_iter", "find_overlapping_no_suffix_iter", "find_iter")
SETTINGS = ((None, None), (4, 16), (0, 16), (0, 0))   # (batch_hist_wave_max, batch_hist_sort_max); None: the default
DEFAULT_WAVE_MAX, DEFAULT_SORT_MAX = 2048, 16384


def _pair(patterns, kind=0, charwise=False, values=None):
    kind = orc.KIND.get(kind, kind)
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p


def _keys(value, length):
    return (np.asarray(value, dtype=np.uint64) << np.uint64(32)) | np.asarray(length, dtype=np.uint64)


class _Slots:
    """(value, length) -> slot against the oracle's outputs(), asserted one to one"""

    def __init__(self, o):
        outs = o.outputs()
        self.n = len(outs)
        keys = _keys(outs[:, 0], outs[:, 1]) if self.n else np.zeros(0, dtype=np.uint64)
        self.order = np.argsort(keys, kind="stable")
        self.sk = keys[self.order]
        assert len(np.unique(self.sk)) == len(self.sk), "patterns share (value, length)"

    def rows(self, m):
        """the oracle's tuples of one document -> [(slot, count)], ascending slots"""
        if len(m) == 0:
            return []
        mk = _keys(m["value"], m["end"] - m["start"])
        at = np.searchsorted(self.sk, mk)
        assert np.all(at < len(self.sk)) and np.array_equal(self.sk[np.minimum(at, len(self.sk) - 1)], mk)
        c = np.bincount(self.order[at], minlength=self.n)
        nz = np.nonzero(c)[0]
        return list(zip(nz.tolist(), c[nz].tolist()))


def _want(o, api, docs, slots=None):
    """per document: the oracle's rows, or None where the reference does not terminate (note D)"""
    slots = slots or _Slots(o)
    out = []
    for d in docs:
        try:
            out.append(slots.rows(getattr(o, api)(d)))
        except orc.OracleError as e:
            assert e.code == 6
            out.append(None)
    return out


def _b(d):
    return d.encode("utf-8") if isinstance(d, str) else bytes(d)


def _device_batch(docs, lead=0):
    """(uint8 CUDA tensor, int64 CUDA offsets); `lead` bytes of other text in front, so that offsets[0] = lead"""
    blobs = [_b(d) for d in docs]
    off = np.zeros(len(blobs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    off += lead
    hay = np.frombuffer(b"a" * lead + b"".join(blobs) + b"\0", dtype=np.uint8)[:int(off[-1]) or 1].copy()
    return torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()


def _route():
    lk = da.last_kernel()
    assert lk.startswith("batch_hist "), lk
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lk)}


def _split(wants, wave_max, sort_max):
    """how many documents each route takes, from the oracle's record counts"""
    r = [sum(c for _, c in w) for w in wants]
    wave = sum(1 for x in r if x <= wave_max)
    group = sum(1 for x in r if wave_max < x <= sort_max)
    return {"records": sum(r), "wave_docs": wave, "group_docs": group, "dense_docs": len(r) - wave - group}


def _set(p, wave_max, sort_max):
    p.set_option("batch_hist_wave_max", wave_max).set_option("batch_hist_sort_max", sort_max)
    return (DEFAULT_WAVE_MAX if wave_max is None else wave_max), (DEFAULT_SORT_MAX if sort_max is None else sort_max)


def _check(p, mode, batch, wants, what, split=None):
    """rows and offsets against the wants, bit for bit; with `split` = (wave_max, sort_max) also the route each document took"""
    if any(w is None for w in wants):
        first = next(i for i, w in enumerate(wants) if w is None)
        with pytest.raises(da.DaachorseError) as ei:
            p.histogram_batch(mode, batch)
        assert ei.value.code == 6 and f"document {first}:" in str(ei.value), (what, str(ei.value))
        return
    rows, offs = p.histogram_batch(mode, batch)
    assert rows.dtype == da.SLOT_COUNT_DTYPE and offs.dtype == np.uint64
    assert offs.tolist() == [0] + np.cumsum([len(w) for w in wants]).tolist(), what
    assert list(zip(rows["slot"].tolist(), rows["count"].tolist())) == [rc for w in wants for rc in w], what
    if split is not None:
        got = _route()
        want = _split(wants, *split)
        assert {k: got[k] for k in want} == want, (what, da.last_kernel())


# --------------------------------------------------------------------------------------------------------------- 1. golden vectors
@pytest.mark.parametrize("charwise", [False, True])
def test_golden_vectors(vectors, charwise):
    n = 0
    for runner, case in iter_vector_runs(vectors):
        api = runner["api"]
        if api not in API_MODE:
            continue
        kind = runner.get("kind", "Standard") if api == "leftmost_find_iter" else "Standard"
        o, p = _pair(case["patterns"], kind, charwise)
        hay = case["haystack"] if charwise else case["haystack"].encode("utf-8")
        docs = [hay, "" if charwise else b"", hay[:len(hay) // 2], hay]
        slots = _Slots(o)
        apis = [api] + (["find_overlapping_no_suffix_iter"] if api == "find_overlapping_iter" else [])
        for a in apis:
            wants = _want(o, a, docs, slots)
            _check(p, API_MODE[a], _device_batch(docs) if n % 2 else docs, wants, (case["name"], a, charwise), split=(DEFAULT_WAVE_MAX, DEFAULT_SORT_MAX))
        n += 1
    assert n == 57 + 61 + 93 + 91


# --------------------------------------------------------------------------------------------------------------------- 2, 3. fuzz
def _fuzz_dicts(rng):
    dicts = [([b"a", b"aa", b"aaa", b"baaa", b"ab", b"abc", b"abcd"], False),      # a suffix chain of depth 3 under baaa, shared prefixes
             ([b"", b"a", b"aa", b"aaa", b"baaa", b"ab", b"b"], True),             # ... with ROOT's own list (Standard only)
             ([b"ab", b"b", b"ab", b"bab", b"ab", b"abab", b"a", b"cabab"], True)]   # copies of one pattern inside chains (Standard only)
    k = int(rng.integers(8, 41))
    pats = list(dict.fromkeys(bytes(rng.choice(list(b"abc"), size=int(rng.integers(1, 7))).tolist()) for _ in range(k)))
    dicts.append((pats, False))
    return dicts


def _fuzz_docs(rng, alphabet, charwise):
    n = int(rng.integers(40, 201))
    lens = [0] + rng.integers(0, 301, size=n - 2).tolist() + [0]
    lens[1], lens[2], lens[3] = 300, 64, 65
    if charwise:
        return ["".join(rng.choice(alphabet, size=x // 2).tolist()) for x in lens]
    return [bytes(rng.choice(alphabet, size=x).tolist()) for x in lens]


def _fuzz(dicts, alphabet, charwise, seed):
    rng = np.random.default_rng(seed)
    routes_seen = set()
    for pats, standard_only in dicts:
        docs = _fuzz_docs(rng, alphabet, charwise)
        batches = (docs, _device_batch(docs))
        for kind in (("Standard",) if standard_only else ("Standard", "LeftmostLongest", "LeftmostFirst")):
            o, p = _pair(pats, kind, charwise)
            p.set_option("batch_piece", 64)
            slots = _Slots(o)
            for api in (STANDARD_APIS if kind == "Standard" else ("leftmost_find_iter",)):
                wants = _want(o, api, docs, slots)
                assert all(w is not None for w in wants)
                for k, (wm, sm) in enumerate(SETTINGS):
                    split = _set(p, wm, sm)
                    _check(p, API_MODE[api], batches[k % 2], wants, (pats, kind, api, wm, sm), split=split)
                    r = _route()
                    routes_seen |= {name for name in ("wave_docs", "group_docs", "dense_docs") if r[name]}
                    if (wm, sm) == (0, 0):
                        assert r["group_docs"] == 0 and r["dense_docs"] == sum(1 for w in wants if w)
                    if api != "find_iter" and kind == "Standard":
                        assert r["pieces"] > len(docs)   # documents span pieces
    assert routes_seen == {"wave_docs", "group_docs", "dense_docs"}


def test_fuzz_bytewise():
    rng = np.random.default_rng(20271)
    _fuzz(_fuzz_dicts(rng), list(b"abc"), False, 20272)


def test_fuzz_charwise():
    alphabet = ["a", "é", "世", "界", "𝄞", "b"]          # 1-, 2-, 3-, 3- and 4-byte scalars
    rng = np.random.default_rng(20273)
    k = int(rng.integers(8, 41))
    dicts = [(["世", "世世", "世世世", "界世世世", "é", "𝄞世", "界世", "界世a"], False),
             (["", "a", "aa", "é", "éé", "aéé", "𝄞", "世𝄞", "aaéé"], True),
             (list(dict.fromkeys("".join(rng.choice(alphabet[:5], size=int(rng.integers(1, 5))).tolist()) for _ in range(k))), False)]
    _fuzz(dicts, alphabet + ["ж"], True, 20274)


# ------------------------------------------------------------------------------------------------------------ 4. route boundaries
ROUTES = {"wave": (1 << 12, 1 << 15), "group": (0, 1 << 15), "dense": (0, 0)}


def test_route_boundaries():
    o, p = _pair([b"a"])
    rs = [0, 1, 7, 8, 9, 31, 32, 33, 100]
    docs = [b"a" * r for r in rs]
    _set(p, 8, 32)
    for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix, ScanMode.Find):
        rows, offs = p.histogram_batch(mode, docs)
        assert offs.tolist() == [0] + list(range(0, len(rs))), mode          # R = 0: no row
        assert rows["slot"].tolist() == [0] * (len(rs) - 1) and rows["count"].tolist() == rs[1:], mode
        r = _route()
        assert (r["records"], r["wave_docs"], r["group_docs"], r["dense_docs"]) == (sum(rs), 4, 3, 2), da.last_kernel()
    # 64 distinct one-byte patterns, documents that are permutations of those bytes: every record is distinct, 64 singleton rows
    rng = np.random.default_rng(41)
    alphabet = np.arange(64, 128, dtype=np.uint8)
    o, p = _pair([bytes([c]) for c in alphabet.tolist()])
    docs = [bytes(rng.permutation(alphabet).tolist()) for _ in range(9)]
    wants = _want(o, "find_overlapping_iter", docs)
    assert all(w == [(s, 1) for s in range(64)] for w in wants)
    for name, (wm, sm) in ROUTES.items():
        split = _set(p, wm, sm)
        for mode in (ScanMode.FindOverlapping, ScanMode.Find):
            _check(p, mode, docs, wants, (name, mode), split=split)
            assert _route()[name + "_docs"] == len(docs)
    # the chain expansion counts on every route
    o, p = _pair([b"a", b"aa", b"aaa", b"aaaa"])
    docs = [b"a" * 50, b"", b"a" * 3]
    wants = _want(o, "find_overlapping_iter", docs)
    assert sorted(c for _, c in wants[0]) == [47, 48, 49, 50] and sum(c for _, c in wants[2]) == 6
    for name, (wm, sm) in ROUTES.items():
        split = _set(p, wm, sm)
        _check(p, ScanMode.FindOverlapping, docs, wants, name, split=split)
        assert _route()[name + "_docs"] >= 2


# ------------------------------------------------------------------------------------------------------ 5. shared (value, length)
@pytest.mark.parametrize("charwise", [False, True])
def test_shared_value_and_length(charwise):
    pats = ["ab", "cd", "abc", "bc", "d", "c", "dab"] if not charwise else ["世界", "界世", "世界a", "世世", "a", "b", "a世界"]
    values = [7, 7, 3, 7, 5, 5, 3]                       # ab / cd / bc share (7, 2), d / c share (5, 1), abc / dab share (3, 3)
    o_shared, p = _pair(pats, charwise=charwise, values=np.array(values, dtype=np.uint32))
    o, _ = _pair(pats, charwise=charwise)              # distinct values (the index), the same trie: the same slot order
    outs, outs_d = p.outputs(), o.outputs()
    assert outs["length"].tolist() == outs_d[:, 1].tolist() and outs["value"].tolist() == [values[v] for v in outs_d[:, 0].tolist()]
    assert len(set(zip(outs["value"].tolist(), outs["length"].tolist()))) < len(outs)
    rng = np.random.default_rng(51)
    alphabet = list("abcdx") if not charwise else ["世", "界", "a", "b", "x"]
    docs = ["".join(rng.choice(alphabet, size=int(rng.integers(0, 120))).tolist()) for _ in range(60)]
    if not charwise:
        docs = [d.encode() for d in docs]
    for api in STANDARD_APIS:
        wants = _want(o, api, docs)
        assert sum(len(w) for w in wants) > 100
        for wm, sm in SETTINGS:
            _set(p, wm, sm)
            _check(p, API_MODE[api], docs, wants, (api, wm, sm))
        # ... and per value, which the shared-value oracle's tuples carry
        rows, offs = p.histogram_batch(API_MODE[api], docs)
        for i in (1, len(docs) // 2, len(docs) - 1):
            part = rows[int(offs[i]):int(offs[i + 1])]
            by_value = np.zeros(8, dtype=np.int64)
            np.add.at(by_value, outs["value"][part["slot"]], part["count"])
            assert by_value.tolist() == np.bincount(getattr(o_shared, api)(docs[i])["value"].astype(np.int64), minlength=8).tolist(), (api, i)


# --------------------------------------------------------------------------------------------------------- 6. device in, device out
def test_device_in_device_out():
    pats = synth.patterns_cfg2(200) + [b"bcd", b"ab", b"a"]
    o, p = _pair(pats)
    rng = np.random.default_rng(61)
    text = synth.wordsoup_haystack(40 << 10, synth.SEEDS["cfg2_dense"], pats, 13, noise_256=32)
    cuts = np.concatenate([[0], np.sort(rng.integers(0, len(text), size=99)), [len(text)]])
    docs = [text[cuts[i]:cuts[i + 1]] for i in range(100)]
    hay, off = _device_batch([d.tobytes() for d in docs], lead=5)
    assert int(off[0]) == 5
    for api in STANDARD_APIS:
        wants = _want(o, api, docs)
        _check(p, API_MODE[api], (hay, off), wants, api)
        host_rows, host_offs = p.histogram_batch(API_MODE[api], docs)
        dm, do = p.histogram_batch_device(API_MODE[api], (hay, off))
        assert dm.dtype == da.SLOT_COUNT_DTYPE and dm.count == len(host_rows) and do.count == len(docs) + 1
        assert dm.to_numpy().tobytes() == host_rows.tobytes() and do.to_numpy().tolist() == host_offs.tolist(), api
        dm.free()
        do.free()
        assert dm.ptr is None and do.ptr is None
    # a decreasing device offset
    bad = torch.tensor([0, 10, 5, 64], dtype=torch.int64, device="cuda")
    for mode in (ScanMode.FindOverlapping, ScanMode.Find):
        with pytest.raises(da.DaachorseError) as ei:
            p.histogram_batch(mode, (hay, bad))
        assert ei.value.code == 1 and "document 1" in str(ei.value)
    # n = 0
    for batch in ([], (hay, torch.zeros(1, dtype=torch.int64, device="cuda"))):
        rows, offs = p.histogram_batch(ScanMode.Find, batch)
        assert len(rows) == 0 and rows.dtype == da.SLOT_COUNT_DTYPE and offs.tolist() == [0]
        dm, do = p.histogram_batch_device(ScanMode.FindOverlapping, batch)
        assert dm.count == 0 and not dm.ptr and do.to_numpy().tolist() == [0]
        dm.free()
        do.free()
    # a device batch with a chain-mode document beyond batch_lane_max: 6, naming document and option
    p.set_option("batch_lane_max", 300)
    long_off = torch.tensor([5, 100, 400, 701, 900], dtype=torch.int64, device="cuda")
    with pytest.raises(da.DaachorseError) as ei:
        p.histogram_batch(ScanMode.Find, (hay, long_off))
    assert ei.value.code == 6 and "document 2 " in str(ei.value) and "batch_lane_max" in str(ei.value)
    assert len(p.histogram_batch(ScanMode.FindOverlapping, (hay, long_off))[1]) == 5


# --------------------------------------------------------------------------------------------------- 7. cross-checks at middle size
def _h32(value, length):
    return synth.mix64(_keys(value, length)) & np.uint64(0xFFFFFFFF)


def test_cross_checks_cfg3_8mib():
    pats = synth.patterns_cfg3(2000)
    n = 8 << 20
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(dev, synth.SEEDS["cfg3_dense"], pats, 20)
    rng = np.random.default_rng(71)
    lens = rng.integers(64, 4097, size=n // 64)
    lens = lens[np.cumsum(lens) <= n]
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    off_d = torch.from_numpy(off).cuda()
    one = torch.tensor([0, 1 << 20], dtype=torch.int64, device="cuda")
    pmas = {"Standard": _pair(pats)[1], "LeftmostLongest": _pair(pats, "LeftmostLongest")[1]}
    for api, mode in API_MODE.items():
        p = pmas["LeftmostLongest" if api == "leftmost_find_iter" else "Standard"]
        outs = p.outputs()
        h = _h32(outs["value"], outs["length"])
        counts, sums = p.scan_count_batch(mode, (dev, off_d))
        rows, offs = p.histogram_batch(mode, (dev, off_d))
        r = _route()
        assert r["wave_docs"] + r["group_docs"] + r["dense_docs"] == len(lens) and r["records"] == int(counts.sum())
        assert len(offs) == len(lens) + 1 and int(offs[-1]) == len(rows) > len(lens)
        doc = np.repeat(np.arange(len(lens)), np.diff(offs).astype(np.int64))
        assert np.all((np.diff(rows["slot"].astype(np.int64)) > 0) | (np.diff(doc) > 0)) and np.all(rows["count"] > 0)   # ascending slots per document
        got_counts = np.zeros(len(lens), dtype=np.uint64)
        np.add.at(got_counts, doc, rows["count"].astype(np.uint64))
        assert got_counts.tolist() == counts.tolist(), api
        got_s1 = np.zeros(len(lens), dtype=np.uint64)
        np.add.at(got_s1, doc, (rows["count"].astype(np.uint64) * h[rows["slot"]]) & np.uint64(0xFFFFFFFF))
        assert (got_s1 & np.uint64(0xFFFFFFFF)).tolist() == (sums >> np.uint64(32)).tolist(), api
        if api in ("find_overlapping_iter", "find_overlapping_no_suffix_iter"):
            dense = p.histogram(mode, dev[:1 << 20])
            rows1, offs1 = p.histogram_batch(mode, (dev, one))
            assert _route()["dense_docs"] == 1
            nz = np.nonzero(dense)[0]
            assert offs1.tolist() == [0, len(nz)] and rows1["slot"].tolist() == nz.tolist() and rows1["count"].tolist() == dense[nz].tolist(), api


# ------------------------------------------------------------------------------------------------------------------ 8. host windows
def test_host_windows():
    """a host batch of 257 MiB + 13 bytes in 1 MiB documents goes as two staged windows (the driver's window constant is 256 MiB, so this
    is the smallest size that crosses it); it equals the device form of the same batch, whose documents all take the dense route"""
    pats = synth.patterns_cfg3(2000)
    o, p = _pair(pats)
    n = (257 << 20) + 13
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(dev, synth.SEEDS["cfg3_dense"], pats, 20)
    off = np.minimum(np.arange(0, 259, dtype=np.int64) << 20, n)
    assert off[-1] == n and off[-2] < n
    off_d = torch.from_numpy(off).cuda()
    rows_d, offs_d = p.histogram_batch(ScanMode.FindOverlapping, (dev, off_d))
    assert _route()["dense_docs"] == 257 and _route()["wave_docs"] == 1
    host = dev.cpu().numpy()
    rows_h, offs_h = p.histogram_batch(ScanMode.FindOverlapping, [host[off[i]:off[i + 1]] for i in range(258)])
    assert _route()["dense_docs"] == 257
    assert offs_h.tolist() == offs_d.tolist() and rows_h.tobytes() == rows_d.tobytes()
    assert int(rows_h["count"].sum()) == int(p.count_batch(ScanMode.FindOverlapping, (dev, off_d)).sum())   # (matches across the cuts are nobody's)
    assert int(rows_h["count"][int(offs_h[257]):].sum()) == p.count(ScanMode.FindOverlapping, dev[257 << 20:])


# ----------------------------------------------------------------------------------------------------- 9. refusals on the device
def test_refusals_on_the_device():
    # note D: a leftmost kind with "", a document that ends inside a longer pattern
    for charwise in (False, True):
        o, p = _pair(["", "abc"] if not charwise else ["", "全世界"], "LeftmostLongest", charwise)
        docs = ["xx", "abc", "ab", "ab"] if not charwise else ["xx", "全世界", "全世", "全"]
        wants = _want(o, "leftmost_find_iter", docs)
        assert [w is None for w in wants] == [False, False, True, True]
        for batch in (docs, _device_batch(docs)):
            _check(p, ScanMode.LeftmostFind, batch, wants, charwise)
        _check(p, ScanMode.LeftmostFind, docs[:2], wants[:2], charwise)
    # 8 bytes times the records against max_result_bytes: [aaaa, a * 20, ""] has 4 + 3 + 20 + 19 = 46 records
    o, p = _pair([b"a", b"aa"])
    docs = [b"aaaa", b"a" * 20, b""]
    p.set_option("max_result_bytes", 8 * 46)
    rows, offs = p.histogram_batch(ScanMode.FindOverlapping, docs)
    assert rows["count"].tolist() == [4, 3, 20, 19] and offs.tolist() == [0, 2, 4, 4]
    p.set_option("max_result_bytes", 8 * 46 - 1)
    for batch in (docs, _device_batch(docs)):
        with pytest.raises(da.DaachorseError) as ei:
            p.histogram_batch(ScanMode.FindOverlapping, batch)
        assert ei.value.code == 4 and "max_result_bytes" in str(ei.value)
    assert p.histogram_batch(ScanMode.Find, docs)[0]["count"].tolist() == [4, 20]      # the 24 records of find_iter fit
