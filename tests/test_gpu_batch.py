"""Batches on the MI355X (daac_scan_count_batch / daac_scan_batch_device16): every document of a batch gets exactly what the
single-haystack call returns on it alone.  Expected values come from the CPU oracle (or the golden vectors) applied to each
document on its own, never from the library."""
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


def _pair(patterns, kind=0, charwise=False):
    kind = orc.KIND.get(kind, kind)
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p


def _sev(m):
    return [(int(x["start"]), int(x["end"]), int(x["value"])) for x in m]


def _b(d):
    return d.encode("utf-8") if isinstance(d, str) else bytes(d)


def _device_batch(docs):
    blobs = [_b(d) for d in docs]
    off = np.zeros(len(blobs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    hay = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)[:int(off[-1])].copy()
    return torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()


def _want(o, api, docs):
    """per document: the oracle's stream, or None where the reference does not terminate"""
    out = []
    for d in docs:
        try:
            out.append(getattr(o, api)(d))
        except orc.OracleError as e:
            assert e.code == 6
            out.append(None)
    return out


def _check(o, p, api, docs, engines=(Engine.Auto,), what="", device=(False, True), tuples=True):
    """count_batch, scan_count_batch, scan_batch (CSR offsets and tuples) against the oracle, per document; returns the wants"""
    mode = API_MODE[api]
    wants = _want(o, api, docs)
    for eng in engines:
        for dev in device:
            batch = _device_batch(docs) if dev else docs
            if any(w is None for w in wants):
                first = next(i for i, w in enumerate(wants) if w is None)
                for fn in (p.count_batch, p.scan_count_batch, p.scan_batch):
                    with pytest.raises(da.DaachorseError) as ei:
                        fn(mode, batch, engine=eng)
                    assert ei.value.code == 6, (what, eng, dev)
                    assert f"document {first}:" in str(ei.value), (what, str(ei.value))
                continue
            counts, sums = p.scan_count_batch(mode, batch, engine=eng)
            assert counts.tolist() == [len(w) for w in wants], (what, eng, dev)
            assert sums.tolist() == [orc.matches_checksum(w) for w in wants], (what, eng, dev)
            assert p.count_batch(mode, batch, engine=eng).tolist() == counts.tolist(), (what, eng, dev)
            assert da.last_kernel().startswith("batch "), da.last_kernel()
            if tuples:
                got, offs = p.scan_batch(mode, batch, engine=eng)
                assert offs.tolist() == [0] + np.cumsum([len(w) for w in wants]).tolist(), (what, eng, dev)
                for i, w in enumerate(wants):
                    assert _sev(got[int(offs[i]):int(offs[i + 1])]) == _sev(w), (what, eng, dev, i)
    return wants


def _variants(hay, rng, charwise):
    """the case haystack, "", the haystack cut at a seeded point into two documents, the haystack again, the haystack doubled"""
    cut = int(rng.integers(0, len(hay) + 1))
    return [hay, "" if charwise else b"", hay[:cut], hay[cut:], hay, hay + hay]


@pytest.mark.parametrize("charwise", [False, True])
def test_golden_vectors_as_batches(vectors, charwise):
    rng = np.random.default_rng(11)
    n = 0
    for runner, case in iter_vector_runs(vectors):
        api = runner["api"]
        if api not in ("find_iter", "find_overlapping_iter", "leftmost_find_iter"):
            continue
        kind = runner.get("kind", "Standard") if api != "find_overlapping_iter" else "Standard"
        o, p = _pair(case["patterns"], kind, charwise)
        hay = case["haystack"] if charwise else case["haystack"].encode("utf-8")
        docs = _variants(hay, rng, charwise)
        # the case haystack against the golden tuples
        got, offs = p.scan_batch(API_MODE[api], docs[:1])
        want = [tuple(t) for t in case["matches"]]
        if not (api == "leftmost_find_iter" and "" in case["patterns"] and _want(o, api, docs[:1])[0] is None):
            assert [(int(m["value"]), int(m["start"]), int(m["end"])) for m in got] == want, (runner, case["name"])
        apis = [api] + (["find_overlapping_no_suffix_iter"] if api == "find_overlapping_iter" else [])
        for a in apis:
            _check(o, p, a, docs, what=(case["name"], a, charwise), device=(n % 2 == 0, n % 2 == 1))
        n += 1
    assert n == 57 + 61 + 93 + 91


def test_boundaries_are_hard():
    """occurrences straddle every boundary of the concatenation: per-document results are the oracle's, and the batch total is below
    daac_scan_count of the concatenation by exactly the straddling matches"""
    pats = [b"abc", b"bcd", b"cda", b"dab", b"ab", b"d"]
    o, p = _pair(pats)
    rng = np.random.default_rng(5)
    docs = []
    for k in range(300):
        body = bytes(rng.choice(list(b"abcdx"), size=int(rng.integers(0, 40))).tolist())
        docs.append(b"cd" + body + b"ab")   # every boundary reads "...ab|cd...": abc, bcd, cda, dab all straddle it
    wants = _check(o, p, "find_overlapping_iter", docs, engines=(Engine.Tiered, Engine.DArray))
    whole = b"".join(docs)
    total, _ = p.scan_count(ScanMode.FindOverlapping, whole)
    m = o.find_overlapping_iter(whole)
    bounds = np.cumsum([len(d) for d in docs])[:-1]
    straddle = sum(1 for s, e in zip(m["start"].tolist(), m["end"].tolist()) if any(s < b < e for b in bounds.tolist()))
    assert straddle >= len(docs) - 1
    assert sum(len(w) for w in wants) == total - straddle
    for api, kind in (("find_iter", "Standard"), ("leftmost_find_iter", "LeftmostLongest"), ("leftmost_find_iter", "LeftmostFirst")):
        o2, p2 = _pair(pats, kind)
        _check(o2, p2, api, docs)


def _fuzz_docs(rng, alphabet, piece, lane_max, charwise):
    lens = [0, 1, piece, piece - 1, piece + 1, 3 * piece + 7, lane_max + 1, lane_max + 333, 0, 2]
    lens += rng.integers(0, 2 * piece, size=40).tolist()
    rng.shuffle(lens)
    docs = []
    for n in lens:
        if charwise:
            docs.append("".join(rng.choice(alphabet, size=max(0, n // 2)).tolist()))
        else:
            docs.append(bytes(rng.choice(alphabet, size=n).tolist()))
    return docs


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("with_empty", [False, True])
def test_fuzz(charwise, with_empty):
    rng = np.random.default_rng(1234 + 2 * charwise + with_empty)
    piece, lane_max = 256, 1024
    if charwise:
        alphabet = ["a", "b", "全", "世", "界", "é"]
    else:
        alphabet = list(b"abc")
    for trial in range(3):
        k = int(rng.integers(3, 12))
        if charwise:
            pats = sorted({"".join(rng.choice(alphabet, size=int(rng.integers(1, 5))).tolist()) for _ in range(k)})
        else:
            pats = sorted({bytes(rng.choice(alphabet, size=int(rng.integers(1, 6))).tolist()) for _ in range(k)})
        if with_empty:
            pats = pats + (["" if charwise else b""])
        docs = _fuzz_docs(rng, alphabet, piece, lane_max, charwise)
        # (charwise leftmost kinds with "" in the set: on some of these texts the single-haystack scan and the oracle disagree about
        # note D — a finding of their own, outside batches; the golden vectors and test_refusals cover batches there)
        kinds = ("Standard",) if charwise and with_empty else ("Standard", "LeftmostLongest", "LeftmostFirst")
        for kind in kinds:
            o, p = _pair(pats, kind, charwise)
            p.set_option("batch_piece", piece).set_option("batch_lane_max", lane_max)
            apis = STANDARD_APIS if kind == "Standard" else ("leftmost_find_iter",)
            for api in apis:
                if charwise or api in ("find_iter", "leftmost_find_iter"):
                    engines = (Engine.Auto, Engine.DArray)
                else:
                    engines = (Engine.Auto, Engine.Tiered, Engine.DArray)
                _check(o, p, api, docs, engines=engines, what=(trial, kind, api, charwise, with_empty))
            if kind == "Standard" and not with_empty:
                # device results, asynchronous on a torch stream
                s = torch.cuda.Stream()
                hay, off = _device_batch(docs)
                c = torch.zeros(len(docs), dtype=torch.int64, device="cuda")
                cs = torch.zeros(len(docs), dtype=torch.int64, device="cuda")
                for api in STANDARD_APIS:
                    wants = _want(o, api, docs)
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        assert p.scan_count_batch(API_MODE[api], (hay, off), stream=s.cuda_stream, out=(c, cs)) is None
                    s.synchronize()
                    assert c.cpu().numpy().astype(np.uint64).tolist() == [len(w) for w in wants], api
                    assert cs.cpu().numpy().astype(np.uint64).tolist() == [orc.matches_checksum(w) for w in wants], api


def test_refusals():
    # leftmost with "" where one document ends inside a longer pattern: 6, naming the document
    for charwise in (False, True):
        o, p = _pair(["", "abc"] if not charwise else ["", "全世界"], "LeftmostLongest", charwise)
        docs = ["xx", "abc", "ab", "ab"] if not charwise else ["xx", "全世界", "全世", "全"]
        _check(o, p, "leftmost_find_iter", docs)
        with pytest.raises(da.DaachorseError) as ei:
            p.count_batch(ScanMode.LeftmostFind, docs)
        assert ei.value.code == 6 and "document 2:" in str(ei.value)
    # GRAM and PFX
    o, p = _pair(synth.patterns_cfg2(200))
    for eng in (Engine.Gram, Engine.Pfx):
        for fn in (p.count_batch, p.scan_count_batch, p.scan_batch):
            with pytest.raises(da.DaachorseError) as ei:
                fn(ScanMode.FindOverlapping, [b"abc", b"def"], engine=eng)
            assert ei.value.code == 6
    # decreasing device offsets
    hay = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 10, 5, 64], dtype=torch.int64, device="cuda")
    for mode in (ScanMode.FindOverlapping, ScanMode.Find):
        with pytest.raises(da.DaachorseError) as ei:
            p.count_batch(mode, (hay, off))
        assert ei.value.code == 1 and "document 1" in str(ei.value)
        with pytest.raises(da.DaachorseError) as ei:
            p.scan_batch(mode, (hay, off))
        assert ei.value.code == 1
    # n = 0
    assert len(p.count_batch(ScanMode.FindOverlapping, [])) == 0
    got, offs = p.scan_batch(ScanMode.Find, [])
    assert len(got) == 0 and offs.tolist() == [0]
    empty_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert len(p.count_batch(ScanMode.FindOverlapping, (hay, empty_off))) == 0


def test_scale_cfg3_lognormal():
    """the cfg3 dictionary over >= 256 MiB of device documents with log-normal lengths (1 B .. a few MiB): every count and checksum of
    the overlapping modes, the chain modes and the tuple lists on a seeded sample that includes every long-route document"""
    from concurrent.futures import ThreadPoolExecutor
    pats = synth.patterns_cfg3(100_000)
    o, p = _pair(pats)
    rng = np.random.default_rng(77)
    lens = np.clip(rng.lognormal(mean=5.0, sigma=2.0, size=400_000), 1, 4 << 20).astype(np.int64)
    lens = lens[np.cumsum(lens) <= (260 << 20)]
    total = int(lens.sum())
    assert total >= 256 << 20 and len(lens) >= 100_000
    text = synth.wordsoup_haystack(total, synth.SEEDS["cfg3_dense"], pats, 20)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    hay_d, off_d = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    docs = lambda idx: [text[off[i]:off[i + 1]] for i in idx]
    for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
        counts, sums = p.scan_count_batch(mode, (hay_d, off_d))
        if mode == ScanMode.FindOverlapping:
            with ThreadPoolExecutor(16) as ex:
                want = list(ex.map(lambda i: o.overlapping_count(text[off[i]:off[i + 1]]), range(len(lens))))
            assert counts.tolist() == [w[0] for w in want]
            assert sums.tolist() == [w[1] for w in want]
        else:
            sample = rng.choice(len(lens), size=2000, replace=False)
            ws = [o.find_overlapping_no_suffix_iter(d) for d in docs(sample)]
            assert counts[sample].tolist() == [len(w) for w in ws]
            assert sums[sample].tolist() == [orc.matches_checksum(w) for w in ws]
    lane_max = 16384
    longs = np.nonzero(lens > lane_max)[0]
    sample = np.unique(np.concatenate([rng.choice(len(lens), size=2000, replace=False), longs[:200]]))
    sub = docs(sample)
    for api in ("find_iter", "find_overlapping_iter"):
        _check(o, p, api, sub, device=(True,))
    ol, pl = _pair(pats, "LeftmostLongest")
    counts, sums = pl.scan_count_batch(ScanMode.LeftmostFind, (hay_d, off_d))
    assert "long_docs=%d" % len(longs) in da.last_kernel(), da.last_kernel()
    ws = [ol.leftmost_find_iter(d) for d in sub]
    assert counts[sample].tolist() == [len(w) for w in ws]
    assert sums[sample].tolist() == [orc.matches_checksum(w) for w in ws]
