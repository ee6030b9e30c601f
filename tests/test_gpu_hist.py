"""Histograms on the MI355X (daac_scan_histogram): per-pattern match counts of the overlapping scans.  Expected values come from the
CPU oracle's tuple stream, each tuple mapped to its slot by (value, end - start) against the oracle's own outputs(); the large runs
are also held against the library's independent count / checksum kernels."""
import numpy as np
import pytest
import torch

from conftest import iter_vector_runs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

MODES = (("find_overlapping_iter", ScanMode.FindOverlapping), ("find_overlapping_no_suffix_iter", ScanMode.FindOverlappingNoSuffix))


def _pair(patterns, values=None, charwise=False, opts=None):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    for k, v in (opts or {}).items():
        p.set_option(k, v)
    return o, p


def _keys(value, length):
    return (np.asarray(value, dtype=np.uint64) << np.uint64(32)) | np.asarray(length, dtype=np.uint64)


def _stream(o, api, hay, begin=0):
    """the oracle's tuples that a scan with this `begin` counts: end in (begin, len], ROOT's list at end 0 when begin == 0"""
    m = getattr(o, api)(hay)
    return m if begin == 0 else m[m["end"] > begin]


def _want(o, api, hay, begin=0):
    """counts per slot from the oracle's tuple stream (the (value, length) -> slot map must be one to one)"""
    outs = o.outputs()
    keys = _keys(outs[:, 0], outs[:, 1])
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    assert len(np.unique(sk)) == len(sk), "patterns share (value, length): use per-value sums"
    m = _stream(o, api, hay, begin)
    mk = _keys(m["value"], m["end"] - m["start"])
    at = np.searchsorted(sk, mk)
    assert np.all(at < len(sk)) and np.array_equal(sk[np.minimum(at, len(sk) - 1)], mk)
    return np.bincount(order[at], minlength=len(outs)).astype(np.uint64)


def _h32(value, length):
    return synth.mix64(_keys(value, length)) & np.uint64(0xFFFFFFFF)


def _s1(p, counts):
    """sum(counts[i] * h32(value_i, length_i)) mod 2^32: the S1 half of scan_count's checksum"""
    o = p.outputs()
    with np.errstate(over="ignore"):
        return int(np.sum(counts * _h32(o["value"], o["length"]), dtype=np.uint64) & np.uint64(0xFFFFFFFF))


def _dev(hay):
    a = np.frombuffer(hay.encode("utf-8") if isinstance(hay, str) else bytes(hay), dtype=np.uint8)
    return torch.from_numpy(a.copy()).cuda()


# --------------------------------------------------------------------------------------------------------------- 1. golden vectors
@pytest.mark.parametrize("charwise", [False, True])
def test_golden_vectors(vectors, charwise):
    n = 0
    for runner, case in iter_vector_runs(vectors):
        if runner["api"] != "find_overlapping_iter":
            continue
        o, p = _pair(case["patterns"], charwise=charwise)
        hay = case["haystack"] if charwise else case["haystack"].encode("utf-8")
        for api, mode in MODES:
            want = _want(o, api, hay)
            got = p.histogram(mode, hay if n % 2 else _dev(hay))
            assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (case["name"], api)
            assert da.last_kernel().startswith("hist "), da.last_kernel()
            assert int(got.sum()) == p.count(mode, hay), (case["name"], api)
            pc = p.pattern_counts(mode, hay)
            outs = p.outputs()
            assert pc.dtype.names == ("value", "length", "count")
            assert pc["count"].tolist() == got.tolist() and pc["value"].tolist() == outs["value"].tolist() and \
                pc["length"].tolist() == outs["length"].tolist(), (case["name"], api)
        n += 1
    assert n == 57


# --------------------------------------------------------------------------------------------------------- 2. small-alphabet fuzz
FUZZ_LENS = (0, 1, 15, 16, 17, 257, 3001)


def _fuzz_dicts(rng):
    dicts = [[b"a", b"aa", b"aaa", b"baaa"],                                   # one suffix chain: slot 3's hit feeds slots 2, 1, 0
             [b"", b"a", b"aa", b"aaa", b"baaa", b"ab", b"b"],                 # ... with ROOT's own list
             [b"ab", b"b", b"ab", b"bab", b"ab", b"abab", b"a"]]               # copies of one pattern inside chains
    for alphabet in (b"ab", b"abc"):
        k = int(rng.integers(5, 41))
        pats = [bytes(rng.choice(list(alphabet), size=int(rng.integers(1, 7))).tolist()) for _ in range(k)]
        pats = list(dict.fromkeys(pats))
        pats += [pats[0], pats[len(pats) // 2]]                                # copies
        if alphabet == b"abc":
            pats.append(b"")
        dicts.append(pats)
    return dicts


def _set_bins(p, bins):
    if bins is None:
        p.set_option("hist_lds_bins")   # the default
    else:
        p.set_option("hist_lds_bins", bins)


def test_fuzz_bytewise():
    rng = np.random.default_rng(20261)
    for pats in _fuzz_dicts(rng):
        o, p = _pair(pats, opts={"threads": 64})
        n_out = len(p.outputs())
        assert n_out == len(pats)
        alphabet = sorted({c for w in pats for c in w} | {ord("c")})
        texts = [bytes(rng.choice(alphabet, size=n).tolist()) for n in FUZZ_LENS]
        texts.append(b"baaa" * 40 + b"aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaab" * 10)
        wants = {(api, i): _want(o, api, t) for api, _ in MODES for i, t in enumerate(texts)}
        for seg in (16, 64):
            p.set_option("seg_bytes", seg)
            for bins in (0, 1, 3, None):
                _set_bins(p, bins)
                for eng in (Engine.Tiered, Engine.DArray):
                    for api, mode in MODES:
                        for i, t in enumerate(texts):
                            got = p.histogram(mode, t if (i + seg) % 2 else _dev(t), engine=eng)
                            assert got.tolist() == wants[(api, i)].tolist(), (pats, len(t), seg, bins, eng, api)
                            assert da.last_engine() == int(eng)
                if bins is not None:
                    assert da.last_kernel() == "hist eng=darray lds_bins=%d" % min(bins, n_out), da.last_kernel()


def test_fuzz_charwise():
    rng = np.random.default_rng(20262)
    alphabet = ["a", "é", "世", "界", "𝄞", "b"]          # 1-, 2-, 3-, 3- and 4-byte scalars
    dicts = [["世", "世世", "世世世", "界世世世", "é", "𝄞世"],
             ["", "a", "aa", "é", "éé", "aéé", "𝄞", "世𝄞", "a"]]
    k = int(rng.integers(5, 41))
    dicts.append(list(dict.fromkeys("".join(rng.choice(alphabet[:5], size=int(rng.integers(1, 5))).tolist()) for _ in range(k))))
    for pats in dicts:
        o, p = _pair(pats, charwise=True, opts={"threads": 64})
        # "b" and "ж" never occur in a pattern: scalars the code mapper does not know
        texts = ["".join(rng.choice(alphabet + ["ж"], size=n).tolist()).encode("utf-8") for n in (0, 1, 5, 6, 7, 90, 1100)]
        texts.append(("界世世世" * 30 + "世" * 40 + "ж世").encode("utf-8"))
        cases = []   # (text, begin): the whole text, and a `begin` inside a character (a continuation byte from a seeded point on)
        for raw in texts:
            cases.append((raw, 0))
            if len(raw) > 40:
                cases.append((raw, next(j for j in range(int(rng.integers(1, len(raw) - 8)), len(raw)) if raw[j] & 0xC0 == 0x80)))
        assert sum(1 for _, b in cases if b) >= 3
        wants = {(api, i): _want(o, api, raw, begin=b) for api, _ in MODES for i, (raw, b) in enumerate(cases)}
        for seg in (16, 64):
            p.set_option("seg_bytes", seg)
            for bins in (0, 1, 3, None):
                _set_bins(p, bins)
                for api, mode in MODES:
                    for i, (raw, b) in enumerate(cases):
                        got = p.histogram(mode, raw if (i + seg) % 2 else _dev(raw), engine=Engine.DArray, begin=b)
                        assert got.tolist() == wants[(api, i)].tolist(), (pats, len(raw), b, seg, bins, api)
                assert da.last_kernel().startswith("hist eng=char"), da.last_kernel()


# ------------------------------------------------------------------------------------------------------- 3. `begin` and sharding
def test_begin_and_sharding():
    pats = synth.patterns_cfg2(200)
    o, p = _pair(pats)
    hay = synth.wordsoup_haystack(64 << 10, synth.SEEDS["cfg2_dense"], pats, 13, noise_256=0)
    big = torch.zeros(len(hay) + 64, dtype=torch.uint8, device="cuda")
    big[5:5 + len(hay)] = torch.from_numpy(hay).cuda()
    forms = {"host": hay, "device": torch.from_numpy(hay).cuda(), "device, unaligned": big[5:5 + len(hay)]}
    assert forms["device, unaligned"].data_ptr() % 16 != 0
    rng = np.random.default_rng(31)
    cuts = [0, 1, len(hay) - 1, len(hay)] + rng.integers(2, len(hay) - 1, size=6).tolist()
    for api, mode in MODES:
        whole = _want(o, api, hay)
        assert whole.sum() > 4000
        for name, h in forms.items():
            for eng in (Engine.Auto, Engine.DArray):
                full = p.histogram(mode, h, engine=eng)
                assert full.tolist() == whole.tolist(), (api, name, eng)
                for cut in cuts:
                    head = p.histogram(mode, h[:cut], engine=eng)
                    tail = p.histogram(mode, h, begin=cut, engine=eng)
                    assert tail.tolist() == _want(o, api, hay, begin=cut).tolist(), (api, name, eng, cut)
                    assert (head + tail).tolist() == full.tolist(), (api, name, eng, cut)
                    assert int(tail.sum()) == p.count(mode, h, begin=cut), (api, name, eng, cut)


# ------------------------------------------------------------------------------------------------------------- 4. device output
def test_device_output():
    pats = synth.patterns_cfg2(200)
    o, p = _pair(pats)
    n = len(p.outputs())
    hay_a = synth.wordsoup_haystack(48 << 10, synth.SEEDS["cfg2_dense"], pats, 13, noise_256=0)
    hay_b = synth.uniform_haystack(32 << 10, synth.SEEDS["cfg2_hay"], b"abcdefgh") .copy()
    hay_b[1000:1000 + len(pats[7])] = np.frombuffer(pats[7], dtype=np.uint8)
    da_, db_ = torch.from_numpy(hay_a).cuda(), torch.from_numpy(hay_b).cuda()
    s = torch.cuda.Stream()
    for api, mode in MODES:
        want_a, want_b = _want(o, api, hay_a), _want(o, api, hay_b)
        assert want_a.tolist() != want_b.tolist()
        out_a = torch.full((n,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")   # garbage: the call overwrites it
        out_b = torch.full((n + 3,), 77, dtype=torch.int64, device="cuda")                  # a longer tensor: the first n are written
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            # two calls back to back on one stream, nothing waited for in between
            assert p.histogram(mode, da_, stream=s.cuda_stream, out=out_a) is None
            assert p.histogram(mode, db_, stream=s.cuda_stream, out=out_b) is None
        s.synchronize()
        assert out_a.cpu().numpy().astype(np.uint64).tolist() == want_a.tolist(), api
        assert out_b[:n].cpu().numpy().astype(np.uint64).tolist() == want_b.tolist(), api
        assert out_b[n:].tolist() == [77, 77, 77]
        assert p.histogram(mode, da_).tolist() == want_a.tolist(), api
        # a host haystack into a device array
        assert p.histogram(mode, hay_b, out=out_a) is None
        torch.cuda.synchronize()
        assert out_a.cpu().numpy().astype(np.uint64).tolist() == want_b.tolist(), api
    with pytest.raises(da.DaachorseError) as ei:
        p.histogram(ScanMode.FindOverlapping, da_, out=torch.zeros(n - 1, dtype=torch.int64, device="cuda"))
    assert ei.value.code == 1


# -------------------------------------------------------------------------------------------------------------- 5. shared values
@pytest.mark.parametrize("charwise", [False, True])
def test_shared_values(charwise):
    if charwise:
        pats = synth.patterns_cfg5(400)
        hay = synth.zipf_text(48 * 4000)
    else:
        pats = synth.patterns_cfg2(300) + [b"ab", b"b", b"bab", b"abab"]
        hay = synth.wordsoup_haystack(64 << 10, synth.SEEDS["cfg2_dense"], pats, 13, noise_256=30, alphabet=b"ab")
    values = (np.arange(len(pats)) * 2654435761 % 7).astype(np.uint32)
    o = (orc.OracleCharwisePma if charwise else orc.OraclePma).build(pats, values=values)
    cls = da.CharwiseDoubleArrayAhoCorasick if charwise else da.DoubleArrayAhoCorasick
    p = cls.with_values(list(zip(pats, values.tolist())))
    assert p.serialize() == o.serialize()
    for api, mode in MODES:
        m = getattr(o, api)(hay)
        assert len(m) > 1000
        want = np.bincount(m["value"].astype(np.int64), minlength=7)
        pc = p.pattern_counts(mode, hay)
        by_value = np.zeros(7, dtype=np.uint64)
        np.add.at(by_value, pc["value"], pc["count"])
        assert by_value.tolist() == want.tolist(), api
        # ... and per (value, length), which the tuples carry too
        kw = np.unique(_keys(m["value"], m["end"] - m["start"]), return_counts=True)
        kg = _keys(pc["value"], pc["length"])
        got = {int(k): int(pc["count"][kg == k].sum()) for k in np.unique(kg)}
        assert {k: v for k, v in got.items() if v} == dict(zip(kw[0].tolist(), kw[1].tolist())), api


# ------------------------------------------------------------------------ 6. a real dictionary against independent kernels
def _check_large(o, p, dev, text_name, engines, api_mode=MODES):
    host_1m = dev[:1 << 20].cpu().numpy()
    for api, mode in api_mode:
        count, checksum = p.scan_count(mode, dev)
        assert count > len(dev) // 256, text_name
        assert p.count(mode, dev) == count
        want_1m = _want(o, api, host_1m)
        for eng in engines:
            for bins in (None, 0):
                p.set_option("hist_lds_bins", bins)
                got = p.histogram(mode, dev, engine=eng)
                assert da.last_kernel().startswith("hist "), da.last_kernel()
                assert bins is None or da.last_kernel().endswith("lds_bins=0"), da.last_kernel()
                assert int(got.sum()) == count, (text_name, api, eng, bins)
                assert _s1(p, got) == checksum >> 32, (text_name, api, eng, bins)
                assert p.histogram(mode, dev[:1 << 20], engine=eng).tolist() == want_1m.tolist(), (text_name, api, eng, bins)
        p.set_option("hist_lds_bins")


def test_cfg3_64mib():
    pats = synth.patterns_cfg3()
    o, p = _pair(pats)
    dev = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    synth.device_uniform(dev, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
    _check_large(o, p, dev, "uniform", (Engine.Tiered, Engine.DArray))
    assert p.count(ScanMode.FindOverlapping, dev) > 0 and da.last_engine() == int(Engine.Gram)   # the count the sums were held against: GRAM's
    synth.device_wordsoup(dev, synth.SEEDS["cfg3_dense"], pats, 20)
    _check_large(o, p, dev, "word soup", (Engine.Auto, Engine.DArray))


def test_cfg5_charwise_16mib():
    pats = synth.patterns_cfg5()
    o, p = _pair(pats, charwise=True)
    n = (16 << 20) - (16 << 20) % synth.CFG5_SLOT
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_zipf_text(dev)
    _check_large(o, p, dev, "zipf", (Engine.Auto,))


# ------------------------------------------------------------ ranges that take several launches, host haystacks in several windows
def test_more_than_one_launch_and_window():
    """a device haystack of 2^32 + 4 KiB bytes goes as three launches (positions past 2^32 included), a host haystack of 257 MiB as two
    staged windows: sums against the independent count / checksum kernels, and the host form against the device form.  The cuts are
    constants of the driver (2^31 bytes per launch, 256 MiB per window), so these are the smallest sizes that cross them; the text is
    generated on the device and the whole test took 0.14 s on an MI355X (4.3 GB of device memory, 257 MiB on the host)."""
    pats = synth.patterns_cfg3(2000)
    o, p = _pair(pats)
    n = (1 << 32) + 4096
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.device_wordsoup(dev, synth.SEEDS["cfg3_dense"], pats, 20)
    count, checksum = p.scan_count(ScanMode.FindOverlapping, dev)
    got = p.histogram(ScanMode.FindOverlapping, dev)
    assert int(got.sum()) == count and _s1(p, got) == checksum >> 32
    tail = p.histogram(ScanMode.FindOverlapping, dev, begin=n - 70000)
    assert tail.tolist() == _want(o, "find_overlapping_iter", dev[n - 70100:].cpu().numpy(), begin=100).tolist()
    m = (257 << 20) + 13
    part = dev[3:3 + m]
    host = part.cpu().numpy()
    for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
        assert p.histogram(mode, host).tolist() == p.histogram(mode, part).tolist()
