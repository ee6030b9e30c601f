"""Every scan path on dictionaries at the limits of the fields the kernels pack (daachorse_amd/synth.py's limit families), against the CPU
oracle built with the same values (tests/test_dictionary_limits_host.py checks the oracle on these families against a brute force).

  - values over the whole u32 range (0, 1, 2^31 - 1, 2^31, 2^32 - 2, 2^32 - 1, never the pattern index): a kernel that reports an output
    slot or the index, keeps 24 bits of the value or sign-extends bit 31 into the checksum fails here
  - patterns at the lengths where a field changes width (K, K + 1, K + 16, K + 17, 19, 20, 31 .. 33, 63 .. 65, 255, 256, 1023 .. 1025,
    4097, 65 537, 2^22 - 1, 2^22), planted across region / segment / window / piece cuts
  - one pattern registered 2, 255, 256 and 257 times (the emitter keeps a state's further copies in 8 bits) and a short one twice
  - charwise automata with 65 535, 65 536 and 2^24 outputs (the walker records' three output_pos layouts)

Each case runs every entry point that takes the dictionary — count, scan_count, scan, scan_device in both formats, the lazy iterator plain
and compact, both steppers through feed and feed_compact, the three batch calls and scan_count_multi over shards with a halo of
max_pattern_len - 1 — for all four iterators and both leftmost kinds, and asserts that the kernel it targets ran.  Tuples must equal the
oracle's, order included; counts and checksums must equal the oracle's matches_checksum.  The only refusal allowed is status 6.
Wall time of the file on one MI355X: about 3 minutes (174 s when it was added; the longest cases are the DARRAY sweep of the long
patterns and the two 2^22 emitter gates, 20 - 50 s each)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

APIS = {orc.STANDARD: [("find_overlapping_iter", ScanMode.FindOverlapping), ("find_overlapping_no_suffix_iter", ScanMode.FindOverlappingNoSuffix),
                       ("find_iter", ScanMode.Find)],
        orc.LEFTMOST_LONGEST: [("leftmost_find_iter", ScanMode.LeftmostFind)],
        orc.LEFTMOST_FIRST: [("leftmost_find_iter", ScanMode.LeftmostFind)]}
STEPPERS = {ScanMode.Find: ("find_stepper", "find_stepper"), ScanMode.FindOverlapping: ("find_overlapping_stepper", "find_overlapping_stepper")}
KINDS = (orc.STANDARD, orc.LEFTMOST_LONGEST, orc.LEFTMOST_FIRST)
REQ = {ScanMode.FindOverlapping: 2, ScanMode.Find: 3, ScanMode.LeftmostFind: 4, ScanMode.FindOverlappingNoSuffix: 5}   # daac_request of the tuples
K_EMIT, K_SEGMENT, K_MICRO, K_CHAIN, K_SELECT = 4, 6, 7, 8, 9   # daac_kernel_family
WALKERS = (int(Engine.Tiered), int(Engine.DArray))


def _tuples_fall_back(info, req, what):
    """a declined gate: the plan names the segment scanners / chain walkers on TIERED or DARRAY for the request, and the engine that
    then served it (read by the caller) is that one"""
    assert info.plan_kernel[req] in (K_SEGMENT, K_MICRO, K_CHAIN) and info.plan_engine[req] in WALKERS, \
        (what, list(info.plan_engine), list(info.plan_kernel), list(info.plan_reason))
    return info.plan_engine[req]


class Refused(Exception):
    pass


def _call(fn, *a, refuse=False, **k):
    """fn(*a, **k); a DaachorseError must be status 6 (and is allowed only where `refuse`)"""
    try:
        return fn(*a, **k)
    except da.DaachorseError as e:
        assert e.code == 6, str(e)
        if not refuse:
            raise
        raise Refused(str(e))


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in ("start", "end", "value"):
        if not np.array_equal(np.asarray(got[f]).astype(np.uint64), want[f].astype(np.uint64)):
            bad = int(np.nonzero(np.asarray(got[f]).astype(np.uint64) != want[f].astype(np.uint64))[0][0])
            raise AssertionError((what, f, bad, got[bad], want[bad]))


def _from16(t16):
    out = np.zeros(len(t16), dtype=da.MATCH_DTYPE)
    out["end"] = t16["end"]
    out["start"] = t16["end"] - t16["length"].astype(np.uint64)
    out["value"] = t16["value"]
    return out


def _from8(runs):
    parts = [np.zeros(0, dtype=da.MATCH_DTYPE)] + [da.bytewise._Stepper.decode8(r, b, eb) for r, b, eb in runs]
    return np.concatenate(parts)


def _pair(pats, values, kind=orc.STANDARD, charwise=False, opts=()):
    O = orc.OracleCharwisePma if charwise else orc.OraclePma
    P = da.CharwiseDoubleArrayAhoCorasick if charwise else da.DoubleArrayAhoCorasick
    o = O.build(pats, values=values, kind=kind)
    p, rest = P.deserialize(o.serialize())
    assert rest == b""
    for k, v in dict(opts).items():
        p.set_option(k, v)
    return o, p.upload()


def _plan(info):
    return list(info.plan_engine)[:6], list(info.plan_kernel)[:6], list(info.plan_reason)[:6]


def _same_plan_as_index_values(pats, info, kind=orc.STANDARD, charwise=False, opts=()):
    """values never change routing: the same dictionary with index values gets the same plan"""
    _, q = _pair(pats, None, kind, charwise, opts)
    assert _plan(q.info()) == _plan(info), (_plan(q.info()), _plan(info))


def _cuts(rng, n, extra=(), host=None):
    """seeded cuts plus `extra`; given `host` (charwise text), moved forward to character boundaries"""
    cs = {int(x) for x in list(rng.integers(0, n + 1, size=4)) + [c for c in extra if 0 <= c <= n]}
    if host is not None:
        cs = {next((d for d in range(c, n) if host[d] & 0xC0 != 0x80), n) for c in cs}
    return sorted(cs)


def sweep(o, p, host, kind, engine=Engine.Auto, refuse=False, rng=None, batch=True, lazy=True, stepper=True, multi=True, cuts=()):
    """every entry point on `host` for the iterators of `kind`, against the oracle; -> {mode: [entry points that answered],
    ("tuples", mode): the engine that served scan_device16}.
    `refuse`: a forced engine may decline a request (status 6 only); AUTO never may."""
    rng = np.random.default_rng(5) if rng is None else rng
    dev = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    chars = host if p.info().charwise else None
    # (charwise shards need max_pattern_len bytes in front, at least 3: a cut may fall inside the character before the shard)
    halo = max(3, int(p.info().max_pattern_len)) if chars is not None else max(0, int(p.info().max_pattern_len) - 1)
    served = {}
    for api, mode in APIS[kind]:
        want = getattr(o, api)(host)
        wcs = (len(want), orc.matches_checksum(want))
        ok = served.setdefault(mode, [])

        def step(name, fn, may_refuse=refuse):
            """a forced engine may refuse a request, and the 8-byte tuple forms a dictionary without end bits to spare: status 6, nothing else"""
            try:
                fn()
                ok.append(name)
            except Refused:
                pass
            except da.DaachorseError as e:   # (a lazy iterator can refuse at its first batch)
                assert e.code == 6 and may_refuse, (name, api, engine, str(e))
        step("count", lambda: _eq(_call(p.count, mode, dev, engine=engine, refuse=refuse), wcs[0], ("count", api, engine)))
        step("scan_count", lambda: _eq(_call(p.scan_count, mode, dev, engine=engine, refuse=refuse), wcs, ("scan_count", api, engine)))
        step("scan", lambda: _same(_call(p.scan, mode, dev, engine=engine, refuse=refuse), want, ("scan", api, engine)))

        def device(fmt16):
            dm = _call(p.scan_device, mode, dev, engine=engine, fmt16=fmt16, refuse=refuse)
            got = dm.to_numpy()
            dm.free()
            _same(_from16(got) if fmt16 else got, want, ("scan_device", fmt16, api, engine))
        step("scan_device24", lambda: device(False))
        step("scan_device16", lambda: device(True))
        served[("tuples", mode)] = da.last_engine()   # (an emitter that gives up hands the list to the segment scanners without an error)
        if lazy:
            def lazy_iter(compact):
                it = _call(getattr(p, api), dev, engine=engine, compact=compact, refuse=refuse or compact)
                runs = []
                while True:
                    r = it.next_batch8() if compact else it.next_batch()
                    if r is None:
                        break
                    runs.append((r[0].copy(), r[1], r[2]) if compact else r.copy())
                it.close()
                got = _from8(runs) if compact else _from16(np.concatenate([np.zeros(0, dtype=da.MATCH16_DTYPE)] + runs))
                _same(got, want, ("iterator", compact, api, engine))
            step("iter", lambda: lazy_iter(False))
            step("iter_compact", lambda: lazy_iter(True), True)
        if stepper and mode in STEPPERS:
            sname, oname = STEPPERS[mode]
            swant = getattr(o, oname)(host)
            raw = host.tobytes()
            cs = _cuts(rng, len(raw), cuts)

            def feed(compact):
                st = _call(getattr(p, sname), engine=engine, refuse=refuse)
                got, prev = [], 0
                for c in cs + [len(raw)]:
                    if compact:
                        r, b, eb = _call(st.feed_compact, raw[prev:c], refuse=True)
                        got.append(st.decode8(r, b, eb))
                    else:
                        got.append(np.array(_call(st.feed, raw[prev:c], refuse=refuse)))
                    prev = c
                _same(np.concatenate([np.zeros(0, dtype=da.MATCH_DTYPE)] + got), swant, ("stepper", compact, cs, api, engine))
            step("stepper", lambda: feed(False))
            step("stepper_compact", lambda: feed(True), True)
        if batch:
            cs = _cuts(rng, len(host), cuts, chars)
            docs = [host[a:b] for a, b in zip([0] + cs, cs + [len(host)])]
            dw = [getattr(o, api)(d) for d in docs]

            def batches():
                counts, sums = _call(p.scan_count_batch, mode, docs, engine=engine, refuse=refuse)
                assert counts.tolist() == [len(w) for w in dw], ("scan_count_batch", api, engine)
                assert sums.tolist() == [orc.matches_checksum(w) for w in dw], ("scan_count_batch checksum", api, engine)
                assert _call(p.count_batch, mode, docs, engine=engine, refuse=refuse).tolist() == counts.tolist()
                got, offs = _call(p.scan_batch, mode, docs, engine=engine, refuse=refuse)
                assert offs.tolist() == [0] + np.cumsum([len(w) for w in dw]).tolist()
                for i, w in enumerate(dw):
                    _same(got[int(offs[i]):int(offs[i + 1])], w, ("scan_batch", i, api, engine))
            step("batch", batches)
        if multi:
            cs = [c for c in _cuts(rng, len(host), cuts, chars) if 0 < c < len(host)]
            bounds = [0] + cs + [len(host)]
            shards = []
            for a, b in zip(bounds, bounds[1:]):
                h = min(halo, a)
                shards.append((0, dev[a - h:b], h, a))

            def multi_call():
                if mode not in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
                    with pytest.raises(da.DaachorseError) as ei:   # (the restart iterators are chains: no shards)
                        da.scan_count_multi(p, mode, shards, engine=engine)
                    assert ei.value.code == 6
                    raise Refused("restart iterator")
                _eq(_call(da.scan_count_multi, p, mode, shards, engine=engine, refuse=refuse), wcs, ("multi", api, engine, halo))
            step("multi", multi_call)
    return served


def _eq(got, want, what):
    assert got == want, (what, got, want)


def _all_kinds(pats, vals, host, charwise=False, opts=(), engine=Engine.Auto, refuse=False, **kw):
    out = {}
    for kind in KINDS:
        o, p = _pair(pats, vals, kind, charwise, opts)
        _same_plan_as_index_values(pats, p.info(), kind, charwise, opts)
        out[kind] = sweep(o, p, host, kind, engine=engine, refuse=refuse, **kw)
    return out


def _host(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------- values
@pytest.fixture(scope="module")
def values_case():
    pats, vals, text = synth.patterns_values(3000, text_bytes=1 << 19)
    return pats, vals, _host(text)


ENGINE_CASES = {
    # name: (options, engine, the kernel family daac_last_kernel() must name after the overlapping count and count + checksum)
    "auto": ({}, Engine.Auto, None),
    "tiered": ({}, Engine.Tiered, "tiered"),
    "darray": ({}, Engine.DArray, "darray"),
    "pfx": ({"pfx": 2}, Engine.Pfx, "pfx"),
    "gram_v1": ({"gram_version": 1}, Engine.Gram, "gram"),
    "gram_v2": ({"gram_version": 2}, Engine.Gram, "gram2"),
    "gram_v4": ({"gram_version": 4}, Engine.Gram, ("gram4", "gram2")),   # (gram4 counts; the checksum stays on gram2_kernels.hip)
    "emit0": ({"emit": 0}, Engine.Auto, None),
    "emit1": ({"emit": 1}, Engine.Auto, None),
    "find3_left3": ({"find3": 2, "left3": 2}, Engine.Auto, None),
}


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_full_range_values(values_case, case):
    """values over the whole u32 range through every engine: the emitter's {p, len | copy << 24, value} records (emit3_kernels.hip:157), the
    v1 / v2 / v3 value tables and the v3c rank blob (upload_layout.hpp, emitter and emitter_rank_tables), find3 / left3's match_hash32(value, len)
    tables (emitter_rank_tables), gram4's inline h, the TIERED / DARRAY output lists and the checksum's mix64(value << 32 | length)"""
    pats, vals, host = values_case
    opts, engine, kernel = ENGINE_CASES[case]
    forced = engine != Engine.Auto
    served = _all_kinds(pats, vals, host, opts=opts, engine=engine, refuse=forced)
    o, p = _pair(pats, vals, orc.STANDARD, opts=opts)
    info = p.info()
    assert info.gram2_available and info.gram_k and not info.gram_wide
    dev = torch.from_numpy(host).cuda()
    if kernel is not None:     # the forced engine served the overlapping count and checksum
        assert {"count", "scan_count"} <= set(served[orc.STANDARD][ScanMode.FindOverlapping]), served
        for call, k in zip((p.count, p.scan_count), (kernel, kernel) if isinstance(kernel, str) else kernel):
            call(ScanMode.FindOverlapping, dev, engine=engine)
            assert da.last_engine() == int(engine) and da.last_kernel().split()[0] == k, (case, da.last_kernel())
    else:
        for req, call in ((0, p.count), (1, p.scan_count)):
            call(ScanMode.FindOverlapping, dev)
            assert da.last_engine() == info.plan_engine[req], (case, req, da.last_kernel(), p.explain())
    if case == "auto":   # (short patterns: the 8-byte tuple forms have the end bits they need)
        for kind in KINDS:
            for mode, names in served[kind].items():
                if isinstance(mode, tuple):
                    continue
                assert {"iter_compact", "stepper_compact"} & set(names) or mode not in STEPPERS, (kind, mode, names)
                assert "iter_compact" in names, (kind, mode, names)
    if case in ("emit1", "auto"):
        assert info.plan_kernel[2] == K_EMIT and info.plan_engine[2] == int(Engine.Gram), p.explain()
        assert served[orc.STANDARD][("tuples", ScanMode.FindOverlapping)] == int(Engine.Gram), "the emitter gave the list up"
    if case == "emit0":
        assert info.plan_kernel[2] != K_EMIT, p.explain()
        assert served[orc.STANDARD][("tuples", ScanMode.FindOverlapping)] in WALKERS
    if case == "find3_left3":
        for kind, mode in ((orc.STANDARD, ScanMode.Find), (orc.LEFTMOST_LONGEST, ScanMode.LeftmostFind), (orc.LEFTMOST_FIRST, ScanMode.LeftmostFind)):
            o, q = _pair(pats, vals, kind, opts=opts)
            ms = o.find_iter(host) if mode == ScanMode.Find else o.leftmost_find_iter(host)
            assert q.scan_count(mode, dev) == (len(ms), orc.matches_checksum(ms))
            assert da.last_engine() == int(Engine.Gram) and q.info().plan_kernel[REQ[mode]] == K_SELECT, (kind, da.last_kernel(), q.explain())
            _same(q.scan(mode, dev), ms, ("select list", kind))


def test_full_range_values_wide():
    """the wide table set (31 .. 62 byte classes, gram2w_kernels.hip) with full-range values"""
    pats = synth.patterns_cfg3_wide(3000)
    vals = synth.full_range_values(len(pats))
    host = synth.wordsoup_haystack(1 << 19, synth.SEEDS["limits"], pats, 24, noise_256=40, alphabet=synth.ALPHA_WIDE)
    o, p = _pair(pats, vals)
    info = p.info()
    assert info.gram_wide, p.explain()
    dev = torch.from_numpy(host).cuda()
    want = o.find_overlapping_iter(host)
    assert p.scan_count(ScanMode.FindOverlapping, dev, engine=Engine.Gram) == (len(want), orc.matches_checksum(want))
    assert da.last_kernel().split()[0] == "gram2w", da.last_kernel()
    _all_kinds(pats, vals, host, lazy=False, stepper=False)


# ---------------------------------------------------------------------------------------------------------- count = (h32 != 0)
# The 8-byte hit record of a depth-(K+1) state carries no count: gram_kernels.hip and gram2_kernels.hip take count = (h32 != 0) there, and the
# table builders decline a K whose depth-(K+1) states break that.  tests/gram_exact.py has (length, value) pairs whose match_hash32 is 0.
# Which K each table set takes for each case, read once from info() on the device and from the layout on the CPU, with the builder's line:
#   (gram_available, gram_k, gram2_available, gram2_k)
ZERO_HASH_TABLES = {
    # a 2-byte word with h32 = 0 is a short pattern for K = 3: COMBO holds {count 1, sum 0} (gram.cpp:84), gram2's M word counts it in its
    # two count bits and its H entry adds 0 (gram2.cpp:124): nothing at depth 4 is irregular, both keep K = 3
    "z_short": (1, 3, 1, 3),
    # a 4-byte word with h32 = 0 is a depth-4 state with a count of 1 and a sum of 0: K = 3 declined (gram.cpp:66, gram2.cpp:105), both take K = 2
    "z_k3": (1, 2, 1, 2),
    # ... and a 3-byte one on top breaks K = 2 as well: no GRAM table set at all (gram.cpp:98 returns false; gram2.cpp likewise), PFX or the walkers serve
    "z_k2": (0, 0, 0, 0),
    # zero hashes at depth 7 and 8 are below depth K + 1: the walkers' records carry their own count (gram.cpp:119) and a tail record adds 1
    # whatever h is (gram_kernels.hip:193): K = 3 stays
    "z_deep": (1, 3, 1, 3),
    # one 4-byte word twice: a depth-4 state with count 2, K = 3 declined by both (gram.cpp:66, gram2.cpp:105)
    "dup_k": (1, 2, 1, 2),
    # four patterns ending at one 3-gram: v1's COMBO holds any count (K = 3); gram2's M word has two count bits (gram2.cpp:124: at most 3) and the
    # 3-byte word registered twice is an irregular depth-3 state for K = 2: no second table set
    "four_short": (1, 3, 0, 0),
}


@pytest.fixture(scope="module")
def zero_hash_cases():
    import gram_exact as ge
    out = {}
    for name, (pats, vals, special) in ge.zero_hash_cases().items():
        out[name] = (pats, vals, special, ge.special_text(pats, special))
    return out


@pytest.mark.parametrize("case", list(ENGINE_CASES))
@pytest.mark.parametrize("name", list(ZERO_HASH_TABLES))
def test_patterns_that_break_count_is_h_nonzero(zero_hash_cases, name, case):
    """k3s with a pattern whose hash is 0 (or two patterns at one state) where the hit record would have to carry a count, through every engine:
    every entry point gives the oracle's answer, a forced engine may refuse (status 6), AUTO may not; the table sets take the K written
    down above.  The text has each special word at its start, at its end, ending at offsets 1023 and 2047 and cut one byte short."""
    pats, vals, special, host = zero_hash_cases[name]
    opts, engine, kernel = ENGINE_CASES[case]
    forced = engine != Engine.Auto
    o, p = _pair(pats, vals, orc.STANDARD, opts=opts)
    info = p.info()
    assert (info.gram_available, info.gram_k, info.gram2_available, info.gram2_k) == ZERO_HASH_TABLES[name], (name, p.explain())
    served = sweep(o, p, host, orc.STANDARD, engine=engine, refuse=forced, cuts=[1023, 1024, 2047, 2048])
    names = set(served[ScanMode.FindOverlapping])
    if not forced:
        assert {"count", "scan_count", "scan", "scan_device24", "scan_device16", "batch", "multi"} <= names, (name, case, names)
    # the first special word at the very end, the last at the very start
    dev = torch.from_numpy(host).cuda()
    first, last = special[0], special[-1]
    for a, b in ((0, len(host)), (len(first) + 1, len(host)), (0, len(host) - len(last) - 1), (0, len(host) - 1)):
        want = o.find_overlapping_iter(host[a:b])
        # (each call on its own: a forced engine that refuses one of them, as the sweep found, must still answer the other)
        for call, answer in (("scan_count", (len(want), orc.matches_checksum(want))), ("count", len(want))):
            try:
                got = getattr(p, call)(ScanMode.FindOverlapping, dev[a:b], engine=engine)
            except da.DaachorseError as e:
                assert e.code == 6 and forced and call not in names, (name, case, call, str(e))
                continue
            assert got == answer and call in names, (name, case, call, a, b, got, answer)
    # the forced GRAM kernels ran on the K the builders took, or refused where there is no table set
    v1_k, v2_k = ZERO_HASH_TABLES[name][1], ZERO_HASH_TABLES[name][3]
    if case == "gram_v1":
        assert ("scan_count" in names) == (v1_k != 0), (name, names)
        if v1_k:
            p.scan_count(ScanMode.FindOverlapping, dev, engine=engine)
            assert da.last_kernel().split()[:2] == ["gram", f"K={v1_k}"], da.last_kernel()
    if case == "gram_v2":
        assert ("scan_count" in names) == (v2_k != 0), (name, names)
        if v2_k:
            p.scan_count(ScanMode.FindOverlapping, dev, engine=engine)
            assert da.last_kernel().split()[:2] == ["gram2", f"K={v2_k}"], da.last_kernel()


# ---------------------------------------------------------------------------------------------------------- lengths
def _k_of_words():
    """K of the table set the handle builds for the families' words (read from the handle, not assumed)"""
    words = synth.patterns_cfg3(400)
    _, p = _pair(words, None)
    return int(p.info().gram2_k)


@pytest.fixture(scope="module")
def lengths_case():
    K = _k_of_words()
    pats, vals, text = synth.patterns_lengths(K)
    return K, pats, vals, _host(text)


LENGTH_CUTS = [c for c in range(0, 1 << 20, 2048)]


@pytest.mark.parametrize("case", ["auto", "tiered", "darray", "pfx", "emit0", "gram_v4"])
def test_long_patterns(lengths_case, case):
    """patterns at every packing edge up to 65 537 bytes, nested with their prefixes and suffixes, planted across cuts: emit3's staged
    {position | length << 10} and 24-bit lengths (upload_layout.hpp, emitter: `fits`), gram2's patterns longer than K + 16 (gram2.hpp:61) and tail records
    (gram2.cpp:187), the compact iterator's / stepper's 32 - bits(max_len) end bits, and batches entering a piece min(halo, rel) bytes
    early with halos longer than a piece (batch_piece 256 and the default)"""
    K, pats, vals, host = lengths_case
    opts, engine, kernel = ENGINE_CASES[case]
    o, p = _pair(pats, vals, opts=opts)
    assert int(p.info().gram2_k) == K and int(p.info().max_pattern_len) == 65537
    for k, v in (("seg_bytes", 64), ("iter_window", 1 << 17)) if case == "darray" else ():
        da.set_option(k, v)
    try:
        served = _all_kinds(pats, vals, host, opts=opts, engine=engine, refuse=engine != Engine.Auto,
                            cuts=[2048 * 7 + 5, 65536 * 3 - 100, 256 * 41 + 1])
    finally:
        da.set_option("seg_bytes", 0)
        da.set_option("iter_window", 64 << 20)
    for kind in KINDS:   # 65 537 bytes leave 15 end bits: less than 4 x halo + 1 MiB, so both 8-byte tuple forms decline (api_iter.hip:317, :548)
        for mode, names in served[kind].items():
            if not isinstance(mode, tuple):
                assert "iter_compact" not in names and "stepper_compact" not in names, (kind, mode, names)
    if case == "auto":
        assert p.info().plan_kernel[2] == K_EMIT, p.explain()   # (the emitter takes patterns of up to 2^22 - 1 bytes)
        assert served[orc.STANDARD][("tuples", ScanMode.FindOverlapping)] == int(Engine.Gram), "the emitter gave the list up"
    if kernel is not None:
        p.count(ScanMode.FindOverlapping, torch.from_numpy(host).cuda(), engine=engine)
        assert da.last_kernel().split()[0] == (kernel if isinstance(kernel, str) else kernel[0]), da.last_kernel()


def test_compact_forms_on_long_patterns():
    """the compact iterator and stepper give 32 - bits(max_len) bits to the end position (api_iter.hip:317, :548): patterns of up to 1025
    bytes leave 21, enough for a window, so both 8-byte tuple forms serve every iterator of every kind with lengths 17 .. 1025 in the list"""
    K = _k_of_words()
    pats, vals, text = synth.patterns_lengths(K, max_len=1025)
    host = _host(text)
    assert max(len(w) for w in pats) == 1025
    da.set_option("iter_window", 1 << 17)
    try:
        served = _all_kinds(pats, vals, host, batch=False, multi=False, cuts=[2048 * 3 + 7, 4096 * 9 - 3])
    finally:
        da.set_option("iter_window", 64 << 20)
    for kind in KINDS:
        for mode, names in served[kind].items():
            if not isinstance(mode, tuple):
                assert "iter_compact" in names and ("stepper_compact" in names or mode not in STEPPERS), (kind, mode, names)


def test_long_patterns_batch_piece(lengths_case):
    """batch pieces of 256 bytes with a halo of 65 536: a piece entered min(halo, rel) bytes early (batch_kernels.hip)"""
    K, pats, vals, host = lengths_case
    docs = [host[:1000], host[1000:70000], host[70000:70256], host[70256:200001], host[200001:300000]]
    for kind in KINDS:
        o, p = _pair(pats, vals, kind, opts={"batch_piece": 256})
        sweep(o, p, host[:300000], kind, lazy=False, stepper=False, multi=False, cuts=[1000, 70000, 70256, 200001])
        if kind == orc.STANDARD:   # the overlapping modes went through the lane pieces (not the single-haystack path of long documents)
            p.count_batch(ScanMode.FindOverlapping, docs)
            lk = dict(kv.split("=") for kv in da.last_kernel().split()[1:])
            assert da.last_kernel().startswith("batch ") and int(lk["pieces"]) > len(docs) and int(lk["long_docs"]) == 0, da.last_kernel()


@pytest.mark.parametrize("max_len,served", [(19, True), (20, False)])
def test_find3_length_gate(max_len, served):
    """find3's tables exist only for max_len <= 19 (upload_layout.hpp, emitter_rank_tables); it stages {position | length << 11} and tests (r.y & 0xffffff) < 32
    (find3_kernels.hip:337): at 19 bytes find3 / left3 serve, at 20 they decline to the chain walkers, with the oracle's answer either way"""
    K = _k_of_words()
    pats, vals, text = synth.patterns_lengths(K, max_len=max_len)
    host = _host(text)
    dev = torch.from_numpy(host).cuda()
    opts = {"find3": 2, "left3": 2}
    for kind, mode in ((orc.STANDARD, ScanMode.Find), (orc.LEFTMOST_LONGEST, ScanMode.LeftmostFind), (orc.LEFTMOST_FIRST, ScanMode.LeftmostFind)):
        o, p = _pair(pats, vals, kind, opts=opts)
        _same_plan_as_index_values(pats, p.info(), kind, opts=opts)
        ms = o.find_iter(host) if mode == ScanMode.Find else o.leftmost_find_iter(host)
        assert p.scan_count(mode, dev) == (len(ms), orc.matches_checksum(ms))
        assert (da.last_engine() == int(Engine.Gram)) == served, (max_len, kind, da.last_kernel(), p.explain())
        assert (p.info().plan_kernel[REQ[mode]] == K_SELECT) == served, p.explain()
        if not served:   # find3 / left3 tables exist only for max_len <= 19: the chain walkers serve, and the plan says so
            assert da.last_engine() == _tuples_fall_back(p.info(), REQ[mode], ("find3 gate", max_len, kind))
        assert p.count(mode, dev) == len(ms)
        _same(p.scan(mode, dev), ms, ("select list", kind, max_len))
        dm = p.scan_device(mode, dev, fmt16=True)
        got = dm.to_numpy()
        dm.free()
        _same(_from16(got), ms, ("select list16", kind, max_len))


@pytest.mark.parametrize("L,emits", [((1 << 22) - 1, True), (1 << 22, False)])
def test_emitter_length_gate(L, emits):
    """emit3 keeps a staged tuple's length in 22 bits: gated off at max_len >= 2^22 (upload_layout.hpp, emitter: `fits`; PFX's emitter in pfx: pfx_emit_ok); one pattern of
    2^22 - 1 bytes goes through the emitter, one of 2^22 bytes to the fallback, and both give the oracle's tuples"""
    pats, vals, text = synth.patterns_single_long(L)
    host = _host(text)
    dev = torch.from_numpy(host).cuda()
    for opts, engine in (({}, Engine.Auto), ({"pfx": 2}, Engine.Pfx)):
        o, p = _pair(pats, vals, opts=opts)
        info = p.info()
        _same_plan_as_index_values(pats, info, opts=opts)
        want = o.find_overlapping_iter(host)
        assert len(want) == 1 and int(want[0]["value"]) == 0xFFFFFFFF
        if engine == Engine.Auto:
            assert (info.plan_kernel[2] == K_EMIT) == emits, (L, p.explain())
            fallback = None if emits else _tuples_fall_back(info, 2, ("emitter length gate", L))
        for fmt16 in (False, True):
            try:
                dm = p.scan_device(ScanMode.FindOverlapping, dev, engine=engine, fmt16=fmt16)
            except da.DaachorseError as e:
                assert e.code == 6 and engine == Engine.Pfx and not emits, str(e)
                continue
            got = dm.to_numpy()
            dm.free()
            _same(_from16(got) if fmt16 else got, want, (L, fmt16, engine))
            if engine == Engine.Auto:
                assert da.last_engine() == (int(Engine.Gram) if emits else fallback), (L, fmt16)
        assert p.scan_count(ScanMode.FindOverlapping, dev, engine=engine) == (1, orc.matches_checksum(want))
        _same(p.scan(ScanMode.FindOverlapping, dev), want, (L, "scan"))


# ---------------------------------------------------------------------------------------------------------- copies
@pytest.mark.parametrize("n_copies", [2, 16, 17, 255, 256, 257])
def test_copies(n_copies):
    """one long pattern registered n times with its own value per copy.  The emitter keeps a state's further copies in 8 bits (erec.w >> 24,
    gram2.cpp:271, up to 256 copies at gram2.cpp:236), but EXPAND places each further copy as an extra at the position where the pattern
    ends, counts a position's extras in 4 bits (emit3_kernels.hip:741) and takes 64 per tile (:719).  The upload gate on the copies
    (upload_layout.hpp, emitter: max_copies <= kEmit3MaxExtrasAtPosition) gives the emitter 16 copies and sends 17 and more to the segment scanners from
    the start; a pattern of <= K bytes registered twice goes there always.  Where the plan names the emitter it must really serve the list
    (daac_last_engine): with 2 copies on dense text, with 16 on text that holds the pattern once per 2 KiB (15 extras per tile).  Copies
    come out in registration order (the crate's per-end output order); find_iter / leftmost report the first copy."""
    K = _k_of_words()
    pats, vals, text = synth.patterns_copies(n_copies, K, spacing=None if n_copies == 2 else 2048)
    host = _host(text)
    long_w = max((w for w in set(pats) if len(w) > K + 1), key=pats.count)
    short = [w for w in set(pats) if len(w) == K and pats.count(w) == 2]
    assert len(short) == 1 and pats.count(long_w) == n_copies and len(long_w) > K + 1
    assert host.tobytes().count(long_w) >= 8
    # the long pattern's copies alone, and with the short duplicate as well (which the emitter never takes)
    no_short = [i for i, w in enumerate(pats) if w != short[0]]
    for sel, emits in ((no_short, n_copies - 1 <= 15), (list(range(len(pats))), False)):
        ps, vs = [pats[i] for i in sel], vals[sel]
        o, p = _pair(ps, vs)
        info = p.info()
        if emits:
            assert info.plan_kernel[2] == K_EMIT, (n_copies, p.explain())
        else:   # regression: the copies gate (upload_layout.hpp, emitter: max_copies <= kEmit3MaxExtrasAtPosition) / the short-duplicate gate (gram2.cpp:236)
            fallback = _tuples_fall_back(info, 2, ("copies gate", n_copies, len(sel)))
            assert info.plan_reason[2] == 5, list(info.plan_reason)   # DAAC_WHY_DUPLICATES
        served = _all_kinds(ps, vs, host, cuts=[4096, 20000])
        got = served[orc.STANDARD][("tuples", ScanMode.FindOverlapping)]
        assert got == (int(Engine.Gram) if emits else fallback), (n_copies, len(sel), got)
        for opts, engine in (({"pfx": 2}, Engine.Pfx), ({"gram_version": 4}, Engine.Gram), ({}, Engine.DArray)):
            o, p = _pair(ps, vs, opts=opts)
            names = sweep(o, p, host, orc.STANDARD, engine=engine, refuse=True, lazy=False, stepper=False, batch=False)[ScanMode.FindOverlapping]
            # (every forced engine serves the overlapping count; DARRAY serves everything)
            assert "count" in names and (engine != Engine.DArray or {"scan_count", "scan", "scan_device24", "scan_device16", "multi"} <= set(names)), \
                (engine, names)


# ---------------------------------------------------------------------------------------------------------- charwise
@pytest.mark.parametrize("n_outputs", [65535, 65536])
def test_charwise_output_layouts(n_outputs):
    """the charwise walker records keep output_pos in 16 bits + a 16-bit child filter below 65 536 outputs and 24 + 8 bits below 2^24
    (upload_layout.hpp, charwise: obits / fbits): 65 535 outputs is the last of the first layout, 65 536 the first of the second.  (Leftmost-first drops the
    patterns that can never match, a word with an earlier word as its prefix, so that kind stays a few outputs below the edge.)"""
    pats, vals, text = synth.patterns_charwise_outputs(n_outputs)
    host = _host(text)
    o, p = _pair(pats, vals, charwise=True)
    assert len(o.outputs()) == n_outputs and int(p.info().outputs_len) == n_outputs and p.info().charwise   # (every copy adds an output)
    _all_kinds(pats, vals, host, charwise=True, multi=True)


def test_charwise_output_layout_unfiltered():
    """2^24 outputs: the walker records carry no child filter (upload_layout.hpp, charwise: obits / fbits).  The dictionary (16 777 216 patterns, almost all copies of
    one the text holds once) takes about 15 s to generate and build on the host, so this case runs count and count + checksum of every
    iterator, and the overlapping tuples, only.  Standard and leftmost-longest reach 2^24 outputs; leftmost-first drops the patterns that
    can never match and stays in the 24-bit layout"""
    n = 1 << 24
    pats, vals, text = synth.patterns_charwise_outputs(n)
    host = _host(text)
    dev = torch.from_numpy(host).cuda()
    for kind in KINDS:
        o, p = _pair(pats, vals, kind, charwise=True)
        assert int(p.info().outputs_len) == len(o.outputs()) and (kind == orc.LEFTMOST_FIRST or len(o.outputs()) == n)
        for api, mode in APIS[kind]:
            want = getattr(o, api)(host)
            assert p.count(mode, dev) == len(want), (kind, api)
            assert p.scan_count(mode, dev) == (len(want), orc.matches_checksum(want)), (kind, api)
            if mode == ScanMode.FindOverlapping:
                assert len(want) > n
                _same(p.scan(mode, dev), want, ("scan", api))
        del o, p
