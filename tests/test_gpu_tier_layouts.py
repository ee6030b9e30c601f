"""The TIERED engine on the MI355X under every tier layout TierEngine::step has a route for (tests/tier_layouts.py; that each layout
exists is proved on the CPU by tests/test_tier_layouts_host.py): 16-bit and 32-bit dense rows, tier-B misses and hits, tier-C records,
the LDS block's offsets as upload_layout.hpp (tiered) computes them, and the histogram's LDS bins behind table blocks of other sizes.

Expected values come from the CPU oracle, never from the library: tuples are compared exactly (start, end, value, order), counts,
checksums and per-slot histogram counts exactly.  Every call names Engine.Tiered and is followed by an assertion that TIERED served it,
and every handle's info() is held against the layout it was built for: a handle that fell back to other tables fails, it does not pass
on another route."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap, ScanMode

import tier_layouts as tl

MODES = (("find_overlapping_iter", ScanMode.FindOverlapping), ("find_overlapping_no_suffix_iter", ScanMode.FindOverlappingNoSuffix))
T = Engine.Tiered
HIST_BINS_DEFAULT = 16384
LDS_LIMIT = 160 * 1024


def _served_by_tiered(what=None):
    assert da.last_engine() == int(T), (what, da.last_engine(), da.last_kernel())


def _same(got, want):
    return len(got) == len(want) and np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]) and \
        np.array_equal(got["value"], want["value"])


def _pad16(x):
    return (x + 15) & ~15


def _table_bytes(shape, C):
    """the LDS block as upload_layout.hpp (tiered) lays it out: rows, tier B's bitmaps and fail links, the dense states' sums, the byte classes"""
    return _pad16(shape["NA"] * C * (4 if shape["row32"] else 2)) + 2 * _pad16((shape["NB"] - shape["NA"]) * 4) + _pad16(shape["NA"] * 8) + 256


def _handle(blob, opts):
    p, rest = da.DoubleArrayAhoCorasick.deserialize(blob)
    assert rest == b""
    for k, v in opts.items():
        p.set_option(k, v)   # before the first upload
    return p


def _check_shape(p, opts, shape, C, what):
    """the handle's tables have the intended shape (a condition of every test below, asserted after the first scan)"""
    i = p.info()
    budget = opts.get("lds_budget", tl.DEFAULT_BUDGET)
    if isinstance(what, str):   # the W layouts, by name
        print(f"{what}: N={i.num_states} NA={i.tier_dense_states} NB={i.tier_lds_states} row32={shape['row32']} "
              f"tier_lds_bytes={i.tier_lds_bytes} (lds_budget {budget})")
    assert i.tiered_available == 1, what
    assert (i.num_states, i.num_classes, i.tier_dense_states, i.tier_lds_states) == (shape["N"], C, shape["NA"], shape["NB"]), what
    assert i.tier_lds_bytes <= budget, (what, i.tier_lds_bytes)
    assert i.tier_lds_bytes == _table_bytes(shape, C), (what, i.tier_lds_bytes)   # 16-bit and 32-bit rows give different blocks


class _Ref:
    """the oracle's answers for one dictionary, each computed once and left unchanged"""

    def __init__(self, patterns):
        self.o = orc.OraclePma.build(patterns)
        self.blob = self.o.serialize()
        self.outputs = self.o.outputs()
        assert len(self.outputs) == len(patterns)
        self.cache = {}

    def want(self, api, key, hay):
        """-> (tuples, checksum, matches per slot) of `hay`; `key` names it"""
        if (api, key) not in self.cache:
            m = getattr(self.o, api)(hay)
            m.setflags(write=False)
            self.cache[(api, key)] = (m, orc.matches_checksum(m), tl.slot_counts(self.outputs, m))
        return self.cache[(api, key)]


def _set_bins(p, bins):
    if bins is None:
        p.set_option("hist_lds_bins")   # the default
    else:
        p.set_option("hist_lds_bins", bins)


def _check_scans(p, ref, key, hay, arg, what):
    """scan, scan_count and count of one haystack, both modes; `arg` is `hay` as the call takes it (host bytes or a device tensor)"""
    for api, mode in MODES:
        want, checksum, _ = ref.want(api, key, hay)
        got = p.scan(mode, arg, engine=T)
        _served_by_tiered(what)
        assert _same(got, want), (what, api, len(got), len(want))
        assert p.scan_count(mode, arg, engine=T) == (len(want), checksum), (what, api)
        _served_by_tiered(what)
        assert p.count(mode, arg, engine=T) == len(want), (what, api)
        _served_by_tiered(what)


def _check_hist(p, ref, key, hay, arg, what, table_bytes=None):
    """histogram of one haystack, both modes, without LDS bins and with the default number of them (behind this layout's tables)"""
    for api, mode in MODES:
        _, _, slots = ref.want(api, key, hay)
        for bins in (0, None):
            _set_bins(p, bins)
            got = p.histogram(mode, arg, engine=T)
            _served_by_tiered(what)
            assert got.dtype == np.uint64 and np.array_equal(got, slots), (what, api, bins)
            if table_bytes is not None:   # the bins lie behind the table block: as many as the option asks for and 160 KiB leave
                room = (LDS_LIMIT - _pad16(max(table_bytes, 1024))) // 4
                lds_bins = 0 if bins == 0 else min(HIST_BINS_DEFAULT, len(slots), room)
                assert da.last_kernel() == f"hist eng=tier lds_bins={lds_bins}", (what, da.last_kernel())
    _set_bins(p, None)


def _device_batch(docs, lead):
    """(uint8 CUDA tensor, int64 CUDA offsets); `lead` bytes of other text in front: offsets[0] = lead, the documents' 16-byte phase moves"""
    blobs = [bytes(d) for d in docs]
    off = np.zeros(len(blobs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    off += lead
    hay = np.frombuffer(b"a" * lead + b"".join(blobs) + b"\0", dtype=np.uint8)[:max(int(off[-1]), 1)].copy()
    return torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()


def _check_batches(p, ref, keyed_docs, what, device_lead=5):
    """count_batch, scan_count_batch, scan_batch and histogram_batch, both modes, documents from the host and on the device; the handle's
    batch_piece is small: a document is scanned as several pieces"""
    docs = [d for _, d in keyed_docs]
    for api, mode in MODES:
        wants = [ref.want(api, k, d) for k, d in keyed_docs]
        counts = [len(w[0]) for w in wants]
        for batch in (docs, _device_batch(docs, device_lead)):
            c = p.count_batch(mode, batch, engine=T)
            _served_by_tiered(what)
            assert c.tolist() == counts, (what, api)
            c, s = p.scan_count_batch(mode, batch, engine=T)
            _served_by_tiered(what)
            assert c.tolist() == counts and s.tolist() == [w[1] for w in wants], (what, api)
            got, offs = p.scan_batch(mode, batch, engine=T)
            _served_by_tiered(what)
            assert offs.tolist() == [0] + np.cumsum(counts).tolist(), (what, api)
            for i, w in enumerate(wants):
                assert _same(got[int(offs[i]):int(offs[i + 1])], w[0]), (what, api, i)
            rows, roffs = p.histogram_batch(mode, batch, engine=T)
            _served_by_tiered(what)
            assert rows.dtype == da.SLOT_COUNT_DTYPE and len(roffs) == len(docs) + 1
            for i, w in enumerate(wants):
                nz = np.nonzero(w[2])[0]
                r = rows[int(roffs[i]):int(roffs[i + 1])]
                assert r["slot"].tolist() == nz.tolist() and r["count"].tolist() == w[2][nz].tolist(), (what, api, i)


def _check_iter(p, ref, key, hay, what):
    """the lazy iterators, window by window (the handle's iter_window is small, its emit option 0)"""
    for api, _ in MODES:
        want = ref.want(api, key, hay)[0]
        it = getattr(p, api)(hay, engine=T)
        parts = []
        while True:
            b = it.next_batch()
            if b is None:
                break
            _served_by_tiered(what)
            parts.append(b.copy())
        it.close()
        got = np.concatenate(parts) if parts else np.zeros(0, dtype=da.MATCH16_DTYPE)
        assert len(got) == len(want) and np.array_equal(got["end"], want["end"]) and np.array_equal(got["value"], want["value"]) and \
            np.array_equal(got["end"] - got["length"].astype(np.uint64), want["start"]), (what, api, len(got), len(want))


# ----------------------------------------------------------------------------------------------------------------- the W dictionaries
@pytest.fixture(scope="module")
def w_refs():
    return {name: _Ref(tl.w_patterns(name)) for name in ("W", "W_lo", "W_hi")}


@pytest.fixture(scope="module")
def w_texts():
    return tl.w_texts()


@pytest.fixture(scope="module")
def w_handles(w_refs, w_texts):
    """one handle per layout, built at its first use and kept for the module; the first scan uploads it and its shape is asserted"""
    made = {}

    def get(layout):
        if layout not in made:
            _, dname, opts, shape = next(l for l in tl.W_LAYOUTS if l[0] == layout)
            ref = w_refs[dname]
            p = _handle(ref.blob, opts)
            p.set_option("batch_piece", 64).set_option("emit", 0).set_option("iter_window", 4096)
            _check_scans(p, ref, "len17", w_texts["len17"], w_texts["len17"].tobytes(), layout)
            _check_shape(p, opts, shape, 32, layout)
            made[layout] = (p, ref, shape)
        return made[layout]
    return get


W_NAMES = [l[0] for l in tl.W_SCANNED]


def test_w_texts_reach_the_ends_of_the_deepest_level(w_refs, w_texts):
    """a condition on the input: the words that end in the lowest and in the highest depth-4 state are found, in every dictionary; and
    a run of `a` reports the chain aaaa -> aaa -> aa -> a at every position from the fourth on"""
    lo, hi = tl.extreme_words()
    for name, ref in w_refs.items():
        pats = tl.w_patterns(name)
        m = ref.want("find_overlapping_iter", "words", w_texts["words"])[0]
        seen = set(m["value"].tolist())
        assert pats.index(lo) in seen and pats.index(hi) in seen, name
        run = ref.want("find_overlapping_iter", "run_a", w_texts["run_a"])[0]
        n = len(w_texts["run_a"])
        assert len(run) == 4 * n - 6 and [pats[v] for v in run["value"][-4:].tolist()] == [b"aaaa", b"aaa", b"aa", b"a"], name
        heads = ref.want("find_overlapping_no_suffix_iter", "run_a", w_texts["run_a"])[0]
        assert len(heads) == n


@pytest.mark.parametrize("layout", W_NAMES)
def test_w_scans(w_handles, w_texts, layout):
    """tuples, count + checksum and count of every text, cut into 16-byte segments and into the default ones; host bytes, and a device
    tensor that begins 0, 1 and 5 bytes behind a 16-byte boundary"""
    p, ref, _ = w_handles(layout)
    for seg in (16, 0):
        p.set_option("seg_bytes", seg)
        for key, hay in w_texts.items():
            _check_scans(p, ref, key, hay, hay.tobytes(), (layout, key, seg))
    p.set_option("seg_bytes", 16)
    base = torch.from_numpy(np.concatenate([np.zeros(16, dtype=np.uint8), w_texts["words"]])).cuda()
    assert base.data_ptr() % 16 == 0
    for off in (0, 1, 5):
        for n in (17, 9001):
            hay = w_texts["words"][off:off + n]
            dev = base[16 + off:16 + off + n]
            assert dev.data_ptr() % 16 == off
            _check_scans(p, ref, ("words", off, n), hay, dev, (layout, "device", off, n))
            _check_hist(p, ref, ("words", off, n), hay, dev, (layout, "device", off, n))
    p.set_option("seg_bytes", 0)


@pytest.mark.parametrize("layout", W_NAMES)
def test_w_histograms(w_handles, w_texts, layout):
    """per-slot counts; the LDS bins begin behind this layout's table block (next to 160 KiB only a few hundred of them are left)"""
    p, ref, shape = w_handles(layout)
    for seg in (16, 0):
        p.set_option("seg_bytes", seg)
        for key, hay in w_texts.items():
            _check_hist(p, ref, key, hay, hay.tobytes(), (layout, key, seg), table_bytes=_table_bytes(shape, 32))
    p.set_option("seg_bytes", 0)


def _w_docs(w_texts):
    words, uniform = w_texts["words"], w_texts["uniform"]
    lo, hi = tl.extreme_words()
    docs = [("len0", words[:0]), ("len1", words[:1]), ("len3", words[:3]), ("len17", words[:17]), (("words", 1, 64), words[1:65]),
            (("uniform", 0, 65), uniform[:65]), (("words", 7, 300), words[7:307]), ("run_a", w_texts["run_a"]), ("len0", words[:0]),
            (("words", 4096, 5000), words[4096:9096]), (("uniform", 11, 7001), uniform[11:7012]),
            ("extremes", np.frombuffer(hi + lo + hi, dtype=np.uint8))]
    return docs


@pytest.mark.parametrize("layout", W_NAMES)
def test_w_batches(w_handles, w_texts, layout):
    p, ref, _ = w_handles(layout)
    _check_batches(p, ref, _w_docs(w_texts), layout)


@pytest.mark.parametrize("layout", W_NAMES)
def test_w_iterators(w_handles, w_texts, layout):
    p, ref, _ = w_handles(layout)
    for key in ("words", "uniform", "len3", "len0"):
        _check_iter(p, ref, key, w_texts[key], (layout, key))
    dev = torch.from_numpy(w_texts["words"][:9001].copy()).cuda()
    _check_iter(p, ref, ("words", 0, 9001), dev, (layout, "device"))


def test_w_unigram_lattice(w_handles, w_texts):
    """tokenize_unigram_batch over words cut from the W text, its lattice scanned by TIERED under the three-tier default layout, against
    tests/test_gpu_tokenize_unigram.py's float32 restatement of the definition"""
    import test_gpu_tokenize_unigram as tu
    p, ref, shape = w_handles("default")
    assert shape["NA"] < shape["NB"] < shape["N"]
    rng = np.random.default_rng(77)
    words = w_texts["words"]
    lo, hi = tl.extreme_words()
    docs, at = [hi + lo, b""], 0
    while at < 3000:
        n = int(rng.integers(1, 41))
        docs.append(words[at:at + n].tobytes())
        at += n
    scores = -rng.integers(1, 64, size=len(ref.outputs)).astype(np.float32) / np.float32(8.0)
    for front in (0, 5):
        tu._check_batch(ref.o, p, docs, scores, -20.0, gaps=(Gap.Bytes,), front=front, engines=(T,), what=("W", front))
        _served_by_tiered(front)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_rows_that_do_not_fit_are_declined(w_refs, w_texts):
    """dense_depth 3 under the default budget: W's rows alone are 139 264 bytes.  The handle has no TIERED tables, Engine.Tiered answers
    status 6 in every call, Engine.Auto is exact on other tables"""
    _, dname, opts, shape = next(l for l in tl.W_LAYOUTS if l[0] == "declined")
    assert shape is None
    ref = w_refs[dname]
    p = _handle(ref.blob, opts)
    p.upload()
    assert p.info().tiered_available == 0
    hay = w_texts["words"][:9001]
    raw = hay.tobytes()
    for api, mode in MODES:
        calls = (lambda: p.scan(mode, raw, engine=T), lambda: p.scan_count(mode, raw, engine=T), lambda: p.count(mode, raw, engine=T),
                 lambda: p.histogram(mode, raw, engine=T), lambda: p.count_batch(mode, [raw, b"ab"], engine=T),
                 lambda: p.scan_count_batch(mode, [raw, b"ab"], engine=T), lambda: p.scan_batch(mode, [raw, b"ab"], engine=T),
                 lambda: p.histogram_batch(mode, [raw, b"ab"], engine=T), lambda: getattr(p, api)(raw, engine=T).next_batch())
        for k, call in enumerate(calls):
            with pytest.raises(da.DaachorseError) as ei:
                call()
            assert ei.value.code == 6, (api, k, str(ei.value))
        want, checksum, slots = ref.want(api, ("words", 0, 9001), hay)
        assert _same(p.scan(mode, raw), want) and da.last_engine() != int(T), api
        assert p.scan_count(mode, raw) == (len(want), checksum) and da.last_engine() != int(T), api
        assert p.count(mode, raw) == len(want), api
        assert np.array_equal(p.histogram(mode, raw), slots) and da.last_engine() != int(T), api


def test_layout_options_after_the_first_upload(w_handles, w_texts):
    """lds_budget, dense_depth and rows_share_pct are read when the tables are laid out: on a handle that has tables they answer status 6
    and change nothing"""
    p, ref, shape = w_handles("root_b5")
    before = p.info()
    for name, value in (("lds_budget", tl.DEFAULT_BUDGET), ("dense_depth", 2), ("rows_share_pct", 100), ("lds_budget", None)):
        with pytest.raises(da.DaachorseError) as ei:
            p.set_option(name, value)
        assert ei.value.code == 6, name
    after = p.info()
    for f in ("tiered_available", "tier_dense_states", "tier_lds_states", "tier_lds_bytes", "num_classes"):
        assert getattr(after, f) == getattr(before, f), f
    assert after.tier_lds_states == shape["NB"] == 6
    _check_scans(p, ref, "uniform", w_texts["uniform"], w_texts["uniform"].tobytes(), "root_b5 after the refusals")


# --------------------------------------------------------------------------------------------------------------- tiny dictionaries
@pytest.mark.parametrize("layout", tl.TINY_LAYOUTS)
def test_tiny_dictionaries(layout):
    """60 seeded pattern sets over {a, b, c} with "" and duplicates among them, as test_fuzz_small_alphabets draws them, each with a
    budget that leaves ROOT's row (or the rows of depth 1) and none, half or all of the other states in tier B: ROOT's own list,
    no-suffix heads, 16-byte segments and batch pieces on tier-B and tier-C states"""
    tiers = set()
    for it, (pats, hay, opts, shape) in enumerate(tl.tiny_cases(layout)):
        ref = _Ref(pats)
        p = _handle(ref.blob, opts)
        p.set_option("batch_piece", 64).set_option("emit", 0).set_option("iter_window", 4096).set_option("seg_bytes", (16, 0)[(it // 2) % 2])
        what = (layout, it, pats, opts)
        raw = hay.tobytes()
        dev = torch.from_numpy(np.concatenate([np.zeros(16 + it % 7, dtype=np.uint8), hay])).cuda()[16 + it % 7:]
        arg = dev if it % 3 == 0 and len(hay) else raw
        _check_scans(p, ref, "hay", hay, arg, what)
        _check_shape(p, opts, shape, tl.trie_shape(pats)[2], what)
        _check_hist(p, ref, "hay", hay, arg, what, table_bytes=_table_bytes(shape, tl.trie_shape(pats)[2]))
        cut = len(hay) // 3
        docs = [("hay", hay), ("empty", hay[:0]), ("head", hay[:cut]), ("tail", hay[cut:]), ("one", hay[:1])]
        _check_batches(p, ref, docs, what, device_lead=it % 17)
        _check_iter(p, ref, "hay", hay, what)
        tiers.add((shape["NA"] < shape["NB"], shape["NB"] < shape["N"]))
    want = {"root_c": (False, True), "root_half": (True, True), "root_all": (True, False), "depth1_half": (True, True)}[layout]
    assert want in tiers, (layout, tiers)
