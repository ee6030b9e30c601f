"""The cases of tests/test_gpu_uninitialised.py and tests/test_uninit_ledger_host.py: every device entry point of include/daachorse_amd.h,
each with the C names it drives, a function that makes the call and returns its whole result in plain values, and the expected value —
from the CPU oracle or from the definitions the neighbouring suites already use (test_gpu_streams.py's case tables, gram_exact,
pack_golden, decode_golden, special_golden, wordpiece_golden, normalize_golden), never from the library.

Importing this module touches no device: handles, texts and expected values are made the first time a case asks for them (World)."""
import ctypes as C
import functools

import numpy as np

import decode_golden as dg
import gram_exact as ge
import normalize_golden as ng
import pack_golden as pg
import special_golden as sg
import test_gpu_streams as ts
import tier_layouts as tl
import wordpiece_golden as wg
from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import Engine, Gap, ScanMode, Split, _ffi, synth

OV, NOSUF, FIND, LEFT = ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix, ScanMode.Find, ScanMode.LeftmostFind
GRAM4_BASE = {"gram_version": 4, "gram_ppl": 32, "gram3_tail": -1, "gram4_filter": 1, "gram_region": 2048, "gram_region_small": 0, "gram_taper_split": -1,
              "threads": 1024, "blocks_per_cu": 1, "gram_slab": 4096}   # test_gpu_gram4_claims.py's BASE
SMALL = 1 << 16
# test_gpu_pfx.py's smallest any-alphabet dictionary whose tuples the PFX emitter serves, on a stretch of its text
PFX_PATS = [b"a", b"ab", b"abc", b"bc", b"c", b"abcabcabcabcabcabcabc", b"cabcabcabcabcabcabcabca", b"bcabcabcabcabcabcabcabcabcabc", b"\xff\x00", b"\x00\xff\x00\xff"]
PFX_TEXT = (b"abcabcabcabcabcabcabcabcabcabcab\xff\x00\xff\x00xx" + b"q" * 300 + b"abcab" * 9) * 10
BATCH_SIZES = (3, 64, 257)

# Entry points that hand out no device scratch, staging or result buffer of their own: they build, describe, configure or release things,
# or only move a finished result.  Everything else in the header must be driven by a case below (tests/test_uninit_ledger_host.py).
HOST_ONLY = {
    "daac_abi_version", "daac_last_error", "daac_free", "daac_last_engine", "daac_last_kernel",
    "daac_bytewise_from_serialized", "daac_bytewise_from_parts", "daac_bytewise_build", "daac_charwise_from_serialized", "daac_charwise_build",
    "daac_pma_serialize", "daac_pma_info", "daac_pma_explain", "daac_pma_free", "daac_pma_outputs",
    "daac_pma_upload", "daac_pma_trim",                       # the tables (DeviceTables::put: zero-padded by contract); the kept workspace released
    "daac_device_free", "daac_device_to_host",                # a finished result released or copied
    "daac_matches_count", "daac_matches_data", "daac_matches_free",
    "daac_splitter_create", "daac_splitter_free", "daac_normalizer_create", "daac_normalizer_free", "daac_normalizer_table_bytes",
    "daac_decoder_create", "daac_decoder_free",
    "daac_set_option", "daac_pma_set_option",
}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).cuda()


def _dev_text(host, shift=5):
    """the bytes in device memory, their first byte `shift` off a 16-byte boundary"""
    import torch
    host = np.frombuffer(bytes(host), dtype=np.uint8) if not isinstance(host, np.ndarray) else host
    buf = torch.zeros(16 + len(host) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(host)].copy_(torch.from_numpy(host.copy()))
    return buf[shift:shift + len(host)]


def _sev16(t):
    return list(zip((t["end"] - t["length"].astype(np.uint64)).tolist(), t["end"].tolist(), t["value"].tolist()))


def _free(dm):
    try:
        return dm.to_numpy()
    finally:
        dm.free()


# the run-time options the cases set on handles they share: every case takes them all away first, so that the route a case takes
# does not depend on the cases that ran before it
CASE_OPTIONS = sorted(set(GRAM4_BASE) | {"find3", "left3", "restart_chain", "select_emit", "find3_window", "overlap_micro", "hist_lds_bins", "iter_window",
                                        "emit_rec_per_kib"})


def _set(p, opts):
    """the case's options on a shared handle, every other option of CASE_OPTIONS at the process-wide value"""
    for k in CASE_OPTIONS:
        if k not in opts:
            p.set_option(k, None)
    for k, v in opts.items():
        p.set_option(k, v)


def _plain_streams_world(w):
    for p in (w.s.p, w.s.pl, w.s.cp, w.s.cpl, w.s.wp):
        _set(p, {})


def _batch_lens(n):
    """document lengths of a batch of n: an empty document in the middle and one at the end; 64: one beyond batch_lane_max (the long route)"""
    rng = np.random.default_rng(7000 + n)
    lens = [int(x) for x in rng.integers(1, {3: 60, 64: 120, 257: 40}[n], size=n)]
    lens[n // 2] = 0
    lens[-1] = 0
    if n == 64:
        lens[5] = 1203
        lens[40] = ts.LANE_MAX
    return lens


class World:
    """handles, texts and expected values, each made once on first use"""

    def __init__(self):
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    # ---- test_gpu_streams.py's world: ten short patterns, Standard and LeftmostLongest, bytewise and charwise, the token models
    @property
    def s(self):
        return self.once("streams", ts._World)

    @property
    def ncu(self):
        import torch
        return self.once("ncu", lambda: torch.cuda.get_device_properties(0).multi_processor_count)

    # ---- the lower-case dictionary of 5 000 words the GRAM engines, the emitter and find3 / left3 serve
    @property
    def cfg3(self):
        return self.once("cfg3", lambda: synth.patterns_cfg3(5000))

    def pair(self, key, patterns, kind=0, opts=None, charwise=False):
        def make():
            o, p = ts._pair(patterns, kind=kind, charwise=charwise)
            for k, v in (opts or {}).items():   # (set once, in front of the upload)
                p.set_option(k, v)
            return o, p
        return self.once(("pair", key), make)

    def gram(self, kind=0):
        """(oracle, handle), uploaded under the default options: a case's own options come after the tables are laid out"""
        def make():
            p, rest = da.DoubleArrayAhoCorasick.deserialize(self.gram_oracle(kind).serialize())
            assert rest == b""
            return p.upload()
        return self.gram_oracle(kind), self.once(("cfg3", kind), make)

    def gram_oracle(self, kind=0):
        return self.once(("cfg3 oracle", kind), lambda: orc.OraclePma.build(self.cfg3, kind=kind))

    def fresh_gram(self):
        """a new handle on the same dictionary: nothing uploaded, nothing remembered of earlier scans"""
        p, rest = da.DoubleArrayAhoCorasick.deserialize(self.gram_oracle().serialize())
        assert rest == b""
        return p

    def text(self, kind, n):
        def make():
            if kind == "uniform":
                return synth.uniform_haystack(n, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
            return synth.wordsoup_haystack(n, synth.SEEDS["cfg3_dense"], self.cfg3, 20)
        return self.once(("text", kind, n), make)

    def dev(self, kind, n, shift=5):
        return self.once(("dev", kind, n, shift), lambda: _dev_text(self.text(kind, n), shift))

    def tuples(self, kind, n, api="find_overlapping_iter", leftmost=False):
        return self.once(("tuples", kind, n, api), lambda: getattr(self.gram_oracle(1 if leftmost else 0), api)(self.text(kind, n)))



class Case:
    def __init__(self, name, entries, run, want):
        self.name, self.entries, self.run, self.want = name, tuple(entries), run, want


CASES = {}


def case(name, entries, run, want):
    assert name not in CASES, name
    for e in entries:
        assert e.startswith("daac_"), e
    CASES[name] = Case(name, entries, run, want)


# ====================================================================================================== 1. the count kernels
def _gram4_count(w, hay, opts, begin=0):
    p = w.gram()[1]
    _set(p, {**GRAM4_BASE, **opts})
    got = p.count(OV, hay, engine=Engine.Gram, begin=begin)
    assert da.last_engine() == int(Engine.Gram) and da.last_kernel().startswith("gram4"), da.last_kernel()
    return got


def _claimed_len(w):
    return (w.ncu * 8 + 1) * 2048   # threads = 512: 8 waves a workgroup, one workgroup per CU; one region more than the launch has waves


for _kind in ("uniform", "soup"):
    def _run(w, kind=_kind):
        n = _claimed_len(w)
        got = _gram4_count(w, w.dev(kind, n, shift=0), {"threads": 512, "gram_taper_split": 0})   # (lead 0: the regions are the text's)
        import re
        m = re.search(r" regions=(\d+) claims=(\d+) ", da.last_kernel())
        assert m and int(m.group(1)) == w.ncu * 8 + 1 and int(m.group(2)) >= 1, da.last_kernel()
        return got
    case(f"gram4-claimed-{_kind}", ["daac_scan_count_only_range"], _run,
         lambda w, kind=_kind: w.gram_oracle().overlapping_count(w.text(kind, _claimed_len(w)), threads=4)[0])

    def _run(w, kind=_kind):
        got = _gram4_count(w, w.dev(kind, SMALL), {})
        assert " claims=0 " in da.last_kernel(), da.last_kernel()
        return got
    case(f"gram4-unclaimed-{_kind}", ["daac_scan_count_only_range"], _run, lambda w, kind=_kind: len(w.tuples(kind, SMALL)))

case("gram4-empty", ["daac_scan_count_only_range"], lambda w: _gram4_count(w, w.dev("soup", SMALL)[:0], {}), lambda w: 0)
# a shard that begins inside the halo: the scan starts at 0, in front of `begin`, and what ends in (0, begin] is counted by a second launch
# (counters at claim + 8, a result word of its own) and subtracted
for _begin in (1, 5):
    case(f"gram4-shard-begin{_begin}", ["daac_scan_count_only_range"],
         lambda w, b=_begin: _gram4_count(w, w.dev("soup", SMALL), {}, begin=b),
         lambda w, b=_begin: int((w.tuples("soup", SMALL)["end"] > b).sum()))


def _gram_world(name):
    import test_gpu_gram_exact as tge
    return tge.world(name)


for _fam, _name in (("v1", "k3s"), ("v2", "k2s"), ("wide", "w40")):
    for _kind in ge.KINDS:
        def _run(w, fam=_fam, name=_name, kind=_kind):
            g = _gram_world(name)
            hay = g.text(kind, 5)
            call = {"v1": lambda c: g.v1(c, hay, 5, 0), "v2": lambda c: g.v2(c, hay, 5), "wide": lambda c: g.wide(c, hay, 5)}[fam]
            cnt, lk = call("count"), da.last_kernel()
            return [cnt, list(call("scan_count")), lk]   # (both labels are asserted whole by test_gpu_gram_exact.World)

        def _want(w, name=_name, kind=_kind):
            a = ge.dictionary(name).answer(kind)
            return [a[0], list(a)]
        case(f"gram-{_fam}-{_name}-{_kind}", ["daac_scan_count_only_range", "daac_scan_count_range"], _run, _want)


def _pfx(w):
    return w.pair("pfx", PFX_PATS, opts={"pfx": 2})


def _pfx_run(w):
    o, p = _pfx(w)
    t = w.once("pfx_dev", lambda: _dev_text(PFX_TEXT, 7))
    out = [p.count(OV, t, engine=Engine.Pfx), list(p.scan_count(OV, t, engine=Engine.Pfx)), ts._sev(p.scan(OV, t, engine=Engine.Pfx)),
           ts._sev(_free(p.scan_device(OV, t, engine=Engine.Pfx))), _sev16(_free(p.scan_device(OV, t, engine=Engine.Pfx, fmt16=True)))]
    assert da.last_engine() == int(Engine.Pfx)
    return out


def _pfx_want(w):
    m = _pfx(w)[0].find_overlapping_iter(PFX_TEXT)
    return [len(m), [len(m), orc.matches_checksum(m)], ts._sev(m), ts._sev(m), ts._sev(m)]


case("pfx-count-checksum-tuples", ["daac_scan_count_only_range", "daac_scan_count_range", "daac_scan", "daac_scan_device", "daac_scan_device16"], _pfx_run, _pfx_want)


def _scan_count_plain(w):
    """daac_scan_count itself (the Python wrappers call the _range forms)"""
    o, p = w.gram()
    _set(p, {})
    t = w.dev("uniform", SMALL)
    cnt, cs = C.c_uint64(), C.c_uint64()
    _ffi.check(_ffi.lib().daac_scan_count(p._h, int(OV), int(Engine.Auto), C.cast(t.data_ptr(), C.POINTER(C.c_uint8)), t.numel(), 1, None, C.byref(cnt), C.byref(cs), None))
    return [cnt.value, cs.value]


case("scan_count-plain", ["daac_scan_count"], _scan_count_plain,
     lambda w: [len(w.tuples("uniform", SMALL)), orc.matches_checksum(w.tuples("uniform", SMALL))])


# ================================================================================================== 2. the segment scanners
def _segment(handle, engine, opts=None):
    """count, count + checksum and tuples (the kernels' three modes) of the overlapping scan, with and without `heads` (no-suffix)"""
    def run(w):
        o, p, text, dev = handle(w, True)
        _set(p, opts or {})
        out = []
        for mode in (OV, NOSUF):
            out += [p.count(mode, dev, engine=engine), list(p.scan_count(mode, dev, engine=engine)), ts._sev(p.scan(mode, dev, engine=engine))]
            assert engine == Engine.Auto or da.last_engine() == int(engine), (da.last_engine(), engine)
        return out

    def want(w):
        o, p, text, dev = handle(w, False)
        out = []
        for api in ("find_overlapping_iter", "find_overlapping_no_suffix_iter"):
            m = getattr(o, api)(text)
            out += [len(m), [len(m), orc.matches_checksum(m)], ts._sev(m)]
        return out
    return run, want


def _rich_handle(w, dev):
    """(oracle, handle, text, the text in device memory where `dev` asks for it)"""
    text = w.once("rich8k", lambda: ts._text(np.random.default_rng(31), ts.SINGLE, ts.RICH))
    return w.s.o, w.s.p, text, w.once("rich8k_dev", lambda: _dev_text(text)) if dev else None


def _tier_handle(layout):
    def handle(w, dev):
        name, dictionary, opts, shape = next(l for l in tl.W_LAYOUTS if l[0] == layout)
        o, p = w.pair(("tier", layout), tl.w_patterns(dictionary), opts=opts)
        text = w.once("tier_text", lambda: tl.w_texts()["words"][:8192 + 17])
        return o, p, text, w.once("tier_dev", lambda: _dev_text(text)) if dev else None
    return handle


def _char_handle(w, dev):
    text = w.once("utf8", lambda: ts._utf8_text(np.random.default_rng(32), ts.SINGLE)).decode()
    return w.s.co, w.s.cp, text, w.once("utf8_dev", lambda: _dev_text(text.encode())) if dev else None


_SEG = ["daac_scan_count_only_range", "daac_scan_count_range", "daac_scan"]
case("segment-darray", _SEG, *_segment(_rich_handle, Engine.DArray, {"overlap_micro": 0}))
case("segment-tiered-rows16", _SEG, *_segment(_tier_handle("default"), Engine.Tiered))
case("segment-tiered-rows32", _SEG, *_segment(_tier_handle("rows32"), Engine.Tiered))
case("segment-charwise", _SEG, *_segment(_char_handle, Engine.Auto, {"overlap_micro": 0}))
case("micro-step-darray", _SEG, *_segment(_rich_handle, Engine.DArray, {"overlap_micro": 1}))
case("micro-step-charwise", _SEG, *_segment(_char_handle, Engine.Auto, {"overlap_micro": 1}))


# ====================================================================================================== 3. the tuple emitter
def _emit_run(p, t, engine):
    out = [ts._sev(p.scan(OV, t, engine=engine)), ts._sev(_free(p.scan_device(OV, t, engine=engine))),
           _sev16(_free(p.scan_device(OV, t, engine=engine, fmt16=True)))]
    assert da.last_engine() == int(Engine.Pfx if engine == Engine.Pfx else Engine.Gram), da.last_engine()
    assert da.last_kernel() == f"emit3 raw={int(engine == Engine.Pfx)} attempts=1", da.last_kernel()
    return out


def _emit_gram(w):
    p = w.gram()[1]
    _set(p, {})
    return _emit_run(p, w.dev("soup", SMALL), Engine.Auto)


case("emit-gram", ["daac_scan", "daac_scan_device", "daac_scan_device16"], _emit_gram, lambda w: [ts._sev(w.tuples("soup", SMALL))] * 3)


RERUN_BYTES = 2 << 20


def _big(m, fmt16=False):
    """a long tuple list in a form that compares fast: how many, and the three columns' bytes"""
    end = m["end"].astype(np.uint64)
    start = end - m["length"].astype(np.uint64) if fmt16 else m["start"].astype(np.uint64)
    return [len(m), start.tobytes(), end.tobytes(), m["value"].astype(np.uint32).tobytes()]


def _raw_dict(w):
    """4 000 patterns of 4 .. 9 random bytes (test_gpu_pfx.py's by_len dictionaries) and 2 MiB of them, two in three, between random bytes"""
    def make():
        rng = np.random.default_rng(8800)
        pats = list(dict.fromkeys(bytes(rng.integers(0, 256, size=int(rng.integers(4, 10))).astype(np.uint8)) for _ in range(4000)))
        k = RERUN_BYTES // 4   # (every part has four bytes at least)
        picks, coin, noise = rng.integers(len(pats), size=k).tolist(), rng.integers(0, 3, size=k).tolist(), rng.integers(0, 256, size=(k, 5), dtype=np.uint8)
        text = np.frombuffer(b"".join(pats[i] if c else noise[j].tobytes() for j, (i, c) in enumerate(zip(picks, coin)))[:RERUN_BYTES], dtype=np.uint8).copy()
        assert len(text) == RERUN_BYTES
        return orc.OraclePma.build(pats), text
    return w.once("raw dict", make)


def _emit_rerun(raw):
    """A new handle (nothing remembered of earlier scans) whose record list is first sized for one deep match per KiB, over 2 MiB of text
    made of the dictionary's words in regions of 1 MiB: one workgroup of at most 16 waves, so the first list has room for about 50 chunks
    of 1 024 records and the text has several hundred thousand deep matches.  The list overflows and the second attempt runs over
    what the first one left in the scratch; daac_last_kernel() says attempts=2."""
    def run(w):
        p, rest = da.DoubleArrayAhoCorasick.deserialize((_raw_dict(w)[0] if raw else w.gram_oracle()).serialize())
        assert rest == b""
        if raw:
            p.set_option("pfx", 2)
        _set(p, {"emit_rec_per_kib": 1, "gram_region": 1 << 20})
        t = w.once("raw dev", lambda: _dev_text(_raw_dict(w)[1])) if raw else w.dev("soup", RERUN_BYTES)
        engine, out = (Engine.Pfx if raw else Engine.Gram), []
        for fmt16 in (False, True):
            out.append(_big(_free(p.scan_device(OV, t, engine=engine, fmt16=fmt16)), fmt16))
            assert da.last_kernel() == f"emit3 raw={int(raw)} attempts={1 if fmt16 else 2}", (da.last_kernel(), "the first scan of a handle reruns, the second knows the size")
        return out

    def want(w):
        m = _raw_dict(w)[0].find_overlapping_iter(_raw_dict(w)[1]) if raw else w.tuples("soup", RERUN_BYTES)
        return [_big(m)] * 2
    return run, want


case("emit-gram-overflow-rerun", ["daac_scan_device", "daac_scan_device16"], *_emit_rerun(False))
case("emit-raw-overflow-rerun", ["daac_scan_device", "daac_scan_device16"], *_emit_rerun(True))


# ================================================================================================ 4. find3 / left3, the chain walkers
def _restart(kind, opts, label):
    leftmost = kind == "leftmost"
    mode, api = (LEFT, "leftmost_find_iter") if leftmost else (FIND, "find_iter")

    def run(w):
        p = w.gram(1 if leftmost else 0)[1]
        _set(p, opts)
        t = w.dev("uniform", SMALL)
        out = [p.count(mode, t)]
        assert da.last_kernel().split()[0] == label, (da.last_kernel(), label)
        out += [list(p.scan_count(mode, t)), ts._sev(p.scan(mode, t)), ts._sev(_free(p.scan_device(mode, t)))]
        return out

    def want(w):
        m = w.tuples("uniform", SMALL, api, leftmost)
        return [len(m), [len(m), orc.matches_checksum(m)], ts._sev(m), ts._sev(m)]
    return run, want


_RESTART = ["daac_scan_count_only_range", "daac_scan_count_range", "daac_scan", "daac_scan_device"]
for _kind, _opt in (("standard", "find3"), ("leftmost", "left3")):
    for _se in (1, 0):   # several windows of 8 192 ends through one d_ctl; the tuples from the selection, and from the chain walkers
        case(f"select-{_kind}-windows-select_emit{_se}", _RESTART,
             *_restart(_kind, {_opt: 2, "find3_window": 8192, "select_emit": _se, "restart_chain": 1}, label="find3"))   # (the label of either selection)
    for _rc in (1, 0):
        case(f"chain-{_kind}-restart_chain{_rc}", _RESTART, *_restart(_kind, {"find3": 0, "left3": 0, "restart_chain": _rc}, label="darray"))


def _char_restart(kind, rc):
    leftmost = kind == "leftmost"
    mode, api = (LEFT, "leftmost_find_iter") if leftmost else (FIND, "find_iter")

    def run(w):
        p = w.s.cpl if leftmost else w.s.cp
        _set(p, {"restart_chain": rc})
        t = _char_handle(w, True)[3]
        out = [p.count(mode, t)]
        assert da.last_kernel() == "charwise", da.last_kernel()   # the charwise walkers, chained or sync-point scanners
        return out + [list(p.scan_count(mode, t)), ts._sev(p.scan(mode, t))]

    def want(w):
        m = getattr(w.s.col if leftmost else w.s.co, api)(_char_handle(w, False)[2])
        return [len(m), [len(m), orc.matches_checksum(m)], ts._sev(m)]
    return run, want


for _kind in ("standard", "leftmost"):
    for _rc in (1, 0):
        case(f"chain-charwise-{_kind}-restart_chain{_rc}", _SEG, *_char_restart(_kind, _rc))


# ================================================================================================ 5. lazy iterators and steppers
ITER_BYTES, ITER_WINDOW = SMALL, 16384   # a host haystack in four windows: both staging buffers are written twice


def _iter(form):
    def run(w):
        p = w.gram()[1]
        _set(p, {"iter_window": ITER_WINDOW})
        host = w.text("uniform", ITER_BYTES).tobytes()
        it = p.find_overlapping_iter(host, compact=form == "next_batch8")
        try:
            got = []
            if form == "next":
                got = [(m.start(), m.end(), m.value()) for m in it]
            elif form == "next_batch":
                while (b := it.next_batch()) is not None:
                    got += _sev16(b)
            else:
                while (r := it.next_batch8()) is not None:
                    got += ts._sev(da.bytewise._Stepper.decode8(*r))
            return got
        finally:
            it.close()
            p.set_option("iter_window", None)
    return run


for _form, _e in (("next", "daac_iter_next"), ("next_batch", "daac_iter_next_batch")):
    case(f"iter-{_form}", ["daac_iter_open", _e, "daac_iter_close"], _iter(_form), lambda w: ts._sev(w.tuples("uniform", ITER_BYTES)))
case("iter-next_batch8", ["daac_iter_open_compact", "daac_iter_next_batch8", "daac_iter_close"], _iter("next_batch8"), lambda w: ts._sev(w.tuples("uniform", ITER_BYTES)))

STEP_TEXT = ("ab全世界a" * 40 + "é世界un" * 30 + "a世").encode()


def _step_cuts():
    """cuts one and two bytes into a three-byte character, one byte into a two-byte one, an empty chunk (a cut twice) and a long chunk"""
    i3, i2 = STEP_TEXT.index("全".encode()), STEP_TEXT.index("é".encode())
    return sorted([i3 + 1, i3 + 12 + 2, 100, 100, i2 + 1, 700])


def _stepper(charwise, api, compact):
    def run(w):
        p = w.s.cp if charwise else w.s.p
        _set(p, {})
        st = getattr(p, api)()
        got, prev = [], 0
        for c in _step_cuts() + [len(STEP_TEXT)]:
            chunk = STEP_TEXT[prev:c]
            if compact:
                got += ts._sev(st.decode8(*st.feed_compact(chunk)))
            else:
                got += ts._sev(st.feed(chunk))
            prev = c
        return got

    def want(w):
        o = w.s.co if charwise else w.s.o
        return ts._sev(getattr(o, api)(STEP_TEXT.decode() if charwise else STEP_TEXT))
    return run, want


for _cw in (False, True):
    for _api in ("find_stepper", "find_overlapping_stepper"):
        for _compact in (False, True):
            case(f"stepper-{'charwise' if _cw else 'bytewise'}-{_api}-{'feed_compact' if _compact else 'feed'}",
                 ["daac_stream_open", "daac_stream_feed_compact" if _compact else "daac_stream_feed", "daac_stream_close"], *_stepper(_cw, _api, _compact))


# ================================================================================================================ 6. histograms
def _hist(bins):
    def run(w):
        o, p, text, dev = _rich_handle(w, True)
        _set(p, {} if bins is None else {"hist_lds_bins": bins})
        return p.histogram(OV, dev).tolist()
    return run


for _bins in (0, None):
    case(f"histogram-lds_bins-{'default' if _bins is None else _bins}", ["daac_scan_histogram"], _hist(_bins),
         lambda w: ts._hist_dense(w.s, w.s.o.find_overlapping_iter(_rich_handle(w, False)[2])))


def _hist_batch_routes(w):
    """test_gpu_batch_hist.py's batch of nine documents that takes all three routes: 4 by a wave, 3 by a workgroup, 2 by dense counters"""
    o, p = w.pair("hist_a", [b"a"], opts={"batch_hist_wave_max": 8, "batch_hist_sort_max": 32})
    rs = [0, 1, 7, 8, 9, 31, 32, 33, 100]
    rows, offs = p.histogram_batch(OV, [b"a" * r for r in rs])
    assert " wave_docs=4 " in da.last_kernel() + " " and " group_docs=3 " in da.last_kernel() + " " and " dense_docs=2 " in da.last_kernel() + " ", da.last_kernel()
    return [list(zip(rows["slot"].tolist(), rows["count"].tolist())), offs.tolist()]


case("histogram_batch-wave-group-dense", ["daac_scan_histogram_batch"], _hist_batch_routes,
     lambda w: [[(0, r) for r in [1, 7, 8, 9, 31, 32, 33, 100]], [0] + list(range(9))])


# ========================================================= 7. test_gpu_streams.py's single-haystack and batch calls, on the null stream
def _entries(name):
    docs_chain = ["daac_split_batch", "daac_spans_rebase", "daac_offsets_compose"]
    table = [("count_batch", ["daac_scan_count_batch"]), ("scan_count_batch", ["daac_scan_count_batch"]), ("scan_batch", ["daac_scan_batch_device16"]),
             ("replace_all_batch", ["daac_replace_all_batch"]), ("replace_all", ["daac_replace_all"]),
             ("tokenize_batch", ["daac_tokenize_batch"]), ("tokenize_unigram_batch", ["daac_tokenize_unigram_batch"]), ("tokenize_unigram", ["daac_tokenize_unigram"]),
             ("tokenize_bpe_docs", ["daac_tokenize_bpe_batch"] + docs_chain), ("tokenize_bpe_batch", ["daac_tokenize_bpe_batch"]), ("tokenize_bpe", ["daac_tokenize_bpe"]),
             ("tokenize_wordpiece_docs-normalizer", ["daac_tokenize_wordpiece_batch", "daac_split_words_space", "daac_normalize_batch", "daac_spans_to_source"] + docs_chain),
             ("tokenize_wordpiece_docs", ["daac_tokenize_wordpiece_batch", "daac_split_words_space"] + docs_chain),
             ("tokenize_wordpiece_batch", ["daac_tokenize_wordpiece_batch"]), ("tokenize_wordpiece", ["daac_tokenize_wordpiece"]), ("tokenize", ["daac_tokenize"]),
             ("histogram_batch", ["daac_scan_histogram_batch"]), ("histogram", ["daac_scan_histogram"]),
             ("normalize_batch", ["daac_normalize_batch"]), ("normalize", ["daac_normalize"]), ("split_batch", ["daac_split_batch"]), ("split", ["daac_split"]),
             ("scan_count", ["daac_scan_count_range"]), ("count", ["daac_scan_count_only_range"]), ("scan_device", ["daac_scan_device"]), ("scan", ["daac_scan"]),
             ("find_iter", ["daac_iter_open", "daac_iter_next", "daac_iter_close"]), ("stepper", ["daac_stream_open", "daac_stream_feed", "daac_stream_close"])]
    for prefix, entries in table:
        if name == prefix or name.startswith(prefix + "-") or name.startswith(prefix + "_device"):
            return entries
    raise KeyError(name)


def _single_input(w, name):
    def make():
        seed = ts.SINGLE_CASES[name][0]
        if seed == "sparse":
            return ts._single_pair(77, ts.SPARSE)[0][0]
        if seed == "word":
            tail = ts._text(np.random.default_rng(5), 17, [b"a", b"b", b"c", b"x", b"s"])
            return np.frombuffer(w.s.long[0] + w.s.long[1] + tail, dtype=np.uint8)
        return ts._single_pair(seed)[0][0]
    return w.once(("single", name), make)


def _single_dev(w, name):
    return w.once(("single_dev", name), lambda: _dev(_single_input(w, name)))


for _name in sorted(ts.SINGLE_CASES):
    case("one-" + _name, _entries(_name),
         lambda w, n=_name: (_plain_streams_world(w), ts.SINGLE_CASES[n][1](w.s, None, _single_dev(w, n)))[1],
         lambda w, n=_name: ts.SINGLE_CASES[n][2](w.s, _single_input(w, n).tobytes()))


def _batch_input(w, name, n):
    """(hay, offsets[, skip]) as numpy arrays: 13 bytes in front of the first document (offsets[0] != 0, off a
    16-byte boundary) and 19 behind the last"""
    def make():
        pieces = ts.BATCH_CASES[name][0]
        rng = np.random.default_rng(8000 + n)
        docs = [ts._text(rng, k, pieces) for k in _batch_lens(n)]
        arrays = list(ts._arrays(docs))
        assert arrays[1][0] == len(ts.FRONT) != 0 and len(docs[n // 2]) == 0 and len(docs[-1]) == 0
        if ts.BATCH_CASES[name][3] == "skip":
            arrays.append((np.random.default_rng(3).random(n) < 0.3).astype(np.uint8) * 7)
        return arrays
    return w.once(("batch", ts.BATCH_CASES[name][0] is ts.WORDS, ts.BATCH_CASES[name][3], n), make)


def _batch_dev(w, name, n):
    return w.once(("batch_dev", ts.BATCH_CASES[name][0] is ts.WORDS, ts.BATCH_CASES[name][3], n), lambda: [_dev(a) for a in _batch_input(w, name, n)])


for _name in sorted(ts.BATCH_CASES):
    for _n in BATCH_SIZES:
        case(f"batch{_n}-{_name}", _entries(_name),
             lambda w, nm=_name, n=_n: (_plain_streams_world(w), ts.BATCH_CASES[nm][1](w.s, None, *_batch_dev(w, nm, n)))[1],
             lambda w, nm=_name, n=_n: ts.BATCH_CASES[nm][2](w.s, *_batch_input(w, nm, n)))


# ============================================================================ 8. the token calls test_gpu_streams.py's tables do not hold
def _ascii_batch(w, n):
    def make():
        rng = np.random.default_rng(8100 + n)
        docs = [ts._text(rng, k, ts.ASCII) for k in _batch_lens(n)]
        hay, off = ts._arrays(docs)
        wo, _, flags = wg.bert_offsets(docs, w.s.bert_table, int(off[0]))
        return docs, hay, off, wo.astype(np.int64), flags
    return w.once(("ascii", n), make)


for _n in BATCH_SIZES:
    case(f"batch{_n}-words_space", ["daac_split_words_space"],
         lambda w, n=_n: w.s.splitters[Split.Bert].words_space((_dev(_ascii_batch(w, n)[1]), _dev(_ascii_batch(w, n)[3]))).tolist(),
         lambda w, n=_n: _ascii_batch(w, n)[4].tolist())


def _to_source(w, n):
    """spans over normalized text, the normalizer's src map and the source batch -> spans over the source (normalize_golden's definition)"""
    def make():
        rng = np.random.default_rng(8200 + n)
        docs = [ts._text(rng, k, ts.RICH) for k in _batch_lens(n)]
        hay, off = ts._arrays(docs)
        spans, src, want, tok_off, out_off = [], [], [], [0], [0]
        for d in docs:
            text, sr = ng.bert_scan(d, ng.OPTIONS["default"])
            _, sp = wg.wordpiece_doc(text, w.s.bert_table, w.s.vocab, 0, 100)
            spans += sp
            src += sr
            want += ng.spans_to_source(sp, sr, d)
            tok_off.append(len(spans))
            out_off.append(len(src))
        return (np.array(spans, dtype=np.int64).reshape(-1, 2), np.array(src, dtype=np.int32), hay, off, np.array(tok_off, dtype=np.int64), np.array(out_off, dtype=np.int64),
                [list(x) for x in want])
    return w.once(("to_source", n), make)


def _to_source_run(w, n):
    spans, src, hay, off, tok, oo, _ = _to_source(w, n)
    sp = _dev(spans)
    da.Normalizer.spans_to_source(sp, _dev(tok), _dev(oo), _dev(src), (_dev(hay), _dev(off)))
    return sp.cpu().numpy().tolist()


for _n in BATCH_SIZES:
    case(f"batch{_n}-spans_to_source", ["daac_spans_to_source"], lambda w, n=_n: _to_source_run(w, n), lambda w, n=_n: _to_source(w, n)[6])


def _specials(w):
    return w.once("specials", lambda: (da.SpecialTokens(sg.specials("bpe")), sg.specials("bpe")))


def _cut_docs(n):
    pieces = [b"<|a|>", b"<|endoftext|>", b"<|b|>", b"he", b"llo ", b"<|", b"|>", b"x", b" "]
    rng = np.random.default_rng(8300 + n)
    return [ts._text(rng, k, pieces) for k in _batch_lens(n)]


def _cut_run(w, n):
    st, _ = _specials(w)
    out = st.cut_batch((_dev(ts._arrays(_cut_docs(n))[0]), _dev(ts._arrays(_cut_docs(n))[1])))
    return [o.tolist() for o in out]


for _n in BATCH_SIZES:
    case(f"batch{_n}-cut_batch", ["daac_cut_batch"], lambda w, n=_n: _cut_run(w, n),
         lambda w, n=_n: [x.tolist() for x in sg.cut(_cut_docs(n), lambda d: sg.leftmost(d, _specials(w)[1]), len(ts.FRONT))])


def _splice_input(n_docs):
    """test_gpu_special.py's random CSR inputs at n_docs documents: text segments of 0 .. 6 tokens, one of 700, specials over 0, 1 or 5
    garbage tokens, empty documents"""
    rng = np.random.default_rng(8400 + n_docs)
    n_segs = 4 * n_docs
    seg_len = rng.integers(1, 30, n_segs)
    values = np.where(rng.integers(0, 3, n_segs) == 0, rng.integers(0, 0xFFFFFFFF, n_segs), sg.TEXT).astype(np.uint32)
    cuts = np.sort(rng.choice(np.arange(n_segs + 1), n_docs - 1))
    cuts[-1] = n_segs   # the last document is empty
    doc_segs = np.concatenate([[0], cuts, [n_segs]]).astype(np.uint64)
    seg_offsets = (11 + np.concatenate([[0], np.cumsum(seg_len)])).astype(np.uint64)
    doc_offsets = seg_offsets[doc_segs.astype(np.int64)]
    counts = np.where(values == sg.TEXT, rng.integers(0, 7, n_segs), rng.choice([0, 1, 5], n_segs))
    counts[int(np.flatnonzero(values == sg.TEXT)[0])] = 700
    seg_tok = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    t = int(seg_tok[-1])
    ids = rng.integers(0, 1 << 32, t, dtype=np.uint64).astype(np.uint32)
    starts = rng.integers(0, 40, t)
    spans = np.stack([starts, starts + rng.integers(0, 9, t)], axis=1).astype(np.uint64)
    return dict(ids=ids, spans=spans, seg_tok=seg_tok, values=values, seg_offsets=seg_offsets, doc_segs=doc_segs, doc_offsets=doc_offsets, hay_len=int(seg_offsets[-1]) + 3)


def _splice_run(w, n):
    import torch
    c = w.once(("splice", n), lambda: _splice_input(n))
    docs = (torch.zeros(c["hay_len"], dtype=torch.uint8, device="cuda"), _dev(c["doc_offsets"]))
    out = da.splice_special(_dev(c["ids"]), _dev(c["spans"]), _dev(c["seg_tok"]), (_dev(c["seg_offsets"]), _dev(c["doc_segs"]), _dev(c["values"])), docs)
    return [o.tolist() for o in out]


def _splice_want(w, n):
    c = w.once(("splice", n), lambda: _splice_input(n))
    return [np.asarray(x).tolist() for x in sg.splice(c["ids"], c["spans"], c["seg_tok"], c["values"], c["seg_offsets"], c["doc_segs"], c["doc_offsets"])]


for _n in BATCH_SIZES:
    case(f"batch{_n}-splice_special", ["daac_tokens_splice"], lambda w, n=_n: _splice_run(w, n), lambda w, n=_n: _splice_want(w, n))

def _compose_input(n):
    rng = np.random.default_rng(8900 + n)
    inner = np.cumsum(rng.integers(0, 9, size=4 * n + 1)).astype(np.int64)
    outer = np.sort(rng.integers(0, 4 * n + 1, size=n + 1)).astype(np.int64)
    outer[0], outer[-1] = 0, 4 * n
    return inner, outer


for _n in BATCH_SIZES:
    case(f"batch{_n}-offsets_compose", ["daac_offsets_compose"],
         lambda w, n=_n: da.offsets_compose(_dev(_compose_input(n)[0]), _dev(_compose_input(n)[1])).tolist(),
         lambda w, n=_n: _compose_input(n)[0][_compose_input(n)[1]].tolist())

BERT_SINGLE = [["special", 101, 0], ["A", 0, 0], ["special", 102, 0]]
BERT_PAIR = BERT_SINGLE + [["B", 0, 1], ["special", 102, 1]]
PACK_FORMS = {"right": dict(padding_side="right"), "left": dict(padding_side="left"), "csr": dict(padding=None)}


def _pack_input(n):
    def seq(seed):
        rng = np.random.default_rng(seed)
        lens = [k // 3 for k in _batch_lens(n)]
        out = []
        for k in lens:
            ends = np.cumsum(rng.integers(1, 6, size=k)).tolist()
            out.append(list(zip(rng.integers(10, 30000, size=k).tolist(), [0] + ends[:-1], ends)))
        return out
    return seq(8500 + n), seq(8600 + n)


def _pack_cfg(form):
    return pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=24, pad_id=7, pad_type_id=1, **PACK_FORMS[form])


def _pack_run(w, n, form):
    a, b = w.once(("pack", n), lambda: _pack_input(n))
    planes = da.Packer(**pg.packer_kwargs(_pack_cfg(form)), dtype=np.int64).pack(pg.flatten(a), pg.flatten(b))
    return {k: v.tolist() for k, v in planes.items()}   # every slot of every plane, the padding included


def _pack_want(w, n, form):
    a, b = w.once(("pack", n), lambda: _pack_input(n))
    return {k: np.asarray(v).tolist() for k, v in pg.pack(a, b, _pack_cfg(form)).items()}


for _n in BATCH_SIZES:
    for _form in PACK_FORMS:
        case(f"batch{_n}-pack-{_form}", ["daac_tokens_pack"], lambda w, n=_n, f=_form: _pack_run(w, n, f), lambda w, n=_n, f=_form: _pack_want(w, n, f))

PACK_DOCS = ["", "-spans", "-normalizer", "-spans-normalizer"]


def _pack_docs_cfg():
    return pg.config(single=BERT_SINGLE, max_length=16, pad_id=7, pad_type_id=1)


def _pack_docs_run(w, n, form):
    """tokenize_wordpiece_docs(pack=): the token result stays in device memory, goes through Packer.pack as a batch of singles and is freed"""
    _plain_streams_world(w)
    hay, off = _batch_dev(w, "tokenize_wordpiece_docs", n)[:2]
    planes = w.s.wp.tokenize_wordpiece_docs((hay, off), w.s.first, w.s.cont, 0, spans="spans" in form, normalizer=w.s.nz if "normalizer" in form else None,
                                            pack=da.Packer(**pg.packer_kwargs(_pack_docs_cfg()), dtype=np.int64))
    assert da.last_kernel().startswith(f"pack docs={n} pair=0 row="), da.last_kernel()
    return {k: v.tolist() for k, v in planes.items()}


def _pack_docs_want(w, n, form):
    docs = ts._split(*_batch_input(w, "tokenize_wordpiece_docs", n)[:2])
    ids, spans, off = ts._wordpiece_docs_want(w.s, docs, "normalizer" in form)
    a = [[(ids[i], spans[i][0], spans[i][1]) for i in range(off[d], off[d + 1])] for d in range(n)]
    planes = pg.pack(a, None, _pack_docs_cfg())
    return {k: np.asarray(v).tolist() for k, v in planes.items() if "spans" in form or k != "offsets"}


for _n in BATCH_SIZES:
    for _form in PACK_DOCS:
        chain = ["daac_tokens_pack", "daac_tokenize_wordpiece_batch", "daac_split_batch", "daac_split_words_space", "daac_offsets_compose"]
        chain += ["daac_spans_rebase"] if "spans" in _form else []
        chain += ["daac_normalize_batch"] + (["daac_spans_to_source"] if "spans" in _form else []) if "normalizer" in _form else []
        case(f"batch{_n}-tokenize_wordpiece_docs-pack{_form}", chain, lambda w, n=_n, f=_form: _pack_docs_run(w, n, f), lambda w, n=_n, f=_form: _pack_docs_want(w, n, f))

DEC_SKIP = 66


def _decoder(w):
    def make():
        import test_gpu_decode as td
        return td._seeded_table()
    return w.once("decoder", make)


def _decode_docs(n):
    rng = np.random.default_rng(8700 + n)
    return [rng.integers(0, DEC_SKIP + 1, size=k // 3).tolist() for k in _batch_lens(n)]


def _decode_run(w, n, form):
    dec, _ = _decoder(w)
    docs = _decode_docs(n)
    if form == "csr":
        tokens = (np.array([i for d in docs for i in d], dtype=np.uint32), np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64))
        texts, starts = dec.decode_batch(tokens, token_starts=True)
    else:
        texts, starts = dec.decode_batch(np.array(_dense_rows(docs), dtype=np.int64), unknown="skip", token_starts=True)
    return [texts, starts.tolist()]


def _dense_rows(docs):
    """a dense int64 plane padded with the special on the right, every fifth token replaced by an id outside [0, 2^32): -1, 2^32 + 5, -2^40"""
    rows = dg.padded(docs, DEC_SKIP)
    junk = [-1, (1 << 32) + 5, -(1 << 40)]
    return [[junk[(i + j) % 3] if (i + j) % 5 == 4 else x for j, x in enumerate(r)] for i, r in enumerate(rows)]


def _decode_want(w, n, form):
    _, table = _decoder(w)
    docs = _decode_docs(n)
    if form == "csr":
        texts, starts = dg.decode_batch(table, docs)
    else:
        texts, starts = dg.decode_batch(table, _dense_rows(docs), unknown="skip")
    return [texts, starts]


for _n in BATCH_SIZES:
    for _form in ("csr", "dense-int64-unknown-skip"):
        case(f"batch{_n}-decode-{_form}", ["daac_tokens_decode"], lambda w, n=_n, f=_form: _decode_run(w, n, f), lambda w, n=_n, f=_form: _decode_want(w, n, f))


# =============================================================================================================== 9. two shards
def _multi(w):
    """one haystack as two shards on device 0, the second with its halo in front"""
    o, p = w.gram()
    _set(p, {})
    t = w.dev("soup", SMALL)
    halo, cut = max(len(x) for x in w.cfg3) - 1, SMALL // 2 + 3
    got = da.scan_count_multi(p, OV, [(0, t[:cut], 0, 0), (0, t[cut - halo:], halo, cut)])
    return list(got)


case("scan_count_multi-two-shards", ["daac_scan_count_multi"], _multi, lambda w: [len(w.tuples("soup", SMALL)), orc.matches_checksum(w.tuples("soup", SMALL))])


def driven():
    """every C entry point some case drives"""
    return functools.reduce(set.union, (set(c.entries) for c in CASES.values()), set())
