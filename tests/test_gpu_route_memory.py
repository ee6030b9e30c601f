"""What a long-lived handle remembers about the text it has seen, and what that does to the restart iterators' routes (api_select.hip chooses, per
request and per window, between the selection kernels — find3_kernels.hip / left3_kernels.hip, Engine.Gram — and the chain walkers).  Every
expected count, checksum and list is the oracle's (reference src/bytewise/iter.rs:58-113, 272-340) on the same bytes; one thread, options
on the handle only, a fresh handle per scenario (the memory lives in the handle's device tables).

Section 1, memory across requests (find_count3_window's gates):
  a  find3_rec_per_kib > kDenseRecPerKib + 1 turns requests of 1 MiB or more away; every sixteenth (find3_skips) looks again, and beyond
     8 MiB it looks at a 4 MiB SAMPLE through the function itself — dense, sparse x 20, dense x 20, sparse again on 12 MiB texts
  b  the same schedule on 2 MiB texts: the sixteenth request is detected whole, no sample
  c  requests below 1 MiB are always tried and overwrite the memory the long requests go by
  d  find3_gave_up >= 2 turns requests of 1 MiB or more away but every sixteenth (find3_retry); one give-up alone does not
  e  emit3_rec_per_kib sizes the next request's record list: from a text without a pattern byte (hint 1) to the word soup the list overflows
     and is rerun with the exact size (attempt == 1) — find3, left3 and the overlapping emitter share the hint
Section 2, text that changes inside one request: a window the selection kernels serve, then one they refuse (find_count3's loop, select_emit's
counted-then-emitted branch: partial sums and the partial list are dropped, the walkers redo the request), and the per-window consumers —
the lazy iterator and the steppers — where a window of one engine hands `next_begin` to a window of the other.
Section 3: emit3_gave_up / emit3_retry of the overlapping emitter, with the give-up text of test_gpu_parity.py::test_gram_tuple_emitter.

The engines each scenario met are printed (one letter per request: G = Engine.Gram, D = DArray, T = Tiered, P = Pfx)."""
import collections
import functools
import re

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

MIB = 1 << 20
GRAM = int(Engine.Gram)

Kind = collections.namedtuple("Kind", "name o mode api opt")
FIND = Kind("find", orc.STANDARD, ScanMode.Find, "find_iter", "find3")
LONGEST = Kind("longest", orc.LEFTMOST_LONGEST, ScanMode.LeftmostFind, "leftmost_find_iter", "left3")
FIRST = Kind("first", orc.LEFTMOST_FIRST, ScanMode.LeftmostFind, "leftmost_find_iter", "left3")
BOTH = [pytest.param(FIND, id="find"), pytest.param(LONGEST, id="longest")]
ALL3 = BOTH + [pytest.param(FIRST, id="first")]


def _same(got, want):
    return len(got) == len(want) and np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]) and \
        np.array_equal(got["value"], want["value"])


def _same16(got16, want):
    return len(got16) == len(want) and np.array_equal(got16["end"], want["end"]) and np.array_equal(got16["value"], want["value"]) and \
        np.array_equal(got16["length"].astype(np.uint64), want["end"] - want["start"])


def _letters(engines):
    return "".join("G" if e == GRAM else Engine(e).name[0] for e in engines)


# ---- dictionaries, texts and the oracle's answers: made once ----
@functools.lru_cache(maxsize=None)
def _patterns(giveup=False):
    """cfg3's full dictionary (K = 3 tables, find3 / left3); `giveup`: test_find3_gives_up_where_the_relaxation_will_not_settle's own — four
    words the relaxation will not settle on over a run of a's, before cfg3's first 3 000.  (The full cfg3 holds "aaaa": one deep match per
    position of such a run, which the density gate turns away before the relaxation is ever tried, and nothing would be given up.)"""
    return [b"aa", b"aaa", b"b", b"ab"] + synth.patterns_cfg3(3000) if giveup else synth.patterns_cfg3()


@functools.lru_cache(maxsize=None)
def _oracle(kind_o, giveup=False):
    return orc.OraclePma.build(_patterns(giveup), kind=kind_o)


@functools.lru_cache(maxsize=None)
def _blob(kind_o, giveup=False):
    return _oracle(kind_o, giveup).serialize()


def _handle(k, giveup=False):
    p, rest = da.DoubleArrayAhoCorasick.deserialize(_blob(k.o, giveup))
    assert rest == b""
    return p


@functools.lru_cache(maxsize=None)
def _text(name):
    if name == "S":    # sparse: test_find3_one_gib_of_cfg3's random text
        return synth.uniform_haystack(12 * MIB, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
    if name == "D":    # dense: its soup of the dictionary's own words
        return synth.wordsoup_haystack(12 * MIB, synth.SEEDS["cfg3_dense"], _patterns(False), 20)
    if name == "B":    # no pattern byte at all: no deep match, the record hint becomes 1
        return np.full(12 * MIB, ord("#"), dtype=np.uint8)
    if name == "GU":   # test_find3_gives_up_where_the_relaxation_will_not_settle's text, beyond the 1 MiB the remembering gate starts at
        return np.frombuffer(b"a" * 700000 + b"b" + b"a" * 400001, dtype=np.uint8)
    if name in ("S2", "D2"):
        return np.ascontiguousarray(_text(name[0])[:2 * MIB])
    if name in ("S3", "D3"):
        return np.ascontiguousarray(_text(name[0])[:3 * MIB])
    if name in ("Ss", "Ds"):
        return np.ascontiguousarray(_text(name[0])[:300000])
    S, D = _text("S"), _text("D")
    if name == "M1":
        return np.concatenate([S[:3 * MIB], D[:3 * MIB], S[3 * MIB:6 * MIB]])
    if name == "M2":
        return np.concatenate([S[:3 * MIB], np.frombuffer(b"a" * 300000 + b"b" + b"a" * 100001, dtype=np.uint8), S[3 * MIB:6 * MIB]])
    if name == "M3":
        return np.concatenate([D[:3 * MIB], S[:3 * MIB]])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _dev(name):
    import torch
    return torch.from_numpy(_text(name).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _want(k, name, giveup=False, api=None):
    """(list, count, checksum) of the oracle's iterator over the whole text"""
    m = getattr(_oracle(k.o, giveup), api or k.api)(_text(name))
    return m, len(m), orc.matches_checksum(m)


def _check_lists(p, k, name, giveup):
    m = _want(k, name, giveup)[0]
    for fmt16 in (True, False):
        dm = p.scan_device(k.mode, _dev(name), fmt16=fmt16)
        got = dm.to_numpy()
        dm.free()
        assert (_same16 if fmt16 else _same)(got, m), (k.name, name, "scan_device", fmt16, da.last_engine())


def _request(p, k, name, giveup=False, lists=False):
    """One request in every form: scan_count and count (and, `lists`, the list in both device formats) against the oracle; -> the engine that
    served scan_count"""
    _, n, cs = _want(k, name, giveup)
    got = p.scan_count(k.mode, _dev(name))
    eng = da.last_engine()
    assert got == (n, cs), (k.name, name, eng)
    assert p.count(k.mode, _dev(name)) == n, (k.name, name, da.last_engine())
    if lists:
        _check_lists(p, k, name, giveup)
    return eng


@pytest.fixture(scope="module", autouse=True)
def _release_texts_and_lists():
    """the texts on the device and the oracle's lists are made once for this module and given back when it is through"""
    yield
    import torch
    for cached in (_dev, _want, _text, _blob, _oracle, _patterns):
        cached.cache_clear()
    torch.cuda.empty_cache()


def _first_gram(engines):
    return next((i for i, e in enumerate(engines) if e == GRAM), None)


def _recovers(engines, what):
    """served by the selection kernels again within sixteen requests (the `& 15u` retry counters), and by them from then on"""
    i = _first_gram(engines)
    assert i is not None and i < 16, (what, _letters(engines))
    assert all(e == GRAM for e in engines[i:]), (what, _letters(engines))


# ---- 1. handle memory across requests ----
def _dense_then_sparse_again(k, sparse, dense):
    p = _handle(k)
    seq = [_request(p, k, sparse, lists=True)]
    assert seq[0] == GRAM, (k.name, "a fresh handle serves the sparse text by selection", _letters(seq))
    seq.append(_request(p, k, dense, lists=True))
    assert seq[1] != GRAM, (k.name, "the dense text goes to the walkers", _letters(seq))
    back = [_request(p, k, sparse, lists=i % 5 == 0) for i in range(20)]
    _recovers(back, (k.name, sparse, "after", dense))
    again = [_request(p, k, dense, lists=i % 5 == 0) for i in range(20)]
    assert GRAM not in again, (k.name, _letters(again))
    once_more = []
    while len(once_more) < 20 and (not once_more or once_more[-1] != GRAM):   # (until it is back; the bound is asserted below)
        once_more.append(_request(p, k, sparse, lists=len(once_more) % 5 == 0))
    _recovers(once_more, (k.name, sparse, "a second time"))
    print(f"\n1 {sparse}/{dense} {k.name}: {_letters(seq)} {_letters(back)} {_letters(again)} {_letters(once_more)}")


@pytest.mark.parametrize("k", BOTH)
def test_dense_then_sparse_again_on_long_requests(k):
    """1a: 12 MiB > 2 x 4 MiB — every sixteenth turned-away request runs find_count3_window on a 4 MiB sample of itself first"""
    _dense_then_sparse_again(k, "S", "D")


@pytest.mark.parametrize("k", BOTH)
def test_dense_then_sparse_again_on_requests_below_the_sample(k):
    """1b: 2 MiB <= 8 MiB — the sixteenth request is detected whole.  (Not LeftmostFirst: its builder drops every word that has an earlier
    word as a prefix, the soup of cfg3's words holds few deep matches of what is left and is no dense text to that handle.)"""
    _dense_then_sparse_again(k, "S2", "D2")


@pytest.mark.parametrize("k", BOTH)
def test_short_requests_rewrite_the_memory(k):
    """1c.  From the code: a request below 1 MiB passes every gate (`len - begin >= 1 << 20` guards them all) and, once selected, stores its own
    deep matches per KiB in find3_rec_per_kib.  So 300 KB of word soup served by the selection kernels leaves the handle `dense` and the next
    12 MiB of random text is turned away (the first of sixteen) — or the short request was given up and the long one is served as before: one
    or the other.  And 300 KB of random text is served by selection whatever came before, leaves the handle `sparse`, and the 12 MiB of
    word soup behind it is detected, found dense and left to the walkers."""
    p = _handle(k)
    assert _request(p, k, "S", lists=True) == GRAM
    short = _request(p, k, "Ds", lists=True)
    long_ = _request(p, k, "S", lists=True)
    assert (short == GRAM) != (long_ == GRAM), (k.name, _letters([short, long_]))
    q = _handle(k)
    assert _request(q, k, "S") == GRAM
    assert _request(q, k, "D", lists=True) != GRAM
    short2 = _request(q, k, "Ss", lists=True)
    assert short2 == GRAM, k.name
    long2 = _request(q, k, "D", lists=True)
    assert long2 != GRAM, k.name
    print(f"\n1c {k.name}: G{_letters([short, long_])} / GD{_letters([short2, long2])}")


@pytest.mark.parametrize("k", BOTH)
def test_give_up_memory(k):
    """1d: two give-ups in a row turn requests of 1 MiB or more away, every sixteenth tries again and a success forgets them; shorter requests
    are tried all along; one give-up alone turns nothing away"""
    p = _handle(k, giveup=True)
    gave = [_request(p, k, "GU", giveup=True, lists=True) for _ in range(2)]
    assert GRAM not in gave, (k.name, _letters(gave))
    back = [_request(p, k, "S2", giveup=True, lists=i % 5 == 0) for i in range(20)]
    assert back[0] != GRAM, (k.name, "two give-ups turn the next long request away", _letters(back))
    _recovers(back, (k.name, "after two give-ups"))
    _, n, cs = _want(k, "GU", True)
    assert p.scan_count(k.mode, _dev("GU")) == (n, cs)   # (one call: every call of a request gives up on its own)
    one = da.last_engine()
    assert one != GRAM
    at_once = _request(p, k, "S2", giveup=True, lists=True)
    assert at_once == GRAM, (k.name, "a single give-up is below the threshold of two")
    # while the long requests are being turned away, a short one is served (and its success forgets the give-ups)
    q = _handle(k, giveup=True)
    gave2 = [_request(q, k, "GU", giveup=True) for _ in range(2)]
    away = _request(q, k, "S2", giveup=True)
    assert GRAM not in gave2 and away != GRAM, (k.name, _letters(gave2 + [away]))
    short = _request(q, k, "Ss", giveup=True, lists=True)
    assert short == GRAM, k.name
    after = _request(q, k, "S2", giveup=True, lists=True)
    assert after == GRAM, k.name
    print(f"\n1d {k.name}: {_letters(gave)} {_letters(back)} {_letters([one, at_once])} / {_letters(gave2 + [away, short, after])}")


@pytest.mark.parametrize("k", BOTH)
def test_record_list_sized_by_the_text_before(k):
    """1e: the list sized from a hint of 1 overflows on the word soup and is rerun once with the exact size — every form of the request right
    behind the text without a pattern byte; then the reverse order (a list sized by the soup for no record at all, then random text).
    That the first list is too short follows from find_count3_window's arithmetic, the results alone do not show it: 12 MiB are 12 288 KiB,
    chunk_cap = 12 289 * 1 / kEmit3Chunk * 2 + 2 * nwaves + 16 with kEmit3Chunk = 1 024 records and 192 regions of 64 KiB, so at most one
    wave each: 24 + 384 + 16 = 424 chunks, 434 176 records filled to the brim — the soup holds some 726 000 deep matches (59.1 per KiB,
    test_host_logic.py).  emit_overlapping3 sizes its list by the same formula."""
    p = _handle(k)
    p.set_option(k.opt, 2)   # (whatever the text: the selection kernels serve the soup, and the blank text behind it is not turned away as dense)
    m, n, cs = _want(k, "D", False)

    def blank():
        assert _request(p, k, "B") == GRAM

    blank()
    assert p.scan_count(k.mode, _dev("D")) == (n, cs) and da.last_engine() == GRAM, k.name
    blank()
    assert p.count(k.mode, _dev("D")) == n and da.last_engine() == GRAM, k.name
    for fmt16 in (True, False):
        blank()
        dm = p.scan_device(k.mode, _dev("D"), fmt16=fmt16)
        assert da.last_engine() == GRAM, k.name
        got = dm.to_numpy()
        dm.free()
        assert (_same16 if fmt16 else _same)(got, m), (k.name, fmt16)
    for lists in (False, True):
        assert _request(p, k, "D", lists=lists) == GRAM
        assert _request(p, k, "B", lists=lists) == GRAM
        assert _request(p, k, "S", lists=lists) == GRAM


def test_record_list_hint_is_shared_with_the_overlapping_emitter():
    """1e: the same pairs through FindOverlapping's tuples (emit_overlapping3 reads and writes the same emit3_rec_per_kib), and across the
    two request kinds: find3's hint sizes the emitter's list and the other way round"""
    p = _handle(FIND)
    ov = lambda name: _want(FIND, name, False, "find_overlapping_iter")

    def overlapping(name, fmt16):
        dm = p.scan_device(ScanMode.FindOverlapping, _dev(name), fmt16=fmt16)
        assert da.last_engine() == GRAM, name
        got = dm.to_numpy()
        dm.free()
        assert (_same16 if fmt16 else _same)(got, ov(name)[0]), (name, fmt16)

    for fmt16 in (True, False):
        overlapping("B", fmt16)
        overlapping("D", fmt16)   # from a hint of 1
        overlapping("B", fmt16)
        overlapping("S", fmt16)
    p.set_option("find3", 2)
    assert _request(p, FIND, "B") == GRAM
    overlapping("D", True)        # find3's hint of 1
    overlapping("B", False)
    assert _request(p, FIND, "D", lists=True) == GRAM   # the emitter's hint of 1


# ---- 2. text that changes inside one request ----
MIXED = [pytest.param("M1", False, id="sparse-dense-sparse"), pytest.param("M2", True, id="sparse-giveup-sparse"), pytest.param("M3", False, id="dense-sparse")]


@pytest.mark.parametrize("k", BOTH)
def test_the_engines_really_alternate_on_the_mixed_text(k):
    """precondition of section 2 under the default setting: M1's first part alone is the selection kernels', its second part alone is not"""
    assert _request(_handle(k), k, "S3") == GRAM
    assert _request(_handle(k), k, "D3") != GRAM
    assert _request(_handle(k, True), k, "S3", giveup=True) == GRAM   # M2's first part, on its dictionary


# where the shards begin (near these offsets, at the end of one of the oracle's matches): inside the first part, inside the second
SHARDS = {"M1": (MIB + MIB // 2 + 12345, 4 * MIB + 54321), "M2": (MIB + MIB // 2 + 12345, 3 * MIB + 150000), "M3": (MIB + MIB // 2 + 12345, 4 * MIB + 54321)}


def _selection_serves(k, name, win, shard):
    """Does a FRESH handle under the default setting end this request on the selection kernels?  From api_select.hip as it reads:
    - M3 from inside its second part is random text to the end: served.
    - M2 meets the run of a's in every other request, at the latest in its fourth window: given up there, whatever the kind.
    - LeftmostFirst drops every word with an earlier word as a prefix; the soup is not dense to it: nothing claimed (None).
    - A leftmost window of `find3_window` = 1 MiB is detected over 1 MiB - 64 + 32 bytes, below the 1 MiB every gate begins at: no window is
      ever weighed, all are served.
    - Otherwise a window (or the one window of the default setting, by its average) holds more than 26 deep matches per KiB: refused —
      on M1 behind windows that were served, whose sums and tuples are dropped."""
    if name == "M3" and shard == 1:
        return True
    if name == "M2":
        return False
    if k is FIRST:
        return None
    if k is LONGEST and win == MIB:
        return True
    return False


@pytest.mark.parametrize("name,giveup", MIXED)
@pytest.mark.parametrize("k", ALL3)
def test_mixed_text_in_one_request(k, name, giveup):
    """windows of one request: served, served, refused (default setting: dense or given up in a LATER window — what the windows before it
    summed and listed is dropped and the walkers answer the whole request), or all served (find3 / left3 = 2 on M1 and M3).  Under the
    default setting every call has a handle of its own — the first refusal would leave the handle `dense` (or, twice, `given up`) and turn
    every later call away at its FIRST window — and the engine it ends on is asserted: that of _selection_serves."""
    m, n, cs = _want(k, name, giveup)
    hay, dev = _text(name), _dev(name)
    shards = []
    for target in SHARDS[name]:   # `begin` is where the chain restarts, so it is put at the end of one of the oracle's matches — the iterator
        i = int(np.searchsorted(m["end"], target))   # restarts there itself and what it reports from then on is the rest of its list
        shards.append((int(m["end"][i]), m[i + 1:]))
    seq = []
    for opt in (None, 2):
        shared = _handle(k, giveup).set_option(k.opt, 2) if opt == 2 else None   # (find3 / left3 = 2: no memory of the text, one handle will do)
        for win in (MIB, MIB + 4096 + 17, None):
            what = (k.name, name, opt, win)

            def call(form, fn, shard=None):
                p = shared if shared is not None else _handle(k, giveup)
                p.set_option("find3_window", win)
                got = fn(p)
                eng = da.last_engine()
                if opt is None:
                    serves = _selection_serves(k, name, win, shard)
                    assert serves is None or (eng == GRAM) == serves, what + (form, shard, _letters([eng]))
                elif not giveup:
                    assert eng == GRAM, what + (form, shard)
                return got, eng

            got, eng = call("scan_count", lambda p: p.scan_count(k.mode, dev))
            seq.append(eng)
            assert got == (n, cs), what
            assert call("count", lambda p: p.count(k.mode, dev))[0] == n, what
            for fmt16 in (True, False):
                dm = call("scan_device", lambda p: p.scan_device(k.mode, dev, fmt16=fmt16))[0]
                lst = dm.to_numpy()
                dm.free()
                assert (_same16 if fmt16 else _same)(lst, m), what + ("scan_device", fmt16)
            assert _same(call("daac_scan", lambda p: p.scan(k.mode, hay))[0], m), what + ("daac_scan",)
            for si, (b, rest) in enumerate(shards):
                assert call("scan_count", lambda p: p.scan_count(k.mode, dev, begin=b), si)[0] == (len(rest), orc.matches_checksum(rest)), what + (b,)
                assert call("count", lambda p: p.count(k.mode, dev, begin=b), si)[0] == len(rest), what + (b,)
    print(f"\n2 {name} {k.name}: default {_letters(seq[:3])}, forced {_letters(seq[3:])}")


def _iterate(p, k, hay, compact):
    """the lazy iterator's batches, concatenated -> ({end, length, value}, the engine of every batch)"""
    it = getattr(p, k.api)(hay, compact=compact)
    ends, lens, vals, engines = [], [], [], []
    while True:
        got = it.next_batch8() if compact else it.next_batch()
        if got is None:
            break
        engines.append(da.last_engine())
        if compact:
            run, base, eb = got
            ends.append((run["end_len"] & np.uint32((1 << eb) - 1)).astype(np.uint64) + np.uint64(base))
            lens.append((run["end_len"] >> np.uint32(eb)).astype(np.uint32))
        else:
            run = got
            ends.append(run["end"].copy())
            lens.append(run["length"].copy())
        vals.append(run["value"].copy())
    it.close()
    out = np.zeros(sum(len(e) for e in ends), dtype=da.bytewise.MATCH16_DTYPE)
    if len(out):
        out["end"], out["length"], out["value"] = np.concatenate(ends), np.concatenate(lens), np.concatenate(vals)
    return out, engines


@pytest.mark.parametrize("name,giveup", MIXED)
@pytest.mark.parametrize("k", BOTH)
def test_mixed_text_through_the_lazy_iterator(k, name, giveup):
    """every window is routed on its own: a window of the selection kernels hands next_begin (the end of its last match, or 64 bytes before
    its end) to a window of the chain walkers (the first sync point at or behind its end) and back"""
    m = _want(k, name, giveup)[0]
    for opt in (None, 2):
        p = _handle(k, giveup)
        p.set_option(k.opt, opt)
        seqs = []
        for win in (MIB, MIB + 37):
            p.set_option("iter_window", win)
            for compact in (False, True):
                got, engines = _iterate(p, k, _dev(name) if compact else _text(name), compact)
                seqs.append(_letters(engines))
                assert len(engines) > 3 and _same16(got, m), (k.name, name, opt, win, compact, seqs[-1])
        print(f"\n2 iterator {name} {k.name} {k.opt}={opt}: {' '.join(seqs)}")
        if name == "M1" and opt is None:   # a fresh handle: the first windows are random text, then the soup begins
            assert seqs[0][0] == "G" and seqs[0].strip("G") != "", seqs[0]
        if name == "M2":   # one give-up is below the threshold of two and the next served window forgets it: selection, walkers and back, in every run
            assert all(re.search("G[^G]+G", q) for q in seqs), seqs


def _ragged(n):
    """test_long_stream_device_chunks_and_bounded_carry's chunk sizes"""
    i, k = 0, 0
    while i < n:
        step = [65536, 1 << 20, 3, 300_001, 4096][k % 5]
        yield i, min(n, i + step), k
        i += step
        k += 1


@pytest.mark.parametrize("name,giveup", MIXED)
def test_mixed_text_through_the_steppers(name, giveup):
    """find_stepper and find_overlapping_stepper, feed and feed_compact: every feed is a request of its own ([what the chain has not decided
    yet | chunk]) — 1 MiB device chunks (each at the remembering gate) and ragged ones (the short ones rewrite the memory)"""
    hay, dev = _text(name), _dev(name)
    o = _oracle(orc.STANDARD, giveup)
    for opt in (None, 2):
        for api in ("find_stepper", "find_overlapping_stepper"):
            want = getattr(o, api)(hay)
            p = _handle(FIND, giveup)
            p.set_option("find3", opt)
            seqs = []
            for compact in (False, True):
                for ragged in (False, True):
                    st = getattr(p, api)()
                    parts, engines = [], []
                    cuts = _ragged(len(hay)) if ragged else ((i, min(len(hay), i + MIB), 1) for i in range(0, len(hay), MIB))
                    for i, j, c in cuts:
                        chunk = dev[i:j] if c % 3 else hay[i:j]
                        parts.append(st.decode8(*st.feed_compact(chunk)) if compact else st.feed(chunk).copy())
                        engines.append(da.last_engine())
                    got = np.concatenate([x for x in parts if len(x)])
                    seqs.append(_letters(engines))
                    assert _same(got, want), (name, opt, api, compact, ragged, seqs[-1])
            print(f"\n2 {api} {name} find3={opt}: {' '.join(seqs)}")
            if name == "M1" and opt is None and api == "find_stepper":   # a fresh handle, 1 MiB chunks: random text first, then the soup
                assert seqs[0][0] == "G" and seqs[0].strip("G") != "", seqs[0]
            if name == "M2" and api == "find_stepper":   # the feed that holds the run of a's is the walkers', those around it are not
                assert all(re.search("G[^G]+G", q) for q in seqs), seqs


# ---- 3. the overlapping emitter's own give-ups ----
def test_overlapping_emitter_gives_up_twice_then_recovers():
    """emit3_gave_up >= 2 turns FindOverlapping's tuple requests of 1 MiB or more away but every sixteenth (emit3_retry); a served one forgets
    the give-ups.  The text it gives up on is test_gram_tuple_emitter's: thirteen deep matches per position."""
    pats = [b"a" * n for n in range(1, 17)]
    o = orc.OraclePma.build(pats)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    hay = np.frombuffer(b"a" * 5000 + b"b" + b"a" * 3000, dtype=np.uint8)
    want = o.find_overlapping_iter(hay)
    for _ in range(2):
        assert _same(p.scan(ScanMode.FindOverlapping, hay), want) and da.last_engine() != GRAM
    want2 = o.find_overlapping_iter(_text("S2"))
    engines = []
    for i in range(20):
        dm = p.scan_device(ScanMode.FindOverlapping, _dev("S2"), fmt16=i % 2 == 0)
        engines.append(da.last_engine())
        got = dm.to_numpy()
        dm.free()
        assert (_same16 if i % 2 == 0 else _same)(got, want2), (i, _letters(engines))
    print(f"\n3 overlapping: {_letters(engines)}")
    assert engines[0] != GRAM, _letters(engines)
    _recovers(engines, "the overlapping emitter")
