"""Every device entry point on a caller's stream (include/daachorse_amd.h: "every device entry point takes a `stream` on which all
of its work is ordered", and several host threads may scan through one handle, each on its own stream).

1. Ordered after the caller's work.  The inputs of a call sit in device memory holding a DECOY: a well-formed input of the same sizes
   with other text and other document boundaries.  On a fresh stream s a device-side delay of about 50 ms is queued and behind it
   the copies of the real inputs over the decoys; the call is then made with stream=s while the delay is still pending.  A launch,
   memset or copy of the library that is not ordered on s reads the decoy and computes the decoy's answer, never an address out of
   range.  test_control shows that other streams do not wait behind s and that the delay is long enough.
2. Every device batch starts `front` bytes into its buffer (offsets[0] != 0, off a 16-byte boundary) and has bytes behind
   offsets[n]; a pattern matches across both ends, so a kernel that looked outside its documents would report it.
3. Four threads, each with its own stream, inputs and expected results of its own size, share the handles, splitters and the
   normalizer, none of them uploaded before the threads start.
4. The n == 0 forms of the batch calls on a stream with work pending in front.

Expected results come from the references the suite has (the CPU oracle, the splice / token / Viterbi / BPE definitions of the other
GPU test modules, the sequential split scanners, wordpiece_golden, normalize_golden), never from the library."""
import contextlib
import gc
import threading
import time

import numpy as np
import pytest
import torch

import normalize_golden as ng
import wordpiece_golden as wg
from oracle import oracle as orc
from test_gpu_batch_hist import _Slots
from test_gpu_replace import _splice
from test_gpu_tokenize import _tokens
from test_gpu_tokenize_bpe import _bpe
from test_gpu_tokenize_unigram import _viterbi
from test_split_host import scan_batch as split_scan_batch
from test_split_rules_host import scan_rule_batch

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, ScanMode, Split

GID = 0x10000   # keeps gap ids apart from values
DELAY_MS = 50.0
# a, b and c are patterns of their own, u and n are not: "un" is the pattern that FRONT and TAIL make match across a batch's ends
PATS = [b"abc", b"bc", b"c", b"cab", b"aa", b"a", b"b", b"un", b"able", b" "]
TABLE = [b"<%d>" % i for i in range(len(PATS))]
SCORES = np.array([-(1.0 + 0.37 * i) for i in range(len(PATS))], dtype=np.float32)
UNK_SCORE = -4.25
# what the texts are drawn from: pattern letters, whitespace, upper case, punctuation, a digit, a contraction, characters of two and
# three bytes (an accent the normalizer strips, an ideograph it pads)
RICH = [b"a", b"b", b"c", b"ab", b"abc", b"cab", b"aa", b" ", b"  ", b"\n", b"un", b"able", b"s", b"!", b"A", b"Cab", "É".encode(), "中".encode(),
        b"7", b"'s", b"x", "é".encode()]
SPARSE = [b"x", b"y", b"z", b" ", b"\n"] * 12 + [b"abc", b"aa"]    # few merges: the BPE definition takes merges x length steps
WORDS = [b"a", b"b", b"c", b"un", b"able", b"s", b"x", b"ab", b"aa", b"!"]
ASCII = [b"a", b"b", b"c", b" ", b"  ", b"\n", b"un", b"!", b"A", b"7", b"\t"]
# 16 documents of 0 .. 300 bytes, empty ones at the front, in the middle and at the end, and one beyond batch_lane_max = 300
LENS = [0, 0, 37, 300, 1, 0, 299, 150, 1203, 16, 0, 255, 64, 17, 128, 0, 0]
LANE_MAX = 300
# "un" is a pattern and neither letter is one alone, so overlapping, standard and leftmost scans all report it where they see it
FRONT = b"z" * 12 + b"u"         # 13 bytes: offsets[0] is off a 16-byte boundary; "u" + the first document's "n" reads un
TAIL = b"n" + b"z" * 18          # the last document ends with "u": un again across offsets[n]
SINGLE = 8192 + 17
ALL_RULES = (Split.Whitespace, Split.Gpt2, Split.Cl100k, Split.Llama3, Split.Bert)


# ------------------------------------------------------------------------------------------------------------------ the data
def _text(rng, n, pieces):
    out = bytearray()
    while len(out) < n:
        out += pieces[int(rng.integers(len(pieces)))]
    return bytes(out[:n])


def _utf8_text(rng, n):
    """n bytes of whole characters of one, two and three bytes; from two bytes on, "n" first and "u" last"""
    chars = ["a", "b", "c", "é", "世", "界", "全", " "]
    if n < 2:
        return b"a" * n
    out = bytearray(b"n")
    while n - 1 - len(out) >= 3:
        out += chars[int(rng.integers(len(chars)))].encode()
    return bytes(out + b"a" * (n - 1 - len(out)) + b"u")


def _edges(docs):
    """the first non-empty document starts with "n" and the last one ends with "u" """
    docs = list(docs)
    first = next(i for i, d in enumerate(docs) if len(d))
    last = max(i for i, d in enumerate(docs) if len(d))
    assert first < last
    docs[first] = b"n" + docs[first][1:]
    docs[last] = docs[last][:-1] + b"u"
    return docs


def _docs(seed, lens, pieces):
    rng = np.random.default_rng(seed)
    if pieces is None:
        return [_utf8_text(rng, n) for n in lens]
    return _edges([_text(rng, n, pieces) for n in lens])


def _arrays(docs, front=FRONT, tail=TAIL):
    """(buffer, offsets) of a device batch as numpy arrays: `front`, the documents, `tail`"""
    off = np.full(len(docs) + 1, len(front), dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    return np.frombuffer(front + b"".join(docs) + tail, dtype=np.uint8).copy(), off


def _pair_docs(seed, pieces=RICH, lens=LENS):
    """-> (real documents, decoy documents): the decoy has the lengths in another order and other text, the same n and total"""
    real = _docs(seed, lens, pieces)
    decoy = _docs(seed + 1000, lens[5:] + lens[:5], pieces)
    assert len(decoy) == len(real) and sum(map(len, decoy)) == sum(map(len, real))
    (hay_r, off_r), (hay_d, off_d) = _arrays(real), _arrays(decoy)
    assert off_r[0] == off_d[0] != 0 and off_r[-1] == off_d[-1] < len(hay_r) == len(hay_d)
    assert not np.array_equal(off_r, off_d) and not np.array_equal(hay_r, hay_d) and np.all(np.diff(off_d) >= 0)
    return real, decoy


def _split(hay, off):
    b = hay.tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def _sev(m):
    return list(zip(m["start"].tolist(), m["end"].tolist(), m["value"].tolist()))


def _pair(patterns, kind=0, charwise=False):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p


class _World:
    """the handles, oracles and tables every test of this file shares"""

    def __init__(self, fresh=False):
        self.o, self.p = _pair(PATS)                       # Standard
        self.ol, self.pl = _pair(PATS, kind=1)             # LeftmostLongest
        for p in (self.p, self.pl):
            p.set_option("batch_lane_max", LANE_MAX)
        self.p.set_option("bpe_doc_max", 16384)
        self.slots = _Slots(self.o)
        cpats = ["全世界", "世界", "界", "a", "é世", "ab", "un"]
        self.co, self.cp = _pair(cpats, charwise=True)
        self.col, self.cpl = _pair(cpats, kind=1, charwise=True)
        for p in (self.cp, self.cpl):
            p.set_option("batch_lane_max", LANE_MAX)
        self.ctable = ["〈%d〉" % i for i in range(len(cpats))]
        # WordPiece: a lower-case vocabulary, and four pieces of 4096 bytes that make the single 8 KiB word cheap for the definition
        rng = np.random.default_rng(99)
        self.long = [_text(rng, 4096, [b"p", b"q"]) for _ in range(4)]
        vocab = {"[UNK]": 0, "un": 1, "##able": 2, "able": 3, "##s": 4, "s": 5, "a": 6, "##a": 7, "b": 8, "##b": 9, "c": 10, "##c": 11, "ab": 12, "##ab": 13,
                 "abc": 14, "##bc": 15, "x": 16, "##x": 17, "!": 18, "7": 19, "##7": 20, "'": 21, "e": 22, "##e": 23, "中": 24, "cab": 25, "##un": 26, "aa": 27}
        self.vocab = {k.encode(): i for k, i in vocab.items()}
        self.vocab.update({self.long[0]: 30, b"##" + self.long[1]: 31, self.long[2]: 32, b"##" + self.long[3]: 33})
        patterns, self.first, self.cont = da.wordpiece_tables(self.vocab)
        self.wp = da.DoubleArrayAhoCorasick.new(patterns)
        self.cc = da.char_classes()
        self.bert_table = wg.class_table(da.bert_char_classes())
        self.splitters = {r: da.Splitter(r, da.bert_char_classes() if r == Split.Bert else None) for r in ALL_RULES}
        self.nz = da.bert_normalizer()
        if fresh:   # bert_normalizer()'s rules in a normalizer that has uploaded nothing yet
            self.nz = da.Normalizer(self.nz.rules, self.nz.pool)

    def handle(self, kind):
        return (self.o, self.p, "find_iter", ScanMode.Find) if kind == "standard" else (self.ol, self.pl, "leftmost_find_iter", ScanMode.LeftmostFind)

    def split_want(self, docs, rule, base):
        if rule in (Split.Whitespace, Split.Gpt2):
            return split_scan_batch(docs, rule, self.cc, base)
        if rule == Split.Bert:
            return wg.bert_offsets(docs, self.bert_table, base)[:2]
        return scan_rule_batch(docs, rule, self.cc, base)


@pytest.fixture(scope="module")
def world():
    return _World()


# ------------------------------------------------------------------------------------------------------------------ the delay
class _Delay:
    """about DELAY_MS of device time queued on the current stream: torch.cuda._sleep, its unit calibrated with two events (this times
    torch's helper, not the library); a chain of matrix products of the same measured length where _sleep does not delay"""

    def __init__(self):
        probe = 20_000_000
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        ms = self._time(lambda: torch.cuda._sleep(probe))
        self.cycles_per_ms = probe / ms if ms > 0 else float("inf")
        self.cycles, self.reps = None, 0
        if 1.0 <= ms <= 10_000.0:
            self.cycles = int(self.cycles_per_ms * DELAY_MS)
            self.measured_ms = self._time(self.queue)
        else:   # _sleep is no delay here
            self.a = torch.ones((2048, 2048), device="cuda")
            self.a @ self.a
            one = self._time(lambda: [self.a @ self.a for _ in range(20)]) / 20
            self.reps = max(1, int(np.ceil(DELAY_MS / one)))
            self.measured_ms = self._time(self.queue)
        print(f"\n[streams] _sleep: {self.cycles_per_ms:.0f} cycles per ms; delay = {self.cycles} cycles / {self.reps} products, measured {self.measured_ms:.1f} ms")

    @staticmethod
    def _time(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def queue(self, ms=DELAY_MS):
        if self.cycles is not None:
            torch.cuda._sleep(int(self.cycles * ms / DELAY_MS))
        else:
            for _ in range(max(1, int(self.reps * ms / DELAY_MS))):
                self.a @ self.a


@pytest.fixture(scope="module")
def delay():
    gc.collect()   # the handles and results that earlier modules left in reference cycles go now (see _no_collection)
    d = _Delay()
    assert d.measured_ms >= 0.6 * DELAY_MS, f"the delay lasts {d.measured_ms:.1f} ms, not about {DELAY_MS} ms"
    return d


def _h(s):
    return None if s is None else s.cuda_stream


def _read(t, s):
    """a device tensor's values through a copy queued on s (None: the null stream)"""
    if s is None:
        return t.cpu().numpy()
    host = torch.empty(t.shape, dtype=t.dtype).pin_memory()
    with torch.cuda.stream(s):
        host.copy_(t, non_blocking=True)
    s.synchronize()
    return host.numpy()


@contextlib.contextmanager
def _no_collection():
    """No cyclic garbage collection inside: a handle, a match list or a device result of an earlier test that the collector finds is
    freed with hipFree / hipHostFree, which wait for the whole device, the pending delay included.  The host would sit out the delay
    and whatever it did next would see the real inputs: the run would prove nothing (or, in test_control, fail)."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _tick(stream):
    """a tiny kernel on `stream` (None: the null stream), waited for"""
    if stream is None:
        torch.zeros(1, device="cuda").add_(1)
        torch.cuda.default_stream().synchronize()
    else:
        with torch.cuda.stream(stream):
            torch.zeros(1, device="cuda").add_(1)
        stream.synchronize()


def _fresh_stream(delay, apart_from=(None,)):
    """torch.cuda.Stream() that does not share a hardware queue with the streams of `apart_from` (None: the null stream).  A process has
    few hardware queues (GPU_MAX_HW_QUEUES) and streams are dealt onto them in turn: work on two streams of one queue runs in the order
    it was submitted, and a delay on one would hold up the other.  The probe: 5 ms of delay on the candidate, a tiny kernel on each of
    the others, and the candidate must still be busy.  This is as far as the harness reaches: a step that the library put on some third
    stream which happens to share the candidate's queue would wait behind the delay and go unnoticed; a step on the null stream, which is
    what a dropped or forgotten `stream` argument gives, does not."""
    for _ in range(16):
        s = torch.cuda.Stream()
        with _no_collection():
            with torch.cuda.stream(s):
                delay.queue(5.0)
            for other in apart_from:
                _tick(other)
            apart = not s.query()
        s.synchronize()
        if apart:
            return s
    pytest.fail("none of 16 fresh streams runs apart from the null stream: the ordered runs could prove nothing")


def _pending(delay, decoys, reals):
    """the decoys in device memory and a fresh stream with the delay and the copies of the real inputs queued -> (stream, tensors)"""
    dev = [torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in decoys]
    pinned = [torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory() for a in reals]
    for d, r in zip(decoys, reals):
        assert d.shape == r.shape and d.dtype == r.dtype
    s = _fresh_stream(delay)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay.queue()
        for t, h in zip(dev, pinned):
            t.copy_(h, non_blocking=True)
    return s, dev, pinned


def _ordered(delay, real, decoy, call, want, in_place=()):
    """One call, ordered after the caller's work.  `real` / `decoy`: the call's device inputs as numpy arrays; call(s, *tensors) makes the
    call on torch stream s (None: the null stream) and returns plain values; want(*arrays) is the reference.  The decoy's result on the
    null stream doubles as the warm-up.  `in_place`: the inputs that the call rewrites (every other one must come back unchanged)."""
    w_real, w_decoy = want(*real), want(*decoy)
    assert w_real != w_decoy, "the decoy has the real input's result: the run could prove nothing"
    warm = [torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in decoy]
    assert call(None, *warm) == w_decoy, "the decoy on the null stream"
    with _no_collection():
        s, dev, pinned = _pending(delay, decoy, real)
        try:
            assert not s.query(), "the delay had drained before the call was made: the run proved nothing"
            got = call(s, *dev)
        finally:
            s.synchronize()
    assert got == w_real, "the call on a stream with the caller's copies pending in front of it"
    for i, (t, a) in enumerate(zip(dev, real)):   # the inputs are the caller's: the real ones, unchanged
        assert i in in_place or np.array_equal(t.cpu().numpy(), a)


def _dev_result(parts):
    """DeviceMatches / DeviceOffsets -> plain values, freed"""
    try:
        return [_plain(x.to_numpy()) for x in parts]
    finally:
        for x in parts:
            x.free()


def _plain(x):
    if isinstance(x, np.ndarray):
        if x.dtype.names and "start" in x.dtype.names:
            return _sev(x)
        if x.dtype.names and "length" in x.dtype.names:      # 16-byte tuples
            return list(zip((x["end"] - x["length"].astype(np.uint64)).tolist(), x["end"].tolist(), x["value"].tolist()))
        if x.dtype.names:
            return [tuple(r) for r in x.tolist()]
        if x.dtype == np.float32:
            return x.view(np.uint32).tolist()                 # scores compare bit for bit
        return x.tolist()
    if isinstance(x, np.float32):
        return int(np.asarray(x).reshape(1).view(np.uint32)[0])
    if isinstance(x, (tuple, list)):
        return [_plain(y) for y in x]
    return x


# -------------------------------------------------------------------------------------------------------------------- control
def test_control(delay):
    """the harness itself: while s holds the delay and the copy, the null stream and a second fresh stream both still read the decoy"""
    decoy = np.full(1 << 16, 1, dtype=np.uint8)
    real = np.full(1 << 16, 3, dtype=np.uint8)
    t = torch.from_numpy(decoy.copy()).cuda()
    pinned = torch.from_numpy(real.copy()).pin_memory()
    gc.collect()   # what earlier tests left behind is freed now, not under the delay
    s = _fresh_stream(delay)
    other = _fresh_stream(delay, apart_from=(None, s))
    for st in (torch.cuda.default_stream(), other):   # the reduction's first launch, and its result's first allocation, not under the delay
        with torch.cuda.stream(st):
            torch.ones(1 << 16, dtype=torch.uint8, device="cuda").sum(dtype=torch.int64)
    torch.cuda.synchronize()
    with _no_collection():
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            delay.queue()
            t.copy_(pinned, non_blocking=True)
        try:
            assert not s.query(), "the delay had drained at once"
            on_null = t.sum(dtype=torch.int64)
            torch.cuda.default_stream().synchronize()
            busy_after_null, ms_null = not s.query(), 1e3 * (time.perf_counter() - t0)
            with torch.cuda.stream(other):
                on_other = t.sum(dtype=torch.int64)
            other.synchronize()
            still, ms_other = not s.query(), 1e3 * (time.perf_counter() - t0)
        finally:
            s.synchronize()
    on_null, on_other = int(on_null.item()), int(on_other.item())
    # what a failure was: host times far below the delay with s no longer busy say a stream waited for s; host times near the delay say
    # the host was held up and the run proved nothing
    seen = (f"null stream read {on_null} after {ms_null:.1f} ms (s busy then: {busy_after_null}), second stream read {on_other} after "
            f"{ms_other:.1f} ms (s busy then: {still}); the decoy sums to {decoy.size}, the delay is {delay.measured_ms:.1f} ms")
    assert on_null == decoy.size and busy_after_null, "a read on the null stream waited for s, or the host was held up: " + seen
    assert on_other == decoy.size and still, "a read on a second stream waited for s, or the host was held up: " + seen
    assert int(t.sum(dtype=torch.int64).item()) == 3 * decoy.size


# ------------------------------------------------------------------------------------------------------- one haystack, ordered
def _single_pair(seed, pieces=RICH):
    rng = np.random.default_rng(seed)
    real, decoy = _text(rng, SINGLE, pieces), _text(rng, SINGLE, pieces)
    return [np.frombuffer(real, dtype=np.uint8)], [np.frombuffer(decoy, dtype=np.uint8)]


def _hist_dense(w, m):
    dense = [0] * w.slots.n
    for slot, c in w.slots.rows(m):
        dense[slot] = c
    return dense


def _single_cases():
    """name -> (seed or input maker, call(w, s, t), want(w, text bytes))"""
    c = {}
    ov = ScanMode.FindOverlapping
    c["count"] = (1, lambda w, s, t: w.p.count(ov, t, stream=_h(s)), lambda w, x: len(w.o.find_overlapping_iter(x)))
    c["scan_count"] = (2, lambda w, s, t: list(w.p.scan_count(ov, t, stream=_h(s))),
                       lambda w, x: [len(w.o.find_overlapping_iter(x)), orc.matches_checksum(w.o.find_overlapping_iter(x))])
    for kind in ("standard", "leftmost"):
        def scan(w, s, t, kind=kind):
            return _sev(w.handle(kind)[1].scan(w.handle(kind)[3], t, stream=_h(s)))

        def scan_device(w, s, t, kind=kind):
            return _dev_result([w.handle(kind)[1].scan_device(w.handle(kind)[3], t, stream=_h(s))])[0]

        def chain(w, x, kind=kind):
            return _sev(getattr(w.handle(kind)[0], w.handle(kind)[2])(x))

        def replace(w, s, t, kind=kind):
            return w.handle(kind)[1].replace_all(t, TABLE, stream=_h(s))

        def replace_want(w, x, kind=kind):
            return _splice(x, getattr(w.handle(kind)[0], w.handle(kind)[2])(x), TABLE)

        def tokenize(w, s, t, kind=kind):
            return _plain(w.handle(kind)[1].tokenize(t, gap=Gap.Bytes, gap_id=GID, spans=True, stream=_h(s)))

        def tokenize_want(w, x, kind=kind):
            return _plain(_tokens(x, getattr(w.handle(kind)[0], w.handle(kind)[2])(x), Gap.Bytes, GID))

        c[f"scan-{kind}"] = (3, scan, chain)
        c[f"scan_device-{kind}"] = (4, scan_device, chain)
        c[f"replace_all-{kind}"] = (5, replace, replace_want)
        c[f"tokenize-{kind}"] = (6, tokenize, tokenize_want)
    c["scan-overlapping"] = (7, lambda w, s, t: _sev(w.p.scan(ov, t, stream=_h(s))), lambda w, x: _sev(w.o.find_overlapping_iter(x)))

    def histogram(w, s, t):
        out = torch.zeros(w.slots.n, dtype=torch.int64, device="cuda")
        torch.cuda.default_stream().synchronize()
        assert w.p.histogram(ov, t, stream=_h(s), out=out) is None
        return _read(out, s).tolist()
    c["histogram"] = (8, histogram, lambda w, x: _hist_dense(w, w.o.find_overlapping_iter(x)))

    def unigram_want(w, x):
        toks, score = _viterbi(x, w.o.find_overlapping_iter(x), SCORES, np.float32(UNK_SCORE), Gap.Chars, GID)
        return [[t[0] for t in toks], [[t[1], t[2]] for t in toks], _plain(score)]
    c["tokenize_unigram"] = (9, lambda w, s, t: _plain(w.p.tokenize_unigram(t, SCORES, UNK_SCORE, gap=Gap.Chars, gap_id=GID, spans=True, stream=_h(s))), unigram_want)

    def bpe_want(w, x):
        toks = _bpe(x, w.o.find_overlapping_iter(x), None, Gap.Bytes, GID)
        return [[t[0] for t in toks], [[t[1], t[2]] for t in toks]]
    c["tokenize_bpe"] = ("sparse", lambda w, s, t: _plain(w.p.tokenize_bpe(t, gap=Gap.Bytes, gap_id=GID, spans=True, stream=_h(s))), bpe_want)

    def wordpiece_want(w, x):
        toks = wg.wordpiece(x, w.vocab, 0, 10000)
        return [[t[0] for t in toks], [[t[1], t[2]] for t in toks]]
    c["tokenize_wordpiece"] = ("word", lambda w, s, t: _plain(w.wp.tokenize_wordpiece(t, w.first, w.cont, 0, max_chars=10000, spans=True, stream=_h(s))),
                               wordpiece_want)

    def normalize_want(w, x):
        out, src = ng.bert_scan(x, ng.OPTIONS["default"])
        return [list(out), src]
    c["normalize"] = (10, lambda w, s, t: _plain(w.nz.normalize(t, src=True, stream=_h(s))), normalize_want)
    for rule in ALL_RULES:
        c[f"split-{rule.name}"] = (11, lambda w, s, t, rule=rule: _plain(w.splitters[rule].split(t, stream=_h(s))),
                                   lambda w, x, rule=rule: w.split_want([x], rule, 0)[0].tolist())

    def find_iter(w, s, t):
        it = w.p.find_iter(t, stream=_h(s))
        try:
            return [(m.start(), m.end(), m.value()) for m in it]
        finally:
            it.close()
    c["find_iter"] = (12, find_iter, lambda w, x: _sev(w.o.find_iter(x)))

    def stepper(w, s, t):
        st = w.p.find_overlapping_stepper(stream=_h(s))
        got = []
        for a, b in ((0, 3001), (3001, 3017), (3017, SINGLE)):   # device chunks: views of the caller's tensor
            got += _sev(st.feed(t[a:b]))
        return got
    c["stepper"] = (13, stepper, lambda w, x: _sev(w.o.find_overlapping_stepper(x)))
    return c


SINGLE_CASES = _single_cases()


@pytest.mark.parametrize("name", sorted(SINGLE_CASES))
def test_one_haystack_is_ordered_after_the_callers_copy(world, delay, name):
    seed, call, want = SINGLE_CASES[name]
    if seed == "sparse":
        real, decoy = _single_pair(77, SPARSE)
    elif seed == "word":
        rng = np.random.default_rng(5)
        tails = [_text(rng, 17, [b"a", b"b", b"c", b"x", b"s"]) for _ in range(2)]
        real = [np.frombuffer(world.long[0] + world.long[1] + tails[0], dtype=np.uint8)]
        decoy = [np.frombuffer(world.long[2] + world.long[3] + tails[1], dtype=np.uint8)]
    else:
        real, decoy = _single_pair(seed)
    assert real[0].size == decoy[0].size == SINGLE
    _ordered(delay, real, decoy, lambda s, t: call(world, s, t), lambda a: want(world, a.tobytes()))


# --------------------------------------------------------------------------------------------------------- batches, ordered
def _per_doc(fn, hay, off):
    return [fn(d) for d in _split(hay, off)]


def _csr(per_doc):
    return [x for d in per_doc for x in d], np.cumsum([0] + [len(d) for d in per_doc]).tolist()


def _tok_lists(per_doc):
    """[[(id, start, end)]] -> [ids, spans, offsets]"""
    flat, off = _csr(per_doc)
    return [[t[0] for t in flat], [[t[1], t[2]] for t in flat], off]


def _wordpiece_docs_want(w, docs, normalize):
    per_doc = []
    for d in docs:
        text, src = ng.bert_scan(d, ng.OPTIONS["default"]) if normalize else (d, None)
        ids, spans = wg.wordpiece_doc(text, w.bert_table, w.vocab, 0, 100)
        if normalize:
            spans = ng.spans_to_source(spans, src, d)
        per_doc.append([(i, a, b) for i, (a, b) in zip(ids, spans)])
    return _tok_lists(per_doc)


def _bpe_docs_want(w, docs):
    per_doc = []
    for d in docs:
        wo, _ = split_scan_batch([d], Split.Gpt2, w.cc, 0)
        toks = []
        for a, b in zip(wo[:-1].tolist(), wo[1:].tolist()):
            toks += [(i, a + x, a + y) for i, x, y in _bpe(d[a:b], w.o.find_overlapping_iter(d[a:b]), None, Gap.Bytes, GID)]
        per_doc.append(toks)
    return _tok_lists(per_doc)


def _batch_cases():
    """name -> (pieces, call(w, s, hay, off[, more]), want(w, hay, off[, more]), extra inputs or None)"""
    c = {}
    for kind, modes in (("standard", (ScanMode.FindOverlapping, ScanMode.Find)), ("leftmost", (ScanMode.LeftmostFind,))):
        for mode in modes:
            api = {ScanMode.FindOverlapping: "find_overlapping_iter", ScanMode.Find: "find_iter", ScanMode.LeftmostFind: "leftmost_find_iter"}[mode]
            tag = f"{kind}-{mode.name}"

            def matches(w, hay, off, kind=kind, api=api):
                return _per_doc(lambda d: getattr(w.handle(kind)[0], api)(d), hay, off)

            def count(w, s, hay, off, kind=kind, mode=mode):
                return w.handle(kind)[1].count_batch(mode, (hay, off), stream=_h(s)).tolist()

            def scan_count(w, s, hay, off, kind=kind, mode=mode):
                n = off.numel() - 1
                cnt, cs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
                torch.cuda.default_stream().synchronize()
                assert w.handle(kind)[1].scan_count_batch(mode, (hay, off), stream=_h(s), out=(cnt, cs)) is None
                return [_read(cnt, s).astype(np.uint64).tolist(), _read(cs, s).astype(np.uint64).tolist()]

            def scan(w, s, hay, off, kind=kind, mode=mode):
                return _plain(w.handle(kind)[1].scan_batch(mode, (hay, off), stream=_h(s)))

            def scan_device(w, s, hay, off, kind=kind, mode=mode):
                return _dev_result(w.handle(kind)[1].scan_batch_device(mode, (hay, off), stream=_h(s)))

            def scan_want(w, hay, off, matches=matches):
                flat, o = _csr([_sev(m) for m in matches(w, hay, off)])
                return [flat, o]

            c[f"count_batch-{tag}"] = (RICH, count, lambda w, hay, off, matches=matches: [len(m) for m in matches(w, hay, off)], None)
            c[f"scan_count_batch-{tag}"] = (RICH, scan_count, lambda w, hay, off, matches=matches: [[len(m) for m in matches(w, hay, off)],
                                                                                                   [orc.matches_checksum(m) for m in matches(w, hay, off)]], None)
            c[f"scan_batch-{tag}"] = (RICH, scan, scan_want, None)
            c[f"scan_batch_device-{tag}"] = (RICH, scan_device, scan_want, None)

        def chain(w, hay, off, kind=kind):
            return _per_doc(lambda d: (d, getattr(w.handle(kind)[0], w.handle(kind)[2])(d)), hay, off)

        def replace(w, s, hay, off, kind=kind):
            return w.handle(kind)[1].replace_all_batch((hay, off), TABLE, stream=_h(s))

        def replace_device(w, s, hay, off, kind=kind):
            out, o = _dev_result(w.handle(kind)[1].replace_all_batch((hay, off), TABLE, stream=_h(s), device=True))
            return [bytes(out[a:b]) for a, b in zip(o, o[1:])]

        def tokenize(w, s, hay, off, kind=kind):
            return _plain(w.handle(kind)[1].tokenize_batch((hay, off), gap=Gap.Chars, gap_id=GID, spans=True, stream=_h(s)))

        def tokenize_want(w, hay, off, chain=chain):
            per_doc = []
            for d, m in chain(w, hay, off):
                ids, sp = _tokens(d, m, Gap.Chars, GID)
                per_doc.append([(i, a, b) for i, (a, b) in zip(ids.tolist(), sp.tolist())])
            return _tok_lists(per_doc)

        c[f"replace_all_batch-{kind}"] = (RICH, replace, lambda w, hay, off, chain=chain: [_splice(d, m, TABLE) for d, m in chain(w, hay, off)], None)
        c[f"replace_all_batch_device-{kind}"] = (RICH, replace_device, lambda w, hay, off, chain=chain: [_splice(d, m, TABLE) for d, m in chain(w, hay, off)], None)
        c[f"tokenize_batch-{kind}"] = (RICH, tokenize, tokenize_want, None)

    def hist_want(w, hay, off):
        flat, o = _csr(_per_doc(lambda d: w.slots.rows(w.o.find_overlapping_iter(d)), hay, off))
        return [flat, o]
    c["histogram_batch"] = (RICH, lambda w, s, hay, off: _plain(w.p.histogram_batch(ScanMode.FindOverlapping, (hay, off), stream=_h(s))), hist_want, None)
    c["histogram_batch_device"] = (RICH, lambda w, s, hay, off: _dev_result(w.p.histogram_batch_device(ScanMode.FindOverlapping, (hay, off), stream=_h(s))),
                                   hist_want, None)

    def unigram_want(w, hay, off):
        res = _per_doc(lambda d: _viterbi(d, w.o.find_overlapping_iter(d), SCORES, np.float32(UNK_SCORE), Gap.Chars, GID), hay, off)
        ids, _, o = _tok_lists([t for t, _ in res])
        return [ids, o, [_plain(sc) for _, sc in res]]
    c["tokenize_unigram_batch"] = (RICH, lambda w, s, hay, off: _plain(w.p.tokenize_unigram_batch((hay, off), SCORES, UNK_SCORE, gap=Gap.Chars, gap_id=GID,
                                                                                                  doc_scores=True, stream=_h(s))), unigram_want, None)

    def bpe_want(w, hay, off):
        ids, _, o = _tok_lists(_per_doc(lambda d: _bpe(d, w.o.find_overlapping_iter(d), None, Gap.Bytes, GID), hay, off))
        return [ids, o]
    c["tokenize_bpe_batch"] = (RICH, lambda w, s, hay, off: _plain(w.p.tokenize_bpe_batch((hay, off), gap=Gap.Bytes, gap_id=GID, stream=_h(s))), bpe_want, None)
    c["tokenize_bpe_docs"] = (RICH, lambda w, s, hay, off: _plain(w.p.tokenize_bpe_docs((hay, off), gap=Gap.Bytes, gap_id=GID, spans=True, stream=_h(s))),
                              lambda w, hay, off: _bpe_docs_want(w, _split(hay, off)), None)

    def wp_batch(w, s, hay, off, skip):
        return _plain(w.wp.tokenize_wordpiece_batch((hay, off), w.first, w.cont, 0, max_chars=400, skip=skip, spans=True, stream=_h(s)))

    def wp_batch_want(w, hay, off, skip):
        return _tok_lists([[] if k else wg.wordpiece(d, w.vocab, 0, 400) for d, k in zip(_split(hay, off), skip.tolist())])
    c["tokenize_wordpiece_batch"] = (WORDS, wp_batch, wp_batch_want, "skip")
    for normalize in (False, True):
        def wp_docs(w, s, hay, off, normalize=normalize):
            return _plain(w.wp.tokenize_wordpiece_docs((hay, off), w.first, w.cont, 0, spans=True, stream=_h(s), normalizer=w.nz if normalize else None))
        c["tokenize_wordpiece_docs" + ("-normalizer" if normalize else "")] = (
            RICH, wp_docs, lambda w, hay, off, normalize=normalize: _wordpiece_docs_want(w, _split(hay, off), normalize), None)
    for rule in ALL_RULES:
        c[f"split_batch-{rule.name}"] = (RICH, lambda w, s, hay, off, rule=rule: _plain(w.splitters[rule].split_batch((hay, off), stream=_h(s))),
                                         lambda w, hay, off, rule=rule: [x.tolist() for x in w.split_want(_split(hay, off), rule, int(off[0]))], None)

    def normalize_want(w, hay, off):
        res = _per_doc(lambda d: ng.bert_scan(d, ng.OPTIONS["default"]), hay, off)
        return [list(b"".join(o for o, _ in res)), np.cumsum([0] + [len(o) for o, _ in res]).tolist(), [x for _, sr in res for x in sr]]
    c["normalize_batch"] = (RICH, lambda w, s, hay, off: _plain(w.nz.normalize_batch((hay, off), src=True, stream=_h(s))), normalize_want, None)
    return c


BATCH_CASES = _batch_cases()


def test_a_pattern_matches_across_both_ends_of_the_batch(world):
    """the layout every batch of this file has: scanning the whole buffer finds un across offsets[0] and across offsets[n]; the matches
    inside the documents are exactly what the per-document reference reports"""
    for docs in _pair_docs(21):
        hay, off = _arrays(docs)
        assert off[0] == len(FRONT) and off[0] % 16 != 0 and off[-1] + len(TAIL) == len(hay)
        whole = world.o.find_overlapping_iter(hay.tobytes())
        s, e = whole["start"].astype(np.int64), whole["end"].astype(np.int64)
        assert np.any((s < off[0]) & (e > off[0])) and np.any((s < off[-1]) & (e > off[-1]))
        doc_of = np.searchsorted(off, s, side="right") - 1
        inside = (s >= off[0]) & (e <= off[-1])
        inside[inside] &= e[inside] <= off[np.minimum(doc_of[inside] + 1, len(off) - 1)]
        assert int(inside.sum()) == sum(len(world.o.find_overlapping_iter(d)) for d in docs) < len(whole)


@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_a_batch_is_ordered_after_the_callers_copy(world, delay, name):
    pieces, call, want, extra = BATCH_CASES[name]
    real_docs, decoy_docs = _pair_docs(100 + sorted(BATCH_CASES).index(name), pieces)
    real, decoy = list(_arrays(real_docs)), list(_arrays(decoy_docs))
    if extra == "skip":
        rng = np.random.default_rng(3)
        real.append((rng.random(len(LENS)) < 0.3).astype(np.uint8) * 7)
        decoy.append((rng.random(len(LENS)) < 0.3).astype(np.uint8))
        assert not np.array_equal(real[2] != 0, decoy[2] != 0)
    _ordered(delay, real, decoy, lambda s, *t: call(world, s, *t), lambda *a: want(world, *a))


def test_words_space_is_ordered_after_the_callers_copy(world, delay):
    """(hay, word_offsets): the real word offsets are the Split.Bert reference's; the decoy has as many words at other places"""
    real_docs, decoy_docs = _pair_docs(300, ASCII)
    (hay_r, off_r), (hay_d, _) = _arrays(real_docs), _arrays(decoy_docs)
    wo_r, _, flags = wg.bert_offsets(real_docs, world.bert_table, int(off_r[0]))
    rng = np.random.default_rng(8)
    wo_d = np.sort(rng.integers(int(off_r[0]), int(off_r[-1]) + 1, size=len(wo_r))).astype(np.int64)
    wo_d[0], wo_d[-1] = off_r[0], off_r[-1]

    def want(hay, wo):   # 1: the word is not empty and begins with whitespace (the text is ASCII)
        return [int(b > a and hay[a] in b" \t\n\r\x0b\x0c") for a, b in zip(wo[:-1].tolist(), wo[1:].tolist())]
    assert want(hay_r, wo_r.astype(np.int64)) == flags.tolist()
    sp = world.splitters[Split.Bert]
    _ordered(delay, [hay_r, wo_r.astype(np.int64)], [hay_d, wo_d], lambda s, hay, wo: sp.words_space((hay, wo), stream=_h(s)).tolist(), want)


def test_spans_to_source_is_ordered_after_the_callers_copy(world, delay):
    """spans, src, the text and its offsets all come behind the delay.  The decoy keeps tok_offsets and out_offsets (they size the call),
    has every src entry 0, spans that start at 0, text of one-byte characters and other boundaries: valid together with any part of the
    real input"""
    real_docs, _ = _pair_docs(301)
    hay_r, off_r = _arrays(real_docs)
    hay_d, off_d = np.full_like(hay_r, ord("a")), off_r.copy()
    for i in range(1, len(real_docs)):   # other boundaries under which every document that has tokens keeps a byte for src = 0
        if len(real_docs[i - 1]) >= 2:
            off_d[i] -= 1
    assert not np.array_equal(off_d, off_r) and np.all(np.diff(off_d) >= 0)
    spans, src, want, tok_off, out_off = [], [], [], [0], [0]
    for d in real_docs:
        text, sr = ng.bert_scan(d, ng.OPTIONS["default"])
        _, sp = wg.wordpiece_doc(text, world.bert_table, world.vocab, 0, 100)
        spans += sp
        src += sr
        want += ng.spans_to_source(sp, sr, d)
        tok_off.append(len(spans))
        out_off.append(len(src))
    assert len(spans) > 50 and [list(x) for x in want] != [list(x) for x in spans]
    spans_r, src_r = np.array(spans, dtype=np.int64).reshape(-1, 2), np.array(src, dtype=np.int32)   # (uint32 values, as torch has them)
    spans_d = spans_r.copy()
    spans_d[:, 0] = 0
    tok = torch.tensor(tok_off, dtype=torch.int64).cuda()
    oo = torch.tensor(out_off, dtype=torch.int64).cuda()

    def call(s, sp, sr, hay, off):
        da.Normalizer.spans_to_source(sp, tok, oo, sr, (hay, off), stream=_h(s))
        return _read(sp, s).tolist()

    def ref(sp, sr, hay, off):
        docs, out = _split(hay, off), []
        for i, d in enumerate(docs):
            out += ng.spans_to_source([tuple(x) for x in sp[tok_off[i]:tok_off[i + 1]].tolist()], sr[out_off[i]:out_off[i + 1]].tolist(), d)
        return [list(x) for x in out]
    real, decoy = [spans_r, src_r, hay_r, off_r], [spans_d, np.zeros_like(src_r), hay_d, off_d]
    assert ref(*real) == [list(x) for x in want]
    _ordered(delay, real, decoy, call, ref, in_place=(0,))   # (the spans tensor is input and result)


@pytest.mark.parametrize("name", ["scan_batch", "replace_all_batch", "tokenize_batch"])
@pytest.mark.parametrize("kind", ["standard", "leftmost"])
def test_a_charwise_batch_is_ordered_after_the_callers_copy(world, delay, name, kind):
    o, p, api, mode = (world.co, world.cp, "find_iter", ScanMode.Find) if kind == "standard" else (world.col, world.cpl, "leftmost_find_iter", ScanMode.LeftmostFind)
    real_docs, decoy_docs = _pair_docs(400, None)

    def chain(hay, off):
        return [(d, getattr(o, api)(d.decode())) for d in _split(hay, off)]
    if name == "scan_batch":
        call = lambda s, hay, off: _plain(p.scan_batch(mode, (hay, off), stream=_h(s)))
        want = lambda hay, off: list(_csr([_sev(m) for _, m in chain(hay, off)]))
    elif name == "replace_all_batch":
        table = [t.encode() for t in world.ctable]
        call = lambda s, hay, off: p.replace_all_batch((hay, off), world.ctable, stream=_h(s))
        want = lambda hay, off: [_splice(d, m, table) for d, m in chain(hay, off)]
    else:
        call = lambda s, hay, off: _plain(p.tokenize_batch((hay, off), gap=Gap.Chars, gap_id=GID, spans=True, stream=_h(s)))

        def want(hay, off):
            per_doc = []
            for d, m in chain(hay, off):
                ids, sp = _tokens(d, m, Gap.Chars, GID)
                per_doc.append([(i, a, b) for i, (a, b) in zip(ids.tolist(), sp.tolist())])
            return _tok_lists(per_doc)
    _ordered(delay, list(_arrays(real_docs)), list(_arrays(decoy_docs)), call, want)


# ------------------------------------------------------------------------------------ front and tail bytes, on the null stream
@pytest.mark.parametrize("front", [1, 13, 37])
@pytest.mark.parametrize("kind,mode,api", [("standard", ScanMode.FindOverlapping, "find_overlapping_iter"), ("standard", ScanMode.Find, "find_iter"),
                                           ("leftmost", ScanMode.LeftmostFind, "leftmost_find_iter")])
def test_front_and_tail_bytes_belong_to_no_document(world, front, kind, mode, api):
    o, p = world.handle(kind)[:2]
    docs = _docs(500 + front, LENS, RICH)
    lead = (b"z" * 40 + b"u")[-front:]
    hay, off = _arrays(docs, lead, TAIL)
    assert off[0] == front and off[0] % 16 != 0
    whole = getattr(o, api)(hay.tobytes())
    s, e = whole["start"].astype(np.int64), whole["end"].astype(np.int64)
    assert np.any((s < off[0]) & (e > off[0])) and np.any((s < off[-1]) & (e > off[-1])), "no match across the batch's ends to find"
    batch = (torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda())
    ms = [getattr(o, api)(d) for d in docs]
    assert p.count_batch(mode, batch).tolist() == [len(m) for m in ms]
    cnt, cs = p.scan_count_batch(mode, batch)
    assert cnt.tolist() == [len(m) for m in ms] and cs.tolist() == [orc.matches_checksum(m) for m in ms]
    assert _plain(p.scan_batch(mode, batch)) == list(_csr([_sev(m) for m in ms]))
    if mode != ScanMode.FindOverlapping:
        want = [_splice(d, m, TABLE) for d, m in zip(docs, ms)]
        assert p.replace_all_batch(batch, TABLE) == want
        out, o_ = _dev_result(p.replace_all_batch(batch, TABLE, device=True))
        assert bytes(out) == b"".join(want) and o_ == np.cumsum([0] + [len(x) for x in want]).tolist()


# ----------------------------------------------------------------------------------------------- n == 0 on a caller's stream
def test_no_document_on_a_stream_with_work_pending(world, delay):
    """one offset, 0, and no data (the count calls and the plain replace_all_batch: nothing at all) from every batch call, on a stream that
    still holds the caller's delay.  (The branch is kept
    exercised; that its clear is ordered on the stream rests on the code: no test makes that race lose reliably.)"""
    w = world
    hay = torch.from_numpy(np.frombuffer(FRONT + TAIL, dtype=np.uint8).copy()).cuda()
    off = torch.full((1,), len(FRONT), dtype=torch.int64, device="cuda")
    skip = torch.zeros(0, dtype=torch.uint8, device="cuda")
    b = (hay, off)
    calls = {
        "scan_batch": lambda h: w.p.scan_batch(ScanMode.Find, b, stream=h),
        "scan_batch_device": lambda h: _dev_result(w.pl.scan_batch_device(ScanMode.LeftmostFind, b, stream=h)),
        "histogram_batch": lambda h: w.p.histogram_batch(ScanMode.FindOverlapping, b, stream=h),
        "histogram_batch_device": lambda h: _dev_result(w.p.histogram_batch_device(ScanMode.FindOverlapping, b, stream=h)),
        "replace_all_batch device": lambda h: _dev_result(w.p.replace_all_batch(b, TABLE, stream=h, device=True)),
        "tokenize_batch": lambda h: w.pl.tokenize_batch(b, spans=True, stream=h),
        "tokenize_unigram_batch": lambda h: w.p.tokenize_unigram_batch(b, SCORES, UNK_SCORE, spans=True, stream=h),
        "tokenize_bpe_batch": lambda h: w.p.tokenize_bpe_batch(b, spans=True, stream=h),
        "tokenize_bpe_docs": lambda h: w.p.tokenize_bpe_docs(b, spans=True, stream=h),
        "tokenize_wordpiece_batch": lambda h: w.wp.tokenize_wordpiece_batch(b, w.first, w.cont, 0, skip=skip, spans=True, stream=h),
        "tokenize_wordpiece_docs": lambda h: w.wp.tokenize_wordpiece_docs(b, w.first, w.cont, 0, spans=True, stream=h),
        "tokenize_wordpiece_docs-normalizer": lambda h: w.wp.tokenize_wordpiece_docs(b, w.first, w.cont, 0, spans=True, stream=h, normalizer=w.nz),
        "charwise scan_batch": lambda h: w.cp.scan_batch(ScanMode.Find, b, stream=h),
        "charwise tokenize_batch": lambda h: w.cpl.tokenize_batch(b, stream=h),
        # no offsets in these results: nothing at all
        "replace_all_batch": lambda h: [w.p.replace_all_batch(b, TABLE, stream=h)],
        "count_batch": lambda h: [w.p.count_batch(ScanMode.FindOverlapping, b, stream=h)],
        "scan_count_batch": lambda h: w.pl.scan_count_batch(ScanMode.LeftmostFind, b, stream=h),
    }
    no_offsets = ("replace_all_batch", "count_batch", "scan_count_batch")
    for name, call in calls.items():
        with _no_collection():
            s = _fresh_stream(delay)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay.queue()
            assert not s.query(), "the delay had drained before the call was made"
            got = _plain(list(call(s.cuda_stream)))
            s.synchronize()
        assert all(len(x) == 0 for x in (got if name in no_offsets else got[:-1])), (name, got)
        assert name in no_offsets or got[-1] == [0], (name, got)


# ------------------------------------------------------------------------------------------------------------------- threads
THREAD_BYTES = [4 << 10, 9 << 10, 17 << 10, 33 << 10]


def _thread_lens(rng, total):
    lens = [0, 1203] + [int(x) for x in rng.integers(0, 600, size=total // 250)]
    while sum(lens) > total - 2:
        lens.pop()
    return lens + [total - sum(lens), 0]


def test_threads_with_inputs_of_their_own_share_the_handles():
    """four threads, six rounds, each thread its own stream, batch and expected results; the handles, splitters and the normalizer are
    shared and nothing is uploaded before the threads start, so the lazy uploads race as well"""
    w = _World(fresh=True)   # new handles, splitters and normalizer: no tables on the device yet
    rules = ALL_RULES
    work = []
    for tid, total in enumerate(THREAD_BYTES):
        rng = np.random.default_rng(900 + tid)
        docs = _docs(900 + tid, _thread_lens(rng, total), RICH)
        hay, off = _arrays(docs)
        assert sum(map(len, docs)) == total
        hb, base = (hay, off), int(off[0])
        lm = [(d, w.ol.leftmost_find_iter(d)) for d in docs]
        tok = []
        for d, m in lm:
            ids, sp = _tokens(d, m, Gap.Chars, GID)
            tok.append([(i, a, b) for i, (a, b) in zip(ids.tolist(), sp.tolist())])
        ov = [w.o.find_overlapping_iter(d) for d in docs]
        uni = [_viterbi(d, m, SCORES, np.float32(UNK_SCORE), Gap.Chars, GID) for d, m in zip(docs, ov)]
        norm = [ng.bert_scan(d, ng.OPTIONS["default"]) for d in docs]
        want = {
            "scan_batch": list(_csr([_sev(m) for m in ov])),
            "histogram_batch": list(_csr([w.slots.rows(m) for m in ov])),
            "replace_all_batch": [_splice(d, m, TABLE) for d, m in lm],
            "tokenize_batch": _tok_lists(tok),
            "tokenize_unigram_batch": [_tok_lists([t for t, _ in uni])[0], _tok_lists([t for t, _ in uni])[2]],
            "tokenize_bpe_docs": _bpe_docs_want(w, docs),
            "tokenize_wordpiece_docs": _wordpiece_docs_want(w, docs, True),
            "split_batch": {r: [x.tolist() for x in w.split_want(docs, r, base)] for r in rules},
            "normalize_batch": [list(b"".join(o for o, _ in norm)), np.cumsum([0] + [len(o) for o, _ in norm]).tolist()],
        }
        n_tok = {"tokenize": len(want["tokenize_batch"][0]), "unigram": len(want["tokenize_unigram_batch"][0]), "wordpiece": len(want["tokenize_wordpiece_docs"][0]),
                 "bpe": len(want["tokenize_bpe_docs"][0])}
        work.append((hb, want, n_tok, len(docs), total))
    assert len({len(x[1]["scan_batch"][0]) for x in work}) == len(work)
    errors = []
    start = threading.Barrier(len(work))

    def worker(tid):
        try:
            (hay, off), want, n_tok, n, total = work[tid]
            b = (torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda())
            torch.cuda.current_stream().synchronize()
            s = torch.cuda.Stream()
            h = s.cuda_stream
            start.wait()
            for rep in range(6):
                assert _plain(w.p.scan_batch(ScanMode.FindOverlapping, b, stream=h)) == want["scan_batch"], "scan_batch"
                assert da.last_kernel().startswith("batch "), da.last_kernel()
                assert _plain(w.p.histogram_batch(ScanMode.FindOverlapping, b, stream=h)) == want["histogram_batch"], "histogram_batch"
                assert da.last_kernel().startswith("batch_hist "), da.last_kernel()
                assert w.pl.replace_all_batch(b, TABLE, stream=h) == want["replace_all_batch"], "replace_all_batch"
                assert da.last_kernel().startswith("replace matches=") and f" out={sum(map(len, want['replace_all_batch']))} " in da.last_kernel(), da.last_kernel()
                assert _plain(w.pl.tokenize_batch(b, gap=Gap.Chars, gap_id=GID, spans=True, stream=h)) == want["tokenize_batch"], "tokenize_batch"
                assert f" tokens={n_tok['tokenize']} " in da.last_kernel() and da.last_kernel().startswith("tokenize "), da.last_kernel()
                assert _plain(w.p.tokenize_unigram_batch(b, SCORES, UNK_SCORE, gap=Gap.Chars, gap_id=GID, stream=h)) == want["tokenize_unigram_batch"], "unigram"
                assert da.last_kernel().startswith(f"unigram docs={n} ") and f" tokens={n_tok['unigram']} " in da.last_kernel(), da.last_kernel()
                assert _plain(w.p.tokenize_bpe_docs(b, gap=Gap.Bytes, gap_id=GID, spans=True, stream=h)) == want["tokenize_bpe_docs"], "tokenize_bpe_docs"
                assert da.last_kernel().startswith("bpe docs=") and f" tokens={n_tok['bpe']} " in da.last_kernel(), da.last_kernel()   # (docs: the words)
                assert _plain(w.wp.tokenize_wordpiece_docs(b, w.first, w.cont, 0, spans=True, stream=h, normalizer=w.nz)) == want["tokenize_wordpiece_docs"], "wordpiece"
                assert da.last_kernel().startswith("wordpiece docs=") and f" tokens={n_tok['wordpiece']} " in da.last_kernel(), da.last_kernel()
                for r in rules:
                    assert _plain(w.splitters[r].split_batch(b, stream=h)) == want["split_batch"][r], ("split_batch", r)
                    words = len(want["split_batch"][r][0]) - 1
                    assert da.last_kernel().startswith("split rule=") and f" docs={n} bytes={total} words={words} " in da.last_kernel(), da.last_kernel()
                assert _plain(w.nz.normalize_batch(b, stream=h)) == want["normalize_batch"], "normalize_batch"
                assert da.last_kernel().startswith("normalize rules="), da.last_kernel()
        except Exception as e:  # noqa: BLE001
            errors.append((tid, repr(e)[:600]))
            start.abort()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(len(work))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
