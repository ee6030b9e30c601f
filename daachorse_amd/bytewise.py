"""Host-side mirror of the crate's bytewise API over the C ABI.

Same names, argument meaning and error behaviour as reference src/bytewise.rs /
src/bytewise/builder.rs, so the parity tests read like the reference's own tests:

    pma = DoubleArrayAhoCorasick.new(["bcd", "ab", "a"])
    [(m.start(), m.end(), m.value()) for m in pma.find_overlapping_iter("abcd")]

Every scan runs on the MI355X through libdaachorse_amd.so; nothing here computes matches.
"""
import ctypes as C
import enum

import numpy as np

from . import _ffi
from ._ffi import DaachorseError

MATCH_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("value", "<u4"), ("_pad", "<u4")])


class MatchKind(enum.IntEnum):
    """src/lib.rs:324-346"""
    Standard = 0
    LeftmostLongest = 1
    LeftmostFirst = 2


class ScanMode(enum.IntEnum):
    FindOverlapping = 0
    Find = 1
    LeftmostFind = 2
    FindOverlappingNoSuffix = 3


class Engine(enum.IntEnum):
    Auto = 0
    Tiered = 1
    DArray = 2
    Gram = 3
    Pfx = 4


class Gap(enum.IntEnum):
    """daac_gap: what tokenize makes of the text between two matches"""
    Skip = 0    # nothing
    Unk = 1     # one token per non-empty gap
    Bytes = 2   # one token per byte, id = gap_id + the byte
    Chars = 3   # one token per UTF-8 code point (a cut in front of every byte that is no continuation byte)


class Split(enum.IntEnum):
    """daac_split_rule: how split_batch cuts a document into words"""
    Whitespace = 0   # \s+|\S+
    Gpt2 = 1         # GPT-2's pre-tokenizer pattern
    Cl100k = 3       # tiktoken's cl100k_base pattern (2 is reserved)
    Llama3 = 4       # the pattern of Llama-3's tokenizer.json
    Bert = 6         # BERT's pre-tokenizer: whitespace runs, every punctuation character alone, runs of everything else (5 is refused)
    O200k = 8        # tiktoken's o200k_base pattern: case phases, marks, contractions as suffixes (7 is refused)


class Match:
    """src/lib.rs:286-320"""
    __slots__ = ("_s", "_e", "_v")

    def __init__(self, start, end, value):
        self._s, self._e, self._v = int(start), int(end), int(value)

    def start(self):
        return self._s

    def end(self):
        return self._e

    def value(self):
        return self._v

    def __eq__(self, o):
        return isinstance(o, Match) and (self._s, self._e, self._v) == (o._s, o._e, o._v)

    def __repr__(self):
        return f"Match(start={self._s}, end={self._e}, value={self._v})"


def _as_bytes(x):
    if isinstance(x, str):
        return x.encode("utf-8")
    return bytes(x)


class _Haystack:
    """A haystack argument: str/bytes/numpy (host) or a torch CUDA uint8 tensor (device)."""

    def __init__(self, h):
        self.keep = h
        self.is_device = 0
        if hasattr(h, "data_ptr") and hasattr(h, "is_cuda"):  # torch tensor
            if h.dtype.itemsize != 1 or not h.is_contiguous():
                raise DaachorseError(1, "haystack tensor must be contiguous uint8")
            self.ptr, self.len, self.is_device = h.data_ptr(), h.numel(), int(h.is_cuda)
            if self.len == 0:
                self.ptr = None
            return
        if isinstance(h, np.ndarray):
            if h.dtype.itemsize != 1:  # a value cast would scan something else than the caller's bytes
                raise DaachorseError(1, "haystack array must have a 1-byte dtype (uint8)")
            a = np.ascontiguousarray(h).view(np.uint8)
        else:
            a = np.frombuffer(_as_bytes(h), dtype=np.uint8)
        self.keep = a
        self.ptr = a.ctypes.data if a.size else None
        self.len = a.size


class _MatchList:
    """Owns a daac_matches handle and exposes its (page-locked) tuples to numpy without a copy."""

    def __init__(self, handle, n):
        self._h = handle
        ptr = _ffi.lib().daac_matches_data(handle)
        self.__array_interface__ = {"data": (ptr, True), "shape": (n,), "typestr": "|V%d" % MATCH_DTYPE.itemsize,
                                    "descr": MATCH_DTYPE.descr, "version": 3}

    def __del__(self):
        try:
            if self._h:
                _ffi.lib().daac_matches_free(self._h)
                self._h = None
        except Exception:
            pass


MATCH16_DTYPE = np.dtype([("end", "<u8"), ("length", "<u4"), ("value", "<u4")])  # daac_match16 = the crate's own Match fields
MATCH8_DTYPE = np.dtype([("value", "<u4"), ("end_len", "<u4")])  # daac_match8: end relative to the run's base | length << end_bits
OUTPUT_DTYPE = np.dtype([("value", "<u4"), ("length", "<u4"), ("parent", "<u4")])  # an output record (a pattern's "slot")
PATTERN_COUNT_DTYPE = np.dtype([("value", "<u4"), ("length", "<u4"), ("count", "<u8")])
SPAN_DTYPE = np.dtype(("<u8", (2,)))  # a token's {start, end}: an array of it has shape [T, 2]
SLOT_COUNT_DTYPE = np.dtype([("slot", "<u4"), ("count", "<u4")])  # daac_slot_count: a row of a batch's documents x slots matrix


class DeviceMatches:
    """`count` tuples at device address `ptr`, in the reference's order: daac_match (24 bytes, MATCH_DTYPE) or, from
    scan_device(fmt16=True), daac_match16 (MATCH16_DTYPE)"""

    def __init__(self, ptr, count, dtype=None):
        self.ptr, self.count, self.dtype = ptr, count, (MATCH_DTYPE if dtype is None else dtype)

    def to_numpy(self, first=0, n=None):
        if self.count and self.ptr is None:
            raise DaachorseError(1, "the device match list has been freed")
        n = self.count - first if n is None else n
        if not (0 <= first <= self.count and 0 <= n <= self.count - first):
            raise DaachorseError(1, f"to_numpy({first}, {n}) outside a list of {self.count} tuples")
        out = np.zeros(n, dtype=self.dtype)
        if n:
            _ffi.check(_ffi.lib().daac_device_to_host(out.ctypes.data, self.ptr + first * self.dtype.itemsize, n * self.dtype.itemsize))
        return out

    def free(self):
        if self.ptr:
            _ffi.lib().daac_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceOffsets:
    """`count` u64 at device address `ptr` (the CSR offsets of a batch's tuple list)"""

    def __init__(self, ptr, count):
        self.ptr, self.count = ptr, count

    def to_numpy(self):
        out = np.zeros(self.count, dtype=np.uint64)
        if self.count:
            if not self.ptr:
                raise DaachorseError(1, "the device offsets have been freed")
            _ffi.check(_ffi.lib().daac_device_to_host(out.ctypes.data, self.ptr, self.count * 8))
        return out

    def free(self):
        if self.ptr:
            _ffi.lib().daac_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _LazyIter:
    """Iterator<Item = Match<u32>> over daac_iter_* (bytewise/iter.rs next())."""

    def __init__(self, pma, mode, haystack, engine, stream, compact=False):
        self._pma = pma
        self._h = _Haystack(haystack)
        self._it = C.c_void_p()
        self._compact = bool(compact)
        opener = _ffi.lib().daac_iter_open_compact if compact else _ffi.lib().daac_iter_open
        _ffi.check(opener(pma._h, int(mode), int(engine), self._h.ptr, self._h.len, self._h.is_device, stream, C.byref(self._it)))

    def __iter__(self):
        return self

    def __next__(self):
        m = _ffi.Match()
        r = _ffi.lib().daac_iter_next(self._it, C.byref(m))
        if r == 1:
            return Match(m.start, m.end, m.value)
        if r == 0:
            raise StopIteration
        _ffi.check(-r)

    def next_batch(self):
        """daac_iter_next_batch: the next run of matches as a structured numpy VIEW {end u64, length u32, value u32} of the iterator's
        own window buffer (valid until the next call), or None when the iterator is exhausted."""
        import numpy as np
        p, n = C.c_void_p(), C.c_size_t()
        r = _ffi.lib().daac_iter_next_batch(self._it, C.byref(p), C.byref(n))
        if r == 0:
            return None
        if r < 0:
            _ffi.check(-r)
        buf = (C.c_char * (n.value * 16)).from_address(p.value)
        return np.frombuffer(buf, dtype=MATCH16_DTYPE)

    def next_batch8(self):
        """daac_iter_next_batch8 (iterators opened with compact=True): the next run as (view {value u32, end_len u32}, end_base, end_bits) —
        end = end_base + (end_len & ((1 << end_bits) - 1)), length = end_len >> end_bits — or None when the iterator is exhausted."""
        import numpy as np
        p, n, base, eb = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint32()
        r = _ffi.lib().daac_iter_next_batch8(self._it, C.byref(p), C.byref(n), C.byref(base), C.byref(eb))
        if r == 0:
            return None
        if r < 0:
            _ffi.check(-r)
        buf = (C.c_char * (n.value * 8)).from_address(p.value)
        return np.frombuffer(buf, dtype=MATCH8_DTYPE), base.value, eb.value

    def close(self):
        if self._it:
            _ffi.lib().daac_iter_close(self._it)
            self._it = None

    def __del__(self):
        try:
            if self._it:
                _ffi.lib().daac_iter_close(self._it)
                self._it = None
        except Exception:
            pass


class _Stepper:
    """FindStepper / FindOverlappingStepper (bytewise/iter.rs:344-475, charwise/iter.rs:403-534) fed chunk by chunk:
    `feed(chunk)` returns the matches decided so far, positions counted from the first byte ever fed."""

    def __init__(self, pma, mode, engine, stream):
        self._pma = pma
        self._stream = stream
        self._s = C.c_void_p()
        _ffi.check(_ffi.lib().daac_stream_open(pma._h, int(mode), int(engine), stream, C.byref(self._s)))

    def feed(self, chunk):
        h = _Haystack(chunk)
        out = C.c_void_p()
        _ffi.check(_ffi.lib().daac_stream_feed(self._s, h.ptr, h.len, h.is_device, C.byref(out)))
        n = _ffi.lib().daac_matches_count(out)
        if n == 0:
            _ffi.lib().daac_matches_free(out)
            return np.zeros(0, dtype=MATCH_DTYPE)
        return np.asarray(_MatchList(out, n))

    def feed_compact(self, chunk):
        """daac_stream_feed_compact: the same feed with the chunk's matches as 8-byte tuples -> (view {value u32, end_len u32}, end_base, end_bits),
        end = end_base + (end_len & ((1 << end_bits) - 1)), length = end_len >> end_bits; the view is valid until the next feed"""
        h = _Haystack(chunk)
        p, n, base, eb = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint32()
        _ffi.check(_ffi.lib().daac_stream_feed_compact(self._s, h.ptr, h.len, h.is_device, C.byref(p), C.byref(n), C.byref(base), C.byref(eb)))
        if n.value == 0:
            return np.zeros(0, dtype=MATCH8_DTYPE), base.value, eb.value
        buf = (C.c_char * (n.value * 8)).from_address(p.value)
        return np.frombuffer(buf, dtype=MATCH8_DTYPE), base.value, eb.value

    @staticmethod
    def decode8(run, end_base, end_bits):
        """8-byte tuples -> MATCH_DTYPE {start, end, value}"""
        out = np.zeros(len(run), dtype=MATCH_DTYPE)
        el = run["end_len"].astype(np.uint64)
        out["end"] = np.uint64(end_base) + (el & np.uint64((1 << end_bits) - 1))
        out["start"] = out["end"] - (el >> np.uint64(end_bits))
        out["value"] = run["value"]
        return out

    def __del__(self):
        try:
            if self._s:
                _ffi.lib().daac_stream_close(self._s)
                self._s = None
        except Exception:
            pass


class DoubleArrayAhoCorasick:
    """DoubleArrayAhoCorasick<u32> (reference src/bytewise.rs:54-68)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        try:
            if self._h:
                _ffi.lib().daac_pma_free(self._h)
                self._h = None
        except Exception:
            pass

    # ---- construction (bytewise.rs:103-110, 154-161) ------------------------------------------------
    @classmethod
    def new(cls, patterns):
        return DoubleArrayAhoCorasickBuilder().build(patterns)

    @classmethod
    def with_values(cls, patvals):
        return DoubleArrayAhoCorasickBuilder().build_with_values(patvals)

    # ---- (de)serialisation (bytewise.rs:801-820, 868-964) --------------------------------------------
    def serialize(self):
        buf, n = C.c_void_p(), C.c_size_t()
        _ffi.check(_ffi.lib().daac_pma_serialize(self._h, C.byref(buf), C.byref(n)))
        data = C.string_at(buf, n.value)
        _ffi.lib().daac_free(buf)
        return data

    @classmethod
    def deserialize(cls, source):
        """-> (pma, remaining bytes), as the reference returns (Self, &[u8])"""
        source = bytes(source)
        h, consumed = C.c_void_p(), C.c_size_t()
        _ffi.check(_ffi.lib().daac_bytewise_from_serialized(source, len(source), C.byref(h), C.byref(consumed)))
        return cls(h), source[consumed.value:]

    @classmethod
    def from_parts(cls, kind, num_states, outputs, states=None, leftmost_states=None, fails=None):
        def arr(x, cols):
            if x is None:
                return None, 0
            a = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, cols) if cols > 1 else np.ascontiguousarray(x, dtype=np.uint32)
            return a, len(a)
        st, n_st = arr(states, 3)
        ls, n_ls = arr(leftmost_states, 2)
        fl, n_fl = arr(fails, 1)
        if n_fl != n_ls:  # the C ABI copies n_lstates entries from `fails` (bytewise.rs:61-63: the two arrays are parallel)
            raise DaachorseError(1, "`fails` must have one entry per leftmost state")
        ou, n_ou = arr(outputs, 3)
        h = C.c_void_p()
        p = lambda a: a.ctypes.data if a is not None and a.size else None
        _ffi.check(_ffi.lib().daac_bytewise_from_parts(p(st), n_st, p(ls), p(fl), n_ls, p(ou), n_ou, int(kind), int(num_states),
                                                       C.byref(h)))
        return cls(h)

    # ---- introspection -----------------------------------------------------------------------------------
    def info(self):
        i = _ffi.Info()
        i.struct_size = C.sizeof(_ffi.Info)
        _ffi.check(_ffi.lib().daac_pma_info(self._h, C.byref(i)))
        return i

    def explain(self):
        """the engine plan as text: which engine / kernel family serves each kind of request, and why not the fastest one"""
        n = _ffi.lib().daac_pma_explain(self._h, None, 0)
        buf = C.create_string_buffer(n)
        _ffi.lib().daac_pma_explain(self._h, buf, n)
        return buf.value.decode()

    def match_kind(self):
        return MatchKind(self.info().match_kind)

    def num_states(self):
        return self.info().num_states

    def heap_bytes(self):
        return self.info().heap_bytes

    def upload(self, device=0):
        _ffi.check(_ffi.lib().daac_pma_upload(self._h, device))
        return self

    def set_option(self, name, value=None):
        """daac_pma_set_option: an option for THIS handle (overrides the process-wide daac_set_option value); value=None removes the override"""
        _ffi.check(_ffi.lib().daac_pma_set_option(self._h, name.encode(), 0 if value is None else int(value), 1 if value is None else 0))
        return self

    def trim(self):
        """daac_pma_trim: gives back the scratch the handle keeps between calls (tables stay)"""
        _ffi.check(_ffi.lib().daac_pma_trim(self._h))
        return self

    # ---- lazy iterators, crate names (bytewise.rs:190-203, 292-314, 410-428, 547-566) --------------------
    # (compact=True: daac_iter_open_compact — 8-byte tuples over PCIe, read with next_batch8(); iterating match by match works on either)
    def find_iter(self, haystack, engine=Engine.Auto, stream=None, compact=False):
        return _LazyIter(self, ScanMode.Find, haystack, engine, stream, compact)

    def find_overlapping_iter(self, haystack, engine=Engine.Auto, stream=None, compact=False):
        return _LazyIter(self, ScanMode.FindOverlapping, haystack, engine, stream, compact)

    def find_overlapping_no_suffix_iter(self, haystack, engine=Engine.Auto, stream=None, compact=False):
        return _LazyIter(self, ScanMode.FindOverlappingNoSuffix, haystack, engine, stream, compact)

    def leftmost_find_iter(self, haystack, engine=Engine.Auto, stream=None, compact=False):
        return _LazyIter(self, ScanMode.LeftmostFind, haystack, engine, stream, compact)

    # ---- steppers for haystacks that arrive in pieces (bytewise.rs:238-251, 353-375; iter.rs:344-475) ------------------
    def find_stepper(self, engine=Engine.Auto, stream=None):
        return _Stepper(self, ScanMode.Find, engine, stream)

    def find_overlapping_stepper(self, engine=Engine.Auto, stream=None):
        return _Stepper(self, ScanMode.FindOverlapping, engine, stream)

    def find_overlapping_no_suffix_stepper(self, engine=Engine.Auto, stream=None):
        return _Stepper(self, ScanMode.FindOverlappingNoSuffix, engine, stream)

    # ---- eager forms (`.collect()` / `.count()` on the iterators) ---------------------------------------------
    def scan(self, mode, haystack, engine=Engine.Auto, stream=None):
        """-> numpy structured array (start, end, value) in the reference's order"""
        h = _Haystack(haystack)
        out = C.c_void_p()
        _ffi.check(_ffi.lib().daac_scan(self._h, int(mode), int(engine), h.ptr, h.len, h.is_device, stream, C.byref(out)))
        n = _ffi.lib().daac_matches_count(out)
        if n == 0:
            _ffi.lib().daac_matches_free(out)
            return np.zeros(0, dtype=MATCH_DTYPE)
        return np.asarray(_MatchList(out, n))  # read-only view of the library's buffer, freed with the array

    def scan_device(self, mode, haystack, engine=Engine.Auto, stream=None, fmt16=False):
        """-> DeviceMatches: the match list left in device memory (daac_scan_device; fmt16: daac_scan_device16, 16-byte tuples)"""
        h = _Haystack(haystack)
        ptr, n = C.c_void_p(), C.c_uint64()
        fn = _ffi.lib().daac_scan_device16 if fmt16 else _ffi.lib().daac_scan_device
        _ffi.check(fn(self._h, int(mode), int(engine), h.ptr, h.len, h.is_device, stream, C.byref(ptr), C.byref(n)))
        return DeviceMatches(ptr.value, n.value, MATCH16_DTYPE if fmt16 else MATCH_DTYPE)

    def count(self, mode, haystack, engine=Engine.Auto, stream=None, result_dev=None, begin=0):
        """`.count()` of the iterator: the number of matches with end in (begin, len], no checksum; with `result_dev`
        (device pointer to 3 x u64, the count goes to [0]) the call is asynchronous and returns None."""
        h = _Haystack(haystack)
        if result_dev is not None:
            _ffi.check(_ffi.lib().daac_scan_count_only_range(self._h, int(mode), int(engine), h.ptr, h.len, begin, h.is_device, stream,
                                                             None, result_dev))
            return None
        cnt = C.c_uint64()
        _ffi.check(_ffi.lib().daac_scan_count_only_range(self._h, int(mode), int(engine), h.ptr, h.len, begin, h.is_device, stream,
                                                         C.byref(cnt), None))
        return cnt.value

    def scan_count(self, mode, haystack, engine=Engine.Auto, stream=None, result_dev=None, begin=0):
        """-> (count, checksum) of the matches with end in (begin, len]; with `result_dev` (device
        pointer to 3 x u64 = count, S1, S2) the call is asynchronous and returns None."""
        h = _Haystack(haystack)
        if result_dev is not None:
            _ffi.check(_ffi.lib().daac_scan_count_range(self._h, int(mode), int(engine), h.ptr, h.len, begin, h.is_device, stream,
                                                        None, None, result_dev))
            return None
        cnt, cs = C.c_uint64(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_scan_count_range(self._h, int(mode), int(engine), h.ptr, h.len, begin, h.is_device, stream,
                                                    C.byref(cnt), C.byref(cs), None))
        return cnt.value, cs.value

    # ---- batches: many documents in one call, per-document results (daac_scan_count_batch / daac_scan_batch_device16) ------------
    # `docs`: a sequence of str / bytes / uint8 arrays (packed on the host), or (uint8 CUDA tensor, int64 CUDA tensor of n + 1 offsets).
    # Every document gets what the single-haystack call returns on it alone; positions are relative to the document.
    def _count_batch(self, mode, docs, engine, stream, want_checksum, out):
        b = _Batch(docs)
        if out is not None:   # device results: the call is asynchronous on `stream`
            outs = out if isinstance(out, (tuple, list)) else (out,)
            cp = _device_u64(outs[0], b.n)
            sp = _device_u64(outs[1], b.n) if want_checksum else None
            _ffi.check(_ffi.lib().daac_scan_count_batch(self._h, int(mode), int(engine), b.hay, b.off, b.n, b.is_device, stream, cp, sp, 1))
            return None
        counts = np.zeros(b.n, dtype=np.uint64)
        sums = np.zeros(b.n, dtype=np.uint64) if want_checksum else None
        _ffi.check(_ffi.lib().daac_scan_count_batch(self._h, int(mode), int(engine), b.hay, b.off, b.n, b.is_device, stream,
                                                    counts.ctypes.data if b.n else None,
                                                    sums.ctypes.data if want_checksum and b.n else None, 0))
        return (counts, sums) if want_checksum else counts

    def count_batch(self, mode, docs, engine=Engine.Auto, stream=None, out=None):
        """-> np.uint64[n]: `.count()` of every document; with `out` (a CUDA int64 tensor of n) the counts stay there (asynchronous)"""
        return self._count_batch(mode, docs, engine, stream, False, out)

    def scan_count_batch(self, mode, docs, engine=Engine.Auto, stream=None, out=None):
        """-> (counts, checksums), np.uint64[n] each (the checksum of scan_count, ends relative to the document); with `out` =
        (counts tensor, checksums tensor) on the device the results stay there (asynchronous)"""
        return self._count_batch(mode, docs, engine, stream, True, out)

    def scan_batch_device(self, mode, docs, engine=Engine.Auto, stream=None):
        """-> (DeviceMatches of 16-byte tuples {end, length, value}, DeviceOffsets: n + 1 u64 CSR offsets on the device): document i's
        tuples are [offsets[i], offsets[i+1]).  Both are freed with .free() (or when they are collected)."""
        b = _Batch(docs)
        ptr, offs, tot = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_scan_batch_device16(self._h, int(mode), int(engine), b.hay, b.off, b.n, b.is_device, stream,
                                                       C.byref(ptr), C.byref(offs), C.byref(tot)))
        return DeviceMatches(ptr.value, tot.value, MATCH16_DTYPE), DeviceOffsets(offs.value, b.n + 1)

    def scan_batch(self, mode, docs, engine=Engine.Auto, stream=None):
        """-> (MATCH_DTYPE array, start / end / value relative to each document, np.uint64[n + 1] offsets into it)"""
        dm, do = self.scan_batch_device(mode, docs, engine, stream)
        try:
            t16 = dm.to_numpy()
            offsets = do.to_numpy()
        finally:
            dm.free()
            do.free()
        out = np.zeros(len(t16), dtype=MATCH_DTYPE)
        out["end"] = t16["end"]
        out["start"] = t16["end"] - t16["length"].astype(np.uint64)
        out["value"] = t16["value"]
        return out, offsets


    # ---- histograms: per-pattern match counts of an overlapping scan (daac_pma_outputs / daac_scan_histogram) ---------------------
    def outputs(self):
        """-> structured array {value, length, parent} of outputs_len rows: row i is "slot i", the one output record of a pattern
        (parent: 1-based index of the next record of the output list, 0 = none)"""
        n = _ffi.lib().daac_pma_outputs(self._h, None, 0)
        out = np.zeros(n, dtype=OUTPUT_DTYPE)
        if n:
            _ffi.lib().daac_pma_outputs(self._h, out.ctypes.data, n)
        return out

    def histogram(self, mode, haystack, engine=Engine.Auto, stream=None, begin=0, out=None):
        """-> np.uint64[outputs_len]: counts[i] = matches of slot i's pattern among the matches count(mode, haystack, begin=begin)
        counts (FindOverlapping / FindOverlappingNoSuffix); with `out` (a CUDA int64 tensor of outputs_len) the counts stay there
        and the call returns None."""
        h = _Haystack(haystack)
        n = _ffi.lib().daac_pma_outputs(self._h, None, 0)
        if out is not None:
            _ffi.check(_ffi.lib().daac_scan_histogram(self._h, int(mode), int(engine), h.ptr, h.len, begin, h.is_device, stream,
                                                      _device_u64(out, n), 1))
            return None
        counts = np.zeros(n, dtype=np.uint64)
        _ffi.check(_ffi.lib().daac_scan_histogram(self._h, int(mode), int(engine), h.ptr, h.len, begin, h.is_device, stream,
                                                  counts.ctypes.data if n else None, 0))
        return counts

    def pattern_counts(self, mode, haystack, **kw):
        """-> structured array {value, length, count}, one row per pattern (slot): outputs() joined with histogram()"""
        o = self.outputs()
        res = np.zeros(len(o), dtype=PATTERN_COUNT_DTYPE)
        res["value"], res["length"] = o["value"], o["length"]
        res["count"] = self.histogram(mode, haystack, **kw)
        return res

    # ---- per-document pattern counts of a batch, as a CSR matrix (daac_scan_histogram_batch) ------------------------------------
    def histogram_batch_device(self, mode, docs, engine=Engine.Auto, stream=None):
        """-> (DeviceMatches of rows {slot, count} (SLOT_COUNT_DTYPE), DeviceOffsets: n + 1 u64 on the device): document i's rows are
        [offsets[i], offsets[i+1]), one per slot (row of outputs()) that matched in it, in ascending slot order; all four modes.
        Both are freed with .free() (or when they are collected)."""
        b = _Batch(docs)
        ptr, offs, tot = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_scan_histogram_batch(self._h, int(mode), int(engine), b.hay, b.off, b.n, b.is_device, stream,
                                                        C.byref(ptr), C.byref(offs), C.byref(tot)))
        return DeviceMatches(ptr.value, tot.value, SLOT_COUNT_DTYPE), DeviceOffsets(offs.value, b.n + 1)

    def histogram_batch(self, mode, docs, engine=Engine.Auto, stream=None):
        """-> (SLOT_COUNT_DTYPE array of rows, np.uint64[n + 1] offsets into it)"""
        dm, do = self.histogram_batch_device(mode, docs, engine, stream)
        try:
            return dm.to_numpy(), do.to_numpy()
        finally:
            dm.free()
            do.free()

    # ---- replace_all: the text with every match of find_iter / leftmost_find_iter replaced (daac_replace_all[_batch]) ---------------
    # `replacements`: one bytes / str for every match, or a sequence indexed by the match's value (automata built without values:
    # the pattern's index).  mode=None: Find for Standard handles, LeftmostFind otherwise.
    def _replace_mode(self, mode):
        if mode is not None:
            return int(mode)
        return int(ScanMode.Find if self.match_kind() == MatchKind.Standard else ScanMode.LeftmostFind)

    def replace_all(self, haystack, replacements, mode=None, engine=Engine.Auto, stream=None, device=False):
        """-> bytes; device=True: DeviceMatches of uint8 (to_numpy / free), the result left in device memory"""
        r = _Replacements(replacements)
        h = _Haystack(haystack)
        ptr, n, k = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_replace_all(self._h, self._replace_mode(mode), int(engine), h.ptr, h.len, h.is_device, stream,
                                               r.blob_ptr, r.off_ptr, r.n, C.byref(ptr), C.byref(n), C.byref(k)))
        dm = DeviceMatches(ptr.value, n.value, np.dtype(np.uint8))
        dm.n_replaced = k.value
        if device:
            return dm
        try:
            return dm.to_numpy().tobytes()
        finally:
            dm.free()

    def replace_all_batch(self, docs, replacements, mode=None, engine=Engine.Auto, stream=None, device=False):
        """-> list of bytes, one per document (each replaced as a haystack of its own); device=True: (DeviceMatches of uint8,
        DeviceOffsets of n + 1 u64): document i's result is [offsets[i], offsets[i+1])"""
        r = _Replacements(replacements)
        b = _Batch(docs)
        ptr, offs, n, k = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_replace_all_batch(self._h, self._replace_mode(mode), int(engine), b.hay, b.off, b.n, b.is_device, stream,
                                                     r.blob_ptr, r.off_ptr, r.n, C.byref(ptr), C.byref(offs), C.byref(n), C.byref(k)))
        dm, do = DeviceMatches(ptr.value, n.value, np.dtype(np.uint8)), DeviceOffsets(offs.value, b.n + 1)
        dm.n_replaced = k.value
        if device:
            return dm, do
        try:
            out, o = dm.to_numpy().tobytes(), do.to_numpy()
        finally:
            dm.free()
            do.free()
        return [out[int(o[i]):int(o[i + 1])] for i in range(b.n)]

    # ---- tokenize: the values of the matches of find_iter / leftmost_find_iter and the gaps between them as one id list
    # (daac_tokenize[_batch]).  `gap` says what the text between matches becomes (Gap), `gap_id` the id it gets (Gap.Bytes: gap_id +
    # the byte).  mode=None: Find for Standard handles, LeftmostFind otherwise.
    def tokenize(self, haystack, gap=Gap.Unk, gap_id=0, spans=False, mode=None, engine=Engine.Auto, stream=None, device=False):
        """-> ids (np.uint32[T]), or (ids, spans) with spans=True (np.uint64[T, 2], {start, end} in bytes); device=True: the same as
        DeviceMatches (to_numpy / free), left in device memory"""
        h = _Haystack(haystack)
        o = _TokenOuts(spans)
        _ffi.check(_ffi.lib().daac_tokenize(self._h, self._replace_mode(mode), int(engine), h.ptr, h.len, h.is_device, stream, int(gap), int(gap_id),
                                            *o.ptrs(), *o.counts()))
        return self._token_result(o.result(), o.k.value, device)

    def tokenize_batch(self, docs, gap=Gap.Unk, gap_id=0, spans=False, mode=None, engine=Engine.Auto, stream=None, device=False):
        """-> (ids, offsets) or (ids, spans, offsets): every document is tokenized as a haystack of its own, document i's tokens are
        [offsets[i], offsets[i+1]) (np.uint64[n + 1]) and its spans count from its first byte; device=True: DeviceMatches for ids and
        spans, DeviceOffsets for offsets"""
        b = _Batch(docs)
        o = _TokenOuts(spans, b.n)
        _ffi.check(_ffi.lib().daac_tokenize_batch(self._h, self._replace_mode(mode), int(engine), b.hay, b.off, b.n, b.is_device, stream, int(gap),
                                                  int(gap_id), *o.ptrs(), *o.counts()))
        return self._token_result(o.result(), o.k.value, device)

    # ---- tokenize_unigram: the segmentation whose pieces' scores sum highest (daac_tokenize_unigram[_batch]; Standard automata).
    # `scores`: float32, indexed by match value; `unk_score`: the score of an unknown piece, which `gap` makes a byte (Gap.Bytes, id
    # gap_id + the byte) or a UTF-8 code point (Gap.Chars, id gap_id).  One lane walks one document: made for batches of short documents.
    @staticmethod
    def _scores(scores):
        a = np.ascontiguousarray(scores)
        if a.ndim != 1 or a.dtype.kind not in "fiu":
            raise DaachorseError(1, "scores must be a one-dimensional array of numbers")
        return np.ascontiguousarray(a, dtype=np.float32)

    def tokenize_unigram(self, haystack, scores, unk_score, gap=Gap.Chars, gap_id=0, spans=False, engine=Engine.Auto, stream=None, device=False):
        """-> (ids, score), or (ids, spans, score) with spans=True: np.uint32[T], np.uint64[T, 2] ({start, end} in bytes) and the path's
        score, a np.float32; device=True: ids and spans as DeviceMatches (to_numpy / free), left in device memory"""
        h = _Haystack(haystack)
        sc = self._scores(scores)
        o, score = _TokenOuts(spans), C.c_float()
        _ffi.check(_ffi.lib().daac_tokenize_unigram(self._h, int(engine), h.ptr, h.len, h.is_device, stream, sc.ctypes.data if sc.size else None, sc.size,
                                                    C.c_float(unk_score), int(gap), int(gap_id), *o.ptrs(), *o.counts(), C.byref(score)))
        res = self._token_result(o.result(), o.k.value, device)
        return (res if spans else (res,)) + (np.float32(score.value),)

    def tokenize_unigram_batch(self, docs, scores, unk_score, gap=Gap.Chars, gap_id=0, spans=False, doc_scores=False, engine=Engine.Auto, stream=None,
                               device=False):
        """-> (ids, offsets), with spans=True (ids, spans, offsets), with doc_scores=True one more at the end: np.float32[n], every
        document's score.  Document i's tokens are [offsets[i], offsets[i+1]); device=True: DeviceMatches / DeviceOffsets"""
        b = _Batch(docs)
        sc = self._scores(scores)
        o, ds = _TokenOuts(spans, b.n), C.c_void_p()
        _ffi.check(_ffi.lib().daac_tokenize_unigram_batch(self._h, int(engine), b.hay, b.off, b.n, b.is_device, stream, sc.ctypes.data if sc.size else None,
                                                          sc.size, C.c_float(unk_score), int(gap), int(gap_id), *o.ptrs(),
                                                          C.byref(ds) if doc_scores else None, *o.counts()))
        out = o.result()
        if doc_scores:
            out.append(DeviceMatches(ds.value, b.n if ds.value else 0, np.dtype(np.float32)))
        return self._token_result(out, o.k.value, device)

    # ---- tokenize_bpe: byte-pair merging in rank order (daac_tokenize_bpe[_batch]; Standard automata) — tiktoken's byte_pair_merge for
    # one piece of pre-split text.  `ranks`: uint32, indexed by match value (None: a piece's rank is its value; 0xFFFFFFFF: never the
    # product of a merge); a part the vocabulary lacks becomes a byte (Gap.Bytes, id gap_id + the byte) or a UTF-8 code point (Gap.Chars,
    # id gap_id).  One lane merges one document in up to L^2 / 2 steps: a document above option bpe_doc_max (4096) is refused.
    @staticmethod
    def _ranks(ranks):
        if ranks is None:
            return None
        a = np.ascontiguousarray(ranks)
        if a.ndim != 1 or a.dtype.kind not in "iu" or a.size == 0 or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
            raise DaachorseError(1, "ranks must be None or a non-empty one-dimensional array of integers in 0 .. 0xFFFFFFFF")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def tokenize_bpe(self, haystack, ranks=None, gap=Gap.Bytes, gap_id=0, spans=False, engine=Engine.Auto, stream=None, device=False):
        """-> ids (np.uint32[T]), or (ids, spans) with spans=True (np.uint64[T, 2], {start, end} in bytes); device=True: the same as
        DeviceMatches (to_numpy / free), left in device memory"""
        h = _Haystack(haystack)
        rk = self._ranks(ranks)
        o = _TokenOuts(spans)
        _ffi.check(_ffi.lib().daac_tokenize_bpe(self._h, int(engine), h.ptr, h.len, h.is_device, stream, None if rk is None else rk.ctypes.data,
                                                0 if rk is None else rk.size, int(gap), int(gap_id), *o.ptrs(), *o.counts()))
        return self._token_result(o.result(), o.k.value, device)

    def tokenize_bpe_batch(self, docs, ranks=None, gap=Gap.Bytes, gap_id=0, spans=False, engine=Engine.Auto, stream=None, device=False):
        """-> (ids, offsets) or (ids, spans, offsets): every document is merged on its own, document i's tokens are
        [offsets[i], offsets[i+1]) (np.uint64[n + 1]) and its spans count from its first byte; device=True: DeviceMatches for ids and
        spans, DeviceOffsets for offsets"""
        b = _Batch(docs)
        rk = self._ranks(ranks)
        o = _TokenOuts(spans, b.n)
        _ffi.check(_ffi.lib().daac_tokenize_bpe_batch(self._h, int(engine), b.hay, b.off, b.n, b.is_device, stream, None if rk is None else rk.ctypes.data,
                                                      0 if rk is None else rk.size, int(gap), int(gap_id), *o.ptrs(), *o.counts()))
        return self._token_result(o.result(), o.k.value, device)

    def tokenize_bpe_docs(self, docs, ranks=None, split=Split.Gpt2, gap=Gap.Bytes, gap_id=0, spans=False, engine=Engine.Auto, stream=None, device=False,
                          special=None, pack=None):
        """tokenize_bpe behind a pre-tokenizer split, per document: split_batch cuts the documents into words, tokenize_bpe_batch runs over
        (hay, word_offsets) and daac_offsets_compose turns its offsets per word into offsets per document.  -> (ids, offsets) or
        (ids, spans, offsets) as tokenize_bpe_batch gives them, with document i's tokens in [offsets[i], offsets[i+1]) and spans that
        count from the document's first byte.  `split`: a Split rule (the cached default splitter) or a Splitter.  Host documents are
        uploaded once; a word above option bpe_doc_max answers 6.  `special`: None, or a SpecialTokens: the batch is cut around the
        special tokens found in the raw text (SpecialTokens.cut_batch), the chain above runs over the segment batch, so every stretch
        of text between specials is split as a string of its own, and splice_special puts the result back together per document with
        each special as the one token of its id.  n_matches stays the tokenizer scan's count.  `pack`: None, or a Packer: the token
        result goes through Packer.pack as a batch of singles (its template, truncation and padding) and is freed; the call returns
        pack's dict of planes instead."""
        if pack is not None and not isinstance(pack, Packer):
            raise DaachorseError(1, "pack is None or a Packer")
        b = _Batch(docs)
        if not b.is_device:
            b = _Batch(_upload(b))
        sp = split if isinstance(split, Splitter) else _default_splitter(split)
        rk = self._ranks(ranks)
        if special is None:
            out, k = self._bpe_docs_chain(b, sp, rk, gap, gap_id, spans, engine, stream)
        else:
            out, k = _special_docs(b, special, spans, stream, lambda sb: self._bpe_docs_chain(sb, sp, rk, gap, gap_id, spans, engine, stream))
        if pack is not None:
            return _pack_docs(pack, out, stream, device)
        return self._token_result(out, k, device)

    def _bpe_docs_chain(self, b, sp, rk, gap, gap_id, spans, engine, stream):
        """split, tokenize_bpe_batch, spans_rebase and offsets_compose over the device batch b -> ([ids, spans?, doc_offsets] in device
        memory, n_matches)"""
        return self._docs_chain(b, sp, spans, stream, False, lambda wo, n_words, flags, o: _ffi.lib().daac_tokenize_bpe_batch(
            self._h, int(engine), b.hay, wo, n_words, 1, stream, None if rk is None else rk.ctypes.data, 0 if rk is None else rk.size, int(gap), int(gap_id),
            *o.ptrs(), *o.counts()))

    # ---- tokenize_wordpiece: BERT's WordPiece (daac_tokenize_wordpiece[_batch]; Standard automata) — greedy longest-match-first over the
    # initial pieces and the "##" continuation pieces of a word of pre-split text; a word with a position no piece covers, or of more
    # than max_chars characters, is the one token unk_id.  `first_ids` / `cont_ids`: uint32, indexed by match value, 0xFFFFFFFF = no
    # such piece (wordpiece_tables() makes them and the patterns from a vocabulary).
    @staticmethod
    def _piece_ids(name, ids):
        a = np.ascontiguousarray(ids) if ids is not None else None
        if a is None or a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
            raise DaachorseError(1, f"{name} must be a one-dimensional array of integers in 0 .. 0xFFFFFFFF")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def _wordpiece_model(self, first_ids, cont_ids, unk_id, max_chars):
        f, c = self._piece_ids("first_ids", first_ids), self._piece_ids("cont_ids", cont_ids)
        if f.size != c.size:
            raise DaachorseError(1, f"first_ids has {f.size} entries and cont_ids {c.size}: both are indexed by match value (n_ids)")
        if not 0 <= int(unk_id) <= 0xFFFFFFFF:
            raise DaachorseError(1, "unk_id must be in 0 .. 0xFFFFFFFF")
        if not 1 <= int(max_chars) <= 0xFFFFFFFF:
            raise DaachorseError(1, "max_chars must be in 1 .. 0xFFFFFFFF")
        keep = (f, c, np.zeros(1, dtype=np.uint32))   # (an empty table still has an address)
        return keep, (f.ctypes.data if f.size else keep[2].ctypes.data, c.ctypes.data if c.size else keep[2].ctypes.data, f.size, int(unk_id), int(max_chars))

    def tokenize_wordpiece(self, word, first_ids, cont_ids, unk_id, max_chars=100, spans=False, engine=Engine.Auto, stream=None, device=False):
        """-> ids (np.uint32[T]), or (ids, spans) with spans=True (np.uint64[T, 2], {start, end} in bytes); device=True: the same as
        DeviceMatches (to_numpy / free), left in device memory"""
        h = _Haystack(word)
        keep, model = self._wordpiece_model(first_ids, cont_ids, unk_id, max_chars)
        o = _TokenOuts(spans)
        _ffi.check(_ffi.lib().daac_tokenize_wordpiece(self._h, int(engine), h.ptr, h.len, h.is_device, stream, *model, *o.ptrs(), *o.counts()))
        return self._token_result(o.result(), o.k.value, device)

    def tokenize_wordpiece_batch(self, words, first_ids, cont_ids, unk_id, max_chars=100, skip=None, spans=False, engine=Engine.Auto, stream=None,
                                 device=False):
        """-> (ids, offsets) or (ids, spans, offsets): every document is a word, segmented on its own; word i's tokens are
        [offsets[i], offsets[i+1]) (np.uint64[n + 1]) and its spans count from its first byte.  `skip`: None, or one byte per word
        (a uint8 array, a uint8 CUDA tensor or the DeviceMatches of Splitter.words_space): a word whose byte is non-zero yields no
        tokens.  device=True: DeviceMatches for ids and spans, DeviceOffsets for offsets"""
        b = _Batch(words)
        keep, model = self._wordpiece_model(first_ids, cont_ids, unk_id, max_chars)
        skip_keep, skip_ptr = _skip_flags(skip, b.n)
        o = _TokenOuts(spans, b.n)
        _ffi.check(_ffi.lib().daac_tokenize_wordpiece_batch(self._h, int(engine), b.hay, b.off, b.n, b.is_device, stream, *model, skip_ptr, *o.ptrs(),
                                                            *o.counts()))
        return self._token_result(o.result(), o.k.value, device)

    def tokenize_wordpiece_docs(self, docs, first_ids, cont_ids, unk_id, max_chars=100, split=Split.Bert, spans=False, engine=Engine.Auto, stream=None,
                                device=False, normalizer=None, special=None, pack=None):
        """tokenize_wordpiece behind BERT's pre-tokenizer, per document: split_batch cuts the documents into words, words_space tells
        which of them are whitespace, tokenize_wordpiece_batch runs over (hay, word_offsets) with those words skipped and
        daac_offsets_compose turns its offsets per word into offsets per document.  -> (ids, offsets) or (ids, spans, offsets) as
        tokenize_wordpiece_batch gives them, with document i's tokens in [offsets[i], offsets[i+1]) and spans that count from the
        document's first byte.  `split`: a Split rule (the cached default splitter; Split.Bert's has bert_char_classes()) or a
        Splitter.  Host documents are uploaded once.  `normalizer`: None (the text is taken as it is) or a Normalizer, such as
        bert_normalizer(): the documents are normalized on the device first (with src when spans=True), the chain above runs over the
        normalized batch and spans_to_source makes the spans count from the raw document's first byte, as `tokenizers` reports
        offsets.  `special`: None, or a SpecialTokens ([CLS], [SEP], [MASK] ..): the batch is cut around the special tokens found in
        the raw text, in front of the normalizer (SpecialTokens.cut_batch), all of the above runs over the segment batch and
        splice_special puts the result back together per document with each special as the one token of its id.  n_matches stays
        the tokenizer scan's count.  `pack`: None, or a Packer ([CLS] A [SEP], max_length, padding ..): the token result, with its
        raw-text spans when spans=True, goes through Packer.pack as a batch of singles and is freed; the call returns pack's dict of
        planes (input_ids, token_type_ids, attention_mask ..) instead."""
        if pack is not None and not isinstance(pack, Packer):
            raise DaachorseError(1, "pack is None or a Packer")
        b = _Batch(docs)
        if not b.is_device:
            b = _Batch(_upload(b))
        sp = split if isinstance(split, Splitter) else _default_splitter(split)
        keep, model = self._wordpiece_model(first_ids, cont_ids, unk_id, max_chars)
        if normalizer is not None and not isinstance(normalizer, Normalizer):
            raise DaachorseError(1, "normalizer is None or a Normalizer")
        if special is None:
            out, k = self._wordpiece_docs_norm(b, sp, model, spans, engine, stream, normalizer)
        else:
            out, k = _special_docs(b, special, spans, stream, lambda sb: self._wordpiece_docs_norm(sb, sp, model, spans, engine, stream, normalizer))
        if pack is not None:
            return _pack_docs(pack, out, stream, device)
        return self._token_result(out, k, device)

    def _wordpiece_docs_norm(self, b, sp, model, spans, engine, stream, normalizer):
        """_wordpiece_docs_chain over the device batch b, behind the normalizer where there is one -> ([ids, spans?, doc_offsets], n_matches)"""
        if normalizer is None:
            return self._wordpiece_docs_chain(b, sp, model, spans, engine, stream)
        norm = normalizer._run(b, stream, spans)   # out, out_offsets[, src]
        try:
            out, k = self._wordpiece_docs_chain(_DeviceBatch(norm[0].ptr, norm[1].ptr, b.n), sp, model, spans, engine, stream)
            if spans and out[0].count:
                try:
                    _ffi.check(_ffi.lib().daac_spans_to_source(out[1].ptr, out[2].ptr, norm[1].ptr, norm[2].ptr, b.hay, b.off, b.n, out[0].count, 1, stream))
                except Exception:
                    for o in out:
                        o.free()
                    raise
        finally:
            for o in norm:
                o.free()
        return out, k

    def _wordpiece_docs_chain(self, b, sp, model, spans, engine, stream):
        """split, words_space, tokenize_wordpiece_batch, spans_rebase and offsets_compose over the device batch b -> ([ids, spans?,
        doc_offsets] in device memory, n_matches)"""
        return self._docs_chain(b, sp, spans, stream, True, lambda wo, n_words, flags, o: _ffi.lib().daac_tokenize_wordpiece_batch(
            self._h, int(engine), b.hay, wo, n_words, 1, stream, *model, flags, *o.ptrs(), *o.counts()))

    @staticmethod
    def _docs_chain(b, sp, spans, stream, skip_space, call):
        """The chain of the two methods above over the device batch b: split, the words_space flags (skip_space), `call(word_offsets,
        n_words, flags or None, outs)` — the batch call over (hay, word_offsets), which returns its status —, spans_rebase and
        offsets_compose -> ([ids, spans?, doc_offsets] in device memory, n_matches).  What a step has made is freed if a later one fails."""
        wo, dw = sp._run(b, stream)
        n_words = wo.count - 1
        o, doc_offs, flags = _TokenOuts(spans, n_words), C.c_void_p(), None
        try:
            if skip_space:
                flags = sp._words_space(b.hay, 1, wo.ptr, n_words, stream)
            _ffi.check(call(wo.ptr, n_words, flags.ptr if skip_space else None, o))
            out = o.result()
            word_tok = out.pop()
            try:
                if spans and o.n.value:
                    _ffi.check(_ffi.lib().daac_spans_rebase(o.sp.value, word_tok.ptr, wo.ptr, dw.ptr, b.off, n_words, b.n, stream))
                _ffi.check(_ffi.lib().daac_offsets_compose(word_tok.ptr, dw.ptr, b.n + 1, stream, C.byref(doc_offs)))
            except Exception:
                for x in out:
                    x.free()
                raise
            finally:
                word_tok.free()
        finally:
            if flags is not None:
                flags.free()
            wo.free()
            dw.free()
        out.append(DeviceOffsets(doc_offs.value, b.n + 1))
        return out, o.k.value

    @staticmethod
    def _token_result(out, n_matches, device):
        out[0].n_matches = n_matches
        if not device:
            dev = out
            try:
                out = [o.to_numpy() for o in dev]
            finally:
                for o in dev:
                    o.free()
        return out[0] if len(out) == 1 else tuple(out)


class _TokenOuts:
    """The out-arguments of a token call (spans optional; n_docs=None: a single haystack, no offsets) and, after the call, its results"""

    def __init__(self, spans, n_docs=None):
        self.ids, self.n, self.k, self.n_docs = C.c_void_p(), C.c_uint64(), C.c_uint64(), n_docs
        self.sp = C.c_void_p() if spans else None
        self.offs = C.c_void_p() if n_docs is not None else None

    def ptrs(self):
        """dev_ids, dev_spans or NULL and, for a batch, dev_tok_offsets: the call's arguments in this order"""
        return (C.byref(self.ids), C.byref(self.sp) if self.sp is not None else None) + ((C.byref(self.offs),) if self.offs is not None else ())

    def counts(self):
        return C.byref(self.n), C.byref(self.k)

    def result(self):
        """-> [DeviceMatches ids, DeviceMatches spans?, DeviceOffsets offsets?], as _token_result takes them"""
        out = [DeviceMatches(self.ids.value, self.n.value, np.dtype(np.uint32))]
        if self.sp is not None:
            out.append(DeviceMatches(self.sp.value, self.n.value, SPAN_DTYPE))
        if self.offs is not None:
            out.append(DeviceOffsets(self.offs.value, self.n_docs + 1))
        return out


class _Replacements:
    """The replacements argument as daac_replace_all takes it: one blob + n + 1 offsets (host)."""

    def __init__(self, replacements):
        parts = [_as_bytes(replacements)] if isinstance(replacements, (str, bytes, bytearray, memoryview)) else [_as_bytes(x) for x in replacements]
        self.n = len(parts)
        self.offsets = np.zeros(self.n + 1, dtype=np.uint64)
        if parts:
            self.offsets[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        self.blob = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8)
        self.blob_ptr = self.blob.ctypes.data
        self.off_ptr = self.offsets.ctypes.data


class _Batch:
    """A batch argument: a sequence of documents (str / bytes / uint8 arrays), packed into one host buffer + n + 1 offsets, or a pair
    (uint8 CUDA tensor, int64 CUDA tensor of n + 1 offsets) that stays on the device; the offsets may also be the DeviceOffsets of
    split_batch or cut_batch, which are positions in that tensor."""

    def __init__(self, docs):
        if isinstance(docs, tuple) and len(docs) == 2 and hasattr(docs[0], "data_ptr") and isinstance(docs[1], DeviceOffsets):
            hay, off = docs
            if not hay.is_cuda or hay.dtype.itemsize != 1 or not hay.is_contiguous() or not off.ptr or off.count < 1:
                raise DaachorseError(1, "a device batch is (contiguous uint8 CUDA tensor, DeviceOffsets of n + 1 offsets that have not been freed)")
            if hay.numel() == 0:
                hay = _one_granule(hay)
            self.keep = (hay, off)
            self.hay, self.off, self.n, self.is_device = hay.data_ptr(), off.ptr, off.count - 1, 1
            return
        if isinstance(docs, tuple) and len(docs) == 2 and hasattr(docs[0], "data_ptr") and hasattr(docs[1], "data_ptr"):
            hay, off = docs
            if not (hay.is_cuda and off.is_cuda):
                raise DaachorseError(1, "a device batch is (uint8 CUDA tensor, int64 CUDA offsets tensor)")
            if hay.dtype.itemsize != 1 or not hay.is_contiguous() or off.dtype.itemsize != 8 or not off.is_contiguous() or off.dim() != 1 or off.numel() < 1:
                raise DaachorseError(1, "a device batch is (contiguous uint8 tensor, contiguous int64 tensor of n + 1 offsets)")
            if hay.numel() == 0:   # (documents that are all empty still need a buffer to point at)
                hay = _one_granule(hay)
            self.keep = (hay, off)
            self.hay = hay.data_ptr()
            self.off = off.data_ptr()
            self.n = off.numel() - 1
            self.is_device = 1
            return
        parts = []
        for d in docs:
            if isinstance(d, np.ndarray):
                if d.dtype.itemsize != 1:
                    raise DaachorseError(1, "a document array must have a 1-byte dtype (uint8)")
                parts.append(np.ascontiguousarray(d).view(np.uint8).tobytes())
            else:
                parts.append(_as_bytes(d))
        self.offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            self.offsets[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        self.buf = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8)
        self.keep = None
        self.hay = self.buf.ctypes.data
        self.off = self.offsets.ctypes.data
        self.n = len(parts)
        self.is_device = 0


class _DeviceBatch:
    """A batch the library made itself: device addresses of the text and of n + 1 offsets."""

    def __init__(self, hay, off, n):
        self.hay, self.off, self.n, self.is_device, self.keep = hay, off, n, 1, None


def _one_granule(t):
    """a 16-byte device buffer next to tensor t"""
    import torch
    return torch.zeros(16, dtype=torch.uint8, device=t.device)


def _device_u64(out, n):
    """(pointer, tensor) of a CUDA tensor of n 8-byte elements, for results left on the device"""
    if not (hasattr(out, "data_ptr") and out.is_cuda and out.dtype.itemsize == 8 and out.is_contiguous() and out.numel() >= n):
        raise DaachorseError(1, "device results go to a contiguous CUDA tensor of n int64 / uint64 elements")
    return out.data_ptr()


def _upload(b):
    """a host _Batch as the device batch (uint8 CUDA tensor, int64 CUDA offsets tensor)"""
    import torch
    return torch.tensor(b.buf).cuda(), torch.from_numpy(b.offsets.astype(np.int64)).cuda()


def _skip_flags(skip, n):
    """the skip argument of tokenize_wordpiece_batch -> (what keeps it alive, its device pointer or None)"""
    if skip is None:
        return None, None
    if isinstance(skip, DeviceMatches):
        if skip.count != n or skip.dtype.itemsize != 1:
            raise DaachorseError(1, f"skip has {skip.count} entries of {skip.dtype.itemsize} bytes for {n} words of one byte each")
        return skip, skip.ptr
    if hasattr(skip, "data_ptr") and hasattr(skip, "is_cuda"):
        t = skip
    else:
        a = np.ascontiguousarray(skip)
        if a.ndim != 1 or a.dtype.itemsize != 1:
            raise DaachorseError(1, "skip must be a one-dimensional array of one byte per word (uint8)")
        import torch
        t = torch.from_numpy(a.view(np.uint8).copy()).cuda()
    if not t.is_cuda or t.dtype.itemsize != 1 or not t.is_contiguous() or t.numel() != n:
        raise DaachorseError(1, f"skip must be a contiguous uint8 CUDA tensor of one byte per word ({n})")
    return t, (t.data_ptr() if n else None)


_WHITE_SPACE = (0x85, 0xA0, 0x1680) + tuple(range(0x2000, 0x200B)) + (0x2028, 0x2029, 0x202F, 0x205F, 0x3000)
_char_classes = None


def char_classes():
    """The default classes of the code points from U+0080 on, as split_batch takes them: a uint32 array [R, 3] of sorted, disjoint ranges
    {first, last, cls} with cls 1 = L (general categories L*), 2 = N (categories N*) and 3 = S (the non-ASCII White_Space code points:
    U+0085, U+00A0, U+1680, U+2000..U+200A, U+2028, U+2029, U+202F, U+205F, U+3000); every other code point is O.  The categories are
    the standard library's: Unicode `unicodedata.unidata_version` of the running Python.  Computed once and cached (read-only)."""
    global _char_classes
    if _char_classes is None:
        import unicodedata
        white = frozenset(_WHITE_SPACE)
        rows, first, cur = [], 0, 0
        for cp in range(0x80, 0x110001):
            c = 0
            if cp <= 0x10FFFF:
                c = 3 if cp in white else {"L": 1, "N": 2}.get(unicodedata.category(chr(cp))[0], 0)
            if c != cur:
                if cur:
                    rows.append((first, cp - 1, cur))
                first, cur = cp, c
        a = np.array(rows, dtype=np.uint32).reshape(len(rows), 3)
        a.setflags(write=False)
        _char_classes = a
    return _char_classes


_bert_char_classes = None


def bert_char_classes():
    """The classes of the code points from U+0080 on under which Split.Bert gives the words of BERT's pre-tokenizer (`tokenizers`'
    BertPreTokenizer): rows {first, last, cls} as char_classes() has them, with the White_Space code points in S (3), the general
    categories P* in no range (class O: BERT punctuation, every character a word of its own), N* in N (2) and every other code point in
    L (1) — M*, S*, C*, unassigned code points and the surrogates included, which BERT leaves inside words.  The categories are the
    standard library's (Unicode `unicodedata.unidata_version`).  Computed once and cached (read-only)."""
    global _bert_char_classes
    if _bert_char_classes is None:
        import unicodedata
        white = frozenset(_WHITE_SPACE)
        rows, first, cur = [], 0, 0
        for cp in range(0x80, 0x110001):
            c = 0
            if cp <= 0x10FFFF:
                c = 3 if cp in white else {"P": 0, "N": 2}.get(unicodedata.category(chr(cp))[0], 1)
            if c != cur:
                if cur:
                    rows.append((first, cp - 1, cur))
                first, cur = cp, c
        a = np.array(rows, dtype=np.uint32).reshape(len(rows), 3)
        a.setflags(write=False)
        _bert_char_classes = a
    return _bert_char_classes


_o200k_char_classes = None


def o200k_char_classes():
    """The classes of the code points from U+0080 on under which Split.O200k gives the words of tiktoken's o200k_base pattern: rows
    {first, last, cls} as char_classes() has them, with cls 1 = a caseless letter (general categories Lm, Lo), 2 = N (N*), 3 = S (the
    White_Space code points of char_classes()), 4 = an upper letter (Lu, Lt), 5 = a lower letter (Ll) and 6 = a mark (M*); every other
    code point is O.  The categories are the standard library's (Unicode `unicodedata.unidata_version`).  Computed once and cached
    (read-only)."""
    global _o200k_char_classes
    if _o200k_char_classes is None:
        import unicodedata
        white = frozenset(_WHITE_SPACE)
        cls_of = {"Lu": 4, "Lt": 4, "Ll": 5, "Lm": 1, "Lo": 1, "Mn": 6, "Mc": 6, "Me": 6, "Nd": 2, "Nl": 2, "No": 2}
        rows, first, cur = [], 0, 0
        for cp in range(0x80, 0x110001):
            c = 0
            if cp <= 0x10FFFF:
                c = 3 if cp in white else cls_of.get(unicodedata.category(chr(cp)), 0)
            if c != cur:
                if cur:
                    rows.append((first, cp - 1, cur))
                first, cur = cp, c
        a = np.array(rows, dtype=np.uint32).reshape(len(rows), 3)
        a.setflags(write=False)
        _o200k_char_classes = a
    return _o200k_char_classes


class Splitter:
    """daac_splitter: a split rule and the classes of the code points from U+0080 on (`classes`: rows {first, last, cls} as
    char_classes() gives them, the default (o200k_char_classes() under Split.O200k); sorted and disjoint, cls 1 = L, 2 = N, 3 = S, and
    under Split.O200k also 4 = upper, 5 = lower, 6 = mark, with 1 a caseless letter).  Below U+0080 the classes are fixed."""

    def __init__(self, rule=Split.Gpt2, classes=None):
        self._h = None
        a = (o200k_char_classes() if rule == Split.O200k else char_classes()) if classes is None else np.asarray(classes)
        if a.size and (a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise DaachorseError(1, "classes must be rows {first, last, cls} of integers in 0 .. 0xFFFFFFFF")
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 3)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().daac_splitter_create(int(rule), a.ctypes.data if a.size else None, a.shape[0], C.byref(h)))
        self._h, self.rule = h.value, int(rule)

    def _run(self, b, stream):
        wo, dw, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        if not self._h:
            raise DaachorseError(1, "the splitter has been freed")
        _ffi.check(_ffi.lib().daac_split_batch(self._h, b.hay, b.off, b.n, b.is_device, stream, C.byref(wo), C.byref(dw), C.byref(n)))
        return DeviceOffsets(wo.value, n.value + 1), DeviceOffsets(dw.value, b.n + 1)

    def split_batch(self, docs, stream=None, device=False):
        """-> (word_offsets, doc_words): word_offsets holds n_words + 1 positions in the batch's buffer (absolute: (hay, word_offsets) is a
        batch itself; entry 0 is the first document's offset, the last entry the end of the last document), document i's words are
        [doc_words[i], doc_words[i+1]); np.uint64 arrays, or DeviceOffsets (to_numpy / free) with device=True"""
        return _offsets_result(self._run(_Batch(docs), stream), device)

    def split(self, haystack, stream=None, device=False):
        """-> word_offsets of one haystack: n_words + 1 positions, from 0 to its length"""
        h = _Haystack(haystack)
        if not self._h:
            raise DaachorseError(1, "the splitter has been freed")
        wo, n = C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_split(self._h, h.ptr, h.len, h.is_device, stream, C.byref(wo), C.byref(n)))
        return _offsets_result([DeviceOffsets(wo.value, n.value + 1)], device)[0]

    def _words_space(self, hay_ptr, hay_is_device, wo_ptr, n_words, stream):
        if not self._h:
            raise DaachorseError(1, "the splitter has been freed")
        flags = C.c_void_p()
        _ffi.check(_ffi.lib().daac_split_words_space(self._h, hay_ptr, wo_ptr, n_words, hay_is_device, stream, C.byref(flags)))
        return DeviceMatches(flags.value, n_words if flags.value else 0, np.dtype(np.uint8))

    def words_space(self, words, stream=None, device=False):
        """`words` = (hay, word_offsets): a haystack (host bytes or a uint8 CUDA tensor) and the n_words + 1 absolute word offsets of
        split_batch in device memory (DeviceOffsets, or a contiguous int64 / uint64 CUDA tensor).  -> np.uint8[n_words], 1 where the
        word is not empty and its first unit is whitespace (under Split.Whitespace and Split.Bert: the word is whitespace); device=True:
        DeviceMatches of uint8 (to_numpy / free)"""
        if not (isinstance(words, tuple) and len(words) == 2):
            raise DaachorseError(1, "words_space takes (hay, word_offsets)")
        h, wo = _Haystack(words[0]), words[1]
        if isinstance(wo, DeviceOffsets):
            p, cnt = wo.ptr, wo.count
        elif hasattr(wo, "data_ptr") and wo.is_cuda and wo.dtype.itemsize == 8 and wo.is_contiguous() and wo.dim() == 1:
            p, cnt = wo.data_ptr(), wo.numel()
        else:
            raise DaachorseError(1, "word_offsets are DeviceOffsets or a contiguous one-dimensional CUDA tensor of int64 / uint64")
        if cnt < 1:
            raise DaachorseError(1, "word_offsets hold n_words + 1 entries")
        out = self._words_space(h.ptr, h.is_device, p, cnt - 1, stream)
        if device:
            return out
        try:
            return out.to_numpy()
        finally:
            out.free()

    def free(self):
        if self._h:
            _ffi.lib().daac_splitter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _offsets_result(dev, device):
    if device:
        return tuple(dev)
    try:
        return tuple(o.to_numpy() for o in dev)
    finally:
        for o in dev:
            o.free()


_default_splitters = {}


def _default_splitter(rule):
    rule = Split(rule) if rule in (0, 1, 3, 4, 6, 8) else rule
    sp = _default_splitters.get(rule)
    if sp is None:
        sp = _default_splitters[rule] = Splitter(rule, bert_char_classes() if rule == Split.Bert else None)
    return sp


WORDPIECE_NONE = 0xFFFFFFFF   # in first_ids / cont_ids: no such piece


def wordpiece_tables(vocab, prefix="##"):
    """A WordPiece vocabulary {piece: id} (str or bytes keys) -> (patterns, first_ids, cont_ids) for tokenize_wordpiece*: `patterns` is
    the sorted set of every key's bytes together with every key that starts with `prefix` and is longer than it, with the prefix
    removed; first_ids[i] = vocab.get(patterns[i], 0xFFFFFFFF) and cont_ids[i] = vocab.get(prefix + patterns[i], 0xFFFFFFFF)
    (np.uint32) — `tokenizers`' lookup: a key such as ##s is also an initial piece of the literal word "##s".  The automaton is
    DoubleArrayAhoCorasick.new(patterns) (or the charwise one), where a pattern's value is its index."""
    pre = _as_bytes(prefix)
    if not pre:
        raise DaachorseError(1, "prefix must not be empty")
    v = {}
    for key, i in vocab.items():
        k = _as_bytes(key)
        if not 0 <= int(i) < WORDPIECE_NONE:
            raise DaachorseError(1, f"the id of {key!r} is not in 0 .. 0xFFFFFFFE")
        if not k or k in v:
            raise DaachorseError(1, f"the piece {key!r} is empty or comes twice")
        v[k] = int(i)
    patterns = sorted(set(v) | {k[len(pre):] for k in v if k.startswith(pre) and len(k) > len(pre)})
    first = np.array([v.get(s, WORDPIECE_NONE) for s in patterns], dtype=np.uint32)
    cont = np.array([v.get(pre + s, WORDPIECE_NONE) for s in patterns], dtype=np.uint32)
    return patterns, first, cont


def split_batch(docs, rule=Split.Gpt2, stream=None, device=False):
    """Splitter(rule).split_batch(docs) on a cached splitter with the rule's default classes (char_classes(); Split.Bert:
    bert_char_classes(); Split.O200k: o200k_char_classes())"""
    return _default_splitter(rule).split_batch(docs, stream=stream, device=device)


def offsets_compose(inner, outer, stream=None, device=False):
    """daac_offsets_compose: inner[outer] of two device arrays of 8-byte offsets (DeviceOffsets, or contiguous int64 / uint64 CUDA
    tensors) -> np.uint64[len(outer)], or DeviceOffsets with device=True"""
    def arg(x):
        if isinstance(x, DeviceOffsets):
            return x.ptr, x.count
        if not (hasattr(x, "data_ptr") and x.is_cuda and x.dtype.itemsize == 8 and x.is_contiguous() and x.dim() == 1):
            raise DaachorseError(1, "offsets_compose takes DeviceOffsets or contiguous one-dimensional CUDA tensors of int64 / uint64")
        return x.data_ptr(), x.numel()

    (p_in, _), (p_out, n) = arg(inner), arg(outer)
    out = C.c_void_p()
    _ffi.check(_ffi.lib().daac_offsets_compose(p_in, p_out, n, stream, C.byref(out)))
    return _offsets_result([DeviceOffsets(out.value, n)], device)[0]


# ---- special tokens in raw text (daac_cut_batch / daac_tokens_splice): `tokenizers`' added tokens with special=True, tiktoken's
# allowed_special.  They are found in the raw text, leftmost-longest, in front of the normalizer; each is one token with its own id and
# every stretch of text between them is tokenized as a string of its own.
SEGMENT_TEXT = 0xFFFFFFFF   # in seg_values: a text segment


class SpecialTokens:
    """The special tokens of a vocabulary: `tokens` is a {text: id} mapping or a sequence of (text, id), text str or bytes, ids in
    0 .. 0xFFFFFFFE.  `.pma` is the automaton: a DoubleArrayAhoCorasick with MatchKind.LeftmostLongest and value = id.  (An automaton
    built elsewhere, a charwise one for instance, is taken as it is: the C call checks it.)"""

    def __init__(self, tokens):
        if isinstance(tokens, DoubleArrayAhoCorasick):
            self.pma, self.tokens = tokens, None
            return
        items = list(tokens.items()) if hasattr(tokens, "items") else [tuple(t) for t in tokens]
        seen = {}
        for text, i in items:
            t = _as_bytes(text)
            if not t:
                raise DaachorseError(1, "a special token is empty")
            if t in seen:
                raise DaachorseError(1, f"the special token {text!r} comes twice")
            if not 0 <= int(i) < SEGMENT_TEXT:
                raise DaachorseError(1, f"the id of {text!r} is not in 0 .. 0xFFFFFFFE")
            seen[t] = int(i)
        self.tokens = seen
        self.pma = DoubleArrayAhoCorasickBuilder().match_kind(MatchKind.LeftmostLongest).build_with_values(seen.items())

    def _cut(self, b, engine, stream):
        """-> (seg_offsets, doc_segs, seg_values) of the batch b, in device memory"""
        so, ds, sv, n, k = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_cut_batch(self.pma._h, int(engine), b.hay, b.off, b.n, b.is_device, stream, C.byref(so), C.byref(ds), C.byref(sv),
                                             C.byref(n), C.byref(k)))
        values = DeviceMatches(sv.value, n.value, np.dtype(np.uint32))
        values.n_special = k.value
        return DeviceOffsets(so.value, n.value + 1), DeviceOffsets(ds.value, b.n + 1), values

    def cut_batch(self, docs, engine=Engine.Auto, stream=None, device=False):
        """-> (seg_offsets, doc_segs, seg_values): the documents cut at the special tokens.  seg_offsets holds n_segs + 1 positions in
        the batch's buffer (absolute: (hay, seg_offsets) is a batch itself), document i's segments are [doc_segs[i], doc_segs[i+1]) and
        seg_values[s] is the special's id or SEGMENT_TEXT; no segment is empty.  np.uint64, np.uint64 and np.uint32 arrays, or
        DeviceOffsets, DeviceOffsets and DeviceMatches (to_numpy / free) with device=True"""
        return _offsets_result(self._cut(_Batch(docs), engine, stream), device)


def _splice(ids, spans, seg_tok, cut, doc_off, n_docs, stream):
    """daac_tokens_splice over device addresses -> [ids, spans?, doc_tok] in device memory"""
    (p_so, n_so), (p_ds, n_ds), (p_sv, n_sv) = _device_ptr(cut[0], 8, "seg_offsets"), _device_ptr(cut[1], 8, "doc_segs"), _device_ptr(cut[2], 4, "seg_values")
    p_st, n_st = _device_ptr(seg_tok, 8, "seg_tok")
    n_segs = n_so - 1
    if n_segs < 0 or n_sv != n_segs or n_st != n_segs + 1 or n_ds != n_docs + 1:
        raise DaachorseError(1, f"seg_offsets and seg_tok hold n_segs + 1 entries, seg_values n_segs and doc_segs n + 1 = {n_docs + 1}")
    p_ids = _device_ptr(ids, 4, "ids")[0] if ids is not None else None
    p_sp = _device_ptr(spans, 8, "spans")[0] if spans is not None else None
    oi, os_, dt, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.lib().daac_tokens_splice(p_ids, p_sp, p_st, p_sv, p_so, p_ds, doc_off, n_segs, n_docs, stream, C.byref(oi),
                                             C.byref(os_) if spans is not None else None, C.byref(dt), C.byref(n)))
    out = [DeviceMatches(oi.value, n.value, np.dtype(np.uint32))]
    if spans is not None:
        out.append(DeviceMatches(os_.value, n.value, SPAN_DTYPE))
    out.append(DeviceOffsets(dt.value, n_docs + 1))
    return out


def splice_special(ids, spans, seg_tok, cut, docs, stream=None, device=False):
    """daac_tokens_splice: what a tokenizer made of the segment batch of SpecialTokens.cut_batch(docs, device=True), put back together
    per document.  `ids` (uint32), `spans` (pairs of 8-byte offsets relative to the segment, or None) and `seg_tok` (n_segs + 1 token
    offsets per segment) are that tokenizer's results in device memory (DeviceMatches / DeviceOffsets, or contiguous CUDA tensors),
    `cut` the three results of cut_batch, `docs` the batch it was given.  A text segment's tokens are copied, a special segment is the
    one token of its id whatever lies under it, and spans count from the document's first byte.  -> (ids, doc_tok) or (ids, spans,
    doc_tok): np.uint32[T], np.uint64[T, 2], np.uint64[n + 1]; device=True: DeviceMatches, DeviceMatches, DeviceOffsets"""
    if not (isinstance(cut, (tuple, list)) and len(cut) == 3):
        raise DaachorseError(1, "cut is (seg_offsets, doc_segs, seg_values) as cut_batch(device=True) gives them")
    b = _Batch(docs)
    off, keep = b.off, None
    if not b.is_device:
        import torch
        keep = torch.from_numpy(b.offsets.astype(np.int64)).cuda()
        off = keep.data_ptr()
    return _offsets_result(_splice(ids, spans, seg_tok, cut, off, b.n, stream), device)


def _special_docs(b, special, spans, stream, chain):
    """cut the device batch b, run `chain` (segment batch -> ([ids, spans?, seg_tok], n_matches)) and splice -> ([ids, spans?, doc_tok], n_matches)"""
    if not isinstance(special, SpecialTokens):
        raise DaachorseError(1, "special is None or a SpecialTokens")
    cut = special._cut(b, Engine.Auto, stream)
    try:
        out, k = chain(_DeviceBatch(b.hay, cut[0].ptr, cut[0].count - 1))
        try:
            return _splice(out[0], out[1] if spans else None, out[-1], cut, b.off, b.n, stream), k
        finally:
            for o in out:
                o.free()
    finally:
        for o in cut:
            o.free()


# ---- model inputs (daac_tokens_pack): `tokenizers`' TemplateProcessing + enable_truncation + enable_padding over a token result that is
# already in device memory: the template's special tokens around what truncation keeps, padded into the planes a model reads.
_PACK_KINDS = {"special": 0, "a": 1, "b": 2, 0: 0, 1: 1, 2: 2}
_PACK_STRATEGIES = {"longest_first": 0, "only_first": 1, "only_second": 2}
_PACK_SIDES = {"right": 0, "left": 1}


def bert_template(cls_id, sep_id):
    """-> (single, pair): [CLS] A [SEP] and [CLS] A [SEP] B [SEP], type ids 0 for the first half and 1 for B and its [SEP]"""
    single = [("special", cls_id, 0), ("A", 0, 0), ("special", sep_id, 0)]
    return single, single + [("B", 0, 1), ("special", sep_id, 1)]


def roberta_template(bos_id, eos_id):
    """-> (single, pair): <s> A </s> and <s> A </s> </s> B </s>, every type id 0"""
    single = [("special", bos_id, 0), ("A", 0, 0), ("special", eos_id, 0)]
    return single, single + [("special", eos_id, 0), ("B", 0, 0), ("special", eos_id, 0)]


class Packer:
    """daac_tokens_pack's parameters.  `single` and `pair` are templates: lists of pieces (kind, id, type_id) with kind "special", "A" or
    "B" (at most 16; A exactly once in each, B exactly once in `pair` and never in `single`); `single` may also be the (single, pair) of
    bert_template() / roberta_template(), and None is the template of A alone.  `max_length`: None (no truncation) or the longest row,
    special tokens included; `strategy` "longest_first", "only_first" or "only_second"; `truncation_side` "right" keeps a sequence's
    first tokens, "left" its last.  `padding`: "longest", an int (rows of at least that length) or None (no padding: the CSR form);
    `pad_to_multiple_of` rounds the row length up; `padding_side`, `pad_id`, `pad_type_id` as in `tokenizers`.  `dtype`: np.int64 or
    np.int32, the planes' element.  The C call checks the rules and answers in the header's order."""

    def __init__(self, single=None, pair=None, max_length=None, strategy="longest_first", truncation_side="right", padding="longest",
                 pad_to_multiple_of=None, padding_side="right", pad_id=0, pad_type_id=0, dtype=np.int64):
        if pair is None and isinstance(single, tuple) and len(single) == 2 and all(isinstance(t, list) for t in single):
            single, pair = single
        p = _ffi.PackParams()
        p.struct_size = C.sizeof(_ffi.PackParams)
        p.n_single = self._pieces(p.single, [("A", 0, 0)] if single is None else single, "single")
        p.n_pair = self._pieces(p.pair, [] if pair is None else pair, "pair")
        if strategy not in _PACK_STRATEGIES or truncation_side not in _PACK_SIDES or padding_side not in _PACK_SIDES:
            raise DaachorseError(1, "strategy is longest_first, only_first or only_second, and a side is left or right")
        if max_length is not None:
            p.truncate, p.max_length = 1, self._u64(max_length, "max_length")
        p.strategy, p.truncate_left, p.pad_left = _PACK_STRATEGIES[strategy], _PACK_SIDES[truncation_side], _PACK_SIDES[padding_side]
        if padding is None:
            p.padding = 0
        elif isinstance(padding, str):
            if padding != "longest":
                raise DaachorseError(1, 'padding is "longest", a length or None')
            p.padding = 1
        else:
            p.padding, p.pad_length = 2, self._u64(padding, "padding")
        p.pad_multiple = 1 if pad_to_multiple_of is None else self._u64(pad_to_multiple_of, "pad_to_multiple_of")
        p.pad_id, p.pad_type_id = self._u32(pad_id, "pad_id"), self._u32(pad_type_id, "pad_type_id")
        self.dtype = np.dtype(dtype)
        p.width = self.dtype.itemsize if self.dtype.kind in "iu" else 0   # (the C call refuses what is not 4 or 8)
        self.params, self.csr = p, p.padding == 0

    @staticmethod
    def _u32(x, what):
        if not 0 <= int(x) <= 0xFFFFFFFF:
            raise DaachorseError(1, f"{what} must be in 0 .. 0xFFFFFFFF")
        return int(x)

    @staticmethod
    def _u64(x, what):
        if isinstance(x, bool) or not 0 <= int(x) < 1 << 64:
            raise DaachorseError(1, f"{what} must be an integer in 0 .. 2^64 - 1")
        return int(x)

    @classmethod
    def _pieces(cls, dst, pieces, name):
        pieces = list(pieces)
        if len(pieces) > _ffi.PACK_MAX_PIECES:
            raise DaachorseError(1, f"the {name} template has {len(pieces)} pieces: at most {_ffi.PACK_MAX_PIECES}")
        for i, pc in enumerate(pieces):
            kind, tok, type_id = pc
            k = _PACK_KINDS.get(kind.lower() if isinstance(kind, str) else kind)
            if k is None:
                raise DaachorseError(1, f'the {name} template: piece {i} is of kind {kind!r}, not "special", "A" or "B"')
            dst[i].kind, dst[i].id, dst[i].type_id = k, cls._u32(tok, "a piece's id"), cls._u32(type_id, "a piece's type_id")
        return len(pieces)

    @staticmethod
    def _sequence(seq, name, keep):
        """(ids, offsets) or (ids, spans, offsets) -> (ids address, spans address or None, offsets address, tokens, documents)"""
        if not (isinstance(seq, (tuple, list)) and len(seq) in (2, 3)):
            raise DaachorseError(1, f"{name} is (ids, offsets) or (ids, spans, offsets)")
        ids, spans, off = (seq[0], None, seq[1]) if len(seq) == 2 else seq

        def dev(x, dtype, itemsize, what):
            if isinstance(x, np.ndarray) or isinstance(x, (list, tuple)):
                import torch
                a = np.ascontiguousarray(x, dtype=dtype)
                t = torch.from_numpy(a.view(np.int32 if itemsize == 4 else np.int64).copy()).cuda()
                keep.append(t)
                return (t.data_ptr() if t.numel() else None), t.numel()
            return _device_ptr(x, itemsize, what)

        p_ids, n_tok = dev(ids, np.uint32, 4, f"{name}: ids")
        p_off, n_off = dev(off, np.uint64, 8, f"{name}: offsets")
        p_sp = None
        if spans is not None:
            p_sp, n_sp = dev(spans, np.uint64, 8, f"{name}: spans")
            if n_sp != 2 * n_tok:
                raise DaachorseError(1, f"{name}: {n_tok} ids and {n_sp} span words: a pair a token")
        if n_off < 1 or (n_off > 1 and not p_off):
            raise DaachorseError(1, f"{name}: offsets hold n + 1 entries and have not been freed")
        return p_ids if n_tok else None, p_sp if n_tok else None, p_off, n_tok, n_off - 1

    def _run(self, a, b, stream):
        """the call over device addresses -> {plane: DeviceMatches / DeviceOffsets} with .shape = (n, L), or (R,) in the CSR form"""
        keep = []
        a_ids, a_sp, a_off, a_tok, n = self._sequence(a, "a", keep)
        b_ids = b_sp = b_off = None
        b_tok = 0
        with_spans = a_sp is not None or (len(a) == 3 and a_tok == 0)
        if b is not None:
            b_ids, b_sp, b_off, b_tok, n_b = self._sequence(b, "b", keep)
            if n_b != n:
                raise DaachorseError(1, f"a holds {n} documents and b {n_b}: a batch of pairs has one of each")
            if n == 0 and not b_off:
                raise DaachorseError(1, "b: offsets hold n + 1 entries and have not been freed")
            with_spans = with_spans and (b_sp is not None or (len(b) == 3 and b_tok == 0))
        ii, ti, am, sm, of, ro, L, slots = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_tokens_pack(C.byref(self.params), a_ids, a_sp, a_off, a_tok, b_ids, b_sp, b_off, b_tok, n, stream, C.byref(ii), C.byref(ti),
                                               None if self.csr else C.byref(am), C.byref(sm), C.byref(of) if with_spans else None,
                                               C.byref(ro) if self.csr else None, C.byref(L), C.byref(slots)))
        del keep
        shape = (slots.value,) if self.csr else (n, L.value)

        def plane(p, dtype):
            if self.csr:
                m = DeviceMatches(p.value, slots.value, dtype)
            else:   # a row an element: [n, L] through to_numpy
                m = DeviceMatches(p.value, n if L.value else 0, np.dtype((dtype, (L.value,))) if L.value else dtype)
            m.shape = shape + dtype.shape
            return m

        out = {"input_ids": plane(ii, self.dtype), "token_type_ids": plane(ti, self.dtype)}
        if not self.csr:
            out["attention_mask"] = plane(am, self.dtype)
        out["special_tokens_mask"] = plane(sm, self.dtype)
        if with_spans:
            out["offsets"] = plane(of, SPAN_DTYPE)
        if self.csr:
            out["row_offsets"] = DeviceOffsets(ro.value, n + 1)
        return out

    @staticmethod
    def _result(out, device):
        if device:
            return out
        try:
            return {k: v.to_numpy().reshape(v.shape) if isinstance(v, DeviceMatches) else v.to_numpy() for k, v in out.items()}
        finally:
            for v in out.values():
                v.free()

    def pack(self, a, b=None, stream=None, device=False):
        """`a` and `b` are (ids, offsets) or (ids, spans, offsets) of n documents each, as the token calls return them with device=True
        (DeviceMatches / DeviceOffsets), contiguous CUDA tensors, or numpy arrays, which are uploaded; b=None: a batch of singles.
        -> {"input_ids", "token_type_ids", "attention_mask", "special_tokens_mask"} of shape [n, L] and, with spans, "offsets" [n, L, 2]
        (np.uint64); without padding the planes are flat [R], there is no attention mask and "row_offsets" holds n + 1 np.uint64.
        device=True: the same as DeviceMatches / DeviceOffsets (to_numpy / free; .shape is the plane's), left in device memory"""
        return self._result(self._run(a, b, stream), device)


def _pack_docs(pack, out, stream, device):
    """what tokenize_*_docs made ([ids, spans?, doc_offsets] in device memory) through pack, the token result freed"""
    try:
        res = pack._run(tuple(out), None, stream)
    finally:
        for o in out:
            o.free()
    return Packer._result(res, device)


# ---- token ids back to text (daac_decoder_create / daac_tokens_decode): `tokenizers`' decoders as one rule over a table of images, for a
# token result or a plane of ids that is already in device memory.
DECODE_SPECIAL, DECODE_ABSENT = 1, 2   # DAAC_DECODE_SPECIAL, DAAC_DECODE_ABSENT
_WORDPIECE_CLEANUP = ((b" .", b"."), (b" ?", b"?"), (b" !", b"!"), (b" ,", b","), (b" ' ", b"'"), (b" n't", b"n't"), (b" 'm", b"'m"), (b" do not", b" don't"),
                      (b" 's", b"'s"), (b" 've", b"'ve"), (b" 're", b"'re"))   # `tokenizers`' cleanup, in its order


class Decoder:
    """daac_decoder: a table of images over the ids 0 .. n_ids - 1.  `rest` is a sequence indexed by id, or a {id: image} mapping, of
    str / bytes images (None, or an id the mapping leaves out: the id has no entry); `first` likewise, the image a token takes as the
    first KEPT token of its document (None: `rest` throughout; an id it leaves out takes its rest image).  `special`: the ids that
    skip_special_tokens leaves out, or a SpecialTokens, whose ids are flagged and whose images are the specials' own text.  A
    document's text is first[k_0] + rest[k_1] + rest[k_2] + ... over its kept tokens: bytes, never validated or replaced as UTF-8.
    byte_level(), wordpiece() and metaspace() build the tables of `tokenizers`' decoders."""

    def __init__(self, rest, first=None, special=()):
        self._h = None
        r, f = self._images(rest, "rest"), ({} if first is None else self._images(first, "first"))
        ids, texts = self._special(special)
        for i, t in texts.items():
            r[i] = t
            f.pop(i, None)
        if set(f) - set(r):
            raise DaachorseError(1, f"first has an image for id {min(set(f) - set(r))}, which has no rest image")
        n = max(list(r) + list(ids), default=-1) + 1
        pieces, flags, pool, seen = np.zeros((n, 4), dtype=np.uint32), np.full(n, DECODE_ABSENT, dtype=np.uint8), bytearray(), {}

        def place(img):
            at = seen.get(img)
            if at is None:
                at = seen[img] = len(pool)
                pool.extend(img)
            return at, len(img)

        for i, img in r.items():
            pieces[i, 0:2] = place(img)
            pieces[i, 2:4] = place(f.get(i, img))
            flags[i] = 0
        for i in ids:
            flags[i] |= DECODE_SPECIAL
        if len(pool) >= 1 << 32:
            raise DaachorseError(1, f"the images take {len(pool)} bytes: the pool is below 4 GiB")
        self.n_ids, self.pool_bytes = n, len(pool)
        self.rest, self.first, self.special = r, f, frozenset(ids)
        pool_arr = np.frombuffer(bytes(pool) or b"\0", dtype=np.uint8)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().daac_decoder_create(pool_arr.ctypes.data, len(pool), pieces.ctypes.data if n else None, flags.ctypes.data if n else None, n,
                                                  C.byref(h)))
        self._h = h.value

    @staticmethod
    def _images(x, what):
        items = x.items() if hasattr(x, "items") else enumerate(x)
        out = {}
        for i, img in items:
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < SEGMENT_TEXT:
                raise DaachorseError(1, f"{what}: the id {i!r} is not in 0 .. 0xFFFFFFFE")
            if img is not None:
                out[int(i)] = _as_bytes(img)
        return out

    @staticmethod
    def _special(special):
        """-> (the flagged ids, {id: text} of a SpecialTokens)"""
        if isinstance(special, SpecialTokens):
            if special.tokens is None:
                raise DaachorseError(1, "special: a SpecialTokens made from an automaton has no texts; give the ids")
            return sorted(special.tokens.values()), {i: t for t, i in special.tokens.items()}
        ids = []
        for i in special:
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < SEGMENT_TEXT:
                raise DaachorseError(1, f"special: ids in 0 .. 0xFFFFFFFE or a SpecialTokens, not {i!r}")
            ids.append(int(i))
        return sorted(set(ids)), {}

    @staticmethod
    def _by_id(pieces, what):
        """a vocabulary as {piece: id}, or a sequence of pieces indexed by id -> {id: the piece's bytes}"""
        out = {}
        for k, i in (pieces.items() if hasattr(pieces, "items") else ((p, i) for i, p in enumerate(pieces))):
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < SEGMENT_TEXT:
                raise DaachorseError(1, f"{what}: the id of {k!r} is not in 0 .. 0xFFFFFFFE")
            if int(i) in out:
                raise DaachorseError(1, f"{what}: the id {i} comes twice")
            out[int(i)] = _as_bytes(k)
        return out

    @classmethod
    def _build(cls, table, special, rest_of, first_of):
        ids, texts = cls._special(special)
        table.update(texts)   # a special goes through the decoder as any token does: `tokenizers` prints it that way
        return cls({i: rest_of(p) for i, p in table.items()}, {i: first_of(p) for i, p in table.items()}, ids)

    @classmethod
    def byte_level(cls, pieces, gap_id=None, special=()):
        """Byte-level BPE and tiktoken-style rank files: first = rest = the piece's raw bytes, the patterns of the automaton.  `pieces`
        is {piece: id} or a sequence indexed by id; with `gap_id` the ids gap_id + b are the single byte b (Gap.Bytes)."""
        table = cls._by_id(pieces, "pieces")
        if gap_id is not None:
            if isinstance(gap_id, bool) or not 0 <= int(gap_id) <= SEGMENT_TEXT - 256:
                raise DaachorseError(1, "gap_id + 255 must be in 0 .. 0xFFFFFFFE")
            for b in range(256):
                table.setdefault(int(gap_id) + b, bytes([b]))
        return cls._build(table, special, lambda p: p, lambda p: p)

    @classmethod
    def wordpiece(cls, vocab, prefix="##", cleanup=True, special=()):
        """`tokenizers`' decoders.WordPiece: rest is the piece without its prefix, or " " + piece; first is the piece as written (a
        leading prefix stays); with cleanup the eleven replacements are applied to each image."""
        pre = _as_bytes(prefix)

        def clean(img):
            if cleanup:
                for old, new in _WORDPIECE_CLEANUP:
                    img = img.replace(old, new)
            return img

        return cls._build(cls._by_id(vocab, "vocab"), special, lambda p: clean(p[len(pre):] if pre and p.startswith(pre) else b" " + p), clean)

    @classmethod
    def metaspace(cls, pieces, replacement="▁", prepend_scheme="always", byte_fallback=False, special=(), first=None):
        """Metaspace / SentencePiece: every `replacement` in the piece becomes a space; with byte_fallback a piece <0xHH> is the byte
        HH.  Under prepend_scheme "always" or "first" the first image differs, in one of two ways: first="strip_one" takes one leading
        space off (Llama-2's Sequence([Replace, ByteFallback, Fuse, Strip(" ", 1, 0)]); the default with byte_fallback), and
        first="drop_all" leaves out every `replacement` of the piece (what `tokenizers`' decoders.Metaspace does to token 0; the
        default without byte_fallback).  The two agree on every piece whose only `replacement` is a leading one."""
        rep = _as_bytes(replacement)
        if prepend_scheme not in ("always", "first", "never") or first not in (None, "strip_one", "drop_all") or not rep:
            raise DaachorseError(1, 'prepend_scheme is "always", "first" or "never", first "strip_one", "drop_all" or None, and replacement is not empty')
        how = first or ("strip_one" if byte_fallback else "drop_all")
        hexd = b"0123456789ABCDEFabcdef"

        def byte_of(p):
            if byte_fallback and len(p) == 6 and p[:3] == b"<0x" and p[5:] == b">" and p[3] in hexd and p[4] in hexd:
                return bytes([int(p[3:5], 16)])
            return None

        def rest_of(p):
            b = byte_of(p)
            return b if b is not None else p.replace(rep, b" ")

        def first_of(p):
            if prepend_scheme == "never":
                return rest_of(p)
            if how == "drop_all" and byte_of(p) is None:
                return p.replace(rep, b"")
            img = rest_of(p)
            return img[1:] if img.startswith(b" ") else img

        return cls._build(cls._by_id(pieces, "pieces"), special, rest_of, first_of)

    @staticmethod
    def _upload(a, keep):
        import torch
        t = torch.from_numpy(a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()).cuda()
        keep.append(t)
        return t.data_ptr() if t.numel() else None

    @classmethod
    def _tokens(cls, tokens, keep):
        """-> (ids address, element width, offsets address or None, tokens, documents, row length)"""
        if isinstance(tokens, (tuple, list)):
            if len(tokens) not in (2, 3):
                raise DaachorseError(1, "a CSR token result is (ids, offsets) or (ids, spans, offsets)")
            ids, off = tokens[0], tokens[-1]
            host_ids, host_off = isinstance(ids, (np.ndarray, list, tuple)), isinstance(off, (np.ndarray, list, tuple))
            if host_ids:   # (both are looked at before either is uploaded)
                a = np.asarray(ids)
                if a.ndim != 1 or (a.size and (a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 0xFFFFFFFF)):
                    raise DaachorseError(1, "ids of a CSR token result are one-dimensional integers in 0 .. 0xFFFFFFFF")
                a = np.ascontiguousarray(a, dtype=np.uint32)
            if host_off:
                o = np.asarray(off)
                if o.ndim != 1 or o.size < 1 or o.dtype.kind not in "iu" or (o.dtype.kind == "i" and o.min() < 0):
                    raise DaachorseError(1, "offsets hold n + 1 non-negative integers")
                o = np.ascontiguousarray(o, dtype=np.uint64)
            p_ids, n_tok = (cls._upload(a, keep), a.size) if host_ids else _device_ptr(ids, 4, "ids")
            p_off, n_off = (cls._upload(o, keep), o.size) if host_off else _device_ptr(off, 8, "offsets")
            if n_off < 1 or not p_off:
                raise DaachorseError(1, "offsets hold n + 1 entries and have not been freed")
            return (p_ids if n_tok else None), 4, p_off, n_tok, n_off - 1, 0
        x = tokens
        if isinstance(x, DeviceMatches):
            shape = getattr(x, "shape", None)
            if shape is None or len(shape) != 2 or x.dtype.base.kind not in "iu" or x.dtype.base.itemsize not in (4, 8):
                raise DaachorseError(1, "a DeviceMatches plane has .shape == (n, L) and int32 / uint32 / int64 elements")
            if shape[0] * shape[1] and not x.ptr:
                raise DaachorseError(1, "the plane has been freed")
            return x.ptr, x.dtype.base.itemsize, None, shape[0] * shape[1], shape[0], shape[1]
        if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):
            if not x.is_cuda or x.dim() != 2 or not x.is_contiguous() or x.dtype.is_floating_point or x.dtype.itemsize not in (4, 8):
                raise DaachorseError(1, "a plane of ids is a contiguous two-dimensional CUDA tensor of int32 / uint32 / int64")
            return (x.data_ptr() if x.numel() else None), x.dtype.itemsize, None, x.numel(), x.shape[0], x.shape[1]
        if isinstance(x, np.ndarray):
            if x.ndim != 2 or x.dtype not in (np.dtype(np.int32), np.dtype(np.uint32), np.dtype(np.int64)):
                raise DaachorseError(1, "a plane of ids is a two-dimensional array of int32 / uint32 / int64")
            a = np.ascontiguousarray(x)
            return cls._upload(a.reshape(-1), keep), a.dtype.itemsize, None, a.size, a.shape[0], a.shape[1]
        raise DaachorseError(1, "tokens is (ids, offsets), (ids, spans, offsets) or one two-dimensional plane of ids")

    def _run(self, tokens, skip_special_tokens, unknown, token_starts, stream):
        """-> [text (uint8), out_offsets] or [text, out_offsets, token_starts], in device memory"""
        if not self._h:
            raise DaachorseError(1, "the decoder has been freed")
        if unknown not in ("error", "skip"):
            raise DaachorseError(1, 'unknown is "error" or "skip"')
        keep = []
        p_ids, width, p_off, n_tok, n, L = self._tokens(tokens, keep)
        out, oo, ts, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_tokens_decode(self._h, p_ids, width, p_off, n_tok, n, L, int(bool(skip_special_tokens)), int(unknown == "skip"), stream,
                                                 C.byref(out), C.byref(oo), C.byref(ts) if token_starts else None, C.byref(nb)))
        del keep
        res = [DeviceMatches(out.value, nb.value, np.dtype(np.uint8)), DeviceOffsets(oo.value, n + 1)]
        if token_starts:
            res.append(DeviceOffsets(ts.value, n_tok + 1 if ts.value else 0))
        return res

    def decode_batch(self, tokens, skip_special_tokens=True, unknown="error", token_starts=False, stream=None, device=False):
        """`tokens` is (ids, offsets) or (ids, spans, offsets) as every token call returns them (DeviceMatches / DeviceOffsets,
        contiguous CUDA tensors, or numpy arrays, which are uploaded; the spans are not read), or one [n, L] plane of ids: a
        DeviceMatches with .shape == (n, L) as Packer leaves it, a contiguous CUDA tensor or a numpy array of int32 / uint32 / int64,
        where an int64 outside 0 .. 2^32 - 1 (-100) is an id without an entry.  unknown="error" refuses the batch at its lowest such
        token, "skip" leaves them out as `tokenizers` does.  -> a list of bytes, one per document; with token_starts=True (that list,
        np.uint64[T + 1]: where each token's image begins in the concatenated text).  device=True: (DeviceMatches uint8,
        DeviceOffsets), a batch again that goes into tokenize_*_docs or normalize_batch, and the starts as DeviceOffsets"""
        res = self._run(tokens, skip_special_tokens, unknown, token_starts, stream)
        if device:
            return tuple(res)
        try:
            text, off = res[0].to_numpy().tobytes(), res[1].to_numpy()
            docs = [text[int(off[d]):int(off[d + 1])] for d in range(len(off) - 1)]
            return (docs, res[2].to_numpy()) if token_starts else docs
        finally:
            for r in res:
                r.free()

    def decode(self, ids, skip_special_tokens=True, unknown="error", stream=None):
        """one document's ids (a sequence of integers, or a one-dimensional array or CUDA tensor of 4-byte ids) -> bytes"""
        if hasattr(ids, "data_ptr"):
            import torch
            off = torch.tensor([0, ids.numel()], dtype=torch.int64, device=ids.device)
        else:
            ids = np.asarray(ids if isinstance(ids, np.ndarray) else list(ids))
            ids = ids.astype(np.uint32) if ids.size == 0 else ids   # (an empty list has no integer dtype of its own)
            off = np.array([0, ids.size], dtype=np.uint64)
        return self.decode_batch((ids, off), skip_special_tokens=skip_special_tokens, unknown=unknown, stream=stream)[0]

    def free(self):
        if self._h:
            _ffi.lib().daac_decoder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Norm(enum.IntEnum):
    """daac_norm_kind: what a Normalizer's rule does to the code points of its range"""
    Delete = 1     # the code point is removed
    Replace = 2    # its image is pool[off : off + len]
    Pad = 3        # 0x20, the character itself, 0x20
    Hangul = 4     # the arithmetic decomposition of a Hangul syllable into jamo (inside U+AC00 .. U+D7A3 only)


NORM_MAX_LEN = 255   # the longest image of a Replace rule, in bytes


def _device_ptr(x, itemsize, what):
    """(address, elements) of a DeviceMatches, DeviceOffsets or contiguous CUDA tensor with elements of `itemsize` bytes"""
    if isinstance(x, DeviceOffsets):
        if itemsize != 8:
            raise DaachorseError(1, f"{what}: elements of {itemsize} bytes, not DeviceOffsets")
        return x.ptr, x.count
    if isinstance(x, DeviceMatches):
        if x.dtype.itemsize % itemsize:
            raise DaachorseError(1, f"{what}: elements of {itemsize} bytes")
        return x.ptr, x.count * (x.dtype.itemsize // itemsize)
    if not (hasattr(x, "data_ptr") and x.is_cuda and x.dtype.itemsize == itemsize and x.is_contiguous()):
        raise DaachorseError(1, f"{what}: DeviceMatches, DeviceOffsets or a contiguous CUDA tensor with elements of {itemsize} bytes")
    return x.data_ptr(), x.numel()


class Normalizer:
    """daac_normalizer: a per-code-point rewrite.  `rules`: rows {first, last, kind, off, len} of integers, sorted and disjoint, over
    code points from U+0000 on, kind a Norm; `pool`: the bytes the Replace rules point into (off and len are read for them alone; len at
    most NORM_MAX_LEN, the pool at most 2 MiB).  A code point in no rule is copied, and so is every byte that is not part of a
    well-formed UTF-8 sequence inside its document.  bert_normalizer() makes BERT's."""

    def __init__(self, rules, pool=b""):
        self._h = None
        a = np.asarray(rules)
        if a.size and (a.ndim != 2 or a.shape[1] != 5 or a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise DaachorseError(1, "rules must be rows {first, last, kind, off, len} of integers in 0 .. 0xFFFFFFFF")
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 5)
        a.setflags(write=False)
        self.rules, self.pool = a, _as_bytes(pool)
        pool_arr = np.frombuffer(self.pool or b"\0", dtype=np.uint8)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().daac_normalizer_create(a.ctypes.data if a.size else None, a.shape[0], pool_arr.ctypes.data, len(self.pool), C.byref(h)))
        self._h = h.value

    @property
    def table_bytes(self):
        """the bytes of the two-stage table and the pool, as they are uploaded"""
        return int(_ffi.lib().daac_normalizer_table_bytes(self._h)) if self._h else 0

    def _run(self, b, stream, src):
        """-> [out (uint8), out_offsets] or [out, out_offsets, src (uint32)], in device memory"""
        if not self._h:
            raise DaachorseError(1, "the normalizer has been freed")
        out, oo, sr, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_normalize_batch(self._h, b.hay, b.off, b.n, b.is_device, stream, int(bool(src)), C.byref(out), C.byref(oo),
                                                   C.byref(sr) if src else None, C.byref(n)))
        res = [DeviceMatches(out.value, n.value, np.dtype(np.uint8)), DeviceOffsets(oo.value, b.n + 1)]
        if src:
            res.append(DeviceMatches(sr.value, n.value, np.dtype(np.uint32)))
        return res

    def normalize_batch(self, docs, src=False, stream=None, device=False):
        """-> (out, out_offsets) or, with src=True, (out, out_offsets, src): document i's image is out[out_offsets[i] : out_offsets[i+1]]
        (np.uint8, np.uint64[n + 1] from 0: a batch again) and src[k] (np.uint32) is the offset, from the start of its input document,
        of the character that output byte k came from.  device=True: DeviceMatches / DeviceOffsets / DeviceMatches (to_numpy / free)"""
        return _offsets_result(self._run(_Batch(docs), stream, src), device)

    def normalize(self, haystack, src=False, stream=None, device=False):
        """one haystack -> out, or (out, src) with src=True"""
        h = _Haystack(haystack)
        if not self._h:
            raise DaachorseError(1, "the normalizer has been freed")
        out, sr, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().daac_normalize(self._h, h.ptr, h.len, h.is_device, stream, int(bool(src)), C.byref(out), C.byref(sr) if src else None, C.byref(n)))
        res = [DeviceMatches(out.value, n.value, np.dtype(np.uint8))]
        if src:
            res.append(DeviceMatches(sr.value, n.value, np.dtype(np.uint32)))
        res = _offsets_result(res, device)
        return res if src else res[0]

    @staticmethod
    def spans_to_source(spans, tok_offsets, out_offsets, src, docs, stream=None):
        """daac_spans_to_source: the {start, end} spans of tokens over the normalized batch (device memory: DeviceMatches or a CUDA
        tensor of [T, 2] int64 / uint64; document i's are [tok_offsets[i], tok_offsets[i+1])), relative to the normalized document, are
        rewritten in place into spans relative to the input document.  `out_offsets` and `src` are normalize_batch's (device=True),
        `docs` the batch it was given."""
        b = _Batch(docs)
        p_sp, n_sp = _device_ptr(spans, 8, "spans")
        p_to, n_to = _device_ptr(tok_offsets, 8, "tok_offsets")
        p_oo, n_oo = _device_ptr(out_offsets, 8, "out_offsets")
        p_sr, _ = _device_ptr(src, 4, "src")
        if n_to != b.n + 1 or n_oo != b.n + 1 or n_sp % 2:
            raise DaachorseError(1, f"tok_offsets and out_offsets hold n + 1 = {b.n + 1} entries and spans pairs")
        _ffi.check(_ffi.lib().daac_spans_to_source(p_sp, p_to, p_oo, p_sr, b.hay, b.off, b.n, n_sp // 2, b.is_device, stream))

    def free(self):
        if self._h:
            _ffi.lib().daac_normalizer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_CJK_BLOCKS = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B920, 0x2CEAF), (0xF900, 0xFAFF),
               (0x2F800, 0x2FA1F))
_RUST_WHITESPACE = frozenset((0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20) + _WHITE_SPACE)   # char::is_whitespace: White_Space


def bert_normalizer_rules(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True):
    """The rules and the pool of BERT's normalizer (`tokenizers`' BertNormalizer; BasicTokenizer's clean-up) as Normalizer takes them,
    from the running Python's `unicodedata`: per code point the four steps composed in order —
      clean_text: U+0000, U+FFFD and the categories Cc (but for tab, LF and CR), Cf and Co are removed (unassigned code points are
        not); tab, LF, CR and the White_Space code points become U+0020;
      handle_chinese_chars: a character of the CJK ideograph blocks becomes ' ' c ' ';
      strip_accents (None: as `lowercase`): NFD, then the characters of category Mn are dropped; a Hangul syllable stays decomposed;
      lowercase: each character's lower-case mapping, with no rule that reads context (no final sigma).
    Adjacent code points with the same kind (and, for Replace, the same image) are one rule.  -> (np.uint32[R, 5], bytes)"""
    import unicodedata
    strip = bool(lowercase) if strip_accents is None else bool(strip_accents)
    cjk = [False] * 0x110000
    if handle_chinese_chars:
        for lo, hi in _CJK_BLOCKS:
            cjk[lo:hi + 1] = [True] * (hi + 1 - lo)
    category, nfd = unicodedata.category, unicodedata.normalize
    rows, pool, at = [], bytearray(), {}
    run = None   # [first, last, kind, image]
    for cp in range(0x110000):
        kind = image = None
        if not 0xD800 <= cp <= 0xDFFF:   # (a surrogate has no UTF-8 sequence: no rule)
            c = s = chr(cp)
            cat = category(c)
            if clean_text and (cp == 0 or cp == 0xFFFD or (cat in ("Cc", "Cf", "Co") and c not in "\t\n\r")):
                s = ""
            else:
                if clean_text and cp in _RUST_WHITESPACE:
                    s = " "
                elif cjk[cp]:
                    s = " " + c + " "
                if strip and s != " ":
                    s = "".join(ch for ch in nfd("NFD", s) if category(ch) != "Mn")
                if lowercase:
                    s = "".join(ch.lower() for ch in s)
            if s == c:
                pass
            elif s == "":
                kind = Norm.Delete
            elif s == " " + c + " ":
                kind = Norm.Pad
            elif 0xAC00 <= cp <= 0xD7A3 and s == nfd("NFD", c):
                kind = Norm.Hangul
            else:
                kind, image = Norm.Replace, s.encode()
        if run is not None and (kind, image) == (run[2], run[3]):
            run[1] = cp
            continue
        if run is not None and run[2] is not None:
            rows.append(run)
        run = [cp, cp, kind, image]
    if run is not None and run[2] is not None:
        rows.append(run)
    out = np.zeros((len(rows), 5), dtype=np.uint32)
    for i, (first, last, kind, image) in enumerate(rows):
        off = 0
        if image is not None:
            off = at.get(image)
            if off is None:
                off = at[image] = len(pool)
                pool += image
        out[i] = (first, last, int(kind), off, len(image) if image is not None else 0)
    return out, bytes(pool)


_bert_normalizers = {}


def bert_normalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True):
    """The Normalizer of bert_normalizer_rules(...), built once per set of options and cached.  It is `tokenizers`' BertNormalizer but
    for three things: no canonical reordering (of the characters that survive strip_accents only 23 have a combining class, such as
    U+302E and U+1D165: two of them side by side keep their order), bytes that are no well-formed UTF-8 are copied, and the tables are
    those of the running Python (`unicodedata.unidata_version`)."""
    key = (bool(clean_text), bool(handle_chinese_chars), bool(lowercase) if strip_accents is None else bool(strip_accents), bool(lowercase))
    nz = _bert_normalizers.get(key)
    if nz is None:
        nz = _bert_normalizers[key] = Normalizer(*bert_normalizer_rules(*key))
    return nz


def scan_count_multi(pma, mode, shards, engine=Engine.Auto, checksum=True):
    """daac_scan_count_multi: one haystack sharded across the GPUs of a node.  `shards` = [(device, buffer, halo, base)]: `buffer` holds
    `halo` bytes of the haystack in front of the shard and then the shard (a CUDA uint8 tensor on that device, or host bytes for all
    shards), `base` = haystack position of the shard's first byte.  -> (count, checksum) or count; equal to scan_count / count of the
    whole haystack."""
    hs = [_Haystack(b) for _, b, _, _ in shards]
    if len({h.is_device for h in hs}) > 1:
        raise DaachorseError(1, "shards must all be device tensors or all host buffers")
    arr = (_ffi.Shard * len(shards))()
    for i, ((dev, _, halo, base), h) in enumerate(zip(shards, hs)):
        if halo > h.len:
            raise DaachorseError(1, "halo longer than the shard's buffer")
        arr[i] = _ffi.Shard(int(dev), h.ptr, int(halo), h.len - int(halo), int(base))
    cnt, cs = C.c_uint64(), C.c_uint64()
    _ffi.check(_ffi.lib().daac_scan_count_multi(pma._h, int(mode), int(engine), arr, len(shards), hs[0].is_device if hs else 0,
                                                C.byref(cnt), C.byref(cs) if checksum else None))
    return (cnt.value, cs.value) if checksum else cnt.value


class DoubleArrayAhoCorasickBuilder:
    """reference src/bytewise/builder.rs:21-244"""

    def __init__(self):
        self._kind = MatchKind.Standard
        self._num_free_blocks = 16

    def match_kind(self, kind):
        self._kind = MatchKind(kind)
        return self

    def num_free_blocks(self, n):
        assert n >= 1  # builder.rs:113
        self._num_free_blocks = int(n)
        return self

    def build(self, patterns):
        return self._build(list(patterns), None)

    def build_with_values(self, patvals):
        patvals = list(patvals)
        return self._build([p for p, _ in patvals], [v for _, v in patvals])

    def _build(self, patterns, values):
        pats = [_as_bytes(p) for p in patterns]
        offs = np.zeros(len(pats) + 1, dtype=np.uint64)
        if pats:
            offs[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
        blob = np.frombuffer(b"".join(pats) or b"\0", dtype=np.uint8)
        vals = None
        if values is not None:
            if any(not (0 <= int(v) <= 0xFFFFFFFF) for v in values):
                raise DaachorseError(3, "value does not fit u32")
            vals = np.ascontiguousarray(values, dtype=np.uint32)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().daac_bytewise_build(blob.ctypes.data, offs.ctypes.data,
                                                  vals.ctypes.data if vals is not None and vals.size else None,
                                                  len(pats), int(self._kind), self._num_free_blocks, C.byref(h)))
        return DoubleArrayAhoCorasick(h)
