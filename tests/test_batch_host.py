"""Batches (daac_scan_count_batch / daac_scan_batch_device16) on the host side: the exports, and every answer the C ABI gives
before it touches a device — MatchKind mismatch, decreasing host offsets, NULL offsets, the two options.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import ScanMode, _ffi


def _pma(patterns, kind=0):
    p, rest = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(patterns, kind=kind).serialize())
    assert rest == b""
    return p


def _count_batch(p, mode, hay, offsets, n, counts=None):
    h = np.frombuffer(hay or b"\0", dtype=np.uint8)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    counts = np.zeros(max(n, 1), dtype=np.uint64) if counts is None else counts
    return _ffi.lib().daac_scan_count_batch(p._h, int(mode), 0, h.ctypes.data, None if off is None else off.ctypes.data, n, 0, None,
                                            counts.ctypes.data, None, 0)


def _device16_batch(p, mode, hay, offsets, n):
    h = np.frombuffer(hay or b"\0", dtype=np.uint8)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    out, doffs, tot = C.c_void_p(), C.c_void_p(), C.c_uint64()
    return _ffi.lib().daac_scan_batch_device16(p._h, int(mode), 0, h.ctypes.data, None if off is None else off.ctypes.data, n, 0, None,
                                               C.byref(out), C.byref(doffs), C.byref(tot))


def test_batch_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_scan_count_batch", "daac_scan_batch_device16"):
        assert hasattr(lib, name), name
    p = _pma(["ab"])
    for name in ("count_batch", "scan_count_batch", "scan_batch", "scan_batch_device"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name


def test_batch_match_kind_mismatch_answers_5_without_a_device():
    std, left = _pma(["ab", "b"]), _pma(["ab", "b"], kind=1)
    docs = [b"xab", b"", b"bb"]
    for p, mode in ((std, ScanMode.LeftmostFind), (left, ScanMode.Find), (left, ScanMode.FindOverlapping), (left, ScanMode.FindOverlappingNoSuffix)):
        for fn in (p.count_batch, p.scan_count_batch, p.scan_batch_device, p.scan_batch):
            with pytest.raises(da.DaachorseError) as ei:
                fn(mode, docs)
            assert ei.value.code == 5, (fn.__name__, mode)
    c = da.CharwiseDoubleArrayAhoCorasickBuilder().match_kind(da.MatchKind.LeftmostFirst).build(["全世界", "世界"])
    with pytest.raises(da.DaachorseError) as ei:
        c.count_batch(ScanMode.FindOverlapping, ["全世界"])
    assert ei.value.code == 5


def test_batch_bad_offsets_answer_1_before_any_device_work():
    p = _pma(["ab", "b"])
    hay = b"abab"
    for mode in (ScanMode.FindOverlapping, ScanMode.Find, ScanMode.FindOverlappingNoSuffix):
        assert _count_batch(p, mode, hay, [0, 3, 2, 4], 3) == 1, mode
        assert "decrease" in _ffi.lib().daac_last_error().decode()
        assert _device16_batch(p, mode, hay, [0, 3, 2, 4], 3) == 1, mode
        assert _count_batch(p, mode, hay, None, 2) == 1, mode
        assert _device16_batch(p, mode, hay, None, 2) == 1, mode
    # the check comes before the MatchKind's: NULL offsets are always 1
    assert _count_batch(_pma(["ab"], kind=1), ScanMode.LeftmostFind, hay, None, 1) == 1


def test_batch_engines_that_do_not_serve_batches_answer_6_without_a_device():
    p = _pma(["ab", "b"])
    h = np.frombuffer(b"ab", dtype=np.uint8)
    off = np.array([0, 2], dtype=np.uint64)
    counts = np.zeros(1, dtype=np.uint64)
    for eng in (da.Engine.Gram, da.Engine.Pfx):
        assert _ffi.lib().daac_scan_count_batch(p._h, 0, int(eng), h.ctypes.data, off.ctypes.data, 1, 0, None, counts.ctypes.data, None, 0) == 6


def test_batch_options_are_accepted():
    for name, value in (("batch_piece", 4096), ("batch_lane_max", 16384)):
        _ffi.check(_ffi.lib().daac_set_option(name.encode(), value))
    p = _pma(["ab"])
    p.set_option("batch_piece", 1024).set_option("batch_lane_max", 4096)
    p.set_option("batch_piece").set_option("batch_lane_max")
