"""Per-document pattern counts of a batch (daac_scan_histogram_batch) on the host side: the exports, and every answer the C ABI gives
before it touches a device — MatchKind mismatch, engines that do not serve batches, NULL arguments, decreasing host offsets, chain-mode
documents beyond batch_lane_max, the two options.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, _ffi


def _pma(patterns, kind=0):
    p, rest = da.DoubleArrayAhoCorasick.deserialize(orc.OraclePma.build(patterns, kind=kind).serialize())
    assert rest == b""
    return p


def _call(p, mode, hay, offsets, n, engine=0, outs=(True, True, True)):
    """the raw status; `outs` says which of the three out-pointers are given"""
    h = np.frombuffer(hay or b"\0", dtype=np.uint8)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, doffs, tot = C.c_void_p(), C.c_void_p(), C.c_uint64()
    st = _ffi.lib().daac_scan_histogram_batch(p._h, int(mode), int(engine), h.ctypes.data, None if off is None else off.ctypes.data, n, 0, None,
                                              C.byref(rows) if outs[0] else None, C.byref(doffs) if outs[1] else None, C.byref(tot) if outs[2] else None)
    assert st != 0 and rows.value is None and doffs.value is None
    return st


def _msg():
    return _ffi.lib().daac_last_error().decode()


def test_symbol_and_methods_are_exported():
    assert hasattr(C.CDLL(_ffi._build.LIB_PATH), "daac_scan_histogram_batch")
    p = _pma(["ab"])
    for name in ("histogram_batch", "histogram_batch_device"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name
    assert da.SLOT_COUNT_DTYPE.names == ("slot", "count") and da.SLOT_COUNT_DTYPE.itemsize == 8


def test_abi_version_stays_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_match_kind_mismatch_answers_5():
    std, left = _pma(["ab", "b"]), _pma(["ab", "b"], kind=1)
    docs = [b"xab", b"", b"bb"]
    for p, mode in ((std, ScanMode.LeftmostFind), (left, ScanMode.Find), (left, ScanMode.FindOverlapping), (left, ScanMode.FindOverlappingNoSuffix)):
        for fn in (p.histogram_batch, p.histogram_batch_device):
            with pytest.raises(da.DaachorseError) as ei:
                fn(mode, docs)
            assert ei.value.code == 5, (fn.__name__, mode)
    c = da.CharwiseDoubleArrayAhoCorasickBuilder().match_kind(da.MatchKind.LeftmostFirst).build(["全世界", "世界"])
    with pytest.raises(da.DaachorseError) as ei:
        c.histogram_batch(ScanMode.FindOverlapping, ["全世界"])
    assert ei.value.code == 5


def test_engines_that_do_not_serve_batches_answer_6():
    p = _pma(["ab", "b"])
    for eng in (Engine.Gram, Engine.Pfx):
        for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix, ScanMode.Find):
            assert _call(p, mode, b"ab", [0, 2], 1, engine=eng) == 6, (eng, mode)
    # find_iter / leftmost_find_iter run on the double array only
    assert _call(p, ScanMode.Find, b"ab", [0, 2], 1, engine=Engine.Tiered) == 6
    assert _call(_pma(["ab", "b"], kind=1), ScanMode.LeftmostFind, b"ab", [0, 2], 1, engine=Engine.Tiered) == 6
    # ... and so do charwise handles
    c = da.CharwiseDoubleArrayAhoCorasick.new(["全世界", "世界"])
    with pytest.raises(da.DaachorseError) as ei:
        c.histogram_batch(ScanMode.FindOverlapping, ["全世界"], engine=Engine.Tiered)
    assert ei.value.code == 6


def test_null_arguments_answer_1():
    p = _pma(["ab", "b"])
    for mode in (ScanMode.FindOverlapping, ScanMode.Find):
        for outs in ((False, True, True), (True, False, True), (True, True, False)):
            assert _call(p, mode, b"abab", [0, 2, 4], 2, outs=outs) == 1, (mode, outs)
        assert _call(p, mode, b"abab", None, 2) == 1, mode
    # the check comes before the MatchKind's: NULL offsets are always 1
    assert _call(_pma(["ab"], kind=1), ScanMode.Find, b"abab", None, 1) == 1


def test_decreasing_host_offsets_answer_1():
    p = _pma(["ab", "b"])
    for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix, ScanMode.Find):
        assert _call(p, mode, b"abab", [0, 3, 2, 4], 3) == 1, mode
        assert "decrease at document 1" in _msg()


def test_chain_document_beyond_lane_max_answers_6_and_names_document_and_option():
    lane_max = 100
    hay = b"ab" * 200
    offsets = [0, 10, 10 + lane_max, 111 + lane_max, 400]   # lengths 10, lane_max, lane_max + 1, the rest
    for kind, mode in ((0, ScanMode.Find), (1, ScanMode.LeftmostFind), (2, ScanMode.LeftmostFind)):
        p = _pma(["ab", "b"], kind=kind)
        p.set_option("batch_lane_max", lane_max)
        assert _call(p, mode, hay, offsets, 4) == 6, mode
        assert "document 2 " in _msg() and "batch_lane_max" in _msg() and str(lane_max + 1) in _msg(), _msg()
        with pytest.raises(da.DaachorseError) as ei:
            p.histogram_batch(mode, [hay[:10], hay[:lane_max], hay[:lane_max + 1]])
        assert ei.value.code == 6 and "document 2 " in str(ei.value)


def test_options_are_accepted_and_negative_values_answer_1():
    p = _pma(["ab"])
    for name, value in (("batch_hist_wave_max", 2048), ("batch_hist_sort_max", 16384)):
        _ffi.check(_ffi.lib().daac_set_option(name.encode(), value))
        assert _ffi.lib().daac_set_option(name.encode(), -1) == 1
        assert name in _msg()
        p.set_option(name, 0).set_option(name, 7).set_option(name)
        with pytest.raises(da.DaachorseError) as ei:
            p.set_option(name, -5)
        assert ei.value.code == 1
