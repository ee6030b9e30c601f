"""Histograms (daac_pma_outputs / daac_scan_histogram) on the host side: the exports, the output records against the CPU oracle's, and
every answer the C ABI gives before it touches a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, _ffi, synth


def _pair(patterns, values=None, kind=0, charwise=False):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return o, p


def _hist(p, mode, engine=0, hay=b"ab", begin=0, counts="own", length=None):
    h = np.frombuffer(hay or b"\0", dtype=np.uint8)
    if isinstance(counts, str):
        counts = np.zeros(max(1, len(p.outputs())), dtype=np.uint64)
    return _ffi.lib().daac_scan_histogram(p._h, int(mode), int(engine), h.ctypes.data, len(hay) if length is None else length, begin, 0, None,
                                          None if counts is None else counts.ctypes.data, 0)


def test_hist_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_pma_outputs", "daac_scan_histogram"):
        assert hasattr(lib, name), name
    _, p = _pair(["ab"])
    for name in ("outputs", "histogram", "pattern_counts"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name


def _outputs_cases():
    pats, vals, _ = synth.patterns_copies(9, 3)
    return {
        "standard": dict(patterns=synth.patterns_cfg2(300)),
        "leftmost_longest": dict(patterns=synth.patterns_cfg2(300), kind=1),
        "with_empty": dict(patterns=[b"", b"a", b"ab", b"bab", b"b"]),
        "copies": dict(patterns=pats, values=vals),
        "charwise": dict(patterns=["全世界", "世界", "界", "a", "é世"], charwise=True),
    }


@pytest.mark.parametrize("case", ["standard", "leftmost_longest", "with_empty", "copies", "charwise"])
def test_outputs_equal_the_oracles_row_for_row(case):
    o, p = _pair(**_outputs_cases()[case])
    want = o.outputs()
    got = p.outputs()
    assert len(want) > 0 and len(got) == len(want) == p.info().outputs_len
    assert got.dtype.names == ("value", "length", "parent")
    assert np.array_equal(np.stack([got["value"], got["length"], got["parent"]], axis=1), want)
    # the chain the histogram's propagation walks ends: a parent lies before its record
    assert np.all(got["parent"] <= np.arange(len(got)))


def test_outputs_cap_limits_what_is_written():
    o, p = _pair(synth.patterns_cfg2(50))
    want = o.outputs()
    n = len(want)
    buf = np.full((n, 3), 0xDEADBEEF, dtype=np.uint32)
    assert _ffi.lib().daac_pma_outputs(p._h, buf.ctypes.data, 7) == n
    assert np.array_equal(buf[:7], want[:7]) and np.all(buf[7:] == 0xDEADBEEF)
    assert _ffi.lib().daac_pma_outputs(p._h, None, 0) == n
    assert _ffi.lib().daac_pma_outputs(p._h, buf.ctypes.data, n + 100) == n
    assert np.array_equal(buf, want)


def test_hist_match_kind_mismatch_answers_5_without_a_device():
    for kind in (1, 2):
        _, left = _pair(["ab", "b"], kind=kind)
        for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
            assert _hist(left, mode) == 5, (kind, mode)
            with pytest.raises(da.DaachorseError) as ei:
                left.histogram(mode, b"abab")
            assert ei.value.code == 5
            with pytest.raises(da.DaachorseError) as ei:
                left.pattern_counts(mode, b"abab")
            assert ei.value.code == 5
    _, c = _pair(["全世界", "世界"], kind=2, charwise=True)
    with pytest.raises(da.DaachorseError) as ei:
        c.histogram(ScanMode.FindOverlapping, "全世界")
    assert ei.value.code == 5


def test_hist_chain_modes_answer_6_without_a_device():
    _, std = _pair(["ab", "b"])
    _, left = _pair(["ab", "b"], kind=1)
    _, cstd = _pair(["世界", "界"], charwise=True)
    for p, mode in ((std, ScanMode.Find), (left, ScanMode.LeftmostFind), (cstd, ScanMode.Find)):
        assert _hist(p, mode) == 6, mode
        assert "DAAC_FIND_OVERLAPPING" in _ffi.lib().daac_last_error().decode()
        with pytest.raises(da.DaachorseError) as ei:
            p.histogram(mode, b"abab")
        assert ei.value.code == 6


def test_hist_engines_that_do_not_serve_it_answer_6_without_a_device():
    _, p = _pair(["ab", "b"])
    for eng in (Engine.Gram, Engine.Pfx):
        for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
            assert _hist(p, mode, engine=eng) == 6, (eng, mode)
    _, c = _pair(["世界", "界"], charwise=True)
    for eng in (Engine.Tiered, Engine.Gram, Engine.Pfx):
        assert _hist(c, ScanMode.FindOverlapping, engine=eng) == 6, eng


def test_hist_bad_arguments_answer_1_without_a_device():
    _, p = _pair(["ab", "b"])
    for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
        assert _hist(p, mode, counts=None) == 1, mode
        assert _hist(p, mode, hay=b"abab", begin=5) == 1, mode
    with pytest.raises(da.DaachorseError) as ei:
        p.histogram(ScanMode.FindOverlapping, b"abab", begin=5)
    assert ei.value.code == 1
    # an automaton without patterns has no counter to write: NULL counts is fine there, and nothing touches a device
    _, e = _pair([])
    assert len(e.outputs()) == 0
    assert _hist(e, ScanMode.FindOverlapping, counts=None) == 0
    assert len(e.histogram(ScanMode.FindOverlapping, b"abab")) == 0
    assert len(e.pattern_counts(ScanMode.FindOverlappingNoSuffix, b"")) == 0


def test_hist_option_is_accepted_and_rejects_negative_values():
    _, p = _pair(["ab"])
    p.set_option("hist_lds_bins", 0).set_option("hist_lds_bins", 2048).set_option("hist_lds_bins", 1 << 20)
    with pytest.raises(da.DaachorseError) as ei:
        p.set_option("hist_lds_bins", -1)
    assert ei.value.code == 1
    p.set_option("hist_lds_bins")
    # process-wide, a negative value is turned away the same way (and so leaves the process's value as it was)
    assert _ffi.lib().daac_set_option(b"hist_lds_bins", -1) == 1
    assert "hist_lds_bins" in _ffi.lib().daac_last_error().decode()


def test_abi_version_is_still_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION
