"""tokenize (daac_tokenize / daac_tokenize_batch) on the host side: the exports, and every answer the C ABI and the Python wrappers give
before they touch a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import Gap, ScanMode, _ffi


def _pair(patterns, kind=0, charwise=False):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return p


class _Call:
    """the raw arguments of the two calls; the out-pointers named in `null` go as NULL"""

    def __init__(self, p, mode, batch=False, hay=b"abab", offsets=(0, 2, 4), gap=Gap.Unk, gap_id=7):
        self.p, self.mode, self.batch, self.gap, self.gap_id = p, int(mode), batch, int(gap), gap_id
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.ids, self.spans, self.tok_off, self.n_tokens, self.n_matches = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.null = set()

    def run(self, engine=0):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        L = _ffi.lib()
        if self.batch:
            return L.daac_tokenize_batch(self.p._h, self.mode, int(engine), ptr(self.hay), ptr(self.offsets), self.n, 0, None, self.gap, self.gap_id,
                                         ref("ids", self.ids), ref("spans", self.spans), ref("tok_off", self.tok_off), ref("n_tokens", self.n_tokens),
                                         ref("n_matches", self.n_matches))
        return L.daac_tokenize(self.p._h, self.mode, int(engine), ptr(self.hay), len(self.hay), 0, None, self.gap, self.gap_id, ref("ids", self.ids),
                               ref("spans", self.spans), ref("n_tokens", self.n_tokens), ref("n_matches", self.n_matches))


def test_tokenize_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_tokenize", "daac_tokenize_batch"):
        assert hasattr(lib, name), name
    p = _pair(["ab"])
    for name in ("tokenize", "tokenize_batch"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name
    assert [(g.name, int(g)) for g in da.Gap] == [("Skip", 0), ("Unk", 1), ("Bytes", 2), ("Chars", 3)]
    assert "Gap" in da.__all__


@pytest.mark.parametrize("batch", [False, True])
def test_tokenize_bad_arguments_answer_1_without_a_device(batch):
    p = _pair(["ab", "b"])
    for name in ("ids", "n_tokens", "n_matches") + (("tok_off",) if batch else ()):
        c = _Call(p, ScanMode.Find, batch)
        c.null.add(name)
        assert c.run() == 1, name
    for gap in (-1, 4, 255):
        assert _Call(p, ScanMode.Find, batch, gap=gap).run() == 1, gap
        assert "gap" in _ffi.lib().daac_last_error().decode()
    # byte fallback: gap_id + 255 has to fit 32 bits; the other rules take any gap_id
    assert _Call(p, ScanMode.Find, batch, gap=Gap.Bytes, gap_id=0xFFFFFFFF - 254).run() == 1
    assert _Call(p, ScanMode.Find, batch, gap=Gap.Bytes, gap_id=0xFFFFFFFF).run() == 1
    assert _Call(p, 7, batch).run() == 1                                               # no such mode
    if batch:   # the batch calls' own argument rules
        assert _Call(p, ScanMode.Find, True, offsets=(0, 3, 2)).run() == 1
        assert "document 1" in _ffi.lib().daac_last_error().decode()
        c = _Call(p, ScanMode.Find, True)
        c.offsets = None   # NULL offsets with n > 0
        assert c.run() == 1
        c = _Call(p, ScanMode.Find, True)
        c.hay = None
        assert c.run() == 1
    # the wrappers raise the same
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_batch([b"ab"], gap=4) if batch else p.tokenize(b"abab", gap=4)
    assert ei.value.code == 1
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_batch([b"ab"], gap=Gap.Bytes, gap_id=0xFFFFFF01) if batch else p.tokenize(b"abab", gap=Gap.Bytes, gap_id=0xFFFFFF01)
    assert ei.value.code == 1


@pytest.mark.parametrize("batch", [False, True])
def test_tokenize_overlapping_modes_answer_6_without_a_device(batch):
    std, left, cstd = _pair(["ab", "b"]), _pair(["ab", "b"], kind=1), _pair(["世界", "界"], charwise=True)
    for p in (std, left, cstd):
        for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
            assert _Call(p, mode, batch).run() == 6, mode
            assert "no gaps" in _ffi.lib().daac_last_error().decode()
            with pytest.raises(da.DaachorseError) as ei:
                p.tokenize_batch([b"ab"], mode=mode) if batch else p.tokenize(b"abab", mode=mode)
            assert ei.value.code == 6


@pytest.mark.parametrize("batch", [False, True])
def test_tokenize_match_kind_mismatch_answers_5_without_a_device(batch):
    std, cstd = _pair(["ab", "b"]), _pair(["世界", "界"], charwise=True)
    lefts = [_pair(["ab", "b"], kind=1), _pair(["ab", "b"], kind=2), _pair(["世界", "界"], kind=2, charwise=True)]
    for p, mode in [(std, ScanMode.LeftmostFind), (cstd, ScanMode.LeftmostFind)] + [(q, ScanMode.Find) for q in lefts]:
        assert _Call(p, mode, batch).run() == 5, mode
        with pytest.raises(da.DaachorseError) as ei:
            p.tokenize_batch([b"ab"], spans=True, mode=mode) if batch else p.tokenize(b"abab", spans=True, mode=mode)
        assert ei.value.code == 5


def test_tokenize_argument_errors_come_before_mode_errors():
    """1 (a bad gap) is answered before 6 and 5 are looked at, as the header lists them"""
    p = _pair(["ab", "b"])
    assert _Call(p, ScanMode.FindOverlapping, gap=9).run() == 1
    assert _Call(p, ScanMode.LeftmostFind, gap=9).run() == 1


def test_tokenize_leaves_the_abi_version_at_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION
