"""replace_all (daac_replace_all / daac_replace_all_batch) on the host side: the exports, and every answer the C ABI and the Python
wrappers give before they touch a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, _ffi


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
    """the raw arguments of the two calls, each replaceable by None (NULL)"""

    def __init__(self, p, mode, batch=False, hay=b"abab", offsets=(0, 2, 4), repl=b"xyz", repl_offsets=(0, 1, 3), n_repl=2):
        self.p, self.mode, self.batch, self.n_repl = p, int(mode), batch, n_repl
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.repl = None if repl is None else np.frombuffer(repl or b"\0", dtype=np.uint8)
        self.repl_offsets = None if repl_offsets is None else np.asarray(repl_offsets, dtype=np.uint64)
        self.out, self.out_off, self.out_len, self.n_replaced = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.null = set()

    def run(self, engine=0):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        L = _ffi.lib()
        if self.batch:
            return L.daac_replace_all_batch(self.p._h, self.mode, int(engine), ptr(self.hay), ptr(self.offsets), self.n, 0, None, ptr(self.repl),
                                            ptr(self.repl_offsets), self.n_repl, ref("out", self.out), ref("out_off", self.out_off),
                                            ref("out_len", self.out_len), ref("n_replaced", self.n_replaced))
        return L.daac_replace_all(self.p._h, self.mode, int(engine), ptr(self.hay), len(self.hay), 0, None, ptr(self.repl), ptr(self.repl_offsets),
                                  self.n_repl, ref("out", self.out), ref("out_len", self.out_len), ref("n_replaced", self.n_replaced))


def test_replace_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_replace_all", "daac_replace_all_batch"):
        assert hasattr(lib, name), name
    p = _pair(["ab"])
    for name in ("replace_all", "replace_all_batch"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name


@pytest.mark.parametrize("batch", [False, True])
def test_replace_bad_arguments_answer_1_without_a_device(batch):
    p = _pair(["ab", "b"])
    outs = ("out", "out_len", "n_replaced") + (("out_off",) if batch else ())
    for name in outs:
        c = _Call(p, ScanMode.Find, batch)
        c.null.add(name)
        assert c.run() == 1, name
    assert _Call(p, ScanMode.Find, batch, n_repl=0).run() == 1
    assert _Call(p, ScanMode.Find, batch, repl_offsets=None).run() == 1
    assert _Call(p, ScanMode.Find, batch, repl_offsets=(0, 3, 1)).run() == 1
    assert "decrease" in _ffi.lib().daac_last_error().decode()
    assert _Call(p, ScanMode.Find, batch, repl=None).run() == 1                       # NULL blob, 3 bytes of replacements
    assert _Call(p, ScanMode.Find, batch, n_repl=1, repl_offsets=(0, 1 << 32)).run() == 1   # offsets end at 4 GiB
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


@pytest.mark.parametrize("batch", [False, True])
def test_replace_overlapping_modes_answer_6_without_a_device(batch):
    std, left, cstd = _pair(["ab", "b"]), _pair(["ab", "b"], kind=1), _pair(["世界", "界"], charwise=True)
    for p in (std, left, cstd):
        for mode in (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix):
            assert _Call(p, mode, batch).run() == 6, mode
            assert "no splice" in _ffi.lib().daac_last_error().decode()
            with pytest.raises(da.DaachorseError) as ei:
                p.replace_all_batch([b"ab"], b"x", mode=mode) if batch else p.replace_all(b"abab", b"x", mode=mode)
            assert ei.value.code == 6


@pytest.mark.parametrize("batch", [False, True])
def test_replace_match_kind_mismatch_answers_5_without_a_device(batch):
    std, cstd = _pair(["ab", "b"]), _pair(["世界", "界"], charwise=True)
    lefts = [_pair(["ab", "b"], kind=1), _pair(["ab", "b"], kind=2), _pair(["世界", "界"], kind=2, charwise=True)]
    for p, mode in [(std, ScanMode.LeftmostFind), (cstd, ScanMode.LeftmostFind)] + [(q, ScanMode.Find) for q in lefts]:
        assert _Call(p, mode, batch).run() == 5, mode
        with pytest.raises(da.DaachorseError) as ei:
            p.replace_all_batch([b"ab"], [b"x", b"y"], mode=mode) if batch else p.replace_all(b"abab", [b"x", b"y"], mode=mode)
        assert ei.value.code == 5


def test_mode_none_picks_the_iterator_of_the_kind():
    """mode=None: Find for Standard handles, LeftmostFind otherwise; a mode that is given is passed on as it is"""
    cases = [(_pair(["ab", "b"]), 0), (_pair(["ab", "b"], kind=1), 1), (_pair(["ab", "b"], kind=2), 2), (_pair(["世界"], charwise=True), 0),
             (_pair(["世界"], kind=1, charwise=True), 1)]
    for p, kind in cases:
        assert int(p.match_kind()) == kind
        assert p._replace_mode(None) == int(ScanMode.Find if kind == 0 else ScanMode.LeftmostFind)
        for mode in ScanMode:
            assert p._replace_mode(mode) == int(mode)
        # the wrappers hand an empty replacement table on: 1, before the mode is looked at
        for call in (lambda: p.replace_all(b"abab", []), lambda: p.replace_all_batch([b"ab", b""], [])):
            with pytest.raises(da.DaachorseError) as ei:
                call()
            assert ei.value.code == 1


def test_replacements_argument_forms():
    from daachorse_amd.bytewise import _Replacements
    r = _Replacements("é")
    assert r.n == 1 and r.offsets.tolist() == [0, 2] and r.blob.tobytes() == "é".encode()
    r = _Replacements(b"[x]")
    assert r.n == 1 and r.offsets.tolist() == [0, 3]
    r = _Replacements([b"<A>", "", "界"])
    assert r.n == 3 and r.offsets.tolist() == [0, 3, 3, 6] and r.blob.tobytes() == b"<A>" + "界".encode()
    r = _Replacements([b""])
    assert r.n == 1 and r.offsets.tolist() == [0, 0]


def test_replace_leaves_the_abi_version_at_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION
