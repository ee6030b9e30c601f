"""tokenize_bpe (daac_tokenize_bpe / daac_tokenize_bpe_batch) on the host side: the exports, every answer the C ABI and the Python
wrappers give before they touch a device, the option bpe_doc_max, and the kernel file's per-lane bodies run on the CPU under ASan and
UBSan (tests/native/bpe_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

import daachorse_amd as da
from daachorse_amd import Gap, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(patterns, kind=0, charwise=False, values=None):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return p


class _Call:
    """the raw arguments of the two calls; the out-pointers named in `null` go as NULL"""

    def __init__(self, p, batch=False, hay=b"abab", offsets=(0, 2, 4), ranks=None, gap=Gap.Chars, gap_id=7):
        self.p, self.batch, self.gap, self.gap_id = p, batch, int(gap), gap_id
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.ranks = None if ranks is None else np.asarray(ranks, dtype=np.uint32)
        self.n_ranks = 0 if ranks is None else len(self.ranks)
        self.ids, self.spans, self.tok_off = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.n_tokens, self.n_matches = C.c_uint64(), C.c_uint64()
        self.null = set()

    def run(self, engine=0):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        L = _ffi.lib()
        if self.batch:
            return L.daac_tokenize_bpe_batch(self.p._h, int(engine), ptr(self.hay), ptr(self.offsets), self.n, 0, None, ptr(self.ranks), self.n_ranks,
                                             self.gap, self.gap_id, ref("ids", self.ids), ref("spans", self.spans), ref("tok_off", self.tok_off),
                                             ref("n_tokens", self.n_tokens), ref("n_matches", self.n_matches))
        return L.daac_tokenize_bpe(self.p._h, int(engine), ptr(self.hay), len(self.hay), 0, None, ptr(self.ranks), self.n_ranks, self.gap, self.gap_id,
                                   ref("ids", self.ids), ref("spans", self.spans), ref("n_tokens", self.n_tokens), ref("n_matches", self.n_matches))


def _err():
    return _ffi.lib().daac_last_error().decode()


def _wrapper(p, batch, **kw):
    """the Python wrapper on the same text as _Call -> (the status it raises, the message)"""
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_bpe_batch([b"ab", b"ab"], **kw) if batch else p.tokenize_bpe(b"abab", **kw)
    return ei.value.code, str(ei.value)


def test_bpe_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_tokenize_bpe", "daac_tokenize_bpe_batch"):
        assert hasattr(lib, name), name
    p = _pair(["ab"])
    for name in ("tokenize_bpe", "tokenize_bpe_batch"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.DoubleArrayAhoCorasick, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name


@pytest.mark.parametrize("batch", [False, True])
def test_bpe_bad_arguments_answer_1_without_a_device(batch):
    p = _pair(["ab", "b"])   # values 0 and 1
    # a NULL required pointer (spans may be NULL: they are not wanted then)
    for name in ("ids", "n_tokens", "n_matches") + (("tok_off",) if batch else ()):
        c = _Call(p, batch)
        c.null.add(name)
        assert c.run() == 1, name
        assert "null" in _err()
    # gap: DAAC_GAP_BYTES or DAAC_GAP_CHARS only
    for gap in (-1, int(Gap.Skip), int(Gap.Unk), 4, 255):
        assert _Call(p, batch, gap=gap).run() == 1, gap
        assert "gap" in _err()
        code, msg = _wrapper(p, batch, gap=gap)
        assert code == 1 and "gap" in msg, gap
    # byte fallback: gap_id + 255 has to fit 32 bits; Gap.Chars takes any gap_id
    for gid in (0xFFFFFFFF - 254, 0xFFFFFFFF):
        assert _Call(p, batch, gap=Gap.Bytes, gap_id=gid).run() == 1
        assert "gap_id" in _err()
        code, msg = _wrapper(p, batch, gap=Gap.Bytes, gap_id=gid)
        assert code == 1 and "gap_id" in msg
    assert _Call(p, batch, gap=Gap.Chars, gap_id=0xFFFFFFFF, ranks=(0,)).run() == 1 and "n_ranks" in _err()   # past the gap_id check
    # ranks == NULL with n_ranks != 0, and the reverse
    c = _Call(p, batch)
    c.n_ranks = 2
    assert c.run() == 1 and "ranks is NULL" in _err()
    c = _Call(p, batch, ranks=(0, 1))
    c.n_ranks = 0
    assert c.run() == 1 and "n_ranks is 0" in _err()
    # a table must reach the largest value among the outputs
    assert _Call(p, batch, ranks=(5,)).run() == 1 and "n_ranks" in _err()
    code, msg = _wrapper(p, batch, ranks=[5])
    assert code == 1 and "n_ranks" in msg
    big = _pair(["ab", "b"], values=[3, 1000])
    assert _Call(big, batch, ranks=[0] * 1000).run() == 1 and "1000" in _err()
    code, msg = _wrapper(big, batch, ranks=[0] * 1000)
    assert code == 1 and "n_ranks" in msg
    # what the wrapper itself refuses as a table
    for bad in ([], [[0, 1]], [0.5, 1.0], [-1, 0], [0, 1 << 32]):
        code, msg = _wrapper(p, batch, ranks=bad)
        assert code == 1 and "ranks" in msg, bad
    if batch:   # the batch calls' own offset rules
        assert _Call(p, True, offsets=(0, 3, 2)).run() == 1
        assert "document 1" in _err()
        c = _Call(p, True)
        c.offsets = None   # NULL offsets with n > 0
        assert c.run() == 1 and "offsets" in _err()
        c = _Call(p, True)
        c.hay = None
        assert c.run() == 1 and "hay" in _err()
    else:
        c = _Call(p, False)
        assert _ffi.lib().daac_tokenize_bpe(p._h, 0, None, 4, 0, None, None, 0, int(Gap.Chars), 7, C.byref(c.ids), None, C.byref(c.n_tokens),
                                            C.byref(c.n_matches)) == 1
        assert "hay" in _err()


@pytest.mark.parametrize("batch", [False, True])
def test_bpe_leftmost_automata_answer_5_without_a_device(batch):
    lefts = [_pair(["ab", "b"], kind=1), _pair(["ab", "b"], kind=2), _pair(["世界", "界"], kind=1, charwise=True), _pair(["世界", "界"], kind=2, charwise=True)]
    for p in lefts:
        for gap in (Gap.Bytes, Gap.Chars):
            assert _Call(p, batch, gap=gap).run() == 5
            assert "standard" in _err()
            assert _Call(p, batch, gap=gap, ranks=(1, 0)).run() == 5
            assert _wrapper(p, batch, gap=gap)[0] == 5
            assert _wrapper(p, batch, gap=gap, spans=True, ranks=[1, 0])[0] == 5


@pytest.mark.parametrize("batch", [False, True])
def test_bpe_argument_errors_come_before_the_kind_error(batch):
    """every status-1 family is answered before 5 is looked at, in the order the header lists them"""
    for p in (_pair(["ab", "b"], kind=1), _pair(["世界", "界"], kind=2, charwise=True)):
        c = _Call(p, batch)
        c.null.add("n_tokens")
        assert c.run() == 1
        assert _Call(p, batch, gap=Gap.Unk).run() == 1
        assert _Call(p, batch, gap=Gap.Bytes, gap_id=0xFFFFFFFF).run() == 1
        c = _Call(p, batch)
        c.n_ranks = 1
        assert c.run() == 1
        c = _Call(p, batch, ranks=(0, 1))
        c.n_ranks = 0
        assert c.run() == 1
        assert _Call(p, batch, ranks=(0,)).run() == 1
        if batch:
            assert _Call(p, True, offsets=(0, 3, 2)).run() == 1
        assert _wrapper(p, batch, gap=Gap.Skip)[0] == 1 and _wrapper(p, batch, ranks=[0])[0] == 1
        # ... and in the header's order among themselves: a NULL out-pointer, the gap, gap_id, the two NULL / 0 rules, n_ranks, the offsets
        c = _Call(p, batch, gap=Gap.Unk, gap_id=0xFFFFFFFF, ranks=(0,), offsets=(0, 3, 2))
        c.null.add("ids")
        assert c.run() == 1 and "null" in _err()
        assert _Call(p, batch, gap=Gap.Unk, gap_id=0xFFFFFFFF, ranks=(0,), offsets=(0, 3, 2)).run() == 1 and "gap is neither" in _err()
        assert _Call(p, batch, gap=Gap.Bytes, gap_id=0xFFFFFFFF, ranks=(0,), offsets=(0, 3, 2)).run() == 1 and "gap_id" in _err()
        c = _Call(p, batch, gap=Gap.Bytes, ranks=(0,), offsets=(0, 3, 2))
        c.n_ranks = 0
        assert c.run() == 1 and "n_ranks is 0" in _err()
        assert _Call(p, batch, ranks=(0,), offsets=(0, 3, 2)).run() == 1 and "does not cover" in _err()
        if batch:
            assert _Call(p, True, ranks=(0, 1), offsets=(0, 3, 2)).run() == 1 and "offsets decrease" in _err()
        assert _Call(p, batch).run() == 5
        assert _Call(p, batch, ranks=(0, 0xFFFFFFFF)).run() == 5


def test_bpe_leaves_the_abi_version_at_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_bpe_doc_max_option_and_the_cap_on_host_offsets():
    """1 .. 65536 per handle and process-wide; a host document above the cap answers 6 before a device is looked for"""
    p = _pair(["ab", "b"])
    for ok in (1, 100, 4096, 65536):
        p.set_option("bpe_doc_max", ok)
    for bad in (0, -1, 65537, 1 << 40):
        with pytest.raises(da.DaachorseError) as ei:
            p.set_option("bpe_doc_max", bad)
        assert ei.value.code == 1 and "bpe_doc_max" in str(ei.value), bad
        with pytest.raises(da.DaachorseError) as ei:
            da.set_option("bpe_doc_max", bad)
        assert ei.value.code == 1, bad
    da.set_option("bpe_doc_max", 4096)   # the default, set again
    p.set_option("bpe_doc_max", 3)
    assert _Call(p, False, hay=b"abab").run() == 6
    assert "document 0" in _err() and "4 bytes" in _err() and "pre-split" in _err()
    assert _Call(p, True, hay=b"ababab", offsets=(0, 2, 6)).run() == 6
    assert "document 1" in _err() and "bpe_doc_max" in _err()
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_bpe_batch([b"a", b"", b"abab"])
    assert ei.value.code == 6 and "document 2" in str(ei.value)
    p.set_option("bpe_doc_max")   # the override gone: 4096 again
    assert _Call(p, False, hay=b"a" * 4097).run() == 6 and "4097" in _err()
    # a leftmost automaton answers 5 whatever the length
    q = _pair(["ab", "b"], kind=1)
    assert _Call(q, False, hay=b"a" * 5000).run() == 5


def test_bpe_lane_bodies_on_the_host_under_sanitizers(tmp_path):
    """the merge and write bodies of bpe_kernels.hip as plain C++, 4 000 random rounds of documents and tuple lists against the definition"""
    exe = str(tmp_path / "bpe_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "bpe_check.cpp")])
    for seed in (1, 2):
        r = subprocess.run([exe, "2000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 2000 rounds") and r.stderr == "", (r.stdout, r.stderr)
