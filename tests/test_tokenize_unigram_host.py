"""tokenize_unigram (daac_tokenize_unigram / daac_tokenize_unigram_batch) on the host side: the exports, every answer the C ABI and the
Python wrappers give before they touch a device, and the kernel file's per-lane bodies run on the CPU under ASan and UBSan
(tests/native/unigram_check.cpp, a stand-alone program).  No GPU."""
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

    def __init__(self, p, batch=False, hay=b"abab", offsets=(0, 2, 4), scores=(-1.0, -2.0), unk=-5.0, gap=Gap.Chars, gap_id=7):
        self.p, self.batch, self.gap, self.gap_id, self.unk = p, batch, int(gap), gap_id, unk
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.scores = None if scores is None else np.asarray(scores, dtype=np.float32)
        self.n_scores = 0 if scores is None else len(self.scores)
        self.ids, self.spans, self.tok_off, self.doc_scores = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.n_tokens, self.n_matches, self.score = C.c_uint64(), C.c_uint64(), C.c_float()
        self.null = set()

    def run(self, engine=0):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        L = _ffi.lib()
        if self.batch:
            return L.daac_tokenize_unigram_batch(self.p._h, int(engine), ptr(self.hay), ptr(self.offsets), self.n, 0, None, ptr(self.scores), self.n_scores,
                                                 C.c_float(self.unk), self.gap, self.gap_id, ref("ids", self.ids), ref("spans", self.spans),
                                                 ref("tok_off", self.tok_off), ref("doc_scores", self.doc_scores), ref("n_tokens", self.n_tokens),
                                                 ref("n_matches", self.n_matches))
        return L.daac_tokenize_unigram(self.p._h, int(engine), ptr(self.hay), len(self.hay), 0, None, ptr(self.scores), self.n_scores, C.c_float(self.unk),
                                       self.gap, self.gap_id, ref("ids", self.ids), ref("spans", self.spans), ref("n_tokens", self.n_tokens),
                                       ref("n_matches", self.n_matches), ref("score", self.score))


def _wrapper(p, batch, **kw):
    """the Python wrapper with the same defaults as _Call -> the status it raises"""
    a = dict(scores=[-1.0, -2.0], unk_score=-5.0)
    a.update(kw)
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_unigram_batch([b"ab", b"ab"], **a) if batch else p.tokenize_unigram(b"abab", **a)
    return ei.value.code


def test_unigram_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_tokenize_unigram", "daac_tokenize_unigram_batch"):
        assert hasattr(lib, name), name
    p = _pair(["ab"])
    for name in ("tokenize_unigram", "tokenize_unigram_batch"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.DoubleArrayAhoCorasick, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name


@pytest.mark.parametrize("batch", [False, True])
def test_unigram_bad_arguments_answer_1_without_a_device(batch):
    p = _pair(["ab", "b"])   # values 0 and 1
    err = lambda: _ffi.lib().daac_last_error().decode()
    # a NULL required pointer (spans, the scores of the documents and the single score may be NULL: they are not looked at here)
    for name in ("ids", "n_tokens", "n_matches") + (("tok_off",) if batch else ()):
        c = _Call(p, batch)
        c.null.add(name)
        assert c.run() == 1, name
    # gap: DAAC_GAP_BYTES or DAAC_GAP_CHARS only
    for gap in (-1, int(Gap.Skip), int(Gap.Unk), 4, 255):
        assert _Call(p, batch, gap=gap).run() == 1, gap
        assert "gap" in err()
        assert _wrapper(p, batch, gap=gap) == 1, gap
    # byte fallback: gap_id + 255 has to fit 32 bits; Gap.Chars takes any gap_id (it gets past this check: see the next one fail instead)
    for gid in (0xFFFFFFFF - 254, 0xFFFFFFFF):
        assert _Call(p, batch, gap=Gap.Bytes, gap_id=gid).run() == 1
        assert "gap_id" in err()
        assert _wrapper(p, batch, gap=Gap.Bytes, gap_id=gid) == 1
    assert _Call(p, batch, gap=Gap.Chars, gap_id=0xFFFFFFFF, scores=(0.0,)).run() == 1 and "n_scores" in err()
    # n_scores must be above the largest value among the outputs
    for scores in (None, (), (-1.0,)):
        assert _Call(p, batch, scores=scores).run() == 1, scores
        assert "n_scores" in err()
    assert _wrapper(p, batch, scores=[-1.0]) == 1 and _wrapper(p, batch, scores=[]) == 1
    big = _pair(["ab", "b"], values=[3, 1000])
    assert _Call(big, batch, scores=[0.0] * 1000).run() == 1 and "1000" in err()
    assert _wrapper(big, batch, scores=[0.0] * 1000) == 1
    c = _Call(p, batch)
    c.scores = None   # NULL scores with n_scores > 0
    assert c.run() == 1
    # scores and unk_score: finite, at most 1e20 in magnitude
    for bad in (float("nan"), float("inf"), float("-inf"), 1.0001e20, -1.0001e20, 3e38):
        assert _Call(p, batch, scores=(0.0, bad)).run() == 1, bad
        assert "scores[1]" in err()
        assert _Call(p, batch, unk=bad).run() == 1, bad
        assert "unk_score" in err()
        assert _wrapper(p, batch, scores=[bad, 0.0]) == 1, bad
        assert _wrapper(p, batch, unk_score=bad) == 1, bad
    if batch:   # the batch calls' own offset rules
        assert _Call(p, True, offsets=(0, 3, 2)).run() == 1
        assert "document 1" in err()
        c = _Call(p, True)
        c.offsets = None   # NULL offsets with n > 0
        assert c.run() == 1
        c = _Call(p, True)
        c.hay = None
        assert c.run() == 1 and "hay" in err()
    else:
        c = _Call(p, False)
        c.hay, n = None, 4
        assert _ffi.lib().daac_tokenize_unigram(p._h, 0, None, n, 0, None, c.scores.ctypes.data, 2, C.c_float(-5.0), int(Gap.Chars), 7, C.byref(c.ids), None,
                                                C.byref(c.n_tokens), C.byref(c.n_matches), None) == 1


def test_unigram_accepts_scores_at_the_bound():
    """1e20 itself is a legal score: a leftmost automaton gets past the score checks to the kind check's 5"""
    p = _pair(["ab", "b"], kind=1)
    assert _Call(p, scores=(1e20, -1e20), unk=-1e20).run() == 5


@pytest.mark.parametrize("batch", [False, True])
def test_unigram_leftmost_automata_answer_5_without_a_device(batch):
    lefts = [_pair(["ab", "b"], kind=1), _pair(["ab", "b"], kind=2), _pair(["世界", "界"], kind=1, charwise=True), _pair(["世界", "界"], kind=2, charwise=True)]
    for p in lefts:
        for gap in (Gap.Bytes, Gap.Chars):
            assert _Call(p, batch, gap=gap).run() == 5
            assert "standard" in _ffi.lib().daac_last_error().decode()
            assert _wrapper(p, batch, gap=gap) == 5
            assert _wrapper(p, batch, gap=gap, spans=True) == 5


@pytest.mark.parametrize("batch", [False, True])
def test_unigram_argument_errors_come_before_the_kind_error(batch):
    """every status-1 family is answered before 5 is looked at, as the header lists them"""
    for p in (_pair(["ab", "b"], kind=1), _pair(["世界", "界"], kind=2, charwise=True)):
        c = _Call(p, batch)
        c.null.add("n_tokens")
        assert c.run() == 1
        assert _Call(p, batch, gap=Gap.Unk).run() == 1
        assert _Call(p, batch, gap=Gap.Bytes, gap_id=0xFFFFFFFF).run() == 1
        assert _Call(p, batch, scores=(0.0,)).run() == 1
        assert _Call(p, batch, scores=(0.0, float("nan"))).run() == 1
        assert _Call(p, batch, unk=float("inf")).run() == 1
        if batch:
            assert _Call(p, True, offsets=(0, 3, 2)).run() == 1
        assert _wrapper(p, batch, gap=Gap.Skip) == 1 and _wrapper(p, batch, unk_score=float("nan")) == 1
        assert _Call(p, batch).run() == 5


def test_unigram_leaves_the_abi_version_at_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_unigram_lane_bodies_on_the_host_under_sanitizers(tmp_path):
    """the forward, count and write bodies of unigram_kernels.hip as plain C++, 4 000 random lattices against the definition"""
    exe = str(tmp_path / "unigram_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "unigram_check.cpp")])
    for seed in (1, 2):
        r = subprocess.run([exe, "2000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 2000 lattices") and r.stderr == "", (r.stdout, r.stderr)
