"""The CPU oracle on the dictionaries of daachorse_amd/synth.py's limit families (full-range values, patterns at the packing lengths, many
copies of one pattern, charwise output counts), checked against a brute force written from the semantics the crate documents.

The golden vectors do not pin the oracle on dictionaries like these, and tests/test_gpu_dictionary_limits.py takes the oracle as its
truth, so the oracle is proven here first, on small instances of every family:
  - overlapping: every occurrence of every pattern, as a multiset of (start, end, value); at one end, longer patterns first and the
    copies of one pattern in registration order
  - standard non-overlapping: the earliest end, then the longest pattern ending there
  - leftmost-longest: the leftmost start, then the longest pattern
  - leftmost-first: the leftmost start, then the earliest-registered pattern
Which copy of a duplicate find_iter / leftmost-longest report is not fixed by these definitions: that detail is compared with the
oracle only (it reports the first registered copy)."""
from collections import Counter, defaultdict

import numpy as np
import pytest

from daachorse_amd import synth
from oracle import oracle as orc


def _occurrences(pats, vals, text):
    """(start, end, value, index) of every occurrence of every pattern, by naive search"""
    out = []
    for i, (p, v) in enumerate(zip(pats, vals)):
        at = text.find(p)
        while at >= 0:
            out.append((at, at + len(p), int(v), i))
            at = text.find(p, at + 1)
    return out


def _sev(m):
    return [(int(x["start"]), int(x["end"]), int(x["value"])) for x in m]


def _check_overlapping(got, occ):
    assert Counter(got) == Counter((s, e, v) for s, e, v, _ in occ)
    assert [e for _, e, _ in got] == sorted(e for _, e, _ in got)       # by end
    reg = defaultdict(list)
    for s, e, v, i in sorted(occ, key=lambda t: t[3]):
        reg[(s, e)].append(v)
    by_end = defaultdict(list)
    for s, e, v in got:
        by_end[e].append((s, v))
    for e, row in by_end.items():
        starts = [s for s, _ in row]
        assert starts == sorted(starts), e                                # longer patterns first
        for s in set(starts):
            assert [v for s2, v in row if s2 == s] == reg[(s, e)], (s, e)  # copies in registration order


def _standard(occ, n):
    """earliest end, then the longest pattern ending there; the next match starts at or after that end.  -> (start, end, {values})"""
    by_end = defaultdict(list)
    for s, e, v, i in occ:
        by_end[e].append((s, v, i))
    out, pos = [], 0
    for e in sorted(by_end):
        cands = [(s, v) for s, v, _ in by_end[e] if s >= pos]
        if not cands:
            continue
        s = min(s for s, _ in cands)
        out.append((s, e, {v for s2, v in cands if s2 == s}))
        pos = e
    return out


def _leftmost(occ, longest):
    by_start = defaultdict(list)
    for s, e, v, i in occ:
        by_start[s].append((e, v, i))
    out, pos = [], 0
    for s in sorted(by_start):
        if s < pos:
            continue
        row = by_start[s]
        if longest:
            e = max(e for e, _, _ in row)
            out.append((s, e, {v for e2, v, _ in row if e2 == e}))
        else:
            e, v, _ = min(row, key=lambda t: t[2])
            out.append((s, e, {v}))
        pos = e
    return out


def _check_stream(got, want):
    """start and end exactly; the value one of the pattern's copies (the copy itself is the oracle's to pick)"""
    assert [(s, e) for s, e, _ in got] == [(s, e) for s, e, _ in want]
    for (s, e, v), (_, _, vs) in zip(got, want):
        assert v in vs, (s, e, v, vs)


def _check_all(pats, vals, text):
    occ = _occurrences(pats, vals, text)
    o = orc.OraclePma.build(pats, values=vals)
    _check_overlapping(_sev(o.find_overlapping_iter(text)), occ)
    std = _sev(o.find_iter(text))
    _check_stream(std, _standard(occ, len(text)))
    first_copy = {}
    for p, v in zip(pats, vals):
        first_copy.setdefault(p, int(v))
    assert all(v == first_copy[text[s:e]] for s, e, v in std)   # (the oracle reports a duplicate's first copy)
    for kind, longest in ((orc.LEFTMOST_LONGEST, True), (orc.LEFTMOST_FIRST, False)):
        lo = orc.OraclePma.build(pats, values=vals, kind=kind)
        got = _sev(lo.leftmost_find_iter(text))
        _check_stream(got, _leftmost(occ, longest))
        assert all(v == first_copy[text[s:e]] for s, e, v in got)
    return occ


def test_values_family():
    """full-range values (synth.full_range_values: 0, 1, 2^31 - 1, 2^31, 2^32 - 2, 2^32 - 1, no value equal to its index) come out
    unchanged from every stream"""
    pats, vals, text = synth.patterns_values(300, text_bytes=20000)
    assert set(synth.EDGE_VALUES) <= set(vals.tolist()) and not np.any(vals == np.arange(len(vals)))
    occ = _check_all(pats, vals, text)
    assert {v for _, _, v, _ in occ} & set(synth.EDGE_VALUES)


@pytest.mark.parametrize("K", [2, 3])
def test_lengths_family(K):
    """patterns at every packing length up to 4097 bytes (K, K+1, K+16, K+17, 19, 20, 31 .. 33, 63 .. 65, 255, 256, 1023 .. 1025, 4097) and
    their prefixes / suffixes, planted across cuts: each long pattern is found where it was planted"""
    pats, vals, text = synth.patterns_lengths(K, max_len=4097, n_words=60)
    assert {K, K + 1, K + 16, K + 17, 19, 20, 33, 65, 256, 1025, 4097} <= {len(p) for p in pats}
    occ = _check_all(pats, vals, text)
    found = Counter(e - s for s, e, _, _ in occ)
    assert all(found[L] >= 3 for L in (K + 17, 64, 1024, 4097)), found


def test_lengths_family_full():
    """the whole length list (to 65 537 bytes): the overlapping stream only (the restart streams are covered above)"""
    pats, vals, text = synth.patterns_lengths(3)
    assert max(len(p) for p in pats) == 65537
    occ = _occurrences(pats, vals, text)
    _check_overlapping(_sev(orc.OraclePma.build(pats, values=vals).find_overlapping_iter(text)), occ)
    assert sum(e - s == 65537 for s, e, _, _ in occ) == 3


@pytest.mark.parametrize("n_copies", [2, 255, 256, 257])
def test_copies_family(n_copies):
    """one long pattern registered 2 .. 257 times, one K-byte pattern twice: every copy is reported, in registration order, with its own value"""
    pats, vals, text = synth.patterns_copies(n_copies, 3, text_bytes=6000)
    long_w = max(set(pats), key=pats.count)
    assert pats.count(long_w) == n_copies and len(set(vals.tolist())) == len(vals)
    occ = _check_all(pats, vals, text)
    assert sum(1 for s, e, _, i in occ if pats[i] == long_w) == n_copies * text.count(long_w) > 0


def test_charwise_outputs_family():
    """charwise: the output count is the pattern count (copies included), and the overlapping stream is the brute force's"""
    pats, vals, text = synth.patterns_charwise_outputs(5000, n_words=500, text_bytes=20000)
    text.decode("utf-8")
    assert len(pats) == 5000
    o = orc.OracleCharwisePma.build(pats, values=vals)
    assert len(o.outputs()) == 5000                                    # (a copy adds an output)
    assert len(orc.OracleCharwisePma.build(pats[:-1], values=vals[:-1]).outputs()) == 4999
    occ = _occurrences(pats, vals, text)
    _check_overlapping(_sev(o.find_overlapping_iter(text)), occ)
    assert sum(1 for _, _, _, i in occ if pats[i] == pats[-1]) == len(pats) - 500   # the bulk copies: their pattern once in the text
    for kind, longest in ((orc.LEFTMOST_LONGEST, True), (orc.LEFTMOST_FIRST, False)):
        _check_stream(_sev(orc.OracleCharwisePma.build(pats, values=vals, kind=kind).leftmost_find_iter(text)), _leftmost(occ, longest))
    _check_stream(_sev(o.find_iter(text)), _standard(occ, len(text)))
