"""tests/gram_exact.py on the CPU (no GPU): the generators are deterministic, every feature the GPU tests aim at is in the dictionaries and
the texts, the zero-hash constants hash to zero, and the oracle alone answers every case the GPU tests ask it."""
import numpy as np
import pytest

from daachorse_amd import synth
from oracle import oracle as orc

import gram_exact as ge

NAMES = list(ge.SPECS)


def test_generators_are_deterministic():
    for name in NAMES:
        a, b = ge.Dictionary(name), ge.Dictionary(name)
        assert a.words == b.words and a.paths == b.paths
        for kind in ge.KINDS:
            assert np.array_equal(a.text(kind), b.text(kind)) and len(a.text(kind)) == ge.TEXT_BYTES
        assert np.array_equal(a.text_of(a.words, 50_000, 21), b.text_of(b.words, 50_000, 21))
    a, b = ge.zero_hash_cases(), ge.zero_hash_cases()
    assert list(a) == list(b) == ["z_short", "z_k3", "z_k2", "z_deep", "dup_k", "four_short"]
    for name in a:
        assert a[name][0] == b[name][0] and np.array_equal(a[name][1], b[name][1]) and a[name][2] == b[name][2]
        assert np.array_equal(ge.special_text(a[name][0], a[name][2]), ge.special_text(b[name][0], b[name][2]))


def _single_path_below(words, head):
    """the words that pass through `head`, as the edges of the trie below it: one path?"""
    below = sorted({w[len(head):] for w in words if w[:len(head)] == head and len(w) > len(head)}, key=len)
    return all(below[-1][:len(x)] == x for x in below), len(below[-1]), len(below)


def test_k3s_has_what_the_kernels_are_aimed_at():
    d = ge.dictionary("k3s")
    words, lens = d.words, {len(w) for w in d.words}
    assert 380 <= len(words) <= 480 and set(b"".join(words)) == set(ge.ALPHA8)
    assert {1, 2, 3, 4, 5} <= lens                      # short patterns for K = 3 and K = 2, own patterns at depth 4 and 5
    have = set(words)
    assert sum(1 for w in words if len(w) >= 7 and w[:4] in have and w[:5] in have) >= 10   # words that are prefixes of longer words
    # single paths of 9 .. 16 edges below depth 6: the state at depth 6 + edges - 8 is a tail record (at most 8 edges, gram.cpp:146), the
    # states above it on the path are ordinary records
    assert [len(w) - 6 for w in d.paths] == ge.PATH_EDGES
    for w in d.paths:
        single, edges, ends = _single_path_below(words, w[:6])
        assert single and edges == len(w) - 6 and ends == (2 if edges in (12, 15) else 1), (w, single, edges, ends)
    assert len(d.long_word) == 22
    # tail records right below the walkers' first record: a word of 7 or 8 letters alone below its depth-6 / depth-5 state
    assert any(len(w) in (7, 8) and _single_path_below(words, w[:6])[2] == 1 for w in words)
    assert all(len(w) >= 4 for w in ge.dictionary("k3n").words) and ge.dictionary("k3n").words == [w for w in words if len(w) >= 4]
    assert ge.dictionary("k2s").words == words and ge.dictionary("k2n").words == [w for w in words if len(w) >= 3]
    assert ge.dictionary("k2s").budget == ge.dictionary("k2n").budget == ge.K2_BUDGET
    # K2_BUDGET lies between what build_gram_tables needs for K = 2 and for K = 3 with nine classes (gram.cpp:89), whatever COMBO holds
    pad16 = lambda x: (x + 15) & ~15

    def table_bytes(C, K, combos):
        bwords = (C ** (K + 1) + 31) // 32
        return 1024 + pad16(C ** K * 2) + pad16(combos * 8) + pad16(bwords * 4 + 8) + pad16((bwords + 1) // 2) + pad16((bwords + 7) // 8 * 4) + 64
    assert table_bytes(9, 2, 9 ** 2 + 1) <= ge.K2_BUDGET < table_bytes(9, 3, 1)


def test_wide_and_32_class_dictionaries():
    w40 = ge.dictionary("w40")
    assert set(b"".join(w40.words)) == set(ge.ALPHA39) and len(ge.ALPHA39) == 39 and len(w40.long_word) == 22
    c32, c32n = ge.dictionary("c32"), ge.dictionary("c32n")
    # c32n: c32 without its one- and two-byte words — no short pattern for K = 2 —, still all 31 bytes, the stem and what stands behind it
    assert c32n.words == [w for w in c32.words if len(w) >= 3] and min(len(w) for w in c32.words) == 1 and len(c32n.words) < len(c32.words)
    assert bytes(sorted(set(b"".join(c32n.words)))) == ge.ALPHA31 and all(w in c32n.words for w in ge.C32_WORDS)
    used = sorted(set(b"".join(c32.words)))
    assert bytes(used) == ge.ALPHA31 and len(used) == 31
    # classes are numbered over the used bytes in ascending order (repack.cpp): '_' is class 31, 'O' class 15
    assert used.index(ge.Z31[0]) + 1 == 31 and used.index(ge.Z15[0]) + 1 == 15
    have = set(c32.words)
    assert all(w in have for w in ge.C32_WORDS)
    assert not any(w.startswith(ge.STEM + ge.Z15) or w.startswith(ge.STEM + b"E" + ge.Z15) for w in c32.words)
    assert sum(1 for w in c32.words if w.startswith(ge.STEM)) == len(ge.C32_WORDS)


@pytest.mark.parametrize("name", ["c32", "c32n"])
def test_c32_texts_carry_the_class_31_byte_at_the_lane_63_edges(name):
    d = ge.dictionary(name)
    for kind in ge.KINDS:
        t = d.text(kind).tobytes()
        for last, behind in ge.C32_PLANTS:
            assert t[last - 2:last + 1 + len(behind)] == (ge.STEM + behind)[:ge.TEXT_BYTES - (last - 2)], (kind, last)
        ends = {int(e) for e in d.tuples(kind)["end"]}
        # first behind the stem at 1023 mod 1024 (both) and 2047 mod 2048; second behind it at 2047 mod 2048; both at 1023 mod 1024
        assert t[1024] == ge.Z31[0] and t[4096] == ge.Z31[0] and t[2049] == ge.Z31[0] and t[3072:3074] == ge.Z31 * 2
        assert {1025, 1026, 2050, 2051, 3073, 3074, 4097, 4098} <= ends       # the words through the class-31 byte end there
        assert t[-1] == ge.Z31[0] and t[-5:-2] == ge.STEM and ge.TEXT_BYTES in ends
        for n in (1025, 2050, 4097):                                          # lengths at which the class-31 byte is the text's last
            assert t[n - 1] == ge.Z31[0] and n in ge.LENGTHS + ge.C32_LENGTHS
        # the controls with the class-15 byte in the same places: the stem, and nothing through the byte behind it
        assert t[5120] == ge.Z15[0] and 5120 in ends and not any(int(m["start"]) == 5117 and int(m["end"]) > 5120 for m in d.tuples(kind))


def test_soup_ends_inside_a_tail_record_when_cut():
    for name in ("k3s", "k3n", "k2s", "k2n", "w40"):
        d = ge.dictionary(name)
        t = d.text("soup").tobytes()
        assert t.endswith(d.long_word)
        full = d.answer("soup")
        for cut in range(1, 10):
            assert d.answer("soup", ge.TEXT_BYTES - cut)[0] < full[0]
        m = d.tuples("soup")
        assert any(int(x["end"]) == ge.TEXT_BYTES and int(x["end"] - x["start"]) == 22 for x in m)
        # every third word is cut short, fillers of no pattern separate some words: soup is not deep
        assert sum(t.count(bytes([b])) for b in ge.OUTSIDE) > 200
        assert not any(b in d.text("deep").tobytes() for b in ge.OUTSIDE)
        assert all(d.text("uniform").tobytes().count(bytes([b])) > 20 for b in ge.OUTSIDE)


def test_zero_hash_constants():
    for length, values in ge.ZERO_HASH.items():
        for v in values:
            z = int(synth.mix64(np.uint64((v << 32) | length)))
            assert z & 0xFFFFFFFF == 0 and ge.match_hash32(v, length) == 0, (length, v, hex(z))
    assert ge.match_hash32(1, 4) != 0
    assert sorted(ge.ZERO_HASH) == [2, 3, 4, 7, 8]


def test_zero_hash_cases_hold_their_special_words():
    base = set(ge.dictionary("k3s").words)
    cases = ge.zero_hash_cases()
    shape = {"z_short": [2], "z_k3": [4], "z_k2": [3, 4], "z_deep": [7, 8, 8, 8], "dup_k": [4], "four_short": [3, 2, 1]}
    for name, (pats, vals, special) in cases.items():
        assert sorted(len(w) for w in special) == sorted(shape[name]), (name, special)
        assert len(pats) == len(vals) and pats[:len(base)] == ge.dictionary("k3s").words
        zero = [(w, int(v)) for w, v in zip(pats, vals) if ge.match_hash32(int(v), len(w)) == 0]
        assert [len(w) for w, _ in zero] == {"z_short": [2], "z_k3": [4], "z_k2": [3, 4], "z_deep": [7, 8]}.get(name, []), (name, zero)
        t = ge.special_text(pats, special)
        raw = t.tobytes()
        assert len(t) == ge.TEXT_BYTES
        for w in special:
            assert raw.count(w) >= (7 if w in (special[0], special[-1]) else 1), (name, w)
        # every special word once cut one byte short, between fillers, where special_text plants them (the piece ends at offset 5000)
        blank = ge.OUTSIDE[:1]
        cut = blank + blank.join(w[:-1] for w in special) + blank
        assert raw[5000 - len(cut):5000] == cut and all(blank + w[:-1] + blank in cut for w in special), (name, cut)
        first, last = special[0], special[-1]
        assert raw[len(first) + 1:].startswith(last) and raw[:-(len(last) + 1)].endswith(first)
        assert raw[:3072].endswith(first) and raw[:4096].endswith(last)
        assert raw.startswith(special[0]) and raw.endswith(special[-1])
        assert raw[:1024].endswith(special[-1]) and raw[:2048].endswith(special[0])
        # the oracle, built with the values, answers: count and checksum over the tuples it lists
        o = orc.OraclePma.build(pats, values=vals)
        m = o.find_overlapping_iter(t)
        assert o.overlapping_count(t) == (len(m), orc.matches_checksum(m))
        for w in special:
            want_vals = {int(v) for x, v in zip(pats, vals) if x == w}
            assert want_vals <= {int(v) for v in m["value"]}, (name, w)
    # z_deep: one zero-hash word on a branching path, one alone at the end of a single path below depth 6
    pats, _, special = cases["z_deep"]
    w7, w8 = special[0], special[-1]
    assert len(w7) == 7 and len(w8) == 8 and sum(1 for w in pats if w[:7] == w7) == 3
    assert [w for w in pats if w[:6] == w8[:6]] == [w8]
    # dup_k: the same four-byte word twice; four_short: four patterns ending at one 3-gram
    assert cases["dup_k"][0].count(cases["dup_k"][2][0]) == 2
    p4, s3 = cases["four_short"][0], cases["four_short"][2][0]
    assert p4.count(s3) == 2 and p4.count(s3[1:]) == 1 and p4.count(s3[2:]) == 1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_answers_every_case(name):
    """prefixes and shards as subsets of one find_overlapping_iter per text = the oracle run on the prefix itself"""
    d = ge.dictionary(name)
    halo = max(len(w) for w in d.words) - 1
    for kind in ge.KINDS:
        t = d.text(kind)
        m = d.tuples(kind)
        assert len(m) > 0 and d.answer(kind) == (len(m), orc.matches_checksum(m)) == d.oracle.overlapping_count(t)
        for n in ge.LENGTHS + ge.C32_LENGTHS:
            assert d.answer(kind, n) == d.oracle.overlapping_count(t[:n]), (name, kind, n)
        for begin in (1, 3, 4, halo, halo + 1, 1024, 2049, ge.TEXT_BYTES - 1):
            got = d.answer(kind, None, begin)
            assert got[0] == int((m["end"] > begin).sum()) and got[0] + d.answer(kind, begin)[0] == len(m)
    # deep text hits and goes on past depth K + 2 everywhere (matches of six bytes and more: walkers), uniform text seldom
    def long_matches(kind):
        m = d.tuples(kind)
        return int((m["end"] - m["start"] >= 6).sum())
    assert long_matches("deep") > 400 and long_matches("deep") > 5 * long_matches("uniform"), (long_matches("deep"), long_matches("uniform"))
