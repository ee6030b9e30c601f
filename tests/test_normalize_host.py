"""Normalizer, bert_normalizer() and the C ABI of daac_normalize_batch on the host side: the rules against the fixture and `tokenizers`
through a sequential scanner in Python, hand cases for each kind, every answer the C ABI gives before it touches a device, and the
per-position functions with both passes run on the CPU under ASan and UBSan (tests/native/normalize_check.cpp, a stand-alone program).
No GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import normalize_golden as ng

import daachorse_amd as da
from daachorse_amd import Norm, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _ffi.lib().daac_last_error().decode()


@functools.lru_cache(maxsize=None)
def _rules(name):
    return da.bert_normalizer_rules(*ng.OPTIONS[name])


def _normalize(text, rules, pool):
    return ng.scan(text.encode() if isinstance(text, str) else text, ng.rules_image(rules, pool))[0]


def test_normalizer_names_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_normalizer_create", "daac_normalizer_free", "daac_normalize_batch", "daac_normalize", "daac_spans_to_source"):
        assert hasattr(lib, name), name
    assert [int(k) for k in (Norm.Delete, Norm.Replace, Norm.Pad, Norm.Hangul)] == [1, 2, 3, 4]
    assert callable(da.Normalizer.normalize_batch) and callable(da.Normalizer.normalize) and callable(da.Normalizer.spans_to_source)
    assert "normalizer" in da.DoubleArrayAhoCorasick.tokenize_wordpiece_docs.__code__.co_varnames
    assert "normalizer" in da.CharwiseDoubleArrayAhoCorasick.tokenize_wordpiece_docs.__code__.co_varnames


@pytest.mark.parametrize("name", sorted(ng.OPTIONS))
def test_bert_rules_are_sorted_disjoint_and_accepted(name):
    rules, pool = _rules(name)
    assert rules.dtype == np.uint32 and rules.ndim == 2 and rules.shape[1] == 5 and len(rules) > 10
    assert (rules[:, 0] <= rules[:, 1]).all() and (rules[1:, 0] > rules[:-1, 1]).all() and rules[-1, 1] <= 0x10FFFF
    assert set(rules[:, 2].tolist()) <= {1, 2, 3, 4}
    rep = rules[rules[:, 2] == int(Norm.Replace)]
    assert (rep[:, 3].astype(np.int64) + rep[:, 4] <= len(pool)).all() and rep[:, 4].max() <= da.bytewise.NORM_MAX_LEN
    assert not ((rules[:, 0] <= 0xDFFF) & (rules[:, 1] >= 0xD800)).any()   # no rule touches a surrogate
    nz = da.Normalizer(rules, pool)   # daac_normalizer_create validates without a device
    # the private-use, CJK and Hangul ranges collapse to a block each: far below one entry per mapped code point
    assert 0 < nz.table_bytes < 256 * 1024
    nz.free()


def test_bert_rules_default_shape():
    rules, pool = _rules("default")
    mapped = int((rules[:, 1].astype(np.int64) - rules[:, 0] + 1).sum())
    assert 230_000 < mapped < 240_000          # about 234 000 code points are not mapped to themselves
    assert int(rules[rules[:, 2] == 2][:, 4].max()) == 12   # the longest image
    hangul = rules[rules[:, 2] == int(Norm.Hangul)]
    assert hangul[:, :2].tolist() == [[0xAC00, 0xD7A3]]
    assert da.bert_normalizer() is da.bert_normalizer(strip_accents=True)   # None means "as lowercase"; cached per option set


@pytest.mark.parametrize("name", sorted(ng.OPTIONS))
def test_rules_scanner_equals_the_fixture(name):
    rules, pool = _rules(name)
    image = ng.rules_image(rules, pool)
    for d, want in zip(ng.docs(), ng.expected(name)):
        assert ng.scan(d, image)[0] == want, d


@pytest.mark.parametrize("name", sorted(ng.OPTIONS))
def test_rules_equal_the_definition_per_code_point(name):
    """per code point, the rules against the four steps composed (normalize_golden.bert_image): every code point outside the uniform
    interiors of the CJK, Hangul, private-use and unassigned ranges, and both edges of each of those"""
    image = ng.rules_image(*_rules(name))
    opts = ng.OPTIONS[name]
    for lo, hi in ((0, 0x3500), (0x4DB0, 0x4E10), (0x9FF0, 0xAC20), (0xD780, 0xD7FF), (0xE000, 0xE010), (0xF8F0, 0x20010), (0x2A6D0, 0x2A710), (0x2B730, 0x2B750),
                   (0x2B810, 0x2B930), (0x2CEA0, 0x2CEC0), (0x2F7F0, 0x2FA30), (0xE0000, 0xE01FF), (0xEFFF0, 0xF0010), (0xFFFF0, 0x100010), (0x10FFF0, 0x10FFFF)):
        for cp in range(lo, hi + 1):
            raw = chr(cp).encode()
            assert image(cp, raw) == ng.bert_image(cp, *opts).encode(), hex(cp)


@pytest.mark.parametrize("name", sorted(ng.OPTIONS))
def test_rules_scanner_equals_tokenizers(name):
    tokenizers = pytest.importorskip("tokenizers")
    o = ng.OPTIONS[name]
    norm = tokenizers.normalizers.BertNormalizer(clean_text=o[0], handle_chinese_chars=o[1], strip_accents=o[2], lowercase=o[3])
    image = ng.rules_image(*_rules(name))
    for d in ng.docs():
        assert ng.scan(d, image)[0] == norm.normalize_str(d.decode()).encode(), d


def test_hand_cases():
    default, keep = _rules("default"), _rules("keep_accents")
    assert _normalize("H\u00e9llo WORLD", *default) == b"hello world"
    assert _normalize("He\u0301llo", *default) == b"hello"                                       # a combining accent
    assert _normalize("H\u00e9llo", *keep) == "h\u00e9llo".encode()
    assert _normalize("a\0b\ufffdc\u200dd\ue000e\x07f", *default) == b"abcdef"                   # Delete
    assert _normalize("a\tb\nc\u00a0d\u3000e", *default) == b"a b c d e"                          # Replace, a range with one image
    assert _normalize("x\u4e2dy", *default) == "x \u4e2d y".encode()                             # Pad
    assert _normalize("\uac01\uac00", *default) == "\u1100\u1161\u11a8\u1100\u1161".encode()    # Hangul: three jamo and two
    assert _normalize("\uac01", *keep) == "\uac01".encode()
    assert _normalize("\uf900", *default) == " \u8c48 ".encode()                                 # a compatibility ideograph: padded, then decomposed
    assert _normalize("\uf900", *_rules("clean_only")) == "\uf900".encode()
    assert _normalize("\u0130", *default) == b"i" and _normalize("\u0130", *keep) == "i\u0307".encode()
    assert _normalize("\u039f\u0394\u039f\u03a3 \u1e9e \u01c5", *keep) == "\u03bf\u03b4\u03bf\u03c3 \u00df \u01c6".encode()   # no final sigma
    assert _normalize("\0\u200d\ufffd\ue000", *default) == b""                                  # a document that becomes empty
    assert _normalize(b"A\xc3(\xe4\xb8", *default) == b"a\xc3(\xe4\xb8"                          # ill-formed bytes are copied
    out, src = ng.scan("\ud55c\u00c9\u4e2dx".encode(), ng.rules_image(*default))
    assert out == "\u1112\u1161\u11ab".encode() + b"e \xe4\xb8\xad x" and src == [0] * 9 + [3] + [5] * 5 + [8]


def test_spans_to_source_definition():
    raw = "\ud55c\u00c9\u4e2dx".encode()
    out, src = ng.scan(raw, ng.rules_image(*_rules("default")))
    jamo = [(0, 3), (3, 6), (6, 9)]
    assert ng.spans_to_source(jamo + [(9, 10), (11, 14), (15, 16)], src, raw) == [(0, 3)] * 3 + [(3, 5), (5, 8), (8, 9)]
    assert ng.spans_to_source([(0, 0), (10, 10), (16, 16)], src, raw) == [(0, 0), (5, 5), (9, 9)]
    a = b"A\0b"
    out, src = ng.scan(a, ng.rules_image(*_rules("default")))
    assert out == b"ab" and ng.spans_to_source([(0, 1), (1, 2), (0, 2)], src, a) == [(0, 1), (2, 3), (0, 3)]


def test_fixture_tokens_follow_from_the_definitions():
    """rules scanner -> Split.Bert -> WordPiece -> spans_to_source gives the full Tokenizer's ids and offsets on every document"""
    import wordpiece_golden as wg
    vocab, unk_id, max_chars, prefix = wg.model()
    table = wg.class_table(da.bert_char_classes())
    image = ng.rules_image(*_rules("default"))
    ids, spans = ng.tokens()
    differ = 0
    for d, want_ids, want_spans in zip(ng.docs(), ids, spans):
        out, src = ng.scan(d, image)
        got_ids, got_spans = wg.wordpiece_doc(out, table, vocab, unk_id, max_chars, prefix.encode())
        assert (got_ids, ng.spans_to_source(got_spans, src, d)) == (want_ids, want_spans), d
        differ += wg.wordpiece_doc(d, table, vocab, unk_id, max_chars, prefix.encode())[0] != want_ids
    assert differ > len(ids) // 2   # the normalizer matters to most documents


# ------------------------------------------------------------------------------------------------ status 1, before a device is touched
def _create(rows, pool=b"", n=None, null_out=False, null_pool=False):
    a = np.array(rows, dtype=np.uint32).reshape(-1, 5)
    p = np.frombuffer(pool or b"\0", dtype=np.uint8)
    h = C.c_void_p()
    st = _ffi.lib().daac_normalizer_create(a.ctypes.data if a.size else None, len(a) if n is None else n, None if null_pool else p.ctypes.data, len(pool),
                                           None if null_out else C.byref(h))
    if st == 0:
        _ffi.lib().daac_normalizer_free(h)
    return st


def test_create_refuses_bad_rules():
    D, R, P, H = 1, 2, 3, 4
    assert _create([]) == 0 and _create([(0x41, 0x5A, D, 0, 0), (0x61, 0x61, R, 1, 2)], b"xyz") == 0
    bad = {
        "a NULL out": dict(rows=[], null_out=True),
        "NULL rules with a count": dict(rows=[], n=2),
        "a NULL pool with a length": dict(rows=[], pool=b"ab", null_pool=True),
        "unsorted": dict(rows=[(0x61, 0x61, D, 0, 0), (0x41, 0x41, D, 0, 0)]),
        "overlapping": dict(rows=[(0x41, 0x50, D, 0, 0), (0x50, 0x5A, D, 0, 0)]),
        "last < first": dict(rows=[(0x42, 0x41, D, 0, 0)]),
        "last above U+10FFFF": dict(rows=[(0x10FFFF, 0x110000, D, 0, 0)]),
        "an unknown kind": dict(rows=[(0x41, 0x41, 5, 0, 0)]),
        "kind 0": dict(rows=[(0x41, 0x41, 0, 0, 0)]),
        "a surrogate in a Replace single": dict(rows=[(0xD800, 0xD800, R, 0, 1)], pool=b"x"),
        "off + len beyond the pool": dict(rows=[(0x41, 0x41, R, 2, 2)], pool=b"xyz"),
        "len above the cap": dict(rows=[(0x41, 0x41, R, 0, 256)], pool=b"x" * 300),
        "Hangul below its block": dict(rows=[(0xABFF, 0xAC00, H, 0, 0)]),
        "Hangul above its block": dict(rows=[(0xD7A3, 0xD7A4, H, 0, 0)]),
    }
    for what, kw in bad.items():
        assert _create(**kw) == 1, what
        assert _err(), what
    assert _create([(0x41, 0x41, R, 0, 255)], b"x" * 255) == 0 and _create([(0xAC00, 0xD7A3, H, 0, 0)]) == 0 and _create([(0x41, 0x41, P, 9, 9)]) == 0
    with pytest.raises(da.DaachorseError):
        da.Normalizer([(1, 2, 3)])


def test_normalize_batch_status_1_without_a_device():
    lib = _ffi.lib()
    nz = da.Normalizer([(0x41, 0x41, 1, 0, 0)])
    hay = np.frombuffer(b"abcdef", dtype=np.uint8)
    out, oo, src, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    good = np.array([0, 3, 6], dtype=np.uint64)
    down = np.array([0, 4, 3], dtype=np.uint64)

    def call(h=nz._h, hay_p=hay.ctypes.data, off=good, nd=2, want_src=0, p_out=C.byref(out), p_oo=C.byref(oo), p_src=C.byref(src), p_n=C.byref(n)):
        return lib.daac_normalize_batch(h, hay_p, off.ctypes.data if off is not None else None, nd, 0, None, want_src, p_out, p_oo, p_src, p_n)

    assert call(h=None) == 1 and call(p_out=None) == 1 and call(p_oo=None) == 1 and call(p_n=None) == 1
    assert call(want_src=1, p_src=None) == 1
    assert call(off=None) == 1 and call(off=down) == 1 and "decrease" in _err()
    assert call(hay_p=None) == 1
    assert lib.daac_normalize(None, hay.ctypes.data, 6, 0, None, 0, C.byref(out), None, C.byref(n)) == 1
    assert lib.daac_normalize(nz._h, None, 6, 0, None, 0, C.byref(out), None, C.byref(n)) == 1
    assert lib.daac_normalize(nz._h, hay.ctypes.data, 6, 0, None, 1, C.byref(out), None, C.byref(n)) == 1
    # status 6: with src a document has fewer than 2^32 - 1 bytes (host offsets: decided before the text is touched)
    huge = np.array([0, 0xFFFFFFFF], dtype=np.uint64)
    assert call(off=huge, nd=1, want_src=1) == 6 and "2^32" in _err()
    # spans_to_source
    sp = np.zeros(2, dtype=np.uint64)
    assert lib.daac_spans_to_source(None, sp.ctypes.data, sp.ctypes.data, sp.ctypes.data, hay.ctypes.data, good.ctypes.data, 2, 1, 0, None) == 1
    assert lib.daac_spans_to_source(sp.ctypes.data, sp.ctypes.data, sp.ctypes.data, sp.ctypes.data, hay.ctypes.data, down.ctypes.data, 2, 1, 0, None) == 1
    assert lib.daac_spans_to_source(sp.ctypes.data, sp.ctypes.data, sp.ctypes.data, sp.ctypes.data, hay.ctypes.data, good.ctypes.data, 0, 1, 0, None) == 1
    assert lib.daac_spans_to_source(None, None, None, None, None, None, 0, 0, 0, None) == 0
    nz.free()
    with pytest.raises(da.DaachorseError):
        nz.normalize_batch([b"a"])


def test_normalize_functions_on_the_host_under_sanitizers(tmp_path):
    """norm_unit and norm_store at every position of 2 x 3 000 random batches, both passes at tiles of 64, 128 and 1024 positions with
    src and out_offsets, and norm_span_to_source on random spans, all in buffers of exactly their size, against a sequential scanner in
    the same program"""
    exe = str(tmp_path / "normalize_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "normalize_check.cpp")])
    for seed in (1, 2):
        r = subprocess.run([exe, "3000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 3000 rounds") and r.stderr == "", (r.stdout, r.stderr)
