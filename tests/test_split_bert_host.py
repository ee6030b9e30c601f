"""Split.Bert (DAAC_SPLIT_BERT), bert_char_classes() and daac_split_words_space on the host side: the classes against unicodedata and
daac_splitter_create, the sequential scanner of tests/wordpiece_golden.py on hand cases, every answer the C ABI gives before it touches
a device, and the rule's branch of split_start with the words-space body run on the CPU under ASan and UBSan
(tests/native/split_bert_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
import os
import subprocess
import unicodedata

import numpy as np
import pytest

import wordpiece_golden as wg

import daachorse_amd as da
from daachorse_amd import Split, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHITE = {0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000}


def _err():
    return _ffi.lib().daac_last_error().decode()


def test_split_bert_is_exported_and_creates():
    assert int(Split.Bert) == 6 and Split.Bert.name == "Bert"
    assert hasattr(C.CDLL(_ffi._build.LIB_PATH), "daac_split_words_space")
    assert callable(da.Splitter.words_space) and callable(da.bert_char_classes)
    for classes in (None, da.bert_char_classes(), np.zeros((0, 3), dtype=np.uint32)):
        sp = da.Splitter(Split.Bert, classes)
        assert sp.rule == 6
        sp.free()
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_bert_char_classes_are_sorted_disjoint_and_accepted():
    cc = da.bert_char_classes()
    assert cc is da.bert_char_classes() and cc.dtype == np.uint32 and cc.ndim == 2 and cc.shape[1] == 3 and not cc.flags.writeable
    assert (cc[:, 0] <= cc[:, 1]).all() and (cc[1:, 0] > cc[:-1, 1]).all() and cc[0, 0] >= 0x80 and cc[-1, 1] <= 0x10FFFF
    assert set(cc[:, 2].tolist()) == {1, 2, 3}
    h = C.c_void_p()
    assert _ffi.lib().daac_splitter_create(int(Split.Bert), cc.ctypes.data, cc.shape[0], C.byref(h)) == 0, _err()
    _ffi.lib().daac_splitter_free(h)
    table = wg.class_table(cc)
    for cp in range(0x80, 0x110000):
        cat = unicodedata.category(chr(cp))[0]
        want = wg.S if cp in WHITE else wg.O if cat == "P" else wg.N if cat == "N" else wg.L
        assert table[cp] == want, hex(cp)
    # what BERT leaves inside words: marks, symbols, controls, unassigned code points, surrogates
    for cp in (0x301, 0x20AC, 0xAD, 0x200B, 0x378, 0xD800, 0x10FFFF):
        assert table[cp] == wg.L, hex(cp)
    for cp in (0xBF, 0x2014, 0x3001, 0xFF01):
        assert table[cp] == wg.O, hex(cp)
    # below U+0080 the fixed classes are BERT's: every printable character that is neither alphanumeric nor a space is punctuation
    for cp in range(0x21, 0x7F):
        assert (table[cp] == wg.O) == (not chr(cp).isalnum()), hex(cp)


def test_bert_scan_hand_cases():
    table = wg.class_table(da.bert_char_classes())

    def words(text):
        d = text if isinstance(text, bytes) else text.encode()
        return [(d[s:e], sp) for s, e, sp in wg.bert_scan(d, table)]

    assert words("") == []
    assert words("it's  a") == [(b"it", False), (b"'", False), (b"s", False), (b"  ", True), (b"a", False)]
    assert words("a1b2 ...") == [(b"a1b2", False), (b" ", True), (b".", False), (b".", False), (b".", False)]
    assert words("世界、日本　x€5") == [("世界".encode(), False), ("、".encode(), False), ("日本".encode(), False), ("　".encode(), True), ("x€5".encode(), False)]
    assert words(" \t\n ") == [(" \t\n ".encode(), True)]
    assert words(b"a\xe3\x80") == [(b"a", False), (b"\xe3", False), (b"\x80", False)]   # a cut character is bytes of class O
    assert words(b"a\x01b") == [(b"a", False), (b"\x01", False), (b"b", False)]         # an ASCII control character is O here
    wo, dw, sp = wg.bert_offsets([b"ab cd", b"", b"!x"], table, base=3)
    assert wo.tolist() == [3, 5, 6, 8, 9, 10] and dw.tolist() == [0, 3, 3, 5] and sp.tolist() == [0, 1, 0, 0, 0]


def test_words_space_bad_arguments_answer_1_without_a_device():
    sp = da.Splitter(Split.Bert)
    L_ = _ffi.lib()
    flags = C.c_void_p()
    wo = np.zeros(3, dtype=np.uint64)   # (never read: the answers below come before a device is touched)
    assert L_.daac_split_words_space(None, b"ab", wo.ctypes.data, 2, 0, None, C.byref(flags)) == 1 and "null" in _err()
    assert L_.daac_split_words_space(sp._h, b"ab", wo.ctypes.data, 2, 0, None, None) == 1 and "null" in _err()
    assert L_.daac_split_words_space(sp._h, None, wo.ctypes.data, 2, 0, None, C.byref(flags)) == 1 and "null" in _err()
    assert L_.daac_split_words_space(sp._h, b"ab", None, 2, 0, None, C.byref(flags)) == 1 and "null" in _err()
    flags.value = 1
    assert L_.daac_split_words_space(sp._h, None, None, 0, 0, None, C.byref(flags)) == 0 and flags.value is None   # no word: NULL
    for bad in (b"ab", (b"ab",), (b"ab", np.zeros(3, dtype=np.uint64)), (b"ab", [0, 1, 2])):
        with pytest.raises(da.DaachorseError) as ei:
            sp.words_space(bad)
        assert ei.value.code == 1, bad
    sp.free()


def test_split_bert_functions_on_the_host_under_sanitizers(tmp_path):
    """the Split.Bert branch of split_start at every position of 2 x 3 000 rounds of random documents, and split_word_space on every word
    and on random byte ranges, all in buffers of exactly their size, against a sequential scanner in the same program"""
    exe = str(tmp_path / "split_bert_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "split_bert_check.cpp")])
    for seed in (1, 2):
        r = subprocess.run([exe, "3000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 3000 rounds") and r.stderr == "", (r.stdout, r.stderr)
