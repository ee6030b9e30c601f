"""split_batch (daac_splitter_create / daac_split_batch / daac_split / daac_offsets_compose) on the host side: a pure-Python sequential
scanner `_scan` that restates the definition (the GPU tests' reference), that scanner against the `regex` module where it is installed,
char_classes() against unicodedata, every answer the C ABI gives before it touches a device, and the kernel file's per-position
functions run on the CPU under ASan and UBSan (tests/native/split_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
import os
import random
import subprocess
import unicodedata

import numpy as np
import pytest

import daachorse_amd as da
from daachorse_amd import Split, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GPT2_PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
WHITESPACE_PATTERN = r"\s+|\S+"
O, L, N, S = 0, 1, 2, 3

# what random documents are drawn from: the contraction letters, ', space, newline, a letter, a digit, punctuation, characters of two,
# three and four bytes of every class, and malformed UTF-8
ALPHABET = ([c.encode() for c in "streveml" "ld" "'' " " \nA7!"] + [c.encode("utf-8") for c in "\u00e9\u6f22\u0663\u00b2\u0085\u00a0\u3000\U0001d400"] +
            [bytes.fromhex(h) for h in ("80", "C3", "E6BC", "EDA080", "F4908080", "C0AF", "E080AF", "F09F", "FF")])


# ------------------------------------------------------------------------------------------------------------- the definition
_tables = {}


def _class_array(classes):
    """classes (rows {first, last, cls}) -> the class of every code point, the fixed ASCII classes included"""
    key = id(classes)
    if key not in _tables:
        a = np.zeros(0x110000, dtype=np.uint8)
        for first, last, cls in np.asarray(classes).reshape(-1, 3).tolist():
            a[first:last + 1] = cls
        a[:0x80] = O
        a[ord("A"):ord("Z") + 1] = L
        a[ord("a"):ord("z") + 1] = L
        a[ord("0"):ord("9") + 1] = N
        a[0x09:0x0E] = S
        a[0x20] = S
        _tables[key] = (classes, a.tolist())   # (the key's object is kept alive)
    return _tables[key][1]


def _well_formed(d, i):
    """Unicode Table 3-7 at d[i:] -> (bytes, code point) of a well-formed sequence inside d, or (0, None)"""
    n = len(d)
    b0 = d[i]

    def cont(k, lo=0x80, hi=0xBF):
        return k < n and lo <= d[k] <= hi

    if 0xC2 <= b0 <= 0xDF:
        if cont(i + 1):
            return 2, (b0 & 0x1F) << 6 | d[i + 1] & 0x3F
    elif 0xE0 <= b0 <= 0xEF:
        lo, hi = (0xA0, 0xBF) if b0 == 0xE0 else (0x80, 0x9F) if b0 == 0xED else (0x80, 0xBF)
        if cont(i + 1, lo, hi) and cont(i + 2):
            return 3, (b0 & 0x0F) << 12 | (d[i + 1] & 0x3F) << 6 | d[i + 2] & 0x3F
    elif 0xF0 <= b0 <= 0xF4:
        lo, hi = (0x90, 0xBF) if b0 == 0xF0 else (0x80, 0x8F) if b0 == 0xF4 else (0x80, 0xBF)
        if cont(i + 1, lo, hi) and cont(i + 2) and cont(i + 3):
            return 4, (b0 & 0x07) << 18 | (d[i + 1] & 0x3F) << 12 | (d[i + 2] & 0x3F) << 6 | d[i + 3] & 0x3F
    return 0, None


_units_of_last = [None, None]   # the last document's units: both rules scan the same document


def _units(d, classes):
    """-> (at, cls, byte): per unit its first byte's position, its class, and its byte if it is a single ASCII byte (else -1)"""
    if _units_of_last[0] == (d, id(classes)):
        return _units_of_last[1]
    table = _class_array(classes)
    at, cls, byte = [], [], []
    i, n = 0, len(d)
    while i < n:
        at.append(i)
        b0 = d[i]
        if b0 < 0x80:
            cls.append(table[b0])
            byte.append(b0)
            i += 1
            continue
        k, cp = _well_formed(d, i)
        cls.append(table[cp] if k else O)
        byte.append(-1)
        i += k or 1
    _units_of_last[:] = [(d, id(classes)), (at, cls, byte)]
    return at, cls, byte


_CONTRACTIONS = (b"'s", b"'t", b"'re", b"'ve", b"'m", b"'ll", b"'d")


def _scan(doc, rule, classes):
    """The words of one document as their boundaries [0, .., len(doc)] ([0] for an empty document): the sequential scanner over the
    document's units.  At each position it tries the alternatives of the rule's pattern in order; each is greedy and gives back what it
    must (the optional space, the fifth alternative's run)."""
    d = bytes(doc)
    at, cls, byte = _units(d, classes)
    n = len(at)
    bounds = [0]

    def run(i, want):
        while i < n and (cls[i] == want):
            i += 1
        return i

    def run_not_space(i):
        while i < n and cls[i] != S:
            i += 1
        return i

    i = 0
    while i < n:
        e = i
        if rule == Split.Whitespace:
            e = run(i, S) if cls[i] == S else run_not_space(i)
        else:
            for c in _CONTRACTIONS:                                  # 's|'t|'re|'ve|'m|'ll|'d
                if list(c) == byte[i:i + len(c)]:
                    e = i + len(c)
                    break
            if e == i:
                for want in (L, N, O):                               #  ?\p{L}+ |  ?\p{N}+ |  ?[^\s\p{L}\p{N}]+
                    for first in ((i + 1, i) if byte[i] == 0x20 else (i,)):   # with the space, then without it
                        to = run(first, want)
                        if to > first:
                            e = to
                            break
                    if e != i:
                        break
            if e == i:                                               # \s+(?!\S): the whole run, then ever shorter ones
                full = run(i, S)
                for to in range(full, i, -1):
                    if to == n or cls[to] == S:
                        e = to
                        break
                if e == i:                                           # \s+
                    e = full
        assert e > i, (d, i)
        i = e
        bounds.append(at[i] if i < n else len(d))
    return bounds


def scan_batch(docs, rule, classes, base=0):
    """-> (word_offsets, doc_words) of a batch whose first document begins at `base`, as daac_split_batch defines them"""
    wo, dw, pos = [], [0], base
    for d in docs:
        b = _scan(d, rule, classes)
        wo += [pos + x for x in b[:-1]]
        dw.append(len(wo))
        pos += len(d)
    return np.array(wo + [pos], dtype=np.uint64), np.array(dw, dtype=np.uint64)


def random_doc(rng, max_pieces):
    return b"".join(rng.choice(ALPHABET) for _ in range(rng.randrange(max_pieces + 1)))


# -------------------------------------------------------------------------------------------------- the scanner against `regex`
def _ranges(table):
    """a class per code point (from U+0080 on) -> rows {first, last, cls}"""
    rows, first, cur = [], 0, 0
    for cp in range(0x80, 0x110001):
        c = table[cp] if cp < 0x110000 else 0
        if c != cur:
            if cur:
                rows.append((first, cp - 1, cur))
            first, cur = cp, c
    return np.array(rows, dtype=np.uint32).reshape(-1, 3)


@pytest.fixture(scope="module")
def regex_table():
    """the class of every code point as the `regex` module sees it: \\p{L}, \\p{N} and \\s over all code points"""
    regex = pytest.importorskip("regex")
    every = "".join(map(chr, range(0x110000)))
    table = [O] * 0x110000
    for pat, cls in ((r"\p{L}", L), (r"\p{N}", N), (r"\s", S)):
        for ch in regex.findall(pat, every):
            assert table[ord(ch)] == O, hex(ord(ch))   # the three sets are disjoint
            table[ord(ch)] = cls
    return table


def test_scan_equals_the_regex_module(regex_table):
    regex = pytest.importorskip("regex")
    assert regex_table[:0x80] == _class_array(_ranges(regex_table))[:0x80]   # the fixed ASCII classes are regex's
    classes = _ranges(regex_table)
    pats = {Split.Gpt2: regex.compile(GPT2_PATTERN), Split.Whitespace: regex.compile(WHITESPACE_PATTERN)}
    rng = random.Random(20261018)
    for k in range(20000):
        d = random_doc(rng, 6 if k % 2 else 24)
        s = d.decode("utf-8", errors="surrogateescape")
        for rule, pat in pats.items():
            pieces = [m.group() for m in pat.finditer(s)]
            assert "".join(pieces) == s, (d, rule)
            want = [0]
            for p in pieces:
                want.append(want[-1] + len(p.encode("utf-8", errors="surrogateescape")))
            assert _scan(d, rule, classes) == want, (d, rule)


def test_scan_hand_cases():
    cc = da.char_classes()

    def words(text, rule=Split.Gpt2):
        d = text if isinstance(text, bytes) else text.encode()
        b = _scan(d, rule, cc)
        return [d[s:e] for s, e in zip(b, b[1:])]

    assert words("it's we'll  a\n'd !'s 123abc") == [b"it", b"'s", b" we", b"'ll", b" ", b" a", b"\n", b"'d", b" !'", b"s", b" 123", b"abc"]
    assert words("a   ") == [b"a", b"   "]
    assert words("  'll") == [b" ", b" '", b"ll"]
    assert words("x's't") == [b"x", b"'s", b"'t"]
    assert words("'s") == [b"'s"] and words("'l") == [b"'", b"l"] and words("") == []
    assert words("a  b", Split.Whitespace) == [b"a", b"  ", b"b"]
    assert words("é漢 ٣²　x") == ["é漢".encode(), " ٣²".encode(), "　".encode(), b"x"]
    assert words(b"\xe6\xbc a\xa2") == [b"\xe6\xbc", b" a", b"\xa2"]   # a cut character is bytes of class O


# ----------------------------------------------------------------------------------------------------------- char_classes()
def test_char_classes_agree_with_unicodedata():
    cc = da.char_classes()
    assert cc is da.char_classes() and cc.dtype == np.uint32 and cc.shape[1] == 3 and not cc.flags.writeable
    assert "unidata_version" in da.char_classes.__doc__
    assert (cc[:, 0] <= cc[:, 1]).all() and (cc[1:, 0] > cc[:-1, 1]).all() and cc[0, 0] >= 0x80 and cc[-1, 1] <= 0x10FFFF
    table = _class_array(cc)
    white = {0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000}
    for cp in range(0x80, 0x110000):
        want = S if cp in white else {"L": L, "N": N}.get(unicodedata.category(chr(cp))[0], O)
        assert table[cp] == want, hex(cp)
    assert sum(1 for cp in range(0x110000) if table[cp] == S) == 25


def test_char_classes_differ_from_regex_only_on_unassigned_code_points(regex_table):
    table = _class_array(da.char_classes())
    diff = [cp for cp in range(0x110000) if table[cp] != regex_table[cp]]
    print("code points on which char_classes() and the regex module differ:", len(diff))
    assert all(unicodedata.category(chr(cp)) == "Cn" for cp in diff), [hex(cp) for cp in diff if unicodedata.category(chr(cp)) != "Cn"][:10]
    assert [cp for cp in range(0x110000) if regex_table[cp] == S] == [cp for cp in range(0x110000) if table[cp] == S]
    assert sum(1 for c in regex_table if c == S) == 25


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def _err():
    return _ffi.lib().daac_last_error().decode()


def _create(rule, rows):
    a = np.asarray(rows, dtype=np.uint32).reshape(-1, 3)
    h = C.c_void_p()
    st = _ffi.lib().daac_splitter_create(int(rule), a.ctypes.data if a.size else None, a.shape[0], C.byref(h))
    if st == 0:
        _ffi.lib().daac_splitter_free(h)
    else:
        assert not h.value
    return st


def test_split_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_splitter_create", "daac_splitter_free", "daac_split_batch", "daac_split", "daac_offsets_compose", "daac_spans_rebase"):
        assert hasattr(lib, name), name
    for name in ("Split", "Splitter", "char_classes", "split_batch", "offsets_compose"):
        assert hasattr(da, name), name
    assert (int(Split.Whitespace), int(Split.Gpt2)) == (0, 1)
    assert callable(da.DoubleArrayAhoCorasick.tokenize_bpe_docs)


def test_split_leaves_the_abi_version_at_6():
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_splitter_create_bad_arguments_answer_1():
    L_ = _ffi.lib()
    assert L_.daac_splitter_create(1, None, 0, None) == 1 and "null" in _err()
    for rule in (-1, 2, 255):
        assert _create(rule, []) == 1 and "rule" in _err(), rule
    h = C.c_void_p()
    assert L_.daac_splitter_create(1, None, 3, C.byref(h)) == 1 and "ranges is NULL" in _err()
    ok = [(0x80, 0x80, 3), (0xC0, 0xFF, 1), (0x660, 0x669, 2), (0x10FFFF, 0x10FFFF, 1)]
    assert _create(Split.Gpt2, ok) == 0 and _create(Split.Whitespace, ok) == 0 and _create(Split.Gpt2, []) == 0
    bad = {"last < first": [(0xC1, 0xC0, 1)],
           "U+0080": [(0x7F, 0x90, 1)],
           "U+10FFFF": [(0x10FFFF, 0x110000, 1)],
           "cls": [(0xC0, 0xFF, 0)],
           "sorted": [(0x100, 0x1FF, 1), (0xC0, 0xFF, 1)]}
    for word, rows in bad.items():
        assert _create(Split.Gpt2, rows) == 1 and word in _err(), (word, _err())
    assert _create(Split.Gpt2, [(0xC0, 0xFF, 4)]) == 1 and "cls" in _err()
    assert _create(Split.Gpt2, [(0xC0, 0xFF, 1), (0xFF, 0x1FF, 1)]) == 1 and "sorted" in _err()     # overlapping
    assert _create(Split.Gpt2, [(0xC0, 0xFF, 1), (0xC0, 0xFF, 2)]) == 1 and "sorted" in _err()      # twice
    # the wrapper raises the same status, and refuses what is no table of rows
    with pytest.raises(da.DaachorseError) as ei:
        da.Splitter(Split.Gpt2, [(0x100, 0x1FF, 1), (0xC0, 0xFF, 1)])
    assert ei.value.code == 1 and "sorted" in str(ei.value)
    for rows in ([1, 2, 3], [(0xC0, 0xFF)], [(0xC0, -1, 1)], [(0.5, 1.5, 1.0)]):
        with pytest.raises(da.DaachorseError) as ei:
            da.Splitter(Split.Gpt2, rows)
        assert ei.value.code == 1, rows
    with pytest.raises(da.DaachorseError) as ei:
        da.Splitter(7)
    assert ei.value.code == 1


class _Call:
    """the raw arguments of daac_split_batch on a host batch; the out-pointers named in `null` go as NULL"""

    def __init__(self, sp, hay=b"ab cd", offsets=(0, 2, 5)):
        self.sp = sp
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.wo, self.dw, self.nw = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self.null = set()

    def run(self):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        return _ffi.lib().daac_split_batch(self.sp, ptr(self.hay), ptr(self.offsets), self.n, 0, None, ref("wo", self.wo), ref("dw", self.dw), ref("nw", self.nw))


def test_split_bad_arguments_answer_1_without_a_device():
    sp = da.Splitter(Split.Gpt2)
    L_ = _ffi.lib()
    for name in ("wo", "dw", "nw"):
        c = _Call(sp._h)
        c.null.add(name)
        assert c.run() == 1 and "null" in _err(), name
    assert _Call(None).run() == 1 and "null" in _err()
    # the batch calls' own offset rules
    assert _Call(sp._h, offsets=(0, 3, 2)).run() == 1 and "document 1" in _err()
    c = _Call(sp._h)
    c.offsets = None   # NULL offsets with n > 0
    assert c.run() == 1 and "offsets" in _err()
    c = _Call(sp._h)
    c.hay = None
    assert c.run() == 1 and "hay" in _err()
    # n = 0 passes every check, NULL hay and offsets included: what is left is the device (0 with one, 7 without)
    c = _Call(sp._h, offsets=None)
    c.hay = None
    st = c.run()
    assert st in (0, 7), (st, _err())
    if st == 0:
        assert c.nw.value == 0
        for p in (c.wo, c.dw):
            out = np.ones(1, dtype=np.uint64)
            assert L_.daac_device_to_host(out.ctypes.data, p, 8) == 0 and out[0] == 0
            L_.daac_device_free(p)
    c = _Call(sp._h, offsets=None)
    c.null.add("dw")
    assert c.run() == 1
    # the single haystack and the gather
    wo, nw = C.c_void_p(), C.c_uint64()
    assert L_.daac_split(None, b"ab", 2, 0, None, C.byref(wo), C.byref(nw)) == 1 and "null" in _err()
    assert L_.daac_split(sp._h, b"ab", 2, 0, None, None, C.byref(nw)) == 1 and "null" in _err()
    assert L_.daac_split(sp._h, b"ab", 2, 0, None, C.byref(wo), None) == 1 and "null" in _err()
    assert L_.daac_split(sp._h, None, 2, 0, None, C.byref(wo), C.byref(nw)) == 1 and "hay" in _err()
    assert L_.daac_offsets_compose(None, None, 0, None, None) == 1 and "null" in _err()
    assert L_.daac_offsets_compose(None, None, 3, None, C.byref(wo)) == 1 and "null" in _err()
    sp.free()
    sp.free()   # twice is fine
    with pytest.raises(da.DaachorseError) as ei:
        sp.split_batch([b"ab"])
    assert ei.value.code == 1 and "freed" in str(ei.value)


def test_split_position_functions_on_the_host_under_sanitizers(tmp_path):
    """split_reach and split_start of split_kernels.hip as plain C++, at every position of 2 x 3 000 random batches against a sequential
    scanner: both rules, documents of 0 .. 40 bytes in buffers of exactly their size, batches with offsets[0] > 0"""
    exe = str(tmp_path / "split_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "split_check.cpp")])
    for seed in (1, 2):
        r = subprocess.run([exe, "3000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 3000 rounds") and r.stderr == "", (r.stdout, r.stderr)
