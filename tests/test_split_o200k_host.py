"""Split.O200k on the host side: a pure-Python sequential scanner `scan_o200k` for tiktoken's o200k_base pattern in the style of
test_split_rules_host.scan_rule (the GPU tests' reference), that scanner against the stored fixture tests/golden/split_o200k_cases.json
(word boundaries from the `regex` module and from `tokenizers`), against both libraries on every short string over a small alphabet and on
fresh random documents where they are installed, malformed UTF-8 through the scanner alone, what the C ABI answers before a device, and
the kernel file's per-position functions run on the CPU under ASan and UBSan (tests/native/split_o200k_check.cpp, a stand-alone
program).  No GPU."""
import ctypes as C
import itertools
import json
import os
import random
import subprocess

import numpy as np
import pytest

import daachorse_amd as da
from daachorse_amd import Split, _ffi
from test_split_host import L, N, O, S, _units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "split_o200k_cases.json")

O200K_PATTERN = (r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
                 r"|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
                 r"|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+")
UP, LOW, MARK = 4, 5, 6   # the classes Split.O200k adds; L (1) is then a caseless letter

SMALL = ["a", "A", "\u4e2d", "\u0301", "0", " ", "\n", "\t", "'", "!", "/", "s", "S"]
WIDE = SMALL + ["\u00e9", "\u00c9", "\u01c5", "\u02b0", "\u0663", "\u017f", "\u2028", "\u00a0", "\r", "t", "T", "l", "L", "e", "v", "r", "m", "d", "D"]
STRAY = [bytes.fromhex(h) for h in ("80", "BF", "C3", "C5", "CC", "E4B8", "EDA080", "F4908080", "C0AF", "E080AF", "F09F", "FF")]


# ------------------------------------------------------------------------------------------------------------- the definition
def _units_o200k(d, classes):
    """_units with the fixed ASCII classes of Split.O200k: A-Z upper, a-z lower"""
    at, cls, byte = _units(d, classes)
    cls = [UP if 0x41 <= b <= 0x5A else LOW if 0x61 <= b <= 0x7A else c for c, b in zip(cls, byte)]
    return at, cls, byte


_UPPER_SIDE = (UP, L, MARK)    # [\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]
_LOWER_SIDE = (LOW, L, MARK)   # [\p{Ll}\p{Lm}\p{Lo}\p{M}]
_LETTER = (UP, LOW, L)         # \p{L}


def scan_o200k(doc, classes):
    """The words of one document under Split.O200k as their boundaries [0, .., len(doc)] ([0] for an empty document): the sequential
    scanner over the document's units.  At each position it tries the alternatives of the pattern in order, each greedy and giving back
    what it took as a backtracking matcher does."""
    d = bytes(doc)
    at, cls, byte = _units_o200k(d, classes)
    n = len(at)
    bounds = [0]

    def fold(i):
        """the letter unit i folds to: an ASCII letter in either case, U+017F where it is a letter"""
        if i >= n:
            return None
        if byte[i] >= 0:
            return chr(byte[i]).lower() if chr(byte[i]).isalpha() else None
        end = at[i + 1] if i + 1 < n else len(d)
        return "s" if d[at[i]:end] == b"\xc5\xbf" and cls[i] in _LETTER else None

    def is_nl(i):
        return byte[i] in (0x0A, 0x0D)

    def run(i, pred, stop=None):
        stop = n if stop is None else min(stop, n)
        while i < stop and pred(i):
            i += 1
        return i

    def suffix(e):
        """(?i:'s|'t|'re|'ve|'m|'ll|'d)? at unit e"""
        if e < n and byte[e] == 0x27:
            a, b = fold(e + 1), fold(e + 2)
            if a in ("s", "t", "m", "d"):
                return e + 2
            if a is not None and b is not None and byte[e + 1] >= 0 and a + b in ("re", "ve", "ll"):
                return e + 3
        return e

    def word(i, first):
        """alternative 1 or 2 at unit i: the optional prefix, taken first and then given back"""
        prefix = cls[i] not in _LETTER and cls[i] != N and not is_nl(i)
        for start in ((i + 1, i) if prefix else (i,)):
            top = run(start, lambda k: cls[k] in _UPPER_SIDE)
            if first:    # U* Lw+: the upper side gives back one unit at a time
                for u_end in range(top, start - 1, -1):
                    to = run(u_end, lambda k: cls[k] in _LOWER_SIDE)
                    if to > u_end:
                        return suffix(to)
            elif top > start:   # U+ Lw*
                return suffix(run(top, lambda k: cls[k] in _LOWER_SIDE))
        return i

    i = 0
    while i < n:
        e = word(i, True)
        if e == i:
            e = word(i, False)
        if e == i and cls[i] == N:                                     # \p{N}{1,3}
            e = run(i, lambda k: cls[k] == N, i + 3)
        if e == i:                                                     #  ?[^\s\p{L}\p{N}]+[\r\n/]*
            for first in ((i + 1, i) if byte[i] == 0x20 else (i,)):
                to = run(first, lambda k: cls[k] in (O, MARK))
                if to > first:
                    e = run(to, lambda k: is_nl(k) or byte[k] == 0x2F)
                    break
        if e == i:                                                     # the whitespace alternatives
            assert cls[i] == S, (d, i)
            full = run(i, lambda k: cls[k] == S)
            last_nl = max((k for k in range(i, full) if is_nl(k)), default=-1)
            if last_nl >= 0:                                           # \s*[\r\n]+: as far as the run's last newline
                e = last_nl + 1
            elif full == n or full - 1 == i:                           # \s+(?!\S) keeps the whole run at the end; \s+ takes one unit
                e = full
            else:                                                      # \s+(?!\S): all but the run's last unit
                e = full - 1
        assert e > i, (d, i)
        i = e
        bounds.append(at[i] if i < n else len(d))
    return bounds


def scan_o200k_batch(docs, classes, base=0):
    """-> (word_offsets, doc_words) of a batch whose first document begins at `base`, as daac_split_batch defines them"""
    wo, dw, pos = [], [0], base
    for d in docs:
        b = scan_o200k(d, classes)
        wo += [pos + x for x in b[:-1]]
        dw.append(len(wo))
        pos += len(d)
    return np.array(wo + [pos], dtype=np.uint64), np.array(dw, dtype=np.uint64)


def byte_bounds(pieces):
    out = [0]
    for p in pieces:
        out.append(out[-1] + len(p.encode("utf-8")))
    return out


def random_text(rng, max_chars, chars=WIDE):
    return "".join(rng.choice(chars) for _ in range(rng.randrange(max_chars + 1)))


def random_bytes_doc(rng, max_pieces):
    """as random_text, with malformed UTF-8 among the pieces, cut anywhere"""
    pieces = [rng.choice(STRAY) if rng.random() < 0.15 else rng.choice(WIDE).encode() for _ in range(rng.randrange(max_pieces + 1))]
    d = b"".join(pieces)
    return d[:rng.randrange(len(d) + 1)] if rng.random() < 0.3 else d


@pytest.fixture(scope="module")
def fixture_cases():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


# ------------------------------------------------------------------------------------------------- the scanner and the fixture
def test_scanner_equals_the_fixture_on_every_document(fixture_cases):
    cc = da.o200k_char_classes()
    assert len(fixture_cases) >= 300
    for case in fixture_cases:
        assert scan_o200k(case["text"].encode("utf-8"), cc) == case["o200k"], case["text"]
        assert case["o200k"] == case["o200k_tokenizers"], case["text"]


def test_scanner_hand_cases():
    cc = da.o200k_char_classes()

    def words(text, classes=cc):
        d = text if isinstance(text, bytes) else text.encode()
        b = scan_o200k(d, classes)
        return "|".join(d[s:e].decode("utf-8", "replace") for s, e in zip(b, b[1:]))

    m = "\u0301"
    for want in ("HTMLParser", "XMLHttp|Request", "hello|World", "a中|B", "A中Bc", "AB中|CD", "AB中CDe", "AB中CD中|EF| x",
                 f"!{m}abc", f"!!{m}|abc", f" !{m}|abc", f"!{m * 5}abc", f"!!{m * 5}|abc", f" !{m * 5}|abc", f"{m}|A", f"a{m}|B", f"A{m}|B| c",
                 "don't", " DON'T", " don'T", " he'll", " x'ſ", "a's|'t", "A's|B", "ab's|Cd", "ab|C's", "1|'s", "x|''|s", " '|s's",
                 "!\n/|!", "!/!", "a|/\n/|b", "123|456|78", "a|  \n\n|  ", "a|   ", "a| | b", "\tab|-cd", "\n|ab", "ǅa|ǅ", ""):
        assert words(want.replace("|", "")) == want, want
    assert words(b"a\xffb \xc5") == "a|�b| �"   # a stray byte is a unit of class O
    assert words("éÉ中", da.char_classes()) == "éÉ中" and words("éÉ中") == "é|É中"   # without case classes every letter is caseless


def _pieces_of(pat, s):
    pieces = [m.group() for m in pat.finditer(s)]
    assert "".join(pieces) == s, s
    return pieces


def test_scanner_equals_both_libraries_on_every_short_string():
    """every string of up to 4 symbols over the 13-symbol alphabet (30 940 strings) and 20 000 random ones of up to 24 symbols: all
    strings of up to 5 take longer than 20 s through the three matchers here, the stand-alone program runs the device functions over
    all strings of up to 6"""
    regex = pytest.importorskip("regex")
    tokenizers = pytest.importorskip("tokenizers")
    cc = da.o200k_char_classes()
    pat = regex.compile(O200K_PATTERN)
    pre = tokenizers.pre_tokenizers.Split(tokenizers.Regex(O200K_PATTERN), "isolated")
    rng = random.Random(20261022)
    strings = ("".join(t) for k in range(1, 5) for t in itertools.product(SMALL, repeat=k))
    for s in itertools.chain(strings, (random_text(rng, 24, SMALL) for _ in range(20000))):
        want = byte_bounds(_pieces_of(pat, s))
        assert scan_o200k(s.encode("utf-8"), cc) == want, s
        assert byte_bounds([p for p, _ in pre.pre_tokenize_str(s)]) == want, s


def test_scanner_equals_both_libraries_on_random_documents():
    regex = pytest.importorskip("regex")
    tokenizers = pytest.importorskip("tokenizers")
    cc = da.o200k_char_classes()
    pat = regex.compile(O200K_PATTERN)
    pre = tokenizers.pre_tokenizers.Split(tokenizers.Regex(O200K_PATTERN), "isolated")
    rng = random.Random(20261023)
    for k in range(20000):
        s = random_text(rng, 8 if k % 2 else 24)
        want = byte_bounds(_pieces_of(pat, s))
        assert scan_o200k(s.encode("utf-8"), cc) == want, s
        assert byte_bounds([p for p, _ in pre.pre_tokenize_str(s)]) == want, s


def test_o200k_char_classes_agree_with_unicodedata():
    import unicodedata
    cc = da.o200k_char_classes()
    assert cc is da.o200k_char_classes() and not cc.flags.writeable and cc.dtype == np.uint32 and cc.shape[1] == 3
    assert cc[0, 0] >= 0x80 and (cc[1:, 0] > cc[:-1, 1]).all() and (cc[:, 2] >= 1).all() and (cc[:, 2] <= 6).all()
    a = np.zeros(0x110000, dtype=np.uint8)
    for first, last, cls in cc.tolist():
        a[first:last + 1] = cls
    plain = np.zeros(0x110000, dtype=np.uint8)
    for first, last, cls in da.char_classes().tolist():
        plain[first:last + 1] = cls
    assert ((a == S) == (plain == S)).all() and ((a == N) == (plain == N)).all()
    assert (np.isin(a, (L, UP, LOW)) == (plain == L)).all()
    for cp, want in ((0xE9, LOW), (0xC9, UP), (0x1C5, UP), (0x2B0, L), (0x4E2D, L), (0x301, MARK), (0x663, N), (0x17F, LOW), (0xA0, S), (0x2014, O)):
        assert a[cp] == want, hex(cp)
    for cp in range(0x80, 0x3000):
        cat = unicodedata.category(chr(cp))
        assert (a[cp] == MARK) == (cat[0] == "M") and (a[cp] == UP) == (cat in ("Lu", "Lt")), hex(cp)


def test_malformed_utf8_is_units_of_class_o():
    """every stray byte splits as a one-byte unit of class O does: the boundaries are those of the document with 0x01 in its place"""
    cc = da.o200k_char_classes()
    rng = random.Random(20261024)
    seen = 0
    for _ in range(5000):
        d = random_bytes_doc(rng, 16)
        at, cls, byte = _units_o200k(d, cc)
        twin = bytearray(d)
        for k, a in enumerate(at):
            if byte[k] < 0 and (at[k + 1] if k + 1 < len(at) else len(d)) - a == 1:   # a byte from 0x80 on that is a unit of its own
                assert cls[k] == O
                twin[a] = 0x01
                seen += 1
        b = scan_o200k(d, cc)
        assert b == scan_o200k(bytes(twin), cc), d
        assert b[0] == 0 and b[-1] == len(d) and all(x < y for x, y in zip(b, b[1:])) and set(b[:-1]) <= set(at), d
    assert seen > 3000


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def _create(rule, rows=()):
    h = C.c_void_p()
    a = np.ascontiguousarray(np.array(rows, dtype=np.uint32).reshape(-1, 3))
    st = _ffi.lib().daac_splitter_create(int(rule), a.ctypes.data if a.size else None, a.shape[0], C.byref(h))
    if st == 0:
        _ffi.lib().daac_splitter_free(h)
    return st


def test_rule_8_creates_with_classes_1_to_6():
    assert int(Split.O200k) == 8
    assert _create(8) == 0
    assert _create(8, [(0x100 + 16 * c, 0x100 + 16 * c + 3, c) for c in range(1, 7)]) == 0
    for bad in (0, 7, 8, 255):
        assert _create(8, [(0x100, 0x103, bad)]) == 1 and "cls" in _ffi.lib().daac_last_error().decode(), bad
    for rule in (-1, 2, 5, 7, 9, 255):
        assert _create(rule) == 1 and "rule" in _ffi.lib().daac_last_error().decode(), rule
    for rule in (0, 1, 3, 4, 6):   # every other rule goes on refusing the case classes
        assert _create(rule, [(0x100, 0x103, 3)]) == 0
        for bad in (4, 5, 6):
            assert _create(rule, [(0x100, 0x103, bad)]) == 1 and "cls" in _ffi.lib().daac_last_error().decode(), (rule, bad)
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_python_splitters_of_the_rule():
    sp = da.Splitter(Split.O200k)
    assert sp.rule == 8
    sp.free()
    sp = da.Splitter(Split.O200k, da.char_classes())   # every non-ASCII letter caseless
    assert sp.rule == 8
    sp.free()
    with pytest.raises(da.DaachorseError) as ei:
        da.Splitter(Split.Gpt2, da.o200k_char_classes())
    assert ei.value.code == 1 and "cls" in str(ei.value)


def test_o200k_functions_on_the_host_under_sanitizers(tmp_path):
    """the class and map functions, the wave and tile compositions, the carry resolution and o200k_start of split_kernels.hip as plain
    C++, at every position against a sequential scanner in the same program: every string of up to 6 symbols over the 13-symbol
    alphabet, then random batches with tiles of 64, 128 and 1024 positions, runs several tiles long, documents in buffers of exactly their
    size, offsets[0] > 0, empty documents, malformed UTF-8, and the table with and without U+017F as a letter"""
    exe = str(tmp_path / "split_o200k_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "split_o200k_check.cpp")])
    r = subprocess.run([exe, "1200", "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK 1200 rounds") and r.stderr == "", (r.stdout, r.stderr)
