"""Split.Cl100k and Split.Llama3 on the host side: a pure-Python sequential scanner `scan_rule` for the two patterns in the style of
test_split_host._scan (the GPU tests' reference), that scanner against the stored fixture tests/golden/split_rules_cases.json (word
boundaries from the `regex` module and, for Llama-3, from `tokenizers`), against both libraries on fresh random documents where they are
installed, malformed UTF-8 through the scanner alone, what the C ABI answers before a device, and the kernel file's scan and decision
functions run on the CPU under ASan and UBSan (tests/native/split_rules_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "split_rules_cases.json")

LLAMA3_PATTERN = r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"
CL100K_PATTERN = r"'(?i:[sdmt]|ll|ve|re)|[^\r\n\p{L}\p{N}]?+\p{L}++|\p{N}{1,3}+| ?[^\s\p{L}\p{N}]++[\r\n]*+|\s++$|\s*[\r\n]|\s+(?!\S)|\s+"
PATTERNS = {Split.Cl100k: CL100K_PATTERN, Split.Llama3: LLAMA3_PATTERN}
RULES = (Split.Cl100k, Split.Llama3)

# what random documents are drawn from: the contraction letters in both cases, digits, spaces, newlines, other whitespace of one, two and
# three bytes, ', punctuation, a letter of two and of three bytes, U+017F (folds to s), a digit of two bytes and U+212A (folds to k)
CHARS = list("sStTrReEvVmMlLdD" "0159" "    " "\n\n\r\t\x0b\u0085  " "'''" "!.-" "é中ſ٣K")
STRAY = [bytes.fromhex(h) for h in ("80", "BF", "C3", "C5", "E4B8", "EDA080", "F4908080", "C0AF", "E080AF", "F09F", "FF")]
_LONG_S = frozenset(b"\xc5\xbf")


def random_text(rng, max_chars):
    return "".join(rng.choice(CHARS) for _ in range(rng.randrange(max_chars + 1)))


def random_bytes_doc(rng, max_pieces):
    """as random_text, with malformed UTF-8 among the pieces, cut anywhere"""
    pieces = [rng.choice(STRAY) if rng.random() < 0.15 else rng.choice(CHARS).encode() for _ in range(rng.randrange(max_pieces + 1))]
    d = b"".join(pieces)
    return d[:rng.randrange(len(d) + 1)] if rng.random() < 0.3 else d


# ------------------------------------------------------------------------------------------------------------- the definition
def scan_rule(doc, rule, classes):
    """The words of one document under Split.Cl100k or Split.Llama3 as their boundaries [0, .., len(doc)] ([0] for an empty document):
    the sequential scanner over the document's units.  At each position it tries the alternatives of the pattern in order."""
    d = bytes(doc)
    at, cls, byte = _units(d, classes)
    n = len(at)
    bounds = [0]

    def fold(i):
        """the letter unit i folds to: an ASCII letter in either case, U+017F where it is a letter"""
        if i >= n:
            return None
        if byte[i] >= 0:
            return chr(byte[i]).lower() if chr(byte[i]).isalpha() else None
        end = at[i + 1] if i + 1 < n else len(d)
        return "s" if d[at[i]:end] == b"\xc5\xbf" and cls[i] == L else None

    def is_nl(i):
        return byte[i] in (0x0A, 0x0D)

    def run(i, pred):
        while i < n and pred(i):
            i += 1
        return i

    i = 0
    while i < n:
        e = i
        if byte[i] == 0x27:                                            # (?i:'s|'t|'re|'ve|'m|'ll|'d)
            a, b = fold(i + 1), fold(i + 2)
            if a in ("s", "t", "m", "d"):
                e = i + 2
            elif a is not None and b is not None and a + b in ("re", "ve", "ll") and byte[i + 1] >= 0:
                e = i + 3
        if e == i:                                                     # [^\r\n\p{L}\p{N}]?\p{L}+
            first = i if cls[i] == L else i + 1 if cls[i] != N and not is_nl(i) else n
            to = run(first, lambda k: cls[k] == L)
            if to > first:
                e = to
        if e == i and cls[i] == N:                                     # \p{N}{1,3}
            e = min(run(i, lambda k: cls[k] == N), i + 3)
        if e == i:                                                     #  ?[^\s\p{L}\p{N}]+[\r\n]*
            for first in ((i + 1, i) if byte[i] == 0x20 else (i,)):
                to = run(first, lambda k: cls[k] == O)
                if to > first:
                    e = run(to, is_nl)
                    break
        if e == i:                                                     # the whitespace alternatives
            assert cls[i] == S, (d, i)
            full = run(i, lambda k: cls[k] == S)
            last_nl = max((k for k in range(i, full) if is_nl(k)), default=-1)
            if rule == Split.Cl100k and full == n:                     # \s++$
                e = n
            elif last_nl >= 0:                                         # \s*[\r\n]+ and \s*[\r\n]: as far as the run's last newline
                e = last_nl + 1
            elif full == n or full - 1 == i:                           # \s+(?!\S) keeps the whole run at the end; \s+ takes one unit
                e = full
            else:                                                      # \s+(?!\S): all but the run's last unit
                e = full - 1
        assert e > i, (d, i)
        i = e
        bounds.append(at[i] if i < n else len(d))
    return bounds


def scan_rule_batch(docs, rule, classes, base=0):
    """-> (word_offsets, doc_words) of a batch whose first document begins at `base`, as daac_split_batch defines them"""
    wo, dw, pos = [], [0], base
    for d in docs:
        b = scan_rule(d, rule, classes)
        wo += [pos + x for x in b[:-1]]
        dw.append(len(wo))
        pos += len(d)
    return np.array(wo + [pos], dtype=np.uint64), np.array(dw, dtype=np.uint64)


def byte_bounds(pieces):
    out = [0]
    for p in pieces:
        out.append(out[-1] + len(p.encode("utf-8")))
    return out


@pytest.fixture(scope="module")
def fixture_cases():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


# ------------------------------------------------------------------------------------------------- the scanner and the fixture
def test_scanner_equals_the_fixture_on_every_document(fixture_cases):
    cc = da.char_classes()
    assert len(fixture_cases) >= 300
    differ = 0
    for case in fixture_cases:
        d = case["text"].encode("utf-8")
        assert scan_rule(d, Split.Cl100k, cc) == case["cl100k"], case["text"]
        assert scan_rule(d, Split.Llama3, cc) == case["llama3"], case["text"]
        assert case["llama3"] == case["llama3_tokenizers"], case["text"]
        differ += case["cl100k"] != case["llama3"]
    assert differ >= 10   # the fixture holds whitespace runs that reach the end


def test_scanner_hand_cases():
    cc = da.char_classes()

    def words(text, rule=Split.Llama3):
        d = text if isinstance(text, bytes) else text.encode()
        b = scan_rule(d, rule, cc)
        return [d[s:e].decode("utf-8", "replace") for s, e in zip(b, b[1:])]

    assert words("it's WE'LL  a\n'D !'s 123abc") == ["it", "'s", " WE", "'LL", " ", " a", "\n", "'D", " !'", "s", " ", "123", "abc"]
    assert words("1281") == ["128", "1"] and words("12345678") == ["123", "456", "78"] and words("1٣23") == ["1٣2", "3"]
    assert words("x'ſ y'K") == ["x", "'ſ", " y", "'K"] and words("x'K") == ["x", "'K"]
    assert words("a!\n\n b") == ["a", "!\n\n", " b"] and words("a\n\n b") == ["a", "\n\n", " b"]
    assert words("a \n  b") == ["a", " \n", " ", " b"] and words("a  \n\n  ") == ["a", "  \n\n", "  "]
    assert words("a  \n\n  ", Split.Cl100k) == ["a", "  \n\n  "]
    assert words("a   ") == ["a", "   "] and words("a   ", Split.Cl100k) == ["a", "   "]
    assert words("\tab-cd") == ["\tab", "-cd"] and words("\nab") == ["\n", "ab"] and words("") == []
    assert words(b"a\xffb \xc5") == ["a", "�b", " �"]   # a stray byte is a unit of class O


def test_scanner_equals_the_regex_module_on_random_documents():
    regex = pytest.importorskip("regex")
    cc = da.char_classes()
    pats = {rule: regex.compile(p) for rule, p in PATTERNS.items()}
    rng = random.Random(20261019)
    for k in range(20000):
        s = random_text(rng, 8 if k % 2 else 24)
        for rule, pat in pats.items():
            pieces = [m.group() for m in pat.finditer(s)]
            assert "".join(pieces) == s, (s, rule)
            assert scan_rule(s.encode("utf-8"), rule, cc) == byte_bounds(pieces), (s, rule)


def test_llama3_scanner_equals_tokenizers_on_random_documents():
    tokenizers = pytest.importorskip("tokenizers")
    cc = da.char_classes()
    pre = tokenizers.pre_tokenizers.Split(tokenizers.Regex(LLAMA3_PATTERN), "isolated")
    rng = random.Random(20261020)
    for k in range(5000):
        s = random_text(rng, 8 if k % 2 else 24)
        pieces = [p for p, _ in pre.pre_tokenize_str(s)]
        assert "".join(pieces) == s, s
        assert scan_rule(s.encode("utf-8"), Split.Llama3, cc) == byte_bounds(pieces), s


def test_malformed_utf8_is_units_of_class_o():
    """every stray byte splits as a one-byte unit of class O does: the boundaries are those of the document with 0x01 in its place"""
    cc = da.char_classes()
    rng = random.Random(20261021)
    seen = 0
    for _ in range(5000):
        d = random_bytes_doc(rng, 16)
        at, cls, byte = _units(d, cc)
        twin = bytearray(d)
        for k, a in enumerate(at):
            if byte[k] < 0 and (at[k + 1] if k + 1 < len(at) else len(d)) - a == 1:   # a byte from 0x80 on that is a unit of its own
                assert cls[k] == O
                twin[a] = 0x01
                seen += 1
        for rule in RULES:
            b = scan_rule(d, rule, cc)
            assert b == scan_rule(bytes(twin), rule, cc), (d, rule)
            assert b[0] == 0 and b[-1] == len(d) and all(x < y for x, y in zip(b, b[1:])) and set(b[:-1]) <= set(at), (d, rule)
    assert seen > 3000


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def _create(rule):
    h = C.c_void_p()
    st = _ffi.lib().daac_splitter_create(int(rule), None, 0, C.byref(h))
    if st == 0:
        _ffi.lib().daac_splitter_free(h)
    return st


def test_the_two_rules_create_and_2_stays_refused():
    assert (int(Split.Cl100k), int(Split.Llama3)) == (3, 4)
    assert (int(Split.Whitespace), int(Split.Gpt2)) == (0, 1)
    assert _create(3) == 0 and _create(4) == 0
    for rule in (-1, 2, 5, 7, 255):
        assert _create(rule) == 1 and "rule" in _ffi.lib().daac_last_error().decode(), rule
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION
    for rule in RULES:
        sp = da.Splitter(rule)
        assert sp.rule == int(rule)
        sp.free()
    with pytest.raises(da.DaachorseError) as ei:
        da.Splitter(2)
    assert ei.value.code == 1


def test_scan_functions_on_the_host_under_sanitizers(tmp_path):
    """the predicate bits, the word and tile functions, the carry resolution and split_start_scanned of split_kernels.hip as plain C++,
    at every position of random batches against a sequential scanner in the same program: both rules, tiles of 64, 128 and 1024
    positions, long runs across tiles, documents in buffers of exactly their size, batches with offsets[0] > 0"""
    exe = str(tmp_path / "split_rules_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "split_rules_check.cpp")])
    for seed in (1, 2):
        r = subprocess.run([exe, "1500", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 1500 rounds") and r.stderr == "", (r.stdout, r.stderr)
