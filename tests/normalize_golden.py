"""The normalizer fixture of tests/golden/ (written by make_normalize_golden.py from `tokenizers`) as the host tests and the GPU tests read
it, and the definitions in pure Python that the generator checked against `tokenizers` on every document: BertNormalizer as a
substitution per code point, the sequential scanner of a document under such a substitution or under a Normalizer's rules, and the way
back from spans over the normalized text to spans over the input.  A plain helper: no test lives here, and nothing here reads
`tokenizers` or the library."""
import bisect
import functools
import json
import os
import unicodedata

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DELETE, REPLACE, PAD, HANGUL = 1, 2, 3, 4
# the option sets of the fixture: (clean_text, handle_chinese_chars, strip_accents, lowercase)
OPTIONS = {"default": (True, True, True, True), "keep_accents": (True, True, False, True), "clean_only": (True, False, False, False)}
CJK_BLOCKS = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B920, 0x2CEAF), (0xF900, 0xFAFF),
              (0x2F800, 0x2FA1F))
# Rust's char::is_whitespace: the 25 White_Space code points
WHITESPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
# the characters outside Mn with a non-zero combining class: what NFD's canonical reordering can still move once Mn is dropped
REORDERED = frozenset([0x1B44, 0x1BAA, 0x1BF2, 0x1BF3, 0x302E, 0x302F, 0xA953, 0xA9C0, 0x111C0, 0x11235, 0x1134D, 0x116B6, 0x1193D, 0x16FF0, 0x16FF1,
                       0x1D165, 0x1D166, *range(0x1D16D, 0x1D173)])


@functools.lru_cache(maxsize=None)
def load():
    with open(os.path.join(GOLDEN, "normalize_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def docs():
    return [d.encode() for d in load()["docs"]]


def expected(name):
    """tokenizers' normalize_str of every document under the option set `name`, as bytes"""
    return [d.encode() for d in load()["normalized"][name]]


def tokens():
    """-> (ids, byte spans) per document: the full Tokenizer's under the default options, spans relative to the raw document"""
    import wordpiece_golden as wg
    c = load()
    return c["ids"], [[tuple(x) for x in p["raw"]] if isinstance(p, dict) else wg.unpack_spans(p) for p in c["tok_spans"]]


# ---------------------------------------------------------------------------------------------------------- the definitions
def bert_image(cp, clean_text=True, handle_chinese_chars=True, strip_accents=True, lowercase=True):
    """BertNormalizer on one character: the four steps in order -> str"""
    c = chr(cp)
    if clean_text:
        if cp == 0 or cp == 0xFFFD or (unicodedata.category(c) in ("Cc", "Cf", "Co") and c not in "\t\n\r"):
            return ""
        if cp in WHITESPACE:
            c = " "
    s = c
    if handle_chinese_chars and any(lo <= cp <= hi for lo, hi in CJK_BLOCKS):
        s = " " + c + " "
    if strip_accents:
        s = "".join(ch for ch in unicodedata.normalize("NFD", s) if unicodedata.category(ch) != "Mn")
    if lowercase:
        s = "".join(ch.lower() for ch in s)
    return s


def units(d):
    """a document's units -> [(at, length, code point or None)]: a well-formed UTF-8 sequence (Unicode Table 3-7) inside the document is
    one unit, every other byte a unit of its own with no code point"""
    out, i, n = [], 0, len(d)
    while i < n:
        b0 = d[i]
        k, cp = 1, b0 if b0 < 0x80 else None
        if b0 >= 0x80:
            need = 2 if 0xC2 <= b0 <= 0xDF else 3 if 0xE0 <= b0 <= 0xEF else 4 if 0xF0 <= b0 <= 0xF4 else 0
            try:
                ch = bytes(d[i:i + need]).decode("utf-8") if need and i + need <= n else ""   # (strict: overlong forms and surrogates raise)
            except UnicodeDecodeError:
                ch = ""
            if len(ch) == 1:
                k, cp = need, ord(ch)
        out.append((i, k, cp))
        i += k
    return out


def scan(doc, image):
    """The sequential scanner: `image(cp, unit bytes)` -> bytes.  -> (the normalized document, per output byte the offset of its unit)"""
    d = bytes(doc)
    out, src = bytearray(), []
    for at, k, cp in units(d):
        img = d[at:at + k] if cp is None else image(cp, d[at:at + k])
        out += img
        src += [at] * len(img)
    return bytes(out), src


def bert_scan(doc, options):
    cache = {}

    def image(cp, raw):
        if cp not in cache:
            cache[cp] = bert_image(cp, *options).encode()
        return cache[cp]
    return scan(doc, image)


def hangul_jamo(cp):
    s = cp - 0xAC00
    return "".join(chr(x) for x in ([0x1100 + s // 588, 0x1161 + s % 588 // 28] + ([0x11A7 + s % 28] if s % 28 else []))).encode()


def rules_image(rules, pool):
    """a Normalizer's rules (rows {first, last, kind, off, len}) and pool -> the `image` of scan()"""
    rows = [tuple(int(x) for x in r) for r in rules]
    firsts = [r[0] for r in rows]

    def image(cp, raw):
        i = bisect.bisect_right(firsts, cp) - 1
        if i < 0 or cp > rows[i][1]:
            return raw
        _, _, kind, off, ln = rows[i]
        return {DELETE: b"", REPLACE: pool[off:off + ln], PAD: b" " + raw + b" ", HANGUL: hangul_jamo(cp) if kind == HANGUL else b""}[kind]
    return image


def scan_batch(docs_, image):
    """-> (out, out_offsets, src) of a batch as daac_normalize_batch defines them"""
    out, offs, src = bytearray(), [0], []
    for d in docs_:
        o, s = scan(d, image)
        out += o
        src += s
        offs.append(len(out))
    return bytes(out), offs, src


def spans_to_source(spans, src, doc):
    """{start, end} over the normalized document -> over the input document: start -> src[start], end -> src[end - 1] + the length of the
    input unit there, an empty span at p -> src[p] twice (src at the output's length: the input's length)"""
    d = bytes(doc)
    length = {at: k for at, k, _ in units(d)}
    out = []
    for s, e in spans:
        if s == e:
            v = src[s] if s < len(src) else len(d)
            out.append((v, v))
        else:
            out.append((src[s], src[e - 1] + length[src[e - 1]]))
    return out
