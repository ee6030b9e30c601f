"""Small dictionaries for the count + checksum GRAM kernels (gram_kernels.hip, gram2_kernels.hip, gram2w_kernels.hip), their texts and
what the CPU oracle finds in them — shared by tests/test_gram_exact_host.py, tests/test_gpu_gram_exact.py and the zero-hash cases of
tests/test_gpu_dictionary_limits.py (a plain module, imported by name; everything is generated from seeds).

The dictionaries are small on purpose: every table set fits the LDS with the rank directory forced either way, every launch shape fits,
and the oracle answers at once.

  k3s   ~400 words over 8 letters: lengths 1, 2 and 3, own patterns at depth 4 and 5, words that are prefixes of longer words, and eight
        single paths of 9 .. 16 edges below depth 6 (tail records, and a tail record below ordinary records)          K = 3, short patterns
  k3n   k3s without the words shorter than 4 bytes                                                                     K = 3, none
  k2s   k3s with the tables squeezed to K = 2 (option gram_lds_budget = K2_BUDGET, read at upload)                     K = 2, short patterns
  k2n   k2s without the words shorter than 3 bytes                                                                     K = 2, none
  c32   31 distinct pattern bytes: 32 byte classes, the most the 5-bit class fields hold                               K = 2, short patterns
  c32n  c32 without the words shorter than 3 bytes: the only 32-class dictionary the 32-positions-per-lane instances take  K = 2, none
  w40   k3s with its words over 39 byte values: the wide table set (gram2w)

K2_BUDGET.  build_gram_tables (gram.cpp:89) takes K = 3 when 1024 + pad16(2 C^3) + pad16(8 combos) + pad16(4 ceil(C^4 / 32) + 8) +
pad16(words / 2) + pad16(4 ceil(words / 8)) + 64 bytes fit the budget.  With C = 9 that is 3 616 bytes + the COMBO table, at least 3 632;
K = 2 needs 1 408 bytes + at most 83 COMBO entries, 2 072 at the most.  9 216, the value the suite uses on 27-class dictionaries, leaves
these 9-class ones at K = 3; 3 072 lies between the two sums whatever the COMBO tables hold.

Texts, per dictionary, TEXT_BYTES = 3 * 2048 + 5 bytes each:
  soup     words joined by 0 .. 2 filler bytes, every third word cut short; ends with the 16-edge path's word, so that a prefix of the
           text 1 .. 9 bytes shorter ends inside a tail record or a walker's look-ahead dword
  uniform  random bytes over the alphabet and two bytes of no pattern
  deep     words with nothing between them: every position hits and goes on
(c32, c32n: each with the class-31 byte planted behind a depth-3 hit at the lane-63 edges, see C32_PLANTS.)

`ZERO_HASH`: (length, value) pairs whose match_hash32 = low32(mix64(value << 32 | length)) is 0 — found by exhaustive search over all 2^32
values per length; lengths 1, 5, 6, 9 and 10 have none.  A depth-(K+1) hit record carries no count: the kernels take count = (h32 != 0),
so a pattern with such a value at depth K + 1 is one the table builders must decline that K for."""
import numpy as np

from oracle import oracle as orc

ALPHA8 = b"acdeinrs"
OUTSIDE = b" \xc3"                      # two bytes of no pattern
ALPHA31 = bytes(range(0x41, 0x60))     # 'A' .. '_': classes 1 .. 31 in byte order (repack.cpp numbers the used bytes ascending)
Z31 = ALPHA31[30:31]                   # '_': class 31
Z15 = ALPHA31[14:15]                   # 'O': class 15 = 31 & 15
ALPHA39 = bytes(range(0x30, 0x57))     # '0' .. 'V': 39 pattern bytes, 40 classes
TEXT_BYTES = 3 * 2048 + 5
K2_BUDGET = 3072
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, TEXT_BYTES]
SHIFTS = [0, 5, 13, 15]
KINDS = ("soup", "uniform", "deep")
PATH_EDGES = list(range(9, 17))        # the single paths below depth 6

# name: (alphabet, shortest word kept, gram_lds_budget or None)
SPECS = {"k3s": (ALPHA8, 1, None), "k3n": (ALPHA8, 4, None), "k2s": (ALPHA8, 1, K2_BUDGET), "k2n": (ALPHA8, 3, K2_BUDGET),
         "c32": (ALPHA31, 1, None), "c32n": (ALPHA31, 3, None), "w40": (ALPHA39, 1, None)}
# what info() and the launch label must say: (gram_k, short)
EXPECT = {"k3s": (3, 1), "k3n": (3, 0), "k2s": (2, 1), "k2n": (2, 0), "c32": (2, 1), "c32n": (2, 0)}

ZERO_HASH = {2: (186830009, 2729480790, 3607083306), 3: (3409562211, 4261456336), 4: (1387117448, 3996936941, 4239958913),
             7: (2246160355, 2429703670), 8: (2774234896, 4182769736)}

# c32: the stem is a pattern and a depth-3 state (K + 1 with K = 2); behind it the class-31 byte as the first and as the second byte, each
# as a pattern, and the class-15 byte in the same places as no pattern (a class field cut to four bits finds those instead)
STEM = b"BCD"
C32_WORDS = [STEM, STEM + Z31, STEM + Z31 + b"E", STEM + b"E" + Z31, STEM + b"E" + Z31 + b"F", STEM + Z31 + Z31, STEM + b"E"]
# (offset of the stem's last byte, what follows): 1023 mod 1024 is the last position lane 63 owns in a step of 16 positions per lane,
# 2047 mod 2048 in a step of 32 — which only a dictionary without short patterns gets (gram_kernels.hip, launch_rl): c32n; on c32 those
# offsets are further 1023 mod 1024 edges.  The text's last bytes are planted as well
C32_PLANTS = [(1023, Z31 + b"E"), (2047, b"E" + Z31 + b"F"), (3071, Z31 + Z31), (4095, Z31 + b"E"), (5119, Z15 + b"E"),
              (1023 - 512, b"E" + Z15), (TEXT_BYTES - 3, b"E" + Z31)]
C32_LENGTHS = [2050, 4097, TEXT_BYTES - 1]   # (1025 and the whole text as well:) the class-31 byte as the text's last byte, one and two behind the stem


def match_hash32(value, length):
    from daachorse_amd import synth
    return int(synth.mix64(np.uint64((int(value) << 32) | int(length)))) & 0xFFFFFFFF


def _word(rng, al, n):
    return al[rng.integers(0, len(al), size=n)].tobytes()


def _generate(alphabet, seed=2024):
    """the k3s word list over `alphabet` (its first 8 bytes carry the structure; a wider alphabet only spreads the random letters)"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(alphabet, dtype=np.uint8)
    words = {}

    def add(w):
        words.setdefault(bytes(w))
    for size, many in ((1, 2), (2, 8), (3, 20), (4, 60), (5, 60), (6, 60), (7, 60), (8, 50), (9, 20), (11, 10)):
        have = len(words)
        while len(words) < have + many:
            add(_word(rng, al, size))
    # prefixes of longer words, down to one letter below and up to the whole of them
    for w in [w for w in words if len(w) >= 7][::5]:
        for cut in (4, 5, len(w) - 1):
            add(w[:cut])
    # single paths of 9 .. 16 edges below a depth-6 state: a 6-letter head no other word passes through, then `edges` letters; two of
    # them with a second word ending on the path (a state under which two patterns end gets no tail record)
    paths = []
    for edges in PATH_EDGES:
        while True:
            head = _word(rng, al, 6)
            if not any(w[:6] == head or head[:len(w)] == w and len(w) > 4 for w in words):
                break
        w = head + _word(rng, al, edges)
        add(w)
        paths.append(w)
        if edges in (12, 15):
            add(w[:6 + 5])
    return list(words), paths


class Dictionary:
    def __init__(self, name):
        alphabet, shortest, budget = SPECS[name]
        self.name, self.alphabet, self.budget = name, alphabet, budget
        if name in ("c32", "c32n"):
            rng = np.random.default_rng(31)
            al = np.frombuffer(alphabet, dtype=np.uint8)
            words = {}
            # every one of the 31 bytes in a pattern (one-byte words for a few of them); no random word begins as the stem does
            for b in alphabet:
                w = bytes([b]) + _word(rng, al, 2)
                words.setdefault(w if w != STEM else w[::-1])
            for size, many in ((1, 3), (2, 10), (3, 30), (4, 60), (5, 60), (6, 50), (7, 40), (9, 20)):
                have = len(words)
                while len(words) < have + many:
                    w = _word(rng, al, size)
                    if w[:3] != STEM and STEM not in w:
                        words.setdefault(w)
            self.words = [w for w in list(words) + C32_WORDS if len(w) >= shortest]
            self.paths = []
        else:
            words, self.paths = _generate(alphabet)
            self.words = [w for w in words if len(w) >= shortest]
        assert len(set(self.words)) == len(self.words)
        self.long_word = max(self.paths, key=len) if self.paths else None   # 6 + 16 bytes
        self._oracle = None
        self._texts = {}
        self._tuples = {}
        self._answers = {}

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = orc.OraclePma.build(self.words)
        return self._oracle

    def blob(self):
        return self.oracle.serialize()

    # ---- texts ----
    def _finish(self, text, kind):
        t = np.frombuffer(text[:TEXT_BYTES], dtype=np.uint8).copy()
        assert len(t) == TEXT_BYTES
        if self.name in ("c32", "c32n"):
            for last, behind in C32_PLANTS:
                piece = np.frombuffer(STEM + behind, dtype=np.uint8)
                piece = piece[:TEXT_BYTES - (last - 2)]
                t[last - 2:last - 2 + len(piece)] = piece
        elif kind == "soup":   # ends with the 16-edge path's word
            t[TEXT_BYTES - len(self.long_word):] = np.frombuffer(self.long_word, dtype=np.uint8)
        return t

    def text(self, kind, n=None):
        """`soup`, `uniform` or `deep`: the whole text or its first n bytes"""
        if kind not in self._texts:
            rng = np.random.default_rng({"soup": 11, "uniform": 12, "deep": 13}[kind])
            words = self.words
            if kind == "uniform":
                al = np.frombuffer(self.alphabet + OUTSIDE, dtype=np.uint8)
                raw = al[rng.integers(0, len(al), size=TEXT_BYTES)].tobytes()
            else:
                picks = rng.integers(0, len(words), size=TEXT_BYTES).tolist()   # (more than enough: every word has a byte at least)
                parts, size = [], 0
                for i, k in enumerate(picks):
                    w = words[k]
                    if kind == "soup":
                        if i % 3 == 2 and len(w) > 1:
                            w = w[:len(w) - 1 - int(rng.integers(0, min(3, len(w) - 1)))]   # cut short by 1 .. 3 bytes
                        w = w + bytes(OUTSIDE[int(x)] for x in rng.integers(0, 2, size=int(rng.integers(0, 3))))
                    parts.append(w)
                    size += len(w)
                    if size >= TEXT_BYTES:
                        break
                raw = b"".join(parts)
            self._texts[kind] = self._finish(raw, kind)
        t = self._texts[kind]
        return t if n is None else t[:n]

    def text_of(self, words, n, seed):
        """n bytes of soup of any length asked for (the several-regions cases); made once per (n, seed)"""
        key = ("long", n, seed)
        if key not in self._texts:
            rng = np.random.default_rng(seed)
            mean = sum(len(w) for w in words) / len(words) + 1
            picks = rng.integers(0, len(words), size=int(n / mean * 1.2) + 64).tolist()
            fill = rng.integers(0, 3, size=len(picks)).tolist()
            text = b"".join(words[k] + OUTSIDE[:1] * f for k, f in zip(picks, fill))
            assert len(text) >= n
            self._texts[key] = np.frombuffer(text[:n], dtype=np.uint8).copy()
        return self._texts[key]

    # ---- what the oracle finds: find_overlapping_iter once per text, every answer a subset of it ----
    def tuples(self, kind):
        if kind not in self._tuples:
            self._tuples[kind] = self.oracle.find_overlapping_iter(self.text(kind))
        return self._tuples[kind]

    def answer(self, kind, n=None, begin=0):
        """(count, checksum) of the matches with begin < end <= n of the text: what a scan of its first n bytes reports from `begin` on
        (begin = 0: all of them; no pattern is empty, so none ends at 0)"""
        n = TEXT_BYTES if n is None else n
        key = (kind, n, begin)
        if key not in self._answers:
            m = self.tuples(kind)
            sub = m[(m["end"] <= n) & (m["end"] > begin)]
            self._answers[key] = (len(sub), orc.matches_checksum(sub))
        return self._answers[key]


_cache = {}


def dictionary(name):
    if name not in _cache:
        _cache[name] = Dictionary(name)
    return _cache[name]


# ---------------------------------------------------------------- dictionaries that break "count = (h32 != 0)" (ZERO_HASH)
SPECIAL_AT = (0, 1023, 2047)   # a special word at the text's start, ending at these offsets, at its end, and once cut one byte short


def _fresh(words, rng, al, size, taken=()):
    """a word of `size` letters that no word of the list begins with, is, or is a prefix of"""
    while True:
        w = _word(rng, al, size)
        if w not in taken and not any(x[:size] == w or w[:len(x)] == x and len(x) >= 4 for x in words):
            return w


def zero_hash_cases():
    """name -> (patterns, values, the special words): k3s with index values + the patterns the issue's table adds"""
    base = dictionary("k3s").words
    al = np.frombuffer(ALPHA8, dtype=np.uint8)
    rng = np.random.default_rng(404)
    out = {}

    def case(name, extra):
        pats = list(base) + [w for w, _ in extra]
        vals = np.array(list(range(len(base))) + [v for _, v in extra], dtype=np.uint32)
        out[name] = (pats, vals, list(dict.fromkeys(w for w, _ in extra)))
    short2 = next(w for w in (_word(rng, al, 2) for _ in range(1000)) if w not in base)
    case("z_short", [(short2, ZERO_HASH[2][0])])
    w4 = _fresh(base, rng, al, 4)
    case("z_k3", [(w4, ZERO_HASH[4][0])])
    w3 = next(w for w in (_word(rng, al, 3) for _ in range(1000)) if w not in base)
    case("z_k2", [(w3, ZERO_HASH[3][0]), (w4, ZERO_HASH[4][1])])
    # length 7 on a branching path (an ordinary deep record: two longer words go on from it), length 8 alone at the end of a single path
    # from depth 6 on (K = 3: the depth-6 state is a tail record of two edges with this one pattern)
    w7 = _fresh(base, rng, al, 7)
    w8 = _fresh(base, rng, al, 8, taken=(w7,))
    while w8[:6] == w7[:6]:
        w8 = _fresh(base, rng, al, 8, taken=(w7,))
    case("z_deep", [(w7, ZERO_HASH[7][0]), (w7 + b"a", 7001), (w7 + b"c", 7002), (w8, ZERO_HASH[8][0])])
    case("dup_k", [(w4, 4001), (w4, 4002)])
    # four patterns ending at one K-gram (K = 3): a 3-byte word twice, its 2-byte and 1-byte suffixes
    s3 = next(w for w in (_word(rng, al, 3) for _ in range(1000)) if w not in base and w[1:] not in base and w[2:] not in base)
    case("four_short", [(s3, 3001), (s3, 3002), (s3[1:], 3003), (s3[2:], 3004)])
    return out


def special_text(pats, special, seed=5):
    """TEXT_BYTES of word soup with the special words planted: the first at the text's start and the last right behind it, the last at the
    text's end and the first right in front of it (so the text without its first len(first) + 1 bytes begins with the last, and without its
    last len(last) + 1 bytes ends with the first), first and last each ending at an offset 1023 mod 1024 and at one 2047 mod 2048, every
    one of them once between fillers and once cut one byte short"""
    rng = np.random.default_rng(seed)
    picks = rng.integers(0, len(pats), size=TEXT_BYTES).tolist()
    parts, size = [], 0
    for k in picks:
        parts.append(pats[k] + OUTSIDE[:1] * int(rng.integers(0, 2)))
        size += len(parts[-1])
        if size >= TEXT_BYTES:
            break
    t = np.frombuffer(b"".join(parts)[:TEXT_BYTES], dtype=np.uint8).copy()
    blank = OUTSIDE[:1]
    first, last = special[0], special[-1]

    def put_end(end, piece):   # the piece's last byte at offset end - 1
        t[end - len(piece):end] = np.frombuffer(piece, dtype=np.uint8)
    head = first + blank + last + blank
    put_end(len(head), head)
    put_end(512, blank + blank.join(special) + blank)
    put_end(1024, blank + first + blank + last)      # the last special word ends at offset 1023, the first at 2047 ...
    put_end(2048, blank + last + blank + first)
    put_end(3072, blank + last + blank + first)      # ... and the other way round at 1023 mod 1024 and 2047 mod 2048
    put_end(4096, blank + first + blank + last)
    put_end(5000, blank + blank.join(w[:-1] for w in special) + blank)
    put_end(TEXT_BYTES, blank + first + blank + last)
    return t
