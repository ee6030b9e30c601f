"""Dictionaries on either side of 65 536 depth-(K+1) trie states, their texts and what the CPU oracle finds in them — shared by
tests/test_gram_u32dir_host.py and tests/test_gpu_gram_u32dir.py (a plain module, imported by name; everything is generated from seeds).

A GRAM table set keeps a rank directory over the continuation bits of its M words.  Its entries are 16 bits wide while the dictionary has
fewer than 65 536 states at depth K + 1 (gram2.cpp: `s16 = n_deep < 65536`); from 65 536 on they are 32 bits wide, there is no per-word
directory, and every consumer runs another compiled kernel.  With K = 3 the depth-4 states are the distinct 4-byte prefixes of the words
of four bytes and more, so a dictionary's side of the threshold is counted here from its sorted prefix list, without the tables.

  big20   70 000 four-letter prefixes over a-t, each grown by 0-4 letters           (small tables: every launch shape fits)
  big20s  big20's words on 20 scattered byte values, in the same order              (class table instead of arithmetic classes)
  big18   the same construction over a-r                                            (no perfect hash is found: records by rank)
  big26   the same over a-z                                                         (M words and directory of the benchmark's size)
  edge_hi 65 536 prefixes over a-t; edge_lo: edge_hi without the word of its last prefix — 65 535, the largest u16 directory

Every dictionary also holds a few words of one to three letters, so that the short-pattern bits of the M words are in use.

Texts, per dictionary: `soup` (256 KiB of words end to end), `high` (256 KiB of soup of the words whose prefix has rank >= 65 536 in sorted
order — the only hits a directory cut to 16 bits gets wrong; the edge pair: of the last 1 000 prefixes), `holes` (1 MiB + 3 uniform over the
alphabet and space, one byte in eight a byte of no pattern) and `long` (word soup of any length asked for, for the claimed-regions cases)."""
import numpy as np

from oracle import oracle as orc

LETTERS = b"abcdefghijklmnopqrstuvwxyz"
# ascending, so that a translated dictionary keeps its sorted order (ranks are the same), and no contiguous range
SCATTERED = bytes([3, 9, 17, 33, 34, 40, 47, 48, 57, 65, 70, 77, 80, 90, 97, 99, 101, 110, 120, 122, 130, 150, 170, 190, 200, 210, 230, 250, 255])
THRESHOLD = 65536
SOUP_BYTES = 256 << 10
HOLES_BYTES = (1 << 20) + 3

# name: (letters, prefixes, seed, scattered bytes)
SPECS = {"big20": (20, 70000, 20, False), "big20s": (20, 70000, 20, True), "big18": (18, 70000, 18, False), "big26": (26, 70000, 26, False),
         "edge_hi": (20, THRESHOLD, 77, False), "edge_lo": (20, THRESHOLD, 77, False)}


def _generate(letters, n_prefixes, seed):
    """n_prefixes words of 4-8 letters with pairwise distinct 4-letter prefixes + 38 words of 1-3 letters, over the first `letters` of a-z"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(LETTERS[:letters], dtype=np.uint8)
    codes = rng.choice(letters ** 4, size=n_prefixes, replace=False)
    head = np.stack([al[(codes // letters ** (3 - i)) % letters] for i in range(4)], axis=1)
    ext_len = rng.integers(0, 5, size=n_prefixes)
    ext = al[rng.integers(0, letters, size=(n_prefixes, 4))]
    words = [head[i].tobytes() + ext[i, :ext_len[i]].tobytes() for i in range(n_prefixes)]
    short = set()
    for size, many in ((1, 2), (2, 12), (3, 24)):
        part = set()
        while len(part) < many:
            part.add(al[rng.integers(0, letters, size=size)].tobytes())
        short |= part
    return words + sorted(short)


def prefix_keys(words):
    """the distinct 4-byte prefixes of the words of four bytes and more, as big-endian numbers, ascending: index = rank of the depth-4 state"""
    heads = np.frombuffer(b"".join(w[:4] for w in words if len(w) >= 4), dtype=">u4").astype(np.uint32)
    return np.unique(heads)


class Dictionary:
    def __init__(self, name):
        letters, n_prefixes, seed, scattered = SPECS[name]
        self.name, self.letters = name, letters
        words = _generate(letters, n_prefixes, seed)
        if name == "edge_lo":   # without the one word of the last prefix
            last = max(w[:4] for w in words if len(w) >= 4)
            words = [w for w in words if w[:4] != last]
        self.alphabet = LETTERS[:letters]
        if scattered:
            table = bytes.maketrans(LETTERS[:letters], SCATTERED[:letters])
            words = [w.translate(table) for w in words]
            self.alphabet = SCATTERED[:letters]
        self.words = words
        self.keys = prefix_keys(words)
        self.n_deep = len(self.keys)
        assert len(set(words)) == len(words) and self.n_deep == len([w for w in words if len(w) >= 4])   # one word per prefix
        # the words the `high` text is made of
        if self.n_deep > THRESHOLD:
            floor = self.keys[THRESHOLD]
        else:
            floor = self.keys[self.n_deep - 1000]
        self.high_words = [w for w in words if len(w) >= 4 and int.from_bytes(w[:4], "big") >= int(floor)]
        self._oracle = None
        self._texts = {}
        self._counts = {}
        self._tuples = {}

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = orc.OraclePma.build(self.words)
        return self._oracle

    def blob(self):
        return self.oracle.serialize()

    # ---- texts ----
    def _soup(self, words, n, seed):
        rng = np.random.default_rng(seed)
        mean = sum(len(w) for w in words) / len(words)
        picks = rng.integers(0, len(words), size=int(n / mean * 1.1) + 64).tolist()
        text = b"".join(words[i] for i in picks)
        assert len(text) >= n
        return np.frombuffer(text[:n], dtype=np.uint8).copy()

    def text(self, kind, n=None):
        """`soup`, `high`, `holes` (whole or their first n bytes) or `long` (n bytes of word soup)"""
        if kind == "long":
            key = ("long", n)
            if key not in self._texts:
                self._texts[key] = self._soup(self.words, n, 4)
            return self._texts[key]
        if kind not in self._texts:
            if kind == "soup":
                t = self._soup(self.words, SOUP_BYTES, 1)
            elif kind == "high":
                t = self._soup(self.high_words, SOUP_BYTES, 2)
            elif kind == "holes":
                rng = np.random.default_rng(3)
                al = np.frombuffer(self.alphabet + b" ", dtype=np.uint8)
                lo, hi = min(self.alphabet), max(self.alphabet)
                # bytes of no pattern: just below the alphabet's range, just above it, inside it where it has gaps, 0x80 and up
                outside = np.array(sorted({b for b in list(range(max(0, lo - 3), lo)) + list(range(hi + 1, min(256, hi + 4))) + [lo + 1, hi - 1, 0x80, 0xc3, 0xff]
                                           if b not in self.alphabet}), dtype=np.uint8)
                t = al[rng.integers(0, len(al), size=HOLES_BYTES)]
                at = np.arange(0, HOLES_BYTES, 8) + rng.integers(0, 8, size=(HOLES_BYTES + 7) // 8)
                at = at[at < HOLES_BYTES]
                t[at] = outside[rng.integers(0, len(outside), size=len(at))]
            else:
                raise KeyError(kind)
            self._texts[kind] = t
        t = self._texts[kind]
        return t if n is None else t[:n]

    # ---- what the oracle finds (computed once) ----
    def count(self, kind, n=None, begin=0):
        """(count, checksum) of find_overlapping_iter over the text as a haystack of its own; begin: only the matches that end behind it"""
        key = (kind, n, begin)
        if key not in self._counts:
            if begin == 0:
                self._counts[key] = self.oracle.overlapping_count(self.text(kind, n), threads=4)
            else:
                m = self.tuples(kind, n)
                self._counts[key] = (int((m["end"] > begin).sum()), orc.matches_checksum(m[m["end"] > begin]))
        return self._counts[key]

    def tuples(self, kind, n=None):
        key = (kind, n)
        if key not in self._tuples:
            self._tuples[key] = self.oracle.find_overlapping_iter(self.text(kind, n))
        return self._tuples[key]

    # ---- the condition on the inputs ----
    def deep_hits(self, text):
        """(positions of the text where a 4-byte prefix of the dictionary ends, how many of them on a prefix of rank >= 65 536)"""
        t = np.ascontiguousarray(text)
        win = (t[:-3].astype(np.uint32) << 24) | (t[1:-2].astype(np.uint32) << 16) | (t[2:-1].astype(np.uint32) << 8) | t[3:].astype(np.uint32)
        idx = np.searchsorted(self.keys, win)
        hit = self.keys[np.minimum(idx, self.n_deep - 1)] == win
        return int(hit.sum()), int((hit & (idx >= THRESHOLD)).sum())


_cache = {}


def dictionary(name):
    if name not in _cache:
        _cache[name] = Dictionary(name)
    return _cache[name]
