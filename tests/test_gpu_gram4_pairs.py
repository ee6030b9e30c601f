"""gram4's count kernel after round 11 — the M-word address shared between the two positions of a pair (gram4_index.hpp), slab entries with the
gathered record first, hit-list entries as LDS addresses, the count sum and the probe's pass mask — against the oracle's find_overlapping_iter
count of the same bytes: every body (FILT + hash, FILT + rank, plain, TAIL) at 16 and 32 positions per lane, K = 3 with arithmetic classes and
with a class table, K = 2; texts short enough to end inside a lane's first pair and long enough for several regions per wave, from every buffer
alignment, with bytes of no pattern on either side of a pair, and word soup with the walker slab at its minimum so that it drains in mid-region."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode

SCATTERED = bytes([3, 9, 17, 33, 34, 40, 47, 48, 57, 65, 70, 77, 80, 90, 97, 99, 101, 110, 120, 122, 130, 150, 170, 190, 200, 210, 230, 250, 255])
LENGTHS = [1, 31, 32, 33, 2047, 2048, 2049, 3 * 2048 + 5, (1 << 20) + 3]
BODIES = [("filt+hash", "hash", {"gram3_tail": 0}), ("filt+rank", "rank", {"gram3_tail": 0}),
          ("plain", "hash", {"gram4_filter": 0, "gram3_tail": 0}), ("tail", "hash", {"gram3_tail": 1})]


# What daac_last_kernel() must say for each dictionary and body, so that a label is what ran.  a: 79 KB of M words, room for the Bloom array beside
# either front table.  b: 108 KB of M words and a class table; the perfect hash's displacement table (a byte a bucket) leaves the Bloom array room, the
# coarse directory (13.5 KB) does not, so its records by rank run without the filter (FILT + rank over a class table: dictionary a with gram4_arith = 0 in
# test_other_launch_shapes).  c: twenty words hold fewer keys than the smallest Bloom array is built for (64 words), so the handle has no filter and no
# hash: the four option sets run its plain and TAIL bodies at K = 2.
EXPECT = {
    ("a", "filt+hash"): {"arith": "1", "filter": "1", "mph": "1", "tail": "0"}, ("a", "filt+rank"): {"arith": "1", "filter": "1", "mph": "0", "tail": "0"},
    ("a", "plain"): {"arith": "1", "filter": "0", "mph": "0", "tail": "0"}, ("a", "tail"): {"arith": "1", "tail": "1"},
    ("b", "filt+hash"): {"arith": "0", "filter": "1", "mph": "1", "tail": "0"}, ("b", "filt+rank"): {"arith": "0", "filter": "0", "mph": "0", "tail": "0"},
    ("b", "plain"): {"arith": "0", "filter": "0", "mph": "0", "tail": "0"}, ("b", "tail"): {"arith": "0", "tail": "1"},
    ("c", "filt+hash"): {"arith": "1", "filter": "0", "mph": "0", "tail": "0"}, ("c", "filt+rank"): {"arith": "1", "filter": "0", "mph": "0", "tail": "0"},
    ("c", "plain"): {"arith": "1", "filter": "0", "mph": "0", "tail": "0"}, ("c", "tail"): {"arith": "1", "tail": "1"},
}


def _words_a():
    """about 2 000 words over a-z, 1-9 letters, three in five grown from one of 120 stems of 4 or 5 letters"""
    rng = np.random.default_rng(5)
    al = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    stems = [bytes(al[rng.integers(0, 26, size=int(rng.integers(4, 6)))]) for _ in range(120)]
    out = set()
    while len(out) < 2000:
        if rng.random() < 0.6:
            s = stems[int(rng.integers(0, len(stems)))]
            out.add(s + bytes(al[rng.integers(0, 26, size=int(rng.integers(0, 10 - len(s))))]))
        else:
            out.add(bytes(al[rng.integers(0, 26, size=int(rng.integers(1, 10)))]))
    return sorted(out)


def _dictionaries():
    a = _words_a()
    to_scattered = bytes.maketrans(b"abcdefghijklmnopqrstuvwxyz", SCATTERED[:26])
    b = sorted(set(w.translate(to_scattered) for w in a) | {SCATTERED[26:], SCATTERED[25:28], SCATTERED[27:] + SCATTERED[:2]})
    # two patterns "a": four patterns end with the 3-gram "aaa", more than an M word's two count bits hold — the upload takes K = 2
    c = [b"a", b"a", b"aa", b"aaa", b"ab", b"abc", b"abcd", b"abcde", b"bca", b"bcab", b"cab", b"cabc", b"cabca", b"bb", b"bbc", b"bbca", b"ccc",
         b"cccc", b"ccccc", b"abcabc"]
    return {"a": (a, b"abcdefghijklmnopqrstuvwxyz ", 3), "b": (b, SCATTERED + b" ", 3), "c": (c, b"abcde ", 2)}


class _Case:
    """one dictionary: the oracle, a handle with the hash and one with records by rank, the texts and their counts (worked out once)"""

    def __init__(self, name):
        import torch
        pats, alpha, k = _dictionaries()[name]
        self.name, self.pats = name, pats
        self.oracle = orc.OraclePma.build(pats)
        self.handles = {}
        for how, mph in (("hash", 8), ("rank", 0)):
            p, _ = da.DoubleArrayAhoCorasick.deserialize(self.oracle.serialize())
            p.set_option("gram4_mph", mph)   # (read when the tables are laid out)
            info = p.upload().info()
            assert info.gram2_available and info.gram2_k == k, (name, info.gram2_k)
            self.handles[how] = p
        rng = np.random.default_rng(2024)
        al = np.frombuffer(alpha, dtype=np.uint8)
        lo, hi = int(min(al[:-1])), int(max(al[:-1]))
        uniform = al[rng.integers(0, len(al), size=LENGTHS[-1])]
        # one byte in eight replaced by a byte of no pattern: below the range, above it, 0x80 and up — at even and at odd offsets
        outside = np.array([b for b in list(range(max(0, lo - 3), lo)) + list(range(hi + 1, min(256, hi + 4))) + [0x80, 0xc3, 0xff] if bytes([b]) not in alpha] or [0],
                           dtype=np.uint8)
        holes = uniform.copy()
        at = np.arange(0, len(holes), 8) + rng.integers(0, 8, size=(len(holes) + 7) // 8)
        at = at[at < len(holes)]
        holes[at] = outside[rng.integers(0, len(outside), size=len(at))]
        soup = np.frombuffer(b"".join(pats[i] for i in rng.integers(0, len(pats), size=(256 << 10) // 2 + 64).tolist())[:256 << 10], dtype=np.uint8).copy()
        assert len(soup) == 256 << 10
        self.texts = {"uniform": uniform, "holes": holes, "soup": soup}
        self.want = {(t, n): len(self.oracle.find_overlapping_iter(self.texts[t][:n])) for t in ("uniform", "holes") for n in LENGTHS}
        self.want[("soup", len(soup))] = len(self.oracle.find_overlapping_iter(soup))
        # each text once on the device behind 16 spare bytes: [16 - s + s ..] views start at every alignment without further copies
        self.dev = {}
        for t, v in self.texts.items():
            for s in range(16):
                buf = torch.empty(16 + len(v) + 16, dtype=torch.uint8, device="cuda")
                buf[s:s + len(v)] = torch.from_numpy(v).cuda()
                self.dev[(t, s)] = buf[s:s + len(v)]

    def count(self, how, text, shift, n, **opts):
        p = self.handles[how]
        for k, v in {"gram_version": 4, "gram_ppl": 32, "gram3_tail": 0, "gram2_rfull": 1, "threads": 1024, "gram4_arith": 1, "gram4_filter": 1, "gram_region": 2048,
                     "gram_slab": 4096, **opts}.items():
            p.set_option(k, v)
        got = p.count(ScanMode.FindOverlapping, self.dev[(text, shift)][:n], engine=Engine.Gram)
        lk = da.last_kernel()
        assert da.last_engine() == int(Engine.Gram) and lk.startswith("gram4 "), lk
        return got, dict(kv.split("=") for kv in lk.split()[1:])

    def ran(self, label, lk, ppl=32):
        """the launch was the body the label names: daac_last_kernel()'s fields against EXPECT"""
        want = {"ppl": str(ppl), **EXPECT[(self.name, label)]}
        assert {k: lk[k] for k in want} == want, (self.name, label, lk, want)


_cases = {}


@pytest.fixture(params=["a", "b", "c"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    return _cases[request.param]


@pytest.mark.parametrize("body", BODIES, ids=[b[0] for b in BODIES])
def test_every_length_and_alignment(case, body):
    """texts i and ii: every length around a lane's share, a step and a region, from every alignment of the buffer, at 16 and 32 positions per lane"""
    _, how, opts = body
    for text in ("uniform", "holes"):
        for n in LENGTHS:
            for ppl in (16, 32):
                for shift in range(16):
                    got, lk = case.count(how, text, shift, n, gram_ppl=ppl, **opts)
                    assert got == case.want[(text, n)], (case.name, body[0], text, n, ppl, shift, lk, got, case.want[(text, n)])
                    case.ran(body[0], lk, ppl)


@pytest.mark.parametrize("body", BODIES, ids=[b[0] for b in BODIES])
def test_word_soup_with_the_smallest_slab(case, body):
    """text iii: nearly every hit goes on; the slab at its minimum drains in mid-region, with raw entries and entries written back side by side"""
    _, how, opts = body
    n = len(case.texts["soup"])
    for ppl in (16, 32):
        for shift, region in ((0, 2048), (5, 0)):
            got, lk = case.count(how, "soup", shift, n, gram_ppl=ppl, gram_slab=0, gram_region=region, **opts)
            assert got == case.want[("soup", n)], (case.name, body[0], ppl, shift, region, lk, got)
            case.ran(body[0], lk, ppl)


def test_other_launch_shapes(case):
    """512 threads, the class table where the classes could be arithmetic, the coarse directory, the body by the density probe"""
    n = LENGTHS[-1]
    for opts in ({"threads": 512}, {"threads": 512, "gram_ppl": 16}, {"gram4_arith": 0}, {"gram2_rfull": 0}, {"gram2_rfull": 0, "gram3_tail": 1},
                 {"gram3_tail": -1, "gram_region": 0}, {"gram4_arith": 0, "gram4_filter": 0, "gram2_rfull": 0, "threads": 512}):
        for how in ("hash", "rank"):
            for text, shift in (("uniform", 3), ("holes", 8)):
                got, lk = case.count(how, text, shift, n, **opts)
                assert got == case.want[(text, n)], (case.name, how, text, opts, lk, got)
                assert lk["waves"] == str(opts.get("threads", 1024) // 64) and (case.name != "a" or lk["arith"] == str(opts.get("gram4_arith", 1))), (opts, lk)
                if case.name == "a":
                    assert lk["filter"] == str(opts.get("gram4_filter", 1)) and lk["mph"] == ("1" if how == "hash" and lk["filter"] == "1" else "0"), (opts, lk)
            m = len(case.texts["soup"])
            got, lk = case.count(how, "soup", 1, m, gram_slab=0, **opts)
            assert got == case.want[("soup", m)], (case.name, how, opts, lk, got)
