"""Dictionaries and upload options that put the TIERED tables (build_tier_tables, repack.cpp) into every layout TierEngine::step has a
route for: dense rows of 16-bit and of 32-bit entries (tier A), states whose child bitmap and fail link lie in LDS (tier B) and states
read as one record from HBM (tier C).  tests/test_tier_layouts_host.py proves on the CPU that each layout named here exists;
tests/test_gpu_tier_layouts.py runs the device calls under each of them.

States are numbered breadth first and, inside one depth, in byte order of their prefixes: states [0, NA) are tier A, [NA, NB) tier B,
[NB, N) tier C.  Rows are 32-bit as soon as the states up to one level below the dense ones number 32 768 or more.
"""
import numpy as np

ALPHABET = b"abcdefghijklmnopqrstuvwxyz01234"   # 31 letters: with "no pattern byte" the 32 classes TIERED can take
OTHER = ord(" ")                                # a byte of no pattern (class 0)
HEADS = [bytes([x, ord("a")]) for x in ALPHABET] + [b"ab", b"bb"]

# prefixes of words of W: outputs and output chains (aaaa -> aaa -> aa -> a), no new states; "ab" twice: two slots in one list
PREFIXES = [b"a", b"aa", b"aaa", b"ab", b"ba", b"baa", b"b", b"bb", b"0a", b"0a0", b"za", b"zaz", b"ab"]

DEFAULT_BUDGET = 96 * 1024
BIG_BUDGET = 158 * 1024        # 161 792
MAX_BUDGET = 160 * 1024        # the largest lds_budget the option takes: what a workgroup can have


def w_words():
    """every head + z + t: 33 * 31 * 31 = 31 713 words, in construction order (head, then z, then t)"""
    return [h + bytes([z, t]) for h in HEADS for z in ALPHABET for t in ALPHABET]


def w_patterns(name):
    """W, W_lo (W without its last 33 words: 32 767 states, the largest id 32 766 still fits 15 bits) or W_hi (without its last 32:
    32 768 states, the first dictionary whose rows are 32-bit at dense_depth 3)"""
    words = w_words()
    drop = {"W": 0, "W_lo": 33, "W_hi": 32}[name]
    return words[:len(words) - drop] + PREFIXES


def root_only_budget(C, k=0):
    """lds_budget that leaves ROOT's 16-bit row (2C + 8 bytes of rows and sums) and k tier-B states (8 bytes each)"""
    return 320 + 2 * C + 8 + 8 * k


# (name, dictionary, options, what build_tier_tables gives: N / NA / NB / row32, or None where it declines)
W_LAYOUTS = [
    ("default",     "W",    {},                                                          dict(N=32801, NA=65,   NB=11728, row32=0)),
    ("rows32",      "W",    {"lds_budget": BIG_BUDGET, "dense_depth": 3},                dict(N=32801, NA=1088, NB=2776,  row32=1)),
    ("rows16_edge", "W_lo", {"lds_budget": BIG_BUDGET, "dense_depth": 3},                dict(N=32767, NA=1087, NB=11488, row32=0)),
    ("rows32_edge", "W_hi", {"lds_budget": BIG_BUDGET, "dense_depth": 3},                dict(N=32768, NA=1087, NB=2792,  row32=1)),
    ("rows32_auto", "W",    {"lds_budget": BIG_BUDGET, "rows_share_pct": 100},           dict(N=32801, NA=1088, NB=2776,  row32=1)),
    ("rows32_max",  "W",    {"lds_budget": MAX_BUDGET, "dense_depth": 3},                dict(N=32801, NA=1088, NB=3032,  row32=1)),
    ("declined",    "W",    {"lds_budget": DEFAULT_BUDGET, "dense_depth": 3},            None),
    ("root_c",      "W",    {"lds_budget": root_only_budget(32), "dense_depth": 0},      dict(N=32801, NA=1,    NB=1,     row32=0)),
    ("root_b5",     "W",    {"lds_budget": 432, "dense_depth": 0},                       dict(N=32801, NA=1,    NB=6,     row32=0)),
    ("root_b40",    "W",    {"lds_budget": 712, "dense_depth": 0},                       dict(N=32801, NA=1,    NB=41,    row32=0)),
]
W_SCANNED = [l for l in W_LAYOUTS if l[3] is not None]


def w_texts(seed=20260):
    """-> {name: uint8 array}; 64 KiB each for the two long ones"""
    rng = np.random.default_rng(seed)
    words = w_words()
    n = 1 << 16
    uniform = rng.choice(np.frombuffer(ALPHABET + bytes([OTHER]), dtype=np.uint8), size=n)
    picked = [min(words), max(words)] + [words[i] for i in rng.integers(0, len(words), size=n // 4 - 2).tolist()]
    soup = np.frombuffer(b"".join(picked), dtype=np.uint8)
    assert len(soup) == n
    texts = {"uniform": uniform, "words": soup, "run_a": np.full(4099, ord("a"), dtype=np.uint8)}
    for k in (0, 1, 3, 17):    # 3 is shorter than the halo's reach of a 4-byte pattern; 17 is one 16-byte vector and a byte
        texts[f"len{k}"] = soup[:k]
    return texts


def extreme_words():
    """the words that end in the lowest and the highest depth-4 state: tier B and tier C wherever NA < NB < N"""
    words = w_words()
    return min(words), max(words)


def trie_shape(patterns):
    """-> (N, states of depth <= 1, C) of the patterns' trie: what the tiny layouts' budgets are worked out from"""
    pats = [bytes(p) for p in patterns]
    prefixes = {p[:i] for p in pats for i in range(len(p) + 1)} | {b""}
    return len(prefixes), sum(1 for p in prefixes if len(p) <= 1), 1 + len({c for p in pats for c in p})


def tiny_patterns(rng):
    """as tests/test_gpu_parity.py::test_fuzz_small_alphabets draws them: up to six patterns of up to five bytes over {a, b, c},
    "" and duplicates among them"""
    npat = int(rng.integers(1, 7))
    return [bytes(rng.integers(97, 100, size=int(rng.integers(0, 6))).astype(np.uint8)) for _ in range(npat)]


TINY_LAYOUTS = ("root_c", "root_half", "root_all", "depth1_half")


def tiny_layout(name, patterns):
    """-> (options, {N, NA, NB, row32}) of a tiny dictionary under one of TINY_LAYOUTS"""
    N, n1, C = trie_shape(patterns)
    if name == "depth1_half":
        k = (N - n1) // 2
        opts = {"lds_budget": 320 + n1 * (2 * C + 8) + 8 * k, "dense_depth": 1}
        NA = n1
    else:
        k = {"root_c": 0, "root_half": (N - 1) // 2, "root_all": N + 1}[name]
        opts = {"lds_budget": root_only_budget(C, k), "dense_depth": 0}
        NA = 1
    return opts, dict(N=N, NA=NA, NB=min(N, NA + k), row32=0)


def tiny_cases(layout, trials=60):
    """the seeded trials of one layout -> [(patterns, haystack, options, shape)]; odd trials' text has a byte of no pattern"""
    rng = np.random.default_rng(4321 + TINY_LAYOUTS.index(layout))
    out = []
    for it in range(trials):
        pats = tiny_patterns(rng)
        hay = rng.integers(97, 100 + (it % 2), size=int(rng.integers(0, 400)), dtype=np.uint8)
        opts, shape = tiny_layout(layout, pats)
        out.append((pats, hay, opts, shape))
    return out


def slot_counts(outputs, m):
    """tuples -> matches per slot (row of outputs()), each tuple mapped by (value, end - start); asserted one to one"""
    outs = np.asarray(outputs)
    key = lambda v, l: (np.asarray(v, dtype=np.uint64) << np.uint64(32)) | np.asarray(l, dtype=np.uint64)
    keys = key(outs[:, 0], outs[:, 1])
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    assert len(np.unique(sk)) == len(sk), "patterns share (value, length)"
    mk = key(m["value"], m["end"] - m["start"])
    at = np.searchsorted(sk, mk)
    assert np.all(at < len(sk)) and np.array_equal(sk[np.minimum(at, len(sk) - 1)], mk)
    return np.bincount(order[at], minlength=len(outs)).astype(np.uint64)
