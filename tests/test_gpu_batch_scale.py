"""The batch calls on the MI355X where the code does something else than at toy scale: more than 8192 scanned counts (A), more items than
one turn of a capped grid takes (B), and positions across and above 2^32 in the batch's buffer (C).

Documents come from pools of at most 256 short documents (tests/batch_scale.py).  Expected values come from the references the suite
already uses, run once per pool document — the CPU oracle for counts, checksums, tuples and histogram rows, the pure-Python definitions
(`_bpe`, `_viterbi`, `_tokens`, `_splice`, the split scanners, special_golden, normalize_golden, wordpiece_golden) for the rest — and are
laid out for the whole batch by `expand`, which tests/test_batch_scale_host.py holds against the per-document loop.  Never from the
library, at a low base or otherwise.  Every comparison is exact; unigram scores are compared as their uint32 views.

A. launch_exclusive_scan (scan_kernels.hip) sums up to 4 * kScanChunk = 8192 counts in one workgroup and more in three launches.  The
   scans of this family sum units + 1 counts.  The units are the documents in batch_layout, the tuple and histogram passes and the BPE,
   unigram and WordPiece tokenizers (api_batch.hip, api_bpe.hip, api_unigram.hip, api_wordpiece.hip): n = 8191 is the last size one
   workgroup sums, 8192 and 8193 the first two it does not, 12289 six chunks and one.  replace_all_batch and tokenize_batch sum per
   match besides (api_replace.hip, api_tokenize.hip), about 2.4 n here.  normalize_batch sums per tile of kNormTile = 1024 bytes of
   text and has no closing entry (api_normalize.hip), so its batches have 8191, 8192, 8193 and 12289 tiles, whatever their documents:
   8192 tiles are the last size one workgroup sums there.
B. One batch of n = 2^20 + 257 documents: more than 4096 blocks x 256 lanes (batch_plan, batch_reduce, batch_doc_offsets:
   batch_kernels.hip launch_batch_plan / _reduce / _doc_offsets; split_mark, split_docs, offsets_compose, spans_rebase, both
   split_words_space: split_kernels.hip; normalize_docs, spans_to_source: normalize_kernels.hip; batch_hist_classify:
   batch_hist_kernels.hip; replace_doc_offsets: replace_kernels.hip) and more than num_cu * 8 blocks x 256 lanes of the chain walkers
   (launch_batch_chain) and the pieces of launch_batch_pieces.  With more than 2^21 matches or rows the 8192 x 256 grids of tokenize_prep,
   replace_size, replace_finish and batch_hist_copy take a second turn too.  A smaller batch of more than 65536 x 4 segments does the
   same to splice_write_kernel, which takes a wave per segment (cut_kernels.hip).
C. The same calls on a window of a buffer of 4 GiB + 64 MiB of which nothing else is initialised, once with position 2^32 inside a
   multi-byte character (and a pattern occurrence, a special token) of a document in the middle of the batch, once wholly above 2^32.
   Absolute results (word_offsets, seg_offsets) are the reference's plus the base, relative ones are unchanged.

Deliberately not pinned here, because none is a few-seconds test with an independent reference: the 65536-block caps of the BPE, unigram,
WordPiece and cut kernels (a second turn above 16 777 216 documents), split_batch's second grid dimension (above 2^20 tiles, 1 GiB of
text), tokenize_tiles / replace_tiles (above 8 GiB), totals above 2^32 tokens or tuples, and normalize_longest_kernel, which
api_normalize.hip launches only with src for 4 GiB of text and more: its second turn needs that much initialised text in more than 2^20
documents."""
import re

import numpy as np
import pytest
import torch

import batch_scale as bs
import normalize_golden as ng
import special_golden as sg
from oracle import oracle as orc
from test_gpu_tokenize_unigram import _bits, _viterbi
from test_gpu_tokenize_wordpiece import VOCAB

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, ScanMode, Split

GID = 0x10000
MODES = (ScanMode.FindOverlapping, ScanMode.FindOverlappingNoSuffix, ScanMode.Find, ScanMode.LeftmostFind)
CHAIN_MODES = (ScanMode.Find, ScanMode.LeftmostFind)
A_SIZES = (8191, 8192, 8193, 12289)
N_BIG = bs.TURN + 257
RULES = (Split.Gpt2, Split.Cl100k, Split.O200k, Split.Bert, Split.Whitespace)
SPEC = [(b"<|e|>", 7), (b"<|end|>", 9), (b"<|", 11)]
P32 = 1 << 32
LANE_MAX = 1024   # batch_lane_max of the automata of part C: the document across 2^32 is longer and takes the long route


def _kind(mode):
    return 1 if mode == ScanMode.LeftmostFind else 0


def _eq(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][0])
            raise AssertionError((what, j, "first difference at item", at, g[at].tolist(), w[at].tolist()))


def _lk(key):
    m = re.search(r"\b%s=(\d+)" % key, da.last_kernel())
    assert m, (key, da.last_kernel())
    return int(m.group(1))


def _device(hay, off, base=101, front=b"\xe4\xb8", tail=b"\x96bc"):
    """the packed batch behind `base` bytes that belong to no document, in a buffer of its own"""
    big = torch.empty(base + len(hay) + 64, dtype=torch.uint8, device="cuda")
    return bs.high_window(big, (hay, off), base, front, tail)


def _tuples(got):
    return got["start"], got["end"], got["value"]


class _Family:
    """one dictionary as a Standard and a LeftmostLongest automaton (oracle and library), its pool and the references per pool document"""

    def __init__(self, charwise=False, empty=False, seed=3):
        pats = list(bs.CHAR_PATTERNS if charwise else bs.BYTE_PATTERNS) + ([""] if empty else [])
        self.n_pat = len(pats) - empty
        self.o, self.p = {}, {}
        for kind in (0, 1):
            if charwise:
                self.o[kind] = orc.OracleCharwisePma.build(pats, kind=kind)
                self.p[kind], rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(self.o[kind].serialize())
            else:
                self.o[kind] = orc.OraclePma.build(pats, kind=kind)
                self.p[kind], rest = da.DoubleArrayAhoCorasick.deserialize(self.o[kind].serialize())
            assert rest == b""
        keep = (lambda d: bs.terminates(self.o[1], ScanMode.LeftmostFind, d)) if empty else None
        self.pool = bs.make_pool(bs.CHAR_HAND if charwise else bs.BYTE_HAND, bs.CHAR_LETTERS if charwise else bs.BYTE_LETTERS, 64, seed, keep=keep)
        assert bs._b(self.pool[0]) == b""
        self.charwise, self.cache = charwise, {}
        self.tail = "界".encode() if charwise else b"\x96bc"   # completes a pattern behind a document that ends in its prefix

    def ref(self, what, *args):
        """bs.ref_<what> over the pool, computed once: scan, hist, matches, replace and tokenize take (mode, ..), bpe and unigram do not"""
        key = (what,) + tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args)
        if key not in self.cache:
            if what in ("bpe", "unigram"):
                self.cache[key] = getattr(bs, "ref_" + what)(self.o[0], self.pool, *args)
            else:
                self.cache[key] = getattr(bs, "ref_" + what)(self.o[_kind(args[0])], args[0], self.pool, *args[1:])
        return self.cache[key]

    def pins(self):
        return bs.pins_of(self.ref("matches", ScanMode.Find), self.pool)


class _World:
    def __init__(self):
        self.items = {}

    def get(self, key, make):
        if key not in self.items:
            self.items[key] = make()
        return self.items[key]

    def family(self, charwise=False, empty=False):
        return self.get(("family", charwise, empty), lambda: _Family(charwise, empty))

    def wordpiece(self, charwise=False):
        def make():
            patterns, first, cont = da.wordpiece_tables(VOCAB)
            new = da.CharwiseDoubleArrayAhoCorasick.new if charwise else da.DoubleArrayAhoCorasick.new
            return new([x.decode() for x in patterns] if charwise else patterns), first, cont, {k.encode(): i for k, i in VOCAB.items()}
        return self.get(("wordpiece", charwise), make)

    def special(self):
        return self.get("special", lambda: da.SpecialTokens(SPEC))

    def normalizer(self):
        return self.get("normalizer", lambda: (da.bert_normalizer(*ng.OPTIONS["default"]), ng.rules_image(*da.bert_normalizer_rules(*ng.OPTIONS["default"]))))

    def text_pool(self):
        return self.get("text_pool", lambda: bs.make_pool(bs.TEXT_HAND, bs.TEXT_LETTERS, 96, 5, max_letters=8))


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.items.clear()
    torch.cuda.empty_cache()


def _scores(n_pat):
    return -np.random.default_rng(2).random(n_pat).astype(np.float32) * 3


def _ranks(n_pat):
    return np.random.default_rng(1).permutation(n_pat).astype(np.uint32)


# ------------------------------------------------------------------------------------------------- the checks A, B and C share
def _route(mode, n, long_docs):
    """the route daac_last_kernel() reports for a batch scan: the overlapping modes cut every document into pieces (one each here: no
    document is longer than a piece) and take none through the long route, the chain modes take `long_docs` through it"""
    assert da.last_kernel().startswith("batch "), da.last_kernel()
    if mode in CHAIN_MODES:
        assert (_lk("lane_docs"), _lk("long_docs")) == (n - long_docs, long_docs), da.last_kernel()
    else:
        assert (_lk("pieces"), _lk("lane_docs"), _lk("long_docs")) == (n, n, 0), da.last_kernel()


def _check_scans(fam, idx, batch, what, modes=MODES, long_docs=0):
    """count_batch, scan_count_batch and scan_batch against the oracle's per-pool results, and the route each call reports"""
    for mode in modes:
        p = fam.p[_kind(mode)]
        counts, sums, tuples = fam.ref("scan", mode)
        c, s = p.scan_count_batch(mode, batch)
        _eq((c, s), (counts[idx], sums[idx]), (what, mode, "scan_count_batch"))
        _route(mode, len(idx), long_docs)
        _eq((p.count_batch(mode, batch),), (counts[idx],), (what, mode, "count_batch"))
        _route(mode, len(idx), long_docs)
        got, offs = p.scan_batch(mode, batch)
        _route(mode, len(idx), long_docs)
        want = bs.expand(tuples, idx)
        _eq((offs,) + _tuples(got), want, (what, mode, "scan_batch"))
        assert int(offs[-1]) == int(counts[idx].sum())


def _check_histogram(fam, idx, batch, what, modes=MODES):
    rows = 0
    for mode in modes:
        got, offs = fam.p[_kind(mode)].histogram_batch(mode, batch)
        w_off, slot, count = bs.expand(fam.ref("hist", mode), idx)
        assert got.dtype == da.SLOT_COUNT_DTYPE
        _eq((offs, got["slot"], got["count"]), (w_off, slot, count), (what, mode, "histogram_batch"))
        assert da.last_kernel().startswith("batch_hist ") and _lk("records") == int(count.astype(np.int64).sum()), da.last_kernel()
        assert _lk("wave_docs") + _lk("group_docs") + _lk("dense_docs") == len(idx), da.last_kernel()
        rows = max(rows, len(slot))
    return rows


def _table(fam):
    return [b"<%d>" % i for i in range(fam.n_pat)]


def _check_replace(fam, idx, batch, what, modes=CHAIN_MODES):
    for mode in modes:
        p = fam.p[_kind(mode)]
        w_off, w_out = bs.expand(fam.ref("replace", mode, tuple(_table(fam))), idx)
        dm, do = p.replace_all_batch(batch, _table(fam), mode=mode, device=True)
        try:
            k = int(fam.ref("matches", mode)[idx].sum())
            assert dm.n_replaced == k and da.last_kernel().startswith(f"replace matches={k} out={len(w_out)} "), da.last_kernel()
            _eq((do.to_numpy(), dm.to_numpy()), (w_off, w_out), (what, mode, "replace_all_batch"))
        finally:
            dm.free()
            do.free()


def _check_tokenize(fam, idx, batch, what, modes=CHAIN_MODES, gaps=(Gap.Unk, Gap.Chars)):
    for mode in modes:
        p = fam.p[_kind(mode)]
        k = int(fam.ref("matches", mode)[idx].sum())
        for gap in gaps:
            w_off, w_ids, w_sp = bs.expand(fam.ref("tokenize", mode, gap, GID), idx)
            ids, sp, off = p.tokenize_batch(batch, gap=gap, gap_id=GID, spans=True, mode=mode)
            assert da.last_kernel().startswith(f"tokenize matches={k} tokens={len(w_ids)} "), da.last_kernel()
            _eq((off, ids, sp), (w_off, w_ids, w_sp), (what, mode, gap, "tokenize_batch"))
            ids, off = p.tokenize_batch(batch, gap=gap, gap_id=GID, mode=mode)
            _eq((off, ids), (w_off, w_ids), (what, mode, gap, "tokenize_batch without spans"))


def _check_bpe(fam, idx, batch, what):
    p = fam.p[0]
    k = int(fam.ref("matches", ScanMode.FindOverlapping)[idx].sum())
    for ranks, gap in ((None, Gap.Bytes), (_ranks(fam.n_pat), Gap.Chars)):
        want = bs.expand(fam.ref("bpe", ranks, gap, GID), idx)
        ids, sp, off = p.tokenize_bpe_batch(batch, ranks, gap=gap, gap_id=GID, spans=True)
        assert da.last_kernel().startswith(f"bpe docs={len(idx)} matches={k} tokens={len(want[1])} "), da.last_kernel()
        _eq((off, ids, sp), want, (what, gap, "tokenize_bpe_batch"))
        ids, off = p.tokenize_bpe_batch(batch, ranks, gap=gap, gap_id=GID)
        _eq((off, ids), want[:2], (what, gap, "tokenize_bpe_batch without spans"))


def _check_unigram(fam, idx, batch, what):
    p = fam.p[0]
    k = int(fam.ref("matches", ScanMode.FindOverlapping)[idx].sum())
    for gap in (Gap.Chars, Gap.Bytes):
        toks, sc = fam.ref("unigram", _scores(fam.n_pat), -2.5, gap, GID)
        want = bs.expand(toks, idx)
        ids, sp, off, ds = p.tokenize_unigram_batch(batch, _scores(fam.n_pat), -2.5, gap=gap, gap_id=GID, spans=True, doc_scores=True)
        assert da.last_kernel().startswith(f"unigram docs={len(idx)} matches={k} tokens={len(want[1])} "), da.last_kernel()
        _eq((off, ids, sp), want, (what, gap, "tokenize_unigram_batch"))
        assert ds.dtype == np.float32 and np.array_equal(_bits(ds), _bits(sc[idx])), (what, gap, "document scores")


def _is_utf8(d):
    try:
        d.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _word_pool(charwise=False):
    """the words of part A and C; a charwise automaton reads UTF-8 only (its documents are UTF-8 each on their own)"""
    pool = bs.make_pool(bs.WORD_HAND, bs.WORD_LETTERS, 64, 4, keep=_is_utf8 if charwise else None)
    return pool, (np.arange(len(pool)) % 5 == 3).astype(np.uint8)


def _check_wordpiece(model, pool, skip_pool, idx, batch, what):
    p, first, cont, vocab = model
    o = orc.OraclePma.build(da.wordpiece_tables(VOCAB)[0])   # the pieces' automaton: the call's scan counts every word, skipped or not
    k = int(bs.ref_matches(o, ScanMode.FindOverlapping, pool)[idx].sum())
    for skip in (skip_pool, None):
        want = bs.expand(bs.ref_wordpiece(pool, vocab, 0, 6, skip), idx)
        flags = None if skip is None else skip[idx]
        ids, sp, off = p.tokenize_wordpiece_batch(batch, first, cont, 0, 6, skip=flags, spans=True)
        assert da.last_kernel().startswith(f"wordpiece docs={len(idx)} matches={k} tokens={len(want[1])} "), da.last_kernel()
        _eq((off, ids, sp), want, (what, skip is not None, "tokenize_wordpiece_batch"))


def _check_normalize(world, per_pool, idx, n_bytes, batch, what):
    """normalize_batch with and without src against the scanner's per-pool results (offsets, bytes, src)"""
    nz, _ = world.normalizer()
    w_off, w_out, w_src = bs.expand(per_pool, idx)
    out, off, src = nz.normalize_batch(batch, src=True)
    assert da.last_kernel().startswith("normalize rules=") and (_lk("docs"), _lk("bytes"), _lk("out")) == (len(idx), n_bytes, len(w_out)), da.last_kernel()
    _eq((off, out, src), (w_off, w_out, w_src), (what, "normalize_batch with src"))
    out, off = nz.normalize_batch(batch)
    _eq((off, out), (w_off, w_out), (what, "normalize_batch"))


def _norm_pool():
    return bs.make_pool(bs.NORM_HAND, bs.NORM_LETTERS, 64, 7)


# --------------------------------------------------------------------------------------------------------- A. the chunked sum
def _batches(pool, idx, hay, off, **kw):
    """the batch as a host list and as a device batch whose offsets[0] is not 0"""
    return (("host", [pool[i] for i in idx.tolist()]), ("device", _device(hay, off, **kw)))


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("n", A_SIZES)
def test_a_scans(world, n, charwise):
    fam = world.family(charwise)
    idx, hay, off = bs.pooled(fam.pool, n, 100 + n, pins=fam.pins(), turns=(8192,))
    for src, batch in _batches(fam.pool, idx, hay, off, tail=fam.tail):
        _check_scans(fam, idx, batch, (n, src))


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("n", A_SIZES)
def test_a_histogram(world, n, charwise):
    fam = world.family(charwise)
    idx, hay, off = bs.pooled(fam.pool, n, 200 + n, pins=fam.pins(), turns=(8192,))
    for src, batch in _batches(fam.pool, idx, hay, off, tail=fam.tail):
        _check_histogram(fam, idx, batch, (n, src))


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("n", A_SIZES)
def test_a_replace_and_tokenize(world, n, charwise):
    fam = world.family(charwise)
    idx, hay, off = bs.pooled(fam.pool, n, 300 + n, pins=fam.pins(), turns=(8192,))
    for src, batch in _batches(fam.pool, idx, hay, off, tail=fam.tail):
        _check_replace(fam, idx, batch, (n, src))
        _check_tokenize(fam, idx, batch, (n, src))


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("n", A_SIZES)
def test_a_bpe_and_unigram(world, n, charwise):
    fam = world.family(charwise)
    idx, hay, off = bs.pooled(fam.pool, n, 400 + n, pins=fam.pins(), turns=(8192,))
    for src, batch in _batches(fam.pool, idx, hay, off, tail=fam.tail):
        _check_bpe(fam, idx, batch, (n, src))
        _check_unigram(fam, idx, batch, (n, src))


@pytest.mark.parametrize("charwise", [False, True])
@pytest.mark.parametrize("n", A_SIZES)
def test_a_wordpiece(world, n, charwise):
    pool, skip_pool = _word_pool(charwise)
    idx, hay, off = bs.pooled(pool, n, 500 + n, pins=[2, 4, 5, 7, 9], turns=(8192,))
    for src, batch in _batches(pool, idx, hay, off, front=b"un", tail=b"s"):
        _check_wordpiece(world.wordpiece(charwise), pool, skip_pool, idx, batch, (n, src))


NORM_TILE = 1024   # kNormTile


def _norm_batch(tiles, seed):
    """normalize_batch sums one count per tile of kNormTile bytes of text, not per document: a batch of exactly `tiles` tiles, the
    last one five bytes short.  Documents of about 1 KiB join the pool, and one filler document brings the total to the byte.
    -> (pool, idx)"""
    rng = np.random.default_rng(seed)
    letters = [bs.NORM_LETTERS[i] for i in range(len(bs.NORM_LETTERS))]
    pool = _norm_pool() + [b"".join(letters[i] for i in rng.integers(0, len(letters), 500).tolist()) + b"%d" % j for j in range(8)]
    target = tiles * NORM_TILE - 5
    lens = np.array([len(d) for d in pool])
    draw = np.where(rng.random(3 * tiles) < 0.25, rng.integers(0, 64, 3 * tiles), rng.integers(64, len(pool), 3 * tiles))
    keep = int(np.searchsorted(np.cumsum(lens[draw]), target - 3000))
    fill = target - int(lens[draw[:keep]].sum())
    assert 3000 <= fill < 6000
    filler = ("Ab\u00c9 \u4e2d\ud55c\0" * fill).encode()[:fill - 1] + b"Z"
    return pool + [filler], np.concatenate([draw[:keep // 2], [len(pool)], draw[keep // 2:keep]]).astype(np.int64)


@pytest.mark.parametrize("tiles", A_SIZES)
def test_a_normalize(world, tiles):
    """the scanned array has one entry per tile: 8191 and 8192 tiles are summed by one workgroup, 8193 and 12289 in three launches"""
    pool, idx = _norm_batch(tiles, 600 + tiles)
    hay, off = bs.pack_idx(pool, idx)
    assert -(-len(hay) // NORM_TILE) == tiles and len(hay) % NORM_TILE
    per_pool = bs.ref_normalize(pool, world.normalizer()[1])
    for src, batch in _batches(pool, idx, hay, off, front=b"\xe4\xb8", tail=b"\xad"):
        _check_normalize(world, per_pool, idx, len(hay), batch, (tiles, src))
        assert f"tile={NORM_TILE}" in da.last_kernel(), da.last_kernel()


# ------------------------------------------------------------------------------------------------------ B. the second turn
def _big(world, key, pool, pins, seed, **kw):
    """the pooled batch of N_BIG documents on the device, built once: (idx, host offsets, device batch)"""
    def make():
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert N_BIG > 4096 * 256 and N_BIG > 2048 * cu, (N_BIG, cu)
        idx, hay, off = bs.pooled(pool, N_BIG, seed, pins=pins)
        assert len({int(idx[a]) for a in bs.marks(N_BIG)}) == 5 and bs.marks(N_BIG) == [0, bs.TURN - 1, bs.TURN, bs.TURN + 1, N_BIG - 1]
        return idx, off, _device(hay, off, **kw)
    return world.get(("big", key), make)


@pytest.mark.parametrize("which", ["bytewise", "charwise", "empty pattern"])
def test_b_scans_of_more_documents_than_one_turn(world, which):
    """batch_plan, batch_reduce, batch_doc_offsets (grid_for(.., 256, 4096): a second turn above 1 048 576 documents), the piece kernel
    (launch_batch_pieces: num_cu * bpc blocks) and both chain kernels (launch_batch_chain: num_cu * 8 blocks of 256 lanes); with "" among
    the patterns leftmost_empty_doc on the second turn"""
    fam = world.family(which == "charwise", which == "empty pattern")
    idx, _, batch = _big(world, which, fam.pool, fam.pins(), 21, tail=fam.tail)
    _check_scans(fam, idx, batch, which)


def test_b_histogram_rows(world):
    """batch_hist_classify (4096 x 256) past 2^20 documents and batch_hist_copy (8192 x 256) past 2^21 rows"""
    fam = world.family()
    idx, _, batch = _big(world, "bytewise", fam.pool, fam.pins(), 21, tail=fam.tail)
    assert _check_histogram(fam, idx, batch, "histogram") > 1 << 21


def test_b_replace(world):
    """replace_size and replace_finish (8192 x 256) past 2^21 matches, replace_doc_offsets (4096 x 256) past 2^20 documents"""
    fam = world.family()
    idx, _, batch = _big(world, "bytewise", fam.pool, fam.pins(), 21, tail=fam.tail)
    assert int(fam.ref("matches", ScanMode.Find)[idx].sum()) > 1 << 21
    _check_replace(fam, idx, batch, "replace")


def test_b_tokenize(world):
    """tokenize_prep (8192 x 256) past 2^21 matches"""
    fam = world.family()
    idx, _, batch = _big(world, "bytewise", fam.pool, fam.pins(), 21, tail=fam.tail)
    assert int(fam.ref("matches", ScanMode.Find)[idx].sum()) > 1 << 21
    _check_tokenize(fam, idx, batch, "tokenize", gaps=(Gap.Unk,))


def _text_batch(world):
    pool = world.text_pool()
    return (pool,) + _big(world, "text", pool, [3, 4, 5, 6, 7], 22, front=b"\xe6\xbc", tail=b"\xa2's")


@pytest.mark.parametrize("rule", RULES)
def test_b_split_of_more_documents_and_words_than_one_turn(world, rule):
    """split_mark and split_docs (split_grid(.., 256, 4096)) past 2^20 documents, both split_words_space kernels and offsets_compose
    past 2^20 words"""
    pool, idx, off, batch = _text_batch(world)
    base = int(batch[1][0])
    w_wo, w_dw, w_space = bs.expand_split(world.get(("ref_split", rule), lambda: bs.ref_split(pool, rule)), idx, off + base)
    assert len(w_space) > 1 << 20
    sp = da.Splitter(rule, da.bert_char_classes() if rule == Split.Bert else None)
    wo, dw = sp.split_batch(batch, device=True)
    try:
        assert _lk("words") == len(w_space) and _lk("docs") == N_BIG, da.last_kernel()
        _eq((wo.to_numpy(), dw.to_numpy()), (w_wo, w_dw), (rule, "split_batch"))
        _eq((sp.words_space((batch[0], wo)),), (w_space,), (rule, "words_space"))
        _eq((da.offsets_compose(wo, dw),), ((off + base).astype(np.uint64),), (rule, "offsets_compose: word_offsets[doc_words] are the document offsets"))
    finally:
        wo.free()
        dw.free()
        sp.free()


def test_b_bpe_docs(world):
    """spans_rebase and offsets_compose (4096 x 256) past 2^20 words behind the split"""
    pool, idx, off, batch = _text_batch(world)
    fam = world.family()
    want = bs.expand(bs.ref_bpe_docs(fam.o[0], pool, Split.Gpt2, None, Gap.Chars, GID), idx)
    n_words = len(bs.expand(world.get(("ref_split", Split.Gpt2), lambda: bs.ref_split(pool, Split.Gpt2)), idx)[1])
    assert n_words > 1 << 20 and len(want[1]) > 1 << 20
    ids, sp, doc_tok = fam.p[0].tokenize_bpe_docs(batch, split=Split.Gpt2, gap=Gap.Chars, gap_id=GID, spans=True)
    assert da.last_kernel().startswith(f"bpe docs={n_words} ") and _lk("tokens") == len(want[1]), da.last_kernel()   # (a word is a document of the inner call)
    _eq((doc_tok, ids, sp), want, "tokenize_bpe_docs")


def test_b_wordpiece_docs_behind_the_normalizer(world):
    """normalize_docs (4096 x 256) past 2^20 documents, spans_rebase past 2^20 words and spans_to_source past 2^20 tokens.
    (normalize_longest is launched only for 4 GiB of text and more: not here.)"""
    pool, idx, off, batch = _text_batch(world)
    p, first, cont, vocab = world.wordpiece()
    nz, image = world.normalizer()
    want = bs.expand(bs.ref_wordpiece_docs(pool, vocab, 0, 6, image), idx)
    normalized = [ng.scan(bs._b(d), image)[0] for d in pool]   # the words of the inner call: Split.Bert's over the normalized text
    n_words = len(bs.expand(bs.ref_split(normalized, Split.Bert), idx)[1])
    assert n_words > 1 << 20 and len(want[1]) > 1 << 20
    ids, sp, doc_tok = p.tokenize_wordpiece_docs(batch, first, cont, 0, 6, spans=True, normalizer=nz)
    assert da.last_kernel().startswith(f"wordpiece docs={n_words} ") and _lk("tokens") == len(want[1]), da.last_kernel()
    _eq((doc_tok, ids, sp), want, "tokenize_wordpiece_docs")


def _unigram_text(fam):
    def text(seg):
        toks, _ = _viterbi(seg, fam.o[0].find_overlapping_iter(seg), _scores(fam.n_pat), np.float32(-2.5), Gap.Chars, GID)
        return bs._triples(toks)
    return text


def _tokenize_text(fam):
    from test_gpu_tokenize import _tokens

    def text(seg):
        ids, spans = _tokens(seg, fam.o[1].leftmost_find_iter(seg), Gap.Unk, GID)
        return ids.tolist(), [tuple(x) for x in spans.tolist()]
    return text


def test_b_splice_of_more_segments_than_one_turn(world):
    """splice_write_kernel takes a wave per segment on at most kCutMaxBlocks = 65536 blocks of 4 waves (cut_kernels.hip
    launch_splice_write): a second turn above 262 144 segments.  150 000 documents, most of them text, a special, text."""
    fam = world.family()
    st = world.special()
    pool = bs.make_pool([b"", b"a<|e|>b", b"ab<|e|>c", "é<|end|>bc".encode(), b"xyz", b"<|e|>", b"<|end|>", b"abc", b"<|e|><|e|>"], bs.SPECIAL_LETTERS, 24, 8)
    rng = np.random.default_rng(23)
    idx = np.concatenate([rng.integers(1, 4, 142_000), rng.integers(0, len(pool), 8_000)])
    rng.shuffle(idx)
    per_pool = bs.ref_cut(pool, SPEC)
    turn = 65536 * 4
    at = int(np.searchsorted(bs.expand(per_pool, idx)[0], turn, side="right")) - 1   # the document that holds segment 262 144
    idx[at - 2:at + 3] = [1, 2, 3, 1, 2]   # five documents of three segments around the kernel's turn boundary, neighbours differ
    hay, off = bs.pack_idx(pool, idx)
    batch = _device(hay, off, front=b"<|e", tail=b"|>")
    base = int(batch[1][0])
    w_so, w_ds, w_sv = bs.expand_cut(per_pool, idx, off + base)
    n_segs = len(w_sv)
    assert n_segs > turn and (idx == 0).sum() and (idx == 5).sum() and (idx == 4).sum()
    assert w_ds[at - 2] <= turn - 3 and turn + 3 <= w_ds[at + 3], "three-segment documents lie on either side of segment 262 144"
    cut = st.cut_batch(batch, device=True)
    try:
        n_special = int((w_sv != sg.TEXT).sum())
        assert da.last_kernel().startswith(f"cut docs={len(idx)} matches={n_special} segs={n_segs} ") and cut[2].n_special == n_special, da.last_kernel()
        _eq([c.to_numpy() for c in cut], (w_so, w_ds, w_sv), "cut_batch")
        ids, spans, seg_tok = fam.p[1].tokenize_batch((batch[0], cut[0]), gap=Gap.Unk, gap_id=GID, spans=True, mode=ScanMode.LeftmostFind, device=True)
        try:
            want = bs.expand(bs._tok_csr(bs._per_doc(pool, _tokenize_text(fam), SPEC)), idx)
            got = da.splice_special(ids, spans, seg_tok, cut, batch)
            assert da.last_kernel().startswith(f"splice docs={len(idx)} segs={n_segs} tokens={len(want[1])}"), da.last_kernel()
            _eq((got[2], got[0], got[1]), want, "splice_special behind tokenize_batch")
        finally:
            for x in (ids, spans, seg_tok):
                x.free()
    finally:
        for c in cut:
            c.free()
    want = bs.expand(bs.ref_bpe_docs(fam.o[0], pool, Split.Gpt2, None, Gap.Bytes, GID, SPEC), idx)
    ids, sp, doc_tok = fam.p[0].tokenize_bpe_docs(batch, split=Split.Gpt2, gap=Gap.Bytes, gap_id=GID, spans=True, special=st)
    _eq((doc_tok, ids, sp), want, "tokenize_bpe_docs with special tokens")


# ---------------------------------------------------------------------------------- C. positions across and above 2^32
@pytest.fixture(scope="module")
def big():
    t = torch.empty(P32 + (64 << 20), dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()


def _mixed(pool, unit, ok, seed, min_len=0, half=150):
    """A mixed batch over pool + [middle]: two empty documents, `half` pool documents, an empty one, the middle document, an empty one,
    the same pool documents in another order, an empty one.  The halves hold the same bytes, so the middle of the batch lies in the
    middle document: copies of `unit`, as many as make `ok(position in the unit)` true 5 bytes in front of the batch's middle, where
    the first base of part C puts position 2^32.  -> (pool + [middle], idx)"""
    rng = np.random.default_rng(seed)
    front = rng.integers(1, len(pool), half)
    size = len(bs._b(unit))
    reps = max(8, -(-min_len // size))
    while not ok((size * reps // 2 - 5) % size) or size * reps % 2:
        reps += 1
        assert reps < 4096, "no number of copies puts the middle inside the unit as asked"
    idx = np.concatenate([[0, 0], front, [0, len(pool), 0], rng.permutation(front), [0]]).astype(np.int64)
    return list(pool) + [unit * reps], idx


def _bases(total):
    return (P32 - total // 2 + 5, P32 + (1 << 25) + 3)


def _window(big, pool, idx, which, **kw):
    """the mixed batch at base number `which` -> (host offsets from 0, base, device batch); at the first base the window contains
    position 2^32, inside the middle document, and the byte there is a continuation byte or lies inside the unit"""
    hay, off = bs.pack_idx(pool, idx)
    total = int(off[-1])
    assert total <= 1 << 20 and bs._b(pool[int(idx[0])]) == b"" and bs._b(pool[int(idx[-1])]) == b""
    base = _bases(total)[which]
    assert base % 16 != 0
    if which == 0:
        mid = int(np.nonzero(idx == len(pool) - 1)[0][0])
        assert base < P32 < base + total and base + off[mid] < P32 < base + off[mid + 1], "the middle document lies across 2^32"
    else:
        assert base > P32
    return off, base, bs.high_window(big, (hay, off), base, **kw)


def _inside_a_character_of(unit):
    """positions of `unit` that are neither its start nor the start of one of its characters"""
    u = bs._b(unit)
    return lambda r: r != 0 and (u[r] & 0xC0) == 0x80


def _c_family(world, charwise):
    def make():
        unit = "世界"
        fam = _Family(charwise)
        pool, idx = _mixed(fam.pool, unit if charwise else unit.encode(), _inside_a_character_of(unit), 31, min_len=LANE_MAX + 1)
        fam.pool = pool
        for p in fam.p.values():
            p.set_option("batch_lane_max", LANE_MAX)
        return fam, idx
    return world.get(("c family", charwise), make)


@pytest.mark.parametrize("which", [0, 1], ids=["across 2^32", "above 2^32"])
@pytest.mark.parametrize("charwise", [False, True])
def test_c_scans_histogram_replace_and_tokenize(world, big, charwise, which):
    """count_batch, scan_count_batch, scan_batch, histogram_batch, replace_all_batch and tokenize_batch; the middle document, a run of
    one pattern of two three-byte characters, is longer than batch_lane_max and takes the long route of api_batch.hip"""
    fam, idx = _c_family(world, charwise)
    off, base, batch = _window(big, fam.pool, idx, which, front="世".encode()[:2], tail=fam.tail)
    _check_scans(fam, idx, batch, (charwise, which), long_docs=1)
    _check_histogram(fam, idx, batch, (charwise, which), modes=MODES[:2])
    for p in fam.p.values():   # (histogram_batch refuses a document above batch_lane_max in the chain modes: the default serves it)
        p.set_option("batch_lane_max")
    try:
        _check_histogram(fam, idx, batch, (charwise, which), modes=CHAIN_MODES)
    finally:
        for p in fam.p.values():
            p.set_option("batch_lane_max", LANE_MAX)
    _check_replace(fam, idx, batch, (charwise, which))
    assert _lk("long_docs") == 1, da.last_kernel()
    _check_tokenize(fam, idx, batch, (charwise, which))
    assert _lk("long_docs") == 1, da.last_kernel()


@pytest.mark.parametrize("which", [0, 1], ids=["across 2^32", "above 2^32"])
@pytest.mark.parametrize("charwise", [False, True])
def test_c_bpe_unigram_and_wordpiece(world, big, charwise, which):
    def make():
        unit = "世界"
        fam = _Family(charwise)
        fam.pool, idx = _mixed(fam.pool, unit if charwise else unit.encode(), _inside_a_character_of(unit), 32)
        return fam, idx
    fam, idx = world.get(("c tokenizers", charwise), make)
    off, base, batch = _window(big, fam.pool, idx, which, front="世".encode()[:2], tail=fam.tail)
    _check_bpe(fam, idx, batch, (charwise, which))
    _check_unigram(fam, idx, batch, (charwise, which))
    words, skip_pool = _word_pool(charwise)
    pool, idx = world.get(("c words", charwise), lambda: _mixed(words, "aé、".encode(), _inside_a_character_of("aé、"), 33))
    off, base, batch = _window(big, pool, idx, which, front=b"un", tail=b"s")
    _check_wordpiece(world.wordpiece(charwise), pool, np.append(skip_pool, 0).astype(np.uint8), idx, batch, (charwise, which))


@pytest.mark.parametrize("which", [0, 1], ids=["across 2^32", "above 2^32"])
def test_c_split_words_space_compose_and_normalize(world, big, which):
    """word_offsets are absolute: the scanner's plus the base; split_docs_kernel's p % kSplitTile and the tiles' positions at 2^32"""
    unit = "é漢 'll"
    pool, idx = world.get("c text", lambda: _mixed(world.text_pool(), unit.encode(), _inside_a_character_of(unit), 34))
    off, base, batch = _window(big, pool, idx, which, front=b"\xe6\xbc", tail=b"\xa2's")
    for rule in RULES + (Split.Llama3,):
        w_wo, w_dw, w_space = bs.expand_split(world.get(("c ref_split", rule), lambda: bs.ref_split(pool, rule)), idx, off + base)
        sp = da.Splitter(rule, da.bert_char_classes() if rule == Split.Bert else None)
        wo, dw = sp.split_batch(batch, device=True)
        try:
            _eq((wo.to_numpy(), dw.to_numpy()), (w_wo, w_dw), (rule, which, "split_batch"))
            assert which or (w_wo < P32).any() and (w_wo > P32).any()
            _eq((sp.words_space((batch[0], wo)),), (w_space,), (rule, which, "words_space"))
            _eq((da.offsets_compose(wo, dw),), ((off + base).astype(np.uint64),), (rule, which, "offsets_compose"))
        finally:
            wo.free()
            dw.free()
            sp.free()
    unit = "É中한"
    pool, idx = world.get("c norm", lambda: _mixed(_norm_pool(), unit.encode(), _inside_a_character_of(unit), 35))
    off, base, batch = _window(big, pool, idx, which, front=b"\xe4\xb8", tail=b"\xad")
    nz, image = world.normalizer()
    w_off, w_out, w_src = bs.expand(world.get("c ref_normalize", lambda: bs.ref_normalize(pool, image)), idx)
    out, o_off, src = nz.normalize_batch(batch, src=True)
    _eq((o_off, out, src), (w_off, w_out, w_src), (which, "normalize_batch with src"))


@pytest.mark.parametrize("which", [0, 1], ids=["across 2^32", "above 2^32"])
def test_c_cut_and_the_chains_around_special_tokens(world, big, which):
    """seg_offsets are absolute; cut_batch -> tokenize_unigram_batch -> splice_special and the *_docs chains pass their DeviceOffsets on
    without a host step.  At the first base a special token lies across 2^32 (and, in the second batch, a three-byte character)."""
    fam = world.family()
    st = world.special()
    base_pool = world.get("c special pool", lambda: bs.make_pool(bs.SPECIAL_HAND + bs.TEXT_HAND[1:], bs.SPECIAL_LETTERS + bs.TEXT_LETTERS, 96, 12, max_letters=8))
    for unit, ok, tag in ((b"a<|e|>", lambda r: 2 <= r <= 5, "special"), ("世<|end|> una".encode(), lambda r: r in (1, 2), "character")):
        pool, idx = world.get(("c special", tag), lambda: _mixed(base_pool, unit, ok, 36))
        off, base, batch = _window(big, pool, idx, which, front=b"<|e", tail=b"|>")
        w_so, w_ds, w_sv = bs.expand_cut(world.get(("c ref_cut", tag), lambda: bs.ref_cut(pool, SPEC)), idx, off + base)
        cut = st.cut_batch(batch, device=True)
        try:
            _eq([c.to_numpy() for c in cut], (w_so, w_ds, w_sv), (tag, which, "cut_batch"))
            assert which or (w_so < P32).any() and (w_so > P32).any()
            ids, spans, seg_tok, ds = fam.p[0].tokenize_unigram_batch((batch[0], cut[0]), _scores(fam.n_pat), -2.5, gap=Gap.Chars, gap_id=GID, spans=True,
                                                                      doc_scores=True, device=True)
            try:
                want = bs.expand(world.get(("c ref_unigram_docs", tag), lambda: bs._tok_csr(bs._per_doc(pool, _unigram_text(fam), SPEC))), idx)
                got = da.splice_special(ids, spans, seg_tok, cut, batch)
                _eq((got[2], got[0], got[1]), want, (tag, which, "cut_batch -> tokenize_unigram_batch -> splice_special"))
            finally:
                for x in (ids, spans, seg_tok, ds):
                    x.free()
        finally:
            for c in cut:
                c.free()
        want = bs.expand(world.get(("c ref_bpe_docs", tag), lambda: bs.ref_bpe_docs(fam.o[0], pool, Split.Gpt2, None, Gap.Bytes, GID, SPEC)), idx)
        ids, sp, doc_tok = fam.p[0].tokenize_bpe_docs(batch, split=Split.Gpt2, gap=Gap.Bytes, gap_id=GID, spans=True, special=st)
        _eq((doc_tok, ids, sp), want, (tag, which, "tokenize_bpe_docs with special tokens"))
        p, first, cont, vocab = world.wordpiece()
        nz, image = world.normalizer()
        want = bs.expand(world.get(("c ref_wordpiece_docs", tag), lambda: bs.ref_wordpiece_docs(pool, vocab, 0, 6, image, SPEC)), idx)
        ids, sp, doc_tok = p.tokenize_wordpiece_docs(batch, first, cont, 0, 6, spans=True, normalizer=nz, special=st)
        _eq((doc_tok, ids, sp), want, (tag, which, "tokenize_wordpiece_docs with the normalizer and special tokens"))
