"""tokenize_bpe, tokenize_bpe_docs, split_batch and tokenize_unigram on the MI355X against `tokenizers` and sentencepiece: a trained
byte-level BPE vocabulary (all 256 bytes, merges whose rank order is the merge order) and a trained unigram model (float scores of an
EM fit, pieces in several scripts) over a few hundred noisy documents.  The expected ids and word boundaries are the libraries' own,
read from tests/golden/tokenizer_*.json (tests/golden/make_tokenizer_golden.py writes them and tests/test_tokenizer_golden_host.py ties
them to the references of the neighbouring GPU suites); nothing here reads the libraries.  Every comparison is exact but one, the
document score, whose bound is derived where it is used.

The mapping from each model family to this library's calls is the one README gives:
  byte-level BPE     patterns = the pieces' bytes, value = id = rank, Gap.Bytes, the text split into words first (Split.Gpt2);
  sentencepiece      "▁" for every space on the caller's side, value = id, every piece but <unk>, unk_score = min score - 10,
                     Gap.Chars with gap_id = unk_id; sentencepiece reports a run of unknown code points once, this library once per
                     code point, and the caller (here: collapse) joins them."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
import tokenizer_golden as tg

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap, Split

GID = 1 << 20   # above every id: every byte is in the BPE vocabulary, so no token may reach it
ENGINES = (Engine.Auto, Engine.DArray)


def _pair(patterns, values):
    o = orc.OraclePma.build(patterns, values=values)
    p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return p


def _device_batch(docs, front):
    """(hay, offsets) on the device; `front` bytes that belong to no document come first, so offsets[0] != 0"""
    off = np.full(len(docs) + 1, front, dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(b"\xe6" * front + b"".join(docs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _dev(hay):
    return torch.from_numpy(np.frombuffer(hay, dtype=np.uint8).copy()).cuda()


def _forms(docs, front=7):
    """a batch as a host list and as a device batch with offsets[0] != 0"""
    return (("host", docs), ("device", _device_batch(docs, front)))


def _per_doc(off, *arrays):
    off = off.tolist()
    return [tuple(a[s:e].tolist() for a in arrays) for s, e in zip(off, off[1:])]


def _tiles(spans, length):
    return [s for s, _ in spans] + [length] == [0] + [e for _, e in spans] if spans else length == 0


@pytest.fixture(scope="module")
def bpe():
    pieces = tg.bpe_pieces()
    return _pair(pieces, np.arange(len(pieces), dtype=np.uint32))


@pytest.fixture(scope="module")
def bpe_permuted():
    """the same vocabulary with value = pi(id) and ranks[pi(id)] = id -> (automaton, ranks, pi^-1)"""
    pieces = tg.bpe_pieces()
    pi, ranks = tg.permutation(len(pieces))
    return _pair(pieces, pi), ranks, np.argsort(pi)


@pytest.fixture(scope="module")
def unigram():
    pats, values, scores, unk_id, unk_score = tg.unigram_model()
    return _pair(pats, values), scores, unk_id, unk_score


# ------------------------------------------------------------------------------------------------------------------ BPE, words
def _check_words(p, words, want_ids, ranks=None, back=None, what=None):
    pieces = tg.bpe_pieces()
    for eng in ENGINES:
        for src, arg in _forms(words):
            ids, sp, off = p.tokenize_bpe_batch(arg, ranks, gap=Gap.Bytes, gap_id=GID, spans=True, engine=eng)
            assert ids.dtype == np.uint32 and sp.dtype == np.uint64 and off.dtype == np.uint64 and len(off) == len(words) + 1, (what, eng, src)
            if back is not None:
                assert ids.max() < len(back)
                ids = back[ids]
            assert len(ids) == 0 or ids.max() < GID, (what, eng, src)
            for w, want, (got, spans) in zip(words, want_ids, _per_doc(off, ids, sp)):
                assert got == want, (what, eng, src, w)
                assert _tiles(spans, len(w)) and [w[s:e] for s, e in spans] == [pieces[i] for i in want], (what, eng, src, w)
            ids2, off2 = p.tokenize_bpe_batch(arg, ranks, gap=Gap.Bytes, gap_id=GID, engine=eng)
            assert np.array_equal(ids2 if back is None else back[ids2], ids) and np.array_equal(off2, off), (what, eng, src)


def test_bpe_all_distinct_words_equal_tokenizers(bpe):
    words, word_ids = tg.bpe_words()
    assert len(words) > 600 and max(map(len, words)) > 16
    _check_words(bpe, words, word_ids, what="value = id = rank")


def test_bpe_rank_table_over_permuted_values_equals_tokenizers(bpe_permuted):
    p, ranks, back = bpe_permuted
    words, word_ids = tg.bpe_words()
    _check_words(p, words, word_ids, ranks, back, what="ranks[pi(id)] = id")


@pytest.mark.parametrize("n", tg.BATCH_SIZES)
def test_bpe_word_batches_at_wave_and_workgroup_edges(bpe, n):
    words, word_ids = tg.bpe_words()
    _check_words(bpe, words[:n], word_ids[:n], what=n)


# --------------------------------------------------------------------------------------------------- BPE, documents end to end
def test_bpe_docs_behind_the_gpt2_split_equal_tokenizers(bpe):
    c = tg.load("bpe_cases")
    pieces = tg.bpe_pieces()
    docs = [d.encode() for d in c["docs"]]
    empty = [i for i, d in enumerate(docs) if not d]
    assert empty[-1] == len(docs) - 1 and 0 < empty[0] < len(docs) - 1   # an empty document in the middle and one at the end
    for eng in ENGINES:
        for src, arg in _forms(docs, front=11):
            ids, sp, off = bpe.tokenize_bpe_docs(arg, split=Split.Gpt2, gap_id=GID, spans=True, engine=eng)
            assert ids.dtype == np.uint32 and len(off) == len(docs) + 1 and off[0] == 0 and off[-1] == len(ids) and ids.max() < GID, (eng, src)
            for d, want, (got, spans) in zip(docs, c["ids"], _per_doc(off, ids, sp)):
                assert got == want, (eng, src, d)
                assert _tiles(spans, len(d)) and [d[s:e] for s, e in spans] == [pieces[i] for i in want], (eng, src, d)
            for i in empty:
                assert off[i] == off[i + 1]
            ids2, off2 = bpe.tokenize_bpe_docs(arg, split=Split.Gpt2, gap_id=GID, engine=eng)
            assert np.array_equal(ids2, ids) and np.array_equal(off2, off), (eng, src)


def test_split_batch_gives_tokenizers_words():
    c = tg.load("bpe_cases")
    docs = [d.encode() for d in c["docs"]]
    want_dw = np.cumsum([0] + [len(b) - 1 for b in c["word_bounds"]]).tolist()
    for front, arg in ((0, docs), (13, _device_batch(docs, 13))):
        want, at = [], front
        for d, bounds in zip(docs, c["word_bounds"]):
            want += [at + b for b in bounds[:-1]]
            at += len(d)
        wo, dw = da.split_batch(arg, Split.Gpt2)
        assert wo.dtype == np.uint64 and dw.dtype == np.uint64
        assert dw.tolist() == want_dw and wo.tolist() == want + [at], front
    sp = da.Splitter(Split.Gpt2)
    for d, bounds in list(zip(docs, c["word_bounds"]))[:40]:
        assert sp.split(d).tolist() == bounds, d


def test_bpe_single_haystack_on_three_words(bpe, bpe_permuted):
    """tokenize_bpe takes one piece of pre-split text: the three longest distinct words"""
    words, word_ids = tg.bpe_words()
    pieces = tg.bpe_pieces()
    p2, ranks, back = bpe_permuted
    for i in sorted(range(len(words)), key=lambda i: (-len(words[i]), words[i]))[:3]:
        for hay in (words[i], _dev(words[i])):
            for eng in ENGINES:
                ids, sp = bpe.tokenize_bpe(hay, gap=Gap.Bytes, gap_id=GID, spans=True, engine=eng)
                assert ids.tolist() == word_ids[i] and _tiles(sp.tolist(), len(words[i])), words[i]
                assert [words[i][s:e] for s, e in sp.tolist()] == [pieces[t] for t in word_ids[i]]
                assert bpe.tokenize_bpe(hay, gap=Gap.Bytes, gap_id=GID, engine=eng).tolist() == word_ids[i]
                assert back[p2.tokenize_bpe(hay, ranks, gap=Gap.Bytes, gap_id=GID, engine=eng)].tolist() == word_ids[i]


# -------------------------------------------------------------------------------------------------------------------- unigram
def _check_score(got, ids, scores, unk_id, unk_score, what):
    """The document score is best[L]: the float32 sums s_k = fl(s_{k-1} + x_k) along the path in text order, x_k the score of token k
    (unk_score for an unknown one), s_0 = 0.  Each of the T additions rounds to nearest, so it errs by at most half an ulp of its result,
    |s_k - (s_{k-1} + x_k)| <= 2^-24 |s_k|, and the errors add up to |s_T - sum x_k| <= T * 2^-24 * max_k |s_k|.  Every x_k is negative
    here, so the sums fall monotonically and max_k |s_k| = |s_T|, the device's own figure; the exact sum is taken in float64, whose own
    error (T * 2^-53 relative) is nine orders below the bound."""
    xs = np.array([unk_score if i == unk_id else scores[i] for i in ids], dtype=np.float64)
    assert (xs < 0).all()
    exact = float(xs.sum())
    bound = len(ids) * 2.0 ** -24 * max(abs(exact), abs(float(got)))
    assert abs(float(got) - exact) <= bound, (what, float(got), exact, bound)
    # and the definition's own statement, which is stronger: the very float32 chain, bit for bit
    s = np.float32(0.0)
    for x in xs.astype(np.float32):
        s = s + x
    assert np.float32(got).view(np.uint32) == s.view(np.uint32), (what, float(got), float(s))


def _check_unigram(model, texts, want_ids, what=None):
    p, scores, unk_id, unk_score = model
    pieces = tg.load("unigram_vocab")["pieces"]
    for eng in ENGINES:
        for src, arg in _forms(texts, front=5):
            ids, sp, off, sc = p.tokenize_unigram_batch(arg, scores, unk_score, gap=Gap.Chars, gap_id=unk_id, spans=True, doc_scores=True, engine=eng)
            assert ids.dtype == np.uint32 and sp.dtype == np.uint64 and off.dtype == np.uint64 and sc.dtype == np.float32, (what, eng, src)
            assert len(off) == len(texts) + 1 and len(sc) == len(texts) and off[-1] == len(ids)
            for k, (t, want, (got, spans)) in enumerate(zip(texts, want_ids, _per_doc(off, ids, sp))):
                assert tg.collapse(got, unk_id) == want, (what, eng, src, t)
                assert _tiles(spans, len(t)), (what, eng, src, t)
                for i, (s, e) in zip(got, spans):
                    if i != unk_id:
                        assert t[s:e] == pieces[i].encode(), (what, eng, src, t)
                    else:   # one code point, and one that is no piece
                        assert len(t[s:e].decode()) == 1 and t[s:e].decode() not in pieces, (what, eng, src, t)
                _check_score(sc[k], got, scores, unk_id, unk_score, (what, eng, src, t))
            ids2, off2 = p.tokenize_unigram_batch(arg, scores, unk_score, gap=Gap.Chars, gap_id=unk_id, engine=eng)
            assert np.array_equal(ids2, ids) and np.array_equal(off2, off), (what, eng, src)


def test_unigram_all_documents_equal_sentencepiece(unigram):
    c = tg.load("unigram_cases")
    texts = [tg.sp_text(d) for d in c["docs"]]
    empty = [i for i, t in enumerate(texts) if not t]
    assert empty[-1] == len(texts) - 1 and 0 < empty[0] < len(texts) - 1 and len(texts) >= 257
    _check_unigram(unigram, texts, c["ids"], what="all")


@pytest.mark.parametrize("n", tg.BATCH_SIZES)
def test_unigram_batches_at_wave_and_workgroup_edges(unigram, n):
    c = tg.load("unigram_cases")
    _check_unigram(unigram, [tg.sp_text(d) for d in c["docs"][:n]], c["ids"][:n], what=n)


def test_unigram_paths_of_equal_score_go_sentencepieces_way(unigram):
    """documents with several best segmentations (-|--|-- and --|--|-): sentencepiece keeps the first candidate it meets, the longest
    piece into a position, which is the first that find_overlapping_iter reports"""
    c = tg.load("unigram_cases")
    assert c["sensitivity"]["tie_docs_changed_by_shortest_first"] >= 3
    _check_unigram(unigram, [tg.sp_text(d) for d in c["tie_docs"]], c["tie_ids"], what="ties")


def test_unigram_single_haystack_on_three_documents(unigram):
    p, scores, unk_id, unk_score = unigram
    c = tg.load("unigram_cases")
    for i in sorted(range(len(c["docs"])), key=lambda i: (-len(c["docs"][i]), i))[:3]:
        t = tg.sp_text(c["docs"][i])
        for hay in (t, _dev(t)):
            for eng in ENGINES:
                ids, sp, score = p.tokenize_unigram(hay, scores, unk_score, gap=Gap.Chars, gap_id=unk_id, spans=True, engine=eng)
                assert tg.collapse(ids.tolist(), unk_id) == c["ids"][i] and _tiles(sp.tolist(), len(t)), t
                _check_score(score, ids.tolist(), scores, unk_id, unk_score, t)
                ids2, score2 = p.tokenize_unigram(hay, scores, unk_score, gap=Gap.Chars, gap_id=unk_id, engine=eng)
                assert ids2.tolist() == ids.tolist() and score2.view(np.uint32) == score.view(np.uint32)
